// Host-side pieces the conv dispatchers share: the A/B switches, tile geometry, the persistent-grid rule, the table row of a
// kernel instantiation and the plan a dispatcher computes before it launches anything (plan_conv_f32 / plan_conv_f16).
#pragma once
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "kernels.h"

namespace mi355 {

// A/B switch MI355_X: "0" = off, anything else (default) = on.  Read once per process.
inline bool env_switch(const char *name) {
    static std::mutex mu;
    static std::map<std::string, bool> seen;
    std::lock_guard<std::mutex> lk(mu);
    auto it = seen.find(name);
    if (it == seen.end()) {
        const char *e = getenv(name);
        it = seen.emplace(name, !(e && e[0] == '0')).first;
    }
    return it->second;
}
// MI355_CONV_IMPL: 0 = always the one-tile-per-workgroup kernels, 1 = always the pipelined persistent kernel, 2 = auto (default;
// conv3d.hip "host side" has the measurements).  The fp16 path knows two settings: 0, and everything else.
inline int conv_impl() {
    static const int v = [] { const char *e = getenv("MI355_CONV_IMPL"); return !e ? 2 : (e[0] == '0' ? 0 : (e[0] == '1' ? 1 : 2)); }();
    return v;
}

// Output tile (log2 dims), its grid over the volume and the input halo brick.
struct TileGeom {
    int lx = 0, ly = 0, lz = 0;
    int tiles_x = 0, tiles_y = 0, tiles_z = 0;
    int IX = 0, IY = 0, IZ = 0;
    long tiles_per_n() const { return (long)tiles_x * tiles_y * tiles_z; }
    int brickvox() const { return IX * IY * IZ; }
    bool whole(int Do, int Ho, int Wo) const { return Do % (1 << lz) == 0 && Ho % (1 << ly) == 0 && Wo % (1 << lx) == 0; }
};

// Output tile (power-of-two dims, 128*MF voxels): x as long as the volume allows (up to 32:
// x-consecutive lanes are the conflict-free LDS pattern and give the longest contiguous global
// rows), then the (y, z) split with the smallest input brick.
inline void choose_tile(int Do, int Ho, int Wo, int stride, int voxels, int *lz, int *ly, int *lx) {
    auto p2cap = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };
    const int cz = p2cap(Do), cy = p2cap(Ho), cx = p2cap(Wo);
    const int L = ilog2_exact(voxels);
    int x = cx < 5 ? cx : 5;
    if (x > L) x = L;
    long best = -1;
    int bz = L - x, by = 0;
    for (int y = 0; x + y <= L; ++y) {
        const int z = L - x - y;
        const int oy = y > cy ? y - cy : 0, oz = z > cz ? z - cz : 0;  // lanes wasted past the volume
        const long brick = (long)(((1 << y) - 1) * stride + 3) * (((1 << z) - 1) * stride + 3);
        const long cost = ((long)(oy + oz) << 32) + brick;
        if (best < 0 || cost < best) {
            best = cost; bz = z; by = y;
        }
    }
    *lz = bz; *ly = by; *lx = x;
}
// a fixed tile of 2^lz x 2^ly x 2^lx output voxels over an IZ x IY x IX brick
inline TileGeom fixed_tile(int Do, int Ho, int Wo, int lz, int ly, int lx, int IZ, int IY, int IX) {
    TileGeom g;
    g.lz = lz; g.ly = ly; g.lx = lx;
    g.tiles_x = ceil_div(Wo, 1 << lx); g.tiles_y = ceil_div(Ho, 1 << ly); g.tiles_z = ceil_div(Do, 1 << lz);
    g.IX = IX; g.IY = IY; g.IZ = IZ;
    return g;
}
// the chosen tile of `voxels` output voxels of a 3x3x3 conv of stride `st`
inline TileGeom chosen_tile(int Do, int Ho, int Wo, int st, int voxels) {
    int lz, ly, lx;
    choose_tile(Do, Ho, Wo, st, voxels, &lz, &ly, &lx);
    return fixed_tile(Do, Ho, Wo, lz, ly, lx, ((1 << lz) - 1) * st + 3, ((1 << ly) - 1) * st + 3, ((1 << lx) - 1) * st + 3);
}
// geometry fields of a kernel argument struct (ConvArgs, ConvArgsH)
template <typename Args>
inline void set_geometry(Args &a, const TileGeom &g) {
    a.lx = g.lx; a.ly = g.ly; a.lz = g.lz;
    a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y; a.tiles_z = g.tiles_z;
    a.IX = g.IX; a.IY = g.IY; a.IZ = g.IZ;
    a.div_tiles_per_n = make_fastdiv(g.tiles_x * g.tiles_y * g.tiles_z);
    a.div_tiles_x = make_fastdiv(g.tiles_x);
    a.div_tiles_y = make_fastdiv(g.tiles_y);
    a.div_IX = make_fastdiv(g.IX);
    a.div_IY = make_fastdiv(g.IY);
}

// grid.x of a persistent kernel: `workgroups` resident on the chip in total, shared by the gy cout blocks; a multiple of 8
// (blockIdx.x & 7 labels the XCD group) and no more than the tiles need
inline int persistent_grid_x(int workgroups, int gy, long tiles) {
    int gx = workgroups / gy;
    gx = gx < 8 ? 8 : (gx / 8) * 8;
    const int need = (int)((tiles + 7) / 8) * 8;
    return gx > need ? need : gx;
}

// One launched instantiation: its function, its name as rocprofv3 prints it (what bench.py, the profiles and the tests key on)
// and the dynamic-LDS limit raised for it so far (one process per GPU).
struct KernelRow {
    const void *fn;
    const char *name, *name_splitk;
    size_t lds_limit;
};
#define MI355_KERNEL_ROW(...) {(const void *)&__VA_ARGS__, #__VA_ARGS__, #__VA_ARGS__ " split-K", 48 * 1024}
// the row whose name is the printf-style `fmt`, or null: the planners spell an instantiation by its template arguments
template <size_t N>
inline KernelRow *find_row(KernelRow (&rows)[N], const char *fmt, ...) {
    char name[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
    for (KernelRow &r : rows)
        if (strcmp(r.name, name) == 0) return &r;
    return nullptr;
}
// `table | name` lines of a table's rows, and the four tables' own listings (mi355_conv_kernel_names): what ships, whether or not
// a planner ever selects it
template <size_t N>
inline void list_rows(const char *table, KernelRow (&rows)[N], std::string *out) {
    for (KernelRow &r : rows) *out += std::string(table) + " | " + r.name + "\n";
}
void list_f32_rows(std::string *out);    // conv3d.hip
void list_wino3_rows(std::string *out);  // conv3d_wino3.hip
void list_f16_rows(std::string *out);    // conv3d_f16.hip
void list_s2h_rows(std::string *out);    // conv3d_f16_s2.hip
inline const char *tf(bool b) { return b ? "true" : "false"; }
// launch `r` with 256 threads per workgroup; `args` = the kernel's one argument struct
inline int launch_row(KernelRow &r, dim3 grid, size_t lds_bytes, hipStream_t s, void *args) {
    if (lds_bytes > r.lds_limit) {
        MI355_HIP(hipFuncSetAttribute(r.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        r.lds_limit = lds_bytes;
    }
    void *argv[1] = {args};
    MI355_HIP(hipLaunchKernel(r.fn, grid, dim3(256), argv, lds_bytes, s));
    return MI355_OK;
}

// What a dispatcher decided for one call; plain data, computed without touching the device.
enum ConvFamily { FAM_SIMPLE, FAM_PIPE, FAM_WINO2, FAM_WINO3, FAM_S2DMA, FAM_DMA };
enum ConvPack { PACK_MAIN, PACK_C16, PACK_WINO2, PACK_WINO3 };
struct ConvPlan {
    KernelRow *row = nullptr;
    const char *name = nullptr;  // row->name, or row->name_splitk
    int family = FAM_SIMPLE;
    int pack = PACK_MAIN;        // which weight pack of the layer the kernel reads
    int nf = 1;                  // 32-cout fragments per workgroup
    TileGeom g;
    long tiles = 0;              // over all samples
    unsigned gx = 0, gy = 1, gz = 1;
    size_t lds_bytes = 0;
    int ksplit = 1;              // split-K slices (1 = none)
};
inline void plan_set(ConvPlan *p, KernelRow *row, int family, const TileGeom &g, long tiles, unsigned gx, unsigned gy, size_t lds_bytes) {
    p->row = row; p->name = row->name; p->family = family; p->g = g; p->tiles = tiles;
    p->gx = gx; p->gy = gy; p->gz = 1; p->lds_bytes = lds_bytes; p->ksplit = 1;
}

// Split-K of the one-tile-per-workgroup kernels (both dtypes).  Small launches (deep levels: few voxels, hundreds of channels)
// leave most CUs idle and run one long serial chain of chunks per workgroup: the channel chunks are split over blockIdx.z, raw
// partial sums are written and a finishing pass adds them in slice order (deterministic).  As many slices as still fit the chip
// in ONE round of workgroups (256 CUs x 2): rounding up (round 2) gave the 8^3 level 80 x 7 = 560 workgroups - 48 of them ran
// behind the other 512 and doubled the launch's critical path.  Returns the slice count, or 0 for no split.
inline int splitk_slices(long units, int nchunks) {
    int S = (int)(512 / units);
    if (S > nchunks / 4) S = nchunks / 4;
    if (S > 8) S = 8;
    return (units < 256 && S >= 2) ? S : 0;
}

int plan_conv_f32(const ConvWeights &w, const ConvCall &c, ConvPlan *p);
int plan_conv_f16(const ConvWeightsH &w, const ConvCallH &c, ConvPlan *p);
// steps of the planners that live beside their kernels: true = the call fits and *p is its plan
bool plan_wino3(const ConvWeights &w, const ConvCall &c, ConvPlan *p, bool force = false);  // conv3d_wino3.hip
bool plan_s2dma(const ConvWeights &w, const ConvCall &c, ConvPlan *p, bool force = false);  // conv3d.hip
bool plan_f16_s2dma(const ConvWeightsH &w, const ConvCallH &c, ConvPlan *p);  // conv3d_f16_s2.hip
int launch_wino3(const ConvWeights &w, const ConvCall &c, const ConvPlan &p, hipStream_t s);
int launch_f16_s2dma(const ConvWeightsH &w, const ConvCallH &c, const ConvPlan &p, hipStream_t s);

// The transposed conv's plan for M = N*D*H*W input voxels (tconv.hip): a row of tconv_rows, its grid and its static LDS; or
// the refusal of a shape the kernels do not take.  tconv2_mfma is plan_tconv + launch_tconv.
struct TconvPlan {
    KernelRow *row = nullptr;
    bool persistent = false;  // version 3: grid.x workgroups stride over the voxel tiles
    unsigned gx = 0, gy = 1;
    size_t lds_bytes = 0;
};
int plan_tconv(int dtype, int cin, int cout, long M, TconvPlan *p);
int launch_tconv(const TConvWeights &w, const TconvPlan &p, const void *in, int N, int D, int H, int W, void *out, hipStream_t s);

}  // namespace mi355
