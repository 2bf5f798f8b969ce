// Shared stage 0 of the sliding window (sw_share_plan.hip): the tile tensors gathered from the whole-volume and slab results of encoder
// stage 0 - by volume row, by output box or the shells alone -, the stage-0 view of a tile into a whole-volume tensor and the mask
// that zeroes a whole-volume tensor outside the padded volume.  fp32 NDHWC, 16 B per lane.
#include "kernels.h"

#include <algorithm>

namespace mi355 {

// ------------------------------------------------------------------ shared stage 0: tile tensor from whole-volume + slab results
// One workgroup = one (z, y) row of one whole-volume result: the row is read ONCE and written to every sample (tile) of that result
// that holds it - walking the tiles instead re-read each volume row from HBM once per tile, 4.7 times per voxel at step 0.5.  Whether
// a tile's row lies in a z or y shell is workgroup-uniform (the whole row then comes from that slab), the x shells are decided per
// voxel.  Four 16-byte loads in flight per lane before the first store.
// One tensor of the gather: the sources, the destination, the shell depth and the channel quads per voxel.
struct S0GatherSet {
    const float *wv, *slab[3];
    float *out;
    int r, C4;
};
// voxel (v0, v1, v2) of slab `idx` of axis ax, given the tile voxel (z, y, x) and the face's side: along ax the slab's own layer
// (a hi slab covers the last t[ax] layers of the tile), across it the tile voxel plus the tile's origin inside the slab
static __device__ __forceinline__ int64_t s0_slab_voxel(const S0GatherArgs &a, const S0Sample &sm, const int *sub, int ax, int side, int idx, int z, int y, int x) {
    int v[3] = {z, y, x};
    if (side) v[ax] -= a.P[ax] - a.t[ax];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += a.so[ax][k] ? sm.org[k] : (k != ax ? sub[k] : 0);
    return (((int64_t)idx * a.D[ax][0] + v[0]) * a.D[ax][1] + v[1]) * a.D[ax][2] + v[2];
}

// where voxel (z, y, x) of sample n comes from (as a pointer to its first channel quad): the first shell that holds it, z before y
// before x, else the whole-volume tensor - stage0_gather_row's sources and precedence, per voxel
static __device__ __forceinline__ const f32x4 *s0_voxel_source(const S0GatherArgs &a, const S0GatherSet &t, int n, int z, int y, int x) {
    const S0Sample &sm = a.smp[n];
    const int r = t.r;
    const int64_t C4 = t.C4;
    if (sm.slab[0] >= 0 && z < r) return (const f32x4 *)t.slab[0] + s0_slab_voxel(a, sm, a.sub[n], 0, 0, sm.slab[0], z, y, x) * C4;
    if (sm.slab[1] >= 0 && z >= a.P[0] - r) return (const f32x4 *)t.slab[0] + s0_slab_voxel(a, sm, a.sub[n], 0, 1, sm.slab[1], z, y, x) * C4;
    if (sm.slab[2] >= 0 && y < r) return (const f32x4 *)t.slab[1] + s0_slab_voxel(a, sm, a.sub[n], 1, 0, sm.slab[2], z, y, x) * C4;
    if (sm.slab[3] >= 0 && y >= a.P[1] - r) return (const f32x4 *)t.slab[1] + s0_slab_voxel(a, sm, a.sub[n], 1, 1, sm.slab[3], z, y, x) * C4;
    if (sm.slab[4] >= 0 && x < r) return (const f32x4 *)t.slab[2] + s0_slab_voxel(a, sm, a.sub[n], 2, 0, sm.slab[4], z, y, x) * C4;
    if (sm.slab[5] >= 0 && x >= a.P[2] - r) return (const f32x4 *)t.slab[2] + s0_slab_voxel(a, sm, a.sub[n], 2, 1, sm.slab[5], z, y, x) * C4;
    return (const f32x4 *)t.wv + ((((int64_t)sm.wv * a.Ve[0] + sm.org[0] + z) * a.Ve[1] + sm.org[1] + y) * a.Ve[2] + sm.org[2] + x) * C4;
}

static __device__ __forceinline__ void stage0_gather_row(const S0GatherArgs &a, const S0GatherSet &t, int m, int Z, int Y) {
    const int r = t.r, C4 = t.C4;
    const f32x4 *wrow = (const f32x4 *)t.wv + (((int64_t)m * a.Ve[0] + Z) * a.Ve[1] + Y) * a.Ve[2] * C4;
    const int volq = a.Ve[2] * C4, rowq = a.P[2] * C4;
    constexpr int U = 4;
    for (int q0 = threadIdx.x; q0 < volq; q0 += U * 256) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (q0 + u * 256 < volq) v[u] = wrow[q0 + u * 256];
        for (int n = 0; n < a.n; ++n) {
            const S0Sample &sm = a.smp[n];
            const int z = Z - sm.org[0], y = Y - sm.org[1];
            if (sm.wv != m || (unsigned)z >= (unsigned)a.P[0] || (unsigned)y >= (unsigned)a.P[1]) continue;
            // the row's source when a z or y shell holds it: slab base (in quads) of voxel x = 0
            const f32x4 *row = nullptr;
            if (sm.slab[0] >= 0 && z < r)
                row = (const f32x4 *)t.slab[0] + s0_slab_voxel(a, sm, a.sub[n], 0, 0, sm.slab[0], z, y, 0) * C4;
            else if (sm.slab[1] >= 0 && z >= a.P[0] - r)
                row = (const f32x4 *)t.slab[0] + s0_slab_voxel(a, sm, a.sub[n], 0, 1, sm.slab[1], z, y, 0) * C4;
            else if (sm.slab[2] >= 0 && y < r)
                row = (const f32x4 *)t.slab[1] + s0_slab_voxel(a, sm, a.sub[n], 1, 0, sm.slab[2], z, y, 0) * C4;
            else if (sm.slab[3] >= 0 && y >= a.P[1] - r)
                row = (const f32x4 *)t.slab[1] + s0_slab_voxel(a, sm, a.sub[n], 1, 1, sm.slab[3], z, y, 0) * C4;
            // (the x slabs: base of the slab's voxel that holds tile voxel x = 0, lo, and x = P2 - t2, hi)
            const f32x4 *xlo = sm.slab[4] < 0 ? nullptr : (const f32x4 *)t.slab[2] + s0_slab_voxel(a, sm, a.sub[n], 2, 0, sm.slab[4], z, y, 0) * C4;
            const f32x4 *xhi = sm.slab[5] < 0 ? nullptr : (const f32x4 *)t.slab[2] + s0_slab_voxel(a, sm, a.sub[n], 2, 1, sm.slab[5], z, y, a.P[2] - a.t[2]) * C4;
            f32x4 *dst = (f32x4 *)t.out + (((int64_t)n * a.P[0] + z) * a.P[1] + y) * rowq;
            const int qorg = sm.org[2] * C4;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = q0 + u * 256 - qorg;  // quad of the tile's row
                if (q0 + u * 256 >= volq || (unsigned)q >= (unsigned)rowq) continue;
                const int x = q / C4;
                f32x4 val = v[u];
                if (row) val = row[q];
                else if (xlo && x < r) val = xlo[q];
                else if (xhi && x >= a.P[2] - r) val = xhi[q - (a.P[2] - a.t[2]) * C4];
                dst[q] = val;
            }
        }
    }
}

// A second tensor may ride along (the shared skip half of the last decoder stage's concat conv, sliding_window.hip): same samples, same
// slab indices, its own sources, channel count and shell depth.
__global__ __launch_bounds__(256) void stage0_gather_kernel(S0GatherArgs a) {
    const int m = blockIdx.y;
    const int Z = (int)blockIdx.x / a.Ve[1], Y = (int)blockIdx.x - Z * a.Ve[1];
    const S0GatherSet t0 = {a.wv, {a.slab[0], a.slab[1], a.slab[2]}, a.out, a.r, a.C4};
    stage0_gather_row(a, t0, m, Z, Y);
    if (a.out2) {
        const S0GatherSet t1 = {a.wv2, {a.slab2[0], a.slab2[1], a.slab2[2]}, a.out2, a.r2, a.C42};
        stage0_gather_row(a, t1, m, Z, Y);
    }
}

// The same gather with the grid over what is WRITTEN (by_box; the sub-boxes of the shared level 1): the n output boxes are one
// contiguous run of (sample, z, y) rows of P2 * C4 quads; a workgroup takes `rows_per_wg` consecutive rows, a lane one 16-byte piece
// at a time, four loads in flight before the first store.  The row form above walks every row of the whole volume and, per row, every
// sample: right for tiles that cover the volume several times over, but for thin sub-boxes most of its 256-lane workgroups find
// a 16-voxel piece or nothing.  Sources and precedence per voxel are the row form's (s0_voxel_source): bit-identical.
__global__ __launch_bounds__(256) void stage0_gather_box_kernel(S0GatherArgs a, int rows_per_wg) {
    const S0GatherSet t = {a.wv, {a.slab[0], a.slab[1], a.slab[2]}, a.out, a.r, a.C4};
    const unsigned C4 = (unsigned)t.C4, rowq = (unsigned)a.P[2] * C4, plane = (unsigned)a.P[0] * (unsigned)a.P[1];
    const unsigned rows = (unsigned)a.n * plane;  // (host: rows * rowq < 2^31)
    const unsigned row0 = blockIdx.x * (unsigned)rows_per_wg;
    const unsigned nrow = rows - row0 < (unsigned)rows_per_wg ? rows - row0 : (unsigned)rows_per_wg;
    const unsigned chunk = nrow * rowq;
    f32x4 *dst = (f32x4 *)t.out + (int64_t)row0 * rowq;
    constexpr int U = 4;
    for (unsigned j0 = threadIdx.x; j0 < chunk; j0 += U * 256) {
        const f32x4 *src[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned j = j0 + u * 256;
            if (j >= chunk) continue;
            const unsigned rr = j / rowq, q = j - rr * rowq, row = row0 + rr;
            const unsigned n = row / plane, zy = row - n * plane;
            const unsigned z = zy / (unsigned)a.P[1], y = zy - z * (unsigned)a.P[1];
            const unsigned x = q / C4, c4 = q - x * C4;
            src[u] = s0_voxel_source(a, t, (int)n, (int)z, (int)y, (int)x) + c4;
        }
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (j0 + u * 256 < chunk) v[u] = *src[u];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (j0 + u * 256 < chunk) dst[j0 + u * 256] = v[u];
    }
}

static int stage0_gather_check(const S0GatherArgs &a, int n_samples, int *n_wv);
static_assert(sizeof(S0GatherArgs) + sizeof(int) <= 4096, "the gather's arguments must fit the kernel-argument block");
int stage0_gather(const S0GatherArgs &a, int n_samples, hipStream_t s, bool by_box) {
    int n_wv = 0;
    MI355_TRY(stage0_gather_check(a, n_samples, &n_wv));
    const int64_t rowq = (int64_t)a.P[2] * a.C4, rows = (int64_t)n_samples * a.P[0] * a.P[1];
    if (by_box && !a.out2 && rows * rowq < (1ll << 31)) {  // (one tensor; a larger gather stays with the row form)
        S0GatherArgs k = a;
        k.n = n_samples;
        const int rows_per_wg = (int)std::max<int64_t>(1, (4 * 256 + rowq - 1) / rowq);  // about one pass of the unrolled loop
        hipLaunchKernelGGL(stage0_gather_box_kernel, dim3((unsigned)((rows + rows_per_wg - 1) / rows_per_wg)), dim3(256), 0, s, k, rows_per_wg);
        MI355_HIP(hipGetLastError());
        return MI355_OK;
    }
    MI355_REQUIRE((int64_t)a.Ve[0] * a.Ve[1] < (1ll << 31), "stage0_gather: grid too large");
    S0GatherArgs k = a;
    k.n = n_samples;
    hipLaunchKernelGGL(stage0_gather_kernel, dim3((unsigned)(a.Ve[0] * a.Ve[1]), (unsigned)n_wv), dim3(256), 0, s, k);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// ---- the same for a tensor whose reader takes a stage-0 view (kernels.h S0View): the shells alone.  Per sample the shell voxels are
// enumerated as three boxes - A: the planes within r of a z face that has a slab, whole; B: of the other planes the rows within r
// of such a y face; C: of the other rows the voxels within r of such an x face - so the grid covers what is written and nothing
// else, and consecutive lanes write consecutive 16-byte pieces.  Sources and precedence are stage0_gather_row's.
struct S0ShellDims {
    int lo[3], hi[3];   // axis a: [0, lo) and [hi, P) lie in a shell
    unsigned nA, nB, nC;  // voxels per box
};
static __host__ __device__ inline S0ShellDims s0_shell_dims(const int P[3], int r, const int faces[6]) {
    S0ShellDims d;
    for (int a = 0; a < 3; ++a) { d.lo[a] = faces[2 * a] >= 0 ? r : 0; d.hi[a] = faces[2 * a + 1] >= 0 ? P[a] - r : P[a]; }
    const unsigned nz = (unsigned)(d.lo[0] + P[0] - d.hi[0]), ny = (unsigned)(d.lo[1] + P[1] - d.hi[1]), nx = (unsigned)(d.lo[2] + P[2] - d.hi[2]);
    d.nA = nz * (unsigned)P[1] * (unsigned)P[2];
    d.nB = ((unsigned)P[0] - nz) * ny * (unsigned)P[2];
    d.nC = ((unsigned)P[0] - nz) * ((unsigned)P[1] - ny) * nx;
    return d;
}
int64_t stage0_shell_voxels(const int P[3], int r, const int faces[6]) {
    const S0ShellDims d = s0_shell_dims(P, r, faces);
    return (int64_t)d.nA + d.nB + d.nC;
}

__global__ __launch_bounds__(256) void stage0_gather_shell_kernel(S0GatherArgs a, int which) {
    const S0GatherSet t = which ? S0GatherSet{a.wv2, {a.slab2[0], a.slab2[1], a.slab2[2]}, a.out2, a.r2, a.C42}
                                : S0GatherSet{a.wv, {a.slab[0], a.slab[1], a.slab[2]}, a.out, a.r, a.C4};
    const int n = blockIdx.y, r = t.r;
    const unsigned C4 = (unsigned)t.C4;
    const S0Sample &sm = a.smp[n];
    const S0ShellDims d = s0_shell_dims(a.P, r, sm.slab);
    const unsigned i = blockIdx.x * 256u + threadIdx.x;   // (host: voxels of a tile * C4 < 2^31)
    if (i >= (d.nA + d.nB + d.nC) * C4) return;
    unsigned w = i / C4;
    const unsigned c4 = i - w * C4;
    auto shell_at = [](unsigned k, int lo, int hi) { return (int)k < lo ? (int)k : hi + ((int)k - lo); };  // k-th shell plane of an axis
    int z, y, x;
    if (w < d.nA) {
        const unsigned plane = (unsigned)a.P[1] * (unsigned)a.P[2];
        const unsigned kz = w / plane; w -= kz * plane;
        z = shell_at(kz, d.lo[0], d.hi[0]);
        y = (int)(w / (unsigned)a.P[2]); x = (int)(w - (unsigned)y * (unsigned)a.P[2]);
    } else if (w < d.nA + d.nB) {
        w -= d.nA;
        const unsigned ny = (unsigned)(d.lo[1] + a.P[1] - d.hi[1]), plane = ny * (unsigned)a.P[2];
        const unsigned kz = w / plane; w -= kz * plane;
        z = d.lo[0] + (int)kz;
        const unsigned ky = w / (unsigned)a.P[2];
        y = shell_at(ky, d.lo[1], d.hi[1]); x = (int)(w - ky * (unsigned)a.P[2]);
    } else {
        w -= d.nA + d.nB;
        const unsigned ny = (unsigned)(d.lo[1] + a.P[1] - d.hi[1]), nx = (unsigned)(d.lo[2] + a.P[2] - d.hi[2]);
        const unsigned plane = ((unsigned)a.P[1] - ny) * nx;
        const unsigned kz = w / plane; w -= kz * plane;
        z = d.lo[0] + (int)kz;
        const unsigned ky = w / nx;
        y = d.lo[1] + (int)ky; x = shell_at(w - ky * nx, d.lo[2], d.hi[2]);
    }
    const f32x4 *src = s0_voxel_source(a, t, n, z, y, x);  // (every enumerated voxel lies in a shell: never the whole-volume tensor)
    ((f32x4 *)t.out)[((((int64_t)n * a.P[0] + z) * a.P[1] + y) * a.P[2] + x) * C4 + c4] = src[c4];
}

static int stage0_gather_check(const S0GatherArgs &a, int n_samples, int *n_wv) {
    MI355_REQUIRE(n_samples > 0 && n_samples <= S0_MAX_SAMPLES, "stage0_gather: %d samples (max %d)", n_samples, S0_MAX_SAMPLES);
    MI355_REQUIRE(a.C4 > 0 && a.r > 0, "stage0_gather: bad channel count / shell depth");
    MI355_REQUIRE(!a.out2 || (a.wv2 && a.C42 > 0 && a.r2 >= a.r), "stage0_gather: bad second tensor");
    const int rmax = a.out2 ? a.r2 : a.r;
    for (int k = 0; k < 3; ++k)
        MI355_REQUIRE(a.t[k] >= 2 * rmax && a.P[k] >= a.t[k] && a.Ve[k] >= a.P[k], "stage0_gather: axis %d: patch %d, slab %d, volume %d, r %d", k, a.P[k], a.t[k], a.Ve[k], rmax);
    for (int i = 0; i < n_samples; ++i)
        for (int k = 0; k < 3; ++k)
            MI355_REQUIRE(a.smp[i].org[k] >= 0 && a.smp[i].org[k] + a.P[k] <= a.Ve[k], "stage0_gather: sample %d leaves the volume", i);
    // a slab holds every tile voxel that is read from it: its own thickness along its axis; across it the tile's extent with the
    // tile at 0, or the volume's with the tile at its origin (inside the volume, above)
    // sub-boxes: a sample lies inside its tile, and a face of it that takes a shell is a face of the tile - a slab holds the t
    // outermost layers of the TILE, which s0_slab_voxel addresses from the sample's own face; without sub-boxes every offset is zero
    const bool boxes = a.T[0] > 0;
    for (int i = 0; i < n_samples; ++i)
        for (int k = 0; k < 3; ++k) {
            MI355_REQUIRE(boxes ? a.sub[i][k] >= 0 && a.sub[i][k] + a.P[k] <= a.T[k] && a.sub[i][k] <= a.smp[i].org[k] : (a.T[k] == 0 && a.sub[i][k] == 0),
                          "stage0_gather: sample %d: sub-box offset %d on axis %d (tile %d)", i, a.sub[i][k], k, a.T[k]);
            MI355_REQUIRE(!boxes || ((a.smp[i].slab[2 * k] < 0 || a.sub[i][k] == 0) && (a.smp[i].slab[2 * k + 1] < 0 || a.sub[i][k] + a.P[k] == a.T[k])),
                          "stage0_gather: sample %d: a shell at a face on axis %d that is not the tile's (offset %d, extent %d of %d)", i, k, a.sub[i][k], a.P[k], a.T[k]);
        }
    for (int ax = 0; ax < 3; ++ax)
        for (int k = 0; k < 3; ++k) {
            const int want = k == ax ? a.t[k] : (a.so[ax][k] ? a.Ve[k] : (boxes ? a.T[k] : a.P[k]));
            MI355_REQUIRE((a.so[ax][k] == 0 || (a.so[ax][k] == 1 && k != ax)) && a.D[ax][k] == want,
                          "stage0_gather: slab of axis %d: extent %d along %d (expected %d)", ax, a.D[ax][k], k, want);
        }
    *n_wv = 0;
    for (int i = 0; i < n_samples; ++i) {
        MI355_REQUIRE(a.smp[i].wv >= 0 && a.smp[i].wv < 65535, "stage0_gather: sample %d: whole-volume index %d", i, a.smp[i].wv);
        *n_wv = a.smp[i].wv + 1 > *n_wv ? a.smp[i].wv + 1 : *n_wv;
    }
    return MI355_OK;
}

int stage0_gather_shells(const S0GatherArgs &a, int n_samples, int which, hipStream_t s) {
    int n_wv = 0;
    MI355_TRY(stage0_gather_check(a, n_samples, &n_wv));
    MI355_REQUIRE(which == 0 || (which == 1 && a.out2), "stage0_gather_shells: tensor %d", which);
    const int C4 = which ? a.C42 : a.C4, r = which ? a.r2 : a.r;
    MI355_REQUIRE((int64_t)a.P[0] * a.P[1] * a.P[2] * C4 < (1ll << 31), "stage0_gather_shells: tile too large");
    int64_t most = 0;
    for (int i = 0; i < n_samples; ++i) most = std::max(most, stage0_shell_voxels(a.P, r, a.smp[i].slab));
    if (most == 0) return MI355_OK;  // no sample has a face inside the volume
    S0GatherArgs k = a;
    k.n = n_samples;
    hipLaunchKernelGGL(stage0_gather_shell_kernel, dim3((unsigned)((most * C4 + 255) / 256), (unsigned)n_samples), dim3(256), 0, s, k, which);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// The view of n samples into a whole-volume tensor (kernels.h): pure host code.
int stage0_view_make(const float *src, int n_wv, const int Ve[3], const int P[3], int C, int depth, const S0Sample *smp, int n, S0View *out) {
    *out = S0View();
    MI355_REQUIRE(src && n_wv > 0 && C > 0 && depth > 0 && smp, "stage-0 view: bad argument");
    MI355_REQUIRE(n > 0 && n <= S0_VIEW_MAX_SAMPLES, "stage-0 view: %d samples (max %d)", n, S0_VIEW_MAX_SAMPLES);
    for (int k = 0; k < 3; ++k) MI355_REQUIRE(P[k] > 0 && Ve[k] >= P[k] && 2 * depth <= P[k], "stage-0 view: axis %d: tile %d, volume %d, shell %d", k, P[k], Ve[k], depth);
    // what a reader forms in 32 bits: a sample's origin as a voxel index (unsigned), and per lane the element offset of a piece from
    // its brick's or tile's corner - at most 5 planes + 9 rows + 65 voxels (stride-2 brick), 2 rows + 8 voxels (addend)
    MI355_REQUIRE((int64_t)n_wv * Ve[0] * Ve[1] * Ve[2] < (1ll << 32) && 8ll * Ve[1] * Ve[2] * C < (1ll << 31),
                  "stage-0 view: a tensor of %d x %d x %d x %d voxels x %d channels exceeds the 32-bit offsets", n_wv, Ve[0], Ve[1], Ve[2], C);
    S0View v;
    for (int i = 0; i < n; ++i) {
        MI355_REQUIRE(smp[i].wv >= 0 && smp[i].wv < n_wv, "stage-0 view: sample %d: whole-volume index %d of %d", i, smp[i].wv, n_wv);
        for (int k = 0; k < 3; ++k)
            MI355_REQUIRE(smp[i].org[k] >= 0 && smp[i].org[k] + P[k] <= Ve[k], "stage-0 view: sample %d leaves its tensor on axis %d (%d + %d > %d)", i, k, smp[i].org[k], P[k], Ve[k]);
        v.smp[i].off = (unsigned)((((int64_t)smp[i].wv * Ve[0] + smp[i].org[0]) * Ve[1] + smp[i].org[1]) * Ve[2] + smp[i].org[2]);
        v.smp[i].faces = 0;
        for (int f = 0; f < 6; ++f) v.smp[i].faces |= smp[i].slab[f] >= 0 ? 1u << f : 0u;
    }
    for (int i = n; i < S0_VIEW_MAX_SAMPLES; ++i) v.smp[i] = v.smp[0];  // (never indexed; a defined value all the same)
    v.src = src; v.sy = Ve[2]; v.sz = Ve[1] * Ve[2]; v.depth = depth;
    *out = v;
    return MI355_OK;
}

// Zero outside [0, Zp): the voxels are enumerated as three boxes, z >= Zp0 | z < Zp0, y >= Zp1 | z < Zp0, y < Zp1, x >= Zp2.
__global__ void stage0_mask_kernel(f32x4 *x, int Ve0, int Ve1, int Ve2, int Zp0, int Zp1, int Zp2, int C4, int64_t nA, int64_t nB, int64_t nC) {
    const int64_t total = (nA + nB + nC) * C4;
    f32x4 *xn = x + (int64_t)blockIdx.y * Ve0 * Ve1 * Ve2 * C4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t w = i / C4;
        const int c4 = (int)(i - w * C4);
        int vz, vy, vx;
        if (w < nA) {
            vz = Zp0 + (int)(w / ((int64_t)Ve1 * Ve2)); w %= (int64_t)Ve1 * Ve2;
            vy = (int)(w / Ve2); vx = (int)(w % Ve2);
        } else if (w < nA + nB) {
            w -= nA;
            const int64_t plane = (int64_t)(Ve1 - Zp1) * Ve2;
            vz = (int)(w / plane); w %= plane;
            vy = Zp1 + (int)(w / Ve2); vx = (int)(w % Ve2);
        } else {
            w -= nA + nB;
            const int64_t plane = (int64_t)Zp1 * (Ve2 - Zp2);
            vz = (int)(w / plane); w %= plane;
            vy = (int)(w / (Ve2 - Zp2)); vx = Zp2 + (int)(w % (Ve2 - Zp2));
        }
        xn[(((int64_t)vz * Ve1 + vy) * Ve2 + vx) * C4 + c4] = zero;
    }
}

int stage0_mask(float *x, int N, const int Ve[3], const int Zp[3], int C, hipStream_t s) {
    MI355_REQUIRE(C % 4 == 0 && N > 0 && N <= 65535, "stage0_mask: C = %d, N = %d", C, N);
    for (int k = 0; k < 3; ++k) MI355_REQUIRE(Zp[k] > 0 && Zp[k] <= Ve[k], "stage0_mask: axis %d: %d of %d", k, Zp[k], Ve[k]);
    const int64_t nA = (int64_t)(Ve[0] - Zp[0]) * Ve[1] * Ve[2], nB = (int64_t)Zp[0] * (Ve[1] - Zp[1]) * Ve[2],
                  nC = (int64_t)Zp[0] * Zp[1] * (Ve[2] - Zp[2]);
    const int64_t total = (nA + nB + nC) * (C / 4);
    if (total == 0) return MI355_OK;
    int64_t bx = (total + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(stage0_mask_kernel, dim3((unsigned)bx, (unsigned)N), dim3(256), 0, s, (f32x4 *)x, Ve[0], Ve[1], Ve[2], Zp[0], Zp[1],
                       Zp[2], C / 4, nA, nB, nC);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

}  // namespace mi355
