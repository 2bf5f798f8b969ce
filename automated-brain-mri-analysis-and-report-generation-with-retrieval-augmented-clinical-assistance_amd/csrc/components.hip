// Connected components of a binary volume on the device: what feature_extraction/step3_multiplicity.py
// gets from scipy.ndimage.label (:58-59, :222-223) and then derives per component with one whole-volume comparison each
// (:63-121, :227-242), and what nnU-Net v1's remove_all_but_the_largest_connected_component needs.
//
// Labelling = label equivalence with union-find.  parent[i] is a LINEAR VOXEL INDEX (int32, -1 = background) and every
// link goes from the larger index to the smaller, so parent[i] <= i at all times: every pointer chase strictly decreases
// and ends, whatever other threads do meanwhile, and the root of a finished tree is the component's first voxel in raster
// order - which is how scipy numbers components, so ranking the roots by index gives scipy's labels.
//
//   1 local    a workgroup labels one 4 x 8 x 64 brick in LDS (union over the backward half of the neighbourhood: 3 of 6,
//              9 of 18, 13 of 26) and writes the GLOBAL index of every voxel's brick-local root; it writes inside its brick only
//   2 seam     threads over the voxels with a backward neighbour in another brick unite the two trees in the global array
//   3 flatten  parent[i] = root(i), and the number of roots (parent[i] == i) per 2048-voxel chunk
//   4 scan     exclusive prefix sum of the chunk counts (one workgroup), total = number of components
//   5 rank     labels[root] = 1 + number of roots before it; background = 0
//   6 relabel  labels[i] = labels[parent[i]] for the other foreground voxels
//
// No workgroup ever waits for another: no flags, no spin loops, no grid barrier; the launch boundaries are the only
// ordering between the passes.  In the seam and flatten passes the parent array is shared between workgroups while it
// changes: every read of it is a relaxed agent-scope atomic load and every write an atomic.  A stale parent is still an
// ancestor in the same tree (links are only ever added at roots, and flattening replaces a parent by an ancestor of it),
// and the returning atomicMin of a link carries the truth: if the word had already moved, the loop continues from the value
// it returns.  Staleness costs iterations, not correctness.
//
// Statistics: one pass over the label map, all integers, so the table does not depend on arrival order.  A lane keeps the
// running totals of the component it is in and lets go of them only when it meets another one; at the end of a wave's range
// the lanes that hold the same component are reduced with a butterfly, the waves of a workgroup are merged where they agree,
// and only then a row of the table in memory sees one atomic per column (a 100 000-voxel lesion would otherwise send 10^6
// atomics to ten words, which memory-side atomics serialise).
#include "volume_common.h"

namespace mi355 {

constexpr int BX = 64, BY = 8, BZ = 4, BRICK = BX * BY * BZ;  // brick of the local pass: 8 KB of labels + 2 KB of flags in LDS
constexpr int CHUNK = 2048;                                   // voxels per workgroup in the flatten / rank passes
constexpr int NCOL = 14;                                      // columns of the statistics table
constexpr int MAX_COMPONENTS = 65536;                         // rows of the persistent statistics table
constexpr size_t TABLE_BYTES = (size_t)MAX_COMPONENTS * NCOL * sizeof(long long);
constexpr long long COORD_NONE = 1ll << 40;                   // minimum of a row no voxel has reached

__device__ __forceinline__ int ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find_global(const int *par, int a) {
    for (int p = ld(par + a); p != a; p = ld(par + a)) a = p;  // p < a: ends
    return a;
}
__device__ void unite_global(int *par, int a, int b) {
    for (;;) {
        a = find_global(par, a);
        b = find_global(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);  // link the larger root under the smaller
        if (old == a) return;                   // it still was a root: linked
        a = old;                                // somebody linked it first (old < a): go on from there
    }
}
__device__ __forceinline__ int find_local(volatile int *par, int a) {
    for (int p = par[a]; p != a; p = par[a]) a = p;
    return a;
}
__device__ void unite_local(int *par, int a, int b) {
    for (;;) {
        a = find_local(par, a);
        b = find_local(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

// is (dz, dy, dx) a backward neighbour (before the voxel in raster order) of the chosen connectivity (the rank of scipy's
// generate_binary_structure(3, conn))?
__device__ __forceinline__ bool backward(int dz, int dy, int dx, int conn) {
    if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) return false;
    return (dz != 0) + (dy != 0) + (dx != 0) <= conn;  // conn 1: faces (6), 2: faces and edges (18), 3: corners too (26)
}

__global__ __launch_bounds__(256) void ccl_local_kernel(const uint8_t *mask, int d0, int d1, int d2, int nbx, int nby, int conn,
                                                        int *par) {
    __shared__ int lp[BRICK];
    __shared__ uint8_t fg[BRICK];
    const int bid = blockIdx.x;
    const int bx = (bid % nbx) * BX, by = ((bid / nbx) % nby) * BY, bz = (bid / (nbx * nby)) * BZ;
    for (int i = threadIdx.x; i < BRICK; i += 256) {
        const int x = i % BX, y = (i / BX) % BY, z = i / (BX * BY);
        const bool in = bz + z < d0 && by + y < d1 && bx + x < d2;
        fg[i] = in && mask[((int64_t)(bz + z) * d1 + by + y) * d2 + bx + x] != 0;
        lp[i] = i;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BRICK; i += 256) {
        if (!fg[i]) continue;
        const int x = i % BX, y = (i / BX) % BY, z = i / (BX * BY);
        for (int dz = -1; dz <= 0; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!backward(dz, dy, dx, conn)) continue;
                    const int xx = x + dx, yy = y + dy, zz = z + dz;
                    if (xx < 0 || xx >= BX || yy < 0 || yy >= BY || zz < 0) continue;
                    const int j = (zz * BY + yy) * BX + xx;
                    if (fg[j]) unite_local(lp, i, j);
                }
    }
    __syncthreads();
    // (the brick-local order of two voxels is their raster order in the volume too: the local root is the first voxel)
    for (int i = threadIdx.x; i < BRICK; i += 256) {
        const int x = i % BX, y = (i / BX) % BY, z = i / (BX * BY);
        if (!(bz + z < d0 && by + y < d1 && bx + x < d2)) continue;
        const int64_t g = ((int64_t)(bz + z) * d1 + by + y) * d2 + bx + x;
        if (!fg[i]) { par[g] = -1; continue; }
        const int r = find_local(lp, i);
        const int rx = r % BX, ry = (r / BX) % BY, rz = r / (BX * BY);
        par[g] = (int)(((int64_t)(bz + rz) * d1 + by + ry) * d2 + bx + rx);
    }
}

__global__ __launch_bounds__(256) void ccl_seam_kernel(int d0, int d1, int d2, int conn, int *par) {
    const int64_t V = (int64_t)d0 * d1 * d2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < V; g += (int64_t)gridDim.x * 256) {
        const unsigned u = (unsigned)g;
        const int x = (int)(u % (unsigned)d2), y = (int)((u / (unsigned)d2) % (unsigned)d1), z = (int)(u / ((unsigned)d2 * (unsigned)d1));
        if (x % BX && (x + 1) % BX && y % BY && (y + 1) % BY && z % BZ) continue;  // no neighbour of it lies in another brick
        if (ld(par + g) < 0) continue;
        for (int dz = -1; dz <= 0; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!backward(dz, dy, dx, conn)) continue;
                    const int xx = x + dx, yy = y + dy, zz = z + dz;
                    if (xx < 0 || xx >= d2 || yy < 0 || yy >= d1 || zz < 0) continue;
                    if (xx / BX == x / BX && yy / BY == y / BY && zz / BZ == z / BZ) continue;  // the local pass united these
                    const int64_t h = ((int64_t)zz * d1 + yy) * d2 + xx;
                    if (ld(par + h) >= 0) unite_global(par, (int)g, (int)h);
                }
    }
}

// parent[i] = root(i) (other threads may still walk through i: they find the old parent or the root, both ancestors);
// counts[block] = roots among the block's CHUNK voxels
__global__ __launch_bounds__(256) void ccl_flatten_kernel(int *par, int64_t V, int *counts) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int n = 0;
    for (int it = 0; it < CHUNK / 256; ++it) {
        const int64_t i = (int64_t)blockIdx.x * CHUNK + it * 256 + threadIdx.x;
        if (i >= V) break;
        const int p = ld(par + i);
        if (p < 0) continue;
        const int r = find_global(par, p);
        if (r != p) st(par + i, r);
        n += r == (int)i;
    }
    for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[] -> exclusive prefix sums in place, *total = their sum.  One workgroup.
__global__ __launch_bounds__(1024) void ccl_scan_kernel(int *counts, int n, int *total) {
    __shared__ int buf[1024];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        const int c = i < n ? counts[i] : 0;
        buf[t] = c;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int v = t >= off ? buf[t - off] : 0;
            __syncthreads();
            buf[t] += v;
            __syncthreads();
        }
        if (i < n) counts[i] = carry + buf[t] - c;
        carry += buf[1023];
        __syncthreads();
    }
    if (t == 0) *total = carry;
}

__global__ __launch_bounds__(256) void ccl_rank_kernel(const int *par, int64_t V, const int *offsets, int *labels) {
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int running = offsets[blockIdx.x];
    for (int it = 0; it < CHUNK / 256; ++it) {
        const int64_t i = (int64_t)blockIdx.x * CHUNK + it * 256 + threadIdx.x;
        const int p = i < V ? par[i] : -1;
        const bool root = p >= 0 && p == (int)i;
        const unsigned long long m = __ballot(root);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int before = 0, tot = 0;
        for (int ww = 0; ww < 4; ++ww) {
            const int c = wcnt[ww];
            before += ww < w ? c : 0;
            tot += c;
        }
        if (root) labels[i] = running + before + __popcll(m & ((1ull << lane) - 1ull)) + 1;
        else if (i < V && p < 0) labels[i] = 0;
        running += tot;
        __syncthreads();
    }
}

__global__ void ccl_relabel_kernel(const int *par, int64_t V, int *labels) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = par[i];
        if (p >= 0 && p != (int)i) labels[i] = labels[p];  // (roots were written by the launch before, and are not written here)
    }
}

// ------------------------------------------------------------------------------------------------------- statistics
// columns: 0 count, 1..3 coordinate sums, 4..6 minima, 7..9 maxima, 10..13 voxels with seg value 1..4
__device__ __forceinline__ long long col_identity(int k) { return k >= 4 && k <= 6 ? COORD_NONE : (k >= 7 && k <= 9 ? -1 : 0); }
__device__ __forceinline__ long long col_combine(int k, long long a, long long b) {
    return k >= 4 && k <= 6 ? (a < b ? a : b) : (k >= 7 && k <= 9 ? (a > b ? a : b) : a + b);
}
__device__ __forceinline__ void col_flush(long long *table, int label, int k, long long v) {
    long long *w = table + (size_t)(label - 1) * NCOL + k;
    if (k >= 4 && k <= 6) atomicMin(w, v);
    else if (k >= 7 && k <= 9) atomicMax(w, v);
    else if (v) atomicAdd((unsigned long long *)w, (unsigned long long)v);
}

__global__ void ccl_table_init_kernel(long long *table, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) table[i] = col_identity(i % NCOL);
}

constexpr int STAT_CHUNK = 4096;  // voxels per workgroup: 1024 consecutive ones per wave

__global__ __launch_bounds__(256) void ccl_stats_kernel(const int *labels, const uint8_t *seg, int d1, int d2, int64_t V, int n_comp,
                                                        long long *table) {
    __shared__ long long wred[4][NCOL];
    __shared__ int wlab[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wlab[w] = 0;
    int cur = 0;
    long long v[NCOL];
#pragma unroll
    for (int k = 0; k < NCOL; ++k) v[k] = col_identity(k);
    const int64_t base = (int64_t)blockIdx.x * STAT_CHUNK + w * (STAT_CHUNK / 4);
    for (int it = 0; it < STAT_CHUNK / 256; ++it) {
        const int64_t i = base + it * 64 + lane;
        if (i >= V) break;
        const int l = labels[i];
        if (l < 1 || l > n_comp) continue;  // background, or a label beyond the table: never written
        if (l != cur) {
            if (cur) {
#pragma unroll
                for (int k = 0; k < NCOL; ++k) { col_flush(table, cur, k, v[k]); v[k] = col_identity(k); }
            }
            cur = l;
        }
        const unsigned u = (unsigned)i;
        const unsigned zy = u / (unsigned)d2;
        const long long c2 = u - zy * (unsigned)d2, c0 = zy / (unsigned)d1, c1 = zy - (unsigned)c0 * (unsigned)d1;
        const int sv = seg ? seg[i] : 0;
        v[0] += 1; v[1] += c0; v[2] += c1; v[3] += c2;
        v[4] = min(v[4], c0); v[5] = min(v[5], c1); v[6] = min(v[6], c2);
        v[7] = max(v[7], c0); v[8] = max(v[8], c1); v[9] = max(v[9], c2);
        v[10] += sv == 1; v[11] += sv == 2; v[12] += sv == 3; v[13] += sv == 4;
    }
    // the lanes of the wave that ended in the same component are reduced together; the first such group waits in LDS for the
    // other waves, any further group (a wave that straddles several components) goes to the table at once
    unsigned long long pending = __ballot(cur != 0);
    bool first = true;
    while (pending) {
        const int L = __shfl(cur, __ffsll((long long)pending) - 1);
        const bool mine = cur == L;
        long long out = 0;
#pragma unroll
        for (int k = 0; k < NCOL; ++k) {
            long long r = mine ? v[k] : col_identity(k);
            for (int m = 1; m < 64; m <<= 1) r = col_combine(k, r, __shfl_xor(r, m));
            if (lane == k) out = r;
        }
        if (lane < NCOL) {
            if (first) wred[w][lane] = out;
            else col_flush(table, L, lane, out);
        }
        if (first && lane == 0) wlab[w] = L;
        first = false;
        pending &= ~__ballot(mine);
    }
    __syncthreads();
    if (threadIdx.x < NCOL) {
        const int k = threadIdx.x;
        int curL = 0;
        long long acc = 0;
        for (int ww = 0; ww < 4; ++ww) {
            const int L = wlab[ww];
            if (!L) continue;
            if (L == curL) acc = col_combine(k, acc, wred[ww][k]);
            else {
                if (curL) col_flush(table, curL, k, acc);
                curL = L;
                acc = wred[ww][k];
            }
        }
        if (curL) col_flush(table, curL, k, acc);
    }
}

__global__ void ccl_filter_kernel(const int *labels, const uint8_t *seg, int64_t n, const uint8_t *keep, int n_comp, uint8_t *out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int l = labels[i];
        const bool drop = l >= 1 && l <= n_comp && !keep[l];
        out[i] = drop ? 0 : seg[i];
    }
}

}  // namespace mi355

using namespace mi355;

// scratch slot SCR_COMPONENTS: [statistics table, TABLE_BYTES | work area]; the work area holds, for a labelling,
// [total i32, pad to 256 B | chunk counts i32 | parent i32 V] and, for a filter, the keep table.
static int label_components(const uint8_t *mask_dev, int d0, int d1, int d2, int connectivity, int32_t *labels_dev, int32_t *n_components_host,
                            void *stream) {
    MI355_REQUIRE(mask_dev && labels_dev && n_components_host && d0 >= 1 && d1 >= 1 && d2 >= 1, "label_components: bad argument");
    const int64_t V = (int64_t)d0 * d1 * d2;
    MI355_REQUIRE(V < (1ll << 31), "label_components: %dx%dx%d has 2^31 voxels or more (parents are int32 voxel indices)", d0, d1, d2);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nchunks = (V + CHUNK - 1) / CHUNK;
    const size_t counts_bytes = ((size_t)nchunks * sizeof(int) + 255) / 256 * 256;
    char *scr = nullptr;
    MI355_TRY(device_scratch(SCR_COMPONENTS, s, TABLE_BYTES + 256 + counts_bytes + (size_t)V * sizeof(int), (void **)&scr));
    int *total = (int *)(scr + TABLE_BYTES), *counts = (int *)(scr + TABLE_BYTES + 256), *par = (int *)(scr + TABLE_BYTES + 256 + counts_bytes);
    const int nbx = ceil_div(d2, BX), nby = ceil_div(d1, BY), nbz = ceil_div(d0, BZ);
    const int64_t nbricks = (int64_t)nbx * nby * nbz;  // <= V < 2^31
    hipLaunchKernelGGL(ccl_local_kernel, dim3((unsigned)nbricks), dim3(256), 0, s, mask_dev, d0, d1, d2, nbx, nby, connectivity, par);
    hipLaunchKernelGGL(ccl_seam_kernel, dim3(grid_for(V, 256, 16384)), dim3(256), 0, s, d0, d1, d2, connectivity, par);
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, par, V, counts);
    hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, s, counts, (int)nchunks, total);
    hipLaunchKernelGGL(ccl_rank_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, (const int *)par, V, (const int *)counts, labels_dev);
    hipLaunchKernelGGL(ccl_relabel_kernel, dim3(grid_for(V, 256, 16384)), dim3(256), 0, s, (const int *)par, V, labels_dev);
    int n = 0;
    MI355_TRY(read_back(&n, total, sizeof(int), s));
    *n_components_host = n;
    return MI355_OK;
}

extern "C" int mi355_label_components(const uint8_t *mask_dev, int d0, int d1, int d2, int connectivity, int32_t *labels_dev,
                                      int32_t *n_components_host, void *stream) {
    MI355_REQUIRE(connectivity == 1 || connectivity == 3, "label_components: connectivity %d (1 = 6 neighbours, 3 = 26 neighbours)", connectivity);
    return label_components(mask_dev, d0, d1, d2, connectivity, labels_dev, n_components_host, stream);
}

// the same labelling named by the size of the neighbourhood, 18 (faces and edges) included
extern "C" int mi355_label_components_nb(const uint8_t *mask_dev, int d0, int d1, int d2, int neighbours, int32_t *labels_dev,
                                         int32_t *n_components_host, void *stream) {
    MI355_REQUIRE(neighbours == 6 || neighbours == 18 || neighbours == 26, "label_components_nb: %d neighbours (6, 18 or 26)", neighbours);
    return label_components(mask_dev, d0, d1, d2, neighbours == 6 ? 1 : (neighbours == 18 ? 2 : 3), labels_dev, n_components_host, stream);
}

extern "C" int mi355_component_stats(const int32_t *labels_dev, const uint8_t *seg_dev, int d0, int d1, int d2, int n_components,
                                     int64_t *stats_host, void *stream) {
    MI355_REQUIRE(labels_dev && d0 >= 1 && d1 >= 1 && d2 >= 1 && n_components >= 0, "component_stats: bad argument");
    MI355_REQUIRE(n_components <= MAX_COMPONENTS, "component_stats: %d components, the table holds %d (label map too fragmented for per-component statistics)",
                  n_components, MAX_COMPONENTS);
    const int64_t V = (int64_t)d0 * d1 * d2;
    MI355_REQUIRE(V < (1ll << 31), "component_stats: %dx%dx%d has 2^31 voxels or more", d0, d1, d2);
    if (n_components == 0) return MI355_OK;
    MI355_REQUIRE(stats_host, "component_stats: null output");
    hipStream_t s = (hipStream_t)stream;
    long long *table = nullptr;
    MI355_TRY(device_scratch(SCR_COMPONENTS, s, TABLE_BYTES + 256, (void **)&table));
    const int cells = n_components * NCOL;
    hipLaunchKernelGGL(ccl_table_init_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, s, table, cells);
    hipLaunchKernelGGL(ccl_stats_kernel, dim3((unsigned)((V + STAT_CHUNK - 1) / STAT_CHUNK)), dim3(256), 0, s, (const int *)labels_dev, seg_dev,
                       d1, d2, V, n_components, table);
    MI355_TRY(read_back(stats_host, table, (size_t)cells * sizeof(long long), s));
    return MI355_OK;
}

extern "C" int mi355_component_filter(const int32_t *labels_dev, const uint8_t *seg_dev, int64_t n, const uint8_t *keep_host,
                                      int n_components, uint8_t *out_dev, void *stream) {
    MI355_REQUIRE(labels_dev && seg_dev && out_dev && keep_host && n >= 0 && n_components >= 0, "component_filter: bad argument");
    hipStream_t s = (hipStream_t)stream;
    char *scr = nullptr;
    MI355_TRY(device_scratch(SCR_COMPONENTS, s, TABLE_BYTES + 256 + (size_t)n_components + 1, (void **)&scr));
    uint8_t *keep = (uint8_t *)(scr + TABLE_BYTES);
    // (pageable host memory: the copy has left keep_host when this returns, and is ordered on the stream like the kernel)
    MI355_HIP(hipMemcpyAsync(keep, keep_host, (size_t)n_components + 1, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ccl_filter_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, (const int *)labels_dev, seg_dev, n, (const uint8_t *)keep,
                       n_components, out_dev);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}
