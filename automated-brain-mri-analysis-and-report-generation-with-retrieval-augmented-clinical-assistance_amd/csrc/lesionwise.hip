// The three device pieces of lesion-wise scoring (brats_amd.evaluate.lesionwise_metrics) that the labelling of
// components.hip and the surfaces / distance map / gather of surface_distance.hip do not cover:
//   1  binary erosion / dilation with the 6-, 18- or 26-neighbourhood, several steps per launch on a brick staged in LDS
//   2  the joint histogram of two int32 label maps (which components of one map meet which of the other, and in how many voxels)
//   3  out[i] = table[labels[i]]: a label map through a per-component table, to bytes or to int32
//
// All volumes are [d0][d1][d2] C-order with fewer than 2^31 voxels.  Integers only; where threads meet they meet in integer atomics,
// which commute, everything else has one writer per word.  No workgroup waits for another one: every ordering is a launch boundary.
// Nothing here takes device scratch: the second morphology buffer, the histogram and the lookup table live in memory the caller hands
// in with its size, and every word of it that is read was written by the same call before.  A refused call writes to no output.
//
// Morphology: a workgroup owns a brick of MN_BZ x MN_BY x 64 output voxels and keeps it as bit-planes in LDS: one 128-bit word per
// (z, y) row, bit i = the voxel at x = x0 - 32 + i, so the brick's 64 voxels sit in the middle with 32 bits of halo on either side, and
// k rows of halo around the brick along z and y (k = the steps of this launch, at most MI355_MORPH_NB_LDS_STEPS <= 32).  Staging is
// one ballot per 64 bytes of a row; positions outside the volume are 0 (scipy's border_value).  A step is word-parallel: a thread owns
// a row, ORs (dilation) or ANDs (erosion) the up to nine rows around it - those whose (dz, dy) leaves room for an x offset within the
// neighbourhood are widened by a one-bit shift to both sides first - and writes the row to the other LDS buffer.  Step s = 1..k
// recomputes the rows that lie s or more inside the staged block: such a row depends on staged rows only, and a bit that lies s or
// more inside the 128 on bits at most s away, so after k steps the brick itself is exact; what lies nearer the rim holds values that
// nothing reads again.  Rows and bits outside the volume are cleared in every step - they must not carry a dilation back inside.
// More than MI355_MORPH_NB_LDS_STEPS iterations are several such launches that ping-pong between the output and the caller's `tmp`.
// LDS: 2 x 16 x 24 rows x 16 bytes = 12 KiB per workgroup of 256 threads.
//
// Histogram: a workgroup owns PC_CHUNK voxels and counts the pairs whose table index lies below PC_LDS_BINS into 32-bit LDS bins (a
// bin holds at most PC_CHUNK, so it cannot wrap), flushed with one 64-bit global atomic per nonzero bin; a table that fits the bins
// sees no other global atomic.  Pairs beyond the bins - a larger table's rows past the first ones - go to 64-bit global atomics
// directly; the background row (label 0 of the first map), where most voxels of a sparse map fall, is among the first.  Before
// either, the lanes of a wave that hold the pair of the wave's first pending lane fold into that lane, PC_ROUNDS times: a map where
// one pair holds almost every voxel costs one atomic per wave and round, not 64 on one address.  A label outside 0..n never forms an
// address: it is counted in the word behind the table, and a nonzero count there refuses the call.
#include "volume_common.h"

namespace mi355 {

constexpr int MN_BZ = MI355_MORPH_NB_BRICK0, MN_BY = MI355_MORPH_NB_BRICK1, MN_BX = MI355_MORPH_NB_BRICK2;
constexpr int MN_STEPS = MI355_MORPH_NB_LDS_STEPS;
constexpr int MN_XHALO = 32;  // bits of a row word on either side of the brick's 64
constexpr int MN_ROWS = (MN_BZ + 2 * MN_STEPS) * (MN_BY + 2 * MN_STEPS);
static_assert(MN_BX == 64 && MN_STEPS <= MN_XHALO, "a row is one ballot wide; the x halo is half a ballot on either side");
static_assert(2 * MN_ROWS * 16 <= 48 * 1024, "both LDS buffers of a brick with the deepest halo");

constexpr int PC_LDS_BINS = MI355_PAIR_LDS_BINS;
constexpr int64_t PC_MAX_ENTRIES = MI355_PAIR_TABLE_MAX;
constexpr int PC_CHUNK = 16384;  // voxels per workgroup (64 per thread): what a 32-bit LDS bin can hold at most
constexpr int PC_ROUNDS = 2;
constexpr int LK_MAX_LABEL = MI355_LOOKUP_MAX_LABEL;
constexpr int LK_TABLE_OFFSET = 16;  // bytes: the work buffer starts with the word that counts the labels out of range
static_assert(PC_CHUNK % 256 == 0 && PC_LDS_BINS * 4 <= 48 * 1024, "whole rounds of 256 threads; the bins fit LDS");

// ------------------------------------------------------------------------------------------- erosion / dilation, 6 / 18 / 26
struct Row128 { unsigned long long lo, hi; };  // bit i of lo = x0 - 32 + i, bit i of hi = x0 + 32 + i

// bits [a, b) of a 64-bit word, a and b clipped to 0..64
__device__ __forceinline__ unsigned long long bit_range(int a, int b) {
    a = a < 0 ? 0 : a;
    b = b > 64 ? 64 : b;
    if (a >= b) return 0ull;
    const unsigned long long upto_b = b == 64 ? ~0ull : ((1ull << b) - 1ull);
    return upto_b & ~((1ull << a) - 1ull);  // a < b <= 64, so a <= 63
}

// CONN = 1, 2, 3: the offsets with at most CONN nonzero coordinates, scipy's generate_binary_structure(3, CONN)
template <bool DILATE, int CONN>
__global__ __launch_bounds__(256) void morph_nb_kernel(const uint8_t *in, int d0, int d1, int d2, int nby, int nbx, int k, uint8_t *out) {
    __shared__ Row128 rows[2][MN_ROWS];
    const int ez = MN_BZ + 2 * k, ey = MN_BY + 2 * k;  // the staged rows
    int b = blockIdx.x;
    const int bx = b % nbx;
    b /= nbx;
    const int by = b % nby, bz = b / nby;
    const int z0 = bz * MN_BZ - k, y0 = by * MN_BY - k, x0 = bx * MN_BX;  // staged row 0 is (z0, y0); bit 32 of a row is x0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < ez * ey; r += 4) {  // (the same r in every lane of a wave)
        const int lz = r / ey, z = z0 + lz, y = y0 + (r - lz * ey);
        const bool row_inside = z >= 0 && z < d0 && y >= 0 && y < d1;
        const uint8_t *line = in + ((int64_t)(row_inside ? z : 0) * d1 + (row_inside ? y : 0)) * d2;
        Row128 w;
        {
            const int x = x0 - MN_XHALO + lane;
            w.lo = __ballot(row_inside && x >= 0 && x < d2 && x >= x0 - k && line[x] != 0);
        }
        {
            const int x = x0 + MN_XHALO + lane;
            w.hi = __ballot(row_inside && x < d2 && x < x0 + MN_BX + k && line[x] != 0);
        }
        if (lane == 0) rows[0][r] = w;
    }
    // the bits of a row that lie inside the volume
    const unsigned long long in_lo = bit_range(MN_XHALO - x0, d2 - x0 + MN_XHALO), in_hi = bit_range(-MN_XHALO - x0, d2 - x0 - MN_XHALO);
    __syncthreads();
    int cur = 0;
    for (int s = 1; s <= k; ++s) {
        const int rz = ez - 2 * s, ry = ey - 2 * s;  // the rows s or more inside the staged block
        const Row128 *src = rows[cur];
        Row128 *dst = rows[cur ^ 1];
        for (int c = threadIdx.x; c < rz * ry; c += 256) {
            const int qz = c / ry, lz = qz + s, ly = c - qz * ry + s;
            const int z = z0 + lz, y = y0 + ly;
            const int at = lz * ey + ly;
            // `wide`: the rows whose offset (dz, dy) leaves room for dx = +-1 inside the neighbourhood; `plain`: the others that belong to it
            unsigned long long wlo = DILATE ? 0ull : ~0ull, whi = wlo, plo = wlo, phi = wlo;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    const int nz = (dz != 0) + (dy != 0);
                    if (nz > CONN) continue;
                    const Row128 v = src[at + dz * ey + dy];
                    if (nz + 1 <= CONN) {
                        wlo = DILATE ? (wlo | v.lo) : (wlo & v.lo);
                        whi = DILATE ? (whi | v.hi) : (whi & v.hi);
                    } else {
                        plo = DILATE ? (plo | v.lo) : (plo & v.lo);
                        phi = DILATE ? (phi | v.hi) : (phi & v.hi);
                    }
                }
            const unsigned long long up_lo = wlo << 1, up_hi = (whi << 1) | (wlo >> 63);      // the value of x - 1 at x (0 enters at the rim)
            const unsigned long long dn_lo = (wlo >> 1) | (whi << 63), dn_hi = whi >> 1;      // the value of x + 1 at x
            Row128 o;
            o.lo = DILATE ? (wlo | up_lo | dn_lo | plo) : (wlo & up_lo & dn_lo & plo);
            o.hi = DILATE ? (whi | up_hi | dn_hi | phi) : (whi & up_hi & dn_hi & phi);
            const bool row_inside = z >= 0 && z < d0 && y >= 0 && y < d1;
            o.lo = row_inside ? (o.lo & in_lo) : 0ull;
            o.hi = row_inside ? (o.hi & in_hi) : 0ull;
            dst[at] = o;
        }
        __syncthreads();
        cur ^= 1;
    }
    const Row128 *res = rows[cur];
    for (int r = wave; r < MN_BZ * MN_BY; r += 4) {
        const int lz = r / MN_BY, ly = r - lz * MN_BY;
        const int z = bz * MN_BZ + lz, y = by * MN_BY + ly, x = x0 + lane;
        if (z >= d0 || y >= d1 || x >= d2) continue;
        const Row128 w = res[(lz + k) * ey + ly + k];
        const unsigned long long mid = (w.lo >> MN_XHALO) | (w.hi << MN_XHALO);  // bit i = x0 + i
        out[((int64_t)z * d1 + y) * d2 + x] = (uint8_t)((mid >> lane) & 1ull);
    }
}

template <bool DILATE>
static inline void launch_morph_nb(int conn, unsigned blocks, hipStream_t s, const uint8_t *in, int d0, int d1, int d2, int nby, int nbx, int k,
                                   uint8_t *out) {
    if (conn == 1) hipLaunchKernelGGL((morph_nb_kernel<DILATE, 1>), dim3(blocks), dim3(256), 0, s, in, d0, d1, d2, nby, nbx, k, out);
    else if (conn == 2) hipLaunchKernelGGL((morph_nb_kernel<DILATE, 2>), dim3(blocks), dim3(256), 0, s, in, d0, d1, d2, nby, nbx, k, out);
    else hipLaunchKernelGGL((morph_nb_kernel<DILATE, 3>), dim3(blocks), dim3(256), 0, s, in, d0, d1, d2, nby, nbx, k, out);
}

// ------------------------------------------------------------------------------------------- joint histogram of two label maps
// The lanes that hold the key of the first pending lane fold into it, `rounds` times: returns what this lane has to add for its key
// (0: folded into another lane, or key < 0 = nothing to count).  Every lane of the wave must call it.
__device__ __forceinline__ int wave_fold_equal(int key, int rounds) {
    const int lane = threadIdx.x & 63;
    int weight = key >= 0 ? 1 : 0;
    bool pending = key >= 0;
    for (int r = 0; r < rounds; ++r) {
        const unsigned long long active = __ballot(pending);
        if (!active) break;  // the same in every lane
        const int leader = __ffsll((long long)active) - 1;
        const int leader_key = __shfl(key, leader);
        const bool same = pending && key == leader_key;
        const unsigned long long group = __ballot(same);
        if (lane == leader) weight = __popcll(group);
        else if (same) weight = 0;
        pending = pending && !same;
    }
    return weight;
}

// table[a * (nb + 1) + b] += 1 for every voxel; table[(na + 1) * (nb + 1)] += the voxels with a label outside 0..na / 0..nb
__global__ __launch_bounds__(256) void pair_counts_kernel(const int *a, int na, const int *b, int nb, int64_t V, unsigned long long *table) {
    __shared__ unsigned bins[PC_LDS_BINS];
    const int entries = (na + 1) * (nb + 1);
    const int binned = entries < PC_LDS_BINS ? entries : PC_LDS_BINS;
    for (int i = threadIdx.x; i < binned; i += 256) bins[i] = 0;
    __syncthreads();
    int bad = 0;
    for (int r = 0; r < PC_CHUNK / 256; ++r) {
        const int64_t i = (int64_t)blockIdx.x * PC_CHUNK + r * 256 + threadIdx.x;
        int key = -1;
        if (i < V) {
            const int x = a[i], y = b[i];
            if ((unsigned)x <= (unsigned)na && (unsigned)y <= (unsigned)nb) key = x * (nb + 1) + y;
            else ++bad;
        }
        const int w = wave_fold_equal(key, PC_ROUNDS);
        if (w) {
            if (key < PC_LDS_BINS) atomicAdd(&bins[key], (unsigned)w);
            else atomicAdd(&table[key], (unsigned long long)w);
        }
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&table[entries], (unsigned long long)bad);
    __syncthreads();
    for (int i = threadIdx.x; i < binned; i += 256)
        if (bins[i]) atomicAdd(&table[i], (unsigned long long)bins[i]);
}

// ------------------------------------------------------------------------------------------- a label map through a table
__global__ __launch_bounds__(256) void count_labels_out_of_range_kernel(const int *labels, int64_t V, int n, unsigned *count) {
    int c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) c += (unsigned)labels[i] > (unsigned)n;
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned)c);
}

template <typename T>
__global__ __launch_bounds__(256) void label_lookup_kernel(const int *labels, int64_t V, int n, const T *table, T *out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        const int l = labels[i];
        out[i] = (unsigned)l <= (unsigned)n ? table[l] : (T)0;  // (every label was found in range by the launch before)
    }
}

template <typename T>
static int label_lookup(const char *what, const int32_t *labels_dev, int64_t V, int n, const T *table_host, void *work_dev, int64_t work_bytes, T *out_dev,
                        void *stream) {
    MI355_REQUIRE(labels_dev && table_host && work_dev && out_dev, "%s: null pointer", what);
    MI355_REQUIRE((const void *)out_dev != (const void *)labels_dev, "%s: the output must not be the label map", what);
    MI355_REQUIRE(V >= 1 && V < (1ll << 31), "%s: %lld voxels (1 .. 2^31 - 1)", what, (long long)V);
    MI355_REQUIRE(n >= 0 && n <= LK_MAX_LABEL, "%s: labels 0..%d, the table holds 0..%d at most", what, n, LK_MAX_LABEL);
    const int64_t need = LK_TABLE_OFFSET + ((int64_t)n + 1) * (int64_t)sizeof(T);
    MI355_REQUIRE(work_bytes >= need, "%s: %lld bytes of working memory, a table of %d entries needs %lld", what, (long long)work_bytes, n + 1, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    MI355_TRY(bind_device());
    unsigned *count = (unsigned *)work_dev;
    T *table = (T *)((char *)work_dev + LK_TABLE_OFFSET);
    MI355_HIP(hipMemsetAsync(count, 0, sizeof(unsigned), s));
    // (pageable host memory: the copy has left table_host when this returns, and is ordered on the stream like the kernels)
    MI355_HIP(hipMemcpyAsync(table, table_host, ((size_t)n + 1) * sizeof(T), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(count_labels_out_of_range_kernel, dim3(grid_for(V, 256 * 16, 2048)), dim3(256), 0, s, (const int *)labels_dev, V, n, count);
    unsigned bad = 0;
    MI355_TRY(read_back(&bad, count, sizeof(unsigned), s));
    MI355_REQUIRE(bad == 0, "%s: %u voxels carry a label outside 0..%d: nothing was written", what, bad, n);
    hipLaunchKernelGGL(label_lookup_kernel<T>, dim3(grid_for(V, 256 * 4, 16384)), dim3(256), 0, s, (const int *)labels_dev, V, n, (const T *)table, out_dev);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_binary_morphology_nb(const uint8_t *mask_dev, int d0, int d1, int d2, int dilate, int neighbours, int iterations, uint8_t *out_dev,
                                          uint8_t *tmp_dev, int64_t tmp_bytes, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("binary_morphology_nb", d0, d1, d2, &V));
    MI355_REQUIRE(mask_dev && out_dev && mask_dev != out_dev, "binary_morphology_nb: null or aliased pointers (out must not be the input)");
    MI355_REQUIRE(neighbours == 6 || neighbours == 18 || neighbours == 26, "binary_morphology_nb: %d neighbours (6, 18 or 26)", neighbours);
    MI355_REQUIRE(iterations >= 1 && iterations <= 65535,
                  "binary_morphology_nb: iterations %d (1 or more; scipy's 'until nothing changes' (< 1) is not offered)", iterations);
    const int launches = ceil_div(iterations, MN_STEPS);
    if (launches > 1) {
        MI355_REQUIRE(tmp_dev && tmp_dev != mask_dev && tmp_dev != out_dev, "binary_morphology_nb: %d iterations are %d launches of %d steps at most and need a "
                      "second buffer: tmp is null or aliases the input or the output", iterations, launches, MN_STEPS);
        MI355_REQUIRE(tmp_bytes >= V, "binary_morphology_nb: tmp has %lld bytes, %dx%dx%d needs %lld", (long long)tmp_bytes, d0, d1, d2, (long long)V);
    }
    hipStream_t s = (hipStream_t)stream;
    MI355_TRY(bind_device());
    const int nbz = ceil_div(d0, MN_BZ), nby = ceil_div(d1, MN_BY), nbx = ceil_div(d2, MN_BX);
    const unsigned blocks = (unsigned)((int64_t)nbz * nby * nbx);  // <= V < 2^31
    const int conn = neighbours == 6 ? 1 : (neighbours == 18 ? 2 : 3);
    const uint8_t *src = mask_dev;
    int left = iterations;
    for (int l = 0; l < launches; ++l) {
        const int k = left < MN_STEPS ? left : MN_STEPS;
        uint8_t *dst = (launches - 1 - l) % 2 == 0 ? out_dev : tmp_dev;  // the last launch writes out_dev
        if (dilate) launch_morph_nb<true>(conn, blocks, s, src, d0, d1, d2, nby, nbx, k, dst);
        else launch_morph_nb<false>(conn, blocks, s, src, d0, d1, d2, nby, nbx, k, dst);
        src = dst;
        left -= k;
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_label_pair_counts(const int32_t *labels_a_dev, int n_a, const int32_t *labels_b_dev, int n_b, int64_t V, int64_t *table_dev,
                                       int64_t table_words, int64_t *counts_host, void *stream) {
    MI355_REQUIRE(labels_a_dev && labels_b_dev && table_dev && counts_host, "label_pair_counts: null pointer");
    MI355_REQUIRE(V >= 1 && V < (1ll << 31), "label_pair_counts: %lld voxels (1 .. 2^31 - 1)", (long long)V);
    MI355_REQUIRE(n_a >= 0 && n_b >= 0, "label_pair_counts: %d and %d labels", n_a, n_b);
    const int64_t entries = ((int64_t)n_a + 1) * ((int64_t)n_b + 1);
    MI355_REQUIRE(entries <= PC_MAX_ENTRIES, "label_pair_counts: %d and %d labels make a table of %lld entries, %lld at most", n_a, n_b, (long long)entries,
                  (long long)PC_MAX_ENTRIES);
    MI355_REQUIRE(table_words >= entries + 1, "label_pair_counts: %lld words of working memory, the %d x %d table needs %lld (its entries and one)",
                  (long long)table_words, n_a + 1, n_b + 1, (long long)(entries + 1));
    hipStream_t s = (hipStream_t)stream;
    MI355_TRY(bind_device());
    unsigned long long *table = (unsigned long long *)table_dev;
    MI355_HIP(hipMemsetAsync(table, 0, (size_t)(entries + 1) * sizeof(unsigned long long), s));
    const unsigned blocks = (unsigned)((V + PC_CHUNK - 1) / PC_CHUNK);
    hipLaunchKernelGGL(pair_counts_kernel, dim3(blocks), dim3(256), 0, s, (const int *)labels_a_dev, n_a, (const int *)labels_b_dev, n_b, V, table);
    unsigned long long bad = 0;
    MI355_TRY(read_back(&bad, table + entries, sizeof(bad), s));
    MI355_REQUIRE(bad == 0, "label_pair_counts: %llu voxels carry a label outside 0..%d / 0..%d: nothing was written", bad, n_a, n_b);
    MI355_TRY(read_back(counts_host, table, (size_t)entries * sizeof(unsigned long long), s));
    return MI355_OK;
}

extern "C" int mi355_label_lookup(const int32_t *labels_dev, int64_t V, int n, const uint8_t *table_host, void *work_dev, int64_t work_bytes,
                                  uint8_t *out_dev, void *stream) {
    return label_lookup<uint8_t>("label_lookup", labels_dev, V, n, table_host, work_dev, work_bytes, out_dev, stream);
}

extern "C" int mi355_label_lookup_i32(const int32_t *labels_dev, int64_t V, int n, const int32_t *table_host, void *work_dev, int64_t work_bytes,
                                      int32_t *out_dev, void *stream) {
    return label_lookup<int32_t>("label_lookup_i32", labels_dev, V, n, table_host, work_dev, work_bytes, out_dev, stream);
}
