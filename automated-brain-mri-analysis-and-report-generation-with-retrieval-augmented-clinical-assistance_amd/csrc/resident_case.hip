// The hand-off between the inference driver and the analysis of a case that is still on the device (brats_amd.pipeline;
// DESIGN.md row 8f-12).  The driver holds a case in file order - [C][Z][Y][X], the memory of the NIfTI files - while every
// evaluator and feature entry point takes [x][y][z] volumes, so the one thing the join needs is the axis reversal
//
//     dst[c][k][j][i] = src[c][i][j][k]        src [C][d0][d1][d2], dst [C][d2][d1][d0], both contiguous
//
// of float32 modalities (4 bytes per element) and of uint8 label maps (1 byte).  Bits are moved, nothing is computed.
//
// For every (c, j) this is the transpose of a d0 x d2 matrix whose rows lie d1 * d2 elements apart in the source and d1 * d0
// apart in the destination.  A workgroup of 256 threads owns one tile of one such matrix: it reads the tile along d2, the
// source's fastest axis, parks it in LDS, and after one barrier writes it along d0, the destination's fastest axis, so both
// sides of the copy are runs of consecutive addresses.
//
//   4-byte elements: a 64 x 64 tile, one element per lane; a wave reads 256 consecutive bytes of a source row and writes 256
//     consecutive bytes of a destination row.  The LDS rows are 65 words long: the write of a row (lane = k) and the read of a
//     column (lane = i, word i * 65 + k) both touch 32 different banks per 32 lanes.
//   1-byte elements: a 128 x 128 tile in 4 x 4 blocks.  A thread loads four source rows of a block as one 32-bit word each,
//     transposes the sixteen bytes in registers and stores the four words of the transposed block to LDS; afterwards every
//     thread moves one word of a transposed row from LDS to the destination.  Half a wave reads 128 consecutive bytes of a
//     source row and writes 128 consecutive bytes of a destination row, four bytes per lane on either side.  A block that
//     leaves the matrix (the last 1..3 elements of a row or column) is loaded and stored byte by byte.  LDS row r of block
//     column kb is kept at row r * 32 + kb of 33 words: the 32 lanes that store one r of 32 block columns, and the 32 lanes
//     that read one row, each touch 32 different banks.
//
// A row of the source or destination starts wherever the caller's pointer and the shape put it, so the 32-bit accesses of the
// byte variant are made through memcpy: they are correct at any address (the HSA ABI runs the device with unaligned access
// enabled, and the compiler emits one dword access for them).  float32 elements are aligned to 4 bytes by their type.
//
// No device scratch, no atomics, one writer per output element; a refused call launches nothing and so writes nothing.
#include "volume_common.h"

namespace mi355 {

constexpr int RA_F_TILE = 64;                    // float32: the tile is RA_F_TILE x RA_F_TILE elements
constexpr int RA_F_PITCH = RA_F_TILE + 1;        // words per LDS row
constexpr int RA_B_TILE = 128;                   // uint8: the tile is RA_B_TILE x RA_B_TILE elements
constexpr int RA_B_BLOCKS = RA_B_TILE / 4;       // 4 x 4 blocks per tile side
constexpr int RA_B_PITCH = RA_B_BLOCKS + 1;      // words per LDS row
static_assert(RA_F_TILE == 64 && RA_B_BLOCKS == 32, "a wave spans one tile row (float32), half a wave one (uint8)");
static_assert(RA_F_TILE * RA_F_PITCH * 4 <= 48 * 1024 && RA_B_TILE * RA_B_PITCH * 4 <= 48 * 1024, "static LDS");

// The tile of a workgroup: blockIdx.x counts (c, j, tile along d0, tile along d2), the last fastest.
struct RaTile {
    int64_t src0, dst0;  // element offsets of the tile's (i0, k0) in the source and in the destination
    int i0, k0;
};
__device__ __forceinline__ RaTile ra_tile(int d0, int d1, int d2, int ni, int nk, int tile) {
    unsigned b = blockIdx.x;
    const unsigned tk = b % (unsigned)nk;
    b /= (unsigned)nk;
    const unsigned ti = b % (unsigned)ni;
    b /= (unsigned)ni;
    const unsigned j = b % (unsigned)d1, c = b / (unsigned)d1;
    RaTile t;
    t.i0 = (int)ti * tile;
    t.k0 = (int)tk * tile;
    const int64_t plane = (int64_t)c * d0 * d1 * d2;  // a channel has as many elements on either side
    t.src0 = plane + ((int64_t)t.i0 * d1 + j) * d2 + t.k0;
    t.dst0 = plane + ((int64_t)t.k0 * d1 + j) * d0 + t.i0;
    return t;
}

__global__ __launch_bounds__(256) void reverse_axes_b32_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int d0, int d1, int d2,
                                                               int ni, int nk) {
    __shared__ uint32_t tile[RA_F_TILE * RA_F_PITCH];
    const RaTile t = ra_tile(d0, d1, d2, ni, nk, RA_F_TILE);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t src_row = (int64_t)d1 * d2, dst_row = (int64_t)d1 * d0;
    if (t.k0 + lane < d2)
        for (int i = wave; i < RA_F_TILE && t.i0 + i < d0; i += 4) tile[i * RA_F_PITCH + lane] = src[t.src0 + i * src_row + lane];
    __syncthreads();
    if (t.i0 + lane < d0)
        for (int k = wave; k < RA_F_TILE && t.k0 + k < d2; k += 4) dst[t.dst0 + k * dst_row + lane] = tile[lane * RA_F_PITCH + k];
}

// a 32-bit word at any address
__device__ __forceinline__ uint32_t load_word(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ void store_word(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

__global__ __launch_bounds__(256) void reverse_axes_b8_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int d0, int d1, int d2, int ni,
                                                              int nk) {
    __shared__ uint32_t tile[RA_B_TILE * RA_B_PITCH];
    const RaTile t = ra_tile(d0, d1, d2, ni, nk, RA_B_TILE);
    const int64_t src_row = (int64_t)d1 * d2, dst_row = (int64_t)d1 * d0;
    const int in_i = d0 - t.i0, in_k = d2 - t.k0;  // what the matrix holds from the tile's corner on (>= 1)
    // block (ib, kb) = rows i0 + 4 ib .. + 3, columns k0 + 4 kb .. + 3; kb runs with the lane, so half a wave reads one run of a source row
    for (int b = threadIdx.x; b < RA_B_BLOCKS * RA_B_BLOCKS; b += 256) {
        const int kb = b % RA_B_BLOCKS, ib = b / RA_B_BLOCKS;
        const int i = 4 * ib, k = 4 * kb;
        if (i >= in_i || k >= in_k) continue;  // nothing of this block is read back below
        uint32_t a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a[r] = 0u;
            if (i + r >= in_i) continue;
            const uint8_t *p = src + t.src0 + (i + r) * src_row + k;
            if (k + 4 <= in_k) {
                a[r] = load_word(p);
            } else {
                for (int m = 0; k + m < in_k; ++m) a[r] |= (uint32_t)p[m] << (8 * m);
            }
        }
        // byte m of a[r] = element (i + r, k + m)  ->  byte r of word m = the same element: row k + m of the transposed tile
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t w = ((a[0] >> (8 * m)) & 0xffu) | (((a[1] >> (8 * m)) & 0xffu) << 8) | (((a[2] >> (8 * m)) & 0xffu) << 16) |
                               (((a[3] >> (8 * m)) & 0xffu) << 24);
            tile[(m * RA_B_BLOCKS + kb) * RA_B_PITCH + ib] = w;
        }
    }
    __syncthreads();
    // word (k, ib) = elements (i0 + 4 ib .. + 3, k0 + k); ib runs with the lane, so half a wave writes one run of a destination row
    for (int w = threadIdx.x; w < RA_B_TILE * RA_B_BLOCKS; w += 256) {
        const int ib = w % RA_B_BLOCKS, k = w / RA_B_BLOCKS;
        const int i = 4 * ib;
        if (i >= in_i || k >= in_k) continue;
        const uint32_t v = tile[((k & 3) * RA_B_BLOCKS + (k >> 2)) * RA_B_PITCH + ib];
        uint8_t *p = dst + t.dst0 + k * dst_row + i;
        if (i + 4 <= in_i) {
            store_word(p, v);
        } else {
            for (int m = 0; i + m < in_i; ++m) p[m] = (uint8_t)(v >> (8 * m));
        }
    }
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_reverse_axes(const void *src_dev, void *dst_dev, int channels, int d0, int d1, int d2, int elem_bytes, void *stream) {
    MI355_REQUIRE(src_dev && dst_dev, "reverse_axes: null pointer");
    MI355_REQUIRE(channels >= 1 && d0 >= 1 && d1 >= 1 && d2 >= 1, "reverse_axes: bad shape %d x %dx%dx%d (every dimension 1 or more)", channels, d0, d1, d2);
    MI355_REQUIRE(elem_bytes == 1 || elem_bytes == 4, "reverse_axes: %d bytes per element (1 or 4)", elem_bytes);
    // (each partial product stays below 2^62: four factors below 2^31 are multiplied one at a time and checked after each)
    int64_t n = (int64_t)channels * d0;
    const bool fits = n < MI355_REVERSE_AXES_MAX_ELEMENTS && (n *= d1) < MI355_REVERSE_AXES_MAX_ELEMENTS && (n *= d2) < MI355_REVERSE_AXES_MAX_ELEMENTS;
    MI355_REQUIRE(fits, "reverse_axes: %d x %dx%dx%d has 2^31 elements or more", channels, d0, d1, d2);
    const uintptr_t a = (uintptr_t)src_dev, b = (uintptr_t)dst_dev, bytes = (uintptr_t)n * (uintptr_t)elem_bytes;
    MI355_REQUIRE(a + bytes <= b || b + bytes <= a, "reverse_axes: the source and the destination overlap (%lld bytes each)", (long long)bytes);
    MI355_REQUIRE(elem_bytes == 1 || ((a | b) & 3) == 0, "reverse_axes: a pointer to 4-byte elements that is not aligned to 4 bytes");
    hipStream_t s = (hipStream_t)stream;
    MI355_TRY(bind_device());
    const int tile = elem_bytes == 4 ? RA_F_TILE : RA_B_TILE;
    const int ni = ceil_div(d0, tile), nk = ceil_div(d2, tile);
    const unsigned blocks = (unsigned)((int64_t)channels * d1 * ni * nk);  // <= n < 2^31
    if (elem_bytes == 4)
        hipLaunchKernelGGL(reverse_axes_b32_kernel, dim3(blocks), dim3(256), 0, s, (const uint32_t *)src_dev, (uint32_t *)dst_dev, d0, d1, d2, ni, nk);
    else
        hipLaunchKernelGGL(reverse_axes_b8_kernel, dim3(blocks), dim3(256), 0, s, (const uint8_t *)src_dev, (uint8_t *)dst_dev, d0, d1, d2, ni, nk);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}
