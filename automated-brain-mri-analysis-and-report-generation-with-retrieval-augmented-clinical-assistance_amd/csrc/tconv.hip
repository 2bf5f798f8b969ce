// ConvTranspose3d(k=2, s=2, bias=False) on the matrix cores: fp32 tensors NDHWC, fp16 tensors channel-blocked
// ([N][C / 8][V][8], common.h).
//
// Replaces the `tu[u]` modules of the reference decoder
// (model_architecture/generic_UNet.py:363-364, applied at :435).  With kernel == stride the
// op is 8 independent 1x1x1 GEMMs, one per output parity (a,b,c):
//     out[n, 2z+a, 2y+b, 2x+c, co] = sum_ci in[n,z,y,x,ci] * W[ci, co, a, b, c]
// M = input voxels (flattened N*D*H*W), K = Cin, N = Cout per parity.  One tile = 128 input voxels (4 voxel fragments) x 32
// couts x ALL 8 output parities; wave w owns parities {2w, 2w+1}.  Per K group (8 channels in fp32, 16 in fp16) a wave reads 4
// voxel fragments (B operand, from the LDS image of the tile) and 2 weight fragments (A operand, from a host-permuted pack) for
// its MFMAs; D = W^T x X, so a lane holds one voxel and 16 couts.  The input is read Cout/32 times in total instead of 8*Cout/32.
//
// Every kernel here is built from the same three parts - stage_chunk, mfma_group, store_tile - and differs in where the weights
// live and how many tiles a workgroup takes:
//   version 2   weights fetched per K group, one tile per workgroup;
//   version 3   weights in registers, the workgroup strides over the tiles (plan_tconv says when).
#include "conv_plan.h"

#include <vector>

namespace mi355 {

// ---------------------------------------------------------------------------------------------- the parts
// LDS image of a tile's input: planar [16-B piece of the channels][voxel], plane stride padded by one slot so that the staging
// writes are conflict-free too.  Beside it, one 4-KB transpose buffer per wave (store_tile).
template <typename T> constexpr int PIECE = 16 / sizeof(T);  // elements of a 16-B piece: 4 floats, 8 halfs
template <typename T> constexpr int KGROUP = 2 * PIECE<T>;   // channels of one K group: lanes 0-31 / 32-63 hold a piece each
template <typename T> constexpr int XPLANE = 128 * PIECE<T> + PIECE<T>;
template <typename T> constexpr int TRBUF = 4096 / sizeof(T);
template <typename T> using Frag = T __attribute__((ext_vector_type(16 / sizeof(T))));  // f32x4, f16x8
constexpr size_t tconv_lds_bytes(int pieces) { return (size_t)pieces * XPLANE<char> + 4 * TRBUF<char>; }

// Staging of one channel chunk of the 128 voxels from m0 on (rows past M repeat the last voxel).  The voxels go through LDS with
// whole-line loads; a fragment-shaped load straight from global would touch 64 lines per instruction for 16 B each, and the
// texture path, not the matrix pipe, would set the pace.
// Both forms: the `np` 16-B pieces of the channels from channel c0 on, into an image of NP pieces.
// fp32, NDHWC: 16 consecutive lanes read the 256 contiguous bytes of one voxel (NP = 16; the volume's shape is not needed).
template <int NP>
__device__ __forceinline__ void stage_chunk(float *xs, const float *__restrict__ in, int m0, int M, int Cin, int c0, int np, int, int, int,
                                            const FastDiv &, const FastDiv &, const FastDiv &) {
    static_assert(NP == 16, "a voxel's pieces are the low four bits of the thread's index");
    const int tid = threadIdx.x;
#pragma unroll
    for (int k2 = 0; k2 < NP / 2; ++k2) {
        const int i = k2 * 256 + tid, v = i >> 4, q = i & 15;
        int vg = m0 + v;
        if (vg >= M) vg = M - 1;
        if (q < np) *(f32x4 *)(xs + q * XPLANE<float> + v * 4) = *(const f32x4 *)(in + (size_t)vg * Cin + c0 + q * 4);
    }
}
// fp16, channel-blocked: consecutive lanes = consecutive voxels of one 8-channel block.
template <int NP>
__device__ __forceinline__ void stage_chunk(_Float16 *xs, const _Float16 *__restrict__ in, int m0, int M, int Cin, int c0, int np, int D, int H,
                                            int W, const FastDiv &divW, const FastDiv &divH, const FastDiv &divD) {
    const int tid = threadIdx.x;
    __builtin_assume(tid < 256);  // q < NP: a caller that stages all NP pieces (np = NP) has no test per piece
    const long Vi = (long)D * H * W;
#pragma unroll
    for (int k2 = 0; k2 < NP / 2; ++k2) {  // 128 voxels x NP blocks = NP / 2 pieces per thread
        const int i = k2 * 256 + tid, v = i & 127, q = i >> 7;
        int vg = m0 + v;
        if (vg >= M) vg = M - 1;
        const uint32_t ns = fdiv(fdiv(fdiv((uint32_t)vg, divW), divH), divD);
        if (q < np) *(f32x4 *)(xs + q * XPLANE<_Float16> + v * 8) = *(const f32x4 *)(in + (((long)ns * (Cin >> 3) + (c0 >> 3) + q) * Vi + (vg - (long)ns * Vi)) * 8);
    }
}

// One K group: the wave's two parities (weight fragments w0, w1) x the four voxel fragments of the image's planes 2g, 2g + 1
// (lanes 0-31 / 32-63 take the two halves of the group).
// (consecutive MFMAs go to different accumulators: eight independent chains)
__device__ __forceinline__ void mfma_2x4(f32x16 (&acc)[2][4], const f32x4 (&w)[2], const f32x4 (&x)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)  // a 16-B piece = 4 K steps of 32x32x2
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) acc[pp][mf] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[pp][j], x[mf][j], acc[pp][mf], 0, 0, 0);
}
__device__ __forceinline__ void mfma_2x4(f32x16 (&acc)[2][4], const f16x8 (&w)[2], const f16x8 (&x)[4]) {
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) acc[pp][mf] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[pp], x[mf], acc[pp][mf], 0, 0, 0);
}
template <typename T>
__device__ __forceinline__ void mfma_group(f32x16 (&acc)[2][4], const T *xs, int g, const Frag<T> (&w)[2]) {
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    Frag<T> x[4];
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) x[mf] = *(const Frag<T> *)(xs + (2 * g + half) * XPLANE<T> + (mf * 32 + l31) * PIECE<T>);
    mfma_2x4(acc, w, x);
}

// (n, z, y, x) of input voxel v
__device__ __forceinline__ void decode_voxel(int v, int D, int H, int W, const FastDiv &divW, const FastDiv &divH, const FastDiv &divD,
                                             uint32_t *n, int *z, int *y, int *x) {
    const uint32_t q1 = fdiv((uint32_t)v, divW);
    *x = v - (int)q1 * W;
    const uint32_t q2 = fdiv(q1, divH);
    *y = (int)q1 - (int)q2 * H;
    *n = fdiv(q2, divD);
    *z = (int)q2 - (int)*n * D;
}
// a lane's 64-bit `v`, as lane `src` holds it
__device__ __forceinline__ long shfl_long(long v, int src) {
    const int lo = __shfl((int)(v & 0xffffffff), src), hi = __shfl((int)(v >> 32), src);
    return ((long)hi << 32) | (unsigned)lo;
}

// `v`, opaque to the compiler: what is derived from it is computed where it is used.  store_tile takes the thread index this
// way.  Left to itself the compiler computes the lane's dozen swizzled LDS addresses once, in front of a persistent kernel's
// tile loop, and carries them through it in registers that version 3 does not have: tconv2_f16_mfma_v3_kernel<8> spilled five
// of them and reloaded them for every tile, tconv2_f32_mfma_v3_kernel<8> sat six registers under the limit.  Per tile they are
// some twenty VALU instructions beside 128 or more MFMAs.
__device__ __forceinline__ int per_call(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// The store of a tile.  A lane holds one voxel and 16 couts, so a direct store instruction touches 32 different 128-B lines with
// 16-B pieces - 16 K line operations per workgroup through the texture path, as many cycles as the MFMAs take.  Each fragment
// therefore goes through the wave's 4-KB LDS transpose buffer `tr` (XOR-swizzled 16-B pieces, conflict-free both ways) and is
// stored as whole lines.  The output offset of a voxel's parity-(0,0,0) row (-1 = voxel beyond the tensor), not the voxel index,
// travels through the shuffles: no 64-bit multiply per store.
// fp32, NDHWC: a 32-voxel x 32-cout tile per parity; 8 lanes per voxel, 8 lines per instruction.
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[2][4], float *tr, float *out, int m0, int M, int Cout, int nb, int D, int H,
                                           int W, const FastDiv &divW, const FastDiv &divH, const FastDiv &divD) {
    const int tid = per_call(threadIdx.x), lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int Ho = 2 * H, Wo = 2 * W, Do = 2 * D;
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
        const int v = m0 + mf * 32 + l31;
        uint32_t n;
        int z, y, x;
        decode_voxel(v < M ? v : M - 1, D, H, W, divW, divH, divD, &n, &z, &y, &x);
        const long vox000 = v < M ? ((((long)n * Do + 2 * z) * Ho + 2 * y) * Wo + 2 * x) * Cout : -1;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int pos = wave * 2 + pp;
            const int pa = pos >> 2, pb = (pos >> 1) & 1, pc = pos & 1;
            const long padd = (((long)pa * Ho + pb) * Wo + pc) * Cout + nb * 32;
            // write: row = voxel l31, 16-B piece (2*g4 + half) at physical piece (piece ^ (row & 7))
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 val = {acc[pp][mf][4 * g4], acc[pp][mf][4 * g4 + 1], acc[pp][mf][4 * g4 + 2], acc[pp][mf][4 * g4 + 3]};
                *(f32x4 *)(tr + l31 * 32 + (((2 * g4 + half) ^ (l31 & 7)) << 2)) = val;
            }
            // read back: lane = (row r, piece c); the row's output offset comes from the lane that owns the voxel
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int r = it * 8 + (lane >> 3), c = lane & 7;
                const f32x4 val = *(const f32x4 *)(tr + r * 32 + ((c ^ (r & 7)) << 2));
                const long vo = shfl_long(vox000, r);
                if (vo >= 0) *(f32x4 *)(out + (vo + padd) + c * 4) = val;
            }
        }
    }
}
// fp16, channel-blocked ([N][Cout / 8][Vo][8]): a wave's two parities (pa, pb, 0) and (pa, pb, 1) are x-neighbours, so a row of
// the buffer is (voxel, 2 parities x 32 couts) = 128 B, and the 32 input voxels of a fragment (one x-row when W >= 32) become 64
// consecutive output voxels = 1 KiB contiguous in each of the four 8-cout blocks.
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[2][4], _Float16 *tr, _Float16 *out, int m0, int M, int Cout, int nb, int D,
                                           int H, int W, const FastDiv &divW, const FastDiv &divH, const FastDiv &divD) {
    const int tid = per_call(threadIdx.x), lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int Ho = 2 * H, Wo = 2 * W, Do = 2 * D;
    const int pa = wave >> 1, pb = wave & 1;
    const long Vo = (long)Do * Ho * Wo;
    const long padd = ((long)pa * Ho + pb) * Wo;  // voxels
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
        const int v = m0 + mf * 32 + l31;
        uint32_t n;
        int z, y, x;
        decode_voxel(v < M ? v : M - 1, D, H, W, divW, divH, divD, &n, &z, &y, &x);
        // 16-B piece index of output voxel (2z, 2y, 2x) in cout block nb * 4 of sample n
        const long vox000 = v < M ? ((long)n * (Cout >> 3) + nb * 4) * Vo + (((long)2 * z) * Ho + 2 * y) * Wo + 2 * x : -1;
        // write: row = voxel l31; 16-B piece pp*4 + g4 at physical piece (piece ^ (row & 7))
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f16x4 hv = {(_Float16)acc[pp][mf][4 * g4], (_Float16)acc[pp][mf][4 * g4 + 1],
                                  (_Float16)acc[pp][mf][4 * g4 + 2], (_Float16)acc[pp][mf][4 * g4 + 3]};
                *(f16x4 *)(tr + l31 * 64 + (((pp * 4 + g4) ^ (l31 & 7)) << 3) + half * 4) = hv;
            }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            // store `it` = cout block it: lane -> (input voxel r = lane >> 1, x parity = lane & 1)
            const int r = lane >> 1, pc = lane & 1;
            const f32x4 val = *(const f32x4 *)(tr + r * 64 + (((pc * 4 + it) ^ (r & 7)) << 3));
            const long vo = shfl_long(vox000, r);
            if (vo >= 0) *(f32x4 *)(out + (vo + (long)it * Vo + padd + pc) * 8) = val;
        }
    }
}

// the weight fragments of wave `wave`'s parity 2 * wave + pp, cout block nb: [G groups][64 lanes][16 B] (tconv_pack)
template <typename T>
__device__ __forceinline__ const T *weight_row(const T *wp, int pp, int nblk, int nb, int G) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return wp + ((size_t)((wave * 2 + pp) * nblk + nb) * G) * (64 * PIECE<T>) + lane * PIECE<T>;
}

// ---------------------------------------------------------------------------------------------- the kernels
// Version 2: the image holds 64 channels at a time, the last chunk may be partial.
template <typename T>
__device__ __forceinline__ void tconv2_v2(const T *__restrict__ in, const T *__restrict__ wp, T *out, int M, int Cin, int Cout, int D, int H, int W,
                                          const FastDiv &divW, const FastDiv &divH, const FastDiv &divD) {
    constexpr int NP = 64 / PIECE<T>;
    __shared__ __attribute__((aligned(16))) T xs[NP * XPLANE<T>];
    __shared__ __attribute__((aligned(16))) T tr[4][TRBUF<T>];
    static_assert(sizeof(xs) + sizeof(tr) == tconv_lds_bytes(NP), "plan_tconv reports this size");
    const int nblk = Cout >> 5, nb = (int)blockIdx.y, m0 = (int)blockIdx.x * 128;
    const T *wrow[2];
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) wrow[pp] = weight_row(wp, pp, nblk, nb, Cin / KGROUP<T>);
    f32x16 acc[2][4];  // (zeroed in place: through a helper, or by `= {}`, the fp32 kernel takes 16 more registers)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[pp][mf][r] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += 64) {
        const int np = (Cin - c0 < 64 ? Cin - c0 : 64) / PIECE<T>;  // pieces in this chunk, an even number (Cin % KGROUP == 0)
        if (c0) __syncthreads();
        stage_chunk<NP>(xs, in, m0, M, Cin, c0, np, D, H, W, divW, divH, divD);
        __syncthreads();
        const int gn = np >> 1;
        constexpr int UNROLL = sizeof(T) == 4 ? 2 : 1;
#pragma unroll UNROLL
        for (int g = 0; g < gn; ++g) {
            Frag<T> wv[2];
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) wv[pp] = *(const Frag<T> *)(wrow[pp] + (size_t)(c0 / KGROUP<T> + g) * (64 * PIECE<T>));
            mfma_group(acc, xs, g, wv);
        }
    }
    store_tile(acc, tr[threadIdx.x >> 6], out, m0, M, Cout, nb, D, H, W, divW, divH, divD);
}
__global__ __launch_bounds__(256) void tconv2_f32_mfma_v2_kernel(const float *__restrict__ in, const float *__restrict__ wp, float *out, int M,
                                                                int Cin, int Cout, int D, int H, int W, FastDiv divW, FastDiv divH,
                                                                FastDiv divD) {
    tconv2_v2(in, wp, out, M, Cin, Cout, D, H, W, divW, divH, divD);
}
// Two workgroups per CU (round 2): left to itself hipcc spread this kernel over 146 VGPRs + 128 AGPRs, one wave per SIMD, and a
// workgroup that loads, computes and stores in sequence had nothing to overlap with (137 -> 111 us per launch; three per CU spill).
__global__ __launch_bounds__(256, 2) void tconv2_f16_mfma_v2_kernel(const _Float16 *__restrict__ in, const _Float16 *__restrict__ wp,
                                                                   _Float16 *out, int M, int Cin, int Cout, int D, int H, int W,
                                                                   FastDiv divW, FastDiv divH, FastDiv divD) {
    tconv2_v2(in, wp, out, M, Cin, Cout, D, H, W, divW, divH, divD);
}

// Version 3: version 2 made persistent, with the wave's weights in registers.  A workgroup of version 2 re-reads its weight block
// from the L2 for every 128 voxels (fp16, Cin = 128: Cin x 512 B, as many bytes as the 64 KiB of output it stores - the L1 moved
// 2.5 x the HBM traffic of a kernel that should be bound by its output stream), waits for each fragment in front of the MFMAs
// that use it, and has nothing to overlap its load - compute - store sequence with but the other workgroups of its CU.  Here the two
// parities' fragments of a wave stay in 8 G registers (G K groups, fixed at compile time) and the workgroup strides over the voxel
// tiles; per tile only the 128 x Cin input block comes through the L1.  The image holds up to 16 pieces: 64 channels at a time
// in fp32, as in version 2, and all Cin <= 128 at once in fp16.
template <typename T, int G>
__device__ __forceinline__ void tconv2_v3(const T *__restrict__ in, const T *__restrict__ wp, T *out, int M, int Cout, int D, int H, int W,
                                          const FastDiv &divW, const FastDiv &divH, const FastDiv &divD) {
    constexpr int Cin = G * KGROUP<T>;
    constexpr int NP = Cin / PIECE<T> < 16 ? Cin / PIECE<T> : 16;
    __shared__ __attribute__((aligned(16))) T xs[NP * XPLANE<T>];
    __shared__ __attribute__((aligned(16))) T tr[4][TRBUF<T>];
    static_assert(sizeof(xs) + sizeof(tr) == tconv_lds_bytes(NP), "plan_tconv reports this size");
    const int nblk = Cout >> 5, nb = (int)blockIdx.y;
    Frag<T> wreg[G][2];
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
        for (int g = 0; g < G; ++g) wreg[g][pp] = *(const Frag<T> *)(weight_row(wp, pp, nblk, nb, G) + (size_t)g * (64 * PIECE<T>));
    const int ntiles = (M + 127) >> 7;
    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
        const int m0 = tile * 128;
        f32x16 acc[2][4];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int mf = 0; mf < 4; ++mf)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[pp][mf][r] = 0.f;
#pragma unroll
        for (int g0 = 0; g0 < G; g0 += NP / 2) {
            if (g0 || tile != (int)blockIdx.x) __syncthreads();  // the previous image's fragment reads are done
            stage_chunk<NP>(xs, in, m0, M, Cin, g0 * KGROUP<T>, NP, D, H, W, divW, divH, divD);
            __syncthreads();
#pragma unroll
            for (int g = 0; g < NP / 2; ++g) mfma_group(acc, xs, g, wreg[g0 + g]);
        }
        store_tile(acc, tr[threadIdx.x >> 6], out, m0, M, Cout, nb, D, H, W, divW, divH, divD);
    }
}
// (Cin = 64 only, plan_tconv: at Cin = 128 - 128 weight registers, one workgroup per CU - version 3 measured slower than version
//  2, 3.4 against 3.0 ms for 128 -> 64 @ 8 x 32^3)
template <int G>
__global__ __launch_bounds__(256, G <= 8 ? 2 : 1) void tconv2_f32_mfma_v3_kernel(const float *__restrict__ in, const float *__restrict__ wp,
                                                                                float *out, int M, int Cout, int D, int H, int W,
                                                                                FastDiv divW, FastDiv divH, FastDiv divD) {
    tconv2_v3<float, G>(in, wp, out, M, Cout, D, H, W, divW, divH, divD);
}
template <int G>
__global__ __launch_bounds__(256, 2) void tconv2_f16_mfma_v3_kernel(const _Float16 *__restrict__ in, const _Float16 *__restrict__ wp,
                                                                   _Float16 *out, int M, int Cout, int D, int H, int W, FastDiv divW,
                                                                   FastDiv divH, FastDiv divD) {
    tconv2_v3<_Float16, G>(in, wp, out, M, Cout, D, H, W, divW, divH, divD);
}

// ---------------------------------------------------------------------------------------------- host side
static int tconv_channels_ok(int dtype, int cin, int cout) {
    const int kg = dtype == MI355_F16 ? KGROUP<_Float16> : KGROUP<float>;
    MI355_REQUIRE(cin > 0 && cout > 0 && cin % kg == 0 && cout % 32 == 0, "%stconv %d->%d: need cin %% %d == 0 and cout %% 32 == 0",
                  dtype == MI355_F16 ? "fp16 " : "", cin, cout, kg);
    return MI355_OK;
}

// pack: [pos = a*4+b*2+c][cout block][g][lane][j]; cout = nb*32 + (lane&31), cin = g*KGROUP + (lane>>5)*PIECE + j
template <typename T>
static int tconv_pack_upload(DeviceAllocs &mem, const float *w_host, int cin, int cout, void **wp_dev) {
    const int G = cin / KGROUP<T>, nblk = cout / 32;
    std::vector<T> packed((size_t)8 * nblk * G * 64 * PIECE<T>);
    size_t o = 0;
    for (int pos = 0; pos < 8; ++pos)
        for (int nb = 0; nb < nblk; ++nb)
            for (int g = 0; g < G; ++g)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < PIECE<T>; ++j, ++o) {
                        const int co = nb * 32 + (lane & 31);
                        const int ci = g * KGROUP<T> + (lane >> 5) * PIECE<T> + j;
                        packed[o] = (T)w_host[((size_t)ci * cout + co) * 8 + pos];
                    }
    return mem.upload(packed.data(), packed.size() * sizeof(T), wp_dev);
}

int tconv_weights_upload(DeviceAllocs &mem, const float *w_host, int cin, int cout, int dtype, TConvWeights *out) {
    MI355_TRY(tconv_channels_ok(dtype, cin, cout));
    TConvWeights tw;
    tw.cin = cin; tw.cout = cout; tw.dtype = dtype;
    MI355_TRY(dtype == MI355_F16 ? tconv_pack_upload<_Float16>(mem, w_host, cin, cout, &tw.wp_dev) : tconv_pack_upload<float>(mem, w_host, cin, cout, &tw.wp_dev));
    *out = tw;
    return MI355_OK;
}

static KernelRow tconv_rows[] = {
    MI355_KERNEL_ROW(tconv2_f32_mfma_v2_kernel),
    MI355_KERNEL_ROW(tconv2_f32_mfma_v3_kernel<8>),
    MI355_KERNEL_ROW(tconv2_f16_mfma_v2_kernel),
    MI355_KERNEL_ROW(tconv2_f16_mfma_v3_kernel<2>),
    MI355_KERNEL_ROW(tconv2_f16_mfma_v3_kernel<4>),
    MI355_KERNEL_ROW(tconv2_f16_mfma_v3_kernel<8>),
};

int plan_tconv(int dtype, int cin, int cout, long M, TconvPlan *p) {
    MI355_TRY(tconv_channels_ok(dtype, cin, cout));
    MI355_REQUIRE(M > 0 && M < (1l << 30), "tconv: %ld voxels out of range", M);
    const bool f16 = dtype == MI355_F16;
    const long ntiles = (M + 127) / 128;
    const int nblk = cout / 32, G = cin / (f16 ? KGROUP<_Float16> : KGROUP<float>);
    KernelRow *v3 = env_switch("MI355_TCONV_V3") && ntiles >= 1024 ? find_row(tconv_rows, "tconv2_%s_mfma_v3_kernel<%d>", f16 ? "f16" : "f32", G) : nullptr;
    p->persistent = v3 != nullptr;
    p->row = v3 ? v3 : find_row(tconv_rows, "tconv2_%s_mfma_v2_kernel", f16 ? "f16" : "f32");
    p->gy = (unsigned)nblk;
    p->gx = (unsigned)ntiles;
    if (v3) {  // two workgroups per CU and cout block share the 512 resident slots
        const long gx = 512 / nblk < 8 ? 8 : 512 / nblk;
        if (gx < ntiles) p->gx = (unsigned)gx;
    }
    const int pieces = f16 ? (v3 ? cin / 8 : 8) : 16;
    p->lds_bytes = tconv_lds_bytes(pieces);
    return MI355_OK;
}

int launch_tconv(const TConvWeights &w, const TconvPlan &p, const void *in, int N, int D, int H, int W, void *out, hipStream_t s) {
    int M = (int)((long)N * D * H * W), cin = w.cin, cout = w.cout;
    FastDiv divW = make_fastdiv(W), divH = make_fastdiv(H), divD = make_fastdiv(D);
    const void *wp = w.wp_dev;
    void *args[] = {&in, &wp, &out, &M, &cin, &cout, &D, &H, &W, &divW, &divH, &divD};
    void *args_v3[] = {&in, &wp, &out, &M, &cout, &D, &H, &W, &divW, &divH, &divD};  // (Cin is the instantiation's)
    MI355_HIP(hipLaunchKernel(p.row->fn, dim3(p.gx, p.gy), dim3(256), p.persistent ? args_v3 : args, 0, s));
    return MI355_OK;
}

int tconv2_mfma(const TConvWeights &w, const void *in, int N, int D, int H, int W, void *out, hipStream_t s, const char **kernel_name) {
    TconvPlan p;
    MI355_TRY(plan_tconv(w.dtype, w.cin, w.cout, (long)N * D * H * W, &p));
    if (kernel_name) *kernel_name = p.row->name;
    return launch_tconv(w, p, in, N, D, H, W, out, s);
}

}  // namespace mi355

