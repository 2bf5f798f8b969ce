// The body of conv3_f32_s2dma_kernel, included by conv3d.hip twice: S2DMA_VIEW = 0 is the plain kernel (its listing does not
// change when the view code below does); S2DMA_VIEW = 1 is conv3_f32_s2dma_kernel_view, which reads its input
// through a stage-0 view (kernels.h S0View): in0 holds only the shells of its samples, every other voxel is read in place from the
// whole-volume tensor the view names.  Per tile (decode, scalar): the sample's view words, the brick corner's voxel index in the
// view's tensor and which brick planes / rows / columns lie in a shell - planes and rows as one-hot fields that a piece tests with
// one AND against its own (the spare bits of dma_pk), columns as two bounds.  Per piece: the second offset and a branch-free
// select.  The DMA count per wave is the same.
// (Shared as text and not as a function template: handed its arguments through a reference or a copy, the plain kernel compiled to
// a different listing - the loads of its arguments are then no longer known to be loads of kernel arguments.)
// No include guard: S2DMA_VIEW is defined by the including file.
template <int TXL>
#if S2DMA_VIEW
__global__ __launch_bounds__(256, 1) void conv3_f32_s2dma_kernel_view(S2ViewArgs va) {
    const Wino2Args &pa = va.w;
    const S0View &vw = va.v;
#else
__global__ __launch_bounds__(256, 1) void conv3_f32_s2dma_kernel(Wino2Args pa) {
#endif
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ConvArgs &p = pa.c;
    typedef S2Geom<TXL> GM;
    constexpr int IX = GM::IX, IY = GM::IY, BV = GM::BV;
    constexpr int S2_BUF_FLOATS = GM::BUF_FLOATS, S2_WSLOT_FLOATS = GM::WSLOT_FLOATS, S2_RSTRIDE = GM::RSTRIDE;
    constexpr int S2_WPIECE_BYTES = GM::WPIECE_BYTES, S2_WLO_BYTES = GM::WPIECE_BYTES, S2_WPLANE_BYTES = 3 * GM::WPIECE_BYTES;
    // the lo pieces of the two ring slots: static, beside the dynamic image whose size the plan pins (hi + mid = the old 18 KiB slot)
    __shared__ __attribute__((aligned(16))) unsigned wlo[2 * S2_WLO_BYTES / 4];
    typedef unsigned s2u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned s2u32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 s2bf16x8 __attribute__((ext_vector_type(8)));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l31 = lane & 31;
    float *wring = lds + 2 * S2_BUF_FLOATS;

    const int xcd = (int)blockIdx.x & 7, li = (int)blockIdx.x >> 3;
    const int nl = ((int)gridDim.x - xcd + 7) >> 3;
    const int q8 = pa.total_tiles >> 3, r8 = pa.total_tiles & 7;
    const int lo = xcd * q8 + (xcd < r8 ? xcd : r8);
    const int hi = lo + q8 + (xcd < r8 ? 1 : 0);
    int tile = lo + li;
    if (tile >= hi) return;

#if S2DMA_VIEW
    // voff, faces: the view words of sample n (S0ViewSample).  What a brick derives from them is scalar arithmetic in dma_brick and
    // not kept per tile: three tile positions are live across the main loop, and the scalar registers are what this kernel is short of.
    struct TileCoord { int n, oz0, oy0, ox0; unsigned voff, faces; };
    // planes c0 .. c0 + n - 1 of an axis, as bits: those below lo or at / above hi
    auto shell_bits = [](int c0, int n, int lo, int hi) {
        int a = lo - c0, b = hi - c0;
        a = a < 0 ? 0 : (a > n ? n : a);
        b = b < 0 ? 0 : (b > n ? n : b);
        return ((1u << a) - 1u) | (((1u << n) - 1u) & ~((1u << b) - 1u));
    };
#else
    struct TileCoord { int n, oz0, oy0, ox0; };
#endif
    auto decode = [&](int t) {
        TileCoord tc;
        tc.n = (int)fdiv((uint32_t)t, p.div_tiles_per_n);
        const int tt = t - tc.n * (int)p.div_tiles_per_n.d;
        int tile_x, tile_y, tile_z;
        tile_from_id(tt, pa.order, tile_x, tile_y, tile_z);
        tc.oz0 = tile_z << 1; tc.oy0 = tile_y * GM::TY; tc.ox0 = tile_x << TXL;
#if S2DMA_VIEW
        const S0ViewSample sm = vw.smp[tc.n & (S0_VIEW_MAX_SAMPLES - 1)];  // (host: N <= S0_VIEW_MAX_SAMPLES; the index never leaves the arguments)
        tc.voff = sm.off; tc.faces = sm.faces;
#endif
        return tc;
    };

    // brick DMA: 7 ranges per wave, both quads of a range back to back.  Range r = voxels [59r, 59r + 64) of a quad
    // plane; overlaps carry identical data, the tail of range 27 runs into the next plane (or the padding).
    unsigned dma_pk[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        int bv = (wave + 4 * k) * S2_RSTRIDE + lane;
        const int over = bv >= BV ? 1 : 0;
        bv -= over * BV;
        const int rr = bv / IX, bx = bv - rr * IX;
        const int rz = rr / IY, ry = rr - rz * IY;
        dma_pk[k] = (unsigned)(rz | (ry << 4) | (bx << 8) | (over << 16));
#if S2DMA_VIEW
        dma_pk[k] |= (1u << (17 + rz)) | (1u << (22 + ry));  // one-hot, against TileCoord::mzy (rz <= 4, ry <= 8)
#endif
    }
    auto dma_brick = [&](const TileCoord &tc, int ch, int k, float *buf) {
        const int rng = wave + 4 * k;
        const int cglob = ch * 8;
#if S2DMA_VIEW
        const float *src = p.in0; const int Csrc = p.C0, coff = cglob;  // (host: a view comes with a single input tensor, C1 == 0)
#else
        const float *src; int Csrc, coff;
        if (cglob < p.C0) { src = p.in0; Csrc = p.C0; coff = cglob; }
        else { src = p.in1; Csrc = p.C1; coff = cglob - p.C0; }
#endif
        src += ((((size_t)tc.n * p.Di + (2 * tc.oz0 - 1)) * p.Hi + (2 * tc.oy0 - 1)) * p.Wi + (2 * tc.ox0 - 1)) * (long)Csrc + coff;
        const unsigned pk = dma_pk[k];
#if S2DMA_VIEW
        const int rz = pk & 15, ry = (pk >> 4) & 15, bx = (pk >> 8) & 255, over = (pk >> 16) & 1;
#else
        const int rz = pk & 15, ry = (pk >> 4) & 15, bx = (pk >> 8) & 255, over = pk >> 16;
#endif
        const bool in_vol = ((unsigned)(2 * tc.oz0 - 1 + rz) < (unsigned)p.Di) && ((unsigned)(2 * tc.oy0 - 1 + ry) < (unsigned)p.Hi) &&
                            ((unsigned)(2 * tc.ox0 - 1 + bx) < (unsigned)p.Wi);
        const int voff = ((rz * p.Hi + ry) * p.Wi + bx) * Csrc + over * 4;
#if S2DMA_VIEW
        // Scalar, per brick: the voxel index of its corner in the view's tensor, its planes (bit 17 + rz) and rows (bit 22 + ry) that
        // lie in a shell as one-hot fields, and the bounds of its columns that do not.
        // Per piece: its address in the view's tensor (the view's strides in place of Hi, Wi), taken unless the piece lies in a shell;
        // the in-volume select stays in front: a halo piece beyond a tile face is zero although the view has neighbours there
        // (host: C1 == 0, and every offset formed here fits 32 bits)
        const int z0 = 2 * tc.oz0 - 1, y0 = 2 * tc.oy0 - 1, x0 = 2 * tc.ox0 - 1, dpt = vw.depth;
        const long vbase = (long)tc.voff + (long)z0 * vw.sz + (long)y0 * vw.sy + x0;
        const unsigned mz = shell_bits(z0, GM::IZ, (tc.faces & 1u) ? dpt : 0, (tc.faces & 2u) ? p.Di - dpt : p.Di);
        const unsigned my = shell_bits(y0, IY, (tc.faces & 4u) ? dpt : 0, (tc.faces & 8u) ? p.Hi - dpt : p.Hi);
        const unsigned mzy = (mz << 17) | (my << 22);
        const int xlo = ((tc.faces & 16u) ? dpt : 0) - x0, xhi = ((tc.faces & 32u) ? p.Wi - dpt : p.Wi) - x0;
        const float *vsrc = vw.src + (vbase * (long)Csrc + coff);
        const int vvoff = ((rz * vw.sz + ry * vw.sy) + bx) * Csrc + over * 4;
        const bool shell = (pk & mzy) != 0 || (unsigned)(bx - xlo) >= (unsigned)(xhi - xlo);
        const float *gin = shell ? src + voff : vsrc + vvoff;
        const float *g0 = in_vol ? gin : pa.zeros;
        const float *g1 = (in_vol && over == 0) ? gin : pa.zeros;
#else
        const float *g0 = in_vol ? src + voff : pa.zeros;
        const float *g1 = (in_vol && over == 0) ? src + voff : pa.zeros;  // quad 1's overrun lanes fill padding
#endif
        asm volatile("" : "+v"(g0), "+v"(g1));
        float *dst = buf + rng * S2_RSTRIDE * 4;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g0,
                                         (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g1,
                                         (__attribute__((address_space(3))) void *)(dst + BV * 4 - 4), 16, 16, 0);
    };
    // weight DMA: dz plane `dz` of chunk `ch` = 27 KiB contiguous in the split pack (pack_conv_weights_s2split): KiB 0-8 the hi pieces,
    // 9-17 the mid pieces - together one slot of the ring -, 18-26 the lo pieces, which go to the slot's half of wlo.  KiB k goes to
    // wave k & 3, round k >> 2.
    const char *wblk = (const char *)p.wp + (size_t)blockIdx.y * p.nchunks * (3 * S2_WPLANE_BYTES);
    auto dma_weights = [&](int ch, int dz, int slot, int i_lo = 0, int i_hi = 7) {
        const char *wsrc = wblk + ((size_t)ch * 3 + dz) * S2_WPLANE_BYTES + lane * 16;
        char *whm = (char *)(wring + slot * S2_WSLOT_FLOATS), *wl = (char *)(wlo + slot * (S2_WLO_BYTES / 4));
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            if (i < i_lo || i >= i_hi) continue;  // (compile-time at the call sites)
            // (no branch: KiB 27 does not exist - wave 3 fetches KiB 26 a second time in the last round, the same bytes into the
            //  same place as wave 2)
            const int kib = wave + 4 * i < 27 ? wave + 4 * i : 26;
            char *dst = kib < 18 ? whm + kib * 1024 : wl + (kib - 18) * 1024;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wsrc + kib * 1024),
                                             (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        }
    };

    // wave w = z plane w >> 1, y rows (w & 1) * TY/2 ..; lane = (y row, x); floats: input voxel (2z, 2y, 2x) at tap 0, quad `half`
    const int ay = (wave & 1) * (GM::TY / 2) + (l31 >> TXL), ax = l31 & (GM::TX - 1);
    const int a_base = half * BV * 4 + (((wave >> 1) * 2 * IY + ay * 2) * IX + 2 * ax) * 4;

    TileCoord cur = decode(tile);
#pragma unroll
    for (int k = 0; k < 7; ++k) dma_brick(cur, 0, k, lds);
    dma_weights(0, 0, 0);
    __syncthreads();

    int buf = 0, wslot = 0;
    for (; tile < hi; tile += nl) {
        // acc: the hi x hi products; acc_s: the five small ones (<= 2^-7 of them, so their roundings weigh 2^-7 as much) - added once
        // per tile, so an output carries one chain's roundings and not six
        f32x16 acc[1][2], acc_s[2];
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[0][nf][r] = 0.f; acc_s[nf][r] = 0.f; }
        const int ntile = tile + nl;
        const TileCoord nxt_tile = ntile < hi ? decode(ntile) : cur;

        for (int ch = 0; ch < p.nchunks; ++ch) {
            const bool last_ch = ch == p.nchunks - 1;
            const bool have_next = !last_ch || ntile < hi;
            // (without a next chunk the fetches re-stage the current one into the idle buffers: no branch in the MFMA stream)
            const TileCoord nxt = last_ch ? nxt_tile : cur;   // (nxt_tile = cur past the last tile)
            const int nch = have_next ? (last_ch ? 0 : ch + 1) : ch;
            const float *bufc = lds + buf * S2_BUF_FLOATS;
            float *bufn = lds + (buf ^ 1) * S2_BUF_FLOATS;
#pragma unroll
            for (int dz = 0; dz < 3; ++dz) {
                // Fetches of the step, oldest first: the next weight plane (7 rounds of one DMA per wave; rounds 0-3 in front of the
                // tap loop, where the wave waits for its first LDS reads anyway), then ranges of the next chunk's brick (dz 0: ranges
                // 0-3, dz 1: 4-6, dz 2: none).  The weights are read in the next step and must have landed at this step's barrier;
                // the brick is read three steps on.  A step of 60 bf16 MFMAs is shorter than a fetch from HBM takes, so the barrier
                // leaves the step's brick DMAs - the youngest, two per range - in flight (vmcnt(8), vmcnt(6)) and only dz 2, in front
                // of the buffer switch, drains them all.
                // (The waits at the step's end count on this order: exactly 2 * S2_BRICK_N brick DMAs are issued behind the 7 weight
                // DMAs of the step, and vmcnt retires in order.  A change of the schedule here changes S2_BRICK_RANGES, not a literal.)
                constexpr int S2_BRICK_RANGES[3] = {4, 3, 0};
                static_assert(S2_BRICK_RANGES[0] + S2_BRICK_RANGES[1] + S2_BRICK_RANGES[2] == 7, "a wave fetches 7 ranges of a brick");
                const int S2_BRICK_LO = dz == 0 ? 0 : S2_BRICK_RANGES[0], S2_BRICK_N = S2_BRICK_RANGES[dz];  // (dz: compile-time, the loop is unrolled)
                auto step_fetch = [&](int piece) {
                    if (piece < 7) {
                        if (dz < 2) dma_weights(ch, dz + 1, wslot ^ 1, piece, piece + 1);
                        else dma_weights(nch, 0, wslot ^ 1, piece, piece + 1);
                    } else if (piece - 7 < S2_BRICK_N) dma_brick(nxt, nch, S2_BRICK_LO + piece - 7, bufn);
                };
                // The plane's product on the bf16 matrix pipe (DESIGN.md section 5 "split-bf16").  An fp32 value is cut into three
                // bf16 pieces by truncation, v = v0 + v1 + v2 exactly (8 + 8 + 8 significant bits); the weights arrive cut (the split
                // pack), the inputs are cut here.  Six of the nine piece products are summed, smallest first, in fp32 inside the MFMA:
                //   x2 w0, x0 w2, x1 w1, x1 w0, x0 w1, x0 w0        (dropped: x1 w2, x2 w1, x2 w2, each <= 2^-24 |x w|)
                // One v_mfma_f32_32x32x16_bf16 takes K = 16 = 2 taps x 8 channels: a lane's 8 elements are its quad of tap A, then its
                // quad of tap B, in both operands.  Group 0 of a plane is tap 0 alone (the input's second half is zero, the weight's a
                // second copy of tap 0: finite), groups 1-4 are taps (1, 2) (3, 4) (5, 6) (7, 8).  The order of groups and products is
                // the same in both tile shapes and in the view twin: their outputs agree bit for bit.
                // Domain: zeros and finite values whose last bit is a normal fp32 (|v| >= 2^-103) split exactly.  A non-finite input
                // does not survive the split as itself: for +-inf the residual is inf - inf, so the output is NaN where an fp32 product
                // gave +-inf (NaN stays NaN); the same holds for a non-finite weight through the host split.
                const char *whm = (const char *)(wring + wslot * S2_WSLOT_FLOATS), *wl = (const char *)(wlo + wslot * (S2_WLO_BYTES / 4));
                auto read_a = [&](int t) {
                    const int dy = t / 3, dx = t - dy * 3;
                    return *(const f32x4 *)(bufc + a_base + ((dz * IY + dy) * IX + dx) * 4);
                };
                auto read_b = [&](int g, s2u32x4 (&b)[3][2]) {
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc)
#pragma unroll
                        for (int nf = 0; nf < 2; ++nf) {
                            const char *base = pc < 2 ? whm + pc * S2_WPIECE_BYTES : wl;
                            if (g == 0) {
                                const s2u32x2 t = *(const s2u32x2 *)(base + nf * 512 + lane * 8);
                                b[pc][nf][0] = t[0]; b[pc][nf][1] = t[1]; b[pc][nf][2] = t[0]; b[pc][nf][3] = t[1];
                            } else b[pc][nf] = *(const s2u32x4 *)(base + 1024 + (g - 1) * 2048 + nf * 1024 + lane * 16);
                        }
                };
                auto cut = [](float v) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & 0xffff0000u); };
                auto pk = [](float e0, float e1) {  // the bf16 truncations of e0 (low half) and e1 (high half)
                    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, e1), __builtin_bit_cast(unsigned, e0), 0x07060302u);
                };
                // unit u = values 2u, 2u + 1 of (tap A, tap B) -> dword u of the three pieces; 6 + 5 VALU instructions, the subtractions exact
                auto split_hi = [&](const f32x4 (&v)[2], int u, s2u32x4 (&x)[3], float (&r)[8]) {
                    const float e0 = v[u >> 1][(u & 1) * 2], e1 = v[u >> 1][(u & 1) * 2 + 1];
                    x[0][u] = pk(e0, e1);
                    r[2 * u] = e0 - cut(e0); r[2 * u + 1] = e1 - cut(e1);
                    x[1][u] = pk(r[2 * u], r[2 * u + 1]);
                };
                auto split_lo = [&](int u, s2u32x4 (&x)[3], const float (&r)[8]) {
                    x[2][u] = pk(r[2 * u] - cut(r[2 * u]), r[2 * u + 1] - cut(r[2 * u + 1]));
                };
                constexpr int PX[6] = {2, 0, 1, 1, 0, 0}, PW[6] = {0, 2, 1, 0, 1, 0};
                f32x4 ar[2], ar_n[2];
                s2u32x4 xs[3], xs_n[3], b_cur[3][2], b_nxt[3][2], b_nn[3][2];
                float rs[8];
                ar[0] = read_a(0);
                read_b(0, b_cur);
#pragma unroll
                for (int piece = 0; piece < 4; ++piece) step_fetch(piece);
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) xs[pc] = s2u32x4{0u, 0u, 0u, 0u};
                split_hi(ar, 0, xs, rs); split_hi(ar, 1, xs, rs);
                split_lo(0, xs, rs); split_lo(1, xs, rs);
                ar[0] = read_a(1); ar[1] = read_a(2);
                read_b(1, b_nxt);
                // Per MFMA gap (32 cycles, the VALU free beside it): half a unit of the next group's split behind MFMAs 1-8, the reads of
                // the group after it behind MFMA 9 - with an LDS-DMA in flight hipcc waits lgkmcnt(0), so they are waited for at the
                // next group's MFMA 1 -, one fetch piece behind MFMAs 0, 10 and 11 of groups 0-2.
#pragma unroll
                for (int g = 0; g < 5; ++g) {
#pragma unroll
                    for (int m = 0; m < 12; ++m) {
                        const int pr = m >> 1, nf = m & 1;
                        f32x16 &dst = pr == 5 ? acc[0][nf] : acc_s[nf];
                        dst = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(s2bf16x8, b_cur[PW[pr]][nf]),
                                                                      __builtin_bit_cast(s2bf16x8, xs[PX[pr]]), dst, 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        if (g < 4 && m >= 1 && m <= 8) {
                            if ((m - 1) & 1) split_lo((m - 1) >> 1, xs_n, rs);
                            else split_hi(ar, (m - 1) >> 1, xs_n, rs);
                        }
                        if (g < 3 && m == 9) {
                            ar_n[0] = read_a(2 * g + 3); ar_n[1] = read_a(2 * g + 4);
                            read_b(g + 2, b_nn);
                        }
                        if (m == 0 || m >= 10) {
                            const int piece = 4 + g * 3 + (m == 0 ? 0 : m - 9);
                            if (piece < 7 + S2_BRICK_N) step_fetch(piece);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc) {
                        if (g < 4) { xs[pc] = xs_n[pc]; b_cur[pc][0] = b_nxt[pc][0]; b_cur[pc][1] = b_nxt[pc][1]; }
                        if (g < 3) { b_nxt[pc][0] = b_nn[pc][0]; b_nxt[pc][1] = b_nn[pc][1]; }
                    }
                    if (g < 3) { ar[0] = ar_n[0]; ar[1] = ar_n[1]; }
                }
                // explicit: a ds_read is ordered behind an LDS-DMA only by the issuer's vmcnt + a barrier.  (Raw barrier: a
                // __syncthreads() would drain the brick DMAs as well.  The MFMAs above have consumed every LDS read of the step.)
                if (dz == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * S2_BRICK_RANGES[0]) : "memory");
                else if (dz == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * S2_BRICK_RANGES[1]) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");  // the other weight slot may be read now; after dz 2 the other brick buffer as well
                wslot ^= 1;
            }
            buf ^= 1;
        }
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) acc[0][nf] += acc_s[nf];
        ConvArgs q = p;
        q.lx = TXL; q.ly = 6 - TXL; q.lz = 1;  // voxel v = wave * 32 + lane: x = v & (TX-1), y = (v >> TXL) & (TY-1), z = v >> 6
        conv_epilogue<1, 2>(acc, q, cur.n, cur.oz0, cur.oy0, cur.ox0, (int)blockIdx.y * 64);
        cur = nxt_tile;
    }
}
