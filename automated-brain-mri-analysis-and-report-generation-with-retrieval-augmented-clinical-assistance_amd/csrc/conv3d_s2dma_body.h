// The body of conv3_f32_s2dma_kernel, included by conv3d.hip twice: S2DMA_VIEW = 0 is the kernel as it always was, token for token
// (its listing does not change when the view code below does); S2DMA_VIEW = 1 is conv3_f32_s2dma_kernel_view, which reads its input
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
    // weight DMA: dz plane `dz` of chunk `ch` = 18 KiB contiguous in the pack; KiB i goes to wave i & 3
    const float *wblk = p.wp + (size_t)blockIdx.y * p.nchunks * (27 * 2 * 256);
    auto dma_weights = [&](int ch, int dz, float *slot, int i_lo = 0, int i_hi = 5) {
        const float *wsrc = wblk + ((size_t)ch * 27 + dz * 9) * (2 * 256) + lane * 4;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            if (i < i_lo || i >= i_hi) continue;  // (compile-time at the call sites)
            // (no branch: KiB 18 and 19 do not exist - waves 2 and 3 fetch KiB 16 and 17 a second time in the last round,
            //  the same bytes into the same slot as waves 0 and 1)
            const int kib = wave + 4 * i < 18 ? wave + 4 * i : wave + 4 * i - 2;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wsrc + kib * 256),
                                             (__attribute__((address_space(3))) void *)(slot + kib * 256), 16, 0, 0);
        }
    };

    // wave w = z plane w >> 1, y rows (w & 1) * TY/2 ..; lane = (y row, x); floats: input voxel (2z, 2y, 2x) at tap 0, quad `half`
    const int ay = (wave & 1) * (GM::TY / 2) + (l31 >> TXL), ax = l31 & (GM::TX - 1);
    const int a_base = half * BV * 4 + (((wave >> 1) * 2 * IY + ay * 2) * IX + 2 * ax) * 4;

    TileCoord cur = decode(tile);
#pragma unroll
    for (int k = 0; k < 7; ++k) dma_brick(cur, 0, k, lds);
    dma_weights(0, 0, wring);
    __syncthreads();

    int buf = 0, wslot = 0;
    for (; tile < hi; tile += nl) {
        f32x16 acc[1][2];
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][nf][r] = 0.f;
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
                // fetches of the step: the next weight plane and a third of the next chunk's brick - issued from inside the tap loop
                // (round 4: in front of it, their ~11 DMAs and address arithmetic ran with the matrix pipe idle, once per step)
                auto step_fetch = [&](int piece) {
                    if (piece < 2) {  // the weight plane's 18 KiB: rounds 0-1, then 2-4
                        const int lo = piece == 0 ? 0 : 2, hi = piece == 0 ? 2 : 5;
                        if (dz < 2) dma_weights(ch, dz + 1, wring + (wslot ^ 1) * S2_WSLOT_FLOATS, lo, hi);
                        else dma_weights(nch, 0, wring + (wslot ^ 1) * S2_WSLOT_FLOATS, lo, hi);
                    } else {
                        const int q = piece - 1;
                        const int k = dz == 0 ? q - 1 : (dz == 1 ? 2 + q : 4 + q);   // dz 0: ranges 0 1 2, dz 1: 3 4, dz 2: 5 6
                        if (q <= (dz == 0 ? 3 : 2)) dma_brick(nxt, nch, k, bufn);
                    }
                };
                const float *wcur = wring + wslot * S2_WSLOT_FLOATS + lane * 4;
                f32x4 a_cur, a_nxt, b_cur[2], b_nxt[2];
                a_cur = *(const f32x4 *)(bufc + a_base + dz * IY * IX * 4);
                b_cur[0] = *(const f32x4 *)(wcur);
                b_cur[1] = *(const f32x4 *)(wcur + 256);
                // The next tap's fragments are read BEHIND the first two MFMAs of this tap (round 4).  With an LDS-DMA in flight hipcc
                // does not count LDS reads (every wait is lgkmcnt(0)): read at the top of the tap, as before, the three reads
                // were waited for on the spot - their latency exposed nine times a step, which is what kept this kernel's matrix
                // pipe at 0.72.  Now the wait comes in front of the NEXT tap's first MFMA, six MFMAs later.
#pragma unroll
                for (int t = 0; t < 9; ++t) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int nf = 0; nf < 2; ++nf) {
                            acc[0][nf] = __builtin_amdgcn_mfma_f32_32x32x2f32(b_cur[nf][j], a_cur[j], acc[0][nf], 0, 0, 0);
                            if (j == 0 && nf == 1) {
                                __builtin_amdgcn_sched_barrier(0);
                                if (t + 1 < 9) {
                                    const int dy = (t + 1) / 3, dx = (t + 1) - dy * 3;
                                    a_nxt = *(const f32x4 *)(bufc + a_base + ((dz * IY + dy) * IX + dx) * 4);
                                    b_nxt[0] = *(const f32x4 *)(wcur + (t + 1) * 512);
                                    b_nxt[1] = *(const f32x4 *)(wcur + (t + 1) * 512 + 256);
                                }
                                if (t < 5) step_fetch(t);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    a_cur = a_nxt; b_cur[0] = b_nxt[0]; b_cur[1] = b_nxt[1];
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // explicit: a ds_read is ordered behind an LDS-DMA only by the issuer's vmcnt + a barrier
                __syncthreads();  // retires the step's DMAs (vmcnt(0)); the other weight slot / brick buffer may be read now
                wslot ^= 1;
            }
            buf ^= 1;
        }
        ConvArgs q = p;
        q.lx = TXL; q.ly = 6 - TXL; q.lz = 1;  // voxel v = wave * 32 + lane: x = v & (TX-1), y = (v >> TXL) & (TY-1), z = v >> 6
        conv_epilogue<1, 2>(acc, q, cur.n, cur.oz0, cur.oy0, cur.ox0, (int)blockIdx.y * 64);
        cur = nxt_tile;
    }
}
