// Body of the weight-gradient pass (train_mlp_wgrad.hip: tl_wgrad_kernel, and the weight-gradient range of train_mlp_pair.hip's tl_pair_kernel).
// Included as TEXT (see tl_gemm_body.inc) with TPW, UPW, GATHER, DCLS, DY, L1X (compile-time), `p` (the TlWgrad argument) and
// PN2_BX / PN2_BY / PN2_GX in scope, and PN2_MASKED (compile-time bool: true = the rows of a ragged batch, train_mlp_ragged.hip:
// the validity word p.mask[block] travels two blocks ahead like the unit loads -- a scalar load, so the vector loads keep their
// one instruction sequence -- and wg_store_unit<.., true> zeroes the padding rows of both operands; false: p.mask is not looked at).
// The masked text is taken in and out by the PREPROCESSOR (PN2_MW_*), not by an `if` on a constant: with the word as one more
// reference parameter of the lambdas below, two of tl_pair_kernel's dense instantiations went 16-20 bytes per lane deeper into
// scratch, although nothing read it.
#if PN2_MASKED
#define PN2_MW_PARAM , unsigned &mw
#define PN2_MW_ARG(X) , X
#define PN2_MW_LOAD(INB, B) mw = p.mask[(INB) ? (B) : 0];
#define PN2_MW_STORE(I) wg_store_unit<DCLS, true>(un[I], r[I], lane, img, zr, zpitch, imgA, p.tus, mw)
#else
#define PN2_MW_PARAM
#define PN2_MW_ARG(X)
#define PN2_MW_LOAD(INB, B)
#define PN2_MW_STORE(I) wg_store_unit<DCLS>(un[I], r[I], lane, img, zr, zpitch, imgA, p.tus)
#endif
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // uniform: scalar branches
    const int us = PN2_BY / p.tslabs, ts = PN2_BY % p.tslabs;
    const int ntiles = p.tus + p.tts, nunits = 2 * ntiles, nout = p.tus * p.tts;
    const int imgv = ntiles * 3 * 2 * 64;                           // 16-byte vectors of one block image
    u32x4 *img0 = reinterpret_cast<u32x4 *>(smem);
    u32x4 *img1 = (DY && p.single) ? img0 : img0 + imgv;
    const long long blocks = p.rows / 32, step = PN2_GX;
    f32x16 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.0f;
    WgRaw ra[UPW], rb[UPW];
#if PN2_MASKED
    unsigned mwa = 0u, mwb = 0u;
#endif
    WgUnit un[UPW];
    // (measured: taking the unit loads away from the waves that produce the data gradient -- the block's critical path --
    // made the pass slower, 286 -> 306 us at the metric shape: the other waves' second unit costs more than it frees)
#pragma unroll
    for (int i = 0; i < UPW; ++i) un[i] = wg_plan_unit(p, wave + 8 * i, nunits, us, ts, lane);
    // output tiles of this wave: image slots of their two operands (fixed)
    int xa_off[TPW], xb_off[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int q = wave + 8 * i, u = q < nout ? q / p.tts : 0, t = q < nout ? q % p.tts : 0, tg = ts * p.tts + t;
        const bool shared = p.dmode == A_FILL && p.xshare && tg >= p.tf && tg < p.tf + p.tus;
        xa_off[i] = u * 384;
        xb_off[i] = (shared ? tg - p.tf : p.tus + t) * 384;
    }
    const int sw0 = wg_swz(lane, 0), sw1 = 64 + wg_swz(lane, 1);     // lane's fragment of K16 step 0 / 1 inside a (tile, level)
    const int grows = p.group_rows > 0 ? p.group_rows : 32;
    // ---- data-gradient role: the LAST dy_nt waves take one output tile each (they own the fewest dW tiles)
    const int dyt = DY ? uni(7 - wave < p.dy_nt ? 7 - wave : -1) : -1;
    const u32x4 *wl = img0 + (size_t)((DY && p.single) ? 1 : 2) * imgv;      // packed W^T, resident
    const int zpitch = p.tus * 32 + 2;                             // raw rows of the layer below: 8 rows apart = 16 banks apart
    float *zr0 = DY ? reinterpret_cast<float *>(const_cast<u32x4 *>(wl) + (size_t)p.dy_tk * p.dy_nt * kPairVec) : nullptr;
    float *zr1 = (DY && !p.single) ? zr0 + 32 * zpitch : zr0;
    u32x4 *ia0 = (DY && p.dy_acopy) ? reinterpret_cast<u32x4 *>(zr0 + (size_t)(p.single ? 1 : 2) * 32 * zpitch) : nullptr;
    u32x4 *ia1 = (DY && p.dy_acopy && !p.single) ? ia0 + (size_t)p.dy_tk * 384 : ia0;
    // centred coordinates of the block's rows (l1x): two blocks ahead in registers like the units, 32 x 16 bytes per image
    float4 *xr0 = DY ? reinterpret_cast<float4 *>(reinterpret_cast<char *>(smem) + p.xr_off) : nullptr;
    float4 *xr1 = (DY && !p.single) ? xr0 + 32 : xr0;
    float4 xpa = {0.f, 0.f, 0.f, 0.f}, xpb = {0.f, 0.f, 0.f, 0.f};
    double sda[3] = {0.0, 0.0, 0.0};
    double sd1 = 0.0, sd2 = 0.0;
    // transposed reads: lane = row r of the block = fragment slot (e_r, half hl_r, j_r) of the image; its eight values of a
    // K16 step are slots of eight channels' fragments: byte address = tile * 6144 + level * 2048 + 256 * (K16 step) + tb + 16 (j ^ sg)
    int tb = 0, sg16 = 0, sa0 = 0, sa1 = 0;
    if (DY) {
        const int r = lane & 31, g = lane >> 5, er = r >> 4, hr = (r >> 3) & 1, jr = r & 7;
        tb = er * 1024 + (8 * g + 32 * hr) * 16 + jr * 2;
        sg16 = (g | (hr << 1) | (er << 2)) << 4;
        sa0 = lane ^ (g | (hr << 1));                              // lane's fragment of K16 step 0 / 1 in the A-layout copy
        sa1 = 64 + (lane ^ (g | (hr << 1) | 4));
    }
    float dy_ea = 0.0f, dy_ec = 0.0f, dy_b = 0.0f;
    if (DY && dyt >= 0) {
        const int col = dyt * 32 + (lane & 31);
        dy_ec = 1.0f;                                              // no mask: y = 0 * z + 1 > 0
        if (col < p.dy_cols) {
            if (p.dy_zprev) { dy_ea = p.dy_ea[col]; dy_ec = p.dy_ec[col]; }
            if (p.dy_bias) dy_b = p.dy_bias[col];
        }
    }
    if (DY) {
        u32x4 *wdst = const_cast<u32x4 *>(wl);
        const int nv = p.dy_tk * p.dy_nt * kPairVec;
        for (int i = threadIdx.x; i < nv; i += kTlThreads) wdst[i] = p.dy_w[i];
        // the raw rows are only written when the first operand goes through a ReLU (a masked pass); an unmasked pass reads them
        // too (times zero): defined values
        const int nz = (p.single ? 1 : 2) * 32 * zpitch;
        for (int i = threadIdx.x; i < nz; i += kTlThreads) zr0[i] = 0.0f;
    }
    auto load = [&](long long b, WgRaw (&r)[UPW] PN2_MW_PARAM) __attribute__((always_inline)) {   // the same instruction sequence for every wave and block
        const bool inb = b < blocks;
        PN2_MW_LOAD(inb, b)
        const long long row0 = (inb ? b : 0) * 32;
        const int grp_u = (int)((unsigned)row0 / (unsigned)grows), off_u = (int)row0 - grp_u * grows;
#pragma unroll
        for (int i = 0; i < UPW; ++i) wg_load_unit<GATHER, DCLS>(p, un[i], row0, grp_u, off_u, lane, inb, r[i]);
    };
    auto tiles_of_wave = [&](const u32x4 *img) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            if (wave + 8 * i < nout) {
                const u32x4 *xa = img + xa_off[i], *xb = img + xb_off[i];
                {
                    const u32x4 a[3] = {xa[sw0], xa[128 + sw0], xa[256 + sw0]};
                    const u32x4 d[3] = {xb[sw0], xb[128 + sw0], xb[256 + sw0]};
                    acc[i] = mma_x6<false>(a, d, acc[i]);
                }
                {
                    const u32x4 a[3] = {xa[sw1], xa[128 + sw1], xa[256 + sw1]};
                    const u32x4 d[3] = {xb[sw1], xb[128 + sw1], xb[256 + sw1]};
                    acc[i] = mma_x6<false>(a, d, acc[i]);
                }
            }
        }
    };
    // ROLE = 1: this wave also produces tile dyt of the data gradient
#ifdef PN2_WG_TIMING
    unsigned long long tph[6] = {0, 0, 0, 0, 0, 0}, tlast = __builtin_readcyclecounter();
#define PN2_TICK(K) { const unsigned long long tnow = __builtin_readcyclecounter(); tph[K] += tnow - tlast; tlast = tnow; }
#else
#define PN2_TICK(K)
#endif
    auto xload = [&](long long b) __attribute__((always_inline)) {      // rows of block b (an empty descriptor when there are none: no branch)
        const bool inb = b < blocks && p.l1x != nullptr;
        const rsrc_t rx = make_rsrc(inb ? p.l1x + (size_t)b * 32 : nullptr, inb ? 512u : 0u);
        return bload4(rx, (lane & 31) * 16, 0);
    };
    auto block = [&](long long b, WgRaw (&r)[UPW] PN2_MW_PARAM, u32x4 *img, float *zr, u32x4 *imgA, float4 *xr, float4 &xp, auto role) __attribute__((always_inline)) {
        constexpr bool ROLE = decltype(role)::value;
        PN2_TICK(5)
#pragma unroll
        for (int i = 0; i < UPW; ++i) PN2_MW_STORE(i);
        if (L1X && ROLE && dyt == 0 && lane < 32) xr[lane] = xp;
        PN2_TICK(0)
        __syncthreads();
        PN2_TICK(1)
        const int hl = lane >> 5, col = dyt * 32 + (lane & 31);
        const int voff = (ROLE && col < p.dy_cols) ? (4 * hl * p.dy_pitch + col) * 4 : kWgOob;
        const int rstep = uni(p.dy_pitch * 4);
        load(b + 2 * step, r PN2_MW_ARG(mw));
        if (L1X && ROLE && dyt == 0) xp = xload(b + 2 * step);
        tiles_of_wave(img);
        PN2_TICK(2)
        if (ROLE) {
            f32x16 d;
#pragma unroll
            for (int v = 0; v < 16; ++v) d[v] = 0.0f;
            const char *ib = reinterpret_cast<const char *>(img) + tb;
            if (DCLS != D_TOP && imgA) {
                // A operand straight from the producers' A-layout copy
                for (int u = 0; u < p.dy_tk; ++u) {
                    const u32x4 *ta = imgA + (size_t)u * 384;
                    ActSplit sp;
#pragma unroll
                    for (int lv = 0; lv < 3; ++lv) {
                        sp.p[0][lv] = ta[lv * 128 + sa0];
                        sp.p[1][lv] = ta[lv * 128 + sa1];
                    }
                    d = stream_pair<true>(wl + (size_t)u * p.dy_nt * kPairVec, dyt, lane, sp, d);
                }
            } else {
                // A operand = the weight gradient's image read transposed (eight 2-byte reads per fragment)
                for (int u = 0; u < p.dy_tk; ++u) {
                    const int it = (DCLS == D_TOP && p.xshare && u >= p.dy_tf) ? u - p.dy_tf : p.tus + u;
                    const char *tp = ib + (size_t)it * 6144;
                    ActSplit sp;
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int lv = 0; lv < 3; ++lv) {
                            const char *q = tp + lv * 2048 + e * 256;
                            unsigned h[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j) h[j] = *reinterpret_cast<const unsigned short *>(q + ((j << 4) ^ sg16));
                            u32x4 f = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
                            sp.p[e][lv] = f;
                        }
                    d = stream_pair<true>(wl + (size_t)u * p.dy_nt * kPairVec, dyt, lane, sp, d);
                }
            }
            PN2_TICK(3)
            // epilogue of the data-gradient GEMM: lane = column, register v = row 8 (v >> 2) + 4 hl + (v & 3). Branch-free:
            // every row of the layer below is read from LDS up front (one wait), an unmasked pass multiplies it by zero
            // (dy_out == nullptr: an empty descriptor -- the stores below are issued and dropped, the instruction stream stays the same)
            const rsrc_t ro = make_rsrc(p.dy_out ? p.dy_out + (size_t)b * 32 * p.dy_pitch : nullptr,
                                        p.dy_out ? 32u * (unsigned)p.dy_pitch * 4u : 0u);
            f32x16 zz;
            {
                const float *zs = zr + 4 * hl * zpitch + dyt * 32 + (lane & 31);
#pragma unroll
                for (int v = 0; v < 16; ++v) zz[v] = zs[(8 * (v >> 2) + (v & 3)) * zpitch];
            }
            float s1 = 0.0f, s2 = 0.0f;
            f32x16 gv;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float y = __fadd_rn(__fmul_rn(dy_ea, zz[v]), dy_ec);        // unmasked pass: ea = 0, ec = 1
                const float g = y > 0.0f ? __fadd_rn(d[v], dy_b) : 0.0f;         // ReLU of the layer below
                gv[v] = g;
                s1 = __fadd_rn(s1, g);
                s2 = fmaf(g, zz[v], s2);
            }
            if (L1X) {
                // layer 1 below has the three coordinates as its input: dy's product with the rows' coordinates is what its
                // weight gradient needs (see TlWgrad::l1x); dy itself is not written
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float4 xv = xr[8 * (v >> 2) + 4 * hl + (v & 3)];      // the same address in 32 lanes: LDS broadcast
                    a0 = fmaf(xv.x, gv[v], a0);
                    a1 = fmaf(xv.y, gv[v], a1);
                    a2 = fmaf(xv.z, gv[v], a2);
                }
                if (voff != kWgOob) { sda[0] += (double)a0; sda[1] += (double)a1; sda[2] += (double)a2; }
            }
            if (L1X) {
            } else if (p.dy_nt_store) {
#pragma unroll
                for (int v = 0; v < 16; ++v) bstore<true>(gv[v], ro, voff, (8 * (v >> 2) + (v & 3)) * rstep);
            } else {
#pragma unroll
                for (int v = 0; v < 16; ++v) bstore<false>(gv[v], ro, voff, (8 * (v >> 2) + (v & 3)) * rstep);
            }
            if (voff != kWgOob) {
                sd1 += (double)s1;
                sd2 += (double)s2;
            }
            PN2_TICK(4)
        }
        if (DY && p.single) __syncthreads();                       // the one image is rewritten by the next block
    };
    if (DCLS == D_TOP) {
        // the column of ones (sum over the rows of h): fragment slot j of lanes with c == 0 is bf16 1.0 at level 1, constant
#pragma unroll
        for (int i = 0; i < UPW; ++i) {
            if (un[i].kind == K_ONES) {
                const unsigned one2 = (lane & 31) == 0 ? 0x3f803f80u : 0u;
                const u32x4 ones = {one2, one2, one2, one2}, zero = {0u, 0u, 0u, 0u};
                for (int b = 0; b < 2; ++b) {
                    u32x4 *o = (b ? img1 : img0) + ((size_t)un[i].tile * 3 * 2 + un[i].e) * 64 + wg_swz(lane, un[i].e);
                    o[0] = ones; o[128] = zero; o[256] = zero;
                }
            }
        }
    }
    long long blk = PN2_BX;
    load(blk, ra PN2_MW_ARG(mwa));
    load(blk + step, rb PN2_MW_ARG(mwb));
    if (L1X && DY && dyt == 0) { xpa = xload(blk); xpb = xload(blk + step); }
    auto run = [&](auto role) __attribute__((always_inline)) {
        for (; blk < blocks; blk += 2 * step) {
            block(blk, ra PN2_MW_ARG(mwa), img0, zr0, ia0, xr0, xpa, role);
            if (blk + step < blocks) block(blk + step, rb PN2_MW_ARG(mwb), img1, zr1, ia1, xr1, xpb, role);      // uniform over the workgroup
        }
    };
    if (DY && dyt >= 0) run(std::true_type{}); else run(std::false_type{});
#ifdef PN2_WG_TIMING
    if (p.timing && PN2_BX == 0 && PN2_BY == 0 && lane == 0)
        for (int k = 0; k < 6; ++k) p.timing[wave * 6 + k] = tph[k];
#endif
    if (DY && dyt >= 0 && p.dy_stats) {
        // per-channel sums of this workgroup's rows: ONE row of the (workgroups, 2, pitch) partial array, summed in a fixed
        // order by the finalisation kernel
        const int col = dyt * 32 + (lane & 31);
        const double d1 = sd1 + __shfl_xor(sd1, 32), d2 = sd2 + __shfl_xor(sd2, 32);
        if (lane < 32 && col < p.dy_cols) {
            p.dy_stats[((size_t)PN2_BX * 2 + 0) * p.dy_pitch + col] = d1;
            p.dy_stats[((size_t)PN2_BX * 2 + 1) * p.dy_pitch + col] = d2;
        }
    }
    if (L1X && DY && dyt >= 0 && p.l1a) {
        const int col = dyt * 32 + (lane & 31);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = sda[k] + __shfl_xor(sda[k], 32);
            if (lane < 32 && col < p.dy_cols) p.l1a[((size_t)PN2_BX * 3 + k) * p.dy_pitch + col] = a;
        }
    }
    // dump: D[i = input channel mlp_chan(v, hl)][j = output channel lane & 31] of tile (u, t); one slab per WORKGROUP
    float4 *dst = reinterpret_cast<float4 *>(p.partial) + ((size_t)PN2_BY * PN2_GX + PN2_BX) * nout * 256;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int q = wave + 8 * i;
        if (q < nout) {
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const float4 o = {acc[i][4 * v4], acc[i][4 * v4 + 1], acc[i][4 * v4 + 2], acc[i][4 * v4 + 3]};
                dst[(size_t)q * 256 + v4 * 64 + lane] = o;
            }
        }
    }
#undef PN2_MW_PARAM
#undef PN2_MW_ARG
#undef PN2_MW_LOAD
#undef PN2_MW_STORE
