// Body of the training GEMM pass (train_mlp_gemm.hip: tl_gemm_kernel, and the GEMM range of train_mlp_pair.hip's tl_pair_kernel). Included as TEXT into
// the kernel that runs it, with the names in scope that it uses: NS, AMODE (compile-time), `p` (the kernel's TlGemm argument
// itself or a reference to it), PN2_BX / PN2_BY / PN2_GX (the workgroup's position in its (gx, slabs) grid and gx), PN2_STATS
// (compile-time bool: false = the "no statistics" variant of the frozen-statistics node, train_mlp_frozen.hip -- no per-tile
// sums, no sd1 / sd2 registers, no LDS reduction, no partial row; p.stats is not looked at), PN2_MASKED (compile-time bool: true =
// the rows of a ragged batch, train_mlp_ragged.hip -- the lane's row of the A operand is taken as ZERO where its bit of the
// item's validity word p.mask[item] is clear, a select behind the prologue: whatever the row holds, NaN included, never enters
// a product; a zero row gives a zero output row, adds nothing to the sums and fails E_MASK's test. false: p.mask is not looked at).
// Text, not a function: as an inlined function taking the argument struct by reference the stand-alone kernels compiled
// differently -- the struct's fields became values live from the kernel's start instead of scalar loads at their uses, and
// the weight-gradient kernels that carry the data gradient went 100-400 bytes per lane deeper into scratch.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int kpad = p.tk * 32;
    float *lp0 = reinterpret_cast<float *>(smem), *lp1 = lp0 + kpad, *lp2 = lp1 + kpad;
    u32x4 *wst = reinterpret_cast<u32x4 *>(lp2 + kpad);
    const int tid = threadIdx.x, lane = tid & 63, hl = lane >> 5, s = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);             // wave-uniform: item bases live in SGPRs
    const int slab = PN2_BY;
    constexpr int kStageV = NS * kPairVec;
    constexpr int PV = (kStageV + kTlThreads - 1) / kTlThreads;
    constexpr bool PREFZ = (AMODE == A_DZ || AMODE == A_FILL) && NS <= 2;              // prefetch the ReLU mask's source rows (E_MASK)
    // A tiles in flight ahead of the MFMAs (register budget). FOUR for the plain / ReLU prologues with narrow slabs: on a level
    // of a few thousand rows a wave is alone on its SIMD, its k loop is a chain of memory latencies (1.6 us per tile with two
    // tiles ahead: 63 us for the 40 k tiles of part_seg's FP1, 2,048 rows) and the registers of a third and fourth slot are there
    constexpr int DEPTH = AMODE >= A_DZ ? 1 : ((AMODE == A_PLAIN || AMODE == A_RELU) && NS <= 2) ? 4 : 2;
    const u32x4 *wsrc = p.wpacked + (size_t)slab * p.tk * kStageV;

    if (AMODE == A_FILL) {
        for (int i = tid; i < kpad; i += kTlThreads) {
            const int j = i - p.tk0 * 32;
            lp0[i] = i < p.K0 ? p.p0[i] : (j >= 0 && j < p.K1) ? p.q0[j] : 0.0f;
            lp1[i] = (j >= 0 && j < p.K1) ? p.q1[j] : 0.0f;
            lp2[i] = 0.0f;
        }
    } else if (AMODE >= A_RELU) {
        for (int i = tid; i < kpad; i += kTlThreads) {
            const bool in = i < p.K;
            lp0[i] = in ? p.p0[i] : 0.0f;
            lp1[i] = in ? p.p1[i] : 0.0f;
            lp2[i] = (in && AMODE >= A_DZ) ? p.p2[i] : 0.0f;
        }
    }
    if (p.resident)
        for (int i = tid; i < p.tk * kStageV; i += kTlThreads) wst[i] = wsrc[i];
    __syncthreads();

    const long long items = p.rows / 32;
    const long long rounds = (items + kTlWaves - 1) / kTlWaves;
    u32x4 pre[PV];
    if (!p.resident) {
#pragma unroll
        for (int i = 0; i < PV; ++i) {
            const int j = tid + i * kTlThreads;
            if (j < kStageV) pre[i] = wsrc[j];
        }
    }
    unsigned parity = 0;
    double sd1[NS], sd2[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) { sd1[t] = 0.0; sd2[t] = 0.0; }

    // per-column parameters of the epilogue (the lane's columns never change): fetched once -- a global load inside the
    // round loop would be waited for with vmcnt(0), which also drains the A prefetch
    float ep0[NS], ep1[NS], ep2[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int col = (slab * NS + t) * 32 + s;
        ep0[t] = 0.0f; ep1[t] = 0.0f; ep2[t] = 0.0f;
        if (col < p.N) {
            if (p.emode == E_MASK) { ep0[t] = p.ea[col]; ep1[t] = p.ec[col]; }
            else if (p.emode != E_PLAIN && p.bias) ep0[t] = p.bias[col];
            if (p.emode == E_POOL) ep1[t] = p.pool_gamma[col] >= 0.0f ? 0.0f : -0.0f;      // sign mask: the pool takes the min of z where gamma < 0
            if ((p.emode == E_MASK || p.emode == E_PLAIN) && p.bias) ep2[t] = p.bias[col];
        }
    }
    // The A operand is a STREAM of k tiles -- (round, u) in consumption order, across rounds -- and runs TWO tiles ahead of
    // the MFMAs in two register slots: these passes move 0.5-1 KB per MFMA, so what they need is bytes in flight
    // (8 KB per wave, 64 KB per CU). Gathered rows (layer 1 of an SA level) take two steps: the point index is fetched
    // when the slot is assigned, the coordinates / features it points to one step later, so neither wait is exposed.
    struct Slot { ARaw raw; RowCtx rc; long long round, row0, row; int u; bool active, valid, pending; unsigned mw; };
    auto assign = [&](Slot &sl, long long round, int u) {
        sl.round = round; sl.u = u; sl.valid = round < rounds;
        const long long item = round * kTlWaves + wave;
        sl.row0 = item * 32; sl.row = sl.row0 + s;
        sl.active = sl.valid && item < items;
        sl.rc = tl_row_ctx<AMODE>(p, sl.row, sl.active);
        sl.pending = sl.valid;
        if (PN2_MASKED) sl.mw = p.mask[sl.active ? item : 0];     // wave-uniform: a scalar load, beside the vector loads in flight
    };
    auto fetch = [&](Slot &sl) {
        if (sl.pending) tl_load_raw<AMODE>(p, sl.row0, sl.row, sl.rc, sl.u, hl, sl.active, sl.raw);
        sl.pending = false;
    };
    f32x16 acc[NS], zp[PREFZ ? NS : 1];
    auto consume = [&](Slot &sl, Slot &other) {
        if (AMODE == A_GATHER) fetch(other);                       // second step of the other slot's gather
        long long nr = other.round;                               // the step consumed after this one
        int nu = other.u;
        bool nvalid = other.valid;
        if (DEPTH == 1) {
            nu = sl.u + 1; nr = sl.round;
            if (nu >= p.tk) { nu = 0; nr += PN2_GX; }
            nvalid = nr < rounds;
        }
        const u32x4 *stage;
        if (p.resident) {
            stage = wst + (size_t)sl.u * kStageV;
        } else {
            u32x4 *dst = wst + (parity & 1u) * kStageV;
#pragma unroll
            for (int i = 0; i < PV; ++i) {
                const int j = tid + i * kTlThreads;
                if (j < kStageV) dst[j] = pre[i];
            }
            __syncthreads();
            if (nvalid) {                                          // the next step's weights
                const u32x4 *nsrc = wsrc + (size_t)nu * kStageV;
#pragma unroll
                for (int i = 0; i < PV; ++i) {
                    const int j = tid + i * kTlThreads;
                    if (j < kStageV) pre[i] = nsrc[j];
                }
            }
            stage = dst;
            ++parity;
        }
        if (sl.u == 0) {
#pragma unroll
            for (int t = 0; t < NS; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[t][v] = 0.0f;
        }
        f32x16 xa = tl_finish<AMODE>(sl.raw, sl.rc, sl.u, p.tk0, hl, lp0, lp1, lp2);
        if (PN2_MASKED) {                                          // a padding row is absent: h = 0 / dz = 0, by a select
            const bool rv = (sl.mw >> s) & 1u;
#pragma unroll
            for (int v = 0; v < 16; ++v) xa[v] = rv ? xa[v] : 0.0f;
        }
        const ActSplit sp = split_act(xa);
        const bool last = sl.u + 1 == p.tk;
        const long long erow0 = sl.row0, eitem = sl.round * kTlWaves + wave;
        const bool eactive = sl.active;
        if (PREFZ && last && p.emode == E_MASK && eactive) {        // the mask's source rows, under the last tile's MFMAs
            const rsrc_t rz = make_rsrc(p.zprev + (size_t)erow0 * p.N, 32u * (unsigned)p.N * 4u);
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                const int col = (slab * NS + t) * 32 + s;
                if (col < p.N) {
#pragma unroll
                    for (int v = 0; v < 16; ++v)
                        zp[t][v] = bload(rz, (4 * hl * p.N + col) * 4, (8 * (v >> 2) + (v & 3)) * p.N * 4);
                }
            }
        }
        {                                                          // this slot: the tile DEPTH steps ahead
            long long r2 = nr;
            int u2 = nu;
            if (DEPTH >= 2) {
                u2 = nu + DEPTH - 1;
                while (u2 >= p.tk) { u2 -= p.tk; r2 += PN2_GX; }
            }
            if (nvalid) assign(sl, r2, u2); else sl.valid = false;
            if ((AMODE != A_GATHER || DEPTH == 1) && sl.valid) fetch(sl);
        }
#pragma unroll
        for (int t = 0; t < NS; ++t) acc[t] = stream_pair<true>(stage, t, lane, sp, acc[t]);
        if (!last) return;
        // ---- epilogue: lane = column 32(slab NS + t) + s, register v = row row0 + mlp_chan(v, hl) ----------------------
        // buffer addressing: descriptor at the item's first row, lane offset = (4 hl) rows + its column, uniform offset = the
        // register's row 8(v >> 2) + (v & 3)
        const unsigned obytes = 32u * (unsigned)p.N * 4u;
        const rsrc_t ro = make_rsrc(p.emode == E_PLAIN ? nullptr : p.out + (size_t)erow0 * p.N, p.emode == E_PLAIN ? 0u : obytes);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int col = (slab * NS + t) * 32 + s;
            const bool ok = eactive && col < p.N;
            const int voff = (4 * hl * p.N + col) * 4;
            if (p.emode == E_STORE || p.emode == E_POOL) {
                // (no bias: the pre-norm tensors are stored without it, pn2_mlp_train_forward; ep0 is 0 in these modes)
                float s1 = 0.0f, s2 = 0.0f;
                const f32x16 &val = acc[t];
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    s1 = __fadd_rn(s1, val[v]);
                    s2 = fmaf(val[v], val[v], s2);
                }
                if (PN2_STATS && ok && !(p.lab & 2)) {
                    sd1[t] += (double)s1;
                    sd2[t] += (double)s2;
                }
                if (ok && !(p.lab & 1) && p.out) {
                    if (p.nt) {
#pragma unroll
                        for (int v = 0; v < 16; ++v) bstore<true>(val[v], ro, voff, (8 * (v >> 2) + (v & 3)) * p.N * 4);
                    } else {
#pragma unroll
                        for (int v = 0; v < 16; ++v) bstore<false>(val[v], ro, voff, (8 * (v >> 2) + (v & 3)) * p.N * 4);
                    }
                }
                if (p.emode == E_POOL) {
                    // The extremum of z over the rows of the item that the pool will select -- of each half item when a group is
                    // 16 rows: registers 0-7 hold rows 0-15, registers 8-15 rows 16-31 -- with the row number of its FIRST
                    // occurrence; the other half of the rows lives in lane l ^ 32. Which extremum is known at launch: batch
                    // norm + ReLU are monotone per channel, increasing where gamma >= 0 (max), decreasing where gamma < 0 (min
                    // = max of -z: one sign flip per value instead of a second compare / select chain and a second pair of
                    // partial arrays). Fully unrolled: a runtime-indexed register array would live in scratch.
                    const unsigned sgn = __float_as_uint(ep1[t]);
                    float mx[2];
                    int ax[2];
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        mx[hf] = __uint_as_float(__float_as_uint(val[8 * hf]) ^ sgn); ax[hf] = 8 * hf;
#pragma unroll
                        for (int v = 8 * hf + 1; v < 8 * hf + 8; ++v) {
                            const float q = __uint_as_float(__float_as_uint(val[v]) ^ sgn);
                            if (q > mx[hf]) { mx[hf] = q; ax[hf] = v; }
                        }
                    }
                    if (p.prow != 16) {                            // one group: registers 8-15 come after 0-7 in row order
                        if (mx[1] > mx[0]) { mx[0] = mx[1]; ax[0] = ax[1]; }
                    }
                    const int halves = p.prow == 16 ? 2 : 1;
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        if (hf < halves) {
                            float bx = mx[hf];
                            int rx = mlp_chan(ax[hf], hl);
                            const float omx = __shfl_xor(bx, 32);
                            const int orx = __shfl_xor(rx, 32);
                            if (omx > bx || (omx == bx && orx < rx)) { bx = omx; rx = orx; }
                            if (ok && hl == 0) {
                                const size_t o = (size_t)(eitem * halves + hf) * p.N + col;
                                p.pmax[o] = __uint_as_float(__float_as_uint(bx) ^ sgn);
                                p.pamax[o] = rx - hf * 16;
                            }
                        }
                    }
                }
            } else if (p.emode == E_MASK) {
                const float ea = ep0[t], ec = ep1[t];
                float s1 = 0.0f, s2 = 0.0f;
                if (ok) {
                    if (!PREFZ) {                                  // wide slabs: no registers to spare, fetched here
                        const rsrc_t rz = make_rsrc(p.zprev + (size_t)erow0 * p.N, obytes);
#pragma unroll
                        for (int v = 0; v < 16; ++v) zp[0][v] = bload(rz, voff, (8 * (v >> 2) + (v & 3)) * p.N * 4);
                    }
                    const f32x16 &zz = zp[PREFZ ? t : 0];
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const float y = __fadd_rn(__fmul_rn(ea, zz[v]), ec);
                        const float g = y > 0.0f ? __fadd_rn(acc[t][v], ep2[t]) : 0.0f;   // ReLU of the layer below
                        if (p.nt) bstore<true>(g, ro, voff, (8 * (v >> 2) + (v & 3)) * p.N * 4);
                        else bstore<false>(g, ro, voff, (8 * (v >> 2) + (v & 3)) * p.N * 4);
                        if (PN2_STATS) {
                            s1 = __fadd_rn(s1, g);
                            s2 = fmaf(g, zz[v], s2);
                        }
                    }
                    if (PN2_STATS) {
                        sd1[t] += (double)s1;
                        sd2[t] += (double)s2;
                    }
                }
            } else {
                if (eactive && col >= p.col0 && col < p.col1) {
#pragma unroll
                    for (int v = 0; v < 16; ++v)
                        p.out[(size_t)(erow0 + mlp_chan(v, hl)) * p.out_pitch + (col - p.col0)] = __fadd_rn(acc[t][v], ep2[t]);
                }
            }
        }
    };
    Slot s0;
    assign(s0, PN2_BX, 0);
    fetch(s0);
    if (DEPTH == 4) {
        Slot s1, s2, s3;
        auto after = [&](const Slot &a, Slot &b) __attribute__((always_inline)) {       // b <- the step after a, its loads issued
            long long r = a.round;
            int u = a.u + 1;
            if (u >= p.tk) { u = 0; r += PN2_GX; }
            if (a.valid) assign(b, r, u); else b.valid = false;
            if (b.valid) fetch(b);
        };
        after(s0, s1);
        after(s1, s2);
        after(s2, s3);
        while (s0.valid) {
            consume(s0, s1);
            if (!s1.valid) break;
            consume(s1, s2);
            if (!s2.valid) break;
            consume(s2, s3);
            if (!s3.valid) break;
            consume(s3, s0);
        }
    } else if (DEPTH == 2) {
        Slot s1;
        long long r1 = PN2_BX;
        int u1 = 1;
        if (u1 >= p.tk) { u1 = 0; r1 += PN2_GX; }
        if (s0.valid) assign(s1, r1, u1); else s1.valid = false;
        if (s1.valid) fetch(s1);
        while (s0.valid) {
            consume(s0, s1);
            if (!s1.valid) break;
            consume(s1, s0);
        }
    } else {
        while (s0.valid) consume(s0, s0);
    }
    if (PN2_STATS && p.emode != E_PLAIN && p.stats) {
        // per-channel sums of this workgroup's rows: the eight waves' partial sums meet in LDS and leave as ONE row of the
        // (row workgroups, 2, N) partial array -- no atomics (2048 waves adding into the same 2N addresses serialise in the
        // L2 for ~100 us per pass), and the finalisation kernel adds the rows in a fixed order
        __syncthreads();                                           // the weight stages are dead: reuse their LDS
        double *red = reinterpret_cast<double *>(smem);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const double d1 = sd1[t] + __shfl_xor(sd1[t], 32), d2 = sd2[t] + __shfl_xor(sd2[t], 32);
            if (hl == 0) {
                red[(wave * 2 + 0) * (NS * 32) + t * 32 + s] = d1;
                red[(wave * 2 + 1) * (NS * 32) + t * 32 + s] = d2;
            }
        }
        __syncthreads();
        if (tid < 2 * NS * 32) {
            const int which = tid / (NS * 32), c = tid % (NS * 32), col = slab * NS * 32 + c;
            double sum = 0.0;
#pragma unroll
            for (int w = 0; w < kTlWaves; ++w) sum += red[(w * 2 + which) * (NS * 32) + c];
            if (col < p.N) {
                double *dst = p.stats + ((size_t)PN2_BX * 2 + which) * p.N + col;
                if (p.fin.ticket) tl_fin_store(dst, sum); else *dst = sum;      // folded finalisation: write-through (TlFin)
            }
        }
        // the finalisation of these sums, by the workgroup of this pass that finishes last (TlFin, train_mlp_kernels.h; tl_fin_tail, train_mlp_device.h)
        if (p.fin.ticket) tl_fin_tail<kTlThreads>(p.fin, smem);
    }
