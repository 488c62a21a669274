// Body of gemm144l_dma_kernel / gemm144l64_dma_kernel (gemm.hip): included inside a kernel that declares DT, EPI, the PRIMX_GEMM_PARAMS
// arguments and TILE_ROWS = 128 or 64 (the tile's rows; the eight compute waves are 2 K groups x 4 row groups of TILE_ROWS / 4 rows).
    PRIMX_GEMM_ARGS(DT);
    unsigned long long pr0 = 0, pc0 = 0, pc1 = 0, pc2 = 0, pc_stg = 0, pc_iss = 0;   // PRIMX_GEMM_PROF=1 timeline of compute wave 0 (see g_gemm_prof)
    if (pl_prof) { pr0 = __builtin_amdgcn_s_memrealtime(); pc0 = __builtin_readcyclecounter(); }
    static_assert(EPI == EPI_LINEAR || EPI == EPI_GATE_RESIDUAL || EPI == EPI_HEADS || EPI == EPI_GATE_RESIDUAL_LN ||
                  EPI == EPI_GATE_RESIDUAL_FOLD || EPI == EPI_HEADS_FOLD || EPI == EPI_LINEAR_FOLD || EPI == EPI_F32OUT,
                  "row-major epilogues only");
    constexpr bool GATE_RES = EPI == EPI_GATE_RESIDUAL || EPI == EPI_GATE_RESIDUAL_LN || EPI == EPI_GATE_RESIDUAL_FOLD;
    constexpr bool HEADS = EPI == EPI_HEADS || EPI == EPI_HEADS_FOLD;
    constexpr bool FOLD_P = EPI == EPI_GATE_RESIDUAL_FOLD;                          // producer of a folded LayerNorm site
    constexpr bool FOLD_C = EPI == EPI_HEADS_FOLD || EPI == EPI_LINEAR_FOLD;        // consumer
    using S = typename T16<DT>::S;
    using V8 = typename T16<DT>::V8;
    using V4e = typename T16<DT>::V4;
    typedef __attribute__((address_space(1))) const void GV;
    typedef __attribute__((address_space(3))) void LV;
    constexpr int BM = TILE_ROWS, BN = 144, MI = BM / 64, NI = 9, NST = 3;   // (4 stages fit and measured no better, also with cold weights in the step: 9.31 -> 9.36 ms)
    constexpr int ROWS = BM + BN, STAGE = ROWS * 64, NINST = ROWS / 8, NL = NINST / 2;   // 17 wave-instructions per loader per tile (13 at 64 rows)
    static_assert((NST - 1) * NL <= 63, "vmcnt is a 6-bit counter");
    static_assert(BM == 128 || (BM == 64 && EPI == EPI_HEADS_FOLD), "64 rows: the heads-fold consumer only (the producer's row sums and the LayerNorm tail count 128 rows)");
    constexpr int RS = BN + 4;
    constexpr int ROWMAJOR_HALVES = 2 * BM * RS * 2;
    constexpr int LDS_HALVES = (NST * STAGE > ROWMAJOR_HALVES) ? NST * STAGE : ROWMAJOR_HALVES;
    // fold consumer, behind the ring: (mu', rho) of the tile's 128 rows, then u and v of its 144 columns - fetched ONCE per workgroup
    // at kernel start (every thread loading the vectors of its nine units from L2 was 147 KB through the L1 per workgroup: to_q
    // 19.2 vs 17.7 us)
    // (+ BM pairs nobody reads: where the mirrored rows of GemmArgs::fold_mirror leave theirs - they run the SAME instructions as the tile's own rows)
    constexpr int STAT_HALVES = FOLD_C ? BM * 4 + 2 * BN * 2 + BM * 4 : 0;
    static_assert((LDS_HALVES + STAT_HALVES) * 2 <= 160 * 1024 && NINST % 2 == 0, "LDS budget / loader split");
    __shared__ __attribute__((aligned(16))) S smem[LDS_HALVES + STAT_HALVES];
    // (Round 2 left an untested option here - the LOADER waves fetching 5 of the 9 fp32 residual row-chunks of every thread by
    // LDS-DMA into the 47 KB behind the ring.  Measured in round 3, same box: gate-residual 19.3 / 19.5 vs 19.2 / 18.4 us at
    // K = 1152, 49.6 / 47.8 vs 46.6 / 49.3 us at K = 4608, the configs[1] step 9.23 - 9.27 vs 9.12 - 9.17 ms: slower.  vmcnt is ONE
    // in-order counter per wave: the residual rows come from MALL / HBM, the tiles from L2, and every counted "tile landed" wait
    // of the loader also waited for the slower loads queued before it.  The same rows requested by the COMPUTE waves before the
    // main loop (their vmcnt queue is never waited on in the loop; 4 / 6 / 8 of the 9 chunks in 16 / 24 / 32 more VGPRs, 32-bit
    // offsets, no scratch) measured no better either: gate-residual 19.9 - 20.8 vs 19.8 - 20.3 us at K = 1152, the step 9.23 - 9.26 /
    // 9.30 - 9.34 / 9.30 - 9.33 vs 9.19 - 9.24 ms (tools/gpu/r3_s2.sh).  The epilogue does not wait for the residual READ: the
    // timeline of the Linear epilogue, which reads nothing, already shows it - 2.6k cycles of parking, 4.1k of store issue and
    // 4.7k until the last store is acknowledged, i.e. the 256 workgroups' simultaneous WRITE burst.  Both options removed.)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = pl_N / BN, mt = (pl_M + BM - 1) / BM;
    const int id = xcd_remap(blockIdx.x, nt * mt);
    const int m0 = (id / nt) * BM, n0 = (id % nt) * BN;
    const int nk = pl_K / BK;

    if (wave >= 8) {
        if (PRIMX_LOADER_PRIO) __builtin_amdgcn_s_setprio(PRIMX_LOADER_PRIO);
        // ---------------- loader wave lw: instructions t = lw * 17 + i, rows 8t .. 8t+7 of the 272-row stage image
        const int lw = wave - 8;
        const S* gp[NL];
        // (producer, tile-uniform: the row tiles from pl_ab_from on read the one row pl_Ab as every row of A - GemmArgs::a_bcast)
        const bool a_one = FOLD_P && pl_Ab != nullptr && m0 >= pl_ab_from;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int row = 8 * (lw * NL + i) + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            gp[i] = (row < BM) ? (a_one ? pl_Ab + c * 8 : pl_A + (int64_t)min(m0 + row, pl_M - 1) * pl_K + c * 8)
                               : pl_W + (int64_t)(n0 + row - BM) * pl_K + c * 8;
        }
        auto issue = [&](int kt, int stage) {
#pragma unroll
            for (int i = 0; i < NL; ++i)
                __builtin_amdgcn_global_load_lds((GV*)(uintptr_t)(gp[i] + kt * BK),
                                                 (LV*)(smem + stage * STAGE + (lw * NL + i) * 512), 16, 0, 0);
        };
#pragma unroll
        for (int s0 = 0; s0 < NST; ++s0) issue(min(s0, nk - 1), s0);
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NST - 1) * NL) : "memory");   // P: tile 0 landed
        int st = 0;
        for (int kt = 0; kt < nk; ++kt) {
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NST - 2) * NL) : "memory");   // S_kt: tile kt+1 landed, NST - 2 newer ones may fly
            issue(min(kt + NST, nk - 1), st);                                              // tile kt's stage is free now
            st = (st == NST - 1) ? 0 : st + 1;
        }
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");                   // D
        asm volatile("s_barrier" ::: "memory");                                          // E
        if constexpr (FOLD_P) asm volatile("s_barrier" ::: "memory");                    // H (every wave executes every barrier)
        if constexpr (EPI == EPI_GATE_RESIDUAL_LN) {
            if (pl_rest.ln_light & 8) asm volatile("s_barrier\n\ts_barrier" ::: "memory");   // F, G of the LayerNorm tail (every wave executes every barrier)
        }
        return;
    }

    // ---------------- compute waves: the tile / wave roles of gemm144_dma_kernel
    if (PRIMX_COMPUTE_PRIO) __builtin_amdgcn_s_setprio(PRIMX_COMPUTE_PRIO);
    const int kg = wave >> 2, wm = wave & 3;
    const int lr = lane & 15, lg = lane >> 4;
    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int a_row = wm * (16 * MI) + lr;
    const int chunk = kg * 4 + lg;
    auto read_frags = [&](int stage, V8 (&a)[MI], V8 (&b)[NI]) {
        const S* As = smem + stage * STAGE;
        const S* Ws = As + BM * 64;
#pragma unroll
        for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const V8*>(As + lds_off(a_row + i * 16, chunk));
#pragma unroll
        for (int j = 0; j < NI; ++j) b[j] = *reinterpret_cast<const V8*>(Ws + lds_off(lr + j * 16, chunk));
    };
    auto multiply = [&](const V8 (&a)[MI], const V8 (&b)[NI]) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = T16<DT>::mfma16(a[i], b[j], acc[i][j]);
    };
    constexpr int NROWCH = (BM * (BN / 4) + 511) / 512;                                // (64 rows: 4.5 - the fifth chunk is half full)
    constexpr bool ROWCH_RAGGED = (BM * (BN / 4)) % 512 != 0;
    f32x4 xpre[NROWCH];
    // fold consumer: the tile's row statistics from the producer's partial sums, while the loaders fetch the first tiles (requested
    // BEFORE the prefetch lines: vmcnt is in-order, the wait for these must not include those)
    f32x2* const fstat = reinterpret_cast<f32x2*>(smem + LDS_HALVES);
    float* const fu = reinterpret_cast<float*>(smem + LDS_HALVES + BM * 4);              // u[144], then v[144]
    FoldPartials fpart;
    f32x2 fu2 = {0.f, 0.f}, fv2 = {0.f, 0.f};
    const int tuv = tid - BM;                                                            // threads 128 .. 199: two columns each (64 rows: 64 .. 135)
    // GemmArgs::fold_mirror: waves 4, 5 of a column tile 0 workgroup own the mirrored rows (wave-uniform; 64 rows: wave 0 the tile's own, wave 4
    // the mirrored ones, waves 1 - 2 copy u / v - disjoint like waves 0 - 1, 4 - 5 and 2 - 3 at 128).  ONE call site for both kinds
    // of rows - the same instructions, hence the same bits, as the launch that multiplies those rows runs on them (two call sites
    // contracted mean + centre differently: 1 ulp in a few per cent of the rows); the mirrored rows' LDS pairs go behind u / v, unread.
    const bool st_own = wave < BM / 64;
    [[maybe_unused]] bool st_rows = false, st_tile0 = false;
    [[maybe_unused]] int st_m0 = m0, st_M = pl_M, st_t = tid;
    [[maybe_unused]] f32x2* st_dst = fstat;
    if constexpr (FOLD_C) {
        const bool mirror = p.fold_mirror > 0 && n0 == 0 && wave >= 4 && wave < 4 + BM / 64;
        st_rows = st_own || mirror;
        st_tile0 = n0 == 0;
        if (mirror) {
            st_m0 = m0 + p.fold_mirror; st_M = pl_M + p.fold_mirror; st_t = tid - 256;
            st_dst = reinterpret_cast<f32x2*>(smem + LDS_HALVES + BM * 4 + 2 * BN * 2);
        }
        if (st_rows) fpart = fold_stats_load<DT>(p, st_M, st_m0, st_t);
        else if (tuv < BN / 2) {
            fu2 = *reinterpret_cast<const f32x2*>(p.fold_u + n0 + 2 * tuv);
            fv2 = *reinterpret_cast<const f32x2*>(p.fold_v + n0 + 2 * tuv);
        }
    }
    const pf_u32x2 pf_v = gemm_prefetch_lines<DT>(p, wave, lane);                        // (the launch's prefetch range)
    if constexpr (FOLD_C) {
        if (st_rows) fold_stats_finish<DT>(p, fpart, st_M, pl_K, st_m0, st_t, st_tile0, st_dst);
        else if (tuv < BN / 2) {
            *reinterpret_cast<f32x2*>(fu + 2 * tuv) = fu2;
            *reinterpret_cast<f32x2*>(fu + BN + 2 * tuv) = fv2;
        }
    }
    asm volatile("s_barrier" ::: "memory");                                              // P
    if (pl_prof) pc1 = __builtin_readcyclecounter();
    V8 a0[MI], b0[NI], a1[MI], b1[NI];
    read_frags(0, a0, b0);
    int st_next = 1;
    auto step = [&](const V8 (&ac)[MI], const V8 (&bc)[NI], V8 (&an)[MI], V8 (&bn)[NI]) {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                 // S_kt
        read_frags(st_next, an, bn);
        multiply(ac, bc);
        st_next = (st_next == NST - 1) ? 0 : st_next + 1;
    };
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        step(a0, b0, a1, b1);
        step(a1, b1, a0, b0);
    }
    if (kt < nk) step(a0, b0, a1, b1);
    asm volatile("" ::"v"(pf_v[0]), "v"(pf_v[1]));                                                        // the prefetch requests have returned
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                     // D: the stages may be reused
    if (pl_prof) pc2 = __builtin_readcyclecounter();

    // ---------------- epilogue: both K halves park their accumulators as fp32 [half][128][148]; row-major walk, 4 columns
    // per thread, 9 row-chunks each (the form of gemm144_dma_kernel).  The residual / gate / bias vectors are
    // requested AFTER the parking (the accumulator registers are free by then: held across it they spilled) and land under
    // the barrier
    float* red = reinterpret_cast<float*>(smem);
    float* mine = red + kg * (BM * RS);
    // (72 ds_write_b32 per lane.  With the MFMA operands swapped the accumulator holds C^T and a tile parks with 18 ds_write_b128 -
    // measured in round 3, same box: gate-residual 18.8 / 48.4 vs 19.1 / 47.5 us, the step 9.06 - 9.13 vs 8.90 - 8.97 ms: slower
    // (16 lanes write the same 4 columns of 16 rows, 592 bytes apart: the row stride that suits the walk below conflicts there).)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[(wm * (16 * MI) + mi * 16 + 4 * lg + r) * RS + ni * 16 + lr] = acc[mi][ni][r];
    __builtin_amdgcn_sched_barrier(0);
    // EPI_HEADS: the tile lies inside ONE (repetition, segment): everything that needs a division is tile-uniform
    int h_hh0 = 0, h_dd0 = 0, h_bb0 = 0, h_tok0 = 0, h_rs = 0, h_seg = 0;
    S* h_dst = nullptr;
    if (HEADS) {
        const int per = p.heads * p.dh;
        const int seg_all = n0 / per, rep_i = seg_all / p.n_seg;
        h_seg = seg_all - rep_i * p.n_seg;
        const int w0 = n0 - seg_all * per;
        h_hh0 = w0 / p.dh;
        h_dd0 = w0 - h_hh0 * p.dh;
        h_bb0 = m0 / p.rows_per_batch;
        h_tok0 = m0 - h_bb0 * p.rows_per_batch;
        h_rs = heads_row_stride(h_seg == 0 ? p.kind[0] : h_seg == 1 ? p.kind[1] : p.kind[2], p.DP);
        h_dst = (h_seg == 0 ? p.dst[0] : h_seg == 1 ? p.dst[1] : p.dst[2]) +
                rep_i * (h_seg == 0 ? p.rep_stride[0] : h_seg == 1 ? p.rep_stride[1] : p.rep_stride[2]);
    }
    V4e bpre[NROWCH], gpre[NROWCH];
    V4e spre[FOLD_P ? NROWCH : 1];             // fold producer: the next LayerNorm's scale vector, the row's (centre, scale)
    f32x2 cpre[FOLD_P ? NROWCH : 1];
#pragma unroll
    for (int i = 0; i < NROWCH; ++i) {
        const int cid = tid + 512 * i;
        const int row = cid / (BN / 4), c4 = cid - row * (BN / 4);
        const int m = min(m0 + row, pl_M - 1);
        bpre[i] = V4e{};
        if (!FOLD_C && p.bias) bpre[i] = *reinterpret_cast<const V4e*>(p.bias + n0 + 4 * c4);
        if (GATE_RES) {
            gpre[i] = *reinterpret_cast<const V4e*>(p.gate + (int64_t)(m / p.rows_per_batch) * p.gate_stride + n0 + 4 * c4);
            xpre[i] = *reinterpret_cast<const f32x4*>(p.x + (int64_t)m * pl_N + n0 + 4 * c4);
            if constexpr (FOLD_P) {
                spre[i] = *reinterpret_cast<const V4e*>(p.ln_scale + (int64_t)(m / p.rows_per_batch) * p.ln_mod_stride + n0 + 4 * c4);
                cpre[i] = reinterpret_cast<const f32x2*>(p.fold_c)[m];
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                     // E
    if (pl_prof) pc_stg = __builtin_readcyclecounter();
#pragma unroll
    for (int i = 0; i < NROWCH; ++i) {
        const int cid = tid + 512 * i;
        if constexpr (ROWCH_RAGGED) {
            if (cid >= BM * (BN / 4)) continue;
        }
        const int row = cid / (BN / 4), c4 = cid - row * (BN / 4);
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(red + row * RS + 4 * c4);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(red + BM * RS + row * RS + 4 * c4);
        if (m0 + row >= pl_M) continue;
        if (HEADS) {
            int d = h_dd0 + 4 * c4, hh = h_hh0;          // d < dh + 144 <= 4 dh
            if (d >= p.dh) { d -= p.dh; ++hh; }
            if (d >= p.dh) { d -= p.dh; ++hh; }
            if (d >= p.dh) { d -= p.dh; ++hh; }
            int tok = h_tok0 + row, bb = h_bb0;          // tok < rows_per_batch + 128 <= 2 rows_per_batch
            if (tok >= p.rows_per_batch) { tok -= p.rows_per_batch; ++bb; }
            const V4e bv = bpre[i];
            V4e o;
            if constexpr (FOLD_C) {
                const f32x4 pre = fold_apply(v0 + v1, fstat[row], *reinterpret_cast<const f32x4*>(fu + 4 * c4),
                                             *reinterpret_cast<const f32x4*>(fu + BN + 4 * c4));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float y = rnd16<DT>(pre[j]);
                    if (h_seg == 0 && p.scale0 != 1.0f) y = rnd16<DT>(p.scale0 * y);
                    o[j] = (S)y;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float y = rnd16<DT>(v0[j] + v1[j] + (float)bv[j]);
                    if (h_seg == 0 && p.scale0 != 1.0f) y = rnd16<DT>(p.scale0 * y);
                    o[j] = (S)y;
                }
            }
            out_store(reinterpret_cast<V4e*>(h_dst + (((int64_t)bb * p.heads + hh) * p.n_pad + tok) * h_rs + d), o);
        } else if (GATE_RES) {
            const V4e gv = gpre[i], bv = bpre[i];
            f32x4 xv = xpre[i];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                xv[j] = xv[j] + rnd16<DT>((float)gv[j] * rnd16<DT>(v0[j] + v1[j] + (float)bv[j]));
            out_store(reinterpret_cast<f32x4*>(p.x + (int64_t)(m0 + row) * pl_N + n0 + 4 * c4), xv);
            if constexpr (FOLD_P) {
                // the next site's operand and this unit's share of the row statistics; the partial sums go back into the unit's
                // own (dead) slot of the parking area
                const V4e sv = spre[i];
                const f32x2 cr = cpre[i];
                float s1 = 0.f, s2 = 0.f;
                V4e o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = xv[j] - cr[0];
                    s1 += d;
                    s2 = __builtin_fmaf(d, d, s2);
                    o[j] = (S)((d * cr[1]) * rnd16<DT>(1.0f + (float)sv[j]));
                }
                out_store(reinterpret_cast<V4e*>(p.ln_out + (int64_t)(m0 + row) * pl_N + n0 + 4 * c4), o);
                *reinterpret_cast<f32x2*>(red + row * RS + 4 * c4) = f32x2{s1, s2};
            }
        } else if constexpr (EPI == EPI_LINEAR) {
            epilogue_row4<DT, EPI>(p, m0 + row, n0 + 4 * c4, v0 + v1, bpre[i]);
        } else if constexpr (EPI == EPI_F32OUT) {
            // fp32 rows (p.x); the bias joins the rows from p.rows_per_batch on (epilogue_quad's EPI_F32OUT)
            const V4e bv = bpre[i];
            const bool wb = p.bias && m0 + row >= p.rows_per_batch;
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = v0[j] + v1[j] + (wb ? (float)bv[j] : 0.f);
            out_store(reinterpret_cast<f32x4*>(p.x + (int64_t)(m0 + row) * pl_N + n0 + 4 * c4), o);
        } else if constexpr (EPI == EPI_LINEAR_FOLD) {
            out_store(reinterpret_cast<V4e*>(p.out + (int64_t)(m0 + row) * pl_N + n0 + 4 * c4),
                      fold_out4<DT>(p, fold_apply(v0 + v1, fstat[row], *reinterpret_cast<const f32x4*>(fu + 4 * c4),
                                                  *reinterpret_cast<const f32x4*>(fu + BN + 4 * c4))));
        }
    }
    if (pl_prof) pc_iss = __builtin_readcyclecounter();
    if constexpr (FOLD_P) {
        // row sums of the tile: 36 units per row -> thread (row, quarter) adds nine, the four quarters meet by DPP - a fixed order
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                 // H
        const int row = tid >> 2, qu = tid & 3;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(red + row * RS + 4 * (qu * 9 + k));
            s1 += v[0];
            s2 += v[1];
        }
        s1 = quad_sum(s1);
        s2 = quad_sum(s2);
        if (qu == 0 && m0 + row < pl_M)
            *reinterpret_cast<f32x2*>(p.fold_part + ((int64_t)(m0 + row) * nt + n0 / BN) * 2) = f32x2{s1, s2};
    }
    if constexpr (EPI == EPI_GATE_RESIDUAL_LN) {
        // ---------------- LayerNorm + modulate of the 128-row block, in the tail of the GEMM that completes its rows
        // (dit_crossattn.py:55-57: every gated residual add is followed by the LayerNorm of the next branch).  The nt column
        // tiles of a row block are nt workgroups; a row is complete when all of them have stored.  The waves of a workgroup meet
        // at a barrier, wave 0 counts the workgroup in on sync[2 g] and waits until all nt have arrived, a second barrier releases
        // the others, and every wave normalises ITS share of the block's rows - 128 / (8 nt) pairs, one row per half-wave, the row
        // body of ln_modulate_row32_kernel (ln_row.h: same bits).  Departures are counted on sync[2 g + 1]; the last one zeroes both
        // words, so a block's words are zero between launches whatever nt the next launch has.
        // MEASURED (round 4, same box, configs[1] step): bit-identical to the two launches and SLOWER in every protocol - one
        // arrival per wave 12.8 ms, one per workgroup 10.25 ms (agent-scope or same-XCD fences, L1 / L2 invalidate or none, sleep 2
        // or 8, counter read by load or by returning atomic: all within 0.03 ms), agent-scope release with its L2 write-back
        // 13.8 - 14.8 ms, against 8.99 ms with the LayerNorm as a launch of its own.  The fused kernel lasts 50 us where the GEMM
        // (28) and the LayerNorm (7) + a boundary (1.3) take 36: serialized same-address atomics cost ~0.5 us each and a waiting
        // workgroup sees the last arrival only microseconds later - a dependent kernel launch is the cheaper hand-over between CUs
        // on this part.  The route therefore runs only when the caller passes `sync` words (DiT.ln_in_kernel, off by default).
        // Why the in-kernel wait is safe: the waited-for workgroups never depend on the waiting ones and are dispatched no later
        // than them - the workgroups of a block have consecutive ids on one XCD (mt % 8 == 0, checked by the host; the id -> XCD
        // mapping itself by a probe launch, xcd_mapping_ok), the dispatcher hands out ids in order, so whenever the XCD's CUs are
        // all held by waiting workgroups the oldest block among them is complete (32 CUs >= 3 whole blocks of 8).  A bounded spin
        // (~1 s) turns a violated assumption into a counted error (primx_ln_sync_timeouts) instead of a hang.
        // p.ln_light (PRIMX_LN_MODE): bit 0 = same-XCD release (stores acknowledged by the shared L2, no L2 write-back), bits 1-2 =
        // acquire (0: agent-scope fence = L2 invalidate, 1: this CU's L1 only, 2: none), bit 3 = ONE arrival per workgroup (the
        // waves meet at a workgroup barrier, wave 0 counts in and waits, a second barrier releases the others) instead of one per
        // wave, bits 4-7 = s_sleep argument of the wait loop
        const int mode = p.ln_light;
        const bool per_wg = (mode & 8) != 0;
        const unsigned per = per_wg ? (unsigned)nt : (unsigned)nt * 8u;
        unsigned* cnt = p.sync + 2 * (m0 / BM);
        if (mode & 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (per_wg) asm volatile("s_barrier" ::: "memory");                             // F: every wave's stores are out
        if (lane == 0 && (!per_wg || wave == 0)) {
            __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int spins = 0;
            const int nap = (mode >> 4) & 15;
            // (reading the counter with a returning atomic instead of the agent-scope load measured the same step time; an L1
            // invalidate + plain load never saw the arrivals: round 4, profiles/r4_experiments.txt)
            auto seen = [&]() -> unsigned { return __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
            while (seen() < per) {
                if (nap >= 8) __builtin_amdgcn_s_sleep(8);
                else if (nap >= 4) __builtin_amdgcn_s_sleep(4);
                else if (nap >= 2) __builtin_amdgcn_s_sleep(2);
                else __builtin_amdgcn_s_sleep(1);
                if (++spins > (1 << 20)) {
                    atomicAdd(&g_ln_sync_timeouts, 1u);
                    break;
                }
            }
        }
        if (per_wg) asm volatile("s_barrier" ::: "memory");                             // G: the block's rows are complete
        const int acq = (mode >> 1) & 3;
        if (acq == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        else if (acq == 1) asm volatile("buffer_inv sc0" ::: "memory");
        else asm volatile("" ::: "memory");
        const int q = (n0 / BN) * 8 + wave;                   // this wave among the block's `per`
        for (int r = 2 * q + (lane >> 5); r < BM; r += 2 * (int)per) {
            const int m = m0 + r;
            if (m >= pl_M) continue;
            const int64_t bo = (int64_t)(m / p.rows_per_batch) * p.ln_mod_stride;
            ln_row32<DT, 9>(p.x + (int64_t)m * pl_N, p.ln_shift + bo, p.ln_scale + bo, p.ln_out + (int64_t)m * pl_N, lane & 31, p.ln_eps);
        }
        if (lane == 0 && (!per_wg || wave == 0)) {
            const unsigned d = __hip_atomic_fetch_add(cnt + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == per - 1) {                                // everybody has passed the wait: the words go back to zero
                __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(cnt + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (pl_prof) {
        __builtin_amdgcn_s_waitcnt(0);   // the stores have been acknowledged
        const unsigned long long pc3 = __builtin_readcyclecounter(), pr1 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            atomicMin(&g_gemm_prof[0], pr0); atomicMax(&g_gemm_prof[1], pr1);
            atomicAdd(&g_gemm_prof[2], pc1 - pc0); atomicAdd(&g_gemm_prof[3], pc2 - pc1);
            atomicAdd(&g_gemm_prof[4], pc3 - pc2); atomicAdd(&g_gemm_prof[5], 1ull); atomicAdd(&g_gemm_prof[6], pr0);
            atomicAdd(&g_gemm_prof[7], ((pc_stg - pc2) << 32) | (pc_iss - pc_stg));          // (parking + the barrier behind it | the walk's issue)
            atomicAdd(&g_gemm_prof[8], pr1 - pr0); atomicAdd(&g_gemm_prof[9], pc3 - pc0);
            if (blockIdx.x < 4096) {
                unsigned xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                g_gemm_wg[blockIdx.x][0] = pr0; g_gemm_wg[blockIdx.x][1] = pr1 - pr0; g_gemm_wg[blockIdx.x][2] = pc3 - pc0;
                g_gemm_wg[blockIdx.x][3] = ((unsigned long long)(xcc & 15) << 32) | (unsigned)(pc3 - pc2);
            }
        }
    }
