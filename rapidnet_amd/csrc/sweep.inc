// sweep.inc -- members of rn::Ctx<T> that launch one sweep of the solver and the main pass of its dual update (included inside the struct
// body of rapidnet_capi.hip).  A sweep is DECIDED first and launched afterwards: sweep_plan fills a SweepPlan from the batch's flags, the
// sweep's arguments and the context's shape and knobs; launch_sweep then runs the product (1) and, per right-hand side, the steps
//   sweep_chains_up (2a)   sweep_exchange (2b)   sweep_crown_up (2c)   launch_v_lv (3)   sweep_down (4)
// Which instantiation of a kernel template a launch runs is chosen by a selector beside the template's launch (stream_kernel, slab_kernel,
// up_chain_kernel, ...): all instantiations of one family and one T share a signature, and every launch is written once.

    int stage_nodes(int k) const { return h_stageCum[k + 1] - h_stageCum[k]; }
    // span of the streaming kernel: G columns = G*SPC 16-byte slots, NL slots per thread.  Preferred: spans that are whole
    // 128-byte lines (G*SPC*16 % 128 == 0) -- otherwise every span boundary splits a cache line between two wave-loads
    // that are issued at different times, and the non-temporal stream fetches that line twice (measured with
    // FETCH_SIZE: 4.35 GB per launch with G = 5, 4.14 GB with G = 8 on the 493-scenario tree, 6 % of the kernel's time)
    // -- with at most 2 slots per thread, then the best lane utilisation, then the larger span.  Without a line-aligned
    // candidate: the G that fills a multiple of STREAM_THREADS slots best.
    void stream_shape(int *G, int *NL) const {
        const int SPC = LD * block_elem() / 16;      // (LD counts entries of the storage type)
        int bestG = 0, bestNL = 0, bestClass = -1; double bestU = -1;
        for (int g = 1; g <= std::min(ny, 64); g++) {
            const int slots = g * SPC, nl = (slots + STREAM_THREADS - 1) / STREAM_THREADS;
            if (nl > STREAM_NLMAX) break;
            const bool aligned = ((long long)slots * 16) % 128 == 0;
            const int cls = aligned ? (nl <= 2 ? 2 : 1) : 0;
            const double u = (double)slots / ((double)nl * STREAM_THREADS);
            const bool tie = std::fabs(u - bestU) <= 1e-9;
            if (cls > bestClass || (cls == bestClass && (u > bestU + 1e-9 || (tie && cls > 0)))) { bestClass = cls; bestU = u; bestG = g; bestNL = nl; }
        }
        if (bestG == 0) { bestG = 1; bestNL = (SPC + STREAM_THREADS - 1) / STREAM_THREADS; }
#ifdef RN_STREAM_G   // tuning builds: force the span
        bestG = RN_STREAM_G; bestNL = (bestG * SPC + STREAM_THREADS - 1) / STREAM_THREADS;
#endif
        *G = bestG; *NL = bestNL;
    }
    size_t stream_lds(int G) const { return (size_t)(((ny + 3) & ~3) + (size_t)G * LD) * sizeof(T); }
    // k_stream_gemv's split last round (kernels.hpp, StreamSplit): applies when the launch is longer than one round, its last round
    // is at most half full (two workgroups per block still fit one round), every block of that round lies in the last
    // STREAM_SPLIT_STAGES stages of the chain region (the consumers add the second partial there) and a block has at least two
    // groups of spans.  splitFirst = nodes: no split.
    T *d_my2 = nullptr;
    int splitFirst = -1, splitSpanHalf = 0;
    bool streamTwoPerCU = false;
    // the skip of operator spans that meet no nonzero entry of w (k_stream.hpp, stream_walk; RN_KNOB_STREAM_SKIP = 0: every span): what every workgroup of
    // the most recent launch walked is in d_streamLive (rn_debug_stream_live, rn_algorithmic_bytes); lastStreamGrid = 0: no launch yet
    int2 *d_streamLive = nullptr;
    int *d_streamUnits = nullptr;      // the units each workgroup walked (rn_debug_stream_units)
    int lastStreamGrid = 0, lastStreamSplitFirst = 0;
    bool stream_skip() const { return knob[RN_KNOB_STREAM_SKIP] != 0; }
    // The skip at HALF-span granularity (k_stream.hpp, stream_walk_half; RN_KNOB_STREAM_HALF, default on): where the kernel's units are half-spans
    // (NL = 2, G even) and half a span is a whole number of 64-byte HALF lines.  fp32 blocks of 2nv = 194 rows: 8 columns x 196 floats = 6 272 B =
    // 49 whole lines.  fp64: LD = 194, 4 columns x 194 doubles = 6 208 B = 48.5 lines -- a span's two halves share its middle line, so a lone
    // live half fetches 49 lines for 48.5 and two live halves request the middle line in two wave-loads (as every wave-load boundary inside a
    // span always did: 1 KB wave-loads over columns of 1 552 B); measured on the 493-scenario tree, profiles/ab_stream_half.txt.  A half that
    // is not even a whole number of half lines is not skipped by itself (no such shape was measured).
    // Off: both halves take their span's liveness.  RN_KNOB_STREAM_SKIP = 1 FORCES the skip by whole spans, the form that value has always selected
    // (tests/test_gpu_stream_skip.py holds rn_algorithmic_bytes of such contexts to the bytes of the live spans); the half-spans belong to the
    // library's own choice, knob -1.
    bool stream_half_on() const {
        int G, NL;
        stream_shape(&G, &NL);
        return stream_half_on(G, NL);
    }
    bool stream_half_on(int G, int NL) const {
        return knob[RN_KNOB_STREAM_SKIP] < 0 && knob[RN_KNOB_STREAM_HALF] != 0 && NL == 2 && G % 2 == 0 && ((long long)(G / 2) * LD * block_elem()) % 64 == 0;
    }
    size_t stream_nz_bytes() const { return (size_t)((ny + 63) / 64 + 1) * 8; }      // the column mask behind the kernel's LDS sets
    int stream_split_setup() {
        if (!d_streamLive && !structured) { if (int rc = dalloc(&d_streamLive, (size_t)2 * d.nodes)) return rc; }
        if (!d_streamUnits && !structured) { if (int rc = dalloc(&d_streamUnits, (size_t)2 * d.nodes)) return rc; }
        if (splitFirst >= 0) return RN_OK;
        splitFirst = d.nodes;
        const int mode = knob[RN_KNOB_STREAM_SPLIT] != 0;
        int G, NL;
        stream_shape(&G, &NL);
        const int D = NL <= 2 ? RN_STREAM_D : RN_STREAM_D_WIDE, groups = (ny / G) / D;
        const int r = d.nodes % numCUs, cs = chainStage, K = h_stageCum[cs + 1] - h_stageCum[cs];
        // which instantiation the launches run: the one with the split's second code path allocates fewer registers (122 instead of
        // 150), so two workgroups share a CU -- start-up and drain of the launch overlap better, the steady state is slower in fp64 and
        // FASTER in fp32 (half-size blocks: the per-workgroup prologue and epilogue weigh double there).  Same-box A/B, one | two per
        // CU, ms per iteration: fp64 whole tree (42 rounds) 0.6733 | 0.6854, 1/2 shard 0.3712 | 0.3736, 1/4 shard (10.7 rounds)
        // 0.2101 | 0.2119, 1/8 shard (5.4 rounds) 0.1352 | 0.1318; fp32 whole tree 0.3838 | 0.3752 (the streaming kernel 313 -> 303 us
        // = 0.84 of the HBM peak).  So the rule was: fp32 always, fp64 for launches of fewer than 8 rounds.
        // With the skip of spans that meet no nonzero dual entry (stream_walk) a workgroup's first group waits for w and a block is about half
        // its bytes: the per-workgroup start-up weighs in fp64 as it did in fp32, and the instantiation is 123 VGPRs with groups of four spans
        // (four waves per SIMD: two workgroups do share a CU).  Same-box A/B on the whole fp64 tree (tools/ab_stream_skip.py), one | two per CU,
        // ms per iteration: with the skip 0.4073 | 0.3778 (the streaming launch 336 -> 305 us), every span walked (knob 0) 0.7000 | 0.6659.
        // So: always.  (The 1/2 and 1/4 shards were not measured again with the skip.)
        // The SPLIT of the last round stays with the launches that had it before (it changes the order of the sums in the last stages, so a
        // context of the old one-per-CU rule keeps the bits it always computed), or follows the knob.
        bool splitOk = sizeof(T) == 4 || store32() || d.nodes < 8 * numCUs;      // (fp32 storage: the fp32 context's block bytes, its rule)
        streamTwoPerCU = true;
        if (knob[RN_KNOB_STREAM_TWO_PER_CU] >= 0) splitOk = streamTwoPerCU = knob[RN_KNOB_STREAM_TWO_PER_CU] != 0;
        if (!mode || !streamTwoPerCU || !splitOk || structured || d.nodes <= numCUs || r == 0 || 2 * r > numCUs || groups < 2) return RN_OK;
        if (d.N - cs < STREAM_SPLIT_STAGES || r > STREAM_SPLIT_STAGES * K) return RN_OK;     // (the cut never moves the chain region's END)
        if (int rc = dalloc(&d_my2, (size_t)r * 2 * d.nv)) return rc;
        splitFirst = d.nodes - r;
        splitSpanHalf = (groups + 1) / 2 * D;       // whole groups; the first half gets the odd one (the second also walks the ragged last span)
        return RN_OK;
    }
    // The instantiations of k_stream_gemv: the blocks' storage type, SPLIT, NR and NL are each chosen HERE and nowhere else (all kernels of one T
    // share a signature).  Two right-hand sides run the unsplit kernel; one runs the SPLIT one where two workgroups share a CU.
    typedef void (*StreamKernel)(SweepArgs<T>, int, int, StreamSplit<T>, StreamRhs2<T>);
    template <typename ST, bool SPLIT, int NR>
    static StreamKernel stream_kernel_nl(int NL) {
        switch (NL) {
            case 1: return k_stream_gemv<T, 1, SPLIT, NR, ST>;
            case 2: return k_stream_gemv<T, 2, SPLIT, NR, ST>;
            case 3: return k_stream_gemv<T, 3, SPLIT, NR, ST>;
            default: return k_stream_gemv<T, 4, SPLIT, NR, ST>;
        }
    }
    template <typename ST>
    static StreamKernel stream_kernel_of(bool twoPerCU, bool pair, int NL) {
        return pair ? stream_kernel_nl<ST, false, 2>(NL) : twoPerCU ? stream_kernel_nl<ST, true, 1>(NL) : stream_kernel_nl<ST, false, 1>(NL);
    }
    static StreamKernel stream_kernel(bool stored32, bool twoPerCU, bool pair, int NL) {
        if constexpr (sizeof(T) == 8) { if (stored32) return stream_kernel_of<float>(twoPerCU, pair, NL); }
        return stream_kernel_of<T>(twoPerCU, pair, NL);
    }
    bool ensure_stream_lds() {   // > 64 KB of dynamic LDS needs the function attribute (once): every kernel the selector can return
        static const bool ok = [] {
            bool all = true;
            for (int stored32 = 0; stored32 < (sizeof(T) == 8 ? 2 : 1); stored32++)
                for (int form = 0; form < 3; form++)
                    for (int NL = 1; NL <= STREAM_NLMAX; NL++)
                        all = all && hipFuncSetAttribute((const void *)stream_kernel(stored32 != 0, form == 1, form == 2, NL), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
            return all;
        }();
        return ok;
    }
    // second != nullptr: two right-hand sides in one pass (k_stream_gemv NR = 2; see stream_pair_ok)
    int launch_stream(const SweepArgs<T> &a, const StreamRhs2<T> *second = nullptr) {
        int G, NL;
        stream_shape(&G, &NL);
        RN_CHECK(NL <= STREAM_NLMAX, RN_E_ARG, "k_stream_gemv: more than 4096 values per operator column are not supported (2*nv too large)");
        const size_t lds = stream_lds(G), nzb = stream_nz_bytes();
        RN_CHECK(lds + nzb <= 64 * 1024 || (lds + nzb <= 160 * 1024 && ensure_stream_lds()), RN_E_ARG, "k_stream_gemv: a span of operator columns does not fit the CU's LDS");
        const int node0 = h_stageCum[a.chainStage];   // first node of the chain region as this sweep sees it
        const StreamSplit<T> sp{a.splitFirst, splitSpanHalf, d_my2, stream_skip() ? 1 : 0, d_streamLive, stream_half_on(G, NL) ? 1 : 0, d_streamUnits};
        const int grid = d.nodes + (d.nodes - a.splitFirst);      // two workgroups for every block of the split round
        lastStreamGrid = grid; lastStreamSplitFirst = a.splitFirst;
        if (second && store32()) {
            // (both sets are doubles over a span chosen for 4-byte entries: twice the native pair's LDS for the same operator width, so
            //  past 64 KB the launch takes the function attribute like the one-vector launch does)
            RN_CHECK(a.splitFirst >= d.nodes, RN_E_STATE, "k_stream_gemv over fp32 storage with two right-hand sides: unsplit launches only");
            RN_CHECK(2 * lds + nzb <= 64 * 1024 || (2 * lds + nzb <= 160 * 1024 && ensure_stream_lds()), RN_E_ARG, "k_stream_gemv over fp32 storage with two right-hand sides: the two LDS sets do not fit the CU's LDS");
        } else if (second) {
            RN_CHECK(a.splitFirst >= d.nodes && 2 * lds + nzb <= 64 * 1024, RN_E_STATE, "k_stream_gemv with two right-hand sides: unsplit launches only");
        }
        hipLaunchKernelGGL(stream_kernel(store32(), streamTwoPerCU, second != nullptr, NL), dim3(grid), dim3(STREAM_THREADS), (second ? 2 : 1) * lds + nzb, stream,
                           a, G, node0, sp, second ? *second : StreamRhs2<T>{nullptr, nullptr, nullptr});
        return RN_OK;
    }
    // rn_set_sweep_pairing: RN_PAIR_AUTO (default), RN_PAIR_ON (AUTO plus fp32-stored blocks), RN_PAIR_OFF (never)
    int pairReq = RN_PAIR_AUTO;
    // two right-hand sides in one streaming pass are possible for dense per-node blocks, and
    //   blocks in the context's own type (k_stream_gemv NR = 2): both LDS sets in 64 KB, no split last round;
    //   fp32-stored blocks (k_stream_gemv with ST = float, NR = 2; bitwise the two sweeps, its gain not measured yet): behind RN_PAIR_ON only, a split
    //   last round included -- the pair sweep then runs unsplit (launch_sweep), the context's other sweeps keep their split.  Its LDS sets
    //   are doubles over a span chosen for 4-byte entries (twice the columns): twice the native pair's bytes at the same operator width, so
    //   they may take the CU's whole 160 KB (ensure_stream_lds, at the launch) -- at 64 KB nv = 32 with ny = 80 would already not pair
    bool stream_pair_ok() const {
        if (structured || pairReq == RN_PAIR_OFF) return false;
        int G, NL;
        stream_shape(&G, &NL);
        if (store32()) return pairReq == RN_PAIR_ON && 2 * stream_lds(G) + stream_nz_bytes() <= 160 * 1024;
        return !(splitFirst >= 0 && splitFirst < d.nodes) && 2 * stream_lds(G) + stream_nz_bytes() <= 64 * 1024;
    }
    static int slab_stride(int kp) { return (kp + 59) / 64 * 64 + 4; }   // >= kp, = 4 (mod 64): conflict-free MFMA B reads
    // waves per slab workgroup.  Many slabs (more workgroups than CUs): the count in {4, 6, 8} that wastes the least SIMD
    // time on idle tile slots (throughput).  Few slabs (small or sharded trees: every workgroup has a CU to itself): the
    // count with the shortest critical path per workgroup (latency).
    // which MFMA loop the slab kernels run (slab_mfma): the software-pipelined one when a launch has at most one workgroup per CU
    // (small or sharded trees: nothing else hides the operand latency) and in fp32 (half the registers: the workgroups still share
    // a CU); the lean one otherwise.  Measured, k_gemm_vlv, lean | pipelined: 31-scenario tree 14.0 | 12.5 us, 1/8 shard 19.4 |
    // 17.7, 1/2 shard (340 slabs) 27.3 | 28.1, whole 493-scenario tree 30.0 | 35.8; fp32 wide network (k_gemm_prep_m2) 954 | 574.
    bool few_slabs() const {
        const int force = knob[RN_KNOB_SLAB_PIPE];
        return force >= 0 ? force != 0 : ((d.nodes + 15) / 16 <= numCUs || sizeof(T) == 4);
    }
    int slab_waves(int tilesA, int kstepsA, int tilesB, int kstepsB) const {
        const bool few = (d.nodes + 15) / 16 <= numCUs;
        int best = 4; long bestCost = -1;
        for (int nw : {4, 6, 8, 12, 16}) {
            if (nw > SLAB_MAX_WAVES || (nw > 8 && !few)) continue;
            const long path = (long)((tilesA + nw - 1) / nw) * kstepsA + (long)((tilesB + nw - 1) / nw) * kstepsB;
            const long cost = few ? path * 16 + nw : (long)nw * path;
            if (bestCost < 0 || cost < bestCost) { best = nw; bestCost = cost; }
        }
        return best;
    }
    // The instantiations of the slab products: PIPE (the software-pipelined MFMA loop, few_slabs) and CT (slabs per workgroup, wide_ct) are chosen
    // HERE; the launches and the function attributes go through these.
    typedef void (*SlabKernel)(GemmArgs<T>, int);
    typedef void (*PrepM2Kernel)(GemmArgs<T>, SweepArgs<T>, int);
    typedef void (*CompKernel)(GemmArgs<T>, int, SweepArgs<T>, int);
    typedef void (*VlvKernel)(GemmArgs<T>, GemmArgs<T>, int, int, SweepArgs<T>, int, int);
    typedef void (*VlvWideKernel)(GemmArgs<T>, GemmArgs<T>, int, int, SweepArgs<T>, int);
    template <int EPI>
    static SlabKernel slab_kernel(bool pipe) { return pipe ? k_gemm_slab<T, EPI, true> : k_gemm_slab<T, EPI, false>; }
    static PrepM2Kernel prep_m2_kernel(bool pipe) { return pipe ? k_gemm_prep_m2<T, true> : k_gemm_prep_m2<T, false>; }
    static CompKernel comp_kernel(bool pipe) { return pipe ? k_gemm_comp<T, true> : k_gemm_comp<T, false>; }
    static VlvKernel vlv_kernel(bool pipe) { return pipe ? k_gemm_vlv<T, true> : k_gemm_vlv<T, false>; }
    static VlvWideKernel vlv_wide_kernel(int ct) { return ct == 2 ? k_gemm_vlv_wide<T, 2> : k_gemm_vlv_wide<T, 3>; }
    // What the launching steps below chose (rn_debug_slab_product's info[]): written only while the hook has set slabRep; slot 0 is the first
    // (or only) launch of a step, slot 1 the second of a pair that runs as two launches.
    enum { SLABK_NONE = 0, SLABK_VLV = 1, SLABK_VLV_WIDE = 2, SLABK_COMP = 3, SLABK_PREP_M2 = 4, SLABK_SLAB = 5, SLABK_SHARED = 6, SLABK_STRUCT_PREP = 7 };
    struct SlabReport { int kernel[2], nw[2], grid[2]; long long lds[2]; int pipe, frag, ct, pre; };
    SlabReport *slabRep = nullptr;
    void slab_report(int slot, int kernel, int nw, int grid, size_t lds, bool pipe, bool frag, int ct) {
        if (!slabRep) return;
        slabRep->kernel[slot] = kernel; slabRep->nw[slot] = nw; slabRep->grid[slot] = grid; slabRep->lds[slot] = (long long)lds;
        if (slot == 0) { slabRep->pipe = pipe ? 1 : 0; slabRep->frag = frag ? 1 : 0; slabRep->ct = ct; }
    }
    // The shared-operator products are launched in two steps: the *_args functions build the GemmArgs a sweep gives them, the run_* functions
    // choose the kernel and its shape and launch.  rn_debug_slab_product builds the same arguments over scratch buffers and goes through the
    // same run_* functions.
    // sweepSplit: the splitFirst of the sweep whose m1 `aux` holds (SweepArgs; -1: the context's own -- a pair sweep runs unsplit on a split context)
    template <int EPI>
    GemmArgs<T> gemm_args(const T *Mp, int m, int k, const T *in, int ldin, T *out, int ldout, const T *aux, int ldaux, int sweepSplit = -1) const {
        GemmArgs<T> g{Mp, m, k, pad16(m), pad4(k), in, ldin, out, ldout, aux, ldaux, d_prob, d.nodes};
        const int sf = sweepSplit >= 0 ? sweepSplit : splitFirst;
        if (EPI == EPI_V && !structured && sf >= 0 && sf < d.nodes) { g.aux2 = d_my2; g.auxSplit = sf; }   // k_stream_gemv's split last round
        return g;
    }
    template <int EPI>
    void run_gemm(const GemmArgs<T> &g, int slot = 0) {
#if RN_GEMM_SLAB
        const int SB = slab_stride(g.kp);
        const size_t lds = (size_t)16 * SB * sizeof(T);
        if (lds <= 64 * 1024) {   // slab kernel (default); falls back to the tile kernel when the slab does not fit
            const int nw = slab_waves((g.m + 15) / 16, g.kp / 4, 0, 0);
            slab_report(slot, SLABK_SLAB, nw, (d.nodes + 15) / 16, lds, few_slabs(), g.Mf != nullptr, 0);
            hipLaunchKernelGGL(slab_kernel<EPI>(few_slabs()), dim3((d.nodes + 15) / 16), dim3(64 * nw), lds, stream, g, SB);
            return;
        }
#endif
        const int units = (g.mp / (16 * GEMM_RT)) * ((d.nodes + 15) / 16);   // one 64 x 16 output tile per workgroup
        slab_report(slot, SLABK_SHARED, GEMM_WAVES, units, 0, false, false, 0);
        hipLaunchKernelGGL((k_gemm_shared<T, EPI, RN_GEMM_KS>), dim3(units), dim3(GEMM_THREADS), 0, stream, g);
    }
    template <int EPI>
    void launch_gemm(const T *Mp, int m, int k, const T *in, int ldin, T *out, int ldout, const T *aux, int ldaux, int sweepSplit = -1) {
        run_gemm<EPI>(gemm_args<EPI>(Mp, m, k, in, ldin, out, ldout, aux, ldaux, sweepSplit));
    }
    // structured mode, (1) of the sweep: a_i = F_i' xi_i, b_i = G_i' psi_i and m2_i = [Bbt | L'] [a_i; b_i]
    GemmArgs<T> prep_m2_args(const SweepArgs<T> &a) const {
        const int nx = d.nx, nu = d.nu, nv = d.nv;
        GemmArgs<T> g{d_BLp, nv, nx + nu, pad16(nv), pad4(nx + nu), a.ab, nx + nu, a.my + nv, 2 * nv, nullptr, 0, d_prob, d.nodes};
        if (frag_on()) g.Mf = d_BLf;
        return g;
    }
    void run_prep_m2(GemmArgs<T> g, const SweepArgs<T> &a) {
#if RN_GEMM_SLAB
        const int SB = slab_stride(g.kp);
        const size_t lds = (size_t)16 * SB * sizeof(T);
        if (lds <= 64 * 1024) {
            const int nw = slab_waves((g.m + 15) / 16, g.kp / 4, 0, 0);
            slab_report(0, SLABK_PREP_M2, nw, (d.nodes + 15) / 16, lds, few_slabs(), g.Mf != nullptr, 0);
            hipLaunchKernelGGL(prep_m2_kernel(few_slabs()), dim3((d.nodes + 15) / 16), dim3(64 * nw), lds, stream, g, a, SB);
            return;
        }
#endif
        const long long tot = (long long)d.nodes * (d.nx + d.nu);
        const int blocks = (int)std::min<long long>(4096, (tot + 255) / 256);
        hipLaunchKernelGGL(k_struct_prep<T>, dim3(blocks), dim3(256), 0, stream, a);
        g.Mf = nullptr;      // (the products outside the slab family read the column-major copy)
        run_gemm<EPI_LV>(g);
        if (slabRep) slabRep->pre = SLABK_STRUCT_PREP;
    }
    void launch_prep_m2(const SweepArgs<T> &a) { run_prep_m2(prep_m2_args(a), a); }
    bool v_lv_is_slab() const {
#if RN_GEMM_SLAB
        return (size_t)16 * (slab_stride(pad4(d.nv + d.nx)) + slab_stride(pad4(d.nv))) * sizeof(T) <= 64 * 1024;
#else
        return false;
#endif
    }
    // slabs per workgroup of k_gemm_vlv_wide (0: use k_gemm_vlv): 3 when every CU gets many slabs (more than four per CU: the
    // shared operators' stream from L2, re-read per slab, is then what the launch waits for; fp32 wide network, 21 slabs per CU:
    // 1 047 -> 780 us), and only if the workgroup's LDS (ct slab buffers; > 64 KB needs the function attribute, set once) is
    // granted.  With two or three slabs per CU (493-scenario tree) the plain kernel is as fast or faster (30.0 vs 31.2 us).
    int wideCt = -1;
    int wide_ct(int nSlabs, size_t ldsPerSlab) {
        if (wideCt >= 0) return wideCt;
        wideCt = 0;
        int want = nSlabs > 4 * numCUs ? 3 : 0;
        if (knob[RN_KNOB_VLV_WIDE] >= 0) want = std::min(3, knob[RN_KNOB_VLV_WIDE]);   // 0 / 1: off
        for (; want >= 2; want--) {
            const size_t bytes = ldsPerSlab * want;
            if (bytes > 160 * 1024) continue;
            // (the attribute belongs to the function, not to this context: always the device's whole LDS)
            if (bytes <= 64 * 1024 || hipFuncSetAttribute((const void *)vlv_wide_kernel(want), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess) { wideCt = want; break; }
            (void)hipGetLastError();
        }
        return wideCt;
    }
    // values of LDS scratch behind the slab buffers of k_gemm_vlv for the root's children (0: not granted / switched off)
    int crownScratchVals = -1;
    int crown_scratch(size_t ldsSlab) {
        if (crownScratchVals >= 0) return crownScratchVals;
        crownScratchVals = 0;
        const size_t want = (size_t)h_childCount[0] * (d.nv + 2 * d.nx), bytes = ldsSlab + want * sizeof(T);
        if (bytes > 160 * 1024) return 0;
        if (bytes > 64 * 1024) {
            // the attribute belongs to the function, not to this context: always the device's whole LDS, never a smaller value later
            if (hipFuncSetAttribute((const void *)vlv_kernel(true), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
                hipFuncSetAttribute((const void *)vlv_kernel(false), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
                (void)hipGetLastError();
                return 0;
            }
        }
        crownScratchVals = (int)want;
        return crownScratchVals;
    }
    static int wide_waves() { return std::min(RN_WIDE_THREADS / 64, 8); }
    size_t crown_lin_lds(int lin) const {      // k_up_crown_lin's LDS: [parts][W2], parts as the kernel counts them
        const int w2 = d.nv + 2 * d.nx + d.nu, span = w2 - ((lin & 2) ? d.nv : 0), wp = (span + 63) / 64 * 64;
        return (size_t)std::max(1, CROWN_THREADS / wp) * w2 * sizeof(T);
    }
    // Structured mode, linear form: Bs of every node (one full leaf-to-root pass of the linear form: chain walks, crown stages, the root) and
    // c_i = -Rinv Bs_i / (2 p_i) (one product with the first nv columns of [Rinv | T1 | T2]) -- when the affine terms have changed, i.e. once per control step.
    int lin_const_refresh(const SweepArgs<T> &a0) {
        SweepArgs<T> c = a0;
        // the linear form with the Bs columns, no bookkeeping, nothing folded: every crown stage down to the root.  (No exchange either: the
        // linear form exists on unsharded contexts only -- sweep_args sets lin when cutStage <= 0 -- so c.cutSums is null and sweep_crown_up
        // never reaches sweep_exchange; a sharded linear form would need a plan of its own here)
        SweepPlan p{};
        Batch none{};
        c.lin = p.lin = 1;
        sweep_chains_up(none, p, c);
        if (int rc = sweep_crown_up(none, p, c)) return rc;
        launch_gemm<EPI_V>(d_RT2p, d.nv, d.nv, d_sk2, d.nv + d.nx + d.nu, d_vconst, d.nv, nullptr, 0);
        if (d_MCp) launch_gemm<EPI_LV>(d_LBLp, d.nu + d.nx, d.nv, d_vconst, d.nv, d_lvconst, d.nu + d.nx, nullptr, 0);      // [L ; B L] c_i
        if (lin_fold()) {
            const long long tot = (long long)d.nodes * (d.nu + d.nx);
            hipLaunchKernelGGL(k_fold_affine<>, dim3((unsigned)std::min<long long>((tot + 255) / 256, (long long)numCUs * 8)), dim3(256), 0, stream, (void *)d_lvconst, (const void *)d_uhat,
                               (const void *)d_eb, (const void *)d_prevUhat, (const int *)d_parent, d.nodes, d.nu, d.nx, sizeof(T) == 8 ? 1 : 0);
        }
        RN_HIP(hipGetLastError());
        linConstValid = true;
        return RN_OK;
    }
    // SweepArgs::lin of a sweep's launches, from sweep_args' 0 / 1: the walks leave the Bs columns alone (bit 1); the forward walk's affine terms ride in
    // the product's constant (bit 2)
    int lin_bits(int lin) const { return (lin && lin_const()) ? (lin_fold() ? 7 : 3) : lin; }
    // (3) of the sweep: v_i and [L v_i ; B L v_i] for all nodes.  v_lv_args: the two products' arguments as the sweep `a` shapes them (gC: the
    // one product with the composite operator, where the sweep takes that form -- the return value says so)
    bool v_lv_args(const SweepArgs<T> &a, GemmArgs<T> &gV, GemmArgs<T> &gL, GemmArgs<T> &gC) const {
        const int nx = d.nx, nu = d.nu, nv = d.nv;
        gV = GemmArgs<T>{d_RTp, nv, nv + nx, pad16(nv), pad4(nv + nx), a.sk, nv + nx, a.v, nv, a.my, 2 * nv, d_prob, d.nodes, a.my2, a.splitFirst};
        if (a.lin) gV = GemmArgs<T>{d_RT2p, nv, nv + nx + nu, pad16(nv), pad4(nv + nx + nu), a.sk2, nv + nx + nu, a.v, nv, nullptr, 0, d_prob, d.nodes, nullptr, d.nodes};
        if (!a.writePrimal) gV.out = nullptr;   // slab kernel only: v stays in LDS for the second product
        if (structured) gV.aux = nullptr;       // m1_i is folded into the v product (d_my's m1 half stays zero): the epilogue has nothing to fetch
        if (a.lin & 2) {        // Bs's term is the constant c_i (lin_const_refresh): v_i = c_i - [T1 | T2] [q_i + kappa_i ; Bu_i] / (2 p_i); a Hessian sweep (beta = 0) has none
            gV = GemmArgs<T>{d_T12p, nv, nx + nu, pad16(nv), pad4(nx + nu), a.sk2 + nv, nv + nx + nu, a.writePrimal ? a.v : nullptr, nv,
                             a.beta == d_zero ? nullptr : d_vconst, nv, d_prob, d.nodes, nullptr, d.nodes};
        }
        gL = GemmArgs<T>{d_LBLp, nu + nx, nv, pad16(nu + nx), pad4(nv), a.v, nv, a.lvb, nu + nx, nullptr, 0, d_prob, d.nodes};
        if (frag_on()) { gV.Mf = (a.lin & 2) ? d_T12f : (a.lin ? d_RT2f : d_RTf); gL.Mf = d_LBLf; }
        if (!((a.lin & 2) && lin_comp())) return false;
        // one product with the composite operator (k_gemm_comp); v_i, when it is stored, by a launch of its own
        gC = GemmArgs<T>{d_MCp, nu + nx, nx + nu, pad16(nu + nx), pad4(nx + nu), a.sk2 + nv, nv + nx + nu, a.lvb, nu + nx,
                         a.beta == d_zero ? nullptr : d_lvconst, nu + nx, d_prob, d.nodes, nullptr, d.nodes};
        if (frag_on()) gC.Mf = d_MCf;
        return true;
    }
    void run_comp(const GemmArgs<T> &gC, const SweepArgs<T> &a, int foldRoot) {
        const int SBc = slab_stride(gC.kp), nSlabs = (d.nodes + 15) / 16;
        const int nwc = slab_waves((gC.m + 15) / 16, gC.kp / 4, 0, 0);
        slab_report(0, SLABK_COMP, nwc, nSlabs, (size_t)16 * SBc * sizeof(T), few_slabs(), gC.Mf != nullptr, 0);
        hipLaunchKernelGGL(comp_kernel(few_slabs()), dim3(nSlabs), dim3(64 * nwc), (size_t)16 * SBc * sizeof(T), stream, gC, SBc, a, foldRoot);
    }
    void run_v_lv(const GemmArgs<T> &gV, const GemmArgs<T> &gL, const SweepArgs<T> &a, int foldRoot) {
#if RN_GEMM_SLAB
        const int SB = slab_stride(gV.kp), SV = slab_stride(gL.kp);
        const size_t lds = (size_t)16 * (SB + SV) * sizeof(T);
        if (lds <= 64 * 1024) {
            const int nSlabs = (d.nodes + 15) / 16;
            // many slabs per CU: one workgroup per CU with CT slabs each, every A fragment (from L2) used CT times (k_gemm_vlv_wide)
            const int ct = wide_ct(nSlabs, lds);
            if (ct >= 2 && foldRoot != 2) {
                const int grid = (nSlabs + ct - 1) / ct, threads = 64 * wide_waves();
                slab_report(0, SLABK_VLV_WIDE, wide_waves(), grid, lds * ct, true, gV.Mf != nullptr, ct);
                hipLaunchKernelGGL(vlv_wide_kernel(ct), dim3(grid), dim3(threads), lds * ct, stream, gV, gL, SB, SV, a, foldRoot);
                return;
            }
            const int nw = slab_waves((gV.m + 15) / 16, gV.kp / 4, (gL.m + 15) / 16, gL.kp / 4);
            // sharded two-stage crown (foldRoot = 2): scratch for the root's children behind the slab buffers, so that workgroup 0 -- the
            // launch's critical path -- fills its own slab in LDS instead of draining its stores and reading them back
            const int scratch = foldRoot == 2 ? crown_scratch(lds) : 0;
            const size_t ldsAll = lds + (size_t)scratch * sizeof(T);
            slab_report(0, SLABK_VLV, nw, nSlabs, ldsAll, few_slabs(), gV.Mf != nullptr, 1);
            hipLaunchKernelGGL(vlv_kernel(few_slabs()), dim3(nSlabs), dim3(64 * nw), ldsAll, stream, gV, gL, SB, SV, a, foldRoot, scratch);
            return;
        }
#endif
        // two launches: v is always stored (the second product reads it back), from the column-major operators; the context's own split
        // decides about the second partial of m1 as in every product outside the slab pair
        GemmArgs<T> g1 = gemm_args<EPI_V>(gV.M, gV.m, gV.k, gV.in, gV.ldin, const_cast<T *>(gL.in), gV.ldout, a.my, 2 * d.nv, a.splitFirst);
        g1.prob = gV.prob; if (g1.aux2) g1.aux2 = gV.aux2;
        GemmArgs<T> g2 = gL; g2.Mf = nullptr;
        run_gemm<EPI_V>(g1, 0);
        run_gemm<EPI_LV>(g2, 1);   // [L v_i ; B L v_i]
    }
    void launch_v_lv(const SweepArgs<T> &a, int foldRoot) {
        GemmArgs<T> gV, gL, gC;
        if (v_lv_args(a, gV, gL, gC)) {
            run_comp(gC, a, foldRoot);
            if (a.writePrimal) {
                const bool hess = a.beta == d_zero;
                if (hess || vEager || a.v != d_v) launch_gemm<EPI_V>(d_T12p, d.nv, d.nx + d.nu, a.sk2 + d.nv, d.nv + d.nx + d.nu, a.v, d.nv, hess ? nullptr : d_vconst, d.nv);
                else vPending = true;
            }
            return;
        }
        run_v_lv(gV, gL, a, foldRoot);
    }
    // crown handling of the forward sweep: 0 = crown launches of their own; 1 = every chain workgroup walks its crown path and
    // the first descendant chain of a crown node writes it; 2 (sharded) = crown nodes dealt round-robin to the workgroups
    int fold_crown_mode(int cs, bool sharded) const {
        return (RN_FOLD_CROWN_DOWN && cs >= 1 && cs <= CROWN_MAX_DEPTH) ? (sharded ? (h_stageCum[cs] <= 256 ? 2 : 0) : 1) : 0;
    }
    // lanes per chain of k_up_chain_cut, or 0 when the merged launch does not apply: the cut lies right above the chains and every
    // cut parent's local chains fit side by side in one workgroup
    int up_cut_lanes() const {
        if (cutStage <= 0 || cutStage < chainStage) return 0;
        const int lanesPer = (d.nv + d.nx + 63) / 64 * 64;
        if (lanesPer > UPCUT_THREADS) return 0;
        int most = 0;
        for (int i = h_stageCum[cutStage - 1]; i < h_stageCum[cutStage]; i++) most = std::max(most, h_childCount[i]);
        if (most * lanesPer > UPCUT_THREADS) return 0;
        return lanesPer;
    }
    // The instantiations of the walks (as stream_kernel above: chosen here and nowhere else)
    typedef void (*UpChainKernel)(SweepArgs<T>, FinArgs);
    typedef void (*UpChainCutKernel)(SweepArgs<T>, T *, int, int, FinArgs);
    typedef void (*CutSumsKernel)(SweepArgs<T>, T *, int, FinArgs);
    typedef void (*DownChainKernel)(SweepArgs<T>, int);
    typedef void (*DownChainDualKernel)(SweepArgs<T>, int, DualArgs<T>, double, int);
    static UpChainKernel up_chain_kernel(bool lin, bool split) { return lin ? k_up_chain_lin<T> : split ? k_up_chain<T, true> : k_up_chain<T, false>; }
    static UpChainCutKernel up_chain_cut_kernel(bool split, bool gather) {
        return gather ? (split ? k_up_chain_cut<T, true, true> : k_up_chain_cut<T, false, true>) : (split ? k_up_chain_cut<T, true> : k_up_chain_cut<T, false>);
    }
    static CutSumsKernel cut_sums_kernel(bool gather) { return gather ? k_cut_partial_sums<T, true> : k_cut_partial_sums<T, false>; }
    static DownChainKernel down_chain_kernel(bool unsc) { return unsc ? k_down_chain<T, true, RN_DOWN_PF_UNSC> : k_down_chain<T, false>; }
    static DownChainDualKernel down_chain_dual_kernel(bool materialize, bool upRide) {
        return upRide ? k_down_chain_dual<T, false, true> : materialize ? k_down_chain_dual<T, true> : k_down_chain_dual<T, false>;
    }
    // Everything one sweep decides, taken before its first launch (sweep_plan) and read by the steps below.
    enum SweepForm { FORM_DENSE = 0, FORM_STRUCT, FORM_LIN };      // what stands in front of the walks: k_stream_gemv, k_gemm_prep_m2, or nothing (the linear form)
    enum FinRide { FIN_NONE = 0, FIN_CHAIN, FIN_CROWN, FIN_CUT };   // the launch that carries the previous iteration's bookkeeping (Batch::pendingFin)
    struct SweepPlan {
        int phase = 0;
        SweepForm form = FORM_DENSE;
        int lin = 0;                     // SweepArgs::lin of the steps: 0, or the linear form with its bits (1, 3, 7)
        bool oneShot = false;            // the exchange at the cut is pushed to the peers' inboxes by the launch that produces the payload
        bool mergedCut = false;          // k_up_chain_cut: chain walks and the cut parents' local sums in one launch ...
        int cutLanes = 0;                // ... with that many lanes per chain
        bool rodeUp = false;             // the chain walk was done by the previous iteration's fused launch (Batch::upDone)
        FinRide fin = FIN_NONE;
        int foldRoot = 0;                // 1 / 2: the root's (and, sharded, stage 1's) recursion step runs inside the v / Lv launch
        bool fusedCrown = false;         // k_down_crown_all instead of one k_down_crown per stage
        int foldCrown = 0, nCrownWg = 0; // fold_crown_mode, and the workgroups it adds to the forward walk's grid
        bool fuse = false, upRide = false;   // the fused walk + dual update runs (materialising: Batch::fuseMat) / carries the next sweep's chain walk
        int fuseSplit = 1;               // its workgroups per chain
        int downGrid = 0;                // grid of the forward walk's launch, fused or not
        bool unsc = false;               // k_down_chain UNSC: the walk leaves the primal values in Hx
    };
    // a: the sweep's arguments as launch_sweep has set them up (cutSums, chainStage, lin as sweep_args left it, writePrimal, hx); inBatch: the
    // sweep is an iteration of an rn_apg_iterate batch (bt is the caller's, not launch_sweep's own empty one)
    SweepPlan sweep_plan(const Batch &bt, bool inBatch, const SweepArgs<T> &a, int phase, bool hess) const {
        SweepPlan p{};
        const int cs = a.chainStage;
        p.phase = phase;
        p.lin = lin_bits(a.lin);
        p.form = p.lin ? FORM_LIN : structured ? FORM_STRUCT : FORM_DENSE;
        // one-shot exchange (inside rn_apg_iterate batches only): the launch that produces the cut parents' local sums pushes them
        // to every peer, the crown launch gathers them -- no collective in between
        p.oneShot = transport == 1 && peerReady && inBatch && phase == 0 && a.cutSums != nullptr && !hess;
        p.rodeUp = bt.upDone && a.lin && phase == 0 && !hess;
        // sharded, cut right above the chains, few local chains per cut parent: one launch does the chain walks AND the cut
        // parents' local children sums (k_up_chain_cut)
        p.cutLanes = (phase != 2 && a.cutSums) ? up_cut_lanes() : 0;
        p.mergedCut = p.cutLanes > 0;
        // the previous iteration's fold / history entry / distance check.  Sharded (optimistic exchange): it rides in the launch that leaves the
        // payload in d_cut, merged or not.  Single GPU: in the chain walk -- or, when that walk rode in the previous iteration's fused walk +
        // dual update, with the first crown launch
        if (bt.pendingFin && phase != 2) p.fin = a.cutSums ? FIN_CUT : p.rodeUp ? FIN_CROWN : FIN_CHAIN;
        // small crowns are walked by ONE workgroup per direction (stage after stage inside the kernel)
        p.fusedCrown = cs > 0 && h_stageCum[cs] <= 64;
        // the root's own recursion step is folded into workgroup 0 of the v / Lv launch (one launch less) whenever that
        // launch is the slab kernel and stage 0 is not the multi-GPU exchange stage (single GPU: also when the root IS the whole crown --
        // the 31-scenario tree: one launch of 4.6 us less, helper path 40.2 -> 38.8 us)
        // 2: sharded with a two-stage crown whose stage 1 is the exchange stage -- its (presummed) step is folded as well
        p.foldRoot = (RN_FOLD_ROOT && phase == 0 && cs >= (a.cutSums ? 2 : 1) && !(a.cutSums && cutStage == 1) && v_lv_is_slab()) ? 1 : 0;
        if (p.foldRoot && a.cutSums && cs == 2 && cutStage == 2) p.foldRoot = 2;
        // shallow crowns: every chain workgroup walks its own crown path (k_down_chain, foldCrown) -- no crown launch.
        // single GPU: the first descendant chain of a crown node writes it (1); sharded: workgroup 0 writes them all (2),
        // because a replicated crown node may have no chain on this rank while its Hx still feeds the replicated duals
        p.foldCrown = fold_crown_mode(cs, a.cutSums != nullptr);
        // sharded (foldCrown = 2): one more workgroup per replicated crown node, which writes that node while the chains are walked
        p.nCrownWg = p.foldCrown == 2 ? h_stageCum[cs] : 0;
        const size_t fuseLds = fuse_lds();
        p.fuseSplit = fuse_split();                               // workgroups per chain of the fused launch
        const int fuseGrid = a.K * p.fuseSplit + p.nCrownWg;
        // (every workgroup leaves one entry in d_partials: trees with more chains than it holds take the two launches)
        p.fuse = bt.fuseReq && p.foldCrown && phase == 0 && !hess && fuseLds <= 64 * 1024 && fuseGrid <= std::max(ELT_MAX_BLOCKS, RN_DUAL_STAGE_MAX_BLOCKS);
        // structured mode, linear form, inner iteration of a batch: the NEXT sweep's chain walk rides in this launch (phase C) when that sweep
        // has a crown launch to host the bookkeeping workgroup the chain walk otherwise carries (one workgroup per chain only: the walk needs the chain's rows in one tile)
        p.upRide = p.fuse && p.lin && !bt.fuseMat && p.foldCrown == 1 && p.fuseSplit == 1 && (cs - 1 >= (p.foldRoot ? 1 : 0)) && knob[RN_KNOB_STRUCT_LINEAR] != 2;
        p.downGrid = p.fuse ? fuseGrid : a.K + p.nCrownWg;
        // inner iterations of an optimistic batch whose dual update is the stage-tiled kernel reading w: the walk leaves the primal values and
        // the dual update scales them (k_down_chain UNSC / k_dual_stage SCALE: the walk requests no preconditioner entries; bitwise the same Hx)
        p.unsc = !p.fuse && bt.optimistic && !a.writePrimal && phase == 0 && !hess && p.foldCrown && dualU != 0 && a.hx == d_hx && unscaled_on();
        return p;
    }
    size_t fuse_lds() const { return (size_t)d.N * ny * sizeof(T); }      // k_down_chain_dual: Hx of the chain's N - cs nodes and of up to cs crown nodes
    // The bookkeeping arguments of the launch that carries the previous iteration's fold (empty: this launch is not the one, or nothing is
    // pending -- the launch then has no extra workgroup).  Taking them clears Batch::pendingFin.  Sharded: the rank's dist^2 goes to the tail of
    // the cut payload and nothing is decided here (thresholds -1); single GPU: the distance check against the thresholds
    FinArgs take_fin(Batch &bt, const SweepPlan &p, FinRide here) {
        if (p.fin != here || !bt.pendingFin) return FinArgs{};
        bt.pendingFin = false;
        if (here == FIN_CUT) return FinArgs{d_partials, main_partials(), d_state, (void *)(d_cut + cut_tail_offset()), d_hist, d_histParts, histCap, -1.0, -1.0};
        return FinArgs{d_partials, main_partials(), d_state, nullptr, d_hist, d_histParts, histCap, penX / stepSize, penXs / stepSize};
    }
    // (2a) leaf-to-root vector recursion, the chains: one launch -- merged with the cut parents' local sums where the plan says so -- or none,
    // when the previous iteration's fused launch did the walk.  Clears Batch::upDone
    void sweep_chains_up(Batch &bt, const SweepPlan &p, SweepArgs<T> &a) {
        bt.upDone = false;
        if (p.mergedCut) {
            const int nPar = stage_nodes(cutStage - 1);
            const FinArgs fin = take_fin(bt, p, FIN_CUT);
            const size_t ldsCut = (size_t)(UPCUT_THREADS / p.cutLanes) * (d.nv + 2 * d.nx) * sizeof(T);
            hipLaunchKernelGGL(up_chain_cut_kernel(a.splitFirst < d.nodes, p.oneShot), dim3(nPar + (fin.partials ? 1 : 0)), dim3(UPCUT_THREADS), ldsCut, stream, a, d_cut, nPar, p.cutLanes, fin);
            if (p.oneShot) a.peer.nranks = 0;      // d_cut holds the all-rank sums: every later launch of this sweep is the collective path's
        } else if (p.phase != 2 && !p.rodeUp) {
            // single-GPU optimistic bookkeeping: the previous iteration's fold / history entry / distance check rides here
            const FinArgs fin = take_fin(bt, p, FIN_CHAIN);
            hipLaunchKernelGGL(up_chain_kernel(p.lin != 0, a.splitFirst < d.nodes), dim3(a.K + (fin.partials ? 1 : 0)), dim3(CHAIN_THREADS), 0, stream, a, fin);
        }
    }
    // (2b) multi-GPU: the children sums of the cut parents (stage k = cutStage - 1), all-reduced or pushed one-shot
    int sweep_exchange(Batch &bt, const SweepPlan &p, SweepArgs<T> &a, int k) {
        if (p.phase == 2) return RN_OK;              // payload already summed by the caller
        if (!p.mergedCut) {   // (k_up_chain_cut has already left the payload in d_cut)
            // optimistic exchange: the bookkeeping of the previous iteration's dual update rides in this launch
            const FinArgs fin = take_fin(bt, p, FIN_CUT);
            hipLaunchKernelGGL(cut_sums_kernel(p.oneShot), dim3(stage_nodes(k) + (fin.partials ? 1 : 0)), dim3(CUT_THREADS), 0, stream, a, d_cut, stage_nodes(k), fin);
            if (p.oneShot) a.peer.nranks = 0;      // d_cut holds the all-rank sums
        }
        if (p.phase == 1 || !has_comm()) return RN_OK;     // emulation, or a single-rank "sharded" run
        if (p.oneShot) return RN_OK;                       // the payload has gone to the peers' inboxes straight from the kernel
        const size_t cnt = (size_t)stage_nodes(k) * (d.nv + 2 * d.nx);
        return all_reduce(d_cut, cnt + (bt.carry_tail() ? 2 : 0), sizeof(T) == 8, "ncclAllReduce(cut payload)");
    }
    // (2c) the crown, stage by stage up to the root -- or to stage 1 where the v / Lv launch does the rest (foldRoot) -- with the exchange at the
    // cut in front of its stage.  Phase 1 ends behind the exchange
    int sweep_crown_up(Batch &bt, const SweepPlan &p, SweepArgs<T> &a) {
        const int w = d.nv + 2 * d.nx, wp = (w + 63) / 64 * 64;
        const size_t ldsCrown = (size_t)std::max(1, CROWN_THREADS / wp) * w * sizeof(T);
        for (int k = a.chainStage - 1; k >= (p.foldRoot ? 1 : 0); k--) {
            if (p.phase == 2 && k > cutStage - 1) continue;          // done in phase 1
            if (a.cutSums && k == cutStage - 1) {
                if (int rc = sweep_exchange(bt, p, a, k)) return rc;
                if (p.phase == 1) return RN_OK;
                if (p.foldRoot == 2) continue;                       // done by the v / Lv launch
            }
            if (p.lin) {
                const FinArgs fin = take_fin(bt, p, FIN_CROWN);      // (first crown launch of a sweep whose chain walk rode along)
                hipLaunchKernelGGL(k_up_crown_lin<T>, dim3(stage_nodes(k) + (fin.partials ? 1 : 0)), dim3(CROWN_THREADS), crown_lin_lds(p.lin), stream, a, k, stage_nodes(k), fin);
            }
            else hipLaunchKernelGGL(k_up_crown<T>, dim3(stage_nodes(k)), dim3(CROWN_THREADS), ldsCrown, stream, a, k);
        }
        return RN_OK;
    }
    // (4) root-to-leaf: u, x and Hx in one pass (crown, then the chains).  The chains' launch is the fused walk + dual update where the plan
    // says so (it answers Batch::fuseReq with fuseDone, and sets upDone when it carries the next sweep's chain walk), else k_down_chain -- which
    // sets Batch::hxUnscaled when it leaves the primal values in Hx
    int sweep_down(Batch &bt, const SweepPlan &p, SweepArgs<T> &a) {
        const int cs = a.chainStage;
        if (p.foldCrown) { if (int rc = ensure_chain_anc(cs)) return rc; a.chainAnc = d_chainAnc; }
        else if (p.fusedCrown) hipLaunchKernelGGL(k_down_crown_all<T>, dim3(1), dim3(CROWN_THREADS), 0, stream, a, cs);
        else for (int k = 0; k < cs; k++) hipLaunchKernelGGL(k_down_crown<T>, dim3(stage_nodes(k)), dim3(CHAIN_THREADS), 0, stream, a, k);
        if (p.fuse) {
            hipLaunchKernelGGL(down_chain_dual_kernel(bt.fuseMat, p.upRide), dim3(p.downGrid), dim3(CHAIN_THREADS), fuse_lds(), stream, a, p.foldCrown, bt.fuseArgs, bt.fuseLn, p.fuseSplit);
            if (p.upRide) bt.upDone = true;
            bt.fuseDone = true; mainPartials = p.downGrid;
        } else {
            hipLaunchKernelGGL(down_chain_kernel(p.unsc), dim3(p.downGrid), dim3(CHAIN_THREADS), 0, stream, a, p.foldCrown);
            if (p.unsc) bt.hxUnscaled = true;
        }
        return RN_OK;
    }
    // the steps behind the product (1) for one right-hand side, on the context's stream, as one interval of profiling class 1
    int sweep_steps(Batch &bt, const SweepPlan &p, SweepArgs<T> &a) {
        hipEvent_t e1 = prof_begin(1);
        sweep_chains_up(bt, p, a);
        if (int rc = sweep_crown_up(bt, p, a)) return rc;
        // (phase 1 ends behind the exchange, inside sweep_crown_up: with the cut payload set its loop always reaches stage cutStage - 1 --
        //  foldRoot is 0 outside phase 0 and the chains start at or below the cut -- so nothing of a phase-1 sweep is left to skip but (3) and (4))
        if (p.phase != 1) {
            // (3) v_i = m1_i - (Rinv s_i + Rinv Bbt kappa_i) / (2 p_i) ; lv_i = L v_i    (batched over all nodes, MFMA)
            launch_v_lv(a, p.foldRoot);
            if (int rc = sweep_down(bt, p, a)) return rc;
        }
        prof_end(e1);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // the second right-hand side of a pair: its input and first-product results (d_myB, d_qaB), its outputs where a Hessian sweep always leaves
    // them; ownScratch: a scratch set of its own for the steps, so that they can run beside the first right-hand side's
    SweepArgs<T> second_rhs_args(const SweepArgs<T> &a, const T *input, bool ownScratch) const {
        SweepArgs<T> b = a;
        b.w = input; b.my = d_myB; b.qa = d_qaB;
        b.x = d_xdir; b.u = d_udir; b.hx = d_hxDir;
        if (ownScratch) { b.sk = d_skB; b.rkq = d_rkqB; b.v = d_vB; b.lvb = d_lvbB; b.bw = d_bwB; }
        return b;
    }
    // phase: 0 = whole sweep; 1 = up to (and including) the cut parents' partial children sums; 2 = the rest,
    // assuming the summed payload is in d_cut (tests emulate the all-reduce between two contexts on one GPU)
    // hessianInput != nullptr: SmpcController::computeHessianOracalGlobalFbe (SmpcController.cu:884-1055) -- the same
    // sweep evaluated at `hessianInput` with sigma = 0 and every affine term zero, writing xdir / udir / H * dir
    // primalOut = false (inner iterations of a batch): x, u and v are not stored, only Hx (what the dual update reads)
    // (fp32-stored blocks on a context whose streaming launch has a split last round: THIS sweep runs unsplit -- a.splitFirst = nodes, which
    // every consumer of my2 follows: k_up_chain's selection, the v product's second partial -- and leaves d_my2 and the context's split alone)
    // hessianInput2 (with hessianInput; stream_pair_ok()): TWO Hessian sweeps whose inputs do not depend on each other's results share
    // ONE pass over the operator blocks (k_stream_gemv NR = 2); the vector recursions and shared-operator products then run once per
    // right-hand side.  The first sweep's results go to the pair buffers (d_xdirB, d_udirB, d_hxDirB), the second's where a Hessian
    // sweep always leaves them (d_xdir, d_udir, d_hxDir).  Bitwise the results of two launch_sweep calls.
    // batch: the rn_apg_iterate batch this sweep is an iteration of (nullptr: none -- the sweep then reads and writes a batch of its own, in which
    // every flag is false)
    // hessOut (with hessianInput, no pair): the Hessian sweep leaves x, u, H * dir and v in the caller's buffers instead of d_xdir, d_udir,
    // d_hxDir and d_v, and does not run the once-per-control-step refresh (lipschitz.inc: a context without FBE buffers, at any point
    // between two entry points)
    // certOut (no batch, no Hessian input, whole sweep; certificate.inc): the solve step evaluated at certOut->w instead of the accelerated dual,
    // with every affine term in place, leaving x, u, Hx and v in the caller's buffers: d_x, d_u, d_v, d_hx and primalSwept stay as they are, and a
    // pending v product -- whose input this sweep overwrites -- is run first
    struct HessOut { T *x, *u, *hx, *v; };
    struct CertOut { const T *w; T *x, *u, *hx, *v; };
    int launch_sweep(Batch *batch, int phase = 0, const T *hessianInput = nullptr, bool primalOut = true, const T *hessianInput2 = nullptr, const HessOut *hessOut = nullptr,
                     const CertOut *certOut = nullptr) {
        RN_CHECK(!hessOut || (hessianInput && !hessianInput2 && primalOut), RN_E_STATE, "launch_sweep: an output override belongs to a single Hessian sweep");
        RN_CHECK(!certOut || (!batch && phase == 0 && !hessianInput && primalOut), RN_E_STATE, "launch_sweep: a certificate sweep is a whole solve step outside a batch");
        Batch none{};
        Batch &bt = batch ? *batch : none;
        SweepArgs<T> a = sweep_args(bt);
        a.writePrimal = primalOut ? 1 : 0;
        if (primalOut && !hessianInput && !certOut) primalSwept = true;      // (rn_plan_report: d_x and d_u hold a plan from here on)
        if (vPending) { if (hessianInput || certOut) { if (int rc = v_flush()) return rc; } else vPending = false; }      // (see v_flush)
        if (certOut) { a.w = certOut->w; a.x = certOut->x; a.u = certOut->u; a.hx = certOut->hx; a.v = certOut->v; }
        if (hessianInput) {
            a.w = hessianInput;
            a.beta = d_zero; a.uhat = d_zero; a.e = d_zero; a.eb = d_zero; a.bw0 = d_zero;
            a.curX = d_zero; a.prevU = d_zero; a.prevUhat = d_zero;
            a.x = d_xdir; a.u = d_udir; a.hx = d_hxDir;
            if (hessOut) { a.x = hessOut->x; a.u = hessOut->u; a.hx = hessOut->hx; a.v = hessOut->v; }
        }
        const bool pair = hessianInput2 != nullptr;
        if (pair) {
            RN_CHECK(hessianInput && phase == 0 && d_myB && stream_pair_ok(), RN_E_STATE, "launch_sweep: a pair of sweeps needs two Hessian inputs, the pair buffers and a dense launch that can run unsplit");
            a.x = d_xdirB; a.u = d_udirB; a.hx = d_hxDirB;
            if (store32()) a.splitFirst = d.nodes;
        }
        RN_CHECK(phase == 0 || a.cutSums, RN_E_STATE, "rn_debug_sweep_phase needs rn_set_cut_stage and nranks > 1");
        const SweepPlan p = sweep_plan(bt, batch != nullptr, a, phase, hessianInput != nullptr);
        if (p.oneShot) {
            // 0 is the "never written" tag; the wrap skips TWO values (... fffffffe, ffffffff, 2, 3 ...) so that the parity -- which of the
            // two inbox buffers an exchange uses -- keeps alternating (the tag 2 of four billion exchanges ago is long overwritten)
            if (++peerSeq == 0) peerSeq = 2;
            a.peer = h_peer; a.peerSeq = peerSeq; a.peerTail = (bt.pendingFin && bt.carry_tail()) ? 1 : 0;
        }
        // (1) all per-node mat-vecs of the backward sweep in one streaming launch
        // (a Hessian sweep with outputs of its own -- the Lipschitz estimate -- reads none of them and may run before the affine terms exist: the
        //  refresh stays with the first sweep that needs it)
        if (aux_dirty && !hessOut) {   // iteration-invariant pieces of the forward sweep (once per control step)
            launch_gemm<EPI_Z>(d_Bp, d.nx, d.nu, d_uhat, d.nu, d_eb, d.nx, d_e, d.nx);            // eb_i = e_i + B uhat_i
            hipLaunchKernelGGL(k_bw0<>, dim3(1), dim3(128), 0, stream, (const void *)d_B, d.nx, d.nu, (const void *)d_prevU, (const void *)d_prevUhat, (void *)d_bw0, sizeof(T) == 8 ? 1 : 0);
            aux_dirty = false;
            linConstValid = false;      // (the affine terms may have changed: beta)
        }
        if ((p.lin & 2) && !hessianInput && !linConstValid) { if (int rc = lin_const_refresh(a)) return rc; }
        a.lin = p.lin;
        if (phase != 2 && p.form != FORM_LIN) {      // (the structured mode's linear form has no product in front of the chain walks: class 0 stays empty)
            hipEvent_t e0 = prof_begin(0);
            if (p.form == FORM_STRUCT) {
                launch_prep_m2(a);
            } else {
                const StreamRhs2<T> r2{hessianInput2, d_myB, d_qaB};
                if (int rc = launch_stream(a, pair ? &r2 : nullptr)) return rc;
            }
            prof_end(e0);
        }
        // (2) - (4) per right-hand side
        if (!pair) return sweep_steps(bt, p, a);
        const bool beside = stream2 && !prof;      // (while profiling every interval is bracketed on the one stream)
        SweepArgs<T> b = second_rhs_args(a, hessianInput2, beside);
        if (!beside) {
            if (int rc = sweep_steps(bt, p, a)) return rc;
            return sweep_steps(bt, p, b);
        }
        // the two right-hand sides' helper chains (five dependent, latency-bound launches each) do not touch each other's buffers:
        // the second runs on a stream of its own with a scratch set of its own, forked behind the streaming pass and joined here
        RN_HIP(hipEventRecord(evFork, stream));
        RN_HIP(hipStreamWaitEvent(stream2, evFork, 0));
        std::swap(stream, stream2);
        int rcB = sweep_steps(bt, p, b);
        if (rcB == RN_OK && hipEventRecord(evJoin, stream) != hipSuccess) rcB = RN_E_HIP;
        std::swap(stream, stream2);
        if (rcB) return rcB;
        if (int rc = sweep_steps(bt, p, a)) return rc;
        RN_HIP(hipStreamWaitEvent(stream, evJoin, 0));
        return RN_OK;
    }
    // launch shape of k_dual_stage: one tile of ELT_THREADS * trips 16-byte vectors per workgroup, tiles never cross a stage
    void dual_stage_setup() {
        dualU = 0; dualBlocks = eltBlocks;
        constexpr int VN = 16 / (int)sizeof(T);
        if (!RN_DUAL_REGEN || !RN_DUAL_STAGE || ny % VN) return;
        const int vpn = ny / VN, cs = chainStage, K = h_stageCum[cs + 1] - h_stageCum[cs], node0 = h_stageCum[cs];
        if (vpn < 2) return;   // one vector per node: floor(2^32 / 1) + 1 does not fit the 32-bit magic -- the flat kernel runs
        const unsigned long long lim = (1ull << 32) / (unsigned)vpn;          // range in which umulhi(j, magic) == j / vpn
        if ((unsigned long long)K * vpn >= lim || (unsigned long long)node0 * vpn >= lim || (unsigned long long)d.nodes * vpn >= (1ull << 31)) return;
        const int forced = knob[RN_KNOB_DUAL_TRIPS] > 0 ? knob[RN_KNOB_DUAL_TRIPS] : 0;
        // workgroups: at most one resident round (numCUs x 8 workgroups of 4 waves) so that every workgroup's loads start at
        // once; measured on the 493-scenario tree: 1 trip (5 113 workgroups) 21.9 us, 2-3 trips 20.8, 4-6 trips 21.6-24 us
        // vectors that do not fit the 256 MiB Infinity Cache stream from HBM: there 4x as many (smaller) workgroups and the
        // double-buffered variant measured best (wide4096 fp32, 1.3 GB per launch: 279 -> 257 us)
        const bool cacheResident = 5.0 * (double)ntot() * sizeof(T) <= 256.0 * 1024 * 1024;
        const long long resident = std::min<long long>((long long)numCUs * (cacheResident ? 8 : 32), RN_DUAL_STAGE_MAX_BLOCKS);   // d_partials holds that many
        for (int pass = 0; pass < 2 && dualU == 0; pass++)
            for (int trips : {1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 48, 64}) {
                if (forced > 0 && trips != forced) continue;
                const long long tile = (long long)ELT_THREADS * trips;
                const long long bps = ((long long)K * vpn + tile - 1) / tile, cb = ((long long)node0 * vpn + tile - 1) / tile;
                const long long blocks = cb + bps * (d.N - cs);
                if (blocks > (pass == 0 && forced <= 0 ? resident : (long long)RN_DUAL_STAGE_MAX_BLOCKS)) continue;
                dshape = DualStageShape{cs, K, node0, (int)bps, (int)cb, vpn, (unsigned int)((1ull << 32) / (unsigned)vpn) + 1u, trips, 0.0};
                dualU = (!cacheResident && trips >= 2) ? 2 : 1;
                if (knob[RN_KNOB_DUAL_PIPE] > 0) dualU = knob[RN_KNOB_DUAL_PIPE] >= 2 ? 2 : 1;
                dualBlocks = (int)blocks;
                break;
            }
    }
    // main pass of the fused dual update (prox as a pure projection, residual, dual update, arg-max partials, next
    // extrapolation): the stage-tiled k_dual_stage, or the flat grid-stride k_dual_fused (eltBlocks partials) where the shape is not eligible
    // and in exact sharded batches, whose fix-up pass and k_finalize fold eltBlocks partials (run_batch; rn_get_kernel_info reports the same rule)
    bool dual_main_flat(bool optimisticBatch) const { return dualU == 0 || (!optimisticBatch && has_comm() && cutStage > 0); }
    typedef void (*DualFusedKernel)(DualArgs<T>);
    typedef void (*DualStageKernel)(DualArgs<T>, DualStageShape);
    static DualFusedKernel dual_fused_kernel(bool materialize, bool fixup) {
        return fixup ? (materialize ? k_dual_fused<T, true, true> : k_dual_fused<T, false, true>) : (materialize ? k_dual_fused<T, true, false> : k_dual_fused<T, false, false>);
    }
    // (SCALE -- Hx = sqrt(p_i) d_k * (primal value) is formed by the kernel, behind an unscaled walk -- exists for the non-materialising pass only)
    static DualStageKernel dual_stage_kernel(bool materialize, int pipe, bool scale) {
        if (scale) return pipe == 1 ? k_dual_stage<T, false, 1, true> : k_dual_stage<T, false, 2, true>;
        if (materialize) return pipe == 1 ? k_dual_stage<T, true, 1> : k_dual_stage<T, true, 2>;
        return pipe == 1 ? k_dual_stage<T, false, 1> : k_dual_stage<T, false, 2>;
    }
    // "build the arguments" / "launch them", as v_lv_args / run_v_lv: what the main pass of ONE iteration is -- which kernel, how many workgroups
    // (= partials), whether Hx has to be scaled in front -- and the launch of exactly that.  run_batch (launch_dual_main) and rn_debug_dual_update
    // go through the same two steps.
    struct DualMainLaunch {
        bool flat, scale, preScale;   // k_dual_fused / k_dual_stage; SCALE instantiation; k_hx_scale in front (unscaled Hx that SCALE cannot take)
        int blocks, pipe;
        DualStageShape g;             // (stage-tiled only; lnNext filled in)
    };
    DualMainLaunch dual_main_args(bool flat, bool hxUnscaled, bool materialize, double lnNext) const {
        DualMainLaunch m{};
        m.flat = flat;
        m.scale = hxUnscaled && !materialize && !flat;      // unscaled walk: k_dual_stage SCALE forms Hx; every other consumer gets it scaled first
        m.preScale = hxUnscaled && !m.scale;
        m.blocks = flat ? eltBlocks : dualBlocks;
        m.pipe = flat ? 0 : dualU;
        if (!flat) { m.g = dshape; m.g.lnNext = lnNext; }
        return m;
    }
    void run_dual_main(const DualMainLaunch &m, const DualArgs<T> &a, bool materialize) {
        if (m.flat) {
            hipLaunchKernelGGL(dual_fused_kernel(materialize, false), dim3(m.blocks), dim3(ELT_THREADS), 0, stream, a);
            return;
        }
        hipLaunchKernelGGL(dual_stage_kernel(materialize, m.pipe, m.scale), dim3(m.blocks), dim3(ELT_THREADS), 0, stream, a, m.g);
    }
    void launch_dual_main(Batch &b, const DualArgs<T> &a, bool materialize) {
        const bool hxUnscaled = std::exchange(b.hxUnscaled, false);
        // ensure_tables(h_it + n) has run: the table covers every iteration of the batch
        const DualMainLaunch m = dual_main_args(dual_main_flat(b.optimistic), hxUnscaled, materialize, h_lam[h_it + 1 - lamBase]);
        if (m.preScale) hx_scale_now(d_hx);
        mainPartials = m.blocks;
        run_dual_main(m, a, materialize);
    }
    // The bookkeeping of an iteration that gets launches of its own, in the three forms run_batch knows (the fourth rides in the next sweep: FinArgs).
    // Everything they touch arrives in the DualArgs (state, partials, history) and in the parameters: rn_debug_dual_update hands them scratch.
    // optimistic: fold, history entry, distance check into the verdict flag (single GPU) or the dist^2 into the cut payload's tail (sharded)
    void run_close_optimistic(const DualArgs<T> &a, int nMain, T *tail, bool sharded, int recFirst, int recN, double recTol, BatchRecord *hostRec) {
        hipLaunchKernelGGL(k_finalize_optimistic<T>, dim3(1), dim3(ELT_THREADS), 0, stream, (const Partial *)a.partials, nMain, a.st, tail, a.hist, a.histParts,
                           a.histCap, sharded ? -1.0 : a.thrX, sharded ? -1.0 : a.thrS, recFirst, sharded ? -1 : recN, recTol, sharded ? nullptr : hostRec);
    }
    // exact, sharded: tree-global distances -- sum the ranks' dist^2 (2 doubles) before deciding; the flat fix-up pass; the history entry
    int run_close_exact_sharded(const DualArgs<T> &a, bool materialize, double *dist2) {
        hipLaunchKernelGGL(k_reduce_dist<>, dim3(1), dim3(ELT_THREADS), 0, stream, (const Partial *)a.partials, eltBlocks, dist2);
        if (has_comm()) { if (int rc = all_reduce(dist2, 2, true, "ncclAllReduce(dist)")) return rc; }
        hipLaunchKernelGGL(k_decide_from<>, dim3(1), dim3(1), 0, stream, (const double *)dist2, a.st, a.thrX, a.thrS);
        hipLaunchKernelGGL(dual_fused_kernel(materialize, true), dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a);
        hipLaunchKernelGGL(k_finalize<>, dim3(1), dim3(ELT_THREADS), 0, stream, (const Partial *)a.partials, eltBlocks, a.st, a.hist, a.histParts, a.histCap);
        return RN_OK;
    }
    // exact, single GPU: the (small) fix-up launch also decides and does the bookkeeping (k_dual.hpp, decideHere).  The arguments first -- the
    // caller may add a batch record to them -- then the launch.
    DualArgs<T> exact_fixup_args(DualArgs<T> a, int itHost, int nMain, Partial *fixPartials) const {
        a.finalizedEarly = 1;
        a.decideHere = 1; a.itHost = itHost; a.nMain = nMain; a.mainPartials = a.partials; a.partials = fixPartials;
        return a;
    }
    int exact_fixup_blocks() const { return std::min(eltBlocks, RN_FIXUP_BLOCKS); }
    void run_exact_fixup(const DualArgs<T> &a, bool materialize) {
        hipLaunchKernelGGL(dual_fused_kernel(materialize, true), dim3(exact_fixup_blocks()), dim3(ELT_THREADS), 0, stream, a);
    }
