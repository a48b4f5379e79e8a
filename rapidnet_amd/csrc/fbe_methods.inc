// fbe_methods.inc -- members of rn::Ctx<T> for the global-FBE and NAMA outer loops (included inside the struct body
// of rapidnet_capi.hip).  Reference: SmpcController.cu:884-1476 (steps), 1529-1586 (loops).  The control flow that
// depends on computed scalars (L-BFGS skip rule, line-search acceptance) runs on the host exactly as the reference
// does; everything that touches a vector is a kernel of fbe_kernels.hpp or the tree sweep of kernels.hpp.
    int algorithm = 0;   // RN_ALG_APG / RN_ALG_GLOBAL_FBE / RN_ALG_NAMA
    int lbfgsSize = 0, lbfgsCol = 0, lbfgsMem = 0, lbfgsSkip = 0;
    double lbfgsH = 1;
    std::vector<double> h_rho;   // lbfgsBufferRho, lbfgsSize + 1 entries (columns 1..lbfgsSize are addressed, see below)
    // y-layout vectors: previous dual, current / previous L-BFGS "Yvec" (FBE gradient or NAMA residual), direction,
    // H * (x direction); per-node x / u directions; scratch S, Y; the L-BFGS buffers; a zero block for the oracle
    T *d_prevY = nullptr, *d_g = nullptr, *d_gPrev = nullptr, *d_dir = nullptr, *d_hxDir = nullptr;
    T *d_xdir = nullptr, *d_udir = nullptr, *d_S = nullptr, *d_Yv = nullptr, *d_matS = nullptr, *d_matY = nullptr, *d_zero = nullptr;
    T *d_W = nullptr;
    bool lastPairAccepted = false, preDotValid = false;      // value_and_buffer -> lbfgs_two_loop_impl: the recursion's first dot product is already reduced
    const double *preDotPartials = nullptr, *preDotScal = nullptr;
    T *d_S0 = nullptr, *d_Yv0 = nullptr;       // the scratch pair as allocated (fbe_reset puts every column back where it was allocated)
    std::vector<T *> h_colS, h_colY;           // where the L-BFGS columns live
    double *d_dotPartials = nullptr, *d_dotPartials2 = nullptr, *d_valPartials = nullptr, *d_scal = nullptr, *d_alphaArr = nullptr;
    int valueBlocks = 1;
    // the line search with all candidates evaluated at once (fbe_kernels.hpp, k_ls_*): per-block partials and the folded scalars
    double *d_lsEval = nullptr, *d_lsVal = nullptr, *d_lsScal = nullptr;
    // NAMA's pair of Hessian sweeps in one pass over the operator blocks (launch_sweep, hessianInput2): the second right-hand side's
    // [m1; m2] / a_i and the first one's results
    T *d_myB = nullptr, *d_qaB = nullptr, *d_xdirB = nullptr, *d_udirB = nullptr, *d_hxDirB = nullptr;
    // ... and the second right-hand side's helper chain on a stream of its own (launch_sweep): its scratch set, the fork / join events
    T *d_skB = nullptr, *d_rkqB = nullptr, *d_vB = nullptr, *d_lvbB = nullptr, *d_bwB = nullptr;
    hipStream_t stream2 = nullptr;
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    long sweepPairs = 0;
    // the value's primal terms on the matrix cores (k_value_mfma): W stored padded like the sweep's shared operators
    T *d_Wp = nullptr;
    bool valueMfma = false;
    // one workgroup per CU walks the slabs b, b + grid, ...: its W fragments are fetched once
    int vmBlocks() const { return std::min((d.nodes + 15) / 16, numCUs); }
    double *d_infHist = nullptr; int infHistCap = 0;   // the loops' primal infeasibilities, four parts per iteration (read back once per call)
    int lsValueBlocks = 1;
    bool lsFused = false;   // the fused evaluation is available (its LDS tile fits)
    long lsSearches = 0, lsBatches = 0, lsSequential = 0;   // searches run, candidate batches evaluated, searches sent down the sequential path

    int set_algorithm(int alg, int bufferSize) override {
        RN_CHECK(alg == RN_ALG_APG || alg == RN_ALG_GLOBAL_FBE || alg == RN_ALG_NAMA, RN_E_ARG, "rn_set_algorithm: unknown algorithm");
        if (alg == RN_ALG_APG) { algorithm = alg; return RN_OK; }
        RN_CHECK(bufferSize >= 1 && bufferSize <= 32, RN_E_ARG, "rn_set_algorithm: lbfgsBufferSize must be in [1, 32]");
        RN_CHECK(lbfgsSize == 0 || lbfgsSize == bufferSize, RN_E_STATE, "rn_set_algorithm: lbfgsBufferSize cannot change");
        RN_HIP(hipSetDevice(device));
        if (!d_matS) {
            const size_t n = (size_t)ntot(), N_ = d.nodes;
            // the reference allocates lbfgsSize columns and addresses columns 1..lbfgsSize (SmpcController.cu:1146,
            // 256-257); one spare column keeps the same indexing inside the allocation
#define DA(ptr, cnt) if (int rc = dalloc(&ptr, (size_t)(cnt))) return rc;
            DA(d_prevY, n) DA(d_g, n) DA(d_gPrev, n) DA(d_dir, n) DA(d_hxDir, n) DA(d_S, n) DA(d_Yv, n)
            DA(d_xdir, N_ * d.nx) DA(d_udir, N_ * d.nu)
            DA(d_matS, (size_t)(bufferSize + 1) * n) DA(d_matY, (size_t)(bufferSize + 1) * n)
            if (!d_zero) { DA(d_zero, N_ * (size_t)std::max(d.nu, std::max(d.nx, d.nv))) }      // (an earlier rn_estimate_lipschitz may have made it)
            valueBlocks = std::min((d.nodes + VALUE_TILE - 1) / VALUE_TILE, 1024);
            DA(d_dotPartials, (size_t)ELT_MAX_BLOCKS * DOT_MAX) DA(d_dotPartials2, (size_t)ELT_MAX_BLOCKS * DOT_MAX) DA(d_valPartials, (size_t)valueBlocks * DOT_MAX)
            DA(d_scal, FBE_SCALARS) DA(d_alphaArr, 64)
            lsValueBlocks = std::min((d.nodes + LS_TILE - 1) / LS_TILE, 1024);
            DA(d_infHist, 4 * 1024) infHistCap = 1024;
            DA(d_lsEval, (size_t)ELT_MAX_BLOCKS * LS_K * LS_EVAL) DA(d_lsVal, (size_t)lsValueBlocks * LS_K * 2) DA(d_lsScal, LS_K * LS_SCAL)
#undef DA
            {   // the candidates' du tiles in LDS: [LS_K][nu][LS_TILE]; more than 64 KB needs the function attribute, more than the CU has: sequential search
                // (the attribute asks for what the tile needs: the kernel's static arrays share the CU's 160 KB, so asking for all of it is refused)
                const size_t ldsLs = (size_t)LS_K * d.nu * LS_TILE * sizeof(T);
                lsFused = ldsLs <= 160 * 1024 &&
                          (ldsLs <= 64 * 1024 || hipFuncSetAttribute((const void *)k_ls_value<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsLs) == hipSuccess);
                (void)hipGetLastError();
                if (knob[RN_KNOB_LS_SEQUENTIAL] > 0) lsFused = false;   // A/B runs, tests: the trial-by-trial search
            }
            {   // W for k_value_mfma (a slab's elements fit the per-thread registers for nu <= 32 VM_MAXE; RAPIDNET_VALUE_MFMA=0: the vector-ALU kernels)
                bool want = 16 * d.nu <= 64 * VM_WAVES * VM_MAXE;
                if (knob[RN_KNOB_VALUE_MFMA] == 0) want = false;
                if (want) {
                    if (int rc = dalloc(&d_Wp, (size_t)pad16(d.nu) * pad4(d.nu))) return rc;
                    if (factored) {     // W is on the device already (otherwise the factor step fills d_Wp as well)
                        std::vector<T> hw((size_t)d.nu * d.nu);
                        RN_HIP(hipMemcpyAsync(hw.data(), d_W, hw.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
                        RN_HIP(hipStreamSynchronize(stream));
                        std::vector<double> hd(hw.begin(), hw.end());
                        if (int rc = upload_padded(d_Wp, hd.data(), d.nu, d.nu)) return rc;
                    }
                    valueMfma = true;
                }
            }
            RN_HIP(hipMemsetAsync(d_zero, 0, N_ * (size_t)std::max(d.nu, std::max(d.nx, d.nv)) * sizeof(T), stream));
            for (T *v : {d_prevY, d_g, d_gPrev, d_dir, d_hxDir, d_S, d_Yv}) RN_HIP(hipMemsetAsync(v, 0, n * sizeof(T), stream));
            RN_HIP(hipMemsetAsync(d_xdir, 0, N_ * d.nx * sizeof(T), stream));
            RN_HIP(hipMemsetAsync(d_udir, 0, N_ * d.nu * sizeof(T), stream));
            lbfgsSize = bufferSize;
            d_S0 = d_S; d_Yv0 = d_Yv;
            h_rho.assign((size_t)bufferSize + 1, 0.0);
        }
        if (alg == RN_ALG_NAMA) { if (int rc = ensure_pair_buffers()) return rc; }
        algorithm = alg;
        return fbe_reset();
    }
    // NAMA's pair buffers, the second helper chain's scratch set, its stream and the events: allocated once, when the context could pair (dense
    // blocks; fp32-stored ones behind RN_PAIR_ON only -- rn_set_sweep_pairing) and RN_KNOB_NAMA_PAIR does not force the sequential path
    int ensure_pair_buffers() {
        if (d_myB || structured || pairReq == RN_PAIR_OFF || (store32() && pairReq != RN_PAIR_ON) || knob[RN_KNOB_NAMA_PAIR] == 0) return RN_OK;
        const size_t n = (size_t)ntot(), N_ = d.nodes;
        if (int rc = dalloc(&d_qaB, N_ * d.nx)) return rc;
        if (int rc = dalloc(&d_xdirB, N_ * d.nx)) return rc;
        if (int rc = dalloc(&d_udirB, N_ * d.nu)) return rc;
        if (int rc = dalloc(&d_hxDirB, n)) return rc;
        if (int rc = dalloc(&d_skB, N_ * (d.nv + d.nx))) return rc;
        if (int rc = dalloc(&d_rkqB, N_ * (d.nv + 2 * d.nx))) return rc;
        if (int rc = dalloc(&d_vB, N_ * d.nv)) return rc;
        if (int rc = dalloc(&d_lvbB, N_ * (d.nu + d.nx))) return rc;
        if (int rc = dalloc(&d_bwB, N_ * d.nx)) return rc;
        if (!stream2) RN_HIP(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
        if (!evFork) RN_HIP(hipEventCreateWithFlags(&evFork, hipEventDisableTiming));
        if (!evJoin) RN_HIP(hipEventCreateWithFlags(&evJoin, hipEventDisableTiming));
        return dalloc(&d_myB, N_ * 2 * d.nv);      // (last: d_myB != nullptr says the whole set is there)
    }
    // the context as it stands pairs the two Hessian sweeps of its next NAMA line search
    // (cutStage <= 0: a cut context -- even one without a communicator, which RN_FBE_READY allows -- keeps ONE cut buffer d_cut, and the two
    //  helper chains of the pair would both write and read it)
    bool pair_active() const { return d_myB && stream_pair_ok() && !fbe_sharded() && cutStage <= 0; }
    // SmpcController::initialiseAlgorithm (FBE / NAMA part, :436-449) + initaliseLbfgBuffer (:453-468)
    int fbe_reset() override {
        RN_CHECK(algorithm != RN_ALG_APG && d_matS, RN_E_STATE, "rn_fbe_reset: select RN_ALG_GLOBAL_FBE or RN_ALG_NAMA first");
        if (int rc = apg_reset()) return rc;
        const size_t bytes = (size_t)ntot() * sizeof(T);
        RN_HIP(hipMemsetAsync(d_prevY, 0, bytes, stream));
        if (algorithm == RN_ALG_GLOBAL_FBE) RN_HIP(hipMemsetAsync(d_g, 0, bytes, stream));
        else RN_HIP(hipMemsetAsync(d_res, 0, bytes, stream));
        RN_HIP(hipMemsetAsync(d_matS, 0, bytes * (lbfgsSize + 1), stream));
        RN_HIP(hipMemsetAsync(d_matY, 0, bytes * (lbfgsSize + 1), stream));
        // logical column c lives in h_colS[c] / h_colY[c]; updates exchange a column with the scratch pair (d_S, d_Yv) instead of copying
        d_S = d_S0; d_Yv = d_Yv0;
        h_colS.resize((size_t)lbfgsSize + 1); h_colY.resize((size_t)lbfgsSize + 1);
        for (int c = 0; c <= lbfgsSize; c++) { h_colS[c] = d_matS + (size_t)c * ntot(); h_colY[c] = d_matY + (size_t)c * ntot(); }
        lbfgsCol = 0; lbfgsMem = 0; lbfgsSkip = 0; lbfgsH = 1;
        preDotValid = false;
        std::fill(h_rho.begin(), h_rho.end(), 0.0);
        return RN_OK;
    }
#define RN_FBE_READY(what) RN_CHECK(algorithm != RN_ALG_APG && d_matS, RN_E_STATE, what ": select RN_ALG_GLOBAL_FBE or RN_ALG_NAMA first"); \
                           RN_CHECK(factored && affine_ready, RN_E_STATE, what " before the factor step / affine terms"); \
                           RN_CHECK(cutStage <= 0 || nranks == 1 || has_comm(), RN_E_STATE, what ": a shard of several ranks needs a communicator (rn_comm_init with an id, " \
                                    "or an installed all-reduce): the loops' dot products, value terms and distances are tree-global"); \
                           RN_HIP(hipSetDevice(device));

    // Sharded contexts: every reduction of the loops is tree-global.  The replicated crown counts on rank 0 only (dot_first /
    // value_first_node are where the other ranks start counting) and every finished group of scalars is all-reduced over the
    // ranks, so all of them see the same values and take the same skip / line-search decisions.
    bool fbe_sharded() const { return cutStage > 0 && has_comm(); }
    // (only where the scalars ARE all-reduced: a cut context without communicator -- one rank driving the sharded code path --
    //  counts its whole local tree, crown included)
    long long dot_first() const { return (fbe_sharded() && rank != 0) ? (long long)h_stageCum[cutStage] * ny : 0; }
    int value_first_node() const { return (fbe_sharded() && rank != 0) ? h_stageCum[cutStage] : 0; }
    int reduce_scalars(double *p, int cnt) { return fbe_sharded() ? all_reduce(p, (size_t)cnt, true, "ncclAllReduce(FBE scalars)") : RN_OK; }
    // up to DOT_MAX dot products over the y range -> d_scal[0..cnt)
    int launch_dots(std::initializer_list<std::pair<const T *, const T *>> pairs) {
        DotArgs<T> g{};
        int c = 0;
        for (auto &p : pairs) { g.a[c] = p.first; g.b[c] = p.second; c++; }
        g.cnt = c; g.n = ntot(); g.partials = d_dotPartials; g.first = dot_first();
        hipLaunchKernelGGL(k_dots<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, g);
        hipLaunchKernelGGL(k_dots_finish<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_dotPartials, eltBlocks, c, d_scal);
        RN_HIP(hipGetLastError());
        return reduce_scalars(d_scal, c);
    }
    int read_scalars(double *host, int first, int n) {
        RN_HIP(hipMemcpyAsync(host, d_scal + first, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        return RN_OK;
    }
    // proximalFunG + computeFixedPointResidual (+ the negated residual both quasi-Newton loops continue with) in ONE pass
    // over the duals instead of four launches; <w, res> and <res, res> -- what computeValueFbe needs of these vectors -- are
    // reduced on the way and left in d_scal[0..1] (value_fbe_impl(.., true) picks them up).  Same values as the step-wise calls.
    int prox_residual(T *gneg) {
        DualArgs<T> a = dual_args();
        a.w = p_acc_view;
        hipLaunchKernelGGL(k_prox_res<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a, gneg, d_dotPartials);
        if (fbe_sharded()) {   // tree-global distances: the ranks' dist^2 summed before the trip decision (SmpcController.cu:792, :810)
            hipLaunchKernelGGL(k_reduce_dist<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_partials, eltBlocks, d_dist2);
            if (int rc = all_reduce(d_dist2, 2, true, "ncclAllReduce(dist)")) return rc;
            hipLaunchKernelGGL(k_decide_from<>, dim3(1), dim3(1), 0, stream, d_dist2, d_state, a.thrX, a.thrS);
        } else hipLaunchKernelGGL(k_decide<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_partials, eltBlocks, d_state, a.thrX, a.thrS);
        hipLaunchKernelGGL(k_prox_soft_res<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a, gneg, d_dotPartials);
        hipLaunchKernelGGL(k_dots_finish<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_dotPartials, eltBlocks, 2, d_scal);
        RN_HIP(hipGetLastError());
        return reduce_scalars(d_scal, 2);
    }
    // SmpcController::computeHessianOracalGlobalFbe (:884-1055): the tree sweep with sigma = 0 and no affine terms
    int hessian_sweep(const T *in) {
        return launch_sweep(nullptr, 0, in);
    }
    int hessian_oracle() override {   // input = what devPtrVecHessianOracleXi/Psi point at (:356-357, :408-409)
        RN_FBE_READY("rn_compute_hessian_oracle")
        return hessian_sweep(algorithm == RN_ALG_NAMA ? d_res : d_g);
    }
    // SmpcController::computeGradientFbe (:1077-1097)
    int gradient_fbe() override { return gradient_fbe_impl(false); }
    // negDone: g = -res has already been written by the fused prox (prox_residual)
    int gradient_fbe_impl(bool negDone) {
        RN_FBE_READY("rn_compute_gradient_fbe")
        if (!negDone) hipLaunchKernelGGL(k_axpby<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_g, d_res, d_res, (T)-1, (T)0, ntot());
        if (int rc = hessian_sweep(d_g)) return rc;
        hipLaunchKernelGGL(k_axpby<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_g, d_g, d_hxDir, (T)1, (T)stepSize, ntot());
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // SmpcController::updateFixedPointResidualNamaAlgorithm (:1060-1072)
    int nama_residual() override {
        RN_FBE_READY("rn_update_fixed_point_residual_nama")
        hipLaunchKernelGGL(k_axpby<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_g, d_res, d_res, (T)-1, (T)0, ntot());
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // SmpcController::computeLbfgsDirection = updateLbfgsBuffer (:1103-1169) + twoLoopRecursionLbfgs (:1175-1229).  Called as
    // one step, the "direction := -gradient" that ends the first half rides in the first pass of the second
    int lbfgs_direction() override {
        if (int rc = lbfgs_update_buffer_impl(false)) return rc;
        return lbfgs_two_loop_impl(true);
    }
    int lbfgs_update_buffer() override { return lbfgs_update_buffer_impl(true); }
    int lbfgs_two_loop() override { return lbfgs_two_loop_impl(false); }
    // SmpcController::updateLbfgsBuffer (:1103-1169): s / y differences, skip rule, buffer column, H0 scaling, direction := -g
    int lbfgs_update_buffer_impl(bool writeDirection) {
        RN_FBE_READY("rn_update_lbfgs_buffer")
        buffer_launch(d_scal);
        RN_HIP(hipGetLastError());
        if (int rc = reduce_scalars(d_scal, 4)) return rc;
        double sc[4];
        if (int rc = read_scalars(sc, 0, 4)) return rc;
        return buffer_host(sc, writeDirection);
    }
    // the device half: S, Y and the four dot products of the skip rule / scaling in one pass (was k_lbfgs_diffs + k_dots) -> out[0..4)
    // extra: also the two candidates for the dot product the two-loop recursion starts with (k_lbfgs_diffs_dots) -> out[4], out[5]
    void buffer_launch(double *out, bool extra = false) {
        const long long n = ntot();
        const T *sPrev = (extra && lbfgsMem > 0) ? (const T *)h_colS[lbfgsCol] : nullptr;
        hipLaunchKernelGGL(k_lbfgs_diffs_dots<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_S, d_Yv, p_xi, d_prevY, d_g, d_gPrev, d_dotPartials, n, dot_first(),
                           extra ? 1 : 0, sPrev);
        hipLaunchKernelGGL(k_dots_finish<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_dotPartials, eltBlocks, extra ? 6 : 4, out);
    }
    // the host half, on the four (tree-global) scalars
    int buffer_host(const double *sc, bool writeDirection) {
        const long long n = ntot();
        lastPairAccepted = false;
        T normGrad = (T)std::sqrt(sc[0]);
        const T invRho = (T)sc[1], normY = (T)std::sqrt(sc[2]), normS = (T)std::sqrt(sc[3]);
        if (normGrad < 1) normGrad = normGrad * normGrad * normGrad;                               // :1133-1135
        if (invRho / (normS * normS) > (T)1e-6 * normGrad) {                                       // :1137
            lbfgsCol = 1 + (lbfgsCol % lbfgsSize);
            lbfgsMem = std::min(lbfgsMem + 1, lbfgsSize);
            // the new pair becomes column lbfgsCol by exchanging buffers (the column it replaces becomes the scratch pair the next
            // update writes): no copy of two n-vectors
            std::swap(h_colY[lbfgsCol], d_Yv);
            std::swap(h_colS[lbfgsCol], d_S);
            lastPairAccepted = true;
            h_rho[lbfgsCol] = (double)((T)1 / invRho);
        } else lbfgsSkip++;
        const T gammaH = invRho / (normY * normY);                                                 // :1151-1156
        if (gammaH < 0 || std::fabs((double)(gammaH - (T)lbfgsH)) == 0) lbfgsH = 1; else lbfgsH = (double)gammaH;
        if (writeDirection) hipLaunchKernelGGL(k_axpby<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_dir, d_g, d_g, (T)-1, (T)0, n);   // :1158-1161
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // SmpcController::twoLoopRecursionLbfgs (:1175-1229).  Every step is ONE pass over the direction that also reduces the dot
    // product the next step needs (k_lbfgs_fused; the reference and the first version here: a dot launch + an axpy launch per
    // step); the coefficients stay on the device.  directionFromGradient: start from -g instead of reading the direction.
    int lbfgs_two_loop_impl(bool directionFromGradient) {
        RN_FBE_READY("rn_two_loop_recursion_lbfgs")
        const long long n = ntot();
        auto col1 = [&](int is) { int c = lbfgsCol - is; if (c < 0) c = lbfgsMem + c; return c; };           // first loop, is = 0 .. mem-1
        auto col2 = [&](int is) { int c = lbfgsCol - is + 1; if (c < 0) c = lbfgsMem + c; return c; };       // second loop, is = mem .. 1
        int arc = RN_OK;
        // One GPU: a step's dot product is folded from its partials by every workgroup of the NEXT step (fold_dot0: bitwise
        // what k_dots_finish computes), so the recursion is 2 m + 2 launches instead of 4 m + 3; the partial buffers alternate
        // because a step writes its own partials while others still read the previous step's.  Sharded contexts keep the
        // finish launch: the scalar has to be all-reduced before anybody uses it.
        const bool foldInConsumer = !fbe_sharded();
        double *pbuf[2] = {d_dotPartials, d_dotPartials2};
        int cur = 0;                       // buffer the next producing step writes
        const double *pending = nullptr;   // partials of the dot product the next consuming step needs
        const double *scalIn = d_scal;     // where a step finds the dot product when it does not fold it itself
        T srcScale = 0;
        auto fused = [&](const T *src, const T *vec, double rho, int c, int mode, T scale, const T *next, int post = 0) {
            double *mine = pbuf[cur];
            hipLaunchKernelGGL(k_lbfgs_fused<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_dir, src, vec, scalIn, rho, d_alphaArr, c, mode, scale, next,
                               mine, n, dot_first(), mode >= 0 ? pending : nullptr, eltBlocks, post, srcScale);
            scalIn = d_scal; srcScale = 0;
            pending = nullptr;
            if (next) {
                if (foldInConsumer) { pending = mine; cur ^= 1; }
                else {
                    hipLaunchKernelGGL(k_dots_finish<>, dim3(1), dim3(ELT_THREADS), 0, stream, mine, eltBlocks, 1, d_scal);
                    if (arc == RN_OK) arc = reduce_scalars(d_scal, 1);
                }
            }
        };
        const T *firstS = lbfgsMem > 0 ? h_colS[col1(0)] : nullptr;
        // inside the loops the start of the recursion (dir = -gradient and <newest S, dir>) rides in the first step: the dot product came
        // out of k_lbfgs_diffs_dots as <S, g> (value_and_buffer), so the step runs with -rho and +<S, g> (the same product, exactly) and
        // forms -g on the fly instead of reading the direction
        const bool startRides = directionFromGradient && preDotValid && lbfgsMem > 0;
        preDotValid = false;
        if (startRides) {
            if (foldInConsumer) { pending = preDotPartials; cur = 1; }      // the partials live in pbuf[0]: the first step writes pbuf[1]
        } else if (directionFromGradient) fused(d_g, nullptr, 0.0, 0, -1, (T)-1, firstS);
        else if (firstS) { if (int rc = launch_dots({{firstS, d_dir}})) return rc; }
        for (int is = 0; is < lbfgsMem; is++) {
            const int c = col1(is);
            const bool first = startRides && is == 0;
            if (first) { scalIn = preDotScal; srcScale = (T)-1; }
            const double rho = first ? -h_rho[c] : h_rho[c];
            if (is + 1 < lbfgsMem) fused(first ? (const T *)d_g : nullptr, h_colY[c], rho, c, 0, (T)0, h_colS[col1(is + 1)]);
            else fused(first ? (const T *)d_g : nullptr, h_colY[c], rho, c, 0, (T)lbfgsH, h_colY[col2(lbfgsMem)], 1);      // the last step: the scaling by H0 between the loops rides along
        }
        if (lbfgsMem == 0) fused(d_dir, nullptr, 0.0, 0, -1, (T)lbfgsH, nullptr);
        for (int is = lbfgsMem; is > 0; is--) {
            const int c = col2(is);
            fused(nullptr, h_colS[c], h_rho[c], c, 1, (T)0, is > 1 ? h_colY[col2(is - 1)] : nullptr);
        }
        RN_HIP(hipGetLastError());
        return arc;
    }
    // SmpcController::computeValueFbe (:1416-1476)
    int value_fbe(double *value) override { return value_fbe_impl(value, false); }
    // dotsReady: <w, res> and <res, res> are already in d_scal[0..1] (prox_residual ran on the current w)
    int value_fbe_impl(double *value, bool dotsReady) {
        RN_CHECK(value, RN_E_ARG, "rn_compute_value_fbe: null output");
        RN_FBE_READY("rn_compute_value_fbe")
        if (int rc = value_launch(dotsReady)) return rc;
        if (int rc = reduce_scalars(d_scal + 8, 2)) return rc;
        double sc[10];
        IterState st;
        RN_HIP(hipMemcpyAsync(&st, d_state, sizeof st, hipMemcpyDeviceToHost, stream));
        if (int rc = read_scalars(sc, 0, 10)) return rc;
        *value = value_host(sc, st);
        return RN_OK;
    }
    // the device half: <w, res>, <res, res> -> d_scal[0..1] (unless they are there already), the two value terms -> d_scal[8..9]
    int value_launch(bool dotsReady) {
        if (!dotsReady) {
            DotArgs<T> g{};
            g.a[0] = p_acc_view; g.b[0] = d_res; g.a[1] = d_res; g.b[1] = d_res; g.cnt = 2; g.n = ntot(); g.partials = d_dotPartials; g.first = dot_first();
            hipLaunchKernelGGL(k_dots<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, g);
            hipLaunchKernelGGL(k_dots_finish<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_dotPartials, eltBlocks, 2, d_scal);
            if (int rc = reduce_scalars(d_scal, 2)) return rc;
        }
        if (valueMfma) {
            const int SBw = slab_stride(pad4(d.nu));
            hipLaunchKernelGGL(k_value_mfma<T>, dim3(vmBlocks()), dim3(64 * VM_WAVES), (size_t)16 * SBw * sizeof(T), stream, (const T *)d_u, (const T *)d_udir, (const T *)d_prevU,
                               (const int *)d_parent, (const T *)d_prob, (const T *)d_Wp, pad16(d.nu), pad4(d.nu), (const T *)d_alpha, d.nu, d.nodes, LsTaus<T>{}, 1, d_valPartials,
                               DOT_MAX, 0, value_first_node(), SBw);
        } else {
            hipLaunchKernelGGL(k_value_terms<T>, dim3(valueBlocks), dim3(VALUE_THREADS), (size_t)VALUE_TILE * d.nu * sizeof(T), stream, d_u, d_prevU, d_parent,
                               d_prob, d_W, d_alpha, d.nu, d.nodes, d_valPartials, value_first_node());
        }
        hipLaunchKernelGGL(k_dots_finish<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_valPartials, valueMfma ? vmBlocks() : valueBlocks, 2, d_scal + 8);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // the host half: computeValueFbe's sum (:1416-1476) on sc[0..1], sc[8..9] and the prox distances
    double value_host(const double *sc, const IterState &st) const {
        const double thrX = penX / stepSize, thrS = penXs / stepSize;
        // value of g at the prox point: zero inside the sets, gamma * dist(prox point, C) once the soft branch trips
        const T gX = st.distX > thrX ? (T)(penX * (st.distX - thrX)) : (T)0;
        const T gS = st.distS > thrS ? (T)(penXs * (st.distS - thrS)) : (T)0;
        T cost = (T)sc[0];
        cost = cost + (T)0.5 * (T)stepSize * (T)sc[1];
        cost = cost + gX + gS;
        cost = cost + (T)sc[8];
        cost = cost + (T)sc[9];
        return (double)cost;
    }
    // the loops' "value, then L-BFGS buffer" (computeValueFbe + updateLbfgsBuffer) with ONE blocking read-back instead of two: both
    // device halves are enqueued (they do not depend on each other: the buffer's dot products go to d_scal[4..8)), then the ten
    // scalars come back together and the two host halves run in the reference's order
    int value_and_buffer(double *value) {
        if (int rc = value_launch(true)) return rc;
        buffer_launch(d_scal + 10, true);
        RN_HIP(hipGetLastError());
        if (int rc = reduce_scalars(d_scal + 8, 8)) return rc;      // sharded: [8..10) value terms, [10..16) buffer dots ([0..2) were reduced by prox_residual)
        double sc[16];
        IterState st;
        RN_HIP(hipMemcpyAsync(&st, d_state, sizeof st, hipMemcpyDeviceToHost, stream));
        if (int rc = read_scalars(sc, 0, 16)) return rc;
        *value = value_host(sc, st);
        if (int rc = buffer_host(sc + 10, false)) return rc;
        // the recursion's first dot product <newest S column, -gradient> is there already: dot 4 if the new pair became the newest column,
        // dot 5 (the newest column so far) if the pair was skipped -- its partials for the one-GPU fold, its reduced value for shards
        const int j = lastPairAccepted ? 4 : 5;
        preDotPartials = d_dotPartials + j; preDotScal = d_scal + 10 + j; preDotValid = lbfgsMem > 0;
        return RN_OK;
    }
    int trial_step(T tau) {
        TrialArgs<T> g{d_x, d_u, p_acc_view, d_hx, d_xdir, d_udir, d_dir, d_hxDir, (long long)d.nodes * d.nx, (long long)d.nodes * d.nu, ntot(), tau};
        hipLaunchKernelGGL(k_trial_step<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, g);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // common tail of both line searches (:1272-1300, :1381-1409): all candidates of a batch evaluated at once (fbe_kernels.hpp, k_ls_*)
    // vdSign != 0: the search direction's slope <Yvec, dir> (d_scal[0], enqueued by the caller; vdSign = -1: its negative) has not
    // been read yet -- it comes back with the first batch's values, and the reference's rule on it (:1262-1270, :1370-1379: positive:
    // nothing applied, tau stays; |.| < 1e-4: tau = 0) is applied before anything is: one blocking read-back less per iteration.
    // The first batch is then evaluated for nothing in the iterations that take neither branch of the search (rare).
    int line_search_loop(double valueY, T *tauOut, int vdSign = 0) {
        if (!lsFused) {
            if (vdSign != 0) {
                double vd;
                if (int rc = read_scalars(&vd, 0, 1)) return rc;
                const T valueDirection = vdSign > 0 ? (T)vd : -(T)vd;
                if (valueDirection > 0) return RN_OK;
                if (std::fabs((double)valueDirection) < 1e-4) { *tauOut = 0; return RN_OK; }
            }
            lsSearches++; lsSequential++;
            return line_search_loop_sequential(valueY, tauOut, 0, (T)1);
        }
        const int maxStep = 10;
        // the increment of every trial if all before it are accepted (the reference's update of tau, :1284-1297)
        T taus[maxStep + 1];
        {
            T tau = 1;
            for (int i = 0; i <= maxStep; i++) {
                taus[i] = tau;
                const int iStep = i + 1;
                if (iStep < maxStep) { if (iStep == 1) tau = -1; tau = tau + (T)(1 / std::pow(2.0, iStep)); }
            }
        }
        const double thrX = penX / stepSize, thrS = penXs / stepSize;
        int done = 0;                      // trials applied to the device state so far (all of them accepted)
        bool stop = false;
        while (!stop && done < maxStep + 1) {
            // first batch: four candidates (tau = 1 ... 1/8 decide most searches, and the value pass costs 21 us per candidate on the
            // 493-scenario tree); whoever needs more gets batches of LS_K
            const int nEval = std::min(done == 0 ? LS_FIRST : LS_K, maxStep + 1 - done);
            LsTaus<T> ts{};
            ts.n = nEval;
            for (int c = 0; c < nEval; c++) ts.tau[c] = taus[done + c];
            DualArgs<T> a = dual_args();
            a.w = p_acc_view;
            hipLaunchKernelGGL(k_ls_eval<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a, (const T *)d_dir, (const T *)d_hxDir, ts, d_lsEval);
            if (valueMfma) {
                const int SBw = slab_stride(pad4(d.nu));
                hipLaunchKernelGGL(k_value_mfma<T>, dim3(vmBlocks()), dim3(64 * VM_WAVES), (size_t)16 * SBw * sizeof(T), stream, (const T *)d_u, (const T *)d_udir, (const T *)d_prevU,
                                   (const int *)d_parent, (const T *)d_prob, (const T *)d_Wp, pad16(d.nu), pad4(d.nu), (const T *)d_alpha, d.nu, d.nodes, ts, 0, d_lsVal,
                                   LS_K * 2, 2, value_first_node(), SBw);
            } else {
                hipLaunchKernelGGL(k_ls_value<T>, dim3(lsValueBlocks), dim3(VALUE_THREADS), (size_t)LS_K * d.nu * LS_TILE * sizeof(T), stream, (const T *)d_u, (const T *)d_udir,
                                   (const T *)d_prevU, (const int *)d_parent, (const T *)d_prob, (const T *)d_W, (const T *)d_alpha, d.nu, d.nodes, ts, d_lsVal, value_first_node());
            }
            hipLaunchKernelGGL(k_ls_finish<>, dim3(nEval * LS_SCAL), dim3(ELT_THREADS), 0, stream, (const double *)d_lsEval, eltBlocks, (const double *)d_lsVal,
                               valueMfma ? vmBlocks() : lsValueBlocks, d_lsScal);
            RN_HIP(hipGetLastError());
            if (int rc = reduce_scalars(d_lsScal, nEval * LS_SCAL)) return rc;      // sharded: ONE all-reduce for the whole batch
            double sc[LS_K * LS_SCAL], vd = 0;
            RN_HIP(hipMemcpyAsync(sc, d_lsScal, (size_t)nEval * LS_SCAL * sizeof(double), hipMemcpyDeviceToHost, stream));
            if (vdSign != 0 && done == 0) RN_HIP(hipMemcpyAsync(&vd, d_scal, sizeof(double), hipMemcpyDeviceToHost, stream));
            RN_HIP(hipStreamSynchronize(stream));
            if (vdSign != 0 && done == 0) {
                const T valueDirection = vdSign > 0 ? (T)vd : -(T)vd;
                if (valueDirection > 0) return RN_OK;                                        // "LBFGS direction is positive": nothing applied
                if (std::fabs((double)valueDirection) < 1e-4) { *tauOut = 0; return RN_OK; }
            }
            if (done == 0) lsSearches++;
            lsBatches++;
            // the reference's accept / stop logic over the batch's values
            int use = 0;
            for (int c = 0; c < nEval; c++) {
                const double *v = sc + c * LS_SCAL;
                if (std::sqrt(v[2]) > thrX || std::sqrt(v[3]) > thrS) {
                    // this candidate's prox takes the soft-constraint branch: its value needs the tree-global distances first -- the trials
                    // from here on run one by one (the state stands after the `done + use` accepted trials)
                    if (use > 0) { if (int rc = apply_trials(ts, use)) return rc; }
                    lsSequential++;
                    return line_search_loop_sequential(valueY, tauOut, done + use, taus[done + use]);
                }
                T cost = (T)v[0];                                   // computeValueFbe (:1416-1476), as value_fbe_impl spells it
                cost = cost + (T)0.5 * (T)stepSize * (T)v[1];
                cost = cost + (T)0 + (T)0;
                cost = cost + (T)v[4];
                cost = cost + (T)v[5];
                use = c + 1;
                if (!((T)(double)cost <= (T)valueY)) { stop = true; break; }   // the value exceeds the reference value: this trial is the last
            }
            if (int rc = apply_trials(ts, use)) return rc;
            done += use;
        }
        if (int rc = prox_residual(nullptr)) return rc;      // z, res, distances of the final state (what the last sequential trial leaves)
        *tauOut = taus[done - 1];
        return RN_OK;
    }
    int fbe_counters(long *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_fbe_counters: null output");
        out[0] = lsSearches; out[1] = lsBatches; out[2] = lsSequential; out[3] = sweepPairs;
        return RN_OK;
    }
    // x, u, w, Hx after the first `n` trials of a batch, in one pass
    int apply_trials(LsTaus<T> ts, int n) {
        ts.n = n;
        TrialArgs<T> g{d_x, d_u, p_acc_view, d_hx, d_xdir, d_udir, d_dir, d_hxDir, (long long)d.nodes * d.nx, (long long)d.nodes * d.nu, ntot(), (T)0};
        hipLaunchKernelGGL(k_trial_multi<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, g, ts);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // the trials one by one, from trial `iStep` on with increment `tau` (the reference's loop as written)
    int line_search_loop_sequential(double valueY, T *tauOut, int iStep, T tau) {
        const int maxStep = 10;
        while (iStep < maxStep + 1) {
            if (int rc = trial_step(tau)) return rc;
            if (int rc = prox_residual(nullptr)) return rc;
            double val;
            if (int rc = value_fbe_impl(&val, true)) return rc;
            if ((T)val <= (T)valueY) {
                iStep = iStep + 1;
                if (iStep < maxStep) {
                    if (iStep == 1) tau = -1;
                    tau = tau + (T)(1 / std::pow(2.0, iStep));
                }
            } else iStep = maxStep + 1;
        }
        *tauOut = tau;
        return RN_OK;
    }
    // SmpcController::computeLineSearchLbfgsUpdate (:1242-1305)
    int line_search_fbe(double valueY, double *tauOut) override {
        RN_CHECK(tauOut, RN_E_ARG, "rn_line_search_lbfgs_update: null output");
        RN_FBE_READY("rn_line_search_lbfgs_update")
        T tau = 1;
        if (int rc = hessian_sweep(d_dir)) return rc;          // the swap / oracle / swap of :1251-1255
        if (int rc = launch_dots({{d_g, d_dir}})) return rc;
        // valueDirection = <g, dir>: positive -> "LBFGS direction is positive", nothing applied, tau stays 1 (:1262-1263); tiny -> tau = 0;
        // otherwise the search (the rule is applied inside, on the value that comes back with the first batch)
        if (int rc = line_search_loop(valueY, &tau, +1)) return rc;
        *tauOut = std::fabs((double)tau);
        return RN_OK;
    }
    // SmpcController::computeLineSearchAmeLbfgsUpdate (:1311-1414)
    // the two element-wise launches of the AME line search's opening (SmpcController.cu:1332-1340), in the order its sweeps allow (line_search_ame):
    // w += lambda res, x += lambda xdir, u += lambda udir, Hx += lambda HxDir with the directions of the sweep on the residual ...
    void launch_ame_trial_step(const T *xdir, const T *udir, const T *hxDir) {
        TrialArgs<T> g{d_x, d_u, p_acc_view, d_hx, xdir, udir, d_res, hxDir, (long long)d.nodes * d.nx, (long long)d.nodes * d.nu, ntot(), (T)stepSize};
        hipLaunchKernelGGL(k_trial_step<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, g);
    }
    // ... and the direction's correction dir -= lambda res
    void launch_ame_correction() { hipLaunchKernelGGL(k_axpby<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_dir, d_dir, d_res, (T)1, (T)-stepSize, ntot()); }
    int line_search_ame(double valueY, double *tauOut) override {
        RN_CHECK(tauOut, RN_E_ARG, "rn_line_search_ame_lbfgs_update: null output");
        RN_FBE_READY("rn_line_search_ame_lbfgs_update")
        T tau = 1;
        if (int rc = launch_dots({{d_res, d_dir}})) return rc;                                 // valueDirection = -<res, dir>, read with the search's first batch
        if (pair_active()) {
            // the reference's two Hessian oracles (:1331 on the residual, :1341-1345 on the corrected direction) do not feed each other:
            // the direction's correction (:1338-1340) only needs the residual.  So the correction comes first and both sweeps share one
            // pass over the operator blocks -- a third of the iteration's HBM traffic; same values as the sequence below.
            launch_ame_correction();                                                               // :1338-1340
            if (int rc = launch_sweep(nullptr, 0, d_res, true, d_dir)) return rc;                  // :1331 and :1341-1345
            launch_ame_trial_step(d_xdirB, d_udirB, d_hxDirB);                                     // :1332-1337
            sweepPairs++;
        } else {
            if (int rc = hessian_sweep(d_res)) return rc;                                          // :1331
            launch_ame_trial_step(d_xdir, d_udir, d_hxDir);                                        // :1332-1337
            launch_ame_correction();                                                               // :1338-1340
            if (int rc = hessian_sweep(d_dir)) return rc;                                          // :1341-1345
        }
        if (int rc = line_search_loop(valueY, &tau, -1)) return rc;
        RN_HIP(hipGetLastError());
        *tauOut = std::fabs((double)tau);
        return RN_OK;
    }
    int fbe_dual_update() {
        hipLaunchKernelGGL(k_fbe_dual_update<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_gPrev, d_g, d_prevY, p_xi, p_acc_view, d_res, (T)stepSize, ntot());
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // SmpcController::algorithmGlobalFbe (:1529-1555) / algorithmNama (:1559-1586)
    int algorithm_fbe_nama(int maxIt, double *primalInfs, double *valueFbe, double *tauHist) override {
        RN_CHECK(maxIt >= 0, RN_E_ARG, "rn_algorithm_global_fbe / rn_algorithm_nama: negative iteration count");
        RN_FBE_READY("rn_algorithm_global_fbe / rn_algorithm_nama")
        if (int rc = fbe_reset()) return rc;
        if (int rc = step_rule_on_entry()) return rc;
        if (maxIt > infHistCap) {          // 1 024 iterations are there from rn_set_algorithm on; a longer loop gets a larger array (the old one stays until rn_destroy)
            const int cap = std::max(1024, 2 * maxIt);
            if (int rc = dalloc(&d_infHist, (size_t)4 * cap)) return rc;
            infHistCap = cap;
        }
        for (int it = 0; it < maxIt; it++) {
            if (int rc = solve_step()) return rc;
            if (int rc = prox_residual(d_g)) return rc;            // prox, residual, g = -res (= nama_residual, first line of gradient_fbe)
            if (algorithm == RN_ALG_GLOBAL_FBE) { if (int rc = gradient_fbe_impl(true)) return rc; }
            if (it > 0) {
                double val, tau;
                if (int rc = value_and_buffer(&val)) return rc;        // computeValueFbe + updateLbfgsBuffer, one read-back
                if (int rc = lbfgs_two_loop_impl(true)) return rc;
                if (int rc = (algorithm == RN_ALG_GLOBAL_FBE ? line_search_fbe(val, &tau) : line_search_ame(val, &tau))) return rc;
                if (valueFbe) valueFbe[it - 1] = val;
                if (tauHist) tauHist[it - 1] = tau;
            }
            if (int rc = fbe_dual_update()) return rc;
            // updatePrimalInfeasibity (:1480-1496): folded on the device into d_infHist[4 it ...] = (v_xi, -v_xi, v_psi, -v_psi); all
            // iterations' entries come back in one read after the loop (sharded: after ONE max all-reduce over all of them)
            hipLaunchKernelGGL(k_absmax<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_res, ntot(), d.nx, ny, d_partials);
            hipLaunchKernelGGL(k_inf_fold<>, dim3(1), dim3(ELT_THREADS), 0, stream, (const Partial *)d_partials, eltBlocks, d_infHist + 4 * (size_t)it);
            RN_HIP(hipGetLastError());
        }
        if (maxIt > 0) {
            if (fbe_sharded()) { if (int rc = all_reduce(d_infHist, (size_t)4 * maxIt, true, "ncclAllReduce(primal infeasibilities)", 2 /* ncclMax */)) return rc; }
            std::vector<double> h((size_t)4 * maxIt);
            RN_HIP(hipMemcpyAsync(h.data(), d_infHist, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
            RN_HIP(hipStreamSynchronize(stream));
            if (primalInfs)
                for (int it = 0; it < maxIt; it++) {
                    const double *q = h.data() + 4 * (size_t)it;
                    const double vX = q[0] >= q[1] ? q[0] : -q[1], vP = q[2] >= q[3] ? q[2] : -q[3];   // largest magnitude and its sign (as rn_update_primal_infeasibility)
                    primalInfs[it] = vX > vP ? vX : vP;
                }
        }
        return RN_OK;
    }
    int lbfgs_state(int set, int *col, int *mem, double *H, double *rho) override {
        RN_CHECK(lbfgsSize > 0, RN_E_STATE, "rn_lbfgs_state: select RN_ALG_GLOBAL_FBE or RN_ALG_NAMA first");
        RN_CHECK(col && mem && H, RN_E_ARG, "rn_lbfgs_state: null pointer");
        if (set) {
            RN_CHECK(*col >= 0 && *col <= lbfgsSize && *mem >= 0 && *mem <= lbfgsSize, RN_E_ARG, "rn_lbfgs_state: column / memory out of range");
            lbfgsCol = *col; lbfgsMem = *mem; lbfgsH = *H;
            if (rho) for (int i = 0; i <= lbfgsSize; i++) h_rho[i] = rho[i];
        } else {
            *col = lbfgsCol; *mem = lbfgsMem; *H = lbfgsH;
            if (rho) for (int i = 0; i <= lbfgsSize; i++) rho[i] = h_rho[i];
        }
        return RN_OK;
    }
    // one column of matS (which = 0) or matY (which = 1), in the reference's (all xi | all psi) order
    int lbfgs_column(int set, int which, int col, double *host, size_t cnt) override {
        RN_CHECK(lbfgsSize > 0, RN_E_STATE, "rn_lbfgs_column: select RN_ALG_GLOBAL_FBE or RN_ALG_NAMA first");
        RN_CHECK(host && (which == 0 || which == 1) && col >= 0 && col <= lbfgsSize && cnt == (size_t)ntot(), RN_E_ARG, "rn_lbfgs_column: bad argument");
        RN_HIP(hipSetDevice(device));
        T *base = (which == 0 ? h_colS : h_colY)[col];
        const size_t nxi = (size_t)d.nodes * 2 * d.nx, nps = (size_t)d.nodes * d.nu;
        for (int part = 0; part < 2; part++) {
            const int off = part == 0 ? 0 : 2 * d.nx, dim = part == 0 ? 2 * d.nx : d.nu;
            double *h = host + (part == 0 ? 0 : nxi);
            const size_t m = part == 0 ? nxi : nps;
            if (set) {
                if (int rc = upload(d_tmp, h, m)) return rc;
                hipLaunchKernelGGL(k_pack<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, base, d_tmp, ny, off, dim, (long long)d.nodes, 1);
                RN_HIP(hipStreamSynchronize(stream));
            } else {
                hipLaunchKernelGGL(k_pack<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, base, d_tmp, ny, off, dim, (long long)d.nodes, 0);
                if (int rc = download(h, d_tmp, m)) return rc;
            }
        }
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
