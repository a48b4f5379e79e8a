// lipschitz.inc -- members of rn::Ctx<T> that estimate the dual Lipschitz constant L = lambda_max(K H^-1 K') of the operators the context
// holds by power sweeps on the device, and the step-size rule that uses it (included inside the struct body of rapidnet_capi.hip).  Entry
// points served (include/rapidnet.h):
//   rn_estimate_lipschitz, rn_get_lipschitz     the estimate and the record it left
//   rn_set_step_rule, rn_get_step_rule          stepSize = margin / NORM on entry of the solves (opt-in)
// The reference has no counterpart: its stepSize is a figure computed offline and written into the configuration file.  The linear map
// is the Hessian sweep (launch_sweep with a Hessian input, SmpcController::computeHessianOracalGlobalFbe); what is here is the loop
// around it -- k_dots for s = <w, w> and t = <v, w>, k_power_step (fbe_kernels.hpp) for v = w / sqrt(s) and the record -- with buffers of
// its own, so that a call between any two entry points leaves every iterate, the L-BFGS memory and the batch state alone.
// Summation order: k_dots' element order and k_dots_finish's fold order, fp64 accumulation on fp32 contexts too, no atomics: two calls
// return the same bits.  Sharded contexts count the replicated crown on rank 0 only (dot_first) and sum s and t over the ranks
// (reduce_scalars) before k_power_step reads them: every rank holds the same bits.

    static_assert(RN_LIP_COLS == 4 && RN_LIP_ITERATIONS == 3, "k_power_step writes NORM, RAYLEIGH, RESIDUAL; the host appends ITERATIONS");
    // v, w in the y layout; the sweep's x, u and v outputs; dot partials, the reduced pair (sharded), the history [cap][3].  Allocated by the
    // first estimate and kept: a context that never asks holds none of them and launches nothing
    T *d_lipV = nullptr, *d_lipW = nullptr, *d_lipX = nullptr, *d_lipU = nullptr, *d_lipPv = nullptr;
    double *d_lipPartials = nullptr, *d_lipScal = nullptr, *d_lipHist = nullptr;
    int lipHistCap = 0;
    bool lipHeld = false, lipStale = false;
    double lipRec[RN_LIP_COLS] = {0, 0, 0, 0};
    // M = K H^-1 K' has changed (the factor step, caller-owned blocks, their storage type, the probabilities): the held estimate is another
    // operator's.  Bounds, tree errors, forecasts and the state do not enter M
    void lip_invalidate() { if (lipHeld) lipStale = true; }
    int lip_buffers(int maxIt) {
        const size_t n = (size_t)ntot(), N_ = d.nodes;
        if (!d_zero) {      // a context that never selected FBE / NAMA: the zero block the Hessian sweep reads its affine terms from
            const size_t nz = N_ * (size_t)std::max(d.nu, std::max(d.nx, d.nv));
            T *z = nullptr;
            if (int rc = dalloc(&z, nz)) return rc;
            RN_HIP(hipMemsetAsync(z, 0, nz * sizeof(T), stream));
            d_zero = z;
        }
        if (maxIt > lipHistCap) {      // (a longer loop gets a larger table; the old one stays until rn_destroy)
            const int cap = std::max(64, maxIt);
            if (int rc = dalloc(&d_lipHist, (size_t)3 * cap)) return rc;
            lipHistCap = cap;
        }
        if (d_lipV) return RN_OK;
        if (int rc = dalloc(&d_lipW, n)) return rc;
        if (int rc = dalloc(&d_lipX, N_ * d.nx)) return rc;
        if (int rc = dalloc(&d_lipU, N_ * d.nu)) return rc;
        if (int rc = dalloc(&d_lipPv, N_ * d.nv)) return rc;
        if (int rc = dalloc(&d_lipPartials, (size_t)ELT_MAX_BLOCKS * DOT_MAX)) return rc;
        if (int rc = dalloc(&d_lipScal, 2)) return rc;
        return dalloc(&d_lipV, n);      // last: the sign that the set exists
    }
    // The library's own start: element c of GLOBAL node g is a hash of i = g * ny + c and the seed (splitmix64's finaliser), mapped to [-1, 1) and
    // rounded to the context's type -- a shard starts from the one-GPU context's vector, and numpy restates it bit for bit (rapidnet.h)
    static double lip_hash(unsigned long long seed, unsigned long long i) {
        unsigned long long x = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 27; x *= 0x94D049BB133111EBull;
        x ^= x >> 31;
        return (double)(x >> 11) * (1.0 / 4503599627370496.0) - 1.0;      // 2^-52
    }
    int lip_start(const double *startXi, const double *startPsi, unsigned long long seed) {
        if (startXi) {      // the caller's arrays, in the layout of rn_set(RN_BUF_XI / RN_BUF_PSI), through its staging buffer
            if (int rc = upload(d_tmp, startXi, (size_t)d.nodes * 2 * d.nx)) return rc;
            y_pack(d_lipW, d_tmp, 0, 2 * d.nx, (long long)d.nodes, true);
            RN_HIP(hipStreamSynchronize(stream));
            if (int rc = upload(d_tmp, startPsi, (size_t)d.nodes * d.nu)) return rc;
            y_pack(d_lipW, d_tmp, 2 * d.nx, d.nu, (long long)d.nodes, true);
            RN_HIP(hipGetLastError());
            return RN_OK;
        }
        std::vector<double> h((size_t)ntot());
        for (int node = 0; node < d.nodes; node++) {
            const unsigned long long g = globalNode.empty() ? (unsigned long long)node : (unsigned long long)globalNode[node];
            for (int c = 0; c < ny; c++) h[(size_t)node * ny + c] = lip_hash(seed, g * (unsigned long long)ny + (unsigned long long)c);
        }
        return upload(d_lipW, h.data(), h.size());
    }
    // s = <w, w> and (withT) t = <v, w> into d_lipPartials; sharded: folded and summed over the ranks into d_lipScal
    int lip_dots(bool withT) {
        DotArgs<T> g{};
        g.a[0] = d_lipW; g.b[0] = d_lipW; g.a[1] = d_lipV; g.b[1] = d_lipW;
        g.cnt = withT ? 2 : 1; g.n = ntot(); g.partials = d_lipPartials; g.first = dot_first();
        hipLaunchKernelGGL(k_dots<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, g);
        if (fbe_sharded()) {
            hipLaunchKernelGGL(k_dots_finish<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_lipPartials, eltBlocks, g.cnt, d_lipScal);
            RN_HIP(hipGetLastError());
            return reduce_scalars(d_lipScal, g.cnt);
        }
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // v = w / sqrt(s) (normalise) and record `row` (>= 0) from the dots lip_dots left
    int lip_step(bool withT, bool normalise, int row) {
        PowerArgs g{};
        g.v = d_lipV; g.w = d_lipW; g.partials = d_lipPartials; g.nblocks = eltBlocks; g.cnt = withT ? 2 : 1;
        g.scal = fbe_sharded() ? d_lipScal : nullptr;
        g.hist = d_lipHist; g.row = row; g.n = ntot(); g.normalise = normalise ? 1 : 0; g.f64 = sizeof(T) == 8 ? 1 : 0;
        hipLaunchKernelGGL(k_power_step<>, dim3(normalise ? eltBlocks : 1), dim3(ELT_THREADS), 0, stream, g);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    int estimate_lipschitz(int maxIt, double tol, int checkEvery, const double *startXi, const double *startPsi, unsigned long long seed, double *out,
                           double *history) override {
        const std::string fn = "rn_estimate_lipschitz";
        RN_CHECK(out, RN_E_ARG, fn + ": null output");
        RN_CHECK(maxIt >= 1, RN_E_ARG, fn + ": maxIterations must be at least 1");
        RN_CHECK(tol >= 0 && std::isfinite(tol), RN_E_ARG, fn + ": the tolerance must be finite and >= 0");      // (a NaN fails the comparison)
        RN_CHECK((startXi == nullptr) == (startPsi == nullptr), RN_E_ARG, fn + ": give both start arrays or neither");
        RN_CHECK(factored, RN_E_STATE, fn + " before rn_factor_step");
        RN_CHECK(!poisoned, RN_E_STATE, fn + ": an earlier batch failed half-way; call rn_apg_reset first");
        RN_CHECK(cutStage <= 0 || nranks == 1 || has_comm(), RN_E_STATE, fn + ": a shard of several ranks needs a communicator (rn_comm_init with an id, "
                 "or an installed all-reduce): the norms are tree-global");
        RN_HIP(hipSetDevice(device));
        if (int rc = lip_buffers(maxIt)) return rc;
        if (int rc = lip_start(startXi, startPsi, seed)) return rc;
        const int every = checkEvery > 0 ? checkEvery : RN_LIP_CHECK_EVERY;
        const HessOut ho{d_lipX, d_lipU, d_lipW, d_lipPv};
        double rec[3] = {0, 0, 0};
        int done = 0;
        bool dotsCurrent = false;      // d_lipPartials (d_lipScal) hold the dots of the current w: an early-stop check has just formed them
        for (int k = 1; k <= maxIt; k++) {
            if (!dotsCurrent) { if (int rc = lip_dots(k >= 2)) return rc; }
            dotsCurrent = false;
            if (int rc = lip_step(k >= 2, true, k >= 2 ? k - 2 : -1)) return rc;
            if (int rc = launch_sweep(nullptr, 0, d_lipV, true, nullptr, &ho)) return rc;
            done = k;
            if (tol > 0 && k % every == 0 && k < maxIt) {      // the record of this iteration, behind one synchronisation
                if (int rc = lip_dots(true)) return rc;
                if (int rc = lip_step(true, false, k - 1)) return rc;
                dotsCurrent = true;
                RN_HIP(hipMemcpyAsync(rec, d_lipHist + (size_t)3 * (k - 1), sizeof rec, hipMemcpyDeviceToHost, stream));
                RN_HIP(hipStreamSynchronize(stream));
                if (!(rec[0] > 0) || !std::isfinite(rec[0]) || rec[2] <= tol) break;
            }
        }
        if (!dotsCurrent) {      // the closing record: s and t of the last w
            if (int rc = lip_dots(true)) return rc;
            if (int rc = lip_step(true, false, done - 1)) return rc;
        }
        std::vector<double> hist((size_t)3 * done);
        RN_HIP(hipMemcpyAsync(hist.data(), d_lipHist, hist.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        RN_CHECK(hist[0] > 0 && std::isfinite(hist[0]), RN_E_ARG, fn + ": the start vector's norm is 0 or not finite");
        if (history) std::copy(hist.begin(), hist.end(), history);
        for (int c = 0; c < 3; c++) out[c] = lipRec[c] = hist[(size_t)3 * (done - 1) + c];
        out[RN_LIP_ITERATIONS] = lipRec[RN_LIP_ITERATIONS] = (double)done;
        lipHeld = true; lipStale = false;
        return RN_OK;
    }
    int get_lipschitz(double *out, int *stale) override {
        RN_CHECK(out, RN_E_ARG, "rn_get_lipschitz: null output");
        RN_CHECK(lipHeld, RN_E_STATE, "rn_get_lipschitz: no estimate was computed yet (rn_estimate_lipschitz)");
        for (int c = 0; c < RN_LIP_COLS; c++) out[c] = lipRec[c];
        if (stale) *stale = lipStale ? 1 : 0;
        return RN_OK;
    }

    // ---- the step-size rule ------------------------------------------------------------------------------
    // RN_STEP_FIXED (default): stepSize is rn_set_parameters', nothing is launched.  RN_STEP_LIPSCHITZ: the solves (rn_control_action,
    // rn_algorithm_apg, rn_apg_solve, rn_algorithm_global_fbe / _nama) estimate on entry when no estimate is held or the held one is stale --
    // stepIters iterations, the library's start, seed 0 -- and run with stepSize = margin / NORM.  stepFixed keeps rn_set_parameters' figure.
    int stepRule = RN_STEP_FIXED, stepIters = RN_LIP_RULE_ITERATIONS;
    double stepMargin = 0.9, stepFixed = 1e-4;
    void apply_step_size(double step) { stepSize = step; }      // (the one place a step size enters the context: rn_set_parameters and the rule)
    int set_step_rule(int rule, double margin, int iterations) override {
        RN_CHECK(rule == RN_STEP_FIXED || rule == RN_STEP_LIPSCHITZ, RN_E_ARG, "rn_set_step_rule: RN_STEP_FIXED or RN_STEP_LIPSCHITZ");
        if (rule == RN_STEP_FIXED) { stepRule = rule; apply_step_size(stepFixed); return RN_OK; }
        RN_CHECK(margin > 0 && margin <= 1, RN_E_ARG, "rn_set_step_rule: the margin must lie in (0, 1]");
        stepRule = rule; stepMargin = margin; stepIters = iterations > 0 ? iterations : RN_LIP_RULE_ITERATIONS;
        if (lipHeld && !lipStale) apply_step_size(stepMargin / lipRec[RN_LIP_NORM]);
        return RN_OK;
    }
    int get_step_rule(int *rule, double *margin, int *iterations, double *inForce) override {
        if (rule) *rule = stepRule;
        if (margin) *margin = stepMargin;
        if (iterations) *iterations = stepIters;
        if (inForce) *inForce = stepSize;
        return RN_OK;
    }
    int step_rule_on_entry() {
        if (stepRule != RN_STEP_LIPSCHITZ) return RN_OK;
        if (!lipHeld || lipStale) {
            double rec[RN_LIP_COLS];
            if (int rc = estimate_lipschitz(stepIters, 0.0, 0, nullptr, nullptr, 0ull, rec, nullptr)) return rc;
        }
        apply_step_size(stepMargin / lipRec[RN_LIP_NORM]);
        return RN_OK;
    }
