// plan_bands.inc -- members of rn::Ctx<T> that report what the plan a context holds looks like across the tree (included inside the struct
// body of rapidnet_capi.hip).  Entry points served (include/rapidnet.h):
//   rn_plan_quantiles          weighted quantiles of every component of x or u per stage, host
//   rn_plan_quantiles_device   the same table where the kernel left it
//   rn_plan_paths              the rows of x or u along every leaf's path, host
// The reference has no counterpart: its read-outs end at one realised trajectory.  What the forms share stands once: the argument and state
// checks (bands_check), the buffers (bands_buffers), the source of the rows -- the context's own arrays, or on a shard the table every rank
// packs its rows into and the communicator sums (bands_source) -- and the launch of k_plan_bands (k_plan.hpp).

    static_assert(BANDS_WIDTH == bands::MAX_WIDTH && BANDS_LEVELS == bands::MAX_LEVELS && BANDS_LEVELS == RN_BAND_MAX_LEVELS, "k_plan.hpp, bands_host.hpp and rapidnet.h name the same caps");
    // [N][dim][nq]; [leaves][N][dim]; [leaves]; one word; shards: [full nodes][dim + 1], the full tree's parent and nodesPerStageCumul.  All sized
    // for the larger of nx and nu, allocated by the first call and kept: a context that never asks holds none of them and launches nothing
    double *d_bandQuant = nullptr, *d_bandPaths = nullptr, *d_bandTable = nullptr;
    int *d_bandLeafNode = nullptr, *d_bandFlag = nullptr, *d_bandParent = nullptr, *d_bandCum = nullptr;
    std::vector<int> fullCum, fullParent;      // rn_create_sharded: the FULL tree's nodesPerStageCumul [N + 1] and parents (-1 for the root)
    void set_full_tree(const int *cum, const int *ancestor, int N, int nodes) override {
        fullCum.assign(cum, cum + N + 1);
        fullParent.resize(nodes);
        for (int i = 0; i < nodes; i++) fullParent[i] = ancestor[i] - 1;
    }
    bool bands_sharded() const { return nranks > 1 && cutStage > 0; }
    const std::vector<int> &bands_cum() const { return bands_sharded() ? fullCum : h_stageCum; }
    int bands_nodes() const { return bands_sharded() ? fullNodes : d.nodes; }
    int bands_leaves() const { return bands_cum()[d.N] - bands_cum()[d.N - 1]; }
    int bands_buffers() {
        if (d_bandQuant) return RN_OK;
        const size_t dim = (size_t)std::max(d.nx, d.nu), leaves = (size_t)bands_leaves();
        if (int rc = dalloc(&d_bandPaths, leaves * d.N * dim)) return rc;
        if (int rc = dalloc(&d_bandLeafNode, leaves)) return rc;
        if (int rc = dalloc(&d_bandFlag, (size_t)1)) return rc;
        if (bands_sharded()) {
            if (int rc = dalloc(&d_bandTable, (size_t)fullNodes * (dim + 1))) return rc;
            if (int rc = dalloc(&d_bandParent, (size_t)fullNodes)) return rc;
            if (int rc = dalloc(&d_bandCum, (size_t)d.N + 1)) return rc;
            RN_HIP(hipMemcpyAsync(d_bandParent, fullParent.data(), fullParent.size() * sizeof(int), hipMemcpyHostToDevice, stream));
            RN_HIP(hipMemcpyAsync(d_bandCum, fullCum.data(), fullCum.size() * sizeof(int), hipMemcpyHostToDevice, stream));
            RN_HIP(hipStreamSynchronize(stream));
        }
        return dalloc(&d_bandQuant, (size_t)d.N * dim * BANDS_LEVELS);      // last: the sign that all of them exist
    }
    // x and u need nothing to be current (rn_get reads them as they stand), and the probabilities are those in force, whether or not the
    // affine terms have followed them yet
    int bands_check(const std::string &fn, int which) {
        RN_CHECK(which == RN_BAND_X || which == RN_BAND_U, RN_E_ARG, fn + ": which must be RN_BAND_X or RN_BAND_U");
        RN_CHECK(factored && primalSwept, RN_E_STATE, fn + " before the first sweep of a solve: x and u hold no plan yet");
        RN_CHECK(!poisoned, RN_E_STATE, fn + ": an earlier batch failed half-way; call rn_apg_reset first");
        if (bands_sharded())
            RN_CHECK(lib_sharded() && has_comm() && (int)fullCum.size() == d.N + 1 && (int)fullParent.size() == fullNodes, RN_E_STATE,
                     fn + ": a sharded context must come from rn_create_sharded and hold a communicator");
        RN_CHECK(bands::width_ok(bands_cum().data(), d.N), RN_E_STATE,
                 fn + ": a stage holds " + std::to_string(bands::widest_stage(bands_cum().data(), d.N)) + " nodes, the cap is " + std::to_string(bands::MAX_WIDTH) +
                     " (the sort's keys of one stage stay in LDS)");
        return RN_OK;
    }
    // Fills the part of the arguments that says where the rows are.  On a shard: the table zeroed, this rank's rows packed into it (rank 0 the
    // crown's as well), summed over the ranks -- exact, one rank at most holds a nonzero value at each entry -- so that every rank goes on
    // with the same bits of the whole tree.
    int bands_source(BandsArgs &a, int which) {
        a.f64 = sizeof(T) == 8 ? 1 : 0;
        a.dim = which == RN_BAND_X ? d.nx : d.nu;
        a.N = d.N; a.nodes = d.nodes; a.leaves = bands_leaves();
        a.src = which == RN_BAND_X ? d_x : d_u; a.prob = d_prob; a.rowStride = a.dim; a.probStride = 1;
        a.parent = d_parent; a.stageCum = d_stageCum;
        a.quant = d_bandQuant; a.paths = d_bandPaths; a.leafNode = d_bandLeafNode; a.flag = d_bandFlag;
        if (!bands_sharded()) return RN_OK;
        const size_t cnt = (size_t)fullNodes * (a.dim + 1);
        RN_HIP(hipMemsetAsync(d_bandTable, 0, cnt * sizeof(double), stream));
        a.phase = 2; a.gmap = d_gmap; a.crownNodes = h_stageCum[cutStage]; a.writeCrown = (rank == 0); a.table = d_bandTable;
        const long long work = (long long)d.nodes * (a.dim + 1);
        hipLaunchKernelGGL(k_plan_bands<>, dim3((unsigned)std::max<long long>(1, std::min<long long>(numCUs * 4, (work + BANDS_THREADS - 1) / BANDS_THREADS))),
                           dim3(BANDS_THREADS), 0, stream, a);
        RN_HIP(hipGetLastError());
        if (int rc = all_reduce(d_bandTable, cnt, true, "ncclAllReduce(plan bands, rows)")) return rc;
        a.f64 = 1; a.nodes = fullNodes;
        a.src = d_bandTable; a.prob = d_bandTable + a.dim; a.rowStride = a.probStride = a.dim + 1;
        a.parent = d_bandParent; a.stageCum = d_bandCum;
        return RN_OK;
    }
    // the quantile launch on the context's stream: nothing is waited for
    int bands_quantiles_run(const std::string &fn, int which, size_t nq, const double *q) {
        RN_CHECK(q, RN_E_ARG, fn + ": null levels");
        BandsArgs a{};
        const int lv = bands::sort_levels(nq, q, a.q, a.slot);
        RN_CHECK(lv != bands::LEVELS_COUNT, RN_E_ARG, fn + ": between 1 and " + std::to_string(bands::MAX_LEVELS) + " levels");
        RN_CHECK(lv == bands::LEVELS_OK, RN_E_ARG, fn + ": a level outside [0, 1]");
        if (int rc = bands_check(fn, which)) return rc;
        RN_HIP(hipSetDevice(device));
        if (int rc = bands_buffers()) return rc;
        a.nq = (int)nq;
        if (int rc = bands_source(a, which)) return rc;
        RN_HIP(hipMemsetAsync(d_bandFlag, 0, sizeof(int), stream));
        a.phase = 0;
        hipLaunchKernelGGL(k_plan_bands<>, dim3((unsigned)(d.N * a.dim)), dim3(BANDS_THREADS), 0, stream, a);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    int plan_quantiles(int which, size_t nq, const double *q, size_t stages, double *out) override {
        const std::string fn = "rn_plan_quantiles";
        RN_CHECK(out, RN_E_ARG, fn + ": null output");
        RN_CHECK(stages == (size_t)d.N, RN_E_ARG, fn + ": stages must be dims.N");
        if (int rc = bands_quantiles_run(fn, which, nq, q)) return rc;
        const size_t dim = which == RN_BAND_X ? d.nx : d.nu;
        int bad = 0;
        RN_HIP(hipMemcpyAsync(out, d_bandQuant, stages * dim * nq * sizeof(double), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipMemcpyAsync(&bad, d_bandFlag, sizeof(int), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        RN_CHECK(bad == 0, RN_E_STATE, fn + ": the plan holds " + std::to_string(bad) + " values that are not finite");
        return RN_OK;
    }
    int plan_quantiles_device(int which, size_t nq, const double *q, void **out) override {
        const std::string fn = "rn_plan_quantiles_device";
        RN_CHECK(out, RN_E_ARG, fn + ": null output");
        *out = nullptr;
        if (int rc = bands_quantiles_run(fn, which, nq, q)) return rc;
        *out = d_bandQuant;
        return RN_OK;
    }
    int plan_paths(int which, size_t leaves, double *out, int *leafNode) override {
        const std::string fn = "rn_plan_paths";
        RN_CHECK(out, RN_E_ARG, fn + ": null output");
        RN_CHECK(which == RN_BAND_X || which == RN_BAND_U, RN_E_ARG, fn + ": which must be RN_BAND_X or RN_BAND_U");
        RN_CHECK(!bands_sharded() || (int)fullCum.size() == d.N + 1, RN_E_STATE, fn + ": a sharded context must come from rn_create_sharded");
        RN_CHECK(leaves == (size_t)bands_leaves(), RN_E_ARG, fn + ": leaves must be the number of nodes of the whole tree's last stage");
        if (int rc = bands_check(fn, which)) return rc;
        RN_HIP(hipSetDevice(device));
        if (int rc = bands_buffers()) return rc;
        BandsArgs a{};
        if (int rc = bands_source(a, which)) return rc;
        a.phase = 1;
        hipLaunchKernelGGL(k_plan_bands<>, dim3((unsigned)leaves), dim3(BANDS_THREADS), 0, stream, a);
        RN_HIP(hipGetLastError());
        RN_HIP(hipMemcpyAsync(out, d_bandPaths, leaves * d.N * a.dim * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (leafNode) RN_HIP(hipMemcpyAsync(leafNode, d_bandLeafNode, leaves * sizeof(int), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        return RN_OK;
    }
