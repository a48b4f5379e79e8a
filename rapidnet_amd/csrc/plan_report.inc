// plan_report.inc -- members of rn::Ctx<T> that report what the plan a context holds costs and where it violates its bounds (included
// inside the struct body of rapidnet_capi.hip).  Entry points served (include/rapidnet.h):
//   rn_plan_report             the per-stage table, host
//   rn_plan_report_scenarios   the per-leaf table and the node of every row, host
//   rn_plan_report_device      both tables where the kernel left them
// They generalise the reference's closed-loop KPIs -- SmpcController::updateKpi and the read-outs getEconomicKpi, getSmoothKpi, getSafeKpi,
// getNetworkKpi (SmpcController.cu:1819-1859), sums over one realised trajectory -- to the scenario tree of the plan at hand.  What the
// forms share stands once: the state check, the buffers (plan_buffers) and the two launches with their collectives (plan_run; k_plan_report,
// k_plan.hpp).

    static_assert(PLAN_COLS == RN_PLAN_COLS && PLAN_SUMS == RN_PLAN_SHORT_MAX, "k_plan.hpp and rapidnet.h name the same columns");
    // x and u hold a plan once a sweep of the solve path has stored its primal iterates (launch_sweep sets this)
    bool primalSwept = false;
    // [nodes][PLAN_COLS]; [PLAN_COLS][N], sum columns first; [leaves][PLAN_COLS]; [leaves].  Allocated by the first report and kept: a context
    // that never asks holds none of them and launches nothing
    double *d_planNode = nullptr, *d_planStage = nullptr, *d_planLeaf = nullptr;
    int *d_planLeafNode = nullptr;
    int plan_leaves() const { return h_stageCum[d.N] - h_stageCum[d.N - 1]; }
    int plan_buffers() {
        if (d_planNode) return RN_OK;
        if (int rc = dalloc(&d_planStage, (size_t)d.N * PLAN_COLS)) return rc;
        if (int rc = dalloc(&d_planLeaf, (size_t)plan_leaves() * PLAN_COLS)) return rc;
        if (int rc = dalloc(&d_planLeafNode, (size_t)plan_leaves())) return rc;
        return dalloc(&d_planNode, (size_t)d.nodes * PLAN_COLS);      // last: the sign that all four exist
    }
    // The two launches on the context's stream, no host synchronisation in between, and -- sharded contexts -- the collectives that make the
    // per-stage table the whole tree's on every rank: the sum block summed, then passed through a MAX all-reduce so that every rank holds the
    // same bits whatever order a collective added them in (launch_restart_test's agreement pass); the maxima block through a MAX all-reduce.
    // x and u need nothing to be current (rn_get reads them as they stand: only v is computed on demand, v_flush).
    int plan_run(const std::string &fn) {
        RN_CHECK(factored, RN_E_STATE, fn + " before rn_factor_step");
        RN_CHECK(affine_ready, RN_E_STATE, fn + " before the affine terms (rn_eliminate_input_disturbance_coupling)");
        RN_CHECK(primalSwept, RN_E_STATE, fn + " before the first sweep: x and u hold no plan yet");
        RN_CHECK(plan_lds_bytes(d.nu) <= (size_t)64 * 1024, RN_E_ARG, fn + ": nu is too large for the tile of input differences in LDS");
        RN_HIP(hipSetDevice(device));
        if (int rc = plan_buffers()) return rc;
        PlanArgs a{};
        a.f64 = sizeof(T) == 8 ? 1 : 0;
        a.nodes = d.nodes; a.nx = d.nx; a.nu = d.nu; a.ny = ny; a.N = d.N; a.leaves = plan_leaves();
        a.x = d_x; a.u = d_u; a.alpha = d_alpha; a.prevU = d_prevU; a.prob = d_prob; a.W = d_W; a.blo = d_blo; a.bhi = d_bhi;
        a.bStrideStage = b_stride_stage(); a.bStrideNode = b_stride_node();
        a.parent = d_parent; a.stageOf = d_stageOf; a.stageCum = d_stageCum;
        a.crownStages = 0; a.countCrown = 1;
        if (cutStage > 0) { a.crownStages = cutStage; a.countCrown = (rank == 0); }
        a.node = d_planNode; a.stage = d_planStage; a.leaf = d_planLeaf; a.leafNode = d_planLeafNode;
        const size_t lds = plan_lds_bytes(d.nu);
        const int tiles = (d.nodes + PLAN_TILE - 1) / PLAN_TILE;
        a.phase = 0;
        hipLaunchKernelGGL(k_plan_report<>, dim3(std::max(1, std::min(tiles, numCUs * 4))), dim3(PLAN_THREADS), lds, stream, a);
        a.phase = 1;
        hipLaunchKernelGGL(k_plan_report<>, dim3(d.N + (a.leaves + PLAN_THREADS - 1) / PLAN_THREADS), dim3(PLAN_THREADS), lds, stream, a);
        RN_HIP(hipGetLastError());
        if (has_comm() && cutStage > 0) {
            const size_t sums = (size_t)PLAN_SUMS * d.N, maxima = (size_t)(PLAN_COLS - PLAN_SUMS) * d.N;
            if (int rc = all_reduce(d_planStage, sums, true, "ncclAllReduce(plan report, sums)")) return rc;
            if (int rc = all_reduce(d_planStage, sums, true, "ncclAllReduce(plan report, agreement)", 2 /* ncclMax */)) return rc;
            if (int rc = all_reduce(d_planStage + sums, maxima, true, "ncclAllReduce(plan report, maxima)", 2 /* ncclMax */)) return rc;
        }
        return RN_OK;
    }
    int plan_report(size_t stages, double *perStage) override {
        const std::string fn = "rn_plan_report";
        RN_CHECK(perStage, RN_E_ARG, fn + ": null output");
        RN_CHECK(stages == (size_t)d.N, RN_E_ARG, fn + ": stages must be dims.N");
        if (int rc = plan_run(fn)) return rc;
        std::vector<double> cm((size_t)d.N * PLAN_COLS);      // column-major on the device (k_plan.hpp)
        RN_HIP(hipMemcpyAsync(cm.data(), d_planStage, cm.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        for (int k = 0; k < d.N; k++) for (int c = 0; c < PLAN_COLS; c++) perStage[(size_t)k * PLAN_COLS + c] = cm[(size_t)c * d.N + k];
        return RN_OK;
    }
    int plan_report_scenarios(size_t leaves, double *perLeaf, int *leafNode) override {
        const std::string fn = "rn_plan_report_scenarios";
        RN_CHECK(perLeaf, RN_E_ARG, fn + ": null output");
        RN_CHECK(leaves == (size_t)plan_leaves(), RN_E_ARG, fn + ": leaves must be the context's (local) number of nodes at the last stage");
        if (int rc = plan_run(fn)) return rc;
        RN_HIP(hipMemcpyAsync(perLeaf, d_planLeaf, leaves * PLAN_COLS * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (leafNode) RN_HIP(hipMemcpyAsync(leafNode, d_planLeafNode, leaves * sizeof(int), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        return RN_OK;
    }
    int plan_report_device(void **perStage, void **perLeaf, size_t *leaves) override {
        const std::string fn = "rn_plan_report_device";
        RN_CHECK(perStage && perLeaf && leaves, RN_E_ARG, fn + ": null output");
        *perStage = nullptr; *perLeaf = nullptr; *leaves = 0;
        if (int rc = plan_run(fn)) return rc;
        *perStage = d_planStage; *perLeaf = d_planLeaf; *leaves = (size_t)plan_leaves();
        return RN_OK;
    }
