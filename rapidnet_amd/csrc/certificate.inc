// certificate.inc -- members of rn::Ctx<T> that take the solve certificate: the value of the dual function at the multiplier the context
// would warm-start from, the penalised primal value of the Lagrangian's minimiser there, and what qualifies both (included inside the struct
// body of rapidnet_capi.hip).  Entry points served (include/rapidnet.h):
//   rn_solve_certificate          the record, host (one synchronisation)
//   rn_solve_certificate_device   the record where the kernel left it (none)
// and the buffers RN_BUF_CERT_X / RN_BUF_CERT_U.  Extension: built on the reference's solveStep (SmpcController.cu:563-755), proximalFunG
// (:759-835) and computeValueFbe's primal terms (:1066-1146).  Three steps on the context's stream, no host synchronisation in between:
//   1  launch_sweep with y+ (p_upd) as its input and outputs of the certificate's own (CertOut): x(y), u(y), Hz(y), v(y).  Whatever form the
//      context runs -- dense, structured, fp32-stored blocks, the split last round, a shard's exchange -- is the sweep's own business.
//   2  k_plan_report's node phase on x(y), u(y): alpha' u, du' W du and the largest u-box violation of every node (COST's summation order).
//   3  k_certificate (k_plan.hpp): the flat pass over y, Hz(y) and the bounds rows, the fold of the node rows, the record.
// The sweep's scratch (the streaming product's results, the walks' running sums, a shard's cut payload) is overwritten as by any sweep; no
// RN_BUF_* buffer, iterate, history entry, batch flag or checkpoint is touched, so the next rn_apg_iterate continues bit for bit.  A v product
// left pending by the last primal sweep (v_flush) is run first: its input lives in that scratch.

    static_assert(CERT_REC == RN_CERT_COLS && RN_CERT_VALID == 13, "k_plan.hpp and rapidnet.h name the same columns");
    // x(y), u(y), Hz(y), v(y); the node table of step 2; the record, the sum block with the maxima, the partials and the arrival counter in
    // one allocation.  Allocated by the first certificate and kept: a context that never asks holds none of them and launches nothing
    T *d_certX = nullptr, *d_certU = nullptr, *d_certHz = nullptr, *d_certV = nullptr;
    double *d_certNode = nullptr, *d_cert = nullptr;
    bool certTaken = false;      // RN_BUF_CERT_X / _U hold a certificate's x(y), u(y)
    double *cert_rec() const { return d_cert; }
    double *cert_sums() const { return d_cert + CERT_REC; }
    double *cert_partials() const { return d_cert + 2 * CERT_REC; }
    unsigned int *cert_ticket() const { return reinterpret_cast<unsigned int *>(d_cert + 2 * CERT_REC + (size_t)ELT_MAX_BLOCKS * CERT_PART); }
    int cert_buffers() {
        const size_t N_ = d.nodes;      // (each buffer by itself: a call that follows one whose allocation failed part-way allocates only what is missing)
        if (!d_certX) { if (int rc = dalloc(&d_certX, N_ * d.nx)) return rc; }
        if (!d_certU) { if (int rc = dalloc(&d_certU, N_ * d.nu)) return rc; }
        if (!d_certV) { if (int rc = dalloc(&d_certV, N_ * d.nv)) return rc; }
        if (!d_certHz) { if (int rc = dalloc(&d_certHz, (size_t)ntot())) return rc; }
        if (!d_certNode) { if (int rc = dalloc(&d_certNode, N_ * PLAN_COLS)) return rc; }
        if (!d_cert) { if (int rc = dalloc(&d_cert, 2 * CERT_REC + (size_t)ELT_MAX_BLOCKS * CERT_PART + 1)) return rc; }
        return RN_OK;
    }
    int cert_run(const std::string &fn) {
        RN_CHECK(factored, RN_E_STATE, fn + " before rn_factor_step");
        RN_CHECK(affine_ready, RN_E_STATE, fn + " before the affine terms (rn_eliminate_input_disturbance_coupling)");
        RN_CHECK(algorithm == RN_ALG_APG, RN_E_STATE, fn + ": global FBE and NAMA keep their multiplier in another buffer; the certificate is APG's");
        RN_CHECK(p_upd != nullptr, RN_E_STATE, fn + " before rn_apg_reset: the context holds no multiplier yet");
        RN_CHECK(!poisoned, RN_E_STATE, fn + ": an earlier batch failed half-way; call rn_apg_reset first");
        RN_CHECK(cutStage <= 0 || nranks == 1 || has_comm(), RN_E_STATE, fn + ": a shard of several ranks needs a communicator (rn_comm_init with an id, "
                 "or an installed all-reduce): the sums are tree-global");
        RN_CHECK(plan_lds_bytes(d.nu) <= (size_t)64 * 1024, RN_E_ARG, fn + ": nu is too large for the tile of input differences in LDS");
        RN_HIP(hipSetDevice(device));
        if (int rc = cert_buffers()) return rc;
        // 1: the sweep at y+
        const CertOut co{p_upd, d_certX, d_certU, d_certHz, d_certV};
        if (int rc = launch_sweep(nullptr, 0, nullptr, true, nullptr, nullptr, &co)) return rc;
        // 2: the node terms of x(y), u(y)
        const bool sharded = cutStage > 0 && has_comm();
        PlanArgs pa{};
        pa.f64 = sizeof(T) == 8 ? 1 : 0;
        pa.nodes = d.nodes; pa.nx = d.nx; pa.nu = d.nu; pa.ny = ny; pa.N = d.N; pa.leaves = plan_leaves();
        pa.x = d_certX; pa.u = d_certU; pa.alpha = d_alpha; pa.prevU = d_prevU; pa.prob = d_prob; pa.W = d_W; pa.blo = d_blo; pa.bhi = d_bhi;
        pa.bStrideStage = b_stride_stage(); pa.bStrideNode = b_stride_node();
        pa.parent = d_parent; pa.stageOf = d_stageOf; pa.stageCum = d_stageCum;
        pa.node = d_certNode;
        pa.phase = 0;
        const int tiles = (d.nodes + PLAN_TILE - 1) / PLAN_TILE;
        hipLaunchKernelGGL(k_plan_report<>, dim3(std::max(1, std::min(tiles, numCUs * 4))), dim3(PLAN_THREADS), plan_lds_bytes(d.nu), stream, pa);
        // 3: the flat pass, the fold, the record
        CertArgs a{};
        a.phase = 0; a.f64 = pa.f64;
        a.y = p_upd; a.hz = d_certHz; a.sqrtp = d_sqrtp; a.dy = d_dy; a.blo = d_blo; a.bhi = d_bhi; a.prob = d_prob; a.stageOf = d_stageOf;
        a.bStrideStage = pa.bStrideStage; a.bStrideNode = pa.bStrideNode;
        a.nx = d.nx; a.ny = ny; a.nodes = d.nodes; a.n = ntot();
        a.crownElems = 0; a.crownNodes = 0; a.countCrown = 1;
        if (cutStage > 0) { a.crownNodes = h_stageCum[cutStage]; a.crownElems = (long long)a.crownNodes * ny; a.countCrown = (rank == 0); }
        a.node = d_certNode; a.gammaX = penX; a.gammaS = penXs;
        a.count = (double)(d.nodes - (a.countCrown ? 0 : a.crownNodes)) * (double)d.nx;
        a.partials = cert_partials(); a.ticket = cert_ticket(); a.sums = cert_sums(); a.rec = cert_rec();
        a.finish = sharded ? 0 : 1;
        RN_HIP(hipMemsetAsync(a.ticket, 0, sizeof(double), stream));
        hipLaunchKernelGGL(k_certificate<>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a);
        RN_HIP(hipGetLastError());
        if (sharded) {      // the sums over the ranks, an agreement pass (launch_restart_test), the maxima; then the record from what every rank holds alike
            if (int rc = all_reduce(a.sums, CERT_SUMS, true, "ncclAllReduce(certificate, sums)")) return rc;
            if (int rc = all_reduce(a.sums, CERT_SUMS, true, "ncclAllReduce(certificate, agreement)", 2 /* ncclMax */)) return rc;
            if (int rc = all_reduce(a.sums + CERT_SUMS, CERT_PART - CERT_SUMS, true, "ncclAllReduce(certificate, maxima)", 2 /* ncclMax */)) return rc;
            a.phase = 1;
            hipLaunchKernelGGL(k_certificate<>, dim3(1), dim3(ELT_THREADS), 0, stream, a);
            RN_HIP(hipGetLastError());
        }
        certTaken = true;
        return RN_OK;
    }
    int solve_certificate(double *out) override {
        const std::string fn = "rn_solve_certificate";
        RN_CHECK(out, RN_E_ARG, fn + ": null output");
        if (int rc = cert_run(fn)) return rc;
        RN_HIP(hipMemcpyAsync(out, cert_rec(), CERT_REC * sizeof(double), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        return RN_OK;
    }
    // rn_debug_certificate_hz (include/rapidnet_debug.h): the kernel's own Hz(y), through the staging buffer of rn_get
    int certificate_hz(double *hzXi, double *hzPsi) override {
        RN_CHECK(hzXi && hzPsi, RN_E_ARG, "rn_debug_certificate_hz: null output");
        RN_CHECK(certTaken, RN_E_STATE, "rn_debug_certificate_hz: no certificate was taken yet (rn_solve_certificate)");
        RN_HIP(hipSetDevice(device));
        y_pack(d_certHz, d_tmp, 0, 2 * d.nx, (long long)d.nodes, false);
        RN_HIP(hipGetLastError());
        if (int rc = download(hzXi, d_tmp, (size_t)d.nodes * 2 * d.nx)) return rc;
        y_pack(d_certHz, d_tmp, 2 * d.nx, d.nu, (long long)d.nodes, false);
        RN_HIP(hipGetLastError());
        return download(hzPsi, d_tmp, (size_t)d.nodes * d.nu);
    }
    int solve_certificate_device(void **record) override {
        const std::string fn = "rn_solve_certificate_device";
        RN_CHECK(record, RN_E_ARG, fn + ": null output");
        *record = nullptr;
        if (int rc = cert_run(fn)) return rc;
        *record = cert_rec();
        return RN_OK;
    }
