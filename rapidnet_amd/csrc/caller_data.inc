// caller_data.inc -- members of rn::Ctx<T> through which a caller hands data to a live context or reads it back (included inside the
// struct body of rapidnet_capi.hip).  Entry points served (include/rapidnet.h):
//   raw access        rn_buffer_size, rn_get / rn_set, rn_get_range / rn_set_range, rn_device_pointer
//   operator blocks   rn_get_operator / rn_set_operator (one node), rn_get_operators / rn_set_operators and their _device forms (all nodes)
//   tree data         rn_set_tree_data, rn_set_tree_data_device, rn_get_tree_data
//   bounds            rn_set_bounds, rn_set_bounds_device, rn_get_bounds, rn_get_bounds_layout
// What the forms share stands once: the argument check of caller arrays (check_caller_arrays), the staging buffer of the host forms
// (HostStage, stage_open / stage_copy / stage_close), the raw getters' and setters' implementation (raw_get / raw_set) and the geometry
// of Phi, Psi, D, F inside a node's block (op_geom).

    // ---- raw access --------------------------------------------------------------------------------------
    // maps a buffer id to (y-layout base, offset, dim); false: not a dual-shaped buffer (plain() knows the others).  The bases are read
    // here, at call time: p_xi, p_upd and p_acc_view swap during a solve.
    bool ymap(int id, T **base, int *off, int *dim) const {
        const int nx = d.nx, nu = d.nu;
        // a (xi, psi) pair of ids is the two halves of one [node][2nx + nu] vector: xi its first 2nx columns, psi the nu behind them
        struct Pair { int xi, psi; T *Ctx::*base; bool fbe; };
        static const Pair pairs[] = {
            {RN_BUF_XI, RN_BUF_PSI, &Ctx::p_xi, false}, {RN_BUF_ACC_XI, RN_BUF_ACC_PSI, &Ctx::p_acc_view, false},
            {RN_BUF_UPD_XI, RN_BUF_UPD_PSI, &Ctx::p_upd, false}, {RN_BUF_PRIMAL_XI, RN_BUF_PRIMAL_PSI, &Ctx::d_hx, false},
            {RN_BUF_DUAL_XI, RN_BUF_DUAL_PSI, &Ctx::d_z, false}, {RN_BUF_RES_XI, RN_BUF_RES_PSI, &Ctx::d_res, false},
            // the FBE / NAMA vectors exist once rn_set_algorithm selected one of them (d_matS)
            {RN_BUF_PREV_XI, RN_BUF_PREV_PSI, &Ctx::d_prevY, true}, {RN_BUF_LBFGS_CUR_YVEC_XI, RN_BUF_LBFGS_CUR_YVEC_PSI, &Ctx::d_g, true},
            {RN_BUF_LBFGS_PREV_YVEC_XI, RN_BUF_LBFGS_PREV_YVEC_PSI, &Ctx::d_gPrev, true}, {RN_BUF_LBFGS_DIR_XI, RN_BUF_LBFGS_DIR_PSI, &Ctx::d_dir, true},
            {RN_BUF_PRIMAL_XI_DIR, RN_BUF_PRIMAL_PSI_DIR, &Ctx::d_hxDir, true}};
        for (const Pair &p : pairs) {
            if (id != p.xi && id != p.psi) continue;
            if (p.fbe && !d_matS) return false;
            *base = this->*p.base; *off = id == p.xi ? 0 : 2 * nx; *dim = id == p.xi ? 2 * nx : nu;
            return true;
        }
        // the scaled bounds: columns of their own in the tables of lower and upper bounds
        const struct { int id; T *base; int off, dim; } bnd[] = {{RN_BUF_XMIN, d_lo, 0, nx}, {RN_BUF_XMAX, d_hi, 0, nx}, {RN_BUF_XS, d_lo, nx, nx},
                                                                 {RN_BUF_UMIN, d_lo, 2 * nx, nu}, {RN_BUF_UMAX, d_hi, 2 * nx, nu}};
        for (const auto &b : bnd)
            if (id == b.id) { *base = b.base; *off = b.off; *dim = b.dim; return true; }
        return false;
    }
    T *plain(int id, size_t *n) const {
        const size_t N_ = d.nodes;
        switch (id) {
            case RN_BUF_X: *n = N_ * d.nx; return d_x;
            case RN_BUF_U: *n = N_ * d.nu; return d_u;
            case RN_BUF_V: *n = N_ * d.nv; return d_v;
            case RN_BUF_UHAT: *n = N_ * d.nu; return d_uhat;
            case RN_BUF_E: *n = N_ * d.nx; return d_e;
            case RN_BUF_BETA: *n = N_ * d.nv; return d_beta;
            case RN_BUF_ALPHA: *n = N_ * d.nu; return d_alpha;
            case RN_BUF_XDIR: *n = d_xdir ? N_ * d.nx : 0; return d_xdir;
            case RN_BUF_UDIR: *n = d_udir ? N_ * d.nu : 0; return d_udir;
            case RN_BUF_CERT_X: *n = certTaken ? N_ * d.nx : 0; return certTaken ? d_certX : nullptr;      // (rn_solve_certificate: x(y), u(y); read-only)
            case RN_BUF_CERT_U: *n = certTaken ? N_ * d.nu : 0; return certTaken ? d_certU : nullptr;
            default: *n = 0; return nullptr;
        }
    }
    // The scaled bounds (Engine.cuh:294-314 getSysXmin ... getSysUmax; Engine.cu:433-463) live interleaved in the dual layout here ([node][ny]: the
    // fused dual update rebuilds them from tables).  A caller that asks for their device pointers gets node-major copies in the reference's layout,
    // made on the first request (5 arrays, (3 nx + 2 nu) reals per node) and refreshed by every later factor step.
    T *d_bnd[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // columns off .. off + dim of `nodes` rows of a y-layout vector to (toY: from) a node-major array
    void y_pack(T *y, T *flat, int off, int dim, long long nodes, bool toY) {
        hipLaunchKernelGGL(k_pack<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, y, flat, ny, off, dim, nodes, toY ? 1 : 0);
    }
    int refresh_bounds_copies() {
        if (!d_bnd[0]) return RN_OK;
        const int ids[5] = {RN_BUF_XMIN, RN_BUF_XMAX, RN_BUF_XS, RN_BUF_UMIN, RN_BUF_UMAX};
        for (int i = 0; i < 5; i++) {
            T *b; int off, dim;
            if (!ymap(ids[i], &b, &off, &dim)) continue;
            y_pack(b, d_bnd[i], off, dim, (long long)d.nodes, false);
        }
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    int device_pointer(int id, void **ptr, size_t *n, int *prec) override {
        RN_CHECK(ptr && n && prec, RN_E_ARG, "rn_device_pointer: null output");
        *ptr = nullptr; *n = 0; *prec = sizeof(T) == 8 ? RN_F64 : RN_F32;
        if (id >= RN_BUF_XMIN && id <= RN_BUF_UMAX) {
            RN_CHECK(factored, RN_E_STATE, "rn_device_pointer: the scaled bounds exist after rn_factor_step");
            RN_HIP(hipSetDevice(device));
            if (!d_bnd[0]) {
                const size_t dims[5] = {(size_t)d.nx, (size_t)d.nx, (size_t)d.nx, (size_t)d.nu, (size_t)d.nu};
                for (int i = 0; i < 5; i++) if (int rc = dalloc(&d_bnd[i], (size_t)d.nodes * dims[i])) return rc;
                if (int rc = refresh_bounds_copies()) return rc;
                RN_HIP(hipStreamSynchronize(stream));
            }
            const int i = id - RN_BUF_XMIN;
            *ptr = d_bnd[i]; *n = (size_t)d.nodes * (i < 3 ? d.nx : d.nu);
            return RN_OK;
        }
        size_t cnt = 0;
        if (id == RN_BUF_V) { vEager = true; if (int rc = v_flush()) return rc; }      // from now on v is computed with every sweep that stores the primal iterates
        T *p = plain(id, &cnt);
        RN_CHECK(p != nullptr && cnt > 0, RN_E_ARG, "rn_device_pointer: this buffer is not kept in the reference's layout on the device (or not allocated yet): use rn_get");
        *ptr = p; *n = cnt;
        return RN_OK;
    }
    size_t buffer_size(int id) const override {
        T *b; int off, dim; size_t n;
        if (ymap(id, &b, &off, &dim)) return (size_t)d.nodes * dim;
        plain(id, &n);
        return n;
    }
    // rn_get / rn_set are rn_get_range / rn_set_range over the whole buffer (whole: first = 0 and n must be the buffer's size).  `fn` is
    // the entry point the caller called: every message names it.  Elements [first, first + n) in the reference's node-major layout.
    // What raw_span finds: `nodes` whole nodes of a dual-shaped buffer from y on (columns off .. off + dim), or n elements from p on.
    struct RawSpan { T *y; int off, dim; long long nodes; T *p; };
    int raw_span(const std::string &fn, bool write, bool whole, int id, size_t first, size_t n, RawSpan *s) {
        T *b; int off, dim; size_t cnt;
        if (ymap(id, &b, &off, &dim)) {
            RN_CHECK(!write || id < RN_BUF_XMIN || id > RN_BUF_UMAX, RN_E_ARG, fn + ": the scaled bounds are read-only");
            cnt = (size_t)d.nodes * dim;
            if (whole) RN_CHECK(n == cnt, RN_E_ARG, fn + ": size mismatch");
            else RN_CHECK(first % dim == 0 && n % dim == 0 && first + n <= cnt, RN_E_ARG, fn + ": dual-shaped buffers are addressed in whole nodes");
            *s = RawSpan{b + (first / dim) * ny, off, dim, (long long)(n / dim), nullptr};
            return RN_OK;
        }
        // A pending v (v_flush) is the one difference between the whole-buffer and the range form of a set, and it is meant: a set of the
        // whole buffer drops the product without launching it (the caller's values replace every element), a partial set computes it first
        // (the rest of the buffer must be the sweep's) -- as every get does.
        if (id == RN_BUF_V) {
            if (write && whole) vPending = false;
            else if (int rc = v_flush()) return rc;
        }
        if (id == RN_BUF_CERT_X || id == RN_BUF_CERT_U) {
            RN_CHECK(!write, RN_E_ARG, fn + ": the certificate's x(y), u(y) are read-only");
            RN_CHECK(certTaken, RN_E_ARG, fn + ": no certificate was taken yet (rn_solve_certificate): the buffer is empty");
        }
        T *p = plain(id, &cnt);
        RN_CHECK(p != nullptr, RN_E_ARG, fn + ": unknown buffer id");
        if (whole) RN_CHECK(n == cnt, RN_E_ARG, fn + ": size mismatch");
        else RN_CHECK(first + n <= cnt, RN_E_ARG, fn + ": range outside the buffer");
        *s = RawSpan{nullptr, 0, 0, 0, p + first};
        return RN_OK;
    }
    int raw_get(const char *name, bool whole, int id, size_t first, size_t n, double *host) {
        const std::string fn(name);
        RN_CHECK(host, RN_E_ARG, fn + ": null host pointer");
        RN_HIP(hipSetDevice(device));
        RawSpan s;
        if (int rc = raw_span(fn, false, whole, id, first, n, &s)) return rc;
        if (!s.y) return download(host, s.p, n);
        y_pack(s.y, d_tmp, s.off, s.dim, s.nodes, false);
        RN_HIP(hipGetLastError());
        return download(host, d_tmp, n);
    }
    int raw_set(const char *name, bool whole, int id, size_t first, size_t n, const double *host) {
        const std::string fn(name);
        RN_CHECK(host, RN_E_ARG, fn + ": null host pointer");
        RN_HIP(hipSetDevice(device));
        RawSpan s;
        if (int rc = raw_span(fn, true, whole, id, first, n, &s)) return rc;
        if (!s.y) {
            if (id == RN_BUF_UHAT || id == RN_BUF_E || id == RN_BUF_BETA) { affine_ready = true; aux_dirty = true; }
            return upload(s.p, host, n);
        }
        if (int rc = upload(d_tmp, host, n)) return rc;
        y_pack(s.y, d_tmp, s.off, s.dim, s.nodes, true);
        RN_HIP(hipGetLastError());
        RN_HIP(hipStreamSynchronize(stream));
        if (id == RN_BUF_ACC_XI || id == RN_BUF_ACC_PSI) {   // the view becomes the sweep input
            if (p_acc_view != p_acc) std::swap(p_acc, p_acc_other);
            acc_ready = true;
        } else if (id == RN_BUF_XI || id == RN_BUF_PSI || id == RN_BUF_UPD_XI || id == RN_BUF_UPD_PSI) {
            acc_ready = false;
        }
        return RN_OK;
    }
    int get(int id, double *host, size_t n) override { return raw_get("rn_get", true, id, 0, n, host); }
    int set(int id, const double *host, size_t n) override { return raw_set("rn_set", true, id, 0, n, host); }
    int get_range(int id, size_t first, size_t n, double *host) override { return raw_get("rn_get_range", false, id, first, n, host); }
    int set_range(int id, size_t first, size_t n, const double *host) override { return raw_set("rn_set_range", false, id, first, n, host); }
    // ---- operator blocks ---------------------------------------------------------------------------------
    // Where RN_OP_PHI, _PSI, _D, _F (0 .. 3) lie inside a node's interleaved block of ny columns: [Phi | Psi] in rows 0 .. nv - 1 over
    // [D | F] in rows nv .. 2 nv - 1; Phi and D take the 2 nx xi columns, Psi and F the nu psi columns behind them.  Each is nv x cols, col-major.
    struct OpGeom { int cols, c0, r0; };
    OpGeom op_geom(int op) const {
        const bool xiCols = (op == RN_OP_PHI || op == RN_OP_D), top = (op == RN_OP_PHI || op == RN_OP_PSI);
        return OpGeom{xiCols ? 2 * d.nx : d.nu, xiCols ? 0 : 2 * d.nx, top ? 0 : d.nv};
    }
    size_t op_elems(int op) const { return (size_t)d.nv * op_geom(op).cols; }      // one node's
    int get_operator(int op, int node, double *host, size_t n) override {
        RN_CHECK(factored, RN_E_STATE, "rn_get_operator before rn_factor_step");
        RN_CHECK(host && node >= 0 && node < d.nodes, RN_E_ARG, "rn_get_operator: bad node");
        const int nx = d.nx, nu = d.nu, nv = d.nv;
        if (int rc = refresh_h_prob()) return rc;
        const double p = h_prob[node];
        if (op == RN_OP_OMEGA) { RN_CHECK(n == (size_t)nv * nv, RN_E_ARG, "rn_get_operator: size"); for (size_t i = 0; i < n; i++) host[i] = h_Rinv[i] / p; return RN_OK; }
        if (op == RN_OP_G) { RN_CHECK(n == (size_t)nv * nx, RN_E_ARG, "rn_get_operator: size"); for (size_t i = 0; i < n; i++) host[i] = h_Bbt[i]; return RN_OK; }
        if (op == RN_OP_THETA) {
            RN_CHECK(n == (size_t)nv * nx, RN_E_ARG, "rn_get_operator: size");
            std::vector<double> t((size_t)nv * nx);
            h_gemm(false, false, nv, nx, nv, h_Rinv.data(), nv, h_Bbt.data(), nv, t.data());
            for (size_t i = 0; i < n; i++) host[i] = -0.5 * t[i] / p;
            return RN_OK;
        }
        RN_CHECK(op == RN_OP_PHI || op == RN_OP_PSI || op == RN_OP_D || op == RN_OP_F, RN_E_ARG, "rn_get_operator: unknown operator id");
        const OpGeom g = op_geom(op);
        const int cols = g.cols;
        RN_CHECK(n == op_elems(op), RN_E_ARG, "rn_get_operator: size");
        RN_HIP(hipSetDevice(device));
        if (structured) {   // no stored blocks: evaluate the factor-step formula (kernels.hpp, k_expand_operators) on the host
            const bool xiCols = g.c0 == 0, top = g.r0 == 0;
            const int k = h_stageOf[node];
            const double sp = std::sqrt(p);
            const double *dk = h_diag.data() + (size_t)k * (2 * nx + nu);
            for (int c = 0; c < cols; c++) {
                const int j = xiCols ? c % nx : c;
                const double dc = xiCols ? dk[nu + c] : dk[c];
                const double *m = top ? (xiCols ? h_T1.data() : h_T2.data()) + (size_t)j * nv : (xiCols ? h_Bbt.data() : h_Lt.data()) + (size_t)j * nv;
                const double sc = top ? -0.5 * dc / sp : sp * dc;
                for (int r = 0; r < nv; r++) host[r + (size_t)c * nv] = sc * m[r];
            }
            return RN_OK;
        }
        std::vector<double> blk((size_t)ny * LD);
        if (int rc = download_block(node, blk.data())) return rc;
        for (int c = 0; c < cols; c++) for (int r = 0; r < nv; r++) host[r + (size_t)c * nv] = blk[(size_t)(g.c0 + c) * LD + g.r0 + r];
        return RN_OK;
    }
    // One node's block as the caller wants it (the counterpart of rn_get_operator; the reference's Engine hands out the device pointers of
    // these arrays, Engine.cuh:170-230, so a caller may overwrite any block): Phi_i, Psi_i, D_i, Ftil_i -- the blocks solveStep multiplies
    // with at SmpcController.cu:617-638.  Omega / Theta / G are K identical copies of shared matrices in the reference: not per-node here.
    int set_operator(int op, int node, const double *host, size_t n) override {
        RN_CHECK(factored, RN_E_STATE, "rn_set_operator before rn_factor_step");
        RN_CHECK(host && node >= 0 && node < d.nodes, RN_E_ARG, "rn_set_operator: bad node");
        RN_CHECK(op == RN_OP_PHI || op == RN_OP_PSI || op == RN_OP_D || op == RN_OP_F, RN_E_ARG,
                 "rn_set_operator: only the per-node blocks Phi, Psi, D, F can be handed in (Omega, Theta, G are shared matrices scaled by p_i)");
        const OpGeom g = op_geom(op);
        const int nv = d.nv;
        RN_CHECK(n == op_elems(op), RN_E_ARG, "rn_set_operator: size");
        RN_CHECK(opsMode != RN_OPS_STRUCTURED, RN_E_STATE, "rn_set_operator: the context was created with RN_OPS_STRUCTURED (no per-node blocks); use RN_OPS_AUTO or RN_OPS_DENSE");
        RN_HIP(hipSetDevice(device));
        if (structured) { if (int rc = materialise_dense()) return rc; }
        lip_invalidate();
        std::vector<double> blk((size_t)ny * LD);
        if (int rc = download_block(node, blk.data())) return rc;
        for (int c = 0; c < g.cols; c++) for (int r = 0; r < nv; r++) blk[(size_t)(g.c0 + c) * LD + g.r0 + r] = host[r + (size_t)c * nv];
        return upload_block(node, blk.data());      // (fp32 storage: the caller's values rounded to nearest)
    }
    // ---- caller arrays: the argument check of every bulk form, the staging buffer of the host forms -----------
    // one array a caller hands in (p NULL: not given): `count` elements, `shape` says so in words; dev: where a host form staged it
    struct CallerArray { const void *p; size_t count; const char *shape; void *dev; };
    // a caller's device array: memory of this context's device (hipPointerGetAttributes) that holds `bytes` bytes from p on.  Anything
    // else -- a host pointer above all -- is refused here, before a kernel could see it
    int check_device_array(const void *p, size_t bytes, size_t elem, const std::string &what, const char *shape) {
        RN_CHECK(((uintptr_t)p & (elem - 1)) == 0, RN_E_ARG, what + ": a pointer is not aligned to its element type");
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); err = what + ": a pointer is not device memory"; return RN_E_ARG; }
        RN_CHECK(at.type == hipMemoryTypeDevice, RN_E_ARG, what + ": a pointer is not device memory");
        RN_CHECK(at.device == device, RN_E_ARG, what + ": a pointer is memory of another device than the context's");
        hipDeviceptr_t base = nullptr; size_t len = 0;
        if (hipMemGetAddressRange(&base, &len, (hipDeviceptr_t)p) == hipSuccess)
            RN_CHECK((const char *)p >= (const char *)base && (size_t)((const char *)p - (const char *)base) + bytes <= len, RN_E_ARG,
                     what + ": an array is shorter than " + shape + " elements");
        else (void)hipGetLastError();
        return RN_OK;
    }
    // some array given, a known precision, and -- device forms -- every given array device memory of this context's device
    int check_caller_arrays(const std::string &what, int callerPrec, bool dev, const CallerArray *a, int n) {
        static const char *const number[] = {"no", "one", "two", "three", "four", "five"};
        int given = 0;
        for (int i = 0; i < n; i++) given += a[i].p != nullptr;
        RN_CHECK(given > 0, RN_E_ARG, what + ": all " + number[n] + " arrays are NULL");
        RN_CHECK(callerPrec == RN_F64 || callerPrec == RN_F32, RN_E_ARG, what + ": precision is RN_F32 or RN_F64");
        const size_t elem = callerPrec == RN_F64 ? 8 : 4;
        for (int i = 0; dev && i < n; i++)
            if (a[i].p) { if (int rc = check_device_array(a[i].p, a[i].count * elem, elem, what, a[i].shape)) return rc; }
        return RN_OK;
    }
    // The host forms run the kernel of their device form behind a device buffer that lives inside the call: hipMalloc'd here, outside
    // dalloc -- not one of the context's allocations, not counted in allocatedBytes.  Everything that uses it goes to the context's stream;
    // release() synchronises that stream and then frees.  `first` keeps the first error of what was enqueued (stage_close reports it).
    struct HostStage {
        hipStream_t stream;
        char *base = nullptr;
        hipError_t first = hipSuccess;
        explicit HostStage(hipStream_t s) : stream(s) {}
        HostStage(const HostStage &) = delete;
        ~HostStage() { (void)release(); }
        bool ok() const { return first == hipSuccess; }
        void note(hipError_t e) { if (first == hipSuccess) first = e; }
        hipError_t release() {
            if (!base) return hipSuccess;
            const hipError_t es = hipStreamSynchronize(stream);
            (void)hipFree(base);
            base = nullptr;
            return es;
        }
    };
    // lays the given arrays (doubles, `count` each) out at 256-byte-rounded offsets of one buffer and allocates it: a[i].dev
    int stage_open(HostStage &st, CallerArray *a, int n) {
        const auto room = [](const CallerArray &c) { return c.p ? (c.count * sizeof(double) + 255) / 256 * 256 : (size_t)0; };
        size_t bytes = 0, at = 0;
        for (int i = 0; i < n; i++) bytes += room(a[i]);
        RN_HIP(hipMalloc((void **)&st.base, bytes));
        for (int i = 0; i < n; i++) if (a[i].p) { a[i].dev = st.base + at; at += room(a[i]); }
        return RN_OK;
    }
    // the given arrays to (toHost: from) their places in the buffer, on the context's stream; stops at the first error
    void stage_copy(HostStage &st, const CallerArray *a, int n, bool toHost) {
        for (int i = 0; i < n && st.ok(); i++) if (a[i].p) {
            const size_t bytes = a[i].count * sizeof(double);
            st.note(toHost ? hipMemcpyAsync(const_cast<void *>(a[i].p), a[i].dev, bytes, hipMemcpyDeviceToHost, stream)
                           : hipMemcpyAsync(a[i].dev, a[i].p, bytes, hipMemcpyHostToDevice, stream));
        }
    }
    // the end of every form, after everything that uses the buffer is enqueued: synchronise, free, then report the first error
    int stage_close(HostStage &st) {
        const hipError_t es = st.release();
        RN_HIP(st.first);
        RN_HIP(es);
        return RN_OK;
    }
    // ---- all blocks at once (rn_set_operators / rn_get_operators and their _device forms; k_pack_operators, k_misc.hpp) ----
    static constexpr size_t PACK_STAGING_BYTES = (size_t)64 << 20;   // the host forms' device staging buffer (rapidnet.h says so)
    // `count` nodes from `node0` on, to or from caller arrays that START at node0; one launch on the context's stream
    void pack_launch(bool toBlocks, bool callerF64, void *const op[4], int node0, int count) {
        PackOpsArgs a{};
        a.A = store32() ? (void *)(d_A32 + (size_t)node0 * strideA) : (void *)(d_A + (size_t)node0 * strideA);
        a.strideA = strideA; a.LD = LD; a.nv = d.nv; a.nx2 = 2 * d.nx; a.nu = d.nu; a.nodes = count;
        for (int i = 0; i < 4; i++) a.op[i] = op[i];
        a.callerF64 = callerF64 ? 1 : 0; a.storedF64 = block_elem() == 8 ? 1 : 0;
        const long long perNode = (long long)ny * (LD / (16 / block_elem()));
        const int gx = (int)std::min<long long>((perNode + PACK_THREADS - 1) / PACK_THREADS, (long long)numCUs * 4);
        const int gy = std::max(1, std::min(count, numCUs * 4 / gx));
        a.toBlocks = toBlocks ? 1 : 0;
        hipLaunchKernelGGL(k_pack_operators<>, dim3(gx, gy), dim3(PACK_THREADS), 0, stream, a);
    }
    // set = true: rn_set_operators(_device), false: rn_get_operators(_device); op: Phi, Psi, D, F of `nodes` nodes each (the set forms only read them)
    int pack_operators(bool set, size_t nodes, int callerPrec, bool dev, void *const *op) {
        const std::string what = std::string(set ? "rn_set_operators" : "rn_get_operators") + (dev ? "_device" : "");
        RN_CHECK(factored, RN_E_STATE, what + " before rn_factor_step");
        RN_CHECK(nodes == (size_t)d.nodes, RN_E_ARG, what + ": nodes must be the context's (local) node count");
        if (set) RN_CHECK(opsMode != RN_OPS_STRUCTURED, RN_E_STATE, what + ": the context was created with RN_OPS_STRUCTURED (no per-node blocks); use RN_OPS_AUTO or RN_OPS_DENSE");
        else RN_CHECK(!structured, RN_E_STATE, what + ": the context holds no dense blocks (structured operator mode); rn_get_operator evaluates one node's block");
        RN_HIP(hipSetDevice(device));
        CallerArray a[4];
        for (int i = 0; i < 4; i++) a[i] = CallerArray{op[i], nodes * op_elems(i), "nodes x nv x columns", nullptr};
        if (int rc = check_caller_arrays(what, callerPrec, dev, a, 4)) return rc;
        if (set && structured) { if (int rc = materialise_dense()) return rc; }     // (RN_OPS_AUTO, first block of the caller's: allocates and synchronises, once)
        if (set) lip_invalidate();
        if (!dev) return pack_staged(set, a);
        pack_launch(set, callerPrec == RN_F64, op, 0, d.nodes);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    int set_operators(size_t nodes, int callerPrec, bool dev, const void *const *op) override {
        void *p[4] = {const_cast<void *>(op[0]), const_cast<void *>(op[1]), const_cast<void *>(op[2]), const_cast<void *>(op[3])};   // (read only: TO_BLOCKS)
        return pack_operators(true, nodes, callerPrec, dev, p);
    }
    int get_operators(size_t nodes, int callerPrec, bool dev, void *const *op) override { return pack_operators(false, nodes, callerPrec, dev, op); }
    // the host forms: the same kernel behind a staging buffer of at most PACK_STAGING_BYTES (one node's arrays if those are larger; the
    // 256-byte rounding of four offsets is taken off first), whole nodes per chunk
    int pack_staged(bool toBlocks, const CallerArray *all) {
        size_t per[4], perNode = 0;      // one node's elements of each given array, one node's bytes
        for (int i = 0; i < 4; i++) { per[i] = all[i].p ? op_elems(i) : 0; perNode += per[i] * sizeof(double); }
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)d.nodes, (PACK_STAGING_BYTES - 4 * 256) / perNode));
        CallerArray a[4];
        for (int i = 0; i < 4; i++) a[i] = CallerArray{all[i].p, (size_t)chunk * per[i], all[i].shape, nullptr};
        HostStage st(stream);
        if (int rc = stage_open(st, a, 4)) return rc;
        void *dv[4] = {a[0].dev, a[1].dev, a[2].dev, a[3].dev};
        for (int n0 = 0; n0 < d.nodes && st.ok(); n0 += chunk) {
            const int cnt = std::min(chunk, d.nodes - n0);
            for (int i = 0; i < 4; i++) if (a[i].p) { a[i].p = static_cast<const double *>(all[i].p) + (size_t)n0 * per[i]; a[i].count = (size_t)cnt * per[i]; }
            if (toBlocks) stage_copy(st, a, 4, false);
            if (st.ok()) { pack_launch(toBlocks, true, dv, n0, cnt); st.note(hipGetLastError()); }
            if (!toBlocks) stage_copy(st, a, 4, true);
        }
        return stage_close(st);
    }
    // ---- scenario probabilities and tree errors in place (rn_set_tree_data, rn_set_tree_data_device, rn_get_tree_data; k_tree_data, k_misc.hpp) ----
    bool lib_sharded() const { return nranks > 1 && !globalNode.empty() && d_gmap != nullptr; }   // made by rn_create_sharded
    int refresh_h_prob() {
        if (!hProbStale) return RN_OK;
        RN_HIP(hipSetDevice(device));
        if (d_prob64) {
            RN_HIP(hipMemcpyAsync(h_prob.data(), d_prob64, (size_t)d.nodes * sizeof(double), hipMemcpyDeviceToHost, stream));
            RN_HIP(hipStreamSynchronize(stream));
        } else if (int rc = download(h_prob.data(), d_prob, (size_t)d.nodes)) return rc;
        hProbStale = false;
        return RN_OK;
    }
    void tree_data_launch(bool callerF64, const void *prob, const void *errD, const void *errP) {
        TreeDataArgs a{};
        a.prob = prob; a.errD = errD; a.errP = errP; a.ctxF64 = sizeof(T) == 8 ? 1 : 0; a.callerF64 = callerF64 ? 1 : 0;
        a.gmap = lib_sharded() ? d_gmap : nullptr;
        a.nodes = d.nodes; a.nd = d.nd; a.nu = d.nu;
        a.dprob = d_prob; a.dsqrtp = d_sqrtp; a.derrD = d_errD; a.derrP = d_errP; a.prob64 = d_prob64; a.bad = d_treeBad;
        a.nPar = lib_sharded() ? nCutPar : 0; a.cutFirst = cutFirstFull; a.cutC0 = d_cutC0; a.cutNc = d_cutNc; a.fullP = d_fullP; a.fullE = d_fullE;
        a.momE = d_momE; a.momP = d_momP;
        const long long work = std::max<long long>((long long)d.nodes * std::max(std::max(d.nd, d.nu), 1), (long long)a.nPar * (d.nd + 1));
        const int blocks = (int)std::max<long long>(1, std::min<long long>(TREE_MAX_BLOCKS, (work + TREE_THREADS - 1) / TREE_THREADS));
        hipLaunchKernelGGL(k_tree_data<>, dim3(blocks), dim3(TREE_THREADS), 0, stream, a);
    }
    int set_tree_data(size_t nodes, int callerPrec, bool dev, const void *prob, const void *errD, const void *errP) override {
        const std::string what = dev ? "rn_set_tree_data_device" : "rn_set_tree_data";
        const bool lib = lib_sharded();
        RN_CHECK(nodes == (size_t)(lib ? fullNodes : d.nodes), RN_E_ARG,
                 what + (lib ? ": nodes must be the FULL tree's node count on a context made by rn_create_sharded" : ": nodes must be the context's node count"));
        RN_CHECK(!lib || !(prob || errD) || (cutContiguous && d_momE), RN_E_STATE, what + ": the children of a cut parent are not contiguous in the full tree");
        RN_HIP(hipSetDevice(device));
        CallerArray a[3] = {{prob, nodes, "nodes", nullptr}, {errD, nodes * (size_t)d.nd, "nodes x nd", nullptr}, {errP, nodes * (size_t)d.nu, "nodes x nu", nullptr}};
        if (int rc = check_caller_arrays(what, callerPrec, dev, a, 3)) return rc;
        if (!dev && prob) {
            const double *p = static_cast<const double *>(prob);
            for (size_t i = 0; i < nodes; i++) RN_CHECK(p[i] > 0.0 && std::isfinite(p[i]), RN_E_ARG, what + ": probNode must be positive and finite");
        }
        if (prob && factored) { if (int rc = v_flush()) return rc; }      // (a pending v is the previous probabilities')
        HostStage st(stream);
        if (dev) {
            tree_data_launch(callerPrec == RN_F64, prob, errD, errP);
        } else {   // the same kernel behind a staging copy
            if (int rc = stage_open(st, a, 3)) return rc;
            stage_copy(st, a, 3, false);
            if (!st.ok()) return stage_close(st);
            tree_data_launch(true, a[0].dev, a[1].dev, a[2].dev);
        }
        st.note(hipGetLastError());
        int rcx = RN_OK;
        if (st.ok() && prob && factored) {      // what of the factor step depends on p, in the storage type in force; in front of the synchronisation
            rcx = launch_expand();
            if (rcx == RN_OK) rcx = refresh_bounds_copies();
        }
        if (int rc = stage_close(st)) return rc;      // (a device form holds no buffer: no synchronisation)
        if (rcx != RN_OK) return rcx;
        if (prob) {
            if (dev) { treeCheckPending = true; hProbStale = true; }
            else {
                const double *p = static_cast<const double *>(prob);
                for (int i = 0; i < d.nodes; i++) h_prob[i] = p[lib ? globalNode[i] : i];
                treeCheckPending = false; treeBad = false; treeBadCount = 0; hProbStale = false;
            }
            affine_ready = false; linConstValid = false; aux_dirty = true;      // the affine terms and every control-step constant read p
            lip_invalidate();      // (the operators carry powers of p_i: a held Lipschitz estimate is the old tree's)
        }
        if ((prob || errD) && cutStage > 0 && nranks > 1 && !lib) moments_set = false;   // sharded by hand: the caller's moments are the old tree's
        return RN_OK;
    }
    int get_tree_data(size_t nodes, double *prob, double *errD, double *errP) override {
        RN_CHECK(prob || errD || errP, RN_E_ARG, "rn_get_tree_data: all three arrays are NULL");
        RN_CHECK(nodes == (size_t)d.nodes, RN_E_ARG, "rn_get_tree_data: nodes must be the context's (local) node count");
        RN_HIP(hipSetDevice(device));
        if (prob) {
            if (d_prob64) {
                RN_HIP(hipMemcpyAsync(prob, d_prob64, nodes * sizeof(double), hipMemcpyDeviceToHost, stream));
                RN_HIP(hipStreamSynchronize(stream));
            } else if (int rc = download(prob, d_prob, nodes)) return rc;
        }
        if (errD) { if (int rc = download(errD, d_errD, nodes * d.nd)) return rc; }
        if (errP) { if (int rc = download(errP, d_errP, nodes * d.nu)) return rc; }
        return RN_OK;
    }
    // ---- box and safety bounds per stage or per node in place (rn_set_bounds, rn_set_bounds_device, rn_get_bounds; k_tree_data, k_misc.hpp;
    // replaces Engine.cuh:294-314 getSysXmin() ... getSysUmax() and Engine.cu preconditionConstraintX/U) ----
    void bounds_launch(int gran, bool callerF64, const void *const *b) {
        TreeDataArgs a{};
        a.ctxF64 = sizeof(T) == 8 ? 1 : 0; a.callerF64 = callerF64 ? 1 : 0;
        a.nodes = d.nodes; a.nd = d.nd; a.nu = d.nu; a.nx = d.nx; a.ny = ny;
        for (int i = 0; i < 5; i++) { a.bnd[i] = b[i]; a.bndCopy[i] = d_bnd[i]; }
        a.bRows = (int)bounds_rows(gran); a.bRowStage = gran == RN_BOUNDS_PER_STAGE ? 1 : 0; a.bRowNode = gran == RN_BOUNDS_PER_NODE ? 1 : 0;
        a.stageOf = d_stageOf; a.sqrtpIn = d_sqrtp; a.dy = d_dy;
        a.blo = d_bloG[gran]; a.bhi = d_bhiG[gran]; a.lo = d_lo; a.hi = d_hi;
        const long long work = (long long)d.nodes * ny;
        const int blocks = (int)std::max<long long>(1, std::min<long long>(BOUNDS_MAX_BLOCKS, (work + TREE_THREADS - 1) / TREE_THREADS));
        hipLaunchKernelGGL(k_tree_data<>, dim3(blocks), dim3(TREE_THREADS), 0, stream, a);
    }
    int set_bounds(int gran, size_t rows, int callerPrec, bool dev, const void *const *b) override {
        const std::string what = dev ? "rn_set_bounds_device" : "rn_set_bounds";
        RN_CHECK(factored, RN_E_STATE, what + " before rn_factor_step");
        RN_CHECK(bounds::known(gran), RN_E_ARG, what + ": granularity is RN_BOUNDS_SHARED, _PER_STAGE or _PER_NODE");
        RN_CHECK(rows == bounds_rows(gran), RN_E_ARG, what + ": rows must be 1 (shared), dims.N (per stage) or the context's (local) node count (per node)");
        RN_CHECK(bounds::table_fits(rows, ny), RN_E_ARG, what + ": the table does not fit a 32-bit index");
        RN_HIP(hipSetDevice(device));
        const int nx = d.nx, nu = d.nu;
        CallerArray a[5];
        int given = 0;
        for (int i = 0; i < 5; i++) { a[i] = CallerArray{b[i], rows * (i < 3 ? nx : nu), i < 3 ? "rows x nx" : "rows x nu", nullptr}; given += b[i] != nullptr; }
        if (int rc = check_caller_arrays(what, callerPrec, dev, a, 5)) return rc;
        RN_CHECK(gran == boundsGran || given == 5, RN_E_ARG, what + ": a call that changes the granularity needs all five arrays");
        if (!dev) {
            // every value finite, lower <= upper pair by pair; the half of a pair that was not given as the context holds it (bounds.hpp)
            const double *hb[5], *cur[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            for (int i = 0; i < 5; i++) hb[i] = static_cast<const double *>(b[i]);
            bool need[5];
            bounds::needed_from_context(hb, need);
            std::vector<double> held[5];
            if (need[0] || need[1] || need[3] || need[4]) {
                double *out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
                for (int i = 0; i < 5; i++) if (need[i]) { held[i].resize(a[i].count); out[i] = held[i].data(); cur[i] = out[i]; }
                if (int rc = get_bounds(rows, out)) return rc;
            }
            const int bad = bounds::validate(rows, nx, nu, hb, cur);
            RN_CHECK(bad != bounds::NOT_FINITE, RN_E_ARG, what + ": a bound is not finite");
            RN_CHECK(bad != bounds::XMIN_ABOVE_XMAX, RN_E_ARG, what + ": xmin > xmax");
            RN_CHECK(bad != bounds::UMIN_ABOVE_UMAX, RN_E_ARG, what + ": umin > umax");
        }
        if (!d_bloG[gran]) {      // the first set at this granularity: its table, kept from here on
            if (int rc = dalloc(&d_bloG[gran], rows * (size_t)ny)) return rc;
            if (int rc = dalloc(&d_bhiG[gran], rows * (size_t)ny)) return rc;
        }
        HostStage st(stream);
        if (dev) {
            bounds_launch(gran, callerPrec == RN_F64, b);
        } else {   // the same kernel behind a staging copy
            if (int rc = stage_open(st, a, 5)) return rc;
            stage_copy(st, a, 5, false);
            if (!st.ok()) return stage_close(st);
            const void *dv[5] = {a[0].dev, a[1].dev, a[2].dev, a[3].dev, a[4].dev};
            bounds_launch(gran, true, dv);
        }
        st.note(hipGetLastError());
        if (int rc = stage_close(st)) return rc;      // (a device form holds no buffer: no synchronisation)
        d_blo = d_bloG[gran]; d_bhi = d_bhiG[gran]; boundsGran = gran;
        return RN_OK;
    }
    int get_bounds_layout(int *gran, size_t *rows) override {
        RN_CHECK(gran && rows, RN_E_ARG, "rn_get_bounds_layout: null output");
        RN_CHECK(factored, RN_E_STATE, "rn_get_bounds_layout before rn_factor_step");
        *gran = boundsGran; *rows = bounds_rows(boundsGran);
        return RN_OK;
    }
    int get_bounds(size_t rows, double *const *out) override {
        RN_CHECK(factored, RN_E_STATE, "rn_get_bounds before rn_factor_step");
        RN_CHECK(out[0] || out[1] || out[2] || out[3] || out[4], RN_E_ARG, "rn_get_bounds: all five arrays are NULL");
        RN_CHECK(rows == bounds_rows(boundsGran), RN_E_ARG, "rn_get_bounds: rows must be what rn_get_bounds_layout reports");
        RN_HIP(hipSetDevice(device));
        const int nx = d.nx, nu = d.nu;
        std::vector<double> lo(rows * (size_t)ny), hi(rows * (size_t)ny);
        if (int rc = download(lo.data(), d_blo, lo.size())) return rc;
        if (int rc = download(hi.data(), d_bhi, hi.size())) return rc;
        bounds::unpack_tables(rows, nx, nu, lo.data(), hi.data(), out);
        return RN_OK;
    }
