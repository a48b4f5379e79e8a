// shift_warm_start.inc -- members of rn::Ctx<T> that move the duals of the last solve one stage toward the root of the scenario tree (included
// inside the struct body of rapidnet_capi.hip, behind plan_bands.inc whose full-tree arrays it shares).  Entry points served (include/rapidnet.h):
//   rn_shift_warm_start   y, y+ := the shifted y+ (k_shift_duals, k_dual.hpp)
//   rn_set_shift_map      a caller's node correspondence in place of the built-in rule
//   rn_get_shift_map      the correspondence in force
// The reference has no counterpart (it has no warm start at all).  The built-in correspondence is host code of its own (shift_map.hpp).  The
// gather is out of place without scratch: it reads y+ and writes y, which the warm start overwrites anyway, and y+ := y is one copy on the
// stream.  A context that never calls these holds nothing for them and launches nothing.

    // [nodes] each: the row every local node inherits (of y+, or on a shard of the whole tree's table; -1: from zero) and that row's stage;
    // shards: [full nodes][ny + 1].  Allocated by the first shift and kept.
    int *d_shiftSrc = nullptr, *d_shiftStage = nullptr;
    double *d_shiftTable = nullptr;
    std::vector<int> shiftUserMap;               // rn_set_shift_map: [full nodes]; empty: the built-in rule
    std::vector<int> h_shiftSrc, h_shiftStage;   // what the device arrays hold
    int shiftKey = -2;                           // the rootChild the device arrays were built for; -3: the caller's map; -2: nothing yet
    int shift_nodes() const { return bands_nodes(); }
    const int *shift_parent() const { return bands_sharded() ? fullParent.data() : h_parent.data(); }
    int shift_root_children() const { return shift::root_children(shift_parent(), shift_nodes()); }
    int shift_check_sharded(const std::string &fn) {
        if (bands_sharded())
            RN_CHECK(lib_sharded() && has_comm() && (int)fullCum.size() == d.N + 1 && (int)fullParent.size() == fullNodes, RN_E_STATE,
                     fn + ": a sharded context must come from rn_create_sharded and hold a communicator");
        return RN_OK;
    }
    int shift_buffers() {
        if (d_shiftSrc) return RN_OK;
        if (bands_sharded()) { if (int rc = dalloc(&d_shiftTable, (size_t)fullNodes * (ny + 1))) return rc; }
        if (int rc = dalloc(&d_shiftStage, (size_t)d.nodes)) return rc;
        return dalloc(&d_shiftSrc, (size_t)d.nodes);      // last: the sign that all of them exist
    }
    ShiftArgs shift_args() const {
        ShiftArgs a{};
        a.f64 = sizeof(T) == 8 ? 1 : 0;
        a.nodes = d.nodes; a.ny = ny;
        a.yp = p_upd; a.out = p_xi; a.dy = d_dy; a.prob = d_prob; a.prob64 = d_prob64; a.stageOf = d_stageOf;
        a.srcRow = d_shiftSrc; a.srcStage = d_shiftStage;
        return a;
    }
    unsigned shift_blocks(long long work) const { return (unsigned)std::max<long long>(1, std::min<long long>((long long)numCUs * 8, (work + ELT_THREADS - 1) / ELT_THREADS)); }
    // shards: the table zeroed, this rank's rows of y+ and its probabilities packed into it (rank 0 the crown's as well), summed over the
    // ranks -- exact, one rank at most holds a nonzero value at each entry -- so that every rank goes on with the same bits of the whole tree
    int shift_table() {
        const size_t cnt = (size_t)fullNodes * (ny + 1);
        RN_HIP(hipMemsetAsync(d_shiftTable, 0, cnt * sizeof(double), stream));
        ShiftArgs a = shift_args();
        a.phase = 1; a.table = d_shiftTable; a.gmap = d_gmap; a.crownNodes = h_stageCum[cutStage]; a.writeCrown = (rank == 0);
        hipLaunchKernelGGL(k_shift_duals<>, dim3(shift_blocks((long long)d.nodes * (ny + 1))), dim3(ELT_THREADS), 0, stream, a);
        RN_HIP(hipGetLastError());
        return all_reduce(d_shiftTable, cnt, true, "ncclAllReduce(shifted warm start, rows)");
    }
    // rootChild = -1: the root's child with the largest probability in force, ties to the lowest index.  The one form that waits for the
    // stream: the few values are read back (one GPU: only after a device-form rn_set_tree_data; a shard: from the summed table)
    int shift_most_probable(bool tableReady, int *child) {
        const int nc = shift_root_children();
        *child = 0;
        if (nc <= 1) return RN_OK;
        std::vector<double> p((size_t)nc);
        if (bands_sharded()) {
            if (!tableReady) { if (int rc = shift_table()) return rc; }
            std::vector<double> rows((size_t)nc * (ny + 1));      // the root's children are nodes 1 .. nc of the whole tree
            RN_HIP(hipMemcpyAsync(rows.data(), d_shiftTable + (size_t)(ny + 1), rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
            RN_HIP(hipStreamSynchronize(stream));
            for (int r = 0; r < nc; r++) p[r] = rows[(size_t)r * (ny + 1) + ny];
        } else {
            if (int rc = refresh_h_prob()) return rc;
            for (int r = 0; r < nc; r++) p[r] = h_prob[h_childStart[0] + r];
        }
        *child = shift::most_probable(p.data(), nc);
        return RN_OK;
    }
    // the whole tree's correspondence in force: the caller's, or the built-in one of `child`
    void shift_full_map(int child, std::vector<int> &map) const {
        if (!shiftUserMap.empty()) { map = shiftUserMap; return; }
        map.resize((size_t)shift_nodes());
        shift::build_map(shift_parent(), shift_nodes(), child, map.data());
    }
    // the device arrays follow the correspondence in force; nothing moves while it stays what they were built for
    int shift_upload(int child) {
        const int key = shiftUserMap.empty() ? child : -3;
        if (key == shiftKey) return RN_OK;
        std::vector<int> map, stage((size_t)shift_nodes());
        shift_full_map(child, map);
        shift::stages_of(bands_cum().data(), d.N, stage.data());
        h_shiftSrc.resize((size_t)d.nodes); h_shiftStage.resize((size_t)d.nodes);
        for (int i = 0; i < d.nodes; i++) {
            const int m = map[bands_sharded() ? globalNode[i] : i];
            h_shiftSrc[i] = m; h_shiftStage[i] = m >= 0 ? stage[m] : 0;
        }
        RN_HIP(hipMemcpyAsync(d_shiftSrc, h_shiftSrc.data(), (size_t)d.nodes * sizeof(int), hipMemcpyHostToDevice, stream));
        RN_HIP(hipMemcpyAsync(d_shiftStage, h_shiftStage.data(), (size_t)d.nodes * sizeof(int), hipMemcpyHostToDevice, stream));
        shiftKey = key;
        return RN_OK;
    }
    int shift_child_ok(const std::string &fn, int rootChild) {
        const int nc = shift_root_children();
        RN_CHECK(rootChild >= -1 && rootChild < std::max(nc, 1), RN_E_ARG, fn + ": rootChild must be -1 or a child number of the root (it has " + std::to_string(nc) + ")");
        return RN_OK;
    }
    int shift_warm_start(int rootChild) override {
        const std::string fn = "rn_shift_warm_start";
        if (int rc = shift_check_sharded(fn)) return rc;
        RN_CHECK(algorithm == RN_ALG_APG, RN_E_STATE, fn + ": global FBE and NAMA keep an L-BFGS memory that belongs to the unshifted duals; the shift is APG's");
        RN_CHECK(!poisoned, RN_E_STATE, fn + ": an earlier batch failed half-way; call rn_apg_reset first");
        RN_CHECK(factored && h_it > 0, RN_E_STATE, fn + " before a first solve: there are no duals to shift");
        if (shiftUserMap.empty()) { if (int rc = shift_child_ok(fn, rootChild)) return rc; }
        RN_HIP(hipSetDevice(device));
        if (int rc = shift_buffers()) return rc;
        const bool sharded = bands_sharded();
        if (sharded) { if (int rc = shift_table()) return rc; }
        int child = rootChild;
        if (shiftUserMap.empty() && rootChild < 0) { if (int rc = shift_most_probable(true, &child)) return rc; }
        if (int rc = shift_upload(child)) return rc;
        ShiftArgs a = shift_args();
        a.phase = 0; a.table = sharded ? d_shiftTable : nullptr;
        hipLaunchKernelGGL(k_shift_duals<>, dim3(shift_blocks(ntot())), dim3(ELT_THREADS), 0, stream, a);
        RN_HIP(hipGetLastError());
        RN_HIP(hipMemcpyAsync(p_upd, p_xi, (size_t)ntot() * sizeof(T), hipMemcpyDeviceToDevice, stream));   // y+ := y
        acc_ready = false;   // as apg_restart_keep_duals leaves it: the next iteration re-derives w from (y, y+)
        return RN_OK;
    }
    int set_shift_map(size_t nodes, const int *map) override {
        const std::string fn = "rn_set_shift_map";
        if (!map) { shiftUserMap.clear(); shiftKey = -2; return RN_OK; }
        RN_CHECK(!bands_sharded() || (lib_sharded() && (int)fullParent.size() == fullNodes), RN_E_STATE, fn + ": a sharded context must come from rn_create_sharded");
        RN_CHECK(nodes == (size_t)shift_nodes(), RN_E_ARG, fn + ": nodes must be the node count of the whole tree");
        RN_CHECK(shift::map_ok(map, nodes), RN_E_ARG, fn + ": an entry is neither a node of the tree nor -1");
        shiftUserMap.assign(map, map + nodes);
        shiftKey = -2;
        return RN_OK;
    }
    int get_shift_map(int rootChild, size_t nodes, int *map) override {
        const std::string fn = "rn_get_shift_map";
        RN_CHECK(map, RN_E_ARG, fn + ": null output");
        RN_CHECK(!bands_sharded() || (lib_sharded() && (int)fullParent.size() == fullNodes), RN_E_STATE, fn + ": a sharded context must come from rn_create_sharded");
        RN_CHECK(nodes == (size_t)shift_nodes(), RN_E_ARG, fn + ": nodes must be the node count of the whole tree");
        int child = rootChild;
        if (shiftUserMap.empty()) {
            if (int rc = shift_child_ok(fn, rootChild)) return rc;
            if (rootChild < 0) {
                RN_CHECK(!bands_sharded(), RN_E_ARG, fn + ": on a shard name the child (the most probable one is found by rn_shift_warm_start's collective)");
                RN_HIP(hipSetDevice(device));
                if (int rc = shift_most_probable(false, &child)) return rc;
            }
        }
        std::vector<int> m;
        shift_full_map(child, m);
        std::copy(m.begin(), m.end(), map);
        return RN_OK;
    }
