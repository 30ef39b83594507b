// mg_spectra.h -- MGSolver: the Chebyshev windows of the levels.  Lanczos runs with full reorthogonalisation, one chain
// of small launches per level (captured into a hipGraph, replayed per design iteration, side by side on streams of
// their own) or one launch on one XCD; estimate_spectra() schedules them beside the coarsest level's factorisation.
// Included by mg.h after the declaration of MGSolver.
#pragma once

// Chebyshev windows of the stencil / coarse levels (and of the fine level if opt.fine_eig)
template <int DOF>
int MGSolver<DOF>::estimate_spectra(int first_level) {
    // One rank: the estimates of the levels are independent chains of small kernels -> one stream per level,
    // forked from and joined to the solver's stream (the device overlaps their launch-latency-bound steps).
    const bool serial = sw_lanczos_serial();
    // the coarsest level solved exactly needs no window: its factorisation takes the place of its Lanczos run
    const bool direct = coarse_direct_ok();
    const bool early = cd_early && direct;  // factorisation enqueued by the owner already (its event is recorded)
    cd_early = false;
    struct ReadyReset {  // the level events belong to this assembly only
        bool *f;
        ~ReadyReset() {
            for (int i = 0; i < LV_SLOTS; i++) f[i] = false;
        }
    } ready_reset{lv_ready_set};
    if (!early) cd.factored = false, cd_inverse_owed = false;
    if (!grid->has_comm && !serial && nlv - first_level >= 2) {
        hipStream_t main = grid->stream;
        if (!lan_fork) TP_HIP(hipEventCreateWithFlags(&lan_fork, hipEventDisableTiming));
        TP_HIP(hipEventRecord(lan_fork, main));
        int rc = TP_OK;
        const bool serial_host = sw_lanczos_one_thread();
        struct Replay {
            hipStream_t s;
            int l;
        };
        bool chain_on_main = false;
        std::vector<Replay> replay;
        // coarsest level first: with the exact coarse solve its chain (factorisation) is the longest one
        // (with the factorisation the other levels' chains share ONE stream: the device has four hardware queues, and
        // streams that share a queue run one after the other -- the factorisation must not be the one that waits)
        for (int l = nlv - 1; l >= first_level && rc == TP_OK; l--) {
            if (early && l == nlv - 1) continue;
            // stream of this level's chain: with the factorisation, level `first_level` on one stream, the levels
            // between it and the coarsest one on the owner's spare stream (or on the same one if there is none)
            hipStream_t ls;
            if (direct && l != nlv - 1) {
                // round 6: the levels beyond first_level + 1 run on the solver's own stream -- it has nothing else to do
                // until the chains are in (its queue was the idle fourth one), and two levels' chains one after the other on
                // the spare stream had become the longest path of the set-up once the chains lost their reduction launches
                const int on_main = sw_lanczos_on_main();
                if (l > first_level + 1 && side_stream && on_main == 1) {
                    ls = main;
                    chain_on_main = true;
                } else if (l > first_level + 1 && side_stream && on_main == 2) {
                    if (!lan_stream[l]) TP_HIP(hipStreamCreateWithFlags(&lan_stream[l], hipStreamNonBlocking));
                    ls = lan_stream[l];
                } else if (l != first_level && side_stream) {
                    ls = side_stream;
                } else {
                    if (!lan_stream[first_level]) TP_HIP(hipStreamCreateWithFlags(&lan_stream[first_level], hipStreamNonBlocking));
                    ls = lan_stream[first_level];
                }
            } else {
                if (!lan_stream[l]) TP_HIP(hipStreamCreateWithFlags(&lan_stream[l], hipStreamNonBlocking));
                ls = lan_stream[l];
            }
            if (!lan_done[l]) TP_HIP(hipEventCreateWithFlags(&lan_done[l], hipEventDisableTiming));
            TP_HIP(hipStreamWaitEvent(ls, (lv_ready_set[l] && l != nlv - 1) ? lv_ready[l] : lan_fork, 0));
            const int steps = (l == nlv - 1 && l > 0) ? NLANCZOS_COARSE : opt.nlanczos;
            // A captured chain is replayed from a helper thread (round 4): hipGraphLaunch of a ~100-node chain keeps
            // the calling thread for 0.6-1.3 ms (rocprofv3 --hip-trace), so three replays issued one after the other
            // made the LAST level's chain start 1-2 ms late whatever stream it was on -- the set-up was bound by
            // the host.  Chains that share a stream share a thread (order on the stream = order of the calls).
            if (!(direct && l == nlv - 1) && !serial_host && lanczos_graph_replayable(l)) {
                lan[l].m = steps;
                replay.push_back({ls, l});
                continue;
            }
            grid->stream = ls;  // everything the run launches goes to the level's stream
            rc = (direct && l == nlv - 1) ? coarse_direct_factor() : lanczos_graph(l, steps);
            grid->stream = main;
            if (rc == TP_OK && hipEventRecord(lan_done[l], ls) != hipSuccess) rc = TP_ERR_HIP;
        }
        if (!replay.empty()) {
            int dev = 0;
            (void)hipGetDevice(&dev);
            std::vector<hipStream_t> streams;
            for (const Replay &r : replay)
                if (std::find(streams.begin(), streams.end(), r.s) == streams.end()) streams.push_back(r.s);
            std::vector<int> trc(streams.size(), TP_OK);
            std::vector<std::thread> th;
            for (size_t q = 0; q < streams.size(); q++)
                th.emplace_back([&, q, dev]() {
                    if (hipSetDevice(dev) != hipSuccess) {
                        trc[q] = TP_ERR_HIP;
                        return;
                    }
                    for (const Replay &r : replay) {
                        if (r.s != streams[q]) continue;
                        if (hipGraphLaunch(lan_graph[r.l], r.s) != hipSuccess || hipEventRecord(lan_done[r.l], r.s) != hipSuccess) trc[q] = TP_ERR_HIP;
                    }
                });
            if (early) rc = enqueue_owed_inverse();  // (while the helper threads sit in hipGraphLaunch)
            for (std::thread &t : th) t.join();
            for (size_t q = 0; q < streams.size(); q++)
                if (trc[q] != TP_OK) {   // a failed replay: drop the graphs, enqueue the chains the plain way
                    (void)hipGetLastError();
                    for (const Replay &r : replay) {
                        if (r.s != streams[q]) continue;
                        lan_graph_state[r.l] = -1;
                        grid->stream = r.s;
                        const int rc2 = lanczos_enqueue(r.l, lan[r.l].m);
                        grid->stream = main;
                        if (rc2 == TP_OK && hipEventRecord(lan_done[r.l], r.s) != hipSuccess) rc = TP_ERR_HIP;
                        if (rc2) rc = rc2;
                    }
                }
        }
        if (early && rc == TP_OK) rc = enqueue_owed_inverse();  // (no replay this time: behind the directly enqueued chains)
        // Round 5: the factorisation is NOT joined here.  Nothing on the host depends on it (no Ritz values to read), and
        // the solve does not touch the factor before the first V-cycle reaches the coarsest level -- ~0.35 ms of
        // fine-level and level-1..3 work into the solve.  The solver's stream waits for the chain's event right before the
        // first triangular product (coarse_direct_apply); until then the factorisation (ONE workgroup column on one
        // XCD, 1.4 ms) runs beside the head of the solve.  TP_NO_DEFER_FACTOR=1: joined here, as in round 4.
        const bool no_defer = sw_no_defer_factor();
        const bool defer = direct && !no_defer && !tp_defer_disabled() && lan_done[nlv - 1] && rc == TP_OK;
        for (int l = first_level; l < nlv; l++)
            if (lan_done[l] && !(defer && l == nlv - 1)) (void)hipStreamWaitEvent(main, lan_done[l], 0);
        for (int l = first_level; l < nlv; l++)
            if (lan_stream[l] && !(defer && l == nlv - 1)) (void)hipStreamSynchronize(lan_stream[l]);
        if (side_stream) (void)hipStreamSynchronize(side_stream);
        if (chain_on_main) (void)hipStreamSynchronize(main);
        cd_pending = cd_deferred_last = defer;
        if (rc) return rc;
        for (int l = first_level; l < nlv; l++) {
            if (direct && l == nlv - 1)
                lv[l].lam = lv[l].lam_min = 1.0;  // (not used)
            else if (l == nlv - 1 && l > 0)
                lanczos_finish(l, &lv[l].lam, &lv[l].lam_min);
            else
                lanczos_finish(l, &lv[l].lam);
        }
        return TP_OK;
    }
    if (early) TP_TRY(enqueue_owed_inverse());
    for (int l = first_level; l < nlv; l++) {
        const bool rep = replicate && l >= rep0;   // the level's estimate comes from its replicated copy: same operator, same
        const int r = rep ? rix(l) : l;             // hashed start vector, no communication
        if (l == nlv - 1 && l > 0 && direct) {
            TP_TRY(coarse_direct_factor());
            lv[l].lam = lv[l].lam_min = 1.0;
            if (rep) lv[r].lam = lv[r].lam_min = 1.0;
        } else if (l == nlv - 1 && l > 0) {
            TP_TRY(lanczos(r, NLANCZOS_COARSE, &lv[r].lam, &lv[r].lam_min));
            lv[l].lam = lv[r].lam;
            lv[l].lam_min = lv[r].lam_min;
        } else {
            TP_TRY(lanczos(r, opt.nlanczos, &lv[r].lam));
            lv[l].lam = lv[r].lam;
        }
    }
    return TP_OK;
}

template <int DOF>
int MGSolver<DOF>::mark_level_ready(int l) {
    const bool off = sw_no_level_events();
    if (off || grid->has_comm || l < 0 || l >= LV_SLOTS) return TP_OK;
    if (!lv_ready[l]) TP_HIP(hipEventCreateWithFlags(&lv_ready[l], hipEventDisableTiming));
    TP_HIP(hipEventRecord(lv_ready[l], grid->stream));
    lv_ready_set[l] = true;
    return TP_OK;
}

// sum over ranks of n device doubles (chunks of the 16-double framework buffer)
template <int DOF>
int MGSolver<DOF>::allreduce_dev(double *p, int n, bool local_only) {
    if (!grid->has_comm || local_only) return TP_OK;
    for (int o = 0; o < n; o += 16) {
        const int c = n - o < 16 ? n - o : 16;
        TP_HIP(hipMemcpyAsync(grid->comm.red, p + o, sizeof(double) * c, hipMemcpyDeviceToDevice, grid->stream));
        {
            CommMark cm(grid, 2, grid->stream);
            if (grid->comm.allreduce_sum(grid->comm.user, c)) return TP_ERR_COMM;
        }
        TP_HIP(hipMemcpyAsync(p + o, grid->comm.red, sizeof(double) * c, hipMemcpyDeviceToDevice, grid->stream));
    }
    return TP_OK;
}

// Extreme Ritz values of `steps` Lanczos iterations on D^-1/2 A D^-1/2 with FULL
// reorthogonalisation (classical Gram-Schmidt twice): the estimates are then reproducible to
// ~1e-13 between implementations, which the residual-history parity needs.  All coefficients
// stay on the device; one host read at the end.
// Enqueues a Lanczos run for level l on grid->stream (everything stays on the device, coefficients are copied to
// the level's pinned host buffer at the end); lanczos_finish evaluates them once the stream has drained.
template <int DOF>
int MGSolver<DOF>::lanczos_enqueue(int l, int steps) {
    Level<DOF> &L = lv[l];
    LanBuf &B = lan[l];
    if (steps > 128) steps = 128;
    const long off = L.own_off(), n = L.own_n(), nd = L.ndof();
    // small levels: one workgroup per dot product writes its result directly (no second reduction stage)
    const int nb = n <= 65536 ? 1 : grid_for(n, 256);
    const int gn = (int)((L.g.owned_nodes() + BLK - 1) / BLK);
    hipStream_t s = grid->stream;
    const size_t need = (size_t)nd * (size_t)(steps + 1);
    if (need > B.cap) {
        B.cap = 0;
        // zeroed once: the chain reads and writes the owned range of every basis vector only
        TP_TRY(B.V.alloc_zero(need, s));
        B.cap = need;
    }
    if (!B.coef) TP_TRY(B.coef.alloc(520));
    if (!B.part) TP_TRY(B.part.alloc(256 * 130));
    if (!B.hc) TP_HIP(hipHostMalloc((void **)&B.hc, sizeof(double) * 520));
    // Round 6: the reductions of the chain end inside the kernels that produce them (TP_LANCZOS_TAILS=0: second launches, as
    // before) -- per step 3 launches of k_reduce_multi less, |w|^2 from the second Gram-Schmidt subtraction instead of a dot
    // product of its own, and on the level-1 operator the D^-1/2 scaling in its epilogue: 12 -> 6 dependent launches per step
    // on level 1, 10 -> 6 on the stencil levels, 7 -> 6 where one workgroup per vector does the dot products.
    const bool tails = sw_lanczos_tails();
    if (tails && !B.ticket) {
        TP_TRY(B.ticket.alloc_zero(TICKET_WORDS, s));
        TP_TRY(B.mticket.alloc_zero((size_t)MT_WORDS * 130, s));
    }
    double *V = B.V, *coef = B.coef, *part = B.part;
    unsigned *mt = tails ? B.mticket : nullptr, *tk = tails ? B.ticket : nullptr;
    auto multi_dot = [&](const double *A, int nv, const double *wv, double *out) -> int {
        TP_LAUNCH(k_multi_dot, dim3(nb, nv), dim3(BLK), 0, s, A, nd, nv, wv, off, n, nb == 1 ? out : part, nb == 1 ? nullptr : mt, out);
        if (nb > 1 && !mt) TP_LAUNCH(k_reduce_multi, dim3(nv), dim3(BLK), 0, s, part, nb, nv, out);
        return TP_OK;
    };
    // coef: h1[129] h2[129] alpha[128] beta[128] bb[1]
    double *h1 = coef, *h2 = coef + 129, *al = coef + 258, *be = coef + 386, *bb = coef + 514;
    double *w = L.d, *t = L.r, *dis = L.b;  // scratch that smooth() never swaps: stable addresses for the graph
    TP_LAUNCH((k_lanczos_init<DOF>), dim3(gn), dim3(BLK), 0, s, L.g, V, dis, L.dinv, coef, 520);
    TP_TRY(multi_dot(V, 1, V, bb));
    TP_TRY(allreduce_dev(bb, 1, L.no_comm));
    TP_LAUNCH(k_lanczos_next, dim3(grid_for(n)), dim3(BLK), 0, s, V, bb, 0, be, V, off, n, dis, t);  // normalise v0
    // w = D^-1/2 A D^-1/2 v_j: the first scaling is written by k_lanczos_next together with v_j, the second one
    // by the operator's epilogue where the level is a stored stencil or the level-1 pattern (NodeArgs::dinv of EPI_APPLY)
    const bool scaled_apply = L.kind == LV_DIA || (DOF == 3 && L.kind == LV_MACRO && tails);
    const int ga = grid_for(n);
    for (int j = 0; j < steps; j++) {
        if (scaled_apply) {
            TP_TRY(halo(l, t));
            NodeArgs a{};
            a.x = t;
            a.out = w;
            a.dinv = dis;
            TP_TRY(op<EPI_APPLY>(l, a));
        } else {
            TP_TRY(apply(l, t, w));
            TP_LAUNCH(k_pw_mult, dim3(grid_for(n)), dim3(BLK), 0, s, w + off, dis + off, w + off, n);
        }
        for (int pass = 0; pass < 2; pass++) {
            double *h = pass ? h2 : h1;
            TP_TRY(multi_dot(V, j + 1, w, h));
            TP_TRY(allreduce_dev(h, j + 1, L.no_comm));
            // the second pass also records alpha[j] = h1[j] + h2[j] -- and, with the tails, |w|^2 of what it leaves
            if (pass && tails)
                TP_LAUNCH(k_multi_axpy<true>, dim3(ga), dim3(BLK), 0, s, V, nd, j + 1, h, w, off, n, h1, al, part, tk, bb);
            else
                TP_LAUNCH(k_multi_axpy<false>, dim3(ga), dim3(BLK), 0, s, V, nd, j + 1, h, w, off, n,
                          pass ? h1 : nullptr, al, nullptr, nullptr, nullptr);
        }
        if (!tails) TP_TRY(multi_dot(w, 1, w, bb));
        TP_TRY(allreduce_dev(bb, 1, L.no_comm));
        TP_LAUNCH(k_lanczos_next, dim3(grid_for(n)), dim3(BLK), 0, s, w, bb, j, be, V + (size_t)(j + 1) * nd,
                           off, n, dis, t);
        grid->launches += tails ? 6 : ((nb == 1 ? 8 : 11) - (scaled_apply ? 1 : 0));
    }
    B.m = steps;
    TP_HIP(hipMemcpyAsync(B.hc, coef, sizeof(double) * 520, hipMemcpyDeviceToHost, s));
    return TP_OK;
}

// The coarsest level's run as ONE launch on one XCD (coarse_run.h: k_lanczos_run_xcd): where the Chebyshev run of the
// level qualifies for the one-XCD form; TP_NO_LANCZOS_XCD=1 keeps the chain of launches.
template <int DOF>
bool MGSolver<DOF>::lanczos_xcd_ok(int l, int steps) const {
    if (sw_no_lanczos_xcd() || tp_xcd_disabled() || steps > LAN_MAXS || steps < 2) return false;
    if (!(l == cd_level() && base(l) > 0)) return false;
    return xcd_eligible(l, LAN_XS, 4);  // (8 rows per thread: the basis no longer fits the LDS)
}

template <int DOF>
int MGSolver<DOF>::lanczos_xcd(int l, int steps) {
    Level<DOF> &L = lv[l];
    LanBuf &B = lan[l];
    hipStream_t s = grid->stream;
    if (!B.coef) TP_TRY(B.coef.alloc(520));
    if (!B.part) TP_TRY(B.part.alloc(256 * 130));
    if (!B.hc) TP_HIP(hipHostMalloc((void **)&B.hc, sizeof(double) * 520));
    if (!lan_ctl) {
        TP_TRY(lan_ctl.alloc_zero(1, s));
    }
    TP_HIP(hipMemsetAsync(B.coef, 0, sizeof(double) * 520, s));
    DiaOp<DOF> o{L.S, L.ndof(), L.g};
    int P;
    const int R = xcd_rows_per_thread(L.own_n(), &P);
    if (R == 1) TP_LAUNCH((k_lanczos_run_xcd<DOF, 1>), dim3(8 * P), dim3(RUN_WG), 0, s, o, L.dinv, B.part, B.coef + 258, B.coef + 386, steps, lan_ctl, P);
    else if (R == 2) TP_LAUNCH((k_lanczos_run_xcd<DOF, 2>), dim3(8 * P), dim3(RUN_WG), 0, s, o, L.dinv, B.part, B.coef + 258, B.coef + 386, steps, lan_ctl, P);
    else TP_LAUNCH((k_lanczos_run_xcd<DOF, 4>), dim3(8 * P), dim3(RUN_WG), 0, s, o, L.dinv, B.part, B.coef + 258, B.coef + 386, steps, lan_ctl, P);
    grid->launches += 1;
    B.m = steps;
    TP_HIP(hipMemcpyAsync(B.hc, B.coef, sizeof(double) * 520, hipMemcpyDeviceToHost, s));
    return TP_OK;
}

// is the captured chain of level l valid for the vectors it would run on now?
template <int DOF>
bool MGSolver<DOF>::lanczos_graph_replayable(int l) const {
    const Level<DOF> &L = lv[l];
    const void *key[5] = {L.r, L.b, L.d, L.corr, (const void *)(intptr_t)topology_epoch};
    return lan_graph_state[l] == 1 && memcmp(key, lan_graph_key[l], sizeof(key)) == 0 && !lanczos_xcd_ok(l, opt.nlanczos) &&
           !sw_no_graph() && !tp_debug_sync();
}

// replay (or capture, or plain enqueue) of the run of level l on grid->stream
template <int DOF>
int MGSolver<DOF>::lanczos_graph(int l, int steps) {
    static const bool no_graph = sw_no_graph() || tp_debug_sync();  // (latched here: the first run decides for the process)
    Level<DOF> &L = lv[l];
    hipStream_t s = grid->stream;
    if (lanczos_xcd_ok(l, steps)) return lanczos_xcd(l, steps);
    // the chain reads/writes these vectors by address, and set_bc may rebuild the correction lists
    const void *key[5] = {L.r, L.b, L.d, L.corr, (const void *)(intptr_t)topology_epoch};
    if (lan_graph_state[l] == 1 && memcmp(key, lan_graph_key[l], sizeof(key)) != 0) {
        (void)hipGraphExecDestroy(lan_graph[l]);
        lan_graph[l] = nullptr;
        lan_graph_state[l] = 0;
    }
    if (no_graph || lan_graph_state[l] < 0) return lanczos_enqueue(l, steps);
    if (lan_graph_state[l] == 1) {
        lan[l].m = steps;
        const long launches = grid->launches;
        (void)launches;
        if (hipGraphLaunch(lan_graph[l], s) == hipSuccess) return TP_OK;
        lan_graph_state[l] = -1;
        return lanczos_enqueue(l, steps);
    }
    // first use: allocate outside the capture (a warm-up run), then capture the identical chain
    int rc = lanczos_enqueue(l, steps);
    if (rc) return rc;
    // the legacy default stream cannot capture: the chain is recorded on the spare stream and replayed where it belongs
    hipStream_t cs = (s == nullptr && side_stream) ? side_stream : s;
    if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        lan_graph_state[l] = -1;
        return TP_OK;  // the warm-up run above already did the work
    }
    const long l0 = grid->launches;
    const double b0 = grid->alg_bytes, f0 = grid->flops;
    grid->stream = cs;
    rc = lanczos_enqueue(l, steps);
    grid->stream = s;
    grid->launches = l0;  // the captured chain was not executed
    grid->alg_bytes = b0;
    grid->flops = f0;
    hipGraph_t g = nullptr;
    const hipError_t e1 = hipStreamEndCapture(cs, &g);
    if (rc || e1 != hipSuccess || !g || hipGraphInstantiate(&lan_graph[l], g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        lan_graph[l] = nullptr;
        lan_graph_state[l] = -1;
        return rc;
    }
    (void)hipGraphDestroy(g);
    memcpy(lan_graph_key[l], key, sizeof(key));
    lan_graph_state[l] = 1;
    return TP_OK;
}

template <int DOF>
void MGSolver<DOF>::lanczos_finish(int l, double *lam_out, double *lam_min_out) {
    const LanBuf &B = lan[l];
    const double *ha = B.hc + 258, *hb = B.hc + 386;
    int m = B.m;
    for (int j = 0; j < m; j++)  // breakdown (invariant subspace): truncate like the CPU path
        if (!(hb[j] > 1e-14 * fabs(ha[j]))) {
            m = j + 1;
            break;
        }
    *lam_out = tridiag_lmax(m, ha, hb);
    if (lam_min_out) *lam_min_out = tridiag_lmin(m, ha, hb);
}

template <int DOF>
int MGSolver<DOF>::lanczos(int l, int steps, double *lam_out, double *lam_min_out) {
    if (lanczos_xcd_ok(l, steps)) TP_TRY(lanczos_xcd(l, steps));
    else TP_TRY(lanczos_enqueue(l, steps));
    TP_HIP(hipStreamSynchronize(grid->stream));
    lanczos_finish(l, lam_out, lam_min_out);
    return TP_OK;
}
