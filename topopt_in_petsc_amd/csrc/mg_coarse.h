// mg_coarse.h -- MGSolver: the coarsest level.  Its exact solve (coarse_direct.h: factorisation beside the set-up,
// two triangular products per visit), its Chebyshev run in one launch (coarse_run.h), the give-up bookkeeping of the
// one-XCD kernels, and the opt-in replayed smoothing run.  Included by mg.h after the declaration of MGSolver.
#pragma once

// ---- the long smoothing run of the coarsest level (30 steps of 4-5 us kernels) as a hipGraph: captured when its
// arguments change -- the Chebyshev window once per design iteration, the x/x2 roles alternate between consecutive
// V-cycles (odd number of steps) -- and replayed for the other V-cycles of the solve.  Launches per design
// iteration at 128^3: 1660 -> 1016.  Time: 30.93 against 30.82 ms (three runs each, +-0.05): the two captures and
// instantiations per design iteration cost what the saved host launches bring -- outside a profiler the host
// keeps up with these kernels, the device does not wait for it.  Hence opt-in (TP_SMOOTH_GRAPH=1), kept as the
// evidence for that statement.
// (switches.h: sw_smooth_graph)
template <int DOF>
void MGSolver<DOF>::smooth_graphs_free() {
    for (SmoothGraph &g : sgraph) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        g = SmoothGraph();
    }
    if (sg_stream) (void)hipStreamDestroy(sg_stream);
    sg_stream = nullptr;
}

template <int DOF>
int MGSolver<DOF>::smooth_replay(int l, const double *b, int k, bool zero_guess, bool first_done, double theta, double delta) {
    Level<DOF> &L = lv[l];
    hipStream_t s = grid->stream;
    const int flags = (zero_guess ? 1 : 0) | (first_done ? 2 : 0);
    SmoothGraph *hit = nullptr, *victim = &sgraph[0];
    for (SmoothGraph &g : sgraph) {
        if (g.exec && g.level == l && g.ptr[0] == b && g.ptr[1] == L.x && g.ptr[2] == L.x2 && g.ptr[3] == L.d && g.theta == theta &&
            g.delta == delta && g.k == k && g.flags == flags)
            hit = &g;
        if (g.stamp < victim->stamp) victim = &g;
    }
    if (sw_debug_graph()) fprintf(stderr, "smooth graph: level %d %s\n", l, hit ? "hit" : "miss");
    if (hit && hipGraphLaunch(hit->exec, s) == hipSuccess) {
        hit->stamp = ++sg_clock;
        if (hit->swap) std::swap(L.x, L.x2);
        grid->launches += 1;
        grid->alg_bytes += hit->bytes;
        grid->flops += hit->flops;
        return TP_OK;
    }
    if (hit) {  // a replay that failed: drop the graph, run the launches
        (void)hipGetLastError();
        (void)hipGraphExecDestroy(hit->exec);
        *hit = SmoothGraph();
    }
    // first use of this argument set: run it directly now, capture the identical run for the next time
    double *const xa = L.x, *const xb = L.x2;  // roles before the run
    sg_capturing = true;
    int rc = smooth(l, b, k, zero_guess, -1, first_done);
    if (rc) {
        sg_capturing = false;
        return rc;
    }
    const bool swapped = L.x != xa;
    if (victim->exec) (void)hipGraphExecDestroy(victim->exec);
    *victim = SmoothGraph();
    // captured on a stream of our own (the grid's stream may be the legacy default stream, which cannot capture);
    // the graph is replayed on the grid's stream
    if (!sg_stream && hipStreamCreateWithFlags(&sg_stream, hipStreamNonBlocking) != hipSuccess) sg_stream = nullptr;
    if (!sg_stream || hipStreamBeginCapture(sg_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        sg_capturing = false;
        return TP_OK;
    }
    const long l0 = grid->launches;
    const double b0 = grid->alg_bytes, f0 = grid->flops;
    L.x = xa;  // the captured run starts from the same roles and leaves them like the direct run did
    L.x2 = xb;
    grid->stream = sg_stream;
    rc = smooth(l, b, k, zero_guess, -1, first_done);
    grid->stream = s;
    hipGraph_t g = nullptr;
    const hipError_t e1 = hipStreamEndCapture(sg_stream, &g);
    SmoothGraph ng;
    ng.bytes = grid->alg_bytes - b0;
    ng.flops = grid->flops - f0;
    grid->launches = l0;  // the captured chain was not executed
    grid->alg_bytes = b0;
    grid->flops = f0;
    sg_capturing = false;
    L.x = swapped ? xb : xa;
    L.x2 = swapped ? xa : xb;
    if (rc || e1 != hipSuccess || !g || hipGraphInstantiate(&ng.exec, g, nullptr, nullptr, 0) != hipSuccess) {
        if (sw_debug_graph()) fprintf(stderr, "smooth graph: capture failed rc=%d e1=%d g=%p\n", rc, (int)e1, (void *)g);
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        return TP_OK;  // the direct run above did the work
    }
    if (sw_debug_graph()) fprintf(stderr, "smooth graph: captured level %d k %d swap %d\n", l, k, (int)swapped);
    (void)hipGraphDestroy(g);
    ng.ptr[0] = b;
    ng.ptr[1] = xa;
    ng.ptr[2] = xb;
    ng.ptr[3] = L.d;
    ng.theta = theta;
    ng.delta = delta;
    ng.k = k;
    ng.flags = flags;
    ng.level = l;
    ng.swap = swapped;
    ng.stamp = ++sg_clock;
    *victim = ng;
    return TP_OK;
}

// ---- the coarsest level solved exactly (coarse_direct.h): opt.coarse_direct, one rank or the replicated copy
template <int DOF>
int MGSolver<DOF>::enqueue_owed_inverse() {
    if (!cd_inverse_owed) return TP_OK;
    cd_inverse_owed = false;
    const int l = nlv - 1;
    hipStream_t main = grid->stream;
    grid->stream = lan_stream[l];
    const int rc = coarse_direct_factor(2);
    grid->stream = main;
    if (rc) return rc;
    TP_HIP(hipEventRecord(lan_done[l], lan_stream[l]));
    return TP_OK;
}

// Called by the owner as soon as the coarsest level's stencil is enqueued (before the other levels are finished): the
// factorisation goes to the coarsest level's stream right away.  One rank only (the replicated copy of a multi-rank
// run is built later, setup_replicated); estimate_spectra then leaves the level alone.
template <int DOF>
int MGSolver<DOF>::coarse_direct_early(bool *started) {
    *started = false;
    const bool serial = sw_lanczos_serial();
    if (grid->has_comm || serial || opt.ksp_mode != 0 || nlv < 3 || !coarse_direct_ok()) return TP_OK;
    const int l = nlv - 1;
    hipStream_t main = grid->stream;
    if (!lan_fork) TP_HIP(hipEventCreateWithFlags(&lan_fork, hipEventDisableTiming));
    if (!lan_stream[l]) TP_HIP(hipStreamCreateWithFlags(&lan_stream[l], hipStreamNonBlocking));
    if (!lan_done[l]) TP_HIP(hipEventCreateWithFlags(&lan_done[l], hipEventDisableTiming));
    TP_HIP(hipEventRecord(lan_fork, main));
    TP_HIP(hipStreamWaitEvent(lan_stream[l], lan_fork, 0));
    // Only the fill and the factorisation itself now: the inverse's 17 launches follow from estimate_spectra, once the
    // rest of the assembly and the spectra chains are enqueued -- they are not needed for 1.4 ms, and enqueueing them here
    // kept the solver's stream idle for their host time in the middle of the assembly (round 6).
    const bool split_enq = sw_cd_split_enqueue();
    grid->stream = lan_stream[l];
    const int rc = coarse_direct_factor(split_enq ? 1 : 3);
    grid->stream = main;
    if (rc) return rc;
    cd_inverse_owed = split_enq;
    if (!split_enq) TP_HIP(hipEventRecord(lan_done[l], lan_stream[l]));
    cd_early = true;
    *started = true;
    return TP_OK;
}

template <int DOF>
bool MGSolver<DOF>::coarse_direct_ok() const {
    if (!opt.coarse_direct || sw_no_coarse_direct() || tp_xcd_disabled() || nlv < 2 || DOF != 3) return false;
    const Level<DOF> &L = lv[cd_level()];
    if (L.kind != LV_DIA || (grid->has_comm && !L.no_comm) || L.own_n() != L.ndof() || L.ndof() > CD_MAXROWS) return false;
    const long hb = (long)DOF * (L.g.plane() + L.g.nx + 1) + DOF - 1;
    const int KB = (int)((hb + CD_NB - 1) / CD_NB);
    if (!(KB >= 1 && KB <= CD_KBMAX && L.ndof() >= 4 * CD_NB)) return false;
    // a level of <= 448 rows runs its Chebyshev steps inside ONE workgroup at 0.4 us each (coarse_run.h): a
    // factorisation per assembly does not pay there -- coarse_direct = 2 asks for it anyway
    return opt.coarse_direct >= 2 || L.ndof() > (long)RUN_RPB * 8;
}

template <int DOF>
void MGSolver<DOF>::coarse_direct_free() {
    if (cd_pending && lan_stream[nlv - 1]) (void)hipStreamSynchronize(lan_stream[nlv - 1]);
    cd_pending = false;
    cd.factored = false;
    cd.level = -1;
}

// factor + invert on grid->stream (the caller puts it on a stream of its own beside the spectra chains)
// parts: 1 = band fill + factorisation, 2 = the triangular inverse behind it, 3 = both
template <int DOF>
int MGSolver<DOF>::coarse_direct_factor(int parts) {
    const int l = cd_level();
    Level<DOF> &L = lv[l];
    hipStream_t s = grid->stream;
    CdGeom g;
    g.n = (int)L.ndof();
    g.np = (g.n + CD_NB - 1) / CD_NB * CD_NB;
    g.nblk = g.np / CD_NB;
    g.KB = (int)(((long)DOF * (L.g.plane() + L.g.nx + 1) + DOF - 1 + CD_NB - 1) / CD_NB);
    if (cd.level != l || cd.g.np != g.np || cd.g.KB != g.KB) {
        coarse_direct_free();
        TP_TRY(cd.Lb.alloc((size_t)g.nblk * (g.KB + 1) * CD_NB * CD_NB));
        TP_TRY(cd.Ld.alloc((size_t)g.nblk * CD_NB * CD_NB));
        TP_TRY(cd.Linv.alloc((size_t)g.nblk * CD_NB * CD_NB));
        TP_TRY(cd.W.alloc((size_t)g.np * g.np));
        TP_TRY(cd.Tm.alloc((size_t)g.np * g.np));
        TP_TRY(cd.Wt.alloc((size_t)g.np * g.np));
        TP_TRY(cd.y.alloc((size_t)g.np));
        TP_TRY(cd.ctl.alloc_zero(1, s));
        cd.level = l;
    }
    cd.g = g;
    const int P = g.KB + 1;
    if (parts & 1) {
    TP_HIP(hipMemsetAsync(cd.Lb, 0, sizeof(double) * (size_t)g.nblk * (g.KB + 1) * CD_NB * CD_NB, s));
    DiaOp<DOF> o{L.S, L.ndof(), L.g};
    TP_LAUNCH((k_cd_fill<DOF>), dim3((g.np + CD_T - 1) / CD_T), dim3(CD_T), 0, s, o, g, cd.Lb);
    const int stages = sw_cd_stages();  // (timing aid: 1 fill, 2 + factor, 3 all)
    const bool prof_on = sw_cd_prof();  // (timing aid: ticks per phase, printed per factorisation)
    DevBuf<long long> prof;
    if (prof_on) TP_TRY(prof.alloc_zero(8 * 32, s));
    if (stages >= 2) TP_LAUNCH(k_cd_factor, dim3(8 * P), dim3(CD_T), 0, s, g, cd.Lb, cd.Ld, cd.ctl, P, prof);
    if (prof_on) {
        long long h[8 * 32];
        TP_HIP(hipStreamSynchronize(s));
        TP_HIP(hipMemcpy(h, prof, sizeof(h), hipMemcpyDeviceToHost));
        prof.reset();
        int rate = 100000;
        (void)hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, 0);
        for (int r = 0; r < P; r += (P > 4 ? P / 3 : 1))
            fprintf(stderr, "cd factor rank %2d us: A %.0f | B diag %.0f | B look-ahead %.0f | barrier1 %.0f | C %.0f | barrier2 %.0f | loop %.0f\n", r,
                    h[r * 8 + 0] * 1e3 / rate, h[r * 8 + 1] * 1e3 / rate, h[r * 8 + 2] * 1e3 / rate, h[r * 8 + 3] * 1e3 / rate, h[r * 8 + 4] * 1e3 / rate,
                    h[r * 8 + 5] * 1e3 / rate, h[r * 8 + 7] * 1e3 / rate);
    }
    }
    if (!(parts & 2)) return TP_OK;
    if (sw_cd_stages() >= 3) {
        TP_LAUNCH(k_cd_diag_inv, dim3(g.nblk), dim3(WAVE), 0, s, cd.Ld, cd.Linv);
        const bool dc = !sw_cd_invert_columns();  // (1: round 3's block-column substitution)
        if (dc) {
            TP_LAUNCH(k_cd_dc_diag, dim3(g.nblk), dim3(CD_T), 0, s, g, cd.Linv, cd.W, cd.Wt);
            for (int lv = 1; (1 << (lv - 1)) < g.nblk; lv++) {
                const int half = 1 << (lv - 1), nseg = (g.nblk + 2 * half - 1) / (2 * half);
                TP_LAUNCH(k_cd_dc_t, dim3(half, std::min(g.KB, half), nseg), dim3(WAVE), 0, s, g, lv, cd.Lb, cd.W, cd.Tm);
                TP_LAUNCH(k_cd_dc_w, dim3(half, half, nseg), dim3(WAVE), 0, s, g, lv, cd.Tm, cd.W, cd.Wt);
                grid->launches += 2;
            }
        } else {
            TP_LAUNCH(k_cd_invert, dim3(g.nblk), dim3(CD_T), 0, s, g, cd.Lb, cd.Linv, cd.W, cd.Wt);
        }
    }
    grid->launches += 4;
    const double nb2 = (double)g.np * g.np;
    grid->alg_bytes += 8.0 * (27.0 * DOF * DOF * L.g.nodes() + nb2);  // stencil in, W and W^T (lower halves) out
    grid->flops += (double)g.np * g.KB * CD_NB * (g.KB * CD_NB + g.np);  // band Cholesky + triangular inverse
    cd.factored = true;
    return TP_OK;
}

// the factorisation enqueued by this assembly is still running on its side stream: the solver's stream waits for it
// (device-side; the host does not block)
template <int DOF>
int MGSolver<DOF>::join_pending_factor() {
    if (cd_pending) {
        cd_pending = false;
        TP_HIP(hipStreamWaitEvent(grid->stream, lan_done[nlv - 1], 0));
    }
    return TP_OK;
}

// x = A^-1 b on level cd.level
template <int DOF>
int MGSolver<DOF>::coarse_direct_apply(int l, const double *b) {
    Level<DOF> &L = lv[l];
    TP_TRY(join_pending_factor());
    const int rows_per = CD_T / WAVE, nb = (cd.g.n + rows_per - 1) / rows_per;
    TP_LAUNCH(k_cd_tri<false>, dim3(nb), dim3(CD_T), 0, grid->stream, cd.g, cd.W, b, cd.y);
    TP_LAUNCH(k_cd_tri<true>, dim3(nb), dim3(CD_T), 0, grid->stream, cd.g, cd.Wt, cd.y, L.x);
    grid->launches += 2;
    grid->alg_bytes += 8.0 * ((double)cd.g.n * cd.g.n + 4.0 * cd.g.n);
    grid->flops += 2.0 * (double)cd.g.n * cd.g.n;
    return TP_OK;
}

// ---- the coarsest level's run in one launch (coarse_run.h)
// did a one-XCD kernel (Chebyshev run, Lanczos run, factorisation) give up?  Blocking read of the sticky flags.
template <int DOF>
bool MGSolver<DOF>::xcd_gaveup() {
    (void)join_pending_factor();
    unsigned long long f[3] = {0ull, 0ull, 0ull};
    XcdRunCtrl *blocks[3] = {run_ctl, lan_ctl, cd.ctl};
    for (int q = 0; q < 3; q++)
        if (blocks[q]) (void)hipMemcpyAsync(&f[q], &blocks[q]->gaveup[0], sizeof(unsigned long long), hipMemcpyDeviceToHost, grid->stream);
    (void)hipStreamSynchronize(grid->stream);
    gaveup_mask = (f[0] ? 1 : 0) | (f[1] ? 2 : 0) | (f[2] ? 4 : 0);
    return gaveup_mask != 0;
}

template <int DOF>
void MGSolver<DOF>::xcd_reset_controls() {
    for (XcdRunCtrl *b : {run_ctl.p, lan_ctl.p, cd.ctl.p})
        if (b) (void)hipMemsetAsync(b, 0, sizeof(XcdRunCtrl), grid->stream);
    cd_early = cd_inverse_owed = false;
    cd.factored = false;
}

// after an assembly that failed half way: no chain of a side stream may still be running when the next one starts
template <int DOF>
void MGSolver<DOF>::join_side_streams() {
    for (int i = 0; i < LV_SLOTS; i++)
        if (lan_stream[i]) (void)hipStreamSynchronize(lan_stream[i]);
    if (side_stream) (void)hipStreamSynchronize(side_stream);
    cd_early = cd_inverse_owed = false;
    cd_pending = false;
}

// rows per thread: the fewest that bring the run down to `want` workgroups (barrier cost grows with their number)
template <int DOF>
int MGSolver<DOF>::run_rows_per_thread(long rows, int *wgs) {
    const int want = sw_run_wgs();
    int R = 1;
    while (R < 8 && (rows + (long)RUN_RPB * R - 1) / ((long)RUN_RPB * R) > want) R *= 2;
    *wgs = (int)((rows + (long)RUN_RPB * R - 1) / ((long)RUN_RPB * R));
    return R;
}

template <int DOF>
int MGSolver<DOF>::xcd_rows_per_thread(long rows, int *wgs) {  // as few rows per thread as 32 workgroups allow
    int R = 1;
    while (R < 8 && (rows + (long)RUN_RPB * R - 1) / ((long)RUN_RPB * R) > 32) R *= 2;
    *wgs = (int)((rows + (long)RUN_RPB * R - 1) / ((long)RUN_RPB * R));
    return R;
}

// 3: one launch whose workgroups all sit on ONE XCD and exchange the iterate through its L2 (coarse_run.h; on for
//    449 .. 14336 rows held by one rank unless TP_NO_COARSE_XCD / TP_NO_COARSE_RUN: 2.3 us per step against 3-4 per launch)
// 0: separate launches; 1: one launch of ONE workgroup (iterate in LDS; on unless TP_NO_COARSE_RUN);
// 2: one launch of several workgroups with a barrier per step (opt-in TP_COARSE_RUN=1: measured at 128^3 / C1 / C3 it
// costs what its launches cost, 19.7 against 19.6 ms at 654 against 1471 launches per design iteration -- a step inside
// the kernel is 2.6-3.2 us (tools/probe/step_probe.hip), a dependent launch 3.1 us: the XCDs' L2 slices are not coherent,
// either way the iterate makes a round trip through the memory side; and a spinning kernel is a liability on a shared
// device)
template <int DOF>
int MGSolver<DOF>::coarse_run_mode(int l, int nsteps) const {
    const Level<DOF> &L = lv[l];
    if (sg_capturing || DOF != 3 || L.kind != LV_DIA || !coarsest(l)) return 0;
    if (!(L.no_comm || !grid->has_comm) || nsteps < 4 || nsteps > RUN_MAXK) return 0;
    int wgs;
    const int R = run_rows_per_thread(L.own_n(), &wgs);
    if (L.own_n() <= (long)RUN_RPB * 8 && L.ndof() <= RUN_XS && L.own_n() == L.ndof()) return sw_no_coarse_run() ? 0 : 1;
    if (sw_coarse_run()) return wgs <= RUN_MAX_WGS && run_stage_doubles(L.g, DOF, R) <= RUN_XS ? 2 : 0;
    // 3: the run on one XCD (coarse_run.h): one rank, at most 32 workgroups (one per CU of an XCD), R <= 2
    if (sw_no_coarse_run() || sw_no_coarse_xcd() || tp_xcd_disabled()) return 0;
    return xcd_eligible(l, RUN_XS, 8) ? 3 : 0;
}

// the level fits a run on one XCD: all its rows on this rank (one rank, or the replicated copy of the coarsest
// level), 2 .. 32 workgroups (one per CU of an XCD) of at most max_r rows per thread
template <int DOF>
bool MGSolver<DOF>::xcd_eligible(int l, long stage_cap, int max_r) const {
    const Level<DOF> &L = lv[l];
    if (sg_capturing || DOF != 3 || L.kind != LV_DIA || (grid->has_comm && !L.no_comm) || tp_debug_sync()) return false;
    int wx;
    const int Rx = xcd_rows_per_thread(L.own_n(), &wx);
    return Rx <= max_r && wx <= 32 && wx >= 2 && run_stage_doubles(L.g, DOF, Rx) <= stage_cap && L.own_n() == L.ndof();
}

// steps it0 .. k-1 of smooth() (it0 >= 1: the direction vector L.d is valid)
template <int DOF>
int MGSolver<DOF>::coarse_run(int l, const double *b, int it0, int k, double sigma, double delta, int mode) {
    Level<DOF> &L = lv[l];
    if (!run_cnt) {
        TP_TRY(run_cnt.alloc_zero(2));
    }
    ChebRunCoef cr;
    cr.nsteps = k - it0;
    double rho = 1.0 / sigma;
    for (int s = 0; s < cr.nsteps; s++) {
        const double rn = 1.0 / (2.0 * sigma - rho);
        cr.c1[s] = rn * rho;
        cr.c2[s] = 2.0 * rn / delta;
        rho = rn;
    }
    DiaOp<DOF> o{L.S, L.ndof(), L.g};
    if (mode == 1) {
        TP_LAUNCH((k_dia_cheb_run<DOF, 8, true>), dim3(1), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_cnt, run_base);
    } else if (mode == 3) {
        if (!run_ctl) {
            TP_TRY(run_ctl.alloc_zero(1, grid->stream));
        }
        int P;
        const int R = xcd_rows_per_thread(L.own_n(), &P);
        if (R == 1) TP_LAUNCH((k_dia_cheb_run_xcd<DOF, 1>), dim3(8 * P), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_ctl, P);
        else if (R == 2) TP_LAUNCH((k_dia_cheb_run_xcd<DOF, 2>), dim3(8 * P), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_ctl, P);
        else if (R == 4) TP_LAUNCH((k_dia_cheb_run_xcd<DOF, 4>), dim3(8 * P), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_ctl, P);
        else TP_LAUNCH((k_dia_cheb_run_xcd<DOF, 8>), dim3(8 * P), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_ctl, P);
        if (cr.nsteps & 1) std::swap(L.x, L.x2);
    } else {
        int wgs;
        const int R = run_rows_per_thread(L.own_n(), &wgs);
        if (R == 1) TP_LAUNCH((k_dia_cheb_run<DOF, 1, false>), dim3(wgs), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_cnt, run_base);
        else if (R == 2) TP_LAUNCH((k_dia_cheb_run<DOF, 2, false>), dim3(wgs), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_cnt, run_base);
        else if (R == 4) TP_LAUNCH((k_dia_cheb_run<DOF, 4, false>), dim3(wgs), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_cnt, run_base);
        else TP_LAUNCH((k_dia_cheb_run<DOF, 8, false>), dim3(wgs), dim3(RUN_WG), 0, grid->stream, o, b, L.dinv, L.d, L.x, L.x2, cr, run_cnt, run_base);
        run_base += (unsigned long long)(cr.nsteps - 1) * wgs;  // no barrier after the last step
        if (cr.nsteps & 1) std::swap(L.x, L.x2);
    }
    coarse_runs++;
    const long nown = L.g.owned_nodes();
    count_launch(grid, cr.nsteps * (27.0 * DOF * DOF + 6.0 * DOF) * 8.0 * nown, cr.nsteps * 2.0 * 27 * DOF * DOF * (double)nown);
    return TP_OK;
}
