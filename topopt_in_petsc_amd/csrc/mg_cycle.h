// mg_cycle.h -- MGSolver: the levels' storage, the Chebyshev-Jacobi smoother, the V-cycle (PCMG, multiplicative, zero
// initial guesses) with its replicated coarse levels, and the preconditioned CG around it.  Included by mg.h after the
// declaration of MGSolver.
#pragma once

template <int DOF>
int MGSolver<DOF>::alloc_levels() {
    for (int l = 0; l < nlv; l++) {
        Level<DOF> &L = lv[l];
        L.g = make_geom(grid, l);
        TP_TRY(alloc_vectors(l));
    }
    for (int i = nlv; i < LV_SLOTS; i++) lv[i] = Level<DOF>();  // (value-initialised: every pointer null)
    const bool no_rep = sw_no_replicate();
    replicate = allow_replicate && grid->has_comm && nlv > 1 && !no_rep;
    rep0 = nlv - 1;
    if (replicate) {
        // Which coarse levels are replicated?  Always the coarsest one; from the first stored-stencil level (>= 2) on whose
        // slab holds at most two element layers -- there a level's kernels are at their launch floor and every operator
        // application is followed by a halo exchange that costs more than the kernel --; TP_REPLICATE_FROM=l (2 .. nlv - 1)
        // fixes it, TP_REPLICATE_FROM=0 keeps the coarsest level only.
        const int from_env = sw_replicate_from();
        if (from_env >= 2 && from_env <= nlv - 1) {
            // a forced level must fit: one padded slab of it in the communicator's staging buffer (gather_owned), and its
            // replicated stencil (27 DOF^2 doubles per row, on EVERY rank) within 2 GiB -- else the next thinner level
            rep0 = from_env;
            while (rep0 < nlv - 1) {
                const Geom &c = lv[rep0].g;
                const long pad = (long)DOF * c.plane() * (c.ez_own + 1);
                const double rep_bytes = 8.0 * 27 * DOF * DOF * (double)c.plane() * c.nz_glob;
                if (pad <= grid->comm.cap && rep_bytes <= 2147483648.0) break;
                fprintf(stderr, "topopt_amd: TP_REPLICATE_FROM=%d: level %d does not fit (one slab of it: %ld doubles against a staging "
                                "buffer of %ld; replicated stencil %.2f GB per rank, limit 2): replicating from level %d\n",
                        from_env, rep0, pad, (long)grid->comm.cap, rep_bytes / 1e9, rep0 + 1);
                rep0++;
            }
        } else if (from_env < 0) {
            for (int l = 2; l < nlv - 1; l++)
                if (lv[l].g.ez_own <= 2) {
                    rep0 = l;
                    break;
                }
        }
        for (int l = rep0; l < nlv; l++) {
            Level<DOF> &R = lv[rix(l)];
            const Geom &c = lv[l].g;
            R.g = c;
            R.g.nzl = c.nz_glob;
            R.g.ez_own = R.g.ezl = c.nz_glob - 1;
            R.g.own_lo = 0;
            R.g.own_hi = c.nz_glob - 1;
            R.g.gz0 = 0;
            R.g.has_lo = R.g.has_hi = 0;
            R.kind = LV_DIA;
            R.no_comm = true;
            TP_TRY(alloc_vectors(rix(l)));
            TP_TRY(alloc_stencil(rix(l), 28 * DOF, true));   // (+ DOF slices: row-sum correction of the mirrored reads)
        }
    }
    for (DevBuf<double> *p : {&cg_r, &cg_p, &cg_w, &cg_p2}) TP_TRY(p->alloc_zero((size_t)lv[0].ndof(), grid->stream));
    return TP_OK;
}

template <int DOF>
int MGSolver<DOF>::alloc_vectors(int i) {
    Level<DOF> &L = lv[i];
    LevelStore &st = store[i];
    for (DevBuf<double> *p : {&st.b, &st.x, &st.x2, &st.r, &st.d, &st.dinv}) TP_TRY(p->alloc_zero((size_t)L.ndof(), grid->stream));
    L.b = st.b, L.x = st.x, L.x2 = st.x2, L.r = st.r, L.d = st.d, L.dinv = st.dinv;
    return TP_OK;
}
template <int DOF>
int MGSolver<DOF>::alloc_stencil(int i, int slices, bool on_stream) {
    const size_t n = (size_t)slices * (size_t)lv[i].ndof();
    TP_TRY(on_stream ? store[i].S.alloc_zero(n, grid->stream) : store[i].S.alloc_zero(n));
    lv[i].S = store[i].S;
    return TP_OK;
}
template <int DOF>
int MGSolver<DOF>::alloc_elem_matrices(int i) {
    TP_TRY(store[i].Kel.alloc(576 * (size_t)lv[i].g.elems_stored()));
    lv[i].Kel = store[i].Kel;
    return TP_OK;
}

template <int DOF>
void MGSolver<DOF>::free_levels() {
    smooth_graphs_free();
    refksp_free(*this);
    coarse_direct_free();
    for (LanBuf &b : lan) {
        (void)hipHostFree(b.hc);
        b.hc = nullptr;
    }
    for (int i = 0; i < LV_SLOTS; i++) {
        if (lan_graph[i]) (void)hipGraphExecDestroy(lan_graph[i]);
        lan_graph[i] = nullptr;
        lan_graph_state[i] = 0;
        if (lan_stream[i]) (void)hipStreamDestroy(lan_stream[i]);
        if (lan_done[i]) (void)hipEventDestroy(lan_done[i]);
        lan_stream[i] = nullptr;
        lan_done[i] = nullptr;
    }
    if (lan_fork) (void)hipEventDestroy(lan_fork);
    lan_fork = nullptr;
    for (int i = 0; i < LV_SLOTS; i++) {
        if (lv_ready[i]) (void)hipEventDestroy(lv_ready[i]);
        lv_ready[i] = nullptr;
        lv_ready_set[i] = false;
    }
    for (int i = 0; i < LV_SLOTS; i++) {
        if (pend_ev[i]) (void)hipEventDestroy(pend_ev[i]);
        pend_ev[i] = nullptr;
        pend[i].ptr = nullptr;
    }
}

// Jacobi diagonal + Chebyshev bound of a matrix-free level
template <int DOF>
int MGSolver<DOF>::setup_matfree_level(int l, const double *h_KE) {
    Level<DOF> &L = lv[l];
    MatfreeOp<DOF> o{L.KE, L.E, L.mask, L.g};
    TP_LAUNCH((k_matfree_diag<DOF>), dim3((int)((L.g.owned_nodes() + BLK - 1) / BLK)), dim3(BLK), 0,
                       grid->stream, o, L.dinv);
    count_launch(grid, 8.0 * DOF * L.g.owned_nodes() + 8.0 * L.g.own_elems(), 16.0 * DOF * L.g.owned_nodes());
    if (l == 0) {
        // the element matrix of a solver never changes: the bound (a 24 x 24 Jacobi eigenvalue iteration on the host,
        // ~90 us during which the device had nothing queued) is computed once
        if (!(fine_bound > 0.0)) {
            const double lb = elem_lambda_bound(8 * DOF, h_KE);
            fine_bound = lb > 1.0 ? lb : 1.0;
        }
        L.lam = fine_bound;
    }
    return TP_OK;
}

// every rank's owned rows of `nseg` consecutive level vectors (stride src_stride / dst_stride) -> the
// replicated global arrays.  Rank q owns global planes q*ez + (q>0) .. (q+1)*ez.
template <int DOF>
int MGSolver<DOF>::gather_owned(Level<DOF> &L, const double *src, Level<DOF> &R, double *dst, int nseg, long src_stride,
                                long dst_stride) {
    const tp_comm &c = grid->comm;
    const long pl = (long)DOF * L.g.plane();
    const long pad = pl * (L.g.ez_own + 1);  // rank 0 owns one plane more than the others
    const int per = (int)(c.cap / pad);
    if (per < 1) return TP_ERR_ARG;
    hipStream_t s = grid->stream;
    for (int s0 = 0; s0 < nseg; s0 += per) {
        const int ns = nseg - s0 < per ? nseg - s0 : per;
        for (int q = 0; q < ns; q++)
            TP_HIP(hipMemcpyAsync(c.send_lo + (long)q * pad, src + (long)(s0 + q) * src_stride + L.own_off(),
                                  sizeof(double) * (size_t)L.own_n(), hipMemcpyDeviceToDevice, s));
        {
            CommMark cm(grid, 3, s);
            if (c.allgather(c.user, (long)ns * pad)) return TP_ERR_COMM;
        }
        for (int rk = 0; rk < grid->nranks; rk++) {
            const long p0 = (long)rk * L.g.ez_own + (rk > 0 ? 1 : 0), np = L.g.ez_own + (rk == 0 ? 1 : 0);
            for (int q = 0; q < ns; q++)
                TP_HIP(hipMemcpyAsync(dst + (long)(s0 + q) * dst_stride + pl * p0,
                                      c.gather + (long)rk * ns * pad + (long)q * pad, sizeof(double) * (size_t)(pl * np),
                                      hipMemcpyDeviceToDevice, s));
        }
    }
    return TP_OK;
}

// (re)build the replicated coarsest level from the ranks' owned stencil rows
template <int DOF>
int MGSolver<DOF>::setup_replicated() {
    if (!replicate) return TP_OK;
    for (int l = rep0; l < nlv; l++) {
        Level<DOF> &L = lv[l], &R = lv[rix(l)];
        if (L.kind != LV_DIA) return TP_ERR_STATE;   // (only stored-stencil levels have rows to gather)
        TP_TRY(gather_owned(L, L.S, R, R.S, 27 * DOF, L.ndof(), R.ndof()));
        TP_TRY(gather_owned(L, L.dinv, R, R.dinv, 1));
        if constexpr (DOF == 3) {   // the replicated copy owns every row: its own correction of the mirrored reads
            TP_LAUNCH(k_dia_sym_fix, dim3((int)((R.g.owned_nodes() + BLK - 1) / BLK)), dim3(BLK), 0, grid->stream, R.g, R.S, (long)R.ndof());
            count_launch(grid);
        }
    }
    return TP_OK;
}

// Chebyshev(k)-Jacobi; the iterate ping-pongs between L.x and L.x2, on exit L.x holds it
// dot_slot >= 0: the LAST step also leaves b . x in scal[dot_slot] (this rank's part; fine tile kernel only)
template <int DOF>
int MGSolver<DOF>::smooth(int l, const double *b, int k, bool zero_guess, int dot_slot, bool first_done) {
    if (replicate && l == nlv - 1) {
        // coarsest level replicated on every rank: one all-gather of the right-hand side instead of a
        // halo exchange per Chebyshev step; the result comes back with its ghost planes filled
        // (the V-cycle itself enters the replicated levels in vcycle(); this branch serves direct calls on the slab's level)
        Level<DOF> &R = lv[rix(l)];
        TP_TRY(gather_owned(lv[l], b, R, R.b, 1));
        TP_TRY(smooth(rix(l), R.b, k, zero_guess));  // (first_done never holds here: vcycle does not fuse on this path)
        Level<DOF> &L = lv[l];
        TP_HIP(hipMemcpyAsync(L.x, R.x + (long)DOF * L.g.plane() * L.g.gz0, sizeof(double) * (size_t)L.ndof(),
                              hipMemcpyDeviceToDevice, grid->stream));
        return TP_OK;
    }
    Level<DOF> &L = lv[l];
    if (cd.factored && l == cd.level && dot_slot < 0) return coarse_direct_apply(l, b);
    double theta, delta;
    cheb_window(l, &theta, &delta);
    if (!sg_capturing && dot_slot < 0 && k >= 8 && L.kind == LV_DIA && (L.no_comm || !grid->has_comm) && sw_smooth_graph())
        return smooth_replay(l, b, k, zero_guess, first_done, theta, delta);
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    int it = 0;
    if (zero_guess && first_done) {
        it = 1;  // x = dinv b / theta is already there (written by the restriction that produced b)
    } else if (zero_guess) {
        const long pl = (long)DOF * L.g.plane();
        TP_TRY(planes_split(l, L.x, [&](int p0, int np) -> int {
            TP_LAUNCH(k_cheb_first, dim3(grid_for(pl * np)), dim3(BLK), 0, grid->stream, L.x,
                      three_term(L) ? nullptr : L.d, b, L.dinv, 1.0 / theta, pl * p0, pl * np);
            return TP_OK;
        }));
        count_launch(grid, 32.0 * L.own_n(), 2.0 * L.own_n());
        it = 1;
    }
    if (it >= 1 && dot_slot < 0) {
        const int mode = coarse_run_mode(l, k - it);
        if (mode) return coarse_run(l, b, it, k, sigma, delta, mode);
    }
    for (; it < k; it++) {
        NodeArgs a{};
        a.x = L.x;
        a.out = L.x2;
        a.b = b;
        a.d = L.d;
        a.dinv = L.dinv;
        a.prev_zero = (zero_guess && it == 1) ? 1 : 0;
        if (it == 0) {
            a.c1 = 0.0;
            a.c2 = 1.0 / theta;
        } else {
            const double rn = 1.0 / (2.0 * sigma - rho);
            a.c1 = rn * rho;
            a.c2 = 2.0 * rn / delta;
            rho = rn;
        }
        TP_TRY(halo(l, L.x));
        if (dot_slot >= 0 && it == k - 1) {
            a.partials = grid->partials;
            a.ticket = tail_ticket(grid);
            a.red_out = grid->scal + dot_slot;
            TP_TRY(op<EPI_CHEB_DOT>(l, a));
        } else {
            TP_TRY(op<EPI_CHEB>(l, a, true));
        }
        std::swap(L.x, L.x2);
    }
    return TP_OK;
}

// Chebyshev window of level l.  The coarsest level is a SOLVE (the reference runs a Krylov method there,
// LinearElasticity.cc:720-731): its window spans the whole spectrum
template <int DOF>
void MGSolver<DOF>::cheb_window(int l, double *theta, double *delta) const {
    const Level<DOF> &L = lv[l];
    const bool solve_level = coarsest(l) && base(l) > 0;
    const double lmin = solve_level ? L.lam_min : opt.cheb_lo * L.lam, lmax = opt.cheb_hi * L.lam;
    *theta = 0.5 * (lmax + lmin);
    *delta = 0.5 * (lmax - lmin);
}

// can the last post-smoothing step of a V-cycle return r . z ?  (fine tile kernel, at least one fused step)
template <int DOF>
bool MGSolver<DOF>::can_fuse_rz() const {
    const int fine_v = sw_fine_v();
    const bool off = sw_no_fuse_rz();
    return !off && (fine_v >= 2 || fine_v == 0) && nlv > 1 && three_term(lv[0]) && opt.nsmooth >= 1;
}

// the fine level's pre-smoothing of a V-cycle for the right-hand side `b`, enqueued AHEAD of the cycle: the Krylov
// loop issues it for the next iteration before it waits for this iteration's residual norm, so that the device
// has ~200 us of work while the host wakes up (vcycle(0, b) then starts behind it).  It writes multigrid scratch
// only; if the iteration turns out to be the last one, it was for nothing.
template <int DOF>
int MGSolver<DOF>::vcycle_head(const double *b) {
    head_for = nullptr;
    if (nlv < 2) return TP_OK;
    TP_TRY(smooth(0, b, opt.nsmooth, true, -1, fine_first_done));
    head_for = b;
    return TP_OK;
}

// PCMG multiplicative V-cycle with zero initial guesses; result in lv[l].x
// cycles[l]: how often level l + 1 is cycled per visit of level l (1 = V, 2 = W: PCMGSetCycleType /
// PCMGSetCycleTypeOnLevel).  As PCMGMCycle_Private does it: the coarser level's iterate is zeroed once, further cycles
// run on the same right-hand side from the iterate (zero_guess = false: the pre-smoother's non-zero-guess branch);
// one cycle only into the coarsest level.
template <int DOF>
int MGSolver<DOF>::vcycle(int l, const double *b, int dot_slot, bool first_done, bool zero_guess) {
    Level<DOF> &L = lv[l];
    if (coarsest(l)) return smooth(l, b, opt.ncoarse, zero_guess, -1, first_done);
    if (l == 0 && head_for == b) head_for = nullptr;  // pre-smoothed already (vcycle_head)
    else TP_TRY(smooth(l, b, opt.nsmooth, zero_guess, -1, first_done));
    {
        NodeArgs a{};
        a.x = L.x;
        a.out = L.r;
        a.b = b;
        TP_TRY(halo(l, L.x));
        TP_TRY(op<EPI_RESID>(l, a, true));
    }
    Level<DOF> &C = lv[l + 1];   // (slab levels and replicated slots alike: the next coarser level sits in the next slot)
    TP_TRY(halo(l, L.r));
    // from here down the levels are the replicated copies: restriction into the slab's part of the right-hand side, one
    // all-gather, the coarser levels on every rank without any exchange, the slab's window of the result back
    const bool enter_rep = replicate && !is_rep(l) && l + 1 == rep0;
    const int cyc = coarsest(l + 1) ? 1 : cycles[base(l)];
    // the restriction also takes the coarse level's first Chebyshev step from the zero guess (one launch less per
    // level and V-cycle); not when the coarse level is the replicated copy, whose right-hand side is gathered first
    const bool no_fuse_first = sw_no_fuse_first();
    const bool fuse_first = !no_fuse_first && !enter_rep && !(cd.factored && coarsest(l + 1)) &&
                            (coarsest(l + 1) ? opt.ncoarse : opt.nsmooth) >= 1;
    double th = 1.0, de = 1.0;
    if (fuse_first) cheb_window(l + 1, &th, &de);
    auto restrict_planes = [&](int p0, int np) -> int {
        const long cpl = C.g.plane();
        TP_LAUNCH((k_restrict<DOF>), dim3((int)((cpl * np + BLK - 1) / BLK)), dim3(BLK), 0, grid->stream, C.g, L.g, L.r, C.b,
                  fuse_first ? C.dinv : nullptr, fuse_first ? C.x : nullptr, fuse_first && !three_term(C) ? C.d : nullptr,
                  1.0 / th, cpl * (p0 - C.g.own_lo), cpl * np);
        return TP_OK;
    };
    if (fuse_first) TP_TRY(planes_split(l + 1, C.x, restrict_planes));  // the coarse level's first iterate is read with ghosts next
    else TP_TRY(restrict_planes(C.g.own_lo, C.g.own_hi - C.g.own_lo + 1));
    count_launch(grid, 8.0 * DOF * (L.g.owned_nodes() + C.g.owned_nodes()), 2.0 * 27 * DOF * C.g.owned_nodes());
    if (enter_rep) {
        const int r = rix(l + 1);
        Level<DOF> &R = lv[r];
        TP_TRY(gather_owned(C, C.b, R, R.b, 1));
        TP_TRY(vcycle(r, R.b, -1, false));
        for (int c = 1; c < cyc; c++) TP_TRY(vcycle(r, R.b, -1, false, false));
        TP_HIP(hipMemcpyAsync(C.x, R.x + (long)DOF * C.g.plane() * C.g.gz0, sizeof(double) * (size_t)C.ndof(),
                              hipMemcpyDeviceToDevice, grid->stream));   // (own planes and ghosts)
    } else {
        TP_TRY(vcycle(l + 1, C.b, -1, fuse_first));
        for (int c = 1; c < cyc; c++) TP_TRY(vcycle(l + 1, C.b, -1, false, false));
        TP_TRY(halo(l + 1, C.x));
    }
    TP_TRY(planes_split(l, L.x, [&](int p0, int np) -> int {
        const long fpl = L.g.plane();
        TP_LAUNCH((k_prolong_add<DOF>), dim3((int)((fpl * np + BLK - 1) / BLK)), dim3(BLK), 0, grid->stream, C.g, L.g, C.x,
                  L.x, fpl * (p0 - L.g.own_lo), fpl * np);
        return TP_OK;
    }));
    count_launch(grid, 8.0 * DOF * (2 * L.g.owned_nodes() + C.g.owned_nodes()), 2.0 * 8 * DOF * L.g.owned_nodes());
    return smooth(l, b, opt.nsmooth, false, l == 0 ? dot_slot : -1);
}

// z = M r : one V-cycle.  Returns the pointer holding z (lv[0].x).
template <int DOF>
int MGSolver<DOF>::precond(const double *r, double **z, int dot_slot) {
    if (opt.ksp_mode == 1) return refksp_precond(*this, r, z);
    TP_TRY(vcycle(0, r, dot_slot));
    TP_TRY(drain_halos());
    *z = lv[0].x;
    return TP_OK;
}

// KSPSolve, KSPCG with the unpreconditioned norm, reference norm ||b||
// (KSPConvergedDefault with a nonzero initial guess)
template <int DOF>
int MGSolver<DOF>::solve(const double *b, double *x, int *its_out, double *rnorm_out, double *bnorm_out, double *hist,
                         int hist_cap) {
    if (!ready) return TP_ERR_STATE;
    if (opt.ksp_mode == 1) return refksp_solve(*this, b, x, its_out, rnorm_out, bnorm_out, hist, hist_cap);
    Level<DOF> &L = lv[0];
    hipStream_t s = grid->stream;
    const long off = L.own_off(), n = L.own_n();
    const int nb = grid_for(n, 2048);  // one resident round of workgroups; the reduction tail wants few arrivals
    double *r = cg_r, *p = cg_p, *p_alt = cg_p2, *w = cg_w;
    {
        NodeArgs a{};
        a.x = x;
        a.out = r;
        a.b = b;
        TP_TRY(halo(0, x));
        if (SYMKE_KRYLOV && DOF == 3 && L.use_tile) {
            // the initial residual belongs to the Krylov method: its operator is the Krylov product (matfree_tile.h:
            // SYMKE_KRYLOV -- KE's action on the iterate's translation part included), not the V-cycle's residual kernel
            a.b = nullptr;
            a.partials = grid->partials;
            a.ticket = tail_ticket(grid);
            a.red_out = grid->scal + S_PW;   // (x0 . A x0: not used)
            TP_TRY(op<EPI_APPLY_DOT>(0, a));
            TP_TRY(finish_tail<1>(grid, last_nblocks, S_PW));
            TP_LAUNCH(k_axpby, dim3(grid_for(n)), dim3(BLK), 0, s, r + off, 1.0, b + off, -1.0, n);   // r = b - A x
            count_launch(grid, 24.0 * n, 1.0 * n);
        } else {
            TP_TRY(op<EPI_RESID>(0, a));
        }
    }
    TP_LAUNCH(k_dot2, dim3(nb), dim3(BLK), 0, s, b, b, r, r, off, n, grid->partials);
    count_launch(grid, 16.0 * n, 4.0 * n);
    TP_TRY(reduce_partials<2>(grid, nb, S_BB));
    double v2[2];
    // the first V-cycle's fine pre-smoothing goes out BEFORE the host waits for the two norms (as the loop does for every
    // later iteration): the device has work while the host wakes up; wasted only when the warm start is converged already
    const bool spec_head = !sw_no_spec_head();
    head_for = nullptr;
    fine_first_done = false;  // (a previous solve that returned through TP_TRY inside its loop may have left it set)
    // on slabs a wasted head also wastes its halo exchanges: not when max_it = 0 or the previous solve needed no iteration
    if (spec_head && opt.ksp_mode == 0 && nlv >= 2 && !sg_capturing && opt.max_it > 0 && !(grid->has_comm && last_solve_its == 0)) {
        TP_TRY(read_scal_begin(grid, S_BB, 2));
        TP_TRY(vcycle_head(r));
        TP_TRY(read_scal_end(grid, 2, v2));
    } else {
        TP_TRY(read_scal(grid, S_BB, 2, v2));
    }
    const double bnorm = sqrt(v2[0]);
    double rnorm = sqrt(v2[1]);
    const double ttol = fmax(opt.rtol * bnorm, opt.atol);
    if (bnorm_out) *bnorm_out = bnorm;
    if (hist && hist_cap > 0) hist[0] = rnorm;
    int its = 0, rc = TP_OK;
    int rz_cur = S_RZ0, rz_old = S_RZ1;
    const bool fuse_cg = !sw_no_cg_fuse();
    if (rnorm > ttol) {
        for (its = 1; its <= opt.max_it; its++) {
            double *z;
            if (can_fuse_rz()) {  // r . z comes out of the V-cycle's last smoothing step
                TP_TRY(precond(r, &z, rz_cur));
                TP_TRY(finish_tail<1>(grid, last_nblocks, rz_cur));
            } else {
                TP_TRY(precond(r, &z));
                TP_TRY(dot_to_slot(grid, r + off, z + off, n, rz_cur));
            }
            // one rank, second-generation fine kernel: p = z + beta p inside the product's launch (fine_tile.h: the staged
            // input is fma(beta, p_old, z), the owner of a node stores it to the other p buffer) -- one pass over p and z
            // and one launch less per iteration; same values, bit for bit
            const bool fuse_p = fuse_cg && !grid->has_comm && runs_fine_tile(L) && !sg_capturing;
            if (fuse_p) {
                NodeArgs a{};
                a.x = its == 1 ? z : p;   // (first iteration: p = z -- beta 0 on z itself, whatever the buffer holds)
                a.pz = z;
                a.pnew = p_alt;
                a.pscal = its == 1 ? nullptr : grid->scal;
                a.slot_new = rz_cur;
                a.slot_old = rz_old;
                a.out = w;
                a.partials = grid->partials;
                a.ticket = tail_ticket(grid);
                a.red_out = grid->scal + S_PW;
                TP_TRY(op<EPI_APPLY_DOT>(0, a));
                TP_TRY(finish_tail<1>(grid, last_nblocks, S_PW));
                std::swap(p, p_alt);
            } else {
                {
                    const long pl = (long)DOF * L.g.plane();
                    TP_TRY(planes_split(0, p, [&](int p0, int np) -> int {
                        TP_LAUNCH(k_cg_update_p, dim3(grid_for(pl * np)), dim3(BLK), 0, s, p, z, grid->scal, rz_cur, rz_old,
                                  its == 1 ? 1 : 0, pl * p0, pl * np);
                        return TP_OK;
                    }));
                }
                count_launch(grid, 24.0 * n, 2.0 * n);
                NodeArgs a{};
                a.x = p;
                a.out = w;
                a.partials = grid->partials;
                a.ticket = tail_ticket(grid);
                a.red_out = grid->scal + S_PW;
                TP_TRY(halo(0, p));
                TP_TRY(op<EPI_APPLY_DOT>(0, a));
                TP_TRY(finish_tail<1>(grid, last_nblocks, S_PW));
            }
            // one rank: ||r||^2 goes straight to pinned host memory from the reduction's last workgroup (no copy in
            // the stream), and the update also writes the first Chebyshev step of the next V-cycle (see the kernel)
            const bool direct_rr = fuse_cg && !grid->has_comm && tail_ticket(grid) && grid->h_scal_dev;
            const bool fuse_first = direct_rr && spec_head && its < opt.max_it && nlv >= 2 && opt.nsmooth >= 1 && three_term(L) &&
                                    !sg_capturing;
            double th0 = 1.0, de0 = 1.0;
            if (fuse_first) cheb_window(0, &th0, &de0);
            const bool cg_nt = sw_cg_nt();  // on (TP_CG_NT=0: plain loads / stores)
            if (cg_nt && n >= (1L << 22))   // (below ~32 MB a vector lives in the caches anyway: the hint costs 0.5 % at C1 / C2)
                TP_LAUNCH(k_cg_update_xr<true>, dim3(nb), dim3(BLK), 0, s, x, r, p, w, grid->scal, rz_cur, off, n,
                          grid->partials, tail_ticket(grid), grid->scal + S_RR, direct_rr ? grid->h_scal_dev : nullptr,
                          fuse_first ? L.x : nullptr, L.dinv, 1.0 / th0);
            else
                TP_LAUNCH(k_cg_update_xr<false>, dim3(nb), dim3(BLK), 0, s, x, r, p, w, grid->scal, rz_cur, off, n,
                          grid->partials, tail_ticket(grid), grid->scal + S_RR, direct_rr ? grid->h_scal_dev : nullptr,
                          fuse_first ? L.x : nullptr, L.dinv, 1.0 / th0);
            count_launch(grid, (fuse_first ? 64.0 : 48.0) * n, 6.0 * n);
            TP_TRY(finish_tail<1>(grid, nb, S_RR));
            double rr;
            if (direct_rr) {
                if (!grid->ev_scal) TP_HIP(hipEventCreateWithFlags(&grid->ev_scal, hipEventDisableTiming));
                TP_HIP(hipEventRecord(grid->ev_scal, s));
            } else {
                TP_TRY(read_scal_begin(grid, S_RR, 1));
            }
            fine_first_done = fuse_first;
            if (spec_head && its < opt.max_it) TP_TRY(vcycle_head(r));  // next iteration's first kernels, then wait
            fine_first_done = false;
            TP_TRY(read_scal_end(grid, 1, &rr));
            rnorm = sqrt(rr);
            if (hist && its < hist_cap) hist[its] = rnorm;
            if (rnorm <= ttol) break;
            if (!(rnorm <= opt.dtol * bnorm)) {  // also catches NaN
                rc = TP_ERR_DIVERGED;
                break;
            }
            if (its == opt.max_it) break;
            std::swap(rz_cur, rz_old);
        }
    }
    head_for = nullptr;
    TP_TRY(drain_halos());
    gaveup_seen = false;
    if (rc == TP_ERR_DIVERGED) gaveup_seen = xcd_gaveup();  // (before the control blocks are cleared below)
    if (rc == TP_ERR_DIVERGED && run_cnt) {
        // a multi-workgroup coarse run that gave up leaves its give-up flag set and fewer arrivals than run_base
        // assumes: every later run would time out as well.  Start the counters over.
        TP_HIP(hipMemsetAsync(run_cnt, 0, 2 * sizeof(unsigned long long), s));
        run_base = 0;
    }
    if (rc == TP_ERR_DIVERGED && run_ctl) TP_HIP(hipMemsetAsync(run_ctl, 0, sizeof(XcdRunCtrl), s));
    if (rc == TP_ERR_DIVERGED && lan_ctl) TP_HIP(hipMemsetAsync(lan_ctl, 0, sizeof(XcdRunCtrl), s));
    if (rc == TP_ERR_DIVERGED && cd.ctl) TP_HIP(hipMemsetAsync(cd.ctl, 0, sizeof(XcdRunCtrl), s));
    if (its_out) *its_out = its;
    if (rnorm_out) *rnorm_out = rnorm;
    last_solve_its = its;
    return rc;
}
