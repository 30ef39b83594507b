// conduction_api.h -- the tp_conduction handle: steady heat conduction on the grid, solved by MGSolver<1> with the fine
// level of conduction.h and true Galerkin stencil levels below it.  Included from topopt_amd.hip behind the elasticity
// entry points (k_simp, k_mul).  DESIGN.md 4.17.
#pragma once

struct tp_conduction {
    tp_grid *grid;
    MGSolver<1> mg;
    double KT[64], v8[8];
    DevBuf<double> d_KT, d_M;      // element matrix, 8 child matrices (level 0 -> 1, elements without clamped nodes)
    DevBuf<double> d_k;            // conductivities, own + ghost-above layer
    DevBuf<uint8_t> d_mask;        // clamped bit per local node
    DevBuf<unsigned> d_nbmask;     // mask bits of the 27 neighbours per local node
    DevBuf<double> d_N, d_bN;      // copy of N, RHS .* N scratch
    DevBuf<double> d_resp;         // block partials of tp_conduction_response, (TP_MAX_CASES + 1) x resp_nb
    long resp_nb;
    bool have_bc, assembled;
};

static ConductionOp cond_op(const tp_conduction *c) {
    ConductionOp o{c->d_k, c->d_nbmask, {}, c->mg.lv[0].g};
    for (int q = 0; q < 8; q++) o.v[q] = c->v8[q];
    return o;
}

extern "C" int tp_conduction_create(tp_conduction **out, tp_grid *g, const tp_solver_opts *o) {
    if (!out || !g || !o) return TP_ERR_ARG;
    TP_TRY(check_solver_opts(g, o, false, true));   // (the reference's FGMRES configuration belongs to the elasticity solver)
    std::unique_ptr<tp_conduction> c(new tp_conduction());
    c->grid = g;
    c->resp_nb = 0;
    c->have_bc = c->assembled = false;
    MGSolver<1> &mg = c->mg;
    mg.grid = g;
    mg.nlv = o->nlvls;
    mg.opt = *o;
    mg.allow_replicate = o->nlvls >= 3;   // every coarse level is a stored stencil; the slab rule above is elasticity's
    conduction_element_box(g->o.hx, g->o.hy, g->o.hz, c->KT, c->v8);
    double M[8 * 64];
    cond_child_matrices(c->KT, M);
    TP_TRY(mg.alloc_levels());
    Geom q = make_geom(g, 0);
    TP_TRY(c->d_KT.alloc(64));
    TP_TRY(c->d_M.alloc(8 * 64));
    TP_HIP(hipMemcpy(c->d_KT, c->KT, sizeof(c->KT), hipMemcpyHostToDevice));
    TP_HIP(hipMemcpy(c->d_M, M, sizeof(M), hipMemcpyHostToDevice));
    TP_TRY(c->d_k.alloc_zero((size_t)((long)q.ex * q.ey * (q.ez_own + 1))));
    TP_TRY(c->d_mask.alloc_zero((size_t)q.nodes()));
    TP_TRY(c->d_nbmask.alloc_zero((size_t)q.nodes()));
    TP_TRY(c->d_N.alloc((size_t)q.nodes()));
    TP_TRY(c->d_bN.alloc((size_t)q.nodes()));
    for (int l = 0; l < mg.nlv; l++) {
        Level<1> &L = mg.lv[l];
        L.kind = l == 0 ? LV_MATFREE : LV_DIA;
        if (l == 0) {
            L.KE = c->d_KT;
            L.E = c->d_k;
            L.mask = c->d_mask;
            L.nbmask = c->d_nbmask;
            for (int v = 0; v < 8; v++) L.kt8[v] = c->v8[v];
        } else {
            TP_TRY(mg.alloc_stencil(l, 27, false));
            TP_TRY(mg.store[l].Kel.alloc(64 * (size_t)L.g.elems_stored()));
            L.Kel = mg.store[l].Kel;
        }
    }
    *out = c.release();
    return TP_OK;
}
extern "C" int tp_conduction_destroy(tp_conduction *c) {
    if (!c) return TP_OK;
    (void)hipStreamSynchronize(c->grid->stream);
    delete c;
    return TP_OK;
}
extern "C" int tp_conduction_get_ke(const tp_conduction *c, double *kt_host_64) {
    if (!c || !kt_host_64) return TP_ERR_ARG;
    std::memcpy(kt_host_64, c->KT, sizeof(c->KT));
    return TP_OK;
}
extern "C" int tp_conduction_set_bc(tp_conduction *c, const double *N) {
    if (!c || !N) return TP_ERR_ARG;
    tp_grid *g = c->grid;
    c->mg.topology_epoch++;
    Geom q = c->mg.lv[0].g;
    const long nn = q.nodes();
    TP_LAUNCH(k_cond_nbmask, dim3(grid_for(nn)), dim3(BLK), 0, g->stream, q, N, c->d_mask, c->d_nbmask);
    TP_HIP(hipMemcpyAsync(c->d_N, N, sizeof(double) * (size_t)nn, hipMemcpyDeviceToDevice, g->stream));
    count_launch(g, 16.0 * nn, 0.0);
    c->have_bc = true;
    c->assembled = false;
    return TP_OK;
}

static bool cond_params_ok(double kmin, double kmax, double penal) {
    return std::isfinite(kmin) && std::isfinite(kmax) && std::isfinite(penal) && kmin > 0.0 && kmax > kmin && penal >= 1.0;
}

extern "C" int tp_conduction_assemble(tp_conduction *c, const double *xPhys, double kmin, double kmax, double penal) {
    if (!c || !xPhys || !cond_params_ok(kmin, kmax, penal)) return TP_ERR_ARG;
    if (!c->have_bc) return TP_ERR_STATE;
    tp_grid *g = c->grid;
    MGSolver<1> &mg = c->mg;
    hipStream_t s = g->stream;
    const Geom q0 = mg.lv[0].g;
    const long nel = q0.own_elems(), lay = (long)q0.ex * q0.ey;
    c->assembled = false;
    for (bool &b : mg.lv_ready_set) b = false;
    TP_LAUNCH(k_simp, dim3(grid_for(nel)), dim3(BLK), 0, s, xPhys, kmin, kmax, penal, c->d_k, nel);
    count_launch(g, 16.0 * nel, 3.0 * nel);
    // ghost layer above <- the upper neighbour's first own layer
    TP_TRY(exchange_segments(g, c->d_k, nullptr, nullptr, c->d_k + nel, lay, 1, lay));
    const ConductionOp op = cond_op(c);
    {   // fine level: Jacobi diagonal, Chebyshev bound from the element matrix (computed once)
        Level<1> &L = mg.lv[0];
        TP_LAUNCH(k_cond_diag, dim3((int)((q0.owned_nodes() + BLK - 1) / BLK)), dim3(BLK), 0, s, op, L.dinv);
        count_launch(g, 12.0 * q0.owned_nodes() + 8.0 * nel, 8.0 * q0.owned_nodes());
        if (!(mg.fine_bound > 0.0)) {
            const double lb = elem_lambda_bound(8, c->KT);
            mg.fine_bound = lb > 1.0 ? lb : 1.0;
        }
        L.lam = mg.fine_bound;
    }
    for (int l = 1; l < mg.nlv; l++) {
        Level<1> &F = mg.lv[l - 1], &C = mg.lv[l];
        const long nEc = C.g.own_elems();
        const unsigned nbk = (unsigned)((nEc + BLK / WAVE - 1) / (BLK / WAVE));
        if (l == 1) {
            TP_LAUNCH(k_cond_galerkin_fine, dim3(nbk), dim3(BLK), 0, s, F.g, C.g, c->d_k, c->d_mask, op, c->d_M, C.Kel);
            count_launch(g, 8.0 * nel + 8.0 * 64 * nEc, 2.0 * 8 * 64 * nEc);
        } else {
            TP_LAUNCH(k_cond_galerkin_coarse, dim3(nbk), dim3(BLK), 0, s, F.g, C.g, F.Kel, C.Kel);
            count_launch(g, 8.0 * 64 * 9.0 * nEc, 2.0 * 8 * 2 * 8 * 64 * nEc);
        }
        // coarse ghost element layer above <- the upper neighbour's first own layer (one contiguous block of 64 * clay doubles)
        const long clay = (long)C.g.ex * C.g.ey;
        TP_TRY(exchange_segments(g, C.Kel, nullptr, nullptr, C.Kel + 64 * clay * C.g.ez_own, clay, 64, clay));
        const int gn = (int)((C.g.owned_nodes() + BLK - 1) / BLK);
        TP_LAUNCH(k_cond_elem_to_dia, dim3(gn, 27), dim3(BLK), 0, s, C.g, C.Kel, C.S, C.dinv);
        count_launch(g, 8.0 * (64.0 * C.g.elems_stored() + 28.0 * C.g.owned_nodes()), 64.0 * C.g.owned_nodes());
    }
    mg.ready = true;
    int rc = mg.setup_replicated();
    if (rc == TP_OK) rc = mg.estimate_spectra(mg.opt.fine_eig ? 0 : 1);
    if (rc != TP_OK) {  // join what the failed set-up left running on the side streams
        mg.join_side_streams();
        (void)hipStreamSynchronize(s);
        return rc;
    }
    c->assembled = true;
    return TP_OK;
}

extern "C" int tp_conduction_apply(tp_conduction *c, const double *u, double *y) {
    if (!c || !u || !y) return TP_ERR_ARG;
    if (!c->assembled) return TP_ERR_STATE;
    return c->mg.apply(0, const_cast<double *>(u), y);
}

// the same product through the Krylov method's kernel form (EPI_APPLY_DOT: CG's A p with its fused p . A p); *dot = u . y over
// all ranks, NULL: not read back, the host does not wait
extern "C" int tp_conduction_apply_dot(tp_conduction *c, const double *u, double *y, double *dot) {
    if (!c || !u || !y) return TP_ERR_ARG;
    if (!c->assembled) return TP_ERR_STATE;
    TP_TRY(c->mg.apply_krylov(const_cast<double *>(u), y));
    return dot ? read_scal(c->grid, S_PW, 1, dot) : TP_OK;
}

extern "C" int tp_conduction_solve(tp_conduction *c, const double *RHS, double *T, int *its, double *rnorm, double *bnorm,
                                   double *hist, int hist_cap) {
    if (!c || !RHS || !T || hist_cap < 0 || (hist_cap > 0 && !hist)) return TP_ERR_ARG;
    if (!c->assembled) return TP_ERR_STATE;
    tp_grid *g = c->grid;
    const long n = c->mg.lv[0].ndof();
    TP_LAUNCH(k_mul, dim3(grid_for(n)), dim3(BLK), 0, g->stream, c->d_bN, RHS, c->d_N, n);   // RHS .* N, on a scratch copy
    count_launch(g, 24.0 * n, 1.0 * n);
    return c->mg.solve(c->d_bN, T, its, rnorm, bnorm, hist, hist_cap);
}

extern "C" int tp_conduction_set_tolerances(tp_conduction *c, double rtol, double atol, double dtol, int max_it) {
    if (!c) return TP_ERR_ARG;   // negative = keep
    if (rtol >= 0) c->mg.opt.rtol = rtol;
    if (atol >= 0) c->mg.opt.atol = atol;
    if (dtol >= 0) c->mg.opt.dtol = dtol;
    if (max_it >= 0) c->mg.opt.max_it = max_it;
    return TP_OK;
}

extern "C" int tp_conduction_response(tp_conduction *c, int ncase, const double *const *T, const double *const *V, const double *w,
                                      const double *xPhys, double kmin, double kmax, double penal, double volfrac, double *f_case,
                                      double *fx, double *gx, double *dfdx, double *dgdx) {
    if (!c || !T || !xPhys || ncase < 1 || ncase > TP_MAX_CASES || !cond_params_ok(kmin, kmax, penal) || !std::isfinite(volfrac))
        return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!T[l] || (w && !std::isfinite(w[l]))) return TP_ERR_ARG;
    if (!c->have_bc) return TP_ERR_STATE;
    tp_grid *g = c->grid;
    const Geom q = c->mg.lv[0].g;
    const long nel = q.own_elems();
    const long nel_glob = (long)g->ex * g->ey * g->ez_glob;
    CondRespArgs a{};
    a.ncase = ncase;
    const double *distinct[2 * TP_MAX_CASES];
    int ndistinct = 0;
    auto note = [&](const double *p) {
        for (int i = 0; i < ndistinct; i++)
            if (distinct[i] == p) return;
        distinct[ndistinct++] = p;
    };
    for (int l = 0; l < ncase; l++) {
        a.T[l] = T[l];
        a.V[l] = (V && V[l]) ? V[l] : T[l];
        a.w[l] = w ? w[l] : 1.0;
        note(a.T[l]);
        note(a.V[l]);
    }
    for (int i = 0; i < ndistinct; i++) TP_TRY(halo_nodes(g, q, const_cast<double *>(distinct[i]), 1));
    const int nb = (int)((nel + BLK - 1) / BLK);
    const ConductionOp op = cond_op(c);
    if (!fx && !gx && !f_case) {  // sensitivities only: no reduction, no host synchronisation
        if (dfdx) {
            TP_LAUNCH(k_cond_response<false>, dim3(nb), dim3(BLK), 0, g->stream, q, op, a, xPhys, kmin, kmax, penal, dfdx, (double *)nullptr);
            count_launch(g, 8.0 * q.owned_nodes() * ndistinct + 16.0 * nel, 2.0 * 72 * nel * ncase);
        }
    } else {
        if (c->resp_nb < nb) {
            TP_HIP(hipStreamSynchronize(g->stream));
            c->resp_nb = 0;
            TP_TRY(c->d_resp.alloc((TP_MAX_CASES + 1) * (size_t)nb));
            c->resp_nb = nb;
        }
        TP_LAUNCH(k_cond_response<true>, dim3(nb), dim3(BLK), 0, g->stream, q, op, a, xPhys, kmin, kmax, penal, dfdx, c->d_resp.p);
        count_launch(g, 8.0 * q.owned_nodes() * ndistinct + 16.0 * nel, 2.0 * 72 * nel * ncase);
        TP_TRY(reduce_partials_n(g, c->d_resp, nb, ncase + 1, S_TMP));
        double v[TP_MAX_CASES + 1];
        TP_TRY(read_scal(g, S_TMP, ncase + 1, v));
        double f = 0.0;
        for (int l = 0; l < ncase; l++) {
            if (f_case) f_case[l] = v[l];
            f = fma(a.w[l], v[l], f);
        }
        if (fx) *fx = f;
        if (gx) *gx = v[ncase] / (double)nel_glob - volfrac;
    }
    if (dgdx) TP_TRY(tp_vec_set(g, dgdx, 1.0 / (double)nel_glob, nel));
    return TP_OK;
}

// ---- level by level (tests): vectors [dev, the level's local nodes]; mg_levels.h
static LevelRef<1> levels(const tp_conduction *c) {
    if (!c) return {nullptr, TP_ERR_ARG};
    return {const_cast<MGSolver<1> *>(&c->mg), c->assembled ? TP_OK : TP_ERR_STATE};
}
extern "C" int tp_conduction_level_count(const tp_conduction *c) { return lv_count(levels(c)); }
extern "C" long tp_conduction_level_nodes(const tp_conduction *c, int l) { return lv_nodes(levels(c), l); }
extern "C" double tp_conduction_level_lambda(const tp_conduction *c, int l) { return lv_lambda(levels(c), l); }
extern "C" double tp_conduction_level_lambda_min(const tp_conduction *c, int l) { return lv_lambda_min(levels(c), l); }
extern "C" int tp_conduction_level_apply(tp_conduction *c, int l, const double *u, double *y) { return lv_apply(levels(c), l, u, y); }
extern "C" int tp_conduction_level_diag(tp_conduction *c, int l, double *d) { return lv_diag(levels(c), l, d); }
extern "C" int tp_conduction_smooth(tp_conduction *c, int l, const double *b, double *x, int k, int zero_guess) {
    return lv_smooth(levels(c), l, b, x, k, zero_guess);
}
extern "C" int tp_conduction_level_residual(tp_conduction *c, int l, const double *b, const double *x, double *r) {
    return lv_residual(levels(c), l, b, x, r);
}
extern "C" int tp_conduction_restrict(tp_conduction *c, int l, const double *rf, double *rc) { return lv_restrict(levels(c), l, rf, rc); }
extern "C" int tp_conduction_prolong_add(tp_conduction *c, int l, const double *xc, double *xf) { return lv_prolong_add(levels(c), l, xc, xf); }
extern "C" int tp_conduction_last_op_form(const tp_conduction *c, int *form4) { return lv_last_op_form(levels(c), form4); }
extern "C" int tp_conduction_last_stats(const tp_conduction *c, double *alg_bytes, double *flops, long *launches) {
    return lv_last_stats(levels(c), alg_bytes, flops, launches);
}
