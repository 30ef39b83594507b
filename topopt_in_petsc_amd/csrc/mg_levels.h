// mg_levels.h -- what every owner of an MGSolver<DOF> shares outside the solve: the check of tp_solver_opts against the grid at
// creation, and the hierarchy level by level (tests, tools, bench.py) behind tp_elasticity_* / tp_conduction_* / tp_pdefilter_*.
// Included after mg.h.  The argument rules live here, once, in the order include/topopt_amd.h states them; a handle supplies a
// LevelRef and nothing else.  Every rule answers before anything is launched.  DESIGN.md 3.
#pragma once

// tp_solver_opts against the grid: 1 .. TP_MAX_LEVELS levels, every direction divisible by 2^(nlvls-1) (TopOpt.cc:183-201; here
// also per slab), ksp_mode 0 or -- where the owner has it, and on one device only -- 1, and on slabs (slab_rule) at least two
// element layers per rank on every level that stays distributed: the boundary-first halo overlap and the level-1 ghost rows
// assume a rank's two boundary planes are distinct; the replicated coarsest level (three or more levels) may come down to one.
// Decided from global sizes: the same answer on every rank.
static int check_solver_opts(const tp_grid *g, const tp_solver_opts *o, bool allow_ksp1, bool slab_rule) {
    if (o->nlvls < 1 || o->nlvls > TP_MAX_LEVELS) return TP_ERR_ARG;
    const int f = 1 << (o->nlvls - 1);
    if (g->ex % f || g->ey % f || g->ez_own % f) return TP_ERR_ARG;
    if (o->ksp_mode != 0 && !(allow_ksp1 && o->ksp_mode == 1)) return TP_ERR_ARG;
    if (o->ksp_mode == 1 && g->has_comm) {
        fprintf(stderr, "topopt_amd: ksp_mode 1 (the reference's FGMRES / GMRES / SOR configuration) runs on one device only\n");
        return TP_ERR_ARG;
    }
    if (slab_rule && g->has_comm) {
        const int last_distributed = o->nlvls >= 3 ? o->nlvls - 2 : o->nlvls - 1;
        if ((g->ez_own >> last_distributed) < 2) {
            fprintf(stderr, "topopt_amd: %d element layers per rank are too few for %d multigrid levels on slabs (need >= %d)\n",
                    g->ez_own, o->nlvls, 2 << last_distributed);
            return TP_ERR_ARG;
        }
    }
    return TP_OK;
}

// A handle as the level calls see it.  mg: its solver, NULL where there is none to ask (a NULL handle, a filter that is not of
// type 2): TP_ERR_ARG.  state: what the calls that need an assembled operator answer, TP_OK once there is one.
template <int DOF>
struct LevelRef {
    MGSolver<DOF> *mg;
    int state;
};

// The guard of every call on level l: handle and arguments, then the state, then the level.  The transfers go between l and
// l + 1 and touch no operator: both levels must exist, no assembly is asked for.
template <int DOF>
static int lv_guard(LevelRef<DOF> r, bool args_ok, int l, bool transfer = false) {
    if (!r.mg || !args_ok) return TP_ERR_ARG;
    if (!transfer && r.state != TP_OK) return r.state;
    return l >= 0 && l + (transfer ? 1 : 0) < r.mg->nlv ? TP_OK : TP_ERR_ARG;
}
template <int DOF>
static bool lv_has(LevelRef<DOF> r, int l) { return r.mg && l >= 0 && l < r.mg->nlv; }

template <int DOF>
static int lv_count(LevelRef<DOF> r) { return r.mg ? r.mg->nlv : -TP_ERR_ARG; }
template <int DOF>
static long lv_nodes(LevelRef<DOF> r, int l) { return lv_has(r, l) ? r.mg->lv[l].g.nodes() : -(long)TP_ERR_ARG; }
template <int DOF>
static double lv_lambda(LevelRef<DOF> r, int l) { return lv_has(r, l) ? r.mg->lv[l].lam : NAN; }
template <int DOF>
static double lv_lambda_min(LevelRef<DOF> r, int l) { return lv_has(r, l) ? r.mg->lv[l].lam_min : NAN; }

template <int DOF>
static int lv_apply(LevelRef<DOF> r, int l, const double *u, double *y) {
    TP_TRY(lv_guard(r, u && y, l));
    return r.mg->apply(l, const_cast<double *>(u), y);
}
// the reciprocal Jacobi diagonal
template <int DOF>
static int lv_diag(LevelRef<DOF> r, int l, double *d) {
    TP_TRY(lv_guard(r, d != nullptr, l));
    Level<DOF> &L = r.mg->lv[l];
    TP_HIP(hipMemcpyAsync(d, L.dinv, sizeof(double) * (size_t)L.ndof(), hipMemcpyDeviceToDevice, r.mg->grid->stream));
    return TP_OK;
}
// k Chebyshev-Jacobi steps on x (k == 0: the two copies alone, what bench.py subtracts)
template <int DOF>
static int lv_smooth(LevelRef<DOF> r, int l, const double *b, double *x, int k, int zero_guess) {
    TP_TRY(lv_guard(r, b && x && k >= 0, l));
    MGSolver<DOF> &mg = *r.mg;
    Level<DOF> &L = mg.lv[l];
    const size_t nb = sizeof(double) * (size_t)L.ndof();
    if (!zero_guess) TP_HIP(hipMemcpyAsync(L.x, x, nb, hipMemcpyDeviceToDevice, mg.grid->stream));
    TP_TRY(mg.smooth(l, b, k, zero_guess != 0));
    TP_TRY(mg.drain_halos());
    TP_HIP(hipMemcpyAsync(x, L.x, nb, hipMemcpyDeviceToDevice, mg.grid->stream));
    return TP_OK;
}
// r = b - A_l x through the residual epilogue of the level's kernel, as the V-cycle forms it (ghost planes of x refreshed first)
template <int DOF>
static int lv_residual(LevelRef<DOF> r, int l, const double *b, const double *x, double *res) {
    TP_TRY(lv_guard(r, b && x && res, l));
    MGSolver<DOF> &mg = *r.mg;
    TP_TRY(mg.halo(l, const_cast<double *>(x)));
    NodeArgs a{};
    a.x = x;
    a.out = res;
    a.b = b;
    TP_TRY(mg.template op<EPI_RESID>(l, a));
    return mg.drain_halos();
}
template <int DOF>
static int lv_restrict(LevelRef<DOF> r, int l, const double *rf, double *rc) {
    TP_TRY(lv_guard(r, rf && rc, l, true));
    MGSolver<DOF> &mg = *r.mg;
    TP_TRY(mg.halo(l, const_cast<double *>(rf)));
    const Geom &C = mg.lv[l + 1].g;
    TP_LAUNCH((k_restrict<DOF>), dim3((int)((C.owned_nodes() + BLK - 1) / BLK)), dim3(BLK), 0, mg.grid->stream, C, mg.lv[l].g, rf, rc);
    return TP_OK;
}
template <int DOF>
static int lv_prolong_add(LevelRef<DOF> r, int l, const double *xc, double *xf) {
    TP_TRY(lv_guard(r, xc && xf, l, true));
    MGSolver<DOF> &mg = *r.mg;
    TP_TRY(mg.halo(l + 1, const_cast<double *>(xc)));
    TP_LAUNCH((k_prolong_add<DOF>), dim3((int)((mg.lv[l].g.owned_nodes() + BLK - 1) / BLK)), dim3(BLK), 0, mg.grid->stream,
              mg.lv[l + 1].g, mg.lv[l].g, xc, xf);
    return TP_OK;
}
template <int DOF>
static int lv_last_op_form(LevelRef<DOF> r, int *form4) {
    if (!r.mg || !form4) return TP_ERR_ARG;
    for (int i = 0; i < 4; i++) form4[i] = r.mg->last_form[i];
    return TP_OK;
}
// bytes moved / flops / launches since the last call, by the algorithmic model of DESIGN.md; the counters start again
template <int DOF>
static int lv_last_stats(LevelRef<DOF> r, double *alg_bytes, double *flops, long *launches) {
    if (!r.mg || !r.mg->grid) return TP_ERR_ARG;
    tp_grid *g = r.mg->grid;
    if (alg_bytes) *alg_bytes = g->alg_bytes;
    if (flops) *flops = g->flops;
    if (launches) *launches = g->launches;
    g->alg_bytes = g->flops = 0.0;
    g->launches = 0;
    return TP_OK;
}
