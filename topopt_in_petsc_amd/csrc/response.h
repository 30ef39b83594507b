// response.h -- compliance-type responses of the state and their sensitivities: the single-case objective (k_objective, the
// reference's form) and the weighted response of several load cases (k_response).  Included from topopt_amd.hip behind the
// elasticity entry points.  DESIGN.md 4.8.
#pragma once

// fx = sum_e E_e u_e^T KE u_e, dfdx_e = -p x^(p-1) (Emax-Emin) u_e^T KE u_e, partial sum x
// (LinearElasticity.cc:405-437); one thread per own element, KE rows wave-uniform.
// REDUCE = false: the sensitivities alone (LinearElasticity.cc:299-361) -- no sums, nothing for the host to wait for.
template <bool REDUCE>
__global__ __launch_bounds__(BLK) void k_objective(Geom g, const double *__restrict__ KE, const double *__restrict__ U,
                                                   const double *__restrict__ x, double Emin, double Emax, double penal,
                                                   double *__restrict__ dfdx, double *__restrict__ partials) {
    const long nel = g.own_elems();
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    double f = 0.0, vol = 0.0;
    if (t < nel) {
        int i, j, k;
        elem_ijk(g, t, i, j, k);
        double ue[24];
        gather24(g, i, j, k, U, ue);
        double uKu = 0.0;
#pragma unroll
        for (int r = 0; r < 24; r++) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 24; c++) s = fma(KE[r * 24 + c], ue[c], s);
            uKu = fma(ue[r], s, uKu);
        }
        const double xe = x[t];
        f = (Emin + pow(xe, penal) * (Emax - Emin)) * uKu;
        vol = xe;
        if (dfdx) dfdx[t] = -1.0 * penal * pow(xe, penal - 1) * (Emax - Emin) * uKu;
    }
    if (!REDUCE) return;
    f = block_sum(f);
    vol = block_sum(vol);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = f;
        partials[gridDim.x + blockIdx.x] = vol;
    }
}

extern "C" int tp_elasticity_objective(tp_elasticity *e, const double *U, const double *xPhys, double Emin, double Emax,
                                       double penal, double volfrac, double *fx, double *gx, double *dfdx,
                                       double *dgdx) {
    tp_grid *g = e->grid;
    Geom q = e->mg.lv[0].g;
    const long nel = q.own_elems();
    const long nel_glob = (long)g->ex * g->ey * g->ez_glob;
    TP_TRY(halo_nodes(g, q, const_cast<double *>(U), 3));  // DMGlobalToLocal, :388-390
    const int nb = (int)((nel + BLK - 1) / BLK);
    if (!fx && !gx) {  // sensitivities only: no reduction, no host synchronisation
        if (dfdx) {
            TP_LAUNCH(k_objective<false>, dim3(nb), dim3(BLK), 0, g->stream, q, e->d_KE, U, xPhys, Emin, Emax, penal, dfdx, g->partials);
            count_launch(g, 24.0 * q.owned_nodes() + 16.0 * nel, 2.0 * 600 * nel);
        }
    } else {
        TP_LAUNCH(k_objective<true>, dim3(nb), dim3(BLK), 0, g->stream, q, e->d_KE, U, xPhys, Emin, Emax, penal, dfdx, g->partials);
        count_launch(g, 24.0 * q.owned_nodes() + 16.0 * nel, 2.0 * 600 * nel);
        TP_TRY(reduce_partials<2>(g, nb, S_TMP));
        double v[2];
        TP_TRY(read_scal(g, S_TMP, 2, v));
        if (fx) *fx = v[0];
        if (gx) *gx = v[1] / (double)nel_glob - volfrac;
    }
    if (dgdx) TP_TRY(tp_vec_set(g, dgdx, 1.0 / (double)nel_glob, nel));
    return TP_OK;
}
// The reference's split forms (main.cc can call either pair instead of the fused method):
// ComputeObjectiveConstraints minus the solve (LinearElasticity.cc:237-294): fx and gx of the state U, no sensitivities
extern "C" int tp_elasticity_objective_only(tp_elasticity *e, const double *U, const double *xPhys, double Emin, double Emax,
                                            double penal, double volfrac, double *fx, double *gx) {
    if (!e || !U || !xPhys || !fx || !gx) return TP_ERR_ARG;
    return tp_elasticity_objective(e, U, xPhys, Emin, Emax, penal, volfrac, fx, gx, nullptr, nullptr);
}
// ComputeSensitivities (LinearElasticity.cc:299-361): dfdx, dgdx of the state U as it is -- no solve, no sums
extern "C" int tp_elasticity_sensitivities(tp_elasticity *e, const double *U, const double *xPhys, double Emin, double Emax,
                                           double penal, double *dfdx, double *dgdx) {
    if (!e || !U || !xPhys || !dfdx) return TP_ERR_ARG;
    return tp_elasticity_objective(e, U, xPhys, Emin, Emax, penal, 0.0, nullptr, nullptr, dfdx, dgdx);
}

// ---- several load cases: the weighted response  sum_l w_l sum_e E_e v_l^T KE u_l  and its sensitivity in one pass
// (V_l = U_l: compliance of case l; V_l an adjoint state: the sensitivity of any linear response of U_l).
// One thread per own element like k_objective, the cases in a loop inside the thread: xPhys is read once, pow is
// evaluated once (x^p = x^(p-1) x), dfdx is written once.  The registers hold ONE case's u_e at a time (48 VGPRs); v_e is
// never held -- entry r is read where row r of KE u_e is complete, and used once.  BILINEAR = false (every V_l is U_l)
// has no loads of V at all.  REDUCE: ncase + 1 block sums (f_l = sum_e E_e v_l^T KE u_l, unweighted, and the volume) to
// partials[value][block], same layout and summation order as k_objective's two.
struct RespArgs {
    const double *U[TP_MAX_CASES];
    const double *V[TP_MAX_CASES];  // BILINEAR: never NULL (the host puts U[l] where the caller passed none)
    double w[TP_MAX_CASES];
    int ncase;
};
template <bool BILINEAR, bool REDUCE>
__global__ __launch_bounds__(BLK) void k_response(Geom g, const double *__restrict__ KE, RespArgs a,
                                                  const double *__restrict__ x, double Emin, double Emax, double penal,
                                                  double *__restrict__ dfdx, double *__restrict__ partials) {
    const long nel = g.own_elems();
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    const bool in = t < nel;
    long nd0 = 0;
    double xe = 0.0, xp1 = 0.0, E = 0.0;
    if (in) {
        int i, j, k;
        elem_ijk(g, t, i, j, k);
        nd0 = elem_node0(g, i, j, k);
        xe = x[t];
        xp1 = pow(xe, penal - 1);
        E = Emin + (xe == 0.0 ? 0.0 : xp1 * xe) * (Emax - Emin);  // (x = 0: x^p = 0 for p > 0 whatever x^(p-1) is)
    }
    double acc = 0.0;
    for (int l = 0; l < a.ncase; l++) {
        double vKu = 0.0;
        if (in) {
            double ue[24];
            gather24(g, nd0, a.U[l], ue);
            const double *__restrict__ V = BILINEAR ? a.V[l] : nullptr;
#pragma unroll
            for (int r = 0; r < 24; r++) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < 24; c++) s = fma(KE[r * 24 + c], ue[c], s);
                double vr = ue[r];
                if (BILINEAR) vr = V[3 * corner_node(g, nd0, r / 3) + r % 3];
                vKu = fma(vr, s, vKu);
            }
            acc = fma(a.w[l], vKu, acc);
        }
        if (REDUCE) {  // (every thread of the workgroup passes here: l is uniform)
            const double f = block_sum(E * vKu);
            if (threadIdx.x == 0) partials[(long)l * gridDim.x + blockIdx.x] = f;
        }
    }
    if (in && dfdx) dfdx[t] = -1.0 * penal * xp1 * (Emax - Emin) * acc;
    if (REDUCE) {
        const double vol = block_sum(xe);
        if (threadIdx.x == 0) partials[(long)a.ncase * gridDim.x + blockIdx.x] = vol;
    }
}

extern "C" int tp_elasticity_response(tp_elasticity *e, int ncase, const double *const *U, const double *const *V, const double *w,
                                      const double *xPhys, double Emin, double Emax, double penal, double volfrac, double *f_case,
                                      double *fx, double *gx, double *dfdx, double *dgdx) {
    if (!e || !U || !xPhys || ncase < 1 || ncase > TP_MAX_CASES) return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!U[l]) return TP_ERR_ARG;
    tp_grid *g = e->grid;
    Geom q = e->mg.lv[0].g;
    const long nel = q.own_elems();
    const long nel_glob = (long)g->ex * g->ey * g->ez_glob;
    RespArgs a{};
    a.ncase = ncase;
    bool bilinear = false;
    const double *distinct[2 * TP_MAX_CASES];
    int ndistinct = 0;
    auto note = [&](const double *p) {
        for (int i = 0; i < ndistinct; i++)
            if (distinct[i] == p) return;
        distinct[ndistinct++] = p;
    };
    for (int l = 0; l < ncase; l++) {
        a.U[l] = U[l];
        a.V[l] = (V && V[l]) ? V[l] : U[l];
        a.w[l] = w ? w[l] : 1.0;
        bilinear = bilinear || a.V[l] != a.U[l];
        note(a.U[l]);
        note(a.V[l]);
    }
    for (int i = 0; i < ndistinct; i++) TP_TRY(halo_nodes(g, q, const_cast<double *>(distinct[i]), 3));  // DMGlobalToLocal, :388-390
    const int nb = (int)((nel + BLK - 1) / BLK);
    auto launch = [&](bool reduce, double *partials) -> int {  // one of the four instantiations
        auto k = bilinear ? (reduce ? k_response<true, true> : k_response<true, false>)
                          : (reduce ? k_response<false, true> : k_response<false, false>);
        TP_LAUNCH(k, dim3(nb), dim3(BLK), 0, g->stream, q, e->d_KE, a, xPhys, Emin, Emax, penal, dfdx, partials);
        count_launch(g, 24.0 * q.owned_nodes() * ndistinct + 16.0 * nel, 2.0 * 600 * nel * ncase);
        return TP_OK;
    };
    if (!fx && !gx && !f_case) {  // sensitivities only: no reduction, no host synchronisation
        if (dfdx) TP_TRY(launch(false, nullptr));
    } else {
        if (e->resp_nb < nb) {  // (the grid's own partials hold four values per workgroup)
            TP_HIP(hipStreamSynchronize(g->stream));
            e->resp_nb = 0;
            TP_TRY(e->d_resp.alloc((TP_MAX_CASES + 1) * (size_t)nb));
            e->resp_nb = nb;
        }
        TP_TRY(launch(true, e->d_resp));
        TP_TRY(reduce_partials_n(g, e->d_resp, nb, ncase + 1, S_TMP));
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
