// bodyforce.h -- self-weight: a design-dependent body force b (per unit volume at full density) on the trilinear hex, its
// consistent nodal load and the term it adds to the sensitivity of any linear response of the state.  Included from
// topopt_amd.hip behind stress.h.  DESIGN.md 4.12.
//
// V_e = hx hy hz, x_e the physical density the responses are evaluated on.
// Mass interpolation (the form of Du & Olhoff, "Topological design of freely vibrating continuum structures for maximum values
// of simple and multiple eigenfrequencies and frequency gaps", Struct. Multidisc. Optim. 34 (2007)): linear, C1-damped below
// x_low so that m / E stays bounded under SIMP.  With t = x / x_low (formed as x * (1 / x_low)):
//   x >= x_low or x_low = 0:  m(x) = x,                     m'(x) = 1
//   x <  x_low:               m(x) = x t^5 (6 - 5 t),       m'(x) = t^5 (36 - 35 t)
// (x_low = 0.1: 6e5 x^6 - 5e6 x^7; m(x_low) = x_low, m'(x_low) = 1, m' >= 0 on [0, 1]).  Evaluated in the factored form.
// Load:         f_n = (V_e / 8) b  sum_{e contains n} m(x_e)       -- the same for the three components up to b_c; owned node
//               planes, ghost planes untouched, supports NOT applied (tp_elasticity_solve multiplies by N); <= 8 incident
//               elements in one fixed order, elements outside the mesh skipped.  A gather: no atomics, the same bits on any
//               number of slabs.
// Sensitivity:  d (v^T N f) / dx_e = m'(x_e) (V_e / 8) sum_{a = 1..8} sum_c b_c N_{a,c} v_{a,c}   for a state or adjoint v; N is
//               applied inside, so v need not vanish on the clamped dofs.  Linear in v: several fields are weighted and summed
//               in the thread, one pass.
// Totals with K u = N (F + f(x)):  c = (F + f)^T u = u^T K u,  dc/dx_e = -p x^(p-1) (Emax - Emin) u_e^T KE u_e + 2 d(u^T N f)/dx_e;
// a stress p-norm with adjoint lam gains + d(lam^T N f)/dx_e (factor 1).
//
// m is evaluated where it is used, eight times per node in k_body_load: about 12 flops each against 56 bytes per node, far
// below the machine balance; a separate m(x) array would cost a launch and 16 bytes per element more.  The one thing that
// crosses the slab border is the upper neighbour's first own layer of x (one ghost layer, exchange_segments).
#pragma once

struct BodyPar {
    double vb[3];    // (V_e / 8) b_c
    double x_low, inv_low;  // inv_low = 1 / x_low (0 where x_low = 0: that branch is never taken for x >= 0)
};
struct BodyFields {
    const double *V[TP_MAX_CASES];
    double w[TP_MAX_CASES];
    int ncase;
};

__host__ __device__ __forceinline__ double body_mass(double x, double x_low, double inv_low) {
    if (x >= x_low) return x;
    const double t = x * inv_low, t2 = t * t;
    return x * ((t2 * t2 * t) * (6.0 - 5.0 * t));
}
__host__ __device__ __forceinline__ double body_dmass(double x, double x_low, double inv_low) {
    if (x >= x_low) return 1.0;
    const double t = x * inv_low, t2 = t * t;
    return (t2 * t2 * t) * (36.0 - 35.0 * t);
}

// One thread per OWNED node, the gather of k_stress_adjoint_rhs with one scalar per element.  Element layers 0 .. ez_own - 1
// come from x, layer ez_own (slabs with an upper neighbour: g.ezl = ez_own + 1) from the ghost layer xg.  rhs may be rhs_base:
// a thread reads its own three values before it writes them.
__global__ __launch_bounds__(BLK) void k_body_load(Geom g, BodyPar p, const double *__restrict__ x, const double *__restrict__ xg,
                                                   const double *rhs_base, double *rhs) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    const long n = g.plane() * g.own_lo + t;
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
    double s = 0.0;
#pragma unroll
    for (int n8 = 0; n8 < 8; n8++) {
        const int ei = i - (n8 & 1), ej = j - ((n8 >> 1) & 1), ek = k - (n8 >> 2);
        if (ei < 0 || ei >= g.ex || ej < 0 || ej >= g.ey || ek < 0 || ek >= g.ezl) continue;
        const long lay = (long)ei + (long)g.ex * ej;
        const double xe = ek < g.ez_own ? x[lay + (long)g.ex * g.ey * ek] : xg[lay];
        s += body_mass(xe, p.x_low, p.inv_low);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double r = p.vb[c] * s;
        if (rhs_base) r = rhs_base[3 * n + c] + r;
        rhs[3 * n + c] = r;
    }
}

// One thread per own element in the pattern of k_objective: b_c N_{a,c} of the eight corners stays in registers (24 values), the
// fields stream past it one after the other.  dfdx += scale m'(x_e) (V_e / 8) sum_l w_l sum_a sum_c b_c N v_l.
__global__ __launch_bounds__(BLK) void k_body_sens(Geom g, BodyPar p, BodyFields a, const double *__restrict__ N,
                                                   const double *__restrict__ x, double scale, double *__restrict__ dfdx) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.own_elems()) return;
    int i, j, k;
    elem_ijk(g, t, i, j, k);
    const long nd0 = elem_node0(g, i, j, k);
    double bn[24];
    gather24(g, nd0, N, bn);
#pragma unroll
    for (int r = 0; r < 24; r++) bn[r] = p.vb[r % 3] * bn[r];
    double acc = 0.0;
    for (int l = 0; l < a.ncase; l++) {
        double ve[24], s = 0.0;
        gather24(g, nd0, a.V[l], ve);
#pragma unroll
        for (int r = 0; r < 24; r++) s = fma(bn[r], ve[r], s);
        acc = fma(a.w[l], s, acc);
    }
    dfdx[t] += (scale * body_dmass(x[t], p.x_low, p.inv_low)) * acc;
}

#ifndef TP_BODIES_ONLY  // (tools/mass_bodies_check.cpp takes the kernels and m, m' alone)
static bool body_par(const double *b3, double x_low, const tp_grid *g, BodyPar *p) {
    if (!(x_low >= 0.0 && x_low < 1.0)) return false;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(b3[c])) return false;
    if (!g) return true;  // (the checks alone)
    const double v8 = g->o.hx * g->o.hy * g->o.hz / 8.0;
    for (int c = 0; c < 3; c++) p->vb[c] = v8 * b3[c];
    p->x_low = x_low;
    p->inv_low = x_low > 0.0 ? 1.0 / x_low : 0.0;
    return true;
}

extern "C" int tp_elasticity_body_load(tp_elasticity *e, const double *xPhys, const double *b3, double x_low, const double *rhs_base,
                                       double *rhs) {
    if (!e || !xPhys || !b3 || !rhs || !body_par(b3, x_low, nullptr, nullptr)) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    Geom q = e->mg.lv[0].g;
    BodyPar p;
    body_par(b3, x_low, g, &p);
    const long lay = (long)q.ex * q.ey, nown = q.owned_nodes();
    if (g->has_comm) {  // the ghost element layer above <- the upper neighbour's first own layer, as tp_elasticity_assemble fills d_E
        if (!e->d_xg) TP_TRY(e->d_xg.alloc((size_t)lay));
        TP_TRY(exchange_segments(g, xPhys, nullptr, nullptr, e->d_xg, lay, 1, lay));
    }
    TP_LAUNCH(k_body_load, dim3((int)((nown + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, p, xPhys, (const double *)e->d_xg, rhs_base, rhs);
    count_launch(g, 8.0 * q.own_elems() + (rhs_base ? 48.0 : 24.0) * nown, (8.0 * 12 + 6) * nown);
    return TP_OK;
}

extern "C" int tp_elasticity_body_sensitivity(tp_elasticity *e, int ncase, const double *const *V, const double *w, const double *xPhys,
                                              const double *b3, double x_low, double scale, double *dfdx) {
    if (!e || !V || !xPhys || !b3 || !dfdx || ncase < 1 || ncase > TP_MAX_CASES) return TP_ERR_ARG;
    if (!body_par(b3, x_low, nullptr, nullptr) || !std::isfinite(scale)) return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!V[l]) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    Geom q = e->mg.lv[0].g;
    BodyPar p;
    body_par(b3, x_low, g, &p);
    BodyFields a{};
    a.ncase = ncase;
    int ndistinct = 0;
    for (int l = 0; l < ncase; l++) {
        a.V[l] = V[l];
        a.w[l] = w ? w[l] : 1.0;
        bool seen = false;
        for (int m = 0; m < l; m++) seen = seen || V[m] == V[l];
        if (!seen) {
            TP_TRY(halo_nodes(g, q, const_cast<double *>(V[l]), 3));  // DMGlobalToLocal, as tp_elasticity_response
            ndistinct++;
        }
    }
    const long nel = q.own_elems();
    TP_LAUNCH(k_body_sens, dim3((int)((nel + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, p, a, (const double *)e->d_N, xPhys, scale, dfdx);
    count_launch(g, 24.0 * nel + 24.0 * q.owned_nodes() * (ndistinct + 1), (48.0 * ncase + 2.0 * ncase + 24 + 12) * nel);
    return TP_OK;
}
#endif
