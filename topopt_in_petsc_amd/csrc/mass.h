// mass.h -- the consistent mass matrix of the trilinear hex as an operator, and the mass half of an eigenvalue's design
// sensitivity.  Included from topopt_amd.hip behind bodyforce.h, whose mass interpolation m(x) it shares.  DESIGN.md 4.14.
//
// M_e = rho0 m(x_e) V_e (M8 (x) I_3), V_e = hx hy hz, M8[a,b] = (1/8) prod_axis (2/3 if corners a, b share that coordinate, else
// 1/3): 1/27, 1/54, 1/108, 1/216 for corner pairs that differ along 0, 1, 2, 3 axes; sum_ab M8 = 1.  B = N M N.
//   k_mass_coef   c_e = rho0 V_e m(x_e) for the own element layers and the ghost layer above (slabs), once per design
//   k_mass_apply  y = N M N u on the owned node planes: a gather, one thread per owned node.  The <= 8 incident elements in one
//                 fixed order (outside the mesh: coefficient 0), the 27 node-pair weights w_o = f_o sum_{e contains both} c_e formed
//                 once and used for the three components, the 27 neighbours in one fixed order.  No atomics, no sum depends on the
//                 partition: the same bits on any number of slabs.
//   k_mass_sens   out_e += scale m'(x_e) rho0 V_e sum_l w_l (N v_l)_e^T (M8 (x) I_3) (N v_l)_e, one thread per own element
// The two bodies are host-callable functions of the thread index, so that a stand-alone host program can run them thread by
// thread on exactly sized buffers.
#pragma once

struct MassPar {
    double rv;              // rho0 V_e
    double x_low, inv_low;  // as BodyPar
};

// f_o of the node pair at offset o: (1/8) (2/3)^(3 - d) (1/3)^d with d = number of non-zero offset components
__host__ __device__ constexpr double mass_pair_weight(int d) {
    return d == 0 ? 1.0 / 27.0 : (d == 1 ? 1.0 / 54.0 : (d == 2 ? 1.0 / 108.0 : 1.0 / 216.0));
}

// element layers 0 .. ez_own - 1 from x, layer ez_own (g.ezl = ez_own + 1) from the ghost layer xg
__global__ __launch_bounds__(BLK) void k_mass_coef(Geom g, MassPar p, const double *__restrict__ x, const double *__restrict__ xg,
                                                   double *__restrict__ mc) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.elems_stored()) return;
    const long own = g.own_elems();
    const double xe = t < own ? x[t] : xg[t - own];
    mc[t] = p.rv * body_mass(xe, p.x_low, p.inv_low);
}

// owned node t of the slab: y[3 n + c] = N_c(n) sum_o w_o N_c(n + o) u_c(n + o)
__host__ __device__ __forceinline__ void mass_apply_node(const Geom g, long t, const double *__restrict__ mc,
                                                         const double *__restrict__ N, const double *__restrict__ u,
                                                         double *__restrict__ y) {
    const long n = g.plane() * g.own_lo + t;
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
    double c[8];
#pragma unroll
    for (int n8 = 0; n8 < 8; n8++) {
        const int ei = i - (n8 & 1), ej = j - ((n8 >> 1) & 1), ek = k - (n8 >> 2);
        const bool in = ei >= 0 && ei < g.ex && ej >= 0 && ej < g.ey && ek >= 0 && ek < g.ezl;
        c[n8] = in ? mc[(long)ei + (long)g.ex * (ej + (long)g.ey * ek)] : 0.0;
    }
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int oz = -1; oz <= 1; oz++)
#pragma unroll
        for (int oy = -1; oy <= 1; oy++)
#pragma unroll
            for (int ox = -1; ox <= 1; ox++) {
                // element n8 (the node is its corner (n8 & 1, n8 >> 1 & 1, n8 >> 2)) holds the neighbour too if along every
                // axis the offset is 0 or points into the element
                double s = 0.0;
#pragma unroll
                for (int n8 = 0; n8 < 8; n8++) {
                    const int dx = n8 & 1, dy = (n8 >> 1) & 1, dz = n8 >> 2;
                    const bool both = (ox == 0 || ox == (dx ? -1 : 1)) && (oy == 0 || oy == (dy ? -1 : 1)) &&
                                      (oz == 0 || oz == (dz ? -1 : 1));
                    if (both) s += c[n8];
                }
                const int ni = i + ox, nj = j + oy, nk = k + oz;
                if (ni < 0 || ni >= g.nx || nj < 0 || nj >= g.ny || nk < 0 || nk >= g.nzl) continue;
                const double w = mass_pair_weight((ox != 0) + (oy != 0) + (oz != 0)) * s;
                const long m = (long)ni + (long)g.nx * (nj + (long)g.ny * nk);
#pragma unroll
                for (int d = 0; d < 3; d++) acc[d] = fma(w, N[3 * m + d] * u[3 * m + d], acc[d]);
            }
#pragma unroll
    for (int d = 0; d < 3; d++) y[3 * n + d] = N[3 * n + d] * acc[d];
}

// own element t: the quadratic form of every field on the element's 24 values, weighted, times scale m'(x_e) rho0 V_e
struct MassFields {
    const double *V[TP_MAX_CASES];
    double w[TP_MAX_CASES];
    int ncase;
};
__host__ __device__ __forceinline__ void mass_sens_elem(const Geom g, const MassPar p, const MassFields &a, long t,
                                                        const double *__restrict__ N, const double *__restrict__ x, double scale,
                                                        double *__restrict__ out) {
    const int i = (int)(t % g.ex), j = (int)((t / g.ex) % g.ey), k = (int)(t / ((long)g.ex * g.ey));
    const long nd0 = (long)i + (long)g.nx * (j + (long)g.ny * k);
    double nn[24];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const long nd = nd0 + LXc(b) + (long)g.nx * (LYc(b) + (long)g.ny * LZc(b));
#pragma unroll
        for (int d = 0; d < 3; d++) nn[3 * b + d] = N[3 * nd + d];
    }
    double acc = 0.0;
    for (int l = 0; l < a.ncase; l++) {
        const double *__restrict__ V = a.V[l];
        double ve[24];
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const long nd = nd0 + LXc(b) + (long)g.nx * (LYc(b) + (long)g.ny * LZc(b));
#pragma unroll
            for (int d = 0; d < 3; d++) ve[3 * b + d] = nn[3 * b + d] * V[3 * nd + d];
        }
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            double r[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int b2 = 0; b2 < 8; b2++) {
                const double f = mass_pair_weight((LXc(b) != LXc(b2)) + (LYc(b) != LYc(b2)) + (LZc(b) != LZc(b2)));
#pragma unroll
                for (int d = 0; d < 3; d++) r[d] = fma(f, ve[3 * b2 + d], r[d]);
            }
#pragma unroll
            for (int d = 0; d < 3; d++) s = fma(ve[3 * b + d], r[d], s);
        }
        acc = fma(a.w[l], s, acc);
    }
    out[t] += (scale * (p.rv * body_dmass(x[t], p.x_low, p.inv_low))) * acc;
}

__global__ __launch_bounds__(BLK) void k_mass_apply(Geom g, const double *__restrict__ mc, const double *__restrict__ N,
                                                    const double *__restrict__ u, double *__restrict__ y) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    mass_apply_node(g, t, mc, N, u, y);
}
__global__ __launch_bounds__(BLK) void k_mass_sens(Geom g, MassPar p, MassFields a, const double *__restrict__ N,
                                                   const double *__restrict__ x, double scale, double *__restrict__ out) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.own_elems()) return;
    mass_sens_elem(g, p, a, t, N, x, scale, out);
}

#ifndef TP_BODIES_ONLY  // (a stand-alone host program runs the bodies above thread by thread: tools/mass_bodies_check.cpp)
extern "C" int tp_elasticity_mass_assemble(tp_elasticity *e, const double *xPhys, double rho0, double x_low) {
    if (!e || !xPhys || !(rho0 > 0.0) || !std::isfinite(rho0) || !(x_low >= 0.0 && x_low < 1.0)) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    Geom q = e->mg.lv[0].g;
    MassPar p{rho0 * (g->o.hx * g->o.hy * g->o.hz), x_low, x_low > 0.0 ? 1.0 / x_low : 0.0};
    const long lay = (long)q.ex * q.ey, nst = q.elems_stored();
    if (!e->d_mc) TP_TRY(e->d_mc.alloc((size_t)nst));
    if (g->has_comm) {  // the ghost element layer above <- the upper neighbour's first own layer, as tp_elasticity_body_load
        if (!e->d_xg) TP_TRY(e->d_xg.alloc((size_t)lay));
        TP_TRY(exchange_segments(g, xPhys, nullptr, nullptr, e->d_xg, lay, 1, lay));
    }
    TP_LAUNCH(k_mass_coef, dim3((int)((nst + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, p, xPhys, (const double *)e->d_xg,
              (double *)e->d_mc);
    count_launch(g, 16.0 * nst, 12.0 * nst);
    e->mass_rv = p.rv, e->mass_xlow = p.x_low, e->mass_invlow = p.inv_low;
    e->have_mass = true;
    return TP_OK;
}

extern "C" int tp_elasticity_mass_apply(tp_elasticity *e, const double *u, double *y) {
    if (!e || !u || !y || u == y) return TP_ERR_ARG;
    if (!e->have_bc || !e->have_mass) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    Geom q = e->mg.lv[0].g;
    TP_TRY(halo_nodes(g, q, const_cast<double *>(u), 3));
    const long nown = q.owned_nodes();
    TP_LAUNCH(k_mass_apply, dim3((int)((nown + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, (const double *)e->d_mc,
              (const double *)e->d_N, u, y);
    count_launch(g, 72.0 * nown + 8.0 * q.elems_stored(), (27.0 * 9 + 27 * 4 + 3) * nown);
    return TP_OK;
}

extern "C" int tp_elasticity_mass_sensitivity(tp_elasticity *e, int ncase, const double *const *V, const double *w,
                                              const double *xPhys, double scale, double *out) {
    if (!e || !V || !xPhys || !out || ncase < 1 || ncase > TP_MAX_CASES || !std::isfinite(scale)) return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!V[l]) return TP_ERR_ARG;
    if (!e->have_bc || !e->have_mass) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    Geom q = e->mg.lv[0].g;
    MassFields a{};
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
    TP_LAUNCH(k_mass_sens, dim3((int)((nel + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, MassPar{e->mass_rv, e->mass_xlow, e->mass_invlow}, a, (const double *)e->d_N,
              xPhys, scale, out);
    count_launch(g, 24.0 * nel + 24.0 * q.owned_nodes() * (ndistinct + 1), (24.0 * 18 + 26) * ncase * nel);
    return TP_OK;
}
#endif
