// thermoelastic.h -- thermal expansion as a design-dependent load on the elastic problem: a nodal temperature field T makes
// element e push on its 24 dofs with beta(x_e) G (T_e - T_ref), G the 24 x 8 coupling matrix of the box element
// (elements.h: thermal_coupling_box).  The load, its transpose (the right-hand side of the thermal adjoint) and its partial
// sensitivity at fixed T.  Included from topopt_amd.hip behind bodyforce.h.  DESIGN.md 4.18.
//
//   theta = T - T_ref at the nodes;  beta(x) = alpha (Emin + x^pb (Emax - Emin)),  beta'(x) = alpha pb x^(pb-1) (Emax - Emin)
//   Load:         f_th = sum_e beta_e G theta_e, owned node planes, ghost planes untouched, supports NOT applied
//                 (tp_elasticity_solve multiplies by N).
//   Transpose:    g_n = scale sum_{e contains n} beta_e sum_{a,c} G[(a,c), b(e,n)] (N sum_l w_l v_l)_{a,c}: a scalar per owned
//                 node, N applied inside, the fields combined first (the pass is linear in them).
//   Sensitivity:  dfdx_e += scale beta'_e sum_l w_l (N v_l)_e^T G theta_e.
//   Totals with K u = N (F + f_th), A(k) T = N_T q:  c = u^T K u,
//                 dc/dx_e = -p x^(p-1) (Emax - Emin) u_e^T KE u_e + 2 beta'_e (N u)_e^T G theta_e
//                           - 2 p x^(p-1) (kmax - kmin) mu_e^T KT T_e,   A mu = N_T g(u).
//
// G[(a,c), b] = sgn_c(a) gm[3 c + m]: the sign is corner a's side of axis c, m the number of the two other axes along which a
// and b differ.  The nine magnitudes are kernel arguments (scalar registers), never read from memory.
// beta and beta' are formed by a pass of their own (k_thermal_coef), own layers and the ghost layer above: two pow per element
// there instead of eight per node inside the gathers.  What crosses the slab border: the upper neighbour's first own layer of
// x (exchange_segments, as tp_elasticity_body_load), one halo plane of T and of every v (halo_nodes).
#pragma once

struct ThermPar {
    double gm[9];                    // |G| by component and number of differing other axes
    double alpha, T_ref, Emin, dE, pb;
};
struct ThermFields {
    const double *V[TP_MAX_CASES];
    double w[TP_MAX_CASES];
    int ncase;
};

// corner a's bit along axis d, and which of the three magnitudes of component c couples corners a and b (compile time in the
// unrolled loops)
__host__ __device__ constexpr int therm_bit(int a, int d) { return d == 0 ? LXc(a) : (d == 1 ? LYc(a) : LZc(a)); }
__host__ __device__ constexpr int therm_m(int a, int b, int c) {
    return (therm_bit(a, (c + 1) % 3) != therm_bit(b, (c + 1) % 3) ? 1 : 0) + (therm_bit(a, (c + 2) % 3) != therm_bit(b, (c + 2) % 3) ? 1 : 0);
}
// neighbour slot of corner b seen from corner a of the same element: (dz + 1) 9 + (dy + 1) 3 + (dx + 1)
__host__ __device__ constexpr int therm_q(int a, int b) {
    return (LZc(b) - LZc(a) + 1) * 9 + (LYc(b) - LYc(a) + 1) * 3 + (LXc(b) - LXc(a) + 1);
}

// One thread per stored element (own layers, and the ghost layer above from xg on a slab with an upper neighbour).  The pass is
// bound by its pow: an output nobody asked for (NULL) is not formed.
__global__ __launch_bounds__(BLK) void k_thermal_coef(Geom g, ThermPar p, const double *__restrict__ x, const double *__restrict__ xg,
                                                      double *__restrict__ beta, double *__restrict__ dbeta) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.elems_stored()) return;
    const long nown = g.own_elems();
    const double xe = t < nown ? x[t] : xg[t - nown];
    if (beta) beta[t] = p.alpha * (p.Emin + pow(xe, p.pb) * p.dE);
    if (dbeta) dbeta[t] = p.alpha * p.pb * pow(xe, p.pb - 1.0) * p.dE;
}

// the 27 neighbour addresses of a node, clamped axis by axis to the mesh and the local planes: a step beyond the border stays on
// the node's own row, column or plane.  A clamped address is read but its value enters no sum: it belongs to the corners of
// elements beyond the mesh only, which are skipped.  Three offsets per axis instead of 27 selected addresses.
struct ThermNb {
    int cx, cy, cz;
    long ox[3], oy[3], oz[3];
    __device__ __forceinline__ ThermNb(const Geom &g, int i, int j, int k) {
        cx = i == 0 ? 0 : (i >= g.ex ? 2 : 1), cy = j == 0 ? 0 : (j >= g.ey ? 2 : 1), cz = k == 0 ? 0 : (k >= g.ezl ? 2 : 1);
        ox[0] = cx == 0 ? 0 : -1, ox[1] = 0, ox[2] = cx == 2 ? 0 : 1;
        oy[0] = cy == 0 ? 0 : -(long)g.nx, oy[1] = 0, oy[2] = cy == 2 ? 0 : (long)g.nx;
        oz[0] = cz == 0 ? 0 : -g.plane(), oz[1] = 0, oz[2] = cz == 2 ? 0 : g.plane();
    }
    __device__ __forceinline__ long at(long n, int dx, int dy, int dz) const { return n + ox[dx + 1] + oy[dy + 1] + oz[dz + 1]; }
    // the element in which the node is corner a exists
    __device__ __forceinline__ bool elem(int a) const {
        return !((LXc(a) ? cx == 0 : cx == 2) || (LYc(a) ? cy == 0 : cy == 2) || (LZc(a) ? cz == 0 : cz == 2));
    }
};

// One thread per OWNED node.  The 27 values of theta once (ThermNb's addresses), then the <= 8 elements in corner order a = 0 .. 7 (the node is corner
// a of element (i, j, k) - L(a)), per element and component the 8-term sum of magnitudes times theta, the sign and beta_e in one
// fma.  rhs may be rhs_base: a thread reads its own three values before it writes them.
__global__ __launch_bounds__(BLK) void k_thermal_load(Geom g, ThermPar p, const double *__restrict__ beta, const double *__restrict__ T,
                                                      const double *rhs_base, double *rhs) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    const long n = g.plane() * g.own_lo + t;
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
    const ThermNb nb(g, i, j, k);
    double th[27];
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                th[(dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)] = T[nb.at(n, dx, dy, dz)] - p.T_ref;
            }
    double f[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 8; a++) {
        if (!nb.elem(a)) continue;
        const double be = beta[(long)(i - LXc(a)) + (long)g.ex * ((j - LYc(a)) + (long)g.ey * (k - LZc(a)))];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < 8; b++) s = fma(p.gm[3 * c + therm_m(a, b, c)], th[therm_q(a, b)], s);
            f[c] = fma(therm_bit(a, c) ? be : -be, s, f[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double r = f[c];
        if (rhs_base) r = rhs_base[3 * n + c] + r;
        rhs[3 * n + c] = r;
    }
}

// One thread per owned node, the transpose gather, component by component in a loop that is NOT unrolled: 27 neighbour values
// of N sum_l w_l v_l of component c (fields outermost, so that a field's 27 loads are in flight together) and the eight element
// sums live, not 27 x 3 values.  (Unrolled, the compiler moves the loads of all three components -- read-only, no-alias -- to
// the top whatever the source order: 256 VGPRs + 132 AGPRs, one wave per SIMD, 305 us at 128^3 against the load's 30;
// DESIGN 4.18.)  So that the loop body is the same code for every c it works in the frame of the axes (c, c + 1, c + 2): the
// sign comes from the corner's bit along the first axis, the magnitude from the two others, and only the three address offsets
// per axis and the three magnitudes are selected by c.  Element sums in that frame, rr[4 e0 + 2 e1 + e2] (the node is the
// TEMPERATURE corner (e0, e1, e2) of the element), inside it a = (a0, a1, a2) in index order; they are added to the element's
// own corner index r[b] at the end of each c.  Then the <= 8 elements in corner order with beta_e.
__global__ __launch_bounds__(BLK) void k_thermal_adjoint_rhs(Geom g, ThermPar p, ThermFields fl, const double *__restrict__ N,
                                                             const double *__restrict__ beta, double scale, double *__restrict__ out) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    const long n = g.plane() * g.own_lo + t;
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
    const ThermNb nb(g, i, j, k);
    double r[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
        long o0[3], o1[3], o2[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            o0[d] = c == 0 ? nb.ox[d] : (c == 1 ? nb.oy[d] : nb.oz[d]);
            o1[d] = c == 0 ? nb.oy[d] : (c == 1 ? nb.oz[d] : nb.ox[d]);
            o2[d] = c == 0 ? nb.oz[d] : (c == 1 ? nb.ox[d] : nb.oy[d]);
        }
        const double gm[3] = {c == 0 ? p.gm[0] : (c == 1 ? p.gm[3] : p.gm[6]), c == 0 ? p.gm[1] : (c == 1 ? p.gm[4] : p.gm[7]),
                              c == 0 ? p.gm[2] : (c == 1 ? p.gm[5] : p.gm[8])};
        double v[27];
#pragma unroll
        for (int q = 0; q < 27; q++) v[q] = 0.0;
        for (int l = 0; l < fl.ncase; l++) {
            const double *__restrict__ V = fl.V[l];
            const double wl = fl.w[l];
#pragma unroll
            for (int q = 0; q < 27; q++) v[q] = fma(wl, V[3 * (n + o0[q / 9] + o1[(q / 3) % 3] + o2[q % 3]) + c], v[q]);
        }
#pragma unroll
        for (int q = 0; q < 27; q++) v[q] = N[3 * (n + o0[q / 9] + o1[(q / 3) % 3] + o2[q % 3]) + c] * v[q];
        double rr[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int e0 = e >> 2, e1 = (e >> 1) & 1, e2 = e & 1;
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 8; a++) {
                const int a0 = a >> 2, a1 = (a >> 1) & 1, a2 = a & 1;
                const double gv = gm[(a1 != e1 ? 1 : 0) + (a2 != e2 ? 1 : 0)];
                s = fma(a0 ? gv : -gv, v[9 * (a0 - e0 + 1) + 3 * (a1 - e1 + 1) + (a2 - e2 + 1)], s);
            }
            rr[e] = s;
        }
        // frame bits -> the element's own corner index: (e0, e1, e2) are the bits along (x, y, z), (y, z, x), (z, x, y)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int e0 = e >> 2, e1 = (e >> 1) & 1, e2 = e & 1;
            if (c == 0) r[corner_of(e0, e1, e2)] += rr[e];
            else if (c == 1) r[corner_of(e2, e0, e1)] += rr[e];
            else r[corner_of(e1, e2, e0)] += rr[e];
        }
    }
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        if (!nb.elem(b)) continue;
        s = fma(beta[(long)(i - LXc(b)) + (long)g.ex * ((j - LYc(b)) + (long)g.ey * (k - LZc(b)))], r[b], s);
    }
    out[n] = scale * s;
}

// One thread per own element in the pattern of k_body_sens: N .* (G theta_e), 24 values, stays in registers, the fields stream
// past it.  dfdx += scale beta'_e sum_l w_l (N v_l)_e^T G theta_e.
__global__ __launch_bounds__(BLK) void k_thermal_sens(Geom g, ThermPar p, ThermFields fl, const double *__restrict__ N,
                                                      const double *__restrict__ dbeta, const double *__restrict__ T, double scale,
                                                      double *__restrict__ dfdx) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.own_elems()) return;
    int i, j, k;
    elem_ijk(g, t, i, j, k);
    const long nd0 = elem_node0(g, i, j, k);
    double th[8];
#pragma unroll
    for (int b = 0; b < 8; b++) th[b] = T[corner_node(g, nd0, b)] - p.T_ref;
    double gt[24];
    gather24(g, nd0, N, gt);
#pragma unroll
    for (int a = 0; a < 8; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < 8; b++) s = fma(p.gm[3 * c + therm_m(a, b, c)], th[b], s);
            gt[3 * a + c] = gt[3 * a + c] * (therm_bit(a, c) ? s : -s);
        }
    double acc = 0.0;
    for (int l = 0; l < fl.ncase; l++) {
        double ve[24], s = 0.0;
        gather24(g, nd0, fl.V[l], ve);
#pragma unroll
        for (int r = 0; r < 24; r++) s = fma(gt[r], ve[r], s);
        acc = fma(fl.w[l], s, acc);
    }
    dfdx[t] += (scale * dbeta[t]) * acc;
}

#ifndef TP_BODIES_ONLY  // (a stand-alone translation unit takes the kernels alone)
static bool therm_par_ok(const tp_thermal_par *par) {
    return par && std::isfinite(par->alpha) && std::isfinite(par->T_ref) && std::isfinite(par->Emin) && std::isfinite(par->Emax) &&
           std::isfinite(par->penal_beta) && par->penal_beta >= 1.0 && par->Emin >= 0.0 && par->Emax > par->Emin;
}

// beta (want & 1), beta' (want & 2) of this design on the own layers and the ghost layer above; fills p
static int therm_coef(tp_elasticity *e, const double *xPhys, const tp_thermal_par *par, ThermPar *p, int want) {
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    for (int m = 0; m < 9; m++) p->gm[m] = e->G9[m];
    p->alpha = par->alpha, p->T_ref = par->T_ref, p->Emin = par->Emin, p->dE = par->Emax - par->Emin, p->pb = par->penal_beta;
    const long lay = (long)q.ex * q.ey, nst = q.elems_stored();
    if (!e->d_beta) {
        TP_TRY(e->d_beta.alloc((size_t)(lay * (q.ez_own + 1))));
        TP_TRY(e->d_dbeta.alloc((size_t)(lay * (q.ez_own + 1))));
    }
    if (g->has_comm) {  // the ghost element layer above <- the upper neighbour's first own layer, as tp_elasticity_body_load
        if (!e->d_xg) TP_TRY(e->d_xg.alloc((size_t)lay));
        TP_TRY(exchange_segments(g, xPhys, nullptr, nullptr, e->d_xg, lay, 1, lay));
    }
    TP_LAUNCH(k_thermal_coef, dim3((int)((nst + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, *p, xPhys, (const double *)e->d_xg,
              (want & 1) ? (double *)e->d_beta : nullptr, (want & 2) ? (double *)e->d_dbeta : nullptr);
    count_launch(g, (want == 3 ? 24.0 : 16.0) * nst, (want == 3 ? 6.0 : 3.0) * nst);
    return TP_OK;
}

static int therm_fields(tp_elasticity *e, int ncase, const double *const *V, const double *w, ThermFields *a, int *ndistinct) {
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    *a = ThermFields{};
    a->ncase = ncase;
    *ndistinct = 0;
    for (int l = 0; l < ncase; l++) {
        a->V[l] = V[l];
        a->w[l] = w ? w[l] : 1.0;
        bool seen = false;
        for (int m = 0; m < l; m++) seen = seen || V[m] == V[l];
        if (!seen) {
            TP_TRY(halo_nodes(g, q, const_cast<double *>(V[l]), 3));  // DMGlobalToLocal, as tp_elasticity_response
            (*ndistinct)++;
        }
    }
    return TP_OK;
}

extern "C" int tp_elasticity_get_thermal_coupling(const tp_elasticity *e, double *G_host_192) {
    if (!e || !G_host_192) return TP_ERR_ARG;
    std::memcpy(G_host_192, e->G, sizeof(e->G));
    return TP_OK;
}

// introspection for the parity tests: beta and beta' of the own elements as k_thermal_coef leaves them; one of the two outputs may
// be NULL: that coefficient is then not formed, as in the three calls below
extern "C" int tp_elasticity_thermal_coefficients(tp_elasticity *e, const double *xPhys, const tp_thermal_par *par, double *beta,
                                                  double *dbeta) {
    if (!e || !xPhys || (!beta && !dbeta) || !therm_par_ok(par)) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    ThermPar p;
    TP_TRY(therm_coef(e, xPhys, par, &p, (beta ? 1 : 0) | (dbeta ? 2 : 0)));
    const size_t nb = sizeof(double) * (size_t)e->mg.lv[0].g.own_elems();
    if (beta) TP_HIP(hipMemcpyAsync(beta, e->d_beta, nb, hipMemcpyDeviceToDevice, e->grid->stream));
    if (dbeta) TP_HIP(hipMemcpyAsync(dbeta, e->d_dbeta, nb, hipMemcpyDeviceToDevice, e->grid->stream));
    return TP_OK;
}

extern "C" int tp_elasticity_thermal_load(tp_elasticity *e, const double *xPhys, const double *T, const tp_thermal_par *par,
                                          const double *rhs_base, double *rhs) {
    if (!e || !xPhys || !T || !rhs || !therm_par_ok(par)) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    ThermPar p;
    TP_TRY(therm_coef(e, xPhys, par, &p, 1));
    TP_TRY(halo_nodes(g, q, const_cast<double *>(T), 1));
    const long nown = q.owned_nodes();
    TP_LAUNCH(k_thermal_load, dim3((int)((nown + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, p, (const double *)e->d_beta, T, rhs_base, rhs);
    count_launch(g, 8.0 * q.elems_stored() + (8.0 + (rhs_base ? 48.0 : 24.0)) * nown, (27.0 + 8 * 3 * 18) * nown);
    return TP_OK;
}

extern "C" int tp_elasticity_thermal_sensitivity(tp_elasticity *e, int ncase, const double *const *V, const double *w, const double *xPhys,
                                                 const double *T, const tp_thermal_par *par, double scale, double *dfdx) {
    if (!e || !V || !xPhys || !T || !dfdx || ncase < 1 || ncase > TP_MAX_CASES) return TP_ERR_ARG;
    if (!therm_par_ok(par) || !std::isfinite(scale)) return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!V[l]) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    ThermPar p;
    TP_TRY(therm_coef(e, xPhys, par, &p, 2));
    ThermFields a;
    int ndistinct;
    TP_TRY(therm_fields(e, ncase, V, w, &a, &ndistinct));
    TP_TRY(halo_nodes(g, q, const_cast<double *>(T), 1));
    const long nel = q.own_elems();
    TP_LAUNCH(k_thermal_sens, dim3((int)((nel + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, p, a, (const double *)e->d_N,
              (const double *)e->d_dbeta, T, scale, dfdx);
    count_launch(g, 24.0 * nel + 8.0 * q.owned_nodes() + 24.0 * q.owned_nodes() * (ndistinct + 1), (8.0 + 24 * 17 + 50.0 * ncase + 3) * nel);
    return TP_OK;
}

extern "C" int tp_elasticity_thermal_adjoint_rhs(tp_elasticity *e, int ncase, const double *const *V, const double *w,
                                                 const double *xPhys, const tp_thermal_par *par, double scale, double *gout) {
    if (!e || !V || !xPhys || !gout || ncase < 1 || ncase > TP_MAX_CASES) return TP_ERR_ARG;
    if (!therm_par_ok(par) || !std::isfinite(scale)) return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!V[l]) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    ThermPar p;
    TP_TRY(therm_coef(e, xPhys, par, &p, 1));
    ThermFields a;
    int ndistinct;
    TP_TRY(therm_fields(e, ncase, V, w, &a, &ndistinct));
    const long nown = q.owned_nodes();
    TP_LAUNCH(k_thermal_adjoint_rhs, dim3((int)((nown + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, p, a, (const double *)e->d_N,
              (const double *)e->d_beta, scale, gout);
    count_launch(g, 8.0 * q.elems_stored() + (24.0 * (ndistinct + 1) + 8.0) * nown, (81.0 * (2 * ncase + 1) + 8 * 50 + 1) * nown);
    return TP_OK;
}
#endif
