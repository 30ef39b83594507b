// geomstiff.h -- the geometric (stress) stiffness of the trilinear hex as an operator, and its two derivatives: the pieces of a
// linear buckling analysis B phi = mu A phi with B = -N G(x, u) N.  Included from topopt_amd.hip behind mass.h, whose field
// list (MassFields) it shares.  DESIGN.md 4.19.
//
// Per element, at the 8 Gauss points of hex8_stiffness_box (weight wq = hx hy hz / 8; tables of elements.h:
// hex8_geom_tables_box): sigma(gp) = C0 B(gp) u_e, the unit-modulus stress, S its symmetric 3 x 3 tensor,
//   g_e[a,b] = sum_gp wq gradN_a(gp)^T S(gp) gradN_b(gp),   G_e = Es(x_e) (g_e (x) I_3),   Es(x) = Emax x^p  (no Emin).
// g_e is symmetric and its rows sum to zero, so the 28 entries a < b say everything:
//   (G psi)_a = Es sum_{b != a} g_e[a,b] (psi_b - psi_a).
//   k_geom_modulus      Es(x_e), own element layers and the ghost layer above (slabs)
//   k_geom_coef         Es(x_e) g_e[a,b], a < b, plane by plane (entry p of element t at gc[p * stored + t]): 224 B per element,
//                       once per design and state.  The ghost layer's matrices are formed here like the own ones: the slab
//                       holds both node planes of u that they need (the top owned plane and the ghost plane above it).
//   k_geom_apply        y = N G N phi on the owned node planes: a gather, one thread per owned node.  The <= 8 incident
//                       elements in one fixed order (outside the mesh: nothing), the 26 node-pair weights formed once and used
//                       for the three components, the neighbours in one fixed order.  No atomics, no sum depends on the
//                       partition: the same bits on any number of slabs.
//   k_geom_sens         out_e += scale p x_e^(p-1) Emax sum_l w_l (N phi_l)_e^T (g_e(u_e) (x) I_3) (N phi_l)_e, one thread per own
//                       element, Gauss point by Gauss point as sigma : (grad phi^T grad phi); no 8 x 8 matrix is formed
//   k_geom_adjoint_rhs  out = scale sum_l w_l d((N phi_l)^T G (N phi_l)) / du on the owned node planes, supports not applied: per
//                       element Es wq sum_gp (C0 B(gp))^T s(gp), s the Voigt vector (s11, s22, s33, 2 s12, 2 s23, 2 s13) of
//                       s_ij = sum_k d phi_k/dx_i d phi_k/dx_j; a gather over the <= 8 incident elements in one fixed order
// The bodies are host-callable functions of the thread index, so that a stand-alone host program can run them thread by thread on
// exactly sized buffers (tools/geom_bodies_check.cpp).
#pragma once

constexpr int GEOM_NP = 28;    // pairs a < b of the 8 corners
constexpr int GEOM_TAB = 192 + 1152;  // gradN, then C0 B

// index of the pair (a, b), a != b, in the upper triangle taken row by row
__host__ __device__ constexpr int geom_pair(int a, int b) {
    return (a < b ? a : b) * 7 - ((a < b ? a : b) * ((a < b ? a : b) - 1)) / 2 + ((a < b ? b - a : a - b) - 1);
}
// the displacement component that shear row r (3: xy, 4: yz, 5: zx) does not see
__host__ __device__ constexpr int geom_row_skips(int r, int c) { return r >= 3 && c == (r == 3 ? 2 : (r == 4 ? 0 : 1)); }

// sigma(gp q) = (C0 B(q)) ue, rows xx, yy, zz, xy, yz, zx; the structural zeros of the shear rows are left out
__host__ __device__ __forceinline__ void geom_sigma(const double *__restrict__ cb, int q, const double (&ue)[24], double (&sg)[6]) {
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 24; j++) {
            if (geom_row_skips(r, j % 3)) continue;
            s = fma(cb[(6 * q + r) * 24 + j], ue[j], s);
        }
        sg[r] = s;
    }
}
// H[3 k + d] = d v_k / dx_d at Gauss point q
__host__ __device__ __forceinline__ void geom_grad(const double *__restrict__ gn, int q, const double (&ve)[24], double (&H)[9]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < 8; b++) s = fma(gn[(3 * q + d) * 8 + b], ve[3 * b + k], s);
            H[3 * k + d] = s;
        }
}
// the Voigt vector (s11, s22, s33, 2 s12, 2 s23, 2 s13) of s_ij = sum_k H[k][i] H[k][j]
__host__ __device__ __forceinline__ void geom_voigt(const double (&H)[9], double (&s)[6]) {
    s[0] = fma(H[6], H[6], fma(H[3], H[3], H[0] * H[0]));
    s[1] = fma(H[7], H[7], fma(H[4], H[4], H[1] * H[1]));
    s[2] = fma(H[8], H[8], fma(H[5], H[5], H[2] * H[2]));
    s[3] = 2.0 * fma(H[6], H[7], fma(H[3], H[4], H[0] * H[1]));
    s[4] = 2.0 * fma(H[7], H[8], fma(H[4], H[5], H[1] * H[2]));
    s[5] = 2.0 * fma(H[6], H[8], fma(H[3], H[5], H[0] * H[2]));
}

__global__ __launch_bounds__(BLK) void k_geom_modulus(Geom g, double Emax, double penal, const double *__restrict__ x,
                                                      const double *__restrict__ xg, double *__restrict__ es) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.elems_stored()) return;
    const long own = g.own_elems();
    es[t] = Emax * pow(t < own ? x[t] : xg[t - own], penal);
}

// stored element t (own layers from x, the ghost layer above from xg): the 28 entries of Es g_e
__host__ __device__ __forceinline__ void geom_coef_elem(const Geom g, long t, const double *__restrict__ tab, double wq, double Emax,
                                                        double penal, const double *__restrict__ x, const double *__restrict__ xg,
                                                        const double *__restrict__ U, double *__restrict__ gc) {
    const double *__restrict__ gn = tab, *__restrict__ cb = tab + 192;
    const int i = (int)(t % g.ex), j = (int)((t / g.ex) % g.ey), k = (int)(t / ((long)g.ex * g.ey));
    const long nd0 = (long)i + (long)g.nx * (j + (long)g.ny * k);
    const long own = g.own_elems(), nst = g.elems_stored();
    double ue[24];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const long nd = nd0 + LXc(b) + (long)g.nx * (LYc(b) + (long)g.ny * LZc(b));
#pragma unroll
        for (int d = 0; d < 3; d++) ue[3 * b + d] = U[3 * nd + d];
    }
    double acc[GEOM_NP];
#pragma unroll
    for (int p = 0; p < GEOM_NP; p++) acc[p] = 0.0;
#pragma unroll 1
    for (int q = 0; q < 8; q++) {
        double sg[6];
        geom_sigma(cb, q, ue, sg);
        double tb[24];   // S gradN_b
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const double g0 = gn[(3 * q + 0) * 8 + b], g1 = gn[(3 * q + 1) * 8 + b], g2 = gn[(3 * q + 2) * 8 + b];
            tb[3 * b + 0] = fma(sg[5], g2, fma(sg[3], g1, sg[0] * g0));
            tb[3 * b + 1] = fma(sg[4], g2, fma(sg[1], g1, sg[3] * g0));
            tb[3 * b + 2] = fma(sg[2], g2, fma(sg[4], g1, sg[5] * g0));
        }
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = a + 1; b < 8; b++) {
                const double v = fma(gn[(3 * q + 2) * 8 + a], tb[3 * b + 2],
                                     fma(gn[(3 * q + 1) * 8 + a], tb[3 * b + 1], gn[(3 * q + 0) * 8 + a] * tb[3 * b + 0]));
                acc[geom_pair(a, b)] += v;
            }
    }
    const double es = (Emax * pow(t < own ? x[t] : xg[t - own], penal)) * wq;
#pragma unroll
    for (int p = 0; p < GEOM_NP; p++) gc[(long)p * nst + t] = es * acc[p];
}

// owned node t of the slab: y_c(n) = N_c(n) sum_o w_o (psi_c(n + o) - psi_c(n)), psi = N phi
__host__ __device__ __forceinline__ void geom_apply_node(const Geom g, long t, const double *__restrict__ gc,
                                                         const double *__restrict__ N, const double *__restrict__ u,
                                                         double *__restrict__ y) {
    const long n = g.plane() * g.own_lo + t, nst = g.elems_stored();
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
    long el[8];
    bool in[8];
#pragma unroll
    for (int n8 = 0; n8 < 8; n8++) {
        const int ei = i - (n8 & 1), ej = j - ((n8 >> 1) & 1), ek = k - (n8 >> 2);
        in[n8] = ei >= 0 && ei < g.ex && ej >= 0 && ej < g.ey && ek >= 0 && ek < g.ezl;
        el[n8] = (long)ei + (long)g.ex * (ej + (long)g.ey * ek);
    }
    double nn[3], pn[3], acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < 3; d++) nn[d] = N[3 * n + d], pn[d] = nn[d] * u[3 * n + d];
#pragma unroll
    for (int oz = -1; oz <= 1; oz++)
#pragma unroll
        for (int oy = -1; oy <= 1; oy++)
#pragma unroll
            for (int ox = -1; ox <= 1; ox++) {
                if (ox == 0 && oy == 0 && oz == 0) continue;
                const int ni = i + ox, nj = j + oy, nk = k + oz;
                if (ni < 0 || ni >= g.nx || nj < 0 || nj >= g.ny || nk < 0 || nk >= g.nzl) continue;
                // element n8 (the node is its corner (n8 & 1, n8 >> 1 & 1, n8 >> 2)) holds the neighbour too if along every
                // axis the offset is 0 or points into the element
                double w = 0.0;
#pragma unroll
                for (int n8 = 0; n8 < 8; n8++) {
                    const int dx = n8 & 1, dy = (n8 >> 1) & 1, dz = n8 >> 2;
                    const bool both = (ox == 0 || ox == (dx ? -1 : 1)) && (oy == 0 || oy == (dy ? -1 : 1)) &&
                                      (oz == 0 || oz == (dz ? -1 : 1));
                    if (both) {
                        const int p = geom_pair(corner_of(dx, dy, dz), corner_of(dx + ox, dy + oy, dz + oz));
                        if (in[n8]) w += gc[(long)p * nst + el[n8]];
                    }
                }
                const long m = (long)ni + (long)g.nx * (nj + (long)g.ny * nk);
#pragma unroll
                for (int d = 0; d < 3; d++) acc[d] = fma(w, N[3 * m + d] * u[3 * m + d] - pn[d], acc[d]);
            }
#pragma unroll
    for (int d = 0; d < 3; d++) y[3 * n + d] = nn[d] * acc[d];
}

// own element t: sum_l w_l sum_gp sigma(gp) . s_l(gp), times scale p x^(p-1) Emax wq
__host__ __device__ __forceinline__ void geom_sens_elem(const Geom g, const MassFields &a, long t, const double *__restrict__ tab,
                                                        double wq, double Emax, double penal, const double *__restrict__ N,
                                                        const double *__restrict__ x, const double *__restrict__ U, double scale,
                                                        double *__restrict__ out) {
    const double *__restrict__ gn = tab, *__restrict__ cb = tab + 192;
    const int i = (int)(t % g.ex), j = (int)((t / g.ex) % g.ey), k = (int)(t / ((long)g.ex * g.ey));
    const long nd0 = (long)i + (long)g.nx * (j + (long)g.ny * k);
    double sg[8][6];
    {
        double ue[24];
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const long nd = nd0 + LXc(b) + (long)g.nx * (LYc(b) + (long)g.ny * LZc(b));
#pragma unroll
            for (int d = 0; d < 3; d++) ue[3 * b + d] = U[3 * nd + d];
        }
#pragma unroll
        for (int q = 0; q < 8; q++) geom_sigma(cb, q, ue, sg[q]);
    }
    double acc = 0.0;
    for (int l = 0; l < a.ncase; l++) {
        const double *__restrict__ V = a.V[l];
        double ve[24];
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const long nd = nd0 + LXc(b) + (long)g.nx * (LYc(b) + (long)g.ny * LZc(b));
#pragma unroll
            for (int d = 0; d < 3; d++) ve[3 * b + d] = N[3 * nd + d] * V[3 * nd + d];
        }
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            double H[9], sv[6];
            geom_grad(gn, q, ve, H);
            geom_voigt(H, sv);
#pragma unroll
            for (int r = 0; r < 6; r++) s = fma(sg[q][r], sv[r], s);
        }
        acc = fma(a.w[l], s, acc);
    }
    out[t] += (scale * (penal * pow(x[t], penal - 1.0) * Emax * wq)) * acc;
}

// owned node t of the slab: the three derivatives with respect to u at that node
__host__ __device__ __forceinline__ void geom_adjoint_node(const Geom g, const MassFields &a, long t, const double *__restrict__ tab,
                                                           double wq, const double *__restrict__ es, const double *__restrict__ N,
                                                           double scale, double *__restrict__ out) {
    const double *__restrict__ gn = tab, *__restrict__ cb = tab + 192;
    const long n = g.plane() * g.own_lo + t;
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
    double rc[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int n8 = 0; n8 < 8; n8++) {
        const int dx = n8 & 1, dy = (n8 >> 1) & 1, dz = n8 >> 2;
        const int ei = i - dx, ej = j - dy, ek = k - dz;
        if (!(ei >= 0 && ei < g.ex && ej >= 0 && ej < g.ey && ek >= 0 && ek < g.ezl)) continue;
        const int ca = dz * 4 + (dy ? (dx ? 2 : 3) : (dx ? 1 : 0));   // corner_of, at run time
        const long nd0 = (long)ei + (long)g.nx * (ej + (long)g.ny * ek);
        double S[8][6];
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
            for (int r = 0; r < 6; r++) S[q][r] = 0.0;
#pragma unroll 1
        for (int l = 0; l < a.ncase; l++) {
            const double *__restrict__ V = a.V[l];
            const double wl = a.w[l];
            double ve[24];
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const long nd = nd0 + LXc(b) + (long)g.nx * (LYc(b) + (long)g.ny * LZc(b));
#pragma unroll
                for (int d = 0; d < 3; d++) ve[3 * b + d] = N[3 * nd + d] * V[3 * nd + d];
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                double H[9], sv[6];
                geom_grad(gn, q, ve, H);
                geom_voigt(H, sv);
#pragma unroll
                for (int r = 0; r < 6; r++) S[q][r] = fma(wl, sv[r], S[q][r]);
            }
        }
        double re[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (geom_row_skips(r, c)) continue;
                    re[c] = fma(cb[(6 * q + r) * 24 + 3 * ca + c], S[q][r], re[c]);
                }
        const double ee = es[(long)ei + (long)g.ex * (ej + (long)g.ey * ek)] * wq;
#pragma unroll
        for (int c = 0; c < 3; c++) rc[c] = fma(ee, re[c], rc[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * n + c] = scale * rc[c];
}

__global__ __launch_bounds__(BLK) void k_geom_coef(Geom g, const double *__restrict__ tab, double wq, double Emax, double penal,
                                                   const double *__restrict__ x, const double *__restrict__ xg,
                                                   const double *__restrict__ U, double *__restrict__ gc) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.elems_stored()) return;
    geom_coef_elem(g, t, tab, wq, Emax, penal, x, xg, U, gc);
}
__global__ __launch_bounds__(BLK) void k_geom_apply(Geom g, const double *__restrict__ gc, const double *__restrict__ N,
                                                    const double *__restrict__ u, double *__restrict__ y) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    geom_apply_node(g, t, gc, N, u, y);
}
__global__ __launch_bounds__(BLK) void k_geom_sens(Geom g, MassFields a, const double *__restrict__ tab, double wq, double Emax,
                                                   double penal, const double *__restrict__ N, const double *__restrict__ x,
                                                   const double *__restrict__ U, double scale, double *__restrict__ out) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.own_elems()) return;
    geom_sens_elem(g, a, t, tab, wq, Emax, penal, N, x, U, scale, out);
}
__global__ __launch_bounds__(BLK) void k_geom_adjoint_rhs(Geom g, MassFields a, const double *__restrict__ tab, double wq,
                                                          const double *__restrict__ es, const double *__restrict__ N, double scale,
                                                          double *__restrict__ out) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    geom_adjoint_node(g, a, t, tab, wq, es, N, scale, out);
}

#ifndef TP_BODIES_ONLY  // (a stand-alone host program runs the bodies above thread by thread: tools/geom_bodies_check.cpp)
static bool geom_par_ok(double Emax, double penal) {
    return Emax > 0.0 && std::isfinite(Emax) && penal >= 1.0 && std::isfinite(penal);
}

// the tables on the device (first use) and the upper neighbour's first own layer of xPhys in d_xg
static int geom_prepare(tp_elasticity *e, const double *xPhys) {
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    if (!e->d_gtab) {
        TP_TRY(e->d_gtab.alloc((size_t)GEOM_TAB));
        TP_HIP(hipMemcpyAsync(e->d_gtab, e->GT, sizeof(e->GT), hipMemcpyHostToDevice, g->stream));
        TP_HIP(hipStreamSynchronize(g->stream));
    }
    if (g->has_comm) {  // the ghost element layer above <- the upper neighbour's first own layer, as tp_elasticity_body_load
        const long lay = (long)q.ex * q.ey;
        if (!e->d_xg) TP_TRY(e->d_xg.alloc((size_t)lay));
        TP_TRY(exchange_segments(g, xPhys, nullptr, nullptr, e->d_xg, lay, 1, lay));
    }
    return TP_OK;
}

static int geom_fields(tp_elasticity *e, int ncase, const double *const *V, const double *w, MassFields *a, int *ndistinct) {
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    *a = MassFields{};
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

extern "C" int tp_elasticity_get_geom_tables(const tp_elasticity *e, double *gradN_host_192, double *cb_host_1152) {
    if (!e || !gradN_host_192 || !cb_host_1152) return TP_ERR_ARG;
    std::memcpy(gradN_host_192, e->GT, sizeof(double) * 192);
    std::memcpy(cb_host_1152, e->GT + 192, sizeof(double) * 1152);
    return TP_OK;
}

extern "C" int tp_elasticity_geom_assemble(tp_elasticity *e, const double *xPhys, const double *U, double Emax, double penal) {
    if (!e || !xPhys || !U || !geom_par_ok(Emax, penal)) return TP_ERR_ARG;
    if (!e->have_bc) return TP_ERR_STATE;
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    const long nst = q.elems_stored();
    TP_TRY(geom_prepare(e, xPhys));
    if (!e->d_gc) TP_TRY(e->d_gc.alloc((size_t)(GEOM_NP * nst)));
    TP_TRY(halo_nodes(g, q, const_cast<double *>(U), 3));
    TP_LAUNCH(k_geom_coef, dim3((int)((nst + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, (const double *)e->d_gtab, e->geom_wq, Emax, penal,
              xPhys, (const double *)e->d_xg, U, (double *)e->d_gc);
    count_launch(g, (8.0 + 8.0 * GEOM_NP) * nst + 24.0 * q.owned_nodes(), (8.0 * (2 * 120 + 2 * 72 + 6 * GEOM_NP) + GEOM_NP) * nst);
    e->have_geom = true;
    return TP_OK;
}

extern "C" int tp_elasticity_geom_apply(tp_elasticity *e, const double *phi, double *y) {
    if (!e || !phi || !y || phi == y) return TP_ERR_ARG;
    if (!e->have_geom) return TP_ERR_ARG;
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    TP_TRY(halo_nodes(g, q, const_cast<double *>(phi), 3));
    const long nown = q.owned_nodes();
    TP_LAUNCH(k_geom_apply, dim3((int)((nown + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, (const double *)e->d_gc, (const double *)e->d_N,
              phi, y);
    count_launch(g, 72.0 * nown + 8.0 * GEOM_NP * q.elems_stored(), (56.0 + 26.0 * 10 + 6) * nown);
    return TP_OK;
}

extern "C" int tp_elasticity_geom_sensitivity(tp_elasticity *e, int ncase, const double *const *Phi, const double *w, const double *xPhys,
                                              const double *U, double Emax, double penal, double scale, double *out) {
    if (!e || !Phi || !xPhys || !U || !out || ncase < 1 || ncase > TP_MAX_CASES) return TP_ERR_ARG;
    if (!geom_par_ok(Emax, penal) || !std::isfinite(scale)) return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!Phi[l]) return TP_ERR_ARG;
    if (!e->have_geom) return TP_ERR_ARG;
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    MassFields a;
    int ndistinct;
    TP_TRY(geom_fields(e, ncase, Phi, w, &a, &ndistinct));
    TP_TRY(halo_nodes(g, q, const_cast<double *>(U), 3));
    const long nel = q.own_elems();
    TP_LAUNCH(k_geom_sens, dim3((int)((nel + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, a, (const double *)e->d_gtab, e->geom_wq, Emax, penal,
              (const double *)e->d_N, xPhys, U, scale, out);
    count_launch(g, 24.0 * nel + 24.0 * q.owned_nodes() * (ndistinct + 2), (8.0 * 240 + (24.0 + 8 * (144 + 30 + 12) + 2) * ncase + 30) * nel);
    return TP_OK;
}

extern "C" int tp_elasticity_geom_adjoint_rhs(tp_elasticity *e, int ncase, const double *const *Phi, const double *w, const double *xPhys,
                                              double Emax, double penal, double scale, double *out) {
    if (!e || !Phi || !xPhys || !out || ncase < 1 || ncase > TP_MAX_CASES) return TP_ERR_ARG;
    if (!geom_par_ok(Emax, penal) || !std::isfinite(scale)) return TP_ERR_ARG;
    for (int l = 0; l < ncase; l++)
        if (!Phi[l] || Phi[l] == out) return TP_ERR_ARG;
    if (!e->have_geom) return TP_ERR_ARG;
    tp_grid *g = e->grid;
    const Geom q = e->mg.lv[0].g;
    const long nst = q.elems_stored(), nown = q.owned_nodes();
    TP_TRY(geom_prepare(e, xPhys));
    if (!e->d_ges) TP_TRY(e->d_ges.alloc((size_t)nst));
    TP_LAUNCH(k_geom_modulus, dim3((int)((nst + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, Emax, penal, xPhys, (const double *)e->d_xg,
              (double *)e->d_ges);
    count_launch(g, 16.0 * nst, 3.0 * nst);
    MassFields a;
    int ndistinct;
    TP_TRY(geom_fields(e, ncase, Phi, w, &a, &ndistinct));
    TP_LAUNCH(k_geom_adjoint_rhs, dim3((int)((nown + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, q, a, (const double *)e->d_gtab, e->geom_wq,
              (const double *)e->d_ges, (const double *)e->d_N, scale, out);
    count_launch(g, 8.0 * nst + (24.0 * (ndistinct + 1) + 24.0) * nown, 8.0 * ((24.0 + 8 * (144 + 30 + 12)) * ncase + 8 * 30 + 8) * nown);
    return TP_OK;
}
#endif
