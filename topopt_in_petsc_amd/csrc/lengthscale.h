// lengthscale.h -- minimum length scale by geometric constraints (Zhou, Lazarov, Wang, Sigmund: "Minimum length scale in topology
// optimization by geometric constraints", CMAME 293 (2015)): one scalar constraint for the solid phase and one for the void
// phase on the filtered field rt = xTilde and the projected field rb = xPhys.  No solve.  Included from topopt_amd.hip behind
// filter.h, whose Heaviside derivative (k_heaviside_chain) it restates.
//
//   e+_a = min(i_a + 1, n_a - 1),  e-_a = max(i_a - 1, 0)   (clamped at the DOMAIN boundary; global count along z)
//   d_{a,e} = rt[e+_a] - rt[e-_a],  G_e = sum_a (d_{a,e} / (2 h_a))^2,  E_e = exp(-c G_e)
//   solid: a = rb,      m = min(rt - eta_s, 0),  a' = H'(rt),   m' = 1
//   void:  a = 1 - rb,  m = min(eta_v - rt, 0),  a' = -H'(rt),  m' = -1
//   T_e = a_e E_e m_e^2,  S = sum_e T_e (all ranks),  g = S / (n eps) - 1             (n: GLOBAL element count)
//   dS/drt_j = a'_j E_j m_j^2 + 2 a_j E_j m_j m'_j + sum_a ( sum_{e: e+_a = j} w_{a,e} - sum_{e: e-_a = j} w_{a,e} ),
//   w_{a,e} = -c T_e d_{a,e} / (2 h_a^2);   e+_a = j: e = j - 1, and e = j on the last index;  e-_a = j: e = j + 1, and e = j on the first
//
// Both kinds in one call: they share d, G and E, and the passes are bandwidth bound.  Every read of a neighbour is a plain cached
// load: a wave reads its x neighbours from the lines it holds anyway, the y and z neighbours are rows another wave of the same or
// the next workgroup streams through the L2 (7 loads, 1 line of HBM traffic per element and field).  No LDS tile, no atomics.
// S is the sum of the layer sums in ascending GLOBAL z on one rank and on many, so g -- and every bit of the gradient, which is
// a gather -- does not depend on the number of slabs.
#pragma once

struct LsGeom {
    int ex, ey, ez_own, e0z, ez_glob;
    long lay;
};
struct LsParams {
    double c, eta_s, eta_v;
    double ihx, ihy, ihz;     // 1 / (2 h_a)
    double wx, wy, wz;        // -c / (2 h_a^2)
    double hp_beta, hp_eta, hp_den;  // H'(rt) = beta (1 - tanh^2(beta (rt - eta))) / den; proj off: beta = 0 marks H' = 1
    double inv_ne;            // 1 / (n eps)
    int kinds;                // 1 solid | 2 void
};

// d_{a,e} of the three axes at element (i, j, k): rt points at own layer 0, ghost layers (two on each side on more than one rank)
// lie below and above it; k is the LOCAL layer, clamped through its global index.
__device__ __forceinline__ void ls_deltas(const LsGeom q, const double *__restrict__ rt, int i, int j, int k, double &dx, double &dy,
                                          double &dz) {
    const int kg = k + q.e0z;
    const long row = (long)q.ex * j + q.lay * k;
    dx = rt[row + min(i + 1, q.ex - 1)] - rt[row + max(i - 1, 0)];
    const long col = i + q.lay * k;
    dy = rt[col + (long)q.ex * min(j + 1, q.ey - 1)] - rt[col + (long)q.ex * max(j - 1, 0)];
    const long pil = i + (long)q.ex * j;
    dz = rt[pil + q.lay * (min(kg + 1, q.ez_glob - 1) - q.e0z)] - rt[pil + q.lay * (max(kg - 1, 0) - q.e0z)];
}
__device__ __forceinline__ double ls_E(const LsParams p, double dx, double dy, double dz) {
    const double qx = dx * p.ihx, qy = dy * p.ihy, qz = dz * p.ihz;
    return exp(-p.c * (qx * qx + qy * qy + qz * qz));
}

// Forward: one thread per own element, a workgroup never straddles a z layer (grid: blocks per layer x own layers).  Ts / Tv point
// at own layer 0 of the ghosted term buffers.  part[kind][layer * blocks-per-layer + block] = the block's sum of T.
__global__ __launch_bounds__(BLK) void k_lengthscale_terms(const LsGeom q, const LsParams p, const double *__restrict__ rt,
                                                           const double *__restrict__ rb, double *__restrict__ Ts,
                                                           double *__restrict__ Tv, double *__restrict__ part) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    const int k = blockIdx.y;
    double ts = 0.0, tv = 0.0;
    if (t < q.lay) {
        const int i = (int)(t % q.ex), j = (int)(t / q.ex);
        const long e = t + q.lay * k;
        double dx, dy, dz;
        ls_deltas(q, rt, i, j, k, dx, dy, dz);
        const double E = ls_E(p, dx, dy, dz), r = rt[e], a = rb[e];
        if (p.kinds & 1) {
            const double m = fmin(r - p.eta_s, 0.0);
            ts = a * E * (m * m);
            Ts[e] = ts;
        }
        if (p.kinds & 2) {
            const double m = fmin(p.eta_v - r, 0.0);
            tv = (1.0 - a) * E * (m * m);
            Tv[e] = tv;
        }
    }
    const double ss = block_sum(ts), sv = block_sum(tv);
    if (threadIdx.x == 0) {
        const long nb = (long)gridDim.x * gridDim.y, b = (long)blockIdx.y * gridDim.x + blockIdx.x;
        part[b] = ss;
        part[nb + b] = sv;
    }
}
// One workgroup per layer and kind: lsum[kind * layers + k] = the sum of layer k's bpl block sums in a fixed order.  The short
// serial pass over the layer sums in ascending global z is the host's (tp_lengthscale_constraints): it holds them anyway.
__global__ __launch_bounds__(BLK) void k_lengthscale_layers(const double *__restrict__ part, int bpl, double *__restrict__ lsum) {
    const int k = blockIdx.x, nl = gridDim.x, kind = blockIdx.y;
    double s = 0.0;
    for (int b = threadIdx.x; b < bpl; b += BLK) s += part[((long)kind * nl + k) * bpl + b];
    s = block_sum(s);
    if (threadIdx.x == 0) lsum[kind * nl + k] = s;
}

// One axis of the stencil term at index x of n: T0 / d0 at the element itself, Tm / dm at x - 1, Tp / dp at x + 1 (read only where
// they exist), w = -c / (2 h^2).  Fixed order: (x - 1), (x on the last index), -(x + 1), -(x on the first index).
__device__ __forceinline__ double ls_axis(int x, int n, double w, double T0, double d0, double Tm, double dm, double Tp, double dp) {
    double s = 0.0;
    if (x > 0) s += w * Tm * dm;
    if (x == n - 1) s += w * T0 * d0;
    if (x < n - 1) s -= w * Tp * dp;
    if (x == 0) s -= w * T0 * d0;
    return s;
}
// Adjoint, a gather: one thread per own element j evaluates dS/drt_j / (n eps) of both kinds from rt (distance <= 2), rb_j and T
// (distance <= 1).  Ts / Tv: own layer 0 of the ghosted term buffers (one ghost layer on each side filled on more than one rank).
__global__ __launch_bounds__(BLK) void k_lengthscale_adjoint(const LsGeom q, const LsParams p, const double *__restrict__ rt,
                                                             const double *__restrict__ rb, const double *__restrict__ Ts,
                                                             const double *__restrict__ Tv, double *__restrict__ dgs,
                                                             double *__restrict__ dgv) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    const int k = blockIdx.y;
    if (t >= q.lay) return;
    const int i = (int)(t % q.ex), j = (int)(t / q.ex), kg = k + q.e0z;
    const long e = t + q.lay * k;
    double dx, dy, dz;
    ls_deltas(q, rt, i, j, k, dx, dy, dz);
    const double E = ls_E(p, dx, dy, dz), r = rt[e], a = rb[e];
    double hp = 1.0;
    if (p.hp_beta != 0.0) {
        const double th = tanh(p.hp_beta * (r - p.hp_eta));
        hp = p.hp_beta * (1.0 - th * th) / p.hp_den;
    }
    // d of the six neighbours along their own axis: the neighbour's e+ is this element or the one behind it
    const long ox = 1, oy = q.ex;
    const double dxm = i > 0 ? r - rt[e - ox * (i - max(i - 2, 0))] : 0.0;
    const double dxp = i < q.ex - 1 ? rt[e + ox * (min(i + 2, q.ex - 1) - i)] - r : 0.0;
    const double dym = j > 0 ? r - rt[e - oy * (j - max(j - 2, 0))] : 0.0;
    const double dyp = j < q.ey - 1 ? rt[e + oy * (min(j + 2, q.ey - 1) - j)] - r : 0.0;
    const double dzm = kg > 0 ? r - rt[e - q.lay * (kg - max(kg - 2, 0))] : 0.0;
    const double dzp = kg < q.ez_glob - 1 ? rt[e + q.lay * (min(kg + 2, q.ez_glob - 1) - kg)] - r : 0.0;
#define TP_LS_KIND(T, OUT, A, AP, M, MP)                                                                                    \
    do {                                                                                                                    \
        const double T0 = T[e];                                                                                             \
        const double Txm = i > 0 ? T[e - ox] : 0.0, Txp = i < q.ex - 1 ? T[e + ox] : 0.0;                                   \
        const double Tym = j > 0 ? T[e - oy] : 0.0, Typ = j < q.ey - 1 ? T[e + oy] : 0.0;                                   \
        const double Tzm = kg > 0 ? T[e - q.lay] : 0.0, Tzp = kg < q.ez_glob - 1 ? T[e + q.lay] : 0.0;                      \
        double s = (AP) * E * ((M) * (M)) + 2.0 * (A) * E * (M) * (MP);                                                     \
        s += ls_axis(i, q.ex, p.wx, T0, dx, Txm, dxm, Txp, dxp);                                                            \
        s += ls_axis(j, q.ey, p.wy, T0, dy, Tym, dym, Typ, dyp);                                                            \
        s += ls_axis(kg, q.ez_glob, p.wz, T0, dz, Tzm, dzm, Tzp, dzp);                                                      \
        OUT[e] = s * p.inv_ne;                                                                                              \
    } while (0)
    if (dgs) {
        const double m = fmin(r - p.eta_s, 0.0);
        TP_LS_KIND(Ts, dgs, a, hp, m, 1.0);
    }
    if (dgv) {
        const double m = fmin(p.eta_v - r, 0.0);
        TP_LS_KIND(Tv, dgv, 1.0 - a, -hp, m, -1.0);
    }
#undef TP_LS_KIND
}

struct tp_lengthscale {
    tp_grid *grid;
    int bpl;
    long nel, lay;
    DevBuf<double> rtg;      // [dev] xTilde with two ghost layers on each side; more than one rank only
    DevBuf<double> Ts, Tv;   // [dev] the terms with one ghost layer on each side
    DevBuf<double> part;     // [dev] 2 * bpl * ez_own block partials of k_lengthscale_terms
    DevBuf<double> lsum;     // [dev] 2 * ez_own layer sums
};

extern "C" int tp_lengthscale_destroy(tp_lengthscale *ls) {
    if (!ls) return TP_OK;
    (void)hipStreamSynchronize(ls->grid->stream);
    delete ls;
    return TP_OK;
}
extern "C" int tp_lengthscale_create(tp_lengthscale **out, tp_grid *g) {
    if (!out || !g) return TP_ERR_ARG;
    if (g->nranks > 1 && g->ez_own < 2) return TP_ERR_ARG;  // the gradient reaches two layers into the neighbour slab
    std::unique_ptr<tp_lengthscale> ls(new tp_lengthscale());
    ls->grid = g;
    ls->lay = (long)g->ex * g->ey;
    ls->nel = ls->lay * g->ez_own;
    ls->bpl = (int)((ls->lay + BLK - 1) / BLK);
    if (g->has_comm) TP_TRY(ls->rtg.alloc_zero((size_t)(g->ez_own + 4) * ls->lay));
    TP_TRY(ls->Ts.alloc_zero((size_t)(g->ez_own + 2) * ls->lay));
    TP_TRY(ls->Tv.alloc_zero((size_t)(g->ez_own + 2) * ls->lay));
    TP_TRY(ls->part.alloc_zero(2 * (size_t)ls->bpl * g->ez_own));
    TP_TRY(ls->lsum.alloc_zero(2 * (size_t)g->ez_own));
    *out = ls.release();
    return TP_OK;
}
// the terms of the last call, own elements (either may be NULL)
extern "C" int tp_lengthscale_get_terms(tp_lengthscale *ls, double *T_solid, double *T_void) {
    if (!ls) return TP_ERR_ARG;
    const size_t nb = sizeof(double) * (size_t)ls->nel;
    if (T_solid) TP_HIP(hipMemcpyAsync(T_solid, ls->Ts + ls->lay, nb, hipMemcpyDeviceToDevice, ls->grid->stream));
    if (T_void) TP_HIP(hipMemcpyAsync(T_void, ls->Tv + ls->lay, nb, hipMemcpyDeviceToDevice, ls->grid->stream));
    return TP_OK;
}
extern "C" int tp_lengthscale_constraints(tp_lengthscale *ls, const double *xTilde, const double *xPhys, int proj, double beta,
                                          double eta, double c, double eta_s, double eta_v, double eps, int kinds, double *g_out,
                                          double *S_out, double *dg_solid, double *dg_void) {
    if (!ls || !xTilde || !xPhys || kinds < 1 || kinds > 3) return TP_ERR_ARG;
    if (!std::isfinite(c) || !std::isfinite(eps) || !std::isfinite(eta_s) || !std::isfinite(eta_v) || !std::isfinite(beta) ||
        !std::isfinite(eta))
        return TP_ERR_ARG;
    if (c < 0.0 || !(eps > 0.0) || !(eta_s > 0.0 && eta_s < 1.0) || !(eta_v > 0.0 && eta_v < 1.0)) return TP_ERR_ARG;
    if (proj && (!(beta > 0.0) || !(eta >= 0.0 && eta <= 1.0))) return TP_ERR_ARG;
    tp_grid *g = ls->grid;
    const int nl = g->ez_own;
    const long lay = ls->lay, nel = ls->nel;
    const double n = (double)(lay * g->ez_glob), hx = g->o.hx, hy = g->o.hy, hz = g->o.hz;
    const LsGeom q = {g->ex, g->ey, nl, g->rank * nl, g->ez_glob, lay};
    LsParams p;
    p.c = c, p.eta_s = eta_s, p.eta_v = eta_v;
    p.ihx = 1.0 / (2.0 * hx), p.ihy = 1.0 / (2.0 * hy), p.ihz = 1.0 / (2.0 * hz);
    p.wx = -c / (2.0 * hx * hx), p.wy = -c / (2.0 * hy * hy), p.wz = -c / (2.0 * hz * hz);
    p.hp_beta = proj ? beta : 0.0, p.hp_eta = eta;
    p.hp_den = proj ? tanh(beta * eta) + tanh(beta * (1.0 - eta)) : 1.0;
    p.inv_ne = 1.0 / (n * eps);
    p.kinds = kinds;
    const double *rt = xTilde;
    if (g->has_comm) {  // two ghost layers of xTilde on each side
        double *own = ls->rtg + 2 * lay;
        TP_HIP(hipMemcpyAsync(own, xTilde, sizeof(double) * (size_t)nel, hipMemcpyDeviceToDevice, g->stream));
        TP_TRY(exchange_segments(g, own, ls->rtg, own + (long)(nl - 2) * lay, own + (long)nl * lay, lay, 2, lay));
        count_launch(g, 16.0 * nel, 0.0);
        rt = own;
    }
    double *Ts = ls->Ts + lay, *Tv = ls->Tv + lay;
    const int nk = (kinds & 1) + ((kinds >> 1) & 1);
    TP_LAUNCH(k_lengthscale_terms, dim3(ls->bpl, nl), dim3(BLK), 0, g->stream, q, p, rt, xPhys, Ts, Tv, ls->part);
    count_launch(g, (16.0 + 8.0 * nk) * nel, (14.0 + 20.0 + 5.0 * nk) * nel);  // differences and G, exp ~ 20, a term and its sum
    TP_LAUNCH(k_lengthscale_layers, dim3(nl, 2), dim3(BLK), 0, g->stream, ls->part, ls->bpl, ls->lsum);
    count_launch(g, 16.0 * ls->bpl * nl, 2.0 * ls->bpl * nl);
    // the one host read; the layer sums of all ranks side by side (grid.h: gather_slots; x + 0 is exact), then S in ascending
    // global z -- the same additions on one rank and on many
    std::vector<double> mine(2 * (size_t)nl), layer((size_t)g->ez_glob);
    TP_HIP(hipMemcpyAsync(mine.data(), ls->lsum, sizeof(double) * mine.size(), hipMemcpyDeviceToHost, g->stream));
    TP_HIP(hipStreamSynchronize(g->stream));
    for (int kind = 0; kind < 2; kind++) {
        if (!(kinds & (1 << kind))) continue;
        if (g->has_comm)
            TP_TRY(gather_slots(g, g->ez_glob, g->rank * nl, nl, mine.data() + (size_t)kind * nl, layer.data()));
        else
            std::memcpy(layer.data(), mine.data() + (size_t)kind * nl, sizeof(double) * (size_t)nl);
        double S = 0.0;
        for (double s : layer) S += s;
        if (S_out) S_out[kind] = S;
        if (g_out) g_out[kind] = S / (n * eps) - 1.0;
    }
    double *ds = (kinds & 1) ? dg_solid : nullptr, *dv = (kinds & 2) ? dg_void : nullptr;
    if (!ds && !dv) return TP_OK;
    // one ghost layer of each term that is differentiated
    if (ds) TP_TRY(exchange_segments(g, Ts, Ts - lay, Ts + (long)(nl - 1) * lay, Ts + (long)nl * lay, lay, 1, lay));
    if (dv) TP_TRY(exchange_segments(g, Tv, Tv - lay, Tv + (long)(nl - 1) * lay, Tv + (long)nl * lay, lay, 1, lay));
    const int nd = (ds ? 1 : 0) + (dv ? 1 : 0);
    TP_LAUNCH(k_lengthscale_adjoint, dim3(ls->bpl, nl), dim3(BLK), 0, g->stream, q, p, rt, xPhys, (const double *)Ts, (const double *)Tv,
              ds, dv);
    count_launch(g, (16.0 + 16.0 * nd) * nel, (14.0 + 20.0 + 20.0 + 6.0 + 40.0 * nd) * nel);  // G, exp, tanh, the six d, ~40 per kind
    return TP_OK;
}
