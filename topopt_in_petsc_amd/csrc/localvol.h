// localvol.h -- local volume constraint (Wu, Aage, Westermann, Sigmund: "Infill optimization for additive manufacturing",
// IEEE TVCG 24 (2018)): the mean density in a ball of radius R around every element, aggregated by a p-norm into ONE
// constraint value and its sensitivity.  Included from topopt_amd.hip behind filter.h, whose convolution it shares.
//
//   N_e = { j : |c_j - c_e| < R }  (strict, truncated at the domain boundary, as the cone filter's neighbourhood)
//   cnt_e = |N_e|,  rb_e = (sum_{j in N_e} rho_j) / cnt_e
//   S = sum_e rb_e^p (all ranks),  pn = (S / n)^(1/p),  g = pn / alpha - 1      (n: GLOBAL element count)
//   dg/drho_j = sum_{e in N_j} c_e,  c_e = t_e^(p-1) / (alpha n cnt_e),  t_e = rb_e / pn <= n^(1/p)   (N is symmetric)
//
// The ball indicator is a 0/1 weight table for conv_apply (filter.h): both ball sums are the cone filter's kernels, launches
// and ghost-layer exchange.  Two streaming kernels of its own sit between them.  No atomics anywhere; S is summed layer by
// layer in ascending GLOBAL z, so the value -- and with it every bit of dgdx -- does not depend on the number of slabs.
#pragma once

// rb -> rb^p: one thread per own element, a workgroup never straddles a z layer (grid: blocks per layer x own layers).
// part[b] = the block's sum of rb^p, part[nb + b] = its max rb, b = layer * blocks-per-layer + block.
__global__ __launch_bounds__(BLK) void k_localvol_pow(const double *__restrict__ rb, long lay, double p, double *__restrict__ part) {
    const long i = blockIdx.x * (long)BLK + threadIdx.x;
    double r = 0.0, v = 0.0;
    if (i < lay) {
        r = rb[(long)blockIdx.y * lay + i];
        v = pow(r, p);
    }
    const double sp = block_sum(v);
    const double mx = block_max(r);  // (fmax drops a NaN; the sum carries it: a NaN density gives pn = NaN)
    if (threadIdx.x == 0) {
        const long nb = (long)gridDim.x * gridDim.y, b = (long)blockIdx.y * gridDim.x + blockIdx.x;
        part[b] = sp;
        part[nb + b] = mx;
    }
}
// One workgroup, fixed order: out[2 + k] = sum of layer k's bpl block sums, out[0] = their sum in ascending k, out[1] = max.
__global__ __launch_bounds__(BLK) void k_localvol_reduce(const double *__restrict__ part, int bpl, int nlayers, double *__restrict__ out) {
    const long nb = (long)bpl * nlayers;
    double tot = 0.0;
    for (int k = 0; k < nlayers; k++) {
        double s = 0.0;
        for (int b = threadIdx.x; b < bpl; b += BLK) s += part[(long)k * bpl + b];
        s = block_sum(s);
        if (threadIdx.x == 0) {
            out[2 + k] = s;
            tot += s;
        }
    }
    double m = 0.0;
    for (long b = threadIdx.x; b < nb; b += BLK) m = fmax(m, part[nb + b]);
    m = block_max(m);
    if (threadIdx.x == 0) {
        out[0] = tot;
        out[1] = m;
    }
}
// Once pn is known: c_e = t_e^(p-1) / (alpha n cnt_e) with t_e = rb_e / pn (no overflow for any p), written straight into
// the own part of the ghosted buffer the second ball sum reads.  pn = 0: c = 0 everywhere.  an = alpha * n.
__global__ __launch_bounds__(BLK) void k_localvol_coef(long nel, const double *__restrict__ rb, const double *__restrict__ cnt,
                                                       double pn, double p, double an, double *__restrict__ xg_own) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= nel) return;
    xg_own[t] = pn != 0.0 ? pow(rb[t] / pn, p - 1.0) / (an * cnt[t]) : 0.0;
}

struct tp_localvol {
    tp_grid *grid;
    int conn, bpl;
    double R;
    long nel, lay;
    DevBuf<double> wtab, xg, cnt, rb;
    DevBuf<double> part;  // [dev] 2 * bpl * ez_own block partials of k_localvol_pow
    DevBuf<double> red;   // [dev] 2 + ez_own: sum, max, layer sums
    int last_kernel = 0;
};

static int localvol_conv(tp_localvol *lv, double *out, const double *d1) {
    const ConvArgs a = {lv->grid, lv->conn, lv->wtab, lv->xg, lv->nel, lv->lay, &lv->last_kernel};
    return conv_apply(&a, out, d1, nullptr);
}
static int localvol_fill(tp_localvol *lv, const double *x) {
    tp_grid *g = lv->grid;
    TP_LAUNCH(k_fill_pw, dim3(grid_for(lv->nel)), dim3(BLK), 0, g->stream, lv->xg + lv->conn * lv->lay, x, (const double *)nullptr, 0,
              lv->nel);
    count_launch(g, 16.0 * lv->nel, 0.0);
    return TP_OK;
}

extern "C" int tp_localvol_destroy(tp_localvol *lv) {
    if (!lv) return TP_OK;
    (void)hipStreamSynchronize(lv->grid->stream);
    delete lv;
    return TP_OK;
}
extern "C" int tp_localvol_create(tp_localvol **out, tp_grid *g, double R) {
    if (!out || !g || !(R > 0.0) || !std::isfinite(R)) return TP_ERR_ARG;
    const double dx = g->o.hx, dy = g->o.hy, dz = g->o.hz;
    // the cone filter's ElemConn and its clamp (tp_filter_create)
    int conn = (int)fmax(ceil(R / dx) - 1, fmax(ceil(R / dy) - 1, ceil(R / dz) - 1));
    conn = std::min(conn, std::min(g->ex / 2, std::min(g->ey / 2, g->ez_glob / 2)));
    if (conn < 0) conn = 0;
    if (g->nranks > 1 && conn > g->ez_own) return TP_ERR_ARG;
    std::unique_ptr<tp_localvol> lv(new tp_localvol());
    lv->grid = g;
    lv->R = R;
    lv->conn = conn;
    lv->lay = (long)g->ex * g->ey;
    lv->nel = lv->lay * g->ez_own;
    lv->bpl = (int)((lv->lay + BLK - 1) / BLK);
    const int w1 = 2 * conn + 1;
    std::vector<double> w((size_t)w1 * w1 * w1);
    for (int dk = -conn; dk <= conn; dk++)
        for (int dj = -conn; dj <= conn; dj++)
            for (int di = -conn; di <= conn; di++) {
                const double dist = sqrt((di * dx) * (di * dx) + (dj * dy) * (dj * dy) + (dk * dz) * (dk * dz));
                w[((size_t)(dk + conn) * w1 + (dj + conn)) * w1 + (di + conn)] = dist < R ? 1.0 : 0.0;  // strict, as filter.h
            }
    const size_t ng = (size_t)(g->ez_own + 2 * conn) * lv->lay;
    TP_TRY(lv->wtab.alloc(w.size()));
    TP_HIP(hipMemcpy(lv->wtab, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
    TP_TRY(lv->xg.alloc(ng));
    TP_TRY(lv->cnt.alloc((size_t)lv->nel));
    TP_TRY(lv->rb.alloc((size_t)lv->nel));
    TP_TRY(lv->part.alloc(2 * (size_t)lv->bpl * g->ez_own));
    TP_TRY(lv->red.alloc((size_t)(2 + g->ez_own)));
    // cnt = ball_sum(1), the way Hs = H * 1 is made
    TP_LAUNCH(k_set, dim3(grid_for((long)ng)), dim3(BLK), 0, g->stream, lv->xg, 1.0, (long)ng);
    TP_TRY(localvol_conv(lv.get(), lv->cnt, nullptr));
    *out = lv.release();
    return TP_OK;
}
extern "C" int tp_localvol_stencil_width(const tp_localvol *lv) { return lv ? lv->conn : -1; }
extern "C" int tp_localvol_last_kernel(const tp_localvol *lv) { return lv ? lv->last_kernel : 0; }
extern "C" int tp_localvol_get_count(tp_localvol *lv, double *cnt) {
    if (!lv || !cnt) return TP_ERR_ARG;
    TP_HIP(hipMemcpyAsync(cnt, lv->cnt, sizeof(double) * (size_t)lv->nel, hipMemcpyDeviceToDevice, lv->grid->stream));
    return TP_OK;
}
extern "C" int tp_localvol_mean(tp_localvol *lv, const double *xPhys, double *rhobar) {
    if (!lv || !xPhys || !rhobar) return TP_ERR_ARG;
    TP_TRY(localvol_fill(lv, xPhys));
    return localvol_conv(lv, rhobar, lv->cnt);
}
extern "C" int tp_localvol_constraint(tp_localvol *lv, const double *xPhys, double alpha, double p, double *g_out, double *pn_out,
                                      double *rhobar_max, double *rhobar, double *dgdx) {
    if (!lv || !xPhys) return TP_ERR_ARG;
    if (!(p >= 1.0) || !std::isfinite(p) || !(alpha > 0.0) || !std::isfinite(alpha)) return TP_ERR_ARG;
    tp_grid *g = lv->grid;
    const long nel = lv->nel;
    const int nl = g->ez_own;
    double *rb = rhobar ? rhobar : lv->rb;
    TP_TRY(localvol_fill(lv, xPhys));
    TP_TRY(localvol_conv(lv, rb, lv->cnt));
    TP_LAUNCH(k_localvol_pow, dim3(lv->bpl, nl), dim3(BLK), 0, g->stream, rb, lv->lay, p, lv->part);
    count_launch(g, 8.0 * nel, 1.0 * nel);
    TP_LAUNCH(k_localvol_reduce, dim3(1), dim3(BLK), 0, g->stream, lv->part, lv->bpl, nl, lv->red);
    count_launch(g);
    double S, mx;
    if (!g->has_comm) {  // the one host read
        TP_HIP(hipMemcpyAsync(g->h_scal, lv->red, sizeof(double) * 2, hipMemcpyDeviceToHost, g->stream));
        TP_HIP(hipStreamSynchronize(g->stream));
        S = g->h_scal[0];
        mx = g->h_scal[1];
    } else {
        // Layer sums of all ranks side by side (grid.h: gather_slots; x + 0 is exact), then S in ascending global z -- the order
        // k_localvol_reduce has on one rank.  The maximum: rank_max.
        std::vector<double> mine((size_t)(2 + nl)), layer((size_t)g->ez_glob);
        TP_HIP(hipMemcpyAsync(mine.data(), lv->red, sizeof(double) * mine.size(), hipMemcpyDeviceToHost, g->stream));
        TP_HIP(hipStreamSynchronize(g->stream));
        TP_TRY(gather_slots(g, g->ez_glob, g->rank * nl, nl, mine.data() + 2, layer.data()));
        S = 0.0;
        for (double s : layer) S += s;
        mx = mine[1];
        TP_TRY(rank_max(g, &mx));
    }
    const double n = (double)((long)g->ex * g->ey * g->ez_glob);
    const double pn = S != 0.0 ? pow(S / n, 1.0 / p) : 0.0;
    if (pn_out) *pn_out = pn;
    if (g_out) *g_out = pn / alpha - 1.0;
    if (rhobar_max) *rhobar_max = mx;
    if (!dgdx) return TP_OK;
    TP_LAUNCH(k_localvol_coef, dim3((int)((nel + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, nel, rb, lv->cnt, pn, p, alpha * n,
              lv->xg + lv->conn * lv->lay);
    count_launch(g, 24.0 * nel, 3.0 * nel);
    return localvol_conv(lv, dgdx, nullptr);
}
