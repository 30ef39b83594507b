// overhang.h -- overhang (self-support) filter for additive manufacturing: Langelaar, "An additive manufacturing filter for
// topology optimization of print-ready designs", Struct. Multidisc. Optim. 55 (2017), 3-D form of "Topology optimization of
// 3D self-supporting structures for additive manufacturing", Additive Manufacturing 12 (2016).  Included from topopt_amd.hip
// behind grid.h.  DESIGN.md 4.11.
//
// Build axis a in {y, z}, sign +-; layer 0 lies on the baseplate (lowest index for +, highest for -); in-plane (i, r) = x and
// the remaining axis.  Q = P + ln 5 / ln xi0.  Forward, bottom-up:
//   xi_0 = x_0;  l >= 1:  t = p * xi of layer l-1 with p = xi^(P-1),
//   S = t(i,r) + t(i-1,r) + t(i+1,r) + t(i,r-1) + t(i,r+1)   (left to right; outside the mesh: 0),
//   Xi = S^(1/Q) (0 if S < S_MIN),  d = x - Xi,  rho = sqrt(d^2 + eps),  xi = (x + Xi - rho + sqrt(eps)) / 2,
//   a = (1 - d/rho)/2,  w = (1 + d/rho)/2 * (P/Q) * Xi/S (0 if S < S_MIN),  p = xi^(P-1);  layer 0: a = 1, w = 0.
// S_MIN = 2^-960: a support sum below it counts as no support.  Xi / S = S^(1/Q - 1) alone leaves the exponent range long before
// the Jacobian entry p w does (P = 40: S < 4e-317, a supporting xi near 1e-8, gives w = inf; S underflown to 0 loses the term):
// with the floor Xi / S <= 2^960 for every admissible Q >= 1, and p of the supporting cell stays normal.  The price is a jump of
// S_MIN^(1/Q) in Xi, 2e-8 at the defaults; S >= S_MIN keeps its bits.
// Transpose, top-down, in place:  lambda_l = g_l + p_l * sum_5 (w lambda)_{l+1} over the same cross in the same order,
//   out_l = a_l lambda_l  (top layer: the sum is 0).  A gather: no atomics, no pow.
//
// Both sweeps advance C layers per launch (TP_OVERHANG_CHUNK): a workgroup owns a 32 x 8 in-plane tile, reads the layer
// before its chunk over the tile widened by the chunk length and carries the widening down by one per layer in two
// ping-pong LDS planes; it stores its own tile only.  The redundant rim cells go through the same two per-cell functions on
// the same values, so every C gives the same bits.  No grid-wide barrier, no persistent kernel.
#pragma once

constexpr int OV_TX = 32, OV_TR = 8;  // own tile: x (the unit-stride lane direction) by the other in-plane axis
constexpr int OV_MAXVEC = 8;
constexpr int OV_LDS_CAP = 65536;     // bytes of LDS one transpose launch may ask for (the static limit; no attribute to raise)
constexpr double OV_S_MIN = 0x1p-960; // support sums below this count as none (head of the file)

struct OvPar {
    double Pm1, invQ, PoverQ, eps, sqeps;
};
// element (i, r, layer l) sits at base + i + r * sR + l * sL.  z build: sR = ex, sL = +-ex*ey; y build: sR = ex*ey, sL = +-ex.
struct OvGeom {
    int ni, nr, nl;
    long sR, sL, base;
};
struct OvVecs {
    double *v[OV_MAXVEC];
};

// ---- the two per-cell functions: every instantiation, every rank count and the rim cells call these ----
__device__ __forceinline__ void ov_cell_fwd(double x, double t0, double t1, double t2, double t3, double t4, const OvPar &par,
                                            double &xi, double &a, double &w, double &p, double &t) {
#pragma clang fp contract(off)
    const double S = (((t0 + t1) + t2) + t3) + t4;
    double Xi = 0.0, sw = 0.0;
    if (S >= OV_S_MIN) {
        Xi = pow(S, par.invQ);
        sw = par.PoverQ * (Xi / S);
    }
    const double d = x - Xi;
    const double rho = sqrt(d * d + par.eps);
    xi = 0.5 * (((x + Xi) - rho) + par.sqeps);
    const double q = d / rho;
    a = 0.5 * (1.0 - q);
    w = (0.5 * (1.0 + q)) * sw;
    p = pow(xi, par.Pm1);
    t = p * xi;
}
__device__ __forceinline__ void ov_cell_adj(double g, double p, double a, double w, double m0, double m1, double m2, double m3,
                                            double m4, double &out, double &m) {
#pragma clang fp contract(off)
    const double s = (((m0 + m1) + m2) + m3) + m4;
    const double lam = g + p * s;
    out = a * lam;
    m = w * lam;
}

// layer 0 of the sweep on the rank that holds the baseplate: xi = x, a = 1, w = 0, p = x^(P-1)
__global__ __launch_bounds__(BLK) void k_overhang_first(OvGeom q, double Pm1, const double *__restrict__ x, double *__restrict__ xi,
                                                        double *__restrict__ ca, double *__restrict__ cw, double *__restrict__ cp) {
    const long e = blockIdx.x * (long)BLK + threadIdx.x;
    if (e >= (long)q.ni * q.nr) return;
    const long o = q.base + e % q.ni + (e / q.ni) * q.sR;
    const double v = x[o];
    xi[o] = v;
    ca[o] = 1.0;
    cw[o] = 0.0;
    cp[o] = pow(v, Pm1);
}
// the ghost layer received from the rank before this one in the sweep: p = xi^(P-1), formed here as the sender formed it
__global__ __launch_bounds__(BLK) void k_overhang_ghost(long n, double Pm1, const double *__restrict__ xig, double *__restrict__ pg) {
    const long e = blockIdx.x * (long)BLK + threadIdx.x;
    if (e < n) pg[e] = pow(xig[e], Pm1);
}

// Layers l0 .. l0 + n - 1 (1 <= n <= C) of the forward sweep.  (xi_prev, p_prev): layer l0 - 1 at i + r * prev_sR -- the own
// arrays or the ghost layer; they may alias xi / cp (other layers), hence no __restrict__ on those.
template <int C>
__global__ __launch_bounds__(BLK) void k_overhang_fwd(OvGeom q, OvPar par, int l0, int n, const double *__restrict__ x, double *xi,
                                                      double *__restrict__ ca, double *__restrict__ cw, double *cp,
                                                      const double *xi_prev, const double *p_prev, long prev_sR) {
    constexpr int PW = OV_TX + 2 * C, PH = OV_TR + 2 * C;
    __shared__ double tpl[2][PH * PW];
    const int i0 = blockIdx.x * OV_TX - C, r0 = blockIdx.y * OV_TR - C;  // mesh coordinates of the plane's origin
    {
        const int wd = OV_TX + 2 * n, cells = wd * (OV_TR + 2 * n);
        for (int e = threadIdx.x; e < cells; e += BLK) {
            const int pi = C - n + e % wd, pr = C - n + e / wd;
            const int i = i0 + pi, r = r0 + pr;
            double v = 0.0;
            if (i >= 0 && i < q.ni && r >= 0 && r < q.nr) {
                const long o = i + r * prev_sR;
                v = p_prev[o] * xi_prev[o];
            }
            tpl[0][pr * PW + pi] = v;
        }
    }
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < n; k++) {
        const int h = n - 1 - k;  // widening of this layer: its rim feeds the layers above, the last layer has none
        const int wd = OV_TX + 2 * h, cells = wd * (OV_TR + 2 * h);
        const long lo = q.base + (long)(l0 + k) * q.sL;
        const double *T = tpl[cur];
        for (int e = threadIdx.x; e < cells; e += BLK) {
            const int pi = C - h + e % wd, pr = C - h + e / wd;  // 1 <= pi <= PW - 2, 1 <= pr <= PH - 2 as h <= C - 1
            const int i = i0 + pi, r = r0 + pr, c = pr * PW + pi;
            double tn = 0.0;
            if (i >= 0 && i < q.ni && r >= 0 && r < q.nr) {
                const long o = lo + i + r * q.sR;
                double xv, av, wv, pv;
                ov_cell_fwd(x[o], T[c], T[c - 1], T[c + 1], T[c - PW], T[c + PW], par, xv, av, wv, pv, tn);
                if (pi >= C && pi < C + OV_TX && pr >= C && pr < C + OV_TR) {
                    xi[o] = xv;
                    ca[o] = av;
                    cw[o] = wv;
                    cp[o] = pv;
                }
            }
            if (k + 1 < n) tpl[cur ^ 1][c] = tn;
        }
        __syncthreads();
        cur ^= 1;
    }
}

// Layers lt, lt - 1, .., lt - n + 1 (1 <= n <= C) of the transpose for nv vectors.  m_in: (w lambda) of layer lt + 1 at
// v * ni * nr + i + r * ni, m_out receives that of layer lt - n + 1.  gin == gout only for C = 1: a wider chunk reads g on
// its rim, inside other workgroups' tiles, so it must not overwrite g during the launch.
template <int C>
__global__ __launch_bounds__(BLK) void k_overhang_adj(OvGeom q, int lt, int n, int nv, OvVecs gin, OvVecs gout,
                                                      const double *__restrict__ ca, const double *__restrict__ cw,
                                                      const double *__restrict__ cp, const double *__restrict__ m_in,
                                                      double *__restrict__ m_out) {
    constexpr int PW = OV_TX + 2 * C, PH = OV_TR + 2 * C, PP = PW * PH;
    extern __shared__ double mpl[];  // [2][nv][PP]
    const int i0 = blockIdx.x * OV_TX - C, r0 = blockIdx.y * OV_TR - C;
    const long pl = (long)q.ni * q.nr;
    {
        const int wd = OV_TX + 2 * n, cells = wd * (OV_TR + 2 * n);
        for (int e = threadIdx.x; e < cells; e += BLK) {
            const int pi = C - n + e % wd, pr = C - n + e / wd;
            const int i = i0 + pi, r = r0 + pr;
            const bool in = i >= 0 && i < q.ni && r >= 0 && r < q.nr;
            for (int v = 0; v < nv; v++) mpl[v * PP + pr * PW + pi] = in ? m_in[v * pl + i + (long)r * q.ni] : 0.0;
        }
    }
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < n; k++) {
        const int h = n - 1 - k;
        const int wd = OV_TX + 2 * h, cells = wd * (OV_TR + 2 * h);
        const long lo = q.base + (long)(lt - k) * q.sL;
        const bool last = k + 1 == n;
        for (int e = threadIdx.x; e < cells; e += BLK) {
            const int pi = C - h + e % wd, pr = C - h + e / wd;
            const int i = i0 + pi, r = r0 + pr, c = pr * PW + pi;
            if (i >= 0 && i < q.ni && r >= 0 && r < q.nr) {
                const long o = lo + i + r * q.sR;
                const double pv = cp[o], av = ca[o], wv = cw[o];  // once per cell, for all vectors
                const bool own = pi >= C && pi < C + OV_TX && pr >= C && pr < C + OV_TR;
                for (int v = 0; v < nv; v++) {
                    const double *M = mpl + (cur * nv + v) * PP;
                    double out, mn;
                    ov_cell_adj(gin.v[v][o], pv, av, wv, M[c], M[c - 1], M[c + 1], M[c - PW], M[c + PW], out, mn);
                    if (!last) mpl[((cur ^ 1) * nv + v) * PP + c] = mn;
                    if (own) {
                        gout.v[v][o] = out;
                        if (last) m_out[v * pl + i + (long)r * q.ni] = mn;
                    }
                }
            } else if (!last) {
                for (int v = 0; v < nv; v++) mpl[((cur ^ 1) * nv + v) * PP + c] = 0.0;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

struct tp_overhang {
    tp_grid *grid;
    int axis, sign;
    int have_fwd, last_chunk;
    double P, eps, xi0, Q;
    OvGeom q;
    long nel, pl;
    DevBuf<double> ca, cw, cp;   // [dev, own elements] coefficients of the last forward sweep
    DevBuf<double> xig, pg;      // [dev, one layer] ghost layer of xi and its p (slabs)
    DevBuf<double> medge[2];     // [dev, OV_MAXVEC layers] (w lambda) of the layer a transpose launch ended on, ping-pong
    DevBuf<double> scratch;      // [dev, scratch_nv * own elements] out-of-place target of the transpose at C > 1, made on first use
    int scratch_nv;
};

static bool overhang_params_ok(double P, double eps, double xi0) {
    if (!std::isfinite(P) || !std::isfinite(eps) || !std::isfinite(xi0)) return false;
    if (!(P >= 1.0) || !(eps > 0.0) || !(xi0 > 0.0 && xi0 < 1.0)) return false;
    return P + log(5.0) / log(xi0) >= 1.0;
}
static OvPar overhang_par(const tp_overhang *ov) {
    OvPar par;
    par.Pm1 = ov->P - 1.0;
    par.invQ = 1.0 / ov->Q;
    par.PoverQ = ov->P / ov->Q;
    par.eps = ov->eps;
    par.sqeps = sqrt(ov->eps);
    return par;
}
// position of this rank in the forward sweep (0 holds the baseplate)
static int overhang_pos(const tp_overhang *ov) { return ov->sign > 0 ? ov->grid->rank : ov->grid->nranks - 1 - ov->grid->rank; }

extern "C" int tp_overhang_destroy(tp_overhang *ov) {
    if (!ov) return TP_OK;
    (void)hipStreamSynchronize(ov->grid->stream);
    delete ov;
    return TP_OK;
}
extern "C" int tp_overhang_set_params(tp_overhang *ov, double P, double eps, double xi0) {
    if (!ov || !overhang_params_ok(P, eps, xi0)) return TP_ERR_ARG;
    ov->P = P;
    ov->eps = eps;
    ov->xi0 = xi0;
    ov->Q = P + log(5.0) / log(xi0);
    ov->have_fwd = 0;  // the stored coefficients belong to the former parameters
    return TP_OK;
}
extern "C" int tp_overhang_create(tp_overhang **out, tp_grid *g, int axis, int sign) {
    if (!out || !g || (axis != 1 && axis != 2) || (sign != 1 && sign != -1)) return TP_ERR_ARG;
    if (g->nranks > 1 && axis != 2) return TP_ERR_ARG;  // the in-plane neighbours of a y build cross the slab border in every layer
    std::unique_ptr<tp_overhang> ov(new tp_overhang());
    ov->grid = g;
    ov->axis = axis;
    ov->sign = sign;
    (void)tp_overhang_set_params(ov.get(), 40.0, 1e-4, 0.5);
    const long lay = (long)g->ex * g->ey;
    OvGeom &q = ov->q;
    q.ni = g->ex;
    q.nr = axis == 2 ? g->ey : g->ez_own;
    q.nl = axis == 2 ? g->ez_own : g->ey;
    q.sR = axis == 2 ? g->ex : lay;
    const long sl = axis == 2 ? lay : g->ex;
    q.sL = sign > 0 ? sl : -sl;
    q.base = sign > 0 ? 0 : (q.nl - 1) * sl;
    ov->nel = lay * g->ez_own;
    ov->pl = (long)q.ni * q.nr;
    for (DevBuf<double> *p : {&ov->ca, &ov->cw, &ov->cp}) TP_TRY(p->alloc((size_t)ov->nel));
    for (DevBuf<double> *p : {&ov->xig, &ov->pg}) TP_TRY(p->alloc((size_t)ov->pl));
    for (DevBuf<double> *p : {&ov->medge[0], &ov->medge[1]}) TP_TRY(p->alloc((size_t)ov->pl * OV_MAXVEC));
    *out = ov.release();
    return TP_OK;
}
extern "C" int tp_overhang_last_chunk(const tp_overhang *ov) { return ov ? ov->last_chunk : 0; }
// read-only copies of the coefficients the last forward sweep left for the transpose (own elements); each may be NULL
extern "C" int tp_overhang_get_coefficients(tp_overhang *ov, double *a, double *w, double *p) {
    if (!ov || !ov->have_fwd) return TP_ERR_ARG;
    const size_t nb = sizeof(double) * (size_t)ov->nel;
    if (a) TP_HIP(hipMemcpyAsync(a, ov->ca, nb, hipMemcpyDeviceToDevice, ov->grid->stream));
    if (w) TP_HIP(hipMemcpyAsync(w, ov->cw, nb, hipMemcpyDeviceToDevice, ov->grid->stream));
    if (p) TP_HIP(hipMemcpyAsync(p, ov->cp, nb, hipMemcpyDeviceToDevice, ov->grid->stream));
    return TP_OK;
}

template <int C>
static int overhang_sweep_fwd(tp_overhang *ov, const double *x, double *xi, bool first) {
    tp_grid *g = ov->grid;
    const OvGeom &q = ov->q;
    const OvPar par = overhang_par(ov);
    const int nb = (int)((ov->pl + BLK - 1) / BLK);
    int l0 = 0;
    if (first) {
        TP_LAUNCH(k_overhang_first, dim3(nb), dim3(BLK), 0, g->stream, q, par.Pm1, x, xi, ov->ca, ov->cw, ov->cp);
        count_launch(g, 40.0 * ov->pl, 0.0);
        l0 = 1;
    } else {
        TP_LAUNCH(k_overhang_ghost, dim3(nb), dim3(BLK), 0, g->stream, ov->pl, par.Pm1, (const double *)ov->xig, ov->pg);
        count_launch(g, 16.0 * ov->pl, 0.0);
    }
    const dim3 tiles((q.ni + OV_TX - 1) / OV_TX, (q.nr + OV_TR - 1) / OV_TR);
    for (; l0 < q.nl; l0 += C) {
        const int n = q.nl - l0 < C ? q.nl - l0 : C;
        const long po = q.base + (long)(l0 - 1) * q.sL;  // (unused for the ghost layer)
        const double *xp = l0 == 0 ? ov->xig : xi + po, *pp = l0 == 0 ? ov->pg : ov->cp + po;
        TP_LAUNCH(k_overhang_fwd<C>, tiles, dim3(BLK), 0, g->stream, q, par, l0, n, x, xi, ov->ca, ov->cw, ov->cp, xp, pp,
                  l0 == 0 ? (long)q.ni : q.sR);
        count_launch(g, (40.0 * n + 16.0) * ov->pl, 0.0);
    }
    return TP_OK;
}
template <int C>
static int overhang_sweep_adj(tp_overhang *ov, int nv, double *const *gv, bool top) {
    tp_grid *g = ov->grid;
    const OvGeom &q = ov->q;
    OvVecs gin, gout;
    for (int v = 0; v < OV_MAXVEC; v++) {
        gin.v[v] = v < nv ? gv[v] : nullptr;
        gout.v[v] = v < nv ? (C == 1 ? gv[v] : ov->scratch + (long)v * ov->nel) : nullptr;
    }
    if (top) TP_HIP(hipMemsetAsync(ov->medge[0], 0, sizeof(double) * (size_t)nv * ov->pl, g->stream));
    const dim3 tiles((q.ni + OV_TX - 1) / OV_TX, (q.nr + OV_TR - 1) / OV_TR);
    const size_t lds = sizeof(double) * 2 * (size_t)nv * (OV_TX + 2 * C) * (OV_TR + 2 * C);
    int cur = 0;
    for (int lt = q.nl - 1; lt >= 0; lt -= C) {
        const int n = lt + 1 < C ? lt + 1 : C;
        TP_LAUNCH(k_overhang_adj<C>, tiles, dim3(BLK), lds, g->stream, q, lt, n, nv, gin, gout, (const double *)ov->ca,
                  (const double *)ov->cw, (const double *)ov->cp, (const double *)ov->medge[cur], ov->medge[cur ^ 1]);
        count_launch(g, (24.0 + 16.0 * nv) * n * ov->pl, 0.0);
        cur ^= 1;
    }
    if (C > 1)
        for (int v = 0; v < nv; v++)
            TP_HIP(hipMemcpyAsync(gv[v], gout.v[v], sizeof(double) * (size_t)ov->nel, hipMemcpyDeviceToDevice, g->stream));
    return TP_OK;
}
// vectors one transpose launch carries: its two planes per vector within OV_LDS_CAP (8 at C <= 2, 6 at C = 4, 3 at C = 8)
static int overhang_group(int C) {
    const int g = (int)(OV_LDS_CAP / (sizeof(double) * 2 * (OV_TX + 2 * C) * (OV_TR + 2 * C)));
    return g < OV_MAXVEC ? g : OV_MAXVEC;
}

extern "C" int tp_overhang_forward(tp_overhang *ov, const double *x, double *xi) {
    if (!ov || !x || !xi || x == xi) return TP_ERR_ARG;
    tp_grid *g = ov->grid;
    const int C = sw_overhang_chunk(), N = g->nranks, pos = overhang_pos(ov);
    // the recursion runs along the slab axis: the ranks sweep one after the other, the finished rank's outermost own layer of
    // xi becoming the next one's ghost layer.  Every rank joins every exchange; what it receives out of turn is overwritten.
    double *edge = xi + ov->q.base + (long)(ov->q.nl - 1) * ov->q.sL;
    for (int turn = 0; turn < N; turn++) {
        if (turn == pos) {
            switch (C) {
                case 1: TP_TRY(overhang_sweep_fwd<1>(ov, x, xi, pos == 0)); break;
                case 2: TP_TRY(overhang_sweep_fwd<2>(ov, x, xi, pos == 0)); break;
                case 4: TP_TRY(overhang_sweep_fwd<4>(ov, x, xi, pos == 0)); break;
                default: TP_TRY(overhang_sweep_fwd<8>(ov, x, xi, pos == 0)); break;
            }
        }
        if (turn < N - 1) {
            if (ov->sign > 0)
                TP_TRY(exchange_segments(g, nullptr, ov->xig, edge, nullptr, ov->pl, 1, ov->pl));
            else
                TP_TRY(exchange_segments(g, edge, nullptr, nullptr, ov->xig, ov->pl, 1, ov->pl));
        }
    }
    ov->have_fwd = 1;
    ov->last_chunk = C;
    return TP_OK;
}
extern "C" int tp_overhang_adjoint(tp_overhang *ov, int nvec, double *const *gv) {
    if (!ov || !gv || nvec < 1 || nvec > OV_MAXVEC) return TP_ERR_ARG;
    for (int v = 0; v < nvec; v++)
        if (!gv[v]) return TP_ERR_ARG;
    if (!ov->have_fwd) return TP_ERR_ARG;
    tp_grid *g = ov->grid;
    const int C = sw_overhang_chunk(), N = g->nranks, apos = N - 1 - overhang_pos(ov), G = overhang_group(C);
    if (C > 1 && ov->scratch_nv < (nvec < G ? nvec : G)) {
        TP_HIP(hipStreamSynchronize(g->stream));
        ov->scratch_nv = 0;
        TP_TRY(ov->scratch.alloc((size_t)(nvec < G ? nvec : G) * ov->nel));
        ov->scratch_nv = nvec < G ? nvec : G;
    }
    const int nchunks = (ov->q.nl + C - 1) / C;
    for (int v0 = 0; v0 < nvec; v0 += G) {
        const int nv = nvec - v0 < G ? nvec - v0 : G;
        // the other way round: each rank hands (w lambda) of its first own layer to the rank before it in the forward sweep
        for (int turn = 0; turn < N; turn++) {
            if (turn == apos) {
                switch (C) {
                    case 1: TP_TRY(overhang_sweep_adj<1>(ov, nv, gv + v0, apos == 0)); break;
                    case 2: TP_TRY(overhang_sweep_adj<2>(ov, nv, gv + v0, apos == 0)); break;
                    case 4: TP_TRY(overhang_sweep_adj<4>(ov, nv, gv + v0, apos == 0)); break;
                    default: TP_TRY(overhang_sweep_adj<8>(ov, nv, gv + v0, apos == 0)); break;
                }
            }
            if (turn < N - 1) {
                const double *fin = ov->medge[nchunks & 1];  // where a sweep of nchunks launches from medge[0] ends
                if (ov->sign > 0)
                    TP_TRY(exchange_segments(g, fin, nullptr, nullptr, ov->medge[0], ov->pl, nv, ov->pl));
                else
                    TP_TRY(exchange_segments(g, nullptr, ov->medge[0], fin, nullptr, ov->pl, nv, ov->pl));
            }
        }
    }
    ov->last_chunk = C;
    return TP_OK;
}
