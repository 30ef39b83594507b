// casting.h -- casting (draw-direction) filter: along the draw axis a cast, moulded or forged part has no undercut and no
// enclosed cavity.  Included from topopt_amd.hip behind grid.h.  DESIGN.md 4.20.
//
// Draw axis a in {x, y, z} with n global element layers k = 0 .. n-1, parting index p in [0, n]: the cells k >= p (upper die,
// withdrawn towards +a) are made non-increasing in k, the cells k < p (lower die) non-decreasing.  Forward, upper range, from
// k = n-1 down to p (the lower range is the mirror image from k = 0 up to p-1):
//   c_{n-1} = x_{n-1}, q_{n-1} = 1;   d = x_k - c_{k+1},  rho = sqrt(d*d + eps),  c_k = 0.5 * ((x_k + c_{k+1}) + rho),  q_k = d / rho.
// Transpose, in place, against the sweep, upper range k = p .. n-1:
//   mu_p = g_p;   out_k = (0.5 * (1 + q_k)) * mu_k,   mu_{k+1} = g_{k+1} + (0.5 * (1 - q_k)) * mu_k.
// No in-plane neighbours: every line of cells along the draw axis is independent of every other one.
//
// Three kernel forms, all through the two per-cell functions:
//   1  walk: one thread per line, lanes along x, the thread steps through its range with the layer stride (y and z draws);
//   2  LDS-staged x draw: the lines ARE the unit-stride runs, so a workgroup of CX_LINES lines moves along x in tiles of CX_TX
//      cells that go through LDS: coalesced rows in, one thread per line over the tile's columns, coalesced rows out;
//   3  the walk kernel on x lines (line stride ex, cell stride 1): TP_CASTING_XFORM=0, the comparison of form 2.
// Where a carry leaves a kernel's reach -- a tile edge of form 2, a slab border of a z draw -- the transpose hands on
// t = 0.0 + (0.5 * (1 - q)) * mu, cast_cell_adj with g_next = 0.0, and the receiver forms mu = g + t: the same two roundings in
// the same order as g_next + (0.5 * (1 - q)) * mu in one piece, so the values are those of an unbroken walk.
#pragma once

constexpr int CAST_MAXVEC = 8;
constexpr int CAST_BLK = 64;    // walk kernels: one wave per workgroup, so 16 384 lines spread over 256 CUs
constexpr int CAST_AHEAD = 4;   // layers the walk kernels load ahead of the recurrence
constexpr int CX_LINES = 64;    // form 2: lines of a workgroup, one thread each
constexpr int CX_TX = 32;       // cells of a tile along x: rows of 256 B
constexpr int CX_PITCH = CX_TX + 1;   // odd row pitch in doubles: the 32 lanes of a half walk one column on 32 distinct 8-byte banks
constexpr int CX_ROWS = CX_LINES * CX_TX / CAST_BLK;   // tile rows a thread stages: 32

// line (i, r), i < ni, r < nr, has its cell k at i * sI + r * sR + k * sL; the line's number i + r * ni indexes the carry arrays
struct CastGeom {
    int ni, nr;
    long sI, sR, sL;
};
// cells lo .. hi-1 of every line, walked upwards (step +1, from lo) or downwards (step -1, from hi-1); carry: the walk goes on
// from a value handed in, it does not start here; emit: the transpose writes what it hands on
struct CastRange {
    int lo, hi, step, carry, emit;
};
struct CastRanges {
    CastRange r[2];
};
struct CastVecs {
    double *v[CAST_MAXVEC];
};

// ---- the two per-cell functions: every kernel form, axis and rank count calls these ----
__device__ __forceinline__ void cast_cell_fwd(double x, double c_prev, double eps, double &c, double &q) {
#pragma clang fp contract(off)
    const double d = x - c_prev;
    const double rho = sqrt(d * d + eps);
    c = 0.5 * ((x + c_prev) + rho);
    q = d / rho;
}
__device__ __forceinline__ void cast_cell_adj(double g_next, double q, double mu, double &out, double &mu_next) {
#pragma clang fp contract(off)
    out = (0.5 * (1.0 + q)) * mu;
    mu_next = g_next + (0.5 * (1.0 - q)) * mu;
}

// ---- form 1 (and 3): the walk ----
// blockIdx.y picks the range; cin: c of the cell before the range's first one, per line (read if carry)
__global__ __launch_bounds__(CAST_BLK) void k_cast_walk_fwd(CastGeom q, CastRanges rs, double eps, const double *__restrict__ x,
                                                            double *__restrict__ c, double *__restrict__ cq,
                                                            const double *__restrict__ cin0, const double *__restrict__ cin1) {
    const CastRange R = rs.r[blockIdx.y];
    const double *cin = blockIdx.y ? cin1 : cin0;
    const long e = blockIdx.x * (long)CAST_BLK + threadIdx.x;
    const int m = R.hi - R.lo;
    if (e >= (long)q.ni * q.nr || m <= 0) return;
    const long st = R.step * q.sL;
    const long o = (e % q.ni) * q.sI + (e / q.ni) * q.sR + (long)(R.step > 0 ? R.lo : R.hi - 1) * q.sL;
    double xb[CAST_AHEAD];
#pragma unroll
    for (int d = 0; d < CAST_AHEAD; d++) xb[d] = x[o + min(d, m - 1) * st];   // (clamped, not predicated: past the end a value nobody reads)
    double cp = R.carry ? cin[e] : 0.0;
    for (int j0 = 0; j0 < m; j0 += CAST_AHEAD) {
#pragma unroll
        for (int d = 0; d < CAST_AHEAD; d++) {
            const int j = j0 + d;
            if (j < m) {
                const double xv = xb[d];
                xb[d] = x[o + min(j + CAST_AHEAD, m - 1) * st];
                double cv = xv, qv = 1.0;
                if (j > 0 || R.carry) cast_cell_fwd(xv, cp, eps, cv, qv);
                c[o + j * st] = cv;
                cq[o + j * st] = qv;
                cp = cv;
            }
        }
    }
}
// g[v] <- J^T g[v] on the range, in place.  tin / tout: [NV][lines] of the hand-over value t (see the head of the file)
template <int NV>
__global__ __launch_bounds__(CAST_BLK) void k_cast_walk_adj(CastGeom q, CastRanges rs, CastVecs g, const double *__restrict__ cq,
                                                            const double *__restrict__ tin0, const double *__restrict__ tin1,
                                                            double *__restrict__ tout0, double *__restrict__ tout1) {
    const CastRange R = rs.r[blockIdx.y];
    const double *tin = blockIdx.y ? tin1 : tin0;
    double *tout = blockIdx.y ? tout1 : tout0;
    const long nl = (long)q.ni * q.nr;
    const long e = blockIdx.x * (long)CAST_BLK + threadIdx.x;
    const int m = R.hi - R.lo;
    if (e >= nl || m <= 0) return;
    const long st = R.step * q.sL;
    const long o = (e % q.ni) * q.sI + (e / q.ni) * q.sR + (long)(R.step > 0 ? R.lo : R.hi - 1) * q.sL;
    // q of the cells j .. j + AHEAD - 1 and g of the cells j + 1 .. j + AHEAD wait in registers
    double qb[CAST_AHEAD], gb[CAST_AHEAD][NV], mu[NV];
#pragma unroll
    for (int d = 0; d < CAST_AHEAD; d++) {
        qb[d] = cq[o + min(d, m - 1) * st];
#pragma unroll
        for (int v = 0; v < NV; v++) gb[d][v] = g.v[v][o + min(d + 1, m - 1) * st];
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const double g0 = g.v[v][o];
        mu[v] = R.carry ? g0 + tin[v * nl + e] : g0;
    }
    for (int j0 = 0; j0 < m; j0 += CAST_AHEAD) {
#pragma unroll
        for (int d = 0; d < CAST_AHEAD; d++) {
            const int j = j0 + d;
            if (j < m) {
                const double qv = qb[d];
                qb[d] = cq[o + min(j + CAST_AHEAD, m - 1) * st];
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const double gn = j + 1 < m ? gb[d][v] : 0.0;
                    gb[d][v] = g.v[v][o + min(j + 1 + CAST_AHEAD, m - 1) * st];
                    double out, mn;
                    cast_cell_adj(gn, qv, mu[v], out, mn);
                    g.v[v][o + j * st] = out;
                    mu[v] = mn;
                }
            }
        }
    }
    if (R.emit) {
#pragma unroll
        for (int v = 0; v < NV; v++) tout[v * nl + e] = mu[v];
    }
}

// ---- form 2: the x draw through LDS ----
// The field is a row-major matrix [L lines][ex].  Tile T holds the columns 32 T .. 32 T + 31 (rows of 256 B, aligned where ex is
// a multiple of 32) of CX_LINES lines.  Staging: thread t moves column t % 32 of the rows t / 32 + 2 i, i < 32 -- a half-wave per
// row in global memory, consecutive doubles in LDS.  The walk: thread t takes row t, column by column, at pitch 33.
// (addresses clamped into the range and the block's lines, not predicated: what lands outside is never walked into a stored cell)
__device__ __forceinline__ void cx_load(double (&pre)[CX_ROWS], const double *__restrict__ src, long line0, long L, int ex, int T,
                                        int lo, int hi) {
    const int k = min(max(T * CX_TX + (int)(threadIdx.x & (CX_TX - 1)), lo), hi - 1);
    const int last = (int)min((long)CX_LINES, L - line0) - 1;
    const double *b = src + line0 * ex;
#pragma unroll
    for (int i = 0; i < CX_ROWS; i++) pre[i] = b[min((int)(threadIdx.x >> 5) + 2 * i, last) * ex + k];
}
__device__ __forceinline__ void cx_put(const double (&pre)[CX_ROWS], double *s) {
    const int col = threadIdx.x & (CX_TX - 1);
#pragma unroll
    for (int i = 0; i < CX_ROWS; i++) s[((threadIdx.x >> 5) + 2 * i) * CX_PITCH + col] = pre[i];
}
__device__ __forceinline__ void cx_store(double *__restrict__ dst, const double *s, long line0, long L, int ex, int T, int lo, int hi) {
    const int col = threadIdx.x & (CX_TX - 1), k = T * CX_TX + col;
    if (k < lo || k >= hi) return;
#pragma unroll 4
    for (int i = 0; i < CX_ROWS; i++) {
        const int row = (threadIdx.x >> 5) + 2 * i;
        if (line0 + row < L) dst[(line0 + row) * ex + k] = s[row * CX_PITCH + col];
    }
}
__global__ __launch_bounds__(CAST_BLK) void k_cast_x_fwd(long L, int ex, CastRanges rs, double eps, const double *__restrict__ x,
                                                         double *__restrict__ c, double *__restrict__ cq) {
    __shared__ double sx[CX_LINES * CX_PITCH], sq[CX_LINES * CX_PITCH];
    const CastRange R = rs.r[blockIdx.y];
    if (R.hi <= R.lo) return;
    const long line0 = blockIdx.x * (long)CX_LINES;
    const int Tlo = R.lo / CX_TX, Thi = (R.hi - 1) / CX_TX, nt = Thi - Tlo + 1;
    double pre[CX_ROWS];
    cx_load(pre, x, line0, L, ex, R.step > 0 ? Tlo : Thi, R.lo, R.hi);
    double *row = sx + threadIdx.x * CX_PITCH, *rowq = sq + threadIdx.x * CX_PITCH;
    double cp = 0.0;
    for (int t = 0; t < nt; t++) {
        const int T = R.step > 0 ? Tlo + t : Thi - t;
        cx_put(pre, sx);
        __syncthreads();
        if (t + 1 < nt) cx_load(pre, x, line0, L, ex, T + R.step, R.lo, R.hi);   // the next tile travels during the walk
        const int c0 = max(R.lo, T * CX_TX) - T * CX_TX, c1 = min(R.hi, (T + 1) * CX_TX) - T * CX_TX;   // columns c0 .. c1-1
        for (int j = 0; j < c1 - c0; j++) {
            const int col = R.step > 0 ? c0 + j : c1 - 1 - j;
            const double xv = row[col];
            double cv = xv, qv = 1.0;
            if (t > 0 || j > 0) cast_cell_fwd(xv, cp, eps, cv, qv);
            row[col] = cv;
            rowq[col] = qv;
            cp = cv;
        }
        __syncthreads();
        cx_store(c, sx, line0, L, ex, T, R.lo, R.hi);
        cx_store(cq, sq, line0, L, ex, T, R.lo, R.hi);
        __syncthreads();
    }
}
// per tile q is staged once for all nv vectors, then each vector's tile goes through the second plane; the vectors take turns in
// a loop that is not unrolled (registers as for one vector), so each line's hand-over values wait in LDS
__global__ __launch_bounds__(CAST_BLK) void k_cast_x_adj(long L, int ex, CastRanges rs, int nv, CastVecs g, const double *__restrict__ cq) {
    __shared__ double sg[CX_LINES * CX_PITCH], sq[CX_LINES * CX_PITCH], tc[CAST_MAXVEC * CX_LINES];
    const CastRange R = rs.r[blockIdx.y];
    if (R.hi <= R.lo) return;
    const long line0 = blockIdx.x * (long)CX_LINES;
    const int Tlo = R.lo / CX_TX, Thi = (R.hi - 1) / CX_TX, nt = Thi - Tlo + 1;
    double pre[CX_ROWS];
    cx_load(pre, cq, line0, L, ex, R.step > 0 ? Tlo : Thi, R.lo, R.hi);
    double *row = sg + threadIdx.x * CX_PITCH;
    const double *rowq = sq + threadIdx.x * CX_PITCH;
    for (int t = 0; t < nt; t++) {
        const int T = R.step > 0 ? Tlo + t : Thi - t;
        const int c0 = max(R.lo, T * CX_TX) - T * CX_TX, c1 = min(R.hi, (T + 1) * CX_TX) - T * CX_TX;
        cx_put(pre, sq);
        cx_load(pre, g.v[0], line0, L, ex, T, R.lo, R.hi);
#pragma unroll 1
        for (int v = 0; v < nv; v++) {
            cx_put(pre, sg);
            __syncthreads();
            // what is staged next travels during the walk: the next vector's tile, or q of the next tile
            if (v + 1 < nv)
                cx_load(pre, g.v[v + 1], line0, L, ex, T, R.lo, R.hi);
            else if (t + 1 < nt)
                cx_load(pre, cq, line0, L, ex, T + R.step, R.lo, R.hi);
            const int first = R.step > 0 ? c0 : c1 - 1;
            double mu = t > 0 ? row[first] + tc[v * CX_LINES + threadIdx.x] : row[first];
            for (int j = 0; j < c1 - c0; j++) {
                const int col = first + R.step * j;
                const double gn = j + 1 < c1 - c0 ? row[col + R.step] : 0.0;
                double out, mn;
                cast_cell_adj(gn, rowq[col], mu, out, mn);
                row[col] = out;
                mu = mn;
            }
            tc[v * CX_LINES + threadIdx.x] = mu;
            __syncthreads();
            cx_store(g.v[v], sg, line0, L, ex, T, R.lo, R.hi);
            __syncthreads();
        }
    }
}

struct tp_casting {
    tp_grid *grid;
    int axis, parting;   // parting: global
    int n;               // global layers along the axis
    int have_fwd, last_form;
    double eps;
    long nel, lay;
    DevBuf<double> cq;          // [dev, own elements] q of the last forward sweep
    DevBuf<double> cin[2];      // [dev, one layer] z draw on slabs: c of the layer beyond the own ones, upper / lower range
    DevBuf<double> tin[2];      // [dev, CAST_MAXVEC layers] ... the transpose's hand-over value received, upper / lower range
    DevBuf<double> tout[2];     // [dev, CAST_MAXVEC layers] ... and to be sent
};

static bool casting_args_ok(const tp_grid *g, int axis, int parting) {
    if (!g || axis < 0 || axis > 2 || parting < 0) return false;
    return true;
}
extern "C" int tp_casting_destroy(tp_casting *c) {
    if (!c) return TP_OK;
    (void)hipStreamSynchronize(c->grid->stream);
    delete c;
    return TP_OK;
}
extern "C" int tp_casting_set_params(tp_casting *c, double eps) {
    if (!c || !std::isfinite(eps) || !(eps > 0.0)) return TP_ERR_ARG;
    c->eps = eps;
    c->have_fwd = 0;  // the stored coefficients belong to the former parameter
    return TP_OK;
}
extern "C" int tp_casting_create(tp_casting **out, tp_grid *g, int axis, int parting) {
    if (!out || !casting_args_ok(g, axis, parting)) return TP_ERR_ARG;
    const int n = axis == 0 ? g->ex : axis == 1 ? g->ey : g->ez_glob;
    if (parting > n) return TP_ERR_ARG;
    std::unique_ptr<tp_casting> c(new tp_casting());
    c->grid = g;
    c->axis = axis;
    c->parting = parting;
    c->n = n;
    c->eps = 1e-6;
    c->lay = (long)g->ex * g->ey;
    c->nel = c->lay * g->ez_own;
    TP_TRY(c->cq.alloc((size_t)c->nel));
    if (axis == 2 && g->nranks > 1) {
        for (DevBuf<double> *p : {&c->cin[0], &c->cin[1]}) TP_TRY(p->alloc((size_t)c->lay));
        for (DevBuf<double> *p : {&c->tin[0], &c->tin[1], &c->tout[0], &c->tout[1]}) TP_TRY(p->alloc((size_t)c->lay * CAST_MAXVEC));
    }
    *out = c.release();
    return TP_OK;
}
extern "C" int tp_casting_last_form(const tp_casting *c) { return c ? c->last_form : 0; }
// read-only copy of q of the last forward sweep (own elements)
extern "C" int tp_casting_get_q(tp_casting *c, double *q) {
    if (!c || !q || !c->have_fwd) return TP_ERR_ARG;
    TP_HIP(hipMemcpyAsync(q, c->cq, sizeof(double) * (size_t)c->nel, hipMemcpyDeviceToDevice, c->grid->stream));
    return TP_OK;
}

// lines and strides of the walk kernel on this rank
static CastGeom casting_geom(const tp_casting *c) {
    const tp_grid *g = c->grid;
    CastGeom q;
    if (c->axis == 0) {   // form 3: the lines are the rows
        q.ni = g->ey * g->ez_own, q.nr = 1, q.sI = g->ex, q.sR = 0, q.sL = 1;
    } else if (c->axis == 1) {
        q.ni = g->ex, q.nr = g->ez_own, q.sI = 1, q.sR = c->lay, q.sL = g->ex;
    } else {
        q.ni = g->ex, q.nr = g->ey, q.sI = 1, q.sR = g->ex, q.sL = c->lay;
    }
    return q;
}
// the own part [a, nl) of the upper range and [0, a) of the lower one
static int casting_split(const tp_casting *c, int *nl) {
    const tp_grid *g = c->grid;
    const int z0 = c->axis == 2 ? g->rank * g->ez_own : 0;
    *nl = c->axis == 2 ? g->ez_own : c->n;
    const int a = c->parting - z0;
    return a < 0 ? 0 : a > *nl ? *nl : a;
}
static int casting_form(const tp_casting *c) { return c->axis != 0 ? 1 : sw_casting_xform() ? 2 : 3; }

static int casting_launch_fwd(tp_casting *c, int form, const CastRanges &rs, int nrg, const double *x, double *out) {
    tp_grid *g = c->grid;
    long cells = 0;
    for (int k = 0; k < nrg; k++) cells += rs.r[k].hi - rs.r[k].lo;
    if (form == 2) {
        const long L = (long)g->ey * g->ez_own;
        TP_LAUNCH(k_cast_x_fwd, dim3((unsigned)((L + CX_LINES - 1) / CX_LINES), nrg), dim3(CAST_BLK), 0, g->stream, L, g->ex, rs, c->eps, x,
                  out, c->cq);
        count_launch(g, 24.0 * cells * L, 0.0);
    } else {
        const CastGeom q = casting_geom(c);
        const long nl = (long)q.ni * q.nr;
        TP_LAUNCH(k_cast_walk_fwd, dim3((unsigned)((nl + CAST_BLK - 1) / CAST_BLK), nrg), dim3(CAST_BLK), 0, g->stream, q, rs, c->eps, x,
                  out, c->cq, (const double *)c->cin[0], (const double *)c->cin[1]);
        count_launch(g, 24.0 * cells * nl, 0.0);
    }
    return TP_OK;
}
template <int NV>
static int casting_launch_adj(tp_casting *c, int form, const CastRanges &rs, int nrg, double *const *gv) {
    tp_grid *g = c->grid;
    CastVecs vs;
    for (int v = 0; v < CAST_MAXVEC; v++) vs.v[v] = v < NV ? gv[v] : nullptr;
    long cells = 0;
    for (int k = 0; k < nrg; k++) cells += rs.r[k].hi - rs.r[k].lo;
    if (form == 2) {
        const long L = (long)g->ey * g->ez_own;
        TP_LAUNCH(k_cast_x_adj, dim3((unsigned)((L + CX_LINES - 1) / CX_LINES), nrg), dim3(CAST_BLK), 0, g->stream, L, g->ex, rs, NV, vs,
                  (const double *)c->cq);
        count_launch(g, (8.0 + 16.0 * NV) * cells * L, 0.0);
    } else {
        const CastGeom q = casting_geom(c);
        const long nl = (long)q.ni * q.nr;
        TP_LAUNCH(k_cast_walk_adj<NV>, dim3((unsigned)((nl + CAST_BLK - 1) / CAST_BLK), nrg), dim3(CAST_BLK), 0, g->stream, q, rs, vs,
                  (const double *)c->cq, (const double *)c->tin[0], (const double *)c->tin[1], (double *)c->tout[0], (double *)c->tout[1]);
        count_launch(g, (8.0 + 16.0 * NV) * cells * nl, 0.0);
    }
    return TP_OK;
}
static int casting_launch_adj_nv(tp_casting *c, int form, const CastRanges &rs, int nrg, int nv, double *const *gv) {
    switch (nv) {
        case 1: return casting_launch_adj<1>(c, form, rs, nrg, gv);
        case 2: return casting_launch_adj<2>(c, form, rs, nrg, gv);
        case 3: return casting_launch_adj<3>(c, form, rs, nrg, gv);
        case 4: return casting_launch_adj<4>(c, form, rs, nrg, gv);
        case 5: return casting_launch_adj<5>(c, form, rs, nrg, gv);
        case 6: return casting_launch_adj<6>(c, form, rs, nrg, gv);
        case 7: return casting_launch_adj<7>(c, form, rs, nrg, gv);
        default: return casting_launch_adj<8>(c, form, rs, nrg, gv);
    }
}

extern "C" int tp_casting_forward(tp_casting *c, const double *x, double *out) {
    if (!c || !x || !out || x == out) return TP_ERR_ARG;
    tp_grid *g = c->grid;
    const int form = casting_form(c);
    int nl;
    const int a = casting_split(c, &nl);
    // slot 0: the upper range, downwards from the top; slot 1: the lower range, upwards from the bottom
    const CastRange up = {a, nl, -1, 0, 0}, low = {0, a, +1, 0, 0};
    if (c->axis != 2 || g->nranks == 1) {   // rank-local: both ranges in one launch
        CastRanges rs = {{up, low}};
        TP_TRY(casting_launch_fwd(c, form, rs, 2, x, out));
    } else {
        // the recursion runs along the slab axis: the upper range's sweep comes down from the top rank, the lower range's goes up
        // from rank 0, one slab per turn each, a layer of c crossing the border after every turn.  Serial in the number of slabs.
        // Every rank joins every exchange; what it receives out of turn is overwritten before it is read.
        const int N = g->nranks, r = g->rank;
        for (int turn = 0; turn < N; turn++) {
            CastRanges rs = {{{0, 0, -1, 0, 0}, {0, 0, +1, 0, 0}}};
            if (turn == N - 1 - r) rs.r[0] = up, rs.r[0].carry = r < N - 1;
            if (turn == r) rs.r[1] = low, rs.r[1].carry = r > 0;
            if (rs.r[0].hi > rs.r[0].lo || rs.r[1].hi > rs.r[1].lo) TP_TRY(casting_launch_fwd(c, form, rs, 2, x, out));
            if (turn < N - 1)
                TP_TRY(exchange_segments(g, out, c->cin[1], out + (long)(nl - 1) * c->lay, c->cin[0], c->lay, 1, c->lay));
        }
    }
    c->have_fwd = 1;
    c->last_form = form;
    return TP_OK;
}
extern "C" int tp_casting_adjoint(tp_casting *c, int nvec, double *const *gv) {
    if (!c || !gv || nvec < 1 || nvec > CAST_MAXVEC) return TP_ERR_ARG;
    for (int v = 0; v < nvec; v++)
        if (!gv[v]) return TP_ERR_ARG;
    if (!c->have_fwd) return TP_ERR_ARG;
    tp_grid *g = c->grid;
    const int form = casting_form(c);
    int nl;
    const int a = casting_split(c, &nl);
    // against the sweeps: the upper range upwards from the parting plane, the lower range downwards from it
    const CastRange up = {a, nl, +1, 0, 0}, low = {0, a, -1, 0, 0};
    if (c->axis != 2 || g->nranks == 1) {
        CastRanges rs = {{up, low}};
        TP_TRY(casting_launch_adj_nv(c, form, rs, 2, nvec, gv));
    } else {
        const int N = g->nranks, r = g->rank, z0 = r * g->ez_own;
        for (int turn = 0; turn < N; turn++) {
            CastRanges rs = {{{0, 0, +1, 0, 0}, {0, 0, -1, 0, 0}}};
            if (turn == r) rs.r[0] = up, rs.r[0].carry = z0 > c->parting, rs.r[0].emit = r < N - 1;
            if (turn == N - 1 - r) rs.r[1] = low, rs.r[1].carry = z0 + nl < c->parting, rs.r[1].emit = r > 0;
            if (rs.r[0].hi > rs.r[0].lo || rs.r[1].hi > rs.r[1].lo) TP_TRY(casting_launch_adj_nv(c, form, rs, 2, nvec, gv));
            if (turn < N - 1)   // the upper range's t goes up, the lower range's goes down
                TP_TRY(exchange_segments(g, c->tout[1], c->tin[0], c->tout[0], c->tin[1], c->lay, nvec, c->lay));
        }
    }
    c->last_form = form;
    return TP_OK;
}
