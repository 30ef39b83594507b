// conduction.h -- steady heat conduction: the scalar operator  A = N K(k) N + (I - N)  with one conductivity per element and
// Dirichlet rows (heat sink, T = 0), and the kernels that build its Galerkin hierarchy.  DESIGN.md 4.17.
//
//   ConductionOp            the fine level for k_node<1, Op, EPI>: 27 neighbour values + one word of mask bits + 8 conductivities
//                           per node instead of the gather's 64 + 64 + 8 (MatfreeOp<1>), the sum in the gather's own order
//   k_cond_nbmask           the mask bits of the 27 neighbours of every node, once per set of supports
//   k_cond_diag             Jacobi diagonal of the fine level
//   k_cond_galerkin_fine    level 0 -> 1 element matrices (8 x 8) from the conductivities
//   k_cond_galerkin_coarse  level l -> l + 1 from the stored element matrices
//   k_cond_elem_to_dia      element matrices -> 27 diagonals (DiaOp<1>) and the Jacobi diagonal
//   k_cond_response         thermal compliance of one or several load cases and its sensitivity
//
// Element matrices of a coarse level are stored element-major, Kel[elem * 64 + 8 I + J], reference corner order.
// Included by mg.h (the operator is launched by MGSolver<1>::op_matfree_node); the handle and the C entry points are in
// conduction_api.h.
#pragma once
#include "common.h"
#include "operators.h"

// corner a of the reference order -> its bit along axis d (c_LX / c_LY / c_LZ as arithmetic: the index may differ per lane)
__host__ __device__ inline int cond_cbit(int a, int d) { return d == 0 ? (((a & 3) == 1 || (a & 3) == 2) ? 1 : 0) : (d == 1 ? ((a >> 1) & 1) : (a >> 2)); }
// trilinear weight of coarse corner I at corner a of the child at position c = cx + 2 cy + 4 cz (host_W of galerkin.h): a product
// over the axes of 1, 1/2 or 0 -- exact
__host__ __device__ inline double cond_w(int c, int a, int I) {
    double w = 1.0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int p = ((c >> d) & 1) + cond_cbit(a, d);
        w *= cond_cbit(I, d) ? 0.5 * p : 1.0 - 0.5 * p;
    }
    return w;
}
// which of the 8 distinct values of a box element's matrix couples corners a and b: the axes along which they differ
__host__ __device__ constexpr int cond_vidx(int a, int b) {
    return (LXc(a) != LXc(b) ? 1 : 0) + (LYc(a) != LYc(b) ? 2 : 0) + (LZc(a) != LZc(b) ? 4 : 0);
}

// ---------------------------------------------------------------------------
// The fine level.  y_n = sum over the 8 elements a around node n (n is their corner a) of k_a sum_b KT[a][b] (N u)_b, rows of
// clamped nodes y_n = u_n.  The 27 neighbour values are loaded once and zeroed where the neighbour is clamped (bit q of
// nbm[n]: neighbour at offset q = (dz + 1) 9 + (dy + 1) 3 + (dx + 1)); an element beyond the mesh takes conductivity 0 and
// reads from clamped addresses, so the sum has one shape for every node: a = 0 .. 7, inside it b = 0 .. 7, fma throughout --
// the order of MatfreeOp<1>, whose skipped elements are this form's fma(0, s, y) = y: the two forms give the same bits.
// The 8 distinct entries of KT are kernel arguments (scalar registers).
struct ConductionOp {
    const double *__restrict__ kc;      // per stored element
    const unsigned *__restrict__ nbm;   // per node
    double v[8];                        // KT by differing axes (cond_vidx)
    Geom g;

    __device__ inline void classes(int i, int j, int k, int &cx, int &cy, int &cz) const {
        // element (i-1 .. i) x (j-1 .. j) x (k-1 .. k) existence, as MatfreeOp tests it (local layers [0, ezl))
        cx = i == 0 ? 0 : (i >= g.ex ? 2 : 1), cy = j == 0 ? 0 : (j >= g.ey ? 2 : 1), cz = k == 0 ? 0 : (k >= g.ezl ? 2 : 1);
    }
    // the conductivities of the 8 elements around the node, 0 for those beyond the mesh
    __device__ inline void conductivities(int i, int j, int k, int cx, int cy, int cz, double ka[8]) const {
#pragma unroll
        for (int a = 0; a < 8; a++) {
            const bool ex = !((LXc(a) ? cx == 0 : cx == 2) || (LYc(a) ? cy == 0 : cy == 2) || (LZc(a) ? cz == 0 : cz == 2));
            const int ei = ex ? i - LXc(a) : 0, ej = ex ? j - LYc(a) : 0, ek = ex ? k - LZc(a) : 0;
            const double kv = kc[(long)ei + (long)g.ex * (ej + (long)g.ey * ek)];
            ka[a] = ex ? kv : 0.0;
        }
    }
    __device__ inline void apply(const double *__restrict__ u, int i, int j, int k, long n, double y[1]) const {
        int cx, cy, cz;
        classes(i, j, k, cx, cy, cz);
        const unsigned m = nbm[n];
        double w[27];
#pragma unroll
        for (int dz = -1; dz <= 1; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const bool ok = !((dx < 0 && cx == 0) || (dx > 0 && cx == 2) || (dy < 0 && cy == 0) || (dy > 0 && cy == 2) ||
                                      (dz < 0 && cz == 0) || (dz > 0 && cz == 2));
                    const long nb = ok ? n + dx + (long)g.nx * (dy + (long)g.ny * dz) : n;   // (conductivity 0 there)
                    w[(dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)] = u[nb];
                }
        const double own = w[13];
#pragma unroll
        for (int q = 0; q < 27; q++) w[q] = ((m >> q) & 1u) ? 0.0 : w[q];
        double ka[8];
        conductivities(i, j, k, cx, cy, cz, ka);
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 8; a++) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const int q = (LZc(b) - LZc(a) + 1) * 9 + (LYc(b) - LYc(a) + 1) * 3 + (LXc(b) - LXc(a) + 1);
                t = fma(v[cond_vidx(a, b)], w[q], t);
            }
            s = fma(ka[a], t, s);
        }
        y[0] = ((m >> 13) & 1u) ? own : s;
    }
    // the node's own entry of N K N + (I - N)
    __device__ inline void diag_block(long n, int i, int j, int k, double D[1]) const {
        int cx, cy, cz;
        classes(i, j, k, cx, cy, cz);
        double ka[8];
        conductivities(i, j, k, cx, cy, cz, ka);
        double d = 0.0;
#pragma unroll
        for (int a = 0; a < 8; a++) d = fma(ka[a], v[0], d);
        D[0] = ((nbm[n] >> 13) & 1u) ? 1.0 : d;
    }
};

// mask byte (bit 0: clamped) and the mask bits of the 27 neighbours of every LOCAL node (ghost planes included: their own bits
// are what a neighbour's row reads); a neighbour beyond the local planes counts as free
__global__ __launch_bounds__(BLK) void k_cond_nbmask(Geom g, const double *__restrict__ N, uint8_t *__restrict__ mask,
                                                     unsigned *__restrict__ nbm) {
    const long nn = g.nodes();
    for (long n = blockIdx.x * (long)BLK + threadIdx.x; n < nn; n += (long)gridDim.x * BLK) {
        const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
        unsigned m = 0;
        for (int q = 0; q < 27; q++) {
            const int dx = q % 3 - 1, dy = (q / 3) % 3 - 1, dz = q / 9 - 1;
            if (i + dx < 0 || i + dx >= g.nx || j + dy < 0 || j + dy >= g.ny || k + dz < 0 || k + dz >= g.nzl) continue;
            if (N[n + dx + (long)g.nx * (dy + (long)g.ny * dz)] == 0.0) m |= 1u << q;
        }
        nbm[n] = m;
        mask[n] = (uint8_t)((m >> 13) & 1u);
    }
}

// Jacobi diagonal of the fine level: dinv_n = 1 / sum_a k_a KT[a][a], 1 on a clamped row
__global__ __launch_bounds__(BLK) void k_cond_diag(ConductionOp op, double *__restrict__ dinv) {
    const Geom &g = op.g;
    const long plane = g.plane();
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    const int k = g.own_lo + (int)(t / plane);
    const int rem = (int)(t % plane);
    const int j = rem / g.nx, i = rem % g.nx;
    const long n = t + plane * g.own_lo;
    double D[1];
    op.diag_block(n, i, j, k, D);
    dinv[n] = ((op.nbm[n] >> 13) & 1u) ? 1.0 : 1.0 / D[0];
}

// ---------------------------------------------------------------------------
// Galerkin levels (galerkin.h: A_c = P^T A P element by element, K_E = sum_c W_c^T K_c W_c, the Dirichlet identity spread over
// the elements sharing the node with weight 1 / multiplicity), 8 x 8.
// ---------------------------------------------------------------------------
// M[c][64] = W_c^T KT W_c, the 8 child matrices of an element without clamped nodes (host, once per KT; summed in long double
// and rounded once)
inline void cond_child_matrices(const double *KT, double *M /* 8 * 64 */) {
    for (int c = 0; c < 8; c++)
        for (int I = 0; I < 8; I++)
            for (int J = 0; J < 8; J++) {
                long double s = 0.0L;
                for (int a = 0; a < 8; a++)
                    for (int b = 0; b < 8; b++) s += (long double)cond_w(c, a, I) * (long double)KT[a * 8 + b] * (long double)cond_w(c, b, J);
                M[c * 64 + I * 8 + J] = (double)s;
            }
}

// Level 0 -> 1: a wave per own coarse element, lane = entry (I, J).  K_E = sum_c k_c M_c where none of the element's 27 fine
// nodes is clamped; otherwise sum_c [ k_c W_c^T N_c KT N_c W_c + W_c^T D_c W_c ] term by term.  Either way one fixed order.
__global__ __launch_bounds__(BLK) void k_cond_galerkin_fine(Geom gf, Geom gc, const double *__restrict__ kc,
                                                            const uint8_t *__restrict__ mask, ConductionOp kt,
                                                            const double *__restrict__ M, double *__restrict__ Kel) {
    const long t = blockIdx.x * (long)(BLK / WAVE) + (threadIdx.x >> 6);  // own coarse element (uniform over the wave)
    if (t >= gc.own_elems()) return;
    const int e = threadIdx.x & 63, I = e >> 3, J = e & 7;
    const int Ie = (int)(t % gc.ex), Je = (int)((t / gc.ex) % gc.ey), Ke = (int)(t / ((long)gc.ex * gc.ey));
    // the masks of the element's 27 fine nodes, one per lane, as one wave-uniform word: bit di + 3 dj + 9 dk
    unsigned mine = 0;
    if (e < 27) mine = mask[(long)(2 * Ie + e % 3) + (long)gf.nx * ((2 * Je + (e / 3) % 3) + (long)gf.ny * (2 * Ke + e / 9))];
    const unsigned mm = (unsigned)__ballot(mine != 0);
    double kch[8];
#pragma unroll
    for (int c = 0; c < 8; c++)
        kch[c] = kc[(long)(2 * Ie + (c & 1)) + (long)gf.ex * ((2 * Je + ((c >> 1) & 1)) + (long)gf.ey * (2 * Ke + (c >> 2)))];
    double acc = 0.0;
    if (mm == 0) {
#pragma unroll
        for (int c = 0; c < 8; c++) acc = fma(kch[c], M[c * 64 + e], acc);
    } else {
        for (int c = 0; c < 8; c++) {
            const int cb[3] = {c & 1, (c >> 1) & 1, c >> 2};
            double sk = 0.0;
            for (int a = 0; a < 8; a++) {
                const double wI = cond_w(c, a, I);
                if (wI == 0.0) continue;
                const int ax = cond_cbit(a, 0), ay = cond_cbit(a, 1), az = cond_cbit(a, 2);
                const bool ma = (mm >> ((cb[0] + ax) + 3 * (cb[1] + ay) + 9 * (cb[2] + az))) & 1u;
                if (ma) {
                    // Dirichlet identity of node a, shared between the elements around it: multiplicity from its GLOBAL position
                    const double wJ = cond_w(c, a, J);
                    if (wJ == 0.0) continue;
                    const int ia = 2 * Ie + cb[0] + ax, ja = 2 * Je + cb[1] + ay, kg = 2 * Ke + cb[2] + az + gf.gz0;
                    const int mult = ((ia == 0 || ia == gf.nx - 1) ? 1 : 2) * ((ja == 0 || ja == gf.ny - 1) ? 1 : 2) *
                                     ((kg == 0 || kg == gf.nz_glob - 1) ? 1 : 2);
                    acc += wI * wJ / (double)mult;
                    continue;
                }
                for (int b = 0; b < 8; b++) {
                    const double wJ = cond_w(c, b, J);
                    const bool mb = (mm >> ((cb[0] + cond_cbit(b, 0)) + 3 * (cb[1] + cond_cbit(b, 1)) + 9 * (cb[2] + cond_cbit(b, 2)))) & 1u;
                    if (wJ == 0.0 || mb) continue;
                    const int vi = (ax != cond_cbit(b, 0) ? 1 : 0) + (ay != cond_cbit(b, 1) ? 2 : 0) + (az != cond_cbit(b, 2) ? 4 : 0);
                    sk = fma(wI * wJ, kt.v[vi], sk);
                }
            }
            acc = fma(kch[c], sk, acc);
        }
    }
    Kel[t * 64 + e] = acc;
}

// Level l -> l + 1 (l >= 1): a wave per own coarse element, four per workgroup.  Per child two 8-term contractions through LDS,
// T = K_c W_c (lane (a, J)), then W_c^T T (lane (I, J)), the children added in the order c = 0 .. 7.
__global__ __launch_bounds__(BLK) void k_cond_galerkin_coarse(Geom gf, Geom gc, const double *__restrict__ Kf, double *__restrict__ Kc) {
    __shared__ double s_A[BLK / WAVE][64], s_T[BLK / WAVE][64];
    const int wv = threadIdx.x >> 6, e = threadIdx.x & 63, I = e >> 3, J = e & 7;
    const long t = blockIdx.x * (long)(BLK / WAVE) + wv;
    const bool valid = t < gc.own_elems();
    const long tt = valid ? t : 0;
    const int Ie = (int)(tt % gc.ex), Je = (int)((tt / gc.ex) % gc.ey), Ke = (int)(tt / ((long)gc.ex * gc.ey));
    double acc = 0.0;
    for (int c = 0; c < 8; c++) {
        const long ch = (long)(2 * Ie + (c & 1)) + (long)gf.ex * ((2 * Je + ((c >> 1) & 1)) + (long)gf.ey * (2 * Ke + (c >> 2)));
        s_A[wv][e] = Kf[ch * 64 + e];
        __syncthreads();
        double s = 0.0;   // T[a = I][J]
#pragma unroll
        for (int b = 0; b < 8; b++) s = fma(s_A[wv][I * 8 + b], cond_w(c, b, J), s);
        s_T[wv][e] = s;
        __syncthreads();
        double r = 0.0;
#pragma unroll
        for (int a = 0; a < 8; a++) r = fma(cond_w(c, a, I), s_T[wv][a * 8 + J], r);
        acc += r;
        __syncthreads();
    }
    if (valid) Kc[t * 64 + e] = acc;
}

// Element matrices -> the 27 diagonals of DiaOp<1>, S[blk * nrows + n], and the Jacobi diagonal from the centre one.
// thread = owned node, blockIdx.y = neighbour offset; the <= 8 elements around the node in corner order.
__global__ __launch_bounds__(BLK) void k_cond_elem_to_dia(Geom g, const double *__restrict__ Kel, double *__restrict__ S,
                                                          double *__restrict__ dinv) {
    const long nrows = g.nodes();
    const long plane = g.plane();
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    const int blk = blockIdx.y;
    const int di = blk % 3 - 1, dj = (blk / 3) % 3 - 1, dk = blk / 9 - 1;
    const int k = g.own_lo + (int)(t / plane);
    const int rem = (int)(t % plane);
    const int j = rem / g.nx, i = rem % g.nx;
    const long n = t + plane * g.own_lo;
    double acc = 0.0;
    for (int I = 0; I < 8; I++) {
        const int lx = cond_cbit(I, 0), ly = cond_cbit(I, 1), lz = cond_cbit(I, 2);
        const int ei = i - lx, ej = j - ly, ek = k - lz;   // element in which this node is corner I
        if (ei < 0 || ei >= g.ex || ej < 0 || ej >= g.ey || ek < 0 || ek >= g.ezl) continue;
        const int jx = lx + di, jy = ly + dj, jz = lz + dk;  // the neighbour as a corner of that element
        if (jx < 0 || jx > 1 || jy < 0 || jy > 1 || jz < 0 || jz > 1) continue;
        acc += Kel[((long)ei + (long)g.ex * (ej + (long)g.ey * ek)) * 64 + I * 8 + corner_of(jx, jy, jz)];
    }
    S[(long)blk * nrows + n] = acc;
    if (blk == 13) dinv[n] = 1.0 / acc;
}

// ---------------------------------------------------------------------------
// Thermal compliance and its sensitivity (response.h's k_response with 8-vectors): per case l the unweighted sum
// f_l = sum_e k_e v_e^T KT t_e, and dfdx_e = -p x^(p-1) (kmax - kmin) sum_l w_l v_e^T KT t_e.  One thread per own element, the
// cases in a loop, every sum in a fixed order.
// ---------------------------------------------------------------------------
struct CondRespArgs {
    const double *T[TP_MAX_CASES];
    const double *V[TP_MAX_CASES];   // never NULL (the host puts T[l] where the caller passed none)
    double w[TP_MAX_CASES];
    int ncase;
};
template <bool REDUCE>
__global__ __launch_bounds__(BLK) void k_cond_response(Geom g, ConductionOp kt, CondRespArgs a, const double *__restrict__ x,
                                                       double kmin, double kmax, double penal, double *__restrict__ dfdx,
                                                       double *__restrict__ partials) {
    const long nel = g.own_elems();
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    const bool in = t < nel;
    long nd0 = 0;
    double xe = 0.0, xp1 = 0.0, ke = 0.0;
    if (in) {
        int i, j, k;
        elem_ijk(g, t, i, j, k);
        nd0 = elem_node0(g, i, j, k);
        xe = x[t];
        xp1 = pow(xe, penal - 1);
        ke = kmin + (xe == 0.0 ? 0.0 : xp1 * xe) * (kmax - kmin);  // (x = 0: x^p = 0 for p > 0 whatever x^(p-1) is)
    }
    double acc = 0.0;
    for (int l = 0; l < a.ncase; l++) {
        double vKt = 0.0;
        if (in) {
            double te[8], ve[8];
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const long nd = corner_node(g, nd0, c);
                te[c] = a.T[l][nd];
                ve[c] = a.V[l][nd];
            }
#pragma unroll
            for (int r = 0; r < 8; r++) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < 8; c++) s = fma(kt.v[cond_vidx(r, c)], te[c], s);
                vKt = fma(ve[r], s, vKt);
            }
            acc = fma(a.w[l], vKt, acc);
        }
        if (REDUCE) {  // (every thread of the workgroup passes here: l is uniform)
            const double f = block_sum(ke * vKt);
            if (threadIdx.x == 0) partials[(long)l * gridDim.x + blockIdx.x] = f;
        }
    }
    if (in && dfdx) dfdx[t] = -1.0 * penal * xp1 * (kmax - kmin) * acc;
    if (REDUCE) {
        const double vol = block_sum(xe);
        if (threadIdx.x == 0) partials[(long)a.ncase * gridDim.x + blockIdx.x] = vol;
    }
}
