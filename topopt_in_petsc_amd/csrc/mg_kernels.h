// mg_kernels.h -- the free kernels and host helpers of the multigrid-preconditioned CG (mg.h): the CG vector updates,
// the Lanczos chain's kernels, the tridiagonal eigenvalue bisections and the element bound of the matrix-free level.
#pragma once
#include "common.h"

// CG scalar slots in tp_grid::scal
enum { S_BB = 0, S_RR = 1, S_PW = 2, S_RZ0 = 3, S_RZ1 = 4, S_TMP = 8 };

// x += alpha p, r -= alpha w, ||r||^2 (also to pinned host memory if out_host); z1 != NULL: also the first Chebyshev step of
// the NEXT V-cycle's pre-smoothing from its zero guess, z1 = dinv r / theta (k_cheb_first: the same product in the same
// order) -- one pass over r less and one launch less per Krylov iteration
// NT: x, p and w pass through with non-temporal loads / stores -- none of the three is read again before ~10 other vectors
// of the same size have gone by, while r and z1 are the next kernel's input: the hint keeps the streamed ones from
// displacing them in the Infinity Cache.  Measured at 128^3 (two runs each, round 5): 12.50 / 12.48 -> 12.40 / 12.32 ms per
// design iteration, the following fine-level Chebyshev launches 58.9 / 57.3 -> 54.7 / 54.4 us (in-step roofline fraction
// 0.40-0.41 -> 0.43).  Measured and dropped in the same round: the stores of r and z1 non-temporal as well (12.39 / 12.28 against
// 12.37 / 12.23: the next kernel then misses them), the restriction reading the fine residual non-temporally (12.6-12.8: slower)
template <bool NT>
__global__ __launch_bounds__(BLK) void k_cg_update_xr(double *__restrict__ x, double *__restrict__ r,
                                                      const double *__restrict__ p, const double *__restrict__ w,
                                                      const double *__restrict__ scal, int slot_rz, long off, long n,
                                                      double *__restrict__ partials, unsigned *ticket,
                                                      double *__restrict__ out, double *__restrict__ out_host,
                                                      double *__restrict__ z1, const double *__restrict__ dinv, double inv_theta) {
    const double alpha = scal[slot_rz] / scal[S_PW];
    double s = 0.0;
    for (long i = blockIdx.x * (long)BLK + threadIdx.x; i < n; i += (long)gridDim.x * BLK) {
        const long q = off + i;
        double rn;
        if constexpr (NT) {
            __builtin_nontemporal_store(fma(alpha, __builtin_nontemporal_load(p + q), __builtin_nontemporal_load(x + q)), x + q);
            rn = fma(-alpha, __builtin_nontemporal_load(w + q), r[q]);
        } else {
            x[q] = fma(alpha, p[q], x[q]);
            rn = fma(-alpha, w[q], r[q]);
        }
        r[q] = rn;
        s = fma(rn, rn, s);
        if (z1) z1[q] = dinv[q] * rn * inv_theta;
    }
    const double v[1] = {block_sum(s)};
    reduce_tail<1>(v, partials, gridDim.x, blockIdx.x, ticket, out, out_host);
}
// p = z + (rz_new/rz_old) p   (first: p = z)
__global__ __launch_bounds__(BLK) void k_cg_update_p(double *__restrict__ p, const double *__restrict__ z,
                                                     const double *__restrict__ scal, int slot_new, int slot_old,
                                                     int first, long off, long n) {
    const double beta = first ? 0.0 : scal[slot_new] / scal[slot_old];
    for (long i = blockIdx.x * (long)BLK + threadIdx.x; i < n; i += (long)gridDim.x * BLK) {
        const long q = off + i;
        p[q] = first ? z[q] : fma(beta, p[q], z[q]);
    }
}
// two dot products in one pass: partials[b] = a1.b1, partials[nb + b] = a2.b2
__global__ __launch_bounds__(BLK) void k_dot2(const double *__restrict__ a1, const double *__restrict__ b1,
                                              const double *__restrict__ a2, const double *__restrict__ b2, long off,
                                              long n, double *__restrict__ partials) {
    double s1 = 0.0, s2 = 0.0;
    for (long i = blockIdx.x * (long)BLK + threadIdx.x; i < n; i += (long)gridDim.x * BLK) {
        s1 = fma(a1[off + i], b1[off + i], s1);
        s2 = fma(a2[off + i], b2[off + i], s2);
    }
    s1 = block_sum(s1);
    s2 = block_sum(s2);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s1;
        partials[gridDim.x + blockIdx.x] = s2;
    }
}

// Lanczos helpers (owned range)
template <int DOF>
__global__ __launch_bounds__(BLK) void k_lanczos_init(Geom g, double *__restrict__ v, double *__restrict__ dis,
                                                      const double *__restrict__ dinv, double *__restrict__ coef, int ncoef) {
    // the run's coefficient table starts from zero (a memset node in the replayed chain cost ~50 us before its first kernel)
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < ncoef; i += BLK) coef[i] = 0.0;
    const long plane = g.plane();
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    const long n = t + plane * g.own_lo;
    const uint64_t gn = (uint64_t)(n + plane * (long)g.gz0);  // global node id
#pragma unroll
    for (int c = 0; c < DOF; c++) {
        v[n * DOF + c] = hash_u01(gn * DOF + c, 0x5eedULL) - 0.5;
        dis[n * DOF + c] = sqrt(dinv[n * DOF + c]);
    }
}
// partials[q*nb + b] = sum over block b of V_q . w   (grid = (nb, nv); V_q = V + q*stride)
// Round 6: with `mticket` the last workgroup of vector q to arrive adds q's partial sums itself, in k_reduce_multi's order
// (bitwise the same value, one dependent launch less per Gram-Schmidt pass).  Counters as in reduce_tail (common.h), one set
// of 8 shards + top per vector, MT_STRIDE words apart (a cache line of their own each); they rest at 0.
constexpr int MT_STRIDE = 64;             // unsigned words between two counters (256 B)
constexpr int MT_WORDS = 9 * MT_STRIDE;   // per vector
__global__ __launch_bounds__(BLK) void k_multi_dot(const double *__restrict__ V, long stride, int nv,
                                                   const double *__restrict__ w, long off, long n,
                                                   double *__restrict__ partials, unsigned *mticket,
                                                   double *__restrict__ out) {
    const int q = blockIdx.y;
    const double *__restrict__ vq = V + (long)q * stride;
    // 4 independent chains: with one workgroup per vector (small levels) the loop is latency bound
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const long st = (long)gridDim.x * BLK;
    long i = blockIdx.x * (long)BLK + threadIdx.x;
    for (; i + 3 * st < n; i += 4 * st) {
        s0 = fma(vq[off + i], w[off + i], s0);
        s1 = fma(vq[off + i + st], w[off + i + st], s1);
        s2 = fma(vq[off + i + 2 * st], w[off + i + 2 * st], s2);
        s3 = fma(vq[off + i + 3 * st], w[off + i + 3 * st], s3);
    }
    for (; i < n; i += st) s0 = fma(vq[off + i], w[off + i], s0);
    double s = block_sum((s0 + s1) + (s2 + s3));
    const int nb = gridDim.x, b = blockIdx.x;
    if (!mticket) {
        if (threadIdx.x == 0) partials[(long)q * nb + b] = s;
        return;
    }
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __hip_atomic_store(&partials[(long)q * nb + b], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int sh = b & 7;
        const unsigned in_shard = (unsigned)((nb + 7 - sh) >> 3);
        unsigned *base = mticket + (size_t)q * MT_WORDS, *mine_t = base + sh * MT_STRIDE, *top_t = base + 8 * MT_STRIDE;
        int last = 0;
        if (__hip_atomic_fetch_add(mine_t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_shard - 1) {
            __hip_atomic_store(mine_t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned shards = (unsigned)(nb < 8 ? nb : 8);
            last = __hip_atomic_fetch_add(top_t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1;
            if (last) __hip_atomic_store(top_t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    double t = 0.0;
    for (int bb = threadIdx.x; bb < nb; bb += BLK)
        t += __hip_atomic_load(&partials[(long)q * nb + bb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = block_sum(t);
    if (threadIdx.x == 0) out[q] = t;
}
// out[q] = sum_b partials[q*nb + b]; one workgroup per value (grid = nv)
__global__ __launch_bounds__(BLK) void k_reduce_multi(const double *__restrict__ partials, int nb, int nv,
                                                      double *__restrict__ out) {
    const int q = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += BLK) s += partials[(long)q * nb + b];
    s = block_sum(s);
    if (threadIdx.x == 0) out[q] = s;
}
// w -= sum_q h[q] V_q ; acc[q] += h[q]  (device-resident coefficients)
// NORM (round 6): also |w|^2 of the updated vector (the beta of the Lanczos step) -> nrm_out, finished by the last workgroup
// (reduce_tail) or, without a ticket, left as gridDim.x partial sums for k_reduce_multi.
template <bool NORM>
__global__ __launch_bounds__(BLK) void k_multi_axpy(const double *__restrict__ V, long stride, int nv,
                                                    const double *__restrict__ h, double *__restrict__ w, long off,
                                                    long n, const double *__restrict__ hprev, double *__restrict__ alpha,
                                                    double *__restrict__ nrm_part, unsigned *ticket, double *__restrict__ nrm_out) {
    // Lanczos, second Gram-Schmidt pass: alpha[j] = h1[j] + h2[j] with j = nv - 1
    if (hprev && blockIdx.x == 0 && threadIdx.x == 0) alpha[nv - 1] = hprev[nv - 1] + h[nv - 1];
    double nrm = 0.0;
    for (long i = blockIdx.x * (long)BLK + threadIdx.x; i < n; i += (long)gridDim.x * BLK) {
        double acc = w[off + i];
        for (int q = 0; q < nv; q++) acc = fma(-h[q], V[(long)q * stride + off + i], acc);
        w[off + i] = acc;
        if (NORM) nrm = fma(acc, acc, nrm);
    }
    if (NORM) {
        const double v[1] = {block_sum(nrm)};
        reduce_tail<1>(v, nrm_part, gridDim.x, blockIdx.x, ticket, nrm_out);
    }
}
// alpha[j] = h1[j] + h2[j]
__global__ void k_lanczos_alpha(const double *__restrict__ h1, const double *__restrict__ h2, int j,
                                double *__restrict__ alpha) {
    if (threadIdx.x == 0 && blockIdx.x == 0) alpha[j] = h1[j] + h2[j];
}
// beta[j] = sqrt(bb[0]);  v_next = w / beta;  t = dis .* v_next (the scaled input of the next operator application)
__global__ __launch_bounds__(BLK) void k_lanczos_next(const double *__restrict__ w, const double *__restrict__ bb, int j,
                                                      double *__restrict__ beta, double *__restrict__ vnext, long off,
                                                      long n, const double *__restrict__ dis, double *__restrict__ t) {
    const double bt = sqrt(bb[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) beta[j] = bt;
    const double inv = bt > 0.0 ? 1.0 / bt : 0.0;
    for (long i = blockIdx.x * (long)BLK + threadIdx.x; i < n; i += (long)gridDim.x * BLK) {
        const double v = w[off + i] * inv;
        vnext[off + i] = v;
        t[off + i] = dis[off + i] * v;
    }
}

// largest eigenvalue of a symmetric tridiagonal matrix, Sturm bisection
inline double tridiag_lmax(int m, const double *a, const double *b) {
    double lo = a[0], hi = a[0];
    for (int i = 0; i < m; i++) {
        double rad = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i < m - 1 ? fabs(b[i]) : 0.0);
        lo = fmin(lo, a[i] - rad);
        hi = fmax(hi, a[i] + rad);
    }
    for (int it = 0; it < 200; it++) {
        double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        int cnt = 0;
        double q = a[0] - mid;
        if (q < 0) cnt++;
        for (int i = 1; i < m; i++) {
            double den = (fabs(q) < 1e-300) ? 1e-300 : q;
            q = a[i] - mid - b[i - 1] * b[i - 1] / den;
            if (q < 0) cnt++;
        }
        if (cnt >= m) hi = mid;
        else lo = mid;
    }
    return 0.5 * (lo + hi);
}

// smallest eigenvalue of a symmetric tridiagonal matrix, Sturm bisection
inline double tridiag_lmin(int m, const double *a, const double *b) {
    double lo = a[0], hi = a[0];
    for (int i = 0; i < m; i++) {
        double rad = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i < m - 1 ? fabs(b[i]) : 0.0);
        lo = fmin(lo, a[i] - rad);
        hi = fmax(hi, a[i] + rad);
    }
    for (int it = 0; it < 200; it++) {
        double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        int cnt = 0;
        double q = a[0] - mid;
        if (q < 0) cnt++;
        for (int i = 1; i < m; i++) {
            double den = (fabs(q) < 1e-300) ? 1e-300 : q;
            q = a[i] - mid - b[i - 1] * b[i - 1] / den;
            if (q < 0) cnt++;
        }
        if (cnt >= 1) hi = mid;
        else lo = mid;
    }
    return 0.5 * (lo + hi);
}

// lambda_max(diag(KE)^-1 KE) by cyclic Jacobi rotations (n <= 24): the rigorous,
// density-independent Chebyshev bound of the matrix-free level
inline double elem_lambda_bound(int n, const double *KE) {
    std::vector<double> S((size_t)n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) S[i * n + j] = 0.5 * (KE[i * n + j] + KE[j * n + i]) / sqrt(KE[i * n + i] * KE[j * n + j]);
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) off += S[p * n + q] * S[p * n + q];
        if (off < 1e-30) break;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                double apq = S[p * n + q];
                if (fabs(apq) < 1e-300) continue;
                double th = (S[q * n + q] - S[p * n + p]) / (2.0 * apq);
                double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) {
                    double akp = S[k * n + p], akq = S[k * n + q];
                    S[k * n + p] = c * akp - s * akq;
                    S[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {
                    double apk = S[p * n + k], aqk = S[q * n + k];
                    S[p * n + k] = c * apk - s * aqk;
                    S[q * n + k] = s * apk + c * aqk;
                }
            }
    }
    double l = S[0];
    for (int i = 1; i < n; i++) l = fmax(l, S[i * n + i]);
    return l;
}
