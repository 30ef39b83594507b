// robust.h -- robust three-field formulation (Wang, Lazarov, Sigmund, SMO 43, 2011): one filtered field xTilde projected at up to
// three thresholds with one beta -- the eroded, the nominal and the dilated design -- and the chain rule back.
// Included from topopt_amd.hip behind passive.h.
//
//   k_robust_project<NP>  out[k][i] = H(xTilde[i]; beta, eta_k), k < NP: xTilde read once per element for all NP fields.  The
//                         expression is k_heaviside's (filter.h) in the same association, den and t0 evaluated on the device by every
//                         thread before its grid-stride loop, so each field has the bits of a k_heaviside launch at its threshold.
//                         One tanh per field and element: the addition theorem would share tanh(beta x) between the thresholds,
//                         but at beta = 48 it divides 0 by 0.  With labels a void element receives 0.0 and a solid one 1.0 in all
//                         NP fields (the projection followed by tp_passive_impose(.., 0, 1)); with partials the NP sums of the
//                         values as stored leave through block_sum, [field][workgroup].
//   k_robust_chain<NR>    rows[r][i] *= beta (1 - tanh^2(beta (xTilde[i] - eta_r))) / den_r, k_heaviside_chain's expression; the
//                         factor is evaluated once per DISTINCT threshold (at most 3) and element, the rows pick theirs by an index
//                         the host made.  With labels the passive entries of every row are stored as +0.0 (the chain followed by
//                         tp_passive_zero).  All loads of an element are issued before its first store.
// Grid-stride, one element per thread and pass, unit stride on every stream.  Plain loads and stores: the assembly (project) and the
// filter's transpose (chain) read the fields next.  No LDS beyond block_sum's, no atomics.  NP / NR are template parameters: the
// pointer tables travel by value and are indexed by constants only.
#pragma once

struct RobustFields {
    double *v[TP_ROBUST_MAXPROJ];
    double eta[TP_ROBUST_MAXPROJ];
};
struct RobustRows {
    double *v[TP_ROBUST_MAXROWS];
    int which[TP_ROBUST_MAXROWS];  // row -> index into eta
    double eta[TP_ROBUST_MAXPROJ];
    int neta;
};

template <int NP, bool LAB, bool SUM>
__global__ __launch_bounds__(BLK) void k_robust_project(RobustFields a, const double *__restrict__ x, const uint8_t *__restrict__ label,
                                                        double beta, long n, double *__restrict__ partials) {
    double den[NP], t0[NP], s[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
        den[k] = tanh(beta * a.eta[k]) + tanh(beta * (1.0 - a.eta[k]));
        t0[k] = tanh(beta * a.eta[k]);
        s[k] = 0.0;
    }
    for (long i = blockIdx.x * (long)BLK + threadIdx.x; i < n; i += (long)gridDim.x * BLK) {
        const unsigned l = LAB ? label[i] : 0u;
        if (LAB && l) {
            const double val = l == 1 ? 0.0 : 1.0;
#pragma unroll
            for (int k = 0; k < NP; k++) {
                a.v[k][i] = val;
                if (SUM) s[k] += val;
            }
            continue;
        }
        const double xi = x[i];
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const double val = (t0[k] + tanh(beta * (xi - a.eta[k]))) / den[k];
            a.v[k][i] = val;
            if (SUM) s[k] += val;
        }
    }
    if (SUM) {
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const double t = block_sum(s[k]);
            if (threadIdx.x == 0) partials[(long)k * gridDim.x + blockIdx.x] = t;
        }
    }
}

template <int NR, bool LAB>
__global__ __launch_bounds__(BLK) void k_robust_chain(RobustRows a, const double *__restrict__ xt, const uint8_t *__restrict__ label,
                                                      double beta, long n) {
    double den[TP_ROBUST_MAXPROJ];
#pragma unroll
    for (int k = 0; k < TP_ROBUST_MAXPROJ; k++)
        den[k] = k < a.neta ? tanh(beta * a.eta[k]) + tanh(beta * (1.0 - a.eta[k])) : 1.0;
    for (long i = blockIdx.x * (long)BLK + threadIdx.x; i < n; i += (long)gridDim.x * BLK) {
        if (LAB && label[i]) {
#pragma unroll
            for (int r = 0; r < NR; r++) a.v[r][i] = 0.0;
            continue;
        }
        const double xi = xt[i];
        double row[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) row[r] = a.v[r][i];
        double f[TP_ROBUST_MAXPROJ];
#pragma unroll
        for (int k = 0; k < TP_ROBUST_MAXPROJ; k++) {
            f[k] = 0.0;
            if (k < a.neta) {
                const double th = tanh(beta * (xi - a.eta[k]));
                f[k] = beta * (1.0 - th * th) / den[k];
            }
        }
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int w = a.which[r];
            a.v[r][i] = row[r] * (w == 0 ? f[0] : (w == 1 ? f[1] : f[2]));
        }
    }
}

// what both calls ask of their scalars and pointer tables; vecs[k] != xTilde, pairwise distinct
static int robust_check(const tp_grid *g, const double *xTilde, double beta, int n, int nmax, const double *eta, double *const *vecs,
                        const tp_passive *p) {
    if (!g || !xTilde || !eta || !vecs || n < 1 || n > nmax) return TP_ERR_ARG;
    if (!(beta > 0.0) || !std::isfinite(beta)) return TP_ERR_ARG;
    for (int k = 0; k < n; k++) {
        if (!(eta[k] >= 0.0 && eta[k] <= 1.0)) return TP_ERR_ARG;
        if (!vecs[k] || vecs[k] == xTilde) return TP_ERR_ARG;
        for (int j = 0; j < k; j++)
            if (vecs[j] == vecs[k]) return TP_ERR_ARG;
    }
    if (p && p->grid != g) return TP_ERR_ARG;
    return TP_OK;
}

extern "C" int tp_robust_project(tp_grid *g, const double *xTilde, double beta, int nproj, const double *eta, double *const *out,
                                 const tp_passive *p, double *sums) {
    TP_TRY(robust_check(g, xTilde, beta, nproj, TP_ROBUST_MAXPROJ, eta, out, p));
    const long n = (long)g->ex * g->ey * g->ez_own;
    const bool lab = p && p->n_void + p->n_solid > 0;
    if (p && p->n != n) return TP_ERR_ARG;
    RobustFields a{};
    for (int k = 0; k < nproj; k++) a.v[k] = out[k], a.eta[k] = eta[k];
    const int nb = grid_for(n);  // <= 2048 workgroups: nproj partials each fit the grid's 4 x MAX_RED_BLOCKS
    const uint8_t *label = lab ? (const uint8_t *)p->label : nullptr;
    double *partials = sums ? (double *)g->partials : nullptr;
#define TP_ROBUST_GO(NP, LAB, SUM) \
    TP_LAUNCH((k_robust_project<NP, LAB, SUM>), dim3(nb), dim3(BLK), 0, g->stream, a, xTilde, label, beta, n, partials)
#define TP_ROBUST_NP(NP)                  \
    do {                                  \
        if (lab && sums) {                \
            TP_ROBUST_GO(NP, true, true); \
        } else if (lab) {                 \
            TP_ROBUST_GO(NP, true, false);\
        } else if (sums) {                \
            TP_ROBUST_GO(NP, false, true);\
        } else {                          \
            TP_ROBUST_GO(NP, false, false);\
        }                                 \
    } while (0)
    switch (nproj) {
        case 1: TP_ROBUST_NP(1); break;
        case 2: TP_ROBUST_NP(2); break;
        default: TP_ROBUST_NP(3); break;
    }
#undef TP_ROBUST_NP
#undef TP_ROBUST_GO
    count_launch(g, 8.0 * n * (1 + nproj) + (lab ? 1.0 * n : 0.0), 12.0 * n * nproj);
    if (sums) {
        TP_TRY(reduce_partials_n(g, g->partials, nb, nproj, S_TMP));
        TP_TRY(read_scal(g, S_TMP, nproj, sums));
    }
    return TP_OK;
}

extern "C" int tp_robust_chain(tp_grid *g, const double *xTilde, double beta, int nrows, double *const *rows, const double *eta_row,
                               const tp_passive *p) {
    TP_TRY(robust_check(g, xTilde, beta, nrows, TP_ROBUST_MAXROWS, eta_row, rows, p));
    RobustRows a{};
    for (int r = 0; r < nrows; r++) {  // the distinct thresholds, in order of first appearance
        int k = 0;
        while (k < a.neta && a.eta[k] != eta_row[r]) k++;
        if (k == a.neta) {
            if (a.neta == TP_ROBUST_MAXPROJ) return TP_ERR_ARG;
            a.eta[a.neta++] = eta_row[r];
        }
        a.v[r] = rows[r], a.which[r] = k;
    }
    const long n = (long)g->ex * g->ey * g->ez_own;
    const bool lab = p && p->n_void + p->n_solid > 0;
    if (p && p->n != n) return TP_ERR_ARG;
    const uint8_t *label = lab ? (const uint8_t *)p->label : nullptr;
#define TP_ROBUST_GO(NR)                                                                                                  \
    do {                                                                                                                  \
        if (lab)                                                                                                          \
            TP_LAUNCH((k_robust_chain<NR, true>), dim3(grid_for(n)), dim3(BLK), 0, g->stream, a, xTilde, label, beta, n);  \
        else                                                                                                              \
            TP_LAUNCH((k_robust_chain<NR, false>), dim3(grid_for(n)), dim3(BLK), 0, g->stream, a, xTilde, label, beta, n); \
    } while (0)
    switch (nrows) {
        case 1: TP_ROBUST_GO(1); break;
        case 2: TP_ROBUST_GO(2); break;
        case 3: TP_ROBUST_GO(3); break;
        case 4: TP_ROBUST_GO(4); break;
        case 5: TP_ROBUST_GO(5); break;
        case 6: TP_ROBUST_GO(6); break;
        case 7: TP_ROBUST_GO(7); break;
        default: TP_ROBUST_GO(8); break;
    }
#undef TP_ROBUST_GO
    count_launch(g, 8.0 * n * (1 + 2 * nrows) + (lab ? 1.0 * n : 0.0), (12.0 * a.neta + nrows) * n);
    return TP_OK;
}
