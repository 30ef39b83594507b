// blockvec.h -- two passes over a block of q <= TP_MAX_CASES vectors, for the Rayleigh-Ritz step of the subspace iteration
// (DESIGN.md 4.14).  Included from topopt_amd.hip behind mass.h.
//   k_block_gram<Q>     G_ij = X_i . Y_j for all Q^2 pairs in ONE pass: every vector is read once (2 Q n doubles against the
//                       2 Q^2 n of Q^2 dot products), Q^2 accumulators per thread, block_sum per value, then the deterministic
//                       reduce_tail (last workgroup to arrive, fixed order) and the sum over the ranks tp_vec_dot uses.  Each
//                       product is one fma into its own accumulator in index order: with X == Y the entries (i, j) and (j, i)
//                       see the same products in the same order and are equal bit for bit; two calls give the same bits.
//   k_block_combine<Q>  Z_i = sum_j Q_ji Y_j for Q vectors in one pass (Q loads, Q stores per entry), the Q^2 host coefficients
//                       passed by value.  Z must not overlap Y.
// Q is a template parameter: the accumulators and the coefficient table are indexed by constants only and stay in registers.
#pragma once

constexpr int GRAM_BLOCKS = 512;  // 64 values x 512 workgroups of partial sums
// the sums come back through the grid's pinned mirror h_scal (64 doubles, tp_grid_create) and its device buffer holds 64 sums
static_assert(TP_MAX_CASES * TP_MAX_CASES <= 64, "tp_vec_block_gram: q^2 sums must fit h_scal and the head of tp_grid::gram");

struct BlockPtrs {
    const double *X[TP_MAX_CASES];
    const double *Y[TP_MAX_CASES];
};
struct CombineArgs {
    const double *Y[TP_MAX_CASES];
    double *Z[TP_MAX_CASES];
    double c[TP_MAX_CASES * TP_MAX_CASES];  // c[j * Q + i] = Q_ji
};

template <int Q>
__global__ __launch_bounds__(BLK) void k_block_gram(BlockPtrs a, long n, double *__restrict__ partials, unsigned *ticket,
                                                    double *__restrict__ out) {
    double s[Q * Q];
#pragma unroll
    for (int v = 0; v < Q * Q; v++) s[v] = 0.0;
    for (long r = blockIdx.x * (long)BLK + threadIdx.x; r < n; r += (long)gridDim.x * BLK) {
        double x[Q], y[Q];
#pragma unroll
        for (int i = 0; i < Q; i++) x[i] = a.X[i][r];
#pragma unroll
        for (int j = 0; j < Q; j++) y[j] = a.Y[j][r];
#pragma unroll
        for (int i = 0; i < Q; i++)
#pragma unroll
            for (int j = 0; j < Q; j++) s[i * Q + j] = fma(x[i], y[j], s[i * Q + j]);
    }
    double v[Q * Q];
#pragma unroll
    for (int k = 0; k < Q * Q; k++) v[k] = block_sum(s[k]);
    reduce_tail<Q * Q>(v, partials, gridDim.x, blockIdx.x, ticket, out);
}

template <int Q>
__global__ __launch_bounds__(BLK) void k_block_combine(CombineArgs a, long n) {
    for (long r = blockIdx.x * (long)BLK + threadIdx.x; r < n; r += (long)gridDim.x * BLK) {
        double y[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) y[j] = a.Y[j][r];
#pragma unroll
        for (int i = 0; i < Q; i++) {
            double z = a.c[i] * y[0];
#pragma unroll
            for (int j = 1; j < Q; j++) z = fma(a.c[j * Q + i], y[j], z);
            a.Z[i][r] = z;
        }
    }
}

template <int Q>
static int block_gram_launch(tp_grid *g, const BlockPtrs &a, long n, int nb) {
    unsigned *ticket = tail_ticket(g);
    TP_LAUNCH(k_block_gram<Q>, dim3(nb), dim3(BLK), 0, g->stream, a, n, g->gram + 64, ticket, (double *)g->gram);
    count_launch(g, 16.0 * Q * n, 2.0 * Q * Q * n);
    if (!ticket) {  // TP_NO_REDUCE_TAIL: the partial sums alone were left
        TP_LAUNCH(k_reduce_final_n, dim3(1), dim3(BLK), 0, g->stream, (const double *)(g->gram + 64), nb, Q * Q, (double *)g->gram);
        count_launch(g);
    }
    return TP_OK;
}
template <int Q>
static int block_combine_launch(tp_grid *g, const CombineArgs &a, long n) {
    TP_LAUNCH(k_block_combine<Q>, dim3(grid_for(n)), dim3(BLK), 0, g->stream, a, n);
    count_launch(g, 16.0 * Q * n, 2.0 * Q * Q * n);
    return TP_OK;
}

extern "C" int tp_vec_block_gram(tp_grid *g, int q, const double *const *X, const double *const *Y, long n, double *out_qq) {
    if (!g || !X || !Y || !out_qq || q < 1 || q > TP_MAX_CASES || n < 1) return TP_ERR_ARG;
    for (int i = 0; i < q; i++)
        if (!X[i] || !Y[i]) return TP_ERR_ARG;
    if (!g->gram) TP_TRY(g->gram.alloc(64 + 64 * (size_t)GRAM_BLOCKS));
    BlockPtrs a{};
    for (int i = 0; i < q; i++) a.X[i] = X[i], a.Y[i] = Y[i];
    const int nb = grid_for(n, GRAM_BLOCKS);
    switch (q) {
        case 1: TP_TRY(block_gram_launch<1>(g, a, n, nb)); break;
        case 2: TP_TRY(block_gram_launch<2>(g, a, n, nb)); break;
        case 3: TP_TRY(block_gram_launch<3>(g, a, n, nb)); break;
        case 4: TP_TRY(block_gram_launch<4>(g, a, n, nb)); break;
        case 5: TP_TRY(block_gram_launch<5>(g, a, n, nb)); break;
        case 6: TP_TRY(block_gram_launch<6>(g, a, n, nb)); break;
        case 7: TP_TRY(block_gram_launch<7>(g, a, n, nb)); break;
        default: TP_TRY(block_gram_launch<8>(g, a, n, nb)); break;
    }
    const int nv = q * q;
    if (g->has_comm) {  // the sum over the ranks, 16 values -- the hook's buffer -- at a time
        for (int o = 0; o < nv; o += 16) {
            const int cnt = nv - o < 16 ? nv - o : 16;
            CommMark cm(g, 2, g->stream);
            if (g->comm.allreduce_inplace) {
                if (g->comm.allreduce_inplace(g->comm.user, g->gram + o, cnt)) return TP_ERR_COMM;
            } else {
                TP_HIP(hipMemcpyAsync(g->comm.red, g->gram + o, sizeof(double) * cnt, hipMemcpyDeviceToDevice, g->stream));
                if (g->comm.allreduce_sum(g->comm.user, cnt)) return TP_ERR_COMM;
                TP_HIP(hipMemcpyAsync(g->gram + o, g->comm.red, sizeof(double) * cnt, hipMemcpyDeviceToDevice, g->stream));
            }
        }
    }
    // h_scal is also the target of read_scal_begin / read_scal_end (grid.h): those pairs open and close inside one library call
    // (the Krylov loop), never across calls, so no read is pending here; the copy is ordered behind them on the same stream anyway
    TP_HIP(hipMemcpyAsync(g->h_scal, (const double *)g->gram, sizeof(double) * nv, hipMemcpyDeviceToHost, g->stream));
    TP_HIP(hipStreamSynchronize(g->stream));
    for (int v = 0; v < nv; v++) out_qq[v] = g->h_scal[v];
    return TP_OK;
}

extern "C" int tp_vec_block_combine(tp_grid *g, int q, const double *const *Y, const double *Q_qq, double *const *Z, long n) {
    if (!g || !Y || !Q_qq || !Z || q < 1 || q > TP_MAX_CASES || n < 1) return TP_ERR_ARG;
    for (int i = 0; i < q; i++)
        if (!Y[i] || !Z[i]) return TP_ERR_ARG;
    const uintptr_t span = (uintptr_t)n * sizeof(double);
    for (int i = 0; i < q; i++) {
        const uintptr_t z = (uintptr_t)Z[i];
        for (int j = 0; j < q; j++)
            if (z < (uintptr_t)Y[j] + span && (uintptr_t)Y[j] < z + span) return TP_ERR_ARG;  // Z_i overlaps Y_j
        for (int j = 0; j < i; j++)
            if (z < (uintptr_t)Z[j] + span && (uintptr_t)Z[j] < z + span) return TP_ERR_ARG;  // ... or another output
    }
    CombineArgs a{};
    for (int i = 0; i < q; i++) a.Y[i] = Y[i], a.Z[i] = Z[i];
    for (int j = 0; j < q * q; j++) a.c[j] = Q_qq[j];
    switch (q) {
        case 1: return block_combine_launch<1>(g, a, n);
        case 2: return block_combine_launch<2>(g, a, n);
        case 3: return block_combine_launch<3>(g, a, n);
        case 4: return block_combine_launch<4>(g, a, n);
        case 5: return block_combine_launch<5>(g, a, n);
        case 6: return block_combine_launch<6>(g, a, n);
        case 7: return block_combine_launch<7>(g, a, n);
        default: return block_combine_launch<8>(g, a, n);
    }
}
