// passive.h -- passive regions: own elements whose density is fixed (label 1 void, 2 solid) beside the active ones (label 0) the
// optimiser moves.  Included from topopt_amd.hip behind overhang.h.
//
// The optimiser sees the active elements only, as a packed vector in ascending element order; the filter and the physics see
// the full field.  Four kernels move data between the two, several vectors per launch so that the labels / the index list are
// read once per element and not once per vector:
//   k_passive_impose<NV>   full[v][e] = value of e's label on passive e       (labels: 1 byte per element; active e not written)
//   k_passive_zero<NV>     full[v][e] = +0.0 on passive e                     (a store, not a product: NaN and -0.0 go as well)
//   k_passive_gather<NV>   packed[v][a] = full[v][idx[a]]
//   k_passive_scatter<NV>  full[v][idx[a]] = packed[v][a]                     (passive entries of full not written)
// Grid-stride, one element per thread and pass.  The packed side and idx are unit stride; the full side goes through idx, which
// ascends: a wave touches one run of 64 + (passive elements in between) doubles, whole lines wherever the active elements are
// contiguous.  All NV loads of an element are issued before the first store, so no store address has to be compared with a later
// load.  Plain loads and stores: what is written here is read by the next kernel of the iteration (MMA on the packed vectors,
// the filter on the full ones), so the lines should stay in the L2.  No LDS, no atomics.  NV is a template parameter: the pointer
// table travels by value and is indexed by constants only.
#pragma once

struct PassiveVecs {
    double *v[TP_PASSIVE_MAXVEC];
};
struct PassivePairs {
    const double *src[TP_PASSIVE_MAXVEC];
    double *dst[TP_PASSIVE_MAXVEC];
};

template <int NV>
__global__ __launch_bounds__(BLK) void k_passive_impose(PassiveVecs a, const uint8_t *__restrict__ label, long n, double v_void,
                                                        double v_solid) {
    for (long e = blockIdx.x * (long)BLK + threadIdx.x; e < n; e += (long)gridDim.x * BLK) {
        const unsigned l = label[e];
        if (!l) continue;
        const double val = l == 1 ? v_void : v_solid;
#pragma unroll
        for (int v = 0; v < NV; v++) a.v[v][e] = val;
    }
}
template <int NV>
__global__ __launch_bounds__(BLK) void k_passive_zero(PassiveVecs a, const uint8_t *__restrict__ label, long n) {
    for (long e = blockIdx.x * (long)BLK + threadIdx.x; e < n; e += (long)gridDim.x * BLK) {
        if (!label[e]) continue;
#pragma unroll
        for (int v = 0; v < NV; v++) a.v[v][e] = 0.0;
    }
}
template <int NV>
__global__ __launch_bounds__(BLK) void k_passive_gather(PassivePairs a, const int *__restrict__ idx, long na) {
    for (long t = blockIdx.x * (long)BLK + threadIdx.x; t < na; t += (long)gridDim.x * BLK) {
        const long e = idx[t];
        double r[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) r[v] = a.src[v][e];
#pragma unroll
        for (int v = 0; v < NV; v++) a.dst[v][t] = r[v];
    }
}
template <int NV>
__global__ __launch_bounds__(BLK) void k_passive_scatter(PassivePairs a, const int *__restrict__ idx, long na) {
    for (long t = blockIdx.x * (long)BLK + threadIdx.x; t < na; t += (long)gridDim.x * BLK) {
        const long e = idx[t];
        double r[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) r[v] = a.src[v][t];
#pragma unroll
        for (int v = 0; v < NV; v++) a.dst[v][e] = r[v];
    }
}

struct tp_passive {
    tp_grid *grid;
    long n, n_active, n_void, n_solid;  // own elements
    DevBuf<uint8_t> label;              // [dev] n labels
    DevBuf<int> idx;                    // [dev] n_active own element indices, ascending
};

// one switch for the four kernels: LAUNCH(NV) with NV a constant
#define TP_PASSIVE_DISPATCH(nvec, LAUNCH) \
    switch (nvec) {                       \
        case 1: LAUNCH(1); break;         \
        case 2: LAUNCH(2); break;         \
        case 3: LAUNCH(3); break;         \
        case 4: LAUNCH(4); break;         \
        case 5: LAUNCH(5); break;         \
        case 6: LAUNCH(6); break;         \
        case 7: LAUNCH(7); break;         \
        case 8: LAUNCH(8); break;         \
        case 9: LAUNCH(9); break;         \
        case 10: LAUNCH(10); break;       \
        case 11: LAUNCH(11); break;       \
        default: LAUNCH(12); break;       \
    }

extern "C" int tp_passive_destroy(tp_passive *p) {
    if (!p) return TP_OK;
    (void)hipStreamSynchronize(p->grid->stream);
    delete p;
    return TP_OK;
}
extern "C" int tp_passive_create(tp_passive **out, tp_grid *g, const unsigned char *label_host) {
    if (!out || !g || !label_host) return TP_ERR_ARG;
    const long n = (long)g->ex * g->ey * g->ez_own;
    if (n > 0x7fffffffL) return TP_ERR_ARG;  // the index list is int32
    std::vector<int> idx;
    long cnt[3] = {0, 0, 0};
    for (long e = 0; e < n; e++) {
        if (label_host[e] > 2) return TP_ERR_ARG;
        cnt[label_host[e]]++;
    }
    idx.reserve((size_t)cnt[0]);
    for (long e = 0; e < n; e++)
        if (!label_host[e]) idx.push_back((int)e);
    std::unique_ptr<tp_passive> p(new tp_passive());
    p->grid = g;
    p->n = n, p->n_active = cnt[0], p->n_void = cnt[1], p->n_solid = cnt[2];
    TP_TRY(p->label.alloc((size_t)n));
    TP_HIP(hipMemcpy(p->label, label_host, (size_t)n, hipMemcpyHostToDevice));
    if (cnt[0]) {
        TP_TRY(p->idx.alloc(idx.size()));
        TP_HIP(hipMemcpy(p->idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice));
    }
    *out = p.release();
    return TP_OK;
}
extern "C" int tp_passive_counts(const tp_passive *p, long *n_active, long *n_void, long *n_solid) {
    if (!p) return TP_ERR_ARG;
    if (n_active) *n_active = p->n_active;
    if (n_void) *n_void = p->n_void;
    if (n_solid) *n_solid = p->n_solid;
    return TP_OK;
}

static int passive_check_vecs(int nvec, const double *const *a, const double *const *b) {
    if (!a || nvec < 1 || nvec > TP_PASSIVE_MAXVEC) return TP_ERR_ARG;
    for (int v = 0; v < nvec; v++)
        if (!a[v] || (b && !b[v])) return TP_ERR_ARG;
    if (b)
        for (int v = 0; v < nvec; v++)
            for (int w = 0; w < nvec; w++)
                if (a[v] == b[w]) return TP_ERR_ARG;
    return TP_OK;
}

extern "C" int tp_passive_impose(tp_passive *p, int nvec, double *const *x, double v_void, double v_solid) {
    if (!p) return TP_ERR_ARG;
    TP_TRY(passive_check_vecs(nvec, x, nullptr));
    const long np = p->n_void + p->n_solid;
    if (!np) return TP_OK;
    tp_grid *g = p->grid;
    PassiveVecs a{};
    for (int v = 0; v < nvec; v++) a.v[v] = x[v];
#define TP_PASSIVE_GO(NV) \
    TP_LAUNCH(k_passive_impose<NV>, dim3(grid_for(p->n)), dim3(BLK), 0, g->stream, a, (const uint8_t *)p->label, p->n, v_void, v_solid)
    TP_PASSIVE_DISPATCH(nvec, TP_PASSIVE_GO)
#undef TP_PASSIVE_GO
    count_launch(g, 1.0 * p->n + 8.0 * nvec * np, 0.0);
    return TP_OK;
}
extern "C" int tp_passive_zero(tp_passive *p, int nvec, double *const *rows) {
    if (!p) return TP_ERR_ARG;
    TP_TRY(passive_check_vecs(nvec, rows, nullptr));
    const long np = p->n_void + p->n_solid;
    if (!np) return TP_OK;
    tp_grid *g = p->grid;
    PassiveVecs a{};
    for (int v = 0; v < nvec; v++) a.v[v] = rows[v];
#define TP_PASSIVE_GO(NV) TP_LAUNCH(k_passive_zero<NV>, dim3(grid_for(p->n)), dim3(BLK), 0, g->stream, a, (const uint8_t *)p->label, p->n)
    TP_PASSIVE_DISPATCH(nvec, TP_PASSIVE_GO)
#undef TP_PASSIVE_GO
    count_launch(g, 1.0 * p->n + 8.0 * nvec * np, 0.0);
    return TP_OK;
}
extern "C" int tp_passive_gather(tp_passive *p, int nvec, const double *const *full, double *const *packed) {
    if (!p || !packed) return TP_ERR_ARG;
    TP_TRY(passive_check_vecs(nvec, full, packed));
    if (!p->n_active) return TP_OK;
    tp_grid *g = p->grid;
    PassivePairs a{};
    for (int v = 0; v < nvec; v++) a.src[v] = full[v], a.dst[v] = packed[v];
#define TP_PASSIVE_GO(NV) \
    TP_LAUNCH(k_passive_gather<NV>, dim3(grid_for(p->n_active)), dim3(BLK), 0, g->stream, a, (const int *)p->idx, p->n_active)
    TP_PASSIVE_DISPATCH(nvec, TP_PASSIVE_GO)
#undef TP_PASSIVE_GO
    count_launch(g, (4.0 + 16.0 * nvec) * p->n_active, 0.0);
    return TP_OK;
}
extern "C" int tp_passive_scatter(tp_passive *p, int nvec, const double *const *packed, double *const *full) {
    if (!p || !packed) return TP_ERR_ARG;
    TP_TRY(passive_check_vecs(nvec, full, packed));
    if (!p->n_active) return TP_OK;
    tp_grid *g = p->grid;
    PassivePairs a{};
    for (int v = 0; v < nvec; v++) a.src[v] = packed[v], a.dst[v] = full[v];
#define TP_PASSIVE_GO(NV) \
    TP_LAUNCH(k_passive_scatter<NV>, dim3(grid_for(p->n_active)), dim3(BLK), 0, g->stream, a, (const int *)p->idx, p->n_active)
    TP_PASSIVE_DISPATCH(nvec, TP_PASSIVE_GO)
#undef TP_PASSIVE_GO
    count_launch(g, (4.0 + 16.0 * nvec) * p->n_active, 0.0);
    return TP_OK;
}
#undef TP_PASSIVE_DISPATCH
