// link.h -- design-variable linking: mirror symmetry, pattern repetition, extrusion.  Included from
// topopt_amd.hip behind passive.h.
//
// Every axis carries one mode; the reduced design lives on the box nr_x x nr_y x nr_z in natural order (x fastest), and the orbit
// of a reduced variable is the product of its three per-axis preimages.  The optimiser sees the reduced vector; the filter and the
// physics see the full field.  Three linear maps, several vectors per launch:
//   k_link_expand<NV>   full[v][e] = red[v][r(e)]                              (moves bytes)
//   k_link_pick<NV>     red[v][j]  = full[v][first member of orbit(j)]         (moves bytes)
//   k_link_fold<NV>     red[v][j]  = sum of full[v][e] over orbit(j)           (form 1: one reduced variable per thread)
//   k_link_fold_x<NV>   the same sum for an x mode other than none             (form 2: whole x rows staged through LDS)
// The sum has ONE order in every form: sequential, ascending natural element order (z outer, then y, then x), the accumulator
// started with the first member's value (not 0.0: an orbit of -0.0 stays -0.0), plain IEEE adds, no contraction possible (there
// is no product).  So both forms equal a float64 restatement of that loop bit for bit, and no atomics are involved.
// Indices are arithmetic on a per-axis descriptor (mode, ne, nr) that travels by value: no device index arrays.  All NV loads of
// an output are issued before its stores; plain loads and stores: what is written here is read by the next kernel of the
// iteration (MMA on the reduced vectors, the filter on the full ones).  NV is a template parameter: the pointer table travels
// by value and is indexed by constants only.
//
// Form 2.  In form 1 a lane walks its x-preimages in its own row: under x:extrude the lanes of a wave read runs that lie ex
// doubles apart, every lane its own line.  Form 2 gives a workgroup R reduced rows (Iy, Iz) with R nr_x <= BLK threads, one per
// reduced variable; for every (z, y) of the rows' preimages, z outer, it loads the R full rows with consecutive lanes on
// consecutive doubles into LDS, and each thread adds its x-preimages from there, ascending.  Rows whose preimage is shorter (a
// mirror's centre) sit a step out.  The staging buffer holds LINK_TILE doubles shared by the NV vectors, rows at an odd pitch
// (ex | 1: lanes that read a column of rows hit distinct banks), so the form applies while ex <= LINK_ROW_CAP = 512 -- then
// also nr_x <= 256 = BLK for every mode but none; above the cap form 1 runs.
#pragma once

constexpr int LINK_ROW_CAP = 512;                                   // form 2: longest x row staged
constexpr int LINK_TILE = TP_LINK_MAXVEC * (LINK_ROW_CAP | 1);      // doubles of LDS per workgroup (49 248 bytes)

struct LinkAxis {
    int mode, ne, nr;   // 0 none, 1 mirror, 2 repeat (period nr), 3 extrude
};
struct LinkDesc {
    LinkAxis x, y, z;
};
struct LinkPairs {
    const double *src[TP_LINK_MAXVEC];
    double *dst[TP_LINK_MAXVEC];
};

// r(i)
__host__ __device__ inline int link_reduced(const LinkAxis a, int i) {
    return a.mode == 0 ? i : a.mode == 1 ? min(i, a.ne - 1 - i) : a.mode == 2 ? i % a.nr : 0;
}
// the preimage of I, ascending: first + k stride, k < cnt
__host__ __device__ inline void link_preimage(const LinkAxis a, int I, int &first, int &stride, int &cnt) {
    first = a.mode == 3 ? 0 : I;
    stride = a.mode == 1 ? a.ne - 1 - 2 * I : a.mode == 2 ? a.nr : 1;
    cnt = a.mode == 0 ? 1 : a.mode == 1 ? (stride ? 2 : 1) : a.mode == 2 ? a.ne / a.nr : a.ne;
}

template <int NV>
__global__ __launch_bounds__(BLK) void k_link_expand(LinkPairs a, LinkDesc d, long n) {
    for (long e = blockIdx.x * (long)BLK + threadIdx.x; e < n; e += (long)gridDim.x * BLK) {
        const long row = e / d.x.ne;
        const int i = (int)(e - row * d.x.ne), k = (int)(row / d.y.ne), j = (int)(row - (long)k * d.y.ne);
        const long s = ((long)link_reduced(d.z, k) * d.y.nr + link_reduced(d.y, j)) * d.x.nr + link_reduced(d.x, i);
        double r[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) r[v] = a.src[v][s];
#pragma unroll
        for (int v = 0; v < NV; v++) a.dst[v][e] = r[v];
    }
}
template <int NV>
__global__ __launch_bounds__(BLK) void k_link_pick(LinkPairs a, LinkDesc d, long nred) {
    for (long t = blockIdx.x * (long)BLK + threadIdx.x; t < nred; t += (long)gridDim.x * BLK) {
        const long row = t / d.x.nr;
        const int I = (int)(t - row * d.x.nr), K = (int)(row / d.y.nr), J = (int)(row - (long)K * d.y.nr);
        const long e = ((long)(d.z.mode == 3 ? 0 : K) * d.y.ne + (d.y.mode == 3 ? 0 : J)) * d.x.ne + (d.x.mode == 3 ? 0 : I);
        double r[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) r[v] = a.src[v][e];
#pragma unroll
        for (int v = 0; v < NV; v++) a.dst[v][t] = r[v];
    }
}
template <int NV>
__global__ __launch_bounds__(BLK) void k_link_fold(LinkPairs a, LinkDesc d, long nred) {
    for (long t = blockIdx.x * (long)BLK + threadIdx.x; t < nred; t += (long)gridDim.x * BLK) {
        const long row = t / d.x.nr;
        const int I = (int)(t - row * d.x.nr), K = (int)(row / d.y.nr), J = (int)(row - (long)K * d.y.nr);
        int fx, sx, cx, fy, sy, cy, fz, sz, cz;
        link_preimage(d.x, I, fx, sx, cx);
        link_preimage(d.y, J, fy, sy, cy);
        link_preimage(d.z, K, fz, sz, cz);
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) acc[v] = 0.0;
        bool fresh = true;
        for (int kz = 0; kz < cz; kz++)
            for (int ky = 0; ky < cy; ky++) {
                const long base = ((long)(fz + kz * sz) * d.y.ne + (fy + ky * sy)) * d.x.ne + fx;
                for (int kx = 0; kx < cx; kx++) {
                    const long e = base + (long)kx * sx;
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        const double val = a.src[v][e];
                        acc[v] = fresh ? val : acc[v] + val;
                    }
                    fresh = false;
                }
            }
#pragma unroll
        for (int v = 0; v < NV; v++) a.dst[v][t] = acc[v];
    }
}
// form 2: R reduced rows per workgroup and pass, thread tid <-> (row tid / nr_x, reduced x index tid % nr_x)
template <int NV>
__global__ __launch_bounds__(BLK) void k_link_fold_x(LinkPairs a, LinkDesc d, int R, long nrows) {
    __shared__ double tile[LINK_TILE];
    const int ex = d.x.ne, pitch = ex | 1, seg = R * pitch;   // NV seg <= LINK_TILE by the host's choice of R
    const int tr = threadIdx.x / d.x.nr, I = threadIdx.x - tr * d.x.nr;
    int fx, sx, cx;
    link_preimage(d.x, I, fx, sx, cx);
    int cymax, czmax, f_, s_;
    link_preimage(d.y, 0, f_, s_, cymax);   // (a mirror's first index has both members unless the axis has one element)
    link_preimage(d.z, 0, f_, s_, czmax);
    for (long q0 = (long)blockIdx.x * R; q0 < nrows; q0 += (long)gridDim.x * R) {
        const long q = q0 + tr;
        const bool mine = tr < R && q < nrows;
        int fy = 0, sy = 0, cy = 0, fz = 0, sz = 0, cz = 0;
        if (mine) {
            const int K = (int)(q / d.y.nr), J = (int)(q - (long)K * d.y.nr);
            link_preimage(d.y, J, fy, sy, cy);
            link_preimage(d.z, K, fz, sz, cz);
        }
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) acc[v] = 0.0;
        bool fresh = true;
        for (int kz = 0; kz < czmax; kz++)
            for (int ky = 0; ky < cymax; ky++) {
                __syncthreads();   // the previous step's reads are done
                for (int idx = threadIdx.x; idx < R * ex; idx += BLK) {
                    const int r = idx / ex, i = idx - r * ex;
                    const long qr = q0 + r;
                    if (qr >= nrows) break;   // (r ascends with idx: nothing further for this thread)
                    const int K = (int)(qr / d.y.nr), J = (int)(qr - (long)K * d.y.nr);
                    int gy, ty, ny, gz, tz, nz;
                    link_preimage(d.y, J, gy, ty, ny);
                    link_preimage(d.z, K, gz, tz, nz);
                    if (ky >= ny || kz >= nz) continue;
                    const long e = ((long)(gz + kz * tz) * d.y.ne + (gy + ky * ty)) * ex + i;
                    double val[NV];
#pragma unroll
                    for (int v = 0; v < NV; v++) val[v] = a.src[v][e];
#pragma unroll
                    for (int v = 0; v < NV; v++) tile[v * seg + r * pitch + i] = val[v];
                }
                __syncthreads();
                if (mine && ky < cy && kz < cz) {
                    const double *rowp = tile + tr * pitch + fx;
                    for (int kx = 0; kx < cx; kx++) {
#pragma unroll
                        for (int v = 0; v < NV; v++) {
                            const double val = rowp[v * seg + kx * sx];
                            acc[v] = fresh ? val : acc[v] + val;
                        }
                        fresh = false;
                    }
                }
            }
        if (mine) {
#pragma unroll
            for (int v = 0; v < NV; v++) a.dst[v][q * d.x.nr + I] = acc[v];
        }
    }
}

struct tp_link {
    tp_grid *grid;
    LinkDesc d;
    int cells[3];
    long n, nred;   // own elements, own reduced variables
    int form, last_form;
};

#define TP_LINK_DISPATCH(nvec, LAUNCH) \
    switch (nvec) {                    \
        case 1: LAUNCH(1); break;      \
        case 2: LAUNCH(2); break;      \
        case 3: LAUNCH(3); break;      \
        case 4: LAUNCH(4); break;      \
        case 5: LAUNCH(5); break;      \
        case 6: LAUNCH(6); break;      \
        case 7: LAUNCH(7); break;      \
        case 8: LAUNCH(8); break;      \
        case 9: LAUNCH(9); break;      \
        case 10: LAUNCH(10); break;    \
        case 11: LAUNCH(11); break;    \
        default: LAUNCH(12); break;    \
    }

extern "C" int tp_link_destroy(tp_link *l) {
    delete l;   // (holds no device memory: nothing in flight reads it)
    return TP_OK;
}
extern "C" int tp_link_create(tp_link **out, tp_grid *g, const int mode[3], const int cells[3]) {
    if (!out || !g || !mode || !cells) return TP_ERR_ARG;
    const int ne[3] = {g->ex, g->ey, g->ez_own};
    LinkAxis ax[3];
    for (int a = 0; a < 3; a++) {
        if (mode[a] < 0 || mode[a] > 3) return TP_ERR_ARG;
        if (mode[a] == 2 && (cells[a] < 2 || ne[a] % cells[a] != 0)) return TP_ERR_ARG;
        ax[a].mode = mode[a], ax[a].ne = ne[a];
        ax[a].nr = mode[a] == 0 ? ne[a] : mode[a] == 1 ? (ne[a] + 1) / 2 : mode[a] == 2 ? ne[a] / cells[a] : 1;
    }
    if (mode[2] != 0 && g->nranks > 1) return TP_ERR_ARG;   // an orbit along z would cross the slabs
    std::unique_ptr<tp_link> l(new tp_link());
    l->grid = g;
    l->d.x = ax[0], l->d.y = ax[1], l->d.z = ax[2];
    for (int a = 0; a < 3; a++) l->cells[a] = mode[a] == 2 ? cells[a] : 0;
    l->n = (long)ne[0] * ne[1] * ne[2];
    l->nred = (long)ax[0].nr * ax[1].nr * ax[2].nr;
    l->form = l->last_form = 0;
    *out = l.release();
    return TP_OK;
}
extern "C" int tp_link_counts(const tp_link *l, long *n_reduced_own, long nr[3]) {
    if (!l) return TP_ERR_ARG;
    if (n_reduced_own) *n_reduced_own = l->nred;
    if (nr) nr[0] = l->d.x.nr, nr[1] = l->d.y.nr, nr[2] = l->d.z.nr;
    return TP_OK;
}
extern "C" int tp_link_set_form(tp_link *l, int form) {
    if (!l || form < 0 || form > 2) return TP_ERR_ARG;
    l->form = form;
    return TP_OK;
}
extern "C" int tp_link_last_form(const tp_link *l) { return l ? l->last_form : 0; }

static int link_check_vecs(const tp_link *l, int nvec, const double *const *a, const double *const *b) {
    if (!l || !a || !b || nvec < 1 || nvec > TP_LINK_MAXVEC) return TP_ERR_ARG;
    for (int v = 0; v < nvec; v++)
        if (!a[v] || !b[v]) return TP_ERR_ARG;
    for (int v = 0; v < nvec; v++)
        for (int w = 0; w < nvec; w++)
            if (a[v] == b[w]) return TP_ERR_ARG;
    return TP_OK;
}

extern "C" int tp_link_expand(tp_link *l, int nvec, const double *const *red, double *const *full) {
    TP_TRY(link_check_vecs(l, nvec, red, full));
    if (!l->n) return TP_OK;
    tp_grid *g = l->grid;
    LinkPairs a{};
    for (int v = 0; v < nvec; v++) a.src[v] = red[v], a.dst[v] = full[v];
#define TP_LINK_GO(NV) TP_LAUNCH(k_link_expand<NV>, dim3(grid_for(l->n)), dim3(BLK), 0, g->stream, a, l->d, l->n)
    TP_LINK_DISPATCH(nvec, TP_LINK_GO)
#undef TP_LINK_GO
    count_launch(g, 8.0 * nvec * (l->n + l->nred), 0.0);
    return TP_OK;
}
extern "C" int tp_link_pick(tp_link *l, int nvec, const double *const *full, double *const *red) {
    TP_TRY(link_check_vecs(l, nvec, full, red));
    if (!l->n) return TP_OK;
    tp_grid *g = l->grid;
    LinkPairs a{};
    for (int v = 0; v < nvec; v++) a.src[v] = full[v], a.dst[v] = red[v];
#define TP_LINK_GO(NV) TP_LAUNCH(k_link_pick<NV>, dim3(grid_for(l->nred)), dim3(BLK), 0, g->stream, a, l->d, l->nred)
    TP_LINK_DISPATCH(nvec, TP_LINK_GO)
#undef TP_LINK_GO
    count_launch(g, 16.0 * nvec * l->nred, 0.0);
    return TP_OK;
}
// form 2 applies to an x mode other than none whose row fits the staging buffer
static bool link_form2_applies(const tp_link *l) { return l->d.x.mode != 0 && l->d.x.ne <= LINK_ROW_CAP; }
// form 0, the measured rule (profiles/link_timing.txt): form 2 won for x:extrude alone (1.9 to 2.2 times form 1
// on 128^3) and lost for x:mirror, x:repeat:4 and the three-axis combination, where form 1's lanes already read consecutive
// doubles; x:extrude with y or z linked as well was not measured and stays with form 1
static int link_default_form(const tp_link *l) { return l->d.x.mode == 3 && l->d.y.mode == 0 && l->d.z.mode == 0 ? 2 : 1; }
extern "C" int tp_link_fold(tp_link *l, int nvec, const double *const *full, double *const *red) {
    TP_TRY(link_check_vecs(l, nvec, full, red));
    if (!l->n) return TP_OK;
    tp_grid *g = l->grid;
    LinkPairs a{};
    for (int v = 0; v < nvec; v++) a.src[v] = full[v], a.dst[v] = red[v];
    const int want = l->form ? l->form : link_default_form(l);
    const int form = want == 2 && link_form2_applies(l) ? 2 : 1;
    if (form == 2) {
        const int pitch = l->d.x.ne | 1;
        const int R = std::max(1, std::min(BLK / l->d.x.nr, LINK_TILE / nvec / pitch));
        const long nrows = (long)l->d.y.nr * l->d.z.nr;
        const long groups = (nrows + R - 1) / R;
        const int nb = (int)std::min<long>(groups, 4096);
#define TP_LINK_GO(NV) TP_LAUNCH(k_link_fold_x<NV>, dim3(nb), dim3(BLK), 0, g->stream, a, l->d, R, nrows)
        TP_LINK_DISPATCH(nvec, TP_LINK_GO)
#undef TP_LINK_GO
    } else {
#define TP_LINK_GO(NV) TP_LAUNCH(k_link_fold<NV>, dim3(grid_for(l->nred)), dim3(BLK), 0, g->stream, a, l->d, l->nred)
        TP_LINK_DISPATCH(nvec, TP_LINK_GO)
#undef TP_LINK_GO
    }
    l->last_form = form;
    count_launch(g, 8.0 * nvec * (l->n + l->nred), 1.0 * nvec * (l->n - l->nred));
    return TP_OK;
}
#undef TP_LINK_DISPATCH
