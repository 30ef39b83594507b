// stress.h -- relaxed von Mises stress at the element centroids: the field, its p-norm and maximum, and the ingredients of
// the p-norm's sensitivity (explicit part and adjoint load).  Included from topopt_amd.hip behind response.h.  DESIGN.md 4.9.
#pragma once

// s_e = u_e^T M u_e (M = B0^T C^T Vm C B0, elements.h), vm_e = Emax x_e^q sqrt(s_e), pnorm = (sum_e vm_e^P)^(1/P).
// Both kernels take u_e RELATIVE TO THE ELEMENT'S CORNER 0 (d_a = u_a - u_0): M annihilates translations, so the value is
// the same to rounding, an element in rigid translation gets s_e = 0 and M d_e = 0 EXACTLY instead of a rounding residue
// under a square root, and the three columns of corner 0 drop out (441 fma instead of 576).  Indices into M are compile-time
// constants: scalar operand loads, as for KE in k_objective.
// Pass 1, one thread per own element like k_objective: vm_e (if asked), s_e (clamped at 0) for the later passes, and with
// REDUCE the block partials of vm_e^P and of max vm_e, partials[value][block].
template <bool REDUCE>
__global__ __launch_bounds__(BLK) void k_stress_elem(Geom g, const double *__restrict__ M, const double *__restrict__ U,
                                                     const double *__restrict__ x, double Emax, double q, double P,
                                                     double *__restrict__ vm_out, double *__restrict__ s_out,
                                                     double *__restrict__ partials) {
    const long nel = g.own_elems();
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    double vm = 0.0;
    if (t < nel) {
        int i, j, k;
        elem_ijk(g, t, i, j, k);
        double d[24];
        gather24(g, i, j, k, U, d);
#pragma unroll
        for (int r = 3; r < 24; r++) d[r] -= d[r % 3];
        double s = 0.0;
#pragma unroll
        for (int r = 3; r < 24; r++) {
            double m = 0.0;
#pragma unroll
            for (int c = 3; c < 24; c++) m = fma(M[r * 24 + c], d[c], m);
            s = fma(d[r], m, s);
        }
        s = s < 0.0 ? 0.0 : s;  // (M is positive semi-definite; a strain at rounding level may come out below zero; NaN stays)
        if (s != 0.0) vm = Emax * pow(x[t], q) * sqrt(s);
        if (vm_out) vm_out[t] = vm;
        if (s_out) s_out[t] = s;
    }
    if (!REDUCE) return;
    const double sp = block_sum(vm != 0.0 ? pow(vm, P) : 0.0);
    const double mx = block_max(vm);  // (fmax drops a NaN; the sum carries it: a NaN state gives pnorm = NaN as it gives fx = NaN)
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sp;
        partials[gridDim.x + blockIdx.x] = mx;
    }
}
// Between the passes, once pnorm is known: s_e -> c_e = pnorm^(1-P) (Emax x^q)^P s_e^((P-2)/2), the weight of L_e^T M u_e in
// d pnorm / dU, formed as r_e^(P-2) (Emax x^q)^2 / pnorm with r_e = vm_e / pnorm <= 1 (no overflow, no division by s_e),
// in place; and the explicit part dpdx_e = pnorm^(1-P) q Emax^P x^(qP-1) s_e^(P/2) in the power form q pnorm x^(qP-1)
// (Emax sqrt(s_e) / pnorm)^P: x_e = 0 gives 0 (qP > 1) or a finite value (qP = 1), never NaN.  s_e = 0 or pnorm = 0: both 0.
__global__ __launch_bounds__(BLK) void k_stress_coef(long nel, const double *__restrict__ x, double Emax, double q, double P,
                                                     double pnorm, double *__restrict__ sc, double *__restrict__ dpdx) {
    for (long t = blockIdx.x * (long)BLK + threadIdx.x; t < nel; t += (long)gridDim.x * BLK) {
        const double s = sc[t], xe = x[t];
        double c = 0.0, dp = 0.0;
        if (pnorm != 0.0 && s != 0.0) {
            const double a = Emax * pow(xe, q), rs = sqrt(s);
            c = pow(a * rs / pnorm, P - 2.0) * a * (a / pnorm);
            if (q != 0.0) dp = q * pnorm * pow(xe, q * P - 1.0) * pow(Emax * rs / pnorm, P);
        }
        sc[t] = c;
        if (dpdx) dpdx[t] = dp;
    }
}
// Pass 2, one thread per OWNED node: adj_rhs = sum over the node's <= 8 incident elements, in a fixed order, of
// c_e (M d_e)[rows of the node's corner] -- a gather, no atomics, bit-reproducible.  Incident element n8 of the unrolled
// loop lies at (i - dx, j - dy, k - dz) and has the node as its corner corner_of(dx, dy, dz) for every thread: the three rows
// of M are compile-time.  Elements outside the mesh or the slab (layers 0 .. ezl - 1: own + the ghost layer above, whose
// c_e came from the upper neighbour) are skipped, and so are those with c_e = 0.  The Dirichlet mask is not applied here.
__global__ __launch_bounds__(BLK) void k_stress_adjoint_rhs(Geom g, const double *__restrict__ M, const double *__restrict__ U,
                                                            const double *__restrict__ ce, double *__restrict__ out) {
    const long t = blockIdx.x * (long)BLK + threadIdx.x;
    if (t >= g.owned_nodes()) return;
    const long n = g.plane() * g.own_lo + t;
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / g.plane());
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int n8 = 0; n8 < 8; n8++) {
        const int dx = n8 & 1, dy = (n8 >> 1) & 1, dz = n8 >> 2;
        const int a = corner_of(dx, dy, dz);
        const int ei = i - dx, ej = j - dy, ek = k - dz;
        if (ei < 0 || ei >= g.ex || ej < 0 || ej >= g.ey || ek < 0 || ek >= g.ezl) continue;
        const double c = ce[(long)ei + (long)g.ex * (ej + (long)g.ey * ek)];
        if (c == 0.0) continue;
        double d[24];
        gather24(g, ei, ej, ek, U, d);
#pragma unroll
        for (int r = 3; r < 24; r++) d[r] -= d[r % 3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double m = 0.0;
#pragma unroll
            for (int cc = 3; cc < 24; cc++) m = fma(M[(3 * a + r) * 24 + cc], d[cc], m);
            acc[r] = fma(c, m, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 3; r++) out[3 * n + r] = acc[r];
}

extern "C" int tp_elasticity_get_stress_form(const tp_elasticity *e, double *m) {
    if (!e || !m) return TP_ERR_ARG;
    std::memcpy(m, e->VM, sizeof(e->VM));
    return TP_OK;
}
extern "C" int tp_elasticity_stress(tp_elasticity *e, const double *U, const double *xPhys, double Emax, double q, double P,
                                    double *vm, double *pnorm, double *vm_max, double *dpdx, double *adj_rhs) {
    if (!e || !U || !xPhys) return TP_ERR_ARG;
    if (!(P >= 2.0) || !(q >= 0.0) || !(q == 0.0 || q * P >= 1.0)) return TP_ERR_ARG;
    tp_grid *g = e->grid;
    Geom geo = e->mg.lv[0].g;
    const long nel = geo.own_elems(), lay = (long)geo.ex * geo.ey;
    const bool sums = pnorm || vm_max || dpdx || adj_rhs;
    if (!sums && !vm) return TP_OK;
    TP_TRY(halo_nodes(g, geo, const_cast<double *>(U), 3));
    const int nb = (int)((nel + BLK - 1) / BLK);
    const double bytes = 24.0 * geo.owned_nodes() + 8.0 * nel, flops = 2.0 * 462 * nel;
    if (!sums) {  // the field alone: no reduction, nothing for the host to wait for
        TP_LAUNCH(k_stress_elem<false>, dim3(nb), dim3(BLK), 0, g->stream, geo, e->d_VM, U, xPhys, Emax, q, P, vm, (double *)nullptr,
                  (double *)nullptr);
        count_launch(g, bytes + 8.0 * nel, flops);
        return TP_OK;
    }
    double *sc = nullptr;
    if (dpdx || adj_rhs) {
        if (!e->d_sx) TP_TRY(e->d_sx.alloc_zero((size_t)(nel + lay), g->stream));
        sc = e->d_sx;
    }
    TP_LAUNCH(k_stress_elem<true>, dim3(nb), dim3(BLK), 0, g->stream, geo, e->d_VM, U, xPhys, Emax, q, P, vm, sc, g->partials);
    count_launch(g, bytes + 8.0 * nel * ((vm ? 1 : 0) + (sc ? 1 : 0)), flops);
    TP_LAUNCH(k_sum_max_final, dim3(1), dim3(BLK), 0, g->stream, g->partials, nb, g->scal + S_TMP);
    count_launch(g);
    TP_TRY(finish_reduction_n(g, S_TMP, 1));  // the sum over the ranks; the maximum follows below
    double v[2];
    TP_TRY(read_scal(g, S_TMP, 2, v));
    TP_TRY(rank_max(g, &v[1]));
    const double pn = v[0] != 0.0 ? pow(v[0], 1.0 / P) : 0.0;
    if (pnorm) *pnorm = pn;
    if (vm_max) *vm_max = v[1];
    if (!sc) return TP_OK;
    TP_LAUNCH(k_stress_coef, dim3(grid_for(nel)), dim3(BLK), 0, g->stream, nel, xPhys, Emax, q, P, pn, sc, dpdx);
    count_launch(g, (24.0 + (dpdx ? 8.0 : 0.0)) * nel, 8.0 * nel);
    if (!adj_rhs) return TP_OK;
    // the ghost element layer above <- the upper neighbour's first own layer, the way tp_elasticity_assemble fills d_E
    TP_TRY(exchange_segments(g, sc, nullptr, nullptr, sc + nel, lay, 1, lay));
    const long nown = geo.owned_nodes();
    TP_LAUNCH(k_stress_adjoint_rhs, dim3((int)((nown + BLK - 1) / BLK)), dim3(BLK), 0, g->stream, geo, e->d_VM, U, sc, adj_rhs);
    count_launch(g, 48.0 * nown + 8.0 * nel, 2.0 * 8 * (63 + 3) * nown);
    return TP_OK;
}
