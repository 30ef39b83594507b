// The bodies of k_mass_apply and k_mass_sens (csrc/mass.h) as host code, run thread by thread on exactly sized buffers under the
// address and undefined-behaviour sanitizers: 20x12x12, hx != hy != hz, a third of the elements below x_low, 1, 2 and 3 slabs.
// Checks: no access outside a slab's arrays (the sanitizers), owned results bit-equal to the one-slab run, ghost planes of y
// untouched, and the distance from a long double element-by-element sum.  No GPU is used.
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -c -o mass_bodies_check.o tools/mass_bodies_check.cpp
//   hipcc -fsanitize=address,undefined -o mass_bodies_check mass_bodies_check.o && ./mass_bodies_check
#define TP_BODIES_ONLY
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../topopt_in_petsc_amd/csrc/common.h"
#include "../topopt_in_petsc_amd/csrc/bodyforce.h"
#include "../topopt_in_petsc_amd/csrc/mass.h"

static Geom slab_geom(int ex, int ey, int ez, int rank, int nranks) {  // grid.h: make_geom, level 0
    Geom q;
    q.ex = ex, q.ey = ey, q.nx = ex + 1, q.ny = ey + 1;
    q.ez_own = ez / nranks;
    q.has_lo = rank > 0, q.has_hi = rank < nranks - 1;
    q.ezl = q.ez_own + q.has_hi;
    q.nzl = q.ez_own + 1 + q.has_hi;
    q.own_lo = q.has_lo ? 1 : 0, q.own_hi = q.ez_own;
    q.gz0 = rank * q.ez_own;
    q.nz_glob = ez + 1;
    return q;
}
static double rnd(unsigned long long &s) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
}

int main() {
    const int ex = 20, ey = 12, ez = 12, nf = 3;
    const double h[3] = {0.05, 0.04, 0.03}, rho0 = 2.5, x_low = 0.1, w[3] = {0.75, -0.5, 0.0}, scale = -2.0;
    const long nel = (long)ex * ey * ez, plane = (long)(ex + 1) * (ey + 1), nn = plane * (ez + 1);
    unsigned long long seed = 12345;
    std::vector<double> x(nel), N(3 * nn, 1.0), pre(nel);
    std::vector<std::vector<double>> V(nf, std::vector<double>(3 * nn));
    for (long e = 0; e < nel; e++) x[e] = e % 3 == 0 ? 0.01 + 0.085 * rnd(seed) : 0.05 + 0.95 * rnd(seed);
    for (long n = 0; n < nn; n++)
        if (n % (ex + 1) == 0) N[3 * n] = N[3 * n + 1] = N[3 * n + 2] = 0.0;  // the cantilever's clamp
    for (auto &v : V)
        for (auto &a : v) a = 2.0 * rnd(seed) - 1.0;  // not zero on the clamp
    for (auto &a : pre) a = 1e-4 * (2.0 * rnd(seed) - 1.0);
    const MassPar p{rho0 * h[0] * h[1] * h[2], x_low, 1.0 / x_low};
    std::vector<double> y_one, d_one;
    int bad = 0;
    for (int R = 1; R <= 3; R++) {
        for (int rank = 0; rank < R; rank++) {
            const Geom q = slab_geom(ex, ey, ez, rank, R);
            const long z0 = q.gz0, lay = (long)ex * ey;
            // exactly sized local arrays: stored element layers, stored node planes
            std::vector<double> mc((size_t)q.elems_stored()), xs((size_t)q.own_elems()), Nl((size_t)(3 * q.nodes())), y((size_t)(3 * q.nodes()), 5.0),
                d((size_t)q.own_elems());
            for (long t = 0; t < q.elems_stored(); t++) mc[t] = p.rv * body_mass(x[lay * z0 + t], p.x_low, p.inv_low);
            for (long t = 0; t < q.own_elems(); t++) xs[t] = x[lay * z0 + t], d[t] = pre[lay * z0 + t];
            for (long t = 0; t < 3 * q.nodes(); t++) Nl[t] = N[3 * plane * z0 + t];
            std::vector<std::vector<double>> Vl(nf, std::vector<double>((size_t)(3 * q.nodes())));
            for (int l = 0; l < nf; l++)
                for (long t = 0; t < 3 * q.nodes(); t++) Vl[l][t] = V[l][3 * plane * z0 + t];
            for (long t = 0; t < q.owned_nodes(); t++) mass_apply_node(q, t, mc.data(), Nl.data(), Vl[0].data(), y.data());
            MassFields a{};
            a.ncase = nf;
            for (int l = 0; l < nf; l++) a.V[l] = Vl[l].data(), a.w[l] = w[l];
            for (long t = 0; t < q.own_elems(); t++) mass_sens_elem(q, p, a, t, Nl.data(), xs.data(), scale, d.data());
            if (R == 1) {
                y_one = y, d_one = d;
                continue;
            }
            for (long t = 0; t < 3 * q.nodes(); t++) {
                const long k = t / (3 * plane);
                const bool owned = k >= q.own_lo && k <= q.own_hi;
                if (owned ? y[t] != y_one[3 * plane * z0 + t] : y[t] != 5.0) bad++;
            }
            for (long t = 0; t < q.own_elems(); t++)
                if (d[t] != d_one[lay * z0 + t]) bad++;
        }
        printf("%d slab(s): %s\n", R, R == 1 ? "reference run" : (bad ? "MISMATCH" : "owned results bit-equal to one slab, ghost planes untouched"));
    }
    // accuracy of the one-slab run against a long double element-by-element sum
    std::vector<long double> yr(3 * nn, 0.0L), dr(nel);
    long double ytop = 0, yerr = 0, dtop = 0, derr = 0;
    for (long e = 0; e < nel; e++) {
        const int i = (int)(e % ex), j = (int)((e / ex) % ey), k = (int)(e / ((long)ex * ey));
        const long double c = (long double)rho0 * h[0] * h[1] * h[2] * (long double)body_mass(x[e], x_low, 1.0 / x_low);
        long nd[8];
        for (int b = 0; b < 8; b++) nd[b] = (i + LXc(b)) + (long)(ex + 1) * ((j + LYc(b)) + (long)(ey + 1) * (k + LZc(b)));
        long double acc = 0;
        for (int l = 0; l < nf; l++) {
            long double s = 0;
            for (int b = 0; b < 8; b++)
                for (int b2 = 0; b2 < 8; b2++) {
                    const int dd = (LXc(b) != LXc(b2)) + (LYc(b) != LYc(b2)) + (LZc(b) != LZc(b2));
                    const long double f = 1.0L / (dd == 0 ? 27 : dd == 1 ? 54 : dd == 2 ? 108 : 216);
                    for (int c3 = 0; c3 < 3; c3++) {
                        const long double vb = (long double)N[3 * nd[b] + c3] * V[l][3 * nd[b] + c3], vb2 = (long double)N[3 * nd[b2] + c3] * V[l][3 * nd[b2] + c3];
                        s += f * vb * vb2;
                        if (l == 0) yr[3 * nd[b] + c3] += c * f * vb2 * N[3 * nd[b] + c3];
                    }
                }
            acc += (long double)w[l] * s;
        }
        dr[e] = (long double)pre[e] + (long double)scale * (long double)rho0 * h[0] * h[1] * h[2] * (long double)body_dmass(x[e], x_low, 1.0 / x_low) * acc;
    }
    for (long t = 0; t < 3 * nn; t++) ytop = fmaxl(ytop, fabsl(yr[t])), yerr = fmaxl(yerr, fabsl(yr[t] - y_one[t]));
    for (long e = 0; e < nel; e++) dtop = fmaxl(dtop, fabsl(dr[e] - pre[e])), derr = fmaxl(derr, fabsl(dr[e] - d_one[e]));
    printf("mass_apply %.3Le of max|B u|, mass_sens %.3Le of max|term| (floor of the bound 64 * 2^-53 = 7.1e-15)\n", yerr / ytop, derr / dtop);
    if (bad || yerr / ytop > 7.1e-15L || derr / dtop > 7.1e-15L) return 1;
    printf("OK\n");
    return 0;
}
