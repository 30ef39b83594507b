// mma_probe.cc -- the device MMA through the C++ mirror (topopt_host.h) on the synthetic problem of ref_mma_driver.cc,
// on one or more z-slab ranks (`slabrun -n N [--same-device] mma_probe ...`): prints KKTresidual's norms, first before
// any Update (lam = y = z = 0: the inputs are the same on every rank count, bit for bit), then after every Update.
//   mma_probe ex ey ez m iters [a=. c=. d=. asym=i,dec,inc robust=0|1 conmod=0|1 box=1 dump=PATH]
// Output (rank 0): "MMA_PROBE kkt <k> <norm2 %.17e> <normInf %.17e>", k = 0 before the first Update.
// dump=PATH: after every Update each rank appends its slab of x, raw float64, to PATH.<rank> (the slabs in rank order are
// the global vector), and rank 0 prints "MMA_PROBE lam <k> <lam_0 %.17e> ... <lam_m-1>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "slab_comm.h"
#include "topopt_host.h"

// ref_mma_driver.cc's box=1 pattern
static void narrow_box(long nloc, long g0, const double *xp, double *lo, double *hi) {
    for (long i = 0; i < nloc; i++) {
        const long gi = g0 + i;
        if (gi % 5 == 1 && xp[i] + 0.1 <= 1.0) {
            lo[i] = xp[i] + 0.01;
            hi[i] = xp[i] + 0.1;
        } else if (gi % 5 == 3 && xp[i] - 0.1 >= 0.0) {
            lo[i] = xp[i] - 0.1;
            hi[i] = xp[i] - 0.01;
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int ex = atoi(argv[1]), ey = atoi(argv[2]), ez = atoi(argv[3]), m = atoi(argv[4]), iters = atoi(argv[5]);
    if (m < 1 || m > 8) return 2;
    bool acd = false, asym = false, box = false;
    double av = 0.0, cv = 1000.0, dv = 0.0, ai = 0.5, ad = 0.7, ainc = 1.2;
    int robust = 0, conmod = 0;
    std::string dump;
    for (int t = 6; t < argc; t++) {
        const char *s = argv[t];
        if (!strncmp(s, "a=", 2)) acd = true, av = atof(s + 2);
        else if (!strncmp(s, "c=", 2)) acd = true, cv = atof(s + 2);
        else if (!strncmp(s, "d=", 2)) acd = true, dv = atof(s + 2);
        else if (!strncmp(s, "asym=", 5)) {
            if (sscanf(s + 5, "%lf,%lf,%lf", &ai, &ad, &ainc) != 3) return 2;
            asym = true;
        } else if (!strncmp(s, "robust=", 7)) robust = atoi(s + 7);
        else if (!strncmp(s, "conmod=", 7)) conmod = atoi(s + 7);
        else if (!strncmp(s, "box=", 4)) box = atoi(s + 4) != 0;
        else if (!strncmp(s, "dump=", 5)) dump = s + 5;
        else return 2;
    }
    const int nx = ex + 1, ny = ey + 1, nz = ez + 1;
    const double h = 1.0 / ey;
    SlabComm sc;
    if (slab_comm_init(&sc, std::max(4L * 3 * nx * ny, 1L << 16))) return 1;
    const bool root = sc.rank == 0;
    tp_grid_opts go = {nx, ny, nz, h, h, h, sc.rank, sc.nranks, sc.device, nullptr, sc.nranks > 1 ? &sc.hooks : nullptr};
    tp_grid *grid = nullptr;
    PetscErrorCode ierr = tp_grid_create(&grid, &go);
    CHKERRQ(ierr);
    sc.grid = grid;
    const long nloc = tp_grid_local_elems(grid), n = (long)ex * ey * ez;
    std::vector<double> counts((size_t)sc.nranks, 0.0);
    counts[(size_t)sc.rank] = (double)nloc;
    slab_detail::host_reduce(&sc, counts.data(), sc.nranks, 0);
    long g0 = 0;  // global index of this rank's first element (z-slabs in rank order)
    for (int r = 0; r < sc.rank; r++) g0 += (long)counts[(size_t)r];

    Vec x, dfdx, xmin, xmax;
    std::vector<Vec> dgdx((size_t)m);
    for (Vec *v : {&x, &dfdx, &xmin, &xmax}) VecCreate(grid, nloc, v);
    for (Vec &v : dgdx) VecCreate(grid, nloc, &v);
    VecSet(x, 0.3);
    std::vector<double> ac((size_t)m, av), cc((size_t)m, cv), dc((size_t)m, dv);
    MMA *mma = acd ? new MMA(grid, (PetscInt)n, m, x, ac.data(), cc.data(), dc.data()) : new MMA(grid, (PetscInt)n, m, x);
    CHKERRQ(mma->err);
    if (asym) mma->SetAsymptotes(ai, ad, ainc);
    mma->SetRobustAsymptotesType(robust);
    mma->ConstraintModification(conmod ? PETSC_TRUE : PETSC_FALSE);
    std::vector<double> gx((size_t)m);
    FILE *df = nullptr;
    if (!dump.empty()) {
        df = fopen((dump + "." + std::to_string(sc.rank)).c_str(), "wb");
        if (!df) return 3;
    }
    for (int k = 0; k <= iters; k++) {
        double *xp, *dfp;
        VecGetArray(x, &xp);
        VecGetArray(dfdx, &dfp);
        std::vector<double> gl((size_t)m, 0.0);
        for (long i = 0; i < nloc; i++) {
            const double a = 1.0 + 0.3 * sin(0.37 * (double)(g0 + i));
            dfp[i] = -a / ((xp[i] + 0.1) * (xp[i] + 0.1));
        }
        for (int j = 0; j < m; j++) {
            double *gp;
            VecGetArray(dgdx[(size_t)j], &gp);
            for (long i = 0; i < nloc; i++) {
                const double w = 1.0 + 0.5 * cos(0.11 * (double)(g0 + i) * (double)(j + 1));
                gp[i] = w / (double)n;
                gl[(size_t)j] += w * xp[i] / (double)n;
            }
            VecRestoreArray(dgdx[(size_t)j], &gp);
        }
        VecRestoreArray(x, &xp);
        VecRestoreArray(dfdx, &dfp);
        slab_detail::host_reduce(&sc, gl.data(), m, 0);
        for (int j = 0; j < m; j++) gx[(size_t)j] = gl[(size_t)j] - (0.25 + 0.05 * (double)j);
        ierr = mma->SetOuterMovelimit(0.0, 1.0, 0.2, x, xmin, xmax);
        CHKERRQ(ierr);
        if (box) {
            double *lo, *hi;
            VecGetArray(x, &xp);
            VecGetArray(xmin, &lo);
            VecGetArray(xmax, &hi);
            narrow_box(nloc, g0, xp, lo, hi);
            VecRestoreArray(xmin, &lo);
            VecRestoreArray(xmax, &hi);
        }
        if (k > 0) {
            ierr = mma->Update(x, dfdx, gx.data(), dgdx.data(), xmin, xmax);
            CHKERRQ(ierr);
            if (df) {
                VecGetArray(x, &xp);
                const size_t wrote = fwrite(xp, sizeof(double), (size_t)nloc, df);
                VecRestoreArray(x, &xp);
                if (wrote != (size_t)nloc) return 3;
                std::vector<double> lam((size_t)m);
                ierr = mma->GetState(lam.data(), nullptr, nullptr);
                CHKERRQ(ierr);
                if (root) {
                    printf("MMA_PROBE lam %d", k);
                    for (double l : lam) printf(" %.17e", l);
                    printf("\n");
                }
            }
        }
        double n2 = 0.0, nI = 0.0;
        ierr = mma->KKTresidual(x, dfdx, gx.data(), dgdx.data(), xmin, xmax, &n2, &nI);
        CHKERRQ(ierr);
        if (root) printf("MMA_PROBE kkt %d %.17e %.17e\n", k, n2, nI);
    }
    if (df && fclose(df)) return 3;
    delete mma;
    for (Vec *v : {&x, &dfdx, &xmin, &xmax}) VecDestroy(v);
    for (Vec &v : dgdx) VecDestroy(&v);
    tp_grid_destroy(grid);
    slab_comm_free(&sc);
    return 0;
}
