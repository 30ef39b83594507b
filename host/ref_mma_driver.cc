// ref_mma_driver.cc -- acceptance program for the MMA row: the REFERENCE's own MMA class (MMA.cc, compiled unchanged
// from /root/reference in the build container; nothing of it is stored here) on the compat layer, driven with a
// synthetic smooth problem of m constraints for a few iterations; the design vector of every iteration goes to a PETSc
// binary file.  tests/test_mma.py feeds the same functions to the device MMA (tp_mma_*).  This file is ours.
//   ref_mma ex ey ez m iters out.bin [key=value ...]
// Optional settings (tests/test_mma_surface.py), none = the default run:
//   a=, c=, d=        one value for every j, through the a/c/d constructor (MMA.cc:195-242)
//   asym=i,dec,inc    SetAsymptotes          robust=0|1   SetRobustAsymptotesType     conmod=0|1   ConstraintModification
//   kkt=1             KKTresidual after every Update: "REF_MMA_KKT it <k> <norm2> <normInf>"
//   box=1             after SetOuterMovelimit, every 5th variable (global index 1 mod 5) gets a box above x and every
//                     5th (3 mod 5) one below it, so that GenSub's robust re-centring (:581-588) has both cases to do
#include <MMA.h>
#include <petsc.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

// box=1: the same pattern in tests/test_mma_surface.py (_box)
static void narrow_box(PetscInt nloc, long g0, const PetscScalar *xp, PetscScalar *lo, PetscScalar *hi) {
    for (PetscInt i = 0; i < nloc; i++) {
        const long gi = g0 + i;
        if (gi % 5 == 1 && xp[i] + 0.1 <= 1.0) {  // x below the box
            lo[i] = xp[i] + 0.01;
            hi[i] = xp[i] + 0.1;
        } else if (gi % 5 == 3 && xp[i] - 0.1 >= 0.0) {  // x above the box
            lo[i] = xp[i] - 0.1;
            hi[i] = xp[i] - 0.01;
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 7) return 2;
    const PetscInt ex = atoi(argv[1]), ey = atoi(argv[2]), ez = atoi(argv[3]), m = atoi(argv[4]), iters = atoi(argv[5]);
    bool acd = false, asym = false, kkt = false, box = false;
    double av = 0.0, cv = 1000.0, dv = 0.0, ai = 0.5, ad = 0.7, ainc = 1.2;
    int robust = -1, conmod = -1;
    for (int t = 7; t < argc; t++) {
        const char *s = argv[t];
        if (!strncmp(s, "a=", 2)) acd = true, av = atof(s + 2);
        else if (!strncmp(s, "c=", 2)) acd = true, cv = atof(s + 2);
        else if (!strncmp(s, "d=", 2)) acd = true, dv = atof(s + 2);
        else if (!strncmp(s, "asym=", 5)) {
            if (sscanf(s + 5, "%lf,%lf,%lf", &ai, &ad, &ainc) != 3) return 2;
            asym = true;
        } else if (!strncmp(s, "robust=", 7)) robust = atoi(s + 7);
        else if (!strncmp(s, "conmod=", 7)) conmod = atoi(s + 7);
        else if (!strncmp(s, "kkt=", 4)) kkt = atoi(s + 4) != 0;
        else if (!strncmp(s, "box=", 4)) box = atoi(s + 4) != 0;
        else return 2;
    }
    PetscInitialize(&argc, &argv, NULL, NULL);
    PetscErrorCode ierr;
    DM nodes, elems;  // the node mesh defines the job's mesh; the design lives on its element mesh
    ierr = DMDACreate3d(PETSC_COMM_WORLD, DM_BOUNDARY_NONE, DM_BOUNDARY_NONE, DM_BOUNDARY_NONE, DMDA_STENCIL_BOX, ex + 1, ey + 1,
                        ez + 1, PETSC_DECIDE, PETSC_DECIDE, PETSC_DECIDE, 1, 1, 0, 0, 0, &nodes);
    CHKERRQ(ierr);
    DMDASetUniformCoordinates(nodes, 0.0, (double)ex / ey, 0.0, 1.0, 0.0, (double)ez / ey);
    PetscInt md, nd, pd;
    DMDAGetInfo(nodes, NULL, NULL, NULL, NULL, &md, &nd, &pd, NULL, NULL, NULL, NULL, NULL, NULL);
    ierr = DMDACreate3d(PETSC_COMM_WORLD, DM_BOUNDARY_NONE, DM_BOUNDARY_NONE, DM_BOUNDARY_NONE, DMDA_STENCIL_BOX, ex, ey, ez, md, nd,
                        pd, 1, 0, 0, 0, 0, &elems);
    CHKERRQ(ierr);
    Vec x, dfdx, xmin, xmax, xold;
    ierr = DMCreateGlobalVector(elems, &x);
    CHKERRQ(ierr);
    VecDuplicate(x, &dfdx);
    VecDuplicate(x, &xmin);
    VecDuplicate(x, &xmax);
    VecDuplicate(x, &xold);
    Vec *dgdx;
    VecDuplicateVecs(x, m, &dgdx);
    PetscInt n, nloc, zs;
    VecGetSize(x, &n);
    VecGetLocalSize(x, &nloc);
    DMDAGetCorners(elems, NULL, NULL, &zs, NULL, NULL, NULL);
    const long g0 = (long)zs * ex * ey;  // global index of this rank's first element
    VecSet(x, 0.3);
    VecSet(xold, 0.3);
    MMA *mma;
    std::vector<PetscScalar> ac((size_t)m, av), cc((size_t)m, cv), dc((size_t)m, dv);
    if (acd)
        mma = new MMA(n, m, x, ac.data(), cc.data(), dc.data());
    else
        mma = new MMA(n, m, x);
    if (asym) mma->SetAsymptotes(ai, ad, ainc);
    if (robust >= 0) mma->SetRobustAsymptotesType(robust);
    if (conmod >= 0) mma->ConstraintModification(conmod ? PETSC_TRUE : PETSC_FALSE);
    PetscViewer view;
    ierr = PetscViewerBinaryOpen(PETSC_COMM_WORLD, argv[6], FILE_MODE_WRITE, &view);
    CHKERRQ(ierr);
    std::vector<PetscScalar> gx((size_t)m);
    for (PetscInt k = 0; k < iters; k++) {
        PetscScalar *xp, *dfp;
        VecGetArray(x, &xp);
        VecGetArray(dfdx, &dfp);
        std::vector<double> gl((size_t)m, 0.0);
        for (PetscInt i = 0; i < nloc; i++) {  // f = sum_i a_i / (x_i + 0.1): df/dx_i = -a_i / (x_i + 0.1)^2
            const double a = 1.0 + 0.3 * sin(0.37 * (double)(g0 + i));
            dfp[i] = -a / ((xp[i] + 0.1) * (xp[i] + 0.1));
        }
        for (PetscInt j = 0; j < m; j++) {  // g_j = sum_i w_ji x_i / n - c_j
            PetscScalar *gp;
            VecGetArray(dgdx[j], &gp);
            for (PetscInt i = 0; i < nloc; i++) {
                const double w = 1.0 + 0.5 * cos(0.11 * (double)(g0 + i) * (double)(j + 1));
                gp[i] = w / (double)n;
                gl[(size_t)j] += w * xp[i] / (double)n;
            }
            VecRestoreArray(dgdx[j], &gp);
        }
        VecRestoreArray(x, &xp);
        VecRestoreArray(dfdx, &dfp);
        MPI_Allreduce(gl.data(), gx.data(), (int)m, MPI_DOUBLE, MPI_SUM, PETSC_COMM_WORLD);
        for (PetscInt j = 0; j < m; j++) gx[(size_t)j] -= 0.25 + 0.05 * (double)j;
        ierr = mma->SetOuterMovelimit(0.0, 1.0, 0.2, x, xmin, xmax);
        CHKERRQ(ierr);
        if (box) {
            PetscScalar *lo, *hi;
            VecGetArray(x, &xp);
            VecGetArray(xmin, &lo);
            VecGetArray(xmax, &hi);
            narrow_box(nloc, g0, xp, lo, hi);
            VecRestoreArray(x, &xp);
            VecRestoreArray(xmin, &lo);
            VecRestoreArray(xmax, &hi);
        }
        ierr = mma->Update(x, dfdx, gx.data(), dgdx, xmin, xmax);
        CHKERRQ(ierr);
        if (kkt) {
            PetscScalar n2 = 0.0, nI = 0.0;
            ierr = mma->KKTresidual(x, dfdx, gx.data(), dgdx, xmin, xmax, &n2, &nI);
            CHKERRQ(ierr);
            PetscPrintf(PETSC_COMM_WORLD, "REF_MMA_KKT it %d %.17e %.17e\n", (int)(k + 1), n2, nI);
        }
        const PetscScalar ch = mma->DesignChange(x, xold);
        PetscPrintf(PETSC_COMM_WORLD, "REF_MMA it %d ch %.12e g0 %.12e\n", (int)(k + 1), ch, gx[0]);
        VecView(x, view);
    }
    PetscViewerDestroy(&view);
    delete mma;
    VecDestroyVecs(m, &dgdx);
    for (Vec *v : {&x, &dfdx, &xmin, &xmax, &xold}) VecDestroy(v);
    DMDestroy(&elems);
    DMDestroy(&nodes);
    PetscFinalize();
    return 0;
}
