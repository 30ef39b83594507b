/*
 * topopt_amd.h -- C ABI of the MI355X-native hot path of TopOpt_in_PETSc.
 *
 * One shared library (libtopopt_amd.so, HIP, gfx950) replaces what the
 * reference does per design iteration through PETSc:
 *
 *   stiffness "assembly"  -> tp_elasticity_assemble   (LinearElasticity.cc:487-549, :198-200)
 *   KSPSolve (CG + PCMG)  -> tp_elasticity_solve      (LinearElasticity.cc:204, :617-746)
 *   MatMult(K, u)         -> tp_elasticity_apply      (PETSc MatMult on the assembled K)
 *   objective/sensitivity -> tp_elasticity_objective  (LinearElasticity.cc:363-445)
 *   density filter        -> tp_filter_*              (Filter.cc:60-204, :290-463)
 *   Helmholtz PDE filter  -> tp_pdefilter_*           (PDEFilter.cc:189-218, :243-417)
 *
 * Conventions (mirroring PetscErrorCode): every function returns int, 0 = OK,
 * nonzero = error (TP_ERR_*; hipError_t values are passed through offset by
 * TP_ERR_HIP).  No exceptions cross the boundary.  Scalars are double
 * (PetscScalar), indices int (PetscInt, 32 bit) except sizes in bytes/long.
 *
 * Memory: every `double*` argument marked [dev] is a DEVICE pointer to plain
 * contiguous doubles (no torch types).  Host code that only has host arrays
 * (VecGetArray in the reference) uses tp_malloc / tp_memcpy_* below.
 *
 * Layout (identical to the reference's DMDA natural ordering,
 * LinearElasticity.cc:819-826): node id = i + nx*(j + ny*k), dof = 3*node+c
 * (u,v,w interlaced), element id = i + ex*(j + ey*k), x fastest.
 *
 * Partitioning: z-slabs.  Rank r of R owns element layers [r*ez/R, (r+1)*ez/R)
 * and, like DMDA (a rank owns the elements whose upper corner node it owns,
 * LinearElasticity.cc:802-814), the node planes (r*ez/R, (r+1)*ez/R]; rank 0
 * also owns plane 0.  A rank's *local* node array stores planes
 * r*ez/R .. (r+1)*ez/R+1 (one ghost plane either side where a neighbour
 * exists); local element arrays store the own layers only.  With R = 1 local
 * == global.  tp_grid_local_* report the local sizes.
 *
 * Threading: one host thread per context; all work is enqueued on the
 * hipStream_t given at creation (pass the framework's current stream).
 */
#ifndef TOPOPT_AMD_H
#define TOPOPT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TP_OK 0
#define TP_ERR_ARG 1        /* bad argument / mesh not coarsenable (TopOpt.cc:183-201) */
#define TP_ERR_STATE 2      /* call order violated (e.g. solve before assemble) */
#define TP_ERR_DIVERGED 3   /* KSP_DIVERGED_DTOL analogue */
#define TP_ERR_COMM 4       /* communication callback failed */
#define TP_ERR_HIP 1000     /* TP_ERR_HIP + hipError_t */

#define TP_MAX_LEVELS 10

/* ---- communication hooks (z-slab halo + reductions) -------------------- */
/* tp_comm is the set of slab-exchange operations the library calls: a staged neighbour exchange, an all-reduce
 * of up to 16 doubles and an all-gather on staging buffers the host framework owns, plus two optional in-place
 * forms (zero-copy halo of contiguous planes, in-place all-reduce).  All of them are ordered on the stream the grid
 * was created with.  Two implementations exist: the host framework's hooks (torch.distributed with the nccl(=RCCL)
 * backend, gloo in the CPU / one-GPU tests, MPI in a C++ host) and the library's own RCCL path, which replaces the
 * hooks after tp_grid_use_rccl (RCCL is dlopen'ed from the path the host passes, never linked).               */
typedef struct tp_comm {
    void *user;
    double *send_lo, *send_hi, *recv_lo, *recv_hi; /* [dev] staging, cap doubles each */
    double *red;                                   /* [dev] >= 16 doubles, all-reduce scratch */
    long cap;
    /* send send_lo[0..n) to rank-1 and send_hi[0..n) to rank+1, receive recv_lo from
     * rank-1 and recv_hi from rank+1 (absent neighbours are skipped). */
    int (*exchange)(void *user, long n);
    /* in-place sum over ranks of red[0..n) */
    int (*allreduce_sum)(void *user, int n);
    /* gather[r*n .. (r+1)*n) <- rank r's send_lo[0..n), for every rank (n <= cap) */
    double *gather;                                /* [dev] nranks * cap doubles */
    int (*allgather)(void *user, long n);
    /* optional zero-copy halo of contiguous planes (may be NULL -> staged `exchange` is used):
     * to_lo[0..n) -> rank-1, to_hi[0..n) -> rank+1, from_lo <- rank-1, from_hi <- rank+1, all [dev].
     * Returns 0, or 2 = "cannot address these pointers, nothing was sent": the library then uses `exchange`
     * from now on (same message sizes and order, so ranks may differ in their choice); else error. */
    int (*exchange_direct)(void *user, const double *to_lo, double *from_lo, const double *to_hi, double *from_hi,
                           long n);
    /* optional: in-place sum over ranks of p[0..n), p any [dev] address (NULL -> staged through `red`) */
    int (*allreduce_inplace)(void *user, double *p, int n);
    /* optional: issue the FOLLOWING operations on `stream` (a hipStream_t) instead of the grid's stream, until the
     * next call (NULL restores the grid's stream).  With it and exchange_direct the library overlaps the halo of a
     * smoothing step with the step's interior planes on a second stream (DMGlobalToLocalBegin ... End,
     * LinearElasticity.cc:249-250); NULL -> every halo is exchanged on the grid's stream before its consumer. */
    void (*set_stream)(void *user, void *stream);
} tp_comm;

/* ---- grid / partition --------------------------------------------------- */
typedef struct tp_grid_opts {
    int nx, ny, nz;       /* GLOBAL node counts, TopOpt.cc:106-108 (-nx -ny -nz) */
    double hx, hy, hz;    /* element edge lengths */
    int rank, nranks;     /* z-slab partition */
    int device;           /* HIP device ordinal */
    void *stream;         /* hipStream_t; NULL = the null stream */
    const tp_comm *comm;  /* NULL when nranks == 1 */
} tp_grid_opts;

typedef struct tp_grid tp_grid;
int tp_grid_create(tp_grid **g, const tp_grid_opts *o);
int tp_grid_destroy(tp_grid *g);
long tp_grid_local_nodes(const tp_grid *g);     /* nodes in the local array incl. ghost planes */
long tp_grid_local_elems(const tp_grid *g);     /* own elements */
long tp_grid_owned_node_offset(const tp_grid *g); /* first owned node in the local array */
long tp_grid_owned_nodes(const tp_grid *g);
int tp_grid_node_z0(const tp_grid *g);          /* global z index of local node plane 0 */
/* refresh the ghost node planes of a slab-local nodal array with `dof` values per node (DMGlobalToLocalBegin/End,
 * LinearElasticity.cc:249-250); a no-op on one rank */
int tp_grid_halo_nodes(tp_grid *g, double *v, int dof);
int tp_grid_elem_z0(const tp_grid *g);          /* global z index of local element layer 0 */

/* ---- optional: the slab exchange issued directly to RCCL -------------------------------------
 * The reference exchanges ghost layers with MPI inside PETSc (DMGlobalToLocal, VecDot; e.g.
 * LinearElasticity.cc:249-250).  By default the library calls the tp_comm hooks of the host framework; on one
 * node it can instead issue grouped ncclSend/ncclRecv, ncclAllReduce and ncclAllGather itself on the solver's
 * stream (xGMI, no host round trip per halo).  RCCL is not linked: pass the path of the librccl.so the process
 * already uses.  tp_grid_use_rccl is collective over the ranks of the grid (rank 0 creates the id, the host
 * broadcasts the 128 bytes); on failure the tp_comm hooks given at creation stay in place. */
int tp_rccl_load(const char *librccl_path);
int tp_rccl_unique_id(void *id128);
int tp_grid_use_rccl(tp_grid *g, const void *id128);
/* the same with a second unique id: the neighbour exchanges (halo stream) get a communicator of their own, so that RCCL
 * does not order them behind the all-reduces of the solver's stream (one communicator = one queue) */
int tp_grid_use_rccl2(tp_grid *g, const void *id128, const void *id128_halo);
int tp_grid_comm_stats(const tp_grid *g, long *exchanges, long *reductions);   /* RCCL path only, else zeros */
/* ranks the RCCL communicator itself reports (ncclCommCount; 0: no RCCL path, -1: unknown), second communicator in use */
int tp_grid_comm_info(const tp_grid *g, int *rccl_ranks, int *two_communicators);
/* The roofline kernel timed where it runs (bench.py): with on = 1 every launch of the fine level's fused operator +
 * Chebyshev step is bracketed by a pair of HIP events on the grid's stream; the read waits for the stream, returns
 * the summed elapsed time and the number of launches, and clears the list. */
/* Timing of the slab communication where it runs (N > 1): per kind -- 0 blocking halo exchange, 1 halo exchange overlapped on
 * the second stream, 2 all-reduce, 3 all-gather of the replicated coarse levels -- hook calls, host wall time inside the hooks and
 * device time between HIP event pairs around them.  What the reference spends in DMGlobalToLocalBegin/End
 * (/root/reference/LinearElasticity.cc:249-250) and MPI_Allreduce (:283, :429). */
int tp_grid_comm_timer(tp_grid *g, int on);
int tp_grid_comm_timer_read(tp_grid *g, long calls[4], double host_ms[4], double device_ms[4]);
int tp_grid_kernel_timer(tp_grid *g, int on);
int tp_grid_kernel_timer_read(tp_grid *g, double *total_ms, long *launches);
/* the same plus the algorithmic bytes of exactly the timed launches */
int tp_grid_kernel_timer_read2(tp_grid *g, double *total_ms, long *launches, double *alg_bytes);
/* halos that travelled on the second stream, overlapped with the interior planes of their producer (0 if the hooks
 * lack set_stream / exchange_direct, or with TP_OVERLAP=0) */
long tp_grid_overlapped_halos(const tp_grid *g);
/* back to the tp_comm hooks given at creation (destroys the library's communicator) */
int tp_grid_drop_rccl(tp_grid *g);
/* collective: rank-tagged buffers through the grid's CURRENT hooks (staged and in-place exchange, reductions,
 * all-gather); *ok = 1 if this rank received exactly its neighbours' data */
int tp_grid_comm_selfcheck(tp_grid *g, int *ok);
/* Stress test of the reductions that are finished inside the producing kernel (csrc/common.h, reduce_tail): `reps` dot
 * products of two generated vectors of n doubles, back to back, each also computed by the two-launch form (partial sums,
 * then k_reduce_final); *mismatches = how many differ in any bit.  (TP_NO_REDUCE_TAIL=1 switches the in-kernel form off
 * library-wide; the test then compares the two-launch form with itself.) */
int tp_grid_reduction_selftest(tp_grid *g, long n, int reps, int *mismatches);
/* one-rank loop-back check of the RCCL call sequence (the rank is its own lower and upper neighbour):
 * returns TP_OK and the largest deviation in *max_err */
int tp_rccl_selftest(int device, void *stream, long n, double *max_err);

/* ---- device memory helpers (for hosts without a GPU framework) ---------- */
int tp_set_device(int device);             /* hipSetDevice: before tp_malloc of the tp_comm staging buffers */
int tp_malloc(void **p, size_t bytes);
int tp_free(void *p);
/* bytes of device memory the library's own objects (grids, solvers, filters, ... and their work space) hold in this process
 * right now.  Memory from tp_malloc is the caller's and is not counted.  Destroying every object brings it back to 0: a
 * test of ownership reads it before a create and after the destroy. */
long long tp_device_bytes_live(void);
int tp_memcpy_h2d(void *dst, const void *src, size_t bytes);
int tp_memcpy_d2h(void *dst, const void *src, size_t bytes);
int tp_sync(const tp_grid *g);

/* ---- linear elasticity -------------------------------------------------- */
typedef struct tp_solver_opts {
    int nlvls;          /* MG levels, LinearElasticity.cc:23 (-nlvls, default 4) */
    double nu;          /* Poisson ratio, :22 (-nu) */
    double rtol, atol, dtol; /* KSPSetTolerances, :621-623 */
    int max_it;         /* :625 */
    int nsmooth;        /* smoother iterations per sweep, :635 */
    int ncoarse;        /* coarse-solve iterations, :631 */
    double cheb_lo, cheb_hi; /* Chebyshev window as fractions of the eigenvalue estimate */
    int nlanczos;       /* Lanczos steps for the eigenvalue estimates */
    int fine_eig;       /* fine-level estimate: 0 = rigorous element bound (free), 1 = Lanczos like the coarse levels */
    /* 0: CG + V-cycle with Chebyshev/Jacobi smoothers -- the fast path (the option string of SURVEY 8(d));
     * 1: the configuration the reference hard-codes, run as written (a correctness mode, ONE device, ~1000 launches per
     *    Gauss-Seidel sweep): FGMRES(restart) + V-cycle whose smoothers are GMRES(nsmooth) for nsmooth iterations and whose
     *    coarse solve is GMRES(coarse_restart), at most ncoarse iterations to coarse_rtol on the preconditioned residual
     *    (LinearElasticity.cc:620-746, PDEFilter.cc:276-378; csrc/refksp.h) */
    int ksp_mode;
    int restart;         /* KSPGMRESSetRestart of the outer FGMRES, :624 (100) */
    int smooth_pc;       /* PC of the level smoothers: 0 PCJACOBI, 1 PCSOR (one local symmetric sweep, omega 1), :745 */
    int coarse_pc;       /* PC of the coarse solve, :731 */
    int coarse_restart;  /* :632 (30) */
    double coarse_rtol;  /* :628 (1e-8) */
    /* ksp_mode 0, coarsest level: 0 = Chebyshev run of ncoarse steps on [smallest Ritz value, cheb_hi * largest];
     * 1 = exact solve (banded Cholesky + explicit triangular inverse, csrc/coarse_direct.h) where the level has at most
     * 4096 rows on one rank (or is replicated) -- closer to the reference's coarse KSP to rtol 1e-8 (:628-632) than a
     * fixed polynomial; larger or distributed coarsest grids fall back to 0, and so do grids of <= 448 rows, whose
     * Chebyshev run stays inside one workgroup (2 = exact also there) */
    int coarse_direct;
} tp_solver_opts;
void tp_solver_default_opts(tp_solver_opts *o);
/* The option structs grow at their END from round to round.  A host built against an older header would have the library
 * read past its struct: hosts compare these two numbers with their own header at load time (the Python host in lib.py,
 * the C++ hosts in host/topopt_host.h) and refuse to run on a mismatch. */
#define TP_ABI_VERSION 4
int tp_abi_version(void);                 /* the library's TP_ABI_VERSION */
unsigned long tp_solver_opts_size(void);  /* the library's sizeof(tp_solver_opts) */

typedef struct tp_elasticity tp_elasticity;
/* LinearElasticity::LinearElasticity + SetUpLoadAndBC (LinearElasticity.cc:12-180):
 * computes KE (Hex8Isoparametric, :841-998).  N [dev, local nodes*3, 1 = free /
 * 0 = clamped] and RHS [dev, local nodes*3] are the Dirichlet and load vectors;
 * tp_elasticity_cantilever fills them with the reference's load case. */
int tp_elasticity_create(tp_elasticity **e, tp_grid *g, const tp_solver_opts *o);
/* the same with the caller's element matrix (row-major 24x24, reference corner order) instead of the built-in
 * Hex8Isoparametric: what a host that "assembles" with MatSetValuesLocal has computed itself (:118-123, :519-524) */
int tp_elasticity_create_ke(tp_elasticity **e, tp_grid *g, const tp_solver_opts *o, const double *ke_host_576);
int tp_elasticity_destroy(tp_elasticity *e);
int tp_elasticity_get_ke(const tp_elasticity *e, double *ke_host_576);
/* The element matrix the fine-level kernels apply INSIDE THE PRECONDITIONER (smoother, V-cycle residual): KE in its packed
 * Walsh-Hadamard block form, 36 values -- the 33 structural ones and KE's three translation residues; it differs from KE by
 * less than one unit in the last place of KE's largest entry -- as a double-double pair hi + lo (host arrays of 576).
 * Test/diagnostic entry point: the parity checks hand it to the extended-precision arbiter (the 80-bit rebuild of the CPU checker). */
int tp_elasticity_get_ke_effective(const tp_elasticity *e, double *hi_host_576, double *lo_host_576);
/* The element matrix of the KRYLOV operator -- A p and the initial residual of CG (KSPSolve,
 * /root/reference/LinearElasticity.cc:204; tp_elasticity_apply_krylov): the packed form plus the translation mode's
 * column and row of T KE T / 64 exactly as KE has them (132 more values).  On a displacement field whose translation
 * dominates its strain (any iterate of the state solve) its action is KE's to rounding; the residual history follows the
 * reference's KE to 1e-12.  Same double-double convention. */
int tp_elasticity_get_ke_krylov(const tp_elasticity *e, double *hi_host_576, double *lo_host_576);
int tp_elasticity_cantilever(tp_elasticity *e, double *N, double *RHS);      /* :143-171 */
int tp_elasticity_set_bc(tp_elasticity *e, const double *N);                /* N [dev] */
/* AssembleStiffnessMatrix + KSPSetOperators/KSPSetUp (:487-549, :198-200):
 * E = Emin + x^p (Emax-Emin), Galerkin coarse operators, Jacobi diagonals,
 * Chebyshev windows.  xPhys [dev, own elements].  RHS is NOT modified here;
 * tp_elasticity_solve multiplies the load by N as :542 does. */
int tp_elasticity_assemble(tp_elasticity *e, const double *xPhys, double Emin, double Emax, double penal);
/* MatMult with the operator  N K(x) N + (I - N).  u, y [dev, local nodes*3];
 * ghost planes of u are refreshed internally, y is valid on owned planes. */
int tp_elasticity_apply(tp_elasticity *e, const double *u, double *y);
/* The same product with the operator the Krylov method multiplies with inside tp_elasticity_solve (KE_krylov, see
 * tp_elasticity_get_ke_krylov): KE's action to rounding on fields whose translation dominates their strain.
 * tp_elasticity_apply itself applies the packed form (tp_elasticity_get_ke_effective: within 5e-16 max|KE| of KE entrywise). */
int tp_elasticity_apply_krylov(tp_elasticity *e, const double *u, double *y);
/* The same call, which also returns the value of the product's fused dot product: *dot (host) = u . y summed over the owned
 * dofs of all ranks -- CG's p . A p, accumulated per thread inside the kernel and finished by its reduction tail.  y is
 * tp_elasticity_apply_krylov's bit for bit.  For tests of who owns a seam node in that sum. */
int tp_elasticity_apply_krylov_dot(tp_elasticity *e, const double *u, double *y, double *dot);
/* KSPSolve(ksp, RHS, U) with a warm start from U (:204, :647).  U, RHS [dev,
 * local nodes*3].  its / rnorm as KSPGetIterationNumber / KSPGetResidualNorm
 * (:212-213).  hist (host, may be NULL) receives ||b - A x_k|| for k = 0..its,
 * at most hist_cap entries. */
int tp_elasticity_solve(tp_elasticity *e, const double *RHS, double *U, int *its, double *rnorm, double *bnorm,
                        double *hist, int hist_cap);
/* ComputeObjectiveConstraintsSensitivities minus the solve (:377-437):
 * fx = sum E_e u^T KE u, gx = sum x / n - volfrac, dfdx, dgdx = 1/n.
 * U [dev, local nodes*3], xPhys, dfdx, dgdx [dev, own elements] (dgdx may be NULL). */
int tp_elasticity_objective(tp_elasticity *e, const double *U, const double *xPhys, double Emin, double Emax,
                            double penal, double volfrac, double *fx, double *gx, double *dfdx, double *dgdx);
/* The reference's split forms.  ComputeObjectiveConstraints minus the solve (/root/reference/LinearElasticity.cc:237-294):
 * fx and gx of the state U, no sensitivities written. */
int tp_elasticity_objective_only(tp_elasticity *e, const double *U, const double *xPhys, double Emin, double Emax,
                                 double penal, double volfrac, double *fx, double *gx);
/* ComputeSensitivities (/root/reference/LinearElasticity.cc:299-361): dfdx = -p x^(p-1) (Emax - Emin) u^T KE u and
 * dgdx = 1/n (may be NULL) of the state U as it is -- no solve, no reduction, no host synchronisation. */
int tp_elasticity_sensitivities(tp_elasticity *e, const double *U, const double *xPhys, double Emin, double Emax,
                                double penal, double *dfdx, double *dgdx);
/* Several load cases on one design: the weighted response  sum_l w_l sum_e E_e v_l^T KE u_l  and its sensitivity,
 * all cases in ONE pass over the elements (xPhys read once, dfdx written once, one reduction and one host
 * synchronisation for all sums).  V_l = U_l is the compliance of case l; V_l an adjoint state gives the sensitivity of
 * any linear response of U_l.  Pointer convention of tp_mma_update's dgdx: host arrays of device pointers.  The ghost
 * planes of every distinct vector are refreshed first.  With fx, gx and f_case all NULL nothing is reduced and the host
 * does not wait (tp_elasticity_sensitivities' contract).  ncase = 1, V = w = NULL: tp_elasticity_objective's dfdx bit
 * for bit; its fx to rounding (x^p is formed as x^(p-1) x).  TP_ERR_ARG unless 1 <= ncase <= TP_MAX_CASES and e, U,
 * xPhys and every U[l] are given. */
#define TP_MAX_CASES 8
int tp_elasticity_response(tp_elasticity *e, int ncase,
        const double *const *U,   /* host array of ncase [dev] pointers, local nodes*3 each            */
        const double *const *V,   /* same; NULL, or an entry NULL: V_l = U_l (compliance)              */
        const double *w,          /* host, ncase weights; NULL = all 1                                  */
        const double *xPhys, double Emin, double Emax, double penal, double volfrac,
        double *f_case,           /* host, ncase: f_l = sum_e E_e v_l^T KE u_l, UNWEIGHTED; may be NULL */
        double *fx, double *gx,   /* fx = sum_l w_l f_l ; gx as tp_elasticity_objective; may be NULL    */
        double *dfdx,             /* [dev] -p x^(p-1) (Emax-Emin) sum_l w_l v_l^T KE u_l ; may be NULL  */
        double *dgdx);            /* [dev] 1/n ; may be NULL                                            */
/* Relaxed von Mises stress at the element centroids, its p-norm over all ranks, and the two ingredients of the
 * p-norm's design sensitivity.  U [dev, local nodes*3] (ghost planes refreshed inside); xPhys [dev, own elements].
 * With B0 the strain-displacement matrix at the centroid, C the unit-modulus isotropic matrix and Vm the von Mises matrix,
 * M = B0^T C^T Vm C B0 (tp_elasticity_get_stress_form; always from the grid's h and opts.nu, also with a caller's KE):
 *   s_e = u_e^T M u_e,  vm_e = Emax x_e^q sqrt(s_e),  pnorm = (sum_e vm_e^P)^(1/P)
 *   dpdx_e  = pnorm^(1-P) q Emax^P x_e^(qP-1) s_e^(P/2)                        (explicit part, 0 at x_e = 0)
 *   adj_rhs = d pnorm / dU = sum_e pnorm^(1-P) (Emax x_e^q)^P s_e^((P-2)/2) L_e^T M u_e   (owned planes; N NOT applied)
 * Total derivative: solve K lambda = N adj_rhs (tp_elasticity_solve applies N), then
 *   d pnorm / dx = dpdx + dfdx of tp_elasticity_response(ncase 1, U = u, V = lambda, w = NULL), no sums.
 * Elements with s_e = 0 contribute exactly 0; pnorm = 0 leaves dpdx and adj_rhs all zero.  With only vm asked for
 * nothing is reduced and the host does not wait; otherwise one reduction and one host read.
 * TP_ERR_ARG unless P >= 2, q >= 0 and (q == 0 or q P >= 1). */
int tp_elasticity_stress(tp_elasticity *e, const double *U, const double *xPhys, double Emax, double q, double P,
        double *vm,       /* [dev, own elements]; may be NULL */
        double *pnorm,    /* host; may be NULL */
        double *vm_max,   /* host, max over all ranks; may be NULL */
        double *dpdx,     /* [dev, own elements] explicit part; may be NULL */
        double *adj_rhs); /* [dev, local nodes*3] d pnorm / dU on owned planes; may be NULL */
int tp_elasticity_get_stress_form(const tp_elasticity *e, double *m_host_576);
/* Self-weight: a body force b = (b_x, b_y, b_z) per unit volume at full density (rho g) that moves with the material.
 * V_e = hx hy hz; mass interpolation m(x) = x for x >= x_low (or x_low = 0), m(x) = x t^5 (6 - 5 t) with t = x / x_low below
 * (m' = t^5 (36 - 35 t); C1 at x_low, m / x^p bounded), x >= 0.
 *   load:         rhs_n = rhs_base_n + (V_e / 8) b sum_{e contains n} m(x_e)   on the OWNED node planes (ghost planes are left
 *                 as they are; supports not applied -- tp_elasticity_solve multiplies by N); rhs_base NULL = 0, rhs == rhs_base
 *                 works in place.  A gather in one fixed order: the same bits on any number of slabs.
 *   sensitivity:  dfdx_e += scale m'(x_e) (V_e / 8) sum_l w_l sum_{a = 1..8} sum_c b_c N_{a,c} V_l,{a,c}   (the supports N of the
 *                 handle applied inside; the ghost planes of every distinct V_l are refreshed first).
 * With K u = N (F + f(x)):  d(u^T K u)/dx = tp_elasticity_response's dfdx + the term with V = u, scale = 2; a response with
 * adjoint state lam gains the term with V = lam, scale = 1.  Neither call reduces anything or makes the host wait.
 * TP_ERR_ARG unless e, xPhys, b3, rhs / dfdx and every V[l] are given, 0 <= x_low < 1, b3 and scale are finite and
 * 1 <= ncase <= TP_MAX_CASES; TP_ERR_STATE before the supports are set. */
int tp_elasticity_body_load(tp_elasticity *e, const double *xPhys /*[dev, own elements]*/, const double *b3 /*host, 3*/,
                            double x_low, const double *rhs_base /*[dev, local nodes*3] or NULL*/, double *rhs /*[dev]*/);
int tp_elasticity_body_sensitivity(tp_elasticity *e, int ncase, const double *const *V /*host array of [dev] pointers*/,
                            const double *w /*host, NULL = all 1*/, const double *xPhys, const double *b3, double x_low,
                            double scale, double *dfdx /*[dev, own elements], added to*/);
/* Thermal expansion: a nodal temperature field T loads the structure.  theta = T - T_ref at the nodes; element e pushes on its 24
 * dofs with beta(x_e) G theta_e, G[(a,c), b] = 1 / (1 - 2 nu) int dN_a/dx_c N_b dV the 24 x 8 coupling matrix of the box element
 * (row 3 a + c, row major; nu the handle's), beta(x) = alpha (Emin + x^penal_beta (Emax - Emin)).
 *   load:         rhs_n = rhs_base_n + sum_{e contains n} beta(x_e) (G theta_e)_n on the OWNED node planes (ghost planes are left
 *                 as they are; supports not applied -- tp_elasticity_solve multiplies by N); rhs_base NULL = 0, rhs == rhs_base
 *                 works in place.  A gather in one fixed order: the same bits on any number of slabs.
 *   sensitivity:  dfdx_e += scale beta'(x_e) sum_l w_l (N V_l)_e^T G theta_e   (the partial derivative at fixed T).
 *   adjoint rhs:  g_n = scale sum_{e contains n} beta(x_e) sum_{a,c} G[(a,c), b(e,n)] (N sum_l w_l V_l)_{a,c}: the transpose of the
 *                 load, one scalar per OWNED node -- the right-hand side of the thermal adjoint.
 * The supports N of the handle are applied inside; the ghost planes of T and of every distinct V_l are refreshed first.  With
 * K u = N (F + f_th) and A(k) T = N_T q:  d(u^T K u)/dx = tp_elasticity_response's dfdx + the sensitivity with V = u, scale = 2,
 * + tp_conduction_response's dfdx with T = [T], V = [mu], w = [2], where A mu = N_T g(u) (scale 1).  No call reduces anything
 * or makes the host wait.
 * TP_ERR_ARG unless every pointer but rhs_base and w is given, alpha and T_ref are finite, penal_beta >= 1, Emin >= 0,
 * Emax > Emin, scale is finite and 1 <= ncase <= TP_MAX_CASES; TP_ERR_STATE before the supports are set. */
typedef struct { double alpha, T_ref, Emin, Emax, penal_beta; } tp_thermal_par;
int tp_elasticity_thermal_load(tp_elasticity *e, const double *xPhys /*[dev, own elements]*/, const double *T /*[dev, local nodes]*/,
                            const tp_thermal_par *par, const double *rhs_base /*[dev, local nodes*3] or NULL*/, double *rhs /*[dev]*/);
int tp_elasticity_thermal_sensitivity(tp_elasticity *e, int ncase, const double *const *V /*host array of [dev] pointers*/,
                            const double *w /*host, NULL = all 1*/, const double *xPhys, const double *T,
                            const tp_thermal_par *par, double scale, double *dfdx /*[dev, own elements], added to*/);
int tp_elasticity_thermal_adjoint_rhs(tp_elasticity *e, int ncase, const double *const *V, const double *w, const double *xPhys,
                            const tp_thermal_par *par, double scale, double *g /*[dev, local nodes], owned planes written*/);
int tp_elasticity_get_thermal_coupling(const tp_elasticity *e, double *G_host_192);
/* introspection for parity tests: beta(x_e) and beta'(x_e) of the own elements, as the three calls above form them; one of the
 * two outputs may be NULL (the load and the adjoint rhs form beta alone, the sensitivity beta' alone) */
int tp_elasticity_thermal_coefficients(tp_elasticity *e, const double *xPhys, const tp_thermal_par *par,
                            double *beta /*[dev, own elements]*/, double *dbeta /*[dev, own elements]*/);
/* The consistent mass matrix as an operator, and the mass half of an eigenvalue's design sensitivity (free vibration:
 * A phi = lambda B phi with A = N K N + (I - N), what tp_elasticity_apply applies, and B = N M N).
 *   M_e = rho0 m(x_e) V_e (M8 (x) I_3),  M8[a,b] = (1/8) prod_axis (2/3 if corners a, b share that coordinate, else 1/3)
 * (1/27, 1/54, 1/108, 1/216 for corner pairs that differ along 0, 1, 2, 3 axes; sum_ab M8 = 1), m, m' and x_low those of the
 * self-weight above.
 *   mass_assemble:    rho0 V_e m(x_e) of the own elements and the ghost layer above, once per design; what the two calls below use
 *   mass_apply:       y = N M N u on the OWNED node planes (the ghost planes of u are refreshed inside, those of y are left as
 *                     they are; u != y).  A gather in one fixed order: the same bits on any number of slabs.
 *   mass_sensitivity: out_e += scale m'(x_e) rho0 V_e sum_l w_l (N V_l)_e^T (M8 (x) I_3) (N V_l)_e   (rho0, x_low of the last
 *                     mass_assemble; xPhys the design it was called with; w NULL = all 1; ghost planes of every distinct V_l
 *                     refreshed first).  No reduction, the host does not wait.
 * For a mode with phi^T B phi = 1:  d lambda / dx = dfdx of tp_elasticity_response(U = V = phi) with the sign turned
 * (+p x^(p-1) (Emax - Emin) phi_e^T KE phi_e) plus the term with V = phi, scale = -lambda.
 * TP_ERR_ARG, before the grid is touched, unless e, xPhys, u, y, out and every V[l] are given, rho0 > 0 and finite,
 * 0 <= x_low < 1, 1 <= ncase <= TP_MAX_CASES and scale is finite; TP_ERR_STATE before the supports are set, and for the last two
 * before mass_assemble. */
int tp_elasticity_mass_assemble(tp_elasticity *e, const double *xPhys /*[dev, own elements]*/, double rho0, double x_low);
int tp_elasticity_mass_apply(tp_elasticity *e, const double *u /*[dev, local nodes*3]*/, double *y /*[dev, local nodes*3]*/);
int tp_elasticity_mass_sensitivity(tp_elasticity *e, int ncase, const double *const *V /*host array of [dev] pointers*/,
                            const double *w /*host, NULL = all 1*/, const double *xPhys, double scale,
                            double *out /*[dev, own elements], added to*/);
/* The geometric (stress) stiffness as an operator and its two derivatives: the pieces of a linear buckling analysis
 * B phi = mu A phi with B = -N G(x, u) N, A as above, u the state of one load case (load factors 1 / mu of the positive mu).
 *   sigma(gp) = C0 B(gp) u_e at the 8 Gauss points of the element (2 x 2 x 2 rule, weight hx hy hz / 8, C0 the unit-modulus
 *   isotropic matrix),  g_e[a,b] = sum_gp w gradN_a(gp)^T S(sigma(gp)) gradN_b(gp)  (8 x 8, symmetric, rows sum to zero),
 *   G_e = Emax x_e^penal (g_e (x) I_3)  -- no Emin: a void element carries no stress stiffness.
 *   geom_assemble:    Emax x_e^penal g_e(u_e) of the own elements and the ghost layer above (28 entries a < b), once per design
 *                     and state; the ghost planes of U are refreshed inside
 *   geom_apply:       y = N G N phi on the OWNED node planes (the ghost planes of phi are refreshed inside, those of y are left
 *                     as they are; phi != y).  A gather in one fixed order: the same bits on any number of slabs.
 *   geom_sensitivity: out_e += scale penal x_e^(penal-1) Emax sum_l w_l (N Phi_l)_e^T (g_e(U_e) (x) I_3) (N Phi_l)_e  (w NULL = all
 *                     1; ghost planes of every distinct Phi_l and of U refreshed first).  No reduction, the host does not wait.
 *   geom_adjoint_rhs: out = scale sum_l w_l d((N Phi_l)^T G (N Phi_l)) / dU on the OWNED node planes, supports not applied
 *                     (tp_elasticity_solve multiplies by N); ghost planes of out stay.  A gather in one fixed order.
 * TP_ERR_ARG, before the grid is touched, unless every pointer is given, Emax > 0, penal >= 1 and scale are finite and
 * 1 <= ncase <= TP_MAX_CASES; TP_ERR_ARG for the last three before a geom_assemble; TP_ERR_STATE for geom_assemble before
 * the supports are set. */
int tp_elasticity_geom_assemble(tp_elasticity *e, const double *xPhys /*[dev, own elements]*/, const double *U /*[dev, local nodes*3]*/,
                            double Emax, double penal);
int tp_elasticity_geom_apply(tp_elasticity *e, const double *phi /*[dev, local nodes*3]*/, double *y /*[dev, local nodes*3]*/);
int tp_elasticity_geom_sensitivity(tp_elasticity *e, int ncase, const double *const *Phi /*host array of [dev] pointers*/,
                            const double *w /*host, NULL = all 1*/, const double *xPhys, const double *U, double Emax, double penal,
                            double scale, double *out /*[dev, own elements], added to*/);
int tp_elasticity_geom_adjoint_rhs(tp_elasticity *e, int ncase, const double *const *Phi /*host array of [dev] pointers*/,
                            const double *w /*host, NULL = all 1*/, const double *xPhys, double Emax, double penal, double scale,
                            double *out /*[dev, local nodes*3]*/);
/* the element's tables for the parity tests: gradN[(3 gp + d) * 8 + n] = dN_n/dx_d, cb[(6 gp + r) * 24 + j] = (C0 B(gp))[r][j] */
int tp_elasticity_get_geom_tables(const tp_elasticity *e, double *gradN_host_192, double *cb_host_1152);
/* introspection for parity tests */
/* KSPSetTolerances (LinearElasticity.cc:646); a negative value keeps the current one (PETSC_DEFAULT) */
int tp_elasticity_set_tolerances(tp_elasticity *le, double rtol, double atol, double dtol, int max_it);
/* The parity solver as a literal PETSc 3.11 option string with the numeric per-level Chebyshev windows of the last
 * tp_elasticity_assemble (KSPSetFromOptions, LinearElasticity.cc:659; -mg_levels_N_ksp_chebyshev_eigenvalues a,b):
 * someone with a PETSc build can paste it on the reference's command line and compare the residual history.
 * Returns the length of the full string (buf receives at most cap-1 characters), or -1 before the first assembly. */
int tp_elasticity_petsc_options(const tp_elasticity *e, char *buf, size_t cap);
/* PCMGSetCycleType / PCMGSetCycleTypeOnLevel: cycles[l] cycles of level l + 1 per visit of level l (l = 0 finest, 1 = V,
 * 2 = W; PETSc's form: same right-hand side, the next cycle starts from the previous one's iterate); one cycle into the
 * coarsest level whatever is set */
int tp_elasticity_set_cycles(tp_elasticity *e, const int *cycles, int n);
/* ---- the multigrid hierarchy level by level (tests, tools, bench.py) ----
 * tp_elasticity_, tp_conduction_ and tp_pdefilter_ carry the same calls on their solver's levels (0 = the finest): level_count,
 * level_nodes, level_lambda, level_lambda_min, level_apply, level_diag, smooth, level_residual, restrict, prolong_add,
 * last_op_form, last_stats (the PDE filter: no level_residual, no last_stats).  Vectors: [dev, the level's local dofs].
 * ONE contract, every rule answered before anything is launched or written, checked in this order:
 *   1. a NULL handle, a NULL vector or output pointer (form4 too; the three of last_stats may be NULL), k < 0 in smooth:
 *      TP_ERR_ARG.  level_count and level_nodes answer -TP_ERR_ARG, the lambdas NaN -- for a NULL handle or a level that is not
 *      there; these four ask for no assembly.
 *   2. a handle that cannot answer: elasticity and conduction TP_ERR_STATE before the first assemble (level_apply, level_diag,
 *      smooth, level_residual, and the elasticity-only precond, level_pc, level_gs, level_gmres, smooth_dot); the PDE filter
 *      TP_ERR_ARG on EVERY call for a filter that is not of type 2 (its hierarchy is complete from tp_filter_create on).
 *      restrict, prolong_add, last_op_form and last_stats ask for no assembly.
 *   3. a level the hierarchy does not have: TP_ERR_ARG; restrict and prolong_add go between level and level + 1 and need both.
 * smooth with k == 0 is legal (the two copies alone), except on the PDE filter (TP_ERR_ARG).  What is particular to a call comes
 * after these: TP_ERR_STATE from level_pc / level_gs / level_gmres outside ksp_mode 1 and from smooth_dot on a level whose kernel
 * carries no fused dot. */
int tp_elasticity_level_count(const tp_elasticity *e);
long tp_elasticity_level_nodes(const tp_elasticity *e, int level);
double tp_elasticity_level_lambda(const tp_elasticity *e, int level);
/* lower end of the Chebyshev window of the coarsest level (smallest Ritz value of its 40-step Lanczos run; the reference
 * has GMRES there and needs no window: /root/reference/src/LinearElasticity.cc:760-790); 0 on the other levels */
double tp_elasticity_level_lambda_min(const tp_elasticity *e, int level);
/* rows of the coarsest level if the last assembly factored it for the exact coarse solve (tp_solver_opts.coarse_direct),
 * 0 if the Chebyshev run is in use (option off, level too large or distributed) */
int tp_elasticity_coarse_direct_active(const tp_elasticity *e);
/* Process-wide state of the recovery from one-XCD persistent kernels that gave up (their workgroups not co-resident: a
 * shared device): how many recoveries so far, whether the one-XCD forms are off, whether the coarse factorisation is no
 * longer deferred into the head of the solve (the softer first answer when only that chain gave up).  No reference
 * counterpart: PETSc's KSPSolve (LinearElasticity.cc:204) has no persistent kernels. */
int tp_xcd_status(int *giveups, int *xcd_forms_off, int *defer_off);
int tp_elasticity_level_apply(tp_elasticity *e, int level, const double *u, double *y); /* [dev, level local dofs] */
int tp_elasticity_level_diag(tp_elasticity *e, int level, double *d);
int tp_elasticity_precond(tp_elasticity *e, const double *r, double *z); /* one V-cycle */
/* ksp_mode 1 level by level (tests): z = M^-1 r with PCJACOBI (pc 0) or PCSOR (pc 1) on a level; the level's left-
 * preconditioned GMRES(m) for at most `its` iterations on x (rtol < 0: no convergence test, as PCMG runs its smoothers) */
int tp_elasticity_level_pc(tp_elasticity *e, int level, int pc, const double *r, double *z);
/* one in-place Gauss-Seidel sweep of PCSOR on x, from the iterate x holds: forward (backward == 0) or backward.  Forward from
 * zero, then backward, is tp_elasticity_level_pc(pc 1) launch for launch.  TP_ERR_STATE outside ksp_mode 1. */
int tp_elasticity_level_gs(tp_elasticity *e, int level, int backward, const double *b, double *x);
int tp_elasticity_level_gmres(tp_elasticity *e, int level, int pc, int m, int its, double rtol, const double *b, double *x,
                              int zero_guess, int *its_done);
/* k Chebyshev-Jacobi steps on a level (the fused operator+update kernel): x <- smooth(b, x) */
int tp_elasticity_smooth(tp_elasticity *e, int level, const double *b, double *x, int k, int zero_guess);
/* The same sweep with the LAST step's fused dot product: *dot (host) = b . x_out, the r . z that the V-cycle's last
 * post-smoothing step hands to CG; x is tp_elasticity_smooth's bit for bit.  TP_ERR_STATE where the level's kernel carries no
 * fused dot (anything but the fine tile kernels of generation 2 and 3), TP_ERR_ARG where no operator step would run
 * (k < 1; the zero guess with k < 2: its first step is a scaling). */
int tp_elasticity_smooth_dot(tp_elasticity *e, int level, const double *b, double *x, int k, int zero_guess, double *dot);
/* r = b - A_level x through the residual epilogue of the level's operator kernel, as the V-cycle forms it before every
 * restriction (the ghost planes of x are refreshed first; r is valid on the owned planes).  On level 0 the operator is the
 * preconditioner's packed form (tp_elasticity_get_ke_effective), not the Krylov product. */
int tp_elasticity_level_residual(tp_elasticity *e, int level, const double *b, const double *x, double *r);
int tp_elasticity_restrict(tp_elasticity *e, int level, const double *rf, double *rc);
int tp_elasticity_prolong_add(tp_elasticity *e, int level, const double *xc, double *xf);
/* bytes moved / flops of the last call, by the algorithmic model of DESIGN.md */
int tp_elasticity_last_stats(const tp_elasticity *e, double *alg_bytes, double *flops, long *kernel_launches);
/* which kernel form the last operator application (apply, level_apply, smooth, ...) launched, for tests that force a form
 * through the environment and must not pass on another one: form4[0] 1 fine tile kernel, 2 level 1 applied from the fine
 * densities, 3 per-node matrix-free kernel, 4 stored stencil; [1] fine: generation 1..3, level 1: 1 if the Dirichlet
 * correction was fused, per-node kernel: 1 if it applied the scalar (Helmholtz) operator from its 27-point weight table,
 * 0 for the gather over the elements (elasticity always; the PDE filter with TP_NO_PDE_STENCIL), stencil: threads per
 * row 9 / 3 / 1; [2] fine: tile 0 = 15 x 15 nodes, 1 = 16x16, 2 = 32x8,
 * 3 = 32x16, stencil: 1 = node form; [3] fine and level 1: z-chunk length, stencil: 1 = mirrored reads */
int tp_elasticity_last_op_form(const tp_elasticity *e, int *form4);

/* ---- steady heat conduction ------------------------------------------------
 * The scalar problem  A(k) T = N q,  A = N K(k) N + (I - N):  one conductivity per element, k_e = kmin + x_e^penal (kmax - kmin),
 * the element matrix KT = int grad N_a . grad N_b of the grid's box element (8 x 8, reference corner order), N a 0/1 vector
 * per local node (0: heat sink, T = 0).  Solved like the elasticity problem: CG preconditioned by one multigrid V-cycle with
 * Chebyshev-Jacobi smoothing, the fine level applied from the conductivities, every coarser level a true Galerkin product
 * P^T A P stored as 27 diagonals, the coarsest one a Chebyshev run of ncoarse steps over its whole spectrum (coarse_direct is
 * ignored).  tp_solver_opts as for elasticity (nu unused); ksp_mode 1 is TP_ERR_ARG at creation, and so is a mesh that does not
 * coarsen nlvls - 1 times or a slab too thin for it.
 * Every call answers TP_ERR_ARG -- before the handle or the grid is touched -- for a NULL handle or vector, kmin <= 0,
 * kmax <= kmin, penal < 1, any non-finite parameter, ncase outside 1..TP_MAX_CASES, a level the hierarchy does not have; and
 * TP_ERR_STATE before set_bc (assemble, response) or before assemble (apply, solve, the level calls). */
typedef struct tp_conduction tp_conduction;
int tp_conduction_create(tp_conduction **c, tp_grid *g, const tp_solver_opts *o);
int tp_conduction_destroy(tp_conduction *c);                    /* NULL: TP_OK */
int tp_conduction_get_ke(const tp_conduction *c, double *kt_host_64);
int tp_conduction_set_bc(tp_conduction *c, const double *N /*[dev, local nodes], 0/1*/);
int tp_conduction_assemble(tp_conduction *c, const double *xPhys /*[dev, own elements]*/, double kmin, double kmax, double penal);
int tp_conduction_apply(tp_conduction *c, const double *u, double *y);   /* y = A u, [dev, local nodes] */
/* the same product as CG forms it, with the fused dot product: *dot (host) = u . y over all ranks; dot NULL: nothing is read
 * back and the host does not wait */
int tp_conduction_apply_dot(tp_conduction *c, const double *u, double *y, double *dot);
/* RHS .* N is solved for (as tp_elasticity_solve does it), warm-started from T; its / rnorm / bnorm / hist as there */
int tp_conduction_solve(tp_conduction *c, const double *RHS, double *T, int *its, double *rnorm, double *bnorm, double *hist,
                        int hist_cap);
/* tp_elasticity_response's contract with 8-vectors:  f_case[l] = sum_e k_e v_e^T KT t_e (V[l] NULL: v = t, the thermal compliance of
 * case l),  *fx = sum_l w_l f_case[l],  *gx = sum x / n_elements - volfrac,  dfdx_e = -penal x^(penal-1) (kmax - kmin) sum_l w_l v_e^T KT t_e,
 * dgdx = 1 / n_elements.  One pass over the elements, one reduction, one host read; with f_case, fx and gx all NULL nothing is
 * reduced and the host does not wait.  The ghost planes of every distinct T[l], V[l] are refreshed first. */
int tp_conduction_response(tp_conduction *c, int ncase,
        const double *const *T,   /* host array of ncase [dev] pointers, local nodes each              */
        const double *const *V,   /* NULL, or ncase entries, each NULL (= T[l]) or a [dev] vector       */
        const double *w,          /* host, ncase weights; NULL = all 1                                  */
        const double *xPhys, double kmin, double kmax, double penal, double volfrac,
        double *f_case, double *fx, double *gx, double *dfdx, double *dgdx);
int tp_conduction_set_tolerances(tp_conduction *c, double rtol, double atol, double dtol, int max_it);   /* negative: keep */
/* the hierarchy level by level, as the tp_elasticity_ calls of the same names; vectors [dev, the level's local nodes].
 * level_count / level_nodes answer -TP_ERR_ARG, the lambdas NaN, where the others answer TP_ERR_ARG (the contract stated above
 * tp_elasticity_level_count: this family's, now every family's). */
int tp_conduction_level_count(const tp_conduction *c);
long tp_conduction_level_nodes(const tp_conduction *c, int level);
double tp_conduction_level_lambda(const tp_conduction *c, int level);
double tp_conduction_level_lambda_min(const tp_conduction *c, int level);
int tp_conduction_level_apply(tp_conduction *c, int level, const double *u, double *y);
int tp_conduction_level_diag(tp_conduction *c, int level, double *dinv);
int tp_conduction_smooth(tp_conduction *c, int level, const double *b, double *x, int k, int zero_guess);
int tp_conduction_level_residual(tp_conduction *c, int level, const double *b, const double *x, double *r);
int tp_conduction_restrict(tp_conduction *c, int level, const double *rf, double *rc);
int tp_conduction_prolong_add(tp_conduction *c, int level, const double *xc, double *xf);
/* form4 as tp_elasticity_last_op_form; the fine level is a per-node kernel ([0] = 3) with [1] = 2 for the register form of
 * conduction.h and 0 for the gather over the elements (TP_NO_COND_STENCIL set) */
int tp_conduction_last_op_form(const tp_conduction *c, int *form4);
int tp_conduction_last_stats(const tp_conduction *c, double *alg_bytes, double *flops, long *kernel_launches);

/* ---- density / sensitivity filter (Filter.cc) --------------------------- */
typedef struct tp_filter tp_filter;
/* Filter::Filter + SetUp (Filter.cc:25-38, :290-463).  filterType 0 = sensitivity,
 * 1 = density, 2 = PDE (Helmholtz), other = none; rmin is an absolute length.  Type 2: pde_opts (NULL: the reference's) are
 * checked against the grid as tp_elasticity_create checks its own -- nlvls outside 1..TP_MAX_LEVELS, a mesh that does not coarsen
 * nlvls - 1 times, a ksp_mode other than 0 or 1 (1: one device only) are TP_ERR_ARG -- without the slab-thickness rule. */
int tp_filter_create(tp_filter **f, tp_grid *g, int filterType, double rmin, const tp_solver_opts *pde_opts);
/* y = H x, the un-normalised cone filter: MatMult(H, x, y) of Filter.cc:68, :173, :181 (types 0, 1) */
int tp_filter_mult_h(tp_filter *f, const double *x, double *y);
int tp_filter_destroy(tp_filter *f);
int tp_filter_stencil_width(const tp_filter *f);        /* ElemConn, Filter.cc:326 */
/* which cone-filter kernel the last convolution (project, gradients, mult_h) launched, for tests: 1 LDS-tiled, 2 several
 * outputs per thread along z, 3 wide (ElemConn 3..8), 4 streamed ring (9..24), 5 generic loop; 0 none yet */
int tp_filter_last_kernel(const tp_filter *f);
int tp_filter_get_hs(tp_filter *f, double *Hs);          /* [dev, own elements] */
/* PDE filter (type 2): the 8x8 Helmholtz element matrix KF of PDEFilt::PDEFilterMatrix (PDEFilter.cc:472-576), host */
int tp_filter_get_kf(const tp_filter *f, double *kf_host_64);
/* Filter::FilterProject (:60-117): x -> xTilde -> xPhys [dev, own elements] */
int tp_filter_project(tp_filter *f, const double *x, double *xTilde, double *xPhys, int projectionFilter, double beta,
                      double eta);
/* Filter::Gradients (:120-204): dfdx and dgdx[0..m) filtered in place */
int tp_filter_gradients(tp_filter *f, const double *x, const double *xTilde, double *dfdx, int m, double **dgdx,
                        int projectionFilter, double beta, double eta);
int tp_filter_mnd(tp_filter *f, const double *x, double *mnd);   /* GetMND, :206-225 */
int tp_filter_last_pde_its(const tp_filter *f, int *its, double *rnorm);
/* PDE filter (type 2), the operators of PDEFilt::FilterProject one by one (PDEFilter.cc:198-210): T x (element ->
 * node, the caller scales by the element volume), the Helmholtz solve K_f u = rhs (warm start from u), T^T u, and
 * K_f u itself.  Nodal arrays: [dev, local nodes]; element arrays: [dev, own elements]. */
int tp_pdefilter_elem_to_node(tp_filter *f, const double *x_elem, double *rhs_nodal);
int tp_pdefilter_solve(tp_filter *f, const double *rhs_nodal, double *u_nodal);
int tp_pdefilter_node_to_elem(tp_filter *f, const double *u_nodal, double *x_elem);
int tp_pdefilter_apply(tp_filter *f, const double *u_nodal, double *y_nodal);
/* The PDE filter's scalar multigrid hierarchy level by level, for tests: the contract stated above tp_elasticity_level_count
 * (level 0 of level_apply is tp_pdefilter_apply; level_diag exports the reciprocal Jacobi diagonal).  Vectors: [dev, the level's
 * local nodes].  Particular to the filter: anything but a filter of type 2 is TP_ERR_ARG on every call, smooth refuses k == 0,
 * and there is no level_residual and no last_stats. */
int tp_pdefilter_level_count(const tp_filter *f);
long tp_pdefilter_level_nodes(const tp_filter *f, int level);
double tp_pdefilter_level_lambda(const tp_filter *f, int level);
double tp_pdefilter_level_lambda_min(const tp_filter *f, int level);
int tp_pdefilter_level_apply(tp_filter *f, int level, const double *u, double *y);
int tp_pdefilter_level_diag(tp_filter *f, int level, double *dinv);
int tp_pdefilter_smooth(tp_filter *f, int level, const double *b, double *x, int k, int zero_guess);
int tp_pdefilter_restrict(tp_filter *f, int level, const double *rf, double *rc);
int tp_pdefilter_prolong_add(tp_filter *f, int level, const double *xc, double *xf);
int tp_pdefilter_last_op_form(const tp_filter *f, int *form4);

/* ---- local volume constraint (no reference counterpart; Wu, Aage, Westermann, Sigmund 2018) ---- */
/* The mean density in a ball of radius R around every element, held below alpha through ONE p-norm constraint:
 *   N_e = { j : |c_j - c_e| < R } over element centres (strict; truncated at the domain boundary, as the cone filter),
 *   cnt_e = |N_e|,  rhobar_e = (sum_{j in N_e} xPhys_j) / cnt_e,
 *   pn = ((sum_e rhobar_e^p) / n)^(1/p) over all ranks (n = global element count),  g = pn / alpha - 1,
 *   dgdx_j = sum_{e in N_j} t_e^(p-1) / (alpha n cnt_e),  t_e = rhobar_e / pn        (pn = 0: dgdx = 0).
 * A handle of its own on a grid (any filter type beside it, R unrelated to rmin).  The ball sums are the cone filter's
 * convolution kernels on a 0/1 table; on more than one rank TP_ERR_ARG if the stencil is wider than a slab.  All arrays
 * [dev, own elements].  The sum over the elements runs layer by layer in ascending global z: the results do not depend on
 * the number of slabs, and two calls give the same bits. */
typedef struct tp_localvol tp_localvol;
int tp_localvol_create(tp_localvol **lv, tp_grid *g, double R);   /* TP_ERR_ARG unless R > 0 */
int tp_localvol_destroy(tp_localvol *lv);
int tp_localvol_stencil_width(const tp_localvol *lv);             /* max over the axes of ceil(R/h) - 1, clamped to half the mesh */
int tp_localvol_get_count(tp_localvol *lv, double *cnt);          /* cnt_e */
/* kernel of the last ball sum: the codes of tp_filter_last_kernel */
int tp_localvol_last_kernel(const tp_localvol *lv);
/* rhobar alone: one ball sum, no reduction, the host does not wait */
int tp_localvol_mean(tp_localvol *lv, const double *xPhys, double *rhobar);
/* TP_ERR_ARG unless p >= 1 and alpha > 0.  Without dgdx: one ball sum, one reduction, one host read (one rank); with it
 * a coefficient pass and a second ball sum follow, no further read. */
int tp_localvol_constraint(tp_localvol *lv, const double *xPhys, double alpha, double p,
        double *g,          /* host; may be NULL */
        double *pn,         /* host; may be NULL */
        double *rhobar_max, /* host, max over all ranks; may be NULL */
        double *rhobar,     /* [dev, own elements]; may be NULL */
        double *dgdx);      /* [dev, own elements]; may be NULL */

/* ---- minimum length scale by geometric constraints (no reference counterpart; Zhou, Lazarov, Wang, Sigmund 2015) ---- */
/* Two scalar constraints on the filtered field rt = xTilde and the projected field rb = xPhys, one for the solid phase and
 * one for the void phase; no solve.  With e+_a / e-_a the neighbours of element e along axis a, clamped at the DOMAIN boundary
 * (at a slab border the neighbour is the other rank's element), h_a the spacing and n the GLOBAL element count:
 *   d_{a,e} = rt[e+_a] - rt[e-_a],  G_e = sum_a (d_{a,e} / (2 h_a))^2,  E_e = exp(-c G_e)        (c in units of length^2)
 *   solid: a = rb, m = min(rt - eta_s, 0);   void: a = 1 - rb, m = min(eta_v - rt, 0)
 *   T_e = a_e E_e m_e^2,  S = sum_e T_e over all ranks,  g = S / (n eps) - 1
 * dg_* receive the TOTAL derivative dg / d xTilde: the projection's H' (the parameters tp_filter_project was called with; proj = 0:
 * rb = rt, H' = 1) and the stencil's transpose are inside, so the rows go back through tp_filter_gradients_from_tilde and not
 * through tp_filter_gradients.  kinds: 1 solid | 2 void; a call that asks for one kind writes only that one (g[0], S[0], dg_solid:
 * solid; g[1], S[1], dg_void: void).  All arrays [dev, own elements].  S is summed layer by layer in ascending global z: g and
 * every bit of the gradients do not depend on the number of slabs, and two calls give the same bits.  On more than one rank slabs
 * of fewer than 2 layers are TP_ERR_ARG at creation.  TP_ERR_ARG, before the handle is used, for a NULL handle, xTilde or xPhys,
 * kinds outside 1..3, c < 0, eps <= 0, any non-finite parameter, eta_s or eta_v outside (0, 1), proj with beta <= 0 or eta
 * outside [0, 1]. */
typedef struct tp_lengthscale tp_lengthscale;
int tp_lengthscale_create(tp_lengthscale **ls, tp_grid *g);
int tp_lengthscale_destroy(tp_lengthscale *ls);              /* NULL: TP_OK */
int tp_lengthscale_constraints(tp_lengthscale *ls, const double *xTilde, const double *xPhys,
                               int proj, double beta, double eta,
                               double c, double eta_s, double eta_v, double eps, int kinds /* 1 solid | 2 void */,
                               double *g /*[2], host; may be NULL*/, double *S /*[2], host; may be NULL*/,
                               double *dg_solid, double *dg_void /* d g / d xTilde, either may be NULL */);
/* T_e of the last call, own elements; either may be NULL */
int tp_lengthscale_get_terms(tp_lengthscale *ls, double *T_solid, double *T_void);
/* rows[i] <- (d xTilde / d x)^T rows[i], i < m, in place: the filter's transpose with no projection chain (types 1, 2).
 * TP_ERR_ARG for filter type 0, whose "gradient" is a heuristic on dfdx and not a transpose. */
int tp_filter_gradients_from_tilde(tp_filter *f, const double *x, int m, double **rows);

/* ---- overhang (self-support) filter (no reference counterpart; Langelaar 2016 / 2017) ---- */
/* A "printed" density xi built from the blueprint density x layer by layer from the baseplate: every element takes the smooth
 * minimum of its own density and the smooth maximum of the five elements that support it in the layer below (itself and its
 * four in-plane neighbours: 45 degrees).  Build axis 1 (y) or 2 (z), sign +1 (baseplate at the lowest index) or -1; in-plane
 * (i, r) = x and the remaining axis; Q = P + ln 5 / ln xi0; defaults P = 40, eps = 1e-4, xi0 = 0.5.
 *   xi_0 = x_0;  S = sum over the cross of xi_{l-1}^P (outside the mesh: 0),  Xi = S^(1/Q),  d = x - Xi,  rho = sqrt(d^2 + eps),
 *   xi = (x + Xi - rho + sqrt(eps)) / 2          (no clamp: min(x, Xi) <= xi <= min(x, Xi) + sqrt(eps) / 2)
 * A filter, not a constraint: the responses are evaluated on xi and their gradients come back through the transpose of the
 * forward sweep's Jacobian, which works in place on up to 8 vectors at once from coefficients the forward sweep left in the
 * handle.  All arrays [dev, own elements].  z builds work on any number of slabs (the ranks sweep one after the other, the
 * results are those of one rank bit for bit); TP_ERR_ARG for a y build on more than one rank and for any other axis.
 * Both sweeps advance TP_OVERHANG_CHUNK layers per launch; every value gives the same bits. */
typedef struct tp_overhang tp_overhang;
int tp_overhang_create(tp_overhang **ov, tp_grid *g, int axis /*1 y, 2 z*/, int sign /*+1, -1*/);
int tp_overhang_destroy(tp_overhang *ov);                       /* NULL: 0 */
/* TP_ERR_ARG unless P >= 1, eps > 0, 0 < xi0 < 1 and Q >= 1; a forward call must follow before the next transpose */
int tp_overhang_set_params(tp_overhang *ov, double P, double eps, double xi0);
int tp_overhang_forward(tp_overhang *ov, const double *x, double *xi);   /* TP_ERR_ARG if x == xi */
/* g[v] <- J^T g[v], v < nvec, 1 <= nvec <= 8; TP_ERR_ARG without a forward call on this handle before it */
int tp_overhang_adjoint(tp_overhang *ov, int nvec, double *const *g);
int tp_overhang_last_chunk(const tp_overhang *ov);              /* layers per launch of the last sweep */
/* copies of the coefficients the last forward call stored for the transpose, [dev, own elements] each, any of them may be
 * NULL: a, w, p of the formulas above (layer 0: a = 1, w = 0).  Read-only; TP_ERR_ARG before a forward call. */
int tp_overhang_get_coefficients(tp_overhang *ov, double *a, double *w, double *p);

/* ---- casting (draw-direction) filter (no reference counterpart) ---- */
/* A "cast" density c built from the blueprint density x line by line along the draw axis: a part that leaves a mould along that
 * axis has no undercut and no enclosed cavity, so along every line of elements c falls monotonically away from the mould's
 * base.  Axis 0 (x), 1 (y) or 2 (z) with n global element layers; the parting index p in [0, n] splits every line: the cells
 * k >= p (upper die, withdrawn towards +axis) become non-increasing in k, the cells k < p (lower die) non-decreasing.  p = 0 is
 * the one-sided draw "+axis" (the part sits on a base at the lowest index), p = n is "-axis", between them a two-sided mould
 * with a plane parting surface between the layers p - 1 and p.  Upper range, from k = n - 1 down to p (the lower range is the
 * mirror image from k = 0 up to p - 1):
 *   c_{n-1} = x_{n-1};  d = x_k - c_{k+1},  rho = sqrt(d^2 + eps),  c_k = (x_k + c_{k+1} + rho) / 2
 *   (a smooth running maximum, no clamp: with m steps behind it  hardmax <= c <= hardmax + m sqrt(eps) / 2;  default eps = 1e-6)
 * A filter, not a constraint: the responses are evaluated on c and their gradients come back through the transpose of the
 * sweep's Jacobian, which works in place on up to 8 vectors at once from one coefficient array the forward sweep left in the
 * handle.  All arrays [dev, own elements].  No line has a neighbour, so x and y draws are rank-local on z-slabs; a z draw runs
 * as a pipeline over the slabs, one after the other, and gives the results of one rank bit for bit.  The x draw has two kernel
 * forms with equal bits, chosen per call by TP_CASTING_XFORM. */
typedef struct tp_casting tp_casting;
int tp_casting_create(tp_casting **c, tp_grid *g, int axis /*0 x, 1 y, 2 z*/, int parting /*0 .. n_axis global*/);
int tp_casting_destroy(tp_casting *c);                          /* NULL: 0 */
/* TP_ERR_ARG unless eps > 0 and finite; a forward call must follow before the next transpose */
int tp_casting_set_params(tp_casting *c, double eps);
int tp_casting_forward(tp_casting *c, const double *x, double *out);   /* TP_ERR_ARG if x == out */
/* g[v] <- J^T g[v], v < nvec, 1 <= nvec <= 8; TP_ERR_ARG without a forward call on this handle before it */
int tp_casting_adjoint(tp_casting *c, int nvec, double *const *g);
int tp_casting_last_form(const tp_casting *c);                  /* 1 walk, 2 LDS-staged x, 3 strided x walk */
/* copy of q of the last forward call, [dev, own elements] (a sweep's first cell: 1).  Read-only; TP_ERR_ARG before a forward call. */
int tp_casting_get_q(tp_casting *c, double *q);

/* ---- passive regions: elements held at a fixed density (no reference counterpart) ---- */
/* Labels per own element, natural order: 0 active, 1 void, 2 solid.  The optimiser works on the active elements alone, packed in
 * ascending element order (n_active entries); the filter and the physics work on the full fields (all own elements) with the
 * passive values imposed.  The labels come from the host once; create builds the int32 index list of the active elements there
 * and uploads both.  TP_ERR_ARG for a label above 2.
 * The four per-iteration calls take host arrays of nvec [dev] pointers, 1 <= nvec <= TP_PASSIVE_MAXVEC (the objective row, the 7
 * constraint rows MMA allows, the design and spare), and handle all of them in ONE launch:
 *   impose   passive entries of every x[v] <- v_void / v_solid by label; active entries are not written
 *   zero     passive entries of every rows[v] <- +0.0 whatever they held (NaN included); active entries are not written
 *   gather   packed[v][a] = full[v][idx[a]], a < n_active
 *   scatter  full[v][idx[a]] = packed[v][a]; passive entries of full are not written
 * TP_ERR_ARG, before the handle is used, for a NULL handle, array or vector, nvec outside 1..TP_PASSIVE_MAXVEC, and for
 * full[v] == packed[w] with any v, w.  Without active elements gather and scatter, without passive ones impose and zero, return
 * TP_OK and launch nothing. */
#define TP_PASSIVE_MAXVEC 12
typedef struct tp_passive tp_passive;
int tp_passive_create(tp_passive **p, tp_grid *g, const unsigned char *label_host /* own elements, natural order */);
int tp_passive_destroy(tp_passive *p);                          /* NULL: TP_OK */
int tp_passive_counts(const tp_passive *p, long *n_active, long *n_void, long *n_solid);   /* own elements; each may be NULL */
int tp_passive_impose(tp_passive *p, int nvec, double *const *x, double v_void, double v_solid);
int tp_passive_zero(tp_passive *p, int nvec, double *const *rows);
int tp_passive_gather(tp_passive *p, int nvec, const double *const *full, double *const *packed);
int tp_passive_scatter(tp_passive *p, int nvec, const double *const *packed, double *const *full);

/* ---- design-variable linking: mirror symmetry, pattern repetition, extrusion (no reference counterpart) ---- */
/* One mode per axis (x, y, z) of the own elements, ne of them along the axis:
 *   0 none     r(i) = i                 nr = ne           preimage of I: {I}
 *   1 mirror   r(i) = min(i, ne-1-i)    nr = (ne+1)/2     {I, ne-1-I}, one member where they coincide
 *   2 repeat   r(i) = i mod (ne/cells)  nr = ne/cells     {I, I+nr, .., I+(cells-1) nr}; cells >= 2 divides ne
 *   3 extrude  r(i) = 0                 nr = 1            {0 .. ne-1}
 * The optimiser works on the reduced vector, the box nr_x x nr_y x nr_z in natural order (x fastest); the filter and the physics
 * work on the full fields.  The orbit of a reduced variable is the product of its three preimages.  cells[a] is read for mode 2 only.
 * The three per-iteration calls take host arrays of nvec [dev] pointers, 1 <= nvec <= TP_LINK_MAXVEC, and handle all of them in ONE
 * launch:
 *   expand  full[v][e] = red[v][r(e)]
 *   fold    red[v][j]  = the sum of full[v][e] over orbit(j): sequential in ascending natural element order (z outer, then y,
 *           then x), started with the first member's value, plain IEEE adds -- the same bits from every kernel form and run
 *   pick    red[v][j]  = full[v][first member of orbit(j)]
 * set_form chooses fold's kernel for this handle: 0 the measured rule, 1 one reduced variable per thread, 2 x rows staged through
 * LDS where that applies (an x mode other than none, at most 512 elements along x; form 1 otherwise); last_form reports the form
 * of the last fold (0 before the first, and for NULL).
 * TP_ERR_ARG, before the handle or the grid's stream is used, for a NULL handle, array or vector, nvec outside 1..TP_LINK_MAXVEC,
 * any source pointer equal to any destination pointer, a mode outside 0..3, repeat with fewer than 2 cells or a cell count that
 * does not divide ne, a form outside 0..2, and a z mode other than none on a grid of more than one rank (with x and y links every
 * orbit lies inside a slab: a rank's reduced vector is nr_x x nr_y x ez_own and nothing is communicated). */
#define TP_LINK_MAXVEC 12
typedef struct tp_link tp_link;
int tp_link_create(tp_link **l, tp_grid *g, const int mode[3], const int cells[3]);
int tp_link_destroy(tp_link *l);                                /* NULL: TP_OK */
int tp_link_counts(const tp_link *l, long *n_reduced_own, long nr[3]);   /* each may be NULL */
int tp_link_expand(tp_link *l, int nvec, const double *const *red, double *const *full);
int tp_link_fold(tp_link *l, int nvec, const double *const *full, double *const *red);
int tp_link_pick(tp_link *l, int nvec, const double *const *full, double *const *red);
int tp_link_set_form(tp_link *l, int form);
int tp_link_last_form(const tp_link *l);

/* ---- robust design: eroded / nominal / dilated projections of one filtered field (no reference counterpart) ---- */
/* project  out[k][i] = H(xTilde[i]; beta, eta[k]) for k < nproj in ONE launch that reads xTilde once; each field has the bits of
 *          tp_filter_project's projection at its threshold.  With p a void element receives 0.0 and a solid one 1.0 in every field
 *          (the projection followed by tp_passive_impose(.., 0, 1)).  With sums the nproj sums of the values as stored, over all
 *          ranks, are returned to the host (one read, blocking); without, nothing is reduced and the host does not wait.
 * chain    rows[r][i] *= dH/dxTilde(xTilde[i]; beta, eta_row[r]), tp_filter_gradients' projection factor; the factor is evaluated
 *          once per distinct threshold -- at most TP_ROBUST_MAXPROJ of them -- and element.  With p the passive entries of every
 *          row are stored as +0.0 whatever they held (the chain followed by tp_passive_zero).
 * TP_ERR_ARG, before the grid is used, for a NULL grid, field, array or vector, nproj outside 1..TP_ROBUST_MAXPROJ, nrows outside
 * 1..TP_ROBUST_MAXROWS, more than TP_ROBUST_MAXPROJ distinct eta_row, beta <= 0 or not finite, a threshold outside [0, 1], an
 * out[k] / rows[r] equal to xTilde or to another one, and a p of another grid. */
#define TP_ROBUST_MAXPROJ 3
#define TP_ROBUST_MAXROWS 8
int tp_robust_project(tp_grid *g, const double *xTilde, double beta, int nproj, const double *eta /* [nproj], host */,
                      double *const *out /* [nproj] dev, own elements */, const tp_passive *p /* or NULL */,
                      double *sums /* [nproj] host, or NULL */);
int tp_robust_chain(tp_grid *g, const double *xTilde, double beta, int nrows, double *const *rows /* dev */,
                    const double *eta_row /* [nrows], host */, const tp_passive *p /* or NULL */);

/* ---- MMA optimizer step on the device (MMA.cc) ------------ */
typedef struct tp_mma tp_mma;
/* MMA::MMA(n, m, x) (MMA.cc:108-190): a = 0, c = 1000, d = 0, asymptote factors 0.5 / 0.7 / 1.2.
 * n_local = own design variables of this rank, n_global = all of them; x [dev, n_local].
 * TP_ERR_ARG unless 1 <= m <= 7: the m + m^2 sums of a dual Newton step come back in one 64-value host buffer. */
int tp_mma_create(tp_mma **mma, tp_grid *g, long n_local, long n_global, int m, const double *x);
int tp_mma_destroy(tp_mma *mma);
/* SetOuterMovelimit (MMA.cc:386-405) */
int tp_mma_set_outer_movelimit(tp_mma *mma, double Xmin, double Xmax, double movlim, const double *x, double *xmin,
                               double *xmax);
/* Update (MMA.cc:499-518): x is overwritten by the new design.  gx: host array of m constraint
 * values; dgdx: host array of m DEVICE pointers.  inner_its (may be NULL): Newton steps taken. */
int tp_mma_update(tp_mma *mma, double *x, const double *dfdx, const double *gx, const double *const *dgdx,
                  const double *xmin, const double *xmax, int *inner_its);
/* DesignChange (MMA.cc:407-426): ch = max |x - xold| over all ranks, then xold <- x */
int tp_mma_design_change(tp_mma *mma, const double *x, double *xold, double *ch);
int tp_mma_get_state(const tp_mma *mma, double *lam, double *z, int *k);
/* MMA::Restart (MMA.cc:319-360): copy out the iterates/asymptotes a restart needs (device arrays, n_local each);
 * restart_set = the restart constructor (MMA.cc:22-106): continue at outer iteration k with these. */
int tp_mma_restart_get(const tp_mma *mma, double *xo1, double *xo2, double *U, double *L);
int tp_mma_restart_set(tp_mma *mma, int k, const double *xo1, const double *xo2, const double *U, const double *L);
/* The settings below take effect at the next Update and survive tp_mma_restart_set.
 * The a/c/d constructors (MMA.cc:195-242; restart :22-106): the subproblem's penalty numbers, host arrays of m
 * (NULL = keep the current values: a = 0, c = 1000, d = 0 after tp_mma_create).  d is stored; MMA.cc never reads it. */
int tp_mma_set_subproblem(tp_mma *mma, const double *a, const double *c, const double *d);
/* SetAsymptotes (MMA.cc:362-370): asymptote initialisation, decrease and increase factors */
int tp_mma_set_asymptotes(tp_mma *mma, double init, double decrease, double increase);
/* SetRobustAsymptotesType (MMA.cc:372-384; GenSub :574-589): 0 (default) or 1 (wider L/U clamps, asymptotes of a
 * variable outside [xmin, xmax] re-centred on it); any other value: type 0 and TP_ERR_ARG */
int tp_mma_set_robust_asymptotes_type(tp_mma *mma, int val);
/* ConstraintModification (MMA.h:53; GenSub :604-612): on != 0 adds p0/q0's convexifying terms to pij/qij */
int tp_mma_constraint_modification(tp_mma *mma, int on);
/* KKTresidual (MMA.cc:428-496) at the multipliers of the last Update (lam = y = z = 0 before the first one):
 * argument convention of tp_mma_update (x, dfdx, xmin, xmax [dev]; gx host array of m constraint values; dgdx host
 * array of m device pointers).  norm2 / normInf: over all ranks. */
int tp_mma_kkt_residual(tp_mma *mma, const double *x, const double *dfdx, const double *gx, const double *const *dgdx,
                        const double *xmin, const double *xmax, double *norm2, double *normInf);

/* ---- streaming helpers used by the driver (main.cc:68-73, TopOpt.cc) ----- */
int tp_vec_scale(tp_grid *g, double *x, double a, long n);
int tp_vec_set(tp_grid *g, double *x, double a, long n);
/* BLAS-1 surface behind the PETSc-named adapter (petsc_shim.h): VecAXPY/VecAXPBY, VecPointwiseMult/Divide,
 * VecDot/VecSum (n = the caller's OWNED range; the result is summed over the ranks of the grid) */
int tp_vec_axpby(tp_grid *g, double *y, double a, const double *x, double b, long n);
int tp_vec_pointwise(tp_grid *g, double *w, const double *x, const double *y, int divide, long n);
int tp_vec_dot(tp_grid *g, const double *x, const double *y /* NULL: sum of x */, long n, double *out);
/* Blocks of q <= TP_MAX_CASES vectors (host arrays of q [dev] pointers, n entries each), one pass over the data each.
 * block_gram: out_qq[i * q + j] (host) = X_i . Y_j over n local entries -- the caller passes OWNED ranges, as for tp_vec_dot --
 * summed over the ranks of the grid; every vector is read once; deterministic (with X == Y the entries (i, j) and (j, i) are
 * equal bit for bit, and two calls give the same bits).  block_combine: Z_i = sum_j Q_qq[j * q + i] Y_j over n entries (pass
 * the whole local arrays: ghost planes included, a combined field needs no refresh); no Z_i may overlap a Y_j or another Z.
 * TP_ERR_ARG, before the grid is touched, for NULL arguments or vectors, q outside 1..TP_MAX_CASES, n < 1 or an overlap. */
int tp_vec_block_gram(tp_grid *g, int q, const double *const *X, const double *const *Y, long n, double *out_qq);
int tp_vec_block_combine(tp_grid *g, int q, const double *const *Y, const double *Q_qq /*host, q*q*/, double *const *Z, long n);
/* synthetic density of SURVEY.md 8(d), indexed by GLOBAL element id */
int tp_synth_density(tp_grid *g, double *x, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* TOPOPT_AMD_H */
