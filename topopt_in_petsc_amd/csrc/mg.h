// mg.h -- CG preconditioned by a geometric-multigrid V-cycle with
// Chebyshev-Jacobi smoothing, for DOF unknowns per node (3 = elasticity,
// 1 = Helmholtz filter).  Replaces KSPSolve(KSPCG) + PCApply_MG + the level
// KSPCHEBYSHEV/PCJACOBI smoothers the reference reaches through PETSc
// (LinearElasticity.cc:617-746, PDEFilter.cc:269-417).
//
// This file declares Level<DOF> and MGSolver<DOF>: the data, then one line per member function.  The bodies are in the
// headers included at the end, by topic:
//   mg_kernels.h   free kernels and host helpers (CG updates, Lanczos kernels, tridiagonal bisections)
//   mg_op.h        op<EPI>() and the launcher of each level kind, halos in flight, apply()
//   mg_spectra.h   Chebyshev windows: Lanczos chains, their graphs, estimate_spectra()
//   mg_coarse.h    the coarsest level: exact solve, one-launch runs, give-up bookkeeping, smooth graph
//   mg_cycle.h     level storage, smoother, V-cycle, preconditioned CG
#pragma once
#include <algorithm>
#include <thread>

#include "galerkin.h"
#include "grid.h"
#include "operators.h"
#include "conduction.h"
#include "coarse_run.h"
#include "matfree_tile.h"
#include "fine_tile.h"
#include "fine_u4.h"
#include "coarse_direct.h"
#include "mg_kernels.h"

enum { LV_MATFREE = 0, LV_DIA = 1, LV_MACRO = 2 };

template <int DOF>
struct Level {
    Geom g;
    int kind;
    // matrix-free levels
    const double *KE;       // [dev] (8 DOF)^2
    const double *E;        // [dev] per stored element, or null
    const uint8_t *mask;    // [dev] per node, or null
    // stencil levels
    double *S;              // [dev] 27*DOF diagonals x (DOF*nodes)
    double *Kel;            // [dev] coarse element matrices (DOF = 3 Galerkin levels)
    double *dinv;
    double lam;             // estimate / bound of lambda_max(D^-1 A)
    double lam_min = 0.0;   // coarsest level: smallest Ritz value (coarse-solve window)
    double *b, *x, *x2, *r, *d;
    bool no_comm = false;   // replicated (global) copy of the coarsest level: no halo, no reductions over ranks
    bool use_tile = false;  // DOF == 3 matrix-free level with a box-symmetric KE: tuned kernel
    int sym_slot = -1;                // slot of the packed SymKE in constant memory
    // LV_MACRO (level 1 applied from the fine densities)
    int fex = 0, fey = 0;             // fine element counts
    // Dirichlet correction (elements containing a clamped fine node)
    const double *dK = nullptr;       // [dev] nflag x 576
    const int *flag_list = nullptr;   // [dev] flagged stored coarse elements
    const int *corr_nodes = nullptr;  // [dev] affected owned nodes
    const int *corr_adj = nullptr;    // [dev] 8 per affected node
    int ncorr_nodes = 0, nflag = 0;
    double *corr_tmp = nullptr;       // [dev] nflag x 24 element-row products
    double *corr = nullptr;           // [dev] level dofs, zero outside the affected nodes
    const uint8_t *colmask = nullptr; // [dev] per node column: OR of mask over z
    const double *wtab = nullptr;     // [dev] DOF == 1, constant coefficients: 27 x 27 stencil table (operators.h: ScalarStencilOp)
    const unsigned *nbmask = nullptr; // [dev] DOF == 1, one coefficient per element and Dirichlet rows: mask bits of a node's 27 neighbours (conduction.h: ConductionOp)
    double kt8[8] = {};               // ... and the 8 distinct entries of its element matrix
    long ndof() const { return (long)DOF * g.nodes(); }
    long own_off() const { return (long)DOF * g.plane() * g.own_lo; }
    long own_n() const { return (long)DOF * g.owned_nodes(); }
};

template <int DOF>
struct MGSolver;
// the reference's hard-coded FGMRES / GMRES / SOR configuration (refksp.h), tp_solver_opts::ksp_mode = 1
template <int DOF>
int refksp_solve(MGSolver<DOF> &mg, const double *b, double *x, int *its, double *rnorm, double *bnorm, double *hist, int hist_cap);
template <int DOF>
int refksp_precond(MGSolver<DOF> &mg, const double *r, double **z);
template <int DOF>
void refksp_free(MGSolver<DOF> &mg);

template <int DOF>
struct MGSolver {
    // =====================================================================================================
    // data
    // =====================================================================================================
    // ---- levels
    tp_grid *grid = nullptr;
    void *refksp = nullptr;  // RefKsp<DOF>: work space of the ksp_mode 1 solver
    int nlv = 0;
    // lv[0 .. nlv-1]: the levels of this rank's slab.  Several ranks: the coarse levels rep0 .. nlv-1 also exist as REPLICATED
    // global copies at lv[nlv + (l - rep0)] (no halo, no reductions over ranks: every rank runs them redundantly from one
    // all-gather of the right-hand side per visit).  rep0 = nlv - 1 (the coarsest level only) unless the slabs are thin or
    // TP_REPLICATE_FROM says otherwise (round 5: the agglomeration of the coarse levels, taken to its end).
    static constexpr int LV_SLOTS = 2 * (TP_MAX_LEVELS + 1);
    Level<DOF> lv[LV_SLOTS];
    bool replicate = false;
    int rep0 = -1;                       // first replicated level (valid if replicate)
    int rix(int l) const { return nlv + (l - rep0); }                  // slot of the replicated copy of level l >= rep0
    int base(int i) const { return i < nlv ? i : rep0 + (i - nlv); }   // level number of slot i
    bool coarsest(int i) const { return base(i) == nlv - 1; }
    bool is_rep(int i) const { return i >= nlv; }
    bool allow_replicate = false;  // set by the owner when the coarsest level is a stored stencil (elasticity)
    tp_solver_opts opt;
    // Storage of every slot's level vectors, stencil and element matrices: lv[i] holds plain views of it (Level is copied and
    // read by the kernels' argument structs).  alloc_levels allocates the vectors; the owner asks for S and Kel where its
    // level kind has them.
    struct LevelStore {
        DevBuf<double> b, x, x2, r, d, dinv, S, Kel;
    } store[LV_SLOTS];
    DevBuf<double> cg_r, cg_p, cg_w, cg_p2;
    bool ready = false;
    int last_nblocks = 0;  // workgroups (= reduction partials) of the last op<EPI_APPLY_DOT>
    // what the last op<>() launched, for the tests (tp_elasticity_last_op_form): [0] 1 fine tile kernel, 2 level 1 from the fine
    // densities, 3 per-node matrix-free, 4 stored stencil; [1] fine: generation, level 1: correction fused, per-node: 1 = the scalar
    // operator's 27-point table (ScalarStencilOp), 2 = the conduction operator from registers (ConductionOp), 0 = the gather over
    // the elements (MatfreeOp), stencil: row split;
    // [2] fine: tile 0 15 x 15 nodes, 1 16x16, 2 32x8, 3 32x16, stencil: node form; [3] fine, level 1: z-chunk, stencil: mirrored reads
    int last_form[4] = {0, 0, 0, 0};
    static constexpr int NLANCZOS_COARSE = 40;
    double fine_bound = 0.0;  // Chebyshev bound of the matrix-free fine level (setup_matfree_level: computed once)
    long topology_epoch = 0;  // bumped by the owner whenever lists/buffers referenced by the operators are rebuilt
    // cycles[l]: how often level l + 1 is cycled per visit of level l (1 = V, 2 = W: PCMGSetCycleType /
    // PCMGSetCycleTypeOnLevel).  As PCMGMCycle_Private does it: the coarser level's iterate is zeroed once, further cycles
    // run on the same right-hand side from the iterate (zero_guess = false: the pre-smoother's non-zero-guess branch);
    // one cycle only into the coarsest level.
    int cycles[TP_MAX_LEVELS + 1] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

    // ---- state of the Krylov loop (mg_cycle.h)
    const double *head_for = nullptr;  // right-hand side whose fine pre-smoothing is already enqueued (vcycle_head)
    bool fine_first_done = false;  // the CG update has written x1 = dinv b / theta of the fine level already (solve())
    int last_solve_its = -1;  // iteration count of the previous solve (-1: none yet)

    // ---- halos in flight on the second stream (one per level: the output of the last split launch; mg_op.h)
    struct PendingHalo {
        const double *ptr = nullptr;
    };
    PendingHalo pend[LV_SLOTS];
    hipEvent_t pend_ev[LV_SLOTS] = {};

    // ---- spectra (mg_spectra.h)
    // Lanczos work space per level (kept across design iterations): basis, coefficients, reduction partials, pinned
    // host copy of the coefficients; the runs of different levels are independent and may share the device
    struct LanBuf {
        DevBuf<double> V, coef, part;
        double *hc = nullptr;
        DevBuf<unsigned> ticket, mticket;  // arrival counters of the chain's in-kernel reductions (its own: the chains of the levels run side by side)
        size_t cap = 0;
        int m = 0;
    };
    LanBuf lan[LV_SLOTS];
    // the run of a level is a static chain of ~400-1000 small launches: captured once into a hipGraph and replayed
    // every design iteration (host cost: one launch); rebuilt when the captured pointers may have changed
    hipGraphExec_t lan_graph[LV_SLOTS] = {};
    const void *lan_graph_key[LV_SLOTS][5] = {};
    int lan_graph_state[LV_SLOTS] = {};  // 0: not tried, 1: valid, -1: capture failed -> direct launches
    hipStream_t lan_stream[LV_SLOTS] = {};
    hipEvent_t lan_fork = nullptr, lan_done[LV_SLOTS] = {};
    // Round 6: the owner may say when a level's operator is complete (mark_level_ready, recorded on the solver's stream in the
    // middle of the assembly); that level's spectrum chain then waits for this event instead of for the end of the whole
    // assembly -- level 1's chain needs two small kernels, not the stencils of the levels below it.  Valid for one assembly.
    hipEvent_t lv_ready[LV_SLOTS] = {};
    bool lv_ready_set[LV_SLOTS] = {};
    DevBuf<XcdRunCtrl> lan_ctl;         // [dev] control block of the one-XCD Lanczos run
    hipStream_t side_stream = nullptr;  // owner's spare stream (idle during estimate_spectra): a second one for the chains

    // ---- the coarsest level solved exactly (coarse_direct.h; mg_coarse.h): opt.coarse_direct, one rank or the replicated copy
    struct CoarseDirect {
        CdGeom g{};
        DevBuf<double> Lb, Tm, Ld, Linv, W, Wt, y;
        DevBuf<XcdRunCtrl> ctl;
        int level = -1;       // the level the factor belongs to (nlv - 1, or nlv: the replicated copy)
        bool factored = false;
    } cd;
    int cd_level() const { return replicate ? rix(nlv - 1) : nlv - 1; }
    bool cd_early = false;              // this assembly's factorisation is already under way (coarse_direct_early)
    bool cd_inverse_owed = false;       // ... and its triangular inverse is still to be enqueued behind it (estimate_spectra)
    bool cd_pending = false;            // ... and is still running on its side stream: the solver's stream waits for it (join_pending_factor)
    bool cd_deferred_last = false;  // the last assembly's factorisation ran beside the head of the solve (give-up severity)

    // ---- the coarsest level's run in one launch (coarse_run.h; mg_coarse.h)
    DevBuf<unsigned long long> run_cnt;     // [dev] arrival counter (monotone over the runs) + give-up flag
    DevBuf<XcdRunCtrl> run_ctl;             // [dev] control block of the one-XCD run (zero between runs)
    bool gaveup_seen = false;               // the last diverged solve found a give-up flag raised by a one-XCD kernel
    int gaveup_mask = 0;  // which control block raised the flag xcd_gaveup() found: 1 Chebyshev run, 2 Lanczos run, 4 factorisation
    unsigned long long run_base = 0;        // arrivals of all runs so far
    long coarse_runs = 0;

    // ---- the coarsest level's smoothing run as a replayed hipGraph (opt-in, TP_SMOOTH_GRAPH=1; mg_coarse.h)
    struct SmoothGraph {
        hipGraphExec_t exec = nullptr;
        const void *ptr[4] = {nullptr, nullptr, nullptr, nullptr};  // b, x, x2, d
        double theta = 0.0, delta = 0.0;
        int k = 0, flags = 0, level = -1;
        bool swap = false;      // the run leaves x and x2 exchanged
        double bytes = 0.0, flops = 0.0;  // accounting of one run
        long stamp = 0;
    };
    SmoothGraph sgraph[4];
    bool sg_capturing = false;
    hipStream_t sg_stream = nullptr;
    long sg_clock = 0;

    // =====================================================================================================
    // mg_op.h -- operator application
    // =====================================================================================================
    // what op<EPI>() works out once and hands to the launcher of the level's kind; the launcher leaves its accounting in it
    struct OpLaunch {
        int l = 0;                // slot of the level
        long nown = 0;            // owned nodes
        int nb = 0;               // workgroups of a thread-per-node launch
        int n_bnd = 0;            // owned planes that a neighbour slab reads (0 .. 2)
        bool out_halo = false;    // the caller reads the ghost planes of the output next
        bool split = false;       // tile levels: boundary planes first, their exchange under way, then the interior
        double bytes = 0.0, flops = 0.0;
    };
    // out = A_l x with epilogue EPI (operators.h): picks the launcher of the level's kind, counts the launch
    template <int EPI>
    int op(int l, NodeArgs a, bool out_halo = false);
    // the tile-tuned level 0: generations 3 / 2 / 1
    template <int EPI>
    int op_fine(OpLaunch &c, const NodeArgs &a);
    // level 1 applied from the fine densities, with its Dirichlet-correction launches
    template <int EPI>
    int op_macro(OpLaunch &c, const NodeArgs &a);
    // generic matrix-free level (k_node), including the DOF 1 scalar stencil
    template <int EPI>
    int op_matfree_node(OpLaunch &c, const NodeArgs &a);
    // stored-stencil level (k_dia_row, k_dia_row_split, k_dia_node3), boundary rows first on slabs
    template <int EPI>
    int op_stencil(OpLaunch &c, const NodeArgs &a);
    // output planes of pass 0 (boundary) / 1 (interior) of a split tile launch; the whole owned range if not split
    static void tile_ranges(const Level<DOF> &L, bool split, int pass, int &lo, int &hi, int &r1lo, int &r1hi);
    // behind the boundary pass: start the exchange of `out`'s ghost planes on the second stream
    int after_boundary(int l, double *out);
    // arguments of a tile launch (fine level; op_macro fills in level 1's own fields)
    static TileArgs tile_args(const Level<DOF> &L, int lo, int hi, int kz, int r1lo, int r1hi);
    // Fine tile kernel: Chebyshev in its 3-term form  u+ = u + c1 (u - u-) + c2 D^-1 (b - A u); u- sits in the output
    // buffer (read and overwritten by the same thread), so no direction vector is streamed.
    static bool three_term(const Level<DOF> &L) { return DOF == 3 && L.kind == LV_MATFREE && L.use_tile; }
    // which kernel generation serves a tuned matrix-free level (0: none)
    static int fine_generation(const Level<DOF> &L);
    static bool runs_fine_tile(const Level<DOF> &L) { return fine_generation(L) == 2; }
    // the stream waits for the halo in flight of level l / of every level (DMGlobalToLocalEnd)
    int drain_halo(int l);
    int drain_halos();
    // a node-wise kernel over whole owned planes of `out`, boundary planes first where the overlap is available
    template <class F>
    int planes_split(int l, double *out, F launch);
    // refresh the ghost planes of v (nothing to do if its exchange is already under way)
    int halo(int l, double *v);
    // y = A_l u (ghost planes of u refreshed first)
    int apply(int l, double *u, double *y);
    // y = A_0 u with the operator of the Krylov method
    int apply_krylov(double *u, double *y);

    // =====================================================================================================
    // mg_spectra.h -- Chebyshev windows
    // =====================================================================================================
    // Chebyshev windows of the stencil / coarse levels (and of the fine level if opt.fine_eig)
    int estimate_spectra(int first_level);
    // owner: level l's operator is complete (its spectrum chain may start)
    int mark_level_ready(int l);
    // sum over ranks of n device doubles
    int allreduce_dev(double *p, int n, bool local_only = false);
    // enqueue a Lanczos run of level l on grid->stream; lanczos_finish evaluates it once the stream has drained
    int lanczos_enqueue(int l, int steps);
    // the coarsest level's run as ONE launch on one XCD: may it, and do it
    bool lanczos_xcd_ok(int l, int steps) const;
    int lanczos_xcd(int l, int steps);
    // is the captured chain of level l valid for the vectors it would run on now?
    bool lanczos_graph_replayable(int l) const;
    // replay (or capture, or plain enqueue) of the run of level l on grid->stream
    int lanczos_graph(int l, int steps);
    // extreme Ritz values from the coefficients of the finished run
    void lanczos_finish(int l, double *lam_out, double *lam_min_out = nullptr);
    // enqueue, wait, finish
    int lanczos(int l, int steps, double *lam_out, double *lam_min_out = nullptr);

    // =====================================================================================================
    // mg_coarse.h -- the coarsest level
    // =====================================================================================================
    void smooth_graphs_free();
    // the smoothing run of level l from a captured graph (captured on the first use of an argument set)
    int smooth_replay(int l, const double *b, int k, bool zero_guess, bool first_done, double theta, double delta);
    // enqueue the triangular inverse that coarse_direct_early left for later
    int enqueue_owed_inverse();
    // owner: the coarsest level's stencil is enqueued -- start its factorisation on a stream of its own right away
    int coarse_direct_early(bool *started);
    // does the exact coarse solve apply to this hierarchy?
    bool coarse_direct_ok() const;
    void coarse_direct_free();
    // factor + invert on grid->stream; parts: 1 = band fill + factorisation, 2 = the triangular inverse, 3 = both
    int coarse_direct_factor(int parts = 3);
    // the solver's stream waits for a factorisation still running on its side stream
    int join_pending_factor();
    // x = A^-1 b on level cd.level
    int coarse_direct_apply(int l, const double *b);
    // did a one-XCD kernel (Chebyshev run, Lanczos run, factorisation) give up?  Blocking read of the sticky flags.
    bool xcd_gaveup();
    void xcd_reset_controls();
    // after an assembly that failed half way: no chain of a side stream may still be running when the next one starts
    void join_side_streams();
    // rows per thread of a run: the fewest that bring it down to TP_RUN_WGS / 32 workgroups
    static int run_rows_per_thread(long rows, int *wgs);
    static int xcd_rows_per_thread(long rows, int *wgs);
    // form of the coarsest level's run: 0 separate launches, 1 one workgroup, 2 several with a barrier, 3 one XCD
    int coarse_run_mode(int l, int nsteps) const;
    // the level fits a run on one XCD
    bool xcd_eligible(int l, long stage_cap, int max_r) const;
    // steps it0 .. k-1 of smooth() in one launch
    int coarse_run(int l, const double *b, int it0, int k, double sigma, double delta, int mode);

    // =====================================================================================================
    // mg_cycle.h -- storage, smoother, V-cycle, preconditioned CG
    // =====================================================================================================
    int alloc_levels();
    // the six vectors of slot i, zeroed on the grid's stream; level i's stencil (`slices` x ndof doubles, zeroed on that stream or before the call returns) and its element matrices
    int alloc_vectors(int i);
    int alloc_stencil(int i, int slices, bool on_stream);
    int alloc_elem_matrices(int i);
    // graphs, streams, events, pinned memory and the reference solver's work space (device memory dies with its DevBufs)
    void free_levels();
    ~MGSolver() { free_levels(); }
    // Jacobi diagonal + Chebyshev bound of a matrix-free level
    int setup_matfree_level(int l, const double *h_KE);
    // every rank's owned rows of `nseg` consecutive level vectors -> the replicated global arrays
    int gather_owned(Level<DOF> &L, const double *src, Level<DOF> &R, double *dst, int nseg, long src_stride = 0,
                     long dst_stride = 0);
    // (re)build the replicated coarse levels from the ranks' owned stencil rows
    int setup_replicated();
    // Chebyshev(k)-Jacobi; on exit L.x holds the iterate.  dot_slot >= 0: the LAST step also leaves b . x in scal[dot_slot]
    int smooth(int l, const double *b, int k, bool zero_guess, int dot_slot = -1, bool first_done = false);
    // Chebyshev window of level l (the coarsest level's spans its whole spectrum)
    void cheb_window(int l, double *theta, double *delta) const;
    // can the last post-smoothing step of a V-cycle return r . z ?
    bool can_fuse_rz() const;
    // the fine level's pre-smoothing of a V-cycle for right-hand side b, enqueued AHEAD of the cycle
    int vcycle_head(const double *b);
    // PCMG multiplicative V-cycle with zero initial guesses; result in lv[l].x
    int vcycle(int l, const double *b, int dot_slot = -1, bool first_done = false, bool zero_guess = true);
    // z = M r : one V-cycle.  Returns the pointer holding z (lv[0].x).
    int precond(const double *r, double **z, int dot_slot = -1);
    // KSPSolve, KSPCG with the unpreconditioned norm, reference norm ||b||
    int solve(const double *b, double *x, int *its_out, double *rnorm_out, double *bnorm_out, double *hist, int hist_cap);
};

#include "mg_op.h"
#include "mg_spectra.h"
#include "mg_coarse.h"
#include "mg_cycle.h"
