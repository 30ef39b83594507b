// switches.h -- every environment variable the product library reads, one accessor each.  No other file under csrc/
// calls getenv.  (The host side -- host/, lib.py, api.py -- reads its own process plumbing: TP_RANK, TP_SHM, TP_LIB, ...)
//
// Two classes, and a switch keeps its class:
//   * LATCHED once per process (a function-local static const): set it before the library's first use;
//   * READ ON EVERY CALL: the tests flip these inside one process.
// "set" below means present in the environment with any value, the empty string included.  DESIGN.md 6, "Run-time switches", lists them all.
#pragma once
#include <cstdlib>
#include <cstring>

// ===========================================================================
// process state that travels with the switches (not environment variables)
// ===========================================================================
// The one-XCD persistent kernels (coarse_run.h: Chebyshev run, Lanczos run; coarse_direct.h: factorisation) rely on their
// workgroups being co-resident.  When one of them gives up (its peers did not show up within ~1 s: a device shared with
// another process' persistent kernels) the library redoes the work with the launch-per-step forms and keeps the
// one-XCD forms OFF for the rest of the process (topopt_amd.hip: redo_without_xcd).
inline bool &tp_xcd_disabled() {
    static bool off = false;
    return off;
}
// Round 6: the coarse factorisation, a chain of one-XCD kernels, runs on a side stream BESIDE the head of the
// solve (mg.h: cd_pending) -- full-device kernels are queued while its later kernels start, so their co-residency is a
// little less certain than on an idle device.  A give-up of THAT chain alone first costs the deferral (the factorisation is
// joined at the end of the set-up again, round 4's behaviour), not the one-XCD forms; only a give-up without the deferral
// switches them off.  Every recovery is counted (tp_xcd_status).
inline bool &tp_defer_disabled() {
    static bool off = false;
    return off;
}
inline int &tp_giveup_count() {
    static int n = 0;
    return n;
}

// helpers of this file: is the variable set / its integer value or `dflt` / "on unless set to 0"
inline bool sw_set(const char *name) { return getenv(name) != nullptr; }
inline int sw_int(const char *name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }
inline bool sw_not_zero(const char *name) { return !(getenv(name) && atoi(getenv(name)) == 0); }

// ===========================================================================
// LATCHED ONCE PER PROCESS
// ===========================================================================
// ---- debugging

// TP_DEBUG_SYNC=1 (default off): synchronise the device after every launch, so that an asynchronous fault is reported at
// the launch that caused it; implies no graph capture, no smooth graph, no one-XCD runs, no level-2 side stream
inline bool tp_debug_sync() {
    static const bool v = getenv("TP_DEBUG_SYNC") != nullptr && atoi(getenv("TP_DEBUG_SYNC")) != 0;
    return v;
}

// ---- fine level and level 1 (mg_op.h)

// TP_FINE_V=1|2|3 (default 0 = by mesh size): generation of the fine-level kernel, 3 fine_u4.h, 2 fine_tile.h, 1 matfree_tile.h (mg_op.h: fine_generation, tools/ab3.sh)
inline int sw_fine_v() {
    static const int v = sw_int("TP_FINE_V", 0);
    return v;
}
// TP_XCD_REMAP=0 (default 1): tiles that share cache lines meet in one XCD's L2 (PMC: -30 % fetch traffic, -5 % time)
inline int sw_xcd_remap() {
    static const int v = sw_int("TP_XCD_REMAP", 1);
    return v;
}
// TP_TILE_KZ=n (default 0 = fine_kz's choice): z-chunk length of the fine tile kernels
inline int sw_tile_kz() {
    static const int v = sw_int("TP_TILE_KZ", 0);
    return v;
}
// TP_FINE_SHAPE=1|2|3 (default 0 = by mesh size): third generation's tile, 1: 16x16, 2: 32x8, 3: the 32x16 experiment (profiles/r03_fine_probe_shapes.txt)
inline int sw_fine_shape() {
    static const int v = sw_int("TP_FINE_SHAPE", 0);
    return v;
}
// TP_MACRO_KZ=n (default 0 = by level size): z-chunk length of the level-1 tile kernel
inline int sw_macro_kz() {
    static const int v = sw_int("TP_MACRO_KZ", 0);
    return v;
}
// TP_NO_CORR_FUSE set (default fused on one rank): level 1's Dirichlet correction as two launches ahead of the tiles
inline bool sw_no_corr_fuse() {
    static const bool v = sw_set("TP_NO_CORR_FUSE");
    return v;
}
// TP_NO_PDE_STENCIL set (default stencil form): the constant-coefficient scalar operator through the generic matrix-free kernel
inline bool sw_no_pde_stencil() {
    static const bool v = sw_set("TP_NO_PDE_STENCIL");
    return v;
}

// ---- stored-stencil levels (mg_op.h: op_stencil)

// TP_DIA_SPLIT=1|3|9 (default -1 = by level size): threads that share a stencil row
inline int sw_dia_split() {
    static const int v = sw_int("TP_DIA_SPLIT", -1);
    return v;
}
// TP_DIA_NODE=0 (default on): DOF 3, the row form instead of the node form k_dia_node3 (round 6: 27.9 -> 19.0 us per step on C3's level 2)
inline bool sw_dia_node() {
    static const bool v = sw_not_zero("TP_DIA_NODE");
    return v;
}
// TP_NO_DIA_SYM set (default mirrored): every coefficient read from its own row instead of the mirrored reads
inline bool sw_no_dia_sym() {
    static const bool v = sw_set("TP_NO_DIA_SYM");
    return v;
}
// TP_STENCIL_OVERLAP=0 (default on): slabs, one launch per stencil product instead of boundary rows first (round 5)
inline bool sw_stencil_overlap() {
    static const bool v = sw_not_zero("TP_STENCIL_OVERLAP");
    return v;
}

// ---- reductions

// TP_NO_REDUCE_TAIL set (default in-kernel tails): partial sums only, k_reduce_final as a second launch (common.h: reduce_tail)
inline bool sw_no_reduce_tail() {
    static const bool v = sw_set("TP_NO_REDUCE_TAIL");
    return v;
}

// ---- spectra (mg_spectra.h)

// TP_LANCZOS_SERIAL set (default side by side): the levels' Lanczos chains one after the other on the solver's stream; also no early factorisation
inline bool sw_lanczos_serial() {
    static const bool v = sw_set("TP_LANCZOS_SERIAL");
    return v;
}
// TP_LANCZOS_ONE_THREAD set (default helper threads): captured chains replayed from the calling thread (round 4: 0.6-1.3 ms of host time each)
inline bool sw_lanczos_one_thread() {
    static const bool v = sw_set("TP_LANCZOS_ONE_THREAD");
    return v;
}
// TP_LANCZOS_ON_MAIN=0|2 (default 1): with the factorisation, the chains of the levels beyond the second on the solver's stream (1), a stream each (2), the spare stream (0) (round 6)
inline int sw_lanczos_on_main() {
    static const int v = sw_int("TP_LANCZOS_ON_MAIN", 1);
    return v;
}
// TP_LANCZOS_TAILS=0 (default on; also off under TP_NO_REDUCE_TAIL): the chain's reductions as second launches (round 6: 12 -> 6 dependent launches per step on level 1)
inline bool sw_lanczos_tails() {
    static const bool v = sw_not_zero("TP_LANCZOS_TAILS") && !getenv("TP_NO_REDUCE_TAIL");
    return v;
}
// TP_NO_LEVEL_EVENTS set (default events): a level's spectrum chain waits for the whole assembly, not for its own level (round 6)
inline bool sw_no_level_events() {
    static const bool v = sw_set("TP_NO_LEVEL_EVENTS");
    return v;
}

// ---- exact coarse solve (mg_coarse.h, coarse_direct.h)

// TP_NO_DEFER_FACTOR set (default deferred): the factorisation joined at the end of the set-up, as in round 4
inline bool sw_no_defer_factor() {
    static const bool v = sw_set("TP_NO_DEFER_FACTOR");
    return v;
}
// TP_CD_SPLIT_ENQUEUE=0 (default on): the early factorisation enqueues its triangular inverse at once instead of from estimate_spectra (round 6)
inline bool sw_cd_split_enqueue() {
    static const bool v = sw_not_zero("TP_CD_SPLIT_ENQUEUE");
    return v;
}
// TP_CD_STAGES=1|2 (default 3; timing aid): stop the factorisation after 1 the fill, 2 + the factor, 3 all
inline int sw_cd_stages() {
    static const int v = sw_int("TP_CD_STAGES", 3);
    return v;
}
// TP_CD_PROF set (default off; timing aid): ticks per phase, printed per factorisation
inline bool sw_cd_prof() {
    static const bool v = sw_set("TP_CD_PROF");
    return v;
}
// TP_CD_INVERT_COLUMNS set (default divide and conquer): round 3's block-column substitution for the triangular inverse
inline bool sw_cd_invert_columns() {
    static const bool v = sw_set("TP_CD_INVERT_COLUMNS");
    return v;
}
// TP_RUN_WGS=n (default 16; timing aid): workgroups the multi-workgroup coarse run aims for
inline int sw_run_wgs() {
    static const int v = sw_int("TP_RUN_WGS", 16);
    return v;
}

// ---- multigrid cycle and Krylov loop (mg_cycle.h)

// TP_NO_REPLICATE set (default replicated): several ranks, no replicated copies of the coarse levels
inline bool sw_no_replicate() {
    static const bool v = sw_set("TP_NO_REPLICATE");
    return v;
}
// TP_REPLICATE_FROM=l (default -1 = by slab thickness; an empty string counts as unset): first replicated level, 2 .. nlv - 1; 0 keeps the coarsest only (round 5)
inline int sw_replicate_from() {
    static const int v = (getenv("TP_REPLICATE_FROM") && *getenv("TP_REPLICATE_FROM")) ? atoi(getenv("TP_REPLICATE_FROM")) : -1;
    return v;
}
// TP_NO_FUSE_RZ set (default fused): r . z by a dot product of its own instead of the V-cycle's last smoothing step
inline bool sw_no_fuse_rz() {
    static const bool v = sw_set("TP_NO_FUSE_RZ");
    return v;
}
// TP_NO_FUSE_FIRST set (default fused): the restriction does not take the coarse level's first Chebyshev step
inline bool sw_no_fuse_first() {
    static const bool v = sw_set("TP_NO_FUSE_FIRST");
    return v;
}
// TP_NO_SPEC_HEAD set (default on): the next V-cycle's fine pre-smoothing is not enqueued ahead of the host's wait
inline bool sw_no_spec_head() {
    static const bool v = sw_set("TP_NO_SPEC_HEAD");
    return v;
}
// TP_NO_CG_FUSE set (default fused): p update outside the product, ||r||^2 read back through the stream
inline bool sw_no_cg_fuse() {
    static const bool v = sw_set("TP_NO_CG_FUSE");
    return v;
}
// TP_CG_NT=0 (default on): plain instead of non-temporal loads / stores in the CG update (round 5: 12.50 -> 12.40 ms at 128^3)
inline bool sw_cg_nt() {
    static const bool v = sw_not_zero("TP_CG_NT");
    return v;
}

// ---- operator set-up (topopt_amd.hip)

// TP_NO_L2_FAST set (default fast): level 2's element matrices through the generic contraction
inline bool sw_no_l2_fast() {
    static const bool v = sw_set("TP_NO_L2_FAST");
    return v;
}
// TP_NO_L2_ASIDE set (default side stream; also off under TP_NO_L2_FAST and TP_DEBUG_SYNC): level 2's element matrices on the solver's stream
inline bool sw_no_l2_aside() {
    static const bool v = sw_set("TP_NO_L2_ASIDE") || sw_no_l2_fast() || tp_debug_sync();
    return v;
}
// TP_NO_SETUP_REORDER set (default two passes): the set-up level by level, not the factorisation's chain first (round 3)
inline bool sw_no_setup_reorder() {
    static const bool v = sw_set("TP_NO_SETUP_REORDER");
    return v;
}
// TP_L2_BLOCKS=n (default 512): workgroups per component of k_galerkin_l2_fast
inline long sw_l2_blocks() {
    static const long v = getenv("TP_L2_BLOCKS") ? atol(getenv("TP_L2_BLOCKS")) : 512;
    return v;
}

// ---- density filter (filter.h)

// TP_NO_FILTER_TILE set (default tiled): the filter's generic kernels
inline bool sw_no_filter_tile() {
    static const bool v = sw_set("TP_NO_FILTER_TILE");
    return v;
}
// TP_FILTER_ZMULTI=n (default -1 = by mesh size): output planes per thread of the tiled filter
inline int sw_filter_zmulti() {
    static const int v = sw_int("TP_FILTER_ZMULTI", -1);
    return v;
}

// ===========================================================================
// READ ON EVERY CALL (the tests switch these within one process)
// ===========================================================================

// TP_TEST_FORCE_GIVEUP="<mode>" or "<mode>:<rank>" (test switch): does it ask rank `rank` for recovery branch `mode`?
// rank < 0: does it ask ANY rank (the collective agreement must then be reached by all of them)
inline bool tp_test_force_giveup(int mode, int rank) {
    const char *e = getenv("TP_TEST_FORCE_GIVEUP");
    if (!e || atoi(e) != mode) return false;
    const char *c = strchr(e, ':');
    return rank < 0 || !c || atoi(c + 1) == rank;
}
// TP_OVERLAP=0 (default on; read when a grid is created): every halo on the grid's stream, before its consumer
inline bool sw_overlap() { return sw_not_zero("TP_OVERLAP"); }
// TP_NO_TILE set (default tuned; read per assembly): no packed symmetric KE, hence the generic fine-level kernel
inline bool sw_no_tile() { return sw_set("TP_NO_TILE"); }
// TP_NO_MACRO set (default on; read per assembly): level 1 as a stored stencil instead of applied from the fine densities
inline bool sw_no_macro() { return sw_set("TP_NO_MACRO"); }
// TP_NO_COND_STENCIL set (default register form; read per launch): the conduction operator's fine level through the generic
// gather MatfreeOp<1> instead of ConductionOp (conduction.h); the same bits either way
inline bool sw_no_cond_stencil() { return sw_set("TP_NO_COND_STENCIL"); }
// TP_SMOOTH_GRAPH=1 (default off, and off under TP_DEBUG_SYNC): the coarsest level's smoothing run as a replayed hipGraph (measured 0.3 % SLOWER at 128^3, mg_coarse.h)
inline bool sw_smooth_graph() {
    const char *e = getenv("TP_SMOOTH_GRAPH");
    return e && atoi(e) != 0 && !tp_debug_sync();
}
// TP_DEBUG_GRAPH set (default off; timing aid): hit / miss / capture lines of the smooth graph on stderr
inline bool sw_debug_graph() { return sw_set("TP_DEBUG_GRAPH"); }
// TP_NO_COARSE_DIRECT set (default per tp_solver_opts::coarse_direct): no factorisation of the coarsest level
inline bool sw_no_coarse_direct() { return sw_set("TP_NO_COARSE_DIRECT"); }
// TP_NO_COARSE_RUN set (default on): the coarsest level's Chebyshev steps as separate launches (no run kernel of any form)
inline bool sw_no_coarse_run() { return sw_set("TP_NO_COARSE_RUN"); }
// TP_COARSE_RUN=1 (default off): the multi-workgroup run with a barrier per step (19.7 against 19.6 ms at 128^3, tools/probe/step_probe.hip)
inline bool sw_coarse_run() {
    const char *sw = getenv("TP_COARSE_RUN");
    return sw && atoi(sw) == 1;
}
// TP_NO_COARSE_XCD set (default on): no Chebyshev run on one XCD (coarse_run.h: 2.3 us per step against 3-4 per launch)
inline bool sw_no_coarse_xcd() { return sw_set("TP_NO_COARSE_XCD"); }
// TP_NO_LANCZOS_XCD set (default on): the coarsest level's Lanczos run as a chain of launches, not one launch on one XCD
inline bool sw_no_lanczos_xcd() { return sw_set("TP_NO_LANCZOS_XCD"); }
// TP_OVERHANG_CHUNK=1|2|4|8 (default 4, the fastest measured; any other value counts as unset): layers per launch of the overhang filter's two sweeps
// (overhang.h); every value gives the same bits, tp_overhang_last_chunk reports what ran
inline int sw_overhang_chunk() {
    const int c = sw_int("TP_OVERHANG_CHUNK", 4);
    return (c == 1 || c == 2 || c == 4 || c == 8) ? c : 4;
}
// TP_CASTING_XFORM=0|1 (default 1; any other value counts as unset): form of the casting filter's x draw (casting.h), 1 the
// LDS-staged kernels, 0 the walk kernels on x lines; both give the same bits, tp_casting_last_form reports what ran (2 or 3)
inline bool sw_casting_xform() {
    const int v = sw_int("TP_CASTING_XFORM", 1);
    return v != 0;
}
// TP_NO_GRAPH set (default graphs): the Lanczos chains are enqueued, not captured and replayed.  Read per call by
// lanczos_graph_replayable; lanczos_graph latches it on its first run (mg_spectra.h), as before.
inline bool sw_no_graph() { return sw_set("TP_NO_GRAPH"); }
