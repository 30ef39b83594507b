// mg_op.h -- MGSolver: applying a level's operator.  op<EPI>() picks the launcher of the level's kind (op_fine,
// op_macro, op_matfree_node, op_stencil); around it the halos in flight, the plane-split launches and the plain
// products built on it.  Included by mg.h after the declaration of MGSolver.
#pragma once

// z-chunk length of the fine tile kernels.  The chip holds 768 workgroups of them at once (3 per CU: 168 VGPRs,
// 49 KB LDS).  A grid that fills those slots ONCE with equal chunks has no second, partly empty round and the least
// redundant z-halo (measured, DESIGN.md 4.1: 128^3 kz 15 -> 729 workgroups beats kz 8 -> 1377 by 10 %; 128x64x64
// kz 4 -> 765 beats kz 8 by 20 %); that only pays while the chunks stay short enough to fill >= 90 % of the slots,
// otherwise several rounds of kz ~ 8..32 are better (256x128x128: kz 8 beats kz 33).
inline int fine_kz(int planes, int tiles, int fine_v, int SLOTS = 768) {
    if (fine_v >= 2 || fine_v == 0) {
        const int tz1 = SLOTS / tiles;
        if (tz1 >= 1) {
            const int kz1 = (planes + tz1 - 1) / tz1;
            const int n1 = tiles * ((planes + kz1 - 1) / kz1);
            if (kz1 >= 3 && kz1 <= 20 && 10 * n1 >= 9 * SLOTS) return kz1;
        }
    }
    int kz = (int)((long)planes * tiles / 5120);  // ~5k workgroups
    kz = kz < 8 ? 8 : (kz > 32 ? 32 : kz);
    // small grids: shorter chunks until the workgroup slots of the chip are filled once
    if ((long)tiles * ((planes + 7) / 8) < SLOTS) kz = (int)((long)planes * tiles / SLOTS);
    const int kmin = (long)tiles * ((planes + 3) / 4) < 256 ? 2 : 4;  // 64x32x32 elements: kz 2 beats 4 by 5 % of the step
    if (kz < kmin) kz = kmin;
    return kz > planes ? planes : kz;
}

// Which kernel generation serves a tuned matrix-free level?  ONE place decides, op<>() launches what it says and solve()
// asks it before it hands the fused p update to the product (only k_fine_tile takes NodeArgs::pz / pnew: ADVICE r4).
// 3: fine_u4.h (its 32-bit window arithmetic needs every vector of the level below 2 GB), 2: fine_tile.h, 1: matfree_tile.h
// TP_FINE_V (switches.h) forces one; 0 (default) = by mesh size: the third generation from 160 tiles of 32 x 8 per z-chunk
// on (256x128x128 and larger), the second below -- measured through the library on the BASELINE meshes (tools/ab3.sh):
// 256^3 319 / 411 us against 334 / 471 (product / Chebyshev step), 256x128x128 79 / 127 against 82 / 130, 128^3 41 / 65
// against 41 / 60, 128x64x64 17.8 / 22.5 against 16.7 / 21.7.  On the small meshes one round of workgroups covers the mesh
// and the launch lasts as long as its slowest workgroup -- a tile with a Dirichlet condition, which the third generation
// serves ~25 % slower than a free one.
template <int DOF>
int MGSolver<DOF>::fine_generation(const Level<DOF> &L) {
    if (!(DOF == 3 && L.kind == LV_MATFREE && L.use_tile)) return 0;
    const int fine_v = sw_fine_v();
    const int t32 = ((L.g.nx + 30) / 31) * ((L.g.ny + 6) / 7);   // 32 x 8 tiles per z-chunk
    if ((fine_v >= 3 || (fine_v == 0 && t32 >= 160)) && 24.0 * L.g.nodes() < 2.0e9) return 3;
    return (fine_v >= 2 || fine_v == 0) ? 2 : 1;
}

// ---- operator application with one of the epilogues -------------------
// out_halo: the ghost planes of a.out will be read next (another operator application, a grid transfer).  On the
// tile levels the slab's boundary planes are then produced FIRST, their exchange starts on the second stream and
// overlaps with the interior planes (halo() of the consumer waits for it); everywhere else out_halo is ignored
// and the consumer's halo() exchanges as before.  Per-node arithmetic does not depend on the split: bitwise the
// same result.
template <int DOF>
template <int EPI>
int MGSolver<DOF>::op(int l, NodeArgs a, bool out_halo) {
    Level<DOF> &L = lv[l];
    OpLaunch c;
    c.l = l;
    c.out_halo = out_halo;
    c.nown = L.g.owned_nodes();
    c.nb = (int)((c.nown + BLK - 1) / BLK);
    last_nblocks = c.nb;
    if (pend[l].ptr && (pend[l].ptr == a.out || pend[l].ptr != a.x)) TP_TRY(drain_halo(l));  // stale / about to be overwritten
    c.n_bnd = (L.g.has_lo ? 1 : 0) + (L.g.has_hi ? 1 : 0);
    const bool tile_level = DOF == 3 && ((L.kind == LV_MATFREE && L.use_tile) || L.kind == LV_MACRO);
    c.split = out_halo && tile_level && EPI != EPI_APPLY_DOT && EPI != EPI_CHEB_DOT && !L.no_comm && c.n_bnd > 0 &&
              halo_can_overlap(grid) && (L.g.own_hi - L.g.own_lo + 1) > c.n_bnd;
    if (DOF == 3 && L.kind == LV_MATFREE && L.use_tile) {
        TP_TRY(op_fine<EPI>(c, a));
    } else if constexpr (EPI == EPI_CHEB_DOT) {
        return TP_ERR_STATE;  // only the fine tile kernel carries the fused b . x_out
    } else if (DOF == 3 && L.kind == LV_MACRO) {
        TP_TRY(op_macro<EPI>(c, a));
    } else if (L.kind == LV_MATFREE) {
        TP_TRY(op_matfree_node<EPI>(c, a));
    } else {
        TP_TRY(op_stencil<EPI>(c, a));
    }
    double bytes = c.bytes;
    if (EPI == EPI_RESID) bytes += 8.0 * DOF * c.nown;
    // d (r/w), b, dinv -- the fine tile kernel instead reads b and the previous iterate (3-term form, diagonal on the fly)
    // (3-term form: the first step of a sweep -- c1 = 0 or the zero guess -- does not read a previous iterate)
    if (EPI == EPI_CHEB || EPI == EPI_CHEB_DOT) bytes += (three_term(L) ? ((a.c1 != 0.0 && !a.prev_zero) ? 2.0 : 1.0) : 4.0) * 8.0 * DOF * c.nown;
    if (grid->kt_on && l == 0 && (EPI == EPI_CHEB || EPI == EPI_CHEB_DOT) && !c.split && !sg_capturing) grid->kt_bytes += bytes;
    count_launch(grid, bytes, c.flops);
    if (c.split) grid->launches++;
    return TP_OK;
}

// the two passes of a split tile launch: boundary planes (one or two single-plane ranges), then the interior
template <int DOF>
void MGSolver<DOF>::tile_ranges(const Level<DOF> &L, bool split, int pass, int &lo, int &hi, int &r1lo, int &r1hi) {
    lo = L.g.own_lo, hi = L.g.own_hi, r1lo = 0, r1hi = -1;
    if (!split) return;
    if (pass == 0) {
        if (L.g.has_lo && L.g.has_hi) lo = hi = L.g.own_lo, r1lo = r1hi = L.g.own_hi;
        else if (L.g.has_lo) hi = lo;
        else lo = hi;
    } else {
        lo += L.g.has_lo ? 1 : 0;
        hi -= L.g.has_hi ? 1 : 0;
    }
}
// behind the boundary pass of a split launch: DMGlobalToLocalBegin on the output
template <int DOF>
int MGSolver<DOF>::after_boundary(int l, double *out) {
    if (!pend_ev[l]) TP_HIP(hipEventCreateWithFlags(&pend_ev[l], hipEventDisableTiming));
    const int rc = halo_nodes_begin(grid, lv[l].g, out, DOF, pend_ev[l]);
    if (rc == TP_OK) pend[l].ptr = out;
    return rc == 2 ? TP_OK : rc;  // 2: no in-place exchange after all -> the consumer's halo() does it
}
// arguments of a tile launch over the output planes [lo, hi] (and [r1lo, r1hi]) in chunks of kz: the fine level's; level 1
// (op_macro) fills its own fields in afterwards
template <int DOF>
TileArgs MGSolver<DOF>::tile_args(const Level<DOF> &L, int lo, int hi, int kz, int r1lo, int r1hi) {
    return TileArgs{L.g.nx, L.g.ny, L.g.nzl, L.g.ex, L.g.ey, L.g.ezl, lo, hi, kz,
                    L.E, L.mask, L.colmask, L.sym_slot * SYMKE_STRIDE, 0, 0, nullptr, sw_xcd_remap(), 0, r1lo, r1hi,
                    0, nullptr, nullptr, 0, nullptr};
}

// The tile-tuned fine level: generation 3 (fine_u4.h), 2 (fine_tile.h: k_fine_tile) or 1 (matfree_tile.h: k_matfree_tile), as
// fine_generation() says.  The generations share the pass loop, the timer marks and the accounting; they differ in the
// chunk length, the grid and the kernel.
template <int DOF>
template <int EPI>
int MGSolver<DOF>::op_fine(OpLaunch &c, const NodeArgs &a) {
    Level<DOF> &L = lv[c.l];
    constexpr bool IS_CHEB = (EPI == EPI_CHEB || EPI == EPI_CHEB_DOT);
    const int tx = (L.g.nx + TOUT - 1) / TOUT, ty = (L.g.ny + TOUT - 1) / TOUT;
    const int planes = L.g.own_hi - L.g.own_lo + 1;
    const int kz_env = sw_tile_kz(), fine_v = sw_fine_v();
    const int gen = fine_generation(L);
    if (a.pz && gen != 2) return TP_ERR_STATE;  // the fused p update exists in k_fine_tile only: never run it on a kernel that ignores it
    // third generation: tile shape by mesh size -- measured on the BASELINE meshes (profiles/r03_fine_probe_shapes.txt): the long
    // rows of 32 x 8 win once a chunk of them fills the chip (256^3, 512x256x256; Chebyshev from 256x128x128)
    const int shape_env = sw_fine_shape();                       // 1: 16x16, 2: 32x8
    const int t32 = ((L.g.nx + 30) / 31) * ((L.g.ny + 6) / 7);   // 32 x 8 tiles per z-chunk
    const bool wide = gen == 3 && (shape_env ? shape_env >= 2 : t32 >= (IS_CHEB ? 160 : 256));
    // generations 2 and 1: one chunk length for all passes
    int kz21 = kz_env > 0 ? kz_env : fine_kz(planes, tx * ty, fine_v);
    if (kz21 > planes) kz21 = planes;
    const bool timed = grid->kt_on && IS_CHEB && !c.split && !sg_capturing;
    if (timed) kernel_timer_mark(grid);
    for (int pass = 0; pass < (c.split ? 2 : 1); pass++) {
        int lo, hi, r1lo, r1hi;
        tile_ranges(L, c.split, pass, lo, hi, r1lo, r1hi);
        int kz = kz21;
        if (gen == 3) {  // by the planes of the pass
            const int pl = hi - lo + 1;
            if (wide) {
                const int nch = kz_env > 0 ? (pl + kz_env - 1) / kz_env : (pl + 42) / 43;  // chunks of <= 43 planes, balanced
                kz = (pl + nch - 1) / nch;
            } else {
                kz = kz_env > 0 ? kz_env : fine_kz(pl > 0 ? pl : 1, tx * ty, fine_v, IS_CHEB ? 512 : 768);
                if (kz > pl && pl > 0) kz = pl;
            }
        }
        const int tz = (hi - lo + kz) / kz + (r1hi - r1lo + kz) / kz;
        const TileArgs ta = tile_args(L, lo, hi, kz, r1lo, r1hi);
        dim3 gdim(tx, ty, tz);
        if (wide) gdim = shape_env == 3 ? dim3((L.g.nx + 30) / 31, (L.g.ny + 14) / 15, tz) : dim3((L.g.nx + 30) / 31, (L.g.ny + 6) / 7, tz);
        last_nblocks = gdim.x * gdim.y * gdim.z;
        if (wide && shape_env == 3) {  // experiment: 32 x 16 threads (31 x 15 nodes out: 1.10 instead of 1.18 x the bytes), one workgroup of 8 waves per CU
            TP_LAUNCH((k_fine_u4<EPI, 32, 16, 1, true>), gdim, dim3(512), 0, grid->stream, ta, a);
        } else if (wide) {
            TP_LAUNCH((k_fine_u4<EPI, 32, 8, 2, true>), gdim, dim3(256), 0, grid->stream, ta, a);
        } else if (gen == 3) {
            TP_LAUNCH((k_fine_u4<EPI, 16, 16, IS_CHEB ? 2 : 3, true>), gdim, dim3(256), 0, grid->stream, ta, a);
        } else if (gen == 2) {
            TP_LAUNCH((k_fine_tile<EPI>), gdim, dim3(TILE * TILE), 0, grid->stream, ta, a);
        } else {
            if constexpr (EPI == EPI_CHEB_DOT) return TP_ERR_STATE;
            else TP_LAUNCH((k_matfree_tile<EPI, 0>), gdim, dim3(TILE * TILE), 0, grid->stream, ta, a);
        }
        if (c.split && pass == 0) TP_TRY(after_boundary(c.l, a.out));
        last_form[0] = 1, last_form[1] = gen, last_form[2] = wide ? (shape_env == 3 ? 3 : 2) : (gen == 3 ? 1 : 0), last_form[3] = kz;
    }
    if (timed) kernel_timer_mark(grid);
    c.bytes = 16.0 * DOF * c.nown + 8.0 * L.g.own_elems();
    c.flops = 2.0 * 576 * (double)L.g.own_elems();
    return TP_OK;
}

// Level 1 applied from the fine densities (k_matfree_tile<., 1>), with the launches of its Dirichlet correction
template <int DOF>
template <int EPI>
int MGSolver<DOF>::op_macro(OpLaunch &c, const NodeArgs &a) {
    Level<DOF> &L = lv[c.l];
    const int tx = (L.g.nx + TOUT - 1) / TOUT, ty = (L.g.ny + TOUT - 1) / TOUT;
    const int planes = L.g.own_hi - L.g.own_lo + 1;
    const int kz_env = sw_macro_kz();
    int kz = kz_env > 0 ? kz_env : (int)((long)planes * tx * ty / 768);
    if (kz_env <= 0) {
        // small levels: chunks short enough for about one workgroup per CU (64^3..192x64x64 elements: kz 1-2
        // instead of 4 is 3-9 % of the whole design iteration), never longer than 4 below one round of slots
        int kmin = (int)(((long)planes * tx * ty + 128) / 256);
        kmin = kmin < 1 ? 1 : (kmin > 4 ? 4 : kmin);
        kz = kz < kmin ? kmin : (kz > 64 ? 64 : kz);
    }
    if (kz > planes) kz = planes;
    // Dirichlet correction of the level-1 operator.  One launch computes tiles AND element-row products
    // (extra workgroups behind the tiles), a second one adds the gathered products to the result.  Slab runs keep
    // the older order (products first, added by the tiles): the boundary planes of a boundary-first launch
    // leave for the neighbour right after the first pass and must be final by then.
    const bool fuse_corr = L.ncorr_nodes && !grid->has_comm && !sw_no_corr_fuse() && EPI != EPI_APPLY_DOT;  // slabs: one order for both halo modes
    if (L.ncorr_nodes && !fuse_corr) {
        TP_LAUNCH(k_macro_corr_rows, dim3((L.nflag * 24 + BLK - 1) / BLK), dim3(BLK), 0, grid->stream, L.g,
                           L.dK, L.flag_list, L.nflag, a.x, L.corr_tmp);
        TP_LAUNCH(k_macro_corr_gather, dim3((L.ncorr_nodes + BLK - 1) / BLK), dim3(BLK), 0, grid->stream,
                           L.corr_nodes, L.corr_adj, L.ncorr_nodes, L.corr_tmp, L.corr, L.nflag);
        count_launch(grid);
        count_launch(grid);
    }
    for (int pass = 0; pass < (c.split ? 2 : 1); pass++) {
        int lo, hi, r1lo, r1hi;
        tile_ranges(L, c.split, pass, lo, hi, r1lo, r1hi);
        int tz = (hi - lo + kz) / kz + (r1hi - r1lo + kz) / kz;
        const int ntiles = tx * ty * tz;
        last_nblocks = ntiles;
        if (fuse_corr) tz += ((L.nflag * 24 + BLK - 1) / BLK + tx * ty - 1) / (tx * ty);  // row-product workgroups
        TileArgs ta = tile_args(L, lo, hi, kz, r1lo, r1hi);
        ta.mask = nullptr, ta.colmask = nullptr;
        ta.fex = L.fex, ta.fey = L.fey;
        ta.corr = (L.ncorr_nodes && !fuse_corr) ? L.corr : nullptr;
        ta.macg_off = L.sym_slot * MACG_STRIDE;
        ta.ntiles = ntiles, ta.cr_dK = L.dK, ta.cr_list = L.flag_list, ta.cr_nflag = L.nflag, ta.cr_tmp = L.corr_tmp;
        TP_LAUNCH((k_matfree_tile<EPI, 1>), dim3(tx, ty, tz), dim3(TILE * TILE), 0, grid->stream, ta, a);
        if (c.split && pass == 0) TP_TRY(after_boundary(c.l, a.out));
    }
    last_form[0] = 2, last_form[1] = fuse_corr ? 1 : 0, last_form[2] = 0, last_form[3] = kz;
    if (fuse_corr) {
        if constexpr (EPI != EPI_APPLY_DOT) {
            TP_LAUNCH((k_macro_corr_apply<EPI>), dim3((L.ncorr_nodes + BLK - 1) / BLK), dim3(BLK), 0, grid->stream,
                      L.corr_nodes, L.corr_adj, L.ncorr_nodes, L.corr_tmp, L.nflag, a);
        }
        count_launch(grid);
    }
    c.bytes = 16.0 * DOF * c.nown + 8.0 * 8.0 * L.g.own_elems();
    c.flops = 2.0 * 576 * 8.0 * (double)L.g.own_elems();
    return TP_OK;
}

// A matrix-free level without a tuned kernel: a thread per node (k_node); the constant-coefficient scalar operator of
// DOF 1 in its 27-point stencil form, the variable-coefficient one (conduction) from registers
template <int DOF>
template <int EPI>
int MGSolver<DOF>::op_matfree_node(OpLaunch &c, const NodeArgs &a) {
    Level<DOF> &L = lv[c.l];
    bool as_stencil = false, cond_form = false;
    if constexpr (DOF == 1) {
        if (L.wtab && !L.E && !L.mask && !sw_no_pde_stencil()) {   // constant-coefficient scalar operator: its 27-point stencil form
            ScalarStencilOp so{L.wtab, L.g};
            TP_LAUNCH((k_node<1, ScalarStencilOp, EPI>), dim3(c.nb), dim3(BLK), 0, grid->stream, so, a);
            c.bytes = 16.0 * c.nown;
            c.flops = 2.0 * 27 * (double)c.nown;
            as_stencil = true;
        } else if (L.nbmask && L.E && !sw_no_cond_stencil()) {   // one coefficient per element, Dirichlet rows: 27 values + 8 coefficients from registers
            ConductionOp co{L.E, L.nbmask, {}, L.g};
            for (int q = 0; q < 8; q++) co.v[q] = L.kt8[q];
            TP_LAUNCH((k_node<1, ConductionOp, EPI>), dim3(c.nb), dim3(BLK), 0, grid->stream, co, a);
            c.bytes = 16.0 * c.nown + 8.0 * L.g.own_elems();
            c.flops = 2.0 * 72 * (double)c.nown;
            as_stencil = true;
            cond_form = true;
        }
    }
    if (!as_stencil) {
        MatfreeOp<DOF> o{L.KE, L.E, L.mask, L.g};
        TP_LAUNCH((k_node<DOF, MatfreeOp<DOF>, EPI>), dim3(c.nb), dim3(BLK), 0, grid->stream, o, a);
        c.bytes = 16.0 * DOF * c.nown + (L.E ? 8.0 * L.g.own_elems() : 0.0);
        c.flops = 2.0 * (8 * DOF) * (8 * DOF) * (double)L.g.own_elems();
    }
    last_form[0] = 3, last_form[1] = cond_form ? 2 : (as_stencil ? 1 : 0), last_form[2] = last_form[3] = 0;
    return TP_OK;
}

// A stored-stencil level: k_dia_row, k_dia_row_split or k_dia_node3 by the size of the level; on slabs the rows of the
// boundary planes first
template <int DOF>
template <int EPI>
int MGSolver<DOF>::op_stencil(OpLaunch &c, const NodeArgs &a) {
    Level<DOF> &L = lv[c.l];
    DiaOp<DOF> o{L.S, L.ndof(), L.g};
    const long rows_all = c.nown * DOF;
    // the row split (how many threads share a row) follows the size of the LEVEL, not of the launch: the boundary-first
    // launches below must sum every row in the order the single launch would
    const int nbr_all = (int)((rows_all + BLK - 1) / BLK);
    const int split_env = sw_dia_split();
    // DOF 3, round 6: the node form (k_dia_node3: a wave per z-offset, mirrored reads) serves EVERY level beyond the 9-way
    // class.  Measured per Chebyshev step against the unsplit row form the large levels used to run: C3's level 2 (70 785
    // nodes) 27.9 -> 19.0 us, the 256^3 class's (274 625) 121.5 -> 73.2, C5's (545 025) 231.7 -> 158.2 -- the mirrored reads
    // halve the coefficient stream out of HBM (the second use comes from the L2 / Infinity Cache); an unsplit node form
    // (one thread over all 27 neighbours) measured 209 / 387 us: too many registers per thread to keep the stream busy.
    const bool by_node = sw_dia_node();
    const int rsplit = split_env >= 0 ? split_env : (nbr_all < 128 ? 9 : ((DOF == 3 && by_node) ? 3 : (nbr_all < 512 ? 3 : 1)));
    // (the mirrored reads come with a row-sum correction that exists for DOF 3 only: a scalar stencil level reads its own rows)
    const bool sym = DOF == 3 && !sw_no_dia_sym();
    auto launch_rows = [&](long t0, long tn, long t1, long tn1) -> int {
        o.t0 = t0, o.tn = tn, o.t1 = t1, o.tn1 = tn1;
        const long rows = tn < 0 ? rows_all : tn + tn1;
        int nbr = 0;
        if (rsplit == 9) {
            nbr = (int)((rows + BLK / 9 - 1) / (BLK / 9));
            TP_LAUNCH((k_dia_row_split<DOF, EPI, 9>), dim3(nbr), dim3(BLK), 0, grid->stream, o, a);
            last_form[0] = 4, last_form[1] = 9, last_form[2] = 0, last_form[3] = 0;
        } else if (rsplit == 3) {
            // round 6: a thread per node and z-offset (k_dia_node3: the same bits, a third of the waves); TP_DIA_NODE=0: per row
            bool done = false;
            if constexpr (DOF == 3) {
                if (by_node && EPI != EPI_APPLY_DOT) {
                    nbr = (int)((rows / 3 + 63) / 64);
                    if (sym) {
                        TP_LAUNCH((k_dia_node3<EPI, true>), dim3(nbr), dim3(192), 0, grid->stream, o, a);
                        last_form[0] = 4, last_form[1] = 3, last_form[2] = 1, last_form[3] = 1;
                    } else {
                        TP_LAUNCH((k_dia_node3<EPI, false>), dim3(nbr), dim3(192), 0, grid->stream, o, a);
                        last_form[0] = 4, last_form[1] = 3, last_form[2] = 1, last_form[3] = 0;
                    }
                    done = true;
                }
            }
            if (!done) {
                nbr = (int)((rows + BLK / 3 - 1) / (BLK / 3));
                if (sym) {
                    TP_LAUNCH((k_dia_row_split<DOF, EPI, 3, true>), dim3(nbr), dim3(BLK), 0, grid->stream, o, a);
                    last_form[0] = 4, last_form[1] = 3, last_form[2] = 0, last_form[3] = 1;
                } else {
                    TP_LAUNCH((k_dia_row_split<DOF, EPI, 3>), dim3(nbr), dim3(BLK), 0, grid->stream, o, a);
                    last_form[0] = 4, last_form[1] = 3, last_form[2] = 0, last_form[3] = 0;
                }
            }
        } else {
            nbr = (int)((rows + BLK - 1) / BLK);
            TP_LAUNCH((k_dia_row<DOF, EPI>), dim3(nbr), dim3(BLK), 0, grid->stream, o, a);
            last_form[0] = 4, last_form[1] = 1, last_form[2] = 0, last_form[3] = 0;
        }
        last_nblocks = nbr;
        return TP_OK;
    };
    // Halo overlap on the stencil levels (round 5; slabs): the rows of the one or two boundary planes in ONE launch
    // first, their exchange on the second stream, then the interior rows -- as on the tile levels, bitwise the same
    // result (a row's sum does not depend on the launch it is computed in).  TP_STENCIL_OVERLAP=0: one launch, the
    // consumer's halo() exchanges.
    const int planes = L.g.own_hi - L.g.own_lo + 1;
    const bool split_dia = sw_stencil_overlap() && c.out_halo && EPI != EPI_APPLY_DOT && !L.no_comm && c.n_bnd > 0 && halo_can_overlap(grid) &&
                           planes > c.n_bnd && !sg_capturing;
    if (split_dia) {
        const long pr = (long)DOF * L.g.plane();
        const bool both = L.g.has_lo && L.g.has_hi;
        TP_TRY(launch_rows(L.g.has_lo ? 0 : rows_all - pr, pr, both ? rows_all - pr : 0, both ? pr : 0));
        TP_TRY(after_boundary(c.l, a.out));
        TP_TRY(launch_rows(L.g.has_lo ? pr : 0, rows_all - pr * c.n_bnd, 0, 0));
        grid->launches++;
    } else {
        TP_TRY(launch_rows(0, -1, 0, 0));
    }
    c.bytes = (27.0 * DOF * DOF + 2.0 * DOF) * 8.0 * c.nown;
    c.flops = 2.0 * 27 * DOF * DOF * (double)c.nown;
    return TP_OK;
}

// ---- halos in flight on the second stream (one per level: the output of the last split launch)
template <int DOF>
int MGSolver<DOF>::drain_halo(int l) {  // DMGlobalToLocalEnd
    if (pend[l].ptr) {
        TP_HIP(hipStreamWaitEvent(grid->stream, pend_ev[l], 0));
        pend[l].ptr = nullptr;
    }
    return TP_OK;
}

template <int DOF>
int MGSolver<DOF>::drain_halos() {
    for (int l = 0; l < LV_SLOTS; l++) TP_TRY(drain_halo(l));
    return TP_OK;
}

// A kernel that writes whole owned planes of `out` one node at a time (vector updates, grid transfers), issued so
// that the ghost planes of `out` travel while its interior is computed: launch(p0, np) covers the owned planes
// [p0, p0 + np).  Tile levels of a slab run with the overlap available: boundary plane(s) first, exchange started
// on the second stream, then the interior; everywhere else one launch over all owned planes (the consumer's
// halo() exchanges).
template <int DOF>
template <class F>
int MGSolver<DOF>::planes_split(int l, double *out, F launch) {
    Level<DOF> &L = lv[l];
    const int lo = L.g.own_lo, hi = L.g.own_hi;
    const int n_bnd = (L.g.has_lo ? 1 : 0) + (L.g.has_hi ? 1 : 0);
    const bool tile_level = DOF == 3 && ((L.kind == LV_MATFREE && L.use_tile) || L.kind == LV_MACRO);
    if (pend[l].ptr) TP_TRY(drain_halo(l));
    if (!(tile_level && !L.no_comm && n_bnd > 0 && halo_can_overlap(grid) && hi - lo + 1 > n_bnd)) return launch(lo, hi - lo + 1);
    if (L.g.has_lo) TP_TRY(launch(lo, 1));
    if (L.g.has_hi) TP_TRY(launch(hi, 1));
    if (!pend_ev[l]) TP_HIP(hipEventCreateWithFlags(&pend_ev[l], hipEventDisableTiming));
    const int rc = halo_nodes_begin(grid, L.g, out, DOF, pend_ev[l]);
    if (rc == TP_OK) pend[l].ptr = out;
    else if (rc != 2) return rc;
    return launch(lo + (L.g.has_lo ? 1 : 0), hi - lo + 1 - n_bnd);
}

template <int DOF>
int MGSolver<DOF>::halo(int l, double *v) {
    if (lv[l].no_comm) return TP_OK;
    if (pend[l].ptr == v) return drain_halo(l);  // already under way: ordered behind it, nothing to exchange
    return halo_nodes(grid, lv[l].g, v, DOF);
}

// y = A_l u (ghost planes of u refreshed first)
template <int DOF>
int MGSolver<DOF>::apply(int l, double *u, double *y) {
    TP_TRY(halo(l, u));
    NodeArgs a{};
    a.x = u;
    a.out = y;
    return op<EPI_APPLY>(l, a);
}

// y = A_0 u with the operator of the Krylov method (the kernel of CG's A p; its dot product u . A u is discarded)
template <int DOF>
int MGSolver<DOF>::apply_krylov(double *u, double *y) {
    TP_TRY(halo(0, u));
    NodeArgs a{};
    a.x = u;
    a.out = y;
    a.partials = grid->partials;
    a.ticket = tail_ticket(grid);
    a.red_out = grid->scal + S_PW;
    TP_TRY(op<EPI_APPLY_DOT>(0, a));
    return finish_tail<1>(grid, last_nblocks, S_PW);
}
