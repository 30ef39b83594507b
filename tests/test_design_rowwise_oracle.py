"""The yardstick of tests/test_gpu_design_rowwise.py held on the CPU (tests/design_rowwise.py: the cases, the row scales, the
constants).  For every family -- overhang, casting, local volume, length scale -- on every case of that module:

  * the float64 restatement stays within a QUARTER of every row-wise bound against the 80-bit one; the achieved constants are
    printed beside that quarter, and the largest of each is what stands beside the constant in tests/design_rowwise.py;
  * every scale is finite and non-negative, and zero only where the reference is exactly zero;
  * one planted error per family on the largest row below 1e-8 of the maximum, of relative size 1e-3: the older metric of that
    family's GPU test (kept as rowwise.rel, with that test's own bound) accepts it, the row-wise bound rejects it and names the
    row; where the older metric does see it, that is asserted and a second error at half of what the older metric accepts is
    planted (as tests/test_response_rowwise_oracle.py does);
  * one broken seam read per filter, on the restatement: the transpose of the overhang with the T[c + PW] neighbour dropped along
    a tile edge (r = 7 | 8) -- on the rows where the older metric accepts the loss, the row-wise bound rejects it -- and that of the
    casting filter with the tile hand-over dropped at k = 32 of an x draw, which both metrics see on every field;
  * the column x = (1e-8, 0.5, 0.5), g = 1 of the overhang filter: without the floor on the support sum the float64
    restatement gives w = inf; with it float64 and 80-bit agree row by row and are finite."""
import numpy as np
import pytest

from tests import casting_ref as cref
from tests import design_rowwise as dr
from tests import lengthscale_ref as lsref
from tests import localvol_ref as lvref
from tests import overhang_ref as oref
from tests import rowwise as rw

LD = np.longdouble
MEASURED = {}


def note(prefix, got):
    for k, v in got.items():
        MEASURED[prefix + k] = max(MEASURED.get(prefix + k, 0.0), v)


def _report(prefix, quarters):
    print("float64 restatement against the 80-bit one, largest achieved c so far (bound: a quarter of the constant): "
          + ", ".join("%s %.2f (%g)" % (k, MEASURED[prefix + k], q) for k, q in quarters.items() if prefix + k in MEASURED))


def _scale_ok(ref, scale, label, exact=False):
    """exact: rows of scale 0 may carry a value that is no result of arithmetic (layer 0 of the overhang: xi = x, a = 1)"""
    s, r = np.asarray(scale), np.asarray(ref)
    assert np.isfinite(s.astype(np.float64)).all() and (s >= 0).all(), label
    assert exact or not r[s == 0].any(), "%s: a row of scale 0 whose reference is not 0" % label


# ---------------------------------------------------------------------------------------------------------------------
# the restatements within a quarter
# ---------------------------------------------------------------------------------------------------------------------
def _ov_f64(case):
    fd = oref.forward(case["x"], case["ne"], case["build"], np.float64, *case["params"])
    return fd, [oref.adjoint(fd, g, case["ne"], case["build"]) for g in case["g"]]


@pytest.mark.parametrize("build", dr.OV_BUILDS)
@pytest.mark.parametrize("ne", dr.OV_MESHES)
def test_overhang_restatement_within_a_quarter(ne, build):
    for pi in range(len(dr.OV_PARAMS)):
        for kind in dr.ov_fields(ne, build, pi):
            c = dr.ov_case(ne, build, kind, pi)
            for k in ("xi", "a", "w"):
                _scale_ok(c["fl"][k], c["scale"][k], c["label"] + " " + k, exact=True)
            fd, outs = _ov_f64(c)
            note("ov_", dr.ov_hold(c, fd["xi"], fd["a"], fd["w"], fd["p"], outs, div=4, tag="restatement "))
    _report("ov_", dict(xi=dr.C_OV_XI / 4, a=dr.C_OV_COEF / 4, w=dr.C_OV_COEF / 4, p=dr.C_OV_POW / 4, adj=dr.c_ov_adj(1) / 4))


def test_the_cases_left_out_are_the_ones_whose_branch_roundings_decide():
    """OV_UNDECIDABLE is no wider than it has to be: on each of its cases the margin assertion of ov_case fires (on every other
    combination of mesh, build, field and parameter set it does not: the test above runs them all)"""
    assert len(dr.OV_UNDECIDABLE) == 16 and all(pi in (1, 2) for _, _, _, pi in dr.OV_UNDECIDABLE)
    for ne, build, kind, pi in sorted(dr.OV_UNDECIDABLE):
        with pytest.raises(AssertionError, match="too close to S_MIN") as e:
            dr.ov_case(ne, build, kind, pi)
        print(pi, str(e.value))


def test_tail_field_reaches_the_band_and_stays_off_the_floor():
    """what the tail field is for: at the default parameters, without the floor, float64 has non-finite w on it and cells whose
    support sum vanished although the 80-bit one is positive; with the floor every support sum is a factor 2 off S_MIN (ov_case
    asserts it) and both branches occur"""
    for ne in dr.OV_MESHES:
        for build in ("+z", "-y"):
            if oref.layers(np.zeros(ne[0] * ne[1] * ne[2]), ne, build).shape[0] < 3:
                continue
            c = dr.ov_case(ne, build, "tail", 0)
            with np.errstate(all="ignore"):
                f0 = oref.forward(c["x"], ne, build, np.float64, s_min=0.0)
            l0 = oref.forward(c["x"], ne, build, LD, s_min=0.0)
            lost = int(((f0["S"] == 0) & (l0["S"] > 0)).sum())
            S = c["fl"]["S"]
            below, above = int(((S > 0) & (S < oref.S_MIN)).sum()), int((S >= oref.S_MIN).sum())
            print("%s %s: without the floor %d non-finite w, %d support sums lost in float64; with it %d cells below S_MIN, %d above"
                  % (ne, build, int((~np.isfinite(f0["w"])).sum()), lost, below, above))
            assert not np.isfinite(f0["w"]).all() and (lost > 0 or ne[0] < 14)       # (7e-9 is planted from 14 cells along x on)
            assert below > 0 and above > 0


@pytest.mark.parametrize("ne", dr.CAST_MESHES)
def test_casting_restatement_within_a_quarter(ne):
    for draw in cref.draws(ne):
        for kind in dr.CAST_FIELDS:
            c = dr.cast_case(ne, draw, kind)
            for k in ("c", "q"):
                _scale_ok(c["fl"][k], c["scale"][k], c["label"] + " " + k, exact=True)
            fd = cref.forward(c["x"], ne, draw, np.float64)
            outs = [cref.adjoint(fd, g, ne, draw) for g in c["g"]]
            note("cast_", dr.cast_hold(c, fd["c"], fd["q"], outs, div=4, tag="restatement "))
    _report("cast_", dict(c=dr.C_CAST_C / 4, q=dr.C_CAST_Q / 4, adj=dr.c_cast_adj(1) / 4))


@pytest.mark.parametrize("p", dr.LV_PS)
@pytest.mark.parametrize("mesh", sorted(dr.LV_MESHES))
def test_local_volume_restatement_within_a_quarter(mesh, p):
    ne, h, R = dr.LV_MESHES[mesh]
    for kind in dr.LV_FIELDS:
        c = dr.lv_case(ne, h, R, kind, p)
        f = lvref.reference(c["rho"], ne, h, R, dr.LV_ALPHA, p, dtype=np.float64)
        got = dr.lv_hold(c, f["rb"], f["dgdx"], div=4, tag="restatement ")
        note("lv_%s_" % mesh, got)
        # a ball of zeros: exactly 0 (scale 0), and the 0/1 designs do have such rows
        if kind in ("one_solid", "half") and mesh != "d":
            assert (c["ref"]["rb"] == 0).any()
    _report("lv_%s_" % mesh, dict(rb=c["c"][0] / 4, dgdx=c["c"][1] / 4))


@pytest.mark.parametrize("pj", range(len(dr.LS_PROJ)))
@pytest.mark.parametrize("mesh", sorted(dr.LS_MESHES))
def test_length_scale_restatement_within_a_quarter(mesh, pj):
    for kind in dr.LS_FIELDS:
        c = dr.ls_case(mesh, kind, pj)
        f = lsref.reference(c["rt"], c["ne"], c["h"], c["c"], dr.LS_ETA_S, dr.LS_ETA_V, dr.LS_EPS, c["proj"], c["beta"], lsref.ETA,
                            rb=c["rb"], dtype=np.float64)
        for name in ("solid", "void"):
            for k in ("T_", "dg_"):
                _scale_ok(c["r80"][k + name], c["scale"][k + name], c["label"] + " " + k + name)
            note("ls_", dr.ls_hold(c, name, f["T_" + name], f["dg_" + name], div=4, tag="restatement "))
        if kind in dr.DESIGNS:      # rt in {0, 1}: m = 0 exactly on the solid (void) cells -- bit-zero rows of T
            assert (c["scale"]["T_solid"] == 0).any() and (c["scale"]["T_void"] == 0).any()
    _report("ls_", dict(T=dr.C_LS_T / 4, dg=dr.C_LS_DG / 4))


# ---------------------------------------------------------------------------------------------------------------------
# planted errors: the older metric of each family's GPU test, restated with that test's own bound
# ---------------------------------------------------------------------------------------------------------------------
def _old_16d(got, ref, f64):
    """overhang, casting, length scale: max(16 x the float64 restatement's distance, 64 eps) of the maximum"""
    return float(rw.rel(got, ref)), max(16 * float(rw.rel(f64, ref)), 64 * dr.EPS)


def _planted(name, f64, ref, scale, c, old, where, candidates=None, old_sees_it=False, below=1e-8):
    """-> the row.  old_sees_it: the families whose older bound does see 1e-3 of the row (1e-3 of a row at 1e-8 of the maximum is
    1e-11 of the maximum; a bound of 64 eps sees it unless the row lies below 7e-12).  The issue expects the older metric to accept;
    where it cannot, that fact is asserted, the row-wise bound must STILL reject the 1e-3 error, and an error the older metric does
    accept (half its bound on this row) is planted and must be rejected too"""
    f64 = np.asarray(f64, dtype=np.float64)
    bad, row = dr.plant(ref, scale, candidates, below=below)
    got, bound = old(bad.astype(np.float64), ref, f64)
    print("%s: row %d (|ref| / max |ref| = %.1e, scale / max scale = %.1e) x (1 + %g): older metric %.3e (its bound %.1e: %s)"
          % (name, row, float(abs(ref[row]) / np.abs(ref).max()), float(scale[row] / scale.max()), dr.PLANT, got, bound,
             "seen" if got > bound else "accepted"))
    assert (got > bound) == old_sees_it, "the older metric %s the planted error" % ("sees" if got > bound else "does not see")
    if old_sees_it:
        with pytest.raises(AssertionError, match=r"worst: row %d," % row):
            dr.hold(bad.astype(np.float64), ref, scale, c, where)
        delta = 0.5 * bound * float(np.abs(ref).max() / abs(ref[row]))        # half of what the older metric accepts here
        assert delta < dr.PLANT
        bad = np.array(ref, dtype=LD)
        bad[row] = bad[row] * (1 + LD(delta))
        got, bound = old(bad.astype(np.float64), ref, f64)
        print("%s: row %d x (1 + %.2e): older metric %.3e (its bound %.1e: accepted)" % (name, row, delta, got, bound))
        assert got <= bound
    with pytest.raises(AssertionError, match=r"worst: row %d," % row) as e:
        dr.hold(bad.astype(np.float64), ref, scale, c, where)
    print("    row-wise, c = %g: rejected -- %s" % (c, str(e.value)[:260]))
    dr.hold(f64, ref, scale, c, where)          # (the unplanted result passes)
    return row


def test_planted_error_overhang_transpose():
    """out = a lambda with a >= eps / 4 = 2.5e-5 and lambda = g + ..: a row of the transpose is below 1e-8 of the maximum only by
    cancellation or a small g, never by its terms -- the overhang filter's rows of large range are p and w (the next test).  Here
    the largest row below 1e-4 of the maximum whose terms are that small too: the older metric sees 1e-3 of it, and accepts
    3.5e-11, which the row-wise bound rejects"""
    ne, build = (16, 12, 20), "+z"
    c = dr.ov_case(ne, build, "tail", 0)
    fd, outs = _ov_f64(c)
    co = {k: fd[k].astype(LD) for k in ("a", "w", "p")}
    ref, scale = oref.adjoint(co, c["g"][0], ne, build), oref.adjoint(co, np.abs(c["g"][0]), ne, build)
    _planted("overhang transpose", outs[0], ref, scale, dr.c_ov_adj(c["nl"]), _old_16d, {"label": c["label"] + " transpose", "dims": ne, "dof": 0},
             old_sees_it=True, below=1e-4)


def test_planted_error_overhang_p():
    """the overhang filter's planted error of the issue: the stored coefficients were not held at all -- whatever the older
    metric is given, it accepts -- so 1e-3 on p of a cell below 1e-8 of the largest p passed; the row-wise bound rejects it"""
    ne, build = (16, 12, 20), "+z"
    c = dr.ov_case(ne, build, "random", 0)
    fd, _ = _ov_f64(c)
    bad, row = dr.plant(c["fl"]["p"])
    with pytest.raises(AssertionError, match=r"worst: row %d," % row) as e:
        dr.hold(bad.astype(np.float64), c["fl"]["p"], c["scale"]["p"], dr.C_OV_POW, {"label": c["label"] + " p", "dims": ne, "dof": 0}, floor=dr.OV_FLOOR)
    print("overhang p: row %d x (1 + 1e-3): rejected -- %s" % (row, str(e.value)[:260]))
    dr.hold(fd["p"], c["fl"]["p"], c["scale"]["p"], dr.C_OV_POW, {"label": c["label"] + " p", "dims": ne, "dof": 0}, floor=dr.OV_FLOOR)


def test_planted_error_casting_transpose():
    ne, draw = (70, 37, 11), "+x"
    c = dr.cast_case(ne, draw, "random")
    fd = cref.forward(c["x"], ne, draw, np.float64)
    out = cref.adjoint(fd, c["g"][0], ne, draw)
    qd = fd["q"].astype(LD)
    ref, scale = cref.adjoint(dict(q=qd), c["g"][0], ne, draw), cref.adjoint(dict(q=qd), np.abs(c["g"][0]), ne, draw)
    _planted("casting transpose", out, ref, scale, dr.c_cast_adj(c["n"]), _old_16d, {"label": c["label"] + " transpose", "dims": ne, "dof": 0},
             old_sees_it=True)


def test_planted_error_local_volume_dgdx():
    """mesh a, checker, p = 16: min dgdx / max dgdx = 7.9e-14"""
    ne, h, R = dr.LV_MESHES["a"]
    c = dr.lv_case(ne, h, R, "checker", 16.0)
    f = lvref.reference(c["rho"], ne, h, R, dr.LV_ALPHA, 16.0, dtype=np.float64)
    b = lvref.bounds(c["conn"], 16.0)["dgdx"]
    ref = c["ref"]["dgdx"]
    print("min dgdx / max dgdx = %.2e" % float(ref.min() / ref.max()))
    _planted("local volume dgdx", f["dgdx"], ref, ref, c["c"][1], lambda got, r, f64: (float(rw.rel(got, r)), b),
             {"label": c["label"] + " dgdx", "dims": ne, "dof": 0})


@pytest.mark.parametrize("key", ["T_void", "T_solid"])
def test_planted_error_length_scale(key):
    """T: a row is small where m^2 or E is.  (dg gathers its neighbours' terms: no row of it is below 1e-8 of the maximum by its
    terms on these fields; its rows that small are cancellations, which no relative bound can hold)"""
    c = dr.ls_case("b", "checker", 2)
    f = lsref.reference(c["rt"], c["ne"], c["h"], c["c"], dr.LS_ETA_S, dr.LS_ETA_V, dr.LS_EPS, c["proj"], c["beta"], lsref.ETA, rb=c["rb"],
                        dtype=np.float64)
    _planted("length scale " + key, f[key], c["r80"][key], c["scale"][key], dr.C_LS_T if key[0] == "T" else dr.C_LS_DG, _old_16d,
             {"label": c["label"] + " " + key, "dims": c["ne"], "dof": 0}, old_sees_it=True)


# ---------------------------------------------------------------------------------------------------------------------
# broken seam reads, on the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_overhang_transpose_with_a_tile_edge_neighbour_dropped():
    """k_overhang_adj reads M[c + PW], the neighbour at r + 1; along the tile edge r = 7 that value comes from the rim.  The 80-bit
    recursion with that one read replaced by 0 on the cells of the edge where the loss is below HALF of what the older metric
    accepts: the older metric accepts, the row-wise bound rejects"""
    ne, build = (16, 12, 20), "+z"
    c = dr.ov_case(ne, build, "random", 0)
    fd, outs = _ov_f64(c)
    co = {k: fd[k].astype(LD) for k in ("a", "w", "p")}
    g = c["g"][0]
    ref, scale = oref.adjoint(co, g, ne, build), oref.adjoint(co, np.abs(g), ne, build)
    _, bound = _old_16d(ref.astype(np.float64), ref, outs[0])
    limit = LD(0.5 * bound) * np.abs(ref).max()
    bad = np.zeros(ref.size, dtype=LD)
    G, O = oref.layers(g.astype(LD), ne, build), oref.layers(bad, ne, build)
    A, W, Pc = (oref.layers(co[k], ne, build) for k in ("a", "w", "p"))
    m = np.zeros_like(G[0])
    hit = 0
    for l in range(G.shape[0] - 1, -1, -1):
        s = oref._cross(m)
        loss = A[l][7] * Pc[l][7] * np.abs(m[8])           # what out_l(r = 7) loses with m(r = 8) unread
        drop = (loss > 0) & (loss < limit)
        s_bad = s.copy()
        s_bad[7] = np.where(drop, s[7] - m[8], s[7])       # (the last addition of the cross: the term leaves without a trace)
        hit += int(drop.sum())
        lam = G[l] + Pc[l] * s                             # the recursion itself goes on unbroken: ONE read, not its consequences
        O[l] = A[l] * (G[l] + Pc[l] * s_bad)
        m = W[l] * lam
    got, bound = _old_16d(bad.astype(np.float64), ref, outs[0])
    print("overhang %s: T[c + PW] unread on %d cells of the tile edge: older metric %.3e (its bound %.1e)" % (c["label"], hit, got, bound))
    assert hit > 0 and got <= bound
    with pytest.raises(AssertionError, match="worst: row") as e:
        dr.hold(bad.astype(np.float64), ref, scale, dr.c_ov_adj(c["nl"]), {"label": c["label"] + " transpose, edge read dropped", "dims": ne, "dof": 0})
    print("    row-wise: rejected -- %s" % str(e.value)[:260])


def test_casting_transpose_with_the_tile_hand_over_dropped():
    """k_cast_x_adj hands mu across the tile edge through tc[]: the 80-bit recursion of a "+x" draw with the hand-over into cell
    k = 32 dropped (mu = g alone) on every line.  On record: here the older metric is NOT blind -- on every field the smallest loss
    on a line is above 4e-13 of the maximum, its bound is 9.4e-15 -- so it is asserted to see the break, and the row-wise bound
    must see it too, on every line"""
    ne, draw = (70, 37, 11), "+x"
    for kind in dr.CAST_FIELDS:
        c = dr.cast_case(ne, draw, kind)
        fd = cref.forward(c["x"], ne, draw, np.float64)
        out = cref.adjoint(fd, c["g"][0], ne, draw)
        qd, g = fd["q"].astype(LD), c["g"][0]
        ref, scale = cref.adjoint(dict(q=qd), g, ne, draw), cref.adjoint(dict(q=qd), np.abs(g), ne, draw)
        bad = ref.copy()
        G, O, Q = cref.lines(g.astype(LD), ne, 0), cref.lines(bad, ne, 0), cref.lines(qd, ne, 0)
        O[32] = (LD(0.5) * (1 + Q[32])) * G[32]         # "+x": the transpose runs from k = 0 up, mu_32 = g_32 + t_31; here without t_31
        got, bound = _old_16d(bad.astype(np.float64), ref, out)
        d = np.abs(cref.lines(bad - ref, ne, 0)[32])
        allow = dr.c_cast_adj(c["n"]) * dr.EPS * cref.lines(scale, ne, 0)[32]
        print("%s: tc[] hand-over dropped at k = 32: older metric %.3e (its bound %.1e); lines beyond the row-wise bound: %d of %d"
              % (c["label"], got, bound, int((d > allow).sum()), d.size))
        assert got > bound and (d > allow).all()
        with pytest.raises(AssertionError, match="worst: row"):
            dr.hold(bad.astype(np.float64), ref, scale, dr.c_cast_adj(c["n"]), {"label": c["label"] + " transpose, hand-over dropped", "dims": ne, "dof": 0})


# ---------------------------------------------------------------------------------------------------------------------
# the column of the overhang filter
# ---------------------------------------------------------------------------------------------------------------------
def test_overhang_column_with_a_tiny_support():
    """1 x 1 x 3, x = (1e-8, 0.5, 0.5), g = 1.  Without the floor the float64 restatement forms sw = (P/Q) Xi / S with
    S = 1e-320: w = inf and J^T g = (inf, ..); with S = 0 (x_0 = 7e-9) the row loses its support term.  With the floor on S
    (S < 2^-960: no support) float64 and 80-bit agree row by row and are finite"""
    ne, build = (1, 1, 3), "+z"
    g = np.ones(3)
    for x0 in (1.0e-8, 1.2e-8, 7e-9):
        x = np.array([x0, 0.5, 0.5])
        with np.errstate(all="ignore"):
            f0 = oref.forward(x, ne, build, np.float64, s_min=0.0)
            j0 = oref.adjoint(f0, g, ne, build)
        l0 = oref.forward(x, ne, build, LD, s_min=0.0)
        print("x0 = %g without the floor: float64 w = %s, J^T g = %s; 80-bit J^T g = %s"
              % (x0, f0["w"], j0, oref.adjoint(l0, g, ne, build).astype(np.float64)))
        if x0 != 7e-9:
            assert np.isinf(f0["w"][1]) and not np.isfinite(j0[0])
        else:
            assert f0["S"][1] == 0 and l0["S"][1] > 0
        fl, fd = oref.forward(x, ne, build, LD), oref.forward(x, ne, build, np.float64)
        sc = dr.ov_scales(x, ne, build, fl, dr.OV_PARAMS[0])
        case = dict(ne=ne, build=build, fl=fl, scale=sc, g=[g], nl=3, label="column x0 = %g" % x0)
        outs = [oref.adjoint(fd, g, ne, build)]
        got = dr.ov_hold(case, fd["xi"], fd["a"], fd["w"], fd["p"], outs, div=4)
        jl = oref.adjoint(fl, g, ne, build)
        print("    with the floor: J^T g = %s (80-bit %s), achieved c %s" % (outs[0], jl.astype(np.float64), got))
        assert all(np.isfinite(fd[k]).all() for k in fd) and np.isfinite(outs[0]).all()
        assert fd["w"][1] == 0 and fl["w"][1] == 0 and outs[0][0] == 1.0


def test_report_of_the_measured_constants():
    """(last in the file: what the tests above measured, for the comments beside the constants in tests/design_rowwise.py)"""
    for k in sorted(MEASURED):
        print("%-14s %.3f" % (k, MEASURED[k]))
