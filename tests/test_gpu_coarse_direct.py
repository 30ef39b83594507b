"""The exact coarse solve (csrc/coarse_direct.h) over its whole admission window, and the overlapped set-up it sits in.

The window as a table (rw.CD_CASES, rw.cd_geom: band widths 1 .. 12 blocks, 5 .. 124 blocks, last blocks with and without
padding, both ends of the row count), every design at a modulus contrast of 1e9 (the five 0/1 generators of tests/rowwise.py and
the synthetic density), a seeded right-hand side and a column of the inverse.  One worker process per setting of the latched
switches (tests/coarse_direct_worker.py) assembles blocks, checker, blocks, checker and then the other designs on ONE solver
object and uses every assembly at once -- no synchronisation of the test's own between assembly and first use.

The solve.  Coarse matrices here have condition numbers of 1e11 .. 5e13: no fixed tolerance fits.  With x_a the 80-bit arbiter's
banded Cholesky solve on its own Galerkin hierarchy (MG.coarse_solve) and d(v) the distance of v from x_a -- in the energy norm
of the arbiter's matrix relative to x_a's, and as a relative maximum norm, each held on its own -- the device is held to
    d(device) <= 16 max(d(oracle), d(numpy W), floor)
against two float64 references: the oracle's banded Cholesky solve, and the device's METHOD restated in numpy on the oracle's
matrix (W = L^-1 by triangular solves, x = W^T (W b)); floor = rw.CD_FLOOR, the oracle's own distance where the matrix is well
conditioned.  Both inverse forms (divide and conquer, TP_CD_INVERT_COLUMNS=1) are held to it, and to each other at the same
bound.  The figures measured for the references and the device stand above rw.CD_CASES.

Stale data.  The second visit to a design equals the first bit for bit in everything dumped (coarse solves, V-cycle, every
level's operator, Jacobi diagonal and window), while the two designs differ by far more than the bound: a wait missing between
the factorisation's side stream, level 2's side stream, the spectrum chains or a level event and their consumers reads the
OTHER design's data and shows.  And the set-up's switches that only move work between streams and threads (TP_LANCZOS_SERIAL,
TP_NO_L2_ASIDE, TP_NO_SETUP_REORDER, TP_NO_LEVEL_EVENTS, TP_NO_DEFER_FACTOR, TP_CD_SPLIT_ENQUEUE=0, TP_LANCZOS_ONE_THREAD --
mg_spectra.h, mg_coarse.h and elasticity_setup_from_E launch the same kernels with the same arguments under each of them, the
coarsest level's Lanczos run included: lanczos() and lanczos_graph() both take lanczos_xcd / lanczos_enqueue), all together and
each alone, give the bits of the default set-up, residual history of the solve included; no mode recovered from a give-up.

Cost.  A worker process runs inside whichever test asks for it first -- the default one all ten cases with eight assemblies each
and the rejected geometries, about 3 s on the MI355X -- and every later test of that process only compares: the first test of a
process carries its time, and a worker that fails fails every test that reads it, with the worker's own message.  The parent's
references (two hierarchies and a dense inverse per case and design) are computed once and shared; the largest case takes 3 s
of CPU time per design."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rowwise as rw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERIAL = {"TP_LANCZOS_SERIAL": "1", "TP_NO_L2_ASIDE": "1", "TP_NO_SETUP_REORDER": "1", "TP_NO_LEVEL_EVENTS": "1", "TP_NO_DEFER_FACTOR": "1",
          "TP_CD_SPLIT_ENQUEUE": "0", "TP_LANCZOS_ONE_THREAD": "1"}
SWITCHES = tuple(SERIAL) + ("TP_CD_INVERT_COLUMNS", "TP_NO_L2_FAST", "TP_L2_BLOCKS", "TP_NO_COARSE_DIRECT", "TP_DEBUG_SYNC", "TP_TEST_FORCE_GIVEUP")
ALL = ",".join(str(i) for i in range(len(rw.CD_CASES)))
# process -> (environment, cases, the rejected geometries too)
PROCESSES = {"default": ({}, ALL, 1), "columns": ({"TP_CD_INVERT_COLUMNS": "1"}, ALL, 0),
             "serial": (SERIAL, ",".join(str(i) for i in rw.CD_SETUP_CASES), 0)}
PROCESSES.update({"only_" + k: ({k: v}, str(rw.CD_SETUP_CASES[1]), 0) for k, v in SERIAL.items()})
_WORK, _REF = {}, {}


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def worker(tmp_path_factory, name):
    """one subprocess per setting of the switches, shared by the tests that compare its outputs"""
    if name not in _WORK:
        env, cases, rej = PROCESSES[name]
        out = str(tmp_path_factory.mktemp("cd_" + name) / "out.npz")
        e = dict(os.environ)
        for k in SWITCHES:
            e.pop(k, None)
        e.update(env)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "coarse_direct_worker.py"), out, cases, str(rej)], env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-3000:]
        d = np.load(out)
        _WORK[name] = {k: d[k] for k in d.files}
    return _WORK[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def references(orc, arb, d, ci, kind):
    """{right-hand side: (x_a, d(oracle), d(numpy W), the rw.CdNorm of the arbiter's matrix, (residual of the oracle's solve, of the
    numpy restatement's, b))} of one (case, design), computed once"""
    if (ci, kind) not in _REF:
        mesh, nlv = rw.CD_CASES[ci][:2]
        step = rw.CD_SEQUENCE.index(kind)
        x = d["c%d_s%d_x" % (ci, step)]
        assert np.array_equal(x, rw.cd_design(orc, kind, mesh))
        ref = rw.CdRef(orc, arb, mesh, nlv, d["c%d_KE" % ci], orc.simp(x), d["c%d_N" % ci])
        out = {}
        for name, b in rw.cd_rhs(rw.cd_geom(mesh, nlv)[0], ci).items():
            xa, xo, xw = ref.solves(b)
            out[name] = (xa, ref.dist(xo, xa), ref.dist(xw, xa), ref.norm, (ref.residual(b, xo), ref.residual(b, xw), b))
        _REF[(ci, kind)] = out
    return _REF[(ci, kind)]


def bound(do, dw):
    return tuple(rw.CD_MARGIN * max(o, w, f) for o, w, f in zip(do, dw, rw.CD_FLOOR))


@pytest.mark.parametrize("ci", range(len(rw.CD_CASES)))
def test_admitted_geometries_report_their_rows(tmp_path_factory, ci):
    """coarse_direct_active() after every assembly == the table's rows for coarse_direct = 2, and for coarse_direct = 1; the
    table itself == the restated admission rule (also held on the CPU, tests/test_rowwise_oracle.py)"""
    d = worker(tmp_path_factory, "default")
    mesh, nlv, rows1, rows2 = rw.CD_CASES[ci]
    assert (rw.cd_rows(mesh, nlv, 1), rw.cd_rows(mesh, nlv, 2)) == (rows1, rows2) and rows2 == rw.cd_geom(mesh, nlv)[1] > 0
    assert int(d["c%d_active_cd1" % ci][0]) == rows1, (mesh, int(d["c%d_active_cd1" % ci][0]), rows1)
    for step in range(len(rw.CD_SEQUENCE)):
        assert int(d["c%d_s%d_active" % (ci, step)][0]) == rows2, (mesh, step)
    assert tuple(d["c%d_xcd" % ci]) == (0, 0, 0), "a one-XCD kernel gave up: %s" % (d["c%d_xcd" % ci],)


def test_rejected_geometries_fall_back_bit_for_bit(tmp_path_factory):
    """too many rows, too few rows, and the small levels under coarse_direct = 1: 0 rows, and the solve of coarse_direct = 0"""
    d = worker(tmp_path_factory, "default")
    tags = [("rej%d" % q, (1, 2), m) for q, (m, _) in enumerate(rw.CD_REJECTED)] + [("rejc%d" % ci, (1,), c[0]) for ci, c in enumerate(rw.CD_CASES) if c[2] == 0]
    assert len(tags) >= 4
    for tag, cds, mesh in tags:
        for c in cds:
            assert int(d["%s_cd%d_active" % (tag, c)][0]) == 0, (mesh, c)
            assert int(d["%s_cd%d_its" % (tag, c)][0]) == int(d["%s_cd0_its" % tag][0]) > 0, (mesh, c)
            assert same_bits(d["%s_cd%d_U" % (tag, c)], d["%s_cd0_U" % tag]) and np.abs(d["%s_cd0_U" % tag]).max() > 0, (mesh, c)
    for mesh, nlv in rw.CD_REJECTED:
        assert rw.cd_rows(mesh, nlv, 1) == rw.cd_rows(mesh, nlv, 2) == 0


@pytest.mark.parametrize("kind", rw.CD_DESIGNS)
@pytest.mark.parametrize("ci", range(len(rw.CD_CASES)))
def test_exact_coarse_solve_within_16x_of_the_references(tmp_path_factory, orc, arb, ci, kind):
    """d(device) <= 16 max(d(oracle), d(numpy W), floor) in both norms, for both inverse forms, and the two forms' distance from
    each other at the same bound (the module's docstring)"""
    forms = {f: worker(tmp_path_factory, f) for f in ("default", "columns")}
    mesh, nlv = rw.CD_CASES[ci][:2]
    step = rw.CD_SEQUENCE.index(kind)
    refs = references(orc, arb, forms["default"], ci, kind)
    fails = []
    for name, (xa, do, dw, nrm, (ro, rw_, b)) in refs.items():
        bd = bound(do, dw)
        xs = {f: d["c%d_s%d_xs_%s" % (ci, step, name)] for f, d in forms.items()}
        for f, v in xs.items():
            assert np.isfinite(v).all(), (mesh, kind, name, f)
            dv = nrm.dist(v, xa)
            print("CD %s %d levels KB %d %-9s %-6s %-7s: d(oracle) %.2e %.2e  d(numpy W) %.2e %.2e  d(device) %.2e %.2e  bound %.2e %.2e"
                  % ((mesh, nlv, rw.cd_geom(mesh, nlv)[2], kind, name, f) + do + dw + dv + bd))
            if not (dv[0] <= bd[0] and dv[1] <= bd[1]):
                fails.append((f, name, dv, bd))
            # second line, independent of the arbiter's hierarchy: the device's OWN operator applied to its solution against b, at
            # 16 x the references' own residual max|A x - b| / max|b| (float64 solves and product, the oracle's matrix; it carries
            # the rounding of its own product as the device's does: the references measure 1 .. 4 eps max(|A| |x|) / max|b|)
            rd = float(np.abs(forms[f]["c%d_s%d_Axs_%s" % (ci, step, name)] - b).max() / np.abs(b).max())
            rb = rw.CD_MARGIN * max(ro, rw_)
            print("CD %s %-9s %-6s %-7s: residual oracle %.2e numpy W %.2e device %.2e bound %.2e" % (mesh, kind, name, f, ro, rw_, rd, rb))
            if not rd <= rb:
                fails.append((f, name, "residual", rd, rb))
        # the two forms against each other: the same norms, about the divide-and-conquer result
        dd = np.asarray(xs["columns"], dtype=np.longdouble) - np.asarray(xs["default"], dtype=np.longdouble)
        dm = (float(nrm.energy(dd) / nrm.energy(xa)), float(np.abs(dd).max() / np.abs(xa).max()))
        print("CD %s %-9s %-6s forms apart: %.2e %.2e" % (mesh, kind, name, dm[0], dm[1]))
        if not (dm[0] <= bd[0] and dm[1] <= bd[1]):
            fails.append(("forms apart", name, dm, bd))
    assert not fails, (mesh, kind, fails)


def test_inverse_forms_are_two_forms(tmp_path_factory):
    """TP_CD_INVERT_COLUMNS took effect: the block-column substitution sums in another order than the divide and conquer, so
    over the table the two workers' solutions are NOT all bit-equal (a switch that the library no longer read would run the
    default form twice and pass every bound)"""
    a, b = worker(tmp_path_factory, "default"), worker(tmp_path_factory, "columns")
    keys = [k for k in a if "_xs_" in k]
    assert len(keys) == len(rw.CD_CASES) * len(rw.CD_SEQUENCE) * 2 and all(k in b for k in keys)
    differ = [k for k in keys if not same_bits(a[k], b[k])]
    print("CD inverse forms: %d of %d solutions differ in bits" % (len(differ), len(keys)))
    assert differ, "the two inverse forms gave the same bits everywhere: did TP_CD_INVERT_COLUMNS take effect?"
    # what does not pass through the inverse is the same in both processes
    for k in a:
        if k.endswith(("_dinv1", "_lam1", "_apply1")):
            assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize("form", ["default", "columns"])
@pytest.mark.parametrize("ci", range(len(rw.CD_CASES)))
def test_revisited_design_is_bit_equal_and_designs_differ(tmp_path_factory, orc, arb, ci, form):
    """blocks, checker, blocks, checker on one solver object: visit 2 of each design == visit 1 bit for bit in every dumped
    quantity, and the two designs differ by more than 100 x the bound of the solve -- so data of the previous assembly, read
    through a missing wait, cannot pass"""
    d = worker(tmp_path_factory, form)
    mesh, nlv = rw.CD_CASES[ci][:2]
    keys = sorted(k[len("c%d_s0_" % ci):] for k in d if k.startswith("c%d_s0_" % ci))
    assert {"z", "xs_normal", "xs_unit", "Axs_normal", "apply%d" % (nlv - 1), "dinv1", "lam1"} <= set(keys), keys
    for first, second in ((0, 2), (1, 3)):
        assert rw.CD_SEQUENCE[first] == rw.CD_SEQUENCE[second]
        for k in keys:
            a, b = d["c%d_s%d_%s" % (ci, first, k)], d["c%d_s%d_%s" % (ci, second, k)]
            assert np.isfinite(a).all(), (mesh, k)
            assert same_bits(a, b), "%s %s: %s of visit 2 of %s differs from visit 1 (max |diff| %.3e of %.3e)" % (
                form, mesh, k, rw.CD_SEQUENCE[first], np.abs(a - b).max() if a.shape == b.shape else np.nan, np.abs(a).max())
    # A against B: the coarse solve relative to the bound of this case; the V-cycle, the operators and the Jacobi diagonals of the
    # levels >= 1: at least a hundredth of the entries moved by more than a hundredth of their size
    ra, rb = references(orc, arb, worker(tmp_path_factory, "default"), ci, "blocks"), references(orc, arb, worker(tmp_path_factory, "default"), ci, "checker")
    for name in ra:
        xa, do, dw, nrm = ra[name][:4]
        bd = max(bound(do, dw)[1], bound(rb[name][1], rb[name][2])[1])
        apart = nrm.dist(d["c%d_s1_xs_%s" % (ci, name)], xa)[1]
        dev_a = nrm.dist(d["c%d_s0_xs_%s" % (ci, name)], xa)[1]
        print("CD %s %s %s: designs apart %.2e, bound %.2e, device on A %.2e" % (mesh, form, name, apart, bd, dev_a))
        assert apart >= 100 * bd, (mesh, name, apart, bd)
    for k in ["z"] + ["apply%d" % l for l in range(1, nlv)] + ["dinv%d" % l for l in range(1, nlv)]:
        # (entry by entry: the largest entries belong to the clamped rows, which no design moves)
        a, b = d["c%d_s0_%s" % (ci, k)], d["c%d_s1_%s" % (ci, k)]
        moved = int((np.abs(a - b) > 1e-2 * np.maximum(np.abs(a), np.abs(b))).sum())
        assert moved >= max(10, a.size // 100), (mesh, k, moved, a.size)


@pytest.mark.parametrize("mode", [m for m in PROCESSES if m not in ("default", "columns")])
def test_overlapped_setup_equals_the_serial_one(tmp_path_factory, mode):
    """every switch that moves the set-up's work between streams and threads, all seven together (both set-up cases) and each
    alone (the three-level case): the bits of the default set-up in every level's operator, Jacobi diagonal and window, the
    coarse solve, the V-cycle and the residual history of KSPSolve from a zero start, after each of the four assemblies of the
    A / B / A / B sequence.  None of them changes a kernel or the order of a sum (the module's docstring): no exception."""
    ref, d = worker(tmp_path_factory, "default"), worker(tmp_path_factory, mode)
    cases = [int(v) for v in PROCESSES[mode][1].split(",")]
    for ci in cases:
        mesh, nlv = rw.CD_CASES[ci][:2]
        assert tuple(d["c%d_xcd" % ci]) == (0, 0, 0) and tuple(ref["c%d_xcd" % ci]) == (0, 0, 0), (mode, d["c%d_xcd" % ci], ref["c%d_xcd" % ci])
        keys = sorted(k for k in ref if k.startswith("c%d_s" % ci))
        assert sorted(k for k in d if k.startswith("c%d_s" % ci)) == keys
        assert {"c%d_s3_hist" % ci, "c%d_s2_lam%d" % (ci, nlv - 2), "c%d_s1_dinv1" % ci, "c%d_s7_xs_unit" % ci} <= set(keys)
        for k in keys:
            assert same_bits(ref[k], d[k]), "%s %s: %s differs from the default set-up (max |diff| %.3e of %.3e)" % (
                mode, mesh, k, np.abs(ref[k] - d[k]).max() if ref[k].shape == d[k].shape else np.nan, np.abs(ref[k]).max())
        for step in range(4):
            h = ref["c%d_s%d_hist" % (ci, step)]
            assert h.size >= 3 and np.isfinite(h).all() and (h > 0).all(), (mesh, step, h)
