"""The fusions the Krylov loop takes by default against their unfused forms, on 0/1 designs.

mg_cycle.h and mg_kernels.h say of each of them "same values, bit for bit"; nothing held them to it, and no test, tool or
benchmark ever set one of their off-switches.  One subprocess per setting (the library latches its switches once per process;
tests/cg_fusions_worker.py): the two rw.COARSE_MESHES x blocks, checker, zlayer x cantilever and scattered Dirichlet dofs, one
rank, the fine kernel of generation 2 (asserted: the CG direction formed inside the product runs there only), nsmooth 2,
ncoarse 20, the benchmark's cycle pattern cut to the level count, exactly 40 iterations (rtol tiny, dtol huge).  Dumped:
precond(r) of a seeded r, the residual history and U.

    setting                     against the default setting
    TP_NO_FUSE_FIRST=1          precond(r), history and U bit-equal   (the restriction / the CG update do not write the next
                                                                       level's / V-cycle's first Chebyshev step)
    TP_NO_CG_FUSE=1             the same, bit-equal                   (p = z + beta p outside the product, ||r||^2 through the stream)
    TP_NO_SPEC_HEAD=1           the same, bit-equal                   (no pre-smoothing enqueued ahead of the host's wait)
    TP_NO_FUSE_RZ=1             precond(r) bit-equal; the history within RZ_TOL of the default's, entry by entry, relative
                                to the entry: r . z by a dot kernel of its own is another summation order (the value itself is
                                held in tests/test_gpu_rowwise.py::test_fine_fused_dot_values)
    all four together           as TP_NO_FUSE_RZ=1

RZ_TOL is not chosen: it is 16 x the spread of the same histories among summation orders that exist already and are all
legitimate.  Measured on the MI355X on these cases, each against the default, max over cases and entries of |h - h0| / h0:
    TP_NO_REDUCE_TAIL=1 (second-launch tails)       0          bit-equal, as its comment says
    TP_FINE_V=3 (generation 3)                      0          bit-equal on these meshes: "identical bits from generation 2 on"
    TP_TILE_KZ=3 / 5 (another z-chunking: p . A p and r . z summed in another order)      3.7e-8 / 4.3e-8
    TP_FINE_V=1 (generation 1: another order inside the product as well)                 2.2e-8
so RZ_SPREAD_MEASURED = 4.3e-8 and RZ_TOL = 16 x that = 6.9e-7.  (Every one of them has its worst entry in the same case, mesh 0
zlayer cantilever, where the residual stagnates; the other eleven cases spread by <= 1.5e-9.)  TP_NO_FUSE_RZ=1 itself measured
4.5e-8 there, all four together the same.

One larger case for the non-temporal CG update, which only runs from 2^22 dofs: 128 x 104 x 104 elements (the smallest shape of
the project's aspect that reaches it), three levels, blocks, 5 iterations, TP_CG_NT=0 against the default: history and U
bit-equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rowwise as rw
KINDS = rw.CG_FUSION_KINDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = ("TP_NO_FUSE_FIRST", "TP_NO_CG_FUSE", "TP_NO_SPEC_HEAD", "TP_NO_FUSE_RZ")
SWITCHES = OFF + ("TP_CG_NT", "TP_FINE_V", "TP_FINE_SHAPE", "TP_TILE_KZ", "TP_NO_TILE", "TP_NO_REDUCE_TAIL")
SETTINGS = {
    "default": {},
    "no_fuse_first": {"TP_NO_FUSE_FIRST": "1"},
    "no_cg_fuse": {"TP_NO_CG_FUSE": "1"},
    "no_spec_head": {"TP_NO_SPEC_HEAD": "1"},
    "no_fuse_rz": {"TP_NO_FUSE_RZ": "1"},
    "all_four": {k: "1" for k in OFF},
}
RZ_SPREAD_MEASURED = 4.3e-8     # among existing summation orders (the docstring's table)
RZ_TOL = 16 * RZ_SPREAD_MEASURED
_WORK = {}


def worker(tmp_path_factory, mode, setting, env, gen=2, timeout=280):
    if (mode, setting) not in _WORK:
        out = str(tmp_path_factory.mktemp("cg") / "out.npz")
        e = dict(os.environ)
        for k in SWITCHES:
            e.pop(k, None)
        e.update(env)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cg_fusions_worker.py"), mode, str(gen), out], env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-3000:]
        d = np.load(out)
        _WORK[(mode, setting)] = {k: d[k] for k in d.files}
    return _WORK[(mode, setting)]


def tags():
    return ["c%d_%s_s%d" % (m, kind, s) for m in range(len(rw.COARSE_MESHES)) for kind in KINDS for s in (0, 1)]


def hist_spread(a, b):
    return float(np.max(np.abs(a - b) / b))


@pytest.mark.parametrize("setting", ["no_fuse_first", "no_cg_fuse", "no_spec_head"])
def test_fusion_is_bit_equal_to_its_unfused_form(tmp_path_factory, setting):
    d0, d1 = worker(tmp_path_factory, "small", "default", {}), worker(tmp_path_factory, "small", setting, SETTINGS[setting])
    for t in tags():
        for what in ("z", "hist", "U"):
            a, b = d1["%s_%s" % (t, what)], d0["%s_%s" % (t, what)]
            assert a.shape == b.shape and (what != "hist" or len(a) == 41), (setting, t, what, a.shape)
            assert np.array_equal(a, b), "%s %s: %s differs from the default's in %d of %d entries, first at %d, max |diff| / max = %.3e" % (
                setting, t, {"z": "precond(r)", "hist": "the residual history", "U": "U"}[what], int((a != b).sum()), a.size,
                int(np.flatnonzero(a != b)[0]), np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("setting", ["no_fuse_rz", "all_four"])
def test_unfused_rz_keeps_the_preconditioner_and_the_history(tmp_path_factory, setting):
    d0, d1 = worker(tmp_path_factory, "small", "default", {}), worker(tmp_path_factory, "small", setting, SETTINGS[setting])
    worst = 0.0
    for t in tags():
        assert np.array_equal(d1[t + "_z"], d0[t + "_z"]), "%s %s: precond(r) differs from the default's" % (setting, t)
        s = hist_spread(d1[t + "_hist"], d0[t + "_hist"])
        print("%s %s: history within %.3e of the default's (last entry / first %.2e)" % (setting, t, s, d0[t + "_hist"][-1] / d0[t + "_hist"][0]))
        worst = max(worst, s)
    assert worst <= RZ_TOL, (setting, worst, RZ_TOL)


def test_nontemporal_cg_update_is_bit_equal(tmp_path_factory):
    d0 = worker(tmp_path_factory, "large", "default", {}, timeout=120)
    d1 = worker(tmp_path_factory, "large", "cg_nt_0", {"TP_CG_NT": "0"}, timeout=120)
    assert len(d0["large_hist"]) == 6
    for what in ("hist", "U"):
        assert np.array_equal(d1["large_" + what], d0["large_" + what]), "TP_CG_NT=0: %s differs from the default's" % what
