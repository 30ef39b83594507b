"""The float64 oracle of the reference solver configuration (oracle/refksp.py) against the bounds of tests/refksp_rowwise.py, on
the CPU: its Gauss-Seidel sweeps are held to a QUARTER of each constant on every mesh, design kind and boundary condition of
tests/test_gpu_refksp_rowwise.py, its level GMRES is measured against the long-double restatement (the device's bound is 16 x that
distance), and an error of 1e-7 planted on the solid rows of a sweep is shown to fail the row-wise check while the older metric
passes it at the 1e-12 of tests/test_gpu_refksp.py::test_sor_and_jacobi_on_every_level.

MEASURED here (printed by the tests; pytest -s):
    sweeps, achieved c, largest over rr.CASES x rr.KINDS x both boundary conditions, forward and backward, of a bound / 4:
        level 0   4.47 of 32        level 1   2.12 of 64        level 2   3.41 of 64
    level GMRES, 4 iterations from zero and 4 more from the iterate, distance from the long-double restatement, largest over
    rr.GMRES_CASES x rw.GENERATORS (cantilever), solid / void rows (recorded as rr.GMRES_MEASURED):
        PCSOR     level 0  1.41e-14 / 7.05e-15    level 1  3.29e-14 / 1.15e-14    level 2  3.47e-14 / 1.08e-14
        PCJACOBI  level 0  2.72e-15 / 1.12e-15    level 1  6.45e-15 / 2.18e-15    level 2  1.80e-14 / 3.60e-15
    planted 1e-7 on the solid rows of PCSOR's backward sweep, 16 x 8 x 4 blocks and checker, 30 x 14 x 10 blocks, every level: the
        older metric moves by 1.4e-16 .. 5.6e-15 (passes 1e-12), the row-wise c is 2.6e7 .. 4.2e8 (of 128 / 256)
"""
import numpy as np
import pytest

from oracle import refksp
from tests import refksp_rowwise as rr
from tests import rowwise as rw

_H = {}
SWEPT, GM = {}, {}


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def hierarchy(orc, arb, m, scattered, kind):
    key = (m, scattered, kind)
    if key not in _H:
        _H.clear()                                  # one at a time: the parametrisation visits a key's tests in a row
        case = rr.CASES[m]
        (ex, ey, ez), nlv, _ = case
        nx, ny, nz = ex + 1, ey + 1, ez + 1
        KE = orc.hex8_ke_box(*rr.box(case), 0.3)
        N = rr.scattered_N(nx, ny, nz, np.random.default_rng(50 + m)) if scattered else orc.cantilever_bc(nx, ny, nz, rr.box(case))[0]
        _H[key] = rr.Hierarchy(orc, arb, case, KE, orc.simp(rr.design(orc, kind, (ex, ey, ez))), N)
    return _H[key]


@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("scattered", [0, 1])
@pytest.mark.parametrize("m", range(len(rr.CASES)))
def test_oracle_sweeps_hold_a_quarter_of_the_bound(orc, arb, m, scattered, kind):
    H = hierarchy(orc, arb, m, scattered, kind)
    rng = np.random.default_rng(rr.case_seed(m, scattered, kind))
    for l in range(H.nlv):
        A = H.mg.csr(l)
        b, x0 = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
        parts = refksp.ssor_parts(A)
        for backward in (False, True):
            x1 = rr.oracle_sweep(A, b, x0, backward, parts)
            lab = "oracle %s %s %s level %d %s sweep" % (rr.CASES[m][0], "scattered" if scattered else "cantilever", kind, l,
                                                         "backward" if backward else "forward")
            c = H.check_sweep(l, b, x0, x1, backward, lab, rr.c_gs(l) / 4)
            SWEPT[l] = max(SWEPT.get(l, 0.0), c)
    print("ORACLE SWEEPS achieved so far", {l: "%.3g of %g" % (v, rr.c_gs(l) / 4) for l, v in sorted(SWEPT.items())})


def test_long_double_sweep_is_the_sequential_one(orc, arb):
    """the restatement's own sweep (natural row order, 80-bit) leaves a mixed residual of 80-bit size, and the float64 loops agree
    with it to the row-wise bound: the two references stand where they should"""
    H = hierarchy(orc, arb, 0, 1, "checker")
    rng = np.random.default_rng(3)
    for l in range(H.nlv):
        M = H.csr(l)
        b, x0 = rng.standard_normal(M.n), rng.standard_normal(M.n)
        for backward in (False, True):
            x1 = M.sweep(b, x0, backward)
            res = M.sweep_residual(b, x0, x1, backward)
            s = rr.sweep_scale(orc, H.mg, l, H.dims, H.KE, H.E, H.N, b, x0, x1)
            pos = s > 0
            assert (np.abs(res[pos]).astype(np.float64) <= rr.c_gs(l) * 2.0 ** -64 * s[pos]).all()
            assert (res[~pos] == 0).all()


@pytest.mark.parametrize("kind", rw.GENERATORS)
@pytest.mark.parametrize("m", rr.GMRES_CASES)
def test_oracle_gmres_distance_from_the_long_double_restatement(orc, arb, m, kind):
    """no row scale is claimed: GMRES's coefficients couple all rows.  Measured per class of rows; 16 x this is the device's bound"""
    H = hierarchy(orc, arb, m, 0, kind)
    rng = np.random.default_rng(rr.case_seed(m, 0, kind) + 5)
    for l in range(H.nlv):
        A, M = H.mg.csr(l), H.csr(l)
        parts, cls = refksp.ssor_parts(A), M.classes()
        b = rng.standard_normal(M.n)
        for pc in (1, 0):
            P = (lambda r: refksp.ssor_apply(A, r, parts)) if pc else (lambda r: r / A.diagonal())
            Pl = M.ssor if pc else (lambda r: r / M.diag)
            xo, its, _ = refksp.gmres_left(A, P, b, None, 4, 4)
            xl, its_l = rr.gmres_ld(M, Pl, b, None, 4, 4)
            assert its == its_l == 4
            xo2, _, _ = refksp.gmres_left(A, P, b, xo, 4, 4)
            xl2, _ = rr.gmres_ld(M, Pl, b, xo, 4, 4)       # from the SAME iterate: the second run's own distance
            for name, mask in cls.items():
                for a, r in ((xo, xl), (xo2, xl2)):
                    d = rr.class_dist(a, r, mask)
                    if d is not None:
                        k = (pc, l, name)
                        GM[k] = max(GM.get(k, 0.0), d)
                        assert d <= 4 * rr.GMRES_MEASURED[(pc, l)][0 if name == "solid" else 1], (rr.CASES[m][0], kind, k, d)
    print("ORACLE GMRES distance so far", {k: "%.3g" % v for k, v in sorted(GM.items())})


def test_planted_error_fails_rowwise_and_passes_the_old_metric(orc, arb):
    """a relative error of 1e-7 on every solid row of the oracle's sweep: the row-wise check sees it, max|a - b| / max|b| does not"""
    for m, kind in ((0, "blocks"), (0, "checker"), (3, "blocks")):
        H = hierarchy(orc, arb, m, 0, kind)
        rng = np.random.default_rng(11)
        for l in range(H.nlv):
            A, M = H.mg.csr(l), H.csr(l)
            r = rng.standard_normal(M.n)
            solid = M.classes()["solid"]
            if l == 0:
                solid &= H.N != 0                   # (a Dirichlet row is the identity: nothing is computed there)
            # the production form: the symmetric sweep from a zero guess, as test_sor_and_jacobi_on_every_level compares it
            z = refksp.ssor_apply(A, r)
            y = rr.oracle_sweep(A, r, np.zeros(M.n))
            zb = rr.oracle_sweep(A, r, y, True)
            assert np.array_equal(zb, z)
            bad = np.where(solid, zb * (1 + 1e-7), zb)
            old = rw.rel(bad, z)
            assert old <= 1e-12, (rr.CASES[m][0], kind, l, old)
            lab = "planted %s %s level %d" % (rr.CASES[m][0], kind, l)
            H.check_sweep(l, r, y, zb, True, lab)                       # the unplanted sweep passes
            with pytest.raises(AssertionError, match="rows beyond"):
                H.check_sweep(l, r, y, bad, True, lab)
            res = M.sweep_residual(r, y, bad, True)
            s = rr.sweep_scale(orc, H.mg, l, H.dims, H.KE, H.E, H.N, r, y, bad)
            print("PLANTED %s %s level %d: old metric %.3g (passes 1e-12), row-wise c %.3g of %g"
                  % (rr.CASES[m][0], kind, l, old, rw.achieved(np.zeros(M.n), res, s), rr.c_gs(l)))
