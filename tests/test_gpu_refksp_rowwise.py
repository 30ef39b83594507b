"""The reference solver configuration (ksp_mode 1, csrc/refksp.h) held ROW BY ROW on 0/1 designs: the Gauss-Seidel sweeps of PCSOR
(k_gs_wave) by their componentwise backward error against the 80-bit arbiter's matrices, PCJACOBI by its one product, the level
GMRES against a long-double restatement per class of rows -- tests/refksp_rowwise.py: why, the bounds, their counts and the
float64 oracle's own figures (tests/test_refksp_rowwise_oracle.py holds the oracle to a quarter of each bound on the CPU).

Sweeps: rr.CASES (the edges of k_gs_wave's thread grid and wavefront count; every mesh was admitted as listed) x the five 0/1
generators and the synthetic density (Emin = 1e-9) x the cantilever and scattered single-component Dirichlet dofs (the mask branch of
MatfreeOp::diag_block), on every level, seeded normal b and x0, through LinearElasticity.level_gs -- one sweep of RefKsp::ssor's own
launches.  Held: a forward and a backward sweep from a non-zero iterate; forward from zero then backward is level_pc(l, 1, b) bit
for bit; a Dirichlet row returns b bit for bit; two calls give the same bits; level_pc(l, 0, r) is one product by dinv.

ACHIEVED on the MI355X (c in units of eps x row scale; recorded for the reader, the bounds come from the counts):

                     sweeps from x0 != 0      from zero / PCSOR's backward    synthetic density
    level   bound    forward / backward, 0/1  sweep, 0/1                      (worst of the four)     PCJACOBI (bound 1)
    0       128      0.94 / 0.92              0.99 / 1.01                     2.91                    0.999
    1       256      10.2 / 11.9              10.7 / 9.76                     3.28                    0.995
    2       256      8.39 / 8.23              9.28 / 9.08                     3.29                    0.991
    level GMRES, distance from the long-double restatement (solid / void rows; bound 16 x the oracle's, rr.GMRES_MEASURED):
        PCSOR     level 0  9.0e-15 / 3.3e-15   level 1  4.8e-14 / 3.9e-15   level 2  3.2e-14 / 1.6e-14     worst device / bound 0.10
        PCJACOBI  level 0  3.6e-15 / 1.3e-15   level 1  4.3e-15 / 1.0e-15   level 2  3.0e-14 / 1.8e-15
    GMRES(12) x 12, PCJACOBI, level 0 with 62073 / 68607 owned dofs against float64 gmres_left: 7.2e-16 / 3.8e-16 (bound 1e-10)

A DEFECT THIS FILE SHOWED: from a non-zero iterate k_gs_wave returned xo + (b - xo) on a Dirichlet row, b only to rounding; it now
stores b itself (PCSOR's zero guess never met the case: its bits did not move).

PLANTED ERRORS (each run once against a scratch copy of the library, values only):
    (a) k_gs_wave's update scaled by 1 + 1e-7 on the rows with D[r][r] > 1e-3
    (b) the in-node correction dropped (the rows of a node do not see each other's new values)
    outcome, both alike: all 72 cases of test_sweeps_and_jacobi_rowwise and all 15 of test_level_gmres_against_the_long_double_
    restatement fail.  tests/test_gpu_refksp.py fails 7 of its 11 tests under (b) AND under (a) -- the expectation for (a) was that
    it would pass: on its synthetic density nearly every row has D > 1e-3, the largest rows included, so its SOR comparison moves
    to 2.2e-8 (bound 1e-12).  What it cannot see is such an error on rows that are not the largest: the 0/1 designs, planted on
    the CPU in tests/test_refksp_rowwise_oracle.py (older metric 1.4e-16 .. 5.6e-15, row-wise c 2.6e7 .. 4.2e8).
"""
import numpy as np
import pytest

from oracle import refksp
from tests import refksp_rowwise as rr
from tests import rowwise as rw
from tests import scipy_check as sc
from tests.test_gpu_parity import dev, host, make, rel, tp  # noqa: F401  (tp is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ACHIEVED = {}
_LE, _H = {}, {}


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def note(l, what, c, bound):
    ACHIEVED[(l, what)] = (max(ACHIEVED.get((l, what), (0.0, bound))[0], c), bound)


def solver(tp, m, scattered):
    """one LinearElasticity in ksp_mode 1 per (mesh, boundary condition), shared by the designs (the previous one is closed)"""
    if (m, scattered) not in _LE:
        for grid, le, _ in _LE.values():
            le.close()
            grid.close()
        _LE.clear()
        from tests import rowwise_worker as worker
        case = rr.CASES[m]
        (ex, ey, ez), nlv, _ = case
        nx, ny, nz = ex + 1, ey + 1, ez + 1
        grid = tp.Grid(nx, ny, nz, rr.box(case))
        le = tp.LinearElasticity(grid, tp.SolverOptions.reference_elasticity(nlvls=nlv))
        worker.bc(le, nx, ny, nz, scattered, np.random.default_rng(50 + m))
        _LE[(m, scattered)] = (grid, le, host(le.N))
    return _LE[(m, scattered)]


def assembled(tp, orc, arb, m, scattered, kind):
    """-> (le, the references of this design): the device assembled with the design, the oracle and the arbiter with KE, the
    oracle's moduli of the same design and the device's Dirichlet vector"""
    grid, le, N = solver(tp, m, scattered)
    case = rr.CASES[m]
    x = rr.design(orc, kind, case[0])
    le.AssembleStiffnessMatrix(dev(x), 1e-9, 1.0, 3.0)
    key = (m, scattered, kind)
    if key not in _H:
        _H.clear()
        _H[key] = rr.Hierarchy(orc, arb, case, le.KE, orc.simp(x), N)
    return le, _H[key]


@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("scattered", [0, 1])
@pytest.mark.parametrize("m", range(len(rr.CASES)))
def test_sweeps_and_jacobi_rowwise(tp, orc, arb, m, scattered, kind):
    le, H = assembled(tp, orc, arb, m, scattered, kind)
    assert le.level_count() == H.nlv
    rng = np.random.default_rng(rr.case_seed(m, scattered, kind))
    group = "synth" if kind == "synth" else "0/1"
    for l in range(H.nlv):
        n = 3 * le.level_nodes(l)
        assert n == H.csr(l).n
        b, x0 = rng.standard_normal(n), rng.standard_normal(n)
        bd = dev(b)
        lab = "%s %s %s level %d: " % (rr.CASES[m][0], "scattered" if scattered else "cantilever", kind, l)
        clamped = (H.N == 0) if l == 0 else np.zeros(n, dtype=bool)
        for backward in (0, 1):
            name = "backward" if backward else "forward"
            x1 = host(le.level_gs(l, backward, bd, dev(x0)))
            c = H.check_sweep(l, b, x0, x1, backward, lab + name + " sweep from a non-zero iterate")
            note(l, "%s %s" % (name, group), c, rr.c_gs(l))
            assert np.array_equal(x1[clamped], b[clamped]), lab + name + ": a Dirichlet row must return b bit for bit"
            assert np.array_equal(host(le.level_gs(l, backward, bd, dev(x0))), x1), lab + name + ": two calls differ"
        # the new export is the production path: forward from zero, then backward, is PCSOR's bits
        y = host(le.level_gs(l, 0, bd, dev(np.zeros(n))))
        z = host(le.level_gs(l, 1, bd, dev(y)))
        zp = host(le.level_pc(l, 1, bd))
        assert np.array_equal(z, zp), lab + "forward from zero + backward differs from level_pc(l, 1, b)"
        assert np.array_equal(host(le.level_pc(l, 1, bd)), zp), lab + "two PCSOR calls differ"
        assert np.array_equal(zp[clamped], b[clamped])
        note(l, "forward zero " + group, H.check_sweep(l, b, np.zeros(n), y, 0, lab + "forward sweep from zero"), rr.c_gs(l))
        note(l, "backward pcsor " + group, H.check_sweep(l, b, y, zp, 1, lab + "PCSOR's backward sweep"), rr.c_gs(l))
        # PCJACOBI: one rounded product by the level's own dinv
        dinv = host(le.level_dinv(l))
        zj = host(le.level_pc(l, 0, bd))
        p = rr.ld(b) * rr.ld(dinv)
        note(l, "jacobi", rw.assert_rowwise(zj, p, np.abs(p.astype(np.float64)) * rr.JACOBI_REF_SLACK, rr.C_JACOBI,
                                            {"label": lab + "PCJACOBI", "dims": H.level_dims(l)}), rr.C_JACOBI)
    print("ACHIEVED", {"level %d %s" % k: "%.3g of %g" % v for k, v in sorted(ACHIEVED.items())})


def test_level_gs_refuses_other_modes(tp, orc):
    grid, le, mg, x, KE, N, R = make(tp, orc, 16, 8, 4, 2)
    v = le.level_vec(0)
    with pytest.raises(tp.TopOptError) as err:
        le.level_gs(0, 0, v, v.clone())
    assert err.value.code == 2            # TP_ERR_STATE, as level_pc and level_gmres answer outside ksp_mode 1
    le.close()
    grid.close()


# ---- the level GMRES ------------------------------------------------------------------------------------------------------------
GM = {}


@pytest.mark.parametrize("kind", rw.GENERATORS)
@pytest.mark.parametrize("m", rr.GMRES_CASES)
def test_level_gmres_against_the_long_double_restatement(tp, orc, arb, m, kind):
    """4 iterations from zero and 4 more from the iterate, PCSOR and PCJACOBI, every level.  GMRES's coefficients couple all rows, so
    NO ROW SCALE IS CLAIMED: the distance is measured over the solid rows and over the void rows separately, and each is bounded by
    16 x the float64 oracle's own distance from the same restatement (rr.GMRES_MEASURED)"""
    le, H = assembled(tp, orc, arb, m, 0, kind)
    rng = np.random.default_rng(rr.case_seed(m, 0, kind) + 5)
    for l in range(H.nlv):
        M = H.csr(l)
        cls = M.classes()
        b = rng.standard_normal(M.n)
        for pc in (1, 0):
            Pl = M.ssor if pc else (lambda r: r / M.diag)
            xd, its = le.level_gmres(l, pc, 4, 4, dev(b), dev(np.zeros(M.n)), zero_guess=True)
            xd = host(xd)
            xl, its_l = rr.gmres_ld(M, Pl, b, None, 4, 4)
            assert its == its_l == 4
            xd2, its2 = le.level_gmres(l, pc, 4, 4, dev(b), dev(xd))
            xl2, _ = rr.gmres_ld(M, Pl, b, xd, 4, 4)        # from the device's own iterate: the second run's own distance
            assert its2 == 4
            for name, mask in cls.items():
                for start, a, r in (("zero", xd, xl), ("iterate", host(xd2), xl2)):
                    d = rr.class_dist(a, r, mask)
                    if d is None:
                        continue
                    k = (pc, l, name)
                    GM[k] = max(GM.get(k, 0.0), d)
                    print("GMRES %s %s pc %d level %d %s from %s: %.3g of %.3g" % (rr.CASES[m][0], kind, pc, l, name, start, d, rr.gmres_bound(pc, l, name)))
                    assert d <= rr.gmres_bound(pc, l, name), (rr.CASES[m][0], kind, k, start, d, rr.gmres_bound(pc, l, name))
    print("GMRES ACHIEVED", {k: "%.3g" % v for k, v in sorted(GM.items())})


@pytest.mark.parametrize("mesh,nlv,owned", [((32, 32, 18), 2, 62073), ((32, 32, 20), 3, 68607)])
def test_gmres_reductions_either_side_of_one_workgroup(tp, orc, mesh, nlv, owned):
    """dots() and norm() sum n <= 65536 owned dofs in one workgroup and more in grid_for(n, 256) workgroups plus a second launch
    (68607: 256 workgroups and a second grid stride with a tail); GMRES(12) for 12 iterations crosses the 8-vector chunk of the
    basis under both"""
    grid, le, mg, x, KE, N, R = make(tp, orc, *mesh, nlv, ksp_mode=1)
    assert mg.size(0) == owned
    A = mg.csr(0)
    dg = A.diagonal()
    b = np.random.default_rng(21).standard_normal(owned)
    xo, its_o, _ = refksp.gmres_left(A, lambda r: r / dg, b, None, 12, 12)
    xd, its = le.level_gmres(0, 0, 12, 12, dev(b), dev(np.zeros(owned)), zero_guess=True)
    assert its == its_o == 12
    d = rel(host(xd), xo)
    print("GMRES(12) level 0 of %s: %.3g" % (mesh, d))
    assert d <= 1e-10          # tests/test_gpu_refksp.py::test_level_gmres's tolerance from the zero guess
    le.close()
    grid.close()


def test_edge_paths(tp, orc):
    """zero right-hand side, b = 0 on a level, max_it = 0"""
    ex, ey, ez, nlv = 16, 8, 4, 3
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    for max_it in (200, 0):
        grid = tp.Grid(nx, ny, nz, 1.0 / ey)
        le = tp.LinearElasticity(grid, tp.SolverOptions.reference_elasticity(nlvls=nlv, max_it=max_it))
        le.SetUpLoadAndBC()
        if max_it:
            le.SetBC(le.N.clone(), torch.zeros_like(le.RHS))
        le.AssembleStiffnessMatrix(dev(rw.design("blocks", ex, ey, ez, 4)), 1e-9, 1.0, 3.0)
        u0 = torch.zeros_like(le.U) if max_it else dev(np.random.default_rng(5).standard_normal(3 * nx * ny * nz))
        le.U.copy_(u0)
        assert le.KSPSolve(hist_cap=8) == 0
        assert torch.isfinite(le.U).all() and torch.equal(le.U, u0)
        if max_it:
            for l in range(nlv):
                for pc in (1, 0):
                    z = le.level_vec(l)
                    xz, its = le.level_gmres(l, pc, 4, 4, z, dev(np.ones(z.numel())), zero_guess=True)
                    assert its == 0 and not xz.any()
                    x1 = dev(np.random.default_rng(6).standard_normal(z.numel()))
                    xk, its = le.level_gmres(l, pc, 4, 0, dev(np.ones(z.numel())), x1.clone())      # its = 0: nothing runs
                    assert its == 0 and torch.equal(xk, x1)
        le.close()
        grid.close()


@pytest.mark.parametrize("m", [3, 5])
def test_reference_pdefilter_on_odd_and_anisotropic_meshes(tp, orc, m):
    """RefKsp<1> (Filter type 2 with SolverOptions.reference_pdefilter) against RefSolver, as tests/test_gpu_refksp.py holds it on
    16 x 8 x 8: the 30 x 14 x 10 mesh (15 x 7 x 5 coarse elements) and the box of three different spacings, two levels"""
    case = rr.CASES[m]
    (ex, ey, ez), _, _ = case
    hx, hy, hz = rr.box(case)
    rmin = 2.56 * min(hx, hy, hz)
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, (hx, hy, hz))
    f = tp.Filter(grid, 2, rmin, tp.SolverOptions.reference_pdefilter(nlvls=2))
    x = np.random.default_rng(4).random(ex * ey * ez)
    xt, xp = grid.elem_vec(), grid.elem_vec()
    f.FilterProject(dev(x), xt, xp)
    mg = orc.MG(ex + 1, ey + 1, ez + 1, 1, 2)
    mg.assemble(f.KF())
    T = sc.elem_to_node_T(ex, ey, ez)
    S = refksp.RefSolver(mg, restart=20, rtol=1e-8, dtol=1e3, max_it=60, nsmooth=1, ncoarse=10, smooth_pc=0, coarse_pc=0, coarse_restart=10)
    u, its_o, hist_o = S.solve(hx * hy * hz * (T @ x), x0=T @ x)
    its, rn = f.last_pde_solve()
    assert its == its_o
    assert rn == pytest.approx(hist_o[-1], rel=1e-5)
    assert rel(host(xt), np.clip(T.T @ u, 0, 1)) <= 1e-9
    f.close()
    grid.close()
