"""GPU parity of ksp_mode 1 -- the solver configuration the reference hard-codes (FGMRES + PCMG with GMRES / SOR level
solvers, LinearElasticity.cc:620-746; GMRES / Jacobi, PDEFilter.cc:276-378), csrc/refksp.h -- against its CPU
restatement oracle/refksp.py, building block by building block and as a whole.  FP64; tolerances per assertion."""
import math

import numpy as np
import pytest

from oracle import refksp
from tests import scipy_check as sc
from tests.test_gpu_parity import dev, host, make, rel, tp  # noqa: F401  (tp is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_sor_and_jacobi_on_every_level(tp, orc):
    """PCSOR = one symmetric Gauss-Seidel sweep from a zero guess, run wavefront by wavefront on the device: the fine level
    takes its rows from the moduli (no stored matrix), the coarse levels from their stencils"""
    grid, le, mg, x, KE, N, R = make(tp, orc, 16, 8, 8, 3, ksp_mode=1)
    rng = np.random.default_rng(0)
    for l in range(3):
        A = mg.csr(l)
        r = rng.standard_normal(mg.size(l))
        assert rel(host(le.level_pc(l, 1, dev(r))), refksp.ssor_apply(A, r)) <= 1e-12
        assert rel(host(le.level_pc(l, 0, dev(r))), r / A.diagonal()) <= 1e-14


@pytest.mark.parametrize("pc", [1, 0])
def test_level_gmres(tp, orc, pc):
    grid, le, mg, x, KE, N, R = make(tp, orc, 16, 8, 8, 3, ksp_mode=1)
    rng = np.random.default_rng(1)
    for l in range(3):
        A = mg.csr(l)
        M = (lambda r: refksp.ssor_apply(A, r)) if pc else (lambda r: r / A.diagonal())
        b = rng.standard_normal(mg.size(l))
        # a smoother as PCMG runs it: 4 iterations, no test; from zero, then from the iterate
        xo, its_o, _ = refksp.gmres_left(A, M, b, None, 4, 4)
        xd, its = le.level_gmres(l, pc, 4, 4, dev(b), dev(np.zeros_like(b)), zero_guess=True)
        assert its == its_o == 4
        assert rel(host(xd), xo) <= 1e-10
        xo2, _, _ = refksp.gmres_left(A, M, b, xo, 4, 4)
        xd2, _ = le.level_gmres(l, pc, 4, 4, dev(b), xd.clone())
        assert rel(host(xd2), xo2) <= 1e-9
    # the coarse solve: restarts and the test on the preconditioned residual
    A = mg.csr(2)
    M = (lambda r: refksp.ssor_apply(A, r)) if pc else (lambda r: r / A.diagonal())
    xo, its_o, hist = refksp.gmres_left(A, M, b, None, 10, 60, rtol=1e-8, atol=1e-50, dtol=1e5, test=True)
    xd, its = le.level_gmres(2, pc, 10, 60, dev(b), dev(np.zeros_like(b)), zero_guess=True, rtol=1e-8)
    assert its == its_o
    assert rel(host(xd), xo) <= 1e-7


@pytest.mark.parametrize("kind,nlv", [("synth", 3), ("uniform", 2)])
def test_reference_configuration_vcycle_and_solve(tp, orc, kind, nlv):
    grid, le, mg, x, KE, N, R = make(tp, orc, 16, 8, 8, nlv, kind, ksp_mode=1)
    S = refksp.RefSolver(mg)
    r = np.random.default_rng(2).standard_normal(mg.n)
    assert rel(host(le.precond(dev(r))), S.vcycle(0, r)) <= 1e-8
    its = le.KSPSolve(hist_cap=300)
    Uo, its_o, hist_o = S.solve(R * N)
    assert its == its_o
    h = le.last_hist
    assert len(h) == len(hist_o)
    # measured: first ten entries 1.3e-12 (synth, 3 levels) and 7.6e-11 (uniform, 2 levels: 3 iterations, the whole history);
    # whole history 1.5e-10 / 7.6e-11; U 9.7e-16 / 2.5e-13
    assert np.abs(h[:10] / hist_o[:10] - 1).max() <= 1e-10           # as test_solve_residual_history holds the CG path
    assert np.abs(h / hist_o - 1).max() <= 1e-9
    assert rel(host(le.U), Uo) <= 1e-11
    assert le.last_bnorm == pytest.approx(np.linalg.norm(R * N), rel=1e-14)
    assert le.KSPSolve() == 0      # warm start from the converged state
    # the option string says what ran
    s = le.petsc_options()
    assert "-ksp_type fgmres" in s and "-mg_levels_pc_type sor" in s and "-mg_coarse_ksp_gmres_restart 30" in s


def test_converged_state_is_the_fast_paths(tp, orc):
    """the two configurations solve the same system: at a tight tolerance displacement, compliance and sensitivities agree"""
    a = make(tp, orc, 32, 16, 16, 3, rtol=1e-11, max_it=400)
    b = make(tp, orc, 32, 16, 16, 3, rtol=1e-11, max_it=400, ksp_mode=1)
    out = []
    for grid, le, mg, x, KE, N, R in (a, b):
        dfdx, dgdx = grid.elem_vec(), grid.elem_vec()
        fx, gx = le.ComputeObjectiveConstraintsSensitivities(dfdx, dgdx, dev(x), 1e-9, 1.0, 3.0, 0.12)
        out.append((fx, host(dfdx), host(le.U), le.last_its))
    assert out[1][3] < out[0][3]                      # far stronger smoother: fewer outer iterations
    assert out[1][0] == pytest.approx(out[0][0], rel=1e-9)
    assert rel(out[1][1], out[0][1]) <= 1e-8
    assert rel(out[1][2], out[0][2]) <= 1e-8


def test_reference_pdefilter_configuration(tp, orc):
    ex, ey, ez = 16, 8, 8
    h = 1.0 / ey
    rmin = 2.56 * h
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    f = tp.Filter(grid, 2, rmin, tp.SolverOptions.reference_pdefilter())
    x = np.random.default_rng(4).random(ex * ey * ez)
    xt, xp = grid.elem_vec(), grid.elem_vec()
    f.FilterProject(dev(x), xt, xp)
    kf, _ = orc.pde_kf(h, h, h, rmin / 2 / np.sqrt(3))
    mg = orc.MG(ex + 1, ey + 1, ez + 1, 1, 3)
    mg.assemble(kf)
    T = sc.elem_to_node_T(ex, ey, ez)
    S = refksp.RefSolver(mg, restart=20, rtol=1e-8, dtol=1e3, max_it=60, nsmooth=1, ncoarse=10, smooth_pc=0, coarse_pc=0,
                         coarse_restart=10)
    u, its_o, hist_o = S.solve(h ** 3 * (T @ x), x0=T @ x)      # PDEFilter.cc:198-210
    its, rn = f.last_pde_solve()
    assert its == its_o
    assert rn == pytest.approx(hist_o[-1], rel=1e-5)
    assert rel(host(xt), np.clip(T.T @ u, 0, 1)) <= 1e-9
    # and the fast configuration gives the same filtered field to the solver tolerance
    f0 = tp.Filter(grid, 2, rmin)
    xt0 = grid.elem_vec()
    f0.FilterProject(dev(x), xt0, xp)
    assert rel(host(xt), host(xt0)) <= 1e-6


# ---- the outer FGMRES's own products (initial / restart residual, A Z_j) are the Krylov operator's ---------------------------
# A rigid translation on a free mesh of unit moduli: the reference's KE answers it with a small vector of its own (its rows do
# not sum to exactly 0), the Krylov operator (KE_krylov, MatMultKrylov) with that vector to rounding, the packed form the
# V-cycle applies (KE_effective, MatMult) with a different one -- 11 % short in norm on this mesh (pinned on the CPU in
# tests/test_oracle_refksp.py).  So a residual norm of the outer method says which operator formed it.
_TV = np.array([1000.0, -2000.0, 500.0])


def _free_mesh(tp, ex, ey, ez, nlv, **kw):
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    grid = tp.Grid(nx, ny, nz, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions.reference_elasticity(nlvls=nlv, **kw))
    n = 3 * nx * ny * nz
    le.SetBC(torch.ones(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"))
    le.AssembleStiffnessMatrix(grid.elem_vec(1.0), 0.0, 1.0, 3.0)
    return grid, le, np.tile(_TV, nx * ny * nz), (nx, ny, nz)


def _ld_apply(dims, K, u):
    """the matrix-free gather of element matrix K on the free mesh of unit moduli, summed in 80-bit arithmetic"""
    from oracle import arbiter as arb
    return np.asarray(arb.matfree_apply(*dims, 3, np.asarray(K, dtype=np.longdouble), None, None,
                                        np.asarray(u, dtype=np.longdouble)), dtype=np.longdouble)


def _fgmres_rebuilt(le, x0, steps, prod_res, prod_arn):
    """FGMRES(1) with b = 0 from x0 for `steps` iterations, from the library's primitives: each restart forms r = -prod_res(x),
    V0 = r / ||r||, Z = le.precond(V0) (the ksp_mode 1 V-cycle), w = prod_arn(Z), one classical Gram-Schmidt step and one Givens
    rotation; returns the recurrence residual norms [||r_0||, ||r_1||, ...] and the first V0, Z.  One step of it is also the
    first step of FGMRES(m) for any m."""
    x, hist, first = x0.clone(), [], None
    for _ in range(steps):
        r = -prod_res(x)
        beta = torch.linalg.norm(r).item()
        if not hist:
            hist.append(beta)
        v = r * (1.0 / beta)
        z = le.precond(v)
        w = prod_arn(z)
        h0 = torch.dot(v, w).item()
        h1 = torch.linalg.norm(w - h0 * v).item()
        d = math.hypot(h0, h1)
        hist.append(beta * h1 / d)
        x = x + (beta * h0 / (d * d)) * z
        if first is None:
            first = (host(v), host(z))
    return np.array(hist), first


def test_outer_residual_is_the_krylov_product(tp, orc):
    """FGMRES's initial residual (max_it = 0: ||r_0|| is all it computes) and its restart residual go through the Krylov
    operator: ||r_0|| = ||KE t|| of the 80-bit gather to rounding, where the packed form would give it 11 % short"""
    grid, le, t, dims = _free_mesh(tp, 24, 12, 12, 3, max_it=0)
    KE = le.KE
    n_ke = float(np.sqrt(np.sum(_ld_apply(dims, KE, t) ** 2)))
    n_eff = float(np.sqrt(np.sum(_ld_apply(dims, le.KE_effective(), t) ** 2)))
    assert abs(n_eff / n_ke - 1) >= 0.05          # the probe discriminates (CPU, 80-bit): -11.2 %
    le.U.copy_(dev(t))
    assert le.KSPSolve(hist_cap=4) == 0
    h0 = float(le.last_hist[0])
    assert abs(h0 / n_ke - 1) <= 2e-4             # measured -7.4e-5 (the packed form: -11.3 %)
    le.close()
    # FGMRES(1): the second iteration starts from a restart residual of the first iterate x1.  x1 = t + y Z0 cancels most of
    # the translation, so ||b - A x1|| carries the rounding of that sum: the step is rebuilt from the library's own x1 (a
    # max_it = 1 solve), not from a recomputed one
    grid2, le2, t, dims = _free_mesh(tp, 24, 12, 12, 3, max_it=1, restart=1)
    le2.U.copy_(dev(t))
    assert le2.KSPSolve(hist_cap=4) == 1
    x1 = le2.U.clone()
    le2.close()
    grid3, le3, t, dims = _free_mesh(tp, 24, 12, 12, 3, max_it=2, restart=1)
    le3.U.copy_(dev(t))
    assert le3.KSPSolve(hist_cap=4) == 2
    h = np.array(le3.last_hist)
    assert len(h) == 3
    kry, _ = _fgmres_rebuilt(le3, x1, 1, le3.MatMultKrylov, le3.MatMultKrylov)
    pck, _ = _fgmres_rebuilt(le3, x1, 1, le3.MatMult, le3.MatMultKrylov)     # the restart residual from the packed form
    assert abs(h[2] / kry[1] - 1) <= 1e-10       # measured 1.1e-16
    assert abs(pck[1] / kry[1] - 1) >= 0.02      # measured 3.7 %
    le3.close()
    grid.close()
    grid2.close()
    grid3.close()


def test_arnoldi_product_is_the_krylov_product(tp, orc):
    """FGMRES's A Z_j is the Krylov operator's: the first recurrence residual ||r_1|| (max_it = 1) is the one rebuilt from
    MatMultKrylov and the library's own V-cycle; rebuilt from MatMult (packed) it is 5 % off.  In 80-bit arithmetic on the same
    V0, Z0, the Krylov operator's element matrix and the reference's KE give the same ||r_1||"""
    grid, le, t, dims = _free_mesh(tp, 24, 12, 12, 3, max_it=1)
    td = dev(t)
    le.U.copy_(td)
    assert le.KSPSolve(hist_cap=4) == 1
    h = np.array(le.last_hist)
    kry, (v0, z0) = _fgmres_rebuilt(le, td, 1, le.MatMultKrylov, le.MatMultKrylov)
    pck, _ = _fgmres_rebuilt(le, td, 1, le.MatMult, le.MatMult)
    # the same step with products in 80-bit arithmetic on the library's V0 and Z0
    LD = np.longdouble

    def r1_of(K, w=None):
        beta = np.sqrt(np.sum(_ld_apply(dims, K, t) ** 2))
        w = _ld_apply(dims, K, z0) if w is None else w.astype(LD)
        v = v0.astype(LD)
        a0 = np.dot(v, w)
        a1 = np.sqrt(np.sum((w - a0 * v) ** 2))
        return float(beta * a1 / np.sqrt(a0 * a0 + a1 * a1))

    r1_kk, r1_ke = r1_of(le.KE_krylov()), r1_of(le.KE)
    # ... with the product w = A Z0 summed in double on the CPU (the oracle's matrix-free gather of the same KE_krylov)
    r1_dbl = r1_of(le.KE_krylov(), orc.matfree_apply(*dims, 3, np.asarray(le.KE_krylov(), dtype=np.float64), None, None, z0))
    # measured: the library's ||r1|| IS the step rebuilt from MatMultKrylov (0 apart); from MatMult it is 5.1 % off
    assert abs(h[0] / kry[0] - 1) <= 1e-10
    assert abs(h[1] / kry[1] - 1) <= 1e-10
    assert abs(pck[1] / kry[1] - 1) >= 0.05
    # On Z0 the Krylov operator is the reference's KE: in 80-bit arithmetic the two give ||r1|| 5.3e-5 apart.  The library's
    # double-precision value is 6.3 % from them, and that is the rounding of w = A Z0 in double, not the operator: Z0 is a
    # translation of rms 2.6e14 with a deviation of 2.9e12 and ||A Z0|| ~ 1, so its products cancel ~14 decades -- the CPU's
    # double gather of the same KE_krylov lands 22 % away.  No double-precision product can be held to the 80-bit one here.
    assert abs(r1_kk / r1_ke - 1) <= 1e-3
    assert abs(r1_dbl / r1_kk - 1) >= 0.1
    assert abs(h[1] / r1_kk - 1) <= abs(r1_dbl / r1_kk - 1)
    le.close()
    grid.close()


@pytest.mark.parametrize("mesh,nlv", [((32, 16, 16), 3), ((64, 32, 32), 4)])
def test_reference_configuration_against_the_oracle_at_scale(tp, orc, mesh, nlv):
    """The configuration the reference hard-codes (SolverOptions.reference_elasticity) on a cantilever with the filtered synthetic
    density, against its CPU restatement ON THE OPERATORS THE LIBRARY APPLIES: the outer products from KE_krylov, the V-cycle's
    level-0 products from KE_effective, PCSOR and the Galerkin hierarchy from KE (csrc/refksp.h)"""
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    grid = tp.Grid(nx, ny, nz, h)
    x = grid.synth_density()
    flt = tp.Filter(grid, 1, 2.56 * h)
    xt, xp = grid.elem_vec(), grid.elem_vec()
    flt.FilterProject(x, xt, xp)
    xpn = host(xp)
    le = tp.LinearElasticity(grid, tp.SolverOptions.reference_elasticity(nlvls=nlv))
    le.SetUpLoadAndBC()
    df, dg = grid.elem_vec(), grid.elem_vec()
    fx, _ = le.ComputeObjectiveConstraintsSensitivities(df, dg, xp, 1e-9, 1.0, 3.0, 0.12, hist_cap=300)
    its, hg, U, dfn = le.last_its, np.array(le.last_hist), host(le.U), host(df)
    kf, kk, KE = le.KE_effective(), le.KE_krylov(), le.KE
    le.close()
    N, R = orc.cantilever_bc(nx, ny, nz, h)
    E = orc.simp(xpn)
    mg = orc.MG(nx, ny, nz, 3, nlv)
    mg.assemble(KE, E, N)
    S = refksp.RefSolver(mg, A_outer=refksp.fine_operator(orc, nx, ny, nz, kk, E, N),
                         A_level0=refksp.fine_operator(orc, nx, ny, nz, kf, E, N))
    Uo, its_o, ho = S.solve(R * N)
    fo, _, dfo, _ = orc.compliance_sens(nx, ny, nz, KE, Uo, xpn)
    assert its == its_o
    assert len(hg) == len(ho)
    k = min(10, its + 1)
    # the operator's share: the same restatement on the reference's KE alone
    Uk, its_k, hk = refksp.RefSolver(mg).solve(R * N)
    fk = orc.compliance_sens(nx, ny, nz, KE, Uk, xpn)[0]
    m = min(len(hk), len(ho))
    # measured (32 x 16 x 16, 5 iterations / 64 x 32 x 32, 11): history 5.4e-12 / 7.1e-12 (first ten and whole), U 1.1e-13 /
    # 2.9e-12, fx 4.5e-13 / 8.8e-12, dfdx 2.1e-14 / 8.4e-13 of max |dfdx|
    assert np.abs(hg[:k] / ho[:k] - 1).max() <= 1e-10
    assert np.abs(hg / ho - 1).max() <= 1e-10
    assert rel(U, Uo) <= 3e-11
    assert abs(fx / fo - 1) <= 1e-10
    assert np.abs(dfn - dfo).max() <= 1e-11 * np.abs(dfo).max()
    # the operator's share: on the reference's KE the restatement moves by 1.8e-11 / 3.1e-11 (history) and 4.0e-13 / 8.9e-12 (fx),
    # and the library is as close to it: 2.4e-11 / 2.9e-11 (history), 4.6e-14 / 1.8e-13 (fx) -- the double restatement's own
    # rounding of these products, not the operators, sets the gaps
    assert its_k == its
    assert np.abs(ho[:m] / hk[:m] - 1).max() <= 1e-10
    assert np.abs(hg[:m] / hk[:m] - 1).max() <= 1e-10
    assert abs(fx / fk - 1) <= 1e-11
    grid.close()
