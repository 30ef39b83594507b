"""Stress constraint: the von Mises p-norm kernels (tp_elasticity_stress) against a numpy restatement in 80-bit arithmetic,
the adjoint load against finite differences of the device's own p-norm, the whole sensitivity against a sparse direct solve,
and the driver with the p-norm as a second MMA constraint.

    eps_e = B0 u_e,  sigma_e = Emax x_e^q C eps_e,  M = B0^T C^T Vm C B0,  s_e = u_e^T M u_e,  vm_e = Emax x_e^q sqrt(s_e)
    pnorm = (sum_e vm_e^P)^(1/P),  dpdx_e = pnorm^(1-P) q Emax^P x_e^(qP-1) s_e^(P/2)
    adj_rhs = sum_e pnorm^(1-P) (Emax x_e^q)^P s_e^((P-2)/2) L_e^T M u_e
    K lam = N adj_rhs,  d pnorm / dx_e = dpdx_e - p x_e^(p-1) (Emax - Emin) lam_e^T KE u_e

Bounds: 600 fused multiply-adds per element at 2^-53 each on O(1) data are about 7e-14, a decade for cancellation and pow gives
1e-12 (the argument of tests/test_gpu_loadcases.py); forming vm^P multiplies the relative error by P <= 8: 1e-11 for dpdx and
adj_rhs.  Every figure is printed with its bound before it is asserted.

The numpy restatement itself was held to central differences on the CPU (eps 1e-6, both meshes, all three (q, P)):
adj . W to 1.3e-11 ... 1.0e-10 relative, dpdx at an element to 1e-8.
"""
import numpy as np
import pytest

from tests.stress_ref import EMAX, LD, NU, elem_dofs, stress_ref, vonmises_form     # the 80-bit restatement

pytestmark = pytest.mark.gpu

# (elements, h): 1024 elements, cubic; 1920: no multiple of the workgroup (256), not tile-aligned, hx != hy != hz
MESHES = [((16, 8, 8), (0.125, 0.125, 0.125)), ((20, 12, 8), (0.05, 0.04, 0.03))]
QP = [(0.0, 2.0), (0.5, 2.0), (0.5, 8.0)]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _check(label, got, bound):
    print("%-66s measured %.3e   bound %.1e" % (label, got, bound))
    assert got <= bound, (label, got, bound)


_CACHE = {}


def _case(tp, idx):
    """per mesh, computed once and left alone: grid, solver object, synthetic density, a random state and numpy's M"""
    if idx in _CACHE:
        return _CACHE[idx]
    (ex, ey, ez), h = MESHES[idx]
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=3, nu=NU))
    xp = grid.synth_density()
    rng = np.random.default_rng(300 + ex)
    U = rng.uniform(-1.0, 1.0, 3 * (ex + 1) * (ey + 1) * (ez + 1))
    c = dict(grid=grid, le=le, xp=xp, xo=xp.cpu().numpy().copy(), U=U, Ud=_dev(U), M=vonmises_form(h), dofs=elem_dofs(ex, ey, ez),
             nel=ex * ey * ez, nnode=(ex + 1) * (ey + 1) * (ez + 1), tag="%dx%dx%d" % (ex, ey, ez), ref={})
    _CACHE[idx] = c
    return c


def _ref(c, q, P):
    if (q, P) not in c["ref"]:
        c["ref"][(q, P)] = stress_ref(c["M"], c["dofs"], c["U"], c["xo"], q, P)
    return c["ref"][(q, P)]


def _full_call(c, q, P, U=None, xp=None):
    g, le = c["grid"], c["le"]
    vm, dpdx, adj = g.elem_vec(), g.elem_vec(), g.node_vec(3)
    pn, mx = le.Stress(c["xp"] if xp is None else xp, EMAX, q, P, U=c["Ud"] if U is None else U, vm=vm, dpdx=dpdx, adj_rhs=adj)
    return pn, mx, vm.cpu().numpy(), dpdx.cpu().numpy(), adj.cpu().numpy()


# ---- 1
@pytest.mark.parametrize("idx", [0, 1])
def test_von_mises_form(tp, idx):
    c = _case(tp, idx)
    M = c["le"].StressForm().reshape(24, 24)
    Mr = c["M"]
    top = float(np.abs(Mr).max())
    _check("%s max|M - M_numpy| / max|M|" % c["tag"], float(np.abs(M - Mr).max()) / top, 1e-14)
    _check("%s max|M - M^T| / max|M|" % c["tag"], float(np.abs(M - M.T).max()) / top, 1e-14)
    for comp in range(3):
        t = np.zeros(24)
        t[comp::3] = 1.0
        _check("%s max|M translation_%d| / max|M|" % (c["tag"], comp), float(np.abs(M @ t).max()) / top, 1e-13)


# ---- 2
@pytest.mark.parametrize("q,P", QP)
@pytest.mark.parametrize("idx", [0, 1])
def test_element_pass(tp, idx, q, P):
    c = _case(tp, idx)
    r = _ref(c, q, P)
    pn, mx, vm, _, _ = _full_call(c, q, P)
    tag = "%s q=%g P=%g" % (c["tag"], q, P)
    _check("%s max|vm - vm_ref| / max|vm_ref|" % tag, float(np.abs(vm - r["vm"]).max() / r["vm_max"]), 1e-12)
    print("%s vm_max %.17g, max of the device's vm %.17g" % (tag, mx, vm.max()))
    assert mx == vm.max()
    _check("%s |pnorm / pnorm_ref - 1|" % tag, abs(float(pn / r["pnorm"] - 1)), 1e-12)
    # pnorm and vm_max alone: the same numbers
    assert c["le"].Stress(c["xp"], EMAX, q, P, U=c["Ud"]) == (pn, mx)


# ---- 3
@pytest.mark.parametrize("q,P", [(0.5, 8.0), (0.5, 2.0)])
@pytest.mark.parametrize("idx", [0, 1])
def test_sensitivity_ingredients(tp, idx, q, P):
    c = _case(tp, idx)
    r = _ref(c, q, P)
    _, _, _, dpdx, adj = _full_call(c, q, P)
    tag = "%s q=%g P=%g" % (c["tag"], q, P)
    _check("%s max|dpdx - ref| / max|ref|" % tag, float(np.abs(dpdx - r["dpdx"]).max() / np.abs(r["dpdx"]).max()), 1e-11)
    _check("%s max|adj_rhs - ref| / max|ref|" % tag, float(np.abs(adj - r["adj"]).max() / np.abs(r["adj"]).max()), 1e-11)
    # dpdx or adj_rhs alone: the same bits as in the full call
    g, le = c["grid"], c["le"]
    d1, a1 = g.elem_vec(), g.node_vec(3)
    le.Stress(c["xp"], EMAX, q, P, U=c["Ud"], dpdx=d1)
    le.Stress(c["xp"], EMAX, q, P, U=c["Ud"], adj_rhs=a1)
    assert np.array_equal(d1.cpu().numpy(), dpdx) and np.array_equal(a1.cpu().numpy(), adj)


# ---- 4
@pytest.mark.parametrize("idx", [0, 1])
def test_adjoint_load_against_finite_differences_of_the_device_pnorm(tp, idx):
    """adj_rhs . W against (pnorm(U + eps W) - pnorm(U - eps W)) / 2 eps, eps = 1e-6, all three evaluations on the device.
    Truncation O(eps^2), cancellation about 1e-12 / eps; bound 1e-6 relative."""
    c = _case(tp, idx)
    q, P, eps = 0.5, 8.0, 1e-6
    W = np.random.default_rng(77 + idx).uniform(-1.0, 1.0, c["U"].size)
    _, _, _, _, adj = _full_call(c, q, P)
    le = c["le"]
    pp, _ = le.Stress(c["xp"], EMAX, q, P, U=_dev(c["U"] + eps * W))
    pm, _ = le.Stress(c["xp"], EMAX, q, P, U=_dev(c["U"] - eps * W))
    fd = (pp - pm) / (2 * eps)
    an = float(np.dot(adj.astype(LD), W.astype(LD)))
    print("%s adj_rhs . W = %.12e, central difference %.12e" % (c["tag"], an, fd))
    _check("%s |adj_rhs . W / fd - 1|" % c["tag"], abs(an / fd - 1), 1e-6)


# ---- 5
def _rigid_lower_half(c):
    (ex, ey, ez), _ = MESHES[0]
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    U = c["U"].copy().reshape(nz, ny, nx, 3)
    U[: nz // 2 + 1] = np.array([0.3, -0.7, 0.11])       # planes 0 .. nz/2: the element layers 0 .. nz/2 - 1 do not strain
    rigid = np.zeros((ez, ey, ex), dtype=bool)
    rigid[: nz // 2] = True
    return U.reshape(-1), rigid.reshape(-1)


@pytest.mark.parametrize("q,P", [(0.5, 8.0), (0.5, 2.0), (0.0, 2.0)])
def test_degenerate_rigid_translation(tp, q, P):
    """a rigid translation on the lower planes, random above: finite everywhere, and exactly zero where s_e = 0 -- vm and
    dpdx of those elements, and adj_rhs at the nodes all of whose elements are such"""
    c = _case(tp, 0)
    U, rigid = _rigid_lower_half(c)
    pn, mx, vm, dpdx, adj = _full_call(c, q, P, U=_dev(U))
    assert np.isfinite(pn) and np.isfinite(mx) and pn > 0
    for a in (vm, dpdx, adj):
        assert np.isfinite(a).all()
    assert not vm[rigid].any() and not dpdx[rigid].any() and vm[~rigid].min() > 0
    touched = np.zeros(c["nnode"] * 3, dtype=bool)
    touched[c["dofs"][~rigid].ravel()] = True              # dofs of nodes with at least one straining element
    assert not adj[~touched].any() and (~touched).sum() > 0
    r = stress_ref(c["M"], c["dofs"], U, c["xo"], q, P, relative=True)
    _check("rigid half q=%g P=%g max|vm - ref| / max" % (q, P), float(np.abs(vm - r["vm"]).max() / r["vm_max"]), 1e-12)
    _check("rigid half q=%g P=%g max|adj - ref| / max" % (q, P), float(np.abs(adj - r["adj"]).max() / np.abs(r["adj"]).max()), 1e-11)


@pytest.mark.parametrize("q,P", [(0.5, 8.0), (0.5, 2.0), (0.125, 8.0)])
def test_degenerate_zero_density(tp, q, P):
    """some x_e exactly 0 (q P > 1, and q P = 1 where x^(qP-1) = 0^0 = 1): finite, vm = 0 there, and no contribution to adj_rhs"""
    c = _case(tp, 0)
    xo = c["xo"].copy()
    zero = np.zeros(c["nel"], dtype=bool)
    zero[::7] = True
    xo[zero] = 0.0
    pn, mx, vm, dpdx, adj = _full_call(c, q, P, xp=_dev(xo))
    for a in (vm, dpdx, adj, np.array([pn, mx])):
        assert np.isfinite(a).all()
    assert not vm[zero].any()
    if q * P > 1:
        assert not dpdx[zero].any()
    r = stress_ref(c["M"], c["dofs"], c["U"], xo, q, P)
    _check("x = 0 q=%g P=%g max|dpdx - ref| / max" % (q, P), float(np.abs(dpdx - r["dpdx"]).max() / np.abs(r["dpdx"]).max()), 1e-11)
    _check("x = 0 q=%g P=%g max|adj - ref| / max" % (q, P), float(np.abs(adj - r["adj"]).max() / np.abs(r["adj"]).max()), 1e-11)


def test_degenerate_zero_state_and_bad_arguments(tp):
    c = _case(tp, 0)
    g, le = c["grid"], c["le"]
    import torch
    for q, P in QP:
        vm, dpdx, adj = g.elem_vec(1.0), g.elem_vec(1.0), torch.ones_like(c["Ud"])
        pn, mx = le.Stress(c["xp"], EMAX, q, P, U=g.node_vec(3), vm=vm, dpdx=dpdx, adj_rhs=adj)
        assert pn == 0.0 and mx == 0.0
        assert not vm.any() and not dpdx.any() and not adj.any()
    # the whole sensitivity on the zero state: no adjoint solve, lam and dsdx all zeros
    assert not le.U.any()
    dsdx = g.elem_vec(1.0)
    assert le.StressSensitivity(dsdx, c["xp"], 1e-9, EMAX, 3.0, 0.5, 8.0) == (0.0, 0.0, 0)
    assert not dsdx.any() and not le.lam.any() and le.adjoint_its == 0
    for q, P in [(0.5, 1.0), (-0.1, 8.0), (0.05, 8.0)]:
        with pytest.raises(tp.api.TopOptError, match="TP_ERR_ARG"):
            le.Stress(c["xp"], EMAX, q, P, U=c["Ud"])


# ---- 6
@pytest.mark.parametrize("idx", [0, 1])
def test_only_vm_is_one_launch_and_the_same_bits(tp, idx):
    c = _case(tp, idx)
    g, le = c["grid"], c["le"]
    _, _, vm_full, _, _ = _full_call(c, 0.5, 8.0)
    vm = g.elem_vec()
    le.pop_stats()
    assert le.Stress(c["xp"], EMAX, 0.5, 8.0, U=c["Ud"], vm=vm) == (None, None)
    launches = le.pop_stats()[2]
    print("%s launches of the vm-only call: %d" % (c["tag"], launches))
    assert launches == 1
    assert np.array_equal(vm.cpu().numpy(), vm_full)


# ---- 7
def _assemble(dofs, KE, E, n):
    import scipy.sparse as sp
    rows = np.repeat(dofs, 24, axis=1).ravel()
    cols = np.tile(dofs, (1, 24)).ravel()
    vals = (E[:, None] * KE.ravel()[None, :]).ravel()
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def _solver(dofs, KE, E, Nv):
    """-> solve(b) for (N K N + I - N) y = N b"""
    n = Nv.size
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        D = sp.diags(Nv)
        A = (D @ _assemble(dofs, KE, E, n) @ D + sp.diags(1.0 - Nv)).tocsc()
        lu = spl.splu(A)
        return lambda b: lu.solve(Nv * b)
    except ImportError:                                    # dense fall-back
        K = np.zeros((n, n))
        for e in range(dofs.shape[0]):
            K[np.ix_(dofs[e], dofs[e])] += E[e] * KE
        A = Nv[:, None] * K * Nv[None, :] + np.diag(1.0 - Nv)
        return lambda b: np.linalg.solve(A, Nv * b)


def test_whole_sensitivity_against_a_direct_solve(tp):
    """StressSensitivity's dsdx on the 16x8x8 cantilever against the same formulas in numpy with both systems solved directly.
    dsdx is bilinear in (u, lam) and one solver produces both at one tolerance: with delta_u the measured relative error of the
    state, the bound is max(100 delta_u, 1e-10).  The reference's own dsdx is held to central differences first."""
    (ex, ey, ez), h = MESHES[0]
    Emin, Emax, penal, q, P = 1e-3, 1.0, 3.0, 0.5, 8.0
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=3, nu=NU, rtol=1e-12))
    le.SetUpLoadAndBC()
    xp = grid.synth_density()
    dsdx = grid.elem_vec()
    le.AssembleStiffnessMatrix(xp, Emin, Emax, penal)
    its_u = le.KSPSolve()
    rec = (le.last_its, le.last_rnorm, le.last_bnorm, list(le.case_its))
    pn, mx, its = le.StressSensitivity(dsdx, xp, Emin, Emax, penal, q, P)
    assert its > 0 and le.adjoint_its == its and le.adjoint_bnorm > 0
    print("adjoint solve: %d iterations, rnorm / bnorm %.3e" % (its, le.adjoint_rnorm / le.adjoint_bnorm))
    assert rec == (le.last_its, le.last_rnorm, le.last_bnorm, list(le.case_its)) and rec[0] == its_u   # the state's records stay
    # reference
    x, Nv, R = xp.cpu().numpy(), le.N.cpu().numpy(), le.RHS.cpu().numpy()
    KE, M, dofs = le.KE.reshape(24, 24), vonmises_form(h), elem_dofs(ex, ey, ez)

    def pnorm_of(xv):
        u = _solver(dofs, KE, Emin + xv ** penal * (Emax - Emin), Nv)(R)
        return float(stress_ref(M, dofs, u, xv, q, P)["pnorm"]), u

    solve = _solver(dofs, KE, Emin + x ** penal * (Emax - Emin), Nv)
    u = solve(R)
    r = stress_ref(M, dofs, u, x, q, P)
    lam = solve(np.asarray(r["adj"], dtype=np.float64))
    lKu = np.einsum("er,rc,ec->e", lam[dofs].astype(LD), KE.astype(LD), u[dofs].astype(LD))
    ref = np.asarray(r["dpdx"] - penal * x.astype(LD) ** (penal - 1) * (Emax - Emin) * lKu, dtype=np.float64)
    top = float(np.abs(ref).max())
    print("adjoint term / explicit term (max norms): %.3f" % (float(np.abs(ref - np.asarray(r["dpdx"], dtype=np.float64)).max())
                                                            / float(np.abs(r["dpdx"]).max())))
    for e in (int(np.argmax(np.abs(ref))), 5, ex * ey * (ez // 2) + ex * (ey // 2) + ex // 2):
        d = 1e-6
        xa, xb = x.copy(), x.copy()
        xa[e] += d
        xb[e] -= d
        fd = (pnorm_of(xa)[0] - pnorm_of(xb)[0]) / (2 * d)
        _check("reference dsdx[%d] = %.6e against central differences, / max|dsdx|" % (e, ref[e]), abs(ref[e] - fd) / top, 1e-6)
    Ud = le.U.cpu().numpy()
    du = float(np.abs(Ud - u).max() / np.abs(u).max())
    print("delta_u = max|U_dev - U_ref| / max|U_ref| = %.3e; state its %d, adjoint its %d" % (du, its_u, its))
    _check("|pnorm / pnorm_ref - 1|", abs(pn / float(r["pnorm"]) - 1), max(100 * du, 1e-10))
    _check("max|dsdx_dev - dsdx_ref| / max|dsdx_ref|", float(np.abs(dsdx.cpu().numpy() - ref).max()) / top, max(100 * du, 1e-10))
    grid.close()


# ---- 8
def test_driver_with_a_stress_limit(tp):
    import torch
    kw = dict(nxyz=(33, 17, 17), nlvls=3)
    probe = tp.TopOpt(stress_limit=1.0, **kw)
    L = 0.8 * probe.step()["stress_pnorm"]
    probe.grid.close()
    assert L > 0
    opt = tp.TopOpt(stress_limit=L, **kw)
    rec = opt.step()
    assert opt.m == 2 and len(opt.dgdx) == 2
    for k in ("stress_pnorm", "stress_max", "gx_stress"):
        assert np.isfinite(rec[k])
    assert rec["gx_stress"] == rec["stress_pnorm"] / L - 1.0 and rec["ksp_its_adjoint"] > 0
    assert rec["gx_stress"] == pytest.approx(0.25, rel=1e-9)
    assert rec["ksp_its"] == opt.physics.last_its and opt.physics.adjoint_its == rec["ksp_its_adjoint"]
    # the same step from the public pieces
    nx, ny, nz = kw["nxyz"]
    h = (2.0 / (nx - 1), 1.0 / (ny - 1), 1.0 / (nz - 1))
    g = tp.Grid(nx, ny, nz, h)
    le = tp.LinearElasticity(g, tp.SolverOptions(nlvls=3, nu=0.3))
    le.SetUpLoadAndBC()
    flt = tp.Filter(g, 1, 0.08)
    x, xt, xp = g.elem_vec(0.12), g.elem_vec(0.12), g.elem_vec(0.12)
    df, dg = g.elem_vec(), [g.elem_vec(), g.elem_vec()]
    xmin, xmax = g.elem_vec(), g.elem_vec()
    mma = tp.MMA(g, x, 2)
    flt.FilterProject(x, xt, xp, False, 0.1, 0.0)
    fx, gx = le.ComputeObjectiveConstraintsSensitivities(df, dg[0], xp, 1e-9, 1.0, 3.0, 0.12)
    df.mul_(10.0 / fx)
    pn, mx, its = le.StressSensitivity(dg[1], xp, 1e-9, 1.0, 3.0, 0.5, 8.0)
    dg[1].div_(L)
    flt.Gradients(x, xt, df, dg, False, 0.1, 0.0)
    mma.SetOuterMovelimit(0.0, 1.0, 0.2, x, xmin, xmax)
    mma.Update(x, df, [gx, pn / L - 1.0], dg, xmin, xmax)
    assert (fx, gx, pn, mx, its) == (rec["fx"], rec["gx"], rec["stress_pnorm"], rec["stress_max"], rec["ksp_its_adjoint"])
    assert torch.equal(x, opt.x), "the driver's step differs from the step composed by hand"
    g.close()
    # ten iterations: printed, not asserted
    for _ in range(9):
        rec = opt.step()
    print("gx_stress over ten iterations: " + " ".join("%.4f" % r["gx_stress"] for r in opt.history))
    print("gx (volume) over ten iterations: " + " ".join("%.4f" % r["gx"] for r in opt.history))
    print("adjoint iterations: " + " ".join("%d" % r["ksp_its_adjoint"] for r in opt.history))
    opt.grid.close()
    # no limit: nothing of it in the record, one constraint
    plain = tp.TopOpt(**kw)
    rp = plain.step()
    assert plain.m == 1 and len(plain.dgdx) == 1 and plain.physics.lam is None
    assert not [k for k in rp if "stress" in k or "adjoint" in k]
    plain.grid.close()
