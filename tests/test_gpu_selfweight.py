"""Self-weight: the body load and its sensitivity term (tp_elasticity_body_load, tp_elasticity_body_sensitivity) against the
80-bit numpy restatement tests/selfweight_ref.py, the whole compliance derivative against a sparse direct solve, the stress
p-norm's derivative with the moving load against central differences of the device's own p-norm, and the driver.

Bounds.  Load: <= 8 additions, 2 multiplications and the 6-operation polynomial at 2^-53 each are about 2e-15 of max|f|; two
decades of margin: 1e-13.  Sensitivity term: 24 ncase + 6 operations at 2^-53, at most 2.2e-14 of max|term| for 8 fields; a decade:
1e-13 (the pre-filled dfdx is of the term's own size, its addition is one of the operations).  Whole derivative: bilinear in the
state, which one solver delivers at one tolerance -- max(100 delta_u, 1e-10) of max|dfdx| (the rule of tests/test_gpu_stress.py).
Every figure is printed with its bound before it is asserted."""
import numpy as np
import pytest

from tests import selfweight_ref as ref

pytestmark = pytest.mark.gpu

LD = ref.LD
NU = 0.3
MESHES = [((16, 8, 8), (0.125, 0.125, 0.125)), ((20, 12, 8), (0.05, 0.04, 0.03))]   # those of tests/test_gpu_stress.py
B = (0.3, -0.7, 1.1)
FIELDS = ["random", "halflow", "zeros", "ones"]
WEIGHTS = [0.75, -0.5, 0.0, 1.0, 0.3, -1.2, 2.0, 0.1]


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _check(label, got, bound):
    print("%-78s measured %.3e   bound %.1e" % (label, got, bound))
    assert got <= bound, (label, got, bound)


def field(kind, nel, seed=0):
    rng = np.random.default_rng(500 + seed)
    if kind == "random":
        return rng.uniform(0.0, 1.0, nel)
    if kind == "halflow":                      # every other element below x_low = 0.1
        x = rng.uniform(0.1, 1.0, nel)
        x[::2] = rng.uniform(0.0, 0.1, x[::2].size)
        return x
    return np.zeros(nel) if kind == "zeros" else np.ones(nel)


_CACHE = {}


def _case(tp, idx):
    """per mesh, made once and left alone: grid, solver object with the cantilever's supports, numpy's dofs, N, random fields"""
    if idx in _CACHE:
        return _CACHE[idx]
    (ex, ey, ez), h = MESHES[idx]
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=3, nu=NU))
    le.SetUpLoadAndBC()
    nnode = (ex + 1) * (ey + 1) * (ez + 1)
    rng = np.random.default_rng(700 + ex)
    V = [rng.uniform(-1.0, 1.0, 3 * nnode) for _ in range(tp.lib.MAX_CASES)]      # do NOT vanish on the supports
    c = dict(grid=grid, le=le, h=h, dofs=ref.elem_dofs(ex, ey, ez), nel=ex * ey * ez, nnode=nnode, N=le.N.cpu().numpy(), V=V,
             Vd=[_dev(v) for v in V], tag="%dx%dx%d" % (ex, ey, ez))
    assert (c["N"] == 0).any()
    _CACHE[idx] = c
    return c


# ---- 1
@pytest.mark.parametrize("x_low", [0.0, 0.1])
@pytest.mark.parametrize("idx", [0, 1])
def test_load_against_the_restatement(tp, idx, x_low):
    import torch
    c = _case(tp, idx)
    g, le = c["grid"], c["le"]
    le.SetBodyForce(B, x_low)
    vol = ref.volume(c["h"])
    for kind in FIELDS:
        x = field(kind, c["nel"], idx)
        xd = _dev(x)
        fr = ref.load(x, c["dofs"], c["nnode"], c["h"], B, x_low)
        top = float(np.abs(fr).max())
        tag = "%s x_low %.1f %s" % (c["tag"], x_low, kind)
        f = g.node_vec(3)
        f.fill_(7.0)                                  # (every owned entry is written)
        le.BodyLoad(xd, f)
        fh = f.cpu().numpy()
        if top == 0.0:
            print("%s: max|f| = %.1e (all zero asked for)" % (tag, np.abs(fh).max()))
            assert not fh.any()
        else:
            _check("%s max|f - f_ref| / max|f_ref|" % tag, float(np.abs(fh - fr).max()) / top, 1e-13)
            tot = vol * ref.mass(x, x_low).sum()
            for comp in range(3):
                s = fh.astype(LD)[comp::3].sum()
                _check("%s |sum_n f_%d / (V b_%d sum m) - 1|" % (tag, comp, comp), float(abs(s / (tot * LD(B[comp])) - 1)), 1e-12)
        # with a base of the load's own size, out of place and in place
        base = np.random.default_rng(9).uniform(-1.0, 1.0, fr.size) * (top if top else 1e-3)
        bd = _dev(base)
        out = g.node_vec(3)
        le.BodyLoad(xd, out, base=bd)
        oh = out.cpu().numpy()
        assert np.array_equal(bd.cpu().numpy(), base), "the base array was written to"
        if top == 0.0:
            assert np.array_equal(oh, base)
        else:
            _check("%s max|out - (base + f_ref)| / max|f_ref|" % tag, float(np.abs(oh - (base.astype(LD) + fr)).max()) / top, 1e-13)
        inpl = bd.clone()
        le.BodyLoad(xd, inpl, base=inpl)
        assert torch.equal(inpl, out), "%s: rhs == rhs_base gives other bits than the call out of place" % tag
    le.SetBodyForce(None)


# ---- 2
@pytest.mark.parametrize("x_low", [0.0, 0.1])
@pytest.mark.parametrize("idx", [0, 1])
def test_sensitivity_term_against_the_restatement(tp, idx, x_low):
    c = _case(tp, idx)
    g, le = c["grid"], c["le"]
    le.SetBodyForce(B, x_low)
    for kind in ("random", "halflow"):
        x = field(kind, c["nel"], idx)
        xd = _dev(x)
        per_field = [ref.sens_term(x, c["dofs"], c["h"], B, x_low, c["N"], v) for v in c["V"]]
        no_N = ref.sens_term(x, c["dofs"], c["h"], B, x_low, np.ones_like(c["N"]), c["V"][0])
        assert float(np.abs(no_N - per_field[0]).max()) > 1e-3 * float(np.abs(per_field[0]).max())   # a missing N would show
        for ncase in (1, 2, tp.lib.MAX_CASES):
            for scale in (1.0, 2.0):
                for w in ((None, WEIGHTS[:ncase]) if ncase == 1 else (WEIGHTS[:ncase],)):
                    wv = [1.0] * ncase if w is None else w
                    term = LD(scale) * sum(LD(wl) * t for wl, t in zip(wv, per_field))
                    top = float(np.abs(term).max())
                    pre = np.random.default_rng(ncase).uniform(-1.0, 1.0, c["nel"]) * top
                    d = _dev(pre)
                    le.BodySensitivity(c["Vd"][:ncase], w, xd, scale, d)
                    err = float(np.abs(d.cpu().numpy() - (pre.astype(LD) + term)).max()) / top
                    _check("%s x_low %.1f %s ncase %d scale %g%s max|dfdx - (pre + term)| / max|term|"
                           % (c["tag"], x_low, kind, ncase, scale, " w=None" if w is None else ""), err, 1e-13)
    if x_low > 0:     # m'(0) = 0: exactly nothing is added, and no NaN
        pre = np.random.default_rng(1).uniform(-1.0, 1.0, c["nel"])
        d = _dev(pre)
        le.BodySensitivity(c["Vd"][:2], WEIGHTS[:2], g.elem_vec(0.0), 2.0, d)
        assert np.array_equal(d.cpu().numpy(), pre)
    else:             # x_low = 0: m' = 1 also at x = 0
        d = g.elem_vec(0.0)
        le.BodySensitivity(c["Vd"][:1], None, g.elem_vec(0.0), 1.0, d)
        t0 = ref.sens_term(np.zeros(c["nel"]), c["dofs"], c["h"], B, 0.0, c["N"], c["V"][0])
        _check("%s x_low 0 at x = 0 max|dfdx - term| / max|term|" % c["tag"], float(np.abs(d.cpu().numpy() - t0).max() / np.abs(t0).max()), 1e-13)
    le.SetBodyForce(None)


# ---- 3
def _solver(ne, KE, E, Nv):
    """-> solve(b) for (N K N + I - N) y = N b, sparse direct (tests/scipy_check.py)"""
    from tests import scipy_check as sc
    import scipy.sparse.linalg as spl
    lu = spl.splu(sc.assemble(ne[0], ne[1], ne[2], KE, E=E, N=Nv).tocsc())
    return lambda b: lu.solve(Nv * b)


X_LOW3 = 0.3      # tests 3 and 4: x in [0.2, 0.9], so a seventh of the elements lies in the damped range


@pytest.mark.parametrize("two_cases", [False, True])
def test_whole_derivative_against_a_direct_solve(tp, two_cases):
    """ComputeObjectiveConstraintsSensitivities with SetBodyForce on the 16x8x8 cantilever (Emin 1e-3, rtol 1e-12, random x in
    [0.2, 0.9]; one case, and two with the weights (1, 0.5)) against the restatement evaluated on a sparse direct solve of the
    same system: fx = sum_l w_l (F_l + f)^T u_l and dfdx, both to max(100 delta_u, 1e-10)"""
    (ex, ey, ez), h = MESHES[0]
    Emin, Emax, penal, volfrac = 1e-3, 1.0, 3.0, 0.5
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=3, nu=NU, rtol=1e-12))
    le.SetUpLoadAndBC()
    if two_cases:
        le.SetUpLoadAndBC_Top(0.5)
    le.SetBodyForce(B, X_LOW3)
    x = np.random.default_rng(41).uniform(0.2, 0.9, ex * ey * ez)
    xd, dfdx, dgdx = _dev(x), grid.elem_vec(), grid.elem_vec()
    fixed = [le.LoadCaseRHS(l).clone() for l in range(le.ncases)]
    fx, gx = le.ComputeObjectiveConstraintsSensitivities(dfdx, dgdx, xd, Emin, Emax, penal, volfrac)
    for l in range(le.ncases):
        assert (le.LoadCaseRHS(l) == fixed[l]).all(), "the fixed load of case %d was changed" % l
    # the same from the formulas, with a direct solve
    Nv, KE, dofs = le.N.cpu().numpy(), le.KE.reshape(24, 24), ref.elem_dofs(ex, ey, ez)
    fb = np.asarray(ref.load(x, dofs, (ex + 1) * (ey + 1) * (ez + 1), h, B, X_LOW3), dtype=np.float64)
    solve = _solver((ex, ey, ez), KE, Emin + x ** penal * (Emax - Emin), Nv)
    fx_ref, dref, du, cl_top, bo_top = LD(0), 0, 0.0, 0.0, 0.0
    for l in range(le.ncases):
        F = fixed[l].cpu().numpy() + fb
        u = solve(F)
        w = LD(le.case_weight[l])
        fx_ref += w * np.dot((Nv * F).astype(LD), u.astype(LD))
        dc, classical, body = ref.dcdx(x, dofs, h, B, X_LOW3, Nv, KE, u, Emin, Emax, penal)
        dref = dref + w * dc
        cl_top, bo_top = max(cl_top, float(np.abs(classical).max())), max(bo_top, float(np.abs(body).max()))
        du = max(du, float(np.abs(le.LoadCaseU(l).cpu().numpy() - u).max() / np.abs(u).max()))
        assert np.array_equal(le.TotalRHS(l).cpu().numpy(), F) or float(np.abs(le.TotalRHS(l).cpu().numpy() - F).max()) <= 1e-13 * np.abs(F).max()
    top = float(np.abs(dref).max())
    bound = max(100 * du, 1e-10)
    print("%d case(s): delta_u = %.3e, CG iterations %s; max|self-weight term| / max|classical term| = %.3f; dfdx from %.3e to %.3e"
          % (le.ncases, du, le.case_its, bo_top / cl_top, float(dref.min()), float(dref.max())))
    _check("%d case(s) |fx / ((F + f)^T u) - 1|" % le.ncases, float(abs(fx / fx_ref - 1)), bound)
    _check("%d case(s) max|dfdx_dev - dfdx_ref| / max|dfdx_ref|" % le.ncases, float(np.abs(dfdx.cpu().numpy() - dref).max()) / top, bound)
    # ComputeSensitivities on the state as it is: the same derivative
    d2 = grid.elem_vec()
    le.ComputeSensitivities(d2, dgdx, xd, Emin, Emax, penal)
    _check("%d case(s) ComputeSensitivities: max|dfdx - dfdx_ref| / max|dfdx_ref|" % le.ncases, float(np.abs(d2.cpu().numpy() - dref).max()) / top, bound)
    assert abs(gx - (x.mean() - volfrac)) <= 1e-14
    grid.close()


# ---- 4
def test_stress_derivative_with_self_weight_against_central_differences_of_the_device_pnorm(tp):
    """StressSensitivity's dsdx . W against (pnorm(x + eps W) - pnorm(x - eps W)) / 2 eps, eps = 1e-6, bound 1e-6 relative; every
    evaluation is a full assembly + body load + solve at rtol 1e-12 on the device.  The load moves with x, so the derivative needs
    + d(lam^T N f)/dx: the restatement with direct solves on the CPU (same mesh, x, W, b, x_low) puts that term at
    (term . W) / (dsdx . W) = 1.494e-2 (dsdx . W = -1.898107474e+01 there, its own central difference off by 4.6e-8; without the
    term off by 1.494e-2, four orders above the bound).  The test also takes the term out again on the device and sees the
    comparison fail."""
    (ex, ey, ez), h = MESHES[0]
    Emin, Emax, penal, q, P, eps = 1e-3, 1.0, 3.0, 0.5, 8.0, 1e-6
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=3, nu=NU, rtol=1e-12))
    le.SetUpLoadAndBC()
    le.SetBodyForce(B, X_LOW3)
    rng = np.random.default_rng(41)
    x = rng.uniform(0.2, 0.9, ex * ey * ez)
    W = rng.uniform(-1.0, 1.0, x.size)

    def pnorm_of(xv):
        xd = _dev(xv)
        le.SolveState(xd, Emin, Emax, penal)
        return le.Stress(xd, Emax, q, P)[0]

    xd, dsdx = _dev(x), grid.elem_vec()
    le.SolveState(xd, Emin, Emax, penal)
    pn, mx, its = le.StressSensitivity(dsdx, xd, Emin, Emax, penal, q, P)
    an = float(np.dot(dsdx.cpu().numpy().astype(LD), W.astype(LD)))
    without = dsdx.clone()
    le.BodySensitivity([le.lam], None, xd, -1.0, without)
    an0 = float(np.dot(without.cpu().numpy().astype(LD), W.astype(LD)))
    fd = (pnorm_of(x + eps * W) - pnorm_of(x - eps * W)) / (2 * eps)
    print("pnorm %.9e, adjoint iterations %d; dsdx . W = %.12e, central difference %.12e; without the load's term %.12e (the term is %.3e of the whole)"
          % (pn, its, an, fd, an0, (an - an0) / an))
    _check("|dsdx . W / fd - 1|", abs(an / fd - 1), 1e-6)
    assert abs(an0 / fd - 1) > 1e-6, "the comparison does not see the load's term"
    grid.close()


# ---- 5
def test_nothing_changes_when_off(tp):
    """three driver iterations with body_force=None and with body_force=(0, 0, 0): a zero load and a zero term added are exact"""
    import torch
    kw = dict(nxyz=(17, 9, 9), nlvls=3, rmin=0.2)
    runs = []
    for b in (None, (0.0, 0.0, 0.0)):
        opt = tp.TopOpt(body_force=b, **kw)
        hist = [opt.step() for _ in range(3)]
        runs.append((hist, opt.x.clone()))
        assert ("body_share" in hist[0]) == (b is not None)
        assert (opt.physics.body_force is None) == (b is None) and (b is not None or opt.physics._case_total == [])
        opt.grid.close()
    (h0, x0), (h1, x1) = runs
    for r0, r1 in zip(h0, h1):
        print("itr %d: fx %.17g / %.17g, gx %.17g / %.17g, ch %.17g / %.17g" % (r0["itr"], r0["fx"], r1["fx"], r0["gx"], r1["gx"], r0["ch"], r1["ch"]))
        assert (r0["fx"], r0["gx"], r0["ch"], r0["ksp_its"]) == (r1["fx"], r1["gx"], r1["ch"], r1["ksp_its"])
    assert torch.equal(x0, x1)


# ---- 6
def test_driver_with_gravity(tp):
    """32x16x16 on the 2 x 1 x 1 domain, ten iterations, gravity along -z.  The cantilever's line load is 0.001 on 17 nodes with
    half loads at the two ends: 0.016 in all.  The uniform start has the mass volfrac x volume = 0.12 x 2 (0.12 >= x_low: m = x), so
    |b| = 0.0667 gives the weight 0.016008."""
    kw = dict(nxyz=(33, 17, 17), nlvls=3)
    bz = -0.0667
    plain = tp.TopOpt(**kw)
    hp = [plain.step() for _ in range(10)]
    plain.grid.close()
    first_ok = next((k for k, r in enumerate(hp) if r["gx"] <= 1e-3), None)
    print("without a body force gx: " + " ".join("%.5f" % r["gx"] for r in hp))
    assert first_ok is not None
    for point_load in (True, False):
        opt = tp.TopOpt(body_force=(0.0, 0.0, bz), point_load=point_load, **kw)
        weight = abs(bz) * float(opt.xPrint.sum()) * (2.0 / 32) * (1.0 / 16) * (1.0 / 16)
        total_point = float(opt.physics.LoadCaseRHS(0).abs().sum())
        print("point_load %s: weight of the start %.6f, total point load %.6f" % (point_load, weight, total_point))
        assert abs(weight - 0.016008) < 1e-9 and total_point == pytest.approx(0.016 if point_load else 0.0, abs=1e-15)
        hist = []
        for k in range(10):
            hist.append(opt.step())
            if k == 0:
                df_max = float(opt.dfdx.max())
        print("point_load %s fx: %s" % (point_load, " ".join("%.4e" % r["fx"] for r in hist)))
        print("point_load %s gx: %s" % (point_load, " ".join("%.5f" % r["gx"] for r in hist)))
        print("point_load %s body_share: %s; max of the filtered dfdx in iteration 1: %.3e"
              % (point_load, " ".join("%.6f" % r["body_share"] for r in hist), df_max))
        for r in hist:
            assert all(np.isfinite(v) for v in r.values() if isinstance(v, float)), r
        assert all(r["gx"] <= 1e-3 for r in hist[first_ok:])
        if point_load:
            assert all(0.0 < r["body_share"] < 1.0 for r in hist)
        else:
            assert all(abs(r["body_share"] - 1.0) <= 1e-14 for r in hist)
            assert df_max > 0.0        # the cone filter's weights are positive: a positive filtered entry needs a positive raw one
        opt.grid.close()
