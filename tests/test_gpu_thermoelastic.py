"""Thermal expansion on the device, kernel by kernel against the 80-bit forms of tests/thermoelastic_ref.py, then
the coupled chain of the driver against direct solves of both state problems.

Per kernel, on the five one-level meshes and both designs, row by row within the constants of tests/thermoelastic_ref.py: beta
and beta' (k_thermal_coef, the device pow inside), the load alone, on a base and in place (the same bits), the adjoint right-hand
side and the sensitivity with one field and with three weighted ones, the sensitivity accumulated onto what dfdx held; the
transpose identity <N v, load(theta)> = <adjoint_rhs(v), theta> within the two chains' bounds; ThermalCoupling() against the
quadrature.  Coupled gradient: 16 x 8 x 8, three levels, rtol 1e-10, the driver's chain against the direct-solve gradient at
max(100 delta, 1e-10) of its maximum, delta the measured relative distance of the device states from the direct solves', both
thermal modes.  Driver: three design iterations on 8 x 8 x 4 against the same loop assembled from oracle pieces, all three
solves' iteration counts equal.  Every device figure is printed with its bound before it is asserted.

Achieved on the MI355X (recorded for the reader; the bounds come from tests/thermoelastic_ref.py), worst over the meshes and
designs: beta 3.4 and beta' 3.9 (bounds 64), load 4.2 (128), adjoint right-hand side 3.1 (64), sensitivity 1.5 (64), transpose
identity 1e-3 of its bound, G 0.90 (16); coupled gradient 3.8e-12 of its maximum with the states 7.2e-12 from the direct solves'
(bound 7.2e-10); driver: the design within 1.4e-14 of the reference loop's, iteration counts 10 / 6 / 6, 9 / 6 / 6, 9 / 6 / 6 on both
sides.  The 19 tests: 3.5 s.
"""
import numpy as np
import pytest

from tests import conduction_ref as cr
from tests import rowwise as rw
from tests import thermoelastic_ref as tr

pytestmark = pytest.mark.gpu
LD = np.longdouble
_REF = {}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def show(what, got, bound):
    print("%-84s %.4g (bound %.4g)" % (what, got, bound))
    return got


def held(got, ref, scale, c, label, dims, dof):
    show(label + ": achieved c", rw.achieved(got, ref, scale), c)
    return rw.assert_rowwise(got, ref, scale, c, {"label": label, "dims": dims, "dof": dof})


def reference(case, kind):
    """the case's data and its longdouble passes, made once"""
    def make():
        ne, h = case[:2]
        p, x = tr.par(kind), cr.design(kind, *ne)
        N, R = tr.cantilever(ne, h)
        T, v0, v1, v2 = tr.fields(ne, 1)
        w, base = [0.75, -0.5, 1.25], cr.design("mixed", *ne, seed=3) - 0.5
        out = dict(ne=ne, h=h, p=p, x=x, N=N, R=R, T=T, V=[v0, v1, v2], w=w, base=base, nd=(ne[0] + 1, ne[1] + 1, ne[2] + 1))
        out["beta"], out["dbeta"] = tr.beta(x, p, LD), tr.dbeta(x, p, LD)
        out["load"], out["load_s"] = tr.load(ne, h, x, T, p, dtype=LD), tr.load(ne, h, x, T, p, absolute=True)
        for key, Vl, wl in (("1", [v0], None), ("3", [v0, v1, v2], w)):
            out["adj" + key] = tr.adjoint_rhs(ne, h, x, Vl, wl, N, p, 1.5, dtype=LD)
            out["adj_s" + key] = tr.adjoint_rhs(ne, h, x, Vl, wl, N, p, 1.5, absolute=True)
            out["sens" + key] = tr.sensitivity(ne, h, x, Vl, wl, N, T, p, 2.0, dtype=LD)
            out["sens_s" + key] = tr.sensitivity(ne, h, x, Vl, wl, N, T, p, 2.0, absolute=True)
        return out
    return cached(("reference", case[:2], kind), make)


def device(tp, P):
    nx, ny, nz = P["nd"]
    grid = tp.Grid(nx, ny, nz, P["h"])
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
    le.SetBC(dev(P["N"]), dev(P["R"]))
    p = P["p"]
    le.SetThermalExpansion(p["alpha"], p["T_ref"], p["pb"], p["Emin"], p["Emax"])
    return grid, le


@pytest.mark.parametrize("kind", sorted(tr.DESIGNS))
@pytest.mark.parametrize("case", tr.FINE_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_kernels_row_by_row(tp, case, kind):
    import torch
    P = reference(case, kind)
    grid, le = device(tp, P)
    ne, nd, p = P["ne"], P["nd"], P["p"]
    tag = "%s %s" % (kind, ne)
    x, T, V = dev(P["x"]), dev(P["T"]), [dev(v) for v in P["V"]]
    assert (P["V"][0][P["N"] == 0] != 0).all() and p["T_ref"] != 0
    # ---- k_thermal_coef
    b, db = le.ThermalCoefficients(x)
    held(host(b), P["beta"], np.abs(P["beta"]).astype(np.float64), tr.C_BETA, tag + " beta", ne, 0)
    held(host(db), P["dbeta"], np.abs(P["dbeta"]).astype(np.float64), tr.C_DBETA, tag + " beta'", ne, 0)
    # ---- the load: alone, on a base, in place
    f = le.ThermalLoad(x, T, grid.node_vec(3).fill_(7.0))
    held(host(f), P["load"], P["load_s"], tr.C_LOAD, tag + " load", nd, 3)
    base = V[1].clone()
    fb = le.ThermalLoad(x, T, grid.node_vec(3).fill_(7.0), base=base)
    held(host(fb), P["V"][1].astype(LD) + P["load"], P["load_s"] + np.abs(P["V"][1]), tr.C_LOAD, tag + " load on a base", nd, 3)
    assert torch.equal(base, V[1])
    assert torch.equal(le.ThermalLoad(x, T, base, base=base), fb)                       # rhs == rhs_base
    # ---- the transpose and the sensitivity
    g1 = None
    for key, Vl, w in (("1", V[:1], None), ("3", V, P["w"])):
        g = le.ThermalAdjointRHS(Vl, w, x, 1.5, grid.node_vec(1).fill_(7.0))
        held(host(g), P["adj" + key], P["adj_s" + key], tr.C_ADJ, "%s adjoint rhs, %d fields" % (tag, len(Vl)), nd, 1)
        g1 = g if g1 is None else g1
        df = dev(P["base"])
        le.ThermalSensitivity(Vl, w, x, T, 2.0, df)                                     # accumulated, not overwritten
        held(host(df), P["base"].astype(LD) + P["sens" + key], P["sens_s" + key] + np.abs(P["base"]), tr.C_SENS,
             "%s sensitivity, %d fields" % (tag, len(Vl)), ne, 0)
    for v, orig in zip(V + [T, x], P["V"] + [P["T"], P["x"]]):
        assert np.array_equal(host(v), orig)                                           # the inputs are left as they were
    # ---- the transpose identity on the device's own vectors, inner products in longdouble on the host
    th = tr.theta(P["T"], p, LD)
    lhs = ((P["N"] * P["V"][0]).astype(LD) * host(f).astype(LD)).sum()
    rhs = (host(g1).astype(LD) / LD(1.5) * th).sum()
    major = float((np.abs(P["V"][0]) * P["load_s"]).sum())
    bound = (tr.C_LOAD + tr.C_ADJ + 1) * tr.EPS * major
    show(tag + " |<N v, load(theta)> - <adjoint_rhs(v), theta>|", float(abs(lhs - rhs)), bound)
    assert float(abs(lhs - rhs)) <= bound
    grid.close()


@pytest.mark.parametrize("case", tr.FINE_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_coupling_matrix(tp, case):
    ne, h = case[:2]
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
    G = le.ThermalCoupling().reshape(24, 8)
    gq = tr.G_quadrature(h)
    top = float(np.abs(gq).max())
    d = float(np.abs(G.astype(LD) - gq).max()) / (tr.EPS * top)
    show("h = %s: ThermalCoupling() against the quadrature, achieved c" % (h,), d, tr.C_G)
    assert d <= tr.C_G and np.array_equal(G, tr.G(h))
    grid.close()


def coupled_reference(orc, mode):
    """direct solves on the gradient case at alpha such that |f_th| = |F|"""
    def make():
        ne, h, nlv = tr.GRADIENT_CASE
        KE = np.asarray(orc.hex8_ke_box(h, h, h, tr.NU))
        x = cr.design("mixed", *ne)
        dT = 0.8 if mode == "uniform" else None
        unit = tr.Coupled(ne, h, KE, tr.par("mixed", alpha=1.0), mode, dT)
        s1 = unit.state(x)
        alpha = float(np.linalg.norm(unit.N * unit.F) / np.linalg.norm(unit.N * s1["f_th"]))
        cp = tr.Coupled(ne, h, KE, tr.par("mixed", alpha=alpha), mode, dT)
        s = cp.state(x)
        return cp, x, s, cp.gradient(x, s), alpha
    return cached(("coupled", mode), make)


@pytest.mark.parametrize("mode", ["conduction", "uniform"])
def test_coupled_gradient(tp, orc, mode):
    cp, x, s, G, alpha = coupled_reference(orc, mode)
    ne, h, nlv = tr.GRADIENT_CASE
    p = cp.p
    opt = tp.TopOpt(nxyz=(ne[0] + 1, ne[1] + 1, ne[2] + 1), xc=(0, ne[0] * h, 0, ne[1] * h, 0, ne[2] * h), nlvls=nlv, rmin=2.56 * h, filter=1,
                    volfrac=0.3, physics="thermoelastic", alpha=alpha, T_ref=p["T_ref"], thermal=mode, delta_T=cp.delta_T,
                    Emin=p["Emin"], kmin=cp.kmin, solver=tp.SolverOptions(nlvls=nlv, rtol=1e-10, max_it=200))
    assert opt.physics_kind == "thermoelastic" and isinstance(opt.physics, tp.api.LinearElasticity)
    assert np.array_equal(host(opt.physics.N), cp.N) and np.array_equal(host(opt.physics.RHS), cp.F)
    opt.xPhys.copy_(dev(x))
    fx, gx = opt._thermoelastic_step()
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    deltas = {"u": rel(host(opt.physics.U), s["u"])}
    if mode == "conduction":
        assert isinstance(opt.thermal, tp.api.HeatConduction) and opt._its_thermal > 0 and opt._its_thermal_adjoint > 0
        deltas["T"], deltas["mu"] = rel(host(opt.thermal.T), s["T"]), rel(host(opt.mu), G["mu"])
    else:   # no conduction handle exists and no adjoint solve is counted
        assert opt.thermal is None and opt._its_thermal == 0 and opt._its_thermal_adjoint == 0 and not hasattr(opt, "mu")
    delta = max(deltas.values())
    bound = max(100 * delta, 1e-10)
    d = float(np.abs(host(opt.dfdx) - G["dc"]).max() / np.abs(G["dc"]).max())
    print("%s: alpha %.4e, c %.12e (direct solves %.12e); iterations elastic %d, conduction %d, thermal adjoint %d; state distances %s"
          % (mode, alpha, fx, s["c"], opt.physics.last_its, opt._its_thermal, opt._its_thermal_adjoint, {k: "%.2e" % v for k, v in deltas.items()}))
    show(mode + ": max|dc/dx - direct-solve gradient| / max|gradient|", d, bound)
    assert d <= bound and abs(fx / s["c"] - 1) <= bound
    # without the new terms the gradient misses the bound
    assert float(np.abs(G["elastic"] - G["dc"]).max() / np.abs(G["dc"]).max()) > bound
    opt.grid.close()


def test_driver_three_design_iterations(tp, orc):
    """TopOpt(physics="thermoelastic") against the same loop assembled from oracle pieces: orc.MG solves of both problems and of
    the thermal adjoint at rtol 1e-10 (warm-started like the driver), the restated passes, orc.Filter, orc.MMA in device order.
    The design within 1e-9, the bound tests/test_gpu_conduction.py's driver test uses; all three iteration counts equal"""
    (ex, ey, ez), nlv, nit = tr.DRIVER_CASE
    ne = (ex, ey, ez)
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    vf, rmin, kmin, Emin, alpha, T_ref = 0.3, 2.56 / ey, 1e-3, 1e-9, 2e-4, 0.25
    opt = tp.TopOpt(nxyz=(nx, ny, nz), xc=(0, ex * h, 0, 1, 0, ez * h), nlvls=nlv, rmin=rmin, filter=1, volfrac=vf, physics="thermoelastic",
                    alpha=alpha, T_ref=T_ref, solver=tp.SolverOptions(nlvls=nlv, rtol=1e-10, max_it=200))
    p = dict(alpha=alpha, T_ref=T_ref, Emin=Emin, Emax=1.0, pb=3.0)
    KE = np.asarray(orc.hex8_ke_box(h, h, h, tr.NU))
    kt, NT = cr.KT(h), cr.sink_mask(nx, ny, nz)
    q = NT * cr.load(nx, ny, nz, h)
    N, F = orc.cantilever_bc(nx, ny, nz, h)
    assert np.array_equal(host(opt.physics.N), N) and np.array_equal(host(opt.physics.RHS), F) and np.array_equal(host(opt.thermal.N), NT)
    filt = orc.Filter(nx, ny, nz, h, rmin)
    mgT, mgU = orc.MG(nx, ny, nz, 1, nlv), orc.MG(nx, ny, nz, 3, nlv)
    x = np.full(ex * ey * ez, vf)
    mma = orc.MMA(x, 1)
    mma.set_device_order()
    n = nx * ny * nz
    T, U, mu, fscale, fxs = np.zeros(n), np.zeros(3 * n), np.zeros(n), 1.0, []
    xt, xp = filt.project(1, x)
    for it in range(nit):
        mgT.assemble(kt, cr.conductivity(xp, kmin), NT)
        T, its_T, _ = mgT.solve(q, x0=T, rtol=1e-10, maxit=200)
        mgU.assemble(KE, orc.simp(xp, Emin, 1.0, 3.0), N)
        rhs = N * (F + tr.load(ne, h, xp, T, p))
        U, its_U, _ = mgU.solve(rhs, x0=U, rtol=1e-10, maxit=200)
        fx, gx, df, dg = orc.compliance_sens(nx, ny, nz, KE, U, xp, Emin, 1.0, 3.0, vf)
        df = df + tr.sensitivity(ne, h, xp, [U], None, N, T, p, 2.0)
        g = tr.adjoint_rhs(ne, h, xp, [U], None, N, p)
        mu, its_mu, _ = mgT.solve(NT * g, x0=mu, rtol=1e-10, maxit=200)
        df = df + cr.response((nx, ny, nz), h, [T], [mu], [2.0], xp, kmin)["dfdx"]
        if it == 0:
            fscale = 10.0 / fx
        dfs = filt.gradient(1, x, xt, df * fscale)
        dgs = filt.gradient(1, x, xt, dg)
        xmin, xmax = mma.SetOuterMovelimit(0.0, 1.0, 0.2, x)
        x = mma.Update(x, dfs, [gx], [dgs], xmin, xmax)
        xt, xp = filt.project(1, x)
        rec = opt.step()
        fxs.append(rec["fx"])
        d = float(np.abs(host(opt.x) - x).max())
        print("iteration %d: fx %.10e (reference %.10e), gx %.3e, T_max %.6e (reference %.6e); iterations elastic %d (%d), conduction %d (%d), "
              "thermal adjoint %d (%d)" % (it + 1, rec["fx"], fx, rec["gx"], rec["T_max"], T.max(), rec["ksp_its"], its_U, rec["ksp_its_thermal"], its_T,
                                           rec["ksp_its_thermal_adjoint"], its_mu))
        show("iteration %d: max|x - x_reference|" % (it + 1), d, 1e-9)
        assert (rec["ksp_its"], rec["ksp_its_thermal"], rec["ksp_its_thermal_adjoint"]) == (its_U, its_T, its_mu)
        assert rec["fx"] == pytest.approx(fx, rel=1e-9) and rec["T_max"] == pytest.approx(T.max(), rel=1e-9) and d <= 1e-9
    opt.grid.close()


def test_elasticity_keeps_its_bits(tp):
    """physics="elasticity" on the driver's mesh: two iterations give the bits of the calls the driver made before this physics
    existed -- the same objects driven by hand (no thermal method is touched: thermal is None, no totals are formed)"""
    import torch
    (ex, ey, ez), nlv, _ = tr.DRIVER_CASE
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    kw = dict(nxyz=(nx, ny, nz), xc=(0, ex * h, 0, 1, 0, ez * h), nlvls=nlv, rmin=2.56 / ey, filter=1, volfrac=0.3)
    opt = tp.TopOpt(**kw)
    assert opt.physics_kind == "elasticity" and opt.thermal is None and opt.physics.thermal is None and opt.physics._case_total == []
    recs = [opt.step() for _ in range(2)]
    x_driver = opt.x.clone()
    opt.grid.close()
    # the same two iterations by hand, as smoke() and the reference's main.cc order them
    grid = tp.Grid(nx, ny, nz, h)
    le, flt = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=nlv)), tp.Filter(grid, 1, 2.56 / ey)
    le.SetUpLoadAndBC()
    x, xt, xp = grid.elem_vec(0.3), grid.elem_vec(0.3), grid.elem_vec(0.3)
    df, dg, xmin, xmax, xold = grid.elem_vec(), grid.elem_vec(), grid.elem_vec(), grid.elem_vec(), grid.elem_vec(0.3)
    mma = tp.MMA(grid, x, 1)
    flt.FilterProject(x, xt, xp)
    fscale = 1.0
    for it in range(2):
        fx, gx = le.ComputeObjectiveConstraintsSensitivities(df, dg, xp, 1e-9, 1.0, 3.0, 0.3)
        if it == 0:
            fscale = 10.0 / fx
        df.mul_(fscale)
        flt.Gradients(x, xt, df, [dg])
        mma.SetOuterMovelimit(0.0, 1.0, 0.2, x, xmin, xmax)
        mma.Update(x, df, [gx], [dg], xmin, xmax)
        mma.DesignChange(x, xold)
        flt.FilterProject(x, xt, xp)
        assert fx == recs[it]["fx"] and gx == recs[it]["gx"] and le.last_its == recs[it]["ksp_its"]
    assert torch.equal(x, x_driver)
    grid.close()
