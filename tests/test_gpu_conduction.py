"""Heat conduction on the device, kernel by kernel against the 80-bit arbiter and the float64 oracle.

Fine operator: both forms -- ConductionOp (k_node<1, ConductionOp>, last_op_form 3,2,0,0) and the gather (k_node<1, MatfreeOp<1>>,
TP_NO_COND_STENCIL set, 3,0,0,0), flipped inside the process (the switch is read per launch) -- through MatMult, level_dinv,
smooth k = 1, 2, 3 from a zero and a non-zero guess and level_residual, row by row within the constants of
tests/conduction_ref.py; sink rows return u exactly; the two forms give the same bits (they sum in one order).
Hierarchy: every level's product and diagonal against the arbiter's P^T A P, the transfers, the windows against the oracle's.
Solve: iteration count equal to the oracle's, the residual history within test_solve_residual_history's three bounds.
Response: dfdx per element within its own majorant, the sums at 1e-13.  Driver: three design iterations against the same loop
assembled from oracle pieces.  Every device figure is printed with its bound before it is asserted.

Achieved on the MI355X (recorded for the reader; the bounds come from tests/conduction_ref.py), levels 0 / 1 / 2 / 3, worst over
the meshes, designs and forms: product 3.8 / 1.8 / 1.2 / 0.6 (bounds 64 / 64 / 128 / 128), Jacobi diagonal 5.2 / 6.1 / 4.0 / 4.5
(128), residual 2.2 / 1.5 / 1.3 / 0.7 (64 / 64 / 128 / 128), Chebyshev step 1 3.8 / 2.6 / 1.9 / 1.5 (64 / 64 / 128 / 128), steps 2
and 3 4.4 / 1.2 / 0.5 / 0.4 (128), restrict 4.2, prolong_add 2.0 (64), dfdx 2.8 (128), the fused u . A u 1.4 (32); windows equal
to the oracle's to 2.4e-14; solve: iterations 15 .. 17 = the oracle's, history 6.2e-12 / 1.5e-10 / 1.1e-7 against 1e-10 / 1e-9 /
1e-6, T 2.1e-14; driver: the design within 1.9e-14 of the reference loop's.  The 23 tests: 3.5 s.
"""
import os

import numpy as np
import pytest

from tests import conduction_ref as cr
from tests import rowwise as rw

pytestmark = pytest.mark.gpu
FORMS = {"registers": (None, (3, 2, 0, 0)), "gather": ("1", (3, 0, 0, 0))}
SWITCH = "TP_NO_COND_STENCIL"
_REF = {}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


@pytest.fixture(autouse=True)
def _switch_restored():
    old = os.environ.get(SWITCH)
    yield
    os.environ.pop(SWITCH, None)
    if old is not None:
        os.environ[SWITCH] = old


def set_form(form):
    os.environ.pop(SWITCH, None)
    if FORMS[form][0] is not None:
        os.environ[SWITCH] = FORMS[form][0]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ld(a):
    return np.ascontiguousarray(a, dtype=np.longdouble)


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def show(what, got, bound):
    print("%-72s %.4g (bound %.4g)" % (what, got, bound))
    return got


def held(got, ref, scale, c, label, dims, dof=1):
    a = rw.achieved(got, ref, scale)
    show(label + ": achieved c", a, c)
    return rw.assert_rowwise(got, ref, scale, c, {"label": label, "dims": dims, "dof": dof})


def problem(orc, arb, case, kind, **mgkw):
    """the case's data and its two reference hierarchies (float64 oracle, 80-bit arbiter), made once"""
    def make():
        (ex, ey, ez), h, nlv = case[:3]
        nx, ny, nz = ex + 1, ey + 1, ez + 1
        kt, x, N = cr.KT(h), cr.design(kind, ex, ey, ez), cr.sink_mask(nx, ny, nz)
        k = cr.conductivity(x, cr.DESIGNS[kind])
        mg = orc.MG(nx, ny, nz, 1, nlv, **mgkw)
        mg.assemble(kt, k, N)
        amg = arb.MG(nx, ny, nz, 1, nlv, **mgkw)
        amg.assemble(ld(kt), ld(k), ld(N))
        return dict(dims=(nx, ny, nz), ne=(ex, ey, ez), h=h, nlv=nlv, kt=kt, x=x, N=N, k=k, mg=mg, amg=amg, kmin=cr.DESIGNS[kind],
                    b=N * cr.load(nx, ny, nz, h))
    return cached(("problem", case[:3], kind, tuple(sorted(mgkw.items()))), make)


def device(tp, P, **opts):
    nx, ny, nz = P["dims"]
    grid = tp.Grid(nx, ny, nz, P["h"])
    hc = tp.HeatConduction(grid, tp.SolverOptions(nlvls=P["nlv"], **opts))
    hc.SetBC(dev(P["N"]), dev(P["b"]))
    hc.AssembleConductivityMatrix(dev(P["x"]), P["kmin"], cr.KMAX, cr.PENAL)
    return grid, hc


def window(hc, nlv, l):
    lam = hc.level_lambda(l)
    lmin = hc.level_lambda_min(l) if (l == nlv - 1 and l > 0) else 0.1 * lam
    return 0.5 * (1.1 * lam + lmin), 0.5 * (1.1 * lam - lmin)


def check_level(orc, P, hc, l, tag, form=None):
    """product, diagonal, residual and Chebyshev steps 1, 2, 3 from a zero and a non-zero guess on level l -> the device's product"""
    dims = rw.level_dims(*P["dims"], l)
    mg, amg = P["mg"], P["amg"]
    n = mg.size(l)
    assert hc.level_nodes(l) == n
    u, b = cr.inputs(n, 10 + l)
    free = (P["N"] != 0) if l == 0 else np.ones(n, dtype=bool)
    sl, ya = cached(("scale", tag, l), lambda: (cr.scale_level(orc, mg, l, P["dims"], P["kt"], P["k"], P["N"], u), amg.apply(l, ld(u))))
    expect = None if form is None else FORMS[form][1]
    y = host(hc.level_apply(l, dev(u)) if l else hc.MatMult(dev(u)))
    if l == 0:
        assert hc.last_op_form() == expect, (hc.last_op_form(), expect)
        assert (u[~free] != 0).all() and np.array_equal(y[~free], u[~free])     # the sink rows return u exactly
    else:
        assert hc.last_op_form()[0] == 4
    held(y, ya, sl * free, cr.c_op(l), "%s level %d product" % (tag, l), dims)
    if l == 0:   # the Krylov method's form of the product: the same bits, and the VALUE of its fused u . A u against an 80-bit sum
        yk, dot = hc.MatMultDot(dev(u))
        assert hc.last_op_form() == expect and np.array_equal(host(yk), y)
        terms = ld(u) * ld(y)
        c = rw.c_dot(1, rw.dot_workgroups((3, 0, 0, 0), dims))
        show("%s fused u . A u: |difference| / (eps sum |terms|)" % tag, float(abs(dot - terms.sum()) / (rw.EPS * np.abs(terms).sum())), c)
        assert abs(dot - terms.sum()) <= c * rw.EPS * np.abs(terms).sum()
    dinv = host(hc.level_dinv(l))
    da = np.asarray(amg.diag(l), dtype=np.float64)
    held(1.0 / dinv, amg.diag(l), np.abs(da), cr.c_diag(l), "%s level %d Jacobi diagonal" % (tag, l), dims)
    r = host(hc.level_residual(l, dev(b), dev(u)))
    held(r, ld(b) - ya, np.abs(b) + sl, cr.c_resid(l), "%s level %d residual" % (tag, l), dims)
    theta, delta = window(hc, P["nlv"], l)
    for zero in (True, False):
        x0 = np.zeros(n) if zero else u
        xs = {0: x0}
        for k in (1, 2, 3):
            xs[k] = host(hc.smooth(l, dev(b), dev(x0), k, zero))
            if l == 0:
                assert hc.last_op_form() == expect or (zero and k == 1)       # (the zero guess's first step is a scaling)
        xa = ld(x0) + ld(dinv) * (ld(b) - (0 if zero else ya)) / np.longdouble(theta)
        sc = rw.scale_smooth(0.0 if zero else sl, dinv, 1.0 / theta, b, x0)
        held(xs[1], xa, sc, cr.c_smooth(l), "%s level %d Chebyshev step 1, zero guess %d" % (tag, l, zero), dims)
        for k in (2, 3):
            c1, c2 = rw.cheb_coeffs(theta, delta, k)
            x1, x2 = xs[k - 1], xs[k - 2]
            xa = rw.step_k_ref(x1, x2, c1, c2, dinv, b, amg.apply(l, ld(x1)))
            sc = rw.scale_smooth_k(cr.scale_level(orc, mg, l, P["dims"], P["kt"], P["k"], P["N"], x1), dinv, c1, c2, b, x1, x2)
            held(xs[k], xa, sc, cr.c_smooth_k(l), "%s level %d Chebyshev step %d, zero guess %d" % (tag, l, k, zero), dims)
    return y, dinv, r, xs


@pytest.mark.parametrize("kind", sorted(cr.DESIGNS))
@pytest.mark.parametrize("case", cr.FINE_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_fine_operator_both_forms(tp, orc, arb, case, kind):
    P = problem(orc, arb, case, kind)
    grid, hc = device(tp, P)
    assert np.array_equal(hc.KT, P["kt"])
    out = {}
    for form in FORMS:
        set_form(form)
        out[form] = check_level(orc, P, hc, 0, "%s %s %s" % (form, kind, P["ne"]), form)
    (ya, da, ra, xa), (yb, db, rb, xb) = out["registers"], out["gather"]
    assert np.array_equal(ya, yb) and np.array_equal(da, db) and np.array_equal(ra, rb)     # one summation order: the same bits
    assert all(np.array_equal(xa[k], xb[k]) for k in xa)
    grid.close()


@pytest.mark.parametrize("kind", sorted(cr.DESIGNS))
@pytest.mark.parametrize("case", cr.LEVEL_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_hierarchy_row_by_row(tp, orc, arb, case, kind):
    P = problem(orc, arb, case, kind)
    grid, hc = device(tp, P)
    mg, amg, nlv = P["mg"], P["amg"], P["nlv"]
    assert hc.level_count() == nlv
    tag = "%s %s" % (kind, P["ne"])
    for l in range(nlv):
        check_level(orc, P, hc, l, tag, "registers" if l == 0 else None)
        got, ref = hc.level_lambda(l), mg.lam(l)
        show("%s level %d lambda: relative difference from the oracle's" % (tag, l), abs(got / ref - 1), 1e-10)
        assert abs(got / ref - 1) <= 1e-10
        if l == nlv - 1:
            got, ref = hc.level_lambda_min(l), mg.lam_min(l)
            show("%s level %d lambda_min: relative difference from the oracle's" % (tag, l), abs(got / ref - 1), 1e-10)
            assert abs(got / ref - 1) <= 1e-10
        if l + 1 < nlv:
            dims, cdims = rw.level_dims(*P["dims"], l), rw.level_dims(*P["dims"], l + 1)
            rf, = cr.inputs(mg.size(l), 20 + l, 1)
            xc, = cr.inputs(mg.size(l + 1), 30 + l, 1)
            xf, = cr.inputs(mg.size(l), 50 + l, 1)
            held(host(hc.restrict(l, dev(rf))), amg.restrict(l, ld(rf)), rw.scale_restrict(mg, l, rf), rw.C_RESTRICT, "%s restrict %d" % (tag, l), cdims)
            held(host(hc.prolong_add(l, dev(xc), dev(xf))), ld(xf) + amg.prolong(l, ld(xc)), rw.scale_prolong_add(mg, l, xc, xf), rw.C_PROLONG,
                 "%s prolong_add %d" % (tag, l), dims)
    grid.close()


@pytest.mark.parametrize("kind", sorted(cr.DESIGNS))
@pytest.mark.parametrize("ci", cr.SOLVE_CASES)
def test_solve_against_the_oracle(tp, orc, arb, ci, kind):
    case = cr.LEVEL_CASES[ci]
    P = problem(orc, arb, case, kind, nsmooth=cr.SOLVE["nsmooth"], ncoarse=cr.SOLVE["ncoarse"])
    To, its_o, hist_o = cached(("solve", ci, kind), lambda: P["mg"].solve(P["b"], rtol=cr.SOLVE["rtol"], maxit=200))
    assert 0 < its_o <= 50
    grid, hc = device(tp, P, nsmooth=cr.SOLVE["nsmooth"], ncoarse=cr.SOLVE["ncoarse"], rtol=cr.SOLVE["rtol"], max_it=4 * its_o)
    its = hc.KSPSolve(hist_cap=4 * its_o + 1)
    h, bn = hc.last_hist, hc.last_bnorm
    tag = "%s %s" % (kind, P["ne"])
    print("%s: %d iterations, the oracle %d" % (tag, its, its_o))
    assert its == its_o and len(h) == len(hist_o)
    d = np.abs(h / hist_o - 1)
    big = hist_o > 1e-7 * bn
    show(tag + " residual history, first ten entries", d[:10].max(), 1e-10)
    show(tag + " residual history above 1e-7 |b|", d[big].max(), 1e-9)
    show(tag + " residual history, all", d.max(), 1e-6)
    show(tag + " max|T - T_oracle| / max|T_oracle|", rw.rel(host(hc.T), To), 1e-9)
    show(tag + " |b|: relative difference", abs(bn / np.linalg.norm(P["b"]) - 1), 1e-14)
    assert d[:10].max() <= 1e-10 and d[big].max() <= 1e-9 and d.max() <= 1e-6
    assert rw.rel(host(hc.T), To) <= 1e-9
    assert bn == pytest.approx(np.linalg.norm(P["b"]), rel=1e-14)
    assert hc.KSPSolve() == 0          # warm start from the converged state
    grid.close()


@pytest.mark.parametrize("kind", sorted(cr.DESIGNS))
def test_response(tp, orc, arb, kind):
    """sums: a float64 sum of n terms is within n eps of the sum of their absolute values, 1e-13 for the project's VecDot; the
    compliance's terms are non-negative, so for V = T that is 1e-13 of the value itself; a bilinear f_l and the weighted fx of
    mixed signs are held to 1e-13 of the sum of their terms' majorants"""
    import torch
    (ex, ey, ez), h, _ = cr.LEVEL_CASES[0]
    P = problem(orc, arb, ((ex, ey, ez), h, 1), kind)
    grid, hc = device(tp, P)
    n, nel = np.prod(P["dims"]), ex * ey * ez
    T, V = cr.inputs(n, 40)
    vf, kmin = 0.3, P["kmin"]
    for Tl, Vl, w in (([T], None, None), ([T], [V], None), ([T, V, V], [V, None, T], [0.75, -0.5, 0.0]), ([T, V, T], None, [0.75, -0.5, 0.0])):
        tag = "%s ncase %d %s" % (kind, len(Tl), "V = T" if Vl is None else "V != T")
        ref = cr.response(P["dims"], h, Tl, Vl, w, P["x"], kmin, volfrac=vf, dtype=np.longdouble)
        df, dg = grid.elem_vec(7.0), grid.elem_vec(7.0)
        Vd = None if Vl is None else [None if v is None else dev(v) for v in Vl]
        Td = [dev(t) for t in Tl]
        fx, gx, fc = hc.Response(Td, Vd, w, dev(P["x"]), kmin, cr.KMAX, cr.PENAL, vf, df, dg)
        held(host(df), ref["dfdx"], ref["major"], cr.C_DFDX, tag + " dfdx", (ex, ey, ez), dof=0)
        assert np.array_equal(host(dg), np.full(nel, 1.0 / nel))
        ws = [1.0] * len(Tl) if w is None else w
        majs = []
        for l in range(len(Tl)):
            same = Vl is None or Vl[l] is None
            maj = abs(float(ref["f_case"][l])) if same else ref["f_major"][l]
            majs.append(maj)
            show("%s f_case[%d]: |difference| / %s" % (tag, l, "itself" if same else "its terms"), abs(fc[l] - float(ref["f_case"][l])) / maj, 1e-13)
            assert abs(fc[l] - float(ref["f_case"][l])) <= 1e-13 * maj
        mfx = sum(abs(wl) * m for wl, m in zip(ws, majs))
        show(tag + " fx: |difference| / its terms", abs(fx - float(ref["fx"])) / mfx, 1e-13)
        show(tag + " gx: |difference|", abs(gx - float(ref["gx"])), 1e-15)
        assert abs(fx - float(ref["fx"])) <= 1e-13 * mfx and abs(gx - float(ref["gx"])) <= 1e-15
        # no sums asked for: nothing comes back, the same sensitivities bit for bit
        df2 = grid.elem_vec(7.0)
        assert hc.Response(Td, Vd, w, dev(P["x"]), kmin, cr.KMAX, cr.PENAL, vf, df2, None, sums=False) == (None, None, None)
        assert torch.equal(df, df2)
    grid.close()


def test_driver_three_design_iterations(tp, orc):
    """TopOpt(physics="heat") against the same loop assembled from oracle pieces: orc.MG solve at rtol 1e-10 (warm-started like the
    driver), the restated sensitivities, orc.Filter, orc.MMA in device order.  The design within 1e-9, the bound tests/test_mma.py
    holds the device MMA to against the reference class"""
    (ex, ey, ez), nlv, nit = cr.DRIVER_CASE
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    vf, rmin, kmin = 0.3, 2.56 / ey, 1e-3
    opt = tp.TopOpt(nxyz=(nx, ny, nz), xc=(0, ex * h, 0, 1, 0, ez * h), nlvls=nlv, rmin=rmin, filter=1, volfrac=vf, physics="heat",
                    solver=tp.SolverOptions(nlvls=nlv, rtol=1e-10, max_it=200))
    assert opt.physics_kind == "heat" and isinstance(opt.physics, tp.api.HeatConduction)
    kt, N = cr.KT(h), cr.sink_mask(nx, ny, nz)
    b = N * cr.load(nx, ny, nz, h)
    assert np.array_equal(host(opt.physics.N), N) and np.array_equal(host(opt.physics.RHS), cr.load(nx, ny, nz, h))
    filt, mg = orc.Filter(nx, ny, nz, h, rmin), orc.MG(nx, ny, nz, 1, nlv)
    x = np.full(ex * ey * ez, vf)
    mma = orc.MMA(x, 1)
    mma.set_device_order()
    T, fscale, fxs = np.zeros(nx * ny * nz), 1.0, []
    xt, xp = filt.project(1, x)
    for it in range(nit):
        mg.assemble(kt, cr.conductivity(xp, kmin), N)
        T, its_o, _ = mg.solve(b, x0=T, rtol=1e-10, maxit=200)
        r = cr.response((nx, ny, nz), h, [T], None, None, xp, kmin, volfrac=vf)
        if it == 0:
            fscale = 10.0 / r["fx"]
        df = filt.gradient(1, x, xt, r["dfdx"] * fscale)
        dg = filt.gradient(1, x, xt, r["dgdx"])
        xmin, xmax = mma.SetOuterMovelimit(0.0, 1.0, 0.2, x)
        x = mma.Update(x, df, [r["gx"]], [dg], xmin, xmax)
        xt, xp = filt.project(1, x)
        rec = opt.step()
        fxs.append(rec["fx"])
        d = float(np.abs(host(opt.x) - x).max())
        print("iteration %d: fx %.10e (reference %.10e), gx %.3e, solver iterations %d (reference %d)" % (it + 1, rec["fx"], r["fx"], rec["gx"], rec["ksp_its"], its_o))
        show("iteration %d: max|x - x_reference|" % (it + 1), d, 1e-9)
        assert rec["ksp_its"] == its_o and rec["fx"] == pytest.approx(r["fx"], rel=1e-9) and d <= 1e-9
    assert fxs[-1] < fxs[0]
    opt.grid.close()
