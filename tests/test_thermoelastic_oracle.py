"""The conditions the bounds of tests/test_gpu_thermoelastic.py rest on, held on the CPU: the closed form of the
coupling matrix G against Gauss quadrature of B^T D0 phi N_b in 80-bit arithmetic, its self-equilibrium, free expansion against
the project's own KE, the transpose identity of load and adjoint right-hand side, the whole coupled gradient against central
differences of the compliance by direct solves of both state problems in both thermal modes, and the float64 forms of
tests/thermoelastic_ref.py within a QUARTER of every row-wise constant against the longdouble ones on every mesh and design the
GPU tests use."""
import numpy as np
import pytest

from tests import conduction_ref as cr
from tests import rowwise as rw
from tests import thermoelastic_ref as tr

LD = np.longdouble
MEASURED = {}
BOXES = [c[1] for c in tr.FINE_CASES]
ALL_CASES = [c[:2] for c in tr.FINE_CASES + tr.SLAB_CASES]


def note(key, c):
    MEASURED[key] = max(MEASURED.get(key, 0.0), c)
    return c


@pytest.mark.parametrize("h", BOXES, ids=str)
def test_closed_form_G_against_quadrature(h):
    """the quadrature is exact for the integrand: the longdouble closed form equals it to a few longdouble ulp, and the float64
    closed form (the library's arithmetic) sits within C_G eps of max|G|"""
    gq, gl, g64 = tr.G_quadrature(h), tr.G(h, dtype=LD), tr.G(h)
    top = float(np.abs(gq).max())
    d_ld = float(np.abs(gl - gq).max()) / (float(np.finfo(LD).eps) * top)
    d64 = note("G", float(np.abs(g64.astype(LD) - gq).max()) / (tr.EPS * top))
    print("h = %s: longdouble closed form off the quadrature by %.2f longdouble ulp of max|G| (bound 32); float64 form: achieved c = %.3f (bound %d)"
          % (h, d_ld, d64, tr.C_G))
    assert d_ld <= 32 and d64 <= tr.C_G
    assert len(np.unique(np.abs(g64))) <= 9


@pytest.mark.parametrize("h", BOXES, ids=str)
def test_element_load_is_self_equilibrated(h):
    """sum_a G[(a,c), b] = 0 for every c and b: in the closed form the corners on the two sides of axis c carry the same magnitudes"""
    g = tr.G(h).reshape(8, 3, 8)
    s = np.abs(g.sum(axis=0)).max()
    print("h = %s: max |sum_a G| = %.3e (bound %.3e)" % (h, s, 8 * tr.EPS * np.abs(g).sum(axis=0).max()))
    assert s <= 8 * tr.EPS * np.abs(g).sum(axis=0).max()
    gq = tr.G_quadrature(h).reshape(8, 3, 8)
    assert float(np.abs(gq.sum(axis=0)).max()) <= 32 * float(np.finfo(LD).eps) * float(np.abs(gq).sum(axis=0).max())


@pytest.mark.parametrize("h", BOXES, ids=str)
def test_free_expansion_is_stress_free(orc, h):
    """KE (corner positions) = G 1 at unit modulus: the strain (1, 1, 1, 0, 0, 0) loads the element as a unit temperature rise
    does.  KE is the project's own (the oracle's restatement of elements.h, bit-equal to tests/golden/ref_ke.bin on its box)"""
    hx, hy, hz = cr.h3(h)
    KE = np.asarray(orc.hex8_ke_box(hx, hy, hz, tr.NU)).reshape(24, 24)
    xc = tr.corner_coordinates(h)
    lhs = KE @ xc
    rhs = tr.G(h, dtype=LD).sum(axis=1)
    scale = np.abs(KE) @ np.abs(xc) + np.abs(tr.G(h)).sum(axis=1)
    c = note("free", rw.assert_rowwise(lhs, rhs, scale, tr.C_FREE, {"label": "KE x = G 1, h = %s" % (h,), "dims": (2, 2, 2), "dof": 3}))
    print("h = %s: KE x against G 1: achieved c = %.3f (bound %d)" % (h, c, tr.C_FREE))
    # with another Poisson ratio the identity fails by far more than the bound: the check ties G to the KE's nu
    other = tr.G(h, nu=0.25, dtype=LD).sum(axis=1)
    assert float(np.abs(lhs - other).max()) > 1e3 * tr.C_FREE * tr.EPS * scale.max()


@pytest.mark.parametrize("kind", sorted(tr.DESIGNS))
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_float64_forms_within_a_quarter_of_every_bound(case, kind):
    ne, h = case
    nel = ne[0] * ne[1] * ne[2]
    p = tr.par(kind)
    x = cr.design(kind, *ne)
    N, _ = tr.cantilever(ne, h)
    T, v0, v1, v2 = tr.fields(ne, 1)
    assert (np.abs(v0[N == 0]) > 0).any() and p["T_ref"] != 0
    tag = "%s %s" % (kind, ne)
    nd = (ne[0] + 1, ne[1] + 1, ne[2] + 1)
    where = lambda what, dof: {"label": "%s %s" % (what, tag), "dims": ne if dof == 0 else nd, "dof": dof}
    # ---- the interpolation on its own
    b64, bld = tr.beta(x, p), tr.beta(x, p, LD)
    note("beta", rw.assert_rowwise(b64, bld, np.abs(b64), tr.C_BETA / 4, where("beta", 0)))
    d64, dld = tr.dbeta(x, p), tr.dbeta(x, p, LD)
    note("dbeta", rw.assert_rowwise(d64, dld, np.abs(d64), tr.C_DBETA / 4, where("beta'", 0)))
    # ---- the load, alone and on a base
    s = tr.load(ne, h, x, T, p, absolute=True)
    f64, fld = tr.load(ne, h, x, T, p), tr.load(ne, h, x, T, p, dtype=LD)
    note("load", rw.assert_rowwise(f64, fld, s, tr.C_LOAD / 4, where("load", 3)))
    note("load", rw.assert_rowwise(v1 + f64, v1.astype(LD) + fld, s + np.abs(v1), tr.C_LOAD / 4, where("load on a base", 3)))
    # ---- the transpose and the sensitivity, one field and three weighted ones
    for Vl, w in (([v0], None), ([v0, v1, v2], [0.75, -0.5, 1.25])):
        sg = tr.adjoint_rhs(ne, h, x, Vl, w, N, p, 1.5, absolute=True)
        g64, gld = tr.adjoint_rhs(ne, h, x, Vl, w, N, p, 1.5), tr.adjoint_rhs(ne, h, x, Vl, w, N, p, 1.5, dtype=LD)
        note("adjoint", rw.assert_rowwise(g64, gld, sg, tr.C_ADJ / 4, where("adjoint rhs, %d fields," % len(Vl), 1)))
        base = cr.design("mixed", *ne, seed=3) - 0.5
        ss = tr.sensitivity(ne, h, x, Vl, w, N, T, p, 2.0, absolute=True) + np.abs(base)
        s64 = base + tr.sensitivity(ne, h, x, Vl, w, N, T, p, 2.0)
        sld = base.astype(LD) + tr.sensitivity(ne, h, x, Vl, w, N, T, p, 2.0, dtype=LD)
        note("sens", rw.assert_rowwise(s64, sld, ss, tr.C_SENS / 4, where("sensitivity, %d fields," % len(Vl), 0)))
    assert s.shape == (3 * np.prod(nd),) and nel == x.size
    print("measured so far (achieved c, float64 against longdouble):", {k: round(v, 2) for k, v in sorted(MEASURED.items())})


@pytest.mark.parametrize("kind", sorted(tr.DESIGNS))
@pytest.mark.parametrize("case", ALL_CASES[:4], ids=lambda c: "x".join(str(v) for v in c[0]))
def test_transpose_identity(case, kind):
    """<N v, f_th(theta)> = <g(v), theta>: the two passes are transposes of each other through N.  The inner products are formed in
    longdouble from the float64 vectors, so what is left is the two chains: (C_LOAD + C_ADJ) eps of the common majorant
    <|v|, |f_th|(|theta|)>"""
    ne, h = case
    p = tr.par(kind)
    x = cr.design(kind, *ne)
    N, _ = tr.cantilever(ne, h)
    T, v0, _, _ = tr.fields(ne, 2)
    th = tr.theta(T, p, LD)
    assert (v0[N == 0] != 0).all()
    f = tr.load(ne, h, x, T, p)
    g = tr.adjoint_rhs(ne, h, x, [v0], None, N, p)
    lhs = ((N * v0).astype(LD) * f.astype(LD)).sum()
    rhs = (g.astype(LD) * th).sum()
    major = float((np.abs(v0) * tr.load(ne, h, x, T, p, absolute=True)).sum())
    bound = (tr.C_LOAD + tr.C_ADJ) * tr.EPS * major
    print("%s %s: <N v, f> = %.15e, <g, theta> = %.15e, |difference| / bound = %.3f" % (kind, ne, float(lhs), float(rhs), float(abs(lhs - rhs)) / bound))
    assert float(abs(lhs - rhs)) <= bound
    # without N inside the transpose the two sides differ: the fields do not vanish on the supports
    g_free = tr.adjoint_rhs(ne, h, x, [v0], None, np.ones_like(N), p)
    assert float(abs((g_free.astype(LD) * th).sum() - lhs)) > 1e3 * bound


@pytest.mark.parametrize("mode", ["conduction", "uniform"])
def test_coupled_gradient_against_central_differences(orc, mode):
    """dc/dx_e (elastic term + load term at fixed T + thermal adjoint term) against central differences of c(x) = u^T K u with
    both state problems solved directly, 6 x 4 x 4, the mixed design at kmin = 1e-3, Emin = 1e-9, alpha such that |f_th| = |F|.
    Bound per element as tests/test_conduction_oracle.py states its own: the truncation error, estimated from the steps d and 2 d
    (their difference is 3 x the error at d; twice that is allowed), plus the rounding 4 eps cond |c| / d of the two solves, cond
    the larger of the two operators' condition numbers"""
    from tests import scipy_check as sc
    ne, h = tr.CPU_GRADIENT_CASE
    hx, hy, hz = cr.h3(h)
    KE = np.asarray(orc.hex8_ke_box(hx, hy, hz, tr.NU))
    x = cr.design("mixed", *ne)
    dT = 0.8 if mode == "uniform" else None
    unit = tr.Coupled(ne, h, KE, tr.par("mixed", alpha=1.0), mode, dT)
    s1 = unit.state(x)
    alpha = float(np.linalg.norm(unit.N * unit.F) / np.linalg.norm(unit.N * s1["f_th"]))
    cp = tr.Coupled(ne, h, KE, tr.par("mixed", alpha=alpha), mode, dT)
    s0 = cp.state(x)
    ratio = np.linalg.norm(cp.N * s0["f_th"]) / np.linalg.norm(cp.N * cp.F)
    assert 0.5 < ratio < 2.0
    G = cp.gradient(x, s0)
    K = sc.assemble(*ne, cp.KE, E=cp.E(x), N=cp.N)
    cond = np.linalg.cond(K.toarray())
    if mode == "conduction":
        A = sc.assemble(*ne, cp.KT, E=cr.conductivity(x, cp.kmin), N=cp.NT, dof=1)
        cond = max(cond, np.linalg.cond(A.toarray()))
    else:
        assert G["mu"] is None and not G["adjoint"].any()
    d, worst, c0 = 1e-4, 0.0, s0["c"]
    needed = {"thermal": 0, "adjoint": 0}      # elements at which the comparison fails without the term
    for e in range(x.size):
        fd = []
        for step in (d, 2 * d):
            xp, xm = x.copy(), x.copy()
            xp[e] += step
            xm[e] -= step
            fd.append((cp.state(xp)["c"] - cp.state(xm)["c"]) / (2 * step))
        bound = 2.0 * abs(fd[1] - fd[0]) / 3.0 + 4 * tr.EPS * cond * abs(c0) / d
        worst = max(worst, abs(G["dc"][e] - fd[0]) / bound)
        assert abs(G["dc"][e] - fd[0]) <= bound, (e, G["dc"][e], fd, bound)
        for name in needed:
            needed[name] += abs(G["dc"][e] - G[name][e] - fd[0]) > bound
    assert needed["thermal"] > x.size // 2 and (needed["adjoint"] > x.size // 2 if mode == "conduction" else needed["adjoint"] == 0), needed
    print("%s: alpha %.4e (|f_th| / |F| = %.3f), c = %.6e; dc/dx against central differences: worst |difference| / bound = %.3f, cond = %.2e; "
          "max|term| elastic %.3e, load %.3e, adjoint %.3e; elements at which the comparison needs the term: %s of %d"
          % (mode, alpha, ratio, c0, worst, cond, np.abs(G["elastic"]).max(), np.abs(G["thermal"]).max(), np.abs(G["adjoint"]).max(), needed, x.size))
