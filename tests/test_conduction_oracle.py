"""The conditions the bounds of tests/test_gpu_conduction.py rest on, held on the CPU: on every mesh and design
the GPU tests use, the float64 oracle (oracle.MG(dof=1), orc.matfree_apply) stays within a QUARTER of every row-wise constant of
tests/conduction_ref.py against the 80-bit arbiter; the closed form of KT; the restated sensitivity against a central difference
of the thermal compliance by a direct solve; the sink set; and the oracle's convergence on every solver case."""
import numpy as np
import pytest

from tests import conduction_ref as cr
from tests import rowwise as rw

MEASURED = {}
ALL_CASES = [c[:3] for c in cr.FINE_CASES + cr.LEVEL_CASES + cr.SLAB_CASES]


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def ld(a):
    return np.ascontiguousarray(a, dtype=np.longdouble)


def note(key, c):
    MEASURED[key] = max(MEASURED.get(key, 0.0), c)


@pytest.mark.parametrize("kind", sorted(cr.DESIGNS))
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: "x".join(str(v) for v in c[0]))
def test_oracle_within_a_quarter_of_every_bound(orc, arb, case, kind):
    (ex, ey, ez), h, nlv = case
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    dims = (nx, ny, nz)
    kt = cr.KT(h)
    x = cr.design(kind, ex, ey, ez)
    k = cr.conductivity(x, cr.DESIGNS[kind])
    N = cr.sink_mask(nx, ny, nz)
    free = N != 0
    mg = orc.MG(nx, ny, nz, 1, nlv)
    mg.assemble(kt, k, N)
    amg = arb.MG(nx, ny, nz, 1, nlv)
    amg.assemble(ld(kt), ld(k), ld(N))
    tag = "%s %s" % (kind, case[0])
    # ---- level 0 through the matrix-free gather; the sink rows return u exactly
    u, = cr.inputs(nx * ny * nz, 1, 1)
    assert (u[~free] != 0).all()
    y = orc.matfree_apply(nx, ny, nz, 1, kt, k, N, u)
    assert np.array_equal(y[~free], u[~free])
    ya = arb.matfree_apply(nx, ny, nz, 1, ld(kt), ld(k), ld(N), ld(u))
    s0 = cr.scale_fine(orc, dims, kt, k, u) * free
    note("fine", rw.assert_rowwise(y, ya, s0, cr.C_FINE / 4, {"label": "oracle fine " + tag, "dims": dims, "dof": 1}))
    assert np.abs(mg.apply(0, u) - y).max() <= 4 * cr.EPS * s0.max()      # (the assembled CSR product is the same operator)
    for l in range(nlv):
        ldims = rw.level_dims(nx, ny, nz, l)
        where = lambda what: {"label": "oracle %s level %d %s" % (what, l, tag), "dims": ldims, "dof": 1}
        n = mg.size(l)
        u, b = cr.inputs(n, 10 + l)
        sl = cr.scale_level(orc, mg, l, dims, kt, k, N, u)
        ya = amg.apply(l, ld(u))
        note("level%d" % l, rw.assert_rowwise(mg.apply(l, u), ya, sl, cr.c_op(l) / 4, where("apply")))
        da = np.asarray(amg.diag(l), dtype=np.float64)
        note("diag%d" % l, rw.assert_rowwise(mg.diag(l), amg.diag(l), np.abs(da), cr.c_diag(l) / 4, where("diagonal")))
        note("resid%d" % l, rw.assert_rowwise(b - mg.apply(l, u), ld(b) - ya, np.abs(b) + sl, cr.c_resid(l) / 4, where("residual")))
        dinv = 1.0 / mg.diag(l)
        lam = mg.lam(l)
        lmin = mg.lam_min(l) if (l == nlv - 1 and l > 0) else 0.1 * lam
        theta, delta = 0.5 * (1.1 * lam + lmin), 0.5 * (1.1 * lam - lmin)
        for zero in (True, False):
            x0 = np.zeros(n) if zero else u
            xa = ld(x0) + ld(dinv) * (ld(b) - (0 if zero else ya)) / np.longdouble(theta)
            sc = rw.scale_smooth(0.0 if zero else sl, dinv, 1.0 / theta, b, x0)
            note("smooth%d" % l, rw.assert_rowwise(mg.smooth(l, b, x0, 1, zero), xa, sc, cr.c_smooth(l) / 4, where("Chebyshev step, zero %d," % zero)))
            xs = {0: x0}
            for kk in (2, 3):
                for j in (kk - 2, kk - 1, kk):
                    if j not in xs:
                        xs[j] = mg.smooth(l, b, x0, j, zero)
                c1, c2 = rw.cheb_coeffs(theta, delta, kk)
                x1, x2 = xs[kk - 1], xs[kk - 2]
                xa = rw.step_k_ref(x1, x2, c1, c2, dinv, b, amg.apply(l, ld(x1)))
                sc = rw.scale_smooth_k(cr.scale_level(orc, mg, l, dims, kt, k, N, x1), dinv, c1, c2, b, x1, x2)
                note("smooth_k%d" % l, rw.assert_rowwise(xs[kk], xa, sc, cr.c_smooth_k(l) / 4, where("Chebyshev step %d, zero %d," % (kk, zero))))
        if l + 1 < nlv:
            rf, = cr.inputs(n, 20 + l, 1)
            xc, = cr.inputs(mg.size(l + 1), 30 + l, 1)
            note("restrict", rw.assert_rowwise(mg.restrict(l, rf), amg.restrict(l, ld(rf)), rw.scale_restrict(mg, l, rf), rw.C_RESTRICT / 4,
                                               {"label": "oracle restrict %d %s" % (l, tag), "dims": rw.level_dims(nx, ny, nz, l + 1), "dof": 1}))
            note("prolong", rw.assert_rowwise(b + mg.prolong(l, xc), ld(b) + amg.prolong(l, ld(xc)), rw.scale_prolong_add(mg, l, xc, b),
                                              rw.C_PROLONG / 4, where("prolong_add")))
    # ---- the response's float64 restatement against the longdouble one
    T, V = cr.inputs(nx * ny * nz, 40)
    for Vl, w in ((None, None), ([V, None, T], [0.75, -0.5, 0.0])):
        Tl = [T] if Vl is None else [T, V, V]
        r64 = cr.response(dims, h, Tl, Vl, w, x, cr.DESIGNS[kind])
        rld = cr.response(dims, h, Tl, Vl, w, x, cr.DESIGNS[kind], dtype=np.longdouble)
        note("dfdx", rw.assert_rowwise(r64["dfdx"], rld["dfdx"], r64["major"], cr.C_DFDX / 4, {"label": "dfdx " + tag, "dims": (ex, ey, ez), "dof": 0}))
    print("measured so far (achieved c, oracle against arbiter):", {k_: round(v, 2) for k_, v in sorted(MEASURED.items())})


def test_element_matrix_closed_form(orc):
    for h in (0.25, (0.05, 0.04, 0.03), (0.125, 0.125, 0.1), 1.0 / 31, 1.0 / 16):
        hx, hy, hz = cr.h3(h)
        kt = cr.KT(h).reshape(8, 8)
        ktl = cr.KT(h, np.longdouble).reshape(8, 8)
        top = np.abs(kt).max()
        assert np.array_equal(kt, kt.T)
        assert np.abs(kt.sum(axis=1)).max() <= 8 * cr.EPS * np.abs(kt).sum(axis=1).max()
        assert len(np.unique(kt)) <= 8
        assert np.abs(kt - ktl.astype(np.float64)).max() <= 4 * 2 * cr.EPS * top
        kf2, _ = orc.pde_kf(hx, hy, hz, 2.0)
        kf1, _ = orc.pde_kf(hx, hy, hz, 1.0)
        d = np.abs((kf2 - kf1) / 3.0 - kt.reshape(-1)).max()
        # (KF's entries carry the mass term, up to 1 / 3 of... their own size: 4 ulp of the larger of the two matrices' entries)
        print("h = %s: |(KF(2) - KF(1)) / 3 - KT| = %.3e, bound %.3e" % (h, d, 4 * 2 * cr.EPS * max(top, np.abs(kf2).max() / 3)))
        assert d <= 4 * 2 * cr.EPS * max(top, np.abs(kf2).max() / 3)


def test_sink_set_is_never_empty():
    for m in (1, 2, 3, 8):
        for n in (1, 2, 3, 8):
            N = cr.sink_mask(4, m + 1, n + 1).reshape(n + 1, m + 1, 4)
            assert (N[:, :, 0] == 0).any() and (N[:, :, 1:] == 1).all(), (m, n)
    N = cr.sink_mask(3, 9, 9).reshape(9, 9, 3)     # |2j - 8| <= 2: j = 3, 4, 5
    assert np.array_equal(np.flatnonzero(N[4, :, 0] == 0), [3, 4, 5]) and (N[0, :, 0] == 1).all()


def test_restated_sensitivity_against_a_central_difference(orc):
    """dfdx_e = -p x^(p-1) (kmax - kmin) t_e^T KT t_e is the derivative of the thermal compliance c(x) = b^T A(x)^-1 b: central
    differences of c by a scipy direct solve at 4 x 3 x 2 elements.  Bound per element: the truncation error, estimated from the steps
    d and 2 d (their difference is 3 x the error at d; twice that is allowed), plus the rounding 4 eps cond(A) |c| / d of the two
    solves."""
    import scipy.sparse.linalg as spl
    ex, ey, ez, h = 4, 3, 2, (0.3, 0.25, 0.2)
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    kt, N = cr.KT(h), cr.sink_mask(nx, ny, nz)
    b = N * cr.load(nx, ny, nz, h)
    kmin = cr.DESIGNS["mixed"]
    x = cr.design("mixed", ex, ey, ez)

    def solve(xv):
        mg = orc.MG(nx, ny, nz, 1, 1)
        mg.assemble(kt, cr.conductivity(xv, kmin), N)
        A = mg.csr(0).tocsc()
        return spl.spsolve(A, b), A

    T, A = solve(x)
    c0 = float(b @ T)
    cond = np.linalg.cond(A.toarray())
    got = cr.response((nx, ny, nz), h, [T], None, None, x, kmin)["dfdx"]
    d = 1e-4
    worst = 0.0
    for e in range(x.size):
        fd = []
        for step in (d, 2 * d):
            xp, xm = x.copy(), x.copy()
            xp[e] += step
            xm[e] -= step
            fd.append((float(b @ solve(xp)[0]) - float(b @ solve(xm)[0])) / (2 * step))
        bound = 2.0 * abs(fd[1] - fd[0]) / 3.0 + 4 * cr.EPS * cond * abs(c0) / d
        worst = max(worst, abs(got[e] - fd[0]) / bound)
        assert abs(got[e] - fd[0]) <= bound, (e, got[e], fd, bound)
    print("dfdx against central differences: worst |difference| / bound = %.3f, cond(A) = %.2e" % (worst, cond))


@pytest.mark.parametrize("kind", sorted(cr.DESIGNS))
@pytest.mark.parametrize("ci", cr.SOLVE_CASES + ["slab0", "slab1"])
def test_oracle_converges_on_every_solver_case(orc, ci, kind):
    (ex, ey, ez), h, nlv = (cr.SLAB_CASES[int(ci[4:])] if isinstance(ci, str) else cr.LEVEL_CASES[ci])[:3]
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    kt, N = cr.KT(h), cr.sink_mask(nx, ny, nz)
    mg = orc.MG(nx, ny, nz, 1, nlv, nsmooth=cr.SOLVE["nsmooth"], ncoarse=cr.SOLVE["ncoarse"])
    mg.assemble(kt, cr.conductivity(cr.design(kind, ex, ey, ez), cr.DESIGNS[kind]), N)
    b = N * cr.load(nx, ny, nz, h)
    T, its, hist = mg.solve(b, rtol=cr.SOLVE["rtol"], maxit=200)
    print("%s %s: %d iterations to rtol %g, ||r|| / ||b|| = %.3e" % (kind, (ex, ey, ez), its, cr.SOLVE["rtol"], hist[-1] / np.linalg.norm(b)))
    assert 0 < its <= 50 and hist[-1] <= cr.SOLVE["rtol"] * np.linalg.norm(b)
    # the GPU tests run with max_it = 4 x this count: the solve from the converged state then takes none
    assert mg.solve(b, x0=T, rtol=cr.SOLVE["rtol"], maxit=4 * its)[1] == 0
