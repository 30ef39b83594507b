"""The yardstick of tests/test_gpu_rowwise.py held on the CPU: on every 0/1 generator of tests/rowwise.py, on two meshes, the
float64 oracle stays within a QUARTER of the row-wise bound the HIP kernels are held to -- every level of a 3-level hierarchy,
the transfers, the Jacobi diagonal, one Chebyshev step, dfdx and the cone filter, each against the 80-bit arbiter.  And the helper itself: an error
planted where the stiffness is small passes the suite's older metric rel() and fails assert_rowwise.

Operation counts behind the constants: tests/rowwise.py, beside each constant."""
import numpy as np
import pytest

from tests import rowwise as rw

MESHES = [(36, 20, 12), (44, 12, 8)]      # elements; three levels; x beyond the seams 30..32, y beyond 14..16 on the first
NLV = 3
MEASURED = {}


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def ld(a):
    return np.ascontiguousarray(a, dtype=np.longdouble)


def note(key, c):
    MEASURED[key] = max(MEASURED.get(key, 0.0), c)


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("kind", rw.GENERATORS)
def test_oracle_within_a_quarter_of_every_bound(orc, arb, kind, mesh):
    from oracle.ke_effective import ke_effective, ke_krylov
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    x = rw.design(kind, ex, ey, ez, kz=4)
    assert set(np.unique(x)) <= {rw.XMIN, 1.0} and (x == 1.0).any() and (x == rw.XMIN).any()
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    N, R = orc.cantilever_bc(nx, ny, nz, h)
    E = orc.simp(x)
    mg = orc.MG(nx, ny, nz, 3, NLV)
    mg.assemble(KE, E, N)
    amg = arb.MG(nx, ny, nz, 3, NLV)
    amg.assemble(ld(KE), ld(E), ld(N))
    rng = np.random.default_rng(ex + ez)
    free = N != 0
    # ---- level 0: the oracle on KE against the arbiter on the packed forms the kernels apply (their distance from KE is
    # part of the bound, and must not eat it)
    u = rng.standard_normal(3 * nx * ny * nz)
    s0 = rw.scale_fine(orc, nx, ny, nz, KE, E, u) * free
    y = orc.matfree_apply(nx, ny, nz, 3, KE, E, N, u)
    assert np.array_equal(y[~free], u[~free])
    for name, K in (("apply", ke_effective(KE)), ("apply_krylov", ke_krylov(KE))):
        ya = arb.matfree_apply(nx, ny, nz, 3, ld(K), ld(E), ld(N), ld(u))
        note("fine", rw.assert_rowwise(y, ya, s0, rw.C_FINE / 4, {"label": "oracle %s %s %s" % (name, kind, mesh), "dims": (nx, ny, nz)}))
    assert s0[free].min() < 1e-6 * s0.max() or kind == "one_void"       # the rows this file is about exist
    # ---- coarser levels, one Chebyshev step on every level, transfers
    for l in range(NLV):
        dims = rw.level_dims(nx, ny, nz, l)
        n = mg.size(l)
        u, b = rng.standard_normal(n), rng.standard_normal(n)
        sl = rw.scale_level(orc, mg, l, (nx, ny, nz), KE, E, N, u)
        ya = amg.apply(l, ld(u))
        if l > 0:
            note("level", rw.assert_rowwise(mg.apply(l, u), ya, sl, rw.c_level(l) / 4, {"label": "oracle level %d %s %s" % (l, kind, mesh), "dims": dims}))
        da = np.asarray(amg.diag(l), dtype=np.float64)
        note("diag%d" % min(l, 1), rw.assert_rowwise(mg.diag(l), amg.diag(l), np.abs(da), rw.c_diag(l) / 4, {"label": "oracle diagonal level %d %s %s" % (l, kind, mesh), "dims": dims}))
        dinv = 1.0 / mg.diag(l)
        lam = mg.lam(l)
        lmin = mg.lam_min(l) if l == NLV - 1 else 0.1 * lam
        theta = 0.5 * (1.1 * lam + lmin)
        for zero in (True, False):
            x0 = np.zeros(n) if zero else u
            xa = ld(x0) + ld(dinv) * (ld(b) - (0 if zero else ya)) / np.longdouble(theta)
            sc = rw.scale_smooth(0.0 if zero else sl, dinv, 1.0 / theta, b, x0)
            note("smooth", rw.assert_rowwise(mg.smooth(l, b, x0, 1, zero), xa, sc, rw.c_smooth(l) / 4,
                                             {"label": "oracle Chebyshev step level %d zero %d %s %s" % (l, zero, kind, mesh), "dims": dims}))
        if l + 1 < NLV:
            rf, xc = rng.standard_normal(n), rng.standard_normal(mg.size(l + 1))
            note("restrict", rw.assert_rowwise(mg.restrict(l, rf), amg.restrict(l, ld(rf)), rw.scale_restrict(mg, l, rf), rw.C_RESTRICT / 4,
                                               {"label": "oracle restrict %d %s %s" % (l, kind, mesh), "dims": rw.level_dims(nx, ny, nz, l + 1)}))
            note("prolong", rw.assert_rowwise(b + mg.prolong(l, xc), ld(b) + amg.prolong(l, ld(xc)), rw.scale_prolong_add(mg, l, xc, b), rw.C_PROLONG / 4,
                                              {"label": "oracle prolong_add %d %s %s" % (l, kind, mesh), "dims": dims}))
    # ---- dfdx on a converged state
    U, its, _ = mg.solve(R * N, rtol=1e-8, maxit=400)
    _, _, df, _ = orc.compliance_sens(nx, ny, nz, KE, U, x)
    _, _, dfa, _ = arb.compliance_sens(nx, ny, nz, ld(KE), ld(U), ld(x))
    note("dfdx", rw.assert_rowwise(df, dfa, rw.scale_dfdx(nx, ny, nz, KE, U, x), rw.C_DFDX / 4,
                                   {"label": "oracle dfdx %s %s" % (kind, mesh), "dims": (ex, ey, ez), "dof": 0}))
    # ---- cone filter, forward and gradients, types 0 and 1 (ElemConn 1, 2, 5)
    df0 = rng.standard_normal(x.size)
    for rfac in rw.FILTER_RFACS[:3]:
        of, af = orc.Filter(nx, ny, nz, h, rfac * h), arb.Filter(nx, ny, nz, h, rfac * h)
        cone = rw.Cone(ex, ey, ez, h, rfac * h, of.conn)
        assert rw.rel(cone.Hs, of.hs()) <= 1e-12
        for ftype in (1, 0):
            w = {"dims": (ex, ey, ez), "dof": 0}
            xt, xta = of.project(ftype, x)[0], af.project(ftype, ld(x))[0]
            note("filter", rw.assert_rowwise(xt, xta, cone.scale_forward(ftype, x), rw.c_filter(of.conn) / 4,
                                             dict(w, label="oracle filter type %d rfac %g %s %s" % (ftype, rfac, kind, mesh))))
            g, ga = of.gradient(ftype, x, xt, df0), af.gradient(ftype, ld(x), ld(xt), ld(df0))
            note("filter", rw.assert_rowwise(g, ga, cone.scale_gradient(ftype, x, df0), rw.c_filter(of.conn) / 4,
                                             dict(w, label="oracle filter gradient type %d rfac %g %s %s" % (ftype, rfac, kind, mesh))))
    print("measured oracle-vs-arbiter constants so far:", {k: round(v, 3) for k, v in MEASURED.items()})


def test_planted_error_passes_rel_and_fails_rowwise(orc, arb):
    """31 x 17 x 9 elements, blocks + checkerboard: a relative error of 1e-6 planted in every free row whose scale is below 1e-6
    of the largest moves the product by < 1e-13 under rel() -- every older assertion passes -- and by ~1e9 eps of the row scale"""
    ex, ey, ez = 31, 17, 9
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    x = np.maximum(rw.design("blocks", ex, ey, ez), rw.design("checker", ex, ey, ez))
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    N, _ = orc.cantilever_bc(nx, ny, nz, h)
    E = orc.simp(x)
    u = np.random.default_rng(0).standard_normal(3 * nx * ny * nz)
    free = N != 0
    s = rw.scale_fine(orc, nx, ny, nz, KE, E, u) * free
    ya = arb.matfree_apply(nx, ny, nz, 3, ld(KE), ld(E), ld(N), ld(u))
    y = orc.matfree_apply(nx, ny, nz, 3, KE, E, N, u)
    w = {"label": "planted", "dims": (nx, ny, nz), "kz": 4}
    assert s[free].min() <= 1e-8 * s.max()
    assert rw.assert_rowwise(y, ya, s, rw.C_FINE / 4, w) <= 4.0           # the oracle itself: a few eps of the row scale
    small = free & (s < 1e-6 * s.max())
    assert small.sum() > 1000
    bad = y.copy()
    bad[small] *= 1.0 + 1e-6
    assert rw.rel(bad, y) <= 1e-13 and rw.rel(bad, np.asarray(ya, dtype=np.float64)) <= 1e-13
    with pytest.raises(AssertionError, match=r"i mod 15 = \d+, i mod 31 = \d+, j mod 7 = \d+, plane offset in its z-chunk \(kz 4\) = \d"):
        rw.assert_rowwise(bad, ya, s, rw.C_FINE, w)
    assert rw.achieved(bad, ya, s) >= 1e6
    # a Dirichlet row (scale 0) that does not return u bit for bit fails too
    bad = y.copy()
    row = int(np.flatnonzero(~free)[0])
    bad[row] = np.nextafter(bad[row], np.inf)
    with pytest.raises(AssertionError, match="must match exactly"):
        rw.assert_rowwise(bad, ya, s, rw.C_FINE, w)
