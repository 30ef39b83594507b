"""The yardstick of tests/test_gpu_rowwise.py held on the CPU: on every 0/1 generator of tests/rowwise.py, on two meshes, the
float64 oracle stays within a QUARTER of the row-wise bound the HIP kernels are held to -- every level of a 3-level hierarchy,
the transfers, the Jacobi diagonal, one Chebyshev step, steps 2, 3, 4 (and 20 on the coarsest level) of a sweep, the V-cycle's
residual, dfdx and the cone filter, each against the 80-bit arbiter.  And the helper itself: an error
planted where the stiffness is small passes the suite's older metric rel() and fails assert_rowwise; so does a later Chebyshev
step whose c1 term is dropped on the rows of small scale.

The same for the Helmholtz (PDE) filter's scalar hierarchy (tests/test_gpu_pde_rowwise.py): the oracle within a quarter of each
constant on every mesh, regime and input of rw.PDE_CASES, and two planted errors in a numpy restatement of the 27 x 27 class
table -- two axes exchanged (invisible on a cube, caught on the anisotropic box) and one coarse weight off by 2^-40.

The slab cases (rw.SLAB_FINE, rw.SLAB_COARSE, rw.SLAB_GENERATORS with the two seam designs): the oracle within a quarter of the
one-rank constants on every mesh with its own level count, both boundary conditions and all seven designs; SlabPartition's
arithmetic on every level of every case; and seam errors planted in a float64 restatement that computes rank by rank from
slab-local arrays -- each passes rel() and fails the row-wise bound.

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


def quarter_of_the_level_bounds(orc, arb, mesh, nlv, KE, x, N, rng, lab, no_void_rows=False):
    """the float64 oracle within a QUARTER of every level bound on one mesh, design and boundary condition: the products, the
    Jacobi diagonal, the Chebyshev steps, the residual and the transfers of every level -> (mg, amg)"""
    from oracle.ke_effective import ke_effective, ke_krylov
    ex, ey, ez = mesh
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    assert set(np.unique(x)) <= {rw.XMIN, 1.0} and (x == 1.0).any() and (x == rw.XMIN).any()
    E = orc.simp(x)
    mg = orc.MG(nx, ny, nz, 3, nlv)
    mg.assemble(KE, E, N)
    amg = arb.MG(nx, ny, nz, 3, nlv)
    amg.assemble(ld(KE), ld(E), ld(N))
    free = N != 0
    # ---- level 0: the oracle on KE against the arbiter on the packed forms the kernels apply (their distance from KE is
    # part of the bound, and must not eat it)
    u = rng.standard_normal(3 * nx * ny * nz)
    s0 = rw.scale_fine(orc, nx, ny, nz, KE, E, u) * free
    y = orc.matfree_apply(nx, ny, nz, 3, KE, E, N, u)
    assert np.array_equal(y[~free], u[~free])
    for name, K in (("apply", ke_effective(KE)), ("apply_krylov", ke_krylov(KE))):
        ya = arb.matfree_apply(nx, ny, nz, 3, ld(K), ld(E), ld(N), ld(u))
        note("fine", rw.assert_rowwise(y, ya, s0, rw.C_FINE / 4, {"label": "oracle %s %s" % (name, lab), "dims": (nx, ny, nz)}))
    assert s0[free].min() < 1e-6 * s0.max() or no_void_rows       # the rows this file is about exist
    # ---- coarser levels, one Chebyshev step on every level, transfers
    for l in range(nlv):
        dims = rw.level_dims(nx, ny, nz, l)
        n = mg.size(l)
        u, b = rng.standard_normal(n), rng.standard_normal(n)
        sl = rw.scale_level(orc, mg, l, (nx, ny, nz), KE, E, N, u)
        ya = amg.apply(l, ld(u))
        if l > 0:
            note("level", rw.assert_rowwise(mg.apply(l, u), ya, sl, rw.c_level(l) / 4, {"label": "oracle level %d %s" % (l, lab), "dims": dims}))
        da = np.asarray(amg.diag(l), dtype=np.float64)
        note("diag%d" % min(l, 1), rw.assert_rowwise(mg.diag(l), amg.diag(l), np.abs(da), rw.c_diag(l) / 4, {"label": "oracle diagonal level %d %s" % (l, lab), "dims": dims}))
        dinv = 1.0 / mg.diag(l)
        lam = mg.lam(l)
        lmin = mg.lam_min(l) if (l == nlv - 1 and l > 0) else 0.1 * lam
        theta = 0.5 * (1.1 * lam + lmin)
        for zero in (True, False):
            x0 = np.zeros(n) if zero else u
            xa = ld(x0) + ld(dinv) * (ld(b) - (0 if zero else ya)) / np.longdouble(theta)
            sc = rw.scale_smooth(0.0 if zero else sl, dinv, 1.0 / theta, b, x0)
            note("smooth", rw.assert_rowwise(mg.smooth(l, b, x0, 1, zero), xa, sc, rw.c_smooth(l) / 4,
                                             {"label": "oracle Chebyshev step level %d zero %d %s" % (l, zero, lab), "dims": dims}))
        # ---- the V-cycle's residual b - A x, and step k of a sweep from the oracle's own x_{k-1}, x_{k-2} (rw.c_smooth_k)
        sb = np.abs(b) + sl
        note("resid%d" % l, rw.assert_rowwise(b - mg.apply(l, u), ld(b) - ya, sb, rw.c_resid(l) / 4,
                                              {"label": "oracle residual level %d %s" % (l, lab), "dims": dims}))
        delta = 0.5 * (1.1 * lam - lmin)
        for zero in (True, False):
            x0 = np.zeros(n) if zero else u
            xs = {0: x0}
            for k in (2, 3, 4) + ((20,) if l == nlv - 1 else ()):
                for j in (k - 2, k - 1, k):
                    if j not in xs:
                        xs[j] = mg.smooth(l, b, x0, j, zero)
                c1, c2 = rw.cheb_coeffs(theta, delta, k)
                x1, x2 = xs[k - 1], xs[k - 2]
                xa = rw.step_k_ref(x1, x2, c1, c2, dinv, b, amg.apply(l, ld(x1)))
                sc = rw.scale_smooth_k(rw.scale_level(orc, mg, l, (nx, ny, nz), KE, E, N, x1), dinv, c1, c2, b, x1, x2)
                note("smooth_k%d" % l, rw.assert_rowwise(xs[k], xa, sc, rw.c_smooth_k(l) / 4,
                                                         {"label": "oracle Chebyshev step %d level %d zero %d %s" % (k, l, zero, lab), "dims": dims}))
        if l + 1 < nlv:
            rf, xc = rng.standard_normal(n), rng.standard_normal(mg.size(l + 1))
            note("restrict", rw.assert_rowwise(mg.restrict(l, rf), amg.restrict(l, ld(rf)), rw.scale_restrict(mg, l, rf), rw.C_RESTRICT / 4,
                                               {"label": "oracle restrict %d %s" % (l, lab), "dims": rw.level_dims(nx, ny, nz, l + 1)}))
            note("prolong", rw.assert_rowwise(b + mg.prolong(l, xc), ld(b) + amg.prolong(l, ld(xc)), rw.scale_prolong_add(mg, l, xc, b), rw.C_PROLONG / 4,
                                              {"label": "oracle prolong_add %d %s" % (l, lab), "dims": dims}))
    return mg, amg


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("kind", rw.SLAB_GENERATORS)
def test_oracle_within_a_quarter_of_every_bound(orc, arb, kind, mesh):
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    x = rw.design(kind, ex, ey, ez, kz=4, nranks=2)          # (the two seam designs: two slabs of 6 and of 4 element layers)
    assert set(np.unique(x)) <= {rw.XMIN, 1.0} and (x == 1.0).any() and (x == rw.XMIN).any()
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    N, R = orc.cantilever_bc(nx, ny, nz, h)
    rng = np.random.default_rng(ex + ez)
    mg, amg = quarter_of_the_level_bounds(orc, arb, mesh, NLV, KE, x, N, rng, "%s %s" % (kind, mesh), kind == "one_void")
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


def test_planted_step_error_passes_rel_and_fails_rowwise(orc, arb):
    """step 7 of a sweep from the zero guess (the longest sweep test_chebyshev_smoother runs), restated in numpy (float64) from
    the oracle's x_6 and x_5 on 31 x 17 x 9 elements, blocks + checkerboard: it holds the row-wise bound.  With the c1 term dropped
    on every row whose scale is below 1e-6 of the largest it still passes rel() <= 1e-10 and fails the row-wise assertion.
    Which rows those are: dinv ~ 1 / E, so under a right-hand side of one size the VOID rows carry iterates 1e9 times larger
    than the rows that touch a solid element, and rel() measures everything against them; the rows of small scale are the
    4923 that touch solid material.  (The same error planted into step 2 measures 5.8e-10 under rel(): E_void / E_solid = 2e-9
    times c1 = 0.53; the direction shrinks from step to step, 8e-11 at step 7.)"""
    ex, ey, ez, k = 31, 17, 9, 7
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    x = np.maximum(rw.design("blocks", ex, ey, ez), rw.design("checker", ex, ey, ez))
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    N, _ = orc.cantilever_bc(nx, ny, nz, h)
    E = orc.simp(x)
    mg, amg = orc.MG(nx, ny, nz, 3, 1), arb.MG(nx, ny, nz, 3, 1)
    mg.assemble(KE, E, N)
    amg.assemble(ld(KE), ld(E), ld(N))
    b = np.random.default_rng(1).standard_normal(3 * nx * ny * nz)
    lam = mg.lam(0)
    theta, delta = 0.5 * (1.1 * lam + 0.1 * lam), 0.5 * (1.1 * lam - 0.1 * lam)
    c1, c2 = rw.cheb_coeffs(theta, delta, k)
    dinv = 1.0 / mg.diag(0)
    x1, x2 = mg.smooth(0, b, np.zeros_like(b), k - 1, True), mg.smooth(0, b, np.zeros_like(b), k - 2, True)
    Ax1 = mg.apply(0, x1)
    step = lambda c1_rows: x1 + (c1_rows * (x1 - x2) + c2 * (dinv * (b - Ax1)))
    xa = rw.step_k_ref(x1, x2, c1, c2, dinv, b, amg.apply(0, ld(x1)))
    sc = rw.scale_smooth_k(rw.scale_fine(orc, nx, ny, nz, KE, E, x1, N), dinv, c1, c2, b, x1, x2)
    w = {"label": "planted step", "dims": (nx, ny, nz)}
    good = step(c1)
    assert rw.assert_rowwise(good, xa, sc, rw.c_smooth_k(0) / 4, w) <= 8.0
    assert rw.rel(good, mg.smooth(0, b, np.zeros_like(b), k, True)) <= 1e-14          # the restatement is the oracle's step
    small = sc < 1e-6 * sc.max()
    assert small.sum() > 1000 and (~small).sum() > 1000
    bad = step(np.where(small, 0.0, c1))
    assert rw.rel(bad, good) <= 1e-10 and rw.rel(bad, np.asarray(xa, dtype=np.float64)) <= 1e-10
    with pytest.raises(AssertionError, match=r"rows beyond %g eps scale" % rw.c_smooth_k(0)):
        rw.assert_rowwise(bad, xa, sc, rw.c_smooth_k(0), w)
    assert rw.achieved(bad, xa, sc) >= 1e6


# =====================================================================================================================
# z-slabs: the cases, designs and boundary conditions of rw.SLAB_FINE / rw.SLAB_COARSE / rw.SLAB_GENERATORS
# =====================================================================================================================
SLAB_CASES = [(mesh, ranks, 1) for mesh, ranks in rw.SLAB_FINE] + list(rw.SLAB_COARSE)


@pytest.mark.parametrize("case", range(len(SLAB_CASES)))
def test_oracle_within_a_quarter_on_the_slab_cases(orc, arb, case):
    """every mesh of rw.SLAB_FINE and rw.SLAB_COARSE with its own level count, both boundary conditions, the seven designs (the
    seam designs with the case's rank count): the oracle within a quarter of the one-rank constants the slab forms are held to,
    and dfdx of a seeded state"""
    mesh, nranks, nlv = SLAB_CASES[case]
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    for scattered in (0, 1):
        N, _ = rw.slab_bc(orc, nx, ny, nz, h, scattered, 15000 + 10 * case + scattered)
        for kind in rw.SLAB_GENERATORS:
            x = rw.design(kind, ex, ey, ez, 4, nranks)
            rng = np.random.default_rng(100 * case + scattered)
            lab = "%s %s %d levels %s" % (kind, mesh, nlv, "scattered" if scattered else "cantilever")
            quarter_of_the_level_bounds(orc, arb, mesh, nlv, KE, x, N, rng, lab, kind == "one_void")
            U = rng.standard_normal(3 * nx * ny * nz)
            _, _, df, _ = orc.compliance_sens(nx, ny, nz, KE, U, x)
            _, _, dfa, _ = arb.compliance_sens(nx, ny, nz, ld(KE), ld(U), ld(x))
            note("dfdx", rw.assert_rowwise(df, dfa, rw.scale_dfdx(nx, ny, nz, KE, U, x), rw.C_DFDX / 4, {"label": "oracle dfdx " + lab, "dims": mesh, "dof": 0}))
    print("measured oracle-vs-arbiter constants so far:", {k: round(v, 3) for k, v in MEASURED.items()})


def test_slab_partitions_tile_every_level_once():
    """SlabPartition on every slab case: on every level the ranks' owned node planes and element layers cover the mesh exactly
    once, a local array is its owned planes plus one ghost plane per neighbour, and the seam designs are what their names say"""
    from topopt_in_petsc_amd.partition import SlabPartition
    for mesh, nranks, nlv in SLAB_CASES:
        ex, ey, ez = mesh
        assert ez % nranks == 0 and (ez // nranks) % (1 << (nlv - 1)) == 0 and ex % (1 << (nlv - 1)) == 0 and ey % (1 << (nlv - 1)) == 0
        assert rw.slab_owned_planes(ez + 1, nranks) == [SlabPartition(ex + 1, ey + 1, ez + 1, r, nranks).n_owned_nodes // ((ex + 1) * (ey + 1)) for r in range(nranks)]
        for l in range(nlv):
            nodes, elems = np.zeros(((ez >> l) + 1), dtype=int), np.zeros(ez >> l, dtype=int)
            for r in range(nranks):
                p = SlabPartition(ex + 1, ey + 1, ez + 1, r, nranks).level(l)
                assert (p.nx, p.ny, p.nz) == rw.level_dims(ex + 1, ey + 1, ez + 1, l)
                assert p.nz_local == (p.own_hi - p.own_lo + 1) + p.has_lo + p.has_hi
                nodes[p.node_z0 + p.own_lo:p.node_z0 + p.own_hi + 1] += 1
                elems[p.elem_z0:p.elem_z0 + p.ez_own] += 1
                g, o = p.global_slice(3), p.owned_slice(3)
                assert g.start + o.start == 3 * p.plane * (p.node_z0 + p.own_lo) and o.stop - o.start == 3 * p.n_owned_nodes
            assert (nodes == 1).all() and (elems == 1).all(), (mesh, l, nodes, elems)
        own = ez // nranks
        step = rw.design("seam_step", ex, ey, ez, 4, nranks).reshape(ez, -1)
        void = rw.design("seam_void", ex, ey, ez, 4, nranks).reshape(ez, -1)
        for r in range(1, nranks):
            below, above = (1.0, rw.XMIN) if r % 2 else (rw.XMIN, 1.0)
            assert (step[r * own - 1] == below).all() and (step[r * own] == above).all()
            assert (void[r * own - 1] == rw.XMIN).all() and (void[r * own] == rw.XMIN).all()
        assert (void == rw.XMIN).all(1).sum() == 2 * (nranks - 1)


def slab_restatement(orc, mesh, nranks, K, E, N, u, ghost_layer=None):
    """y = A u in float64 computed RANK BY RANK from slab-local arrays (cut with SlabPartition: the local node planes, the own
    element layers and the ghost element layer above), the owned rows gathered.  ghost_layer(rank, E_local, layer size) may
    replace the moduli of the ghost element layer: the planted errors"""
    from topopt_in_petsc_amd.partition import SlabPartition
    ex, ey, ez = mesh
    lay, out = ex * ey, []
    for r in range(nranks):
        p = SlabPartition(ex + 1, ey + 1, ez + 1, r, nranks)
        El = E[lay * p.elem_z0:lay * (p.elem_z0 + p.nz_local - 1)].copy()       # the layers between the local node planes
        if p.has_hi and ghost_layer is not None:
            El[-lay:] = ghost_layer(r, El, lay)
        g = p.global_slice(3)
        yl = orc.matfree_apply(p.nx, p.ny, p.nz_local, 3, K, El, N[g].copy(), u[g].copy())
        out.append(yl[p.owned_slice(3)])
    return np.concatenate(out)


@pytest.mark.parametrize("case", (0, 1))
def test_planted_seam_errors_pass_rel_and_fail_rowwise(orc, arb, case):
    """(16, 8, 6) and (33, 4, 9) on three ranks, the scattered Dirichlet mask, a float64 restatement that computes rank by rank
    from slab-local arrays.  As it stands it holds the row-wise bounds.  Planted:

    1. the ghost element layer above a seam taken from the wrong side (the rank's OWN top layer mirrored up).  On 0 / 1 designs
       this is all or nothing: on seam_void both layers are void and not one bit moves, on seam_step the seam rows gain or lose
       a solid layer and rel() fails too (asserted below: a gross error, which the older metric does see).  The error of this
       kind that rel() cannot see is a ghost layer whose VOID moduli are off -- by 1e-7 relative here, the figure of the
       single-rank commits: it passes rel() <= 1e-12 and fails assert_rowwise on seam_void (on seam_step every seam row
       touches a solid layer and the same plant is 1e-16 of the row: rightly within the bound).
    2. a seam plane's ghost contribution left out of the Jacobi diagonal: the product keeps its bits and the diagonal passes
       rel() <= 1e-9 (above a void layer: 2.4e-10), fails assert_rowwise on both.
    3. a seam node counted by both neighbours in the dot product u . A u: the vectors are untouched (rel() = 0), the value fails
       the dot bound rw.c_dot_slab on both designs on the seeded field, and on seam_void on the field of void rows only."""
    from topopt_in_petsc_amd.partition import SlabPartition
    mesh, nranks = rw.SLAB_FINE[case]
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    N, _ = rw.slab_bc(orc, nx, ny, nz, h, 1, 15000 + 10 * case + 1)
    u = np.random.default_rng(case).standard_normal(3 * nx * ny * nz)
    free = N != 0
    kd = np.diag(np.diag(KE.reshape(24, 24))).reshape(-1)
    w = {"label": "slab restatement", "dims": (nx, ny, nz)}
    for kind in ("seam_void", "seam_step"):
        x = rw.design(kind, ex, ey, ez, 4, nranks)
        E = orc.simp(x)
        s = rw.scale_fine(orc, nx, ny, nz, KE, E, u) * free
        ya = arb.matfree_apply(nx, ny, nz, 3, ld(KE), ld(E), ld(N), ld(u))
        ya64 = np.asarray(ya, dtype=np.float64)
        good = slab_restatement(orc, mesh, nranks, KE, E, N, u)
        assert np.array_equal(good, orc.matfree_apply(nx, ny, nz, 3, KE, E, N, u))     # rank by rank, the oracle's own rows
        assert rw.assert_rowwise(good, ya, s, rw.C_FINE / 4, w) <= 4.0
        # ---- 1. the ghost element layer from the wrong side: nothing or gross; its void moduli off by 1e-7: the blind spot
        mirrored = slab_restatement(orc, mesh, nranks, KE, E, N, u, lambda r, El, lay: El[-2 * lay:-lay])
        if kind == "seam_void":
            assert np.array_equal(mirrored, good)
        else:
            assert rw.rel(mirrored, ya64) > 1e-3
            with pytest.raises(AssertionError, match="rows beyond"):
                rw.assert_rowwise(mirrored, ya, s, rw.C_FINE, w)
        bad = slab_restatement(orc, mesh, nranks, KE, E, N, u, lambda r, El, lay: np.where(El[-lay:] < 1e-6, El[-lay:] * (1.0 + 1e-7), El[-lay:]))
        assert rw.rel(bad, ya64) <= 1e-12 and not np.array_equal(bad, good)
        if kind == "seam_void":
            with pytest.raises(AssertionError, match="rows beyond"):
                rw.assert_rowwise(bad, ya, s, rw.C_FINE, w)
            assert rw.achieved(bad, ya, s) >= 1e6
        else:       # every seam row of seam_step touches a solid layer: 1e-7 of a void term is 1e-16 of the row, no error at all
            rw.assert_rowwise(bad, ya, s, rw.C_FINE, w)
        # ---- 2. the Jacobi diagonal without the ghost layer's terms on the seam planes
        one = np.ones_like(u)
        dga = np.asarray(arb.matfree_apply(nx, ny, nz, 3, ld(kd), ld(E), ld(N), ld(one)))
        dg64 = dga.astype(np.float64)
        dgood = slab_restatement(orc, mesh, nranks, kd, E, N, one)
        assert rw.assert_rowwise(dgood, dga, np.abs(dg64), rw.c_diag(0) / 4, w) <= 16.0
        dbad = slab_restatement(orc, mesh, nranks, kd, E, N, one, lambda r, El, lay: np.zeros(lay))
        # (no test holds the diagonal under rel() today -- the product is untouched, rel() = 0 <= 1e-12 there; under rel() the
        # diagonal itself moves by half a void entry, 2.4e-10 of the largest: below the 1e-9 the suite asks of level_lambda)
        first = slice(0, 3 * nx * ny * (2 * (ez // nranks))) if kind == "seam_step" else slice(None)     # seam_step: the ghost layer above
        assert rw.rel(dbad[first], dg64[first]) <= 1e-9 and not np.array_equal(dbad[first], dgood[first])  # the SECOND seam is solid, a gross error
        with pytest.raises(AssertionError, match="rows beyond"):
            rw.assert_rowwise(dbad, dga, np.abs(dg64), rw.c_diag(0), w)
        # ---- 3. a seam node counted by both neighbours in u . A u
        parts = [SlabPartition(nx, ny, nz, r, nranks) for r in range(nranks)]
        void = (rw.scale_fine(orc, nx, ny, nz, KE, E, u, N) <= 1e-6 * s.max())
        c = rw.c_dot_slab([1] * nranks, [(p.n_owned_nodes + 255) // 256 for p in parts])
        for seeded, uu in ((True, u), (False, u * void)):
            y = slab_restatement(orc, mesh, nranks, KE, E, N, uu)
            terms = ld(uu) * ld(y)
            ref, size = terms.sum(), float(np.abs(terms).sum())
            dots = lambda lo: sum(float(np.dot(uu[3 * nx * ny * (p.node_z0 + lo(p)):3 * nx * ny * (p.node_z0 + p.own_hi + 1)],
                                               y[3 * nx * ny * (p.node_z0 + lo(p)):3 * nx * ny * (p.node_z0 + p.own_hi + 1)])) for p in parts)
            once, twice = dots(lambda p: p.own_lo), dots(lambda p: 0)
            assert np.count_nonzero(terms) > 100
            assert abs(np.longdouble(once) - ref) <= c * rw.EPS * size
            if seeded or kind == "seam_void":       # (the void-rows-only field is zero on the seam planes of seam_step: they touch solid layers)
                assert abs(np.longdouble(twice) - ref) > c * rw.EPS * size, (kind, once, twice)


# =====================================================================================================================
# the Helmholtz (PDE) filter's scalar hierarchy
# =====================================================================================================================
def pde_kf(orc, case, ratio):
    hx, hy, hz = rw.pde_box(case)
    return orc.pde_kf(hx, hy, hz, ratio * min(hx, hy, hz) / 2.0 / np.sqrt(3.0))[0]       # the filter's conversion of rmin


@pytest.mark.parametrize("m", range(len(rw.PDE_CASES) + 1))
def test_pde_oracle_within_a_quarter_of_every_bound(orc, arb, m):
    case = rw.PDE_CASES[m] if m < len(rw.PDE_CASES) else rw.PDE_SLAB3
    (ex, ey, ez), _, nlv, ratios = case
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    for r, ratio in enumerate(ratios):
        ref = rw.PdeRef(orc, arb, (nx, ny, nz), nlv, pde_kf(orc, case, ratio))
        mg, amg = ref.mg, ref.amg
        lab = "oracle pde mesh %s rmin/h %g " % ((ex, ey, ez), ratio)
        for l in range(nlv):
            dims = rw.level_dims(nx, ny, nz, l)
            w = {"dims": dims, "dof": 1}
            inp = rw.pde_inputs(dims, rw.pde_seed(m, r, l))
            for name, u in inp.items():
                if name == "b":
                    continue
                note("pde level %d" % l, rw.assert_rowwise(mg.apply(l, u), amg.apply(l, ld(u)), ref.scale(l, u), rw.c_pde_level(l) / 4,
                                                    dict(w, label=lab + "level %d apply %s" % (l, name))))
            da = np.asarray(amg.diag(l), dtype=np.float64)
            assert (da > 0).all()
            note("pde diag %d" % l, rw.assert_rowwise(mg.diag(l), amg.diag(l), np.abs(da), rw.c_pde_diag(l) / 4, dict(w, label=lab + "level %d diagonal" % l)))
            note("pde diag majorant / entry %d" % l, float((ref.mga.diag(l) / da).max()))
            u, b = inp["normal"], inp["b"]
            dinv, theta = 1.0 / mg.diag(l), ref.theta(l, mg.lam(l), mg.lam_min(l))
            # the estimates the device is held to at rel 1e-9 are that well determined: the arbiter's agree with the oracle's
            assert mg.lam(l) == pytest.approx(float(amg.lam(l)), rel=1e-10), (lab, l)
            ya, sl = amg.apply(l, ld(u)), ref.scale(l, u)
            for zero in (True, False):
                x0 = np.zeros_like(u) if zero else u
                xa = ld(x0) + ld(dinv) * (ld(b) - (0 if zero else ya)) / np.longdouble(theta)
                sc = rw.scale_smooth(0.0 if zero else sl, dinv, 1.0 / theta, b, x0)
                note("pde smooth %d" % l, rw.assert_rowwise(mg.smooth(l, b, x0, 1, zero), xa, sc, rw.c_pde_smooth(l) / 4,
                                                     dict(w, label=lab + "level %d Chebyshev step zero %d" % (l, zero))))
            delta = theta - (mg.lam_min(l) if (l == nlv - 1 and l > 0) else 0.1 * mg.lam(l))
            for zero in (True, False):
                x0 = np.zeros_like(u) if zero else u
                xs = {0: x0}
                for k in (2, 3):
                    for j in (k - 1, k):
                        if j not in xs:
                            xs[j] = mg.smooth(l, b, x0, j, zero)
                    c1, c2 = rw.cheb_coeffs(theta, delta, k)
                    x1, x2 = xs[k - 1], xs[k - 2]
                    xa = rw.step_k_ref(x1, x2, c1, c2, dinv, b, amg.apply(l, ld(x1)))
                    sc = rw.scale_smooth_k(ref.scale(l, x1), dinv, c1, c2, b, x1, x2)
                    note("pde smooth_k %d" % l, rw.assert_rowwise(xs[k], xa, sc, rw.c_pde_smooth_k(l) / 4,
                                                           dict(w, label=lab + "level %d Chebyshev step %d zero %d" % (l, k, zero))))
            if l + 1 < nlv:
                cd = rw.level_dims(nx, ny, nz, l + 1)
                xc = rw.pde_inputs(cd, rw.pde_seed(m, r, l + 1))
                for name in rw.PDE_FIELDS:
                    note("pde restrict", rw.assert_rowwise(mg.restrict(l, inp[name]), amg.restrict(l, ld(inp[name])), rw.scale_restrict(mg, l, inp[name]),
                                                           rw.C_RESTRICT / 4, {"dims": cd, "dof": 1, "label": lab + "restrict %d %s" % (l, name)}))
                    note("pde prolong", rw.assert_rowwise(b + mg.prolong(l, xc[name]), ld(b) + amg.prolong(l, ld(xc[name])), rw.scale_prolong_add(mg, l, xc[name], b),
                                                          rw.C_PROLONG / 4, dict(w, label=lab + "prolong_add %d %s" % (l, name))))
    # element <-> node: a float64 restatement in the kernels' order of summation against the same in 80-bit arithmetic, held to
    # the kernels' own bound (7 rounded additions; there is no oracle function to hold to a quarter of it)
    rng = np.random.default_rng(rw.pde_seed(m, 9, 9))
    for x, u in ((rng.random(ex * ey * ez), rng.random(nx * ny * nz)), (np.ones(ex * ey * ez), np.ones(nx * ny * nz))):
        note("pde T", rw.assert_rowwise(rw.pde_T(x, ex, ey, ez), rw.pde_T(x, ex, ey, ez, np.longdouble), rw.pde_T(np.abs(x), ex, ey, ez), rw.C_PDE_T,
                                        {"dims": (nx, ny, nz), "dof": 1, "label": "numpy T %s" % (case[0],)}))
        note("pde T", rw.assert_rowwise(rw.pde_Tt(u, ex, ey, ez), rw.pde_Tt(u, ex, ey, ez, np.longdouble), rw.pde_Tt(np.abs(u), ex, ey, ez), rw.C_PDE_T,
                                        {"dims": (ex, ey, ez), "dof": 0, "label": "numpy T^T %s" % (case[0],)}))
    print("measured oracle-vs-arbiter constants so far:", {k: round(v, 3) for k, v in MEASURED.items()})


def table_hierarchy(kf, nlv, swap_xy=False, perturb=None):
    """the class tables of the levels from the 8 x 8 matrices (rw.pde_galerkin, rw.pde_table).  swap_xy: every table indexed with
    the x and y axes exchanged, classes and offsets alike; perturb = (level, class, offset, relative error)"""
    out, K = [], np.asarray(kf, dtype=np.float64).reshape(8, 8)
    for l in range(nlv):
        W = rw.pde_table(K)
        if swap_xy:
            W = W.reshape(3, 3, 3, 3, 3, 3).transpose(0, 2, 1, 3, 5, 4).reshape(27, 27).copy()
        if perturb and perturb[0] == l:
            W[perturb[1], perturb[2]] *= 1.0 + perturb[3]
        out.append(W)
        K = rw.pde_galerkin(K)
    return out


def test_pde_planted_table_errors(orc, arb):
    """Why the cubes are blind and what the anisotropic box sees: the class table with x and y exchanged gives the SAME numbers
    on a cube (K_f is invariant under permutations of the axes) and fails assert_rowwise on the box (0.05, 0.04, 0.03); one weight
    of one edge class of level 1 off by 2^-40 relative fails it too -- the converged filter cannot see that one at all (level 1
    is part of the preconditioner only)."""
    nlv = 3
    for m, blind in ((0, False), (1, True)):
        case = rw.PDE_CASES[m]
        (ex, ey, ez), _, _, _ = case
        nx, ny, nz = ex + 1, ey + 1, ez + 1
        kf = pde_kf(orc, case, 2.56)
        ref = rw.PdeRef(orc, arb, (nx, ny, nz), nlv, kf)
        good, swapped = table_hierarchy(kf, nlv), table_hierarchy(kf, nlv, swap_xy=True)
        for l in range(nlv):
            dims = rw.level_dims(nx, ny, nz, l)
            u = rw.pde_inputs(dims, rw.pde_seed(m, 1, l))["normal"]
            ya, s = ref.amg.apply(l, ld(u)), ref.scale(l, u)
            w = {"dims": dims, "dof": 1, "label": "table restatement mesh %s level %d" % (case[0], l)}
            y = rw.pde_table_apply(good[l], dims, u)
            rw.assert_rowwise(y, ya, s, rw.c_pde_level(l), w)                      # the restatement is the operator
            ys = rw.pde_table_apply(swapped[l], dims, u)
            if blind:
                assert rw.achieved(ys, ld(y), s) <= 8.0                            # the same weights, to the last bits of kf's symmetry
                rw.assert_rowwise(ys, ya, s, rw.c_pde_level(l), w)
            else:
                with pytest.raises(AssertionError, match=r"node \(\d+, \d+, \d+\)"):
                    rw.assert_rowwise(ys, ya, s, rw.c_pde_level(l), w)
    # one weight of an edge class (x low, y low, z inside: class (1 3 + 0) 3 + 0 = 9; its +z neighbour: offset 2 9 + 4 = 22) of
    # level 1 on the anisotropic box
    case = rw.PDE_CASES[0]
    (ex, ey, ez), _, _, _ = case
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    kf = pde_kf(orc, case, 2.56)
    ref = rw.PdeRef(orc, arb, (nx, ny, nz), nlv, kf)
    bad = table_hierarchy(kf, nlv, perturb=(1, 9, 22, 2.0 ** -40))
    dims = rw.level_dims(nx, ny, nz, 1)
    u = rw.pde_inputs(dims, rw.pde_seed(0, 1, 1))["normal"]
    assert bad[1][9, 22] != 0.0
    with pytest.raises(AssertionError, match=r"node \(0, 0, \d+\)"):
        rw.assert_rowwise(rw.pde_table_apply(bad[1], dims, u), ref.amg.apply(1, ld(u)), ref.scale(1, u), rw.c_pde_level(1),
                          {"dims": dims, "dof": 1, "label": "one weight of level 1 off by 2^-40"})


# =====================================================================================================================
# the admission window of the exact coarse solve as a table (tests/test_gpu_coarse_direct.py)
# =====================================================================================================================
def test_coarse_direct_geometry_table():
    """rw.cd_geom / rw.cd_rows reproduce the figures the table was written from, the window's edges, and the geometries the
    older tests reach (tests/test_gpu_parity.py: KB 6, 9, 10)"""
    want = {((4, 4, 48), 3): ((2, 2, 13), 156, 1, 5, 4), ((8, 8, 24), 3): ((3, 3, 7), 189, 2, 6, 3), ((12, 12, 28), 3): ((4, 4, 8), 384, 3, 12, 0),
            ((28, 12, 20), 3): ((8, 4, 6), 576, 4, 18, 0), ((20, 20, 20), 3): ((6, 6, 6), 648, 5, 21, 24), ((28, 28, 12), 3): ((8, 8, 4), 768, 7, 24, 0),
            ((28, 32, 16), 3): ((8, 9, 5), 1080, 8, 34, 8), ((36, 36, 16), 3): ((10, 10, 5), 1500, 11, 47, 4),
            ((36, 40, 44), 3): ((10, 11, 12), 3960, 12, 124, 8), ((64, 32, 32), 4): ((9, 5, 5), 675, 6, 22, 29)}
    assert [(c[0], c[1]) for c in rw.CD_CASES] == list(want)
    for mesh, nlv, rows1, rows2 in rw.CD_CASES:
        assert rw.cd_geom(mesh, nlv) == want[(mesh, nlv)], (mesh, rw.cd_geom(mesh, nlv))
        rows = want[(mesh, nlv)][1]
        assert rows2 == rows == rw.cd_rows(mesh, nlv, 2) and rows1 == rw.cd_rows(mesh, nlv, 1) == (rows if rows > 448 else 0)
        assert rw.cd_rows(mesh, nlv, 0) == 0
    # every band width 1 .. 12, a padded and an unpadded last block, more than 69 blocks, three cases below 449 rows
    assert sorted({rw.cd_geom(c[0], c[1])[2] for c in rw.CD_CASES}) == [1, 2, 3, 4, 5, 6, 7, 8, 11, 12]
    assert {rw.cd_geom(c[0], c[1])[4] == 0 for c in rw.CD_CASES} == {True, False}
    assert max(rw.cd_geom(c[0], c[1])[3] for c in rw.CD_CASES) == 124 and sum(c[2] == 0 for c in rw.CD_CASES) == 3
    # rejected: too many rows (at an admissible band), too few rows
    assert rw.cd_geom((40, 36, 48), 3)[1:3] == (4290, 12) and rw.cd_geom((8, 8, 8), 3)[1] == 81
    assert all(rw.cd_rows(m, n, cd) == 0 for m, n in rw.CD_REJECTED for cd in (1, 2))
    # the band too wide (test_coarsest_level_too_wide_for_the_exact_solve_falls_back): 11 x 11 x 7 nodes, 13 blocks
    assert rw.cd_geom((40, 40, 24), 3)[2] == 13 and rw.cd_rows((40, 40, 24), 3, 2) == 0
    # the older tests' geometries: test_coarsest_level_solved_exactly and test_exact_coarse_solve_inverse_forms_agree
    old = [((64, 32, 32), 4), ((48, 24, 24), 3), ((64, 64, 64), 4), ((24, 40, 24), 3), ((32, 32, 32), 3)]
    geo = [rw.cd_geom(m, n) for m, n in old]
    assert sorted({g[2] for g in geo}) == [6, 9, 10] and sorted({g[4] for g in geo}) == [9, 15, 21, 29]
    assert min(g[3] for g in geo) == 22 and max(g[3] for g in geo) == 69
    assert all(rw.cd_rows(m, n, 1) == g[1] for (m, n), g in zip(old, geo))
    # the design sequence of the stale-data test: A, B, A, B first, and every design once after that
    assert rw.CD_SEQUENCE[:4] == ("blocks", "checker", "blocks", "checker") and set(rw.CD_SEQUENCE) == set(rw.CD_DESIGNS)
    assert rw.CD_CASES[rw.CD_SETUP_CASES[0]][:2] == ((64, 32, 32), 4) and rw.CD_CASES[rw.CD_SETUP_CASES[1]][:2] == ((28, 12, 20), 3)
