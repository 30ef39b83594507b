"""Linear buckling: the stress-stiffness operator, its two derivatives, the mode solver for the indefinite pencil B phi = mu A phi,
the sensitivity of J = (sum mu_i^P)^(1/P) with its adjoint solve, and the driver's constraint, against the numpy / scipy
restatement tests/buckling_ref.py.

Bounds.  Kernels (geom_apply, geom_sensitivity, geom_adjoint_rhs): the result lies within 16 x the distance of the float64
restatement from the 80-bit one, and at least 64 * 2^-53, relative to the result's maximum.  Identities: a dot product of such a
result with a vector v is off by that bound times sum|v| max|result|; 256 * 2^-53 of the two sides' such products.  Eigenvalues: the Ritz
values of the largest positive eigenvalues are LOWER bounds, mu_i <= mu_ref (1 + 1e-12), and 1 - mu_i / mu_ref <= max(1e-10, 16 x
the distance of the restatement's own subspace iteration from eigh); mu_ref are eigh's values refined by an 80-bit Rayleigh
quotient of eigh's vectors.  The modes are computed on the restatement's state u (a sparse direct solve), so that both sides hold
the same B; the sensitivity tests run on the device's own state.  Sensitivity: 1e-6 against the restated gradient, 1e-5 against
the device's own central difference (tests/test_buckling_oracle.py prints the restatement's own distance from its central
difference: 1e-8 at most).  Every figure is printed with its bound before it is asserted."""
import numpy as np
import pytest

from tests import buckling_ref as ref

pytestmark = pytest.mark.gpu

LD = ref.LD
U53 = 2.0 ** -53
EMAX_K = 2.5          # kernels: not 1, so that a dropped factor shows
WEIGHTS = [0.75, -0.5, 0.0]
DESIGNS = {"01": ref.design_01, "mixed": ref.design_mixed}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _check(label, got, bound):
    print("%-92s measured %.3e   bound %.1e" % (label, got, bound))
    assert got <= bound, (label, got, bound)


_CACHE = {}


def _kcase(tp, idx, kind):
    """per kernel mesh and design, made once and left alone: grid, solver object with the cantilever's supports, design, a smooth
    state and three smooth fields (all times N), the assembled coefficients"""
    if ("k", idx, kind) in _CACHE:
        return _CACHE[("k", idx, kind)]
    ne, h = ref.KERNEL_MESHES[idx]
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
    le.SetUpLoadAndBC()
    nnode = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
    N = le.N.cpu().numpy()
    assert (N == 0).any() and np.array_equal(N, ref.clamp_N(ne))
    U = ref.smooth_field(ne, 300 + idx) * N
    V = [ref.smooth_field(ne, 400 + 10 * idx + l) * N for l in range(3)]
    x = DESIGNS[kind](ne, 40 + idx)
    if kind == "mixed":
        assert (x < 0.1).mean() >= 0.3
    c = dict(grid=grid, le=le, ne=ne, h=h, dofs=ref.elem_dofs(*ne), nel=x.size, nnode=nnode, N=N, U=U, Ud=_dev(U),
             V=V, Vd=[_dev(v) for v in V], x=x, xd=_dev(x), tag="%dx%dx%d %s" % (ne + (kind,)))
    le.GeomAssemble(c["xd"], EMAX_K, ref.PENAL, U=c["Ud"])
    _CACHE[("k", idx, kind)] = c
    return c


KCASES = [(i, k) for i in range(len(ref.KERNEL_MESHES)) for k in ("01", "mixed")]


# ---- 0
def test_tables_against_the_restatement(tp):
    for idx in (0, 3):
        c = _kcase(tp, idx, "mixed")
        gn, cb = c["le"].GeomTables()
        gr, cr, _, _ = ref.tables(c["h"], ref.NU, LD)
        _check("%s max|gradN - ref| / max|ref|" % c["tag"], float(np.abs(gn - gr).max() / np.abs(gr).max()), 8 * U53)
        _check("%s max|C0 B - ref| / max|ref|" % c["tag"], float(np.abs(cb - cr).max() / np.abs(cr).max()), 16 * U53)


# ---- 1
@pytest.mark.parametrize("idx,kind", KCASES)
def test_geom_apply_against_the_restatement(tp, idx, kind):
    c = _kcase(tp, idx, kind)
    g, le = c["grid"], c["le"]
    args = (c["x"], c["dofs"], c["nnode"], c["h"], ref.NU, EMAX_K, ref.PENAL, c["N"], c["U"])
    ys = []
    for l, (v, vd) in enumerate(zip(c["V"][:2], c["Vd"][:2])):
        yr, y64 = ref.geom_apply(*args, v, LD), ref.geom_apply(*args, v, np.float64)
        top = float(np.abs(yr).max())
        bound = max(16 * float(np.abs(y64 - yr).max()) / top, 64 * U53)
        y = g.node_vec(3)
        y.fill_(7.0)
        le.GeomMult(vd, y)
        yh = y.cpu().numpy()
        _check("%s field %d max|G phi - ref| / max|ref|" % (c["tag"], l), float(np.abs(yh - yr).max()) / top, bound)
        assert not yh[c["N"] == 0].any(), "N G N phi is not zero on the clamped dofs: N is missing on the left"
        ys.append((yh, top, bound))
    (Gu, _, bu), (Gv, _, bv) = ys
    u, v = c["V"][0].astype(LD), c["V"][1].astype(LD)
    a, b = float(u @ Gv.astype(LD)), float(v @ Gu.astype(LD))
    scale = float(np.abs(u) @ np.abs(Gv).astype(LD))
    _check("%s |phi^T (G psi) - psi^T (G phi)| / sum |phi| |G psi|" % c["tag"], abs(a - b) / scale, max(bu, bv))


def test_geom_apply_repeats_bit_for_bit(tp):
    import torch
    c = _kcase(tp, 3, "mixed")
    y1, y2 = c["le"].GeomMult(c["Vd"][0]), c["le"].GeomMult(c["Vd"][0])
    assert torch.equal(y1, y2) and float(y1.abs().max()) > 0


# ---- 2
@pytest.mark.parametrize("idx,kind", KCASES)
def test_geom_sensitivity_against_the_restatement(tp, idx, kind):
    c = _kcase(tp, idx, kind)
    le, scale = c["le"], -2.0
    args = (c["x"], c["dofs"], c["h"], ref.NU, EMAX_K, ref.PENAL, c["N"], c["U"], c["V"], WEIGHTS, scale)
    tr, t64 = ref.geom_sens(*args, LD), ref.geom_sens(*args, np.float64)
    top = float(np.abs(tr).max())
    bound = max(16 * float(np.abs(t64 - tr).max()) / top, 64 * U53)
    pre = np.random.default_rng(idx).uniform(-1.0, 1.0, c["nel"]) * top
    d = _dev(pre)
    le.GeomSensitivity(c["Vd"], WEIGHTS, c["xd"], c["Ud"], EMAX_K, ref.PENAL, scale, d)
    got = d.cpu().numpy()
    _check("%s max|out - (pre + term)| / max|term|" % c["tag"], float(np.abs(got - (pre.astype(LD) + tr)).max()) / top, bound)
    assert float(np.abs(got - tr).max()) / top > 0.1, "the kernel overwrote out instead of adding to it"
    void = c["x"] == 0.0
    if void.any():
        assert np.array_equal(got[void], pre[void]), "a void element changed its entry"
    t1 = ref.geom_sens(*args[:8], c["V"][:1], [1.0], 1.0, LD)        # w = None: all weights 1
    d1 = c["grid"].elem_vec(0.0)
    le.GeomSensitivity(c["Vd"][:1], None, c["xd"], c["Ud"], EMAX_K, ref.PENAL, 1.0, d1)
    _check("%s w=None max|out - term| / max|term|" % c["tag"], float(np.abs(d1.cpu().numpy() - t1).max() / np.abs(t1).max()), bound)


# ---- 3
@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("idx,kind", KCASES)
def test_geom_adjoint_rhs_against_the_restatement(tp, idx, kind, nf):
    c = _kcase(tp, idx, kind)
    le = c["le"]
    w = WEIGHTS[:nf] if nf > 1 else [1.0]
    args = (c["x"], c["dofs"], c["nnode"], c["h"], ref.NU, EMAX_K, ref.PENAL, c["N"], c["V"][:nf], w, -2.0)
    rr, r64 = ref.geom_adjoint_rhs(*args, LD), ref.geom_adjoint_rhs(*args, np.float64)
    top = float(np.abs(rr).max())
    bound = max(16 * float(np.abs(r64 - rr).max()) / top, 64 * U53)
    out = c["grid"].node_vec(3)
    out.fill_(7.0)
    le.GeomAdjointRHS(c["Vd"][:nf], w if nf > 1 else None, c["xd"], EMAX_K, ref.PENAL, -2.0, out)
    got = out.cpu().numpy()
    _check("%s %d field(s) max|rhs - ref| / max|ref|" % (c["tag"], nf), float(np.abs(got - rr).max()) / top, bound)
    clamped = c["N"] == 0
    assert np.abs(rr[clamped]).max() > 0 and got[clamped].any()     # supports not applied: the clamped rows carry values


# ---- 4
@pytest.mark.parametrize("idx,kind", KCASES)
def test_identities_on_the_device(tp, idx, kind):
    """U^T adjoint_rhs(phi) = phi^T G(U) phi (G is linear in U) and sum_e (x_e / p) sens_e = phi^T G phi (G_e is x_e^p times a
    matrix free of x), all three from the device's own kernels"""
    c = _kcase(tp, idx, kind)
    le, g = c["le"], c["grid"]
    phi, phid = c["V"][0], c["Vd"][0]
    Gphi = le.GeomMult(phid).cpu().numpy().astype(LD)
    quad = float(phi.astype(LD) @ Gphi)
    r = g.node_vec(3)
    le.GeomAdjointRHS([phid], None, c["xd"], EMAX_K, ref.PENAL, 1.0, r)
    rh = r.cpu().numpy().astype(LD)
    lhs = float(c["U"].astype(LD) @ rh)
    # every entry of r, of G phi and of the sensitivity is held to 64 * 2^-53 of its vector's maximum (or the restatement's own
    # float64 distance) by the tests above, so a dot product with v is off by that times sum|v| max|.|; 256 * 2^-53 of the two
    # sides' sum|v| max|.| covers both
    mag_q = float(np.abs(phi).sum() * np.abs(Gphi).max())
    mag_r = float(np.abs(c["U"]).sum() * np.abs(rh).max())
    _check("%s |U^T adjoint_rhs(phi) - phi^T G phi| / (sum|U| max|r| + sum|phi| max|G phi|)" % c["tag"], abs(lhs - quad) / (mag_r + mag_q), 256 * U53)
    s = g.elem_vec(0.0)
    le.GeomSensitivity([phid], None, c["xd"], c["Ud"], EMAX_K, ref.PENAL, 1.0, s)
    terms = c["x"].astype(LD) / LD(ref.PENAL) * s.cpu().numpy().astype(LD)
    mag_s = float(c["x"].sum() / ref.PENAL * s.abs().max())
    _check("%s |sum_e x_e / p sens_e - phi^T G phi| / (sum x_e / p max|sens| + sum|phi| max|G phi|)" % c["tag"],
           abs(float(terms.sum()) - quad) / (mag_s + mag_q), 256 * U53)
    assert abs(quad) > 1e-6 * float(np.abs(phi).astype(LD) @ np.abs(Gphi)), "the quadratic form vanishes: the identities compare nothing"


def test_void_elements_contribute_exactly_nothing(tp):
    import torch
    c = _kcase(tp, 1, "01")
    le, g = c["le"], c["grid"]
    zero = g.elem_vec(0.0)
    le.GeomAssemble(zero, EMAX_K, ref.PENAL, U=c["Ud"])
    y = le.GeomMult(c["Vd"][0])
    pre = _dev(np.random.default_rng(3).uniform(-1, 1, c["nel"]))
    s = pre.clone()
    le.GeomSensitivity(c["Vd"], WEIGHTS, zero, c["Ud"], EMAX_K, ref.PENAL, -2.0, s)
    r = g.node_vec(3)
    r.fill_(7.0)
    le.GeomAdjointRHS(c["Vd"], WEIGHTS, zero, EMAX_K, ref.PENAL, -2.0, r)
    le.GeomAssemble(c["xd"], EMAX_K, ref.PENAL, U=c["Ud"])          # leave the cached object as it was
    assert not y.any() and torch.equal(s, pre) and not r.any()
    # in the 0/1 design a node whose eight elements are all void sees nothing either
    yv = le.GeomMult(c["Vd"][0]).cpu().numpy().reshape(-1, 3)
    solid = np.zeros(c["nnode"], dtype=bool)
    solid[(c["dofs"][c["x"] > 0][:, ::3] // 3).ravel()] = True
    assert (~solid).any() and not yv[~solid].any()


def test_calls_before_assemble_are_refused(tp):
    grid = tp.Grid(4, 4, 4, 0.25)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
    le.SetUpLoadAndBC()
    v, x = grid.node_vec(3), grid.elem_vec(0.5)
    for call in (lambda: le.GeomMult(v), lambda: le.GeomSensitivity([v], None, x, v, 1.0, 3.0, 1.0, grid.elem_vec()),
                 lambda: le.GeomAdjointRHS([v], None, x, 1.0, 3.0, 1.0, grid.node_vec(3))):
        with pytest.raises(tp.TopOptError) as ei:
            call()
        assert ei.value.code == 1
    with pytest.raises(tp.TopOptError):
        le.BucklingVectors()
    grid.close()


# ---- 5
def _mcase(tp, orc, name):
    """per mode case, made once: device objects on an assembly of the design, the restatement's pencil, its eigh (refined), its own
    subspace iteration, and the device's modes on the restatement's state"""
    if ("m", name) in _CACHE:
        return _CACHE[("m", name)]
    c = dict(ref.MODE_CASES[name])
    ne, h, nev = c["ne"], c["h"], c["nev"]
    x = c["design"](ne, c["seed"])
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=c["nlvls"], nu=ref.NU, rtol=1e-12, max_it=2000))
    if c["load"] == "axial":
        le.SetUpLoadAndBC_Axial()
    else:
        le.SetUpLoadAndBC()
    # the oracle's KE, not the restatement's own: a bending mode's energy is what is left of 1e4 times as much that cancels
    # element by element, and one ulp of max|KE| in the reference's matrix moves mu by 3e-12 (measured)
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], ref.NU)).reshape(24, 24)
    P = ref.Pencil(ne, h, x, ref.clamp_N(ne), ref.case_load(c), ref.EMIN, ref.EMAX, ref.PENAL, ref.NU, KE=KE)
    assert np.array_equal(le.N.cpu().numpy(), P.N)
    _check("%s max|RHS - restated load|" % name, float(np.abs(le.RHS.cpu().numpy() - P.F).max()), 4 * U53 * float(np.abs(P.F).max()))
    xd = _dev(x)
    le.AssembleStiffnessMatrix(xd, ref.EMIN, ref.EMAX, ref.PENAL)
    mu64, Phi, mu_all = P.modes(nev + 1)
    mu = P.refine(Phi)
    th_ref = ref.subspace_iteration(P, nev, tol=1e-8)[0]
    own = float(np.abs(th_ref[:nev] / mu64[:nev] - 1).max())
    Ud = _dev(P.u)
    out = le.BucklingModes(nev, xd, ref.EMAX, ref.PENAL, U=Ud, tol=1e-8)
    c.update(grid=grid, le=le, x=x, xd=xd, P=P, mu=mu, mu64=mu64, mu_all=mu_all, Phi=Phi, own=own, out=out, Ud=Ud, tag=name)
    print("%s: eigh, largest positive %s; most negative %s; 80-bit refinement moves them by %s; the restatement's own subspace "
          "iteration is %.3e from eigh" % (name, " ".join("%.9e" % v for v in mu64), " ".join("%.6e" % v for v in mu_all[:3]),
                                          " ".join("%.2e" % float(v) for v in (mu / mu64 - 1)[:nev]), own))
    print("%s: device %s in %d iterations, %d solver iterations, residuals %s, gap %.3f; Ritz values %s"
          % (name, " ".join("%.9e" % v for v in out["mu"]), out["iters"], out["ksp_its"], " ".join("%.2e" % r for r in out["residuals"]),
             out["gap"], " ".join("%.4e" % v for v in out["ritz"])))
    _CACHE[("m", name)] = c
    return c


def _mode_checks(c):
    nev, P, out, name = c["nev"], c["P"], c["out"], c["tag"]
    assert max(out["residuals"]) <= 1e-8 and len(out["mu"]) == nev
    rel = [float(LD(t) / m - 1) for t, m in zip(out["mu"], c["mu"][:nev])]
    bound = max(1e-10, 16 * c["own"])
    for i, r in enumerate(rel):
        print("%s mode %d: mu / mu_ref - 1 = %+.3e (lower bound: <= +1e-12; accuracy bound -%.1e)" % (name, i, r, bound))
    assert all(r <= 1e-12 for r in rel), rel
    assert all(r >= -bound for r in rel), rel
    assert out["factor"] == pytest.approx(1.0 / out["mu"][0], rel=1e-15)
    vecs = [v.cpu().numpy() for v in c["le"].BucklingVectors()]
    assert len(vecs) == nev
    Av = [P.apply_ld(v)[0] for v in vecs]
    G = np.array([[float(vecs[i].astype(LD) @ Av[j]) for j in range(nev)] for i in range(nev)])
    _check("%s max|Phi^T A Phi - I|" % name, float(np.abs(G - np.eye(nev)).max()), 1e-12)
    return vecs


def test_buckling_modes_through_the_double_mode_of_a_square_column(tp, orc):
    c = _mcase(tp, orc, "column")
    mu, out = c["mu"], c["out"]
    assert float(abs(mu[1] / mu[0] - 1)) < 1e-8 and float(mu[2] / mu[1]) < 0.5
    vecs = _mode_checks(c)
    for i, v in enumerate(vecs):                              # any basis of the plane
        _check("column vector %d sine of the A-angle to the double mode's plane" % i, ref.subspace_angle(c["P"].A, c["Phi"][:, :2], v), 1e-4)
        assert not v[c["P"].N == 0].any()
    J, Jr = ref.Pencil.J_of(out["mu"]), ref.Pencil.J_of(mu[:2])
    rel = float(J / Jr - 1)
    print("column: J = %.12e, reference %.12e, J / J_ref - 1 = %+.3e; %d iterations" % (float(J), float(Jr), rel, out["iters"]))
    assert -max(1e-10, 16 * c["own"]) <= rel <= 1e-12
    ninth = np.sort(np.abs(c["mu_all"]))[::-1][8]
    print("column: |mu_9| / mu_2 = %.4f" % (ninth / c["mu64"][1]))


def test_buckling_modes_of_a_random_field(tp, orc):
    c = _mcase(tp, orc, "random")
    assert float(c["mu"][0] / c["mu"][1] - 1) >= 0.02 and float(c["mu"][2] / c["mu"][1]) < 0.5
    vecs = _mode_checks(c)
    for i, v in enumerate(vecs):
        _check("random mode %d sine of the A-angle to the reference vector" % i, ref.subspace_angle(c["P"].A, c["Phi"][:, i:i + 1], v), 1e-4)


def test_the_sign_rule(tp, orc):
    """the reference's line load on 16x2x8: the eigenvalue of largest magnitude is negative; the returned mu_1 is the largest
    POSITIVE one and no negative Ritz vector is among BucklingVectors()"""
    c = _mcase(tp, orc, "sign")
    mu_all, out = c["mu_all"], c["out"]
    print("sign: most negative %.6e, largest positive %.6e, next positive %.6e" % (mu_all[0], mu_all[-1], mu_all[-2]))
    assert -mu_all[0] > mu_all[-1] > 0
    assert out["mu"][0] > 0 and min(out["ritz"]) < 0
    vecs = _mode_checks(c)
    assert len(vecs) == 1
    v = vecs[0]
    _check("sign mode 0 sine of the A-angle to the reference vector", ref.subspace_angle(c["P"].A, c["Phi"][:, :1], v), 1e-4)
    Av, Bv = c["P"].apply_ld(v)
    assert float(v.astype(LD) @ Bv) > 0, "the returned vector is a mode of the reversed load"


def test_buckling_modes_refuses_to_return_wrong_values(tp, orc):
    c = _mcase(tp, orc, "random")
    le = c["le"]
    with pytest.raises(tp.TopOptError) as ei:
        le.BucklingModes(c["nev"], c["xd"], ref.EMAX, ref.PENAL, U=c["Ud"], tol=1e-14, max_iter=1)
    print(ei.value)
    assert "residuals" in str(ei.value) and "Ritz values" in str(ei.value)
    with pytest.raises(ValueError):
        le.BucklingModes(9, c["xd"], ref.EMAX, ref.PENAL)
    with pytest.raises(ValueError):
        le.BucklingModes(2, c["xd"], ref.EMAX, ref.PENAL, guard=7)
    # the reversed state: every eigenvalue changes its sign, and a column in tension has its two eigenvalues of largest
    # magnitude on the negative side; a block of two without guard vectors ends there: fewer than nev positive Ritz values at
    # the end is an error, not a value
    with pytest.raises(tp.TopOptError) as ei:
        le.BucklingModes(c["nev"], c["xd"], ref.EMAX, ref.PENAL, U=-c["Ud"], guard=0, tol=1e-8, max_iter=8)
    print(ei.value)
    assert "positive Ritz values" in str(ei.value)
    le._buck = None
    c["out"] = le.BucklingModes(c["nev"], c["xd"], ref.EMAX, ref.PENAL, U=c["Ud"], tol=1e-8)     # leave the cached object converged


# ---- 6
@pytest.mark.parametrize("name", ["column", "random"])
def test_buckling_sensitivity(tp, orc, name):
    """dJ/dx . W of the device, on the device's own state, against the restated one (1e-6), against the device's own central
    difference of J (bound 1e-5; step 1e-4: the truncation error of the central difference is of the order step^2 = 1e-8 of the
    derivative, and the noise of the state solves at rtol 1e-12 divided by the step stays two orders below the bound), and
    without the adjoint term (must be off by more than 100 x that bound)"""
    c = _mcase(tp, orc, name)
    le, P, nev, eps = c["le"], c["P"], c["nev"], 1e-4
    W = np.random.default_rng(31).uniform(-1.0, 1.0, c["x"].size)
    if name == "column":                                     # a direction with the section's symmetry keeps the pair double
        W = 0.5 * (W + W.reshape(c["ne"][2], c["ne"][1], c["ne"][0]).transpose(1, 0, 2).reshape(-1))

    def modes_of(xv, tol):
        xd = _dev(xv)
        le.SolveState(xd, ref.EMIN, ref.EMAX, ref.PENAL)
        return xd, le.BucklingModes(nev, xd, ref.EMAX, ref.PENAL, tol=tol)

    xd, o = modes_of(c["x"], 1e-9)
    _check("%s max|u device - u restated| / max|u|" % name, float(np.abs(le.U.cpu().numpy() - P.u).max() / np.abs(P.u).max()), 1e-8)
    out = c["grid"].elem_vec(3.0)                            # (overwritten by the first pass, added to by the others)
    J, its = le.BucklingSensitivity(out, xd, ref.EMIN, ref.EMAX, ref.PENAL, 8.0)
    assert its > 0 and le.adjoint_its == its and le.adjoint_rnorm <= 1e-11 * le.adjoint_bnorm
    an = float(out.cpu().numpy().astype(LD) @ W.astype(LD))
    full, stiff, explicit, state = P.dJ(c["mu"], c["Phi"][:, :nev], 8.0, parts=True)
    an_ref, no_adj = float(full @ W.astype(LD)), float((stiff + explicit) @ W.astype(LD))
    _check("%s |J / restated - 1|" % name, abs(J / float(P.J_of(c["mu"][:nev])) - 1), 1e-9)
    _check("%s |dJ/dx . W / restated - 1|" % name, abs(an / an_ref - 1), 1e-6)
    J2, its2 = le.BucklingSensitivity(c["grid"].elem_vec(), xd, ref.EMIN, ref.EMAX, ref.PENAL, 8.0)     # the adjoint state warm-starts
    assert its2 < its and J2 == J
    Jp = float(ref.Pencil.J_of(modes_of(c["x"] + eps * W, 1e-10)[1]["mu"]))
    Jm = float(ref.Pencil.J_of(modes_of(c["x"] - eps * W, 1e-10)[1]["mu"]))
    fd = (Jp - Jm) / (2 * eps)
    print("%s: J %.9e, dJ/dx . W = %.12e, restated %.12e, device central difference %.12e; without the adjoint term %.12e; "
          "adjoint solve %d iterations" % (name, J, an, an_ref, fd, no_adj, its))
    _check("%s |dJ/dx . W / device central difference - 1|" % name, abs(an / fd - 1), 1e-5)
    assert abs(no_adj / fd - 1) > 100 * 1e-5, "the comparison does not see the adjoint term"
    modes_of(c["x"], 1e-9)


# ---- 7
KW = dict(nxyz=(17, 5, 5), xc=(0.0, 4.0, 0.0, 1.0, 0.0, 1.0), nlvls=2, rmin=0.5, volfrac=0.5, load="axial")


def test_driver_off_is_the_parent_behaviour_bit_for_bit(tp):
    """buckling_limit=None: three iterations of a TopOpt built before any of the buckling machinery of this process's library was
    touched by IT and three of one whose solver object ran BucklingModes and BucklingSensitivity first -- the records are equal key
    for key, bit for bit, under the reference's load"""
    import torch
    kw = dict(nxyz=(17, 9, 9), nlvls=3, rmin=0.2, volfrac=0.3)
    a = tp.TopOpt(**kw)
    ha = [a.step() for _ in range(3)]
    xa = a.x.clone()
    assert a.physics._buck is None and a.physics._buck_adj is None and a.m == 1 and a._k_buck is None
    a.grid.close()
    b = tp.TopOpt(**kw)
    ph = b.physics                                           # the machinery, used beside the loop on a state of its own
    ph.AssembleStiffnessMatrix(b.xPrint, b.Emin, b.Emax, b.penal)
    U = b.grid.node_vec(3)
    rc = ph._solve(ph.AxialLoad(), U)[0]
    assert rc == 0
    ph.BucklingModes(2, b.xPrint, b.Emax, b.penal, U=U, tol=1e-4)
    ph.BucklingSensitivity(b.grid.elem_vec(), b.xPrint, b.Emin, b.Emax, b.penal)
    ph._buck = None
    assert not ph.U.any()
    hb = [b.step() for _ in range(3)]
    for ra, rb in zip(ha, hb):
        assert set(ra) == set(rb) and not any("buckling" in k for k in ra)
        for k in ra:
            if k != "time":
                assert ra[k] == rb[k], (k, ra[k], rb[k])
    assert torch.equal(xa, b.x)
    b.grid.close()


def test_driver_with_a_buckling_constraint(tp, orc):
    """three iterations of TopOpt(load="axial", buckling_limit=...) on 16x4x4 against the loop's pieces restated: in every iteration
    the record's mu, load factor and g against the restatement's pencil on the design the iteration saw (1e-8: the state solve runs
    at rtol 1e-10 here, the modes at the residual 1e-6, whose square is what an eigenvalue feels), and the row MMA saw against
    the restated gradient scaled by the limit and taken through the device's filter chain (1e-6)"""
    ne, h = (16, 4, 4), (0.25, 0.25, 0.25)
    so = tp.SolverOptions(nlvls=2, nu=ref.NU, rtol=1e-10, max_it=2000)
    plain = tp.TopOpt(solver=so, **KW)
    plain.physics.SolveState(plain.xPrint, plain.Emin, plain.Emax, plain.penal)
    mu0 = plain.physics.BucklingModes(2, plain.xPrint, plain.Emax, plain.penal)["mu"]
    plain.grid.close()
    limit = 1.2 / float(ref.Pencil.J_of(mu0))               # 1.2 x iteration 1's 1 / J of an unconstrained run
    opt = tp.TopOpt(buckling_limit=limit, solver=so, **KW)
    assert opt.m == 2 and opt._k_buck == 1 and len(opt.dgdx) == 2
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], ref.NU)).reshape(24, 24)
    N, F = ref.clamp_N(ne), ref.load_axial(ne)
    assert np.array_equal(opt.physics.N.cpu().numpy(), N) and float(np.abs(opt.physics.RHS.cpu().numpy() - F).max()) <= 1e-16
    hist = []
    for k in range(3):
        x_in, xt_in, xp_in = opt.x.clone(), opt.xTilde.clone(), opt.xPrint.cpu().numpy()
        r = opt.step()
        hist.append(r)
        print("itr %d: fx %.6e gx %+.5f gx_buckling %+.6f mu %s factor %.6e gap %.3f iters %d ksp_its_buckling %d"
              % (r["itr"], r["fx"], r["gx"], r["gx_buckling"], " ".join("%.6e" % v for v in r["buckling_mu"]), r["buckling_factor"],
                 r["buckling_gap"], r["buckling_iters"], r["ksp_its_buckling"]))
        for key in ("buckling_mu", "buckling_factor", "gx_buckling", "buckling_iters", "ksp_its_buckling", "buckling_gap"):
            assert key in r
        P = ref.Pencil(ne, h, xp_in, N, F, opt.Emin, opt.Emax, opt.penal, ref.NU, KE=KE)
        mu, Phi, _ = P.modes(2)
        J = float(P.J_of(mu))
        _check("itr %d max|mu / restated - 1|" % r["itr"], float(np.abs(np.array(r["buckling_mu"]) / mu - 1).max()), 1e-8)
        _check("itr %d |gx_buckling - (limit J - 1)|" % r["itr"], abs(r["gx_buckling"] - (limit * J - 1.0)), 1e-7)
        assert r["buckling_factor"] == pytest.approx(1.0 / r["buckling_mu"][0], rel=1e-15)
        raw = _dev(np.asarray(limit * P.dJ(mu, Phi, opt.buckling_P), dtype=np.float64))
        filtered, dummy = raw.clone(), opt.grid.elem_vec()
        opt.filt.Gradients(x_in, xt_in, dummy, [filtered])
        row = opt.dgdx[1]
        top = float(row.abs().max())
        _check("itr %d max|row MMA saw - filtered restated row| / max|row|" % r["itr"], float((row - filtered).abs().max()) / top, 1e-6)
        assert float((row - raw).abs().max()) / top > 1e-3, "the row bypassed the filter chain"
    assert abs(hist[0]["gx_buckling"] - 0.2) < 1e-6            # the limit is 1.2 x this design's 1 / J
    opt.grid.close()
