"""Lowest eigenfrequencies: the mass operator, the mass half of the eigenvalue sensitivity, the two block-vector passes, the
subspace iteration and the driver's frequency constraint against the numpy / scipy restatement tests/eigen_ref.py.

Bounds.  Kernels (mass_apply, mass_sensitivity): the result lies within 16 x the distance of the float64 restatement from the
80-bit one, and at least 64 * 2^-53, relative to the result's maximum.  block_gram: 1e-13 relative, the bound tests/test_cpp_host.py
holds VecDot to (the vectors are positive, so sum |x y| is the dot product itself).  block_combine: 64 * 2^-53 * sum_j |Q_ji| |Y_j|
entry by entry.  Eigenvalues: theta_i >= lambda_i (1 - 1e-12) and theta_i / lambda_i - 1 <= max(1e-10, 16 x the distance of the
restatement's own subspace iteration from eigh); lambda_i here are eigh's values refined by an 80-bit Rayleigh quotient of eigh's
vectors (tests/eigen_ref.py: Pencil.refine), which carry the 80-bit rounding alone.  tests/test_eigen_abi.py holds every mesh and
design used here to the conditions these bounds rest on.  Every figure is printed with its bound before it is asserted."""
import numpy as np
import pytest

from tests import eigen_ref as ref

pytestmark = pytest.mark.gpu

LD = ref.LD
U53 = 2.0 ** -53
RHO0 = 2.5          # kernels: not 1, so that a dropped factor shows
WEIGHTS = [0.75, -0.5, 0.0]
NS = [1, 63, 64, 65, 1001, 262145]


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _check(label, got, bound):
    print("%-86s measured %.3e   bound %.1e" % (label, got, bound))
    assert got <= bound, (label, got, bound)


_CACHE = {}


def _kcase(tp, idx):
    """per kernel mesh, made once and left alone: grid, solver object with the cantilever's supports, design, fields, references"""
    if ("k", idx) in _CACHE:
        return _CACHE[("k", idx)]
    ne, h = ref.KERNEL_MESHES[idx]
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
    le.SetUpLoadAndBC()
    nnode = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
    rng = np.random.default_rng(900 + idx)
    V = [rng.uniform(-1.0, 1.0, 3 * nnode) for _ in range(3)]         # do NOT vanish on the supports
    x = ref.design_mixed(ne, 20 + idx)
    c = dict(grid=grid, le=le, ne=ne, h=h, dofs=ref.elem_dofs(*ne), nel=ne[0] * ne[1] * ne[2], nnode=nnode, N=le.N.cpu().numpy(),
             V=V, Vd=[_dev(v) for v in V], x=x, xd=_dev(x), tag="%dx%dx%d" % ne)
    assert (c["N"] == 0).any() and np.array_equal(c["N"], ref.cantilever_N(*ne))
    le.MassAssemble(c["xd"], RHO0, ref.X_LOW)
    _CACHE[("k", idx)] = c
    return c


# ---- 1
@pytest.mark.parametrize("idx", range(len(ref.KERNEL_MESHES)))
def test_mass_apply_against_the_restatement(tp, idx):
    import torch
    c = _kcase(tp, idx)
    g, le = c["grid"], c["le"]
    args = (c["x"], c["dofs"], c["nnode"], c["h"], RHO0, ref.X_LOW, c["N"])
    ys = []
    for l, (v, vd) in enumerate(zip(c["V"][:2], c["Vd"][:2])):
        yr, y64 = ref.mass_apply(*args, v, LD), ref.mass_apply(*args, v, np.float64)
        top = float(np.abs(yr).max())
        bound = max(16 * float(np.abs(y64 - yr).max()) / top, 64 * U53)
        y = g.node_vec(3)
        y.fill_(7.0)
        le.MassMult(vd, y)
        yh = y.cpu().numpy()
        _check("%s field %d max|B u - ref| / max|ref|" % (c["tag"], l), float(np.abs(yh - yr).max()) / top, bound)
        assert not yh[c["N"] == 0].any(), "B u is not zero on the clamped dofs: N is missing on the left"
        no_right = ref.mass_apply(*args[:-1], np.ones_like(c["N"]), v, LD) * c["N"]
        assert float(np.abs(no_right - yr).max()) > 1e-3 * top            # N missing on the right would show
        ys.append((yh, top, bound))
    (Bu, top_u, bu), (Bv, top_v, bv) = ys
    u, v = c["V"][0].astype(LD), c["V"][1].astype(LD)
    a, b = float(u @ Bv.astype(LD)), float(v @ Bu.astype(LD))
    scale = float(np.abs(u) @ np.abs(Bv).astype(LD))
    _check("%s |u^T (B v) - v^T (B u)| / sum |u| |B v|" % c["tag"], abs(a - b) / scale, max(bu, bv))
    # the same call with the mass of another density: rho0 scales, bit for bit a product by 2 (a power of two)
    le.MassAssemble(c["xd"], 2 * RHO0, ref.X_LOW)
    y2 = le.MassMult(c["Vd"][0])
    le.MassAssemble(c["xd"], RHO0, ref.X_LOW)
    assert torch.equal(y2, 2 * le.MassMult(c["Vd"][0]))


def test_mass_apply_repeats_bit_for_bit(tp):
    """two calls give the same bits (the ghost planes of y: tests/eigen_worker.py, one rank has none)"""
    import torch
    c = _kcase(tp, 3)
    y1, y2 = c["le"].MassMult(c["Vd"][0]), c["le"].MassMult(c["Vd"][0])
    assert torch.equal(y1, y2)


# ---- 2
@pytest.mark.parametrize("idx", range(len(ref.KERNEL_MESHES)))
def test_mass_sensitivity_against_the_restatement(tp, idx):
    c = _kcase(tp, idx)
    le, scale = c["le"], -2.0
    args = (c["x"], c["dofs"], c["h"], RHO0, ref.X_LOW, c["N"], c["V"], WEIGHTS, scale)
    tr, t64 = ref.mass_sens(*args, LD), ref.mass_sens(*args, np.float64)
    top = float(np.abs(tr).max())
    bound = max(16 * float(np.abs(t64 - tr).max()) / top, 64 * U53)
    pre = np.random.default_rng(idx).uniform(-1.0, 1.0, c["nel"]) * top
    d = _dev(pre)
    le.MassSensitivity(c["Vd"], WEIGHTS, c["xd"], scale, d)
    got = d.cpu().numpy()
    _check("%s max|out - (pre + term)| / max|term|" % c["tag"], float(np.abs(got - (pre.astype(LD) + tr)).max()) / top, bound)
    assert float(np.abs(got - tr).max()) / top > 0.1, "the kernel overwrote out instead of adding to it"
    no_N = ref.mass_sens(*args[:5], np.ones_like(c["N"]), *args[6:], LD)
    assert float(np.abs(no_N - tr).max()) > 1e-3 * top                     # a missing N would show
    # w = None: all weights 1
    t1 = ref.mass_sens(*args[:6], c["V"][:1], [1.0], 1.0, LD)
    d1 = c["grid"].elem_vec(0.0)
    le.MassSensitivity(c["Vd"][:1], None, c["xd"], 1.0, d1)
    _check("%s w=None max|out - term| / max|term|" % c["tag"], float(np.abs(d1.cpu().numpy() - t1).max() / np.abs(t1).max()), bound)


# ---- 3
@pytest.fixture(scope="module")
def blocks(tp):
    """eight positive vectors of the longest length, made once; shorter tests take prefixes"""
    rng = np.random.default_rng(77)
    host = [rng.uniform(0.25, 1.25, max(NS)) for _ in range(16)]
    grid = tp.Grid(5, 5, 5, 0.25)
    return dict(grid=grid, X=host[:8], Y=host[8:], Xd=[_dev(v) for v in host[:8]], Yd=[_dev(v) for v in host[8:]])


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("q", [1, 5, 8])
def test_block_gram(tp, blocks, q, n):
    g = blocks["grid"]
    X, Y = [v[:n] for v in blocks["Xd"][:q]], [v[:n] for v in blocks["Yd"][:q]]
    G = g.BlockGram(X, Y)
    Gr = np.array([[blocks["X"][i][:n].astype(LD) @ blocks["Y"][j][:n].astype(LD) for j in range(q)] for i in range(q)])
    _check("q %d n %d max|G / G_ref - 1|" % (q, n), float(np.abs(G / Gr - 1).max()), 1e-13)
    assert np.array_equal(G, g.BlockGram(X, Y)), "two calls give different bits"
    S = g.BlockGram(X, X)
    assert np.array_equal(S, S.T), "X^T X is not symmetric bit for bit"
    # one dot product at a time: the same numbers to the same bound
    import ctypes as C
    v = C.c_double()
    g.L.tp_vec_dot(g.handle, X[q - 1].data_ptr(), Y[0].data_ptr(), n, C.byref(v))
    _check("q %d n %d |G[q-1, 0] / tp_vec_dot - 1|" % (q, n), abs(G[q - 1, 0] / v.value - 1), 1e-13)


# ---- 4
@pytest.mark.parametrize("n", NS)
def test_block_combine(tp, blocks, n):
    import torch
    g, q = blocks["grid"], 5
    Q = np.random.default_rng(n).uniform(-1.0, 1.0, (q, q))
    Y = [v[:n] for v in blocks["Yd"][:q]]
    Z = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(q)]
    g.BlockCombine(Y, Q, Z)
    Yh = np.stack([blocks["Y"][j][:n] for j in range(q)], axis=1).astype(LD)
    Zr, mag = Yh @ Q.astype(LD), np.abs(Yh) @ np.abs(Q).astype(LD)
    err = max(float((np.abs(Z[i].cpu().numpy() - Zr[:, i]) / mag[:, i]).max()) for i in range(q))
    _check("q 5 n %d max_i |Z_i - sum_j Q_ji Y_j| / sum_j |Q_ji| |Y_j|" % n, err, 64 * U53)
    assert all(torch.equal(Y[j], blocks["Yd"][j][:n]) for j in range(q)), "an input was written to"
    lo = 1 if 1 < n < max(NS) else 0
    with pytest.raises(tp.TopOptError) as ei:              # Z_0 reaches into Y_1 (shifted by one entry where there is room)
        g.BlockCombine(Y, Q, [blocks["Yd"][1][lo:n + lo]] + Z[1:])
    assert ei.value.code == 1
    with pytest.raises(tp.TopOptError):
        g.BlockCombine(Y, Q, Y)


# ---- 5
def _ecase(tp, orc, name):
    """per eigen mesh, made once: device objects on an assembly of the design, the pencil of the restatement, its eigh (refined) and
    its own subspace iteration"""
    if ("e", name) in _CACHE:
        return _CACHE[("e", name)]
    c = dict(ref.EIGEN_CASES[name])
    ne, h, nev = c["ne"], c["h"], c["nev"]
    x = c["design"](ne, c["seed"])
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=c["nlvls"], nu=0.3))
    le.SetUpLoadAndBC()
    xd = _dev(x)
    le.AssembleStiffnessMatrix(xd, ref.EMIN, ref.EMAX, ref.PENAL)
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], 0.3)).reshape(24, 24)      # the oracle's, not the object's own
    P = ref.Pencil(ne, h, KE, x, ref.cantilever_N(*ne), ref.EMIN, ref.EMAX, ref.PENAL, ref.RHO0, ref.X_LOW)
    assert np.array_equal(le.N.cpu().numpy(), P.N)
    lam64, Phi = P.eigh(nev + 1)
    lam = P.refine(lam64, Phi)
    th_ref = P.subspace(nev, tol=1e-8)[0]
    own = float(np.abs(th_ref[:nev] / lam64[:nev] - 1).max())
    out = le.Eigenmodes(nev, xd, ref.RHO0, ref.X_LOW, tol=1e-8)
    c.update(grid=grid, le=le, x=x, xd=xd, P=P, lam=lam, lam64=lam64, Phi=Phi, own=own, out=out, tag=name)
    print("%s: eigh %s; 80-bit refinement moves them by %s; the restatement's own subspace iteration is %.3e from eigh"
          % (name, " ".join("%.9e" % v for v in lam64[:nev]), " ".join("%.2e" % float(v) for v in (lam / lam64 - 1)[:nev]), own))
    print("%s: device %s in %d iterations, %d solver iterations, residuals %s, gap %.3f"
          % (name, " ".join("%.9e" % v for v in out["lam"]), out["iters"], out["ksp_its"], " ".join("%.2e" % r for r in out["residuals"]), out["gap"]))
    _CACHE[("e", name)] = c
    return c


@pytest.mark.parametrize("name", ["box", "cube"])
def test_eigenmodes_against_dense_eigh(tp, orc, name):
    c = _ecase(tp, orc, name)
    nev, P, out = c["nev"], c["P"], c["out"]
    assert max(out["residuals"]) <= 1e-8 and len(out["lam"]) == nev
    rel = [float(LD(t) / l - 1) for t, l in zip(out["lam"], c["lam"][:nev])]
    bound = max(1e-10, 16 * c["own"])
    for i, r in enumerate(rel):
        print("%s mode %d: theta / lambda - 1 = %+.3e (upper bound: >= -1e-12; accuracy bound %.1e)" % (name, i, r, bound))
    assert all(r >= -1e-12 for r in rel), rel
    assert all(r <= bound for r in rel), rel
    true_gap = float(c["lam"][nev] / c["lam"][nev - 1] - 1)
    print("%s: gap %.6f, lambda_4 / lambda_3 - 1 = %.6f (the guard vector's Ritz value is an upper bound and not converged)" % (name, out["gap"], true_gap))
    assert true_gap - 1e-9 <= out["gap"] <= 1.1 * true_gap + 0.1
    vecs = [v.cpu().numpy() for v in c["le"].EigenVectors()]
    for i, v in enumerate(vecs):
        _check("%s mode %d sine of the B-angle to the reference eigenspace" % (name, i), ref.subspace_angle(P.B, c["Phi"][:, i:i + 1], v), 1e-4)
        assert not v[P.N == 0].any()
    Bv = [ref.mass_apply(c["x"], P.dofs, P.nnode, c["h"], ref.RHO0, ref.X_LOW, P.N, v, LD) for v in vecs]
    G = np.array([[float(vecs[i].astype(LD) @ Bv[j]) for j in range(nev)] for i in range(nev)])
    _check("%s max|Phi^T B Phi - I|" % name, float(np.abs(G - np.eye(nev)).max()), 1e-12)


def test_eigenmodes_through_a_double_eigenvalue(tp, orc):
    c = _ecase(tp, orc, "square")
    lam, out = c["lam"], c["out"]
    assert float(lam[1] / lam[0] - 1) < 1e-8
    J, Jr = sum(1.0 / LD(t) for t in out["lam"]), (1 / lam[:2]).sum()
    rel = float(J / Jr - 1)
    print("square: J = %.12e, reference %.12e, J / J_ref - 1 = %+.3e" % (float(J), float(Jr), rel))
    assert -max(1e-10, 16 * c["own"]) <= rel <= 1e-12        # theta >= lambda: J <= J_ref
    vecs = [v.cpu().numpy() for v in c["le"].EigenVectors()]
    for i, v in enumerate(vecs):                              # any basis of the plane
        _check("square vector %d sine of the B-angle to the double mode's plane" % i, ref.subspace_angle(c["P"].B, c["Phi"][:, :2], v), 1e-4)


def test_eigenmodes_refuses_to_return_unconverged_values(tp, orc):
    c = _ecase(tp, orc, "cube")
    with pytest.raises(tp.TopOptError) as ei:
        c["le"].Eigenmodes(c["nev"], c["xd"], ref.RHO0, ref.X_LOW, tol=1e-14, max_iter=1)
    print(ei.value)
    assert "residuals" in str(ei.value)
    with pytest.raises(ValueError):
        c["le"].Eigenmodes(7, c["xd"])
    c["le"].Eigenmodes(c["nev"], c["xd"], ref.RHO0, ref.X_LOW, tol=1e-8)     # leave the cached object converged


# ---- 6
@pytest.mark.parametrize("name", ["box", "square"])
def test_eigen_sensitivity(tp, orc, name):
    """dJ/dx . W of the device against the restated one (1e-6: the restatement's own distance from its central difference, which
    tests/test_eigen_abi.py prints, is far below), against the device's own central difference of J (step 1e-6, bound 1e-5), and
    without the mass term (must be off by more than 100 x that bound)"""
    c = _ecase(tp, orc, name)
    le, P, nev, eps = c["le"], c["P"], c["nev"], 1e-6
    W = np.random.default_rng(31).uniform(-1.0, 1.0, c["x"].size)
    if name == "square":                                     # a direction with the section's symmetry keeps the pair double
        W = 0.5 * (W + W.reshape(c["ne"][2], c["ne"][1], c["ne"][0]).transpose(1, 0, 2).reshape(-1))
    le.AssembleStiffnessMatrix(c["xd"], ref.EMIN, ref.EMAX, ref.PENAL)
    le.Eigenmodes(nev, c["xd"], ref.RHO0, ref.X_LOW, tol=1e-8)
    out = c["grid"].elem_vec(3.0)                            # (overwritten by the first pass, added to by the second)
    J = le.EigenSensitivity(out, c["xd"], ref.EMIN, ref.EMAX, ref.PENAL)
    an = float(out.cpu().numpy().astype(LD) @ W.astype(LD))
    an_ref = float(P.dJ(c["lam"], c["Phi"], nev) @ W.astype(LD))
    stiff = float(P.dJ(c["lam"], c["Phi"], nev, mass_term=False) @ W.astype(LD))
    _check("%s |dJ/dx . W / restated - 1|" % name, abs(an / an_ref - 1), 1e-6)

    def J_of(xv):
        xd = _dev(xv)
        le.AssembleStiffnessMatrix(xd, ref.EMIN, ref.EMAX, ref.PENAL)
        return sum(1.0 / LD(t) for t in le.Eigenmodes(nev, xd, ref.RHO0, ref.X_LOW, tol=1e-10, max_iter=60)["lam"])

    fd = float((J_of(c["x"] + eps * W) - J_of(c["x"] - eps * W)) / (2 * LD(eps)))
    print("%s: J %.9e, dJ/dx . W = %.12e, restated %.12e, device central difference %.12e; the stiffness term alone %.12e"
          % (name, J, an, an_ref, fd, stiff))
    _check("%s |dJ/dx . W / device central difference - 1|" % name, abs(an / fd - 1), 1e-5)
    assert abs(stiff / fd - 1) > 100 * 1e-5, "the comparison does not see the mass term"
    le.AssembleStiffnessMatrix(c["xd"], ref.EMIN, ref.EMAX, ref.PENAL)
    le.Eigenmodes(nev, c["xd"], ref.RHO0, ref.X_LOW, tol=1e-8)


# ---- 7
KW = dict(nxyz=(17, 9, 9), nlvls=3, rmin=0.2, volfrac=0.3)


def test_driver_off_is_the_parent_behaviour_bit_for_bit(tp):
    """frequency_limit=None: three iterations of a TopOpt built before any of the eigen machinery of this process's library was
    touched by IT and three of one built after another object ran Eigenmodes -- the records are equal key for key, bit for bit"""
    import torch
    a = tp.TopOpt(**KW)
    ha = [a.step() for _ in range(3)]
    xa = a.x.clone()
    assert a.physics._eig is None and a.m == 1
    a.grid.close()
    b = tp.TopOpt(**KW)
    b.physics.AssembleStiffnessMatrix(b.xPrint, b.Emin, b.Emax, b.penal)
    b.physics.Eigenmodes(2, b.xPrint)                       # the machinery, used beside the loop
    b.physics._eig = None
    hb = [b.step() for _ in range(3)]
    for ra, rb in zip(ha, hb):
        assert set(ra) == set(rb) and not any(k.startswith("eig") or k == "gx_frequency" for k in ra)
        for k in ra:
            if k != "time":
                assert ra[k] == rb[k], (k, ra[k], rb[k])
    assert torch.equal(xa, b.x)
    b.grid.close()


def test_driver_with_a_frequency_constraint(tp):
    plain = tp.TopOpt(**KW)
    plain.physics.AssembleStiffnessMatrix(plain.xPrint, plain.Emin, plain.Emax, plain.penal)
    lam0 = plain.physics.Eigenmodes(3, plain.xPrint)["lam"]
    plain.grid.close()
    limit = 1.2 * 3.0 / sum(1.0 / l for l in lam0)          # 1.2 x the harmonic mean of iteration 1 of an unconstrained run
    opt = tp.TopOpt(frequency_limit=limit, **KW)
    assert opt.m == 2 and opt._k_freq == 1 and len(opt.dgdx) == 2
    hist = []
    for k in range(6):
        hist.append(opt.step())
        if k == 0:
            row = opt.dgdx[1].clone()
            raw = opt.grid.elem_vec()
    for r in hist:
        print("itr %d: fx %.6e gx %+.5f gx_frequency %+.6f eig %s gap %.3f eig_iters %d ksp_its_eigen %d"
              % (r["itr"], r["fx"], r["gx"], r["gx_frequency"], " ".join("%.6e" % v for v in r["eig"]), r["eig_gap"], r["eig_iters"], r["ksp_its_eigen"]))
        for key in ("eig", "gx_frequency", "eig_iters", "ksp_its_eigen", "eig_gap"):
            assert key in r
        assert len(r["eig"]) == 3 and all(np.isfinite(v) and v > 0 for v in r["eig"])
    r1 = hist[0]
    assert r1["gx_frequency"] == pytest.approx(limit / 3 * sum(1.0 / v for v in r1["eig"]) - 1, abs=1e-14)
    assert abs(r1["gx_frequency"] - 0.2) < 1e-4             # the limit is 1.2 x this design's harmonic mean
    assert hist[2]["eig_iters"] < hist[0]["eig_iters"], "no warm start across design iterations"
    # the row went through the filter chain: the raw dJ/dx of the uniform start, scaled by limit / 3 and taken through
    # Filter.Gradients, is what MMA saw in iteration 1 -- and the raw row is not
    x1 = opt.grid.elem_vec(KW["volfrac"])
    opt.physics.AssembleStiffnessMatrix(x1, opt.Emin, opt.Emax, opt.penal)
    fresh = tp.LinearElasticity(opt.grid, tp.SolverOptions(nlvls=3, nu=0.3))
    fresh.SetUpLoadAndBC()
    fresh.AssembleStiffnessMatrix(x1, opt.Emin, opt.Emax, opt.penal)
    fresh.Eigenmodes(3, x1)
    fresh.EigenSensitivity(raw, x1, opt.Emin, opt.Emax, opt.penal)
    raw.mul_(limit / 3)
    filtered, dummy = raw.clone(), opt.grid.elem_vec()
    opt.filt.Gradients(x1, x1, dummy, [filtered])
    top = float(row.abs().max())
    _check("max|row MMA saw - filtered raw row| / max|row|", float((row - filtered).abs().max()) / top, 1e-6)
    assert float((row - raw).abs().max()) / top > 1e-3, "the row bypassed the filter chain"
    opt.grid.close()
