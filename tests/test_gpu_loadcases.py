"""Several load cases: the fused weighted response kernel (tp_elasticity_response) against the oracle and against numpy,
repeated solves on one assembly, the driver loop and its restart files.

Bounds of the kernel tests: 600 fused multiply-adds per element and case at 2^-53 each on O(1) data are about 7e-14; an order
of magnitude for cancellation and pow gives 1e-12.  Every figure is printed with its bound before it is asserted."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MESHES = [(16, 8, 8), (20, 12, 8)]      # 1024 elements; 1920: no multiple of the workgroup (256), not tile-aligned
WEIGHTS = [0.5, 0.0, 2.0, -1.0, 1.5, 0.25, 3.0, 1.0]
EMIN, EMAX, PENAL, VOLFRAC = 1e-9, 1.0, 3.0, 0.12
LX, LY, LZ = [0, 1, 1, 0, 0, 1, 1, 0], [0, 0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1, 1, 1]   # include/topopt_amd.h


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _elem_dofs(ex, ey, ez):
    """[nel, 24] global dofs of every element: node i + nx (j + ny k), element i + ex (j + ey k), corner order of the header"""
    nx, ny = ex + 1, ey + 1
    k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    cols = []
    for a in range(8):
        nd = (i + LX[a]) + nx * ((j + LY[a]) + ny * (k + LZ[a]))
        cols += [3 * nd, 3 * nd + 1, 3 * nd + 2]
    return np.stack(cols, axis=1)


_CACHE = {}


def _case(tp, orc, mesh):
    """per mesh, computed once and left alone: the solver object, densities, 8 random U and V, the oracle's per-case compliance
    and sensitivity, and numpy's v_e^T KE u_e per element (80-bit accumulation)"""
    if mesh in _CACHE:
        return _CACHE[mesh]
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    grid = tp.Grid(nx, ny, nz, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=3))
    le.SetUpLoadAndBC()
    xp = grid.synth_density()
    xo = xp.cpu().numpy().copy()                       # the oracle gets the device's densities: identical inputs
    assert np.abs(xo - orc.synth_density(ex, ey, ez, h)).max() < 1e-15
    rng = np.random.default_rng(100 + ex)
    n = 3 * nx * ny * nz
    U = [rng.uniform(-1.0, 1.0, n) for _ in range(8)]
    V = [rng.uniform(-1.0, 1.0, n) for _ in range(8)]
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    sens = [orc.compliance_sens(nx, ny, nz, KE, u, xo, EMIN, EMAX, PENAL, VOLFRAC) for u in U]
    dofs = _elem_dofs(ex, ey, ez)
    ke = le.KE.reshape(24, 24).astype(np.longdouble)
    vKu = [np.einsum("er,rc,ec->e", v[dofs].astype(np.longdouble), ke, u[dofs].astype(np.longdouble)) for u, v in zip(U, V)]
    c = dict(grid=grid, le=le, xp=xp, xo=xo, U=U, V=V, Ud=[_dev(u) for u in U], Vd=[_dev(v) for v in V], sens=sens, vKu=vKu,
             nel=ex * ey * ez)
    _CACHE[mesh] = c
    return c


def _check(label, got, want, bound):
    print("%-58s measured %.3e   bound %.1e" % (label, got, bound))
    assert got <= bound, (label, got, want, bound)


def _compare(c, ncase, fx, gx, fc, dfdx, dgdx, f_o, gx_o, df_o, tag):
    w = WEIGHTS[:ncase]
    fx_o = float(sum(wl * fl for wl, fl in zip(w, f_o)))
    _check("%s |fx/fx_o - 1|" % tag, abs(fx / fx_o - 1), fx_o, 1e-12)
    for l in range(ncase):
        _check("%s |f_case[%d]/f_o - 1|" % (tag, l), abs(fc[l] / float(f_o[l]) - 1), f_o[l], 1e-12)
    _check("%s max|dfdx - dfdx_o| / max|dfdx_o|" % tag, float(np.abs(dfdx - df_o).max() / np.abs(df_o).max()), 0, 1e-12)
    _check("%s |gx - gx_o|" % tag, abs(gx - gx_o), gx_o, 1e-13)
    assert np.array_equal(dgdx, np.full(c["nel"], 1.0 / c["nel"]))


@pytest.mark.parametrize("ncase", [1, 3, 8])
@pytest.mark.parametrize("mesh", MESHES)
def test_response_kernel_against_the_oracle(tp, orc, mesh, ncase):
    """compliance of ncase random states, weights with a zero and a negative one: one call against the oracle's
    compliance_sens per case combined in numpy"""
    c = _case(tp, orc, mesh)
    w = WEIGHTS[:ncase]
    df, dg = c["grid"].elem_vec(), c["grid"].elem_vec()
    fx, gx, fc = c["le"].Response(c["Ud"][:ncase], None, w, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, df, dg)
    f_o = [c["sens"][l][0] for l in range(ncase)]
    df_o = sum(wl * c["sens"][l][2] for l, wl in enumerate(w))
    _compare(c, ncase, fx, gx, fc, df.cpu().numpy(), dg.cpu().numpy(), f_o, c["sens"][0][1], df_o, "%dx%dx%d L=%d" % (mesh + (ncase,)))


@pytest.mark.parametrize("ncase", [1, 3, 8])
@pytest.mark.parametrize("mesh", MESHES)
def test_bilinear_form_against_numpy(tp, orc, mesh, ncase):
    """V_l != U_l: sum_e E_e v_e^T KE u_e from le.KE with the header's node numbering (numpy, 80-bit); one case of three keeps
    V_l = U_l (entry None) beside the distinct ones; V = U given explicitly is V = NULL bit for bit"""
    c = _case(tp, orc, mesh)
    le, xo, w = c["le"], c["xo"], WEIGHTS[:ncase]
    E = EMIN + xo.astype(np.longdouble) ** 3 * (EMAX - EMIN)
    coef = -PENAL * xo.astype(np.longdouble) ** 2 * (EMAX - EMIN)
    sym = 1 if ncase >= 3 else None                      # this case: V_l = U_l through a None entry
    Vd = [None if l == sym else c["Vd"][l] for l in range(ncase)]
    vKu = [c["vKu"][l] for l in range(ncase)]
    if sym is not None:                                  # its u_e^T KE u_e, in 80 bits like the others
        ue = c["U"][sym][_elem_dofs(*mesh)].astype(np.longdouble)
        vKu[sym] = np.einsum("er,rc,ec->e", ue, le.KE.reshape(24, 24).astype(np.longdouble), ue)
    f_o = [float((E * v).sum()) for v in vKu]
    df_o = (coef * sum(wl * v for wl, v in zip(w, vKu))).astype(np.float64)
    df, dg = c["grid"].elem_vec(), c["grid"].elem_vec()
    fx, gx, fc = le.Response(c["Ud"][:ncase], Vd, w, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, df, dg)
    _compare(c, ncase, fx, gx, fc, df.cpu().numpy(), dg.cpu().numpy(), f_o, float(xo.mean() - VOLFRAC), df_o,
             "bilinear %dx%dx%d L=%d" % (mesh + (ncase,)))
    # V = U explicitly == V = NULL, bit for bit
    d0, d1 = c["grid"].elem_vec(), c["grid"].elem_vec()
    r0 = le.Response(c["Ud"][:ncase], None, w, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d0)
    r1 = le.Response(c["Ud"][:ncase], c["Ud"][:ncase], w, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d1)
    assert r0 == r1 and np.array_equal(d0.cpu().numpy(), d1.cpu().numpy())


@pytest.mark.parametrize("mesh", MESHES)
def test_one_case_equals_todays_call(tp, orc, mesh):
    """Response([U]) against Objective on the same state.  dfdx and gx are the same bits (same operations in the same order);
    fx is held to 1e-12: the fused kernel evaluates pow once per element and forms x^p as x^(p-1) x, one rounding away from
    k_objective's second pow.  And with one load case ComputeObjectiveConstraintsSensitivities still calls
    tp_elasticity_objective: bit-equal to an explicit Objective call on the state it leaves."""
    c = _case(tp, orc, mesh)
    le, g = c["le"], c["grid"]
    le.U.copy_(c["Ud"][0])
    d0, g0, d1, g1 = g.elem_vec(), g.elem_vec(), g.elem_vec(), g.elem_vec()
    fx0, gx0 = le.Objective(c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d0, g0)
    fx1, gx1, fc = le.Response([le.U], None, None, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d1, g1)
    print("fx bits equal: %s" % (fx0 == fx1))
    _check("one case |fx/fx_objective - 1|", abs(fx1 / fx0 - 1), fx0, 1e-12)
    assert fc == [fx1] and gx1 == gx0
    assert np.array_equal(d1.cpu().numpy(), d0.cpu().numpy()), "dfdx of one case differs from tp_elasticity_objective's"
    assert np.array_equal(g1.cpu().numpy(), g0.cpu().numpy())
    # the one-case path of the fused method
    le.U.zero_()
    assert le.ncases == 1
    d2, g2, d3, g3 = g.elem_vec(), g.elem_vec(), g.elem_vec(), g.elem_vec()
    fx2, gx2 = le.ComputeObjectiveConstraintsSensitivities(d2, g2, c["xp"], EMIN, EMAX, PENAL, VOLFRAC)
    fx3, gx3 = le.Objective(c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d3, g3)
    assert (fx2, gx2) == (fx3, gx3) and np.array_equal(d2.cpu().numpy(), d3.cpu().numpy())
    assert le.case_its == [le.last_its] and le.last_its > 0


@pytest.mark.parametrize("mesh", MESHES)
def test_no_host_synchronisation_without_sums(tp, orc, mesh):
    """fx, gx and f_case all NULL: one launch (two with the dgdx fill), no reduction launch; dfdx the same bits as with sums"""
    c = _case(tp, orc, mesh)
    le, g, w = c["le"], c["grid"], WEIGHTS[:3]
    Vd = [c["Vd"][0], None, c["Vd"][2]]
    d0, d1, d2, dg = g.elem_vec(), g.elem_vec(), g.elem_vec(), g.elem_vec()
    le.pop_stats()
    assert le.Response(c["Ud"][:3], Vd, w, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d0, sums=False) == (None, None, None)
    assert le.pop_stats()[2] == 1
    le.Response(c["Ud"][:3], Vd, w, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d1, dg, sums=False)
    assert le.pop_stats()[2] == 2
    le.Response(c["Ud"][:3], Vd, w, c["xp"], EMIN, EMAX, PENAL, VOLFRAC, d2)
    byt, _, n = le.pop_stats()
    assert n == 2                                           # the kernel and ONE reduction of all four sums
    nodes = (mesh[0] + 1) * (mesh[1] + 1) * (mesh[2] + 1)
    assert byt == 24.0 * nodes * 5 + 16.0 * c["nel"]        # five distinct vectors: three U, two V
    assert np.array_equal(d0.cpu().numpy(), d2.cpu().numpy()) and np.array_equal(d1.cpu().numpy(), d2.cpu().numpy())
    assert np.array_equal(dg.cpu().numpy(), np.full(c["nel"], 1.0 / c["nel"]))


def test_argument_checks_with_a_real_handle(tp, orc):
    c = _case(tp, orc, MESHES[0])
    le = c["le"]
    with pytest.raises(tp.api.TopOptError, match="TP_ERR_ARG"):
        le.Response([], None, None, c["xp"], EMIN, EMAX, PENAL, VOLFRAC)
    with pytest.raises(tp.api.TopOptError, match="TP_ERR_ARG"):
        le.Response([c["Ud"][0]] * 9, None, None, c["xp"], EMIN, EMAX, PENAL, VOLFRAC)
    with pytest.raises(tp.api.TopOptError, match="TP_ERR_ARG"):
        le.Response([c["Ud"][0], None], None, None, c["xp"], EMIN, EMAX, PENAL, VOLFRAC)
    g = tp.Grid(9, 5, 5, 0.25)
    le2 = tp.LinearElasticity(g, tp.SolverOptions(nlvls=2))
    for _ in range(7):
        le2.AddLoadCase(g.node_vec(3))
    assert le2.ncases == 8
    with pytest.raises(tp.api.TopOptError, match="TP_MAX_CASES"):
        le2.AddLoadCase(g.node_vec(3))
    g.close()


def _top_rhs(nx, ny, nz):
    R = np.zeros((nz, ny, nx, 3))
    R[nz - 1, :, nx - 1, 2] = 0.001
    R[nz - 1, 0, nx - 1, 2] = 0.0005
    R[nz - 1, ny - 1, nx - 1, 2] = 0.0005
    return R.reshape(-1)


def test_several_solves_on_one_assembly(tp, orc):
    """one assemble, then: case 0, case "top", case 0 again from a zeroed U.  The third solve repeats the first bit for bit
    (iteration count and residual history): nothing of a solve outlives it but the state; case "top" is the oracle's solve of
    its right-hand side at the bounds tests/test_gpu_configs.py uses for one case."""
    ex, ey, ez, nlv = 16, 8, 8, 3
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    grid = tp.Grid(nx, ny, nz, h)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=nlv, rtol=1e-8))
    le.SetUpLoadAndBC()
    top = le.SetUpLoadAndBC_Top()
    assert top == 1 and np.array_equal(le.LoadCaseRHS(1).cpu().numpy(), _top_rhs(nx, ny, nz))
    xp = grid.synth_density()
    le.AssembleStiffnessMatrix(xp, EMIN, EMAX, PENAL)
    its0 = le.KSPSolve(hist_cap=256)
    hist0, U0 = le.last_hist.copy(), le.U.clone()
    its1 = le.KSPSolve(hist_cap=256, case=1)
    hist1 = le.last_hist.copy()
    assert le.case_its == [its0, its1] and le.last_its == its1
    le.U.zero_()
    its2 = le.KSPSolve(hist_cap=256)
    assert its2 == its0 and np.array_equal(le.last_hist, hist0), (its0, its2)
    import torch
    assert torch.equal(le.U, U0)
    # case "top" against the oracle
    xo = orc.synth_density(ex, ey, ez, h)
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    N, R = orc.cantilever_bc(nx, ny, nz, h)
    mg = orc.MG(nx, ny, nz, 3, nlv)
    mg.assemble(KE, orc.simp(xo), N)
    U, its, hist = mg.solve(_top_rhs(nx, ny, nz) * N, rtol=1e-8)
    assert its1 == its and its > 3
    _check("case top: max|hist/hist_o - 1|", float(np.abs(hist1 / hist - 1).max()), 0, 1e-10)
    _check("case top: max|U - U_o| / max|U_o|", float(np.abs(le.LoadCaseU(1).cpu().numpy() - U).max() / np.abs(U).max()), 0, 1e-9)
    grid.close()


def test_driver_loop_with_two_load_cases_matches_the_oracle_loop(tp, orc):
    """main.cc's loop with the weighted objective f = f_0 + 0.5 f_top against the same loop driven by the oracle: two solves (each
    warm-started from its own state) and a weighted sum per iteration; bounds of tests/test_mma.py's one-case loop test"""
    ex, ey, ez, nlv = 32, 16, 16, 3
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    rmin = 2.56 * h
    kw = dict(nxyz=(nx, ny, nz), xc=(0, 2, 0, 1, 0, 1), nlvls=nlv, rmin=rmin)
    opt = tp.TopOpt(solver=tp.SolverOptions(nlvls=nlv, rtol=1e-8), loadcases=[("top", 0.5)], **kw)
    KE = orc.hex8_ke_box(h, h, h, 0.3)
    N, R = orc.cantilever_bc(nx, ny, nz, h)
    Rs, ws = [R, _top_rhs(nx, ny, nz)], [1.0, 0.5]
    flt = orc.Filter(nx, ny, nz, h, rmin)
    mg = orc.MG(nx, ny, nz, 3, nlv)
    n = ex * ey * ez
    x = np.full(n, 0.12)
    xt, xp = flt.project(1, x)
    mma = orc.MMA(x, 1)
    xold = x.copy()
    Us = [np.zeros(3 * nx * ny * nz) for _ in Rs]
    fscale = None
    for it in range(4):
        rec = opt.step()
        mg.assemble(KE, orc.simp(xp), N)
        its, fs, df = [], [], 0.0
        for l in range(2):
            Us[l], k, _ = mg.solve(Rs[l] * N, x0=Us[l], rtol=1e-8)
            f, gx, d, dg = orc.compliance_sens(nx, ny, nz, KE, Us[l], xp)
            its.append(k)
            fs.append(f)
            df = df + ws[l] * d
        fx = ws[0] * fs[0] + ws[1] * fs[1]
        if fscale is None:
            fscale = 10.0 / fx
        df = flt.gradient(1, x, xt, df * fscale)
        dg = flt.gradient(1, x, xt, dg)
        xmin, xmax = mma.SetOuterMovelimit(0.0, 1.0, 0.2, x)
        x = mma.Update(x, df, [gx], [dg], xmin, xmax)
        ch = mma.DesignChange(x, xold)
        xt, xp = flt.project(1, x)
        assert rec["ksp_its_case"] == its and rec["ksp_its"] == sum(its), (it, rec["ksp_its_case"], its)
        assert rec["fx"] == pytest.approx(fx, rel=1e-7)
        for l in range(2):
            assert rec["f_case"][l] == pytest.approx(fs[l], rel=1e-7)
        assert rec["gx"] == pytest.approx(gx, abs=1e-10)
        assert rec["ch"] == pytest.approx(ch, abs=1e-7)
        assert np.abs(opt.x.cpu().numpy() - x).max() <= 1e-6
    assert opt.fscale == pytest.approx(fscale, rel=1e-7)     # fscale = 10 / (weighted total)
    opt.grid.close()
    # loadcases=None: the record of a TopOpt built without the keyword, number for number
    a = tp.TopOpt(solver=tp.SolverOptions(nlvls=nlv, rtol=1e-8), **kw)
    b = tp.TopOpt(solver=tp.SolverOptions(nlvls=nlv, rtol=1e-8), loadcases=None, **kw)
    for _ in range(2):
        ra, rb = a.step(), b.step()
        assert sorted(ra) == sorted(rb) and "f_case" not in ra
        assert {k: v for k, v in ra.items() if k != "time"} == {k: v for k, v in rb.items() if k != "time"}
    a.grid.close()
    b.grid.close()


def test_restart_with_two_load_cases(tp, tmp_path):
    """4 iterations with a workdir, restart, run to 6: fx of iterations 5-6 is the uninterrupted run's to rel 1e-9 and the
    per-case iteration counts are equal (every case resumes from its own state in RestartSol0x.dat); a file with one state
    leaves the second case at zero; with one case the file is today's, byte for byte"""
    from topopt_in_petsc_amd.driver import TopOpt
    from topopt_in_petsc_amd.mpiio import read_petsc_vecs, write_petsc_vecs
    kw = dict(nxyz=(33, 17, 17), nlvls=3, rmin=0.1, volfrac=0.3)
    two = dict(loadcases=[("top", 0.5)], **kw)
    ref = TopOpt(**two)
    ref.run(max_itr=6)
    wd = str(tmp_path / "two")
    a = TopOpt(workdir=wd, output=False, **two)
    a.run(max_itr=4)
    sol = os.path.join(wd, "RestartSol00.dat")
    states = read_petsc_vecs(sol)
    assert len(states) == 2 and states[0].size == 3 * 33 * 17 * 17
    assert np.array_equal(states[0], a.physics.U.cpu().numpy()) and np.array_equal(states[1], a.physics.LoadCaseU(1).cpu().numpy())
    rs = dict(restartFileVec=os.path.join(wd, "Restart00.dat"), restartFileItr=os.path.join(wd, "Restart00_itr_f0.dat"))
    b = TopOpt(restartFileVecSol=sol, **rs, **two)
    assert b.itr == 4
    b.fscale = a.fscale        # the "%e" companion keeps 7 digits (TopOpt.cc:548); compare the loop itself
    b.run(max_itr=6)
    assert [r["itr"] for r in b.history] == [5, 6]
    for r0, r1 in zip(ref.history[4:], b.history):
        assert r1["fx"] == pytest.approx(r0["fx"], rel=1e-9)
        assert r1["ksp_its_case"] == r0["ksp_its_case"]
    # fewer states than cases: the others stay at zero
    one = os.path.join(wd, "one_state.dat")
    write_petsc_vecs(one, states[:1])
    c = TopOpt(restartFileVecSol=one, **rs, **two)
    assert np.array_equal(c.physics.U.cpu().numpy(), states[0]) and float(c.physics.LoadCaseU(1).abs().max()) == 0.0
    for t in (ref, a, b, c):
        t.grid.close()
    # one case: byte-identical files with and without the keyword
    w0, w1 = str(tmp_path / "k0"), str(tmp_path / "k1")
    p = TopOpt(workdir=w0, output=False, **kw)
    q = TopOpt(workdir=w1, output=False, loadcases=None, **kw)
    p.run(max_itr=2)
    q.run(max_itr=2)
    raw = open(os.path.join(w0, "RestartSol00.dat"), "rb").read()
    assert raw == open(os.path.join(w1, "RestartSol00.dat"), "rb").read()
    assert len(raw) == 8 + 8 * 3 * 33 * 17 * 17      # one Vec: header + the state, as before
    assert np.array_equal(read_petsc_vecs(os.path.join(w0, "RestartSol00.dat"))[0], p.physics.U.cpu().numpy())
    p.grid.close()
    q.grid.close()
