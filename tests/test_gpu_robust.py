"""Robust design on the device (tp_robust_project / tp_robust_chain, TopOpt(robust=...)).

The two kernels restate k_heaviside and k_heaviside_chain for several thresholds at once, so they are held to Filter.FilterProject
and Filter.Gradients bit for bit.  The driver is held to a loop written here from the classes that existed before (three
FilterProject calls, Gradients per row, Passive, MMA): both sides then run kernels that give the same bits, so the records and the
designs are equal bit for bit."""
import functools
import os

import numpy as np
import pytest

from tests.test_gpu_passive import KW, MESHES, PATTERNS, SHAPES, _bits, _labels, _payload

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
BETAS = (0.1, 4.0, 48.0)
THRESHOLDS = ((0.7, 0.5, 0.3), (0.5, 0.5, 0.5), (1.0, 0.5, 0.0))
ETAS = (0.7, 0.5, 0.3)
RKW = dict(KW, projectionFilter=True, beta=4.0, robust=ETAS)


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _salted(n, seed):
    """n values in [0, 1] with exact 0, 1, -0.0 and the thresholds among them, spread over the field (as many as fit)"""
    import torch
    a = np.random.default_rng(seed).uniform(0.0, 1.0, n)
    salts = [0.0, 1.0, -0.0, 0.7, 0.5, 0.3]
    for j, v in enumerate(salts[:n]):
        a[j * (n // len(salts)) if n >= len(salts) else j] = v
    if n > 64:
        a[-1], a[63], a[64] = 0.5, -0.0, 1.0     # the last element, and both sides of a wave's border
    return torch.from_numpy(a).cuda()


def _projection(flt0, xT, beta, eta):
    """Filter.FilterProject's xPhys at (beta, eta) from a sensitivity filter (type 0) whose x AND xTilde are the tensor xT itself:
    the filter step copies nothing, the projection kernel alone runs"""
    import torch
    out = torch.full_like(xT, float("nan"))
    flt0.FilterProject(xT, xT, out, True, beta, eta)
    return out


def _sum_bound(v):
    """|any float64 summation order - exact sum| <= (n - 1) eps sum|v_i| (Higham, Accuracy and Stability, 4.2, first order)"""
    v = np.asarray(v)
    return (v.size - 1) * EPS * float(np.abs(v.astype(np.longdouble)).sum())


# ---- 1, 2: the projection and its sums -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh", MESHES, ids=lambda m: "x".join(map(str, m)))
def test_projection_equals_filterproject_bit_for_bit(tp, mesh):
    """1, 2 and 3 fields at beta = 0.1, 4, 48 and three sets of thresholds: every out[k] has the bytes of FilterProject's xPhys at
    eta_k, with labels those of Passive.Impose(.., 0, 1) behind it; no NaN of the pre-filled outputs survives, xTilde keeps its
    bytes, equal thresholds give equal bytes; every returned sum lies within (n - 1) eps sum|v| of the 80-bit sum of the stored
    field, and the unreduced call returns None and stores the same bytes"""
    import torch
    n = mesh[0] * mesh[1] * mesh[2]
    grid = tp.Grid(mesh[0] + 1, mesh[1] + 1, mesh[2] + 1, 1.0)
    try:
        assert grid.n_own_elems == n
        flt0, rb = tp.Filter(grid, 0, 0.5), tp.Robust(grid)
        xT = _salted(n, n)
        keep = _bits(xT).clone()
        regions = [(pat, tp.Passive(grid, _labels(pat, n))) for pat in PATTERNS]
        worst = 0.0
        for beta in BETAS:
            want = {eta: _projection(flt0, xT, beta, eta) for eta in sorted({e for th in THRESHOLDS for e in th})}
            for pat, pr in [(None, None)] + regions:
                imposed = {eta: (pr.Impose([w.clone()], 0.0, 1.0)[0] if pr is not None else w) for eta, w in want.items()}
                # the 80-bit sum and the bound of each expected field, once: the stored fields must have these very bytes
                host = {eta: w.cpu().numpy() for eta, w in imposed.items()}
                exact = {eta: float(v.astype(np.longdouble).sum()) for eta, v in host.items()}
                bounds = {eta: _sum_bound(v) for eta, v in host.items()}
                for th in THRESHOLDS:
                    for nproj in (1, 2, 3):
                        what = "%s beta=%g eta=%r nproj=%d labels=%s" % ("x".join(map(str, mesh)), beta, th, nproj, pat)
                        outs = [_payload(n, k) for k in range(nproj)]
                        sums = rb.Project(xT, beta, th[:nproj], outs, passive=pr)
                        assert len(sums) == nproj
                        for k in range(nproj):
                            assert not bool(torch.isnan(outs[k]).any()), what + ": a NaN survived"
                            assert torch.equal(_bits(outs[k]), _bits(imposed[th[k]])), what + ": field %d" % k
                            off, bound = abs(sums[k] - exact[th[k]]), bounds[th[k]]
                            worst = max(worst, off / bound if bound else off)
                            assert off <= bound, what + ": sum %d off by %.3e (bound %.3e)" % (k, off, bound)
                        if th[0] == th[1] == th[2]:
                            assert all(torch.equal(_bits(outs[0]), _bits(o)) for o in outs[1:]), what
                        again = [_payload(n, k) for k in range(nproj)]
                        assert rb.Project(xT, beta, th[:nproj], again, passive=pr, sums=False) is None
                        assert all(torch.equal(_bits(a), _bits(o)) for a, o in zip(again, outs)), what + ": without sums"
                        assert torch.equal(_bits(xT), keep), what + ": xTilde was written"
        print("%s: largest |sum - 80-bit sum| / bound %.3e" % ("x".join(map(str, mesh)), worst))
        # all solid: the sum is the element count itself
        solid = tp.Passive(grid, np.full(n, 2, dtype=np.uint8))
        outs = [_payload(n, k) for k in range(3)]
        assert rb.Project(xT, 4.0, ETAS, outs, passive=solid) == [float(n)] * 3 and all(bool((o == 1.0).all()) for o in outs)
        void = tp.Passive(grid, np.full(n, 1, dtype=np.uint8))
        assert rb.Project(xT, 4.0, ETAS, outs, passive=void) == [0.0] * 3 and all(bool((_bits(o) == 0).all()) for o in outs)
    finally:
        grid.close()


def test_field_counts_outside_1_to_3_and_a_foreign_passive_handle_are_refused(tp):
    grid, other = tp.Grid(8, 6, 4, 1.0), tp.Grid(8, 6, 4, 1.0)
    try:
        rb, xT = tp.Robust(grid), grid.elem_vec(0.4)
        outs = [grid.elem_vec() for _ in range(4)]
        foreign = tp.Passive(other, _labels("random", other.n_own_elems))
        for call in (lambda: rb.Project(xT, 4.0, [], []), lambda: rb.Project(xT, 4.0, [0.7, 0.5, 0.3, 0.1], outs),
                     lambda: rb.Project(xT, 4.0, [0.7, 0.5], [outs[0], xT]), lambda: rb.Project(xT, 4.0, [0.7, 0.5], [outs[0], outs[0]]),
                     lambda: rb.Project(xT, 0.0, [0.5], outs[:1]), lambda: rb.Project(xT, 4.0, [1.5], outs[:1]),
                     lambda: rb.Project(xT, 4.0, ETAS, outs[:3], passive=foreign), lambda: rb.Chain(xT, 4.0, outs[:2], ETAS[:2], passive=foreign)):
            with pytest.raises(tp.TopOptError) as ei:
                call()
            assert ei.value.code == 1
        with pytest.raises(ValueError):
            rb.Project(xT, 4.0, ETAS, outs[:2])
    finally:
        grid.close()
        other.close()


# ---- 3: the ordering --------------------------------------------------------------------------------------------------------

def test_eroded_nominal_dilated_are_ordered_element_by_element(tp):
    """out_e <= out_n <= out_d with a slack of 8 eps on 1001 salted elements, beta from 0.1 to 48, at (0.7, 0.5, 0.3) and at the
    widest thresholds (1, 0.5, 0): what K(eroded) <= K(nominal) <= K(dilated), and with it the one solve per iteration, rests on"""
    grid = tp.Grid(8, 12, 14, 1.0)     # 7 x 11 x 13 elements
    try:
        rb, n = tp.Robust(grid), grid.n_own_elems
        xT = _salted(n, 5)
        worst = 0.0
        for beta in (0.1, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 48.0):
            for th in ((0.7, 0.5, 0.3), (1.0, 0.5, 0.0)):
                e, m, d = [grid.elem_vec() for _ in range(3)]
                rb.Project(xT, beta, th, [e, m, d], sums=False)
                worst = max(worst, float((e - m).max()), float((m - d).max()))
                assert bool((e <= m + 8 * EPS).all()) and bool((m <= d + 8 * EPS).all()), (beta, th)
        print("largest out_e - out_n or out_n - out_d: %.3e (slack %.3e)" % (worst, 8 * EPS))
    finally:
        grid.close()


# ---- 4: the chain rule ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ftype,mesh", [(1, (16, 8, 8)), (1, (7, 11, 13)), (2, (16, 8, 8))], ids=["density", "density-odd", "pde"])
def test_chain_then_transpose_equals_filter_gradients_bit_for_bit(tp, ftype, mesh):
    """Chain(rows, etas) followed by GradientsFromTilde(x, rows) against Filter.Gradients(.., True, beta, eta_r) row by row on a copy,
    1, 2, 5 and 8 rows with the thresholds mixed over the rows; with labels the passive entries are +0.0 by sign bit where the row
    held NaN or -0.0, and the active ones are those of the call without labels"""
    import torch
    n = mesh[0] * mesh[1] * mesh[2]
    grid = tp.Grid(mesh[0] + 1, mesh[1] + 1, mesh[2] + 1, 0.125)
    try:
        flt, rb = tp.Filter(grid, ftype, 0.2), tp.Robust(grid)
        x, xT = _salted(n, 11), _salted(n, 12)
        gen = torch.Generator(device="cuda").manual_seed(7)
        lab_h = _labels("random", n)
        pr, lab = tp.Passive(grid, lab_h), torch.from_numpy(lab_h).cuda()
        for beta in (BETAS if ftype == 1 else (4.0,)):
            for nrows in (1, 2, 5, 8):
                etas = [ETAS[(2 * r + nrows) % 3] for r in range(nrows)]
                assert nrows < 3 or len(set(etas)) == 3
                rows0 = [torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5 for _ in range(nrows)]
                what = "filter %d beta=%g nrows=%d" % (ftype, beta, nrows)
                # the chain alone, without and with labels
                plain = [r.clone() for r in rows0]
                rb.Chain(xT, beta, plain, etas)
                dirty = [r.clone() for r in rows0]
                for v, r in enumerate(dirty):
                    r[lab != 0] = _payload(n, v)[lab != 0]
                    r[::3] = torch.where(lab[::3] != 0, torch.full_like(r[::3], -0.0), r[::3])
                rb.Chain(xT, beta, dirty, etas, passive=pr)
                for r, p0 in zip(dirty, plain):
                    assert bool((_bits(r)[lab != 0] == 0).all()), what + ": a passive entry is not +0.0"
                    assert torch.equal(_bits(r)[lab == 0], _bits(p0)[lab == 0]), what + ": active entries with labels"
                # ... and through the filter's transpose
                flt.GradientsFromTilde(x, plain)
                for r0, got, eta in zip(rows0, plain, etas):
                    want = r0.clone()
                    flt.Gradients(x, xT, want, [], True, beta, eta)
                    assert torch.equal(_bits(got), _bits(want)), what + " eta=%g" % eta
        rows = [grid.elem_vec(1.0) for _ in range(9)]
        for call in (lambda: rb.Chain(xT, 4.0, [], []), lambda: rb.Chain(xT, 4.0, rows, [0.5] * 9),
                     lambda: rb.Chain(xT, 4.0, rows[:4], [0.7, 0.5, 0.3, 0.1])):
            with pytest.raises(tp.TopOptError) as ei:
                call()
            assert ei.value.code == 1
        assert all(bool((r == 1.0).all()) for r in rows)
    finally:
        grid.close()


# ---- 5: the driver ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case_labels():
    from topopt_in_petsc_amd.api import passive_labels
    lab = passive_labels(KW["nxyz"], KW["xc"], SHAPES)
    lab.setflags(write=False)
    return lab


def _independent_loop(tp, labels, nit, ftype, beta, etas, every=20):
    """the robust loop from LinearElasticity, Filter (three FilterProject calls, Gradients per row), Passive and MMA; Robust.Project
    gives the three sums alone, into fields nothing else reads"""
    import torch
    nx, ny, nz = KW["nxyz"]
    h, volfrac, Xmin, Xmax, movlim = 2.0 / (nx - 1), KW["volfrac"], 0.0, 1.0, 0.2
    g = tp.Grid(nx, ny, nz, (h, h, h))
    le = tp.LinearElasticity(g, tp.SolverOptions(nlvls=KW["nlvls"], nu=0.3))
    le.SetUpLoadAndBC()
    flt, rb = tp.Filter(g, ftype, KW["rmin"]), tp.Robust(g)
    n = g.n_own_elems
    pr, x0 = None, volfrac
    if labels is not None:
        pr = tp.Passive(g, np.array(labels))
        x0 = (volfrac * n - pr.n_solid) / pr.n_active
    x = g.elem_vec(x0)
    xT, xE, xN, xD = [g.elem_vec(volfrac) for _ in range(4)]
    spare = [g.elem_vec() for _ in range(3)]
    dfdx, dgdx = g.elem_vec(), g.elem_vec()
    if pr is not None:
        pr.Impose([x], Xmin, Xmax)
        xa, dfa, dga = pr.packed_vec(x0), pr.packed_vec(), pr.packed_vec()
    else:
        xa, dfa, dga = x, dfdx, dgdx
    xmin, xmax, xold = torch.zeros_like(xa), torch.zeros_like(xa), torch.full_like(xa, x0)
    mma = tp.MMA(g, xa, 1, n_global=pr.n_active if pr is not None else None)

    def filter_project():
        for field, eta in ((xE, etas[0]), (xN, etas[1]), (xD, etas[2])):
            flt.FilterProject(x, xT, field, True, beta, eta)
        if pr is not None:
            pr.Impose([xE, xN, xD], 0.0, 1.0)
        return rb.Project(xT, beta, etas, spare, passive=pr)

    S = filter_project()
    hist = []
    for itr in range(1, nit + 1):
        fx, _ = le.ComputeObjectiveConstraintsSensitivities(dfdx, dgdx, xE, 1.0e-9, 1.0, 3.0, volfrac)
        if itr == 1:
            fscale = 10.0 / fx
        if itr == 1 or itr % every == 0:
            vd = volfrac * S[2] / S[1]
        gx = S[2] / (n * vd) - 1.0
        dgdx.fill_(1.0 / (n * vd))
        dfdx.mul_(fscale)
        if pr is not None:
            pr.Zero([dfdx, dgdx])
        flt.Gradients(x, xT, dfdx, [], True, beta, etas[0])
        flt.Gradients(x, xT, dgdx, [], True, beta, etas[2])
        if pr is not None:
            pr.Gather([dfdx, dgdx], [dfa, dga])
        mma.SetOuterMovelimit(Xmin, Xmax, movlim, xa, xmin, xmax)
        mma.Update(xa, dfa, [gx], [dga], xmin, xmax)
        if pr is not None:
            pr.Scatter([xa], [x])
        ch = mma.DesignChange(xa, xold)
        if (ch < 0.01 or itr % 10 == 0) and beta < 48.0 and gx < 0.000001:
            beta = min(beta + 1 if beta < 7 else beta * 1.2, 48.0)
        S = filter_project()
        hist.append(dict(fx=fx, gx=gx, ch=ch, lam=mma.state()[0], vd=vd))
    out = dict(hist=hist, x=x.clone(), xPhys=xN.clone(), xErode=xE.clone(), xDilate=xD.clone())
    g.close()
    return out


@pytest.mark.parametrize("passive", [False, True], ids=["all-active", "passive"])
@pytest.mark.parametrize("ftype", [1, 2])
def test_driver_equals_an_independent_loop_bit_for_bit(tp, ftype, passive):
    """three design iterations at beta = 4, thresholds (0.7, 0.5, 0.3), density and PDE filter, with and without passive regions: x,
    xPhys, xErode, xDilate, fx, gx, ch and MMA's lam equal those of the loop above bit for bit"""
    import torch
    labels = _case_labels() if passive else None
    t = tp.TopOpt(passive=SHAPES if passive else None, filter=ftype, **RKW)
    lams = []
    for _ in range(3):
        t.step()
        lams.append(t.mma.state()[0])
    want = _independent_loop(tp, labels, 3, ftype, 4.0, ETAS)
    for r, lam, w in zip(t.history, lams, want["hist"]):
        print("filter %d passive %d itr %d: fx %r / %r, gx %r / %r, ch %r / %r, lam %r / %r, V_d* %r / %r, vol_real %r"
              % (ftype, passive, r["itr"], r["fx"], w["fx"], r["gx"], w["gx"], r["ch"], w["ch"], lam, w["lam"], r["vol_dilated_target"],
                 w["vd"], r["vol_real"]))
    for r, lam, w in zip(t.history, lams, want["hist"]):
        assert (r["fx"], r["gx"], r["ch"], lam, r["vol_dilated_target"]) == (w["fx"], w["gx"], w["ch"], w["lam"], w["vd"])
    for name in ("x", "xPhys", "xErode", "xDilate"):
        assert torch.equal(_bits(getattr(t, name)), _bits(want[name])), name
    assert float((t.xDilate - t.xErode).min()) >= -8 * EPS and float((t.xDilate - t.xErode).max()) > 0.01
    # where V_d* has just been set the dilated constraint IS the nominal design's volume constraint, S_n / (n volfrac) - 1
    r0 = t.history[0]
    assert r0["vol_dilated_target"] == pytest.approx(KW["volfrac"] * r0["vol_real"][2] / r0["vol_real"][1], rel=1e-15)
    assert r0["gx"] == pytest.approx(r0["vol_real"][1] / KW["volfrac"] - 1.0, abs=1e-14)
    if passive:
        lab = torch.from_numpy(np.array(labels)).cuda()
        for f in (t.xErode, t.xPhys, t.xDilate):
            assert bool((f[lab == 2] == 1.0).all()) and bool((f[lab == 1] == 0.0).all())
    t.grid.close()


def test_without_robust_the_driver_makes_no_robust_call(tp, monkeypatch):
    """robust=None: no projector, no field, and neither library call is made during construction and a step"""
    from topopt_in_petsc_amd import api

    def never(*a, **kw):
        raise AssertionError("a robust call without robust")
    monkeypatch.setattr(api.Robust, "Project", never)
    monkeypatch.setattr(api.Robust, "Chain", never)
    t = tp.TopOpt(projectionFilter=True, beta=4.0, eta=0.5, **KW)
    rec = t.step()
    assert t.projector is None and not hasattr(t, "xErode") and "vol_real" not in rec and "f_real" not in rec
    t.grid.close()


# ---- 6: thresholds that all but coincide ------------------------------------------------------------------------------------

def test_nearly_equal_thresholds_follow_the_plain_projected_run(tp):
    """robust = (0.5 + 1e-12, 0.5, 0.5 - 1e-12) against TopOpt(projectionFilter=True, eta=0.5), three iterations at beta = 4, within
    what the restart test of tests/test_mma.py demands: fx rel 1e-9, x 1e-9, ch rel 1e-7.

    The three designs then differ by about beta 1e-12 = 4e-12 per element, and V_d* = volfrac (1 + O(1e-11)); the volume constraint
    is the plain run's divided by volfrac (g = S_d / (n V_d*) - 1 against S_n / n - volfrac), which rescales MMA's multiplier and
    leaves the minimiser of its subproblem where it is.  Measured: fx off by 2.0e-11 .. 2.9e-10 (relative), ch by 4.0e-11 ..
    7.2e-11, x by 1.9e-11 at most: the tolerances hold as they stand."""
    d = 1e-12
    a = tp.TopOpt(projectionFilter=True, beta=4.0, eta=0.5, **KW)
    b = tp.TopOpt(**dict(RKW, robust=(0.5 + d, 0.5, 0.5 - d)))
    for _ in range(3):
        ra, rb = a.step(), b.step()
        print("itr %d: fx %.15e / %.15e (rel %.3e), ch %.15e / %.15e (rel %.3e), gx %.6e / %.6e, max |x - x| %.3e"
              % (ra["itr"], ra["fx"], rb["fx"], abs(rb["fx"] / ra["fx"] - 1), ra["ch"], rb["ch"], abs(rb["ch"] / ra["ch"] - 1), ra["gx"],
                 rb["gx"], float((a.x - b.x).abs().max())))
    for ra, rb in zip(a.history, b.history):
        assert rb["fx"] == pytest.approx(ra["fx"], rel=1e-9)
        assert rb["ch"] == pytest.approx(ra["ch"], rel=1e-7, abs=1e-12)
    assert float((a.x - b.x).abs().max()) < 1e-9
    a.grid.close()
    b.grid.close()


# ---- 7: the report ----------------------------------------------------------------------------------------------------------

def test_report_orders_the_realisations_and_leaves_the_eroded_solve_alone(tp):
    """robust_report = 1: f_e >= f_n >= f_d and vol_e <= vol_n <= vol_d in every record; the eroded solve's CG iteration counts, and
    fx, are those of the same run with robust_report = 0, so its warm start is undisturbed"""
    quiet, loud = tp.TopOpt(**RKW), tp.TopOpt(robust_report=1, **RKW)
    for _ in range(3):
        q, r = quiet.step(), loud.step()
        print("itr %d: f_real %r, vol_real %r, CG iterations %d (without report %d)" % (r["itr"], r["f_real"], r["vol_real"], r["ksp_its"], q["ksp_its"]))
        assert "f_real" not in q
        fe, fn, fd = r["f_real"]
        ve, vn, vd = r["vol_real"]
        assert fe == r["fx"] and fe >= fn >= fd > 0.0 and ve <= vn <= vd
        assert r["ksp_its"] == q["ksp_its"] and r["fx"] == q["fx"] and r["ch"] == q["ch"]
    every_other = tp.TopOpt(robust_report=2, **RKW)
    assert ["f_real" in every_other.step() for _ in range(2)] == [False, True]
    for t in (quiet, loud, every_other):
        t.grid.close()


# ---- 8: the gradients -------------------------------------------------------------------------------------------------------

ELEMS = (13 + 16 * (3 + 8 * 0), 13 + 16 * (4 + 8 * 1), 14 + 16 * (3 + 8 * 2))


def _rows_and_differences(tp, kw, elems, s=1e-3):
    """-> (t, [(dfdx_e, central difference of the compliance of the design the objective sees)], volume row, x0): the rows are those
    MMA receives in the first iteration (the objective's over its scale), the state solved to rtol 1e-12"""
    t = tp.TopOpt(solver=tp.SolverOptions(nlvls=KW["nlvls"], rtol=1e-12), **kw)
    seen, update = [], t.mma.Update

    def spy(x, dfdx, gx, dgdx, xmin, xmax):
        seen.append((dfdx.clone(), dgdx[0].clone()))
        return update(x, dfdx, gx, dgdx, xmin, xmax)
    t.mma.Update = spy
    x0 = t.x.clone()
    t.step()
    dfdx, row = (seen[0][0] / t.fscale).cpu().numpy(), seen[0][1].cpu().numpy()
    pairs = []
    for e in elems:
        f = []
        for sign in (1.0, -1.0):
            t.x.copy_(x0)
            t.x[e] += sign * s
            t._filter_project()
            design = t.xErode if t.robust is not None else t.xPrint
            f.append(t.physics.ComputeObjectiveConstraints(design, t.Emin, t.Emax, t.penal, t.volfrac)[0])
        pairs.append((float(dfdx[e]), (f[0] - f[1]) / (2 * s)))
    return t, pairs, row, x0


def test_gradients_against_central_differences(tp):
    """The volume row against the central difference (step s = 1e-3) of S_d(x) / (n V_d*) on three elements, and the objective's row
    against that of the eroded design's compliance.

    Volume row, bound: the difference quotient of a smooth function is off by at most s^2 / 6 max|d^3 S_d / dx_e^3| and by the
    rounding of its two values over 2 s.  d^3 S_d / dx_e^3 = sum_i H'''(xTilde_i) w_ie^3 with w_ie = d xTilde_i / d x_e in [0, 1], so
    it is at most max|H'''| sum_i w_ie; |H'''| <= 2 beta^3 / den (|tanh'''| <= 2), and with the density filter sum_i w_ie =
    sum_i H_ie / Hs_i <= Hs_e / min Hs <= max Hs / min Hs.  A sum of n values is off by at most (n - 1) eps S_d.  Together
      (s^2 / 6 * 2 beta^3 / den * max Hs / min Hs + 2 (n - 1) eps S_d / (2 s)) / (n V_d*),
    2.4e-8 here, about 1e-5 of an entry (2.3e-3).  Measured: 2.9e-10 at most.

    Objective's row: the allowed |difference - dfdx| is measured in this test through TopOpt(robust=None, projectionFilter=True,
    eta=0.7), whose xPhys is the eroded design, on the same elements -- times 4 for the different design point (the plain run
    starts at x = volfrac as well, so the point is in fact the same and the factor is slack).  Measured: 3.0e-7 in both runs
    (5e-7 of dfdx), ratio 1.0."""
    import math
    s = 1e-3
    t, pairs, row, x0 = _rows_and_differences(tp, RKW, ELEMS, s)
    n, vd, beta, eta_d = 16 * 8 * 8, t.history[0]["vol_dilated_target"], 4.0, ETAS[2]
    Hs = t.filt.Hs()
    den = math.tanh(beta * eta_d) + math.tanh(beta * (1.0 - eta_d))
    S_d = t.history[0]["vol_real"][2] * n
    bound = (s * s / 6.0 * 2.0 * beta ** 3 / den * float(Hs.max() / Hs.min()) + 2.0 * (n - 1) * EPS * S_d / (2.0 * s)) / (n * vd)
    worst_v = 0.0
    for e in ELEMS:
        S = []
        for sign in (1.0, -1.0):
            t.x.copy_(x0)
            t.x[e] += sign * s
            t._filter_project()
            S.append(t._S[2])
        fd = (S[0] - S[1]) / (2 * s) / (n * vd)
        worst_v = max(worst_v, abs(fd - row[e]))
        print("volume row, element %d: device %.12e, central difference %.12e, off by %.3e (bound %.3e)" % (e, row[e], fd, abs(fd - row[e]), bound))
        assert row[e] > 0.0 and abs(fd - row[e]) <= bound
    t.grid.close()
    plain, pairs0, _, _ = _rows_and_differences(tp, dict(KW, projectionFilter=True, beta=4.0, eta=ETAS[0]), ELEMS, s)
    plain.grid.close()
    for name, pp in (("robust", pairs), ("plain eta=0.7", pairs0)):
        for e, (an, fd) in zip(ELEMS, pp):
            print("objective row (%s), element %d: dfdx %.12e, central difference %.12e, off by %.3e" % (name, e, an, fd, abs(fd - an)))
    e_robust, e_plain = max(abs(fd - an) for an, fd in pairs), max(abs(fd - an) for an, fd in pairs0)
    print("objective row: robust %.3e, plain at eta = 0.7 %.3e (allowed %.3e); volume row: largest %.3e (bound %.3e)"
          % (e_robust, e_plain, 4 * e_plain, worst_v, bound))
    assert all(an < 0.0 for an, _ in pairs) and e_robust <= 4 * e_plain


# ---- 9: restart -------------------------------------------------------------------------------------------------------------

def test_restart_files_carry_the_dilated_target(tp, tmp_path):
    """robust_volume_every = 2: V_d* is set in iterations 1, 2 and 4.  Stop after iteration 3, restart from the files, run 4 and 5: what
    tests/test_mma.py's restart test demands; iteration 3's V_d* (set in 2) comes back from the third number of the _itr_f0 file,
    digit for digit.  A run without `robust` writes the two numbers in the reference's format, nothing else"""
    kw = dict(RKW, robust_volume_every=2)
    ref = tp.TopOpt(**kw)
    ref.run(max_itr=5)
    assert [r["vol_dilated_target"] != p["vol_dilated_target"] for p, r in zip(ref.history, ref.history[1:])] == [True, False, True, False]
    wd = str(tmp_path / "robust")
    a = tp.TopOpt(workdir=wd, **kw)
    a.run(max_itr=3)
    words = open(os.path.join(wd, "Restart00_itr_f0.dat")).read().split()
    assert len(words) == 3 and int(words[0]) == 3 and float(words[2]) == a.vd_target == ref.history[2]["vol_dilated_target"]
    b = tp.TopOpt(restartFileVec=os.path.join(wd, "Restart00.dat"), restartFileItr=os.path.join(wd, "Restart00_itr_f0.dat"),
                  restartFileVecSol=os.path.join(wd, "RestartSol00.dat"), **kw)
    assert b.itr == 3 and b.fscale == pytest.approx(a.fscale, rel=1e-6) and b.vd_target == a.vd_target
    b.fscale = a.fscale        # the "%e" companion keeps 7 digits; compare the loop itself
    b.run(max_itr=5)
    for r0, r1 in zip(ref.history[3:], b.history):
        print("itr %d: fx %r, restarted %r; ch %r, restarted %r; V_d* %r, restarted %r"
              % (r0["itr"], r0["fx"], r1["fx"], r0["ch"], r1["ch"], r0["vol_dilated_target"], r1["vol_dilated_target"]))
        assert r0["itr"] == r1["itr"]
        assert r1["fx"] == pytest.approx(r0["fx"], rel=1e-9)
        assert r1["vol_dilated_target"] == pytest.approx(r0["vol_dilated_target"], rel=1e-9)
    # xold is not part of the restart set: the first ch is against the start value
    assert b.history[1]["ch"] == pytest.approx(ref.history[4]["ch"], rel=1e-7, abs=1e-12)
    assert float((b.x - ref.x).abs().max()) < 1e-9
    # without robust: "%d  %e\n", as mpiio.write_restart has always written it
    wd2 = str(tmp_path / "plain")
    c = tp.TopOpt(workdir=wd2, **KW)
    c.run(max_itr=1)
    assert open(os.path.join(wd2, "Restart00_itr_f0.dat"), "rb").read() == ("%d  %e\n" % (1, c.fscale)).encode()
    for t in (ref, a, b, c):
        t.grid.close()
