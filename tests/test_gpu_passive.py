"""Passive regions on the device (tp_passive, TopOpt(passive=...)).

The four kernels move data, so they are held to numpy / torch indexing byte for byte.  The driver is held to a loop written here
from the classes that existed before (LinearElasticity, Filter, MMA(n_global=...)) with torch indexing where the driver uses the new
kernels: both sides run the same kernels in the same order everywhere else, so the records and the designs are equal bit for bit."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# own-element counts 1, 63, 64, 65, 255, 256, 257, 1001, and 552 960: one more pass than grid_for's 2048 workgroups of 256 cover
MESHES = [(1, 1, 1), (63, 1, 1), (64, 1, 1), (13, 5, 1), (17, 15, 1), (16, 16, 1), (257, 1, 1), (7, 11, 13), (96, 80, 72)]
PATTERNS = ("all_active", "all_passive", "alternating", "first_passive", "last_passive", "one_active_in_the_last_wave", "random")
NVECS = (1, 2, 9, 12)
NAN_BITS = 0x7FF8000000000000
# the driver's case: 16 x 8 x 8 elements, 3 levels, the cantilever (load along the edge x = 2, z = 0), a solid box over the loaded
# edge and a void sphere in the middle
SHAPES = [("solid", "box", (1.75, 2.0, 0.0, 1.0, 0.0, 0.25)), ("void", "sphere", (1.0, 0.5, 0.5, 0.3))]
KW = dict(nxyz=(17, 9, 9), xc=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0), nlvls=3, rmin=0.2, volfrac=0.3)


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _labels(pattern, n):
    lab = np.zeros(n, dtype=np.uint8)
    if pattern == "all_passive":
        lab[:] = 1 + (np.arange(n) % 2)
    elif pattern == "alternating":
        lab[1::2] = 1 + (np.arange(n)[1::2] // 2) % 2
    elif pattern == "first_passive":
        lab[0] = 2
    elif pattern == "last_passive":
        lab[-1] = 1
    elif pattern == "one_active_in_the_last_wave":
        lab[:] = 1 + (np.arange(n) % 2)
        lab[(n - 1) // 64 * 64 + ((n - 1) % 64) // 2] = 0
    elif pattern == "random":
        lab[:] = np.random.default_rng(n).choice(3, size=n, p=[0.5, 0.2, 0.3])
    return lab


def _bits(t):
    import torch
    return t.view(torch.int64)


def _payload(n, v):
    """n NaNs, each with its own payload: whatever is not to be written must come back with these very bytes"""
    import torch
    return (torch.arange(n, dtype=torch.int64, device="cuda") + (NAN_BITS + 1 + (v << 32))).view(torch.float64)


def _random_bits(n, seed):
    """n doubles of arbitrary bytes (NaNs, infinities, denormals and both zeros among them)"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, device="cuda", generator=gen).view(torch.float64)


@pytest.mark.parametrize("mesh", MESHES, ids=lambda m: "x".join(map(str, m)))
def test_kernels_move_exactly_the_bytes_indexing_moves(tp, mesh):
    """impose, zero, gather and scatter with 1, 2, 9 and 12 vectors on every label pattern against torch indexing, byte for byte;
    entries that must not be written keep their NaN payloads; zero leaves +0.0 by sign bit"""
    import torch
    n = mesh[0] * mesh[1] * mesh[2]
    grid = tp.Grid(mesh[0] + 1, mesh[1] + 1, mesh[2] + 1, 1.0)
    try:
        assert grid.n_own_elems == n
        for pattern in PATTERNS:
            lab_h = _labels(pattern, n)
            pr = tp.Passive(grid, lab_h)
            lab = torch.from_numpy(lab_h).cuda()
            idx = torch.nonzero(lab == 0).flatten()
            na = idx.numel()
            assert pr.counts() == (na, int((lab == 1).sum()), int((lab == 2).sum())) and pr.n_active == na
            for nvec in NVECS:
                what = "%s %s nvec=%d" % ("x".join(map(str, mesh)), pattern, nvec)
                # gather
                full = [_random_bits(n, 100 * v + nvec) for v in range(nvec)]
                keep = [f.clone() for f in full]
                packed = [_payload(na, v) for v in range(nvec)]
                pr.Gather(full, packed)
                for v in range(nvec):
                    assert torch.equal(_bits(packed[v]), _bits(keep[v])[idx]), what + ": gather"
                    assert torch.equal(_bits(full[v]), _bits(keep[v])), what + ": gather wrote its source"
                # scatter: the inverse on the active entries, nothing on the passive ones
                target = [_payload(n, v) for v in range(nvec)]
                pr.Scatter(packed, target)
                for v in range(nvec):
                    want = _bits(_payload(n, v)).clone()
                    want[idx] = _bits(keep[v])[idx]
                    assert torch.equal(_bits(target[v]), want), what + ": scatter"
                # impose: the value of the label, active entries untouched
                target = [_payload(n, v) for v in range(nvec)]
                pr.Impose(target, -0.0, 0.75)
                for v in range(nvec):
                    want = _payload(n, v)
                    want[lab == 1], want[lab == 2] = -0.0, 0.75
                    assert torch.equal(_bits(target[v]), _bits(want)), what + ": impose"
                # zero: +0.0 whatever was there (NaN payloads, and -0.0 on every third entry)
                target = [_payload(n, v) for v in range(nvec)]
                for t in target:
                    t[::3] = -0.0
                before = [_bits(t).clone() for t in target]
                pr.Zero(target)
                for v in range(nvec):
                    want = before[v]
                    want[lab != 0] = 0          # all bits clear: +0.0
                    assert torch.equal(_bits(target[v]), want), what + ": zero"
            pr.close()
    finally:
        grid.close()


def test_vector_counts_outside_1_to_12_and_labels_above_2_are_refused(tp):
    grid = tp.Grid(8, 6, 4, 1.0)
    try:
        n = grid.n_own_elems
        pr = tp.Passive(grid, _labels("random", n))
        full, packed = [grid.elem_vec() for _ in range(13)], [pr.packed_vec() for _ in range(13)]
        for vecs, pk in (([], []), (full, packed)):
            for call in (lambda: pr.Impose(vecs, 0.0, 1.0), lambda: pr.Zero(vecs), lambda: pr.Gather(vecs, pk), lambda: pr.Scatter(pk, vecs)):
                with pytest.raises(tp.TopOptError) as ei:
                    call()
                assert ei.value.code == 1
        with pytest.raises(tp.TopOptError) as ei:
            pr.Gather([full[0], full[1]], [packed[0], full[0][:pr.n_active]])     # full[0] is packed[1]
        assert ei.value.code == 1
        bad = _labels("random", n)
        bad[n // 2] = 3
        with pytest.raises(tp.TopOptError) as ei:
            tp.Passive(grid, bad)
        assert ei.value.code == 1
        with pytest.raises(ValueError):
            tp.Passive(grid, bad[:-1])
    finally:
        grid.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case_labels():
    from topopt_in_petsc_amd.api import passive_labels
    lab = passive_labels(KW["nxyz"], KW["xc"], SHAPES)
    lab.setflags(write=False)
    return lab


def _independent_loop(tp, labels, nit, ftype, proj, beta, eta):
    """main.cc's loop body with passive regions from the classes that were there before and torch indexing"""
    import torch
    nx, ny, nz = KW["nxyz"]
    h, volfrac, Xmin, Xmax, movlim = 2.0 / (nx - 1), KW["volfrac"], 0.0, 1.0, 0.2
    g = tp.Grid(nx, ny, nz, (h, h, h))
    le = tp.LinearElasticity(g, tp.SolverOptions(nlvls=KW["nlvls"], nu=0.3))
    le.SetUpLoadAndBC()
    flt = tp.Filter(g, ftype, KW["rmin"])
    lab = torch.from_numpy(np.array(labels)).cuda()
    idx, void, solid, passive = torch.nonzero(lab == 0).flatten(), lab == 1, lab == 2, lab != 0
    n, na, ns = lab.numel(), int((lab == 0).sum()), int((lab == 2).sum())
    x0 = (volfrac * n - ns) / na
    x = g.elem_vec(x0)
    x[void], x[solid] = Xmin, Xmax
    xa = torch.full((na,), x0, dtype=torch.float64, device="cuda")
    xT, xP, dfdx, dgdx = g.elem_vec(volfrac), g.elem_vec(volfrac), g.elem_vec(), g.elem_vec()
    xmin, xmax, xold = torch.zeros_like(xa), torch.zeros_like(xa), torch.full_like(xa, x0)
    mma = tp.MMA(g, xa, 1, n_global=na)

    def filter_project():
        flt.FilterProject(x, xT, xP, proj, beta, eta)
        xP[void], xP[solid] = 0.0, 1.0

    filter_project()
    hist = []
    for itr in range(1, nit + 1):
        fx, gx = le.ComputeObjectiveConstraintsSensitivities(dfdx, dgdx, xP, 1.0e-9, 1.0, 3.0, volfrac)
        if itr == 1:
            fscale = 10.0 / fx
        dfdx.mul_(fscale)
        dfdx[passive], dgdx[passive] = 0.0, 0.0
        flt.Gradients(x, xT, dfdx, [dgdx], proj, beta, eta)
        dfa, dga = dfdx[idx], dgdx[idx]
        mma.SetOuterMovelimit(Xmin, Xmax, movlim, xa, xmin, xmax)
        mma.Update(xa, dfa, [gx], [dga], xmin, xmax)
        x[idx] = xa
        ch = mma.DesignChange(xa, xold)
        if proj and (ch < 0.01 or itr % 10 == 0) and beta < 48.0 and gx < 0.000001:
            beta = min(beta + 1 if beta < 7 else beta * 1.2, 48.0)
        filter_project()
        hist.append(dict(fx=fx, gx=gx, ch=ch, lam=mma.state()[0]))
    out = dict(hist=hist, x=x.clone(), xPhys=xP.clone())
    g.close()
    return out


@pytest.mark.parametrize("proj", [False, True], ids=["plain", "projected"])
@pytest.mark.parametrize("ftype", [1, 2])
def test_driver_equals_an_independent_loop_bit_for_bit(tp, ftype, proj):
    """three design iterations, density and PDE filter, projection off and on at beta = 4: x, xPhys, fx, gx, ch and MMA's lam equal
    those of the loop above bit for bit; the regions are exact in xPhys and x"""
    import torch
    labels = _case_labels()
    beta, eta = (4.0, 0.5) if proj else (0.1, 0.0)
    t = tp.TopOpt(passive=SHAPES, filter=ftype, projectionFilter=proj, beta=beta, eta=eta, **KW)
    assert t.n_active == int((labels == 0).sum()) and np.array_equal(t.labels_own, labels)
    lams = []
    for _ in range(3):
        t.step()
        lams.append(t.mma.state()[0])
    want = _independent_loop(tp, labels, 3, ftype, proj, beta, eta)
    for r, lam, w in zip(t.history, lams, want["hist"]):
        print("filter %d proj %d itr %d: fx %r / %r, gx %r / %r, ch %r / %r, lam %r / %r, n_active %d"
              % (ftype, proj, r["itr"], r["fx"], w["fx"], r["gx"], w["gx"], r["ch"], w["ch"], lam, w["lam"], r["n_active"]))
    for r, lam, w in zip(t.history, lams, want["hist"]):
        assert (r["fx"], r["gx"], r["ch"], lam) == (w["fx"], w["gx"], w["ch"], w["lam"]) and r["n_active"] == t.n_active
    assert torch.equal(_bits(t.x), _bits(want["x"])) and torch.equal(_bits(t.xPhys), _bits(want["xPhys"]))
    lab = torch.from_numpy(np.array(labels)).cuda()
    assert bool((t.xPhys[lab == 2] == 1.0).all()) and bool((t.xPhys[lab == 1] == 0.0).all())
    assert bool((t.x[lab == 2] == t.Xmax).all()) and bool((t.x[lab == 1] == t.Xmin).all())
    assert torch.equal(t.xa, t.x[lab == 0]) and float((t.x[lab == 0] - t._x0).abs().max()) > 0.0
    t.grid.close()


def test_no_passive_elements_is_no_change(tp):
    """a label array of zeros: the history of passive=None bit for bit over three iterations"""
    import torch
    a = tp.TopOpt(**KW)
    b = tp.TopOpt(passive=np.zeros(16 * 8 * 8, dtype=np.uint8), **KW)
    for _ in range(3):
        ra, rb = a.step(), b.step()
        print("itr %d: fx %r / %r, gx %r / %r, ch %r / %r, mnd %r / %r" % (ra["itr"], ra["fx"], rb["fx"], ra["gx"], rb["gx"], ra["ch"],
                                                                         rb["ch"], ra["mnd"], rb["mnd"]))
        assert rb.pop("n_active") == 1024
        assert {k: v for k, v in ra.items() if k != "time"} == {k: v for k, v in rb.items() if k != "time"}
    assert torch.equal(_bits(a.x), _bits(b.x)) and torch.equal(_bits(a.xPhys), _bits(b.xPhys)) and torch.equal(_bits(b.xa), _bits(b.x))
    a.grid.close()
    b.grid.close()


def chain_rule_errors(tp, zero=True):
    """-> (errors of the six elements, their kinds, bound); zero=False leaves the Zero call out (the check that the test can fail)"""
    import torch
    labels = _case_labels()
    nx, ny, nz = KW["nxyz"]
    ex, ey, ez = nx - 1, ny - 1, nz - 1
    h, rmin, s = 2.0 / ex, KW["rmin"], 0.5
    g = tp.Grid(nx, ny, nz, (h, h, h))
    flt, pr = tp.Filter(g, 1, rmin), tp.Passive(g, labels)
    n, na = labels.size, pr.n_active
    rng = np.random.default_rng(23)
    w_h = rng.uniform(-1.0, 1.0, n)
    xa_h = rng.uniform(0.1, 0.45, na)                      # x + s stays below 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, xT, xP = g.elem_vec(), g.elem_vec(), g.elem_vec()
    pr.Impose([x], 0.0, 1.0)

    def xphys(xa_vals):
        pr.Scatter([dev(xa_vals)], [x])
        flt.FilterProject(x, xT, xP)
        pr.Impose([xP], 0.0, 1.0)
        return xP.cpu().numpy().astype(np.longdouble)

    # the elements: active ones with a passive face neighbour (five, spread over the candidates) and one with no passive element
    # within three elements along any axis
    L3 = labels.reshape(ez, ey, ex)
    pas = np.pad(L3 != 0, 1)
    face = (pas[1:-1, 1:-1, :-2] | pas[1:-1, 1:-1, 2:] | pas[1:-1, :-2, 1:-1] | pas[1:-1, 2:, 1:-1] | pas[:-2, 1:-1, 1:-1] | pas[2:, 1:-1, 1:-1])
    near = np.zeros_like(face)
    p3 = np.pad(L3 != 0, 3)
    for dk in range(7):
        for dj in range(7):
            for di in range(7):
                near |= p3[dk:dk + ez, dj:dj + ey, di:di + ex]
    active = (L3 == 0).reshape(-1)
    touching = np.nonzero(active & face.reshape(-1))[0]
    far = np.nonzero(active & ~near.reshape(-1))[0]
    assert touching.size >= 5 and far.size >= 1
    elems = [int(touching[k]) for k in np.linspace(0, touching.size - 1, 5).astype(int)] + [int(far[far.size // 2])]
    pos = {int(e): a for a, e in enumerate(np.nonzero(active)[0])}
    # the device's gradient: Gather(Gradients(Zero(w)))
    row, spare = dev(w_h), dev(w_h)
    if zero:
        pr.Zero([row])
    flt.Gradients(x, xT, row, [spare])
    grad = pr.packed_vec()
    pr.Gather([row], [grad])
    grad = grad.cpu().numpy()
    base = xphys(xa_h)
    w_ld = w_h.astype(np.longdouble)
    errs = []
    for e in elems:
        moved = xa_h.copy()
        moved[pos[e]] += s
        quotient = float((w_ld * (xphys(moved) - base)).sum() / np.longdouble(s))
        errs.append(abs(quotient - grad[pos[e]]))
        print("element %d (%s): device %.17g, difference quotient %.17g, off by %.3e" % (e, "touching" if e != elems[-1] else "far", grad[pos[e]], quotient, errs[-1]))
    # T: the terms of one filter sum, the elements closer than rmin (strict, as the filter counts)
    r = int(np.ceil(rmin / h))
    o = np.arange(-r, r + 1) * h
    T = int((np.sqrt(o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) < rmin).sum())
    bound = 5 * T * (T + 2) * 2.0 ** -53 * float(np.abs(w_h).max())
    print("T = %d stencil terms, max|w| = %.6f: bound %.3e" % (T, float(np.abs(w_h).max()), bound))
    g.close()
    return errs, bound


def test_chain_rule_stops_at_the_passive_elements(tp):
    """J(xa) = w . xPhys(xa), xPhys = Impose(FilterProject(Scatter(xa))) with the density filter and no projection, is linear in xa,
    so its difference quotient at the step s = 0.5 is dJ/dxa_k but for rounding.  The device's gradient Gather(Gradients(Zero(w))) is
    held to it on five active elements with a passive face neighbour and one far from any passive element.

    The bound, with eps = 2^-53, T the terms of a filter sum and x <= 1 everywhere (xa <= 0.45 + s):
      * an entry xTilde_i = (sum of <= T products H_ij x_j >= 0) / Hs_i carries a relative error of at most (T + 2) eps, so an
        absolute one of at most (T + 2) eps; the quotient sums w_i (xPhys+_i - xPhys_i) in 80-bit arithmetic over the <= T elements
        i whose sum holds x_k (the others see the same bits twice and give an exact 0), each difference off by at most 2 (T + 2) eps:
        |error of the quotient| <= T max|w| 2 (T + 2) eps / s = 4 T (T + 2) eps max|w|;
      * the device's entry is sum_i H_ik (w_i / Hs_i) over <= T terms of mixed sign, each at most max|w| in size (H_ik <= rmin =
        H_ii <= Hs_i): off by at most (T + 2) eps T max|w|.
    Together 5 T (T + 2) eps max|w| -- a multiple of eps (stencil terms) max|w|; with T = 19 it is 2.2e-13 max|w|.
    Measured: 0 .. 2.6e-16.  Checked once by hand that the test fails without the Zero call: the five touching elements are then
    off by 3.7e-3 .. 9.6e-2 (the filter carries w from the passive neighbours, whose xPhys does not move), the far one stays
    at 2.6e-16."""
    errs, bound = chain_rule_errors(tp)
    assert max(errs) <= bound, (errs, bound)


def objective_gradient_pairs(tp, passive, elems, s=1e-3):
    """-> [(dfdx, central difference of the true compliance)] of the elements, the state solved to rtol 1e-12; dfdx is the row MMA
    receives in the first iteration, over the objective's scale"""
    import torch
    t = tp.TopOpt(passive=passive, solver=tp.SolverOptions(nlvls=KW["nlvls"], rtol=1e-12), **KW)
    seen, update = [], t.mma.Update

    def spy(x, dfdx, gx, dgdx, xmin, xmax):
        seen.append(dfdx.clone())
        return update(x, dfdx, gx, dgdx, xmin, xmax)
    t.mma.Update = spy
    x0 = t.x.clone()
    t.step()
    dfdx = (seen[0] / t.fscale).cpu().numpy()
    if passive is not None:
        pos = {int(e): a for a, e in enumerate(np.nonzero(t.labels_own == 0)[0])}
        assert dfdx.size == t.n_active
    pairs = []
    for e in elems:
        f = []
        for sign in (1.0, -1.0):
            t.x.copy_(x0)
            t.x[e] += sign * s
            t._filter_project()
            f.append(t.physics.ComputeObjectiveConstraints(t.xPrint, t.Emin, t.Emax, t.penal, t.volfrac)[0])
        fd, an = (f[0] - f[1]) / (2 * s), float(dfdx[pos[e] if passive is not None else e])
        pairs.append((an, fd))
        print("%s element %d, step %g: dfdx %.12e, central difference %.12e, off by %.3e (%.3e of dfdx)"
              % ("passive" if passive is not None else "none   ", e, s, an, fd, abs(fd - an), abs(fd - an) / abs(an)))
    t.grid.close()
    return pairs


def test_objective_gradient_beside_the_solid_box(tp):
    """the packed dfdx of three active elements beside the solid box against the central difference (step 1e-3) of the true
    compliance, |difference - dfdx|.  The allowed error is measured: the same difference on the same mesh and elements through
    TopOpt(passive=None), times 4 for the different design point.

    The error is compared as it stands, not over each run's own |dfdx|: a sweep of the step over 1e-4 .. 4e-3 shows no s^2 trend in
    either run (both wander between 6e-13 and 7e-11), so what is measured is the rounding of the two compliances over 2 s, about
    1e-14 fx / (2 s), and fx has the same size in both runs -- while dfdx beside the box is 3.4 times smaller with the box solid
    (1.40e-4 against 4.73e-4 at element 61), so the same noise is 3.4 times more of it.  Measured at step 1e-3: without passive
    regions 7.5e-12, 6.2e-13, 4.2e-12 (1.6e-8, 2.3e-9, 6.4e-9 of dfdx); with them 1.7e-11, 1.4e-12, 5.4e-12 (1.2e-7, 1.6e-8,
    2.6e-8 of dfdx): 2.3 times the largest.  Over the sweep the ratio of the largest errors lies between 1.5 and 3.0."""
    # beside the box x in [1.75, 2], z in [0, 0.25] (elements i >= 14, k <= 1): i = 13 at k = 0 and 1, and k = 2 above it at i = 14
    elems = [13 + 16 * (3 + 8 * 0), 13 + 16 * (4 + 8 * 1), 14 + 16 * (3 + 8 * 2)]
    lab = _case_labels()
    assert all(lab[e] == 0 for e in elems) and lab[elems[0] + 1] == 2 and lab[elems[1] + 1] == 2 and lab[elems[2] - 128] == 2
    e_none = max(abs(fd - an) for an, fd in objective_gradient_pairs(tp, None, elems))
    e_passive = max(abs(fd - an) for an, fd in objective_gradient_pairs(tp, SHAPES, elems))
    print("objective gradient: without passive regions %.3e, with %.3e (allowed %.3e)" % (e_none, e_passive, 4 * e_none))
    assert e_passive <= 4 * e_none


def test_restart_files_continue_the_run_with_passive_regions(tp, tmp_path):
    """stop after iteration 3, restart from the files, run iterations 4 and 5: what tests/test_mma.py's restart test demands of a run
    without passive regions; the files keep their full-length layout"""
    from topopt_in_petsc_amd.mpiio import read_petsc_vecs
    kw = dict(KW, passive=SHAPES)
    ref = tp.TopOpt(**kw)
    ref.run(max_itr=5)
    wd = str(tmp_path)
    a = tp.TopOpt(workdir=wd, **kw)
    a.run(max_itr=3)
    vecs = read_petsc_vecs(os.path.join(wd, "Restart00.dat"))
    lab = _case_labels()
    assert len(vecs) == 6 and all(v.size == lab.size for v in vecs)
    packed = [a.regions.packed_vec() for _ in range(4)]
    a.mma.Restart(*packed)                                       # xo1, xo2, U, L as MMA holds them
    for v, p in zip(vecs[2:], packed):
        assert not v[lab != 0].any() and np.array_equal(v[lab == 0], p.cpu().numpy()) and p.abs().max() > 0
    assert np.array_equal(vecs[0], a.x.cpu().numpy()) and np.array_equal(vecs[1], a.xPhys.cpu().numpy())
    b = tp.TopOpt(restartFileVec=os.path.join(wd, "Restart00.dat"), restartFileItr=os.path.join(wd, "Restart00_itr_f0.dat"),
                  restartFileVecSol=os.path.join(wd, "RestartSol00.dat"), **kw)
    assert b.itr == 3 and b.fscale == pytest.approx(a.fscale, rel=1e-6)
    b.fscale = a.fscale        # the "%e" companion keeps 7 digits; compare the loop itself
    b.run(max_itr=5)
    for r0, r1 in zip(ref.history[3:], b.history):
        print("itr %d: fx %r, restarted %r; ch %r, restarted %r" % (r0["itr"], r0["fx"], r1["fx"], r0["ch"], r1["ch"]))
        assert r0["itr"] == r1["itr"] and r1["n_active"] == r0["n_active"]
        assert r1["fx"] == pytest.approx(r0["fx"], rel=1e-9)
    # xold is not part of the restart set: the first ch is against the start value
    assert b.history[1]["ch"] == pytest.approx(ref.history[4]["ch"], rel=1e-7, abs=1e-12)
    assert float((b.x - ref.x).abs().max()) < 1e-9
    for t in (ref, a, b):
        t.grid.close()
