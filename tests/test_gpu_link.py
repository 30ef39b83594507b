"""Design-variable linking on the device (tp_link, TopOpt(link=...)).

Expand and pick move data, so they are held to numpy indexing byte for byte.  Fold is a sum with one fixed order, so every kernel
form is held to the float64 restatement of that order (tests/link_ref.py) bit for bit, on fields that make the order visible.  The
driver is held to a loop written here from the classes that existed before (LinearElasticity, Filter, MMA(n_global=...)) with torch
indexing where the driver uses the new kernels: both sides run the same kernels in the same order everywhere else, so the records
and the designs are equal bit for bit."""
import os

import numpy as np
import pytest

from tests import link_ref as lr

pytestmark = pytest.mark.gpu

NVECS = (1, 2, 9, 12)
NAN_BITS = 0x7FF8000000000000
ROW_CAP = 512          # form 2 stages x rows of at most this many elements (csrc/link.h: LINK_ROW_CAP)
# the driver's case: 16 x 8 x 8 elements, 3 levels, the cantilever
KW = dict(nxyz=(17, 9, 9), xc=(0.0, 2.0, 0.0, 1.0, 0.0, 1.0), nlvls=3, rmin=0.2, volfrac=0.3)
NE = (16, 8, 8)
KERNEL_CASES = [(ne, None) for ne in lr.BOXES] + [lr.BIG_MIRROR]


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _bits(t):
    import torch
    return t.view(torch.int64)


def _payload(n, v):
    """n NaNs, each with its own payload: an entry that is not written comes back with these very bytes"""
    import torch
    return (torch.arange(n, dtype=torch.int64, device="cuda") + (NAN_BITS + 1 + (v << 32))).view(torch.float64)


def _random_bits(n, seed):
    """n doubles of arbitrary bytes (NaNs, infinities, denormals and both zeros among them)"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, device="cuda", generator=gen).view(torch.float64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fold_fields(spec, ne):
    """three base fields and their float64 folds: mixed magnitudes with both signs and zeros, the same with all -0.0 orbits, a
    0/1 design.  Vector v of a call is base v % 3 times 2^(v // 3) -- a power of two scales every partial sum exactly, so its
    fold is the base's times the same power"""
    n = ne[0] * ne[1] * ne[2]
    bases = [lr.order_field(n, 3 + n), lr.negative_zero_field(spec, ne, 5 + n), lr.design_field(n, 7 + n)]
    return bases, [lr.fold(spec, ne, b) for b in bases]


def _check_maps(tp, grid, ne, spec, forms_seen):
    import torch
    n = ne[0] * ne[1] * ne[2]
    lk = tp.Link(grid, lr.spec_dict(spec))
    nr = lr.reduced_counts(spec, ne)
    nred = nr[0] * nr[1] * nr[2]
    assert lk.counts() == (nred, nr) and lk.n_reduced == nred and lk.last_form() == 0
    rmap = _dev(lr.reduced_map(spec, ne))
    first = _dev(lr.pick(spec, ne, np.arange(n)))
    bases, folds = _fold_fields(spec, ne)
    two_applies = spec[0][0] != "none" and ne[0] <= ROW_CAP
    for nvec in NVECS:
        what = "%s %s nvec=%d" % ("x".join(map(str, ne)), lr.spec_name(spec), nvec)
        # expand: every entry written, with the bytes of its reduced variable
        red = [_random_bits(nred, 100 * v + nvec) for v in range(nvec)]
        keep = [r.clone() for r in red]
        full = [_payload(n, v) for v in range(nvec)]
        lk.Expand(red, full)
        for v in range(nvec):
            assert torch.equal(_bits(full[v]), _bits(keep[v])[rmap]), what + ": expand"
            assert torch.equal(_bits(red[v]), _bits(keep[v])), what + ": expand wrote its source"
        # pick: the first member of every orbit
        src = [_random_bits(n, 200 * v + nvec) for v in range(nvec)]
        keep = [s.clone() for s in src]
        out = [_payload(nred, v) for v in range(nvec)]
        lk.Pick(src, out)
        for v in range(nvec):
            assert torch.equal(_bits(out[v]), _bits(keep[v])[first]), what + ": pick"
            assert torch.equal(_bits(src[v]), _bits(keep[v])), what + ": pick wrote its source"
        # fold: the canonical order, every form
        src = [_dev(bases[v % 3] * 2.0 ** (v // 3)) for v in range(nvec)]
        want = [_dev(folds[v % 3] * 2.0 ** (v // 3)) for v in range(nvec)]
        for form in (0, 1, 2):
            lk.set_form(form)
            out = [_payload(nred, v) for v in range(nvec)]
            lk.Fold(src, out)
            ran = lk.last_form()
            rule = 2 if two_applies and spec[0][0] == "extrude" and spec[1][0] == spec[2][0] == "none" else 1      # form 0: the measured rule
            assert ran == (1 if form == 1 or not two_applies else 2 if form == 2 else rule), what + ": form %d ran %d" % (form, ran)
            forms_seen.add((form, ran))
            for v in range(nvec):
                assert torch.equal(_bits(out[v]), _bits(want[v])), what + ": fold, form %d (ran %d), vector %d" % (form, ran, v)
        lk.set_form(0)
    lk.close()


@pytest.mark.parametrize("ne,only", KERNEL_CASES, ids=["x".join(map(str, ne)) + ("_" + lr.spec_name(only).replace(":", "_") if only else "") for ne, only in KERNEL_CASES])
def test_kernels_equal_the_restatement_bit_for_bit(tp, ne, only):
    """expand, pick and fold (forms 0, 1 and 2) with 1, 2, 9 and 12 vectors on every spec the box admits.  96 x 80 x 72 has 552 960
    full elements and 192 x 80 x 72 under x:mirror as many reduced ones: one pass beyond the 2048 x 256 threads of a launch"""
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0)
    seen = set()
    try:
        assert grid.n_own_elems == ne[0] * ne[1] * ne[2]
        for spec in ([only] if only else lr.specs_for(ne)):
            _check_maps(tp, grid, ne, spec, seen)
        assert (1, 1) in seen and (2, 2) in seen       # x linked rows of at most ROW_CAP elements were among the specs
    finally:
        grid.close()


@pytest.mark.parametrize("ex", [ROW_CAP, ROW_CAP + 2], ids=["at_the_cap", "above_the_cap"])
def test_forms_on_each_side_of_the_staging_cap(tp, ex):
    """a row of 512 elements is staged (form 2 runs), one of 514 is not (form 1 runs whatever was asked for); same bits"""
    ne = (ex, 3, 2)
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0)
    try:
        for spec in ((lr.MIRROR, lr.NONE, lr.NONE), (lr.repeat(2), lr.NONE, lr.NONE), (lr.EXTRUDE, lr.NONE, lr.NONE),
                     (lr.MIRROR, lr.MIRROR, lr.EXTRUDE)):
            seen = set()
            _check_maps(tp, grid, ne, spec, seen)
            assert ((2, 2) in seen) == (ex <= ROW_CAP) and ((2, 1) in seen) == (ex > ROW_CAP), (ex, seen)
    finally:
        grid.close()


def test_vector_counts_outside_1_to_12_and_shared_vectors_are_refused(tp):
    grid = tp.Grid(7, 5, 3, 1.0)
    try:
        lk = tp.Link(grid, "x:mirror")
        full, red = [grid.elem_vec() for _ in range(13)], [lk.reduced_vec() for _ in range(13)]
        for f, r in (([], []), (full, red)):
            for call in (lambda: lk.Expand(r, f), lambda: lk.Fold(f, r), lambda: lk.Pick(f, r)):
                with pytest.raises(tp.TopOptError) as ei:
                    call()
                assert ei.value.code == 1
        with pytest.raises(tp.TopOptError) as ei:
            lk.Fold([full[0], full[1]], [red[0], full[0][:lk.n_reduced]])       # full[0] is red[1]
        assert ei.value.code == 1
        with pytest.raises(tp.TopOptError):
            lk.set_form(3)
        with pytest.raises(ValueError):
            tp.Link(grid, "x:repeat:4")                                          # 6 elements along x
    finally:
        grid.close()


@pytest.mark.parametrize("mode", [lr.MIRROR, lr.repeat(2), lr.repeat(3)], ids=lambda m: ":".join(map(str, m)))
def test_fold_with_axes_swapped_gives_the_swapped_result(tp, mode):
    """a single-axis mirror or repeat sums the same members in the same order whichever axis carries it: the field transposed and the
    mode moved to y or z gives the transposed fold, bit for bit"""
    import torch
    ne = (12, 6, 6)
    f3 = lr.order_field(12 * 6 * 6, 41).reshape(6, 6, 12)                        # [z, y, x]
    outs = {}
    for axis, perm in ((0, (0, 1, 2)), (1, (0, 2, 1)), (2, (2, 1, 0))):           # the x axis of f3 becomes axis `axis`
        g3 = np.ascontiguousarray(f3.transpose(perm))
        box = (g3.shape[2], g3.shape[1], g3.shape[0])
        spec = [lr.NONE, lr.NONE, lr.NONE]
        spec[axis] = mode
        grid = tp.Grid(box[0] + 1, box[1] + 1, box[2] + 1, 1.0)
        lk = tp.Link(grid, lr.spec_dict(tuple(spec)))
        out = lk.reduced_vec()
        lk.Fold([_dev(g3.reshape(-1))], [out])
        nr = lk.nr
        outs[axis] = out.cpu().numpy().reshape(nr[2], nr[1], nr[0]).transpose(perm)   # back to [z, y, reduced x]
        grid.close()
    assert outs[0].shape == outs[1].shape == outs[2].shape
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64)) and np.array_equal(outs[0].view(np.int64), outs[2].view(np.int64))
    assert np.array_equal(outs[0].reshape(-1).view(np.int64), lr.fold((mode, lr.NONE, lr.NONE), ne, f3.reshape(-1)).view(np.int64))


# ---- the driver ------------------------------------------------------------------------------------------------------------

class TorchLink:
    """tests/link_ref.py on torch tensors: expand by indexing, fold as the same sequence of adds"""

    def __init__(self, spec, ne):
        self.rmap = _dev(lr.reduced_map(spec, ne))
        self.steps = [(_dev(e), _dev(ok)) for e, ok in lr.orbit_positions(spec, ne)]
        self.first = self.steps[0][0]
        self.nred = self.first.numel()

    def expand(self, red):
        return red[self.rmap]

    def fold(self, full):
        import torch
        acc = full[self.steps[0][0]].clone()
        started = self.steps[0][1].clone()
        assert bool(started.all())
        for e, ok in self.steps[1:]:
            acc = torch.where(ok, acc + full[e], acc)
        return acc

    def linked(self, x):
        """x equals the expansion of its orbits' first members, byte for byte"""
        import torch
        return torch.equal(_bits(x), _bits(x[self.first][self.rmap]))


def _independent_loop(tp, spec, nit, ftype, proj, beta, eta):
    """main.cc's loop body with linking from the classes that were there before and torch indexing"""
    import torch
    nx, ny, nz = KW["nxyz"]
    h, volfrac, Xmin, Xmax, movlim = 2.0 / (nx - 1), KW["volfrac"], 0.0, 1.0, 0.2
    g = tp.Grid(nx, ny, nz, (h, h, h))
    le = tp.LinearElasticity(g, tp.SolverOptions(nlvls=KW["nlvls"], nu=0.3))
    le.SetUpLoadAndBC()
    flt = tp.Filter(g, ftype, KW["rmin"])
    tl = TorchLink(spec, NE)
    x = g.elem_vec(volfrac)
    xr = torch.full((tl.nred,), volfrac, dtype=torch.float64, device="cuda")
    xT, xP, dfdx, dgdx = g.elem_vec(volfrac), g.elem_vec(volfrac), g.elem_vec(), g.elem_vec()
    xmin, xmax, xold = torch.zeros_like(xr), torch.zeros_like(xr), torch.full_like(xr, volfrac)
    mma = tp.MMA(g, xr, 1, n_global=tl.nred)
    flt.FilterProject(x, xT, xP, proj, beta, eta)
    hist = []
    for itr in range(1, nit + 1):
        fx, gx = le.ComputeObjectiveConstraintsSensitivities(dfdx, dgdx, xP, 1.0e-9, 1.0, 3.0, volfrac)
        if itr == 1:
            fscale = 10.0 / fx
        dfdx.mul_(fscale)
        flt.Gradients(x, xT, dfdx, [dgdx], proj, beta, eta)
        dfr, dgr = tl.fold(dfdx), tl.fold(dgdx)
        mma.SetOuterMovelimit(Xmin, Xmax, movlim, xr, xmin, xmax)
        mma.Update(xr, dfr, [gx], [dgr], xmin, xmax)
        x.copy_(tl.expand(xr))
        ch = mma.DesignChange(xr, xold)
        if proj and (ch < 0.01 or itr % 10 == 0) and beta < 48.0 and gx < 0.000001:
            beta = min(beta + 1 if beta < 7 else beta * 1.2, 48.0)
        flt.FilterProject(x, xT, xP, proj, beta, eta)
        hist.append(dict(fx=fx, gx=gx, ch=ch, lam=mma.state()[0]))
    out = dict(hist=hist, x=x.clone(), xPhys=xP.clone())
    g.close()
    return out


Y_SPECS = {"y:mirror": (lr.NONE, lr.MIRROR, lr.NONE), "y:repeat:2": (lr.NONE, lr.repeat(2), lr.NONE), "y:extrude": (lr.NONE, lr.EXTRUDE, lr.NONE)}


@pytest.mark.parametrize("name", list(Y_SPECS))
@pytest.mark.parametrize("proj", [False, True], ids=["plain", "projected"])
@pytest.mark.parametrize("ftype", [1, 2])
def test_driver_equals_an_independent_loop_bit_for_bit(tp, ftype, proj, name):
    """three design iterations, density and PDE filter, projection off and on at beta = 4: x, xPhys, fx, gx, ch and MMA's lam equal
    those of the loop above bit for bit; x is exactly linked after every iteration"""
    import torch
    spec = Y_SPECS[name]
    beta, eta = (4.0, 0.5) if proj else (0.1, 0.0)
    t = tp.TopOpt(link=name, filter=ftype, projectionFilter=proj, beta=beta, eta=eta, **KW)
    tl = TorchLink(spec, NE)
    assert t.n_reduced == tl.nred == t.xr.numel()
    lams = []
    for _ in range(3):
        t.step()
        lams.append(t.mma.state()[0])
        assert tl.linked(t.x) and torch.equal(_bits(t.x), _bits(tl.expand(t.xr)))
    want = _independent_loop(tp, spec, 3, ftype, proj, beta, eta)
    for r, lam, w in zip(t.history, lams, want["hist"]):
        print("%s filter %d proj %d itr %d: fx %r / %r, gx %r / %r, ch %r / %r, lam %r / %r, n_reduced %d"
              % (name, ftype, proj, r["itr"], r["fx"], w["fx"], r["gx"], w["gx"], r["ch"], w["ch"], lam, w["lam"], r["n_reduced"]))
    for r, lam, w in zip(t.history, lams, want["hist"]):
        assert (r["fx"], r["gx"], r["ch"], lam) == (w["fx"], w["gx"], w["ch"], w["lam"]) and r["n_reduced"] == tl.nred
    assert torch.equal(_bits(t.x), _bits(want["x"])) and torch.equal(_bits(t.xPhys), _bits(want["xPhys"]))
    assert float((t.x - KW["volfrac"]).abs().max()) > 0.0
    t.grid.close()


def test_all_none_is_no_change(tp):
    """a spec that links nothing: the history of link=None bit for bit over three iterations"""
    import torch
    a = tp.TopOpt(**KW)
    b = tp.TopOpt(link={"x": "none", "y": "none", "z": "none"}, **KW)
    for _ in range(3):
        ra, rb = a.step(), b.step()
        print("itr %d: fx %r / %r, gx %r / %r, ch %r / %r, mnd %r / %r" % (ra["itr"], ra["fx"], rb["fx"], ra["gx"], rb["gx"], ra["ch"],
                                                                         rb["ch"], ra["mnd"], rb["mnd"]))
        assert "n_reduced" not in ra and rb.pop("n_reduced") == 16 * 8 * 8
        assert {k: v for k, v in ra.items() if k != "time"} == {k: v for k, v in rb.items() if k != "time"}
    assert torch.equal(_bits(a.x), _bits(b.x)) and torch.equal(_bits(a.xPhys), _bits(b.xPhys)) and torch.equal(_bits(b.xr), _bits(b.x))
    a.grid.close()
    b.grid.close()


CHAIN_SPECS = ((lr.NONE, lr.MIRROR, lr.NONE), (lr.NONE, lr.EXTRUDE, lr.NONE), (lr.MIRROR, lr.repeat(2), lr.EXTRUDE))


@pytest.mark.parametrize("spec", CHAIN_SPECS, ids=lr.spec_name)
def test_chain_rule_through_the_fold(tp, spec):
    """J(xr) = w . xPhys(xr), xPhys = FilterProject(Expand(xr)) with the density filter and no projection, is linear in xr, so its
    difference quotient at the step s = 0.5 is dJ/dxr_j but for rounding.  The device's gradient Fold(Gradients(w)) is held to it
    on six reduced variables spread over the reduced box.

    The bound, as DESIGN 4.15 derives its own, with eps = 2^-53, T the terms of a filter sum, S the orbit size and x <= 1
    everywhere (xr <= 0.45 + s):
      * an entry of xTilde carries an absolute error of at most (T + 2) eps; the quotient sums w_i (xPhys+_i - xPhys_i) in 80-bit
        arithmetic over the <= S T elements whose filter sum holds a member of the orbit (the others see the same bits twice and give
        an exact 0), each difference off by at most 2 (T + 2) eps: |error of the quotient| <= S T max|w| 2 (T + 2) eps / s
        = 4 S T (T + 2) eps max|w|;
      * a single entry of Gradients(w) is sum_i H_ik (w_i / Hs_i) over <= T terms of at most max|w| each: off by at most
        (T + 2) eps T max|w| and at most T max|w| in size; the fold adds S of them with S - 1 roundings of partial sums of at most
        S T max|w|: off by at most S (T + 2) T eps max|w| + (S - 1) S T eps max|w|.
    Together (5 S T (T + 2) + (S - 1) S T) eps max|w|."""
    import torch
    nx, ny, nz = KW["nxyz"]
    h, rmin, s = 2.0 / NE[0], KW["rmin"], 0.5
    g = tp.Grid(nx, ny, nz, (h, h, h))
    flt, lk = tp.Filter(g, 1, rmin), tp.Link(g, lr.spec_dict(spec))
    n, nred = NE[0] * NE[1] * NE[2], lk.n_reduced
    rng = np.random.default_rng(29)
    w_h, xr_h = rng.uniform(-1.0, 1.0, n), rng.uniform(0.1, 0.45, nred)
    x, xT, xP = g.elem_vec(), g.elem_vec(), g.elem_vec()

    def xphys(vals):
        lk.Expand([_dev(vals)], [x])
        flt.FilterProject(x, xT, xP)
        return xP.cpu().numpy().astype(np.longdouble)

    base = xphys(xr_h)
    row, spare, grad = _dev(w_h), _dev(w_h), lk.reduced_vec()
    flt.Gradients(x, xT, row, [spare])
    lk.Fold([row], [grad])
    grad = grad.cpu().numpy()
    sizes = lr.orbit_sizes(spec, NE)
    r = int(np.ceil(rmin / h))
    o = np.arange(-r, r + 1) * h
    T = int((np.sqrt(o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) < rmin).sum())
    wmax, eps = float(np.abs(w_h).max()), 2.0 ** -53
    w_ld = w_h.astype(np.longdouble)
    worst = 0.0
    for j in [int(v) for v in np.linspace(0, nred - 1, 6).astype(int)]:
        moved = xr_h.copy()
        moved[j] += s
        quotient = float((w_ld * (xphys(moved) - base)).sum() / np.longdouble(s))
        S = int(sizes[j])
        bound = (5 * S * T * (T + 2) + (S - 1) * S * T) * eps * wmax
        err = abs(quotient - grad[j])
        worst = max(worst, err / bound)
        print("%s reduced variable %d (orbit of %d): device %.17g, difference quotient %.17g, off by %.3e (bound %.3e)"
              % (lr.spec_name(spec), j, S, grad[j], quotient, err, bound))
        assert err <= bound
    assert float(np.abs(grad).max()) > 1e-3 and worst <= 1.0
    g.close()


FD_STEPS = (1e-4, 4e-4, 1e-3, 4e-3)     # the sweep of DESIGN 4.22
FD_COMPARE = (1e-4,)                    # the step the test holds: see its docstring
FD_CASES = ((dict(x="none"), (lr.NONE, lr.NONE, lr.NONE)), ("y:mirror", Y_SPECS["y:mirror"]), ("y:extrude", Y_SPECS["y:extrude"]))


def objective_gradient_errors(tp, link, var, steps=FD_STEPS):
    """-> {step: |central difference of the true compliance - dfdx|} of reduced variable `var` (an element with link=None), the state
    solved to rtol 1e-12; dfdx is the row MMA receives in the first iteration, over the objective's scale"""
    t = tp.TopOpt(link=link, solver=tp.SolverOptions(nlvls=KW["nlvls"], rtol=1e-12), **KW)
    seen, update = [], t.mma.Update

    def spy(x, dfdx, gx, dgdx, xmin, xmax):
        seen.append(dfdx.clone())
        return update(x, dfdx, gx, dgdx, xmin, xmax)
    t.mma.Update = spy
    t.step()
    an = float((seen[0] / t.fscale)[var])
    x0 = t.grid.elem_vec(KW["volfrac"])                       # the design dfdx was taken at
    errs = {}
    for s in steps:
        f = []
        for sign in (1.0, -1.0):
            if t.linker is None:
                t.x.copy_(x0)
                t.x[var] += sign * s
            else:
                xr = t.linker.reduced_vec(KW["volfrac"])
                xr[var] += sign * s
                t.linker.Expand([xr], [t.x])
            t._filter_project()
            f.append(t.physics.ComputeObjectiveConstraints(t.xPrint, t.Emin, t.Emax, t.penal, t.volfrac)[0])
        fd = (f[0] - f[1]) / (2 * s)
        errs[s] = abs(fd - an)
        print("link %-10s variable %d, step %g: dfdx %.12e, central difference %.12e, off by %.3e (%.3e of dfdx)"
              % (link, var, s, an, fd, errs[s], errs[s] / abs(an)))
    t.grid.close()
    return errs


def test_objective_gradient_of_linked_variables(tp):
    """the folded dfdx of three reduced variables with orbits of 1, 2 and ne_y = 8 elements (all none, y:mirror, y:extrude) against
    central differences of the true compliance, |difference - dfdx|, beside the same quantity for three single elements with
    link=None measured in the same test.  A folded entry is the sum of S single derivatives, so the linked error may be
    4 S times the largest unlinked one.

    Measured over the sweep FD_STEPS = 1e-4, 4e-4, 1e-3, 4e-3: the unlinked elements are off by at most 3.5e-11, 2.9e-12,
    1.0e-11, 1.6e-10; all none repeats the first element's figures digit for digit; y:mirror 1.2e-11, 4.6e-13, 1.1e-11, 1.8e-10;
    y:extrude 1.9e-11, 2.1e-10, 1.3e-9, 2.1e-8.  The extruded variable shows a clean s^2 trend from 4e-4 on (x 6.2 and x 16 for
    steps x 2.5 and x 4: the truncation term of the central difference, the third derivative along a direction that moves eight
    elements at once), the single elements one from 1e-3 on; at 1e-4 neither does -- there the rounding of the two compliances
    over 2 s rules both -- so the comparison is made at 1e-4: 1.9e-11 against the allowed 4 x 8 x 3.5e-11 = 1.1e-9."""
    # the element (i, j, k) = (13, 3, 2) and what it belongs to: itself; its mirror pair in y (j = 3, 4); the whole y line
    e = 13 + 16 * (3 + 8 * 2)
    e_none = max(max(objective_gradient_errors(tp, None, v, FD_COMPARE).values()) for v in (e, e + 16, 5 + 16 * (1 + 8 * 6)))
    for (link, spec), var, S in zip(FD_CASES, (e, 13 + 16 * (3 + 4 * 2), 13 + 16 * 2), (1, 2, 8)):
        assert lr.orbit_sizes(spec, NE)[var] == S and lr.reduced_map(spec, NE)[e] == var
        err = max(objective_gradient_errors(tp, link, var, FD_COMPARE).values())
        print("objective gradient, orbit of %d: unlinked %.3e, linked %.3e (allowed %.3e)" % (S, e_none, err, 4 * S * e_none))
        assert err <= 4 * S * e_none


def test_restart_files_continue_the_run_with_links(tp, tmp_path):
    """stop after iteration 3, restart from the files, run iterations 4 and 5: what tests/test_mma.py's restart test demands of a run
    without links; the files keep their full-length layout, MMA's vectors expanded"""
    from topopt_in_petsc_amd.mpiio import read_petsc_vecs
    kw = dict(KW, link="y:mirror")
    spec = Y_SPECS["y:mirror"]
    ref = tp.TopOpt(**kw)
    ref.run(max_itr=5)
    wd = str(tmp_path)
    a = tp.TopOpt(workdir=wd, **kw)
    a.run(max_itr=3)
    vecs = read_petsc_vecs(os.path.join(wd, "Restart00.dat"))
    assert len(vecs) == 6 and all(v.size == 16 * 8 * 8 for v in vecs)
    reduced = [a.linker.reduced_vec() for _ in range(4)]
    a.mma.Restart(*reduced)                                      # xo1, xo2, U, L as MMA holds them
    for v, p in zip(vecs[2:], reduced):
        assert np.array_equal(v, lr.expand(spec, NE, p.cpu().numpy())) and p.abs().max() > 0
    assert np.array_equal(vecs[0], a.x.cpu().numpy()) and np.array_equal(vecs[1], a.xPhys.cpu().numpy())
    b = tp.TopOpt(restartFileVec=os.path.join(wd, "Restart00.dat"), restartFileItr=os.path.join(wd, "Restart00_itr_f0.dat"),
                  restartFileVecSol=os.path.join(wd, "RestartSol00.dat"), **kw)
    assert b.itr == 3 and b.fscale == pytest.approx(a.fscale, rel=1e-6)
    assert np.array_equal(b.xr.cpu().numpy(), a.xr.cpu().numpy()) and np.array_equal(b.x.cpu().numpy(), a.x.cpu().numpy())
    b.fscale = a.fscale        # the "%e" companion keeps 7 digits; compare the loop itself
    b.run(max_itr=5)
    for r0, r1 in zip(ref.history[3:], b.history):
        print("itr %d: fx %r, restarted %r; ch %r, restarted %r" % (r0["itr"], r0["fx"], r1["fx"], r0["ch"], r1["ch"]))
        assert r0["itr"] == r1["itr"] and r1["n_reduced"] == r0["n_reduced"]
        assert r1["fx"] == pytest.approx(r0["fx"], rel=1e-9)
    # xold is not part of the restart set: the first ch is against the start value
    assert b.history[1]["ch"] == pytest.approx(ref.history[4]["ch"], rel=1e-7, abs=1e-12)
    assert float((b.x - ref.x).abs().max()) < 1e-9
    for t in (ref, a, b):
        t.grid.close()


@pytest.mark.parametrize("extra", [dict(casting="+z"), dict(robust=(0.7, 0.5, 0.3), projectionFilter=True, beta=4.0)], ids=["casting", "robust"])
def test_links_combine_with_casting_and_with_robust(tp, extra):
    """three iterations of link with casting="+z" and of link with robust: finite records, x exactly linked"""
    import math
    spec = (lr.MIRROR, lr.MIRROR, lr.NONE)
    t = tp.TopOpt(link={"x": "mirror", "y": "mirror"}, **dict(KW, **extra))
    tl = TorchLink(spec, NE)
    for _ in range(3):
        r = t.step()
        print({k: v for k, v in r.items() if isinstance(v, float)})
        assert all(math.isfinite(v) for v in r.values() if isinstance(v, float)) and r["n_reduced"] == 8 * 4 * 8
        assert tl.linked(t.x)
    assert float((t.x - KW["volfrac"]).abs().max()) > 0.0
    t.grid.close()
