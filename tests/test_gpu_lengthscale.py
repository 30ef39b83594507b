"""Geometric length-scale constraints on the device (tp_lengthscale) against the numpy restatement in 80-bit
arithmetic of tests/lengthscale_ref.py, whose docstring carries the formulas.

Bounds (as tests/test_gpu_coarse_direct.py takes its own): for S, g (relative) and dg, T (relative to the largest entry) the distance
d64 of the SAME restatement run in float64 from the 80-bit one is measured per case; the device is allowed 16 d64 -- the project's
margin for two correct float64 evaluations that differ by their summation order and their exp / tanh -- and never less than
64 * 2^-53.  Every figure is printed beside its bound before anything is asserted."""
import functools

import numpy as np
import pytest

from tests import lengthscale_ref as ref

pytestmark = pytest.mark.gpu

LD = ref.LD
ETA_S, ETA_V, EPS = 0.75, 0.25, 1e-6
KIND_NAMES = {1: "solid", 2: "void", 3: "both"}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _grid(tp, ne, h):
    return tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, tuple(h))


@functools.lru_cache(maxsize=None)
def _case(mesh, kind, proj):
    """computed once per case and left unchanged: the fields, the 80-bit results and the bounds"""
    ne, h = ref.MESHES[mesh]
    rt = ref.field(kind, ne, h)
    rb = ref.projected(rt, proj)
    bounds, r80 = ref.d64_bounds(rt, rb, ne, h, ref.default_c(h), proj, eta_s=ETA_S, eta_v=ETA_V, eps=EPS)
    return rt, rb, r80, bounds


def _call(tp, ls, grid, rt, rb, h, proj, kinds, grads=True):
    dgs = grid.elem_vec(7.0) if grads else None
    dgv = grid.elem_vec(7.0) if grads else None
    r = ls.Constraints(rt, rb, ref.default_c(h), ETA_S, ETA_V, EPS, KIND_NAMES[kinds], bool(proj), ref.BETA, ref.ETA, dg_solid=dgs,
                       dg_void=dgv)
    ts, tv = ls.Terms(bool(kinds & 1), bool(kinds & 2))
    return r, dict(solid=dgs, void=dgv), dict(solid=ts, void=tv)


@pytest.mark.parametrize("proj", [0, 1])
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("mesh", sorted(ref.MESHES))
def test_terms_sums_constraints_and_gradients_against_the_restatement(tp, mesh, kind, proj):
    """kinds 1, 2 and 3: T, S, g and dg inside their bounds; a call for one kind leaves the other's outputs alone; kinds = 3 gives the
    bits of kinds = 1 and kinds = 2"""
    import torch
    ne, h = ref.MESHES[mesh]
    rt_h, rb_h, r80, b = _case(mesh, kind, proj)
    grid = _grid(tp, ne, h)
    try:
        ls = tp.LengthScale(grid)
        rt, rb = _dev(rt_h), _dev(rb_h)
        got = {k: _call(tp, ls, grid, rt, rb, h, proj, k) for k in (1, 2, 3)}
        fails = []
        for k in (1, 2, 3):
            r, dg, T = got[k]
            for bit, name in ((1, "solid"), (2, "void")):
                if not k & bit:
                    assert r["g_" + name] is None and r["S_" + name] is None
                    assert torch.equal(dg[name], torch.full_like(dg[name], 7.0)), "kinds=%d wrote dg_%s" % (k, name)
                    continue
                e = dict(S=ref.distance(r["S_" + name], r80["S_" + name]), g=ref.distance(r["g_" + name], r80["g_" + name]),
                         dg=ref.distance(dg[name].cpu().numpy(), r80["dg_" + name], True),
                         T=ref.distance(T[name].cpu().numpy(), r80["T_" + name], True))
                print("%s %s proj=%d kinds=%d %s: S %.3e (bound %.3e); g %.3e (bound %.3e); dg %.3e (bound %.3e); T %.3e (bound %.3e)"
                      % (mesh, kind, proj, k, name, e["S"], b["S_" + name], e["g"], b["g_" + name], e["dg"], b["dg_" + name], e["T"],
                         b["T_" + name]), flush=True)
                fails += ["kinds=%d %s %s: %.3e > %.3e" % (k, name, q, e[q], b[q + "_" + name]) for q in e if not e[q] <= b[q + "_" + name]]
        assert not fails, fails
        for bit, name in ((1, "solid"), (2, "void")):
            one, both = got[bit], got[3]
            assert one[0]["S_" + name] == both[0]["S_" + name] and one[0]["g_" + name] == both[0]["g_" + name]
            assert torch.equal(one[1][name], both[1][name]) and torch.equal(one[2][name], both[2][name])
    finally:
        grid.close()


def test_two_calls_give_the_same_bits_and_the_forward_only_call_the_same_values(tp):
    import torch
    ne, h = ref.MESHES["b"]
    rt_h, rb_h, _, _ = _case("b", "random", 1)
    grid = _grid(tp, ne, h)
    try:
        ls = tp.LengthScale(grid)
        rt, rb = _dev(rt_h), _dev(rb_h)
        a, b = _call(tp, ls, grid, rt, rb, h, 1, 3), _call(tp, ls, grid, rt, rb, h, 1, 3)
        fwd = _call(tp, ls, grid, rt, rb, h, 1, 3, grads=False)
        assert a[0] == b[0] == fwd[0]
        for name in ("solid", "void"):
            assert torch.equal(a[1][name], b[1][name]) and torch.equal(a[2][name], b[2][name]) and torch.equal(a[2][name], fwd[2][name])
    finally:
        grid.close()


@pytest.mark.parametrize("proj", [0, 1])
@pytest.mark.parametrize("mesh", ["a", "b"])
def test_gradient_against_central_differences_of_the_device(tp, mesh, proj):
    """dg . W against (g(rt + s W) - g(rt - s W)) / (2 s) of the device's own g, s = 1e-6, relative 1e-6; the projected field the
    device is given follows the perturbed one"""
    ne, h = ref.MESHES[mesh]
    n, s = ne[0] * ne[1] * ne[2], 1e-6
    rt = ref.field("random", ne, h)
    W = np.random.default_rng(11).uniform(-1.0, 1.0, n)
    grid = _grid(tp, ne, h)
    try:
        ls = tp.LengthScale(grid)
        run = lambda f, grads: _call(tp, ls, grid, _dev(f), _dev(ref.projected(f, proj)), h, proj, 3, grads)
        r0, dg, _ = run(rt, True)
        rp, rm = run(rt + s * W, False)[0], run(rt - s * W, False)[0]
        errs = {}
        for name in ("solid", "void"):
            an = float((dg[name].cpu().numpy().astype(LD) * W).sum())
            fd = (rp["g_" + name] - rm["g_" + name]) / (2 * s)
            errs[name] = abs(fd - an) / abs(an)
            print("%s proj=%d %s: dg.W %.9e, central difference %.9e, off by %.3e (bound 1e-6)" % (mesh, proj, name, an, fd, errs[name]))
        assert max(errs.values()) <= 1e-6
    finally:
        grid.close()


@pytest.mark.parametrize("ftype", [1, 2])
def test_chain_through_the_filter_against_central_differences(tp, ftype):
    """x -> FilterProject -> Constraints: the central difference of g along W against GradientsFromTilde(x, [dg]) . W, s = 1e-6,
    relative 1e-6, 16x8x8, projection on.  The Helmholtz filter's solves run to rtol 1e-13: at its default 1e-8 the difference
    of two solves would carry 1e-8 / 1e-6 of the value"""
    ne, h = ref.MESHES["a"]
    n, s = ne[0] * ne[1] * ne[2], 1e-6
    rng = np.random.default_rng(17)
    x_h, W = rng.uniform(0.2, 0.8, n), rng.uniform(-1.0, 1.0, n)
    grid = _grid(tp, ne, h)
    try:
        po = tp.SolverOptions(nlvls=3, rtol=1e-13, dtol=1e3, max_it=200, nsmooth=2, ncoarse=10) if ftype == 2 else None
        flt, ls = tp.Filter(grid, ftype, 2.5 * h[0], po), tp.LengthScale(grid)
        xt, xp = grid.elem_vec(), grid.elem_vec()

        def run(xv, grads):
            x = _dev(xv)
            flt.FilterProject(x, xt, xp, True, ref.BETA, ref.ETA)
            r, dg, _ = _call(tp, ls, grid, xt, xp, h, 1, 3, grads)
            if grads:
                flt.GradientsFromTilde(x, [dg["solid"], dg["void"]])
            return r, dg

        r0, dg = run(x_h, True)
        rp, rm = run(x_h + s * W, False)[0], run(x_h - s * W, False)[0]
        errs = {}
        for name in ("solid", "void"):
            an = float((dg[name].cpu().numpy().astype(LD) * W).sum())
            fd = (rp["g_" + name] - rm["g_" + name]) / (2 * s)
            errs[name] = abs(fd - an) / abs(an)
            print("filter %d %s: g %.6e, dg.W %.9e, central difference %.9e, off by %.3e (bound 1e-6)"
                  % (ftype, name, r0["g_" + name], an, fd, errs[name]))
        assert max(errs.values()) <= 1e-6
    finally:
        grid.close()


def test_the_sensitivity_filter_has_no_transpose(tp):
    ne, h = ref.MESHES["a"]
    grid = _grid(tp, ne, h)
    try:
        flt = tp.Filter(grid, 0, 2.5 * h[0])
        with pytest.raises(tp.TopOptError) as ei:
            flt.GradientsFromTilde(grid.elem_vec(0.5), [grid.elem_vec(1.0)])
        assert ei.value.code == 1
    finally:
        grid.close()


def test_uniform_field_on_the_device(tp):
    """rt = 0.5: S_solid = n H(0.5) 0.0625 and the gradient is its pointwise part alone, the same value in every element"""
    ne, h = ref.MESHES["a"]
    n = ne[0] * ne[1] * ne[2]
    grid = _grid(tp, ne, h)
    try:
        ls = tp.LengthScale(grid)
        r, dg, _ = _call(tp, ls, grid, grid.elem_vec(0.5), grid.elem_vec(0.5), h, 0, 3)
        print("uniform: S_solid %.17g, S_void %.17g (n * 0.5 * 0.0625 = %.17g)" % (r["S_solid"], r["S_void"], n * 0.03125))
        assert r["S_solid"] == n * 0.03125 and r["S_void"] == n * 0.03125      # every term and every partial sum is exact
        for name in ("solid", "void"):
            assert float(dg[name].min()) == float(dg[name].max())
    finally:
        grid.close()


EXISTING_KEYS = {"itr", "fx", "fx_scaled", "gx", "ch", "mnd", "time", "ksp_its", "ksp_rerr", "mma_inner"}
NEW_KEYS = {"gx_solid", "gx_void", "length_S_solid", "length_S_void"}


def _spy(t):
    """what MMA receives: (gx, clones of the rows) of every Update"""
    seen, orig = [], t.mma.Update

    def update(x, dfdx, gx, dgdx, xmin, xmax):
        seen.append((list(gx), [d.clone() for d in dgdx]))
        return orig(x, dfdx, gx, dgdx, xmin, xmax)
    t.mma.Update = update
    return seen


def test_driver_with_the_length_scale_constraints(tp):
    """32x16x16, projection on, both kinds, six iterations"""
    import torch
    kw = dict(nxyz=(33, 17, 17), volfrac=0.5, nlvls=3, projectionFilter=True, length_scale="both")
    t = tp.TopOpt(**kw)
    assert t.m == 3 and len(t.dgdx) == 3 and t._k_length == (1, 2)
    assert t.length_scale_c == t.rmin ** 4 / (2.0 / 32) ** 2
    seen = _spy(t)
    hist = [t.step() for _ in range(6)]
    for key in ("gx", "gx_solid", "gx_void", "length_S_solid", "length_S_void", "mnd"):
        print(key + ":", " ".join("%.6g" % r[key] for r in hist))
    assert set(hist[0]) == EXISTING_KEYS | NEW_KEYS
    assert all(np.isfinite(r[k]) for r in hist for k in NEW_KEYS)
    assert seen[0][0][1:] == [hist[0]["gx_solid"], hist[0]["gx_void"]] and len(seen[0][1]) == 3
    t.grid.close()
    # before length_scale_start: recorded, but MMA sees g = -1 and a zero row
    t3 = tp.TopOpt(length_scale_start=3, **kw)
    seen3 = _spy(t3)
    r = t3.step()
    assert seen3[0][0][1:] == [-1.0, -1.0] and r["gx_solid"] == hist[0]["gx_solid"] and r["gx_void"] == hist[0]["gx_void"]
    assert all(torch.equal(row, torch.zeros_like(row)) for row in seen3[0][1][1:])
    assert torch.equal(seen3[0][1][0], seen[0][1][0])
    t3.grid.close()
    # the overhang filter does not see the length-scale rows: the same bits with and without it
    to = tp.TopOpt(overhang="+z", **kw)
    seeno = _spy(to)
    ro = to.step()
    assert ro["gx_solid"] == hist[0]["gx_solid"] and ro["gx_void"] == hist[0]["gx_void"]
    assert all(torch.equal(a, b) for a, b in zip(seeno[0][1][1:], seen[0][1][1:])) and float(seen[0][1][1].abs().max()) > 0.0
    to.grid.close()
    # off: nothing new
    t0 = tp.TopOpt(**dict(kw, length_scale=None))
    assert t0.m == 1 and t0.lengthscale is None and len(t0.dgdx) == 1
    assert set(t0.step()) == EXISTING_KEYS
    t0.grid.close()
