"""Casting filter on the device (tp_casting) against the numpy restatement in 80-bit arithmetic of
tests/casting_ref.py, whose docstring carries the formulas.

 1. Forward and transpose against the 80-bit restatement.  The bound is measured, not fixed: the double restatement's own
    distance d from the 80-bit one on the same input (c absolute, the transpose relative to its maximum), times 16, floor
    64 * 2^-53.  The margin covers the device's sqrt and divide being within a couple of ulp where libm's are within one.  With it
    the sandwich, monotonicity to 4 ulp and the absence of NaN on the device's output.
 2. Equal bits across forms: TP_CASTING_XFORM 0 and 1; the x draw against the z and the y draw of the axis-swapped fields; the
    transpose of 3 and of 8 vectors at once against single-vector calls.
 3. (J^T g) . W of the device against the central difference of the device's own Forward: eps = 1e-4, h = 1e-6, relative 1e-6.
 4. The driver with casting="+z" and casting="y:8".

Meshes: 70x37x11 has partial x tiles (the tile is 32 cells), partial line blocks (64 lines) and 11 layers; 33x5x3 is one cell
past a tile; 4x1x1 is a single line along x, 1x1x4 has lines of length 1 along x.  On every mesh all six one-sided draws and the
two-sided ones at p = 1, n - 1 and a mid index off any tile edge (x:33 on 70).  Every figure is printed with its bound before it
is asserted."""
import os

import numpy as np
import pytest

from tests import casting_ref as ref

pytestmark = pytest.mark.gpu

LD = ref.LD
MESHES = ref.MESHES
FIELDS = ref.FIELDS
EXISTING_KEYS = {"itr", "fx", "fx_scaled", "gx", "ch", "mnd", "time", "ksp_its", "ksp_rerr", "mma_inner"}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


@pytest.fixture
def xform():
    """sets TP_CASTING_XFORM (read on every call) and puts the environment back"""
    old = os.environ.get("TP_CASTING_XFORM")

    def set_form(v):
        os.environ["TP_CASTING_XFORM"] = str(v)
    yield set_form
    if old is None:
        os.environ.pop("TP_CASTING_XFORM", None)
    else:
        os.environ["TP_CASTING_XFORM"] = old


def _grid(tp, ne):
    return tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0 / ne[1])


def _run(tp, grid, draw, x, g, eps=None):
    """-> [c] + transposes of g, device tensors, and the form that ran"""
    cf = tp.Casting(grid, draw)
    try:
        if eps is not None:
            cf.params(eps)
        c, gv = grid.elem_vec(), [ref.dev(v) for v in g]
        cf.Forward(ref.dev(x), c)
        form = cf.last_form()
        cf.Adjoint(gv)
        assert cf.last_form() == form
        return [c] + gv, form
    finally:
        cf.close()


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("ne", MESHES)
def test_forward_and_transpose_against_the_80_bit_restatement(tp, xform, ne, kind):
    """check 1, every draw of the mesh, the x draws in both forms"""
    grid = _grid(tp, ne)
    try:
        for draw in ref.draws(ne):
            for form in ((1, 0) if "x" in draw else (1,)):
                xform(form)
                ref.check_against_reference(tp, grid, ne, draw, kind)
    finally:
        grid.close()


@pytest.mark.parametrize("ne", MESHES)
def test_both_x_forms_give_the_same_bits(tp, xform, ne):
    """check 2a: TP_CASTING_XFORM 0 and 1 on every x draw and field, c and three transposes; q enters through the transposes,
    also crosswise: the coefficients of one form under the transpose of the other; last_form reports what ran"""
    import torch
    grid = _grid(tp, ne)
    try:
        for draw in [d for d in ref.draws(ne) if "x" in d]:
            for kind in FIELDS:
                x, g = ref.references(ne, draw, kind)[:2]
                res = {}
                for v, want in ((1, 2), (0, 3)):
                    xform(v)
                    res[v], form = _run(tp, grid, draw, x, g)
                    assert form == want
                same = [torch.equal(a, b) for a, b in zip(res[0], res[1])]
                print("%s %s %s: LDS-staged against strided walk: c %s, transposes %s" % (ref.name(ne), draw, kind, same[0], same[1:]))
                assert all(same)
                cf = tp.Casting(grid, draw)
                xform(1)
                cf.Forward(ref.dev(x), grid.elem_vec())
                xform(0)
                gv = [ref.dev(v) for v in g]
                cf.Adjoint(gv)
                assert cf.last_form() == 3 and all(torch.equal(a, b) for a, b in zip(res[1][1:], gv))
                cf.close()
        for draw in ("+y", "-z"):
            assert _run(tp, grid, draw, *ref.references(ne, draw, "random")[:2])[1] == 1
    finally:
        grid.close()


@pytest.mark.parametrize("ne", MESHES)
def test_x_draw_equals_the_z_and_y_draws_of_the_swapped_fields(tp, xform, ne):
    """check 2b: one recurrence through the same two per-cell functions whatever the axis and the kernel form"""
    import torch
    for other in ("z", "y"):
        a, b = 0, ref.AXES[other]
        ns = ref.swap(np.zeros(ne[0] * ne[1] * ne[2]), ne, a, b)[1]
        g1, g2 = _grid(tp, ne), _grid(tp, ns)
        try:
            for draw in [d for d in ref.draws(ne) if "x" in d]:
                x, g = ref.references(ne, draw, "random")[:2]
                xs, gs = ref.swap(x, ne, a, b)[0], [ref.swap(v, ne, a, b)[0] for v in g]
                for form in (1, 0):
                    xform(form)
                    rx = _run(tp, g1, draw, x, g)[0]
                    ro = _run(tp, g2, draw.replace("x", other), xs, gs)[0]
                    same = [bool(np.array_equal(ref.swap(p.cpu().numpy(), ne, a, b)[0], q.cpu().numpy())) for p, q in zip(rx, ro)]
                    print("%s %s (form %d) against %s on the swapped field: c %s, transposes %s"
                          % (ref.name(ne), draw, 2 if form else 3, draw.replace("x", other), same[0], same[1:]))
                    assert all(same)
        finally:
            g1.close()
            g2.close()


@pytest.mark.parametrize("draw", ["+x", "x:33", "-y", "z:5"])
def test_three_and_eight_vectors_at_once_equal_single_calls(tp, xform, draw):
    """check 2c, the x draws in both forms; nine vectors are refused"""
    import torch
    ne = (70, 37, 11)
    x, g = ref.references(ne, draw, "random")[:2]
    rng = np.random.default_rng(23)
    g8 = list(g) + [rng.uniform(-1.0, 1.0, x.size) for _ in range(5)]
    grid = _grid(tp, ne)
    try:
        for form in ((1, 0) if "x" in draw else (1,)):
            xform(form)
            cf = tp.Casting(grid, draw)
            cf.Forward(ref.dev(x), grid.elem_vec())
            single = []
            for v in g8:
                t = ref.dev(v)
                cf.Adjoint([t])
                single.append(t)
            three = [ref.dev(v) for v in g]
            cf.Adjoint(three)
            eight = [ref.dev(v) for v in g8]
            cf.Adjoint(eight)
            assert all(torch.equal(a, b) for a, b in zip(three, single)) and all(torch.equal(a, b) for a, b in zip(eight, single))
            assert float(single[0].abs().max()) > 0
            with pytest.raises(tp.TopOptError) as ei:
                cf.Adjoint([ref.dev(v) for v in g8] + [ref.dev(g[0])])     # nine
            assert ei.value.code == 1
            cf.close()
    finally:
        grid.close()


@pytest.mark.parametrize("ne", MESHES)
def test_transpose_against_central_differences_of_the_device(tp, ne):
    """check 3: random field, eps = 1e-4 (at 1e-6 the curvature 1 / sqrt(eps) of the kink puts a checkerboard at 1.1e-6)"""
    h, eps = 1e-6, 1e-4
    rng = np.random.default_rng(11)
    n = ne[0] * ne[1] * ne[2]
    x, W, g = ref.field("random", ne), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    grid = _grid(tp, ne)
    try:
        for draw in ref.draws(ne):
            cf = tp.Casting(grid, draw)
            cf.params(eps)
            fp, fm, f0 = grid.elem_vec(), grid.elem_vec(), grid.elem_vec()
            cf.Forward(ref.dev(x + h * W), fp)
            cf.Forward(ref.dev(x - h * W), fm)
            cf.Forward(ref.dev(x), f0)
            jg = ref.dev(g)
            cf.Adjoint([jg])
            cf.close()
            an = float((jg.cpu().numpy().astype(LD) * W).sum())
            fd = float((g * (fp.cpu().numpy().astype(LD) - fm.cpu().numpy().astype(LD))).sum() / (2 * LD(h)))
            err = abs(fd - an) / abs(an)
            print("%s %s: (J^T g).W %.9e, central difference %.9e, off by %.3e (bound 1e-6)" % (ref.name(ne), draw, an, fd, err))
            assert err <= 1e-6
    finally:
        grid.close()


def test_a_transpose_needs_a_forward_call_and_the_parameter_resets_it(tp):
    ne = (16, 12, 20)
    grid = _grid(tp, ne)
    try:
        cf = tp.Casting(grid, "z:7")
        g = grid.elem_vec(1.0)
        with pytest.raises(tp.TopOptError) as ei:
            cf.Adjoint([g])
        assert ei.value.code == 1
        x, c = ref.dev(ref.field("random", ne)), grid.elem_vec()
        with pytest.raises(tp.TopOptError):
            cf.Forward(x, x)
        cf.Forward(x, c)
        cf.Adjoint([g])
        cf.params(1e-3)
        with pytest.raises(tp.TopOptError):
            cf.Adjoint([g])
        with pytest.raises(tp.TopOptError):
            cf.params(0.0)
        with pytest.raises(ValueError):
            tp.Casting(grid, "z:20")
        # another eps reaches the kernels: against the restatement with it, to the floor-or-16-d rule of check 1
        cf.Forward(x, c)
        fl = ref.forward(x.cpu().numpy(), ne, "z:7", LD, 1e-3)["c"]
        fd = ref.forward(x.cpu().numpy(), ne, "z:7", np.float64, 1e-3)["c"]
        d, e = float(np.abs(fd.astype(LD) - fl).max()), float(np.abs(c.cpu().numpy().astype(LD) - fl).max())
        print("eps = 1e-3: double off by d = %.3e, device by %.3e" % (d, e))
        assert e <= max(16 * d, 64 * ref.U53)
    finally:
        grid.close()


@pytest.mark.parametrize("draw", ["+z", "y:8"])
def test_driver_with_the_casting_filter(tp, draw):
    """check 4: 32x16x16, volfrac 0.3, ten iterations"""
    import torch
    ne = (32, 16, 16)
    t = tp.TopOpt(nxyz=(33, 17, 17), volfrac=0.3, nlvls=3, casting=draw)
    assert t.m == 1 and t.xPrint is not t.xPhys and t.overhang_filter is None
    hist = [t.step() for _ in range(10)]
    print("fx:", " ".join("%.4f" % r["fx"] for r in hist))
    print("gx:", " ".join("%.6f" % r["gx"] for r in hist))
    print("cast_fill:", " ".join("%.6f" % r["cast_fill"] for r in hist))
    assert set(hist[0]) >= EXISTING_KEYS and "cast_fill" in hist[0]
    assert all(np.isfinite(v) for r in hist for v in r.values())
    assert hist[-1]["fx"] < hist[0]["fx"]
    assert all(r["cast_fill"] >= 0.0 for r in hist)
    again = t.grid.elem_vec()
    t.casting_filter.Forward(t.xPhys, again)
    assert torch.equal(again, t.xPrint)
    xp, c = t.xPhys.cpu().numpy(), t.xPrint.cpu().numpy()
    mono = ref.monotone_breach_ulps(c, ne, draw)
    # the sandwich's two sides are exact; c carries its roundings: five operations per step on numbers below 2, at most 16 steps
    br, tol = ref.sandwich_breach(xp, c.astype(LD), ne, draw, t.casting_eps), 16 * 5 * 2 * ref.U53
    print("%s: largest rise of xPrint along a sweep %.2f ulp (allowed 4); xPrint leaves the sandwich around hardcummax(xPhys) by %.3e "
          "(allowed %.3e)" % (draw, mono, br, tol))
    assert mono <= 4.0 and br <= tol
    t.grid.close()


def test_driver_without_casting_is_the_former_code_path(tp):
    """casting=None: the same records as a run that never names the field, bit for bit, and no copy of xPhys"""
    kw = dict(nxyz=(33, 17, 17), volfrac=0.3, nlvls=3)
    a = tp.TopOpt(casting=None, **kw)
    assert a.xPrint is a.xPhys and a.casting_filter is None
    ha = [a.step() for _ in range(3)]
    a.grid.close()
    b = tp.TopOpt(**kw)
    hb = [b.step() for _ in range(3)]
    b.grid.close()
    for ra, rb in zip(ha, hb):
        assert set(ra) == EXISTING_KEYS
        assert {k: v for k, v in ra.items() if k != "time"} == {k: v for k, v in rb.items() if k != "time"}
