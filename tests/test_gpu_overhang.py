"""Overhang filter on the device (tp_overhang) against the numpy restatement in 80-bit arithmetic of
tests/overhang_ref.py, whose docstring carries the formulas.

 1. Forward and transpose against the 80-bit restatement.  The bound is measured, not fixed: the double restatement's own
    distance d from the 80-bit one on the same input (xi absolute, the transpose relative to its maximum), times 16, floor
    64 * 2^-53.  The margin covers the device's pow and sqrt being a couple of ulps where libm's are within one; the order of the
    five-term sums is the same on both sides.
 2. TP_OVERHANG_CHUNK = 1, 2, 4, 8 give the same bits in xi and in the transpose (which reads the three coefficient arrays).
 3. Adjoint of three vectors at once equals three single-vector calls bit for bit.
 4. (J^T g) . W of the device against the central difference of the device's own Forward, h = 1e-6, relative 1e-6.
 5. The sandwich min(x, Xi) <= xi <= min(x, Xi) + sqrt(eps)/2 and the absence of NaN on the device's output (with 1).
 6. The driver with overhang="+z".

The meshes put tile edges and partial chunks to work: the tile is 32 x 8, so 70x37x11 has three tiles along x and five along y,
neither a multiple, and 11 layers, a multiple of neither 4 nor 8; 1x1x4 is a single column.  Every figure is printed with its
bound before it is asserted."""
import os

import numpy as np
import pytest

from tests import overhang_ref as ref

pytestmark = pytest.mark.gpu

LD = ref.LD
MESHES = [(70, 37, 11), (16, 12, 20), (3, 3, 3), (1, 1, 4)]
FIELDS = ["random", "checker", "zerolayers"]
EXISTING_KEYS = {"itr", "fx", "fx_scaled", "gx", "ch", "mnd", "time", "ksp_its", "ksp_rerr", "mma_inner"}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


@pytest.fixture
def chunk():
    """sets TP_OVERHANG_CHUNK (read on every call) and puts the environment back"""
    old = os.environ.get("TP_OVERHANG_CHUNK")

    def set_chunk(c):
        os.environ["TP_OVERHANG_CHUNK"] = str(c)
    yield set_chunk
    if old is None:
        os.environ.pop("TP_OVERHANG_CHUNK", None)
    else:
        os.environ["TP_OVERHANG_CHUNK"] = old


def _grid(tp, ne):
    return tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0 / ne[1])


@pytest.mark.parametrize("build", ["+z", "-z", "+y"])
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("ne", MESHES)
def test_forward_and_transpose_against_the_80_bit_restatement(tp, ne, kind, build):
    """checks 1 and 5"""
    ref.check_against_reference(tp, ne, build, kind)


@pytest.mark.parametrize("build", ["+z", "-y"])
@pytest.mark.parametrize("ne", MESHES)
def test_every_chunk_length_gives_the_same_bits(tp, chunk, ne, build):
    """check 2, all three fields; last_chunk reports what ran"""
    import torch
    grid = _grid(tp, ne)
    try:
        ov = tp.Overhang(grid, build)
        for kind in FIELDS:
            x, g = ref.references(ne, build, kind)[:2]
            res = {}
            for c in (1, 2, 4, 8):
                chunk(c)
                xi, gv = grid.elem_vec(), [ref.dev(v) for v in g]
                ov.Forward(ref.dev(x), xi)
                assert ov.last_chunk() == c
                ov.Adjoint(gv)
                assert ov.last_chunk() == c
                res[c] = [xi] + gv
            for c in (2, 4, 8):
                same = [torch.equal(a, b) for a, b in zip(res[1], res[c])]
                print("%s %s %s: chunk %d against 1: xi %s, transposes %s" % ("x".join(map(str, ne)), build, kind, c, same[0], same[1:]))
                assert all(same)
            # coefficients of one chunk length, transpose of another
            chunk(8)
            xi = grid.elem_vec()
            ov.Forward(ref.dev(x), xi)
            chunk(1)
            gv = [ref.dev(v) for v in g]
            ov.Adjoint(gv)
            assert all(torch.equal(a, b) for a, b in zip(res[1][1:], gv))
    finally:
        grid.close()


@pytest.mark.parametrize("c", [1, 8])
def test_three_vectors_at_once_equal_three_single_calls(tp, chunk, c):
    """check 3; at chunk 8 one launch carries three vectors, so eight vectors go in groups: held to the single calls as well"""
    import torch
    ne, build = (70, 37, 11), "+z"
    x, g = ref.references(ne, build, "random")[:2]
    rng = np.random.default_rng(23)
    g8 = list(g) + [rng.uniform(-1.0, 1.0, x.size) for _ in range(5)]
    chunk(c)
    grid = _grid(tp, ne)
    try:
        ov = tp.Overhang(grid, build)
        ov.Forward(ref.dev(x), grid.elem_vec())
        single = []
        for v in g8:
            t = ref.dev(v)
            ov.Adjoint([t])
            single.append(t)
        three = [ref.dev(v) for v in g]
        ov.Adjoint(three)
        eight = [ref.dev(v) for v in g8]
        ov.Adjoint(eight)
        assert all(torch.equal(a, b) for a, b in zip(three, single)) and all(torch.equal(a, b) for a, b in zip(eight, single))
        assert float(single[0].abs().max()) > 0
        with pytest.raises(tp.TopOptError) as ei:
            ov.Adjoint([ref.dev(v) for v in g8] + [ref.dev(g[0])])     # nine
        assert ei.value.code == 1
    finally:
        grid.close()


@pytest.mark.parametrize("build", ["+z", "-z", "+y", "-y"])
@pytest.mark.parametrize("ne", [(16, 12, 20), (70, 37, 11)])
def test_transpose_against_central_differences_of_the_device(tp, ne, build):
    """check 4"""
    h = 1e-6
    rng = np.random.default_rng(11)
    n = ne[0] * ne[1] * ne[2]
    x, W, g = rng.uniform(0.1, 0.9, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    grid = _grid(tp, ne)
    try:
        ov = tp.Overhang(grid, build)
        fp, fm, f0 = grid.elem_vec(), grid.elem_vec(), grid.elem_vec()
        ov.Forward(ref.dev(x + h * W), fp)
        ov.Forward(ref.dev(x - h * W), fm)
        ov.Forward(ref.dev(x), f0)
        jg = ref.dev(g)
        ov.Adjoint([jg])
        an = float((jg.cpu().numpy().astype(LD) * W).sum())
        fd = float((g * (fp.cpu().numpy().astype(LD) - fm.cpu().numpy().astype(LD))).sum() / (2 * LD(h)))
        err = abs(fd - an) / abs(an)
        print("%s %s: (J^T g).W %.9e, central difference %.9e, off by %.3e (bound 1e-6)" % ("x".join(map(str, ne)), build, an, fd, err))
        assert err <= 1e-6
    finally:
        grid.close()


def test_a_transpose_needs_a_forward_call_and_parameters_reset_it(tp):
    ne = (16, 12, 20)
    grid = _grid(tp, ne)
    try:
        ov = tp.Overhang(grid, "+z")
        g = grid.elem_vec(1.0)
        with pytest.raises(tp.TopOptError) as ei:
            ov.Adjoint([g])
        assert ei.value.code == 1
        x, xi = ref.dev(ref.field("random", ne)), grid.elem_vec()
        with pytest.raises(tp.TopOptError):
            ov.Forward(x, x)
        ov.Forward(x, xi)
        ov.Adjoint([g])
        ov.params(20.0, 1e-3, 0.4)
        with pytest.raises(tp.TopOptError):
            ov.Adjoint([g])
        with pytest.raises(tp.TopOptError):
            ov.params(3.0, 1e-4, 0.5)
        # other parameters reach the kernels: against the restatement with them, to the floor-or-16-d rule of check 1
        ov.Forward(x, xi)
        fl = ref.forward(x.cpu().numpy(), ne, "+z", LD, 20.0, 1e-3, 0.4)["xi"]
        fd = ref.forward(x.cpu().numpy(), ne, "+z", np.float64, 20.0, 1e-3, 0.4)["xi"]
        d, e = float(np.abs(fd.astype(LD) - fl).max()), float(np.abs(xi.cpu().numpy().astype(LD) - fl).max())
        print("P = 20, eps = 1e-3, xi0 = 0.4: double off by d = %.3e, device by %.3e" % (d, e))
        assert e <= max(16 * d, 64 * ref.U53)
    finally:
        grid.close()


def test_driver_with_the_overhang_filter(tp):
    """check 6: 32x16x16, volfrac 0.3, overhang "+z", ten iterations"""
    import torch
    kw = dict(nxyz=(33, 17, 17), volfrac=0.3, nlvls=3)
    t = tp.TopOpt(overhang="+z", **kw)
    assert t.m == 1 and t.xPrint is not t.xPhys
    hist = [t.step() for _ in range(10)]
    print("fx:", " ".join("%.4f" % r["fx"] for r in hist))
    print("gx:", " ".join("%.6f" % r["gx"] for r in hist))
    print("print_loss:", " ".join("%.6f" % r["print_loss"] for r in hist))
    assert set(hist[0]) == EXISTING_KEYS | {"print_loss"}
    assert all(np.isfinite(v) for r in hist for v in r.values())
    again = t.grid.elem_vec()
    t.overhang_filter.Forward(t.xPhys, again)
    assert torch.equal(again, t.xPrint)
    assert hist[-1]["fx"] < hist[0]["fx"]
    assert hist[-1]["gx"] <= 1e-3
    assert all(r["print_loss"] >= 0.0 for r in hist)
    t.grid.close()
    # overhang=None is the former code path: the same records as a run that never names the field, and no copy of xPhys
    a = tp.TopOpt(overhang=None, **kw)
    assert a.xPrint is a.xPhys and a.overhang_filter is None
    ha = [a.step() for _ in range(3)]
    a.grid.close()
    b = tp.TopOpt(**kw)
    hb = [b.step() for _ in range(3)]
    b.grid.close()
    for ra, rb in zip(ha, hb):
        assert set(ra) == EXISTING_KEYS
        assert {k: v for k, v in ra.items() if k != "time"} == {k: v for k, v in rb.items() if k != "time"}
