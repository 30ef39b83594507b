"""CPU-side checks of the overhang filter's boundary: the header declares the tp_overhang calls, the binding knows each with a
matching argument count, the ABI number stays, the argument rules answer before anything touches a device, the driver has the
new field -- and the numpy restatement the GPU tests measure against (tests/overhang_ref.py) is itself held to central
differences, to the sandwich property and to its fixed points."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import overhang_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1
LD = ref.LD
CALLS = (("tp_overhang_create", 4), ("tp_overhang_destroy", 1), ("tp_overhang_set_params", 4), ("tp_overhang_forward", 3),
         ("tp_overhang_adjoint", 3), ("tp_overhang_last_chunk", 1), ("tp_overhang_get_coefficients", 4))
MESHES = [(16, 12, 20), (70, 37, 11)]
FIELDS = ["random", "mid", "checker", "half", "ones", "zerolayers"]


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_overhang_calls_and_the_binding_has_them():
    """the handle type and the seven functions on it: eight declarations"""
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+tp_overhang\s+tp_overhang\s*;", src)
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4


def test_argument_rules_answer_before_any_launch():
    """every TP_ERR_ARG comes before the first use of the grid or of a device array, so a zeroed block of host memory can stand
    in for a handle or a grid (as tests/test_localvol_abi.py does)"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    ov = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    y = C.cast(C.create_string_buffer(64), C.c_void_p)
    out = C.c_void_p()
    assert L.tp_overhang_create(None, ov, 2, 1) == TP_ERR_ARG
    assert L.tp_overhang_create(C.byref(out), None, 2, 1) == TP_ERR_ARG
    for axis, sign in ((0, 1), (3, 1), (-1, 1), (2, 0), (2, 2), (1, -2)):     # ov stands in for a grid
        assert L.tp_overhang_create(C.byref(out), ov, axis, sign) == TP_ERR_ARG
    assert L.tp_overhang_destroy(None) == 0
    good = (40.0, 1e-4, 0.5)
    assert L.tp_overhang_set_params(None, *good) == TP_ERR_ARG
    for bad in ((0.5, 1e-4, 0.5), (float("nan"), 1e-4, 0.5), (40.0, 0.0, 0.5), (40.0, -1e-4, 0.5), (40.0, 1e-4, 0.0),
                (40.0, 1e-4, 1.0), (40.0, 1e-4, 1.5), (3.0, 1e-4, 0.5)):     # the last: Q = 3 - 2.32 < 1
        assert L.tp_overhang_set_params(ov, *bad) == TP_ERR_ARG
    assert L.tp_overhang_set_params(ov, *good) == 0
    assert L.tp_overhang_forward(None, x, y) == TP_ERR_ARG
    assert L.tp_overhang_forward(ov, None, y) == TP_ERR_ARG
    assert L.tp_overhang_forward(ov, x, None) == TP_ERR_ARG
    assert L.tp_overhang_forward(ov, x, x) == TP_ERR_ARG
    one, nul = (C.c_void_p * 1)(x.value), (C.c_void_p * 2)(x.value, None)
    assert L.tp_overhang_adjoint(None, 1, one) == TP_ERR_ARG
    assert L.tp_overhang_adjoint(ov, 1, None) == TP_ERR_ARG
    assert L.tp_overhang_adjoint(ov, 0, one) == TP_ERR_ARG
    assert L.tp_overhang_adjoint(ov, 9, one) == TP_ERR_ARG
    assert L.tp_overhang_adjoint(ov, 2, nul) == TP_ERR_ARG
    assert L.tp_overhang_adjoint(ov, 1, one) == TP_ERR_ARG                    # no forward call on this handle yet
    assert L.tp_overhang_last_chunk(None) == 0 and L.tp_overhang_last_chunk(ov) == 0
    assert L.tp_overhang_get_coefficients(None, x, y, x) == TP_ERR_ARG
    assert L.tp_overhang_get_coefficients(ov, x, y, x) == TP_ERR_ARG          # no forward call on this handle yet


def test_driver_has_the_overhang_field_and_refuses_other_strings():
    from topopt_in_petsc_amd.api import Overhang
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert "overhang" in f and f["overhang"] is None
    for name in ("Forward", "Adjoint", "params", "last_chunk", "Coefficients"):
        assert hasattr(Overhang, name)
    assert set(Overhang.BUILDS) == {"+z", "-z", "+y", "-y"}
    for bad in ("+x", "-x", "z", "up", ""):        # before the grid is made: no device needed
        with pytest.raises(ValueError):
            TopOpt(overhang=bad)


@pytest.mark.parametrize("ne", MESHES)
def test_restatement_transpose_against_its_own_central_differences(ne):
    """g . (F(x + h W) - F(x - h W)) / 2h against (J^T g) . W in 80-bit arithmetic, h = 1e-6, relative 1e-6"""
    h = LD(1e-6)
    rng = np.random.default_rng(11)
    n = ne[0] * ne[1] * ne[2]
    x, W, g = rng.uniform(0.1, 0.9, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    for build in ("+z", "-y"):
        f0 = ref.forward(x, ne, build)
        an = (ref.adjoint(f0, g, ne, build) * W).sum()
        fp = ref.forward(x.astype(LD) + h * W, ne, build)["xi"]
        fm = ref.forward(x.astype(LD) - h * W, ne, build)["xi"]
        fd = (g * (fp - fm)).sum() / (2 * h)
        err = float(abs(fd - an) / abs(an))
        print("%s %s: (J^T g).W %.9e, central difference off by %.3e (bound 1e-6)" % ("x".join(map(str, ne)), build, float(an), err))
        assert err <= 1e-6


@pytest.mark.parametrize("ne", MESHES + [(3, 3, 3), (1, 1, 4)])
@pytest.mark.parametrize("kind", FIELDS)
def test_restatement_sandwich_and_no_nan(ne, kind):
    """min(x, Xi) <= xi <= min(x, Xi) + sqrt(eps)/2 on every field, to the roundings of xi itself: four operations on numbers
    below 2 (4 * 2^-64 * 2 in 80-bit arithmetic); no NaN in xi or in the transpose, whole zero layers included"""
    x = ref.field(kind, ne)
    g = np.random.default_rng(5).uniform(-1.0, 1.0, x.size)
    for build in ("+z", "-z", "+y"):
        f = ref.forward(x, ne, build)
        out = ref.adjoint(f, g, ne, build)
        br = ref.sandwich_breach(x, f)
        print("%s %s %s: breach %.3e" % ("x".join(map(str, ne)), build, kind, br))
        assert br <= 8 * 2.0 ** -64
        assert all(np.isfinite(f[k].astype(np.float64)).all() for k in f) and np.isfinite(out.astype(np.float64)).all()


def test_restatement_fixed_points():
    """uniform 0.5: every interior cell keeps 0.5 to 1e-15 (Q is chosen so: five supports at xi0 give Xi = xi0, and x = Xi gives
    xi = x).  Interior means that the whole support cone lies inside the mesh -- a cell of layer l at least l cells from the
    in-plane boundary: the count stays 5 at the boundary, so a boundary cell falls below 0.5 and the deficit moves inwards by one
    cell per layer.  All ones: the published overshoot, settling at 1.00449, stays at or below 1.005"""
    ne = (16, 12, 20)
    xi = ref.layers(ref.forward(ref.field("half", ne), ne, "+z")["xi"], ne, "+z")
    dev = max(float(np.abs(xi[l, l:ne[1] - l, l:ne[0] - l] - LD(0.5)).max()) for l in range(6))
    edge = float(LD(0.5) - xi[1, 0, 0])
    one = ref.forward(ref.field("ones", ne), ne, "+z")["xi"]
    print("uniform 0.5: interior off by %.3e (bound 1e-15), the corner of layer 1 lies %.3e below; ones: max %.6f, top layer %.6f"
          % (dev, edge, float(one.max()), float(ref.layers(one, ne, "+z")[-1, 5, 8])))
    assert dev <= 1e-15 and edge > 1e-4
    assert float(one.max()) <= 1.005 and float(one.min()) >= 0.9
