"""CPU-side checks of the casting filter's boundary: the header declares the tp_casting calls, the binding knows each with a
matching argument count, the ABI number stays, the argument rules answer before anything touches a device, the draw strings
parse, and the driver has the new fields and refuses the combinations it must, before any device object exists."""
import ctypes as C
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1
CALLS = (("tp_casting_create", 4), ("tp_casting_destroy", 1), ("tp_casting_set_params", 2), ("tp_casting_forward", 3),
         ("tp_casting_adjoint", 3), ("tp_casting_last_form", 1), ("tp_casting_get_q", 2))


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_casting_calls_and_the_binding_has_them():
    """the handle type and the seven functions on it: eight declarations, call by call"""
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+tp_casting\s+tp_casting\s*;", src)
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4
    assert lib.load_library().tp_abi_version() == 4


def test_argument_rules_answer_before_any_launch():
    """every TP_ERR_ARG comes before the first use of the grid's stream or of a device array, so a zeroed block of host memory
    can stand in for a handle or a grid (as tests/test_overhang_abi.py does); a zeroed grid has no layers, so every parting
    index above 0 lies outside it"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    cf = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    y = C.cast(C.create_string_buffer(64), C.c_void_p)
    out = C.c_void_p()
    assert L.tp_casting_create(None, cf, 2, 0) == TP_ERR_ARG
    assert L.tp_casting_create(C.byref(out), None, 2, 0) == TP_ERR_ARG
    for axis, parting in ((-1, 0), (3, 0), (7, 0), (0, -1), (1, -1), (2, -5), (0, 1), (1, 2), (2, 1 << 20)):   # cf stands in for a grid
        assert L.tp_casting_create(C.byref(out), cf, axis, parting) == TP_ERR_ARG
    assert not out.value
    assert L.tp_casting_destroy(None) == 0
    assert L.tp_casting_set_params(None, 1e-6) == TP_ERR_ARG
    for bad in (0.0, -1e-6, float("nan"), float("inf"), -float("inf")):
        assert L.tp_casting_set_params(cf, bad) == TP_ERR_ARG
    assert L.tp_casting_set_params(cf, 1e-6) == 0
    assert L.tp_casting_forward(None, x, y) == TP_ERR_ARG
    assert L.tp_casting_forward(cf, None, y) == TP_ERR_ARG
    assert L.tp_casting_forward(cf, x, None) == TP_ERR_ARG
    assert L.tp_casting_forward(cf, x, x) == TP_ERR_ARG
    one, nul = (C.c_void_p * 1)(x.value), (C.c_void_p * 2)(x.value, None)
    assert L.tp_casting_adjoint(None, 1, one) == TP_ERR_ARG
    assert L.tp_casting_adjoint(cf, 1, None) == TP_ERR_ARG
    assert L.tp_casting_adjoint(cf, 0, one) == TP_ERR_ARG
    assert L.tp_casting_adjoint(cf, 9, one) == TP_ERR_ARG
    assert L.tp_casting_adjoint(cf, 2, nul) == TP_ERR_ARG
    assert L.tp_casting_adjoint(cf, 1, one) == TP_ERR_ARG                    # no forward call on this handle yet
    assert L.tp_casting_last_form(None) == 0 and L.tp_casting_last_form(cf) == 0
    assert L.tp_casting_get_q(None, x) == TP_ERR_ARG
    assert L.tp_casting_get_q(cf, None) == TP_ERR_ARG
    assert L.tp_casting_get_q(cf, x) == TP_ERR_ARG                           # no forward call on this handle yet


def test_draw_strings():
    from topopt_in_petsc_amd.api import Casting
    ne = (70, 37, 11)
    assert Casting.parse("+x", ne) == (0, 0) and Casting.parse("-x", ne) == (0, 70)
    assert Casting.parse("+y", ne) == (1, 0) and Casting.parse("-y", ne) == (1, 37)
    assert Casting.parse("+z", ne) == (2, 0) and Casting.parse("-z", ne) == (2, 11)
    assert Casting.parse("x:33", ne) == (0, 33) and Casting.parse("y:1", ne) == (1, 1) and Casting.parse("z:10", ne) == (2, 10)
    assert Casting.parse("-z") == (2, None) and Casting.parse("z:400") == (2, 400)
    for bad in ("x", "z", "+", "", "up", "+w", "x:", "x:-1", "x:0", "x:70", "z:11", "y:1.5", "+x:3", "xy:3", " +x", None, 2):
        with pytest.raises(ValueError):
            Casting.parse(bad, ne)
    for name in ("Forward", "Adjoint", "params", "last_form", "Q"):
        assert hasattr(Casting, name)


def test_driver_has_the_casting_fields_and_refuses_before_any_device_object():
    """wrong strings, a parting index outside the mesh, a bad eps, casting with overhang, and casting wherever overhang is
    refused: heat, thermoelastic, robust.  All of it host arithmetic in __post_init__ ahead of the grid: no device needed"""
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["casting"] is None and f["casting_eps"] == 1e-6
    for bad in ("x", "up", "", "+w", "x:0", "x:64", "z:32", "y:99", "z:1.5"):        # the default mesh is 64 x 32 x 32 elements
        with pytest.raises(ValueError):
            TopOpt(casting=bad)
    for bad in (0.0, -1e-6, float("nan"), float("inf"), "1e-6"):
        with pytest.raises(ValueError):
            TopOpt(casting="+z", casting_eps=bad)
    with pytest.raises(ValueError, match="overhang"):
        TopOpt(casting="+z", overhang="+z")
    with pytest.raises(ValueError, match="casting"):
        TopOpt(casting="+z", physics="heat")
    with pytest.raises(ValueError, match="casting"):
        TopOpt(casting="y:8", physics="thermoelastic", alpha=1e-3)
    with pytest.raises(ValueError, match="casting"):
        TopOpt(casting="-x", robust=(0.7, 0.5, 0.3), projectionFilter=True)
