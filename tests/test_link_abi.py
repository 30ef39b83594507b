"""CPU-side checks of design-variable linking's boundary: the header declares the tp_link calls, the binding knows
each with a matching argument count, the ABI number stays, every argument rule answers before anything touches a device, the link
strings parse, and the driver refuses what it cannot run before it makes a grid."""
import ctypes as C
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1
CALLS = (("tp_link_create", 4), ("tp_link_destroy", 1), ("tp_link_counts", 3), ("tp_link_expand", 4), ("tp_link_fold", 4),
         ("tp_link_pick", 4), ("tp_link_set_form", 2), ("tp_link_last_form", 1))


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_link_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    assert re.search(r"typedef\s+struct\s+tp_link\s+tp_link\s*;", src)
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4
    assert lib.load_library().tp_abi_version() == 4
    assert re.search(r"#define\s+TP_LINK_MAXVEC\s+12\b", src) and lib.LINK_MAXVEC == 12


def test_argument_rules_answer_before_any_launch():
    """every TP_ERR_ARG comes before the first use of the handle or of the grid's stream, so zeroed blocks of host memory can stand
    in for both.  A zeroed grid has no elements and no ranks: creating a handle on it succeeds for every valid mode, and the three
    maps then return TP_OK without a launch"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    g = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    h = C.cast(C.create_string_buffer(1 << 12), C.c_void_p)       # a zeroed handle: no elements
    bufs = [C.create_string_buffer(64) for _ in range(26)]
    vec = lambda k: C.cast(bufs[k], C.c_void_p)
    arr = lambda ks: (C.c_void_p * max(len(ks), 1))(*[None if k is None else vec(k) for k in ks])
    i3 = lambda *v: (C.c_int * 3)(*v)
    a12, b12, a13 = arr(range(12)), arr(range(12, 24)), arr(range(13))
    out = C.c_void_p()
    # create
    assert L.tp_link_create(None, g, i3(0, 0, 0), i3(0, 0, 0)) == TP_ERR_ARG
    assert L.tp_link_create(C.byref(out), None, i3(0, 0, 0), i3(0, 0, 0)) == TP_ERR_ARG
    assert L.tp_link_create(C.byref(out), g, None, i3(0, 0, 0)) == TP_ERR_ARG
    assert L.tp_link_create(C.byref(out), g, i3(0, 0, 0), None) == TP_ERR_ARG
    for modes in ((-1, 0, 0), (4, 0, 0), (0, 7, 0), (0, 0, -2), (0, 0, 4)):
        assert L.tp_link_create(C.byref(out), g, i3(*modes), i3(2, 2, 2)) == TP_ERR_ARG, modes
    for modes, cells in (((2, 0, 0), (1, 0, 0)), ((2, 0, 0), (0, 0, 0)), ((0, 2, 0), (2, -3, 2)), ((0, 0, 2), (2, 2, 1))):
        assert L.tp_link_create(C.byref(out), g, i3(*modes), i3(*cells)) == TP_ERR_ARG, (modes, cells)
    assert not out.value
    assert L.tp_link_destroy(None) == 0
    # a handle on the zeroed grid: valid modes pass (cells are read for repeat only), counts of an empty box
    for modes, cells, nr in (((0, 0, 0), (0, 0, 0), (0, 0, 0)), ((1, 2, 3), (-5, 2, -5), (0, 0, 1)), ((3, 3, 3), (0, 0, 0), (1, 1, 1))):
        made = C.c_void_p()
        assert L.tp_link_create(C.byref(made), g, i3(*modes), i3(*cells)) == 0 and made.value
        n, got = C.c_long(7), (C.c_long * 3)(7, 7, 7)
        assert L.tp_link_counts(made, C.byref(n), got) == 0 and tuple(got) == nr and n.value == nr[0] * nr[1] * nr[2]
        assert L.tp_link_counts(made, None, None) == 0
        for nvec in (1, 12):
            assert L.tp_link_expand(made, nvec, a12, b12) == 0 and L.tp_link_fold(made, nvec, a12, b12) == 0
            assert L.tp_link_pick(made, nvec, a12, b12) == 0
        assert L.tp_link_last_form(made) == 0
        assert L.tp_link_destroy(made) == 0
    assert L.tp_link_counts(None, None, None) == TP_ERR_ARG
    # the three maps
    calls = (L.tp_link_expand, L.tp_link_fold, L.tp_link_pick)
    for nvec, x in ((1, None), (0, a12), (-1, a12), (13, a13), (2, arr([0, None])), (12, arr(list(range(11)) + [None]))):
        for call in calls:
            assert call(h, nvec, x, b12) == TP_ERR_ARG and call(h, nvec, b12, x) == TP_ERR_ARG, (nvec, call.__name__)
    shared = arr([12, 13, 1])
    for call in calls:
        assert call(None, 1, a12, b12) == TP_ERR_ARG
        for nvec, one, two in ((1, a12, a12), (3, a12, shared), (12, a12, arr(list(range(12, 23)) + [0]))):
            assert call(h, nvec, one, two) == TP_ERR_ARG and call(h, nvec, two, one) == TP_ERR_ARG
        assert call(h, 12, a12, b12) == 0                  # no element: nothing to launch
    # the form
    assert L.tp_link_set_form(None, 1) == TP_ERR_ARG
    for bad in (-1, 3, 17):
        assert L.tp_link_set_form(h, bad) == TP_ERR_ARG
    for form in (0, 1, 2):
        assert L.tp_link_set_form(h, form) == 0
    assert L.tp_link_last_form(None) == 0 and L.tp_link_last_form(h) == 0


def test_a_z_link_on_more_than_one_rank_and_a_cell_count_that_does_not_divide_are_refused():
    """these two rules read the grid's element and rank counts: a stand-in grid is a zeroed block in which every int is set to the
    value wanted -- whatever the layout, ex = ey = ez_own = nranks = that value, and nothing else of the block is read"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    i3 = lambda *v: (C.c_int * 3)(*v)
    out = C.c_void_p()
    six = (C.c_int * (1 << 12))(*([6] * (1 << 12)))         # 6 elements per axis on "6 ranks"
    g6 = C.cast(six, C.c_void_p)
    for modes in ((0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 2, 3)):
        assert L.tp_link_create(C.byref(out), g6, i3(*modes), i3(2, 2, 2)) == TP_ERR_ARG, modes
    for modes, cells in (((2, 0, 0), (4, 0, 0)), ((0, 2, 0), (0, 5, 0)), ((2, 2, 0), (2, 12, 0))):
        assert L.tp_link_create(C.byref(out), g6, i3(*modes), i3(*cells)) == TP_ERR_ARG, (modes, cells)
    assert not out.value
    made = C.c_void_p()
    assert L.tp_link_create(C.byref(made), g6, i3(1, 2, 0), i3(0, 3, 0)) == 0      # x and y links pass on several ranks
    n, nr = C.c_long(), (C.c_long * 3)()
    assert L.tp_link_counts(made, C.byref(n), nr) == 0 and tuple(nr) == (3, 2, 6) and n.value == 36
    assert L.tp_link_destroy(made) == 0
    one = (C.c_int * (1 << 12))(*([1] * (1 << 12)))         # one element per axis on one rank: z links pass
    made = C.c_void_p()
    assert L.tp_link_create(C.byref(made), C.cast(one, C.c_void_p), i3(1, 3, 3), i3(0, 0, 0)) == 0
    assert L.tp_link_counts(made, C.byref(n), nr) == 0 and tuple(nr) == (1, 1, 1) and n.value == 1
    assert L.tp_link_destroy(made) == 0


def test_link_strings():
    from topopt_in_petsc_amd.api import Link, parse_link
    ne = (12, 6, 5)
    assert parse_link({"x": "mirror", "y": ("repeat", 3), "z": "extrude"}, ne) == ((1, 2, 3), (0, 3, 0))
    assert parse_link(["x:mirror", "y:repeat:3", "z:extrude"], ne) == ((1, 2, 3), (0, 3, 0))
    assert parse_link("y:mirror", ne) == ((0, 1, 0), (0, 0, 0)) and parse_link("z:mirror", ne) == ((0, 0, 1), (0, 0, 0))
    assert parse_link({"x": "repeat:4"}, ne) == ((2, 0, 0), (4, 0, 0)) and parse_link({"x": ["repeat", 2]}, ne) == ((2, 0, 0), (2, 0, 0))
    assert parse_link([], ne) == parse_link({}, ne) == parse_link("x:none", ne) == ((0, 0, 0), (0, 0, 0))
    assert parse_link("x:repeat:7") == ((2, 0, 0), (7, 0, 0))                     # no element counts: not checked
    for bad in (["x:mirror", "x:extrude"], ["y:repeat:2", "y:repeat:3"],           # an axis twice
                "x:flip", "w:mirror", "mirror", "x", "", "x:", ":mirror", {"x": "rotate"}, {"q": "mirror"},   # unknown
                "x:repeat", "x:repeat:", "x:repeat:1", "x:repeat:0", "x:repeat:-2", "x:repeat:2.5", "x:mirror:2", "z:extrude:1",
                {"x": ("repeat", 1)}, {"x": ("repeat", 2.0)}, {"x": ("repeat",)}, {"x": 3}, {"x": None}, 7, None, [3],
                "x:repeat:5", "y:repeat:4", "z:repeat:2", {"z": ("repeat", 3)}):    # cells that do not divide 12, 6, 5
        with pytest.raises(ValueError):
            parse_link(bad, ne)
    for name in ("Expand", "Fold", "Pick", "counts", "reduced_vec", "set_form", "last_form", "close"):
        assert hasattr(Link, name)
    assert Link.MAXVEC == 12


def test_driver_has_the_field_and_refuses_before_any_device_object():
    """link with passive, a z link on several ranks, and every parse error: ValueErrors of __post_init__ ahead of the grid"""
    import numpy as np
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["link"] is None
    kw = dict(nxyz=(13, 7, 5), nlvls=1)          # 12 x 6 x 4 elements
    with pytest.raises(ValueError, match="passive"):
        TopOpt(link="y:mirror", passive=np.zeros(12 * 6 * 4, dtype=np.uint8), **kw)
    for spec in ("z:mirror", "z:extrude", "z:repeat:2", {"x": "mirror", "z": "extrude"}):
        for rank in (0, 1):
            with pytest.raises(ValueError, match="z link"):
                TopOpt(link=spec, nranks=2, rank=rank, **kw)
    for bad in ("x:flip", ["y:mirror", "y:extrude"], "x:repeat:5", "y:repeat:4", "z:repeat:3", "x:repeat:1", "q:mirror", 3):
        with pytest.raises(ValueError):
            TopOpt(link=bad, **kw)
