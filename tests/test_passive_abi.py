"""CPU-side checks of the passive-region boundary: the header declares the seven calls, the binding knows each
with a matching argument count, the ABI number stays, every argument rule answers before anything touches a device, the label
helper is held to hand-counted cases, and the driver refuses what it cannot run before it makes a grid."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1
CALLS = (("tp_passive_create", 3), ("tp_passive_destroy", 1), ("tp_passive_counts", 4), ("tp_passive_impose", 5),
         ("tp_passive_zero", 3), ("tp_passive_gather", 4), ("tp_passive_scatter", 4))
# the hand-counted box: 4 x 3 x 2 elements of edge 1, centres at 0.5, 1.5, ...; element (i, j, k) has index i + 4 (j + 3 k)
NXYZ, XC = (5, 4, 3), (0.0, 4.0, 0.0, 3.0, 0.0, 2.0)


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_passive_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4
    assert re.search(r"#define\s+TP_PASSIVE_MAXVEC\s+12\b", src) and lib.PASSIVE_MAXVEC == 12


def test_argument_rules_answer_before_any_launch():
    """every rule comes before the first use of the handle, so a zeroed block of host memory can stand in for one; with valid
    arguments the zeroed block reads as no active and no passive element, and the four calls return TP_OK without a launch"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    p = C.cast(C.create_string_buffer(1 << 12), C.c_void_p)
    bufs = [C.create_string_buffer(64) for _ in range(26)]
    vec = lambda k: C.cast(bufs[k], C.c_void_p)
    arr = lambda ks: (C.c_void_p * max(len(ks), 1))(*[None if k is None else vec(k) for k in ks])
    a12, b12, a13 = arr(range(12)), arr(range(12, 24)), arr(range(13))
    out = C.c_void_p()
    assert L.tp_passive_create(None, p, vec(0)) == TP_ERR_ARG
    assert L.tp_passive_create(C.byref(out), None, vec(0)) == TP_ERR_ARG
    assert L.tp_passive_create(C.byref(out), p, None) == TP_ERR_ARG
    assert L.tp_passive_destroy(None) == 0
    assert L.tp_passive_counts(None, None, None, None) == TP_ERR_ARG
    for nvec, x in ((1, None), (0, a12), (-1, a12), (13, a13), (2, arr([0, None])), (12, arr(list(range(11)) + [None]))):
        assert L.tp_passive_impose(p, nvec, x, 0.0, 1.0) == TP_ERR_ARG, (nvec, "impose")
        assert L.tp_passive_zero(p, nvec, x) == TP_ERR_ARG, (nvec, "zero")
        assert L.tp_passive_gather(p, nvec, x, b12) == TP_ERR_ARG and L.tp_passive_gather(p, nvec, b12, x) == TP_ERR_ARG
        assert L.tp_passive_scatter(p, nvec, x, b12) == TP_ERR_ARG and L.tp_passive_scatter(p, nvec, b12, x) == TP_ERR_ARG
    assert L.tp_passive_impose(None, 1, a12, 0.0, 1.0) == TP_ERR_ARG and L.tp_passive_zero(None, 1, a12) == TP_ERR_ARG
    assert L.tp_passive_gather(None, 1, a12, b12) == TP_ERR_ARG and L.tp_passive_scatter(None, 1, a12, b12) == TP_ERR_ARG
    # full[v] == packed[w] for any v, w: the same vector, and one shared between different positions
    shared = arr([12, 13, 1])
    for nvec, one, two in ((1, a12, a12), (3, a12, shared), (12, a12, arr(list(range(12, 23)) + [0]))):
        assert L.tp_passive_gather(p, nvec, one, two) == TP_ERR_ARG and L.tp_passive_gather(p, nvec, two, one) == TP_ERR_ARG
        assert L.tp_passive_scatter(p, nvec, one, two) == TP_ERR_ARG and L.tp_passive_scatter(p, nvec, two, one) == TP_ERR_ARG
    # no element of either kind: nothing to launch
    for nvec in (1, 12):
        assert L.tp_passive_impose(p, nvec, a12, 0.0, 1.0) == 0 and L.tp_passive_zero(p, nvec, a12) == 0
        assert L.tp_passive_gather(p, nvec, a12, b12) == 0 and L.tp_passive_scatter(p, nvec, b12, a12) == 0
    cnt = [C.c_long(7) for _ in range(3)]
    assert L.tp_passive_counts(p, *[C.byref(c) for c in cnt]) == 0 and [c.value for c in cnt] == [0, 0, 0]


def test_labels_of_hand_counted_shapes():
    from topopt_in_petsc_amd.api import passive_labels
    where = lambda shapes, v: sorted(np.nonzero(passive_labels(NXYZ, XC, shapes) == v)[0].tolist())
    lab = passive_labels(NXYZ, XC, [])
    assert lab.dtype == np.uint8 and lab.shape == (24,) and not lab.any()
    # a box with the centre (1.5, 1.5, 0.5) of element (1, 1, 0) on its lower x face, its upper y face and both z faces, and no other
    box = ("solid", "box", (1.5, 2.4, 0.6, 1.5, 0.5, 0.5))
    assert where([box], 2) == [5] and where([box], 1) == []
    # a sphere about the centre of the face between elements (1, 1, 0) and (2, 1, 0): both centres lie h / 2 = 0.5 away
    assert where([("void", "sphere", (2.0, 1.5, 0.5, 0.4))], 1) == []
    assert where([("void", "sphere", (2.0, 1.5, 0.5, 0.6))], 1) == [5, 6]
    assert where([("void", "sphere", (2.0, 1.5, 0.5, 0.5))], 1) == [5, 6]            # on the boundary
    # cylinders: along z through the centres of the column (0, 0, .); along x through the row (., 1, 1)
    assert where([("solid", "cylinder", (2, 0.5, 0.5, 0.1))], 2) == [0, 12]
    assert where([("solid", "cylinder", ("z", 0.5, 0.5, 0.1))], 2) == [0, 12]
    assert where([("void", "cylinder", ("x", 1.5, 1.5, 0.1))], 1) == [16, 17, 18, 19]
    assert where([("void", "cylinder", (1, 2.5, 0.5, 0.1))], 1) == [2, 6, 10]
    # later shapes override earlier ones
    everything, ball = ("solid", "box", (0, 4, 0, 3, 0, 2)), ("void", "sphere", (2.0, 1.5, 0.5, 0.6))
    assert where([everything, ball], 1) == [5, 6] and len(where([everything, ball], 2)) == 22
    assert where([ball, everything], 1) == [] and len(where([ball, everything], 2)) == 24
    # physical coordinates: the same box moved and scaled
    moved = passive_labels(NXYZ, (10.0, 12.0, -3.0, 0.0, 1.0, 2.0), [("solid", "box", (10.75, 11.2, -2.4, -1.5, 1.25, 1.25))])
    assert sorted(np.nonzero(moved == 2)[0].tolist()) == [5]
    for bad in ([("solid", "box", (0, 1, 0, 1))], [("full", "box", (0, 1, 0, 1, 0, 1))], [("void", "cone", (0, 1, 0, 1))],
                [("void", "cylinder", (3, 0.5, 0.5, 0.1))], ["solid:box"]):
        with pytest.raises(ValueError):
            passive_labels(NXYZ, XC, bad)


def _unbuilt(**kw):
    """a TopOpt with its defaults and no __post_init__: the label check alone, which is host arithmetic"""
    from topopt_in_petsc_amd.driver import TopOpt
    t = TopOpt.__new__(TopOpt)
    for f in dataclasses.fields(TopOpt):
        setattr(t, f.name, f.default if f.default is not dataclasses.MISSING else f.default_factory())
    for k, v in dict(dict(nxyz=NXYZ, xc=XC), **kw).items():
        setattr(t, k, v)
    return t


def test_driver_has_the_field_and_refuses_what_it_cannot_run_before_it_makes_a_grid():
    from topopt_in_petsc_amd.api import Passive, passive_labels
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["passive"] is None
    assert all(hasattr(Passive, name) for name in ("Impose", "Zero", "Gather", "Scatter", "counts", "close"))
    lab = np.zeros(24, dtype=np.uint8)
    lab[[0, 1, 2]], lab[[20, 21]] = 1, 2
    # what passes: 19 active elements start at (0.3 * 24 - 2) / 19, the volume constraint at equality
    t = _unbuilt(passive=lab, volfrac=0.3)
    got = t._check_passive()
    assert got.dtype == np.uint8 and np.array_equal(got, lab) and t.n_active == 19 and t._x0 == (0.3 * 24 - 2) / 19
    assert abs((t._x0 * 19 + 2) / 24 - 0.3) < 1e-15
    t = _unbuilt(passive=[("void", "sphere", (2.0, 1.5, 0.5, 0.6))], volfrac=0.3)
    assert np.array_equal(t._check_passive(), passive_labels(NXYZ, XC, [("void", "sphere", (2.0, 1.5, 0.5, 0.6))])) and t.n_active == 22
    t = _unbuilt(passive=np.zeros(24, dtype=np.uint8))
    t._check_passive()
    assert t._x0 == t.volfrac and t.n_active == 24
    # every refusal is a ValueError of __post_init__, raised before Grid(...): no device needed
    rank0_passive = np.concatenate([np.ones(12, dtype=np.uint8), np.zeros(12, dtype=np.uint8)])
    three_solid = np.array([2] * 3 + [0] * 21, dtype=np.uint8)      # 3 / 24 = 0.125 >= volfrac = 0.12
    twenty_void = np.array([1] * 20 + [0] * 4, dtype=np.uint8)      # x0 = 0.5 * 24 / 4 = 3 > Xmax
    cases = (dict(passive=np.zeros(23, dtype=np.uint8)), dict(passive=np.zeros((4, 6), dtype=np.uint8)),
             dict(passive=np.array([0] * 23 + [3])), dict(passive=np.array([0] * 23 + [-1])),
             dict(passive=np.ones(24, dtype=np.uint8)), dict(passive=np.full(24, 2, dtype=np.uint8), volfrac=1.0),
             dict(passive=[("void", "box", XC)]),
             dict(passive=rank0_passive, nranks=2, rank=0), dict(passive=rank0_passive, nranks=2, rank=1),
             dict(passive=rank0_passive[::-1].copy(), nranks=2, rank=0),
             dict(passive=lab, length_scale="both"), dict(passive=np.zeros(24, dtype=np.uint8), length_scale="solid"),
             dict(passive=three_solid, volfrac=0.12), dict(passive=three_solid, volfrac=0.125),
             dict(passive=twenty_void, volfrac=0.5),
             dict(passive=np.array([2] * 2 + [1] * 2 + [0] * 20, dtype=np.uint8), volfrac=0.3, Xmin=0.35))
    for kw in cases:
        with pytest.raises(ValueError):
            TopOpt(**dict(dict(nxyz=NXYZ, xc=XC, nlvls=1), **kw))
        with pytest.raises(ValueError):
            _unbuilt(**kw)._check_passive()
