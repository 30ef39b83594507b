"""CPU-side checks of the robust-design boundary: the header declares the two calls, the binding knows each with a
matching argument count, the ABI number stays, every argument rule answers before anything touches a device, the driver has its
three fields and refuses what it cannot run before it makes a grid, and the schedule of V_d* is held to hand arithmetic."""
import ctypes as C
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1
CALLS = (("tp_robust_project", 8), ("tp_robust_chain", 7))


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_robust_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4
    assert re.search(r"#define\s+TP_ROBUST_MAXPROJ\s+3\b", src) and lib.ROBUST_MAXPROJ == 3
    assert re.search(r"#define\s+TP_ROBUST_MAXROWS\s+8\b", src) and lib.ROBUST_MAXROWS == 8


def test_argument_rules_answer_before_the_grid_is_touched():
    """every rule comes before the first use of the grid, so a zeroed block of host memory can stand in for one; the zeroed block
    that stands in for a passive handle names no grid, so it belongs to another one"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    g = C.cast(C.create_string_buffer(1 << 14), C.c_void_p)
    p = C.cast(C.create_string_buffer(1 << 12), C.c_void_p)
    bufs = [C.create_string_buffer(64) for _ in range(12)]
    vec = lambda k: C.cast(bufs[k], C.c_void_p)
    arr = lambda ks: (C.c_void_p * max(len(ks), 1))(*[None if k is None else vec(k) for k in ks])
    dbl = lambda vs: (C.c_double * max(len(vs), 1))(*vs)
    xt, inf, nan = vec(11), float("inf"), float("nan")
    e3, o3, sums = dbl([0.7, 0.5, 0.3]), arr([0, 1, 2]), dbl([0.0] * 3)
    e8, r8 = dbl([0.7, 0.5, 0.3, 0.7, 0.5, 0.3, 0.7, 0.5]), arr(range(8))

    def project(grid=g, x=xt, beta=4.0, nproj=3, eta=e3, out=o3, pas=None, s=sums):
        return L.tp_robust_project(grid, x, beta, nproj, eta, out, pas, s)

    def chain(grid=g, x=xt, beta=4.0, nrows=8, rows=r8, eta=e8, pas=None):
        return L.tp_robust_chain(grid, x, beta, nrows, rows, eta, pas)

    # NULL grid, field, array, vector
    for call in (project, chain):
        assert call(grid=None) == TP_ERR_ARG and call(x=None) == TP_ERR_ARG and call(eta=None) == TP_ERR_ARG
    assert project(out=None) == TP_ERR_ARG and chain(rows=None) == TP_ERR_ARG
    assert project(out=arr([0, None, 2])) == TP_ERR_ARG and project(nproj=1, out=arr([None])) == TP_ERR_ARG
    assert chain(rows=arr([0, 1, 2, 3, 4, 5, 6, None])) == TP_ERR_ARG and chain(nrows=1, rows=arr([None])) == TP_ERR_ARG
    # the counts
    for nproj in (0, -1, 4):
        assert project(nproj=nproj, eta=dbl([0.5] * 4), out=arr(range(4))) == TP_ERR_ARG, nproj
    for nrows in (0, -1, 9):
        assert chain(nrows=nrows, rows=arr(range(9)), eta=dbl([0.5] * 9)) == TP_ERR_ARG, nrows
    # more than three distinct thresholds over the rows
    assert chain(nrows=4, eta=dbl([0.7, 0.5, 0.3, 0.1])) == TP_ERR_ARG
    assert chain(nrows=8, eta=dbl([0.7, 0.5, 0.3, 0.7, 0.5, 0.3, 0.7, 0.5000001])) == TP_ERR_ARG
    # beta
    for beta in (0.0, -4.0, inf, -inf, nan):
        assert project(beta=beta) == TP_ERR_ARG and chain(beta=beta) == TP_ERR_ARG, beta
    # a threshold outside [0, 1]
    for bad in (-1e-300, 1.0000000000000002, inf, nan):
        assert project(eta=dbl([0.7, bad, 0.3])) == TP_ERR_ARG and project(nproj=1, eta=dbl([bad])) == TP_ERR_ARG, bad
        assert chain(eta=dbl([0.7] * 7 + [bad])) == TP_ERR_ARG and chain(nrows=1, eta=dbl([bad])) == TP_ERR_ARG, bad
    # an output that is xTilde, or another output
    assert project(out=arr([0, 11, 2])) == TP_ERR_ARG and project(nproj=1, out=arr([11])) == TP_ERR_ARG
    assert project(out=arr([0, 1, 0])) == TP_ERR_ARG and project(nproj=2, out=arr([1, 1])) == TP_ERR_ARG
    assert chain(rows=arr([0, 1, 2, 3, 4, 5, 6, 11])) == TP_ERR_ARG and chain(nrows=1, rows=arr([11])) == TP_ERR_ARG
    assert chain(rows=arr([0, 1, 2, 3, 4, 5, 6, 0])) == TP_ERR_ARG and chain(nrows=2, rows=arr([3, 3])) == TP_ERR_ARG
    # a passive handle of another grid
    assert project(pas=p) == TP_ERR_ARG and project(pas=p, s=None) == TP_ERR_ARG and chain(pas=p) == TP_ERR_ARG
    # the boundaries themselves pass every rule: eta 0 and 1, one field, one row -- they fail only at the foreign handle, which is
    # the last rule
    assert project(nproj=2, eta=dbl([1.0, 0.0]), out=arr([0, 1]), pas=p) == TP_ERR_ARG


def _fields():
    from topopt_in_petsc_amd.driver import TopOpt
    return {d.name: d.default for d in dataclasses.fields(TopOpt)}


def test_driver_has_the_fields_and_refuses_what_it_cannot_run_before_it_makes_a_grid(monkeypatch):
    from topopt_in_petsc_amd import api, driver
    from topopt_in_petsc_amd.driver import TopOpt
    f = _fields()
    assert f["robust"] is None and f["robust_volume_every"] == 20 and f["robust_report"] == 0
    assert all(hasattr(api.Robust, name) for name in ("Project", "Chain")) and api.Robust.MAXPROJ == 3 and api.Robust.MAXROWS == 8

    def no_grid(*a, **kw):
        raise AssertionError("a grid was made")
    monkeypatch.setattr(driver, "Grid", no_grid)
    ok = dict(nxyz=(5, 4, 3), xc=(0.0, 4.0, 0.0, 3.0, 0.0, 2.0), nlvls=1, robust=(0.7, 0.5, 0.3), projectionFilter=True)
    cases = (dict(robust=(0.5, 0.5, 0.5)), dict(robust=(0.3, 0.5, 0.7)), dict(robust=(0.7, 0.5, 0.5)), dict(robust=(0.7, 0.7, 0.3)),
             dict(robust=(1.0, 0.5, 0.3)), dict(robust=(0.7, 0.5, 0.0)), dict(robust=(1.2, 0.5, 0.3)), dict(robust=(0.7, 0.5, -0.1)),
             dict(robust=(0.7, 0.5)), dict(robust=(0.7, 0.5, 0.3, 0.1)), dict(robust=(0.7, float("nan"), 0.3)), dict(robust=0.5),
             dict(projectionFilter=False), dict(filter=0), dict(eta=0.4), dict(eta=0.7),
             dict(robust_volume_every=0), dict(robust_volume_every=-3), dict(robust_volume_every=2.5),
             dict(body_force=(0.0, 0.0, -1.0)), dict(stress_limit=1.0), dict(local_volume=0.6, local_volume_R=0.3),
             dict(frequency_limit=1.0), dict(overhang="+z"), dict(length_scale="both"))
    for kw in cases:
        with pytest.raises(ValueError):
            TopOpt(**dict(ok, **kw))
    # what passes every refusal reaches the grid: the defaults, eta at eta_n, filters 1 and 2, load cases, passive shapes, kkt
    for kw in (dict(), dict(eta=0.5), dict(filter=2), dict(loadcases=[("top", 0.5)]), dict(kkt=True, robust_volume_every=1, robust_report=2),
               dict(passive=[("void", "sphere", (2.0, 1.5, 0.5, 0.6))], volfrac=0.3), dict(mma_robust_asymptotes=1)):
        with pytest.raises(AssertionError, match="a grid was made"):
            TopOpt(**dict(ok, **kw))


def test_dilated_volume_target_and_its_schedule():
    """V_d* = volfrac S_d / S_n: with volfrac = 0.3, S_d = 12, S_n = 8 the dilated design holds 1.5 times the nominal one's material,
    so it is held to 0.45; the updates fall at iterations 1, 20, 40 for every = 20"""
    from topopt_in_petsc_amd.driver import robust_volume_due, robust_volume_target
    assert robust_volume_target(0.3, 12.0, 8.0) == pytest.approx(0.45, rel=1e-15)
    assert robust_volume_target(0.3, 8.0, 8.0) == 0.3
    assert [i for i in range(1, 50) if robust_volume_due(i, 20)] == [1, 20, 40]
    assert [i for i in range(1, 8) if robust_volume_due(i, 2)] == [1, 2, 4, 6]
    assert [i for i in range(1, 5) if robust_volume_due(i, 1)] == [1, 2, 3, 4]
