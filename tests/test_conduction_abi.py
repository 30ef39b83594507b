"""CPU-side checks of the heat-conduction boundary: the header declares every call, the binding knows each with
a matching argument count, the ABI number stays, every argument rule answers before anything touches a device, and the driver
has `physics` and refuses what it cannot run with "heat" before it makes a grid."""
import ctypes as C
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG, TP_ERR_STATE = 1, 2
# name, arguments, C return type
CALLS = (("tp_conduction_create", 3, "int"), ("tp_conduction_destroy", 1, "int"), ("tp_conduction_get_ke", 2, "int"),
         ("tp_conduction_set_bc", 2, "int"), ("tp_conduction_assemble", 5, "int"), ("tp_conduction_apply", 3, "int"), ("tp_conduction_apply_dot", 4, "int"),
         ("tp_conduction_solve", 8, "int"), ("tp_conduction_response", 15, "int"), ("tp_conduction_set_tolerances", 5, "int"),
         ("tp_conduction_level_count", 1, "int"), ("tp_conduction_level_nodes", 2, "long"), ("tp_conduction_level_lambda", 2, "double"),
         ("tp_conduction_level_lambda_min", 2, "double"), ("tp_conduction_level_apply", 4, "int"), ("tp_conduction_level_diag", 3, "int"),
         ("tp_conduction_smooth", 6, "int"), ("tp_conduction_level_residual", 5, "int"), ("tp_conduction_restrict", 4, "int"),
         ("tp_conduction_prolong_add", 4, "int"), ("tp_conduction_last_op_form", 2, "int"), ("tp_conduction_last_stats", 4, "int"))
CTYPE = {"int": C.c_int, "long": C.c_long, "double": C.c_double}


def _declared_args(src, name, ret):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;]*?)\)\s*;" % (ret, name), src, re.S)
    assert m, "include/topopt_amd.h does not declare %s %s" % (ret, name)
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_conduction_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs, ret in CALLS:
        declared = _declared_args(src, name, ret)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is CTYPE[ret] and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4 and lib.load_library().tp_abi_version() == 4
    from topopt_in_petsc_amd import api
    for name in ("KT", "SetBC", "SetUpLoadAndBC", "AssembleConductivityMatrix", "MatMult", "MatMultDot", "KSPSolve", "SolveState", "Response",
                 "ComputeObjectiveConstraintsSensitivities", "SetTolerances", "level_count", "level_nodes", "level_lambda",
                 "level_lambda_min", "level_vec", "level_apply", "level_dinv", "smooth", "restrict", "prolong_add", "last_op_form",
                 "pop_stats", "close"):
        assert hasattr(api.HeatConduction, name), name


def test_argument_rules_answer_before_any_launch():
    """every rule comes before the first use of the handle or the grid, so a zeroed block of host memory can stand in for one; with
    valid arguments the zeroed block reads as "no supports set, nothing assembled" and the calls answer TP_ERR_STATE"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    p = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    bufs = [C.create_string_buffer(64) for _ in range(6)]
    v = lambda k: C.cast(bufs[k], C.c_void_p)
    out = C.c_void_p()
    o = lib.SolverOpts()
    L.tp_solver_default_opts(C.byref(o))
    nan, inf = float("nan"), float("inf")
    # create / destroy / get_ke / set_bc
    assert L.tp_conduction_create(None, p, C.byref(o)) == TP_ERR_ARG
    assert L.tp_conduction_create(C.byref(out), None, C.byref(o)) == TP_ERR_ARG
    assert L.tp_conduction_create(C.byref(out), p, None) == TP_ERR_ARG
    o.nlvls = 0
    assert L.tp_conduction_create(C.byref(out), p, C.byref(o)) == TP_ERR_ARG
    o.nlvls, o.ksp_mode = 1, 1          # (a zeroed grid has 0 elements every way: any level count divides them)
    assert L.tp_conduction_create(C.byref(out), p, C.byref(o)) == TP_ERR_ARG
    assert L.tp_conduction_destroy(None) == 0
    assert L.tp_conduction_get_ke(None, v(0)) == TP_ERR_ARG and L.tp_conduction_get_ke(p, None) == TP_ERR_ARG
    assert L.tp_conduction_set_bc(None, v(0)) == TP_ERR_ARG and L.tp_conduction_set_bc(p, None) == TP_ERR_ARG
    # assemble: NULL, kmin > 0, kmax > kmin, penal >= 1, all finite
    good = (1e-3, 1.0, 3.0)
    bad = ((0.0, 1.0, 3.0), (-1e-3, 1.0, 3.0), (1.0, 1.0, 3.0), (1.0, 0.5, 3.0), (1e-3, 1.0, 0.5), (nan, 1.0, 3.0), (1e-3, nan, 3.0),
           (1e-3, 1.0, nan), (1e-3, inf, 3.0), (1e-3, 1.0, inf))
    assert L.tp_conduction_assemble(None, v(0), *good) == TP_ERR_ARG and L.tp_conduction_assemble(p, None, *good) == TP_ERR_ARG
    for b in bad:
        assert L.tp_conduction_assemble(p, v(0), *b) == TP_ERR_ARG, b
    assert L.tp_conduction_assemble(p, v(0), *good) == TP_ERR_STATE
    # apply / solve
    assert L.tp_conduction_apply(None, v(0), v(1)) == TP_ERR_ARG and L.tp_conduction_apply(p, None, v(1)) == TP_ERR_ARG
    assert L.tp_conduction_apply(p, v(0), None) == TP_ERR_ARG and L.tp_conduction_apply(p, v(0), v(1)) == TP_ERR_STATE
    dot = C.c_double()
    assert L.tp_conduction_apply_dot(None, v(0), v(1), C.byref(dot)) == TP_ERR_ARG and L.tp_conduction_apply_dot(p, None, v(1), None) == TP_ERR_ARG
    assert L.tp_conduction_apply_dot(p, v(0), None, None) == TP_ERR_ARG and L.tp_conduction_apply_dot(p, v(0), v(1), None) == TP_ERR_STATE
    its, rn, bn = C.c_int(), C.c_double(), C.c_double()
    tail = (C.byref(its), C.byref(rn), C.byref(bn))
    assert L.tp_conduction_solve(None, v(0), v(1), *tail, None, 0) == TP_ERR_ARG
    assert L.tp_conduction_solve(p, None, v(1), *tail, None, 0) == TP_ERR_ARG
    assert L.tp_conduction_solve(p, v(0), None, *tail, None, 0) == TP_ERR_ARG
    assert L.tp_conduction_solve(p, v(0), v(1), *tail, None, 4) == TP_ERR_ARG and L.tp_conduction_solve(p, v(0), v(1), *tail, v(2), -1) == TP_ERR_ARG
    assert L.tp_conduction_solve(p, v(0), v(1), *tail, None, 0) == TP_ERR_STATE
    # response: 1 <= ncase <= TP_MAX_CASES, every T[l], the material rule, finite weights and volfrac
    arr = lambda ks: (C.c_void_p * max(len(ks), 1))(*[None if k is None else v(k) for k in ks])
    w3 = (C.c_double * 8)(0.75, -0.5, 0.0)
    fx = C.c_double(7.0)
    resp = lambda c, n, T, V, w, x, mat, vf: L.tp_conduction_response(c, n, T, V, w, x, mat[0], mat[1], mat[2], vf, None, C.byref(fx), None, v(4), v(5))
    T3 = arr([0, 1, 2])
    assert resp(None, 3, T3, None, w3, v(3), good, 0.3) == TP_ERR_ARG and resp(p, 3, None, None, w3, v(3), good, 0.3) == TP_ERR_ARG
    assert resp(p, 3, T3, None, w3, None, good, 0.3) == TP_ERR_ARG
    for n, T in ((0, T3), (-1, T3), (lib.MAX_CASES + 1, arr([0] * 9)), (3, arr([0, None, 2])), (1, arr([None]))):
        assert resp(p, n, T, None, None, v(3), good, 0.3) == TP_ERR_ARG, n
    for b in bad:
        assert resp(p, 3, T3, None, w3, v(3), b, 0.3) == TP_ERR_ARG, b
    assert resp(p, 3, T3, None, (C.c_double * 8)(0.75, nan, 0.0), v(3), good, 0.3) == TP_ERR_ARG
    assert resp(p, 3, T3, None, w3, v(3), good, nan) == TP_ERR_ARG
    assert resp(p, 3, T3, arr([None, 1, None]), w3, v(3), good, 0.3) == TP_ERR_STATE and fx.value == 7.0
    assert L.tp_conduction_set_tolerances(None, 1e-8, -1.0, -1.0, -1) == TP_ERR_ARG
    # the level calls
    assert L.tp_conduction_level_count(None) == -TP_ERR_ARG and L.tp_conduction_level_count(p) == 0
    assert L.tp_conduction_level_nodes(None, 0) == -TP_ERR_ARG and L.tp_conduction_level_nodes(p, 0) == -TP_ERR_ARG
    assert L.tp_conduction_level_lambda(None, 0) != L.tp_conduction_level_lambda(None, 0)            # NaN
    assert L.tp_conduction_level_lambda_min(p, 3) != L.tp_conduction_level_lambda_min(p, 3)
    for fn, extra in ((L.tp_conduction_level_apply, ()), (L.tp_conduction_restrict, ()), (L.tp_conduction_prolong_add, ())):
        assert fn(None, 0, v(0), v(1)) == TP_ERR_ARG and fn(p, 0, None, v(1)) == TP_ERR_ARG and fn(p, 0, v(0), None) == TP_ERR_ARG
    assert L.tp_conduction_level_apply(p, 0, v(0), v(1)) == TP_ERR_STATE
    assert L.tp_conduction_restrict(p, 0, v(0), v(1)) == TP_ERR_ARG and L.tp_conduction_prolong_add(p, 0, v(0), v(1)) == TP_ERR_ARG   # no such level
    assert L.tp_conduction_level_diag(None, 0, v(0)) == TP_ERR_ARG and L.tp_conduction_level_diag(p, 0, None) == TP_ERR_ARG
    assert L.tp_conduction_level_diag(p, 0, v(0)) == TP_ERR_STATE
    assert L.tp_conduction_smooth(None, 0, v(0), v(1), 1, 1) == TP_ERR_ARG and L.tp_conduction_smooth(p, 0, None, v(1), 1, 1) == TP_ERR_ARG
    assert L.tp_conduction_smooth(p, 0, v(0), None, 1, 1) == TP_ERR_ARG and L.tp_conduction_smooth(p, 0, v(0), v(1), -1, 1) == TP_ERR_ARG
    assert L.tp_conduction_smooth(p, 0, v(0), v(1), 1, 1) == TP_ERR_STATE
    assert L.tp_conduction_level_residual(None, 0, v(0), v(1), v(2)) == TP_ERR_ARG and L.tp_conduction_level_residual(p, 0, v(0), v(1), None) == TP_ERR_ARG
    assert L.tp_conduction_level_residual(p, 0, v(0), v(1), v(2)) == TP_ERR_STATE
    f4 = (C.c_int * 4)(9, 9, 9, 9)
    assert L.tp_conduction_last_op_form(None, f4) == TP_ERR_ARG and L.tp_conduction_last_op_form(p, None) == TP_ERR_ARG
    assert L.tp_conduction_last_op_form(p, f4) == 0 and list(f4) == [0, 0, 0, 0]
    assert L.tp_conduction_last_stats(None, None, None, None) == TP_ERR_ARG and L.tp_conduction_last_stats(p, None, None, None) == TP_ERR_ARG


def _unbuilt(**kw):
    """a TopOpt with its defaults and no __post_init__"""
    from topopt_in_petsc_amd.driver import TopOpt
    t = TopOpt.__new__(TopOpt)
    for f in dataclasses.fields(TopOpt):
        setattr(t, f.name, f.default if f.default is not dataclasses.MISSING else f.default_factory())
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_driver_has_physics_and_refuses_what_heat_cannot_run_before_it_makes_a_grid(monkeypatch):
    from topopt_in_petsc_amd import driver
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["physics"] == "elasticity" and f["kmin"] == 1e-3 and f["kmax"] == 1.0 and f["penal"] == 3.0

    def no_grid(*a, **k):
        raise AssertionError("a refused combination reached Grid(...)")
    monkeypatch.setattr(driver, "Grid", no_grid)
    base = dict(nxyz=(5, 4, 3), xc=(0.0, 4.0, 0.0, 3.0, 0.0, 2.0), nlvls=1, physics="heat")
    cases = (dict(loadcases=[("top", 0.5)]), dict(stress_limit=1.0), dict(body_force=(0.0, 0.0, -1.0)), dict(frequency_limit=10.0),
             dict(robust=(0.7, 0.5, 0.3), projectionFilter=True), dict(overhang="+z"), dict(local_volume=0.6, local_volume_R=0.3),
             dict(length_scale="both"), dict(kmin=0.0), dict(kmin=1.0, kmax=1.0), dict(kmax=float("inf")), dict(penal=0.5),
             dict(physics="thermal"))
    for kw in cases:
        with pytest.raises(ValueError):
            TopOpt(**dict(base, **kw))
    for kw in cases[:-1]:
        with pytest.raises(ValueError):
            _unbuilt(**dict(dict(physics="heat"), **kw))._check_heat()
    # what passes the check goes on to the grid: plain heat, and heat with passive regions
    _unbuilt(physics="heat")._check_heat()
    for kw in (dict(), dict(passive=[("void", "sphere", (2.0, 1.5, 0.5, 0.6))], volfrac=0.3)):
        with pytest.raises(AssertionError, match="reached Grid"):
            TopOpt(**dict(base, **kw))
