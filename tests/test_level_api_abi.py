"""CPU-side checks of the level-by-level multigrid calls: one contract for tp_elasticity_*, tp_conduction_* and
tp_pdefilter_*, stated once in include/topopt_amd.h and written once in csrc/mg_levels.h.  The method of test_conduction_abi.py: a
zeroed block of host memory stands in for a handle, every rule answers before the handle's contents are used, nothing is
launched.  A zeroed elasticity or conduction handle reads as "nothing assembled, no levels"; a zeroed filter is of type 0, not 2."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG, TP_ERR_STATE = 1, 2
TP_MAX_LEVELS = 10
# suffix, arguments with the handle, C return type
LEVEL_CALLS = (("level_count", 1, "int"), ("level_nodes", 2, "long"), ("level_lambda", 2, "double"), ("level_lambda_min", 2, "double"),
               ("level_apply", 4, "int"), ("level_diag", 3, "int"), ("smooth", 6, "int"), ("restrict", 4, "int"),
               ("prolong_add", 4, "int"), ("last_op_form", 2, "int"))
WITH_STATS = (("level_residual", 5, "int"), ("last_stats", 4, "int"))
# prefix -> (calls, what a zeroed handle answers where an assembly is needed)
FAMILIES = {"tp_elasticity": (LEVEL_CALLS + WITH_STATS, TP_ERR_STATE), "tp_conduction": (LEVEL_CALLS + WITH_STATS, TP_ERR_STATE),
            "tp_pdefilter": (LEVEL_CALLS, TP_ERR_ARG)}
CTYPE = {"int": C.c_int, "long": C.c_long, "double": C.c_double}


def _declared_args(src, name, ret):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;]*?)\)\s*;" % (ret, name), src, re.S)
    assert m, "include/topopt_amd.h does not declare %s %s" % (ret, name)
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_header_declares_the_level_calls_and_the_binding_has_them(prefix):
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    assert re.search(r"#define\s+TP_MAX_LEVELS\s+%d\b" % TP_MAX_LEVELS, src)
    for suffix, nargs, ret in FAMILIES[prefix][0]:
        name = "%s_%s" % (prefix, suffix)
        declared = _declared_args(src, name, ret)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is CTYPE[ret] and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    if prefix == "tp_pdefilter":   # the filter's family stays without these two, in the library and in the class
        from topopt_in_petsc_amd import api
        for suffix, _, _ in WITH_STATS:
            assert "%s_%s" % (prefix, suffix) not in lib.SYMBOLS
        assert not hasattr(api.Filter, "level_residual") and not hasattr(api.Filter, "pop_stats")
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4


@pytest.mark.parametrize("prefix", sorted(FAMILIES))
def test_one_contract_answers_before_any_launch(prefix):
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    fn = lambda suffix: getattr(L, "%s_%s" % (prefix, suffix))
    unassembled = FAMILIES[prefix][1]
    p = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    bufs = [C.create_string_buffer(64) for _ in range(3)]
    v = lambda k: C.cast(bufs[k], C.c_void_p)
    isnan = lambda x: x != x
    # the four that answer a value: a NULL handle or a missing level, and nothing else
    assert fn("level_count")(None) == -TP_ERR_ARG
    assert fn("level_count")(p) == (-TP_ERR_ARG if prefix == "tp_pdefilter" else 0)
    assert fn("level_nodes")(None, 0) == -TP_ERR_ARG and fn("level_nodes")(p, 0) == -TP_ERR_ARG and fn("level_nodes")(p, -1) == -TP_ERR_ARG
    for name in ("level_lambda", "level_lambda_min"):
        assert isnan(fn(name)(None, 0)) and isnan(fn(name)(p, 0)) and isnan(fn(name)(p, 3)) and isnan(fn(name)(p, -1))
    # two vectors: NULL handle, each NULL vector; then the state (apply) or the missing level l + 1 (the transfers)
    for name in ("level_apply", "restrict", "prolong_add"):
        assert fn(name)(None, 0, v(0), v(1)) == TP_ERR_ARG and fn(name)(p, 0, None, v(1)) == TP_ERR_ARG and fn(name)(p, 0, v(0), None) == TP_ERR_ARG, name
    assert fn("level_apply")(p, 0, v(0), v(1)) == unassembled
    assert fn("restrict")(p, 0, v(0), v(1)) == TP_ERR_ARG and fn("prolong_add")(p, 0, v(0), v(1)) == TP_ERR_ARG
    assert fn("restrict")(p, -1, v(0), v(1)) == TP_ERR_ARG and fn("prolong_add")(p, -1, v(0), v(1)) == TP_ERR_ARG
    assert fn("level_diag")(None, 0, v(0)) == TP_ERR_ARG and fn("level_diag")(p, 0, None) == TP_ERR_ARG
    assert fn("level_diag")(p, 0, v(0)) == unassembled
    # smooth: k < 0 is an argument error, whatever the state; k == 0 is legal but for the filter
    assert fn("smooth")(None, 0, v(0), v(1), 1, 1) == TP_ERR_ARG and fn("smooth")(p, 0, None, v(1), 1, 1) == TP_ERR_ARG
    assert fn("smooth")(p, 0, v(0), None, 1, 1) == TP_ERR_ARG and fn("smooth")(p, 0, v(0), v(1), -1, 1) == TP_ERR_ARG
    assert fn("smooth")(p, 0, v(0), v(1), 1, 1) == unassembled
    assert fn("smooth")(p, 0, v(0), v(1), 0, 0) == unassembled     # (the filter: TP_ERR_ARG, as for every k it refuses)
    f4 = (C.c_int * 4)(9, 9, 9, 9)
    assert fn("last_op_form")(None, f4) == TP_ERR_ARG and fn("last_op_form")(p, None) == TP_ERR_ARG
    if prefix == "tp_pdefilter":
        assert fn("last_op_form")(p, f4) == TP_ERR_ARG and list(f4) == [9, 9, 9, 9]
    else:
        assert fn("last_op_form")(p, f4) == 0 and list(f4) == [0, 0, 0, 0]
        assert fn("level_residual")(None, 0, v(0), v(1), v(2)) == TP_ERR_ARG
        for k in range(3):
            assert fn("level_residual")(p, 0, *[None if j == k else v(j) for j in range(3)]) == TP_ERR_ARG, k
        assert fn("level_residual")(p, 0, v(0), v(1), v(2)) == TP_ERR_STATE
        assert fn("last_stats")(None, None, None, None) == TP_ERR_ARG and fn("last_stats")(p, None, None, None) == TP_ERR_ARG


def test_elasticity_only_calls_share_the_guard():
    """NULL handle or vector: TP_ERR_ARG; then TP_ERR_STATE before the first assembly -- nothing of the zeroed handle is used"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    p = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    bufs = [C.create_string_buffer(64) for _ in range(2)]
    v = lambda k: C.cast(bufs[k], C.c_void_p)
    dot, done = C.c_double(), C.c_int()
    calls = ((L.tp_elasticity_precond, ()), (L.tp_elasticity_level_pc, (0, 1)), (L.tp_elasticity_level_gs, (0, 0)))
    for fn, head in calls:
        assert fn(None, *head, v(0), v(1)) == TP_ERR_ARG and fn(p, *head, None, v(1)) == TP_ERR_ARG and fn(p, *head, v(0), None) == TP_ERR_ARG
        assert fn(p, *head, v(0), v(1)) == TP_ERR_STATE
    gm = lambda h, b, x: L.tp_elasticity_level_gmres(h, 0, 0, 4, 4, -1.0, b, x, 1, C.byref(done))
    assert gm(None, v(0), v(1)) == TP_ERR_ARG and gm(p, None, v(1)) == TP_ERR_ARG and gm(p, v(0), None) == TP_ERR_ARG
    assert gm(p, v(0), v(1)) == TP_ERR_STATE
    sd = lambda h, b, x, k, zg, d: L.tp_elasticity_smooth_dot(h, 0, b, x, k, zg, d)
    assert sd(None, v(0), v(1), 2, 0, C.byref(dot)) == TP_ERR_ARG and sd(p, None, v(1), 2, 0, C.byref(dot)) == TP_ERR_ARG
    assert sd(p, v(0), None, 2, 0, C.byref(dot)) == TP_ERR_ARG and sd(p, v(0), v(1), 2, 0, None) == TP_ERR_ARG
    assert sd(p, v(0), v(1), 0, 0, C.byref(dot)) == TP_ERR_ARG and sd(p, v(0), v(1), 1, 1, C.byref(dot)) == TP_ERR_ARG
    assert sd(p, v(0), v(1), 2, 1, C.byref(dot)) == TP_ERR_STATE
    assert L.tp_elasticity_coarse_direct_active(None) == 0 and L.tp_elasticity_coarse_direct_active(p) == 0


@pytest.mark.parametrize("nlvls", (0, -3, TP_MAX_LEVELS + 1))
def test_filter_create_refuses_a_level_count_out_of_range(nlvls):
    """the options are checked against the grid before either is used: a zeroed block stands in for the grid (0 elements every
    way, which any level count divides)"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    g = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    out = C.c_void_p()
    o = lib.SolverOpts()
    L.tp_solver_default_opts(C.byref(o))
    o.nlvls = nlvls
    assert L.tp_filter_create(C.byref(out), g, 2, 1.5, C.byref(o)) == TP_ERR_ARG and not out.value
    for create in (L.tp_elasticity_create, L.tp_conduction_create):
        assert create(C.byref(out), g, C.byref(o)) == TP_ERR_ARG and not out.value
    o.nlvls, o.ksp_mode = 1, 2
    assert L.tp_filter_create(C.byref(out), g, 2, 1.5, C.byref(o)) == TP_ERR_ARG and not out.value
