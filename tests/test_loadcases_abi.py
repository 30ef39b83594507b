"""CPU-side checks of the load-case boundary: the header declares tp_elasticity_response and TP_MAX_CASES, the binding
knows them, and the argument checks answer before anything touches a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1


def _header():
    return open(os.path.join(ROOT, "include", "topopt_amd.h")).read()


def test_header_declares_the_response_call_and_the_binding_has_it():
    from topopt_in_petsc_amd import lib
    src = _header()
    m = re.search(r"#define\s+TP_MAX_CASES\s+(\d+)", src)
    assert m, "include/topopt_amd.h does not define TP_MAX_CASES"
    assert int(m.group(1)) == lib.MAX_CASES == 8
    assert re.search(r"\bint\s+tp_elasticity_response\s*\(\s*tp_elasticity\s*\*\s*e\s*,\s*int\s+ncase\b", src)
    res, args = lib.SYMBOLS["tp_elasticity_response"]
    assert res is C.c_int and len(args) == 15
    assert hasattr(lib.load_library(), "tp_elasticity_response")
    # no option struct changed: the ABI number stays
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4


def test_argument_checks_answer_before_any_launch():
    """tests/test_abi.py calls into the library without a device (tp_solver_default_opts); the argument checks of
    tp_elasticity_response are reachable the same way because they come before the first use of the handle: a NULL handle, and
    -- behind a zeroed block of host memory standing in for one -- ncase = 0, ncase = TP_MAX_CASES + 1, U = NULL, one U[l] NULL,
    xPhys = NULL"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    call = L.tp_elasticity_response
    dummy = C.create_string_buffer(1 << 20)       # never dereferenced by a call that fails its checks
    e = C.cast(dummy, C.c_void_p)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    u = C.cast(C.create_string_buffer(64), C.c_void_p).value

    def go(handle, ncase, U, xp):
        return call(handle, ncase, U, None, None, xp, 1e-9, 1.0, 3.0, 0.12, None, None, None, None, None)

    ok2 = (C.c_void_p * 2)(u, u)
    assert go(None, 2, ok2, x) == TP_ERR_ARG
    assert go(e, 0, ok2, x) == TP_ERR_ARG
    assert go(e, -1, ok2, x) == TP_ERR_ARG
    nine = (C.c_void_p * (lib.MAX_CASES + 1))(*([u] * (lib.MAX_CASES + 1)))
    assert go(e, lib.MAX_CASES + 1, nine, x) == TP_ERR_ARG
    assert go(e, 2, None, x) == TP_ERR_ARG
    assert go(e, 2, (C.c_void_p * 2)(u, None), x) == TP_ERR_ARG
    assert go(e, 2, ok2, None) == TP_ERR_ARG
