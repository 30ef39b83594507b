"""CPU-side checks of the buckling boundary: the header declares the five calls, the binding knows them, the ABI number stays, the
argument rules answer before anything touches a device, calls before an assemble are refused, and the driver validates its new
fields before the grid is made."""
import ctypes as C
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG, TP_ERR_STATE = 1, 2
FIVE = (("tp_elasticity_geom_assemble", 5), ("tp_elasticity_geom_apply", 3), ("tp_elasticity_geom_sensitivity", 10),
        ("tp_elasticity_geom_adjoint_rhs", 9), ("tp_elasticity_get_geom_tables", 3))


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_five_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs in FIVE:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    names = [re.split(r"[\s\*]+", a)[-1] for a in _declared_args(src, "tp_elasticity_geom_sensitivity")]
    assert names == ["e", "ncase", "Phi", "w", "xPhys", "U", "Emax", "penal", "scale", "out"]
    names = [re.split(r"[\s\*]+", a)[-1] for a in _declared_args(src, "tp_elasticity_geom_adjoint_rhs")]
    assert names == ["e", "ncase", "Phi", "w", "xPhys", "Emax", "penal", "scale", "out"]
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4 and lib.load_library().tp_abi_version() == 4


def test_argument_rules_answer_before_any_launch():
    """every TP_ERR_ARG comes before the first use of the grid or of a device array, so a zeroed block of host memory can stand in
    for the handle (as tests/test_eigen_abi.py does); that handle has no supports and no assemble behind it: geom_assemble with good
    arguments answers TP_ERR_STATE, the three other calls TP_ERR_ARG (no assemble yet), still without touching the grid"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    e = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    u = C.cast(C.create_string_buffer(64), C.c_void_p)
    r = C.cast(C.create_string_buffer(64), C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def asm(handle=e, xp=x, U=u, Emax=1.0, penal=3.0):
        return L.tp_elasticity_geom_assemble(handle, xp, U, Emax, penal)

    assert asm(handle=None) == TP_ERR_ARG and asm(xp=None) == TP_ERR_ARG and asm(U=None) == TP_ERR_ARG
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert asm(Emax=bad) == TP_ERR_ARG
    for bad in (0.5, -1.0, nan, inf):
        assert asm(penal=bad) == TP_ERR_ARG
    assert asm() == TP_ERR_STATE and asm(penal=1.0) == TP_ERR_STATE

    assert L.tp_elasticity_geom_apply(None, x, r) == TP_ERR_ARG
    assert L.tp_elasticity_geom_apply(e, None, r) == TP_ERR_ARG
    assert L.tp_elasticity_geom_apply(e, x, None) == TP_ERR_ARG
    assert L.tp_elasticity_geom_apply(e, x, x) == TP_ERR_ARG
    assert L.tp_elasticity_geom_apply(e, x, r) == TP_ERR_ARG          # before an assemble

    one = (C.c_void_p * 1)(x.value)
    eight = (C.c_void_p * 8)(*([x.value] * 8))
    nul = (C.c_void_p * 2)(x.value, None)
    w = (C.c_double * 8)(*([1.0] * 8))

    def sens(handle=e, ncase=1, V=one, xp=x, U=u, Emax=1.0, penal=3.0, scale=-2.0, out=r):
        return L.tp_elasticity_geom_sensitivity(handle, ncase, V, w, xp, U, Emax, penal, scale, out)

    def adj(handle=e, ncase=1, V=one, xp=x, Emax=1.0, penal=3.0, scale=-2.0, out=r):
        return L.tp_elasticity_geom_adjoint_rhs(handle, ncase, V, w, xp, Emax, penal, scale, out)

    for f in (sens, adj):
        assert f(handle=None) == TP_ERR_ARG and f(V=None) == TP_ERR_ARG and f(xp=None) == TP_ERR_ARG and f(out=None) == TP_ERR_ARG
        assert f(ncase=0) == TP_ERR_ARG and f(ncase=-1) == TP_ERR_ARG and f(ncase=9, V=eight) == TP_ERR_ARG
        assert f(ncase=2, V=nul) == TP_ERR_ARG
        for bad in (nan, inf, -inf):
            assert f(scale=bad) == TP_ERR_ARG and f(Emax=bad) == TP_ERR_ARG
        assert f(Emax=0.0) == TP_ERR_ARG and f(penal=0.5) == TP_ERR_ARG
        assert f() == TP_ERR_ARG and f(ncase=8, V=eight) == TP_ERR_ARG        # good arguments, but before an assemble
    assert sens(U=None) == TP_ERR_ARG

    assert L.tp_elasticity_get_geom_tables(None, x, r) == TP_ERR_ARG
    assert L.tp_elasticity_get_geom_tables(e, None, r) == TP_ERR_ARG and L.tp_elasticity_get_geom_tables(e, x, None) == TP_ERR_ARG


def test_driver_has_the_buckling_fields_and_refuses_bad_values():
    from topopt_in_petsc_amd.api import LinearElasticity
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["buckling_limit"] is None and f["buckling_modes"] == 2 and f["buckling_P"] == 8.0
    assert f["buckling_tol"] == 1e-6 and f["buckling_case"] == 0 and f["load"] == "cantilever"
    for name in ("GeomAssemble", "GeomMult", "GeomSensitivity", "GeomAdjointRHS", "GeomTables", "BucklingModes", "BucklingVectors",
                 "BucklingSensitivity", "SetUpLoadAndBC_Axial"):
        assert callable(getattr(LinearElasticity, name))
    nan, inf = float("nan"), float("inf")
    for kw in (dict(buckling_limit=0.0), dict(buckling_limit=-1.0), dict(buckling_limit=nan), dict(buckling_limit=inf),
               dict(buckling_limit=1.0, buckling_modes=0), dict(buckling_limit=1.0, buckling_modes=5), dict(buckling_limit=1.0, buckling_modes=1.5),
               dict(buckling_limit=1.0, buckling_P=0.5), dict(buckling_limit=1.0, buckling_P=nan),
               dict(buckling_limit=1.0, buckling_tol=0.0), dict(buckling_limit=1.0, buckling_tol=nan),
               dict(buckling_limit=1.0, buckling_case=1), dict(buckling_limit=1.0, buckling_case=-1),
               dict(buckling_limit=1.0, body_force=(0.0, 0.0, -1.0)),
               dict(buckling_limit=1.0, physics="thermoelastic", alpha=1e-3, thermal="uniform", delta_T=1.0),
               dict(buckling_limit=1.0, physics="heat"),
               dict(load="sideways"), dict(load="axial", physics="heat")):
        with pytest.raises(ValueError):      # before the grid is made: no device needed
            TopOpt(**kw)
