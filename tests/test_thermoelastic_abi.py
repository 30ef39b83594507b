"""CPU-side checks of the thermoelastic boundary: the header declares the four calls and the parameter block, the
binding knows them with matching argument counts, the ABI number stays, the argument rules answer before anything touches a
device, and TopOpt(physics="thermoelastic") refuses what it does not support before a grid is made -- while "elasticity" and "heat"
construct their checks as before."""
import ctypes as C
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG, TP_ERR_STATE = 1, 2
CALLS = (("tp_elasticity_thermal_load", 6), ("tp_elasticity_thermal_sensitivity", 9), ("tp_elasticity_thermal_adjoint_rhs", 8),
         ("tp_elasticity_get_thermal_coupling", 2))


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_thermal_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    names = lambda f: [re.split(r"[\s\*]+", a)[-1] for a in _declared_args(src, f)]
    assert names("tp_elasticity_thermal_load") == ["e", "xPhys", "T", "par", "rhs_base", "rhs"]
    assert names("tp_elasticity_thermal_sensitivity") == ["e", "ncase", "V", "w", "xPhys", "T", "par", "scale", "dfdx"]
    assert names("tp_elasticity_thermal_adjoint_rhs") == ["e", "ncase", "V", "w", "xPhys", "par", "scale", "g"]
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tp_thermal_par\s*;", src)
    assert m and [v.strip() for v in m.group(1).replace("double", "").strip(" ;").split(",")] == ["alpha", "T_ref", "Emin", "Emax", "penal_beta"]
    assert [f[0] for f in lib.ThermalPar._fields_] == ["alpha", "T_ref", "Emin", "Emax", "penal_beta"] and C.sizeof(lib.ThermalPar) == 40
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4


def test_argument_rules_answer_before_any_launch():
    """every TP_ERR_ARG comes before the first use of the grid or of a device array, so a zeroed block of host memory can stand
    in for the handle (as tests/test_selfweight_abi.py does); that handle has no supports: a call that passes the argument rules
    answers TP_ERR_STATE, still without touching the grid"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    e = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    t = C.cast(C.create_string_buffer(64), C.c_void_p)
    r = C.cast(C.create_string_buffer(64), C.c_void_p)
    nan, inf = float("nan"), float("inf")
    good = dict(alpha=1e-3, T_ref=0.25, Emin=1e-9, Emax=1.0, penal_beta=3.0)
    P = lambda **kw: C.byref(lib.ThermalPar(**{**good, **kw}))
    bad_pars = [dict(alpha=nan), dict(alpha=inf), dict(T_ref=nan), dict(T_ref=-inf), dict(penal_beta=0.5), dict(penal_beta=nan),
                dict(Emin=-1e-9), dict(Emin=nan), dict(Emax=1e-9), dict(Emax=0.0), dict(Emax=nan), dict(Emin=2.0)]
    ok_pars = [dict(), dict(penal_beta=1.0), dict(Emin=0.0), dict(alpha=0.0), dict(alpha=-1.0, T_ref=-3.0)]

    def load(handle=e, xp=x, T=t, par=None, rhs=r):
        return L.tp_elasticity_thermal_load(handle, xp, T, P() if par is None else par, None, rhs)

    assert load(handle=None) == TP_ERR_ARG and load(xp=None) == TP_ERR_ARG and load(T=None) == TP_ERR_ARG and load(rhs=None) == TP_ERR_ARG
    assert L.tp_elasticity_thermal_load(e, x, t, None, None, r) == TP_ERR_ARG
    for kw in bad_pars:
        assert load(par=P(**kw)) == TP_ERR_ARG, kw
    for kw in ok_pars:
        assert load(par=P(**kw)) == TP_ERR_STATE, kw

    one = (C.c_void_p * 1)(x.value)
    eight = (C.c_void_p * 8)(*([x.value] * 8))
    nul = (C.c_void_p * 2)(x.value, None)
    w = (C.c_double * 8)(*([1.0] * 8))

    def sens(handle=e, ncase=1, V=one, xp=x, T=t, par=None, scale=2.0, dfdx=r):
        return L.tp_elasticity_thermal_sensitivity(handle, ncase, V, w, xp, T, P() if par is None else par, scale, dfdx)

    def adj(handle=e, ncase=1, V=one, xp=x, par=None, scale=1.0, g=r):
        return L.tp_elasticity_thermal_adjoint_rhs(handle, ncase, V, w, xp, P() if par is None else par, scale, g)

    for call, out in ((sens, "dfdx"), (adj, "g")):
        assert call(handle=None) == TP_ERR_ARG and call(V=None) == TP_ERR_ARG and call(xp=None) == TP_ERR_ARG
        assert call(**{out: None}) == TP_ERR_ARG
        assert call(ncase=0) == TP_ERR_ARG and call(ncase=-1) == TP_ERR_ARG and call(ncase=9, V=eight) == TP_ERR_ARG
        assert call(ncase=2, V=nul) == TP_ERR_ARG
        for bad in (nan, inf, -inf):
            assert call(scale=bad) == TP_ERR_ARG
        for kw in bad_pars:
            assert call(par=P(**kw)) == TP_ERR_ARG, kw
        assert call() == TP_ERR_STATE and call(ncase=8, V=eight) == TP_ERR_STATE
    assert sens(T=None) == TP_ERR_ARG
    assert L.tp_elasticity_thermal_sensitivity(e, 1, one, None, x, t, None, 2.0, r) == TP_ERR_ARG
    assert L.tp_elasticity_thermal_adjoint_rhs(e, 1, one, None, x, None, 1.0, r) == TP_ERR_ARG
    assert L.tp_elasticity_thermal_sensitivity(e, 1, one, None, x, t, P(), 2.0, r) == TP_ERR_STATE      # w NULL = all 1
    buf = (C.c_double * 192)()
    assert L.tp_elasticity_get_thermal_coupling(None, buf) == TP_ERR_ARG and L.tp_elasticity_get_thermal_coupling(e, None) == TP_ERR_ARG


def test_api_has_the_thermal_methods():
    from topopt_in_petsc_amd.api import HeatConduction, LinearElasticity, check_thermal
    for name in ("SetThermalExpansion", "SetTemperature", "ThermalLoad", "ThermalSensitivity", "ThermalAdjointRHS", "ThermalCoupling", "TotalRHS"):
        assert callable(getattr(LinearElasticity, name)), name
    assert callable(HeatConduction.SolveAdjoint)
    assert check_thermal(1e-3, 0, 3, 1e-9, 1) == (1e-3, 0.0, 1e-9, 1.0, 3.0)
    nan = float("nan")
    for bad in ((nan, 0, 3, 0, 1), (1, nan, 3, 0, 1), (1, 0, 0.9, 0, 1), (1, 0, 3, -1, 1), (1, 0, 3, 1, 1), ("a", 0, 3, 0, 1), (None, 0, 3, 0, 1)):
        with pytest.raises(ValueError):
            check_thermal(*bad)


REFUSED = [dict(loadcases=[("top", 1.0)]), dict(stress_limit=1.0), dict(body_force=(0.0, 0.0, -1.0)), dict(frequency_limit=1.0),
           dict(robust=(0.7, 0.5, 0.3), projectionFilter=True), dict(overhang="+z"), dict(local_volume=0.5, local_volume_R=0.2),
           dict(length_scale="both")]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: sorted(kw)[0])
def test_driver_refuses_unsupported_combinations_before_a_grid_is_made(kw):
    from topopt_in_petsc_amd.driver import TopOpt
    with pytest.raises(ValueError, match="thermoelastic"):
        TopOpt(physics="thermoelastic", alpha=1e-3, **kw)
    with pytest.raises(ValueError, match="thermoelastic"):
        TopOpt(physics="thermoelastic", alpha=1e-3, thermal="uniform", delta_T=1.0, **kw)


def test_driver_fields_and_parameter_rules():
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["alpha"] is None and f["T_ref"] == 0.0 and f["thermal_penal"] is None and f["thermal"] == "conduction" and f["delta_T"] is None
    nan, inf = float("nan"), float("inf")
    te = dict(physics="thermoelastic")
    for kw in (dict(te),                                                     # no alpha
               dict(te, alpha=nan), dict(te, alpha=inf), dict(te, alpha=1e-3, T_ref=nan),
               dict(te, alpha=1e-3, thermal_penal=0.5), dict(te, alpha=1e-3, penal=0.5),
               dict(te, alpha=1e-3, thermal="radiation"),
               dict(te, alpha=1e-3, delta_T=1.0),                            # delta_T without "uniform"
               dict(te, alpha=1e-3, thermal="uniform"),                      # "uniform" without delta_T
               dict(te, alpha=1e-3, thermal="uniform", delta_T=nan),
               dict(te, alpha=1e-3, kmin=0.0), dict(te, alpha=1e-3, kmin=2.0), dict(te, alpha=1e-3, kmax=inf),
               dict(te, alpha=1e-3, Emin=-1.0), dict(te, alpha=1e-3, Emin=1.0, Emax=1.0),
               dict(te, alpha=1e-3, point_load=False),
               dict(alpha=1e-3), dict(physics="heat", alpha=1e-3), dict(delta_T=1.0), dict(physics="heat", delta_T=1.0),
               dict(physics="thermal")):
        with pytest.raises(ValueError):      # before the grid is made: no device needed
            TopOpt(**kw)


def test_elasticity_and_heat_construct_as_before():
    """without a device both reach the grid's constructor -- their own checks pass as they did -- and fail there for want of a
    GPU; with one they construct.  Either way no ValueError"""
    from topopt_in_petsc_amd.driver import TopOpt
    for kw in (dict(), dict(physics="elasticity"), dict(physics="heat"), dict(physics="thermoelastic", alpha=1e-3),
               dict(physics="thermoelastic", alpha=1e-3, thermal="uniform", delta_T=2.0, T_ref=1.0, thermal_penal=2.0)):
        try:
            opt = TopOpt(nxyz=(9, 5, 5), xc=(0, 2, 0, 1, 0, 1), nlvls=2, **kw)
        except ValueError:
            raise
        except Exception as exc:             # no GPU here: the grid says so
            assert "GPU" in str(exc) or "hip" in str(exc).lower() or "cuda" in str(exc).lower(), exc
            continue
        assert opt.physics_kind == kw.get("physics", "elasticity")
        opt.grid.close()
