"""CPU-side checks of the local volume boundary: the header declares the tp_localvol calls, the binding knows each with a
matching argument count, the ABI number stays, the argument rules answer before anything touches a device, the driver has the
new fields -- and the numpy restatement the GPU tests measure against (tests/localvol_ref.py) is itself held to central
differences and to Euler's identity."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import localvol_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1
CALLS = (("tp_localvol_create", 3), ("tp_localvol_destroy", 1), ("tp_localvol_stencil_width", 1), ("tp_localvol_get_count", 2),
         ("tp_localvol_last_kernel", 1), ("tp_localvol_mean", 3), ("tp_localvol_constraint", 9))
# (elements, h, R): the two small meshes of tests/test_gpu_localvol.py
CASES = [((16, 8, 8), (0.125, 0.125, 0.125), 2.5 * 0.125), ((20, 12, 8), (0.05, 0.04, 0.03), 0.11)]


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_localvol_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    names = [re.split(r"[\s\*]+", a)[-1] for a in _declared_args(src, "tp_localvol_constraint")]
    assert names == ["lv", "xPhys", "alpha", "p", "g", "pn", "rhobar_max", "rhobar", "dgdx"]
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4


def test_argument_rules_answer_before_any_launch():
    """TP_ERR_ARG unless p >= 1, alpha > 0, R > 0, and for a NULL handle, grid or density: all of it comes before the first use of
    the handle, so a zeroed block of host memory can stand in for one (as tests/test_stress_abi.py does)"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    lv = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)     # never dereferenced by a call that fails its checks
    x = C.cast(C.create_string_buffer(64), C.c_void_p)

    def go(handle, xp, alpha, p):
        return L.tp_localvol_constraint(handle, xp, alpha, p, None, None, None, None, None)

    assert go(None, x, 0.6, 16.0) == TP_ERR_ARG
    assert go(lv, None, 0.6, 16.0) == TP_ERR_ARG
    assert go(lv, x, 0.6, 0.5) == TP_ERR_ARG             # p < 1
    assert go(lv, x, 0.6, float("nan")) == TP_ERR_ARG
    assert go(lv, x, 0.0, 16.0) == TP_ERR_ARG            # alpha <= 0
    assert go(lv, x, -1.0, 16.0) == TP_ERR_ARG
    out = C.c_void_p()
    assert L.tp_localvol_create(C.byref(out), None, 0.3) == TP_ERR_ARG
    assert L.tp_localvol_create(C.byref(out), lv, 0.0) == TP_ERR_ARG        # R <= 0 (lv stands in for a grid)
    assert L.tp_localvol_create(C.byref(out), lv, -0.3) == TP_ERR_ARG
    assert L.tp_localvol_mean(None, x, x) == TP_ERR_ARG
    assert L.tp_localvol_get_count(None, x) == TP_ERR_ARG
    assert L.tp_localvol_destroy(None) == 0


def test_driver_has_the_local_volume_fields_and_refuses_bad_values():
    from topopt_in_petsc_amd.api import LocalVolume
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["local_volume"] is None and f["local_volume_R"] is None and f["local_volume_p"] == 16.0 and f["m"] == 1
    for name in ("Mean", "Constraint", "count", "stencil_width"):
        assert hasattr(LocalVolume, name)
    # the argument rules of the driver come before the grid is made: no device needed
    for kw in (dict(local_volume=0.4), dict(local_volume=0.4, local_volume_R=0.0), dict(local_volume=-0.1, local_volume_R=0.2),
               dict(local_volume=0.0, local_volume_R=0.2)):
        with pytest.raises(ValueError):
            TopOpt(**kw)


@pytest.mark.parametrize("ne,h,R", CASES)
@pytest.mark.parametrize("p", [1.0, 16.0])
def test_restatement_gradient_against_its_own_central_differences_and_euler(ne, h, R, p):
    """analytic dg/drho . W against (g(rho + eps W) - g(rho - eps W)) / (2 eps), eps = 1e-6, relative 1e-6 (the figures of
    tests/test_gpu_stress.py); sum_j rho_j dg/drho_j = pn / alpha to 1e-15 relative in 80-bit arithmetic (a few hundred roundings
    at 2^-64)"""
    alpha, eps = 0.6, 1e-6
    rng = np.random.default_rng(11)
    n = ne[0] * ne[1] * ne[2]
    rho, W = rng.uniform(0.1, 0.9, n), rng.uniform(-1.0, 1.0, n)
    r0 = ref.reference(rho, ne, h, R, alpha, p)
    gp = ref.reference(rho.astype(ref.LD) + ref.LD(eps) * W, ne, h, R, alpha, p)["g"]
    gm = ref.reference(rho.astype(ref.LD) - ref.LD(eps) * W, ne, h, R, alpha, p)["g"]
    fd, an = (gp - gm) / (2 * ref.LD(eps)), (r0["dgdx"] * W).sum()
    e_fd = float(abs(fd - an) / abs(an))
    e_eu = float(abs((rho * r0["dgdx"]).sum() - r0["pn"] / alpha) / (r0["pn"] / alpha))
    print("%s p=%g: conn %d, dg.W %.6e, central difference off by %.3e (bound 1e-6); Euler off by %.3e (bound 1e-15)"
          % ("x".join(map(str, ne)), p, ref.stencil_width(ne, h, R), float(an), e_fd, e_eu))
    assert e_fd <= 1e-6 and e_eu <= 1e-15


def test_restatement_uniform_field_and_counts():
    """rho = rho0: rb = rho0, g = rho0 / alpha - 1, sum dg/drho = 1 / alpha; cnt of an interior element of the cubic mesh at
    R = 2.5 h is the 81 lattice points with i^2 + j^2 + k^2 < 6.25, a corner element sees one octant of them (27)"""
    ne, h, R = CASES[0]
    n = ne[0] * ne[1] * ne[2]
    r = ref.reference(np.full(n, 0.12), ne, h, R, 0.6, 16.0)
    assert abs(float(r["g"]) - (0.12 / 0.6 - 1)) < 1e-15 and abs(float(r["dgdx"].sum()) - 1 / 0.6) < 1e-15
    inside = sum(1 for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3) if i * i + j * j + k * k < 6.25)
    octant = sum(1 for i in range(0, 3) for j in range(0, 3) for k in range(0, 3) if i * i + j * j + k * k < 6.25)
    cnt = r["cnt"].reshape(ne[2], ne[1], ne[0])
    assert inside == 81 and cnt[4, 4, 8] == inside and cnt[0, 0, 0] == octant
