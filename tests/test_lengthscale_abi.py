"""CPU-side checks of the length-scale boundary: the header declares the five calls, the binding knows each with a matching
argument count, the ABI number stays, the argument rules answer before anything touches a device, the driver has the new fields
-- and the numpy restatement the GPU tests measure against (tests/lengthscale_ref.py) is itself held to central differences, to
the activity condition on every field the GPU tests use, and to the closed form on a uniform field."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import lengthscale_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG = 1
LD = ref.LD
CALLS = (("tp_lengthscale_create", 2), ("tp_lengthscale_destroy", 1), ("tp_lengthscale_constraints", 15),
         ("tp_lengthscale_get_terms", 3), ("tp_filter_gradients_from_tilde", 4))
# the meshes of the central-difference check: 6x5x4 anisotropic and 8x4x4
FD_CASES = [((6, 5, 4), (0.05, 0.04, 0.03)), ((8, 4, 4), (0.25, 0.25, 0.25))]


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_lengthscale_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs in CALLS:
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    names = [re.split(r"[\s\*]+", a)[-1] for a in _declared_args(src, "tp_lengthscale_constraints")]
    assert names == ["ls", "xTilde", "xPhys", "proj", "beta", "eta", "c", "eta_s", "eta_v", "eps", "kinds", "g", "S", "dg_solid",
                     "dg_void"]
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4


def test_argument_rules_answer_before_any_launch():
    """every rule of the header comes before the first use of the handle, so a zeroed block of host memory can stand in for one"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    ls = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)     # never dereferenced by a call that fails its checks
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    nan, inf = float("nan"), float("inf")
    ok = dict(ls=ls, xt=x, xp=x, proj=1, beta=8.0, eta=0.5, c=0.1, eta_s=0.75, eta_v=0.25, eps=1e-6, kinds=3)

    def go(**kw):
        a = dict(ok, **kw)
        return L.tp_lengthscale_constraints(a["ls"], a["xt"], a["xp"], a["proj"], a["beta"], a["eta"], a["c"], a["eta_s"], a["eta_v"],
                                            a["eps"], a["kinds"], None, None, None, None)

    bad = [dict(ls=None), dict(xt=None), dict(xp=None), dict(kinds=0), dict(kinds=4), dict(kinds=-1), dict(c=-1e-3), dict(c=nan),
           dict(c=inf), dict(eps=0.0), dict(eps=-1e-6), dict(eps=nan), dict(eps=inf), dict(eta_s=0.0), dict(eta_s=1.0), dict(eta_s=nan),
           dict(eta_v=0.0), dict(eta_v=1.0), dict(eta_v=-0.2), dict(eta_v=nan), dict(beta=0.0), dict(beta=-1.0), dict(beta=nan),
           dict(beta=inf), dict(eta=-0.1), dict(eta=1.1), dict(eta=nan), dict(proj=0, beta=nan), dict(proj=0, eta=inf)]
    for kw in bad:
        assert go(**kw) == TP_ERR_ARG, kw
    out = C.c_void_p()
    assert L.tp_lengthscale_create(C.byref(out), None) == TP_ERR_ARG
    assert L.tp_lengthscale_create(None, ls) == TP_ERR_ARG
    assert L.tp_lengthscale_get_terms(None, x, x) == TP_ERR_ARG
    assert L.tp_lengthscale_destroy(None) == 0
    # the filter's transpose: a zeroed block reads as filter type 0, which has none
    rows = (C.c_void_p * 1)(x)
    assert L.tp_filter_gradients_from_tilde(None, x, 1, rows) == TP_ERR_ARG
    assert L.tp_filter_gradients_from_tilde(ls, None, 1, rows) == TP_ERR_ARG
    assert L.tp_filter_gradients_from_tilde(ls, x, 1, None) == TP_ERR_ARG
    assert L.tp_filter_gradients_from_tilde(ls, x, 1, rows) == TP_ERR_ARG


def test_driver_has_the_length_scale_fields_and_refuses_bad_values():
    from topopt_in_petsc_amd.api import Filter, LengthScale
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["length_scale"] is None and f["length_scale_c"] is None and f["length_scale_eta"] == (0.75, 0.25)
    assert f["length_scale_eps"] > 0.0 and f["length_scale_start"] == 1 and f["m"] == 1
    print("length_scale_eps default: %g" % f["length_scale_eps"])
    assert hasattr(LengthScale, "Constraints") and hasattr(Filter, "GradientsFromTilde")
    # the argument rules of the driver come before the grid is made: no device needed
    for kw in (dict(length_scale="both", filter=0), dict(length_scale="thin"), dict(length_scale="both", length_scale_c=0.0),
               dict(length_scale="both", length_scale_c=-1.0), dict(length_scale="solid", length_scale_eps=0.0),
               dict(length_scale="void", length_scale_eps=-1e-6), dict(length_scale="both", length_scale_eta=(1.0, 0.25)),
               dict(length_scale="both", length_scale_eta=(0.75, 0.0)), dict(length_scale="both", length_scale_start=0)):
        with pytest.raises(ValueError):
            TopOpt(**kw)


@pytest.mark.parametrize("ne,h", FD_CASES)
@pytest.mark.parametrize("proj", [0, 1])
def test_restatement_gradient_against_its_own_central_differences(ne, h, proj):
    """analytic dg/drt . W against (g(rt + s W) - g(rt - s W)) / (2 s), s = 1e-6, relative 1e-6 (the figures of
    tests/test_localvol_abi.py), both kinds; the projected field follows the perturbed one"""
    s, c = 1e-6, ref.default_c(h)
    n = ne[0] * ne[1] * ne[2]
    rt = ref.field("random", ne, h)
    W = np.random.default_rng(11).uniform(-1.0, 1.0, n)
    r0 = ref.reference(rt, ne, h, c, proj=proj)
    rp = ref.reference(rt.astype(LD) + LD(s) * W, ne, h, c, proj=proj)
    rm = ref.reference(rt.astype(LD) - LD(s) * W, ne, h, c, proj=proj)
    for kind in ("solid", "void"):
        fd, an = (rp["g_" + kind] - rm["g_" + kind]) / (2 * LD(s)), (r0["dg_" + kind] * W).sum()
        err = float(abs(fd - an) / abs(an))
        print("%s proj=%d %s: dg.W %.6e, central difference off by %.3e (bound 1e-6)" % ("x".join(map(str, ne)), proj, kind, float(an), err))
        assert err <= 1e-6


@pytest.mark.parametrize("mesh", sorted(ref.MESHES))
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("proj", [0, 1])
def test_activity_condition_on_the_fields_of_the_gpu_tests(mesh, kind, proj):
    """at least a quarter of the elements carry T_e > 1e-6 max T for each kind, and max c G_e < 40: E is nowhere near underflow"""
    ne, h = ref.MESHES[mesh]
    n = ne[0] * ne[1] * ne[2]
    r = ref.reference(ref.field(kind, ne, h), ne, h, ref.default_c(h), proj=proj)
    cg = float((ref.default_c(h) * r["G"]).max())
    act = {k: int((r["T_" + k] > 1e-6 * r["T_" + k].max()).sum()) for k in ("solid", "void")}
    print("%s %s proj=%d: active solid %d, void %d of %d; max c G %.3f" % (mesh, kind, proj, act["solid"], act["void"], n, cg))
    assert 4 * act["solid"] >= n and 4 * act["void"] >= n and cg < 40.0


def test_restatement_on_a_uniform_field():
    """rt = 0.5: G = 0, S_solid = n H(0.5) 0.0625, and the stencil term of the gradient is exactly zero"""
    ne, h = ref.MESHES["a"]
    n = ne[0] * ne[1] * ne[2]
    for proj in (0, 1):
        r = ref.reference(np.full(n, 0.5), ne, h, ref.default_c(h), proj=proj)
        H = ref.heaviside(0.5, ref.BETA, ref.ETA) if proj else LD(0.5)
        assert not r["G"].any() and not r["stencil_solid"].any() and not r["stencil_void"].any()
        assert abs(r["S_solid"] - n * H * LD(0.0625)) <= 1e-17 * n and abs(r["S_void"] - n * (1 - H) * LD(0.0625)) <= 1e-17 * n
