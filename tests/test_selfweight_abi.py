"""CPU-side checks of the self-weight boundary: the header declares the two calls, the binding knows them with matching argument
counts, the ABI number stays, the argument rules answer before anything touches a device, the driver has the three new fields --
and the numpy restatement the GPU tests measure against (tests/selfweight_ref.py) is itself held to central differences, to its
matching conditions at x_low, to the partition of unity and to central differences of the compliance of a small cantilever."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import selfweight_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG, TP_ERR_STATE = 1, 2
LD = ref.LD
B = (0.3, -0.7, 1.1)


def _declared_args(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, "include/topopt_amd.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_the_body_force_calls_and_the_binding_has_them():
    from topopt_in_petsc_amd import lib
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    for name, nargs in (("tp_elasticity_body_load", 6), ("tp_elasticity_body_sensitivity", 9)):
        declared = _declared_args(src, name)
        res, args = lib.SYMBOLS[name]
        print("%s: header %d arguments, binding %d" % (name, len(declared), len(args)))
        assert res is C.c_int and len(declared) == len(args) == nargs
        assert hasattr(lib.load_library(), name)
    names = [re.split(r"[\s\*]+", a)[-1] for a in _declared_args(src, "tp_elasticity_body_sensitivity")]
    assert names == ["e", "ncase", "V", "w", "xPhys", "b3", "x_low", "scale", "dfdx"]
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4


def test_argument_rules_answer_before_any_launch():
    """every TP_ERR_ARG comes before the first use of the grid or of a device array, so a zeroed block of host memory can stand
    in for the handle (as tests/test_overhang_abi.py does); that handle has no supports: a call that passes the argument rules
    answers TP_ERR_STATE, still without touching the grid"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    e = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    r = C.cast(C.create_string_buffer(64), C.c_void_p)
    b = (C.c_double * 3)(*B)
    nan, inf = float("nan"), float("inf")

    def load(handle=e, xp=x, b3=b, x_low=0.1, rhs=r):
        return L.tp_elasticity_body_load(handle, xp, b3, x_low, None, rhs)

    assert load(handle=None) == TP_ERR_ARG
    assert load(xp=None) == TP_ERR_ARG
    assert load(b3=None) == TP_ERR_ARG
    assert load(rhs=None) == TP_ERR_ARG
    for bad in (-0.1, 1.0, 1.5, nan, inf):
        assert load(x_low=bad) == TP_ERR_ARG
    for bad in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf)):
        assert load(b3=(C.c_double * 3)(*bad)) == TP_ERR_ARG
    assert load() == TP_ERR_STATE and load(x_low=0.0) == TP_ERR_STATE

    one = (C.c_void_p * 1)(x.value)
    eight = (C.c_void_p * 8)(*([x.value] * 8))
    nul = (C.c_void_p * 2)(x.value, None)
    w = (C.c_double * 8)(*([1.0] * 8))

    def sens(handle=e, ncase=1, V=one, xp=x, b3=b, x_low=0.1, scale=2.0, dfdx=r):
        return L.tp_elasticity_body_sensitivity(handle, ncase, V, w, xp, b3, x_low, scale, dfdx)

    assert sens(handle=None) == TP_ERR_ARG
    assert sens(V=None) == TP_ERR_ARG
    assert sens(xp=None) == TP_ERR_ARG
    assert sens(b3=None) == TP_ERR_ARG
    assert sens(dfdx=None) == TP_ERR_ARG
    assert sens(ncase=0) == TP_ERR_ARG and sens(ncase=-1) == TP_ERR_ARG
    assert sens(ncase=9, V=eight) == TP_ERR_ARG
    assert sens(ncase=2, V=nul) == TP_ERR_ARG
    for bad in (-0.1, 1.0, nan):
        assert sens(x_low=bad) == TP_ERR_ARG
    for bad in (nan, inf, -inf):
        assert sens(scale=bad) == TP_ERR_ARG
    assert sens(b3=(C.c_double * 3)(0.0, nan, 0.0)) == TP_ERR_ARG
    assert sens() == TP_ERR_STATE and sens(ncase=8, V=eight) == TP_ERR_STATE


def test_driver_has_the_body_force_fields_and_refuses_bad_values():
    from topopt_in_petsc_amd.api import LinearElasticity
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["body_force"] is None and f["body_force_xlow"] == 0.1 and f["point_load"] is True
    for name in ("SetBodyForce", "BodyLoad", "BodySensitivity"):
        assert callable(getattr(LinearElasticity, name))
    nan = float("nan")
    for kw in (dict(body_force=(0.0, 0.0)), dict(body_force=(0.0, 0.0, 0.0, 1.0)), dict(body_force=(0.0, nan, 0.0)),
               dict(body_force=(0.0, 0.0, float("inf"))), dict(body_force="gravity"), dict(body_force=9.81),
               dict(body_force=(0.0, 0.0, -1.0), body_force_xlow=1.0), dict(body_force=(0.0, 0.0, -1.0), body_force_xlow=-0.1),
               dict(body_force=(0.0, 0.0, -1.0), body_force_xlow=nan), dict(body_force_xlow=1.5), dict(point_load=False)):
        with pytest.raises(ValueError):      # before the grid is made: no device needed
            TopOpt(**kw)


@pytest.mark.parametrize("x_low", [0.0, 0.1, 0.3])
def test_restatement_derivative_against_central_differences(x_low):
    """m' against (m(x + d) - m(x - d)) / 2d, d = 1e-6, relative 1e-8, on both sides of x_low"""
    d = LD(1e-6)
    pts = [0.02, 0.05, 0.09, 0.2, 0.29, 0.31, 0.5, 0.9, 1.0, 1.004]
    pts += [0.5 * x_low, 0.9 * x_low, 1.1 * x_low] if x_low else []
    x = np.array(pts, dtype=LD)
    fd = (ref.mass(x + d, x_low) - ref.mass(x - d, x_low)) / (2 * d)
    an = ref.dmass(x, x_low)
    err = np.abs(fd - an) / np.abs(an)
    for xv, a, f, e in zip(x, an, fd, err):
        print("x_low %.1f x %.4f: m' %.12e, central difference %.12e, off by %.3e (bound 1e-8)" % (x_low, float(xv), float(a), float(f), float(e)))
    assert float(err.max()) <= 1e-8
    assert float(ref.dmass(np.linspace(0.0, 1.0, 2001), x_low).min()) >= 0.0


@pytest.mark.parametrize("x_low", [0.1, 0.3])
def test_restatement_matches_the_line_at_x_low(x_low):
    """m(x_low) = x_low and m'(x_low) = 1 to 4 ulp, and so for the damped branch's own polynomials at t = 1"""
    ulp = float(np.finfo(LD).eps)
    xl = LD(x_low)
    m, dm = ref.mass(np.array([xl]), x_low)[0], ref.dmass(np.array([xl]), x_low)[0]
    print("x_low %.1f: |m - x_low| / x_low = %.3e, |m' - 1| = %.3e (bound 4 ulp = %.3e)" % (x_low, float(abs(m - xl) / xl), float(abs(dm - 1)), 4 * ulp))
    assert float(abs(m - xl) / xl) <= 4 * ulp and float(abs(dm - 1)) <= 4 * ulp
    t = LD(1)                                    # the damped branch itself at t = 1
    assert float(abs(t ** 5 * (6 - 5 * t) - 1)) <= 4 * ulp and float(abs(t ** 5 * (36 - 35 * t) - 1)) <= 4 * ulp


@pytest.mark.parametrize("ne,h", [((16, 8, 8), (0.125, 0.125, 0.125)), ((20, 12, 8), (0.05, 0.04, 0.03)), ((3, 2, 1), (1.0, 0.5, 0.25))])
@pytest.mark.parametrize("x_low", [0.0, 0.1])
def test_restatement_partition_of_unity(ne, h, x_low):
    """sum_n f_n = V_e b sum_e m(x_e) to 1e-15 relative in 80-bit arithmetic"""
    nel, nnode = ne[0] * ne[1] * ne[2], (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
    x = np.random.default_rng(3).uniform(0.0, 1.0, nel)
    x[::2] *= 0.15
    f = ref.load(x, ref.elem_dofs(*ne), nnode, h, B, x_low).reshape(-1, 3)
    tot = ref.volume(h) * ref.mass(x, x_low).sum()
    for c in range(3):
        err = float(abs(f[:, c].sum() - tot * LD(B[c])) / abs(tot * LD(B[c])))
        print("%s x_low %.1f component %d: sum f %.15e, off by %.3e (bound 1e-15)" % ("x".join(map(str, ne)), x_low, c, float(f[:, c].sum()), err))
        assert err <= 1e-15


def _cantilever(ex, ey, ez, h):
    """supports and line load of the cantilever (clamp x = xmin; load -0.001 in z along x = xmax, z = zmin, half at the ends)"""
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    N = np.ones((nz, ny, nx, 3))
    N[:, :, 0, :] = 0.0
    R = np.zeros((nz, ny, nx, 3))
    R[0, :, nx - 1, 2] = -0.001
    R[0, 0, nx - 1, 2] = R[0, ny - 1, nx - 1, 2] = -0.0005
    return N.reshape(-1), R.reshape(-1)


@pytest.mark.parametrize("x_low", [0.0, 0.1])
def test_restatement_total_derivative_against_central_differences_of_the_compliance(orc, x_low):
    """6x4x4, Emin 1e-3, the cantilever's supports and load plus self-weight, K from the oracle's KE and a sparse direct solve:
    dc/dx . W against (c(x + eps W) - c(x - eps W)) / 2 eps, eps = 1e-6, relative 1e-6"""
    from tests import scipy_check as sc
    import scipy.sparse.linalg as spl
    (ex, ey, ez), h = (6, 4, 4), (0.25, 0.25, 0.25)
    Emin, Emax, penal, eps = 1e-3, 1.0, 3.0, 1e-6
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], 0.3)).reshape(24, 24)
    N, R = _cantilever(ex, ey, ez, h)
    dofs, nnode = ref.elem_dofs(ex, ey, ez), (ex + 1) * (ey + 1) * (ez + 1)
    assert np.array_equal(dofs[:, ::3] // 3, sc.elem_nodes(ex, ey, ez))
    rng = np.random.default_rng(17)
    x = rng.uniform(0.02, 0.9, ex * ey * ez)
    x[::3] = rng.uniform(0.01, 0.09, x[::3].size)      # a third below x_low = 0.1
    W = rng.uniform(-1.0, 1.0, x.size)
    # a body force whose load is of the size of the point load (0.004 in all): the two terms of dc/dx are both visible
    scale = 0.004 / (float(ref.volume(h)) * x.sum() * 1.3)
    b = tuple(scale * v for v in B)

    def state(xv):
        F = R + np.asarray(ref.load(xv, dofs, nnode, h, b, x_low), dtype=np.float64)
        K = sc.assemble(ex, ey, ez, KE, E=Emin + xv ** penal * (Emax - Emin), N=N)
        u = spl.splu(K.tocsc()).solve(N * F)
        return float(np.dot((N * F).astype(LD), u.astype(LD))), u

    c0, u = state(x)
    dc, classical, body = ref.dcdx(x, dofs, h, b, x_low, N, KE, u, Emin, Emax, penal)
    an = float((dc * W).sum())
    fd = (state(x + eps * W)[0] - state(x - eps * W)[0]) / (2 * eps)
    err = abs(an / fd - 1)
    print("x_low %.1f: c %.6e, dc/dx . W %.9e (classical %.3e, self-weight %.3e), central difference %.9e, off by %.3e (bound 1e-6)"
          % (x_low, c0, an, float((classical * W).sum()), float((body * W).sum()), fd, err))
    assert err <= 1e-6
    assert abs(float((body * W).sum())) > 1e-3 * abs(an)      # without the new term the comparison fails
    assert float(body.max()) > 0 > float(classical.max())     # the total is not of one sign term by term
