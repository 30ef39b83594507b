"""CPU-side checks of the eigenfrequency boundary: the header declares the five calls, the binding knows them, the ABI number
stays, the argument rules answer before anything touches a device, the driver validates its new fields -- and the numpy / scipy
restatement the GPU tests measure against (tests/eigen_ref.py) is itself held to the mass matrix's sums, to positive definiteness,
to central differences of J = sum 1 / lambda_i (through a double eigenvalue too), and to the conditions on every mesh and design of
the GPU tests that their bounds rest on."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from tests import eigen_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP_ERR_ARG, TP_ERR_STATE = 1, 2
LD = ref.LD
FIVE = (("tp_elasticity_mass_assemble", 4), ("tp_elasticity_mass_apply", 3), ("tp_elasticity_mass_sensitivity", 7),
        ("tp_vec_block_gram", 6), ("tp_vec_block_combine", 6))


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
    names = [re.split(r"[\s\*]+", a)[-1] for a in _declared_args(src, "tp_elasticity_mass_sensitivity")]
    assert names == ["e", "ncase", "V", "w", "xPhys", "scale", "out"]
    assert re.search(r"#define\s+TP_ABI_VERSION\s+4\b", src) and lib.ABI_VERSION == 4 and lib.load_library().tp_abi_version() == 4


def test_argument_rules_answer_before_any_launch():
    """every TP_ERR_ARG comes before the first use of the grid or of a device array, so a zeroed block of host memory can stand in
    for the handle (as tests/test_selfweight_abi.py does); that handle has no supports and no mass: a call that passes the
    argument rules answers TP_ERR_STATE, still without touching the grid"""
    from topopt_in_petsc_amd import lib
    L = lib.load_library()
    e = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    r = C.cast(C.create_string_buffer(64), C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def asm(handle=e, xp=x, rho0=1.0, x_low=0.1):
        return L.tp_elasticity_mass_assemble(handle, xp, rho0, x_low)

    assert asm(handle=None) == TP_ERR_ARG and asm(xp=None) == TP_ERR_ARG
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert asm(rho0=bad) == TP_ERR_ARG
    for bad in (-0.1, 1.0, 1.5, nan, inf):
        assert asm(x_low=bad) == TP_ERR_ARG
    assert asm() == TP_ERR_STATE and asm(x_low=0.0) == TP_ERR_STATE

    assert L.tp_elasticity_mass_apply(None, x, r) == TP_ERR_ARG
    assert L.tp_elasticity_mass_apply(e, None, r) == TP_ERR_ARG
    assert L.tp_elasticity_mass_apply(e, x, None) == TP_ERR_ARG
    assert L.tp_elasticity_mass_apply(e, x, r) == TP_ERR_STATE

    one = (C.c_void_p * 1)(x.value)
    eight = (C.c_void_p * 8)(*([x.value] * 8))
    nul = (C.c_void_p * 2)(x.value, None)
    w = (C.c_double * 8)(*([1.0] * 8))

    def sens(handle=e, ncase=1, V=one, xp=x, scale=-2.0, out=r):
        return L.tp_elasticity_mass_sensitivity(handle, ncase, V, w, xp, scale, out)

    assert sens(handle=None) == TP_ERR_ARG and sens(V=None) == TP_ERR_ARG and sens(xp=None) == TP_ERR_ARG and sens(out=None) == TP_ERR_ARG
    assert sens(ncase=0) == TP_ERR_ARG and sens(ncase=-1) == TP_ERR_ARG and sens(ncase=9, V=eight) == TP_ERR_ARG
    assert sens(ncase=2, V=nul) == TP_ERR_ARG
    for bad in (nan, inf, -inf):
        assert sens(scale=bad) == TP_ERR_ARG
    assert sens() == TP_ERR_STATE and sens(ncase=8, V=eight) == TP_ERR_STATE

    # the two block calls: NULL, q and the overlap are refused before the grid (here: NULL, or a zeroed block) is looked at
    out = (C.c_double * 64)()
    buf = C.create_string_buffer(8 * 64)
    base = C.cast(buf, C.c_void_p).value
    Y = (C.c_void_p * 2)(base, base + 8 * 16)
    Z = (C.c_void_p * 2)(base + 8 * 32, base + 8 * 48)
    Q = (C.c_double * 4)(1.0, 0.0, 0.0, 1.0)
    g = e
    assert L.tp_vec_block_gram(None, 2, Y, Y, 16, out) == TP_ERR_ARG
    assert L.tp_vec_block_gram(g, 2, None, Y, 16, out) == TP_ERR_ARG and L.tp_vec_block_gram(g, 2, Y, None, 16, out) == TP_ERR_ARG
    assert L.tp_vec_block_gram(g, 2, Y, Y, 16, None) == TP_ERR_ARG
    assert L.tp_vec_block_gram(g, 0, Y, Y, 16, out) == TP_ERR_ARG and L.tp_vec_block_gram(g, 9, Y, Y, 16, out) == TP_ERR_ARG
    assert L.tp_vec_block_gram(g, 2, nul, Y, 16, out) == TP_ERR_ARG and L.tp_vec_block_gram(g, 2, Y, nul, 16, out) == TP_ERR_ARG
    assert L.tp_vec_block_combine(None, 2, Y, Q, Z, 16) == TP_ERR_ARG
    assert L.tp_vec_block_combine(g, 2, None, Q, Z, 16) == TP_ERR_ARG and L.tp_vec_block_combine(g, 2, Y, None, Z, 16) == TP_ERR_ARG
    assert L.tp_vec_block_combine(g, 2, Y, Q, None, 16) == TP_ERR_ARG
    assert L.tp_vec_block_combine(g, 0, Y, Q, Z, 16) == TP_ERR_ARG and L.tp_vec_block_combine(g, 9, Y, Q, Z, 16) == TP_ERR_ARG
    assert L.tp_vec_block_combine(g, 2, nul, Q, Z, 16) == TP_ERR_ARG
    assert L.tp_vec_block_combine(g, 2, Y, Q, Y, 16) == TP_ERR_ARG                                    # Z is Y
    Zo = (C.c_void_p * 2)(base + 8 * 32, base + 8 * 24)                                              # Z_1 reaches into Y_1
    assert L.tp_vec_block_combine(g, 2, Y, Q, Zo, 16) == TP_ERR_ARG
    Zz = (C.c_void_p * 2)(base + 8 * 32, base + 8 * 40)                                              # Z_1 reaches into Z_0
    assert L.tp_vec_block_combine(g, 2, Y, Q, Zz, 16) == TP_ERR_ARG


def test_driver_has_the_frequency_fields_and_refuses_bad_values():
    from topopt_in_petsc_amd.api import LinearElasticity
    from topopt_in_petsc_amd.driver import TopOpt
    f = {d.name: d.default for d in dataclasses.fields(TopOpt)}
    assert f["frequency_limit"] is None and f["frequency_modes"] == 3 and f["frequency_rho"] == 1.0
    assert f["frequency_xlow"] == 0.1 and f["frequency_tol"] == 1e-6
    for name in ("MassAssemble", "MassMult", "MassSensitivity", "Eigenmodes", "EigenVectors", "EigenSensitivity"):
        assert callable(getattr(LinearElasticity, name))
    nan = float("nan")
    for kw in (dict(frequency_limit=0.0), dict(frequency_limit=-1.0), dict(frequency_limit=nan),
               dict(frequency_limit=1.0, frequency_rho=0.0), dict(frequency_limit=1.0, frequency_rho=-2.0),
               dict(frequency_limit=1.0, frequency_modes=7), dict(frequency_limit=1.0, frequency_modes=0),
               dict(frequency_limit=1.0, frequency_xlow=1.0), dict(frequency_limit=1.0, frequency_tol=0.0)):
        with pytest.raises(ValueError):      # before the grid is made: no device needed
            TopOpt(**kw)


def test_m8_sums():
    M = ref.m8(LD)
    ulp = float(np.finfo(LD).eps)
    print("M8 row sums - 1/8: %s; sum - 1: %.3e" % (" ".join("%.1e" % float(v - LD(1) / 8) for v in M.sum(axis=1)), float(M.sum() - 1)))
    assert float(np.abs(M.sum(axis=1) - LD(1) / 8).max()) <= 4 * ulp and float(abs(M.sum() - 1)) <= 8 * ulp
    assert np.array_equal(M, M.T)
    vals = sorted(set(np.round(np.asarray(M, dtype=np.float64) * 216).astype(int).ravel()))
    assert vals == [1, 2, 4, 8]        # 1/216, 1/108, 1/54, 1/27


@pytest.mark.parametrize("ne,h", [((3, 2, 2), (1.0, 0.5, 0.25)), ((6, 4, 4), (0.1, 0.1, 0.05)), ((20, 12, 8), (0.05, 0.04, 0.03))])
def test_total_mass(ne, h):
    """1^T M 1 = 3 rho0 V_e sum m(x_e) to 1e-15 relative, in 80-bit arithmetic, for the free mass matrix (before N)"""
    nnode, rho0 = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1), 2.5
    x = ref.design_mixed(ne, 3)
    y = ref.mass_apply(x, ref.elem_dofs(*ne), nnode, h, rho0, ref.X_LOW, np.ones(3 * nnode), np.ones(3 * nnode), LD)
    tot = 3 * LD(rho0) * ref.volume(h) * ref.mass(x, ref.X_LOW).sum()
    err = float(abs(y.sum() / tot - 1))
    print("%s: 1^T M 1 = %.15e, off by %.3e (bound 1e-15)" % ("x".join(map(str, ne)), float(y.sum()), err))
    assert err <= 1e-15


def test_mass_matrix_is_symmetric_positive_definite():
    ne, h = (3, 2, 2), (1.0, 0.5, 0.25)
    M = ref.assemble_M(ne, h, ref.design_mixed(ne, 4), 1.0, ref.X_LOW).toarray()
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    print("3x2x2: max|M - M^T| = %.3e, eigenvalues from %.3e to %.3e" % (np.abs(M - M.T).max(), ev.min(), ev.max()))
    assert np.abs(M - M.T).max() <= 1e-18 and ev.min() > 0


def _fd_case(orc, ne, h, x, nev, seed):
    eps = 1e-6
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], 0.3)).reshape(24, 24)
    N = ref.cantilever_N(*ne)
    W = np.random.default_rng(seed).uniform(-1.0, 1.0, x.size)
    pen = lambda xv: ref.Pencil(ne, h, KE, xv, N, ref.EMIN, ref.EMAX, ref.PENAL, ref.RHO0, ref.X_LOW)
    P = pen(x)
    lam, Phi = P.eigh(nev + 1)
    an = float((P.dJ(lam, Phi, nev) * W).sum())
    stiff_only = float((P.dJ(lam, Phi, nev, mass_term=False) * W).sum())
    fd = float((pen(x + eps * W).J(nev) - pen(x - eps * W).J(nev)) / (2 * LD(eps)))
    return lam, an, stiff_only, fd


def test_restated_gradient_against_central_differences(orc):
    """6x4x4, h = (0.1, 0.1, 0.05), Emin 1e-3, densities uniform(0.05, 1) (both branches of m), nev = 3: dJ/dx . W against central
    differences of J, eps = 1e-6, bound 1e-6"""
    ne, h = (6, 4, 4), (0.1, 0.1, 0.05)
    x = np.random.default_rng(17).uniform(0.05, 1.0, ne[0] * ne[1] * ne[2])
    assert (x < ref.X_LOW).any() and (x > ref.X_LOW).any()
    lam, an, stiff_only, fd = _fd_case(orc, ne, h, x, 3, 18)
    err = abs(an / fd - 1)
    print("lambda %s; dJ/dx . W = %.12e, central difference %.12e, off by %.3e (bound 1e-6); without the mass term off by %.3e"
          % (" ".join("%.6e" % v for v in lam), an, fd, err, abs(stiff_only / fd - 1)))
    assert lam[3] / lam[2] - 1 >= 0.05
    assert err <= 1e-6
    assert abs(stiff_only / fd - 1) > 1e-4          # the stiffness term alone is not the derivative


def test_restated_gradient_through_a_double_eigenvalue(orc):
    """the square-section 6x4x4 cube mesh at uniform density, nev = 2: the double bending mode lies whole inside the sum, J is
    differentiable although neither eigenvalue is"""
    ne, h = (6, 4, 4), (0.25, 0.25, 0.25)
    x = np.full(ne[0] * ne[1] * ne[2], 0.5)
    lam, an, stiff_only, fd = _fd_case(orc, ne, h, x, 2, 19)
    err = abs(an / fd - 1)
    print("lambda %s (pair apart by %.1e); dJ/dx . W = %.12e, central difference %.12e, off by %.3e (bound 1e-6); without the mass term off by %.3e"
          % (" ".join("%.9e" % v for v in lam), lam[1] / lam[0] - 1, an, fd, err, abs(stiff_only / fd - 1)))
    assert lam[1] / lam[0] - 1 < 1e-8 and lam[2] / lam[1] - 1 >= 0.05
    assert err <= 1e-6


@pytest.mark.parametrize("name", sorted(ref.EIGEN_CASES) + sorted(ref.SLAB_CASES))
def test_conditions_of_the_gpu_cases(orc, name):
    """conditions, not measurements: the gap behind the sum, separated or truly clustered modes inside it, both branches of m"""
    c = {**ref.EIGEN_CASES, **ref.SLAB_CASES}[name]
    ne, h, nev = c["ne"], c["h"], c["nev"]
    x = c["design"](ne, c["seed"])
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], 0.3)).reshape(24, 24)
    lam = ref.Pencil(ne, h, KE, x, ref.cantilever_N(*ne), ref.EMIN, ref.EMAX, ref.PENAL, ref.RHO0, ref.X_LOW).eigh(nev + 1)[0]
    steps = lam[1:] / lam[:-1] - 1
    below = float((x < ref.X_LOW).mean())
    print("%s: lambda %s, steps %s, %.0f %% of the elements below x_low" % (name, " ".join("%.6e" % v for v in lam),
                                                                         " ".join("%.3e" % v for v in steps), 100 * below))
    assert steps[nev - 1] >= 0.05
    assert all(s >= 0.05 or s < 1e-8 for s in steps[:nev - 1])
    assert below >= 0.25 and 1.0 - below >= 0.25


@pytest.mark.parametrize("idx", range(len(ref.KERNEL_MESHES)))
def test_designs_of_the_kernel_meshes_meet_both_branches(idx):
    ne, _ = ref.KERNEL_MESHES[idx]
    x = ref.design_mixed(ne, 20 + idx)
    below = float((x < ref.X_LOW).mean())
    assert below >= 0.25 and 1.0 - below >= 0.25
