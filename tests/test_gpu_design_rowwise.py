"""The design-side kernel families on the device, every row held to its own scale (tests/design_rowwise.py: the scales, the
constants with their counts, the cases; tests/test_design_rowwise_oracle.py holds the float64 restatements to a quarter of each
constant on the CPU).  |got_i - ref_i| <= c eps scale_i for EVERY row i, rows of scale 0 bit for bit:

  overhang      xi, the stored a, w, p (Overhang.Coefficients) and three transposes, on four meshes x four builds, at the default
                parameters, at (20, 1e-3, 0.4) and at P = 20.5, on nine fields (but for the 16 cases of
                design_rowwise.OV_UNDECIDABLE, where roundings decide the branch at S_MIN), at TP_OVERHANG_CHUNK 1, 2, 4 and 8.  The `tail`
                field carries supporting cells at 1.0e-8, 1.2e-8 and 7e-9: without the floor on the support sum (csrc/overhang.h)
                the first two give w = inf and a non-finite transpose, the third loses its support term.
  casting       c, the stored q (Casting.Q) and three transposes, on six meshes x every draw x seven fields, the x draws at
                TP_CASTING_XFORM 1 and 0.
  local volume  rhobar and dgdx, each row relative to its own value, on the meshes a (tiled), b (wide), c (ring) x the four 0/1
                designs x p = 1, 16 (the three older fields: tests/test_gpu_localvol.py, same check); a ball of zeros gives exactly
                0.  The forms behind a latched switch -- generic on 3x3x3, several outputs along z on mesh a -- run the same
                assertions in their child processes (tests/localvol_worker.py calls
                localvol_ref.check_against_reference on the same fields; tests/test_gpu_localvol.py starts them).
  length scale  T and dg of both kinds on six meshes x seven fields at proj = 0, proj = 1 (beta 8) and proj = 1 at beta = 64; a
                row with m = 0 exactly is bit-zero in T.

The transposes are held to the 80-bit recursion on the DEVICE'S OWN exported coefficients; what the coefficients may be off by is
held separately.  Achieved on the MI355X, the largest c per family over all cases and forms (bound in brackets):

  overhang      xi 1.16 (32), a 1.01 (64), w 2.26 (64), p 1.95 (32; every subnormal p within one spacing: the device keeps float64
                subnormals), transposes 5.39 (128 .. 512), over the chunk lengths 1, 2, 4, 8
  casting       c 0.96 (16), q 2.29 (64), transposes 6.71 (128 .. 256), both x forms
  local volume  rhobar / dgdx, p = 1 and p = 16:  a 6.62 (256) / 9.41 (1024), 46.3 (8192);  b 9.09 (512) / 12.4 (2048), 56.7 (16384);
                c 40.8 (8192) / 56.5 (32768), 189 (262144) -- the older fields included (tests/test_gpu_localvol.py);
                generic on 3x3x3 (kernel 5) 2.47 (64) / 0.83 (256), 39.5 (2048);  several outputs along z on mesh a (kernel 2,
                TP_FILTER_ZMULTI 2 and 4 alike) 6.62 (256) / 9.41 (1024), 46.3 (8192): the child processes print them
  on slabs      the one-rank results the 2- and 3-slab runs equal bit for bit (16x8x8, 16x8x12; coefficients included):
                overhang xi 0.85, a 0.93, w 1.66, p 1.73, transposes 2.79; casting c 0.90, q 2.09, transposes 3.25;
                local volume rhobar 10.7 (512), dgdx 45.7 (16384)
  length scale  T 5.17 (64), dg 5.38 (64), the largest on mesh f (70 cells along x)

With ov_cell_fwd as it was (S != 0 instead of S >= S_MIN) the same library fails the `tail` and `blocks` cases of the overhang at xi
already -- the reference's floor moves Xi by 2e-8 there -- and stores w = inf on the planted cells: on the column x = (1e-8, 0.5, 0.5),
g = 1 it returned J^T g = (inf, 1.76e-4, 1.01e-4), on (7e-9, 0.5, 0.5) the first row as 1.0 where the 80-bit value without the
floor is 1.589; on the tail field of 16x12x20, "+z", 10 non-finite w and 44 non-finite rows of the transpose.

Every reference is computed once per case (functools.lru_cache in the helper) and left unchanged."""
import os

import numpy as np
import pytest

from tests import casting_ref as cref
from tests import design_rowwise as dr
from tests import lengthscale_ref as lsref
from tests import localvol_ref as lvref
from tests import overhang_ref as oref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


@pytest.fixture
def env():
    """sets environment switches that the library reads on every call and puts the environment back"""
    old = {}

    def set_env(name, value):
        old.setdefault(name, os.environ.get(name))
        os.environ[name] = str(value)
    yield set_env
    for name, v in old.items():
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = v


def _worst(best, got):
    for k, v in got.items():
        best[k] = max(best.get(k, 0.0), v)


@pytest.mark.parametrize("build", dr.OV_BUILDS)
@pytest.mark.parametrize("ne", dr.OV_MESHES)
def test_overhang_row_by_row(tp, env, ne, build):
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0 / ne[1])
    best = {}
    try:
        ov = tp.Overhang(grid, build)
        for pi, params in enumerate(dr.OV_PARAMS):
            ov.params(*params)
            for kind in dr.ov_fields(ne, build, pi):
                case = dr.ov_case(ne, build, kind, pi)
                first = None
                for chunk in dr.OV_CHUNKS:
                    env("TP_OVERHANG_CHUNK", chunk)
                    xi, gv = grid.elem_vec(), [oref.dev(v) for v in case["g"]]
                    ov.Forward(oref.dev(case["x"]), xi)
                    assert ov.last_chunk() == chunk
                    coef = ov.Coefficients()
                    ov.Adjoint(gv)
                    res = [v.cpu().numpy() for v in [xi] + list(coef) + gv]
                    # a chunk length whose every bit equals one already held is held; any other goes through the bounds itself
                    if first is None or not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, res)):
                        _worst(best, dr.ov_hold(case, res[0], res[1], res[2], res[3], res[4:], tag="chunk %d: " % chunk))
                    first = first or res
        print("overhang %s %s, largest achieved c (bound): xi %.2f (%g), a %.2f, w %.2f (%g), p %.2f (%g), transposes %.2f (%g)"
              % ("x".join(map(str, ne)), build, best["xi"], dr.C_OV_XI, best["a"], best["w"], dr.C_OV_COEF, best["p"], dr.C_OV_POW,
                 best["adj"], dr.c_ov_adj(case["nl"])))
    finally:
        grid.close()


def test_overhang_coefficients_need_a_forward_call(tp):
    grid = tp.Grid(4, 4, 4, 1.0 / 3)
    try:
        ov = tp.Overhang(grid, "+z")
        with pytest.raises(tp.TopOptError) as ei:
            ov.Coefficients()
        assert ei.value.code == 1
        ov.Forward(oref.dev(np.full(27, 0.5)), grid.elem_vec())
        a, w, p = (v.cpu().numpy() for v in ov.Coefficients())
        assert (a[:9] == 1).all() and (w[:9] == 0).all() and (p > 0).all()                      # layer 0: a = 1, w = 0
        ov.params(20.0, 1e-3, 0.4)
        with pytest.raises(tp.TopOptError):
            ov.Coefficients()
        cf = tp.Casting(grid, "+z")
        with pytest.raises(tp.TopOptError) as ei:
            cf.Q()
        assert ei.value.code == 1
        cf.Forward(oref.dev(np.full(27, 0.5)), grid.elem_vec())
        assert (cf.Q().cpu().numpy()[18:] == 1).all()                                        # the sweep's first layer
        cf.params(1e-5)
        with pytest.raises(tp.TopOptError):
            cf.Q()
    finally:
        grid.close()


@pytest.mark.parametrize("ne", dr.CAST_MESHES)
def test_casting_row_by_row(tp, env, ne):
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0 / ne[1])
    best = {}
    try:
        for draw in cref.draws(ne):
            cf = tp.Casting(grid, draw)
            for kind in dr.CAST_FIELDS:
                case = dr.cast_case(ne, draw, kind)
                for xform in (dr.CAST_XFORMS if "x" in draw else (1,)):
                    env("TP_CASTING_XFORM", xform)
                    c, gv = grid.elem_vec(), [cref.dev(v) for v in case["g"]]
                    cf.Forward(cref.dev(case["x"]), c)
                    assert cf.last_form() == (1 if "x" not in draw else 2 if xform else 3)
                    q = cf.Q()
                    cf.Adjoint(gv)
                    _worst(best, dr.cast_hold(case, c.cpu().numpy(), q.cpu().numpy(), [v.cpu().numpy() for v in gv], tag="xform %d: " % xform))
            cf.close()
        print("casting %s, largest achieved c (bound): c %.2f (%g), q %.2f (%g), transposes %.2f (up to %g)"
              % (cref.name(ne), best["c"], dr.C_CAST_C, best["q"], dr.C_CAST_Q, best["adj"], dr.c_cast_adj(max(ne))))
    finally:
        grid.close()


@pytest.mark.parametrize("p", dr.LV_PS)
@pytest.mark.parametrize("mesh,kernels", [("a", {1, 2}), ("b", {3}), ("c", {4})])
def test_local_volume_row_by_row(tp, mesh, kernels, p):
    """through the shared check: the present assertions and the row-wise ones, on the 0/1 designs (the older fields go through the
    same check in tests/test_gpu_localvol.py)"""
    ne, h, R = dr.LV_MESHES[mesh]
    for kind in dr.DESIGNS:
        got = lvref.check_against_reference(tp, ne, h, R, kind, p, dr.LV_ALPHA, expect_kernel=kernels)
        case = dr.lv_case(ne, h, R, kind, p, dr.LV_ALPHA)
        zero = case["ref"]["rb"] == 0
        assert not got["rb"][zero].any() and not got["dgdx"][case["ref"]["dgdx"] == 0].any()


@pytest.mark.parametrize("pj", range(len(dr.LS_PROJ)))
@pytest.mark.parametrize("mesh", sorted(dr.LS_MESHES))
def test_length_scale_row_by_row(tp, mesh, pj):
    ne, h = dr.LS_MESHES[mesh]
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, tuple(h))
    best = {}
    try:
        ls = tp.LengthScale(grid)
        for kind in dr.LS_FIELDS:
            case = dr.ls_case(mesh, kind, pj)
            dgs, dgv = grid.elem_vec(7.0), grid.elem_vec(7.0)
            ls.Constraints(oref.dev(case["rt"]), oref.dev(case["rb"]), case["c"], dr.LS_ETA_S, dr.LS_ETA_V, dr.LS_EPS, "both",
                           bool(case["proj"]), case["beta"], lsref.ETA, dg_solid=dgs, dg_void=dgv)
            ts, tv = ls.Terms()
            for name, T, dg in (("solid", ts, dgs), ("void", tv, dgv)):
                _worst(best, dr.ls_hold(case, name, T.cpu().numpy(), dg.cpu().numpy()))
        print("length scale %s proj=%d beta=%g, largest achieved c (bound): T %.2f (%g), dg %.2f (%g)"
              % (mesh, case["proj"], case["beta"], best["T"], dr.C_LS_T, best["dg"], dr.C_LS_DG))
    finally:
        grid.close()
