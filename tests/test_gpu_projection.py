"""The Heaviside projection (k_heaviside), its chain rule (k_heaviside_chain through k_robust_chain, bit-equal to it:
tests/test_gpu_robust.py), GetMND (k_mnd) and the PETSc quotient (k_pw_div, and the cone kernels' divisions through the sensitivity
filter) held row by row against 80-bit values at exact 0, -0.0, 1, at the threshold and next to it, where a tanh changes method or
saturates, from beta = 0.1 to 64, from one element to fields whose grid-stride loops take a second trip.

Rows, scales and constants: tests/projection_ref.py (the constants come from the operation counts and the CPU's float64 figures,
tests/test_projection_oracle.py, never from what the kernels achieve).  ACHIEVED on the MI355X, for the reader (units of 2^-53 x
the row's scale; largest over all cases and sizes):

    projection alone, n = 1 .. 531 441       bound 64     4.0 at every size (the CPU's float64 figure too: there it is the row
                                                          x = the smallest normal number at beta = 0.1, eta = 0, beta x subnormal)
    y(0), y(-0.0)                                         exactly 0.0 in all 30 cases at every size
    chain alone, n = 1 .. 531 441            bound 64     2.59 / 2.53 / 2.76 / 2.50 / 2.45 / 2.96 / 3.20
    chain composed with the cone filter      c_filter(ElemConn) + 64
        12x8x8, ElemConn 2, types 1 / 0      bound 320    0.016 / 0.029
        26x22x20, ElemConn 2, types 1 / 0    bound 320    0.023 / 0.028
        26x22x20, ElemConn 5, types 1 / 0    bound 4160   0.013 / 0.018
    GetMND, random field, n = 1 / 255 / 257  bound 32     0.088 / 1.12 / 2.25
        n = 2 113 536                        bound 64     0.17
    GetMND, 0/1 and all 0.5                               exactly 0 and exactly 1 at every size
    VecPointwiseDivide, n = 1 .. 524 289                  bit for bit
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import projection_ref as pr
from tests import rowwise as rw

pytestmark = pytest.mark.gpu
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ld(a):
    return np.ascontiguousarray(a, dtype=LD)


def _mesh(tp, elems):
    """(grid, sensitivity filter of stencil width 0) on a mesh of ex x ey x ez elements"""
    ex, ey, ez = elems
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0)
    assert grid.n_own_elems == ex * ey * ez
    return grid, tp.Filter(grid, 0, 0.5)


def _fields(n, beta, eta):
    """the fields of one size: one, or for the one-element mesh every salt in turn"""
    return [pr.field(n, beta, eta, s) for s in range(len(pr.salts(beta, eta)) if n == 1 else 1)]


# ---- the projection alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(pr.SIZES))
def test_projection_rows(tp, n):
    """FilterProject of a sensitivity filter whose x and xTilde are one tensor (the projection kernel alone runs), every case of
    projection_ref.CASES: every row within C_FORWARD of the 80-bit value; 0 <= y <= 1; y(1) == 1 exactly (numerator and den are the
    same expression there); y(0) and y(-0.0) non-negative (a negative xPhys under a fractional penal is NaN); y non-decreasing over
    the sorted field with a slack of 8 eps"""
    import torch
    grid, flt0 = _mesh(tp, pr.SIZES[n])
    try:
        worst, zero_exact, zero_max = 0.0, True, 0.0
        for beta, eta in pr.CASES:
            for x in _fields(n, beta, eta):
                xT = dev(x)
                keep = xT.clone()
                out = torch.full_like(xT, float("nan"))
                flt0.FilterProject(xT, xT, out, True, beta, eta)
                assert torch.equal(xT.view(torch.int64), keep.view(torch.int64)), "xTilde was written"
                y = host(out)
                what = "projection n=%d beta=%g eta=%g" % (n, beta, eta)
                worst = max(worst, rw.assert_rowwise(y, pr.H(x, beta, eta, LD), pr.scale_forward(x, beta, eta), pr.C_FORWARD,
                                                     {"label": what, "dims": (n, 1, 1), "dof": 0}))
                assert (y >= 0.0).all() and (y <= 1.0).all(), what + ": outside [0, 1]"
                assert (y[x == 1.0] == 1.0).all(), what + ": y(1) != 1"
                y0 = y[x == 0.0]      # both zeros
                assert (y0 >= 0.0).all() and not np.signbit(y0[y0 != 0]).any(), what + ": y(0) negative"
                if y0.size:
                    zero_exact, zero_max = zero_exact and bool((y0 == 0.0).all()), max(zero_max, float(y0.max()))
                o = np.argsort(x, kind="stable")
                assert (np.diff(y[o]) >= -pr.MONOTONE_SLACK).all(), what + ": not monotone, largest drop %.3e" % float(-np.diff(y[o]).min())
        print("ACHIEVED projection n=%d: %.3g of %g; y(0), y(-0.0) exactly 0 in every case: %s (largest %.3e)" % (n, worst, pr.C_FORWARD, zero_exact, zero_max))
    finally:
        grid.close()


# ---- the chain alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(pr.SIZES))
def test_chain_rows(tp, n):
    """Robust.Chain with one row (k_robust_chain, bit-equal to k_heaviside_chain), the same sizes, cases and fields, df of mixed signs
    with exact zeros: every row within C_CHAIN of the 80-bit product df H'(x); a zero of df stays a zero"""
    grid, _ = _mesh(tp, pr.SIZES[n])
    try:
        rb, worst = tp.Robust(grid), 0.0
        for beta, eta in pr.CASES:
            for seed, x in enumerate(_fields(n, beta, eta)):
                df = pr.rows(n, seed)
                row = dev(df)
                rb.Chain(dev(x), beta, [row], [eta])
                got = host(row)
                what = "chain n=%d beta=%g eta=%g" % (n, beta, eta)
                worst = max(worst, rw.assert_rowwise(got, pr.chain(df, x, beta, eta, LD), pr.scale_chain(df, x, beta, eta), pr.C_CHAIN,
                                                     {"label": what, "dims": (n, 1, 1), "dof": 0}))
                assert (got[df == 0] == 0).all(), what
        print("ACHIEVED chain n=%d: %.3g of %g" % (n, worst, pr.C_CHAIN))
    finally:
        grid.close()


# ---- the chain composed with the filter -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh,rfac", [((12, 8, 8), 2.56), (rw.FILTER_MESH, 2.56), (rw.FILTER_MESH, 5.12)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "r%g" % v)
def test_chain_composed_with_the_filter(tp, arb, mesh, rfac):
    """Filter.Gradients(.., True, 48, eta), density and sensitivity filter, against the arbiter's Filter.gradient with projection.
    xTilde is the salted field of (48, eta), x a design with exact zeros and ones.  Scale: the chain's scale pushed through
    rw.Cone.scale_gradient; an error of C_CHAIN eps of it on every entry passes the non-negative weights unchanged and the filter adds
    c_filter(ElemConn) eps of the same majorant: the bound is their sum.  Sensitivity filter: the rows with x_i = 0 are exactly 0.0"""
    ex, ey, ez = mesh
    n, h, beta = ex * ey * ez, 1.0 / ey, 48.0
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    try:
        af = arb.Filter(ex + 1, ey + 1, ez + 1, h, rfac * h)
        cone = rw.Cone(ex, ey, ez, h, rfac * h, af.conn)
        c = rw.c_filter(af.conn) + pr.C_CHAIN
        r = np.random.default_rng(n).random(n)
        x = np.where(r < 0.2, 0.0, np.where(r > 0.8, 1.0, 1e-3 + (1.0 - 1e-3) * r))
        for ftype in (1, 0):
            f = tp.Filter(grid, ftype, rfac * h)
            assert f.ElemConn == af.conn
            for eta in (0.3, 0.5, 0.7):
                xT, df0 = pr.field(n, beta, eta), pr.rows(n, int(10 * eta))
                df = dev(df0)
                f.Gradients(dev(x), dev(xT), df, [], True, beta, eta)
                got = host(df)
                ga = af.gradient(ftype, ld(x), ld(xT), ld(df0), True, beta, eta)
                s = cone.scale_gradient(ftype, x, pr.scale_chain(df0, xT, beta, eta))
                what = "chain + filter type %d %s rfac %g ElemConn %d eta %g" % (ftype, "x".join(map(str, mesh)), rfac, af.conn, eta)
                if ftype == 0:
                    assert (got[x == 0] == 0).all() and not np.signbit(got[x == 0]).any(), what + ": a row with x = 0 is not 0.0"
                    s = np.where(x == 0, 0.0, s)
                a = rw.assert_rowwise(got, ga, s, c, {"label": what, "dims": mesh, "dof": 0})
                print("ACHIEVED %s: %.3g of %g" % (what, a, c))
            f.close()
    finally:
        grid.close()


# ---- GetMND -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(pr.MND_SIZES))
def test_mnd(tp, n):
    """0/1 gives exactly 0, all 0.5 exactly 1, a random field lies within c_mnd(n) eps sum|terms| / n of the 80-bit sum; the largest
    size is past 8192 x 256 elements, where the launch is capped and every thread takes a second trip"""
    grid, flt0 = _mesh(tp, pr.MND_SIZES[n])
    try:
        for name, (x, exact) in pr.mnd_fields(n).items():
            got = flt0.GetMND(dev(x))
            if exact is not None:
                assert got == exact, (n, name, got)
                continue
            ref, bound = pr.mnd(x, LD), pr.c_mnd(n) * pr.EPS * float(np.abs(pr.mnd_terms(x, LD)).sum()) / n
            off = abs(float(LD(got) - ref))
            print("ACHIEVED GetMND n=%d: |got - 80-bit sum| = %.3e = %.3g of %g eps sum|terms| / n" % (n, off, off / bound * pr.c_mnd(n), pr.c_mnd(n)))
            assert off <= bound, (n, got, float(ref), off, bound)
    finally:
        grid.close()


# ---- the shim's VecPointwiseDivide ------------------------------------------------------------------------------------------

def _shim():
    from tests.test_cpp_host import _build
    _build()
    L = C.CDLL(os.path.join(ROOT, "topopt_in_petsc_amd", "libtopopt_petsc_shim.so"))
    vp, d = C.c_void_p, C.c_double
    L.DMDACreate3d.argtypes = [C.c_int] * 5 + [C.c_int] * 8 + [vp, vp, vp, C.POINTER(vp)]
    L.DMDASetUniformCoordinates.argtypes = [vp] + [d] * 6
    L.DMCreateGlobalVector.argtypes = L.VecDuplicate.argtypes = [vp, C.POINTER(vp)]
    L.VecGetSize.argtypes = [vp, C.POINTER(C.c_int)]
    L.VecGetArray.argtypes = L.VecRestoreArray.argtypes = [vp, C.POINTER(C.POINTER(d))]
    L.VecPointwiseDivide.argtypes = [vp, vp, vp]
    L.VecDestroy.argtypes = L.DMDestroy.argtypes = [C.POINTER(vp)]
    return L


@pytest.mark.parametrize("n", list(pr.DIVIDE_SIZES))
def test_shim_pointwise_divide_with_zero_denominators(n):
    """VecPointwiseDivide of the PETSc-named adapter (k_pw_div) on element vectors of n = 1 .. 524 289 entries (one entry in the
    grid-stride loop's second trip) with +0.0, -0.0 and 0 / 0 among the denominators: 0 there, the correctly rounded quotient
    elsewhere, bit for bit against numpy; w = x as well (Filter.cc:70 divides in place)"""
    L = _shim()
    vp, d = C.c_void_p, C.c_double
    ex, ey, ez = pr.DIVIDE_SIZES[n]
    da, de, x, y, w = vp(), vp(), vp(), vp(), vp()
    assert L.DMDACreate3d(0, 0, 0, 0, 1, ex + 1, ey + 1, ez + 1, -1, -1, -1, 3, 1, None, None, None, C.byref(da)) == 0
    assert L.DMDASetUniformCoordinates(da, 0, 1, 0, 1, 0, 1) == 0
    assert L.DMDACreate3d(0, 0, 0, 0, 1, ex, ey, ez, -1, -1, -1, 1, 1, None, None, None, C.byref(de)) == 0
    try:
        assert L.DMCreateGlobalVector(de, C.byref(x)) == 0 and L.VecDuplicate(x, C.byref(y)) == 0 and L.VecDuplicate(x, C.byref(w)) == 0
        size = C.c_int()
        L.VecGetSize(x, C.byref(size))
        assert size.value == n
        rng = np.random.default_rng(n)
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        b[::3], b[1::7], a[::6] = 0.0, -0.0, 0.0
        b[-1] = 0.0                       # the last entry: at 524 289 the one of the second trip
        a[-1] = 1.0

        def put(v, src):
            p = C.POINTER(d)()
            assert L.VecGetArray(v, C.byref(p)) == 0
            np.ctypeslib.as_array(p, shape=(n,))[:] = src
            assert L.VecRestoreArray(v, C.byref(p)) == 0

        def get(v):
            p = C.POINTER(d)()
            assert L.VecGetArray(v, C.byref(p)) == 0
            out = np.ctypeslib.as_array(p, shape=(n,)).copy()
            assert L.VecRestoreArray(v, C.byref(p)) == 0
            return out

        put(x, a), put(y, b), put(w, np.full(n, np.nan))
        want = pr.petsc_div(a, b)
        assert (want[b == 0] == 0).all() and np.isfinite(want).all()
        assert L.VecPointwiseDivide(w, x, y) == 0
        assert np.array_equal(get(w).view(np.int64), want.view(np.int64)), "w = x / y"
        assert L.VecPointwiseDivide(x, x, y) == 0
        assert np.array_equal(get(x).view(np.int64), want.view(np.int64)), "x = x / y in place"
    finally:
        for v in (x, y, w):
            if v:
                L.VecDestroy(C.byref(v))
        L.DMDestroy(C.byref(de))
        L.DMDestroy(C.byref(da))


# ---- the driver -------------------------------------------------------------------------------------------------------------

def test_driver_sensitivity_filter_survives_designs_on_their_bounds(tp):
    """TopOpt(filter=0) on 8 x 8 x 4 elements with a passive void block, three iterations from a design that sits on its lower bound
    Xmin = 0 on 32 active elements (what MMA returns sooner or later): every record value and x finite, the void elements at Xmin,
    the elements on the bound stay there, fx falls.

    The sensitivity filter divides by x.  Before the quotient followed PETSc's rule (0 where the denominator is 0) the rows of the
    elements at 0 were -inf or NaN, and this run ended in NaN: MMA's first update returned a NaN design (measured with the previous
    library: x and mnd are NaN after iteration 1).  The passive void elements alone do not show it -- their rows are divided by 0 as
    well, but Gather drops them before MMA -- and from the uniform start no active element reaches 0 within three iterations
    (measured: that run is finite with the previous library too), hence the start on the bound."""
    import torch
    from topopt_in_petsc_amd.api import passive_labels
    nxyz, xc = (9, 9, 5), (0.0, 1.0, 0.0, 1.0, 0.0, 0.5)
    shapes = [("void", "box", (0.375, 0.625, 0.375, 0.625, 0.0, 0.5))]
    t = tp.TopOpt(nxyz=nxyz, xc=xc, nlvls=2, rmin=0.2, volfrac=0.3, filter=0, passive=shapes)
    try:
        lab = torch.from_numpy(passive_labels(nxyz, xc, shapes)).cuda()
        assert int((lab == 1).sum()) == 2 * 2 * 4 and t.Xmin == 0.0
        k, j, i = np.meshgrid(np.arange(4), np.arange(8), np.arange(8), indexing="ij")
        low = torch.from_numpy(((i >= 6) & (k >= 2)).reshape(-1)).cuda()       # the free end's upper half: 2 x 8 x 2 elements
        assert int(low.sum()) == 32 and not bool((low & (lab != 0)).any())
        t.x[low] = t.Xmin
        t.regions.Gather([t.x], [t.xa])
        t.xold.copy_(t.xa)
        t._filter_project()
        for _ in range(3):
            rec = t.step()
            print("itr %d: fx %r gx %r ch %r mnd %r, smallest active x %r, active elements at 0: %d"
                  % (rec["itr"], rec["fx"], rec["gx"], rec["ch"], rec["mnd"], float(t.x[lab == 0].min()), int(((t.x == 0) & (lab == 0)).sum())))
            for key, v in rec.items():
                if isinstance(v, float):
                    assert np.isfinite(v), (rec["itr"], key, v)
            assert bool(torch.isfinite(t.x).all()) and bool(torch.isfinite(t.xPhys).all()), rec["itr"]
            assert bool((t.x[lab == 1] == t.Xmin).all()) and bool((t.xPhys[lab == 1] == 0.0).all())
            assert bool((t.x[low] == 0.0).all()), "an element on the bound, whose filtered sensitivity is 0, moved"
        fx = [r["fx"] for r in t.history]
        assert fx[-1] < fx[0], fx
    finally:
        t.grid.close()
