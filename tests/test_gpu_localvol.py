"""Local volume constraint on the device (tp_localvol) against the numpy restatement in 80-bit arithmetic of
tests/localvol_ref.py, whose docstring carries the formulas.  With u = 2^-53, taps = (2 conn + 1)^3:

 2. rhobar: one chain of at most taps additions of non-negative terms <= 1 (the weights are 0 or 1: the fma rounds once, like the
    addition) and one division: |d| <= (taps + 8) u, relative and, rhobar being <= 1, absolute.  On a 0/1 field every partial sum
    is an integer below 2^53: exact, and rhobar is the one rounding of the division.
 3. pn, g, rhobar_max: the rhobar bound through x^p, pow and the reduction: p (taps + 8) u + 64 u relative; rhobar_max as rhobar.
 4. dgdx: the coefficient through t^(p-1), then a second chain: (p + 1) (taps + 8) u * 2 of its maximum.
 5. Euler's identity on the device's own outputs, sum rho dgdx = pn / alpha, to the bound of 4 times pn / alpha.

Every figure is printed with its bound before it is asserted.  The library reads its switches once per process, so the cases
that need one (the generic kernel, several outputs along z on a small mesh) run in a child process each."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import localvol_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = ref.LD
ALPHA = 0.6
# name: (elements, h, R, kernels of Filter.last_kernel the ball sum may run).  No centre distance ties with R: on the cubic
# meshes squared distances are integers in h^2; on b, 25 i^2 + 16 j^2 + 9 k^2 = 121 has no integer solution.
MESHES = {
    "a": ((16, 8, 8), (0.125, 0.125, 0.125), 2.5 * 0.125, {1, 2}),        # conn 2: tiled
    "b": ((20, 12, 8), (0.05, 0.04, 0.03), 0.11, {3}),                     # conn 3: wide; not tile-aligned, hx != hy != hz
    "c": ((20, 20, 20), (0.05, 0.05, 0.05), 9.5 * 0.05, {4}),              # conn 9: streamed ring, 8000 elements
}
MESH_D = ((3, 3, 3), (0.25, 0.25, 0.25), 1.5 * 0.25)                      # conn 1: generic fallback with tiling switched off


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _grid(tp, ne, h):
    return tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, tuple(h))


@pytest.mark.parametrize("p", [1.0, 16.0])
@pytest.mark.parametrize("kind", ["random", "checker", "half"])
@pytest.mark.parametrize("mesh", ["a", "b", "c"])
def test_counts_means_constraint_and_sensitivity_against_the_restatement(tp, mesh, kind, p):
    """checks 1 to 5"""
    ne, h, R, kernels = MESHES[mesh]
    ref.check_against_reference(tp, ne, h, R, kind, p, ALPHA, expect_kernel=kernels)


def _child(args, env_extra):
    e = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "localvol_worker.py"), "kernel"] + [str(a) for a in args], env=e,
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "kernel OK" in r.stdout, r.stdout[-3000:] + "\n" + r.stderr[-3000:]


def test_generic_kernel_on_3x3x3():
    """mesh d: every ball is truncated on every side; TP_NO_FILTER_TILE routes the ball sum to the generic loop (kernel 5)"""
    ne, h, R = MESH_D
    _child(ne + h + (R, "5"), dict(TP_NO_FILTER_TILE="1"))


@pytest.mark.parametrize("zm", [2, 4])
def test_several_outputs_along_z_on_mesh_a(zm):
    """the form large meshes take at conn 2 (kernel 2), forced on mesh a by TP_FILTER_ZMULTI"""
    ne, h, R, _ = MESHES["a"]
    _child(ne + h + (R, "2"), dict(TP_FILTER_ZMULTI=str(zm)))


@pytest.mark.parametrize("p", [1.0, 16.0])
@pytest.mark.parametrize("mesh", ["a", "b", "c"])
def test_uniform_field(tp, mesh, p):
    """check 6: rho = 0.12 gives g = 0.12 / alpha - 1 and sum dgdx = 1 / alpha, both to 1e-13"""
    ne, h, R, _ = MESHES[mesh]
    grid = _grid(tp, ne, h)
    try:
        lv = tp.LocalVolume(grid, R)
        x, dg = grid.elem_vec(0.12), grid.elem_vec()
        g, pn, mx = lv.Constraint(x, ALPHA, p, dgdx=dg)
        s = float(dg.cpu().numpy().astype(LD).sum())
        e_g, e_s = abs(g - (0.12 / ALPHA - 1)), abs(s - 1 / ALPHA)
        print("%s p=%g: g off by %.3e, sum dgdx off by %.3e (bounds 1e-13); rhobar_max %.17g" % (mesh, p, e_g, e_s, mx))
        assert e_g <= 1e-13 and e_s <= 1e-13
    finally:
        grid.close()


@pytest.mark.parametrize("p", [1.0, 16.0])
@pytest.mark.parametrize("mesh", ["a", "b"])
def test_sensitivity_against_central_differences_of_the_device(tp, mesh, p):
    """check 7: dgdx . W against (g(rho + eps W) - g(rho - eps W)) / (2 eps) of the device's own g, eps = 1e-6, relative 1e-6"""
    ne, h, R, _ = MESHES[mesh]
    n, eps = ne[0] * ne[1] * ne[2], 1e-6
    rng = np.random.default_rng(11)
    rho, W = rng.uniform(0.1, 0.9, n), rng.uniform(-1.0, 1.0, n)
    grid = _grid(tp, ne, h)
    try:
        lv = tp.LocalVolume(grid, R)
        dg = grid.elem_vec()
        lv.Constraint(_dev(rho), ALPHA, p, dgdx=dg)
        an = float((dg.cpu().numpy().astype(LD) * W).sum())
        gp = lv.Constraint(_dev(rho + eps * W), ALPHA, p)[0]
        gm = lv.Constraint(_dev(rho - eps * W), ALPHA, p)[0]
        fd = (gp - gm) / (2 * eps)
        err = abs(fd - an) / abs(an)
        print("%s p=%g: dgdx.W %.9e, central difference %.9e, off by %.3e (bound 1e-6)" % (mesh, p, an, fd, err))
        assert err <= 1e-6
    finally:
        grid.close()


def test_zero_field_and_nan(tp):
    """check 8: rho = 0 gives pn = 0, g = -1, dgdx = 0 without a NaN; a NaN in rho reaches g as NaN"""
    import torch
    ne, h, R, _ = MESHES["a"]
    grid = _grid(tp, ne, h)
    try:
        lv = tp.LocalVolume(grid, R)
        for p in (1.0, 16.0):
            dg, rb = grid.elem_vec(7.0), grid.elem_vec(7.0)
            g, pn, mx = lv.Constraint(grid.elem_vec(0.0), ALPHA, p, dgdx=dg, rhobar=rb)
            print("p=%g zero field: g %r pn %r max %r, dgdx in [%r, %r]" % (p, g, pn, mx, float(dg.min()), float(dg.max())))
            assert pn == 0.0 and g == -1.0 and mx == 0.0
            assert torch.equal(dg, torch.zeros_like(dg)) and torch.equal(rb, torch.zeros_like(rb))
            x = _dev(ref.field("random", ne))
            x[517] = float("nan")
            g, pn, mx = lv.Constraint(x, ALPHA, p, dgdx=dg)
            print("p=%g NaN at one element: g %r pn %r" % (p, g, pn))
            assert np.isnan(g) and np.isnan(pn)
    finally:
        grid.close()


def test_two_calls_give_the_same_bits(tp):
    """check 9"""
    import torch
    ne, h, R, _ = MESHES["b"]
    grid = _grid(tp, ne, h)
    try:
        lv = tp.LocalVolume(grid, R)
        x = _dev(ref.field("random", ne))
        out = []
        for _ in range(2):
            dg, rb = grid.elem_vec(), grid.elem_vec()
            out.append((lv.Constraint(x, ALPHA, 16.0, dgdx=dg, rhobar=rb), dg, rb))
        assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    finally:
        grid.close()


def test_argument_errors_leave_the_outputs_alone(tp):
    """check 10: p < 1, alpha <= 0, R <= 0 and a NULL handle are TP_ERR_ARG; nothing is written"""
    import torch
    ne, h, R, _ = MESHES["a"]
    grid = _grid(tp, ne, h)
    try:
        lv = tp.LocalVolume(grid, R)
        x, dg, rb = grid.elem_vec(0.3), grid.elem_vec(7.0), grid.elem_vec(7.0)
        for alpha, p in ((ALPHA, 0.999), (0.0, 16.0), (-0.5, 16.0), (ALPHA, float("nan"))):
            with pytest.raises(tp.TopOptError) as ei:
                lv.Constraint(x, alpha, p, dgdx=dg, rhobar=rb)
            assert ei.value.code == 1
        for bad_R in (0.0, -0.1):
            with pytest.raises(tp.TopOptError) as ei:
                tp.LocalVolume(grid, bad_R)
            assert ei.value.code == 1
        assert grid.L.tp_localvol_constraint(None, x.data_ptr(), ALPHA, 16.0, None, None, None, rb.data_ptr(), dg.data_ptr()) == 1
        assert grid.L.tp_localvol_mean(None, x.data_ptr(), rb.data_ptr()) == 1
        torch.cuda.synchronize()
        assert torch.equal(dg, torch.full_like(dg, 7.0)) and torch.equal(rb, torch.full_like(rb, 7.0))
    finally:
        grid.close()


EXISTING_KEYS = {"itr", "fx", "fx_scaled", "gx", "ch", "mnd", "time", "ksp_its", "ksp_rerr", "mma_inner"}


def test_driver_with_the_local_volume_constraint(tp):
    """check 11: 32x16x16, volfrac 0.5, local_volume 0.4, R = 3.5 h, p = 16, ten iterations"""
    h = 2.0 / 32
    kw = dict(nxyz=(33, 17, 17), volfrac=0.5, nlvls=3)
    t = tp.TopOpt(local_volume=0.4, local_volume_R=3.5 * h, local_volume_p=16.0, **kw)
    assert t.m == 2 and t.localvol.stencil_width == 3
    hist = [t.step() for _ in range(10)]
    print("gx_local:", " ".join("%.6f" % r["gx_local"] for r in hist))
    print("local_max:", " ".join("%.6f" % r["local_max"] for r in hist))
    print("gx:", " ".join("%.6f" % r["gx"] for r in hist))
    assert set(hist[0]) == EXISTING_KEYS | {"gx_local", "local_pnorm", "local_max"}
    assert abs(hist[0]["gx_local"] - (0.5 / 0.4 - 1)) <= 1e-12          # the start is uniform
    assert all(r["local_max"] <= 1.0 for r in hist)
    assert hist[-1]["gx_local"] < hist[0]["gx_local"]
    t.grid.close()
    t0 = tp.TopOpt(**kw)
    assert t0.m == 1 and t0.localvol is None and len(t0.dgdx) == 1
    assert set(t0.step()) == EXISTING_KEYS
    t0.grid.close()
    t2 = tp.TopOpt(local_volume=0.4, local_volume_R=3.5 * h, stress_limit=300.0, **kw)
    assert t2.m == 3 and len(t2.dgdx) == 3
    r = t2.step()
    print("volume %.6f, stress %.6f, local %.6f" % (r["gx"], r["gx_stress"], r["gx_local"]))
    assert abs(r["gx_local"] - 0.25) <= 1e-12 and r["gx_stress"] == r["stress_pnorm"] / 300.0 - 1.0
    # the order [volume, stress, local]: the local constraint's sensitivity is the third array (positive everywhere: a ball sum
    # of positive coefficients through the density filter), the stress sensitivity the second
    assert float(t2.dgdx[2].min()) > 0.0 and abs(float(t2.dgdx[2].sum()) - 1 / 0.4) <= 1e-9
    t2.grid.close()
