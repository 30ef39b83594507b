"""The rest of the reference optimizer's public surface on the device (MMA.h:29-140): KKTresidual, SetAsymptotes,
SetRobustAsymptotesType, ConstraintModification and the a/c/d constructors -- C ABI, Python binding, C++ mirror,
against the oracle, a numpy restatement of GenSub and the reference's own MMA class."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MMA = os.path.join(ROOT, "oracle", "_ref", "ref_mma")
NEW = ["tp_mma_set_subproblem", "tp_mma_set_asymptotes", "tp_mma_set_robust_asymptotes_type",
       "tp_mma_constraint_modification", "tp_mma_kkt_residual"]
METHODS = ["SetAsymptotes", "SetRobustAsymptotesType", "ConstraintModification", "KKTresidual"]


# ---------------------------------------------------------------------------------------------------------- CPU
def test_new_entry_points_are_declared_bound_and_exported():
    from topopt_in_petsc_amd import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "topopt_amd.h")).read(), flags=re.S)
    dll = ctypes.CDLL(lib.build())
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in lib.SYMBOLS, name
        assert hasattr(dll, name), name


def test_python_mma_has_the_reference_methods():
    import inspect
    from topopt_in_petsc_amd.api import MMA
    for name in METHODS:
        assert callable(getattr(MMA, name, None)), name
    assert list(inspect.signature(MMA.KKTresidual).parameters) == ["self", "x", "dfdx", "gx", "dgdx", "xmin", "xmax"]
    assert list(inspect.signature(MMA.__init__).parameters)[-3:] == ["a", "c", "d"]


def test_host_mirror_compiles_the_reference_signatures(tmp_path):
    """code written against MMA.h's members compiles against host/topopt_host.h"""
    src = tmp_path / "snippet.cc"
    src.write_text(r'''
#include "topopt_host.h"
PetscErrorCode use(tp_grid *g, Vec x, Vec dfdx, Vec *dgdx, Vec xmin, Vec xmax) {
    PetscScalar a[1] = {0.0}, c[1] = {1000.0}, d[1] = {0.0}, gx[1] = {0.0}, norm2, normInf;
    MMA *mma = new MMA(g, 100, 1, x, a, c, d);
    PetscErrorCode ierr = mma->SetAsymptotes(0.2, 0.65, 1.05);
    ierr = mma->ConstraintModification(PETSC_TRUE);
    ierr = mma->SetRobustAsymptotesType(1);
    ierr = mma->Update(x, dfdx, gx, dgdx, xmin, xmax);
    ierr = mma->KKTresidual(x, dfdx, gx, dgdx, xmin, xmax, &norm2, &normInf);
    delete mma;
    return ierr;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "host"),
                        "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------- helpers
def _kkt_np(x, dfdx, gx, dgdx, xmin, xmax, lam, a, y, z):
    """MMA.cc:452-493 in numpy"""
    ri = dfdx.copy()
    for j in range(len(lam)):
        ri = ri + lam[j] * dgdx[j]
    mu_min = np.where((x < xmin + 1.0e-5) & (ri > 0.0), ri, 0.0)
    mu_max = np.where((x > xmax - 1.0e-5) & (ri < 0.0), -ri, 0.0)
    ri = ri + (-mu_min + mu_max)
    r2, r3 = mu_min * (x - xmin), mu_max * (xmax - x)
    n2 = float(np.sum(ri * ri) + np.sum(r2 * r2) + np.sum(r3 * r3))
    ni = float(max(np.abs(ri).max(), np.abs(r2).max(), np.abs(r3).max()))
    t = 0.0
    for j in range(len(lam)):
        t += lam[j] * (a[j] * z + y[j] - gx[j])
    return float(np.sqrt(n2 + t ** 2)), max(abs(t), ni)


def _box(x, xmin, xmax, g0=0):
    """ref_mma_driver.cc's box=1 pattern (torch, in place): every 5th variable with its box above x, every 5th below"""
    import torch
    gi = torch.arange(x.numel(), device=x.device) + g0
    below = (gi % 5 == 1) & (x + 0.1 <= 1.0)
    above = (gi % 5 == 3) & (x - 0.1 >= 0.0)
    xmin.copy_(torch.where(below, x + 0.01, torch.where(above, x - 0.1, xmin)))
    xmax.copy_(torch.where(below, x + 0.1, torch.where(above, x - 0.01, xmax)))


def _gensub_LU(k, x, xo1, xo2, L, U, xmin, xmax, asy=(0.5, 0.7, 1.2), robust=0):
    """the asymptotes of MMA.cc:532-591 (k < 3: csrc/mma.h's form of the VecAXPBYPCZ pair :533-536), numpy"""
    ai, ad, ainc = asy
    if k < 3:
        return (x + (-ai) * xmax) + ai * xmin, (x + ai * xmax) + (-ai) * xmin
    helpvar = (x - xo1) * (xo1 - xo2)
    gamma = np.where(helpvar < 0.0, ad, np.where(helpvar > 0.0, ainc, 1.0))
    L = x - gamma * (xo1 - L)
    U = x + gamma * (U - xo1)
    xmi = np.maximum(1.0e-5, xmax - xmin)
    if robust == 0:
        L = np.minimum(np.maximum(L, x - 10.0 * xmi), x - 0.01 * xmi)
        U = np.minimum(np.maximum(U, x + 0.01 * xmi), x + 10.0 * xmi)
        return L, U
    L = np.minimum(np.maximum(L, x - 100.0 * xmi), x - 1.0e-4 * xmi)
    U = np.minimum(np.maximum(U, x + 1.0e-4 * xmi), x + 100.0 * xmi)
    lo, hi = xmin - 1.0e-5, xmax + 1.0e-5
    below, above = x < lo, x > hi
    L = np.where(below, x - (hi - x) / 0.9, L)
    U = np.where(below, x + (hi - x) / 0.9, U)
    L = np.where(above, x - (x - lo) / 0.9, L)
    U = np.where(above, x + (x - lo) / 0.9, U)
    return L, U


def _synthetic(x, w, n):
    """ref_mma_driver.cc's problem on the device: f = sum a_i / (x_i + 0.1), g_j = sum w_ji x_i / n - (0.25 + 0.05 j)"""
    import torch
    i = torch.arange(n, dtype=torch.float64, device="cuda")
    a = 1.0 + 0.3 * torch.sin(0.37 * i)
    dfdx = (-a / ((x + 0.1) * (x + 0.1))).contiguous()
    dgdx = [(wj / n).contiguous() for wj in w]
    gx = [float((wj * x).sum() / n) - (0.25 + 0.05 * j) for j, wj in enumerate(w)]
    return dfdx, gx, dgdx


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3])
def test_kkt_residual_matches_the_oracle(orc, m):
    """KKTresidual after each of 8 updates, device vs orc_mma_kkt with the oracle in the device's summation order (lam
    bit-identical): normInf bit-equal, norm2 to 1e-13 (only the order of the sum differs).  Also before any Update."""
    import torch
    import topopt_in_petsc_amd as tp
    n = 12 * 8 * 8
    rng = np.random.default_rng(5)
    c = rng.random(n) + 0.1
    W = rng.random((m, n)) + 0.5
    W /= W.sum(axis=1, keepdims=True)
    vj = 0.3 * (1.0 + 0.05 * np.arange(m))
    grid = tp.Grid(13, 9, 9, 0.125)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x = np.full(n, 0.3)
    xd = dev(x)
    m_o, m_d = orc.MMA(x, m), tp.MMA(grid, xd, m)
    m_o.set_device_order()
    xmin_d, xmax_d = grid.elem_vec(), grid.elem_vec()
    for it in range(9):
        df = -c / x ** 2 * (10.0 / 2000.0)
        g = [float(W[j] @ x - vj[j]) for j in range(m)]
        dg = [W[j].copy() for j in range(m)]
        xmin, xmax = m_o.SetOuterMovelimit(1e-3, 1.0, 0.2, x)
        m_d.SetOuterMovelimit(1e-3, 1.0, 0.2, xd, xmin_d, xmax_d)
        if it > 0:
            x = m_o.Update(x, df, g, dg, xmin, xmax)
            m_d.Update(xd, dev(df), g, [dev(d) for d in dg], xmin_d, xmax_d)
            assert np.array_equal(xd.cpu().numpy(), x), it
            assert np.array_equal(np.asarray(m_d.state()[0]), m_o.state()[0]), it
        n2_o, ni_o = m_o.kkt(x, df, g, dg, xmin, xmax)
        n2_d, ni_d = m_d.KKTresidual(xd, dev(df), g, [dev(d) for d in dg], xmin_d, xmax_d)
        assert ni_d == ni_o, (it, ni_d, ni_o)
        assert abs(n2_d - n2_o) <= 1e-13 * n2_o, (it, n2_d, n2_o)


@pytest.mark.gpu
@pytest.mark.parametrize("robust,conmod", [(1, 0), (0, 1), (1, 1)])
def test_gensub_branches_match_a_restatement(robust, conmod):
    """L/U after every Update, read back through Restart, bit-equal to the numpy restatement of MMA.cc:532-591 on the
    box pattern (x outside its box on both sides), 6 updates so that k >= 3 three times; both re-centring cases of
    robust type 1 must actually occur.  With constraint modification the design differs from the run without."""
    import torch
    import topopt_in_petsc_amd as tp
    ex, ey, ez, m = 16, 8, 8, 2
    n = ex * ey * ez
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ey)
    i = torch.arange(n, dtype=torch.float64, device="cuda")
    w = [1.0 + 0.5 * torch.cos(0.11 * i * (j + 1)) for j in range(m)]

    def run(robust, conmod, check):
        x = torch.full((n,), 0.3, dtype=torch.float64, device="cuda")
        xmin, xmax = torch.zeros_like(x), torch.zeros_like(x)
        xo1, xo2, U, L = (torch.zeros_like(x) for _ in range(4))
        mma = tp.MMA(grid, x, m)
        mma.SetRobustAsymptotesType(robust)
        mma.ConstraintModification(bool(conmod))
        hits, xs = [0, 0], []
        for k in range(1, 7):
            dfdx, gx, dgdx = _synthetic(x, w, n)
            mma.SetOuterMovelimit(0.0, 1.0, 0.2, x, xmin, xmax)
            _box(x, xmin, xmax)
            mma.Restart(xo1, xo2, U, L)
            h = [t.cpu().numpy().copy() for t in (x, xo1, xo2, L, U, xmin, xmax)]
            mma.Update(x, dfdx, gx, dgdx, xmin, xmax)
            xs.append(x.cpu().numpy().copy())
            if not check:
                continue
            mma.Restart(xo1, xo2, U, L)
            Le, Ue = _gensub_LU(k, *h, robust=robust)
            assert np.array_equal(L.cpu().numpy(), Le), (k, np.abs(L.cpu().numpy() - Le).max())
            assert np.array_equal(U.cpu().numpy(), Ue), (k, np.abs(U.cpu().numpy() - Ue).max())
            if k >= 3:
                hits[0] += int((h[0] < h[5] - 1e-5).sum())
                hits[1] += int((h[0] > h[6] + 1e-5).sum())
        return hits, xs

    hits, xs = run(robust, conmod, True)
    print("elements below / above their box at k >= 3:", hits)
    assert hits[0] > 0 and hits[1] > 0
    if conmod:
        _, xs0 = run(robust, 0, False)
        assert any(not np.array_equal(a, b) for a, b in zip(xs, xs0))


@pytest.mark.gpu
def test_invalid_robust_type_falls_back_to_zero():
    """MMA.cc:378-382: an invalid type leaves type 0 (here: an error the caller sees)"""
    import torch
    import topopt_in_petsc_amd as tp
    grid = tp.Grid(9, 5, 5, 0.25)
    x = grid.elem_vec(0.3)
    mma = tp.MMA(grid, x, 1)
    with pytest.raises(tp.TopOptError):
        mma.SetRobustAsymptotesType(2)
    mma.SetRobustAsymptotesType(1)
    with pytest.raises(ValueError):
        tp.MMA(grid, x, 1, a=[1.0, 2.0])
    torch.cuda.synchronize()


_REF_CASES = [  # (id, tokens, m, slab ranks of the reference run)
    ("robust-box", ["robust=1", "box=1"], 1, 1),
    ("robust-box", ["robust=1", "box=1"], 3, 2),
    ("conmod", ["conmod=1"], 1, 2),
    ("conmod", ["conmod=1"], 3, 1),
    ("asym", ["asym=0.2,0.65,1.05"], 1, 1),
    ("asym", ["asym=0.2,0.65,1.05"], 3, 2),
    ("acd", ["a=1", "c=100", "d=1"], 2, 1),
    ("acd", ["a=1", "c=100", "d=1"], 2, 2),
    ("defaults", [], 1, 2),
    ("defaults", [], 3, 1),
]


GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_mma_settings")


@pytest.mark.gpu
@pytest.mark.parametrize("name,tokens,m,nproc", _REF_CASES, ids=["%s-m%d-np%d" % (c[0], c[2], c[3]) for c in _REF_CASES])
def test_settings_against_the_references_own_mma_class(name, tokens, m, nproc):
    """the REFERENCE's MMA.cc with these settings (host/ref_mma_driver.cc, kkt=1) and the device MMA with the same ones:
    the design of every iteration to 1e-9 (test_mma.py's bound), KKTresidual's two norms to 1e-10 relative.  The
    reference's results are the recorded ones of tests/golden/ref_mma_settings (make_ref_mma_settings.py) and, where
    oracle/_ref/ref_mma was built from this tree's driver, also a live run.
    With a = 1, c = 100 the elastic variable z is positive and the element terms vanish (the bound multipliers take up
    ri), so the norms are the term sum_j lam_j (a_j z + y_j - g_j) of MMA.cc:487-492 alone, i.e. lam and z themselves.
    The dual solver fixes those only to its stopping tolerance: two summation orders give the same design bit for bit
    but lam to ~1e-9 relative (the bound test_mma.py holds lam to).  That case is held to 5e-9 (measured: 1.5e-9)."""
    import sys
    import torch
    import topopt_in_petsc_amd as tp
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_ref_mma_settings import EX as ex, EY as ey, EZ as ez, ITERS as iters, case_id, run_ref_mma
    rec = np.load(os.path.join(GOLDEN, case_id(name, m, nproc) + ".npz"))
    assert list(rec["tokens"]) == tokens + ["kkt=1"]
    refs = [("recorded", rec["x"], rec["kkt"])]
    if os.path.exists(REF_MMA):
        xs_live, kkt_live = run_ref_mma(tokens, m, nproc)
        if kkt_live is not None:   # a ref_mma without the settings runs the defaults: nothing to compare
            refs.append(("live", xs_live, kkt_live))
    n = ex * ey * ez
    kv = dict(t.split("=") for t in tokens)
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ey)
    i = torch.arange(n, dtype=torch.float64, device="cuda")
    x = torch.full((n,), 0.3, dtype=torch.float64, device="cuda")
    xmin, xmax = torch.zeros_like(x), torch.zeros_like(x)
    acd = {k: float(kv[k]) for k in "acd" if k in kv}
    mma = tp.MMA(grid, x, m, **acd)
    if "asym" in kv:
        mma.SetAsymptotes(*[float(v) for v in kv["asym"].split(",")])
    mma.SetRobustAsymptotesType(int(kv.get("robust", 0)))
    mma.ConstraintModification(kv.get("conmod", "0") == "1")
    w = [1.0 + 0.5 * torch.cos(0.11 * i * (j + 1)) for j in range(m)]
    worst, worst_kkt, zs, share = {r[0]: 0.0 for r in refs}, {r[0]: 0.0 for r in refs}, [], 0.0
    for k in range(iters):
        dfdx, gx, dgdx = _synthetic(x, w, n)
        mma.SetOuterMovelimit(0.0, 1.0, 0.2, x, xmin, xmax)
        if kv.get("box") == "1":
            _box(x, xmin, xmax)
        mma.Update(x, dfdx, gx, dgdx, xmin, xmax)
        n2, ni = mma.KKTresidual(x, dfdx, gx, dgdx, xmin, xmax)
        lam, z, _ = mma.state()
        zs.append(z)
        cj = float(kv.get("c", 1000.0))
        t = sum(lam[j] * (float(kv.get("a", 0.0)) * z + max(0.0, lam[j] - cj) - gx[j]) for j in range(m))
        share = max(share, abs(t) / n2)
        xk = x.cpu().numpy()
        for what, xs_ref, kkt_ref in refs:
            worst[what] = max(worst[what], float(np.abs(xk - xs_ref[k]).max()))
            worst_kkt[what] = max(worst_kkt[what], abs(n2 / kkt_ref[k][0] - 1.0), abs(ni / kkt_ref[k][1] - 1.0))
    print("%s m=%d np=%d: worst |x - x_ref| %s, worst KKT relative %s, largest share of the lam term in norm2 %.3f, z %s"
          % (name, m, nproc, worst, worst_kkt, share, zs))
    for what, _, _ in refs:
        assert worst[what] <= 1e-9, (what, worst[what])
        assert worst_kkt[what] <= (5e-9 if "a" in kv else 1e-10), (what, worst_kkt[what])
    if "a" in kv:
        assert max(zs) > 0.0, zs


@pytest.mark.gpu
def test_kkt_residual_across_slab_ranks():
    """host/mma_probe (the C++ mirror) on 1 and on 2 slab ranks of one GPU.  Before the first Update (lam = 0) the
    inputs are bit-identical: normInf exactly, norm2 to 1e-13.  After updates lam carries the rank count's summation
    order in its last bits, so the norms agree to rounding (1e-9 relative)."""
    probe = os.path.join(ROOT, "host", "mma_probe")
    args = ["16", "8", "8", "3", "6", "robust=1", "box=1"]
    res = []
    for nproc in (1, 2):
        r = subprocess.run([os.path.join(ROOT, "host", "slabrun"), "-n", str(nproc), "--same-device", probe] + args,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res.append([tuple(float(v) for v in l.split()[3:5]) for l in r.stdout.splitlines() if l.startswith("MMA_PROBE kkt ")])
    one, two = res
    assert len(one) == len(two) == 7
    assert two[0][1] == one[0][1], (one[0], two[0])
    assert abs(two[0][0] - one[0][0]) <= 1e-13 * one[0][0], (one[0], two[0])
    for a, b in zip(one[1:], two[1:]):
        assert abs(b[0] / a[0] - 1.0) <= 1e-9 and abs(b[1] / a[1] - 1.0) <= 1e-9, (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("m,tokens", [(4, []), (7, ["robust=1", "box=1"])], ids=["m4", "m7-robust-box"])
def test_many_constraints_across_slab_ranks(orc, tmp_path, m, tokens):
    """mma_reduce sends its m + m^2 sums through the comm hook 16 at a time: m = 4 (20 values, two chunks) and m = 7 (56
    values, four chunks) on 1, 2 and 3 slab ranks of one GPU, 16 x 8 x 12, host/mma_probe with dump=.  Against the
    one-rank run, slabs concatenated in rank order: every iteration's design to 1e-9, lam to 1e-9 of its largest entry
    (test_mma.py's form of the bound), both KKT norms to 1e-9 relative, and before the first Update normInf exactly and
    norm2 to 1e-13 -- the bounds the suite holds two summation orders of the same step to.  The one-rank run itself is held
    to the oracle in reference order at 1e-9, on the problem rebuilt in numpy (numpy's sin / cos against libm's in the last
    bit of the inputs: no bit-equality asked)."""
    from test_oracle_mma_settings import run_oracle_synthetic
    ex, ey, ez, iters = 16, 8, 12, 6
    n = ex * ey * ez
    probe = os.path.join(ROOT, "host", "mma_probe")
    runs = {}
    for nproc in (1, 2, 3):
        dump = str(tmp_path / ("x%d" % nproc))
        r = subprocess.run([os.path.join(ROOT, "host", "slabrun"), "-n", str(nproc), "--same-device", probe, str(ex), str(ey),
                            str(ez), str(m), str(iters)] + tokens + ["dump=" + dump], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (nproc, r.stdout[-2000:] + r.stderr[-2000:])
        lines = r.stdout.splitlines()
        kkt = np.array([[float(v) for v in l.split()[3:5]] for l in lines if l.startswith("MMA_PROBE kkt ")])
        lam = np.array([[float(v) for v in l.split()[3:]] for l in lines if l.startswith("MMA_PROBE lam ")])
        slabs = [np.fromfile("%s.%d" % (dump, rk), dtype=np.float64) for rk in range(nproc)]
        assert all(s.size % iters == 0 for s in slabs) and sum(s.size for s in slabs) == iters * n, [s.size for s in slabs]
        xs = np.concatenate([s.reshape(iters, -1) for s in slabs], axis=1)
        assert kkt.shape == (iters + 1, 2) and lam.shape == (iters, m) and xs.shape == (iters, n)
        runs[nproc] = (xs, lam, kkt)
    xs1, lam1, kkt1 = runs[1]
    for nproc in (2, 3):
        xs, lam, kkt = runs[nproc]
        assert kkt[0][1] == kkt1[0][1], (nproc, kkt[0], kkt1[0])
        assert abs(kkt[0][0] - kkt1[0][0]) <= 1e-13 * kkt1[0][0], (nproc, kkt[0], kkt1[0])
        dx = float(np.abs(xs - xs1).max())
        dlam = float((np.abs(lam - lam1).max(axis=1) / np.maximum(np.abs(lam1).max(axis=1), 1.0)).max())
        dkkt = float(np.abs(kkt[1:] / kkt1[1:] - 1.0).max())
        print("m = %d, %d ranks against 1: design %.2e, lam %.2e, KKT %.2e" % (m, nproc, dx, dlam, dkkt))
        assert dx <= 1e-9 and dlam <= 1e-9 and dkkt <= 1e-9, (nproc, dx, dlam, dkkt)
    xs_o, kkt_o, lam_o = run_oracle_synthetic(orc, n, m, iters, tokens, kkt_before=True)
    dx = float(np.abs(xs1 - xs_o).max())
    dlam = float((np.abs(lam1 - lam_o).max(axis=1) / np.maximum(np.abs(lam_o).max(axis=1), 1.0)).max())
    dkkt = float(np.abs(kkt1 / kkt_o - 1.0).max())
    print("m = %d, 1 rank against the oracle in reference order: design %.2e, lam %.2e, KKT %.2e" % (m, dx, dlam, dkkt))
    assert dx <= 1e-9 and dlam <= 1e-9 and dkkt <= 1e-9, (dx, dlam, dkkt)
    assert not np.array_equal(xs1[0], xs1[-1])


_DRIVER_KW = dict(nxyz=(33, 17, 17), nlvls=3, rmin=0.1, volfrac=0.3)
_RECORD_KEYS = {"itr", "fx", "fx_scaled", "gx", "ch", "mnd", "time", "ksp_its", "ksp_rerr", "mma_inner"}


@pytest.mark.gpu
def test_driver_kkt_records_match_numpy():
    """TopOpt(kkt=True): each record's kkt_norm2 / kkt_normInf = MMA.cc:428-496 in numpy on the gathered vectors of
    that iteration (x just returned by Update, Update's other arguments) and state()'s lam, to 1e-12"""
    from topopt_in_petsc_amd.driver import TopOpt
    opt = TopOpt(kkt=True, **_DRIVER_KW)
    for _ in range(10):
        rec = opt.step()
        assert set(rec) == _RECORD_KEYS | {"kkt_norm2", "kkt_normInf"}
        lam, z, _ = opt.mma.state()
        y = [max(0.0, l - 1000.0) for l in lam]
        get = lambda t: t.cpu().numpy().astype(np.float64)
        n2, ni = _kkt_np(get(opt.x), get(opt.dfdx), [rec["gx"]], [get(opt.dgdx[0])], get(opt.xmin), get(opt.xmax),
                         lam, [0.0], y, z)
        assert abs(rec["kkt_norm2"] - n2) <= 1e-12 * n2, (rec["itr"], rec["kkt_norm2"], n2)
        assert abs(rec["kkt_normInf"] - ni) <= 1e-12 * ni, (rec["itr"], rec["kkt_normInf"], ni)


@pytest.mark.gpu
def test_driver_defaults_are_todays_run():
    """all defaults: the records carry today's keys; passing the reference's defaults explicitly (a = 0, c = 1000,
    d = 0, asymptotes 0.5 / 0.7 / 1.2, robust 0, no constraint modification) gives the same run bit for bit, and other
    asymptote factors reach the kernel (a different design history)"""
    from topopt_in_petsc_amd.driver import TopOpt

    def run(**kw):
        opt = TopOpt(**_DRIVER_KW, **kw)
        recs, xs = [], []
        for _ in range(6):
            recs.append(opt.step())
            xs.append(opt.x.cpu().numpy().copy())
        return recs, xs

    r0, x0 = run()
    r1, x1 = run(aMMA=0.0, cMMA=1000.0, dMMA=0.0, mma_asymptotes=(0.5, 0.7, 1.2), mma_robust_asymptotes=0,
                 mma_constraint_modification=False)
    _, x2 = run(mma_asymptotes=(0.2, 0.65, 1.05))
    for a, b, xa, xb in zip(r0, r1, x0, x1):
        assert set(a) == _RECORD_KEYS and set(b) == _RECORD_KEYS
        assert (a["fx"], a["ch"], a["ksp_its"]) == (b["fx"], b["ch"], b["ksp_its"])
        assert np.array_equal(xa, xb)
    assert any(not np.array_equal(a, b) for a, b in zip(x0, x2))
