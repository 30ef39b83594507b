"""The oracle MMA's settings (oracle/mma_oracle.c: a/c/d, SetAsymptotes, SetRobustAsymptotesType,
ConstraintModification) against what the REFERENCE's own MMA class computed with them: the recorded runs of
tests/golden/ref_mma_settings (make_ref_mma_settings.py), no GPU.  The helpers below restate ref_mma_driver.cc's
synthetic problem in numpy; tests/test_gpu_mma_shapes.py and tests/test_mma_surface.py use them too."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_mma_settings")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_ref_mma_settings import EX, EY, EZ, ITERS, case_id  # noqa: E402

_REF_CASES = [  # tests/test_mma_surface.py's list: (id, tokens, m, slab ranks of the reference run)
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


def synthetic_np(x, m):
    """ref_mma_driver.cc's problem: f = sum a_i / (x_i + 0.1), g_j = sum w_ji x_i / n - (0.25 + 0.05 j)"""
    n = x.size
    i = np.arange(n, dtype=np.float64)
    a = 1.0 + 0.3 * np.sin(0.37 * i)
    dfdx = -a / ((x + 0.1) * (x + 0.1))
    w = [1.0 + 0.5 * np.cos(0.11 * i * (j + 1)) for j in range(m)]
    dgdx = [wj / n for wj in w]
    gx = [float((wj * x).sum() / n) - (0.25 + 0.05 * j) for j, wj in enumerate(w)]
    return dfdx, gx, dgdx


def box_np(x, xmin, xmax):
    """ref_mma_driver.cc's box=1 pattern: every 5th variable with its box above x, every 5th below"""
    gi = np.arange(x.size)
    below = (gi % 5 == 1) & (x + 0.1 <= 1.0)
    above = (gi % 5 == 3) & (x - 0.1 >= 0.0)
    lo = np.where(below, x + 0.01, np.where(above, x - 0.1, xmin))
    hi = np.where(below, x + 0.1, np.where(above, x - 0.01, xmax))
    return lo, hi


def configure(mma, tokens):
    """apply ref_mma_driver.cc's key=value settings (but a/c/d: see acd_of) to an oracle or a device MMA"""
    kv = dict(t.split("=") for t in tokens)
    if "asym" in kv:
        mma.SetAsymptotes(*[float(v) for v in kv["asym"].split(",")])
    mma.SetRobustAsymptotesType(int(kv.get("robust", 0)))
    mma.ConstraintModification(kv.get("conmod", "0") == "1")
    return kv


def acd_of(tokens):
    kv = dict(t.split("=") for t in tokens)
    return {k: float(kv[k]) for k in "acd" if k in kv}


def run_oracle_synthetic(orc, n, m, iters, tokens, kkt_before=False):
    """the oracle in reference order on the synthetic problem: the designs, KKTresidual's norms and lam after every
    Update (kkt_before: also the norms before the first one, as host/mma_probe prints them)"""
    x = np.full(n, 0.3)
    mma = orc.MMA(x, m, **acd_of(tokens))
    kv = configure(mma, tokens)
    xs, kkts, lams = [], [], []
    for k in range(iters):
        dfdx, gx, dgdx = synthetic_np(x, m)
        xmin, xmax = mma.SetOuterMovelimit(0.0, 1.0, 0.2, x)
        if kv.get("box") == "1":
            xmin, xmax = box_np(x, xmin, xmax)
        if kkt_before and k == 0:
            kkts.append(mma.kkt(x, dfdx, gx, dgdx, xmin, xmax))
        x = mma.Update(x, dfdx, gx, dgdx, xmin, xmax)
        kkts.append(mma.kkt(x, dfdx, gx, dgdx, xmin, xmax))    # kkt=1: the new design with Update's other arguments
        xs.append(x.copy())
        lams.append(mma.state()[0].copy())
    return np.stack(xs), np.array(kkts), np.stack(lams)


def test_case_list_is_the_surface_tests():
    from test_mma_surface import _REF_CASES as theirs
    assert theirs == _REF_CASES


@pytest.mark.parametrize("name,tokens,m,nproc", _REF_CASES, ids=[case_id(c[0], c[2], c[3]) for c in _REF_CASES])
def test_oracle_settings_against_the_references_recorded_runs(orc, name, tokens, m, nproc):
    """The extended oracle, summing left to right like MMA.cc, against the reference's recorded run of each setting:
    every iteration's design to 1e-9, KKTresidual's two norms to 1e-10 relative (5e-9 with a = 1, where the norms are lam
    and z themselves and the dual solver fixes those only to its stopping tolerance) -- the bounds the device is held to
    in test_settings_against_the_references_own_mma_class.  The records of two reference ranks differ from the serial
    oracle only in the order of the sums; the same bounds apply.
    Measured: design <= 5.6e-16 in every case, KKT <= 2.8e-14 relative, with a = 1 7.6e-10 (one rank) and 1.5e-9 (two)."""
    rec = np.load(os.path.join(GOLDEN, case_id(name, m, nproc) + ".npz"))
    assert list(rec["tokens"]) == tokens + ["kkt=1"]
    xs, kkt, _ = run_oracle_synthetic(orc, EX * EY * EZ, m, ITERS, tokens)
    worst = float(np.abs(xs - rec["x"]).max())
    worst_kkt = float(np.abs(kkt / rec["kkt"] - 1.0).max())
    print("%s: worst |x - x_ref| %.3e, worst KKT relative %.3e" % (case_id(name, m, nproc), worst, worst_kkt))
    assert worst <= 1e-9, worst
    assert worst_kkt <= (5e-9 if "a=1" in tokens else 1e-10), worst_kkt
    if "robust=1" in tokens or "conmod=1" in tokens or "asym=0.2,0.65,1.05" in tokens or "a=1" in tokens:
        ref0, _, _ = run_oracle_synthetic(orc, EX * EY * EZ, m, ITERS, [])
        assert not np.array_equal(ref0, xs)          # the setting reached the oracle's code


def test_oracle_rejects_an_invalid_robust_type(orc):
    mma = orc.MMA(np.full(8, 0.3), 1)
    with pytest.raises(ValueError):
        mma.SetRobustAsymptotesType(2)
    with pytest.raises(ValueError):
        orc.MMA(np.full(8, 0.3), 2, a=[1.0])
