"""The device MMA (csrc/mma.h) against the oracle in the device's summation order (oracle/mma_oracle.c), BIT FOR BIT, at the
shapes, signs and constraint counts where the kernels can go wrong:

  * element counts that are no multiple of the workgroup (256) or of the wave (64), below one wave, exactly at the grid
    cap of 1024 workgroups (262144), one element into the second grid stride (262145) and a second stride with a tail
    that is no multiple of 64 (265923 = 67 x 63 x 63);
  * objective and constraint gradients of both signs with exact zeros, so that the q / (x - L) halves of k_mma_gensub,
    k_mma_xyz and of the dual Hessian carry values;
  * every admitted number of constraints, 1 ... 7, and the refusal of 0, 8 and 9;
  * all four k_mma_gensub<ROBUST, CONMOD> instantiations with a tail and with a second stride.

Inputs are made once in numpy and handed unchanged to both sides.  Per case and after every Update: the design, the
asymptotes L / U, lam and the number of inner Newton steps are equal bit for bit, so are SetOuterMovelimit's outputs,
DesignChange and KKTresidual's normInf; KKTresidual's norm2 is held to 1e-13 relative (test_mma_surface.py's bound).
Every branch the issue names is counted from the oracle's and from the device's own vectors; the two counts are equal case
by case and test_every_branch_was_entered asserts that each is positive over the module.

Since this file the oracle adds KKTresidual's squares in the device's order too (three per element in the element's
thread, k_mma_kkt; then k_sum_max_final's order) when set_device_order() is on: left to right over 8e5 positive terms its
norm2 sat at 2e-14 ... 6e-14 of the device's, too close to the 1e-13 bound to mean anything.  The model of the order of
every other sum (workgroups of 256 striding over min(ceil(n / 256), 1024) groups, shuffle trees) needed no change.

The issue's sign-mixed problem alone cannot tell one grid cap from another (see _spike): two "spiked" cases at 262145 and
265923 are added for that.  No difference between device and oracle was found at any shape; mma.h and common.h are
unchanged.

MEASURED on the MI355X (46 tests of this file: 15 s, the slowest case 2.3 s, n = 262145 / 265923 with m = 7):
  * design, L, U, lam, z, inner steps, SetOuterMovelimit, DesignChange, normInf: bit-equal in all 39 cases at every
    iteration, and in the 9 awkward places of test_maxima_in_awkward_places (DesignChange 0.125, normInf 7.5 exactly);
  * norm2: relative difference 0.0 in every case and place (bound 1e-13), with the oracle's sum in the device's order;
  * branch counts per size, summed over the size's cases (h- / h+ / h0: helpvar at k >= 3; a / in / b: new x at alpha,
    between, at beta; L^ Lv U^ Uv: L clamped from below / above, U from below / above; lam>c; below / above: robust type 1)
        n        h-       h+      h0        a       in        b     L^     Lv     U^     Uv  lam>c   below   above
        1         0        0      12        0       16        0      0      0      0      0      0       0       0
       45         5      258     277      328      180      212      8      8      8      8      0       0       0
       63        12      336     408      484      238      286     10     10     10     10      0       0       0
       64        13      336     419      501      236      287     10     10     10     10      0       0       0
       65        11      352     417      498      253      289     10     10     10     10      0       0       0
      255        25     1438    1597     1801     1112     1167     40     40     40     40      0       0       0
      256        28     1444    1600     1807     1122     1167     40     40     40     40      0       0       0
      257        30     1447    1607     1818     1126     1168     40     40     40     40      0       0       0
     1001       963    37544   27559    34275    32930    20883    693    728    728    693      0    2400    1714
   262144         0   517478    6810   676140   439533   457191  40330      0      0  40330      9       0       0
   262145       296  1065992  244437  1108885   977359   797351  60495  40330  40330  60495     29       0       0
   265923     16200  2899047  541752  2472879  2808730  1898312 102280  81824  81824 102280     53  212740  212736
    dfdx and dgdx are > 0, < 0 and == 0 at every size but 1 (there both are 0); z > 0 in all 8 (n = 1001) and 4
    (n = 265923) iterations of the a = 1, c = 100 cases; constraint modification changes every iteration's design;
  * planted errors, each against an otherwise identical library: the grid cap of tp_mma_update at 2048 (with its partial
    buffer enlarged, so that nothing is written out of bounds) fails both spiked cases and n265923-m2-acd; qv[j] / xl
    dropped from k_mma_xyz's gradient sum fails every case from n = 45 on and test_admission_window; M->red for M->red + o
    in mma_reduce fails both cases of test_mma_surface.py::test_many_constraints_across_slab_ranks.  The old MMA tests pass
    under the first and the third; the second also fails the two recorded conmod cases of test_mma_surface.py.
    i <= n for i < n in k_mma_change was not run: restated on the CPU over the guarded buffers of
    test_maxima_in_awkward_places it returns 2e30 for 0.125 and overwrites xold's guard.
"""
import os
import subprocess
import time

import numpy as np
import pytest

from test_oracle_mma_settings import box_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1024 * 256                      # grid_for(n, 1024) workgroups of 256: one grid stride
SMALL = [1, 45, 63, 64, 65, 255, 256, 257]
SETTINGS = {   # name -> (a/c/d, asymptotes, robust type, constraint modification, box pattern)
    "default": (None, None, 0, False, False),
    "acd": (dict(a=1.0, c=100.0, d=1.0), None, 0, False, False),                       # k_mma_gensub<0, 0>, z > 0
    "robust-box": (None, None, 1, False, True),                                       # k_mma_gensub<1, 0>
    "conmod": (None, None, 0, True, False),                                           # k_mma_gensub<0, 1>
    "robust-conmod-asym": (None, (0.2, 0.65, 1.05), 1, True, True),                   # k_mma_gensub<1, 1>
    "spiked": (None, None, 0, False, False),                                          # see _spike
}
SPIKES = [3, 70, 130, 1024 * 256, 1024 * 256 + 3, 1024 * 256 + 70, 1024 * 256 + 300]
# (n, m, iterations, setting).  8 iterations at the small sizes; at the large ones as few as keep a case at seconds
# (the oracle in device order is the cost), at least 3 so that the k >= 3 asymptote update runs.
CASES = ([(n, m, 8, "default") for n in SMALL for m in (1, 2)]
         + [(1001, m, 8, "default") for m in range(1, 8)]
         + [(CAP, 1, 3, "default"), (CAP, 2, 3, "default")]
         + [(n, m, it, "default") for n in (CAP + 1, 265923) for m, it in ((2, 4), (7, 3))]
         + [(n, 2, 8 if n == 1001 else 4, s) for n in (1001, 265923) for s in SETTINGS if s not in ("default", "spiked")]
         + [(n, 2, 4, "spiked") for n in (CAP + 1, 265923)])
BRANCHES = ["helpvar<0", "helpvar>0", "helpvar==0", "x==alpha", "x==beta", "alpha<x<beta", "L clamped from below",
            "L clamped from above", "U clamped from below", "U clamped from above", "dfdx>0", "dfdx<0", "dfdx==0",
            "dgdx>0", "dgdx<0", "dgdx==0", "lam>c", "z>0 (a=1, c=100)", "below its box (robust 1)",
            "above its box (robust 1)", "conmod changes the design"]
COUNTS = {}        # case -> {branch: count}, from the oracle's vectors (the device's are asserted equal to them)
DESIGNS = {}       # (n, "default") at m = 2 -> the designs of every iteration, for the conmod comparison
WORST = {}         # case -> worst relative difference of KKTresidual's norm2


def _problem(n, m):
    """sign-mixed gradients with exact zeros: dfdx = sin(0.37 i) (1 + x), zero where i % 7 == 0; dgdx_j = (cos(0.11 i (j + 1))
    + 0.3) / n, zero where i % 11 == 0; g_j linear, feasible by 0.01 (j + 1) at x = 0.3"""
    ii = np.arange(n)
    i = ii.astype(np.float64)
    s = np.sin(0.37 * i)
    s[ii % 7 == 0] = 0.0
    dg = []
    for j in range(m):
        d = (np.cos(0.11 * i * (j + 1)) + 0.3) / n
        d[ii % 11 == 0] = 0.0
        dg.append(d)
    return s, dg


def _spike(dg, n):
    """The sums of the problem above cannot tell one grid cap from another: a thread's second-stride term is 1e-6 of a sum
    whose last bit is worth 1e-16, and a tree sum's low levels are rounded away at its top (the oracle with 2048 for 1024
    workgroups gives the same lam, bit for bit, at 262145 and at 265923).  With all but a few constraint gradients scaled
    down by 2^-20 and those few up by 2^10 a handful of terms carry each sum, some of them in the second stride: (x_1 + y_1) + x_2 in a thread that
    takes two strides against (x_1 + x_2) + y_1 without, and lam differs in most iterations (checked on the oracle)."""
    out = []
    for j, d in enumerate(dg):
        e = np.array([i for i in SPIKES if i < n])
        big = np.where(d[e] != 0.0, d[e], (1.0 + 0.1 * j) / n) * 2.0 ** 10
        d = d * 2.0 ** -20
        d[e] = big
        out.append(d)
    return out


def _count(k, setting, xin, xo1, xo2, Lp, Up, xmin, xmax, L, U, xnew, dfdx, dg, lam, c, z):
    """the branches of one Update (its k-th), from one side's own vectors"""
    acd, _, robust, _, _ = SETTINGS[setting]
    cnt = dict.fromkeys(BRANCHES, 0)
    alpha, beta = np.maximum(xmin, 0.9 * L + 0.1 * xin), np.minimum(xmax, 0.9 * U + 0.1 * xin)
    cnt["x==alpha"] = int((xnew == alpha).sum())
    cnt["x==beta"] = int((xnew == beta).sum())
    cnt["alpha<x<beta"] = int(((alpha < xnew) & (xnew < beta)).sum())
    assert ((alpha <= xnew) & (xnew <= beta)).all()
    for name, v in (("dfdx", dfdx), ("dgdx", np.concatenate(dg))):
        cnt[name + ">0"], cnt[name + "<0"], cnt[name + "==0"] = int((v > 0).sum()), int((v < 0).sum()), int((v == 0).sum())
    cnt["lam>c"] = int((np.asarray(lam) > c).sum())
    if acd:
        cnt["z>0 (a=1, c=100)"] = int(z > 0.0)
    if k >= 3:
        helpvar = (xin - xo1) * (xo1 - xo2)
        cnt["helpvar<0"], cnt["helpvar>0"] = int((helpvar < 0).sum()), int((helpvar > 0).sum())
        cnt["helpvar==0"] = int((helpvar == 0).sum())
        if robust == 0:
            asy = SETTINGS[setting][1] or (0.5, 0.7, 1.2)
            gamma = np.where(helpvar < 0.0, asy[1], np.where(helpvar > 0.0, asy[2], 1.0))
            Lraw, Uraw = xin - gamma * (xo1 - Lp), xin + gamma * (Up - xo1)
            xmi = np.maximum(1.0e-5, xmax - xmin)
            cnt["L clamped from below"] = int((Lraw < xin - 10.0 * xmi).sum())
            cnt["L clamped from above"] = int((Lraw > xin - 0.01 * xmi).sum())
            cnt["U clamped from below"] = int((Uraw < xin + 0.01 * xmi).sum())
            cnt["U clamped from above"] = int((Uraw > xin + 10.0 * xmi).sum())
        else:
            cnt["below its box (robust 1)"] = int((xin < xmin - 1.0e-5).sum())
            cnt["above its box (robust 1)"] = int((xin > xmax + 1.0e-5).sum())
    return cnt


def _run_case(orc, case, tp=None):
    """oracle (device order) and, with tp, the device in lockstep on the same inputs; fills COUNTS[case]"""
    n, m, iters, setting = case
    acd, asy, robust, conmod, box = SETTINGS[setting]
    s, dg = _problem(n, m)
    if setting == "spiked":
        dg = _spike(dg, n)
    x = np.full(n, 0.3)
    m_o = orc.MMA(x, m, **(acd or {}))
    m_o.set_device_order()
    sides = [m_o]
    if tp is not None:
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        host = lambda t: t.cpu().numpy()
        grid = tp.Grid(9, 5, 5, 0.25)
        xd = dev(x)
        m_d = tp.MMA(grid, xd, m, n_global=n, **(acd or {}))
        sides.append(m_d)
        xold_d, xmin_d, xmax_d = dev(x), dev(np.zeros(n)), dev(np.zeros(n))
        dg_d = [dev(d) for d in dg]
        r_xo1, r_xo2, r_U, r_L = (dev(np.zeros(n)) for _ in range(4))
    for mm in sides:
        if asy:
            mm.SetAsymptotes(*asy)
        mm.SetRobustAsymptotesType(robust)
        mm.ConstraintModification(conmod)
    c = (acd or {}).get("c", 1000.0)
    xold_o = x.copy()
    total = dict.fromkeys(BRANCHES, 0)
    worst, xs = 0.0, []
    Lp, Up = np.zeros(n), np.zeros(n)
    xo1, xo2 = x.copy(), x.copy()
    pinch = np.arange(n) % 13 == 5
    for it in range(iters):
        dfdx = s * (1.0 + x)
        gx = [float(dg[j] @ (x - 0.3)) - 0.01 * (j + 1) for j in range(m)]
        xmin, xmax = m_o.SetOuterMovelimit(0.0, 1.0, 0.2, x)
        if tp is not None:
            m_d.SetOuterMovelimit(0.0, 1.0, 0.2, xd, xmin_d, xmax_d)
            assert np.array_equal(host(xmin_d), xmin) and np.array_equal(host(xmax_d), xmax), (case, it)
        if box:
            xmin, xmax = box_np(x, xmin, xmax)
        elif it == 2:
            # the third Update sees a box of 1e-4 around every 13th variable: its asymptotes, 0.1 ... 0.2 away, are pulled
            # in to 10 box widths, and the Update after that finds them nearer than 0.01 of the restored box
            xmin = np.where(pinch, np.maximum(xmin, x - 5.0e-5), xmin)
            xmax = np.where(pinch, np.minimum(xmax, x + 5.0e-5), xmax)
        xin = x
        x = m_o.Update(xin, dfdx, gx, dg, xmin, xmax)
        L, U = m_o.asymptotes()
        lam, z = m_o.state()
        assert np.isfinite(x).all() and np.isfinite(lam).all(), (case, it)
        alpha, beta, _, _ = m_o.subproblem()
        assert np.array_equal(alpha, np.maximum(xmin, 0.9 * L + 0.1 * xin)), (case, it)
        assert np.array_equal(beta, np.minimum(xmax, 0.9 * U + 0.1 * xin)), (case, it)
        cnt = _count(it + 1, setting, xin, xo1, xo2, Lp, Up, xmin, xmax, L, U, x, dfdx, dg, lam, c, z)
        ch_o = m_o.DesignChange(x, xold_o)
        n2_o, ni_o = m_o.kkt(x, dfdx, gx, dg, xmin, xmax)
        if tp is not None:
            xmin_d.copy_(dev(xmin))
            xmax_d.copy_(dev(xmax))
            dfdx_d = dev(dfdx)
            m_d.Restart(r_xo1, r_xo2, r_U, r_L)
            before = [host(t).copy() for t in (xd, r_xo1, r_xo2, r_L, r_U)]
            m_d.Update(xd, dfdx_d, gx, dg_d, xmin_d, xmax_d)
            m_d.Restart(r_xo1, r_xo2, r_U, r_L)
            xg, Lg, Ug = host(xd), host(r_L), host(r_U)
            lam_d, z_d, k_d = m_d.state()
            where = (case, it)
            assert np.array_equal(xg, x), (where, float(np.abs(xg - x).max()))
            assert m_d.last_inner == m_o.last_inner, (where, m_d.last_inner, m_o.last_inner)
            assert np.array_equal(np.asarray(lam_d), lam), (where, lam_d, lam)
            assert z_d == z and k_d == it + 1, where
            assert np.array_equal(Lg, L) and np.array_equal(Ug, U), where
            assert np.array_equal(before[0], xin) and np.array_equal(host(r_xo1), xin), where
            cnt_d = _count(it + 1, setting, *before, host(xmin_d), host(xmax_d), Lg, Ug, xg, host(dfdx_d),
                           [host(t) for t in dg_d], lam_d, c, z_d)
            assert cnt_d == cnt, (where, cnt_d, cnt)
            ch_d = m_d.DesignChange(xd, xold_d)
            assert ch_d == ch_o, (where, ch_d, ch_o)
            assert np.array_equal(host(xold_d), x), where
            n2_d, ni_d = m_d.KKTresidual(xd, dfdx_d, gx, dg_d, xmin_d, xmax_d)
            assert ni_d == ni_o, (where, ni_d, ni_o)
            rel = abs(n2_d - n2_o) / n2_o
            worst = max(worst, rel)
            assert rel <= 1e-13, (where, n2_d, n2_o)
        for key in BRANCHES:
            total[key] += cnt[key]
        xo2, xo1, Lp, Up = xo1, xin, L, U
        xs.append(x)
    if setting == "default" and m == 2 and n in (1001, 265923):
        DESIGNS[(n, setting)] = xs
    COUNTS[case], WORST[case] = total, worst
    return xs


def _id(case):
    return "n%d-m%d-%s" % (case[0], case[1], case[3])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_device_mma_is_the_oracle_bit_for_bit(orc, case):
    """every assertion of the module docstring for one (n, m, setting); with constraint modification the design differs
    from the run without it"""
    import topopt_in_petsc_amd as tp
    t0 = time.time()
    xs = _run_case(orc, case, tp)
    n, m, iters, setting = case
    if SETTINGS[setting][3] and not SETTINGS[setting][2]:
        if (n, "default") not in DESIGNS:
            _run_case(orc, (n, 2, iters, "default"))
        differs = sum(int(not np.array_equal(a, b)) for a, b in zip(xs, DESIGNS[(n, "default")]))
        COUNTS[case]["conmod changes the design"] = differs
        assert differs > 0
    print("%s: %d iterations, worst relative norm2 difference %.2e, %.1f s; %s"
          % (_id(case), iters, WORST[case], time.time() - t0, {k: v for k, v in COUNTS[case].items() if v}))


@pytest.mark.gpu
def test_every_branch_was_entered(orc):
    """Over the module every branch of BRANCHES was entered, counted from vectors that the device reproduced bit for bit
    (a case that was not run in this session is run on the oracle alone first).  Printed per size."""
    for case in CASES:
        if case not in COUNTS:
            _run_case(orc, case)
    conmod = [c for c in CASES if c[3] == "conmod"]
    for case in conmod:
        if not COUNTS[case]["conmod changes the design"]:
            xs, x0 = _run_case(orc, case), DESIGNS.get((case[0], "default")) or _run_case(orc, case[:3] + ("default",))
            COUNTS[case]["conmod changes the design"] = sum(int(not np.array_equal(a, b)) for a, b in zip(xs, x0))
    for n in sorted({c[0] for c in CASES}):
        tot = {k: sum(COUNTS[c][k] for c in CASES if c[0] == n) for k in BRANCHES}
        print("n = %d: %s" % (n, tot))
    for key in BRANCHES:
        assert sum(COUNTS[c][key] for c in CASES) > 0, key
    # the settings' own branches are entered with a tail (1001) and with a second stride (265923)
    for n in (1001, 265923):
        at = lambda s, n=n: COUNTS[(n, 2, 8 if n == 1001 else 4, s)]
        assert at("acd")["z>0 (a=1, c=100)"] > 0, n
        for s in ("robust-box", "robust-conmod-asym"):
            assert at(s)["below its box (robust 1)"] > 0 and at(s)["above its box (robust 1)"] > 0, (n, s)
        assert at("conmod")["conmod changes the design"] > 0, n
    # and at n = 1001 alone every branch that needs no setting, helpvar < 0 included
    plain = [b for b in BRANCHES if "(" not in b and "conmod" not in b and b != "lam>c"]
    for key in plain:
        assert sum(COUNTS[c][key] for c in CASES if c[0] == 1001) > 0, key


def _awkward_places(n):
    """the last element, the first element of the second grid stride, and the middle of the last, partial wave"""
    tail = n % 64
    return sorted({n - 1} | ({CAP} if n > CAP else set()) | ({n - tail + tail // 2} if tail else set()))


GUARD = 1.0e30


def _guarded(a, guard):
    """a on the device as the first a.size elements of a buffer that is one element longer: a kernel that steps one element
    past the end (i <= n for i < n) reads or writes the guard, inside the allocation, and the result or the guard shows it"""
    import torch
    buf = torch.from_numpy(np.concatenate([a, [guard]])).cuda()
    return buf, buf[:a.size]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 257, CAP + 1, 265923])
def test_maxima_in_awkward_places(orc, n):
    """k_mma_change / k_max_final and k_mma_kkt / k_sum_max_final with the one extreme element in the last place of the
    vector, in the first place of the second grid stride and inside the last, partial wave: DesignChange returns that one
    difference exactly (0.125, and xold becomes x), KKTresidual's normInf is that one element's |dfdx| (7.5; before any
    Update lam = 0 and x is interior, so the residual is dfdx itself) and its norm2 the oracle's to 1e-13.  Every vector
    is followed by a guard element of +-1e30 in the same allocation: an off-by-one at the end would return 2e30 and 1e30."""
    import torch
    import topopt_in_petsc_amd as tp
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    grid = tp.Grid(9, 5, 5, 0.25)
    i = np.arange(n, dtype=np.float64)
    xold = 0.25 + 0.125 * np.cos(0.01 * i) ** 2
    small = 1.0e-3 * np.sin(0.37 * i)
    dg = [np.full(n, 1.0 / n)]
    m_o = orc.MMA(xold, 1)
    m_o.set_device_order()
    x0_d = dev(xold)
    m_d = tp.MMA(grid, x0_d, 1, n_global=n)
    dg_buf, dg_d = _guarded(dg[0], GUARD)
    lo_buf, lo_d = _guarded(np.zeros(n), -GUARD)
    hi_buf, hi_d = _guarded(np.ones(n), GUARD)
    places = _awkward_places(n)
    assert n - 1 in places and (n <= CAP or CAP in places) and len(places) >= (2 if n % 64 > 2 else 1)
    for p in places:
        x = xold.copy()
        x[p] = xold[p] + 0.125
        assert x[p] - xold[p] == 0.125
        x_buf, xd = _guarded(x, GUARD)
        xold_buf, xold_d = _guarded(xold, -GUARD)
        ch = m_d.DesignChange(xd, xold_d)
        assert ch == 0.125, (n, p, ch)
        assert ch == m_o.DesignChange(x, xold.copy())
        assert np.array_equal(xold_buf.cpu().numpy(), np.concatenate([x, [-GUARD]])), (n, p)
        assert m_d.DesignChange(xd, xold_d) == 0.0, (n, p)
        dfdx = small.copy()
        dfdx[p] = -7.5
        df_buf, df_d = _guarded(dfdx, GUARD)
        n2_o, ni_o = m_o.kkt(x, dfdx, [0.0], dg, np.zeros(n), np.ones(n))
        n2_d, ni_d = m_d.KKTresidual(xd, df_d, [0.0], [dg_d], lo_d, hi_d)
        assert ni_d == 7.5 and ni_o == 7.5, (n, p, ni_d, ni_o)
        assert abs(n2_d - n2_o) <= 1e-13 * n2_o, (n, p, n2_d, n2_o)
        for buf, g in ((x_buf, GUARD), (xold_buf, -GUARD), (df_buf, GUARD), (dg_buf, GUARD), (lo_buf, -GUARD), (hi_buf, GUARD)):
            assert float(buf[n]) == g, (n, p)
        print("n = %d, extreme at %d: DesignChange %.17g, normInf %.17g, norm2 relative difference %.2e"
              % (n, p, ch, ni_d, abs(n2_d - n2_o) / n2_o))


@pytest.mark.gpu
def test_admission_window(orc):
    """tp_mma_create admits 1 <= m <= 7 (m + m^2 <= 64 values fit the host's reduction buffer; m = 7 runs in the cases
    above): m = 0, 8 and 9 raise, and after each refusal the same grid serves a fresh MMA whose first step is the
    oracle's bit for bit"""
    import torch
    import topopt_in_petsc_amd as tp
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = 45
    grid = tp.Grid(9, 5, 5, 0.25)
    s, dg = _problem(n, 2)
    x0 = np.full(n, 0.3)
    for bad in (0, 8, 9):
        xd = dev(x0)
        with pytest.raises(tp.TopOptError):
            tp.MMA(grid, xd, bad, n_global=n)
        m_o, m_d = orc.MMA(x0, 2), tp.MMA(grid, xd, 2, n_global=n)
        m_o.set_device_order()
        xmin_d, xmax_d = dev(np.zeros(n)), dev(np.zeros(n))
        dfdx, gx = s * (1.0 + x0), [-0.01, -0.02]
        xmin, xmax = m_o.SetOuterMovelimit(0.0, 1.0, 0.2, x0)
        m_d.SetOuterMovelimit(0.0, 1.0, 0.2, xd, xmin_d, xmax_d)
        x = m_o.Update(x0, dfdx, gx, dg, xmin, xmax)
        m_d.Update(xd, dev(dfdx), gx, [dev(d) for d in dg], xmin_d, xmax_d)
        assert np.array_equal(xd.cpu().numpy(), x), bad
        assert np.array_equal(np.asarray(m_d.state()[0]), m_o.state()[0]), bad
        assert not np.array_equal(x, x0)
        m_d.close()


@pytest.mark.gpu
def test_mma_probe_refuses_eight_constraints():
    """host/mma_probe with m = 8: the create's error code (TP_ERR_ARG = 1) is the exit status and no step is taken"""
    r = subprocess.run([os.path.join(ROOT, "host", "slabrun"), "-n", "1", "--same-device",
                        os.path.join(ROOT, "host", "mma_probe"), "16", "8", "8", "8", "2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
    assert "MMA_PROBE" not in r.stdout, r.stdout[-2000:]
