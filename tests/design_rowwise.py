"""Row-wise error bounds for the design-side kernel families: overhang filter, casting filter, local volume constraint, length
scale constraints (a plain helper module: no fixtures, no collection hooks; the counterpart of tests/response_rowwise.py).

Why: these outputs span many decades -- p = xi^(P-1) with P = 40, rhobar^(p-1) with p = 16, E = exp(-c G), a transpose weighted
by (1 +- q) / 2 -- and max|got - ref| / max|ref| leaves every row far below the maximum unchecked.  Here every row i is held to

    |got_i - ref_i| <= c * eps * scale_i,        eps = 2^-53                                      (rowwise.assert_rowwise)

`ref` and `scale_i` in 80-bit arithmetic from the restatements' own quantities (overhang_ref, casting_ref, localvol_ref,
lengthscale_ref).  No row is left out; a row of scale 0 must match bit for bit.

OVERHANG (csrc/overhang.h).  xi: the local rounding propagated through the reference's own Jacobian, layer by layer:
    e_0 = 0 (layer 0 is x itself),   e_l = loc_l + w_l * cross(p_{l-1} e_{l-1}),   loc = |x| + Xi (1 + |ln Xi|) + rho + sqrt(eps)
(d xi_l / d xi_{l-1,j} = w_l p_{l-1,j}: the products the transpose forms; |ln Xi|: the kernel raises S to the float64 nearest to
1/Q, which moves Xi by |ln Xi| eps / 2 relative -- 6 eps at (P, xi0) = (20, 0.4) on S = 1e-200 -- and Xi likewise below).
The stored coefficients:
    p   c_pow p + (P-1) xi^(P-2) c_xi e, and an absolute floor of one subnormal spacing, 2^-1074 (nothing else has a floor)
    a   |a| + |q| (q = d / rho is rounded at size |q|, whatever is left of 1 - q) + (eps / rho^3) (the derivative of q) times the
        allowance on d = x - Xi, which is |x| + Xi + sw cross(p e) with sw = (P/Q) Xi / S
    w   w (1 + |ln Xi|) + sw/2 times a's terms + w (1 - 1/Q) times the relative allowance of S, (S + P cross(p e)) / S
The transposes are held to the 80-bit recursion run on the DEVICE'S OWN exported coefficients (the rule of
tests/test_gpu_rowwise.py for the Chebyshev step and its dinv); the scale is the same recursion on |g| -- every coefficient is
non-negative.  What the coefficients themselves may be off by is held above.
A support sum below S_MIN = 2^-960 counts as none (overhang_ref); ov_case asserts that no cell of the tail field has its S within
a factor 2 of S_MIN, and no cell of any case within 1024 times S's own allowance, or a rounding would flip the branch and the
comparison would mean nothing.

CASTING (csrc/casting.h).  c: e_first = 0,  e_k = (|x| + |c_prev| + rho) + 0.5 (1 - q_k) e_prev.  q: |q| + (eps / rho^3) times
(|x| + |c_prev| + e_prev); a sweep's first cell (q = 1, c = x) must match bit for bit.  Transposes as for the overhang.

LOCAL VOLUME (csrc/localvol.h).  rhobar and dgdx are sums of non-negative terms: each row relative to its OWN value, with the
counts of localvol_ref.bounds (taps + 8; (p + 1)(taps + 8) 2, the pn factor inside held relative).  A row whose ball holds
only zeros must be exactly 0.

LENGTH SCALE (csrc/lengthscale.h).  The rule of tests/response_rowwise.py: every factor by its absolute value, the differences
of the stencil term (+w at e+, -w at e-) by sums, the three terms of dS summed in absolute value; every term carrying E times
(1 + c G_e) for the rounding of the exponent; 1 - th^2 of H' by 1 + th^2.  A row with m = 0 exactly is bit-zero in T.

THE CONSTANTS follow the rule of tests/rowwise.py: the larger of the operation count read off the kernel and 16 x what the
float64 restatement measures against the 80-bit one over all cases below (tests/test_design_rowwise_oracle.py holds the
restatement to a QUARTER of each), rounded up to a power of two; never from what the HIP kernels achieve."""
import functools

import numpy as np

from tests import casting_ref as cref
from tests import lengthscale_ref as lsref
from tests import localvol_ref as lvref
from tests import overhang_ref as oref
from tests import rowwise as rw

LD = np.longdouble
EPS = rw.EPS
PLANT = 1e-3                      # relative size of the planted errors
DESIGNS = ("blocks", "one_solid", "one_void", "zlayer")      # rowwise.design, mapped to exact 0 / 1


def design01(kind, ne):
    return np.where(rw.design(kind, *ne) == rw.XMIN, 0.0, 1.0)


def hold(got, ref_ld, scale_ld, c, where, floor=0):
    """rowwise.assert_rowwise with the scale kept in 80-bit: rows whose scale lies below 2^-600 (p of a nearly void cell and its
    subnormal floor) are lifted by 2^512 in got, ref and scale alike -- exact in every one of them -- so that eps * scale does not
    underflow in float64.  floor: an absolute allowance on top of c eps scale (whatever c is).  -> the achieved c"""
    got = np.asarray(got, dtype=np.float64)
    scale_ld = np.asarray(scale_ld, dtype=LD) + LD(floor) / (LD(c) * LD(EPS))
    assert np.isfinite(got).all(), "%s: %d non-finite rows, the first at row %d" % (where.get("label"), int((~np.isfinite(got)).sum()),
                                                                                  int(np.flatnonzero(~np.isfinite(got))[0]))
    f = np.where((scale_ld > 0) & (scale_ld < LD(2.0) ** -600), LD(2.0) ** 512, LD(1))
    return rw.assert_rowwise((got.astype(LD) * f).astype(np.float64), np.asarray(ref_ld, dtype=LD) * f, (scale_ld * f).astype(np.float64), c, where)


# =====================================================================================================================
# overhang
# =====================================================================================================================
# xi.  Count per layer: pow and product of t (2), the four additions of S, pow(S, 1/Q), d, d d, + eps, sqrt, x + Xi, - rho,
# + sqrt(eps): 14 -> 16.  float64 restatement against the 80-bit one, measured over OV_CASES: 1.16 (x 16 = 18.6 -> 32).
C_OV_XI = 32
# a, w.  Count on top of the allowance on d: d, d d, + eps, sqrt, the division, 1 -+ q (6); w also Xi / S, x P/Q, the product (9)
# -> 16.  Measured: a 1.01, w 2.26 (x 16 = 36.1 -> 64).
C_OV_COEF = 64
# p = pow(xi, P - 1): one rounded pow on top of xi's allowance: 2.  Measured on the rows above 2^-960, which the floor has no part
# in: 1.15 (x 16 = 18.3 -> 32).
C_OV_POW = 32
OV_FLOOR = LD(2.0) ** -1074
OV_MESHES = [(70, 37, 11), (16, 12, 20), (3, 3, 3), (1, 1, 4)]
OV_BUILDS = ("+y", "-y", "+z", "-z")
OV_PARAMS = ((oref.P, oref.EPS, oref.XI0), (20.0, 1e-3, 0.4), (20.5, 1e-4, 0.5))
OV_FIELDS = ("random", "checker", "zerolayers") + DESIGNS + ("plate", "tail")
OV_CHUNKS = (1, 2, 4, 8)
# At P = 20 the floor on S sits at xi = S_MIN^(1/20) = 3.5e-15, where xi is all rounding (its allowance is eps sqrt(eps_par) = 4e-18
# absolute, times P in S): a void region deep enough walks xi down through that value, the branch at S_MIN is then decided by
# roundings, and w = 0 or 1e270 cannot be compared.  The cases below are the ones -- and the only ones -- in which ov_case's margin
# assertion fires (tests/test_design_rowwise_oracle.py asserts that it does on each of them); they are left out at the parameter
# sets 1 and 2, every other combination runs.  (At P = 40 the floor sits at xi = 6e-8, relative allowance 1e-9: nothing is left out.)
OV_UNDECIDABLE = {(ne, b, k, pi) for pi in (1, 2) for ne, b, k in (
    ((70, 37, 11), "+y", "blocks"), ((70, 37, 11), "-y", "blocks"), ((70, 37, 11), "+y", "one_solid"), ((70, 37, 11), "-y", "one_solid"),
    ((16, 12, 20), "+z", "blocks"), ((16, 12, 20), "-z", "blocks"), ((16, 12, 20), "+z", "plate"), ((16, 12, 20), "-z", "plate"))}


def ov_fields(ne, build, pi):
    return tuple(k for k in OV_FIELDS if (tuple(ne), build, k, pi) not in OV_UNDECIDABLE)


OV_CASES = [(ne, b, k, p) for ne in OV_MESHES for b in OV_BUILDS for p in range(len(OV_PARAMS)) for k in ov_fields(ne, b, p)]
# the tail field: values between TAIL_LO and TAIL_HI, none inside the gap.  x^40 of the gap's ends lies a factor 1e6 below and
# 1e4 above S_MIN = 2^-960 (1.03e-289), also five-fold: (4e-8)^40 = 1.2e-296, (8e-8)^40 = 1.3e-284
TAIL_LO, TAIL_HI, TAIL_GAP = 1e-10, 1e-6, (4e-8, 8e-8)
TAIL_PLANTS = ((32, 8, 1.0e-8), (5, 3, 1.2e-8), (12, 5, 7e-9))       # (i, r) of a cross of five cells and its value


def c_ov_adj(nl):
    """the transpose over nl layers from given coefficients.  Count: 7 roundings per layer (m = w lambda, four additions, the
    product with p, the addition of g) and the product with a: 7 nl + 1 -> 8 / 32 / 128 / 256 / 512 for 1 / 3, 4 / 11, 12 / 20
    / 37 layers.  float64 recursion against the 80-bit one on the same coefficients, measured: 5.36 (x 16 = 86 -> 128): the
    measured value sets the constant up to 11 layers, the count from 12 on."""
    return max(128, rw.pow2(7 * nl + 1))


def ov_field(kind, ne, seed=3):
    """overhang_ref.field, the 0/1 designs, and
    plate: solid layers at both ends of z over void (one solid layer over void over solid, from either end)
    tail:  mid densities (0.1 .. 0.9) everywhere but on the outermost planes of y and z -- the baseplate layer of every build,
           the layer UNDER the mid-density layers -- which are log-uniform in [1e-10, 1e-6] outside TAIL_GAP, with crosses of five
           cells planted at 1.0e-8 (w = inf without the floor on S), 1.2e-8 and 7e-9 (S = 0 in float64: the support term lost)"""
    ex, ey, ez = ne
    if kind in DESIGNS:
        return design01(kind, ne)
    if kind == "plate":
        a = np.zeros((ez, ey, ex))
        a[[0, ez - 1]] = 1.0
        return a.ravel()
    if kind != "tail":
        return oref.field(kind, ne, seed)
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 0.9, (ez, ey, ex))
    lo, hi = np.log(TAIL_LO), np.log(TAIL_HI)
    g0, g1 = np.log(TAIL_GAP[0]), np.log(TAIL_GAP[1])
    u = rng.uniform(0.0, (g0 - lo) + (hi - g1), (ez, ey, ex))
    t = np.exp(np.where(u < g0 - lo, lo + u, g1 + (u - (g0 - lo))))
    t = np.where((t >= TAIL_GAP[0]) & (t <= TAIL_GAP[1]), TAIL_GAP[0] * 0.5, t)     # (the ends, to whatever exp rounds them)
    for axis, n in ((0, ez), (1, ey)):
        for pl in (sorted({0, n - 1}) if n >= 3 else []):       # (fewer than three layers: no layer lies under a mid-density one)
            sl = [slice(None)] * 3
            sl[axis] = pl
            sub_a, sub_t = a[tuple(sl)], t[tuple(sl)].copy()      # [other axis, x]
            for m, (i, r, v) in enumerate(TAIL_PLANTS):
                if m == 0:                                        # the first cross is planted on every mesh, against its last cell
                    i, r = min(i, ex - 1), min(r, sub_t.shape[0] - 1)
                elif i + 1 >= ex or r + 1 >= sub_t.shape[0]:
                    continue
                for di, dr in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
                    if 0 <= i + di < ex and 0 <= r + dr < sub_t.shape[0]:
                        sub_t[r + dr, i + di] = v
            sub_a[...] = sub_t
    return a.ravel()


def ov_scales(x, ne, build, fl, params):
    """-> dict(xi, a, w, p) of row scales (80-bit, flat) from the 80-bit forward fl, by the formulas of the module docstring; the
    ratios C_OV_XI / C_OV_COEF and C_OV_XI / C_OV_POW turn the allowance on xi into units of the coefficient's own constant"""
    P_, eps_, xi0 = (LD(v) for v in params)
    Q = P_ + np.log(LD(5)) / np.log(xi0)
    sqeps = np.sqrt(eps_)
    rx, rp = LD(C_OV_XI) / C_OV_COEF, LD(C_OV_XI) / C_OV_POW
    out = {k: np.zeros(x.size, dtype=LD) for k in ("xi", "a", "w", "p", "S")}
    X = oref.layers(np.asarray(x).astype(LD), ne, build)
    F = {k: oref.layers(fl[k], ne, build) for k in ("xi", "Xi", "S", "a", "w", "p")}
    O = {k: oref.layers(v, ne, build) for k, v in out.items()}
    O["p"][0] = F["p"][0]                           # layer 0: xi = x, a = 1, w = 0 exactly (scale 0); p one rounded pow
    for l in range(1, X.shape[0]):
        prop = oref._cross(F["p"][l - 1] * O["xi"][l - 1])
        S, Xi = F["S"][l], F["Xi"][l]
        sup = Xi != 0
        Ss = np.where(sup, S, LD(1))
        sw = np.where(sup, (P_ / Q) * (Xi / Ss), LD(0))
        # Xi = S^(1/Q) with 1/Q rounded to float64: relative |ln Xi| eps on top of the pow's own rounding
        amp = 1 + np.abs(np.log(np.where(sup, Xi, LD(1))))
        d = X[l] - Xi
        rho = np.sqrt(d * d + eps_)
        q = d / rho
        O["xi"][l] = (np.abs(X[l]) + Xi * amp + rho + sqeps) + F["w"][l] * prop
        dq = (eps_ / rho ** 3) * (np.abs(X[l]) + Xi * amp + sw * prop)
        O["a"][l] = (np.abs(F["a"][l]) + np.abs(q)) + rx * dq
        rel_s = np.where(sup, (Ss + rx * P_ * prop) / Ss, LD(0))
        O["w"][l] = F["w"][l] * amp + LD(0.5) * sw * (np.abs(q) + rx * dq) + F["w"][l] * (1 - 1 / Q) * rel_s
        O["p"][l] = F["p"][l] + rp * (P_ - 1) * np.abs(F["xi"][l]) ** (P_ - 2) * O["xi"][l]
        O["S"][l] = S + rx * P_ * prop                 # (the allowance on S itself, in units of C_OV_COEF eps: ov_case's margin)
    return out


@functools.lru_cache(maxsize=32)
def ov_case(ne, build, kind, pi=0):
    """computed once per case and left unchanged: x, g[3], the 80-bit forward, the row scales; asserts the distance of every
    support sum from S_MIN"""
    params = OV_PARAMS[pi]
    x = ov_field(kind, ne)
    g = [np.random.default_rng(17 + v).uniform(-1.0, 1.0, x.size) for v in range(3)]
    fl = oref.forward(x, ne, build, LD, *params)
    S, sc = fl["S"], ov_scales(x, ne, build, fl, params)
    # no rounding may flip the branch at S_MIN: every S is further from it than 1024 times its own allowance (the cascade of a
    # void region over a solid one passes S_MIN wherever it happens to); on the tail field, built for it, by a factor 2
    near = np.abs(S - LD(oref.S_MIN)) <= 1024 * C_OV_COEF * LD(EPS) * sc["S"]
    if kind == "tail":
        near |= (S >= LD(oref.S_MIN) / 2) & (S < LD(oref.S_MIN) * 2)
    assert not near.any(), "%s %s %s: %d support sums too close to S_MIN" % (ne, build, kind, int(near.sum()))
    nl = oref.layers(x, ne, build).shape[0]
    return dict(ne=ne, build=build, kind=kind, params=params, x=x, g=g, fl=fl, scale=sc, nl=nl,
                label="overhang %s %s %s P=%g eps=%g xi0=%g" % ("x".join(map(str, ne)), build, kind, *params))


def ov_hold(case, xi, a, w, p, outs, div=1, tag=""):
    """xi and the stored coefficients against the 80-bit forward, the transposes `outs` of case["g"] against the 80-bit recursion
    on the coefficients (a, w, p) handed in.  div = 4: the oracle's quarter.  -> the achieved c per quantity"""
    ne, build, fl, sc = case["ne"], case["build"], case["fl"], case["scale"]
    wh = lambda q: {"label": "%s%s %s" % (tag, case["label"], q), "dims": ne, "dof": 0}
    got = dict(xi=hold(xi, fl["xi"], sc["xi"], C_OV_XI / div, wh("xi")), a=hold(a, fl["a"], sc["a"], C_OV_COEF / div, wh("a")),
               w=hold(w, fl["w"], sc["w"], C_OV_COEF / div, wh("w")))
    hold(p, fl["p"], sc["p"], C_OV_POW / div, wh("p"), floor=OV_FLOOR)
    big = fl["p"] >= LD(2.0) ** -960        # the figure reported for p: the rows the floor has no part in
    got["p"] = rw.achieved(np.asarray(p)[big], fl["p"][big], sc["p"][big].astype(np.float64))
    co = {k: np.asarray(v, dtype=np.float64).astype(LD) for k, v in (("a", a), ("w", w), ("p", p))}
    assert all((v >= 0).all() for v in co.values()), wh("coefficients")["label"]
    got["adj"] = 0.0
    for v, o in enumerate(outs):
        ref = oref.adjoint(co, case["g"][v], ne, build)
        scale = oref.adjoint(co, np.abs(case["g"][v]), ne, build)
        got["adj"] = max(got["adj"], hold(o, ref, scale, c_ov_adj(case["nl"]) / div, wh("transpose %d" % v)))
    return got


# =====================================================================================================================
# casting
# =====================================================================================================================
# c.  Count per cell: d, d d, + eps, sqrt, x + c_prev, + rho (the halving is exact): 6 -> 8.  Measured over CAST_CASES: 0.96
# (x 16 = 15.3 -> 16).
C_CAST_C = 16
# q.  d, d d, + eps, sqrt, the division: 5 -> 8.  Measured: 2.29 (x 16 = 36.6 -> 64).
C_CAST_Q = 64
CAST_MESHES = cref.MESHES
CAST_FIELDS = tuple(cref.FIELDS) + DESIGNS
CAST_XFORMS = (1, 0)


def c_cast_adj(n):
    """the transpose along a sweep of at most n cells from given q.  Count: 3 roundings per cell (1 - q, the product with mu, the
    addition of g; the halving is exact) and 1 + q and its product: 3 n + 2 -> 8 / 16 / 32 / 64 / 128 / 256 for 1 / 3, 4 / 5 / 11,
    12, 20 / 33, 37 / 70 cells.  Measured: 6.71 (x 16 = 107 -> 128): the measured value sets the constant up to 37 cells, the
    count at 70."""
    return max(128, rw.pow2(3 * n + 2))


def cast_field(kind, ne, draw):
    return design01(kind, ne) if kind in DESIGNS else cref.field(kind, ne, draw)


def cast_scales(x, ne, draw, fl, eps=cref.EPS):
    eps_ = LD(eps)
    rx = LD(C_CAST_C) / C_CAST_Q
    axis, p = cref.parse(draw, ne)
    out = {k: np.zeros(x.size, dtype=LD) for k in ("c", "q")}
    X, Cv = cref.lines(np.asarray(x).astype(LD), ne, axis), cref.lines(fl["c"], ne, axis)
    E, SQ = cref.lines(out["c"], ne, axis), cref.lines(out["q"], ne, axis)
    for ks in cref._sweeps(ne[axis], p):
        for j in range(1, len(ks)):
            k, kp = ks[j], ks[j - 1]
            d = X[k] - Cv[kp]
            rho = np.sqrt(d * d + eps_)
            q = d / rho
            loc = np.abs(X[k]) + np.abs(Cv[kp])
            E[k] = (loc + rho) + LD(0.5) * (1 - q) * E[kp]
            SQ[k] = np.abs(q) + (eps_ / rho ** 3) * (loc + rx * E[kp])
    return out


@functools.lru_cache(maxsize=32)
def cast_case(ne, draw, kind):
    x = cast_field(kind, ne, draw)
    g = [np.random.default_rng(17 + v).uniform(-1.0, 1.0, x.size) for v in range(3)]
    fl = cref.forward(x, ne, draw, LD)
    return dict(ne=ne, draw=draw, kind=kind, x=x, g=g, fl=fl, scale=cast_scales(x, ne, draw, fl), n=ne[cref.parse(draw, ne)[0]],
                label="casting %s %s %s" % (cref.name(ne), draw, kind))


def cast_hold(case, c, q, outs, div=1, tag=""):
    ne, draw, fl, sc = case["ne"], case["draw"], case["fl"], case["scale"]
    wh = lambda s: {"label": "%s%s %s" % (tag, case["label"], s), "dims": ne, "dof": 0}
    got = dict(c=hold(c, fl["c"], sc["c"], C_CAST_C / div, wh("c")), q=hold(q, fl["q"], sc["q"], C_CAST_Q / div, wh("q")))
    qd = np.asarray(q, dtype=np.float64).astype(LD)
    assert (np.abs(qd) <= 1).all(), wh("q")["label"]
    got["adj"] = 0.0
    for v, o in enumerate(outs):
        ref = cref.adjoint(dict(q=qd), case["g"][v], ne, draw)
        scale = cref.adjoint(dict(q=qd), np.abs(case["g"][v]), ne, draw)
        got["adj"] = max(got["adj"], hold(o, ref, scale, c_cast_adj(case["n"]) / div, wh("transpose %d" % v)))
    return got


# =====================================================================================================================
# local volume
# =====================================================================================================================
LV_MESHES = {
    "a": ((16, 8, 8), (0.125, 0.125, 0.125), 2.5 * 0.125),        # conn 2: tiled (and z-multi in a child process)
    "b": ((20, 12, 8), (0.05, 0.04, 0.03), 0.11),                  # conn 3: wide
    "c": ((20, 20, 20), (0.05, 0.05, 0.05), 9.5 * 0.05),           # conn 9: streamed ring
    "d": ((3, 3, 3), (0.25, 0.25, 0.25), 1.5 * 0.25),              # conn 1: generic, in a child process
}
LV_FIELDS = ("random", "checker", "half") + DESIGNS
LV_PS = (1.0, 16.0)
LV_ALPHA = 0.6


def lv_field(kind, ne):
    return design01(kind, ne) if kind in DESIGNS else lvref.field(kind, ne)


def c_lv(conn, p):
    """(rhobar, dgdx): the counts of localvol_ref.bounds in units of eps -- taps + 8 and (p + 1)(taps + 8) 2 -- rounded up to
    powers of two: rhobar 64 / 256 / 512 / 8192 at conn 1 / 2 / 3 / 9, dgdx at p = 1 four times and at p = 16 32 times that.
    float64 restatement against the 80-bit one, measured over LV_MESHES, LV_FIELDS, LV_PS, (rhobar, dgdx) per mesh: d 2.47, 39.5;
    a 6.62, 46.3; b 9.09, 56.7; c 40.8, 189 -- x 16 = 40, 631; 106, 740; 145, 907; 653, 3018, every one below its count (35,
    1190; 133, 4522; 351, 11934; 6867, 233478 at p = 16; at p = 1 dgdx measures 0.83, 9.41, 12.4, 56.5 against 140 .. 27468)."""
    b = lvref.bounds(conn, p)
    return rw.pow2(b["rb"] / EPS), rw.pow2(b["dgdx"] / EPS)


@functools.lru_cache(maxsize=32)
def lv_case(ne, h, R, kind, p, alpha=LV_ALPHA):
    rho = lv_field(kind, ne)
    ref = lvref.reference(rho, ne, h, R, alpha, p)
    conn = lvref.stencil_width(ne, h, R)
    return dict(ne=ne, rho=rho, ref=ref, conn=conn, p=p, c=c_lv(conn, p),
                label="local volume %s %s p=%g conn %d" % ("x".join(map(str, ne)), kind, p, conn))


def lv_hold(case, rb, dgdx, div=1, tag=""):
    """each row relative to its own value: the scale IS the reference"""
    ref, (c_rb, c_dg) = case["ref"], case["c"]
    wh = lambda s: {"label": "%s%s %s" % (tag, case["label"], s), "dims": case["ne"], "dof": 0}
    return dict(rb=hold(rb, ref["rb"], ref["rb"], c_rb / div, wh("rhobar")), dgdx=hold(dgdx, ref["dgdx"], ref["dgdx"], c_dg / div, wh("dgdx")))


# =====================================================================================================================
# length scale
# =====================================================================================================================
# T = a E m^2.  Count: on G the three differences, scalings and squares chained (3), two additions, the product with c (6, the
# factor of c G); exp, a (the void kind's 1 - rb), m, m m, two products (6, the factor of 1): 6 (1 + c G) -> 8.  Measured over
# LS_CASES: 3.68 (x 16 = 59 -> 64).
C_LS_T = 64
# dg.  Count: T's (6) + w T d of a stencil term (3), the six stencil terms and the two local ones summed (8), H' (tanh, square,
# difference, product, division: 5), the scaling by 1 / (n eps): 23 -> 32.  Measured: 3.73 (x 16 = 60 -> 64).
C_LS_DG = 64
LS_MESHES = lsref.MESHES
LS_FIELDS = tuple(lsref.KINDS) + DESIGNS
LS_PROJ = ((0, lsref.BETA), (1, lsref.BETA), (1, 64.0))       # (proj, beta)
LS_ETA_S, LS_ETA_V, LS_EPS = 0.75, 0.25, 1e-6


def ls_field(kind, ne, h):
    return design01(kind, ne) if kind in DESIGNS else lsref.field(kind, ne, h)


def ls_scales(rt, rb, ne, h, c, r80, proj, beta, eta=lsref.ETA, eta_s=LS_ETA_S, eta_v=LS_ETA_V, eps=LS_EPS):
    """-> {"T_solid", "T_void", "dg_solid", "dg_void"}: the absolute majorants of the module docstring"""
    n = rt.size
    rt, rb, c = np.asarray(rt).astype(LD), np.asarray(rb).astype(LD), LD(c)
    nb = lsref._neighbours(ne)
    d = [np.abs(rt[p] - rt[m]) for p, m in nb]
    amp = r80["E"] * (1 + c * r80["G"])
    if proj:
        th = np.tanh(LD(beta) * (rt - LD(eta)))
        hp = LD(beta) * (1 + th * th) / (np.tanh(LD(beta) * LD(eta)) + np.tanh(LD(beta) * (1 - LD(eta))))
    else:
        hp = np.ones(n, dtype=LD)
    out = {}
    for name, a, m in (("solid", np.abs(rb), np.minimum(rt - LD(eta_s), 0)), ("void", np.abs(1 - rb), np.minimum(LD(eta_v) - rt, 0))):
        T = a * amp * m * m
        st = np.zeros(n, dtype=LD)
        for ax in range(3):
            w = c * T * d[ax] / (2 * LD(h[ax]) ** 2)
            np.add.at(st, nb[ax][0], w)
            np.add.at(st, nb[ax][1], w)
        out["T_" + name] = T
        out["dg_" + name] = (hp * amp * m * m + 2 * a * amp * np.abs(m) + st) / (n * LD(eps))
    return out


@functools.lru_cache(maxsize=32)
def ls_case(mesh, kind, pj):
    ne, h = LS_MESHES[mesh]
    proj, beta = LS_PROJ[pj]
    rt = ls_field(kind, ne, h)
    rb = lsref.heaviside(rt, beta, lsref.ETA, np.float64) if proj else np.array(rt, dtype=np.float64)
    c = lsref.default_c(h)
    r80 = lsref.reference(rt, ne, h, c, LS_ETA_S, LS_ETA_V, LS_EPS, proj, beta, lsref.ETA, rb=rb)
    return dict(mesh=mesh, ne=ne, h=h, c=c, proj=proj, beta=beta, rt=rt, rb=rb, r80=r80,
                scale=ls_scales(rt, rb, ne, h, c, r80, proj, beta), label="length scale %s %s proj=%d beta=%g" % (mesh, kind, proj, beta))


def ls_hold(case, name, T, dg, div=1, tag=""):
    """name: "solid" or "void"; T, dg: that kind's terms and gradient"""
    wh = lambda s: {"label": "%s%s %s_%s" % (tag, case["label"], s, name), "dims": case["ne"], "dof": 0}
    r80, sc = case["r80"], case["scale"]
    return dict(T=hold(T, r80["T_" + name], sc["T_" + name], C_LS_T / div, wh("T")),
                dg=hold(dg, r80["dg_" + name], sc["dg_" + name], C_LS_DG / div, wh("dg")))


# =====================================================================================================================
# planted errors
# =====================================================================================================================
def plant(ref_ld, scale=None, candidates=None, below=1e-8, rel=PLANT):
    """the reference with ONE row multiplied by 1 + rel: the row of largest magnitude among those below `below` of the maximum
    -- with its scale below that too, where given: a row that is small because its terms are, not because they cancel -- (and
    among `candidates`, a boolean mask, where given) -> (array, row)"""
    ref_ld = np.asarray(ref_ld, dtype=LD)
    mag = np.abs(ref_ld)
    ok = (mag > 0) & (mag < LD(below) * mag.max())
    if scale is not None:
        ok &= np.asarray(scale, dtype=LD) < LD(below) * mag.max()
    if candidates is not None:
        ok &= candidates
    assert ok.any(), "no row below %g of the maximum" % below
    row = int(np.flatnonzero(ok)[np.argmax(mag[ok])])
    bad = ref_ld.copy()
    bad[row] = bad[row] * (1 + LD(rel))
    return bad, row
