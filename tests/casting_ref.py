"""numpy restatement of the casting (draw-direction) filter (include/topopt_amd.h: tp_casting), generic in the
dtype (double and np.longdouble), and the checks of the device against it that the GPU tests and the slab worker share.  Not a
test module.

Draw axis a in {x, y, z} with n element layers k = 0 .. n-1 and a parting index p in [0, n]: "+a" is p = 0, "-a" is p = n, "a:K"
is p = K.  Upper range k >= p, swept from k = n-1 down to p; the lower range k < p is the mirror image, swept from k = 0 up:

    c_first = x_first, q_first = 1;   d = x_k - c_prev,  rho = sqrt(d*d + eps),  c_k = 0.5 * ((x_k + c_prev) + rho),  q_k = d / rho
    transpose, against the sweep:  mu_first' = g_first';  out_k = (0.5 * (1 + q_k)) * mu_k,  mu_next = g_next + (0.5 * (1 - q_k)) * mu_k

the same operations in the same order as cast_cell_fwd and cast_cell_adj (csrc/casting.h).  Fields are flat, x fastest, then y,
then z, as the library's element vectors."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
EPS = 1e-6
AXES = {"x": 0, "y": 1, "z": 2}
MESHES = [(70, 37, 11), (33, 5, 3), (16, 12, 20), (3, 3, 3), (4, 1, 1), (1, 1, 4)]
FIELDS = ["random", "checker", "zerolayers"]


def parse(draw, ne):
    """-> (axis, p)"""
    if draw[0] in "+-":
        axis = AXES[draw[1]]
        return axis, (0 if draw[0] == "+" else ne[axis])
    axis, p = AXES[draw[0]], int(draw[2:])
    assert draw[1] == ":" and 1 <= p <= ne[axis] - 1, draw
    return axis, p


def draws(ne):
    """all six one-sided draws, and per axis the two-sided ones at p = 1, n - 1 and a mid index off any tile edge (33 on 70)"""
    out = []
    for name, axis in AXES.items():
        n = ne[axis]
        out += ["+" + name, "-" + name]
        for p in sorted({1, n - 1, 33 if n == 70 else n // 2}):
            if 1 <= p <= n - 1:
                out.append("%s:%d" % (name, p))
    return out


def lines(flat, ne, axis):
    """view of a flat field as [layer along the axis, ...]"""
    ex, ey, ez = ne
    a = np.asarray(flat).reshape(ez, ey, ex)
    return a if axis == 2 else np.moveaxis(a, 1 if axis == 1 else 2, 0)


def swap(flat, ne, a, b):
    """the field with the axes a and b exchanged -> (flat, ne)"""
    if a == b:
        return np.ascontiguousarray(flat), tuple(ne)
    v = np.asarray(flat).reshape(ne[2], ne[1], ne[0])
    v = np.swapaxes(v, 2 - a, 2 - b)
    n2 = list(ne)
    n2[a], n2[b] = ne[b], ne[a]
    return np.ascontiguousarray(v).ravel(), tuple(n2)


def _sweeps(n, p):
    """the forward sweeps' layer orders: upper range downwards, lower range upwards"""
    return [list(range(n - 1, p - 1, -1)), list(range(0, p))]


def forward(x, ne, draw, dtype=LD, eps=EPS):
    """-> dict(c, q), flat"""
    T = dtype
    axis, p = parse(draw, ne)
    eps_, half = T(eps), T(0.5)
    x = np.asarray(x).astype(T)
    out = {k: np.zeros(x.size, dtype=T) for k in ("c", "q")}
    X, Cv, Qv = lines(x, ne, axis), lines(out["c"], ne, axis), lines(out["q"], ne, axis)
    for ks in _sweeps(ne[axis], p):
        prev = None
        for k in ks:
            if prev is None:
                Cv[k], Qv[k] = X[k], 1
            else:
                d = X[k] - prev
                rho = np.sqrt(d * d + eps_)
                Cv[k] = half * ((X[k] + prev) + rho)
                Qv[k] = d / rho
            prev = Cv[k].copy()
    return out


def adjoint(f, g, ne, draw):
    """J^T g from the coefficients of forward()"""
    T = f["q"].dtype.type
    axis, p = parse(draw, ne)
    half, one = T(0.5), T(1)
    out = np.zeros(f["q"].size, dtype=T)
    G, O, Q = lines(np.asarray(g).astype(T), ne, axis), lines(out, ne, axis), lines(f["q"], ne, axis)
    for ks in _sweeps(ne[axis], p):
        t = None
        for k in reversed(ks):
            mu = G[k] if t is None else G[k] + t
            O[k] = (half * (one + Q[k])) * mu
            t = (half * (one - Q[k])) * mu
    return out


def hardmax(x, ne, draw):
    """the hard filter: running maximum from the sweep's start, and the number of steps m from there, both flat"""
    axis, p = parse(draw, ne)
    x = np.asarray(x)
    h, m = np.zeros(x.size, dtype=x.dtype), np.zeros(x.size)
    X, H, M = lines(x, ne, axis), lines(h, ne, axis), lines(m, ne, axis)
    for ks in _sweeps(ne[axis], p):
        for j, k in enumerate(ks):
            H[k] = X[k] if j == 0 else np.maximum(X[k], H[ks[j - 1]])
            M[k] = j
    return h, m


def sandwich_breach(x, c, ne, draw, eps=EPS):
    """how far c leaves [hardmax, hardmax + m sqrt(eps)/2], m the steps from the sweep's start; <= 0 means inside"""
    T = c.dtype.type
    h, m = hardmax(np.asarray(x).astype(T), ne, draw)
    return float(max((h - c).max(), (c - h - m.astype(T) * np.sqrt(T(eps)) / 2).max()))


def monotone_breach_ulps(c, ne, draw):
    """the largest rise of c along a sweep (exact arithmetic: none) in units of the spacing of c's dtype at that value"""
    axis, p = parse(draw, ne)
    Cv = lines(c, ne, axis)
    worst = 0.0
    for ks in _sweeps(ne[axis], p):
        for j in range(1, len(ks)):
            rise = (Cv[ks[j - 1]] - Cv[ks[j]]) / np.spacing(np.abs(Cv[ks[j]]) + np.finfo(c.dtype).tiny)
            worst = max(worst, float(rise.max()))
    return worst


def field(kind, ne, draw="+z", seed=3):
    ex, ey, ez = ne
    n = ex * ey * ez
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(0.0, 1.0, n)
    if kind == "checker":
        k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
        return ((i + j + k) % 2).astype(np.float64).ravel()
    if kind == "zerolayers":   # every third layer along the draw axis zero, the sweep's first among them
        a = rng.uniform(0.0, 1.0, n)
        lines(a, ne, parse(draw, ne)[0])[::3] = 0.0
        return a
    if kind == "ones":
        return np.ones(n)
    if kind == "uniform":
        return np.full(n, 0.12)
    raise ValueError(kind)


_cache = {}


def references(ne, draw, kind, eps=EPS):
    """(x, g[3], forward in 80-bit, forward in double, J^T g in 80-bit [3], in double [3]); computed once, not to be modified"""
    key = (tuple(ne), draw, kind, eps)
    if key not in _cache:
        x = field(kind, ne, draw)
        g = [np.random.default_rng(17 + v).uniform(-1.0, 1.0, x.size) for v in range(3)]
        fl, fd = forward(x, ne, draw, LD, eps), forward(x, ne, draw, np.float64, eps)
        _cache[key] = (x, g, fl, fd, [adjoint(fl, gv, ne, draw) for gv in g], [adjoint(fd, gv, ne, draw) for gv in g])
    return _cache[key]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def name(ne):
    return "x".join(map(str, ne))


def check_against_reference(tp, grid, ne, draw, kind):
    """The device against the 80-bit restatement.  The bound is the double restatement's own distance d from the 80-bit one on
    the same input, times 16, with a floor of 64 * 2^-53: c absolute, the transpose relative to its maximum.  Also the sandwich,
    monotonicity to 4 ulp and the absence of NaN on the device's output.  Then row by row (tests/design_rowwise.py): c, the
    stored q and the transposes, the latter against the 80-bit recursion on the device's own q.  -> the figures"""
    from tests import design_rowwise as dr
    x, g, fl, fd, al, ad = references(ne, draw, kind)
    cf = tp.Casting(grid, draw)
    try:
        c = grid.elem_vec()
        cf.Forward(dev(x), c)
        gv = [dev(v) for v in g]
        cf.Adjoint(gv)
        c_h = c.cpu().numpy()
        out_h = [v.cpu().numpy() for v in gv]
        q_h = cf.Q().cpu().numpy()
    finally:
        cf.close()
    d_c = float(np.abs(fd["c"].astype(LD) - fl["c"]).max())
    e_c = float(np.abs(c_h.astype(LD) - fl["c"]).max())
    b_c = max(16 * d_c, 64 * U53)
    print("%s %s %s: c: double restatement off the 80-bit one by d = %.3e, device by %.3e (bound %.3e)"
          % (name(ne), draw, kind, d_c, e_c, b_c))
    res = [(e_c, b_c)]
    for v in range(3):
        mx = float(np.abs(al[v]).max())
        d_a = float(np.abs(ad[v].astype(LD) - al[v]).max()) / mx
        e_a = float(np.abs(out_h[v].astype(LD) - al[v]).max()) / mx
        b_a = max(16 * d_a, 64 * U53)
        print("    transpose of vector %d (max %.3e): double off by d = %.3e, device by %.3e (bound %.3e)" % (v, mx, d_a, e_a, b_a))
        res.append((e_a, b_a))
    assert np.isfinite(c_h).all() and all(np.isfinite(o).all() for o in out_h)
    # the sandwich on the device's c: its two sides are exact in exact arithmetic, and c carries the error bounded above
    br = sandwich_breach(x, c_h.astype(LD), ne, draw)
    mono = monotone_breach_ulps(c_h, ne, draw)
    print("    sandwich: device c leaves [hardmax, hardmax + m sqrt(eps)/2] by %.3e (allowed: the bound on c, %.3e); largest rise "
          "along a sweep %.2f ulp (allowed 4)" % (br, b_c, mono))
    assert br <= b_c
    assert mono <= 4.0
    for e, b in res:
        assert e <= b
    case = dr.cast_case(tuple(ne), draw, kind)
    assert np.array_equal(case["x"], x) and all(np.array_equal(a, b) for a, b in zip(case["g"], g))
    got = dr.cast_hold(case, c_h, q_h, out_h)
    print("    row-wise, achieved c (bound): c %.2f (%g), q %.2f (%g), transposes %.2f (%g)"
          % (got["c"], dr.C_CAST_C, got["q"], dr.C_CAST_Q, got["adj"], dr.c_cast_adj(case["n"])))
    return res
