"""numpy restatement of the overhang (self-support) filter (include/topopt_amd.h: tp_overhang), generic in the
dtype (double and np.longdouble), and the checks of the device against it that the GPU tests and the slab worker share.  Not a
test module.

Build axis a in {y, z}, sign +-; layer 0 lies on the baseplate (lowest index for +, highest for -); in-plane (i, r) = x and the
remaining axis.  P = 40, eps = 1e-4, xi0 = 0.5, Q = P + ln 5 / ln xi0.

    xi_0 = x_0;  l >= 1:  t = p * xi of layer l - 1,  p = xi^(P-1)
    S = t(i,r) + t(i-1,r) + t(i+1,r) + t(i,r-1) + t(i,r+1)        left to right, 0 outside the mesh
    Xi = S^(1/Q) (0 if S < S_MIN),  d = x - Xi,  rho = sqrt(d^2 + eps),  xi = ((x + Xi) - rho + sqrt(eps)) / 2
    a = (1 - d/rho) / 2,  w = ((1 + d/rho) / 2) * ((P/Q) * (Xi/S)) (0 if S < S_MIN),  p = xi^(P-1);  layer 0: a = 1, w = 0
    transpose, top layer first:  lambda_l = g_l + p_l * sum_5 (w lambda)_{l+1}  (same cross, same order),  out_l = a_l lambda_l

S_MIN = 2^-960 in every dtype: a support sum below it counts as no support, because Xi/S = S^(1/Q - 1) leaves float64's range
(P = 40: S < 4e-317) long before the Jacobian entry p w does.  The 80-bit restatement applies the same floor, so that both sides
take the same branch; the fields keep S a factor 2 away from it (tests/design_rowwise.py asserts that).

Fields are flat, x fastest, then y, then z, as the library's element vectors."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
BUILDS = {"+y": (1, 1), "-y": (1, -1), "+z": (2, 1), "-z": (2, -1)}
P, EPS, XI0 = 40.0, 1e-4, 0.5
S_MIN = 2.0 ** -960


def layers(flat, ne, build):
    """view of a flat field as [layer, r, i], layer 0 on the baseplate"""
    ex, ey, ez = ne
    axis, sign = BUILDS[build]
    a = np.asarray(flat).reshape(ez, ey, ex)
    v = a if axis == 2 else np.moveaxis(a, 1, 0)
    return v if sign > 0 else v[::-1]


def _cross(t):
    """the five-term sum, in the order of the kernels"""
    tp = np.zeros((t.shape[0] + 2, t.shape[1] + 2), dtype=t.dtype)
    tp[1:-1, 1:-1] = t
    return (((tp[1:-1, 1:-1] + tp[1:-1, :-2]) + tp[1:-1, 2:]) + tp[:-2, 1:-1]) + tp[2:, 1:-1]


def forward(x, ne, build, dtype=LD, P=P, eps=EPS, xi0=XI0, s_min=S_MIN):
    """-> dict(xi, Xi, S, a, w, p), flat; Xi of layer 0 is set to x (it has no support term), its S to 0.  s_min = 0 is the
    filter without the floor (S != 0), kept for the regression test of the floor"""
    T = dtype
    P_, eps_ = T(P), T(eps)
    Q = P_ + np.log(T(5)) / np.log(T(xi0))
    invQ, PoverQ, sqeps, Pm1 = 1 / Q, P_ / Q, np.sqrt(eps_), P_ - 1
    x = np.asarray(x).astype(T)
    out = {k: np.zeros(x.size, dtype=T) for k in ("xi", "Xi", "S", "a", "w", "p")}
    X = layers(x, ne, build)
    V = {k: layers(v, ne, build) for k, v in out.items()}
    V["xi"][0], V["Xi"][0], V["a"][0], V["w"][0] = X[0], X[0], 1, 0
    V["p"][0] = X[0] ** Pm1
    for l in range(1, X.shape[0]):
        S = _cross(V["p"][l - 1] * V["xi"][l - 1])
        nz = (S >= T(s_min)) & (S != 0)
        Ss = np.where(nz, S, T(1))
        Xi = np.where(nz, Ss ** invQ, T(0))
        sw = np.where(nz, PoverQ * (Xi / Ss), T(0))
        d = X[l] - Xi
        rho = np.sqrt(d * d + eps_)
        xi = T(0.5) * (((X[l] + Xi) - rho) + sqeps)
        q = d / rho
        V["xi"][l], V["Xi"][l], V["S"][l] = xi, Xi, S
        V["a"][l] = T(0.5) * (1 - q)
        V["w"][l] = (T(0.5) * (1 + q)) * sw
        V["p"][l] = xi ** Pm1
    return out


def adjoint(f, g, ne, build):
    """J^T g from the coefficients of forward()"""
    T = f["a"].dtype
    out = np.zeros(f["a"].size, dtype=T)
    G, O = layers(np.asarray(g).astype(T), ne, build), layers(out, ne, build)
    A, W, Pc = (layers(f[k], ne, build) for k in ("a", "w", "p"))
    m = np.zeros_like(G[0])
    for l in range(G.shape[0] - 1, -1, -1):
        lam = G[l] + Pc[l] * _cross(m)
        O[l] = A[l] * lam
        m = W[l] * lam
    return out


def field(kind, ne, seed=3):
    ex, ey, ez = ne
    n = ex * ey * ez
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(0.0, 1.0, n)
    if kind == "mid":
        return rng.uniform(0.1, 0.9, n)
    if kind == "checker":
        k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
        return ((i + j + k) % 2).astype(np.float64).ravel()
    if kind == "half":
        return np.full(n, 0.5)
    if kind == "ones":
        return np.ones(n)
    if kind == "zerolayers":   # whole zero layers along z (the baseplate layer among them) and, on taller meshes, along y
        a = rng.uniform(0.0, 1.0, n).reshape(ez, ey, ex)
        a[[k for k in (0, 3, 4) if k < ez]] = 0.0
        if ey > 4:
            a[:, [0, 2]] = 0.0
        return a.ravel()
    raise ValueError(kind)


def sandwich_breach(x, f, eps=EPS):
    """how far xi leaves [min(x, Xi), min(x, Xi) + sqrt(eps)/2], layer 0 (xi = x) included; <= 0 means inside"""
    lo = np.minimum(np.asarray(x).astype(f["xi"].dtype), f["Xi"])
    return float(max((lo - f["xi"]).max(), (f["xi"] - lo - np.sqrt(f["xi"].dtype.type(eps)) / 2).max()))


_cache = {}


def references(ne, build, kind):
    """(x, g[3], forward in 80-bit, forward in double, J^T g in 80-bit [3], in double [3]); computed once, not to be modified"""
    key = (tuple(ne), build, kind)
    if key not in _cache:
        x = field(kind, ne)
        n = x.size
        g = [np.random.default_rng(17 + v).uniform(-1.0, 1.0, n) for v in range(3)]
        fl, fd = forward(x, ne, build, LD), forward(x, ne, build, np.float64)
        _cache[key] = (x, g, fl, fd, [adjoint(fl, gv, ne, build) for gv in g], [adjoint(fd, gv, ne, build) for gv in g])
    return _cache[key]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def check_against_reference(tp, ne, build, kind):
    """The device against the 80-bit restatement.  The bound is the double restatement's own distance d from the 80-bit one on
    the same input, times 16, with a floor of 64 * 2^-53: xi absolute, the transpose relative to its maximum.  Also the
    sandwich property and the absence of NaN on the device's output.  Then row by row (tests/design_rowwise.py): xi, the stored
    coefficients a, w, p and the transposes, the latter against the 80-bit recursion on the device's own coefficients.
    -> the figures"""
    from tests import design_rowwise as dr
    x, g, fl, fd, al, ad = references(ne, build, kind)
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0 / ne[1])
    try:
        ov = tp.Overhang(grid, build)
        xi = grid.elem_vec()
        ov.Forward(dev(x), xi)
        gv = [dev(v) for v in g]
        ov.Adjoint(gv)
        xi_h = xi.cpu().numpy()
        out_h = [v.cpu().numpy() for v in gv]
        coef_h = [v.cpu().numpy() for v in ov.Coefficients()]
    finally:
        grid.close()
    d_xi = float(np.abs(fd["xi"].astype(LD) - fl["xi"]).max())
    e_xi = float(np.abs(xi_h.astype(LD) - fl["xi"]).max())
    b_xi = max(16 * d_xi, 64 * U53)
    print("%s %s %s: xi: double restatement off the 80-bit one by d = %.3e, device by %.3e (bound %.3e)"
          % ("x".join(map(str, ne)), build, kind, d_xi, e_xi, b_xi))
    res = [(e_xi, b_xi)]
    for v in range(3):
        mx = float(np.abs(al[v]).max())
        d_a = float(np.abs(ad[v].astype(LD) - al[v]).max()) / mx
        e_a = float(np.abs(out_h[v].astype(LD) - al[v]).max()) / mx
        b_a = max(16 * d_a, 64 * U53)
        print("    transpose of vector %d (max %.3e): double off by d = %.3e, device by %.3e (bound %.3e)" % (v, mx, d_a, e_a, b_a))
        res.append((e_a, b_a))
    assert np.isfinite(xi_h).all() and all(np.isfinite(o).all() for o in out_h)
    # the sandwich on the device's xi against Xi of the 80-bit restatement: both sides carry a few roundings of numbers
    # below 2, and Xi moves with xi of the layer below by at most its error bound
    br = sandwich_breach(x, dict(xi=xi_h.astype(LD), Xi=fl["Xi"]))
    print("    sandwich: device xi leaves [min(x, Xi), min(x, Xi) + sqrt(eps)/2] by %.3e (allowed: the bound on xi, %.3e)" % (br, b_xi))
    assert br <= b_xi
    for e, b in res:
        assert e <= b
    case = dr.ov_case(tuple(ne), build, kind, 0)
    assert np.array_equal(case["x"], x) and all(np.array_equal(a, b) for a, b in zip(case["g"], g))
    got = dr.ov_hold(case, xi_h, *coef_h, out_h)
    print("    row-wise, achieved c (bound): xi %.2f (%g), a %.2f, w %.2f (%g), p %.2f (%g), transposes %.2f (%g)"
          % (got["xi"], dr.C_OV_XI, got["a"], got["w"], dr.C_OV_COEF, got["p"], dr.C_OV_POW, got["adj"], dr.c_ov_adj(case["nl"])))
    return res
