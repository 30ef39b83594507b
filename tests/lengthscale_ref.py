"""numpy restatement of the geometric length-scale constraints (include/topopt_amd.h: tp_lengthscale), in 80-bit arithmetic by
default and through the same code in float64, and the fields and bounds the CPU and GPU tests share.  Not a test module.

    e+_a = min(i_a + 1, n_a - 1),  e-_a = max(i_a - 1, 0),  d_{a,e} = rt[e+_a] - rt[e-_a]
    G_e = sum_a (d_{a,e} / (2 h_a))^2,  E_e = exp(-c G_e)
    solid: a = rb, m = min(rt - eta_s, 0), a' = H'(rt), m' = 1;   void: a = 1 - rb, m = min(eta_v - rt, 0), a' = -H'(rt), m' = -1
    T_e = a_e E_e m_e^2,  S = sum_e T_e,  g = S / (n eps) - 1
    dS/drt_j = a'_j E_j m_j^2 + 2 a_j E_j m_j m'_j + sum_a (sum_{e: e+_a = j} w_{a,e} - sum_{e: e-_a = j} w_{a,e}),
    w_{a,e} = -c T_e d_{a,e} / (2 h_a^2),  dg/drt = dS/drt / (n eps)
    H(rt) = (tanh(beta eta) + tanh(beta (rt - eta))) / (tanh(beta eta) + tanh(beta (1 - eta))),  proj = 0: rb = rt, H' = 1

The stencil term is formed as its definition reads: every element e adds w_{a,e} at e+_a and subtracts it at e-_a (a scatter; the
library gathers).  Fields are flat, x fastest."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
FLOOR = 64 * U53
BETA, ETA = 8.0, 0.5          # the projection of the cases with proj = 1
# (elements, h): the meshes of tests/test_gpu_lengthscale.py
MESHES = {
    "a": ((16, 8, 8), (0.125, 0.125, 0.125)),      # baseline
    "b": ((20, 12, 8), (0.05, 0.04, 0.03)),        # not aligned to a workgroup or tile; anisotropic
    "c": ((3, 3, 3), (0.25, 0.25, 0.25)),          # every element touches the boundary
    "d": ((5, 2, 7), (0.2, 0.2, 0.2)),             # along y, e+ and e- are both clamped for every element
    "e": ((7, 1, 5), (0.2, 0.2, 0.2)),             # d_y = 0
    "f": ((70, 5, 3), (0.1, 0.1, 0.1)),            # an x extent above one wave
}
KINDS = ("random", "checker", "half")


def default_c(h):
    """c = (2.5 h_min)^4 / h_min^2: the paper's c = r^4 for a filter radius of 2.5 elements"""
    hm = min(h)
    return (2.5 * hm) ** 4 / hm ** 2


def heaviside(rt, beta, eta, dtype=LD):
    rt, beta, eta = np.asarray(rt).astype(dtype), dtype(beta), dtype(eta)
    return (np.tanh(beta * eta) + np.tanh(beta * (rt - eta))) / (np.tanh(beta * eta) + np.tanh(beta * (1 - eta)))


def heaviside_prime(rt, beta, eta, dtype=LD):
    rt, beta, eta = np.asarray(rt).astype(dtype), dtype(beta), dtype(eta)
    th = np.tanh(beta * (rt - eta))
    return beta * (1 - th * th) / (np.tanh(beta * eta) + np.tanh(beta * (1 - eta)))


def _neighbours(ne):
    """per axis (x, y, z): flat indices of e+_a and e-_a for every element"""
    ex, ey, ez = ne
    k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
    flat = lambda ii, jj, kk: (ii + ex * (jj + ey * kk)).ravel()
    return [(flat(np.minimum(i + 1, ex - 1), j, k), flat(np.maximum(i - 1, 0), j, k)),
            (flat(i, np.minimum(j + 1, ey - 1), k), flat(i, np.maximum(j - 1, 0), k)),
            (flat(i, j, np.minimum(k + 1, ez - 1)), flat(i, j, np.maximum(k - 1, 0)))]


def reference(rt, ne, h, c, eta_s=0.75, eta_v=0.25, eps=1e-6, proj=0, beta=BETA, eta=ETA, rb=None, dtype=LD):
    """-> dict(G, E, T_solid, T_void, S_*, g_*, dg_*, stencil_*); rb: the projected field where the caller has one (the device is
    given one in float64), else H(rt) in `dtype`"""
    n = ne[0] * ne[1] * ne[2]
    rt = np.asarray(rt).astype(dtype)
    c, eps = dtype(c), dtype(eps)
    if rb is None:
        rb = heaviside(rt, beta, eta, dtype) if proj else rt
    rb = np.asarray(rb).astype(dtype)
    hp = heaviside_prime(rt, beta, eta, dtype) if proj else np.ones(n, dtype=dtype)
    nb = _neighbours(ne)
    d = [rt[p] - rt[m] for p, m in nb]
    G = sum((d[a] / (2 * dtype(h[a]))) ** 2 for a in range(3))
    E = np.exp(-c * G)
    out = dict(G=G, E=E)
    for name, a, m, ap, mp in (("solid", rb, np.minimum(rt - dtype(eta_s), 0), hp, 1),
                               ("void", 1 - rb, np.minimum(dtype(eta_v) - rt, 0), -hp, -1)):
        T = a * E * m * m
        S = T.sum()
        st = np.zeros(n, dtype=dtype)
        for ax in range(3):
            w = -c * T * d[ax] / (2 * dtype(h[ax]) ** 2)
            np.add.at(st, nb[ax][0], w)
            np.add.at(st, nb[ax][1], -w)
        dS = ap * E * m * m + 2 * a * E * m * mp + st
        out["T_" + name], out["S_" + name], out["g_" + name] = T, S, S / (n * eps) - 1
        out["dg_" + name], out["stencil_" + name] = dS / (n * eps), st
    return out


# ---- the fields of the tests: xTilde (element order: x fastest) ----
def cone_filter(x, ne, h, R):
    """density filter with the cone weights max(R - |c_i - c_j|, 0), truncated at the boundary and normalised (numpy, float64)"""
    ex, ey, ez = ne
    a = np.asarray(x, dtype=np.float64).reshape(ez, ey, ex)
    num, den = np.zeros_like(a), np.zeros_like(a)
    cx, cy, cz = (int(np.ceil(R / hd)) for hd in h)
    for dk in range(-cz, cz + 1):
        for dj in range(-cy, cy + 1):
            for di in range(-cx, cx + 1):
                w = R - np.sqrt((di * h[0]) ** 2 + (dj * h[1]) ** 2 + (dk * h[2]) ** 2)
                x0, x1, y0, y1, z0, z1 = max(0, -di), min(ex, ex - di), max(0, -dj), min(ey, ey - dj), max(0, -dk), min(ez, ez - dk)
                if w <= 0 or x0 >= x1 or y0 >= y1 or z0 >= z1:
                    continue
                num[z0:z1, y0:y1, x0:x1] += w * a[z0 + dk:z1 + dk, y0 + dj:y1 + dj, x0 + di:x1 + di]
                den[z0:z1, y0:y1, x0:x1] += w
    return (num / den).ravel()


def field(kind, ne, h, seed=3):
    ex, ey, ez = ne
    n = ex * ey * ez
    k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
    R = 2.5 * min(h)
    if kind == "random":
        return np.random.default_rng(seed).uniform(0.05, 0.95, n)
    if kind == "checker":   # 0/1 checkerboard of 2^3 blocks through the density filter
        return cone_filter((((i // 2) + (j // 2) + (k // 2)) % 2).astype(np.float64).ravel(), ne, h, R)
    if kind == "half":      # a step from 0.1 to 0.9 across the middle of x through the density filter
        return cone_filter(np.where(i < ex // 2, 0.1, 0.9).astype(np.float64).ravel(), ne, h, R)
    raise ValueError(kind)


def projected(rt, proj):
    """what the device is given as xPhys: H(xTilde) in float64, or xTilde itself"""
    return heaviside(rt, BETA, ETA, np.float64) if proj else np.array(rt, dtype=np.float64)


def distance(a, b, rel_to_max=False):
    """|a - b| of two scalars relative to |b|, or the largest |a - b| of two arrays relative to max |b|"""
    if rel_to_max:
        mx = float(np.abs(b).max())
        return float(np.abs(np.asarray(a).astype(LD) - b).max()) / mx if mx != 0 else float(np.abs(a).max())
    return float(abs(LD(a) - b) / abs(b)) if b != 0 else float(abs(a))


def d64_bounds(rt, rb, ne, h, c, proj, r80=None, **kw):
    """Distance of the float64 restatement from the 80-bit one for S, g (relative) and dg, T (relative to the largest entry), times
    16 -- the margin for two correct float64 evaluations that differ by their summation order and their exp / tanh -- and never
    below 64 * 2^-53.  -> (bounds, the 80-bit results)"""
    r80 = r80 or reference(rt, ne, h, c, proj=proj, rb=rb, **kw)
    r64 = reference(rt, ne, h, c, proj=proj, rb=rb, dtype=np.float64, **kw)
    b = {}
    for name in ("solid", "void"):
        for key in ("S_", "g_"):
            b[key + name] = max(16 * distance(r64[key + name], r80[key + name]), FLOOR)
        for key in ("dg_", "T_"):
            b[key + name] = max(16 * distance(r64[key + name], r80[key + name], True), FLOOR)
    return b, r80
