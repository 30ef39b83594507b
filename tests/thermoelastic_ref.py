"""Reference pieces of the thermoelastic tests in plain numpy (a helper module: no fixtures, no collection hooks): the coupling
matrix G in closed form and by Gauss quadrature, the interpolation beta of the thermal stress coefficient, the thermal load, its
transpose and its partial sensitivity as dense passes over the elements in float64 or numpy.longdouble, their row scales, the
constants of the row-wise bounds, and the coupled compliance with its gradient by sparse direct solves of both state problems.

Row-wise bounds follow tests/rowwise.py:  |got_i - arbiter_i| <= c 2^-53 scale_i,  scale_i the same pass on |theta|, |v|, |G|,
|beta| with all-ones N, c the larger of the operation count of the row's chain and 16 x what the float64 forms here measure
against the longdouble ones on the CPU, rounded up to a power of two.  tests/test_thermoelastic_oracle.py holds the float64 forms
to a QUARTER of every constant on every mesh and design below; the measured values stand beside the counts.
"""
import numpy as np

from tests import conduction_ref as cr
from tests.rowwise import EPS, _pow2   # noqa: F401  (EPS is re-exported)

LD = np.longdouble
LOC = np.array([cr.LX, cr.LY, cr.LZ]).T       # corner a -> (lx, ly, lz)
NU = 0.3

# ---- the cases: the five one-level meshes of conduction_ref.FINE_CASES, both designs (mixed, and 0/1 at Emin = 1e-9)
FINE_CASES = cr.FINE_CASES
SLAB_CASES = [((16, 8, 8), (0.125, 0.125, 0.1), 2), ((12, 8, 12), 0.25, 3)]     # elements, h, ranks
DESIGNS = {"mixed": 1e-9, "binary": 1e-9}                                     # design -> Emin (Emax = 1)
GRADIENT_CASE = ((16, 8, 8), 0.125, 3)       # elements, h, levels: the coupled gradient on the device
CPU_GRADIENT_CASE = ((6, 4, 4), 0.25)
DRIVER_CASE = ((8, 8, 4), 2, 3)              # elements, levels, design iterations


def par(kind="mixed", alpha=0.37, T_ref=0.25, pb=3.0):
    """the thermal parameters of a test: T_ref is not 0"""
    return dict(alpha=alpha, T_ref=T_ref, Emin=DESIGNS[kind], Emax=1.0, pb=pb)


# =====================================================================================================================
# constants.  Counts of the longest chain of a row; measured: the float64 forms against the longdouble ones on this CPU over
# FINE_CASES and SLAB_CASES x DESIGNS (tests/test_thermoelastic_oracle.py prints them)
# =====================================================================================================================
# G in closed form: pre = 0.5 / (1 - 2 nu) (3 roundings), the area, its division, the product: 6.  Measured against the 80-bit
# quadrature, relative to max|G|: 0.90 (x 16 = 14.4) -> 16.
C_G = 16
# KE x = G 1: the 24-term row of KE against the corner coordinates and the 8-term row of G: 32.  Measured, relative to
# sum_j |KE_ij| |x_j| + sum_b |G_ib|: 2.34 (x 16 = 37.5) -> 64 from the measured value.
C_FREE = 64
# beta = alpha (Emin + x^pb dE): pow (<= 2 ulp on the device), the product, the sum, the product with alpha: 5 -> 8.
# Measured (numpy float64 against longdouble): 3.63 (x 16 = 58) -> 64.
C_BETA = 64
# beta' = alpha pb x^(pb-1) dE: pow (2), three products: 5 -> 8.  Measured: 3.27 (x 16 = 52) -> 64.
C_DBETA = 64
# load row: theta's subtraction (1), the 8-term sum, beta (5), the product with it, 8 elements: 23 -> 32.  Measured: 5.22
# (x 16 = 83.5) -> 128 from the measured value.  On a base the row gains one addition and its scale |rhs_base|.
C_LOAD = 128
# adjoint row: the weighted sum of <= 3 fields (3), the 24-term sum, beta (5), its product, 8 elements, scale: 42 -> 64.
# Measured: 3.44 (x 16 = 55) -> 64 either way.
C_ADJ = 64
# sensitivity per element: theta (1), G theta (8), the 24-term dot product, the weighted sum over <= 3 fields (3), beta' (5), two
# scale products, the addition into dfdx: 45 -> 64 from the count.  Measured: 1.31 (x 16 = 21).
C_SENS = 64


# =====================================================================================================================
# the coupling matrix
# =====================================================================================================================
def G(h, nu=NU, dtype=np.float64):
    """G[(a,c), b] = 1 / (1 - 2 nu) int dN_a/dx_c N_b dV on a box, [24, 8]: along axis c the factor -+ 1/2 by corner a's side,
    along the two other axes M_d = h_d [[2, 1], [1, 2]] / 6 -- formed as the library does: pre = 0.5 / (1 - 2 nu), then
    pre * (h_d1 h_d2 / {9, 18, 36})"""
    hh = [dtype(v) for v in cr.h3(h)]
    pre = dtype(0.5) / (dtype(1) - dtype(2) * dtype(nu))
    out = np.zeros((24, 8), dtype=dtype)
    for c in range(3):
        area = hh[(c + 1) % 3] * hh[(c + 2) % 3]
        mag = [pre * (area / dtype(9)), pre * (area / dtype(18)), pre * (area / dtype(36))]
        for a in range(8):
            for b in range(8):
                m = int(LOC[a, (c + 1) % 3] != LOC[b, (c + 1) % 3]) + int(LOC[a, (c + 2) % 3] != LOC[b, (c + 2) % 3])
                out[3 * a + c, b] = mag[m] if LOC[a, c] else -mag[m]
    return out


def G_quadrature(h, nu=NU):
    """int B^T D0 phi N_b by 2 x 2 x 2 Gauss quadrature in longdouble: B the 6 x 24 strain-displacement matrix (rows xx, yy, zz,
    xy, yz, zx), D0 the unit-modulus isotropic matrix, phi = (1, 1, 1, 0, 0, 0).  The integrand is at most quadratic along each
    axis: the rule is exact"""
    hh = [LD(v) for v in cr.h3(h)]
    nu = LD(nu)
    lam, mu = nu / ((1 + nu) * (1 - 2 * nu)), 1 / (2 * (1 + nu))
    D0 = np.zeros((6, 6), dtype=LD)
    D0[:3, :3] = lam
    for i in range(3):
        D0[i, i] = lam + 2 * mu
        D0[i + 3, i + 3] = mu
    s = D0 @ np.array([1, 1, 1, 0, 0, 0], dtype=LD)
    sg = 2 * LOC.astype(LD) - 1
    gp = 1 / np.sqrt(LD(3))
    rows = ((0, 0), (1, 1), (2, 2))               # normal strain rows: component c, derivative axis c
    shear = ((3, 0, 1), (3, 1, 0), (4, 1, 2), (4, 2, 1), (5, 2, 0), (5, 0, 2))   # (row, component, derivative axis)
    out = np.zeros((24, 8), dtype=LD)
    for px in (-gp, gp):
        for py in (-gp, gp):
            for pz in (-gp, gp):
                xi = (px, py, pz)
                Nb = np.array([np.prod([(1 + sg[b, d] * xi[d]) / 2 for d in range(3)]) for b in range(8)], dtype=LD)
                dN = np.zeros((3, 8), dtype=LD)
                for d in range(3):
                    for a in range(8):
                        o = [(1 + sg[a, e] * xi[e]) / 2 for e in range(3) if e != d]
                        dN[d, a] = sg[a, d] / hh[d] * o[0] * o[1]
                B = np.zeros((6, 24), dtype=LD)
                for r, c in rows:
                    B[r, c::3] = dN[c]
                for r, c, d in shear:
                    B[r, c::3] += dN[d]
                wdet = hh[0] * hh[1] * hh[2] / 8
                out += wdet * np.outer(B.T @ s, Nb)
    return out


def corner_coordinates(h, dtype=np.float64):
    """the positions of the 8 corners, interleaved (x, y, z): a displacement field of unit strain in every direction"""
    hh = np.array([dtype(v) for v in cr.h3(h)], dtype=dtype)
    return (LOC.astype(dtype) * hh[None, :]).reshape(-1)


# =====================================================================================================================
# interpolation
# =====================================================================================================================
def beta(x, p, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return dtype(p["alpha"]) * (dtype(p["Emin"]) + x ** dtype(p["pb"]) * (dtype(p["Emax"]) - dtype(p["Emin"])))


def dbeta(x, p, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return dtype(p["alpha"]) * dtype(p["pb"]) * x ** dtype(p["pb"] - 1.0) * (dtype(p["Emax"]) - dtype(p["Emin"]))


# =====================================================================================================================
# the three passes, dense over the elements
# =====================================================================================================================
def elem_nodes(ex, ey, ez):
    nx, ny = ex + 1, ey + 1
    k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    return np.stack([(i + l[0]) + nx * ((j + l[1]) + ny * (k + l[2])) for l in LOC], axis=1)


def elem_dofs(ex, ey, ez):
    nd = elem_nodes(ex, ey, ez)
    return (3 * nd[:, :, None] + np.arange(3)[None, None, :]).reshape(nd.shape[0], 24)


def theta(T, p, dtype=np.float64):
    return np.asarray(T, dtype=dtype) - dtype(p["T_ref"])


def load(ne, h, x, T, p, nu=NU, dtype=np.float64, absolute=False):
    """f_th = sum_e beta_e G theta_e on all 3 n dofs (supports not applied); absolute: the row scale, |beta| |G| |theta|"""
    ex, ey, ez = ne
    nd, dofs = elem_nodes(ex, ey, ez), elem_dofs(ex, ey, ez)
    Gm, be, th = G(h, nu, dtype), beta(x, p, dtype), theta(T, p, dtype)
    if absolute:
        Gm, be, th = np.abs(Gm), np.abs(be), np.abs(th)
    fe = be[:, None] * (th[nd] @ Gm.T)
    out = np.zeros(3 * (ex + 1) * (ey + 1) * (ez + 1), dtype=dtype)
    np.add.at(out, dofs.reshape(-1), fe.reshape(-1))
    return out


def combine(V_list, w, dtype=np.float64, absolute=False):
    w = [1.0] * len(V_list) if w is None else w
    acc = np.zeros(np.asarray(V_list[0]).shape, dtype=dtype)
    for wl, v in zip(w, V_list):
        v = np.asarray(v, dtype=dtype)
        acc = acc + (abs(dtype(wl)) * np.abs(v) if absolute else dtype(wl) * v)
    return acc


def adjoint_rhs(ne, h, x, V_list, w, N, p, scale=1.0, nu=NU, dtype=np.float64, absolute=False):
    """g_n = scale sum_{e contains n} beta_e sum_{a,c} G[(a,c), b(e,n)] (N sum_l w_l v_l)_{a,c}; absolute: the row scale (N = 1)"""
    ex, ey, ez = ne
    nd, dofs = elem_nodes(ex, ey, ez), elem_dofs(ex, ey, ez)
    Gm, be = G(h, nu, dtype), beta(x, p, dtype)
    v = combine(V_list, w, dtype, absolute)
    if absolute:
        Gm, be, scale = np.abs(Gm), np.abs(be), abs(scale)
    else:
        v = np.asarray(N, dtype=dtype) * v
    ge = be[:, None] * (v[dofs] @ Gm)
    out = np.zeros((ex + 1) * (ey + 1) * (ez + 1), dtype=dtype)
    np.add.at(out, nd.reshape(-1), ge.reshape(-1))
    return dtype(scale) * out


def sensitivity(ne, h, x, V_list, w, N, T, p, scale=1.0, nu=NU, dtype=np.float64, absolute=False):
    """scale beta'_e sum_l w_l (N v_l)_e^T G theta_e per element; absolute: the row scale"""
    ex, ey, ez = ne
    nd, dofs = elem_nodes(ex, ey, ez), elem_dofs(ex, ey, ez)
    Gm, db, th = G(h, nu, dtype), dbeta(x, p, dtype), theta(T, p, dtype)
    v = combine(V_list, w, dtype, absolute)
    if absolute:
        Gm, db, th, scale = np.abs(Gm), np.abs(db), np.abs(th), abs(scale)
    else:
        v = np.asarray(N, dtype=dtype) * v
    return dtype(scale) * db * np.einsum("er,er->e", v[dofs], th[nd] @ Gm.T)


def fields(ne, seed):
    """-> T [n], v0, v1, v2 [3 n]: seeded, nowhere small in particular (supports and sink included): normal + 0.5"""
    n = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
    rng = np.random.default_rng(7100 + seed)
    return [rng.standard_normal(n) + 0.5] + [rng.standard_normal(3 * n) + 0.5 for _ in range(3)]


def cantilever(ne, h):
    """supports and line load of the project's cantilever (clamp x = xmin; -0.001 in z along x = xmax, z = zmin, half at the ends)"""
    nx, ny, nz = ne[0] + 1, ne[1] + 1, ne[2] + 1
    N = np.ones((nz, ny, nx, 3))
    N[:, :, 0, :] = 0.0
    R = np.zeros((nz, ny, nx, 3))
    R[0, :, nx - 1, 2] = -0.001
    R[0, 0, nx - 1, 2] = R[0, ny - 1, nx - 1, 2] = -0.0005
    return N.reshape(-1), R.reshape(-1)


# =====================================================================================================================
# the coupled problem by direct solves
# =====================================================================================================================
class Coupled:
    """K(x) u = N (F + f_th(x, T)),  A(x) T = N_T q  (mode "conduction") or T = T_ref + delta_T (mode "uniform"), c = u^T K u and
    dc/dx by the two adjoint terms, sparse direct solves throughout"""

    def __init__(self, ne, h, KE, p, mode="conduction", delta_T=None, kmin=1e-3, kmax=1.0, penal=3.0, q0=1.0, nu=NU):
        self.ne, self.h, self.p, self.mode, self.delta_T, self.nu = ne, h, p, mode, delta_T, nu
        self.KE = np.asarray(KE, dtype=np.float64).reshape(24, 24)
        self.kmin, self.kmax, self.penal = kmin, kmax, penal
        self.dims = (ne[0] + 1, ne[1] + 1, ne[2] + 1)
        self.N, self.F = cantilever(ne, h)
        self.NT = cr.sink_mask(*self.dims)
        self.q = cr.load(*self.dims, h, q0)
        self.KT = cr.KT(h).reshape(8, 8)
        self.nd, self.dofs = elem_nodes(*ne), elem_dofs(*ne)

    def E(self, x):
        return self.p["Emin"] + x ** self.penal * (self.p["Emax"] - self.p["Emin"])

    def temperature(self, x):
        import scipy.sparse.linalg as spl
        from tests import scipy_check as sc
        if self.mode == "uniform":
            return np.full(np.prod(self.dims), self.p["T_ref"] + self.delta_T), None
        A = sc.assemble(*self.ne, self.KT, E=cr.conductivity(x, self.kmin, self.kmax, self.penal), N=self.NT, dof=1).tocsc()
        lu = spl.splu(A)
        return lu.solve(self.NT * self.q), lu

    def state(self, x):
        """-> dict(c, u, T, f_th, rhs, lu_A)"""
        import scipy.sparse.linalg as spl
        from tests import scipy_check as sc
        T, luA = self.temperature(x)
        f_th = load(self.ne, self.h, x, T, self.p, self.nu)
        rhs = self.N * (self.F + f_th)
        K = sc.assemble(*self.ne, self.KE, E=self.E(x), N=self.N).tocsc()
        u = spl.splu(K).solve(rhs)
        return dict(c=float(np.dot(rhs.astype(LD), u.astype(LD))), u=u, T=T, f_th=f_th, rhs=rhs, lu_A=luA)

    def gradient(self, x, s=None):
        """-> dict(dc, elastic, thermal, adjoint, mu, g) on the state s (solved here if None)"""
        s = self.state(x) if s is None else s
        u, T = s["u"], s["T"]
        dE = self.p["Emax"] - self.p["Emin"]
        ue = u[self.dofs]
        elastic = -self.penal * x ** (self.penal - 1) * dE * np.einsum("er,rs,es->e", ue, self.KE, ue)
        thermal = sensitivity(self.ne, self.h, x, [u], None, self.N, T, self.p, 2.0, self.nu)
        out = dict(elastic=elastic, thermal=thermal, adjoint=np.zeros_like(x), mu=None, g=None)
        if self.mode == "conduction":
            g = adjoint_rhs(self.ne, self.h, x, [u], None, self.N, self.p, 1.0, self.nu)
            mu = s["lu_A"].solve(self.NT * g)
            out["adjoint"] = cr.response(self.dims, self.h, [T], [mu], [2.0], x, self.kmin, self.kmax, self.penal)["dfdx"]
            out["mu"], out["g"] = mu, g
        out["dc"] = elastic + thermal + out["adjoint"]
        return out
