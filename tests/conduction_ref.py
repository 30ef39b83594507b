"""Reference pieces of the heat-conduction tests in plain numpy (a helper module: no fixtures, no collection hooks): the element
matrix KT in closed form, the built-in sink and load, the designs, the row scales and constants of the row-wise bounds, and the
thermal compliance with its gradient in float64 or numpy.longdouble.

Row-wise bounds follow tests/rowwise.py:  |got_i - arbiter_i| <= c 2^-53 scale_i,  scale_i the same operator applied to |u| with |KT|
and all-ones masks (on level l: R S_{l-1}(P |u|)), c the larger of the operation count of the row's chain and 16 x what the
float64 oracle measures against the 80-bit arbiter on the CPU, rounded up to a power of two.  tests/test_conduction_oracle.py
holds the oracle to a QUARTER of every constant on every mesh and design below; the measured values stand beside the counts.
"""
import numpy as np

from tests.rowwise import EPS, _pow2   # noqa: F401  (EPS is re-exported)

LX, LY, LZ = (0, 1, 1, 0, 0, 1, 1, 0), (0, 0, 1, 1, 0, 0, 1, 1), (0, 0, 0, 0, 1, 1, 1, 1)    # the reference's corner order

# ---- the cases of tests/test_gpu_conduction.py and tests/test_gpu_conduction_slabs.py: elements, h, levels
FINE_CASES = [
    ((3, 3, 3), 0.25, 1),
    ((5, 2, 7), (0.05, 0.04, 0.03), 1),
    ((7, 1, 5), 0.25, 1),                      # every node lies on a y boundary
    ((20, 12, 8), (0.05, 0.04, 0.03), 1),
    ((33, 31, 63), 1.0 / 31, 1),               # 69 632 nodes: several workgroups and a tail
]
LEVEL_CASES = [
    ((16, 8, 8), (0.125, 0.125, 0.1), 3),
    ((8, 4, 12), 0.25, 3),
    ((32, 16, 16), 1.0 / 16, 4),
]
SOLVE_CASES = [0, 2]                           # indices into LEVEL_CASES
SLAB_CASES = [((16, 8, 8), (0.125, 0.125, 0.1), 3, 2), ((12, 8, 12), 0.25, 3, 3)]   # ..., ranks
# design name -> kmin (kmax = 1, penal = 3): a mixed field, and a 0/1 field whose void rows are 1e-9 of the solid ones
DESIGNS = {"mixed": 1e-3, "binary": 1e-9}
KMAX, PENAL = 1.0, 3.0
SOLVE = dict(nsmooth=2, ncoarse=30, rtol=1e-10)
DRIVER_CASE = ((8, 8, 4), 2, 3)                # elements, levels, design iterations


def h3(h):
    return (h, h, h) if np.isscalar(h) else tuple(h)


def KT(h, dtype=np.float64):
    """int grad N_a . grad N_b over a box element at unit conductivity: Sx (x) My (x) Mz + Mx (x) Sy (x) Mz + Mx (x) My (x) Sz with
    S = [[1, -1], [-1, 1]] / h, M = h [[2, 1], [1, 2]] / 6 per axis -> 64 values, row major, reference corner order"""
    hx, hy, hz = (dtype(v) for v in h3(h))
    S = [np.array([[1, -1], [-1, 1]], dtype=dtype) / v for v in (hx, hy, hz)]
    M = [np.array([[2, 1], [1, 2]], dtype=dtype) * v / dtype(6) for v in (hx, hy, hz)]
    out = np.zeros((8, 8), dtype=dtype)
    for a in range(8):
        for b in range(8):
            ia, ib = (LX[a], LY[a], LZ[a]), (LX[b], LY[b], LZ[b])
            f = lambda A, d: A[d][ia[d], ib[d]]
            out[a, b] = f(S, 0) * f(M, 1) * f(M, 2) + f(M, 0) * f(S, 1) * f(M, 2) + f(M, 0) * f(M, 1) * f(S, 2)
    return out.reshape(-1)


def sink_mask(nx, ny, nz):
    """N of the built-in problem (nodes): 0 on the face i = 0 where |2j - (ny-1)| <= max(1, (ny-1)//4) and
    |2k - (nz-1)| <= max(1, (nz-1)//4), 1 elsewhere"""
    j, k = np.arange(ny), np.arange(nz)
    sj = np.abs(2 * j - (ny - 1)) <= max(1, (ny - 1) // 4)
    sk = np.abs(2 * k - (nz - 1)) <= max(1, (nz - 1) // 4)
    N = np.ones((nz, ny, nx))
    N[:, :, 0] = 1.0 - (sk[:, None] & sj[None, :])
    return N.reshape(-1)


def load(nx, ny, nz, h, q0=1.0):
    """uniform volumetric source: rhs_n = q0 hx hy hz / 8 x (number of elements around node n)"""
    hx, hy, hz = h3(h)
    around = lambda n: np.where((np.arange(n) == 0) | (np.arange(n) == n - 1), 1.0, 2.0)
    cnt = around(nz)[:, None, None] * around(ny)[None, :, None] * around(nx)[None, None, :]
    return (q0 * hx * hy * hz / 8.0 * cnt).reshape(-1)


def design(kind, ex, ey, ez, seed=0):
    """xPhys per element: "mixed" in [0.05, 1], "binary" 0/1 at equal odds"""
    r = np.random.default_rng(4242 + 17 * seed + ex + 100 * ey + 10000 * ez).random(ex * ey * ez)
    return 0.05 + 0.95 * r if kind == "mixed" else (r < 0.5).astype(np.float64)


def conductivity(x, kmin, kmax=KMAX, penal=PENAL, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return dtype(kmin) + x ** dtype(penal) * (dtype(kmax) - dtype(kmin))


def inputs(n, seed, count=2):
    """seeded vectors that do not vanish anywhere in particular (the sink included): normal + 0.5"""
    rng = np.random.default_rng(9000 + seed)
    return [rng.standard_normal(n) + 0.5 for _ in range(count)]


# =====================================================================================================================
# constants.  Counts as the issue states them; measured: oracle against arbiter on this CPU over FINE_CASES, LEVEL_CASES and
# SLAB_CASES x DESIGNS (tests/test_conduction_oracle.py prints them)
# =====================================================================================================================
# fine product: per element 8 fma and the conductivity's product, 8 elements: <= 44 in either summation order.
# Measured: 3.74 for the gather (orc.matfree_apply; x 16 = 60), 6.00 for the assembled CSR row -> 64 from the count.
C_FINE = 64


def c_level(l):
    """Galerkin level l >= 1: the 27-term row, 8 coarse elements, and per Galerkin step two 8-term contractions and 8 children:
    35 + 24 l = 59, 83, 107 -> 64, 128, 128.  Measured: 1.97 / 2.32 / 0.91 on levels 1 / 2 / 3 (x 16 <= 38)."""
    return _pow2(35 + 24 * l)


def c_op(l):
    return C_FINE if l == 0 else c_level(l)


def c_diag(l):
    """the Jacobi diagonal (exported as its reciprocal), RELATIVE to the row's own entry.  Count: level 0 the 8-element sum of
    positive terms, the reciprocal and the test's own division back: 10; level l the coefficient's formation, 8 + 24 l, + 2: 34,
    58, 82.  Measured: 5.22 / 6.85 / 6.53 / 6.05 on levels 0 .. 3 (x 16 = 84, 110, 105, 97): the measured values set all four."""
    return 128


def c_resid(l):
    """r = b - A_l x: the product's count + 1: 45, 60, 84, 108 -> 64, 64, 128, 128.  Measured: 3.72 / 1.62 / 1.98 / 0.81 on
    levels 0 .. 3 (x 16 <= 60)."""
    return _pow2((44 if l == 0 else 35 + 24 * l) + 1)


def c_smooth(l):
    """one Chebyshev step x1 = x0 + (1 / theta) dinv (b - A x0) from the device's dinv and window: the product's count + 5: 49,
    64, 88, 112 -> 64, 64, 128, 128.  Measured: 3.13 / 2.20 / 1.60 / 1.35 on levels 0 .. 3 (x 16 <= 51)."""
    return _pow2((44 if l == 0 else 35 + 24 * l) + 5)


def c_smooth_k(l):
    """step k >= 2 of a sweep from the device's own x_{k-1}, x_{k-2}: c_smooth's count + 4: 53, 68, 92, 116.  Measured: 4.55 /
    1.45 / 0.84 / 0.28 on levels 0 .. 3 (x 16 = 73, 24, 14, 5): level 0 takes 128 from the measured value, the others 128 from the
    count."""
    return 128


# the transfers are rowwise.py's with one component: C_RESTRICT, C_PROLONG (64 both).  Measured here: 4.20 and 2.17.
# dfdx per element: v_e^T KT t_e as 8 dot products of 8 terms and an 8-term sum (16), the weighted sum over <= 3 cases (6),
# pow(x, p - 1) (<= 2), three scale factors (3): 27.  Measured (float64 numpy restatement against longdouble): 7.89 (x 16 = 127) -> 128.
C_DFDX = 128


# =====================================================================================================================
# row scales (orc: the float64 oracle module)
# =====================================================================================================================
def scale_fine(orc, dims, kt, k, u, N=None):
    """sum over the elements of a row of k_e sum_b |KT[a][b]| |u_b| (N -> ones: a clamped neighbour only lowers the true sum).
    With N: a Dirichlet row carries |u| instead, the identity the operator has there"""
    nx, ny, nz = dims
    au = np.abs(np.asarray(u, dtype=np.float64))
    s = orc.matfree_apply(nx, ny, nz, 1, np.abs(np.asarray(kt, dtype=np.float64)), orc.f64(k), np.ones(nx * ny * nz), au)
    return s if N is None else np.where(np.asarray(N) != 0, s, au)


def scale_level(orc, mg, l, dims, kt, k, N, u):
    """S_l(|u|) = R_{l-1} ... R_0 S_0(P_0 ... P_{l-1} |u|); mg: an assembled orc.MG of the same mesh (its transfers are used)"""
    v = np.abs(np.asarray(u, dtype=np.float64))
    for m in range(l - 1, -1, -1):
        v = mg.prolong(m, v)
    s = scale_fine(orc, dims, kt, k, v, N)
    for m in range(l):
        s = mg.restrict(m, s)
    return s


# =====================================================================================================================
# thermal compliance and its gradient
# =====================================================================================================================
def elem_gather(nx, ny, nz, T, dtype=np.float64):
    """[elements, 8]: the nodal values on every element's corners, reference corner order"""
    t = np.asarray(T, dtype=dtype).reshape(nz, ny, nx)
    return np.stack([t[LZ[a]:nz - 1 + LZ[a], LY[a]:ny - 1 + LY[a], LX[a]:nx - 1 + LX[a]].reshape(-1) for a in range(8)], axis=1)


def response(dims, h, T_list, V_list, w, x, kmin, kmax=KMAX, penal=PENAL, volfrac=0.3, dtype=np.float64):
    """-> dict(f_case, f_major, fx, gx, dfdx, dgdx, major): f_l = sum_e k_e v_e^T KT t_e (f_major: sum_e k_e |v_e|^T |KT| |t_e|), fx = sum_l w_l f_l, gx = mean(x) - volfrac,
    dfdx_e = -p x^(p-1) (kmax - kmin) sum_l w_l v_e^T KT t_e, and the majorant p x^(p-1) (kmax - kmin) sum_l |w_l| |v_e|^T |KT| |t_e|"""
    nx, ny, nz = dims
    K = KT(h, dtype).reshape(8, 8)
    x = np.asarray(x, dtype=dtype)
    k = conductivity(x, kmin, kmax, penal, dtype)
    w = [dtype(1)] * len(T_list) if w is None else [dtype(v) for v in w]
    f_case, f_major, acc, maj = [], [], np.zeros(x.size, dtype=dtype), np.zeros(x.size, dtype=dtype)
    for l, T in enumerate(T_list):
        V = T if V_list is None or V_list[l] is None else V_list[l]
        te, ve = elem_gather(nx, ny, nz, T, dtype), elem_gather(nx, ny, nz, V, dtype)
        vKt = np.einsum("ea,ab,eb->e", ve, K, te)
        aKa = np.einsum("ea,ab,eb->e", np.abs(ve), np.abs(K), np.abs(te))
        f_case.append((k * vKt).sum())
        f_major.append(float((k * aKa).sum()))
        acc += w[l] * vKt
        maj += abs(w[l]) * aKa
    pre = dtype(penal) * x ** dtype(penal - 1) * (dtype(kmax) - dtype(kmin))
    return dict(f_case=f_case, f_major=f_major, fx=sum(wl * f for wl, f in zip(w, f_case)), gx=x.sum() / dtype(x.size) - dtype(volfrac),
                dfdx=-pre * acc, dgdx=np.full(x.size, 1.0 / x.size), major=(pre * maj).astype(np.float64))
