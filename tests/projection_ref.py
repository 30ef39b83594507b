"""Reference pieces of the projection tests in plain numpy (a helper module: no fixtures, no collection hooks): the smooth Heaviside
projection, its derivative, the measure of non-discreteness and PETSc's pointwise quotient in float64 or numpy.longdouble, the
cases (beta, eta, salted fields), and the row scales and constants of the row-wise bounds.

Row-wise bounds follow tests/rowwise.py:  |got_i - ref_i| <= c 2^-53 scale_i,  ref the 80-bit value.  The scales follow the
expressions as the reference writes them (Filter.h:80-88), so what cancels in them is the scale's business, not a failure:

    forward   y_i  = (t0 + th_i) / den,                t0 = tanh(beta eta), th_i = tanh(beta (x_i - eta)),
                                                       den = t0 + tanh(beta (1 - eta))
              scale_i = (|t0| + |th_i|) / den          (t0 + th_i cancels at x -> 0)
    chain     df_i beta (1 - th_i^2) / den
              scale_i = |df_i| beta (1 + th_i^2) / den (1 - th_i^2 cancels where the projection saturates)

c is the larger of the operation count of the row's chain and 16 x what the float64 restatement below measures against the 80-bit
one on the CPU over every case of CASES (tests/test_projection_oracle.py prints the figures and holds the restatement and the
oracle to a QUARTER of each constant), rounded up to a power of two.
"""
import numpy as np

from tests.rowwise import EPS, _pow2   # noqa: F401  (EPS is re-exported)

BETAS = (0.1, 1.0, 4.0, 16.0, 48.0, 64.0)
ETAS = (0.0, 0.3, 0.5, 0.7, 1.0)
CASES = [(b, e) for b in BETAS for e in ETAS]
# the projection alone and the chain alone: elements of the field; (ex, ey, ez) of a mesh with that many.  531 441 = 81^3 is the
# first size at which grid_for's 2048 workgroups of 256 stride (> 524 288)
SIZES = {1: (1, 1, 1), 63: (63, 1, 1), 64: (4, 4, 4), 65: (5, 13, 1), 257: (257, 1, 1), 1001: (7, 11, 13), 531441: (81, 81, 81)}
STRIDE = 2048 * 256
# GetMND: 2 113 536 = 129 x 128 x 128 is past MAX_RED_BLOCKS x 256 = 2 097 152, where k_mnd's launch is capped and strides
MND_SIZES = {1: (1, 1, 1), 255: (15, 17, 1), 257: (257, 1, 1), 2113536: (129, 128, 128)}
MAX_RED_BLOCKS, BLK = 8192, 256
# VecPointwiseDivide through the shim: element meshes (the Vec lives on the element DMDA of a node mesh one larger each way)
DIVIDE_SIZES = {1: (1, 1, 1), 255: (15, 17, 1), 256: (16, 16, 1), 257: (257, 1, 1), 524289: (3, 174763, 1)}
# where a tanh changes method or saturates: |beta (x - eta)| on both sides of these (2^-28: tanh(x) = x below it; 0.5 and 1: the
# expm1 forms' switch in the usual implementations; 19 and 22: tanh rounds to 1 in float64 from there on)
TANH_EDGES = (2.0 ** -28, 0.5, 1.0, 19.0, 22.0)
TINY = float(np.finfo(np.float64).tiny)     # the smallest normal number
MONOTONE_SLACK = 8 * EPS                    # as tests/test_gpu_robust.py


# =====================================================================================================================
# the operations
# =====================================================================================================================
def parts(x, beta, eta, dtype=np.float64):
    """-> (t0, th, den) as the kernels form them: every operation rounded in `dtype`"""
    x, beta, eta = np.asarray(x, dtype=dtype), dtype(beta), dtype(eta)
    t0 = np.tanh(beta * eta)
    return t0, np.tanh(beta * (x - eta)), t0 + np.tanh(beta * (dtype(1) - eta))


def H(x, beta, eta, dtype=np.float64):
    """(tanh(beta eta) + tanh(beta (x - eta))) / (tanh(beta eta) + tanh(beta (1 - eta)))"""
    t0, th, den = parts(x, beta, eta, dtype)
    return (t0 + th) / den


def dH(x, beta, eta, dtype=np.float64):
    """beta (1 - tanh^2(beta (x - eta))) / den"""
    _, th, den = parts(x, beta, eta, dtype)
    return dtype(beta) * (dtype(1) - th * th) / den


def chain(df, x, beta, eta, dtype=np.float64):
    """df_i H'(x_i), the product the kernels store"""
    return np.asarray(df, dtype=dtype) * dH(x, beta, eta, dtype)


def mnd_terms(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    return dtype(4) * x * (dtype(1) - x)


def mnd(x, dtype=np.float64):
    """sum_i 4 x_i (1 - x_i) / n  (Filter.cc:206-225)"""
    t = mnd_terms(x, dtype)
    return t.sum() / dtype(t.size)


def petsc_div(a, b, dtype=np.float64):
    """PETSc's VecPointwiseDivide: a / b, and 0 where b is 0"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    zero = b == 0
    return np.where(zero, dtype(0), a / np.where(zero, dtype(1), b))


# =====================================================================================================================
# row scales (float64: their own rounding, 1e-16 of themselves, does not matter)
# =====================================================================================================================
def scale_forward(x, beta, eta):
    t0, th, den = parts(x, beta, eta)
    return (abs(t0) + np.abs(th)) / den


def scale_chain(df, x, beta, eta):
    _, th, den = parts(x, beta, eta)
    return np.abs(np.asarray(df, dtype=np.float64)) * beta * (1.0 + th * th) / den


# =====================================================================================================================
# constants, in units of eps = 2^-53 x scale.  A tanh within 2 ulp counts 4.  Measured: the float64 restatement above against the
# longdouble one, largest over CASES x the fields of every size in SIZES but the largest (tests/test_projection_oracle.py)
# =====================================================================================================================
# forward: th = tanh(beta (x - eta)): the subtraction and the product move the argument by 2 eps of itself, and |a tanh'(a)| <=
# |tanh(a)|: 2, the tanh 4 -> 6 |th|; t0: the product 1, the tanh 4 -> 5 |t0|; the sum 1; den = t0 + t1 the same way: 5 + 1 = 6 of
# itself; the division 1: 6 + 1 + 6 + 1 = 14.  Measured: 4.00 (x 16 = 64) -> 64 from the measured value: the row x = the smallest
# normal number at beta = 0.1, eta = 0, where beta x is subnormal and keeps 49 bits (<= 8 eps of itself; not in the count).  Every
# other row: 2.90.
C_FORWARD = 64
# chain: th 6 as above, th^2: 2 x 6 + 1 = 13 th^2, 1 - th^2: + 1, all of it below 13 (1 + th^2); x beta 1, / den 6 + 1, x df 1:
# 13 + 1 + 1 + 7 + 1 = 23.  Measured: 3.32 (x 16 = 53) -> 64 from the measured value.
C_CHAIN = 64


def mnd_chain(n):
    """longest chain of rounded operations a term of GetMND's sum passes through: 1 - x and the product (2; 4 x is exact), the
    thread's grid-stride additions ceil(n / (workgroups x 256)), the workgroup's sum (wave_sum's 6 shuffle stages, then the 4 waves'
    sums added in turn: 10), k_reduce_final over the partials (a thread adds every 256th: ceil(workgroups / 256); the workgroup's
    sum again: 10) and the division by n (1)"""
    nb = min(max((n + BLK - 1) // BLK, 1), MAX_RED_BLOCKS)
    return 2 + (n + nb * BLK - 1) // (nb * BLK) + 10 + (nb + 255) // 256 + 10 + 1


def c_mnd(n):
    """|got - sum / n| <= c eps sum |terms| / n, the sum formed in 80-bit arithmetic: c = the chain's length rounded up to a power of
    two, as rw.c_dot derives its constant.  Such a bound holds for any float64 summation of that depth: no oracle figure.
    n = 1, 255, 257: 25 -> 32; 2 113 536: 2 + 2 + 10 + 32 + 10 + 1 = 57 -> 64."""
    return _pow2(mnd_chain(n))


# =====================================================================================================================
# the fields
# =====================================================================================================================
def salts(beta, eta):
    """the values a projection kernel can go wrong at, all in [0, 1]: exact 0.0, -0.0, 1.0 and eta itself, eta +- 2^-k for k = 1,
    10, 30, 52, the smallest normal number, and x with |beta (x - eta)| a factor 1 -+ 2^-10 either side of every TANH_EDGES, above
    and below eta (those that fall outside [0, 1] are left out)"""
    s = [0.0, -0.0, 1.0, eta]
    s += [eta + sg * 2.0 ** -k for k in (1, 10, 30, 52) for sg in (1.0, -1.0)]
    s.append(TINY)
    s += [eta + sg * t * f / beta for t in TANH_EDGES for f in (1.0 - 2.0 ** -10, 1.0 + 2.0 ** -10) for sg in (1.0, -1.0)]
    return [v for v in s if 0.0 <= v <= 1.0]


def field(n, beta, eta, seed=0):
    """n values in [0, 1]: seeded uniform ones with salts(beta, eta) spread evenly over the field; 0.0 at index 0 and 1.0 at n - 1;
    from 257 elements on -0.0 and eta at 63 and 64 (both sides of a wave's border); every salt again from index 524 288 on, where
    the grid-stride loop takes its second trip.  A field shorter than the list of salts holds the list from `seed` on."""
    s = salts(beta, eta)
    if n < len(s) + 2:
        return np.array([s[(seed + i) % len(s)] for i in range(n)], dtype=np.float64)
    a = np.random.default_rng(1000 * n + seed).uniform(0.0, 1.0, n)
    for j, v in enumerate(s):
        i = 1 + (j * (n - 2)) // len(s)
        a[i + 2 if n >= 257 and i in (63, 64) else i] = v
    a[0], a[n - 1] = 0.0, 1.0
    if n >= 257:
        a[63], a[64] = -0.0, eta
    if n > STRIDE + len(s):
        a[STRIDE:STRIDE + len(s)] = s
    return a


def rows(n, seed=0):
    """a gradient row of mixed signs with exact zeros of both signs"""
    df = np.random.default_rng(77 * n + seed).standard_normal(n)
    df[5::7] = 0.0
    df[3::11] = -0.0
    return df


def mnd_fields(n):
    """{name: (field, exact value or None)}: 0/1 gives exactly 0, all 0.5 exactly 1 (every term is exactly 0 or 1 and n < 2^53)"""
    r = np.random.default_rng(5 * n + 1)
    return {"zero_one": ((r.random(n) < 0.5).astype(np.float64), 0.0), "half": (np.full(n, 0.5), 1.0), "random": (r.random(n), None)}
