"""Row-wise bounds for the reference solver configuration (ksp_mode 1, csrc/refksp.h): the Gauss-Seidel sweeps of PCSOR, PCJACOBI
and the level GMRES, on 0/1 designs (a plain helper module in the manner of tests/rowwise.py: no fixtures, no collection hooks).

WHY.  On a 0/1 design (Emin = 1e-9) one symmetric sweep of a unit normal vector returns ~5e10 on void rows and ~1e2 on solid
rows; rel(a, b) = max|a - b| / max|b| therefore holds the solid rows to five digits at best, and a relative error of 1e-7 on every
row with a large diagonal moves it by 1e-14 or less (tests/test_refksp_rowwise_oracle.py plants it).

THE SWEEP is held by its COMPONENTWISE BACKWARD ERROR, which needs no ordering argument: a forward Gauss-Seidel sweep from x0 to
x1 in natural row order satisfies, row by row and exactly,

    b_i - sum_{j <= i} a_ij x1_j - sum_{j > i} a_ij x0_j = 0          (backward sweep: j >= i takes x1, j < i takes x0)

so the residual of that mixed product, formed in 80-bit arithmetic on the 80-bit arbiter's matrix (oracle/arbiter.py), is held to

    |res_i| <= c eps (|b_i| + S_l(max(|x0|, |x1|))_i),        eps = 2^-53,

S_l the row-scale majorant of tests/rowwise.py (scale_fine / scale_level: on the levels >= 1 it carries the rounding of the stored
Galerkin coefficients as it does for c_level).  Level 0's sweep reads the moduli and the element matrix KE itself (RefKsp::pc_apply
builds MatfreeOp from L.KE, not from the packed form the products use), so the arbiter's matrix is assembled from KE.  A Dirichlet
row of level 0 is the identity: scale 0, x1_i = b_i bit for bit.

THE CONSTANTS: the count of rounded operations of a row, and 16 x what the float64 oracle's own sweep (oracle_sweep below: the
triangular solves of oracle/refksp.py's ssor_apply) achieves on the CPU; the larger, rounded up to a power of two (the rule of tests/rowwise.py).

    level 0   count: the row's product as C_FINE counts it (50; the gather form the sweep runs is shorter: 24-term chains, the
              modulus scale, the 8-element sum) + the in-node correction (<= 2 fma) + the subtraction, the division, the sum with
              the old value (3) + the node's diagonal block formed on the fly (8-element sum and modulus scale, the division by
              it: 11) = 66 -> 128.
              measured (oracle, every mesh, design and boundary condition of CASES): 4.47 (x 16 = 72 -> 128)
    level l   count: c_level(l)'s 89 + 56 l + the in-node correction (2) + subtraction, division, sum (3) = 94 + 56 l
              -> 256, 256, 512 for l = 1, 2, 3 (the diagonal block is read from the stored stencil: inside c_level's count).
              measured: 2.12 on level 1, 3.41 on level 2 (x 16 = 34, 55)
    (the MI355X's achieved figures: the table in tests/test_gpu_refksp_rowwise.py and DESIGN.md section 4.6 -- 1.01, 11.9, 9.28)
    PCJACOBI  z = dinv r, one rounded product: c = 1 against the 80-bit product of the device's own dinv (whose scale carries the
              80-bit product's own rounding, 2^-64: a factor 1 + 2^-11).  The dinv itself is held by tests/test_gpu_rowwise.py.

THE LEVEL GMRES (left-preconditioned, classical Gram-Schmidt, 4 iterations) couples all rows through its coefficients, so no row
scale is claimed for it: the distance from a long-double restatement (gmres_ld below: the 80-bit CSR, a SEQUENTIAL long-double
symmetric sweep in natural row order as preconditioner -- no wavefronts: the reference must not share the kernel's ordering
argument -- Givens rotations and back substitution by hand) is measured separately over the solid rows and over the void rows
(LevelCsr.classes: by the diagonal, d > 1e-3 max d), each as max|x - x_ld| over the class relative to max|x_ld| over the class, and
bounded by 16 x the float64 oracle's own distance (oracle/refksp.py gmres_left): GMRES_MEASURED below.
"""
import numpy as np

from tests import rowwise as rw

EPS = rw.EPS
LD = np.longdouble

# (elements, levels, (hx, hy, hz) or None = cube of h = 1 / ey): the edges of k_gs_wave's thread grid (ny x planes threads in
# workgroups of 256) and of its wavefront count
CASES = [
    ((16, 8, 4), 3, None),                  # coarsest level 5 x 3 x 2 nodes
    ((2, 2, 40), 2, None),                  # nx at its minimum, long in z
    ((12, 20, 8), 3, None),                 # ny > nx
    ((30, 14, 10), 2, None),                # odd node counts on the coarse level
    ((16, 16, 16), 3, None),                # 17 x 17 = 289 threads: a second, partial workgroup
    ((10, 6, 4), 2, (0.05, 0.04, 0.03)),    # dx != dy != dz
]
KINDS = rw.GENERATORS + ("synth",)
GMRES_CASES = (1, 0, 2)                     # indices into CASES: the three smallest meshes
DIAG_SPLIT = 1e-3                           # solid rows: diagonal above this fraction of the largest


def c_gs(l):
    """one Gauss-Seidel sweep on level l (counts and measured figures: the module docstring)"""
    return rw.pow2(66) if l == 0 else rw.pow2(94 + 56 * l)


C_JACOBI = 1
JACOBI_REF_SLACK = 1.0 + 2.0 ** -11         # the 80-bit product's own rounding (2^-64) in units of eps = 2^-53

# the distance of the float64 oracle's gmres_left from gmres_ld, 4 iterations from zero and 4 more from the iterate, largest over
# GMRES_CASES x rw.GENERATORS x both starts, measured on the CPU by tests/test_refksp_rowwise_oracle.py (which prints them and fails
# if the oracle moves beyond 4 x these); the device's bound is GMRES_MARGIN x them: (pc, level) -> (solid rows, void rows)
GMRES_MEASURED = {
    (1, 0): (1.41e-14, 7.05e-15), (1, 1): (3.29e-14, 1.15e-14), (1, 2): (3.47e-14, 1.08e-14),
    (0, 0): (2.72e-15, 1.12e-15), (0, 1): (6.45e-15, 2.18e-15), (0, 2): (1.80e-14, 3.60e-15),
}
GMRES_MARGIN = 16


def gmres_bound(pc, l, cls):
    return GMRES_MARGIN * GMRES_MEASURED[(pc, l)][0 if cls == "solid" else 1]


def ld(a):
    return np.ascontiguousarray(a, dtype=LD)


def box(case):
    (ex, ey, ez), _, h = case
    return h if h is not None else (1.0 / ey,) * 3


def design(orc, kind, mesh):
    return rw.cd_design(orc, kind, mesh)


def scattered_N(nx, ny, nz, rng):
    """the Dirichlet vector rowwise_worker.bc draws (single components of scattered nodes, and the first line of nodes)"""
    N = np.ones(3 * nx * ny * nz)
    N[rng.random(N.size) < 2e-2] = 0.0
    N[: 3 * nx].reshape(-1, 3)[:, :] = 0.0
    return N


def case_seed(m, scattered, kind):
    return 9000 + 100 * m + 10 * scattered + KINDS.index(kind)


class LevelCsr:
    """a level's matrix from the arbiter as 80-bit CSR arrays (orc_mg_level_csr, as rowwise.CdNorm reads it)"""

    def __init__(self, amg, l):
        n, nnz = amg.size(l), amg.L.orc_mg_level_nnz(amg.h, l)
        self.n = n
        self.rp, self.ci, self.v = np.zeros(n + 1, dtype=np.int64), np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=LD)
        amg.L.orc_mg_level_csr(amg.h, l, self.rp.ctypes.data, self.ci.ctypes.data, self.v.ctypes.data)
        assert (np.diff(self.rp) > 0).all()
        self.row = np.repeat(np.arange(n), np.diff(self.rp))
        on = self.ci == self.row
        assert on.sum() == n
        self.diag = self.v[on]

    def apply(self, u):
        return np.add.reduceat(self.v * ld(u)[self.ci], self.rp[:-1])

    def sweep_residual(self, b, x0, x1, backward):
        """b_i - sum_{j <= i} a_ij x1_j - sum_{j > i} a_ij x0_j (backward: mirrored), in 80-bit arithmetic"""
        x0, x1 = ld(x0), ld(x1)
        new = (self.ci >= self.row) if backward else (self.ci <= self.row)
        return ld(b) - np.add.reduceat(self.v * np.where(new, x1[self.ci], x0[self.ci]), self.rp[:-1])

    def sweep(self, b, x, backward=False):
        """one sequential Gauss-Seidel sweep in 80-bit arithmetic, rows in natural order (descending for a backward sweep)"""
        x, b = ld(x).copy(), ld(b)
        rp, ci, v, dg = self.rp.tolist(), self.ci, self.v, self.diag
        for i in (range(self.n - 1, -1, -1) if backward else range(self.n)):
            lo, hi = rp[i], rp[i + 1]
            x[i] += (b[i] - np.dot(v[lo:hi], x[ci[lo:hi]])) / dg[i]
        return x

    def ssor(self, r):
        """PCSOR: forward then backward from a zero guess"""
        return self.sweep(r, self.sweep(r, np.zeros(self.n, dtype=LD)), backward=True)

    def classes(self):
        """{"solid": rows whose diagonal exceeds DIAG_SPLIT of the largest, "void": the others}"""
        d = self.diag.astype(np.float64)
        solid = d > DIAG_SPLIT * d.max()
        return {"solid": solid, "void": ~solid}


def oracle_sweep(A, b, x0, backward=False, parts=None):
    """the float64 oracle's sweep from x0, by the triangular solves oracle/refksp.py's ssor_apply is made of: forward
    (D + L) x1 = b - U x0, backward (D + U) x1 = b - L x0 (ssor_apply(A, r) is the backward sweep of the forward sweep of zero)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from oracle import refksp
    DL, DU, L = refksp.ssor_parts(A) if parts is None else parts
    if backward:
        return spla.spsolve_triangular(DU, b - L @ x0, lower=False)
    return spla.spsolve_triangular(DL, b - sp.triu(DU, 1, format="csr") @ x0, lower=True)


def sweep_scale(orc, mg, l, dims, KE, E, N, b, x0, x1):
    """|b| + S_l(max(|x0|, |x1|)); a Dirichlet row of level 0: 0 (it must return b bit for bit)"""
    v = np.maximum(np.abs(np.asarray(x0, dtype=np.float64)), np.abs(np.asarray(x1, dtype=np.float64)))
    ab = np.abs(np.asarray(b, dtype=np.float64))
    if l == 0:
        return (ab + rw.scale_fine(orc, *dims, KE, E, v, N)) * (np.asarray(N) != 0)
    return ab + rw.scale_level(orc, mg, l, dims, KE, E, N, v)


def gmres_ld(M, pc, b, x0, m, maxit):
    """oracle/refksp.py's gmres_left (no convergence test: PCMG's smoothers run their iterations) restated in 80-bit arithmetic on a
    LevelCsr M; pc(r) the preconditioner; x0 None: zero guess.  -> (x, its)"""
    b = ld(b)
    x = np.zeros(M.n, dtype=LD) if x0 is None else ld(x0).copy()
    its, done = 0, maxit < 1
    while not done:
        r = pc(b if (x0 is None and its == 0) else b - M.apply(x))
        beta = np.sqrt(np.dot(r, r))
        if beta == 0 or its >= maxit:
            break
        V = np.zeros((m + 1, M.n), dtype=LD)
        V[0] = r / beta
        R = np.zeros((m + 1, m), dtype=LD)
        cs, sn, g = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD), np.zeros(m + 1, dtype=LD)
        g[0] = beta
        j = 0
        while j < m and its < maxit:
            w = pc(M.apply(V[j]))
            h = np.zeros(m + 2, dtype=LD)
            for q in range(j + 1):          # classical Gram-Schmidt: every dot product with the unmodified w
                h[q] = np.dot(V[q], w)
            for q in range(j + 1):
                w = w - h[q] * V[q]
            hn = np.sqrt(np.dot(w, w))
            h[j + 1] = hn
            if hn > 0:
                V[j + 1] = w / hn
            for i in range(j):              # the earlier rotations, then the one that annihilates h[j + 1]
                a = cs[i] * h[i] + sn[i] * h[i + 1]
                h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
                h[i] = a
            d = np.sqrt(h[j] * h[j] + h[j + 1] * h[j + 1])
            cs[j], sn[j] = (h[j] / d, h[j + 1] / d) if d > 0 else (LD(1), LD(0))
            h[j] = d
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            R[: j + 1, j] = h[: j + 1]
            its += 1
            j += 1
            if hn == 0:
                done = True
                break
        if its >= maxit:
            done = True
        y = np.zeros(j, dtype=LD)
        for i in range(j - 1, -1, -1):      # back substitution
            s = g[i]
            for q in range(i + 1, j):
                s = s - R[i, q] * y[q]
            y[i] = s / R[i, i] if R[i, i] != 0 else LD(0)
        for q in range(j):
            x = x + y[q] * V[q]
    return x, its


def class_dist(x, x_ld, mask):
    """max|x - x_ld| over the class / max|x_ld| over the class (None for an empty class)"""
    if not mask.any():
        return None
    d = np.abs(ld(x) - x_ld)[mask].max()
    return float(d / np.abs(x_ld)[mask].max())


class Hierarchy:
    """The references of one (case, design, boundary condition): the float64 oracle's hierarchy (row scales, the oracle's own
    sweeps) and the 80-bit arbiter's (the matrices everything is held to)"""

    def __init__(self, orc, arb, case, KE, E, N):
        (ex, ey, ez), nlv, _ = case
        self.dims, self.nlv = (ex + 1, ey + 1, ez + 1), nlv
        self.KE, self.E, self.N = np.asarray(KE, dtype=np.float64), np.asarray(E, dtype=np.float64), np.asarray(N, dtype=np.float64)
        self.orc = orc
        self.mg, self.amg = orc.MG(*self.dims, 3, nlv), arb.MG(*self.dims, 3, nlv)
        self.mg.assemble(self.KE, self.E, self.N)
        self.amg.assemble(ld(self.KE), ld(self.E), ld(self.N))
        self._csr = {}

    def csr(self, l):
        if l not in self._csr:
            self._csr[l] = LevelCsr(self.amg, l)
        return self._csr[l]

    def level_dims(self, l):
        return rw.level_dims(*self.dims, l)

    def check_sweep(self, l, b, x0, x1, backward, label, c=None):
        """assert_rowwise on the sweep's mixed residual; -> the achieved c"""
        res = self.csr(l).sweep_residual(b, x0, x1, backward)
        s = sweep_scale(self.orc, self.mg, l, self.dims, self.KE, self.E, self.N, b, x0, x1)
        return rw.assert_rowwise(np.zeros(res.size), res, s, c_gs(l) if c is None else c, {"label": label, "dims": self.level_dims(l)})
