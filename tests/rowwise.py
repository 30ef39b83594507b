"""Row-wise error bounds for the operator kernels on 0/1 designs (a plain helper module: no fixtures, no collection hooks).

Why: rel(a, b) = max|a - b| / max|b| measures every row against the LARGEST row.  With Emin = 1e-9, Emax = 1, p = 3 the rows
of K(x) that touch only void elements are ~1e-9 of the largest ones, so a tolerance of 1e-13 max|y| leaves them unchecked
beyond four digits -- and a converged design is exactly such a field.  Here every row i is held to

    |got_i - ref_i| <= c * eps * scale_i,        eps = 2^-53,

`ref` from the 80-bit arbiter (oracle/arbiter.py) and `scale_i` the sum of the absolute values of the terms that make up
row i (a majorant of it, computed with the float64 oracle -- its own rounding, 1e-16 of itself, does not matter):

    level 0      s = matfree_apply(KE -> max|KE| ones, E, N -> ones, |u|)  =  sum_{e in i} E_e max|KE| ||u_e||_1
    level l > 0  S_l(v) = restrict(S_{l-1}(prolong(v))), v = |u|: P and R are non-negative, so this bounds |R A P| |u| and
                 the rounding of the stored Galerkin coefficients alike
    transfers    R |r|  and  |x_f| + P |x_c|
    one Chebyshev step   |x0| + c dinv (|b| + S_l(|x0|)),  c = 1 / theta of the level's window
    dfdx         p x^(p-1) (Emax - Emin) max|KE| ||u_e||_1^2   per element
    cone filter  H'|x| / Hs + (H|x| / Hs) rho  with the majorant weights H' = H + (R + L) B (class Cone below: B the 0/1
                 pattern of H, L the largest element-centre coordinate, rho = (R + L) B1 / Hs); gradients: the same on |df|
    Helmholtz filter   level l: |K_f|_l |u|, the scalar hierarchy assembled from abs(kf); element <-> node: T|x|, T^T|u|
                 (the section "the Helmholtz (PDE) filter's scalar hierarchy" below)

THE CONSTANTS c come from the length of the chain of rounded operations of the form, never from what the HIP kernels
achieve; beside each: the count, and what the float64 oracle measures against the arbiter on the CPU
(tests/test_rowwise_oracle.py holds the oracle to a QUARTER of each, on every generator below).  Rule: the larger of the
count and 16 x the measured value, rounded up to a power of two.
"""
import numpy as np

EPS = 2.0 ** -53

# ---- level 0 product (apply, apply_krylov, residual): 3 + 3 butterfly stages of the Walsh-Hadamard form, dot products of
# at most 24 terms, the modulus scale, the 8-element nodal sum, ~5 eps of representation error of the packed form against
# its double-double export: gamma ~ 50.  Oracle against arbiter, measured: 1.11 over the generators (x 16 = 18); 0.57
# on the planted-error mesh.
C_FINE = 64


def c_level(l):
    """stored / applied Galerkin level l >= 1.  Count: the row's dot product over 27 neighbours x 3 components (81), the nodal
    sum over 8 coarse elements (8), and per Galerkin step l' <= l the two contractions of a child's 24 dofs with the
    interpolation weights (24 + 24 additions; the weights are powers of two, their products exact) and the sum over the 8
    children (8): 89 + 56 l -> 256 for l = 1, 2, 512 for l = 3, 4.  The reference hierarchy is the arbiter's Galerkin
    product of KE; level 1 applied from the fine densities uses a packed tensor of KE's children, whose representation error
    (~5 eps of max|KE|, as on level 0) is inside this count's slack (145 of 256).  Oracle against arbiter, measured: 5.24 (x 16 = 84)."""
    return _pow2(89 + 56 * l)


def c_diag(l):
    """the Jacobi diagonal (exported as its reciprocal), RELATIVE to the row's own diagonal entry.  Count: level 0 the 8-element
    sum of positive terms, the modulus scale, the reciprocal and the test's own division back: 11; level l the
    coefficient's formation as in c_level (8 + 56 l) + 2: 66, 122, 178.  Oracle (assembled CSR) against arbiter, measured:
    3.94 on level 0 (x 16 = 63 -> 64), 14.7 on levels 1, 2 (x 16 = 235 -> 256): the measured values set both."""
    return 64 if l == 0 else max(256, _pow2(10 + 56 * l))


# restriction: a coarse row gathers <= 27 fine nodes with power-of-two weights: 27 additions.  Measured: 3.26 (x 16 = 52 -> 64).
C_RESTRICT = 64
# prolongation + add: <= 8 coarse nodes, then the sum with x_f: 9.  Measured: 2.10 (x 16 = 34 -> 64).
C_PROLONG = 64


def c_smooth(l):
    """one Chebyshev step x1 = x0 + (1/theta) dinv (b - A x0), the reference step formed in 80-bit arithmetic from the
    DEVICE's dinv and window.  Count: the product's chain (C_FINE or c_level(l)'s count) + 1/theta, b - Ax, x dinv, x 1/theta,
    + x0 (5); the fine level forms its Jacobi diagonal on the fly (8-element sum of positive terms + modulus scale +
    reciprocal: 11) -> 50 + 16 = 66 -> 128 on level 0, 94 + 56 l -> 256 / 256 / 512 on levels 1 / 2 / 3.  Oracle against
    arbiter, measured: 3.20 (x 16 = 51)."""
    return _pow2(66) if l == 0 else _pow2(94 + 56 * l)


def c_smooth_k(l):
    """step k >= 2 of a sweep, x_k = x_{k-1} + c1 (x_{k-1} - x_{k-2}) + c2 dinv (b - A x_{k-1}), the reference step formed in 80-bit
    arithmetic from the DEVICE's own x_{k-1}, x_{k-2}, dinv and window.  Count: c_smooth(l)'s + the subtraction, its product
    with c1, the sum with the residual term, and one unit for the levels that keep the direction d = x_{k-1} - x_{k-2} as a
    stored vector (it differs from the difference of the stored iterates by <= eps |x_{k-1}|, which the scale's first term
    carries): + 4 -> 70 -> 128 on level 0, 98 + 56 l -> 154, 210, 266 -> 256 / 256 / 512 on levels 1 / 2 / 3.  Oracle against
    arbiter (step k from the oracle's own x_{k-1}, x_{k-2}; k = 2, 3, 4 and 20 on the coarsest level), measured on the meshes of
    tests/test_rowwise_oracle.py: 1.97 / 1.23 / 0.74 on levels 0 / 1 / 2 (x 16 = 32, 20, 12)."""
    return _pow2(70) if l == 0 else _pow2(98 + 56 * l)


def c_resid(l):
    """the V-cycle's residual r = b - A_l x (EPI_RESID).  Count: the product's chain (C_FINE's 50, c_level(l)'s 89 + 56 l) + the
    subtraction: 51 -> 64 = C_FINE on level 0, 90 + 56 l -> 256 / 256 / 512 = c_level(l) above.  Oracle against arbiter,
    measured: 1.07 / 4.16 / 3.82 on levels 0 / 1 / 2 (x 16 = 18, 67, 62)."""
    return _pow2(51) if l == 0 else _pow2(90 + 56 * l)


def dot_chain(kz, nwg):
    """longest chain of additions a term of a fused dot product passes through (EPI_APPLY_DOT's u . A u, EPI_CHEB_DOT's b . x_out):
    the thread's fma chain over the kz planes of its z-chunk x 3 components (per-node kernel: kz = 1), the workgroup's sum
    (wave_sum's 6 shuffle stages, then the 4 waves' sums added in turn), and the reduction tail over the nwg partials (a thread
    of the last workgroup adds every 256th partial: ceil(nwg / 256); then the workgroup's sum again): 3 kz + 20 + ceil(nwg / 256)"""
    return 3 * kz + 20 + (nwg + 255) // 256


def c_dot(kz, nwg):
    """|got - sum| <= c eps sum |terms|, the sum formed in 80-bit arithmetic from the device's OWN vectors (the products inside the
    fma are exact): c = the chain's length rounded up to a power of two.  Such a bound holds for any float64 summation of that
    depth: no oracle figure, like C_PDE_T."""
    return _pow2(dot_chain(kz, nwg))


def dot_workgroups(form, dims):
    """workgroups (= partials) of a fused-dot launch over the whole level: form as last_op_form returns it, dims the node counts"""
    nx, ny, nz = dims
    kind, _, shape, kz = (int(v) for v in form)
    if kind == 3:                           # a thread per node
        return (nx * ny * nz + 255) // 256
    assert kind == 1 and kz >= 1, form
    tiles = ((nx + 30) // 31) * ((ny + 6) // 7) if shape == 2 else ((nx + 14) // 15) * ((ny + 14) // 15)
    return tiles * ((nz + kz - 1) // kz)


# dfdx per element: u_e^T KE u_e as 24 dot products of 24 terms and a 24-term sum (48), pow(x, p - 1) (<= 2), three scale
# factors (3): 53.  Measured: 6.91 (x 16 = 111 -> 128).
C_DFDX = 128


# the meshes of tests/test_gpu_rowwise.py (elements; COARSE_MESHES with their level count)
# elements; nx = 15, 16, 17, 31, 32, 33, 62, 63 and ny = 7, 8, 9, 15, 16 (the seams of the 15-node and the 31 x 7 tiles and one plane
# either side), 45 planes twice (more than the 43-plane chunk of the 32 x 8 tiles), and the two odd meshes of test_odd_sized_mesh_apply
FILTER_MESH = (26, 22, 20)      # cone filter: ElemConn 10 needs 20 elements every way
FILTER_RFACS = (1.5, 2.56, 5.12, 10.24)   # ElemConn 1, 2 (tiled), 5 (wide), 10 (streamed ring)
FINE_MESHES = [(14, 6, 2), (15, 7, 3), (16, 8, 44), (30, 14, 7), (31, 15, 12), (32, 6, 9), (61, 8, 16), (62, 15, 44), (31, 17, 5), (33, 4, 2)]
COARSE_MESHES = [((36, 28, 20), 3), ((40, 24, 16), 4)]
# later Chebyshev steps, the residual epilogue and the fused dot products (the arbiter's products of the device's own iterates
# cannot be shared between forms): smaller than one tile / the seams of both tile shapes / 45 planes, more than one z-chunk
STEP_MESHES = [(14, 6, 2), (31, 15, 12), (16, 8, 44)]
STEP_KS = (2, 3)                # step k of a sweep from a zero and from a non-zero guess; the coarsest level also STEP_K_COARSEST
CG_FUSION_KINDS = ("blocks", "checker", "zlayer")       # tests/test_gpu_cg_fusions.py, on COARSE_MESHES
STEP_K_COARSEST = 20            # (from the zero guess the default there is the one-launch run, coarse_run.h)


def c_filter(conn):
    """cone filter, forward and gradients.  Count: one fma chain over the (2 conn + 1)^3 window for H v, the same for Hs, the
    division and the gradient forms' pre- / post-scalings (3): 2 (2 conn + 1)^3 + 3 -> conn 1: 57 -> 64, 2: 253 -> 256,
    5: 2665 -> 4096, 10: 18525 -> 32768.  The chain is long, but every weight is non-negative: the scale is the size of the
    row's own terms.  The weights R - dist cancel: the reference forms dist from element-centre COORDINATES (size <= L), so each
    weight carries an absolute error of ~eps (R + L) whatever its size -- the scale's second term (Cone), not the constant.
    Oracle against arbiter, measured: 1.11 (x 16 = 18) at conn 1, 2, 5."""
    return _pow2(2 * (2 * conn + 1) ** 3 + 3)


def _pow2(v):
    return 1 << int(np.ceil(np.log2(v)))


pow2 = _pow2        # (the name for other helper modules: tests/response_rowwise.py)


# =====================================================================================================================
# the Helmholtz (PDE) filter's scalar hierarchy (tests/test_gpu_pde_rowwise.py): K_f of an anisotropic box, one 8 x 8 matrix per
# level, no moduli and no Dirichlet rows.  Row scales: level l  |K_f|_l |u| -- the hierarchy assembled from abs(kf) applied to
# abs(u): the transfer weights are non-negative, so the Galerkin product of |kf| majorises the terms of every coarse row and the
# rounding of the coarse 8 x 8 matrices; transfers and the Chebyshev step as above; element <-> node  T|x| and T^T|u|; the
# Jacobi diagonal relative to its own entry.
# =====================================================================================================================
def c_pde_level(l):
    """K_f on level l.  Count: the gather form sums 8 elements x 8 corners (64 fma; the table form 7 additions per weight and 27
    fma: 34), and per Galerkin step the sum over the children c and their corners a, b of W[c, a, I] KF[a, b] W[c, b, J]: of
    its 512 terms at most 5^3 = 125 are non-zero (per axis the pairs (child, corner) that see a coarse node: 3 of 4; both
    corners: 5 of 8 on the diagonal, 4 off it), the weights are powers of two: 64 + 125 l -> 64, 189, 314.  Oracle (assembled
    CSR, Galerkin by sparse products) against arbiter, measured over the meshes, regimes and inputs of PDE_CASES and PDE_SLAB3:
    4.88 / 4.81 / 3.38 on levels 0 / 1 / 2 (x 16 = 78, 77, 54): level 0 takes 128 from the measured value, the levels 1 and 2
    take 256 and 512 from the count."""
    return max(128, _pow2(64 + 125 * l))


def c_pde_diag(l):
    """the scalar Jacobi diagonal (exported as its reciprocal), RELATIVE to the row's own entry.  Count: the 8-element sum of
    positive entries, the reciprocal and the test's own division back: 10, and 125 per Galerkin step: 10, 135, 260.  Oracle
    against arbiter, measured: 1.84 / 4.49 / 7.59 on levels 0 / 1 / 2 (x 16 = 30, 72, 121) -> 32 from the measured value, 256
    and 512 from the count.  (A coarse diagonal entry is the energy of a hat function, a sum of terms of both signs: where the
    stiffness dominates, rmin / h = 100, its |kf| majorant is 3.0 times the entry on level 1 and 12.0 times on level 2 -- the
    oracle's growing figures; a worst-case sum would need count x majorant, the bound keeps to the rule.)"""
    return 32 if l == 0 else _pow2(10 + 125 * l)


def c_pde_smooth(l):
    """one Chebyshev step on level l with the level's STORED dinv: the product's count + 1/theta, b - Ax, x dinv, x 1/theta,
    + x0 (5): 69, 194, 319 -> 128, 256, 512.  Oracle against arbiter, measured: 2.92 / 3.09 / 2.56 (x 16 <= 50)."""
    return _pow2(69 + 125 * l)


def c_pde_smooth_k(l):
    """step k >= 2 of a sweep on level l (c_smooth_k's form and reference): c_pde_smooth's count + 4: 73, 198, 323 -> 128, 256,
    512.  Oracle against arbiter, measured on PDE_CASES (k = 2, 3): 3.63 / 2.49 / 1.53 (x 16 <= 59)."""
    return _pow2(73 + 125 * l)


# the scalar transfers are the elasticity's with one component: C_RESTRICT, C_PROLONG.  Measured on PDE_CASES: 2.90 and 2.52
# (x 16 = 46 and 40 -> 64 both).
# element <-> node: 8 terms of 0.125 x (exact products), the first addition to 0 exact: 7 rounded additions -> 8, a bound that
# holds for ANY float64 evaluation in that order.  (No oracle function: tests/test_rowwise_oracle.py holds a float64 numpy
# restatement, summed in the kernels' order, to the same 8 -- it measures 3.04; the rule's 16 x measured = 64 would only be
# looser than what the count already guarantees.)
C_PDE_T = 8

# elements, (hx, hy, hz) or None = cube of h = 1 / ey, levels, rmin / min(h)
PDE_RATIOS = (0.08, 2.56, 100.0)     # mass term dominates / the project's default / stiffness dominates, rows cancel
PDE_CASES = [
    ((20, 12, 8), (0.05, 0.04, 0.03), 3, PDE_RATIOS),   # anisotropic; coarsest 5 x 3 x 2
    ((8, 4, 4), None, 3, PDE_RATIOS),                   # coarsest 2 x 1 x 1: one element wide, every node in a boundary class
    ((13, 7, 3), (0.1, 0.07, 0.2), 1, (2.56,)),         # odd sizes; 448 nodes
    ((33, 4, 2), None, 1, (2.56,)),                     # 510 nodes: two workgroups, the second partly filled
    ((36, 28, 20), (0.03, 0.04, 0.05), 3, (2.56,)),     # many workgroups on every level
]
PDE_STEP_CASES = 2                                      # later Chebyshev steps (STEP_KS): the first two cases, all their regimes
PDE_SLABS = [(0, 2), (None, 3)]                         # (case, ranks); None: (8, 4, 12) cube below, three slabs
PDE_SLAB3 = ((8, 4, 12), None, 3, (2.56,))
_LX, _LY, _LZ = (0, 1, 1, 0, 0, 1, 1, 0), (0, 0, 1, 1, 0, 0, 1, 1), (0, 0, 0, 0, 1, 1, 1, 1)    # the reference's corner order


def pde_box(case):
    (ex, ey, ez), h = case[0], case[1]
    return h if h is not None else (1.0 / ey,) * 3


def pde_unit_nodes(dims):
    """[(name, (a, b, a'))]: a corner, an edge, a face and an interior node a of the level (on a level one element wide: what
    there is of them), its diagonal neighbour b (towards the inside) and its mirror image a' through the centre of the box"""
    nx, ny, nz = dims
    idx = lambda p: p[0] + nx * (p[1] + ny * p[2])
    out = []
    for name, a in (("corner", (0, 0, 0)), ("edge", (nx // 2, 0, 0)), ("face", (nx // 2, ny // 2, 0)), ("interior", (nx // 2, ny // 2, nz // 2))):
        b = tuple(v + 1 if v + 1 < n else v - 1 for v, n in zip(a, dims))
        am = tuple(n - 1 - v for v, n in zip(a, dims))
        out.append((name, (idx(a), idx(b), idx(am))))
    return out


def pde_inputs(dims, seed):
    """the inputs of one level: {name: vector}: seeded normal field (and a second one: right-hand side / coarse vector), the
    constant 1, the linear field i + 2 j + 3 k, unit vectors (pde_unit_nodes)"""
    nx, ny, nz = dims
    n = nx * ny * nz
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out = {"normal": rng.standard_normal(n), "b": rng.standard_normal(n), "one": np.ones(n), "linear": (i + 2.0 * j + 3.0 * k).reshape(-1)}
    for name, nodes in pde_unit_nodes(dims):
        for t, q in zip(("a", "b", "m"), nodes):
            e = np.zeros(n)
            e[q] = 1.0
            out["unit_%s_%s" % (name, t)] = e
    return out


PDE_FIELDS = ("normal", "one", "linear")


def pde_seed(m, r, l):
    return 7000 + 100 * m + 10 * r + l


def pde_t_inputs(m, nel, nn):
    """the inputs of the element <-> node transfers of case m: {name: (element field, nodal field)}"""
    rng = np.random.default_rng(pde_seed(m, 9, 9))
    return {"seeded": (rng.random(nel), rng.random(nn)), "one": (np.ones(nel), np.ones(nn))}


def pde_T(x, ex, ey, ez, dtype=np.float64):
    """T x: node <- the eighth of every adjacent element, summed in the kernel's order (corner a = 0 .. 7 of the node)"""
    p = np.zeros((ez + 2, ey + 2, ex + 2), dtype=dtype)
    p[1:-1, 1:-1, 1:-1] = np.asarray(x, dtype=dtype).reshape(ez, ey, ex)
    s = np.zeros((ez + 1, ey + 1, ex + 1), dtype=dtype)
    for a in range(8):       # element (i - LX[a], j - LY[a], k - LZ[a]) -> padded index + 1
        s += dtype(0.125) * p[1 - _LZ[a]:ez + 2 - _LZ[a], 1 - _LY[a]:ey + 2 - _LY[a], 1 - _LX[a]:ex + 2 - _LX[a]]
    return s.reshape(-1)


def pde_Tt(u, ex, ey, ez, dtype=np.float64):
    """T^T u: element <- the eighth of each of its 8 nodes, in corner order"""
    v = np.asarray(u, dtype=dtype).reshape(ez + 1, ey + 1, ex + 1)
    s = np.zeros((ez, ey, ex), dtype=dtype)
    for a in range(8):
        s += dtype(0.125) * v[_LZ[a]:ez + _LZ[a], _LY[a]:ey + _LY[a], _LX[a]:ex + _LX[a]]
    return s.reshape(-1)


def pde_table(KF):
    """numpy restatement of the 27 x 27 class table of the scalar operator from its 8 x 8 element matrix: W[class, offset],
    class = (cz 3 + cy) 3 + cx with c = 0 no lower element / 1 both / 2 no upper element along the axis, offset =
    (dz + 1) 9 + (dy + 1) 3 + (dx + 1); W = sum over the existing elements around the node (the node their corner a) of KF[a, b]
    at the offset of corner b"""
    KF = np.asarray(KF).reshape(8, 8)
    W = np.zeros((27, 27), dtype=KF.dtype)
    for cz in range(3):
        for cy in range(3):
            for cx in range(3):
                w = W[(cz * 3 + cy) * 3 + cx]
                for a in range(8):
                    if any((c == 0) if l else (c == 2) for l, c in ((_LX[a], cx), (_LY[a], cy), (_LZ[a], cz))):
                        continue
                    for b in range(8):
                        w[(_LZ[b] - _LZ[a] + 1) * 9 + (_LY[b] - _LY[a] + 1) * 3 + (_LX[b] - _LX[a] + 1)] += KF[a, b]
    return W


def pde_table_apply(W, dims, u):
    """y = A u from the class table: what the table kernel computes, in numpy"""
    nx, ny, nz = dims
    cls = lambda n: np.where(np.arange(n) == 0, 0, np.where(np.arange(n) == n - 1, 2, 1))
    cz, cy, cx = np.meshgrid(cls(nz), cls(ny), cls(nx), indexing="ij")
    c = (cz * 3 + cy) * 3 + cx
    p = np.zeros((nz + 2, ny + 2, nx + 2), dtype=W.dtype)
    p[1:-1, 1:-1, 1:-1] = np.asarray(u, dtype=W.dtype).reshape(nz, ny, nx)
    y = np.zeros((nz, ny, nx), dtype=W.dtype)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y += W[c, (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)] * p[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx]
    return y.reshape(-1)


def pde_galerkin(KF):
    """the next coarser level's 8 x 8 matrix: sum over the 8 children c of W_c^T KF W_c, W_c[a, I] the trilinear weight of coarse
    corner I at corner a of child c (constant coefficients: one matrix per level)"""
    KF = np.asarray(KF).reshape(8, 8)
    out = np.zeros((8, 8), dtype=KF.dtype)
    for c in range(8):
        Wc = np.zeros((8, 8), dtype=KF.dtype)
        for a in range(8):
            pos = (_LX[c] + _LX[a], _LY[c] + _LY[a], _LZ[c] + _LZ[a])          # fine coordinates 0 .. 2 inside the coarse element
            for I in range(8):
                w = 1.0
                for q, L in zip(pos, (_LX[I], _LY[I], _LZ[I])):
                    w *= (q / 2.0) if L else (1.0 - q / 2.0)
                Wc[a, I] = w
        out += Wc.T @ KF @ Wc
    return out


class PdeRef:
    """The references of one filter: the float64 oracle hierarchy of kf (row scales of the transfers, the oracle's own figures),
    the same of abs(kf) (row scales of the products) and the 80-bit arbiter's of kf."""

    def __init__(self, orc, arb, dims, nlv, kf):
        nx, ny, nz = dims
        self.dims, self.nlv = dims, nlv
        kf = np.asarray(kf, dtype=np.float64)
        self.mg, self.mga, self.amg = orc.MG(nx, ny, nz, 1, nlv), orc.MG(nx, ny, nz, 1, nlv), arb.MG(nx, ny, nz, 1, nlv)
        self.mg.assemble(kf)
        self.mga.assemble(np.abs(kf))
        self.amg.assemble(np.ascontiguousarray(kf, dtype=np.longdouble))

    def scale(self, l, u):
        return self.mga.apply(l, np.abs(np.asarray(u, dtype=np.float64)))

    def theta(self, l, lam, lam_min):
        return 0.5 * (1.1 * lam + (lam_min if (l == self.nlv - 1 and l > 0) else 0.1 * lam))


# =====================================================================================================================
# 0/1 designs: x in {XMIN, 1}, deterministic, any mesh; element (i, j, k) at x[i + ex (j + ey k)]
# =====================================================================================================================
XMIN = 1e-3
GENERATORS = ("blocks", "checker", "one_solid", "one_void", "zlayer")
# =====================================================================================================================
# z-slabs: the cases on which the elasticity hierarchy's slab forms are to be held (tests/test_rowwise_oracle.py holds the float64
# oracle to a quarter of every constant on them; the device side is not in the tree yet).  A row's arithmetic does not depend on
# who owns it: the one-rank constants above hold row for row (level 1's correction adds its gathered products to the tile's sum
# on one rank and on slabs alike, compact ghost rows included: the same count).  The fused dot products alone have a longer
# chain: c_dot_slab.
# =====================================================================================================================
SLAB_GENERATORS = GENERATORS + ("seam_step", "seam_void")       # design(kind, ..., nranks=): the last two need the rank count
# (mesh in elements, ranks): two element layers per rank, the thinnest the library accepts (the middle rank's interior pass is
# empty) / odd ez_own, 510 nodes per plane pair / nx = 32, ny = 16 on the seams of both tile shapes, 8 planes per rank / two
# ranks (the auto form only): both are end ranks, an even split
SLAB_FINE = [((16, 8, 6), 3), ((33, 4, 9), 3), ((31, 15, 24), 3), ((31, 15, 12), 2)]
# (mesh, ranks, levels): the one-rank coarse mesh in x and y, two layers per rank on level 2 / two layers per rank on level 3 /
# ONE layer per rank on the coarsest level (check_solver_opts allows it: that level is solved on its replicated copy; the
# slab's own stored stencil there feeds that copy and is held like every other level)
SLAB_COARSE = [((36, 28, 24), 3, 3), ((24, 8, 48), 3, 4), ((16, 8, 12), 3, 3)]


def slab_inputs(job, m, scattered, l, n, nc):
    """(u, b, xc) of level l: seeded GLOBAL vectors of n and nc (next coarser level; 0: none) entries, the same on every rank
    and in the parent"""
    rng = np.random.default_rng(20000 + 5000 * (job == "coarse") + 100 * m + 10 * scattered + l)
    return rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nc)


def slab_bc(orc, nx, ny, nz, h, scattered, seed):
    """(N, R) on the GLOBAL mesh: the cantilever, or the scattered Dirichlet mask of tests/rowwise_worker.py: bc"""
    if not scattered:
        return orc.cantilever_bc(nx, ny, nz, h)
    rng = np.random.default_rng(seed)
    N = np.ones(3 * nx * ny * nz)
    N[rng.random(N.size) < 2e-2] = 0.0
    N[: 3 * nx] = 0.0
    return N, rng.standard_normal(N.size) * 1e-3


def slab_owned_planes(nz, nranks):
    """node planes each rank owns: ez_own each, rank 0 also plane 0"""
    own = (nz - 1) // nranks
    return [own + (1 if r == 0 else 0) for r in range(nranks)]


def c_dot_slab(kzs, nwgs):
    """a fused dot product on slabs: rank r's partial goes through dot_chain(kzs[r], nwgs[r]) over its own workgroups, the
    all-reduce adds nranks - 1 more additions: the power of two above the longest such chain.  Holds for any float64 summation of
    that depth: no oracle figure, like c_dot"""
    return _pow2(max(dot_chain(k, w) for k, w in zip(kzs, nwgs)) + len(nwgs) - 1)


# node planes that carry block faces: the seams of the 15-node tiles (15, 30 -> 14..16, 30..32 with the tiles' overlap) and of
# the 31 x 7 tiles (31; 7, 14), and one plane either side of them
_FX = (13, 14, 15, 16, 17, 29, 30, 31, 32, 33)
_FY = (5, 6, 7, 8, 9, 13, 14, 15, 16, 17)


def design(kind, ex, ey, ez, kz=8, nranks=1):
    """-> float64 array of ex ey ez densities; kz: z-chunk length of the kernel under test (node planes per chunk), or a tuple
    of the lengths of several forms (product and Chebyshev step may chunk differently): a solid layer at every boundary;
    nranks: the z-slabs of the two seam designs (SLAB_GENERATORS), ez / nranks element layers each"""
    solid = np.zeros((ez, ey, ex), dtype=bool)
    if kind in ("seam_step", "seam_void"):
        assert nranks >= 2 and ez % nranks == 0 and ez // nranks >= 2, (kind, ez, nranks)
        own = ez // nranks
        if kind == "seam_step":         # slab r solid for even r: solid below the first seam and void above it, the reverse at the next
            solid[(np.arange(ez) // own) % 2 == 0] = True
        else:                           # the element layer below and the one above every seam void, everything else solid
            solid[:] = True
            for r in range(1, nranks):
                solid[r * own - 1:r * own + 1] = False
    elif kind == "blocks":
        # block m: one with its LOW faces on the planes i = _FX[m], j = _FY[m], one with its HIGH faces there (they touch along
        # an edge only), w = 2..4 elements wide, in a band of two element layers of its own
        for m in range(len(_FX)):
            w, k0 = 2 + m % 3, (2 * m) % max(ez, 1)
            for (i0, i1), (j0, j1) in ((( _FX[m], _FX[m] + w), (_FY[m], _FY[m] + w)), ((_FX[m] - w, _FX[m]), (_FY[m] - w, _FY[m]))):
                i0, i1, j0, j1 = max(i0, 0), min(i1, ex), max(j0, 0), min(j1, ey)
                # a mesh that ends before the plane still gets the block against its last plane
                if i0 >= i1:
                    i0, i1 = max(ex - w, 0), ex
                if j0 >= j1:
                    j0, j1 = max(ey - w, 0), ey
                solid[k0:k0 + 2, j0:j1, i0:i1] = True
    elif kind == "checker":
        k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
        lo = lambda n: n // 4
        hi = lambda n: max(n // 4 + 1, n - n // 4)
        region = (i >= lo(ex)) & (i < hi(ex)) & (j >= lo(ey)) & (j < hi(ey)) & (k >= lo(ez)) & (k < hi(ez))
        solid = region & ((i + j + k) % 2 == 0)
    elif kind == "one_solid":
        solid[ez // 2, ey // 2, ex // 2] = True
    elif kind == "one_void":
        solid[:] = True
        solid[ez // 2, ey // 2, ex // 2] = False
    elif kind == "zlayer":
        # the element layer whose lower node plane is the FIRST plane of a chunk: k = kz, 2 kz, ... (its upper plane is the chunk's
        # second plane, the layer below it belongs to the chunk before); a mesh of one chunk: its last layer
        kzs = kz if isinstance(kz, (tuple, list)) else (kz,)
        ks = sorted({k for k in range(1, ez) for q in kzs if k % max(q, 1) == 0}) or [ez - 1]
        solid[ks, :, :] = True
    else:
        raise ValueError(kind)
    return np.where(solid, 1.0, XMIN).reshape(-1)


# the cone filter alone also sees designs with EXACT zeros (Xmin = 0: MMA puts designs on their bounds, Passive holds void elements
# there): blocks and checker with XMIN replaced by 0.0.  Not in GENERATORS -- the operator tests iterate over that.
FILTER_ZERO_KINDS = ("blocks_zero", "checker_zero")


def filter_design(kind, ex, ey, ez, kz=8):
    """design() for the cone filter's tests: the kinds of GENERATORS, and those of FILTER_ZERO_KINDS"""
    if kind not in FILTER_ZERO_KINDS:
        return design(kind, ex, ey, ez, kz)
    x = design(kind[:-len("_zero")], ex, ey, ez, kz)
    return np.where(x == XMIN, 0.0, x)


# =====================================================================================================================
# row scales
# =====================================================================================================================
def level_dims(nx, ny, nz, l):
    return ((nx - 1) >> l) + 1, ((ny - 1) >> l) + 1, ((nz - 1) >> l) + 1


def scale_fine(orc, nx, ny, nz, KE, E, u, N=None):
    """sum over the elements of a row of E_e max|KE| ||u_e||_1 (N -> ones: a clamped neighbour only lowers the true sum).  With N:
    a Dirichlet row carries |u| instead, the identity the operator has there -- what the coarser levels' Galerkin products see
    of it (on level 0 itself those rows must return u bit for bit: the caller sets their scale to 0)"""
    n = 3 * nx * ny * nz
    kmax = np.full(576, float(np.abs(np.asarray(KE, dtype=np.float64)).max()))
    au = np.abs(np.asarray(u, dtype=np.float64))
    s = orc.matfree_apply(nx, ny, nz, 3, kmax, orc.f64(E), np.ones(n), au)
    return s if N is None else np.where(np.asarray(N) != 0, s, au)


def scale_level(orc, mg, l, dims, KE, E, N, u):
    """S_l(|u|) = R_{l-1} ... R_0 S_0(P_0 ... P_{l-1} |u|); mg: an assembled orc.MG of the same mesh (its transfers are used)"""
    v = np.abs(np.asarray(u, dtype=np.float64))
    for m in range(l - 1, -1, -1):
        v = mg.prolong(m, v)
    s = scale_fine(orc, *dims, KE, E, v, N)
    for m in range(l):
        s = mg.restrict(m, s)
    return s


def scale_restrict(mg, l, rf):
    return mg.restrict(l, np.abs(np.asarray(rf, dtype=np.float64)))


def scale_prolong_add(mg, l, xc, xf):
    return np.abs(np.asarray(xf, dtype=np.float64)) + mg.prolong(l, np.abs(np.asarray(xc, dtype=np.float64)))


def scale_smooth(s_x0, dinv, inv_theta, b, x0):
    """|x0| + c dinv (|b| + S_l(|x0|)); s_x0 = S_l(|x0|) (zeros for a zero guess)"""
    return np.abs(x0) + inv_theta * np.abs(dinv) * (np.abs(b) + s_x0)


def cheb_coeffs(theta, delta, k):
    """(c1, c2) of step k >= 2 of a sweep, by MGSolver::smooth's recurrence in float64 (the host code's own arithmetic)"""
    sigma = theta / delta
    rho = 1.0 / sigma
    for _ in range(1, k):
        rn = 1.0 / (2.0 * sigma - rho)
        c1, c2 = rn * rho, 2.0 * rn / delta
        rho = rn
    return c1, c2


def step_k_ref(x1, x2, c1, c2, dinv, b, Ax1_ld):
    """x_k in 80-bit arithmetic from x_{k-1}, x_{k-2} and the arbiter's A x_{k-1}"""
    L = lambda a: np.asarray(a, dtype=np.longdouble)
    return L(x1) + np.longdouble(c1) * (L(x1) - L(x2)) + np.longdouble(c2) * L(dinv) * (L(b) - Ax1_ld)


def scale_smooth_k(s_x1, dinv, c1, c2, b, x1, x2):
    """|x_{k-1}| + c1 (|x_{k-1}| + |x_{k-2}|) + c2 dinv (|b| + S_l(|x_{k-1}|)); s_x1 = S_l(|x_{k-1}|)"""
    return np.abs(x1) + abs(c1) * (np.abs(x1) + np.abs(x2)) + abs(c2) * np.abs(dinv) * (np.abs(b) + s_x1)


def elem_u1(nx, ny, nz, U):
    """||u_e||_1 per element"""
    a = np.abs(np.asarray(U, dtype=np.float64)).reshape(nz, ny, nx, 3).sum(-1)
    s = np.zeros((nz - 1, ny - 1, nx - 1))
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                s += a[dk:nz - 1 + dk, dj:ny - 1 + dj, di:nx - 1 + di]
    return s.reshape(-1)


def scale_dfdx(nx, ny, nz, KE, U, x, Emin=1e-9, Emax=1.0, penal=3.0):
    return penal * np.asarray(x, dtype=np.float64) ** (penal - 1) * (Emax - Emin) * float(np.abs(KE).max()) * elem_u1(nx, ny, nz, U) ** 2


class Cone:
    """The cone filter's matrix in numpy, for the row scales: H (weights R - dist < R, dist from the integer offsets), its 0/1
    pattern B (dist < R (1 + 1e-12): a weight that one side rounds to zero and the other does not is below eps R either way), and
    the majorant H' = H + (R + L) B -- every weight plus the absolute error eps (R + L) it can carry (c_filter's docstring)."""

    def __init__(self, ex, ey, ez, h, R, conn):
        self.shape, self.conn, self.R = (ez, ey, ex), conn, R
        hx, hy, hz = (h, h, h) if np.isscalar(h) else h
        self.L = max(ex * hx, ey * hy, ez * hz)
        self.taps = []
        for dk in range(-conn, conn + 1):
            for dj in range(-conn, conn + 1):
                for di in range(-conn, conn + 1):
                    dist = np.sqrt((di * hx) ** 2 + (dj * hy) ** 2 + (dk * hz) ** 2)
                    if dist < R * (1 + 1e-12):
                        self.taps.append((dk, dj, di, max(R - dist, 0.0)))
        one = np.ones(ex * ey * ez)
        self.Hs, self.n = self.H(one), self.B(one)
        self.rho = (R + self.L) * self.n / self.Hs

    def _conv(self, v, weight):
        c, (ez, ey, ex) = self.conn, self.shape
        p = np.zeros((ez + 2 * c, ey + 2 * c, ex + 2 * c))
        p[c:c + ez, c:c + ey, c:c + ex] = np.asarray(v, dtype=np.float64).reshape(self.shape)
        out = np.zeros(self.shape)
        for dk, dj, di, w in self.taps:
            out += weight(w) * p[c + dk:c + dk + ez, c + dj:c + dj + ey, c + di:c + di + ex]
        return out.reshape(-1)

    def H(self, v):
        return self._conv(v, lambda w: w)

    def B(self, v):
        return self._conv(v, lambda w: 1.0)

    def M(self, v):
        return self._conv(v, lambda w: w + self.R + self.L)

    def scale_forward(self, ftype, x):
        """type 1: x~ = H x / Hs; type 0 copies x: scale 0, i.e. bit for bit"""
        ax = np.abs(x)
        return self.M(ax) / self.Hs + self.H(ax) / self.Hs * self.rho if ftype == 1 else np.zeros(ax.size)

    def scale_gradient(self, ftype, x, df):
        """type 1: H (df / Hs); type 0: (H (df x) / Hs) / max(1e-3, x), the reference's divisor -- and 0 where x is exactly 0: the
        quotient is PETSc's, 0.0 there, bit for bit"""
        x, adf = np.asarray(x, dtype=np.float64), np.abs(df)
        if ftype == 1:
            g = adf / self.Hs
            return self.M(g) + self.H(g * self.rho)
        v = adf * np.abs(x)
        return np.where(x == 0, 0.0, (self.M(v) / self.Hs + self.H(v) / self.Hs * self.rho) / np.maximum(1e-3, x))


# =====================================================================================================================
# the assertion
# =====================================================================================================================
def rel(a, b):
    """the suite's older metric (tests/test_gpu_parity.py), kept here for the planted-error test"""
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def achieved(got, ref_ld, scale):
    """max_i |got - ref|_i / (eps scale_i) over the rows with scale > 0 (0.0 if there are none)"""
    d = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref_ld, dtype=np.longdouble)).astype(np.float64)
    pos = scale > 0
    return float((d[pos] / (EPS * scale[pos])).max()) if pos.any() else 0.0


def _describe(row, where):
    nx, ny, nz = where["dims"]
    dof, kz = where.get("dof", 3), where.get("kz", 0)
    n, c = (row // dof, row % dof) if dof else (row, -1)
    i, j, k = n % nx, (n // nx) % ny, n // (nx * ny)
    what = "node" if dof else "element"
    return ("%s (%d, %d, %d)%s, i mod 15 = %d, i mod 31 = %d, j mod 7 = %d, plane offset in its z-chunk (kz %s) = %s"
            % (what, i, j, k, " component %d" % c if dof else "", i % 15, i % 31, j % 7, kz or "-", (k - where.get("k0", 0)) % kz if kz else "-"))


describe = _describe        # (the name for other helper modules: tests/response_rowwise.py)


def assert_rowwise(got, ref_ld, scale, c, where):
    """fails if |got - ref|_i > c eps scale_i for ANY row i; rows with scale == 0 must match exactly.  where: {"label": the kernel
    form and case, "dims": (nx, ny, nz) of the level (element counts for element vectors), "dof": 3 / 1 / 0 (0: element
    vector), "kz": z-chunk length of the form (0: none), "k0": first plane of the chunking}.  -> the achieved c"""
    got = np.asarray(got)
    scale = np.asarray(scale, dtype=np.float64)
    assert got.shape == scale.shape == np.asarray(ref_ld).shape, (where.get("label"), got.shape, scale.shape, np.asarray(ref_ld).shape)
    assert np.isfinite(got).all() and np.isfinite(scale).all() and (scale >= 0).all(), where.get("label")
    d = np.abs(got.astype(np.longdouble) - np.asarray(ref_ld, dtype=np.longdouble)).astype(np.float64)
    zero = scale == 0
    if (d[zero] != 0).any():
        row = int(np.flatnonzero(zero & (d != 0))[0])
        raise AssertionError("%s: row %d has scale 0 and must match exactly, |got - ref| = %.3e (%d such rows); %s"
                             % (where.get("label"), row, d[row], int((d[zero] != 0).sum()), _describe(row, where)))
    ratio = np.zeros_like(d)
    ratio[~zero] = d[~zero] / (EPS * scale[~zero])
    row = int(np.argmax(ratio))
    if ratio[row] > c:
        raise AssertionError("%s: %d of %d rows beyond %g eps scale; worst: row %d, achieved c = %.4g (|got - ref| = %.3e, scale = %.3e, "
                             "scale / max scale = %.1e); %s" % (where.get("label"), int((ratio > c).sum()), ratio.size, c, row, ratio[row],
                                                                d[row], scale[row], scale[row] / scale.max(), _describe(row, where)))
    return float(ratio[row])


# =====================================================================================================================
# the exact coarse solve (csrc/coarse_direct.h; tests/test_gpu_coarse_direct.py): its admission window as a table, the designs
# and right-hand sides of its cases, and the distances its result is held to
# =====================================================================================================================
CD_NB, CD_KBMAX, CD_MINROWS, CD_MAXROWS, CD_RUN_ROWS = 32, 12, 128, 4096, 448


def cd_geom(mesh, nlv):
    """-> (coarsest node dims, rows, KB, blocks, padding) of the coarsest level of a mesh (elements) with nlv levels: MGSolver's
    coarse_direct_factor() restated -- half bandwidth 3 (nx ny + nx + 1) + 2 in blocks of 32 rows, rows padded to whole blocks"""
    ex, ey, ez = mesh
    cx, cy, cz = level_dims(ex + 1, ey + 1, ez + 1, nlv - 1)
    rows = 3 * cx * cy * cz
    KB = (3 * (cx * cy + cx + 1) + 2 + CD_NB - 1) // CD_NB
    blocks = (rows + CD_NB - 1) // CD_NB
    return (cx, cy, cz), rows, KB, blocks, blocks * CD_NB - rows


def cd_rows(mesh, nlv, coarse_direct):
    """rows LinearElasticity.coarse_direct_active() must report (0: the Chebyshev run): coarse_direct_ok() restated -- 128 ..
    4096 rows, 1 .. 12 blocks of band, and below 449 rows (the one-workgroup Chebyshev run) only for coarse_direct = 2"""
    _, rows, KB, _, _ = cd_geom(mesh, nlv)
    ok = coarse_direct >= 1 and nlv >= 2 and CD_MINROWS <= rows <= CD_MAXROWS and 1 <= KB <= CD_KBMAX and (coarse_direct >= 2 or rows > CD_RUN_ROWS)
    return rows if ok else 0


# (mesh in elements, levels, rows reported for coarse_direct = 1, for coarse_direct = 2): coarsest nodes, KB, blocks, padding; why
# KB = 1 needs a coarsest plane of 2 x 2 nodes: 4 x 4 x 48 elements with three levels -- the library accepts the mesh and every
# level's kernel runs on it, so the table starts at KB = 1.  KB 9 and 10 are the older tests' (tests/test_gpu_parity.py).
#
# MEASURED, energy norm of the distance from the arbiter's solve (largest over the six designs, both right-hand sides; the
# maximum norm stays within a factor of 3 of it everywhere): the float64 oracle's banded Cholesky and the numpy restatement of
# the device's method on the CPU; the device (MI355X, both inverse forms: they agree to three digits) for the reader -- the
# bound is 16 x the larger REFERENCE figure of the same design and right-hand side, never the device's own.  Worst ratio of a
# device distance to its bound over the table: 0.18.  The two inverse forms stand <= 1.1e-10 (energy) / 7.8e-15 (maximum norm)
# from each other.  Per design, the spread is that of the condition number: checker / blocks 1e-7 .. 5e-5, one_solid 1e-8,
# one_void, zlayer and synth 1e-15 .. 6e-12 (the floor's regime).
#     mesh, levels       KB    oracle    numpy W   device        worst design
#     4x4x48, 3           1    6.7e-14   6.9e-14   6.8e-14       one_solid (every other design: <= 4.3e-15)
#     8x8x24, 3           2    2.1e-06   2.1e-06   6.8e-07       blocks
#     12x12x28, 3         3    5.9e-07   5.6e-07   7.2e-07       blocks
#     28x12x20, 3         4    5.7e-06   4.6e-06   4.3e-06       checker (device: blocks)
#     20x20x20, 3         5    8.9e-07   1.2e-06   1.0e-06       blocks
#     28x28x12, 3         7    1.0e-06   8.9e-07   1.7e-06       blocks, checker
#     28x32x16, 3         8    7.9e-06   6.6e-06   1.1e-06       blocks (device: checker)
#     36x36x16, 3        11    5.8e-06   4.9e-06   4.1e-06       blocks (device: checker)
#     36x40x44, 3        12    2.0e-06   2.4e-06   2.3e-07       checker
#     64x32x32, 4         6    5.1e-05   5.3e-05   1.8e-05       checker
# The oracle and the numpy restatement stand this close to each other because most of the distance is the float64 rounding of the
# coarse MATRIX (two or three Galerkin products of moduli nine decades apart), which they share; the explicit inverse adds nothing.
CD_CASES = [
    ((4, 4, 48), 3, 0, 156),        # 2x2x13, KB 1, 5 blocks, pad 4: one ring slot; coarse_direct = 2 only
    ((8, 8, 24), 3, 0, 189),        # 3x3x7, KB 2, 6 blocks, pad 3: ring shorter than the four waves; coarse_direct = 2 only
    ((12, 12, 28), 3, 0, 384),      # 4x4x8, KB 3, 12 blocks, pad 0; coarse_direct = 2 only
    ((28, 12, 20), 3, 576, 576),    # 8x4x6, KB 4, 18 blocks, pad 0: no padding, admitted by default
    ((20, 20, 20), 3, 648, 648),    # 6x6x6, KB 5, 21 blocks, pad 24
    ((28, 28, 12), 3, 768, 768),    # 8x8x4, KB 7, 24 blocks, pad 0
    ((28, 32, 16), 3, 1080, 1080),  # 8x9x5, KB 8, 34 blocks, pad 8
    ((36, 36, 16), 3, 1500, 1500),  # 10x10x5, KB 11, 47 blocks, pad 4
    ((36, 40, 44), 3, 3960, 3960),  # 10x11x12, KB 12, 124 blocks, pad 8: widest band and most blocks, 7 levels of divide and conquer, ragged last segment
    ((64, 32, 32), 4, 675, 675),    # 9x5x5, KB 6, 22 blocks, pad 29: four levels, the early factorisation with level 2 beside it
]
# rejected whatever the option says: 0 rows, and the solve of coarse_direct = 0 bit for bit
CD_REJECTED = [
    ((40, 36, 48), 3),              # 11x10x13: 4290 rows at KB 12, too many rows
    ((8, 8, 8), 3),                 # 3x3x3: 81 rows, too few
]
CD_DESIGNS = ("blocks", "checker", "one_solid", "one_void", "zlayer", "synth")
CD_SEQUENCE = ("blocks", "checker", "blocks", "checker", "one_solid", "one_void", "zlayer", "synth")      # A, B, A, B, then the rest
CD_SETUP_CASES = (9, 3)             # indices into CD_CASES: the overlapped set-up against the serial one (the second: every switch alone)
CD_MARGIN = 16                      # the margin this file gives every measured constant
# floor of the bound (energy norm, maximum norm): the largest d(oracle) over the one_void designs of CD_CASES, where the matrix is
# well conditioned -- 5.99e-12 and 8.53e-12, both on the four-level case -- rounded up to a power of two
CD_FLOOR = (2.0 ** -37, 2.0 ** -36)


def cd_design(orc, kind, mesh):
    ex, ey, ez = mesh
    return orc.synth_density(ex, ey, ez, 1.0 / ey) if kind == "synth" else design(kind, ex, ey, ez, 4)


def cd_rhs(dims, case):
    """{name: right-hand side} on the coarsest level: a seeded normal field, and one supported on one node -- on ONE of its three
    dofs, component y of the central node, so that the solution is a single column of the inverse (a load on all three
    components would be a sum of three columns)"""
    cx, cy, cz = dims
    n = 3 * cx * cy * cz
    e = np.zeros(n)
    e[3 * (cx // 2 + cx * (cy // 2 + cy * (cz // 2))) + 1] = 1.0
    return {"normal": np.random.default_rng(4000 + case).standard_normal(n), "unit": e}


class CdNorm:
    """dist(v, x_a) = (energy norm of v - x_a in the arbiter's coarsest matrix relative to x_a's, max|v - x_a| / max|x_a|); the
    matrix is kept as 80-bit CSR arrays and applied in 80-bit arithmetic"""

    def __init__(self, amg, l):
        n, nnz = amg.size(l), amg.L.orc_mg_level_nnz(amg.h, l)
        self.rp, self.ci, self.v = np.zeros(n + 1, dtype=np.int64), np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.longdouble)
        amg.L.orc_mg_level_csr(amg.h, l, self.rp.ctypes.data, self.ci.ctypes.data, self.v.ctypes.data)
        assert (np.diff(self.rp) > 0).all()

    def energy(self, u):
        u = np.asarray(u, dtype=np.longdouble)
        return np.sqrt(np.dot(u, np.add.reduceat(self.v * u[self.ci], self.rp[:-1])))

    def dist(self, v, xa):
        d = np.asarray(v, dtype=np.longdouble) - xa
        return float(self.energy(d) / self.energy(xa)), float(np.abs(d).max() / np.abs(xa).max())


class CdRef:
    """The references of one (case, design): the arbiter's coarse_solve on its own Galerkin hierarchy of KE, E, N (80-bit), the
    float64 oracle's, and the device's METHOD restated in numpy on the oracle's coarse matrix: L = Cholesky, W = L^-1 by
    triangular solves, x = W^T (W b).  norm: the CdNorm of the arbiter's matrix."""

    def __init__(self, orc, arb, mesh, nlv, KE, E, N):
        import scipy.linalg as sla
        ex, ey, ez = mesh
        L = lambda a: np.ascontiguousarray(a, dtype=np.longdouble)
        self.mg, self.amg = orc.MG(ex + 1, ey + 1, ez + 1, 3, nlv, 2, 20), arb.MG(ex + 1, ey + 1, ez + 1, 3, nlv, 2, 20)
        for m, f in ((self.mg, orc.f64), (self.amg, L)):
            m.set_coarse_direct(True)
            m.assemble(f(KE), f(E), f(N))
        self.lc = nlv - 1
        self.norm = CdNorm(self.amg, self.lc)
        self.A = self.mg.csr(self.lc)
        A = self.A.toarray()
        self.W = sla.solve_triangular(np.linalg.cholesky(A), np.eye(A.shape[0]), lower=True)

    def solves(self, b):
        """-> (x_a, x_oracle, x_numpy_W)"""
        return self.amg.coarse_solve(np.ascontiguousarray(b, dtype=np.longdouble)), self.mg.coarse_solve(b), self.W.T @ (self.W @ b)

    def dist(self, v, xa):
        return self.norm.dist(v, xa)

    def residual(self, b, x):
        """max|A x - b| / max|b| in float64 with the oracle's coarsest matrix"""
        return float(np.abs(self.A @ x - b).max() / np.abs(b).max())
