"""Row-wise error bounds for the response kernels -- stress (stress.h), stress stiffness (geomstiff.h), mass (mass.h), body force
(bodyforce.h) and the fused multi-case response (response.h) -- on 0/1 designs.  A plain helper module: no fixtures, no hooks.
The cases, the row scales and the constants of tests/test_response_rowwise_oracle.py (CPU) and
tests/test_gpu_response_rowwise.py; the assertion, the designs and the reasons are those of tests/rowwise.py.

Every row i of every kernel is held to  |got_i - ref_i| <= c eps scale_i,  eps = 2^-53, `ref` the 80-bit restatement of
tests/eigen_ref.py, tests/buckling_ref.py, tests/selfweight_ref.py, tests/stress_ref.py (dfdx: oracle/arbiter.py).

THE ROW SCALE, one rule for every kernel: scale_i is the restatement of the same quantity with every table entry, coefficient,
weight and field replaced by its absolute value and every difference a - b inside it (u_a - u_0 of the stress form, psi_b - psi_a
of the stress stiffness) by |a| + |b|, evaluated in float64.  The kernels that add to their output get |pre_i| added.  Rows of
scale 0 must match bit for bit (void-only nodes on the exact-zero design, the clamped dofs of MassMult / GeomMult): that is
rowwise.assert_rowwise.  No row is left out.

Under a square root and a power (stress) the rule needs one more step, because the relative error of s_e = u_e^T M u_e is
unbounded under cancellation: with A_e = |d_e|^T |M| |d_e|, |d_a| = |u_a| + |u_0|, the device's s_e lies in
I_e = [max(s_ref - C_S eps A_e, 0), s_ref + C_S eps A_e]; vm_e, dpdx_e and the adjoint weight c_e are held to the image of I_e
under their formula (monotone in s, pnorm from the reference), widened by the formula's own roundings relative to the value
(C_VM, C_POW); pnorm to the image under the sum and the P-th root.  s_ref == 0 exactly (elements in rigid translation): exactly 0.
adj_rhs: scale_i = sum_e c_e (|M| |d_e|)[rows of the node's corner]; the half-width of c_e times |M d_e| is added to the
allowance, so that a row is not charged for the weight's own permitted error.

THE CONSTANTS: the rule of tests/rowwise.py -- the larger of the count of rounded operations in the form's longest chain (read
off the kernel) and 16 x what the float64 restatement measures against the 80-bit one on the CPU
(tests/test_response_rowwise_oracle.py holds it to a QUARTER of each), rounded up to a power of two.  Never from what the HIP
kernels achieve.  "Measured": the largest figure over every mesh, design and field below.
"""
import numpy as np

from tests import buckling_ref as bref
from tests import eigen_ref as eref
from tests import rowwise as rw
from tests import selfweight_ref as sref
from tests import stress_ref as stref

EPS, LD = rw.EPS, np.longdouble

# ---- mass_apply_node: 27 fma, the 8-term coefficient sum, the pair weight (1), the two N products (2), and the coefficient
# rho0 V m(x) itself (the polynomial's 6 + 2 products): 46.  Measured: 3.68 (x 16 = 59).
C_MASS = 64
# mass_sens_elem: N v (1), the 8-term row of M8 (8), the 24-term quadratic form (24), the sum over <= 8 fields (8), the prefactor
# scale rho0 V m'(x) (the polynomial's 6 + 3 products) and the addition to out (1): 51.  Measured: 10.04 (x 16 = 161): the
# measured value sets it.
C_MASS_SENS = 256
# geom_coef_elem, the longest chain of one entry: the <= 24-term geom_sigma (24), the two 3-term products S gradN_b and
# gradN_a . (3 + 3), the accumulation over the 8 Gauss points (8), Emax x^p wq (pow + 2 products) and its product (4): 42.
# geom_apply_node on top of it: the 8-term weight sum (8), psi_b - psi_a with its two N products (3), 26 fma (26), N on the
# left (1): 80.  Measured: 0.77 (x 16 = 13).
C_GEOM = 128
# geom_sens_elem: geom_sigma (24), geom_grad (8), geom_voigt (3 + the doubling, exact), the 48-term sum over Gauss points and
# rows (48), the sum over <= 8 fields (8), the prefactor scale p x^(p-1) Emax wq (pow + 4 products: 5), the addition (1): 97.
# Measured: 1.58 (x 16 = 26).
C_GEOM_SENS = 128
# geom_adjoint_node: N phi (1), geom_grad (8), geom_voigt (3), the weighted sum over <= 8 fields (8), the 48-term contraction
# with C0 B (48), Emax x^p wq (pow + 2 products + 1: 4), the 8-element sum (8), scale (1): 81.  Measured: 2.16 (x 16 = 35).
C_GEOM_ADJ = 128
# k_body_load: the 8-term sum of m(x_e) (8), each term the polynomial's 6 roundings (6), the product with (V / 8) b (1), the
# base (1): 16.  Measured: 6.17 (x 16 = 99; the eight terms of a void-only node carry the SAME rounding of m(1e-3), which does
# not average out): the measured value sets it.
C_BODY = 128
# k_body_sens: (V / 8) b N (2), the 24-term dot product (24), the sum over <= 8 fields (8), scale m'(x) (the polynomial's 6 + 1),
# the product and the addition (2): 43.  Measured: 2.48 (x 16 = 40).
C_BODY_SENS = 64
# k_stress_elem: d_a = u_a - u_0 (1), 21 x 21 fma (441), the clamp (exact): 442.  Measured: 1.13 (x 16 = 19).
C_S = 512
# vm = Emax pow(x, q) sqrt(s): pow (not correctly rounded: 2), product, sqrt, product: 5.  Measured, as the used fraction of the
# widened image of I_e times the constant (an upper figure): 0.11 (x 16 = 2).
C_VM = 8
# k_stress_coef, for P <= 8: the argument a sqrt(s) / pnorm carries 5 roundings (pow, product, sqrt, product, division) and
# pnorm's own <= 8 eps (c_pnorm's 32 on the sum, the P-th root of it: 32 / P + 1 <= 8 for P >= 5; P = 2: the argument's power
# is 0 or 2), which pow(., P - 2) or pow(., P) multiplies by up to P = 8: 104; pow's own rounding and the three products
# around it (4): 108.  Measured (an upper figure, as for C_VM): 0.41 (x 16 = 7).
C_POW = 128
# k_stress_adjoint_rhs: d_a = u_a - u_0 (1), the 21-term row of M (21), 8 fma with c_e (8): 30.  Measured: 1.09 (x 16 = 18).
C_ADJ = 32
# k_response: C_DFDX's count (53) + the sum over <= 8 cases (8): 61; measured (float64 oracle's compliance_sens summed per case
# against the arbiter's): 2.16 (x 16 = 35).
C_RESPONSE = 64


def c_pnorm(nwg):
    """pnorm relative to itself (a sum of positive terms): pow(vm, P) (1), rowwise.dot_chain's workgroup sum and tail over
    nwg partials (20 + ceil(nwg / 256)), the P-th root (pow: 1), its argument 1 / P (1): such a bound holds for any float64
    summation of that depth -- no oracle figure, like rowwise.c_dot"""
    return rw.pow2(rw.dot_chain(0, nwg) + 3)


# =====================================================================================================================
# cases
# =====================================================================================================================
assert eref.KERNEL_MESHES == bref.KERNEL_MESHES
# (elements, h): the four kernel meshes of eigen_ref / buckling_ref (the last: hx != hy != hz); 33 x 17 x 9: more than 256
# elements along no axis, 6120 nodes (no multiple of 256), the block faces of rowwise.design on its planes
MESHES = list(eref.KERNEL_MESHES) + [((33, 17, 9), (0.06, 0.05, 0.04))]
# 69120 elements = 270 workgroups of 256: the second trip of the one-workgroup reduction tails
REDUCTION_MESH = ((48, 40, 36), (0.025, 0.03, 0.035))
REDUCTION_DESIGNS = ("checker", "one_solid")
DESIGNS = rw.GENERATORS + ("blocks0",)      # blocks0: "blocks" with EXACT zeros in place of XMIN
X_LOWS = (0.1, 0.0)
RHO0, EMAX, PENAL, NU = 2.5, 2.5, 3.0, 0.3    # (not 1, so that a dropped factor shows)
EMIN_R, EMAX_R = 1e-9, 1.0                    # the multi-case response: the moduli of tests/rowwise.py
BVEC = (0.3, -0.7, 1.1)
WEIGHTS = [0.75, -0.5, 0.0]
CASE_WEIGHTS = [0.5, -1.0, 2.0, 0.0, 1.5, 0.25, 3.0, 1.0]
QP = [(0.5, 8.0), (0.5, 2.0), (0.0, 2.0), (0.125, 8.0)]      # the last: q P = 1, x^(qP-1) = 1 at x = 0
PLANT = 1e-3


def design(kind, ne):
    if kind == "blocks0":
        return np.where(rw.design("blocks", *ne) == 1.0, 1.0, 0.0)
    return rw.design(kind, *ne)


def nnodes(ne):
    return (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)


def fields(ne, seed, count=3):
    """uniform(-1, 1) nodal fields; they do NOT vanish on the supports"""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, 3 * nnodes(ne)) for _ in range(count)]


def translation_field(ne, seed):
    """a rigid translation of size 1 plus a perturbation of relative size 1e-6 -- u_e^T M u_e cancels six digits -- and NO
    perturbation on the two lowest node planes: the element layer 0 is in rigid translation, s_e = 0 exactly"""
    nz, ny, nx = ne[2] + 1, ne[1] + 1, ne[0] + 1
    U = np.tile(np.array([0.3, -0.7, 0.64]), nx * ny * nz).reshape(nz, ny, nx, 3)
    p = 1e-6 * np.random.default_rng(seed).uniform(-1.0, 1.0, U.shape)
    p[:2] = 0.0
    return (U + p).reshape(-1)


def stress_states(ne, seed):
    return {"random": fields(ne, seed, 1)[0], "translation": translation_field(ne, seed + 1)}


def _assemble(dofs, fe, n, N=None):
    y = np.zeros(n)
    np.add.at(y, dofs, fe)
    return y if N is None else np.asarray(N, dtype=np.float64) * y


# =====================================================================================================================
# row scales (float64)
# =====================================================================================================================
def scale_mass_apply(x, dofs, nnode, h, rho0, x_low, N, u):
    """every entry of M8 and every coefficient rho0 V m(x) is positive: the restatement on |u|"""
    return eref.mass_apply(x, dofs, nnode, h, rho0, x_low, N, np.abs(u), np.float64)


def scale_mass_sens(x, dofs, h, rho0, x_low, N, V, w, scale, pre=None):
    s = eref.mass_sens(x, dofs, h, rho0, x_low, N, [np.abs(v) for v in V], np.abs(w), abs(scale), np.float64)
    return s if pre is None else s + np.abs(pre)


class GeomAbs:
    """the tables of buckling_ref.tables with every entry replaced by its absolute value, and the forms built from them"""

    def __init__(self, h, nu=NU):
        gn, cb, _, wq = bref.tables(h, nu, np.float64)
        self.gn, self.cb, self.wq = np.abs(gn), np.abs(cb), float(wq)

    def ghat(self, ue):
        """|g_e| [nel, 8, 8]: sum_gp wq |gradN_a|^T |S| |gradN_b|, |S| from |C0 B| |u_e|"""
        S = bref.stress_tensor(np.einsum("qrj,ej->eqr", self.cb, np.abs(ue)))
        return self.wq * np.einsum("qia,eqij,qjb->eab", self.gn, S, self.gn)

    def apply(self, x, dofs, nnode, Emax, penal, N, U, phi):
        """N_i sum_e Es sum_{b != a} |g_e|[a, b] (|psi_b| + |psi_a|), psi = N phi"""
        g = self.ghat(np.asarray(U, dtype=np.float64)[dofs])
        g[:, np.arange(8), np.arange(8)] = 0.0
        pe = np.abs(np.asarray(N, dtype=np.float64) * phi)[dofs].reshape(-1, 8, 3)
        fe = np.einsum("eab,ebk->eak", g, pe) + g.sum(axis=2)[:, :, None] * pe
        Es = Emax * np.asarray(x, dtype=np.float64) ** penal
        return _assemble(dofs, (Es[:, None, None] * fe).reshape(-1, 24), 3 * nnode, N)

    def sens(self, x, dofs, Emax, penal, N, U, Phi, w, scale, pre=None):
        g = self.ghat(np.asarray(U, dtype=np.float64)[dofs])
        acc = np.zeros(dofs.shape[0])
        for wl, phi in zip(w, Phi):
            pe = np.abs(np.asarray(N, dtype=np.float64) * phi)[dofs].reshape(-1, 8, 3)
            acc += abs(wl) * np.einsum("eak,eab,ebk->e", pe, g, pe)
        x = np.asarray(x, dtype=np.float64)
        s = abs(scale) * penal * x ** (penal - 1) * Emax * acc
        return s if pre is None else s + np.abs(pre)

    def adjoint_rhs(self, x, dofs, nnode, Emax, penal, N, Phi, w, scale):
        sv = np.zeros((dofs.shape[0], 8, 6))
        for wl, phi in zip(w, Phi):
            pe = np.abs(np.asarray(N, dtype=np.float64) * phi)[dofs].reshape(-1, 8, 3)
            H = np.einsum("qdb,ebk->eqkd", self.gn, pe)
            s = np.einsum("eqki,eqkj->eqij", H, H)
            sv += abs(wl) * np.stack([s[..., 0, 0], s[..., 1, 1], s[..., 2, 2], 2 * s[..., 0, 1], 2 * s[..., 1, 2], 2 * s[..., 0, 2]], axis=-1)
        Es = Emax * np.asarray(x, dtype=np.float64) ** penal
        re = (Es * self.wq)[:, None] * np.einsum("qrj,eqr->ej", self.cb, sv)
        return abs(scale) * _assemble(dofs, re, 3 * nnode)


def body_load64(x, dofs, nnode, h, b, x_low):
    """the float64 restatement of selfweight_ref.load (which is 80-bit): m by eigen_ref's float64 form"""
    per = eref.mass64(x, x_low) * (np.float64(h[0]) * np.float64(h[1]) * np.float64(h[2]) / 8.0)
    return _assemble(dofs, per[:, None] * np.tile(np.asarray(b, dtype=np.float64), 8)[None, :], 3 * nnode)


def scale_body_load(x, dofs, nnode, h, b, x_low, base=None):
    s = body_load64(x, dofs, nnode, h, np.abs(b), x_low)
    return s if base is None else s + np.abs(base)


def body_sens(x, dofs, h, b, x_low, N, V, w, scale):
    """scale sum_l w_l d(v_l^T N f)/dx_e: selfweight_ref.sens_term weighted, 80-bit"""
    acc = np.zeros(dofs.shape[0], dtype=LD)
    for wl, v in zip(w, V):
        acc = acc + LD(wl) * sref.sens_term(x, dofs, h, b, x_low, N, v)
    return LD(scale) * acc


def body_sens64(x, dofs, h, b, x_low, N, V, w, scale):
    """the float64 restatement of the same (selfweight_ref is 80-bit): m' by eigen_ref's float64 form"""
    bN = np.tile(np.asarray(b, dtype=np.float64), 8)[None, :] * np.asarray(N, dtype=np.float64)[dofs]
    acc = np.zeros(dofs.shape[0])
    for wl, v in zip(w, V):
        acc = acc + wl * (bN * np.asarray(v, dtype=np.float64)[dofs]).sum(axis=1)
    return (scale * (eref.dmass64(x, x_low) * (np.float64(h[0]) * np.float64(h[1]) * np.float64(h[2]) / 8.0))) * acc


def scale_body_sens(x, dofs, h, b, x_low, N, V, w, scale, pre=None):
    s = body_sens64(x, dofs, h, np.abs(b), x_low, N, [np.abs(v) for v in V], np.abs(w), abs(scale))
    return s if pre is None else s + np.abs(pre)


def scale_response(nx, ny, nz, KE, Us, Vs, w, x, Emin=EMIN_R, Emax=EMAX_R, penal=PENAL):
    """rowwise.scale_dfdx summed with |w_l|; a bilinear case (V_l given): ||v_e||_1 ||u_e||_1 in place of ||u_e||_1^2"""
    x = np.asarray(x, dtype=np.float64)
    pre = penal * x ** (penal - 1) * (Emax - Emin) * float(np.abs(KE).max())
    s = np.zeros(x.size)
    for wl, u, v in zip(w, Us, Vs):
        if v is None:
            s += abs(wl) * rw.scale_dfdx(nx, ny, nz, KE, u, x, Emin, Emax, penal)
        else:
            s += abs(wl) * pre * rw.elem_u1(nx, ny, nz, u) * rw.elem_u1(nx, ny, nz, v)
    return s


# =====================================================================================================================
# stress: intervals
# =====================================================================================================================
def stress_bounds(M, dofs, U, x, q, P, Emax=EMAX, nwg=1, div=1):
    """-> dict: ref (stress_ref, 80-bit, corner-relative), A, and (lo, hi) pairs for s, vm, dpdx, pnorm; c (the adjoint weight,
    reference) with its half-width; adj_scale, the row scale of adj_rhs with the weights' half-width folded in for C_ADJ.
    div: every constant is divided by it (the oracle test: 4).

    HOW MUCH THIS HOLDS depends on the state.  On the random state A_e is of the size of s_e and I_e is 1e-13 of it wide: vm,
    dpdx and every row of adj_rhs are held to 13 digits.  On the translation-plus-perturbation state |d_a| = |u_a| + |u_0| is
    about 2 while s_e is about 1e-12 |M|, so C_S eps A_e is TENS OF PERCENT of s_e, and with P = 8 the half-width of the weight
    c_e is of the order of c_e itself: there vm, dpdx and adj_rhs are held loosely -- a dropped element would pass -- and the
    small fractions of the interval that the kernels use on that state say little.  What that state does hold: finite values
    everywhere, the corner-relative form's result inside the interval that the formula's own cancellation allows, and exact
    zeros where s_ref == 0.  The rows themselves are held by the random state."""
    r = stref.stress_ref(M, dofs, U, x, q, P, Emax, LD, relative=True)
    M64 = np.asarray(M, dtype=np.float64)
    au = np.abs(np.asarray(U, dtype=np.float64))[dofs]
    d = au + np.tile(au[:, :3], (1, 8))
    d[:, :3] = 0.0
    Md = d @ np.abs(M64)
    A = np.einsum("er,er->e", d, Md)
    s, pn = r["s"], r["pnorm"]
    e = lambda c: LD(c * EPS / div)
    wd = e(C_S) * A.astype(LD)
    rigid = s == 0
    s_lo, s_hi = np.where(rigid, 0, np.maximum(s - wd, 0)), np.where(rigid, 0, s + wd)
    xe, qq, PP = np.asarray(x).astype(LD), LD(q), LD(P)
    a = LD(Emax) * xe ** qq
    vm_lo, vm_hi = a * np.sqrt(s_lo) * (1 - e(C_VM)), a * np.sqrt(s_hi) * (1 + e(C_VM))
    cp = c_pnorm(nwg)
    root = lambda v: (v ** PP).sum() ** (1 / PP)
    out = dict(ref=r, A=A, rigid=rigid, c_adj=C_ADJ / div, s=(s_lo, s_hi), vm=(vm_lo, vm_hi), pnorm=(root(vm_lo) * (1 - e(cp)), root(vm_hi) * (1 + e(cp))))
    n = r["adj"].size
    if pn == 0:
        z = np.zeros(len(xe), dtype=LD)
        out.update(dpdx=(z, z), c=z, c_half=z, adj_scale=np.zeros(n))
        return out
    if q != 0:
        dp = lambda sv: qq * pn * xe ** (qq * PP - 1) * (LD(Emax) * np.sqrt(sv) / pn) ** PP
        out["dpdx"] = (dp(s_lo) * (1 - e(C_POW)), dp(s_hi) * (1 + e(C_POW)))
    else:
        out["dpdx"] = (np.zeros(len(xe), dtype=LD),) * 2
    with np.errstate(divide="ignore", invalid="ignore"):
        cf = lambda sv: np.where(sv > 0, pn ** (1 - PP) * a ** PP * sv ** ((PP - 2) / 2), 0)
        c, c_lo, c_hi = cf(s), cf(s_lo) * (1 - e(C_POW)), cf(s_hi) * (1 + e(C_POW))
    half = np.maximum(c_hi - c, c - c_lo)
    ue = np.asarray(U).astype(LD)[dofs]
    ue = ue - np.tile(ue[:, :3], (1, 8))
    aMu = np.abs(ue @ np.asarray(M).astype(LD)).astype(np.float64)
    c64, h64 = c.astype(np.float64), half.astype(np.float64)
    out.update(c=c, c_half=half,
               adj_scale=_assemble(dofs, c64[:, None] * Md, n) + _assemble(dofs, h64[:, None] * aMu, n) / (C_ADJ * EPS / div))
    return out


def assert_interval(got, lo, hi, ref, where):
    """fails if got_i lies outside [lo_i, hi_i] for ANY row (lo == hi: bit for bit) -> the largest fraction of the way from
    ref to the interval's end that a row has gone (<= 1)"""
    g = np.atleast_1d(np.asarray(got)).astype(LD)
    lo, hi, ref = (np.atleast_1d(np.asarray(v, dtype=LD)) for v in (lo, hi, ref))
    assert g.shape == lo.shape == hi.shape == ref.shape and np.isfinite(g.astype(np.float64)).all(), where.get("label")
    assert (lo <= ref).all() and (ref <= hi).all(), where.get("label")
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(g >= ref, (g - ref) / (hi - ref), (ref - g) / (ref - lo))
    frac = np.where(g == ref, 0, frac).astype(np.float64)            # (0 / 0 where the interval is a point and hit)
    bad = (g < lo) | (g > hi)
    if bad.any():
        row = int(np.flatnonzero(bad)[np.argmax(np.abs((g - ref)[bad]).astype(np.float64) / np.maximum((hi - lo)[bad].astype(np.float64), 1e-300))])
        raise AssertionError("%s: %d of %d rows outside their interval; worst: row %d, got %.17g, interval [%.17g, %.17g], reference %.17g "
                             "(|reference| / max = %.1e); %s" % (where.get("label"), int(bad.sum()), bad.size, row, float(g[row]), float(lo[row]),
                                                                float(hi[row]), float(ref[row]), float(abs(ref[row]) / max(np.abs(ref).max(), LD(1e-300))),
                                                                rw.describe(row, where) if "dims" in where else ""))
    return float(frac.max())


# =====================================================================================================================
# planted errors (tests/test_response_rowwise_oracle.py)
# =====================================================================================================================
def void_only_nodes(ne, x):
    """[3 nnode] True on the dofs of the nodes none of whose incident elements is solid"""
    dofs = sref.elem_dofs(*ne)
    solid = np.zeros(3 * nnodes(ne), dtype=bool)
    solid[dofs[np.asarray(x) == 1.0].ravel()] = True
    return ~solid


def plant(ref_ld, scale, candidates):
    """-> (the 80-bit result with ONE row multiplied by 1 + PLANT, the row): among `candidates` (bool) the row whose scale is
    smallest but positive and whose value is not zero"""
    ok = candidates & (scale > 0) & (np.asarray(ref_ld) != 0)
    assert ok.any()
    row = int(np.flatnonzero(ok)[np.argmin(scale[ok])])
    out = np.array(ref_ld, dtype=LD)
    out[row] = out[row] * (1 + LD(PLANT))
    return out, row


# =====================================================================================================================
# the cases: one generator per family -> dicts with the inputs of one kernel call, the 80-bit reference `ref`, the float64
# restatement `f64`, the row scale and the constant.  tests/test_response_rowwise_oracle.py holds f64 to a quarter of the
# bound, tests/test_gpu_response_rowwise.py runs the call on the device.
# =====================================================================================================================
def _mesh(mesh):
    ne, h = mesh
    return ne, h, sref.elem_dofs(*ne), nnodes(ne), eref.cantilever_N(*ne)


def _pre(scale_term, seed):
    """what the adding kernels find in their output: of the size of the ROW's own term (a value of the size of the largest
    row would bury the void rows' terms under its rounding), 0 where the term's scale is 0"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, scale_term.size) * scale_term


def mass_cases(mesh, kind, x_low, seed=900):
    ne, h, dofs, nn, N = _mesh(mesh)
    x, V = design(kind, ne), fields(ne, seed)
    tag = "mass %s %s x_low %g" % ("x".join(map(str, ne)), kind, x_low)
    node, elem = {"dims": tuple(n + 1 for n in ne)}, {"dims": ne, "dof": 0}
    for l in (0, 1):
        a = (x, dofs, nn, h, RHO0, x_low, N, V[l])
        yield dict(op="apply", x=x, u=V[l], ref=eref.mass_apply(*a, LD), f64=eref.mass_apply(*a, np.float64), scale=scale_mass_apply(*a),
                   c=C_MASS, where=dict(node, label="%s MassMult field %d" % (tag, l)))
    for Vs, w, sc in ((V, WEIGHTS, -2.0), (V[:1], None, 1.0)):
        wv = [1.0] * len(Vs) if w is None else w
        a = (x, dofs, h, RHO0, x_low, N, Vs, wv, sc)
        pre = _pre(scale_mass_sens(*a), seed + 7) if w is not None else np.zeros(x.size)
        yield dict(op="sens", x=x, V=Vs, w=w, sc=sc, pre=pre, ref=pre.astype(LD) + eref.mass_sens(*a, LD), f64=pre + eref.mass_sens(*a, np.float64),
                   scale=scale_mass_sens(*a, pre=pre), c=C_MASS_SENS, where=dict(elem, label="%s MassSensitivity %s" % (tag, "w=None" if w is None else "3 fields")))


def geom_cases(mesh, kind, seed=400):
    ne, h, dofs, nn, N = _mesh(mesh)
    x, V = design(kind, ne), fields(ne, seed)
    ga = GeomAbs(h)
    node, elem = {"dims": tuple(n + 1 for n in ne)}, {"dims": ne, "dof": 0}
    base = "geom %s %s" % ("x".join(map(str, ne)), kind)
    for sname, U in (("random", fields(ne, seed + 50, 1)[0]), ("smooth", bref.smooth_field(ne, seed + 60))):
        tag = "%s state %s" % (base, sname)
        for l in (0, 1):
            a = (x, dofs, nn, h, NU, EMAX, PENAL, N, U, V[l])
            yield dict(op="apply", x=x, U=U, u=V[l], ref=bref.geom_apply(*a, LD), f64=bref.geom_apply(*a, np.float64),
                       scale=ga.apply(x, dofs, nn, EMAX, PENAL, N, U, V[l]), c=C_GEOM, where=dict(node, label="%s GeomMult field %d" % (tag, l)))
        for Vs, w, sc in ((V, WEIGHTS, -2.0), (V[:1], None, 1.0)):
            wv = [1.0] * len(Vs) if w is None else w
            a = (x, dofs, h, NU, EMAX, PENAL, N, U, Vs, wv, sc)
            st = ga.sens(x, dofs, EMAX, PENAL, N, U, Vs, wv, sc)
            pre = _pre(st, seed + 7) if w is not None else np.zeros(x.size)
            yield dict(op="sens", x=x, U=U, V=Vs, w=w, sc=sc, pre=pre, ref=pre.astype(LD) + bref.geom_sens(*a, LD), f64=pre + bref.geom_sens(*a, np.float64),
                       scale=st + np.abs(pre), c=C_GEOM_SENS, where=dict(elem, label="%s GeomSensitivity %s" % (tag, "w=None" if w is None else "3 fields")))
    for Vs, w in ((V[:1], None), (V, WEIGHTS)):
        wv = [1.0] * len(Vs) if w is None else w
        a = (x, dofs, nn, h, NU, EMAX, PENAL, N, Vs, wv, -2.0)
        yield dict(op="adjoint", x=x, V=Vs, w=w, sc=-2.0, ref=bref.geom_adjoint_rhs(*a, LD), f64=bref.geom_adjoint_rhs(*a, np.float64),
                   scale=ga.adjoint_rhs(x, dofs, nn, EMAX, PENAL, N, Vs, wv, -2.0), c=C_GEOM_ADJ,
                   where=dict(node, label="%s GeomAdjointRHS %d field(s)" % (base, len(Vs))))


def body_cases(mesh, kind, x_low, seed=700):
    ne, h, dofs, nn, N = _mesh(mesh)
    x, V = design(kind, ne), fields(ne, seed)
    tag = "body %s %s x_low %g" % ("x".join(map(str, ne)), kind, x_low)
    node, elem = {"dims": tuple(n + 1 for n in ne)}, {"dims": ne, "dof": 0}
    fr, f64, s0 = sref.load(x, dofs, nn, h, BVEC, x_low), body_load64(x, dofs, nn, h, BVEC, x_low), scale_body_load(x, dofs, nn, h, BVEC, x_low)
    yield dict(op="load", x=x, base=None, ref=fr, f64=f64, scale=s0, c=C_BODY, where=dict(node, label="%s BodyLoad" % tag))
    base = _pre(s0, seed + 3)
    yield dict(op="load", x=x, base=base, ref=base.astype(LD) + fr, f64=base + f64, scale=s0 + np.abs(base), c=C_BODY,
               where=dict(node, label="%s BodyLoad with a base (and in place)" % tag))
    for Vs, w, sc in ((V[:1], None, 1.0), (V, WEIGHTS, 2.0)):
        wv = [1.0] * len(Vs) if w is None else w
        a = (x, dofs, h, BVEC, x_low, N, Vs, wv, sc)
        st = scale_body_sens(*a)
        pre = _pre(st, seed + 7) if w is not None else np.zeros(x.size)
        yield dict(op="sens", x=x, V=Vs, w=w, sc=sc, pre=pre, ref=pre.astype(LD) + body_sens(*a), f64=pre + body_sens64(*a), scale=st + np.abs(pre),
                   c=C_BODY_SENS, where=dict(elem, label="%s BodySensitivity %d field(s)" % (tag, len(Vs))))


def stress_cases(mesh, kind, nwg=1, div=1, seed=300, qps=QP, states=None):
    """-> dicts: the state, (q, P) and stress_bounds of them (div: see there)"""
    ne, h, dofs, nn, _ = _mesh(mesh)
    x, M = design(kind, ne), stref.vonmises_form(h)
    for sname, U in (states or stress_states(ne, seed)).items():
        for q, P in qps:
            yield dict(x=x, U=U, q=q, P=P, M=M, dofs=dofs, b=stress_bounds(M, dofs, U, x, q, P, EMAX, nwg, div), ne=ne,
                       label="stress %s %s state %s q=%g P=%g" % ("x".join(map(str, ne)), kind, sname, q, P))


def check_stress(c, vm, pnorm, vm_max, dpdx, adj):
    """the five outputs of one Stress call (device, or the float64 restatement) against the bounds of a stress case -> achieved
    figures {name: fraction of the interval used / achieved c}"""
    b, ne, lab = c["b"], c["ne"], c["label"]
    r = b["ref"]
    elem, node = {"dims": ne, "dof": 0}, {"dims": tuple(n + 1 for n in ne)}
    out = {"vm": assert_interval(vm, *b["vm"], r["vm"], dict(elem, label=lab + " vm")),
           "dpdx": assert_interval(dpdx, *b["dpdx"], r["dpdx"], dict(elem, label=lab + " dpdx")),
           "pnorm": assert_interval(pnorm, *b["pnorm"], r["pnorm"], {"label": lab + " pnorm"})}
    if vm_max is not None:
        assert vm_max == np.max(vm), (lab, vm_max, np.max(vm))
    for name, a in (("vm", vm), ("dpdx", dpdx)):
        assert not np.asarray(a)[b["rigid"]].any(), "%s: %s is not exactly 0 where s_e = 0" % (lab, name)
    out["adj"] = rw.assert_rowwise(np.asarray(adj, dtype=np.float64), r["adj"], b["adj_scale"], b["c_adj"], dict(node, label=lab + " adj_rhs"))
    return out


def response_ref(arb, KE, ne, Us, Vs, w, x):
    """dfdx of the weighted response in 80-bit arithmetic: the quadratic cases by arbiter.compliance_sens, the bilinear ones
    (V_l given) by -p x^(p-1) (Emax - Emin) v_e^T KE u_e"""
    nx, ny, nz = (n + 1 for n in ne)
    L = lambda a: np.ascontiguousarray(a, dtype=LD)
    dofs = sref.elem_dofs(*ne)
    out = np.zeros(x.size, dtype=LD)
    for wl, u, v in zip(w, Us, Vs):
        if v is None:
            df = arb.compliance_sens(nx, ny, nz, L(KE), L(u), L(x), EMIN_R, EMAX_R, PENAL, 0.12)[2]
        else:
            df = -LD(PENAL) * L(x) ** (LD(PENAL) - 1) * (LD(EMAX_R) - LD(EMIN_R)) * sref.uKu(KE, dofs, u, v)
        out = out + LD(wl) * np.asarray(df, dtype=LD)
    return out


def response_f64(orc, KE, ne, Us, Vs, w, x):
    nx, ny, nz = (n + 1 for n in ne)
    dofs = sref.elem_dofs(*ne)
    K = np.asarray(KE, dtype=np.float64).reshape(24, 24)
    out = np.zeros(x.size)
    for wl, u, v in zip(w, Us, Vs):
        if v is None:
            df = orc.compliance_sens(nx, ny, nz, KE, u, x, EMIN_R, EMAX_R, PENAL, 0.12)[2]
        else:
            df = -PENAL * x ** (PENAL - 1) * (EMAX_R - EMIN_R) * np.einsum("er,rc,ec->e", v[dofs], K, u[dofs])
        out = out + wl * df
    return out


def response_cases(mesh, kind, seed=100):
    """-> dicts: ncase states U, the second fields V (None: the quadratic form; one case of the bilinear calls keeps V_l = U_l),
    the weights and the row scale's ingredients; the reference needs KE: response_ref"""
    ne, h, _, _, _ = _mesh(mesh)
    x = design(kind, ne)
    Us, Vs = fields(ne, seed, 8), fields(ne, seed + 1, 8)
    for ncase in (1, 3, 8):
        for bilinear in (False, True):
            V = [None if (not bilinear or (l == 1 and ncase >= 3)) else Vs[l] for l in range(ncase)]
            yield dict(x=x, ne=ne, h=h, U=Us[:ncase], V=V, w=CASE_WEIGHTS[:ncase],
                       where={"dims": ne, "dof": 0, "label": "response %s %s %d case(s) %s" % ("x".join(map(str, ne)), kind, ncase, "bilinear" if bilinear else "quadratic")})
