"""Every operator kernel form held to a ROW-WISE error bound on 0/1 designs, against the 80-bit arbiter (tests/rowwise.py:
why, the row scales, the generators, the constants and the operation counts behind them).

The library latches its switches once per process: one subprocess per form (tests/rowwise_worker.py), which runs all meshes,
both boundary conditions (cantilever: unmasked tiles; scattered Dirichlet dofs: masked tiles) and the five 0/1 generators,
ASSERTS that the forced form is the one that launched (LinearElasticity.last_op_form: generation, tile shape, z-chunk;
stencil split, node / row form, mirrored reads) and dumps inputs and outputs; this file compares.  References: the arbiter on
the matrix the kernels apply (KE_effective for apply and the Chebyshev step, KE_krylov for apply_krylov, both as the library
exports them, hi + lo); the Chebyshev step formed in 80-bit arithmetic from the device's own dinv and window.  Three more
test functions share a second worker run per form (modes fine_steps / coarse_steps): steps 2 and 3 of a sweep (20 on the
coarsest level), the residual epilogue through LinearElasticity.level_residual, and the VALUES of the fused dot products
(MatMultKrylovDot, smooth_dot) -- ownership of the seam nodes and the summation, on the seeded field and on a field of void
rows only.

Bounds (c, in units of eps x row scale) and the worst c the kernels ACHIEVED on the MI355X (recorded for the reader; the
bounds come from the operation counts and the oracle's own CPU figures in tests/rowwise.py, not from these):

    form                                              bound   achieved
    fine gen 1 / 2 / 3 16x16 / 3 32x8 / 32x8 kz 3 / auto (identical bits from generation 2 on)
        apply, apply_krylov                             64    0.92, 0.93
        Jacobi diagonal (relative to the entry)          64    8.4
        Chebyshev step, zero / non-zero guess           128    2.4 / 8.7
    fine per-node kernel (TP_NO_TILE)
        apply, apply_krylov / diagonal / steps    64 / 64 / 128    1.1 / 5.8 / 2.4, 3.7
    level 1 from the fine densities (fused and unfused correction, TP_MACRO_KZ=3)
        apply / diagonal / steps                 256 / 256 / 256    7.8 / 26.6 / 2.5, 4.3
    level 1 stored (TP_NO_MACRO), split 9 / 3 / 1
        apply / diagonal / steps                 256 / 256 / 256    8.1 .. 9.3 / 26.6 / 2.5, 3.5
    stored stencil, levels 2, 3: split 9; 3 node / row, mirrored / plain; 1
        apply                                     256, 512    4.6; 5.2; 6.0
        diagonal / steps                   256 / 256, 512    40.9 / 2.7, 3.8
    level 2's element matrices by the generic contraction (TP_NO_L2_FAST) / the fast one on 7 workgroups (TP_L2_BLOCKS=7)
        apply / diagonal / steps            256, 512 / 256 / 256, 512    4.6 / 34.3, 40.9 / 2.7, 3.1 and 2.6, 3.5
    later Chebyshev steps (step k from the device's own x_{k-1}, x_{k-2}; rw.STEP_MESHES on level 0, rw.COARSE_MESHES above), the
    residual epilogue b - A x, and the values of the fused dot products (against the 80-bit sum of the device's own vectors, in
    units of eps x sum |terms|; bound: the power of two above the chain 3 kz + 20 + ceil(workgroups / 256), rw.c_dot)
        fine gen 2 / 3 / auto: steps 2, 3 zero / non-zero   128    1.9 / 1.9   (gen 1: 1.9 / 2.0; per-node: 1.3 / 2.0;
                                                                                level 0 of the coarse meshes: 1.9 / 2.3)
        fine, every form: residual                           64    1.0         (per-node: 1.1)
        u . A u (EPI_APPLY_DOT), every fine form        32, 128    2.4         (32 x 8 tiles, kz 23: 2.1 of 128; per-node 1.7)
        b . x_out (EPI_CHEB_DOT), generations 2 and 3    32, 128    2.1
        level 1 from the fine densities: steps / residual   256    1.7, 1.5 / 5.5
        level 1 stored, split 9 / 3 / 1: steps / residual   256    1.4, 1.6 / 7.9, 6.8, 8.1
        stencil, levels 2, 3: steps 2, 3 / residual    256, 512    2.5, 2.5 / 7.7
        coarsest level, step 20 zero (one-launch run) / non-zero    512    1.0 / 1.6
    restrict / prolong_add (every level pair)       64 / 64    4.1 / 2.9
    dfdx on a converged state (rtol 1e-5)              128    2.2
    cone filter, Hs / forward / gradients, the same for the tiled, z-multi, wide, ring and generic kernels (the two designs with
    exact zeros, rw.FILTER_ZERO_KINDS, included: they leave the figures where they were)
        ElemConn 1                                       64    0.02 / 0.06 / 0.04
        ElemConn 2                                      256    0.24 / 0.35 / 0.17
        ElemConn 5                                     4096    0.92 / 1.7 / 0.61
        ElemConn 10                                   32768    5.9 / 16.4 / 1.4

The Chebyshev step's reference is formed in 80-bit arithmetic from the device's exported dinv and window; that dinv is itself
held row by row, relative to its own entry, against the arbiter's diagonal (the void rows included), so a Jacobi diagonal that
is wrong where the stiffness is small fails here.  The cone filter's scale carries a term for the rounding of its weights
R - dist (tests/rowwise.py: Cone, c_filter)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rowwise as rw

pytestmark = pytest.mark.gpu
FINE_MESHES, COARSE_MESHES = rw.FINE_MESHES, rw.COARSE_MESHES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("TP_FINE_V", "TP_FINE_SHAPE", "TP_TILE_KZ", "TP_NO_TILE", "TP_NO_MACRO", "TP_NO_CORR_FUSE", "TP_DIA_SPLIT", "TP_DIA_NODE",
            "TP_NO_DIA_SYM", "TP_MACRO_KZ", "TP_NO_L2_FAST", "TP_L2_BLOCKS")

# form -> (environment, expected last_op_form)
FINE_FORMS = {
    "gen1": ({"TP_FINE_V": "1"}, "1,1,0,*"),
    "gen2": ({"TP_FINE_V": "2"}, "1,2,0,*"),
    "gen3_16x16": ({"TP_FINE_V": "3", "TP_FINE_SHAPE": "1"}, "1,3,1,*"),
    "gen3_32x8": ({"TP_FINE_V": "3", "TP_FINE_SHAPE": "2"}, "1,3,2,*"),
    "gen3_32x8_kz3": ({"TP_FINE_V": "3", "TP_FINE_SHAPE": "2", "TP_TILE_KZ": "3"}, "1,3,2,<=3"),
    "auto": ({}, "1,*,*,*"),
    "per_node": ({"TP_NO_TILE": "1"}, "3,0,0,0"),
}
# form -> (environment, expected form of the levels >= 2, of level 1, dfdx too)
COARSE_FORMS = {
    "level1_from_fine_fused_corr": ({}, "4,*,*,*", "2,1,0,*", 1),
    "level1_from_fine_unfused_corr_kz3": ({"TP_NO_CORR_FUSE": "1", "TP_MACRO_KZ": "3"}, "4,*,*,*", "2,0,0,<=3", 0),
    "level1_stored": ({"TP_NO_MACRO": "1"}, "4,*,*,*", "4,*,*,*", 0),
    "stencil_split9": ({"TP_NO_MACRO": "1", "TP_DIA_SPLIT": "9"}, "4,9,0,0", "4,9,0,0", 0),
    "stencil_split3_node_mirrored": ({"TP_NO_MACRO": "1", "TP_DIA_SPLIT": "3"}, "4,3,1,1", "4,3,1,1", 0),
    "stencil_split3_node_plain": ({"TP_NO_MACRO": "1", "TP_DIA_SPLIT": "3", "TP_NO_DIA_SYM": "1"}, "4,3,1,0", "4,3,1,0", 0),
    "stencil_split3_row_mirrored": ({"TP_NO_MACRO": "1", "TP_DIA_SPLIT": "3", "TP_DIA_NODE": "0"}, "4,3,0,1", "4,3,0,1", 0),
    "stencil_split3_row_plain": ({"TP_NO_MACRO": "1", "TP_DIA_SPLIT": "3", "TP_DIA_NODE": "0", "TP_NO_DIA_SYM": "1"}, "4,3,0,0", "4,3,0,0", 0),
    "stencil_split1": ({"TP_NO_MACRO": "1", "TP_DIA_SPLIT": "1"}, "4,1,0,0", "4,1,0,0", 0),
    # level 2's Galerkin contraction in its other forms (elasticity_setup_from_E): every element through the generic
    # contraction, and the fast one as a grid stride of few workgroups -- the operators are the default job's
    "level2_generic_contraction": ({"TP_NO_L2_FAST": "1"}, "4,*,*,*", "2,1,0,*", 0),
    "level2_fast_contraction_7_workgroups": ({"TP_L2_BLOCKS": "7"}, "4,*,*,*", "2,1,0,*", 0),
}
L2_FORMS = {"level2_generic_contraction": False, "level2_fast_contraction_7_workgroups": True}    # form -> bit-equal to the default job
ACHIEVED = {}
_REF = {}


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def ld(a):
    return np.ascontiguousarray(a, dtype=np.longdouble)


def run_worker(tmp_path, mode, env, *args):
    out = str(tmp_path / "out.npz")
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rowwise_worker.py"), mode, args[0], out] + list(args[1:]), env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-3000:]
    return np.load(out)


def note(form, what, c, bound):
    k = (form, what)
    ACHIEVED[k] = (max(ACHIEVED.get(k, (0.0, bound))[0], c), bound)


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


@pytest.mark.parametrize("form", list(FINE_FORMS))
def test_fine_level_rowwise(tmp_path, orc, arb, form):
    env, expect = FINE_FORMS[form]
    d = run_worker(tmp_path, "fine", env, expect)
    for m, (ex, ey, ez) in enumerate(FINE_MESHES):
        nx, ny, nz = ex + 1, ey + 1, ez + 1
        for scattered in (0, 1):
            tag = "m%d_s%d" % (m, scattered)
            N, u, b, KE = d[tag + "_N"], d[tag + "_u"], d[tag + "_b"], d[tag + "_KE"]
            kf, kk = (d[tag + "_kf"], d[tag + "_kk"]) if form != "per_node" else (ld(KE), ld(KE))
            if form == "per_node":
                assert np.array_equal(d[tag + "_kf"], ld(KE))        # without the tile kernels the library applies KE itself
            free = N != 0
            for kind in rw.GENERATORS:
                t = "%s_%s" % (tag, kind)
                x, kz = d[t + "_x"], int(d[t + "_form"][3])
                E = orc.simp(x)
                key = (m, scattered, form == "per_node", x.tobytes())

                def refs():
                    s = rw.scale_fine(orc, nx, ny, nz, KE, E, u, N)
                    return (s, arb.matfree_apply(nx, ny, nz, 3, ld(kf), ld(E), ld(N), ld(u)),
                            arb.matfree_apply(nx, ny, nz, 3, ld(kk), ld(E), ld(N), ld(u)))
                s, ya, yk = cached(key, refs)
                w = {"dims": (nx, ny, nz), "kz": kz}
                lab = "%s mesh %s %s %s kz %d: " % (form, (ex, ey, ez), "scattered" if scattered else "cantilever", kind, kz)
                note(form, "apply", rw.assert_rowwise(d[t + "_apply"], ya, s * free, rw.C_FINE, dict(w, label=lab + "apply")), rw.C_FINE)
                note(form, "apply_krylov", rw.assert_rowwise(d[t + "_krylov"], yk, s * free, rw.C_FINE, dict(w, label=lab + "apply_krylov")), rw.C_FINE)
                dinv, lam = d[t + "_dinv"], float(d[t + "_lam"][0])
                # the Jacobi diagonal itself, row by row relative to its own entry (the step's reference below is formed from it)
                # (diagonal of N K N + I - N: the element matrix with its off-diagonal entries zeroed, applied to ones)
                kd = np.diag(np.diag(np.asarray(kf).reshape(24, 24))).reshape(-1)
                dg = cached(key + ("diag",), lambda: np.asarray(arb.matfree_apply(nx, ny, nz, 3, ld(kd), ld(E), ld(N), ld(np.ones_like(u)))))
                note(form, "dinv", rw.assert_rowwise(1.0 / dinv, dg, np.abs(dg.astype(np.float64)), rw.c_diag(0), dict(w, label=lab + "Jacobi diagonal")), rw.c_diag(0))
                theta = 0.5 * (1.1 * lam + 0.1 * lam)
                wc = dict(w, kz=int(d[t + "_formc"][3]))
                for name, x0, yx, sx in (("cheb0", np.zeros_like(u), 0, 0.0), ("cheb1", u, ya, s)):
                    xa = ld(x0) + ld(dinv) * (ld(b) - yx) / np.longdouble(theta)
                    sc = rw.scale_smooth(sx, dinv, 1.0 / theta, b, x0)
                    note(form, name, rw.assert_rowwise(d[t + "_" + name], xa, sc, rw.c_smooth(0), dict(wc, label=lab + "Chebyshev step " + name)), rw.c_smooth(0))
    print("ACHIEVED", form, {k[1]: "%.3g of %g" % v for k, v in ACHIEVED.items() if k[0] == form})


@pytest.mark.parametrize("form", list(COARSE_FORMS))
def test_coarse_levels_transfers_and_dfdx_rowwise(tmp_path, orc, arb, form):
    env, expect, lvl1, dfdx = COARSE_FORMS[form]
    d = run_worker(tmp_path, "coarse", env, expect, lvl1, str(dfdx))
    for m, ((ex, ey, ez), nlv) in enumerate(COARSE_MESHES):
        nx, ny, nz = ex + 1, ey + 1, ez + 1
        tag = "c%d" % m
        N, KE = d[tag + "_N"], d[tag + "_KE"]
        for kind in rw.GENERATORS:
            t = "%s_%s" % (tag, kind)
            x = d[t + "_x"]
            E = orc.simp(x)

            def hier():
                mg, amg = orc.MG(nx, ny, nz, 3, nlv), arb.MG(nx, ny, nz, 3, nlv)
                mg.assemble(KE, E, N)
                amg.assemble(ld(KE), ld(E), ld(N))
                return mg, amg
            xk = hash(x.tobytes())
            mg, amg = cached(("hier", m, kind, xk), hier)
            lab = "%s mesh %s %d levels %s: " % (form, (ex, ey, ez), nlv, kind)
            for l in range(nlv):
                dims = rw.level_dims(nx, ny, nz, l)
                u, b = d["%s_u%d" % (t, l)], d["%s_b%d" % (t, l)]
                if l > 0:
                    sl, ya = cached(("lvl", m, kind, xk, l), lambda: (rw.scale_level(orc, mg, l, (nx, ny, nz), KE, E, N, u), amg.apply(l, ld(u))))
                    f = tuple(int(v) for v in d["%s_form%d" % (t, l)])
                    w = {"dims": dims, "kz": f[3] if f[0] == 2 else 0}
                    name = "level1 " if l == 1 else "stencil "
                    note(form, name + "apply", rw.assert_rowwise(d["%s_apply%d" % (t, l)], ya, sl, rw.c_level(l), dict(w, label=lab + "level %d apply, form %s" % (l, f))),
                         rw.c_level(l))
                    dinv, (lam, lam_min) = d["%s_dinv%d" % (t, l)], d["%s_lam%d" % (t, l)]
                    dg = np.asarray(amg.diag(l))
                    note(form, name + "dinv", rw.assert_rowwise(1.0 / dinv, dg, np.abs(dg.astype(np.float64)), rw.c_diag(l),
                                                                dict(w, label=lab + "level %d Jacobi diagonal" % l)), rw.c_diag(l))
                    theta = 0.5 * (1.1 * lam + (lam_min if l == nlv - 1 else 0.1 * lam))
                    for nm, x0, yx, sx in (("cheb0", np.zeros_like(u), 0, 0.0), ("cheb1", u, ya, sl)):
                        xa = ld(x0) + ld(dinv) * (ld(b) - yx) / np.longdouble(theta)
                        sc = rw.scale_smooth(sx, dinv, 1.0 / theta, b, x0)
                        note(form, name + nm, rw.assert_rowwise(d["%s_%s_%d" % (t, nm, l)], xa, sc, rw.c_smooth(l),
                                                                dict(w, label=lab + "level %d Chebyshev step %s, form %s" % (l, nm, f))), rw.c_smooth(l))
                if l + 1 < nlv:
                    xc = d["%s_xc%d" % (t, l)]
                    note(form, "restrict", rw.assert_rowwise(d["%s_restrict%d" % (t, l)], amg.restrict(l, ld(u)), rw.scale_restrict(mg, l, u), rw.C_RESTRICT,
                                                             {"dims": rw.level_dims(nx, ny, nz, l + 1), "label": lab + "restrict %d -> %d" % (l, l + 1)}), rw.C_RESTRICT)
                    note(form, "prolong_add", rw.assert_rowwise(d["%s_prolong%d" % (t, l)], ld(b) + amg.prolong(l, ld(xc)), rw.scale_prolong_add(mg, l, xc, b),
                                                                rw.C_PROLONG, {"dims": dims, "label": lab + "prolong_add %d -> %d" % (l + 1, l)}), rw.C_PROLONG)
            if dfdx:
                U = d[t + "_U"]
                its, relres = d[t + "_conv"]
                assert relres <= 1e-5, (lab, its, relres)       # a converged state (the reference's own rtol)
                _, _, dfa, _ = arb.compliance_sens(nx, ny, nz, ld(KE), ld(U), ld(x))
                note(form, "dfdx", rw.assert_rowwise(d[t + "_df"], dfa, rw.scale_dfdx(nx, ny, nz, KE, U, x), rw.C_DFDX,
                                                     {"dims": (ex, ey, ez), "dof": 0, "label": lab + "dfdx"}), rw.C_DFDX)
    print("ACHIEVED", form, {k[1]: "%.3g of %g" % v for k, v in ACHIEVED.items() if k[0] == form})


# =====================================================================================================================
# later Chebyshev steps, the residual epilogue, the values of the fused dot products (rw.STEP_MESHES, rw.COARSE_MESHES)
# =====================================================================================================================
_WORK = {}


def worker_once(tmp_path_factory, mode, form, env, *args):
    """one subprocess per form and mode, shared by the test functions that compare its outputs"""
    if (mode, form) not in _WORK:
        d = run_worker(tmp_path_factory.mktemp(mode), mode, env, *args)
        _WORK[(mode, form)] = {k: d[k] for k in d.files}
    return _WORK[(mode, form)]


def window(l, nlv, lam, lam_min):
    lmin = lam_min if (l == nlv - 1 and l > 0) else 0.1 * lam
    return 0.5 * (1.1 * lam + lmin), 0.5 * (1.1 * lam - lmin)


def check_later_steps(form, what, get, l, nlv, ks, b, u, A, S, where, lab):
    """step k of the sweeps from the zero guess and from u, for k in ks: the device's x_k against the step formed in 80-bit
    arithmetic from its own x_{k-1}, x_{k-2}, dinv and window.  A(v): the arbiter's product, S(v): the row scale S_l(|v|), both
    cached by the bits of v (forms that produce the same iterates share them)"""
    dinv, (lam, lam_min) = get("dinv"), get("lam")
    theta, delta = window(l, nlv, float(lam), float(lam_min))
    c = rw.c_smooth_k(l)
    for zero in (1, 0):
        xs = lambda j: (np.zeros_like(u) if zero else u) if j == 0 else get("z%d_x%d" % (zero, j))
        for k in ks:
            c1, c2 = rw.cheb_coeffs(theta, delta, k)
            x1, x2 = xs(k - 1), xs(k - 2)
            xa = rw.step_k_ref(x1, x2, c1, c2, dinv, b, A(x1))
            sc = rw.scale_smooth_k(S(x1), dinv, c1, c2, b, x1, x2)
            note(form, "%sstep %s %s" % (what, "2, 3" if k <= 3 else k, "zero" if zero else "non-zero"),
                 rw.assert_rowwise(xs(k), xa, sc, c, dict(where, label=lab + "Chebyshev step %d of a sweep from %s" % (k, "the zero guess" if zero else "u"))), c)


def fine_case_refs(orc, arb, d, form, m, scattered):
    ex, ey, ez = rw.STEP_MESHES[m]
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    tag = "m%d_s%d" % (m, scattered)
    N, KE = d[tag + "_N"], d[tag + "_KE"]
    kf = d[tag + "_kf"] if form != "per_node" else ld(KE)
    return (ex, ey, ez), (nx, ny, nz), tag, N, KE, kf


def fine_ops(orc, arb, dims, KE, kf, E, N, key):
    nx, ny, nz = dims
    A = lambda v: cached(key + ("A", hash(v.tobytes())), lambda: arb.matfree_apply(nx, ny, nz, 3, ld(kf), ld(E), ld(N), ld(v)))
    S = lambda v: cached(key + ("S", hash(v.tobytes())), lambda: rw.scale_fine(orc, nx, ny, nz, KE, E, v, N))
    return A, S


@pytest.mark.parametrize("form", list(FINE_FORMS))
def test_fine_later_steps_and_residual_rowwise(tmp_path_factory, orc, arb, form):
    """steps 2 and 3 of a sweep (the three-term form: load_prev, prev_zero) and r = b - A x through EPI_RESID, row by row"""
    env, expect = FINE_FORMS[form]
    d = worker_once(tmp_path_factory, "fine_steps", form, env, expect)
    for m in range(len(rw.STEP_MESHES)):
        for scattered in (0, 1):
            mesh, dims, tag, N, KE, kf = fine_case_refs(orc, arb, d, form, m, scattered)
            u, b = d[tag + "_u"], d[tag + "_b"]
            for kind in rw.GENERATORS:
                t = "%s_%s" % (tag, kind)
                x = d[t + "_x"]
                E = orc.simp(x)
                A, S = fine_ops(orc, arb, dims, KE, kf, E, N, ("steps", m, scattered, form == "per_node", hash(x.tobytes())))
                lab = "%s mesh %s %s %s: " % (form, mesh, "scattered" if scattered else "cantilever", kind)
                check_later_steps(form, "", lambda name: d[t + "_" + name], 0, 1, rw.STEP_KS, b, u, A, S,
                                  {"dims": dims, "kz": int(d[t + "_formk"][3])}, lab)
                note(form, "residual", rw.assert_rowwise(d[t + "_resid"], ld(b) - A(u), np.abs(b) + S(u), rw.c_resid(0),
                                                         {"dims": dims, "kz": int(d[t + "_formr"][3]), "label": lab + "residual"}), rw.c_resid(0))
    print("ACHIEVED", form, {k[1]: "%.3g of %g" % v for k, v in ACHIEVED.items() if k[0] == form})


@pytest.mark.parametrize("form", list(FINE_FORMS))
def test_fine_fused_dot_values(tmp_path_factory, orc, arb, form):
    """p . A p of EPI_APPLY_DOT (every form) and b . x_out of EPI_CHEB_DOT (generations 2, 3) against the sums formed in 80-bit
    arithmetic from the device's own vectors: who owns a seam node, and the summation.  Two inputs: the seeded fields, and the
    same set to zero wherever the row's scale exceeds 1e-6 of the largest -- void terms only, where a node counted twice or not
    at all is a whole term and not 1e-9 of one.  (The worker asserts the vectors bit-equal to MatMultKrylov's and smooth's.)"""
    env, expect = FINE_FORMS[form]
    d = worker_once(tmp_path_factory, "fine_steps", form, env, expect)
    gen = int(d["gen"][0])
    assert gen >= 2 or form in ("gen1", "per_node"), (form, gen)       # every other form carries the fused b . x_out
    for m in range(len(rw.STEP_MESHES)):
        for scattered in (0, 1):
            mesh, dims, tag, N, KE, kf = fine_case_refs(orc, arb, d, form, m, scattered)
            for kind in rw.GENERATORS:
                for name in ("n", "v"):
                    t = "%s_%s_dot_%s" % (tag, kind, name)
                    lab = "%s mesh %s %s %s input %s: " % (form, mesh, "scattered" if scattered else "cantilever", kind, name)
                    pairs = [("u . A u", d[t + "_u"], d[t + "_y"], float(d[t + "_pw"][0]), d[t + "_formy"])]
                    if gen >= 2:
                        pairs += [("b . x_out, zero guess %d" % z, d[t + "_b"], d["%s_z%d_x" % (t, z)], float(d["%s_z%d_bx" % (t, z)][0]),
                                   d["%s_z%d_form" % (t, z)]) for z in (0, 1)]
                    for what, a, v, got, f in pairs:
                        terms = ld(a) * ld(v)
                        ref, size = terms.sum(), float(np.abs(terms).sum())
                        kz, nwg = (int(f[3]) if int(f[0]) == 1 else 1), rw.dot_workgroups(f, dims)
                        c = rw.c_dot(kz, nwg)
                        assert np.isfinite(got), (lab, what)
                        # rows that touch void elements only exist on every design but one_void (there the sum is an exact 0)
                        assert np.count_nonzero(terms) >= (3 if (name == "n" or kind != "one_void") else 0), (lab, what)
                        err = float(abs(np.longdouble(got) - ref))
                        print("%s%s: got %.17g, |got - ref| = %.3e = %.3g eps sum|terms|, bound %d (kz %d, %d workgroups)" % (lab, what, got, err, err / (rw.EPS * max(size, 1e-300)), c, kz, nwg))
                        assert err <= c * rw.EPS * size, "%s%s: |got - ref| = %.3e > %d eps sum|terms| = %.3e (kz %d, %d workgroups)" % (lab, what, err, c, c * rw.EPS * size, kz, nwg)
                        note(form, "dot " + what.split(",")[0], err / (rw.EPS * max(size, 1e-300)), c)
    print("ACHIEVED", form, {k[1]: "%.3g of %g" % v for k, v in ACHIEVED.items() if k[0] == form})


@pytest.mark.parametrize("form", list(COARSE_FORMS))
def test_coarse_later_steps_and_residual_rowwise(tmp_path_factory, orc, arb, form):
    """steps 2 and 3 of a sweep on every level (the stored direction d), step 20 on the coarsest level (from the zero guess: the
    one-launch run), and the residual epilogue of every level"""
    env, expect, lvl1, _ = COARSE_FORMS[form]
    d = worker_once(tmp_path_factory, "coarse_steps", form, env, expect, lvl1)
    for m, ((ex, ey, ez), nlv) in enumerate(COARSE_MESHES):
        nx, ny, nz = ex + 1, ey + 1, ez + 1
        tag = "c%d" % m
        N, KE, kf = d[tag + "_N"], d[tag + "_KE"], d[tag + "_kf"]
        for kind in rw.GENERATORS:
            t = "%s_%s" % (tag, kind)
            x = d[t + "_x"]
            E = orc.simp(x)

            def hier():
                mg, amg = orc.MG(nx, ny, nz, 3, nlv), arb.MG(nx, ny, nz, 3, nlv)
                mg.assemble(KE, E, N)
                amg.assemble(ld(KE), ld(E), ld(N))
                return mg, amg
            xk = hash(x.tobytes())
            mg, amg = cached(("hier", m, kind, xk), hier)
            lab = "%s mesh %s %d levels %s: " % (form, (ex, ey, ez), nlv, kind)
            for l in range(nlv):
                dims = rw.level_dims(nx, ny, nz, l)
                u, b = d["%s_u%d" % (t, l)], d["%s_b%d" % (t, l)]
                if l == 0:
                    A, S = fine_ops(orc, arb, (nx, ny, nz), KE, kf, E, N, ("steps0", m, xk))
                else:
                    A = lambda v: cached(("A", m, xk, l, hash(v.tobytes())), lambda: amg.apply(l, ld(v)))
                    S = lambda v: cached(("S", m, xk, l, hash(v.tobytes())), lambda: rw.scale_level(orc, mg, l, (nx, ny, nz), KE, E, N, v))
                f = tuple(int(v) for v in d["%s_l%d_formr" % (t, l)])
                w = {"dims": dims, "kz": f[3] if f[0] in (1, 2) else 0}
                name = "level 0 " if l == 0 else ("level1 " if l == 1 else "stencil ")
                ks = rw.STEP_KS + ((rw.STEP_K_COARSEST,) if l == nlv - 1 else ())
                check_later_steps(form, name, lambda q: d["%s_l%d_%s" % (t, l, q)], l, nlv, ks, b, u, A, S, w, lab + "level %d form %s " % (l, f))
                note(form, name + "residual", rw.assert_rowwise(d["%s_l%d_resid" % (t, l)], ld(b) - A(u), np.abs(b) + S(u), rw.c_resid(l),
                                                                dict(w, label=lab + "level %d residual, form %s" % (l, f))), rw.c_resid(l))
    if form in L2_FORMS:
        # did the latched switch take effect?  Against the default job's dump (same inputs, same worker): the generic contraction
        # sums level 2's element matrices in another order -- its Jacobi diagonals on the levels >= 2 are NOT all the default's
        # bits; k_galerkin_l2_fast forms an element with the same arithmetic whichever workgroup takes it, so 7 workgroups must
        # reproduce EVERY bit of the default job (an element left out or formed twice by the stride would show here; that the
        # stride ran is visible in no result, by construction)
        env0, expect0, lvl10, _ = COARSE_FORMS["level1_from_fine_fused_corr"]
        d0 = worker_once(tmp_path_factory, "coarse_steps", "level1_from_fine_fused_corr", env0, expect0, lvl10)
        assert sorted(d0) == sorted(d)
        differ = [k for k in sorted(d) if not (d0[k].shape == d[k].shape and np.array_equal(d0[k], d[k]))]
        print("L2 form %s: %d of %d dumped arrays differ from the default job's bits" % (form, len(differ), len(d)))
        if L2_FORMS[form]:
            assert not differ, differ[:8]
        else:
            assert any(k.endswith("_l2_dinv") for k in differ), differ[:8]
            assert not [k for k in differ if "_l0_" in k or "_l1_" in k], "levels 0 and 1 do not depend on level 2's contraction"
    print("ACHIEVED", form, {k[1]: "%.3g of %g" % v for k, v in ACHIEVED.items() if k[0] == form})


# form -> (environment, ElemConn -> kernel that must run: 1 tiled, 2 several outputs along z, 3 wide, 4 streamed ring, 5 generic)
FILTER_FORMS = {
    "by_radius": ({}, "1:1,2:1,5:3,10:4"),
    "zmulti4": ({"TP_FILTER_ZMULTI": "4"}, "1:2,2:2,5:3,10:4"),
    "generic": ({"TP_NO_FILTER_TILE": "1"}, "1:5,2:5,5:5,10:5"),
}


@pytest.mark.parametrize("form", list(FILTER_FORMS))
def test_cone_filter_rowwise(tmp_path, orc, arb, form):
    """forward and gradients, types 0 and 1, rfac 1.5, 2.56 (tiled), 5.12 (wide), 10.24 (streamed ring), on the 0/1 designs and on the
    two with exact zeros (rw.FILTER_ZERO_KINDS): there the sensitivity filter's rows with x_i = 0 must be exactly 0.0 -- PETSc's
    quotient, which the arbiter forms too -- and every other row keeps its bound"""
    env, expect = FILTER_FORMS[form]
    out = str(tmp_path / "out.npz")
    e = dict(os.environ)
    for k in ("TP_FILTER_ZMULTI", "TP_NO_FILTER_TILE"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rowwise_worker.py"), "filter", expect, out], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-3000:]
    d = np.load(out)
    ex, ey, ez = rw.FILTER_MESH
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    df0 = d["df0"]
    for rfac in rw.FILTER_RFACS:
        af = cached(("af", rfac), lambda: arb.Filter(nx, ny, nz, h, rfac * h))
        cone = cached(("cone", rfac), lambda: rw.Cone(ex, ey, ez, h, rfac * h, af.conn))
        c = rw.c_filter(af.conn)
        for ftype in (1, 0):
            t = "r%g_t%d" % (rfac, ftype)
            assert int(d[t + "_conn"][0]) == af.conn
            w = {"dims": (ex, ey, ez), "dof": 0}
            lab = "filter %s type %d rfac %g ElemConn %d " % (form, ftype, rfac, af.conn)
            note("filter " + form, "Hs conn %d" % af.conn, rw.assert_rowwise(d[t + "_hs"], af.hs(), cone.M(np.ones(ex * ey * ez)), c, dict(w, label=lab + "Hs")), c)
            for kind in rw.GENERATORS + rw.FILTER_ZERO_KINDS:
                x = rw.filter_design(kind, ex, ey, ez, 4)
                if kind in rw.FILTER_ZERO_KINDS and ftype == 0:
                    got0 = d["%s_%s_df" % (t, kind)][x == 0]
                    assert got0.size and (got0 == 0).all() and not np.signbit(got0).any(), lab + kind + ": a row with x = 0 is not 0.0"
                xta, ga = cached(("fref", rfac, ftype, kind), lambda: (af.project(ftype, ld(x))[0], None))
                ga = cached(("gref", rfac, ftype, kind), lambda: af.gradient(ftype, ld(x), xta, ld(df0)))
                note("filter " + form, "forward conn %d" % af.conn,
                     rw.assert_rowwise(d["%s_%s_xt" % (t, kind)], xta, cached(("sf", rfac, ftype, kind), lambda: cone.scale_forward(ftype, x)), c, dict(w, label=lab + kind + " forward")), c)
                note("filter " + form, "gradient conn %d" % af.conn,
                     rw.assert_rowwise(d["%s_%s_df" % (t, kind)], ga, cached(("sg", rfac, ftype, kind), lambda: cone.scale_gradient(ftype, x, df0)), c, dict(w, label=lab + kind + " gradient")), c)
    print("ACHIEVED", "filter " + form, {k[1]: "%.3g of %g" % v for k, v in ACHIEVED.items() if k[0] == "filter " + form})
