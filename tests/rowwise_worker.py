"""Worker of tests/test_gpu_rowwise.py: one process per setting of the latched library switches.  Runs every mesh, boundary
condition and 0/1 design of its job through the kernels, asserts that the FORCED form is the one that launched
(LinearElasticity.last_op_form), and dumps inputs and outputs to one .npz; the parent compares them with the 80-bit arbiter.

usage: rowwise_worker.py filter <conn:kernel,...> <out.npz>      kernel as Filter.last_kernel returns it
       rowwise_worker.py fine <expect> <out.npz>
       rowwise_worker.py coarse <expect of the levels >= 2> <out.npz> <expect of level 1> <0|1: dfdx on a solved state too>
       rowwise_worker.py fine_steps <expect> <out.npz>          later Chebyshev steps, residual epilogue, fused dot products
       rowwise_worker.py coarse_steps <expect of the levels >= 2> <out.npz> <expect of level 1>       the same on every level
expect: "kind,a,b,c" as last_op_form returns them, '*' = any, '<=n' = at most n"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import topopt_in_petsc_amd as tp  # noqa: E402
from tests import rowwise as rw  # noqa: E402

FINE_MESHES, COARSE_MESHES = rw.FINE_MESHES, rw.COARSE_MESHES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(form, expect, what):
    for got, want in zip(form, expect):
        if want.startswith("<="):
            assert got <= int(want[2:]), "%s: form %s, expected %s" % (what, form, expect)
        elif want != "*":
            assert got == int(want), "%s: form %s, expected %s: the forced kernel form did not run" % (what, form, expect)


def bc(le, nx, ny, nz, scattered, rng):
    if not scattered:
        le.SetUpLoadAndBC()
        return
    N = np.ones(3 * nx * ny * nz)
    N[rng.random(N.size) < 2e-2] = 0.0
    N[: 3 * nx].reshape(-1, 3)[:, :] = 0.0
    le.SetBC(dev(N), dev(rng.standard_normal(N.size) * 1e-3))


def fine(expect, res):
    for m, (ex, ey, ez) in enumerate(FINE_MESHES):
        nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
        for scattered in (0, 1):
            rng = np.random.default_rng(100 * m + scattered)
            grid = tp.Grid(nx, ny, nz, h)
            le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
            bc(le, nx, ny, nz, scattered, rng)
            u, b = rng.standard_normal(3 * nx * ny * nz), rng.standard_normal(3 * nx * ny * nz)
            tag = "m%d_s%d" % (m, scattered)
            res[tag + "_N"], res[tag + "_u"], res[tag + "_b"] = host(le.N), u, b
            res[tag + "_kf"], res[tag + "_kk"], res[tag + "_KE"] = le.KE_effective(), le.KE_krylov(), le.KE
            # the chunk lengths of the product and of the Chebyshev step (they may differ), from a first assembly
            le.AssembleStiffnessMatrix(dev(rw.design("one_void", ex, ey, ez)), 1e-9, 1.0, 3.0)
            le.MatMult(dev(u))
            kza = le.last_op_form()[3]
            le.smooth(0, dev(b), dev(u), 1, False)
            kzs = (kza, le.last_op_form()[3])
            for kind in rw.GENERATORS:
                x = rw.design(kind, ex, ey, ez, tuple(k or 8 for k in kzs))
                le.AssembleStiffnessMatrix(dev(x), 1e-9, 1.0, 3.0)
                t = "%s_%s" % (tag, kind)
                res[t + "_x"] = x
                res[t + "_apply"] = host(le.MatMult(dev(u)))
                form = le.last_op_form()
                check(form, expect, "%s apply" % t)
                res[t + "_form"] = np.asarray(form)
                res[t + "_krylov"] = host(le.MatMultKrylov(dev(u)))
                check(le.last_op_form(), expect[:3], "%s apply_krylov" % t)
                res[t + "_cheb0"] = host(le.smooth(0, dev(b), torch.zeros_like(dev(b)), 1, True))
                res[t + "_cheb1"] = host(le.smooth(0, dev(b), dev(u), 1, False))
                check(le.last_op_form(), expect[:3], "%s Chebyshev step" % t)
                res[t + "_formc"] = np.asarray(le.last_op_form())
                res[t + "_dinv"] = host(le.level_dinv(0))
                res[t + "_lam"] = np.asarray([le.level_lambda(0)])
            le.close()
            grid.close()


def coarse(expect, res, lvl1, dfdx):
    for m, ((ex, ey, ez), nlv) in enumerate(COARSE_MESHES):
        nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
        rng = np.random.default_rng(500 + m)
        grid = tp.Grid(nx, ny, nz, h)
        le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=nlv, rtol=1e-5, max_it=3000, dtol=1e300))
        le.SetUpLoadAndBC()
        tag = "c%d" % m
        res[tag + "_N"], res[tag + "_R"], res[tag + "_KE"] = host(le.N), host(le.RHS), le.KE
        for kind in rw.GENERATORS:
            # level 1's chunks are in level-1 planes: two fine element layers each -> fine layers at multiples of 2 kz
            x = rw.design(kind, ex, ey, ez, 2 * int(os.environ.get("TP_MACRO_KZ", "2")))
            le.AssembleStiffnessMatrix(dev(x), 1e-9, 1.0, 3.0)
            t = "%s_%s" % (tag, kind)
            res[t + "_x"] = x
            for l in range(nlv):
                n = 3 * le.level_nodes(l)
                u, b = rng.standard_normal(n), rng.standard_normal(n)
                res["%s_u%d" % (t, l)], res["%s_b%d" % (t, l)] = u, b
                if l > 0:
                    res["%s_apply%d" % (t, l)] = host(le.level_apply(l, dev(u)))
                    form = le.last_op_form()
                    e = lvl1 if l == 1 else expect
                    check(form, e, "%s level %d" % (t, l))
                    res["%s_form%d" % (t, l)] = np.asarray(form)
                    res["%s_cheb0_%d" % (t, l)] = host(le.smooth(l, dev(b), torch.zeros_like(dev(b)), 1, True))
                    res["%s_cheb1_%d" % (t, l)] = host(le.smooth(l, dev(b), dev(u), 1, False))
                    check(le.last_op_form(), e[:3], "%s level %d Chebyshev step" % (t, l))
                    res["%s_dinv%d" % (t, l)] = host(le.level_dinv(l))
                    res["%s_lam%d" % (t, l)] = np.asarray([le.level_lambda(l), le.level_lambda_min(l)])
                if l + 1 < nlv:
                    xc = rng.standard_normal(3 * le.level_nodes(l + 1))
                    res["%s_xc%d" % (t, l)] = xc
                    res["%s_restrict%d" % (t, l)] = host(le.restrict(l, dev(u)))
                    res["%s_prolong%d" % (t, l)] = host(le.prolong_add(l, dev(xc), dev(b)))
            if dfdx:
                le.U.zero_()
                le.KSPSolve()
                df, dg = grid.elem_vec(), grid.elem_vec()
                le.ComputeSensitivities(df, dg, dev(x), 1e-9, 1.0, 3.0)
                res[t + "_U"], res[t + "_df"] = host(le.U), host(df)
                res[t + "_conv"] = np.asarray([le.last_its, le.last_rnorm / le.last_bnorm])
        le.close()
        grid.close()


def sweeps(le, l, b, u, ks, res, t):
    """the device's own iterates x_{k-2}, x_{k-1}, x_k of the sweeps from the zero guess and from u: res[t_z<zero>_x<j>]"""
    for zero in (1, 0):
        for j in sorted({j for k in ks for j in (k - 2, k - 1, k) if j > 0}):
            x0 = torch.zeros_like(dev(b)) if zero else dev(u)
            res["%s_z%d_x%d" % (t, zero, j)] = host(le.smooth(l, dev(b), x0, j, bool(zero)))


def fine_steps(expect, res):
    from oracle import oracle as orc
    gen = None
    for m, (ex, ey, ez) in enumerate(rw.STEP_MESHES):
        nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
        for scattered in (0, 1):
            rng = np.random.default_rng(300 + 10 * m + scattered)
            grid = tp.Grid(nx, ny, nz, h)
            le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
            bc(le, nx, ny, nz, scattered, rng)
            n = 3 * nx * ny * nz
            u, b = rng.standard_normal(n), rng.standard_normal(n)
            tag = "m%d_s%d" % (m, scattered)
            N = host(le.N)
            res[tag + "_N"], res[tag + "_u"], res[tag + "_b"] = N, u, b
            res[tag + "_kf"], res[tag + "_KE"] = le.KE_effective(), le.KE
            # the chunk lengths of every launch under test (they may differ), from a first assembly
            le.AssembleStiffnessMatrix(dev(rw.design("one_void", ex, ey, ez)), 1e-9, 1.0, 3.0)
            kzs = []
            for call in (lambda: le.smooth(0, dev(b), dev(u), 2, False), lambda: le.level_residual(0, dev(b), dev(u)),
                         lambda: le.MatMultKrylovDot(dev(u))):
                call()
                kzs.append(le.last_op_form()[3] or 8)
            for kind in rw.GENERATORS:
                x = rw.design(kind, ex, ey, ez, tuple(kzs))
                le.AssembleStiffnessMatrix(dev(x), 1e-9, 1.0, 3.0)
                t = "%s_%s" % (tag, kind)
                res[t + "_x"] = x
                sweeps(le, 0, b, u, rw.STEP_KS, res, t)
                check(le.last_op_form(), expect, "%s Chebyshev step %d" % (t, max(rw.STEP_KS)))
                res[t + "_formk"] = np.asarray(le.last_op_form())
                res[t + "_dinv"] = host(le.level_dinv(0))
                res[t + "_lam"] = np.asarray([le.level_lambda(0), le.level_lambda_min(0)])
                res[t + "_resid"] = host(le.level_residual(0, dev(b), dev(u)))
                check(le.last_op_form(), expect, "%s residual" % t)
                res[t + "_formr"] = np.asarray(le.last_op_form())
                # ---- the fused dot products: the seeded fields, and the same set to zero wherever the row's scale exceeds 1e-6 of
                # the largest -- a sum of void terms only
                s = rw.scale_fine(orc, nx, ny, nz, le.KE, orc.simp(x), u, N)
                void = s <= 1e-6 * s.max()
                for name, uu, bb in (("n", u, b), ("v", u * void, b * void)):
                    res["%s_dot_%s_u" % (t, name)], res["%s_dot_%s_b" % (t, name)] = uu, bb
                    y, d = le.MatMultKrylovDot(dev(uu))
                    form = le.last_op_form()
                    check(form, expect, "%s apply_krylov_dot" % t)
                    assert torch.equal(y, le.MatMultKrylov(dev(uu))), "%s: MatMultKrylovDot's product differs from MatMultKrylov's" % t
                    res["%s_dot_%s_y" % (t, name)], res["%s_dot_%s_pw" % (t, name)], res["%s_dot_%s_formy" % (t, name)] = host(y), np.asarray([d]), np.asarray(form)
                    gen = form[1] if form[0] == 1 else 0
                    for zero in (0, 1):
                        x0 = lambda: torch.zeros_like(dev(bb)) if zero else dev(uu)
                        if gen >= 2:
                            xo, d = le.smooth_dot(0, dev(bb), x0(), 2, bool(zero))
                            form = le.last_op_form()
                            check(form, expect, "%s smooth_dot" % t)
                            assert torch.equal(xo, le.smooth(0, dev(bb), x0(), 2, bool(zero))), "%s: smooth_dot's iterate differs from smooth's" % t
                            k = "%s_dot_%s_z%d" % (t, name, zero)
                            res[k + "_x"], res[k + "_bx"], res[k + "_form"] = host(xo), np.asarray([d]), np.asarray(form)
                        else:       # no fused b . x_out on this kernel: an error, not a silent number
                            try:
                                le.smooth_dot(0, dev(bb), x0(), 2, bool(zero))
                            except tp.TopOptError as err:
                                assert err.code == 2, err
                            else:
                                raise AssertionError("%s: smooth_dot on a kernel without the fused dot returned a value" % t)
            le.close()
            grid.close()
    res["gen"] = np.asarray([gen])


def coarse_steps(expect, res, lvl1):
    for m, ((ex, ey, ez), nlv) in enumerate(COARSE_MESHES):
        nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
        rng = np.random.default_rng(700 + m)
        grid = tp.Grid(nx, ny, nz, h)
        le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=nlv))
        le.SetUpLoadAndBC()
        tag = "c%d" % m
        res[tag + "_N"], res[tag + "_KE"], res[tag + "_kf"] = host(le.N), le.KE, le.KE_effective()
        for kind in rw.GENERATORS:
            x = rw.design(kind, ex, ey, ez, 2 * int(os.environ.get("TP_MACRO_KZ", "2")))
            le.AssembleStiffnessMatrix(dev(x), 1e-9, 1.0, 3.0)
            t = "%s_%s" % (tag, kind)
            res[t + "_x"] = x
            for l in range(nlv):
                n = 3 * le.level_nodes(l)
                u, b = rng.standard_normal(n), rng.standard_normal(n)
                res["%s_u%d" % (t, l)], res["%s_b%d" % (t, l)] = u, b
                e = ["1", "*", "*", "*"] if l == 0 else (lvl1 if l == 1 else expect)
                tl = "%s_l%d" % (t, l)
                sweeps(le, l, b, u, rw.STEP_KS, res, tl)        # (last: k = 3 from u, separate launches on every level)
                check(le.last_op_form(), e[:3], "%s level %d Chebyshev step" % (t, l))
                if l == nlv - 1:
                    sweeps(le, l, b, u, (rw.STEP_K_COARSEST,), res, tl)
                res[tl + "_dinv"] = host(le.level_dinv(l))
                res[tl + "_lam"] = np.asarray([le.level_lambda(l), le.level_lambda_min(l)])
                res[tl + "_resid"] = host(le.level_residual(l, dev(b), dev(u)))
                form = le.last_op_form()
                check(form, e, "%s level %d residual" % (t, l))
                res[tl + "_formr"] = np.asarray(form)
        le.close()
        grid.close()


def cone_filter(expect, res):
    want = dict((int(a), int(b)) for a, b in (p.split(":") for p in expect))
    ex, ey, ez = rw.FILTER_MESH
    h = 1.0 / ey
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
    rng = np.random.default_rng(900)
    df0 = rng.standard_normal(ex * ey * ez)
    res["df0"] = df0
    for rfac in rw.FILTER_RFACS:
        for ftype in (1, 0):
            f = tp.Filter(grid, ftype, rfac * h)
            conn = f.ElemConn
            assert f.last_kernel() == want[conn], "ElemConn %d: kernel %d ran for Hs, expected %d" % (conn, f.last_kernel(), want[conn])
            t = "r%g_t%d" % (rfac, ftype)
            res[t + "_conn"], res[t + "_hs"] = np.asarray([conn]), host(f.Hs())
            for kind in rw.GENERATORS + rw.FILTER_ZERO_KINDS:
                x = rw.filter_design(kind, ex, ey, ez, 4)
                xt, xp = grid.elem_vec(), grid.elem_vec()
                f.FilterProject(dev(x), xt, xp)
                if ftype == 1:
                    assert f.last_kernel() == want[conn], (conn, f.last_kernel())
                df = dev(df0)
                f.Gradients(dev(x), xt, df, [])
                assert f.last_kernel() == want[conn], (conn, f.last_kernel())
                res["%s_%s_xt" % (t, kind)], res["%s_%s_df" % (t, kind)] = host(xt), host(df)
            f.close()
    grid.close()


if __name__ == "__main__":
    mode, expect, out = sys.argv[1], sys.argv[2].split(","), sys.argv[3]
    tp.load_library()
    res = {}
    if mode == "filter":
        cone_filter(expect, res)
    elif mode == "fine":
        fine(expect, res)
    elif mode == "fine_steps":
        fine_steps(expect, res)
    elif mode == "coarse_steps":
        coarse_steps(expect, res, sys.argv[4].split(","))
    else:
        coarse(expect, res, sys.argv[4].split(","), int(sys.argv[5]))
    np.savez(out, **res)
    print("rowwise worker %s OK" % mode)
