"""Worker of tests/test_gpu_coarse_direct.py: one process per setting of the latched library switches (TP_CD_INVERT_COLUMNS, the
switches that serialise the overlapped set-up).  Per case of rw.CD_CASES it assembles the designs of rw.CD_SEQUENCE one after the
other on ONE LinearElasticity -- blocks, checker, blocks, checker, then the rest -- and after every assembly, with nothing between
the assembly and the first use but the library's own events, dumps the exact coarse solve of both right-hand sides, what the
coarsest operator makes of the solutions, precond(r), the rows coarse_direct_active() reports and, for the four assemblies of
the A / B / A / B sequence, level_apply, level_dinv and the Chebyshev window of every level (the set-up cases of rw.CD_SETUP_CASES
also the residual history of KSPSolve from a zero start).  Even assemblies use the coarse solve first, odd ones the V-cycle.
The parent compares.

Every case runs with coarse_direct = 2 (which admits the whole window; from 449 rows on it is the same code as 1); what
coarse_direct = 1 reports for the case comes from a second solver object.

usage: coarse_direct_worker.py <out.npz> <case indices, comma separated, or -> <0|1: the rejected geometries too>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import topopt_in_petsc_amd as tp  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import rowwise as rw  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def options(nlv, cd):
    return tp.SolverOptions(nlvls=nlv, nsmooth=2, ncoarse=20, rtol=1e-6, max_it=30, dtol=1e300, coarse_direct=cd)


def case(ci, res):
    mesh, nlv = rw.CD_CASES[ci][:2]
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    dims = rw.cd_geom(mesh, nlv)[0]
    lc = nlv - 1
    grid = tp.Grid(nx, ny, nz, h)
    tag = "c%d" % ci
    le = tp.LinearElasticity(grid, options(nlv, 1))
    le.SetUpLoadAndBC()
    le.AssembleStiffnessMatrix(dev(rw.cd_design(orc, "synth", mesh)), 1e-9, 1.0, 3.0)
    res[tag + "_active_cd1"] = np.asarray([le.coarse_direct_active()])
    le.close()
    le = tp.LinearElasticity(grid, options(nlv, 2))
    le.SetUpLoadAndBC()
    res[tag + "_N"], res[tag + "_KE"] = host(le.N), le.KE
    rng = np.random.default_rng(4100 + ci)
    bs = rw.cd_rhs(dims, ci)
    r = rng.standard_normal(3 * nx * ny * nz)
    us = [rng.standard_normal(3 * int(np.prod(rw.level_dims(nx, ny, nz, l)))) for l in range(nlv)]
    res[tag + "_r"] = r
    for l in range(nlv):
        res["%s_u%d" % (tag, l)] = us[l]
    for step, kind in enumerate(rw.CD_SEQUENCE):
        x = rw.cd_design(orc, kind, mesh)
        # every device input exists before the assembly: no copy (and no synchronisation with it) between assembly and first use
        xd, rd = dev(x), dev(r)
        bd = {name: dev(b) for name, b in bs.items()}
        xs = {name: torch.zeros_like(b) for name, b in bd.items()}
        ud = [dev(u) for u in us]
        torch.cuda.synchronize()
        le.AssembleStiffnessMatrix(xd, 1e-9, 1.0, 3.0)
        t = "%s_s%d" % (tag, step)
        z = None
        if step % 2:
            z = le.precond(rd)
        for name in bd:
            le.smooth(lc, bd[name], xs[name], 20, True)
        if z is None:
            z = le.precond(rd)
        res[t + "_x"], res[t + "_z"] = x, host(z)
        res[t + "_active"] = np.asarray([le.coarse_direct_active()])
        for name in bd:
            res["%s_xs_%s" % (t, name)] = host(xs[name])
            res["%s_Axs_%s" % (t, name)] = host(le.level_apply(lc, xs[name]))
        if step < 4:
            for l in range(nlv):
                res["%s_apply%d" % (t, l)] = host(le.level_apply(l, ud[l]))
                res["%s_dinv%d" % (t, l)] = host(le.level_dinv(l))
                res["%s_lam%d" % (t, l)] = np.asarray([le.level_lambda(l), le.level_lambda_min(l)])
            if ci in rw.CD_SETUP_CASES:
                le.U.zero_()
                its = le.KSPSolve(hist_cap=64)
                res[t + "_hist"], res[t + "_its"] = np.asarray(le.last_hist), np.asarray([its])
    res[tag + "_xcd"] = np.asarray([int(v) for v in le.xcd_status()])
    le.close()
    grid.close()


def rejected(mesh, nlv, cds, tag, res):
    """a geometry outside the window of coarse_direct in cds: 0 rows, and the solve of coarse_direct = 0"""
    ex, ey, ez = mesh
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ey)
    x = dev(rw.cd_design(orc, "synth", mesh))
    for c in cds + (0,):
        le = tp.LinearElasticity(grid, options(nlv, c))
        le.SetUpLoadAndBC()
        le.AssembleStiffnessMatrix(x, 1e-9, 1.0, 3.0)
        res["%s_cd%d_active" % (tag, c)] = np.asarray([le.coarse_direct_active()])
        its = le.KSPSolve(hist_cap=64)
        res["%s_cd%d_U" % (tag, c)], res["%s_cd%d_its" % (tag, c)] = host(le.U), np.asarray([its])
        le.close()
    grid.close()


if __name__ == "__main__":
    out, cases, rej = sys.argv[1], sys.argv[2], int(sys.argv[3])
    tp.load_library()
    res = {}
    for ci in ([] if cases == "-" else [int(v) for v in cases.split(",")]):
        case(ci, res)
    if rej:
        for q, (mesh, nlv) in enumerate(rw.CD_REJECTED):
            rejected(mesh, nlv, (1, 2), "rej%d" % q, res)
        for ci, c in enumerate(rw.CD_CASES):    # admitted only with coarse_direct = 2
            if c[2] == 0:
                rejected(c[0], c[1], (1,), "rejc%d" % ci, res)
    np.savez(out, **res)
    print("coarse direct worker OK")
