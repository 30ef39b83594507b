"""Worker of tests/test_gpu_cg_fusions.py: one process per setting of the latched library switches (the parent puts them into
the environment).  Runs the cases of its mode with the solver of the benchmark's cycle, asserts the fine kernel generation that
launched, and dumps precond(r) of a seeded r, the residual history and U of a solve of exactly max_it iterations to one .npz.

usage: cg_fusions_worker.py small <generation> <out.npz>      rw.COARSE_MESHES x blocks, checker, zlayer x both boundary conditions
       cg_fusions_worker.py large <generation> <out.npz>      128 x 104 x 104 elements, blocks: the non-temporal CG update's size"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import topopt_in_petsc_amd as tp  # noqa: E402
from tests import rowwise as rw  # noqa: E402
from tests.rowwise_worker import bc, dev, host  # noqa: E402

CYCLES = (1, 3, 1, 1)            # bench.py's pattern (cantilever128), cut to the level count
KINDS = rw.CG_FUSION_KINDS
LARGE = ((128, 104, 104), 3, 5)  # elements, levels, iterations: 3 x 129 x 105 x 105 = 4 266 675 dofs >= 2^22


def run(mesh, nlv, its, kind, scattered, seed, gen, res, tag, with_precond=True):
    ex, ey, ez = mesh
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    rng = np.random.default_rng(seed)
    grid = tp.Grid(nx, ny, nz, h)
    # rtol tiny, dtol huge: exactly max_it iterations
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=nlv, nsmooth=2, ncoarse=20, rtol=1e-300, dtol=1e300, max_it=its))
    bc(le, nx, ny, nz, scattered, rng)
    le.set_cycles(list(CYCLES[:nlv - 1]))
    le.AssembleStiffnessMatrix(dev(rw.design(kind, ex, ey, ez, 8)), 1e-9, 1.0, 3.0)
    r = rng.standard_normal(3 * nx * ny * nz)
    le.MatMult(dev(r))
    form = le.last_op_form()
    assert form[:2] == (1, gen), "%s: fine kernel form %s, expected generation %d" % (tag, form, gen)
    if with_precond:
        res[tag + "_z"] = host(le.precond(dev(r * host(le.N))))
    le.U.zero_()
    assert le.KSPSolve(hist_cap=its + 1) == its, (tag, le.last_its)
    res[tag + "_hist"], res[tag + "_U"] = np.asarray(le.last_hist), host(le.U)
    assert np.isfinite(res[tag + "_hist"]).all() and len(res[tag + "_hist"]) == its + 1, tag
    le.close()
    grid.close()


if __name__ == "__main__":
    mode, gen, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    tp.load_library()
    res = {}
    if mode == "small":
        for m, (mesh, nlv) in enumerate(rw.COARSE_MESHES):
            for kind in KINDS:
                for scattered in (0, 1):
                    run(mesh, nlv, 40, kind, scattered, 900 + 10 * m + scattered, gen, res, "c%d_%s_s%d" % (m, kind, scattered))
    else:
        mesh, nlv, its = LARGE
        run(mesh, nlv, its, "blocks", 0, 990, gen, res, "large", with_precond=False)
    np.savez(out, **res)
    print("cg fusions worker %s OK" % mode)
