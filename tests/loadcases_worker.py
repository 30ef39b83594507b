"""Slab worker of tests/test_gpu_loadcases_slabs.py (launched by torch.distributed.run; every rank shares cuda:0, gloo with
host staging): tp_elasticity_response with three load cases on z-slabs against the one-rank call on the gathered fields.

Every rank builds the same global fields from one seed, takes its slab of them with STALE ghost planes (the call must refresh
them), and runs the one-rank call itself on a grid of its own: fx and every f_case to 1e-12, dfdx of the own layers to 1e-12
of its maximum (the kernel's own rounding, tests/test_gpu_loadcases.py; the slabs add a different summation order)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EMIN, EMAX, PENAL, VOLFRAC = 1e-9, 1.0, 3.0, 0.12
W = [0.5, 0.0, -2.0]


def response_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(5)
    n = 3 * nx * ny * nz
    U = [rng.uniform(-1.0, 1.0, n) for _ in range(3)]
    V = [rng.uniform(-1.0, 1.0, n), None, None]          # case 0 bilinear, cases 1 and 2 compliance
    # ---- one rank, global fields
    g1 = tp.Grid(nx, ny, nz, h)
    le1 = tp.LinearElasticity(g1, tp.SolverOptions(nlvls=2))
    x1 = g1.synth_density()
    d1 = g1.elem_vec()
    fx1, gx1, fc1 = le1.Response([dev(u) for u in U], [None if v is None else dev(v) for v in V], W, x1, EMIN, EMAX, PENAL,
                                 VOLFRAC, d1)
    d1 = d1.cpu().numpy()
    # ---- this rank's slab
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    part = grid.part
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=2))
    gs, es, pl = part.global_slice(3), part.global_elem_slice(), 3 * part.plane

    def slab(a):
        t = a[gs].copy()
        if part.has_lo:
            t[:pl] = 777.0            # stale ghost planes: the call refreshes them
        if part.has_hi:
            t[-pl:] = -777.0
        return dev(t)

    x = x1[es].clone()
    df, dg = grid.elem_vec(), grid.elem_vec()
    fx, gx, fc = le.Response([slab(u) for u in U], [None if v is None else slab(v) for v in V], W, x, EMIN, EMAX, PENAL, VOLFRAC,
                             df, dg)
    worst = max([abs(fx / fx1 - 1)] + [abs(a / b - 1) for a, b in zip(fc, fc1)])
    errd = float(np.abs(df.cpu().numpy() - d1[es]).max() / np.abs(d1).max())
    print("rank %d: max rel error of fx, f_case %.3e (bound 1e-12); dfdx %.3e (bound 1e-12); |gx - gx1| %.3e (bound 1e-13)"
          % (rank, worst, errd, abs(gx - gx1)), flush=True)
    assert worst <= 1e-12 and errd <= 1e-12 and abs(gx - gx1) <= 1e-13
    nel = ex * ey * ez
    assert np.array_equal(dg.cpu().numpy(), np.full(part.n_own_elems, 1.0 / nel))
    # without sums the slabs exchange their ghost planes and launch once: same dfdx, bit for bit
    d2 = grid.elem_vec()
    le.Response([slab(u) for u in U], [None if v is None else slab(v) for v in V], W, x, EMIN, EMAX, PENAL, VOLFRAC, d2, sums=False)
    assert torch.equal(d2, df)
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d response OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"response": response_mode})
