"""Slab worker of tests/test_gpu_selfweight_slabs.py (launched by torch.distributed.run; every rank shares cuda:0, gloo with host
staging).

usage: selfweight_worker.py kernels ex ey ez    the body load on the owned node planes and the sensitivity term on the own element
                                                layers equal the one-rank call on the whole fields BIT FOR BIT (a fixed-order
                                                gather and a per-element pass: no sum depends on the partition); the ghost planes
                                                of the load and the base array stay as they were; the fields come with STALE ghost
                                                planes, which the sensitivity call must refresh
       selfweight_worker.py driver ex ey ez     three driver iterations with a body force: fx of every iteration to 1e-12 relative
                                                and the CG iteration counts equal to the one-rank run's"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = (0.3, -0.7, 1.1)
W = [0.75, -0.5, 0.0]


def kernels_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, (0.05, 0.04, 0.03)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(23)
    V = [rng.uniform(-1.0, 1.0, 3 * nx * ny * nz) for _ in range(3)]
    x = rng.uniform(0.0, 1.0, ex * ey * ez)
    x[::2] *= 0.1                                           # half the elements in the damped range
    base = rng.uniform(-1e-4, 1e-4, 3 * nx * ny * nz)
    pre = rng.uniform(-1e-4, 1e-4, ex * ey * ez)
    g1 = tp.Grid(nx, ny, nz, h)
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    part = grid.part
    gs, es, own, pl = part.global_slice(3), part.global_elem_slice(), part.owned_slice(3), 3 * part.plane
    le1, le = tp.LinearElasticity(g1, tp.SolverOptions(nlvls=2)), tp.LinearElasticity(grid, tp.SolverOptions(nlvls=2))
    le1.SetUpLoadAndBC()
    le.SetUpLoadAndBC()

    def slab(a):
        t = a[gs].copy()
        if part.has_lo:
            t[:pl] = 777.0
        if part.has_hi:
            t[-pl:] = -777.0
        return dev(t)

    for x_low in (0.0, 0.1):
        le1.SetBodyForce(B, x_low)
        le.SetBodyForce(B, x_low)
        # ---- one rank
        f1, o1, d1 = g1.node_vec(3), g1.node_vec(3), dev(pre)
        le1.BodyLoad(dev(x), f1)
        le1.BodyLoad(dev(x), o1, base=dev(base))
        le1.BodySensitivity([dev(v) for v in V], W, dev(x), 2.0, d1)
        # ---- this rank's slab
        xs = dev(x[es])
        f, o, bs = slab(np.zeros_like(base)), slab(np.zeros_like(base)), slab(base)
        before, bs0 = f.clone(), bs.clone()
        le.BodyLoad(xs, f)
        le.BodyLoad(xs, o, base=bs)
        same_f = torch.equal(f[own], f1[gs][own]) and torch.equal(o[own], o1[gs][own])
        ghosts = torch.ones_like(f, dtype=torch.bool)
        ghosts[own] = False
        kept = torch.equal(f[ghosts], before[ghosts]) and torch.equal(o[ghosts], before[ghosts]) and torch.equal(bs, bs0)
        d = dev(pre[es])
        Vs = [slab(v) for v in V]
        le.BodySensitivity(Vs, W, xs, 2.0, d)
        same_d = torch.equal(d, d1[es])
        fresh = all(torch.equal(v.cpu(), torch.from_numpy(u[gs])) for v, u in zip(Vs, V))
        print("rank %d x_low %.1f: load on %d owned planes bit-equal %s, ghost planes and base untouched %s (%d ghost values), "
              "sensitivity term bit-equal %s, ghost planes of the fields refreshed %s"
              % (rank, x_low, f[own].numel() // pl, same_f, kept, int(ghosts.sum()), same_d, fresh), flush=True)
        assert same_f and kept and same_d and fresh
        assert float(f1.abs().max()) > 0 and not torch.equal(d1, dev(pre))
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d kernels OK" % rank, flush=True)


def driver_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    h = 1.0 / ey
    kw = dict(nxyz=(ex + 1, ey + 1, ez + 1), xc=(0.0, ex * h, 0.0, 1.0, 0.0, ez * h), nlvls=2, rmin=1.5 * h, volfrac=0.3,
              body_force=(0.0, 0.0, -0.05), body_force_xlow=0.35)
    one = tp.TopOpt(**kw)
    h1 = [one.step() for _ in range(3)]
    one.grid.close()
    opt = tp.TopOpt(rank=rank, nranks=world, **kw)
    hs = [opt.step() for _ in range(3)]
    for a, b in zip(h1, hs):
        err = abs(b["fx"] / a["fx"] - 1)
        print("rank %d itr %d: fx %.15e, one rank %.15e, off by %.3e (bound 1e-12); CG iterations %d / %d; body_share %.12f / %.12f"
              % (rank, a["itr"], b["fx"], a["fx"], err, b["ksp_its"], a["ksp_its"], b["body_share"], a["body_share"]), flush=True)
    for a, b in zip(h1, hs):
        assert abs(b["fx"] / a["fx"] - 1) <= 1e-12 and b["ksp_its"] == a["ksp_its"]
        assert abs(b["body_share"] - a["body_share"]) <= 1e-10 and 0.0 < b["body_share"] < 1.0
    torch.cuda.synchronize()
    opt.grid.close()
    print("rank %d driver OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"kernels": kernels_mode, "driver": driver_mode})
