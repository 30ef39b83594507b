"""Child processes of tests/test_gpu_passive_slabs.py, under torch.distributed.run, every rank on cuda:0.

usage: passive_worker.py driver ex ey ez      three iterations of TopOpt(passive=...) on the slabs against one rank: the packed counts of
                                              the ranks sum to the global count; fx within 1e-12 (relative) and gx within 1e-13 of the
                                              one-rank record, the bounds of tests/selfweight_worker.py and tests/loadcases_worker.py.
                                              No slab test holds ch; the one test that compares the ch of two runs of the driver,
                                              the restart test of tests/test_mma.py, allows rel 1e-7 (abs 1e-12), and so does this.
                                              (ch is the largest change of an entry of x; what x is off by shows one iteration later
                                              in fx, which is held to 1e-12.)
       passive_worker.py emptyrank ex ey ez   rank 0's slab entirely passive: ValueError on every rank before any device object"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _kw():
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    h = 1.0 / ey
    return dict(nxyz=(ex + 1, ey + 1, ez + 1), xc=(0.0, ex * h, 0.0, 1.0, 0.0, ez * h), nlvls=3, rmin=1.6 * h, volfrac=0.3)


def driver_mode(rank, world):
    import torch.distributed as dist
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    kw = _kw()
    lx, lz = kw["xc"][1], kw["xc"][5]
    # the solid box over the loaded edge (x = lx, z = 0), the void sphere in the middle
    shapes = [("solid", "box", (lx - 0.25, lx, 0.0, 1.0, 0.0, 0.25)), ("void", "sphere", (0.5 * lx, 0.5, 0.5 * lz, 0.3))]
    one = tp.TopOpt(passive=shapes, **kw)
    h1 = [one.step() for _ in range(3)]
    x1 = one.x.clone()
    one.grid.close()
    opt = tp.TopOpt(passive=shapes, rank=rank, nranks=world, **kw)
    counts = [None] * world
    dist.all_gather_object(counts, opt.regions.counts())
    print("rank %d: own (active, void, solid) %r; all ranks %r; global active %d" % (rank, opt.regions.counts(), counts, opt.n_active), flush=True)
    assert sum(c[0] for c in counts) == opt.n_active == one.n_active and opt.xa.numel() == opt.regions.n_active
    assert sum(c[1] for c in counts) > 0 and sum(c[2] for c in counts) > 0
    hs = [opt.step() for _ in range(3)]
    es = opt.grid.part.global_elem_slice()
    for a, b in zip(h1, hs):
        print("rank %d itr %d: fx %.15e, one rank %.15e, off by %.3e (bound 1e-12); |gx - gx1| %.3e (bound 1e-13); |ch - ch1| %.3e (bound 1e-7 ch); "
              "CG iterations %d / %d" % (rank, a["itr"], b["fx"], a["fx"], abs(b["fx"] / a["fx"] - 1), abs(b["gx"] - a["gx"]), abs(b["ch"] - a["ch"]),
                                        b["ksp_its"], a["ksp_its"]), flush=True)
    print("rank %d: max |x - x one rank| on the own slab %.3e" % (rank, float((opt.x - x1[es]).abs().max())), flush=True)
    for a, b in zip(h1, hs):
        assert abs(b["fx"] / a["fx"] - 1) <= 1e-12 and abs(b["gx"] - a["gx"]) <= 1e-13 and abs(b["ch"] - a["ch"]) <= max(1e-7 * abs(a["ch"]), 1e-12)
        assert b["n_active"] == a["n_active"]
    lab = torch.from_numpy(np.array(opt.labels_own)).cuda()
    assert bool((opt.xPhys[lab == 2] == 1.0).all()) and bool((opt.xPhys[lab == 1] == 0.0).all())
    torch.cuda.synchronize()
    opt.grid.close()
    print("rank %d driver OK" % rank, flush=True)


def emptyrank_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    kw = _kw()
    n = (kw["nxyz"][0] - 1) * (kw["nxyz"][1] - 1) * (kw["nxyz"][2] - 1)
    lab = np.zeros(n, dtype=np.uint8)
    lab[:n // world] = 1                     # the whole slab of rank 0 is void
    before = tp.device_bytes_live()
    try:
        tp.TopOpt(passive=lab, rank=rank, nranks=world, **kw)
        raise AssertionError("a slab without an active element was accepted")
    except ValueError as e:
        assert "rank 0" in str(e), e
    assert tp.device_bytes_live() == before == 0
    print("rank %d emptyrank OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"driver": driver_mode, "emptyrank": emptyrank_mode})
