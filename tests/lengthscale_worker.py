"""Child processes of tests/test_gpu_lengthscale_slabs.py, under torch.distributed.run, every rank on cuda:0.

usage: lengthscale_worker.py slabs ex ey ez       T, dg, S and g of both kinds (projection on) on the own layers equal the one-rank call
                                                 on the gathered field bit for bit
       lengthscale_worker.py thin ex ey ez        slabs of fewer than two layers are TP_ERR_ARG on every rank"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import lengthscale_ref as ref  # noqa: E402


def slabs_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ne = tuple(int(v) for v in sys.argv[2:5])
    hh = 1.0 / ne[1]
    h = (hh, hh, hh)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rt = ref.field("random", ne, h, seed=5)
    rb = ref.projected(rt, 1)
    g1 = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, hh)
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, hh, rank=rank, nranks=world)
    ls1, ls = tp.LengthScale(g1), tp.LengthScale(grid)
    es = grid.part.global_elem_slice()
    args = (ref.default_c(h), 0.75, 0.25, 1e-6, "both", True, ref.BETA, ref.ETA)
    dg1, dg = [g1.elem_vec(), g1.elem_vec()], [grid.elem_vec(), grid.elem_vec()]
    r1 = ls1.Constraints(dev(rt), dev(rb), *args, dg_solid=dg1[0], dg_void=dg1[1])
    T1 = ls1.Terms()
    r = ls.Constraints(dev(rt[es]), dev(rb[es]), *args, dg_solid=dg[0], dg_void=dg[1])
    T = ls.Terms()
    same = lambda a, b: "equal" if torch.equal(a, b[es]) else "DIFFERS"
    print("rank %d, %d own layers: T %s %s, dg %s %s; S %r %r (one rank %r %r); g %r %r (one rank %r %r)"
          % (rank, grid.part.n_own_elems // (ne[0] * ne[1]), same(T[0], T1[0]), same(T[1], T1[1]), same(dg[0], dg1[0]),
             same(dg[1], dg1[1]), r["S_solid"], r["S_void"], r1["S_solid"], r1["S_void"], r["g_solid"], r["g_void"], r1["g_solid"],
             r1["g_void"]), flush=True)
    assert all(torch.equal(a, b[es]) for a, b in zip(T + tuple(dg), T1 + tuple(dg1)))
    assert r == r1 and float(dg1[0].abs().max()) > 0 and float(dg1[1].abs().max()) > 0
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d slabs OK" % rank, flush=True)


def thin_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ne = tuple(int(v) for v in sys.argv[2:5])
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0 / ne[1], rank=rank, nranks=world)
    own = grid.part.n_own_elems // (ne[0] * ne[1])
    assert own < 2, "the case needs slabs of one layer"
    try:
        tp.LengthScale(grid)
        raise AssertionError("slabs of %d layer(s) were accepted" % own)
    except tp.TopOptError as e:
        assert e.code == 1, e
    torch.cuda.synchronize()
    grid.close()
    print("rank %d thin OK (%d own layer)" % (rank, own), flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"slabs": slabs_mode, "thin": thin_mode})
