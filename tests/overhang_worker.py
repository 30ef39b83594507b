"""Child processes of tests/test_gpu_overhang_slabs.py, under torch.distributed.run, every rank on cuda:0.

usage: overhang_worker.py slabs ex ey ez        +z and -z: xi, the stored a, w, p and the transpose of two vectors on the own layers
                                                equal the one-rank call on the whole field bit for bit, at chunk lengths 1 and 4;
                                                the one-rank result is held row by row (tests/design_rowwise.py), so the layers
                                                handed over at the slab borders are
       overhang_worker.py ybuild ex ey ez       a y build on more than one rank is TP_ERR_ARG from tp_overhang_create"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import design_rowwise as dr  # noqa: E402
from tests import overhang_ref as ref  # noqa: E402


def slabs_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ne = tuple(int(v) for v in sys.argv[2:5])
    h = 1.0 / ne[1]
    g1 = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h, rank=rank, nranks=world)
    es = grid.part.global_elem_slice()
    for build in ("+z", "-z"):
        x, g = ref.references(ne, build, "random")[:2]
        ov1, ov = tp.Overhang(g1, build), tp.Overhang(grid, build)
        for c in (1, 4):
            os.environ["TP_OVERHANG_CHUNK"] = str(c)
            xi1, xi = g1.elem_vec(), grid.elem_vec()
            ov1.Forward(ref.dev(x), xi1)
            ov.Forward(ref.dev(x[es]), xi)
            gv1, gv = [ref.dev(v) for v in g[:2]], [ref.dev(v[es]) for v in g[:2]]
            ov1.Adjoint(gv1)
            ov.Adjoint(gv)
            co1, co = ov1.Coefficients(), ov.Coefficients()
            same = [torch.equal(xi, xi1[es])] + [torch.equal(a, b[es]) for a, b in zip(gv, gv1)] + [torch.equal(a, b[es]) for a, b in zip(co, co1)]
            print("rank %d %s chunk %d: xi %s, transposes %s, a, w, p %s" % (rank, build, c, same[0], same[1:3], same[3:]), flush=True)
            assert all(same) and ov.last_chunk() == c and float(gv1[0].abs().max()) > 0
            if rank == 0 and c == 1:      # what the slabs equal, row by row against the 80-bit restatement
                got = dr.ov_hold(dr.ov_case(ne, build, "random", 0), xi1.cpu().numpy(), *[v.cpu().numpy() for v in co1], [v.cpu().numpy() for v in gv1])
                print("rank 0 %s row-wise, achieved c: %s" % (build, ", ".join("%s %.2f" % kv for kv in got.items())), flush=True)
        ov.close()
        ov1.close()
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d slabs OK" % rank, flush=True)


def ybuild_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ne = tuple(int(v) for v in sys.argv[2:5])
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0 / ne[1], rank=rank, nranks=world)
    for build in ("+y", "-y"):
        try:
            tp.Overhang(grid, build)
            raise AssertionError("a %s build on %d ranks was accepted" % (build, world))
        except tp.TopOptError as e:
            assert e.code == 1, e
    torch.cuda.synchronize()
    grid.close()
    print("rank %d ybuild OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"slabs": slabs_mode, "ybuild": ybuild_mode})
