"""Child processes of tests/test_gpu_casting_slabs.py, under torch.distributed.run, every rank on cuda:0.

usage: casting_worker.py slabs ex ey ez     z draws one- and two-sided (the parting plane on every slab border, one layer beside
                                            each and inside a slab), +x in both forms and -y: c, the stored q and the transpose of two
                                            vectors on the own layers equal the one-rank call on the whole field bit for bit; the
                                            one-rank result is held row by row (tests/design_rowwise.py), so the hand-over at the
                                            slab borders, t = 0.0 + (0.5 (1 - q)) mu, is"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import casting_ref as ref  # noqa: E402
from tests import design_rowwise as dr  # noqa: E402


def slab_draws(ez, world):
    own = ez // world
    ps = set()
    for b in range(own, ez, own):          # the borders, one layer beside them, the middle of the slab below
        ps |= {b, b - 1, b + 1, b - own // 2}
    return ["+z", "-z"] + ["z:%d" % p for p in sorted(ps) if 1 <= p <= ez - 1] + ["+x", "-y"]


def slabs_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ne = tuple(int(v) for v in sys.argv[2:5])
    h = 1.0 / ne[1]
    g1 = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h, rank=rank, nranks=world)
    es = grid.part.global_elem_slice()
    for draw in slab_draws(ne[2], world):
        x, g = ref.references(ne, draw, "random")[:2]
        for form in ((1, 0) if "x" in draw else (1,)):
            os.environ["TP_CASTING_XFORM"] = str(form)
            cf1, cf = tp.Casting(g1, draw), tp.Casting(grid, draw)
            c1, c = g1.elem_vec(), grid.elem_vec()
            cf1.Forward(ref.dev(x), c1)
            cf.Forward(ref.dev(x[es]), c)
            gv1, gv = [ref.dev(v) for v in g[:2]], [ref.dev(v[es]) for v in g[:2]]
            cf1.Adjoint(gv1)
            cf.Adjoint(gv)
            q1, q = cf1.Q(), cf.Q()
            same = [torch.equal(c, c1[es])] + [torch.equal(a, b[es]) for a, b in zip(gv, gv1)] + [torch.equal(q, q1[es])]
            print("rank %d %s form %d: c %s, transposes %s, q %s" % (rank, draw, cf.last_form(), same[0], same[1:3], same[3]), flush=True)
            assert all(same) and cf.last_form() == cf1.last_form() and float(gv1[0].abs().max()) > 0
            if rank == 0:      # what the slabs equal, row by row against the 80-bit restatement
                got = dr.cast_hold(dr.cast_case(ne, draw, "random"), c1.cpu().numpy(), q1.cpu().numpy(), [v.cpu().numpy() for v in gv1])
                print("rank 0 %s row-wise, achieved c: %s" % (draw, ", ".join("%s %.2f" % kv for kv in got.items())), flush=True)
            cf.close()
            cf1.close()
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d slabs OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"slabs": slabs_mode})
