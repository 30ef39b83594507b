"""Child processes of tests/test_gpu_localvol.py and tests/test_gpu_localvol_slabs.py.

usage: localvol_worker.py kernel ex ey ez hx hy hz R k[,k...]       one process, cuda:0: every field and exponent of the GPU tests on
                                                                   one mesh against the numpy restatement, the ball sum having
                                                                   run one of the kernels k (the library latches its switches
                                                                   once per process: the parent sets them in the environment)
       localvol_worker.py slabs ex ey ez R/h                       under torch.distributed.run, every rank on cuda:0: cnt, rhobar
                                                                   and dgdx of the own layers equal the one-rank call on the
                                                                   gathered field bit for bit, g and pn to 64 * 2^-53; the one-rank
                                                                   rhobar and dgdx are held row by row (tests/design_rowwise.py)
       localvol_worker.py toowide ex ey ez R/h                     the same launch: a stencil wider than a slab is TP_ERR_ARG"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import design_rowwise as dr  # noqa: E402
from tests import localvol_ref as ref  # noqa: E402

ALPHA = 0.6


def kernel_mode():
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ne = tuple(int(v) for v in sys.argv[2:5])
    h = tuple(float(v) for v in sys.argv[5:8])
    R = float(sys.argv[8])
    expect = {int(v) for v in sys.argv[9].split(",")}
    worst = {}
    for kind in dr.LV_FIELDS:       # the fields of the GPU test and the 0/1 designs; the check holds every row (design_rowwise)
        for p in dr.LV_PS:
            got = ref.check_against_reference(tp, ne, h, R, kind, p, ALPHA, expect_kernel=expect)["rowwise"]
            worst[p] = [max(a, b) for a, b in zip(worst.get(p, (0.0, 0.0)), (got["rb"], got["dgdx"]))]
    print("row-wise over all fields, largest achieved c: " + "; ".join("p=%g rhobar %.2f, dgdx %.2f" % (p, *worst[p]) for p in dr.LV_PS), flush=True)
    print("kernel OK", flush=True)


def slabs_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    h = 1.0 / ey
    R = float(sys.argv[5]) * h
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rho = ref.field("random", (ex, ey, ez), seed=5)
    g1 = tp.Grid(nx, ny, nz, h)
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    lv1, lv = tp.LocalVolume(g1, R), tp.LocalVolume(grid, R)
    es = grid.part.global_elem_slice()
    assert lv.stencil_width == lv1.stencil_width == ref.stencil_width((ex, ey, ez), (h, h, h), R)
    assert torch.equal(lv.count(), lv1.count()[es])
    for p in (1.0, 16.0):
        rb1, dg1, rb, dg = g1.elem_vec(), g1.elem_vec(), grid.elem_vec(), grid.elem_vec()
        gv1, pn1, mx1 = lv1.Constraint(dev(rho), ALPHA, p, dgdx=dg1, rhobar=rb1)
        gv, pn, mx = lv.Constraint(dev(rho[es]), ALPHA, p, dgdx=dg, rhobar=rb)
        e_g, e_pn = abs(gv - gv1) / abs(gv1), abs(pn - pn1) / pn1
        print("rank %d p=%g conn %d of %d own layers: rhobar %s, dgdx %s, g %.3e, pn %.3e (bound %.3e), rhobar_max %s"
              % (rank, p, lv.stencil_width, grid.part.n_own_elems // (ex * ey), "equal" if torch.equal(rb, rb1[es]) else "DIFFERS",
                 "equal" if torch.equal(dg, dg1[es]) else "DIFFERS", e_g, e_pn, 64 * ref.U53, "equal" if mx == mx1 else "DIFFERS"),
              flush=True)
        assert torch.equal(rb, rb1[es]) and torch.equal(dg, dg1[es]) and float(dg1.abs().max()) > 0
        if rank == 0:      # what the slabs equal, row by row against the 80-bit restatement, each row relative to itself
            conn = lv1.stencil_width
            case = dict(ne=(ex, ey, ez), ref=ref.reference(rho, (ex, ey, ez), (h, h, h), R, ALPHA, p), c=dr.c_lv(conn, p),
                        label="local volume %dx%dx%d random (seed 5) p=%g conn %d, one rank" % (ex, ey, ez, p, conn))
            got = dr.lv_hold(case, rb1.cpu().numpy(), dg1.cpu().numpy())
            print("rank 0 p=%g row-wise, achieved c (bound): rhobar %.2f (%g), dgdx %.2f (%g)" % (p, got["rb"], case["c"][0], got["dgdx"], case["c"][1]), flush=True)
        assert e_g <= 64 * ref.U53 and e_pn <= 64 * ref.U53 and mx == mx1
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d slabs OK" % rank, flush=True)


def toowide_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    h = 1.0 / ey
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, h, rank=rank, nranks=world)
    conn, own = ref.stencil_width((ex, ey, ez), (h, h, h), float(sys.argv[5]) * h), grid.part.n_own_elems // (ex * ey)
    assert conn > own, "the case needs a stencil wider than a slab"
    try:
        tp.LocalVolume(grid, float(sys.argv[5]) * h)
        raise AssertionError("a stencil of %d layers on slabs of %d was accepted" % (conn, own))
    except tp.TopOptError as e:
        assert e.code == 1, e
    torch.cuda.synchronize()
    grid.close()
    print("rank %d toowide OK (conn %d, %d own layers)" % (rank, conn, own), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel_mode()
    else:
        from tests.slab_launch import run_modes
        run_modes({"slabs": slabs_mode, "toowide": toowide_mode})
