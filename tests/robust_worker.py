"""Child processes of tests/test_gpu_robust_slabs.py, under torch.distributed.run, every rank on cuda:0.

usage: robust_worker.py kernels ex ey ez  Robust.Project (three fields, with labels and sums) and Robust.Chain (two rows, with labels) at
                                          beta = 4 and 48 on the slabs against one rank on the same global field: the own slice of every
                                          field and row bit for bit; the all-reduced sums within (n - 1) eps sum|v| of the 80-bit sum of
                                          the stored fields (the bound of tests/test_gpu_robust.py for any summation order) and within
                                          twice that of the one-rank sums
       robust_worker.py driver ex ey ez   three iterations of TopOpt(robust=(0.7, 0.5, 0.3), passive=...) on the slabs against one rank: fx
                                          within 1e-12 (relative) and gx within 1e-13 of the one-rank record, the bounds of
                                          tests/selfweight_worker.py and tests/loadcases_worker.py; equal CG iteration counts; the three
                                          all-reduced sums against the 80-bit sums of the stored fields of all ranks, as above.
                                          The run starts where every robust run starts, at the driver's default beta = 0.1, the first
                                          value of the continuation.  At beta = 4 the design the state is solved on, eroded at 0.7 from
                                          the uniform start, has a density of 0.04 - 0.07 beside the solid box (1) and the void sphere
                                          (0): its compliance is then not determined to 1e-12 by ANY float64 solve -- measured on these
                                          two meshes between one rank and the slabs, equal iteration counts throughout:
                                            TopOpt(robust=(0.7, 0.5, 0.3), beta=4)                fx off by 1.1e-11 / 4.5e-12 / 4.4e-13
                                            the same, states solved to rtol 1e-12                 5.4e-11 / 1.0e-12 / 6.2e-13
                                            TopOpt(projectionFilter=True, beta=4, eta=0.7),
                                              no robust code involved, the same eroded design     1.1e-11 / 2.2e-12 / 1.8e-13
                                            TopOpt() without projection                           9.4e-14 / 3.2e-13 / 1.4e-14
                                          (largest of the two meshes in iterations 1 / 2 / 3; in iteration 1 the designs are equal bit
                                          for bit, gx differs by 0).  The kernels at beta = 4 and 48 on slabs: mode `kernels`."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS = 2.0 ** -53
ETAS = (0.7, 0.5, 0.3)


def _kw():
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    h = 1.0 / ey
    return dict(nxyz=(ex + 1, ey + 1, ez + 1), xc=(0.0, ex * h, 0.0, 1.0, 0.0, ez * h), nlvls=3, rmin=1.6 * h, volfrac=0.3)


def _shapes(kw):
    """the solid box over the loaded edge (x = lx, z = 0), the void sphere in the middle: it crosses every slab border"""
    lx, lz = kw["xc"][1], kw["xc"][5]
    return [("solid", "box", (lx - 0.25, lx, 0.0, 1.0, 0.0, 0.25)), ("void", "sphere", (0.5 * lx, 0.5, 0.5 * lz, 0.3))]


def _exact_sums(fields, world):
    """the 80-bit sums of the ranks' stored fields over all ranks"""
    import torch.distributed as dist
    own = [float(f.cpu().numpy().astype(np.longdouble).sum()) for f in fields]
    parts = [None] * world
    dist.all_gather_object(parts, own)
    return [sum(p[k] for p in parts) for k in range(len(fields))]


def kernels_mode(rank, world):
    import topopt_in_petsc_amd as tp
    from topopt_in_petsc_amd.api import passive_labels
    torch.cuda.set_device(0)
    kw = _kw()
    (nx, ny, nz), h = kw["nxyz"], 1.0 / (kw["nxyz"][1] - 1)
    n = (nx - 1) * (ny - 1) * (nz - 1)
    labels = passive_labels(kw["nxyz"], kw["xc"], _shapes(kw))
    rng = np.random.default_rng(3)
    xT_h, rows_h = rng.uniform(0.0, 1.0, n), [rng.uniform(-1.0, 1.0, n) for _ in range(2)]
    xT_h[::7] = np.resize([0.0, 1.0, -0.0, 0.7, 0.5, 0.3], xT_h[::7].size)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bits = lambda t: t.view(torch.int64)
    g1 = tp.Grid(nx, ny, nz, h)
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    es = grid.part.global_elem_slice()
    rb1, rb, pr1, pr = tp.Robust(g1), tp.Robust(grid), tp.Passive(g1, labels), tp.Passive(grid, labels[es])
    assert pr1.n_void > 0 and pr1.n_solid > 0     # (a slab may hold none of them: it then takes the launch without labels)
    xT1, xT = dev(xT_h), dev(xT_h[es])
    for beta in (4.0, 48.0):
        f1, f = [g1.elem_vec(float("nan")) for _ in range(3)], [grid.elem_vec(float("nan")) for _ in range(3)]
        S1, S = rb1.Project(xT1, beta, ETAS, f1, passive=pr1), rb.Project(xT, beta, ETAS, f, passive=pr)
        exact = _exact_sums(f, world)
        for k in range(3):
            bound = (n - 1) * EPS * exact[k]     # the fields are non-negative: sum|v| is the sum
            print("rank %d beta %g field %d: all-reduced sum %.15e, one rank %.15e, 80-bit sum %.15e, off by %.3e (bound %.3e)"
                  % (rank, beta, k, S[k], S1[k], exact[k], abs(S[k] - exact[k]), bound), flush=True)
            assert torch.equal(bits(f[k]), bits(f1[k][es])), (beta, k)
            assert abs(S[k] - exact[k]) <= bound and abs(S[k] - S1[k]) <= 2 * bound
        r1, r = [dev(a) for a in rows_h], [dev(a[es]) for a in rows_h]
        rb1.Chain(xT1, beta, r1, [ETAS[0], ETAS[2]], passive=pr1)
        rb.Chain(xT, beta, r, [ETAS[0], ETAS[2]], passive=pr)
        for a, b in zip(r1, r):
            assert torch.equal(bits(b), bits(a[es])), beta
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d kernels OK" % rank, flush=True)


def driver_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    kw = dict(_kw(), projectionFilter=True, robust=ETAS)
    shapes = _shapes(kw)
    one = tp.TopOpt(passive=shapes, **kw)
    assert one.beta == 0.1
    S1, h1, x1 = [list(one._S)], [], None
    for _ in range(3):
        h1.append(one.step())
        S1.append(list(one._S))
    x1 = one.x.clone()
    one.grid.close()
    opt = tp.TopOpt(passive=shapes, rank=rank, nranks=world, **kw)
    n, hs = opt.grid.part.n_own_elems * world, []
    for it in range(4):     # the sums of the start design, then of the design every iteration leaves
        exact = _exact_sums((opt.xErode, opt.xPhys, opt.xDilate), world)
        for k, name in enumerate(("eroded", "nominal", "dilated")):
            bound = (n - 1) * EPS * exact[k]
            print("rank %d after iteration %d, %s: all-reduced sum %.15e, 80-bit sum %.15e, off by %.3e (bound %.3e); one rank %.15e"
                  % (rank, it, name, opt._S[k], exact[k], abs(opt._S[k] - exact[k]), bound, S1[it][k]), flush=True)
            assert abs(opt._S[k] - exact[k]) <= bound
            if it == 0:   # the same bytes on one rank and on the slabs: two summation orders of one field
                assert abs(opt._S[k] - S1[0][k]) <= 2 * bound
        if it < 3:
            hs.append(opt.step())
    es = opt.grid.part.global_elem_slice()
    for a, b in zip(h1, hs):
        print("rank %d itr %d: fx %.15e, one rank %.15e, off by %.3e (bound 1e-12); |gx - gx1| %.3e (bound 1e-13); CG iterations %d / %d; "
              "V_d* %.15e / %.15e" % (rank, a["itr"], b["fx"], a["fx"], abs(b["fx"] / a["fx"] - 1), abs(b["gx"] - a["gx"]), b["ksp_its"],
                                      a["ksp_its"], b["vol_dilated_target"], a["vol_dilated_target"]), flush=True)
    print("rank %d: max |x - x one rank| on the own slab %.3e" % (rank, float((opt.x - x1[es]).abs().max())), flush=True)
    for a, b in zip(h1, hs):
        assert abs(b["fx"] / a["fx"] - 1) <= 1e-12 and abs(b["gx"] - a["gx"]) <= 1e-13 and b["ksp_its"] == a["ksp_its"]
        assert b["vol_real"][0] < b["vol_real"][1] < b["vol_real"][2]
    lab = torch.from_numpy(np.array(opt.labels_own)).cuda()
    for f in (opt.xErode, opt.xPhys, opt.xDilate):
        assert bool((f[lab == 2] == 1.0).all()) and bool((f[lab == 1] == 0.0).all())
    torch.cuda.synchronize()
    opt.grid.close()
    print("rank %d driver OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"kernels": kernels_mode, "driver": driver_mode})
