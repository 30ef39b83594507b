"""Child processes of tests/test_gpu_link_slabs.py, under torch.distributed.run, every rank on cuda:0.

usage: link_worker.py maps ex ey ez     with y:mirror and with x:repeat:2 every orbit lies inside a slab: fold, expand and pick on the own
                                        slab, gathered in rank order, equal the one-rank call and tests/link_ref.py on the whole field
                                        BIT FOR BIT; the reduced counts of the ranks sum to the global count
       link_worker.py driver ex ey ez   three iterations of TopOpt(link=...) with y:mirror and with x:repeat:2 on the slabs against one
                                        rank: fx within 1e-12 (relative), the bound of tests/selfweight_worker.py; gx within 1e-13,
                                        that of tests/loadcases_worker.py; ch within rel 1e-7 (abs 1e-12), what the restart test of
                                        tests/test_mma.py allows; CG iteration counts equal
       link_worker.py zlink ex ey ez    a z link: ValueError on every rank with no device byte allocated"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import link_ref as lr  # noqa: E402

SPECS = {"y:mirror": (lr.NONE, lr.MIRROR, lr.NONE), "x:repeat:2": (lr.repeat(2), lr.NONE, lr.NONE)}


def _kw():
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    h = 1.0 / ey
    return dict(nxyz=(ex + 1, ey + 1, ez + 1), xc=(0.0, ex * h, 0.0, 1.0, 0.0, ez * h), nlvls=3, rmin=1.6 * h, volfrac=0.3)


def _all(obj, world):
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, obj)
    return parts


def maps_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ne = tuple(int(v) for v in sys.argv[2:5])
    n = ne[0] * ne[1] * ne[2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    g1 = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0)
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, 1.0, rank=rank, nranks=world)
    es = grid.part.global_elem_slice()
    for name, spec in SPECS.items():
        lk1, lk = tp.Link(g1, name), tp.Link(grid, name)
        nr = lr.reduced_counts(spec, ne)
        counts = _all(lk.n_reduced, world)
        assert sum(counts) == lk1.n_reduced == nr[0] * nr[1] * nr[2] and lk.nr == (nr[0], nr[1], ne[2] // world)
        rs = slice(sum(counts[:rank]), sum(counts[:rank + 1]))              # the own reduced variables in the global reduced vector
        fields = [lr.order_field(n, 3), lr.negative_zero_field(spec, ne, 5), lr.design_field(n, 7)]
        reds = [np.random.default_rng(9 + v).standard_normal(nr[0] * nr[1] * nr[2]) for v in range(3)]
        # one rank
        f1, r1, p1 = [lk1.reduced_vec() for _ in fields], [g1.elem_vec() for _ in reds], [lk1.reduced_vec() for _ in fields]
        lk1.Fold([dev(f) for f in fields], f1)
        lk1.Expand([dev(r) for r in reds], r1)
        lk1.Pick([dev(f) for f in fields], p1)
        # the slabs
        fs, xs, ps = [lk.reduced_vec() for _ in fields], [grid.elem_vec() for _ in reds], [lk.reduced_vec() for _ in fields]
        for form in (1, 2):
            lk.set_form(form)
            lk.Fold([dev(f[es]) for f in fields], fs)
            got = [np.concatenate(_all(t.cpu().numpy(), world)) for t in fs]
            for v, f in enumerate(fields):
                assert np.array_equal(bits(got[v]), bits(f1[v].cpu().numpy())) and np.array_equal(bits(got[v]), bits(lr.fold(spec, ne, f))), (name, form, v)
        lk.Expand([dev(r[rs]) for r in reds], xs)
        lk.Pick([dev(f[es]) for f in fields], ps)
        for v in range(3):
            full = np.concatenate(_all(xs[v].cpu().numpy(), world))
            assert np.array_equal(bits(full), bits(r1[v].cpu().numpy())) and np.array_equal(bits(full), bits(lr.expand(spec, ne, reds[v])))
            picked = np.concatenate(_all(ps[v].cpu().numpy(), world))
            assert np.array_equal(bits(picked), bits(p1[v].cpu().numpy())) and np.array_equal(bits(picked), bits(lr.pick(spec, ne, fields[v])))
        print("rank %d %s: own reduced %d of %d, fold / expand / pick equal one rank bit for bit" % (rank, name, lk.n_reduced, lk1.n_reduced), flush=True)
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d maps OK" % rank, flush=True)


def driver_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    kw = _kw()
    ne = tuple(n - 1 for n in kw["nxyz"])
    for name, spec in SPECS.items():
        one = tp.TopOpt(link=name, **kw)
        h1 = [one.step() for _ in range(3)]
        x1 = one.x.clone()
        one.grid.close()
        opt = tp.TopOpt(link=name, rank=rank, nranks=world, **kw)
        counts = _all(opt.linker.n_reduced, world)
        assert sum(counts) == opt.n_reduced == one.n_reduced and opt.xr.numel() == opt.linker.n_reduced
        hs = [opt.step() for _ in range(3)]
        es = opt.grid.part.global_elem_slice()
        for a, b in zip(h1, hs):
            print("rank %d %s itr %d: fx %.15e, one rank %.15e, off by %.3e (bound 1e-12); |gx - gx1| %.3e (bound 1e-13); |ch - ch1| %.3e (bound 1e-7 ch); "
                  "CG iterations %d / %d" % (rank, name, a["itr"], b["fx"], a["fx"], abs(b["fx"] / a["fx"] - 1), abs(b["gx"] - a["gx"]), abs(b["ch"] - a["ch"]),
                                            b["ksp_its"], a["ksp_its"]), flush=True)
        print("rank %d %s: max |x - x one rank| on the own slab %.3e" % (rank, name, float((opt.x - x1[es]).abs().max())), flush=True)
        for a, b in zip(h1, hs):
            assert abs(b["fx"] / a["fx"] - 1) <= 1e-12 and abs(b["gx"] - a["gx"]) <= 1e-13 and abs(b["ch"] - a["ch"]) <= max(1e-7 * abs(a["ch"]), 1e-12)
            assert b["ksp_its"] == a["ksp_its"] and b["n_reduced"] == a["n_reduced"]
        # x on the own slab is exactly linked: the expansion of its orbits' first members
        ne_own = (ne[0], ne[1], ne[2] // world)
        x = opt.x.cpu().numpy()
        assert np.array_equal(lr.expand(spec, ne_own, lr.pick(spec, ne_own, x)).view(np.int64), x.view(np.int64))
        torch.cuda.synchronize()
        opt.grid.close()
    print("rank %d driver OK" % rank, flush=True)


def zlink_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    kw = _kw()
    before = tp.device_bytes_live()
    for spec in ("z:mirror", "z:extrude", {"y": "mirror", "z": ("repeat", 2)}):
        try:
            tp.TopOpt(link=spec, rank=rank, nranks=world, **kw)
            raise AssertionError("a z link on %d ranks was accepted" % world)
        except ValueError as e:
            assert "z link" in str(e), e
    assert tp.device_bytes_live() == before == 0
    print("rank %d zlink OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"maps": maps_mode, "driver": driver_mode, "zlink": zlink_mode})
