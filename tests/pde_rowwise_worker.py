"""Worker of tests/test_gpu_pde_rowwise.py: the Helmholtz (PDE) filter's scalar hierarchy kernel by kernel.  The library latches
its switches once per process, so there is one process per form; it runs every mesh, regime and input of rw.PDE_CASES through
Filter.level_apply / level_dinv / smooth (one step; on the first rw.PDE_STEP_CASES cases also steps 2 and 3 of a sweep) / restrict / prolong_add / elem_to_node / node_to_elem, ASSERTS after every operator
call that the forced form is the one that launched (Filter.last_op_form) and dumps the outputs to one .npz (the inputs are
rw.pde_inputs on both sides); the parent compares them with the 80-bit arbiter.

usage: pde_rowwise_worker.py single <expect> <out.npz>             expect: "kind,a,b,c" as last_op_form returns them
       pde_rowwise_worker.py slab <case | -1> <outdir>             (under torch.distributed.run) this rank's slab of the case of
                                                                   rw.PDE_CASES (-1: rw.PDE_SLAB3), ghost planes of every
                                                                   input poisoned: level-0 product, Chebyshev steps, transfers,
                                                                   element <-> node; the OWNED parts to <outdir>/rank<k>.npz"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rowwise as rw  # noqa: E402

POPT = dict(rtol=1e-8, dtol=1e3, max_it=60, nsmooth=2, ncoarse=10)      # the reference's filter solver (PDEFilter.cc:280-357)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(form, expect, what):
    assert tuple(form) == tuple(int(v) for v in expect), "%s: form %s, expected %s: the forced kernel form did not run" % (what, form, expect)


def not_a_pde_filter(tp, grid, h):
    """every level entry point on a cone filter: an error code, not a dereference"""
    f = tp.Filter(grid, 1, 1.5 * min(h))
    v, e = grid.node_vec(1), grid.elem_vec()
    calls = [f.level_count, lambda: f.level_nodes(0), lambda: f.level_lambda(0), lambda: f.level_lambda_min(0), lambda: f.level_apply(0, v),
             lambda: f.level_dinv(0), lambda: f.smooth(0, v, v.clone(), 1), lambda: f.restrict(0, v), lambda: f.prolong_add(0, v, v.clone()),
             f.last_op_form, lambda: f.elem_to_node(e), lambda: f.node_to_elem(v)]
    for c in calls:
        try:
            c()
        except tp.TopOptError as err:
            assert err.code == 1, err
        else:
            raise AssertionError("a level entry point of the PDE filter accepted a cone filter")
    f.close()


def single(expect, res):
    import topopt_in_petsc_amd as tp
    tp.load_library()
    for m, case in enumerate(rw.PDE_CASES):
        (ex, ey, ez), _, nlv, ratios = case
        nx, ny, nz, h = ex + 1, ey + 1, ez + 1, rw.pde_box(case)
        for r, ratio in enumerate(ratios):
            grid = tp.Grid(nx, ny, nz, h)
            if m == 0 and r == 0:
                not_a_pde_filter(tp, grid, h)
            f = tp.Filter(grid, 2, ratio * min(h), tp.SolverOptions(nlvls=nlv, **POPT))
            tag = "m%d_r%d" % (m, r)
            res[tag + "_kf"] = f.KF()
            assert f.level_count() == nlv
            for l in range(nlv):
                dims = rw.level_dims(nx, ny, nz, l)
                assert f.level_nodes(l) == dims[0] * dims[1] * dims[2]
                inp = rw.pde_inputs(dims, rw.pde_seed(m, r, l))
                for name, u in inp.items():
                    if name == "b":
                        continue
                    y = f.level_apply(l, dev(u))
                    check(f.last_op_form(), expect, "%s level %d apply %s" % (tag, l, name))
                    res["%s_apply%d_%s" % (tag, l, name)] = host(y)
                    if l == 0 and name == "normal":          # level 0 of level_apply is tp_pdefilter_apply
                        y0 = torch.zeros_like(y)
                        f.PDEApply(dev(u), y0)
                        check(f.last_op_form(), expect, "%s PDEApply" % tag)
                        assert torch.equal(y, y0)
                u, b = inp["normal"], inp["b"]
                res["%s_dinv%d" % (tag, l)] = host(f.level_dinv(l))
                res["%s_lam%d" % (tag, l)] = np.asarray([f.level_lambda(l), f.level_lambda_min(l)])
                res["%s_cheb0_%d" % (tag, l)] = host(f.smooth(l, dev(b), torch.zeros_like(dev(b)), 1, True))
                res["%s_cheb1_%d" % (tag, l)] = host(f.smooth(l, dev(b), dev(u), 1, False))
                check(f.last_op_form(), expect, "%s level %d Chebyshev step" % (tag, l))
                if m < rw.PDE_STEP_CASES:       # steps 2, 3 of the sweeps from the zero guess and from u: the device's own iterates
                    for zero in (1, 0):
                        for j in range(1, max(rw.STEP_KS) + 1):
                            x0 = torch.zeros_like(dev(b)) if zero else dev(u)
                            res["%s_l%d_z%d_x%d" % (tag, l, zero, j)] = host(f.smooth(l, dev(b), x0, j, bool(zero)))
                    check(f.last_op_form(), expect, "%s level %d Chebyshev step %d" % (tag, l, max(rw.STEP_KS)))
                if l + 1 < nlv:
                    xc = rw.pde_inputs(rw.level_dims(nx, ny, nz, l + 1), rw.pde_seed(m, r, l + 1))
                    for name in rw.PDE_FIELDS:
                        res["%s_restrict%d_%s" % (tag, l, name)] = host(f.restrict(l, dev(inp[name])))
                        res["%s_prolong%d_%s" % (tag, l, name)] = host(f.prolong_add(l, dev(xc[name]), dev(b)))
            for name, (x, u) in rw.pde_t_inputs(m, ex * ey * ez, nx * ny * nz).items():
                res["%s_T_%s" % (tag, name)] = host(f.elem_to_node(dev(x)))
                res["%s_Tt_%s" % (tag, name)] = host(f.node_to_elem(dev(u)))
            f.close()
            grid.close()


def slab_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    m, outdir = int(sys.argv[2]), sys.argv[3]
    case = rw.PDE_CASES[m] if m >= 0 else rw.PDE_SLAB3
    (ex, ey, ez), _, nlv, ratios = case
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, rw.pde_box(case)
    r, ratio = ratios.index(2.56), 2.56
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    f = tp.Filter(grid, 2, ratio * min(h), tp.SolverOptions(nlvls=nlv, **POPT))
    res = {"kf": f.KF()}

    def slab(part, a):
        """this rank's local array of the global level vector a, its ghost planes poisoned: the library must refresh them"""
        t = a[part.global_slice(1)].copy()
        if part.has_lo:
            t[:part.plane] = 777.0
        if part.has_hi:
            t[-part.plane:] = -777.0
        return dev(t)

    for l in range(nlv):
        part = grid.part.level(l)
        own = part.owned_slice(1)
        assert f.level_nodes(l) == part.n_local_nodes
        inp = rw.pde_inputs((part.nx, part.ny, part.nz), rw.pde_seed(m, r, l))
        u, b = inp["normal"], inp["b"]
        if l == 0:
            for name, v in inp.items():
                if name == "b":
                    continue
                res["apply0_%s" % name] = host(f.level_apply(0, slab(part, v)))[own]
                check(f.last_op_form(), (3, 1, 0, 0), "rank %d apply %s" % (rank, name))
            res["dinv0"] = host(f.level_dinv(0))[own]
            res["lam0"] = np.asarray([f.level_lambda(0), f.level_lambda_min(0)])
            res["cheb0_0"] = host(f.smooth(0, slab(part, b), torch.zeros_like(slab(part, b)), 1, True))[own]
            res["cheb1_0"] = host(f.smooth(0, slab(part, b), slab(part, u), 1, False))[own]
            check(f.last_op_form(), (3, 1, 0, 0), "rank %d Chebyshev step" % rank)
        if l + 1 < nlv:
            cpart = grid.part.level(l + 1)
            xc = rw.pde_inputs((cpart.nx, cpart.ny, cpart.nz), rw.pde_seed(m, r, l + 1))
            for name in rw.PDE_FIELDS:
                res["restrict%d_%s" % (l, name)] = host(f.restrict(l, slab(part, inp[name])))[cpart.owned_slice(1)]
                res["prolong%d_%s" % (l, name)] = host(f.prolong_add(l, slab(cpart, xc[name]), slab(part, b)))[own]
    part = grid.part
    for name, (x, u) in rw.pde_t_inputs(m, ex * ey * ez, nx * ny * nz).items():
        res["T_%s" % name] = host(f.elem_to_node(dev(x[part.global_elem_slice()])))[part.owned_slice(1)]
        res["Tt_%s" % name] = host(f.node_to_elem(slab(part, u)))
    torch.cuda.synchronize()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **res)
    f.close()
    grid.close()
    print("rank %d slab OK" % rank, flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "slab":
        from tests.slab_launch import run_modes
        run_modes({"slab": slab_mode})
    else:
        out = {}
        single(sys.argv[2].split(","), out)
        np.savez(sys.argv[3], **out)
        print("pde rowwise worker OK")
