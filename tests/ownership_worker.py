"""Child processes of tests/test_gpu_ownership.py: who owns the library's device memory, read off tp_device_bytes_live().  A fresh
process, so that no object of another test moves the counter.

usage: ownership_worker.py one                  one process, cuda:0: every case of CASES in turn, each on a grid of its own.  Per case:
                                                the counter rises by at least the bytes of the object's main arrays (worked out from
                                                the mesh) while the object lives, is back at its value before the create after
                                                close(), and is 0 after Grid.close().  A case that fails prints its traceback and the
                                                next one runs; "case <name> OK" marks the ones that held.
       ownership_worker.py solve | body_load    under torch.distributed.run, every rank on cuda:0: the same sequence on every rank of
                                                a slab run -- cantilever, assembly and solve (the supports' exchange buffer, the ghost
                                                rows of the flagged elements' matrices, the replicated coarse level); one body load
                                                (the neighbour's layer of densities)"""
import os
import sys
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, H = 16, 1.0 / 16      # elements per direction of the one-process cases, element size
EMIN, EMAX, PENAL = 1e-9, 1.0, 3.0


def level_vector_bytes(ne, nlv, dof):
    """b, x, x2, r, d, dinv of every level of a one-rank hierarchy: 6 vectors of dof doubles per node"""
    return sum(6 * 8 * dof * (ne[0] // 2 ** l + 1) * (ne[1] // 2 ** l + 1) * (ne[2] // 2 ** l + 1) for l in range(nlv))


def owned(tp, grid, at_least, make, use):
    """create -> at least `at_least` bytes more -> use -> close -> the counter of before the create"""
    live = tp.device_bytes_live
    before = live()
    obj = make()
    held = live() - before
    assert held >= at_least, "the counter rose by %d bytes, the object's main arrays alone are %d" % (held, at_least)
    use(obj)
    torch.cuda.synchronize()
    assert live() - before >= held, "the counter fell while the object was alive"
    obj.close()
    assert live() == before, "%d bytes still counted after close()" % (live() - before)
    return held


def elasticity(tp, grid, nlv, supports=None, extras=False, **opts):
    def use(le):
        x = grid.elem_vec(0.5)
        if supports is None:
            le.SetUpLoadAndBC()
        else:   # the cantilever's line load; the face x = 0 clamped, then y = 0: the second call rebuilds the flagged-element lists
            R = torch.zeros(E + 1, E + 1, E + 1, 3, dtype=torch.float64)   # [z, y, x, component]
            R[0, :, E, 2] = -0.001
            R[0, 0, E, 2] = R[0, E, E, 2] = -0.0005
            for face in supports:
                N = torch.ones(E + 1, E + 1, E + 1, 3, dtype=torch.float64)
                if face == "x":
                    N[:, :, 0, :] = 0.0
                else:
                    N[:, 0, :, :] = 0.0
                le.SetBC(N.reshape(-1).cuda(), R.reshape(-1).cuda())
        le.SolveState(x, EMIN, EMAX, PENAL)
        assert le.last_its > 0
        if extras:   # d_resp, d_sx, d_VM and the body load's pass exist before the destroy
            dfdx, dgdx, dpdx, adj = grid.elem_vec(), grid.elem_vec(), grid.elem_vec(), grid.node_vec(3)
            le.Response([le.U], None, None, x, EMIN, EMAX, PENAL, 0.5, dfdx=dfdx, dgdx=dgdx)
            pn, _ = le.Stress(x, EMAX, 0.5, 8.0, dpdx=dpdx, adj_rhs=adj)
            assert pn > 0.0
            le.SetBodyForce((0.0, 0.0, -1.0))
            le.BodyLoad(x, grid.node_vec(3))
    o = tp.SolverOptions(nlvls=nlv, **opts)
    return owned(tp, grid, level_vector_bytes((E, E, E), nlv, 3), lambda: tp.LinearElasticity(grid, o), use)


def cone_filter(ftype):
    def case(tp, grid):
        def use(f):
            x = grid.synth_density()
            f.FilterProject(x, grid.elem_vec(), grid.elem_vec())
        return owned(tp, grid, 3 * 8 * E ** 3, lambda: tp.Filter(grid, ftype, 2.5 * H), use)   # Hs, tmp, and xg with its ghosts
    return case


def pde_filter(tp, grid):
    def use(f):
        x = grid.synth_density()
        f.FilterProject(x, grid.elem_vec(), grid.elem_vec())
    # three levels (the default of the PDE filter) of one unknown per node, and xe, rhs, u on the fine level
    return owned(tp, grid, level_vector_bytes((E, E, E), 3, 1) + 8 * (E ** 3 + 2 * (E + 1) ** 3), lambda: tp.Filter(grid, 2, 2.5 * H), use)


def localvol(tp, grid):
    def use(lv):
        g, pn, mx = lv.Constraint(grid.synth_density(), 0.6, 16.0, dgdx=grid.elem_vec())
        assert pn > 0.0
    return owned(tp, grid, 3 * 8 * E ** 3, lambda: tp.LocalVolume(grid, 2.5 * H), use)   # xg, cnt, rb


def overhang(tp, grid):
    live, before = tp.device_bytes_live, tp.device_bytes_live()

    def use(ov):
        ov.Forward(grid.synth_density(), grid.elem_vec())
        ov.Adjoint([grid.elem_vec(1.0), grid.elem_vec(2.0)])
        # the transpose's out-of-place target is made by its first call: one element field at the least, beside ca, cw, cp
        assert live() - before >= 4 * 8 * E ** 3, "no scratch counted after the transpose (%d bytes)" % (live() - before)
    return owned(tp, grid, 3 * 8 * E ** 3, lambda: tp.Overhang(grid, "+z"), use)


def mma(tp, grid):
    m, n = 2, E ** 3

    def use(opt):
        x = grid.elem_vec(0.5)
        xmin, xmax = grid.elem_vec(0.0), grid.elem_vec(1.0)
        opt.Update(x, grid.elem_vec(-1.0), [0.1, -0.1], [grid.elem_vec(1.0 / n), grid.elem_vec(-1.0 / n)], xmin, xmax)
    return owned(tp, grid, (8 + 2 * m) * 8 * n, lambda: tp.MMA(grid, grid.elem_vec(0.5), m=m), use)   # L .. xo2, pij, qij


def failed_create(tp, grid):
    """Filter(type 2) with ksp_mode 2 is TP_ERR_ARG: four times, and nothing stays behind"""
    before = tp.device_bytes_live()
    for k in range(4):
        try:
            tp.Filter(grid, 2, 2.5 * H, pde_opts=tp.SolverOptions(nlvls=3, ksp_mode=2))
            raise AssertionError("ksp_mode 2 was accepted")
        except tp.TopOptError as err:
            assert err.code == 1, err
        assert tp.device_bytes_live() == before, "refused create %d left %d bytes" % (k + 1, tp.device_bytes_live() - before)
    return 0


CASES = {
    "elasticity_cg": lambda tp, g: elasticity(tp, g, 4),
    "elasticity_coarse_direct": lambda tp, g: elasticity(tp, g, 4, coarse_direct=1),
    "elasticity_reference_solver": lambda tp, g: elasticity(tp, g, 4, ksp_mode=1),
    "elasticity_rebuilt_supports": lambda tp, g: elasticity(tp, g, 3, supports=("x", "y")),
    "elasticity_extras": lambda tp, g: elasticity(tp, g, 4, extras=True),
    "filter_0": cone_filter(0),
    "filter_1": cone_filter(1),
    "filter_2": pde_filter,
    "localvol": localvol,
    "overhang": overhang,
    "mma": mma,
    "failed_create": failed_create,
}

ALL_RETURNED = "all_returned"


def one_mode():
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    assert tp.device_bytes_live() == 0
    for name, case in CASES.items():
        grid, start = None, tp.device_bytes_live()
        try:
            grid = tp.Grid(E + 1, E + 1, E + 1, H)
            assert tp.device_bytes_live() > start, "the grid's own buffers are not counted"
            held = case(tp, grid)
            grid.close()
            assert tp.device_bytes_live() == start, "%d bytes still counted after Grid.close()" % (tp.device_bytes_live() - start)
            print("case %s OK (%d bytes held)" % (name, held), flush=True)
        except Exception:
            print("case %s FAILED\n%s" % (name, traceback.format_exc()), flush=True)
            if grid is not None:
                grid.close()
    left = tp.device_bytes_live()   # at the very end exactly 0 (a case that failed above may have left its object behind)
    print("case %s %s (%d bytes counted at the end)" % (ALL_RETURNED, "OK" if left == 0 else "FAILED", left), flush=True)


# ---- two slabs: 16 x 16 x 32 elements, three levels -> 4 element layers per rank on level 1, the last distributed one
SLAB_NE, SLAB_NLV = (16, 16, 32), 3


def slab_case(rank, world, extras):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ex, ey, ez = SLAB_NE
    assert tp.device_bytes_live() == 0
    grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ex, rank=rank, nranks=world)
    own = (ex, ey, ez // world)

    def use(le):
        x = grid.elem_vec(0.5)
        le.SetUpLoadAndBC()
        if extras:
            le.SetBodyForce((0.0, 0.0, -1.0))
            le.BodyLoad(x, grid.node_vec(3))
        else:
            le.SolveState(x, EMIN, EMAX, PENAL)
            assert le.last_its > 0
    # the own slab's level vectors (ghost planes and the replicated coarse level come on top)
    held = owned(tp, grid, level_vector_bytes(own, SLAB_NLV, 3), lambda: tp.LinearElasticity(grid, tp.SolverOptions(nlvls=SLAB_NLV)), use)
    grid.close()
    assert tp.device_bytes_live() == 0, "%d bytes still counted after Grid.close()" % tp.device_bytes_live()
    print("rank %d held %d bytes" % (rank, held), flush=True)


def solve_mode(rank, world):
    slab_case(rank, world, False)
    print("rank %d solve OK" % rank, flush=True)


def body_load_mode(rank, world):
    slab_case(rank, world, True)
    print("rank %d body_load OK" % rank, flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "one":
        one_mode()
    else:
        from tests.slab_launch import run_modes
        run_modes({"solve": solve_mode, "body_load": body_load_mode})
