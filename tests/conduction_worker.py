"""Slab worker of tests/test_gpu_conduction_slabs.py (launched by torch.distributed.run; every rank shares cuda:0, gloo with host
staging).

usage: conduction_worker.py slabs <case> <design>   case: index into conduction_ref.SLAB_CASES, design: mixed | binary
    - MatMult on the owned node planes and the response's dfdx on the own element layers equal the one-rank call on the whole
      fields BIT FOR BIT (per-node and per-element sums in a fixed order: nothing depends on the partition); the fields come with
      STALE ghost planes, which both calls must refresh;
    - the solve against the serial ORACLE on the whole mesh: iteration count equal, the residual history within the three bounds
      of test_solve_residual_history, the state within 1e-9;
    - the same solve on a grid created with TP_OVERLAP=0: the same history and state bit for bit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def slabs_mode(rank, world):
    import topopt_in_petsc_amd as tp
    from oracle import oracle as orc
    from tests import conduction_ref as cr
    torch.cuda.set_device(0)
    (ex, ey, ez), h, nlv, ranks = cr.SLAB_CASES[int(sys.argv[2])]
    kind = sys.argv[3]
    assert ranks == world
    nx, ny, nz = ex + 1, ey + 1, ez + 1
    kmin = cr.DESIGNS[kind]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    kt, x, N = cr.KT(h), cr.design(kind, ex, ey, ez), cr.sink_mask(nx, ny, nz)
    b = N * cr.load(nx, ny, nz, h)
    # ---- the oracle's solve on the whole mesh
    mg = orc.MG(nx, ny, nz, 1, nlv, nsmooth=cr.SOLVE["nsmooth"], ncoarse=cr.SOLVE["ncoarse"])
    mg.assemble(kt, cr.conductivity(x, kmin), N)
    To, its_o, hist_o = mg.solve(b, rtol=cr.SOLVE["rtol"], maxit=200)
    opts = lambda: tp.SolverOptions(nlvls=nlv, nsmooth=cr.SOLVE["nsmooth"], ncoarse=cr.SOLVE["ncoarse"], rtol=cr.SOLVE["rtol"], max_it=4 * its_o)

    def build(grid, sl_n, sl_e):
        hc = tp.HeatConduction(grid, opts())
        hc.SetBC(dev(N[sl_n]), dev(b[sl_n]))
        hc.AssembleConductivityMatrix(dev(x[sl_e]), kmin, cr.KMAX, cr.PENAL)
        return hc

    g1 = tp.Grid(nx, ny, nz, h)
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    part = grid.part
    gs, es, own, pl = part.global_slice(1), part.global_elem_slice(), part.owned_slice(1), part.plane
    hc1, hc = build(g1, slice(None), slice(None)), build(grid, gs, es)

    def slab(a):   # this rank's planes of a global nodal field, the ghost planes stale
        t = a[gs].copy()
        if part.has_lo:
            t[:pl] = 777.0
        if part.has_hi:
            t[-pl:] = -777.0
        return dev(t)

    # ---- product and sensitivities: the one-rank call's bits
    u, v = cr.inputs(nx * ny * nz, 60)
    y1 = hc1.MatMult(dev(u))
    us = slab(u)
    ys = hc.MatMult(us)
    same_y = torch.equal(ys[own], y1[gs][own])
    fresh = torch.equal(us.cpu(), torch.from_numpy(u[gs]))
    w = [0.75, -0.5, 0.0]
    d1, ds = g1.elem_vec(7.0), grid.elem_vec(7.0)
    f1 = hc1.Response([dev(u), dev(v), dev(v)], [dev(v), None, dev(u)], w, dev(x), kmin, cr.KMAX, cr.PENAL, 0.3, d1, None)
    U, V = slab(u), slab(v)
    fs = hc.Response([U, V, V], [V, None, U], w, dev(x[es]), kmin, cr.KMAX, cr.PENAL, 0.3, ds, None)
    same_d = torch.equal(ds, d1[es])
    print("rank %d %s %s: product on %d owned planes bit-equal %s, ghost planes refreshed %s, dfdx bit-equal %s; fx %.15e, one rank %.15e, gx %.3e / %.3e"
          % (rank, kind, (ex, ey, ez), ys[own].numel() // pl, same_y, fresh, same_d, fs[0], f1[0], fs[1], f1[1]), flush=True)
    assert same_y and fresh and same_d and hc.last_op_form()[:2] == (3, 2)
    # (the sums run over other workgroups and ranks: 1e-13 of the terms' majorants, the bound of tests/test_gpu_conduction.py)
    major = cr.response((nx, ny, nz), h, [u, v, v], [v, None, u], w, x, kmin)["f_major"]
    assert abs(fs[0] - f1[0]) <= 1e-13 * sum(abs(a) * m for a, m in zip(w, major)) and abs(fs[1] - f1[1]) <= 1e-15
    # ---- the solve against the oracle
    its = hc.KSPSolve(hist_cap=4 * its_o + 1)
    hh, bn = hc.last_hist, hc.last_bnorm
    d = np.abs(hh / hist_o - 1) if len(hh) == len(hist_o) else np.array([np.inf])
    big = hist_o > 1e-7 * bn
    rel = lambda a, c: np.abs(a - c).max() / np.abs(c).max()
    dT = rel(hc.T.cpu().numpy()[own], To[gs][own])
    print("rank %d %s %s: %d iterations (oracle %d); history: first ten %.3e (bound 1e-10), above 1e-7 |b| %.3e (1e-9), all %.3e (1e-6); "
          "state %.3e (1e-9); |b| off by %.3e (1e-14)" % (rank, kind, (ex, ey, ez), its, its_o, d[:10].max(), d[big].max() if big.any() else 0.0,
                                                          d.max(), dT, abs(bn / np.linalg.norm(b) - 1)), flush=True)
    assert its == its_o and d[:10].max() <= 1e-10 and d[big].max() <= 1e-9 and d.max() <= 1e-6 and dT <= 1e-9
    assert abs(bn / np.linalg.norm(b) - 1) <= 1e-14
    assert hc.KSPSolve() == 0
    # ---- blocking halos (a grid created with the overlap off): the same bits
    os.environ["TP_OVERLAP"] = "0"
    grid0 = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    os.environ.pop("TP_OVERLAP")
    hc0 = build(grid0, gs, es)
    hc.T.zero_()
    hc.KSPSolve(hist_cap=4 * its_o + 1)
    hc0.KSPSolve(hist_cap=4 * its_o + 1)
    print("rank %d %s %s: halos on the second stream %d (overlap off: %d); histories equal %s, states equal %s"
          % (rank, kind, (ex, ey, ez), grid.halo_overlap, grid0.halo_overlap, np.array_equal(hc0.last_hist, hc.last_hist), torch.equal(hc0.T[own], hc.T[own])), flush=True)
    assert grid0.halo_overlap == 0 and np.array_equal(hc0.last_hist, hc.last_hist) and torch.equal(hc0.T[own], hc.T[own])
    assert np.array_equal(hc.last_hist, hh)
    torch.cuda.synchronize()
    for g in (grid0, grid, g1):
        g.close()
    print("rank %d slabs OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"slabs": slabs_mode})
