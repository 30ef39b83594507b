"""Slab worker of tests/test_gpu_buckling_slabs.py (launched by torch.distributed.run; every rank shares cuda:0, gloo with host
staging).

usage: buckling_worker.py kernels <case>  geom_apply and geom_adjoint_rhs on the owned node planes and geom_sensitivity on the own
                                          element layers equal the one-rank call on the whole fields BIT FOR BIT (fixed-order
                                          gathers: no sum depends on the partition); the ghost planes of the outputs stay as they
                                          were; the state and the fields come with STALE ghost planes, which the calls must refresh
       buckling_worker.py modes <case>    BucklingModes on the slabs, on the restatement's state: eigenvalues within the bound of
                                          the one-rank test; a case with one multigrid level: BucklingModes refuses it (TP_ERR_ARG)
                                          before any launch
<case>: a key of tests/buckling_ref.py SLAB_CASES"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import buckling_ref as ref  # noqa: E402

W = [0.75, -0.5, 0.0]
EMAX_K = 2.5
LD = ref.LD


def _setup(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    c = ref.SLAB_CASES[sys.argv[2]]
    ne, h = c["ne"], c["h"]
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h, rank=rank, nranks=world)
    # (the solver's own tolerance: BucklingModes tightens it to tol / 10 for its solves; the Ritz values are Rayleigh quotients of
    # true products whatever the solves' accuracy)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=c["nlvls"], nu=ref.NU))
    le.SetUpLoadAndBC_Axial()
    return tp, c, grid, le


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def kernels_mode(rank, world):
    tp, c, grid, le = _setup(rank, world)
    ne, h = c["ne"], c["h"]
    x = ref.design_mixed(ne, c["seed"])
    g1 = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    le1 = tp.LinearElasticity(g1, tp.SolverOptions(nlvls=c["nlvls"], nu=ref.NU))
    le1.SetUpLoadAndBC_Axial()
    part = grid.part
    gs, es, own, pl = part.global_slice(3), part.global_elem_slice(), part.owned_slice(3), 3 * part.plane
    N = ref.clamp_N(ne)
    U = ref.smooth_field(ne, 50) * N
    V = [ref.smooth_field(ne, 60 + l) * N for l in range(3)]
    pre = np.random.default_rng(23).uniform(-1e-2, 1e-2, x.size)
    # the axial load itself: the slabs' pieces are the one-rank vector's
    assert torch.equal(le.RHS, le1.RHS[gs]) and abs(float(le1.RHS.sum()) + 1.0) < 1e-14

    def slab(a):
        t = a[gs].copy()
        if part.has_lo:
            t[:pl] = 777.0
        if part.has_hi:
            t[-pl:] = -777.0
        return dev(t)

    # ---- one rank
    le1.GeomAssemble(dev(x), EMAX_K, ref.PENAL, U=dev(U))
    y1 = [le1.GeomMult(dev(v)) for v in V]
    d1 = dev(pre)
    le1.GeomSensitivity([dev(v) for v in V], W, dev(x), dev(U), EMAX_K, ref.PENAL, -2.0, d1)
    r1 = g1.node_vec(3)
    le1.GeomAdjointRHS([dev(v) for v in V], W, dev(x), EMAX_K, ref.PENAL, -2.0, r1)
    # ---- this rank's slab
    xs, Us = dev(x[es]), slab(U)
    le.GeomAssemble(xs, EMAX_K, ref.PENAL, U=Us)
    fresh_u = torch.equal(Us.cpu(), torch.from_numpy(U[gs]))
    Vs = [slab(v) for v in V]
    ghosts = torch.ones(Vs[0].numel(), dtype=torch.bool, device="cuda")
    ghosts[own] = False
    same_y = kept = True
    for v, y_one in zip(Vs, y1):
        y = torch.full_like(v, 5.0)
        le.GeomMult(v, y)
        same_y = same_y and torch.equal(y[own], y_one[gs][own])
        kept = kept and bool((y[ghosts] == 5.0).all())
    fresh = all(torch.equal(v.cpu(), torch.from_numpy(u[gs])) for v, u in zip(Vs, V))
    Vs2, Us2 = [slab(v) for v in V], slab(U)
    d = dev(pre[es])
    le.GeomSensitivity(Vs2, W, xs, Us2, EMAX_K, ref.PENAL, -2.0, d)
    same_d = torch.equal(d, d1[es])
    fresh2 = all(torch.equal(v.cpu(), torch.from_numpy(u[gs])) for v, u in zip(Vs2, V)) and torch.equal(Us2.cpu(), torch.from_numpy(U[gs]))
    Vs3 = [slab(v) for v in V]
    r = torch.full_like(Vs3[0], 5.0)
    le.GeomAdjointRHS(Vs3, W, xs, EMAX_K, ref.PENAL, -2.0, r)
    same_r = torch.equal(r[own], r1[gs][own])
    kept_r = bool((r[ghosts] == 5.0).all())
    print("rank %d: geom_apply on %d owned planes bit-equal %s, ghost planes of y untouched %s (%d ghost values), geom_sensitivity "
          "bit-equal %s, geom_adjoint_rhs bit-equal %s (ghost planes untouched %s), ghost planes of the state and the fields refreshed "
          "%s / %s / %s" % (rank, Vs[0][own].numel() // pl, same_y, kept, int(ghosts.sum()), same_d, same_r, kept_r, fresh_u, fresh, fresh2),
          flush=True)
    assert same_y and kept and same_d and same_r and kept_r and fresh_u and fresh and fresh2
    assert float(y1[0].abs().max()) > 0 and not torch.equal(d1, dev(pre)) and float(r1.abs().max()) > 0
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d kernels OK" % rank, flush=True)


def modes_mode(rank, world):
    tp, c, grid, le = _setup(rank, world)
    ne, h, nev = c["ne"], c["h"], c["nev"]
    x = c["design"](ne, c["seed"])
    xs = dev(x[grid.part.global_elem_slice()])
    le.AssembleStiffnessMatrix(xs, ref.EMIN, ref.EMAX, ref.PENAL)
    if c["nlvls"] < 2:      # slabs of two layers allow one multigrid level only, and BucklingModes does not take that on several ranks
        try:
            le.BucklingModes(nev, xs, ref.EMAX, ref.PENAL, tol=1e-6)
            refused = None
        except tp.TopOptError as exc:
            refused = exc
        print("rank %d: one multigrid level on %d ranks: %s" % (rank, world, refused), flush=True)
        assert refused is not None and refused.code == 1 and le._buck is None
        torch.cuda.synchronize()
        grid.close()
        print("rank %d modes OK" % rank, flush=True)
        return
    from oracle import oracle as orc
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], ref.NU)).reshape(24, 24)      # the oracle's, not the restatement's own
    P = ref.Pencil(ne, h, x, ref.clamp_N(ne), ref.load_axial(ne), ref.EMIN, ref.EMAX, ref.PENAL, ref.NU, KE=KE)
    mu64, Phi, _ = P.modes(nev + 1)
    mu = P.refine(Phi)
    own = float(np.abs(ref.subspace_iteration(P, nev, tol=1e-8)[0][:nev] / mu64[:nev] - 1).max())
    bound = max(1e-10, 16 * own)
    out = le.BucklingModes(nev, xs, ref.EMAX, ref.PENAL, U=dev(P.u[grid.part.global_slice(3)]), tol=1e-6)
    rel = [float(LD(t) / m - 1) for t, m in zip(out["mu"], mu[:nev])]
    print("rank %d: mu %s in %d iterations (%d solver iterations); mu / mu_ref - 1 = %s (<= 1e-12, >= -%.1e; the restatement's "
          "own iteration is %.3e from eigh)" % (rank, " ".join("%.9e" % t for t in out["mu"]), out["iters"], out["ksp_its"],
                                                " ".join("%+.2e" % r for r in rel), bound, own), flush=True)
    assert max(out["residuals"]) <= 1e-6
    assert all(-bound <= r <= 1e-12 for r in rel), rel
    torch.cuda.synchronize()
    grid.close()
    print("rank %d modes OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"kernels": kernels_mode, "modes": modes_mode})
