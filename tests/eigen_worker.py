"""Slab worker of tests/test_gpu_eigen_slabs.py (launched by torch.distributed.run; every rank shares cuda:0, gloo with host
staging).

usage: eigen_worker.py kernels <case>    mass_apply on the owned node planes and mass_sensitivity on the own element layers equal
                                         the one-rank call on the whole fields BIT FOR BIT (fixed-order gathers: no sum depends
                                         on the partition); the ghost planes of y stay as they were; the fields come with STALE
                                         ghost planes, which both calls must refresh; block_gram over the owned ranges of all
                                         ranks against 80-bit sums at 1e-13; block_combine carries the ghost planes along
       eigen_worker.py modes <case>      Eigenmodes at tol 1e-8 on the slabs: eigenvalues within the bound of the one-rank test
                                         of the reference (eigh's values refined in 80-bit arithmetic), upper bounds to 1e-12;
                                         a case with one multigrid level: Eigenmodes refuses it (TP_ERR_ARG) before any launch
<case>: a key of tests/eigen_ref.py SLAB_CASES"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import eigen_ref as ref  # noqa: E402

W = [0.75, -0.5, 0.0]
RHO0 = 2.5
LD = ref.LD


def _setup(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    c = ref.SLAB_CASES[sys.argv[2]]
    ne, h = c["ne"], c["h"]
    grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h, rank=rank, nranks=world)
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=c["nlvls"], nu=0.3))
    le.SetUpLoadAndBC()
    return tp, c, grid, le, c["design"](ne, c["seed"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def kernels_mode(rank, world):
    tp, c, grid, le, x = _setup(rank, world)
    ne, h = c["ne"], c["h"]
    nn = 3 * (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
    g1 = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
    le1 = tp.LinearElasticity(g1, tp.SolverOptions(nlvls=c["nlvls"], nu=0.3))
    le1.SetUpLoadAndBC()
    part = grid.part
    gs, es, own, pl = part.global_slice(3), part.global_elem_slice(), part.owned_slice(3), 3 * part.plane
    rng = np.random.default_rng(23)
    V = [rng.uniform(-1.0, 1.0, nn) for _ in range(3)]
    pre = rng.uniform(-1e-4, 1e-4, x.size)

    def slab(a):
        t = a[gs].copy()
        if part.has_lo:
            t[:pl] = 777.0
        if part.has_hi:
            t[-pl:] = -777.0
        return dev(t)

    # ---- one rank
    le1.MassAssemble(dev(x), RHO0, ref.X_LOW)
    y1 = [le1.MassMult(dev(v)) for v in V]
    d1 = dev(pre)
    le1.MassSensitivity([dev(v) for v in V], W, dev(x), -2.0, d1)
    # ---- this rank's slab
    xs = dev(x[es])
    le.MassAssemble(xs, RHO0, ref.X_LOW)
    Vs = [slab(v) for v in V]
    ghosts = torch.ones(Vs[0].numel(), dtype=torch.bool, device="cuda")
    ghosts[own] = False
    same_y = kept = True
    for v, y_one in zip(Vs, y1):
        y = torch.full_like(v, 5.0)
        le.MassMult(v, y)
        same_y = same_y and torch.equal(y[own], y_one[gs][own])
        kept = kept and bool((y[ghosts] == 5.0).all())
    fresh = all(torch.equal(v.cpu(), torch.from_numpy(u[gs])) for v, u in zip(Vs, V))
    Vs2 = [slab(v) for v in V]
    d = dev(pre[es])
    le.MassSensitivity(Vs2, W, xs, -2.0, d)
    same_d = torch.equal(d, d1[es])
    fresh2 = all(torch.equal(v.cpu(), torch.from_numpy(u[gs])) for v, u in zip(Vs2, V))
    print("rank %d: mass_apply on %d owned planes bit-equal %s, ghost planes of y untouched %s (%d ghost values), mass_sensitivity "
          "bit-equal %s, ghost planes of the fields refreshed %s / %s"
          % (rank, Vs[0][own].numel() // pl, same_y, kept, int(ghosts.sum()), same_d, fresh, fresh2), flush=True)
    assert same_y and kept and same_d and fresh and fresh2
    assert float(y1[0].abs().max()) > 0 and not torch.equal(d1, dev(pre))
    # ---- block_gram over the owned ranges of all ranks; positive vectors, so sum |x y| is the dot product
    P = [rng.uniform(0.25, 1.25, nn) for _ in range(6)]
    Ps = [dev(p[gs]) for p in P]
    G = grid.BlockGram([p[own] for p in Ps[:3]], [p[own] for p in Ps[3:]])
    Gr = np.array([[P[i].astype(LD) @ P[3 + j].astype(LD) for j in range(3)] for i in range(3)])
    err = float(np.abs(G / Gr - 1).max())
    print("rank %d: block_gram over all ranks max|G / G_ref - 1| = %.3e (bound 1e-13)" % (rank, err), flush=True)
    assert err <= 1e-13
    # ---- block_combine on the whole local arrays: the ghost planes come along
    Q = rng.uniform(-1.0, 1.0, (3, 3))
    Z = [torch.zeros_like(p) for p in Ps[:3]]
    grid.BlockCombine(Ps[:3], Q, Z)
    Zr = np.stack([p[gs] for p in P[:3]], axis=1).astype(LD) @ Q.astype(LD)
    mag = np.abs(np.stack([p[gs] for p in P[:3]], axis=1)).astype(LD) @ np.abs(Q).astype(LD)
    cerr = max(float((np.abs(Z[i].cpu().numpy() - Zr[:, i]) / mag[:, i]).max()) for i in range(3))
    print("rank %d: block_combine incl. ghost planes %.3e (bound %.1e)" % (rank, cerr, 64 * 2.0 ** -53), flush=True)
    assert cerr <= 64 * 2.0 ** -53
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d kernels OK" % rank, flush=True)


def modes_mode(rank, world):
    tp, c, grid, le, x = _setup(rank, world)
    ne, h, nev = c["ne"], c["h"], c["nev"]
    xs = dev(x[grid.part.global_elem_slice()])
    le.AssembleStiffnessMatrix(xs, ref.EMIN, ref.EMAX, ref.PENAL)
    if c["nlvls"] < 2:      # slabs of two layers allow one multigrid level only, and Eigenmodes does not take that on several ranks
        try:
            le.Eigenmodes(nev, xs, ref.RHO0, ref.X_LOW, tol=1e-8)
            refused = None
        except tp.TopOptError as exc:
            refused = exc
        print("rank %d: one multigrid level on %d ranks: %s" % (rank, world, refused), flush=True)
        assert refused is not None and refused.code == 1 and le._eig is None
        torch.cuda.synchronize()
        grid.close()
        print("rank %d modes OK" % rank, flush=True)
        return
    out = le.Eigenmodes(nev, xs, ref.RHO0, ref.X_LOW, tol=1e-8)
    from oracle import oracle as orc
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], 0.3)).reshape(24, 24)      # the oracle's, not the object's own
    P = ref.Pencil(ne, h, KE, x, ref.cantilever_N(*ne), ref.EMIN, ref.EMAX, ref.PENAL, ref.RHO0, ref.X_LOW)
    lam64, Phi = P.eigh(nev + 1)
    lam = P.refine(lam64, Phi)
    own = float(np.abs(P.subspace(nev, tol=1e-8)[0][:nev] / lam64[:nev] - 1).max())
    bound = max(1e-10, 16 * own)
    rel = [float(LD(t) / l - 1) for t, l in zip(out["lam"], lam[:nev])]
    print("rank %d: theta %s in %d iterations (%d solver iterations); theta / lambda - 1 = %s (>= -1e-12, <= %.1e; the restatement's "
          "own iteration is %.3e from eigh)" % (rank, " ".join("%.9e" % t for t in out["lam"]), out["iters"], out["ksp_its"],
                                                " ".join("%+.2e" % r for r in rel), bound, own), flush=True)
    assert max(out["residuals"]) <= 1e-8
    assert all(-1e-12 <= r <= bound for r in rel), rel
    torch.cuda.synchronize()
    grid.close()
    print("rank %d modes OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"kernels": kernels_mode, "modes": modes_mode})
