"""Slab worker of tests/test_gpu_thermoelastic_slabs.py (launched by torch.distributed.run; every rank shares cuda:0, gloo with host
staging).

usage: thermoelastic_worker.py kernels <case> <design>   case: index into thermoelastic_ref.SLAB_CASES, design: mixed | binary
    - the thermal load and the adjoint right-hand side on the owned node planes and the sensitivity on the own element layers
      equal the one-rank call on the whole fields BIT FOR BIT (gathers and per-element sums in one fixed order, beta of the
      ghost layer from the neighbour's x: nothing depends on the partition); T and the fields come with STALE ghost planes, which
      the calls must refresh; the ghost planes of the outputs stay as they were;
       thermoelastic_worker.py driver <case>
    - one design iteration of TopOpt(physics="thermoelastic") from the mixed design: fx and dfdx against the direct-solve
      gradient of the whole mesh within the one-rank test's bound, max(100 delta, 1e-10) of its maximum."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels_mode(rank, world):
    import topopt_in_petsc_amd as tp
    from tests import conduction_ref as cr
    from tests import thermoelastic_ref as tr
    torch.cuda.set_device(0)
    ne, h, ranks = tr.SLAB_CASES[int(sys.argv[2])]
    kind = sys.argv[3]
    assert ranks == world
    nx, ny, nz = ne[0] + 1, ne[1] + 1, ne[2] + 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    p, x = tr.par(kind), cr.design(kind, *ne)
    N, R = tr.cantilever(ne, h)
    T, v0, v1, v2 = tr.fields(ne, 5)
    w = [0.75, -0.5, 1.25]
    base = cr.design("mixed", *ne, seed=3) - 0.5

    def build(grid, sl3):
        le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
        le.SetBC(dev(N[sl3]), dev(R[sl3]))
        le.SetThermalExpansion(p["alpha"], p["T_ref"], p["pb"], p["Emin"], p["Emax"])
        return le

    g1 = tp.Grid(nx, ny, nz, h)
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    part = grid.part
    gs1, gs3, es = part.global_slice(1), part.global_slice(3), part.global_elem_slice()
    own1, own3, pl = part.owned_slice(1), part.owned_slice(3), part.plane
    le1, le = build(g1, slice(None)), build(grid, gs3)

    def slab(a, dof):   # this rank's planes of a global nodal field, the ghost planes stale
        t = a[gs3 if dof == 3 else gs1].copy()
        if part.has_lo:
            t[:dof * pl] = 777.0
        if part.has_hi:
            t[-dof * pl:] = -777.0
        return dev(t)

    def ghosts_kept(out, dof, lo=55.0):
        ok = True
        if part.has_lo:
            ok = ok and bool((out[:dof * pl] == lo).all())
        if part.has_hi:
            ok = ok and bool((out[-dof * pl:] == lo).all())
        return ok

    # ---- one rank, whole fields
    X1, T1, V1 = dev(x), dev(T), [dev(v) for v in (v0, v1, v2)]
    f1 = le1.ThermalLoad(X1, T1, g1.node_vec(3), base=V1[1])
    a1 = le1.ThermalAdjointRHS(V1, w, X1, 1.5, g1.node_vec(1))
    d1 = dev(base)
    le1.ThermalSensitivity(V1, w, X1, T1, 2.0, d1)
    # ---- this slab, stale ghost planes everywhere
    Xs, Ts, Vs = dev(x[es]), slab(T, 1), [slab(v, 3) for v in (v0, v1, v2)]
    fs = le.ThermalLoad(Xs, Ts, grid.node_vec(3).fill_(55.0), base=dev(v1[gs3]))
    same_f, kept_f = torch.equal(fs[own3], f1[gs3][own3]), ghosts_kept(fs, 3)
    fresh_T = torch.equal(Ts.cpu(), torch.from_numpy(T[gs1]))
    Vs2 = [slab(v, 3) for v in (v0, v1, v2)]
    a_s = le.ThermalAdjointRHS(Vs2, w, Xs, 1.5, grid.node_vec(1).fill_(55.0))
    same_a, kept_a = torch.equal(a_s[own1], a1[gs1][own1]), ghosts_kept(a_s, 1)
    fresh_V = all(torch.equal(v.cpu(), torch.from_numpy(o[gs3])) for v, o in zip(Vs2, (v0, v1, v2)))
    ds = dev(base[es])
    le.ThermalSensitivity(Vs, w, Xs, slab(T, 1), 2.0, ds)
    same_d = torch.equal(ds, d1[es])
    print("rank %d %s %s: load bit-equal %s (ghost planes kept %s, T refreshed %s), adjoint rhs bit-equal %s (ghost planes kept %s, fields "
          "refreshed %s), sensitivity bit-equal %s" % (rank, kind, ne, same_f, kept_f, fresh_T, same_a, kept_a, fresh_V, same_d), flush=True)
    assert same_f and kept_f and fresh_T and same_a and kept_a and fresh_V and same_d
    torch.cuda.synchronize()
    for g in (grid, g1):
        g.close()
    print("rank %d kernels OK" % rank, flush=True)


def driver_mode(rank, world):
    import topopt_in_petsc_amd as tp
    from oracle import oracle as orc
    from tests import conduction_ref as cr
    from tests import thermoelastic_ref as tr
    torch.cuda.set_device(0)
    ne, h, ranks = tr.SLAB_CASES[int(sys.argv[2])]
    assert ranks == world
    hx, hy, hz = cr.h3(h)
    nlv = 3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    KE = np.asarray(orc.hex8_ke_box(hx, hy, hz, tr.NU))
    x = cr.design("mixed", *ne)
    unit = tr.Coupled(ne, h, KE, tr.par("mixed", alpha=1.0))
    s1 = unit.state(x)
    alpha = float(np.linalg.norm(unit.N * unit.F) / np.linalg.norm(unit.N * s1["f_th"]))
    cp = tr.Coupled(ne, h, KE, tr.par("mixed", alpha=alpha))
    s = cp.state(x)
    G = cp.gradient(x, s)
    opt = tp.TopOpt(nxyz=(ne[0] + 1, ne[1] + 1, ne[2] + 1), xc=(0, ne[0] * hx, 0, ne[1] * hy, 0, ne[2] * hz), nlvls=nlv, rmin=2.56 * hx, filter=1,
                    volfrac=0.3, physics="thermoelastic", alpha=alpha, T_ref=cp.p["T_ref"], Emin=cp.p["Emin"], kmin=cp.kmin,
                    solver=tp.SolverOptions(nlvls=nlv, rtol=1e-10, max_it=200), rank=rank, nranks=world)
    part = opt.grid.part
    gs1, gs3, es, own1, own3 = part.global_slice(1), part.global_slice(3), part.global_elem_slice(), part.owned_slice(1), part.owned_slice(3)
    opt.xPhys.copy_(dev(x[es]))
    fx, gx = opt._thermoelastic_step()
    host = lambda t: t.detach().cpu().numpy()
    rel = lambda a, b, top: float(np.abs(a - b).max() / np.abs(top).max())
    deltas = [rel(host(opt.physics.U)[own3], s["u"][gs3][own3], s["u"]), rel(host(opt.thermal.T)[own1], s["T"][gs1][own1], s["T"]),
              rel(host(opt.mu)[own1], G["mu"][gs1][own1], G["mu"])]
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, max(deltas))
    delta = max(parts)
    bound = max(100 * delta, 1e-10)
    d = rel(host(opt.dfdx), G["dc"][es], G["dc"])
    print("rank %d %s: fx %.15e, direct solves %.15e, off by %.3e; max|dfdx - gradient| / max|gradient| %.3e (bound %.3e, delta %.3e); "
          "iterations elastic %d, conduction %d, thermal adjoint %d" % (rank, ne, fx, s["c"], abs(fx / s["c"] - 1), d, bound, delta,
                                                                        opt.physics.last_its, opt._its_thermal, opt._its_thermal_adjoint), flush=True)
    assert d <= bound and abs(fx / s["c"] - 1) <= bound
    torch.cuda.synchronize()
    opt.grid.close()
    print("rank %d driver OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"kernels": kernels_mode, "driver": driver_mode})
