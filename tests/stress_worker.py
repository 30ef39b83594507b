"""Slab worker of tests/test_gpu_stress_slabs.py (launched by torch.distributed.run; every rank shares cuda:0, gloo with host
staging): tp_elasticity_stress on z-slabs against the one-rank call on the gathered fields.

Every rank builds the same global state from one seed, takes its slab of it with STALE ghost planes (the call must refresh them),
and runs the one-rank call itself on a grid of its own: pnorm and vm_max to 1e-12, vm and dpdx of the own layers to 1e-12 and
1e-11 of their maxima, adj_rhs on the owned planes to 1e-11 of its maximum -- the check of the ghost element layer (its
coefficients come from the upper neighbour) and of the node gather at the slab border."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EMAX, Q, P = 1.0, 0.5, 8.0


def stress_mode(rank, world):
    import topopt_in_petsc_amd as tp
    torch.cuda.set_device(0)
    ex, ey, ez = [int(v) for v in sys.argv[2:5]]
    nx, ny, nz, h = ex + 1, ey + 1, ez + 1, 1.0 / ey
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    U = np.random.default_rng(9).uniform(-1.0, 1.0, 3 * nx * ny * nz)
    # ---- one rank, global fields
    g1 = tp.Grid(nx, ny, nz, h)
    le1 = tp.LinearElasticity(g1, tp.SolverOptions(nlvls=2))
    x1 = g1.synth_density()
    vm1, dp1, ad1 = g1.elem_vec(), g1.elem_vec(), g1.node_vec(3)
    pn1, mx1 = le1.Stress(x1, EMAX, Q, P, U=dev(U), vm=vm1, dpdx=dp1, adj_rhs=ad1)
    vm1, dp1, ad1 = vm1.cpu().numpy(), dp1.cpu().numpy(), ad1.cpu().numpy()
    # ---- this rank's slab
    grid = tp.Grid(nx, ny, nz, h, rank=rank, nranks=world)
    part = grid.part
    le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=2))
    gs, es, pl = part.global_slice(3), part.global_elem_slice(), 3 * part.plane
    Us = U[gs].copy()
    if part.has_lo:
        Us[:pl] = 777.0            # stale ghost planes: the call refreshes them
    if part.has_hi:
        Us[-pl:] = -777.0
    x = x1[es].clone()
    vm, dp, ad = grid.elem_vec(), grid.elem_vec(), grid.node_vec(3)
    pn, mx = le.Stress(x, EMAX, Q, P, U=dev(Us), vm=vm, dpdx=dp, adj_rhs=ad)
    own = part.owned_slice(3)
    ad_own, ad_ref = ad.cpu().numpy()[own], ad1[gs][own]
    e_pn, e_mx = abs(pn / pn1 - 1), abs(mx / mx1 - 1)
    e_vm = float(np.abs(vm.cpu().numpy() - vm1[es]).max() / np.abs(vm1).max())
    e_dp = float(np.abs(dp.cpu().numpy() - dp1[es]).max() / np.abs(dp1).max())
    e_ad = float(np.abs(ad_own - ad_ref).max() / np.abs(ad1).max())
    print("rank %d: pnorm %.3e, vm_max %.3e, vm %.3e (bounds 1e-12); dpdx %.3e, adj_rhs on %d owned planes %.3e (bounds 1e-11)"
          % (rank, e_pn, e_mx, e_vm, e_dp, ad_own.size // pl, e_ad), flush=True)
    assert e_pn <= 1e-12 and e_mx <= 1e-12 and e_vm <= 1e-12 and e_dp <= 1e-11 and e_ad <= 1e-11
    assert np.abs(ad_ref).max() > 0
    # the field alone: no reduction, the same bits
    vm2 = grid.elem_vec()
    assert le.Stress(x, EMAX, Q, P, U=dev(Us), vm=vm2) == (None, None)
    assert torch.equal(vm2, vm)
    torch.cuda.synchronize()
    grid.close()
    g1.close()
    print("rank %d stress OK" % rank, flush=True)


if __name__ == "__main__":
    from tests.slab_launch import run_modes
    run_modes({"stress": stress_mode})
