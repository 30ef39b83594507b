#!/usr/bin/env python
"""Times the von Mises p-norm call (tp_elasticity_stress) and its parts against the one-case tp_elasticity_objective of the same
run -- the element pass does the same kind of arithmetic on the same bytes.  HIP events around back-to-back repeats on the
library's stream, warm-up first, median of several batches.  The rows differ in which outputs are asked for, i.e. in which
kernels run: vm alone is k_stress_elem<false> and nothing else; pnorm adds the block partials, the reduction and the host read;
dpdx adds k_stress_coef; adj_rhs adds k_stress_coef and k_stress_adjoint_rhs.  StressSensitivity is the whole sensitivity of
one design iteration: the full call, the adjoint solve, the bilinear response pass and the axpby -- timed from lam = 0 (the
ceiling) and warm-started from its own converged solution (the floor); a design iteration lies between the two.  Per-kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/stress_timing.py 128 128 128 2`.
usage: stress_timing.py [ex ey ez [batches]]      (default 128 128 128 7)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 7
REPS = 20
EMIN, EMAX, PENAL, Q, P = 1e-9, 1.0, 3.0, 0.5, 8.0

grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ey)
le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=4))
le.SetUpLoadAndBC()
x = grid.synth_density()
gen = torch.Generator(device="cuda").manual_seed(1)
U = torch.rand(grid.n_local_nodes * 3, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
le.U.copy_(U)   # (Objective and ComputeSensitivities read case 0's state)
vm, dpdx, adj, df = grid.elem_vec(), grid.elem_vec(), grid.node_vec(3), grid.elem_vec()


def time_ms(fn, reps=REPS):
    for _ in range(3):
        fn()
    out = []
    for _ in range(BATCHES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def objective_sums():
    le.Objective(x, EMIN, EMAX, PENAL, 0.12, df)


def objective_sens():
    le.ComputeSensitivities(df, None, x, EMIN, EMAX, PENAL)


rows = [
    ("tp_elasticity_stress: vm, pnorm, vm_max, dpdx, adj_rhs (the whole call)", lambda: le.Stress(x, EMAX, Q, P, U=U, vm=vm, dpdx=dpdx, adj_rhs=adj)),
    ("  vm alone (k_stress_elem<false>; no reduction, no host wait)", lambda: le.Stress(x, EMAX, Q, P, U=U, vm=vm)),
    ("  pnorm, vm_max (k_stress_elem<true>, reduction, host read)", lambda: le.Stress(x, EMAX, Q, P, U=U)),
    ("  pnorm, vm_max, dpdx (+ k_stress_coef)", lambda: le.Stress(x, EMAX, Q, P, U=U, dpdx=dpdx)),
    ("  pnorm, vm_max, adj_rhs (+ k_stress_coef, k_stress_adjoint_rhs)", lambda: le.Stress(x, EMAX, Q, P, U=U, adj_rhs=adj)),
    ("yardstick: one tp_elasticity_objective with sums (k_objective<true>)", objective_sums),
    ("yardstick: tp_elasticity_sensitivities (k_objective<false>, no host wait)", objective_sens),
]
print("# %dx%dx%d elements, q = %g, P = %g, %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, Q, P, REPS, BATCHES))
res = {}
for name, fn in rows:
    res[name] = time_ms(fn)
    print("%-78s %8.4f  (%.4f .. %.4f)" % ((name,) + res[name]), flush=True)
t = [res[r[0]][0] for r in rows]
print("by difference: k_stress_coef %.4f, k_stress_adjoint_rhs %.4f, reduction + host read %.4f ms"
      % (t[3] - t[2], t[4] - t[3], t[2] - t[1]))

# the whole sensitivity on a solved state: assemble and solve once, then repeat StressSensitivity (the adjoint warm-starts
# from the previous call's lam, as from the previous design iteration: these repeats are the converged-start floor; the first
# call from lam = 0 is printed separately)
le.U.zero_()
le.AssembleStiffnessMatrix(x, EMIN, EMAX, PENAL)
its_u = le.KSPSolve()
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
pn, mx, its = le.StressSensitivity(df, x, EMIN, EMAX, PENAL, Q, P)
b.record()
torch.cuda.synchronize()
print("StressSensitivity, first call (adjoint from lam = 0: %d iterations; the state solve took %d): %.3f ms; pnorm %.6e, max %.6e"
      % (its, its_u, a.elapsed_time(b), pn, mx), flush=True)
m, lo, hi = time_ms(lambda: le.StressSensitivity(df, x, EMIN, EMAX, PENAL, Q, P), reps=5)
print("%-78s %8.4f  (%.4f .. %.4f)   [%d adjoint iterations]" % ("StressSensitivity repeated (adjoint warm-started from its own solution)", m, lo, hi,
                                                                le.adjoint_its), flush=True)


def cold():
    le.lam.zero_()
    le.StressSensitivity(df, x, EMIN, EMAX, PENAL, Q, P)


m, lo, hi = time_ms(cold, reps=5)
print("%-78s %8.4f  (%.4f .. %.4f)   [%d adjoint iterations]" % ("StressSensitivity from lam = 0 every time (the ceiling of a design iteration)", m, lo, hi,
                                                                le.adjoint_its), flush=True)
grid.close()
