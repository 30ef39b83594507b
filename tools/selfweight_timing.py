#!/usr/bin/env python
"""Times the two self-weight entry points (tp_elasticity_body_load, tp_elasticity_body_sensitivity) against
tp_elasticity_objective -- the element pass whose pattern k_body_sens follows -- with and without its sums, in the same run.
HIP events around back-to-back repeats on the library's stream, warm-up first, median of several batches; beside every time the
bytes of the model and what fraction of the device-to-device copy rate, measured here too, that comes to.
Model: load 8 B per element + 24 B per node (48 with a base); sensitivity term 24 B per element (x, dfdx read and written) +
24 B per node per field + 24 B per node for N; tp_elasticity_objective 16 B per element + 24 B per node.
usage: selfweight_timing.py [ex ey ez [batches]] [> profiles/selfweight_timing.txt]     (default 128 128 128 7)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 7
REPS = 20
B, X_LOW = (0.0, 0.0, -1.0), 0.1


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


grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ey)
le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=4))
le.SetUpLoadAndBC()
le.SetBodyForce(B, X_LOW)
nel, nn = grid.n_own_elems, grid.n_local_nodes
x = grid.synth_density()
f, base, df, dg = grid.node_vec(3), grid.node_vec(3), grid.elem_vec(), grid.elem_vec()
U = [torch.rand(3 * nn, dtype=torch.float64, device=grid.device) - 0.5 for _ in range(tp.lib.MAX_CASES)]
le.U.copy_(U[0])
big = torch.empty(1 << 27, dtype=torch.float64, device=grid.device)     # 1 GiB: beyond the 256 MiB last-level cache
dst = torch.empty_like(big)
copy_ms = time_ms(lambda: dst.copy_(big))
copy_rate = 2 * big.numel() * 8 / (copy_ms[0] * 1e-3)
print("# %dx%dx%d elements, %d nodes, b = %s, x_low = %g; %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, nn, B, X_LOW, REPS, BATCHES))
print("# device-to-device copy of 1 GiB: %.4f ms, %.0f GB/s (read + write)" % (copy_ms[0], copy_rate / 1e9))
rows = [
    ("yardstick: tp_elasticity_objective, dfdx only (no sums, no host read)", 16 * nel + 24 * nn,
     lambda: le.L.tp_elasticity_sensitivities(le.handle, le.U.data_ptr(), x.data_ptr(), 1e-9, 1.0, 3.0, df.data_ptr(), None)),
    ("yardstick: tp_elasticity_objective with fx, gx (sums + host read)", 16 * nel + 24 * nn, lambda: le.Objective(x, 1e-9, 1.0, 3.0, 0.12, df)),
    ("tp_elasticity_body_load, no base", 8 * nel + 24 * nn, lambda: le.BodyLoad(x, f)),
    ("tp_elasticity_body_load, base + f", 8 * nel + 48 * nn, lambda: le.BodyLoad(x, f, base=base)),
    ("tp_elasticity_body_load, in place", 8 * nel + 48 * nn, lambda: le.BodyLoad(x, f, base=f)),
]
for ncase in (1, 2, tp.lib.MAX_CASES):
    rows.append(("tp_elasticity_body_sensitivity, %d field%s" % (ncase, "" if ncase == 1 else "s"), 24 * nel + 24 * nn * (ncase + 1),
                 lambda n=ncase: le.BodySensitivity(U[:n], None, x, 2.0, df)))
for name, nbytes, fn in rows:
    t = time_ms(fn)
    rate = nbytes / (t[0] * 1e-3)
    print("  %-72s %8.4f  (%.4f .. %.4f)   model %7.1f MB -> %6.0f GB/s = %.2f of the copy rate"
          % (name, t[0], t[1], t[2], nbytes / 1e6, rate / 1e9, rate / copy_rate), flush=True)
grid.close()
