#!/usr/bin/env python
"""Times the passes of the eigen-solver (tp_elasticity_mass_apply, tp_vec_block_gram and tp_vec_block_combine at q = 5,
tp_elasticity_mass_sensitivity) against tp_elasticity_apply, q^2 calls of tp_vec_dot and a device-to-device copy in the same run.
HIP events around back-to-back repeats on the library's stream, warm-up first, median of several batches; beside every time the
bytes of the model and what fraction of the copy rate, measured here too, that comes to.
Model: mass_apply 24 B read + 24 B written per node, 24 B per node for N, 8 B per element; block_gram 2 q vector reads; block_combine
q reads + q writes; mass_sensitivity 24 B per element + 24 B per node per field + 24 B per node for N.  block_gram and tp_vec_dot end
with a host read each: their times include it.
usage: eigen_timing.py [ex ey ez [batches]] [> profiles/eigen_timing.txt]     (default 128 128 128 7)"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 7
REPS, Q = 20, 5


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
nel, nn = grid.n_own_elems, grid.n_local_nodes
x = grid.synth_density()
le.AssembleStiffnessMatrix(x, 1e-9, 1.0, 3.0)
le.MassAssemble(x, 1.0, 0.1)
X = [torch.rand(3 * nn, dtype=torch.float64, device=grid.device) - 0.5 for _ in range(Q)]
Y = [torch.rand(3 * nn, dtype=torch.float64, device=grid.device) - 0.5 for _ in range(Q)]
Z = [torch.empty_like(v) for v in X]
Qm = torch.rand(Q, Q, dtype=torch.float64).numpy()
y, df = grid.node_vec(3), grid.elem_vec()
one = C.c_double()


def dots():
    for a in X:
        for b in Y:
            grid.L.tp_vec_dot(grid.handle, a.data_ptr(), b.data_ptr(), a.numel(), C.byref(one))


big = torch.empty(1 << 27, dtype=torch.float64, device=grid.device)     # 1 GiB: beyond the 256 MiB last-level cache
dst = torch.empty_like(big)
copy_ms = time_ms(lambda: dst.copy_(big))
copy_rate = 2 * big.numel() * 8 / (copy_ms[0] * 1e-3)
print("# %dx%dx%d elements, %d nodes, q = %d; %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, nn, Q, REPS, BATCHES))
print("# device-to-device copy of 1 GiB: %.4f ms, %.0f GB/s (read + write)" % (copy_ms[0], copy_rate / 1e9))
rows = [
    ("yardstick: tp_elasticity_apply", 48 * nn + 8 * nel, lambda: le.MatMult(X[0], y)),
    ("tp_elasticity_mass_apply", 72 * nn + 8 * nel, lambda: le.MassMult(X[0], y)),
    ("yardstick: q^2 = %d calls of tp_vec_dot" % (Q * Q), 2 * Q * Q * 24 * nn, dots),
    ("tp_vec_block_gram, q = %d" % Q, 2 * Q * 24 * nn, lambda: grid.BlockGram(X, Y)),
    ("tp_vec_block_combine, q = %d" % Q, 2 * Q * 24 * nn, lambda: grid.BlockCombine(Y, Qm, Z)),
    ("tp_elasticity_mass_sensitivity, 3 fields", 24 * nel + 24 * nn * 4, lambda: le.MassSensitivity(X[:3], None, x, 1.0, df)),
]
for name, nbytes, fn in rows:
    t = time_ms(fn)
    rate = nbytes / (t[0] * 1e-3)
    print("  %-72s %8.4f  (%.4f .. %.4f)   model %7.1f MB -> %6.0f GB/s = %.2f of the copy rate"
          % (name, t[0], t[1], t[2], nbytes / 1e6, rate / 1e9, rate / copy_rate), flush=True)
grid.close()
