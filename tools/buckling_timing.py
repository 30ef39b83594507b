#!/usr/bin/env python
"""Times the passes of the buckling analysis (tp_elasticity_geom_assemble, tp_elasticity_geom_apply, tp_elasticity_geom_sensitivity
and tp_elasticity_geom_adjoint_rhs) against tp_elasticity_mass_apply, tp_elasticity_apply and a device-to-device copy in the same
run.  HIP events around back-to-back repeats on the library's stream, warm-up first, median of several batches; beside every time
the bytes of the model and what fraction of the copy rate, measured here too, that comes to.
Model: geom_assemble 24 B per node for U, 8 B per element for x, 224 B per element written; geom_apply 24 B read + 24 B written per
node, 24 B per node for N, 224 B per element; geom_sensitivity 16 B per element + 24 B per node for U, for N and per field;
geom_adjoint_rhs 8 B per element, 24 B per node for N, per field and for the result.
usage: buckling_timing.py [ex ey ez [batches [out.json]]]     (default 128 128 128 7 profiles/buckling_timing.json)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 7
REPS = 20


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
U = (torch.rand(3 * nn, dtype=torch.float64, device=grid.device) - 0.5) * le.N
X = [torch.rand(3 * nn, dtype=torch.float64, device=grid.device) - 0.5 for _ in range(3)]
le.GeomAssemble(x, 1.0, 3.0, U=U)
y, df = grid.node_vec(3), grid.elem_vec()

big = torch.empty(1 << 27, dtype=torch.float64, device=grid.device)     # 1 GiB: beyond the 256 MiB last-level cache
dst = torch.empty_like(big)
copy_ms = time_ms(lambda: dst.copy_(big))
copy_rate = 2 * big.numel() * 8 / (copy_ms[0] * 1e-3)
print("# %dx%dx%d elements, %d nodes; %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, nn, REPS, BATCHES))
print("# device-to-device copy of 1 GiB: %.4f ms, %.0f GB/s (read + write)" % (copy_ms[0], copy_rate / 1e9))
rows = [
    ("yardstick: tp_elasticity_apply", 48 * nn + 8 * nel, lambda: le.MatMult(X[0], y)),
    ("yardstick: tp_elasticity_mass_apply", 72 * nn + 8 * nel, lambda: le.MassMult(X[0], y)),
    ("tp_elasticity_geom_assemble", 24 * nn + 8 * nel + 224 * nel, lambda: le.GeomAssemble(x, 1.0, 3.0, U=U)),
    ("tp_elasticity_geom_apply", 72 * nn + 224 * nel, lambda: le.GeomMult(X[0], y)),
    ("tp_elasticity_geom_sensitivity, 1 field", 16 * nel + 24 * nn * 3, lambda: le.GeomSensitivity(X[:1], None, x, U, 1.0, 3.0, 1.0, df)),
    ("tp_elasticity_geom_sensitivity, 3 fields", 16 * nel + 24 * nn * 5, lambda: le.GeomSensitivity(X, None, x, U, 1.0, 3.0, 1.0, df)),
    ("tp_elasticity_geom_adjoint_rhs, 1 field", 16 * nel + 24 * nn * 3, lambda: le.GeomAdjointRHS(X[:1], None, x, 1.0, 3.0, 1.0, y)),
    ("tp_elasticity_geom_adjoint_rhs, 3 fields", 16 * nel + 24 * nn * 5, lambda: le.GeomAdjointRHS(X, None, x, 1.0, 3.0, 1.0, y)),
]
record = dict(mesh=[ex, ey, ez], nodes=nn, reps=REPS, batches=BATCHES, copy_ms=copy_ms[0], copy_GBps=copy_rate / 1e9, rows=[])
for name, nbytes, fn in rows:
    t = time_ms(fn)
    rate = nbytes / (t[0] * 1e-3)
    print("  %-72s %8.4f  (%.4f .. %.4f)   model %7.1f MB -> %6.0f GB/s = %.2f of the copy rate"
          % (name, t[0], t[1], t[2], nbytes / 1e6, rate / 1e9, rate / copy_rate), flush=True)
    record["rows"].append(dict(name=name, ms=t[0], ms_min=t[1], ms_max=t[2], model_MB=nbytes / 1e6, GBps=rate / 1e9,
                               of_copy_rate=rate / copy_rate))
out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "buckling_timing.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(record, f, indent=1)
grid.close()
