#!/usr/bin/env python
"""Times the fused weighted response of L load cases (tp_elasticity_response) against the form a user had before it: L calls
of tp_elasticity_objective combined with L - 1 tp_vec_axpby.  HIP events around back-to-back repeats on the library's stream,
warm-up first, median of several batches.  "with sums": every call ends in its host read of the sums, as in the design loop;
"sensitivities only": no reduction, no host synchronisation -- the kernels alone.
usage: loadcases_timing.py [ex ey ez [L]]      (default 128 128 128 3)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import topopt_in_petsc_amd as tp
from topopt_in_petsc_amd.api import _chk, _ptr

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
L = int(sys.argv[4]) if len(sys.argv) > 4 else 3
REPS, BATCHES = 20, 7
args = (1e-9, 1.0, 3.0, 0.12)

grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ey)
le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=4))
x = grid.synth_density()
gen = torch.Generator(device="cuda").manual_seed(1)
U = [torch.rand(grid.n_local_nodes * 3, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1 for _ in range(L)]
w = [0.5, 2.0, -1.0, 1.5, 0.25, 3.0, 1.0, 0.75][:L]
df, tmp = grid.elem_vec(), grid.elem_vec()
n = x.numel()


def fused(sums):
    le.Response(U, None, w, x, *args, df, None, sums=sums)


def separate(sums):
    for l in range(L):
        le.U = U[l]
        out = df if l == 0 else tmp
        if sums:
            le.Objective(x, *args, out)
        else:
            le.ComputeSensitivities(out, None, x, *args[:3])
        if l == 0:
            if w[0] != 1.0:
                _chk(grid.L.tp_vec_scale(grid.handle, _ptr(df), w[0], n), "tp_vec_scale")
        else:
            _chk(grid.L.tp_vec_axpby(grid.handle, _ptr(df), w[l], _ptr(tmp), 1.0, n), "tp_vec_axpby")


def single(sums):
    le.U = U[0]
    if sums:
        le.Objective(x, *args, df)
    else:
        le.ComputeSensitivities(df, None, x, *args[:3])


def time_ms(fn, sums):
    for _ in range(3):
        fn(sums)
    out = []
    for _ in range(BATCHES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(REPS):
            fn(sums)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / REPS)
    return statistics.median(out), min(out), max(out)


print("# %dx%dx%d elements, L = %d load cases, %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, L, REPS, BATCHES))
for sums, label in ((True, "with sums (fx, gx, f_case; one host read per call)"), (False, "sensitivities only (no reduction, no host wait)")):
    print("## " + label)
    for name, fn in (("fused tp_elasticity_response, L cases", fused),
                     ("L x tp_elasticity_objective + scale + (L-1) x tp_vec_axpby", separate),
                     ("one tp_elasticity_objective (single case; k_objective is unchanged)", single)):
        m, lo, hi = time_ms(fn, sums)
        print("%-72s %8.4f  (%.4f .. %.4f)" % (name, m, lo, hi), flush=True)
grid.close()
