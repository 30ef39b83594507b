#!/usr/bin/env python
"""Times the passive-region kernels (tp_passive) against the same work as one torch indexing call per vector: gather (v[idx]),
zero (v[mask] = 0) and scatter (v[idx] = p) with half the elements passive, nvec = 1 + m for m = 1 and m = 4 (the objective's row
and m constraint rows).  HIP events around back-to-back calls on the library's stream, warm-up first, median (min .. max) of several
batches.  The design iteration itself: tools/run_topopt.py 128 128 128 5 5 with and without --passive.
usage: passive_timing.py [ex ey ez [batches]] [> profiles/passive_timing.txt]   (default 128 128 128 5)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 5
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


h = 1.0 / ey
grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
n = ex * ey * ez
print("# %dx%dx%d elements, half of them passive, %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, REPS, BATCHES))
# two layouts of the same share: a solid half box (the active elements contiguous) and a random half (every line half used)
layouts = (("lower half of the box passive", (np.arange(n) < n // 2).astype(np.uint8) * 2),
           ("random half passive", np.random.default_rng(1).choice(np.array([0, 1, 2], dtype=np.uint8), size=n, p=[0.5, 0.25, 0.25])))
with torch.cuda.stream(torch.cuda.default_stream()):
    for name, lab_h in layouts:
        pr = tp.Passive(grid, lab_h)
        lab = torch.from_numpy(lab_h).cuda()
        idx, mask = torch.nonzero(lab == 0).flatten(), lab != 0
        print("%s: %d active of %d" % (name, pr.n_active, n))
        for m in (1, 4):
            full = [grid.synth_density(seed=7 + v) for v in range(1 + m)]
            packed = [pr.packed_vec() for _ in range(1 + m)]

            def torch_gather():
                for f, p in zip(full, packed):
                    torch.index_select(f, 0, idx, out=p)

            def torch_zero():
                for f in full:
                    f[mask] = 0.0

            def torch_scatter():
                for f, p in zip(full, packed):
                    f[idx] = p

            rows = [("tp_passive_gather", lambda: pr.Gather(full, packed), "torch index_select per vector", torch_gather),
                    ("tp_passive_zero", lambda: pr.Zero(full), "torch v[mask] = 0 per vector", torch_zero),
                    ("tp_passive_scatter", lambda: pr.Scatter(packed, full), "torch v[idx] = p per vector", torch_scatter)]
            for mine, fn, theirs, ref in rows:
                a, b = time_ms(fn), time_ms(ref)
                print("  nvec = 1 + %d  %-20s %8.4f  (%.4f .. %.4f)   %-30s %8.4f  (%.4f .. %.4f)   ratio %.2f"
                      % ((m, mine) + a + (theirs,) + b + (b[0] / a[0],)), flush=True)
            # the one launch for xPhys after every FilterProject
            a = time_ms(lambda: pr.Impose(full[:1], 0.0, 1.0))
            print("  nvec = 1      %-20s %8.4f  (%.4f .. %.4f)" % (("tp_passive_impose",) + a), flush=True)
        pr.close()
grid.close()
