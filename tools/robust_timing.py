#!/usr/bin/env python
"""Times the two robust-design kernels (tp_robust_project, tp_robust_chain) against the launches they replace, half the elements
passive at random.
  Project, three fields:  three Filter.FilterProject projections (a sensitivity filter whose x and xTilde are one tensor: the
                          projection kernel alone runs), Passive.Impose on the three fields, and three torch.sum calls read by the
                          host in one copy -- against Project(sums=True); the same without the sums against Project(sums=False)
  Chain, two rows:        the two k_heaviside_chain launches of Filter.Gradients and Passive.Zero.  The two launches cannot be
                          called alone: they are timed as Gradients(projectionFilter=True) minus Gradients(projectionFilter=False)
                          of a sensitivity filter, whose own part is the same in both
HIP events around back-to-back calls on the library's stream, warm-up first, median (min .. max) of several batches.  The design
iteration itself: tools/run_topopt.py 128 64 64 4 20 with and without --robust 0.7,0.5,0.3.
usage: robust_timing.py [ex ey ez [batches]] [> profiles/robust_timing.txt]   (default 128 128 128 5)"""
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
ETAS, BETA = (0.7, 0.5, 0.3), 8.0


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


def row(mine, a, theirs, b):
    print("  %-34s %8.4f  (%.4f .. %.4f)   %-58s %8.4f  (%.4f .. %.4f)   ratio %.2f" % ((mine,) + a + (theirs,) + b + (b[0] / a[0],)), flush=True)


h = 1.0 / ey
grid = tp.Grid(ex + 1, ey + 1, ez + 1, h)
n = ex * ey * ez
print("# %dx%dx%d elements, beta %g, thresholds %s, %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, BETA, ETAS, REPS, BATCHES))
with torch.cuda.stream(torch.cuda.default_stream()):
    flt0, rb = tp.Filter(grid, 0, 0.5 * h), tp.Robust(grid)
    xT = grid.synth_density(seed=7)
    fields = [grid.elem_vec() for _ in range(3)]
    rows = [grid.synth_density(seed=11), grid.synth_density(seed=12)]
    lab_h = np.random.default_rng(1).choice(np.array([0, 1, 2], dtype=np.uint8), size=n, p=[0.5, 0.25, 0.25])
    for name, pr in (("no passive element", None), ("random half passive", tp.Passive(grid, lab_h))):
        print("%s" % name)

        def parts(sums):
            for f, eta in zip(fields, ETAS):
                flt0.FilterProject(xT, xT, f, True, BETA, eta)
            if pr is not None:
                pr.Impose(fields, 0.0, 1.0)
            if sums:
                return torch.stack([torch.sum(f) for f in fields]).tolist()

        seq = "3 projections%s" % (" + Impose" if pr is not None else "")
        row("Project, 3 fields, sums", time_ms(lambda: rb.Project(xT, BETA, ETAS, fields, passive=pr)),
            seq + " + 3 torch.sum, one host read", time_ms(lambda: parts(True)))
        row("Project, 3 fields, no sums", time_ms(lambda: rb.Project(xT, BETA, ETAS, fields, passive=pr, sums=False)),
            seq, time_ms(lambda: parts(False)))
        with_chain = time_ms(lambda: flt0.Gradients(xT, xT, rows[0], [rows[1]], True, BETA, ETAS[0]))
        without = time_ms(lambda: flt0.Gradients(xT, xT, rows[0], [rows[1]], False, BETA, ETAS[0]))
        zero = time_ms(lambda: pr.Zero(rows)) if pr is not None else (0.0, 0.0, 0.0)
        theirs = tuple(with_chain[k] - without[k] + zero[k] for k in range(3))
        print("  (Gradients with projection %.4f, without %.4f, Zero %.4f)" % (with_chain[0], without[0], zero[0]))
        for r in rows:      # the repeated products have driven the rows to 0 or beyond the range: fresh ones
            r.copy_(grid.synth_density(seed=13))
        row("Chain, 2 rows, 2 thresholds", time_ms(lambda: rb.Chain(xT, BETA, rows, [ETAS[0], ETAS[2]], passive=pr)),
            "2 chain launches%s (by difference)" % (" + Zero" if pr is not None else ""), theirs)
grid.close()
