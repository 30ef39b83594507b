#!/usr/bin/env python
"""Times the linking kernels (tp_link): expand, and fold in forms 1 and 2, for x:mirror, x:repeat:4, x:extrude, z:extrude and the
three-axis combination x:mirror y:repeat:2 z:extrude, nvec = 2 and 5 (the objective's row and 1 or 4 constraint rows), against the
same work as one torch call per vector with a host-built map: index_select for expand, index_add_ into a zeroed vector for fold.
(index_add_ adds with atomics: its bits are not reproducible from run to run, and it starts from 0.0.)  HIP events around 20
back-to-back calls on the library's stream, warm-up first; the rows of one spec are timed in alternating windows -- every batch
times each row once, in turn -- and the median (min .. max) of the batches is printed.  The design iteration itself:
tools/run_topopt.py 128 128 128 5 5 with and without --link y:mirror.
usage: link_timing.py [ex ey ez [batches]] [> profiles/link_timing.txt]   (default 128 128 128 5)"""
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
SPECS = ("x:mirror", "x:repeat:4", "x:extrude", "z:extrude", ["x:mirror", "y:repeat:2", "z:extrude"])


def reduced_map(modes, cells, ne):
    """r(e) for every element, flat (host)"""
    idx, nr = [], []
    for mode, c, n in zip(modes, cells, ne):
        i = np.arange(n)
        idx.append(i if mode == 0 else np.minimum(i, n - 1 - i) if mode == 1 else i % (n // c) if mode == 2 else 0 * i)
        nr.append(n if mode == 0 else (n + 1) // 2 if mode == 1 else n // c if mode == 2 else 1)
    return ((idx[2][:, None, None] * nr[1] + idx[1][None, :, None]) * nr[0] + idx[0][None, None, :]).reshape(-1)


def time_rows(rows, reps=REPS):
    """rows: [(name, fn)] -> {name: (median, min, max)} ms per call, the rows alternating inside every batch"""
    for _, fn in rows:
        for _ in range(3):
            fn()
    out = {name: [] for name, _ in rows}
    for _ in range(BATCHES):
        for name, fn in rows:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / reps)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


grid = tp.Grid(ex + 1, ey + 1, ez + 1, 1.0 / ey)
n = ex * ey * ez
print("# %dx%dx%d elements, %d back-to-back calls per batch, rows of a spec alternating inside every batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, REPS, BATCHES))
with torch.cuda.stream(torch.cuda.default_stream()):
    for spec in SPECS:
        lk = tp.Link(grid, spec)
        rmap = torch.from_numpy(reduced_map(lk.modes, lk.cells, (ex, ey, ez))).cuda()
        print("%s: %d reduced of %d" % (spec if isinstance(spec, str) else " ".join(spec), lk.n_reduced, n))
        for nvec in (2, 5):
            full = [grid.synth_density(seed=7 + v) for v in range(nvec)]
            red = [lk.reduced_vec(0.5) for _ in range(nvec)]

            def fold(form):
                def go():
                    lk.set_form(form)
                    lk.Fold(full, red)
                return go

            def torch_expand():
                for f, r in zip(full, red):
                    torch.index_select(r, 0, rmap, out=f)

            def torch_fold():
                for f, r in zip(full, red):
                    r.zero_()
                    r.index_add_(0, rmap, f)

            rows = [("tp_link_expand", lambda: lk.Expand(red, full)), ("torch index_select per vector", torch_expand),
                    ("tp_link_fold form 1", fold(1)), ("tp_link_fold form 2", fold(2)), ("torch zero_ + index_add_ per vector", torch_fold)]
            lk.set_form(2)
            lk.Fold(full, red)
            if lk.last_form() != 2:          # form 2 does not apply (x not linked): no row for it
                rows = [r for r in rows if r[0] != "tp_link_fold form 2"]
            t = time_rows(rows)
            for name, _ in rows:
                print("  nvec = %d  %-38s %8.4f  (%.4f .. %.4f)" % ((nvec, name) + t[name]), flush=True)
            lk.set_form(0)
        lk.close()
grid.close()
