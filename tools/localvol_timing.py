#!/usr/bin/env python
"""Times the local volume constraint (tp_localvol) against the cone filter's un-normalised convolution tp_filter_mult_h at the
SAME stencil width in the same run -- both go through the same convolution kernels, the one with a 0/1 table, the other with the
cone weights.  HIP events around back-to-back repeats on the library's stream, warm-up first, median of several batches.
Rows per radius: Mean (fill + one ball sum), Constraint forward only (+ k_localvol_pow, k_localvol_reduce, the host read),
Constraint with dgdx (+ k_localvol_coef and the second ball sum).  Then the design iteration of the driver at 64x32x32 with and
without the constraint.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/localvol_timing.py 128 128 128 2 0`.
usage: localvol_timing.py [ex ey ez [batches [driver iterations]]] [> profiles/localvol_timing.txt]     (default 128 128 128 7 12)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 7
DRIVER_ITS = int(sys.argv[5]) if len(sys.argv) > 5 else 12
REPS = 20
ALPHA, P = 0.6, 16.0
KERNELS = {1: "tiled", 2: "several outputs along z", 3: "wide", 4: "streamed ring", 5: "generic"}


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
h = 1.0 / ey
x = grid.synth_density()
rb, dg, y = grid.elem_vec(), grid.elem_vec(), grid.elem_vec()
print("# %dx%dx%d elements, alpha = %g, p = %g, %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, ALPHA, P, REPS, BATCHES))
for r_over_h in (2.56, 5.5, 8.5):
    lv, flt = tp.LocalVolume(grid, r_over_h * h), tp.Filter(grid, 1, r_over_h * h)
    assert lv.stencil_width == flt.ElemConn
    rows = [
        ("yardstick: tp_filter_mult_h (fill + cone convolution)", lambda: flt.MultH(x, y)),
        ("tp_localvol_mean (fill + ball sum)", lambda: lv.Mean(x, rb)),
        ("tp_localvol_constraint, forward only (+ pow, reduce, host read)", lambda: lv.Constraint(x, ALPHA, P)),
        ("tp_localvol_constraint with dgdx (+ coef, second ball sum)", lambda: lv.Constraint(x, ALPHA, P, dgdx=dg)),
    ]
    res = [time_ms(fn) for _, fn in rows]
    print("R = %.2f h, stencil width %d (%d taps), ball sum kernel: %s; cone filter kernel: %s"
          % (r_over_h, lv.stencil_width, (2 * lv.stencil_width + 1) ** 3, KERNELS[lv.last_kernel()], KERNELS[flt.last_kernel()]))
    for (name, _), t in zip(rows, res):
        print("  %-66s %8.4f  (%.4f .. %.4f)" % ((name,) + t), flush=True)
    print("  full call / yardstick = %.2f; full call - 2 yardsticks = %.4f ms (the two streaming passes, the reduction, the read)"
          % (res[3][0] / res[0][0], res[3][0] - 2 * res[0][0]), flush=True)
    lv.close()
    flt.close()
grid.close()

if DRIVER_ITS > 0:
    hh = 2.0 / 64
    for name, kw in (("without the constraint", {}), ("local_volume = 0.4, R = 3.5 h, p = 16", dict(local_volume=0.4, local_volume_R=3.5 * hh))):
        t = tp.TopOpt(nxyz=(65, 33, 33), volfrac=0.5, **kw)
        recs = [t.step() for _ in range(DRIVER_ITS)]
        tail = recs[2:]
        print("driver 64x32x32, volfrac 0.5, %s: %.2f ms per design iteration (median of iterations 3..%d), %.1f CG iterations each%s"
              % (name, 1e3 * statistics.median(r["time"] for r in tail), DRIVER_ITS, statistics.mean(r["ksp_its"] for r in tail),
                 "; gx_local " + " ".join("%.4f" % r["gx_local"] for r in recs) if kw else ""), flush=True)
        t.grid.close()
