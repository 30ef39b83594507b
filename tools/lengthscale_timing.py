#!/usr/bin/env python
"""Times the geometric length-scale constraints (tp_lengthscale) against two yardsticks of the same run: the cone filter's
un-normalised convolution tp_filter_mult_h at ElemConn 2, and a device-to-device copy of the call's algorithmic bytes (forward:
2 reads + 2 writes per element; with both gradients 4 reads + 2 writes more).  HIP events around back-to-back calls on the
library's stream, warm-up first, median (min .. max) of several batches.  Then the design iteration of the driver at 64x32x32 with
and without the constraints, and the driver's behaviour over a longer run.  Per-kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/lengthscale_timing.py 128 128 128 2 0 0`.
usage: lengthscale_timing.py [ex ey ez [batches [driver iterations [behaviour iterations]]]] [> profiles/lengthscale_timing.txt]
       (default 128 128 128 5 12 60)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 5
DRIVER_ITS = int(sys.argv[5]) if len(sys.argv) > 5 else 12
BEHAVIOUR_ITS = int(sys.argv[6]) if len(sys.argv) > 6 else 60
REPS = 20
BETA, ETA = 8.0, 0.5


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
flt, ls = tp.Filter(grid, 1, 2.56 * h), tp.LengthScale(grid)
assert flt.ElemConn == 2
x, xt, xp, y = grid.synth_density(), grid.elem_vec(), grid.elem_vec(), grid.elem_vec()
dgs, dgv = grid.elem_vec(), grid.elem_vec()
flt.FilterProject(x, xt, xp, True, BETA, ETA)
c = (2.56 * h) ** 4 / h ** 2
src4, dst4, src10, dst10 = (torch.empty(k * n, dtype=torch.float64, device=x.device) for k in (2, 2, 5, 5))
with torch.cuda.stream(torch.cuda.default_stream()):
    rows = [
        ("yardstick 1: tp_filter_mult_h, ElemConn 2 (fill + cone convolution)", lambda: flt.MultH(x, y)),
        ("yardstick 2a: copy of 2 reads + 2 writes per element", lambda: dst4.copy_(src4)),
        ("yardstick 2b: copy of 6 reads + 4 writes per element", lambda: dst10.copy_(src10)),
        ("tp_lengthscale_constraints, both kinds, forward only", lambda: ls.Constraints(xt, xp, c, projectionFilter=True, beta=BETA, eta=ETA)),
        ("tp_lengthscale_constraints, both kinds, both gradients",
         lambda: ls.Constraints(xt, xp, c, projectionFilter=True, beta=BETA, eta=ETA, dg_solid=dgs, dg_void=dgv)),
        ("tp_lengthscale_constraints, solid only, with its gradient",
         lambda: ls.Constraints(xt, xp, c, kinds="solid", projectionFilter=True, beta=BETA, eta=ETA, dg_solid=dgs)),
    ]
    print("# %dx%dx%d elements, c = %.6g, projection beta = %g, %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
          % (ex, ey, ez, c, BETA, REPS, BATCHES))
    res = [time_ms(fn) for _, fn in rows]
for (name, _), t in zip(rows, res):
    print("  %-70s %8.4f  (%.4f .. %.4f)" % ((name,) + t), flush=True)
print("  forward only / yardstick 1 = %.2f, / copy 2a = %.2f;  with both gradients / yardstick 1 = %.2f, / copy 2b = %.2f"
      % (res[3][0] / res[0][0], res[3][0] / res[1][0], res[4][0] / res[0][0], res[4][0] / res[2][0]), flush=True)
grid.close()

if DRIVER_ITS > 0:
    for name, kw in (("without the constraints", {}), ("length_scale = both", dict(length_scale="both"))):
        t = tp.TopOpt(nxyz=(65, 33, 33), volfrac=0.5, projectionFilter=True, **kw)
        recs = [t.step() for _ in range(DRIVER_ITS)]
        tail = recs[2:]
        print("driver 64x32x32, volfrac 0.5, projection on, %s: %.2f ms per design iteration (median of iterations 3..%d), %.1f CG iterations each"
              % (name, 1e3 * statistics.median(r["time"] for r in tail), DRIVER_ITS, statistics.mean(r["ksp_its"] for r in tail)), flush=True)
        t.grid.close()

if BEHAVIOUR_ITS > 0:
    fmt = lambda recs, key, f="%.4g": " ".join(f % r[key] for r in recs)
    for volfrac in (0.12, 0.5):
        for name, kw in (("length_scale = None", {}), ("length_scale = both, start 1", dict(length_scale="both")),
                         ("length_scale = both, start 20", dict(length_scale="both", length_scale_start=20))):
            t = tp.TopOpt(nxyz=(65, 33, 33), volfrac=volfrac, projectionFilter=True, **kw)
            recs = [t.step() for _ in range(BEHAVIOUR_ITS)]
            sel = [r for r in recs if r["itr"] <= 5 or r["itr"] % 5 == 0]
            print("behaviour 64x32x32, volfrac %g, %s, eps %g, iterations %s:" % (volfrac, name, t.length_scale_eps, " ".join(str(r["itr"]) for r in sel)))
            print("  fx       " + fmt(sel, "fx", "%.5g"))
            print("  gx       " + fmt(sel, "gx"))
            print("  mnd      " + fmt(sel, "mnd"))
            print("  ksp_its  " + fmt(sel, "ksp_its", "%d"))
            if kw:
                print("  gx_solid " + fmt(sel, "gx_solid"))
                print("  gx_void  " + fmt(sel, "gx_void"))
                feas = [r["itr"] for r in recs if r["gx_solid"] <= 0 and r["gx_void"] <= 0 and r["gx"] <= 1e-6]
                print("  feasible (all three constraints <= 0) at %d of %d iterations, first %s, beta at the end %g"
                      % (len(feas), len(recs), feas[0] if feas else "never", t.beta), flush=True)
            t.grid.close()
