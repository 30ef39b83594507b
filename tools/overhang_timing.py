#!/usr/bin/env python
"""Times the overhang filter (tp_overhang) for every chunk length of TP_OVERHANG_CHUNK against the cone filter's un-normalised
convolution tp_filter_mult_h at stencil width 2 in the same run.  HIP events around back-to-back repeats on the library's stream,
warm-up first, median of several batches.  Rows per chunk length: Forward, Adjoint of one vector, Adjoint of three.  Then the
design iteration of the driver at 64x32x32 with and without the filter.
usage: overhang_timing.py [ex ey ez [batches [driver iterations]]] [> profiles/overhang_timing.txt]     (default 128 128 128 5 12)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
BATCHES = int(sys.argv[4]) if len(sys.argv) > 4 else 5
DRIVER_ITS = int(sys.argv[5]) if len(sys.argv) > 5 else 12
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
x = grid.synth_density()
xi, y = grid.elem_vec(), grid.elem_vec()
g = [grid.elem_vec(1.0) for _ in range(3)]
print("# %dx%dx%d elements, build +z (%d layers), %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, ez, REPS, BATCHES))
flt = tp.Filter(grid, 1, 2.56 * h)
assert flt.ElemConn == 2
print("  %-66s %8.4f  (%.4f .. %.4f)" % (("yardstick: tp_filter_mult_h, stencil width 2 (fill + cone convolution)",) + time_ms(lambda: flt.MultH(x, y))),
      flush=True)
ov = tp.Overhang(grid, "+z")
first = None
for c in (1, 2, 4, 8):
    os.environ["TP_OVERHANG_CHUNK"] = str(c)
    rows = [("tp_overhang_forward", lambda: ov.Forward(x, xi)),
            ("tp_overhang_adjoint, 1 vector", lambda: ov.Adjoint(g[:1])),
            ("tp_overhang_adjoint, 3 vectors", lambda: ov.Adjoint(g))]
    print("TP_OVERHANG_CHUNK = %d: %d launches per sweep" % (c, (ez - 1 + c - 1) // c + 1))
    for name, fn in rows:
        for v in g:
            v.fill_(1e-200)   # the transpose works in place: the repeats compound, so start far from overflow
        t = time_ms(fn)
        assert ov.last_chunk() == c
        print("  %-66s %8.4f  (%.4f .. %.4f)" % ((name,) + t), flush=True)
    if first is None:
        first = xi.clone()
    else:
        print("  xi equal to chunk 1 bit for bit: %s" % torch.equal(first, xi))
os.environ.pop("TP_OVERHANG_CHUNK", None)
ov.close()
flt.close()
grid.close()

if DRIVER_ITS > 0:
    for name, kw in (("without the filter", {}), ("overhang = +z", dict(overhang="+z"))):
        t = tp.TopOpt(nxyz=(65, 33, 33), volfrac=0.3, **kw)
        recs = [t.step() for _ in range(DRIVER_ITS)]
        tail = recs[2:]
        print("driver 64x32x32, volfrac 0.3, %s: %.2f ms per design iteration (median of iterations 3..%d), %.1f CG iterations each%s"
              % (name, 1e3 * statistics.median(r["time"] for r in tail), DRIVER_ITS, statistics.mean(r["ksp_its"] for r in tail),
                 "; print_loss " + " ".join("%.4f" % r["print_loss"] for r in recs) if kw else ""), flush=True)
        t.grid.close()
