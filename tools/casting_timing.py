#!/usr/bin/env python
"""Times the casting filter (tp_casting) for the draws +x (both forms of TP_CASTING_XFORM, alternating), +y, +z and z:<ez/2> beside
a device copy, the cone filter's un-normalised convolution tp_filter_mult_h at stencil width 2 and tp_overhang_forward in the same
run.  HIP events around back-to-back repeats on the library's stream, warm-up first, median of several batches.  Rows per draw:
Forward, Adjoint of one vector, Adjoint of three, each with its streaming bytes (24 B per cell forward: x in, c and q out;
8 + 16 nv B per cell for the transpose: q in, nv vectors in and out) and the fraction of its time those bytes would take at the
copy rate of this run.  Then the design iteration of the driver at 64x32x32 with and without the filter.
usage: casting_timing.py [ex ey ez [batches [driver iterations]]] [> profiles/casting_timing.txt]     (default 128 128 128 5 12)"""
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
n = ex * ey * ez
x = grid.synth_density()
c, y = grid.elem_vec(), grid.elem_vec()
g = [grid.elem_vec(1.0) for _ in range(3)]
print("# %dx%dx%d elements, %d back-to-back calls per batch, median (min .. max) of %d batches, ms per call"
      % (ex, ey, ez, REPS, BATCHES))
t_copy = time_ms(lambda: y.copy_(x))
rate = 16.0 * n / (t_copy[0] * 1e-3)   # bytes per second, read + write
print("  %-66s %8.4f  (%.4f .. %.4f)   %.2f TB/s read + write" % (("yardstick: device copy of one field",) + t_copy + (rate / 1e12,)), flush=True)
flt = tp.Filter(grid, 1, 2.56 * h)
assert flt.ElemConn == 2
print("  %-66s %8.4f  (%.4f .. %.4f)" % (("yardstick: tp_filter_mult_h, stencil width 2 (fill + cone convolution)",) + time_ms(lambda: flt.MultH(x, y))),
      flush=True)
ov = tp.Overhang(grid, "+z")
print("  %-66s %8.4f  (%.4f .. %.4f)" % (("yardstick: tp_overhang_forward, +z, default chunk length",) + time_ms(lambda: ov.Forward(x, c))), flush=True)
ov.close()
flt.close()


def rows_of(cf):
    return [("tp_casting_forward", 24.0, lambda: cf.Forward(x, c)),
            ("tp_casting_adjoint, 1 vector", 24.0, lambda: cf.Adjoint(g[:1])),
            ("tp_casting_adjoint, 2 vectors (the driver's call at m = 1)", 40.0, lambda: cf.Adjoint(g[:2])),
            ("tp_casting_adjoint, 3 vectors", 56.0, lambda: cf.Adjoint(g))]


def report(title, name, bytes_per_cell, t):
    ideal = bytes_per_cell * n / rate * 1e3
    print("  %-66s %8.4f  (%.4f .. %.4f)   %5.1f MB, %4.1f %% of the time at the copy rate"
          % ((title + name,) + t + (bytes_per_cell * n / 1e6, 100.0 * ideal / t[0])), flush=True)


FORMS = {1: "walk", 2: "LDS-staged x", 3: "walk on x lines"}
# the two x forms in one pass, alternating, so that a drift of the machine meets both
cf = tp.Casting(grid, "+x")
first = {}
print("draw +x: TP_CASTING_XFORM = 1 (%s) and 0 (%s), alternating" % (FORMS[2], FORMS[3]))
for k, (name, bpc, fn) in enumerate(rows_of(cf)):
    for form in (1, 0):
        os.environ["TP_CASTING_XFORM"] = str(form)
        for v in g:
            v.fill_(1.0)   # the transpose works in place; its weights (1 + q) / 2 and (1 - q) / 2 sum to 1, so repeats stay bounded
        t = time_ms(fn)
        assert cf.last_form() == (2 if form else 3)
        report("XFORM = %d: " % form, name, bpc, t)
        if k == 0:
            first[form] = c.clone()
print("  c of the two forms equal bit for bit: %s" % torch.equal(first[0], first[1]))
os.environ.pop("TP_CASTING_XFORM", None)
cf.close()
for draw in ("+y", "+z", "z:%d" % (ez // 2)):
    cf = tp.Casting(grid, draw)
    print("draw %s (%s, one launch per sweep)" % (draw, FORMS[1]))
    for name, bpc, fn in rows_of(cf):
        for v in g:
            v.fill_(1.0)
        t = time_ms(fn)
        assert cf.last_form() == 1
        report("", name, bpc, t)
    cf.close()
grid.close()

if DRIVER_ITS > 0:
    for name, kw in (("without the filter", {}), ("casting = +z", dict(casting="+z"))):
        t = tp.TopOpt(nxyz=(65, 33, 33), volfrac=0.3, **kw)
        recs = [t.step() for _ in range(DRIVER_ITS)]
        tail = recs[2:]
        print("driver 64x32x32, volfrac 0.3, %s: %.2f ms per design iteration (median of iterations 3..%d), %.1f CG iterations each%s"
              % (name, 1e3 * statistics.median(r["time"] for r in tail), DRIVER_ITS, statistics.mean(r["ksp_its"] for r in tail),
                 "; cast_fill " + " ".join("%.4f" % r["cast_fill"] for r in recs) if kw else ""), flush=True)
        t.grid.close()
