#!/usr/bin/env python
"""Times the heat-conduction fine level: the register form (ConductionOp) against the gather over the elements
(MatfreeOp<1>, TP_NO_COND_STENCIL -- read per launch, so the two forms alternate inside one process) on every epilogue of k_node:
product, residual, Chebyshev step, product + dot.  HIP events around back-to-back calls on the library's stream, after a warm-up,
in windows of at least a second; several windows per form, alternating; median and spread (max - min) / median per form.  The
Chebyshev step is the difference of a 9-step and a 1-step sweep divided by 8 (the sweeps' two copies of the iterate cancel).
Algorithmic bytes: 8 B x (nodes read + nodes written + elements) plus the epilogue's extra vectors (residual: b; Chebyshev step: b,
dinv, d read and written), as a share of 8 TB/s.  Then the assembly, the solve at rtol 1e-5 and one design iteration of the driver.
Prints ONE JSON line and writes it to profiles/conduction_timing.json.
usage: conduction_timing.py [ex ey ez nlvls [windows [window seconds]]]   (default 128 128 128 5 3 1.0)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez, nlv = [int(v) for v in sys.argv[1:5]] if len(sys.argv) > 4 else (128, 128, 128, 5)
WINDOWS = int(sys.argv[5]) if len(sys.argv) > 5 else 3
WINDOW_S = float(sys.argv[6]) if len(sys.argv) > 6 else 1.0
SWITCH, KMIN, KMAX, PENAL, PEAK = "TP_NO_COND_STENCIL", 1e-3, 1.0, 3.0, 8.0e12
FORMS = (("registers", None, (3, 2, 0, 0)), ("gather", "1", (3, 0, 0, 0)))


def set_form(value):
    os.environ.pop(SWITCH, None)
    if value is not None:
        os.environ[SWITCH] = value


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


h = 1.0 / ey
nx, ny, nz = ex + 1, ey + 1, ez + 1
nodes, elems = nx * ny * nz, ex * ey * ez
grid = tp.Grid(nx, ny, nz, h)
hc = tp.HeatConduction(grid, tp.SolverOptions(nlvls=nlv, nsmooth=2, ncoarse=30))
hc.SetUpLoadAndBC()
x = torch.from_numpy((np.random.default_rng(1).random(elems) < 0.5).astype(np.float64)).cuda()       # seeded 0/1 design
L, H = grid.L, hc.handle
u = torch.from_numpy(np.random.default_rng(2).standard_normal(nodes) + 0.5).cuda()
b, y, xs = torch.ones_like(u), torch.zeros_like(u), torch.zeros_like(u)
p = lambda t: C.c_void_p(t.data_ptr())

with torch.cuda.stream(torch.cuda.default_stream()):
    t0 = time.perf_counter()
    hc.AssembleConductivityMatrix(x, KMIN, KMAX, PENAL)
    torch.cuda.synchronize()
    first_assemble_ms = 1e3 * (time.perf_counter() - t0)
    assemble_ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hc.AssembleConductivityMatrix(x, KMIN, KMAX, PENAL)
        torch.cuda.synchronize()
        assemble_ms.append(1e3 * (time.perf_counter() - t0))

    def sweep(k):
        xs.copy_(u)
        assert L.tp_conduction_smooth(H, 0, p(b), p(xs), k, 0) == 0

    calls = {
        "apply": lambda: L.tp_conduction_apply(H, p(u), p(y)),
        "residual": lambda: L.tp_conduction_level_residual(H, 0, p(b), p(u), p(y)),
        "sweep1": lambda: sweep(1),
        "sweep9": lambda: sweep(9),
        "apply_dot": lambda: L.tp_conduction_apply_dot(H, p(u), p(y), None),
    }
    raw = {}
    for name, fn in calls.items():
        for _, value, expect in FORMS:          # warm-up of both forms, and the form check
            set_form(value)
            for _ in range(20):
                fn()
            assert hc.last_op_form() == expect, (name, hc.last_op_form(), expect)
        set_form(None)
        reps = max(20, int(np.ceil(1e3 * WINDOW_S / window_ms(fn, 50))))
        raw[name] = {f[0]: [] for f in FORMS}
        for _ in range(WINDOWS):
            for form, value, _ in FORMS:        # alternating
                set_form(value)
                raw[name][form].append(window_ms(fn, reps))
        raw[name]["reps"] = reps
    set_form(None)
    # the Chebyshev step: (9-step sweep - 1-step sweep) / 8, window by window
    raw["cheb"] = {f[0]: [(a9 - a1) / 8.0 for a9, a1 in zip(raw["sweep9"][f[0]], raw["sweep1"][f[0]])] for f in FORMS}
    extra = {"apply": 0, "residual": 1, "cheb": 4, "apply_dot": 0}
    epilogues = {}
    for name in ("apply", "residual", "cheb", "apply_dot"):
        e = {"bytes": 8.0 * (2 * nodes + elems + extra[name] * nodes)}
        for form, _, _ in FORMS:
            w = raw[name][form]
            med = statistics.median(w)
            e[form] = {"us": 1e3 * med, "spread": (max(w) - min(w)) / med, "windows_us": [1e3 * v for v in w], "share_of_8TBs": e["bytes"] / (1e-3 * med) / PEAK}
        spread_us = max(e[f[0]]["spread"] * e[f[0]]["us"] for f in FORMS)
        e["registers_over_gather"] = e["registers"]["us"] / e["gather"]["us"]
        e["no_slower_beyond_spread"] = bool(e["registers"]["us"] <= e["gather"]["us"] + spread_us)
        epilogues[name] = e
    # the solve at rtol 1e-5 from a zero state, both forms
    solve = {}
    for form, value, _ in FORMS:
        set_form(value)
        hc.SetTolerances(rtol=1e-5)
        t = []
        for _ in range(3):
            hc.T.zero_()
            torch.cuda.synchronize()
            hc.KSPSolve()
            t.append(1e3 * hc.last_solve_s)
        solve[form] = {"ms": statistics.median(t), "its": hc.last_its, "rerr": hc.last_rnorm / hc.last_bnorm}
    set_form(None)
grid.close()

# one design iteration of the driver (filter 1, MMA), median of iterations 3 .. 6
opt = tp.TopOpt(nxyz=(nx, ny, nz), xc=(0, ex * h, 0, 1, 0, ez * h), nlvls=nlv, rmin=2.56 * h, filter=1, volfrac=0.3, physics="heat",
                solver=tp.SolverOptions(nlvls=nlv, nsmooth=2, ncoarse=30))
recs = [opt.step() for _ in range(6)]
opt.grid.close()
out = {"mesh": [ex, ey, ez], "nodes": nodes, "elements": elems, "levels": nlv, "design": "seeded 0/1, kmin 1e-3", "windows": WINDOWS,
       "window_s": WINDOW_S, "epilogues": epilogues, "assemble_ms": {"first": first_assemble_ms, "median": statistics.median(assemble_ms)},
       "solve_rtol_1e-5": solve,
       "design_iteration": {"ms": 1e3 * statistics.median(r["time"] for r in recs[2:]), "ksp_its": [r["ksp_its"] for r in recs], "fx": [r["fx"] for r in recs],
                            "gx": [r["gx"] for r in recs]},
       "condition_met_on_every_epilogue": all(e["no_slower_beyond_spread"] for e in epilogues.values())}
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "conduction_timing.json"), "w") as f:
    f.write(line + "\n")
