#!/usr/bin/env python
"""Times the thermoelastic passes beside the self-weight kernels of the same run, the yardsticks of the gather
(k_body_load) and element-thread (k_body_sens) patterns.  Every entry point forms the coefficient it needs first (k_thermal_coef:
beta for the load and the adjoint right-hand side, beta' for the sensitivity), so a call is that pass plus its own kernel: the
coefficient pass is timed through tp_elasticity_thermal_coefficients, one output at a time, with its device copy timed alone
and taken off, and each kernel is its call minus the pass it ran.  HIP events around back-to-back calls on the
library's stream, after a warm-up, in windows of at least a second; several windows per call, the calls alternating; median and
spread (max - min) / median.  Algorithmic bytes per kernel as count_launch books them, as a share of 8 TB/s.  Then one design
iteration of the driver on a second mesh, thermoelastic (both thermal modes) beside heat and plain elasticity.
Prints ONE JSON line and writes it to profiles/thermoelastic_timing.json.
usage: thermoelastic_timing.py [ex ey ez [windows [window seconds [dex dey dez dlevels diters]]]]   (default 128 128 128 3 1.0 64 32 32 3 10)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import topopt_in_petsc_amd as tp

ex, ey, ez = [int(v) for v in sys.argv[1:4]] if len(sys.argv) > 3 else (128, 128, 128)
WINDOWS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
WINDOW_S = float(sys.argv[5]) if len(sys.argv) > 5 else 1.0
dex, dey, dez, dlv, dit = [int(v) for v in sys.argv[6:11]] if len(sys.argv) > 10 else (64, 32, 32, 3, 10)
PEAK = 8.0e12


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
n, m = nx * ny * nz, ex * ey * ez
grid = tp.Grid(nx, ny, nz, h)
le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=1))
le.SetUpLoadAndBC()
le.SetThermalExpansion(1e-3, 0.25, 3.0, 1e-9, 1.0)
le.SetBodyForce((0.0, 0.0, -1.0), 0.1)
rng = np.random.default_rng(1)
x = torch.from_numpy(0.05 + 0.95 * rng.random(m)).cuda()
T = torch.from_numpy(rng.standard_normal(n) + 0.5).cuda()
v = torch.from_numpy(rng.standard_normal(3 * n) + 0.5).cuda()
f, g, df, c1, c2 = grid.node_vec(3), grid.node_vec(1), grid.elem_vec(), grid.elem_vec(), grid.elem_vec()

with torch.cuda.stream(torch.cuda.default_stream()):
    calls = {
        "copy": lambda: c1.copy_(x),
        "coef_beta_call": lambda: le.ThermalCoefficients(x, beta=c1),
        "coef_dbeta_call": lambda: le.ThermalCoefficients(x, dbeta=c2),
        "load_call": lambda: le.ThermalLoad(x, T, f),
        "adjoint_call": lambda: le.ThermalAdjointRHS([v], None, x, 1.0, g),
        "sens_call": lambda: le.ThermalSensitivity([v], None, x, T, 2.0, df),
        "k_body_load": lambda: le.BodyLoad(x, f),
        "k_body_sens": lambda: le.BodySensitivity([v], None, x, 2.0, df),
    }
    reps = {}
    for name, fn in calls.items():
        for _ in range(20):
            fn()
        reps[name] = max(20, int(np.ceil(1e3 * WINDOW_S / window_ms(fn, 50))))
    raw = {name: [] for name in calls}
    for _ in range(WINDOWS):
        for name, fn in calls.items():          # alternating
            raw[name].append(window_ms(fn, reps[name]))
grid.close()

# window by window: a coefficient pass is its call minus the copy, each kernel its call minus the coefficient pass it ran
raw["k_thermal_coef_beta"] = [a - b for a, b in zip(raw["coef_beta_call"], raw["copy"])]
raw["k_thermal_coef_dbeta"] = [a - b for a, b in zip(raw["coef_dbeta_call"], raw["copy"])]
for k, call, coef in (("k_thermal_load", "load_call", "k_thermal_coef_beta"), ("k_thermal_adjoint_rhs", "adjoint_call", "k_thermal_coef_beta"),
                      ("k_thermal_sens", "sens_call", "k_thermal_coef_dbeta")):
    raw[k] = [a - b for a, b in zip(raw[call], raw[coef])]
BYTES = {
    "k_thermal_coef_beta": 16.0 * m,
    "k_thermal_coef_dbeta": 16.0 * m,
    "k_thermal_load": 8.0 * m + 32.0 * n,
    "k_thermal_adjoint_rhs": 8.0 * m + 56.0 * n,
    "k_thermal_sens": 24.0 * m + 56.0 * n,
    "k_body_load": 8.0 * m + 24.0 * n,
    "k_body_sens": 24.0 * m + 48.0 * n,
}
kernels = {}
for name, nbytes in BYTES.items():
    w = raw[name]
    med = statistics.median(w)
    kernels[name] = {"us": 1e3 * med, "spread": (max(w) - min(w)) / med, "windows_us": [1e3 * t for t in w], "bytes": nbytes,
                     "share_of_8TBs": nbytes / (1e-3 * med) / PEAK}
calls_out = {name: {"us": 1e3 * statistics.median(raw[name]), "spread": (max(raw[name]) - min(raw[name])) / statistics.median(raw[name]), "reps": reps[name]}
             for name in calls}

# one design iteration of the driver (filter 1, MMA), median of iterations 3 .. end
dh = 1.0 / dey
iteration = {}
for label, kw in (("thermoelastic", dict(physics="thermoelastic", alpha=2e-4, T_ref=0.25)),
                  ("thermoelastic_uniform", dict(physics="thermoelastic", alpha=2e-3, T_ref=0.25, thermal="uniform", delta_T=1.0)),
                  ("heat", dict(physics="heat")), ("elasticity", dict())):
    opt = tp.TopOpt(nxyz=(dex + 1, dey + 1, dez + 1), xc=(0, dex * dh, 0, 1, 0, dez * dh), nlvls=dlv, rmin=2.56 * dh, filter=1, **kw)
    recs = [opt.step() for _ in range(dit)]
    opt.grid.close()
    iteration[label] = {"ms": 1e3 * statistics.median(r["time"] for r in recs[2:]), "fx": [r["fx"] for r in recs], "ksp_its": [r["ksp_its"] for r in recs]}
    if "ksp_its_thermal" in recs[0]:
        iteration[label].update(ksp_its_thermal=[r["ksp_its_thermal"] for r in recs], ksp_its_thermal_adjoint=[r["ksp_its_thermal_adjoint"] for r in recs],
                                T_max=[r["T_max"] for r in recs])
out = {"mesh": [ex, ey, ez], "nodes": n, "elements": m, "design": "seeded mixed field in [0.05, 1]", "windows": WINDOWS, "window_s": WINDOW_S,
       "kernels": kernels, "calls": calls_out, "design_iteration": {"mesh": [dex, dey, dez], "levels": dlv, "iterations": dit, **iteration}}
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "thermoelastic_timing.json"), "w") as fh:
    fh.write(line + "\n")
