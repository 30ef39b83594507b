#!/usr/bin/env python
"""End-to-end run of the reference's optimisation loop on the MI355X path.
usage: run_topopt.py [--physics elasticity|heat|thermoelastic [--alpha A] [--thermal uniform:DT] [--t-ref T] [--thermal-penal P]] [--loadcase top[:weight]]... [--stress-limit L [--stress-p P] [--stress-q q]] [--local-volume ALPHA:R] [--overhang +z|-z|+y|-y] [--casting DRAW [--casting-eps E]] [--self-weight bx,by,bz[:xlow] [--no-point-load]] [--length-scale both|solid|void[:C]] [--frequency-limit L[:nev]] [--load cantilever|axial] [--buckling-limit L[:nev]] [--passive solid|void:box|sphere|cylinder:numbers]... [--robust ETA_E,ETA_N,ETA_D[:every]] [--link AXIS:MODE[:CELLS]]... ex ey ez nlvls n_iter [filter [nsmooth ncoarse]]
(e.g. 128 128 128 5 20 1 2 45: the cycle of bench.py; --loadcase top:0.5 adds the line load on the upper edge as a second load
case of weight 0.5 -- the objective becomes the weighted sum of the cases' compliances; --stress-limit L holds the von Mises
p-norm of load case 0 below L as a second constraint, exponent --stress-p (8), stress relaxation x^q with --stress-q (0.5); --local-volume ALPHA:R holds the mean density in a ball of
radius R (a length, the element size is 1/ey) around every element below ALPHA through one p-norm constraint, exponent 16, as
the last constraint; --overhang DIR evaluates every response on the printed density of a part built layer by layer along DIR, the
overhang filter of DESIGN 4.11; --casting DRAW evaluates every response on the density of a part that leaves its mould along DRAW
without undercut or cavity, the casting filter of DESIGN 4.20: +x .. -z for a one-sided mould, x:K, y:K or z:K for a two-sided one
parted between the element layers K - 1 and K, smoothing --casting-eps (1e-6), not together with --overhang; --self-weight bx,by,bz[:xlow] adds the structure's own weight, a body force (per unit volume at full
density) that moves with the design, the mass of elements below xlow (0.1) damped, DESIGN 4.12 -- with --no-point-load it is the only
load; --length-scale KINDS[:C] holds a minimum length scale of the solid and / or the void phase by the geometric constraints of
DESIGN 4.13 as the last constraints, decay C in length^2 (default rmin^4 / h^2), with the Heaviside projection switched on;
--frequency-limit L[:nev] holds the harmonic mean of the lowest nev (3) eigenvalues of K phi = lambda M phi above L, DESIGN 4.14;
--load axial replaces the reference's line load by a uniform traction along -x on the face x = xmax, total 1 (a column in
compression); --buckling-limit L[:nev] holds the lowest linear buckling load factor of load case 0 above L through the p-norm of
the nev (2) largest eigenvalues of -G phi = mu K phi, DESIGN 4.19 -- best together with --load axial;
--passive KIND:SHAPE:numbers holds the elements whose centres lie in a shape at full density (solid) or empty (void), the passive
regions of DESIGN 4.15, in physical coordinates (the box is ex/ey x 1 x ez/ey): box:x0,x1,y0,y1,z0,z1, sphere:cx,cy,cz,r or
cylinder:axis,c1,c2,r (axis x, y or z, infinite along it); later shapes override earlier ones, e.g.
--passive solid:box:1.9,2,0,1,0,0.1 --passive void:sphere:1,0.5,0.5,0.25; --robust 0.7,0.5,0.3[:every] runs the robust formulation of
DESIGN 4.16 with the Heaviside projection switched on: the compliance of the design eroded at 0.7, the volume held on the design
dilated at 0.3 so that the nominal one at 0.5 meets volfrac, the dilated target recomputed every `every` (20) iterations;
--physics heat runs the heat-sink problem of DESIGN 4.17 instead of the cantilever: steady conduction with a sink patch on the face
x = 0 and a uniform source, conductivity 1e-3 + xPhys^3 (1 - 1e-3), the thermal compliance as the objective -- with --passive
only, none of the other options; --physics thermoelastic --alpha A runs the cantilever under its point load plus the thermal
expansion of a temperature field: by default the heat-sink problem's, solved on the same grid, with --thermal
uniform:DT a uniform rise DT above the reference temperature --t-ref (0); --thermal-penal is the exponent of the thermal stress
coefficient's interpolation (the stiffness's) -- with --passive only, none of the other options; --link AXIS:MODE[:CELLS] links
design variables along an axis: x:mirror, y:repeat:4, z:extrude, one per axis -- MMA works on one variable per orbit
and the design is exactly symmetric, periodic or constant along the axis; not together with --passive)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import topopt_in_petsc_amd as tp


def _option(name, needs=""):
    """takes every `name value` / `name=value` out of sys.argv -> the values in order (strings)"""
    vals, rest, i, argv = [], [], 0, sys.argv[1:]
    while i < len(argv):
        a = argv[i]
        if a == name or a.startswith(name + "="):
            if a == name:
                i += 1
                if i >= len(argv):
                    sys.exit("%s needs a value%s" % (name, needs))
            vals.append(argv[i] if a == name else a.split("=", 1)[1])
        else:
            rest.append(a)
        i += 1
    sys.argv[1:] = rest
    return vals


def _last(name, conv=str):
    vals = [conv(v) for v in _option(name)]
    return vals[-1] if vals else None


loadcases = []
for v in _option("--loadcase", ": top[:weight]"):
    name, _, wt = v.partition(":")
    if name != "top":
        sys.exit("--loadcase: the only built-in further load case is 'top', got %r" % name)
    loadcases.append((name, float(wt) if wt else 1.0))
stress_limit, stress_p, stress_q = _last("--stress-limit", float), _last("--stress-p", float), _last("--stress-q", float)
stress = {} if stress_limit is None else dict(stress_limit=stress_limit, stress_P=8.0 if stress_p is None else stress_p,
                                              stress_q=0.5 if stress_q is None else stress_q)
local_volume = _last("--local-volume")
local = {}
if local_volume is not None:
    alpha, sep, radius = local_volume.partition(":")
    if not sep:
        sys.exit("--local-volume needs ALPHA:R, got %r" % local_volume)
    local = dict(local_volume=float(alpha), local_volume_R=float(radius))
overhang, self_weight = _last("--overhang"), _last("--self-weight")
casting_draw, casting_eps = _last("--casting"), _last("--casting-eps", float)
casting = {} if casting_draw is None else dict(casting=casting_draw, **({} if casting_eps is None else dict(casting_eps=casting_eps)))
no_point_load = "--no-point-load" in sys.argv[1:]
sys.argv[1:] = [a for a in sys.argv[1:] if a != "--no-point-load"]
body = {}
if self_weight is not None:
    vec, _, xlow = self_weight.partition(":")
    try:
        body = dict(body_force=tuple(float(v) for v in vec.split(",")), body_force_xlow=float(xlow) if xlow else 0.1)
    except ValueError:
        sys.exit("--self-weight needs bx,by,bz[:xlow], got %r" % self_weight)
    if len(body["body_force"]) != 3:
        sys.exit("--self-weight needs bx,by,bz[:xlow], got %r" % self_weight)
if no_point_load:
    if not body:
        sys.exit("--no-point-load needs --self-weight")
    body["point_load"] = False
length_scale, length = _last("--length-scale"), {}
if length_scale is not None:
    kinds, _, cval = length_scale.partition(":")
    if kinds not in ("both", "solid", "void"):
        sys.exit("--length-scale needs both, solid or void, optionally :C, got %r" % length_scale)
    length = dict(length_scale=kinds, length_scale_c=float(cval) if cval else None, projectionFilter=True)
frequency_limit, frequency = _last("--frequency-limit"), {}
if frequency_limit is not None:
    lim, _, nev = frequency_limit.partition(":")
    try:
        frequency = dict(frequency_limit=float(lim), frequency_modes=int(nev) if nev else 3)
    except ValueError:
        sys.exit("--frequency-limit needs L[:nev], got %r" % frequency_limit)
load_arg = _last("--load") or "cantilever"
if load_arg not in ("cantilever", "axial"):
    sys.exit("--load needs cantilever or axial, got %r" % load_arg)
buckling_limit, buckling = _last("--buckling-limit"), {}
if buckling_limit is not None:
    lim, _, nev = buckling_limit.partition(":")
    try:
        buckling = dict(buckling_limit=float(lim), buckling_modes=int(nev) if nev else 2)
    except ValueError:
        sys.exit("--buckling-limit needs L[:nev], got %r" % buckling_limit)
shapes = []
for v in _option("--passive", ": solid|void:box|sphere|cylinder:numbers"):
    try:
        kind, form, nums = v.split(":")
        nums = nums.split(",")
        axis = [nums.pop(0)] if form == "cylinder" else []     # x, y, z or 0, 1, 2
        shapes.append((kind, form, tuple([a if a in ("x", "y", "z") else int(a) for a in axis] + [float(t) for t in nums])))
    except ValueError:
        sys.exit("--passive needs KIND:SHAPE:numbers, e.g. solid:box:1.9,2,0,1,0,0.1, got %r" % v)
links = _option("--link", ": AXIS:MODE[:CELLS], e.g. y:mirror, x:repeat:4, z:extrude")
robust_arg, robust = _last("--robust"), {}
if robust_arg is not None:
    etas, _, every = robust_arg.partition(":")
    try:
        robust = dict(robust=tuple(float(v) for v in etas.split(",")), robust_volume_every=int(every) if every else 20, projectionFilter=True)
    except ValueError:
        sys.exit("--robust needs ETA_E,ETA_N,ETA_D[:every], e.g. 0.7,0.5,0.3:20, got %r" % robust_arg)
physics = _last("--physics") or "elasticity"
if physics not in ("elasticity", "heat", "thermoelastic"):
    sys.exit("--physics needs elasticity, heat or thermoelastic, got %r" % physics)
thermo = {}
alpha_arg, thermal_arg, tref_arg, tpenal_arg = _last("--alpha"), _last("--thermal"), _last("--t-ref"), _last("--thermal-penal")
if physics == "thermoelastic":
    if alpha_arg is None:
        sys.exit("--physics thermoelastic needs --alpha A")
    try:
        thermo = dict(alpha=float(alpha_arg), T_ref=float(tref_arg) if tref_arg is not None else 0.0,
                      thermal_penal=float(tpenal_arg) if tpenal_arg is not None else None)
        if thermal_arg is not None:
            kind, _, dt = thermal_arg.partition(":")
            if kind != "uniform" or not dt:
                raise ValueError(thermal_arg)
            thermo.update(thermal="uniform", delta_T=float(dt))
    except ValueError:
        sys.exit("--alpha, --t-ref and --thermal-penal need numbers, --thermal needs uniform:DT; got %r, %r, %r, %r" % (alpha_arg, tref_arg, tpenal_arg, thermal_arg))
elif any(v is not None for v in (alpha_arg, thermal_arg, tref_arg, tpenal_arg)):
    sys.exit("--alpha, --thermal, --t-ref and --thermal-penal belong to --physics thermoelastic")
ex, ey, ez, nlv, nit = [int(v) for v in sys.argv[1:6]]
flt = int(sys.argv[6]) if len(sys.argv) > 6 else 1
h = 1.0 / ey
opt = tp.TopOpt(nxyz=(ex + 1, ey + 1, ez + 1), xc=(0, ex * h, 0, 1, 0, ez * h), nlvls=nlv, rmin=2.56 * h, filter=flt,
                loadcases=loadcases or None, **stress, **local, overhang=overhang, **casting, **body, **length, **frequency, load=load_arg, **buckling, passive=shapes or None, link=links or None, **robust, physics=physics, **thermo,
                solver=tp.SolverOptions(nlvls=nlv, **(dict(nsmooth=int(sys.argv[7]), ncoarse=int(sys.argv[8])) if len(sys.argv) > 8 else {})))
print("# %dx%dx%d elements, %d DOF, %d MG levels, filter %d, rmin %.4f" % (ex, ey, ez, (1 if physics == "heat" else 3) * (ex + 1) * (ey + 1) * (ez + 1), nlv, flt, 2.56 * h))
for it in range(nit):
    r = opt.step(verbose=True)
    print("State solver:  iter: %i, rerr.: %e | MMA inner its: %d" % (r["ksp_its"], r["ksp_rerr"], r["mma_inner"]), flush=True)
    if "f_case" in r:
        print("Load cases:    f: %s | iter: %s" % (" ".join("%e" % f for f in r["f_case"]), " ".join("%d" % k for k in r["ksp_its_case"])), flush=True)
    if "stress_pnorm" in r:
        print("Stress:        p-norm: %e, max: %e, gx[1]: %f | adjoint iter: %d"
              % (r["stress_pnorm"], r["stress_max"], r["gx_stress"], r["ksp_its_adjoint"]), flush=True)
    if "print_loss" in r:
        print("Overhang:      build %s, mean(xPhys - xPrint): %f" % (overhang, r["print_loss"]), flush=True)
    if "cast_fill" in r:
        print("Casting:       draw %s, mean(xPrint - xPhys): %f" % (casting_draw, r["cast_fill"]), flush=True)
    if "ksp_its_thermal" in r:
        print("Thermoelastic: T max: %e | conduction iter: %d, thermal adjoint iter: %d" % (r["T_max"], r["ksp_its_thermal"], r["ksp_its_thermal_adjoint"]), flush=True)
    if "body_share" in r:
        print("Self-weight:   b: %s, x_low: %g, body load's share of the compliance: %f" % (",".join("%g" % v for v in opt.body_force), opt.body_force_xlow, r["body_share"]), flush=True)
    if "gx_solid" in r:
        print("Length scale:  c: %g, S: %s | gx[%s]: %s"
              % (opt.length_scale_c, " ".join("%e" % r[k] for k in ("length_S_solid", "length_S_void") if r[k] is not None),
                 ",".join(str(k) for k in opt._k_length), " ".join("%f" % r[k] for k in ("gx_solid", "gx_void") if r[k] is not None)), flush=True)
    if "gx_frequency" in r:
        print("Frequency:     lambda: %s, gap: %f, gx[%d]: %f | subspace iter: %d, solver iter: %d"
              % (" ".join("%e" % v for v in r["eig"]), r["eig_gap"], opt._k_freq, r["gx_frequency"], r["eig_iters"], r["ksp_its_eigen"]), flush=True)
    if "gx_buckling" in r:
        print("Buckling:      mu: %s, load factor: %e, gap: %f, gx[%d]: %f | subspace iter: %d, solver iter: %d"
              % (" ".join("%e" % v for v in r["buckling_mu"]), r["buckling_factor"], r["buckling_gap"], opt._k_buck, r["gx_buckling"],
                 r["buckling_iters"], r["ksp_its_buckling"]), flush=True)
    if "n_active" in r:
        lab = opt.labels_own
        xp = opt.xPhys.cpu().numpy()
        print("Passive:       %d active of %d elements | xPhys exact on the own void elements: %s, solid: %s"
              % (r["n_active"], ex * ey * ez, bool((xp[lab == 1] == 0.0).all()), bool((xp[lab == 2] == 1.0).all())), flush=True)
    if "n_reduced" in r:
        print("Link:          %s | %d reduced of %d design variables" % (" ".join(links), r["n_reduced"], ex * ey * ez), flush=True)
    if "vol_real" in r:
        print("Robust:        eta: %s, beta: %g | volume eroded / nominal / dilated: %s, dilated target: %f"
              % (",".join("%g" % v for v in opt.robust), opt.beta, " ".join("%f" % v for v in r["vol_real"]), r["vol_dilated_target"]), flush=True)
    if "gx_local" in r:
        print("Local volume:  p-norm: %f, max: %f, gx[%d]: %f" % (r["local_pnorm"], r["local_max"], opt.m - 1, r["gx_local"]), flush=True)
