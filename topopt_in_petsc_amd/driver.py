"""The reference's optimisation loop (main.cc:22-141) on top of the MI355X hot path.

`TopOpt` carries the reference's parameters and defaults (TopOpt.cc:102-144) and
`run()` repeats main.cc's STEP 7 loop body:  solve + sensitivities -> objective
scaling -> Filter::Gradients -> move limits -> MMA -> design change -> (beta
continuation) -> FilterProject -> MND, printing the reference's per-iteration line.
Everything stays on the device; the host sees scalars only.
"""
import os
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import mpiio
import ctypes as C

from .api import Casting, Filter, Grid, HeatConduction, LengthScale, LinearElasticity, Link, LocalVolume, MMA, Overhang, Passive, Robust, SolverOptions, _chk, _ptr, check_body_force, check_thermal, parse_link, passive_labels


def robust_volume_target(volfrac, S_d, S_n):
    """V_d*, the volume fraction the DILATED design is held to so that the nominal one meets volfrac: the dilated design holds
    S_d / S_n times the nominal one's material (Wang, Lazarov, Sigmund 2011, section 4)"""
    return volfrac * S_d / S_n


def robust_volume_due(itr, every):
    """whether V_d* is recomputed in design iteration itr (counted from 1): in the first one and in every every-th"""
    return itr == 1 or itr % every == 0


@dataclass
class TopOpt:
    # mesh (TopOpt.cc:106-116; nxyz are NODE counts like -nx -ny -nz)
    nxyz: tuple = (65, 33, 33)
    xc: tuple = (0.0, 2.0, 0.0, 1.0, 0.0, 1.0)
    nu: float = 0.3
    nlvls: int = 4
    # optimisation (TopOpt.cc:118-135)
    volfrac: float = 0.12
    maxItr: int = 400
    rmin: float = 0.08
    penal: float = 3.0
    Emin: float = 1.0e-9
    Emax: float = 1.0
    filter: int = 1
    Xmin: float = 0.0
    Xmax: float = 1.0
    movlim: float = 0.2
    projectionFilter: bool = False
    beta: float = 0.1
    betaFinal: float = 48.0
    eta: float = 0.0
    m: int = 1
    rank: int = 0
    nranks: int = 1
    solver: SolverOptions = None
    # I/O around the loop (main.cc:40, :113-129; TopOpt.cc:400-512): off unless a workdir is given
    workdir: str = None
    output: bool = True            # output_00000.dat (MPIIO container)
    restart: bool = True           # Restart0x.dat / Restart0x_itr_f0.dat / RestartSol0x.dat, alternating
    restartFileVec: str = None     # -restartFileVec / -restartFileItr: continue from these
    restartFileItr: str = None
    restartFileVecSol: str = None  # -restartFileVecSol: the state U (LinearElasticity.cc:590-606)
    onlyLoadDesign: bool = False
    # MMA settings (MMA.h:29-69): None = the values of TopOpt.cc:391-397 (a = 0, c = 1000, d = 0), MMA.cc's asymptote
    # factors 0.5 / 0.7 / 1.2, robust type 0, no constraint modification
    aMMA: object = None
    cMMA: object = None
    dMMA: object = None
    mma_asymptotes: tuple = None
    mma_robust_asymptotes: int = 0
    mma_constraint_modification: bool = False
    kkt: bool = False              # MMA::KKTresidual after every Update -> kkt_norm2 / kkt_normInf in the record
    # further load cases behind the reference's one: a list of (RHS tensor | "top", weight); the objective is the weighted
    # sum of the cases' compliances on the shared supports (None: the reference's single case, nothing changes)
    loadcases: list = None
    # stress constraint: the von Mises p-norm (exponent stress_P, stress relaxation x^stress_q) of load case stress_case held
    # below stress_limit as a second MMA constraint g1 = pnorm / stress_limit - 1 (None: none, nothing changes)
    stress_limit: float = None
    stress_P: float = 8.0
    stress_q: float = 0.5
    stress_case: int = 0
    # local volume constraint: the p-norm (exponent local_volume_p) of the mean density in a ball of radius local_volume_R
    # around every element held below local_volume as an MMA constraint g = pn / local_volume - 1 behind the stress constraint
    # (None: none, nothing changes); the constraints are ordered [volume, stress?, local?, frequency?, solid?, void?]
    local_volume: float = None
    local_volume_R: float = None
    local_volume_p: float = 16.0
    # overhang (self-support) filter: "+z", "-z", "+y" or "-y", the build direction of a part printed layer by layer.  Every
    # response is evaluated on xPrint = Overhang.Forward(xPhys) and its gradient comes back through Overhang.Adjoint (None:
    # xPrint is xPhys itself, nothing changes)
    overhang: str = None
    # casting (draw-direction) filter: "+x" .. "-z", a one-sided mould withdrawn along that axis, or "x:K", "y:K",
    # "z:K", a two-sided one parted between the element layers K - 1 and K.  Every response is evaluated on xPrint = Casting.
    # Forward(xPhys), which has no undercut and no cavity along the axis, and its gradient comes back through Casting.Adjoint.
    # casting_eps: the smoothing of the running maximum; a run of m void cells rises to sqrt(m eps / 2) at most, 0.008 over 128
    # cells at the default.  Not together with overhang: both define xPrint (None: xPrint is xPhys itself, nothing changes)
    casting: str = None
    casting_eps: float = 1e-6
    # self-weight: body_force = (b_x, b_y, b_z), the body force per unit volume at full density (rho g), as a load that moves
    # with xPrint beside the fixed ones; the mass of elements below body_force_xlow is damped.  point_load=False
    # zeroes case 0's fixed load: a part that carries its own weight only (None: no body force, nothing changes)
    body_force: tuple = None
    body_force_xlow: float = 0.1
    point_load: bool = True
    # minimum length scale by geometric constraints: "both", "solid" or "void" adds one MMA constraint per phase
    # behind every other one, g = S / (n length_scale_eps) - 1 on the blueprint (xTilde, xPhys) -- not on xPrint.  length_scale_c:
    # the decay c of exp(-c |grad xTilde|^2) in length^2 (None: rmin^4 / h_min^2, the paper's c = r^4 for r in elements);
    # length_scale_eta: the thresholds (eta_s, eta_v), 0.75 / 0.25 for a length scale equal to the filter size; before iteration
    # length_scale_start the values are recorded but MMA sees g = -1 and a zero row; length_scale_eps = 1e-2 is the value of a
    # measured sweep at which MMA reached feasibility with a structure left, 1e-6 .. 1e-3 did not (None: none, nothing changes)
    length_scale: str = None
    length_scale_c: float = None
    length_scale_eta: tuple = (0.75, 0.25)
    length_scale_eps: float = 1e-2
    length_scale_start: int = 1
    # eigenfrequency constraint: the harmonic mean of the lowest frequency_modes eigenvalues of K phi = lambda M phi
    # (squared angular frequencies; density frequency_rho at x = 1, mass damped below frequency_xlow as for the self-weight) held
    # above frequency_limit as an MMA constraint g = (frequency_limit / nev) sum 1 / lambda_i - 1 behind the local volume's row,
    # on xPrint and the assembly of the state solve; the modes are found by subspace iteration to the residual frequency_tol and
    # warm-started from the previous design iteration (None: none, nothing changes)
    frequency_limit: float = None
    frequency_modes: int = 3
    frequency_rho: float = 1.0
    frequency_xlow: float = 0.1
    frequency_tol: float = 1e-6
    # buckling constraint: the linear buckling load factors of load case buckling_case, 1 / mu_i for the positive
    # eigenvalues of -G(x, u) phi = mu K phi, held above buckling_limit through the p-norm of the buckling_modes largest mu:
    # g = buckling_limit (sum mu_i^buckling_P)^(1/buckling_P) - 1 as an MMA constraint behind the frequency row, on xPrint and the
    # assembly and state of the state solve; the modes are found by subspace iteration to the residual buckling_tol and
    # warm-started from the previous design iteration, the gradient carries an adjoint solve.  For design-independent loads
    # only: not together with body_force or thermoelastic physics (None: none, nothing changes)
    buckling_limit: float = None
    buckling_modes: int = 2
    buckling_P: float = 8.0
    buckling_tol: float = 1e-6
    buckling_case: int = 0
    # the primary load: "cantilever", the reference's line load, or "axial", a uniform traction along -x on the face x = xmax,
    # total 1, behind the same clamped face x = xmin -- a column in compression, the load a buckling user starts from; the name is
    # accepted in loadcases too.  (Under the reference's line load the spectrum of the buckling pencil has both signs with
    # clustered magnitudes -- on 12x8x4 the largest positive mu sits behind five larger negative ones at a ratio of 0.87 -- so the
    # block iteration converges slowly there: a poor first target for the buckling constraint.)
    load: str = "cantilever"
    # passive regions: the global label array (natural order; 0 active, 1 void, 2 solid) or a list of shapes for
    # api.passive_labels.  Void elements are held at x = Xmin, xPhys = 0, solid ones at x = Xmax, xPhys = 1; MMA works on the
    # active elements alone, packed; the volume constraint stays the mean over ALL elements (None: none, nothing changes)
    passive: object = None
    # design-variable linking: per axis "mirror", ("repeat", cells) or "extrude" -- a dict {"y": "mirror"}, or strings
    # "y:mirror", "x:repeat:4", "z:extrude" (one or a list).  MMA works on the reduced design (one variable per orbit); x is its
    # expansion, so the filter and everything behind it see the full field; every gradient row is folded onto the reduced vector
    # in one fixed summation order.  The volume constraint stays the mean over ALL elements.  Not together with passive; a z link
    # needs nranks = 1 (None: none, nothing changes)
    link: object = None
    # robust design: robust = (eta_e, eta_n, eta_d), strictly descending inside (0, 1).  xTilde is projected at the
    # three thresholds with the one beta: xErode, xPhys (the nominal design: output, MND and restart files carry it) and xDilate.
    # The objective is the ERODED design's compliance -- for fixed loads the worst of the three, so one solve per iteration as
    # without -- and the volume is held on the DILATED design at V_d* = volfrac S_d / S_n, recomputed in iteration 1 and every
    # robust_volume_every-th, so that the nominal design meets volfrac.  robust_report = k: every k-th iteration the nominal and
    # the dilated design are solved as well and the record gains f_real (0: never).  (None: none, nothing changes)
    robust: tuple = None
    robust_volume_every: int = 20
    robust_report: int = 0
    # the state problem: "elasticity", or "heat" -- steady conduction with a heat sink and a uniform source (api.
    # HeatConduction.SetUpLoadAndBC), conductivity kmin + xPhys^penal (kmax - kmin), the thermal compliance as the objective.  The
    # filter, the projection, MMA, passive regions, restart files and output are used as they are; after construction `physics` is
    # the solver object, as it always was, and `physics_kind` keeps the name
    physics: str = "elasticity"
    kmin: float = 1.0e-3
    kmax: float = 1.0
    # physics="thermoelastic" (DESIGN 4.18): the cantilever under its point load plus the thermal expansion of a temperature field,
    # beta(x) = alpha (Emin + x^thermal_penal (Emax - Emin)) per unit of T - T_ref (thermal_penal None: penal).  thermal=
    # "conduction": T is solved on the same grid from the heat-sink problem of physics="heat" (kmin, kmax as there) and the
    # sensitivity carries the thermal adjoint; "uniform": T = T_ref + delta_T everywhere, no conduction solve.  After
    # construction `thermal` is the HeatConduction object or None, `thermal_kind` keeps the name
    alpha: float = None
    T_ref: float = 0.0
    thermal_penal: float = None
    thermal: str = "conduction"
    delta_T: float = None
    history: list = field(default_factory=list)

    def __post_init__(self):
        self.physics_kind = self.physics
        if self.physics_kind not in ("elasticity", "heat", "thermoelastic"):
            raise ValueError("physics must be 'elasticity', 'heat' or 'thermoelastic', got %r" % (self.physics,))
        if self.physics_kind == "heat":
            self._check_heat()
        self.thermal_kind = self.thermal
        if self.physics_kind == "thermoelastic":
            self._check_thermoelastic()
        elif self.alpha is not None or self.delta_T is not None:
            raise ValueError("alpha and delta_T belong to physics='thermoelastic', got physics=%r" % (self.physics,))
        if self.robust is not None:
            self._check_robust()
        if self.overhang is not None and self.overhang not in Overhang.BUILDS:
            raise ValueError("overhang must be None or one of %s, got %r" % (", ".join(sorted(Overhang.BUILDS)), self.overhang))
        if self.casting is not None:
            import math
            if self.overhang is not None:
                raise ValueError("casting together with overhang is not supported: both define xPrint")
            Casting.parse(self.casting, tuple(n - 1 for n in self.nxyz))
            if not (isinstance(self.casting_eps, (int, float)) and math.isfinite(self.casting_eps) and self.casting_eps > 0.0):
                raise ValueError("casting_eps must be positive and finite, got %r" % (self.casting_eps,))
        if self.body_force is not None:
            self.body_force, self.body_force_xlow = check_body_force(self.body_force, self.body_force_xlow)
        else:
            check_body_force((0.0, 0.0, 0.0), self.body_force_xlow)
            if not self.point_load:
                raise ValueError("point_load=False needs a body_force: the structure would carry no load")
        if self.length_scale is not None:
            if self.length_scale not in LengthScale.KINDS:
                raise ValueError("length_scale must be None or one of %s, got %r" % (", ".join(sorted(LengthScale.KINDS)), self.length_scale))
            if self.filter == 0:
                raise ValueError("length_scale needs a density or PDE filter: the sensitivity filter (filter=0) has no transpose")
            if self.length_scale_c is not None and not self.length_scale_c > 0.0:
                raise ValueError("length_scale_c must be positive")
            if not self.length_scale_eps > 0.0:
                raise ValueError("length_scale_eps must be positive")
            if len(self.length_scale_eta) != 2 or not all(0.0 < v < 1.0 for v in self.length_scale_eta):
                raise ValueError("length_scale_eta: two thresholds inside (0, 1), got %r" % (self.length_scale_eta,))
            if not self.length_scale_start >= 1:
                raise ValueError("length_scale_start must be at least 1")
        if self.stress_limit is not None:
            if not self.stress_limit > 0.0:
                raise ValueError("stress_limit must be positive")
            self.m = max(self.m, 2)
        self._k_local = None
        if self.local_volume is not None:
            if self.local_volume_R is None:
                raise ValueError("local_volume needs local_volume_R")
            if not self.local_volume > 0.0 or not self.local_volume_R > 0.0:
                raise ValueError("local_volume and local_volume_R must be positive")
            self._k_local = 2 if self.stress_limit is not None else 1
            self.m = max(self.m, self._k_local + 1)
        self._k_freq = None
        if self.frequency_limit is not None:
            import math
            if not (self.frequency_limit > 0.0 and math.isfinite(self.frequency_limit)):
                raise ValueError("frequency_limit must be positive and finite")
            if not (self.frequency_rho > 0.0 and math.isfinite(self.frequency_rho)):
                raise ValueError("frequency_rho must be positive and finite")
            if not 1 <= int(self.frequency_modes) <= 6:
                raise ValueError("frequency_modes: 1 to 6 (the block of frequency_modes + 2 vectors holds at most 8)")
            if not 0.0 <= self.frequency_xlow < 1.0:
                raise ValueError("frequency_xlow must lie in [0, 1)")
            if not self.frequency_tol > 0.0:
                raise ValueError("frequency_tol must be positive")
            self.frequency_modes = int(self.frequency_modes)
            self._k_freq = 1 + (self.stress_limit is not None) + (self.local_volume is not None)
            self.m = max(self.m, self._k_freq + 1)
        if self.load not in ("cantilever", "axial"):
            raise ValueError("load must be 'cantilever' or 'axial', got %r" % (self.load,))
        if self.load == "axial" and self.physics_kind == "heat":
            raise ValueError("load='axial' belongs to the elastic problems, got physics='heat'")
        self._k_buck = None
        if self.buckling_limit is not None:
            import math
            if not (self.buckling_limit > 0.0 and math.isfinite(self.buckling_limit)):
                raise ValueError("buckling_limit must be positive and finite")
            if isinstance(self.buckling_modes, bool) or int(self.buckling_modes) != self.buckling_modes or not 1 <= self.buckling_modes <= 4:
                raise ValueError("buckling_modes: 1 to 4 (the block of 8 vectors keeps as many again for the negative eigenvalues)")
            if not (self.buckling_P >= 1.0 and math.isfinite(self.buckling_P)):
                raise ValueError("buckling_P must be at least 1 and finite")
            if not (self.buckling_tol > 0.0 and math.isfinite(self.buckling_tol)):
                raise ValueError("buckling_tol must be positive and finite")
            ncases = 1 + len(self.loadcases or ())
            if isinstance(self.buckling_case, bool) or int(self.buckling_case) != self.buckling_case or not 0 <= self.buckling_case < ncases:
                raise ValueError("buckling_case must name one of the %d load cases" % ncases)
            if self.body_force is not None:
                raise ValueError("buckling_limit together with body_force is not supported: the gradient holds for a design-independent load")
            self.buckling_modes, self.buckling_case = int(self.buckling_modes), int(self.buckling_case)
            self._k_buck = 1 + (self.stress_limit is not None) + (self.local_volume is not None) + (self.frequency_limit is not None)
            self.m = max(self.m, self._k_buck + 1)
        nx, ny, nz = self.nxyz
        h = ((self.xc[1] - self.xc[0]) / (nx - 1), (self.xc[3] - self.xc[2]) / (ny - 1),
             (self.xc[5] - self.xc[4]) / (nz - 1))
        self._k_length = ()
        if self.length_scale is not None:   # the rows behind every other one
            nk = 2 if self.length_scale == "both" else 1
            self._k_length = tuple(range(self.m, self.m + nk))
            self.m += nk
            if self.length_scale_c is None:
                self.length_scale_c = self.rmin ** 4 / min(h) ** 2
        labels = self._check_passive() if self.passive is not None else None
        if self.link is not None:
            self._check_link()
        self.grid = Grid(nx, ny, nz, h, rank=self.rank, nranks=self.nranks)
        so = self.solver or SolverOptions(nlvls=self.nlvls, nu=self.nu)
        self.physics = (HeatConduction if self.physics_kind == "heat" else LinearElasticity)(self.grid, so)
        if self.load == "axial":
            self.physics.SetUpLoadAndBC_Axial()
        else:
            self.physics.SetUpLoadAndBC()
        if self.physics_kind == "thermoelastic":
            self._setup_thermoelastic(so)
        else:
            self.thermal = None
        # the material interpolation's end values as the physics takes them
        self._dof = 1 if self.physics_kind == "heat" else 3
        self._mat = (self.kmin, self.kmax) if self.physics_kind == "heat" else (self.Emin, self.Emax)
        if self.body_force is not None:
            self.physics.SetBodyForce(self.body_force, self.body_force_xlow)
            self._f_body = self.grid.node_vec(3)
            if not self.point_load:
                self.physics.RHS.zero_()
        for rhs, weight in (self.loadcases or ()):
            if isinstance(rhs, str):
                if rhs == "axial":
                    self.physics.AddLoadCase(self.physics.AxialLoad(), weight)
                elif rhs == "top":
                    self.physics.SetUpLoadAndBC_Top(weight)
                else:
                    raise ValueError("unknown load case %r (the names are 'top' and 'axial')" % (rhs,))
            else:
                self.physics.AddLoadCase(rhs, weight)
        self.filt = Filter(self.grid, self.filter, self.rmin)
        self.localvol = LocalVolume(self.grid, self.local_volume_R) if self.local_volume is not None else None
        self.overhang_filter = Overhang(self.grid, self.overhang) if self.overhang is not None else None
        self.lengthscale = LengthScale(self.grid) if self.length_scale is not None else None
        self.casting_filter = None
        if self.casting is not None:
            self.casting_filter = Casting(self.grid, self.casting)
            self.casting_filter.params(self.casting_eps)
        g = self.grid
        # TopOpt.cc:362-381: all design fields start at volfrac
        self.x = g.elem_vec(self.volfrac)
        self.xTilde, self.xPhys = g.elem_vec(self.volfrac), g.elem_vec(self.volfrac)
        self.xPrint = g.elem_vec(self.volfrac) if (self.overhang_filter or self.casting_filter) is not None else self.xPhys
        self.projector, self.vd_target, self._S = None, None, None
        if self.robust is not None:
            self.projector = Robust(g)
            self.xErode, self.xDilate = g.elem_vec(self.volfrac), g.elem_vec(self.volfrac)
            self._U_real = {1: None, 2: None}   # the nominal and the dilated design's states, robust_report's warm starts
        self.dfdx, self.dgdx = g.elem_vec(), [g.elem_vec() for _ in range(self.m)]
        # what MMA works on: the fields themselves, or with passive regions the packed vectors of the active elements
        self.regions, n_mma = None, None
        self._xd, self._dfd, self._dgd = self.x, self.dfdx, self.dgdx
        new = g.elem_vec
        if labels is not None:
            n_own = g.part.n_own_elems
            self.labels_own = labels[self.rank * n_own:(self.rank + 1) * n_own]
            self.regions = pr = Passive(g, self.labels_own)
            self.x.fill_(self._x0)
            pr.Impose([self.x], self.Xmin, self.Xmax)   # once: the filter sees the fixed neighbours
            new, n_mma = pr.packed_vec, self.n_active
            self.xa = self._xd = new(self._x0)
            self._dfd, self._dgd = new(), [new() for _ in range(self.m)]
        self.linker = None
        if self.link is not None:   # MMA on the reduced design; x, which starts uniform, is its expansion already
            self.linker = lk = Link(g, self.link)
            new, n_mma = lk.reduced_vec, self.n_reduced
            self.xr = self._xd = new(self.volfrac)
            self._dfd, self._dgd = new(), [new() for _ in range(self.m)]
        self.xmin, self.xmax, self.xold = new(), new(), new(self.volfrac if labels is None else self._x0)
        if self.aMMA is None and self.cMMA is None and self.dMMA is None:
            self.mma = MMA(g, self._xd, self.m, n_global=n_mma)
        else:
            self.mma = MMA(g, self._xd, self.m, n_global=n_mma, a=0.0 if self.aMMA is None else self.aMMA,
                           c=1000.0 if self.cMMA is None else self.cMMA, d=0.0 if self.dMMA is None else self.dMMA)
        if self.mma_asymptotes is not None:
            self.mma.SetAsymptotes(*self.mma_asymptotes)
        if self.mma_robust_asymptotes:
            self.mma.SetRobustAsymptotesType(self.mma_robust_asymptotes)
        if self.mma_constraint_modification:
            self.mma.ConstraintModification(True)
        self.fscale = 1.0
        self.itr = 0
        self._flip = True
        self._out = None
        if self.workdir is not None:
            os.makedirs(self.workdir, exist_ok=True)
            if self.output:
                self._out = mpiio.MPIIO(g.part, h, filename=os.path.join(self.workdir, "output_00000.dat"),
                                        xc0=(self.xc[0], self.xc[2], self.xc[4]))
        if self.restartFileVec and self.restartFileItr and os.path.exists(self.restartFileVec) \
                and os.path.exists(self.restartFileItr):
            self.ReadRestartFiles(self.restartFileVec, self.restartFileItr, self.restartFileVecSol)
        # main.cc:48
        self._filter_project()
        if self.robust is not None and self.vd_target is None:
            self.vd_target = robust_volume_target(self.volfrac, self._S[2], self._S[1])

    def _check_heat(self):
        """heat conduction's refusals; host arithmetic on the parameters, before any device object"""
        import math
        for name, what in (("loadcases", "further load cases"), ("stress_limit", "the stress constraint"), ("body_force", "self-weight"),
                           ("frequency_limit", "the eigenfrequency constraint"), ("buckling_limit", "the buckling constraint"), ("robust", "robust design"),
                           ("overhang", "the overhang filter"), ("casting", "the casting filter"),
                           ("local_volume", "the local volume constraint"), ("length_scale", "the length-scale constraints")):
            if getattr(self, name) is not None:
                raise ValueError("physics='heat' together with %s (%s) is not supported" % (name, what))
        if not self.point_load:
            raise ValueError("physics='heat' has no point_load switch: the source is the built-in uniform one")
        if not (math.isfinite(self.kmin) and math.isfinite(self.kmax) and self.kmin > 0.0 and self.kmax > self.kmin):
            raise ValueError("physics='heat' needs 0 < kmin < kmax, both finite; got %r, %r" % (self.kmin, self.kmax))
        if not (math.isfinite(self.penal) and self.penal >= 1.0):
            raise ValueError("physics='heat' needs penal >= 1, got %r" % (self.penal,))

    def _check_thermoelastic(self):
        """the thermoelastic problem's refusals; host arithmetic on the parameters, before any device object"""
        import math
        for name, what in (("loadcases", "further load cases"), ("stress_limit", "the stress constraint"), ("body_force", "self-weight"),
                           ("frequency_limit", "the eigenfrequency constraint"), ("buckling_limit", "the buckling constraint"), ("robust", "robust design"),
                           ("overhang", "the overhang filter"), ("casting", "the casting filter"),
                           ("local_volume", "the local volume constraint"), ("length_scale", "the length-scale constraints")):
            if getattr(self, name) is not None:
                raise ValueError("physics='thermoelastic' together with %s (%s) is not supported" % (name, what))
        if self.alpha is None:
            raise ValueError("physics='thermoelastic' needs alpha, the thermal stress coefficient at Emax per unit of temperature")
        if self.thermal_kind not in ("conduction", "uniform"):
            raise ValueError("thermal must be 'conduction' or 'uniform', got %r" % (self.thermal_kind,))
        if self.thermal_kind == "uniform":
            if self.delta_T is None or not math.isfinite(float(self.delta_T)):
                raise ValueError("thermal='uniform' needs a finite delta_T, the temperature rise above T_ref")
            self.delta_T = float(self.delta_T)
        else:
            if self.delta_T is not None:
                raise ValueError("delta_T belongs to thermal='uniform': with thermal='conduction' the temperature is solved for")
            if not (math.isfinite(self.kmin) and math.isfinite(self.kmax) and self.kmin > 0.0 and self.kmax > self.kmin):
                raise ValueError("thermal='conduction' needs 0 < kmin < kmax, both finite; got %r, %r" % (self.kmin, self.kmax))
        if not (math.isfinite(self.penal) and self.penal >= 1.0):
            raise ValueError("physics='thermoelastic' needs penal >= 1, got %r" % (self.penal,))
        self._thermal_par = check_thermal(self.alpha, self.T_ref, self.penal if self.thermal_penal is None else self.thermal_penal,
                                          self.Emin, self.Emax)

    def _setup_thermoelastic(self, so):
        """the second state problem on the SAME grid, the temperature field the elastic load reads, the thermal adjoint's vectors"""
        g, ph = self.grid, self.physics
        alpha, T_ref, Emin, Emax, pb = self._thermal_par
        ph.SetThermalExpansion(alpha, T_ref, pb, Emin, Emax)
        if self.thermal_kind == "conduction":
            self.thermal = HeatConduction(g, so)
            self.thermal.SetUpLoadAndBC()
            ph.SetTemperature(self.thermal.T)
            # mu persists like the states (warm start across design iterations); the ghost planes of its load stay 0
            self.mu, self._g_th, self._df_th = g.node_vec(1), g.node_vec(1), g.elem_vec()
        else:
            self.thermal = None
            self._T_uniform = g.node_vec(1)
            self._T_uniform.fill_(T_ref + self.delta_T)
            ph.SetTemperature(self._T_uniform)

    def _thermoelastic_step(self):
        """conduction solve -> thermal load and elastic solve -> compliance and its sensitivity at fixed T (the load's term with
        factor 2 inside) -> the thermal adjoint's right-hand side, its solve and the conduction response with weight 2 -> (fx, gx)"""
        ph, th, x = self.physics, self.thermal, self.xPrint
        self._its_thermal = self._its_thermal_adjoint = 0
        if th is not None:
            self._its_thermal = th.SolveState(x, self.kmin, self.kmax, self.penal)
        fx, gx = ph.ComputeObjectiveConstraintsSensitivities(self.dfdx, self.dgdx[0], x, self.Emin, self.Emax, self.penal, self.volfrac)
        if th is not None:
            ph.ThermalAdjointRHS([ph.U], None, x, 1.0, self._g_th)
            self._its_thermal_adjoint = th.SolveAdjoint(self._g_th, self.mu)
            # (tp_conduction_response overwrites its dfdx: through a scratch vector)
            th.Response([th.T], [self.mu], [2.0], x, self.kmin, self.kmax, self.penal, 0.0, dfdx=self._df_th, sums=False)
            self.dfdx.add_(self._df_th)
        return fx, gx

    def _T_max(self):
        """the largest temperature of the field the load was formed from, all ranks"""
        if self.thermal is None:
            return self.T_ref + self.delta_T
        m = float(self.thermal.T[self.grid.part.owned_slice(1)].max())
        if self.nranks == 1:
            return m
        import torch.distributed as dist
        parts = [None] * self.nranks
        dist.all_gather_object(parts, m)
        return max(parts)

    def _check_robust(self):
        """robust mode's refusals; host arithmetic on the parameters, before any device object"""
        import math
        try:
            etas = tuple(float(v) for v in self.robust)
        except (TypeError, ValueError):
            raise ValueError("robust: need three thresholds (eta_e, eta_n, eta_d), got %r" % (self.robust,))
        if len(etas) != 3 or not all(math.isfinite(v) for v in etas) or not 1.0 > etas[0] > etas[1] > etas[2] > 0.0:
            raise ValueError("robust: need 1 > eta_e > eta_n > eta_d > 0, got %r" % (self.robust,))
        if not self.projectionFilter:
            raise ValueError("robust needs projectionFilter=True: the three designs are projections of xTilde")
        if self.filter == 0:
            raise ValueError("robust needs a density or PDE filter: the sensitivity filter (filter=0) has no transpose")
        if self.eta != 0.0 and self.eta != etas[1]:
            raise ValueError("robust: eta = %r is neither its default nor eta_n = %r (xPhys is the nominal design)" % (self.eta, etas[1]))
        if isinstance(self.robust_volume_every, bool) or int(self.robust_volume_every) != self.robust_volume_every \
                or self.robust_volume_every < 1:
            raise ValueError("robust_volume_every must be a whole number of at least 1")
        if isinstance(self.robust_report, bool) or int(self.robust_report) != self.robust_report or self.robust_report < 0:
            raise ValueError("robust_report must be a whole number, 0 for never")
        if self.body_force is not None:
            raise ValueError("robust together with body_force is not supported: with a load that grows with the density the "
                             "eroded design is no longer the worst of the three")
        for name in ("stress_limit", "local_volume", "frequency_limit", "buckling_limit", "overhang", "casting", "length_scale"):
            if getattr(self, name) is not None:
                raise ValueError("robust together with %s is not supported: the constraint would have to choose a realisation" % name)
        self.robust, self.eta = etas, etas[1]
        self.robust_volume_every, self.robust_report = int(self.robust_volume_every), int(self.robust_report)

    def _check_link(self):
        """linking's refusals and the global reduced count n_reduced; host arithmetic on the parameters, before any device object"""
        if self.passive is not None:
            raise ValueError("link together with passive regions is not supported")
        ne = tuple(n - 1 for n in self.nxyz)
        modes, cells = parse_link(self.link, ne)
        if modes[2] != 0 and self.nranks > 1:
            raise ValueError("link: a z link needs nranks = 1 (its orbits would cross the slabs), got nranks = %d" % self.nranks)
        if self.m + 1 > Link.MAXVEC:
            raise ValueError("link: the objective's row and %d constraint rows are more than one Fold takes (%d)" % (self.m, Link.MAXVEC))
        nr = [n if mo == 0 else (n + 1) // 2 if mo == 1 else n // c if mo == 2 else 1 for n, mo, c in zip(ne, modes, cells)]
        self.n_reduced = nr[0] * nr[1] * nr[2]

    def _check_passive(self):
        """the global label array of `passive`, checked; sets n_active (global) and the active elements' start value _x0.
        Everything here is host arithmetic on the global labels: it comes before any device object and needs no communication"""
        nx, ny, nz = self.nxyz
        n = (nx - 1) * (ny - 1) * (nz - 1)
        p = self.passive
        if isinstance(p, (list, tuple)) and (len(p) == 0 or isinstance(p[0], (list, tuple))):
            p = passive_labels(self.nxyz, self.xc, p)
        lab = np.asarray(p)
        if lab.ndim != 1 or lab.size != n:
            raise ValueError("passive: need %d labels (all elements, natural order), got an array of shape %r" % (n, lab.shape))
        if lab.size and (lab.min() < 0 or lab.max() > 2):
            raise ValueError("passive: labels are 0 (active), 1 (void) or 2 (solid)")
        lab = np.ascontiguousarray(lab, dtype=np.uint8)
        if self.length_scale is not None:
            raise ValueError("length_scale together with passive regions is not supported: its constraints differentiate xPhys "
                             "with respect to xTilde on every element")
        n_active, n_solid = int((lab == 0).sum()), int((lab == 2).sum())
        if n_active == 0:
            raise ValueError("passive: no active element is left")
        if (nz - 1) % self.nranks == 0:   # (otherwise the grid refuses the slabs)
            per = lab.reshape(self.nranks, -1)
            empty = [r for r in range(self.nranks) if per[r].all()]
            if empty:
                raise ValueError("passive: the slab of rank %s has no active element" % ", ".join(str(r) for r in empty))
        if n_solid / n >= self.volfrac:
            raise ValueError("passive: the solid elements alone fill %.4f of the volume, volfrac is %.4f" % (n_solid / n, self.volfrac))
        # the volume constraint starts at equality, as in the reference; without passive elements this is volfrac itself
        self._x0 = self.volfrac if n_active == n else (self.volfrac * n - n_solid) / n_active
        if not self.Xmin <= self._x0 <= self.Xmax:
            raise ValueError("passive: the active elements would start at %.4f, outside [Xmin, Xmax] = [%g, %g]" % (self._x0, self.Xmin, self.Xmax))
        self.n_active = n_active
        return lab

    def _filter_project(self):
        """x -> xTilde -> xPhys (main.cc:48, :98), the passive values imposed on xPhys (xTilde stays as filtered), then xPrint; in
        robust mode x -> xTilde -> (xErode, xPhys, xDilate) and their sums"""
        if self.projector is not None:   # the filter alone, then the three projections, the passive values and the sums at once
            self.filt.FilterProject(self.x, self.xTilde, self.xPhys, False)
            self._S = self.projector.Project(self.xTilde, self.beta, self.robust, [self.xErode, self.xPhys, self.xDilate],
                                             passive=self.regions, sums=True)
            return
        self.filt.FilterProject(self.x, self.xTilde, self.xPhys, self.projectionFilter, self.beta, self.eta)
        if self.regions is not None:
            self.regions.Impose([self.xPhys], 0.0, 1.0)
        self._print()

    def _body_share(self):
        """(f_body^T u) / (f_total^T u) of load case 0 on the state just solved, owned node range, all ranks"""
        ph, sl = self.physics, self.grid.part.owned_slice(3)
        ph.BodyLoad(self.xPrint, self._f_body)
        u, out = ph.U[sl], []
        for f in (self._f_body[sl], ph.TotalRHS(0)[sl]):
            v = C.c_double()
            _chk(self.grid.L.tp_vec_dot(self.grid.handle, _ptr(f), _ptr(u), u.numel(), C.byref(v)), "tp_vec_dot")
            out.append(v.value)
        return out[0] / out[1]

    def _solve_realisations(self, f_e):
        """-> [f_e, f_n, f_d]: the nominal and the dilated design solved beside the eroded one, each warm-started from its own
        states of the last report; the eroded design's states and the physics' records of its solve come back as they were"""
        ph = self.physics
        names = ("last_its", "last_rnorm", "last_bnorm", "last_hist", "last_solve_s", "last_f_case")
        kept = {k: getattr(ph, k) for k in names if hasattr(ph, k)}
        lists = {k: list(getattr(ph, k)) for k in ("case_its", "case_rnorm", "case_bnorm")}
        U_e = [ph.LoadCaseU(c).clone() for c in range(ph.ncases)]
        out = [f_e]
        for k, field in ((1, self.xPhys), (2, self.xDilate)):
            if self._U_real[k] is not None:
                for c, u in enumerate(self._U_real[k]):
                    ph.LoadCaseU(c).copy_(u)
            out.append(ph.ComputeObjectiveConstraints(field, self.Emin, self.Emax, self.penal, self.volfrac)[0])
            self._U_real[k] = [ph.LoadCaseU(c).clone() for c in range(ph.ncases)]
        for c, u in enumerate(U_e):
            ph.LoadCaseU(c).copy_(u)
        for k, v in kept.items():
            setattr(ph, k, v)
        for k, v in lists.items():
            getattr(ph, k)[:] = v
        return out

    def _print(self):
        """xPrint follows every FilterProject"""
        if self.overhang_filter is not None:
            self.overhang_filter.Forward(self.xPhys, self.xPrint)
        if self.casting_filter is not None:
            self.casting_filter.Forward(self.xPhys, self.xPrint)

    def step(self, verbose=False):
        """one pass of the loop body, main.cc:54-111; returns the record of this iteration"""
        self.itr += 1
        t1 = time.perf_counter()
        if self.physics_kind == "thermoelastic":
            fx, gx = self._thermoelastic_step()
        else:
            fx, gx = self.physics.ComputeObjectiveConstraintsSensitivities(
                self.dfdx, self.dgdx[0], self.xPrint if self.robust is None else self.xErode, self._mat[0], self._mat[1], self.penal,
                self.volfrac)                                                                    # main.cc:62
        if self.robust is not None:   # the volume on the dilated design, against V_d*
            S, n_glob = list(self._S), self.grid.part.n_own_elems * self.nranks
            if robust_volume_due(self.itr, self.robust_volume_every):
                self.vd_target = robust_volume_target(self.volfrac, S[2], S[1])
            gx = S[2] / (n_glob * self.vd_target) - 1.0
            self.dgdx[0].fill_(1.0 / (n_glob * self.vd_target))
            if self.robust_report and self.itr % self.robust_report == 0:
                f_real = self._solve_realisations(fx)
        if self.body_force is not None:   # (before xPrint moves on)
            body_share = self._body_share()
        if self.physics_kind == "thermoelastic":
            T_max = self._T_max()
        if self.itr == 1:
            self.fscale = 10.0 / fx                                                              # :68-70
        fxs = fx * self.fscale
        self.dfdx.mul_(self.fscale)                                                              # :73
        gxs = [gx]
        if self.stress_limit is not None:   # second constraint on the assembly and state of the solve above
            pnorm, vm_max, its_adj = self.physics.StressSensitivity(self.dgdx[1], self.xPrint, self.Emin, self.Emax, self.penal,
                                                                    self.stress_q, self.stress_P, self.stress_case)
            self.dgdx[1].div_(self.stress_limit)
            gxs.append(pnorm / self.stress_limit - 1.0)
        if self.localvol is not None:       # last constraint, on the density alone
            g_local, pn_local, rb_max = self.localvol.Constraint(self.xPrint, self.local_volume, self.local_volume_p,
                                                                 dgdx=self.dgdx[self._k_local])
            gxs.append(g_local)
        if self.frequency_limit is not None:   # on the assembly of the state solve above; the block of modes warm-starts
            eig = self.physics.Eigenmodes(self.frequency_modes, self.xPrint, self.frequency_rho, self.frequency_xlow,
                                          tol=self.frequency_tol)
            row = self.dgdx[self._k_freq]
            J = self.physics.EigenSensitivity(row, self.xPrint, self.Emin, self.Emax, self.penal)
            row.mul_(self.frequency_limit / self.frequency_modes)
            g_freq = self.frequency_limit / self.frequency_modes * J - 1.0
            gxs.append(g_freq)
        if self.buckling_limit is not None:    # on the assembly and the state of the solve above; modes and adjoint warm-start
            ph = self.physics
            buck = ph.BucklingModes(self.buckling_modes, self.xPrint, self.Emax, self.penal, U=ph.LoadCaseU(self.buckling_case),
                                    tol=self.buckling_tol)
            row = self.dgdx[self._k_buck]
            J_buck, its_buck = ph.BucklingSensitivity(row, self.xPrint, self.Emin, self.Emax, self.penal, self.buckling_P)
            row.mul_(self.buckling_limit)
            g_buck = self.buckling_limit * J_buck - 1.0
            gxs.append(g_buck)
        rows = self.dgdx   # what goes back through the overhang filter and the projection: every row but the length scale's
        if self.lengthscale is not None:    # on the blueprint (xTilde, xPhys); d/dxTilde, the projection's derivative inside
            rows, lrows = self.dgdx[:self._k_length[0]], [self.dgdx[k] for k in self._k_length]
            solid, void = self.length_scale != "void", self.length_scale != "solid"
            ls = self.lengthscale.Constraints(self.xTilde, self.xPhys, self.length_scale_c, self.length_scale_eta[0],
                                              self.length_scale_eta[1], self.length_scale_eps, self.length_scale,
                                              self.projectionFilter, self.beta, self.eta,
                                              dg_solid=lrows[0] if solid else None, dg_void=lrows[-1] if void else None)
            g_length = [ls[k] for k, on in (("g_solid", solid), ("g_void", void)) if on]
            if self.itr < self.length_scale_start:   # recorded, but not yet held
                gxs.extend(-1.0 for _ in g_length)
                for r in lrows:
                    r.zero_()
            else:
                gxs.extend(g_length)
        if self.overhang_filter is not None:   # d/dxPrint -> d/dxPhys, all of them in one sweep
            self.overhang_filter.Adjoint([self.dfdx] + rows)
        if self.casting_filter is not None:
            self.casting_filter.Adjoint([self.dfdx] + rows)
        if self.robust is not None:    # d/dxErode and d/dxDilate -> d/dxTilde, passive entries zeroed, in one launch; then the filter
            self.projector.Chain(self.xTilde, self.beta, [self.dfdx, self.dgdx[0]], [self.robust[0], self.robust[2]], passive=self.regions)
            self.filt.GradientsFromTilde(self.x, [self.dfdx, self.dgdx[0]])
        else:
            if self.regions is not None:   # the rows are d/dxPhys now, and xPhys does not move on passive elements
                self.regions.Zero([self.dfdx] + rows)
            self.filt.Gradients(self.x, self.xTilde, self.dfdx, rows, self.projectionFilter, self.beta, self.eta)
        if self.lengthscale is not None:
            self.filt.GradientsFromTilde(self.x, lrows)
        if self.regions is not None:   # the active entries of the objective's row and every constraint's, one launch
            self.regions.Gather([self.dfdx] + self.dgdx, [self._dfd] + self._dgd)
        if self.linker is not None:    # every row summed over the orbits of the reduced variables, one launch
            self.linker.Fold([self.dfdx] + self.dgdx, [self._dfd] + self._dgd)
        self.mma.SetOuterMovelimit(self.Xmin, self.Xmax, self.movlim, self._xd, self.xmin, self.xmax)  # :81
        self.mma.Update(self._xd, self._dfd, gxs, self._dgd, self.xmin, self.xmax)               # :85
        if self.regions is not None:
            self.regions.Scatter([self.xa], [self.x])
        if self.linker is not None:
            self.linker.Expand([self.xr], [self.x])
        if self.kkt:
            kkt = self.mma.KKTresidual(self._xd, self._dfd, gxs, self._dgd, self.xmin, self.xmax)
        ch = self.mma.DesignChange(self._xd, self.xold)                                          # :89
        if self.projectionFilter:                                                                # :93-95
            self._increase_beta(gx, ch)
        self._filter_project()                                                                   # :98
        mnd = self.filt.GetMND(self.xPrint)                                                      # :102
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        rec = dict(itr=self.itr, fx=fx, fx_scaled=fxs, gx=gx, ch=ch, mnd=mnd, time=t2 - t1,
                   ksp_its=self.physics.last_its, ksp_rerr=self.physics.last_rnorm / self.physics.last_bnorm,
                   mma_inner=self.mma.last_inner)
        if self.kkt:
            rec["kkt_norm2"], rec["kkt_normInf"] = kkt
        if self.physics.ncases > 1:   # ksp_its: the sum over the cases; ksp_rerr: the last case's
            rec["f_case"] = list(self.physics.last_f_case)
            rec["ksp_its_case"] = list(self.physics.case_its)
            rec["ksp_its"] = sum(self.physics.case_its)
        if self.stress_limit is not None:
            rec["stress_pnorm"], rec["stress_max"], rec["gx_stress"], rec["ksp_its_adjoint"] = pnorm, vm_max, gxs[1], its_adj
        if self.localvol is not None:
            rec["gx_local"], rec["local_pnorm"], rec["local_max"] = g_local, pn_local, rb_max
        if self.frequency_limit is not None:
            rec["eig"], rec["gx_frequency"], rec["eig_iters"] = list(eig["lam"]), g_freq, eig["iters"]
            rec["ksp_its_eigen"], rec["eig_gap"] = eig["ksp_its"], eig["gap"]
        if self.buckling_limit is not None:
            rec["buckling_mu"], rec["buckling_factor"], rec["gx_buckling"] = list(buck["mu"]), buck["factor"], g_buck
            rec["buckling_iters"], rec["ksp_its_buckling"], rec["buckling_gap"] = buck["iters"], buck["ksp_its"] + its_buck, buck["gap"]
        if self.lengthscale is not None:
            rec["gx_solid"], rec["gx_void"] = ls["g_solid"], ls["g_void"]
            rec["length_S_solid"], rec["length_S_void"] = ls["S_solid"], ls["S_void"]
        if self.overhang_filter is not None:
            rec["print_loss"] = self._mean(self.xPhys - self.xPrint)
        if self.casting_filter is not None:
            rec["cast_fill"] = self._mean(self.xPrint - self.xPhys)
        if self.body_force is not None:
            rec["body_share"] = body_share
        if self.physics_kind == "thermoelastic":
            rec["ksp_its_thermal"], rec["ksp_its_thermal_adjoint"], rec["T_max"] = self._its_thermal, self._its_thermal_adjoint, T_max
        if self.regions is not None:
            rec["n_active"] = self.n_active
        if self.linker is not None:
            rec["n_reduced"] = self.n_reduced
        if self.robust is not None:   # of the design fx and gx belong to
            rec["vol_real"], rec["vol_dilated_target"] = [v / n_glob for v in S], self.vd_target
            if self.robust_report and self.itr % self.robust_report == 0:
                rec["f_real"] = f_real
        self.history.append(rec)
        if verbose and self.rank == 0:
            print("It.: %i, True fx: %f, Scaled fx: %f, gx[0]: %f, ch.: %f, mnd.: %f, time: %f"
                  % (self.itr, fx, fxs, gx, ch, mnd, t2 - t1), flush=True)                        # :108-111
        return rec

    # ---- restart / output (host-side I/O; vectors gathered in natural = rank order) ----
    def _gather(self, t):
        a = t.detach().cpu().numpy()
        if self.nranks == 1:
            return a
        import torch.distributed as dist
        parts = [None] * self.nranks
        dist.all_gather_object(parts, a)
        return np.concatenate(parts)

    def _mean(self, t):
        """mean over the elements of all ranks (the slabs are equally thick)"""
        m = float(t.mean())
        if self.nranks == 1:
            return m
        import torch.distributed as dist
        parts = [None] * self.nranks
        dist.all_gather_object(parts, m)
        return sum(parts) / self.nranks

    def _own(self, a):
        n = self.grid.part.n_own_elems
        return torch.from_numpy(np.ascontiguousarray(a[self.rank * n:(self.rank + 1) * n])).to(self.x.device)

    def WriteRestartFiles(self):
        """TopOpt::WriteRestartFiles (TopOpt.cc:514-570) + LinearElasticity::WriteRestartFiles (:447-478)"""
        if self.workdir is None or not self.restart:
            return None
        self._flip = not self._flip
        tag = "01" if self._flip else "00"
        g = self.grid
        xo1, xo2, U, L = g.elem_vec(), g.elem_vec(), g.elem_vec(), g.elem_vec()
        if self.linker is not None:   # the files keep their full-length layout: MMA's reduced vectors expanded
            reduced = [self.linker.reduced_vec() for _ in range(4)]
            self.mma.Restart(*reduced)
            self.linker.Expand(reduced, [xo1, xo2, U, L])
        elif self.regions is None:
            self.mma.Restart(xo1, xo2, U, L)
        else:   # the files keep their full-length layout: MMA's packed vectors into zero-filled full ones
            packed = [self.regions.packed_vec() for _ in range(4)]
            self.mma.Restart(*packed)
            self.regions.Scatter(packed, [xo1, xo2, U, L])
        vecs = [self._gather(v) for v in (self.x, self.xPhys, xo1, xo2, U, L)]
        # the further cases' states follow the first Vec (the reference's reader takes the first one only)
        sols = [self._gather(self.physics.LoadCaseU(c)[self.grid.part.owned_slice(self._dof)]) for c in range(self.physics.ncases)]
        prefix = os.path.join(self.workdir, "Restart" + tag)
        if self.rank == 0:
            mpiio.write_restart(prefix, self.itr, self.fscale, *vecs)
            if self.robust is not None:   # V_d* is part of the loop's state between its updates: a third number, all digits
                with open(prefix + "_itr_f0.dat", "w") as f:
                    f.write("%d  %e  %.17e\n" % (self.itr, self.fscale, self.vd_target))
            mpiio.write_petsc_vecs(os.path.join(self.workdir, "RestartSol%s.dat" % tag), sols)
        return prefix

    def ReadRestartFiles(self, vecfile, itrfile, solfile=None):
        """TopOpt::AllocateMMAwithRestart (TopOpt.cc:474-507); solfile = -restartFileVecSol (LinearElasticity.cc:590-606)"""
        x, xPhys, xo1, xo2, U, L = mpiio.read_petsc_vecs(vecfile)
        if self.robust is None:
            itr, fscale = open(itrfile).read().split()
        else:   # a file of a run without `robust` has two numbers: V_d* then comes from the design that was read
            itr, fscale, *vd = open(itrfile).read().split()
            self.vd_target = float(vd[0]) if vd else None
        self.x.copy_(self._own(x))
        self.xPhys.copy_(self._own(xPhys))
        self.fscale = float(fscale)
        self.itr = int(itr)
        if self.regions is not None:   # the files are full length: the design on the active elements ...
            self.regions.Gather([self.x], [self.xa])
        if self.linker is not None:    # the reduced design is the orbits' first members
            self.linker.Pick([self.x], [self.xr])
            self.linker.Expand([self.xr], [self.x])   # (a file of a run without link: x becomes the linked design of its first members)
        if not self.onlyLoadDesign:
            state = [self._own(xo1), self._own(xo2), self._own(U), self._own(L)]
            if self.linker is not None:
                state = self.linker.Pick(state, [self.linker.reduced_vec() for _ in range(4)])
            if self.regions is not None:   # ... and MMA's vectors
                state = self.regions.Gather(state, [self.regions.packed_vec() for _ in range(4)])
            self.mma.SetRestart(self.itr, *state)
        if solfile and os.path.exists(solfile):
            sols = mpiio.read_petsc_vecs(solfile)   # a file with fewer states than cases leaves the others at zero
            sl = self.grid.part.owned_slice(self._dof)
            n0 = self._dof * self.grid.part.plane * (self.grid.part.node_z0 + self.grid.part.own_lo)
            for c, sol in enumerate(sols[:self.physics.ncases]):
                U = self.physics.LoadCaseU(c)
                U.zero_()
                U[sl] = torch.from_numpy(sol[n0:n0 + (sl.stop - sl.start)].copy()).to(self.x.device)

    def WriteVTK(self, itr):
        if self._out is None:
            return
        if self.physics_kind == "heat":   # the point field keeps its three components: the temperature in the first
            U = self.grid.node_vec(3)
            U[0::3] = self.physics.T
            self._out.WriteVTK(U, self.x, self.xTilde, self.xPrint, itr)
        else:
            self._out.WriteVTK(self.physics.U, self.x, self.xTilde, self.xPrint, itr)

    def _increase_beta(self, gx, ch):
        """Filter::IncreaseBeta, Filter.cc:268-288"""
        if (ch < 0.01 or self.itr % 10 == 0) and self.beta < self.betaFinal and gx < 0.000001:
            self.beta = self.beta + 1 if self.beta < 7 else self.beta * 1.2
            self.beta = min(self.beta, self.betaFinal)

    def run(self, max_itr=None, verbose=False):
        ch = 1.0
        n = self.maxItr if max_itr is None else max_itr
        while self.itr < n and ch > 0.01:                                                        # main.cc:54
            beta0 = self.beta
            ch = self.step(verbose)["ch"]
            if self.itr < 11 or self.itr % 20 == 0 or self.beta != beta0:                        # :114-116
                self.WriteVTK(self.itr)
            if self.itr % 10 == 0:                                                               # :119-122
                self.WriteRestartFiles()
        self.WriteRestartFiles()                                                                 # :125-126
        self.WriteVTK(self.itr + 1)                                                              # :129
        return self.history
