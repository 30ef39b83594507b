"""Host-side mirror of the reference's operator interface for the hot path.

Class and method names follow the reference (LinearElasticity.h:21-109,
Filter.h:34-92) so that tests read like the reference's call sites in main.cc;
vectors are 1-D float64 torch tensors on the GPU standing in for PETSc Vecs
(local slab layout, see include/topopt_amd.h).  Everything numerical happens in
libtopopt_amd.so.
"""
import ctypes as C
import os
from dataclasses import dataclass

import torch

from . import lib as _lib
from .comm import SlabComm
from .partition import SlabPartition


class TopOptError(RuntimeError):
    def __init__(self, code, where, message=None):
        """message: the whole text where the code's name alone would not say enough (Eigenmodes: the residuals)"""
        names = {1: "TP_ERR_ARG", 2: "TP_ERR_STATE", 3: "TP_ERR_DIVERGED", 4: "TP_ERR_COMM"}
        msg = names.get(code, "hipError %d" % (code - 1000) if code >= 1000 else str(code))
        super().__init__(message if message is not None else "%s failed: %s" % (where, msg))
        self.code = code


def _chk(code, where):
    if code != 0:
        raise TopOptError(code, where)


def device_bytes_live():
    """bytes of device memory the library's own objects hold in this process (torch's tensors and tp_malloc are not counted)"""
    return int(_lib.load_library().tp_device_bytes_live())


def check_body_force(b, x_low):
    """-> ((b_x, b_y, b_z), x_low) as floats; ValueError unless b is three finite numbers and 0 <= x_low < 1"""
    import math
    try:
        b = tuple(float(v) for v in b)
        x_low = float(x_low)
    except (TypeError, ValueError):
        raise ValueError("body force: need three numbers and a number x_low, got %r, %r" % (b, x_low))
    if len(b) != 3 or not all(math.isfinite(v) for v in b):
        raise ValueError("body force: need three finite numbers (b_x, b_y, b_z), got %r" % (b,))
    if not 0.0 <= x_low < 1.0:
        raise ValueError("body force: x_low must lie in [0, 1), got %r" % (x_low,))
    return b, x_low


def check_thermal(alpha, T_ref, penal_beta, Emin, Emax):
    """-> (alpha, T_ref, Emin, Emax, penal_beta) as floats, the order of tp_thermal_par; ValueError unless alpha and T_ref are
    finite, penal_beta >= 1 and 0 <= Emin < Emax"""
    import math
    try:
        alpha, T_ref, penal_beta, Emin, Emax = (float(v) for v in (alpha, T_ref, penal_beta, Emin, Emax))
    except (TypeError, ValueError):
        raise ValueError("thermal expansion: need numbers, got %r" % ((alpha, T_ref, penal_beta, Emin, Emax),))
    if not (math.isfinite(alpha) and math.isfinite(T_ref)):
        raise ValueError("thermal expansion: alpha and T_ref must be finite, got %r, %r" % (alpha, T_ref))
    if not (math.isfinite(penal_beta) and penal_beta >= 1.0):
        raise ValueError("thermal expansion: the exponent must be at least 1, got %r" % (penal_beta,))
    if not (math.isfinite(Emin) and math.isfinite(Emax) and 0.0 <= Emin < Emax):
        raise ValueError("thermal expansion: need 0 <= Emin < Emax, both finite; got %r, %r" % (Emin, Emax))
    return alpha, T_ref, Emin, Emax, penal_beta


def _ptr(t):
    if t is None:
        return None
    assert t.dtype == torch.float64 and t.is_contiguous() and t.is_cuda, "need a contiguous float64 GPU tensor"
    return t.data_ptr()


class _Handle:
    """A library object behind `handle`, made on a grid that adopted it (Grid._adopt): close() destroys it NOW -- Grid.close()
    does that for every dependent before the grid goes -- and is idempotent; __del__ at the latest.  _destroy: the name of the
    library's destroy call."""
    _destroy = None

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.L, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Levels:
    """The multigrid hierarchy of a handle level by level, for tests, tools and bench.py: the <_prefix>_level_* / _smooth /
    _restrict / _prolong_add / _last_op_form calls of include/topopt_amd.h (one contract for the three families; csrc/mg_levels.h).
    Vectors hold _dof values per local node of the level.  Every error answer raises TopOptError: a non-zero code, the negative
    code of level_count / level_nodes, the NaN of the lambdas."""
    _prefix, _dof = None, 1

    def _level_fn(self, suffix):
        name = "%s_%s" % (self._prefix, suffix)
        return getattr(self.L, name), name

    def _level_call(self, suffix, *args):
        fn, name = self._level_fn(suffix)
        _chk(fn(self.handle, *args), name)

    def _level_value(self, suffix, *args):
        """the four calls that answer a value: a count (-code: an error) or a lambda (NaN: TP_ERR_ARG)"""
        fn, name = self._level_fn(suffix)
        v = fn(self.handle, *args)
        _chk((1 if v != v else 0) if isinstance(v, float) else max(-v, 0), name)
        return v

    def level_count(self):
        return self._level_value("level_count")

    def level_nodes(self, l):
        return self._level_value("level_nodes", l)

    def level_lambda(self, l):
        return self._level_value("level_lambda", l)

    def level_lambda_min(self, l):
        return self._level_value("level_lambda_min", l)

    def level_vec(self, l):
        return torch.zeros(self._dof * self.level_nodes(l), dtype=torch.float64, device=self.grid.device)

    def level_apply(self, l, u):
        y = torch.zeros_like(u)
        self._level_call("level_apply", l, _ptr(u), _ptr(y))
        return y

    def level_dinv(self, l):
        d = self.level_vec(l)
        self._level_call("level_diag", l, _ptr(d))
        return d

    def smooth(self, l, b, x, k, zero_guess=False):
        self._level_call("smooth", l, _ptr(b), _ptr(x), k, int(zero_guess))
        return x

    def restrict(self, l, rf):
        rc = self.level_vec(l + 1)
        self._level_call("restrict", l, _ptr(rf), _ptr(rc))
        return rc

    def prolong_add(self, l, xc, xf):
        self._level_call("prolong_add", l, _ptr(xc), _ptr(xf))
        return xf

    def last_op_form(self):
        """(kind, a, b, c) of the last operator application (tp_elasticity_last_op_form): kind 1 fine tile kernel (generation,
        tile 0 15x15 / 1 16x16 / 2 32x8, z-chunk), 2 level 1 from the fine densities (correction fused, -, z-chunk), 3 per-node
        matrix-free, 4 stored stencil (threads per row, node form, mirrored reads).  Kind 3 on the scalar hierarchies: a = 2 the
        register form of conduction.h, a = 1 the PDE filter's 27-point weight table, a = 0 the gather over the elements
        (TP_NO_COND_STENCIL, TP_NO_PDE_STENCIL)"""
        f = (C.c_int * 4)()
        self._level_call("last_op_form", f)
        return tuple(f)


class _LevelStats(_Levels):
    """... and the two calls that the elasticity and the conduction family have beside them"""

    def level_residual(self, l, b, x):
        """r = b - A_l x through the residual epilogue of the level's kernel, as the V-cycle forms it"""
        r = torch.zeros_like(x)
        self._level_call("level_residual", l, _ptr(b), _ptr(x), _ptr(r))
        return r

    def pop_stats(self):
        b, f, n = C.c_double(), C.c_double(), C.c_long()
        self._level_call("last_stats", C.byref(b), C.byref(f), C.byref(n))
        return b.value, f.value, n.value


@dataclass
class SolverOptions:
    """LinearElasticity.cc:621-635 defaults; smoother = Chebyshev(nsmooth)/Jacobi."""
    nlvls: int = 4
    nu: float = 0.3
    rtol: float = 1.0e-5
    atol: float = 1.0e-50
    dtol: float = 1.0e5
    max_it: int = 200
    nsmooth: int = 4
    ncoarse: int = 30
    cheb_lo: float = 0.1
    cheb_hi: float = 1.1
    nlanczos: int = 10
    fine_eig: int = 0   # 0: element bound on the fine level, 1: Lanczos estimate
    # ksp_mode 1: the configuration the reference hard-codes (FGMRES(restart) + V-cycle with GMRES(nsmooth) smoothers and
    # a GMRES(coarse_restart) coarse solve, PCSOR / PCJACOBI; LinearElasticity.cc:620-746, PDEFilter.cc:276-378) run as
    # written -- a correctness mode on one device; 0: CG + Chebyshev/Jacobi, the fast path
    ksp_mode: int = 0
    restart: int = 100
    smooth_pc: int = 1      # 0 PCJACOBI, 1 PCSOR
    coarse_pc: int = 1
    coarse_restart: int = 30
    coarse_rtol: float = 1.0e-8
    # ksp_mode 0: coarsest level solved exactly (banded Cholesky + explicit triangular inverse, csrc/coarse_direct.h) where it
    # has 449 .. 4096 rows on one rank (2: also below 449, where the Chebyshev run stays inside one workgroup); 0: Chebyshev run
    coarse_direct: int = 0

    @classmethod
    def reference_elasticity(cls, **kw):
        """LinearElasticity::SetUpSolver as hard-coded (LinearElasticity.cc:620-746)"""
        return cls(**{**dict(ksp_mode=1, restart=100, nsmooth=4, ncoarse=30, smooth_pc=1, coarse_pc=1, coarse_restart=30,
                             coarse_rtol=1e-8, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=200), **kw})

    @classmethod
    def reference_pdefilter(cls, **kw):
        """PDEFilt::SetUpSolver as hard-coded (PDEFilter.cc:276-378)"""
        return cls(**{**dict(ksp_mode=1, nlvls=3, restart=20, nsmooth=1, ncoarse=10, smooth_pc=0, coarse_pc=0, coarse_restart=10,
                             coarse_rtol=1e-8, rtol=1e-8, atol=1e-50, dtol=1e3, max_it=60), **kw})

    def c_struct(self):
        return _lib.SolverOpts(self.nlvls, self.nu, self.rtol, self.atol, self.dtol, self.max_it, self.nsmooth,
                               self.ncoarse, self.cheb_lo, self.cheb_hi, self.nlanczos, self.fine_eig, self.ksp_mode,
                               self.restart, self.smooth_pc, self.coarse_pc, self.coarse_restart, self.coarse_rtol,
                               self.coarse_direct)


class Grid:
    """The DMDA stand-in: global node counts, element size, z-slab partition."""

    def __init__(self, nx, ny, nz, h, rank=0, nranks=1, device=None, group=None):
        self.L = _lib.load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the MI355X hot path has no CPU fallback")
        self.part = SlabPartition(nx, ny, nz, rank, nranks)
        self.h = (h, h, h) if isinstance(h, (int, float)) else tuple(h)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.stream = torch.cuda.current_stream(self.device)
        self.comm = None
        comm_p = None
        if nranks > 1:
            self.comm = SlabComm(self.part, self.device, group)
            self.comm.stream = self.stream   # the hooks issue their collectives on the library's stream
            comm_p = C.cast(C.pointer(self.comm.c_struct), C.c_void_p)
        self._opts = _lib.GridOpts(nx, ny, nz, self.h[0], self.h[1], self.h[2], rank, nranks, self.device.index,
                                   self.stream.cuda_stream, comm_p)
        self.handle = C.c_void_p()
        self._children = []   # weak references to the solvers / filters / optimisers built on this grid (close() order)
        _chk(self.L.tp_grid_create(C.byref(self.handle), C.byref(self._opts)), "tp_grid_create")
        self.comm_kind = "none" if nranks == 1 else "torch.distributed hooks"
        if nranks > 1 and self.comm.backend == "nccl" and os.environ.get("TP_COMM", "rccl") != "torch":
            self._use_rccl(group)

    @property
    def halo_overlap(self):
        """number of halos that travelled on the second stream, overlapped with interior planes (0 = none)"""
        return int(self.L.tp_grid_overlapped_halos(self.handle))

    def comm_stats(self):
        """(halo exchanges, all-reduces) the in-library RCCL path has issued so far; (0, 0) on the hooks / one rank"""
        ex, red = C.c_long(0), C.c_long(0)
        self.L.tp_grid_comm_stats(self.handle, C.byref(ex), C.byref(red))
        return ex.value, red.value

    def comm_report(self):
        """what the slab exchange runs on, for the bench line: path, the ranks the RCCL communicator itself reports, whether
        the in-library path passed its collective self-check (or why the grid went back to the host-staged hooks)"""
        n, two = C.c_int(0), C.c_int(0)
        self.L.tp_grid_comm_info(self.handle, C.byref(n), C.byref(two))
        return {"path": self.comm_kind, "ranks": self.part.nranks, "rccl_ranks_seen": n.value, "two_communicators": bool(two.value),
                "selfcheck": getattr(self, "_rccl_selfcheck", "not run (no in-library RCCL path requested)" if self.part.nranks > 1 else "one rank")}

    def reduction_selftest(self, n, reps):
        """`reps` back-to-back dot products over n doubles, in-kernel reduction tail against the two-launch form: mismatches"""
        bad = C.c_int(0)
        _chk(self.L.tp_grid_reduction_selftest(self.handle, int(n), int(reps), C.byref(bad)), "tp_grid_reduction_selftest")
        return bad.value

    def comm_timer(self, on):
        """N > 1: start / stop collecting the communication timing (tp_grid_comm_timer)"""
        _chk(self.L.tp_grid_comm_timer(self.handle, int(on)), "tp_grid_comm_timer")

    def comm_timer_read(self):
        """-> {kind: {"calls", "host_ms", "device_ms"}} for the kinds halo_blocking, halo_overlapped, all_reduce, all_gather"""
        n, h, d = (C.c_long * 4)(), (C.c_double * 4)(), (C.c_double * 4)()
        _chk(self.L.tp_grid_comm_timer_read(self.handle, n, h, d), "tp_grid_comm_timer_read")
        kinds = ("halo_blocking", "halo_overlapped", "all_reduce", "all_gather")
        return {k: {"calls": int(n[i]), "host_ms": float(h[i]), "device_ms": float(d[i])} for i, k in enumerate(kinds)}

    def kernel_timer(self, on):
        """bracket every launch of the fine level's fused Chebyshev step with a HIP event pair (bench.py's roofline)"""
        _chk(self.L.tp_grid_kernel_timer(self.handle, int(on)), "tp_grid_kernel_timer")

    def kernel_timer_read(self):
        """-> (average ms per launch, launches) since the timer was switched on / last read"""
        t, n = C.c_double(0.0), C.c_long(0)
        _chk(self.L.tp_grid_kernel_timer_read(self.handle, C.byref(t), C.byref(n)), "tp_grid_kernel_timer_read")
        return (t.value / n.value if n.value else 0.0), n.value

    def kernel_timer_read2(self):
        """-> (total ms, launches, algorithmic bytes of exactly those launches)"""
        t, n, b = C.c_double(0.0), C.c_long(0), C.c_double(0.0)
        _chk(self.L.tp_grid_kernel_timer_read2(self.handle, C.byref(t), C.byref(n), C.byref(b)), "tp_grid_kernel_timer_read2")
        return t.value, n.value, b.value

    def _use_rccl(self, group):
        """Hand the slab exchange to RCCL inside the library (tp_grid_use_rccl): same RCCL instance as
        torch.distributed's nccl backend, no Python round trip per halo.  Every rank takes the same decision."""
        import torch.distributed as dist
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        ok = os.path.exists(path) and self.L.tp_rccl_load(path.encode()) == 0
        idbuf, idbuf2 = C.create_string_buffer(128), C.create_string_buffer(128)
        if ok and self.part.rank == 0:   # two ids: collectives and neighbour exchanges on communicators of their own
            ok = self.L.tp_rccl_unique_id(idbuf) == 0 and self.L.tp_rccl_unique_id(idbuf2) == 0
        flag = torch.tensor([1 if ok else 0], device=self.device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag[0]) == 0:
            self._rccl_selfcheck = "not run: librccl.so could not be loaded on some rank -> torch.distributed hooks"
            return
        obj = [idbuf.raw + idbuf2.raw if self.part.rank == 0 else None]
        src = 0 if group is None else dist.get_global_rank(group, 0)
        dist.broadcast_object_list(obj, src=src, group=group)
        idb, idb2 = C.create_string_buffer(obj[0][:128], 128), C.create_string_buffer(obj[0][128:], 128)
        # one communicator by default: halo exchanges and all-reduces share it (stream order decides).  A second
        # communicator for the exchanges (TP_RCCL_TWO_COMM=1) lets them run beside the reductions, but two communicators
        # are only guaranteed to make progress concurrently if their kernels can co-reside -- opt-in until a run on two or
        # more GPUs has passed the self-check and a full solve with it
        if os.environ.get("TP_RCCL_TWO_COMM"):
            rc = self.L.tp_grid_use_rccl2(self.handle, idb, idb2)
        else:
            rc = self.L.tp_grid_use_rccl(self.handle, idb)
        flag = torch.tensor([1 if rc == 0 else 0], device=self.device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag[0]) == 0:   # some rank could not create its communicator: every rank goes back to the hooks
            self.L.tp_grid_drop_rccl(self.handle)
            print("topopt_amd: tp_grid_use_rccl failed on a rank; using the torch.distributed hooks", flush=True)
            self._rccl_selfcheck = "not run: ncclCommInitRank failed on some rank -> torch.distributed hooks"
            return
        # trust, but verify: rank-tagged planes through the new path; any rank unhappy -> everybody back to the hooks
        ok = C.c_int(0)
        rc = self.L.tp_grid_comm_selfcheck(self.handle, C.byref(ok))
        flag = torch.tensor([1 if (rc == 0 and ok.value == 1) else 0], device=self.device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag[0]) == 0:
            self.L.tp_grid_drop_rccl(self.handle)
            print("topopt_amd: in-library RCCL exchange failed its self-check; using the torch.distributed hooks", flush=True)
            self._rccl_selfcheck = "fail -> fallback to the torch.distributed hooks"
            return
        self._rccl_selfcheck = "pass"
        self.comm_kind = "rccl (in-library)"

    def _adopt(self, child):
        import weakref
        self._children.append(weakref.ref(child))

    def close(self):
        """Destroy the library objects NOW, dependents first (solvers, filters, optimisers built on this grid), after a
        device synchronisation -- the explicit, ordered counterpart of XxxDestroy in the reference (main.cc:126-134).
        Multi-rank programs call this on every rank before the process group goes (bench.py); idempotent."""
        for ref in list(getattr(self, "_children", ())):
            obj = ref()
            if obj is not None:
                obj.close()
        self._children = []
        if getattr(self, "handle", None):
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            self.L.tp_grid_destroy(self.handle)
            self.handle = None
        self.comm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # sizes of the local arrays
    @property
    def n_local_nodes(self):
        return self.L.tp_grid_local_nodes(self.handle)

    @property
    def n_own_elems(self):
        return self.L.tp_grid_local_elems(self.handle)

    def node_vec(self, dof=3):
        return torch.zeros(self.n_local_nodes * dof, dtype=torch.float64, device=self.device)

    def elem_vec(self, value=0.0):
        return torch.full((self.n_own_elems,), value, dtype=torch.float64, device=self.device)

    def synth_density(self, seed=12345):
        x = self.elem_vec()
        _chk(self.L.tp_synth_density(self.handle, _ptr(x), seed), "tp_synth_density")
        return x

    # ---- blocks of up to TP_MAX_CASES vectors (the Rayleigh-Ritz step of LinearElasticity.Eigenmodes) ----
    def BlockGram(self, X, Y):
        """all len(X)^2 dot products X_i . Y_j over the tensors as they are passed (owned slices: the sum over the ranks is what
        VecDot gives) in one pass -> numpy array [q, q]"""
        import numpy as np
        q = len(X)
        if len(Y) != q:
            raise ValueError("BlockGram: %d and %d vectors" % (q, len(Y)))
        n = X[0].numel() if q else 0
        assert all(v.numel() == n for v in list(X) + list(Y)), "BlockGram: vectors of different lengths"
        Xa = (C.c_void_p * max(q, 1))(*[_ptr(v) for v in X])
        Ya = (C.c_void_p * max(q, 1))(*[_ptr(v) for v in Y])
        out = (C.c_double * max(q * q, 1))()
        _chk(self.L.tp_vec_block_gram(self.handle, q, Xa, Ya, n, out), "tp_vec_block_gram")
        return np.array(out[:q * q]).reshape(q, q)

    def BlockCombine(self, Y, Q, Z):
        """Z_i = sum_j Q[j, i] Y_j for the q vectors of Y in one pass; no Z_i may overlap a Y_j"""
        import numpy as np
        q = len(Y)
        Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
        if len(Z) != q or Q.shape != (q, q):
            raise ValueError("BlockCombine: %d inputs, %d outputs, coefficients of shape %r" % (q, len(Z), Q.shape))
        n = Y[0].numel() if q else 0
        assert all(v.numel() == n for v in list(Y) + list(Z)), "BlockCombine: vectors of different lengths"
        Ya = (C.c_void_p * max(q, 1))(*[_ptr(v) for v in Y])
        Za = (C.c_void_p * max(q, 1))(*[_ptr(v) for v in Z])
        _chk(self.L.tp_vec_block_combine(self.handle, q, Ya, Q.ctypes.data_as(C.POINTER(C.c_double)), Za, n), "tp_vec_block_combine")
        return Z

    def sync(self):
        _chk(self.L.tp_sync(self.handle), "tp_sync")


class LinearElasticity(_Handle, _LevelStats):
    """LinearElasticity (LinearElasticity.h:21-109) on the MI355X."""
    _destroy, _prefix, _dof = "tp_elasticity_destroy", "tp_elasticity", 3

    def __init__(self, grid, opts=None):
        self.grid, self.L = grid, grid.L
        self.opts = opts or SolverOptions()
        self.handle = C.c_void_p()
        self._o = self.opts.c_struct()
        _chk(self.L.tp_elasticity_create(C.byref(self.handle), grid.handle, C.byref(self._o)), "tp_elasticity_create")
        grid._adopt(self)
        self.U = grid.node_vec(3)       # state, persists across design iterations (warm start, :647)
        self.RHS = grid.node_vec(3)
        self.N = grid.node_vec(3)
        self.last_its, self.last_rnorm, self.last_bnorm, self.last_hist = 0, 0.0, 0.0, None
        # load cases: case 0 is RHS / U above; AddLoadCase appends (RHS_l, U_l) -- every case keeps its own state, so
        # each warm-starts from its own previous solution.  The supports N are shared.
        self._case_rhs, self._case_U, self.case_weight = [self.RHS], [self.U], [1.0]
        self.case_its, self.case_rnorm, self.case_bnorm = [0], [0.0], [0.0]
        self.last_f_case = None
        # stress constraint: the adjoint state persists like the states (warm start); allocated by the first StressSensitivity
        self.lam = self._stress_dpdx = self._stress_rhs = None
        self.adjoint_its, self.adjoint_rnorm, self.adjoint_bnorm = 0, 0.0, 0.0
        # self-weight (SetBodyForce): None = off; the total loads F_l + f(xPhys) live in buffers of their own, made on first use
        self.body_force, self.body_xlow, self._case_total = None, 0.1, []
        # thermal expansion (SetThermalExpansion): None = off; the temperature field is the caller's (SetTemperature)
        self.thermal, self._temperature = None, None
        # eigenmodes: the block of Ritz vectors persists like the states (warm start across design iterations); made by the
        # first Eigenmodes call
        self._eig = None
        # buckling modes: the same for BucklingModes; the adjoint state of BucklingSensitivity persists too
        self._buck = self._buck_adj = self._buck_rhs = self._buck_row = None

    @property
    def KE(self):
        import numpy as np
        ke = np.zeros(576)
        _chk(self.L.tp_elasticity_get_ke(self.handle, ke.ctypes.data), "tp_elasticity_get_ke")
        return ke

    def KE_effective(self):
        """the element matrix the fine-level kernels apply inside the preconditioner (smoother, V-cycle residual), as a
        numpy.longdouble array of 576 (hi + lo of the library's double-double pair): KE in its packed block form (36 values),
        < 1 ulp of max|KE| away from KE"""
        import numpy as np
        hi, lo = np.zeros(576), np.zeros(576)
        _chk(self.L.tp_elasticity_get_ke_effective(self.handle, hi.ctypes.data, lo.ctypes.data), "tp_elasticity_get_ke_effective")
        return hi.astype(np.longdouble) + lo.astype(np.longdouble)

    def KE_krylov(self):
        """the element matrix of the Krylov operator (the Krylov method's own products: A p and the initial residual of CG; A Z_j
        and the initial / restart residual of the outer FGMRES in ksp_mode 1; MatMultKrylov -- MatMult applies the packed form,
        KE_effective()): the packed form plus the translation mode's column and row of T KE T / 64 as KE has them;
        numpy.longdouble array of 576"""
        import numpy as np
        hi, lo = np.zeros(576), np.zeros(576)
        _chk(self.L.tp_elasticity_get_ke_krylov(self.handle, hi.ctypes.data, lo.ctypes.data), "tp_elasticity_get_ke_krylov")
        return hi.astype(np.longdouble) + lo.astype(np.longdouble)

    def SetUpLoadAndBC(self):
        """cantilever load case, LinearElasticity.cc:143-171"""
        _chk(self.L.tp_elasticity_cantilever(self.handle, _ptr(self.N), _ptr(self.RHS)), "tp_elasticity_cantilever")

    def SetUpLoadAndBC_MBB(self, load=-0.001):
        """Half MBB beam (BASELINE config 4; SURVEY D5: the reference ships only the cantilever, so this load case is
        data defined by the build): symmetry plane x = xmin (u_x = 0), roller along the edge x = xmax, z = zmin
        (u_z = 0, one node also u_y = 0), line load in -z along the edge x = xmin, z = zmax with half loads at the
        two end nodes.  Single rank or z-slabs (global z index decides)."""
        p = self.grid.part
        nx, ny, nzl = p.nx, p.ny, p.nz_local
        N = torch.ones(nzl, ny, nx, 3, dtype=torch.float64)
        R = torch.zeros(nzl, ny, nx, 3, dtype=torch.float64)
        kz = torch.arange(nzl) + p.node_z0
        N[:, :, 0, 0] = 0.0
        bot, top = kz == 0, kz == p.nz - 1
        N[bot, :, nx - 1, 2] = 0.0
        if bool(bot.any()):
            N[int(torch.nonzero(bot)[0]), 0, nx - 1, 1] = 0.0
        R[top, :, 0, 2] = load
        R[top, 0, 0, 2] = 0.5 * load
        R[top, ny - 1, 0, 2] = 0.5 * load
        self.SetBC(N.reshape(-1).to(self.U.device), R.reshape(-1).to(self.U.device))

    def SetUpLoadAndBC_Top(self, weight=1.0):
        """A second built-in right-hand side for the cantilever, added as a new load case (the supports N stay as they
        are): line load +0.001 in z along the edge x = xmax, z = zmax, half loads at the two end nodes.  Single rank or
        z-slabs (global z index decides).  Returns the index of the case."""
        p = self.grid.part
        nx, ny, nzl = p.nx, p.ny, p.nz_local
        R = torch.zeros(nzl, ny, nx, 3, dtype=torch.float64)
        top = (torch.arange(nzl) + p.node_z0) == p.nz - 1
        R[top, :, nx - 1, 2] = 0.001
        R[top, 0, nx - 1, 2] = 0.0005
        R[top, ny - 1, nx - 1, 2] = 0.0005
        return self.AddLoadCase(R.reshape(-1).to(self.U.device), weight)

    # ---- several load cases on the shared supports N ----
    @property
    def ncases(self):
        return len(self._case_rhs)

    def AddLoadCase(self, RHS, weight=1.0):
        """a further right-hand side (local node layout of self.RHS) with a persistent state of its own, zero at first;
        returns its index.  At most TP_MAX_CASES cases, case 0 (self.RHS / self.U) included."""
        if self.ncases >= _lib.MAX_CASES:
            raise TopOptError(1, "AddLoadCase (more than TP_MAX_CASES = %d load cases)" % _lib.MAX_CASES)
        rhs = self.grid.node_vec(3)
        rhs.copy_(RHS)
        self._case_rhs.append(rhs)
        self._case_U.append(self.grid.node_vec(3))
        self.case_weight.append(float(weight))
        for lst, zero in ((self.case_its, 0), (self.case_rnorm, 0.0), (self.case_bnorm, 0.0)):
            lst.append(zero)
        return self.ncases - 1

    def SetLoadCaseWeight(self, case, weight):
        self.case_weight[case] = float(weight)

    def LoadCaseRHS(self, case):
        return self._case_rhs[case]

    def LoadCaseU(self, case):
        return self._case_U[case]

    def SetBC(self, N, RHS):
        self.N.copy_(N)
        self.RHS.copy_(RHS)
        _chk(self.L.tp_elasticity_set_bc(self.handle, _ptr(self.N)), "tp_elasticity_set_bc")

    def SetTolerances(self, rtol=-1.0, atol=-1.0, dtol=-1.0, max_it=-1):
        """KSPSetTolerances; a negative value keeps the current one.  Keeps self.opts in step with the handle (Eigenmodes restores
        the solver's rtol from there)"""
        _chk(self.L.tp_elasticity_set_tolerances(self.handle, float(rtol), float(atol), float(dtol), int(max_it)), "tp_elasticity_set_tolerances")
        for name, v in (("rtol", rtol), ("atol", atol), ("dtol", dtol), ("max_it", max_it)):
            if v >= 0:
                setattr(self.opts, name, type(getattr(self.opts, name))(v))

    def AssembleStiffnessMatrix(self, xPhys, Emin, Emax, penal):
        _chk(self.L.tp_elasticity_assemble(self.handle, _ptr(xPhys), Emin, Emax, penal), "tp_elasticity_assemble")

    def MatMult(self, u, y=None):
        y = torch.zeros_like(u) if y is None else y
        _chk(self.L.tp_elasticity_apply(self.handle, _ptr(u), _ptr(y)), "tp_elasticity_apply")
        return y

    def MatMultKrylov(self, u, y=None):
        """the product the Krylov method multiplies with inside KSPSolve, CG's and ksp_mode 1's outer FGMRES's (the operator from KE_krylov(): KE's action to rounding on
        translation-dominated fields); MatMult applies the packed form (KE_effective())"""
        y = torch.zeros_like(u) if y is None else y
        _chk(self.L.tp_elasticity_apply_krylov(self.handle, _ptr(u), _ptr(y)), "tp_elasticity_apply_krylov")
        return y

    def MatMultKrylovDot(self, u, y=None):
        """MatMultKrylov that also returns the value of the product's fused dot product: (y, u . y) -- CG's p . A p"""
        y = torch.zeros_like(u) if y is None else y
        d = C.c_double()
        _chk(self.L.tp_elasticity_apply_krylov_dot(self.handle, _ptr(u), _ptr(y), C.byref(d)), "tp_elasticity_apply_krylov_dot")
        return y, d.value

    # ---- self-weight: a body force that moves with the material ----
    def SetBodyForce(self, b, x_low=0.1):
        """b = (b_x, b_y, b_z), the body force per unit volume at full density (rho g); below x_low the mass is damped as
        m(x) = x t^5 (6 - 5 t), t = x / x_low (include/topopt_amd.h).  From now on SolveState solves on F_l + f(xPhys) and the
        sensitivities carry the load's term.  None switches it off again."""
        if b is None:
            self.body_force, self._case_total = None, []
            return
        self.body_force, self.body_xlow = check_body_force(b, x_low)

    def _body3(self):
        if self.body_force is None:
            raise TopOptError(2, "self-weight (no body force set: SetBodyForce)")
        return (C.c_double * 3)(*self.body_force)

    def BodyLoad(self, xPhys, out, base=None):
        """out = base + f(xPhys) on the owned node planes (base None: f alone; out may be base); ghost planes stay"""
        _chk(self.L.tp_elasticity_body_load(self.handle, _ptr(xPhys), self._body3(), self.body_xlow, _ptr(base), _ptr(out)),
             "tp_elasticity_body_load")
        return out

    def BodySensitivity(self, V_list, w, xPhys, scale, dfdx):
        """dfdx += scale * sum_l w_l d(v_l^T N f)/dxPhys (w None: all weights 1); nothing is reduced, the host does not wait"""
        n = len(V_list)
        Va = (C.c_void_p * max(n, 1))(*[_ptr(v) for v in V_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        _chk(self.L.tp_elasticity_body_sensitivity(self.handle, n, Va, wa, _ptr(xPhys), self._body3(), self.body_xlow, float(scale),
                                                   _ptr(dfdx)), "tp_elasticity_body_sensitivity")

    def TotalRHS(self, case):
        """F_case + f(xPhys) of the last SolveState with a body force set (LoadCaseRHS keeps returning the fixed load)"""
        return self._case_total[case]

    def _form_totals(self, xPhys):
        while len(self._case_total) < self.ncases:
            self._case_total.append(self.grid.node_vec(3))
        for rhs, total in zip(self._case_rhs, self._case_total):
            total.copy_(rhs)   # (the ghost planes too)
            if self.body_force is not None:
                self.BodyLoad(xPhys, total, base=total)
            if self.thermal is not None:
                self.ThermalLoad(xPhys, self._temperature_set(), total, base=total)

    # ---- thermal expansion: a temperature field that loads the structure ----
    def SetThermalExpansion(self, alpha, T_ref=0.0, penal_beta=None, Emin=1.0e-9, Emax=1.0):
        """beta(x) = alpha (Emin + x^penal_beta (Emax - Emin)), the thermal stress coefficient per unit of T - T_ref
        (include/topopt_amd.h; penal_beta None: 3).  From now on SolveState solves on F_l + f_th(xPhys, T) with T the field of
        SetTemperature, and the sensitivities carry the load's term at fixed T.  alpha None switches it off again."""
        if alpha is None:
            self.thermal = None
            if self.body_force is None:
                self._case_total = []
            return
        self.thermal = check_thermal(alpha, T_ref, 3.0 if penal_beta is None else penal_beta, Emin, Emax)

    def SetTemperature(self, T):
        """the nodal temperature field (local node layout, one value per node) the thermal load is formed from; kept by
        reference: the caller's solver writes it, SolveState reads it"""
        self._temperature = T

    def _temperature_set(self):
        if self._temperature is None:
            raise TopOptError(2, "thermal expansion (no temperature field: SetTemperature)")
        return self._temperature

    def _thermal_par(self):
        if self.thermal is None:
            raise TopOptError(2, "thermal expansion (not set: SetThermalExpansion)")
        return C.byref(_lib.ThermalPar(*self.thermal))

    def ThermalLoad(self, xPhys, T, out, base=None):
        """out = base + f_th(xPhys, T) on the owned node planes (base None: f_th alone; out may be base); ghost planes stay"""
        _chk(self.L.tp_elasticity_thermal_load(self.handle, _ptr(xPhys), _ptr(T), self._thermal_par(), _ptr(base), _ptr(out)),
             "tp_elasticity_thermal_load")
        return out

    def ThermalSensitivity(self, V_list, w, xPhys, T, scale, dfdx):
        """dfdx += scale * sum_l w_l d(v_l^T N f_th)/dxPhys at fixed T (w None: all weights 1); nothing is reduced"""
        n = len(V_list)
        Va = (C.c_void_p * max(n, 1))(*[_ptr(v) for v in V_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        _chk(self.L.tp_elasticity_thermal_sensitivity(self.handle, n, Va, wa, _ptr(xPhys), _ptr(T), self._thermal_par(), float(scale),
                                                      _ptr(dfdx)), "tp_elasticity_thermal_sensitivity")

    def ThermalAdjointRHS(self, V_list, w, xPhys, scale, out):
        """out = scale * sum_l w_l (d f_th / dT)^T N v_l on the owned node planes, one value per node: the right-hand side of the
        thermal adjoint; ghost planes stay"""
        n = len(V_list)
        Va = (C.c_void_p * max(n, 1))(*[_ptr(v) for v in V_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        _chk(self.L.tp_elasticity_thermal_adjoint_rhs(self.handle, n, Va, wa, _ptr(xPhys), self._thermal_par(), float(scale), _ptr(out)),
             "tp_elasticity_thermal_adjoint_rhs")
        return out

    def ThermalCoefficients(self, xPhys, beta=None, dbeta=None):
        """-> (beta, beta') per own element as the thermal passes form them (parity tests); with one of the two outputs given the
        other is not formed and comes back as None"""
        if beta is None and dbeta is None:
            beta, dbeta = self.grid.elem_vec(), self.grid.elem_vec()
        _chk(self.L.tp_elasticity_thermal_coefficients(self.handle, _ptr(xPhys), self._thermal_par(), _ptr(beta), _ptr(dbeta)),
             "tp_elasticity_thermal_coefficients")
        return beta, dbeta

    def ThermalCoupling(self):
        """the coupling matrix G of the element (24 x 8 row-major, numpy array of 192): f_e = beta G (T_e - T_ref)"""
        import numpy as np
        g = np.zeros(192)
        _chk(self.L.tp_elasticity_get_thermal_coupling(self.handle, g.ctypes.data), "tp_elasticity_get_thermal_coupling")
        return g

    # ---- free vibration: A phi = lambda B phi, A = N K N + (I - N) of the last assembly, B = N M N ----
    def MassAssemble(self, xPhys, rho0=1.0, x_low=0.1):
        """rho0 V_e m(xPhys) for MassMult / MassSensitivity, once per design (m: the damped interpolation of SetBodyForce)"""
        _chk(self.L.tp_elasticity_mass_assemble(self.handle, _ptr(xPhys), float(rho0), float(x_low)), "tp_elasticity_mass_assemble")

    def MassMult(self, u, y=None):
        """y = N M N u on the owned node planes (ghost planes of y stay as they are)"""
        y = torch.zeros_like(u) if y is None else y
        _chk(self.L.tp_elasticity_mass_apply(self.handle, _ptr(u), _ptr(y)), "tp_elasticity_mass_apply")
        return y

    def MassSensitivity(self, V_list, w, xPhys, scale, out):
        """out += scale m'(x) rho0 V_e sum_l w_l (N v_l)^T (M8 (x) I3) (N v_l) (w None: all 1); nothing is reduced"""
        n = len(V_list)
        Va = (C.c_void_p * max(n, 1))(*[_ptr(v) for v in V_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        _chk(self.L.tp_elasticity_mass_sensitivity(self.handle, n, Va, wa, _ptr(xPhys), float(scale), _ptr(out)),
             "tp_elasticity_mass_sensitivity")

    def _eigen_start(self, q):
        """q fixed, linearly independent fields of the GLOBAL node index and component (any slab count starts from the same
        fields), times N: smooth profiles along x in the three directions plus a fixed oscillating part"""
        p = self.grid.part
        gn = torch.arange(p.plane * p.nz_local, dtype=torch.float64) + float(p.plane * p.node_z0)
        xi = (torch.remainder(gn, p.nx) + 1.0) / p.nx
        out = []
        for j in range(q):
            f = torch.zeros(gn.numel(), 3, dtype=torch.float64)
            f[:, j % 3] = xi ** (1 + j // 3)
            for c in range(3):
                f[:, c] += 0.1 * torch.cos(1.7 * (j + 1) * (3.0 * gn + c + 1.0))
            out.append(f.reshape(-1).to(self.U.device) * self.N)
        return out

    def Eigenmodes(self, nev, xPhys, rho0=1.0, x_low=0.1, guard=2, tol=1e-6, max_iter=30):
        """The lowest nev eigenvalues of A phi = lambda B phi on the CURRENT assembly (xPhys: the design it was made from) by
        subspace iteration with Rayleigh-Ritz on a block of q = nev + guard vectors -> dict(lam, iters, ksp_its, residuals, gap).
        Every iteration: Y_j = A^-1 B X_j (tp_elasticity_solve from X_j / theta_j), the products A Y and B Y, the two q x q
        matrices Y^T A Y and Y^T B Y (one pass each), their dense eigenproblem on the host, X = Y Q.  The Ritz values are
        Rayleigh quotients of true products with A: upper bounds whatever the solve's tolerance.  The products are
        MatMultKrylov's, the operator CG itself multiplies with: on the lowest modes, which are dominated by translation element
        by element, it is KE's action to rounding, where MatMult's packed form sits 1e-12 of lambda away (measured).  Stops when
        ||A x_i - theta_i B x_i|| / ||A x_i|| <= tol for every i < nev; TopOptError at max_iter.  A second call with the same q
        starts from the previous block (warm start across design iterations).  During the call the solver's rtol is
        min(opts.rtol, tol / 10); afterwards it is set back to opts.rtol, the value this object holds -- the library has no call
        that reads the handle's tolerance back, so one set behind this object's back through tp_elasticity_set_tolerances is
        replaced by it: change the tolerance through SetTolerances, which keeps opts in step.
        On more than one rank the solver needs at least two multigrid levels: TopOptError (TP_ERR_ARG) otherwise, before anything
        is launched.  The one run of that configuration (three slabs of two layers, one level) did not finish within four minutes
        where one rank takes half a second for the same 1435 solver iterations, and why is not known."""
        import numpy as np
        import scipy.linalg
        nev, guard = int(nev), int(guard)
        q = nev + guard
        if nev < 1 or guard < 0 or q > _lib.MAX_CASES:
            raise ValueError("Eigenmodes: need nev >= 1, guard >= 0 and nev + guard <= TP_MAX_CASES = %d, got %d + %d"
                             % (_lib.MAX_CASES, nev, guard))
        if self.grid.part.nranks > 1 and self.opts.nlvls < 2:
            raise TopOptError(1, "Eigenmodes", "Eigenmodes failed: TP_ERR_ARG (on %d ranks the solver needs at least two multigrid "
                              "levels, it has %d)" % (self.grid.part.nranks, self.opts.nlvls))
        g, sl = self.grid, self.grid.part.owned_slice(3)
        self.MassAssemble(xPhys, rho0, x_low)
        E = self._eig
        if E is None or E["q"] != q:
            E = self._eig = dict(q=q, theta=None, X=self._eigen_start(q))
            for name in ("AX", "BX", "Y", "AY", "BY"):
                E[name] = [g.node_vec(3) for _ in range(q)]
        E["nev"], E["lam"] = nev, None
        X, AX, BX, Y, AY, BY = (E[k] for k in ("X", "AX", "BX", "Y", "AY", "BY"))
        own = lambda vs: [v[sl] for v in vs]
        n_all = X[0].numel()
        ksp_its, res = 0, None
        _chk(self.L.tp_elasticity_set_tolerances(self.handle, min(self.opts.rtol, 0.1 * tol), -1.0, -1.0, -1), "tp_elasticity_set_tolerances")
        try:
            for j in range(q):
                self.MassMult(X[j], BX[j])
            for it in range(1, max_iter + 1):
                for j in range(q):     # Y_j = A^-1 B X_j, from X_j / theta_j
                    if E["theta"] is None:
                        Y[j].zero_()
                    else:
                        Y[j].copy_(X[j])
                        _chk(self.L.tp_vec_scale(g.handle, _ptr(Y[j]), 1.0 / E["theta"][j], n_all), "tp_vec_scale")
                    rc, its, _, _, _ = self._solve(BX[j], Y[j])
                    _chk(rc, "tp_elasticity_solve (eigenmodes)")
                    ksp_its += its
                    # clamped dofs carry exactly 0 (the preconditioner leaves rounding-sized values there)
                    _chk(self.L.tp_vec_pointwise(g.handle, _ptr(Y[j]), _ptr(Y[j]), _ptr(self.N), 0, n_all), "tp_vec_pointwise")
                    self.MatMultKrylov(Y[j], AY[j])
                    self.MassMult(Y[j], BY[j])
                Kt, Mt = g.BlockGram(own(Y), own(AY)), g.BlockGram(own(Y), own(BY))
                Kt, Mt = 0.5 * (Kt + Kt.T), 0.5 * (Mt + Mt.T)
                try:
                    theta, Q = scipy.linalg.eigh(Kt, Mt)
                except (np.linalg.LinAlgError, ValueError) as exc:
                    raise TopOptError(3, "Eigenmodes (Rayleigh-Ritz: the block lost its rank in iteration %d: %s)" % (it, exc))
                g.BlockCombine(Y, Q, X)
                g.BlockCombine(AY, Q, AX)
                g.BlockCombine(BY, Q, BX)
                E["theta"] = [float(t) for t in theta]
                for i in range(nev):   # Y is free until the next solve: A x_i - theta_i B x_i
                    Y[i].copy_(AX[i])
                    _chk(self.L.tp_vec_axpby(g.handle, _ptr(Y[i]), -E["theta"][i], _ptr(BX[i]), 1.0, n_all), "tp_vec_axpby")
                rr, aa = g.BlockGram(own(Y[:nev]), own(Y[:nev])), g.BlockGram(own(AX[:nev]), own(AX[:nev]))
                res = [float(np.sqrt(rr[i, i] / aa[i, i])) for i in range(nev)]
                if max(res) <= tol:
                    break
            else:
                err = TopOptError(3, "Eigenmodes", "Eigenmodes: %d iterations without reaching tol %.1e; residuals %s, Ritz values %s"
                                  % (max_iter, tol, " ".join("%.3e" % r for r in res), " ".join("%.9e" % t for t in E["theta"][:nev])))
                err.residuals = res
                raise err
        finally:
            rc_restore = self.L.tp_elasticity_set_tolerances(self.handle, self.opts.rtol, -1.0, -1.0, -1)
        _chk(rc_restore, "tp_elasticity_set_tolerances (restoring rtol)")
        th = E["theta"]
        E["lam"] = th[:nev]
        return dict(lam=list(th[:nev]), iters=it, ksp_its=ksp_its, residuals=res,
                    gap=(th[nev] / th[nev - 1] - 1.0) if guard > 0 else float("inf"))

    def EigenVectors(self):
        """the nev fields of the last Eigenmodes call, B-normalised (phi_i^T B phi_j = delta_ij); the object's own tensors"""
        if self._eig is None or self._eig["lam"] is None:
            raise TopOptError(2, "EigenVectors (no converged Eigenmodes call)")
        return self._eig["X"][:self._eig["nev"]]

    def EigenSensitivity(self, out, xPhys, Emin, Emax, penal):
        """out = dJ/dx of J = sum_{i < nev} 1 / lambda_i of the last Eigenmodes call -> J: the bilinear pass of Response with
        U = V = Phi and the weights lambda_i^-2, plus the mass term with the weights 1 / lambda_i.  Nothing is reduced."""
        Phi = self.EigenVectors()
        lam = self._eig["lam"]
        self.Response(Phi, None, [1.0 / (l * l) for l in lam], xPhys, Emin, Emax, penal, 0.0, dfdx=out, sums=False)
        self.MassSensitivity(Phi, [1.0 / l for l in lam], xPhys, 1.0, out)
        return sum(1.0 / l for l in lam)

    # ---- linear buckling: B phi = mu A phi, A as above, B = -N G(x, u) N the stress stiffness of a state u ----
    def SetUpLoadAndBC_Axial(self, total=1.0):
        """The cantilever's clamp (face x = xmin) under a uniform traction along -x on the face x = xmax, `total` in sum:
        consistent nodal loads, total / (ey ez) / 4 from every face element to each of its four nodes.  A column in
        compression: the load a buckling analysis starts from.  Single rank or z-slabs (global z index decides)."""
        self.SetUpLoadAndBC()   # the supports
        self.SetBC(self.N, self.AxialLoad(total))

    def AxialLoad(self, total=1.0):
        """the right-hand side of SetUpLoadAndBC_Axial in the local node layout (for AddLoadCase too)"""
        p = self.grid.part
        nx, ny, nzl = p.nx, p.ny, p.nz_local
        R = torch.zeros(nzl, ny, nx, 3, dtype=torch.float64)
        per = float(total) / ((ny - 1) * (p.nz - 1)) / 4.0
        kz = torch.arange(nzl) + p.node_z0
        wz = torch.where((kz == 0) | (kz == p.nz - 1), 1.0, 2.0).to(torch.float64)
        wy = torch.full((ny,), 2.0, dtype=torch.float64)
        wy[0] = wy[ny - 1] = 1.0
        R[:, :, nx - 1, 0] = -per * wz[:, None] * wy[None, :]
        return R.reshape(-1).to(self.U.device)

    def GeomAssemble(self, xPhys, Emax, penal, U=None):
        """Emax x^penal g_e(U_e) for GeomMult, once per design and state (U None: case 0's state)"""
        _chk(self.L.tp_elasticity_geom_assemble(self.handle, _ptr(xPhys), _ptr(self.U if U is None else U), float(Emax), float(penal)),
             "tp_elasticity_geom_assemble")

    def GeomMult(self, phi, y=None):
        """y = N G N phi on the owned node planes (ghost planes of y stay as they are)"""
        y = torch.zeros_like(phi) if y is None else y
        _chk(self.L.tp_elasticity_geom_apply(self.handle, _ptr(phi), _ptr(y)), "tp_elasticity_geom_apply")
        return y

    def GeomSensitivity(self, Phi_list, w, xPhys, U, Emax, penal, scale, out):
        """out += scale penal x^(penal-1) Emax sum_l w_l (N phi_l)^T (g_e(U_e) (x) I3) (N phi_l) (w None: all 1); nothing is reduced"""
        n = len(Phi_list)
        Va = (C.c_void_p * max(n, 1))(*[_ptr(v) for v in Phi_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        _chk(self.L.tp_elasticity_geom_sensitivity(self.handle, n, Va, wa, _ptr(xPhys), _ptr(U), float(Emax), float(penal), float(scale),
                                                   _ptr(out)), "tp_elasticity_geom_sensitivity")

    def GeomAdjointRHS(self, Phi_list, w, xPhys, Emax, penal, scale, out):
        """out = scale sum_l w_l d((N phi_l)^T G (N phi_l)) / dU on the owned node planes, supports not applied; ghost planes stay"""
        n = len(Phi_list)
        Va = (C.c_void_p * max(n, 1))(*[_ptr(v) for v in Phi_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        _chk(self.L.tp_elasticity_geom_adjoint_rhs(self.handle, n, Va, wa, _ptr(xPhys), float(Emax), float(penal), float(scale), _ptr(out)),
             "tp_elasticity_geom_adjoint_rhs")
        return out

    def GeomTables(self):
        """the element's tables (numpy): gradN [8 gp, 3, 8 nodes] and C0 B [8 gp, 6, 24]"""
        import numpy as np
        gn, cb = np.zeros(192), np.zeros(1152)
        _chk(self.L.tp_elasticity_get_geom_tables(self.handle, gn.ctypes.data, cb.ctypes.data), "tp_elasticity_get_geom_tables")
        return gn.reshape(8, 3, 8), cb.reshape(8, 6, 24)

    def BucklingModes(self, nev, xPhys, Emax, penal, U=None, guard=None, tol=1e-6, max_iter=60):
        """The nev largest POSITIVE eigenvalues mu of B phi = mu A phi on the CURRENT assembly (xPhys: the design it was made from;
        U: the state whose stresses make B, default case 0's) -> dict(mu, factor, iters, ksp_its, residuals, gap); the load
        factors are 1 / mu.  Subspace iteration with Rayleigh-Ritz on a block of q = nev + guard vectors in the manner of
        Eigenmodes, with these differences: the iteration is Y_j = A^-1 B X_j, warm-started from mu_j X_j; the Ritz problem is
        eigh(Y^T B Y, Y^T A Y) -- the SPD matrix second (A Y is MatMultKrylov's); B is indefinite, so the block converges to the
        q eigenvalues of largest MAGNITUDE, of both signs, and the wanted ones are the nev largest positive Ritz values --
        convergence is tested on those alone, ||B x - mu A x|| / ||B x|| <= tol.  guard None: q = TP_MAX_CASES, which keeps room
        for the negative ones.  Fewer than nev positive Ritz values in the block at the end, or max_iter reached: TopOptError
        with the residuals and the Ritz values; no wrong value is returned silently.  The rules for rtol and for several ranks
        with fewer than two multigrid levels are Eigenmodes'."""
        import numpy as np
        import scipy.linalg
        nev = int(nev)
        guard = _lib.MAX_CASES - nev if guard is None else int(guard)
        q = nev + guard
        if nev < 1 or guard < 0 or q > _lib.MAX_CASES:
            raise ValueError("BucklingModes: need nev >= 1, guard >= 0 and nev + guard <= TP_MAX_CASES = %d, got %d + %d"
                             % (_lib.MAX_CASES, nev, guard))
        if self.grid.part.nranks > 1 and self.opts.nlvls < 2:
            raise TopOptError(1, "BucklingModes", "BucklingModes failed: TP_ERR_ARG (on %d ranks the solver needs at least two multigrid "
                              "levels, it has %d)" % (self.grid.part.nranks, self.opts.nlvls))
        g, sl = self.grid, self.grid.part.owned_slice(3)
        U = self.U if U is None else U
        self.GeomAssemble(xPhys, Emax, penal, U)
        E = self._buck
        if E is None or E["q"] != q:
            E = self._buck = dict(q=q, theta=None, X=self._eigen_start(q))
            for name in ("AX", "BX", "Y", "AY", "BY"):
                E[name] = [g.node_vec(3) for _ in range(q)]
        E["nev"], E["mu"], E["U"] = nev, None, U
        X, AX, BX, Y, AY, BY = (E[k] for k in ("X", "AX", "BX", "Y", "AY", "BY"))
        own = lambda vs: [v[sl] for v in vs]
        n_all = X[0].numel()
        ksp_its, res, npos = 0, None, 0

        def Bmult(v, out):   # B = -N G N
            self.GeomMult(v, out)
            _chk(self.L.tp_vec_scale(g.handle, _ptr(out), -1.0, n_all), "tp_vec_scale")

        _chk(self.L.tp_elasticity_set_tolerances(self.handle, min(self.opts.rtol, 0.1 * tol), -1.0, -1.0, -1), "tp_elasticity_set_tolerances")
        try:
            for j in range(q):
                Bmult(X[j], BX[j])
            for it in range(1, max_iter + 1):
                for j in range(q):     # Y_j = A^-1 B X_j, from mu_j X_j
                    if E["theta"] is None:
                        Y[j].zero_()
                    else:
                        Y[j].copy_(X[j])
                        _chk(self.L.tp_vec_scale(g.handle, _ptr(Y[j]), E["theta"][j], n_all), "tp_vec_scale")
                    rc, its, _, _, _ = self._solve(BX[j], Y[j])
                    _chk(rc, "tp_elasticity_solve (buckling modes)")
                    ksp_its += its
                    # clamped dofs carry exactly 0 (the preconditioner leaves rounding-sized values there)
                    _chk(self.L.tp_vec_pointwise(g.handle, _ptr(Y[j]), _ptr(Y[j]), _ptr(self.N), 0, n_all), "tp_vec_pointwise")
                    self.MatMultKrylov(Y[j], AY[j])
                    Bmult(Y[j], BY[j])
                Bt, At = g.BlockGram(own(Y), own(BY)), g.BlockGram(own(Y), own(AY))
                Bt, At = 0.5 * (Bt + Bt.T), 0.5 * (At + At.T)
                try:
                    theta, Q = scipy.linalg.eigh(Bt, At)
                except (np.linalg.LinAlgError, ValueError) as exc:
                    raise TopOptError(3, "BucklingModes (Rayleigh-Ritz: the block lost its rank in iteration %d: %s)" % (it, exc))
                order = np.argsort(-theta)            # the positive ones first, the largest in front
                theta, Q = theta[order], np.ascontiguousarray(Q[:, order])
                g.BlockCombine(Y, Q, X)
                g.BlockCombine(AY, Q, AX)
                g.BlockCombine(BY, Q, BX)
                E["theta"] = [float(t) for t in theta]
                npos = int((theta > 0.0).sum())
                if npos < nev:
                    res = None
                    continue
                for i in range(nev):   # Y is free until the next solve: B x_i - mu_i A x_i
                    Y[i].copy_(BX[i])
                    _chk(self.L.tp_vec_axpby(g.handle, _ptr(Y[i]), -E["theta"][i], _ptr(AX[i]), 1.0, n_all), "tp_vec_axpby")
                rr, bb = g.BlockGram(own(Y[:nev]), own(Y[:nev])), g.BlockGram(own(BX[:nev]), own(BX[:nev]))
                res = [float(np.sqrt(rr[i, i] / bb[i, i])) for i in range(nev)]
                if max(res) <= tol:
                    break
            else:
                ritz = " ".join("%.9e" % t for t in E["theta"])
                if npos < nev:
                    err = TopOptError(3, "BucklingModes", "BucklingModes: %d positive Ritz values in the block of %d after %d iterations, "
                                      "%d wanted (the load does not compress the structure enough, or the block is too small); "
                                      "Ritz values %s" % (npos, q, max_iter, nev, ritz))
                else:
                    err = TopOptError(3, "BucklingModes", "BucklingModes: %d iterations without reaching tol %.1e; residuals %s, Ritz values %s"
                                      % (max_iter, tol, " ".join("%.3e" % r for r in res), ritz))
                err.residuals = res
                raise err
        finally:
            rc_restore = self.L.tp_elasticity_set_tolerances(self.handle, self.opts.rtol, -1.0, -1.0, -1)
        _chk(rc_restore, "tp_elasticity_set_tolerances (restoring rtol)")
        th = E["theta"]
        E["mu"] = th[:nev]
        nxt = max([abs(t) for t in th[nev:]], default=0.0)   # the largest magnitude behind the wanted ones
        return dict(mu=list(th[:nev]), factor=1.0 / th[0], iters=it, ksp_its=ksp_its, residuals=res,
                    gap=(1.0 - nxt / th[nev - 1]) if guard > 0 else float("inf"), ritz=list(th))

    def BucklingVectors(self):
        """the nev fields of the last BucklingModes call, A-normalised (phi_i^T A phi_j = delta_ij); the object's own tensors"""
        if self._buck is None or self._buck["mu"] is None:
            raise TopOptError(2, "BucklingVectors (no converged BucklingModes call)")
        return self._buck["X"][:self._buck["nev"]]

    def BucklingSensitivity(self, out, xPhys, Emin, Emax, penal, P=8.0):
        """out = dJ/dx of J = (sum_{i < nev} mu_i^P)^(1/P) of the last BucklingModes call -> (J, its), on the CURRENT assembly and
        the state the modes were made from, for a design-independent load.  With c_i = (mu_i / J)^(P-1):
        the bilinear pass of Response with U = V = Phi and the weights c_i mu_i (-c_i mu_i phi^T dA/dx phi), the explicit part
        of the stress stiffness (GeomSensitivity, weights c_i, scale -1), and the state part: the adjoint solve
        A v = N r, r = -sum c_i d(phi_i^T G phi_i)/du (GeomAdjointRHS), warm-started from the previous call's v, then the bilinear
        pass with U = u, V = v.  The adjoint solve's figures go to adjoint_its / adjoint_rnorm / adjoint_bnorm."""
        Phi = self.BucklingVectors()
        mu, U = self._buck["mu"], self._buck["U"]
        J = sum(m ** P for m in mu) ** (1.0 / P)
        c = [(m / J) ** (P - 1.0) for m in mu]
        if self._buck_adj is None:
            self._buck_adj, self._buck_rhs = self.grid.node_vec(3), self.grid.node_vec(3)   # (ghost planes of the load stay 0)
            self._buck_row = self.grid.elem_vec()
        self.Response(Phi, None, [ci * m for ci, m in zip(c, mu)], xPhys, Emin, Emax, penal, 0.0, dfdx=out, sums=False)
        self.GeomSensitivity(Phi, c, xPhys, U, Emax, penal, -1.0, out)
        self.GeomAdjointRHS(Phi, c, xPhys, Emax, penal, -1.0, self._buck_rhs)
        rc, its, self.adjoint_rnorm, self.adjoint_bnorm, _ = self._solve(self._buck_rhs, self._buck_adj)
        self.adjoint_its = its
        _chk(rc, "tp_elasticity_solve (buckling adjoint)")
        self.Response([U], [self._buck_adj], None, xPhys, Emin, Emax, penal, 0.0, dfdx=self._buck_row, sums=False)
        _chk(self.L.tp_vec_axpby(self.grid.handle, _ptr(out), 1.0, _ptr(self._buck_row), 1.0, out.numel()), "tp_vec_axpby")
        return J, its

    def KSPSolve(self, hist_cap=0, case=0, rhs=None):
        """solve load case `case` on the last assembly, warm-started from that case's own state (rhs: another right-hand side
        than the case's fixed load)"""
        import time
        t0 = time.perf_counter()   # the solve ends with a host read of ||r||: wall time == device time
        rc, its, rn, bn, hist = self._solve(self._case_rhs[case] if rhs is None else rhs, self._case_U[case], hist_cap)
        self.last_solve_s = time.perf_counter() - t0
        self.last_its, self.last_rnorm, self.last_bnorm = its, rn, bn
        self.last_hist = hist[: min(its + 1, hist_cap)] if hist_cap else None
        self.case_its[case], self.case_rnorm[case], self.case_bnorm[case] = its, rn, bn
        _chk(rc, "tp_elasticity_solve")
        return its

    def _solve(self, RHS, U, hist_cap=0):
        """tp_elasticity_solve on the last assembly -> (rc, its, rnorm, bnorm, hist); records nothing, the caller checks rc"""
        import numpy as np
        its, rn, bn = C.c_int(), C.c_double(), C.c_double()
        hist = np.zeros(max(hist_cap, 1))
        rc = self.L.tp_elasticity_solve(self.handle, _ptr(RHS), _ptr(U), C.byref(its), C.byref(rn),
                                        C.byref(bn), hist.ctypes.data if hist_cap else None, hist_cap)
        return rc, its.value, rn.value, bn.value, hist

    def SolveState(self, xPhys, Emin, Emax, penal, hist_cap=0):
        """LinearElasticity.cc:182-223; several load cases: one assembly, then every case in index order"""
        self.AssembleStiffnessMatrix(xPhys, Emin, Emax, penal)
        loaded = self.body_force is not None or self.thermal is not None
        if loaded:
            self._form_totals(xPhys)
        for case in range(self.ncases):
            its = self.KSPSolve(hist_cap, case, rhs=self._case_total[case] if loaded else None)
        return its

    def Response(self, U_list, V_list, w, xPhys, Emin, Emax, penal, volfrac, dfdx=None, dgdx=None, sums=True):
        """tp_elasticity_response: fx = sum_l w_l f_l with f_l = sum_e E_e v_l^T KE u_l, gx, dfdx, dgdx for all cases in
        one pass over the elements -> (fx, gx, f_case).  V_list None, or an entry None: V_l = U_l (compliance);
        w None: all weights 1.  sums=False: nothing is reduced and the host does not wait -> (None, None, None)."""
        n = len(U_list)
        Ua = (C.c_void_p * max(n, 1))(*[_ptr(u) for u in U_list])
        Va = None if V_list is None else (C.c_void_p * max(n, 1))(*[_ptr(v) for v in V_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        fx, gx, fc = C.c_double(), C.c_double(), (C.c_double * max(n, 1))()
        _chk(self.L.tp_elasticity_response(self.handle, n, Ua, Va, wa, _ptr(xPhys), Emin, Emax, penal, volfrac,
                                           fc if sums else None, C.byref(fx) if sums else None, C.byref(gx) if sums else None,
                                           _ptr(dfdx), _ptr(dgdx)), "tp_elasticity_response")
        return (fx.value, gx.value, list(fc)[:n]) if sums else (None, None, None)

    def StressForm(self):
        """the von Mises form M = B0^T C^T Vm C B0 of the element (24 x 24 row-major, numpy array of 576): s_e = u_e^T M u_e"""
        import numpy as np
        m = np.zeros(576)
        _chk(self.L.tp_elasticity_get_stress_form(self.handle, m.ctypes.data), "tp_elasticity_get_stress_form")
        return m

    def Stress(self, xPhys, Emax, q, P, U=None, vm=None, dpdx=None, adj_rhs=None):
        """tp_elasticity_stress on the state U (default: case 0's): vm_e = Emax x_e^q sqrt(u_e^T M u_e) into vm, the explicit
        part of d pnorm / dx into dpdx, d pnorm / dU (owned planes, supports not applied) into adj_rhs -> (pnorm, vm_max).
        With vm the only output nothing is reduced, the host does not wait and (None, None) comes back (the field together with
        the two numbers: ask for dpdx as well)."""
        sums = not (vm is not None and dpdx is None and adj_rhs is None)
        pn, mx = C.c_double(), C.c_double()
        _chk(self.L.tp_elasticity_stress(self.handle, _ptr(self.U if U is None else U), _ptr(xPhys), Emax, q, P, _ptr(vm),
                                         C.byref(pn) if sums else None, C.byref(mx) if sums else None, _ptr(dpdx), _ptr(adj_rhs)),
             "tp_elasticity_stress")
        return (pn.value, mx.value) if sums else (None, None)

    def StressSensitivity(self, dsdx, xPhys, Emin, Emax, penal, q, P, case=0):
        """d pnorm / dx of the von Mises p-norm of load case `case` on the CURRENT assembly and state -> (pnorm, vm_max, its):
        Stress, the adjoint solve K lam = N adj_rhs (warm-started from the previous design iteration's lam), the bilinear
        pass of Response with V = lam, and dsdx += dpdx.  The adjoint solve's figures go to adjoint_its / adjoint_rnorm /
        adjoint_bnorm; last_its and the per-case records of the state solves stay as they are."""
        if self.lam is None:
            self.lam, self._stress_rhs = self.grid.node_vec(3), self.grid.node_vec(3)   # (ghost planes of the load stay 0)
            self._stress_dpdx = self.grid.elem_vec()
        U = self._case_U[case]
        pn, mx = self.Stress(xPhys, Emax, q, P, U=U, dpdx=self._stress_dpdx, adj_rhs=self._stress_rhs)
        if pn == 0.0:   # no stress anywhere: a zero load, whose solution is lam = 0 -- no solve
            self.lam.zero_()
            self.adjoint_its, self.adjoint_rnorm, self.adjoint_bnorm = 0, 0.0, 0.0
            dsdx.zero_()
            return pn, mx, 0
        rc, its, self.adjoint_rnorm, self.adjoint_bnorm, _ = self._solve(self._stress_rhs, self.lam)
        self.adjoint_its = its
        _chk(rc, "tp_elasticity_solve (adjoint)")
        self.Response([U], [self.lam], None, xPhys, Emin, Emax, penal, 0.0, dfdx=dsdx, sums=False)
        if self.body_force is not None:   # d pnorm/dx = dpdx - lam^T (dK/dx u - df/dx)
            self.BodySensitivity([self.lam], None, xPhys, 1.0, dsdx)
        _chk(self.L.tp_vec_axpby(self.grid.handle, _ptr(dsdx), 1.0, _ptr(self._stress_dpdx), 1.0, dsdx.numel()), "tp_vec_axpby")
        return pn, mx, its

    def Objective(self, xPhys, Emin, Emax, penal, volfrac, dfdx=None, dgdx=None):
        fx, gx = C.c_double(), C.c_double()
        _chk(self.L.tp_elasticity_objective(self.handle, _ptr(self.U), _ptr(xPhys), Emin, Emax, penal, volfrac,
                                            C.byref(fx), C.byref(gx), _ptr(dfdx), _ptr(dgdx)),
             "tp_elasticity_objective")
        return fx.value, gx.value

    def _evaluate(self, dfdx, dgdx, sums, xPhys, Emin, Emax, penal, volfrac):
        """objective and sensitivities of the current states -> (fx, gx), (None, None) without sums: one case through the
        reference's three single-case entry points, several through Response (last_f_case: the f_l)"""
        if self.ncases > 1:
            fx, gx, f_case = self.Response(self._case_U, None, self.case_weight, xPhys, Emin, Emax, penal, volfrac, dfdx, dgdx, sums)
            if sums:
                self.last_f_case = f_case
            return fx, gx
        if not sums:
            _chk(self.L.tp_elasticity_sensitivities(self.handle, _ptr(self.U), _ptr(xPhys), Emin, Emax, penal, _ptr(dfdx),
                                                    _ptr(dgdx)), "tp_elasticity_sensitivities")
            return None, None
        if dfdx is not None or dgdx is not None:
            return self.Objective(xPhys, Emin, Emax, penal, volfrac, dfdx, dgdx)
        fx, gx = C.c_double(), C.c_double()
        _chk(self.L.tp_elasticity_objective_only(self.handle, _ptr(self.U), _ptr(xPhys), Emin, Emax, penal, volfrac,
                                                 C.byref(fx), C.byref(gx)), "tp_elasticity_objective_only")
        return fx.value, gx.value

    def ComputeObjectiveConstraintsSensitivities(self, dfdx, dgdx, xPhys, Emin, Emax, penal, volfrac, hist_cap=0):
        """LinearElasticity.cc:363-445 -> (fx, gx); several load cases: fx = sum_l w_l u_l^T K u_l (last_f_case: the f_l)"""
        self.SolveState(xPhys, Emin, Emax, penal, hist_cap)
        fx, gx = self._evaluate(dfdx, dgdx, True, xPhys, Emin, Emax, penal, volfrac)
        if self.body_force is not None:   # u^T K u = (F + f)^T u as it stands; dfdx gains 2 d(u^T N f)/dx per case
            self.BodySensitivity(self._case_U, self.case_weight, xPhys, 2.0, dfdx)
        if self.thermal is not None:      # the same at fixed T; what T's own dependence on the design adds is the caller's
            self.ThermalSensitivity(self._case_U, self.case_weight, xPhys, self._temperature_set(), 2.0, dfdx)
        return fx, gx

    def ComputeObjectiveConstraints(self, xPhys, Emin, Emax, penal, volfrac, hist_cap=0):
        """LinearElasticity.cc:225-297: solve, then fx and gx -- no sensitivities -> (fx, gx)"""
        self.SolveState(xPhys, Emin, Emax, penal, hist_cap)
        return self._evaluate(None, None, True, xPhys, Emin, Emax, penal, volfrac)

    def ComputeSensitivities(self, dfdx, dgdx, xPhys, Emin, Emax, penal, volfrac=0.0):
        """LinearElasticity.cc:299-361: dfdx, dgdx of the current state U (no solve); several load cases: of all states"""
        self._evaluate(dfdx, dgdx, False, xPhys, Emin, Emax, penal, volfrac)
        if self.body_force is not None:
            self.BodySensitivity(self._case_U, self.case_weight, xPhys, 2.0, dfdx)
        if self.thermal is not None:
            self.ThermalSensitivity(self._case_U, self.case_weight, xPhys, self._temperature_set(), 2.0, dfdx)

    # ---- introspection used by the parity tests ----------------------------
    def petsc_options(self):
        """The solver of the last assembly as a literal PETSc 3.11 option string (numeric Chebyshev windows per level)."""
        buf = C.create_string_buffer(8192)
        n = self.L.tp_elasticity_petsc_options(self.handle, buf, len(buf))
        if n < 0:
            raise TopOptError(2, "tp_elasticity_petsc_options (no assembly yet)")
        return buf.value.decode()

    def coarse_direct_active(self):
        """rows of the coarsest level if the last assembly factored it (SolverOptions.coarse_direct), else 0"""
        return self.L.tp_elasticity_coarse_direct_active(self.handle)

    def xcd_status(self):
        """process-wide: (recoveries from one-XCD kernels that gave up, one-XCD forms off, factorisation no longer deferred)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self.L.tp_xcd_status(C.byref(a), C.byref(b), C.byref(c))
        return a.value, bool(b.value), bool(c.value)

    def set_cycles(self, cycles):
        """PCMGSetCycleTypeOnLevel: cycles[l] cycles of level l + 1 per visit of level l (l = 0 finest; 1 = V, 2 = W)"""
        arr = (C.c_int * len(cycles))(*[int(v) for v in cycles])
        _chk(self.L.tp_elasticity_set_cycles(self.handle, arr, len(cycles)), "tp_elasticity_set_cycles")

    def level_pc(self, l, pc, r):
        """ksp_mode 1: z = M^-1 r on level l, pc 0 = PCJACOBI, 1 = PCSOR (one symmetric Gauss-Seidel sweep)"""
        z = torch.zeros_like(r)
        _chk(self.L.tp_elasticity_level_pc(self.handle, l, pc, _ptr(r), _ptr(z)), "tp_elasticity_level_pc")
        return z

    def level_gs(self, l, backward, b, x):
        """ksp_mode 1: one Gauss-Seidel sweep of PCSOR on level l, in place on x from the iterate it holds (forward or backward)"""
        _chk(self.L.tp_elasticity_level_gs(self.handle, l, int(backward), _ptr(b), _ptr(x)), "tp_elasticity_level_gs")
        return x

    def level_gmres(self, l, pc, m, its, b, x, zero_guess=False, rtol=-1.0):
        """ksp_mode 1: the level's left-preconditioned GMRES(m), at most `its` iterations (rtol < 0: no test)"""
        done = C.c_int(0)
        _chk(self.L.tp_elasticity_level_gmres(self.handle, l, pc, m, its, rtol, _ptr(b), _ptr(x), int(zero_guess),
                                              C.byref(done)), "tp_elasticity_level_gmres")
        return x, done.value

    def precond(self, r):
        z = torch.zeros_like(r)
        _chk(self.L.tp_elasticity_precond(self.handle, _ptr(r), _ptr(z)), "tp_elasticity_precond")
        return z

    def smooth_dot(self, l, b, x, k, zero_guess=False):
        """smooth() whose last step is the fused form that also returns b . x_out (CG's r . z): (x, dot)"""
        d = C.c_double()
        _chk(self.L.tp_elasticity_smooth_dot(self.handle, l, _ptr(b), _ptr(x), k, int(zero_guess), C.byref(d)), "tp_elasticity_smooth_dot")
        return x, d.value


def heat_sink_and_load(nx, ny, nz, h, q0=1.0, node_z0=0, nz_local=None):
    """The built-in heat-sink problem on nx x ny x nz nodes (global counts), planes [node_z0, node_z0 + nz_local) of it, as
    torch CPU tensors (N, RHS) in the local node layout.  Sink (N = 0): the nodes of the face i = 0 with
    |2j - (ny-1)| <= max(1, (ny-1)//4) and |2k - (nz-1)| <= max(1, (nz-1)//4), never empty.  Load: a uniform volumetric source,
    rhs_n = q0 hx hy hz / 8 x (number of elements around node n)."""
    nzl = nz if nz_local is None else nz_local
    hx, hy, hz = (h, h, h) if isinstance(h, (int, float)) else tuple(h)
    j, k = torch.arange(ny), torch.arange(nzl) + node_z0
    sj = (2 * j - (ny - 1)).abs() <= max(1, (ny - 1) // 4)
    sk = (2 * k - (nz - 1)).abs() <= max(1, (nz - 1) // 4)
    N = torch.ones(nzl, ny, nx, dtype=torch.float64)
    N[:, :, 0] = 1.0 - (sk[:, None] & sj[None, :]).to(torch.float64)
    around = lambda idx, n: torch.where((idx == 0) | (idx == n - 1), 1.0, 2.0).to(torch.float64)
    cnt = around(k, nz)[:, None, None] * around(j, ny)[None, :, None] * around(torch.arange(nx), nx)[None, None, :]
    return N.reshape(-1), (q0 * hx * hy * hz / 8.0 * cnt).reshape(-1)


class HeatConduction(_Handle, _LevelStats):
    """Steady heat conduction on the MI355X (include/topopt_amd.h: tp_conduction): conductivity k = kmin + x^p (kmax - kmin) per
    element, temperature T per node, heat sink where N = 0.  Methods are named as on LinearElasticity."""
    _destroy, _prefix, _dof = "tp_conduction_destroy", "tp_conduction", 1

    def __init__(self, grid, opts=None):
        self.grid, self.L = grid, grid.L
        self.opts = opts or SolverOptions()
        self.handle = C.c_void_p()
        self._o = self.opts.c_struct()
        _chk(self.L.tp_conduction_create(C.byref(self.handle), grid.handle, C.byref(self._o)), "tp_conduction_create")
        grid._adopt(self)
        self.T = grid.node_vec(1)       # state, persists across design iterations (warm start)
        self.RHS = grid.node_vec(1)
        self.N = grid.node_vec(1)
        self.last_its, self.last_rnorm, self.last_bnorm, self.last_hist = 0, 0.0, 0.0, None

    ncases = 1   # one load, one state: what the driver's records and restart files ask a physics object for

    def LoadCaseU(self, case):
        return self.T

    @property
    def KT(self):
        import numpy as np
        kt = np.zeros(64)
        _chk(self.L.tp_conduction_get_ke(self.handle, kt.ctypes.data), "tp_conduction_get_ke")
        return kt

    def SetUpLoadAndBC(self, q0=1.0):
        """the built-in heat-sink problem (heat_sink_and_load); single rank or z-slabs (global z index decides; the load on the
        owned planes only)"""
        p = self.grid.part
        N, R = heat_sink_and_load(p.nx, p.ny, p.nz, self.grid.h, q0, p.node_z0, p.nz_local)
        off, own = self.L.tp_grid_owned_node_offset(self.grid.handle), self.L.tp_grid_owned_nodes(self.grid.handle)
        R[:off] = 0.0
        R[off + own:] = 0.0
        self.SetBC(N.to(self.T.device), R.to(self.T.device))

    def SetBC(self, N, RHS):
        self.N.copy_(N)
        self.RHS.copy_(RHS)
        _chk(self.L.tp_conduction_set_bc(self.handle, _ptr(self.N)), "tp_conduction_set_bc")

    def SetTolerances(self, rtol=-1.0, atol=-1.0, dtol=-1.0, max_it=-1):
        _chk(self.L.tp_conduction_set_tolerances(self.handle, float(rtol), float(atol), float(dtol), int(max_it)), "tp_conduction_set_tolerances")
        for name, v in (("rtol", rtol), ("atol", atol), ("dtol", dtol), ("max_it", max_it)):
            if v >= 0:
                setattr(self.opts, name, type(getattr(self.opts, name))(v))

    def AssembleConductivityMatrix(self, xPhys, kmin, kmax, penal):
        _chk(self.L.tp_conduction_assemble(self.handle, _ptr(xPhys), kmin, kmax, penal), "tp_conduction_assemble")

    def MatMult(self, u, y=None):
        y = torch.zeros_like(u) if y is None else y
        _chk(self.L.tp_conduction_apply(self.handle, _ptr(u), _ptr(y)), "tp_conduction_apply")
        return y

    def MatMultDot(self, u, y=None, read=True):
        """the product as CG forms it, with its fused dot product -> (y, u . y); read=False: (y, None), the host does not wait"""
        y = torch.zeros_like(u) if y is None else y
        d = C.c_double()
        _chk(self.L.tp_conduction_apply_dot(self.handle, _ptr(u), _ptr(y), C.byref(d) if read else None), "tp_conduction_apply_dot")
        return y, (d.value if read else None)

    def KSPSolve(self, hist_cap=0, rhs=None):
        """solve on the last assembly, warm-started from self.T (rhs: another right-hand side than self.RHS)"""
        import time
        import numpy as np
        its, rn, bn = C.c_int(), C.c_double(), C.c_double()
        hist = np.zeros(max(hist_cap, 1))
        t0 = time.perf_counter()   # the solve ends with a host read of ||r||: wall time == device time
        rc = self.L.tp_conduction_solve(self.handle, _ptr(self.RHS if rhs is None else rhs), _ptr(self.T), C.byref(its), C.byref(rn),
                                        C.byref(bn), hist.ctypes.data if hist_cap else None, hist_cap)
        self.last_solve_s = time.perf_counter() - t0
        self.last_its, self.last_rnorm, self.last_bnorm = its.value, rn.value, bn.value
        self.last_hist = hist[: min(its.value + 1, hist_cap)] if hist_cap else None
        _chk(rc, "tp_conduction_solve")
        return its.value

    def SolveState(self, xPhys, kmin, kmax, penal, hist_cap=0):
        self.AssembleConductivityMatrix(xPhys, kmin, kmax, penal)
        return self.KSPSolve(hist_cap)

    def SolveAdjoint(self, rhs, mu):
        """A mu = N rhs on the last assembly, warm-started from mu (the caller's, as rhs) -> iterations.  The figures go to
        adjoint_its / adjoint_rnorm / adjoint_bnorm; last_its and the records of the state solve stay as they are."""
        its, rn, bn = C.c_int(), C.c_double(), C.c_double()
        rc = self.L.tp_conduction_solve(self.handle, _ptr(rhs), _ptr(mu), C.byref(its), C.byref(rn), C.byref(bn), None, 0)
        self.adjoint_its, self.adjoint_rnorm, self.adjoint_bnorm = its.value, rn.value, bn.value
        _chk(rc, "tp_conduction_solve (adjoint)")
        return its.value

    def Response(self, T_list, V_list, w, xPhys, kmin, kmax, penal, volfrac, dfdx=None, dgdx=None, sums=True):
        """tp_conduction_response: fx = sum_l w_l f_l with f_l = sum_e k_e v_l^T KT t_l, gx, dfdx, dgdx for all cases in one pass
        over the elements -> (fx, gx, f_case).  V_list None, or an entry None: V_l = T_l (thermal compliance); w None: all
        weights 1.  sums=False: nothing is reduced and the host does not wait -> (None, None, None)."""
        n = len(T_list)
        Ta = (C.c_void_p * max(n, 1))(*[_ptr(t) for t in T_list])
        Va = None if V_list is None else (C.c_void_p * max(n, 1))(*[_ptr(v) for v in V_list])
        wa = None if w is None else (C.c_double * max(n, 1))(*[float(v) for v in w])
        fx, gx, fc = C.c_double(), C.c_double(), (C.c_double * max(n, 1))()
        _chk(self.L.tp_conduction_response(self.handle, n, Ta, Va, wa, _ptr(xPhys), kmin, kmax, penal, volfrac,
                                           fc if sums else None, C.byref(fx) if sums else None, C.byref(gx) if sums else None,
                                           _ptr(dfdx), _ptr(dgdx)), "tp_conduction_response")
        return (fx.value, gx.value, list(fc)[:n]) if sums else (None, None, None)

    def ComputeObjectiveConstraintsSensitivities(self, dfdx, dgdx, xPhys, kmin, kmax, penal, volfrac, hist_cap=0):
        """solve, then the thermal compliance fx = T^T K T, the volume constraint gx and their sensitivities -> (fx, gx)"""
        self.SolveState(xPhys, kmin, kmax, penal, hist_cap)
        fx, gx, _ = self.Response([self.T], None, None, xPhys, kmin, kmax, penal, volfrac, dfdx, dgdx)
        return fx, gx


class Filter(_Handle, _Levels):
    """Filter (Filter.h:34-92): filterType 0 sensitivity, 1 density, 2 PDE."""
    _destroy, _prefix, _dof = "tp_filter_destroy", "tp_pdefilter", 1

    def __init__(self, grid, filterType, rmin, pde_opts=None):
        self.grid, self.L = grid, grid.L
        self.filterType = filterType
        self.handle = C.c_void_p()
        po = pde_opts.c_struct() if pde_opts else None
        _chk(self.L.tp_filter_create(C.byref(self.handle), grid.handle, filterType, rmin,
                                     C.byref(po) if po else None), "tp_filter_create")
        grid._adopt(self)

    @property
    def ElemConn(self):
        return self.L.tp_filter_stencil_width(self.handle)

    def last_kernel(self):
        """cone-filter kernel of the last convolution: 1 tiled, 2 several outputs along z, 3 wide, 4 streamed ring, 5 generic"""
        return self.L.tp_filter_last_kernel(self.handle)

    def Hs(self):
        hs = self.grid.elem_vec()
        _chk(self.L.tp_filter_get_hs(self.handle, _ptr(hs)), "tp_filter_get_hs")
        return hs

    def KF(self):
        """PDE filter: the 8x8 Helmholtz element matrix (PDEFilter.cc:472-576), numpy"""
        import numpy as np
        kf = np.zeros(64)
        _chk(self.L.tp_filter_get_kf(self.handle, kf.ctypes.data_as(C.c_void_p)), "tp_filter_get_kf")
        return kf

    def FilterProject(self, x, xTilde, xPhys, projectionFilter=False, beta=0.1, eta=0.0):
        """Filter.cc:60-117"""
        _chk(self.L.tp_filter_project(self.handle, _ptr(x), _ptr(xTilde), _ptr(xPhys), int(projectionFilter), beta,
                                      eta), "tp_filter_project")

    def Gradients(self, x, xTilde, dfdx, dgdx, projectionFilter=False, beta=0.1, eta=0.0):
        """Filter.cc:120-204; dgdx is a list of tensors (m constraints)"""
        arr = (C.c_void_p * max(len(dgdx), 1))(*[_ptr(g) for g in dgdx])
        _chk(self.L.tp_filter_gradients(self.handle, _ptr(x), _ptr(xTilde), _ptr(dfdx), len(dgdx), arr,
                                        int(projectionFilter), beta, eta), "tp_filter_gradients")

    def GradientsFromTilde(self, x, rows):
        """every tensor of the list becomes (d xTilde / d x)^T times itself, in place: the filter's transpose alone, for
        gradients taken with respect to xTilde (LengthScale); no projection chain.  Filter type 0: TP_ERR_ARG"""
        arr = (C.c_void_p * max(len(rows), 1))(*[_ptr(r) for r in rows])
        _chk(self.L.tp_filter_gradients_from_tilde(self.handle, _ptr(x), len(rows), arr), "tp_filter_gradients_from_tilde")
        return rows

    def MultH(self, x, y):
        """y = H x with the cone weights (MatMult(H, ...), Filter.cc:68, :173-189), no division by Hs"""
        _chk(self.L.tp_filter_mult_h(self.handle, _ptr(x), _ptr(y)), "tp_filter_mult_h")

    def PDEApply(self, u, y):
        """y = K_f u, the nodal Helmholtz operator of the PDE filter applied matrix-free (PDEFilter.cc:251-264 assembles it)"""
        _chk(self.L.tp_pdefilter_apply(self.handle, _ptr(u), _ptr(y)), "tp_pdefilter_apply")

    def elem_to_node(self, x):
        """PDE filter: T x, element -> node (the eighth of every adjacent element; PDEFilter.cc:198-202 without the volume)"""
        y = self.grid.node_vec(1)
        _chk(self.L.tp_pdefilter_elem_to_node(self.handle, _ptr(x), _ptr(y)), "tp_pdefilter_elem_to_node")
        return y

    def node_to_elem(self, u):
        """PDE filter: T^T u, node -> element (PDEFilter.cc:210); refreshes the ghost planes of u"""
        x = self.grid.elem_vec()
        _chk(self.L.tp_pdefilter_node_to_elem(self.handle, _ptr(u), _ptr(x)), "tp_pdefilter_node_to_elem")
        return x

    # (type 2: the scalar hierarchy level by level is _Levels)

    def GetMND(self, x):
        v = C.c_double()
        _chk(self.L.tp_filter_mnd(self.handle, _ptr(x), C.byref(v)), "tp_filter_mnd")
        return v.value

    def last_pde_solve(self):
        its, rn = C.c_int(), C.c_double()
        self.L.tp_filter_last_pde_its(self.handle, C.byref(its), C.byref(rn))
        return its.value, rn.value


class LocalVolume(_Handle):
    """Local volume constraint (tp_localvol): the mean density in a ball of radius R around every element, its p-norm
    held below alpha as one constraint g = pn / alpha - 1.  Independent of the Filter and of rmin."""
    _destroy = "tp_localvol_destroy"

    def __init__(self, grid, R):
        self.grid, self.L = grid, grid.L
        self.handle = C.c_void_p()
        _chk(self.L.tp_localvol_create(C.byref(self.handle), grid.handle, float(R)), "tp_localvol_create")
        grid._adopt(self)

    @property
    def stencil_width(self):
        return self.L.tp_localvol_stencil_width(self.handle)

    def last_kernel(self):
        """kernel of the last ball sum, the codes of Filter.last_kernel"""
        return self.L.tp_localvol_last_kernel(self.handle)

    def count(self):
        """elements in every own element's ball (truncated at the domain boundary)"""
        cnt = self.grid.elem_vec()
        _chk(self.L.tp_localvol_get_count(self.handle, _ptr(cnt)), "tp_localvol_get_count")
        return cnt

    def Mean(self, xPhys, out):
        """out = ball mean of xPhys; nothing is reduced and the host does not wait"""
        _chk(self.L.tp_localvol_mean(self.handle, _ptr(xPhys), _ptr(out)), "tp_localvol_mean")
        return out

    def Constraint(self, xPhys, alpha, p=16.0, dgdx=None, rhobar=None):
        """(g, pn, rhobar_max) with g = pn / alpha - 1; dgdx receives dg/dxPhys, rhobar the ball means, where given"""
        g, pn, mx = C.c_double(), C.c_double(), C.c_double()
        _chk(self.L.tp_localvol_constraint(self.handle, _ptr(xPhys), alpha, p, C.byref(g), C.byref(pn), C.byref(mx),
                                           _ptr(rhobar), _ptr(dgdx)), "tp_localvol_constraint")
        return g.value, pn.value, mx.value


class LengthScale(_Handle):
    """Minimum length scale by geometric constraints (tp_lengthscale): one constraint for the solid and one for the void phase
    on the filtered field xTilde and the projected field xPhys, g = S / (n eps) - 1 with S = sum_e a_e exp(-c G_e) m_e^2."""
    _destroy = "tp_lengthscale_destroy"
    KINDS = {"solid": 1, "void": 2, "both": 3}

    def __init__(self, grid):
        self.grid, self.L = grid, grid.L
        self.handle = C.c_void_p()
        _chk(self.L.tp_lengthscale_create(C.byref(self.handle), grid.handle), "tp_lengthscale_create")
        grid._adopt(self)

    def Constraints(self, xTilde, xPhys, c, eta_s=0.75, eta_v=0.25, eps=1e-2, kinds="both", projectionFilter=False, beta=0.1,
                    eta=0.0, dg_solid=None, dg_void=None):
        """-> dict(g_solid, g_void, S_solid, S_void), None for a kind that was not asked for; dg_solid / dg_void receive
        dg / dxTilde (the projection's derivative inside: they go back through Filter.GradientsFromTilde), where given.
        projectionFilter, beta, eta: what FilterProject was called with"""
        if kinds not in self.KINDS:
            raise ValueError("kinds must be one of %s, got %r" % (", ".join(sorted(self.KINDS)), kinds))
        k = self.KINDS[kinds]
        g, S = (C.c_double * 2)(), (C.c_double * 2)()
        _chk(self.L.tp_lengthscale_constraints(self.handle, _ptr(xTilde), _ptr(xPhys), int(projectionFilter), beta, eta, c, eta_s,
                                               eta_v, eps, k, g, S, _ptr(dg_solid), _ptr(dg_void)), "tp_lengthscale_constraints")
        return dict(g_solid=g[0] if k & 1 else None, g_void=g[1] if k & 2 else None,
                    S_solid=S[0] if k & 1 else None, S_void=S[1] if k & 2 else None)

    def Terms(self, solid=True, void=True):
        """(T_solid, T_void) of the last call, own elements; None for one that was not asked for"""
        ts = self.grid.elem_vec() if solid else None
        tv = self.grid.elem_vec() if void else None
        _chk(self.L.tp_lengthscale_get_terms(self.handle, _ptr(ts), _ptr(tv)), "tp_lengthscale_get_terms")
        return ts, tv


def passive_labels(nxyz, xc, shapes):
    """Global label array (numpy uint8, natural order: x fastest, then y, then z; 0 active, 1 void, 2 solid) of a box of
    nxyz NODES spanning xc = (x0, x1, y0, y1, z0, z1) from a list of shapes in physical coordinates:
        ("solid" | "void", "box", (x0, x1, y0, y1, z0, z1))
        (kind, "sphere", (cx, cy, cz, r))
        (kind, "cylinder", (axis, c1, c2, r))     axis 0 / 1 / 2 or "x" / "y" / "z"; infinite along it, (c1, c2) the centre in
                                                  the two other coordinates in ascending axis order
    An element belongs to a shape when its centre xc0_a + (i_a + 0.5) h_a lies inside or on the boundary; later shapes override
    earlier ones.  Host-side set-up, runs once."""
    import numpy as np
    ne = [int(n) - 1 for n in nxyz]
    if len(ne) != 3 or min(ne) < 1 or len(xc) != 6:
        raise ValueError("passive_labels: need three node counts >= 2 and xc = (x0, x1, y0, y1, z0, z1)")
    c = []
    for a in range(3):
        lo, hi = float(xc[2 * a]), float(xc[2 * a + 1])
        c.append(lo + (np.arange(ne[a]) + 0.5) * ((hi - lo) / ne[a]))
    Z, Y, X = np.meshgrid(c[2], c[1], c[0], indexing="ij")
    P = (X, Y, Z)
    lab = np.zeros((ne[2], ne[1], ne[0]), dtype=np.uint8)
    for shape in shapes:
        try:
            kind, form, num = shape
            num = tuple(num)
        except (TypeError, ValueError):
            raise ValueError("passive_labels: a shape is (kind, form, numbers), got %r" % (shape,))
        if kind not in ("void", "solid"):
            raise ValueError("passive_labels: kind must be 'solid' or 'void', got %r" % (kind,))
        if form == "box" and len(num) == 6:
            b = [float(v) for v in num]
            inside = np.ones(lab.shape, dtype=bool)
            for a in range(3):
                inside &= (P[a] >= b[2 * a]) & (P[a] <= b[2 * a + 1])
        elif form == "sphere" and len(num) == 4:
            cx, cy, cz, r = (float(v) for v in num)
            inside = (X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2 <= r * r
        elif form == "cylinder" and len(num) == 4:
            axis = {"x": 0, "y": 1, "z": 2}.get(num[0], num[0])
            if axis not in (0, 1, 2):
                raise ValueError("passive_labels: cylinder axis must be 0, 1, 2 or 'x', 'y', 'z', got %r" % (num[0],))
            u, v = [P[a] for a in range(3) if a != axis]
            c1, c2, r = (float(t) for t in num[1:])
            inside = (u - c1) ** 2 + (v - c2) ** 2 <= r * r
        else:
            raise ValueError("passive_labels: box (6 numbers), sphere (4) or cylinder (axis and 3), got %r" % (shape,))
        lab[inside] = 1 if kind == "void" else 2
    return lab.reshape(-1)


class Passive(_Handle):
    """Passive regions (tp_passive): labels per own element (0 active, 1 void, 2 solid) and the four kernels between the full
    fields the filter and the physics see and the packed vectors of the active elements the optimiser sees.  Every call takes a
    list of 1 to MAXVEC tensors and handles all of them in one launch."""
    _destroy = "tp_passive_destroy"
    MAXVEC = _lib.PASSIVE_MAXVEC

    def __init__(self, grid, labels_own):
        import numpy as np
        self.grid, self.L = grid, grid.L
        lab = np.ascontiguousarray(np.asarray(labels_own), dtype=np.uint8)
        if lab.ndim != 1 or lab.size != grid.n_own_elems:
            raise ValueError("Passive: need %d labels (own elements), got an array of shape %r" % (grid.n_own_elems, lab.shape))
        self.handle = C.c_void_p()
        _chk(self.L.tp_passive_create(C.byref(self.handle), grid.handle, lab.ctypes.data), "tp_passive_create")
        grid._adopt(self)
        self.n_active, self.n_void, self.n_solid = self.counts()

    def counts(self):
        """(n_active, n_void, n_solid) of the own elements"""
        a, v, s = C.c_long(), C.c_long(), C.c_long()
        _chk(self.L.tp_passive_counts(self.handle, C.byref(a), C.byref(v), C.byref(s)), "tp_passive_counts")
        return a.value, v.value, s.value

    def packed_vec(self, value=0.0):
        return torch.full((self.n_active,), value, dtype=torch.float64, device=self.grid.device)

    def _arr(self, vecs, numel):
        for t in vecs:
            assert t.numel() == numel, "Passive: a vector of %d entries where %d are needed" % (t.numel(), numel)
        return (C.c_void_p * max(len(vecs), 1))(*[_ptr(t) for t in vecs])

    def _nothing_active(self, full, packed):
        """no active element: the packed tensors are empty and have no address to hand to the library, which would launch
        nothing for them; the count and the lengths are checked as the library and _arr check them"""
        if self.n_active:
            return False
        if not 1 <= len(full) <= self.MAXVEC:
            raise TopOptError(1, "tp_passive_gather / tp_passive_scatter")
        assert all(t.numel() == 0 for t in packed) and all(t.numel() == self.grid.n_own_elems for t in full)
        return True

    def Impose(self, vecs, v_void, v_solid):
        """passive entries of every full tensor of the list <- v_void / v_solid by label; active entries stay"""
        _chk(self.L.tp_passive_impose(self.handle, len(vecs), self._arr(vecs, self.grid.n_own_elems), float(v_void), float(v_solid)),
             "tp_passive_impose")
        return vecs

    def Zero(self, rows):
        """passive entries of every full tensor of the list <- +0.0; active entries stay"""
        _chk(self.L.tp_passive_zero(self.handle, len(rows), self._arr(rows, self.grid.n_own_elems)), "tp_passive_zero")
        return rows

    def Gather(self, full, packed):
        """packed[v] <- the active entries of full[v], ascending element order"""
        if len(full) != len(packed):
            raise ValueError("Passive.Gather: %d full and %d packed vectors" % (len(full), len(packed)))
        if self._nothing_active(full, packed):
            return packed
        _chk(self.L.tp_passive_gather(self.handle, len(full), self._arr(full, self.grid.n_own_elems),
                                      self._arr(packed, self.n_active)), "tp_passive_gather")
        return packed

    def Scatter(self, packed, full):
        """the active entries of full[v] <- packed[v]; passive entries stay"""
        if len(full) != len(packed):
            raise ValueError("Passive.Scatter: %d packed and %d full vectors" % (len(packed), len(full)))
        if self._nothing_active(full, packed):
            return full
        _chk(self.L.tp_passive_scatter(self.handle, len(full), self._arr(packed, self.n_active),
                                       self._arr(full, self.grid.n_own_elems)), "tp_passive_scatter")
        return full


LINK_MODES = {"none": 0, "mirror": 1, "repeat": 2, "extrude": 3}


def parse_link(spec, ne=None):
    """-> (modes, cells), two 3-tuples for tp_link_create (mode 0 none, 1 mirror, 2 repeat, 3 extrude; cells 0 but for repeat).
    spec: a dict {"x": "mirror", "y": ("repeat", 4), "z": "extrude"}, or strings "x:mirror", "y:repeat:4", "z:extrude" -- one, or a
    list of them.  Axes left out are not linked.  ne: the element counts (x, y, z) the cell counts must divide (None: not checked).
    ValueError for an axis given twice, an unknown axis or mode, a cell count below 2 or one that does not divide its axis."""
    items = []
    if isinstance(spec, dict):
        for axis, how in spec.items():
            if isinstance(how, str):
                items.append((axis,) + tuple(how.split(":")))
            elif isinstance(how, (tuple, list)) and how:
                items.append((axis,) + tuple(how))
            else:
                raise ValueError("link: %r: need a mode name or (\"repeat\", cells), got %r" % (axis, how))
    else:
        if isinstance(spec, str):
            spec = [spec]
        if not isinstance(spec, (list, tuple)):
            raise ValueError("link: need a dict or strings AXIS:MODE[:CELLS], got %r" % (spec,))
        for s in spec:
            if not isinstance(s, str):
                raise ValueError("link: need strings AXIS:MODE[:CELLS], got %r" % (s,))
            items.append(tuple(s.split(":")))
    modes, cells, seen = [0, 0, 0], [0, 0, 0], set()
    for item in items:
        if len(item) < 2 or item[0] not in ("x", "y", "z"):
            raise ValueError("link: need AXIS:MODE[:CELLS] with AXIS x, y or z, got %r" % (":".join(map(str, item)),))
        a, mode = "xyz".index(item[0]), item[1]
        if a in seen:
            raise ValueError("link: axis %s is given twice" % item[0])
        seen.add(a)
        if mode not in LINK_MODES:
            raise ValueError("link: unknown mode %r (the modes are none, mirror, repeat:CELLS, extrude)" % (mode,))
        if len(item) != (3 if mode == "repeat" else 2):
            raise ValueError("link: %s takes %s, got %r" % (mode, "a cell count" if mode == "repeat" else "no argument", ":".join(map(str, item))))
        modes[a] = LINK_MODES[mode]
        if mode == "repeat":
            c = item[2]
            if isinstance(c, bool) or (not isinstance(c, (int, str))) or (isinstance(c, str) and not c.isdigit()):
                raise ValueError("link: repeat needs a whole number of cells, got %r" % (c,))
            c = int(c)
            if c < 2:
                raise ValueError("link: repeat needs at least 2 cells, got %d" % c)
            if ne is not None and ne[a] % c != 0:
                raise ValueError("link: %d cells do not divide the %d elements along %s" % (c, ne[a], item[0]))
            cells[a] = c
    return tuple(modes), tuple(cells)


class Link(_Handle):
    """Design-variable linking (tp_link): per axis none, mirror, repeat:c or extrude, and the three maps between the
    reduced design the optimiser sees (the box nr_x x nr_y x nr_z, x fastest) and the full fields of the filter and the physics.
    Every call takes lists of 1 to MAXVEC tensors and handles all of them in one launch.  Fold's sum has one fixed order (ascending
    element order, the first member first), so its bits do not depend on the kernel form or the run."""
    _destroy = "tp_link_destroy"
    MAXVEC = _lib.LINK_MAXVEC

    def __init__(self, grid, spec):
        self.grid, self.L = grid, grid.L
        part = grid.part
        self.modes, self.cells = parse_link(spec, (part.ex, part.ey, part.ez_own))
        self.handle = C.c_void_p()
        _chk(self.L.tp_link_create(C.byref(self.handle), grid.handle, (C.c_int * 3)(*self.modes), (C.c_int * 3)(*self.cells)),
             "tp_link_create")
        grid._adopt(self)
        self.n_reduced, self.nr = self.counts()

    def counts(self):
        """(own reduced variables, (nr_x, nr_y, nr_z))"""
        n, nr = C.c_long(), (C.c_long * 3)()
        _chk(self.L.tp_link_counts(self.handle, C.byref(n), nr), "tp_link_counts")
        return n.value, tuple(nr)

    def reduced_vec(self, value=0.0):
        return torch.full((self.n_reduced,), value, dtype=torch.float64, device=self.grid.device)

    def set_form(self, form):
        """fold's kernel: 0 the measured rule, 1 one reduced variable per thread, 2 x rows through LDS where that applies"""
        _chk(self.L.tp_link_set_form(self.handle, int(form)), "tp_link_set_form")

    def last_form(self):
        return self.L.tp_link_last_form(self.handle)

    def _call(self, fn, name, src, n_src, dst, n_dst):
        if len(src) != len(dst):
            raise ValueError("Link.%s: %d source and %d destination vectors" % (name, len(src), len(dst)))
        for t, n in [(t, n_src) for t in src] + [(t, n_dst) for t in dst]:
            assert t.numel() == n, "Link: a vector of %d entries where %d are needed" % (t.numel(), n)
        arr = lambda vecs: (C.c_void_p * max(len(vecs), 1))(*[_ptr(t) for t in vecs])
        _chk(fn(self.handle, len(src), arr(src), arr(dst)), "tp_link_" + name.lower())
        return dst

    def Expand(self, reds, fulls):
        """fulls[v][e] <- reds[v][r(e)]"""
        return self._call(self.L.tp_link_expand, "Expand", reds, self.n_reduced, fulls, self.grid.n_own_elems)

    def Fold(self, fulls, reds):
        """reds[v][j] <- the sum of fulls[v] over the orbit of j, in ascending element order"""
        return self._call(self.L.tp_link_fold, "Fold", fulls, self.grid.n_own_elems, reds, self.n_reduced)

    def Pick(self, fulls, reds):
        """reds[v][j] <- fulls[v] at the first member of the orbit of j"""
        return self._call(self.L.tp_link_pick, "Pick", fulls, self.grid.n_own_elems, reds, self.n_reduced)


class Robust:
    """Robust three-field formulation (tp_robust_project / tp_robust_chain): one filtered field projected at up to MAXPROJ
    thresholds with one beta in one launch -- the eroded, nominal and dilated designs -- and the projections' derivatives put on
    up to MAXROWS gradient rows in one launch.  Holds no device object of its own."""
    MAXPROJ, MAXROWS = _lib.ROBUST_MAXPROJ, _lib.ROBUST_MAXROWS

    def __init__(self, grid):
        self.grid, self.L = grid, grid.L

    def _vecs(self, vecs):
        n = self.grid.n_own_elems
        for t in vecs:
            assert t.numel() == n, "Robust: a vector of %d entries where %d are needed" % (t.numel(), n)
        return (C.c_void_p * max(len(vecs), 1))(*[_ptr(t) for t in vecs])

    def Project(self, xTilde, beta, etas, outs, passive=None, sums=True):
        """outs[k] <- H(xTilde; beta, etas[k]), the bits of Filter.FilterProject's projection at that threshold; with a Passive
        the void elements receive 0.0 and the solid ones 1.0 in every field.  sums=True: -> the list of the fields' sums as
        stored, over all ranks (the host waits); sums=False: -> None, nothing is reduced"""
        if len(etas) != len(outs):
            raise ValueError("Robust.Project: %d thresholds and %d fields" % (len(etas), len(outs)))
        assert xTilde.numel() == self.grid.n_own_elems
        k = len(outs)
        eta = (C.c_double * max(k, 1))(*[float(e) for e in etas])
        s = (C.c_double * max(k, 1))() if sums else None
        _chk(self.L.tp_robust_project(self.grid.handle, _ptr(xTilde), float(beta), k, eta, self._vecs(outs),
                                      passive.handle if passive is not None else None, s), "tp_robust_project")
        return [s[i] for i in range(k)] if sums else None

    def Chain(self, xTilde, beta, rows, etas_of_rows, passive=None):
        """rows[r] *= dH/dxTilde(xTilde; beta, etas_of_rows[r]) in place, Filter.Gradients' projection factor; at most MAXPROJ
        distinct thresholds.  With a Passive the passive entries of every row become +0.0"""
        if len(etas_of_rows) != len(rows):
            raise ValueError("Robust.Chain: %d thresholds and %d rows" % (len(etas_of_rows), len(rows)))
        assert xTilde.numel() == self.grid.n_own_elems
        k = len(rows)
        eta = (C.c_double * max(k, 1))(*[float(e) for e in etas_of_rows])
        _chk(self.L.tp_robust_chain(self.grid.handle, _ptr(xTilde), float(beta), k, self._vecs(rows), eta,
                                    passive.handle if passive is not None else None), "tp_robust_chain")
        return rows


class Overhang(_Handle):
    """Overhang (self-support) filter (tp_overhang): the printed density of a part built layer by layer along `build`
    ("+z", "-z", "+y", "-y"; the baseplate lies at the low end for +), and the transpose of its Jacobian."""
    _destroy = "tp_overhang_destroy"
    BUILDS = {"+y": (1, 1), "-y": (1, -1), "+z": (2, 1), "-z": (2, -1)}

    def __init__(self, grid, build="+z"):
        if build not in self.BUILDS:
            raise ValueError("build must be one of %s, got %r" % (", ".join(sorted(self.BUILDS)), build))
        self.grid, self.L, self.build = grid, grid.L, build
        self.handle = C.c_void_p()
        _chk(self.L.tp_overhang_create(C.byref(self.handle), grid.handle, *self.BUILDS[build]), "tp_overhang_create")
        grid._adopt(self)

    def params(self, P=40.0, eps=1e-4, xi0=0.5):
        _chk(self.L.tp_overhang_set_params(self.handle, P, eps, xi0), "tp_overhang_set_params")

    def Forward(self, x, out):
        """out = printed density of x (out must not be x); leaves the coefficients of the transpose in the handle"""
        _chk(self.L.tp_overhang_forward(self.handle, _ptr(x), _ptr(out)), "tp_overhang_forward")
        return out

    def Adjoint(self, vecs):
        """every tensor of the list (1 to 8) becomes J^T times itself, in place, in one sweep"""
        ptrs = (C.c_void_p * len(vecs))(*[_ptr(v) for v in vecs])
        _chk(self.L.tp_overhang_adjoint(self.handle, len(vecs), ptrs), "tp_overhang_adjoint")
        return vecs

    def last_chunk(self):
        """layers per launch of the last sweep (TP_OVERHANG_CHUNK)"""
        return self.L.tp_overhang_last_chunk(self.handle)

    def Coefficients(self):
        """(a, w, p) of the last Forward, own elements: copies of what the transpose reads"""
        a, w, p = (self.grid.elem_vec() for _ in range(3))
        _chk(self.L.tp_overhang_get_coefficients(self.handle, _ptr(a), _ptr(w), _ptr(p)), "tp_overhang_get_coefficients")
        return a, w, p


class Casting(_Handle):
    """Casting (draw-direction) filter (tp_casting): the density of a part that leaves its mould along `draw` without an
    undercut or an enclosed cavity, and the transpose of its Jacobian.  `draw`: "+x", "-x", "+y", "-y", "+z", "-z" -- a
    one-sided mould, the part sitting on a base at the low end for + -- or "x:K", "y:K", "z:K", a two-sided mould whose plane
    parting surface lies between the element layers K - 1 and K (global)."""
    _destroy = "tp_casting_destroy"
    AXES = {"x": 0, "y": 1, "z": 2}

    @classmethod
    def parse(cls, draw, ne=None):
        """-> (axis, parting) of a draw string; parting is None for "-a" while the element counts `ne` are not given.
        ValueError for anything else, and with `ne` for a K outside 1 .. n - 1"""
        ok = isinstance(draw, str) and len(draw) >= 2
        if ok and draw[0] in "+-" and len(draw) == 2 and draw[1] in cls.AXES:
            axis = cls.AXES[draw[1]]
            return axis, (0 if draw[0] == "+" else (None if ne is None else ne[axis]))
        if ok and draw[0] in cls.AXES and draw[1] == ":" and draw[2:].isdigit():
            axis, k = cls.AXES[draw[0]], int(draw[2:])
            if k >= 1 and (ne is None or k <= ne[axis] - 1):
                return axis, k
        raise ValueError('draw must be "+a" or "-a" with a in x, y, z, or "a:K" with 1 <= K <= n_a - 1, got %r' % (draw,))

    def __init__(self, grid, draw="+z"):
        p = grid.part
        self.axis, self.parting = self.parse(draw, (p.ex, p.ey, p.ez))
        self.grid, self.L, self.draw = grid, grid.L, draw
        self.handle = C.c_void_p()
        _chk(self.L.tp_casting_create(C.byref(self.handle), grid.handle, self.axis, self.parting), "tp_casting_create")
        grid._adopt(self)

    def params(self, eps=1e-6):
        _chk(self.L.tp_casting_set_params(self.handle, eps), "tp_casting_set_params")

    def Forward(self, x, out):
        """out = cast density of x (out must not be x); leaves the coefficients of the transpose in the handle"""
        _chk(self.L.tp_casting_forward(self.handle, _ptr(x), _ptr(out)), "tp_casting_forward")
        return out

    def Adjoint(self, vecs):
        """every tensor of the list (1 to 8) becomes J^T times itself, in place, in one sweep"""
        ptrs = (C.c_void_p * len(vecs))(*[_ptr(v) for v in vecs])
        _chk(self.L.tp_casting_adjoint(self.handle, len(vecs), ptrs), "tp_casting_adjoint")
        return vecs

    def last_form(self):
        """kernel form of the last sweep: 1 walk, 2 LDS-staged x draw, 3 walk on x lines (TP_CASTING_XFORM=0)"""
        return self.L.tp_casting_last_form(self.handle)

    def Q(self):
        """q of the last Forward, own elements: a copy of what the transpose reads"""
        q = self.grid.elem_vec()
        _chk(self.L.tp_casting_get_q(self.handle, _ptr(q)), "tp_casting_get_q")
        return q


class MMA(_Handle):
    """MMA (MMA.h:29-140) on the device: the design vectors stay in HBM."""
    _destroy = "tp_mma_destroy"

    def __init__(self, grid, x, m=1, n_global=None, a=None, c=None, d=None):
        """a, c, d: the subproblem's penalty numbers of the a/c/d constructors (MMA.cc:195-242), each a sequence of m
        or one number for all j; None keeps the defaults a = 0, c = 1000, d = 0"""
        self.grid, self.L, self.m = grid, grid.L, m
        self.handle = C.c_void_p()
        n_loc = x.numel()
        n_glob = n_global if n_global is not None else grid.part.ex * grid.part.ey * grid.part.ez
        _chk(self.L.tp_mma_create(C.byref(self.handle), grid.handle, n_loc, n_glob, m, _ptr(x)), "tp_mma_create")
        grid._adopt(self)
        self.last_inner = 0
        if a is not None or c is not None or d is not None:
            _chk(self.L.tp_mma_set_subproblem(self.handle, self._m_array(a), self._m_array(c), self._m_array(d)),
                 "tp_mma_set_subproblem")

    def _m_array(self, v):
        if v is None:
            return None
        v = [float(v)] * self.m if isinstance(v, (int, float)) else [float(t) for t in v]
        if len(v) != self.m:
            raise ValueError("need %d values, got %d" % (self.m, len(v)))
        return (C.c_double * self.m)(*v)

    def SetOuterMovelimit(self, Xmin, Xmax, movlim, x, xmin, xmax):
        _chk(self.L.tp_mma_set_outer_movelimit(self.handle, Xmin, Xmax, movlim, _ptr(x), _ptr(xmin), _ptr(xmax)),
             "tp_mma_set_outer_movelimit")

    def Update(self, x, dfdx, gx, dgdx, xmin, xmax):
        g = (C.c_double * self.m)(*gx)
        dg = (C.c_void_p * self.m)(*[_ptr(t) for t in dgdx])
        it = C.c_int()
        _chk(self.L.tp_mma_update(self.handle, _ptr(x), _ptr(dfdx), g, dg, _ptr(xmin), _ptr(xmax), C.byref(it)),
             "tp_mma_update")
        self.last_inner = it.value

    def SetAsymptotes(self, init, decrease, increase):
        """MMA::SetAsymptotes (MMA.cc:362-370); from the next Update on"""
        _chk(self.L.tp_mma_set_asymptotes(self.handle, float(init), float(decrease), float(increase)), "tp_mma_set_asymptotes")

    def SetRobustAsymptotesType(self, val):
        """MMA::SetRobustAsymptotesType (MMA.cc:372-384): 0 or 1; any other value leaves type 0 and raises"""
        _chk(self.L.tp_mma_set_robust_asymptotes_type(self.handle, int(val)), "tp_mma_set_robust_asymptotes_type")

    def ConstraintModification(self, conMod):
        """MMA::ConstraintModification (MMA.h:53)"""
        _chk(self.L.tp_mma_constraint_modification(self.handle, 1 if conMod else 0), "tp_mma_constraint_modification")

    def KKTresidual(self, x, dfdx, gx, dgdx, xmin, xmax):
        """MMA::KKTresidual (MMA.cc:428-496) at the multipliers of the last Update: returns (norm2, normInf)"""
        g = (C.c_double * self.m)(*gx)
        dg = (C.c_void_p * self.m)(*[_ptr(t) for t in dgdx])
        n2, ni = C.c_double(), C.c_double()
        _chk(self.L.tp_mma_kkt_residual(self.handle, _ptr(x), _ptr(dfdx), g, dg, _ptr(xmin), _ptr(xmax), C.byref(n2),
                                        C.byref(ni)), "tp_mma_kkt_residual")
        return n2.value, ni.value

    def DesignChange(self, x, xold):
        ch = C.c_double()
        _chk(self.L.tp_mma_design_change(self.handle, _ptr(x), _ptr(xold), C.byref(ch)), "tp_mma_design_change")
        return ch.value

    def Restart(self, xo1, xo2, U, L):
        """MMA::Restart (MMA.cc:319-360): copy the two previous iterates and the asymptotes out"""
        _chk(self.L.tp_mma_restart_get(self.handle, _ptr(xo1), _ptr(xo2), _ptr(U), _ptr(L)), "tp_mma_restart_get")

    def SetRestart(self, k, xo1, xo2, U, L):
        """the restart constructor MMA::MMA(n, m, k, xo1, xo2, U, L, ...) (MMA.cc:22-106)"""
        _chk(self.L.tp_mma_restart_set(self.handle, int(k), _ptr(xo1), _ptr(xo2), _ptr(U), _ptr(L)), "tp_mma_restart_set")

    def state(self):
        lam = (C.c_double * self.m)()
        z, k = C.c_double(), C.c_int()
        self.L.tp_mma_get_state(self.handle, lam, C.byref(z), C.byref(k))
        return list(lam), z.value, k.value
