"""numpy / scipy restatement of the free-vibration formulas (include/topopt_amd.h) and nothing else.

    A = N K(x) N + (I - N),  K = sum_e (Emin + x_e^p (Emax - Emin)) KE        (KE: the oracle's hex8_ke_box)
    M_e = rho0 m(x_e) V_e (M8 (x) I_3),  M8[a,b] = (1/8) prod_axis (2/3 if corners a, b share that coordinate else 1/3)
    B = N M N,  A phi = lambda B phi,  phi^T B phi = 1
    d lambda / dx_e = p x_e^(p-1) (Emax - Emin) phi_e^T KE phi_e - lambda rho0 m'(x_e) V_e phi_e^T (M8 (x) I_3) phi_e
    J = sum_{i < nev} 1 / lambda_i,  dJ/dx = - sum_i lambda_i^-2 d lambda_i / dx
m, m' and the connectivity are those of tests/selfweight_ref.py.  Every function takes the arithmetic as `dtype`: numpy.float64 or
numpy.longdouble (80-bit); the distance between the two is what the kernels' bounds are made of."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests import scipy_check as sc
from tests.selfweight_ref import LD, LX, LY, LZ, dmass, elem_dofs, mass, volume  # noqa: F401


def m8(dtype=LD):
    """8 x 8, corner order of the header"""
    two, one = dtype(2) / dtype(3), dtype(1) / dtype(3)
    M = np.empty((8, 8), dtype=dtype)
    for a in range(8):
        for b in range(8):
            f = dtype(1) / dtype(8)
            for La in (LX, LY, LZ):
                f = f * (two if La[a] == La[b] else one)
            M[a, b] = f
    return M


def me24(dtype=LD):
    return np.kron(m8(dtype), np.eye(3, dtype=dtype))


def coef(x, h, rho0, x_low, dtype=LD):
    """rho0 V_e m(x_e)"""
    if dtype is LD:
        return LD(rho0) * volume(h) * mass(x, x_low)
    return np.float64(rho0) * (np.float64(h[0]) * np.float64(h[1]) * np.float64(h[2])) * _mass64(x, x_low)


def _mass64(x, x_low):
    x = np.asarray(x, dtype=np.float64)
    if x_low == 0:
        return x.copy()
    t = np.minimum(x * (1.0 / x_low), 1.0)
    return np.where(x >= x_low, x, x * ((t * t) * (t * t) * t * (6.0 - 5.0 * t)))


def _dmass64(x, x_low):
    x = np.asarray(x, dtype=np.float64)
    if x_low == 0:
        return np.ones_like(x)
    t = np.minimum(x * (1.0 / x_low), 1.0)
    return np.where(x >= x_low, 1.0, (t * t) * (t * t) * t * (36.0 - 35.0 * t))


mass64, dmass64 = _mass64, _dmass64        # (the names for other helper modules: tests/response_rowwise.py)


def mass_apply(x, dofs, nnode, h, rho0, x_low, N, u, dtype=LD):
    """y = N M N u, element by element"""
    Nv = np.asarray(N, dtype=dtype)
    ue = (Nv * np.asarray(u, dtype=dtype))[dofs]
    fe = coef(x, h, rho0, x_low, dtype)[:, None] * (ue @ me24(dtype).T)
    y = np.zeros(3 * nnode, dtype=dtype)
    np.add.at(y, dofs, fe)
    return Nv * y


def quad_form(dofs, N, v, dtype=LD):
    """(N v)_e^T (M8 (x) I_3) (N v)_e [nel]"""
    ve = (np.asarray(N, dtype=dtype) * np.asarray(v, dtype=dtype))[dofs]
    return np.einsum("er,rc,ec->e", ve, me24(dtype), ve)


def mass_sens(x, dofs, h, rho0, x_low, N, V, w, scale, dtype=LD):
    """scale m'(x_e) rho0 V_e sum_l w_l (N v_l)_e^T (M8 (x) I_3) (N v_l)_e [nel]"""
    if dtype is LD:
        pre = dtype(rho0) * volume(h) * dmass(x, x_low)
    else:
        pre = np.float64(rho0) * (np.float64(h[0]) * np.float64(h[1]) * np.float64(h[2])) * _dmass64(x, x_low)
    acc = np.zeros(dofs.shape[0], dtype=dtype)
    for wl, v in zip(w, V):
        acc = acc + dtype(wl) * quad_form(dofs, N, v, dtype)
    return dtype(scale) * pre * acc


def cantilever_N(ex, ey, ez):
    N = np.ones((ez + 1, ey + 1, ex + 1, 3))
    N[:, :, 0, :] = 0.0
    return N.reshape(-1)


def assemble_M(ne, h, x, rho0, x_low, N=None):
    """sparse float64 mass matrix; N given: N M N"""
    c = np.asarray(coef(x, h, rho0, x_low, LD), dtype=np.float64)
    M = sc.assemble(ne[0], ne[1], ne[2], np.asarray(me24(LD), dtype=np.float64), E=c)
    if N is not None:
        D = sp.diags(N)
        M = (D @ M @ D).tocsr()
    return M


def assemble_K(ne, KE, x, Emin, Emax, penal, N=None):
    return sc.assemble(ne[0], ne[1], ne[2], KE, E=Emin + np.asarray(x, dtype=np.float64) ** penal * (Emax - Emin), N=N)


class Pencil:
    """A = N K N + I - N and B = N M N of one mesh and design, the free dofs, and the two solvers of the restatement"""

    def __init__(self, ne, h, KE, x, N, Emin=1e-3, Emax=1.0, penal=3.0, rho0=1.0, x_low=0.1):
        self.ne, self.h, self.x, self.N = ne, h, np.asarray(x, dtype=np.float64), np.asarray(N, dtype=np.float64)
        self.KE = np.asarray(KE, dtype=np.float64).reshape(24, 24)
        self.Emin, self.Emax, self.penal, self.rho0, self.x_low = Emin, Emax, penal, rho0, x_low
        self.dofs = elem_dofs(*ne)
        self.nnode = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
        self.A = assemble_K(ne, self.KE, x, Emin, Emax, penal, N=self.N)
        self.B = assemble_M(ne, h, x, rho0, x_low, N=self.N)
        self.free = np.flatnonzero(self.N > 0)

    def eigh(self, k):
        """dense scipy.linalg.eigh on the free dofs -> (lam[k] ascending, Phi[n, k] on all dofs, B-normalised)"""
        f = self.free
        lam, V = scipy.linalg.eigh(self.A[f][:, f].toarray(), self.B[f][:, f].toarray(), subset_by_index=[0, k - 1])
        Phi = np.zeros((3 * self.nnode, k))
        Phi[f] = V
        return lam, Phi

    def subspace(self, nev, guard=2, tol=1e-8, max_iter=60, seed=5):
        """the same subspace iteration with sparse direct solves -> (theta[q], X[n, q], iterations, residuals)"""
        q = nev + guard
        lu = spl.splu(self.A.tocsc())
        X = self.N[:, None] * np.random.default_rng(seed).uniform(-1.0, 1.0, (3 * self.nnode, q))
        for it in range(1, max_iter + 1):
            Y = lu.solve(self.B @ X)
            AY, BY = self.A @ Y, self.B @ Y
            Kt, Mt = Y.T @ AY, Y.T @ BY
            theta, Q = scipy.linalg.eigh(0.5 * (Kt + Kt.T), 0.5 * (Mt + Mt.T))
            X, AX, BX = Y @ Q, AY @ Q, BY @ Q
            res = np.linalg.norm(AX[:, :nev] - BX[:, :nev] * theta[:nev], axis=0) / np.linalg.norm(AX[:, :nev], axis=0)
            if res.max() <= tol:
                break
        return theta, X, it, res

    def apply_ld(self, u):
        """(A u, B u) in 80-bit arithmetic, element by element"""
        Nv, E = self.N.astype(LD), LD(self.Emin) + self.x.astype(LD) ** LD(self.penal) * (LD(self.Emax) - LD(self.Emin))
        ue = (Nv * np.asarray(u, dtype=LD))[self.dofs]
        y = np.zeros(3 * self.nnode, dtype=LD)
        np.add.at(y, self.dofs, E[:, None] * (ue @ self.KE.astype(LD).T))
        return Nv * y + (1 - Nv) * np.asarray(u, dtype=LD), mass_apply(self.x, self.dofs, self.nnode, self.h, self.rho0, self.x_low, self.N, u, LD)

    def refine(self, lam, Phi):
        """the Rayleigh quotients of eigh's vectors in 80-bit arithmetic: an eigenvector off by d gives its eigenvalue to d^2,
        so these carry the 80-bit rounding alone, where eigh's own values carry 2^-53 lambda_max / lambda_1 -> lam (longdouble)"""
        out = []
        for i in range(Phi.shape[1]):
            Au, Bu = self.apply_ld(Phi[:, i])
            u = Phi[:, i].astype(LD)
            out.append((u @ Au) / (u @ Bu))
        return np.array(out, dtype=LD)

    def J(self, nev, lam=None):
        """sum_{i < nev} 1 / lambda_i (longdouble); lam None: eigh's values refined in 80-bit arithmetic"""
        lam = self.refine(*self.eigh(nev)) if lam is None else lam
        return np.sum(1 / np.asarray(lam[:nev], dtype=LD))

    def dlam(self, lam, phi, mass_term=True):
        """d lambda / dx [nel] of one B-normalised mode, 80-bit"""
        xe, p = self.x.astype(LD), LD(self.penal)
        ue = np.asarray(phi, dtype=LD)[self.dofs]
        stiff = p * xe ** (p - 1) * (LD(self.Emax) - LD(self.Emin)) * np.einsum("er,rc,ec->e", ue, self.KE.astype(LD), ue)
        if not mass_term:
            return stiff
        return stiff - mass_sens(self.x, self.dofs, self.h, self.rho0, self.x_low, self.N, [phi], [1.0], lam, LD)

    def dJ(self, lam, Phi, nev, mass_term=True):
        """dJ/dx [nel] from B-normalised modes (any basis of a cluster that lies whole inside the sum)"""
        out = np.zeros(self.dofs.shape[0], dtype=LD)
        for i in range(nev):
            out = out - self.dlam(lam[i], Phi[:, i], mass_term) / LD(lam[i]) ** 2
        return out


def subspace_angle(B, Phi_ref, v):
    """sine of the angle between v and span(Phi_ref) in the B inner product (Phi_ref B-orthonormal)"""
    Bv = B @ v
    c = Phi_ref.T @ Bv
    r = v - Phi_ref @ c
    return float(np.sqrt(max(r @ (B @ r), 0.0) / (v @ Bv)))


# ---- the meshes and designs of the GPU tests (tests/test_gpu_eigen.py, tests/eigen_worker.py); tests/test_eigen_abi.py holds every
# one of them to the conditions the bounds rest on: a gap behind the last mode of the sum, well separated or truly clustered
# modes inside it, and a quarter of the elements on either side of x_low
X_LOW = 0.1


def design_mixed(ne, seed):
    """uniform(0.05, 1) with every third element in the damped range"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.05, 1.0, ne[0] * ne[1] * ne[2])
    x[::3] = rng.uniform(0.01, 0.095, x[::3].size)
    return x


def design_square(ne, seed):
    """the same kind of field with the symmetry of the square section (y -> -y, z -> -z, y <-> z; ey == ez): the bending pair
    stays a double eigenvalue"""
    ex, ey, ez = ne
    assert ey == ez
    rng = np.random.default_rng(seed)
    r = np.where(rng.uniform(0.0, 1.0, (ez, ey, ex)) < 0.4, rng.uniform(0.01, 0.095, (ez, ey, ex)), rng.uniform(0.05, 1.0, (ez, ey, ex)))
    fold = np.minimum(np.arange(ey), ey - 1 - np.arange(ey))
    a, b = np.minimum(fold[:, None], fold[None, :]), np.maximum(fold[:, None], fold[None, :])
    return r[a, b, :].reshape(-1)


KERNEL_MESHES = [((3, 3, 3), (0.25, 0.25, 0.25)), ((5, 2, 7), (0.25, 0.25, 0.25)), ((7, 1, 5), (0.25, 0.25, 0.25)),
                 ((20, 12, 8), (0.05, 0.04, 0.03))]
EIGEN_CASES = {
    "box": dict(ne=(16, 8, 8), h=(0.125, 0.125, 0.1), nev=3, nlvls=3, design=design_mixed, seed=11),
    "cube": dict(ne=(12, 8, 4), h=(0.125, 0.125, 0.125), nev=3, nlvls=3, design=design_mixed, seed=12),
    "square": dict(ne=(8, 4, 4), h=(0.25, 0.25, 0.25), nev=2, nlvls=2, design=design_square, seed=13),
}
SLAB_CASES = {
    "slab2": dict(ne=(16, 8, 8), h=(0.125, 0.125, 0.1), nev=3, nlvls=3, design=design_mixed, seed=11),
    "slab3": dict(ne=(12, 8, 12), h=(0.125, 0.125, 0.125), nev=3, nlvls=3, design=design_mixed, seed=14),
    # (two own layers per rank: on slabs every distributed level keeps two, so this one has a single level)
    "slab3thin": dict(ne=(8, 8, 6), h=(0.125, 0.125, 0.125), nev=3, nlvls=1, design=design_mixed, seed=15),
}
EMIN, EMAX, PENAL, RHO0 = 1e-3, 1.0, 3.0, 1.0
