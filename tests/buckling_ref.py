"""numpy / scipy restatement of the linear-buckling formulas (include/topopt_amd.h) and nothing else.

    A = N K(x) N + (I - N),  K = sum_e (Emin + x_e^p (Emax - Emin)) KE,  A u = N f
    sigma(gp) = C0 B(gp) u_e at the 2 x 2 x 2 Gauss points (weight w = hx hy hz / 8), S its symmetric 3 x 3 tensor
    g_e[a,b] = sum_gp w gradN_a^T S gradN_b,   G_e = Emax x_e^p (g_e (x) I_3)   (no Emin)
    B = -N G N,  B phi = mu A phi,  phi^T A phi = 1,  load factors 1 / mu of the positive mu
    J = (sum_{i < nev} mu_i^P)^(1/P) over the nev largest positive mu,  c_i = (mu_i / J)^(P-1)
    dJ/dx_e = - sum c_i mu_i p x^(p-1) (Emax - Emin) phi_e^T KE phi_e              (stiffness)
              - sum c_i p x^(p-1) Emax phi_e^T (g_e(u_e) (x) I_3) phi_e           (explicit)
              - p x^(p-1) (Emax - Emin) v_e^T KE u_e,  A v = N r,  r = - sum c_i d(phi_i^T G phi_i)/du      (state)
    r_e = - c_i Emax x^p w sum_gp (C0 B(gp))^T s(gp),  s the Voigt vector (s11, s22, s33, 2 s12, 2 s23, 2 s13) of
    s_ij = sum_k d phi_k/dx_i d phi_k/dx_j
Node order, Gauss points and strain rows (xx, yy, zz, xy, yz, zx; engineering shear) are hex8_stiffness_box's.  Every kernel-level
function takes the arithmetic as `dtype`: numpy.float64 or numpy.longdouble (80-bit); the distance between the two is what the
kernels' bounds are made of."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests.selfweight_ref import LD, LX, LY, LZ, elem_dofs  # noqa: F401

SGN = [[-1, 1, 1, -1, -1, 1, 1, -1], [-1, -1, 1, 1, -1, -1, 1, 1], [-1, -1, -1, -1, 1, 1, 1, 1]]
SEL = [[0, -1, -1, 1, -1, 2], [-1, 1, -1, 0, 2, -1], [-1, -1, 2, -1, 1, 0]]   # sel[d][row]: the component whose d-derivative enters the row


def c0(nu, dtype=LD):
    nu = dtype(nu)
    lam, mu = nu / ((1 + nu) * (1 - 2 * nu)), 1 / (2 * (1 + nu))
    C = np.zeros((6, 6), dtype=dtype)
    C[:3, :3] = lam
    for i in range(3):
        C[i, i] = lam + 2 * mu
        C[i + 3, i + 3] = mu
    return C


def tables(h, nu=0.3, dtype=LD):
    """-> gradN [8 gp, 3, 8 nodes], C0 B [8 gp, 6, 24], B [8 gp, 6, 24], w; Gauss points in the order a, b, c over xi, eta, zeta"""
    g = dtype(0.577350269189626)          # the literal of hex8_stiffness_box
    sg = np.array(SGN, dtype=dtype)
    hh = [dtype(v) for v in h]
    gn, Bm = np.zeros((8, 3, 8), dtype=dtype), np.zeros((8, 6, 24), dtype=dtype)
    q = 0
    for a in (-g, g):
        for b in (-g, g):
            for c in (-g, g):
                p = [a, b, c]
                for d in range(3):
                    o1, o2 = (d + 1) % 3, (d + 2) % 3
                    gn[q, d] = sg[d] / 8 * (1 + sg[o1] * p[o1]) * (1 + sg[o2] * p[o2]) * (2 / hh[d])
                for d in range(3):
                    for row in range(6):
                        if SEL[d][row] >= 0:
                            Bm[q, row, SEL[d][row]::3] = gn[q, d]
                q += 1
    C = c0(nu, dtype)
    cb = np.einsum("rk,qkj->qrj", C, Bm)
    return gn, cb, Bm, hh[0] * hh[1] * hh[2] / 8


def ke(h, nu=0.3, dtype=LD):
    gn, cb, Bm, w = tables(h, nu, dtype)
    return w * np.einsum("qri,qrj->ij", Bm, cb)


def stress_tensor(sg):
    """[..., 6] Voigt (xx, yy, zz, xy, yz, zx) -> [..., 3, 3]"""
    S = np.empty(sg.shape[:-1] + (3, 3), dtype=sg.dtype)
    for (i, j), r in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 2): 4, (0, 2): 5}.items():
        S[..., i, j] = S[..., j, i] = sg[..., r]
    return S


def ghat(ue, h, nu=0.3, dtype=LD):
    """g_e [nel, 8, 8] of the element displacements ue [nel, 24]"""
    gn, cb, _, w = tables(h, nu, dtype)
    S = stress_tensor(np.einsum("qrj,ej->eqr", cb, np.asarray(ue, dtype=dtype)))
    return w * np.einsum("qia,eqij,qjb->eab", gn, S, gn)


def modulus(x, Emax, penal, dtype=LD):
    return dtype(Emax) * np.asarray(x, dtype=dtype) ** dtype(penal)


def geom_apply(x, dofs, nnode, h, nu, Emax, penal, N, U, phi, dtype=LD):
    """y = N G N phi, element by element"""
    Nv = np.asarray(N, dtype=dtype)
    g = ghat(np.asarray(U, dtype=dtype)[dofs], h, nu, dtype)
    pe = (Nv * np.asarray(phi, dtype=dtype))[dofs].reshape(-1, 8, 3)
    fe = modulus(x, Emax, penal, dtype)[:, None, None] * np.einsum("eab,ebk->eak", g, pe)
    y = np.zeros(3 * nnode, dtype=dtype)
    np.add.at(y, dofs, fe.reshape(-1, 24))
    return Nv * y


def quad_form(dofs, h, nu, N, U, phi, dtype=LD):
    """(N phi)_e^T (g_e(U_e) (x) I_3) (N phi)_e [nel]"""
    g = ghat(np.asarray(U, dtype=dtype)[dofs], h, nu, dtype)
    pe = (np.asarray(N, dtype=dtype) * np.asarray(phi, dtype=dtype))[dofs].reshape(-1, 8, 3)
    return np.einsum("eak,eab,ebk->e", pe, g, pe)


def geom_sens(x, dofs, h, nu, Emax, penal, N, U, Phi, w, scale, dtype=LD):
    """scale p x^(p-1) Emax sum_l w_l (N phi_l)_e^T (g_e (x) I_3) (N phi_l)_e [nel]"""
    xe, p = np.asarray(x, dtype=dtype), dtype(penal)
    acc = np.zeros(dofs.shape[0], dtype=dtype)
    for wl, phi in zip(w, Phi):
        acc = acc + dtype(wl) * quad_form(dofs, h, nu, N, U, phi, dtype)
    return dtype(scale) * (p * xe ** (p - 1) * dtype(Emax)) * acc


def geom_adjoint_rhs(x, dofs, nnode, h, nu, Emax, penal, N, Phi, w, scale, dtype=LD):
    """scale sum_l w_l d((N phi_l)^T G (N phi_l)) / du [3 nnode], supports not applied"""
    gn, cb, _, wq = tables(h, nu, dtype)
    Nv = np.asarray(N, dtype=dtype)
    sv = np.zeros((dofs.shape[0], 8, 6), dtype=dtype)
    for wl, phi in zip(w, Phi):
        pe = (Nv * np.asarray(phi, dtype=dtype))[dofs].reshape(-1, 8, 3)
        H = np.einsum("qdb,ebk->eqkd", gn, pe)
        s = np.einsum("eqki,eqkj->eqij", H, H)
        v = np.stack([s[..., 0, 0], s[..., 1, 1], s[..., 2, 2], 2 * s[..., 0, 1], 2 * s[..., 1, 2], 2 * s[..., 0, 2]], axis=-1)
        sv = sv + dtype(wl) * v
    re = (modulus(x, Emax, penal, dtype) * wq)[:, None] * np.einsum("qrj,eqr->ej", cb, sv)
    out = np.zeros(3 * nnode, dtype=dtype)
    np.add.at(out, dofs, re)
    return dtype(scale) * out


# ---- supports and loads
def clamp_N(ne):
    N = np.ones((ne[2] + 1, ne[1] + 1, ne[0] + 1, 3))
    N[:, :, 0, :] = 0.0
    return N.reshape(-1)


def load_cantilever(ne):
    """the reference's line load: -0.001 in z along the edge x = xmax, z = zmin, half loads at the two end nodes"""
    R = np.zeros((ne[2] + 1, ne[1] + 1, ne[0] + 1, 3))
    R[0, :, ne[0], 2] = -0.001
    R[0, 0, ne[0], 2] = R[0, ne[1], ne[0], 2] = -0.0005
    return R.reshape(-1)


def load_axial(ne, total=1.0):
    """uniform traction along -x on the face x = xmax, `total` in sum: consistent nodal loads"""
    R = np.zeros((ne[2] + 1, ne[1] + 1, ne[0] + 1, 3))
    wz, wy = np.full(ne[2] + 1, 2.0), np.full(ne[1] + 1, 2.0)
    wz[0] = wz[-1] = wy[0] = wy[-1] = 1.0
    R[:, :, ne[0], 0] = -(float(total) / (ne[1] * ne[2]) / 4.0) * wz[:, None] * wy[None, :]
    return R.reshape(-1)


def smooth_field(ne, seed):
    """a random smooth nodal field [3 nnode]: a few low trigonometric modes with random amplitudes"""
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(ne[2] + 1) / max(ne[2], 1), np.arange(ne[1] + 1) / max(ne[1], 1), np.arange(ne[0] + 1) / max(ne[0], 1),
                          indexing="ij")
    f = np.zeros(i.shape + (3,))
    for c in range(3):
        for _ in range(4):
            a, kx, ky, kz, ph = rng.uniform(-1, 1), rng.uniform(0.5, 3), rng.uniform(0.5, 3), rng.uniform(0.5, 3), rng.uniform(0, 6.28)
            f[..., c] += a * np.sin(kx * i + ky * j + kz * k + ph)
    return f.reshape(-1)


def design_01(ne, seed):
    return (np.random.default_rng(seed).uniform(0, 1, ne[0] * ne[1] * ne[2]) < 0.6).astype(np.float64)


def design_mixed(ne, seed):
    """uniform(0.1, 1) with every third element below 0.1"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.1, 1.0, ne[0] * ne[1] * ne[2])
    x[::3] = rng.uniform(0.0, 0.095, x[::3].size)
    return x


def _assemble(dofs, Ke, n):
    """sparse matrix from per-element matrices Ke [nel, 24, 24]"""
    rows = np.repeat(dofs, 24, axis=1).ravel()
    cols = np.tile(dofs, (1, 24)).ravel()
    return sp.coo_matrix((np.asarray(Ke, dtype=np.float64).ravel(), (rows, cols)), shape=(n, n)).tocsr()


class Pencil:
    """A and B = -N G(x, u) N of one mesh, design and load, dense eigenpairs, J and its gradient"""

    def __init__(self, ne, h, x, N, F, Emin=1e-6, Emax=1.0, penal=3.0, nu=0.3, KE=None):
        self.ne, self.h, self.nu = ne, h, nu
        self.x, self.N, self.F = np.asarray(x, dtype=np.float64), np.asarray(N, dtype=np.float64), np.asarray(F, dtype=np.float64)
        self.Emin, self.Emax, self.penal = Emin, Emax, penal
        self.KE = np.asarray(ke(h, nu, LD) if KE is None else KE, dtype=np.float64).reshape(24, 24)
        self.dofs = elem_dofs(*ne)
        self.nnode = (ne[0] + 1) * (ne[1] + 1) * (ne[2] + 1)
        self.n = 3 * self.nnode
        self.free = np.flatnonzero(self.N > 0)
        E = Emin + self.x ** penal * (Emax - Emin)
        D = sp.diags(self.N)
        self.A = (D @ _assemble(self.dofs, E[:, None, None] * self.KE[None], self.n) @ D + sp.diags(1.0 - self.N)).tocsr()
        self.lu = spl.splu(self.A.tocsc())
        self.u = self.lu.solve(self.N * self.F)
        g = np.asarray(ghat(self.u[self.dofs], h, nu, LD), dtype=np.float64)
        Ge = (Emax * self.x ** penal)[:, None, None] * np.einsum("eab,kl->eakbl", g, np.eye(3)).reshape(-1, 24, 24)
        self.B = (-(D @ _assemble(self.dofs, Ge, self.n) @ D)).tocsr()

    def eigh_all(self):
        """dense eigh on the free dofs -> (mu ascending [nfree], V [nfree, nfree] A-orthonormal)"""
        f = self.free
        Bd = self.B[f][:, f].toarray()
        return scipy.linalg.eigh(0.5 * (Bd + Bd.T), self.A[f][:, f].toarray())

    def modes(self, k):
        """the k largest POSITIVE mu, descending, with A-normalised vectors on all dofs -> (mu[k], Phi[n, k], mu_all ascending)"""
        mu, V = self.eigh_all()
        idx = np.argsort(-mu)[:k]
        assert (mu[idx] > 0).all(), "fewer than %d positive eigenvalues" % k
        Phi = np.zeros((self.n, k))
        Phi[self.free] = V[:, idx]
        return mu[idx], Phi, mu

    def apply_ld(self, v):
        """(A v, B v) in 80-bit arithmetic, element by element, with the float64 state u"""
        Nv, E = self.N.astype(LD), LD(self.Emin) + self.x.astype(LD) ** LD(self.penal) * (LD(self.Emax) - LD(self.Emin))
        ve = (Nv * np.asarray(v, dtype=LD))[self.dofs]
        y = np.zeros(self.n, dtype=LD)
        np.add.at(y, self.dofs, E[:, None] * (ve @ self.KE.astype(LD).T))
        Bv = -geom_apply(self.x, self.dofs, self.nnode, self.h, self.nu, self.Emax, self.penal, self.N, self.u, v, LD)
        return Nv * y + (1 - Nv) * np.asarray(v, dtype=LD), Bv

    def refine(self, Phi):
        """Rayleigh quotients of eigh's vectors in 80-bit arithmetic: an eigenvector off by d gives its eigenvalue to d^2"""
        out = []
        for i in range(Phi.shape[1]):
            Av, Bv = self.apply_ld(Phi[:, i])
            v = Phi[:, i].astype(LD)
            out.append((v @ Bv) / (v @ Av))
        return np.array(out, dtype=LD)

    @staticmethod
    def J_of(mu, P=8.0):
        mu = np.asarray(mu, dtype=LD)
        return np.sum(mu ** LD(P)) ** (1 / LD(P))

    def J(self, nev, P=8.0):
        mu, Phi, _ = self.modes(nev)
        return self.J_of(self.refine(Phi), P)

    def dJ(self, mu, Phi, P=8.0, adjoint=True, parts=False):
        """dJ/dx [nel] from A-normalised modes (any basis of a cluster that lies whole inside the sum), 80-bit but for the
        adjoint solve"""
        nev = Phi.shape[1]
        mu = np.asarray(mu, dtype=LD)[:nev]
        J = self.J_of(mu, P)
        c = (mu / J) ** (LD(P) - 1)
        xe, p = self.x.astype(LD), LD(self.penal)
        dE = p * xe ** (p - 1) * (LD(self.Emax) - LD(self.Emin))
        KE = self.KE.astype(LD)
        stiff = np.zeros(xe.size, dtype=LD)
        for i in range(nev):
            pe = Phi[:, i].astype(LD)[self.dofs]
            stiff = stiff - c[i] * mu[i] * dE * np.einsum("er,rc,ec->e", pe, KE, pe)
        args = (self.x, self.dofs, self.h, self.nu, self.Emax, self.penal, self.N, self.u)
        explicit = geom_sens(*args, [Phi[:, i] for i in range(nev)], c, -1.0, LD)
        out = stiff + explicit
        state = np.zeros_like(out)
        if adjoint:
            r = geom_adjoint_rhs(self.x, self.dofs, self.nnode, self.h, self.nu, self.Emax, self.penal, self.N,
                                 [Phi[:, i] for i in range(nev)], c, -1.0, LD)
            v = self.lu.solve(self.N * np.asarray(r, dtype=np.float64))
            state = -dE * np.einsum("er,rc,ec->e", v.astype(LD)[self.dofs], KE, self.u.astype(LD)[self.dofs])
            out = out + state
        return (out, stiff, explicit, state) if parts else out

    def perturbed(self, dx):
        return Pencil(self.ne, self.h, self.x + dx, self.N, self.F, self.Emin, self.Emax, self.penal, self.nu, self.KE)


def subspace_angle(A, Phi_ref, v):
    """sine of the angle between v and span(Phi_ref) in the A inner product (Phi_ref A-orthonormal)"""
    Av = A @ v
    c = Phi_ref.T @ Av
    r = v - Phi_ref @ c
    return float(np.sqrt(max(r @ (A @ r), 0.0) / (v @ Av)))


def subspace_iteration(P, nev, q=8, tol=1e-8, max_iter=60, seed=5):
    """the device's iteration with sparse direct solves -> (mu[nev] descending, X, iterations, residuals)"""
    X = P.N[:, None] * np.random.default_rng(seed).uniform(-1.0, 1.0, (P.n, q))
    for it in range(1, max_iter + 1):
        Y = P.lu.solve(P.B @ X)
        AY, BY = P.A @ Y, P.B @ Y
        Bt, At = Y.T @ BY, Y.T @ AY
        th, Q = scipy.linalg.eigh(0.5 * (Bt + Bt.T), 0.5 * (At + At.T))
        o = np.argsort(-th)
        th, Q = th[o], Q[:, o]
        X, AX, BX = Y @ Q, AY @ Q, BY @ Q
        if (th > 0).sum() < nev:
            continue
        res = np.linalg.norm(BX[:, :nev] - AX[:, :nev] * th[:nev], axis=0) / np.linalg.norm(BX[:, :nev], axis=0)
        if res.max() <= tol:
            return th, X, it, res
    raise RuntimeError("the restated subspace iteration did not converge")


# ---- the meshes and designs of the GPU tests
KERNEL_MESHES = [((3, 3, 3), (0.25, 0.25, 0.25)), ((5, 2, 7), (0.25, 0.25, 0.25)), ((7, 1, 5), (0.25, 0.25, 0.25)),
                 ((20, 12, 8), (0.05, 0.04, 0.03))]
EMIN, EMAX, PENAL, NU = 1e-6, 1.0, 3.0, 0.3


def design_uniform(ne, seed):
    return np.full(ne[0] * ne[1] * ne[2], 0.5)


def design_random(ne, seed):
    return np.random.default_rng(seed).uniform(0.3, 1.0, ne[0] * ne[1] * ne[2])


MODE_CASES = {
    "column": dict(ne=(16, 4, 4), h=(1.0, 1.0, 1.0), nev=2, nlvls=2, load="axial", design=design_uniform, seed=0),
    "random": dict(ne=(16, 4, 4), h=(1.0, 1.0, 1.0), nev=2, nlvls=2, load="axial", design=design_random, seed=21),
    "sign": dict(ne=(16, 2, 8), h=(1.0, 1.0, 1.0), nev=1, nlvls=2, load="cantilever", design=design_uniform, seed=0),
}
SLAB_CASES = {
    "slab2": dict(ne=(16, 4, 8), h=(1.0, 1.0, 1.0), nev=2, nlvls=2, load="axial", design=design_uniform, seed=22),
    "slab3": dict(ne=(12, 4, 12), h=(1.0, 1.0, 1.0), nev=2, nlvls=2, load="axial", design=design_random, seed=23),
    "slab3thin": dict(ne=(8, 4, 6), h=(1.0, 1.0, 1.0), nev=2, nlvls=1, load="axial", design=design_random, seed=24),
}


def case_load(c):
    return load_axial(c["ne"]) if c["load"] == "axial" else load_cantilever(c["ne"])
