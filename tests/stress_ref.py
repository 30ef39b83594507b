"""numpy restatement of the von Mises p-norm formulas (include/topopt_amd.h) and nothing else: what
tests/test_gpu_stress.py holds the stress kernels to, importable by the row-wise tests (tests/response_rowwise.py).

    eps_e = B0 u_e,  sigma_e = Emax x_e^q C eps_e,  M = B0^T C^T Vm C B0,  s_e = u_e^T M u_e,  vm_e = Emax x_e^q sqrt(s_e)
    pnorm = (sum_e vm_e^P)^(1/P),  dpdx_e = pnorm^(1-P) q Emax^P x_e^(qP-1) s_e^(P/2)
    adj_rhs = sum_e pnorm^(1-P) (Emax x_e^q)^P s_e^((P-2)/2) L_e^T M u_e
"""
import numpy as np

LD = np.longdouble
NU = 0.3
EMAX = 1.0
LX, LY, LZ = [0, 1, 1, 0, 0, 1, 1, 0], [0, 0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1, 1, 1]   # include/topopt_amd.h


def vonmises_form(h, nu=NU, dtype=LD):
    """M = B0^T C^T Vm C B0 of the hx x hy x hz box element at its centroid; rows xx, yy, zz, xy, yz, zx (engineering shear)"""
    one = dtype(1)
    sg = np.array([[2 * LX[a] - 1, 2 * LY[a] - 1, 2 * LZ[a] - 1] for a in range(8)], dtype=dtype)
    B = np.zeros((6, 24), dtype=dtype)
    for a in range(8):
        dN = [sg[a, d] / (4 * dtype(h[d])) for d in range(3)]         # dN_a/dx_d at xi = eta = zeta = 0
        B[0, 3 * a + 0] = dN[0]
        B[1, 3 * a + 1] = dN[1]
        B[2, 3 * a + 2] = dN[2]
        B[3, 3 * a + 0], B[3, 3 * a + 1] = dN[1], dN[0]               # gamma_xy = du/dy + dv/dx
        B[4, 3 * a + 1], B[4, 3 * a + 2] = dN[2], dN[1]               # gamma_yz = dv/dz + dw/dy
        B[5, 3 * a + 0], B[5, 3 * a + 2] = dN[2], dN[0]               # gamma_zx = du/dz + dw/dx
    nu = dtype(nu)
    lam, mu = nu / ((one + nu) * (one - 2 * nu)), one / (2 * (one + nu))
    C = np.zeros((6, 6), dtype=dtype)
    C[:3, :3] = lam
    C[np.arange(3), np.arange(3)] = lam + 2 * mu
    C[np.arange(3, 6), np.arange(3, 6)] = mu
    Vm = np.zeros((6, 6), dtype=dtype)
    Vm[:3, :3] = -one / 2
    Vm[np.arange(3), np.arange(3)] = one
    Vm[np.arange(3, 6), np.arange(3, 6)] = 3 * one
    S = C @ B
    return S.T @ Vm @ S


def elem_dofs(ex, ey, ez):
    """[nel, 24] global dofs of every element: node i + nx (j + ny k), element i + ex (j + ey k), corner order of the header"""
    nx, ny = ex + 1, ey + 1
    k, j, i = np.meshgrid(np.arange(ez), np.arange(ey), np.arange(ex), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    cols = []
    for a in range(8):
        nd = (i + LX[a]) + nx * ((j + LY[a]) + ny * (k + LZ[a]))
        cols += [3 * nd, 3 * nd + 1, 3 * nd + 2]
    return np.stack(cols, axis=1)


def stress_ref(M, dofs, U, x, q, P, Emax=EMAX, dtype=LD, relative=False):
    """-> dict(s, vm, pnorm, vm_max, dpdx, adj) from the formulas of the module docstring, nothing else.  relative=True takes
    u_e relative to the element's corner 0 (M annihilates translations: the same value to rounding) -- for the one input whose
    point is elements in rigid translation, where u_e^T M u_e itself leaves a rounding residue under the square root"""
    ue = U.astype(dtype)[dofs]
    if relative:
        ue = ue - np.tile(ue[:, :3], (1, 8))
    Mu = ue @ M.astype(dtype)
    s = np.maximum(np.einsum("er,er->e", ue, Mu), 0)
    xe, q, P, Emax = x.astype(dtype), dtype(q), dtype(P), dtype(Emax)
    a = Emax * xe ** q
    vm = a * np.sqrt(s)
    S = (vm ** P).sum()
    out = dict(s=s, vm=vm, vm_max=vm.max(), pnorm=S ** (1 / P))
    n = 3 * (int(dofs.max()) // 3 + 1)
    if S == 0:
        out.update(dpdx=np.zeros(len(xe), dtype=dtype), adj=np.zeros(n, dtype=dtype))
        return out
    pn = out["pnorm"]
    out["dpdx"] = pn ** (1 - P) * q * Emax ** P * xe ** (q * P - 1) * s ** (P / 2) if q != 0 else np.zeros(len(xe), dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(s > 0, pn ** (1 - P) * a ** P * s ** ((P - 2) / 2), 0)
    adj = np.zeros(n, dtype=dtype)
    np.add.at(adj, dofs, c[:, None] * Mu)
    out["adj"] = adj
    return out
