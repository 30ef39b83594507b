"""80-bit numpy restatement of the self-weight formulas (include/topopt_amd.h) and nothing else.

    V_e = hx hy hz,  t = x / x_low
    m(x) = x, m'(x) = 1                                  for x >= x_low or x_low = 0
    m(x) = x (6 t^5 - 5 t^6),  m'(x) = 36 t^5 - 35 t^6   for x < x_low
    f_n = (V_e / 8) b sum_{e contains n} m(x_e)
    d(v^T N f)/dx_e = m'(x_e) (V_e / 8) sum_a sum_c b_c N_{a,c} v_{a,c}
    K u = N (F + f):  c = (F + f)^T u,  dc/dx_e = -p x^(p-1) (Emax - Emin) u_e^T KE u_e + 2 d(u^T N f)/dx_e
"""
import numpy as np

LD = np.longdouble
LX, LY, LZ = [0, 1, 1, 0, 0, 1, 1, 0], [0, 0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1, 1, 1]   # include/topopt_amd.h


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


def mass(x, x_low):
    x = np.asarray(x, dtype=LD)
    if x_low == 0:
        return x.copy()
    t = np.minimum(x / LD(x_low), LD(1))       # (the damped branch is evaluated everywhere and selected below)
    return np.where(x >= LD(x_low), x, x * (t ** 5 * (6 - 5 * t)))


def dmass(x, x_low):
    x = np.asarray(x, dtype=LD)
    if x_low == 0:
        return np.ones_like(x)
    t = np.minimum(x / LD(x_low), LD(1))
    return np.where(x >= LD(x_low), LD(1), t ** 5 * (36 - 35 * t))


def volume(h):
    return LD(h[0]) * LD(h[1]) * LD(h[2])


def load(x, dofs, nnode, h, b, x_low):
    """f [3 nnode]: every element hands m(x_e) V_e / 8 b to its eight corners"""
    f = np.zeros(3 * nnode, dtype=LD)
    per = mass(x, x_low) * (volume(h) / 8)
    np.add.at(f, dofs, per[:, None] * np.tile(np.asarray(b, dtype=LD), 8)[None, :])
    return f


def sens_term(x, dofs, h, b, x_low, N, v):
    """d(v^T N f)/dx_e [nel]"""
    bN = np.tile(np.asarray(b, dtype=LD), 8)[None, :] * np.asarray(N, dtype=LD)[dofs]
    return dmass(x, x_low) * (volume(h) / 8) * (bN * np.asarray(v, dtype=LD)[dofs]).sum(axis=1)


def uKu(KE, dofs, u, v=None):
    ue = np.asarray(u, dtype=LD)[dofs]
    ve = ue if v is None else np.asarray(v, dtype=LD)[dofs]
    return np.einsum("er,rc,ec->e", ve, np.asarray(KE, dtype=LD).reshape(24, 24), ue)


def dcdx(x, dofs, h, b, x_low, N, KE, u, Emin, Emax, penal):
    """total derivative of c = (F + f)^T u -> (dcdx, classical part, self-weight part)"""
    xe = np.asarray(x, dtype=LD)
    classical = -LD(penal) * xe ** (LD(penal) - 1) * (LD(Emax) - LD(Emin)) * uKu(KE, dofs, u)
    body = 2 * sens_term(x, dofs, h, b, x_low, N, u)
    return classical + body, classical, body
