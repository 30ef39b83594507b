"""The numpy / scipy restatement the buckling GPU tests measure against (tests/buckling_ref.py), held to what it must satisfy on its
own: the properties of the element's stress stiffness g_e (rows sum to zero, symmetric, linear in u_e, zero for a rigid
translation, the closed form for a uniform uniaxial strain), the element matrix its tables give against the oracle's KE, the
sign and ordering of the pencil's spectrum, and the analytic gradient of J = (sum mu_i^P)^(1/P) against its own central
difference -- through the double mode of a square column too, and without the adjoint term (must be far off).

The gradient's bound is 1e-6: the measured distances are 4e-10 .. 3e-8 (printed below), more than 10 x inside it."""
import numpy as np
import pytest

from tests import buckling_ref as ref

LD = ref.LD
H1 = (1.0, 1.0, 1.0)


@pytest.mark.parametrize("h", [H1, (0.05, 0.04, 0.03)])
def test_element_matrix_of_the_tables_is_the_oracles(orc, h):
    KE = np.asarray(orc.hex8_ke_box(h[0], h[1], h[2], ref.NU)).reshape(24, 24)
    mine = np.asarray(ref.ke(h, ref.NU, LD), dtype=np.float64)
    err = float(np.abs(mine - KE).max() / np.abs(KE).max())
    print("h %s: max|sum w B^T C0 B - KE| / max|KE| = %.3e (bound 8 * 2^-53)" % (h, err))
    assert err <= 8 * 2.0 ** -53


@pytest.mark.parametrize("h", [H1, (0.05, 0.04, 0.03)])
def test_ghat_properties(h):
    rng = np.random.default_rng(1)
    u, v = rng.uniform(-1, 1, (5, 24)), rng.uniform(-1, 1, (5, 24))
    g, gv = ref.ghat(u, h), ref.ghat(v, h)
    top = float(np.abs(g).max())
    ulp = float(np.finfo(LD).eps)
    rows = float(np.abs(g.sum(axis=2)).max())
    sym = float(np.abs(g - g.transpose(0, 2, 1)).max())
    lin = float(np.abs(ref.ghat(2 * u.astype(LD) - 3 * v.astype(LD), h) - (2 * g - 3 * gv)).max())
    print("h %s: row sums %.3e, asymmetry %.3e, 2u - 3v against 2g(u) - 3g(v) %.3e, all of max|g| = %.3e" % (h, rows / top, sym / top, lin / top, top))
    assert rows <= 64 * ulp * top and sym <= 64 * ulp * top and lin <= 256 * ulp * top
    t = np.tile(np.array([0.3, -1.1, 0.7]), 8)[None, :]
    assert float(np.abs(ref.ghat(t, h)).max()) <= 64 * ulp * 1.1 * top / float(np.abs(u).max())


@pytest.mark.parametrize("h", [H1, (0.05, 0.04, 0.03)])
def test_ghat_of_a_uniform_uniaxial_strain_is_the_closed_form(h):
    """u_x = eps x: the strain is eps in xx alone, sigma = C0[:, 0] eps at every point; with nu = 0 the stress is sigma_xx = eps
    alone and g_e = sigma int dN_a/dx dN_b/dx -- the 1-D stiffness [[1, -1], [-1, 1]] / hx along x times the consistent 1-D mass
    h [[2, 1], [1, 2]] / 6 along y and z (the 2-point rule integrates these quadratics exactly)"""
    eps = 0.01
    ue = np.zeros((1, 24))
    ue[0, 0::3] = eps * h[0] * np.array(ref.LX, dtype=float)
    g = ref.ghat(ue, h, nu=0.0)[0]
    S = lambda a, b: (1 if a == b else -1) / LD(h[0])
    M = lambda d, a, b: LD(h[d]) * (2 if a == b else 1) / 6
    closed = np.array([[LD(eps) * S(ref.LX[a], ref.LX[b]) * M(1, ref.LY[a], ref.LY[b]) * M(2, ref.LZ[a], ref.LZ[b]) for b in range(8)]
                       for a in range(8)])
    err = float(np.abs(g - closed).max() / np.abs(closed).max())
    print("h %s: max|g - sigma int dN/dx dN/dx| / max = %.3e" % (h, err))
    assert err <= 1e-14        # the Gauss point's literal is 1 / sqrt(3) to 16 digits


def _fd_case(orc, ne, load, x, nev, seed, symmetric=False):
    eps = 1e-6
    KE = np.asarray(orc.hex8_ke_box(1.0, 1.0, 1.0, ref.NU)).reshape(24, 24)
    F = ref.load_axial(ne) if load == "axial" else ref.load_cantilever(ne)
    P = ref.Pencil(ne, H1, x, ref.clamp_N(ne), F, ref.EMIN, ref.EMAX, ref.PENAL, ref.NU, KE=KE)
    mu64, Phi, mu_all = P.modes(nev + 1)
    mu = P.refine(Phi)
    W = np.random.default_rng(seed).uniform(-1.0, 1.0, x.size)
    if symmetric:
        W = 0.5 * (W + W.reshape(ne[2], ne[1], ne[0]).transpose(1, 0, 2).reshape(-1))
    full, stiff, explicit, state = P.dJ(mu[:nev], Phi[:, :nev], 8.0, parts=True)
    an, no_adj = float(full @ W.astype(LD)), float((stiff + explicit) @ W.astype(LD))
    fd = float((P.perturbed(eps * W).J(nev) - P.perturbed(-eps * W).J(nev)) / (2 * LD(eps)))
    print("%dx%dx%d %s: mu %s, most negative %.4e; dJ/dx . W = %.12e, central difference %.12e, off by %.3e (bound 1e-6); without the "
          "adjoint term off by %.3e" % (ne + (load, " ".join("%.6e" % v for v in mu64), mu_all[0], an, fd, abs(an / fd - 1), abs(no_adj / fd - 1))))
    return mu, mu_all, abs(an / fd - 1), abs(no_adj / fd - 1)


def test_restated_gradient_through_the_double_mode_of_a_square_column(orc):
    ne = (6, 2, 2)
    mu, mu_all, err, no_adj = _fd_case(orc, ne, "axial", np.full(24, 0.5), 2, 1, symmetric=True)
    assert float(abs(mu[1] / mu[0] - 1)) < 1e-8 and float(mu[2] / mu[1]) < 0.5
    assert err <= 1e-6 and no_adj > 0.1


@pytest.mark.parametrize("ne,seed", [((6, 2, 2), 5), ((8, 2, 2), 3)])
def test_restated_gradient_axial(orc, ne, seed):
    x = np.random.default_rng(seed).uniform(0.3, 1.0, ne[0] * ne[1] * ne[2])
    mu, mu_all, err, no_adj = _fd_case(orc, ne, "axial", x, 2, seed + 10)
    assert float(mu[2] / mu[1]) < 0.9
    assert err <= 1e-6 and no_adj > 0.1


def test_restated_gradient_under_the_cantilever_load(orc):
    """6x4x2 with the reference's line load: a mixed-sign spectrum, the most negative eigenvalue larger in magnitude than the
    largest positive one; the gradient is that of the POSITIVE one"""
    ne = (6, 4, 2)
    x = np.random.default_rng(4).uniform(0.3, 1.0, 48)
    mu, mu_all, err, no_adj = _fd_case(orc, ne, "cantilever", x, 1, 3)
    assert mu_all[0] < 0 < mu[0] and -mu_all[0] > mu[0]
    assert err <= 1e-6 and no_adj > 0.1


def test_adjoint_rhs_is_the_derivative_of_the_quadratic_form():
    """d(phi^T G(u) phi)/du . du against the form's own difference (it is linear in u: the difference is exact to rounding)"""
    ne, h = (3, 2, 2), (0.5, 0.4, 0.3)
    nnode, dofs = 4 * 3 * 3, ref.elem_dofs(*ne)
    N = ref.clamp_N(ne)
    x = ref.design_mixed(ne, 2)
    phi, u, du = (ref.smooth_field(ne, s) * N for s in (1, 2, 3))
    r = ref.geom_adjoint_rhs(x, dofs, nnode, h, ref.NU, 2.5, 3.0, N, [phi], [1.0], 1.0, LD)
    q = lambda uu: (ref.modulus(x, 2.5, 3.0) * ref.quad_form(dofs, h, ref.NU, N, uu, phi, LD)).sum()
    lhs, rhs = float(r @ du.astype(LD)), float(q(u + du) - q(u))
    print("r . du = %.15e, q(u + du) - q(u) = %.15e" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-15 * float(np.abs(r) @ np.abs(du))


@pytest.mark.parametrize("name", sorted(ref.MODE_CASES) + ["slab2"])
def test_conditions_of_the_gpu_cases(name):
    """conditions, not measurements, of every case whose modes a GPU test computes: a clear step behind the wanted modes in
    magnitude, separated or truly double modes inside"""
    c = {**ref.MODE_CASES, **ref.SLAB_CASES}[name]
    ne, nev = c["ne"], c["nev"]
    P = ref.Pencil(ne, c["h"], c["design"](ne, c["seed"]), ref.clamp_N(ne), ref.case_load(c), ref.EMIN, ref.EMAX, ref.PENAL, ref.NU)
    mu, _, mu_all = P.modes(nev + 1)
    mag = np.sort(np.abs(mu_all))[::-1]
    print("%s: positive %s, most negative %.6e, |mu_9| / mu_nev = %.3f" % (name, " ".join("%.6e" % v for v in mu), mu_all[0], mag[8] / mu[nev - 1]))
    assert mu[nev] / mu[nev - 1] < 0.9
    assert all(abs(mu[i + 1] / mu[i] - 1) < 1e-8 or mu[i + 1] / mu[i] < 0.98 for i in range(nev - 1))
    assert mag[8] / mu[nev - 1] < 0.6
