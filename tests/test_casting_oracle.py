"""The numpy restatement of the casting filter (tests/casting_ref.py), which the GPU tests measure the device against, held to
the filter's own properties on the CPU: the sandwich, the growth law of a uniform line, monotonicity, central
differences in 80-bit arithmetic, zeros, the ends p = 0, p = n and n = 1, and the equality of a draw along x with the draw along
z of the axis-swapped field.  Every figure is printed with its bound before it is asserted."""
import numpy as np
import pytest

from tests import casting_ref as ref

LD = ref.LD


@pytest.mark.parametrize("eps", [1e-4, 1e-6])
@pytest.mark.parametrize("n", [16, 128, 512])
def test_sandwich_and_growth_law_on_lines(n, eps):
    """hardmax <= c <= hardmax + m sqrt(eps)/2 on random, checkerboard and zero-layer lines; on a uniform line
    c - x <= sqrt(m eps / 2), from e' = (e + sqrt(e^2 + eps)) / 2, e'^2 <= e^2 + eps/2.  The roundings of c: five operations per
    step on numbers below 2, each step's error passed on with a factor of at most 1, so n * 5 * 2^-64 * 2 in 80-bit arithmetic"""
    ne = (3, 2, n)
    tol = 10 * n * 2.0 ** -64
    for draw in ("+z", "-z", "z:%d" % (n // 2 + 1)):
        for kind in ("random", "checker", "zerolayers", "ones"):
            x = ref.field(kind, ne, draw)
            c = ref.forward(x, ne, draw, LD, eps)["c"]
            br = ref.sandwich_breach(x, c, ne, draw, eps)
            print("n = %d eps = %g %s %s: c leaves the sandwich by %.3e (allowed %.3e)" % (n, eps, draw, kind, br, tol))
            assert br <= tol
        x = ref.field("uniform", ne, draw)
        c = ref.forward(x, ne, draw, LD, eps)["c"]
        m = ref.hardmax(x, ne, draw)[1]
        over = float((c - LD(0.12) - np.sqrt(m.astype(LD) * LD(eps) / 2)).max())
        print("n = %d eps = %g %s uniform 0.12: largest c %.5f, c - x exceeds sqrt(m eps / 2) by %.3e (allowed %.3e)"
              % (n, eps, draw, float(c.max()), over, tol))
        assert over <= tol and float((c - LD(0.12)).min()) >= 0.0


def test_uniform_lines_end_where_they_were_measured():
    """the figures the default eps = 1e-6 rests on: a uniform 0.12 line of 128 cells ends at 0.12791, one of 512 cells at 0.13595,
    and at eps = 1e-4 at 0.2795; a void run of 128 cells stays below 0.008"""
    for n, eps, end, tol in ((128, 1e-6, 0.12791, 5e-6), (512, 1e-6, 0.13595, 5e-6), (512, 1e-4, 0.2795, 5e-5)):
        ne = (1, 1, n)
        c = ref.forward(ref.field("uniform", ne), ne, "+z", LD, eps)["c"]
        print("uniform 0.12, n = %d, eps = %g: ends at %.6f (measured %.5f)" % (n, eps, float(c[0]), end))
        assert abs(float(c[0]) - end) <= tol
    void = ref.forward(np.zeros(128), (1, 1, 128), "+z", LD, 1e-6)["c"]
    print("void run of 128 cells at eps = 1e-6 rises to %.6f (bound sqrt(127e-6 / 2) = %.6f)" % (float(void[0]), np.sqrt(127e-6 / 2)))
    assert float(void[0]) <= 0.008


@pytest.mark.parametrize("dtype", [np.float64, LD])
@pytest.mark.parametrize("ne", ref.MESHES)
def test_monotone_no_nan_and_zeros(ne, dtype):
    """c rises along every sweep (exact in exact arithmetic, to 4 ulp here) on every field, whole zero layers and the all-zero
    field included; rho >= sqrt(eps) > 0, so no NaN and no division by zero in c, q or the transpose"""
    g = np.random.default_rng(5).uniform(-1.0, 1.0, ne[0] * ne[1] * ne[2])
    for draw in ref.draws(ne):
        for kind in ("random", "checker", "zerolayers", "zeros"):
            x = np.zeros(g.size) if kind == "zeros" else ref.field(kind, ne, draw)
            f = ref.forward(x, ne, draw, dtype)
            out = ref.adjoint(f, g, ne, draw)
            mono = ref.monotone_breach_ulps(f["c"], ne, draw)
            assert mono <= 4.0, (draw, kind, mono)
            assert np.isfinite(f["c"].astype(np.float64)).all() and np.isfinite(f["q"].astype(np.float64)).all()
            assert np.isfinite(out.astype(np.float64)).all()
            assert float(np.abs(f["q"]).max()) <= 1.0
    print("%s %s: %d draws, monotone to 4 ulp, finite" % (ref.name(ne), np.dtype(dtype).name, len(ref.draws(ne))))


@pytest.mark.parametrize("ne", ref.MESHES)
def test_transpose_against_central_differences_in_80_bit(ne):
    """g . (F(x + h W) - F(x - h W)) / 2h against (J^T g) . W in 80-bit arithmetic, h = 1e-6, at or below 1e-6 relative; eps = 1e-4
    as on the device (tests/test_gpu_casting.py, check 3)"""
    h = LD(1e-6)
    rng = np.random.default_rng(11)
    n = ne[0] * ne[1] * ne[2]
    x, W, g = ref.field("random", ne), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    for draw in ref.draws(ne):
        f0 = ref.forward(x, ne, draw, LD, 1e-4)
        an = (ref.adjoint(f0, g, ne, draw) * W).sum()
        fp = ref.forward(x.astype(LD) + h * W, ne, draw, LD, 1e-4)["c"]
        fm = ref.forward(x.astype(LD) - h * W, ne, draw, LD, 1e-4)["c"]
        fd = (g * (fp - fm)).sum() / (2 * h)
        err = float(abs(fd - an) / abs(an))
        print("%s %s: (J^T g).W %.9e, central difference off by %.3e (bound 1e-6)" % (ref.name(ne), draw, float(an), err))
        assert err <= 1e-6


def test_ends_of_the_parting_range_and_single_layers():
    """p = 0 and p = n are one sweep each, and mirror images of one another; n = 1 is the identity with a transpose of the
    identity; a two-sided draw is the two one-sided draws of its halves"""
    ne = (5, 4, 9)
    x = ref.field("random", ne)
    g = np.random.default_rng(2).uniform(-1.0, 1.0, x.size)
    up, dn = ref.forward(x, ne, "+z"), ref.forward(x, ne, "-z")
    flip = ref.lines(x, ne, 2)[::-1].ravel()
    upf = ref.forward(flip, ne, "+z")
    assert np.array_equal(ref.lines(upf["c"], ne, 2)[::-1].ravel(), dn["c"])
    assert np.array_equal(ref.adjoint(dn, g, ne, "-z"), ref.lines(ref.adjoint(upf, ref.lines(g, ne, 2)[::-1].ravel(), ne, "+z"), ne, 2)[::-1].ravel())
    two = ref.forward(x, ne, "z:4")
    lay = ne[0] * ne[1]
    lo, hi = ref.forward(x[:4 * lay], (5, 4, 4), "-z"), ref.forward(x[4 * lay:], (5, 4, 5), "+z")
    assert np.array_equal(two["c"], np.concatenate([lo["c"], hi["c"]])) and np.array_equal(two["q"], np.concatenate([lo["q"], hi["q"]]))
    assert np.array_equal(up["c"][-lay:], x[-lay:].astype(LD)) and np.array_equal(dn["c"][:lay], x[:lay].astype(LD))
    for ne1, draw in (((4, 1, 1), "+y"), ((4, 1, 1), "-z"), ((1, 1, 4), "+x"), ((1, 1, 4), "-y")):
        x1 = ref.field("random", ne1)
        f = ref.forward(x1, ne1, draw, np.float64)
        assert np.array_equal(f["c"], x1) and np.array_equal(f["q"], np.ones(4))
        assert np.array_equal(ref.adjoint(f, x1 - 0.5, ne1, draw), x1 - 0.5)


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_a_draw_along_x_equals_the_draw_along_z_of_the_swapped_field(dtype):
    """bit for bit, c, q and the transpose, one- and two-sided: the restatement is one recurrence whatever the axis"""
    ne = (7, 5, 11)
    x = ref.field("random", ne)
    g = np.random.default_rng(4).uniform(-1.0, 1.0, x.size)
    for name, other in (("x", "z"), ("x", "y"), ("y", "z")):
        a, b = ref.AXES[name], ref.AXES[other]
        xs, ns = ref.swap(x, ne, a, b)
        gs = ref.swap(g, ne, a, b)[0]
        for tail in ("+%s", "-%s", "%s:3"):
            da, db = tail % name, tail % other
            fa, fb = ref.forward(x, ne, da, dtype), ref.forward(xs, ns, db, dtype)
            for k in ("c", "q"):
                assert np.array_equal(ref.swap(fa[k], ne, a, b)[0], fb[k]), (da, db, k)
            assert np.array_equal(ref.swap(ref.adjoint(fa, g, ne, da), ne, a, b)[0], ref.adjoint(fb, gs, ns, db))
