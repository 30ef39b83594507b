"""The conditions the bounds of tests/test_gpu_projection.py rest on, held on the CPU: on every case and field the GPU tests use
(the largest size apart) the float64 restatement of tests/projection_ref.py and the oracle's orc_heaviside / orc_heaviside_chain stay
within a QUARTER of C_FORWARD and C_CHAIN against the 80-bit values; the arbiter agrees with the longdouble restatement; oracle and
arbiter divide by PETSc's rule (0 where the denominator is 0); and one planted error per family shows what the row-wise bound sees
and the max-norm bound of tests/test_gpu_parity.py::test_conv_filter does not."""
import numpy as np
import pytest

from tests import projection_ref as pr
from tests import rowwise as rw

LD = np.longdouble
MEASURED = {}
CPU_SIZES = [n for n in pr.SIZES if n < pr.STRIDE]


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def ld(a):
    return np.ascontiguousarray(a, dtype=LD)


def note(key, c):
    MEASURED[key] = max(MEASURED.get(key, 0.0), c)


def fields_of(n, beta, eta):
    """the fields of one size: one, or for the one-element mesh every salt in turn"""
    return [pr.field(n, beta, eta, s) for s in range(len(pr.salts(beta, eta)) if n == 1 else 1)]


@pytest.mark.parametrize("n", CPU_SIZES)
def test_restatement_and_oracle_within_a_quarter_of_the_bounds(orc, arb, n):
    for beta, eta in pr.CASES:
        for seed, x in enumerate(fields_of(n, beta, eta)):
            df = pr.rows(n, seed)
            w = lambda what: {"label": "%s n=%d beta=%g eta=%g" % (what, n, beta, eta), "dims": (n, 1, 1), "dof": 0}
            ya, ca = pr.H(x, beta, eta, LD), pr.chain(df, x, beta, eta, LD)
            sf, sc = pr.scale_forward(x, beta, eta), pr.scale_chain(df, x, beta, eta)
            note("forward restatement", rw.assert_rowwise(pr.H(x, beta, eta), ya, sf, pr.C_FORWARD / 4, w("restated forward")))
            note("forward oracle", rw.assert_rowwise(orc.heaviside(x, beta, eta), ya, sf, pr.C_FORWARD / 4, w("oracle forward")))
            note("chain restatement", rw.assert_rowwise(pr.chain(df, x, beta, eta), ca, sc, pr.C_CHAIN / 4, w("restated chain")))
            note("chain oracle", rw.assert_rowwise(df * orc.heaviside_chain(x, beta, eta), ca, sc, pr.C_CHAIN / 4, w("oracle chain")))
            # the arbiter is the 80-bit reference of the composed tests: it is the longdouble restatement to 2^-4 eps of the scale
            note("forward arbiter", rw.assert_rowwise(arb.heaviside(ld(x), beta, eta).astype(np.float64), ya.astype(np.float64), sf, 1.0,
                                                      w("arbiter forward (rounded)")))
            d = np.abs(arb.heaviside(ld(x), beta, eta) - ya).astype(np.float64)
            assert (d <= pr.EPS / 16 * sf).all(), w("arbiter forward")["label"]
            d = np.abs(ld(df) * arb.heaviside_chain(ld(x), beta, eta) - ca).astype(np.float64)
            assert (d <= pr.EPS / 16 * sc).all(), w("arbiter chain")["label"]
            # what the GPU test asserts outright holds for the reference itself
            y = pr.H(x, beta, eta)
            assert (y >= 0).all() and (y <= 1).all() and (y[x == 1.0] == 1.0).all() and (y[x == 0.0] == 0.0).all()
            o = np.argsort(x, kind="stable")
            assert (np.diff(y[o]) >= -pr.MONOTONE_SLACK).all()
    print("MEASURED n=%d" % n, {k: "%.3g" % v for k, v in sorted(MEASURED.items())})


def test_constants_follow_the_rule():
    """count and power of two as tests/projection_ref.py writes them down"""
    assert pr.C_FORWARD == max(rw.pow2(14), rw.pow2(16 * 4.0)) and pr.C_CHAIN == max(rw.pow2(23), rw.pow2(16 * 3.32))
    assert [pr.mnd_chain(n) for n in pr.MND_SIZES] == [25, 25, 25, 57] and [pr.c_mnd(n) for n in pr.MND_SIZES] == [32, 32, 32, 64]
    assert all(ex * ey * ez == n for table in (pr.SIZES, pr.MND_SIZES, pr.DIVIDE_SIZES) for n, (ex, ey, ez) in table.items())
    for beta, eta in pr.CASES:
        for n in pr.SIZES:
            x = pr.field(n, beta, eta)
            assert x.size == n and (x >= 0).all() and (x <= 1).all()
            if n >= 63:
                for v in pr.salts(beta, eta):     # every salt is there, both zeros by their sign bit
                    assert (x.view(np.int64) == np.float64(v).view(np.int64)).any(), (n, beta, eta, v)
                assert x[0] == 0.0 and x[-1] == 1.0
            if n > pr.STRIDE:
                assert set(np.float64(pr.salts(beta, eta)).view(np.int64)) <= set(x[pr.STRIDE:].view(np.int64))
        a = np.abs(beta * (np.array(pr.salts(beta, eta)) - eta))
        for t in pr.TANH_EDGES:      # both sides of every edge that lies inside [0, 1] at this beta and eta
            if t / beta * (1 + 2.0 ** -10) <= max(eta, 1.0 - eta):
                assert ((a < t) & (a > 0.99 * t)).any() and ((a > t) & (a < 1.01 * t)).any(), (beta, eta, t)


def test_mnd_restatement(orc):
    for n in pr.MND_SIZES:
        if n > pr.STRIDE:
            continue
        for name, (x, exact) in pr.mnd_fields(n).items():
            got, ref = orc.mnd(x), pr.mnd(x, LD)
            if exact is not None:
                assert got == exact == float(ref) == pr.mnd(x), (n, name)
            else:     # the oracle sums n terms in a row: n + 3 rounded operations
                assert abs(got - ref) <= (n + 3) * pr.EPS * float(np.abs(pr.mnd_terms(x, LD)).sum()) / n, (n, name)


def test_petsc_quotient_of_oracle_and_arbiter(orc, arb):
    """w = x / y with zeros of both signs in y (and 0 / 0): 0 there, the correctly rounded quotient elsewhere, bit for bit; the filter's
    gradient of type 0 on a design with exact zeros: 0.0 on those rows, finite everywhere, and the oracle within a quarter of the cone
    filter's bound of the arbiter on the others; types 0 and 1 untouched where nothing is zero"""
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 4099):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        y[::3], y[1::7], x[::6] = 0.0, -0.0, 0.0
        want = pr.petsc_div(x, y)
        assert np.isfinite(want).all() and (want[y == 0] == 0).all() and not np.signbit(want[y == 0]).any()
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(want[y != 0].view(np.int64), (x / y)[y != 0].view(np.int64))
        assert np.array_equal(orc.pointwise_divide(x, y).view(np.int64), want.view(np.int64))
        wa = arb.pointwise_divide(ld(x), ld(y))
        assert np.array_equal(wa, pr.petsc_div(x, y, LD)) and (wa[y == 0] == 0).all()
    ex, ey, ez = 12, 8, 8
    h = 1.0 / ey
    of, af = orc.Filter(ex + 1, ey + 1, ez + 1, h, 2.56 * h), arb.Filter(ex + 1, ey + 1, ez + 1, h, 2.56 * h)
    cone = rw.Cone(ex, ey, ez, h, 2.56 * h, af.conn)
    c = rw.c_filter(af.conn)
    df = rng.standard_normal(ex * ey * ez)
    for kind in ("blocks", "checker"):
        x = rw.design(kind, ex, ey, ez, 4)
        x0 = np.where(x == rw.XMIN, 0.0, x)
        assert (x0 == 0).any() and (x0 == 1).any()
        for ftype in (0, 1):
            g, ga = of.gradient(ftype, x0, x0, df), af.gradient(ftype, ld(x0), ld(x0), ld(df))
            assert np.isfinite(g).all() and np.isfinite(ga.astype(np.float64)).all()
            s = cone.scale_gradient(ftype, x0, df)
            if ftype == 0:
                assert (g[x0 == 0] == 0).all() and (ga[x0 == 0] == 0).all()
                s = np.where(x0 == 0, 0.0, s)
            rw.assert_rowwise(g, ga, s, c / 4, {"label": "oracle gradient type %d %s with zeros" % (ftype, kind), "dims": (ex, ey, ez), "dof": 0})
            xt, _ = of.project(ftype, x0)
            xta, _ = af.project(ftype, ld(x0))
            rw.assert_rowwise(xt, xta, cone.scale_forward(ftype, x0), c / 4, {"label": "oracle forward type %d %s with zeros" % (ftype, kind), "dims": (ex, ey, ez), "dof": 0})


def _saturated_row(beta, eta, sign):
    """x at which H' is 1e-6 of its peak: 1 - th^2 = 1e-6"""
    return eta + sign * np.arctanh(np.sqrt(1.0 - 1e-6)) / beta


def test_planted_errors_the_max_norm_bound_accepts():
    """One planted error per family, 1e-3 of the row's scale, on a row where H' is 1e-6 of its peak (beta = 48, eta = 0.5, a field of
    1001 elements): the row-wise bound rejects each.

    chain: the row's scale is |df_i| beta (1 + th^2) / den, so on a row whose df_i is 1e-12 of the largest the planted error is 1e-15
    of max|row| and test_conv_filter's bound (max norm, 1e-12) accepts it.
    forward: on that row the scale (|t0| + |th|) / den is 1 whatever the row's value (2.5e-7 below eta), so an error of 1e-3 of it
    is 1e-3 of max|y|: the max-norm bound (1e-13) rejects it as well, and the test says so.  Where the max norm is blind for the
    forward family is the other end, a row whose scale itself is small: eta = 0, x = 2^-40 -- planted there too."""
    n, beta, eta = 1001, 48.0, 0.5
    x, df = pr.field(n, beta, eta), np.random.default_rng(1).standard_normal(n) + 3.0
    i = 500
    x[i], df[i] = _saturated_row(beta, eta, -1.0), 1e-12
    assert (1.0 - np.tanh(beta * (x[i] - eta)) ** 2) == pytest.approx(1e-6, rel=1e-6)
    w = {"dims": (n, 1, 1), "dof": 0}
    # chain
    ref, s = pr.chain(df, x, beta, eta, LD), pr.scale_chain(df, x, beta, eta)
    bad = pr.chain(df, x, beta, eta)
    assert rw.assert_rowwise(bad, ref, s, pr.C_CHAIN, dict(w, label="chain")) <= pr.C_CHAIN / 4
    bad[i] += 1e-3 * s[i]
    assert rw.rel(bad, ref.astype(np.float64)) <= 1e-12
    with pytest.raises(AssertionError, match="row %d" % i):
        rw.assert_rowwise(bad, ref, s, pr.C_CHAIN, dict(w, label="planted chain"))
    # forward, the same row
    ref, s = pr.H(x, beta, eta, LD), pr.scale_forward(x, beta, eta)
    bad = pr.H(x, beta, eta)
    assert s[i] == pytest.approx(1.0, rel=1e-6) and bad[i] == pytest.approx(2.5e-7, rel=1e-3)
    bad[i] += 1e-3 * s[i]
    assert rw.rel(bad, ref.astype(np.float64)) > 1e-13
    with pytest.raises(AssertionError, match="row %d" % i):
        rw.assert_rowwise(bad, ref, s, pr.C_FORWARD, dict(w, label="planted forward"))
    # forward, a row of small scale
    eta = 0.0
    x = pr.field(n, beta, eta)
    x[i] = 2.0 ** -40
    ref, s = pr.H(x, beta, eta, LD), pr.scale_forward(x, beta, eta)
    bad = pr.H(x, beta, eta)
    assert rw.assert_rowwise(bad, ref, s, pr.C_FORWARD, dict(w, label="forward")) <= pr.C_FORWARD / 4
    bad[i] += 1e-3 * s[i]
    assert rw.rel(bad, ref.astype(np.float64)) <= 1e-13
    with pytest.raises(AssertionError, match="row %d" % i):
        rw.assert_rowwise(bad, ref, s, pr.C_FORWARD, dict(w, label="planted forward, small scale"))
