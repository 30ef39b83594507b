"""The numpy restatement of design-variable linking (tests/link_ref.py) held to the properties the maps must have,
and to planted errors it must notice -- the device kernels are then held to it bit for bit (tests/test_gpu_link.py).  CPU only."""
import numpy as np
import pytest

from tests import link_ref as lr

SMALL = [b for b in lr.BOXES if b[0] * b[1] * b[2] <= 2000]
CASES = [(ne, spec) for ne in SMALL for spec in lr.specs_for(ne)]
EPS = 2.0 ** -53


@pytest.mark.parametrize("ne,spec", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else lr.spec_name(v))
def test_maps_are_consistent(ne, spec):
    """pick o expand is the identity; expand o pick is the identity on linked fields; the orbit sizes sum to n; expand's image is
    constant on orbits; the reduced counts are those of the table"""
    n = ne[0] * ne[1] * ne[2]
    nr = lr.reduced_counts(spec, ne)
    nred = nr[0] * nr[1] * nr[2]
    rng = np.random.default_rng(n + nred)
    red = rng.standard_normal(nred)
    full = lr.expand(spec, ne, red)
    assert full.shape == (n,) and np.array_equal(lr.pick(spec, ne, full), red)
    assert np.array_equal(lr.expand(spec, ne, lr.pick(spec, ne, full)), full)
    sizes = lr.orbit_sizes(spec, ne)
    assert sizes.shape == (nred,) and sizes.sum() == n and sizes.min() >= 1
    assert np.array_equal(np.bincount(lr.reduced_map(spec, ne), minlength=nred), sizes)
    assert np.array_equal(lr.fold(spec, ne, np.ones(n)), sizes.astype(np.float64))


@pytest.mark.parametrize("ne,spec", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else lr.spec_name(v))
def test_fold_is_the_transpose_of_expand(ne, spec):
    """<expand r, w> - <r, fold w> = 0 exactly.  In floating point, with S the largest orbit and entries of r, w in [-1, 1]: the
    80-bit fold is the exact sum but for (S - 1) roundings of 2^-64 each, which are far below the float64 terms; the float64 fold
    of an orbit carries at most (S - 1) eps S max|w| (S - 1 adds, partial sums at most S in size), so
      |fold64 - fold80|_j <= (S - 1) S eps,
    and the two inner products, evaluated in 80-bit arithmetic on the float64 fold, differ by at most sum_j |r_j| (S - 1) S eps
    <= nred (S - 1) S eps, plus the 80-bit roundings of the two long sums, at most 2 n 2^-64 n -- added to the bound."""
    n = ne[0] * ne[1] * ne[2]
    rng = np.random.default_rng(7 * n + 1)
    nr = lr.reduced_counts(spec, ne)
    nred = nr[0] * nr[1] * nr[2]
    r, w = rng.uniform(-1, 1, nred), rng.uniform(-1, 1, n)
    S = int(lr.orbit_sizes(spec, ne).max())
    f64, f80 = lr.fold(spec, ne, w), lr.fold(spec, ne, w, np.longdouble)
    assert f64.dtype == np.float64 and f80.dtype == np.longdouble
    per_entry = (S - 1) * S * EPS
    assert float(np.abs(f64.astype(np.longdouble) - f80).max()) <= per_entry
    lhs = (lr.expand(spec, ne, r).astype(np.longdouble) * w.astype(np.longdouble)).sum()
    rhs = (r.astype(np.longdouble) * f64.astype(np.longdouble)).sum()
    bound = nred * per_entry + 2.0 * n * n * 2.0 ** -64
    print("%s %s: S = %d, |<Er, w> - <r, Fw>| = %.3e, bound %.3e" % (ne, lr.spec_name(spec), S, abs(float(lhs - rhs)), bound))
    assert abs(float(lhs - rhs)) <= bound
    # against the 80-bit fold the two sides agree to the 80-bit roundings alone
    rhs80 = (r.astype(np.longdouble) * f80).sum()
    assert abs(float(lhs - rhs80)) <= 2.0 * n * n * 2.0 ** -64 + nred * S * 2.0 ** -64


def test_odd_mirror_has_single_member_centre_orbits():
    ne, spec = (5, 4, 3), (lr.MIRROR, lr.NONE, lr.MIRROR)
    sizes = lr.orbit_sizes(spec, ne).reshape(2, 4, 3)      # (nr_z, nr_y, nr_x)
    assert lr.reduced_counts(spec, ne) == (3, 4, 2)
    assert (sizes[:, :, :2] == np.array([4, 2])[:, None, None]).all()     # z: index 0 pairs layers 0 and 2, index 1 is the centre
    assert (sizes[0, :, 2] == 2).all() and (sizes[1, :, 2] == 1).all()     # the x centre column: 2 with the z pair, 1 at the centre
    mem, ok = lr.preimages(lr.MIRROR, 5)
    assert mem[ok].tolist() == [0, 4, 1, 3, 2] and ok.tolist() == [[True, True], [True, True], [True, False]]
    mem, ok = lr.preimages(lr.repeat(3), 6)
    assert mem.tolist() == [[0, 2, 4], [1, 3, 5]] and ok.all()
    mem, ok = lr.preimages(lr.EXTRUDE, 4)
    assert mem.tolist() == [[0, 1, 2, 3]]
    assert np.array_equal(lr.reduced_index(lr.MIRROR, 6), [0, 1, 2, 2, 1, 0])


def test_negative_zero_orbits_stay_negative_zero():
    ne, spec = (6, 4, 2), (lr.MIRROR, lr.repeat(2), lr.EXTRUDE)
    f = lr.negative_zero_field(spec, ne, 3)
    out = lr.fold(spec, ne, f)
    assert np.signbit(out[0]) and out[0] == 0.0 and np.signbit(out[-1]) and out[-1] == 0.0


def test_planted_errors_are_caught():
    """a reversed summation order, a dropped centre plane, an off-by-one cell period: each changes the result on the test fields"""
    ne = (12, 6, 4)
    n = 12 * 6 * 4
    f = lr.order_field(n, 11)
    # reversed order: the same members, other bits
    for spec in ((lr.EXTRUDE, lr.NONE, lr.NONE), (lr.NONE, lr.repeat(3), lr.NONE), (lr.MIRROR, lr.repeat(2), lr.EXTRUDE)):
        a, b = lr.fold(spec, ne, f), lr.fold(spec, ne, f, reverse=True)
        assert not np.array_equal(a, b), lr.spec_name(spec)
        assert float(np.abs(a - b).max()) <= 1e-9 * float(np.abs(f).max())     # (the same sum but for rounding)
    # a dropped centre plane: mirror on an odd axis with the centre's orbit emptied
    ne5, spec = (5, 4, 3), (lr.MIRROR, lr.NONE, lr.NONE)
    g = lr.order_field(60, 5) + 3.0
    good = lr.fold(spec, ne5, g).reshape(3, 4, 3)
    g3 = g.reshape(3, 4, 5)
    dropped = np.stack([g3[:, :, 0] + g3[:, :, 4], g3[:, :, 1] + g3[:, :, 3], np.zeros((3, 4))], axis=-1)
    assert np.array_equal(good[:, :, :2], dropped[:, :, :2]) and not np.array_equal(good[:, :, 2], dropped[:, :, 2])
    assert np.array_equal(good[:, :, 2], g3[:, :, 2])
    # an off-by-one period: repeat:3 on 12 elements has period 4; period 3 or 5 lands elsewhere
    h = np.arange(12, dtype=np.float64) ** 2
    good = lr.fold((lr.repeat(3), lr.NONE, lr.NONE), (12, 1, 1), h)
    assert np.array_equal(good, [h[I] + h[I + 4] + h[I + 8] for I in range(4)])
    for P in (3, 5):
        wrong = [h[I] + h[(I + P) % 12] + h[(I + 2 * P) % 12] for I in range(4)]
        assert not np.array_equal(good, wrong)
    assert np.array_equal(lr.expand((lr.repeat(3), lr.NONE, lr.NONE), (12, 1, 1), np.arange(4.0)), np.tile(np.arange(4.0), 3))
