"""Design-variable linking restated in numpy: helpers of the link tests, not a test.

Per axis a mode -- ("none",), ("mirror",), ("repeat", c), ("extrude",) -- gives the reduced index r(i) and the preimage of a reduced
index, ascending.  A spec is a 3-tuple of such modes (x, y, z); ne the element counts (x, y, z); fields are flat, x fastest.
  expand(spec, ne, red)        full[e] = red[r(e)]
  pick(spec, ne, full)         red[j] = full[first member of orbit(j)]
  fold(spec, ne, full, dtype)  red[j] = the sum over orbit(j) in the canonical order: ascending natural element order (z outer, then
                               y, then x), the accumulator started with the first member's value.  Vectorised over the reduced
                               variables, one add per orbit position; positions an orbit does not have (a mirror's centre) are
                               skipped for it.  dtype float64 restates the kernels; np.longdouble is the 80-bit witness."""
import itertools

import numpy as np

NONE, MIRROR, EXTRUDE = ("none",), ("mirror",), ("extrude",)


def repeat(c):
    return ("repeat", c)


def nr_of(mode, ne):
    kind = mode[0]
    if kind == "none":
        return ne
    if kind == "mirror":
        return (ne + 1) // 2
    if kind == "repeat":
        assert mode[1] >= 2 and ne % mode[1] == 0
        return ne // mode[1]
    assert kind == "extrude"
    return 1


def reduced_index(mode, ne):
    """r(i) for i < ne"""
    i = np.arange(ne)
    kind = mode[0]
    if kind == "none":
        return i
    if kind == "mirror":
        return np.minimum(i, ne - 1 - i)
    if kind == "repeat":
        return i % (ne // mode[1])
    return np.zeros(ne, dtype=np.int64)


def preimages(mode, ne):
    """-> (members [nr, cmax], valid [nr, cmax]): row I holds the preimage of I ascending, padded where it is shorter"""
    r = reduced_index(mode, ne)
    nr = nr_of(mode, ne)
    lists = [np.nonzero(r == I)[0] for I in range(nr)]
    cmax = max(len(l) for l in lists)
    mem, ok = np.zeros((nr, cmax), dtype=np.int64), np.zeros((nr, cmax), dtype=bool)
    for I, l in enumerate(lists):
        mem[I, :len(l)], ok[I, :len(l)] = l, True
    return mem, ok


def reduced_counts(spec, ne):
    return tuple(nr_of(m, n) for m, n in zip(spec, ne))


def reduced_map(spec, ne):
    """r(e) for every element, flat"""
    rx, ry, rz = (reduced_index(m, n) for m, n in zip(spec, ne))
    nrx, nry, _ = reduced_counts(spec, ne)
    return ((rz[:, None, None] * nry + ry[None, :, None]) * nrx + rx[None, None, :]).reshape(-1)


def expand(spec, ne, red):
    return np.asarray(red)[reduced_map(spec, ne)]


def orbit_positions(spec, ne):
    """yields (element index per reduced variable [nred], valid [nred]) for the orbit positions in canonical order"""
    (mx, okx), (my, oky), (mz, okz) = (preimages(m, n) for m, n in zip(spec, ne))
    ex, ey, _ = ne
    for kz, ky, kx in itertools.product(range(mz.shape[1]), range(my.shape[1]), range(mx.shape[1])):
        e = (mz[:, kz][:, None, None] * ey + my[:, ky][None, :, None]) * ex + mx[:, kx][None, None, :]
        ok = okz[:, kz][:, None, None] & oky[:, ky][None, :, None] & okx[:, kx][None, None, :]
        yield e.reshape(-1), ok.reshape(-1)


def pick(spec, ne, full):
    e, ok = next(orbit_positions(spec, ne))
    assert ok.all()
    return np.asarray(full)[e]


def orbit_sizes(spec, ne):
    return sum(ok.astype(np.int64) for _, ok in orbit_positions(spec, ne))


def fold(spec, ne, full, dtype=np.float64, reverse=False):
    """reverse: the planted error of tests/test_link_oracle.py, the same members summed in descending order"""
    full = np.asarray(full).astype(dtype)
    steps = list(orbit_positions(spec, ne))
    if reverse:
        steps = steps[::-1]
    acc, started = np.zeros(steps[0][0].size, dtype=dtype), np.zeros(steps[0][0].size, dtype=bool)
    for e, ok in steps:
        val = full[e]
        first = ok & ~started
        more = ok & started
        acc[first] = val[first]
        acc[more] = acc[more] + val[more]
        started |= ok
    assert started.all()
    return acc


# ---- the cases ----
BOXES = [(1, 1, 1), (5, 4, 3), (6, 4, 2), (63, 1, 1), (64, 1, 1), (65, 2, 1), (129, 3, 2), (257, 1, 1), (12, 6, 4), (96, 80, 72)]
BIG_MIRROR = ((192, 80, 72), (MIRROR, NONE, NONE))


def specs_for(ne):
    """every single-axis mode the box admits (repeat with 2 and 3 cells where they divide), the three-axis combination x:mirror
    y:repeat:2 z:extrude where 2 divides ey, and all none"""
    out = [(NONE, NONE, NONE)]
    for a in range(3):
        modes = [MIRROR, EXTRUDE] + [repeat(c) for c in (2, 3) if ne[a] % c == 0]
        for m in modes:
            s = [NONE, NONE, NONE]
            s[a] = m
            out.append(tuple(s))
    if ne[1] % 2 == 0:
        out.append((MIRROR, repeat(2), EXTRUDE))
    return out


def spec_dict(spec):
    """the spec as api.parse_link takes it"""
    return {a: (m[0] if len(m) == 1 else m) for a, m in zip("xyz", spec) if m[0] != "none"}


def spec_name(spec):
    return " ".join("%s:%s" % (a, ":".join(map(str, m))) for a, m in zip("xyz", spec) if m[0] != "none") or "none"


def order_field(n, seed):
    """finite values that make the summation order visible: magnitudes spread over 30 binades, both signs, and exact +0.0 and
    -0.0 among them"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-15, 15, n) * rng.choice([-1.0, 1.0], n)
    z = rng.random(n)
    f[z < 0.05] = 0.0
    f[(z >= 0.05) & (z < 0.10)] = -0.0
    return f


def design_field(n, seed):
    """a 0/1 design"""
    return (np.random.default_rng(seed).random(n) < 0.4).astype(np.float64)


def negative_zero_field(spec, ne, seed):
    """order_field with the orbit of the last reduced variable (and of the first) entirely -0.0"""
    n = ne[0] * ne[1] * ne[2]
    f = order_field(n, seed)
    r = reduced_map(spec, ne)
    f[(r == r.max()) | (r == 0)] = -0.0
    return f
