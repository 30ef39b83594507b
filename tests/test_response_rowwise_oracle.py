"""The yardstick of tests/test_gpu_response_rowwise.py held on the CPU (tests/response_rowwise.py: the cases, the row scales, the
constants).  For every kernel family -- mass, stress stiffness, stress, body force, the multi-case response -- on every mesh,
design and field of that module:

  * the float64 restatement stays within a QUARTER of the row-wise bound against the 80-bit one (the condition
    tests/test_rowwise_oracle.py sets for the operators): the reference alone stays inside the bound for these inputs;
  * every row scale is finite and non-negative, and zero only where the restatement's result is exactly zero;
  * one planted error per family: the 80-bit result with ONE void-only row (the one of smallest positive scale) multiplied by
    1 + 1e-3 passes the older metric of that family's existing GPU test with that test's own bound -- the gap, on record -- and
    fails assert_rowwise with the new constant, which names the row; for the stress adjoint load also a whole incident element
    dropped at a void-only node.  MassMult (void / solid 6e-13), BodyLoad (6e-13) and the stress adjoint load (1e-12) are
    such.  GeomMult (Emax x^3: 1e-9) and dfdx (x^2: 1e-6) are NOT: there 1e-3 of a void-only row is 3.1e-14 and 1.3e-10 of the
    maximum, which the older bounds (7.4e-15, 1e-12) do see -- those tests hold the void rows to four and five digits.  For
    these two the test asserts that, and plants a second error sized from the older bound itself -- half of what that metric
    accepts on this row, relative errors of 1.2e-4 and 3.9e-6 -- which the older metric accepts and assert_rowwise rejects.

The achieved constants are printed; the largest of each is what stands beside the constant in tests/response_rowwise.py."""
import numpy as np
import pytest

from tests import response_rowwise as rr
from tests import rowwise as rw
from tests import stress_ref as stref

LD = np.longdouble
MEASURED = {}
CASES = [(m, k) for m in range(len(rr.MESHES)) for k in rr.DESIGNS]
PLANT_MESH = rr.MESHES[3]          # 20 x 12 x 8, hx != hy != hz
PLANT_DESIGN = "checker"


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def note(key, c):
    MEASURED[key] = max(MEASURED.get(key, 0.0), c)
    return c


def _scale_ok(c):
    s, ref = np.asarray(c["scale"]), np.asarray(c["ref"])
    assert np.isfinite(s).all() and (s >= 0).all(), c["where"]["label"]
    assert not ref[s == 0].any(), "%s: a row of scale 0 whose reference is not 0" % c["where"]["label"]


def _hold(key, c):
    _scale_ok(c)
    return note(key, rw.assert_rowwise(np.asarray(c["f64"], dtype=np.float64), c["ref"], c["scale"], c["c"] / 4, dict(c["where"], label="restatement " + c["where"]["label"])))


def _report(*keys):
    print("float64 restatement against the 80-bit one, largest achieved c so far (bound: a quarter of the constant): "
          + ", ".join("%s %.2f" % (k, MEASURED[k]) for k in keys if k in MEASURED))


@pytest.mark.parametrize("mi,kind", CASES)
def test_mass_restatement_within_a_quarter(mi, kind):
    for x_low in rr.X_LOWS:
        for c in rr.mass_cases(rr.MESHES[mi], kind, x_low):
            _hold("mass_" + c["op"], c)
    _report("mass_apply", "mass_sens")


@pytest.mark.parametrize("mi,kind", CASES)
def test_geom_restatement_within_a_quarter(mi, kind):
    for c in rr.geom_cases(rr.MESHES[mi], kind):
        _hold("geom_" + c["op"], c)
    _report("geom_apply", "geom_sens", "geom_adjoint")


@pytest.mark.parametrize("mi,kind", CASES)
def test_body_restatement_within_a_quarter(mi, kind):
    for x_low in rr.X_LOWS:
        for c in rr.body_cases(rr.MESHES[mi], kind, x_low):
            _hold("body_" + c["op"], c)
    _report("body_load", "body_sens")


@pytest.mark.parametrize("mi,kind", CASES)
def test_stress_restatement_within_a_quarter(mi, kind):
    """the float64 restatement inside the intervals built with a quarter of every constant; the figures are the fraction of
    that quarter-interval used (x constant / 4 = the achieved c)"""
    for c in rr.stress_cases(rr.MESHES[mi], kind, div=4):
        b = c["b"]
        f = stref.stress_ref(c["M"], c["dofs"], c["U"], c["x"], c["q"], c["P"], rr.EMAX, np.float64, relative=True)
        note("s", rr.assert_interval(f["s"], *b["s"], b["ref"]["s"], {"label": c["label"] + " s", "dims": c["ne"], "dof": 0}) * rr.C_S / 4)
        got = rr.check_stress(c, f["vm"], f["pnorm"], f["vm_max"], f["dpdx"], f["adj"])
        # vm, dpdx: the interval is the image of I_e AND the widening; the fraction times the constant is an upper figure
        note("vm", got["vm"] * rr.C_VM / 4), note("dpdx", got["dpdx"] * rr.C_POW / 4), note("adj", got["adj"]), note("pnorm", got["pnorm"] * rr.c_pnorm(1) / 4)
        s = b["adj_scale"]
        assert np.isfinite(s).all() and (s >= 0).all() and not np.asarray(b["ref"]["adj"])[s == 0].any(), c["label"]
        if c["label"].count("translation"):
            assert b["rigid"].any() and not b["rigid"].all()
    _report("s", "vm", "dpdx", "pnorm", "adj")


@pytest.mark.parametrize("mi,kind", CASES)
def test_response_restatement_within_a_quarter(orc, arb, mi, kind):
    for c in rr.response_cases(rr.MESHES[mi], kind):
        ne, h = c["ne"], c["h"]
        KE = orc.hex8_ke_box(h[0], h[1], h[2], rr.NU)
        nx, ny, nz = (n + 1 for n in ne)
        c.update(ref=rr.response_ref(arb, KE, ne, c["U"], c["V"], c["w"], c["x"]), f64=rr.response_f64(orc, KE, ne, c["U"], c["V"], c["w"], c["x"]),
                 scale=rr.scale_response(nx, ny, nz, KE, c["U"], c["V"], c["w"], c["x"]), c=rr.C_RESPONSE)
        _hold("response", c)
    _report("response")


# ---------------------------------------------------------------------------------------------------------------------
# planted errors: the older metric of each family's GPU test, restated with that test's own bound
# ---------------------------------------------------------------------------------------------------------------------
def _old_eigen_buckling(got, ref, f64):
    """tests/test_gpu_eigen.py, tests/test_gpu_buckling.py: max(16 x float64-to-80-bit distance, 64 eps) of the maximum"""
    return float(rw.rel(got, ref)), max(16 * float(rw.rel(f64, ref)), 64 * rr.EPS)


def _old_of_max(bound):
    return lambda got, ref, f64: (float(rw.rel(got, ref)), bound)


def _planted(name, c, old, candidates, old_sees_it=False):
    """old_sees_it: the families whose older bound does see 1e-3 of a void-only row (module docstring)"""
    bad, row = rr.plant(c["ref"], c["scale"], candidates)
    f64 = np.asarray(c["f64"], dtype=np.float64)
    got, bound = old(bad.astype(np.float64), c["ref"], f64)
    print("%s: row %d (scale / max scale = %.1e) x (1 + %g): older metric %.3e (its bound %.1e: %s)"
          % (name, row, c["scale"][row] / c["scale"].max(), rr.PLANT, got, bound, "accepted" if got <= bound else "seen"))
    # NOT a weakened check: the issue expects the older metric to accept 1e-3 on a void-only row for every family.  For GeomMult
    # and dfdx that cannot be met -- 1e-3 of such a row is 3.1e-14 and 1.3e-10 of the maximum, above the older bounds -- so
    # old_sees_it=True asserts that fact, the row-wise bound must STILL reject the 1e-3 error, and then an error the older
    # metric does accept (half its bound on this row) is planted and must be rejected too.  old_sees_it=False is the issue's
    # outcome to the letter.
    assert (got > bound) == old_sees_it, "the older metric %s the planted error" % ("sees" if got > bound else "does not see")
    if old_sees_it:
        with pytest.raises(AssertionError, match=r"worst: row %d," % row):
            rw.assert_rowwise(bad.astype(np.float64), c["ref"], c["scale"], c["c"], c["where"])
        delta = 0.5 * bound * float(np.abs(c["ref"]).max() / abs(c["ref"][row]))        # half of what the older metric accepts here
        assert delta < rr.PLANT
        bad = np.array(c["ref"], dtype=LD)
        bad[row] = bad[row] * (1 + LD(delta))
        got, bound = old(bad.astype(np.float64), c["ref"], f64)
        print("%s: row %d x (1 + %.2e): older metric %.3e (its bound %.1e: accepted)" % (name, row, delta, got, bound))
        assert got <= bound
    with pytest.raises(AssertionError, match=r"worst: row %d," % row) as e:
        rw.assert_rowwise(bad.astype(np.float64), c["ref"], c["scale"], c["c"], c["where"])
    print("    row-wise, c = %g: rejected (achieved c %.3g) -- %s" % (c["c"], rw.achieved(bad.astype(np.float64), c["ref"], c["scale"]), str(e.value)[:260]))
    rw.assert_rowwise(np.asarray(c["f64"], dtype=np.float64), c["ref"], c["scale"], c["c"], c["where"])     # (the unplanted result passes)


def _void_elems(x):
    return np.asarray(x) != 1.0


def test_planted_error_mass():
    ne, _ = PLANT_MESH
    c = next(rr.mass_cases(PLANT_MESH, PLANT_DESIGN, 0.1))
    _planted("MassMult", c, _old_eigen_buckling, rr.void_only_nodes(ne, c["x"]))


def test_planted_error_stress_stiffness():
    ne, _ = PLANT_MESH
    c = next(rr.geom_cases(PLANT_MESH, PLANT_DESIGN))
    _planted("GeomMult", c, _old_eigen_buckling, rr.void_only_nodes(ne, c["x"]), old_sees_it=True)


def test_planted_error_body_force():
    ne, _ = PLANT_MESH
    c = next(rr.body_cases(PLANT_MESH, PLANT_DESIGN, 0.1))
    _planted("BodyLoad", c, _old_of_max(1e-13), rr.void_only_nodes(ne, c["x"]))


def test_planted_error_response(orc, arb):
    c = next(rr.response_cases(PLANT_MESH, PLANT_DESIGN))
    ne, h = c["ne"], c["h"]
    KE = orc.hex8_ke_box(h[0], h[1], h[2], rr.NU)
    c.update(ref=rr.response_ref(arb, KE, ne, c["U"], c["V"], c["w"], c["x"]), f64=rr.response_f64(orc, KE, ne, c["U"], c["V"], c["w"], c["x"]),
             scale=rr.scale_response(ne[0] + 1, ne[1] + 1, ne[2] + 1, KE, c["U"], c["V"], c["w"], c["x"]), c=rr.C_RESPONSE)
    _planted("Response dfdx", c, _old_of_max(1e-12), _void_elems(c["x"]), old_sees_it=True)


def test_planted_error_stress_adjoint_load():
    """(q, P) = (0.5, 8): the weight of a void element is 1e-12 of a solid one's"""
    ne, _ = PLANT_MESH
    c = next(rr.stress_cases(PLANT_MESH, PLANT_DESIGN, qps=[(0.5, 8.0)]))
    b = c["b"]
    f = stref.stress_ref(c["M"], c["dofs"], c["U"], c["x"], c["q"], c["P"], rr.EMAX, np.float64, relative=True)
    case = dict(ref=b["ref"]["adj"], f64=f["adj"], scale=b["adj_scale"], c=rr.C_ADJ, where={"dims": tuple(n + 1 for n in ne), "label": c["label"] + " adj_rhs"})
    void = rr.void_only_nodes(ne, c["x"])
    _planted("Stress adj_rhs", case, _old_of_max(1e-11), void)
    # a whole incident element dropped at a void-only node: the node of smallest scale, its first incident element
    ok = void & (case["scale"] > 0)
    row = int(np.flatnonzero(ok)[np.argmin(case["scale"][ok])])
    e, col = (int(v[0]) for v in np.nonzero(c["dofs"] == row))
    ue = c["U"].astype(LD)[c["dofs"][e]]
    ue = ue - np.tile(ue[:3], 8)
    bad = np.array(case["ref"], dtype=LD)
    bad[row] -= b["c"][e] * (ue @ c["M"].astype(LD))[col]
    got, bound = _old_of_max(1e-11)(bad.astype(np.float64), case["ref"], None)
    print("Stress adj_rhs: element %d dropped at row %d: older metric %.3e (its bound %.1e: accepted)" % (e, row, got, bound))
    assert got <= bound and bad[row] != case["ref"][row]
    with pytest.raises(AssertionError, match=r"worst: row %d," % row) as err:
        rw.assert_rowwise(bad.astype(np.float64), case["ref"], case["scale"], case["c"], case["where"])
    print("    row-wise, c = %g: rejected -- %s" % (case["c"], str(err.value)[:260]))
