"""The response kernels -- mass (mass.h), stress stiffness (geomstiff.h), von Mises stress (stress.h), body force (bodyforce.h)
and the fused multi-case response (response.h) -- held ROW BY ROW on 0/1 designs against their 80-bit restatements, and their
one-workgroup reduction tails on more than 256 workgroups.  tests/response_rowwise.py: why, the row scales, the stress
intervals, the cases, the constants and the operation counts behind them; tests/test_response_rowwise_oracle.py holds the float64
restatements to a quarter of every bound on the CPU.

One test function per family, parametrised over mesh x design (five meshes, the five 0/1 generators of tests/rowwise.py with
x in {1e-3, 1} and "blocks" with exact zeros), the fields looped inside.  Everything runs in this process: none of these
kernels latches a switch.

Bounds (c, in units of eps x row scale) and the worst c the kernels ACHIEVED on the MI355X (recorded for the reader; the bounds
come from the operation counts and the restatements' own CPU figures, not from these):

    kernel                                                     bound   achieved
    MassMult / MassSensitivity (x_low 0.1 and 0)             64 / 256   6.6 / 3.1
    GeomMult / GeomSensitivity / GeomAdjointRHS         128 / 128 / 128   0.82 / 1.2 / 3.0
    BodyLoad (alone, with a base, in place) / BodySensitivity   128 / 64   8.4 / 4.0
    Response dfdx, 1 / 3 / 8 cases, quadratic and bilinear         64   0.43
    Stress, as the used fraction of each interval (<= 1): vm / dpdx / pnorm   0.0039 / 0.0048 / 0.0008
    Stress adj_rhs                                                 32   1.3
        (the fractions are small because the intervals come from a worst-case count; on the translation state they are wide by
        construction and say little -- tests/response_rowwise.py: stress_bounds -- the rows are held by the random state)
    reductions on 48 x 40 x 36 (270 workgroups), in eps x sum |terms|:
        Response f_case / volume                              32 / 34   2.9 / 1.5
        Stress pnorm (fraction of its interval), vm row-wise        -   0.0013, 0.0063
        LocalVolume mean / p-norm (relative to itself)        32 / 32   17.5 / 8.4
"""
import math

import numpy as np
import pytest

from tests import eigen_ref as eref
from tests import localvol_ref as lref
from tests import response_rowwise as rr
from tests import rowwise as rw

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = [(m, k) for m in range(len(rr.MESHES)) for k in rr.DESIGNS]
ACHIEVED = {}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    return tp


@pytest.fixture(scope="module")
def arb(orc):
    from oracle import arbiter
    arbiter.lib()
    return arbiter


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).cuda()


def _note(key, got, bound):
    ACHIEVED[key] = (max(ACHIEVED.get(key, (0.0, 0))[0], got), bound)
    return got


def _show(family):
    print("ACHIEVED", family, {k: "%.3g of %g" % v for k, v in ACHIEVED.items() if k.startswith(family)})


_CTX = {}


def _ctx(tp, mesh, nlvls=1):
    """per mesh, made once and left alone: the grid and a solver object with the cantilever's supports"""
    if mesh not in _CTX:
        ne, h = mesh
        grid = tp.Grid(ne[0] + 1, ne[1] + 1, ne[2] + 1, h)
        le = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=nlvls, nu=rr.NU))
        le.SetUpLoadAndBC()
        assert np.array_equal(le.N.cpu().numpy(), eref.cantilever_N(*ne))
        _CTX[mesh] = (grid, le)
    return _CTX[mesh]


def _hold(family, c, got):
    a = rw.assert_rowwise(got, c["ref"], c["scale"], c["c"], c["where"])
    print("%-96s achieved c %8.3f   bound %g" % (c["where"]["label"], a, c["c"]))
    return _note("%s %s" % (family, c["op"]), a, c["c"])


# ---- 1
@pytest.mark.parametrize("mi,kind", CASES)
def test_mass(tp, mi, kind):
    g, le = _ctx(tp, rr.MESHES[mi])
    for x_low in rr.X_LOWS:
        xd = None
        for c in rr.mass_cases(rr.MESHES[mi], kind, x_low):
            if xd is None:
                xd = _dev(c["x"])
                le.MassAssemble(xd, rr.RHO0, x_low)
            if c["op"] == "apply":
                y = g.node_vec(3)
                y.fill_(7.0)                          # (every owned entry is written)
                le.MassMult(_dev(c["u"]), y)
                _hold("mass", c, y.cpu().numpy())
            else:
                d = _dev(c["pre"])
                le.MassSensitivity([_dev(v) for v in c["V"]], c["w"], xd, c["sc"], d)
                _hold("mass", c, d.cpu().numpy())
    _show("mass")


# ---- 2
@pytest.mark.parametrize("mi,kind", CASES)
def test_stress_stiffness(tp, mi, kind):
    g, le = _ctx(tp, rr.MESHES[mi])
    xd, state = None, None
    for c in rr.geom_cases(rr.MESHES[mi], kind):
        if xd is None:
            xd = _dev(c["x"])
        if c["op"] != "adjoint" and c["U"] is not state:
            state, Ud = c["U"], _dev(c["U"])
            le.GeomAssemble(xd, rr.EMAX, rr.PENAL, U=Ud)
        if c["op"] == "apply":
            y = g.node_vec(3)
            y.fill_(7.0)
            le.GeomMult(_dev(c["u"]), y)
            _hold("geom", c, y.cpu().numpy())
        elif c["op"] == "sens":
            d = _dev(c["pre"])
            le.GeomSensitivity([_dev(v) for v in c["V"]], c["w"], xd, Ud, rr.EMAX, rr.PENAL, c["sc"], d)
            _hold("geom", c, d.cpu().numpy())
        else:
            out = g.node_vec(3)
            out.fill_(7.0)
            le.GeomAdjointRHS([_dev(v) for v in c["V"]], c["w"], xd, rr.EMAX, rr.PENAL, c["sc"], out)
            _hold("geom", c, out.cpu().numpy())
    _show("geom")


# ---- 3
def _stress_call(g, le, c):
    vm, dpdx, adj = g.elem_vec(7.0), g.elem_vec(7.0), g.node_vec(3)
    adj.fill_(7.0)
    pn, mx = le.Stress(_dev(c["x"]), rr.EMAX, c["q"], c["P"], U=_dev(c["U"]), vm=vm, dpdx=dpdx, adj_rhs=adj)
    return vm.cpu().numpy(), pn, mx, dpdx.cpu().numpy(), adj.cpu().numpy()


@pytest.mark.parametrize("mi,kind", CASES)
def test_stress(tp, mi, kind):
    g, le = _ctx(tp, rr.MESHES[mi])
    for c in rr.stress_cases(rr.MESHES[mi], kind):
        vm, pn, mx, dpdx, adj = _stress_call(g, le, c)
        got = rr.check_stress(c, vm, pn, mx, dpdx, adj)
        print("%-64s fraction of the interval used: vm %.3f dpdx %.3f pnorm %.3f;  adj_rhs achieved c %.3f, bound %g"
              % (c["label"], got["vm"], got["dpdx"], got["pnorm"], got["adj"], rr.C_ADJ))
        for k in ("vm", "dpdx", "pnorm"):
            _note("stress %s (fraction)" % k, got[k], 1)
        _note("stress adj_rhs", got["adj"], rr.C_ADJ)
    _show("stress")


# ---- 4
@pytest.mark.parametrize("mi,kind", CASES)
def test_body_force(tp, mi, kind):
    import torch
    g, le = _ctx(tp, rr.MESHES[mi])
    try:
        for x_low in rr.X_LOWS:
            le.SetBodyForce(rr.BVEC, x_low)
            for c in rr.body_cases(rr.MESHES[mi], kind, x_low):
                xd = _dev(c["x"])
                if c["op"] == "load":
                    out = g.node_vec(3)
                    out.fill_(7.0)
                    bd = None if c["base"] is None else _dev(c["base"])
                    le.BodyLoad(xd, out, base=bd)
                    _hold("body", c, out.cpu().numpy())
                    if bd is not None:
                        assert np.array_equal(bd.cpu().numpy(), c["base"]), "the base array was written to"
                        inpl = bd.clone()
                        le.BodyLoad(xd, inpl, base=inpl)
                        assert torch.equal(inpl, out), "%s: rhs == rhs_base gives other bits" % c["where"]["label"]
                else:
                    d = _dev(c["pre"])
                    le.BodySensitivity([_dev(v) for v in c["V"]], c["w"], xd, c["sc"], d)
                    _hold("body", c, d.cpu().numpy())
    finally:
        le.SetBodyForce(None)
    _show("body")


# ---- 5
@pytest.mark.parametrize("mi,kind", CASES)
def test_multi_case_response(tp, arb, mi, kind):
    g, le = _ctx(tp, rr.MESHES[mi])
    KE = le.KE.copy()
    for c in rr.response_cases(rr.MESHES[mi], kind):
        ne = c["ne"]
        assert len(c["U"]) <= tp.lib.MAX_CASES
        df = g.elem_vec(7.0)
        Vd = None if all(v is None for v in c["V"]) else [None if v is None else _dev(v) for v in c["V"]]
        le.Response([_dev(u) for u in c["U"]], Vd, c["w"], _dev(c["x"]), rr.EMIN_R, rr.EMAX_R, rr.PENAL, 0.12, df, sums=False)
        c.update(op="dfdx", ref=rr.response_ref(arb, KE, ne, c["U"], c["V"], c["w"], c["x"]), c=rr.C_RESPONSE,
                 scale=rr.scale_response(ne[0] + 1, ne[1] + 1, ne[2] + 1, KE, c["U"], c["V"], c["w"], c["x"]))
        _hold("response", c, df.cpu().numpy())
    _show("response")


def test_the_largest_case_count_is_the_librarys(tp):
    assert tp.lib.MAX_CASES == len(rr.CASE_WEIGHTS) == 8


# ---------------------------------------------------------------------------------------------------------------------
# the reductions beyond one trip: 48 x 40 x 36 elements = 270 workgroups of 256
# ---------------------------------------------------------------------------------------------------------------------
NWG = 270


def _big(tp):
    ne, _ = rr.REDUCTION_MESH
    assert (ne[0] * ne[1] * ne[2] + 255) // 256 == NWG > 256
    return _ctx(tp, rr.REDUCTION_MESH, nlvls=3)


def _ramp_top(ne, U):
    """the state scaled up plane by plane (4, 16, 64, 256) on the four highest node planes: the largest vm lies in the last
    element layer"""
    V = U.reshape(ne[2] + 1, ne[1] + 1, ne[0] + 1, 3).copy()
    for m, f in enumerate((4.0, 16.0, 64.0, 256.0)):
        V[ne[2] - 3 + m] *= f
    return V.reshape(-1)


@pytest.mark.parametrize("kind", rr.REDUCTION_DESIGNS)
def test_stress_reduction_beyond_one_trip(tp, kind):
    """pnorm, vm_max and vm with the largest vm in a workgroup beyond the 256th: the second trip of k_sum_max_final's loop"""
    g, le = _big(tp)
    ne, _ = rr.REDUCTION_MESH
    U = _ramp_top(ne, rr.fields(ne, 31, 1)[0])
    (c,) = rr.stress_cases(rr.REDUCTION_MESH, kind, nwg=NWG, qps=[(0.5, 8.0)], states={"ramp": U})
    r = c["b"]["ref"]
    e = int(np.argmax(r["vm"]))
    print("%s: the reference's largest vm %.6e in element %d = workgroup %d; the largest below workgroup 257: %.6e"
          % (c["label"], float(r["vm"][e]), e, e // 256, float(r["vm"][:257 * 256].max())))
    assert e // 256 > 256 and float(r["vm"][:257 * 256].max()) < 0.9 * float(r["vm"][e])
    vm, pn, mx, dpdx, adj = _stress_call(g, le, c)
    got = rr.check_stress(c, vm, pn, mx, dpdx, adj)
    assert mx == vm.max() and int(np.argmax(vm)) // 256 > 256
    print("%s: fraction of the interval used: vm %.3f dpdx %.3f pnorm %.3f (c_pnorm %d);  adj_rhs achieved c %.3f"
          % (c["label"], got["vm"], got["dpdx"], got["pnorm"], rr.c_pnorm(NWG), got["adj"]))
    _note("reduction stress pnorm (fraction)", got["pnorm"], 1), _note("reduction stress vm (fraction)", got["vm"], 1)
    _show("reduction stress")


@pytest.mark.parametrize("kind", rr.REDUCTION_DESIGNS)
def test_response_reduction_beyond_one_trip(tp, kind):
    """3 cases: f_case and the volume against the 80-bit sums of the device's own per-element terms E_e v^T KE u -- the
    device's u^T KE u of a case is its single-case dfdx divided by -p x^(p-1) (Emax - Emin), three roundings away; E_e and the
    product four more.  Bound: (dot_chain(0, 270) + 8 -> 32) eps sum |terms|; the volume's terms are the densities themselves
    (volfrac = 0 in the call: gx is the volume over n, nothing is subtracted from it)"""
    g, le = _big(tp)
    ne, _ = rr.REDUCTION_MESH
    x = rr.design(kind, ne)
    xd, xl = _dev(x), x.astype(LD)
    Us = [_dev(u) for u in rr.fields(ne, 41, 3)]
    fx, gx, fc = le.Response(Us, None, rr.CASE_WEIGHTS[:3], xd, rr.EMIN_R, rr.EMAX_R, rr.PENAL, 0.0)      # volfrac 0: gx = volume / n
    c = rw.pow2(rw.dot_chain(0, NWG) + 8)
    E = LD(rr.EMIN_R) + xl ** 3 * (LD(rr.EMAX_R) - LD(rr.EMIN_R))
    for l in range(3):
        df = g.elem_vec()
        le.Response([Us[l]], None, None, xd, rr.EMIN_R, rr.EMAX_R, rr.PENAL, 0.12, df, sums=False)
        terms = E * (df.cpu().numpy().astype(LD) / (-LD(rr.PENAL) * xl ** 2 * (LD(rr.EMAX_R) - LD(rr.EMIN_R))))
        err = float(abs(LD(fc[l]) - terms.sum()) / (rr.EPS * np.abs(terms).sum()))
        print("%s case %d: f %.17g, |f - sum| = %.3g eps sum|terms|, bound %d" % (kind, l, fc[l], err, c))
        assert _note("reduction response f_case", err, c) <= c
    vol = gx * x.size
    err = float(abs(LD(vol) - xl.sum()) / (rr.EPS * xl.sum()))
    print("%s volume: %.17g, |v - sum| = %.3g eps sum x, bound %d (+ 2: the division by n, and undone)" % (kind, vol, err, c))
    assert _note("reduction response volume", err, c + 2) <= c + 2
    _show("reduction response")


@pytest.mark.parametrize("kind", rr.REDUCTION_DESIGNS + ("top_solid",))
def test_localvol_reduction_beyond_one_trip(tp, kind):
    """8 workgroups per layer x 36 layers = 288 partials: the maximum's strided loop of k_localvol_reduce takes a second trip.
    Sums of positive terms, relative to themselves: the ball mean, the additions of the ball's 19 taps and the division (20)
    -> 32; the p-norm the mean's 20, then pow, the workgroup's and the layer's sums and the 36 layers in turn (2 + 21 + 36 =
    59) under the p-th root (/ p), the root and the division by n (2): 20 + ceil(59 / p) + 2 = 26 -> 32 for p = 16.  The
    maximum is the largest of the device's own means.  Only the MAXIMUM's strided loop of k_localvol_reduce (b < nb = 288) takes
    a second trip here; the sum's loop runs per layer over b < bpl = 8 partials (indexed [layer][block], unlike
    k_sum_max_final's [value][block]) and would need more than 65536 elements in ONE layer for a second trip, which no mesh of
    a few seconds' reference allows: the sum is held here for its 36 layers in turn, not for a second trip.  A third design beside the issue's two, "top_solid" -- one solid element
    in the LAST layer -- puts the largest mean into partial 280 and up, where only the loop's second trip finds it."""
    ne, h = rr.REDUCTION_MESH
    g, _ = _big(tp)
    R, p, alpha = 0.05, 16.0, 0.6
    assert lref.stencil_width(ne, h, R) == 1 and ((ne[0] * ne[1] + 255) // 256) * ne[2] > 256
    if kind == "top_solid":
        x = np.full(ne[0] * ne[1] * ne[2], rw.XMIN)
        x[-(ne[0] * ne[1]) // 2] = 1.0
    else:
        x = rr.design(kind, ne)
    ref = lref.reference(x, ne, h, R, alpha, p)
    lv = tp.LocalVolume(g, R)
    try:
        rb = g.elem_vec()
        gg, pn, mx = lv.Constraint(_dev(x), alpha, p, rhobar=rb)
        rbh = rb.cpu().numpy()
    finally:
        lv.close()
    taps = len(lref.offsets(ne, h, R))
    c_rb, c_pn = rw.pow2(taps + 1), rw.pow2(taps + 1 + math.ceil((2 + 21 + ne[2]) / p) + 2)
    a = rw.assert_rowwise(rbh, ref["rb"], np.asarray(ref["rb"], dtype=np.float64), c_rb, {"label": "localvol mean %s" % kind, "dims": ne, "dof": 0})
    e_pn = float(abs(LD(pn) - ref["pn"]) / ref["pn"] / rr.EPS)
    print("%s: ball mean achieved c %.3f (bound %d); |pn / pn_ref - 1| = %.3g eps (bound %d); max %.17g, max of the device's means %.17g"
          % (kind, a, c_rb, e_pn, c_pn, mx, rbh.max()))
    _note("reduction localvol mean", a, c_rb)
    assert _note("reduction localvol pnorm", e_pn, c_pn) <= c_pn
    assert mx == rbh.max()
    if kind == "top_solid":
        bpl = (ne[0] * ne[1] + 255) // 256
        assert (int(np.argmax(rbh)) // (ne[0] * ne[1])) * bpl >= 256
    assert abs(LD(mx) - ref["rb_max"]) <= c_rb * rr.EPS * ref["rb_max"]
    _show("reduction localvol")
