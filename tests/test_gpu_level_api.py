"""The level-by-level multigrid calls on the device through the Python classes ("The hierarchy level by level"):
one contract on LinearElasticity, HeatConduction and the PDE Filter.  One mesh of 8 x 8 x 8 elements with two levels, the
smallest on which level 0 has a coarser neighbour and level 1 has none.  What is refused is refused before any launch and leaves
its vectors as they were; what is forwarded is the call it was before (level_apply(0) = MatMult bit for bit, the sizes of the
transfers and of the diagonals).  The numbers themselves are held row by row in test_gpu_rowwise, test_gpu_pde_rowwise and
test_gpu_conduction."""
import pytest
import torch

pytestmark = pytest.mark.gpu
NE, NLV = 8, 2
H = 1.0 / NE
DOF = {"elasticity": 3, "conduction": 1, "pdefilter": 1}
ASSEMBLES = ("elasticity", "conduction")
_OBJ = {}


@pytest.fixture(scope="module")
def tp():
    import topopt_in_petsc_amd as tp
    yield tp
    for grid, _ in _OBJ.values():
        grid.close()
    _OBJ.clear()


def fresh(tp, name):
    """-> (grid, object) straight from its constructor: supports set, nothing assembled"""
    grid = tp.Grid(NE + 1, NE + 1, NE + 1, H)
    if name == "elasticity":
        obj = tp.LinearElasticity(grid, tp.SolverOptions(nlvls=NLV))
        obj.SetUpLoadAndBC()
    elif name == "conduction":
        obj = tp.HeatConduction(grid, tp.SolverOptions(nlvls=NLV))
        obj.SetUpLoadAndBC()
    else:
        obj = tp.Filter(grid, 2, 2.5 * H, tp.SolverOptions(nlvls=NLV, rtol=1e-8, dtol=1e3, max_it=60, nsmooth=2, ncoarse=10))
    return grid, obj


def assembled(tp, name):
    """one object per family for the whole file; the tests leave it as they found it"""
    if name not in _OBJ:
        grid, obj = fresh(tp, name)
        x = grid.synth_density()
        if name == "elasticity":
            obj.AssembleStiffnessMatrix(x, 1e-9, 1.0, 3.0)
        elif name == "conduction":
            obj.AssembleConductivityMatrix(x, 1e-3, 1.0, 3.0)
        _OBJ[name] = (grid, obj)
    return _OBJ[name]


def rand_vec(obj, l, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = obj.level_vec(l)
    return (torch.rand(v.numel(), dtype=torch.float64, generator=g) - 0.5).to(v.device)


def refused(tp, code, call, *kept):
    """call() raises TopOptError with `code`, and every tensor of `kept` has the bits it had"""
    before = [t.clone() for t in kept]
    with pytest.raises(tp.TopOptError) as err:
        call()
    print("%s -> code %d" % (err.value, err.value.code))
    assert err.value.code == code
    for t, t0 in zip(kept, before):
        assert torch.equal(t.view(torch.int64), t0.view(torch.int64)), "a refused call wrote to one of its vectors"


@pytest.mark.parametrize("name", ASSEMBLES)
def test_before_the_first_assembly_the_operator_calls_answer_state(tp, name):
    grid, obj = fresh(tp, name)
    try:
        assert obj.level_count() == NLV and obj.level_nodes(0) == (NE + 1) ** 3      # (these four ask for no assembly)
        v, b, x = rand_vec(obj, 0, 1), rand_vec(obj, 0, 2), rand_vec(obj, 0, 3)
        refused(tp, 2, lambda: obj.level_apply(0, v), v)
        refused(tp, 2, lambda: obj.level_dinv(0))
        refused(tp, 2, lambda: obj.smooth(0, b, x, 1), b, x)
        refused(tp, 2, lambda: obj.level_residual(0, b, x), b, x)
        assert obj.restrict(0, v).numel() == DOF[name] * obj.level_nodes(1)          # (the transfers neither)
    finally:
        grid.close()


@pytest.mark.parametrize("name", sorted(DOF))
def test_a_level_the_hierarchy_lacks_is_an_argument_error_and_nothing_is_written(tp, name):
    grid, obj = assembled(tp, name)
    v, b, x = rand_vec(obj, 0, 4), rand_vec(obj, 0, 5), rand_vec(obj, 0, 6)
    xc = rand_vec(obj, 1, 7)
    refused(tp, 1, lambda: obj.level_apply(NLV, v), v)
    refused(tp, 1, lambda: obj.level_apply(-1, v), v)
    refused(tp, 1, lambda: obj.level_nodes(NLV))
    refused(tp, 1, lambda: obj.level_lambda(-1))
    refused(tp, 1, lambda: obj.level_lambda_min(NLV))
    refused(tp, 1, lambda: obj.level_dinv(NLV))
    refused(tp, 1, lambda: obj.smooth(NLV, b, x, 1), b, x)
    refused(tp, 1, lambda: obj.smooth(0, b, x, -1), b, x)
    refused(tp, 1, lambda: obj.restrict(NLV - 1, xc), xc)
    refused(tp, 1, lambda: obj.prolong_add(NLV - 1, xc, x), xc, x)
    refused(tp, 1, lambda: obj.prolong_add(-1, xc, x), xc, x)
    if name in ASSEMBLES:
        refused(tp, 1, lambda: obj.level_residual(NLV, b, x), b, x)
    else:
        refused(tp, 1, lambda: obj.smooth(0, b, x, 0), b, x)      # the PDE filter has no copies-only call
        assert not hasattr(obj, "level_residual") and not hasattr(obj, "pop_stats")


@pytest.mark.parametrize("name", ASSEMBLES)
def test_zero_steps_are_legal_and_return_x_bit_for_bit(tp, name):
    grid, obj = assembled(tp, name)
    b, x = rand_vec(obj, 0, 8), rand_vec(obj, 0, 9)
    x0 = x.clone()
    out = obj.smooth(0, b, x, 0, False)
    assert out is x and torch.equal(x.view(torch.int64), x0.view(torch.int64))


def test_a_cone_filter_has_no_hierarchy(tp):
    grid = tp.Grid(NE + 1, NE + 1, NE + 1, H)
    try:
        f = tp.Filter(grid, 1, 2.5 * H)
        v = grid.node_vec(1)
        refused(tp, 1, f.level_count)
        refused(tp, 1, lambda: f.level_nodes(0))
        refused(tp, 1, lambda: f.level_lambda(0))
        refused(tp, 1, lambda: f.level_apply(0, v), v)
        refused(tp, 1, f.last_op_form)
    finally:
        grid.close()


@pytest.mark.parametrize("name", sorted(DOF))
def test_the_forwards_are_the_calls_they_were(tp, name):
    grid, obj = assembled(tp, name)
    dof = DOF[name]
    assert obj.level_count() == NLV
    assert [obj.level_nodes(l) for l in range(NLV)] == [(NE // 2 ** l + 1) ** 3 for l in range(NLV)]
    assert obj.level_vec(0).numel() == dof * (NE + 1) ** 3
    u = rand_vec(obj, 0, 10)
    y = obj.level_apply(0, u)
    form = obj.last_op_form()
    y_ref = torch.zeros_like(u)
    if name == "pdefilter":
        obj.PDEApply(u, y_ref)
    else:
        obj.MatMult(u, y_ref)
    assert obj.last_op_form() == form and form[0] in (1, 3)
    assert torch.equal(y.view(torch.int64), y_ref.view(torch.int64)) and float(y.abs().max()) > 0.0
    rc = obj.restrict(0, rand_vec(obj, 0, 11))
    assert rc.numel() == dof * obj.level_nodes(1) and bool(torch.isfinite(rc).all()) and float(rc.abs().max()) > 0.0
    xf = torch.zeros_like(u)
    assert obj.prolong_add(0, rc, xf) is xf and float(xf.abs().max()) > 0.0
    for l in range(NLV):
        d = obj.level_dinv(l)
        assert d.numel() == dof * obj.level_nodes(l) and bool(torch.isfinite(d).all()) and float(d.min()) > 0.0
        assert obj.level_lambda(l) > 0.0 and obj.level_lambda_min(l) >= 0.0
    if name in ASSEMBLES:
        obj.pop_stats()
        obj.level_apply(0, u)
        nbytes, flops, launches = obj.pop_stats()
        assert launches >= 1 and nbytes > 0.0 and obj.pop_stats() == (0.0, 0.0, 0)
