"""Thermal expansion on z-slabs: 16 x 8 x 8 on 2 ranks and 12 x 8 x 12 on 3 -- tests/thermoelastic_worker.py
through tests/slab_launch.py, the ranks sharing one GPU (with the test's own process at most four hold it).  The load, the adjoint
right-hand side and the sensitivity equal the one-rank call bit for bit after the halo refresh, the ghost planes of the outputs
stay; one driver iteration gives fx and dfdx within the one-rank test's bound against the direct solves of the whole mesh."""
import pytest

from tests import thermoelastic_ref as tr
from tests.slab_launch import launch

pytestmark = pytest.mark.gpu
IDS = lambda i: "%sx%d" % ("x".join(str(v) for v in tr.SLAB_CASES[i][0]), tr.SLAB_CASES[i][2])


@pytest.mark.parametrize("kind", sorted(tr.DESIGNS))
@pytest.mark.parametrize("ci", range(len(tr.SLAB_CASES)), ids=IDS)
def test_kernels_on_slabs(ci, kind):
    ranks = tr.SLAB_CASES[ci][2]
    assert ranks + 1 <= 4
    launch("thermoelastic_worker.py", "kernels", ranks, [ci, kind], timeout=120)


@pytest.mark.parametrize("ci", range(len(tr.SLAB_CASES)), ids=IDS)
def test_driver_iteration_on_slabs(ci):
    ranks = tr.SLAB_CASES[ci][2]
    assert ranks + 1 <= 4
    launch("thermoelastic_worker.py", "driver", ranks, [ci], timeout=120)
