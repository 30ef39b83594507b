"""Heat conduction on z-slabs: 16 x 8 x 8 on 2 ranks and 12 x 8 x 12 on 3, three levels each, both designs of
tests/conduction_ref.py -- tests/conduction_worker.py through tests/slab_launch.py, the ranks sharing one GPU (with the test's own
process at most four hold it).  The product and the response's dfdx equal the one-rank call bit for bit; the solve is held to
the serial ORACLE by the three history bounds of test_solve_residual_history with an equal iteration count; halo overlap on and
off give the same bits."""
import pytest

from tests import conduction_ref as cr
from tests.slab_launch import launch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", sorted(cr.DESIGNS))
@pytest.mark.parametrize("ci", range(len(cr.SLAB_CASES)), ids=lambda i: "%sx%d" % ("x".join(str(v) for v in cr.SLAB_CASES[i][0]), cr.SLAB_CASES[i][3]))
def test_conduction_on_slabs(ci, kind):
    ranks = cr.SLAB_CASES[ci][3]
    assert ranks + 1 <= 4
    launch("conduction_worker.py", "slabs", ranks, [ci, kind], timeout=120)
