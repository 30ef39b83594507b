"""tp_casting on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the whole field:
tests/casting_worker.py.  With the test process itself at most four processes hold the GPU at a time.

x and y draws are rank-local: no line crosses a slab border.  A z draw runs as a pipeline: the upper range's sweep comes down
from the top rank, the lower range's goes up from rank 0, and what crosses a border is a copy of one layer (c in the forward
sweep, the transpose's hand-over value per vector the other way); every own cell goes through the same per-cell function on the
same values.  So c and the transpose are held to equality."""
import pytest

from tests.slab_launch import launch


# Two slabs of 16x8x8 and three of 16x8x12: four own layers each, the middle rank of three has a neighbour on both sides.  +z, -z
# and z:p with the parting plane on a slab border, one layer beside it and inside a slab, +x in both forms and -y.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (3, (16, 8, 12))])
def test_casting_on_slabs_matches_one_rank(nproc, mesh):
    launch("casting_worker.py", "slabs", nproc, mesh)
