"""tp_elasticity_stress on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the gathered
fields: tests/stress_worker.py.  With the test process itself at most four processes hold the GPU at a time."""
import pytest

from tests.slab_launch import launch


# Two slabs on 16x8x8; three on 16x8x12 (8 layers do not divide by three): the middle rank has a neighbour, a stale ghost plane
# and a ghost element layer's worth of traffic on both sides.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (3, (16, 8, 12))])
def test_stress_on_slabs_matches_one_rank(nproc, mesh):
    launch("stress_worker.py", "stress", nproc, mesh)
