"""Design-variable linking on z-slabs (two and three slab processes sharing one GPU) against one rank: tests/link_worker.py.  With
the test process itself at most four processes hold the GPU at a time."""
import pytest

from tests.slab_launch import launch

# two slabs on 16x8x8 elements; 8 layers do not divide by three, so the three-slab case takes 16x8x12, the depth of the other
# three-slab tests: the middle rank has a neighbour on both sides
CASES = [(2, (16, 8, 8)), (3, (16, 8, 12))]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", CASES)
def test_maps_on_slabs_equal_one_rank_bit_for_bit(nproc, mesh):
    launch("link_worker.py", "maps", nproc, mesh)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", CASES)
def test_driver_with_links_on_slabs_matches_one_rank(nproc, mesh):
    launch("link_worker.py", "driver", nproc, mesh)


@pytest.mark.gpu
def test_a_z_link_is_refused_on_every_rank():
    launch("link_worker.py", "zlink", 2, (16, 8, 8))
