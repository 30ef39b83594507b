"""TopOpt(passive=...) on z-slabs (two and three slab processes sharing one GPU) against one rank: tests/passive_worker.py.  With the
test process itself at most four processes hold the GPU at a time."""
import pytest

from tests.slab_launch import launch


# two slabs on the 16x8x8 case of tests/test_gpu_passive.py; 8 layers do not divide by three, so the three-slab case takes 16x8x12,
# the depth of the other three-slab tests: the middle rank has a neighbour on both sides, and the void sphere crosses both borders
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (3, (16, 8, 12))])
def test_driver_with_passive_regions_on_slabs_matches_one_rank(nproc, mesh):
    launch("passive_worker.py", "driver", nproc, mesh)


@pytest.mark.gpu
def test_a_slab_without_an_active_element_is_refused_on_every_rank():
    launch("passive_worker.py", "emptyrank", 2, (16, 8, 8))
