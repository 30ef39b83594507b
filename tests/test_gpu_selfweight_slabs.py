"""Self-weight on z-slabs (two and three slab processes sharing one GPU) against the one-rank calls: tests/selfweight_worker.py.
With the test process itself at most four processes hold the GPU at a time."""
import pytest

from tests.slab_launch import launch

MESH = (16, 8, 12)      # 12 layers: two slabs of six, three of four -- the middle rank has a neighbour on both sides


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 3])
def test_load_and_sensitivity_term_on_slabs_equal_one_rank_bit_for_bit(nproc):
    launch("selfweight_worker.py", "kernels", nproc, MESH)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 3])
def test_driver_with_a_body_force_on_slabs_matches_one_rank(nproc):
    launch("selfweight_worker.py", "driver", nproc, MESH)
