"""TopOpt(robust=...) with passive regions, and the two robust kernels, on z-slabs (two and three slab processes sharing one GPU) against
one rank: tests/robust_worker.py.  With the test process itself at most four processes hold the GPU at a time."""
import pytest

from tests.slab_launch import launch

# two slabs on the 16x8x8 case of tests/test_gpu_robust.py; 8 layers do not divide by three, so the three-slab case takes 16x8x12, the
# depth of the other three-slab tests: the middle rank has a neighbour on both sides, and the void sphere crosses both borders
CASES = [(2, (16, 8, 8)), (3, (16, 8, 12))]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", CASES)
def test_robust_kernels_on_slabs_match_one_rank(nproc, mesh):
    launch("robust_worker.py", "kernels", nproc, mesh)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", CASES)
def test_robust_driver_on_slabs_matches_one_rank(nproc, mesh):
    launch("robust_worker.py", "driver", nproc, mesh)
