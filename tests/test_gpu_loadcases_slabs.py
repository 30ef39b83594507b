"""tp_elasticity_response on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the gathered
fields: tests/loadcases_worker.py.  With the test process itself at most four processes hold the GPU at a time."""
import pytest

from tests.slab_launch import launch


# Two slabs on the two meshes of the one-rank tests' kind (16x8x8; 20x12x32: not tile-aligned).  A slab partition needs the
# element layers to divide by the number of ranks and, with two multigrid levels, four layers per rank: 8 and 32 layers do not
# divide by three, so the three-slab cases take the nearest depths that do (12 and 36) -- the middle rank then has a neighbour,
# and a stale ghost plane, on both sides.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (2, (20, 12, 32)), (3, (16, 8, 12)), (3, (20, 12, 36))])
def test_response_on_slabs_matches_one_rank(nproc, mesh):
    launch("loadcases_worker.py", "response", nproc, mesh)
