"""tp_localvol on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the gathered field:
tests/localvol_worker.py.  With the test process itself at most four processes hold the GPU at a time.

Each own output of a ball sum is the same chain over the same values on any number of slabs, the ghost layers being copies; the
sum over the elements runs layer by layer in ascending global z on one rank and on many.  So cnt, rhobar and dgdx are held to
equality, g and pn to 64 * 2^-53 relative."""
import pytest

from tests.slab_launch import launch


# Two slabs on 16x8x8 with R = 2.5 h (stencil width 2 of 4 own layers); three on 16x8x12 with R = 3.5 h (3 of 4: the middle rank
# has ghost layers from both sides and a radius that nearly spans a slab); two on 8x8x20: more than 16 element layers, the layer
# sums cross the ranks in two chunks of the sum hook's buffer.  Squared centre distances are integers in h^2.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh,r_over_h", [(2, (16, 8, 8), 2.5), (3, (16, 8, 12), 3.5), (2, (8, 8, 20), 2.5)])
def test_localvol_on_slabs_matches_one_rank(nproc, mesh, r_over_h):
    launch("localvol_worker.py", "slabs", nproc, mesh + (r_over_h,))


# 16x12x12 on three slabs of 4 layers, R = 5.5 h: stencil width 5 (half the mesh allows 6)
@pytest.mark.gpu
def test_stencil_wider_than_a_slab_is_refused_on_every_rank():
    launch("localvol_worker.py", "toowide", 3, (16, 12, 12, 5.5))
