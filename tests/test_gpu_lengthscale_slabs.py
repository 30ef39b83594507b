"""tp_lengthscale on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the gathered field:
tests/lengthscale_worker.py.  With the test process itself at most four processes hold the GPU at a time.

Every term and every entry of the gradients is the same expression over the same values on any number of slabs, the ghost layers
being copies; S is the sum of the layer sums in ascending global z on one rank and on many.  So T, dg, S and g are held to
equality."""
import pytest

from tests.slab_launch import launch


# two slabs on 16x8x8; three of four layers on 16x8x12; three of TWO layers on 8x8x6: the gradient's reach of two layers spans a
# whole slab; two on 8x8x20: more than 16 element layers, the layer sums cross the ranks in two chunks of the sum hook's buffer
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (3, (16, 8, 12)), (3, (8, 8, 6)), (2, (8, 8, 20))])
def test_lengthscale_on_slabs_matches_one_rank(nproc, mesh):
    launch("lengthscale_worker.py", "slabs", nproc, mesh)


# 8x8x3 on three slabs: one own layer
@pytest.mark.gpu
def test_slabs_of_one_layer_are_refused_on_every_rank():
    launch("lengthscale_worker.py", "thin", 3, (8, 8, 3))
