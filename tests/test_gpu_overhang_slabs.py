"""tp_overhang on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the whole field:
tests/overhang_worker.py.  With the test process itself at most four processes hold the GPU at a time.

The ranks sweep one after the other; what crosses the border is a copy of one layer (xi upwards, w * lambda downwards), and every
own cell goes through the same per-cell function on the same values.  So xi and the transpose are held to equality."""
import pytest

from tests.slab_launch import launch


# Two slabs of 16x8x8 and three of 16x8x12: four own layers each, the middle rank of three has a neighbour on both sides.  +z and
# -z, chunk lengths 1 and 4 (a whole slab per launch), xi and the transpose of two vectors.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (3, (16, 8, 12))])
def test_overhang_on_slabs_matches_one_rank(nproc, mesh):
    launch("overhang_worker.py", "slabs", nproc, mesh)


@pytest.mark.gpu
def test_y_build_on_two_ranks_is_refused():
    launch("overhang_worker.py", "ybuild", 2, (16, 8, 8))
