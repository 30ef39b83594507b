"""The stress-stiffness kernels and the buckling mode solver on z-slabs (two and three slab processes sharing one GPU) against the
one-rank calls and the restatement: tests/buckling_worker.py.  With the test process itself at most four processes hold the GPU at
a time.  The cases are those of tests/buckling_ref.py SLAB_CASES: 16x4x8 on two slabs, 12x4x12 on three, and 8x4x6 on three with
two own layers each -- a single multigrid level, which BucklingModes refuses on several ranks as Eigenmodes does."""
import pytest

from tests.slab_launch import launch


@pytest.mark.gpu
@pytest.mark.parametrize("case,nproc", [("slab2", 2), ("slab3", 3)])
def test_geom_kernels_on_slabs(case, nproc):
    launch("buckling_worker.py", "kernels", nproc, [case])


@pytest.mark.gpu
def test_buckling_modes_on_two_slabs():
    launch("buckling_worker.py", "modes", 2, ["slab2"])


@pytest.mark.gpu
def test_buckling_modes_refuses_one_level_on_three_slabs():
    launch("buckling_worker.py", "modes", 3, ["slab3thin"])
