"""The mass operator, the mass sensitivity, the block-vector passes and the subspace iteration on z-slabs (two and three slab
processes sharing one GPU) against the one-rank calls and the restatement: tests/eigen_worker.py.  With the test process itself at
most four processes hold the GPU at a time.  The cases are those of tests/eigen_ref.py SLAB_CASES: 16x8x8 on two slabs, 12x8x12 on
three, and 8x8x6 on three with two own layers each.  The last one passes the kernel test; its subspace iteration is NOT held
to the bound: two layers per rank allow a single multigrid level on slabs, the one run of Eigenmodes in that configuration did not
finish within 240 s (one rank needs 0.45 s for the same 1435 solver iterations, the other two slab cases 13 s and 45 s), the cause
was not found, and Eigenmodes now refuses several ranks with one level.  The test holds it to that refusal."""
import pytest

from tests.slab_launch import launch

CASES = [("slab2", 2), ("slab3", 3), ("slab3thin", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,nproc", CASES)
def test_mass_kernels_and_block_passes_on_slabs(case, nproc):
    launch("eigen_worker.py", "kernels", nproc, [case])


@pytest.mark.gpu
@pytest.mark.parametrize("case,nproc", CASES)
def test_eigenmodes_on_slabs(case, nproc):
    launch("eigen_worker.py", "modes", nproc, [case])
