"""tp_localvol on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the gathered field:
tests/localvol_worker.py.  With the test process itself at most four processes hold the GPU at a time.

Each own output of a ball sum is the same chain over the same values on any number of slabs, the ghost layers being copies; the
sum over the elements runs layer by layer in ascending global z on one rank and on many.  So cnt, rhobar and dgdx are held to
equality, g and pn to 64 * 2^-53 relative."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(mode, nproc, extra, timeout=240):
    """as tests/test_gpu_stress_slabs.py::_launch (subprocess.run is the hardened one of conftest.py)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "localvol_worker.py"), mode] + [str(v) for v in extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    for k in range(nproc):
        assert "rank %d %s OK" % (k, mode) in r.stdout, r.stdout[-2000:]
    return r.stdout


# Two slabs on 16x8x8 with R = 2.5 h (stencil width 2 of 4 own layers); three on 16x8x12 with R = 3.5 h (3 of 4: the middle rank
# has ghost layers from both sides and a radius that nearly spans a slab).  Squared centre distances are integers in h^2.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh,r_over_h", [(2, (16, 8, 8), 2.5), (3, (16, 8, 12), 3.5)])
def test_localvol_on_slabs_matches_one_rank(nproc, mesh, r_over_h):
    _launch("slabs", nproc, mesh + (r_over_h,))


# 16x12x12 on three slabs of 4 layers, R = 5.5 h: stencil width 5 (half the mesh allows 6)
@pytest.mark.gpu
def test_stencil_wider_than_a_slab_is_refused_on_every_rank():
    _launch("toowide", 3, (16, 12, 12, 5.5))
