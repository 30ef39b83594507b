"""tp_elasticity_stress on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the gathered
fields: tests/stress_worker.py.  With the test process itself at most four processes hold the GPU at a time."""
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
    """as tests/test_multirank.py::_launch (subprocess.run is the hardened one of conftest.py: own process group, killed on expiry)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "stress_worker.py"), mode] + [str(v) for v in extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    for k in range(nproc):
        assert "rank %d %s OK" % (k, mode) in r.stdout, r.stdout[-2000:]
    return r.stdout


# Two slabs on 16x8x8; three on 16x8x12 (8 layers do not divide by three): the middle rank has a neighbour, a stale ghost plane
# and a ghost element layer's worth of traffic on both sides.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (3, (16, 8, 12))])
def test_stress_on_slabs_matches_one_rank(nproc, mesh):
    _launch("stress", nproc, mesh)
