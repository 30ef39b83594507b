"""Self-weight on z-slabs (two and three slab processes sharing one GPU) against the one-rank calls: tests/selfweight_worker.py.
With the test process itself at most four processes hold the GPU at a time."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = (16, 8, 12)      # 12 layers: two slabs of six, three of four -- the middle rank has a neighbour on both sides


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(mode, nproc, extra, timeout=240):
    """as tests/test_gpu_stress_slabs.py::_launch (subprocess.run is the hardened one of conftest.py: own process group, killed on expiry)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "selfweight_worker.py"), mode] + [str(v) for v in extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    for k in range(nproc):
        assert "rank %d %s OK" % (k, mode) in r.stdout, r.stdout[-2000:]
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 3])
def test_load_and_sensitivity_term_on_slabs_equal_one_rank_bit_for_bit(nproc):
    _launch("kernels", nproc, MESH)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 3])
def test_driver_with_a_body_force_on_slabs_matches_one_rank(nproc):
    _launch("driver", nproc, MESH)
