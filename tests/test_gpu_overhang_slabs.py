"""tp_overhang on z-slabs (two and three slab processes sharing one GPU) against the one-rank call on the whole field:
tests/overhang_worker.py.  With the test process itself at most four processes hold the GPU at a time.

The ranks sweep one after the other; what crosses the border is a copy of one layer (xi upwards, w * lambda downwards), and every
own cell goes through the same per-cell function on the same values.  So xi and the transpose are held to equality."""
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
    """as tests/test_gpu_localvol_slabs.py::_launch (subprocess.run is the hardened one of conftest.py)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "overhang_worker.py"), mode] + [str(v) for v in extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    for k in range(nproc):
        assert "rank %d %s OK" % (k, mode) in r.stdout, r.stdout[-2000:]
    return r.stdout


# Two slabs of 16x8x8 and three of 16x8x12: four own layers each, the middle rank of three has a neighbour on both sides.  +z and
# -z, chunk lengths 1 and 4 (a whole slab per launch), xi and the transpose of two vectors.
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,mesh", [(2, (16, 8, 8)), (3, (16, 8, 12))])
def test_overhang_on_slabs_matches_one_rank(nproc, mesh):
    _launch("slabs", nproc, mesh)


@pytest.mark.gpu
def test_y_build_on_two_ranks_is_refused():
    _launch("ybuild", 2, (16, 8, 8))
