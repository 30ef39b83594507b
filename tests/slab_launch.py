"""Shared by the slab tests and their workers: start a worker on several ranks (one torch.distributed.run per test, the ranks
sharing one GPU), and the workers' common __main__ tail."""
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(worker, mode, nproc, extra, timeout=240, env_extra=None):
    """run tests/<worker> <mode> <extra...> on nproc ranks -> its stdout; every rank must end with "rank <k> <mode> OK"
    (subprocess.run is the hardened one of conftest.py: own process group, killed on expiry)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", worker), mode] + [str(v) for v in extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    for k in range(nproc):
        assert "rank %d %s OK" % (k, mode) in r.stdout, r.stdout[-2000:]
    return r.stdout


def run_modes(modes):
    """__main__ of a worker: sys.argv[1] names the entry of `modes` to call with (rank, world) inside a gloo process group"""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    try:
        modes[sys.argv[1]](dist.get_rank(), dist.get_world_size())
    finally:
        dist.destroy_process_group()
