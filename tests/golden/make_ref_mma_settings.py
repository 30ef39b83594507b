#!/usr/bin/env python
"""Records what the REFERENCE's own MMA class computes with each setting of tests/test_mma_surface.py (_REF_CASES):
oracle/_ref/ref_mma (host/ref_mma_driver.cc around the reference's MMA.cc) under host/slabrun, every iteration's design
and KKTresidual's two norms.  Reference outputs, frozen so that the comparison does not depend on an oracle/_ref built
from this tree's driver.  Needs oracle/_ref/ref_mma and a GPU (the compat layer).  Run from the repo root:
    python tests/golden/make_ref_mma_settings.py [outdir]      (default: tests/golden/ref_mma_settings)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF_MMA = os.path.join(ROOT, "oracle", "_ref", "ref_mma")
EX, EY, EZ, ITERS = 16, 8, 8, 8


def case_id(name, m, nproc):
    return "%s-m%d-np%d" % (name, m, nproc)


def run_ref_mma(tokens, m, nproc, timeout=300):
    """(designs [ITERS, n], KKT norms [ITERS, 2]) of one ref_mma run; KKT is None if the binary prints no
    REF_MMA_KKT lines (built from a driver without the key=value settings)"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "x.bin")
        r = subprocess.run([os.path.join(ROOT, "host", "slabrun"), "-n", str(nproc), "--same-device", REF_MMA, str(EX),
                            str(EY), str(EZ), str(m), str(ITERS), out] + list(tokens) + ["kkt=1"],
                           capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise RuntimeError("ref_mma failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        raw = open(out, "rb").read()
    n = EX * EY * EZ
    xs = np.stack([np.frombuffer(raw, dtype=">f8", count=n, offset=k * (8 + 8 * n) + 8).astype(np.float64)
                   for k in range(ITERS)])
    kkt = [[float(v) for v in l.split()[3:5]] for l in r.stdout.splitlines() if l.startswith("REF_MMA_KKT it ")]
    return xs, (np.array(kkt) if len(kkt) == ITERS else None)


def main():
    sys.path.insert(0, ROOT)
    from tests.test_mma_surface import _REF_CASES
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_mma_settings")
    os.makedirs(outdir, exist_ok=True)
    for name, tokens, m, nproc in _REF_CASES:
        xs, kkt = run_ref_mma(tokens, m, nproc)
        if kkt is None:
            sys.exit("oracle/_ref/ref_mma prints no KKT lines: rebuild it from this tree (oracle/build_ref_on_shim.sh)")
        path = os.path.join(outdir, case_id(name, m, nproc) + ".npz")
        np.savez_compressed(path, x=xs, kkt=kkt, tokens=np.array(tokens + ["kkt=1"]))
        print(path, xs.shape, kkt[-1])


if __name__ == "__main__":
    main()
