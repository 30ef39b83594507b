"""Every device buffer of the library has one owner (csrc/common.h: DevBuf), and tp_device_bytes_live() counts what the owners hold.
tests/ownership_worker.py runs in a fresh process, so that no object of another test moves the counter: per object the counter
rises by at least the object's main arrays (worked out from the mesh: a counter that never counts fails), returns exactly to its
value before the create after close(), and is exactly 0 after Grid.close().  A create that is refused (Filter type 2 with ksp_mode 2,
four times) leaves nothing behind.  The slab runs hold the same on every rank; with the test process at most three hold the GPU."""
import os
import re
import subprocess
import sys

import pytest

from tests.ownership_worker import ALL_RETURNED, CASES
from tests.slab_launch import launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    """one child for all the one-process cases (16^3 elements each); a case that fails does not stop the others"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ownership_worker.py"), "one"], cwd=ROOT, capture_output=True,
                       text=True, timeout=200)
    return r.stdout, r.stderr, r.returncode


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES) + [ALL_RETURNED])
def test_counter_rises_with_the_object_and_returns_with_its_close(report, case):
    out, err, rc = report
    m = re.search(r"^case %s (OK|FAILED).*?(?=^case |\Z)" % case, out, flags=re.M | re.S)
    print(m.group(0) if m else out[-3000:])
    assert m and m.group(1) == "OK", (m.group(0) if m else "the child never reached this case (exit %s)\n" % rc) + err[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["solve", "body_load"])
def test_two_slabs_give_everything_back_on_every_rank(mode):
    launch("ownership_worker.py", mode, 2, ())
