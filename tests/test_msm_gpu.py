"""The sums of the two verdict algorithms on the device under chosen scalars: msm_child.py loads the profiling
build once and runs the bucket MSM stage by stage for every window width from 8 to 16 in both shapes, and the run sums and key
points of the key-set verdict, against the Python reference of tests/msm_cases.py (test_msm_host.py holds the same cases
against the CPU build and asserts that every class of case is populated)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_msm_and_keyset_sums_stage_by_stage():
    p = subprocess.run([sys.executable, os.path.join(HERE, "msm_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]
    print(p.stdout)
