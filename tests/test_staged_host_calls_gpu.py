"""The eight blocking host-buffer forms that stage their columns in one area through one frame (csrc/staged_host_call.h), in a
fresh process each (staged_host_calls_child.py): every host form's outputs equal, byte for byte, those of its own _dev form on the
same inputs -- back to back at a tiny ragged shape, behind a call that makes the area grow, behind jjs_trim, behind a refused call
of another form, in a second engine of the process, and from two host threads at once."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def child(mode):
    p = subprocess.run([sys.executable, os.path.join(HERE, "staged_host_calls_child.py"), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_eight_forms_interleaved_regrown_trimmed_refused_and_restarted():
    r = child("sequence")
    print(r)
    # the tiny calls fit the smallest area; the call that no longer fits is found by doubling, and the area holds it afterwards
    assert r["staging_after"] > r["staging_before"] and r["grew_at_rows"] >= 8
    assert r["staging_trimmed"] < r["staging_tiny"]
    assert r["refused_calls"] == 16                  # two of each form


def test_two_threads_of_different_forms():
    r = child("threads")
    assert r == {"calls_per_thread": 50, "forms": ["sign_fixed", "verify_share"]}
