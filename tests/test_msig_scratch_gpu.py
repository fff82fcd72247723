"""Regions of the multisignature scratch (csrc/msig_scratch.h) that grow, appear in the middle and move change no call's results:
in a fresh process (msig_scratch_child.py), the six multisignature forms give the same bytes before and after a combine call
beyond the first allocation, a first extended call, and an extended call that makes the ext region grow."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_six_forms_unchanged_while_regions_grow_appear_and_move():
    p = subprocess.run([sys.executable, os.path.join(HERE, "msig_scratch_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r == {"forms": ["combine", "group_combine", "keyset_combine", "verify", "verify_share", "multisig_sign"], "runs": 4,
                 "rows": 4100, "transcripts": 1025}
