"""The memo of a slot's last key-table call on the device (csrc/key_tables.h step 5): tests/key_memo_child.py runs the
sequences of tests/key_memo_cases.py, and those that need a device-sized batch, in one call slot."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_sequences_of_calls_in_one_slot():
    r = subprocess.run([sys.executable, os.path.join(HERE, "key_memo_child.py")], capture_output=True, text=True, timeout=1500)
    print(r.stdout[-6000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and "KEY MEMO OK" in r.stdout
