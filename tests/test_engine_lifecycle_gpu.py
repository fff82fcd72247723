"""The engine's life from jjs_init to jjs_shutdown, twice in one fresh process (engine_lifecycle_child.py): every buffer the
engine grows on demand is grown by a call whose statuses are checked against the oracle, jjs_trim leaves nothing retired and no
key pool, and the second engine of the process allocates, step for step, what the first one did -- tear-down left nothing
behind, and growth is a function of the calls alone."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_two_lifetimes_in_a_fresh_process():
    p = subprocess.run([sys.executable, os.path.join(HERE, "engine_lifecycle_child.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    first, second = r["rounds"]
    assert [name for name, _ in first] == ["resident affine", "resident wire", "resident ext", "host lane", "host pipeline", "key tables",
                                           "verify_all", "key set", "signer group", "inline multisig"]
    for trimmed in r["after_trim"]:
        assert trimmed["retired"] == 0 and trimmed["key_pools"] == 0, trimmed
    assert second == first, "\n".join(f"{a} | {b}" for a, b in zip(first, second) if a != b)
    assert r["stale_handle_rejected"]
