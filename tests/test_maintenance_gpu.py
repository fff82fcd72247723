"""jjs_reserve, jjs_trim, jjs_memory_stats and jjs_path_stats BESIDE live calls (include/jjs_gpu.h lets every call come from any
thread and sets no time for a reserve): each mode of maintenance_child.py in a fresh process -- eight threads of verification
calls through the product library, a ninth that walks a plan of maintenance calls (maintenance_cases.py), every call's statuses
and tally compared with the oracle's.

  reserve-lanes     small host-buffer calls while jjs_reserve(host_buffers=1) grows the lanes step by step, in two engine
                    lifetimes: a reserve must never replace the areas of a lane that calls are copying into, uploading from or
                    reading their statuses from
  reserve-large     host-buffer calls of 65 536 items (the piece-by-piece pipeline, outside the engine's mutex) while a reserve
                    grows the device's staging and sizes the slot such a call owns
  reserve-resident  resident calls on four streams, the key-table path among them, beside reserves and the two statistics calls
  trim              all three kinds of traffic beside twenty jjs_trim

A child that is killed at its limit has hung: nothing is tried again.  MEASURED_S: each child's wall time on an MI355X.
The one-item calls cannot each hold the statuses 0, 1 and 2: they are one item of each status in turn (maintenance_child.py
small_work), so that a status column of zeros is wrong for two calls of three; the calls of 64 and 1 024 items hold all three."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# seconds a child may take: ten times what the mode measured, wall time of the whole child, and never under 60
MEASURED_S = {"reserve-lanes": 2.95, "reserve-large": 3.12, "reserve-resident": 2.55, "trim": 4.10}      # of which 0.9 / 1.2 / 0.6 / 2.1 s behind jjs_init
LIMITS = {mode: max(60, int(10 * s)) for mode, s in MEASURED_S.items()}


@pytest.mark.parametrize("mode", list(MEASURED_S))
def test_maintenance_beside_live_calls(mode):
    p = subprocess.run([sys.executable, os.path.join(HERE, "maintenance_child.py"), mode], capture_output=True, text=True, timeout=LIMITS[mode])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert lines, p.stdout[-2000:] + p.stderr[-3000:]
    r = json.loads(lines[-1])
    print(r)
    assert r["errors"] == [] and r["wrong_statuses"] == 0 and r["wrong_calls"] == 0 and r["wrong_tallies"] == 0, r
    assert all(r["checks"].values()), r["checks"]
    assert p.returncode == 0 and r["ok"] is True, p.stderr[-3000:]
