"""jjs_verify_all_* on the device: the routed entry points (product library) on valid batches of every scheme and size
band, one spoilt item per failure class with the statuses of the inline call, the adversarial constructions, an empty
batch, and four threads at once; then verify_all_child.py forces the verdict algorithm (profiling build) at every size."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from helpers import ARG_ORDER, make_batch, oracle_verify
from verify_all_cases import cancelling_equations, cancelling_torsion, cofactorless_torsion, device_batch, spoil_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCHEMES = ["single", "double", "vargen"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def _dev_verdict(eng, scheme, cols):
    import torch
    v = eng.verify_all(scheme, *cols)
    torch.cuda.synchronize()
    return int(v.cpu().view(torch.int32).item())


@pytest.mark.parametrize("scheme", SCHEMES)
def test_valid_batches_every_size_band(eng, scheme):
    for n in (1, 65, 16385, 1 << 17):
        cols = device_batch(eng, scheme, n, 4096)
        assert _dev_verdict(eng, scheme, cols) == 1, n
        if n <= 16385:
            ok, st = eng.verify_all(scheme, *[c.cpu().numpy() for c in cols])
            assert ok and st is None, n


@pytest.mark.parametrize("scheme", SCHEMES)
def test_empty_batch_is_accepted(eng, scheme):
    import torch
    widths = eng._WIDTHS[scheme]
    assert eng.verify_all(scheme, *[np.zeros((0, w), np.uint8) for w in widths]) == (True, None)
    assert _dev_verdict(eng, scheme, [torch.zeros((0, w), dtype=torch.uint8, device="cuda") for w in widths]) == 1


@pytest.mark.parametrize("scheme", SCHEMES)
def test_one_spoilt_item_statuses_match_inline(eng, scheme):
    import torch
    base = make_batch(scheme, 65, seed=41, n_keys=65, mix=False)
    for name, b in spoil_cases(scheme, base):
        cols = [b[k] for k in ARG_ORDER[scheme]]
        want = oracle_verify(scheme, b)
        ok, st = eng.verify_all(scheme, *cols)
        inline, _ = eng.verify(scheme, *cols)
        assert not ok, name
        assert st.tolist() == inline.tolist() == want.tolist(), name
        assert _dev_verdict(eng, scheme, [torch.from_numpy(c).cuda() for c in cols]) == 0, name


def test_adversarial_constructions_are_rejected(eng):
    for scheme, b in cancelling_equations() + [("single", cancelling_torsion()), ("single", cofactorless_torsion())]:
        want = oracle_verify(scheme, b)
        ok, st = eng.verify_all(scheme, *[b[k] for k in ARG_ORDER[scheme]])
        assert not ok and st.tolist() == want.tolist(), scheme


def test_four_threads_at_once(eng):
    batches = []
    for t in range(4):
        scheme = SCHEMES[t % 3]
        good = make_batch(scheme, 300, seed=60 + t, n_keys=50, mix=False)
        bad = spoil_cases(scheme, good)[t][1]
        batches += [(scheme, good, True), (scheme, bad, False)]
    errors = []

    def worker(k):
        try:
            for _ in range(3):
                for scheme, b, want in batches[2 * k:2 * k + 2]:
                    ok, _ = eng.verify_all(scheme, *[b[c] for c in ARG_ORDER[scheme]], statuses_on_failure=False)
                    assert ok == want, (k, scheme, want)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_verdict_algorithm_forced_at_every_size():
    p = subprocess.run([sys.executable, os.path.join(HERE, "verify_all_child.py")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]
