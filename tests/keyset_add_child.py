"""Child process of test_keyset_add_gpu.py: old indices under a concurrent add.  A set of 64 keys with room reserved for 120;
four threads issue 64-item jjs_keyset_verify host calls whose indices are all below 64 while a fifth performs 8 adds of 8 keys --
seven in place, the last one moving the set; the first gives the lookup table more slots.  Every status of every call equals
the C oracle's, whichever set the call saw; afterwards the set equals jjs_keyset_create of all 128 keys.  Prints "ok" and
exits 0 when every check holds."""
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import keyset_add_cases as ac  # noqa: E402
from helpers import oracle_verify  # noqa: E402

N_ITEMS = 4096


def main() -> None:
    import torch
    import jubjub_schnorr_amd as jjs
    assert torch.cuda.is_available()
    eng = jjs.engine()
    b, h = ac.signed_batch("single", N_ITEMS, 128, 901)       # item i names key i % 128, as the oracle saw it
    keys = np.frombuffer(b"".join(h), np.uint8).reshape(128, 64)
    # what the oracle says of every item with the key it NAMES (a few items carry another key's signature: status 2 either way)
    named = dict(b, PK=np.ascontiguousarray(keys[np.arange(N_ITEMS) % 128]))
    want = oracle_verify("single", named, threads=16).astype(np.uint8)
    idx = (np.arange(N_ITEMS) % 128).astype(np.uint32)
    sig = [b["u"], b["R"], b["m"]]
    old = np.where(idx < 64)[0]
    calls = [old[k:k + 64] for k in range(0, len(old) - 63, 64)]          # 64-item calls, indices below 64
    assert len(calls) >= 16 and len(set(want[old].tolist())) >= 2

    ks = eng.keyset("single", keys[:64])
    ks.reserve(120)
    done, errors = threading.Event(), []

    def verifier(t):
        try:
            k = 0
            while k < 8 or not done.is_set():
                pick = calls[(t + 4 * k) % len(calls)]
                st, tally = ks.verify(idx[pick], *[c[pick] for c in sig])
                if not (st == want[pick]).all() or int(tally.sum()) != 64:
                    errors.append((t, k, st.tolist(), want[pick].tolist()))
                    return
                k += 1
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    def adder():
        try:
            for a in range(8):
                lo = 64 + 8 * a
                got, st = ks.add(keys[lo:lo + 8])
                if got.tolist() != list(range(lo, lo + 8)) or st.any():
                    errors.append(("add", a, got.tolist(), st.tolist()))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(("add", repr(e)))
        finally:
            done.set()

    threads = [threading.Thread(target=verifier, args=(t,)) for t in range(4)] + [threading.Thread(target=adder)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:2]
    g = ks.growth()
    assert g == {"capacity": 180, "add_calls": 8, "relocations": 2, "lookup_rebuilds": 1, "add_known": 0}, g
    with eng.keyset("single", keys) as fresh:
        for s in (ks, fresh):
            st, tally = s.verify(idx, *sig)
            assert (st == want).all(), "the grown set / the created one against the oracle"
            assert s.find(keys).tolist() == list(range(128))
        assert ks.info()["keys"] == fresh.info()["keys"] == 128 and ks.info()["valid_keys"] == fresh.info()["valid_keys"] == 128
        assert (ks.key_status == fresh.key_status).all()
    ks.close()
    eng.trim()
    print("ok")


if __name__ == "__main__":
    main()
