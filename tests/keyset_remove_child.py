"""Child process of test_keyset_remove_gpu.py: calls under a concurrent remove and compact.  A set of 128 keys; two threads issue
64-item jjs_keyset_verify host calls and two 64-item jjs_keyset_verify_keys host calls, all against keys below 64, which are
never removed, while a fifth thread removes keys 64 .. 127 in 8 calls of 8 and then removes from and compacts a SECOND set.
Every status of those calls equals the C oracle's.  A sixth thread names the keys being removed: by index every item gets its
oracle status or 3; by key -- the host form verifies a miss inline -- its oracle status or JJS_STATUS_KEY_NOT_IN_SET, never 3.
(The set has been through one jjs_keyset_remove, of an index beyond it, before the threads start: the header says what a
by-key call queued ahead of a set's FIRST remove may report.)  Afterwards the first set equals jjs_keyset_create of the keys
with the removed ones 0xFF, the second jjs_keyset_create of its survivors.  No call here is meant to fail.  Prints "ok" and
exits 0 when every check holds."""
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import keyset_add_cases as ac  # noqa: E402
import keyset_remove_cases as rc  # noqa: E402
from helpers import oracle_verify  # noqa: E402

N_ITEMS = 4096


def main() -> None:
    import torch
    import jubjub_schnorr_amd as jjs
    assert torch.cuda.is_available()
    eng = jjs.engine()
    b, h = ac.signed_batch("single", N_ITEMS, 128, 901)       # item i names key i % 128, as the oracle saw it
    keys = np.frombuffer(b"".join(h), np.uint8).reshape(128, 64)
    idx = (np.arange(N_ITEMS) % 128).astype(np.uint32)
    named = np.ascontiguousarray(keys[idx])
    want = oracle_verify("single", dict(b, PK=named), threads=16).astype(np.uint8)
    sig = [b["u"], b["R"], b["m"]]
    low, high = np.where(idx < 64)[0], np.where(idx >= 64)[0]
    calls = [low[k:k + 64] for k in range(0, len(low) - 63, 64)]
    doomed = [high[k:k + 64] for k in range(0, len(high) - 63, 64)]
    assert len(calls) >= 16 and len(doomed) >= 16 and len(set(want[low].tolist())) >= 2 and (want[high] == 0).any()

    ks = eng.keyset("single", keys)
    second = eng.keyset("single", keys)
    res, k = ks.remove(np.array([128], np.uint32))
    assert res.tolist() == [rc.NOT_IN_RANGE] and k == 0
    done, errors = threading.Event(), []

    def verifier(t):
        try:
            k = 0
            while k < 8 or not done.is_set():
                pick = calls[(t + 4 * k) % len(calls)]
                cols = [c[pick] for c in sig]
                st, tally = ks.verify(idx[pick], *cols) if t < 2 else ks.verify_keys(named[pick], *cols)
                if not (st == want[pick]).all() or int(tally.sum()) != 64:
                    errors.append((t, k, st.tolist(), want[pick].tolist()))
                    return
                k += 1
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    def names_the_doomed():
        try:
            k = 0
            while k < 8 or not done.is_set():
                pick = doomed[k % len(doomed)]
                cols = [c[pick] for c in sig]
                st, _ = ks.verify(idx[pick], *cols)
                if not ((st == want[pick]) | (st == 3)).all():
                    errors.append(("by index", k, st.tolist(), want[pick].tolist()))
                    return
                st, _ = ks.verify_keys(named[pick], *cols)
                if not ((st == want[pick]) | (st == 6)).all():
                    errors.append(("by key", k, st.tolist(), want[pick].tolist()))
                    return
                k += 1
        except Exception as e:  # noqa: BLE001
            errors.append(("doomed", repr(e)))

    def remover():
        try:
            for a in range(8):
                lo = 64 + 8 * a
                res, k = ks.remove(np.arange(lo, lo + 8, dtype=np.uint32))
                if res.any() or k != 8:
                    errors.append(("remove", a, res.tolist(), k))
                    return
            res, k = second.remove(np.arange(1, 128, 2, dtype=np.uint32))
            m = second.compact()
            if res.any() or k != 64 or m[0::2].tolist() != list(range(64)) or (m[1::2] != rc.GONE).any():
                errors.append(("compact", res.tolist(), k, m.tolist()))
        except Exception as e:  # noqa: BLE001
            errors.append(("remove", repr(e)))
        finally:
            done.set()

    threads = [threading.Thread(target=verifier, args=(t,)) for t in range(4)] + [threading.Thread(target=names_the_doomed), threading.Thread(target=remover)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:2]
    assert ks.removal() == {"removed_keys": 64, "live_keys": 64, "remove_calls": 9, "compact_calls": 0}, ks.removal()
    assert second.removal() == {"removed_keys": 0, "live_keys": 64, "remove_calls": 1, "compact_calls": 1}, second.removal()
    after = np.where(idx < 64, want, 3).astype(np.uint8)
    ff = np.frombuffer(b"".join(rc.with_ff(h, [i >= 64 for i in range(128)])), np.uint8).reshape(128, 64)
    with eng.keyset("single", ff) as fresh:
        for s in (ks, fresh):
            st, _ = s.verify(idx, *sig)
            assert (st == after).all(), "the removed-from set / the created one against the oracle"
            assert s.find(keys).tolist() == list(range(64)) + [rc.MISS] * 64
            assert s.info()["keys"] == 128 and s.info()["valid_keys"] == 64
        assert (ks.key_status == fresh.key_status).all()
    # the compacted set: old index 2 j is new index j
    even = np.where(idx % 2 == 0)[0]
    with eng.keyset("single", keys[0::2]) as fresh:
        for s in (second, fresh):
            st, _ = s.verify(idx[even] // 2, *[c[even] for c in sig])
            assert (st == want[even]).all(), "the compacted set / the created one against the oracle"
            assert s.find(keys).tolist() == [i // 2 if i % 2 == 0 else rc.MISS for i in range(128)]
            assert s.info()["keys"] == 64 == s.info()["valid_keys"]
    ks.close()
    second.close()
    eng.trim()
    print("ok")


if __name__ == "__main__":
    main()
