"""Child process of test_key_memo_gpu.py: the profiling build (for its hit / built counters, include/jjs_gpu_key_memo.h;
no path or window is forced) runs sequences of key-table calls in ONE call slot -- batches of more than 131 072 items on one
stream stay in the first big slot, host-buffer calls in the second -- and checks every status and tally against the C oracle
and every call's hits and built keys against key_memo_cases.MemoModel."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

from helpers import ARG_ORDER, batch_to_extended, make_batch, oracle_verify, to_wire  # noqa: E402
from key_memo_cases import KEY_COLUMNS, MemoModel, concat, sequences, take  # noqa: E402

N_BIG = 140000          # > 131 072: a big slot; every key of the small sets below far more than 128 times (wide windows)


def main() -> None:
    import torch
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    lib.jjs_debug_key_memo_stats.argtypes = [ctypes.c_void_p]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def memo_stats():
        torch.cuda.synchronize()
        out = (ctypes.c_uint64 * 2)()
        assert lib.jjs_debug_key_memo_stats(out) == 0
        return int(out[0]), int(out[1])

    want_cache = {}

    def want_of(scheme, b):
        if id(b) not in want_cache:
            want_cache[id(b)] = (b, oracle_verify(scheme, b))
        return want_cache[id(b)][1]

    def tiled(b, n):
        reps = -(-n // len(b["u"]))
        return {k: np.tile(v, (reps, 1)) for k, v in b.items()}, reps

    def run(scheme, b, n, how="dev"):
        """b tiled to at least n items through one entry point -> (statuses ok, hits, built, path delta)"""
        big, reps = tiled(b, n)
        want = np.tile(want_of(scheme, b), reps)
        h0, b0 = memo_stats()
        p0 = eng.path_stats()
        if how == "dev":
            st, tally = eng.verify(scheme, *[dev(big[k]) for k in ARG_ORDER[scheme]])
        elif how == "ext":
            ext = batch_to_extended(scheme, b)
            st, tally = eng.verify_ext(scheme, *[dev(np.tile(a, (reps, 1))) for a in ext])
        elif how == "wire":
            st, tally = eng.verify_wire(scheme, *[dev(np.tile(a, (reps, 1))) for a in to_wire(scheme, b)])
        else:
            st, tally = eng.verify(scheme, *[big[k] for k in ARG_ORDER[scheme]])                   # host buffers
        h1, b1 = memo_stats()
        p1 = eng.path_stats()
        st = st.cpu().numpy() if hasattr(st, "cpu") else st
        tally = tally.cpu().numpy() if hasattr(tally, "cpu") else tally
        assert (st == want).all(), (scheme, how, int((st != want).sum()))
        assert tally.tolist() == [int((want == k).sum()) for k in range(4)], (scheme, how)
        return h1 - h0, b1 - b0, {k: p1[k] - p0[k] for k in ("key_tables_wide", "key_tables_narrow", "keys_do_not_repeat")}

    def turned_down(scheme, b, n):
        """b tiled, with more distinct (garbage) keys than n / 16: the batch turns the tables down"""
        big, _ = tiled(b, n)
        m = len(big["u"])
        rows = np.arange(m // 12)
        big["PK"] = big["PK"].copy()
        big["PK"][rows] = np.random.default_rng(9).integers(0, 256, (len(rows), 64), dtype=np.uint8)
        want = np.tile(want_of(scheme, b), -(-n // len(b["u"])))
        want[rows] = oracle_verify(scheme, take(big, rows))
        h0, b0 = memo_stats()
        p0 = eng.path_stats()
        st, _ = eng.verify(scheme, *[dev(big[k]) for k in ARG_ORDER[scheme]])
        h1, b1 = memo_stats()
        assert (st.cpu().numpy() == want).all(), scheme
        assert eng.path_stats()["keys_do_not_repeat"] == p0["keys_do_not_repeat"] + 1
        return h1 - h0, b1 - b0

    def total(model_out):
        return sum(model_out[0]), sum(model_out[1])

    # ---- pool growth between calls (first: jjs_trim remembers the size a slot has learnt) -------------------------------
    A = make_batch("single", 96, seed=77, n_keys=24)
    model = MemoModel()
    pool0 = None
    for k, n in enumerate((N_BIG, 2 * N_BIG, 2 * N_BIG)):
        hits, built, _ = run("single", A, n)
        pool = eng.path_stats()["key_pool_bytes"]
        if k == 1:
            assert pool > pool0, (pool0, pool)           # the larger batch made the slot replace its pool
            model.flush()
        pool0 = pool
        assert (hits, built) == total(model.call("single", A, 6)), ("growth", k, hits, built)
        print("growth", k, "hits", hits, "built", built)

    # ---- the sequences of key_memo_cases, every scheme, resident affine calls (wire calls where the step says so) -------
    for scheme in ("single", "double", "vargen"):
        for name, steps in sequences(scheme).items():
            if name == "width 6, 5, 6":
                continue                                   # needs more keys than these sets have: below
            eng.trim(); model = MemoModel()
            for k, (b, window, flags) in enumerate(steps):
                if "new_pool" in flags:
                    eng.trim(); model.flush()
                if not window:
                    got = turned_down(scheme, b, N_BIG)
                elif "off" in flags:
                    got = run(scheme, b, N_BIG, "wire")[:2]
                else:
                    hits, built, path = run(scheme, b, N_BIG)
                    assert path["key_tables_wide"] == 1, (scheme, name, k, path)
                    got = (hits, built)
                want = total(model.call(scheme, b, window, off="off" in flags))
                print(scheme, name, k, "hits", got[0], "built", got[1])
                assert got == want, (scheme, name, k, got, want)

    # ---- width 6 -> 5 -> 5 -> 6 -> 6: 1 200 keys, 160 000 items (133 per key) or 140 000 (116 per key) -----------------
    W = make_batch("single", 2400, seed=91, n_keys=1200)
    eng.trim(); model = MemoModel()
    for k, (n, window) in enumerate(((160000, 6), (140000, 5), (140000, 5), (160000, 6), (160000, 6))):
        hits, built, path = run("single", W, n)
        assert path["key_tables_wide" if window == 6 else "key_tables_narrow"] == 1, (k, path)
        want = total(model.call("single", W, window))
        print("width", k, window, "hits", hits, "built", built)
        assert (hits, built) == want, ("width", k, hits, built, want)

    # ---- the ext and host-buffer entry points ---------------------------------------------------------------------------
    for scheme in ("single", "double", "vargen"):
        C = make_batch(scheme, 120, seed=55, n_keys=20)
        eng.trim(); model = MemoModel()
        for k, how in enumerate(("dev", "ext", "ext", "dev")):
            hits, built, _ = run(scheme, C, N_BIG, how)
            want = total(model.call(scheme, C, 6))
            print(scheme, "ext", k, how, "hits", hits, "built", built)
            assert (hits, built) == want, (scheme, how, k, hits, built, want)
        model = MemoModel()                                # host-buffer calls run in the second big slot: its own memo
        for k in range(3):
            hits, built, _ = run(scheme, C, N_BIG, "host")
            want = total(model.call(scheme, C, 6))
            print(scheme, "host", k, "hits", hits, "built", built)
            assert (hits, built) == want, (scheme, "host", k, hits, built, want)

    # ---- two streams alternating, nobody waits: both big slots are in use, same statuses --------------------------------
    S = make_batch("single", 96, seed=77, n_keys=24)
    big, reps = tiled(S, N_BIG)
    want = np.tile(oracle_verify("single", S), reps)
    args = [dev(big[k]) for k in ARG_ORDER["single"]]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for k in range(6):
        with torch.cuda.stream(streams[k % 2]):
            outs.append(eng.verify("single", *args))
    torch.cuda.synchronize()
    for st, tally in outs:
        assert (st.cpu().numpy() == want).all()
        assert tally.cpu().numpy().tolist() == [int((want == k).sum()) for k in range(4)]
    print("KEY MEMO OK")


if __name__ == "__main__":
    main()
