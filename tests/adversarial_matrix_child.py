"""Child process of test_adversarial_matrix_gpu.py: loads the profiling build and runs the battery of
tests/adversarial_matrix_cases.py through the paths only jjs_debug_* reaches, every status against the C oracle --

  the wide-window batch (the battery tiled to the smallest size at which the key tables engage) with narrow windows forced
  (0x500), in the caller's order instead of grouped by key (0x1000), and with the key arena refused
  (jjs_debug_fail_key_arena: the same statuses through the throughput path);
  the memo sequence of the product test (battery, rotated, twins) with the hits and built keys of every call held against
  the sets of distinct keys (jjs_debug_key_memo_stats);
  the verdict algorithm (0x2000; the product never takes it): the whole battery gives verdict 0 with the oracle's statuses;
  every item of class `exact` and every item of the torsion grid with a non-zero status, alone among 64 valid items at the
  first, the middle and the last position: verdict 0 from the host call and from the _dev call, inline keys and a registered
  key set;
  the forced per-item route of verify_all (0x4000) on the whole battery.

Prints "ok" and exits 0 when every check holds."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import adversarial_matrix_cases as amc  # noqa: E402
from helpers import ARG_ORDER  # noqa: E402

KT_LEAST = {"single": 65536, "double": 32768, "vargen": 32768}
TWO_RANGES_LEAST = 65536 + 32768     # csrc/host_calls.h plan_pieces: the smallest block with two ranges of the key and hash columns
ONE_SLOT_LEAST = 131072 + 1          # above the medium slots: calls that follow each other on one stream share a big slot


def main() -> None:
    import torch
    import jubjub_schnorr_amd as jjs
    from jubjub_schnorr_amd import _ffi
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    lib.jjs_debug_key_memo_stats.argtypes = [ctypes.c_void_p]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tally_of = lambda want: [int((want == k).sum()) for k in range(4)]  # noqa: E731

    def memo_stats():
        torch.cuda.synchronize()
        out = (ctypes.c_uint64 * 2)()
        assert lib.jjs_debug_key_memo_stats(out) == 0
        return int(out[0]), int(out[1])

    def run(scheme, b, want, what, moved):
        """one resident affine call: statuses, tally, and the path counters that moved -> (memo hits, keys built)"""
        args = [dev(a) for a in b]
        h0, b0 = memo_stats()
        before = eng.path_stats()
        st, tally = eng.verify(scheme, *args)
        st, tally = st.cpu().numpy(), tally.cpu().numpy()
        h1, b1 = memo_stats()
        after = eng.path_stats()
        bad = np.nonzero(st != want)[0]
        assert not len(bad), (scheme, what, len(bad), bad[:8].tolist(), st[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert tally.tolist() == tally_of(want), (scheme, what)
        delta = {k: after[k] - before[k] for k in ("throughput", "key_tables_wide", "key_tables_narrow")}
        assert delta == {**dict.fromkeys(delta, 0), **moved}, (scheme, what, delta)
        return h1 - h0, b1 - b0

    def dev_verdict(v):
        torch.cuda.synchronize()
        return int(v.cpu().view(torch.int32).item())

    def counters(ks=None):
        """what a per-item call moves: the paths and the host lanes of the inline calls, the calls of a key set"""
        torch.cuda.synchronize()
        p = eng.path_stats()
        c = {k: p[k] for k in ("latency", "throughput", "lane_calls")}
        if ks is not None:
            info = ks.info()
            c.update(small_calls=info["small_calls"], large_calls=info["large_calls"])
        return c

    def expect_moved(before, after, loose=(), **delta):
        """every counter moved by exactly its delta (none: not at all); a counter named in `loose` may also have moved by one
        (the latency path's, which a host lane's launch counts once for all the calls it carries)"""
        for k, v in before.items():
            d = after[k] - v
            assert d == delta.get(k, 0) or (k in loose and d in (0, 1)), (k, before, after, delta)

    def host_pieces(scheme, b, want):
        """one host-buffer affine call -> the pieces its block travelled in (jjs_debug_host_timing out[3])"""
        before = eng.path_stats()
        st, tally = eng.verify(scheme, *[np.ascontiguousarray(a) for a in b])
        assert (st == want).all() and tally.tolist() == tally_of(want), scheme
        assert eng.path_stats()["key_tables_wide"] == before["key_tables_wide"] + 1
        out = (ctypes.c_double * 8)()
        assert lib.jjs_debug_host_timing(out) == 0
        return int(out[3])

    # ---- the transient key tables, forced ------------------------------------------------------------------------------------
    for scheme in amc.SCHEMES:
        f = amc.forms(scheme)
        b, want = amc.tiled(f.arrays("affine"), f.want(), amc.reps_for(f.n, KT_LEAST[scheme]))
        for path, moved in ((0x500, {"key_tables_narrow": 1}), (0x1000, {"key_tables_wide": 1}), (0x1500, {"key_tables_narrow": 1})):
            assert lib.jjs_debug_force_path(path) == 0
            run(scheme, b, want, hex(path), moved)
        assert lib.jjs_debug_force_path(0) == 0
        assert lib.jjs_debug_fail_key_arena(1) == 0
        run(scheme, b, want, "no key arena", {"throughput": 1})
        assert lib.jjs_debug_fail_key_arena(0) == 0
        # host buffers: the smallest block has one range of the key and hash columns, the block of TWO_RANGES_LEAST items one more
        one = host_pieces(scheme, b, want)
        two = host_pieces(scheme, *amc.tiled(f.arrays("affine"), f.want(), amc.reps_for(f.n, TWO_RANGES_LEAST)))
        print(scheme, "host pieces", one, two)
        assert one >= 1 and two == one + 1, (scheme, one, two)

    # ---- the memo sequence: battery, rotated, twins ----------------------------------------------------------------------------
    for scheme in amc.SCHEMES:
        f, tf = amc.forms(scheme), amc.twin_forms(scheme)[0]
        reps = amc.reps_for(f.n, ONE_SLOT_LEAST)
        first, want = amc.tiled(f.arrays("affine"), f.want(), reps)
        twins, want_twins = amc.tiled(tf.arrays("affine"), tf.want(), reps)
        sets = [[{r.tobytes() for r in c} for c in x.key_arrays("affine")] for x in (f, tf)]
        distinct = sum(len(s) for s in sets[0])
        common = sum(len(a & b) for a, b in zip(*sets))
        fresh = sum(len(b - a) for a, b in zip(*sets))
        assert common > 20 and fresh > 20
        eng.trim()
        moved = {"key_tables_wide": 1}
        assert run(scheme, first, want, "memo: first", moved) == (0, distinct)
        assert run(scheme, [np.roll(a, 1, axis=0) for a in first], np.roll(want, 1), "memo: rotated", moved) == (distinct, 0)
        assert run(scheme, twins, want_twins, "memo: twins", moved) == (common, fresh)

    # ---- the verdict algorithm ---------------------------------------------------------------------------------------------------
    assert lib.jjs_debug_force_path(0x2000) == 0
    placed = 0
    for scheme in amc.SCHEMES:
        f = amc.forms(scheme)
        b, classes = amc.battery(scheme)
        want = f.want()
        cols = f.arrays("affine")
        # the verdict algorithm moves none of the counters of the per-item route: a call that fell back to it would
        c0 = counters()
        assert eng.verify_all(scheme, *cols, statuses_on_failure=False) == (False, None), scheme
        assert dev_verdict(eng.verify_all(scheme, *[dev(c) for c in cols])) == 0, scheme
        expect_moved(c0, counters())
        ok, st = eng.verify_all(scheme, *cols)                 # verdict 0: the statuses come from the per-item host call
        assert ok is False and st.tobytes() == want.tobytes(), scheme
        expect_moved(c0, counters(), loose=("latency",), lane_calls=1)
        keys, idx, _ = amc.registered(scheme, f, "affine")
        with eng.keyset(scheme, *keys) as ks:
            c0 = counters(ks)
            assert ks.verify_all(idx, *f.sig_arrays("affine"), statuses_on_failure=False) == (False, None), scheme
            assert dev_verdict(ks.verify_all(dev(idx), *[dev(c) for c in f.sig_arrays("affine")])) == 0, scheme
            expect_moved(c0, counters(ks))
            ok, st = ks.verify_all(idx, *f.sig_arrays("affine"))
            assert ok is False and st.tobytes() == want.tobytes(), scheme
            expect_moved(c0, counters(ks), small_calls=1)
        # one bad item among 64 valid ones
        good = amc.valid_only(scheme, 64, seed=0x64)
        cols = [good[k] for k in ARG_ORDER[scheme]]
        c0 = counters()
        assert eng.verify_all(scheme, *cols) == (True, None)
        assert dev_verdict(eng.verify_all(scheme, *[dev(c) for c in cols])) == 1
        expect_moved(c0, counters())
        rows = [i for i, c in enumerate(classes) if c == "exact" or (c == "torsion_grid" and want[i] != 0)]
        assert sum(1 for i in rows if classes[i] == "exact") >= 4 and len(rows) >= 100
        both = amc.Forms(scheme, amc.concat(good, amc.subset(b, np.array(rows))))
        keys, idx, _ = amc.registered(scheme, both, "affine")
        with eng.keyset(scheme, *keys) as ks:
            sel = np.arange(64)
            c0 = counters(ks)
            assert ks.verify_all(idx[sel], *[c[sel] for c in both.sig_arrays("affine")]) == (True, None)
            for j in range(len(rows)):
                for pos in (0, 32, 64):
                    sel = np.concatenate([np.arange(pos), [64 + j], np.arange(pos, 64)])
                    what = (scheme, classes[rows[j]], rows[j], pos)
                    one = [c[sel] for c in both.arrays("affine")]
                    assert eng.verify_all(scheme, *one, statuses_on_failure=False) == (False, None), what
                    assert dev_verdict(eng.verify_all(scheme, *[dev(c) for c in one])) == 0, what
                    sigs = [c[sel] for c in both.sig_arrays("affine")]
                    assert ks.verify_all(idx[sel], *sigs, statuses_on_failure=False) == (False, None), what
                    assert dev_verdict(ks.verify_all(dev(idx[sel]), *[dev(c) for c in sigs])) == 0, what
                    placed += 1
            expect_moved(c0, counters(ks))          # none of the placements' calls took the per-item route
    assert placed >= 900

    # ---- the per-item route of verify_all, forced ----------------------------------------------------------------------------------
    assert lib.jjs_debug_force_path(0x4000) == 0
    for scheme in amc.SCHEMES:
        f = amc.forms(scheme)
        want = f.want()
        cols = f.arrays("affine")
        c0 = counters()
        ok, st = eng.verify_all(scheme, *cols)
        assert ok is False and st.tobytes() == want.tobytes(), scheme
        c1 = counters()
        expect_moved(c0, c1, loose=("latency",), lane_calls=1)
        assert dev_verdict(eng.verify_all(scheme, *[dev(c) for c in cols])) == 0, scheme
        expect_moved(c1, counters(), latency=1)
        keys, idx, _ = amc.registered(scheme, f, "affine")
        with eng.keyset(scheme, *keys) as ks:
            c0 = counters(ks)
            ok, st = ks.verify_all(idx, *f.sig_arrays("affine"))
            assert ok is False and st.tobytes() == want.tobytes(), scheme
            assert dev_verdict(ks.verify_all(dev(idx), *[dev(c) for c in f.sig_arrays("affine")])) == 0, scheme
            expect_moved(c0, counters(ks), small_calls=2)
    assert lib.jjs_debug_force_path(0) == 0
    print("ok")


if __name__ == "__main__":
    main()
