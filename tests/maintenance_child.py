"""Child process of tests/test_maintenance_gpu.py: the engine's maintenance calls -- jjs_reserve, jjs_trim, jjs_memory_stats,
jjs_path_stats -- from one thread while up to eight other threads keep verification calls in flight through the product
library.  `python maintenance_child.py MODE`, MODE one of reserve-lanes, reserve-large, reserve-resident, trim.  Every call's
full status vector and its tally are compared with statuses that do not come from the engine: the C oracle's for the small
batches; for the batches signed on the device, every seventh message tampered with, the statuses that construction gives, the
first 4 096 items of each held against the C oracle.  A mismatch or an error of a call is counted, not raised: the run goes on to
its end.  Prints one JSON line and exits 0 only when every check of the mode held."""
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import maintenance_cases as cases  # noqa: E402
from helpers import ARG_ORDER, make_batch, oracle_verify  # noqa: E402

ORACLE_HEAD = 4096          # items of a device-signed batch that the C oracle sees


def tally_of(want):
    return [int((want == k).sum()) for k in range(4)]


def small_work():
    """(scheme, host arrays, expected statuses) of the small calls: per scheme ONE mixed batch of 1 024 items whose statuses the
    oracle computes once; the calls of 1 024 items are the batch, those of 64 a run of it that holds every status, those of one
    item an item of each status in turn -- an all-zero status column never passes for more than one call of three."""
    work = {n: [] for n in cases.SMALL_CALL_ITEMS}
    for scheme, seed in (("single", 7301), ("double", 7302)):
        b = make_batch(scheme, 1024, seed=seed, n_keys=8)
        want = oracle_verify(scheme, b)
        assert set(want.tolist()) >= {0, 1, 2}, (scheme, sorted(set(want.tolist())))

        def cut(lo, hi):
            return scheme, [np.ascontiguousarray(b[k][lo:hi]) for k in ARG_ORDER[scheme]], want[lo:hi].copy()
        work[1024].append(cut(0, 1024))
        runs = [lo for lo in range(0, 1024 - 64 + 1) if set(want[lo:lo + 64].tolist()) >= {0, 1, 2}]
        assert runs, f"{scheme}: no run of 64 items holds the statuses 0, 1 and 2"
        work[64].append(cut(runs[0], runs[0] + 64))
        for status in (0, 1, 2):
            i = int(np.where(want == status)[0][0])
            work[1].append(cut(i, i + 1))
    assert {int(w[0]) for _, _, w in work[1]} == {0, 1, 2}
    return work


def signed_batch(eng, n, n_keys, seed):
    """n single signatures from the device signer over n_keys keys, every seventh message tampered with: (host arrays, device
    tensors, expected statuses).  The first ORACLE_HEAD items are held against the C oracle."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)

    def scal(rows, top):
        t = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, generator=gen)
        t[:, 31] &= top
        return t
    keys = scal(n_keys, 0x07)
    keys[:, 0] |= 1
    sk = keys[torch.arange(n) % n_keys].contiguous().cuda()
    rnd, m = scal(n, 0x07).cuda(), scal(n, 0x3F).cuda()
    u, R, PK = eng.sign("single", sk, rnd, m)
    bad = (torch.arange(n, device="cuda") % 7) == 3
    m[bad, 0] ^= 1
    torch.cuda.synchronize()
    dev = [u, R, PK, m]
    host = [np.ascontiguousarray(t.cpu().numpy()) for t in dev]
    want = (bad.to(torch.uint8) * 2).cpu().numpy()
    head = oracle_verify("single", {k: a[:ORACLE_HEAD] for k, a in zip(ARG_ORDER["single"], host)})
    assert (head == want[:ORACLE_HEAD]).all(), "the statuses by construction are not the oracle's"
    assert set(want.tolist()) == {0, 2}
    return host, dev, want


class Run:
    """What the threads of a mode share: the log of the calls, the mismatches, the errors."""

    def __init__(self):
        self.cv = threading.Condition()
        self.calls = {}              # kind -> [(start, end)]
        self.wrong_calls = 0
        self.wrong_statuses = 0
        self.wrong_tallies = 0
        self.errors = []
        self.done = threading.Event()

    def count(self, kind=None):
        return sum(len(v) for k, v in self.calls.items() if kind in (None, k))

    def note(self, kind, t0, t1, st, tally, want):
        wrong = int((np.asarray(st) != want).sum())
        bad_tally = [int(x) for x in tally] != tally_of(want)
        with self.cv:
            self.calls.setdefault(kind, []).append((t0, t1))
            self.wrong_statuses += wrong
            self.wrong_calls += 1 if wrong else 0
            self.wrong_tallies += 1 if bad_tally else 0
            self.cv.notify_all()

    def error(self, where, e):
        with self.cv:
            self.errors.append(f"{where}: {type(e).__name__}: {e}"[:300])
            self.cv.notify_all()

    def await_calls(self, kind, more):
        """Blocks until `more` further calls of `kind` have ended (or a caller has failed)."""
        with self.cv:
            target = self.count(kind) + more
            self.cv.wait_for(lambda: self.count(kind) >= target or self.errors)

    def overlapped(self, kind, t0, t1):
        with self.cv:
            return any(a < t1 and b > t0 for a, b in self.calls.get(kind, []))


def host_caller(run, eng, items, kind, floor, first=0):
    """A thread of blocking host-buffer calls, back to back over `items` = [(scheme, arrays, want)], until the maintenance
    thread is done and the run has `floor` calls of `kind`."""
    def loop():
        i = first
        try:
            while not (run.done.is_set() and run.count(kind) >= floor) and not run.errors:
                scheme, arrays, want = items[i % len(items)]
                i += 1
                t0 = time.perf_counter()
                st, tally = eng.verify(scheme, *arrays)
                run.note(kind, t0, time.perf_counter(), st, tally, want)
        except Exception as e:  # noqa: BLE001
            run.error(kind, e)
    return threading.Thread(target=loop)


def dev_caller(run, eng, items, kind, floor, first=0):
    """A thread of resident calls on a stream of its own, each waited for and compared; items = [(device tensors, want)]."""
    import torch

    def loop():
        i = first
        try:
            stream = torch.cuda.Stream()
            while not (run.done.is_set() and run.count(kind) >= floor) and not run.errors:
                tensors, want = items[i % len(items)]
                i += 1
                t0 = time.perf_counter()
                with torch.cuda.stream(stream):
                    st, tally = eng.verify("single", *tensors)
                stream.synchronize()
                run.note(kind, t0, time.perf_counter(), st.cpu().numpy(), tally.cpu().numpy(), want)
        except Exception as e:  # noqa: BLE001
            run.error(kind, e)
    return threading.Thread(target=loop)


def small_callers(run, eng, work, threads, floor):
    flat = [item for n in cases.SMALL_CALL_ITEMS for item in work[n]]
    return [host_caller(run, eng, flat, "small", floor, first=3 * t) for t in range(threads)]


def drive(run, callers, maintenance):
    """Starts the callers, runs `maintenance` on a ninth thread, joins everybody."""
    def guarded():
        try:
            maintenance()
        except Exception as e:  # noqa: BLE001
            run.error("maintenance", e)
        finally:
            run.done.set()
    assert len(callers) <= 8
    m = threading.Thread(target=guarded)
    for t in callers:
        t.start()
    m.start()
    m.join()
    for t in callers:
        t.join()


def reserve_steps(run, eng, plan, kind, calls_between):
    """Walks a plan of (scheme, fmt, n, host_buffers) beside the calls: host staging before and after every step, and when the
    step began and ended (overlaps() looks the calls of that time up once every caller has joined)."""
    steps = []
    for scheme, fmt, n, host_buffers in plan:
        run.await_calls(kind, calls_between)
        before = eng.memory_stats()["host_staging"]
        t0 = time.perf_counter()
        eng.reserve(scheme, n, fmt=fmt, host_buffers=host_buffers)
        t1 = time.perf_counter()
        after = eng.memory_stats()["host_staging"]
        steps.append({"scheme": scheme, "fmt": fmt, "n": n, "staging_before": before, "staging_after": after, "t0": t0, "t1": t1})
    return steps


def overlaps(run, kind, steps):
    for s in steps:
        s["overlapped"] = run.overlapped(kind, s["t0"], s["t1"])
        s["ms"] = round((s.pop("t1") - s.pop("t0")) * 1e3, 3)
    return steps


def summary(run, **more):
    r = {"calls": {k: len(v) for k, v in run.calls.items()}, "wrong_calls": run.wrong_calls, "wrong_statuses": run.wrong_statuses,
         "wrong_tallies": run.wrong_tallies, "errors": run.errors[:8]}
    r.update(more)
    return r


def exact(run):
    return not run.errors and run.wrong_calls == 0 and run.wrong_statuses == 0 and run.wrong_tallies == 0


def mode_reserve_lanes(eng, lib):
    work = small_work()
    plan = [(s, f, n, True) for s, f, n in cases.lane_plan()]
    lifetimes, runs = [], []
    for life in range(2):
        if life:                     # a second engine in the same process: its lanes start from nothing again
            lib.jjs_shutdown()
            assert lib.jjs_init(1) == 0
        run = Run()
        runs.append(run)
        steps = []
        drive(run, small_callers(run, eng, work, 8, 500), lambda: steps.extend(reserve_steps(run, eng, plan, "small", 80)))
        lifetimes.append(overlaps(run, "small", steps))
    grew = [[s["staging_after"] > s["staging_before"] for s in steps] for steps in lifetimes]
    checks = {
        "exact": all(exact(r) for r in runs),
        "every_reserve_grew_the_lanes": all(len(g) == len(plan) >= 5 and all(g) for g in grew),
        "every_reserve_overlapped_a_call": all(s["overlapped"] for steps in lifetimes for s in steps),
        "at_least_1000_calls": sum(r.count("small") for r in runs) >= 1000,
    }
    total = Run()
    for r in runs:
        total.wrong_calls += r.wrong_calls; total.wrong_statuses += r.wrong_statuses; total.wrong_tallies += r.wrong_tallies
        total.errors += r.errors
        for k, v in r.calls.items():
            total.calls.setdefault(k, []).extend(v)
    return checks, summary(total, growth=[[(s["n"], s["staging_before"], s["staging_after"]) for s in steps] for steps in lifetimes])


def mode_reserve_large(eng, lib):
    work = small_work()
    host, _, want = signed_batch(eng, cases.LARGE_CALL_ITEMS, 64, seed=4)
    run = Run()
    callers = [host_caller(run, eng, [("single", host, want)], "large", 40) for _ in range(2)] + small_callers(run, eng, work, 6, 0)
    plan = [("single", "affine", n, True) for n in cases.large_plan()]
    steps = []
    drive(run, callers, lambda: steps.extend(reserve_steps(run, eng, plan, "large", 4)))
    overlaps(run, "large", steps)
    grew =[s for s in steps if s["staging_after"] > s["staging_before"]]
    checks = {
        "exact": exact(run),
        "staging_rose_four_times": len(grew) >= 4,
        "every_growth_overlapped_a_large_call": all(s["overlapped"] for s in grew),
        "at_least_40_large_calls": run.count("large") >= 40,
    }
    return checks, summary(run, growth=[(s["n"], s["staging_before"], s["staging_after"]) for s in steps])


def resident_items(eng):
    import torch
    b = make_batch("single", 1000, seed=7310, n_keys=8)
    want = oracle_verify("single", b)
    assert set(want.tolist()) >= {0, 1, 2}
    mixed = ([torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ARG_ORDER["single"]], want)
    _, dev, want_keyed = signed_batch(eng, 65536, 256, seed=5)       # 256 signatures a key: the key-table path
    return [mixed, (dev, want_keyed)]


def mode_reserve_resident(eng, lib):
    items = resident_items(eng)
    run = Run()
    callers = [dev_caller(run, eng, items, "resident", 40, first=t) for t in range(4)]
    seen, not_monotonic, memory = [eng.path_stats()], [], []

    def maintenance():
        for n in cases.resident_plan():
            run.await_calls("resident", 4)
            eng.reserve("single", n, host_buffers=False)
            for _ in range(3):
                s = eng.path_stats()
                not_monotonic.extend(k for k in s if k != "key_pool_bytes" and s[k] < seen[-1][k])
                seen.append(s)
                memory.append(eng.memory_stats())
    drive(run, callers, maintenance)
    import torch
    torch.cuda.synchronize()
    last = eng.path_stats()
    checks = {
        "exact": exact(run),
        "path_stats_never_decreased": not not_monotonic and all(last[k] >= seen[-1][k] for k in last if k != "key_pool_bytes"),
        "key_tables_ran": last["key_tables_wide"] + last["key_tables_narrow"] > seen[0]["key_tables_wide"] + seen[0]["key_tables_narrow"],
        "at_least_40_calls": run.count("resident") >= 40,
    }
    return checks, summary(run, path_stats=last, slot_buffers=[m["slot_buffers"] for m in memory][::3])


def mode_trim(eng, lib):
    work = small_work()
    host, _, want = signed_batch(eng, cases.LARGE_CALL_ITEMS, 64, seed=4)
    items = resident_items(eng)
    # every reserve comes first: nothing grows, and so nothing is retired, by a reserve beside the calls
    for scheme, fmt, n in cases.lane_plan():
        eng.reserve(scheme, n, fmt=fmt, host_buffers=True)
    eng.reserve("single", cases.large_plan()[-1], host_buffers=True)
    eng.reserve("single", cases.resident_plan()[-1], host_buffers=False)
    run = Run()
    callers = small_callers(run, eng, work, 6, 300) + [host_caller(run, eng, [("single", host, want)], "large", 20),
                                                       dev_caller(run, eng, items, "resident", 20)]
    trims = []

    def maintenance():
        for _ in range(20):
            run.await_calls(None, 24)
            t0 = time.perf_counter()
            rc = lib.jjs_trim()
            trims.append({"rc": int(rc), "t0": t0, "t1": time.perf_counter()})
    drive(run, callers, maintenance)
    rc_last = int(lib.jjs_trim())
    after = eng.memory_stats()
    for t in trims:
        t["overlapped"] = any(run.overlapped(k, t["t0"], t["t1"]) for k in ("small", "large", "resident"))
        t["ms"] = (t["t1"] - t["t0"]) * 1e3
    checks = {
        "exact": exact(run),
        "twenty_trims_returned_0": len(trims) == 20 and all(t["rc"] == 0 for t in trims),
        "every_trim_overlapped_a_call": all(t["overlapped"] for t in trims),
        "last_trim_left_nothing_retired": rc_last == 0 and after["retired"] == 0,
        "every_kind_of_call_ran": all(run.count(k) >= 20 for k in ("small", "large", "resident")),
    }
    return checks, summary(run, trim_ms=[round(t["ms"], 2) for t in trims], after_last_trim=after)


MODES = {"reserve-lanes": mode_reserve_lanes, "reserve-large": mode_reserve_large, "reserve-resident": mode_reserve_resident,
         "trim": mode_trim}


def main(mode: str) -> int:
    import torch
    torch.cuda.init()
    import jubjub_schnorr_amd as jjs
    t_start = time.perf_counter()
    eng = jjs.engine()
    checks, record = MODES[mode](eng, eng._lib)
    ok = all(checks.values())
    print(json.dumps({"mode": mode, "ok": bool(ok), "checks": {k: bool(v) for k, v in checks.items()},
                      "wall_s": round(time.perf_counter() - t_start, 3), **record}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
