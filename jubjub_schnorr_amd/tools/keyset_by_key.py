#!/usr/bin/env python3
"""Key sets by key against key sets by index and the inline calls (include/jjs_gpu.h jjs_keyset_verify_keys_dev), the three
modes alternating in one process on one box.  Every call's statuses are compared with the batch's construction.  Writes one
JSON line per case.
    keyset_by_key.py [out.jsonl] [rounds]
Shapes: those of keyset_calls.py (profiles/r05_keyset.jsonl), resident:
  repeat_across   2^17 single signatures over 2^15 registered keys, in the affine, extended and wire formats
  small           1, 64, 1 024, 16 384 items, every scheme
  survey_8d       2^20 single signatures over 4 096 keys
and the time of jjs_keyset_create for 2^15 keys (the lookup table is built inside it).
The expectation each line confirms or refutes: by key costs the by-index time plus the probe (and the normalisation of the
key columns for extended keys), so it beats inline wherever by index does.  No thresholds: the lines are measurements."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import jubjub_schnorr_amd as jjs  # noqa: E402

KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}
MODES = ("inline", "by_index", "by_key")


def batch(eng, scheme, n, n_keys):
    """Resident inputs, the expected statuses, the distinct keys (host) and each item's index among them."""
    a, expect = bench.make_inputs(eng, scheme, n, 0, n_keys=n_keys)
    cat = np.concatenate([a[k].cpu().numpy() for k in KEYCOLS[scheme]], 1)
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    keys = [np.ascontiguousarray(uniq[:, 64 * i:64 * i + 64]) for i in range(len(KEYCOLS[scheme]))]
    return a, expect.cpu().numpy(), keys, inv.reshape(-1).astype(np.uint32)


def extended(eng, pts, seed):
    """Affine (n, 64) on the device -> (n, 96) = u Z || v Z || Z with a random Z per point (the engine's own multiplier)."""
    import torch
    z = np.random.default_rng(seed).integers(0, 256, (pts.shape[0], 32), dtype=np.uint8)
    z[:, 31] &= 0x3F; z[:, 0] |= 1
    zd = torch.from_numpy(z).cuda()
    return torch.cat([eng.debug_fq_mul(pts[:, :32].contiguous(), zd), eng.debug_fq_mul(pts[:, 32:].contiguous(), zd), zd], 1).contiguous()


def timed(fn, want):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = fn()[0]
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    got = st.cpu().numpy()
    if not np.array_equal(got, want):
        raise SystemExit(f"status mismatch ({int((got != want).sum())} items)")
    return dt


def abc(rounds, fns, want):
    """fns: one callable per mode of MODES.  Alternating rounds after one warm-up call of each; medians and spreads in ms."""
    for f in fns:
        timed(f, want)
    t = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            t[k].append(timed(f, want))
    rec = {"status_mismatches": 0, "rounds": rounds}
    for name, v in zip(MODES, t):
        rec[name + "_ms"] = statistics.median(v)
        rec[name + "_spread_ms"] = max(v) - min(v)
    rec["by_key_over_inline"] = rec["by_key_ms"] / rec["inline_ms"]
    rec["by_index_over_inline"] = rec["by_index_ms"] / rec["inline_ms"]
    rec["by_key_minus_by_index_ms"] = rec["by_key_ms"] - rec["by_index_ms"]
    return rec


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_keyset_by_key.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = jjs.engine()
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    # 1. keys that repeat across calls, not within one; the three formats; and what registering 2^15 keys takes
    a, want, keys, idx = batch(eng, "single", 1 << 17, 1 << 15)
    didx = torch.from_numpy(idx).cuda()
    create = []
    for _ in range(rounds + 1):
        t0 = time.perf_counter()
        with eng.keyset("single", keys[0]):
            create.append((time.perf_counter() - t0) * 1e3)
    emit({"case": "keyset_create", "scheme": "single", "keys": len(keys[0]), "create_ms": statistics.median(create[1:]),
          "create_spread_ms": max(create[1:]) - min(create[1:]), "first_create_ms": create[0], "rounds": rounds})
    with eng.keyset("single", keys[0]) as ks:
        r = abc(rounds, [lambda: eng.verify("single", a["u"], a["R"], a["PK"], a["m"]), lambda: ks.verify(didx, a["u"], a["R"], a["m"]),
                         lambda: ks.verify_keys([a["PK"]], a["u"], a["R"], a["m"])], want)
        r.update(case="repeat_across", fmt="affine", scheme="single", items=1 << 17, keys=len(keys[0]))
        emit(r)
        Rx, PKx = extended(eng, a["R"], 1), extended(eng, a["PK"], 2)
        r = abc(rounds, [lambda: eng.verify_ext("single", a["u"], Rx, PKx, a["m"]), lambda: ks.verify(didx, a["u"], Rx, a["m"], fmt="ext"),
                         lambda: ks.verify_keys([PKx], a["u"], Rx, a["m"], fmt="ext")], want)
        r.update(case="repeat_across", fmt="ext", scheme="single", items=1 << 17, keys=len(keys[0]))
        emit(r)
        sig, pk = torch.cat([a["u"], eng.compress(a["R"])], 1).contiguous(), eng.compress(a["PK"])
        r = abc(rounds, [lambda: eng.verify_wire("single", sig, pk, a["m"]), lambda: ks.verify(didx, sig, a["m"], fmt="wire"),
                         lambda: ks.verify_keys([pk], sig, a["m"], fmt="wire")], want)
        r.update(case="repeat_across", fmt="wire", scheme="single", items=1 << 17, keys=len(keys[0]))
        emit(r)
        del Rx, PKx, sig, pk

    # 2. small resident calls
    for scheme in ("single", "double", "vargen"):
        a, want, keys, idx = batch(eng, scheme, 16384, 256)
        with eng.keyset(scheme, *keys) as ks:
            for n in (1, 64, 1024, 16384):
                sub = {k: v[:n].contiguous() for k, v in a.items()}
                di = torch.from_numpy(idx[:n].copy()).cuda()
                sig = [sub["u"]] + [sub[k] for k in RCOLS[scheme]] + [sub["m"]]
                K = [sub[k] for k in KEYCOLS[scheme]]
                r = abc(rounds, [lambda: eng.verify(scheme, *[sub[k] for k in bench.ARG_ORDER[scheme]]), lambda: ks.verify(di, *sig),
                                 lambda: ks.verify_keys(K, *sig)], want[:n])
                r.update(case="small", fmt="affine", scheme=scheme, items=n, keys=len(keys[0]))
                emit(r)

    # 3. SURVEY 8(d): 2^20 single signatures over 4 096 keys
    a, want, keys, idx = batch(eng, "single", 1 << 20, 4096)
    didx = torch.from_numpy(idx).cuda()
    with eng.keyset("single", keys[0]) as ks:
        r = abc(rounds, [lambda: eng.verify("single", a["u"], a["R"], a["PK"], a["m"]), lambda: ks.verify(didx, a["u"], a["R"], a["m"]),
                         lambda: ks.verify_keys([a["PK"]], a["u"], a["R"], a["m"])], want)
        r.update(case="survey_8d_resident", fmt="affine", scheme="single", items=1 << 20, keys=4096)
        emit(r)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
