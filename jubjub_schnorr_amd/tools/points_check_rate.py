#!/usr/bin/env python3
"""`is_valid` alone (include/jjs_gpu.h jjs_keys_check(_dev)) against the two routes a caller had before it, alternating in one
process on one box; resident buffers; medians; every status of every timed call compared with the expectation.  Writes one JSON
line per shape.
    points_check_rate.py [out.jsonl] [rounds]
Shapes: n = 1, 4 096, 2^15, 2^20 keys; affine, extended and wire; one point per item (single keys) and two (double keys); without
outputs and with the affine points as outputs.
Routes:
  check_dev      jjs_keys_check_dev on resident columns
  check_host     jjs_keys_check from host buffers (the staging copies and the round trip included)
  create_destroy jjs_keyset_create + jjs_keyset_destroy of the same keys in the same format from host buffers, n <= 2^15: the only
                 public source of key_status before (it builds the keys' window tables); jjs_trim follows every one, untimed
  verify_dev     jjs_verify_single_dev of n signatures: a check of one point is a strict part of what one verification computes
The expectation each line confirms or refutes: check_dev takes no longer than verify_dev at any shape.  No thresholds: the lines
are measurements; `slower_than_verify` names the shapes that refute it.
The expected statuses come from jjs_debug_point_flags_dev ([r]P by double-and-add, not the residue test) and a range test on the
host."""
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

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def extended(eng, pts, seed):
    """Affine (n, 64) on the device -> (n, 96) = u Z || v Z || Z with a random Z per point (the engine's own multiplier)."""
    import torch
    z = np.random.default_rng(seed).integers(0, 256, (pts.shape[0], 32), dtype=np.uint8)
    z[:, 31] &= 0x3F; z[:, 0] |= 1
    zd = torch.from_numpy(z).cuda()
    return torch.cat([eng.debug_fq_mul(pts[:, :32].contiguous(), zd), eng.debug_fq_mul(pts[:, 32:].contiguous(), zd), zd], 1).contiguous()


def expected(eng, pts):
    """The status of every affine point of a resident column, without the code under test."""
    import torch
    flags = eng.debug_point_flags(pts)
    torch.cuda.synchronize()
    st = np.where((flags.cpu().numpy() & 7) == 3, 0, 1).astype(np.uint8)
    host = pts.cpu().numpy()
    for half in (host[:, :32], host[:, 32:]):
        for i in np.where(half[:, 31] >= 0x73)[0]:
            if int.from_bytes(half[i].tobytes(), "little") >= Q:
                st[i] = 3
    return st


def timed(fn, want):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    got = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    if not np.array_equal(got, want):
        raise SystemExit(f"status mismatch ({int((got != want).sum())} items)")
    return dt


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16_points_check.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = jjs.engine()
    lines, slower = [], []
    for n in (1, 4096, 1 << 15, 1 << 20):
        a, _ = bench.make_inputs(eng, "double", max(n, 2), 0, n_keys=max(n, 2))
        a = {k: v[:n].contiguous() for k, v in a.items()}
        s, s_want = bench.make_inputs(eng, "single", max(n, 2), 0, n_keys=max(n, 2))
        s = {k: v[:n].contiguous() for k, v in s.items()}
        s_want = s_want[:n].cpu().numpy()
        want_col = [expected(eng, a["PK"]), expected(eng, a["PKp"])]
        for pts in (1, 2):
            scheme = "single" if pts == 1 else "double"
            want = want_col[0] if pts == 1 else np.maximum(want_col[0], want_col[1])
            affine = [a["PK"], a["PKp"]][:pts]
            for fmt in ("affine", "ext", "wire"):
                if fmt == "affine":
                    cols = affine
                elif fmt == "ext":
                    cols = [extended(eng, c, 5 + i) for i, c in enumerate(affine)]
                else:
                    cols = [torch.cat([eng.compress(c) for c in affine], 1).contiguous()]
                host = [c.cpu().numpy() for c in cols]
                for outputs in (False, True):
                    routes = {
                        "check_dev": lambda: eng.keys_check(scheme, *cols, fmt=fmt, want_points=outputs)[0],
                        "check_host": lambda: eng.keys_check(scheme, *host, fmt=fmt, want_points=outputs)[0],
                        "verify_dev": lambda: eng.verify("single", s["u"], s["R"], s["PK"], s["m"])[0],
                    }
                    wants = {"check_dev": want, "check_host": want, "verify_dev": s_want, "create_destroy": want}
                    if n <= 1 << 15 and not outputs:
                        def create():
                            with eng.keyset(scheme, host[0], host[1] if len(host) > 1 else None, fmt=fmt) as ks:
                                return ks.key_status
                        routes["create_destroy"] = create
                    def run(name):
                        dt = timed(routes[name], wants[name])
                        if name == "create_destroy":
                            eng.trim()               # untimed: a destroyed set's memory (204 KB of tables per key) goes back only here
                        return dt
                    for name in routes:
                        run(name)
                    t = {name: [] for name in routes}
                    for _ in range(rounds):
                        for name in routes:
                            t[name].append(run(name))
                    rec = {"case": "keys_check", "items": n, "points_per_item": pts, "fmt": fmt, "outputs": outputs, "rounds": rounds,
                           "status_mismatches": 0, "tally": [int((want == k).sum()) for k in range(4)],
                           "device": torch.cuda.get_device_name(0)}
                    for name, v in t.items():
                        rec[name + "_ms"] = statistics.median(v)
                        rec[name + "_spread_ms"] = max(v) - min(v)
                    rec["check_over_verify"] = rec["check_dev_ms"] / rec["verify_dev_ms"]
                    if "create_destroy_ms" in rec:
                        rec["check_host_over_create_destroy"] = rec["check_host_ms"] / rec["create_destroy_ms"]
                    if rec["check_over_verify"] > 1.0:
                        slower.append({k: rec[k] for k in ("items", "points_per_item", "fmt", "outputs", "check_over_verify")})
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
                del cols, host
    summary = {"case": "summary", "expectation": "check_dev_ms <= verify_dev_ms at every shape", "slower_than_verify": slower}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
