#!/usr/bin/env python3
"""Signing and key derivation with a SecretKey (include/jjs_gpu.h jjs_sign_fixed_dev, jjs_public_keys_fixed_dev) beside the old
signers (jjs_sign_single_dev / jjs_sign_double_dev, jjs_public_keys_dev: the yardsticks), alternating in one process on one box on
identical resident inputs.  One JSON line per scheme and shape.
    sign_fixed_rate.py [out.jsonl] [rounds]
Shapes: both schemes at n = 1, 64, 1 024, 16 384, 2^18, 2^20.  The material is made on the device: random scalars below 2^251,
messages below 2^254.  Variants:
    a_old        jjs_sign_single_dev / jjs_sign_double_dev
    b_affine     the new call with n_sk = n, affine outputs     c_wire  the same with the wire outputs as well
    d_one_item   n_sk == 1 (the first key), the per-item route (stride 0) forced (jjs_debug_force_path 0x800000)
    e_one_keyed  n_sk == 1, the keyed route forced (0x400000).  The profiling build is loaded for these two switches, and every
                 variant runs in it.
    f_derive     jjs_public_keys_fixed_dev                      f_old   jjs_public_keys_dev
Every shape is checked once before it is timed: b and c give a's bytes and the compression of them, e gives d's, d's signatures
are those of the old signer on the key tiled, f gives f_old's keys, every status 0.
Per shape and variant: ms per call (median, min, max over the rounds; spread = max - min) and items per second at the median;
`b_over_a`, `c_over_a`, `e_over_d` and `f_over_f_old` are ratios of medians; `e_wins`: e beats d by more than the spread of either
side; the shader clock is read before and after the rounds."""
import json
import os
import statistics
import subprocess
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

import jubjub_schnorr_amd as jjs  # noqa: E402
from jubjub_schnorr_amd import _ffi  # noqa: E402


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "spread": round(max(xs) - min(xs), 4)}


def shader_clock_mhz():
    """The current shader clock of device 0 as rocm-smi prints it (a read; nothing is set), or None."""
    try:
        text = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        for card in json.loads(text).values():
            for key, value in card.items():
                if "sclk" in key.lower() and "mhz" in str(value).lower():
                    return int("".join(ch for ch in str(value).split("Mhz")[0].split("MHz")[0] if ch.isdigit()))
    except Exception:
        pass
    return None


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_sign_fixed.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    device = torch.cuda.get_device_name(0)
    limits = eng.sign_fixed_limits()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    for scheme in ("single", "double"):
        dbl = scheme == "double"
        n_pts = 4 if dbl else 2                                 # the affine columns behind u: R [R'] PK [PK']
        for k, n in enumerate((1, 64, 1024, 16384, 1 << 18, 1 << 20)):
            g = torch.Generator(device="cuda").manual_seed(1800 + k)

            def scalars(top):
                x = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
                x[:, 31] &= top
                x[:, 0] |= 1
                return x.contiguous()
            sk, rnd, m = scalars(0x07), scalars(0x07), scalars(0x3F)      # < 2^251 < r; m < 2^254 < q
            one = sk[:1].contiguous()

            def routed(bit):
                def call():
                    assert lib.jjs_debug_force_path(bit) == 0
                    r = eng.sign_fixed(scheme, one, rnd, m)
                    assert lib.jjs_debug_force_path(0) == 0
                    return r
                return call
            calls = {"a_old": lambda: eng.sign(scheme, sk, rnd, m),
                     "b_affine": lambda: eng.sign_fixed(scheme, sk, rnd, m),
                     "c_wire": lambda: eng.sign_fixed(scheme, sk, rnd, m, wire=True),
                     "d_one_item": routed(0x800000), "e_one_keyed": routed(0x400000),
                     "f_derive": lambda: eng.public_keys_fixed(scheme, sk),
                     "f_old": lambda: eng.public_keys(sk, double=dbl)}
            # checked once before it is timed
            want = calls["a_old"]()
            b, c = calls["b_affine"](), calls["c_wire"]()
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(b[:1 + n_pts], want)) and not int(b[-1].max()), "b"
            assert all(torch.equal(x, y) for x, y in zip(c[:1 + n_pts], want)) and not int(c[-1].max()), "c"
            pts = [eng.compress(x) for x in want[1:]]
            assert torch.equal(c[-3], torch.cat([want[0]] + pts[:n_pts // 2], 1)) and torch.equal(c[-2], torch.cat(pts[n_pts // 2:], 1)), "c, wire"
            d, e = calls["d_one_item"](), calls["e_one_keyed"]()
            tiled = eng.sign(scheme, one.expand(n, 32).contiguous(), rnd, m)
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(d, e)) and not int(d[-1].max()), "d, e"
            assert all(torch.equal(x, y) for x, y in zip(d[:1 + n_pts // 2], tiled)) and torch.equal(d[1 + n_pts // 2], tiled[1 + n_pts // 2][:1]), "d"
            fn, fo = calls["f_derive"](), calls["f_old"]()
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(fn[:-1], fo[:-1])) and not int(fn[-1].max()) and not int(fo[-1].max()), "f"
            del want, b, c, d, e, tiled, fn, fo, pts
            t = {name: [] for name in calls}
            clock_before = shader_clock_mhz()
            for rd in range(rounds + 2):                        # two warm-up rounds: first-use allocations, clocks
                for name, fn in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rd >= 2:
                        t[name].append((time.perf_counter() - t0) * 1e3)
            rec = {"scheme": scheme, "n": n, "rounds": rounds, "device": device, "library": "profiling build",
                   "resident_lanes": limits["resident_lanes"], "keyed_from": limits["keyed_from"],
                   "shader_clock_mhz": [clock_before, shader_clock_mhz()]}
            for name, xs in t.items():
                rec[name + "_ms"] = stats(xs)
                rec[name + "_per_s"] = round(n / (rec[name + "_ms"]["median"] * 1e-3))
            med = lambda name: rec[name + "_ms"]["median"]  # noqa: E731
            rec["b_over_a"] = round(med("b_affine") / med("a_old"), 3)
            rec["c_over_a"] = round(med("c_wire") / med("a_old"), 3)
            rec["e_over_d"] = round(med("e_one_keyed") / med("d_one_item"), 3)
            rec["f_over_f_old"] = round(med("f_derive") / med("f_old"), 3)
            # e beats d by more than the spread of either side
            rec["e_wins"] = bool(med("d_one_item") - med("e_one_keyed") > max(rec["d_one_item_ms"]["spread"], rec["e_one_keyed_ms"]["spread"]))
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            f.flush()
            del sk, rnd, m, one, calls
            eng.trim()
            torch.cuda.empty_cache()
    f.close()


if __name__ == "__main__":
    main()
