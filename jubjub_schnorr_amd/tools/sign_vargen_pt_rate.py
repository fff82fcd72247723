#!/usr/bin/env python3
"""Var-generator signing with the generator as a point (include/jjs_gpu.h jjs_sign_vargen_pt_dev) beside the signer that takes the
generator as a scalar (jjs_sign_vargen_dev, the yardstick), alternating in one process on one box on identical resident inputs.
One JSON line per shape.
    sign_vargen_pt_rate.py [out.jsonl] [rounds]
Shapes: n = 1, 64, 1 024, 16 384, 2^18, 2^20.  The material is made on the device: random scalars below 2^251, the generators
Gen = gen_scalar * G by the yardstick itself.  Variants:
    a_scalar     jjs_sign_vargen_dev on gen_scalar
    b_affine     the per-item route on Gen, affine              c_ext   the same, extended (random Z)        d_wire  the same, compressed
    e_one_item   n_gen == 1 (the first generator), the per-item route (stride 0) forced (jjs_debug_force_path 0x200000)
    f_one_shared n_gen == 1, the shared-generator route forced (0x8000).  The profiling build is loaded for these two switches, and
                 every variant runs in it.
Every shape is checked once before it is timed: b, c and d give a's bytes, f gives e's, every status 0.
Per shape and variant: ms per call (median, min, max over the rounds; spread = max - min) and signatures per second at the
median; `b_over_a` and `f_over_e` are ratios of medians; the shader clock is read before and after the rounds."""
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


def to_extended(eng, Gen, g):
    """(n, 64) affine device points -> (n, 96) U || V || Z with random Z, by the engine's own field product."""
    import torch
    n = Gen.shape[0]
    z = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    z[:, 31] &= 0x3F
    z[:, 0] |= 1
    z = z.contiguous()
    U = eng.debug_fq_mul(Gen[:, :32].contiguous(), z)
    V = eng.debug_fq_mul(Gen[:, 32:].contiguous(), z)
    return torch.cat([U, V, z], dim=1).contiguous()


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_sign_vargen_pt.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    _ffi.select_library(_ffi.PROFILING_LIB_PATH)
    eng = jjs.engine()
    lib = _ffi.lib()
    device = torch.cuda.get_device_name(0)
    limits = eng.sign_limits()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    for k, n in enumerate((1, 64, 1024, 16384, 1 << 18, 1 << 20)):
        g = torch.Generator(device="cuda").manual_seed(1700 + k)

        def scalars(top):
            x = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
            x[:, 31] &= top
            x[:, 0] |= 1
            return x.contiguous()
        sk, gs, rnd, m = scalars(0x07), scalars(0x07), scalars(0x07), scalars(0x3F)      # < 2^251 < r; m < 2^254 < q
        want = eng.sign("vargen", sk, rnd, m, gen_scalar=gs)
        Gen = want[3]
        cols = {"b_affine": ("affine", Gen), "c_ext": ("ext", to_extended(eng, Gen, g)), "d_wire": ("wire", eng.compress(Gen))}
        one = Gen[:1].contiguous()

        def routed(bit):
            def call():
                assert lib.jjs_debug_force_path(bit) == 0
                r = eng.sign_vargen_pt(sk, one, rnd, m)
                assert lib.jjs_debug_force_path(0) == 0
                return r
            return call
        calls = {"a_scalar": lambda: eng.sign("vargen", sk, rnd, m, gen_scalar=gs)}
        for name, (fmt, col) in cols.items():
            calls[name] = (lambda fmt=fmt, col=col: eng.sign_vargen_pt(sk, col, rnd, m, fmt=fmt))
        calls["e_one_item"] = routed(0x200000)
        calls["f_one_shared"] = routed(0x8000)
        # checked once before it is timed
        for name in cols:
            got = calls[name]()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(got[:4], want)) and not int(got[4].max()), name
        e, sh = calls["e_one_item"](), calls["f_one_shared"]()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(e, sh)) and not int(e[4].max()) and torch.equal(e[3], one)
        del got, e, sh
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
        rec = {"n": n, "rounds": rounds, "device": device, "library": "profiling build", "resident_lanes": limits["resident_lanes"],
               "shared_generator_from": limits["shared_generator_from"], "shader_clock_mhz": [clock_before, shader_clock_mhz()]}
        for name, xs in t.items():
            rec[name + "_ms"] = stats(xs)
            rec[name + "_per_s"] = round(n / (rec[name + "_ms"]["median"] * 1e-3))
        rec["b_over_a"] = round(rec["b_affine_ms"]["median"] / rec["a_scalar_ms"]["median"], 3)
        rec["f_over_e"] = round(rec["f_one_shared_ms"]["median"] / rec["e_one_item_ms"]["median"], 3)
        # f beats e by more than the spread of either side
        rec["f_wins"] = bool(rec["e_one_item_ms"]["median"] - rec["f_one_shared_ms"]["median"] >
                             max(rec["e_one_item_ms"]["spread"], rec["f_one_shared_ms"]["spread"]))
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")
        f.flush()
        del sk, gs, rnd, m, want, Gen, cols, one, calls
        eng.trim()
        torch.cuda.empty_cache()
    f.close()


if __name__ == "__main__":
    main()
