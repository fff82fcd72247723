#!/usr/bin/env python3
"""The signer's multisignature call (include/jjs_gpu.h jjs_multisig_sign_dev, signer_row = NULL: every row of every transcript
signs) beside jjs_multisig_combine_dev on the same transcripts and the shares the signing call made -- the same five front passes,
so the difference is what the check pass and the share pass cost against the share verification and the verdicts -- alternating
in one process on one box on identical resident inputs.  One JSON line per shape.
    msig_sign_rate.py [out.jsonl] [rounds]
Shapes: transcripts of 8, 64 and 256 participants at B = 1, 64 and 4 096 transcripts, and one transcript of 1 000 participants.
The material is made on the device: random secrets below 2^251, PK by jjs_public_keys_dev, R and S by jjs_multisig_round1_dev.
Every shape is checked once before it is timed: every sign_status 0 and every share accepted by the combine call.
Per shape: ms per call of each route (median, min, max over the rounds; spread = max - min), shares per second at the median,
and the shader clock read before and after the rounds.  For the transcript of 1 000 participants the kernels of one signing call
are traced (torch.profiler) and `check_pass_share` is the check pass's part of the call's kernel time: its n^2 / 2 compares
beside the (3 + 4 n) / 4 permutations of the binding hash."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

import jubjub_schnorr_amd as jjs  # noqa: E402


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


def material(eng, n, B, seed):
    """B transcripts of n participants, resident: (PK, R, S, m, offsets, sk, r, s)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    N = n * B

    def scalars(rows, top):
        x = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device="cuda", generator=g)
        x[:, 31] &= top
        x[:, 0] |= 1
        return x.contiguous()
    sk, r, s = scalars(N, 0x07), scalars(N, 0x07), scalars(N, 0x07)         # < 2^251 < the group order
    m = scalars(B, 0x3F)                                                    # < 2^254 < q
    PK, bad = eng.public_keys(sk)
    R, S, bad2 = eng.multisig_sign_round1(r, s)
    torch.cuda.synchronize()
    assert not int(bad.max()) and not int(bad2.max())
    return PK, R, S, m, (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32), sk, r, s


def traced_kernels(fn):
    """{kernel name: microseconds} of one call, or None when no trace can be taken."""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower():
                out[ev.name] = out.get(ev.name, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
        return out or None
    except Exception as e:  # noqa: BLE001
        print("no kernel trace:", e, file=sys.stderr)
        return None


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_msig_sign.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    shapes = [(n, B) for n in (8, 64, 256) for B in (1, 64, 4096)] + [(1000, 1)]
    for k, (n, B) in enumerate(shapes):
        PK, R, S, m, offs, sk, r, s = material(eng, n, B, 1400 + k)
        sign = lambda: eng.multisig_sign_round2(PK, R, S, m, offs, sk, r, s)  # noqa: E731
        z, st = sign()
        torch.cuda.synchronize()
        assert not int(st.max()), "the transcripts are valid"
        combine = lambda: eng.multisig_combine(z, PK, R, S, m, offs)  # noqa: E731
        share_st, _, _, _, ts = combine()
        torch.cuda.synchronize()
        assert not int(share_st.max()) and not int(ts.max()), "the combine call accepts every generated share"
        calls = {"sign_ms": sign, "combine_ms": combine}
        t = {name: [] for name in calls}
        clock_before = shader_clock_mhz()
        for rnd in range(rounds + 2):                       # two warm-up rounds: first-use allocations, clocks
            for name, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd >= 2:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        rec = {"participants": n, "transcripts": B, "shares": n * B, "signer_row": None, "rounds": rounds, "device": device,
               "shader_clock_mhz": [clock_before, shader_clock_mhz()]}
        rec.update({name: stats(xs) for name, xs in t.items()})
        for name in calls:
            rec[name.replace("_ms", "_shares_per_s")] = round(n * B / (rec[name]["median"] * 1e-3))
        rec["sign_over_combine"] = round(rec["sign_ms"]["median"] / rec["combine_ms"]["median"], 3)
        if n == 1000:
            kernels = traced_kernels(sign)
            rec["kernel_us"] = {name: round(us, 1) for name, us in sorted(kernels.items())} if kernels else None
            if kernels:
                check = sum(us for name, us in kernels.items() if "msig_sign_check_kernel" in name)
                total = sum(us for name, us in kernels.items() if "kernel" in name.lower())
                rec["check_pass_us"] = round(check, 1)
                rec["check_pass_share"] = round(check / total, 4) if total else None
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")
        f.flush()
        del PK, R, S, m, sk, r, s, z
        eng.trim()
        torch.cuda.empty_cache()
    f.close()


if __name__ == "__main__":
    main()
