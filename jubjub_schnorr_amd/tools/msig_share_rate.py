#!/usr/bin/env python3
"""verify_share on its own (include/jjs_gpu.h jjs_multisig_verify_share_dev, jjs_msig_group_verify_share_dev,
jjs_multisig_verify_share_keyset_dev) with ONE query per transcript, beside the only earlier route to the same answer on the same
transcripts: the combine call of the route (jjs_multisig_combine_dev, jjs_msig_group_combine_dev,
jjs_multisig_combine_keyset_dev) with the query's z at its row and zero filler in the other rows, one byte of whose share_status
is the answer.  The two alternate in one process on one box on identical resident inputs.  One JSON line per shape and route.
    msig_share_rate.py [out.jsonl] [rounds]
Shapes: transcripts of 8, 64 and 256 participants at B = 1, 64 and 4 096 transcripts, and one transcript of 1 000 participants.
Every transcript of a shape has the same n signers (a signer group takes nothing else), so one material serves the three routes:
the inline call gets the keys tiled, the group is registered from them, the key set holds them and key_idx names them in order.
The material is made on the device: random secrets below 2^251, PK by jjs_public_keys_dev, R and S by jjs_multisig_round1_dev,
the shares by jjs_multisig_sign_dev.  Every shape is checked once before it is timed: every query's status 0 on both sides, and
sig_R of the new call equal to the combine call's on the whole valid transcripts.
Per line: ms per call of each side (median, min, max over the rounds; spread = max - min), their ratio at the medians, and the
shader clock read before and after the rounds."""
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
    """B transcripts of the same n signers, resident: (keys (n, 64), PK (N, 64) tiled, R, S, m, offsets, z the signers' shares)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    N = n * B

    def scalars(rows, top):
        x = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device="cuda", generator=g)
        x[:, 31] &= top
        x[:, 0] |= 1
        return x.contiguous()
    sk_n, r, s = scalars(n, 0x07), scalars(N, 0x07), scalars(N, 0x07)       # < 2^251 < the group order
    m = scalars(B, 0x3F)                                                    # < 2^254 < q
    keys, bad = eng.public_keys(sk_n)
    R, S, bad2 = eng.multisig_sign_round1(r, s)
    torch.cuda.synchronize()
    assert not int(bad.max()) and not int(bad2.max())
    PK, sk = keys.repeat(B, 1).contiguous(), sk_n.repeat(B, 1).contiguous()
    offs = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
    z, st = eng.multisig_sign_round2(PK, R, S, m, offs, sk, r, s)
    torch.cuda.synchronize()
    assert not int(st.max()), "the transcripts are valid"
    return keys, PK, R, S, m, offs, z


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_msig_share.jsonl")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = jjs.engine()
    device = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    f = open(out, "w")
    shapes = [(n, B) for n in (8, 64, 256) for B in (1, 64, 4096)] + [(1000, 1)]
    for k, (n, B) in enumerate(shapes):
        keys, PK, R, S, m, offs, z = material(eng, n, B, 2100 + k)
        # one query per transcript: slot t mod n of transcript t, its signer's share
        qt = torch.arange(B, dtype=torch.int32, device="cuda")
        qs = (qt % n).to(torch.int32).contiguous()
        rows = (qt.long() * n + qs.long())
        qz = z[rows].contiguous()
        filler = torch.zeros_like(z)
        filler[rows] = qz
        idx = torch.arange(n, dtype=torch.int32, device="cuda").repeat(B).contiguous()
        group, ks = eng.multisig_group(keys.cpu().numpy()), eng.keyset("single", keys.cpu().numpy())
        routes = {
            "inline": (lambda: eng.multisig_verify_share(PK, R, S, m, offs, qt, qs, qz, want_R=True),
                       lambda: eng.multisig_combine(filler, PK, R, S, m, offs),
                       lambda: eng.multisig_combine(z, PK, R, S, m, offs)[3]),
            "group": (lambda: group.verify_share(R, S, m, qt, qs, qz, want_R=True),
                      lambda: group.combine(filler, R, S, m),
                      lambda: group.combine(z, R, S, m)[2]),
            "keyset": (lambda: ks.multisig_verify_share(idx, R, S, m, offs, qt, qs, qz, want_R=True),
                       lambda: ks.multisig_combine(idx, filler, R, S, m, offs),
                       lambda: ks.multisig_combine(idx, z, R, S, m, offs)[3]),
        }
        for route, (share, combine, whole) in routes.items():
            st, sr = share()
            old = combine()[0]
            want_R = whole()
            torch.cuda.synchronize()
            assert not int(st.max()) and not int(old[rows].max()), "both sides accept the queried shares"
            assert bool((sr == want_R).all()), "sig_R is what combine returns for the valid transcript"
            calls = {"verify_share_ms": share, "combine_ms": combine}
            t = {name: [] for name in calls}
            clock_before = shader_clock_mhz()
            for rnd in range(rounds + 2):                   # two warm-up rounds: first-use allocations, clocks
                for name, fn in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rnd >= 2:
                        t[name].append((time.perf_counter() - t0) * 1e3)
            rec = {"route": route, "participants": n, "transcripts": B, "queries": B, "rounds": rounds, "device": device,
                   "shader_clock_mhz": [clock_before, shader_clock_mhz()]}
            rec.update({name: stats(xs) for name, xs in t.items()})
            rec["verify_share_over_combine"] = round(rec["verify_share_ms"]["median"] / rec["combine_ms"]["median"], 3)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            f.flush()
        group.close(); ks.close()
        del keys, PK, R, S, m, z, filler, qz
        eng.trim()
        torch.cuda.empty_cache()
    f.close()


if __name__ == "__main__":
    main()
