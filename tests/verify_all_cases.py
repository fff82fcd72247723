"""Batches for the tests of jjs_verify_all_* (test_verify_all_gpu.py, verify_all_child.py): valid batches signed on the
device, one spoilt item per failure class, and the constructions that defeat weaker batch checks."""
import numpy as np

import jjs_oracle as o
from helpers import ARG_ORDER, IDENT, fe_bytes, make_batch, pt_bytes, to_int, to_pt, torsion_generator


def device_batch(eng, scheme, n, n_keys, seed=5):
    """n valid signatures over n_keys key pairs, signed on the device: CUDA uint8 columns in ARG_ORDER[scheme]."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed + n)
    n_keys = max(1, min(n_keys, n))

    def rand(rows, top_mask):
        t = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, generator=gen)
        t[:, 31] &= top_mask
        return t

    key_sk = rand(n_keys, 0x07); key_sk[:, 0] |= 1
    key_g = rand(n_keys, 0x07); key_g[:, 0] |= 1
    kidx = torch.arange(n) % n_keys
    sk, g = key_sk[kidx].cuda(), key_g[kidx].cuda()
    rnd, m = rand(n, 0x07).cuda(), rand(n, 0x3F).cuda()
    if scheme == "single":
        u, R, PK = eng.sign(scheme, sk, rnd, m)
        cols = [u, R, PK, m]
    elif scheme == "double":
        u, R, Rp, PK, PKp = eng.sign(scheme, sk, rnd, m)
        cols = [u, R, Rp, PK, PKp, m]
    else:
        u, R, PK, Gen = eng.sign(scheme, sk, rnd, m, gen_scalar=g)
        cols = [u, R, PK, Gen, m]
    torch.cuda.synchronize()
    return [c.contiguous() for c in cols]


def _torsion(k):
    return o.mul(torsion_generator(), k)


def spoil_cases(scheme, base):
    """(name, batch) pairs: base (all valid) with one item spoilt, per failure class, at the first, middle and last item."""
    n = len(base["u"])
    out = []
    for pos in (0, n // 2, n - 1):
        def variant(name, **cols):
            b = {k: v.copy() for k, v in base.items()}
            for k, v in cols.items():
                b[k][pos] = v
            out.append((f"{name}@{pos}", b))
        u = to_int(base["u"][pos])
        variant("bad_u", u=fe_bytes((u + 1) % o.R_ORDER))
        m = base["m"][pos].copy(); m[0] ^= 1
        variant("flipped_m", m=m)
        R = to_pt(base["R"][pos])
        for k in range(1, 8):
            variant(f"R_plus_T{k}", R=pt_bytes(o.add(R, _torsion(k))))
        variant("PK_torsion", PK=pt_bytes(o.add(to_pt(base["PK"][pos]), _torsion(1))))
        variant("identity_R", R=IDENT)
        nc = base["R"][pos].copy(); nc[:32] = fe_bytes(o.Q)
        variant("noncanonical_R", R=nc)
        variant("u_ge_r", u=fe_bytes(o.R_ORDER))
    return out


def _resign_vargen(b, i, gen):
    rng = np.random.default_rng(99)
    sk = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
    k = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
    m = to_int(b["m"][i])
    PK, R = o.mul(gen, sk), o.mul(gen, k)
    c = o.challenge_vargen(R, PK, gen, m)
    b["Gen"][i], b["PK"][i], b["R"][i], b["u"][i] = pt_bytes(gen), pt_bytes(PK), pt_bytes(R), fe_bytes((k - c * sk) % o.R_ORDER)


def cancelling_equations():
    """(scheme, batch): items 0 and 1 carry u_0 + d and u_1 - d, so that their D's sum to O (for the per-item generator
    both items share one generator)."""
    out = []
    for scheme in ("single", "double", "vargen"):
        b = make_batch(scheme, 6, seed=34, n_keys=6, mix=False)
        if scheme == "vargen":
            _resign_vargen(b, 1, to_pt(b["Gen"][0]))
        d = 12345
        b["u"][0] = fe_bytes((to_int(b["u"][0]) + d) % o.R_ORDER)
        b["u"][1] = fe_bytes((to_int(b["u"][1]) - d) % o.R_ORDER)
        out.append((scheme, b))
    return out


def _single_rows(rows):
    return {key: np.stack([r[key] for r in rows]) for key in ARG_ORDER["single"]}


def cancelling_torsion():
    """Two single signatures with R_1 + T and R_2 - T, both prime-order equations holding: R_1 + R_2 is torsion-free."""
    t = torsion_generator()
    rng = np.random.default_rng(35)
    rows = []
    for sgn in (1, -1):
        sk = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
        k = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
        m = int.from_bytes(rng.bytes(40), "little") % o.Q
        PK = o.mul(o.G, sk)
        R = o.add(o.mul(o.G, k), t if sgn > 0 else o.neg(t))
        c = o.challenge_single(R, PK, m)
        rows.append({"u": fe_bytes((k - c * sk) % o.R_ORDER), "R": pt_bytes(R), "PK": pt_bytes(PK), "m": fe_bytes(m)})
    return _single_rows(rows)


def cofactorless_torsion():
    """One single signature with PK + T and R + c T: u G + c PK == R holds exactly, yet both points carry torsion."""
    t = torsion_generator()
    rng = np.random.default_rng(36)
    sk = int.from_bytes(rng.bytes(40), "little") % (o.R_ORDER - 1) + 1
    m = int.from_bytes(rng.bytes(40), "little") % o.Q
    PK = o.add(o.mul(o.G, sk), t)
    for k in range(1, 200):
        for ct in range(8):
            R = o.add(o.mul(o.G, k), o.mul(t, ct))
            c = o.challenge_single(R, PK, m)
            if c % 8 == ct:
                u = (k - c * sk) % o.R_ORDER
                assert o.add(o.mul(o.G, u), o.mul(PK, c)) == R
                return _single_rows([{"u": fe_bytes(u), "R": pt_bytes(R), "PK": pt_bytes(PK), "m": fe_bytes(m)}])
    raise AssertionError("no consistent nonce found")
