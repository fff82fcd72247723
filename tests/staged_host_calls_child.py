"""Child process of tests/test_staged_host_calls_gpu.py: the eight blocking host-buffer forms that share one staging area and one
frame (csrc/staged_host_call.h) -- the inline, signer-group and key-set combine, verify, verify_share, multisig sign, SecretKey
signing and var-generator signing -- in one fresh engine.  Every host form's outputs are compared byte for byte with its own
_dev form on the same inputs (the _dev forms are pinned to the oracles by their own tests).
`sequence`: all eight back to back at a tiny ragged shape, a call that makes the area grow, all eight again, jjs_trim, all eight
again, a refused call of every form with a valid call of another form behind it, jjs_shutdown, jjs_init and one more call.
`threads`: two host threads, 50 calls each, one signing and one checking shares.  One JSON line."""
import ctypes
import json
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import msig_group_cases as gcs  # noqa: E402
import msig_keyset_cases as kcs  # noqa: E402
import msig_share_cases as shc  # noqa: E402
import msig_sign_cases as scs  # noqa: E402
import msig_verify_cases as vcs  # noqa: E402
import multisig_cases as mc  # noqa: E402
import sign_fixed_cases as sfc  # noqa: E402
import sign_vargen_pt_cases as svc  # noqa: E402

SIZES = [0, 1, 3]                 # the tiny ragged shape: an empty transcript, one signer, three; four rows in all
FILL = 0xA5
ERR_ARG = -1                      # include/jjs_gpu.h JJS_ERR_ARG


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def filled(*shape):
    return np.full(shape, FILL, np.uint8)


class Form:
    """One entry point through its Python mirror (numpy arrays: the blocking host form; CUDA tensors: the _dev form), and the same
    host call through the C ABI with prefilled outputs: raw() -> (name, args, outputs)."""

    def __init__(self, name, fn, args, kwargs=None, raw=None, refusals=()):
        self.name, self.fn, self.args, self.kwargs, self.raw, self.refusals = name, fn, args, kwargs or {}, raw, refusals

    def run(self, on_device):
        import torch
        args = self.args
        if on_device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()  # noqa: E731
            args = [up(a) if isinstance(a, np.ndarray) else a for a in args]
        out = self.fn(*args, **self.kwargs)
        out = out if isinstance(out, tuple) else (out,)
        if on_device:
            torch.cuda.synchronize()
        return [(x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)).tobytes() for x in out if x is not None]


def build_forms(eng):
    """The eight forms at the tiny shape.  A refusal is (what, position of the argument, its value, a piece of the message)."""
    B, offs = len(SIZES), np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    n, ol = int(offs[-1]), [int(x) for x in offs]         # ol: the offsets for a mirror, host memory in both forms
    keys, sk_pool = kcs.key_set()
    ks = eng.keyset("single", keys)
    forms = []

    case = mc.valid_transcripts(SIZES, 5100)
    case.corrupt(2, 1)
    z, PK, R, S, m = (case.dirty[k] for k in mc.COLS)
    forms.append(Form("combine", eng.multisig_combine, [z, PK, R, S, m, ol],
                      raw=lambda: ("jjs_multisig_combine", [0, P(z), P(PK), P(R), P(S), P(m), P(offs), B],
                                   [filled(n), filled(B), filled(B, 64), filled(B, 32), filled(B, 64)]),
                      refusals=[("m is null", 5, None, b"null pointer"), ("format 7", 0, 7, b"affine or extended points (format 7)")]))

    gc = gcs.group_transcripts(3, B, 5101)
    gc.case.corrupt(1, 2)
    grp = eng.multisig_group(gc.PK)
    gone = eng.multisig_group(gc.PK)
    stale = gone.handle
    gone.close()
    gz, gR, gS, gm = gc.call_args()
    forms.append(Form("group_combine", grp.combine, [gz, gR, gS, gm],
                      raw=lambda: ("jjs_msig_group_combine", [grp.handle, 0, P(gz), P(gR), P(gS), P(gm), B],
                                   [filled(3 * B), filled(B), filled(B, 32), filled(B, 64)]),
                      refusals=[("a stale group handle", 0, stale, b"unknown or destroyed signer group"),
                                ("format 7", 1, 7, b"affine or extended points (format 7)")]))

    kc = kcs.pool_transcripts(SIZES, 5102, keys, sk_pool)
    kc.case.corrupt(2, 0)
    kidx, kz, kR, kS, km, _ = kc.args()
    forms.append(Form("keyset_combine", ks.multisig_combine, [kidx, kz, kR, kS, km, ol],
                      raw=lambda: ("jjs_multisig_combine_keyset", [ks.handle, 0, P(kidx), P(kz), P(kR), P(kS), P(km), P(offs), B],
                                   [filled(n), filled(B), filled(B, 64), filled(B, 32), filled(B, 64)]),
                      refusals=[("format 7", 1, 7, b"affine or extended points (format 7)"), ("m is null", 6, None, b"null pointer")]))

    vc = vcs.build([[], [2], [0, 1, 3]], 5103, keys, sk_pool)
    vc.spoil_u(1)
    forms.append(Form("verify", eng.multisig_verify, [vc.PK, ol, vc.u, vc.R, vc.m],
                      raw=lambda: ("jjs_multisig_verify", [0, P(vc.PK), P(offs), P(vc.u), P(vc.R), P(vc.m), B], [filled(B, 64), filled(B), filled(32).view(np.uint64)]),
                      refusals=[("agg_pk is null", 7, None, b"null pointer"), ("format 7", 0, 7, b"affine or extended points (format 7)")]))

    sc = shc.ShareCase("inline", mc.valid_transcripts(SIZES, 5104))
    sc.ask(2, 1)
    sc.ask(1, 0, 5, "not the signer's share")
    qt, qs, qz = sc.queries()
    _, sPK, sR, sS, sm = (sc.case.dirty[k] for k in mc.COLS)
    forms.append(Form("verify_share", eng.multisig_verify_share, [sPK, sR, sS, sm, ol, qt, qs, qz], {"want_R": True},
                      raw=lambda: ("jjs_multisig_verify_share", [0, P(sPK), P(sR), P(sS), P(sm), P(offs), B, P(qt), P(qs), P(qz), 2], [filled(2), filled(B, 64)]),
                      refusals=[("format 3", 0, 3, b"verify_share takes affine, extended or wire points (format 3)"),
                                ("m is null", 4, None, b"null pointer")]))

    sg = scs.build(SIZES, 5105)
    _, ssk, sr_, ss_ = sg.call()
    forms.append(Form("multisig_sign", eng.multisig_sign_round2, [sg.PK, sg.R, sg.S, sg.m, ol, ssk, sr_, ss_],
                      raw=lambda: ("jjs_multisig_sign", [0, P(sg.PK), P(sg.R), P(sg.S), P(sg.m), P(offs), B, None, P(ssk), P(sr_), P(ss_), n], [filled(n, 32), filled(n)]),
                      refusals=[("sk is null", 8, None, b"null pointer"), ("the wire format", 0, 2, b"affine or extended points (format 2)")]))

    fsk, frnd, fm = sfc.keyed_call(False, "random", 4)
    forms.append(Form("sign_fixed", eng.sign_fixed, ["single", fsk, frnd, fm], {"wire": True},
                      raw=lambda: ("jjs_sign_fixed", [0, P(fsk), 1, P(frnd), P(fm), 4],
                                   [filled(4, 32), filled(4, 64), None, filled(1, 64), None, filled(4, 64), filled(1, 32), filled(4)]),
                      refusals=[("status is null", 13, None, b"null pointer"), ("scheme 9", 0, 9, b"scheme must be")]))

    vsk, vgen, vrnd, vm, _ = svc.shared_call("5*G", 4)
    forms.append(Form("sign_vargen_pt", eng.sign_vargen_pt, [vsk, vgen, vrnd, vm],
                      raw=lambda: ("jjs_sign_vargen_pt", [0, P(vsk), P(vgen), 1, P(vrnd), P(vm), 4],
                                   [filled(4, 32), filled(4, 64), filled(4, 64), filled(1, 64), filled(4)]),
                      refusals=[("sk is null", 1, None, b"null pointer"), ("format 5", 0, 5, b"format out of range")]))
    assert len(forms) == 8
    return forms


def sequence(eng, lib):
    forms = build_forms(eng)
    staging = lambda: eng.memory_stats()["host_staging"]  # noqa: E731
    want = {f.name: f.run(True) for f in forms}

    def all_host(label):
        for f in forms:
            assert f.run(False) == want[f.name], f"{f.name}, {label}: the host form differs from the _dev form"

    all_host("the first calls")
    seen = staging()
    # the smallest power of two of rows at which a call no longer fits the area
    rows, grew = 4, None
    while grew is None and rows < 1 << 14:
        rows *= 2
        sk, gen, rnd, m, _ = svc.shared_call("5*G", rows)
        big = Form("sign_vargen_pt", eng.sign_vargen_pt, [sk, gen, rnd, m])
        before = staging()
        got = big.run(False)
        after = staging()
        assert got == big.run(True), f"sign_vargen_pt at {rows} rows: the host form differs from the _dev form"
        assert after >= before
        if after > before:
            grew = (rows, before, after)
    assert grew is not None, "no call made the staging area grow"
    all_host("after the area has grown")
    assert staging() == grew[2], "a call at a shape the engine has seen allocated"
    eng.trim()
    trimmed = staging()
    assert trimmed < grew[2], "jjs_trim frees the area"
    all_host("after jjs_trim")
    assert staging() == seen, "the area comes back at the size the tiny calls gave it"

    refused = 0
    for i, f in enumerate(forms):
        nxt = forms[(i + 1) % len(forms)]
        for what, at, value, text in f.refusals:
            name, args, outs = f.raw()
            full = args + [P(o) for o in outs]
            full[at] = value
            rc = getattr(lib, name)(*full)
            assert rc == ERR_ARG and text in lib.jjs_last_error(), (f.name, what, rc, lib.jjs_last_error())
            assert all(o is None or (o.view(np.uint8) == FILL).all() for o in outs), f"{f.name}, {what}: a refused call wrote an output"
            assert nxt.run(False) == want[nxt.name], f"{nxt.name} behind {f.name} refused for {what}"
            refused += 1
        name, args, outs = f.raw()                                   # the same call, nothing spoilt: it is the arguments that were refused
        assert getattr(lib, name)(*args, *[P(o) for o in outs]) == 0, (f.name, lib.jjs_last_error())
        assert not any(o is not None and (o.view(np.uint8) == FILL).all() for o in outs), f"{f.name}: an output was not written"

    lib.jjs_shutdown()                                               # returns: every call above has counted itself out again
    assert lib.jjs_init(1) == 0
    combine = forms[0]
    assert combine.run(False) == want["combine"], "combine in the second engine of the process"
    return {"grew_at_rows": grew[0], "staging_before": grew[1], "staging_after": grew[2], "staging_tiny": seen, "staging_trimmed": trimmed,
            "refused_calls": refused}


def threads(eng, lib, calls=50):
    forms = {f.name: f for f in build_forms(eng)}
    pair = [forms["sign_fixed"], forms["verify_share"]]
    want = [f.run(True) for f in pair]
    for f, w in zip(pair, want):
        assert f.run(False) == w, f"{f.name}: the host form differs from the _dev form"
    bad, start = [], threading.Barrier(2)

    def loop(k):
        start.wait()
        for c in range(calls):
            if pair[k].run(False) != want[k]:
                bad.append((pair[k].name, c))
    ts = [threading.Thread(target=loop, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad, bad[:5]
    return {"calls_per_thread": calls, "forms": [f.name for f in pair]}


def main() -> None:
    import torch
    torch.cuda.init()
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    out = {"sequence": sequence, "threads": threads}[sys.argv[1]](eng, eng._lib)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
