"""Child process of tests/test_msig_scratch_gpu.py: in one fresh engine, the six multisignature forms of staged_host_calls_child
(their _dev forms, at its tiny ragged shape) before and after the calls that make regions of the multisignature scratch
(csrc/msig_scratch.h) grow, appear in the middle and move: an affine combine beyond the first allocation in rows and transcripts,
a tiny extended combine, and the large combine in extended format.  Every repeat must equal the first run byte for byte (the
first runs are pinned to the oracles by the forms' own tests); the large calls must give one transcript's outputs, tiled.
One JSON line; stops at the first failure."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]

import multisig_cases as mc  # noqa: E402
from helpers import to_extended  # noqa: E402
from staged_host_calls_child import build_forms  # noqa: E402

SIX = ("combine", "group_combine", "keyset_combine", "verify", "verify_share", "multisig_sign")
REPS = 1025                      # four signers each: 4100 rows and 1025 transcripts, above the floors of 4096 and 1024


def main() -> None:
    import torch
    torch.cuda.init()
    import jubjub_schnorr_amd as jjs
    eng = jjs.engine()
    forms = [f for f in build_forms(eng) if f.name in SIX]
    assert [f.name for f in forms] == list(SIX)

    def combine(case, ext):
        cols = [case.dirty[k] for k in mc.COLS]
        if ext:
            rng = np.random.default_rng(77)
            cols = [to_extended(c, rng) if c.shape[1] == 64 else c for c in cols]
        got = eng.multisig_combine(*[torch.from_numpy(c).cuda() for c in cols], case.offsets.astype(np.uint32), fmt="ext" if ext else "affine")
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in got]

    first = {f.name: f.run(True) for f in forms}
    runs = 1

    def again(label):
        nonlocal runs
        for f in forms:
            assert f.run(True) == first[f.name], f"{f.name}, {label}: differs from its first run"
        runs += 1

    one = mc.valid_transcripts([4], 5200)
    want = combine(one, False)
    mc.check(one, mc.expected(one), want, "one transcript")
    assert not want[0].any() and not want[4].any(), "the transcript is valid"
    big = mc.tile(one, REPS)
    assert big.n == 4100 and big.T == 1025

    def tiled(got, label):
        for name, g, w in zip(("share_status", "agg_pk", "sig_u", "sig_R", "transcript_status"), got, want):
            assert (g == np.tile(w, (REPS, 1) if w.ndim == 2 else REPS)).all(), f"{label}: {name} is not the single transcript's, tiled"

    tiled(combine(big, False), "the affine call beyond the first allocation")
    again("behind the scratch's growth in rows and transcripts")
    for g, w in zip(combine(one, True), want):
        assert (g == w).all(), "the tiny extended call"
    again("behind the ext region's appearance")
    tiled(combine(big, True), "the extended call beyond the ext region")
    again("behind the ext region's growth")
    print(json.dumps({"forms": [f.name for f in forms], "runs": runs, "rows": big.n, "transcripts": big.T}), flush=True)


if __name__ == "__main__":
    main()
