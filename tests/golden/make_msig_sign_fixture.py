#!/usr/bin/env python3
"""Writes tests/golden/msig_sign_257.npz: the Python model's shares (tests/msig_sign_cases.py `model`: oracle/jjs_oracle.py's
multisig_transcript, 257 hashes of 516 inputs) of msig_sign_cases.long_case(), the transcript of 257 participants, with a digest
of the inputs they were computed for.  Most of a minute.  Run from the repository root after `make -C oracle`:
    python tests/golden/make_msig_sign_fixture.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")):
    sys.path.insert(0, p)

import msig_sign_cases as sc  # noqa: E402

c = sc.long_case()
z, st = sc.model(c, *c.call())
assert not st.any() and z.shape == (257, 32)
np.savez(sc.FIXTURE_257, digest=np.array(c.digest()), z=z)
print("wrote", sc.FIXTURE_257, os.path.getsize(sc.FIXTURE_257), "bytes")
