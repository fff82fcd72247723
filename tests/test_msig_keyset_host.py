"""The multisignature passes over a registered key set (csrc/msig_keyset.h) compiled for the CPU: registration by the kt_*
builders (flags, chains, the window tables of the valid keys), the gather, the two table passes and the refusals, against the CPU
build of the inline passes (hostlib.multisig, byte for byte on the gathered column) and against jjs_oracle_c.multisig_combine
(msig_keyset_cases.expected).  Transcripts of 1, 2, 3 and 8 participants, one key twice in a transcript, a spoilt share in front
of a malformed one, z >= r, an empty transcript, and a refused transcript by each cause between two good ones.  The oracle
comparison leaves no share uncompared; the call with an R coordinate >= q is compared with the inline passes in full."""
import numpy as np
import pytest

import hostlib
import msig_keyset_cases as kcs
import msig_keyset_hostlib as kl
import multisig_cases as mc


@pytest.fixture(scope="module")
def keyset():
    return kcs.key_set()


def run(keys, kc):
    rc, status, got = kl.combine(keys, *kc.args())
    assert rc == 0
    assert status.tolist() == kcs.KEY_STATUS
    for x in got:
        assert x.size == 0 or not (x.reshape(len(x), -1) == 0xA5).all(1).any(), "an output row was not written"
    return got


def test_mix_against_inline_passes_and_oracle(keyset):
    keys, sk = keyset
    kc, where = kcs.host_mix(keys, sk)
    got = run(keys, kc)
    kcs.check_against_inline(kc, got, hostlib.multisig(*kc.inline_args()), "host mix")
    assert mc.check(kc.case, kcs.expected(kc), got, "host mix") == 0
    st, agg, su, sr, ts = got
    off = kc.case.offsets
    for what in ("good 1", "good 2", "good 3", "good 8", "same key twice"):
        t = where[what]
        assert ts[t] == 0 and su[t].any() and sr[t].any() and agg[t].any(), what
    t = where["spoilt then z >= r"]
    assert st[off[t]:off[t + 1]].tolist() == [0, 4, 0, 3] and ts[t] == 4 and agg[t].any() and not su[t].any()
    t = where["z >= r"]
    assert st[off[t]:off[t + 1]].tolist() == [0, 3, 0] and ts[t] == 3
    t = where["empty"]
    assert ts[t] == 5 and not agg[t].any() and not su[t].any() and not sr[t].any()
    for what, _ in kcs.REFUSALS:
        t = where[what]
        assert (st[off[t]:off[t + 1]] == 3).all() and ts[t] == 3, what
        assert not agg[t].any() and not su[t].any() and not sr[t].any(), what
        assert ts[t - 1] == 0 and ts[t + 1] == 0 and su[t - 1].any() and su[t + 1].any(), (what, "the neighbours")
    print("transcript statuses", ts.tolist())


def test_non_canonical_key_refuses_its_transcript(keyset):
    keys, sk = keyset
    kc = kcs.pool_transcripts([2, 3, 1], 920, keys, sk)
    kc.refuse(1, 2, kcs.NONCANONICAL_KEY, "non-canonical")
    got = run(keys, kc)
    kcs.check_against_inline(kc, got, hostlib.multisig(*kc.inline_args()), "non-canonical key")
    assert mc.check(kc.case, kcs.expected(kc), got, "non-canonical key") == 0
    assert got[4].tolist() == [0, 3, 0]


def test_coordinate_out_of_range_against_the_inline_passes_in_full(keyset):
    keys, sk = keyset
    kc, where = kcs.host_mix(keys, sk, seed=930, coord=True)
    got = run(keys, kc)
    kcs.check_against_inline(kc, got, hostlib.multisig(*kc.inline_args()), "R.v >= q")
    t = where["R.v >= q"]
    assert got[0][kc.case.offsets[t]] == 3 and got[4][t] == 3 and not got[2][t].any()


def test_every_row_unusable_and_all_transcripts_empty(keyset):
    keys, sk = keyset
    kc = kcs.pool_transcripts([2, 1], 940, keys, sk)
    kc.refuse(0, 0, 0xFFFFFFFF); kc.refuse(0, 1, kcs.ORDER2_KEY); kc.refuse(1, 0, 16)
    got = run(keys, kc)
    assert (got[0] == 3).all() and (got[4] == 3).all() and not got[1].any() and not got[2].any() and not got[3].any()
    kc = kcs.pool_transcripts([0, 0], 941, keys, sk)
    got = run(keys, kc)
    assert got[4].tolist() == [5, 5] and not got[1].any()
