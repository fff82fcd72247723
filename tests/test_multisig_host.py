"""The multisignature passes (csrc/multisig_core.h) compiled for the CPU, on the cases of multisig_cases.py: the range tests of
msig_share_item, the first-failure rule of msig_verdict_item, identity and small-order points, the last row of the tag table beside
the first computed tag, and empty transcripts between full ones.  test_multisig_gpu.py runs the same cases as HIP kernels, in
every lane mode; the CPU build has no lane modes, so the 8192 boundaries are not repeated here."""
import numpy as np

import hostlib as hl
import jjs_oracle_c as oc
import multisig_cases as mc


def test_c_oracle_agrees_with_python_oracle_on_small_order_points():
    """Identity, order-2 and order-8 points as PK, R and S are new inputs for jjo_multisig_combine as well: before it serves as the
    expected value for them, it is held against the Python oracle on every transcript of small_order_case."""
    case, valid_from = mc.small_order_case()
    assert not case.marks
    e = mc.expected(case)
    for t in range(case.T):
        st, first, agg, su, sr = mc.python_oracle_outputs(case, t)
        lo, hi = int(case.offsets[t]), int(case.offsets[t + 1])
        assert e.st[lo:hi].tolist() == st and e.ts[t] == first, t
        assert e.agg[t].tobytes() == agg and e.su[t].tobytes() == su and e.sr[t].tobytes() == sr, t
    # the transcripts built with a zero secret scalar hold identity points and stay valid; the last but one is identities only
    assert e.ts[valid_from:].tolist() == [0] * (case.T - valid_from)
    ident = mc.pt_bytes(mc.o.IDENTITY).tobytes()
    assert e.agg[valid_from + 3].tobytes() == ident and e.sr[valid_from + 3].tobytes() == ident and not e.su[valid_from + 3].any()


def test_c_oracle_marks_the_out_of_range_encodings():
    """The builder's marks against the oracle's own range tests on the `dirty` arrays: every marked share is 3 there, every
    marked transcript gets no signature, and transcripts without a mark are untouched by the marks of others."""
    case, _ = mc.mixed_call(400, seed=2)
    e = mc.expected(case)
    d = case.dirty
    st, ts, agg, su, sr = oc.multisig_combine(d["z"], d["PK"], d["R"], d["S"], d["m"], case.offsets.astype(np.uint32))
    marked = set()
    for t, kind, j, _ in case.marks:
        marked.add(t)
        lo, hi = int(case.offsets[t]), int(case.offsets[t + 1])
        assert (st[lo:hi] == 3).all() if kind == "m" else st[lo + j] == 3, (t, kind, j)
        assert ts[t] != 0 and not su[t].any() and not sr[t].any(), (t, kind)
    for t in set(range(case.T)) - marked:
        lo, hi = int(case.offsets[t]), int(case.offsets[t + 1])
        assert (st[lo:hi] == e.st[lo:hi]).all() and ts[t] == e.ts[t] and (agg[t] == e.agg[t]).all() and (su[t] == e.su[t]).all()


def test_malformed_first_failure_small_order_and_empty_transcripts():
    """One call: every special transcript in the middle of a reduced form of the device test's call D (empty transcripts at
    the first two and last two indices and in runs between full ones).  2201 shares: the 42 shares beside a coordinate >= q that
    are not compared stay under 2 % of the call (mc.check asserts it)."""
    case, sections = mc.mixed_call(2201, seed=3, T=900, top=6)
    empty = case.sizes() == 0
    assert empty[[0, 1, -2, -1]].all() and empty.sum() > 100 and (empty[2:-3] & empty[3:-2]).any() and (empty[1:-1] & ~empty[:-2] & ~empty[2:]).any()
    got = hl.multisig(*case.args())
    uncompared = mc.check(case, mc.expected(case), got, "host")
    mc.check_sections(case, sections, got, "host")
    assert uncompared == 42


def test_table_last_row_beside_first_computed_tag():
    """256 participants (the last row of the generated tag table) and 257 (the first tag computed at call time) side by side,
    the second with an invalid last share."""
    case = mc.valid_transcripts([mc.TABLE_PARTICIPANTS, mc.TABLE_PARTICIPANTS + 1], seed=5)
    case.corrupt(1, mc.TABLE_PARTICIPANTS)
    got = hl.multisig(*case.args())
    mc.check(case, mc.expected(case), got, "host")
    assert got[4].tolist() == [0, 4] and got[2][0].any() and not got[2][1].any()
