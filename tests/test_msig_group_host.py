"""The signer-group passes (csrc/msig_group.h) compiled for the CPU: registration (d_i, the aggregate key, the tags, the window
tables of every key) and the five passes of a call, against jjs_oracle_c.multisig_combine on the tiled inline form
(msig_group_cases.py).  Groups of 1, 2, 8, 256 and 257 participants -- the last row of the generated tag table and the first
computed tag -- with valid transcripts, a corrupted z at the first, a middle and the last slot, two bad shares in one transcript,
z >= r, m >= q and an R / S coordinate >= q; groups that hold the identity, an order-2 and an order-8 key and the same key
twice; the aggregate key; what registration refuses.  Both lane orders of the share pass give the same bytes.

Calls hold 3 to 40 transcripts, with one exception: the call of the 8-participant group that carries a coordinate >= q has 64
(512 shares), because the 7 other shares of that transcript are not compared (multisig_cases.py) and multisig_cases.check caps
the uncompared shares below 2 % of the call."""
import numpy as np
import pytest

import jjs_oracle as o
import msig_group_cases as gcs
import msig_group_hostlib as gl
import multisig_cases as mc


def run_and_check(gc, label, want_uncompared=0):
    e = mc.expected(gc.case)
    outs = []
    for by_participant in (False, True):
        rc, got, agg = gl.combine(gc.PK, *gc.call_args(), by_participant=by_participant)
        assert rc == 0, label
        assert (agg == e.agg[0]).all() and (e.agg == e.agg[:1]).all(), (label, "aggregate key")
        uncompared = mc.check(gc.case, e, gcs.as_inline_outputs(gc, agg, got), label)
        assert uncompared == want_uncompared, (label, uncompared)
        outs.append(got)
    for x, y in zip(*outs):
        assert (x == y).all(), (label, "the lane order of the share pass changed an output")
    return outs[0], e


@pytest.mark.parametrize("n,T", [(1, 12), (2, 40), (8, 40)])
def test_mix_of_transcripts(n, T):
    gc = gcs.group_transcripts(n, T, seed=100 + n)
    coord = {1: [("R", 0, o.Q), ("S", 1, gcs.ALL_ONES)], 2: [("S", 0, o.Q)], 8: []}[n]       # (8: the call below)
    done = gcs.mix(gc, coord)
    (st, su, sr, ts), e = run_and_check(gc, f"n={n}", want_uncompared=(n - 1) * len(coord))
    print(f"group n={n} T={T}: {[w for _, w in done]}; transcript statuses {ts.tolist()}")
    assert ts[0] == 0 and su[0].any() and sr[0].any()
    for t, what in done:
        lo = t * n
        assert ts[t] != 0 and not su[t].any() and not sr[t].any(), (what, t)
        if what.startswith("corrupt"):
            j = mc._pos(n, what.split()[1])
            assert st[lo:lo + n].tolist() == [4 if k == j else 0 for k in range(n)] and ts[t] == 4, what
        elif what == "two bad shares: 4 then 3":
            assert st[lo] == 4 and st[lo + n - 1] == 3 and ts[t] == 4, what
        elif what == "two bad shares: 3 then 4":
            assert st[lo + n - 1] == 4 and ts[t] == 3 and (st[lo:lo + n] == 3).sum() == 1, what
        elif what == "two invalid shares":
            assert st[lo] == 4 and st[lo + n - 1] == 4 and (st[lo:lo + n] != 0).sum() == 2, what
        elif what == "z = r":
            assert st[lo + n // 2] == 3 and ts[t] == 3, what
        elif what == "m = q":
            assert (st[lo:lo + n] == 3).all() and ts[t] == 3, what
        else:
            assert st[lo + n - 1] == 3, what
    assert (ts[len(done) + 1:] == 0).all()


def test_coordinate_out_of_range_among_eight_participants():
    gc = gcs.group_transcripts(8, 64, seed=120)
    gc.case.bad_coord(31, 0, "R", 1, o.Q)              # the transcript's first share: its status is defined (3)
    (st, su, sr, ts), _ = run_and_check(gc, "n=8 coordinate", want_uncompared=7)
    assert st[31 * 8] == 3 and ts[31] == 3 and not su[31].any() and not sr[31].any()
    assert (np.delete(ts, 31) == 0).all()


@pytest.mark.parametrize("n", [mc.TABLE_PARTICIPANTS, mc.TABLE_PARTICIPANTS + 1])
def test_last_table_tag_and_first_computed_tag(n):
    gc = gcs.group_transcripts(n, 3, seed=130 + n)
    gc.case.corrupt(1, n - 1)
    gc.case.bad_z(2, n // 2, o.R_ORDER)
    (st, su, sr, ts), _ = run_and_check(gc, f"n={n}")
    assert ts.tolist() == [0, 4, 3] and su[0].any() and not su[1].any() and not su[2].any()


def test_identity_and_repeated_keys_stay_valid():
    gc = gcs.group_transcripts(5, 6, seed=140, zero_sk=(1,), same_sk=((3, 0),))
    assert (gc.PK[1] == mc.pt_bytes(o.IDENTITY)).all() and (gc.PK[3] == gc.PK[0]).all()
    gc.case.corrupt(4, 3)                               # the second copy of the repeated key
    (st, su, sr, ts), _ = run_and_check(gc, "identity and repeated keys")
    assert ts.tolist() == [0, 0, 0, 0, 4, 0]
    alone = gcs.group_transcripts(1, 3, seed=141, zero_sk=(0,))          # a group of the identity alone: agg_pk is the identity
    rc, got, agg = gl.combine(alone.PK, *alone.call_args())
    assert rc == 0 and (agg == mc.pt_bytes(o.IDENTITY)).all()
    mc.check(alone.case, mc.expected(alone.case), gcs.as_inline_outputs(alone, agg, got), "identity alone")
    assert got[3].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name,point", mc.small_order_points())
def test_small_order_keys_give_the_inline_bytes(name, point):
    base = gcs.group_transcripts(4, 5, seed=150)
    base.case.corrupt(2, 1)
    for j in (0, 3):
        gc = gcs.with_point(base, j, point)
        (st, su, sr, ts), e = run_and_check(gc, f"{name} at {j}")
        print(f"{name} as key {j}: oracle statuses {e.st.tolist()}")


def test_registration_refuses_no_key_and_a_coordinate_out_of_range():
    gc = gcs.group_transcripts(3, 3, seed=160)
    assert gl.check_keys(gc.PK) == 0
    assert gl.check_keys(np.zeros((0, 64), np.uint8)) == -1
    for j, half, value in ((0, 0, o.Q), (2, 1, o.Q), (1, 0, gcs.ALL_ONES)):
        PK = gc.PK.copy()
        PK[j, 32 * half:32 * half + 32] = mc._fe([value])[0]
        assert gl.check_keys(PK) == -1, (j, half)
        assert gl.combine(PK, *gc.call_args())[0] == -1
    PK = gc.PK.copy()
    PK[1, :32] = mc._fe([o.Q - 1])[0]                   # canonical (whatever point it is): registered
    assert gl.check_keys(PK) == 0


def test_key_with_a_small_order_part_and_shares_the_reference_accepts():
    """PK_0 = sk_0 G + T8: the reference multiplies it by c d_0 REDUCED mod r, and the shares built for that are valid (the
    oracle says 0, the builder planned 0).  Tables of d_0 PK_0 walked with c would compute another small-order part."""
    gc = gcs.torsion_key_case()
    (st, su, sr, ts), e = run_and_check(gc, "torsion key")
    assert e.ts.tolist() == [0] * gc.T and ts.tolist() == [0] * gc.T and su.any(1).all()
