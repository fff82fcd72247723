"""The extended-coordinate multisignature calls on the CPU: normalize_lane in poison mode (csrc/normalize.h) against derived
columns computed in Python integers (msig_ext_cases.py), with launch shapes in which one lane owns several rows; the mode
switched off against what the verify paths are promised; then whole calls -- normalisation in front of the CPU build of the
passes -- against jjs_oracle_c.multisig_combine on the derived columns through multisig_cases.check, inline and by group."""
import numpy as np
import pytest

import hostlib as hl
import jjs_oracle as o
import msig_ext_cases as xc
import msig_ext_hostlib as xh
import msig_group_cases as gcs
import msig_group_hostlib as gh
import multisig_cases as mc


def planted_call():
    """210 shares in ragged transcripts, every kind of unusable point in every column at the four places."""
    x = xc.ExtCase(mc.filler(210, seed=31, top=5), seed=32)
    xc.plant_everywhere(x, boundary=x.T // 2)
    return x


def test_the_case_builder_derives_its_columns_from_integers():
    x = planted_call()
    x.check_derived()
    assert {kind for _, _, _, kind in x.plants} == set(xc.KINDS) and {col for _, _, col, _ in x.plants} == set(xc.POINT_COLS)
    z = [int.from_bytes(x.ext["R"][i, 64:].tobytes(), "little") for i in range(1, 3)]
    assert z == [o.Q - 1, 2], "the chosen Z values sit where no plant overwrites them"
    # a good point sits in the same row as an unusable one
    rows = {x.derived.row(t, j) for t, j, _, _ in x.plants}
    assert any(sum(xc.unusable(x.ext[c][i]) for c in xc.POINT_COLS) in (1, 2) for i in rows)


@pytest.mark.parametrize("lanes", [1, 7, 64, 1000])
def test_poison_mode_gives_the_derived_columns(lanes):
    """lanes = 1: one chain through every row, unusable points first (row 0), in the middle and last (the last row) in it;
    7 and 64: several rows per lane; 1000: a row per lane and idle lanes."""
    x = planted_call()
    ext = [x.ext[c] for c in xc.POINT_COLS]
    outs, bad = xh.normalize(ext, lanes=lanes)
    for c, got in zip(xc.POINT_COLS, outs):
        diff = np.nonzero((got != x.derived.dirty[c]).any(1))[0]
        assert not len(diff), (c, lanes, diff[:8].tolist())
    assert not bad.any(), "poison mode writes no flags"
    # two sources (a group call's row) and one (a registration's column) are the same points
    outs2, _ = xh.normalize(ext[1:], lanes=lanes)
    outs1, _ = xh.normalize(ext[:1], lanes=lanes)
    assert (outs2[0] == outs[1]).all() and (outs2[1] == outs[2]).all() and (outs1[0] == outs[0]).all()


def test_all_points_of_a_lane_unusable_and_a_single_row():
    x = xc.ExtCase(mc.valid_transcripts([3], seed=33), seed=34)
    for j, kind in enumerate(("Z=0", "Z=q", "U=q")):
        for col in xc.POINT_COLS:
            x.plant(0, j, col, kind)
    for lanes in (1, 3):
        outs, _ = xh.normalize([x.ext[c] for c in xc.POINT_COLS], lanes=lanes)
        assert all((got == 0xFF).all() for got in outs), lanes
    one = xc.ExtCase(mc.valid_transcripts([1], seed=35), seed=36)
    outs, _ = xh.normalize([one.ext[c] for c in xc.POINT_COLS], lanes=1)
    assert all((got == one.derived.dirty[c]).all() for c, got in zip(xc.POINT_COLS, outs))


@pytest.mark.parametrize("lanes", [1, 7, 1000])
def test_mode_off_is_what_the_verify_paths_get(lanes):
    """Without poison: the flag of a row is set exactly when one of its coordinates is >= q (per item, not per point), Z = 0
    gives (0, 0) and no flag, usable points of unflagged rows their quotients; byte for byte the harness entry the ingest tests
    have always used."""
    x = planted_call()
    ext = [x.ext[c] for c in xc.POINT_COLS]
    outs, bad = xh.normalize(ext, lanes=lanes, poison=False)
    old_outs, old_bad = hl.normalize(ext, lanes=lanes)
    assert (bad == old_bad).all() and all((a == b).all() for a, b in zip(outs, old_outs))
    big = lambda row: any(int.from_bytes(row[k:k + 32].tobytes(), "little") >= o.Q for k in (0, 32, 64))  # noqa: E731
    want_bad = np.array([any(big(e[i]) for e in ext) for i in range(x.n)], np.uint8)
    assert (bad == want_bad).all() and want_bad.sum() >= 3
    for c, e, got in zip(xc.POINT_COLS, ext, outs):
        for i in range(x.n):
            if want_bad[i]:
                continue
            zero = not e[i, 64:].any()
            assert (got[i] == (0 if zero else x.derived.dirty[c][i])).all(), (c, i)
    assert any(not e[i, 64:].any() and not want_bad[i] for e in ext for i in range(x.n)), "a Z = 0 in a row without a flag"


def full_call():
    """1601 shares: the four transcripts with planted points leave at most 4 x 4 shares uncompared, under 2 % of the call."""
    x = xc.ExtCase(mc.filler(1601, seed=41, top=5), seed=42)
    xc.plant_everywhere(x, boundary=x.T // 3)
    x.derived.bad_z(5, 0, o.R_ORDER)
    return x


def test_whole_call_against_the_oracle_on_the_derived_columns():
    x = full_call()
    e = mc.expected(x.derived)
    assert 0 < e.uncompared and e.uncompared * 50 < x.n, "the planted points stay within the cap of multisig_cases.check"
    affine = hl.multisig(*x.derived.args())
    for lanes in (64, 4096):                       # 26 rows per lane; a row per lane
        got = xh.combine(*x.args(), lanes=lanes)
        assert mc.check(x.derived, e, got, f"ext host lanes={lanes}") == e.uncompared
        for name, a, b in zip(mc.OUTPUTS, got, affine):
            assert (a == b).all(), (name, lanes)
    st, ts = got[0], got[4]
    for t, j, _, _ in x.plants:
        assert st[x.derived.row(t, j)] == 3 and ts[t] != 0 and not got[2][t].any() and not got[3][t].any(), (t, j)


def group_call(n=3, T=120, mix=True):
    gc = gcs.group_transcripts(n, T, seed=50 + n)
    if mix:
        gcs.mix(gc)
    x = xc.ExtCase(gc.case, seed=51)
    pk_ext = xc.to_ext_column(gc.PK, np.random.default_rng(52), xc.CHOSEN_Z)
    return gc, x, pk_ext


def test_group_from_extended_keys_is_the_group_from_affine_keys():
    gc, x, pk_ext = group_call()
    assert (xc.derive_column(pk_ext) == gc.PK).all()
    x.plant(20, 0, "R", "Z=0"); x.plant(21, 2, "S", "V=q+1"); x.plant(119, 2, "R", "Z=q")
    x.check_derived()
    gd = gcs.GroupCase(gc.PK, x.derived)
    e = mc.expected(x.derived)
    for lanes, by_participant in ((1, False), (16, True)):
        rc, got, agg = xh.group_combine(pk_ext, x.derived.dirty["z"], x.ext["R"], x.ext["S"], x.derived.dirty["m"], lanes, by_participant)
        assert rc == 0
        rc2, want, agg2 = gh.combine(gc.PK, *gd.call_args(), by_participant=by_participant)
        assert rc2 == 0 and (agg == agg2).all()
        for a, b in zip(got, want):
            assert (a == b).all(), lanes
        mc.check(x.derived, e, gcs.as_inline_outputs(gd, agg, got), f"ext group lanes={lanes}")
    assert got[0][x.derived.row(20, 0)] == 3 and got[3][20] == 3 and got[3][21] != 0 and got[3][119] != 0


@pytest.mark.parametrize("kind", xc.KINDS)
def test_a_registration_with_an_unusable_key_is_refused(kind):
    gc, x, pk_ext = group_call(T=2, mix=False)
    assert xh.check_keys(pk_ext) == 0
    for j in (0, 2):
        spoilt = pk_ext.copy()
        xc.spoil(spoilt[j], kind)
        assert xh.check_keys(spoilt) == -1, (kind, j)
        rc, _, _ = xh.group_combine(spoilt, x.derived.dirty["z"], x.ext["R"], x.ext["S"], x.derived.dirty["m"])
        assert rc == -1
    assert xh.check_keys(pk_ext[:0]) == -1
