"""The battery of tests/adversarial_matrix_cases.py without a GPU: its class counts per scheme and format, the C oracle against
the Python oracle on the two new classes, the wire model against `decompress` on the battery's own bytes, and the new classes
(`exact`, `precedence`) through every path of the CPU build -- hl.verify, the latency path at 4, 8 and 16 pieces, the key tables
at both window widths, the registered key set in its variants, and both verdict libraries.  When a cell of
test_adversarial_matrix_gpu.py fails, these say whether the shared JJS_HD logic or a device-only part is wrong."""
import numpy as np
import pytest

import adversarial_matrix_cases as amc
import hostlib as hl
import jjs_oracle as o
import keyset_hostlib as kh
import keyset_verdict_hostlib as kv
import verdict_hostlib as vh
from helpers import make_batch, oracle_verify, pt_bytes, to_pt

SCHEMES = list(amc.SCHEMES)


def new_classes(scheme):
    rows = amc.class_rows(scheme, "exact", "precedence")
    return amc.subset(amc.battery(scheme)[0], rows), amc.forms(scheme).want()[rows]


def test_every_class_is_there_in_every_scheme_and_format():
    amc.assert_class_counts()
    assert set(amc.CLASS_COUNTS) == {(s, f) for s in amc.SCHEMES for f in amc.FORMATS}
    for scheme in SCHEMES:
        want = amc.forms(scheme).want()
        assert set(want.tolist()) == {0, 1, 2, 3}
        assert len(amc.battery(scheme)[1]) == len(want)
        print(scheme, "battery of %d items built in %.2f s" % (len(want), amc.BUILD_SECONDS[scheme]), amc.CLASS_COUNTS[(scheme, "affine")])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_c_and_python_oracles_agree_on_the_new_classes(scheme):
    amc.check_new_classes_against_python_oracle(scheme)
    # every exact item: a key column with torsion, and the equation(s) holding as they stand (asserted where they are built)
    b, names, parts = amc.exact_batch(scheme)
    assert len(set(names)) == len(names) and any(any(p) for p in parts) and any(not all(p) for p in parts)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_wire_model_against_decompress_on_the_battery_s_own_bytes(scheme):
    f = amc.forms(scheme)
    b = f.affine
    any_bad = np.zeros(f.n, bool)
    same = np.ones(f.n, bool)
    kinds = set()
    for k in amc.point_cols(scheme):
        big = amc.non_canonical_rows(b[k])
        for i in range(f.n):
            enc = f.wire[k][i].tobytes()
            p = o.decompress(enc)
            assert (p is None) == bool(f.undecodable[k][i]), (k, i)
            if p is not None:
                assert f.decoded[k][i].tobytes() == pt_bytes(p).tobytes() and o.is_on_curve(p) and o.compress(p) == enc, (k, i)
            if big[i]:
                assert p is None, (k, i)                         # a coordinate >= q: one of the undecodable encodings
                kinds.add(enc)
            elif o.is_on_curve(to_pt(b[k][i])):
                assert p == to_pt(b[k][i]), (k, i)                # a point of the curve survives the round trip
            same[i] &= p is not None and p == to_pt(b[k][i])
        any_bad |= f.undecodable[k]
    assert len(kinds) == 3                                        # v >= q, u = 0 with the sign bit, a non-residue
    want_w, want_a = f.want("wire"), f.want("affine")
    assert (want_w[any_bad] == 3).all() and (want_w[same] == want_a[same]).all()
    assert any_bad.sum() >= 3 and set(want_w.tolist()) == {0, 1, 2, 3}
    # keys from one format, signatures from the other: the wire columns alone decide what is undecodable
    key_bad = np.any([f.undecodable[k] for k in amc.KEYCOLS[scheme]], axis=0)
    sig_bad = np.any([f.undecodable[k] for k in amc.RCOLS[scheme]], axis=0)
    assert (f.want("wire", "affine")[key_bad] == 3).all() and (f.want("affine", "wire")[sig_bad] == 3).all()
    assert key_bad.any() and sig_bad.any()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_shapes_the_device_cells_rely_on(scheme):
    """Tiled to the smallest size at which the key tables engage, the battery's keys repeat at least 128 times in every key
    column (wide windows) in every format, and the battery with its filler has more than n / 128 and at most n / 16 keys per
    column (narrow windows).  The twins: distinct bytes, validity flipped, statuses from the oracle."""
    least = 65536 if scheme == "single" else 32768
    f = amc.forms(scheme)
    reps = amc.reps_for(f.n, least)
    n = reps * f.n
    assert reps >= 128 and n - f.n < least <= n
    for cols in (f.key_arrays("affine"), amc.wire_key_columns(f.key_arrays("wire")[0])):
        assert all(d * 128 <= n for d in amc.distinct_keys(cols))
    big, want = amc.tiled(f.affine, f.want(), 3)
    assert (want == oracle_verify(scheme, big)).all()
    assert amc.distinct_keys([big[k] for k in amc.KEYCOLS[scheme]]) == amc.distinct_keys(f.key_arrays("affine"))
    nf = amc.narrow_forms(scheme)
    n = amc.reps_for(nf.n, least) * nf.n
    for cols in (nf.key_arrays("affine"), amc.wire_key_columns(nf.key_arrays("wire")[0])):
        assert all(n < d * 128 and d * 16 <= n for d in amc.distinct_keys(cols)), (n, amc.distinct_keys(cols))
    tf, made, flipped = amc.twin_forms(scheme)
    assert made >= 60 and flipped == made
    changed = np.any([(tf.affine[k] != f.affine[k]).any(1) for k in amc.KEYCOLS[scheme]], axis=0)
    assert 0 < changed.sum() < f.n and (tf.want()[~changed] == f.want()[~changed]).all() and (tf.want() != f.want()).any()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_new_classes_through_every_host_path(scheme):
    b, want = new_classes(scheme)
    st, tally = hl.verify(scheme, b)
    assert st.tolist() == want.tolist()
    assert tally.tolist() == [int((want == k).sum()) for k in range(4)]
    for positions in (4, 8, 16):
        assert hl.verify_small(scheme, b, positions)[0].tolist() == want.tolist(), positions
    for window in (5, 6):
        assert hl.verify_keyed(scheme, b, window)[0].tolist() == want.tolist(), window


@pytest.mark.parametrize("scheme", SCHEMES)
def test_twins_and_tiled_battery_through_the_host_key_tables(scheme):
    """What the device's memo and grouping kernels must reproduce: the battery three times over (keys shared by several items)
    and the twin batch, on the CPU build of the key-table path at both window widths."""
    f = amc.forms(scheme)
    tf = amc.twin_forms(scheme)[0]
    for b, want in (amc.tiled(f.affine, f.want(), 3), (tf.affine, tf.want())):
        for window in (5, 6):
            st = hl.verify_keyed(scheme, b, window)[0]
            bad = np.nonzero(st != want)[0]
            assert not len(bad), (window, bad[:8].tolist(), st[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("scheme", SCHEMES)
def test_new_classes_against_a_registered_key_set_on_the_host(scheme):
    b, want = new_classes(scheme)
    cat = np.ascontiguousarray(np.concatenate([b[k] for k in amc.KEYCOLS[scheme]], 1))
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    keys, idx = [uniq[:, 64 * i:64 * i + 64] for i in range(len(amc.KEYCOLS[scheme]))], inv.reshape(-1).astype(np.uint32)
    for positions in (0, 4, 8, 16):
        st, _ = kh.verify(scheme, keys, idx, b["u"], b["R"], b.get("Rp"), b["m"], positions)
        np.testing.assert_array_equal(st, want, err_msg=f"positions={positions}")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_key_status_reference_of_the_battery_s_keys(scheme):
    """What the device tests hold KeySet.key_status against: the C oracle's point flags, here against the Python oracle's
    `point_is_valid` key by key, in the affine and in the wire registration; and the CPU build of the key set agrees."""
    f = amc.forms(scheme)
    for fmt in ("affine", "wire"):
        keys, idx, first = amc.registered(scheme, f, fmt)
        ref = amc.key_status_reference(scheme, f, fmt, first)
        assert set(ref.tolist()) == {0, 1, 3}
        assert (first == np.array([np.nonzero(idx == k)[0][0] for k in range(len(first))])).all()
        for k, item in enumerate(first):
            if fmt == "wire":
                pts = [o.decompress(f.wire[c][item].tobytes()) for c in amc.KEYCOLS[scheme]]
                malformed = any(p is None for p in pts)
            else:
                pts = [to_pt(f.affine[c][item]) for c in amc.KEYCOLS[scheme]]
                malformed = any(p[0] >= o.Q or p[1] >= o.Q for p in pts)
            want = 3 if malformed else (0 if all(o.point_is_valid(p) for p in pts) else 1)
            assert ref[k] == want, (fmt, k, int(item))
        if fmt == "affine":
            b = f.affine
            _, key_status = kh.verify(scheme, keys, idx, b["u"], b["R"], b.get("Rp"), b["m"], 0)
            np.testing.assert_array_equal(key_status, ref)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_new_classes_under_both_verdict_libraries(scheme):
    """No item of the new classes has status 0: the batch of them is rejected, and so is every one of them alone among valid
    signatures, at the first, a middle or the last position in turn -- inline keys and a registered set."""
    b, want = new_classes(scheme)
    assert (want != 0).all()
    assert vh.verify_all(scheme, b) == 0
    good = make_batch(scheme, 6, seed=33, n_keys=3, mix=False)
    assert vh.verify_all(scheme, good) == 1
    both = amc.concat(good, b)
    cat = np.ascontiguousarray(np.concatenate([both[k] for k in amc.KEYCOLS[scheme]], 1))
    uniq, inv = np.unique(cat, axis=0, return_inverse=True)
    keys, idx = [uniq[:, 64 * i:64 * i + 64] for i in range(len(amc.KEYCOLS[scheme]))], inv.reshape(-1).astype(np.uint32)
    assert kv.verify_all(scheme, keys, idx, both)["verdict"] == 0
    assert kv.verify_all(scheme, keys, idx[:6], good)["verdict"] == 1
    for i in range(len(want)):
        pos = (0, 3, 6)[i % 3]                 # (the device child places every item at all three: adversarial_matrix_child.py)
        sel = np.array(list(range(pos)) + [6 + i] + list(range(pos, 6)))
        one = amc.subset(both, sel)
        assert vh.verify_all(scheme, one) == 0, (i, pos)
        assert kv.verify_all(scheme, keys, idx[sel], one)["verdict"] == 0, (i, pos)
