"""The affine key tables on the device.  The stage records of tests/affine_tables_cases.py through tools/scalarcheck (the same
records the CPU build runs; one of them is one full wave, the others end in a partly filled one), then end to end: single
signatures over 256 keys (wide windows) and over 2 048 keys (narrow windows) at 65 536 items, double and per-item-generator
signatures at 32 768, three calls in one call slot (the first, the same again so that every key is in the slot's memo, one with
half its keys new), a registered key set in both of its variants and a signer group.  The batches are built here so that every
item's status is known by construction -- valid, wrong key, tampered message, a point that is the identity, of order 2 or of
mixed order -- and a 4 096-item sample of every construction is held against the C oracle."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import affine_tables_cases as atc
import scalar_mul_cases as smc
from helpers import ARG_ORDER, IDENT, ORDER2, _add_order2, make_batch, oracle_verify

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "jubjub_schnorr_amd", "tools", "scalarcheck")
KEYCOLS = {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}
RCOLS = {"single": ["R"], "double": ["R", "Rp"], "vargen": ["R"]}
SAMPLE = 4096


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import jubjub_schnorr_amd as jjs
    return jjs.engine()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the stage records ----
@pytest.fixture(scope="module")
def recs(tmp_path_factory):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_tools()
    r = atc.build_records()
    d = tmp_path_factory.mktemp("affine_tables")
    smc.input_words(r).tofile(d / "in.bin")
    p = subprocess.run([EXE, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = np.fromfile(d / "out.bin", np.uint32)
    assert len(out) == atc.output_words(r)
    return atc.attach_outputs(r, out)


def test_stage_records_on_a_full_and_on_partly_filled_waves(recs):
    assert len(recs["kt_add_challenge w=6"]["rows"]) == 64 and len(recs["kt_add_challenge w=5"]["rows"]) % 64
    atc.check_tables_are_affine(recs)
    atc.check_scalars(recs)
    atc.check_challenges(recs)


# ---- batches whose statuses are known by construction ----
@functools.lru_cache(None)
def construct(scheme, n_base, n_keys, seed):
    """n_base items over n_keys keys (item i under key i mod n_keys), all signed by the oracle, then by position: i mod 64 == 3
    takes the next item's public key (status 2), 7 has its message changed (2), 11 / 13 / 17 get the identity / the point of
    order 2 / their own point plus the point of order 2 in one of their point columns in turn (1).  -> (batch, statuses)"""
    b = make_batch(scheme, n_base, seed=seed, n_keys=n_keys, mix=False)
    b = {k: v.copy() for k, v in b.items()}
    want = np.zeros(n_base, np.uint8)
    i = np.arange(n_base)
    cols = KEYCOLS[scheme] + RCOLS[scheme]
    wrong = i[i % 64 == 3]
    own = b["PK"][wrong].copy()
    b["PK"][wrong] = b["PK"][(wrong + 1) % n_base]
    assert not (b["PK"][wrong] == own).all(1).any()
    tamper = i[i % 64 == 7]
    b["m"][tamper, 0] ^= 1
    b["m"][tamper, 31] &= 0x3F
    want[wrong] = want[tamper] = 2
    for cls, point in ((11, IDENT), (13, ORDER2), (17, None)):
        rows = i[i % 64 == cls]
        for j, name in enumerate(cols):
            r = rows[j::len(cols)]
            b[name][r] = point if point is not None else _add_order2(b[name][r])
        want[rows] = 1
    sample = {k: v[:SAMPLE] for k, v in b.items()}
    assert (oracle_verify(scheme, sample) == want[:SAMPLE]).all(), "the construction against the C oracle"
    assert all((want[:SAMPLE] == s).sum() > 0 for s in (0, 1, 2))
    return b, want


def tiled(b, want, reps):
    return {k: np.tile(v, (reps, 1)) for k, v in b.items()}, np.tile(want, reps)


def run(eng, scheme, b, want, path):
    import torch
    torch.cuda.synchronize()
    before = eng.path_stats()
    st, tally = eng.verify(scheme, *[dev(b[k]) for k in ARG_ORDER[scheme]])
    st, tally = st.cpu().numpy(), tally.cpu().numpy()
    after = eng.path_stats()
    bad = np.nonzero(st != want)[0]
    assert not len(bad), (scheme, len(bad), bad[:8].tolist(), st[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert tally.tolist() == [int((want == k).sum()) for k in range(4)]
    assert after[path] == before[path] + 1, (path, before, after)


@pytest.mark.parametrize("n_keys,path", [(256, "key_tables_wide"), (2048, "key_tables_narrow")])
def test_single_65536_items_wide_and_narrow_windows(eng, n_keys, path):
    b, want = construct("single", 8192, n_keys, 41)
    run(eng, "single", *tiled(b, want, 8), path)


@pytest.mark.parametrize("scheme", ["double", "vargen"])
def test_double_and_vargen_32768_items(eng, scheme):
    b, want = construct(scheme, 4096, 128, 43)
    run(eng, scheme, *tiled(b, want, 8), "key_tables_wide")


def test_three_calls_in_one_slot(eng):
    """139 264 items, more than a medium slot takes: calls that follow each other on one stream stay in the first big slot.  The
    second call finds every key in the slot's memo; the third brings half the keys of the first and as many new ones.
    NOT checked here: that the calls shared a slot and how many keys hit -- the product library has no counter for it.  The
    profiling library has (jjs_debug_key_memo_stats), and tests/key_memo_child.py holds every call's hits and built keys of
    such sequences against a model; this test adds the statuses of items that are not valid on tables that outlive a call."""
    a, want_a = construct("single", 8192, 256, 41)
    c, want_c = construct("single", 8192, 256, 47)
    old = (np.arange(8192) % 256) < 128
    half = {k: np.where(old[:, None], a[k], c[k]) for k in a}
    want_half = np.where(old, want_a, want_c)
    assert (oracle_verify("single", {k: v[:SAMPLE] for k, v in half.items()}) == want_half[:SAMPLE]).all()
    eng.trim()
    for b, want in ((a, want_a), (a, want_a), (half, want_half)):
        run(eng, "single", *tiled(b, want, 17), "key_tables_wide")


def test_registered_key_set_both_variants(eng):
    b, want = construct("single", 8192, 256, 41)
    big, want_big = tiled(b, want, 8)
    uniq, idx = np.unique(big["PK"], axis=0, return_inverse=True)
    idx = idx.reshape(-1).astype(np.uint32)
    with eng.keyset("single", np.ascontiguousarray(uniq)) as ks:
        for n in (len(idx), SAMPLE):                   # the large variant (key_verify_kernel) and the latency variant
            st, tally = ks.verify(dev(idx[:n]), dev(big["u"][:n]), dev(big["R"][:n]), dev(big["m"][:n]))
            assert (st.cpu().numpy() == want_big[:n]).all(), n
            assert tally.cpu().numpy().tolist() == [int((want_big[:n] == k).sum()) for k in range(4)]
        info = ks.info()
        assert info["large_calls"] == 1 and info["small_calls"] == 1 and info["window_bits"] == 6


def test_signer_group(eng):
    import msig_group_cases as gcs
    import multisig_cases as mc
    gc = gcs.group_transcripts(3, 40, seed=300, threads=16)
    gcs.mix(gc)
    e = mc.expected(gc.case, 16)
    with eng.multisig_group(gc.PK) as grp:
        out = tuple(x.cpu().numpy() for x in grp.combine(*[dev(x) for x in gc.call_args()]))
        mc.check(gc.case, e, gcs.as_inline_outputs(gc, grp.aggregate_pk, out), "signer group on affine tables")
        assert grp.info()["window_bits"] == 6
