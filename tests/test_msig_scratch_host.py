"""The layout and the growth of the device's multisignature scratch (csrc/msig_scratch.h) compiled for the CPU: at every capacity
vector the regions lie inside the allocation, apart from each other and aligned as the kernels read them, an unasked region is
null, and the allocation is no larger than the formula the engine kept by hand before the walk existed; the growth rule gives
what the five hand-written stanzas it replaces gave."""
import pytest

import msig_scratch_hostlib as ml

BASE = 0x7F0000001300 & ~0xFF            # a 256-byte-aligned address, as the device allocator gives


def caps(rows, transcripts, ext_rows=0, ks=(0, 0), sign=(0, 0), share=(0, 0)):
    return dict(zip(ml.DIMS, (rows, transcripts, ext_rows, *ks, *sign, *share)))


VECTORS = {
    "rows and transcripts": caps(4096, 3072),
    "ext alone": caps(4096, 3072, 4096),
    "key set alone": caps(4096, 3072, ks=(4096, 3072)),
    "sign alone": caps(4096, 3072, sign=(4096, 3072)),
    "share alone": caps(4096, 3072, share=(4096, 3072)),
    "all regions": caps(6144, 3072, 8192, (4096, 4096), (6144, 3072), (12288, 3072)),
    "rows 4097, one transcript": caps(4097, 1),
    "one query": caps(4097, 1, share=(1, 1)),
    "all regions, odd sizes": caps(4097, 1, 4099, (4097, 1), (4101, 3), (1, 1)),
    "all regions, one of everything": caps(1, 1, 1, (1, 1), (1, 1), (1, 1)),
    "transcripts much larger than rows": caps(5, 100003, 7, (5, 100003), (5, 100001), (3, 100005)),
    "optional transcripts 0": caps(4096, 3072, 4096, (4096, 0), (4096, 0), (4096, 0)),
}


def extents(c):
    """Bytes of every region: what the kernels index."""
    ew = ml.ext_words()
    n, t = c["rows"], c["transcripts"]
    return {"tr_of": 4 * n, "d_words": 32 * n, "dpk": 4 * ew * n, "e_pt": 4 * ew * n,
            "a_words": 32 * t, "c_words": 32 * t, "offsets": 4 * (t + 1), "long_tags": 72 * t,
            "norm0": 64 * c["ext_rows"], "norm1": 64 * c["ext_rows"], "norm2": 64 * c["ext_rows"], "prefix": 36 * c["ext_rows"],
            "ks_pk": 64 * c["ks_rows"], "ks_row_key": 4 * c["ks_rows"], "ks_refused": 4 * c["ks_transcripts"],
            "pk_repeats": 4 * c["sign_rows"], "bad_enc": 4 * c["sign_transcripts"], "dup_nonce": 4 * c["sign_transcripts"],
            "sign_agg": 64 * c["sign_transcripts"], "sign_rsa": 64 * c["sign_transcripts"],
            "share_pt": 4 * ew * c["share_queries"], "share_bad": 4 * c["share_transcripts"],
            "share_agg": 64 * c["share_transcripts"], "share_rsa": 64 * c["share_transcripts"]}


def parent_bytes(c):
    """msig_scratch_bytes as the engine had it, slack constants and all: the bound."""
    ew = ml.ext_words()
    q, qt, n, t, e = c["share_queries"], c["share_transcripts"], c["rows"], c["transcripts"], c["ext_rows"]
    k, kt, s, st = c["ks_rows"], c["ks_transcripts"], c["sign_rows"], c["sign_transcripts"]
    return ((q * 4 * ew + qt * (4 + 128) + 128 if q else 0) + n * 4 * (1 + 8 + 2 * ew) + t * 4 * (16 + 1 + 18) + 64 +
            (e * (3 * 64 + 9 * 4) + 64 if e else 0) + (k * (64 + 4) + kt * 4 + 128 if k else 0) + (s * 4 + st * (8 + 128) + 128 if s else 0))


@pytest.mark.parametrize("name", list(VECTORS))
def test_layout(name):
    c = VECTORS[name]
    at, nbytes, flag_words = ml.layout(BASE, c)
    size = extents(c)
    assert ml.ext_words() == 36
    live = []
    for region, dim, align in ml.REGIONS:
        if c[dim] == 0:
            assert at[region] == 0, f"{region}: {dim} is 0, the region is not null"
            continue
        assert at[region] != 0, f"{region} is null"
        assert at[region] % align == 0, f"{region} is not {align}-byte aligned"
        assert BASE <= at[region] and at[region] + size[region] <= BASE + nbytes, f"{region} leaves the allocation"
        if size[region]:
            live.append((at[region], at[region] + size[region], region))
    live.sort()
    for (_, hi, a), (lo, _, b) in zip(live, live[1:]):
        assert hi <= lo, f"{a} and {b} overlap"
    if c["sign_rows"]:                    # one run of words that one memset clears
        assert at["bad_enc"] == at["pk_repeats"] + size["pk_repeats"] and at["dup_nonce"] == at["bad_enc"] + size["bad_enc"]
        assert flag_words == c["sign_rows"] + 2 * c["sign_transcripts"]
    assert nbytes <= parent_bytes(c), (nbytes, parent_bytes(c))
    # the size alone, from a null base: where the same walk ends
    assert ml.layout(0, c)[1] == nbytes


def grown(want):
    cap = 4096
    while cap < want:
        cap <<= 1
    mid = cap // 4 * 3
    return mid if mid >= want else cap


def parent_grown(held, need):
    """ensure_msig_scratch as the engine had it, stanza by stanza."""
    if all(need[d] <= held[d] for d in ml.DIMS):
        return dict(held)
    n, t, e = need["rows"], need["transcripts"], need["ext_rows"]
    ci, ct = grown(max(n, 4096)), grown(max(t, 1024))
    ce = grown(max(e, 4096)) if e else 0
    ci, ct, ce = max(ci, held["rows"]), max(ct, held["transcripts"]), max(ce, held["ext_rows"])
    out = {"rows": ci, "transcripts": ct, "ext_rows": ce}
    for rows, trs in (("ks_rows", "ks_transcripts"), ("sign_rows", "sign_transcripts"), ("share_queries", "share_transcripts")):
        cr = grown(max(need[rows], 4096)) if need[rows] else 0
        cq = grown(max(need[trs], 1024)) if need[rows] else 0
        out[rows], out[trs] = max(cr, held[rows]), max(cq, held[trs])
    return out


EMPTY = caps(0, 0)
FIRST = caps(4096, 3072)                 # what the first tiny call leaves
FULL = caps(6144, 3072, 4096, (4096, 3072), (4096, 3072), (4096, 3072))
PAIRS = {
    "the first call": (EMPTY, caps(4, 3)),
    "the first call, no rows": (EMPTY, caps(0, 1)),
    "need within held": (FULL, caps(6144, 3072, 4096, (1, 3), (4096, 1), (7, 3072))),
    "need equal to held in an optional region only": (FULL, caps(1, 1, share=(4096, 3072))),
    "rows alone": (FULL, caps(6145, 3)),
    "transcripts alone": (FULL, caps(4, 3073)),
    "ext rows alone": (FULL, caps(4, 3, 4097)),
    "share queries alone, beyond the rows": (FULL, caps(4, 3, share=(50000, 3))),
    "sign transcripts alone": (FULL, caps(4, 3, sign=(4, 3073))),
    "ext for the first time": (FIRST, caps(4, 3, 4)),
    "a key set for the first time, the others held": (caps(6144, 3072, 4096, sign=(4096, 3072), share=(4096, 3072)), caps(4, 3, ks=(4, 3))),
    "sign for the first time": (FIRST, caps(4, 3, sign=(4, 3))),
    "share for the first time, one query": (FIRST, caps(4, 3, share=(1, 3))),
    "rows asked for with 0 transcripts": (FIRST, caps(4, 3, ks=(1, 0), sign=(1, 0), share=(1, 0))),
    "transcripts asked for without rows": (FIRST, caps(4, 3, ks=(0, 5), sign=(0, 5), share=(0, 5))),
    "just above the floors": (EMPTY, caps(4097, 1025, 4097, (4097, 1025), (4097, 1025), (4097, 1025))),
    "at the floors": (EMPTY, caps(4096, 1024, 4096, (4096, 1024), (4096, 1024), (4096, 1024))),
    "just above a step of grown()": (FULL, caps(6145, 3073, 6145, (8193, 4097), (12289, 6145), (16385, 8193))),
    "at a step of grown()": (FULL, caps(6144, 3072, 6144, (8192, 4096), (12288, 6144), (16384, 8192))),
    "one grows, one shrinks": (FULL, caps(100000, 1, 1, (1, 1), (1, 1), (1, 1))),
}


@pytest.mark.parametrize("name", list(PAIRS))
def test_growth(name):
    held, need = PAIRS[name]
    got, want = ml.grown(held, need), parent_grown(held, need)
    assert got == want
    assert all(got[d] >= held[d] for d in ml.DIMS), "a capacity shrank"
    if name in ("need within held", "need equal to held in an optional region only"):
        assert got == held
