"""The moments mk_alpha_stats reduces from the tables (mk_alpha_k in mk_table.hip, the host's part in mk_api.hip) field by
field against tests/alpha_moments.exact_moments: big-integer observed / total / freq / sum of squares, sum c ln c at 50
digits.  The tables are built with chosen counts through Counter.load_tsv(bytes) (tests/test_gpu_tsv_load.py verifies that
route), which reaches every table kind and every count up to 2^64 - 1.

  integer fields   equal
  sum_sq           the exact sum rounded to float64 once -- the kernel carries 192 bits, so with any counts at all
  sum_clnc         |got - ref| <= (rows + 8) * 2^-53 * ref (alpha_moments.clnc_bound: rows - 1 additions of non-negative
                   terms in any order, and per term the conversion, the product and a logarithm of 1 ulp -- what the device
                   library documents for its float64 log)
  repeats          the same table gives the same bytes"""
import random
import struct

import numpy as np
import pytest

import alpha_moments as am
from mercat2_amd import diversity, native
from oracle import alpha_ref, cpu_ref

pytestmark = pytest.mark.gpu
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
LETTERS = {NT: b"ACGT", AA: b"ACDEFGHIKLMNPQRSTVWY", RAW: b"ACGT"}
SINGLES = b"nacgtxyz.-*0123456789"   # one-byte keys outside both packed alphabets
SIDE_KEY = b"T" * 32                 # the one-word table's free-slot mark: its count lives beside the table
INT_FIELDS = ("observed", "total", "freq")


# ------------------------------------------------------------------------------------------------ building tables
def _packed_keys(alphabet, k, n, start=0):
    """(n, k) uint8: the numbers start .. start + n - 1 in the alphabet's letters, most significant first."""
    letters = np.frombuffer(LETTERS[alphabet], dtype=np.uint8)
    base, nd = len(letters), min(k, 13)
    assert start + n <= base ** nd
    i = np.arange(start, start + n, dtype=np.uint64)
    pw = np.array([base ** e for e in range(nd - 1, -1, -1)], dtype=np.uint64)
    out = np.full((n, k), letters[0], dtype=np.uint8)
    out[:, k - nd:] = letters[((i[:, None] // pw[None, :]) % np.uint64(base)).astype(np.int64)]
    return out


def _text_keys(alphabet, k, n):
    """n distinct keys no packed table takes: an 'N' ('n' for protein, where N is a residue) in front, or a lower-case
    last letter."""
    if k == 1:
        assert n <= len(SINGLES)
        return np.frombuffer(SINGLES[:n], dtype=np.uint8).reshape(n, 1).copy()
    assert n <= len(LETTERS[alphabet]) ** min(k - 1, 13)
    out = _packed_keys(alphabet, k, n)
    out[0::2, 0] = ord("N") if alphabet != AA else ord("n")
    out[1::2, -1] += 32
    return out


def _tsv(keys, counts):
    flat, k = keys.tobytes(), keys.shape[1]
    assert len(counts) == keys.shape[0]
    return b"".join(flat[i * k:(i + 1) * k] + b"\t%d\n" % c for i, c in enumerate(counts))


def _counts(n, rng, top=1 << 40):
    """n counts from a palette: every count 1..11 (the freq fields and their edge) and values up to ``top``."""
    palette = list(range(1, 12)) + [rng.randint(12, 1000) for _ in range(200)] + [rng.randint(1001, top) for _ in range(200)]
    return [rng.choice(palette) for _ in range(n)]


def _load(ctx, keys, counts, **kw):
    return ctx.load_tsv(_tsv(keys, counts), **kw) if len(counts) else None


def _slots(ctx):
    """Slots (or dense bins) of the tables the context holds, as mk_histo walks them -- the walk of mk_alpha_stats."""
    info = {}
    ctx.histo(10, info)
    return info["slots"]


def _differences(got, counts, slack=1):
    """[(field, got, want)] where ``got`` is not the exact moments of ``counts`` (sum_clnc: beyond slack x the bound)."""
    want = am.exact_moments(counts)
    bad = [(f, got[f], want[f]) for f in INT_FIELDS if got[f] != want[f]]
    if got["sum_sq"] != want["sum_sq"]:
        bad.append(("sum_sq", got["sum_sq"].hex(), want["sum_sq"].hex(), "sum c^2 = %d" % am.sum_squares(counts)))
    err, bound = abs(got["sum_clnc"] - want["sum_clnc"]), slack * am.clnc_bound(want["observed"], want["sum_clnc"])
    if not err <= bound:
        bad.append(("sum_clnc", got["sum_clnc"], want["sum_clnc"], "off by %.3g, bound %.3g" % (err, bound)))
    return bad


def _check(ctx, counts):
    got = ctx.alpha_stats()
    bad = _differences(got, counts)
    assert not bad, bad
    return got


# ---------------------------------------------------------------------------------------------------- table kinds
PACKED = [(NT, 1, "dense", 4), (NT, 3, "dense", 50), (NT, 7, "dense", 5000), (AA, 3, "dense", 3000),
          (NT, 21, "hash64", 3000), (NT, 32, "hash64", 3000), (AA, 12, "hash64", 3000),
          (NT, 33, "hash128", 3000), (NT, 64, "hash128", 3000), (AA, 13, "hash128", 3000), (AA, 25, "hash128", 3000)]


@pytest.mark.parametrize("with_text", [False, True], ids=["packed", "packed+text"])
@pytest.mark.parametrize("alphabet,k,mode,n", PACKED, ids=["%s%d" % ("nt" if p[0] == NT else "aa", p[1]) for p in PACKED])
def test_packed_tables(alphabet, k, mode, n, with_text):
    rng = random.Random(1000 * k + alphabet)
    n_text = 0 if not with_text else min(700, len(SINGLES) if k == 1 else len(LETTERS[alphabet]) ** (k - 1))
    keys = np.vstack([_packed_keys(alphabet, k, n), _text_keys(alphabet, k, n_text)]) if n_text else _packed_keys(alphabet, k, n)
    counts = _counts(n + n_text, rng)
    order = rng.sample(range(n + n_text), n + n_text)
    with native.Counter(k, alphabet) as ctx:
        info = _load(ctx, keys[order], [counts[i] for i in order])
        assert ctx.stats()["mode_name"] == mode and (info["packed_rows"], info["text_rows"]) == (n, n_text)
        _check(ctx, counts)
        # the packed rows alone and the text rows alone are other moments: neither table may be the only one read
        if n_text:
            assert _differences(ctx.alpha_stats(), counts[:n]) and _differences(ctx.alpha_stats(), counts[n:])


@pytest.mark.parametrize("alphabet,k", [(RAW, 9), (NT, 65), (AA, 26)], ids=["raw9", "nt65", "aa26"])
def test_text_only_tables(alphabet, k):
    rng = random.Random(k)
    keys = np.vstack([_packed_keys(alphabet, k, 3000), _text_keys(alphabet, k, 500)])
    counts = _counts(3500, rng)
    with native.Counter(k, alphabet) as ctx:
        info = _load(ctx, keys, counts)
        assert ctx.stats()["mode_name"] == "byref" and (info["packed_rows"], info["text_rows"]) == (0, 3500)
        _check(ctx, counts)


def test_three_tables_in_one_context():
    """Nucleotide 32-mers: one-word rows, rows kept as text and the 32 x 'T' key beside the table.  Both tables hold every
    count 1..10 and counts of up to 2^20 (so that 49 more shows in a float64 sum_sq), the side key counts 7: leaving out either table changes every field, leaving out the side
    key every field a single row can change."""
    rng = random.Random(32)
    low = list(range(1, 11))
    parts = {"packed": (_packed_keys(NT, 32, 2000), low + _counts(1990, rng, 1 << 20)),
             "text": (_text_keys(NT, 32, 900), low + _counts(890, rng, 1 << 20)),
             "side": (np.frombuffer(SIDE_KEY, dtype=np.uint8).reshape(1, 32), [7])}
    everything = [c for _, cs in parts.values() for c in cs]
    whole = am.exact_moments(everything)
    for name in parts:
        rest = am.exact_moments([c for other, (_, cs) in parts.items() if other != name for c in cs])
        changed = {f for f in ("observed", "total", "sum_sq", "sum_clnc") if rest[f] != whole[f]}
        changed |= {i for i in range(1, 11) if rest["freq"][i] != whole["freq"][i]}
        assert changed == {"observed", "total", "sum_sq", "sum_clnc"} | ({7} if name == "side" else set(range(1, 11))), name
    with native.Counter(32, NT) as ctx:
        for keys, counts in parts.values():
            _load(ctx, keys, counts)
        assert ctx.rows() == len(everything)
        _check(ctx, everything)


# -------------------------------------------------------------------------------------------------- launch shapes
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 255, 256, 257])
def test_row_counts_around_a_wave_and_a_workgroup(rows):
    counts = _counts(rows, random.Random(rows))
    with native.Counter(21, NT) as ctx:
        _load(ctx, _packed_keys(NT, 21, rows), counts)
        got = _check(ctx, counts)
        assert got["observed"] == rows


def test_a_grid_at_its_cap_where_every_lane_strides():
    """More slots than 2 x 1024 workgroups x 256 lanes: the launch is capped and every lane takes several slots."""
    rows = 300_000
    counts = _counts(rows, random.Random(7), top=1 << 36)
    with native.Counter(21, NT) as ctx:
        _load(ctx, _packed_keys(NT, 21, rows), counts)
        assert _slots(ctx) >= 2 * 1024 * 256
        _check(ctx, counts)


def test_every_lane_adds_to_the_same_freq_counter():
    counts = [1] * 100_000
    with native.Counter(21, NT) as ctx:
        _load(ctx, _packed_keys(NT, 21, len(counts)), counts)
        got = _check(ctx, counts)
        assert got["freq"][1] == got["total"] == 100_000 and got["sum_clnc"] == 0.0


def test_the_freq_boundary():
    counts = [10, 11] * 5000
    with native.Counter(21, NT) as ctx:
        _load(ctx, _packed_keys(NT, 21, len(counts)), counts)
        got = _check(ctx, counts)
        assert got["freq"] == [0] * 10 + [5000]


# --------------------------------------------------------------------------------------------------------- values
SPECIAL = [(1 << 32) - 1, 1 << 32, (1 << 53) + 1, 1 << 63, (1 << 64) - 1]


@pytest.mark.parametrize("alphabet,k", [(NT, 7), (NT, 21), (NT, 40), (RAW, 9)], ids=["dense", "one-word", "two-word", "text"])
def test_counts_at_the_edges_of_32_53_and_64_bits(alphabet, k):
    """total wraps modulo 2^64 as the header says; the sum of squares passes 2^128 and is still exact."""
    rng = random.Random(k)
    counts = SPECIAL * 3 + [rng.randint(1, 20) for _ in range(500)]
    rng.shuffle(counts)
    assert sum(counts) >= 1 << 64 and am.sum_squares(counts) >= 1 << 128
    with native.Counter(k, alphabet) as ctx:
        _load(ctx, _packed_keys(alphabet, k, len(counts)), counts)
        _check(ctx, counts)
    for one in SPECIAL:  # each alone beside small counts: the sum of squares stays below 2^128
        counts = [one] + [rng.randint(1, 20) for _ in range(70)]
        assert am.sum_squares(counts) < 1 << 128
        with native.Counter(k, alphabet) as ctx:
            _load(ctx, _packed_keys(alphabet, k, len(counts)), counts)
            _check(ctx, counts)


def test_squares_that_no_float64_sum_adds_exactly():
    """5000 counts in [2^31, 2^33): their squares need up to 66 bits, so a float64 running sum rounds at nearly every step
    and ends a few ulps from the exact sum rounded once."""
    rng = random.Random(31)
    palette = [rng.randrange(1 << 31, 1 << 33) for _ in range(am.PALETTE)]
    counts = [rng.choice(palette) for _ in range(5000)]
    naive = 0.0
    for c in counts:
        naive += float(c) * float(c)
    assert naive != float(am.sum_squares(counts))  # (the table does tell the two apart)
    with native.Counter(21, NT) as ctx:
        _load(ctx, _packed_keys(NT, 21, len(counts)), counts)
        _check(ctx, counts)


def test_the_side_key_is_added_in_integers():
    """The 32 x 'T' key with count 2^40 + 1 beside two rows of 2^13.  (2^40 + 1)^2 = 2^80 + 2^41 + 1 rounds to 2^80 + 2^41
    as a float64, and adding 2^27 to that is a tie that falls back; the integer sum 2^80 + 2^41 + 2^27 + 1 rounds up."""
    side, rest = (1 << 40) + 1, [1 << 13, 1 << 13]
    assert float(side) * float(side) + float(am.sum_squares(rest)) != float(am.sum_squares([side] + rest))
    keys = np.vstack([np.frombuffer(SIDE_KEY, dtype=np.uint8).reshape(1, 32), _packed_keys(NT, 32, 2)])
    with native.Counter(32, NT) as ctx:
        _load(ctx, keys, [side] + rest)
        _check(ctx, [side] + rest)


# ---------------------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize("alphabet,k", [(NT, 21), (NT, 40), (RAW, 9)], ids=["one-word", "two-word", "text"])
def test_a_table_that_grows_between_loads(alphabet, k):
    rng = random.Random(k)
    sizes = [300, 3000, 12_000, 40_000]
    keys, counts = _packed_keys(alphabet, k, sum(sizes)), _counts(sum(sizes), rng)
    with native.Counter(k, alphabet) as ctx:
        at, slots = 0, []
        for n in sizes:
            _load(ctx, keys[at:at + n], counts[at:at + n])
            at += n
            _check(ctx, counts[:at])
            slots.append(_slots(ctx))
        assert slots[0] < slots[-1]
        _load(ctx, keys[:5000], counts[:5000])  # the same keys again: counts add up, no new row
        _check(ctx, [2 * c for c in counts[:5000]] + counts[5000:])


@pytest.mark.parametrize("alphabet,k", [(NT, 7), (NT, 21), (NT, 40), (RAW, 9)], ids=["dense", "one-word", "two-word", "text"])
def test_after_filter_min(alphabet, k):
    """Rows below the minimum are gone; where a slot keeps its key with a count of 0 it is no row."""
    rng = random.Random(k)
    counts = _counts(4000, rng)
    with native.Counter(k, alphabet) as ctx:
        _load(ctx, _packed_keys(alphabet, k, len(counts)), counts)
        _check(ctx, counts)
        ctx.filter_min(9)
        kept = [c for c in counts if c >= 9]
        assert 0 < len(kept) < len(counts)
        got = _check(ctx, kept)
        assert got["freq"][:9] == [0] * 9 and got["freq"][9] > 0


def test_a_sharer_answers_for_its_own_tables_and_the_owner_for_all_rows():
    k = 31
    texts = [native.synth_reads(6_000, 40 + i, 1_500, 150, 50 + i, 0, i * 1_500).tobytes() for i in range(3)]
    texts[2] += b">n\n" + b"ACGTTGCANGGATCCATGNA" * 4 + b"\n"
    want = {}
    for text in texts:
        for key, n in cpu_ref.count_text(text, k, 1).items():
            want[key] = want.get(key, 0) + n
    owner, sharer = native.Counter(k, NT), native.Counter(k, NT)
    try:
        sharer.share_table(owner)
        owner.count_chunk(texts[0], 1)
        sharer.count_chunk(texts[1], 1)
        sharer.count_chunk(texts[2], 1)
        own = [ctx.to_dict() for ctx in (owner, sharer)]
        assert own[1] and len(own[0]) + len(own[1]) >= len(want)
        for ctx, table in zip((owner, sharer), own):
            _check(ctx, list(table.values()))
        owner.merge_from(sharer)
        assert owner.to_dict() == want
        _check(owner, list(want.values()))
    finally:
        sharer.share_table(None)
        owner.close()
        sharer.close()


@pytest.mark.parametrize("alphabet,k", [(NT, 5), (NT, 32), (NT, 40), (RAW, 9)], ids=["dense", "one-word", "two-word", "text"])
def test_after_merge_from(alphabet, k):
    """Two contexts with half their keys in common (text rows too, and the key beside the one-word table)."""
    rng = random.Random(k)
    n = 600
    keys = np.vstack([_packed_keys(alphabet, k, n), _text_keys(alphabet, k, 100)] +
                     ([np.frombuffer(SIDE_KEY, dtype=np.uint8).reshape(1, 32)] if k == 32 else []))
    rows = keys.shape[0]
    ca, cb = _counts(rows, rng), _counts(rows, rng)
    in_a = [i for i in range(rows) if i % 4 != 0 or i == rows - 1]
    in_b = [i for i in range(rows) if i % 4 != 1 or i == rows - 1]
    merged = {}
    for idx, cs in ((in_a, ca), (in_b, cb)):
        for i in idx:
            merged[i] = merged.get(i, 0) + cs[i]
    with native.Counter(k, alphabet) as a, native.Counter(k, alphabet) as b:
        _load(a, keys[in_a], [ca[i] for i in in_a])
        _load(b, keys[in_b], [cb[i] for i in in_b])
        a.merge_from(b)
        assert a.rows() == rows
        _check(a, list(merged.values()))
        _check(b, [cb[i] for i in in_b])


# -------------------------------------------------------------------------------------------------- repeatability
def _bytes(st):
    return struct.pack("<13Q2d", st["observed"], st["total"], *st["freq"], st["sum_sq"], st["sum_clnc"])


@pytest.fixture(scope="module")
def varied():
    """2^16 rows (keys, counts): a palette of small counts and counts of up to 33 bits."""
    rng = random.Random(16)
    palette = list(range(1, 12)) + [rng.randrange(1, 1 << 33) for _ in range(am.PALETTE - 11)]
    return _packed_keys(NT, 21, 1 << 16), [rng.choice(palette) for _ in range(1 << 16)]


def test_eight_calls_return_the_same_bytes(varied):
    keys, counts = varied
    with native.Counter(21, NT) as ctx:
        _load(ctx, keys, counts)
        first = _check(ctx, counts)
        seen = {_bytes(ctx.alpha_stats()) for _ in range(8)}
        assert seen == {_bytes(first)}, sorted(seen)


def test_the_same_rows_in_another_order(varied):
    """Another load order is another slot layout (the table grows at other moments, collisions resolve otherwise): the
    integer fields and sum_sq cannot depend on it, sum_clnc only within the bound of either."""
    keys, counts = varied
    order = random.Random(17).sample(range(len(counts)), len(counts))
    with native.Counter(21, NT) as a, native.Counter(21, NT) as b:
        _load(a, keys, counts, piece_bytes=1 << 16)
        _load(b, keys[order], [counts[i] for i in order])
        sa, sb = _check(a, counts), _check(b, counts)
        assert all(sa[f] == sb[f] for f in INT_FIELDS) and sa["sum_sq"] == sb["sum_sq"]
        assert abs(sa["sum_clnc"] - sb["sum_clnc"]) <= 2 * am.clnc_bound(len(counts), sa["sum_clnc"])


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("alphabet,k,kind", [(NT, 7, am.KINDS[2]), (NT, 32, am.KINDS[5]), (AA, 13, am.KINDS[4])],
                         ids=["dense", "one-word", "two-word"])
def test_the_written_table_is_what_the_reference_prints(tmp_path, alphabet, k, kind):
    counts = am.table(kind, 5000, random.Random(k))
    assert not am.dominance_is_exact_tie(counts)
    want = alpha_ref.alpha_table(counts)
    with native.Counter(k, alphabet) as ctx:
        _load(ctx, _packed_keys(alphabet, k, 4900), counts[:4900])
        _load(ctx, _text_keys(alphabet, k, 100), counts[4900:])
        _check(ctx, counts)
        assert diversity.compute_alpha_diversity("s", ctx, tmp_path / "alpha.tsv") == want
    assert (tmp_path / "alpha.tsv").read_text() == "Metric\ts\n" + "".join("%s\t%s\n" % (m, want[m]) for m in alpha_ref.METRICS)
