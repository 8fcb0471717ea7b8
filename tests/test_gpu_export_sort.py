"""The sorted export of one-word tables (mk_binsort.hip: rows binned by key prefix, the bins sorted in LDS) where a
partition sort breaks: row counts around every planning threshold, key widths close to the bin bits, protein codes
that leave bins empty, keys with bit 63 set, the key kept beside the table, a bin at and over the capacity of one
workgroup (the route back to the library sort), counts past 2^32, slots emptied by filter_min, a shared table, a
canonical context.

Tables are built with import_pairs_device from chosen keys and read back with export_pairs_device and export(); the
expected rows are numpy's sort of the same pairs (uint64).  Every case is read a second time with MK_EXPORT_LIBSORT=1
(the library path everywhere) and must be byte-equal."""

import numpy as np
import pytest

from mercat2_amd import native
from oracle import packed_ref as pr

pytestmark = pytest.mark.gpu

U64 = np.uint64
NT, AA = native.ALPHABET_NT2, native.ALPHABET_AA5
# mk_binsort.hip: B grows while (rows >> B) > MEAN_MAX, up to MAX_BITS and the key's bits; a bin of up to SMALL rows is
# sorted by the common kernel, up to CAP by the large one, beyond that the export is taken again by the library sort
MEAN_MAX, MAX_BITS, SMALL, CAP = 724, 14, 2048, 8192


def _torch():
    import torch
    return torch


def dev(a: np.ndarray):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).to("cuda:0")


def table(k, alphabet, keys, counts, canonical=False):
    ctx = native.Counter(k, alphabet, device=0, canonical=canonical)
    if counts.size:
        dk, dc = dev(keys), dev(counts)
        _torch().cuda.synchronize()
        ctx.import_pairs_device(dk.data_ptr(), dc.data_ptr(), counts.size)
    assert ctx.stats()["mode_name"] == "hash64"
    return ctx


def read_both(ctx):
    """(keys, counts) from export_pairs_device and (text, counts) from export()."""
    torch = _torch()
    n = ctx.rows()
    dk = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    dc = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.export_pairs_device(dk.data_ptr(), dc.data_ptr(), n + 1) == n
    torch.cuda.synchronize()
    assert int(dk[n]) == -7 and int(dc[n]) == -7, "the export wrote past its rows"
    text, counts = ctx.export()
    return dk[:n].cpu().numpy().view(U64), dc[:n].cpu().numpy().view(U64), text, counts


def check(ctx, k, bits, keys, counts, monkeypatch):
    """ctx holds the distinct (keys, counts): both exports give them in unsigned key order, by either path."""
    order = np.argsort(keys, kind="stable")
    want_k, want_c = keys[order], counts[order]
    monkeypatch.delenv("MK_EXPORT_LIBSORT", raising=False)
    got = read_both(ctx)
    monkeypatch.setenv("MK_EXPORT_LIBSORT", "1")
    lib = read_both(ctx)
    monkeypatch.delenv("MK_EXPORT_LIBSORT")
    assert got[0].size == want_k.size
    assert np.array_equal(got[0], want_k) and np.array_equal(got[1], want_c)
    assert np.array_equal(got[3], want_c)
    # (the text of every row up to 300 000 rows; of larger tables both ends and one row in 97: the decoder is the host's)
    pick = np.arange(want_k.size) if want_k.size <= 300_000 else np.unique(
        np.concatenate([np.arange(1000), np.arange(0, want_k.size, 97), np.arange(want_k.size - 1000, want_k.size)]))
    assert np.array_equal(got[2][pick], pr.decode64(want_k[pick], k, bits))
    for a, b in zip(got, lib):
        assert a.tobytes() == b.tobytes()


def nt_keys(rng, k, n):
    """n distinct random k-mer keys below the all-ones key, in random order."""
    top = (1 << (2 * k)) - 1 if k < 32 else (1 << 64) - 1
    keys = np.unique(rng.integers(0, top, size=n + n // 4 + 64, dtype=U64))
    assert keys.size >= n
    return rng.permutation(keys)[:n]


def aa_keys(rng, k, n):
    """n distinct protein keys: k letter codes 0..25 of 5 bits (codes 26..31 never occur: bins stay empty)."""
    n = min(n, 26 ** k)
    v = rng.choice(26 ** k, size=n, replace=False).astype(U64) if 26 ** k < 1 << 22 else np.unique(
        rng.integers(0, 26 ** k, size=n + n // 4 + 64, dtype=np.int64)).astype(U64)
    v = rng.permutation(v)[:n]
    assert v.size == n
    key = np.zeros(n, U64)
    for j in range(k):
        key |= (v % U64(26)) << U64(5 * j)
        v = v // U64(26)
    return key


def small_counts(rng, n):
    return rng.integers(1, 1000, size=n, dtype=U64)


# B changes from b to b + 1 between these two row counts
THRESHOLDS = [((MEAN_MAX + 1) << b) - d for b in range(MAX_BITS) for d in (1, 0)]


@pytest.mark.parametrize("rows", [0, 1, 2, 63, 64, 65] + THRESHOLDS)
def test_row_counts_and_planning_thresholds(rows, monkeypatch):
    rng = np.random.default_rng(rows + 1)
    keys = nt_keys(rng, 31, rows)
    counts = small_counts(rng, rows)
    with table(31, NT, keys, counts) as ctx:
        check(ctx, 31, 2, keys, counts, monkeypatch)


@pytest.mark.parametrize("name,k,alphabet", [("nt31", 31, NT), ("nt12", 12, NT), ("aa4", 4, AA), ("aa12", 12, AA)])
def test_key_widths(name, k, alphabet, monkeypatch):
    """200 000 random keys: several bins, some of them empty, at key widths from 20 to 62 bits.  (nt31: the first and the
    last bin are made to hold a row.)"""
    rng = np.random.default_rng(k)
    keys = nt_keys(rng, k, 200_000) if alphabet == NT else aa_keys(rng, k, 200_000)
    if name == "nt31":
        keys = np.unique(np.concatenate([keys, np.array([0, 5, (1 << 62) - 1, (1 << 62) - 9], U64)]))
        # bins left empty on purpose: no key with 0b0101 on top
        keys = rng.permutation(keys[(keys >> U64(58)) != U64(5)])
    counts = small_counts(rng, keys.size)
    with table(k, alphabet, keys, counts) as ctx:
        check(ctx, k, 2 if alphabet == NT else 5, keys, counts, monkeypatch)


def test_full_width_keys_and_the_side_key(monkeypatch):
    """k = 32: keys with bit 63 set and clear (an unsigned compare), and 32 x 'T' -- the all-ones key, kept beside the
    table -- last with its count."""
    rng = np.random.default_rng(32)
    keys = nt_keys(rng, 32, 50_000)
    assert 0 < int((keys >> U64(63)).sum()) < keys.size
    keys = np.concatenate([keys[:1000], np.array([(1 << 64) - 1], U64), keys[1000:]])
    counts = small_counts(rng, keys.size)
    with table(32, NT, keys, counts) as ctx:
        check(ctx, 32, 2, keys, counts, monkeypatch)
        text, got = ctx.export()
        assert bytes(text[-1]) == b"T" * 32 and got[-1] == counts[1000]


@pytest.mark.parametrize("crowd", [SMALL, SMALL + 1, CAP - 1, CAP, CAP + 1])
def test_keys_crowded_under_one_prefix(crowd, monkeypatch):
    """`crowd` keys that share their top 14 bits beside a few thousand others: the bin at the capacity of each sort
    kernel, one row under and one row over -- over CAP the export goes back to the library sort."""
    rng = np.random.default_rng(crowd)
    prefix = U64(0x2ABC) << U64(62 - 14)
    low = np.unique(rng.integers(0, 1 << 48, size=crowd + 64, dtype=U64))[:crowd]
    others = nt_keys(rng, 31, 5000)
    others = others[(others >> U64(61)) == U64(0)]  # (the crowd's bin holds the crowd alone, whatever B is)
    keys = rng.permutation(np.concatenate([prefix | low, others]))
    counts = small_counts(rng, keys.size)
    with table(31, NT, keys, counts) as ctx:
        check(ctx, 31, 2, keys, counts, monkeypatch)


def test_counts_past_32_bits(monkeypatch):
    rng = np.random.default_rng(7)
    keys = nt_keys(rng, 31, 3000)
    counts = rng.integers(1 << 32, 1 << 63, size=keys.size, dtype=U64)
    counts[::3] = small_counts(rng, counts[::3].size)
    with table(31, NT, keys, counts) as ctx:
        check(ctx, 31, 2, keys, counts, monkeypatch)


def test_slots_emptied_by_filter_min(monkeypatch):
    """After filter_min the table may hold keyed slots of count 0: the export skips them."""
    rng = np.random.default_rng(8)
    keys = nt_keys(rng, 31, 30_000)
    counts = rng.integers(1, 10, size=keys.size, dtype=U64)
    with table(31, NT, keys, counts) as ctx:
        ctx.filter_min(5)
        keep = counts >= U64(5)
        assert 0 < keep.sum() < keys.size
        check(ctx, 31, 2, keys[keep], counts[keep], monkeypatch)


def test_shared_table_exported_by_its_owner(monkeypatch):
    """An owner's table that another context's count kernels upsert into (mk_share_table): the owner's export and the
    sharer's, summed, are the sample; each is in key order by either path."""
    k, c = 31, 1
    texts = [native.synth_reads(20_000, 40 + i, 8_000, 150, 50 + i, 0, i * 8_000).tobytes() for i in range(3)]
    ref_keys, ref_counts = pr.count_sample(texts, k, c)
    owner, sharer = native.Counter(k, NT, device=0), native.Counter(k, NT, device=0)
    try:
        sharer.share_table(owner)
        owner.count_chunk(texts[0], c)
        sharer.count_chunk(texts[1], c)
        sharer.count_chunk(texts[2], c)
        parts = []
        for ctx in (owner, sharer):
            monkeypatch.delenv("MK_EXPORT_LIBSORT", raising=False)
            got = read_both(ctx)
            monkeypatch.setenv("MK_EXPORT_LIBSORT", "1")
            lib = read_both(ctx)
            monkeypatch.delenv("MK_EXPORT_LIBSORT")
            assert got[0].size == ctx.rows() and (got[0].size < 2 or (got[0][1:] > got[0][:-1]).all())
            for a, b in zip(got, lib):
                assert a.tobytes() == b.tobytes()
            assert np.array_equal(got[2], pr.decode64(got[0], k)) and np.array_equal(got[3], got[1])
            parts.append(([got[0]], got[1]))
        keys, counts = pr.merge_tables(parts)
        assert np.array_equal(keys[0], ref_keys[0]) and np.array_equal(counts, ref_counts)
    finally:
        sharer.share_table(None)
        owner.close()
        sharer.close()


def test_canonical_context(monkeypatch):
    """A canonical context counts min(k-mer, reverse complement): its keys crowd the low end of the key space."""
    k, c = 31, 1
    text = native.synth_reads(30_000, 61, 6_000, 150, 62).tobytes()
    keys, counts = pr.count_chunk(text, k, c, canonical=True)
    with native.Counter(k, NT, device=0, canonical=True) as ctx:
        ctx.count_chunk(text, c)
        check(ctx, k, 2, keys[0], counts, monkeypatch)
