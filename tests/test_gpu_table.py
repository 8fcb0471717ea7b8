"""The running hash table (mk_table.hip upserts, mk_chunk.hip sizing, mk_api.hip growth) against a numpy reduction of the same
packed keys, where hash tables break: growth from empty over many batches, long probe chains on one home slot and
probing that wraps past the last slot, many lanes adding to a few keys at once, the key kept beside the table, rows
of count 0, sums past 2^32, and TSV counts of 1 to 20 digits.

Rows go in through mk_import_pairs_device / mk_import_rows_device from torch tensors in HBM and come back through
export() / write_tsv(); the reference is oracle/packed_ref.reduce_rows (sort, sum per key) over the same words."""
import numpy as np
import pytest

from mercat2_amd import native
from oracle import cpu_ref, packed_ref as pr

pytestmark = pytest.mark.gpu

U64 = np.uint64
M64 = (1 << 64) - 1
NT, AA = native.ALPHABET_NT2, native.ALPHABET_AA5
# (name, k, alphabet, words per key)
ONE_WORD = [("nt31", 31, NT, 1), ("nt32", 32, NT, 1), ("aa10", 10, AA, 1)]
TWO_WORD = [("nt63", 63, NT, 2), ("nt64", 64, NT, 2)]


def _torch():
    import torch
    return torch


def dev(a: np.ndarray):
    """uint64 numpy -> int64 tensor on the GPU (same bits)."""
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).to("cuda:0")


def rand_keys(rng, k: int, alphabet: int, words: int, n: int):
    """n random valid keys: the key words of k-mers (two-word nucleotide keys keep lo's unused low bits zero, as the
    engine packs them; protein keys hold letter codes 0..25)."""
    if words == 2:
        hi = rng.integers(0, 1 << 64, size=n, dtype=U64)
        lo = rng.integers(0, 1 << 64, size=n, dtype=U64) & U64((M64 << (2 * (64 - k))) & M64)
        return [hi, lo]
    if alphabet == AA:
        v = rng.integers(0, 26 ** k, size=n, dtype=np.int64).astype(U64)
        key = np.zeros(n, U64)
        for j in range(k):
            key |= (v % U64(26)) << U64(5 * j)
            v //= U64(26)
        return [key]
    return [rng.integers(0, 1 << (2 * k), size=n, dtype=U64)]


def distinct_keys(rng, k, alphabet, words, n):
    """n distinct random keys, in random order."""
    keys, _ = pr.reduce_rows(rand_keys(rng, k, alphabet, words, n + n // 8 + 16), np.ones(n + n // 8 + 16, U64))
    perm = rng.permutation(keys[0].size)[:n]
    assert perm.size == n
    return [w[perm] for w in keys]


def put(ctx, words, counts, via: str):
    """Import rows into ctx: 'pairs' (mk_import_pairs_device: key words + a count column) or 'rows'
    (mk_import_rows_device: {key word(s), count} interleaved)."""
    n = counts.size
    if n == 0:
        return
    if via == "pairs":
        keys = dev(words[0] if len(words) == 1 else np.stack(words, axis=1).reshape(-1))
        cnts = dev(counts)
        ctx.import_pairs_device(keys.data_ptr(), cnts.data_ptr(), n)
    else:
        rows = dev(np.stack(list(words) + [counts], axis=1).reshape(-1))
        ctx.import_rows_device(rows.data_ptr(), n)
    _torch().cuda.synchronize()


def text_of(k, alphabet, keys):
    if len(keys) == 2:
        return pr.decode128(keys[0], keys[1], k)
    return pr.decode64(keys[0], k, 2 if alphabet == NT else 5)


def check_export(ctx, k, alphabet, keys, counts):
    """The whole export equals the reference rows (keys ascending = text order), and rows() agrees."""
    assert ctx.rows() == counts.size
    got_k, got_c = ctx.export()
    assert got_k.shape == (counts.size, k)
    assert np.array_equal(got_c, counts), "counts differ"
    assert np.array_equal(got_k, text_of(k, alphabet, keys)), "keys differ"


def reference(batches):
    """The sum of every batch so far: np.unique + a sum per key over the concatenated rows."""
    nw = len(batches[0][0])
    return pr.reduce_rows([np.concatenate([b[0][i] for b in batches]) for i in range(nw)], np.concatenate([b[1] for b in batches]))


# ------------------------------------------------------------------------------------------------ growth from empty
@pytest.mark.parametrize("spec", ONE_WORD + TWO_WORD, ids=lambda s: s[0])
def test_growth_from_empty_zipf_batches(spec):
    """Batches of rows with Zipf-distributed repeats inside a batch and across batches, fresh keys doubling from batch to
    batch: the table starts empty and ends 127 times larger than after the first batch (>= 20 M one-word / 10 M
    two-word rows), so it is regrown (rehashed) several times between imports.  rows() after every batch, the whole
    export at the end."""
    name, k, alphabet, words = spec
    rng = np.random.default_rng(sum(map(ord, name)))
    target = 21_000_000 if words == 1 else 10_500_000
    nb = 7
    unit = target // (2 ** nb - 1)
    pool = distinct_keys(rng, k, alphabet, words, unit * (2 ** nb - 1))
    seen = np.zeros(pool[0].size, dtype=bool)
    total = np.zeros(pool[0].size, dtype=U64)
    rows_after = []
    with native.Counter(k, alphabet, device=0) as ctx:
        assert ctx.words_per_key() == words
        at = 0
        for b in range(nb):
            fresh = np.arange(at, at + unit * 2 ** b)
            at += fresh.size
            # repeats: Zipf ranks over the keys seen so far (hot keys come again in every batch) and inside this batch
            zipf = (rng.zipf(1.2, size=fresh.size // 2) - 1) % at
            inner = fresh[rng.integers(0, fresh.size, size=fresh.size // 4)]
            idx = rng.permutation(np.concatenate([fresh, zipf, inner]))
            cnt = rng.integers(1, 1000, size=idx.size, dtype=U64)
            put(ctx, [w[idx] for w in pool], cnt, "pairs" if b % 2 == 0 else "rows")
            seen[idx] = True
            np.add.at(total, idx, cnt)
            rows_after.append(int(seen.sum()))
            assert ctx.rows() == rows_after[-1], (b, ctx.rows(), rows_after[-1])
        assert rows_after[-1] >= (20_000_000 if words == 1 else 10_000_000)
        assert rows_after[-1] >= 64 * rows_after[0]  # (any table sized for the first batch was regrown at least 3 times)
        keys, counts = pr.reduce_rows(pool, total)  # (keys never imported have a sum of 0: no row)
        check_export(ctx, k, alphabet, keys, counts)


def test_dense_bins_take_pairs_in_batches():
    """Dense mode (nucleotide k = 5): bins stored from a device buffer, then batches of pairs -- repeats, rows of count 0,
    sums past 2^32 -- and the bins read back; export and rows() against the reference."""
    torch = _torch()
    k, nbins = 5, 4 ** 5
    rng = np.random.default_rng(3)
    with native.Counter(k, NT, device=0) as ctx:
        assert ctx.stats()["mode_name"] == "dense"
        start = np.zeros(nbins, U64)
        start[rng.integers(0, nbins, size=100)] = rng.integers(1, 50, size=100, dtype=U64)
        ctx.dense_bins_device(dev(start).data_ptr(), nbins, True)
        batches = [([np.arange(nbins, dtype=U64)], start)]
        for b in range(5):
            n = 400_000
            keys = (rng.zipf(1.1, size=n) - 1).astype(U64) % U64(nbins)
            cnt = rng.integers(0, 1 << 20, size=n, dtype=U64)
            cnt[rng.integers(0, n, size=n // 10)] = 0
            if b == 4:
                keys[:3], cnt[:3] = [7, 7, 1023], [1 << 40, 1 << 40, 1 << 33]
            put(ctx, [keys], cnt, "pairs" if b % 2 else "rows")
            batches.append(([keys], cnt))
            rk, rc = reference(batches)
            assert ctx.rows() == rc.size
        check_export(ctx, k, NT, rk, rc)
        back = torch.zeros(nbins, dtype=torch.int64, device="cuda:0")
        ctx.dense_bins_device(back.data_ptr(), nbins, False)
        want = np.zeros(nbins, U64)
        want[rk[0].astype(np.int64)] = rc
        assert np.array_equal(back.cpu().numpy().view(U64), want)


# ------------------------------------------------------------------------------------ one home slot, wrap-around
def _cluster64(rng, low32: int, n: int):
    """n distinct one-word keys whose mk_mix64 ends in the 32 bits low32: one home slot in any table of <= 2^32 slots
    (low32 = 0xFFFFFFFF: the last slot, so the probe sequence wraps to slot 0)."""
    top = np.unique(rng.integers(0, 1 << 32, size=n + 64, dtype=U64))[:n]
    rng.shuffle(top)
    return pr.unmix64((top << U64(32)) | U64(low32))


def test_one_home_slot_and_wrap_around_one_word():
    """k = 32: 3000 keys on the last slot (every probe wraps), 2000 on slot 0 (where the wrapped chain runs on), the
    all-T key (kept beside the table) among them, and random keys around them; three batches through both entry points,
    then a fourth that doubles the table (the chains are rehashed)."""
    k = 32
    rng = np.random.default_rng(11)
    last, first = _cluster64(rng, 0xFFFFFFFF, 3000), _cluster64(rng, 0, 2000)
    assert np.all(pr.mix64(last) & U64(0xFFFFFFFF) == U64(0xFFFFFFFF))
    background = rand_keys(rng, k, NT, 1, 20_000)[0]
    hostile = np.concatenate([last, first, np.array([M64], U64)])
    batches = []
    with native.Counter(k, NT, device=0) as ctx:
        for b, via in enumerate(["pairs", "rows", "pairs", "rows"]):
            extra = background if b < 3 else rand_keys(rng, k, NT, 1, 600_000)[0]
            keys = np.concatenate([hostile, hostile[rng.integers(0, hostile.size, size=4000)], extra, np.full(5, M64, U64)])
            perm = rng.permutation(keys.size)
            keys = keys[perm]
            cnt = rng.integers(1, 1 << 16, size=keys.size, dtype=U64)
            put(ctx, [keys], cnt, via)
            batches.append(([keys], cnt))
            rk, rc = reference(batches)
            assert ctx.rows() == rc.size, b
            check_export(ctx, k, NT, rk, rc)
        assert rk[0][-1] == U64(M64)  # (the all-T key is a row, the last in text order)


@pytest.mark.parametrize("k", [63, 64])
def test_one_home_slot_and_wrap_around_two_words(k):
    """Two-word keys solved through home128: 3000 keys with one lo on the last slot (differing only in hi), 2000 keys
    with distinct lo on slot 0, 1000 keys differing only in lo, 1000 with hi == lo."""
    rng = np.random.default_rng(k)
    lo_mask = U64((M64 << (2 * (64 - k))) & M64)
    top = np.unique(rng.integers(0, 1 << 32, size=6000, dtype=U64))[:5000] << U64(32)
    rng.shuffle(top)
    lo0 = rng.integers(0, 1 << 64, dtype=U64) & lo_mask
    a_lo = np.full(3000, lo0, U64)
    a_hi = pr.hi_for_mix(a_lo, top[:3000] | U64(0xFFFFFFFF))
    b_lo = np.unique(rng.integers(0, 1 << 64, size=2100, dtype=U64) & lo_mask)[:2000]
    b_hi = pr.hi_for_mix(b_lo, top[3000:3000 + b_lo.size])
    for mask in (1023, (1 << 24) - 1):
        assert np.all(pr.home128(a_hi, a_lo, mask) == U64(mask)) and np.all(pr.home128(b_hi, b_lo, mask) == U64(0))
    c_lo = np.unique(rng.integers(0, 1 << 64, size=1000, dtype=U64) & lo_mask)
    c_hi = np.full(c_lo.size, rng.integers(0, 1 << 64, dtype=U64), U64)
    d = np.unique(rng.integers(0, 1 << 64, size=1000, dtype=U64) & lo_mask)
    hi = np.concatenate([a_hi, b_hi, c_hi, d])
    lo = np.concatenate([a_lo, b_lo, c_lo, d])
    batches = []
    with native.Counter(k, NT, device=0) as ctx:
        for b, via in enumerate(["pairs", "rows", "pairs", "rows"]):
            n_extra = 10_000 if b < 3 else 500_000
            eh, el = rand_keys(rng, k, NT, 2, n_extra)
            pick = rng.integers(0, hi.size, size=3000)
            kh = np.concatenate([hi, hi[pick], eh])
            kl = np.concatenate([lo, lo[pick], el])
            perm = rng.permutation(kh.size)
            cnt = rng.integers(1, 1 << 16, size=kh.size, dtype=U64)
            put(ctx, [kh[perm], kl[perm]], cnt, via)
            batches.append(([kh[perm], kl[perm]], cnt))
            rk, rc = reference(batches)
            assert ctx.rows() == rc.size, b
            check_export(ctx, k, NT, rk, rc)


# ------------------------------------------------------------------------------------------------------- hot keys
@pytest.mark.parametrize("spec", [("nt32", 32, NT, 1), ("nt64", 64, NT, 2), ("nt63", 63, NT, 2)], ids=lambda s: s[0])
@pytest.mark.parametrize("via", ["pairs", "rows"])
def test_hot_keys_many_lanes_few_keys(spec, via):
    """16 M rows holding 64 distinct keys in ONE import: lanes on every XCD claim and add to the same slots at once (the
    two-word table's lock word and publish step under heavy contention).  Exactly 64 rows, every count exact."""
    name, k, alphabet, words = spec
    rng = np.random.default_rng(len(name) + len(via))
    keys = distinct_keys(rng, k, alphabet, words, 64)
    if words == 1:
        keys[0][keys[0] == U64(M64)] = U64(5)  # (64 keys of the table itself; the side key has its own tests)
    n = 16 * 1024 * 1024
    idx = rng.integers(0, 64, size=n)
    cnt = rng.integers(1, 1 << 20, size=n, dtype=U64)
    want = np.bincount(idx, weights=cnt.astype(np.float64), minlength=64)  # (sums < 2^53: exact in a double)
    with native.Counter(k, alphabet, device=0) as ctx:
        put(ctx, [w[idx] for w in keys], cnt, via)
        assert ctx.rows() == 64
        rk, rc = pr.reduce_rows(keys, want.astype(U64))
        assert rc.sum() == cnt.sum()
        check_export(ctx, k, alphabet, rk, rc)


# ------------------------------------------------------------------------------------------------------- edge rows
def _digits_counts():
    """One count of every length from 1 to 20 decimal digits (the largest below 2^64 - 1, the two-word table's lock
    word)."""
    out = [10 ** (d - 1) + 7 * d for d in range(1, 21)] + [9, 4_294_967_295, 4_294_967_296, 10 ** 19 - 1, 2 ** 63, M64 - 1]
    assert sorted({len(str(v)) for v in out}) == list(range(1, 21)) and max(out) < M64
    return np.array(out, dtype=U64)


@pytest.mark.parametrize("spec", [("nt32", 32, NT, 1), ("aa10", 10, AA, 1), ("nt63", 63, NT, 2), ("nt64", 64, NT, 2)],
                         ids=lambda s: s[0])
def test_edge_rows_zero_counts_big_sums_and_tsv(spec, tmp_path):
    """Rows of count 0 add nothing and make no row (fresh keys and keys already held); per-key sums past 2^32 up to
    about 2^62 over several batches; the all-T 32-mer in several batches and among colliding keys; write_tsv equal to
    "%s\t%d\n" for counts of 1 to 20 digits.  (Sums stay below 2^64 - 1: for two-word keys that value is MK_LOCK128,
    "slot claimed, key being written", and a count word holding it would make every later probe of the slot wait.)"""
    name, k, alphabet, words = spec
    rng = np.random.default_rng(77 + k)
    base = distinct_keys(rng, k, alphabet, words, 30_000)
    if words == 1 and k == 32:
        base[0][:3000] = _cluster64(rng, 0xFFFFFFFF, 3000)
        base[0][3000] = U64(M64)
        base = [np.unique(base[0])]
        rng.shuffle(base[0])
        at = int(np.flatnonzero(base[0] == U64(M64))[0])  # (the all-T key among the ordinary keys, not a ghost)
        base[0][[at, 2000]] = base[0][[2000, at]]
    n = base[0].size
    big = np.arange(0, 40)               # sums of ~2^60 a batch, four batches: ~2^62
    mid = np.arange(40, 1000)            # sums past 2^32
    ghosts = np.arange(n - 2000, n)      # only ever imported with count 0
    digits = _digits_counts()
    batches = []
    with native.Counter(k, alphabet, device=0) as ctx:
        for b in range(4):
            idx = np.concatenate([np.arange(0, n - 2000), rng.integers(0, n - 2000, size=5000), ghosts])
            cnt = rng.integers(1, 100, size=idx.size, dtype=U64)
            cnt[big] = U64(2 ** 60) - rng.integers(0, 1 << 20, size=big.size, dtype=U64)
            cnt[mid] = U64(2 ** 31) + rng.integers(0, 1 << 30, size=mid.size, dtype=U64)
            cnt[-2000:] = 0
            cnt[rng.integers(1000, n - 2000, size=3000)] = 0  # zeros for keys the table holds
            if words == 1 and k == 32:
                idx = np.concatenate([idx, np.full(3, 2000)])
                cnt = np.concatenate([cnt, np.array([1, 0, 2 ** 40], U64)])
            perm = rng.permutation(idx.size)
            idx, cnt = idx[perm], cnt[perm]
            put(ctx, [w[idx] for w in base], cnt, "pairs" if b % 2 == 0 else "rows")
            batches.append(([w[idx] for w in base], cnt))
            rk, rc = reference(batches)
            assert ctx.rows() == rc.size <= n - 2000, b
        assert int(rc.max()) > 2 ** 61 and int(rc.max()) < 2 ** 63
        check_export(ctx, k, alphabet, rk, rc)
    # counts of every length, each key once (a table of their own)
    keys = [w[:digits.size] for w in distinct_keys(rng, k, alphabet, words, 64)]
    with native.Counter(k, alphabet, device=0) as ctx:
        put(ctx, keys, digits, "pairs")
        rk, rc = pr.reduce_rows(keys, digits)
        check_export(ctx, k, alphabet, rk, rc)
        out = tmp_path / "t.tsv"
        assert ctx.write_tsv(out, "s") == digits.size
        text = text_of(k, alphabet, rk)
        table = {r.tobytes().decode(): int(c) for r, c in zip(text, rc)}
        assert out.read_text() == cpu_ref.tsv_text("s", table)
        assert {len(str(v)) for v in table.values()} == set(range(1, 21))


# --------------------------------------------------------------------------------------- merge_from, filter_min
@pytest.mark.parametrize("spec", [("nt32", 32, NT, 1), ("nt64", 64, NT, 2)], ids=lambda s: s[0])
def test_merge_from_and_filter_min(spec):
    """Two tables with overlapping keys (one-word: the all-T key in both) summed by merge_from, then filter_min, against
    the numpy sum and filter."""
    name, k, alphabet, words = spec
    rng = np.random.default_rng(99)
    pool = distinct_keys(rng, k, alphabet, words, 900_000)
    if words == 1:
        pool[0][0] = U64(M64)
    ia = rng.permutation(pool[0].size)[:600_000]
    ib = rng.permutation(pool[0].size)[:500_000]
    ca = rng.integers(1, 20, size=ia.size, dtype=U64)
    cb = rng.integers(1, 20, size=ib.size, dtype=U64)
    ca[:10] = U64(3 << 40)
    ia[0] = ib[0] = 0  # (one-word: the all-T key is in both tables)
    with native.Counter(k, alphabet, device=0) as a, native.Counter(k, alphabet, device=0) as b:
        put(a, [w[ia] for w in pool], ca, "pairs")
        put(b, [w[ib] for w in pool], cb, "rows")
        a.merge_from(b)
        rk, rc = pr.reduce_rows([np.concatenate([w[ia], w[ib]]) for w in pool], np.concatenate([ca, cb]))
        check_export(a, k, alphabet, rk, rc)
        check_export(b, k, alphabet, *pr.reduce_rows([w[ib] for w in pool], cb))
        for m in (2, 17, 25):
            a.filter_min(m)
            keep = rc >= U64(m)
            rk, rc = [w[keep] for w in rk], rc[keep]
            check_export(a, k, alphabet, rk, rc)
