"""The per-chunk LDS count kernels at the last split level.

Every kernel below counts a bucket in an LDS table and splits a sub-range whose probe chain grows too long on further
hash bits.  The key sets here are solved (oracle/packed_ref.py) to share the bucket, the home slot and EVERY split bit of
one kernel, so no split can shorten their chain: before the fix such a chunk was refused with MK_ERR_RANGE.  Each test
checks that the deepest level ran (stats()["split_exhausted"]) and that the table is exactly the oracle's:

  mk_part_count_k        protein 6 <= k <= 12       mk_part.hip
  mk_sk_count_k          nucleotide 12 <= k <= 32   mk_skcount.hip (FCAP > 0: a sample's later chunks, fused upsert)
  mk_sk2_count_k         nucleotide 33 <= k <= 64   mk_skmer2.hip
  mk_sk2_countp_k        the pre-filter (MK_FORCE_PREFILTER): keys that share all of sk2p_hash; counted again exactly

and past the table's capacity (more distinct keys in one sub-range than the table has slots) the chunk is refused
cleanly: a non-fused context is left as it was, a fused one refuses everything but mk_reset."""
import functools

import numpy as np
import pytest

from mercat2_amd import native
from oracle import cpu_ref
from oracle import packed_ref as pr

pytestmark = pytest.mark.gpu

AA20 = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


@functools.lru_cache(maxsize=None)
def nt_background(seed: int) -> bytes:
    return native.synth_reads(20_000, seed, 2_000, 150, seed + 1).tobytes()


@functools.lru_cache(maxsize=None)
def aa_background(seed: int) -> bytes:
    """Protein records of a small proteome read over several times (counts >= 2 exist), '*'-terminated as in .faa."""
    rng = np.random.default_rng(seed)
    prot = AA20[rng.integers(0, 20, 8_000)]
    out = []
    for i in range(1_200):
        a = int(rng.integers(0, prot.size - 120))
        out.append(b">bg%d\n%s*\n" % (i, prot[a:a + 120].tobytes()))
    return b"".join(out)


def reps_for(n: int) -> list:
    return [1 + (i % 4) for i in range(n)]  # (-c 3 keeps every other key)


def want_arrays(texts, k: int, c: int):
    tables = [cpu_ref.count_text(t, k, c) for t in texts]
    merged = cpu_ref.merge_counts(tables)
    keys = sorted(merged)
    kmers = np.frombuffer("".join(keys).encode(), np.uint8).reshape(len(keys), k) if keys else np.zeros((0, k), np.uint8)
    return kmers, np.array([merged[x] for x in keys], dtype=np.uint64)


def run_sample(texts, k: int, c: int, alphabet=native.ALPHABET_NT2):
    with native.Counter(k, alphabet, device=0) as ctx:
        for t in texts:
            ctx.count_chunk(t, c)
        kmers, counts = ctx.export()
        st = ctx.stats()
    return kmers, counts, st


def check(texts, k: int, c: int, alphabet=native.ALPHABET_NT2, fused_expected: bool = False):
    kmers, counts, st = run_sample(texts, k, c, alphabet)
    want_k, want_c = want_arrays(texts, k, c)
    assert st["split_exhausted"] > 0, "the last split level was not reached: the restated hash is off"
    assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)
    if fused_expected:
        assert st["fused_chunks"] >= 1, "the hostile chunk was not counted by the fused kernel"
    return st


def samples(hostile: bytes, background: bytes):
    """The hostile set as a sample's only chunk, and as the second chunk of a sample (fused launch when c >= 2)."""
    return {"one": [hostile], "second": [background, hostile]}


# ----------------------------------------------------------------------------------- mk_skcount.hip, 12 <= k <= 32
@functools.lru_cache(maxsize=None)
def skc_text(k: int, n: int) -> bytes:
    keys = pr.skc_hostile(k, n)
    assert keys.size >= min(n, 2000)
    bg = nt_background(10 + k)
    if k == 32:
        bg += b">allT\n" + b"T" * 40 + b"\n"  # (the all-T 32-mer equals the free-slot mark: counted aside)
    return pr.hostile_fasta(pr.decode64(keys, k), reps_for(keys.size), bg)


@pytest.mark.parametrize("k", [31, 32])
@pytest.mark.parametrize("n", [60, 3_000])  # just over the 48-probe limit, and (k = 31) all the solver finds: ~2 000
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("where", ["one", "second"])
def test_skcount_last_split_level(k, n, c, where):
    texts = samples(skc_text(k, n), nt_background(10 + k))[where]
    check(texts, k, c, fused_expected=(where == "second" and c >= 2))


# ----------------------------------------------------------------------------------- mk_skmer2.hip, 33 <= k <= 64
@functools.lru_cache(maxsize=None)
def sk2c_text(k: int, n: int) -> bytes:
    hi, lo = pr.sk2c_hostile(k, n)
    return pr.hostile_fasta(pr.decode128(hi, lo, k), reps_for(hi.size), nt_background(20 + k))


@pytest.mark.parametrize("k", [33, 64])
@pytest.mark.parametrize("n", [70, 1 << 20])  # just over the 64-probe limit, and all the solver finds (~1 000)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("where", ["one", "second"])
def test_sk2_count_last_split_level(k, n, c, where):
    texts = samples(sk2c_text(k, n), nt_background(20 + k))[where]
    check(texts, k, c)


@pytest.mark.parametrize("where", ["one", "second"])
def test_sk2_prefilter_unsplittable_bucket_is_counted_exactly(monkeypatch, where):
    """More than the pre-filter table's 2 048 slots of keys with one sk2p_hash value: its split cannot part them, and
    the chunk is counted again by the exact kernel instead of being refused."""
    k = 48
    hi, lo = pr.sk2p_hostile(k, 2_500)
    hostile = pr.hostile_fasta(pr.decode128(hi, lo, k), [2 + (i % 2) for i in range(hi.size)], nt_background(77))
    monkeypatch.setenv("MK_FORCE_PREFILTER", "1")
    check(samples(hostile, nt_background(77))[where], k, 2)


# ----------------------------------------------------------------------------------- mk_part.hip, protein k <= 12
@functools.lru_cache(maxsize=None)
def part_text(k: int, n: int) -> bytes:
    keys = pr.part_hostile(k, n)
    assert keys.size > 48
    return pr.hostile_fasta(pr.decode64(keys, k, bits=5), reps_for(keys.size), aa_background(5))


@pytest.mark.parametrize("n", [49, 1 << 20])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("where", ["one", "second"])
def test_part_count_last_split_level(n, c, where):
    texts = samples(part_text(12, n), aa_background(5))[where]
    check(texts, 12, c, alphabet=native.ALPHABET_AA5)


# ------------------------------------------------------------------------------------ past the table's capacity
def test_part_over_capacity_is_refused_and_the_context_stays_usable():
    """9 000 protein keys in one sub-range of mk_part_count_k (more than its 8 192 slots): refused, nothing of the chunk
    is in the table, and the context counts on."""
    keys = pr.part_hostile(12, 9_000, same_home=False)
    assert keys.size == 9_000
    hostile = pr.hostile_fasta(pr.decode64(keys, 12, bits=5), [1] * keys.size)
    bg = aa_background(6)
    with native.Counter(12, native.ALPHABET_AA5, device=0) as ctx:
        ctx.count_chunk(bg, 1)
        with pytest.raises(native.MercatHipError) as e:
            ctx.count_chunk(hostile, 1)
        assert e.value.code == -7  # MK_ERR_RANGE
        assert ctx.stats()["split_exhausted"] > 0
        kmers, counts = ctx.export()
        ctx.count_chunk(bg, 1)
        kmers2, counts2 = ctx.export()
    want_k, want_c = want_arrays([bg], 12, 1)
    assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)
    assert np.array_equal(kmers2, want_k) and np.array_equal(counts2, 2 * want_c)


def test_skcount_over_capacity_fused_refuses_until_reset():
    """9 000 31-mers in one sub-range of the one-word count kernel, as a sample's second chunk at -c 2 (fused: the
    survivors of its other sub-ranges are already in the running table when the chunk is refused).  The context then
    refuses every call until mk_reset; after it the same context counts exactly."""
    k = 31
    keys = pr.skc_hostile(k, 9_000, same_home=False)
    assert keys.size == 9_000
    bg = nt_background(99)
    hostile = pr.hostile_fasta(pr.decode64(keys, k), [2] * keys.size, bg)
    with native.Counter(k, native.ALPHABET_NT2, device=0) as ctx:
        ctx.count_chunk(bg, 2)
        with pytest.raises(native.MercatHipError) as e:
            ctx.count_chunk(hostile, 2)
        assert e.value.code == -7  # MK_ERR_RANGE
        assert ctx.stats()["split_exhausted"] > 0
        for call in (ctx.export, ctx.rows, lambda: ctx.count_chunk(bg, 2)):
            with pytest.raises(native.MercatHipError) as e:
                call()
            assert e.value.code == -4  # MK_ERR_STATE
        ctx.reset()
        ctx.count_chunk(bg, 2)
        ctx.count_chunk(bg, 2)
        kmers, counts = ctx.export()
    want_k, want_c = want_arrays([bg, bg], k, 2)
    assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)
