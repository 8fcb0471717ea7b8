"""The numpy helpers the running-table tests stand on (oracle/packed_ref.py), checked on the CPU: mk_mix64 and its
inverse, the home slot of two-word keys, and the packed k-mer counter against the C oracle."""
import numpy as np
import pytest

from oracle import c_oracle, cpu_ref, packed_ref as pr

M64 = (1 << 64) - 1


def _mix_int(x: int) -> int:
    """mk_mix64 (mercat2_amd/csrc/mk_common.h) in Python integers."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


# values of the C definition; 0x9E37...: the splitmix64 finaliser's well-known first output for seed 0
KNOWN = [(0x0, 0x0), (0x1, 0x5692161D100B05E5), (0x2, 0xDBD238973A2B148A), (M64, 0xB4D055FCF2CBBD7B),
         (0x9E3779B97F4A7C15, 0xE220A8397B1DCDAF), (0x0123456789ABCDEF, 0xB2C058E4EBB5112C)]


def test_mix64_known_values_and_inverse():
    xs = np.array([a for a, _ in KNOWN], dtype=np.uint64)
    ys = np.array([b for _, b in KNOWN], dtype=np.uint64)
    assert np.array_equal(pr.mix64(xs), ys)
    assert np.array_equal(pr.unmix64(ys), xs)
    assert all(_mix_int(a) == b for a, b in KNOWN)


def test_mix64_round_trip_on_random_words():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 64, size=200_000, dtype=np.uint64, endpoint=False)
    x[:4] = [0, 1, M64, 1 << 63]
    y = pr.mix64(x)
    assert np.array_equal(pr.unmix64(y), x)
    assert np.array_equal(pr.mix64(pr.unmix64(x)), x)
    assert [int(v) for v in y[:64]] == [_mix_int(int(v)) for v in x[:64]]


def test_collision_keys_share_a_home_slot():
    """What the GPU tests build: one-word keys whose mix shares the low 32 bits (one home slot in every table of up to
    2^32 slots), and two-word keys solved for a chosen home."""
    rng = np.random.default_rng(6)
    want = np.uint64(0xFFFFFFFF)
    top = rng.integers(0, 1 << 32, size=1000, dtype=np.uint64) << np.uint64(32)
    keys = pr.unmix64(top | want)
    assert np.unique(keys).size == 1000
    for mask in (1023, (1 << 20) - 1, (1 << 32) - 1):
        assert np.all((pr.mix64(keys) & np.uint64(mask)) == np.uint64(mask))
    lo = rng.integers(0, 1 << 64, size=500, dtype=np.uint64, endpoint=False)
    hi = pr.hi_for_mix(lo, top[:500] | want)
    for mask in (1023, (1 << 26) - 1):
        assert np.all(pr.home128(hi, lo, mask) == np.uint64(mask))
    # the same against home128 written in Python integers
    for h, l_ in zip(hi[:20].tolist(), lo[:20].tolist()):
        assert _mix_int(h ^ _mix_int((l_ + pr.POLY_B) & M64)) & 0xFFFFFFFF == 0xFFFFFFFF


def test_reduce_rows_sums_and_drops_zero():
    w = [np.array([5, 1, 5, 3, 1, 9], np.uint64), np.array([0, 2, 0, 1, 2, 7], np.uint64)]
    keys, cnt = pr.reduce_rows(w, np.array([1, 2, 3, 0, 4, 0], np.uint64))
    assert [k.tolist() for k in keys] == [[1, 5], [2, 0]] and cnt.tolist() == [6, 4]
    keys, cnt = pr.reduce_rows(w[:1], np.array([1, 2, 3, 0, 4, 0], np.uint64))
    assert keys[0].tolist() == [1, 5] and cnt.tolist() == [6, 4]


@pytest.mark.parametrize("words", [1, 2])
def test_unique_counts_is_reduce_rows_with_ones(words):
    rng = np.random.default_rng(8 + words)
    # few distinct first words, so that runs of equal first words hold several second words
    w = [rng.integers(0, 50, size=20_000, dtype=np.uint64) << np.uint64(40)]
    if words == 2:
        w.append(rng.integers(0, 1 << 64, size=20_000, dtype=np.uint64) % np.uint64(300) * np.uint64(0x9E3779B97F4A7C15))
    k1, c1 = pr.unique_counts(w)
    k2, c2 = pr.reduce_rows(w, np.ones(20_000, np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(k1, k2)) and np.array_equal(c1, c2)
    assert pr.unique_counts([x[:0] for x in w])[1].size == 0


def test_counter_refuses_other_text():
    with pytest.raises(AssertionError):
        pr.read_codes(b">a\nACGT\n>b\nACG\n")
    with pytest.raises(AssertionError):
        pr.read_codes(b">a\nACGN\n")
    with pytest.raises(AssertionError):
        pr.read_codes(b">a\nACGT\nACGT\n")


def _synth(genome, gseed, reads, L, rseed, sub=0, first=0) -> bytes:
    """native.synth_reads (a host function of the library: no GPU needed)."""
    from mercat2_amd import native
    return native.synth_reads(genome, gseed, reads, L, rseed, sub, first).tobytes()


@pytest.mark.parametrize("k", [5, 31, 32, 33, 63, 64])
def test_packed_counter_equals_c_oracle(k):
    chunks = [_synth(3_000, 1, 400, 90, 2), _synth(3_000, 1, 300, 90, 3, 20_000, 400), _synth(50_000, 7, 500, 90, 4)]
    for c in (1, 2):
        want = cpu_ref.merge_counts([c_oracle.count_dict(t, k, c) for t in chunks])
        keys, counts = pr.count_sample(chunks, k, c)
        text = pr.as_text(keys, k)
        got = dict(zip((r.tobytes().decode() for r in text), counts.tolist()))
        assert got == want, (k, c)
        assert list(got) == sorted(got)  # key order is text order


@pytest.mark.parametrize("k", [31, 63])
def test_one_reduction_at_c1_is_the_chunked_sum(k):
    chunks = [_synth(5_000, 21, 600, 150, 22, 10_000), _synth(5_000, 21, 700, 150, 23, 10_000, 600)]
    a_k, a_c = pr.count_sample_c1(chunks, k)
    b_k, b_c = pr.count_sample(chunks, k, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a_k, b_k)) and np.array_equal(a_c, b_c)


@pytest.mark.parametrize("k", [5, 31, 32, 33, 63, 64])
def test_packed_counter_canonical_is_the_folded_oracle(k):
    chunks = [_synth(3_000, 11, 400, 80, 12), _synth(40_000, 13, 500, 80, 14, 10_000)]
    for c in (1, 2):
        want = cpu_ref.merge_counts([{key: n for key, n in cpu_ref.canonical_fold(c_oracle.count_dict(t, k, 0)).items() if n >= c}
                                     for t in chunks])
        keys, counts = pr.count_sample(chunks, k, c, canonical=True)
        got = dict(zip((r.tobytes().decode() for r in pr.as_text(keys, k)), counts.tolist()))
        assert got == want, (k, c)


# ------------------------------------------------------------------------- hostile keys for the per-chunk LDS tables
def test_m_star_has_minimizer_order_zero():
    assert int(pr.sk_order_raw(pr.M_STAR)) & ((1 << 22) - 1) == 0
    orders = pr.sk_order_raw(np.arange(1 << 22, dtype=np.uint64)) & np.uint64((1 << 22) - 1)
    assert np.unique(orders).size == 1 << 22  # a bijection on 11-mers: M_STAR is the only minimizer of order 0


def test_umul24_takes_the_low_24_bits_of_each_operand():
    a, b = 0xAB123456, 0xCD654321
    assert int(pr.umul24(a, b)) == ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & 0xFFFFFFFF


def _mmer_at(keys, k, q):
    return (np.asarray(keys, np.uint64) >> np.uint64(2 * (k - pr.SK_M - q))) & np.uint64((1 << 22) - 1)


@pytest.mark.parametrize("k", [31, 32])
def test_skc_hostile_keys_share_bucket_home_and_every_split_bit(k):
    keys = pr.skc_hostile(k, 300)
    assert keys.size == 300 and np.unique(keys).size == 300
    assert np.all(keys < np.uint64(1 << (2 * k)) if k < 32 else True)
    assert np.all(_mmer_at(keys, k, 0) == np.uint64(pr.M_STAR))  # the window's minimizer, so one bucket at any p1
    for p1_log2 in (8, 13):
        assert np.unique(pr.sk_bucket(_mmer_at(keys, k, 0), p1_log2)).size == 1
    h = pr.skc_hash(keys)
    assert np.unique(pr.skc_home(h)).size == 1 and np.unique(h & np.uint64(0xFFFF)).size == 1


def test_skc_hostile_largest_set_at_k31_is_over_two_thousand():
    keys = pr.skc_hostile(31, 1 << 20)
    assert keys.size > 2_000 and np.unique(keys).size == keys.size
    h = pr.skc_hash(keys)
    assert np.unique(pr.skc_home(h)).size == 1 and np.unique(h & np.uint64(0xFFFF)).size == 1


def test_skc_over_capacity_set_shares_the_sub_range_only():
    keys = pr.skc_hostile(31, 9_000, same_home=False)
    assert keys.size == 9_000 and np.unique(keys).size == 9_000
    assert np.unique(pr.skc_hash(keys) & np.uint64(0xFFFF)).size == 1
    assert np.all(_mmer_at(keys, 31, 0) == np.uint64(pr.M_STAR))


@pytest.mark.parametrize("k", [33, 64])
def test_sk2c_hostile_keys_share_one_hash(k):
    hi, lo = pr.sk2c_hostile(k, 200)
    assert hi.size == 200 and np.unique(hi).size == 200
    assert np.all((hi >> np.uint64(42)) == np.uint64(pr.M_STAR))
    if k < 64:
        assert np.all(lo & np.uint64((1 << (128 - 2 * k)) - 1) == 0)  # unused low bits of lo stay clear
    h = pr.sk2c_hash(hi, lo)
    assert np.unique(h).size == 1 and np.unique(pr.sk2c_home(h)).size == 1
    assert int(pr.sk2c_home(h[0])) < pr.SK2C_SLOTS


def test_sk2p_hostile_keys_share_one_prefilter_hash():
    k = 48
    hi, lo = pr.sk2p_hostile(k, 2_500)
    pairs = set(zip(hi.tolist(), lo.tolist()))
    assert len(pairs) == 2_500
    assert np.all((hi >> np.uint64(42)) == np.uint64(pr.M_STAR))
    assert np.all(lo & np.uint64((1 << (128 - 2 * k)) - 1) == 0)
    assert np.unique(pr.sk2p_hash(hi, lo)).size == 1
    assert np.unique(pr.sk2c_hash(hi, lo)).size > 2_000  # the exact kernel's hash tells them apart


def test_part_hostile_keys_are_protein_kmers_on_one_chain():
    keys = pr.part_hostile(12, 1 << 20)
    assert keys.size > 48 and np.unique(keys).size == keys.size
    assert np.all(keys < np.uint64(1 << 60))
    text = pr.decode64(keys, 12, bits=5)
    assert np.all((text >= ord("A")) & (text <= ord("Z")))
    for p1_log2 in (8, 13):
        b, f, slot = pr.part_hash_fields(keys, p1_log2)
        assert np.unique(b).size == 1 and np.unique(f).size == 1 and np.unique(slot).size == 1


def test_hostile_fasta_counts_are_the_repeats():
    keys = pr.skc_hostile(31, 60)
    rows = pr.decode64(keys, 31)
    text = pr.hostile_fasta(rows, [1 + i % 3 for i in range(60)], b">bg\nACGT\n")
    got = cpu_ref.count_text(text, 31, 1)
    assert got == {rows[i].tobytes().decode(): 1 + i % 3 for i in range(60)}
