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
