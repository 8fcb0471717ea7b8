"""mk_gram and mk_pair_stats through tables with chosen keys: the union join (join_union, mk_join.h) where it decides
something -- a slab cap below one key's entries, a union of one key, empty samples, disjoint key ranges, a far
outlier behind clustered keys (deep bisection, empty ranges, the 4096-part first cut), two-word keys that differ in one
word only, the 2^32 flag set and cleared from slab to slab, the side key, by-reference rows, the raw alphabet, dense
tables (and protein k = 4, the first k past them) and a canonical context.

One-word tables are built with import_pairs_device from chosen keys; two-word tables, dense tables and by-reference
rows by counting FASTA (one record of exactly k bases per k-mer, repeated count times).  The expected rows x n matrix is
built here from one dict per sample (the union of the dicts; the statistics do not depend on the order of the rows),
never from merged_export.  Every case runs both entry points at slab_rows 0, 1, 2, 3, 7 and 1000: rows, the integers
(equal to the reference, hence equal across slab_rows), Gram == dot, canb / seuc within the bounds of
tests/pair_moments.py."""
import random

import numpy as np
import pytest

from mercat2_amd import native
from oracle import cpu_ref

import pair_moments as pm

pytestmark = pytest.mark.gpu

NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
SLABS = (0, 1, 2, 3, 7, 1000)


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def imported(tables, k=31):
    """One one-word context per dict {key: count}; an empty dict is a fresh context that counted nothing."""
    ctxs = []
    for t in tables:
        ctx = native.Counter(k, NT, device=0)
        ctxs.append(ctx)
        if t:
            keys, counts = np.array(list(t.keys()), dtype=np.uint64), np.array(list(t.values()), dtype=np.uint64)
            dk, dc = _dev(keys), _dev(counts)
            _torch().cuda.synchronize()
            ctx.import_pairs_device(dk.data_ptr(), dc.data_ptr(), counts.size)
            assert ctx.words_per_key() == 1
        assert ctx.rows() == len(t)
    return ctxs


def fasta(table):
    """One record of exactly k bases per k-mer, count times."""
    return "".join(">r\n%s\n" % key * c for key, c in table.items()).encode()


def counted(texts, k, alphabet=NT, canonical=False, fold=False):
    """(contexts, dicts): every text counted with min_count 1, and the host oracle's table of the same text."""
    ctxs, tables = [], []
    for t in texts:
        ctx = native.Counter(k, alphabet, device=0, canonical=canonical)
        ctxs.append(ctx)
        if t:
            ctx.count_chunk(t, 1)
        want = cpu_ref.count_text(t, k, 1) if t else {}
        tables.append(cpu_ref.canonical_fold(want) if fold else want)
    return ctxs, tables


def close(ctxs):
    for c in ctxs:
        c.close()


def dense_matrix(tables):
    keys = sorted(set().union(*[set(t) for t in tables]))
    row = {key: r for r, key in enumerate(keys)}
    X = np.zeros((len(keys), len(tables)), dtype=np.uint64)
    for s, t in enumerate(tables):
        for key, c in t.items():
            X[row[key], s] = c
    return X


def check(ctxs, tables, slabs=SLABS):
    X = dense_matrix(tables)
    want = pm.exact_ints(X)
    refs = pm.f64_refs(X) if pm.small_counts(X) else (None, None)
    worst = {"canb": 0.0, "seuc": 0.0}
    for slab in slabs:
        got = native.pair_stats(ctxs, slab_rows=slab)
        assert got["rows"] == X.shape[0], slab
        pm.same_ints(got, want)
        gram, rows = native.gram(ctxs, slab_rows=slab)
        assert rows == X.shape[0], slab
        assert gram == want["dot"], slab
        assert gram == got["dot"], slab
        w = pm.check_f64(got, X, want, *refs)
        worst = {key: max(worst[key], w[key]) for key in worst}
    print("join %d x %d: canb %.4f seuc %.4f of the bound" % (X.shape[0], X.shape[1], worst["canb"], worst["seuc"]))
    return want


def run_imported(tables, slabs=SLABS, k=31):
    ctxs = imported(tables, k)
    try:
        return check(ctxs, tables, slabs)
    finally:
        close(ctxs)


def run_counted(texts, k, alphabet=NT, canonical=False, fold=False, slabs=SLABS, words=None, mode=None):
    ctxs, tables = counted(texts, k, alphabet, canonical, fold)
    try:
        for c, t in zip(ctxs, tables):
            assert c.to_dict() == t  # (the premise: the table holds what the dict says)
            if words is not None and t:
                assert c.words_per_key() == words
            if mode is not None and t:
                assert c.stats()["mode_name"] == mode
        return check(ctxs, tables, slabs), ctxs, tables
    finally:
        close(ctxs)


# ------------------------------------------------------------------------------------------ tiny unions
@pytest.mark.parametrize("n", [1, 2, 9])
def test_union_of_one_key(n):
    """kmin = kmax, span 0; at slab_rows 1 and 2 the key's n entries exceed the cap and the range cannot be cut."""
    want = run_imported([{0x1234_5678_9ABC: 3 + 5 * s} for s in range(n)])
    assert want["rows"] == 1 and want["constant_row"] == (n == 1)
    want = run_imported([{0: 7} for _ in range(n)])  # (the lowest key there is; a constant row)
    assert want["rows"] == 1 and want["constant_row"]


@pytest.mark.parametrize("n", [1, 2, 9])
def test_one_key_per_sample_all_distinct(n):
    want = run_imported([{(1 << 61) - 1 - 977 * s * s: 2 + s} for s in range(n)])
    assert want["rows"] == n and all(want["dot"][i][j] == 0 for i in range(n) for j in range(n) if i != j)


def _random_table(rng, rows, key_top=1 << 62, count_top=1000):
    keys = np.unique(rng.integers(0, key_top, rows, dtype=np.uint64))
    return dict(zip(keys.tolist(), rng.integers(1, count_top, keys.size, dtype=np.uint64).tolist()))


@pytest.mark.parametrize("empty", [(0,), (2,), (3,), (0, 1), (0, 1, 3), (1, 2, 3), (0, 1, 2, 3)],
                         ids=["first", "middle", "last", "first two", "all but 2", "all but first", "all"])
def test_empty_samples(empty):
    rng = np.random.default_rng(11)
    shared = _random_table(rng, 40, key_top=1 << 12)
    tables = [{} if s in empty else {**shared, **_random_table(rng, 60, key_top=1 << 12)} for s in range(4)]
    want = run_imported(tables)
    for s in empty:
        assert want["sums"][s] == 0 and want["dot"][s][s] == 0
    if len(empty) == 4:
        assert want["rows"] == 0 and not want["constant_row"]


def test_disjoint_key_ranges():
    """Slabs with entries of one sample only; between the samples' ranges, ranges with no entry at all."""
    rng = np.random.default_rng(12)
    tables = [{(s << 50) + key: c for key, c in _random_table(rng, 50 + 10 * s, key_top=1 << 10).items()} for s in range(5)]
    want = run_imported(tables)
    assert want["rows"] == sum(len(t) for t in tables) and not want["both"][0, 1:].any()


def test_identical_samples():
    rng = np.random.default_rng(13)
    t = _random_table(rng, 300)
    want = run_imported([dict(t) for _ in range(4)])
    assert want["constant_row"] and want["neq"].sum() == 0


# ------------------------------------------------------------------------------------------ clustered keys, one outlier
def _cluster_tables(keys, outlier):
    """Three samples over 5000 consecutive keys and one far key: all of them; every other one and the outlier; a few."""
    rnd = random.Random(14)
    a = {key: rnd.randint(1, 5) for key in keys}
    b = {key: rnd.randint(6, 9) for key in keys[::2]}
    b[outlier] = 4
    c = {key: rnd.randint(10, 14) for key in keys[100:4000:7]}  # (counts apart: no constant row, seuc is compared)
    return [a, b, c]


@pytest.mark.parametrize("slab", SLABS)
def test_clustered_keys_and_one_outlier_one_word(slab):
    """total / cap > 2048 at slab_rows 2 and 3: the first cut is capped at 4096 parts, all but two of them empty, and the
    cluster is bisected from a span of 2^61 down to single keys."""
    base = 0x0000_0ACE_0000
    tables = _cluster_tables([base + i for i in range(5000)], (1 << 61) + 12345)
    assert 2 * sum(len(t) for t in tables) // 3 > 4096
    want = run_imported(tables, slabs=(slab,))
    assert want["rows"] == 5001 and not want["constant_row"]


def _kmer(value, bases):
    return "".join("ACGT"[(value >> (2 * (bases - 1 - i))) & 3] for i in range(bases))


@pytest.mark.parametrize("slab", SLABS)
def test_clustered_keys_and_one_outlier_two_words(slab):
    """The same at k = 40: the cluster shares its first 33 bases (one hi word, consecutive lo words), the outlier differs in
    the first base."""
    head = "ACGGTCAATGCCGTAAGCTTAGGCATCGATCGA"
    assert len(head) == 33
    tables = _cluster_tables([head + _kmer(3000 + i, 7) for i in range(5000)], "T" + head[1:] + "GATTACA")
    want, _, _ = run_counted([fasta(t) for t in tables], 40, slabs=(slab,), words=2)
    assert want["rows"] == 5001 and not want["constant_row"]


# ------------------------------------------------------------------------------------------ two-word keys, one word apart
def test_two_word_keys_that_differ_in_one_word():
    """k = 40: the first 32 bases are the hi word, the last 8 the lo word.  Four families: one suffix of 32 bases under
    different prefixes (hi differs a little, lo equal), one prefix of 32 bases over different suffixes (hi equal), a shared
    prefix of 8 and a shared suffix of 8 with the rest random.  Every family has keys held by some samples only."""
    rnd = random.Random(15)
    word = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    s32, p32, p8, s8 = word(32), word(32), word(8), word(8)
    families = [[word(8) + s32 for _ in range(12)], [p32 + word(8) for _ in range(12)],
                [p8 + word(32) for _ in range(12)], [word(32) + s8 for _ in range(12)]]
    families[0] += [s32[:8] + s32, p32[-8:] + s32]
    families[1] += [p32 + p32[:8], p32 + s32[-8:]]
    tables = [{} for _ in range(5)]
    for fam in families:
        for key in fam:
            held = rnd.sample(range(5), rnd.randint(1, 4))
            for s in held:
                tables[s][key] = rnd.randint(1, 6)
    want, _, _ = run_counted([fasta(t) for t in tables], 40, words=2)
    assert want["rows"] == len(set().union(*tables)) == sum(len(f) for f in families)


# ------------------------------------------------------------------------------------------ the 2^32 flag across slabs
@pytest.mark.parametrize("where", ["lowest keys", "highest keys", "last sample"])
def test_wide_counts_in_some_slabs_only(where):
    """The join clears and sets the flag per slab: a slab of narrow counts after a wide one (and the reverse) must take
    its own product path.  At slab_rows 7 the 400 keys are some 200 slabs."""
    rng = np.random.default_rng(16)
    keys = np.sort(np.unique(rng.integers(0, 1 << 40, 400, dtype=np.uint64))).tolist()
    tables = [{key: int(rng.integers(1, 1 << 32)) for key in keys if rng.random() < 0.7} for _ in range(4)]
    if where == "last sample":
        for key in list(tables[3])[::3]:
            tables[3][key] = int(rng.integers(1 << 32, 1 << 52))
    else:
        part = keys[:25] if where == "lowest keys" else keys[-25:]
        for t in tables:
            for key in part:
                if key in t and rng.random() < 0.6:
                    t[key] = int(rng.integers(1 << 32, 1 << 52))
    for key in keys[100:300:9]:  # (rows of (2^32 - 1)^2 in the narrow slabs: the carries of the 32 x 32 path)
        tables[0][key] = tables[3][key] = (1 << 32) - 1
        tables[1].pop(key, None)  # (and no constant row: seuc is compared)
    want = run_imported(tables)
    assert want["dot"][0][3] >= 1 << 64 and not want["constant_row"]


# ------------------------------------------------------------------------------------------ side key, by-reference rows, raw
def test_side_key_and_by_reference_rows():
    """k = 32: 32 x 'T' is the key kept beside the one-word table, here in samples 0 and 2 only; lower-case and N windows
    are rows kept as text, some shared between samples.  slab_rows 1 sends the host-joined rows one at a time."""
    rnd = random.Random(17)
    genome = "".join(rnd.choice("ACGT") for _ in range(400))
    texts = []
    for s in range(4):
        recs = []
        for i in range(6):
            at = rnd.randrange(0, 330)
            seq = genome[at:at + 70]
            if i % 3 == 1:
                seq = seq.lower() if s % 2 else seq[:40].lower() + seq[40:]
            if i % 3 == 2:
                seq = seq[:35] + "N" + seq[36:]
            recs.append(">r%d\n%s\n" % (i, seq))
        recs.append(">shared\n%sN%s\n" % (genome[:20], genome[21:50]))
        if s in (0, 2):
            recs.append(">t\n%s\n" % ("T" * (33 + s)))
        texts.append("".join(recs).encode())
    want, ctxs, tables = run_counted(texts, 32)
    assert [("T" * 32) in t for t in tables] == [True, False, True, False]
    assert all(any(set(key) - set("ACGT") for key in t) for t in tables)
    assert want["rows"] > 300


def test_raw_alphabet():
    rng = np.random.default_rng(18)
    ctxs, tables = [], []
    try:
        for s in range(4):
            keys = sorted({bytes(rng.integers(33, 127, 7, dtype=np.uint8)) for _ in range(60)} | {b"shared!"} |
                          ({b"in0and2"} if s % 2 == 0 else set()))
            counts = rng.integers(1, 1000, len(keys)).astype(np.uint64)
            c = native.Counter(7, RAW, device=0)
            ctxs.append(c)
            c.import_exotic(np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), 7), counts)
            tables.append(dict(zip(keys, counts.tolist())))
        want = check(ctxs, tables)
        assert want["rows"] == len(set().union(*tables)) and want["both"][0, 2] >= 2
    finally:
        close(ctxs)


# ------------------------------------------------------------------------------------------ dense tables, canonical
@pytest.mark.parametrize("k,alphabet,letters,mode", [(5, NT, "ACGT", "dense"), (3, AA, "ACDEFGHIKLMNPQRSTVWY", "dense"),
                                                     (4, AA, "ACDEFGHIKLMNPQRSTVWY", "hash64")], ids=["nt5", "aa3", "aa4"])
def test_small_k_tables_that_miss_most_bins(k, alphabet, letters, mode):
    """Dense tables (k * bits <= 15: every bin is a row candidate, mk_export_pairs_device gathers the filled ones) whose
    samples fill a handful of bins, one sample none; protein k = 4 is the first k past dense (20 bits, a one-word table)."""
    rnd = random.Random(19 + k)
    shared = "".join(rnd.choice(letters) for _ in range(12))
    texts = [(">a\n%s\n>b\n%s\n" % (shared, "".join(rnd.choice(letters) for _ in range(10 + 3 * s)))).encode() for s in range(5)]
    texts[2] = b""  # (one sample counted nothing)
    want, _, tables = run_counted(texts, k, alphabet, mode=mode)
    assert 0 < want["rows"] < 70 and want["sums"][2] == 0


def test_canonical_context():
    texts = [native.synth_reads(1000, 7, 20, 100, 70 + s).tobytes() for s in range(3)]
    want, _, _ = run_counted(texts, 31, canonical=True, fold=True)
    assert want["rows"] > 500
