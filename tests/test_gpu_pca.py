"""-pca on the GPU: mk_gram / mk_gram_matrix are the exact Python-int X^T X of the merged table for every kind of
table, and the CLI's pca_<type>/pca.tsv and plot_PCA match the reference's committed files."""
import gzip
import json
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

from mercat2_amd import cli, native, pca

import pair_moments as pm

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
PCA = GOLDEN / "pca"


_xtx = pm.xtx  # (tests/pair_moments.py: X^T X in Python ints)


def _check(ctxs, slab_rows=0):
    _, matrix = native.merged_export(ctxs)
    got, rows = native.gram(ctxs, slab_rows=slab_rows)
    assert rows == matrix.shape[0]
    assert got == _xtx(matrix)
    return rows


def _counted(texts, k, alphabet=native.ALPHABET_NT2, c=1, canonical=False):
    out = []
    for t in texts:
        ctx = native.Counter(k, alphabet, device=0, canonical=canonical)
        ctx.count_chunk(t, c)
        out.append(ctx)
    return out


def _close(ctxs):
    for c in ctxs:
        c.close()


def _reads(seed, n=4000, glen=20_000):
    return native.synth_reads(glen, seed, n, 150, seed + 100).tobytes()


def _protein(seed, n=300, length=200):
    rnd = random.Random(seed)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    base = "".join(rnd.choice(aa) for _ in range(length * 4))
    recs = []
    for i in range(n):
        s = rnd.randrange(0, len(base) - length)
        recs.append(">p%d\n%s\n" % (i, base[s:s + length]))
    return "".join(recs).encode()


@pytest.mark.parametrize("k", [31, 63, 5])
def test_gram_nucleotide_one_two_word_and_dense(k):
    ctxs = _counted([_reads(s) for s in (3, 3, 5, 9)], k, c=1 if k != 5 else 2)
    try:
        assert _check(ctxs) > 0
    finally:
        _close(ctxs)


@pytest.mark.parametrize("k", [5, 8])
def test_gram_protein(k):
    ctxs = _counted([_protein(s) for s in (1, 2, 3, 4)], k, native.ALPHABET_AA5)
    try:
        assert _check(ctxs) > 0
    finally:
        _close(ctxs)


@pytest.mark.parametrize("k", [31, 63])
def test_gram_canonical(k):
    ctxs = _counted([_reads(s) for s in (11, 12, 13, 14)], k, canonical=True)
    try:
        _check(ctxs)
    finally:
        _close(ctxs)


def test_gram_by_reference_rows_and_side_key():
    """Lower-case and N windows are kept as text (by reference); 32 x 'T' is the side key of the one-word table."""
    texts = []
    for s in range(4):
        body = _reads(20 + s, n=500).decode().split("\n")
        seqs = [l if i % 3 else l.lower() for i, l in enumerate(body)]
        texts.append(("\n".join(seqs) + "\n>t\n" + "T" * (40 + s) + "NACGTN" * s + "\n").encode())
    ctxs = _counted(texts, 32)
    try:
        assert sum(c.export_exotic()[0].shape[0] for c in ctxs) > 0
        assert any(c.to_dict().get("T" * 32) for c in ctxs)
        _check(ctxs)
        _check(ctxs, slab_rows=97)
    finally:
        _close(ctxs)


def test_gram_raw_alphabet():
    rnd = np.random.default_rng(5)
    ctxs = []
    try:
        for s in range(4):
            keys = sorted({bytes(rnd.integers(33, 127, 7, dtype=np.uint8)) for _ in range(300)} | {b"shared!"})
            kmers = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), 7)
            counts = rnd.integers(1, 1000, len(keys)).astype(np.uint64)
            c = native.Counter(7, native.ALPHABET_RAW, device=0)
            ctxs.append(c)
            c.import_exotic(kmers, counts)
        _check(ctxs)
    finally:
        _close(ctxs)


def test_gram_counts_beyond_32_bits():
    torch = pytest.importorskip("torch")
    rnd = np.random.default_rng(9)
    ctxs = []
    try:
        for s in range(4):
            keys = np.unique(rnd.integers(0, 1 << 20, 120, dtype=np.uint64))
            counts = rnd.integers(1 << 32, 1 << 58, keys.size, dtype=np.uint64)
            counts[::5] = rnd.integers(1, 100, counts[::5].size, dtype=np.uint64)
            dk = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
            dc = torch.from_numpy(counts.view(np.int64)).to("cuda:0")
            c = native.Counter(31, native.ALPHABET_NT2, device=0)
            ctxs.append(c)
            torch.cuda.synchronize()
            c.import_pairs_device(dk.data_ptr(), dc.data_ptr(), keys.size)
        _check(ctxs)
        _check(ctxs, slab_rows=7)
    finally:
        _close(ctxs)


@pytest.mark.parametrize("n", [1, 4, 70])
def test_gram_sample_counts(n):
    rnd = random.Random(n)
    texts = [("".join(">r\n" + "".join(rnd.choice("ACGT") for _ in range(300)) + "\n" for _ in range(3))).encode()
             for _ in range(n)]
    ctxs = _counted(texts, 5)
    try:
        _check(ctxs)
    finally:
        _close(ctxs)


@pytest.mark.parametrize("k", [31, 63])
def test_gram_many_slabs(k):
    ctxs = _counted([_reads(s, n=1500) for s in (31, 32, 33, 34, 35)], k)
    try:
        rows = _check(ctxs, slab_rows=1000)
        assert rows > 10_000
        _check(ctxs, slab_rows=3)
    finally:
        _close(ctxs)


def test_gram_contexts_listed_on_device_list():
    ctxs = [native.Counter(31, native.ALPHABET_NT2, device=d) for d in [0, 0, 0]]
    try:
        for s, c in enumerate(ctxs):
            c.count_chunk(_reads(40 + s, n=800), 1)
        _check(ctxs)
    finally:
        _close(ctxs)


def test_gram_mismatched_k():
    ctxs = _counted([_reads(1, n=100), _reads(2, n=100)], 31) + _counted([_reads(3, n=100)], 21)
    try:
        with pytest.raises(native.MercatHipError) as e:
            native.gram(ctxs)
        assert e.value.code == -1
    finally:
        _close(ctxs)


@pytest.mark.parametrize("rows,n,top", [(1000, 5, 1 << 20), (3001, 17, 1 << 40), (0, 3, 5), (257, 70, 1 << 31)])
def test_gram_matrix_random(rows, n, top):
    m = np.random.default_rng(rows + n).integers(0, top, (rows, n), dtype=np.uint64)
    assert native.gram_matrix(m) == _xtx(m)


def _golden_scores(key):
    names, rows = [], []
    for line in (PCA / f"{key}.tsv").read_text().splitlines()[1:]:
        parts = line.split("\t")
        names.append(parts[0])
        rows.append([float(x) for x in parts[1:]])
    return names, np.array(rows)


def _compare(path, key):
    names, want = _golden_scores(key)
    got_names, got = _golden_scores_from(path)
    assert got_names == names
    tol = 1e-9 * np.max(np.abs(want))
    assert np.max(np.abs(got - want)) <= tol
    assert (np.sign(got) == np.sign(want)).all()


def _golden_scores_from(path):
    lines = Path(path).read_text().splitlines()
    assert lines[0] == "sample\tPC1\tPC2\tPC3"
    names = [l.split("\t")[0] for l in lines[1:]]
    return names, np.array([[float(x) for x in l.split("\t")[1:]] for l in lines[1:]])


@pytest.mark.parametrize("s", [10, 1])
def test_cli_protein_pca_matches_committed(tmp_path, s, capsys):
    d = tmp_path / "in"
    d.mkdir()
    for f in sorted((GOLDEN / "inputs").glob("*_pro.faa.gz")):
        shutil.copy(f, d / f.name)
    out = tmp_path / "out"
    assert cli.main(["-f", str(d), "-k", "5", "-c", "10", "-s", str(s), "-pca", "-o", str(out)]) == 0
    text = capsys.readouterr().out
    assert "\nRunning PCA" in text and "Using Incremental PCA: False" in text
    _compare(out / "pca_protein" / "pca.tsv", f"faa-5genomes_gz-{s}__protein")


@pytest.mark.parametrize("s", [10, 1])
def test_cli_nucleotide_pca_matches_committed(tmp_path, s):
    d = tmp_path / "in"
    d.mkdir()
    for name in ("DJ", "GIC31", "RW1", "RW2", "Rleg"):
        shutil.copy(GOLDEN / "inputs" / f"{name}.fna.gz", d / f"{name}.fna.gz")
    out = tmp_path / "out"
    assert cli.main(["-f", str(d), "-k", "5", "-c", "10", "-s", str(s), "-pca", "-o", str(out)]) == 0
    _compare(out / "pca_Nucleotide" / "pca.tsv", f"fna-5genomes_gz-{s}__Nucleotide")


def test_cli_pca_three_samples_writes_nothing(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    for f in sorted((GOLDEN / "inputs").glob("*_pro.faa.gz"))[:3]:
        shutil.copy(f, d / f.name)
    out = tmp_path / "out"
    assert cli.main(["-f", str(d), "-k", "5", "-c", "10", "-pca", "-o", str(out)]) == 0
    assert not (out / "pca_protein").exists()


def test_plot_PCA_on_prod_tables(tmp_path):
    index = json.loads((PCA / "index.json").read_text())
    with gzip.open(PCA / "tables.json.gz", "rt") as fh:
        samples = json.load(fh)[index["fna-5genomes_gz-10__prod"]]
    tables = {}
    for name, rows in samples.items():  # the committed tsv_prod/<name>_counts.tsv
        tables[name] = tmp_path / f"{name}_counts.tsv"
        tables[name].write_text(f"k-mer\t{name}_Count\n" + "".join(f"{k}\t{c}\n" for k, c in rows))
    from mercat2_amd.report import merge_tsv_T
    combined = tmp_path / "combined_prod_T.tsv"
    merge_tsv_T(tables, combined)
    out = tmp_path / "pca_prod"
    assert pca.plot_PCA(str(combined), str(out)) == (None, None)
    _compare(out / "pca.tsv", "fna-5genomes_gz-10__prod")
