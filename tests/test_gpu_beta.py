"""Beta diversity on the GPU: mk_pair_stats / mk_pair_stats_matrix against exact numpy / Python-int statistics for
every kind of table, the committed table sets against tests/golden/beta/expected.json, and the CLI's beta and alpha
report files (lib/mercat2_diversity.py, bin/mercat2.py:351-361, 451-461, 479-499) end to end."""
import gzip
import json
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

from mercat2_amd import cli, diversity, native

import pair_moments as pm

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
EXPECTED = json.loads((GOLDEN / "beta" / "expected.json").read_text())
INDEX = json.loads((GOLDEN / "pca" / "index.json").read_text())
ALPHA = json.loads((GOLDEN / "diversity" / "alpha_cases.json").read_text())
EXACT = {"euclidean", "sqeuclidean", "cityblock", "manhattan", "braycurtis", "chebyshev", "hamming", "matching",
         "jaccard", "dice", "rogerstanimoto", "russellrao", "sokalmichener", "sokalsneath", "yule"}


_close_enough, _exact, _same_ints = pm.close_enough, pm.exact, pm.same_ints  # (tests/pair_moments.py)


def _check(ctxs, slab_rows=0):
    _, matrix = native.merged_export(ctxs)
    got = native.pair_stats(ctxs, slab_rows=slab_rows)
    want = _exact(matrix)
    _same_ints(got, want)
    assert _close_enough(got["canb"], want["canb"])
    if not want["constant_row"]:
        assert _close_enough(got["seuc"], want["seuc"])
    return got


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


# ------------------------------------------------------------------------------------------ the statistics
@pytest.mark.parametrize("k", [5, 21, 31, 63, 70])
def test_pair_stats_nucleotide(k):
    ctxs = _counted([_reads(s, n=1500) for s in (3, 3, 5, 9)], k, c=1 if k != 5 else 2)
    try:
        got = _check(ctxs)
        assert got["rows"] > 0
        assert got["neq"][0, 1] == 0 and got["l1"][0][1] == 0  # (samples 0 and 1 are the same reads)
    finally:
        _close(ctxs)


def test_pair_stats_protein():
    ctxs = _counted([_protein(s) for s in (1, 2, 3, 4)], 5, native.ALPHABET_AA5)
    try:
        _check(ctxs)
    finally:
        _close(ctxs)


@pytest.mark.parametrize("k", [31, 63])
def test_pair_stats_canonical(k):
    ctxs = _counted([_reads(s, n=1500) for s in (11, 12, 13)], k, canonical=True)
    try:
        _check(ctxs)
    finally:
        _close(ctxs)


def test_pair_stats_counts_beyond_32_bits():
    torch = pytest.importorskip("torch")
    rnd = np.random.default_rng(9)
    ctxs = []
    try:
        for s in range(4):
            keys = np.unique(rnd.integers(0, 1 << 12, 300, dtype=np.uint64))
            counts = rnd.integers(1 << 32, 1 << 58, keys.size, dtype=np.uint64)  # (128-bit sums)
            counts[::5] = rnd.integers(1, 100, counts[::5].size, dtype=np.uint64)
            dk = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
            dc = torch.from_numpy(counts.view(np.int64)).to("cuda:0")
            c = native.Counter(31, native.ALPHABET_NT2, device=0)
            ctxs.append(c)
            torch.cuda.synchronize()
            c.import_pairs_device(dk.data_ptr(), dc.data_ptr(), keys.size)
        a = _check(ctxs)
        b = _check(ctxs, slab_rows=7)
        _same_ints(a, b)
    finally:
        _close(ctxs)


@pytest.mark.parametrize("n", [1, 2, 9, 300])
def test_pair_stats_sample_counts(n):
    rnd = random.Random(n)
    texts = [("".join(">r\n" + "".join(rnd.choice("ACGT") for _ in range(300)) + "\n" for _ in range(3))).encode()
             for _ in range(n)]
    ctxs = _counted(texts, 5)
    try:
        _check(ctxs)
    finally:
        _close(ctxs)


@pytest.mark.parametrize("k", [31, 63])
def test_pair_stats_many_slabs(k):
    ctxs = _counted([_reads(s, n=1500) for s in (31, 32, 33, 34, 35)], k)
    try:
        whole = _check(ctxs)
        assert whole["rows"] > 10_000
        for slab in (1000, 3):
            part = _check(ctxs, slab_rows=slab)
            _same_ints(part, whole)
    finally:
        _close(ctxs)


def test_pair_stats_f64_repeatable():
    ctxs = _counted([_reads(s, n=2000) for s in (41, 42, 43, 44, 45, 46)], 31)
    try:
        a = native.pair_stats(ctxs)
        b = native.pair_stats(ctxs)
        assert a["canb"].tobytes() == b["canb"].tobytes()
        assert a["seuc"].tobytes() == b["seuc"].tobytes()
        _same_ints(a, b)
    finally:
        _close(ctxs)


def test_pair_stats_contexts_on_one_device():
    ctxs = [native.Counter(31, native.ALPHABET_NT2, device=d) for d in [0, 0, 0]]
    try:
        for s, c in enumerate(ctxs):
            c.count_chunk(_reads(40 + s, n=800), 1)
        _check(ctxs)
    finally:
        _close(ctxs)


def test_pair_stats_matrix_equals_tables():
    ctxs = _counted([_reads(s, n=1500) for s in (51, 52, 53, 54)], 21)
    try:
        _, matrix = native.merged_export(ctxs)
        a = native.pair_stats(ctxs)
        b = native.pair_stats_matrix(matrix)
        _same_ints(a, b)
        assert _close_enough(a["canb"], b["canb"]) and _close_enough(a["seuc"], b["seuc"])
    finally:
        _close(ctxs)


@pytest.mark.parametrize("rows,n,top", [(1000, 5, 1 << 20), (3001, 17, 1 << 40), (257, 70, 1 << 31), (40, 3, 3)])
def test_pair_stats_matrix_random(rows, n, top):
    m = np.random.default_rng(rows + n).integers(0, top, (rows, n), dtype=np.uint64)
    m[::7, 1] = 0
    got, want = native.pair_stats_matrix(m), _exact(m)
    _same_ints(got, want)
    assert _close_enough(got["canb"], want["canb"])
    if not want["constant_row"]:
        assert _close_enough(got["seuc"], want["seuc"])


def test_pair_stats_mismatched_k():
    ctxs = _counted([_reads(1, n=100), _reads(2, n=100)], 31) + _counted([_reads(3, n=100)], 21)
    try:
        with pytest.raises(native.MercatHipError) as e:
            native.pair_stats(ctxs)
        assert e.value.code == -1
    finally:
        _close(ctxs)


def test_pair_stats_mismatched_alphabet():
    ctxs = _counted([_reads(1, n=100)], 5) + _counted([_protein(2, n=20)], 5, native.ALPHABET_AA5)
    try:
        with pytest.raises(native.MercatHipError) as e:
            native.pair_stats(ctxs)
        assert e.value.code == -1
    finally:
        _close(ctxs)


# ------------------------------------------------------------------------------------------ committed answers
def _union(samples):
    names = sorted(samples)
    keys = sorted({k for rows in samples.values() for k, _ in rows})
    col = {k: i for i, k in enumerate(keys)}
    X = np.zeros((len(names), len(keys)), dtype=np.int64)
    for s, name in enumerate(names):
        for k, c in samples[name]:
            X[s, col[k]] = c
    return names, X


def _compare_matrix(metric, got_rows, want_rows):
    if metric in EXACT:
        assert got_rows == want_rows, metric
    else:
        assert _close_enough([[float(v) for v in r] for r in got_rows], [[float(v) for v in r] for r in want_rows]), metric


def test_committed_sets_through_matrix():
    with gzip.open(GOLDEN / "pca" / "tables.json.gz", "rt") as fh:
        sets = json.load(fh)
    for key, want in EXPECTED.items():
        names, X = _union(sets[key])
        assert names == want["names"] and X.shape[1] == want["rows"]
        got = diversity.beta_from_stats(native.pair_stats_matrix(np.ascontiguousarray(X.T)), lambda: X)
        for metric, w in want["metrics"].items():
            if w == "error":
                assert isinstance(got[metric], str), (key, metric)
            else:
                _compare_matrix(metric, [[repr(float(v)) for v in r] for r in got[metric]], w)


# ------------------------------------------------------------------------------------------ the CLI
def _read_beta(path):
    lines = Path(path).read_text().splitlines()
    head = lines[0].split("\t")
    assert head[0] == ""
    names = head[1:]
    rows = [l.split("\t") for l in lines[1:]]
    assert [r[0] for r in rows] == names
    return names, [r[1:] for r in rows]


def _check_cli(out, beta_dir, label, prefix, set_key, alpha_key, text):
    want = EXPECTED[set_key]
    files = sorted(p.name for p in beta_dir.glob(f"*-{label}.tsv"))
    assert files == sorted(f"{m}-{label}.tsv" for m in diversity.BETA_METRICS if m != "mahalanobis")
    for metric in diversity.BETA_METRICS:
        if metric == "mahalanobis":
            continue
        names, rows = _read_beta(beta_dir / f"{metric}-{label}.tsv")
        assert names == want["names"]
        _compare_matrix(metric, rows, want["metrics"][metric])
    d = want["rows"]
    assert ("Error with beta metric: Mahalanobis\nThe number of observations (5) is too small; the covariance matrix is "
            f"singular. For observations with {d} dimensions, at least {d + 1} observations are required.\n") in text
    div = out / "report" / "diversity"
    merged = (out / "report" / f"diversity-{label}.tsv").read_text().splitlines()
    assert merged[0] == "Metric\t" + "\t".join(want["names"])
    assert [l.split("\t")[0] for l in merged[1:]] == diversity.METRICS
    for s, name in enumerate(want["names"]):
        lines = (div / f"{prefix}-{name}.tsv").read_text().splitlines()
        assert lines[0] == f"Metric\t{name}"
        got = dict(l.split("\t") for l in lines[1:])
        assert got == ALPHA[f"{alpha_key}/{name}"]["expected"], name
        assert [l.split("\t")[s + 1] for l in merged[1:]] == [got[m] for m in diversity.METRICS]


@pytest.mark.parametrize("s", [10, 1])
def test_cli_protein_beta_and_alpha(tmp_path, s, capsys):
    d = tmp_path / "in"
    d.mkdir()
    for f in sorted((GOLDEN / "inputs").glob("*_pro.faa.gz")):
        shutil.copy(f, d / f.name)
    out = tmp_path / "out"
    assert cli.main(["-f", str(d), "-k", "5", "-c", "10", "-s", str(s), "-o", str(out)]) == 0
    text = capsys.readouterr().out
    set_key = INDEX[f"faa-5genomes_gz-{s}__protein"]
    _check_cli(out, out / "report" / "beta_diversity", "protein", "protein", set_key, f"faa-5genomes_gz-{s}/protein", text)


@pytest.mark.parametrize("s", [10, 1])
def test_cli_nucleotide_beta_and_alpha(tmp_path, s, capsys):
    d = tmp_path / "in"
    d.mkdir()
    for name in ("DJ", "GIC31", "RW1", "RW2", "Rleg"):
        shutil.copy(GOLDEN / "inputs" / f"{name}.fna.gz", d / f"{name}.fna.gz")
    out = tmp_path / "out"
    assert cli.main(["-f", str(d), "-k", "5", "-c", "10", "-s", str(s), "-o", str(out)]) == 0
    text = capsys.readouterr().out
    set_key = INDEX[f"fna-5genomes_gz-{s}__Nucleotide"]
    _check_cli(out, out / "report" / "diversity", "Nucleotide", "nucleotide", set_key, f"fna-5genomes_gz-{s}/Nucleotide", text)
    assert not (out / "report" / "beta_diversity").exists()


def test_cli_one_sample(tmp_path, capsys):
    d = tmp_path / "in"
    d.mkdir()
    shutil.copy(GOLDEN / "inputs" / "DJ_pro.faa.gz", d / "DJ_pro.faa.gz")
    out = tmp_path / "out"
    assert cli.main(["-f", str(d), "-k", "5", "-c", "10", "-o", str(out)]) == 0
    text = capsys.readouterr().out
    beta = out / "report" / "beta_diversity"
    assert len(list(beta.glob("*-protein.tsv"))) == 20
    for f in beta.glob("*-protein.tsv"):
        assert f.read_text() == "\tDJ_pro\nDJ_pro\t0.0\n", f.name
    assert "Error with beta metric: Mahalanobis\nThe number of observations (1) is too small" in text
    assert (out / "report" / "diversity" / "protein-DJ_pro.tsv").exists()
    assert not (out / "report" / "diversity-protein.tsv").exists()
