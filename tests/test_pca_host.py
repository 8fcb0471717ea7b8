"""Host math of -pca (mercat2_amd/pca.py), no GPU: exact Gram -> centred eigen-decomposition against a numpy SVD
restatement, the reference's committed pca.tsv files rebuilt from their committed count tables, file layout and the
cases that write nothing."""
import gzip
import json
import re
from pathlib import Path

import numpy as np
import pytest

from mercat2_amd import pca

PCA = Path(__file__).resolve().parent / "golden" / "pca"


def _gram(X):
    m = np.asarray(X, dtype=object)
    return m.dot(m.T).tolist()


def _svd_pca(X):
    Xc = np.asarray(X, dtype=np.float64)
    Xc = Xc - Xc.mean(axis=0)
    U, S, _ = np.linalg.svd(Xc, full_matrices=False)
    idx = np.argmax(np.abs(U), axis=0)
    U = U * np.sign(U[idx, range(U.shape[1])])
    lam = S ** 2
    return (U * S)[:, :3], lam[:3] / (len(X) - 1), lam[:3] / lam.sum()


@pytest.mark.parametrize("seed", range(6))
def test_pca_from_gram_matches_svd(seed):
    rnd = np.random.default_rng(seed)
    n, f = int(rnd.integers(4, 12)), int(rnd.integers(20, 300))
    # a spread-out spectrum (no near ties among the top components)
    X = rnd.integers(0, 50, (n, f)) + np.outer(rnd.integers(1, 9, n), rnd.integers(0, 400, f)) \
        + np.outer(rnd.integers(1, 4, n) * 7, rnd.integers(0, 90, f))
    res = pca.pca_from_gram(_gram(X), ["s%d" % i for i in range(n)], f)
    scores, var, ratio = _svd_pca(X)
    np.testing.assert_allclose(res["scores"], scores, rtol=1e-9, atol=1e-9 * np.abs(scores).max())
    np.testing.assert_allclose(res["explained_variance_"], var, rtol=1e-9)
    np.testing.assert_allclose(res["explained_variance_ratio_"], ratio, rtol=1e-9)


def test_pca_from_gram_huge_counts_exact_centring():
    """Counts near 2^40: the centring must not lose the small differences (it is done in integers)."""
    base = 1 << 40
    X = [[base + a, base + 2 * a + 1, base - a, base + 3] for a in (0, 5, 11, 19, 30)]
    res = pca.pca_from_gram(_gram(X), list("abcde"), 4)
    scores, _, _ = _svd_pca(np.asarray(X, dtype=np.float64) - base)
    np.testing.assert_allclose(res["scores"][:, :2], scores[:, :2], rtol=1e-6, atol=1e-6 * np.abs(scores).max())


def _tables():
    with gzip.open(PCA / "tables.json.gz", "rt") as fh:
        sets = json.load(fh)
    # a key listed twice keeps its last count, as merge_tsv_T does
    return {name: {s: {k: c for k, c in rows} for s, rows in samples.items()} for name, samples in sets.items()}


TABLES = _tables()


def _read(path):
    lines = Path(path).read_text().splitlines()
    return lines[0], [l.split("\t")[0] for l in lines[1:]], np.array([[float(x) for x in l.split("\t")[1:]] for l in lines[1:]])


INDEX = json.loads((PCA / "index.json").read_text())


def test_sixteen_committed_files():
    assert len(INDEX) == 16


@pytest.mark.parametrize("key", sorted(INDEX))
def test_committed_pca_rebuilt_from_committed_tables(key, tmp_path):
    tables = TABLES[INDEX[key]]
    names = sorted(tables)
    keys = sorted(set().union(*[set(t) for t in tables.values()]))
    gram = [[sum(tables[a].get(k, 0) * tables[b].get(k, 0) for k in tables[a].keys() & tables[b].keys()) for b in names]
            for a in names]
    res = pca.pca_from_gram(gram, names, len(keys))
    path = pca.write_pca_tsv(res, tmp_path)
    head, got_names, got = _read(path)
    _, want_names, want = _read(PCA / f"{key}.tsv")
    assert head == "sample\tPC1\tPC2\tPC3"
    assert got_names == want_names
    assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))
    assert (np.sign(got) == np.sign(want)).all()


def test_write_layout_and_name_stripping(tmp_path):
    res = {"names": ["DJ_pro", "a_protein", "b_protein_x"], "scores": np.array([[1.5, -2.0, 0.25]] * 3)}
    text = Path(pca.write_pca_tsv(res, tmp_path / "pca_protein")).read_text()
    assert text == ("sample\tPC1\tPC2\tPC3\n"
                    "DJ_pro\t1.5\t-2.0\t0.25\n"
                    "a\t1.5\t-2.0\t0.25\n"
                    "b_x\t1.5\t-2.0\t0.25\n")
    assert re.sub(r"_protein", "", "b_protein_x") == "b_x"


def test_sign_tie_first_entry_wins():
    # two samples mirrored around the mean: the first component's entries tie in magnitude
    X = [[0, 0], [2, 4]] + [[1, 2]] * 2
    res = pca.pca_from_gram(_gram(X), list("abcd"), 2, n_components=1)
    assert res["scores"][0, 0] > 0 and res["scores"][1, 0] < 0


def test_too_few_features_refused():
    with pytest.raises(ValueError):
        pca.pca_from_gram(_gram([[1, 2], [3, 4], [5, 7], [1, 1]]), list("abcd"), 2)


def test_cli_step_three_samples_or_fewer_does_nothing(tmp_path, capsys):
    assert pca.cli_pca({"a": None, "b": None, "c": None}, tmp_path, "protein") is False
    assert not (tmp_path / "pca_protein").exists()
    assert "Running PCA" not in capsys.readouterr().out


def test_cli_step_more_than_1000_samples_refused(tmp_path, capsys):
    assert pca.cli_pca({"s%d" % i: None for i in range(1001)}, tmp_path, "Nucleotide") is False
    out = capsys.readouterr().out
    assert "Running PCA" in out and "IncrementalPCA" in out
    assert not (tmp_path / "pca_Nucleotide").exists()


def test_plot_PCA_refuses_more_than_1000_samples(tmp_path):
    f = tmp_path / "combined_T.tsv"
    f.write_text("sample\tAAA\tCCC\tGGG\n" + "".join("s%d\t1\t2\t%d\n" % (i, i) for i in range(1001)))
    with pytest.raises(ValueError):
        pca.plot_PCA(str(f), str(tmp_path / "out"))
    assert not (tmp_path / "out" / "pca.tsv").exists()


def test_read_matrix_T(tmp_path):
    f = tmp_path / "t.tsv"
    f.write_text("sample\tAAA\tCCC\nx\t1\t0\ny_protein\t5\t7\n")
    names, nf, m = pca.read_matrix_T(f)
    assert names == ["x", "y_protein"] and nf == 2
    assert m.tolist() == [[1, 5], [0, 7]] and m.dtype == np.uint64
