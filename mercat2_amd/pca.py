"""Sample PCA of MerCat2's -pca (lib/mercat2_figures.py:206-291, called from bin/mercat2.py:170-181 for every sample
type with more than three samples): the three principal-component scores of every sample, written to
``pca_<type>/pca.tsv``.

The reference reads the dense ``combined_<type>_T.tsv`` (samples x k-mers) back and fits
``sklearn.decomposition.PCA(n_components=3)``.  Here the GPU computes the exact integer Gram matrix G = X X^T of the
samples' count columns over the union of their k-mers (``native.gram`` from the tables on the GPU,
``native.gram_matrix`` from a dense matrix), and the host finishes in n x n:

* centring in exact integers: n^2 Gc_ij = n^2 G_ij - n a_i - n a_j + b (a_i = sum_j G_ij, b = sum_ij G_ij), rounded once
  to float64;
* the top three eigenpairs of Gc (``numpy.linalg.eigh``, eigenvalues clipped at 0): scores u_j sqrt(lambda_j);
* signs: the largest-magnitude entry of each u_j is made positive (the first on a tie) -- scikit-learn's ``svd_flip``
  with ``u_based_decision=True``, the rule its releases before 1.5 applied and the reference's committed outputs show.

That is exact PCA (``svd_solver='full'``).  The reference's default solver is randomized beyond 13 samples and not
reproducible there; it is exact up to that size, where the two agree.
"""
from __future__ import annotations

import os
import re
from typing import Dict, Sequence

import numpy as np

MAX_SAMPLES = 1000  # beyond this the reference switches to IncrementalPCA (not reproduced here)


def pca_from_gram(gram_ints, names: Sequence[str], n_features: int, n_components: int = 3) -> dict:
    """PCA of the n samples whose exact Gram matrix (n x n Python ints, nested lists or an object array) is given.
    Returns ``names``, ``scores`` (n x n_components float64), ``explained_variance_`` and ``explained_variance_ratio_``.
    Like the reference's PCA it needs n_components <= min(n, n_features): ValueError otherwise."""
    names = list(names)
    n = len(names)
    G = [[int(v) for v in row] for row in gram_ints]
    if len(G) != n or any(len(row) != n for row in G):
        raise ValueError("pca_from_gram: the Gram matrix must be %d x %d" % (n, n))
    if not 1 <= n_components <= min(n, int(n_features)):
        raise ValueError("n_components=%d must be between 1 and min(n_samples, n_features)=%d" %
                         (n_components, min(n, int(n_features))))
    a = [sum(row) for row in G]
    b = sum(a)
    nn = n * n
    gc = np.empty((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(n):
            gc[i, j] = (nn * G[i][j] - n * a[i] - n * a[j] + b) / nn  # (exact integer numerator, one rounding)
    lam, vec = np.linalg.eigh(gc)
    order = np.argsort(lam)[::-1][:n_components]
    lam = np.clip(lam[order], 0.0, None)
    u = vec[:, order]
    pick = np.argmax(np.abs(u), axis=0)
    signs = np.sign(u[pick, np.arange(u.shape[1])])
    signs[signs == 0] = 1.0
    u = u * signs
    scores = u * np.sqrt(lam)
    total = float(np.trace(gc))
    return {
        "names": names,
        "scores": scores,
        "explained_variance_": lam / (n - 1) if n > 1 else np.zeros_like(lam),
        "explained_variance_ratio_": lam / total if total > 0 else np.zeros_like(lam),
        "n_features": int(n_features),
    }


def pca_counters(counters: Dict[str, "object"], n_components: int = 3, slab_rows: int = 0) -> dict:
    """PCA of ``{sample name: native.Counter}`` (sorted names, as the combined tables order them) from the tables on
    the GPU."""
    from . import native
    names = sorted(counters.keys())
    gram, rows = native.gram([counters[n] for n in names], slab_rows=slab_rows)
    return pca_from_gram(gram, names, rows, n_components)


def write_pca_tsv(result: dict, out_path) -> str:
    """``out_path/pca.tsv`` laid out as the reference writes it: header, then each sample's name (``_protein``
    removed) and its scores."""
    os.makedirs(out_path, exist_ok=True)
    pca_tsv = os.path.join(out_path, "pca.tsv")
    with open(pca_tsv, "w") as out:
        print("sample", "PC1", "PC2", "PC3", sep="\t", file=out)
        for name, row in zip(result["names"], result["scores"]):
            out.write(re.sub(r"_protein", "", name))
            for c in row:
                out.write(f"\t{c}")
            out.write("\n")
    return pca_tsv


def read_matrix_T(tsv_file):
    """(names, k-mer count, rows x n uint64 matrix) of a ``combined_*_T.tsv`` (``sample`` + one column per k-mer, one
    line per sample)."""
    names, cols = [], []
    with open(tsv_file) as reader:
        header = reader.readline().rstrip("\n").split("\t")
        n_features = len(header) - 1
        for line in reader:
            parts = line.rstrip("\n").split("\t")
            if not parts or parts == [""]:
                continue
            names.append(parts[0])
            cols.append(np.array([int(x) for x in parts[1:]], dtype=np.uint64))
    matrix = np.stack(cols, axis=1) if cols else np.zeros((n_features, 0), dtype=np.uint64)
    return names, n_features, np.ascontiguousarray(matrix)


def plot_PCA(tsv_file, out_path, lowmem=None, class_file=None, DEBUG=False):
    """plot_PCA of lib/mercat2_figures.py:206 (same arguments): writes ``out_path/pca.tsv`` from a
    ``combined_*_T.tsv`` and returns ``(None, None)`` in place of the two plotly figures (no plots here).
    ``lowmem`` and ``class_file`` change nothing (the reference's IncrementalPCA is not reproduced: more than 1000
    samples raise ValueError; the class file only colours the plots)."""
    from . import native
    names, n_features, matrix = read_matrix_T(tsv_file)
    if len(names) > MAX_SAMPLES:
        raise ValueError("plot_PCA: %d samples: MerCat2 switches to IncrementalPCA beyond %d, which is not part of "
                         "this engine" % (len(names), MAX_SAMPLES))
    print("Using Incremental PCA:", False)
    gram = native.gram_matrix(matrix, device=0)
    write_pca_tsv(pca_from_gram(gram, names, n_features), out_path)
    return None, None


def cli_pca(tables: Dict[str, "object"], out_dir, type_string: str) -> bool:
    """The -pca step of the CLI for one sample type (bin/mercat2.py:170-181): ``out_dir/pca_<type>/pca.tsv`` when more
    than three samples produced a table.  Returns whether the file was written."""
    if len(tables) <= 3:
        return False
    print("\nRunning PCA")
    if len(tables) > MAX_SAMPLES:
        print(f"PCA skipped: {len(tables)} {type_string} samples; MerCat2 switches to IncrementalPCA beyond {MAX_SAMPLES} "
              "samples, which this engine does not reproduce")
        return False
    print("Using Incremental PCA:", False)
    from . import native
    names = sorted(tables.keys())
    gram, rows = native.gram([tables[n] for n in names])
    if rows < 3:
        print(f"PCA skipped: the {type_string} samples hold {rows} different k-mers; three components need at least 3")
        return False
    write_pca_tsv(pca_from_gram(gram, names, rows), os.path.join(str(out_dir), f"pca_{type_string}"))
    return True
