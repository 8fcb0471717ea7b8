"""Drop-ins for ``compute_alpha_diversity`` and ``compute_beta_diversity`` of lib/mercat2_diversity.py (lines 13-105).

The reference reads the sample's TSV back and hands the count column to nine scikit-bio functions
(``skbio.diversity.alpha``: shannon, simpson, simpson_e, goods_coverage, fisher_alpha, dominance,
chao1, chao1_ci, ace).  All nine are functions of a few moments of that column -- rows, sum, sum of
squares, sum of c*ln(c) and the number of rows with count 1..10 -- which ``mk_alpha_stats`` reduces on
the GPU from the table that is already there; the closed forms below turn them into the same
numbers, printed the same way (``round(x, 2)``; 'NA' where scikit-bio raises).  The integer moments and
the sum of squares are exact (rounded to float64 once); shannon of a one-row table prints as the
reference's ``-0.0``.

One limit: ``dominance`` is sum c^2 / n^2 here and a float64 sum of (c/n)^2 in scikit-bio.
Where the true value is an exact decimal tie -- 200 * sum c^2 / n^2 an odd integer -- the two may round
to different sides, and ``simpson`` with them: counts [7, 5, 8] give 138/400 = 0.345, the reference
prints 0.35, this module 0.34.  No moment can repair that.  tests/test_alpha_moments_host.py met it in
3 of 2160 seeded tables of 1..8 rows and in none of 840 tables of 50..5000 rows.

Beta diversity: the reference hands the dense samples x k-mers matrix of combined_<type>_T.tsv to scikit-bio's
``beta_diversity`` (scipy's ``pdist``, scipy 1.8.1 pinned by its recipe) for 21 metrics.  Every one of them is a
closed form of a few per-pair reductions that ``mk_pair_stats`` computes on the GPU in one pass over the union of
the tables (``native.pair_stats``; ``native.pair_stats_matrix`` from a dense matrix); ``beta_from_stats`` finishes
in n x n.  Integer statistics are exact and rounded to float64 once, so the metrics that scipy computes from exact
double sums come out with scipy's bits; canberra, seuclidean, cosine, correlation, minkowski and mahalanobis
depend on float summation order (the reference's own column order is a Python set's).
"""
from __future__ import annotations

import math
import os
from pathlib import Path
from typing import Callable, Dict, Optional, Union

import numpy as np

from . import native

METRICS = ["shannon", "simpson", "simpson_e", "goods_coverage", "fisher_alpha", "dominance", "chao1", "chao1_ci", "ace"]
Z = 1.96            # chao1_ci: scikit-bio's default z-score
RARE = 10           # ace: scikit-bio's default rare_threshold


def _fisher_alpha(n: float, s: float) -> float:
    if s >= n:
        raise RuntimeError("no finite alpha")       # scikit-bio: optimisation fails -> 'NA'
    lo, hi = 1e-12, 1.0
    g = lambda a: a * math.log(1.0 + n / a) - s
    while g(hi) < 0:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if g(mid) < 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _chao1_ci(n: float, o: int, s: int, d: int):
    if s:
        chao = o + s * (s - 1) / (2.0 * (d + 1))
        if not d:
            var = s * (s - 1) / 2.0 + s * (2 * s - 1) ** 2 / 4.0 - s ** 4 / (4.0 * chao)
        else:
            var = (s * (s - 1) / (2.0 * (d + 1)) + s * (2 * s - 1) ** 2 / (4.0 * (d + 1) ** 2) +
                   s ** 2 * d * (s - 1) ** 2 / (4.0 * (d + 1) ** 4))
        t = chao - o
        k = math.exp(abs(Z) * math.sqrt(math.log(1.0 + var / t ** 2)))
        return o + t / k, o + t * k
    p = math.exp(-n / o)
    half = Z * math.sqrt(o * p / (1 - p))
    low = o / (1 - p) - half
    return (o if o >= low else low), o / (1 - p) + half


def _ace(o: int, freq) -> Union[int, float]:
    s_rare = sum(freq[1:RARE + 1])
    singles = freq[1]
    if singles > 0 and singles == s_rare:
        raise ValueError("all rare species are singletons")
    s_abun = o - s_rare
    if s_rare == 0:
        return s_abun
    n_rare = float(sum(i * freq[i] for i in range(1, RARE + 1)))
    c_ace = 1.0 - singles / n_rare
    top = s_rare * sum(i * (i - 1) * freq[i] for i in range(1, RARE + 1))
    gamma = max(top / (c_ace * n_rare * (n_rare - 1)) - 1.0, 0.0)
    return s_abun + s_rare / c_ace + (singles / c_ace) * gamma


def _fmt(v) -> str:
    if isinstance(v, tuple):
        return "[" + ", ".join(_fmt(x) for x in v) + "]"
    if isinstance(v, int):
        return str(v)
    return repr(round(float(v), 2))


def alpha_from_stats(st: dict) -> Dict[str, str]:
    """{metric: printed value} from the moments returned by ``Counter.alpha_stats()``."""
    o, n, freq = int(st["observed"]), float(st["total"]), list(st["freq"])
    out: Dict[str, str] = {}
    if o == 0:
        return {m: "NA" for m in METRICS}
    dom = st["sum_sq"] / (n * n)

    def shannon():
        # scikit-bio sums -p ln p: -0.0 for one row (p = 1), above zero for more.  ln n - sum_clnc / n cancels to a few
        # ulps of ln n there, on either side of zero.
        if o == 1:
            return -0.0
        return max((math.log(n) - st["sum_clnc"] / n) / math.log(2), 0.0)

    values = {
        "shannon": shannon,
        "simpson": lambda: 1.0 - dom,
        "simpson_e": lambda: (1.0 / dom) / o,
        "goods_coverage": lambda: 1.0 - freq[1] / n,
        "fisher_alpha": lambda: _fisher_alpha(n, float(o)),
        "dominance": lambda: dom,
        "chao1": lambda: o + freq[1] * (freq[1] - 1) / (2.0 * (freq[2] + 1)),
        "chao1_ci": lambda: _chao1_ci(n, o, freq[1], freq[2]),
        "ace": lambda: _ace(o, freq),
    }
    for m in METRICS:
        try:
            out[m] = _fmt(values[m]())
        except Exception:
            out[m] = "NA"
    return out


def compute_alpha_diversity(basename: str, counts, out_file, *, device: int = 0) -> Dict[str, str]:
    """compute_alpha_diversity(basename, counts_tsv, out_file) of the reference; ``counts`` may also
    be the sample's Counter (its table is reduced where it is, no TSV re-read)."""
    if isinstance(counts, native.Counter):
        table = alpha_from_stats(counts.alpha_stats())
    else:
        ctx, _ = native.counter_from_tsv(counts, device=device)  # (parsed and inserted on the GPU)
        with ctx:
            table = alpha_from_stats(ctx.alpha_stats())
    with open(out_file, "w") as w:
        w.write("Metric\t%s\n" % basename)
        for m in METRICS:
            w.write("%s\t%s\n" % (m, table[m]))
    return table


# ------------------------------------------------------------------------------------------ beta diversity
BETA_METRICS = ["euclidean", "cityblock", "braycurtis", "canberra", "chebyshev", "correlation", "cosine", "dice",
                "hamming", "jaccard", "mahalanobis", "manhattan", "matching", "minkowski", "rogerstanimoto",
                "russellrao", "seuclidean", "sokalmichener", "sokalsneath", "sqeuclidean", "yule"]
MAX_BETA_SAMPLES = 4096  # mk_pair_stats' limit
NAN_ERROR = "Data must be symmetric and cannot contain NaNs."  # scikit-bio's DistanceMatrix on a NaN


def _ints(a, n: int) -> np.ndarray:
    """n x n object array of Python ints (exact arithmetic) from nested lists or a uint64 array."""
    a = np.asarray(a, dtype=object) if isinstance(a, list) else np.asarray(a).astype(object)
    return a.reshape(n, n)


def _f64(a: np.ndarray) -> np.ndarray:
    """Each exact integer rounded to float64 once."""
    return np.array([float(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def _mahalanobis(X: np.ndarray) -> np.ndarray:
    """scipy's pdist(X, 'mahalanobis') with its default VI = inv(cov(X.T)).T (numpy's inv raises when singular)."""
    X = np.asarray(X, dtype=np.float64)
    VI = np.linalg.inv(np.atleast_2d(np.cov(X.T))).T
    n = X.shape[0]
    out = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            delta = X[i] - X[j]
            out[i, j] = out[j, i] = np.sqrt(delta.dot(VI).dot(delta))
    return out


def beta_from_stats(stats: dict, dense: Optional[Callable[[], np.ndarray]] = None) -> Dict[str, Union[np.ndarray, str]]:
    """{metric: n x n float64 matrix, or the error text the reference prints} in ``BETA_METRICS`` order, from the
    per-pair statistics ``native.pair_stats`` returns (the same keys: dot, l1, cheb, neq, both, canb, seuc, sums,
    rows, constant_row).  ``dense`` gives the samples x rows count matrix; it is needed only for mahalanobis when
    there are more samples than union rows (scipy refuses every other case)."""
    n, d = len(stats["sums"]), int(stats["rows"])
    dot, l1, both = _ints(stats["dot"], n), _ints(stats["l1"], n), _ints(stats["both"], n)
    neq, cheb = _ints(stats["neq"], n), _ints(stats["cheb"], n)
    S = np.array([int(v) for v in stats["sums"]] + [0], dtype=object)[:n]
    Q = np.array([dot[i, i] for i in range(n)] + [0], dtype=object)[:n]
    z = np.array([both[i, i] for i in range(n)] + [0], dtype=object)[:n]
    Si, Sj, Qi, Qj, zi, zj = S[:, None], S[None, :], Q[:, None], Q[None, :], z[:, None], z[None, :]
    ntt = both
    ntf, nft = zi - both, zj - both
    nff = d - zi - zj + both
    R2 = 2 * (ntf + nft)

    def correlation():
        num = d * dot - Si * Sj
        var = d * Q - S * S
        r = _f64(num) / (np.sqrt(_f64(var))[:, None] * np.sqrt(_f64(var))[None, :])
        return 1.0 - np.clip(r, -1.0, 1.0)

    def cosine():
        r = _f64(dot) / (np.sqrt(_f64(Q))[:, None] * np.sqrt(_f64(Q))[None, :])
        return 1.0 - np.clip(r, -1.0, 1.0)

    def jaccard():
        den = zi + zj - both
        return np.where(den == 0, 0.0, _f64(neq) / _f64(den))

    def mahalanobis():
        if n <= d:
            raise ValueError("The number of observations (%d) is too small; the covariance matrix is singular. For "
                             "observations with %d dimensions, at least %d observations are required." % (n, d, d + 1))
        if dense is None:
            raise ValueError("mahalanobis: the dense matrix is needed")
        return _mahalanobis(dense())

    def seuclidean():
        if n >= 2 and stats["constant_row"]:
            return np.full((n, n), np.nan)
        return np.sqrt(np.asarray(stats["seuc"], dtype=np.float64).reshape(n, n))

    def yule():
        half = ntf * nft
        return np.where(half == 0, 0.0, _f64(2 * half) / _f64(ntt * nff + half))

    sq = lambda: _f64(Qi + Qj - 2 * dot)
    rules = {
        "euclidean": lambda: np.sqrt(sq()),
        "cityblock": lambda: _f64(l1),
        "braycurtis": lambda: _f64(l1) / _f64(Si + Sj),
        "canberra": lambda: np.asarray(stats["canb"], dtype=np.float64).reshape(n, n),
        "chebyshev": lambda: _f64(cheb),
        "correlation": correlation,
        "cosine": cosine,
        "dice": lambda: _f64(ntf + nft) / _f64(2 * ntt + ntf + nft),
        "hamming": lambda: _f64(neq) / np.float64(d),
        "jaccard": jaccard,
        "mahalanobis": mahalanobis,
        "manhattan": lambda: _f64(l1),
        "matching": lambda: _f64(neq) / np.float64(d),
        "minkowski": lambda: np.sqrt(sq()),
        "rogerstanimoto": lambda: _f64(R2) / _f64(ntt + nff + R2),
        "russellrao": lambda: _f64(d - ntt) / np.float64(d),
        "seuclidean": seuclidean,
        "sokalmichener": lambda: _f64(R2) / _f64(ntt + nff + R2),
        "sokalsneath": lambda: _f64(R2) / _f64(ntt + R2),
        "sqeuclidean": sq,
        "yule": yule,
    }
    out: Dict[str, Union[np.ndarray, str]] = {}
    off = ~np.eye(n, dtype=bool)
    for m in BETA_METRICS:
        try:
            with np.errstate(all="ignore"):
                v = np.where(off, np.asarray(rules[m](), dtype=np.float64), 0.0)
            out[m] = NAN_ERROR if np.isnan(v).any() else v
        except Exception as e:  # noqa: BLE001 -- printed as the reference prints it
            out[m] = str(e)
    return out


def write_beta_tsv(path, ids, matrix: np.ndarray) -> None:
    """The reference's file: a tab, then the IDs; one row per sample, values as str(numpy.float64)."""
    with open(path, "w") as w:
        w.write("\t" + "\t".join(ids) + "\n")
        for i, name in enumerate(ids):
            w.write(name + "\t" + "\t".join(repr(float(v)) for v in matrix[i]) + "\n")


def _read_combined_T(path) -> tuple:
    """(sample names, samples x k-mers int64 matrix) of a combined_<type>_T.tsv."""
    ids, rows = [], []
    with open(path) as r:
        r.readline()
        for line in r:
            parts = line.rstrip("\n").split("\t")
            ids.append(parts[0])
            rows.append(np.array(parts[1:], dtype=np.int64))
    d = rows[0].size if rows else 0
    return ids, (np.vstack(rows) if rows else np.zeros((0, d), dtype=np.int64))


def compute_beta_diversity(basename: str, counts, outpath, *, device: int = 0) -> Dict[str, Union[np.ndarray, str]]:
    """compute_beta_diversity(basename, counts_tsv, outpath) of the reference: <metric>-<basename>.tsv per metric
    into ``outpath``, 'Error with beta metric: <Metric>' and the error text for the others (no plots).  ``counts``
    is a combined_<type>_T.tsv, or the CLI's {sample: Counter} (the statistics come from the tables on the GPU)."""
    outpath = Path(outpath)
    outpath.mkdir(0o777, True, True)
    if isinstance(counts, dict):
        ids = sorted(counts)
        if len(ids) > MAX_BETA_SAMPLES:
            print(f"Beta diversity skipped: {len(ids)} samples, at most {MAX_BETA_SAMPLES} are supported")
            return {}
        ctxs = [counts[i] for i in ids]
        stats = native.pair_stats(ctxs)
        dense = lambda: native.merged_export(ctxs)[1].T.astype(np.float64)
    else:
        ids, X = _read_combined_T(counts)
        if len(ids) > MAX_BETA_SAMPLES:
            print(f"Beta diversity skipped: {len(ids)} samples, at most {MAX_BETA_SAMPLES} are supported")
            return {}
        stats = native.pair_stats_matrix(np.ascontiguousarray(X.T), device=device)
        dense = lambda: X.astype(np.float64)
    result = beta_from_stats(stats, dense)
    for metric in BETA_METRICS:
        v = result[metric]
        if isinstance(v, str):
            print(f"Error with beta metric: {metric.capitalize()}")
            print(v)
        else:
            write_beta_tsv(outpath / f"{metric}-{basename}.tsv", ids, v)
    return result


def merge_alpha(files: Dict[str, os.PathLike], out_file) -> None:
    """merge_tsv (lib/mercat2_report.py:98-156) over per-sample alpha files, as bin/mercat2.py:479-499 calls it:
    'Metric' and the sorted sample names, then each metric's row (the files share their row order)."""
    names = sorted(files)
    cols = []
    for name in names:
        with open(files[name]) as r:
            r.readline()
            cols.append([line.rstrip("\n").split("\t") for line in r if line.strip()])
    with open(out_file, "w") as w:
        w.write("Metric\t" + "\t".join(names) + "\n")
        for i, row in enumerate(cols[0]):
            w.write(row[0] + "\t" + "\t".join(c[i][1] for c in cols) + "\n")
