"""Copy the reference's committed sample PCA outputs (results/2023-11-29/*/pca_*/pca.tsv) and the count tables they were
computed from into tests/golden/pca/, and check that exact PCA -- the columns of the samples x k-mers union matrix
centred in float64, an SVD, the largest-magnitude entry of each left singular vector made positive -- rebuilds every
committed pca.tsv from its run's committed tsv_*/*_counts.tsv to <= 1e-12 x sigma_1.

    python tests/golden/make_pca_golden.py <reference checkout>

Layout: pca/<run>__<type>.tsv (the committed file); pca/tables.json.gz, each distinct set of count tables once as
{"<set>": {"<sample>": [[kmer, count], ...]}} (rows in file order; gzip with a zero timestamp, so the bytes are
reproducible); pca/index.json ({"<run>__<type>": "<set>"}).  Nothing here imports the reference's code: only its data.
"""
import gzip
import hashlib
import json
import os
import re
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pca")
TSV_DIR = {"Nucleotide": "tsv_nucleotide", "protein": "tsv_protein", "prod": "tsv_prod", "fgs": "tsv_fgs"}


README = """# Sample PCA goldens

Made by `../make_pca_golden.py` from the reference's committed results (data only):

* `<run>__<type>.tsv` -- the 16 committed `results/2023-11-29/<run>/pca_<type>/pca.tsv` (protein, nucleotide,
  prodigal and FragGeneScan samples; `-s 1` and `-s 10`; plain and `.gz` inputs).
* `tables.json.gz` -- each distinct set of the committed `tsv_*/*_counts.tsv` those files were computed from, once:
  `{"<set>": {"<sample>": [[kmer, count], ...]}}`, rows in file order.
* `index.json` -- which set belongs to which file.

The script asserts that exact PCA of the union matrix (columns centred in float64, SVD, the largest-magnitude entry of
each left singular vector made positive) rebuilds every committed file from its tables to <= 1e-12 x sigma_1
(measured: <= 4e-14).
"""


def read_rows(folder):
    """{sample: [[kmer, count], ...]} of a tsv_* folder, rows in file order."""
    out = {}
    for name in sorted(os.listdir(folder)):
        if not name.endswith("_counts.tsv"):
            continue
        rows = []
        with open(os.path.join(folder, name)) as fh:
            fh.readline()
            for line in fh:
                kmer, count = line.split()
                rows.append([kmer, int(count)])
        out[name[: -len("_counts.tsv")]] = rows
    return out


def as_tables(rows):
    """{sample: {kmer: count}}; a key listed twice keeps its last count, as merge_tsv_T does."""
    return {s: {k: c for k, c in r} for s, r in rows.items()}


def exact_pca(tables):
    """(names, scores n x 3, sigma_1): the reference's PCA(n_components=3) with the full solver and the
    u-based sign rule (the rule of the scikit-learn release the committed files were made with)."""
    names = sorted(tables)
    keys = sorted(set().union(*[set(t) for t in tables.values()]))
    X = np.array([[tables[s].get(k, 0) for k in keys] for s in names], dtype=np.float64)
    Xc = X - X.mean(axis=0)
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    idx = np.argmax(np.abs(U), axis=0)
    signs = np.sign(U[idx, range(U.shape[1])])
    U = U * signs
    return names, (U * S)[:, :3], float(S[0])


def read_pca(path):
    names, rows = [], []
    with open(path) as fh:
        fh.readline()
        for line in fh:
            parts = line.rstrip("\n").split("\t")
            names.append(parts[0])
            rows.append([float(x) for x in parts[1:]])
    return names, np.array(rows)


def main(ref):
    results = os.path.join(ref, "results", "2023-11-29")
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    index, seen, sets = {}, {}, {}
    for run in sorted(os.listdir(results)):
        for typ, tsv_dir in TSV_DIR.items():
            pca = os.path.join(results, run, f"pca_{typ}", "pca.tsv")
            if not os.path.exists(pca):
                continue
            folder = os.path.join(results, run, tsv_dir)
            digest = hashlib.sha256()
            for name in sorted(os.listdir(folder)):
                with open(os.path.join(folder, name), "rb") as fh:
                    digest.update(name.encode() + b"\0" + fh.read())
            d = digest.hexdigest()
            if d not in seen:
                seen[d] = f"{run}__{tsv_dir}"
                sets[seen[d]] = read_rows(folder)
            key = f"{run}__{typ}"
            index[key] = seen[d]
            shutil.copyfile(pca, os.path.join(OUT, key + ".tsv"))
            names, scores, s1 = exact_pca(as_tables(sets[seen[d]]))
            got_names, want = read_pca(pca)
            assert got_names == [re.sub(r"_protein", "", n) for n in names], (key, got_names, names)
            err = float(np.max(np.abs(scores - want)))
            assert err <= 1e-12 * s1, (key, err, s1)
            print(f"{key}: {len(names)} samples, tables {seen[d]}, max |diff| = {err:.3g} = {err / s1:.2g} x sigma_1")
    with open(os.path.join(OUT, "tables.json.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, compresslevel=9, mtime=0) as gz:
            gz.write(json.dumps(sets, sort_keys=True, separators=(",", ":")).encode())
    with open(os.path.join(OUT, "index.json"), "w") as fh:
        json.dump(index, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(OUT, "README.md"), "w") as fh:
        fh.write(README)
    assert len(index) == 16, len(index)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MERCAT2_REF", "../mercat2"))
