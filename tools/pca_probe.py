"""Times the parts of -pca on the GPU and the host alternative on the same tables.

    python tools/pca_probe.py synth  [--samples 8] [--reads 10000000] [--genome 5000000] [--k 31] [--c 2]
    python tools/pca_probe.py small  [--samples 64] [--k 5]

Parts: gather (mk_export_pairs_device of every table, sorted keys on the device), mk_gram in all (gather + join + Gram),
the Gram kernel alone (mk_gram_matrix on the dense union matrix, less its host-to-device copy), the host math
(pca_from_gram); and mk_merged_export + numpy (X^T X in float64 after the merge on the host) as the host path.
Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/pca_probe.py ...`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402,F401  (its HIP runtime first, as the tests load it)

from mercat2_amd import native, pca  # noqa: E402


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    r = f(*a, **kw)
    return r, time.perf_counter() - t0


def build(args):
    ctxs = []
    for s in range(args.samples):
        if args.case == "synth":
            text = native.synth_reads(args.genome, 1000 + s, args.reads, 150, 5000 + s).tobytes()
        else:
            rnd = np.random.default_rng(s)
            seq = "".join("ACGT"[x] for x in rnd.integers(0, 4, 200_000))
            text = (">s\n" + seq + "\n").encode()
        c = native.Counter(args.k, native.ALPHABET_NT2, device=0)
        c.count_chunk(text, args.c)
        c.trim()
        ctxs.append(c)
        del text
    return ctxs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("case", choices=["synth", "small"])
    p.add_argument("--samples", type=int, default=None)
    p.add_argument("--reads", type=int, default=10_000_000)
    p.add_argument("--genome", type=int, default=5_000_000)
    p.add_argument("--k", type=int, default=None)
    p.add_argument("--c", type=int, default=None)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--host", action="store_true", help="also time mk_merged_export + numpy")
    args = p.parse_args()
    if args.samples is None:
        args.samples = 8 if args.case == "synth" else 64
    if args.k is None:
        args.k = 31 if args.case == "synth" else 5
    if args.c is None:
        args.c = 2 if args.case == "synth" else 1
    ctxs, t_count = timed(build, args)
    n = len(ctxs)
    out = {"case": args.case, "samples": n, "k": args.k, "c": args.c, "count_s": round(t_count, 3)}
    # gather alone: every table's sorted packed keys on the device
    import torch as T
    t_g = 0.0
    for c in ctxs:
        rows = c.rows()
        w = c.words_per_key()
        keys = T.empty(max(1, rows) * w, dtype=T.int64, device="cuda:0")
        cnts = T.empty(max(1, rows), dtype=T.int64, device="cuda:0")
        T.cuda.synchronize()
        _, dt = timed(c.export_pairs_device, keys.data_ptr(), cnts.data_ptr(), rows)
        t_g += dt
        del keys, cnts
    out["gather_s"] = round(t_g, 4)
    best = None
    for _ in range(args.repeat):
        (g, rows), dt = timed(native.gram, ctxs)
        best = dt if best is None else min(best, dt)
    out["union_rows"] = rows
    out["mk_gram_s"] = round(best, 4)
    res, dt = timed(pca.pca_from_gram, g, ["s%d" % i for i in range(n)], rows)
    out["host_pca_s"] = round(dt, 5)
    # the Gram kernel alone: the dense union matrix through mk_gram_matrix, less its host-to-device copy
    (_, matrix), dt_merge = timed(native.merged_export, ctxs)
    out["merged_export_s"] = round(dt_merge, 3)
    g2, dt_gm = timed(native.gram_matrix, matrix)
    for _ in range(args.repeat - 1):
        _, dt = timed(native.gram_matrix, matrix)
        dt_gm = min(dt_gm, dt)
    assert g2 == g, "mk_gram_matrix and mk_gram differ"
    host = T.from_numpy(matrix.view(np.int64))
    T.cuda.synchronize()
    _, dt_h2d = timed(lambda: (host.to("cuda:0"), T.cuda.synchronize()))
    _, dt_h2d = timed(lambda: (host.to("cuda:0"), T.cuda.synchronize()))
    out["gram_matrix_s"] = round(dt_gm, 4)
    out["h2d_s"] = round(dt_h2d, 4)
    out["matrix_bytes"] = int(matrix.nbytes)
    if args.host:
        _, dt = timed(lambda: matrix.astype(np.float64).T @ matrix.astype(np.float64))
        out["numpy_xtx_s"] = round(dt, 3)
        out["host_path_s"] = round(dt_merge + dt, 3)
    for c in ctxs:
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
