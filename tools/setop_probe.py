"""two tables combined by key on the GPU (Counter.combine / mk_table_op) against the fastest way to the same
table in HBM without it -- export() of both, a numpy join over the packed keys, the rows back in through
import_pairs_device (and, at the small size, through load_tsv, to say which way back is faster) -- in one process.
Every op; warm-ups first, then median (min-max); the yardstick once per op, its rows asserted equal.

    python tools/setop_probe.py [--genome 500000,5000000] [--runs 7]

Tables: synth_reads at k = 31, -c 1 (about 2 rows per base); a = read seed 4, b = the same genome, read seed 5.
Beside it, as descriptions: s_scan against mk_histo's s_scan on a (one read of a), rows/s, and (slots x 16 B) / s_scan
next to the device-to-device copy rate.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mercat2_amd import native  # noqa: E402

K = 31
M64 = (1 << 64) - 1
CODE = np.full(256, 0, dtype=np.uint64)
for i, ch in enumerate(b"ACGT"):
    CODE[ch] = i


def pack(kmers: np.ndarray) -> np.ndarray:
    """(rows, K) ACGT bytes -> the one-word keys (first base most significant): sorted rows give sorted keys."""
    out = np.zeros(kmers.shape[0], dtype=np.uint64)
    for j in range(K):
        out = (out << np.uint64(2)) | CODE[kmers[:, j]]
    return out


def join(ka, ca, kb, cb, op):
    """The rule of mk_table_op over two sorted key columns (thresholds 1) -> (keys, counts), counts not 0."""
    at = np.searchsorted(kb, ka)
    at[at == len(kb)] = 0
    hit = kb[at] == ka if len(kb) else np.zeros(len(ka), dtype=bool)
    cb_of_a = np.where(hit, cb[at] if len(kb) else 0, 0).astype(np.uint64)
    if op == "min":
        keys, cnts = ka, np.minimum(ca, cb_of_a)
    elif op == "left":
        keys, cnts = ka, np.where(hit, ca, 0)
    elif op == "only":
        keys, cnts = ka, np.where(hit, 0, ca)
    elif op == "diff":
        keys, cnts = ka, np.where(ca > cb_of_a, ca - cb_of_a, 0)
    else:
        in_a = np.zeros(len(kb), dtype=bool)
        in_a[at[hit]] = True
        keys = np.concatenate([ka, kb[~in_a]])
        cnts = np.concatenate([np.maximum(ca, cb_of_a) if op == "max" else ca + cb_of_a, cb[~in_a]])
    keep = cnts != 0
    return keys[keep], cnts[keep].astype(np.uint64)


def timed(fn, warmups, runs):
    for _ in range(warmups):
        fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def med(times):
    return "%9.3f ms (%.3f-%.3f)" % (1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times))


def stream_copy_gbs(torch):
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)

    def copy():
        b.copy_(a)
        torch.cuda.synchronize()
    return 2 * a.numel() / statistics.median(timed(copy, 2, 7)) / 1e9


def probe(torch, genome, args, copy_gbs):
    with native.Counter(K, native.ALPHABET_NT2) as a, native.Counter(K, native.ALPHABET_NT2) as b, \
            native.Counter(K, native.ALPHABET_NT2) as dst, native.Counter(K, native.ALPHABET_NT2) as yard:
        a.count_chunk(native.synth_reads(genome, 3, genome // 10, 150, 4), 1)
        b.count_chunk(native.synth_reads(genome, 3, genome // 10, 150, 5), 1)
        hist = {}
        scans_h = []
        for _ in range(5):
            a.histo(100, info=hist)
            scans_h.append(hist["s_scan"])
        floor = statistics.median(scans_h[2:])
        print("genome %d: a %d rows, b %d rows, a's %d slots of 16 B; mk_histo s_scan on a %.3f ms; copy %.0f GB/s" % (
            genome, a.rows(), b.rows(), hist["slots"], 1e3 * floor, copy_gbs), flush=True)
        worst = None
        for op in native.OPS:
            info, scans = {}, []

            def run():
                a.combine(b, op, into=dst, info=info)
                scans.append(info["s_scan"])
            wall = timed(run, 2, args.runs)
            s_scan = statistics.median(scans[2:])
            got_k, got_c = dst.export()

            def by_export(back="pairs"):
                ka, ca = a.export()
                kb, cb = b.export()
                keys, cnts = join(pack(ka), ca, pack(kb), cb, op)
                yard.reset()
                if back == "pairs":
                    d_k = torch.from_numpy(keys.view(np.int64)).cuda()
                    d_c = torch.from_numpy(cnts.view(np.int64)).cuda()
                    torch.cuda.synchronize()
                    yard.import_pairs_device(d_k.data_ptr(), d_c.data_ptr(), len(keys))
                else:
                    text = np.empty((len(keys), K), dtype=np.uint8)  # (built column-wise)
                    for j in range(K):
                        text[:, j] = np.frombuffer(b"ACGT", dtype=np.uint8)[((keys >> np.uint64(2 * (K - 1 - j))) & np.uint64(3)).astype(np.int64)]
                    digits = np.char.mod("%d", cnts.astype(object) if cnts.max(initial=0) > 2 ** 63 else cnts.astype(np.int64))
                    lines = np.char.add(np.char.add(text.view("S%d" % K).ravel().astype(str), "\t"), digits)
                    yard.load_tsv(("\n".join(lines.tolist()) + "\n").encode() if len(lines) else b"")
                yard.rows()
            t0 = time.perf_counter()
            by_export()
            t_yard = time.perf_counter() - t0
            yk, yc = yard.export()
            assert np.array_equal(yk, got_k) and np.array_equal(yc, got_c), "the yardstick's rows differ (%s)" % op
            line = "  %-5s combine %s  s_scan %.3f ms = %.2f x histo  %.0f M rows of a/s  slots x 16 B / s_scan %.0f GB/s  " \
                   "rows_out %d passes %d | yardstick (export, numpy join, import_pairs_device) %.0f ms = %.0f x" % (
                       op, med(wall), 1e3 * s_scan, s_scan / floor, info["rows_a"] / s_scan / 1e6,
                       hist["slots"] * 16 / s_scan / 1e9, info["rows_out"], info["passes"], 1e3 * t_yard,
                       t_yard / statistics.median(wall))
            if genome <= args.tsv_upto and op == "only":
                t0 = time.perf_counter()
                by_export("tsv")
                t_tsv = time.perf_counter() - t0
                yk, yc = yard.export()
                assert np.array_equal(yk, got_k) and np.array_equal(yc, got_c)
                line += " (back through load_tsv instead: %.0f ms)" % (1e3 * t_tsv)
            print(line, flush=True)
            ratio = t_yard / max(wall)
            worst = ratio if worst is None else min(worst, ratio)
            assert max(wall) < t_yard, "combine is not faster than the yardstick (%s)" % op
        print("  every op faster than the yardstick; smallest yardstick / slowest run: %.0f x" % worst, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="500000,5000000", help="genome lengths of the synthetic samples (about 2 rows per base)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--tsv_upto", type=int, default=500000, help="largest genome at which the way back through load_tsv is timed too")
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0))
    copy_gbs = stream_copy_gbs(torch)
    for genome in [int(x) for x in args.genome.split(",")]:
        probe(torch, genome, args, copy_gbs)


if __name__ == "__main__":
    main()
