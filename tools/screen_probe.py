"""reads and one long record screened against tables on the GPU (Counter.screen) against the fastest way to the
same rows without mk_screen -- every window cut on the host, k bytes a base pushed through Counter.lookup, the per-record
reduction in numpy -- in one process, on the same tables.  Warm-ups first, then median (min-max).

    python tools/screen_probe.py [--reads 1000000] [--long 100000000] [--runs 5] [--no-yardstick]
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
READ = 150


def screen_runs(ctx, text, runs):
    """[info of every timed run], rows of the last one."""
    infos, rows = [], None
    for i in range(2 + runs):
        info = {}
        t0 = time.perf_counter()
        rows = ctx.screen(text, info=info)
        info["wall"] = time.perf_counter() - t0
        if i >= 2:
            infos.append(info)
    return infos, rows


def med(infos, field):
    v = [i[field] for i in infos]
    return statistics.median(v), min(v), max(v)


def report(label, infos):
    w = infos[0]["windows"]
    for field in ("s_parse", "s_probe", "s_total", "wall"):
        m, lo, hi = med(infos, field)
        print("    %-34s %-8s %9.2f ms (%.2f-%.2f, %d runs)" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(infos)), flush=True)
    print("    %-34s %.0f M windows/s by s_probe, %.0f M windows/s by s_total; %d pieces, hits %d of %d" % (
        label, w / med(infos, "s_probe")[0] / 1e6, w / med(infos, "s_total")[0] / 1e6, infos[0]["pieces"], infos[0]["hits"], w), flush=True)
    return med(infos, "s_total")[0]


def reads_by_lookup(ctx, data, n_reads, slab=100_000):
    """The parent commit's route for reads of one length: windows cut on the host, Counter.lookup, numpy per read."""
    nl = np.flatnonzero(data == 10)
    starts = nl[0::2] + 1
    out = np.zeros((n_reads, 5), dtype=np.uint64)
    per = READ - K + 1
    for a in range(0, n_reads, slab):
        s = starts[a:a + slab]
        seqs = data[s[:, None] + np.arange(READ)]
        keys = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(seqs, K, axis=1)).reshape(-1, K)
        c = ctx.lookup(keys).reshape(len(s), per)
        out[a:a + len(s)] = np.stack([np.full(len(s), per, dtype=np.uint64), (c >= 1).sum(1).astype(np.uint64), c.sum(1), c.min(1), c.max(1)], 1)
    return out


def long_by_lookup(ctx, seq, slab=10_000_000):
    total = len(seq) - K + 1
    hits = sums = 0
    mn, mx = np.uint64(2**64 - 1), np.uint64(0)
    for a in range(0, total, slab):
        n = min(slab, total - a)
        keys = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(seq[a:a + n + K - 1], K))
        c = ctx.lookup(keys)
        hits += int((c >= 1).sum())
        sums += int(c.sum())
        mn, mx = min(mn, c.min()), max(mx, c.max())
    return np.array([[total, hits, sums % (1 << 64), mn, mx]], dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    reads = native.synth_reads(1_000_000, 3, args.reads, READ, 4)
    rng = np.random.default_rng(11)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, args.long)]
    long_text = np.concatenate([np.frombuffer(b">g\n", dtype=np.uint8), genome, np.frombuffer(b"\n", dtype=np.uint8)])
    other = native.synth_reads(5_000_000, 9, 400_000, READ, 10)  # about two rows a genome base: the 10 M-row table
    own = native.Counter(K, native.ALPHABET_NT2)
    big = native.Counter(K, native.ALPHABET_NT2)
    own.count_chunk(reads, 1)
    big.count_chunk(other, 1)
    big.count_chunk(long_text[: 3 + 2_000_000 + 1], 1)  # (and the head of the long record: hits and misses there too)
    for name, ctx in (("own table", own), ("10 M-row table", big)):
        print("%s: %d rows" % (name, ctx.rows()), flush=True)
        for what, text in (("%d x %d bp reads" % (args.reads, READ), reads), ("one %d-base record" % args.long, long_text)):
            print("  %s, %.0f MB of text" % (what, len(text) / 1e6), flush=True)
            infos, rows = screen_runs(ctx, text, args.runs)
            t_screen = report("Counter.screen", infos)
            if args.no_yardstick:
                continue
            t0 = time.perf_counter()
            want = reads_by_lookup(ctx, reads, args.reads) if text is reads else long_by_lookup(ctx, genome)
            t_yard = time.perf_counter() - t0
            assert (rows == want).all(), "the two routes differ"
            print("    %-34s %9.2f ms (1 run); the rows agree; screen is %.1fx faster (s_total)" % (
                "windows on the host + Counter.lookup", 1e3 * t_yard, t_yard / t_screen), flush=True)
    own.close()
    big.close()


if __name__ == "__main__":
    main()
