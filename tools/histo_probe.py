"""the abundance histogram of a table on the GPU (Counter.histo / histo_device) against the way to the same
numbers without mk_histo -- Counter.export() + np.bincount(np.minimum(counts, high + 1)) -- and beside the wall time of
Counter.alpha_stats(), which reads the same slots, in one process, on one table.  Warm-ups first, then median (min-max).

    python tools/histo_probe.py [--genome 500000,5000000] [--high 10000] [--runs 7]

Tables: synth_reads at k = 31, -c 1 (about 2 rows per base: a spectrum spread around the coverage), and one of as many
rows as the last of them in which every k-mer occurs once (the windows of one random sequence): every lane of every
wave adds to bin 1, the worst case for the bins in LDS.
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


def timed(fn, warmups, runs):
    for _ in range(warmups):
        fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def show(label, times, extra=""):
    print("  %-58s %9.3f ms (%.3f-%.3f, %d runs)%s" % (label, 1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times),
                                                      len(times), extra), flush=True)
    return statistics.median(times)


def stream_copy_gbs(torch):
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)

    def copy():
        b.copy_(a)
        torch.cuda.synchronize()
    t = statistics.median(timed(copy, 2, 7))
    return 2 * a.numel() / t / 1e9


def singletons(rows: int) -> bytes:
    """One record whose `rows` windows of K bases are (as good as surely) all different."""
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(11).integers(0, 4, rows + K - 1)]
    return b">r\n" + bases.tobytes() + b"\n"


def probe(torch, name, data, args, copy_gbs):
    high = args.high
    with native.Counter(K, native.ALPHABET_NT2) as ctx:
        ctx.count_chunk(data, 1)
        del data
        rows = ctx.rows()
        answers, info, dev_info = {}, {}, {}
        d_out = torch.zeros(high + 2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def by_export():
            _, counts = ctx.export()
            answers["export"] = np.bincount(np.minimum(counts, np.uint64(high + 1)).astype(np.int64), minlength=high + 2)

        def by_histo():
            answers["histo"] = ctx.histo(high, info=info)

        scans = []

        def by_device():
            dev_info.update(ctx.histo_device(high, d_out.data_ptr()))
            scans.append(dev_info["s_scan"])

        by_histo()
        print("%s: %d rows in %d slots of 16 B (k = %d, -c 1); bins 1..5: %s; max count %d" % (
            name, rows, info["slots"], K, answers["histo"][1:6].tolist(), info["max_count"]), flush=True)
        t_d = show("Counter.histo_device", timed(by_device, 2, args.runs))
        s_scan = show("scan kernel(s), s_scan", scans[2:])
        print("    slots x 16 B / s_scan = %.0f GB/s (device-to-device copy, read + write: %.0f GB/s)" % (
            info["slots"] * 16 / s_scan / 1e9, copy_gbs))
        assert (d_out.cpu().numpy().view(np.uint64) == answers["histo"]).all()
        t_h = show("Counter.histo, host array", timed(by_histo, 2, args.runs))
        show("Counter.alpha_stats (reads the same slots)", timed(ctx.alpha_stats, 2, args.runs))
        yard = show("yardstick: export() + np.bincount", timed(by_export, 2, args.runs))
        assert (answers["export"].astype(np.uint64) == answers["histo"]).all() and int(answers["histo"].sum()) == rows
        print("  answers agree; yardstick / route: histo %.0fx, histo_device %.0fx" % (yard / t_h, yard / t_d))
        assert t_h < yard and t_d < yard, "a route is slower than the yardstick"
        return s_scan, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="500000,5000000", help="genome lengths of the synthetic samples (about 2 rows per base)")
    ap.add_argument("--high", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0))
    copy_gbs = stream_copy_gbs(torch)
    print("device-to-device copy of 1 GiB (read + write): %.0f GB/s" % copy_gbs)
    rows = s_spread = 0
    for genome in [int(x) for x in args.genome.split(",")]:
        data = native.synth_reads(genome, 3, genome // 10, 150, 4)
        s_spread, rows = probe(torch, "synth_reads, genome %d" % genome, data, args, copy_gbs)
        del data
    s_single, _ = probe(torch, "all singletons", singletons(rows), args, copy_gbs)
    print("s_scan, all singletons / spread table of the same size: %.3f" % (s_single / s_spread))


if __name__ == "__main__":
    main()
