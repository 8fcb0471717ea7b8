"""the counts under reads and under one long record (Counter.track), k = 31, with their yardsticks in the same
process, interleaved with the timed runs: (a) the route there was before -- every window materialised on the host as k
bytes and looked up with Counter.lookup -- run once per shape where it is asked for, its values compared each time;
(b) Counter.screen on the same text, whose s_probe is the same walk without the positional sink; (c) a device-to-device
copy of windows_out x element size bytes, the floor of the track kernel's writes.  The texts come from seeds.  Two
warm-ups, then median (min-max) of the runs.

    python tools/track_probe.py [--pass-reads 100000] [--reads 1000000] [--long 100000000] [--runs 5] [--long-median-runs 1]

Another build of the library (mercat2_amd/csrc/Makefile: OBJDIR=... LIB=../libmercat_hip_ab.so) is probed with
MERCAT_HIP_LIB pointing at it, alternately with the library.
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
FIELDS = ("s_read", "s_parse", "s_probe", "s_place", "s_track", "s_median", "s_write", "s_total", "wall")


def copy_seconds(torch, nbytes):
    """One device-to-device copy of nbytes (hipMemcpyAsync), timed by events."""
    if not nbytes:
        return 0.0
    src = copy_seconds.buf.setdefault(("s", nbytes), torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(65))
    dst = copy_seconds.buf.setdefault(("d", nbytes), torch.empty(nbytes, dtype=torch.uint8, device="cuda"))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    dst.copy_(src)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


copy_seconds.buf = {}


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-22s %-9s %10.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def lookup_route(ctx, text):
    """What a user could do before: the windows of every read as k bytes each, built on the host, through Counter.lookup.
    (Reads of one length on one line each, as synth_reads writes them.)  Returns (counts, seconds)."""
    t0 = time.perf_counter()
    seqs = bytes(text).split(b"\n")[1::2]
    reads = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), -1)
    windows = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(reads, K, axis=1))
    counts = ctx.lookup(windows.reshape(-1, K))
    return counts, time.perf_counter() - t0


def shape(torch, label, ctx, text, runs, median, yardstick=False):
    print("  %s, %.0f MB of text%s" % (label, len(text) / 1e6, ", with the median" if median else ""), flush=True)
    want = None
    if yardstick:
        want, sec = lookup_route(ctx, text)
        print("    %-22s %-9s %10.3f ms (1 run): %d windows as %d bytes each on the host, then Counter.lookup" % (
            "lookup route", "wall", 1e3 * sec, len(want), K), flush=True)
    got = {}
    for sat32 in (False, True):
        name = "Counter.track sat32" if sat32 else "Counter.track u64"
        trk, scr, copies = [], [], []
        for i in range(2 + runs):
            info = {}
            t0 = time.perf_counter()
            counts, offsets, rows, med = ctx.track(text, 1, sat32=sat32, median=median, info=info)
            info["wall"] = time.perf_counter() - t0
            if want is not None:
                assert len(counts) == len(want) and (counts == want).all(), "track differs from the lookup route"
            s_info = {}
            ctx.screen(text, 1, info=s_info)
            c = copy_seconds(torch, info["windows_out"] * counts.itemsize)
            if i >= 2:
                trk.append(info)
                scr.append(s_info)
                copies.append(c)
            del counts, offsets, rows, med
        f = trk[0]
        print("    %s: %d records, %d windows, %d saturated, %d piece(s)" % (name, f["records"], f["windows_out"], f["saturated"], f["pieces"]),
              flush=True)
        m = {field: line(name, field, [i[field] for i in trk]) for field in FIELDS}
        probe = line("Counter.screen", "s_probe", [i["s_probe"] for i in scr])
        c = line("D2D copy", "counts", copies)
        nbytes = f["windows_out"] * (4 if sat32 else 8)
        print("    s_track = %.2f x screen's s_probe, %.2f x the copy; %.1f Gwindows/s, %.0f GB/s written (the copy: %.0f GB/s)" % (
            m["s_track"] / probe, m["s_track"] / c, f["windows_out"] / m["s_track"] / 1e9, nbytes / m["s_track"] / 1e9, nbytes / c / 1e9),
            flush=True)
        if want is not None:
            print("    lookup route / track (wall) = %.1f" % (sec / m["wall"]), flush=True)
            assert m["wall"] < sec, "the pass mark: track is faster end to end than the lookup route"
        got[sat32] = m
    print("    sat32 / u64: s_write %.2f, s_track %.2f, wall %.2f" % tuple(got[True][f] / got[False][f] for f in ("s_write", "s_track", "wall")),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pass-reads", type=int, default=100_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--long-median-runs", type=int, default=1, help="timed runs of the median over the long record (0: skip)")
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    if args.pass_reads:
        text = native.synth_reads(1_000_000, 3, args.pass_reads, READ, 4)
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(text, 1)
            shape(torch, "%d x %d bp reads against their own table" % (args.pass_reads, READ), ctx, text, args.runs, False, yardstick=True)
    if args.reads:
        text = native.synth_reads(1_000_000, 3, args.reads, READ, 4)
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(text, 1)
            shape(torch, "%d x %d bp reads against their own table" % (args.reads, READ), ctx, text, args.runs, False)
            shape(torch, "%d x %d bp reads against their own table" % (args.reads, READ), ctx, text, args.runs, True)
    if args.long:
        rng = np.random.default_rng(11)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, args.long)]
        text = np.concatenate([np.frombuffer(b">g\n", dtype=np.uint8), genome, np.frombuffer(b"\n", dtype=np.uint8)])
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(text[: 3 + 2_000_000 + 1], 1)
            shape(torch, "one %d-base record, a table of its first 2 Mbases" % args.long, ctx, text, args.runs, False)
            if args.long_median_runs:
                for sat32 in (False, True):  # one segment of the segmented sort
                    for i in range(args.long_median_runs):
                        info = {}
                        t0 = time.perf_counter()
                        med = ctx.track(text, 1, sat32=sat32, median=True, info=info)[3]
                        print("    median of the one record (%s): s_median %10.3f ms, wall %.3f s, median %d" % (
                            "sat32" if sat32 else "u64", 1e3 * info["s_median"], time.perf_counter() - t0, int(med[0])), flush=True)


if __name__ == "__main__":
    main()
