"""reads and one long record cut at their first low-abundance k-mer (Counter.trim), k = 31, with the route
there was before and the yardsticks in the same process, interleaved with the timed runs: (a) the parent's only route --
Counter.track(sat32=True), the first low count of every record with numpy, the text sliced in Python -- compared in every
run for equal bytes; (b) Counter.screen on the same text, whose s_probe is the same walk with the row sink; (c)
Counter.filter keeping every record with a k-mer, whose s_gather moves whole records.  The texts come from seeds.  Two
warm-ups, then median (min-max) of the runs.

    python tools/trimreads_probe.py [--reads 1000000] [--long 100000000] [--runs 5]

Pass mark: Counter.trim is faster end to end than the track route on both read texts (asserted).
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
FIELDS = ("s_read", "s_parse", "s_probe", "s_place", "s_first", "s_gather", "s_write", "s_total", "wall")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-22s %-9s %10.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def substitute(text: np.ndarray, at: np.ndarray) -> np.ndarray:
    """The text with the bases at the given positions replaced by the next of A, C, G, T."""
    out = text.copy()
    code = np.zeros(256, dtype=np.uint8)
    code[ACGT] = np.arange(4, dtype=np.uint8)
    out[at] = ACGT[(code[text[at]] + 1) & 3]
    return out


def track_route(ctx, text, at_least):
    """What a user could do before: every count to the host, the first low one of every record with numpy, the text
    sliced in Python.  (Records of one header line and one sequence line, as synth_reads writes them.)"""
    t0 = time.perf_counter()
    counts, offsets, _, _ = ctx.track(text, at_least, sat32=True)
    offsets = offsets.astype(np.int64)
    windows = np.diff(offsets)
    idx = np.flatnonzero(counts < at_least)
    rec = np.searchsorted(offsets, idx, side="right") - 1
    first = np.full(len(windows), -1, dtype=np.int64)
    uniq, pos = np.unique(rec, return_index=True)  # (idx ascends: the first of a record is its first low window)
    first[uniq] = idx[pos] - offsets[uniq]
    kept = np.where(first < 0, windows + K - 1, np.where(first > 0, first + K - 1, 0))
    kept[(windows == 0) | (kept < K)] = 0
    lines = bytes(text).split(b"\n")
    out = b"".join(lines[2 * i] + b"\n" + lines[2 * i + 1][:n] + b"\n" for i, n in enumerate(kept.tolist()) if n)
    return out, kept, time.perf_counter() - t0


def shape(label, ctx, text, at_least, runs, pass_mark):
    print("  %s, %.0f MB of text, at_least %d" % (label, len(text) / 1e6, at_least), flush=True)
    trm, scr, flt, old = [], [], [], []
    for i in range(2 + runs):
        info = {}
        t0 = time.perf_counter()
        out, kept, rows = ctx.trim(text, at_least, info=info)
        info["wall"] = time.perf_counter() - t0
        want, want_kept, sec = track_route(ctx, text, at_least)
        assert out == want and kept.tolist() == want_kept.tolist(), "trim differs from the track route"
        s_info, f_info = {}, {}
        ctx.screen(text, at_least, info=s_info)
        ctx.filter(text, 1, info=f_info)
        if i >= 2:
            trm.append(info)
            scr.append(s_info)
            flt.append(f_info)
            old.append(sec)
        del out, kept, rows, want
    f = trm[0]
    print("    Counter.trim: %d records, %d emitted, %d of them cut, %d dropped; %d of %d bases, %d bytes out, %d piece(s)" % (
        f["records"], f["records_out"], f["records_trimmed"], f["records_dropped"], f["bases_out"], f["bases_in"], f["bytes_out"],
        f["pieces"]), flush=True)
    m = {field: line("Counter.trim", field, [i[field] for i in trm]) for field in FIELDS}
    route = line("track route", "wall", old)
    probe = [i["s_probe"] for i in scr]
    line("Counter.screen", "s_probe", probe)
    gather = line("Counter.filter", "s_gather", [i["s_gather"] for i in flt], " for %d bytes" % flt[0]["bytes_out"])
    print("    track route / trim (wall) = %.1f" % (route / m["wall"]), flush=True)
    if m["s_first"]:
        print("    s_first = %.2f x screen's s_probe (its highest: %.3f ms)%s" % (
            m["s_first"] / statistics.median(probe), 1e3 * max(probe), "  ABOVE IT" if m["s_first"] > max(probe) else ""), flush=True)
    else:
        print("    s_first = 0: every window a hit, the first-low walk is skipped", flush=True)
    if f["bytes_out"] and flt[0]["bytes_out"]:
        print("    s_gather: %.1f GB/s of output (the filter's gather: %.1f GB/s)" % (
            f["bytes_out"] / m["s_gather"] / 1e9, flt[0]["bytes_out"] / gather / 1e9), flush=True)
    if pass_mark:
        assert m["wall"] < route, "the pass mark: trim is faster end to end than the track route"
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    rng = np.random.default_rng(11)
    if args.reads:
        clean = native.synth_reads(1_000_000, 3, args.reads, READ, 4)
        bases = np.flatnonzero(np.isin(clean, ACGT))
        reads = substitute(clean, rng.choice(bases, len(bases) // 100, replace=False))
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(clean, 1)
            shape("%d x %d bp reads, 1 %% substitutions, against the table of the error-free reads" % (args.reads, READ), ctx, reads, 2,
                  args.runs, True)
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(reads, 1)
            shape("the same reads against their own table: nothing is low", ctx, reads, 1, args.runs, True)
    if args.long:
        genome = ACGT[rng.integers(0, 4, args.long)]
        clean = np.concatenate([np.frombuffer(b">g\n", dtype=np.uint8), genome, np.frombuffer(b"\n", dtype=np.uint8)])
        # a substitution every 1550 bases takes 31 windows each: 2 % of them; the first stands behind the first window
        text = substitute(clean, 3 + np.arange(1000, args.long, 1550))
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(clean, 1)
            some = shape("one %d-base record, 2 %% of its windows low" % args.long, ctx, text, 1, args.runs, False)
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(b">x\n" + b"ACGTTGCAGGATCCATGAACGTACGGTCAGTTGACCA" * 4 + b"\n", 1)
            every = shape("the same record, every window low (the contention shape)", ctx, text, 1, args.runs, False)
        print("  s_first, every window low / 2 %% low = %.2f" % (every["s_first"] / some["s_first"]), flush=True)


if __name__ == "__main__":
    main()
