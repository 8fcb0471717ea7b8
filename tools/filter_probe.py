"""reads and one long record filtered against tables on the GPU (Counter.filter), with two yardsticks in the
same process, interleaved with the timed runs: (a) a device-to-device copy of bytes_out bytes, the floor of the gather;
(b) Counter.screen on the same text, whose s_parse and s_probe are the same code.  The texts come from seeds.  Two
warm-ups, then median (min-max) of the runs.

    python tools/filter_probe.py [--reads 1000000] [--long 100000000] [--runs 5]
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
FIELDS = ("s_read", "s_parse", "s_probe", "s_place", "s_gather", "s_write", "s_total", "wall")


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


def med(values):
    return statistics.median(values), min(values), max(values)


def line(label, field, values, extra=""):
    m, lo, hi = med(values)
    print("    %-16s %-9s %9.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def shape(torch, label, ctx, text, rule, invert, runs):
    print("  %s, %.0f MB of text" % (label, len(text) / 1e6), flush=True)
    filt, scr, copies, out = [], [], [], b""
    for i in range(2 + runs):
        info = {}
        t0 = time.perf_counter()
        out, keep, _ = ctx.filter(text, *rule, invert=invert, info=info)
        info["wall"] = time.perf_counter() - t0
        s_info = {}
        t0 = time.perf_counter()
        ctx.screen(text, rule[0], info=s_info)
        s_info["wall"] = time.perf_counter() - t0
        c = copy_seconds(torch, info["bytes_out"])
        if i >= 2:
            filt.append(info)
            scr.append(s_info)
            copies.append(c)
    f = filt[0]
    print("    %d records, %d kept, %d of %d bytes out, preamble %d, %d piece(s)" % (
        f["records"], f["records_out"], f["bytes_out"], len(text), f["preamble"], f["pieces"]), flush=True)
    got = {}
    for field in FIELDS:
        got[field] = line("Counter.filter", field, [i[field] for i in filt])
    for field in ("s_parse", "s_probe", "s_total"):
        m = line("Counter.screen", field, [i[field] for i in scr])
        if field != "s_total":
            print("    %-16s %-9s filter / screen = %.3f" % ("", field, got[field] / m if m else float("nan")), flush=True)
    if f["bytes_out"]:
        c = line("D2D copy", "bytes_out", copies)
        print("    gather = %.2f x the copy; %.0f GB/s written by the gather, %.0f GB/s by the copy" % (
            got["s_gather"] / c, f["bytes_out"] / got["s_gather"] / 1e9, f["bytes_out"] / c / 1e9), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    # reads of two genomes, record by record in turn: a table of the first genome's reads holds every other record
    mine = native.synth_reads(1_000_000, 3, args.reads // 2, READ, 4).tobytes()
    theirs = native.synth_reads(1_000_000, 5, args.reads - args.reads // 2, READ, 6).tobytes()
    text = b"".join(b">" + a + b">" + b for a, b in zip(mine.split(b">")[1:], theirs.split(b">")[1:]))
    reads = np.frombuffer(text, dtype=np.uint8)
    rng = np.random.default_rng(11)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, args.long)]
    long_text = np.concatenate([np.frombuffer(b">g\n", dtype=np.uint8), genome, np.frombuffer(b"\n", dtype=np.uint8)])
    with native.Counter(K, native.ALPHABET_NT2) as one_genome, native.Counter(K, native.ALPHABET_NT2) as own, \
            native.Counter(K, native.ALPHABET_NT2) as head:
        one_genome.count_chunk(mine, 1)
        own.count_chunk(reads, 1)
        head.count_chunk(long_text[: 3 + 2_000_000 + 1], 1)
        every = (1, 1, 1_000_000)  # every k-mer of the read is in the table
        what = "%d x %d bp reads" % (args.reads, READ)
        out = shape(torch, what + ", a table that holds every other read", one_genome, reads, every, False, args.runs)
        assert out == mine, "the reads the table was counted from, and only they, are kept"
        out = shape(torch, what + ", everything kept", own, reads, every, False, args.runs)
        assert out == text
        out = shape(torch, what + ", nothing kept", own, reads, every, True, args.runs)
        assert out == b""
        out = shape(torch, "one %d-base record, kept" % args.long, head, long_text, (1, 1, 0), False, args.runs)
        assert out == long_text.tobytes()


if __name__ == "__main__":
    main()
