"""six-frame ORFs of reads, of one long record and of five genome-sized samples (Counter.orfs), with the only
alternative a user has inside this project -- the rule itself in plain Python, tests/orf_rule.py -- in the same process.
The texts come from seeds.  Two warm-ups, then the median (min-max) of the runs, the legs (text x mode) alternating.

The Python rule takes about a second a megabase, so it runs on a slice of every text (--slice bytes, cut at a record's
start; the whole text where it is shorter): Counter.orfs of that same slice is timed beside it, both outputs are compared
in every run, and the pass mark is asserted there.  The whole texts give the sections' times.

    python tools/orf_probe.py [--reads 1000000] [--long 100000000] [--genomes 5] [--runs 5] [--slice 1000000]

Pass mark: Counter.orfs is faster end to end than tests/orf_rule.py on the same text (asserted, every text and mode).
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from mercat2_amd import native  # noqa: E402
import orf_rule  # noqa: E402

READ = 150
SPAN = 256 * 48  # OR_SPAN
HBM = 8.0e12     # bytes a second, MI355X peak
FIELDS = ("s_read", "s_parse", "s_find", "s_place", "s_emit", "s_write", "s_total", "wall")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MODES = (("stop", dict()), ("start", dict(start=True)))


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-14s %-8s %10.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def reads_text(rng, n: int) -> bytes:
    rec = np.empty((n, 1 + 8 + 1 + READ + 1), dtype=np.uint8)
    rec[:, 0] = ord(">")
    idx = np.arange(n)
    for d in range(8):
        rec[:, 8 - d] = 48 + (idx // 10 ** d) % 10
    rec[:, 9] = 10
    rec[:, 10:10 + READ] = ACGT[rng.integers(0, 4, (n, READ))]
    rec[:, 10 + READ] = 10
    return rec.tobytes()


def genome_text(rng, name: str, size: int, contigs: int) -> bytes:
    """``contigs`` records of together ``size`` bases, wrapped at 60 columns as the reference's genomes are."""
    out = []
    for c in range(contigs):
        seq = ACGT[rng.integers(0, 4, size // contigs)].tobytes()
        out.append(b">%s_%d\n" % (name.encode(), c + 1) + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
    return b"".join(out)


def head_of(text: bytes, limit: int) -> bytes:
    if len(text) <= limit:
        return text
    cut = text.find(b"\n>", limit // 2)
    return text[:cut + 1] if 0 <= cut < limit else text[:limit]  # (one long record: its first bytes are a record too)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000_000)
    ap.add_argument("--genomes", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--slice", type=int, default=1_000_000)
    ap.add_argument("--min_aa", type=int, default=32)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    rng = np.random.default_rng(29)
    texts = []
    if args.reads:
        texts.append(("%d x %d-base reads" % (args.reads, READ), reads_text(rng, args.reads)))
    if args.long:
        texts.append(("one %d-base record" % args.long, b">g\n" + ACGT[rng.integers(0, 4, args.long)].tobytes() + b"\n"))
    sizes = (2_960_000, 313_000, 3_079_000, 3_000_000, 3_100_000)  # the reference's 5-genomes samples are of this order
    for g in range(args.genomes):
        texts.append(("genome %d, %d bases in 20 contigs, wrapped" % (g + 1, sizes[g % 5]), genome_text(rng, "g%d" % (g + 1), sizes[g % 5], 20)))
    legs = [(label, text, head_of(text, args.slice), name, mode) for label, text in texts for name, mode in MODES]
    runs = {i: dict(whole=[], part=[], rule=[]) for i in range(len(legs))}
    with native.Counter(5, native.ALPHABET_NT2) as ctx:
        for rep in range(2 + args.runs):
            for i, (label, text, part, name, mode) in enumerate(legs):
                info = {}
                t0 = time.perf_counter()
                out, rows = ctx.orfs(text, min_aa=args.min_aa, info=info, **mode)
                info["wall"] = time.perf_counter() - t0
                assert info["bytes_out"] == len(out) and info["orfs"] == len(rows) and info["residues"] == int(rows[:, 2].sum())
                t0 = time.perf_counter()
                p_out, p_rows = ctx.orfs(part, min_aa=args.min_aa, **mode)
                p_wall = time.perf_counter() - t0
                if rep >= 2:
                    t0 = time.perf_counter()
                    want, w_rows = orf_rule.expected(part, args.min_aa, **mode)
                    r_wall = time.perf_counter() - t0
                    assert p_out == want and p_rows.tolist() == w_rows, "Counter.orfs differs from the rule: " + label
                    runs[i]["whole"].append(info)
                    runs[i]["part"].append(p_wall)
                    runs[i]["rule"].append(r_wall)
                del out, rows, p_out, p_rows
    for i, (label, text, part, name, mode) in enumerate(legs):
        f = runs[i]["whole"][0]
        n = f["bases"] + f["records"]  # the stream
        print("  %s, %s mode, min_aa %d: %.1f MB of text, %d records, %d ORFs, %d residues, %d bytes out, %d piece(s)" % (
            label, name, args.min_aa, len(text) / 1e6, f["records"], f["orfs"], f["residues"], f["bytes_out"], f["pieces"]), flush=True)
        m = {field: line("Counter.orfs", field, [r[field] for r in runs[i]["whole"]]) for field in FIELDS}
        # bytes from the shapes: the scan reads the stream three times (tile summaries, count, rows), writes 4 bytes a
        # lane and 32 a row; the gather reads 3 stream bytes a residue (cached) and writes the output
        find = 3 * n + 4 * (n // 48) + 32 * f["orfs"]
        print("    s_find  %.2f x s_parse; %.1f GB/s of %d bytes moved (%.1f %% of HBM peak: not bandwidth-bound)" % (
            m["s_find"] / m["s_parse"], find / m["s_find"] / 1e9, find, 100 * find / m["s_find"] / HBM), flush=True)
        emit = 3 * f["residues"] + f["bytes_out"]
        if m["s_emit"]:
            print("    s_emit  %.2f x s_parse; %.1f GB/s of output, %.1f GB/s of %d bytes moved (%.1f %% of HBM peak)" % (
                m["s_emit"] / m["s_parse"], f["bytes_out"] / m["s_emit"] / 1e9, emit / m["s_emit"] / 1e9, emit, 100 * emit / m["s_emit"] / HBM), flush=True)
        print("    s_find + s_place + s_emit = %.2f x s_parse" % ((m["s_find"] + m["s_place"] + m["s_emit"]) / m["s_parse"]), flush=True)
        gpu = line("Counter.orfs", "slice", runs[i]["part"], " for %.1f MB" % (len(part) / 1e6))
        cpu = line("orf_rule.py", "slice", runs[i]["rule"])
        print("    rule / Counter.orfs (wall, the slice) = %.0f" % (cpu / gpu), flush=True)
        assert gpu < cpu, "the pass mark: Counter.orfs is faster end to end than the rule in Python"


if __name__ == "__main__":
    main()
