"""adapter removal on the device (Counter.fastq_adapt_device) on synthetic 150 bp FASTQ reads held in HBM, with
panels of 1, 3 and 376 adapters, beside Counter.fastq_select_device keeping every record of the same text in the same
session -- that call runs the line index and the gather without the scan, so the difference is what the adapter search
costs.  A seeded share of the reads carries a TruSeq read-through at a random offset: the adapter, then random bases to
the end of the read.  s_scan is also given as position x adapter-word compares per second: a candidate position of a
read (those up to its hit, or all L - min_overlap + 1 without one) against 32 bases of one adapter.  Two warm-ups, then
median (min-max) of the runs.

    python tools/adapt_probe.py [--reads 10000000] [--runs 5] [--share 0.3]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mercat2_amd import native  # noqa: E402

READ = 150
MIN_OVERLAP = 8
TRUSEQ = native.ILLUMINA_ADAPTERS[0][1].encode()


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-34s %-9s %9.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def reads_text(n: int, seed: int, share: float) -> bytes:
    """n records '@r\\n' + 150 bases + '\\n+\\n' + 150 qualities + '\\n', built as one array (no Python loop over reads);
    `share` of them have the TruSeq adapter written over their bases from a random offset on (cut off by the read's end)."""
    if n > 1_000_000:  # (a million distinct reads, repeated)
        block = reads_text(1_000_000, seed, share)
        return block * (n // 1_000_000) + block[: (n % 1_000_000) * (len(block) // 1_000_000)]
    rng = np.random.default_rng(seed)
    rec = np.empty((n, 3 + READ + 3 + READ + 1), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, READ), dtype=np.uint8)]
    carries = rng.random(n) < share
    offset = rng.integers(0, READ - MIN_OVERLAP + 1, n)
    adapter = np.frombuffer(TRUSEQ, np.uint8)
    for j in range(len(adapter)):  # (a loop over the adapter's 13 bases, not over reads)
        col = offset + j
        rows = np.nonzero(carries & (col < READ))[0]
        seq[rows, col[rows]] = adapter[j]
    rec[:, 3:3 + READ] = seq
    rec[:, 3 + READ:6 + READ] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + READ:6 + 2 * READ] = ord("I")
    rec[:, -1] = 10
    return rec.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.3)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    n = args.reads
    raw = reads_text(n, 7, args.share)
    rng = np.random.default_rng(376)
    random_panel = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(m))) for m in rng.integers(18, 70, 375)]
    panels = [("1 adapter", [TRUSEQ]), ("3 adapters", [s.encode() for _, s in native.ILLUMINA_ADAPTERS]),
              ("376 adapters", random_panel + [TRUSEQ])]
    d_text = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8)).cuda()
    d_out = torch.empty(len(raw) + 1, dtype=torch.uint8, device="cuda")
    d_keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_rows = torch.empty((n, 5), dtype=torch.int64, device="cuda")
    d_hits = torch.empty(376, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    print("  %d x %d bp reads, %.0f MB of FASTQ in HBM, %.0f %% with a TruSeq read-through, min_overlap %d, max_err 0.1" % (
        n, READ, len(raw) / 1e6, 100 * args.share, MIN_OVERLAP), flush=True)
    with native.Counter(5, native.ALPHABET_NT2) as ctx:
        sel = []
        for label, panel in panels:
            runs = []
            for i in range(2 + args.runs):
                t = ctx.fastq_adapt_device(d_text.data_ptr(), len(raw), d_out.data_ptr(), len(raw) + 1, panel, None, n, d_keep.data_ptr(),
                                           d_rows.data_ptr(), d_hits.data_ptr(), min_overlap=MIN_OVERLAP)
                s = ctx.fastq_select_device(d_text.data_ptr(), len(raw), d_out.data_ptr(), len(raw) + 1, n)
                if i >= 2:
                    runs.append(t)
                    sel.append(s)
            t = runs[0]
            hit = d_rows[:, 2] != native.ADAPT_NO_HIT
            positions = int(torch.where(hit, d_rows[:, 1] + 1, torch.clamp(d_rows[:, 0] - MIN_OVERLAP + 1, min=0)).sum().item())
            words = sum((len(a) + 31) // 32 for a in panel if len(a) >= MIN_OVERLAP)
            print("  %s (%d words of 32 bases): %d records, %d with a hit, %d emitted (%d of them cut), %d of %d bases, %d bytes out" % (
                label, words, t["records"], int(hit.sum().item()), t["records_out"], t["records_trimmed"], t["bases_out"], t["bases_in"],
                t["bytes_out"]), flush=True)
            got = {f: line("Counter.fastq_adapt_device", f, [r[f] for r in runs]) for f in ("s_index", "s_scan", "s_place", "s_gather")}
            print("    scan: %d positions x %d adapter words = %.3g compares, %.3g a second; %.2f ns a read" % (
                positions, words, positions * words, positions * words / got["s_scan"], 1e9 * got["s_scan"] / n), flush=True)
        print("  the same text, every record kept (%d bytes out)" % sel[0]["bytes_out"], flush=True)
        for f in ("s_index", "s_place", "s_gather"):
            line("Counter.fastq_select_device", f, [r[f] for r in sel])


if __name__ == "__main__":
    main()
