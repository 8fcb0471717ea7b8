"""a keep / kept decision applied to the FASTQ text it was taken for (Counter.fastq_select), beside the FASTA
gather it is modelled on, in the same process and interleaved with it: Counter.filter on the fq2fa form of the same
reads gives keep[] (about half kept) and its own s_gather; Counter.fastq_select writes the same reads from the raw
FASTQ text.  Then the same with a kept[] that cuts a third of the reads.  The reads come from seeds.  Two warm-ups,
then median (min-max) of the runs.

    python tools/fqselect_probe.py [--reads 1000000] [--runs 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mercat2_amd import native  # noqa: E402

K = 31
READ = 150
FIELDS = ("s_copy", "s_index", "s_place", "s_gather", "s_write")


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-22s %-9s %9.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def fastq_of(fasta: bytes, seed: int) -> bytes:
    """The one-line FASTA records as FASTQ records with seeded qualities ('!' + 0..40)."""
    lines = fasta.split(b"\n")[:-1]
    n = len(lines) // 2
    qual = (np.random.default_rng(seed).integers(33, 74, (n, READ), dtype=np.uint8)).tobytes()
    return b"".join(b"@" + lines[2 * i][1:] + b"\n" + lines[2 * i + 1] + b"\n+\n" + qual[i * READ:(i + 1) * READ] + b"\n" for i in range(n))


def shape(label, table, fasta, raw, kept, runs):
    print("  %s" % label, flush=True)
    sel, flt = [], []
    for i in range(2 + runs):
        f_info, s_info = {}, {}
        out, keep, _ = table.filter(fasta, 1, 1, 1_000_000, info=f_info)
        fq = table.fastq_select(raw, keep=keep, kept=kept, info=s_info)
        if i >= 2:
            flt.append(f_info)
            sel.append(s_info)
    s, f = sel[0], flt[0]
    if kept is None:
        assert native.fq2fa(fq)[0] == out, "the FASTQ output holds other reads than the FASTA output"
    print("    %d records, %d emitted (%d of them cut), %d of %d bytes out, %d lines; filter: %d of %d bytes out" % (
        s["records"], s["records_out"], s["records_trimmed"], s["bytes_out"], len(raw), s["lines"], f["bytes_out"], len(fasta)), flush=True)
    got = {field: line("Counter.fastq_select", field, [i[field] for i in sel]) for field in FIELDS}
    g = line("Counter.filter", "s_gather", [i["s_gather"] for i in flt])
    line("Counter.filter", "s_place", [i["s_place"] for i in flt])
    rate, ref = s["bytes_out"] / got["s_gather"] / 1e9, f["bytes_out"] / g / 1e9
    print("    gather: %.0f GB/s of FASTQ written against %.0f GB/s of FASTA by fl_gather_k: %.2f x the time per output byte" % (
        rate, ref, ref / rate), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    # reads of two genomes, record by record in turn: a table of the first genome's reads holds every other record
    mine = native.synth_reads(1_000_000, 3, args.reads // 2, READ, 4).tobytes()
    theirs = native.synth_reads(1_000_000, 5, args.reads - args.reads // 2, READ, 6).tobytes()
    fasta = b"".join(b">" + a + b">" + b for a, b in zip(mine.split(b">")[1:], theirs.split(b">")[1:]))
    raw = fastq_of(fasta, 7)
    assert native.fq2fa(raw)[0] == fasta
    n = args.reads // 2 * 2
    rng = np.random.default_rng(11)
    kept = np.where(rng.random(n) < 1 / 3, rng.integers(K, READ, n), READ).astype(np.uint64)
    with native.Counter(K, native.ALPHABET_NT2) as table:
        table.count_chunk(mine, 1)
        what = "%d x %d bp reads, %.0f MB of FASTQ, %.0f MB as FASTA; every other read kept" % (n, READ, len(raw) / 1e6, len(fasta) / 1e6)
        shape(what + ", whole", table, fasta, raw, None, args.runs)
        shape(what + ", a third of them cut", table, fasta, raw, kept, args.runs)


if __name__ == "__main__":
    main()
