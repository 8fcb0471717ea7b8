"""FASTQ reads corrected where they stand (Counter.correct_fastq), k = 31, beside the route there was before --
native.fq2fa on the host, then Counter.correct on the FASTA it gives -- on the same reads and table, in one process,
the legs interleaved.  The workload is 8t's: synthetic reads with 1 % of substituted bases against their own table.  Two
warm-ups, then median (min-max) of the runs.  The run also confirms that fq2fa of the FASTQ output is the FASTA output
and that the wrong bases fall by exactly `fixed`.

    python tools/correct_fastq_probe.py [--reads 1000000] [--runs 5] [--at-least 3]

No pass mark: the figures are written down (profiles/correct_fastq.md).
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
FASTQ_FIELDS = ("s_copy", "s_index", "s_parse", "s_probe", "s_place", "s_track", "s_runs", "s_try", "s_patch", "s_write", "s_total")
FASTA_FIELDS = ("s_read", "s_parse", "s_probe", "s_place", "s_track", "s_runs", "s_try", "s_gather", "s_write", "s_total")


def line(label, field, values):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-34s %-9s %10.3f ms (%.3f-%.3f, %d runs)" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values)), flush=True)
    return m


def fastq_of(fasta: bytes, seed: int) -> bytes:
    """The one-line FASTA records as FASTQ records with seeded qualities ('!' + 0..40)."""
    lines = fasta.split(b"\n")[:-1]
    n = len(lines) // 2
    qual = (np.random.default_rng(seed).integers(33, 74, (n, READ), dtype=np.uint8)).tobytes()
    return b"".join(b"@" + lines[2 * i][1:] + b"\n" + lines[2 * i + 1] + b"\n+\n" + qual[i * READ:(i + 1) * READ] + b"\n" for i in range(n))


def differing(a: bytes, b: bytes):
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    return int(np.count_nonzero(x != y)) if x.shape == y.shape else None


def timed(call):
    info = {}
    t0 = time.perf_counter()
    res = call(info)
    info["wall"] = time.perf_counter() - t0
    return res, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--at-least", type=int, default=3)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    fasta = native.synth_reads(1_000_000, 3, args.reads, READ, 4, 10000).tobytes()
    truth = native.synth_reads(1_000_000, 3, args.reads, READ, 4, 0).tobytes()  # the same reads without their errors, if the draws allow
    raw = fastq_of(fasta, 7)
    assert native.fq2fa(raw)[0] == fasta
    before = differing(fasta, truth)
    if before is None or not 0.005 * READ * args.reads < before < 0.015 * READ * args.reads:
        truth, before = None, None
    with native.Counter(K, native.ALPHABET_NT2) as ctx:
        ctx.count_chunk(fasta, 1)
        print("  %d x %d bp reads against their own table, %.0f MB of FASTQ, %.0f MB as FASTA, at_least %d" % (
            args.reads, READ, len(raw) / 1e6, len(fasta) / 1e6, args.at_least), flush=True)
        new, was = [], []
        for i in range(2 + args.runs):
            res_q, info_q = timed(lambda i_: ctx.correct_fastq(raw, args.at_least, info=i_))

            def old_route(i_):
                t0 = time.perf_counter()
                text = native.fq2fa(raw)[0]
                i_["s_fq2fa"] = time.perf_counter() - t0
                return ctx.correct(text, args.at_least, info=i_)
            res_a, info_a = timed(old_route)
            if i == 0:
                f = info_q
                assert res_q[1].tolist() == res_a[1].tolist() and res_q[2].tolist() == res_a[2].tolist(), "fix or rows differ"
                assert native.fq2fa(res_q[0])[0] == res_a[0], "fq2fa of the FASTQ output is not the FASTA output"
                assert len(res_q[0]) == len(raw) and differing(res_q[0], raw) == f["fixed"] == f["patched"]
                print("  %d records, %d lines, %d windows, %d of them weak; %d runs, %d candidates: %d fixed (%d bytes patched), "
                      "%d ambiguous, %d unfixable; %d piece(s) of FASTQ, %d of FASTA" % (
                          f["records"], f["lines"], f["windows"], f["windows"] - f["hits"], f["runs"], f["candidates"], f["fixed"],
                          f["patched"], f["ambiguous"], f["unfixable"], f["pieces"], info_a["pieces"]), flush=True)
                print("  fq2fa of the FASTQ output equals the FASTA output; fix and rows equal", flush=True)
                if truth is not None:
                    after = differing(native.fq2fa(res_q[0])[0], truth)
                    print("  wrong bases: %d before, %d after, %d fewer for %d fixed" % (before, after, before - after, f["fixed"]), flush=True)
            if i >= 2:
                new.append(info_q)
                was.append(info_a)
            del res_q, res_a
        got = {field: line("Counter.correct_fastq", field, [i[field] for i in new]) for field in FASTQ_FIELDS}
        wall_q = line("Counter.correct_fastq", "wall", [i["wall"] for i in new])
        ref = {field: line("fq2fa + Counter.correct", field, [i[field] for i in was]) for field in FASTA_FIELDS}
        line("fq2fa + Counter.correct", "s_fq2fa", [i["s_fq2fa"] for i in was])
        wall_a = line("fq2fa + Counter.correct", "wall", [i["wall"] for i in was])
        print("  s_index + s_patch %.3f ms against the s_gather + s_write %.3f ms of mk_correct_text that they replace (its own "
              "copy back, s_write, is %.3f ms here); wall %.2f of the old route's" % (
                  1e3 * (got["s_index"] + got["s_patch"]), 1e3 * (ref["s_gather"] + ref["s_write"]), 1e3 * got["s_write"],
                  wall_q / wall_a), flush=True)


if __name__ == "__main__":
    main()
