"""reads thinned to a target depth by their median k-mer count (Counter.normalize), k = 31, with the route
there was before and the yardsticks in the same process, interleaved with the timed runs: (a) the parent's only route --
Counter.track(sat32=True, median=True), the rule in numpy, the text sliced in Python -- compared in every run for equal
bytes; (b) Counter.track on the same text, whose s_track and s_median are the same kernels into a staging buffer; (c)
Counter.filter keeping every record with a k-mer, whose s_gather moves whole records.  Then the median of long records
(Counter.track's s_median): one record of 100 Mbases with 2 % of its windows absent, with every window equal, one of 10
Mbases, and a sweep of one record of 2^14 .. 2^24 windows at k = 5 against a table whose counts fill all four bytes (the
most passes a selection makes).  --package DIR takes mercat2_amd from DIR instead of this tree (the parent commit's
build, for the same measurements by the segmented sort); MERCAT_HIP_LIB names an A/B build of the library.  The texts
come from seeds.  Two warm-ups, then median (min-max) of the runs.

    python tools/norm_probe.py [--reads 1000000] [--long 100000000] [--sweep] [--runs 5] [--package DIR]

Pass mark: Counter.normalize is faster end to end than the track route (asserted).
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

K = 31
READ = 150
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-26s %-9s %10.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def substitute(text: np.ndarray, at: np.ndarray) -> np.ndarray:
    """The text with the bases at the given positions replaced by the next of A, C, G, T."""
    out = text.copy()
    code = np.zeros(256, dtype=np.uint8)
    code[ACGT] = np.arange(4, dtype=np.uint8)
    out[at] = ACGT[(code[text[at]] + 1) & 3]
    return out


def u_of(seed: int, n: int) -> np.ndarray:
    """The upper 32 bits of splitmix64 of records 0 .. n - 1 under seed."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return (z ^ (z >> np.uint64(31))) >> np.uint64(32)


def track_route(ctx, text, target, min_depth, seed):
    """What a user could do before: every count and the medians to the host, the decision with numpy, the text sliced in
    Python.  (Records of one header line and one sequence line, as synth_reads writes them.)"""
    t0 = time.perf_counter()
    _, _, rows, med = ctx.track(text, max(min_depth, 1), sat32=True, median=True)
    m = med.astype(np.uint64)
    keep = (rows[:, 0] > 0) & (m >= min_depth) & ((m <= target) | (u_of(seed, len(m)) * m < np.uint64(target << 32)))
    lines = bytes(text).split(b"\n")
    out = b"".join(lines[2 * i] + b"\n" + lines[2 * i + 1] + b"\n" for i in np.flatnonzero(keep).tolist())
    return out, keep, time.perf_counter() - t0


def reads_shape(native, n_reads, runs):
    text = native.synth_reads(1_000_000, 3, n_reads, READ, 4)
    with native.Counter(K, native.ALPHABET_NT2) as ctx:
        ctx.count_chunk(text, 1)
        _, _, _, med = ctx.track(text, sat32=True, median=True)
        depth = int(np.median(med))
        target = max(1, depth // 4)
        print("  %d x %d bp reads against their own table, %.0f MB of text, depth (the median of the medians) %d, target %d" % (
            n_reads, READ, len(text) / 1e6, depth, target), flush=True)
        nrm, trk, flt, old = [], [], [], []
        for i in range(2 + runs):
            info = {}
            t0 = time.perf_counter()
            out, keep, _, _ = ctx.normalize(text, target, info=info)
            info["wall"] = time.perf_counter() - t0
            want, want_keep, sec = track_route(ctx, text, target, 0, 0)
            assert out == want and keep.tolist() == want_keep.tolist(), "normalize differs from the track route"
            t_info, f_info = {}, {}
            ctx.track(text, sat32=True, median=True, info=t_info)
            ctx.filter(text, 1, info=f_info)
            if i >= 2:
                nrm.append(info)
                trk.append(t_info)
                flt.append(f_info)
                old.append(sec)
            del out, keep, want
        f = nrm[0]
        print("    Counter.normalize: %d records, %d emitted, %d over the target, %d of them thinned out; %d bytes out, %d piece(s)" % (
            f["records"], f["records_out"], f["records_over"], f["records_thinned"], f["bytes_out"], f["pieces"]), flush=True)
        m = {field: line("Counter.normalize", field, [i[field] for i in nrm])
             for field in ("s_read", "s_parse", "s_probe", "s_place", "s_track", "s_median", "s_gather", "s_write", "s_total", "wall")}
        route = line("track route", "wall", old)
        for field in ("s_track", "s_median", "s_write"):
            vals = [i[field] for i in trk]
            line("Counter.track", field, vals, "" if field == "s_write" else
                 "  normalize's: %s its min-max" % ("within" if min(vals) <= m[field] <= max(vals) else "OUTSIDE"))
        gather = line("Counter.filter", "s_gather", [i["s_gather"] for i in flt], " for %d bytes" % flt[0]["bytes_out"])
        print("    track route / normalize (wall) = %.2f" % (route / m["wall"]), flush=True)
        print("    s_gather: %.1f GB/s of output (the filter's gather: %.1f GB/s)" % (
            f["bytes_out"] / m["s_gather"] / 1e9, flt[0]["bytes_out"] / gather / 1e9), flush=True)
        assert m["wall"] < route, "the pass mark: normalize is faster end to end than the track route"


def median_shape(label, ctx, text, runs):
    infos = []
    for i in range(2 + runs):
        info = {}
        t0 = time.perf_counter()
        ctx.track(text, sat32=True, median=True, info=info)
        info["wall"] = time.perf_counter() - t0
        if i >= 2:
            infos.append(info)
    print("  %s: %d records, %d windows" % (label, infos[0]["records"], infos[0]["windows"]), flush=True)
    for field in ("s_track", "s_median", "wall"):
        line("Counter.track", field, [i[field] for i in infos])


def record(seq: np.ndarray) -> np.ndarray:
    return np.concatenate([np.frombuffer(b">g\n", dtype=np.uint8), seq, np.frombuffer(b"\n", dtype=np.uint8)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000_000)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--package", type=str, default=str(Path(__file__).resolve().parent.parent))
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    from mercat2_amd import native
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path(), "|", torch.cuda.get_device_name(0), flush=True)
    rng = np.random.default_rng(11)
    if args.reads and hasattr(native.Counter, "normalize"):
        reads_shape(native, args.reads, args.runs)
    if args.reads:
        text = native.synth_reads(1_000_000, 3, args.reads, READ, 4)
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(text, 1)
            median_shape("%d x %d bp reads against their own table (the short segments)" % (args.reads, READ), ctx, text, args.runs)
    if args.long:
        genome = ACGT[rng.integers(0, 4, args.long)]
        clean = record(genome)
        text = substitute(clean, 3 + np.arange(1000, args.long, 1550))  # (a substitution takes 31 windows: 2 % of them)
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(clean, 1)
            median_shape("one %d-base record, 2 %% of its windows absent" % args.long, ctx, text, args.runs)
        with native.Counter(K, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(b">x\n" + b"ACGTTGCAGGATCCATGAACGTACGGTCAGTTGACCA" * 4 + b"\n", 1)
            median_shape("the same record, every window equal (absent: the contention shape)", ctx, text, args.runs)
            median_shape("one %d-base record, every window equal" % (args.long // 10), ctx, record(genome[:args.long // 10]), args.runs)
        del genome, clean, text
    if args.sweep:
        codes = np.arange(1024, dtype=np.uint64)
        lut = (codes * np.uint64(2654435761)) % np.uint64(2 ** 32 - 5) + np.uint64(1)
        tsv = b"".join(b"%s\t%d\n" % (bytes(ACGT[(c >> (2 * np.arange(4, -1, -1))) & 3]), v) for c, v in zip(codes.astype(np.int64), lut.tolist()))
        with native.Counter(5, native.ALPHABET_NT2) as ctx:
            assert ctx.load_tsv(tsv)["rows"] == 1024
            print("  the sweep: one record at k = 5, counts that fill four bytes", flush=True)
            for e in range(14, 25):
                median_shape("2^%d windows" % e, ctx, record(ACGT[rng.integers(0, 4, (1 << e) + 4)]), args.runs)


if __name__ == "__main__":
    main()
