"""mate-overlap detection on the device (Counter.fastq_overlap_device) on synthetic 2 x 150 bp pairs held in
HBM as interleaved FASTQ, in both modes, beside Counter.fastq_adapt_device (paired, one adapter) on the same text in the
same session -- the line index, the placement and the gather are the same kernels, so the two calls' s_index, s_place and
s_gather should agree in trim mode.  The fragment lengths are drawn so that about a third of the pairs read through (F in
30 .. 149), a third overlap without adapter (F in 150 .. 270) and a third do not overlap at all (independent mates); every
base is then substituted with probability 0.01.  s_scan is also given as candidate x word compares a second: a candidate
offset of a pair (those up to its hit in the rule's order, or all of them without one) against the 64-bit words -- 32
bases -- its overlap touches.  The pairs that do not overlap and are given a hit all the same (chance hits) are counted.
Two warm-ups, then median (min-max) of the runs.

    python tools/overlap_probe.py [--pairs 5000000] [--runs 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mercat2_amd import native  # noqa: E402

READ = 150
MIN_OVERLAP = 30
BLOCK = 1_000_000  # distinct pairs; more are repeats of them
TRUSEQ = native.ILLUMINA_ADAPTERS[0][1].encode()


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-36s %-9s %9.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def pairs_text(n: int, seed: int):
    """(text, kind): n pairs as interleaved records '@r\\n' + 150 bases + '\\n+\\n' + 150 qualities + '\\n', built as arrays
    (no Python loop over pairs); kind[p]: 0 read-through, 1 overlap without adapter, 2 no overlap."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, n)
    frag = np.where(kind == 0, rng.integers(MIN_OVERLAP, READ, n), np.where(kind == 1, rng.integers(READ, 2 * READ - MIN_OVERLAP + 1, n), 3 * READ))
    d = frag - READ  # rc(mate 2) lies under the template's positions d .. d + 149; mate 1 is its positions 0 .. 149
    template = rng.integers(0, 4, (n, 3 * READ), dtype=np.uint8)
    at = d[:, None] + np.arange(READ)[None, :]
    rc = np.where(at >= 0, np.take_along_axis(template, np.clip(at, 0, 3 * READ - 1), axis=1), rng.integers(0, 4, (n, READ), dtype=np.uint8))
    codes = np.stack([template[:, :READ], 3 - rc[:, ::-1]], axis=1)  # (n, 2, 150): mate 1, and mate 2 = revcomp(rc)
    wrong = rng.random(codes.shape) < 0.01
    codes = (codes + wrong * rng.integers(1, 4, codes.shape, dtype=np.uint8)) & 3
    rec = np.empty((n, 2, 3 + READ + 3 + READ + 1), dtype=np.uint8)
    rec[:, :, 0:3] = np.frombuffer(b"@r\n", np.uint8)
    rec[:, :, 3:3 + READ] = np.frombuffer(b"ACGT", np.uint8)[codes]
    rec[:, :, 3 + READ:6 + READ] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, :, 6 + READ:6 + 2 * READ] = rng.integers(40, 74, (n, 2, READ), dtype=np.uint8)
    rec[:, :, -1] = 10
    return rec.reshape(-1), kind


def words_tested():
    """cum[c]: the 64-bit words of mate 1 that the first c candidates of a 150 / 150 pair touch, in the rule's order."""
    P = READ - MIN_OVERLAP + 1
    offsets = list(range(P)) + [-k for k in range(1, READ - MIN_OVERLAP + 1)]
    words = [(min(READ, d + READ) - 1) // 32 - max(d, 0) // 32 + 1 for d in offsets]
    return np.concatenate([[0], np.cumsum(words)]), P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    n = args.pairs
    block, kind = pairs_text(min(n, BLOCK), 7)
    d_block = torch.from_numpy(block).cuda()
    reps = -(-n // BLOCK)
    d_text = (d_block.repeat(reps) if reps > 1 else d_block)[: n * (len(block) // min(n, BLOCK))].contiguous()
    d_kind = torch.from_numpy(kind).cuda().repeat(reps)[:n]
    size = d_text.numel()
    del d_block
    d_out = torch.empty(size + 1, dtype=torch.uint8, device="cuda")
    d_keep = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    d_rows = torch.empty((2 * n, 5), dtype=torch.int64, device="cuda")
    d_hits = torch.empty(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    print("  %d pairs of 2 x %d bp, %.0f MB of interleaved FASTQ in HBM: %d read through, %d overlap, %d do not; 1 %% substitutions; "
          "min_overlap %d, max_mismatch 5, max_err 0.2" % (n, READ, size / 1e6, int((d_kind == 0).sum()), int((d_kind == 1).sum()),
                                                           int((d_kind == 2).sum()), MIN_OVERLAP), flush=True)
    cum, P = words_tested()
    d_cum = torch.from_numpy(cum).cuda()
    fields = ("s_copy", "s_index", "s_scan", "s_place", "s_gather")
    with native.Counter(5, native.ALPHABET_NT2) as ctx:
        got, adapt = {}, []
        for mode in ("trim", "merge"):
            runs = []
            for i in range(2 + args.runs):
                t = ctx.fastq_overlap_device(d_text.data_ptr(), size, d_out.data_ptr(), size + 1, 2 * n, d_keep.data_ptr(), d_rows.data_ptr(),
                                             mode=mode)
                a = ctx.fastq_adapt_device(d_text.data_ptr(), size, d_out.data_ptr(), size + 1, [TRUSEQ], None, 2 * n, d_keep.data_ptr(),
                                           d_rows.data_ptr(), d_hits.data_ptr(), paired=True) if mode == "trim" else None
                if i >= 2:
                    runs.append(t)
                    if a is not None:
                        adapt.append(a)
            if mode == "trim":  # (the rows are the same in both modes; the adapter call has overwritten them)
                ctx.fastq_overlap_device(d_text.data_ptr(), size, d_out.data_ptr(), size + 1, 2 * n, d_keep.data_ptr(), d_rows.data_ptr(), mode=mode)
            t = runs[0]
            print("  mode %s: %d pairs, %d with a hit, %d merged, %d trimmed, %d records out (%d not byte for byte), %d of %d bases, %d bytes out" % (
                mode, t["pairs"], t["pairs_hit"], t["pairs_merged"], t["pairs_trimmed"], t["records_out"], t["records_trimmed"], t["bases_out"],
                t["bases_in"], t["bytes_out"]), flush=True)
            got[mode] = {f: line("Counter.fastq_overlap_device " + mode, f, [r[f] for r in runs]) for f in fields}
        frag = d_rows[0::2, 2]
        hit = frag != native.OVERLAP_NO_HIT
        d_of = frag - READ
        index = torch.where(d_of >= 0, d_of, P - 1 - d_of)  # the hit's place in the rule's order
        tested = torch.where(hit, index + 1, torch.full_like(index, len(cum) - 1))
        candidates, compares = int(tested.sum().item()), int(d_cum[tested].sum().item())
        s = got["trim"]["s_scan"]
        print("  scan: %d candidates, %d candidate x word compares, %.3g a second; %.2f ns a pair" % (candidates, compares, compares / s, 1e9 * s / n),
              flush=True)
        print("  hits: %d of the %d pairs that overlap; chance hits: %d of the %d pairs that do not overlap" % (
            int((hit & (d_kind != 2)).sum().item()), int((d_kind != 2).sum().item()), int((hit & (d_kind == 2)).sum().item()),
            int((d_kind == 2).sum().item())), flush=True)
        print("  the merge writer: s_place %.3f ms in merge mode against %.3f ms in trim mode; its copy of the text: s_copy %.3f ms" % (
            1e3 * got["merge"]["s_place"], 1e3 * got["trim"]["s_place"], 1e3 * got["merge"]["s_copy"]), flush=True)
        print("  the same text through Counter.fastq_adapt_device, paired, one adapter (%d bytes out)" % adapt[0]["bytes_out"], flush=True)
        for f in ("s_index", "s_scan", "s_place", "s_gather"):
            line("Counter.fastq_adapt_device", f, [r[f] for r in adapt])


if __name__ == "__main__":
    main()
