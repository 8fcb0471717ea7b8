"""quality trimming on the device (Counter.fastq_qtrim_device) on synthetic 150 bp FASTQ reads held in HBM,
beside Counter.fastq_select_device keeping every record of the same text in the same session -- that call runs the line
index and the gather without the scan, so the difference is what reading the qualities costs.  s_scan is also given
as bytes of quality and sequence line read per second.  The reads come from seeds: qualities fall towards the 3' end,
so that cut_back = 20 cuts most reads.  Two warm-ups, then median (min-max) of the runs.

    python tools/qtrim_probe.py [--reads 10000000] [--runs 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mercat2_amd import native  # noqa: E402

READ = 150


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-28s %-9s %9.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m


def reads_text(n: int, seed: int) -> bytes:
    """n records '@r\\n' + 150 bases + '\\n+\\n' + 150 qualities + '\\n', built as one array (no Python loop over reads)."""
    if n > 1_000_000:  # (a million distinct reads, repeated: the generator's floats would not fit otherwise)
        block = reads_text(1_000_000, seed)
        return block * (n // 1_000_000) + block[: (n % 1_000_000) * (len(block) // 1_000_000)]
    rng = np.random.default_rng(seed)
    rec = np.empty((n, 3 + READ + 3 + READ + 1), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
    rec[:, 3:3 + READ] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, READ), dtype=np.uint8)]
    rec[:, 3 + READ:6 + READ] = np.frombuffer(b"\n+\n", np.uint8)
    x = np.arange(READ) / READ
    tail = rng.random((n, 1)) * 1.5  # how deep the read's 3' end sinks
    q = np.clip(np.rint(38 - 34 * tail * x ** 3 + rng.normal(0, 3, (n, READ))), 2, 41).astype(np.uint8)
    rec[:, 6 + READ:6 + 2 * READ] = q + 33
    rec[:, -1] = 10
    return rec.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", native.library_path().name, "|", torch.cuda.get_device_name(0), flush=True)
    n = args.reads
    raw = reads_text(n, 7)
    d_text = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8)).cuda()
    d_out = torch.empty(len(raw) + 1, dtype=torch.uint8, device="cuda")
    d_keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_rows = torch.empty((n, 6), dtype=torch.int64, device="cuda")
    d_hist = torch.empty(512, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    print("  %d x %d bp reads, %.0f MB of FASTQ in HBM, cut_back = 20" % (n, READ, len(raw) / 1e6), flush=True)
    trim, sel = [], []
    with native.Counter(5, native.ALPHABET_NT2) as ctx:
        for i in range(2 + args.runs):
            t = ctx.fastq_qtrim_device(d_text.data_ptr(), len(raw), d_out.data_ptr(), len(raw) + 1, n, d_keep.data_ptr(),
                                       d_rows.data_ptr(), d_hist.data_ptr(), cut_back=20)
            s = ctx.fastq_select_device(d_text.data_ptr(), len(raw), d_out.data_ptr(), len(raw) + 1, n)
            if i >= 2:
                trim.append(t)
                sel.append(s)
    t, s = trim[0], sel[0]
    print("    qtrim: %d records, %d emitted (%d of them cut), %d of %d bases, %d bytes out; select: %d bytes out" % (
        t["records"], t["records_out"], t["records_trimmed"], t["bases_out"], t["bases_in"], t["bytes_out"], s["bytes_out"]), flush=True)
    got = {f: line("Counter.fastq_qtrim_device", f, [i[f] for i in trim]) for f in ("s_index", "s_scan", "s_place", "s_gather")}
    ref = {f: line("Counter.fastq_select_device", f, [i[f] for i in sel]) for f in ("s_index", "s_place", "s_gather")}
    read = 2 * t["bases_in"]  # the quality and the sequence line of every record
    print("    scan: %.0f GB/s of quality and sequence line read (%d bytes); the kernels of the call %.3f ms against %.3f ms "
          "of the select call" % (read / got["s_scan"] / 1e9, read, 1e3 * sum(got.values()), 1e3 * sum(ref.values())), flush=True)


if __name__ == "__main__":
    main()
