"""FASTQ mode against the FASTA path on the same reads (one chunk per sample, k = 31, -c 2): seeded synthetic FASTQ
(150-bp reads from a 10 Mbp genome, ~50-byte headers, random qualities) of about 100 MB and 400 MB, and the same reads
written as FASTA (what fq2fa makes of them).  Both are fed from HBM through mk_chunk_feed_device (the same
device-to-device copy into the context's buffer), so the difference is the pre-pass plus the parser's cost on the
blanked bytes.  Also times the host conversion (mk_fq2fa).  Kernel times of the pre-pass: run this under
`rocprofv3 --kernel-trace --stats -- python tools/fastq_probe.py`.

    python tools/fastq_probe.py [reps]"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from mercat2_amd import native


def synth_fastq(reads: int, seed: int) -> bytes:
    fa = native.synth_reads(10_000_000, seed, reads, 150, seed + 1).tobytes()
    lines = fa.split(b"\n")
    qual = np.random.default_rng(seed).integers(33, 75, size=(reads, 150), dtype=np.uint8)
    out = []
    for i in range(reads):
        out += [b"@M00618:17:000000000-A31W7:1:1101:%d:%d 1:N:0:%d" % (i, 1000 + i % 9000, i % 97), lines[2 * i + 1], b"+",
                qual[i].tobytes()]
    return b"\n".join(out) + b"\n"


def timed(ctx, buf, n, reps):
    L, h = ctx._L, ctx._h
    best = 1e9
    for _ in range(reps + 1):
        ctx.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx._check(L.mk_chunk_begin(h))
        ctx._check(L.mk_chunk_feed_device(h, buf.data_ptr(), n))
        ctx._check(L.mk_chunk_end(h, 2))
        ctx.rows()  # (waits for the chunk)
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for reads in (280_000, 1_120_000):
        fq = synth_fastq(reads, 5)
        t0 = time.perf_counter()
        fa, st = native.fq2fa(fq)
        host_s = time.perf_counter() - t0
        dq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).cuda()
        da = torch.frombuffer(bytearray(fa), dtype=torch.uint8).cuda()
        with native.Counter(31) as cq, native.Counter(31) as ca:
            cq.set_fastq(True)
            tq = timed(cq, dq, len(fq), reps)
            assert cq.fastq_stats() == st
            rq = cq.rows()
            ta = timed(ca, da, len(fa), reps)
            assert ca.rows() == rq
        print("reads %d  FASTQ %.1f MB  FASTA %.1f MB  | FASTQ mode %.2f ms  FASTA %.2f ms  ratio %.2f | host mk_fq2fa %.1f ms = %.2f GB/s  rows %d"
              % (reads, len(fq) / 1e6, len(fa) / 1e6, 1e3 * tq, 1e3 * ta, tq / ta, 1e3 * host_s, len(fq) / host_s / 1e9, rq))
        del dq, da


if __name__ == "__main__":
    main()
