"""Where the flat parse lane stops paying (MK_FLAT_MIN_SHARE, mk_chunk.hip): one 100 MiB chunk of 150-base reads whose
header lines are about 10, 30, 60 and 120 bytes long, counted with the lane on and with MK_FP_FLAT=0 (k=31, -c 10).
Per-kernel-family HIP-event times as in tools/parse_probe.py; the scatter walks the header bytes in the flat layout, so
the longer the header lines, the more the partition costs.  python tools/flat_probe.py [chunks]"""
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from mercat2_amd import native

chunks = int(sys.argv[1]) if len(sys.argv) > 1 else 6
TOTAL, READ = 100 << 20, 150
genome = torch.randint(0, 4, (10_000_000,), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
genome = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[genome]
print("header  share  lane  parse us  part us  count us    sum us  flat chunks/refused")
for header in (10, 30, 60, 120):
    rec = header + 1 + READ + 1
    nrec = TOTAL // rec
    text = torch.full((nrec, rec), ord("x"), dtype=torch.uint8, device="cuda")
    text[:, 0] = ord(">")
    number = torch.arange(nrec, device="cuda")
    for d in range(8):  # the record's number, so that header lines differ
        text[:, 1 + d] = (48 + (number // 10 ** (7 - d)) % 10).to(torch.uint8)
    text[:, header] = 10
    text[:, -1] = 10
    start = torch.randint(0, genome.numel() - READ, (nrec,), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    text[:, header + 1:header + 1 + READ] = genome[start[:, None] + torch.arange(READ, device="cuda")[None, :]]
    buf = text.reshape(-1).contiguous()
    torch.cuda.synchronize()
    for lane in ("1", "0"):
        os.environ["MK_FP_FLAT"] = lane
        os.environ["MK_FP_FLAT_SHARE"] = "0"  # (the guard must not decide what is being measured)
        with native.Counter(31, native.ALPHABET_NT2) as ctx:
            for rep in range(2):
                ctx.reset()
                ctx.reset_stats()
                ctx.set_profiling(rep == 1)
                for i in range(chunks):
                    ctx.count_device(buf.data_ptr(), buf.numel(), 10)
            st = ctx.stats()
        us = [1e3 * st["ms_" + f] / max(1, st["n_" + f]) for f in ("parse", "part", "count")]
        print("%6d  %.3f  %4s  %8.1f  %7.1f  %8.1f  %8.1f  %d/%d  rows %d" % (
            header, st["symbols"] / max(1, st["raw_bytes"]), "flat" if lane == "1" else "off", us[0], us[1], us[2], sum(us),
            st["flat_chunks"], st["flat_refused"], st["rows"]), flush=True)
    del text, buf
