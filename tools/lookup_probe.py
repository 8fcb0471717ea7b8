"""a 1 M-key panel looked up in a table on the GPU (Counter.lookup / lookup_device / lookup_text) against the
fastest way to the same answers without mk_lookup -- (a) Counter.to_dict() + dict gets, (b) Counter.export() +
np.searchsorted over the sorted key rows -- in one process, on one table.  Warm-ups first, then median (min-max).

    python tools/lookup_probe.py [--genome 500000,5000000] [--keys 1000000] [--runs 7]

One key a lane against several: a second library beside the first,

    make -C mercat2_amd/csrc OBJDIR=../../build/obj_per1 LIB=../libmercat_hip_per1.so EXTRA=-DLK_PER=1
    MERCAT_HIP_LIB=mercat2_amd/libmercat_hip_per1.so python tools/lookup_probe.py

and compare the "probe kernel, s_probe" lines of the two runs.
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from mercat2_amd import native  # noqa: E402

K = 31


def timed(fn, warmups, runs):
    for _ in range(warmups):
        fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def show(label, times, extra=""):
    print("  %-58s %9.2f ms (%.2f-%.2f, %d runs)%s" % (label, 1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times),
                                                      len(times), extra), flush=True)
    return statistics.median(times)


def stream_copy_gbs(torch):
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)

    def copy():
        b.copy_(a)
        torch.cuda.synchronize()
    t = statistics.median(timed(copy, 2, 7))
    return 2 * a.numel() / t / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="500000,5000000", help="genome lengths of the synthetic samples (about 2 rows per base)")
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--slow-runs", type=int, default=5, help="runs of the yardsticks (whole-table exports)")
    args = ap.parse_args()
    import torch
    print(native.lib().mk_version().decode(), "|", torch.cuda.get_device_name(0))
    copy_gbs = stream_copy_gbs(torch)
    print("device-to-device copy of 1 GiB (read + write): %.0f GB/s" % copy_gbs)
    rng = np.random.default_rng(7)
    for genome in [int(x) for x in args.genome.split(",")]:
        data = native.synth_reads(genome, 3, genome // 10, 150, 4)
        with native.Counter(K, native.ALPHABET_NT2) as ctx, tempfile.TemporaryDirectory() as tmp:
            ctx.count_chunk(data, 1)
            del data
            kmers, counts = ctx.export()
            rows = len(counts)
            half = args.keys // 2
            present = kmers[rng.integers(0, rows, half)]
            absent = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (args.keys - half, K))]
            panel = np.ascontiguousarray(np.concatenate([present, absent])[rng.permutation(args.keys)])
            keys_s = panel.view("S%d" % K).ravel()
            keys_str = [x.decode() for x in keys_s.tolist()]
            print("table: %d rows (k = %d, -c 1, %.0f MB of rows); panel: %d keys, %.0f MB" % (rows, K, rows * (K + 8) / 1e6, args.keys,
                                                                                         panel.nbytes / 1e6), flush=True)
            answers = {}

            def by_dict():
                table = ctx.to_dict()
                answers["dict"] = np.array([table.get(key, 0) for key in keys_str], dtype=np.uint64)

            def by_searchsorted():
                km, cn = ctx.export()
                sorted_keys = km.view("S%d" % K).ravel()
                at = np.minimum(np.searchsorted(sorted_keys, keys_s), len(cn) - 1)
                answers["sorted"] = np.where(sorted_keys[at] == keys_s, cn[at], 0).astype(np.uint64)

            info = {}

            def by_lookup():
                answers["lookup"] = ctx.lookup(panel, info=info)

            d_keys = torch.from_numpy(panel).cuda()
            d_out = torch.zeros(args.keys, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            dev_info = {}

            def by_device():
                dev_info.update(ctx.lookup_device(d_keys.data_ptr(), args.keys, d_out.data_ptr()))

            panel_file = os.path.join(tmp, "panel.txt")
            with open(panel_file, "wb") as fh:
                fh.write(b"\n".join(keys_s.tolist()) + b"\n")
            text_info = {}

            def by_text():
                got, i = ctx.lookup_text(panel_file)
                answers["text"] = got
                text_info.update(i)

            t_a = show("(a) to_dict() + dict gets", timed(by_dict, 1, args.slow_runs))
            t_b = show("(b) export() + np.searchsorted", timed(by_searchsorted, 1, args.slow_runs))
            yard = min(t_a, t_b)
            t_l = show("Counter.lookup, host array", timed(by_lookup, 2, args.runs))
            t_d = show("Counter.lookup_device", timed(by_device, 2, args.runs))
            t_t = show("Counter.lookup_text, file in the page cache", timed(by_text, 2, args.runs))
            answers["device"] = d_out.cpu().numpy().view(np.uint64)
            for name in ("sorted", "lookup", "device", "text"):
                assert (answers[name] == answers["dict"]).all(), name
            print("  answers agree; found %d of %d" % (info["found"], args.keys))
            print("  yardstick / route: lookup %.0fx, lookup_device %.0fx, lookup_text %.0fx" % (yard / t_l, yard / t_d, yard / t_t))
            print("  lookup: s_read %.2f ms, s_probe %.3f ms, s_total %.2f ms; lookup_text: s_read %.2f ms, s_probe (line starts + probe) "
                  "%.3f ms, s_total %.2f ms, %d pieces" % (1e3 * info["s_read"], 1e3 * info["s_probe"], 1e3 * info["s_total"],
                                                          1e3 * text_info["s_read"], 1e3 * text_info["s_probe"],
                                                          1e3 * text_info["s_total"], text_info["pieces"]))
            # the probe kernel alone (HIP events); a library built with -DLK_PER=1 gives the one-key-a-lane figure
            L, st = native.lib(), native.Lookup()
            probe = []
            for i in range(2 + args.runs):
                rc = L.mk_lookup_device(ctx._h, d_keys.data_ptr(), args.keys, 0, d_out.data_ptr(), ctypes.byref(st))
                assert rc == 0, rc
                if i >= 2:
                    probe.append(st.s_probe)
            p = show("probe kernel, s_probe", probe)
            print("    %.0f M keys/s; keys x 64 B / s_probe = %.0f GB/s (device-to-device copy: %.0f GB/s)" % (
                args.keys / p / 1e6, args.keys * 64 / p / 1e9, copy_gbs))


if __name__ == "__main__":
    main()
