"""reads corrected against their own table (Counter.correct), k = 31, beside Counter.trim on the same text and
table -- the call that existed before and walks the same windows once -- in the same process, the legs interleaved: what
finding, trying and applying the candidates costs on top of a walk.  The text is synthetic reads with 1 % of substituted
bases; the table is counted from those reads.  Two warm-ups, then median (min-max) of the runs.

    python tools/correct_probe.py [--reads 1000000] [--runs 5] [--at-least 3] [--parent DIR]

--parent DIR: a tree that holds another build's mercat2_amd (its .py files and libmercat_hip.so) for the trim leg;
without it this build trims.  No pass mark: the figures are written down (profiles/correct_probe.md).
"""
import argparse
import importlib.util
import statistics
import sys
import time
from pathlib import Path

import numpy as np

K = 31
READ = 150
ROOT = Path(__file__).resolve().parent.parent
CORRECT_FIELDS = ("s_read", "s_parse", "s_probe", "s_place", "s_track", "s_runs", "s_try", "s_gather", "s_write", "s_total")
TRIM_FIELDS = ("s_read", "s_parse", "s_probe", "s_place", "s_first", "s_gather", "s_write", "s_total")


def line(label, field, values, extra=""):
    m, lo, hi = statistics.median(values), min(values), max(values)
    print("    %-26s %-9s %10.3f ms (%.3f-%.3f, %d runs)%s" % (label, field, 1e3 * m, 1e3 * lo, 1e3 * hi, len(values), extra), flush=True)
    return m, lo, hi


def other_package(folder: str):
    """mercat2_amd of another tree under another name, with its own copy of the library."""
    init = Path(folder) / "mercat2_amd" / "__init__.py"
    spec = importlib.util.spec_from_file_location("mercat2_parent", init, submodule_search_locations=[str(init.parent)])
    module = importlib.util.module_from_spec(spec)
    sys.modules["mercat2_parent"] = module
    spec.loader.exec_module(module)
    return importlib.import_module("mercat2_parent.native")


def timed(call):
    info = {}
    t0 = time.perf_counter()
    res = call(info)
    info["wall"] = time.perf_counter() - t0
    return res, info


def wrong_bases(text, truth):
    """Bytes in which two texts of the same records differ, or None where they are not laid out alike."""
    a, b = np.frombuffer(text, np.uint8), np.frombuffer(truth, np.uint8)
    return int(np.count_nonzero(a != b)) if a.shape == b.shape else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--at-least", type=int, default=3)
    ap.add_argument("--parent", type=str, default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from mercat2_amd import native
    import torch
    other = other_package(args.parent) if args.parent else native
    print(native.lib().mk_version().decode(), "|", native.library_path(), "|", torch.cuda.get_device_name(0), flush=True)
    print("the trim leg:", other.library_path(), flush=True)
    text = native.synth_reads(1_000_000, 3, args.reads, READ, 4, 10000).tobytes()
    truth = native.synth_reads(1_000_000, 3, args.reads, READ, 4, 0).tobytes()  # the same reads without their errors, if the draws allow
    before = wrong_bases(text, truth)
    if before is None or not 0.005 * READ * args.reads < before < 0.015 * READ * args.reads:
        truth, before = None, None
    with native.Counter(K, native.ALPHABET_NT2) as ctx, other.Counter(K, other.ALPHABET_NT2) as old:
        ctx.count_chunk(text, 1)
        old.count_chunk(text, 1)
        print("  %d x %d bp reads against their own table, %.0f MB of text, at_least %d" % (args.reads, READ, len(text) / 1e6, args.at_least), flush=True)
        new, was = [], []
        for i in range(2 + args.runs):
            res, info = timed(lambda i_: ctx.correct(text, args.at_least, info=i_))
            res_t, info_t = timed(lambda i_: old.trim(text, args.at_least, info=i_))
            if i == 0:
                assert res[2].tolist() == res_t[2].tolist(), "the rows differ"
                f = info
                weak = f["windows"] - f["hits"]
                print("  %d records, %d windows, %d of them weak; %d runs, %d candidates: %d fixed, %d ambiguous, %d unfixable; "
                      "%d piece(s)" % (f["records"], f["windows"], weak, f["runs"], f["candidates"], f["fixed"], f["ambiguous"],
                                       f["unfixable"], f["pieces"]), flush=True)
                print("  probes: %d in the walk (and as many in the track), at most %d in the try kernel (4 alternatives x %d "
                      "windows a candidate at most; %.1f windows a candidate on average if every weak window were tried)" % (
                          f["windows"], 4 * K * f["candidates"], K, weak / max(1, f["candidates"])), flush=True)
                if truth is not None:
                    after = wrong_bases(res[0], truth)
                    second = ctx.correct(res[0], args.at_least)[0]
                    print("  wrong bases: %d before, %s after one pass, %s after two" % (before, after, wrong_bases(second, truth)), flush=True)
                    del second
            if i >= 2:
                new.append(info)
                was.append(info_t)
            del res, res_t
        for field in CORRECT_FIELDS:
            line("Counter.correct", field, [i[field] for i in new])
        m, _, _ = line("Counter.correct", "wall", [i["wall"] for i in new])
        for field in TRIM_FIELDS:
            line("Counter.trim", field, [i[field] for i in was])
        mt, lo, hi = line("Counter.trim", "wall", [i["wall"] for i in was])
        med = lambda rows, field: statistics.median(i[field] for i in rows)
        print("  correct / trim: wall %.2f, s_total %.2f; s_try / s_track %.2f, s_try / s_probe %.2f, (s_track + s_runs + s_try) / "
              "trim's s_first %.2f" % (m / mt, med(new, "s_total") / med(was, "s_total"), med(new, "s_try") / med(new, "s_track"),
                                      med(new, "s_try") / med(new, "s_probe"),
                                      (med(new, "s_track") + med(new, "s_runs") + med(new, "s_try")) / med(was, "s_first")), flush=True)


if __name__ == "__main__":
    main()
