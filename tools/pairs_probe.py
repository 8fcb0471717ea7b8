"""paired reads filtered, trimmed and normalised with the pair as the unit (Counter.pairs), k = 31, beside the
unpaired call of the same op of ANOTHER build of the package -- the parent commit's -- on the same text, in the same
process, the legs interleaved: what the pair costs on top of the records.  The text is synthetic reads with 1 % of
substituted bases against their own table; consecutive records are taken as mates (a pair is a matter of position).
Then the host route for two files: native.interleave and native.split_pairs in GB/s, and kmers.trim_reads from two
files beside the same reads interleaved.  Two warm-ups, then median (min-max) of the runs.

    python tools/pairs_probe.py [--reads 1000000] [--runs 5] [--parent DIR]

--parent DIR: a tree that holds the other build's mercat2_amd (its .py files and libmercat_hip.so); without it the
unpaired calls of this build are the other leg.  Pass mark, printed per op and not asserted: the paired call's median
wall time exceeds the other leg's by no more than that leg's own max - min.
"""
import argparse
import importlib.util
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

K = 31
READ = 150
ROOT = Path(__file__).resolve().parent.parent


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


def ops_shape(native, other, text, runs):
    with native.Counter(K, native.ALPHABET_NT2) as ctx, other.Counter(K, other.ALPHABET_NT2) as old:
        ctx.count_chunk(text, 1)
        old.count_chunk(text, 1)
        _, _, _, med = ctx.track(text, sat32=True, median=True)
        depth = int(np.median(med))
        target = max(1, depth // 4)
        print("  %d x %d bp reads (%d pairs) against their own table, %.0f MB of text, depth %d, norm target %d" % (
            len(med), READ, len(med) // 2, len(text) / 1e6, depth, target), flush=True)
        legs = {
            "filter": (lambda i: ctx.filter_pairs(text, 2, info=i), lambda i: old.filter(text, 2, info=i),
                       ("s_place", "s_gather", "s_write"), ("s_place", "s_gather", "s_write")),
            "trim": (lambda i: ctx.trim_pairs(text, 2, singles=True, info=i), lambda i: old.trim(text, 2, info=i),
                     ("s_place", "s_walk", "s_gather", "s_write"), ("s_place", "s_first", "s_gather", "s_write")),
            "norm": (lambda i: ctx.normalize_pairs(text, target, info=i), lambda i: old.normalize(text, target, info=i),
                     ("s_place", "s_walk", "s_median", "s_gather", "s_write"), ("s_place", "s_track", "s_median", "s_gather", "s_write")),
        }
        seen = {name: ([], []) for name in legs}
        for i in range(2 + runs):
            for name, (paired, unpaired, _, _) in legs.items():
                res, info = timed(paired)
                res_u, info_u = timed(unpaired)
                if i == 0:  # every mate's own result is the other leg's
                    assert res[4].tolist() == res_u[-1].tolist(), name + ": the rows differ"
                    if name == "trim":
                        assert res[3].tolist() == res_u[1].tolist(), "trim: kept differs"
                    if name == "norm":
                        assert res[3].tolist() == res_u[2].tolist(), "norm: the medians differ"
                if i >= 2:
                    seen[name][0].append(info)
                    seen[name][1].append(info_u)
                del res, res_u
        for name, (_, _, fields, fields_u) in legs.items():
            new, was = seen[name]
            f = new[0]
            print("  %s: %d pairs, %d emitted, %d orphans; %d bytes out, %d piece(s); unpaired: %d bytes out" % (
                name, f["pairs"], f["pairs_out"], f["singles_out"], f["bytes_out"], f["pieces"], was[0]["bytes_out"]), flush=True)
            for field in ("s_read", "s_parse", "s_probe") + fields + ("s_total",):
                line("Counter.pairs", field, [i[field] for i in new])
            m, _, _ = line("Counter.pairs", "wall", [i["wall"] for i in new])
            for field in ("s_read", "s_parse", "s_probe") + fields_u + ("s_total",):
                line("unpaired (other build)", field, [i[field] for i in was])
            mu, lo, hi = line("unpaired (other build)", "wall", [i["wall"] for i in was])
            over = m - mu
            print("    pass mark: paired - unpaired = %+.3f ms, the unpaired leg's spread %.3f ms: %s" % (
                1e3 * over, 1e3 * (hi - lo), "met" if over <= hi - lo else "MISSED by %.3f ms" % (1e3 * (over - (hi - lo)))), flush=True)


def host_shape(native, text, runs):
    from mercat2_amd import kmers
    both = bytes(text)
    one, two = native.split_pairs(both)
    assert native.interleave(one, two) == both
    t_in, t_sp = [], []
    for i in range(2 + runs):
        t0 = time.perf_counter()
        native.interleave(one, two)
        t1 = time.perf_counter()
        native.split_pairs(both)
        t2 = time.perf_counter()
        if i >= 2:
            t_in.append(t1 - t0)
            t_sp.append(t2 - t1)
    m, _, _ = line("native.interleave", "wall", t_in)
    print("      %.2f GB/s of output" % (len(both) / m / 1e9), flush=True)
    m, _, _ = line("native.split_pairs", "wall", t_sp)
    print("      %.2f GB/s of input" % (len(both) / m / 1e9), flush=True)
    with tempfile.TemporaryDirectory() as tmp, native.Counter(K, native.ALPHABET_NT2) as ctx:
        tmp = Path(tmp)
        ctx.count_chunk(text, 1)
        for name, data in (("both.fa", both), ("r1.fa", one), ("r2.fa", two)):
            (tmp / name).write_bytes(data)
        t_two, t_one = [], []
        for i in range(2 + runs):
            t0 = time.perf_counter()
            kmers.trim_reads(ctx, tmp / "r1.fa", tmp / "o_1.fa", mate_file=tmp / "r2.fa", out_path2=tmp / "o_2.fa", singles_path=tmp / "s.fa")
            t1 = time.perf_counter()
            kmers.trim_reads(ctx, tmp / "both.fa", tmp / "o.fa", paired=True, singles_path=tmp / "s.fa")
            t2 = time.perf_counter()
            if i >= 2:
                t_two.append(t1 - t0)
                t_one.append(t2 - t1)
        assert native.interleave((tmp / "o_1.fa").read_bytes(), (tmp / "o_2.fa").read_bytes()) == (tmp / "o.fa").read_bytes()
        line("trim_reads, two files", "wall", t_two)
        line("trim_reads, interleaved", "wall", t_one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", type=str, default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from mercat2_amd import native
    import torch
    other = other_package(args.parent) if args.parent else native
    print(native.lib().mk_version().decode(), "|", native.library_path(), "|", torch.cuda.get_device_name(0), flush=True)
    print("the other leg:", other.library_path(), flush=True)
    text = native.synth_reads(1_000_000, 3, args.reads & ~1, READ, 4, 10000)
    ops_shape(native, other, text, args.runs)
    host_shape(native, text, args.runs)


if __name__ == "__main__":
    main()
