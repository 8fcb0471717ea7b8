"""The abundance histogram of a table on the GPU (mk_histo / mk_histo_device, Counter.histo*, native.histo_multi,
report.write_histo_*, -histo).  The expected histogram never comes from the code under test: it is the bincount of the count
column of a table the reference made, of ``export()`` of the same context, or of the counts written into a crafted TSV."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import read_input
from mercat2_amd import cli, native, report
from mercat2_amd.chunker import chunk_offsets

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).parent / "golden"
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE = -1, -4
MAX_HIGH = 1 << 20
M64 = (1 << 64) - 1


def _want(counts, high: int) -> np.ndarray:
    """bins[c] = rows with count c for c <= high, bins[high + 1] = rows above (rows with count 0 are not rows)."""
    counts = np.asarray(counts, dtype=np.uint64)
    counts = counts[counts != 0]
    return np.bincount(np.minimum(counts, np.uint64(high + 1)).astype(np.int64), minlength=high + 2).astype(np.uint64)


def _check(ctx, counts, high: int):
    """histo(high) of ctx against the counts its table is known to hold; returns (bins, info)."""
    py = [int(c) for c in counts if int(c)]
    info = {}
    bins = ctx.histo(high, info=info)
    assert bins.dtype == np.uint64 and bins.shape == (high + 2,)
    assert (bins == _want(counts, high)).all(), "high = %d" % high
    assert bins[0] == 0 and info["over_rows"] == int(bins[high + 1])
    assert info["distinct"] == int(bins.sum()) == len(py)
    assert info["total"] == sum(py) & M64
    assert info["max_count"] == max(py, default=0)
    assert info["over_total"] == sum(c for c in py if c > high) & M64
    assert info["s_scan"] >= 0 and info["s_total"] >= info["s_scan"]
    return bins, info


def _rows(path: Path, k: int):
    """(keys, counts) of a committed count table, by the row rules of the header: k key bytes, a tab, the count."""
    lines = path.read_bytes().split(b"\n")[1:]
    if lines[-1] == b"":
        lines.pop()
    assert all(line[k:k + 1] == b"\t" for line in lines)
    return [line[:k] for line in lines], [int(line[k + 1:]) for line in lines]


# ------------------------------------------------------------------------------- tables the reference made
# table -> (the golden input it came from, alphabet, min_count, chunk bytes)
REFERENCE = {
    "ref_RW1_clean_k5_c10": ("RW1_clean.fna.gz", NT, 10, 0),
    "ref_RW1_pro_k5_c10": ("RW1_pro.faa.gz", AA, 10, 0),
    "ref_RW1_fgs_k5_c10": ("RW1_fgs.faa.gz", AA, 10, 0),
    "ref_Test_R1_k5_c10": ("Test_R1.fna.gz", NT, 10, 0),
    "ref_DJ_pro_k5_c10_s1": ("DJ_pro.faa.gz", AA, 10, 1 << 20),
    "A_k31_c1": ("A.fasta", NT, 1, 0),
    "Scaffolds_with-NNN_k5_c10": ("Scaffolds_with-NNN.fna.gz", NT, 10, 0),
    "edge_ws_k3_c1": ("edge_ws.fa", NT, 1, 0),
    "edge_ws_k5_c1": ("edge_ws.fa", NT, 1, 0),
    "edge_ws_k31_c1": ("edge_ws.fa", NT, 1, 0),
    "edge_lengths_k32_c2": ("edge_lengths.fa", NT, 2, 0),
    "edge_protein_k3_c2": ("edge_protein.faa", AA, 2, 0),
}


@pytest.mark.parametrize("name", sorted(REFERENCE))
def test_reference_tables(name):
    source, alphabet, c, chunk = REFERENCE[name]
    path = GOLDEN / "tsv" / (name + ".tsv")
    k = native.tsv_shape(path)["k"]
    keys, counts = _rows(path, k)
    with native.Counter(k, alphabet) as counted, native.Counter(k, alphabet) as loaded:
        data = read_input(source)  # counted as the reference counted it: -s 1 cuts the inflated text into 1 MiB chunks
        offs = chunk_offsets(data, chunk) if chunk and len(data) >= chunk else [0, len(data)]
        for a, b in zip(offs[:-1], offs[1:]):
            counted.count_chunk(memoryview(data)[a:b], c)
        loaded.load_tsv(path)
        for ctx in (counted, loaded):
            for high in (10000, 10):
                bins, info = _check(ctx, counts, high)
                assert info["distinct"] == len(keys) and info["slots"] > 0
            if name == "edge_lengths_k32_c2":  # the key kept beside the one-word table
                assert counts[keys.index(b"T" * 32)] == 338 and ctx.histo(400)[338] >= 1 and ctx.histo(337)[338] >= 1


# ------------------------------------------------------------------------------------ every table shape
def _synth() -> bytes:
    # (the last record holds bytes outside both alphabets: keys kept as text in every packed context)
    return native.synth_reads(30_000, 3, 1_500, 150, 4).tobytes() + b">odd\n" + b"ACGTTGCANGGATCCATGNAacgtACGGT*CA" * 8 + b"\n"


SHAPES = [("nt", NT, k) for k in (3, 21, 31, 32, 33, 63, 64, 70)] + [("aa", AA, k) for k in (3, 5, 12, 13, 25)] + [("raw", RAW, 9)]


@pytest.mark.parametrize("kind,alphabet,k", SHAPES, ids=["%s_k%d" % (s[0], s[2]) for s in SHAPES])
def test_every_table_shape_against_export(kind, alphabet, k):
    with native.Counter(k, alphabet) as ctx:
        ctx.count_chunk(_synth(), 1)
        _, counts = ctx.export()
        top = int(counts.max())
        alpha = ctx.alpha_stats()
        highs = sorted({h for h in (1, 2, 7, top - 1, top, top + 1) if 1 <= h <= MAX_HIGH})
        assert len(highs) >= 4 and len(counts) == ctx.rows()
        for high in highs:
            bins, info = _check(ctx, counts, high)
            assert info["distinct"] == ctx.rows() == alpha["observed"] and info["total"] == alpha["total"]
            upto = min(high, 10)
            assert bins[1:upto + 1].tolist() == alpha["freq"][1:upto + 1]
            if high >= top:
                assert info["over_rows"] == 0 == info["over_total"]
            if high == top - 1:
                assert info["over_rows"] == int((counts == top).sum()) > 0


# ------------------------------------------------------------------------------------ crafted tables
def _window() -> int:
    text = (ROOT / "mercat2_amd" / "csrc" / "mk_histo.hip").read_text()
    return int(re.search(r"^#define\s+HS_WINDOW\s+(\d+)\s*$", text, flags=re.M).group(1))


def _table_text(counts) -> bytes:
    """A count table at k = 12, nucleotide: row i is the i-th 12-mer in base-4 order with counts[i]."""
    n = len(counts)
    digits = (np.arange(n, dtype=np.int64)[:, None] >> (2 * np.arange(11, -1, -1))) & 3
    keys = np.frombuffer(b"ACGT", dtype=np.uint8)[digits].view("S12").ravel().tolist()
    return b"".join(b"%s\t%d\n" % (key, c) for key, c in zip(keys, counts))


BIG = [(1 << 32) - 1, 1 << 32, 1 << 63, M64]


@functools.lru_cache(maxsize=None)
def _crafted(which: str):
    """(the table's text, its counts as Python ints)."""
    if which == "ramp":  # every bin from 1 to W + 300 holds one row, and four rows far above
        counts = list(range(1, _window() + 301)) + BIG
    elif which == "singletons":
        counts = [1] * 200_000
    else:  # one hot bin away from the first, ten rows beside it
        counts = [37] * 199_990 + list(range(1, 11))
    return _table_text(counts), counts


def test_the_lds_windows_edges_and_64_bit_counts():
    w = _window()
    text, counts = _crafted("ramp")
    n = w + 300
    with native.Counter(12, NT) as ctx:
        assert ctx.load_tsv(text)["rows"] == len(counts) == n + 4
        for high in (w - 2, w - 1, w, w + 1, n, MAX_HIGH):
            bins, info = _check(ctx, counts, high)
            assert bins[1:min(high, n) + 1].tolist() == [1] * min(high, n) and not bins[n + 1:high + 1].any()
            assert int(bins[high + 1]) == 4 + max(0, n - high)
            assert info["max_count"] == M64
            assert info["over_total"] == (sum(BIG) + sum(range(high + 1, n + 1))) % (1 << 64)


@pytest.mark.parametrize("which", ["singletons", "hot_bin"])
def test_skewed_tables(which):
    text, counts = _crafted(which)
    with native.Counter(12, NT) as ctx:
        assert ctx.load_tsv(text)["rows"] == 200_000
        for high in (10000, 5):
            bins, info = _check(ctx, counts, high)
            assert info["slots"] >= 2 * 200_000  # (several workgroups)
        if which == "singletons":
            assert int(ctx.histo(1)[1]) == 200_000
        else:
            assert int(ctx.histo(100)[37]) == 199_990 and int(ctx.histo(5)[6]) == 199_995


# ------------------------------------------------------------------------------------ state and arguments
@pytest.mark.parametrize("alphabet,k", [(NT, 3), (NT, 31), (NT, 63), (AA, 13), (RAW, 9), (NT, 70)])
def test_empty_context_gives_zeros(alphabet, k):
    with native.Counter(k, alphabet) as ctx:
        info = {}
        bins = ctx.histo(100, info=info)
        assert bins.shape == (102,) and not bins.any()
        assert all(info[f] == 0 for f in ("distinct", "total", "max_count", "over_rows", "over_total"))


def test_arguments_and_state():
    L = native.lib()
    with native.Counter(31, NT) as ctx:
        ctx.count_chunk(_synth(), 1)
        _, counts = ctx.export()
        for high in (0, MAX_HIGH + 1):
            with pytest.raises(native.MercatHipError) as e:
                ctx.histo(high)
            assert e.value.code == ARG
        bins = np.zeros(12, dtype=np.uint64)
        assert L.mk_histo(ctx._h, 10, None, None) == ARG and L.mk_histo_device(ctx._h, 10, None, None) == ARG
        assert L.mk_histo(ctx._h, 10, bins.ctypes.data, None) == 0 and (bins == _want(counts, 10)).all()  # (st may be NULL)
        assert L.mk_chunk_begin(ctx._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            ctx.histo(10)
        assert e.value.code == STATE and "chunk is open" in str(e.value)
        assert L.mk_chunk_end(ctx._h, 1) == 0
        first = ctx.histo(10000)
        assert (first == ctx.histo(10000)).all() and (first == _want(counts, 10000)).all()  # called twice; the table only read
        after = ctx.export()[1]
        assert (after == counts).all()
        ctx.trim()
        _check(ctx, counts, 10000)


@pytest.mark.parametrize("alphabet,k", [(NT, 31), (NT, 5), (NT, 63)])
def test_the_tail_of_the_histogram_is_what_a_filter_keeps(alphabet, k):
    c = 9
    with native.Counter(k, alphabet) as ctx:
        ctx.count_chunk(_synth(), 1)
        before = ctx.histo(10000)
        assert before[1:c].any()
        ctx.filter_min(c)
        assert int(before[c:].sum()) == ctx.rows() > 0
        _, counts = ctx.export()
        bins, _ = _check(ctx, counts, 10000)
        assert not bins[1:c].any() and (bins[c:] == before[c:]).all()


def test_device_form_equals_the_host_form():
    import torch
    with native.Counter(31, NT) as ctx:
        ctx.count_chunk(_synth(), 1)
        for high in (3, 10000):
            d_out = torch.full((high + 2,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            info_dev, info = ctx.histo_device(high, d_out.data_ptr()), {}
            want = ctx.histo(high, info=info)
            assert (d_out.cpu().numpy().view(np.uint64) == want).all() and want.sum() == ctx.rows()
            for f in ("distinct", "total", "max_count", "over_rows", "over_total", "slots"):
                assert info_dev[f] == info[f]


# ------------------------------------------------------------------------------------ spread tables
@pytest.mark.parametrize("n,k", [(2, 32), (3, 31), (3, 63), (2, 3)])
def test_histo_multi_over_key_ranges(n, k):
    data = native.synth_reads(50_000, 3, 4_000, 150, 4).tobytes() + b">polyT\n" + b"T" * 200 + b"\n"
    offs = chunk_offsets(data, len(data) // 5)
    assert len(offs) > 4
    ctxs = [native.Counter(k, NT) for _ in range(n)]
    try:
        for i, (a, b) in enumerate(zip(offs[:-1], offs[1:])):  # chunk i -> context i mod n
            ctxs[i % n].count_chunk(memoryview(data)[a:b], 1)
        native.merge_devices(ctxs, native.MERGE_RANGES)
        _, counts = native.export_multi(ctxs)
        for high in (10000, 4):
            assert (native.histo_multi(ctxs, high) == _want(counts, high)).all()
        assert int(native.histo_multi(ctxs, 10).sum()) == native.rows_multi(ctxs) == len(counts)
    finally:
        for c in ctxs:
            c.close()


# -------------------------------------------------------------------------------------------------- CLI
def test_cli_histo_counted_and_loaded(tmp_path, capsys):
    inputs = [str(GOLDEN / "inputs" / name) for name in ("A.fasta", "B.fasta")]
    out, again = tmp_path / "out", tmp_path / "again"
    assert cli.main(["-i"] + inputs + ["-k", "5", "-c", "1", "-skipclean", "-histo", "50", "-o", str(out)]) == 0
    assert "histo_nucleotide.tsv:" in capsys.readouterr().out
    assert cli.main(["-tsv", str(out), "-k", "5", "-histo", "50", "-o", str(again)]) == 0
    bins = {}
    for sample in ("A", "B"):
        _, counts = _rows(out / "tsv_nucleotide" / (sample + "_counts.tsv"), 5)
        bins[sample] = _want(counts, 50)
        text = (out / "histo_nucleotide" / (sample + "_histo.txt")).read_bytes()
        assert text == report.format_histo(bins[sample]) and text
        assert (again / "histo_nucleotide" / (sample + "_histo.txt")).read_bytes() == text
    table = (out / "histo_nucleotide.tsv").read_bytes()
    lines = table.split(b"\n")
    assert lines[0] == b"count\tA\tB" and lines[-1] == b""
    want_rows = [b"%d\t%d\t%d" % (i, bins["A"][i], bins["B"][i]) for i in range(1, 52) if bins["A"][i] or bins["B"][i]]
    assert lines[1:-1] == want_rows and want_rows
    assert (again / "histo_nucleotide.tsv").read_bytes() == table
    # the same files through the report layer, by hand
    with native.Counter(5, NT) as a, native.Counter(5, NT) as b:
        a.load_tsv(out / "tsv_nucleotide" / "A_counts.tsv")
        b.load_tsv(out / "tsv_nucleotide" / "B_counts.tsv")
        report.write_histo_files({"A": a, "B": b}, tmp_path / "hand", 50)
        assert report.write_histo_tsv({"A": a, "B": b}, tmp_path / "hand.tsv", 50) == len(want_rows)
        assert (tmp_path / "hand" / "B_histo.txt").read_bytes() == (out / "histo_nucleotide" / "B_histo.txt").read_bytes()
        assert (tmp_path / "hand.tsv").read_bytes() == table
