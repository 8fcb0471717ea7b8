"""Reads thinned to a target depth by their median k-mer count on the GPU (mk_norm_text / mk_norm_device,
Counter.normalize*, kmers.normalize_reads, report.write_norm_tsv, -norm), and the median of a long record by selection
(mk_track_* and mk_norm_*).  Expected values never come from the code under test: the rule is tests/norm_rule.py (the
reference's line loop, the median, splitmix64 and the decision in plain Python), the medians of the long records are
numpy.sort's, the table is a crafted dict loaded with Counter.load_tsv or the CPU oracle's count of a source text.
Equality is exact everywhere."""
import ctypes
import functools
import gzip
import random
import zlib

import numpy as np
import pytest

import norm_rule
import trim_rule
import walk_seams
from mercat2_amd import cli, kmers, native
from oracle import cpu_ref
from test_gpu_trim import COMP, SPACES, dna, fastq_text, halves_source, load, shapes, wrap

pytestmark = pytest.mark.gpu
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE, NON_ASCII, RANGE = -1, -4, -5, -7
CLIP = 2 ** 32 - 1
SELECT_MIN = native.MEDIAN_SELECT_MIN
COUNTS = ("records_out", "records_short", "records_low", "records_over", "records_thinned")
VALUES = (1, 2, 3, 3, 8, 8, 9, 9, 40, 1000, 5_000_000_000)  # below min_depth 3, at it, at target 8, above it, far above, clipped


def hashed(text: bytes, k: int, values=VALUES) -> dict:
    """Every window of the text (but those that hold a blank: no table line can carry one) at a count its bytes choose."""
    table = {}
    for _, seq in trim_rule.records(text):
        for j in range(len(seq) - k + 1):
            w = seq[j:j + k]
            if not SPACES & set(w):
                table[w.decode()] = values[zlib.crc32(w) % len(values)]
    return table


def check(ctx, text: bytes, table: dict, target: int, min_depth: int = 0, seed: int = 0, invert: bool = False, fold=None,
          folded_table: bool = False, want=None, **kw):
    """Counter.normalize against the rule: bytes, keep, median, rows (those of Counter.screen) and the figures."""
    info = {}
    out, keep, med, rows = ctx.normalize(text, target, min_depth, seed, invert, fold=fold, info=info, **kw)
    want = want or norm_rule.expected(text, table, ctx.k, target, min_depth, seed, invert, folded_table)
    assert med.dtype == np.uint32 and med.tolist() == want["median"]
    assert keep.dtype == bool and keep.tolist() == want["keep"]
    assert out == want["out"]
    assert rows.tolist() == ctx.screen(text, max(min_depth, 1), fold=fold, **kw).tolist()
    assert [int(w) for w in rows[:, 0]] == want["windows"]
    assert {n: info[n] for n in COUNTS} == {n: want[n] for n in COUNTS}
    assert info["records"] == len(want["keep"]) and info["bytes"] == len(text) and info["bytes_out"] == len(out) <= len(text)
    assert info["preamble"] == norm_rule.preamble(text)
    return (out, keep, med, rows), info, want


# --------------------------------------------------------------------------------------------- record shapes
@functools.lru_cache(maxsize=None)
def shaped_text(k: int, headless: bool):
    """test_gpu_trim.shapes and five records whose windows all hold one count: 2, 3, 8, 9 and 5 * 10^9."""
    text, _ = shapes(k, headless)
    flat = [("A", 2), ("C", 3), ("G", 8), ("T", 9)]
    extra = "\n" + "".join(">flat %s\n%s\n" % (c, c * (k + 3)) for c, _ in flat) + ">flat AC\n" + "AC" * (k // 2 + 3)
    text = text + extra.encode()
    table = hashed(text, k)
    for c, v in flat:
        table[c * k] = v
    for w in {("AC" * k)[:k], ("CA" * k)[:k]}:
        table[w] = 5_000_000_000
    return text, table


SHAPE_CONTEXTS = [("nt_k5", NT, 5), ("nt_k31", NT, 31), ("nt_k33", NT, 33), ("aa_k3", AA, 3), ("raw_k9", RAW, 9)]


@pytest.mark.parametrize("headless", [False, True], ids=["blanks_first", "headless"])
@pytest.mark.parametrize("name,alphabet,k", SHAPE_CONTEXTS, ids=[c[0] for c in SHAPE_CONTEXTS])
def test_record_shapes(name, alphabet, k, headless):
    text, table = shaped_text(k, headless)
    with native.Counter(k, alphabet) as ctx:
        load(ctx, table)
        (out, keep, med, rows), info, want = check(ctx, text, table, 8, 3)
        assert info["headless"] == (1 if headless else 0) and info["pieces"] == 1
        assert info["preamble"] == (0 if headless else len("  \n\t\n \x0b\n"))
        # the five flat records: below min_depth, at it, at the target, one above it, clipped
        assert med.tolist()[-5:] == [2, 3, 8, 9, CLIP] and keep.tolist()[-5:-2] == [False, True, True] and not keep[-1]
        assert want["records_short"] >= 2 and want["records_low"] >= 1 and want["records_over"] >= 2 and want["records_thinned"] >= 1
        assert 0 < info["records_out"] < info["records"]
        (out_i, keep_i, _, _), info_i, _ = check(ctx, text, table, 8, 3, invert=True)
        # the two outputs partition the text minus its preamble
        assert (keep != keep_i).all() and len(out) + len(out_i) + info["preamble"] == len(text)
        pos = info["preamble"]
        for raw, _ in norm_rule.records(text):
            assert text[pos:pos + len(raw)] == raw
            pos += len(raw)
        assert pos == len(text) and info_i["records_out"] + info["records_out"] == info["records"]
        for counts in COUNTS[1:]:
            assert info[counts] == info_i[counts]
        check(ctx, text, table, 8, 0)   # no lower bound: only the records without windows are dropped
        check(ctx, text, table, 2, 9, seed=5)  # min_depth above target: nothing between them
        assert [x.tolist() if hasattr(x, "tolist") else x for x in ctx.normalize(b"", 8)] == [b"", [], [], []]
        out, keep, med, rows = ctx.normalize(b"\n  \n", 8)
        assert (out, keep.tolist(), med.tolist(), rows.shape) == (b"", [], [], (0, 5))


# ------------------------------------------------------------------------------------------- call-wide index
def test_the_record_index_runs_over_the_whole_call():
    k = 31
    rng = random.Random(11)
    text = "".join(">d%d\n%s\n" % (i, dna(rng, 60)) for i in range(300)).encode()
    table = hashed(text, k, values=(80,))
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        one, info, want = check(ctx, text, table, 20)
        many, info_p, _ = check(ctx, text, table, 20, piece_bytes=4096)
        assert info["pieces"] == 1 and info_p["pieces"] >= 4
        assert one[0] == many[0] and one[1].tolist() == many[1].tolist()
        assert want["records_over"] == 300 and abs(info["records_out"] - 75) <= 38  # (5 sigma of Binomial(300, 1 / 4) is 37.5)
        other, _, _ = check(ctx, text, table, 20, seed=1, piece_bytes=4096)
        assert other[1].tolist() != one[1].tolist()
        # a piece-local index would repeat the first piece's draws in every piece
        first = int(np.searchsorted(np.cumsum([len(raw) for raw, _ in norm_rule.records(text)]), 4096))
        assert one[1][first:2 * first].tolist() != one[1][:first].tolist()


# ------------------------------------------------------------------------------------------------ tile seams
def test_tile_seams():
    """Three tiles of the walk: a separator on a tile seam, records that cross the second and the third."""
    k = 31
    T = walk_seams.TILE
    rng = random.Random(2)
    lengths = [100, T - 102, T + 4, 40, T, 50]
    recs = [("s%d" % i, dna(rng, n)) for i, n in enumerate(lengths)]
    seps, end = walk_seams.separators(recs)
    assert [p for p, _, _ in seps][:3] == [0, 101, T] and seps[3][0] == 2 * T + 5 and seps[4][0] < 3 * T < seps[5][0] and end > 3 * T
    text = "".join(">%s\n%s" % (name, walk_seams._wrap(seq, 70)) for name, seq in recs).encode()
    table = hashed(text, k)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        one, _, want = check(ctx, text, table, 8, 3)
        assert len(set(want["median"])) >= 2 and 0 < want["records_out"] < len(lengths)
        many, info_p, _ = check(ctx, text, table, 8, 3, want=want, piece_bytes=T)
        assert info_p["pieces"] > 1 and one[0] == many[0]


# ------------------------------------------------------------------------------------------------- selection
CODE = np.full(256, 255, dtype=np.uint8)
CODE[[ord(c) for c in "ACGT"]] = range(4)
K5 = 5


def kmer5_counts(seq: str, lut: np.ndarray) -> np.ndarray:
    """The count under every 5-mer window of a sequence of ACGT from lut[its 2-bit code], by numpy."""
    c = CODE[np.frombuffer(seq.encode(), dtype=np.uint8)].astype(np.int64)
    n = len(c) - K5 + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    code = sum(c[j:j + n] << (2 * (K5 - 1 - j)) for j in range(K5))
    return lut[code]


def lut_table(lut: np.ndarray) -> dict:
    return {"".join("ACGT"[(code >> (2 * (K5 - 1 - j))) & 3] for j in range(K5)): int(v) for code, v in enumerate(lut) if v}


def code_of(kmer: str) -> int:
    return int(sum(int(CODE[ord(ch)]) << (2 * (K5 - 1 - j)) for j, ch in enumerate(kmer)))


def selection_case(name: str):
    """(lut of the 1024 5-mers, [sequences of the long records])."""
    rng = random.Random(name)
    codes = np.arange(1024, dtype=np.uint64)
    w = SELECT_MIN + 1000
    long_seq = dna(rng, w + K5 - 1)
    if name == "top_byte":
        return ((codes % 200) + 1) << np.uint64(24), [long_seq]
    if name == "low_byte":
        return np.uint64(0x12345600) | (codes & np.uint64(255)), [long_seq]
    if name == "all_four":  # and two long records side by side: tiles that hold the end of one and the start of the next
        return (codes * np.uint64(2654435761)) % np.uint64(2 ** 32 - 5) + np.uint64(1), [long_seq, dna(rng, SELECT_MIN + K5)]
    if name == "clipped":
        lut = (codes * np.uint64(2654435761)) % np.uint64(2 ** 32)
        lut[codes % 5 < 3] = 5_000_000_000
        return lut, [long_seq]
    if name == "all_equal":
        return np.full(1024, 7, dtype=np.uint64), [long_seq]
    if name == "absent":  # (a contig the table lacks: the table holds TTTTT alone, the record no T)
        lut = np.zeros(1024, dtype=np.uint64)
        lut[code_of("TTTTT")] = 5
        return lut, ["".join(rng.choice("ACG") for _ in range(w + K5 - 1))]
    if name == "homopolymer":
        return codes + np.uint64(3), ["A" * (w + K5 - 1)]
    # A^m C^n: m - 4 windows AAAAA at 1000, four mixed ones and n - 4 windows CCCCC at 70 000
    lut = np.full(1024, 70_000, dtype=np.uint64)
    lut[code_of("AAAAA")] = 1000
    m = w // 2 + (5 if name == "rank_last_a" else 4)
    return lut, ["A" * m + "C" * (w + K5 - 1 - m)]


SELECTION = ("top_byte", "low_byte", "all_four", "clipped", "all_equal", "absent", "homopolymer", "rank_last_a", "rank_first_after")


@pytest.mark.parametrize("name", SELECTION)
def test_the_median_of_a_long_record_is_selected(name):
    lut, longs = selection_case(name)
    rng = random.Random(4)
    seqs = [dna(rng, 40 + i) for i in range(6)] + longs + [dna(rng, 90), "ACG", dna(rng, SELECT_MIN + K5 - 1), dna(rng, 33)]
    text = "".join(">q%d\n%s" % (i, wrap(s, 80) if i % 2 else s + "\n") for i, s in enumerate(seqs)).encode()
    counts = [kmer5_counts(s, lut) for s in seqs]
    assert [len(c) for c in counts][6] == SELECT_MIN + 1000 and len(counts[-2]) == SELECT_MIN  # (that one is still sorted)
    want64 = [int(np.sort(c)[len(c) // 2]) if len(c) else 0 for c in counts]
    want32 = [min(v, CLIP) for v in want64]
    if name == "rank_last_a":
        assert want64[6] == 1000 and int(np.sort(counts[6])[len(counts[6]) // 2 + 1]) == 70_000
    if name == "rank_first_after":
        assert want64[6] == 70_000 and int(np.sort(counts[6])[len(counts[6]) // 2 - 1]) == 1000
    if name == "clipped":
        assert want64[6] == 5_000_000_000
    with native.Counter(K5, NT) as ctx:
        load(ctx, lut_table(lut))
        info = {}
        out, keep, med, rows = ctx.normalize(text, CLIP, info=info)
        assert med.tolist() == want32 and keep.tolist() == [len(c) > 0 for c in counts] and info["pieces"] == 1
        assert [int(x) for x in rows[:, 0]] == [len(c) for c in counts]
        got, offsets, _, med64 = ctx.track(text, median=True)
        assert med64.dtype == np.uint64 and med64.tolist() == want64
        assert got.tolist() == np.concatenate(counts).tolist()
        got, _, _, med32 = ctx.track(text, median=True, sat32=True)
        assert med32.dtype == np.uint32 and med32.tolist() == want32
        _, _, med_p, _ = ctx.normalize(text, CLIP, piece_bytes=2 * SELECT_MIN)  # the long records in pieces of their own
        assert med_p.tolist() == want32


def test_a_clipped_median_is_kept_at_the_largest_target():
    k = 31
    rng = random.Random(8)
    text = (">deep\n%s\n>shallow\n%s\n" % (dna(rng, 50), dna(rng, 50))).encode()
    table = hashed(text, k, values=(3,))
    table.update({w: 5_000_000_000 for w in hashed(text[:text.index(b">shallow")], k)})
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (_, keep, med, _), info, _ = check(ctx, text, table, CLIP)
        assert med.tolist() == [CLIP, 3] and keep.all() and info["records_over"] == 0
        (_, keep, _, _), info, _ = check(ctx, text, table, CLIP - 1, seed=3)
        assert info["records_over"] == 1


# ------------------------------------------------------------------------------------------------ device call
@functools.lru_cache(maxsize=None)
def mixed_text(k: int):
    rng = random.Random(5 * k)
    head, _ = shapes(k, True)
    reads = "".join(">m%d\n%s\n" % (i, dna(rng, 150)) for i in range(200))
    return head + b"\n" + reads.encode() + (">contig\n" + wrap(dna(rng, 9_000), 60)).encode()


@pytest.mark.parametrize("out_lead", [0, 1, 15])
def test_norm_device_agrees(out_lead):
    import torch
    k = 31
    text = mixed_text(k)
    table = hashed(text, k)
    want = norm_rule.expected(text, table, k, 8, 3, seed=9)
    no, nr = len(want["out"]), len(want["keep"])
    lead = 3  # the text at an odd address
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        w_rows = ctx.screen(text, 3)
        d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((out_lead + no + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_med = torch.full((nr + 1,), -1, dtype=torch.int32, device="cuda")
        d_keep = torch.full((nr + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rows = torch.full((nr + 1, 5), -1, dtype=torch.int64, device="cuda")
        assert d_out.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        info = ctx.normalize_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, no, 8, d_med.data_ptr(),
                                    d_keep.data_ptr(), d_rows.data_ptr(), nr, min_depth=3, seed=9)
        got = d_out.cpu().numpy()
        assert info["bytes_out"] == no and info["records"] == nr and info["pieces"] == 1
        assert {n: info[n] for n in COUNTS} == {n: want[n] for n in COUNTS}
        assert got[out_lead:out_lead + no].tobytes() == want["out"]
        assert (got[:out_lead] == 0xA5).all() and (got[out_lead + no:] == 0xA5).all()
        assert d_med.cpu().numpy().view(np.uint32)[:nr].tolist() == want["median"] and int(d_med[nr]) == -1
        assert d_keep.cpu().numpy()[:nr].astype(bool).tolist() == want["keep"] and int(d_keep[nr]) == 0xA5
        assert d_rows.cpu().numpy().view(np.uint64)[:nr].tolist() == w_rows.tolist() and (d_rows[nr] == -1).all().item()
        with pytest.raises(native.MercatHipError) as e:
            ctx.normalize_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, no - 1, 8, min_depth=3, seed=9)
        assert e.value.code == RANGE
        with pytest.raises(native.MercatHipError) as e:
            ctx.normalize_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr(), no, 8, d_med.data_ptr() + 2, 0, 0, nr)
        assert e.value.code == ARG and "aligned" in str(e.value)
        with pytest.raises(native.MercatHipError) as e:
            ctx.normalize_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr(), no, 8, 0, 0, d_rows.data_ptr() + 4, nr)
        assert e.value.code == ARG


# ------------------------------------------------------------------------------------------ errors and state
GUARD = 0xA5A5A5A5A5A5A5A5


def _raw(ctx, text: bytes, out_cap: int, cap: int, flags: int = 0, rule=(8, 3, 0), null_out: bool = False, null_rule: bool = False,
         piece_bytes: int = 0):
    """mk_norm_text into 0xA5-guarded buffers one element longer than the capacities it is told."""
    out = np.full(out_cap + 1, 0xA5, dtype=np.uint8)
    md = np.full(cap + 1, 0xA5A5A5A5, dtype=np.uint32)
    kp = np.full(cap + 1, 0xA5, dtype=np.uint8)
    rw = np.full((cap + 1, 5), GUARD, dtype=np.uint64)
    out_len, n, st = ctypes.c_size_t(0), ctypes.c_size_t(0), native.Norm()
    r = native.NormRule(*rule)
    rc = native.lib().mk_norm_text(ctx._h, text, len(text), piece_bytes, flags, None if null_rule else ctypes.byref(r),
                                   None if null_out else out.ctypes.data, out_cap, ctypes.byref(out_len), md.ctypes.data,
                                   kp.ctypes.data, rw.ctypes.data, cap, ctypes.byref(n), ctypes.byref(st))
    return {"rc": rc, "out_len": out_len.value, "nrows": n.value, "out": out, "median": md, "keep": kp, "rows": rw, "st": st}


def test_capacities():
    k = 31
    text = mixed_text(k)
    table = hashed(text, k)
    want = norm_rule.expected(text, table, k, 8, 3)
    no, nr = len(want["out"]), len(want["keep"])
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        for piece_bytes in (0, 4096):
            got = _raw(ctx, text, no, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (0, no, nr) and got["st"].bytes_out == no
            assert got["out"][:no].tobytes() == want["out"] and got["out"][no] == 0xA5
            assert got["median"][:nr].tolist() == want["median"] and got["median"][nr] == 0xA5A5A5A5
            assert got["keep"][:nr].astype(bool).tolist() == want["keep"] and got["keep"][nr] == 0xA5
            assert (got["rows"][nr] == GUARD).all()
            # out_cap one short: both needed sizes, nothing past the cap
            got = _raw(ctx, text, no - 1, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr) and got["out"][no - 1] == 0xA5
            assert "bytes" in ctx._L.mk_last_error(ctx._h).decode()
            # cap one short
            got = _raw(ctx, text, no, nr - 1, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr)
            assert (got["rows"][nr - 1] == GUARD).all() and got["keep"][nr - 1] == 0xA5 and got["median"][nr - 1] == 0xA5A5A5A5
            # the sizing call
            got = _raw(ctx, text, 0, 0, null_out=True, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr)
            assert (got["rows"] == GUARD).all() and (got["keep"] == 0xA5).all()
        # median, keep and rows NULL (cap is ignored), st NULL
        out = np.full(no + 1, 0xA5, dtype=np.uint8)
        out_len, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        r = native.NormRule(8, 3, 0)
        rc = native.lib().mk_norm_text(ctx._h, text, len(text), 0, 0, ctypes.byref(r), out.ctypes.data, no, ctypes.byref(out_len), None,
                                       None, None, 0, ctypes.byref(n), None)
        assert (rc, out_len.value, n.value) == (0, no, nr) and out[:no].tobytes() == want["out"] and out[no] == 0xA5


def test_errors_and_state():
    k = 31
    text, table = shaped_text(k, False)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        before, size = ctx.to_dict(), ctx.rows()
        check(ctx, text, table, 8, 3)
        assert ctx.rows() == size and ctx.to_dict() == before
        for rule, word in (((0, 0, 0), "target"), ((2 ** 32, 0, 0), "target"), ((8, 2 ** 32, 0), "min_depth")):
            got = _raw(ctx, text, len(text), 64, rule=rule)
            assert got["rc"] == ARG and word in ctx._L.mk_last_error(ctx._h).decode() and (got["out"] == 0xA5).all()
        got = _raw(ctx, text, len(text), 64, flags=4)
        assert got["rc"] == ARG and "flag" in ctx._L.mk_last_error(ctx._h).decode()
        got = _raw(ctx, text, len(text), 64, null_rule=True)
        assert got["rc"] == ARG and "rule" in ctx._L.mk_last_error(ctx._h).decode()
        got = _raw(ctx, text, len(text), 64, rule=(CLIP, CLIP, 2 ** 64 - 1))
        assert got["rc"] == 0
        with pytest.raises(native.NonAsciiInput):
            ctx.normalize(b">a\nACGT\xc3\xa9ACGT\n", 8)
        with pytest.raises(native.MercatHipError) as e:  # a plain table, folding asked for: refused as screen refuses it
            ctx.normalize(text, 8, fold=True)
        assert e.value.code == ARG
        assert ctx._L.mk_chunk_begin(ctx._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            ctx.normalize(text, 8)
        assert e.value.code == STATE
        assert ctx._L.mk_chunk_end(ctx._h, 1) == 0
        assert ctx.to_dict() == before


# ------------------------------------------------------------------------------------------------------ fold
def test_canonical_fold():
    k = 31
    rng = random.Random(5)
    reads = [dna(rng, 150) for _ in range(40)]
    source = "".join(">s%d\n%s\n" % (i, r[:100 + i]) for i, r in enumerate(reads)).encode() + \
        "".join(">t%d\n%s\n" % (i, r[:120]) for i, r in enumerate(reads[:20])).encode()
    text = "".join(">f%d\n%s\n>r%d\n%s\n" % (i, r, i, r.translate(COMP)[::-1]) for i, r in enumerate(reads)).encode()
    folded = cpu_ref.canonical_fold(cpu_ref.count_text(source, k, 1))
    with native.Counter(k, NT, canonical=True) as ctx:
        ctx.count_chunk(source, 1)
        (_, _, med, _), info, _ = check(ctx, text, folded, 1, 1, folded_table=True)  # fold=None: as the context counts
        assert med[0::2].tolist() == med[1::2].tolist() and set(med.tolist()) == {1, 2} and info["folded"] > 0
        assert info["records_over"] == 40
        check(ctx, text, folded, 1, 1, fold=True, folded_table=True)
        (_, _, med, _), _, _ = check(ctx, text, folded, 1, fold=False)  # taken as they stand: one strand misses
        assert med[0::2].tolist() != med[1::2].tolist()


# ------------------------------------------------------------------------------------------------ files and CLI
def test_normalize_reads_fasta_gz_fastq(tmp_path):
    k = 11
    fq, fa = fastq_text(11, 120)
    # every count of 0 .. 3: the halves, and every other read once more
    source = halves_source(fa) + b"".join(b">c%d\n%s\n" % (i, seq) for i, (_, seq) in enumerate(trim_rule.records(fa)) if i % 2 == 0)
    table = cpu_ref.count_text(source, k, 1)
    for name, data in (("r.fna", fa), ("r.fna.gz", gzip.compress(fa)), ("r.fastq", fq), ("r.fq.gz", gzip.compress(fq))):
        (tmp_path / name).write_bytes(data)
    names = kmers.record_names(fa)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(source, 1)
        for target, min_depth, seed, invert in ((1, 1, 0, False), (1, 0, 7, True)):
            want = norm_rule.expected(fa, table, k, target, min_depth, seed, invert)
            assert 0 < want["records_out"] < len(want["keep"]) and want["records_thinned"] > 0
            for name in ("r.fna", "r.fna.gz", "r.fastq", "r.fq.gz"):
                for dest in ("o.fna", "o.fna.gz"):
                    res = kmers.normalize_reads(ctx, tmp_path / name, tmp_path / dest, target, min_depth, seed, invert,
                                                tsv_path=tmp_path / "o.tsv")
                    data = (tmp_path / dest).read_bytes()
                    if dest.endswith(".gz"):
                        assert data[:2] == b"\x1f\x8b"
                        data = gzip.decompress(data)
                    assert data == want["out"], (name, dest)
                    assert res == {"records": len(want["keep"]), "kept": want["records_out"], "short": want["records_short"],
                                   "low": want["records_low"], "over": want["records_over"], "thinned": want["records_thinned"],
                                   "bytes_out": len(want["out"])}
                    assert (tmp_path / "o.tsv").read_bytes() == b"record\twindows\tmedian\tkept\n" + b"".join(
                        b"%s\t%d\t%d\t%d\n" % (n.encode(), w, m, kp) for n, w, m, kp in zip(names, want["windows"], want["median"], want["keep"]))


def test_cli_norm(tmp_path):
    k = 7
    rng = random.Random(3)
    samples = {"one": "".join(">a%d\n%s\n" % (i, dna(rng, 60)) for i in range(6)), "two": "".join(">b%d\n%s\n" % (i, dna(rng, 60)) for i in range(6))}
    for base, data in samples.items():
        (tmp_path / (base + ".fna")).write_text(data * 2)  # (every k-mer twice)
    one, two = (trim_rule.records(samples[b].encode()) for b in ("one", "two"))
    reads = b"".join(b">o%d x\n%s\n" % (i, one[i % 6][1][i:i + 40]) for i in range(12)) + b">from two\n" + two[4][1][:30] + \
        b"\n  >neither\n" + dna(rng, 40).encode() + b"\n>short\nACG\n>both\n" + one[0][1][:20] + b"\n" + two[0][1][:20] + b"\n"
    (tmp_path / "reads.fa").write_bytes(reads)
    names = kmers.record_names(reads)
    for extra, rule, stem in (([], (20, 0, 0), "kept"), (["-norm_target", "1", "-norm_min", "1", "-norm_seed", "4"], (1, 1, 4), "kept"),
                              (["-norm_target", "1", "-norm_keep", "tossed"], (1, 0, 0), "tossed")):
        out = tmp_path / ("out%d" % len("".join(extra)))
        argv = ["-i", str(tmp_path / "one.fna"), str(tmp_path / "two.fna"), "-k", str(k), "-c", "1", "-skipclean", "-o", str(out),
                "-norm", str(tmp_path / "reads.fa")]
        assert cli.main(argv + extra) == 0
        for base, data in samples.items():
            table = cpu_ref.count_text((data * 2).encode(), k, 1)
            want = norm_rule.expected(reads, table, k, *rule, invert=stem == "tossed")
            assert (out / "norm_nucleotide" / ("%s_%s.fna" % (base, stem))).read_bytes() == want["out"]
            tsv = b"record\twindows\tmedian\tkept\n" + b"".join(
                b"%s\t%d\t%d\t%d\n" % (n.encode(), w, m, kp) for n, w, m, kp in zip(names, want["windows"], want["median"], want["keep"]))
            assert (out / "norm_nucleotide" / ("%s_norm.tsv" % base)).read_bytes() == tsv
            if rule[0] == 1 and base == "one":
                assert want["records_over"] >= 12 and 0 < want["records_thinned"] < want["records_over"]
        assert sorted(p.name for p in (out / "norm_nucleotide").iterdir()) == sorted(
            "%s_%s" % (b, f) for b in samples for f in ("norm.tsv", stem + ".fna"))
        assert not (out / "norm_protein").exists()
