"""Reads trimmed at their first low-abundance k-mer on the GPU (mk_trim_text / mk_trim_device, Counter.trim*,
kmers.trim_reads, report.write_trim_tsv, -trim).  Expected values never come from the code under test: the rule is
tests/trim_rule.py (the reference's line loop and khmer's trim_on_abundance in plain Python), the table is a dict -- every
window of the text at count 5 and chosen windows at 1, loaded with Counter.load_tsv, or the CPU oracle's count of a
source text.  Equality is exact everywhere."""
import ctypes
import functools
import gzip
import random

import numpy as np
import pytest

import trim_rule
import walk_seams
from mercat2_amd import cli, kmers, native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE, NON_ASCII, RANGE = -1, -4, -5, -7
COMP = str.maketrans("ACGT", "TGCA")
SPACES = set(b" \t\x0b\x0c")


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def wrap(seq, width):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


def crafted(text: bytes, k: int, low, high: int = 5) -> dict:
    """Every window of the text at ``high``, the windows (record, index) of ``low`` at 1.  A window that holds a blank is
    left out (no table line can carry it): it is absent, so low."""
    recs = trim_rule.records(text)
    table = {}
    for _, seq in recs:
        for j in range(len(seq) - k + 1):
            w = seq[j:j + k]
            if not SPACES & set(w):
                table[w.decode()] = high
    for r, j in low:
        seq = recs[r][1]
        assert 0 <= j <= len(seq) - k, (r, j)
        table[seq[j:j + k].decode()] = 1
    return table


def load(ctx, table: dict):
    assert ctx.load_tsv(b"".join(b"%s\t%d\n" % (key.encode(), c) for key, c in table.items()))["rows"] == len(table)


def check(ctx, text: bytes, table: dict, at_least: int = 2, min_len: int = 0, fold=None, folded_table: bool = False, want=None, **kw):
    """Counter.trim against the rule: bytes, kept, rows (those of Counter.screen) and the figures."""
    info = {}
    out, kept, rows = ctx.trim(text, at_least, min_len, fold=fold, info=info, **kw)
    w_out, w_kept = want if want is not None else trim_rule.expected(text, table, ctx.k, at_least, min_len, folded_table)
    lengths = [len(seq) for _, seq in trim_rule.records(text)]
    assert kept.dtype == np.uint64 and kept.tolist() == w_kept
    assert out == w_out
    assert rows.tolist() == ctx.screen(text, at_least, fold=fold, **kw).tolist()
    assert [int(w) for w in rows[:, 0]] == [max(0, n - ctx.k + 1) for n in lengths]
    assert info["records"] == len(w_kept) and info["bytes"] == len(text) and info["bytes_out"] == len(w_out) <= len(text) + 1
    assert info["records_out"] == sum(1 for n in w_kept if n) and info["records_dropped"] == sum(1 for n in w_kept if not n)
    assert info["records_trimmed"] == sum(1 for n, full in zip(w_kept, lengths) if 0 < n < full)
    assert info["bases_in"] == sum(lengths) and info["bases_out"] == sum(w_kept)
    return (out, kept, rows), info


# --------------------------------------------------------------------------------------------- record shapes
@functools.lru_cache(maxsize=None)
def shapes(k: int, headless: bool):
    """(text, low windows): every record shape in one text, with the first low window at 0, at 1, in the middle, at
    the last window and nowhere; ends in a record without a newline."""
    rng = random.Random(1000 * k + headless)
    t, low = [], []

    def add(raw, at=None):  # at: the index of the record's low window, counted from the last one if negative
        t.append(raw)
        if at is not None:
            low.append((len(t) - 1, at))

    t.append(dna(rng, k + 2) + "\n" if headless else "  \n\t\n \x0b\n")
    add(">km1 a b\n" + dna(rng, k - 1) + "\n")
    add(">k\n" + dna(rng, k) + "\n")
    add(">k low\n" + dna(rng, k) + "\n", 0)
    add("  >kp1\tx\n" + dna(rng, k + 1) + "\n", 1)
    add(" \t>kp1 whole\n" + dna(rng, k + 1) + "\n")
    add(">h1\n")
    add(">h2\n" + dna(rng, k + 3) + "\n", 2)
    add(">\n" + dna(rng, k + 1) + "\n")
    add(">wrapped\n" + wrap(dna(rng, 3 * k + 5), 7), k + 3)
    s = dna(rng, 2 * k + 4)
    add(">crlf x\r\n" + s[:5] + "\r\n" + s[5:] + "\r\n", -1)
    add(">cr\r" + dna(rng, k + 2) + "\r" + dna(rng, 3) + "\r", 1)
    add(">cr whole\r" + dna(rng, k + 2) + "\r")
    s = dna(rng, k + 6)
    add(">star\n" + s[:3] + "*" + s[3:] + "**\n*\n")
    add(">star low\n" + s[:3] + "*" + dna(rng, k + 3) + "**\n*\n", 4)
    add(">blank\n  " + dna(rng, k + 1) + " \t" + dna(rng, 5) + "  \n")  # (windows 2.. hold a blank: absent)
    for i, at in enumerate((0, 1, 4, -1, None, -2)):
        add(">p%d\n%s\n" % (i, dna(rng, k + 9)), at)
    add(">empty line\n\n" + dna(rng, k + 2) + "\n\n", 2)
    add(">last one\n" + dna(rng, k + 4))
    text = "".join(t).encode()
    recs = trim_rule.records(text)
    assert len(recs) == len(t) - (0 if headless else 1)
    shift = 0 if headless else -1  # (t[0] is the headless record, or blanks that are none)
    low = [(r + shift, at if at >= 0 else len(recs[r + shift][1]) - k + 1 + at) for r, at in low]
    return text, tuple(low)


@pytest.mark.parametrize("headless", [False, True], ids=["blanks_first", "headless"])
@pytest.mark.parametrize("k", [21, 31, 33])
def test_record_shapes(k, headless):
    text, low = shapes(k, headless)
    table = crafted(text, k, low)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (out, kept, rows), info = check(ctx, text, table)
        assert info["headless"] == (1 if headless else 0) and info["pieces"] == 1
        assert info["preamble"] == (0 if headless else len("  \n\t\n \x0b\n"))
        names = [h.split()[0] if h.split() else b"" for h, _ in trim_rule.records(text)]
        at = names.index(b">km1")
        # k - 1: dropped; k: whole; k with its only window low: dropped; k + 1 cut to k; k + 1 whole; a header behind a header
        assert kept[at:at + 7].tolist() == [0, k, 0, k, k + 1, 0, k + 1]
        assert b"  >kp1\tx\n" in out and b" \t>kp1 whole\n" in out and b">crlf x\r\n" in out and b">cr\r" in out
        assert int(kept[names.index(b">blank")]) == k + 1 and out.endswith(b"\n") and not text.endswith(b"\n")
        assert 0 < info["records_trimmed"] < info["records_out"] < info["records"]
        # min_len = k + 2 drops what keeps k or k + 1
        (_, kept2, _), _ = check(ctx, text, table, min_len=k + 2)
        assert kept2[at:at + 7].tolist() == [0] * 7 and 0 < np.count_nonzero(kept2) < np.count_nonzero(kept)
        # at_least above every count: nothing is emitted; at_least 1: only the windows with a blank are low
        (out6, kept6, _), _ = check(ctx, text, table, at_least=6)
        assert out6 == b"" and not kept6.any()
        (_, kept1, _), info1 = check(ctx, text, table, at_least=1)
        assert info1["records_trimmed"] == 1 and info1["records_dropped"] == 2  # ">blank"; k - 1 and the header alone


# ----------------------------------------------------------------------------------------------------- seams
LONG = 25_000  # more than three tiles of the walk
SEAM_P = (0, 1, 31, 32, 33, 63, 64, 2047, 2048, 2049, 8160, 8191, 8192, 8193, 16384, -1)
LEADS = {"none": "", "0_bases": ">a\n\n", "1_base": ">a\nG\n", "31_bases": ">a\n" + "ACGTTGCAGGATCCATGAACGTACGGTCAGT" + "\n"}


@functools.lru_cache(maxsize=None)
def long_seq(k: int) -> str:
    return dna(random.Random(7 * k), LONG)


def long_case(ctx_k: int, lead: str, lows):
    """The long record behind ``lead`` with the windows ``lows`` low: trimmed on a fresh context, against the rule."""
    text = (lead + ">long one\n" + long_seq(ctx_k) + "\n").encode()
    r = len(trim_rule.records(text)) - 1
    table = crafted(text, ctx_k, [(r, p) for p in lows])
    with native.Counter(ctx_k, NT) as ctx:
        load(ctx, table)
        (out, kept, _), info = check(ctx, text, table)
    first = min(lows)
    assert int(kept[r]) == (first + ctx_k - 1 if first else 0)  # (the record's windows are distinct k-mers: asserted below)
    return out, info


@pytest.mark.parametrize("lead", list(LEADS), ids=list(LEADS))
def test_one_low_window_at_every_seam(lead):
    """One record of 25 000 bases with a single low window at p: on both sides of a lane's run, a wave's and a tile's,
    at the first and the last window; with short records in front a lane's run starts inside the record."""
    k = 31
    seq = long_seq(k)
    assert len({seq[j:j + k] for j in range(LONG - k + 1)}) == LONG - k + 1
    for p in SEAM_P:
        p = p if p >= 0 else LONG - k
        out, info = long_case(k, LEADS[lead], (p,))
        if p:
            assert out.endswith((">long one\n" + seq[:p + k - 1] + "\n").encode())
        assert info["records_trimmed"] == (1 if p else 0)


@pytest.mark.parametrize("lows", [(100, 20_000), (20_000, 100), (8192 + 100, 8192 + 2048 + 105), (8192 + 2048 + 105, 8192 + 100),
                                  (2047, 2048), (8191, 8192, 8193), (5, 24_000, 12_000, 6)],
                         ids=["tiles", "tiles_swapped", "waves_of_a_tile", "waves_swapped", "wave_seam", "tile_seam", "many"])
def test_the_smallest_low_window_wins(lows):
    long_case(31, LEADS["1_base"], lows)


def test_every_window_low_and_none_low():
    k = 31
    text = (">long one\n" + long_seq(k) + "\n").encode()
    with native.Counter(k, NT) as ctx:
        load(ctx, crafted(text, k, [], high=1))
        (out, kept, _), info = check(ctx, text, crafted(text, k, [], high=1))
        assert out == b"" and kept.tolist() == [0] and info["records_dropped"] == 1 and info["s_first"] > 0
    reads = "".join(">r%d x\n%s\n" % (i, dna(random.Random(i), 31 + i % 70)) for i in range(200)).encode()
    table = crafted(reads + text, k, [])
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (out, kept, _), info = check(ctx, reads + text, table)  # identity: one-line LF records, nothing low
        assert out == reads + text and info["records_trimmed"] == info["records_dropped"] == 0
        assert info["s_first"] == 0  # (every window a hit: the first-low walk is skipped)
        # an empty text; a text of headers only
        assert [x.tolist() if hasattr(x, "tolist") else x for x in ctx.trim(b"")[:2]] == [b"", []]
        out, kept, rows = ctx.trim(b">a\n>b x\n\n>c")
        assert (out, kept.tolist(), rows.tolist()) == (b"", [0] * 3, [[0] * 5] * 3)
        out, kept, rows = ctx.trim(b"\n  \n")
        assert (out, kept.tolist(), rows.shape) == (b"", [], (0, 5))


@pytest.mark.parametrize("k", [21, 31])
def test_walk_seams(k):
    """Record boundaries on every lane, wave and tile seam of the walk (tests/walk_seams.py), a low window at index
    i % windows of record i; in one piece and in many."""
    recs = walk_seams.seam_records(k)
    text = walk_seams.seam_text(k)
    low = [(i, i % (len(seq) - k + 1)) for i, (_, seq) in enumerate(recs) if len(seq) >= k]
    table = crafted(text, k, low)
    want = trim_rule.expected(text, table, k, 2)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        one, info = check(ctx, text, table, want=want)
        many, info_p = check(ctx, text, table, want=want, piece_bytes=len(text) // 12)
        assert info["pieces"] == 1 and info_p["pieces"] > 8 and one[0] == many[0] and one[1].tolist() == many[1].tolist()
        assert info["records_trimmed"] > 100 and info["records_dropped"] > 10
        assert max(len(seq) for _, seq in recs) > 3 * walk_seams.TILE


def test_many_records_in_one_lanes_run():
    k = 31
    rng = random.Random(3)
    text = "".join(">s%d\n%s\n" % (i, dna(rng, k + i % 4)) for i in range(320)).encode()
    low = [(i, i % 5) for i in range(320) if i % 5 <= i % 4]  # (index i % 5 where the record has that window: mixed outcomes)
    table = crafted(text, k, low)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (_, kept, _), info = check(ctx, text, table)
        assert info["records_out"] > 50 and info["records_trimmed"] > 50 and info["records_dropped"] > 50


# ---------------------------------------------------------------------------------------------------- pieces
@functools.lru_cache(maxsize=None)
def mixed_text(k: int):
    """The record shapes, 400 reads with a low window in most of them, and a wrapped contig."""
    rng = random.Random(5 * k)
    head, low = shapes(k, True)
    n0 = len(trim_rule.records(head))
    reads = "".join(">m%d\n%s\n" % (i, dna(rng, 150)) for i in range(400))
    text = head + b"\n" + reads.encode() + (">contig\n" + wrap(dna(rng, 9_000), 60)).encode()
    low = list(low) + [(n0 + i, (37 * i) % 120) for i in range(400) if i % 3] + [(n0 + 400, 6_000)]
    return text, tuple(low)


def test_pieces():
    k = 31
    text, low = mixed_text(k)
    table = crafted(text, k, low)
    want = trim_rule.expected(text, table, k, 2)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        whole, info = check(ctx, text, table, want=want)
        small, info_s = check(ctx, text, table, want=want, piece_bytes=4096)
        assert info["pieces"] == 1 and info_s["pieces"] > 8 and info_s["headless"] == 1
        assert whole[0] == small[0] and whole[1].tolist() == small[1].tolist() and whole[2].tolist() == small[2].tolist()


# ------------------------------------------------------------------------------------------------ capacities
GUARD = 0xA5A5A5A5A5A5A5A5


def _raw(ctx, text: bytes, out_cap: int, cap: int, flags: int = 0, rule=(2, 0), null_out: bool = False, null_rule: bool = False,
         piece_bytes: int = 0, kept: bool = True, rows: bool = True):
    """mk_trim_text into 0xA5-guarded buffers one element longer than the capacities it is told."""
    out = np.full(out_cap + 1, 0xA5, dtype=np.uint8)
    kp = np.full(cap + 1, GUARD, dtype=np.uint64)
    rw = np.full((cap + 1, 5), GUARD, dtype=np.uint64)
    out_len, n, st = ctypes.c_size_t(0), ctypes.c_size_t(0), native.Trim()
    r = native.TrimRule(*rule)
    rc = native.lib().mk_trim_text(ctx._h, text, len(text), piece_bytes, flags, None if null_rule else ctypes.byref(r),
                                   None if null_out else out.ctypes.data, out_cap, ctypes.byref(out_len),
                                   kp.ctypes.data if kept else None, rw.ctypes.data if rows else None, cap, ctypes.byref(n),
                                   ctypes.byref(st))
    return {"rc": rc, "out_len": out_len.value, "nrows": n.value, "out": out, "kept": kp, "rows": rw, "st": st}


def test_capacities():
    k = 31
    text, low = mixed_text(k)
    table = crafted(text, k, low)
    w_out, w_kept = trim_rule.expected(text, table, k, 2)
    no, nr = len(w_out), len(w_kept)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        w_rows = ctx.screen(text, 2).tolist()
        for piece_bytes in (0, 4096):
            # exactly enough: everything written, the element past each capacity untouched
            got = _raw(ctx, text, no, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (0, no, nr) and got["st"].bytes_out == no
            assert got["out"][:no].tobytes() == w_out and got["out"][no] == 0xA5
            assert got["kept"][:nr].tolist() == w_kept and got["kept"][nr] == GUARD
            assert got["rows"][:nr].tolist() == w_rows and (got["rows"][nr] == GUARD).all()
            # out_cap one short: the needed size, nothing past the cap
            got = _raw(ctx, text, no - 1, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr) and got["out"][no - 1] == 0xA5
            assert "bytes" in ctx._L.mk_last_error(ctx._h).decode()
            # cap one short
            got = _raw(ctx, text, no, nr - 1, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr)
            assert (got["rows"][nr - 1] == GUARD).all() and got["kept"][nr - 1] == GUARD
            # the sizing call
            got = _raw(ctx, text, 0, 0, null_out=True, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr)
            assert (got["rows"] == GUARD).all() and (got["kept"] == GUARD).all()
        # kept NULL, rows NULL, both NULL (cap is ignored), st NULL
        got = _raw(ctx, text, no, nr, kept=False)
        assert got["rc"] == 0 and got["rows"][:nr].tolist() == w_rows and (got["kept"] == GUARD).all()
        got = _raw(ctx, text, no, nr, rows=False)
        assert got["rc"] == 0 and got["kept"][:nr].tolist() == w_kept and (got["rows"] == GUARD).all()
        got = _raw(ctx, text, no, 0, kept=False, rows=False)
        assert (got["rc"], got["out_len"], got["nrows"]) == (0, no, nr) and got["out"][:no].tobytes() == w_out
        out = np.full(no + 1, 0xA5, dtype=np.uint8)
        out_len, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        r = native.TrimRule(2, 0)
        rc = native.lib().mk_trim_text(ctx._h, text, len(text), 0, 0, ctypes.byref(r), out.ctypes.data, no, ctypes.byref(out_len), None,
                                       None, 0, ctypes.byref(n), None)
        assert (rc, out_len.value, n.value) == (0, no, nr) and out[:no].tobytes() == w_out and out[no] == 0xA5
        got = _raw(ctx, b"", 0, 0)
        assert (got["rc"], got["out_len"], got["nrows"]) == (0, 0, 0)


# ------------------------------------------------------------------------------------------ errors and state
def test_errors_and_state():
    k = 31
    text, low = shapes(k, False)
    table = crafted(text, k, low)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        before, size = ctx.to_dict(), ctx.rows()
        check(ctx, text, table)
        assert ctx.rows() == size and ctx.to_dict() == before
        got = _raw(ctx, text, len(text) + 1, 64, rule=(0, 0))
        assert got["rc"] == ARG and "at_least" in ctx._L.mk_last_error(ctx._h).decode() and (got["out"] == 0xA5).all()
        got = _raw(ctx, text, len(text) + 1, 64, flags=2)
        assert got["rc"] == ARG and "flag" in ctx._L.mk_last_error(ctx._h).decode()
        got = _raw(ctx, text, len(text) + 1, 64, null_rule=True)
        assert got["rc"] == ARG and "rule" in ctx._L.mk_last_error(ctx._h).decode()
        with pytest.raises(native.NonAsciiInput):
            ctx.trim(b">a\nACGT\xc3\xa9ACGT\n")
        out, kept, _ = ctx.trim(b">a \xc3\xa9\n" + text.split(b"\n")[6] + b"\n", 1)  # (a header line may hold any bytes)
        assert out.startswith(b">a \xc3\xa9\n") and kept.tolist() == [k]
        with pytest.raises(native.MercatHipError) as e:  # a plain table, folding asked for: refused as screen refuses it
            ctx.trim(text, fold=True)
        assert e.value.code == ARG
        assert ctx._L.mk_chunk_begin(ctx._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            ctx.trim(text)
        assert e.value.code == STATE
        assert ctx._L.mk_chunk_end(ctx._h, 1) == 0
        assert ctx.to_dict() == before
        assert ctx.trim() is None and ctx.to_dict() == before  # (without a text: the working memory is freed, as ever)


# ------------------------------------------------------------------------------------------------ device call
@pytest.mark.parametrize("out_lead", [0, 1, 15])
def test_trim_device_agrees(out_lead):
    import torch
    k = 31
    text, low = mixed_text(k)
    table = crafted(text, k, low)
    lead = 3  # the text at an odd address
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        w_out, w_kept, w_rows = ctx.trim(text)
        assert (w_out, w_kept.tolist()) == trim_rule.expected(text, table, k, 2)
        no, nr = len(w_out), len(w_kept)
        d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((out_lead + no + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_kept = torch.full((nr + 1,), -1, dtype=torch.int64, device="cuda")
        d_rows = torch.full((nr + 1, 5), -1, dtype=torch.int64, device="cuda")
        assert d_out.data_ptr() % 16 == 0 and d_text.data_ptr() % 2 == 0
        torch.cuda.synchronize()
        info = ctx.trim_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, no, d_kept.data_ptr(),
                               d_rows.data_ptr(), nr)
        got = d_out.cpu().numpy()
        assert info["bytes_out"] == no and info["records"] == nr and info["pieces"] == 1
        assert got[out_lead:out_lead + no].tobytes() == w_out
        assert (got[:out_lead] == 0xA5).all() and (got[out_lead + no:] == 0xA5).all()
        assert d_kept.cpu().numpy().view(np.uint64)[:nr].tolist() == w_kept.tolist() and int(d_kept[nr]) == -1
        assert d_rows.cpu().numpy().view(np.uint64)[:nr].tolist() == w_rows.tolist() and (d_rows[nr] == -1).all().item()
        with pytest.raises(native.MercatHipError) as e:
            ctx.trim_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, no - 1)
        assert e.value.code == RANGE
        with pytest.raises(native.MercatHipError) as e:
            ctx.trim_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr(), no, d_kept.data_ptr() + 4, 0, nr)
        assert e.value.code == ARG


# ------------------------------------------------------------------------------------------------ key shapes
def nt_small(seed: int) -> bytes:
    rng = random.Random(seed)
    recs = [">r%d x\n%s\n" % (i, wrap(dna(rng, rng.randrange(30, 260)), 70)) for i in range(60)]
    recs.insert(7, ">odd\n" + "ACGTTGCANGGATCCATGNAacgtACGGT*CAGT" * 6 + "\n>empty\n")
    return "".join(recs).encode()


def aa_small(seed: int) -> bytes:
    rng = random.Random(seed)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    recs = [">p%d\n%s\n" % (i, wrap("".join(rng.choice(letters) for _ in range(rng.randrange(10, 200))), 60)) for i in range(50)]
    recs.insert(9, ">odd\nMKV-LLAX*BZJUOacdeMKVLLAGGHHWWYYPPQQRRSSTTVVMKVLLAAGGHHWWYY.PPQQRRSSTTVVKKLL\n>empty\n")
    return "".join(recs).encode()


def halves_source(text: bytes) -> bytes:
    """Text that gives every count of 0, 1 and 2: the first 60 % of every record once, its first 30 % once more."""
    out = []
    for i, (_, seq) in enumerate(trim_rule.records(text)):
        out.append(b">a%d\n%s\n>b%d\n%s\n" % (i, seq[: 6 * len(seq) // 10], i, seq[: 3 * len(seq) // 10]))
    return b"".join(out)


KEY_SHAPES = [("nt", NT, 4), ("nt", NT, 31), ("nt", NT, 63), ("aa", AA, 5), ("aa", AA, 13), ("raw", RAW, 9)]


@pytest.mark.parametrize("kind,alphabet,k", KEY_SHAPES, ids=["%s_k%d" % (s[0], s[2]) for s in KEY_SHAPES])
def test_other_key_shapes(kind, alphabet, k):
    text = (aa_small if kind == "aa" else nt_small)(3)
    source = halves_source(text)
    table = cpu_ref.count_text(source, k, 1)
    with native.Counter(k, alphabet) as ctx:
        ctx.count_chunk(source, 1)
        for at_least in (1, 2):
            (_, kept, _), info = check(ctx, text, table, at_least)
            if k > 4 and at_least == 1:  # (nearly every 4-mer is in any table; few records hold 63 bases twice)
                assert info["records_trimmed"] > 10
            if alphabet == RAW:
                assert info["packed_windows"] == 0
        assert 0 < np.count_nonzero(kept) < len(kept)  # (at_least 2: records emitted and records dropped)


def test_canonical_fold():
    k = 31
    rng = random.Random(5)
    reads = [dna(rng, 150) for _ in range(40)]
    source = "".join(">s%d\n%s\n" % (i, r[:100 + i]) for i, r in enumerate(reads)).encode()
    text = "".join(">f%d\n%s\n>r%d\n%s\n" % (i, r, i, r.translate(COMP)[::-1]) for i, r in enumerate(reads)).encode()
    folded = cpu_ref.canonical_fold(cpu_ref.count_text(source, k, 1))
    with native.Counter(k, NT, canonical=True) as ctx:
        ctx.count_chunk(source, 1)
        (_, kept, _), info = check(ctx, text, folded, 1, folded_table=True)  # fold=None: as the context counts
        # the forward read keeps what the source held of it; its reverse complement starts in what the source lacks
        assert kept.tolist() == [n for i in range(40) for n in (100 + i, 0)] and info["folded"] > 0
        check(ctx, text, folded, 1, fold=True, folded_table=True)
        check(ctx, text, folded, 1, fold=False)  # taken as they stand: the windows of the other strand miss


# --------------------------------------------------------------------------------------------- cross-check
def test_kept_follows_from_the_track():
    """kept derived from Counter.track's counts (beside the rule's, which check() compares)."""
    k = 31
    text, low = mixed_text(k)
    table = crafted(text, k, low)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (_, kept, _), _ = check(ctx, text, table)
        counts, offsets, _, _ = ctx.track(text, 2)
        derived = []
        for r in range(len(offsets) - 1):
            v = counts[int(offsets[r]):int(offsets[r + 1])]
            lowv = np.flatnonzero(v < 2)
            n = 0 if not len(v) else len(v) + k - 1 if not len(lowv) else int(lowv[0]) + k - 1 if lowv[0] else 0
            derived.append(n if n >= k else 0)
        assert kept.tolist() == derived


# ------------------------------------------------------------------------------------------------ files and CLI
def fastq_text(seed: int, n: int):
    """(FASTQ text, the FASTA fq2fa makes of it): four-line records, quality strings that begin with '>' and '@'."""
    rng = random.Random(seed)
    fq, fa = [], []
    for i in range(n):
        seq = dna(rng, rng.randrange(20, 90))
        qual = (">" if i % 3 == 0 else "@" if i % 3 == 1 else "I") + "".join(rng.choice("!#>@FI+") for _ in range(len(seq) - 1))
        fq.append("@read%d len=%d\n%s\n+%s\n%s\n" % (i, len(seq), seq, "read%d" % i if i % 2 else "", qual))
        fa.append(">read%d len=%d\n%s\n" % (i, len(seq), seq))
    return "".join(fq).encode(), "".join(fa).encode()


def test_trim_reads_fasta_gz_fastq(tmp_path):
    k = 11
    fq, fa = fastq_text(11, 120)
    source = halves_source(fa)
    table = cpu_ref.count_text(source, k, 1)
    for name, data in (("r.fna", fa), ("r.fna.gz", gzip.compress(fa)), ("r.fastq", fq), ("r.fq.gz", gzip.compress(fq))):
        (tmp_path / name).write_bytes(data)
    lengths = [len(seq) for _, seq in trim_rule.records(fa)]
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(source, 1)
        for at_least, min_len in ((2, 0), (1, 30)):
            w_out, w_kept = trim_rule.expected(fa, table, k, at_least, min_len)
            assert 0 < sum(1 for n in w_kept if n) < len(w_kept)
            for name in ("r.fna", "r.fna.gz", "r.fastq", "r.fq.gz"):
                for dest in ("o.fna", "o.fna.gz"):
                    res = kmers.trim_reads(ctx, tmp_path / name, tmp_path / dest, at_least, min_len)
                    data = (tmp_path / dest).read_bytes()
                    if dest.endswith(".gz"):
                        assert data[:2] == b"\x1f\x8b"
                        data = gzip.decompress(data)
                    assert data == w_out, (name, dest)
                    assert res == {"records": len(w_kept), "kept": sum(1 for n in w_kept if n),
                                   "trimmed": sum(1 for n, full in zip(w_kept, lengths) if 0 < n < full),
                                   "dropped": sum(1 for n in w_kept if not n), "bases_in": sum(lengths), "bases_out": sum(w_kept),
                                   "bytes_out": len(w_out)}
            # a property that needs no oracle: every k-mer of the written file is held at_least times
            rows = ctx.screen(tmp_path / "o.fna", at_least)
            assert len(rows) == sum(1 for n in w_kept if n) and (rows[:, 0] == rows[:, 1]).all() and (rows[:, 0] > 0).all()


def test_cli_trim(tmp_path):
    k = 7
    rng = random.Random(3)
    samples = {"one": "".join(">a%d\n%s\n" % (i, dna(rng, 60)) for i in range(6)), "two": "".join(">b%d\n%s\n" % (i, dna(rng, 60)) for i in range(6))}
    for base, data in samples.items():
        (tmp_path / (base + ".fna")).write_text(data * 2)  # (every k-mer twice: the default -trim_min 2 keeps them)
    one, two = (trim_rule.records(samples[b].encode()) for b in ("one", "two"))
    reads = (b">from one\n" + one[1][1][5:45] + b"\n>from two\n" + two[4][1][:30] + b"\n  >neither\n" + dna(rng, 40).encode() +
             b"\n>short\nACG\n>both\n" + one[0][1][:20] + b"\n" + two[0][1][:20] + b"\n")
    (tmp_path / "reads.fa").write_bytes(reads)
    names = ["from", "from", "neither", "short", "both"]
    lengths = [40, 30, 40, 3, 40]
    for extra, rule in (([], (2, 0)), (["-trim_min", "3"], (3, 0)), (["-trim_len", "25"], (2, 25))):
        out = tmp_path / ("out%d" % len("".join(extra)))
        argv = ["-i", str(tmp_path / "one.fna"), str(tmp_path / "two.fna"), "-k", str(k), "-c", "1", "-skipclean", "-o", str(out),
                "-trim", str(tmp_path / "reads.fa")]
        assert cli.main(argv + extra) == 0
        for base, data in samples.items():
            table = cpu_ref.count_text((data * 2).encode(), k, 1)
            w_out, w_kept = trim_rule.expected(reads, table, k, *rule)
            assert (out / "trim_nucleotide" / ("%s_trimmed.fna" % base)).read_bytes() == w_out
            want = b"record\tlength\tkept\n" + b"".join(b"%s\t%d\t%d\n" % (n.encode(), full, kp) for n, full, kp in zip(names, lengths, w_kept))
            assert (out / "trim_nucleotide" / ("%s_trim.tsv" % base)).read_bytes() == want
            if rule == (2, 0):
                assert 0 < sum(1 for n in w_kept if n) < 5 and (base == "two" or any(0 < n < full for n, full in zip(w_kept, lengths)))
            if rule == (3, 0):
                assert not any(w_kept)
        assert sorted(p.name for p in (out / "trim_nucleotide").iterdir()) == ["one_trim.tsv", "one_trimmed.fna", "two_trim.tsv", "two_trimmed.fna"]
        assert not (out / "trim_protein").exists()
