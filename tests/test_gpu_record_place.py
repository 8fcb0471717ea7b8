"""Record placement (fl_tiles_k / fl_scan_k / fl_starts_k, tr_hend_k) and the output gathers (fl_gather_k / fl_edges_k,
tr_gather_k / tr_edges_k) at their seams: the texts of tests/record_seams.py through filter, trim, normalize, correct and
the pairs call (DESIGN section 7 lists the seams).  Expected values never come from the library: rows, ranges and the
rules are tests/filter_rule.py, trim_rule.py, norm_rule.py and correct_rule.py over a dict, the pair rule is restated
below.  Every comparison is exact -- bytes, masks, rows, counters.

The key control: k = 5 (every call here accepts it) and a table, loaded with load_tsv, of the 32 5-mers over {A, C}; see
tests/record_seams.py.  One context serves the module: no call here changes its table."""
import functools

import numpy as np
import pytest

import correct_rule
import filter_rule
import norm_rule
import record_seams as rs
import trim_rule
from mercat2_amd import native

pytestmark = pytest.mark.gpu
K, RULE, AT_LEAST = rs.K, rs.FILTER_RULE, rs.TRIM_AT_LEAST
LEADS = (0, 1, 7, 8, 15)        # of the output from a 16-byte boundary
TEXT_RESIDUES = (0, 1, 8, 15)   # of a device text
DEVICE_FAMILIES = ("lengths", "minimal", "dropped_runs", "last32")
FAMILIES = DEVICE_FAMILIES + ("boundaries", "long")
PIECES = (4096, 8192 + 17)
FILTER_OP, TRIM_OP = native.PAIRS_FILTER, native.PAIRS_TRIM


@pytest.fixture(scope="module")
def ctx():
    c = native.Counter(K, native.ALPHABET_NT2)
    assert c.load_tsv(rs.table_tsv())["rows"] == len(rs.table()) == 32
    yield c
    assert c.to_dict() == rs.table()
    c.close()


class Device:
    """A text in device memory at a chosen residue, an output buffer filled with 0xA5 at a chosen lead."""

    def __init__(self, cap):
        import torch
        self.torch = torch
        self.text = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        self.out = torch.zeros(cap + 128, dtype=torch.uint8, device="cuda")
        assert self.text.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def run(self, call, text: bytes, lead: int, residue: int, want: bytes, room: int):
        """call(text address, out address, out_cap) -> info; the bytes must be ``want`` at ``lead``, 0xA5 all around."""
        torch = self.torch
        self.text[:16] = ord(">")
        self.text[residue:residue + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        region = self.out[:lead + room + 64]
        region.fill_(0xA5)
        torch.cuda.synchronize()
        info = call(self.text.data_ptr() + residue, self.out.data_ptr() + lead, room)
        got = region.cpu().numpy()
        assert info["bytes_out"] == len(want)
        assert got[lead:lead + len(want)].tobytes() == want
        assert (got[:lead] == 0xA5).all() and (got[lead + len(want):] == 0xA5).all()
        return info


@pytest.fixture(scope="module")
def device():
    return Device(64 * 1024)


# ------------------------------------------------------------------------------------------------- the oracles
@functools.lru_cache(maxsize=None)
def want_filter(text: bytes, invert: bool):
    return filter_rule.expected(text, rs.table(), K, RULE, invert)


@functools.lru_cache(maxsize=None)
def want_trim(text: bytes):
    """(out, kept, rows, bases per record)"""
    out, kept = trim_rule.expected(text, rs.table(), K, AT_LEAST)
    return out, kept, filter_rule.ref_rows(text, rs.table(), K, AT_LEAST), [len(seq) for _, seq in trim_rule.records(text)]


def check_filter(ctx, text: bytes, invert: bool, **kw):
    info = {}
    out, keep, rows = ctx.filter(text, RULE[0], RULE[1], RULE[2], invert, info=info, **kw)
    w_out, w_keep, w_rows, w_pre = want_filter(text, invert)
    assert rows.dtype == np.uint64 and rows.shape == (len(w_rows), 5) and rows.tolist() == w_rows
    assert keep.dtype == bool and keep.tolist() == w_keep
    assert out == w_out
    assert info["records"] == len(w_rows) and info["bytes"] == len(text) and info["preamble"] == w_pre
    assert info["records_out"] == sum(w_keep) and info["bytes_out"] == len(w_out)
    assert info["windows"] == sum(r[0] for r in w_rows) and info["hits"] == sum(r[1] for r in w_rows)
    return out, keep, rows, info


def check_both(ctx, text: bytes, **kw):
    """Plain and inverted: with the preamble the two outputs partition the text."""
    plain, inverted = check_filter(ctx, text, False, **kw), check_filter(ctx, text, True, **kw)
    assert (plain[1] ^ inverted[1]).all() and plain[3]["preamble"] == inverted[3]["preamble"]
    assert len(plain[0]) + len(inverted[0]) + plain[3]["preamble"] == len(text)
    return plain, inverted


def check_trim(ctx, text: bytes, **kw):
    info = {}
    out, kept, rows = ctx.trim(text, AT_LEAST, info=info, **kw)
    w_out, w_kept, w_rows, lengths = want_trim(text)
    assert kept.dtype == np.uint64 and kept.tolist() == w_kept
    assert out == w_out
    assert rows.tolist() == w_rows
    assert info["records"] == len(w_kept) and info["bytes"] == len(text) and info["bytes_out"] == len(w_out)
    assert info["records_out"] == sum(1 for n in w_kept if n) and info["records_dropped"] == sum(1 for n in w_kept if not n)
    assert info["records_trimmed"] == sum(1 for n, full in zip(w_kept, lengths) if 0 < n < full)
    assert info["bases_in"] == sum(lengths) and info["bases_out"] == sum(w_kept)
    return out, kept, rows, info


def same(a, b):
    assert a[0] == b[0] and a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist()


# ------------------------------------------------------------------------------------------------- placement
def test_placement_through_filter(ctx):
    text = rs.placement_text()
    whole = check_both(ctx, text)
    assert whole[0][3]["pieces"] == whole[1][3]["pieces"] == 1 and whole[0][3]["headless"] == 0
    assert 0 < whole[0][1].sum() < len(whole[0][1])
    for piece_bytes in PIECES:
        cut = check_both(ctx, text, piece_bytes=piece_bytes)
        assert cut[0][3]["pieces"] > len(text) // (2 * piece_bytes)
        same(whole[0], cut[0])
        same(whole[1], cut[1])


def test_placement_through_trim(ctx):
    text = rs.placement_text()
    whole = check_trim(ctx, text)
    assert whole[3]["pieces"] == 1 and whole[3]["records_trimmed"] > 0 and whole[3]["records_dropped"] > 1000
    for piece_bytes in PIECES:
        cut = check_trim(ctx, text, piece_bytes=piece_bytes)
        assert cut[3]["pieces"] > len(text) // (2 * piece_bytes)
        same(whole, cut)


def test_the_end_of_the_text_through_filter_and_trim(ctx):
    """Texts of every length mod 32 that end in a header line: the byte path of fl_headers_in, tr_hend_k without a
    terminator, with a lone CR and with CR LF, the LF trim writes for a record without one; byte 0 a '>', blanks and a
    '>', no header line at all."""
    for name, text in rs.tail_texts().items():
        plain, inverted = check_both(ctx, text)
        assert plain[3]["headless"] == (1 if name.startswith("headless") else 0), name
        assert plain[3]["preamble"] == 0, name
        check_trim(ctx, text)


# ------------------------------------------------------------------------------------------------- fl_gather_k, fl_edges_k
@pytest.mark.parametrize("family", FAMILIES)
def test_gather_through_filter(ctx, family):
    for name, text in rs.gather_cases("filter")[family].items():
        plain, inverted = check_both(ctx, text)
        assert plain[3]["pieces"] == 1, name


@pytest.mark.parametrize("family", DEVICE_FAMILIES)
def test_gather_through_filter_device(ctx, device, family):
    """mk_filter_device with the output 0, 1, 7, 8 and 15 bytes past a 16-byte boundary (head = 0, 15, 9, 8, 1)."""
    for name, text in rs.gather_cases("filter")[family].items():
        for invert in (True, False):
            w_out, w_keep, w_rows, _ = want_filter(text, invert)
            for lead in LEADS:
                call = lambda src, dst, room: ctx.filter_device(src, len(text), dst, room, at_least=RULE[0], min_hits=RULE[1],
                                                                min_ppm=RULE[2], invert=invert)
                info = device.run(call, text, lead, 0, w_out, len(text))
                assert info["records"] == len(w_rows) and info["records_out"] == sum(w_keep) and info["pieces"] == 1, (name, lead)


@pytest.mark.parametrize("residue", TEXT_RESIDUES)
def test_filter_device_text_residues(ctx, device, residue):
    """The device text itself off a 16-byte boundary (the parser then reads a copy), the last record kept."""
    for name, text in rs.gather_cases("filter")["last32"].items():
        w_out, w_keep, w_rows, _ = want_filter(text, True)
        call = lambda src, dst, room: ctx.filter_device(src, len(text), dst, room, at_least=RULE[0], min_hits=RULE[1], min_ppm=RULE[2],
                                                        invert=True)
        info = device.run(call, text, 7, residue, w_out, len(text))
        assert info["records"] == len(w_rows) and info["records_out"] == sum(w_keep), name


# ------------------------------------------------------------------------------------------------- tr_gather_k, tr_edges_k
@pytest.mark.parametrize("family", FAMILIES)
def test_gather_through_trim(ctx, family):
    for name, text in rs.gather_cases("trim")[family].items():
        assert check_trim(ctx, text)[3]["pieces"] == 1, name


@pytest.mark.parametrize("family", DEVICE_FAMILIES)
def test_gather_through_trim_device(ctx, device, family):
    for name, text in rs.gather_cases("trim")[family].items():
        w_out, w_kept, _, _ = want_trim(text)
        for lead in LEADS:
            call = lambda src, dst, room: ctx.trim_device(src, len(text), dst, room, at_least=AT_LEAST)
            info = device.run(call, text, lead, 0, w_out, len(text) + 1)
            assert info["records"] == len(w_kept) and info["records_out"] == sum(1 for n in w_kept if n), (name, lead)


def test_header_lines_alone_through_correct(ctx, device):
    """mk_correct_* emits every record, a header line alone without an LF of its own (lf == 0): eight of them to a chunk,
    records shorter than k, ordinary ones between them; from the host in one piece and in many, on the device at every lead."""
    text = rs.header_alone_text()
    w_out, w_fix = correct_rule.expected(text, rs.table(), K, AT_LEAST)
    w_rows = filter_rule.ref_rows(text, rs.table(), K, AT_LEAST)
    assert sum(r[2] for r in w_fix) > 5  # (the G in an ordinary record: A and C both mend it)
    for piece_bytes in (0, 64):
        info = {}
        out, fix, rows = ctx.correct(text, AT_LEAST, piece_bytes=piece_bytes, info=info)
        assert out == w_out
        assert [tuple(r) for r in fix.tolist()] == w_fix and rows.tolist() == w_rows
        assert info["records"] == len(w_fix) and info["bytes_out"] == len(w_out) and (info["pieces"] == 1) == (piece_bytes == 0)
        assert [info[c] for c in native.CORRECT_COLUMNS] == [sum(r[i] for r in w_fix) for i in range(4)]
    for lead in LEADS:
        call = lambda src, dst, room: ctx.correct_device(src, len(text), dst, room, at_least=AT_LEAST)
        assert device.run(call, text, lead, 0, w_out, len(text) + 1)["records"] == len(w_fix)


# ------------------------------------------------------------------------------------------------- the other callers
def wiring_texts():
    return {"placement": rs.placement_text(), "boundaries": rs.gather_cases("filter")["boundaries"]["bound_+0"],
            "boundaries_trim": rs.gather_cases("trim")["boundaries"]["bound_+0"]}


@pytest.mark.parametrize("name", ["placement", "boundaries"])
def test_wiring_of_normalize(ctx, name):
    """A target above every count: mk_norm_* keeps exactly the records that have windows, as they stand.  Every record of
    the placement text has some, so that output is the whole text; with min_depth 1 the records over {G, T} (depth 0) go,
    and every start of the placement text is a kept/dropped boundary again."""
    text = wiring_texts()[name]
    for min_depth in (0, 1):
        for invert in (False, True):
            want = norm_rule.expected(text, rs.table(), K, 1000, min_depth, invert=invert)
            assert want["records_over"] == 0
            if min_depth == 0:
                assert want["keep"] == [(w > 0) != invert for w in want["windows"]]
            else:
                assert 1000 < len(want["out"]) < len(text) - 1000
            info = {}
            out, keep, med, rows = ctx.normalize(text, 1000, min_depth, invert=invert, info=info)
            assert out == want["out"]
            assert keep.tolist() == want["keep"] and med.tolist() == want["median"] and [int(w) for w in rows[:, 0]] == want["windows"]
            assert rows.tolist() == filter_rule.ref_rows(text, rs.table(), K, 1)
            assert info["records_out"] == want["records_out"] and info["bytes_out"] == len(want["out"]) and info["preamble"] == 0
            assert info["records_low"] == want["records_low"] and info["records_short"] == want["records_short"]


def even(text: bytes) -> bytes:
    """The text without its last record if it holds an odd number of them."""
    ranges, _ = filter_rule.ref_ranges(text)
    return text if len(ranges) % 2 == 0 else text[:ranges[-1][0]]


@functools.lru_cache(maxsize=None)
def want_pairs(text: bytes, op: int, both: bool):
    """The pair rule over the unpaired rules: filter passes a pair iff either mate matches (``both``: both), trim iff both
    keep something; a mate that passes alone is an orphan (keep 2, in singles)."""
    raws = [raw for raw, _ in norm_rule.records(text)]
    if op == FILTER_OP:
        rows = filter_rule.ref_rows(text, rs.table(), K, RULE[0])
        own, extra, emitted = [filter_rule.matched(r, RULE) for r in rows], None, raws
        passed = [(a and b) if both else (a or b) for a, b in zip(own[0::2], own[1::2])]
    else:
        _, kept, rows, _ = want_trim(text)
        own, extra = [n > 0 for n in kept], kept
        emitted = [header + seq[:n] + b"\n" for (header, seq), n in zip(trim_rule.records(text), kept)]
        passed = [a and b for a, b in zip(own[0::2], own[1::2])]
    assert len(raws) == len(own) == len(rows) and len(raws) % 2 == 0 and b"".join(raws) == text
    keep = [1 if passed[r // 2] else 2 if o else 0 for r, o in enumerate(own)]
    return {"out": b"".join(e for e, kp in zip(emitted, keep) if kp == 1), "singles": b"".join(e for e, kp in zip(emitted, keep) if kp == 2),
            "keep": keep, "own": extra, "rows": rows}


PAIR_CALLS = {"filter_either": (FILTER_OP, False), "filter_both": (FILTER_OP, True), "trim": (TRIM_OP, False)}


@pytest.mark.parametrize("call", list(PAIR_CALLS))
@pytest.mark.parametrize("name", ["placement", "boundaries", "boundaries_trim"])
def test_wiring_of_pairs(ctx, name, call):
    """The placement text alternates matched and unmatched records, so every pair holds one of each: with "either" the
    whole text is emitted, with "both" and under trim every matched record is an orphan -- the singles output then shows
    every start.  The boundaries texts mix all three outcomes."""
    op, both = PAIR_CALLS[call]
    text = even(wiring_texts()[name])
    want = want_pairs(text, op, both)
    assert len(want["out"]) + len(want["singles"]) > 5_000 and (call == "filter_either" or want["keep"].count(0) > 50)
    for piece_bytes in (0, 4096):
        info = {}
        out, singles, keep, own, rows = ctx.pairs(text, op, at_least=RULE[0] if op == FILTER_OP else AT_LEAST, both=both, singles=True,
                                                  piece_bytes=piece_bytes, info=info)
        assert keep.tolist() == want["keep"]
        assert out == want["out"]
        assert singles == want["singles"]
        assert rows.tolist() == want["rows"] and (own is None if op == FILTER_OP else own.tolist() == want["own"])
        assert info["records"] == len(want["keep"]) and info["records_out"] == want["keep"].count(1) == 2 * info["pairs_out"]
        assert info["bytes_out"] == len(want["out"]) and info["bytes_singles"] == len(want["singles"])
        assert info["singles_out"] == want["keep"].count(2) and (info["pieces"] == 1) == (piece_bytes == 0)


# ------------------------------------------------------------------------------------------------- more than 1024 tiles
@pytest.fixture(scope="module")
def many():
    return rs.many_tiles_text(), rs.many_tiles_expected()


@pytest.mark.parametrize("piece_bytes", [0, 1 << 20], ids=["one_piece", "1MiB_pieces"])
def test_more_tiles_than_the_scans_have_threads(ctx, many, piece_bytes):
    """Just over 8 MiB in one piece: 1049 tiles of raw text in fl_scan_k, more than 1024 tiles of parsed symbols in the
    record scan of sc_piece -- every thread of sc_tile_scan owns two tiles; record starts on both sides of the byte where
    thread 512 takes over.  The same from 1 MiB pieces (128 tiles each)."""
    text, want = many
    assert len(text) > rs.SCAN_THREADS * rs.UNITS[3]
    for invert, name in ((False, "plain"), (True, "inverted")):
        info = {}
        out, keep, rows = ctx.filter(text, RULE[0], RULE[1], RULE[2], invert, piece_bytes=piece_bytes, info=info)
        assert rows.tolist() == want["rows"]
        assert keep.tolist() == [m != invert for m in want["matched"]]
        assert out == want[name]
        assert (info["pieces"] == 1) == (piece_bytes == 0) and info["records"] == len(want["rows"]) and info["bytes"] == len(text)
        assert info["records_out"] == int(keep.sum()) and info["bytes_out"] == len(want[name]) and info["preamble"] == 0
        assert info["windows"] == sum(r[0] for r in want["rows"]) and info["hits"] == sum(r[1] for r in want["rows"])
    info = {}
    out, kept, rows = ctx.trim(text, AT_LEAST, piece_bytes=piece_bytes, info=info)
    assert kept.tolist() == want["kept"]
    assert out == want["trim"]
    assert [r[0] for r in rows.tolist()] == [r[0] for r in want["rows"]]  # (hits are those of at_least 2: HIGH is 5, the same)
    assert rows.tolist() == want["rows"]
    assert (info["pieces"] == 1) == (piece_bytes == 0) and info["bytes_out"] == len(want["trim"])
    assert info["records_out"] == sum(1 for n in want["kept"] if n) and info["bases_out"] == sum(want["kept"])
