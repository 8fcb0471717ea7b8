"""The host steps every call that reads a FASTQ text shares -- the line index and its trailing-line rule, the piece
plan, the re-alignment of a device text, the gather and how a call ends -- pinned through all seven calls at once:
mk_fastq_select_*, mk_correct_fastq_*, mk_fastq_qtrim_*, mk_fastq_adapt_*, mk_fastq_overlap_*, mk_fastq_qc_* and
mk_fastq_dedup_*, text and device.  The options are harmless (no cut, no filter, an adapter that matches nothing, mates
that do not overlap, a table that holds every k-mer), so every read comes back whole and a difference is one of the
shared steps.  What is expected comes from the rule modules, never from the library."""
import collections
import ctypes as C
import functools
import random
import re

import numpy as np
import pytest

import adapt_rule as adr
import correct_fastq_rule as cfr
import dedup_rule as ddr
import fastq_select_rule as fsr
import overlap_rule as ovr
import qc_rule as qcr
import qtrim_rule as qtr
from mercat2_amd import native

pytestmark = pytest.mark.gpu
NT = native.ALPHABET_NT2
RANGE, UNSUPPORTED = -7, -8
K = 5
ADAPTER = b"T" * 12  # (no read holds four T in a row)
PHRASE = dict(fsr.PHRASE)
RULE_ERRORS = (fsr.SelectError, cfr.CorrectFastqError, qtr.QtrimError, adr.AdaptError, ovr.OverlapError, qcr.QcError, ddr.DedupError)

# a call, whether records 2p and 2p + 1 are mates, and (select) whether kept[] is given: the line pass then checks the bytes
Variant = collections.namedtuple("Variant", "call paired kept")
VARIANTS = [Variant("select", 0, 0), Variant("select", 0, 1), Variant("correct", 0, 0), Variant("qtrim", 0, 0), Variant("qtrim", 1, 0),
            Variant("adapt", 0, 0), Variant("adapt", 1, 0), Variant("overlap", 1, 0), Variant("qc", 0, 0), Variant("qc", 1, 0),
            Variant("dedup", 0, 0), Variant("dedup", 1, 0)]
ids = lambda v: v.call + ("-paired" if v.paired else "") + ("-kept" if v.kept else "")
variants = pytest.mark.parametrize("v", VARIANTS, ids=ids)
writers = pytest.mark.parametrize("v", [v for v in VARIANTS if v.call != "qc"], ids=ids)
modes = pytest.mark.parametrize("mode", ["text", "device"])


# ------------------------------------------------------------------------------------------------------------- texts
def _reads(rng, lengths, seen):
    out = []
    while len(out) < len(lengths):
        seq = bytes(rng.choice(b"ACGT") for _ in range(lengths[len(out)]))
        if b"TTTT" not in seq and seq not in seen:
            seen.add(seq)
            out.append(seq)
    return out


def _fastq(rng, reads):
    return b"".join(b"@read%d\n%s\n+\n%s\n" % (i, s, bytes(rng.choice(b"5:?DFHIJ") for _ in s)) for i, s in enumerate(reads))


def _texts():
    rng, seen = random.Random(20240), set()
    small = _reads(rng, [5, 40, 17, 33, 16, 31, 9, 24], seen)
    big = _reads(rng, [30] * 120, seen)
    table = {}
    for seq in small + big:
        for j in range(len(seq) - K + 1):
            table[seq[j:j + K].decode()] = 5
    return _fastq(rng, small), _fastq(rng, big), table


SMALL, BIG, TABLE = _texts()
TEXTS = [SMALL, BIG]
assert len(BIG) > 8192  # (more than two tiles of the line passes)


def lengths(text):
    return [len(fsr.content(rec[1])) for rec in fsr.records(text)[0]]


def partial(text, k):
    """The text with the first k lines of one more record behind it."""
    return text + b"".join([b"@open\n", b"ACGTACGT\n", b"+\n"][:k])


def no_at(text, r):
    """The text with the '@' of record r replaced."""
    at = sum(len(b"".join(rec)) for rec in fsr.records(text)[0][:r])
    assert text[at:at + 1] == b"@"
    return text[:at] + b"x" + text[at + 1:]


# ---------------------------------------------------------------------------------------------------------- the rules
def _want(v, text):
    lists = lambda rows: [list(r) for r in rows]
    if v.call == "select":
        return {"out": fsr.expected(text, None, lengths(text) if v.kept else None)}
    if v.call == "correct":
        out, fix = cfr.expected(text, TABLE, K, 2)
        return {"out": out, "fix": lists(fix)}
    if v.call == "qtrim":
        w = qtr.run(text, cut_back=0, cut_front=0, paired=v.paired)
        return {"out": w["out"], "keep": w["keep"], "rows": lists(w["rows"]), "hist": w["hist"]}
    if v.call == "adapt":
        w = adr.run(text, [ADAPTER], None, min_overlap=8, max_err_ppm=0, paired=v.paired)
        return {"out": w["out"], "keep": w["keep"], "rows": lists(w["rows"]), "hits": w["hits"]}
    if v.call == "overlap":
        w = ovr.run(text, which=2)
        return {"out": w["out"], "keep": w["keep"], "rows": lists(w["rows"])}
    if v.call == "qc":
        w = qcr.run(text, paired=v.paired)
        return {name: w[name].tolist() for name in qcr.TABLES + ("rows",)}
    w = ddr.run(text, paired=v.paired)
    return {"out": w["out"], "keep": w["keep"].tolist(), "rows": w["rows"].tolist(), "levels": w["levels"].tolist()}


@functools.lru_cache(maxsize=None)
def want(v, text):
    """(what the call gives, None) or (None, (code, record, kind)) by the call's rule module."""
    try:
        return _want(v, text), None
    except RULE_ERRORS as e:
        return None, (e.code, e.record, e.kind)


# ---------------------------------------------------------------------------------------------------------- the calls
@pytest.fixture(scope="module")
def ctx():
    with native.Counter(K, NT) as c:
        assert c.load_tsv(b"".join(b"%s\t%d\n" % (key.encode(), n) for key, n in TABLE.items()))["rows"] == len(TABLE)
        yield c


def call_text(ctx, v, text, piece_bytes=0):
    pb = dict(piece_bytes=piece_bytes)
    if v.call == "select":
        return {"out": ctx.fastq_select(text, kept=np.array(lengths(text), np.uint64) if v.kept else None, **pb)}
    if v.call == "correct":
        out, fix, _ = ctx.correct_fastq(text, 2, **pb)
        return {"out": out, "fix": fix.tolist()}
    if v.call == "qtrim":
        out, keep, rows, hist = ctx.fastq_qtrim(text, cut_back=0, cut_front=0, paired=bool(v.paired), **pb)
        return {"out": out, "keep": keep.tolist(), "rows": rows.tolist(), "hist": hist.reshape(-1).tolist()}
    if v.call == "adapt":
        out, keep, rows, hits = ctx.fastq_adapt(text, [ADAPTER], min_overlap=8, max_err=0.0, paired=bool(v.paired), **pb)
        return {"out": out, "keep": keep.tolist(), "rows": rows.tolist(), "hits": hits.tolist()}
    if v.call == "overlap":
        out, keep, rows = ctx.fastq_overlap(text, which=2, **pb)
        return {"out": out, "keep": keep.tolist(), "rows": rows.tolist()}
    if v.call == "qc":
        got = ctx.fastq_qc(text, paired=bool(v.paired), rows=True, **pb)
        return {name: got[name].tolist() for name in qcr.TABLES + ("rows",)}
    out, keep, rows, levels = ctx.fastq_dedup(text, paired=bool(v.paired), **pb)
    return {"out": out, "keep": keep.tolist(), "rows": rows.tolist(), "levels": levels.tolist()}


def call_device(ctx, v, text, lead=0):
    """The device twin with the text at a 512-aligned address + lead; every array the call fills is given."""
    import torch
    n, nrec = len(text), len(fsr.records(text)[0])
    room = max(nrec, 1)
    d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
    d_out = torch.full((n + 1 + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    d_keep = torch.zeros((room,), dtype=torch.uint8, device="cuda")
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    host = lambda t, m=nrec: t.cpu().numpy()[:m].tolist()
    ptr, out_ptr = d_text.data_ptr() + lead, d_out.data_ptr()
    assert d_text.data_ptr() % 16 == 0

    def written(info):
        got = d_out.cpu().numpy()
        assert (got[info["bytes_out"]:] == 0xA5).all()
        return got[:info["bytes_out"]].tobytes()

    torch.cuda.synchronize()
    if v.call == "select":
        d_kept = torch.tensor(lengths(text) or [0], dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        info = ctx.fastq_select_device(ptr, n, out_ptr, n + 1, nrec, 0, d_kept.data_ptr() if v.kept else 0)
        return {"out": written(info)}
    if v.call == "correct":
        d_fix = torch.zeros((room + 1, 4), dtype=torch.int32, device="cuda")
        d_rows = i64(room + 1, 5)
        torch.cuda.synchronize()
        info = ctx.correct_fastq_device(ptr, n, out_ptr, n, d_fix.data_ptr(), d_rows.data_ptr(), room + 1, at_least=2)
        return {"out": written(info), "fix": host(d_fix, info["records"])}
    if v.call == "qtrim":
        d_rows, d_hist = i64(room, 6), i64(512)
        torch.cuda.synchronize()
        info = ctx.fastq_qtrim_device(ptr, n, out_ptr, n + 1, nrec, d_keep.data_ptr(), d_rows.data_ptr(), d_hist.data_ptr(), cut_back=0,
                                      cut_front=0, paired=bool(v.paired))
        return {"out": written(info), "keep": host(d_keep), "rows": host(d_rows), "hist": host(d_hist, 512)}
    if v.call == "adapt":
        d_rows, d_hits = i64(room, 5), i64(1)
        torch.cuda.synchronize()
        info = ctx.fastq_adapt_device(ptr, n, out_ptr, n + 1, [ADAPTER], None, nrec, d_keep.data_ptr(), d_rows.data_ptr(),
                                      d_hits.data_ptr(), min_overlap=8, max_err=0.0, paired=bool(v.paired))
        return {"out": written(info), "keep": host(d_keep), "rows": host(d_rows), "hits": host(d_hits, 1)}
    if v.call == "overlap":
        d_rows = i64(room, 5)
        torch.cuda.synchronize()
        info = ctx.fastq_overlap_device(ptr, n, out_ptr, n + 1, nrec, d_keep.data_ptr(), d_rows.data_ptr(), which=2)
        assert d_text.cpu().numpy()[lead:].tobytes() == text  # (the call works on a copy)
        return {"out": written(info), "keep": host(d_keep), "rows": host(d_rows)}
    if v.call == "qc":
        tabs = {name: i64(*shape) for name, shape in native.qc_shapes(512, bool(v.paired)).items()}
        d_rows = i64(room, 4)
        torch.cuda.synchronize()
        ctx.fastq_qc_device(ptr, n, *[tabs[name].data_ptr() for name in qcr.TABLES], d_rows.data_ptr(), nrec, paired=bool(v.paired))
        return dict({name: tabs[name].cpu().numpy().tolist() for name in qcr.TABLES}, rows=host(d_rows))
    d_rows, d_levels = i64(room, 2), i64(102)
    torch.cuda.synchronize()
    info = ctx.fastq_dedup_device(ptr, n, out_ptr, n + 1, nrec, d_keep.data_ptr(), d_rows.data_ptr(), d_levels.data_ptr(),
                                  paired=bool(v.paired))
    return {"out": written(info), "keep": host(d_keep), "rows": host(d_rows), "levels": host(d_levels, 102)}


def check(ctx, v, mode, text, piece_bytes=0, lead=0):
    """The call against its rule: what it gives, or the message of the error the rule states."""
    w, err = want(v, text)
    run = (lambda: call_text(ctx, v, text, piece_bytes)) if mode == "text" else (lambda: call_device(ctx, v, text, lead))
    if err is None:
        got = run()
        assert got == w
        return got
    with pytest.raises(native.MercatHipError) as e:
        run()
    code, record, kind = err
    msg = str(e.value)
    assert e.value.code == code, msg
    assert re.search(r"record %d\b" % record, msg) and PHRASE[kind] in msg, msg
    return msg


def several_pieces(v, text):
    """piece_bytes = 1 is raised to 2 (k + 24) bytes: the rule's cuts say that the text is then more than two pieces."""
    cuts = (qtr.pair_cuts if v.paired else fsr.cuts)(text, 2 * (K + 24))
    assert len(cuts) >= 2
    return cuts


# -------------------------------------------------------------------------------------------------------------- cases
@modes
@variants
def test_trailing_empty_lines(ctx, v, mode):
    for text in TEXTS:
        base = check(ctx, v, mode, text)
        for t in (1, 2, 3):
            got = check(ctx, v, mode, text + b"\n" * t)
            if v.call == "correct":  # (the text comes back byte for byte)
                assert got == dict(base, out=base["out"] + b"\n" * t)
            else:
                assert got == base


@modes
@variants
def test_no_final_newline(ctx, v, mode):
    for text in TEXTS:
        got = check(ctx, v, mode, text[:-1])
        if v.call not in ("correct", "qc"):  # (a record that is written ends in a newline)
            assert got["out"] == text


@modes
@variants
def test_crlf(ctx, v, mode):
    for text in TEXTS:
        got = check(ctx, v, mode, text.replace(b"\n", b"\r\n"))
        if v.call in ("qtrim", "adapt", "overlap", "dedup"):  # (whole records come back as they stand)
            assert got["out"] == text.replace(b"\n", b"\r\n")


@modes
@variants
def test_text_ends_inside_a_record(ctx, v, mode):
    for text in TEXTS:
        nrec = len(fsr.records(text)[0])
        for k in (1, 2, 3):
            for open_end in (False, True):
                broken = partial(text, k)[:-1] if open_end else partial(text, k)
                assert want(v, broken)[1] == (UNSUPPORTED, nrec, "incomplete")
                msg = check(ctx, v, mode, broken)
                assert "(%d of its 4 lines)" % k in msg, msg


@variants
def test_text_ends_inside_a_record_of_the_last_piece(ctx, v):
    for text in TEXTS:
        nrec = len(fsr.records(text)[0])
        for k in (1, 2, 3):
            broken = partial(text, k)
            several_pieces(v, broken)
            assert want(v, broken)[1] == (UNSUPPORTED, nrec, "incomplete")
            msg = check(ctx, v, "text", broken, piece_bytes=1)
            assert "(%d of its 4 lines)" % k in msg, msg


@variants
def test_malformed_record_in_the_first_piece(ctx, v):
    for text in TEXTS:
        ends = np.cumsum([len(b"".join(rec)) for rec in fsr.records(text)[0]])
        r = int(np.searchsorted(ends, several_pieces(v, text)[0], side="right")) - 1  # the last record of the first piece
        broken = no_at(text, r)
        assert want(v, broken)[1] == (UNSUPPORTED, r, "at")
        assert check(ctx, v, "text", broken, piece_bytes=1) == check(ctx, v, "text", broken)
        check(ctx, v, "device", broken)
        assert check(ctx, v, "text", text, piece_bytes=1) == check(ctx, v, "text", text)  # (and the pieces of a good text agree)


@variants
def test_device_text_at_any_address(ctx, v):
    for text in (SMALL, BIG[:-1], SMALL.replace(b"\n", b"\r\n")):
        base = check(ctx, v, "device", text)
        for d in (1, 7, 15):
            assert check(ctx, v, "device", text, lead=d) == base


def raw(ctx, v, mode, text, out_cap):
    """The ABI call with room for out_cap bytes and none of the optional arrays: (rc, out_len, what lies behind out_cap)."""
    L, h, n, nrec = ctx._L, ctx._h, len(text), len(fsr.records(text)[0])
    if mode == "device":
        import torch
        d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        addr, out, pb = d_text.data_ptr(), d_out.data_ptr(), ()
    else:
        h_text, h_out = np.frombuffer(text, np.uint8), np.full(n + 64, 0xA5, np.uint8)
        addr, out, pb = h_text.ctypes.data, h_out.ctypes.data, (0,)
    fn = lambda name: getattr(L, "mk_%s_%s" % (name, mode))
    out_len, cnt = C.c_size_t(0), C.c_size_t(0)
    tail = (out, out_cap, C.byref(out_len), C.byref(cnt))
    if v.call == "select":
        rc = fn("fastq_select")(h, addr, n, *pb, None, None, nrec, 1, out, out_cap, C.byref(out_len), C.byref(native.FastqSelect()))
    elif v.call == "correct":
        rule = native.CorrectFastqRule(2, 0, 0)
        rc = fn("correct_fastq")(h, addr, n, *pb, 0, C.byref(rule), out, out_cap, C.byref(out_len), None, None, 0, C.byref(cnt),
                                 C.byref(native.CorrectFastq()))
    elif v.call == "qtrim":
        opt = native.qtrim_options(cut_back=0, cut_front=0, paired=bool(v.paired))
        rc = fn("fastq_qtrim")(h, addr, n, *pb, C.byref(opt), 0, None, None, None, *tail, C.byref(native.FastqQtrim()))
    elif v.call == "adapt":
        opt = native.adapt_options(min_overlap=8, max_err=0.0, paired=bool(v.paired))
        bases, lens, mates, seqs = native.adapter_arrays([ADAPTER], None)
        rc = fn("fastq_adapt")(h, addr, n, *pb, bases.ctypes.data, lens.ctypes.data, mates.ctypes.data, len(seqs), C.byref(opt), 0, None,
                               None, None, *tail, C.byref(native.FastqAdapt()))
    elif v.call == "overlap":
        opt = native.overlap_options(which=2)
        rc = fn("fastq_overlap")(h, addr, n, *pb, C.byref(opt), 0, None, None, *tail, C.byref(native.FastqOverlap()))
    else:
        opt = native.dedup_options(paired=bool(v.paired))
        rc = fn("fastq_dedup")(h, addr, n, *pb, C.byref(opt), 0, None, None, None, *tail, C.byref(native.FastqDedup()))
    behind = (d_out.cpu().numpy() if mode == "device" else h_out)[out_cap:]
    return rc, out_len.value, behind


@modes
@writers
def test_out_one_byte_short(ctx, v, mode):
    for text in (SMALL, BIG[:-1]):
        size = len(want(v, text)[0]["out"])
        rc, out_len, behind = raw(ctx, v, mode, text, size)
        assert (rc, out_len) == (0, size) and (behind == 0xA5).all()
        rc, out_len, behind = raw(ctx, v, mode, text, size - 1)
        assert (rc, out_len) == (RANGE, size) and (behind == 0xA5).all()
