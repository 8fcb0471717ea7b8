"""Quality trimming and read filtering of a FASTQ text on the GPU (mk_fastq_qtrim_text / mk_fastq_qtrim_device,
Counter.fastq_qtrim*, kmers.qtrim_reads, -qtrim).  Expected bytes, keep, rows, hist, figures and errors never come from
the code under test: the rule is tests/qtrim_rule.py over Python bytes.  Equality is exact everywhere.  The call reads no
table, so the rule-level tests share one small context.

The scan kernel gives a record a row of 16 lanes and a lane one aligned 16-byte granule of the quality line a pass, so a
pass ends at content index 256 p - (address of the line & 15): the seams below are walked with the record starts shifted
through all 16 alignments."""
import ctypes as C
import gzip
import re

import numpy as np
import pytest

import qtrim_rule as rule
from conftest import GOLDEN
from mercat2_amd import cli, kmers, native

pytestmark = pytest.mark.gpu
NT = native.ALPHABET_NT2
ARG, RANGE, UNSUPPORTED = -1, -7, -8
BASES = np.frombuffer(b"ACGT", np.uint8)
FIGURES = ("records", "records_out", "records_trimmed", "dropped_short", "dropped_n", "dropped_lowq", "dropped_meanq", "orphans",
           "bases_in", "bases_out", "bytes_out", "lines")
SEAMS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 239, 240, 241, 242, 255, 256, 257, 271, 272, 273, 511, 512, 513, 4095, 4096, 4097]


@pytest.fixture(scope="module")
def ctx():
    with native.Counter(5, NT) as c:
        yield c


def call_options(o):
    """The rule's options as Counter.fastq_qtrim takes them."""
    kw = {k: o[k] for k in ("cut_back", "cut_front", "min_len", "low_q", "min_mean_q", "phred_base", "which")}
    kw["max_n"] = None if o["max_n"] == rule.NO_LIMIT else o["max_n"]
    kw["max_low_frac"] = o["max_low_ppm"] / 1000000
    kw["paired"] = bool(o["paired"])
    return kw


def check(ctx, text, piece_bytes=0, **kw):
    """Counter.fastq_qtrim against the rule: bytes, keep, rows, hist and figures, or the error's code, record and kind.
    Returns the rule's result (or the message)."""
    o = rule.options(**kw)
    try:
        want = rule.run(text, **kw)
    except rule.QtrimError as err:
        with pytest.raises(native.MercatHipError) as e:
            ctx.fastq_qtrim(text, piece_bytes=piece_bytes, **call_options(o))
        msg = str(e.value)
        assert e.value.code == err.code, msg
        if err.record is not None:
            assert re.search(r"record %d\b" % err.record, msg) and rule.PHRASE[err.kind] in msg, msg
        return msg
    info = {}
    out, keep, rows, hist = ctx.fastq_qtrim(text, piece_bytes=piece_bytes, info=info, **call_options(o))
    assert rows.tolist() == [list(r) for r in want["rows"]]
    assert keep.tolist() == want["keep"]
    assert out == want["out"]
    assert hist.reshape(-1).tolist() == want["hist"]
    assert {f: info[f] for f in FIGURES} == want["figures"]
    return want


def decaying(rng, n, lo=2, hi=40):
    """Qualities that fall towards the 3' end, noisy: both sweeps find work."""
    if not n:
        return b""
    x = np.arange(n) / n
    q = np.clip(np.rint(rng.normal(hi - (hi - lo) * x ** 3, 6)), 0, 41).astype(np.uint8)
    q[: rng.integers(0, 4)] = 8
    return bytes(q + 33)


def record(rng, i, n, nl=b"\n", head_len=None, qual=None):
    head = b"@r%d" % i
    if head_len is not None:
        head = (head + b"x" * head_len)[:max(head_len, 1)]
    seq = bytearray(rng.choice(BASES, n))
    for j in rng.integers(0, max(n, 1), n // 40):
        seq[j] = ord("N") if j % 2 else ord("n")
    return head + nl + bytes(seq) + nl + b"+" + nl + (decaying(rng, n) if qual is None else qual) + nl


def aligned_records(rng, lengths, nl=b"\n", at=0):
    """A record of every length for every alignment 0 .. 15 of its quality line: the header is as long (1 .. 16 bytes) as
    puts the line there.  `at`: the bytes in front of the first record."""
    recs, i = [], 0
    for target in range(16):
        for n in lengths:
            fixed = n + 3 * len(nl) + 1  # what stands between the header and the quality line
            head_len = (target - at - fixed) % 16 or 16
            recs.append(record(rng, i, n, nl, head_len=head_len))
            at += len(recs[-1])
            i += 1
    return recs


def quality_alignments(text):
    """{sequence length: the set of (first byte of the quality line) & 15 over the records of that length}."""
    seen, at = {}, 0
    for head, seq, plus, qual in rule.records(text)[0]:
        seen.setdefault(len(rule.content(seq)), set()).add((at + len(head) + len(seq) + len(plus)) & 15)
        at += len(head) + len(seq) + len(plus) + len(qual)
    return seen


def seam_text(crlf):
    rng = np.random.default_rng(5)
    nl = b"\r\n" if crlf else b"\n"
    recs = aligned_records(rng, SEAMS, nl)
    recs.append(record(rng, len(recs), 70001, nl))
    return b"".join(recs), len(nl)


@pytest.mark.parametrize("ending", ["newline", "open", "1 empty", "2 empty", "3 empty"])
@pytest.mark.parametrize("crlf", [False, True])
def test_seam_lengths(ctx, crlf, ending):
    text, nl = seam_text(crlf)
    if ending == "open":
        text = text[:-nl]
    elif ending != "newline":
        text += b"\n" * int(ending[0])
    seen = quality_alignments(text)
    assert all(seen[n] == set(range(16)) for n in SEAMS)  # (the text's buffer is 16-byte aligned on the device)
    want = check(ctx, text, cut_front=12, cut_back=12, min_len=2, max_n=3, low_q=22, max_low_ppm=250000, min_mean_q=31)
    kinds = set(want["reasons"])
    assert {None, "short", "n", "lowq", "meanq"} <= kinds
    assert any(r[1] > 0 and r[1] + r[2] < r[0] for r in want["rows"])


def test_a_very_long_read_at_every_alignment(ctx):
    rng = np.random.default_rng(6)
    text = b"".join(aligned_records(rng, [70001]))
    assert quality_alignments(text)[70001] == set(range(16))
    want = check(ctx, text, cut_front=12, cut_back=12, min_len=2)
    assert all(0 < r[1] + r[2] < r[0] for r in want["rows"]) and any(r[1] > 0 for r in want["rows"])


# ---------------------------------------------------------------------------------- constructed qualities at a pass seam
# (name, the values laid over a flat read of q = cutoff, whose differences are 0; where the 5' cut lands behind the
# pattern's first byte)
PATTERNS = [("tie", [19, 21, 19], 1), ("touches 0", [19, 21, 18], 3), ("larger maximum behind the stop", [19, 22, 10, 10], 1),
            ("stop at once", [21, 10, 10], None), ("long climb", [19] * 20 + [30], 20)]


def seam_reads(reverse):
    """300-base reads, flat at the cutoff but for one pattern.  Forward: the pattern's first byte at pos, the 5' sweep
    meets it there.  Reverse: the pattern mirrored in place with its first byte -- the one the 3' sweep meets first -- at
    pos, its other bytes below it.  pos runs over 234 .. 265 and the one pass seam of such a read lies at 256 - (a & 15),
    241 .. 256, with a at four or three alignments a position: every event of every pattern falls on the last byte of a
    pass, on the first of the next and to either side.  Returns the text and, a record, where the cut must land: start
    forward, stop in reverse (None: no cut)."""
    rng = np.random.default_rng(11)
    recs, placed, at = [], [], 0
    for name, values, cut_at in PATTERNS:
        for pos in range(234, 266):
            for target in (0, 5, 10, 15) if pos % 2 else (3, 8, 13):
                q = [20] * 300
                if reverse:
                    q[pos - len(values) + 1:pos + 1] = values[::-1]
                    placed.append(None if cut_at is None else pos - cut_at + 1)
                else:
                    q[pos:pos + len(values)] = values
                    placed.append(None if cut_at is None else pos + cut_at)
                recs.append(record(rng, len(recs), 300, head_len=(target - at - 304) % 16 or 16, qual=bytes(v + 33 for v in q)))
                at += len(recs[-1])
    return b"".join(recs), placed


def seam_places(text):
    """{content index at which a record's second pass starts}: 256 - (address of the quality line & 15)."""
    return {256 - a for a in quality_alignments(text)[300]}


def test_five_prime_events_at_the_pass_seam(ctx):
    text, placed = seam_reads(False)
    assert seam_places(text) == {256 - a for a in (0, 3, 5, 8, 10, 13, 15)}
    want = check(ctx, text, cut_front=20, cut_back=0)
    assert [r[1] for r in want["rows"]] == [p or 0 for p in placed]
    check(ctx, text, cut_front=20, cut_back=20, min_len=10)


def test_three_prime_events_at_the_pass_seam(ctx):
    text, placed = seam_reads(True)
    assert seam_places(text) == {256 - a for a in (0, 3, 5, 8, 10, 13, 15)}
    want = check(ctx, text, cut_front=0, cut_back=20)
    assert [r[1] + r[2] for r in want["rows"]] == [300 if p is None else p for p in placed]
    assert [r[1] for r in want["rows"]] == [0] * len(placed)
    check(ctx, text, cut_front=20, cut_back=20, min_len=10)


def test_a_long_read_carries_its_sums(ctx):
    """A sum that stays at or above 0 for 20 000 bases, dips below behind them; the best lies passes back."""
    rng = np.random.default_rng(3)
    q = [19] * 5 + [20] * 9000 + [21, 21, 21] + [20] * 11000 + [40] + [19] * 50
    texts = [record(rng, 0, len(q), qual=bytes(v + 33 for v in q)), record(rng, 1, len(q), qual=bytes(v + 33 for v in reversed(q)))]
    want = check(ctx, b"".join(texts), cut_front=20, cut_back=20)
    assert want["rows"][0][1] == 5 and want["rows"][1][1] + want["rows"][1][2] == len(q) - 5


# ------------------------------------------------------------------------------------------- the two sets of the issue
LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 100, 150, 151, 255, 256, 257, 300] * 40


def model_reads(seed=2024):
    rng = np.random.default_rng(seed)
    recs = []
    for i, n in enumerate(LENGTHS):
        x = np.arange(n) / max(n, 1)
        shape = (i // 16 + i) % 4
        if shape == 0:
            mu = 38 - 34 * x ** 3
        elif shape == 1:
            mu = 37 - 20 * x ** 4
            mu[: rng.integers(1, 12)] = 8
        else:
            mu = np.full(n, 14.0 if shape == 2 else 38.0)
        q = np.clip(np.rint(rng.normal(mu, 5)), 0, 41).astype(np.int64)
        seq = rng.choice(BASES, n)
        seq[(q < 4) & (rng.random(n) < 0.7)] = ord("N")
        recs.append(b"@m%d\n" % i + bytes(seq) + b"\n+\n" + bytes((q + 33).astype(np.uint8)) + b"\n")
    return b"".join(recs)


def test_trimming_set(ctx):
    want = check(ctx, model_reads(), cut_front=20, cut_back=20, min_len=15)
    rows = want["rows"]
    front = sum(1 for L, s, k, *_ in rows if k and s > 0)
    back = sum(1 for L, s, k, *_ in rows if k and s + k < L)
    both = sum(1 for L, s, k, *_ in rows if k and s > 0 and s + k < L)
    emptied = sum(1 for L, s, k, *_ in rows if L and not k)
    whole = sum(1 for L, s, k, *_ in rows if L and k == L)
    print("trimming set: 5' %d, 3' %d, both %d, emptied %d, whole %d of %d" % (front, back, both, emptied, whole, len(rows)))
    assert min(front, back, both, emptied, whole) >= len(rows) // 10


def test_filter_set(ctx):
    want = check(ctx, model_reads(), cut_front=0, cut_back=0, min_len=15, max_n=1, low_q=15, max_low_ppm=200000, min_mean_q=33)
    counts = {k: want["reasons"].count(k) for k in ("short", "n", "lowq", "meanq", None)}
    print("filter set:", counts)
    assert min(counts.values()) >= len(want["rows"]) // 10


# ------------------------------------------------------------------------------------------------------------- pairs
def pair_text():
    rng = np.random.default_rng(9)
    good = lambda i, n: record(rng, i, n, qual=b"G" * n)
    poor = lambda i, n: record(rng, i, n, qual=b"#" * n)
    plan = [(good, good), (good, poor), (poor, good), (poor, poor)] * 5 + [(good, good)] * 3 + [(poor, good)] * 3
    return b"".join(a(2 * p, 40 + p) + b(2 * p + 1, 90 - p) for p, (a, b) in enumerate(plan))


@pytest.mark.parametrize("which", [1, 2])
def test_pairs(ctx, which):
    want = check(ctx, pair_text(), paired=1, which=which, min_len=20)
    assert set(want["keep"]) == {0, 1, 2} and want["figures"]["orphans"] == 13 and want["figures"]["records_out"] > 0


def test_pairs_refusals(ctx):
    text = pair_text()
    odd = join(rule.records(text)[0][:-1])
    assert "odd" in check(ctx, odd, paired=1)
    check(ctx, odd, paired=0)
    check(ctx, text, which=2)  # ARG: the orphans are a matter of pairs


# ------------------------------------------------------------------------------------------------------------ pieces
@pytest.mark.parametrize("paired", [0, 1])
def test_pieces_do_not_show(ctx, paired):
    rng = np.random.default_rng(17)
    lengths = [70, 0, 300, 150, 151, 1, 64, 90] * 6
    text = b"".join(record(rng, i, n) for i, n in enumerate(lengths))
    cuts = native.fastq_cuts(text, 1, pairs=bool(paired)).tolist()
    assert cuts == rule.pair_cuts(text, 1) if paired else len(cuts) > 30  # (the call raises 1 to its least piece)
    whole = check(ctx, text, paired=paired, min_len=10)
    for piece in (1, 200, 777, 5000):
        assert check(ctx, text, piece, paired=paired, min_len=10)["out"] == whole["out"]
    recs = rule.records(text)[0]
    for r in (0, 21, 47):
        bad = join(spoil(rec, "plus") if i == r else rec for i, rec in enumerate(recs))
        for piece in (0, 1, 500):
            assert "record %d " % r in check(ctx, bad, piece, paired=paired)


# ------------------------------------------------------------------------------------------------------------ errors
def spoil(rec, kind):
    """The four lines of a record with one thing wrong."""
    head, seq, plus, qual = rec
    if kind == "at":
        head = b">" + head[1:]
    elif kind == "plus":
        plus = b"-" + plus[1:]
    elif kind == "length":
        qual = qual[:1] + qual
    elif kind == "qual":
        qual = qual[:len(qual) // 2] + b" " + qual[len(qual) // 2 + 1:]
    return head, seq, plus, qual


def join(recs):
    return b"".join(b"".join(r) for r in recs)


def first_records(text, count):
    return join(rule.records(text)[0][:count])


@pytest.mark.parametrize("kind", ["at", "plus", "length", "qual"])
def test_each_malformed_kind(ctx, kind):
    rng = np.random.default_rng(21)
    lengths = [30, 300, 17, 600, 5, 256, 80, 150, 64]
    recs = rule.records(b"".join(record(rng, i, n) for i, n in enumerate(lengths)))[0]
    for where in (0, 4, len(recs) - 1):
        msg = check(ctx, join(spoil(r, kind) if i == where else r for i, r in enumerate(recs)))
        assert isinstance(msg, str) and "record %d " % where in msg
        # the lowest record wins, whatever fails behind it; and the lowest kind in that record
        later = [spoil(r, "at") if i > where else r for i, r in enumerate(recs)]
        assert "record %d " % where in check(ctx, join(spoil(r, kind) if i == where else r for i, r in enumerate(later)))
        assert rule.PHRASE[kind] in check(ctx, join(spoil(spoil(r, "qual"), kind) if i == where else r for i, r in enumerate(recs)))


def test_the_text_ends_inside_a_record(ctx):
    rng = np.random.default_rng(22)
    text = b"".join(record(rng, i, 50) for i in range(5))
    for cut_lines in (1, 2, 3):
        part = b"\n".join(text.split(b"\n")[:16 + cut_lines]) + b"\n"
        assert "record 4 " in check(ctx, part)
        assert "record 4 " in check(ctx, part, 1)


def test_the_phred_base(ctx):
    rng = np.random.default_rng(23)
    text = b"".join(record(rng, i, n) for i, n in enumerate([100, 150, 20]))
    assert rule.PHRASE["qual"] in check(ctx, text, phred_base=64)
    recs = rule.records(text)[0]  # the same reads with qualities from '@' up
    high = b"".join(h + s + p + bytes(b + 31 if b != 10 else b for b in q) for h, s, p, q in recs)
    want = check(ctx, high, phred_base=64, min_len=5)
    assert want["rows"] == rule.run(text, min_len=5)["rows"]
    check(ctx, text, phred_base=50)
    check(ctx, text, cut_back=94)
    check(ctx, text, cut_front=94)


def raw_call(ctx, text, opt, cap, keep, rows, hist, out_cap, device=False):
    """mk_fastq_qtrim_text with the arrays the caller chooses (None: NULL): (rc, out, out_len, nrec, message)."""
    buf = np.frombuffer(text, np.uint8)
    out = np.full(max(out_cap, 0) + 8, 0xA5, np.uint8)
    out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), native.FastqQtrim()
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = ctx._L.mk_fastq_qtrim_text(ctx._h, buf.ctypes.data, len(buf), 0, C.byref(opt), cap, ptr(keep), ptr(rows), ptr(hist),
                                    out.ctypes.data if out_cap >= 0 else None, max(out_cap, 0), C.byref(out_len), C.byref(nrec),
                                    C.byref(st))
    msg = ctx._L.mk_last_error(ctx._h)
    return rc, out, out_len.value, nrec.value, (msg or b"").decode()


def test_cap_room_sizing_and_null_arrays(ctx):
    text = first_records(model_reads(), 400)
    want = rule.run(text, cut_front=20, cut_back=20, min_len=15)
    n, size = len(want["rows"]), len(want["out"])
    opt = native.qtrim_options(cut_back=20, cut_front=20, min_len=15)
    arrays = lambda m: (np.zeros(m, np.uint8), np.zeros((m, 6), np.uint64), np.zeros(512, np.uint64))
    # a cap that is too short: the count comes back
    keep, rows, hist = arrays(n - 1)
    rc, out, out_len, nrec, msg = raw_call(ctx, text, opt, n - 1, keep, rows, hist, size)
    assert (rc, out_len, nrec) == (RANGE, 0, n) and "holds %d records" % n in msg and (out == 0xA5).all()
    # the sizing call, and one byte short: the size comes back, the arrays are complete, nothing is written
    for out_cap in (-1, size - 1):
        keep, rows, hist = arrays(n)
        rc, out, out_len, nrec, msg = raw_call(ctx, text, opt, n, keep, rows, hist, out_cap)
        assert (rc, out_len, nrec) == (RANGE if size else 0, size, n) and (out == 0xA5).all()
        assert keep.tolist() == want["keep"] and rows.tolist() == [list(r) for r in want["rows"]] and hist.tolist() == want["hist"]
    # exactly enough room; each array may be NULL, and cap says nothing without keep and rows
    for drop in (set(), {"keep"}, {"rows"}, {"hist"}, {"keep", "rows"}, {"keep", "rows", "hist"}):
        keep, rows, hist = arrays(n)
        rc, out, out_len, nrec, msg = raw_call(ctx, text, opt, 0 if {"keep", "rows"} <= drop else n, None if "keep" in drop else keep,
                                               None if "rows" in drop else rows, None if "hist" in drop else hist, size)
        assert (rc, out_len, nrec) == (0, size, n), msg
        assert out[:size].tobytes() == want["out"] and (out[size:] == 0xA5).all()
        assert keep.tolist() == ([0] * n if "keep" in drop else want["keep"])
        assert rows.tolist() == ([[0] * 6] * n if "rows" in drop else [list(r) for r in want["rows"]])
        assert hist.tolist() == ([0] * 512 if "hist" in drop else want["hist"])
    # the empty text
    keep, rows, hist = arrays(1)
    rc, out, out_len, nrec, msg = raw_call(ctx, b"", opt, 1, keep, rows, hist, 4)
    assert (rc, out_len, nrec) == (0, 0, 0)


# -------------------------------------------------------------------------------------------------------- device call
@pytest.mark.parametrize("lead,out_lead", [(0, 0), (3, 1), (15, 15)])
def test_device_call_agrees(ctx, lead, out_lead):
    import torch
    text = first_records(model_reads(), 330)
    kw = dict(cut_front=20, cut_back=20, min_len=15, max_n=2, paired=1, which=1)
    want = rule.run(text, **kw)
    n, size = len(want["rows"]), len(want["out"])
    d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
    d_keep = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    d_rows = torch.zeros((n, 6), dtype=torch.int64, device="cuda")
    d_hist = torch.full((512,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.full((out_lead + size + 40,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = ctx.fastq_qtrim_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, size, n, d_keep.data_ptr(),
                                  d_rows.data_ptr(), d_hist.data_ptr(), **call_options(rule.options(**kw)))
    got = d_out.cpu().numpy()
    assert got[out_lead:out_lead + size].tobytes() == want["out"]
    assert (got[:out_lead] == 0xA5).all() and (got[out_lead + size:] == 0xA5).all()
    assert d_keep.cpu().numpy()[:n].tolist() == want["keep"] and (d_keep.cpu().numpy()[n:] == 0xA5).all()
    assert d_rows.cpu().numpy().tolist() == [list(r) for r in want["rows"]]
    assert d_hist.cpu().numpy().tolist() == want["hist"]
    assert {f: info[f] for f in FIGURES} == want["figures"]
    text_out, keep, rows, hist = ctx.fastq_qtrim(text, **call_options(rule.options(**kw)))
    assert text_out == got[out_lead:out_lead + size].tobytes() and keep.tolist() == want["keep"]
    with pytest.raises(native.MercatHipError) as e:  # one byte short: refused, nothing written
        d_out.fill_(0xA5)
        torch.cuda.synchronize()
        ctx.fastq_qtrim_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, size - 1, n, 0, 0, 0,
                               **call_options(rule.options(**kw)))
    assert e.value.code == RANGE and (d_out.cpu().numpy() == 0xA5).all()
    with pytest.raises(native.MercatHipError) as e:
        ctx.fastq_qtrim_device(d_text.data_ptr(), len(text), d_out.data_ptr(), size, n, 0, d_rows.data_ptr() + 4, 0)
    assert e.value.code == ARG and "aligned" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:  # (refused before a byte is read)
        ctx.fastq_qtrim_device(d_text.data_ptr(), 1 << 32, d_out.data_ptr(), size, n, 0, 0, 0)
    assert e.value.code == RANGE and "2^32 - 1" in str(e.value)


# -------------------------------------------------------------------------------------------------------- end to end
def golden_reads():
    return gzip.open(GOLDEN / "inputs" / "Test_R1.fastq.gz", "rb").read()


def summary_of(want):
    """The summary file from the rule's own figures and histograms."""
    from mercat2_amd import report
    return report.format_qtrim_summary(want["figures"], [want["hist"][:256], want["hist"][256:]])


def test_qtrim_reads_on_the_golden_file(tmp_path):
    raw = golden_reads()
    kw = dict(cut_back=36, cut_front=31, min_len=100, max_n=0, low_q=30, max_low_ppm=150000, min_mean_q=35)
    want = rule.run(raw, **kw)
    assert 0 < want["figures"]["records_trimmed"] < want["figures"]["records_out"] < want["figures"]["records"]
    done = kmers.qtrim_reads(GOLDEN / "inputs" / "Test_R1.fastq.gz", tmp_path / "out.fastq.gz", cut_back=36, cut_front=31, min_len=100,
                             max_n=0, low_q=30, max_low_frac=0.15, min_mean_q=35, tsv_path=tmp_path / "out.tsv",
                             summary_path=tmp_path / "summary.tsv", keep_text=True)
    assert gzip.open(tmp_path / "out.fastq.gz", "rb").read() == want["out"] == done["text"]
    assert {f: done[f] for f in FIGURES} == want["figures"] and done["hist"].reshape(-1).tolist() == want["hist"]
    names = [h[1:].split()[0].decode() for h, _, _, _ in rule.records(raw)[0]]
    lines = (tmp_path / "out.tsv").read_bytes().split(b"\n")
    assert lines[0] == b"record\tlength\tstart\tkept\tn\tlow\tqsum\tkeep" and lines[-1] == b"" and len(lines) == len(names) + 2
    assert lines[1:-1] == [("\t".join([n] + [str(v) for v in r] + [str(k)])).encode() for n, r, k in zip(names, want["rows"], want["keep"])]
    assert (tmp_path / "summary.tsv").read_bytes() == summary_of(want)
    # the same reads as a pair of files: mates written to two files, the orphans to a third
    recs = rule.records(raw)[0]
    (tmp_path / "a_1.fastq").write_bytes(join(recs[0::2]))
    (tmp_path / "a_2.fastq").write_bytes(join(recs[1::2]))
    both = rule.run(join(recs), paired=1, **kw)
    lone = rule.run(join(recs), paired=1, which=2, **kw)
    done = kmers.qtrim_reads(tmp_path / "a_1.fastq", tmp_path / "o_1.fastq", cut_back=36, cut_front=31, min_len=100, max_n=0, low_q=30,
                             max_low_frac=0.15, min_mean_q=35, mate_file=tmp_path / "a_2.fastq", out_path2=tmp_path / "o_2.fastq",
                             singles_path=tmp_path / "singles.fastq")
    out = rule.records(both["out"])[0]
    assert (tmp_path / "o_1.fastq").read_bytes() == join(out[0::2]) and (tmp_path / "o_2.fastq").read_bytes() == join(out[1::2])
    assert (tmp_path / "singles.fastq").read_bytes() == lone["out"] and len(lone["out"]) > 0
    assert {f: done[f] for f in FIGURES} == both["figures"] and done["orphans"] > 0


def test_cli_qtrim(tmp_path):
    raw = golden_reads()
    (tmp_path / "Test_R1.fastq").write_bytes(raw)
    want = rule.run(raw, cut_back=35, cut_front=31, min_len=120, max_n=1, min_mean_q=36)
    assert 0 < want["figures"]["records_trimmed"] and want["figures"]["records_out"] < want["figures"]["records"]
    assert cli.main(["-i", str(tmp_path / "Test_R1.fastq"), "-k", "7", "-c", "2", "-qtrim", "35", "-qtrim_front", "31", "-qtrim_len", "120",
                     "-qtrim_n", "1", "-qtrim_mean", "36", "-o", str(tmp_path / "trimmed")]) == 0
    folder = tmp_path / "trimmed" / "qtrim"
    assert sorted(p.name for p in folder.iterdir()) == ["Test_R1_qtrim.fastq", "Test_R1_qtrim.tsv", "Test_R1_summary.tsv"]
    assert (folder / "Test_R1_qtrim.fastq").read_bytes() == want["out"]
    names = [h[1:].split()[0].decode() for h, _, _, _ in rule.records(raw)[0]]
    assert (folder / "Test_R1_qtrim.tsv").read_bytes() == b"record\tlength\tstart\tkept\tn\tlow\tqsum\tkeep\n" + b"".join(
        ("\t".join([n] + [str(v) for v in r] + [str(k)]) + "\n").encode() for n, r, k in zip(names, want["rows"], want["keep"]))
    assert (folder / "Test_R1_summary.tsv").read_bytes() == summary_of(want)
    # the table is the one of the rule's trimmed text counted untrimmed
    (tmp_path / "ref").mkdir()
    (tmp_path / "ref" / "Test_R1.fastq").write_bytes(want["out"])
    assert cli.main(["-i", str(tmp_path / "ref" / "Test_R1.fastq"), "-k", "7", "-c", "2", "-skipclean", "-o", str(tmp_path / "plain")]) == 0
    counts = (tmp_path / "trimmed" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes()
    assert counts == (tmp_path / "plain" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes() and counts.count(b"\n") > 100
    # -skipclean beside -qtrim changes nothing; without -qtrim the file is refused as before
    assert cli.main(["-i", str(tmp_path / "Test_R1.fastq"), "-k", "7", "-c", "2", "-qtrim", "35", "-qtrim_front", "31", "-qtrim_len", "120",
                     "-qtrim_n", "1", "-qtrim_mean", "36", "-skipclean", "-o", str(tmp_path / "both")]) == 0
    assert (tmp_path / "both" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes() == counts
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", str(tmp_path / "Test_R1.fastq"), "-k", "7", "-o", str(tmp_path / "refused")])
    assert "without -skipclean MerCat2 trims FASTQ reads with fastp" in str(e.value)
