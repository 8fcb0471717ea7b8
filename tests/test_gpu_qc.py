"""Per-cycle quality control of a FASTQ text on the GPU (mk_fastq_qc_text / mk_fastq_qc_device, Counter.fastq_qc*,
kmers.qc_reads, -qc).  Expected tables, rows, figures and errors never come from the code under test: the rule is
tests/qc_rule.py over Python bytes.  Equality is exact everywhere.  The call reads no table, so all tests share one small
context.

qc_reads_k gives a record a row of 16 lanes and a lane one aligned 16-byte granule of a line a pass, so a pass ends at
content index 256 p - (address of the line & 15); qc_cycles_k gives a workgroup a tile of 64 cycles and a lane one of
them, with one more tile for the cycles behind max_pos.  The seams below are walked with the record starts shifted through
all 16 alignments."""
import ctypes as C
import gzip
import re

import numpy as np
import pytest

import qc_rule as rule
from conftest import GOLDEN
from mercat2_amd import cli, kmers, native, report

pytestmark = pytest.mark.gpu
NT = native.ALPHABET_NT2
ARG, RANGE, UNSUPPORTED = -1, -7, -8
BASES = np.frombuffer(b"ACGT", np.uint8)
FIGURES = ("records", "lines", "bases", "min_len", "max_len")
SEAMS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]


@pytest.fixture(scope="module")
def ctx():
    with native.Counter(5, NT) as c:
        yield c


def same(got, want, rows=True):
    for name in rule.TABLES:
        assert got[name].shape == want[name].shape and got[name].dtype == np.uint64, name
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:8].tolist())
    if rows:
        assert got["rows"].tolist() == want["rows"].tolist()


def check(ctx, text, piece_bytes=0, rows=True, **kw):
    """Counter.fastq_qc against the rule: the five tables, rows and the figures, or the error's code, record and kind.
    Returns the rule's result (or the message)."""
    o = rule.options(**kw)
    try:
        want = rule.run(text, **kw)
    except rule.QcError as err:
        with pytest.raises(native.MercatHipError) as e:
            ctx.fastq_qc(text, piece_bytes=piece_bytes, rows=rows, max_pos=o["max_pos"], phred_base=o["phred_base"], paired=bool(o["paired"]))
        msg = str(e.value)
        assert e.value.code == err.code, msg
        if err.record is not None:
            assert re.search(r"record %d\b" % err.record, msg) and rule.PHRASE[err.kind] in msg, msg
        return msg
    info = {}
    got = ctx.fastq_qc(text, piece_bytes=piece_bytes, rows=rows, info=info, max_pos=o["max_pos"], phred_base=o["phred_base"],
                       paired=bool(o["paired"]))
    same(got, want, rows)
    assert ("rows" in got) == rows
    assert {f: info[f] for f in FIGURES} == want["figures"]
    return want


def qualities(rng, n, lo=2, hi=41):
    """Qualities that fall towards the 3' end, noisy: every cycle has its own distribution."""
    if not n:
        return b""
    x = np.arange(n) / n
    return bytes(np.clip(np.rint(rng.normal(hi - (hi - lo) * x ** 2, 5)), 0, 60).astype(np.uint8) + 33)


def record(rng, i, n, nl=b"\n", head_len=None, qual=None, seq=None):
    head = b"@r%d" % i
    if head_len is not None:
        head = (head + b"x" * head_len)[:max(head_len, 1)]
    if seq is None:
        seq = bytearray(rng.choice(BASES, n))
        for j in rng.integers(0, max(n, 1), n // 20):
            seq[j] = b"NnacgtU-*"[j % 9]
    return head + nl + bytes(seq) + nl + b"+" + nl + (qualities(rng, n) if qual is None else qual) + nl


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


def join(recs):
    return b"".join(b"".join(r) for r in recs)


# ------------------------------------------------------------------------------------------------------------- seams
@pytest.mark.parametrize("ending", ["newline", "open", "1 empty", "2 empty", "3 empty"])
@pytest.mark.parametrize("crlf", [False, True])
def test_seam_lengths(ctx, crlf, ending):
    rng = np.random.default_rng(5)
    nl = b"\r\n" if crlf else b"\n"
    text = b"".join(aligned_records(rng, SEAMS, nl))
    if ending == "open":
        text = text[:-len(nl)]
    elif ending != "newline":
        text += b"\n" * int(ending[0])
    seen = quality_alignments(text)
    assert all(seen[n] == set(range(16)) for n in SEAMS)  # (the text's buffer is 16-byte aligned on the device)
    want = check(ctx, text, max_pos=512)
    assert want["read_len"][0, 513] == 16 and want["read_len"][0, 512] == 16 and want["pos_qual"][0, 512].sum() == 16
    check(ctx, text, max_pos=512, paired=1)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 150])
def test_max_pos_edges(ctx, P):
    rng = np.random.default_rng(P)
    lengths = [P - 1, P, P + 1, 4 * P]
    text = b"".join(record(rng, i, n) for i, n in enumerate(lengths * 3))
    want = check(ctx, text, max_pos=P)
    assert want["read_len"][0, P] == 3 and want["read_len"][0, P + 1] == 6 and want["pos_qual"][0, P].sum() == 3 * (1 + 3 * P)
    check(ctx, text, max_pos=P, paired=1)
    # no read passes P: the row behind the last cycle stays empty (and its tile is not launched)
    short = b"".join(record(rng, i, n) for i, n in enumerate([P - 1, P] * 3))
    want = check(ctx, short, max_pos=P)
    assert want["pos_qual"][0, P].sum() == 0 and want["read_len"][0, P + 1] == 0 and want["figures"]["max_len"] == [P, 0]


@pytest.mark.parametrize("P", [512, 16384])
def test_a_long_read_among_short_ones(ctx, P):
    rng = np.random.default_rng(6)
    lengths = [150, 0, 151, 70000, 100, 1, 150, 150]
    text = b"".join(record(rng, i, n) for i, n in enumerate(lengths))
    want = check(ctx, text, max_pos=P)
    assert want["pos_qual"][0, P].sum() == 70000 - P and want["figures"]["max_len"] == [70000, 0]
    check(ctx, text, max_pos=P, paired=1)


# -------------------------------------------------------------------------------------------------------- contention
@pytest.fixture(scope="module")
def many_reads():
    """20 000 x 150, every quality byte equal and with random qualities; each with the rule's result, computed once."""
    rng = np.random.default_rng(8)
    n, L = 20000, 150
    seq = rng.choice(BASES, (n, L))
    flat = np.full((n, L), ord("I"), np.uint8)
    noisy = (rng.integers(0, 42, (n, L)) + 33).astype(np.uint8)
    out = {}
    for name, q in (("equal", flat), ("random", noisy)):
        text = b"".join(b"@r%d\n" % i + seq[i].tobytes() + b"\n+\n" + q[i].tobytes() + b"\n" for i in range(n))
        out[name] = (text, rule.run(text, max_pos=512), rule.run(text, max_pos=512, paired=1))
    return out


@pytest.mark.parametrize("which", ["equal", "random"])
def test_contention(ctx, many_reads, which):
    text, want, want_pairs = many_reads[which]
    if which == "equal":
        assert (want["pos_qual"][0, :150, 40] == 20000).all() and want["pos_qual"].sum() == 3000000  # one counter a row
    same(ctx.fastq_qc(text, max_pos=512, rows=True), want)
    same(ctx.fastq_qc(text, max_pos=512, paired=True, rows=True), want_pairs)
    same(ctx.fastq_qc(text, max_pos=512, piece_bytes=1 << 20), want, rows=False)  # the flushes of the pieces add, too


# ---------------------------------------------------------------------------------------------------- quality values
def test_quality_values_and_the_clip(ctx):
    rng = np.random.default_rng(9)
    values = [0, 94, 95, 96, 222]
    recs = [record(rng, i, 40, qual=bytes([33 + v]) * 40) for i, v in enumerate(values)]
    recs.append(record(rng, 5, 300, qual=bytes(33 + values[j % 5] for j in range(300))))
    want = check(ctx, b"".join(recs))
    # (the mixed read's mean is 507 // 5 = 101: the last bin, as the three flat reads from 95 up)
    assert want["pos_qual"][0, 0, 95] == 3 and want["read_qual"][0, 95] == 4 and want["rows"][4, 1] == 40 * 222


def test_phred_base_64(ctx):
    rng = np.random.default_rng(10)
    text = b"".join(record(rng, i, n) for i, n in enumerate([100, 150, 20]))
    assert rule.PHRASE["qual"] in check(ctx, text, phred_base=64)
    recs = rule.records(text)[0]  # the same reads with qualities from '@' up
    high = b"".join(h + s + p + bytes(b + 31 if b != 10 else b for b in q) for h, s, p, q in recs)
    want = check(ctx, high, phred_base=64)
    same(want, rule.run(text))
    for bad in (dict(phred_base=50), dict(max_pos=0), dict(max_pos=16385)):
        check(ctx, text, **bad)


@pytest.mark.parametrize("base", [33, 64])
def test_a_byte_below_the_base_names_its_record(ctx, base):
    rng = np.random.default_rng(11)
    good = lambda i, n: record(rng, i, n, qual=bytes([base + 30]) * n)
    for n, at in ((40, 0), (40, 39), (16, 15), (600, 0), (600, 255), (600, 256), (600, 300), (600, 599)):
        for head_len in (1, 8, 16):  # (the byte in the first lane, the last lane, and a second and third pass)
            q = bytearray([base + 30]) * n
            q[at] = base - 1
            recs = [good(0, 50), good(1, 150), record(rng, 2, n, qual=bytes(q), head_len=head_len), good(3, 20)]
            assert "record 2 " in check(ctx, b"".join(recs), phred_base=base)
    # the lowest record wins, whatever fails behind it
    q = bytearray([base + 30]) * 50
    q[7] = base - 1
    text = good(0, 50) + record(rng, 1, 50, qual=bytes(q)) + b">x\nAC\n+\nII\n" + record(rng, 3, 50, qual=bytes(q))
    assert "record 1 " in check(ctx, text, phred_base=base)


# -------------------------------------------------------------------------------------------------------------- bases
def test_base_classes(ctx):
    rng = np.random.default_rng(12)
    seqs = [b"ACGTNacgtnU-*", b"acgtn" * 40, b"NNNN", b"U-*.xX@" * 30, b"GC" * 64 + b"g", b"A" * 257]
    text = b"".join(record(rng, i, len(s), seq=s) for i, s in enumerate(seqs))
    want = check(ctx, text, max_pos=100)
    # the first 13 cycles by hand: A 2 + 3 + 13, C 2 + 3 + 6, G 2 + 3 + 7, T 2 + 2, N 2 + 2 + 4, other 3 + 13
    assert want["pos_base"][0, :13, :].sum(axis=0).tolist()[:6] == [18, 11, 12, 4, 8, 16]
    assert want["rows"][:, 2].tolist() == [4, 80, 0, 0, 129, 0] and want["rows"][:, 3].tolist() == [2, 40, 4, 0, 0, 0]
    assert (want["pos_base"][:, :, 6:] == 0).all()


# --------------------------------------------------------------------------------------------------------- text shape
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
    check(ctx, b"")
    check(ctx, b"\n\n")
    assert "record 0 " in check(ctx, b"\n\n\n\n")


# -------------------------------------------------------------------------------------------------------------- pairs
def test_pairs(ctx):
    rng = np.random.default_rng(13)
    text = b"".join(record(rng, 2 * p, 100 + p) + record(rng, 2 * p + 1, 60 - p) for p in range(40))
    want = check(ctx, text, paired=1, max_pos=120)
    assert want["read_len"][0, :100].sum() == 0 and want["read_len"][1, 61:].sum() == 0 and want["read_len"][0, 121] == 19
    assert want["figures"]["min_len"] == [100, 21] and want["figures"]["max_len"] == [139, 60]
    single = rule.run(text, max_pos=120)
    assert np.array_equal(want["pos_qual"].sum(axis=0), single["pos_qual"][0])
    odd = join(rule.records(text)[0][:-1])
    assert "odd" in check(ctx, odd, paired=1)
    check(ctx, odd, paired=0)


# ------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("paired", [0, 1])
def test_pieces_do_not_show(ctx, paired):
    rng = np.random.default_rng(17)
    lengths = [70, 0, 300, 150, 151, 1, 64, 90] * 6
    text = b"".join(record(rng, i, n) for i, n in enumerate(lengths))
    cuts = native.fastq_cuts(text, 1, pairs=bool(paired)).tolist()
    assert len(cuts) == (23 if paired else 47)  # (the call raises 1 to its least piece)
    whole = check(ctx, text, paired=paired, max_pos=200)
    for piece in (1, 200, 777, 5000):
        same(check(ctx, text, piece, paired=paired, max_pos=200), whole)
    recs = rule.records(text)[0]
    for r in (0, 21, 47):
        bad = join(spoil(rec, "plus") if i == r else rec for i, rec in enumerate(recs))
        for piece in (0, 1, 500):
            assert "record %d " % r in check(ctx, bad, piece, paired=paired)


# ------------------------------------------------------------------------------------------------------- rows and cap
def raw_call(ctx, text, opt, cap, rows, piece_bytes=0):
    """mk_fastq_qc_text with the rows array the caller chooses (None: NULL): (rc, tables, nrec, message)."""
    buf = np.frombuffer(text, np.uint8)
    got = {name: np.full(shape, 7, np.uint64) for name, shape in native.qc_shapes(opt.max_pos, bool(opt.paired)).items()}
    out = native.QcOut(**{name: a.ctypes.data for name, a in got.items()}, rows=rows.ctypes.data if rows is not None else None)
    nrec, st = C.c_size_t(0), native.FastqQc()
    rc = ctx._L.mk_fastq_qc_text(ctx._h, buf.ctypes.data if len(buf) else None, len(buf), piece_bytes, C.byref(opt), cap, C.byref(out),
                                 C.byref(nrec), C.byref(st))
    msg = ctx._L.mk_last_error(ctx._h)
    return rc, got, nrec.value, (msg or b"").decode()


def test_rows_and_cap(ctx):
    rng = np.random.default_rng(14)
    text = b"".join(record(rng, i, n) for i, n in enumerate([70, 0, 300, 150, 151, 1, 64, 90] * 5))
    want = rule.run(text, max_pos=100)
    n = len(want["rows"])
    opt = native.qc_options(max_pos=100)
    # a cap that is too short: the count comes back, whatever the pieces are
    for piece in (0, 300):
        rows = np.full((n - 1, 4), 9, np.uint64)
        rc, got, nrec, msg = raw_call(ctx, text, opt, n - 1, rows, piece)
        assert (rc, nrec) == (RANGE, n) and "holds %d records" % n in msg
    # exactly enough room; and without rows cap says nothing (the tables were not zero before the call)
    rows = np.full((n + 1, 4), 9, np.uint64)
    rc, got, nrec, msg = raw_call(ctx, text, opt, n, rows)
    assert (rc, nrec) == (0, n), msg
    same(got, want, rows=False)
    assert rows[:n].tolist() == want["rows"].tolist() and (rows[n:] == 9).all()
    rc, got, nrec, msg = raw_call(ctx, text, opt, 0, None)
    assert (rc, nrec) == (0, n), msg
    same(got, want, rows=False)
    rc, got, nrec, msg = raw_call(ctx, b"", opt, 0, None)
    assert (rc, nrec) == (0, 0) and all((a == 0).all() for a in got.values())
    # a table may not be NULL
    out = native.QcOut(**{name: a.ctypes.data for name, a in got.items() if name != "read_gc"})
    buf = np.frombuffer(text, np.uint8)
    rc = ctx._L.mk_fastq_qc_text(ctx._h, buf.ctypes.data, len(buf), 0, C.byref(opt), 0, C.byref(out), None, None)
    assert rc == ARG and "NULL" in ctx._L.mk_last_error(ctx._h).decode()


# -------------------------------------------------------------------------------------------------------- device call
@pytest.mark.parametrize("lead,paired", [(0, False), (3, True), (15, False)])
def test_device_call_agrees(ctx, lead, paired):
    import torch
    rng = np.random.default_rng(15)
    text = b"".join(record(rng, i, n) for i, n in enumerate([70, 0, 300, 150, 151, 1, 64, 90, 513, 2] * 4))
    want = rule.run(text, max_pos=256, paired=int(paired))
    n = len(want["rows"])
    d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
    d_tabs = {name: torch.full(shape, 7, dtype=torch.int64, device="cuda") for name, shape in native.qc_shapes(256, paired).items()}
    d_rows = torch.full((n + 2, 4), 9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptrs = [d_tabs[name].data_ptr() for name in native.QC_TABLES]
    info = ctx.fastq_qc_device(d_text.data_ptr() + lead, len(text), *ptrs, rows_ptr=d_rows.data_ptr(), cap=n, max_pos=256, paired=paired)
    got = {name: d_tabs[name].cpu().numpy().view(np.uint64) for name in native.QC_TABLES}
    got["rows"] = d_rows.cpu().numpy().view(np.uint64)[:n]
    same(got, want)
    assert (d_rows.cpu().numpy()[n:] == 9).all() and {f: info[f] for f in FIGURES} == want["figures"]
    same(ctx.fastq_qc(text, max_pos=256, paired=paired, rows=True), want)
    info = ctx.fastq_qc_device(d_text.data_ptr() + lead, len(text), *ptrs, max_pos=256, paired=paired)  # (no rows, no cap)
    same({name: d_tabs[name].cpu().numpy().view(np.uint64) for name in native.QC_TABLES}, want, rows=False)
    with pytest.raises(native.MercatHipError) as e:
        ctx.fastq_qc_device(d_text.data_ptr() + lead, len(text), *ptrs, rows_ptr=d_rows.data_ptr(), cap=n - 1, max_pos=256, paired=paired)
    assert e.value.code == RANGE and "holds %d records" % n in str(e.value)
    for which in range(5):
        with pytest.raises(native.MercatHipError) as e:
            ctx.fastq_qc_device(d_text.data_ptr(), len(text), *[p + 4 if i == which else p for i, p in enumerate(ptrs)], max_pos=256,
                                paired=paired)
        assert e.value.code == ARG and "aligned" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:
        ctx.fastq_qc_device(d_text.data_ptr(), len(text), *ptrs, rows_ptr=d_rows.data_ptr() + 4, cap=n, max_pos=256, paired=paired)
    assert e.value.code == ARG and "aligned" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:  # (refused before a byte is read)
        ctx.fastq_qc_device(d_text.data_ptr(), 1 << 32, *ptrs, max_pos=256, paired=paired)
    assert e.value.code == RANGE and "2^32 - 1" in str(e.value)


# ----------------------------------------------------------------------------------------------- against existing code
def test_the_histogram_of_fastq_qtrim_is_the_column_sum(ctx):
    rng = np.random.default_rng(16)
    recs = [record(rng, i, n) for i, n in enumerate([150, 151, 600, 0, 64, 90] * 20 + [10])]
    recs.append(record(rng, len(recs), 50, qual=bytes([33 + 94, 33 + 95, 33 + 96, 255, 33 + 200] * 10)))
    text = b"".join(recs)
    hist = ctx.fastq_qtrim(text)[3][0]
    got = ctx.fastq_qc(text, max_pos=200, paired=True)["pos_qual"].sum(axis=(0, 1))
    assert got[:95].tolist() == hist[:95].tolist() and int(got[95]) == int(hist[95:].sum()) == 40


# -------------------------------------------------------------------------------------------------------- end to end
def golden_reads():
    return gzip.open(GOLDEN / "inputs" / "Test_R1.fastq.gz", "rb").read()


def files_of(want):
    """The five files from the rule's tables."""
    return {name: fmt(want) for name, fmt in report.QC_FILES.items()}


def test_qc_reads_on_the_golden_file(tmp_path):
    raw = golden_reads()
    want = rule.run(raw, max_pos=200)
    done = kmers.qc_reads(GOLDEN / "inputs" / "Test_R1.fastq.gz", tmp_path / "one", max_pos=200)
    same(done, want, rows=False)
    assert {f: done[f] for f in FIGURES} == want["figures"] and want["figures"]["bases"] > 0
    assert {name: (tmp_path / ("one_%s.tsv" % name)).read_bytes() for name in report.QC_FILES} == files_of(want)
    # the same reads as a pair of files, the second one gzipped
    recs = rule.records(raw)[0]
    (tmp_path / "a_1.fastq").write_bytes(join(recs[0::2]))
    with gzip.open(tmp_path / "a_2.fastq.gz", "wb") as fh:
        fh.write(join(recs[1::2]))
    both = rule.run(join(recs), max_pos=200, paired=1)
    done = kmers.qc_reads(tmp_path / "a_1.fastq", tmp_path / "two", max_pos=200, mate_file=tmp_path / "a_2.fastq.gz")
    same(done, both, rows=False)
    assert done["min_len"] == both["figures"]["min_len"] and both["read_len"][1].sum() == len(recs) // 2
    assert {name: (tmp_path / ("two_%s.tsv" % name)).read_bytes() for name in report.QC_FILES} == files_of(both)


def test_cli_qc(tmp_path):
    import qtrim_rule
    raw = golden_reads()
    (tmp_path / "Test_R1.fastq").write_bytes(raw)
    trimmed = qtrim_rule.run(raw, cut_back=35, min_len=120)
    assert 0 < trimmed["figures"]["records_trimmed"] and trimmed["figures"]["records_out"] < trimmed["figures"]["records"]
    assert cli.main(["-i", str(tmp_path / "Test_R1.fastq"), "-k", "7", "-c", "2", "-qc", "-qtrim", "35", "-qtrim_len", "120", "-o",
                     str(tmp_path / "out")]) == 0
    folder = tmp_path / "out" / "qc"
    assert sorted(p.name for p in folder.iterdir()) == sorted("Test_R1_%s_%s.tsv" % (stage, name) for stage in ("raw", "clean")
                                                              for name in report.QC_FILES)
    for stage, text in (("raw", raw), ("clean", trimmed["out"])):
        want = files_of(rule.run(text, max_pos=512))
        assert {name: (folder / ("Test_R1_%s_%s.tsv" % (stage, name))).read_bytes() for name in report.QC_FILES} == want
    # per mate, a smaller MAXPOS, no step: one stage; and the count is the one of a run without -qc
    assert cli.main(["-i", str(tmp_path / "Test_R1.fastq"), "-k", "7", "-c", "2", "-qc", "100", "-qc_paired", "-skipclean", "-o",
                     str(tmp_path / "pairs")]) == 0
    want = files_of(rule.run(raw, max_pos=100, paired=1))
    assert sorted(p.name for p in (tmp_path / "pairs" / "qc").iterdir()) == sorted("Test_R1_raw_%s.tsv" % name for name in report.QC_FILES)
    assert {name: (tmp_path / "pairs" / "qc" / ("Test_R1_raw_%s.tsv" % name)).read_bytes() for name in report.QC_FILES} == want
    assert cli.main(["-i", str(tmp_path / "Test_R1.fastq"), "-k", "7", "-c", "2", "-skipclean", "-o", str(tmp_path / "plain")]) == 0
    assert not (tmp_path / "plain" / "qc").exists()
    counts = (tmp_path / "plain" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes()
    assert counts == (tmp_path / "pairs" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes() and counts.count(b"\n") > 100
