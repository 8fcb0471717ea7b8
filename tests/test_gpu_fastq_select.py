"""A keep / kept decision applied to a FASTQ text on the GPU (mk_fastq_select_text / mk_fastq_select_device,
Counter.fastq_select*, kmers.*(fastq_out=True), -fastq_out).  Expected bytes, figures and errors never come from the code
under test: the rule is tests/fastq_select_rule.py over Python bytes.  Equality is exact everywhere.  The call reads no
table, so the rule-level tests share one small context; the end-to-end tests load a table from a dict with
Counter.load_tsv, or count the golden FASTQ file."""
import ctypes as C
import functools
import gzip
import re

import numpy as np
import pytest

import fastq_select_rule as rule
from conftest import GOLDEN
from mercat2_amd import cli, kmers, native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
NT = native.ALPHABET_NT2
ARG, STATE, RANGE, UNSUPPORTED = -1, -4, -7, -8
BASES = np.frombuffer(b"ACGT", np.uint8)
MINIMAL = b"@\n\n+\n\n"
FIGURES = ("records", "records_out", "records_trimmed", "bases_out", "bytes_out", "lines")


@pytest.fixture(scope="module")
def ctx():
    with native.Counter(5, NT) as c:
        yield c


def read(rng, i, n, nl=b"\n", head=None, plus=b"+"):
    seq = bytes(rng.choice(BASES, n))
    qual = bytes(rng.integers(33, 74, n, dtype=np.uint8))
    return (b"@r%d" % i if head is None else head) + nl + seq + nl + plus + nl + qual + nl


def fastq(seed, lengths, crlf=False, final_newline=True):
    rng = np.random.default_rng(seed)
    nl = b"\r\n" if crlf else b"\n"
    text = b"".join(read(rng, i, n, nl) for i, n in enumerate(lengths))
    return text if final_newline else text[:-len(nl)]


def whole(text):
    """The complete records of the text, each as bytes."""
    return [b"".join(r) for r in rule.records(text)[0]]


def first_records(text, nbytes):
    out, size = [], 0
    for rec in whole(text):
        if size + len(rec) > nbytes:
            break
        out.append(rec)
        size += len(rec)
    return b"".join(out)


def seq_lengths(text):
    return [len(rule.content(r[1])) for r in rule.records(text)[0]]


def check(ctx, text, keep=None, kept=None, which=1, piece_bytes=0):
    """Counter.fastq_select against the rule: the bytes and the figures, or the error's code, record and kind."""
    try:
        want = rule.expected(text, keep, kept, which)
    except rule.SelectError as err:
        with pytest.raises(native.MercatHipError) as e:
            ctx.fastq_select(text, keep, kept, which, piece_bytes)
        msg = str(e.value)
        assert e.value.code == err.code, msg
        if err.record is not None:
            assert re.search(r"record %d\b" % err.record, msg) and rule.PHRASE[err.kind] in msg, msg
        if err.counts is not None:
            assert "holds %d records" % err.counts[0] in msg and "announced %d" % err.counts[1] in msg, msg
        return msg
    info = {}
    got = ctx.fastq_select(text, keep, kept, which, piece_bytes, info)
    assert got == want
    assert {f: info[f] for f in FIGURES} == rule.figures(text, keep, kept, which)
    assert len(got) <= len(text) + 1
    return got


def both_ways(ctx, text, seed=0):
    """The text under a random keep, under a random kept (whole, cut, dropped) and under both."""
    rng = np.random.default_rng(seed)
    L = np.array(seq_lengths(text), dtype=np.int64)
    keep = rng.integers(0, 3, len(L))
    kept = np.where(rng.random(len(L)) < 0.4, L, (rng.random(len(L)) * (L + 1)).astype(np.int64))
    check(ctx, text)
    check(ctx, text, keep=keep)
    check(ctx, text, keep=keep, which=2)
    check(ctx, text, kept=kept)
    check(ctx, text, keep=keep, kept=kept)


# --------------------------------------------------------------------------------------------- the line index
def record_with_newline_at(rng, start, target, line):
    """A record that starts at byte `start` and whose line `line` ends with its '\\n' at byte `target`."""
    gap = target - start
    if line == 0:
        rec = read(rng, 0, 4, head=b"@" + b"h" * (gap - 1))
    elif line == 1:
        rec = read(rng, 0, gap - 3, head=b"@r")
    elif line == 2:
        rec = read(rng, 0, 2, head=b"@r", plus=b"+" + b"p" * (gap - 7))
    else:
        rec = read(rng, 0, 2, head=b"@" + b"h" * (gap - 9))
    assert rec[gap:gap + 1] == b"\n" and rec[:gap + 1].count(b"\n") == line + 1
    return rec


@functools.lru_cache(maxsize=None)
def boundary_text():
    """Every line of a record ending with its '\\n' on the last byte of a lane's 16, a wave's 1024 and a tile's 4096
    bytes, and on the first byte of the next; one read of 9 000 bases (tiles without a newline); ends without newline."""
    rng = np.random.default_rng(7)
    parts, size, targets, i = [], 0, [], 0
    for line in range(4):
        for inner in (16 * 3, 1024, 0):  # a multiple of 16 only, of 1024 only, of 4096
            for off in (-1, 0):
                target = 8192 * (len(targets) + 1) + inner + off
                while size + 900 < target:
                    parts.append(read(rng, i, int(rng.integers(0, 200))))
                    size, i = size + len(parts[-1]), i + 1
                parts.append(record_with_newline_at(rng, size, target, line))
                size += len(parts[-1])
                targets.append(target)
    parts.append(read(rng, i, 9000))
    parts.append(read(rng, i + 1, 33)[:-1])
    text = b"".join(parts)
    assert all(text[t] == 10 for t in targets)
    return text


def test_newlines_at_lane_wave_and_tile_edges(ctx):
    text = boundary_text()
    assert len(text) > 24 * 8192 and max(seq_lengths(text)) == 9000 and not text.endswith(b"\n")
    both_ways(ctx, text, 1)
    check(ctx, text, kept=seq_lengths(text), piece_bytes=4096)


@pytest.mark.parametrize("text", [
    b"\n", b"@", MINIMAL, MINIMAL[:-1],
    b"@" + b"h" * 9 + b"\n\n+\n\n", b"@" + b"h" * 10 + b"\n\n+\n\n", b"@" + b"h" * 11 + b"\n\n+\n\n",   # 15, 16, 17 bytes
    b"@\n\n+" + b"p" * 9 + b"\n\n", b"@\n\n+" + b"p" * 10 + b"\n\n", b"@\n\n+" + b"p" * 11 + b"\n\n",
    b"@\nACGTA\n+\nIIIII", b"@\nACGTA\n+\nIIIII\n", b"@\nACGTAC\n+\nIIIIII",                                # 15, 16, 17 bytes
    MINIMAL + b"\n", MINIMAL + b"\n\n\n", MINIMAL * 2 + b"@\n\n+\n",
], ids=lambda t: "%d_bytes" % len(t))
def test_texts_around_one_minimal_record(ctx, text):
    n = len(rule.records(text)[0])
    check(ctx, text)
    check(ctx, text, keep=[1] * n)
    check(ctx, text, keep=[0] * n)
    check(ctx, text, kept=seq_lengths(text))
    check(ctx, text, kept=[min(1, s) for s in seq_lengths(text)])


def test_more_tiles_than_the_scan_has_threads(ctx):
    """4.2 MB: 1025 tiles and more for the 1024 threads of the one-workgroup scan, each of which then owns two tiles --
    the only count at which that scan changes shape."""
    rng = np.random.default_rng(3)
    text = fastq(3, [150] * 13600)
    assert 1025 * 4096 < len(text) < 1100 * 4096
    L = np.full(13600, 150)
    keep = (rng.random(13600) < 0.5).astype(np.uint8)
    kept = np.where(rng.random(13600) < 0.33, rng.integers(0, 150, 13600), L)
    check(ctx, text, keep=keep)
    check(ctx, text, keep=keep, kept=kept)


# ------------------------------------------------------------------------------------------------- the gather
def text_of_output_length(seed, want):
    """(text, keep): records of which the kept ones hold exactly `want` bytes together, dropped ones between them."""
    rng = np.random.default_rng(seed)
    parts, keep, total, i = [], [], 0, 0
    while True:
        for _ in range(int(rng.integers(0, 3))):
            parts.append(read(rng, i, int(rng.integers(0, 60))))
            keep.append(0)
            i += 1
        rec = read(rng, i, int(rng.integers(0, 120)))
        if want - total < len(rec) + 40:
            left = want - total  # the last kept record: its header pads the output to the byte
            rec = MINIMAL if left == 6 else read(rng, i, (left - 6) // 2, head=b"@" + b"h" * ((left - 6) % 2))
            assert len(rec) == left
        parts.append(rec)
        keep.append(1)
        total, i = total + len(rec), i + 1
        if total == want:
            parts.append(read(rng, i, 9))
            keep.append(0)
            return b"".join(parts), keep


@pytest.mark.parametrize("want", [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385])
def test_output_lengths(ctx, want):
    """Around a lane's 16 bytes, a store instruction's 1 KiB, a wave's 4 KiB and a workgroup's 16 KiB.  (No output is 1
    to 5 bytes long: the smallest record holds 6.)"""
    text, keep = text_of_output_length(want, want)
    assert len(check(ctx, text, keep=keep)) == want
    L = seq_lengths(text)
    check(ctx, text, keep=keep, kept=L)
    check(ctx, text, keep=keep, kept=[max(0, n - 1) for n in L])


def test_nothing_kept(ctx):
    text = fastq(5, [20] * 50)
    assert check(ctx, text, keep=[0] * 50) == b"" and check(ctx, text, kept=[0] * 50) == b""
    assert check(ctx, text, keep=[1] * 50, which=2) == b""


def test_minimal_records_three_to_a_chunk(ctx):
    text = MINIMAL * 700
    rng = np.random.default_rng(9)
    assert check(ctx, text) == text
    for p in (0.1, 0.5, 0.9):
        check(ctx, text, keep=(rng.random(700) < p).astype(np.uint8))
    check(ctx, text, keep=[1] * 700, kept=[0] * 700)


@pytest.mark.parametrize("ends_kept", [True, False])
def test_runs_of_dropped_records(ctx, ends_kept):
    keep = [1] if ends_kept else [0, 1]
    for run in (1, 2, 63, 64, 300):
        keep += [0] * run + [1]
    keep += [] if ends_kept else [0]
    rng = np.random.default_rng(13)
    text = fastq(13, rng.integers(0, 31, len(keep)).tolist())
    check(ctx, text, keep=keep)
    check(ctx, text, keep=keep, kept=seq_lengths(text))
    check(ctx, text, keep=[2 * k for k in keep], kept=[max(1, n) - 1 for n in seq_lengths(text)], which=2)


def test_everything_kept_is_the_input(ctx):
    text = fastq(17, np.random.default_rng(17).integers(1, 300, 400).tolist())
    assert check(ctx, text) == text and check(ctx, text, keep=[1] * 400) == text
    assert check(ctx, text, kept=seq_lengths(text)) == text and check(ctx, text, keep=[2] * 400, kept=seq_lengths(text), which=2) == text


@pytest.mark.parametrize("crlf", [False, True], ids=["lf", "crlf"])
@pytest.mark.parametrize("final_newline", [True, False], ids=["closed", "open"])
def test_trimmed_whole_crlf_and_open_records(ctx, crlf, final_newline):
    lengths = [1, 2, 15, 16, 17, 31, 32, 33, 100, 150, 151, 64, 5]
    text = fastq(19, lengths, crlf, final_newline)
    assert seq_lengths(text) == lengths
    copied = check(ctx, text)
    assert copied == (text if final_newline else text + b"\n")  # (CR LF stays CR LF; the open record is closed)
    for kept in ([1] * 13, [n - 1 for n in lengths], lengths, [0] * 12 + [5], [1] * 12 + [0]):
        got = check(ctx, text, kept=kept)
        assert all(len(r[1]) == len(r[3]) for r in rule.records(got)[0])
        check(ctx, text, keep=[1, 0] * 6 + [1], kept=kept)
    if not crlf and final_newline:
        assert check(ctx, text, kept=lengths) == text
    both_ways(ctx, text, 19)


@pytest.mark.parametrize("out_lead", [0, 1, 15])
def test_device_call_agrees(ctx, out_lead):
    import torch
    text = first_records(boundary_text(), 40000)
    L = seq_lengths(text)
    rng = np.random.default_rng(23)
    keep = rng.integers(0, 3, len(L)).astype(np.uint8)
    kept = (rng.random(len(L)) * (np.array(L) + 1)).astype(np.uint64)
    lead = 3
    d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
    d_keep = torch.from_numpy(keep).cuda()
    d_kept = torch.from_numpy(kept.view(np.int64)).cuda()
    assert d_text.data_ptr() % 16 == 0 and d_kept.data_ptr() % 8 == 0
    for kp, kt, which in ((None, None, 1), (d_keep, None, 1), (None, d_kept, 1), (d_keep, d_kept, 2)):
        want = rule.expected(text, None if kp is None else keep, None if kt is None else kept, which)
        d_out = torch.full((out_lead + len(want) + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        assert d_out.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        info = ctx.fastq_select_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, len(want), len(L),
                                       0 if kp is None else kp.data_ptr(), 0 if kt is None else kt.data_ptr(), which)
        got = d_out.cpu().numpy()
        assert got[out_lead:out_lead + len(want)].tobytes() == want
        assert (got[:out_lead] == 0xA5).all() and (got[out_lead + len(want):] == 0xA5).all()
        assert {f: info[f] for f in FIGURES} == rule.figures(text, None if kp is None else keep, None if kt is None else kept, which)
        with pytest.raises(native.MercatHipError) as e:  # one byte short: refused, nothing written
            d_out.fill_(0xA5)
            torch.cuda.synchronize()
            ctx.fastq_select_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, len(want) - 1, len(L),
                                    0 if kp is None else kp.data_ptr(), 0 if kt is None else kt.data_ptr(), which)
        assert e.value.code == RANGE and (d_out.cpu().numpy() == 0xA5).all()
    with pytest.raises(native.MercatHipError) as e:
        ctx.fastq_select_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr(), len(text) + 1, len(L), 0, d_kept.data_ptr() + 4)
    assert e.value.code == ARG and "aligned" in str(e.value)


# ------------------------------------------------------------------------------------------------- the pieces
def test_pieces_do_not_show(ctx):
    """piece_bytes 1 is raised to the smallest piece of the screen calls, 2 * (k + 24) = 58 bytes here: a record or two a
    piece; 64 and 4096 cut elsewhere; 0 takes the text whole."""
    rng = np.random.default_rng(29)
    text = fastq(29, rng.integers(0, 120, 300).tolist() + [700], final_newline=False)
    L = np.array(seq_lengths(text))
    keep = rng.integers(0, 3, len(L))
    kept = (rng.random(len(L)) * (L + 1)).astype(np.int64)
    assert len(native.fastq_cuts(text, 58)) > 200 > len(native.fastq_cuts(text, 4096)) > 3
    for args in ({}, {"keep": keep}, {"kept": kept}, {"keep": keep, "kept": kept, "which": 2}):
        outs, infos = [], []
        for piece in (1, 64, 4096, 0):
            infos.append({})
            outs.append(ctx.fastq_select(text, piece_bytes=piece, info=infos[-1], **args))
        assert outs[0] == outs[1] == outs[2] == outs[3] == rule.expected(text, **args)
        assert all({f: i[f] for f in FIGURES} == rule.figures(text, **args) for i in infos)
    # the same error whatever the pieces: a malformed record in the last piece, one in the first, a wrong count
    last = len(L) - 1
    recs = whole(text)
    broken = {"at": b"".join(recs[:-1]) + b">" + recs[-1][1:], "length": text + b"#",
              "incomplete": b"".join(recs[:-1]) + b"".join(rule.records(text)[0][-1][:2])}
    for kind, bad in broken.items():
        msgs = {check(ctx, bad, piece_bytes=piece) for piece in (1, 64, 4096, 0)}
        assert len(msgs) == 1 and re.search(r"record %d\b" % last, msgs.pop()), kind
    msgs = {check(ctx, text, kept=np.where(np.arange(len(L)) == last, L + 1, kept), piece_bytes=piece) for piece in (1, 64, 4096, 0)}
    assert len(msgs) == 1 and "record %d:" % last in msgs.pop()
    first_and_last = b">" + broken["at"][1:]
    msgs = {check(ctx, first_and_last, piece_bytes=piece) for piece in (1, 64, 4096, 0)}
    assert len(msgs) == 1 and re.search(r"record 0\b", msgs.pop())
    for n in (len(L) - 1, len(L) + 1, 1, 5 * len(L)):
        msgs = {check(ctx, text, keep=[1] * n, piece_bytes=piece) for piece in (1, 64, 4096, 0)}
        assert len(msgs) == 1
        msgs = {check(ctx, first_and_last, keep=[1] * n, piece_bytes=piece) for piece in (1, 64, 4096, 0)}
        assert len(msgs) == 1 and "announced" in msgs.pop()  # (the count is checked first)


# ------------------------------------------------------------------------------------------------- the errors
@pytest.mark.parametrize("kind,bad,kept", [
    ("at", b"rX\nACGT\n+\nIIII\n", None),
    ("at", b"\n@rX\nACGT\n+\nIII\n", None),
    ("plus", b"@rX\nACGT\n\nIIII\n", None),
    ("plus", b"@rX\nACGT\n-+\nIIII\n", None),
    ("length", b"@rX\nACGT\n+\nIII\n", None),
    ("length", b"@rX\nACGT\r\n+\nIIII\r\r\n", None),
    ("length", b"@rX\n\n+\nI\n", None),
    ("blank", b"@rX\nAC GT\n+\nIIIII\n", 1),
    ("blank", b"@rX\nACGT*\n+\nIIIII\n", 1),
    ("blank", b"@rX\n\tACGT\n+\nIIIII\n", 1),
    ("blank", b"@rX\nAC\rGT\n+\nIIIII\n", 1),
    ("blank", b"@rX\nACGT\r\r\n+\nIIIII\n", 1),
    ("blank", b"@rX\nAC\x1fGT\n+\nIIIII\n", 1),
    ("kept", b"@rX\nACGT\n+\nIIII\n", 5),
    ("kept", b"@rX\nACGT\r\n+\nIIII\r\n", 5),
])
@pytest.mark.parametrize("where", [0, 37, 99])
def test_each_malformed_kind(ctx, kind, bad, kept, where):
    lengths = [20] * 100
    good = fastq(31, lengths)
    recs = [b"".join(r) for r in rule.records(good)[0]]
    text = b"".join(recs[:where]) + bad + b"".join(recs[where + 1:])
    if bad.startswith(b"\n"):  # (an empty line shifts the records: the first that fails is the one it opens)
        assert rule.check(text, False) == (where, "at")
    arr = None if kept is None else [20] * where + [kept] + [20] * (99 - where)
    msg = check(ctx, text, kept=arr)
    assert isinstance(msg, str) and re.search(r"record %d\b" % where, msg) and rule.PHRASE[kind] in msg
    if kind == "blank":  # (without kept the sequence line may hold anything)
        assert check(ctx, text, keep=[1] * 100) == text


def test_the_sixteen_bytes_behind_a_lane_decide_a_cr(ctx):
    """A CR as the last byte of a lane's 16: whether it ends the line is in the next lane, or the next tile."""
    for edge in (16, 4096):
        for tail, nqual, fails in ((b"\r\n", 6, False), (b"\rA\n", 8, True)):
            head = b"@" + b"h" * (edge - 9)          # the sequence line starts at edge - 7: its 6 bases, then the CR at edge - 1
            text = head + b"\nACGTAC" + tail + b"+\n" + b"I" * nqual + b"\n"
            assert text[edge - 1] == 13 and text.index(b"\n") == edge - 8
            if fails:
                assert rule.PHRASE["blank"] in check(ctx, text, kept=[3])
            else:
                assert check(ctx, text, kept=[3]) == head + b"\nACG\n+\nIII\n"


def test_counts_which_sizing_and_room(ctx):
    text = fastq(37, [30] * 40)
    for n in (39, 41, 0, 400):
        assert "holds 40 records" in check(ctx, text, keep=[1] * n if n else np.zeros(0, np.uint8))
    assert "announced 1" in check(ctx, b"", keep=[1]) and check(ctx, b"", keep=np.zeros(0, np.uint8)) == b""
    for which in (0, 3, 255):
        with pytest.raises(native.MercatHipError) as e:
            ctx.fastq_select(text, keep=[1] * 40, which=which)
        assert e.value.code == ARG and "which" in str(e.value)
    assert ctx.fastq_select(text, kept=[30] * 40, which=9) == text  # (ignored without keep)
    with pytest.raises(ValueError):
        ctx.fastq_select(text, keep=[1] * 40, kept=[30] * 39)
    # the sizing call, room one byte short, exact room
    L = native.lib()
    keep = np.array([1, 0] * 20, np.uint8)
    want = rule.expected(text, keep=keep)
    need, st = C.c_size_t(0), native.FastqSelect()
    for piece in (0, 64):
        assert L.mk_fastq_select_text(ctx._h, text, len(text), piece, keep.ctypes.data, None, 40, 1, None, 0, C.byref(need), C.byref(st)) == RANGE
        assert need.value == len(want)
        out = np.full(len(want) + 8, 0xEE, np.uint8)
        assert L.mk_fastq_select_text(ctx._h, text, len(text), piece, keep.ctypes.data, None, 40, 1, out.ctypes.data, len(want) - 1,
                                      C.byref(need), C.byref(st)) == RANGE
        assert need.value == len(want) and (out[len(want) - 1:] == 0xEE).all()
        assert L.mk_fastq_select_text(ctx._h, text, len(text), piece, keep.ctypes.data, None, 40, 1, out.ctypes.data, len(want),
                                      C.byref(need), C.byref(st)) == 0
        assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xEE).all() and st.bytes_out == len(want) == need.value
    assert L.mk_fastq_select_text(ctx._h, text, len(text), 0, keep.ctypes.data, None, 40, 1, None, 0, None, None) == ARG


def test_an_open_chunk_is_refused():
    text = fastq(41, [30] * 4)
    with native.Counter(5, NT) as c:
        assert c.fastq_select(text) == text
        assert c._L.mk_chunk_begin(c._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            c.fastq_select(text)
        assert e.value.code == STATE and "chunk" in str(e.value)


def test_the_table_is_left_alone():
    text = fastq(43, [60] * 50)
    fasta, _ = native.fq2fa(text)
    with native.Counter(9, NT) as c:
        c.count_chunk(fasta, 1)
        before = c.to_dict()
        assert c.fastq_select(text, keep=[1, 0] * 25) == rule.expected(text, keep=[1, 0] * 25)
        assert c.to_dict() == before


# ------------------------------------------------------------------------------------------------- end to end
K = 21


@functools.lru_cache(maxsize=None)
def reads(interleaved: bool):
    """(raw FASTQ, its fq2fa form, the count table of the reads as a dict): 600 reads of 100 bases over a genome of 3 000
    with 1 % substitutions -- k-mers seen once where a read has an error, some twenty times elsewhere."""
    fasta = native.synth_reads(3000, 5, 600, 100, 6, 10000).tobytes()
    rng = np.random.default_rng(47)
    recs = fasta.split(b"\n")[:-1]
    raw = b"".join(b"@" + (b"p%d/%d" % (i // 2, 1 + i % 2) if interleaved else recs[2 * i][1:]) + b"\n" + recs[2 * i + 1] + b"\n+\n" +
                   bytes(rng.integers(33, 74, 100, dtype=np.uint8)) + b"\n" for i in range(600))
    fa, st = native.fq2fa(raw)
    assert st["reads"] == 600 and st["headers_dropped"] == 0
    return raw, fa, cpu_ref.count_text(fa, K, 1)


@pytest.fixture(scope="module")
def table():
    with native.Counter(K, NT) as c:
        tab = reads(False)[2]
        assert c.load_tsv(b"".join(b"%s\t%d\n" % (key.encode(), n) for key, n in tab.items()))["rows"] == len(tab)
        yield c


def same_reads(fq, fa_out):
    """The FASTQ output says what the FASTA output of the deciding call says: fq2fa of the one is the other."""
    got, st = native.fq2fa(fq)
    assert got == fa_out and st["headers_dropped"] == 0
    assert all(len(rule.content(r[1])) == len(rule.content(r[3])) for r in rule.records(fq)[0])


def test_filter_trim_and_norm_keep_their_qualities(table):
    raw, fa, _ = reads(False)
    for invert in (False, True):
        out, keep, _ = table.filter(fa, 2, 1, 1000000, invert)
        assert 0 < keep.sum() < 600
        fq = table.fastq_select(raw, keep=keep)
        same_reads(fq, out)
        assert fq == rule.expected(raw, keep=keep.astype(int))
    out, kept, _ = table.trim(fa, 2)
    assert 0 < sum(1 for n in kept if 0 < n < 100) and 0 < sum(1 for n in kept if n == 0) and 0 < sum(1 for n in kept if n == 100)
    fq = table.fastq_select(raw, kept=kept)
    same_reads(fq, out)
    assert fq == rule.expected(raw, kept=kept)
    for invert in (False, True):
        out, keep, _, _ = table.normalize(fa, 4, 0, 1, invert)
        assert 0 < keep.sum() < 600
        fq = table.fastq_select(raw, keep=keep, piece_bytes=4096)
        same_reads(fq, out)
        assert fq == rule.expected(raw, keep=keep.astype(int))


@pytest.mark.parametrize("op,args", [
    ("filter", {"at_least": 2, "min_ppm": 1000000}),
    ("filter", {"at_least": 2, "min_ppm": 1000000, "both": True}),
    ("trim", {"at_least": 2}),
    ("norm", {"target": 4, "seed": 1}),
], ids=["filter_either", "filter_both", "trim", "norm"])
def test_pairs_keep_their_qualities(table, op, args):
    raw, fa, _ = reads(True)
    out, singles, keep, own, _ = table.pairs(fa, op, singles=True, **args)
    kept = own if op == "trim" else None
    assert 0 < int((keep == 1).sum()) < 600 and (op in ("norm", "filter") and not args.get("both") or int((keep == 2).sum()) > 0)
    fq, fq_singles = table.fastq_select(raw, keep, kept, which=1), table.fastq_select(raw, keep, kept, which=2)
    same_reads(fq, out)
    same_reads(fq_singles, singles)
    assert fq == rule.expected(raw, keep, kept, 1) and fq_singles == rule.expected(raw, keep, kept, 2)
    first, second = native.split_pairs_fastq(fq)
    assert (first, second) == rule.split(fq) and first.count(b"\n") == second.count(b"\n") == 2 * int((keep == 1).sum())


def test_the_golden_fastq_file():
    raw = gzip.decompress((GOLDEN / "inputs" / "Test_R1.fastq.gz").read_bytes())
    fa, st = native.fq2fa(raw)
    assert st["headers_dropped"] == 0 and st["reads"] == 250
    with native.Counter(K, NT) as c:
        c.count_chunk(fa, 1)
        out, keep, _ = c.filter(fa, 2, 1, 0)
        assert 0 < keep.sum() < 250
        fq = c.fastq_select(raw, keep=keep)
        same_reads(fq, out)
        assert fq == rule.expected(raw, keep=keep.astype(int))
        out, kept, _ = c.trim(fa, 2)
        fq = c.fastq_select(raw, kept=kept)
        same_reads(fq, out)
        assert fq == rule.expected(raw, kept=kept) and 0 < len(fq) < len(raw)
        assert c.fastq_select(raw) == raw


def test_trim_reads_with_mate_files(table, tmp_path):
    raw, fa, _ = reads(True)
    first, second = rule.split(raw)
    (tmp_path / "r_1.fastq").write_bytes(first)
    with gzip.open(tmp_path / "r_2.fq.gz", "wb") as fh:
        fh.write(second)
    res = kmers.trim_reads(table, tmp_path / "r_1.fastq", tmp_path / "o_1.fastq", 2, mate_file=tmp_path / "r_2.fq.gz",
                           out_path2=tmp_path / "o_2.fastq", singles_path=tmp_path / "o_s.fastq", tsv_path=tmp_path / "o.tsv",
                           fastq_out=True)
    plain = kmers.trim_reads(table, tmp_path / "r_1.fastq", tmp_path / "o_1.fna", 2, mate_file=tmp_path / "r_2.fq.gz",
                             out_path2=tmp_path / "o_2.fna", singles_path=tmp_path / "o_s.fna", tsv_path=tmp_path / "p.tsv")
    o1, o2 = rule.records((tmp_path / "o_1.fastq").read_bytes())[0], rule.records((tmp_path / "o_2.fastq").read_bytes())[0]
    assert len(o1) == len(o2) == res["pairs_kept"] > 0 and res["singles"] > 0
    # mates stay aligned by position: the names differ in their last character only
    assert all(a[0][:-2] == b[0][:-2] and a[0].endswith(b"/1\n") and b[0].endswith(b"/2\n") for a, b in zip(o1, o2))
    assert all(len(r[1]) == len(r[3]) for r in o1 + o2)
    for name in ("o_1", "o_2", "o_s"):
        same_reads((tmp_path / (name + ".fastq")).read_bytes(), (tmp_path / (name + ".fna")).read_bytes())
    assert (tmp_path / "o.tsv").read_bytes() == (tmp_path / "p.tsv").read_bytes()
    assert {k_: v for k_, v in res.items() if k_ != "bytes_out"} == {k_: v for k_, v in plain.items() if k_ != "bytes_out"}
    assert res["bytes_out"] == (tmp_path / "o_1.fastq").stat().st_size + (tmp_path / "o_2.fastq").stat().st_size


def test_kmers_single_file_calls(table, tmp_path):
    raw, fa, _ = reads(False)
    (tmp_path / "r.fastq").write_bytes(raw)
    for name, run, run_fastq, args in (("filter", kmers.filter_reads, None, {"at_least": 2, "min_frac": 1.0}),
                                       ("trim", kmers.trim_reads, None, {"at_least": 2}),
                                       ("norm", kmers.normalize_reads, kmers.normalize_reads_fastq, {"target": 4, "seed": 1})):
        if run_fastq is None:
            res = run(table, tmp_path / "r.fastq", tmp_path / (name + ".fastq"), fastq_out=True, **args)
        else:
            res = run_fastq(table, tmp_path / "r.fastq", tmp_path / (name + ".fastq"), **args)
        plain = run(table, tmp_path / "r.fastq", tmp_path / (name + ".fna"), **args)
        same_reads((tmp_path / (name + ".fastq")).read_bytes(), (tmp_path / (name + ".fna")).read_bytes())
        assert res["bytes_out"] == (tmp_path / (name + ".fastq")).stat().st_size > plain["bytes_out"] > 0
        assert {k_: v for k_, v in res.items() if k_ != "bytes_out"} == {k_: v for k_, v in plain.items() if k_ != "bytes_out"}


def test_cli_trim_paired_singles_fastq_out(tmp_path):
    raw, fa, _ = reads(True)
    (tmp_path / "s.fna").write_bytes(fa)
    (tmp_path / "pairs.fastq").write_bytes(raw)
    base = ["-i", str(tmp_path / "s.fna"), "-k", str(K), "-c", "1", "-skipclean", "-trim", str(tmp_path / "pairs.fastq"), "-paired", "-singles"]
    assert cli.main(base + ["-fastq_out", "-o", str(tmp_path / "fq")]) == 0
    assert cli.main(base + ["-o", str(tmp_path / "fa")]) == 0
    assert sorted(p.name for p in (tmp_path / "fq" / "trim_nucleotide").iterdir()) == ["s_singles.fastq", "s_trim.tsv", "s_trimmed.fastq"]
    for name in ("s_trimmed", "s_singles"):
        fq = (tmp_path / "fq" / "trim_nucleotide" / (name + ".fastq")).read_bytes()
        assert len(fq) > 0
        same_reads(fq, (tmp_path / "fa" / "trim_nucleotide" / (name + ".fna")).read_bytes())
    assert (tmp_path / "fq" / "trim_nucleotide" / "s_trim.tsv").read_bytes() == (tmp_path / "fa" / "trim_nucleotide" / "s_trim.tsv").read_bytes()
