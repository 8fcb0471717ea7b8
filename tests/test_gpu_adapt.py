"""3' adapter removal from a FASTQ text on the GPU (mk_fastq_adapt_text / mk_fastq_adapt_device, Counter.fastq_adapt*,
kmers.adapt_reads, -adapt).  Expected bytes, keep, rows, hits, figures and errors never come from the code under test:
the rule is tests/adapt_rule.py over Python bytes.  Equality is exact everywhere.  The call reads no table, so the
rule-level tests share one small context.

The scan kernel gives a record a wave and a lane one candidate position, 64 positions a block, counted from the aligned
16-byte granule in which the sequence line starts: a block ends at content index 64 b - (address of the line & 15) and
reads 128 bases past its last position.  The lengths below straddle those seams with the sequence line shifted through
all 16 alignments."""
import ctypes as C
import gzip
import re

import numpy as np
import pytest

import adapt_rule as rule
from conftest import GOLDEN
from mercat2_amd import cli, kmers, native

pytestmark = pytest.mark.gpu
NT = native.ALPHABET_NT2
ARG, RANGE, UNSUPPORTED = -1, -7, -8
BASES = np.frombuffer(b"ACGT", np.uint8)
FIGURES = ("records", "records_out", "records_trimmed", "dropped_short", "orphans", "bases_in", "bases_out", "bytes_out", "lines")
KITS = [s.encode() for _, s in native.ILLUMINA_ADAPTERS]
TRU = KITS[0]
LENGTHS = [0, 1, 7, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 4097]  # min_overlap is 8


@pytest.fixture(scope="module")
def ctx():
    with native.Counter(5, NT) as c:
        yield c


def raw_call(ctx, text, adapters, mates, opt, cap, keep, rows, hits, out_cap, piece_bytes=0):
    """mk_fastq_adapt_text with the panel as it stands (duplicates stay) and the arrays the caller chooses (None: NULL):
    (rc, out, out_len, nrec, message, figures)."""
    buf = np.frombuffer(text, np.uint8)
    bases = np.frombuffer(b"".join(adapters), np.uint8).copy()
    lengths = np.array([len(a) for a in adapters], np.uint32)
    m = None if mates is None else np.array(mates, np.uint8)
    out = np.full(max(out_cap, 0) + 8, 0xA5, np.uint8)
    out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), native.FastqAdapt()
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = ctx._L.mk_fastq_adapt_text(ctx._h, buf.ctypes.data if len(buf) else None, len(buf), piece_bytes, bases.ctypes.data,
                                    lengths.ctypes.data, ptr(m), len(adapters), C.byref(opt), cap, ptr(keep), ptr(rows), ptr(hits),
                                    out.ctypes.data if out_cap >= 0 else None, max(out_cap, 0), C.byref(out_len), C.byref(nrec), C.byref(st))
    msg = ctx._L.mk_last_error(ctx._h)
    return rc, out, out_len.value, nrec.value, (msg or b"").decode(), st.as_dict()


def check(ctx, text, adapters, mates=None, piece_bytes=0, **kw):
    """mk_fastq_adapt_text against the rule: bytes, keep, rows, hits and figures, or the error's code, record and kind.
    Returns the rule's result (or the message)."""
    o = rule.options(**kw)
    opt = native.AdaptOpt(**o)
    n = len(rule.records(text)[0])
    keep, rows, hits = np.zeros(n, np.uint8), np.zeros((n, 5), np.uint64), np.zeros(len(adapters), np.uint64)
    rc, out, out_len, nrec, msg, st = raw_call(ctx, text, adapters, mates, opt, n, keep, rows, hits, len(text) + 1, piece_bytes)
    try:
        want = rule.run(text, adapters, mates, **kw)
    except rule.AdaptError as err:
        assert rc == err.code, msg
        if err.record is not None:
            assert re.search(r"record %d\b" % err.record, msg) and rule.PHRASE[err.kind] in msg, msg
        if err.adapter is not None:
            assert re.search(r"adapter %d\b" % err.adapter, msg), msg
        return msg
    assert rc == 0, msg
    assert rows.tolist() == [list(r) for r in want["rows"]]
    assert keep.tolist() == want["keep"]
    assert out[:out_len].tobytes() == want["out"] and (out[out_len:] == 0xA5).all()
    assert hits.tolist() == want["hits"]
    assert {f: st[f] for f in FIGURES} == want["figures"] and nrec == n
    return want


def random_seq(rng, n, alphabet=BASES):
    return bytes(rng.choice(alphabet, n)) if n else b""


def record(i, seq, nl=b"\n", head_len=None):
    head = b"@r%d" % i
    if head_len is not None:
        head = (head + b"x" * head_len)[:max(head_len, 1)]
    return head + nl + seq + nl + b"+" + nl + bytes(33 + (j * 7 + i) % 41 for j in range(len(seq))) + nl


def planted(rng, i, n):
    """A random read of n bases; by turns none, a kit adapter inside it, one that runs off its end, one a base too short
    to count at its end."""
    seq = bytearray(random_seq(rng, n))
    kit = KITS[i % 3]
    turn = i % 4
    if turn == 1 and n > len(kit) + 4:
        at = int(rng.integers(0, n - len(kit)))
        seq[at:at + len(kit)] = kit
    elif turn == 2 and n >= 9:
        ov = int(rng.integers(8, min(len(kit), n) + 1))
        seq[n - ov:] = kit[:ov]
    elif turn == 3 and n >= 8:
        seq[n - 7:] = kit[:7]
    return bytes(seq)


def aligned_records(rng, lengths, nl=b"\n", at=0):
    """A record of every length for every alignment 0 .. 15 of its sequence line: the header is as long (1 .. 16 bytes)
    as puts the line there.  `at`: the bytes in front of the first record."""
    recs, i = [], 0
    for target in range(16):
        for n in lengths:
            head_len = (target - at - len(nl)) % 16 or 16
            recs.append(record(i, planted(rng, i, n), nl, head_len=head_len))
            at += len(recs[-1])
            i += 1
    return recs


def sequence_alignments(text):
    """{sequence length: the set of (first byte of the sequence line) & 15 over the records of that length}."""
    seen, at = {}, 0
    for head, seq, plus, qual in rule.records(text)[0]:
        seen.setdefault(len(rule.content(seq)), set()).add((at + len(head)) & 15)
        at += len(head) + len(seq) + len(plus) + len(qual)
    return seen


_SEAM = {}


def seam_text(crlf):
    if crlf not in _SEAM:
        rng = np.random.default_rng(5)
        nl = b"\r\n" if crlf else b"\n"
        recs = aligned_records(rng, LENGTHS, nl)
        long_ = bytearray(random_seq(rng, 70001))
        long_[69991:] = TRU[:10]  # found by the last of its 1094 blocks
        recs.append(record(len(recs), bytes(long_), nl))
        _SEAM[crlf] = (b"".join(recs), len(nl))
    return _SEAM[crlf]


@pytest.mark.parametrize("ending", ["newline", "open", "1 empty", "2 empty", "3 empty"])
@pytest.mark.parametrize("crlf", [False, True])
def test_seam_lengths(ctx, crlf, ending):
    text, nl = seam_text(crlf)
    if ending == "open":
        text = text[:-nl]
    elif ending != "newline":
        text += b"\n" * int(ending[0])
    seen = sequence_alignments(text)
    assert all(seen[n] == set(range(16)) for n in LENGTHS)  # (the text's buffer is 16-byte aligned on the device)
    want = check(ctx, text, KITS, min_len=2)
    assert want["rows"][-1] == (70001, 69991, 0, 10, 0) and all(h > 20 for h in want["hits"])
    assert 0 in want["keep"] and want["figures"]["records_trimmed"] > 60
    assert any(r[1] == r[0] and r[0] > 200 for r in want["rows"])


def test_a_very_long_read_at_every_alignment(ctx):
    rng = np.random.default_rng(6)
    recs, at = [], 0
    adapter = two_letter(rng, 128, b"AC")
    for target in range(16):
        seq = bytearray(two_letter(rng, 70001, b"GT"))  # G and T only: no chance hit of the A / C adapter
        where = 70001 - 128 + target if target % 2 else 35000 + 63 * target
        seq[where:where + 128] = adapter[:70001 - where]
        recs.append(record(target, bytes(seq), head_len=(target - at - 1) % 16 or 16))
        at += len(recs[-1])
    text = b"".join(recs)
    assert sequence_alignments(text)[70001] == set(range(16))
    want = check(ctx, text, [adapter], min_overlap=100, max_err_ppm=0)
    assert [r[1] for r in want["rows"]] == [70001 - 128 + t if t % 2 else 35000 + 63 * t for t in range(16)]
    assert [r[3] for r in want["rows"]] == [128 - t if t % 2 else 128 for t in range(16)]


# ------------------------------------------------------------------- adapter lengths, placements and overlaps
def two_letter(rng, n, letters):
    return random_seq(rng, n, np.frombuffer(letters, np.uint8))


@pytest.mark.parametrize("m", [1, 31, 32, 33, 64, 65, 96, 127, 128])
def test_every_overlap_of_every_adapter_length(ctx, m):
    """An adapter over A / C in reads over G / T: it hits only where it is planted -- at 0, inside, at every i from L - m
    to L - min_overlap (each overlap once), and not at L - min_overlap + 1."""
    rng = np.random.default_rng(m)
    adapter = two_letter(rng, m, b"AC")
    mo = min(m, 8)
    L = 150
    places = [0, 11] + list(range(L - m, L - mo + 1)) + [L - mo + 1]
    reads = []
    for i, at in enumerate(places):
        seq = bytearray(two_letter(rng, L, b"GT"))
        seq[at:at + m] = adapter[:L - at]
        reads.append(record(i, bytes(seq), head_len=1 + i % 16))
    want = check(ctx, b"".join(reads), [adapter], min_overlap=mo)
    assert want["rows"] == [(L, at, 0, min(m, L - at), 0) for at in places[:-1]] + [(L, L, rule.NO_HIT, 0, 0)]
    assert want["keep"][0] == 0 and want["figures"]["dropped_short"] == 1


@pytest.mark.parametrize("ov", [10, 13, 33, 40, 64, 65, 100, 128])
def test_the_mismatch_budget(ctx, ov):
    """floor(0.1 ov) mismatches hit and one more does not, wherever they stand: at the first base, the last, and on both
    sides of the seam between the first two words (j = 31, 32)."""
    rng = np.random.default_rng(ov)
    adapter = two_letter(rng, 128, b"AC")
    k = ov // 10
    L = 200
    flip = bytes.maketrans(b"AC", b"CA")
    firsts = list(dict.fromkeys(j for j in (0, ov - 1, 31, 32, 63, 64) if j < ov))
    reads, expect = [], []
    for count in (k, k + 1):
        for start in range(len(firsts)):
            order = firsts[start:] + firsts[:start] + [j for j in range(ov) if j not in firsts]
            seq = bytearray(two_letter(rng, L, b"GT"))
            seq[L - ov:] = adapter[:ov]
            for j in order[:count]:
                seq[L - ov + j:L - ov + j + 1] = seq[L - ov + j:L - ov + j + 1].translate(flip)
            reads.append(record(len(reads), bytes(seq), head_len=1 + (3 * len(reads)) % 16))
            expect.append((L, L - ov, 0, ov, k) if count == k else None)
    want = check(ctx, b"".join(reads), [adapter], min_overlap=8)
    for got, exp in zip(want["rows"], expect):
        if exp is not None:
            assert got == exp
        else:  # (a later, shorter overlap may still be admissible: the budget of the planted one is exceeded)
            assert got[1] > L - ov
    # the same reads against the budget in parts per million, at its edge
    check(ctx, b"".join(reads), [adapter], min_overlap=8, max_err_ppm=(k + 1) * 1000000 // ov)
    check(ctx, b"".join(reads), [adapter], min_overlap=8, max_err_ppm=-(-(k + 1) * 1000000 // ov))


def test_wildcards_and_folding(ctx):
    rng = np.random.default_rng(4)
    adapter = bytearray(two_letter(rng, 70, b"AC"))
    for j in (0, 5, 31, 32, 33, 63, 64, 69):
        adapter[j] = ord("N")
    adapter = bytes(adapter)
    plain = adapter.replace(b"N", b"A")
    reads = []
    for i, body in enumerate([plain, adapter, plain.lower(), adapter.lower(), plain.replace(b"A", b"G"), plain[:31] + b"N" + plain[32:],
                              plain[:31] + b"." + plain[32:], plain[:30] + bytes([0xC1]) + plain[31:], plain[:30] + b"n" + plain[31:]]):
        seq = two_letter(rng, 40 + i, b"GT") + body + two_letter(rng, 9, b"gt")
        reads.append(record(i, seq, head_len=1 + (5 * i) % 16))
    text = b"".join(reads)
    strict = check(ctx, text, [adapter], max_err_ppm=0)
    # an adapter N is free whatever the read holds; a read N, '.', 0xC1 against an adapter base mismatch
    assert [r[2] for r in strict["rows"]] == [0, 0, 0, 0, rule.NO_HIT, 0, 0, rule.NO_HIT, rule.NO_HIT]
    loose = check(ctx, text, [adapter.lower()], max_err_ppm=20000)  # one mismatch in 70
    assert [r[4] for r in loose["rows"]] == [0, 0, 0, 0, 0, 0, 0, 1, 1] and loose["rows"][4][2] == rule.NO_HIT
    check(ctx, text, [plain], max_err_ppm=150000)
    check(ctx, text, [b"N" * 20, adapter])  # all wildcards: admissible at 0 of every read


def test_the_choice(ctx):
    rng = np.random.default_rng(8)
    long_ = TRU + b"ACAC"
    tail = lambda n: two_letter(rng, n, b"T")
    reads = [tail(5) + long_ + tail(30), tail(10) + TRU + tail(17) + b"C" * 8 + tail(20), tail(40) + b"C" * 8 + tail(20), tail(70)]
    text = b"".join(record(i, s) for i, s in enumerate(reads))
    assert check(ctx, text, [long_, TRU])["rows"][0] == (52, 5, 0, 17, 0)  # both admissible at 5: the lower index
    assert check(ctx, text, [TRU, long_])["rows"][0] == (52, 5, 0, 13, 0)
    # adapter 5 admissible at 10 beats adapter 0 admissible at 40
    panel = [b"C" * 8, b"G" * 9, b"G" * 10, b"G" * 11, b"G" * 12, TRU]
    want = check(ctx, text, panel)
    assert want["rows"][1] == (68, 10, 5, 13, 0) and want["rows"][2] == (68, 40, 0, 8, 0) and want["hits"] == [1, 0, 0, 0, 0, 2]
    # duplicates report the lowest index of their class: the device compares each distinct (bases, class) once
    dup = [b"G" * 9, TRU, TRU.lower(), b"C" * 8, TRU, b"C" * 8]
    assert check(ctx, text, dup)["hits"] == [0, 2, 0, 1, 0, 0]
    want = check(ctx, text + text, dup, [1, 2, 1, 2, 3, 1], paired=1)
    assert [r[2] for r in want["rows"]] == [2, 1, 5, rule.NO_HIT, 2, 1, 5, rule.NO_HIT]


def test_a_large_panel_over_random_reads(ctx):
    """376 adapters a lane, mostly without a hit: every eighth read carries one of the panel."""
    rng = np.random.default_rng(376)
    panel = [random_seq(rng, int(n)) for n in rng.integers(18, 70, 376)]
    panel[100] = panel[7]
    reads = []
    for i in range(40):
        seq = bytearray(random_seq(rng, int(rng.integers(70, 131))))
        if i % 8 == 0:
            a = panel[(47 * i) % 376]
            at = int(rng.integers(20, len(seq) - 10))
            seq[at:] = a[:len(seq) - at]
        reads.append(record(i, bytes(seq), head_len=1 + i % 16))
    want = check(ctx, b"".join(reads), panel)
    assert sum(want["hits"]) >= 5 and want["hits"][100] == 0 and sum(1 for r in want["rows"] if r[2] == rule.NO_HIT) >= 30


# ------------------------------------------------------------------------------------------------------------- pairs
def pair_text():
    rng = np.random.default_rng(9)
    clean = lambda n: two_letter(rng, n, b"GT")
    first = lambda n: clean(n - 20) + TRU + clean(7)       # cut by the first mates' adapter
    second = lambda n: clean(n - 25) + KITS[1] + clean(6)  # cut by the second mates'
    gone = lambda n: KITS[2] + clean(n - 21)               # the small-RNA adapter at 0, searched in both
    plan = [(clean, clean), (first, second), (second, first), (gone, clean), (clean, gone), (gone, gone), (first, clean)] * 3
    return b"".join(record(2 * p, a(60 + p)) + record(2 * p + 1, b(90 - p)) for p, (a, b) in enumerate(plan))


def call_pairs(ctx, text, which, piece_bytes=0):
    info = {}
    got = ctx.fastq_adapt(text, [TRU, KITS[2]], [KITS[1], KITS[2]], paired=True, which=which, min_len=10, piece_bytes=piece_bytes, info=info)
    return got, info


@pytest.mark.parametrize("which", [1, 2])
def test_pairs(ctx, which):
    text = pair_text()
    want = rule.run(text, [TRU, KITS[2], KITS[1]], [1, 3, 2], paired=1, which=which, min_len=10)
    (out, keep, rows, hits), info = call_pairs(ctx, text, which)
    assert info["adapters"] == [TRU.decode(), KITS[2].decode(), KITS[1].decode()]
    assert out == want["out"] and keep.tolist() == want["keep"] and rows.tolist() == [list(r) for r in want["rows"]]
    assert hits.tolist() == want["hits"] == [6, 12, 3] and {f: info[f] for f in FIGURES} == want["figures"]
    # a class-2 adapter never cuts a first mate, a class-1 adapter never a second: those reads come back whole
    assert [r[2] for r in want["rows"][2:6]] == [0, 2, rule.NO_HIT, rule.NO_HIT]
    assert set(want["keep"]) == {0, 1, 2} and want["figures"]["orphans"] == 6 and len(out) > 0
    for piece in (1, 300, 1000):  # pieces end between pairs and do not show
        assert call_pairs(ctx, text, which, piece)[0][0] == out


def test_pairs_refusals_and_pieces(ctx):
    text = pair_text()
    recs = [b"".join(r) for r in rule.records(text)[0]]
    assert len(native.fastq_cuts(text, 1, pairs=True)) == len(recs) // 2 - 1
    odd = b"".join(recs[:-1])
    assert "odd" in check(ctx, odd, KITS, [1, 2, 3], paired=1)
    check(ctx, odd, KITS, [1, 2, 3], paired=0)
    check(ctx, text, KITS, which=2)  # ARG: the orphans are a matter of pairs
    whole = check(ctx, text, KITS, [1, 2, 3], paired=1, min_len=10)
    for piece in (1, 200, 777, 5000):
        for paired in (0, 1):
            want = check(ctx, text, KITS, [1, 2, 3], piece, paired=paired, min_len=10)
            assert not paired or want["out"] == whole["out"]
    for r in (0, 21, len(recs) - 1):
        bad = b"".join(spoil(rec, "plus") if i == r else rec for i, rec in enumerate(recs))
        for piece in (0, 1, 500):
            assert "record %d " % r in check(ctx, bad, KITS, None, piece, paired=1)
    with pytest.raises(ValueError):
        ctx.fastq_adapt(text, [TRU], [TRU])  # adapters2 without paired


# ------------------------------------------------------------------------------------------------------------ errors
def spoil(rec, kind):
    """A record (bytes) with one thing wrong."""
    head, seq, plus, qual = rec.split(b"\n")[:4]
    if kind == "at":
        head = b">" + head[1:]
    elif kind == "plus":
        plus = b"-" + plus[1:]
    elif kind == "length":
        qual = qual[:1] + qual
    return b"\n".join([head, seq, plus, qual]) + b"\n"


@pytest.mark.parametrize("kind", ["at", "plus", "length"])
def test_each_malformed_kind(ctx, kind):
    rng = np.random.default_rng(21)
    recs = [record(i, planted(rng, i, n)) for i, n in enumerate([30, 300, 17, 600, 5, 256, 80, 150, 64])]
    for where in (0, 4, len(recs) - 1):
        msg = check(ctx, b"".join(spoil(r, kind) if i == where else r for i, r in enumerate(recs)), KITS)
        assert isinstance(msg, str) and "record %d " % where in msg
        # the lowest record wins, whatever fails behind it
        later = [spoil(r, "at") if i > where else r for i, r in enumerate(recs)]
        assert "record %d " % where in check(ctx, b"".join(spoil(r, kind) if i == where else r for i, r in enumerate(later)), KITS)


def test_the_text_ends_inside_a_record(ctx):
    rng = np.random.default_rng(22)
    text = b"".join(record(i, planted(rng, i, 50)) for i in range(5))
    for cut_lines in (1, 2, 3):
        part = b"\n".join(text.split(b"\n")[:16 + cut_lines]) + b"\n"
        assert "record 4 " in check(ctx, part, KITS)
        assert "record 4 " in check(ctx, part, KITS, None, 1)


def test_refused_options_and_panels(ctx):
    rng = np.random.default_rng(23)
    text = b"".join(record(i, planted(rng, i, 60)) for i in range(4))
    for kw in (dict(min_overlap=0), dict(min_overlap=129), dict(max_err_ppm=1000001), dict(which=0), dict(which=2)):
        assert "mk_fastq_adapt_text" in check(ctx, text, KITS, **kw)
    assert "adapter 1 " in check(ctx, text, [TRU, b"ACGU", b"AC-T"])
    assert "adapter 0 " in check(ctx, text, [b"A" * 129])
    assert "adapter 2 " in check(ctx, text, KITS, [1, 2, 4])
    assert "1025 adapters" in check(ctx, text, [TRU] * 1025)
    check(ctx, text, [TRU] * 1024)
    check(ctx, text, [b"A" * 128] * 3, min_overlap=128)
    # qualities are carried, never read
    odd = text[:-3] + b" \x01\n"
    check(ctx, odd, KITS)


def test_cap_room_sizing_and_null_arrays(ctx):
    rng = np.random.default_rng(24)
    text = b"".join(record(i, planted(rng, i, 40 + 3 * i)) for i in range(60))
    want = rule.run(text, KITS, min_len=30)
    n, size = len(want["rows"]), len(want["out"])
    assert 0 < want["figures"]["records_trimmed"] and want["figures"]["dropped_short"] > 0
    opt = native.adapt_options(min_len=30)
    arrays = lambda m: (np.zeros(m, np.uint8), np.zeros((m, 5), np.uint64), np.zeros(3, np.uint64))
    # a cap that is too short: the count comes back
    keep, rows, hits = arrays(n - 1)
    rc, out, out_len, nrec, msg, _ = raw_call(ctx, text, KITS, None, opt, n - 1, keep, rows, hits, size)
    assert (rc, out_len, nrec) == (RANGE, 0, n) and "holds %d records" % n in msg and (out == 0xA5).all()
    # the sizing call, and one byte short: the size comes back, the arrays are complete, nothing is written
    for out_cap in (-1, size - 1):
        keep, rows, hits = arrays(n)
        rc, out, out_len, nrec, msg, _ = raw_call(ctx, text, KITS, None, opt, n, keep, rows, hits, out_cap)
        assert (rc, out_len, nrec) == (RANGE, size, n) and (out == 0xA5).all()
        assert keep.tolist() == want["keep"] and rows.tolist() == [list(r) for r in want["rows"]] and hits.tolist() == want["hits"]
    # exactly enough room; each array may be NULL, and cap says nothing without keep and rows
    for drop in (set(), {"keep"}, {"rows"}, {"hits"}, {"keep", "rows"}, {"keep", "rows", "hits"}):
        keep, rows, hits = arrays(n)
        rc, out, out_len, nrec, msg, st = raw_call(ctx, text, KITS, None, opt, 0 if {"keep", "rows"} <= drop else n,
                                                   None if "keep" in drop else keep, None if "rows" in drop else rows,
                                                   None if "hits" in drop else hits, size)
        assert (rc, out_len, nrec) == (0, size, n), msg
        assert out[:size].tobytes() == want["out"] and (out[size:] == 0xA5).all()
        assert keep.tolist() == ([0] * n if "keep" in drop else want["keep"])
        assert rows.tolist() == ([[0] * 5] * n if "rows" in drop else [list(r) for r in want["rows"]])
        assert hits.tolist() == ([0] * 3 if "hits" in drop else want["hits"])
        assert {f: st[f] for f in FIGURES} == want["figures"]
    # the empty text
    keep, rows, hits = arrays(1)
    rc, out, out_len, nrec, msg, _ = raw_call(ctx, b"", KITS, None, opt, 1, keep, rows, hits, 4)
    assert (rc, out_len, nrec) == (0, 0, 0)


# -------------------------------------------------------------------------------------------------------- device call
@pytest.mark.parametrize("lead,out_lead", [(0, 0), (3, 1), (15, 15)])
def test_device_call_agrees(ctx, lead, out_lead):
    import torch
    rng = np.random.default_rng(30)
    text = b"".join(record(i, planted(rng, i, 30 + (37 * i) % 190)) for i in range(120))
    kw = dict(min_len=40, paired=1, which=1)
    # (TruSeq for first mates, Nextera for second, the small-RNA adapter in both lists: classes 1, 3, 2 in panel order)
    lists = ([KITS[0], KITS[2]], [KITS[1], KITS[2]])
    want = rule.run(text, [KITS[0], KITS[2], KITS[1]], [1, 3, 2], **kw)
    n, size = len(want["rows"]), len(want["out"])
    assert set(want["keep"]) == {0, 1, 2} and all(want["hits"])
    options = dict(min_len=40, paired=True, which=1)
    d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
    d_keep = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    d_rows = torch.zeros((n, 5), dtype=torch.int64, device="cuda")
    d_hits = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.full((out_lead + size + 40,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = ctx.fastq_adapt_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, size, lists[0], lists[1], n,
                                  d_keep.data_ptr(), d_rows.data_ptr(), d_hits.data_ptr(), **options)
    got = d_out.cpu().numpy()
    assert got[out_lead:out_lead + size].tobytes() == want["out"]
    assert (got[:out_lead] == 0xA5).all() and (got[out_lead + size:] == 0xA5).all()
    assert d_keep.cpu().numpy()[:n].tolist() == want["keep"] and (d_keep.cpu().numpy()[n:] == 0xA5).all()
    assert d_rows.cpu().numpy().tolist() == [list(r) for r in want["rows"]]
    assert d_hits.cpu().numpy().tolist() == want["hits"]
    assert {f: info[f] for f in FIGURES} == want["figures"]
    text_out, keep, rows, hits = ctx.fastq_adapt(text, lists[0], lists[1], **options)
    assert text_out == got[out_lead:out_lead + size].tobytes() and keep.tolist() == want["keep"] and hits.tolist() == want["hits"]
    with pytest.raises(native.MercatHipError) as e:  # one byte short: refused, nothing written
        d_out.fill_(0xA5)
        torch.cuda.synchronize()
        ctx.fastq_adapt_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, size - 1, lists[0], lists[1], **options)
    assert e.value.code == RANGE and (d_out.cpu().numpy() == 0xA5).all()
    with pytest.raises(native.MercatHipError) as e:
        ctx.fastq_adapt_device(d_text.data_ptr(), len(text), d_out.data_ptr(), size, KITS, None, n, 0, d_rows.data_ptr() + 4, 0)
    assert e.value.code == ARG and "aligned" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:  # (refused before a byte is read)
        ctx.fastq_adapt_device(d_text.data_ptr(), 1 << 32, d_out.data_ptr(), size, KITS)
    assert e.value.code == RANGE and "2^32 - 1" in str(e.value)


# -------------------------------------------------------------------------------------------------------- end to end
def golden_reads():
    return gzip.open(GOLDEN / "inputs" / "Test_R1.fastq.gz", "rb").read()


def names_of(raw):
    return [h[1:].split()[0].decode() for h, _, _, _ in rule.records(raw)[0]]


def tsv_of(raw, want, adapter_names):
    lines = [b"record\tlength\tkept\tadapter\toverlap\tmismatches\tkeep\n"]
    for name, (L, kept, a, ov, mm), k in zip(names_of(raw), want["rows"], want["keep"]):
        lines.append(("\t".join([name, str(L), str(kept), "-" if a == rule.NO_HIT else adapter_names[a], str(ov), str(mm), str(k)]) + "\n").encode())
    return b"".join(lines)


def summary_of(want, adapter_names):
    f = want["figures"]
    lines = ["metric\tbefore\tafter", "reads\t%d\t%d" % (f["records"], f["records_out"]), "bases\t%d\t%d" % (f["bases_in"], f["bases_out"]),
             "trimmed\t\t%d" % f["records_trimmed"], "dropped_short\t\t%d" % f["dropped_short"], "orphans\t\t%d" % f["orphans"]]
    lines += ["adapter:%s\t\t%d" % (n, h) for n, h in zip(adapter_names, want["hits"]) if h]
    return ("\n".join(lines) + "\n").encode()


def test_adapt_reads_on_the_golden_file(tmp_path):
    raw = golden_reads()
    kit_names = [n for n, _ in native.ILLUMINA_ADAPTERS]
    want = rule.run(raw, KITS, min_overlap=5, max_err_ppm=200000, min_len=100)
    assert 0 < want["figures"]["records_trimmed"] and want["figures"]["dropped_short"] > 0
    done = kmers.adapt_reads(GOLDEN / "inputs" / "Test_R1.fastq.gz", tmp_path / "out.fastq.gz", min_overlap=5, max_err=0.2, min_len=100,
                             tsv_path=tmp_path / "out.tsv", summary_path=tmp_path / "summary.tsv", keep_text=True)
    assert gzip.open(tmp_path / "out.fastq.gz", "rb").read() == want["out"] == done["text"]
    assert {f: done[f] for f in FIGURES} == want["figures"] and done["hits"].tolist() == want["hits"] and done["adapter_names"] == kit_names
    assert (tmp_path / "out.tsv").read_bytes() == tsv_of(raw, want, kit_names)
    assert (tmp_path / "summary.tsv").read_bytes() == summary_of(want, kit_names)
    # the same reads as a pair of files with a panel file for the first mates and a list for the second: mates written
    # to two files, the orphans to a third
    recs = [b"".join(r) for r in rule.records(raw)[0]]
    (tmp_path / "a_1.fastq").write_bytes(b"".join(recs[0::2]))
    (tmp_path / "a_2.fastq").write_bytes(b"".join(recs[1::2]))
    (tmp_path / "panel.fna").write_bytes(b">tru\nAGATCGG\nAAGAGC\n>nex\n" + KITS[1] + b"\n")
    kw = dict(min_overlap=5, max_err_ppm=200000, min_len=100, paired=1)
    both = rule.run(raw, [KITS[0], KITS[1], KITS[2]], [1, 3, 2], which=1, **kw)
    lone = rule.run(raw, [KITS[0], KITS[1], KITS[2]], [1, 3, 2], which=2, **kw)
    done = kmers.adapt_reads(tmp_path / "a_1.fastq", tmp_path / "o_1.fastq", adapters=tmp_path / "panel.fna",
                             adapters2=[("second", KITS[2]), KITS[1].decode()], min_overlap=5, max_err=0.2, min_len=100,
                             mate_file=tmp_path / "a_2.fastq", out_path2=tmp_path / "o_2.fastq", singles_path=tmp_path / "singles.fastq",
                             tsv_path=tmp_path / "pairs.tsv")
    out = [b"".join(r) for r in rule.records(both["out"])[0]]
    assert (tmp_path / "o_1.fastq").read_bytes() == b"".join(out[0::2]) and (tmp_path / "o_2.fastq").read_bytes() == b"".join(out[1::2])
    assert (tmp_path / "singles.fastq").read_bytes() == lone["out"] and len(lone["out"]) > 0
    assert {f: done[f] for f in FIGURES} == both["figures"] and done["orphans"] > 0 and done["adapter_names"] == ["tru", "nex", "second"]
    assert (tmp_path / "pairs.tsv").read_bytes() == tsv_of(raw, both, ["tru", "nex", "second"])


def test_cli_adapt(tmp_path):
    raw = golden_reads()
    (tmp_path / "Test_R1.fastq").write_bytes(raw)
    kit_names = [n for n, _ in native.ILLUMINA_ADAPTERS]
    want = rule.run(raw, KITS, min_overlap=5, max_err_ppm=200000, min_len=100)
    common = ["-i", str(tmp_path / "Test_R1.fastq"), "-k", "7", "-c", "2"]
    flags = ["-adapt", "-adapt_overlap", "5", "-adapt_err", "0.2", "-adapt_len", "100"]
    assert cli.main(common + flags + ["-o", str(tmp_path / "cut")]) == 0
    folder = tmp_path / "cut" / "adapt"
    assert sorted(p.name for p in folder.iterdir()) == ["Test_R1_adapt.fastq", "Test_R1_adapt.tsv", "Test_R1_summary.tsv"]
    assert (folder / "Test_R1_adapt.fastq").read_bytes() == want["out"]
    assert (folder / "Test_R1_adapt.tsv").read_bytes() == tsv_of(raw, want, kit_names)
    assert (folder / "Test_R1_summary.tsv").read_bytes() == summary_of(want, kit_names)
    assert not (tmp_path / "cut" / "qtrim").exists()
    # the table is the one of the rule's output counted untrimmed
    (tmp_path / "ref").mkdir()
    (tmp_path / "ref" / "Test_R1.fastq").write_bytes(want["out"])
    assert cli.main(["-i", str(tmp_path / "ref" / "Test_R1.fastq"), "-k", "7", "-c", "2", "-skipclean", "-o", str(tmp_path / "plain")]) == 0
    counts = (tmp_path / "cut" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes()
    assert counts == (tmp_path / "plain" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes() and counts.count(b"\n") > 100
    # -adapt FILE and -qtrim together: the adapters go first, -qtrim sees what they leave, the count what -qtrim leaves
    import qtrim_rule
    (tmp_path / "panel.fna").write_bytes(b">nextera\n" + KITS[1] + b"\n>truseq\n" + KITS[0] + b"\n")
    first = rule.run(raw, [KITS[1], KITS[0]], min_overlap=5, max_err_ppm=200000)
    second = qtrim_rule.run(first["out"], cut_back=35, min_len=120)
    assert 0 < second["figures"]["records_trimmed"] and second["figures"]["records_out"] < first["figures"]["records_out"]
    assert cli.main(common + ["-adapt", str(tmp_path / "panel.fna"), "-adapt_overlap", "5", "-adapt_err", "0.2", "-qtrim", "35", "-qtrim_len",
                              "120", "-skipclean", "-o", str(tmp_path / "both")]) == 0
    assert (tmp_path / "both" / "adapt" / "Test_R1_adapt.fastq").read_bytes() == first["out"]
    assert (tmp_path / "both" / "adapt" / "Test_R1_adapt.tsv").read_bytes() == tsv_of(raw, first, ["nextera", "truseq"])
    assert (tmp_path / "both" / "qtrim" / "Test_R1_qtrim.fastq").read_bytes() == second["out"]
    (tmp_path / "ref2").mkdir()
    (tmp_path / "ref2" / "Test_R1.fastq").write_bytes(second["out"])
    assert cli.main(["-i", str(tmp_path / "ref2" / "Test_R1.fastq"), "-k", "7", "-c", "2", "-skipclean", "-o", str(tmp_path / "plain2")]) == 0
    counts2 = (tmp_path / "both" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes()
    assert counts2 == (tmp_path / "plain2" / "tsv_nucleotide" / "Test_R1_counts.tsv").read_bytes() and counts2 != counts
