"""Mate-overlap detection in interleaved FASTQ pairs on the GPU (mk_fastq_overlap_text / mk_fastq_overlap_device,
Counter.fastq_overlap*, kmers.overlap_reads, -overlap).  Expected bytes, keep, rows, figures and errors never come from the
code under test: the rule is tests/overlap_rule.py over Python bytes.  Equality is exact everywhere.  The call reads no
table, so the rule-level tests share one small context.

The scan kernel gives a pair a wave and a lane one candidate offset, 64 candidates a block in the rule's order (0 .. L1 -
min_overlap, then -1 .. -(L2 - min_overlap)); each mate's sequence line is loaded through the aligned 16-byte granules it
touches, 32 and one more, and packed into 64-bit words of 32 bases.  The lengths below straddle the word, block and frame
seams with each mate's sequence line shifted through all 16 alignments, and the planted offsets fall on the first and
last candidate of a block, on both sides of offset 0 and on the last candidate of all."""
import ctypes as C
import gzip
import re

import numpy as np
import pytest

import overlap_rule as rule
from mercat2_amd import cli, kmers, native

pytestmark = pytest.mark.gpu
NT = native.ALPHABET_NT2
ARG, RANGE, UNSUPPORTED = -1, -7, -8
BASES = np.frombuffer(b"ACGT", np.uint8)
FIGURES = ("records", "pairs", "pairs_hit", "pairs_merged", "pairs_trimmed", "dropped_short", "skipped_long", "records_out",
           "records_trimmed", "bases_in", "bases_out", "bytes_out", "lines")
LENGTHS = [0, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]  # min_overlap is 8
MODES = [(rule.TRIM, 1), (rule.MERGE, 1), (rule.MERGE, 2)]
MO = 8


@pytest.fixture(scope="module")
def ctx():
    with native.Counter(5, NT) as c:
        yield c


def raw_call(ctx, text, opt, cap, keep, rows, out_cap, piece_bytes=0):
    """mk_fastq_overlap_text with the arrays the caller chooses (None: NULL): (rc, out, out_len, nrec, message, figures)."""
    buf = np.frombuffer(text, np.uint8)
    out = np.full(max(out_cap, 0) + 8, 0xA5, np.uint8)
    out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), native.FastqOverlap()
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = ctx._L.mk_fastq_overlap_text(ctx._h, buf.ctypes.data if len(buf) else None, len(buf), piece_bytes, C.byref(opt), cap, ptr(keep),
                                      ptr(rows), out.ctypes.data if out_cap >= 0 else None, max(out_cap, 0), C.byref(out_len),
                                      C.byref(nrec), C.byref(st))
    msg = ctx._L.mk_last_error(ctx._h)
    return rc, out, out_len.value, nrec.value, (msg or b"").decode(), st.as_dict()


def check(ctx, text, piece_bytes=0, **kw):
    """mk_fastq_overlap_text against the rule: bytes, keep, rows and figures, or the error's code, record and kind.
    Returns the rule's result (or the message)."""
    o = rule.options(**kw)
    opt = native.OverlapOpt(**o)
    n = len(rule.records(text)[0])
    keep, rows = np.zeros(n, np.uint8), np.zeros((n, 5), np.uint64)
    rc, out, out_len, nrec, msg, st = raw_call(ctx, text, opt, n, keep, rows, len(text) + 1, piece_bytes)
    try:
        want = rule.run(text, **kw)
    except rule.OverlapError as err:
        assert rc == err.code, msg
        if err.record is not None:
            assert re.search(r"record %d\b" % err.record, msg) and rule.PHRASE[err.kind] in msg, msg
        return msg
    assert rc == 0, msg
    assert rows.tolist() == [list(r) for r in want["rows"]]
    assert keep.tolist() == want["keep"]
    assert out[:out_len].tobytes() == want["out"] and (out[out_len:] == 0xA5).all()
    assert {f: st[f] for f in FIGURES} == want["figures"] and nrec == n
    return want


def check_modes(ctx, text, piece_bytes=0, **kw):
    """check in trim mode, in merge mode, and for the unmerged pairs of merge mode; returns the three results."""
    return [check(ctx, text, piece_bytes, mode=mode, which=which, **kw) for mode, which in MODES]


def random_seq(rng, n, alphabet=BASES):
    return bytes(rng.choice(alphabet, n)) if n else b""


def random_qual(rng, n):
    return bytes(rng.integers(33, 127, n, dtype=np.uint8)) if n else b""


def record(name, seq, qual, nl=b"\n", head_len=None):
    head = b"@" + name
    if head_len is not None:
        head = (head + b"x" * head_len)[:max(head_len, 1)]
    return head + nl + seq + nl + b"+" + nl + qual + nl


def offset_of(c, L1, L2, mo=MO):
    """The offset of candidate c in the rule's order."""
    P = L1 - mo + 1
    return c if c < P else -(c - P + 1)


def mates(rng, L1, L2, d=None, spoil=()):
    """(s1, s2): random mates of L1 and L2 bases; with d, rc(s2) agrees with s1 over the overlap of offset d, but for the
    overlap positions (counted from the overlap's start) in spoil, which are substituted in mate 1."""
    s1, rc = bytearray(random_seq(rng, L1)), bytearray(random_seq(rng, L2))
    if d is not None:
        lo, hi = rule.overlap_of(d, L1, L2)
        for p in range(lo, hi):
            rc[p - d] = s1[p]
        for j in spoil:
            s1[lo + j] = b"ACGT"[(b"ACGT".index(s1[lo + j]) + 1) % 4]
    return bytes(s1), rule.revcomp(bytes(rc))


def pair(rng, i, s1, s2, nl=b"\n", head1=None, head2=None, q1=None, q2=None):
    q1 = random_qual(rng, len(s1)) if q1 is None else q1
    q2 = random_qual(rng, len(s2)) if q2 is None else q2
    return record(b"p%d/1" % i, s1, q1, nl, head1) + record(b"p%d/2" % i, s2, q2, nl, head2)


def planned_candidates(L1, L2, mo=MO):
    """Candidate indices worth a planted hit: the first and last of every block that exists, both sides of offset 0,
    the last of all."""
    if L1 < mo or L2 < mo:
        return []
    P, total = L1 - mo + 1, L1 - mo + 1 + L2 - mo
    want = {0, P - 1, P, total - 1}
    for b in range(0, total, 64):
        want |= {b, b + 63}
    return sorted(c for c in want if 0 <= c < total)


_SEAM = {}


def seam_text(crlf=False):
    """A pair of every length for every alignment 0 .. 15 of mate 1's sequence line (mate 2's goes through them in
    another order); every fourth alignment mixes the lengths.  The planted candidate walks through planned_candidates."""
    if crlf not in _SEAM:
        rng = np.random.default_rng(11)
        nl = b"\r\n" if crlf else b"\n"
        recs, plan, at, i = [], [], 0, 0
        for target in range(16):
            for idx, L1 in enumerate(LENGTHS):
                L2 = LENGTHS[(idx + target) % len(LENGTHS)] if target % 4 == 1 else L1
                cands = planned_candidates(min(L1, 512), min(L2, 512))
                d = None
                if cands and L1 <= 512 and L2 <= 512 and i % 7 != 6:  # (every seventh pair has no planted overlap)
                    d = offset_of(cands[(target + idx) % len(cands)], L1, L2)
                s1, s2 = mates(rng, L1, L2, d)
                head1 = (target - at - len(nl)) % 16 or 16
                r1 = record(b"p%d/1" % i, s1, random_qual(rng, L1), nl, head1)
                target2 = (5 * target + 3) % 16
                head2 = (target2 - at - len(r1) - len(nl)) % 16 or 16
                r2 = record(b"p%d/2" % i, s2, random_qual(rng, L2), nl, head2)
                recs += [r1, r2]
                plan.append((L1, L2, d))
                at += len(r1) + len(r2)
                i += 1
        _SEAM[crlf] = (b"".join(recs), plan)
    return _SEAM[crlf]


def sequence_alignments(text):
    """[{length: alignments of mate 1's sequence line}, {length: those of mate 2's}]."""
    seen, at = [{}, {}], 0
    for r, (head, seq, plus, qual) in enumerate(rule.records(text)[0]):
        seen[r % 2].setdefault(len(rule.content(seq)), set()).add((at + len(head)) & 15)
        at += len(head) + len(seq) + len(plus) + len(qual)
    return seen


@pytest.mark.parametrize("mode,which", MODES)
def test_seam_lengths_alignments_and_candidates(ctx, mode, which):
    text, plan = seam_text()
    seen = sequence_alignments(text)
    assert all(seen[0][n] == set(range(16)) for n in LENGTHS) and all(len(seen[1][n]) == 16 for n in LENGTHS)
    want = check(ctx, text, mode=mode, which=which, min_overlap=MO)
    # the planted offsets are found (a chance hit in front of one is rare), and they are the seams they were planned as
    found = [(L1, L2, d) for (L1, L2, d), row in zip(plan, want["rows"][0::2]) if d is not None and row[2] == d + L2]
    assert len(found) >= 0.95 * sum(1 for p in plan if p[2] is not None)
    index = lambda L1, L2, d: d if d >= 0 else L1 - MO - d  # the candidate's place in the rule's order
    places = {(index(*f) % 64, index(*f) == f[0] - MO + f[1] - MO) for f in found}
    assert {(0, False), (63, False)} <= places and any(last for _, last in places)
    assert {0, -1} <= {d for _, _, d in found} and any(d == L1 - MO for L1, _, d in found) and any(d == MO - L2 for _, L2, d in found)
    assert any(index(*f) >= 960 for f in found)  # the sixteenth block of a 512 / 512 pair
    assert want["figures"]["skipped_long"] >= 16 and want["figures"]["pairs_hit"] > 150
    if mode == rule.MERGE and which == 1:
        assert any(r[2] > r[0] for r in want["rows"][0::2]) and any(r[2] < r[0] for r in want["rows"][0::2])


@pytest.mark.parametrize("ending", ["open", "1 empty", "3 empty"])
@pytest.mark.parametrize("crlf", [False, True])
def test_line_ends_and_how_the_text_ends(ctx, crlf, ending):
    text, plan = seam_text(crlf)
    recs = [b"".join(r) for r in rule.records(text)[0]]
    text = b"".join(recs[:2 * 19 * 3])  # three alignments of every length
    text = text[:-(2 if crlf else 1)] if ending == "open" else text + b"\n" * int(ending[0])
    for want in check_modes(ctx, text, min_overlap=MO):
        assert want["figures"]["records_out"] > 0 and want["out"].endswith(b"\n")


# ------------------------------------------------------------------------------------------------- the mismatch budget
def budget_pairs():
    rng = np.random.default_rng(12)
    pairs, expect = [], []
    # (overlap, mismatches, hit): ov at min_overlap; mm at max_mismatch (5) and above; mm * 10^6 against 200000 ov
    cases = [(8, 0, True), (8, 1, True), (8, 2, False), (10, 2, True), (10, 3, False), (14, 2, True), (14, 3, False), (24, 4, True),
             (24, 5, False), (25, 5, True), (25, 6, False), (40, 5, True), (40, 6, False), (100, 5, True), (100, 6, False)]
    for ov, mm, hit in cases:
        for side in (0, 1):  # the overlap at the end of mate 1 (d > 0), and read-through (d < 0)
            L1, L2 = 150, 140
            d = L1 - ov if side == 0 else ov - L2
            where = [0, ov - 1, 31, 32, 33, 64, 5][:mm] if ov > 64 else ([0, ov - 1] + list(range(1, ov - 1)))[:mm]
            s1, s2 = mates(rng, L1, L2, d, spoil=where)
            pairs.append((s1, s2))
            expect.append((d + L2, ov, mm) if hit else None)
    return rng, pairs, expect


def test_the_mismatch_budget(ctx):
    rng, pairs, expect = budget_pairs()
    text = b"".join(pair(rng, i, s1, s2, head1=1 + i % 16, head2=1 + (3 * i) % 16) for i, (s1, s2) in enumerate(pairs))
    for want in check_modes(ctx, text, min_overlap=MO):
        for row, exp in zip(want["rows"][0::2], expect):
            if exp is not None:
                assert tuple(row[2:]) == exp
            else:  # (another, shorter overlap may be admissible by chance: the budget of the planted one is exceeded)
                assert row[2] == rule.NO_HIT or row[3] < 100
    assert sum(1 for row, exp in zip(want["rows"][0::2], expect) if exp is None and row[2] == rule.NO_HIT) >= 10
    # the same pairs at the edges of the three limits
    for kw in (dict(max_mismatch=4), dict(max_mismatch=6), dict(max_err_ppm=199999), dict(max_err_ppm=250000), dict(max_err_ppm=0),
               dict(max_err_ppm=1000000, max_mismatch=1000), dict(min_overlap=9), dict(min_overlap=101), dict(max_mismatch=0)):
        check(ctx, text, **dict(dict(min_overlap=MO), **kw))
        check(ctx, text, **dict(dict(min_overlap=MO, mode=rule.TRIM), **kw))


def test_n_lower_case_and_quality_bytes(ctx):
    rng = np.random.default_rng(13)
    L1, L2, ov = 90, 80, 40
    recs = []
    edits = [lambda a, b: (a, b), lambda a, b: (a.lower(), b), lambda a, b: (a, b.lower()),
             # mate 1's overlap is its bases 50 .. 89, mate 2's its bases 40 .. 79, base 50 + j against base 79 - j
             lambda a, b: (a[:60] + b"N" + a[61:], b), lambda a, b: (a, b[:45] + b"N" + b[46:]),           # N inside the overlap
             lambda a, b: (a[:3] + b"Nn" + a[5:], b[:5] + b"n" + b[6:]),                                  # N outside it
             lambda a, b: (a[:60] + b"n" + a[61:], b[:69] + b"n" + b[70:]),                               # N against N
             lambda a, b: (a[:70] + b"." + a[71:], b[:45] + bytes([0xC1]) + b[46:]),                      # bytes that are no base
             lambda a, b: (a[:55] + a[55:65].lower() + a[65:], b[:5] + b"N" * 3 + b[8:])]
    quals = [None, (33, 126), (126, 33), (70, 70), (33, 33), (126, 126)]
    i = 0
    for edit in edits:
        for q in quals:
            s1, s2 = edit(*mates(rng, L1, L2, L1 - ov, spoil=(7, 20) if i % 2 else ()))
            q1 = random_qual(rng, L1) if q is None else bytes([q[0]]) * L1
            q2 = random_qual(rng, L2) if q is None else bytes([q[1]]) * L2
            recs.append(pair(rng, i, s1, s2, head1=1 + i % 16, head2=1 + (7 * i) % 16, q1=q1, q2=q2))
            i += 1
    text = b"".join(recs)
    trim, merge, rest = check_modes(ctx, text, min_overlap=MO)
    assert merge["figures"]["pairs_merged"] == len(edits) * len(quals) and rest["out"] == b""
    assert len({r[4] for r in merge["rows"]}) >= 4
    out = rule.records(merge["out"])[0]
    assert any(b"N" in seq for _, seq, _, _ in out) and any(set(seq) & set(b"acgt") for _, seq, _, _ in out)
    check(ctx, text, min_overlap=MO, max_mismatch=2)
    check(ctx, text, min_overlap=MO, max_mismatch=2, mode=rule.TRIM)


def test_contained_mates_short_fragments_and_min_len(ctx):
    rng = np.random.default_rng(14)
    recs, shapes = [], [(100, 40, 0), (100, 40, 30), (100, 40, 60), (40, 100, 0), (40, 100, -60), (40, 100, -20), (64, 64, 0), (33, 33, -1),
                        (200, 200, -150), (200, 180, -172), (128, 96, 32), (8, 8, 0), (9, 8, 1), (8, 9, -1), (300, 20, 140)]
    for i, (L1, L2, d) in enumerate(shapes):
        s1, s2 = mates(rng, L1, L2, d)
        recs.append(pair(rng, i, s1, s2, head1=1 + (5 * i) % 16, head2=1 + (11 * i) % 16))
    text = b"".join(recs)
    for min_len in (0, 9, 41, 100, 1000):
        results = check_modes(ctx, text, min_overlap=MO, min_len=min_len)
        assert [r[2] for r in results[0]["rows"][0::2]] == [d + L2 for L1, L2, d in shapes]
    assert results[1]["figures"]["dropped_short"] == len(shapes) and results[1]["out"] == b""


# ----------------------------------------------------------------------------------------------- pieces, sizing, errors
def small_text(n_pairs=40, seed=15):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n_pairs):
        L1, L2 = int(rng.integers(20, 160)), int(rng.integers(20, 160))
        turn = i % 3
        d = None if turn == 0 else int(rng.integers(0, L1 - 12)) if turn == 1 else -int(rng.integers(1, L2 - 12))
        recs.append(pair(rng, i, *mates(rng, L1, L2, d), head1=1 + i % 16, head2=1 + (3 * i) % 16))
    return recs


def test_pieces_do_not_show(ctx):
    recs = small_text()
    text = b"".join(recs)
    assert len(native.fastq_cuts(text, 1, pairs=True)) == len(recs) - 1
    for results in zip(*[check_modes(ctx, text, piece, min_overlap=12, min_len=50) for piece in (0, 1, 300, 777, 5000)]):
        assert all(r["out"] == results[0]["out"] for r in results) and len(results[0]["out"]) > 0


def test_an_odd_record_count(ctx):
    text = b"".join(small_text(6))
    odd = b"".join(b"".join(r) for r in rule.records(text)[0][:-1])
    for mode, which in MODES:
        for piece in (0, 1):
            assert "odd" in check(ctx, odd, piece, mode=mode, which=which, min_overlap=12)


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
def test_each_malformed_kind_in_either_mate(ctx, kind):
    recs = [b"".join(r) for r in rule.records(b"".join(small_text(8)))[0]]
    for where in (0, 1, 6, 7, len(recs) - 2, len(recs) - 1):
        bad = [spoil(r, kind) if i == where else r for i, r in enumerate(recs)]
        for mode, which in MODES:
            assert "record %d " % where in check(ctx, b"".join(bad), mode=mode, which=which, min_overlap=12)
        later = [spoil(r, "at") if i > where else r for i, r in enumerate(bad)]  # the lowest record wins
        assert "record %d " % where in check(ctx, b"".join(later), 1, min_overlap=12)


def test_the_text_ends_inside_a_record(ctx):
    text = b"".join(small_text(3))
    for cut_lines in (1, 2, 3):
        part = b"\n".join(text.split(b"\n")[:16 + cut_lines]) + b"\n"
        assert "record 4 " in check(ctx, part, min_overlap=12)
        assert "record 4 " in check(ctx, part, 1, min_overlap=12, mode=rule.TRIM)


def test_refused_options(ctx):
    text = b"".join(small_text(4))
    for kw in (dict(mode=2), dict(min_overlap=0), dict(min_overlap=513), dict(max_err_ppm=1000001), dict(which=0), dict(which=3),
               dict(mode=rule.TRIM, which=2)):
        assert "mk_fastq_overlap_text" in check(ctx, text, **kw)
    check(ctx, text, min_overlap=512)
    check(ctx, text, min_overlap=1, max_mismatch=0, max_err_ppm=0)
    with pytest.raises(ValueError):
        ctx.fastq_overlap(text, mode="join")
    with pytest.raises(ValueError):
        ctx.fastq_overlap(text, max_err=1.5)


@pytest.mark.parametrize("mode,which", MODES)
def test_cap_room_sizing_and_null_arrays(ctx, mode, which):
    text = b"".join(small_text())
    kw = dict(mode=mode, which=which, min_overlap=12, min_len=50)
    want = rule.run(text, **kw)
    n, size = len(want["rows"]), len(want["out"])
    assert size > 0 and set(want["keep"]) == ({0, 1} if mode == rule.TRIM else {0, 1, 2})
    opt = native.OverlapOpt(**rule.options(**kw))
    arrays = lambda m: (np.zeros(m, np.uint8), np.zeros((m, 5), np.uint64))
    keep, rows = arrays(n - 1)  # a cap that is too short: the count comes back
    rc, out, out_len, nrec, msg, _ = raw_call(ctx, text, opt, n - 1, keep, rows, size)
    assert (rc, out_len, nrec) == (RANGE, 0, n) and "holds %d records" % n in msg and (out == 0xA5).all()
    for out_cap in (-1, size - 1):  # the sizing call, and one byte short: the size comes back, the arrays are complete
        keep, rows = arrays(n)
        rc, out, out_len, nrec, msg, _ = raw_call(ctx, text, opt, n, keep, rows, out_cap)
        assert (rc, out_len, nrec) == (RANGE, size, n) and (out == 0xA5).all()
        assert keep.tolist() == want["keep"] and rows.tolist() == [list(r) for r in want["rows"]]
    for drop in (set(), {"keep"}, {"rows"}, {"keep", "rows"}):  # each array may be NULL; cap says nothing without both
        keep, rows = arrays(n)
        rc, out, out_len, nrec, msg, st = raw_call(ctx, text, opt, 0 if {"keep", "rows"} <= drop else n, None if "keep" in drop else keep,
                                                   None if "rows" in drop else rows, size)
        assert (rc, out_len, nrec) == (0, size, n), msg
        assert out[:size].tobytes() == want["out"] and (out[size:] == 0xA5).all()
        assert keep.tolist() == ([0] * n if "keep" in drop else want["keep"])
        assert rows.tolist() == ([[0] * 5] * n if "rows" in drop else [list(r) for r in want["rows"]])
        assert {f: st[f] for f in FIGURES} == want["figures"]
    keep, rows = arrays(1)
    rc, out, out_len, nrec, msg, _ = raw_call(ctx, b"", opt, 1, keep, rows, 4)  # the empty text
    assert (rc, out_len, nrec) == (0, 0, 0)


# -------------------------------------------------------------------------------------------------------- device call
@pytest.mark.parametrize("lead,out_lead", [(0, 0), (3, 1), (15, 15)])
def test_device_call_agrees_and_leaves_its_text_alone(ctx, lead, out_lead):
    import torch
    text = b"".join(small_text(60, seed=16))
    d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text + b"#" * 5, dtype=np.uint8).copy()).cuda()
    before = d_text.cpu().numpy().copy()
    for mode, which in MODES:
        kw = dict(mode=mode, which=which, min_overlap=12, min_len=50)
        want = rule.run(text, **kw)
        n, size = len(want["rows"]), len(want["out"])
        options = dict(mode="merge" if mode else "trim", which=which, min_overlap=12, min_len=50)
        d_keep = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rows = torch.zeros((n, 5), dtype=torch.int64, device="cuda")
        d_out = torch.full((out_lead + size + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        info = ctx.fastq_overlap_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, size, n, d_keep.data_ptr(),
                                        d_rows.data_ptr(), **options)
        got = d_out.cpu().numpy()
        assert got[out_lead:out_lead + size].tobytes() == want["out"]
        assert (got[:out_lead] == 0xA5).all() and (got[out_lead + size:] == 0xA5).all()
        assert d_keep.cpu().numpy()[:n].tolist() == want["keep"] and (d_keep.cpu().numpy()[n:] == 0xA5).all()
        assert d_rows.cpu().numpy().tolist() == [list(r) for r in want["rows"]]
        assert {f: info[f] for f in FIGURES} == want["figures"]
        assert (d_text.cpu().numpy() == before).all()  # (a merging call patches a copy of its own)
        text_out, keep, rows = ctx.fastq_overlap(text, **options)
        assert text_out == want["out"] and keep.tolist() == want["keep"]
        with pytest.raises(native.MercatHipError) as e:  # one byte short: refused, nothing written
            d_out.fill_(0xA5)
            torch.cuda.synchronize()
            ctx.fastq_overlap_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, size - 1, **options)
        assert e.value.code == RANGE and (d_out.cpu().numpy() == 0xA5).all()
    with pytest.raises(native.MercatHipError) as e:
        ctx.fastq_overlap_device(d_text.data_ptr(), len(text), d_out.data_ptr(), size, n, 0, d_rows.data_ptr() + 4)
    assert e.value.code == ARG and "aligned" in str(e.value)
    with pytest.raises(native.MercatHipError) as e:  # (refused before a byte is read)
        ctx.fastq_overlap_device(d_text.data_ptr(), 1 << 32, d_out.data_ptr(), size)
    assert e.value.code == RANGE and "2^32 - 1" in str(e.value)


# -------------------------------------------------------------------------------------------------------- end to end
def names_of(raw):
    return [(h[1:].split() or [b""])[0].decode() for h, _, _, _ in rule.records(raw)[0]]  # (a header may be '@' alone)


def tsv_of(raw, want):
    lines = [b"record\tlength\tkept\tfragment\toverlap\tmismatches\tkeep\n"]
    for name, (L, kept, frag, ov, mm), k in zip(names_of(raw), want["rows"], want["keep"]):
        lines.append(("\t".join([name, str(L), str(kept), "-" if frag == rule.NO_HIT else str(frag), str(ov), str(mm), str(k)]) + "\n").encode())
    return b"".join(lines)


def summary_of(want):
    f = want["figures"]
    lines = ["metric\tbefore\tafter", "reads\t%d\t%d" % (f["records"], f["records_out"]), "bases\t%d\t%d" % (f["bases_in"], f["bases_out"]),
             "pairs\t\t%d" % f["pairs"], "hits\t\t%d" % f["pairs_hit"], "merged\t\t%d" % f["pairs_merged"], "trimmed\t\t%d" % f["pairs_trimmed"],
             "dropped_short\t\t%d" % f["dropped_short"], "skipped_long\t\t%d" % f["skipped_long"], "fragment\tpairs"]
    frags = sorted(r[2] for r in want["rows"][0::2] if r[2] != rule.NO_HIT)
    lines += ["%d\t%d" % (v, frags.count(v)) for v in sorted(set(frags))]
    return ("\n".join(lines) + "\n").encode()


def sample_text():
    return b"".join(small_text(51, seed=17))  # (an odd number of pairs: either file of mates alone is an odd text)


def split(text):
    recs = [b"".join(r) for r in rule.records(text)[0]]
    return b"".join(recs[0::2]), b"".join(recs[1::2])


def test_overlap_reads(tmp_path):
    raw = sample_text()
    first, second = split(raw)
    (tmp_path / "s.fastq").write_bytes(raw)
    (tmp_path / "s_1.fastq").write_bytes(first)
    with gzip.open(tmp_path / "s_2.fq.gz", "wb") as fh:
        fh.write(second)
    kw = dict(min_overlap=12, min_len=50)
    trim = rule.run(raw, mode=rule.TRIM, **kw)
    merge, rest = rule.run(raw, mode=rule.MERGE, which=1, **kw), rule.run(raw, mode=rule.MERGE, which=2, **kw)
    assert trim["figures"]["pairs_trimmed"] > 0 and merge["figures"]["pairs_merged"] > 0 and rest["out"] and merge["figures"]["dropped_short"] > 0
    # merge, interleaved in, gzip out
    done = kmers.overlap_reads(tmp_path / "s.fastq", tmp_path / "m.fastq.gz", unmerged_path=tmp_path / "u.fastq", tsv_path=tmp_path / "m.tsv",
                               summary_path=tmp_path / "m_summary.tsv", keep_text=True, **kw)
    assert gzip.open(tmp_path / "m.fastq.gz", "rb").read() == merge["out"] == done["text"]
    assert (tmp_path / "u.fastq").read_bytes() == rest["out"] == done["unmerged"]
    assert {f: done[f] for f in FIGURES} == merge["figures"]
    assert (tmp_path / "m.tsv").read_bytes() == tsv_of(raw, merge) and (tmp_path / "m_summary.tsv").read_bytes() == summary_of(merge)
    # merge, two files in, the unmerged pairs split
    done = kmers.overlap_reads(tmp_path / "s_1.fastq", tmp_path / "m2.fastq", mate_file=tmp_path / "s_2.fq.gz", unmerged_path=tmp_path / "u_1.fastq",
                               unmerged_path2=tmp_path / "u_2.fastq.gz", **kw)
    assert (tmp_path / "m2.fastq").read_bytes() == merge["out"]
    assert ((tmp_path / "u_1.fastq").read_bytes(), gzip.open(tmp_path / "u_2.fastq.gz", "rb").read()) == split(rest["out"])
    # trim, interleaved, and two files in and out
    done = kmers.overlap_reads(raw, tmp_path / "t.fastq", mode="trim", tsv_path=tmp_path / "t.tsv", summary_path=tmp_path / "t_summary.tsv", **kw)
    assert (tmp_path / "t.fastq").read_bytes() == trim["out"] and {f: done[f] for f in FIGURES} == trim["figures"]
    assert (tmp_path / "t.tsv").read_bytes() == tsv_of(raw, trim) and (tmp_path / "t_summary.tsv").read_bytes() == summary_of(trim)
    kmers.overlap_reads(tmp_path / "s_1.fastq", tmp_path / "t_1.fastq", mode="trim", mate_file=tmp_path / "s_2.fq.gz",
                        out_path2=tmp_path / "t_2.fastq", **kw)
    assert ((tmp_path / "t_1.fastq").read_bytes(), (tmp_path / "t_2.fastq").read_bytes()) == split(trim["out"])


@pytest.mark.parametrize("mode", ["merge", "trim"])
def test_cli_overlap(tmp_path, mode):
    raw = sample_text()
    (tmp_path / "S.fastq").write_bytes(raw)
    kw = dict(min_overlap=12, min_len=50)
    flags = ["-overlap", mode, "-overlap_min", "12", "-overlap_len", "50"]
    assert cli.main(["-i", str(tmp_path / "S.fastq"), "-k", "5", "-c", "1", "-o", str(tmp_path / "run")] + flags) == 0
    folder = tmp_path / "run" / "overlap"
    main = rule.run(raw, mode=rule.MERGE if mode == "merge" else rule.TRIM, **kw)
    if mode == "merge":
        assert sorted(p.name for p in folder.iterdir()) == ["S_merged.fastq", "S_overlap.tsv", "S_summary.tsv", "S_unmerged.fastq"]
        assert (folder / "S_merged.fastq").read_bytes() == main["out"]
        assert (folder / "S_unmerged.fastq").read_bytes() == rule.run(raw, mode=rule.MERGE, which=2, **kw)["out"]
    else:
        assert sorted(p.name for p in folder.iterdir()) == ["S_overlap.fastq", "S_overlap.tsv", "S_summary.tsv"]
        assert (folder / "S_overlap.fastq").read_bytes() == main["out"]
    assert (folder / "S_overlap.tsv").read_bytes() == tsv_of(raw, main) and (folder / "S_summary.tsv").read_bytes() == summary_of(main)
    # the table is the one of the text the rule says the count sees, counted as it stands
    (tmp_path / "ref").mkdir()
    (tmp_path / "ref" / "S.fastq").write_bytes(rule.seen_by_the_count(raw, rule.MERGE if mode == "merge" else rule.TRIM, **kw))
    assert cli.main(["-i", str(tmp_path / "ref" / "S.fastq"), "-k", "5", "-c", "1", "-skipclean", "-o", str(tmp_path / "plain")]) == 0
    counts = (tmp_path / "run" / "tsv_nucleotide" / "S_counts.tsv").read_bytes()
    assert counts == (tmp_path / "plain" / "tsv_nucleotide" / "S_counts.tsv").read_bytes() and counts.count(b"\n") > 100
    # the mates in two files give the same; an odd count names the sample
    first, second = split(raw)
    (tmp_path / "two").mkdir()
    (tmp_path / "two" / "S.fastq").write_bytes(first)
    (tmp_path / "S_2.fastq").write_bytes(second)
    assert cli.main(["-i", str(tmp_path / "two" / "S.fastq"), "-k", "5", "-c", "1", "-skipclean", "-o", str(tmp_path / "run2"), "-overlap_mate",
                     str(tmp_path / "S_2.fastq")] + flags) == 0
    assert (tmp_path / "run2" / "tsv_nucleotide" / "S_counts.tsv").read_bytes() == counts
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", str(tmp_path / "two" / "S.fastq"), "-k", "5", "-c", "1", "-o", str(tmp_path / "run3")] + flags)
    assert "S.fastq" in str(e.value) and "odd" in str(e.value)
