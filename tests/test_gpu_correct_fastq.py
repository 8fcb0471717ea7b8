"""FASTQ reads corrected on the GPU with their qualities kept (mk_correct_fastq_text / mk_correct_fastq_device,
Counter.correct_fastq*, kmers.correct_reads_fastq, -correct_fastq / -correct_qual).  Expected values never come from the
code under test: the rule is tests/correct_fastq_rule.py (plain Python over fastq_select_rule, correct_rule and
trim_rule), the table is a dict loaded with Counter.load_tsv.  Equality is exact everywhere."""
import ctypes
import functools
import gzip
import random
import zlib

import numpy as np
import pytest

import correct_fastq_rule as cfr
import fastq_select_rule as fsr
import trim_rule
from mercat2_amd import cli, kmers, native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
NT, AA = native.ALPHABET_NT2, native.ALPHABET_AA5
ARG, STATE, NON_ASCII, RANGE, UNSUPPORTED = -1, -4, -5, -7, -8
COMP = bytes.maketrans(b"ACGT", b"TGCA")
NEXT = bytes.maketrans(b"ACGT", b"CGTA")


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def sub(seq: bytes, at) -> bytes:
    """``seq`` with the next base of ACGT at every position of ``at`` that it has (negative: from the end)."""
    out = bytearray(seq)
    for p in at:
        if -len(out) <= p < len(out):
            out[p] = bytes([out[p]]).translate(NEXT)[0]
    return bytes(out)


def qual_of(rng, n, first=None):
    q = bytes(rng.choice(b"#$%&'()5:?DFHIJ") for _ in range(n))
    return (first + q[1:]) if first and n else q


def table_of(seqs, k, fold=False, count=None):
    table = {}
    for seq in seqs:
        for j in range(len(seq) - k + 1):
            w = seq[j:j + k]
            if fold and set(w) <= set(b"ACGT"):
                w = min(w, w.translate(COMP)[::-1])
            table[w.decode()] = count if count is not None else table.get(w.decode(), 0) + 1
    return table


def load(ctx, table):
    assert ctx.load_tsv(b"".join(b"%s\t%d\n" % (key.encode(), c) for key, c in table.items()))["rows"] == len(table)


def check(ctx, text, table, at_least=2, new_qual=0, want=None, **kw):
    """Counter.correct_fastq against the rule: bytes, fix, rows (Counter.screen's for the FASTA view) and the figures."""
    info = {}
    out, fix, rows = ctx.correct_fastq(text, at_least, new_qual, info=info, **kw)
    w_out, w_fix = want if want is not None else cfr.expected(text, table, ctx.k, at_least, native.quality_byte(new_qual), ctx.canonical)
    assert out == w_out
    assert fix.dtype == np.uint32 and fix.shape == (len(w_fix), 4) and [tuple(r) for r in fix.tolist()] == w_fix
    assert rows.tolist() == ctx.screen(cfr.view(text), at_least).tolist()
    fig = cfr.figures(text, w_fix)
    assert {n: info[n] for n in fig} == fig and info["patched"] == info["fixed"] and info["bytes_out"] == len(text)
    assert info["preamble"] == 0 and info["s_gather"] == 0 and info["bytes"] == len(text)
    assert info["candidates"] == info["fixed"] + info["ambiguous"] + info["unfixable"]
    return (out, fix, rows), info


# --------------------------------------------------------------------------------------------- record shapes
@functools.lru_cache(maxsize=None)
def shapes(k: int):
    """(clean sequences, FASTQ text with substitutions): every record length, a base substituted at 0, k - 1, k, L - k,
    L - 1, the middle, and two within k of each other; N and a lower-case letter at p and beside it; + lines of length
    1, 17 and L + 40; headers holding '>', '@' and blanks; a quality line that starts with '@'; CR LF records next to LF
    records; an open last record."""
    rng = random.Random(77 * k)
    clean, recs = [], []

    def add(n, at=(), head=None, plus=1, nl=b"\n", first=None, change=None, source=None):
        seq = source if source is not None else dna(rng, n)
        clean.append(seq)
        bad = sub(seq, at)
        if change:
            bad = bad[:change[0]] + change[1] + bad[change[0] + 1:]
        head = head if head is not None else b"@r%d" % len(recs)
        pl = b"+" + (b"x" * (plus - 1) if plus < 40 else head[1:] + b"y" * (plus - len(head)))
        recs.append(head + nl + bad + nl + pl[:max(plus, 1)] + nl + qual_of(rng, len(bad), first) + nl)

    L = 4 * k + 9
    for n in (0, k - 1, k, k + 1, 2 * k + 3):
        add(n, (0,))
    add(k + 1, (-1,), head=b"@ >odd @ header\twith blanks ", plus=17)
    add(2 * k + 3, (k - 1,), head=b"@>", plus=2 * k + 3 + 40, first=b"@")
    for i, at in enumerate(((0,), (k - 1,), (k,), (-k,), (-1,), (L // 2,), (), (k + 2, 2 * k + 1), (k + 2, 2 * k + 2), (0, -1))):
        add(L, at, nl=b"\r\n" if i % 3 == 1 else b"\n", plus=(1, 17, L + 40)[i % 3], first=(b"@", b">", b"+")[i % 3])
    add(L, (), change=(2 * k, b"N"))                                  # an N at p: four alternatives
    with_n = dna(rng, L)
    with_n = with_n[:2 * k + 3] + b"N" + with_n[2 * k + 4:]
    add(L, (2 * k,), source=with_n)                                   # an N beside p: text probes
    add(L, (), change=(2 * k, b"n"))                                  # a lower-case letter at p
    lower = dna(rng, L)
    lower = lower[:10] + lower[10:14].lower() + lower[14:]
    add(L, (16,), source=lower)                                       # a base behind lower-case letters
    add(0, nl=b"\r\n")
    add(2 * k + 4, (-1,))
    text = b"".join(recs)
    return tuple(clean), text[:-1]  # (the last record stays open)


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("k", [5, 31, 32, 33, 63])
def test_record_shapes(k, fold):
    clean, bad = shapes(k)
    table = table_of(clean, k, fold)
    assert not bad.endswith(b"\n") and b"\r\n" in bad
    with native.Counter(k, NT, canonical=fold) as ctx:
        load(ctx, table)
        (out, fix, rows), info = check(ctx, bad, table, 1)
        assert info["pieces"] == 1 and (info["folded"] > 0) == fold and info["headless"] == 0
        if k > 5:  # (no window is there twice by chance: every isolated substitution comes back)
            got = [fsr.content(r[1]) for r in fsr.records(out)[0]]
            two_close = {14, 15}  # two substitutions k - 1 and k apart: one run, too long, left alone
            for r, seq in enumerate(clean):
                if r in two_close:
                    assert fix[r].tolist() == [1, 0, 0, 0] and got[r] != seq
                elif len(seq) > k:
                    assert got[r] == seq, r
            assert info["fixed"] >= 17 and info["text_windows"] > 0
        check(ctx, bad, table, 1, new_qual="!")
        check(ctx, out, table, 1)  # a second pass: the rule again, on what the first one wrote
        for extra in (b"\n", b"\n\n", b"\n\n\n", b"\n\n\n\n"):  # the record closed, then one to three trailing empty lines
            (out2, _, _), info2 = check(ctx, bad + extra, table, 1)
            assert out2 == out + extra and info2["lines"] == info["lines"] + len(extra) - 1


# ----------------------------------------------------------------------------------------------------- seams
K5 = 5
SEAM_CLEAN = b"ACGTTGCAAGGCTTAGACCGATATCGGA"  # every 5-mer once


def seam_text(target: int, which: str, tail: bytes = b""):
    """A text whose one wrong base (position 0 of a read of 6: a run of one window at the record's start), or that base's
    quality byte, is byte ``target`` of the text; clean records in front of it fill the space."""
    seq, rng = SEAM_CLEAN[3:9], random.Random(target)
    body = len(seq) + 1 + 2 if which == "qual" else 0  # bytes between the header's end and the byte
    filler = []
    left = target - body
    while left > 300:
        n = rng.randrange(6, 29)
        rec = b"@f%d\n" % len(filler) + SEAM_CLEAN[:n] + b"\n+\n" + qual_of(rng, n) + b"\n"
        filler.append(rec)
        left -= len(rec)
    assert left >= 2
    head = b"@" + b"h" * (left - 2) + b"\n"
    text = b"".join(filler) + head + sub(seq, (0,)) + b"\n+\n" + qual_of(rng, len(seq)) + b"\n" + tail
    at = len(b"".join(filler)) + len(head) + body
    assert at == target
    return text


@pytest.mark.parametrize("which", ["seq", "qual"])
def test_seams_of_lane_wave_and_tile(which):
    table = table_of([SEAM_CLEAN], K5, count=2)
    tail = b"@t\n" + SEAM_CLEAN + b"\n+\n" + b"I" * len(SEAM_CLEAN) + b"\n"
    with native.Counter(K5, NT) as ctx:
        load(ctx, table)
        for edge in (16, 1024, 4096):
            for target in (edge - 1, edge):
                text = seam_text(target, which, tail)
                (out, fix, _), info = check(ctx, text, table, 2, new_qual="~")
                assert info["fixed"] == 1 and fix[-2].tolist() == [1, 1, 0, 0]
                changed = [i for i, (a, b) in enumerate(zip(out, text)) if a != b]
                assert target in changed and len(changed) == 2 and out[changed[1]] == ord("~")


def test_long_read_and_many_tiles():
    k = 31
    rng = random.Random(31)
    long_read = dna(rng, 9_000)
    reads = [dna(rng, 150) for _ in range(40)]
    table = table_of([long_read] + reads, k, count=3)
    recs = [b"@long\n" + sub(long_read, range(5, 9_000, 997)) + b"\n+\n" + qual_of(rng, 9_000) + b"\n"]
    for i, r in enumerate(reads):  # + lines of 110 KB: more than 1025 tiles of 4096 bytes, few bases
        recs.append(b"@r%d\n" % i + sub(r, (i * 3 % 150,)) + b"\n+" + b"z" * 110_000 + b"\n" + qual_of(rng, 150) + b"\n")
    text = b"".join(recs)
    assert len(text) > 1025 * 4096
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        want = cfr.expected(text, table, k, 2, ord("I"))
        (out, fix, _), info = check(ctx, text, table, 2, new_qual="I", want=want)
        assert fix[0].tolist() == [10, 10, 0, 0] and info["fixed"] == 50 and info["pieces"] == 1
        assert fsr.content(fsr.records(out)[0][0][1]) == long_read
        (out_p, _, _), info_p = check(ctx, text, table, 2, new_qual="I", want=want, piece_bytes=300_000)
        assert out_p == out and info_p["pieces"] > 8


# -------------------------------------------------------------------------------------------------- new_qual
@functools.lru_cache(maxsize=None)
def reads_text(k: int, n: int = 120, seed: int = 1):
    """(genome, FASTQ text): reads of a small genome, a substitution or two in most, LF-terminated."""
    rng = random.Random(seed * 1000 + k)
    genome = dna(rng, 2_000)
    recs = []
    for i in range(n):
        at = rng.randrange(0, len(genome) - 100)
        L = rng.randrange(2 * k, 100) if k < 40 else 100
        seq = sub(genome[at:at + L], [rng.randrange(L), rng.randrange(L)][:i % 3])
        recs.append(b"@read%d len=%d\n" % (i, L) + seq + b"\n+" + (b"read%d" % i if i % 2 else b"") + b"\n" +
                    qual_of(rng, L, (b">", b"@", None)[i % 3]) + b"\n")
    return genome, b"".join(recs)


def test_new_qual():
    k = 15
    genome, text = reads_text(k)
    table = table_of([genome], k, count=3)
    quals = lambda t: [r[3] for r in fsr.records(t)[0]]
    seqs = lambda t: [r[1] for r in fsr.records(t)[0]]
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (plain, fix, _), info = check(ctx, text, table, 2, new_qual=0)
        assert quals(plain) == quals(text) and info["fixed"] > 40
        for q in ("!", b"I", 73):
            (out, fix_q, _), info_q = check(ctx, text, table, 2, new_qual=q)
            assert seqs(out) == seqs(plain) and fix_q.tolist() == fix.tolist()
            want = native.quality_byte(q)
            for s0, s1, q0, q1 in zip(seqs(text), seqs(out), quals(text), quals(out)):
                assert all((b == want) if x != y else (a == b) for x, y, a, b in zip(s0, s1, q0, q1))
        for q in (10, 32, 127, 256):
            with pytest.raises(native.MercatHipError) as e:
                ctx.correct_fastq(text, 2, q)
            assert e.value.code == ARG and "new_qual" in str(e.value)


# ------------------------------------------------------------------------------------------------ thresholds
def test_thresholds():
    k = 15
    genome, text = reads_text(k, seed=2)
    hashed = {key: zlib.crc32(key.encode()) % 7 for key in table_of([genome], k)}
    hashed = {key: c for key, c in hashed.items() if c}
    with native.Counter(k, NT) as ctx:
        load(ctx, hashed)
        for at_least in (1, 2, 5):
            _, info = check(ctx, text, hashed, at_least)
            assert info["runs"] > 100
    own = table_of([fsr.content(r[1]) for r in fsr.records(text)[0]], k, count=1)
    with native.Counter(k, NT) as ctx:
        load(ctx, own)
        (out, fix, _), info = check(ctx, text, own, 1)  # nothing is weak: the text comes back, no run kernel ran
        assert out == text and not fix.any() and info["s_track"] == info["s_try"] == 0 and info["s_patch"] > 0


def test_counts_around_two_to_the_32():
    k = 31
    rng = random.Random(32)
    seqs = [dna(rng, 4 * k) for _ in range(3)]
    big = (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)
    table = {}
    for r, s in enumerate(seqs):
        for j in range(len(s) - k + 1):
            table[s[j:j + k].decode()] = big[2] if r == 0 else big[1 + j % 2] if r == 1 else big[j % 3]
    bad0, bad1 = sub(seqs[0], (50,)), sub(seqs[1], (50,))
    for j in range(50 - k + 1, 51):
        table[bad0[j:j + k].decode()] = big[1]  # present, and weak below 2^32 + 1 only
    text = b"".join(b"@t%d\n%s\n+\n%s\n" % (i, s, qual_of(rng, len(s))) for i, s in enumerate([bad0, bad1, seqs[2]]))
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (out, fix, _), info = check(ctx, text, table, 2 ** 32 + 1, new_qual="#")
        assert fix[0].tolist() == [1, 1, 0, 0] and fsr.content(fsr.records(out)[0][0][1]) == seqs[0] and info["runs"] > 30
        (_, fix, _), info = check(ctx, text, table, 2 ** 32)
        assert fix[0].tolist() == [0, 0, 0, 0] and fix[1].tolist() == [1, 1, 0, 0]


# ----------------------------------------------------------------------------------------------- piece_bytes
def test_piece_bytes():
    k = 15
    genome, text = reads_text(k, seed=3)
    clean, shaped = shapes(k)
    text = shaped + b"\n" + text + b"\n\n"
    table = table_of([genome] + list(clean), k, count=2)
    want = cfr.expected(text, table, k, 2, ord("%"))
    keep = ("runs", "candidates", "fixed", "ambiguous", "unfixable", "bases", "lines", "patched", "records", "windows", "hits")
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        got = {}
        for piece_bytes in (1, 64, 4096, 0):
            (out, fix, rows), info = check(ctx, text, table, 2, "%", want=want, piece_bytes=piece_bytes)
            got[piece_bytes] = (out, fix.tolist(), rows.tolist(), {n: info[n] for n in keep})
            assert (info["pieces"] == 1) == (piece_bytes == 0)
        assert got[1] == got[64] == got[4096] == got[0] and got[0][3]["fixed"] > 40
        assert len(fsr.cuts(text, 4096)) > 2
        # the messages too: a malformed record, and a line the parser reads differently, in the last third of the text
        recs = fsr.records(text)[0]
        r = 2 * len(recs) // 3
        at = sum(len(x) for rec in recs[:r] for x in rec)
        seq_at = at + len(recs[r][0])
        for broken, code in ((text[:at] + b"#" + text[at + 1:], "at"), (text[:seq_at] + b">" + text[seq_at + 1:], "view")):
            with pytest.raises(cfr.CorrectFastqError) as w:
                cfr.expected(broken, table, k, 2)
            assert (w.value.record, w.value.kind) == (r, code)
            messages = set()
            for piece_bytes in (1, 64, 4096, 0):
                with pytest.raises(native.MercatHipError) as e:
                    ctx.correct_fastq(broken, 2, piece_bytes=piece_bytes)
                assert e.value.code == UNSUPPORTED and ("record %d" % r) in str(e.value)
                messages.add(str(e.value))
            assert len(messages) == 1


# ----------------------------------------------------------------------------------------------- device call
def test_device_call():
    import torch
    k = 15
    genome, text = reads_text(k, seed=4)
    table = table_of([genome], k, count=2)
    w_out, w_fix = cfr.expected(text, table, k, 2, ord("!"))
    n, nr = len(text), len(w_fix)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        w_rows = ctx.screen(cfr.view(text), 2).tolist()
        for off in (0, 1, 15):
            d_text = torch.from_numpy(np.frombuffer(b"#" * off + text, dtype=np.uint8).copy()).cuda()
            d_out = torch.full((off + n + 40,), 0xA5, dtype=torch.uint8, device="cuda")
            d_fix = torch.full((nr + 1, 4), -1, dtype=torch.int32, device="cuda")
            d_rows = torch.full((nr + 1, 5), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            info = ctx.correct_fastq_device(d_text.data_ptr() + off, n, d_out.data_ptr() + off, n, d_fix.data_ptr(), d_rows.data_ptr(),
                                            nr, at_least=2, new_qual="!")
            got = d_out.cpu().numpy()
            assert info["bytes_out"] == n and info["records"] == nr and info["patched"] == sum(r[1] for r in w_fix) > 40
            assert got[off:off + n].tobytes() == w_out and (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all()
            assert d_text.cpu().numpy()[off:].tobytes() == text  # (out of place: the input stays)
            assert [tuple(r) for r in d_fix.cpu().numpy().view(np.uint32)[:nr].tolist()] == w_fix and (d_fix[nr] == -1).all().item()
            assert d_rows.cpu().numpy().view(np.uint64)[:nr].tolist() == w_rows and (d_rows[nr] == -1).all().item()
            # in place
            info = ctx.correct_fastq_device(d_text.data_ptr() + off, n, d_text.data_ptr() + off, n, at_least=2, new_qual="!")
            got = d_text.cpu().numpy()
            assert got[off:].tobytes() == w_out and (got[:off] == ord("#")).all() and info["fixed"] == info["patched"]
        d_text = torch.from_numpy(np.frombuffer(text + b"#" * 64, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        for shift in (1, 16, n - 1):  # a partial overlap, either way round
            for a, b in ((0, shift), (shift, 0)):
                if max(a, b) + n > n + 64:
                    continue
                with pytest.raises(native.MercatHipError) as e:
                    ctx.correct_fastq_device(d_text.data_ptr() + a, n, d_text.data_ptr() + b, n)
                assert e.value.code == ARG and "overlap" in str(e.value)
        assert d_text.cpu().numpy()[:n].tobytes() == text
        with pytest.raises(native.MercatHipError) as e:  # room for one byte less
            ctx.correct_fastq_device(d_text.data_ptr(), n, d_text.data_ptr(), n - 1)
        assert e.value.code == RANGE
        with pytest.raises(native.MercatHipError) as e:
            ctx.correct_fastq_device(d_text.data_ptr(), n, d_text.data_ptr(), n, d_fix.data_ptr() + 4, 0, nr)
        assert e.value.code == ARG


# ------------------------------------------------------------------------------------------------- refusals
GUARD = 0xA5A5A5A5A5A5A5A5


def _raw(ctx, text: bytes, out_cap=None, cap=None, flags=0, rule=(2, 0, 0), null_out=False, null_rule=False, piece_bytes=0):
    """mk_correct_fastq_text into 0xA5-guarded buffers one element longer than the capacities it is told."""
    nrec = len(fsr.lines(text)) // 4
    out_cap = len(text) if out_cap is None else out_cap
    cap = nrec if cap is None else cap
    out = np.full(out_cap + 1, 0xA5, dtype=np.uint8)
    fx = np.full((cap + 1, 2), GUARD, dtype=np.uint64)
    rw = np.full((cap + 1, 5), GUARD, dtype=np.uint64)
    out_len, n, st = ctypes.c_size_t(7), ctypes.c_size_t(0), native.CorrectFastq()
    r = native.CorrectFastqRule(*rule)
    rc = native.lib().mk_correct_fastq_text(ctx._h, text, len(text), piece_bytes, flags, None if null_rule else ctypes.byref(r),
                                            None if null_out else out.ctypes.data, out_cap, ctypes.byref(out_len), fx.ctypes.data,
                                            rw.ctypes.data, cap, ctypes.byref(n), ctypes.byref(st))
    return {"rc": rc, "out_len": out_len.value, "nrows": n.value, "out": out, "fix": fx, "rows": rw, "st": st,
            "msg": (ctx._L.mk_last_error(ctx._h) or b"").decode()}


def refused(ctx, text, code, word=None, **kw):
    for piece_bytes in (0, 64):
        got = _raw(ctx, text, piece_bytes=piece_bytes, **kw)
        assert got["rc"] == code and got["out_len"] == 0 and (got["out"] == 0xA5).all(), (got["rc"], got["msg"])
        assert word is None or word in got["msg"], got["msg"]


def test_refusals():
    k = 15
    genome, text = reads_text(k, 30, seed=5)
    table = table_of([genome], k, count=2)
    recs = fsr.records(text)[0]
    offs = [sum(len(x) for rec in recs[:r] for x in rec) for r in range(len(recs))]
    put = lambda at, b: text[:at] + b + text[at + len(b):]
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        for r in (0, len(recs) // 2, len(recs) - 1):
            head, seq, plus, qual = recs[r]
            a_seq, a_plus, a_qual = offs[r] + len(head), offs[r] + len(head) + len(seq), offs[r] + len(head) + len(seq) + len(plus)
            cases = {"at": put(offs[r], b"#"), "plus": put(a_plus, b"-"),
                     "length": text[:a_qual] + text[a_qual + 1:],
                     "blank": put(a_seq + 3, b" "), "star": put(a_seq + len(seq) - 2, b"*"), "view": put(a_seq, b">")}
            for kind, broken in cases.items():
                with pytest.raises(cfr.CorrectFastqError) as w:
                    cfr.expected(broken, table, k, 2)
                assert w.value.code == UNSUPPORTED and w.value.record == r
                word = fsr.PHRASE.get(w.value.kind, "parser")
                refused(ctx, broken, UNSUPPORTED, word)
                refused(ctx, broken, UNSUPPORTED, "record %d" % r)
        refused(ctx, text + b"@x\nACGT\n", UNSUPPORTED, "the text ends inside it")
        refused(ctx, put(offs[7] + len(recs[7][0]) + 5, b"\xc3"), NON_ASCII, "0x80")
        refused(ctx, text, ARG, "at_least", rule=(0, 0, 0))
        refused(ctx, text, ARG, "reserved", rule=(2, 0, 1))
        refused(ctx, text, ARG, "new_qual", rule=(2, 32, 0))
        refused(ctx, text, ARG, "flag", flags=2)
        refused(ctx, text, ARG, "rule", null_rule=True)
        with pytest.raises(native.MercatHipError) as e:  # a plain table, folding asked for: refused as screen refuses it
            ctx.correct_fastq(text, fold=True)
        assert e.value.code == ARG
        assert ctx._L.mk_chunk_begin(ctx._h) == 0
        refused(ctx, text, STATE, "chunk")
        assert ctx._L.mk_chunk_end(ctx._h, 1) == 0
        # capacities: the output's length is known before any work; cap one short is told the record count
        got = _raw(ctx, text, out_cap=len(text) - 1)
        assert (got["rc"], got["out_len"]) == (RANGE, len(text)) and (got["out"] == 0xA5).all() and (got["fix"] == GUARD).all()
        got = _raw(ctx, text, out_cap=0, null_out=True)
        assert (got["rc"], got["out_len"]) == (RANGE, len(text))
        got = _raw(ctx, text, cap=len(recs) - 1)
        assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, len(text), len(recs)) and (got["out"] == 0xA5).all()
        assert (got["fix"][len(recs) - 1] == GUARD).all() and (got["rows"][len(recs) - 1] == GUARD).all()
        got = _raw(ctx, text)
        w_out, w_fix = cfr.expected(text, table, k, 2)
        assert (got["rc"], got["out_len"], got["nrows"]) == (0, len(text), len(recs)) and got["out"][:-1].tobytes() == w_out
        assert got["out"][-1] == 0xA5 and (got["fix"][-1] == GUARD).all() and (got["rows"][-1] == GUARD).all()
        assert [tuple(r) for r in got["fix"][:-1].view(np.uint32).reshape(-1, 4).tolist()] == w_fix
        assert ctx.correct_fastq(b"")[0] == b"" and ctx.correct_fastq(b"\n\n")[0] == b"\n\n"
    for alphabet, kk in ((AA, 5), (NT, 65)):  # a protein context; nucleotide keys kept as text
        with native.Counter(kk, alphabet) as ctx:
            refused(ctx, text, ARG, "nucleotide")


# ---------------------------------------------------------------------------------------- nothing else moves
def test_nothing_else_moves():
    k = 15
    genome, text = reads_text(k, 60, seed=6)
    with native.Counter(k, NT) as ctx:
        ctx.set_fastq(True)
        ctx.count_chunk(text * 2, 1)  # (FASTQ mode: the context's own conversion figures are not zero)
        stats, table, size = ctx.fastq_stats(), ctx.to_dict(), ctx.rows()
        assert stats["lines"] == 2 * len(fsr.lines(text)) and size > 0
        (out, _, _), info = check(ctx, text, table, 3)
        assert info["runs"] > 0
        (out, _, _), info = check(ctx, text, table, 2)  # (every window is there twice)
        assert out == text
        assert ctx.fastq_stats() == stats and ctx.to_dict() == table and ctx.rows() == size
        with pytest.raises(native.MercatHipError):
            ctx.correct_fastq(text[1:], 2)
        assert ctx.fastq_stats() == stats and ctx.to_dict() == table and ctx.rows() == size


# ------------------------------------------------------------------------------------------------ end to end
def test_against_the_fasta_call_and_the_front_ends(tmp_path):
    k = 15
    genome, fq = reads_text(k, 120, seed=7)
    _, fq2 = reads_text(k, 120, seed=8)
    table = table_of([genome], k, count=3)
    fa = native.fq2fa(fq)[0]
    for name, data in (("r.fastq", fq), ("r.fq.gz", gzip.compress(fq)), ("m.fastq", fq2)):
        (tmp_path / name).write_bytes(data)
    w_out, w_fix = cfr.expected(fq, table, k, 2)
    w_out2, w_fix2 = cfr.expected(w_out, table, k, 2)
    assert sum(r[1] for r in w_fix) > 40
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        out, fix, rows = ctx.correct_fastq(fq, 2)
        a_out, a_fix, a_rows = ctx.correct(fa, 2)
        assert native.fq2fa(out)[0] == a_out and fix.tolist() == a_fix.tolist() and rows.tolist() == a_rows.tolist()
        for name in ("r.fastq", "r.fq.gz"):
            res = kmers.correct_reads_fastq(ctx, tmp_path / name, tmp_path / "o.fastq", 2, tsv_path=tmp_path / "o.tsv")
            ref = kmers.correct_reads(ctx, tmp_path / name, tmp_path / "o.fna", 2, tsv_path=tmp_path / "o_fa.tsv")
            assert (tmp_path / "o.fastq").read_bytes() == w_out and (tmp_path / "o.tsv").read_bytes() == (tmp_path / "o_fa.tsv").read_bytes()
            assert set(res) == set(ref) and {n: res[n] for n in res if n != "bytes_out"} == {n: ref[n] for n in ref if n != "bytes_out"}
            assert res["bytes_out"] == len(fq) and res["fixed"] == sum(r[1] for r in w_fix)
        res = kmers.correct_reads_fastq(ctx, tmp_path / "r.fastq", tmp_path / "o2.fastq.gz", 2, rounds=2, new_qual="!")
        assert gzip.decompress((tmp_path / "o2.fastq.gz").read_bytes()) == cfr.expected(cfr.expected(fq, table, k, 2, 33)[0], table, k, 2, 33)[0]
        assert res["runs"] == sum(r[0] for r in w_fix) and res["fixed"] == sum(r[1] for r in w_fix) + sum(r[1] for r in w_fix2)
        both = fsr.interleave(fq, fq2)
        p_out, p_fix = cfr.expected(both, table, k, 2)
        res = kmers.correct_reads_fastq(ctx, tmp_path / "r.fastq", tmp_path / "p_1.fastq", 2, tsv_path=tmp_path / "p.tsv",
                                        mate_file=tmp_path / "m.fastq", out_path2=tmp_path / "p_2.fastq")
        first, second = fsr.split(p_out)
        assert (tmp_path / "p_1.fastq").read_bytes() == first == w_out and (tmp_path / "p_2.fastq").read_bytes() == second
        assert res["records"] == 240 and res["fixed"] == sum(r[1] for r in p_fix)
        assert (tmp_path / "p.tsv").read_bytes().count(b"\n") == 241


def test_cli_correct_fastq(tmp_path):
    k = 9
    rng = random.Random(3)
    sample = b"".join(b">a%d\n%s\n" % (i, dna(rng, 80)) for i in range(6))
    (tmp_path / "one.fna").write_bytes(sample * 2)  # (every k-mer twice: the default -correct_min 2 finds them solid)
    src = [s for _, s in trim_rule.records(sample)]
    reads = [sub(src[1][5:65], (30,)), sub(src[4][:50], (0,)), dna(rng, 40), b"ACG", src[0][:40]]
    mates = [sub(src[2][:60], (59,)), src[3][:50], dna(rng, 30), b"AC", sub(src[3][:40], (20,))]
    fq = lambda seqs, tag: b"".join(b"@%s%d x\n%s\n+\n%s\n" % (tag, i, s, qual_of(rng, len(s))) for i, s in enumerate(seqs))
    r_text, m_text = fq(reads, b"r"), fq(mates, b"m")
    (tmp_path / "reads.fastq").write_bytes(r_text)
    (tmp_path / "reads.fq.gz").write_bytes(gzip.compress(r_text))
    (tmp_path / "mates.fastq").write_bytes(m_text)
    table = cpu_ref.count_text(sample * 2, k, 1)
    argv = ["-i", str(tmp_path / "one.fna"), "-k", str(k), "-c", "1", "-skipclean"]
    for name, extra, q in (("reads.fastq", [], 0), ("reads.fq.gz", ["-correct_qual", "#"], ord("#"))):
        out = tmp_path / ("out_" + name.split(".")[1] + str(q))
        assert cli.main(argv + ["-o", str(out), "-correct", str(tmp_path / name), "-correct_fastq"] + extra) == 0
        w_out, w_fix = cfr.expected(r_text, table, k, 2, q)
        assert w_fix[0] == (1, 1, 0, 0) and w_out != r_text
        assert (out / "correct_nucleotide" / "one_corrected.fastq").read_bytes() == w_out
        want = b"record\tlength\truns\tfixed\tambiguous\tunfixable\n" + b"".join(
            b"r%d\t%d\t%d\t%d\t%d\t%d\n" % ((i, len(s)) + r) for i, (s, r) in enumerate(zip(reads, w_fix)))
        assert (out / "correct_nucleotide" / "one_correct.tsv").read_bytes() == want
        assert sorted(p.name for p in (out / "correct_nucleotide").iterdir()) == ["one_correct.tsv", "one_corrected.fastq"]
    out = tmp_path / "paired"
    assert cli.main(argv + ["-o", str(out), "-correct", str(tmp_path / "reads.fastq"), "-correct_mate", str(tmp_path / "mates.fastq"),
                            "-correct_fastq", "-correct_rounds", "2", "-correct_qual", "!"]) == 0
    want = [cfr.expected(cfr.expected(t, table, k, 2, 33)[0], table, k, 2, 33)[0] for t in (r_text, m_text)]
    assert [(out / "correct_nucleotide" / ("one_corrected_%d.fastq" % i)).read_bytes() for i in (1, 2)] == want
    assert (out / "correct_nucleotide" / "one_correct.tsv").read_bytes().count(b"\n") == 11
