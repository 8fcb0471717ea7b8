"""Isolated substitutions corrected against a table on the GPU (mk_correct_text / mk_correct_device, Counter.correct*,
kmers.correct_reads, report.write_correct_tsv, -correct).  Expected values never come from the code under test: the rule
is tests/correct_rule.py (plain Python over tests/trim_rule.py's records), the table is a dict -- the windows of the
records as they were before a base was substituted, loaded with Counter.load_tsv, or the CPU oracle's count of a source
text.  Equality is exact everywhere."""
import ctypes
import functools
import gzip
import random
import zlib

import numpy as np
import pytest

import correct_rule
import trim_rule
import walk_seams
from mercat2_amd import cli, kmers, native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE, RANGE = -1, -4, -7
COMP = bytes.maketrans(b"ACGT", b"TGCA")
SPACES = set(b" \t\x0b\x0c")
NEXT = bytes.maketrans(b"ACGT", b"CGTA")


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def wrap(seq, width):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


def sub(seq: str, at) -> str:
    """``seq`` with the next base of ACGT at every position of ``at`` that it has (negative: from the end)."""
    out = bytearray(seq.encode())
    for p in at:
        if -len(out) <= p < len(out):
            out[p] = bytes([out[p]]).translate(NEXT)[0]
    return out.decode()


def table_of(text: bytes, k: int, fold: bool = False, count=None) -> dict:
    """Every window of the text's records with the number of times it stands there (or ``count``), under its canonical
    form with ``fold``.  A window that holds a blank is left out (no table line can carry it): it is absent."""
    table = {}
    for _, seq in trim_rule.records(text):
        for j in range(len(seq) - k + 1):
            w = seq[j:j + k]
            if SPACES & set(w):
                continue
            if fold and set(w) <= set(b"ACGT"):
                w = min(w, w.translate(COMP)[::-1])
            table[w.decode()] = count if count is not None else table.get(w.decode(), 0) + 1
    return table


def load(ctx, table: dict):
    assert ctx.load_tsv(b"".join(b"%s\t%d\n" % (key.encode(), c) for key, c in table.items()))["rows"] == len(table)


def check(ctx, text: bytes, table: dict, at_least: int = 2, want=None, **kw):
    """Counter.correct against the rule: bytes, fix, rows (those of Counter.screen) and the figures."""
    info = {}
    out, fix, rows = ctx.correct(text, at_least, info=info, **kw)
    w_out, w_fix = want if want is not None else correct_rule.expected(text, table, ctx.k, at_least, ctx.canonical)
    lengths = [len(seq) for _, seq in trim_rule.records(text)]
    assert fix.dtype == np.uint32 and fix.shape == (len(w_fix), 4) and [tuple(r) for r in fix.tolist()] == w_fix
    assert out == w_out
    assert rows.tolist() == ctx.screen(text, at_least, **kw).tolist()
    assert [int(w) for w in rows[:, 0]] == [max(0, n - ctx.k + 1) for n in lengths]
    assert info["records"] == len(w_fix) and info["bytes"] == len(text) and info["bytes_out"] == len(w_out) <= len(text) + 1
    assert [info[c] for c in native.CORRECT_COLUMNS] == [sum(r[i] for r in w_fix) for i in range(4)]
    assert info["candidates"] == info["fixed"] + info["ambiguous"] + info["unfixable"] and info["bases"] == sum(lengths)
    return (out, fix, rows), info


# --------------------------------------------------------------------------------------------- record shapes
@functools.lru_cache(maxsize=None)
def shapes(k: int, headless: bool, blanks: bool = True):
    """(text as it was, text with substitutions): every record shape in both, a base substituted at 0, k - 1, k, L - k,
    L - 1 or in the middle of the records that have room; ends in a record without a newline."""
    rng = random.Random(1000 * k + headless)
    clean, bad = [], []

    def add(layout, n, at=()):
        seq = dna(rng, n)
        clean.append(layout(seq))
        bad.append(layout(sub(seq, at)))

    line = lambda head: (lambda s: head + s + "\n")
    if headless:
        add(line(""), 2 * k + 2, (k,))
    else:
        clean.append("  \n\t\n \x0b\n")
        bad.append(clean[-1])
    add(line(">km1 a b\n"), k - 1, (0,))
    add(line(">k\n"), k, (0,))
    add(line("  >kp1\tx\n"), k + 1, (0,))
    add(line(" \t>kp1 end\n"), k + 1, (-1,))
    add(lambda s: ">h1\n", 0)
    add(line(">h2\n"), 2 * k + 3, (k - 1,))
    add(line(">\n"), 2 * k + 1, (k,))
    add(lambda s: ">wrapped\n" + wrap(s, 7), 4 * k + 5, (0, 2 * k, -1))
    add(lambda s: ">crlf x\r\n" + s[:5] + "\r\n" + s[5:] + "\r\n", 3 * k + 4, (-k,))
    add(lambda s: ">cr\r" + s[:k + 2] + "\r" + s[k + 2:] + "\r", 2 * k + 5, (k + 1,))
    add(lambda s: ">star\n" + s[:3] + "*" + s[3:] + "**\n*\n", 2 * k + 6, (3,))
    if blanks:
        add(lambda s: ">blank\n  " + s[:2 * k + 1] + " \t" + s[2 * k + 1:] + "  \n", 3 * k + 6, (1,))  # (the windows over the blanks are absent)
    for i, at in enumerate(((0,), (k - 1,), (k,), (-k,), (-1,), (), (k + 2, 2 * k + 1), (k + 2, 2 * k + 2), (k + 2, 2 * k + 3), (0, -1))):
        add(line(">p%d\n" % i), 4 * k + 9, at)
    add(lambda s: ">empty line\n\n" + s + "\n\n", 2 * k + 2, (k - 1,))
    add(lambda s: ">hdr only\n", 0)
    add(lambda s: ">last one\n" + s, 2 * k + 4, (-1,))
    return "".join(clean).encode(), "".join(bad).encode()


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("k", [5, 31, 32, 33, 63])
def test_record_shapes(k, fold):
    for headless in (False, True):
        clean, bad = shapes(k, headless)
        table = table_of(clean, k, fold)
        with native.Counter(k, NT, canonical=fold) as ctx:
            load(ctx, table)
            (out, fix, rows), info = check(ctx, bad, table, 1)
            assert info["headless"] == (1 if headless else 0) and info["pieces"] == 1 and (info["folded"] > 0) == fold
            assert info["preamble"] == (0 if headless else len("  \n\t\n \x0b\n"))
            assert b"  >kp1\tx\n" in out and b">crlf x\r\n" in out and b">cr\r" in out and b">h1\n>h2\n" in out
            assert out.endswith(b"\n") and not bad.endswith(b"\n") and b">hdr only\n>last one\n" in out
            names = [h.split()[0] if h.split() else b"" for h, _ in trim_rule.records(bad)]
            assert fix[names.index(b">km1")].tolist() == [0] * 4
            if k > 5:  # (no window of these texts is there twice by chance: every isolated substitution comes back)
                fixed = trim_rule.records(out)
                for r, (_, seq) in enumerate(trim_rule.records(clean)):
                    if names[r].startswith((b">p6", b">p7")):  # two substitutions k - 1 and k apart: one run, too long
                        assert fix[r].tolist() == [1, 0, 0, 0] and fixed[r][1] != seq
                    elif names[r] not in (b">k", b">km1", b">blank"):
                        assert fixed[r][1] == seq, names[r]
                assert fix[names.index(b">k")].tolist() == [1, 0, 0, 0] and fix[names.index(b">p8")].tolist() == [2, 2, 0, 0]
                assert info["fixed"] >= 20
            else:
                assert info["runs"] > info["candidates"] > 0
            check(ctx, bad, table, 2)
            check(ctx, out, table, 1)  # a second pass: the rule again, on what the first one wrote


# ----------------------------------------------------------------------------------------------------- seams
@functools.lru_cache(maxsize=None)
def seam_texts(k: int):
    """walk_seams' records as they are, and with a base substituted at 0, k - 1, the middle and L - 1 of every record that
    has room (the first two make one run that nothing repairs), at one place in a shorter record, in the long record every
    997 characters."""
    clean, bad = [], []
    for i, (name, seq) in enumerate(walk_seams.seam_records(k)):
        n = len(seq)
        at = range(5, n, 997) if name == "long" else (0, k - 1, n // 2, n - 1) if n >= 3 * k + 3 else (i % max(1, n),)
        clean.append(">%s\n%s" % (name, wrap(seq, 70)))
        bad.append(">%s\n%s" % (name, wrap(sub(seq, at), 70)))
    return "".join(clean).encode(), "".join(bad).encode()


@pytest.mark.parametrize("k", [5, 31])
def test_seams(k):
    import torch
    clean, bad = seam_texts(k)
    assert clean == walk_seams.seam_text(k) and len(bad) == len(clean)
    table = table_of(clean, k)
    at_least = 1 if k > 5 else sorted(table.values())[len(table) // 3]  # (every 5-mer is there: a third of them weak)
    want = correct_rule.expected(bad, table, k, at_least)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        one, info = check(ctx, bad, table, at_least, want=want)
        many, info_p = check(ctx, bad, table, at_least, want=want, piece_bytes=len(bad) // 12)
        assert info["pieces"] == 1 and info_p["pieces"] > 8
        assert {c: info[c] for c in ("runs", "candidates", "fixed", "ambiguous", "unfixable")} == \
            {c: info_p[c] for c in ("runs", "candidates", "fixed", "ambiguous", "unfixable")}
        assert info["fixed"] > (300 if k > 5 else 0) and info["runs"] > info["candidates"] > 300
        w_out, w_fix = want
        no, nr = len(w_out), len(w_fix)
        d_text = torch.from_numpy(np.frombuffer(b"###" + bad, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((1 + no + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_fix = torch.full((nr + 1, 4), -1, dtype=torch.int32, device="cuda")
        d_rows = torch.full((nr + 1, 5), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        dinfo = ctx.correct_device(d_text.data_ptr() + 3, len(bad), d_out.data_ptr() + 1, no, d_fix.data_ptr(), d_rows.data_ptr(), nr,
                                   at_least=at_least)
        got = d_out.cpu().numpy()
        assert dinfo["bytes_out"] == no and dinfo["records"] == nr and dinfo["pieces"] == 1 and dinfo["fixed"] == info["fixed"]
        assert got[1:1 + no].tobytes() == w_out and got[0] == 0xA5 and (got[1 + no:] == 0xA5).all()
        assert [tuple(r) for r in d_fix.cpu().numpy().view(np.uint32)[:nr].tolist()] == w_fix and (d_fix[nr] == -1).all().item()
        assert d_rows.cpu().numpy().view(np.uint64)[:nr].tolist() == one[2].tolist() and (d_rows[nr] == -1).all().item()
        with pytest.raises(native.MercatHipError) as e:
            ctx.correct_device(d_text.data_ptr() + 3, len(bad), d_out.data_ptr() + 1, no - 1, at_least=at_least)
        assert e.value.code == RANGE
        with pytest.raises(native.MercatHipError) as e:
            ctx.correct_device(d_text.data_ptr() + 3, len(bad), d_out.data_ptr(), no, d_fix.data_ptr() + 4, 0, nr, at_least=at_least)
        assert e.value.code == ARG


# ------------------------------------------------------------------------------ bytes outside the alphabet
@pytest.mark.parametrize("k", [31, 33])
def test_bytes_outside_the_alphabet(k):
    rng = random.Random(9 * k)
    L = 4 * k
    seqs = [dna(rng, L) for _ in range(6)]
    with_n = seqs[1][:2 * k + 3] + "N" + seqs[1][2 * k + 4:]  # the source itself holds an N: its windows are text keys
    lower = seqs[4][:10] + seqs[4][10:14].lower() + seqs[4][14:]
    clean = "".join(">s%d\n%s\n" % (i, s) for i, s in enumerate([seqs[0], with_n, seqs[2], seqs[3], lower, seqs[5]])).encode()
    at = 2 * k
    bad = [seqs[0][:at] + "N" + seqs[0][at + 1:],                      # an N at p: four alternatives
           sub(with_n, (at,)),                                        # an N elsewhere inside the run: text probes
           seqs[2][:at] + "n" + seqs[2][at + 1:],                      # a lower-case letter at p
           sub(seqs[3], (at,))[:at + 5] + "N" + seqs[3][at + 6:],      # a substitution and an N five on: one run, too long
           sub(lower, (16,)),                                         # a base behind lower-case letters: p = 16, text probes
           sub(seqs[5], (0,))[:1] + "N" + seqs[5][2:]]                 # the N at 1 is p, but position 0 is wrong too
    text = "".join(">b%d\n%s\n" % (i, s) for i, s in enumerate(bad)).encode()
    table = table_of(clean, k)
    assert any("N" in key for key in table) and any(key != key.upper() for key in table)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (out, fix, _), info = check(ctx, text, table, 1)
        got = [seq.decode() for _, seq in trim_rule.records(out)]
        assert got[0] == seqs[0] and got[1] == with_n and got[2] == seqs[2] and got[4] == lower
        assert fix[:3].tolist() == [[1, 1, 0, 0]] * 3 and fix[3].tolist() == [1, 0, 0, 0] and fix[4].tolist() == [1, 1, 0, 0]
        assert got[5] == bad[5] and fix[5].tolist() == [1, 0, 0, 1] and info["text_windows"] > 0


# ------------------------------------------------------------------------------------------------ thresholds
@functools.lru_cache(maxsize=None)
def mixed_text(k: int):
    """(clean, bad): the record shapes without blanks, 300 reads of a small genome with a substitution or two in most of
    them, and a wrapped contig with a few."""
    rng = random.Random(5 * k)
    head_clean, head_bad = shapes(k, True, blanks=False)
    genome = dna(rng, 3_000)
    clean, bad = [head_clean.decode() + "\n"], [head_bad.decode() + "\n"]
    for i in range(300):
        s = genome[(i * 37) % 2850:][:150]
        clean.append(">m%d\n%s\n" % (i, s))
        bad.append(">m%d\n%s\n" % (i, sub(s, [(i * 13) % 150, (i * 29) % 150][:i % 3])))
    contig = dna(rng, 9_000)
    clean.append(">contig\n" + wrap(contig, 60))
    bad.append(">contig\n" + wrap(sub(contig, (0, 700, 700 + k + 1, 4_000, 4_000 + k - 1, 8_999)), 60))
    return "".join(clean).encode(), "".join(bad).encode()


def test_thresholds():
    k = 31
    clean, bad = mixed_text(k)
    own = table_of(bad, k, count=1)
    with native.Counter(k, NT) as ctx:
        load(ctx, own)
        # at_least 1 against the text's own windows: nothing is weak, every record comes back on one line
        (out, fix, _), info = check(ctx, bad, own, 1)
        assert out == b"".join(h + (s + b"\n" if s else b"") for h, s in trim_rule.records(bad)) and not fix.any()
        assert info["runs"] == info["candidates"] == 0 and info["s_track"] == info["s_runs"] == info["s_try"] == 0
        one_line = b"".join(b">r%d\n%s\n" % (i, s) for i, (_, s) in enumerate(trim_rule.records(bad)) if s)
        assert ctx.correct(one_line, 1)[0] == one_line
    # counts 0 .. 6 by a hash of the window: runs of every length, at 2 and at 5
    hashed = {key: zlib.crc32(key.encode()) % 7 for key in table_of(clean, k)}
    hashed = {key: c for key, c in hashed.items() if c}
    with native.Counter(k, NT) as ctx:
        load(ctx, hashed)
        for at_least in (2, 5):
            _, info = check(ctx, bad, hashed, at_least)
            assert info["runs"] > 1000 and info["candidates"] > 100 and info["s_try"] > 0
    # the clean windows three times each: the substitutions come back
    solid = table_of(clean, k, count=3)
    with native.Counter(k, NT) as ctx:
        load(ctx, solid)
        for at_least in (2, 3):
            _, info = check(ctx, bad, solid, at_least)
            assert info["fixed"] > 150 and info["fixed"] + info["ambiguous"] + info["unfixable"] < info["runs"]
        _, info = check(ctx, bad, solid, 4)  # nothing is solid: every run is a whole record
        assert info["candidates"] == 0 and info["runs"] > 300


def test_counts_around_two_to_the_32():
    k = 31
    rng = random.Random(32)
    seqs = [dna(rng, 4 * k) for _ in range(4)]
    big = (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)
    table = {}
    for r, s in enumerate(seqs):
        for j in range(len(s) - k + 1):
            # record 0: solid; record 1: every third window weak; record 2: k windows weak in the middle, the rest solid;
            # record 3: solid, and below, what repairs its substitution is one short of solid
            c = big[1 + j % 2] if r in (0, 3) else big[j % 3] if r == 1 else big[0] if 40 <= j < 40 + k else big[2]
            table[s[j:j + k]] = c
    bad0, bad3 = sub(seqs[0], (50,)), sub(seqs[3], (50,))
    for j in range(50 - k + 1, 51):
        table[bad0[j:j + k]] = big[0]  # present, and weak
        table[seqs[3][j:j + k]] = big[0]
    text = "".join(">t%d\n%s\n" % (i, s) for i, s in enumerate([bad0, seqs[1], seqs[2], bad3])).encode()
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        (out, fix, rows), info = check(ctx, text, table, 2 ** 32)
        # (record 1: 32 runs of one window; the first and the last have a candidate, which no base repairs)
        assert fix.tolist() == [[1, 1, 0, 0], [(3 * k + 1 + 2) // 3, 0, 0, 2], [1, 0, 0, 1], [1, 0, 0, 1]]
        assert trim_rule.records(out)[0][1].decode() == seqs[0] and int(rows[1, 1]) == (4 * k - k + 1) - fix[1, 0]
        _, info = check(ctx, text, table, 2 ** 32 - 1)  # all that is there is solid: the substitution in record 3 comes back
        assert info["runs"] == info["fixed"] == 1
        _, info = check(ctx, text, table, 2 ** 32 + 1)
        assert info["runs"] > 40


# ------------------------------------------------------------------------------------ capacity and arguments
GUARD = 0xA5A5A5A5A5A5A5A5


def _raw(ctx, text: bytes, out_cap: int, cap: int, flags: int = 0, rule=(2, 0), null_out: bool = False, null_rule: bool = False,
         piece_bytes: int = 0, fix: bool = True, rows: bool = True):
    """mk_correct_text into 0xA5-guarded buffers one element longer than the capacities it is told."""
    out = np.full(out_cap + 1, 0xA5, dtype=np.uint8)
    fx = np.full((cap + 1, 2), GUARD, dtype=np.uint64)
    rw = np.full((cap + 1, 5), GUARD, dtype=np.uint64)
    out_len, n, st = ctypes.c_size_t(0), ctypes.c_size_t(0), native.Correct()
    r = native.CorrectRule(*rule)
    rc = native.lib().mk_correct_text(ctx._h, text, len(text), piece_bytes, flags, None if null_rule else ctypes.byref(r),
                                      None if null_out else out.ctypes.data, out_cap, ctypes.byref(out_len),
                                      fx.ctypes.data if fix else None, rw.ctypes.data if rows else None, cap, ctypes.byref(n),
                                      ctypes.byref(st))
    return {"rc": rc, "out_len": out_len.value, "nrows": n.value, "out": out, "fix": fx, "rows": rw, "st": st}


def test_capacities():
    k = 31
    clean, bad = mixed_text(k)
    table = table_of(clean, k, count=3)
    w_out, w_fix = correct_rule.expected(bad, table, k, 2)
    no, nr = len(w_out), len(w_fix)
    as_rows = lambda fx: [tuple(r) for r in fx.view(np.uint32).reshape(-1, 4).tolist()]
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        w_rows = ctx.screen(bad, 2).tolist()
        for piece_bytes in (0, 4096):
            # exactly enough: everything written, the element past each capacity untouched
            got = _raw(ctx, bad, no, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (0, no, nr) and got["st"].bytes_out == no
            assert got["out"][:no].tobytes() == w_out and got["out"][no] == 0xA5
            assert as_rows(got["fix"][:nr]) == w_fix and (got["fix"][nr] == GUARD).all()
            assert got["rows"][:nr].tolist() == w_rows and (got["rows"][nr] == GUARD).all()
            # out_cap one short: the needed size, nothing past the cap
            got = _raw(ctx, bad, no - 1, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr) and got["out"][no - 1] == 0xA5
            assert "bytes" in ctx._L.mk_last_error(ctx._h).decode()
            # cap one short
            got = _raw(ctx, bad, no, nr - 1, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr)
            assert (got["rows"][nr - 1] == GUARD).all() and (got["fix"][nr - 1] == GUARD).all()
            # the sizing call
            got = _raw(ctx, bad, 0, 0, null_out=True, piece_bytes=piece_bytes)
            assert (got["rc"], got["out_len"], got["nrows"]) == (RANGE, no, nr)
            assert (got["rows"] == GUARD).all() and (got["fix"] == GUARD).all()
        # fix NULL, rows NULL, both NULL (cap is ignored)
        got = _raw(ctx, bad, no, nr, fix=False)
        assert got["rc"] == 0 and got["rows"][:nr].tolist() == w_rows and (got["fix"] == GUARD).all()
        got = _raw(ctx, bad, no, nr, rows=False)
        assert got["rc"] == 0 and as_rows(got["fix"][:nr]) == w_fix and (got["rows"] == GUARD).all()
        got = _raw(ctx, bad, no, 0, fix=False, rows=False)
        assert (got["rc"], got["out_len"], got["nrows"]) == (0, no, nr) and got["out"][:no].tobytes() == w_out
        got = _raw(ctx, b"", 0, 0)
        assert (got["rc"], got["out_len"], got["nrows"]) == (0, 0, 0)


def test_arguments_and_state():
    k = 31
    clean, bad = shapes(k, False)
    table = table_of(clean, k)
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        before, size = ctx.to_dict(), ctx.rows()
        check(ctx, bad, table, 1)
        assert ctx.rows() == size and ctx.to_dict() == before
        for kw, word in (({"rule": (0, 0)}, "at_least"), ({"rule": (2, 1)}, "reserved"), ({"flags": 2}, "flag"), ({"null_rule": True}, "rule")):
            got = _raw(ctx, bad, len(bad) + 1, 64, **kw)
            assert got["rc"] == ARG and word in ctx._L.mk_last_error(ctx._h).decode() and (got["out"] == 0xA5).all(), kw
        with pytest.raises(native.NonAsciiInput):
            ctx.correct(b">a\nACGT\xc3\xa9ACGT\n")
        with pytest.raises(native.MercatHipError) as e:  # a plain table, folding asked for: refused as screen refuses it
            ctx.correct(bad, fold=True)
        assert e.value.code == ARG
        assert ctx._L.mk_chunk_begin(ctx._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            ctx.correct(bad)
        assert e.value.code == STATE
        assert ctx._L.mk_chunk_end(ctx._h, 1) == 0
        assert ctx.to_dict() == before
        # an empty text; a text of only a preamble; header lines only
        out, fix, rows = ctx.correct(b"")
        assert (out, fix.shape, rows.shape) == (b"", (0, 4), (0, 5))
        info = {}
        out, fix, rows = ctx.correct(b"\n  \n", info=info)
        assert (out, fix.shape, rows.shape, info["preamble"], info["records"]) == (b"", (0, 4), (0, 5), 4, 0)
        out, fix, rows = ctx.correct(b">a\n>b x\r\n\n>c")
        assert (out, fix.tolist(), rows.tolist()) == (b">a\n>b x\r\n>c", [[0] * 4] * 3, [[0] * 5] * 3)
    for alphabet, kk in ((AA, 5), (RAW, 9), (NT, 70)):  # a protein context, a raw one, nucleotide keys kept as text
        with native.Counter(kk, alphabet) as ctx:
            with pytest.raises(native.MercatHipError) as e:
                ctx.correct(b">a\nACGTACGTACGTACGT\n")
            assert e.value.code == ARG and "nucleotide" in str(e.value)


# ------------------------------------------------------------------------------------------------ front ends
def fastq_text(seed: int, genome: str, n: int):
    """(FASTQ text, the FASTA fq2fa makes of it): reads of the genome, a substitution in two of three."""
    rng = random.Random(seed)
    fq, fa = [], []
    for i in range(n):
        at = rng.randrange(0, len(genome) - 90)
        seq = sub(genome[at:at + rng.randrange(40, 90)], [rng.randrange(0, 40)][:i % 3])
        qual = (">" if i % 3 == 0 else "@" if i % 3 == 1 else "I") + "".join(rng.choice("!#>@FI+") for _ in range(len(seq) - 1))
        fq.append("@read%d len=%d\n%s\n+%s\n%s\n" % (i, len(seq), seq, "read%d" % i if i % 2 else "", qual))
        fa.append(">read%d len=%d\n%s\n" % (i, len(seq), seq))
    return "".join(fq).encode(), "".join(fa).encode()


def test_correct_reads(tmp_path):
    k = 15
    genome = dna(random.Random(15), 2_000)
    table = table_of((">g\n" + genome + "\n").encode(), k, count=3)
    fq, fa = fastq_text(11, genome, 120)
    fq2, fa2 = fastq_text(12, genome, 120)
    for name, data in (("r.fna", fa), ("r.fna.gz", gzip.compress(fa)), ("r.fastq", fq), ("r.fq.gz", gzip.compress(fq)), ("m.fastq", fq2)):
        (tmp_path / name).write_bytes(data)
    lengths = [len(seq) for _, seq in trim_rule.records(fa)]
    w_out, w_fix = correct_rule.expected(fa, table, k, 2)
    w_out2, w_fix2 = correct_rule.expected(w_out, table, k, 2)
    assert sum(r[1] for r in w_fix) > 40 and w_out != fa
    with native.Counter(k, NT) as ctx:
        load(ctx, table)
        for name in ("r.fna", "r.fna.gz", "r.fastq", "r.fq.gz"):
            for dest in ("o.fna", "o.fna.gz"):
                res = kmers.correct_reads(ctx, tmp_path / name, tmp_path / dest, 2, tsv_path=tmp_path / "o.tsv")
                data = (tmp_path / dest).read_bytes()
                if dest.endswith(".gz"):
                    assert data[:2] == b"\x1f\x8b"
                    data = gzip.decompress(data)
                assert data == w_out, (name, dest)
                assert res == {"records": len(w_fix), "runs": sum(r[0] for r in w_fix), "fixed": sum(r[1] for r in w_fix),
                               "ambiguous": sum(r[2] for r in w_fix), "unfixable": sum(r[3] for r in w_fix),
                               "bases": sum(lengths), "bytes_out": len(w_out)}
                want = b"record\tlength\truns\tfixed\tambiguous\tunfixable\n" + b"".join(
                    b"read%d\t%d\t%d\t%d\t%d\t%d\n" % ((i, n) + r) for i, (n, r) in enumerate(zip(lengths, w_fix)))
                assert (tmp_path / "o.tsv").read_bytes() == want
        # two rounds are two calls: the runs of the first, the outcomes of both
        res = kmers.correct_reads(ctx, tmp_path / "r.fastq", tmp_path / "o2.fna", 2, rounds=2)
        assert (tmp_path / "o2.fna").read_bytes() == w_out2
        assert res["runs"] == sum(r[0] for r in w_fix) and res["fixed"] == sum(r[1] for r in w_fix) + sum(r[1] for r in w_fix2)
        assert res["unfixable"] == sum(r[3] for r in w_fix) + sum(r[3] for r in w_fix2)
        # mates: interleaved, corrected as one text, split again
        both = native.interleave(fa, fa2)
        assert [h for h, _ in trim_rule.records(both)][:3] == [b">read0 len=%d\n" % lengths[0], trim_rule.records(fa2)[0][0], b">read1 len=%d\n" % lengths[1]]
        p_out, p_fix = correct_rule.expected(both, table, k, 2)
        res = kmers.correct_reads(ctx, tmp_path / "r.fastq", tmp_path / "p_1.fna", 2, tsv_path=tmp_path / "p.tsv",
                                  mate_file=tmp_path / "m.fastq", out_path2=tmp_path / "p_2.fna")
        first, second = native.split_pairs(p_out)
        assert (tmp_path / "p_1.fna").read_bytes() == first == w_out and (tmp_path / "p_2.fna").read_bytes() == second
        assert second == correct_rule.expected(fa2, table, k, 2)[0]
        assert res["records"] == 240 and res["fixed"] == sum(r[1] for r in p_fix)
        assert (tmp_path / "p.tsv").read_bytes().count(b"\n") == 241


def test_cli_correct(tmp_path):
    k = 9
    rng = random.Random(3)
    samples = {"one": "".join(">a%d\n%s\n" % (i, dna(rng, 80)) for i in range(6)), "two": "".join(">b%d\n%s\n" % (i, dna(rng, 80)) for i in range(6))}
    for base, data in samples.items():
        (tmp_path / (base + ".fna")).write_text(data * 2)  # (every k-mer twice: the default -correct_min 2 finds them solid)
    one, two = (trim_rule.records(samples[b].encode()) for b in ("one", "two"))
    reads = (b">from one\n" + sub(one[1][1][5:65].decode(), (30,)).encode() + b"\n>from two\n" + sub(two[4][1][:50].decode(), (0,)).encode() +
             b"\n  >neither\n" + dna(rng, 40).encode() + b"\n>short\nACG\n>whole\n" + one[0][1][:40] + b"\n")
    mates = (b">m one\n" + sub(one[2][1][:60].decode(), (59,)).encode() + b"\n>m two\n" + two[3][1][:50] + b"\n>m3\n" + dna(rng, 30).encode() +
             b"\n>m4\nAC\n>m5\n" + sub(one[3][1][:40].decode(), (20,)).encode() + b"\n")
    (tmp_path / "reads.fa").write_bytes(reads)
    (tmp_path / "mates.fa").write_bytes(mates)
    names = ["from", "from", "neither", "short", "whole"]
    lengths = [60, 50, 40, 3, 40]
    argv = ["-i", str(tmp_path / "one.fna"), str(tmp_path / "two.fna"), "-k", str(k), "-c", "1", "-skipclean"]
    for extra, at_least in (([], 2), (["-correct_min", "3"], 3)):
        out = tmp_path / ("out%d" % at_least)
        assert cli.main(argv + ["-o", str(out), "-correct", str(tmp_path / "reads.fa")] + extra) == 0
        for base, data in samples.items():
            table = cpu_ref.count_text((data * 2).encode(), k, 1)
            w_out, w_fix = correct_rule.expected(reads, table, k, at_least)
            assert (out / "correct_nucleotide" / ("%s_corrected.fna" % base)).read_bytes() == w_out
            want = b"record\tlength\truns\tfixed\tambiguous\tunfixable\n" + b"".join(
                b"%s\t%d\t%d\t%d\t%d\t%d\n" % ((n.encode(), full) + r) for n, full, r in zip(names, lengths, w_fix))
            assert (out / "correct_nucleotide" / ("%s_correct.tsv" % base)).read_bytes() == want
            if at_least == 2:
                assert w_fix[0 if base == "one" else 1] == (1, 1, 0, 0) and w_fix[2] == (1, 0, 0, 0)
            else:
                assert not any(r[1] for r in w_fix)
        assert sorted(p.name for p in (out / "correct_nucleotide").iterdir()) == [
            "one_correct.tsv", "one_corrected.fna", "two_correct.tsv", "two_corrected.fna"]
        assert not (out / "correct_protein").exists()
    out = tmp_path / "paired"
    assert cli.main(argv + ["-o", str(out), "-correct", str(tmp_path / "reads.fa"), "-correct_mate", str(tmp_path / "mates.fa"),
                            "-correct_rounds", "2"]) == 0
    table = cpu_ref.count_text((samples["one"] * 2).encode(), k, 1)
    want = [correct_rule.expected(correct_rule.expected(t, table, k, 2)[0], table, k, 2)[0] for t in (reads, mates)]
    assert [(out / "correct_nucleotide" / ("one_corrected_%d.fna" % i)).read_bytes() for i in (1, 2)] == want
    assert (out / "correct_nucleotide" / "one_correct.tsv").read_bytes().count(b"\n") == 11
