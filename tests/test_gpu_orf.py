"""Open reading frames called on the GPU (mk_orf_text / mk_orf_device, Counter.orfs*, kmers.orf_reads,
report.write_orf_tsv, -orf).  Expected values never come from the code under test: the rule is tests/orf_rule.py (the
reference's line loop, a translated reverse-complemented copy and a sort, in plain Python).  Equality is exact
everywhere.  Sequences over G and C hold no stop and no start in any frame, so a stop or a start planted by hand is the
only one: that is how a closing is put on a chosen lane, wave or tile seam of the scan."""
import ctypes
import functools
import gzip
import random

import numpy as np
import pytest

import orf_rule as rule
from conftest import GOLDEN
from mercat2_amd import cli, kmers, native

pytestmark = pytest.mark.gpu
NT, AA = native.ALPHABET_NT2, native.ALPHABET_AA5
ARG, STATE, NON_ASCII, RANGE = -1, -4, -5, -7
SPAN = 256 * 48  # OR_SPAN of mk_orf.hip: the stream positions of one workgroup (tests/test_orf_host.py reads the source)
RUN = 48         # OR_RUN: ... of one lane
SEAMS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257] + list(range(SPAN - 3, SPAN + 4))
MODES = [dict(), dict(start=True), dict(start=True, alt_starts=True), dict(strand="plus"), dict(strand="minus"),
         dict(start=True, strand="minus"), dict(start=True, alt_starts=True, strand="plus")]


@pytest.fixture(scope="module")
def ctx():
    with native.Counter(5, NT) as c:
        yield c


def dna(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def gc(rng, n):
    return dna(rng, n, "GC")


def wrap(seq, width, eol="\n"):
    return "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def plant(seq: str, at: int, word: str) -> str:
    return seq[:at] + word + seq[at + len(word):]


def check(ctx, text: bytes, min_aa: int = 32, piece_bytes: int = 0, **mode):
    """Counter.orfs against the rule: bytes, rows and the figures."""
    info = {}
    out, rows = ctx.orfs(text, min_aa=min_aa, piece_bytes=piece_bytes, info=info, **mode)
    w_out, w_rows = rule.expected(text, min_aa, **mode)
    assert rows.dtype == np.uint64 and rows.shape == (len(w_rows), 4)
    assert rows.tolist() == w_rows
    assert out == w_out
    recs = rule.records(text)
    assert info["records"] == len(recs) and info["bytes"] == len(text) and info["bases"] == sum(len(s) for _, s in recs)
    assert info["orfs"] == len(w_rows) and info["bytes_out"] == len(w_out) and info["residues"] == sum(r[2] for r in w_rows)
    assert info["longest"] == max([r[2] for r in w_rows], default=0)
    assert info["per_frame"] == [sum(1 for r in w_rows if r[3] == f) for f in range(1, 7)]
    return out, rows, info


# ------------------------------------------------------------------------------------------ lengths and min_aa
@pytest.mark.parametrize("min_aa", [1, 32])
def test_lengths_and_min_aa(ctx, min_aa):
    rng = random.Random(7)
    lengths = list(range(9)) + [95, 96, 97]
    for letters in ("GC", "ACGT"):
        recs = [">r%d\n%s\n" % (n, dna(rng, n, letters)) for n in lengths]
        out, rows, _ = check(ctx, "".join(recs).encode(), min_aa)
        for r in recs:  # every record alone, too: the stream's end closes what a separator closed above
            check(ctx, r.encode(), min_aa)
        if letters == "GC" and min_aa == 32:  # 96 bases are 32 codons in one class of each strand, 97 in two
            assert [int(r[0]) for r in rows] == [10, 10, 11, 11, 11, 11]
        if letters == "GC" and min_aa == 1:
            assert [sum(1 for r in rows if r[0] == i) for i in range(6)] == [0, 0, 0, 2, 4, 6]


# ------------------------------------------------------------------------------------------ tile and wave seams
@functools.lru_cache(maxsize=None)
def long_gc():
    return gc(random.Random(11), 2 * SPAN + 5)  # an ORF crosses two tile boundaries: the carry is used twice


@pytest.mark.parametrize("headless", [False, True], ids=["headed", "headless"])
@pytest.mark.parametrize("word", ["TAA", "TTA"], ids=["forward", "reverse"])
def test_one_stop_at_every_seam(ctx, word, headless):
    """One stop in a record that has no other.  Headed: the record starts at stream position 1 (behind the separator);
    headless: at 0, so that the stop's record position is its stream position."""
    seq = long_gc()
    for at in SEAMS:
        text = ("" if headless else ">long one\n") + plant(seq, at, word) + "\n"
        out, rows, _ = check(ctx, text.encode(), 1)
        assert len(rows) >= 6  # (three classes a strand, and what the stop cuts in two)
    for at in (len(seq) - 3, len(seq) - 4, len(seq) - 5, 2 * SPAN - 1, 2 * SPAN):  # ... and at the record's other end
        check(ctx, ((">x\n" if not headless else "") + plant(seq, at, word)).encode(), 32)


@pytest.mark.parametrize("word,mode", [("ATG", dict(start=True)), ("CAT", dict(start=True)), ("GTG", dict(start=True, alt_starts=True)),
                                       ("CAA", dict(start=True, alt_starts=True))], ids=["ATG", "CAT", "GTG", "CAA"])
def test_one_start_at_every_seam(ctx, word, mode):
    seq = long_gc()
    for at in SEAMS:
        for headless in (False, True):
            text = ("" if headless else ">s\n") + plant(seq, at, word) + "\n"
            out, rows, _ = check(ctx, text.encode(), 1, **mode)
            assert 1 <= len(rows) <= 3  # (the planted start, and what its letters spell with their neighbours)
    # a stop on either side of the start, each across a tile boundary from it; then two starts in one stretch
    forward = word[0] in "AG"
    both = plant(plant(plant(seq, 3, "TAA" if forward else "TTA"), SPAN + 3, word), 2 * SPAN, "TAG" if forward else "CTA")
    check(ctx, (">b\n" + both).encode(), 1, **mode)
    two = plant(plant(seq, SPAN - 3, word), SPAN + 3 * 7, word)
    out, rows, _ = check(ctx, (">t\n" + two).encode(), 1, **mode)
    assert 1 <= len(rows) <= 3
    if not mode.get("alt_starts"):  # without alt_starts GTG and CAA start nothing
        for w in ("GTG", "TTG", "CAC", "CAA"):
            assert len(check(ctx, (">n\n" + plant(seq, SPAN, w)).encode(), 1, **mode)[1]) == 0


def test_record_start_shifted_by_the_header(ctx):
    seq = plant(plant(long_gc(), SPAN - 1, "TGA"), SPAN + 64, "TCA")
    for shift in range(16):
        check(ctx, (">" + "h" * shift + " rest of the line\n" + wrap(seq, 61)).encode(), 1)


def test_many_records_in_one_tile(ctx):
    rng = random.Random(5)
    recs = [dna(rng, rng.randrange(3, 41)) for _ in range(300)]
    used = sum(len(s) + 1 for s in recs)  # (a separator a record)
    assert used + 1 < SPAN
    filler = dna(rng, SPAN - used - 1)  # its last base is stream position SPAN - 1: the record ends exactly on the boundary
    text = "".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(recs + [filler]))
    for min_aa in (1, 5):
        check(ctx, text.encode(), min_aa)  # the stream's end stands at position SPAN
        check(ctx, (text + ">next\n" + dna(rng, 50) + "\n").encode(), min_aa)  # a separator does
        check(ctx, (text + ">next\n" + dna(rng, 50) + "\n").encode(), min_aa, start=True)
    # records shorter than a lane's run, many to a lane, in several tiles
    text = "".join(">q%d\n%s\n" % (i, dna(rng, rng.randrange(0, 12))) for i in range(4000))
    check(ctx, text.encode(), 1)
    check(ctx, text.encode(), 2, start=True, alt_starts=True)


# ------------------------------------------------------------------------------------------ text shapes and bytes
def shapes_text(headless: bool) -> bytes:
    rng = random.Random(21)
    t = [gc(rng, 120) + "\n" + gc(rng, 30) + "\n" if headless else " \n\t\n"]
    t.append(">wrapped lf\n" + wrap(dna(rng, 400), 60))
    t.append(">crlf one\r\n" + wrap(dna(rng, 333), 70, "\r\n"))
    t.append(">cr\r" + wrap(dna(rng, 200), 50, "\r"))
    t.append(">only a header\n")
    t.append(">\n" + gc(rng, 150) + "\n")  # an empty name
    t.append("  \t>blanks in front\tx\n" + gc(rng, 150) + "\n")
    t.append(">na\xc3\xafve \xe9\n" + gc(rng, 150) + "\n")
    t.append(">star\n" + dna(rng, 70) + "*" + dna(rng, 70) + "**\n*\n")
    t.append(">lower\n" + dna(rng, 200).lower() + "\n")
    t.append(">mixed Nn Uu\n" + dna(rng, 300, "ACGTNacgtnUu") + "\n")
    t.append(">all n\n" + "N" * 100 + "\n>all n too\n" + "n" * 7 + "\n")
    t.append(">other bytes\n" + dna(rng, 300, "ACGTRYKM-.12") + "\n")
    t.append(">empty lines\n\n" + dna(rng, 100) + "\n\n" + dna(rng, 100) + "\n\n")
    t.append(">open last line\n" + dna(rng, 130))
    return "".join(t).encode("latin-1")


@pytest.mark.parametrize("headless", [False, True], ids=["blanks_first", "headless"])
def test_text_shapes_and_bytes(ctx, headless):
    text = shapes_text(headless)
    for mode in MODES:
        out, rows, info = check(ctx, text, 8, **mode)
        assert info["headless"] == int(headless) and len(rows) > 0
    out, rows, _ = check(ctx, text, 30)
    assert b">na\xc3\xafve_" in out and (b"\n>_" in out) and (b"\n>blanks_" in out)
    if headless:  # the headless record has the empty name; of its 150 bases class 1 ends first, at 148
        assert out.startswith(b">_2_2_1\n")
    assert b"X" * 30 + b"\n" in out  # an all-N record: six frames of X
    with pytest.raises(native.NonAsciiInput):
        ctx.orfs(b">a\nACGT\xc3\xa9ACGT\n")
    check(ctx, b"")
    check(ctx, b"\n\n")
    check(ctx, b">only\n")
    check(ctx, b"ACG", 1)


# ------------------------------------------------------------------------------------------ decimal fields
def test_decimal_fields_and_output_alignment(ctx):
    rng = random.Random(9)
    nines, tens = gc(rng, 1100), gc(rng, 1100)
    for at in (5, 95, 995):  # a stretch begins behind a stop: at 8, 98, 998 and at 9, 99, 999
        nines, tens = plant(nines, at, "TAA"), plant(tens, at + 1, "TAA")
    text = (">a\n" + wrap(dna(rng, 30000), 80) + ">nines\n" + nines + "\n>tens\n" + tens + "\n").encode()
    out, rows, _ = check(ctx, text, 1)
    assert sum(1 for r in rows if r[0] == 0) > 1000  # ranks pass 9 / 10, 99 / 100 and 999 / 1000
    assert {9, 99, 999} <= set(int(r[1]) + 1 for r in rows if r[0] == 1)
    assert {10, 100, 1000} <= set(int(r[1]) + 1 for r in rows if r[0] == 2)
    assert b">nines_9_3_" in out and b">tens_1000_1_" in out and b">a_" in out and b"_1000\n" in out
    at, residues = 0, set()
    for line in out.split(b"\n"):
        if line.startswith(b">"):
            residues.add(at % 16)
        at += len(line) + 1
    assert residues == set(range(16))  # output records start at every residue mod 16
    check(ctx, text, 1, strand="minus")
    check(ctx, text, 3, start=True)


# ------------------------------------------------------------------------------------------------ start mode
def test_start_mode_and_strands(ctx):
    rng = random.Random(13)
    text = "".join(">s%d\n%s\n" % (i, wrap(dna(rng, rng.randrange(50, 2500)), 70)) for i in range(40)).encode()
    seen = {}
    for mode in MODES:
        for min_aa in (1, 20):
            out, rows, _ = check(ctx, text, min_aa, **mode)
            seen[(min_aa,) + tuple(sorted(mode.items()))] = rows
    stop, start, alt = (seen[(1,) + tuple(sorted(m.items()))] for m in MODES[:3])
    assert len(alt) > len(start) > 0 and len(stop) > len(alt)  # stretches without a start yield nothing
    plus, minus = (seen[(1, ("strand", s))] for s in ("plus", "minus"))
    assert len(plus) + len(minus) == len(stop) and set(plus[:, 3].tolist()) == {1, 2, 3} and set(minus[:, 3].tolist()) == {4, 5, 6}
    for bad in (dict(alt_starts=True), dict(strand="neither")):
        with pytest.raises(ValueError):
            ctx.orfs(text, **bad)


# ------------------------------------------------------------------------------------------------ pieces
def test_pieces(ctx):
    rng = random.Random(17)
    text = (dna(rng, 200) + "\n" + "".join(">p%d x\n%s" % (i, wrap(dna(rng, rng.randrange(0, 900)), 60)) for i in range(120))).encode()
    w_out, w_rows = rule.expected(text, 10)
    assert max(r[0] for r in w_rows) > 100
    for piece_bytes in (0, 1, 700, 1500, 20000, len(text)):  # one record a piece, one or two, many, all
        info = {}
        out, rows = ctx.orfs(text, min_aa=10, piece_bytes=piece_bytes, info=info)
        assert out == w_out and rows.tolist() == w_rows  # (record numbers the whole call)
        if piece_bytes == 1:
            assert info["pieces"] > 60
    check(ctx, text, 10, piece_bytes=700, start=True)


# ------------------------------------------------------------------------------------------------ device call
def _raw(ctx, text: bytes, out_cap: int, cap: int, opt=(32, 0), null_out=False, rows=True, null_opt=False, piece_bytes=0):
    out = np.full(out_cap + 8, 0xA5, dtype=np.uint8)
    raw = np.full((cap + 1) * 24, 0xA5, dtype=np.uint8)
    out_len, n, st = ctypes.c_size_t(0), ctypes.c_size_t(0), native.Orf()
    o = native.OrfOpt(*opt)
    rc = ctx._L.mk_orf_text(ctx._h, text, len(text), piece_bytes, None if null_opt else ctypes.byref(o), None if null_out else out.ctypes.data,
                            out_cap, ctypes.byref(out_len), raw.ctypes.data if rows else None, cap, ctypes.byref(n), ctypes.byref(st))
    return dict(rc=rc, out=out, raw=raw, out_len=out_len.value, n=n.value, st=st)


def test_capacities_and_arguments(ctx):
    rng = random.Random(19)
    text = "".join(">c%d\n%s\n" % (i, dna(rng, 700)) for i in range(30)).encode()
    w_out, w_rows = rule.expected(text, 32)
    no, nr = len(w_out), len(w_rows)
    assert nr > 20
    for piece_bytes in (0, 4096):
        got = _raw(ctx, text, no, nr, piece_bytes=piece_bytes)  # exactly enough: the bytes behind each capacity untouched
        assert (got["rc"], got["out_len"], got["n"]) == (0, no, nr) and got["st"].bytes_out == no
        assert got["out"][:no].tobytes() == w_out and (got["out"][no:] == 0xA5).all()
        assert native.orf_rows(got["raw"][:nr * 24].view(native.ORF_ROW_DTYPE)).tolist() == w_rows and (got["raw"][nr * 24:] == 0xA5).all()
        got = _raw(ctx, text, no - 1, nr, piece_bytes=piece_bytes)  # out one short: both needed sizes, nothing past the cap
        assert (got["rc"], got["out_len"], got["n"]) == (RANGE, no, nr) and (got["out"][no - 1:] == 0xA5).all()
        got = _raw(ctx, text, no, nr - 1, piece_bytes=piece_bytes)  # rows one short
        assert (got["rc"], got["out_len"], got["n"]) == (RANGE, no, nr) and (got["raw"][(nr - 1) * 24:] == 0xA5).all()
        msg = ctx._L.mk_last_error(ctx._h).decode()
        assert str(no) in msg and str(nr) in msg
        got = _raw(ctx, text, 0, 0, null_out=True, piece_bytes=piece_bytes)  # the sizing call
        assert (got["rc"], got["out_len"], got["n"]) == (RANGE, no, nr) and (got["raw"] == 0xA5).all()
    got = _raw(ctx, text, no, 0, rows=False)  # rows NULL: cap is ignored
    assert (got["rc"], got["out_len"], got["n"]) == (0, no, nr) and got["out"][:no].tobytes() == w_out
    for opt, word in (((0, 0), "min_aa"), ((32, 16), "flag"), ((32, native.ORF_ALT), "MK_ORF_START"),
                      ((32, native.ORF_PLUS | native.ORF_MINUS), "contradict")):
        got = _raw(ctx, text, no, nr, opt=opt)
        assert got["rc"] == ARG and word in ctx._L.mk_last_error(ctx._h).decode() and (got["out"] == 0xA5).all()
    got = _raw(ctx, text, no, nr, null_opt=True)
    assert got["rc"] == ARG and "opt" in ctx._L.mk_last_error(ctx._h).decode()


def test_device_call(ctx):
    import torch
    rng = random.Random(23)
    text = (">d one\n" + wrap(dna(rng, 5000), 60) + ">d two\n" + dna(rng, 900) + "\n>d three\n" + dna(rng, 40) + "\n").encode()
    w_out, w_rows = rule.expected(text, 12)
    no, nr = len(w_out), len(w_rows)
    for lead in range(16):
        out_lead = (5 * lead + 3) % 16
        host = np.frombuffer(b"#" * lead + text + b"#" * 9, dtype=np.uint8).copy()
        d_text = torch.from_numpy(host).cuda()
        d_out = torch.full((out_lead + no + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rows = torch.full(((nr + 1) * 24,), 0xA5, dtype=torch.uint8, device="cuda")
        assert d_out.data_ptr() % 16 == 0 and d_rows.data_ptr() % 8 == 0
        torch.cuda.synchronize()
        info = ctx.orfs_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, no, d_rows.data_ptr(), nr, min_aa=12)
        got = d_out.cpu().numpy()
        assert info["bytes_out"] == no and info["orfs"] == nr and info["pieces"] == 1 and info["records"] == 3
        assert got[out_lead:out_lead + no].tobytes() == w_out
        assert (got[:out_lead] == 0xA5).all() and (got[out_lead + no:] == 0xA5).all()  # the sentinels around out
        raw = d_rows.cpu().numpy()
        assert native.orf_rows(raw[:nr * 24].view(native.ORF_ROW_DTYPE)).tolist() == w_rows and (raw[nr * 24:] == 0xA5).all()
        assert (d_text.cpu().numpy() == host).all()  # the input is unmodified
    base = d_text.data_ptr() + 15
    with pytest.raises(native.MercatHipError) as e:  # the sizing call
        ctx.orfs_device(base, len(text), 0, 0, min_aa=12)
    assert e.value.code == RANGE and e.value.needed == (no, nr)
    with pytest.raises(native.MercatHipError) as e:
        ctx.orfs_device(base, len(text), d_out.data_ptr(), no - 1, d_rows.data_ptr(), nr - 1, min_aa=12)
    assert e.value.code == RANGE and e.value.needed == (no, nr)
    with pytest.raises(native.MercatHipError) as e:
        ctx.orfs_device(base, len(text), d_out.data_ptr(), no, d_rows.data_ptr() + 4, nr, min_aa=12)
    assert e.value.code == ARG


# ------------------------------------------------------------------------------------------------ context
def test_context_rules():
    rng = random.Random(29)
    text = "".join(">k%d\n%s\n" % (i, dna(rng, 400)) for i in range(20)).encode()
    w_out, w_rows = rule.expected(text, 16)
    with native.Counter(9, NT) as c:
        c.count_chunk(text, 1)
        before, size = c.to_dict(), c.rows()
        out, rows = c.orfs(text, 16)
        assert out == w_out and rows.tolist() == w_rows
        assert c.rows() == size and c.to_dict() == before  # the table's export is what it was
        assert c._L.mk_chunk_begin(c._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            c.orfs(text, 16)
        assert e.value.code == STATE
        assert c._L.mk_chunk_end(c._h, 1) == 0
        assert c.orfs(text, 16)[0] == w_out
    for alphabet, k in ((AA, 5), (native.ALPHABET_RAW, 40), (NT, 63)):  # any context serves
        with native.Counter(k, alphabet) as c:
            out, rows = c.orfs(text, 16)
            assert out == w_out and rows.tolist() == w_rows


# ------------------------------------------------------------------------------------------------ fixture
def test_prodigal_fixture(ctx):
    text = (GOLDEN / "orf" / "RW1_24k.fna").read_bytes()
    prots = rule.proteins((GOLDEN / "orf" / "RW1_24k_pro.faa").read_bytes())
    assert len(prots) == 22
    out, rows, _ = check(ctx, text, 32)
    assert len(rows) == 265

    def seqs(got):
        return [line for line in got.decode().split("\n") if line and not line.startswith(">")]

    stop, start, alt = (seqs(check(ctx, text, 20, **mode)[0]) for mode in MODES[:3])
    assert sum(any(s.endswith(p[1:]) for s in stop) for _, p in prots) == 22
    whole = [p for h, p in prots if "partial=00" in h and "start_type=ATG" in h]
    assert len(whole) == 16 and sum(any(s.endswith(p) for s in start) for p in whole) == 16
    complete = [p for h, p in prots if "partial=00" in h]
    assert len(complete) == 21 and sum(any(s.endswith(p[1:]) for s in alt) for p in complete) == 21


# ------------------------------------------------------------------------------------------------ front ends
def fastq_text(seed: int, reads: int):
    rng = random.Random(seed)
    fq, fa = [], []
    for i in range(reads):
        s = dna(rng, rng.randrange(60, 260))
        fq.append("@read%d extra\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
        fa.append(">read%d extra\n%s\n" % (i, s))
    return "".join(fq).encode(), "".join(fa).encode()


def test_orf_reads_fasta_gz_fastq(tmp_path):
    fq, fa = fastq_text(31, 80)
    assert native.fq2fa(fq)[0] == fa
    for name, data in (("r.fna", fa), ("r.fna.gz", gzip.compress(fa)), ("r.fastq", fq), ("r.fq.gz", gzip.compress(fq))):
        (tmp_path / name).write_bytes(data)
    for mode in (dict(min_aa=20), dict(min_aa=10, start=True, strand="minus")):
        w_out, w_rows = rule.expected(fa, **mode)
        assert len(w_rows) > 10
        names = [n for n, _ in rule.records(fa)]
        w_tsv = b"record\tname\tbegin\tend\tstrand\tframe\taa\n" + b"".join(
            b"%d\t%s\t%d\t%d\t%s\t%d\t%d\n" % (r, names[r], b, b + 3 * aa, b"+" if f < 4 else b"-", f, aa) for r, b, aa, f in w_rows)
        for name in ("r.fna", "r.fna.gz", "r.fastq", "r.fq.gz"):
            for dest in ("o.faa", "o.faa.gz"):
                res = kmers.orf_reads(tmp_path / name, tmp_path / dest, tsv_path=tmp_path / "o.tsv", **mode)
                data = (tmp_path / dest).read_bytes()
                if dest.endswith(".gz"):
                    assert data[:2] == b"\x1f\x8b"
                    data = gzip.decompress(data)
                assert data == w_out, (name, dest)
                assert (tmp_path / "o.tsv").read_bytes() == w_tsv
                assert res["orfs"] == len(w_rows) and res["records"] == 80 and res["bytes_out"] == len(w_out)
                assert not any(key.startswith("s_") for key in res)
    assert kmers.orf_reads(fa, None, min_aa=20)["orfs"] == len(rule.expected(fa, 20)[1])


def test_cli_orf(tmp_path):
    k = 3
    rng = random.Random(37)
    samples = {"one": "".join(">a%d\n%s\n" % (i, wrap(dna(rng, 900), 60)) for i in range(5)),
               "two": "".join(">b%d x\n%s\n" % (i, wrap(dna(rng, 700, "ACGTN" if i == 2 else "ACGT"), 70)) for i in range(6))}
    for base, data in samples.items():
        (tmp_path / (base + ".fna")).write_text(data)
    out = tmp_path / "out"
    argv = ["-i", str(tmp_path / "one.fna"), str(tmp_path / "two.fna"), "-k", str(k), "-c", "1", "-o", str(out)]
    assert cli.main(argv + ["-orf", "20"]) == 0
    assert sorted(p.name for p in (out / "orf").iterdir()) == ["one_orf.faa", "one_orf.tsv", "two_orf.faa", "two_orf.tsv"]
    for base in samples:
        cleaned = gzip.decompress((out / "clean" / ("%s_clean.fna.gz" % base)).read_bytes())
        w_out, w_rows = rule.expected(cleaned, 20)
        assert len(w_rows) > 5
        assert (out / "orf" / ("%s_orf.faa" % base)).read_bytes() == w_out
        assert (out / "orf" / ("%s_orf.tsv" % base)).read_bytes().count(b"\n") == len(w_rows) + 1
    assert b"_1_" in (out / "orf" / "two_orf.faa").read_bytes()
    # the same tables as a separate run over the .faa files with -i
    again = tmp_path / "again"
    assert cli.main(["-i", str(out / "orf" / "one_orf.faa"), str(out / "orf" / "two_orf.faa"), "-k", str(k), "-c", "1", "-o", str(again)]) == 0
    for base in samples:
        table = (out / "tsv_protein" / ("%s_orf_counts.tsv" % base)).read_bytes()
        assert table.count(b"\n") > 100 and table == (again / "tsv_protein" / ("%s_orf_counts.tsv" % base)).read_bytes()
        assert (out / "tsv_nucleotide" / ("%s_counts.tsv" % base)).exists()
    assert (out / "combined_protein.tsv").read_bytes() == (again / "combined_protein.tsv").read_bytes()
    # -skipclean: the raw text; start mode and the strand reach the call
    skip = tmp_path / "skip"
    assert cli.main(argv[:-1] + [str(skip), "-skipclean", "-orf", "-orf_start", "-orf_alt", "-orf_strand", "plus"]) == 0
    for base, data in samples.items():
        assert (skip / "orf" / ("%s_orf.faa" % base)).read_bytes() == rule.expected(data.encode(), 32, True, True, "plus")[0]
    # without -orf nothing of it appears
    plain = tmp_path / "plain"
    assert cli.main(argv[:-1] + [str(plain)]) == 0
    assert not (plain / "orf").exists() and not (plain / "tsv_protein").exists()
    for base in samples:
        assert (plain / "tsv_nucleotide" / ("%s_counts.tsv" % base)).read_bytes() == (out / "tsv_nucleotide" / ("%s_counts.tsv" % base)).read_bytes()
