"""Reads filtered against the GPU tables (mk_filter_text / mk_filter_device, Counter.filter*, kmers.filter_reads, -filter).
Expected output never comes from the code under test: the table is a dict made by the CPU oracle, a record's row is
plain Python over ``dict.get(window, 0)`` on the reference's line loop (restated in tests/filter_rule.py), its byte range
comes from a regular expression over the raw text that knows nothing of the parser, and the rule is applied in Python
integers.
Equality is exact: in the bytes, in the keep mask and in the rows."""
import ctypes
import functools
import gzip
import random

import numpy as np
import pytest

from filter_rule import expected, matched, ref_ranges, ref_records
from mercat2_amd import cli, kmers, native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE, NON_ASCII, RANGE = -1, -4, -5, -7
COMP = str.maketrans("ACGT", "TGCA")
RULES = [(1, 1, 0), (1, 1, 500_000), (2, 1, 1_000_000), (1, 3, 0)]  # (at_least, min_hits, min_ppm)


# ------------------------------------------------------------------------------------------------- the oracle
def check(ctx, text: bytes, table: dict, rule, invert: bool = False, fold=None, folded_table: bool = False, want=None, **kw):
    info = {}
    out, keep, rows = ctx.filter(text, rule[0], rule[1], rule[2], invert, fold=fold, info=info, **kw)
    w_out, w_keep, w_rows, w_pre = want or expected(text, table, ctx.k, rule, invert, folded_table)
    assert rows.dtype == np.uint64 and rows.shape == (len(w_rows), 5) and rows.tolist() == w_rows
    assert keep.dtype == bool and keep.tolist() == w_keep
    assert out == w_out
    assert info["records"] == len(w_rows) and info["bytes"] == len(text) and info["preamble"] == w_pre
    assert info["records_out"] == sum(w_keep) and info["bytes_out"] == len(w_out)
    assert info["windows"] == sum(r[0] for r in w_rows) and info["hits"] == sum(r[1] for r in w_rows)
    return out, keep, rows, info


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def wrap(seq, width):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


# --------------------------------------------------------------------------------------------- record shapes
@functools.lru_cache(maxsize=None)
def shapes(k: int, headless: bool):
    """(text, its short sequences, its long sequence): every record shape of the issue in one text."""
    rng = random.Random(4000 + k)
    long_seq = dna(rng, 40_011)
    short = [dna(rng, k + i % 4) for i in range(300)]
    t = [dna(rng, k + 2) + "\n  \n" if headless else "  \n\t\n*\n \x0b\n"]
    t += ["  >lead blanks\n" + dna(rng, k + 1) + "\n", "\t \x1c>more\x0b\n" + dna(rng, k) + "\n"]
    t += [">h1\n>h2\n" + dna(rng, k + 3) + "\n", ">\n" + dna(rng, k + 1) + "\n", " >\n"]
    t += [">wrapped\n" + wrap(dna(rng, 3 * k + 5), 7)]
    s = dna(rng, 2 * k + 4)
    t += [">crlf\r\n" + s[:5] + "\r\n" + s[5:] + "\r\n", " >crlf2\r\n" + short[3] + "\r\n"]
    t += [">cr\r" + dna(rng, k + 2) + "\r" + dna(rng, 3) + "\r", "  >cr2\r" + short[5] + "\r"]
    s = dna(rng, k + 6)
    t += [">star\n" + s[:3] + "*" + s[3:] + "**\n*\n", ">blank\n  " + dna(rng, 5) + " \t" + dna(rng, k + 1) + "  \n"]
    t += [">before blank lines\n" + short[8] + "\n\n  \n\t\n", ">after them\n" + dna(rng, k) + "\n"]
    s = dna(rng, 2 * k)
    t += [">gt inside\n" + s[:k] + ">" + s[k:] + "\nAC>GT > x\n" + short[9] + "\n"]
    t += [">s%d\n%s\n" % (i, seq) for i, seq in enumerate(short)]  # many records to a lane; offsets of every residue mod 16
    t += [">long\n" + wrap(long_seq, 60)]                          # a record that spans lanes, waves and workgroups
    t += [">t%d\n%s\n" % (i, dna(rng, k + 1 + i)) for i in range(3)]
    t += [">piece of long\n" + long_seq[17_000:17_000 + 2 * k] + "\n", "  >last one"]
    return "".join(t).encode(), tuple(short), long_seq


@functools.lru_cache(maxsize=None)
def other_text(k: int) -> bytes:
    """Another text: half of the long record (a stretch of it twice), some of the short records once, some twice."""
    _, short, long_seq = shapes(k, False)
    rng = random.Random(77 + k)
    t = [">x\n" + wrap(dna(rng, 3_000), 70), ">y\n" + wrap(long_seq[:20_000], 80), ">z\n" + wrap(long_seq[16_000:19_000], 50)]
    t += [">once%d\n%s\n" % (i, short[i]) for i in range(0, 300, 3)]
    t += [">twice%d\n%s\n" % (i, short[i]) for i in range(0, 300, 6)]
    return "".join(t).encode()


@functools.lru_cache(maxsize=None)
def table_of(text: bytes, k: int) -> dict:
    return cpu_ref.count_text(text, k, 1)


@functools.lru_cache(maxsize=None)
def shapes_expected(k: int, headless: bool, rule, invert: bool):
    return expected(shapes(k, headless)[0], table_of(other_text(k), k), k, rule, invert)


@pytest.mark.parametrize("headless", [False, True], ids=["blanks_first", "headless"])
@pytest.mark.parametrize("k", [5, 31])
def test_record_shapes(k, headless):
    text = shapes(k, headless)[0]
    table = table_of(other_text(k), k)
    assert k == 5 or {1, 2} <= set(table.values())
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        for rule in RULES:
            outs = {}
            for invert in (False, True):
                want = shapes_expected(k, headless, rule, invert)
                out, keep, rows, info = check(ctx, text, table, rule, invert, want=want)
                assert info["headless"] == (1 if headless else 0) and info["pieces"] == 1
                outs[invert] = (out, keep, info)
            # the partition: every record in exactly one of the two outputs, the preamble in neither
            (m_out, m_keep, m_info), (u_out, u_keep, u_info) = outs[False], outs[True]
            assert (m_keep ^ u_keep).all() and m_info["preamble"] == u_info["preamble"] == (0 if headless else 10)
            assert len(m_out) + len(u_out) + m_info["preamble"] == len(text)
            ranges, _ = ref_ranges(text)
            assert b"".join(text[a:b] for a, b in ranges) == text[m_info["preamble"]:]
            if k == 31:  # each rule splits this text: both outputs hold records, the long record among the decided ones
                assert 0 < m_keep.sum() < len(m_keep), rule
        assert ctx.to_dict() == table


def test_rules_differ():
    """The four rules give four different selections of the k = 31 text (so none of them is decided by another's code)."""
    keeps = [tuple(shapes_expected(31, False, rule, False)[1]) for rule in RULES]
    assert len(set(keeps)) == len(RULES)


def test_pieces():
    k = 31
    base, short, _ = shapes(k, True)
    rng = random.Random(9)
    text = base + b"\n" + "".join(">e%d\n%s\n" % (i, short[i % 300] if i % 3 else dna(rng, k + i % 5)) for i in range(2_000)).encode()
    table = table_of(other_text(k), k)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        for rule, invert in ((RULES[0], False), (RULES[2], True)):
            want = expected(text, table, k, rule, invert)
            one = check(ctx, text, table, rule, invert, want=want)
            many = check(ctx, text, table, rule, invert, want=want, piece_bytes=4096)
            assert one[3]["pieces"] == 1 and many[3]["pieces"] >= 20 and many[3]["headless"] == 1
            assert one[0] == many[0] and (one[1] == many[1]).all() and one[2].tolist() == many[2].tolist()


# ---------------------------------------------------------------------------------------------------- extremes
def test_extremes():
    k = 5
    text = b" \n\t\n>a\nACGTACGTAC\n>b\nACGTA\n  >c\nTTTTTTT\n>d"
    table = table_of(text, k)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(text, 1)
        # everything kept: the text from the first record on (record d has no windows: it is unmatched, so invert nothing)
        body = b" \n\t\n>a\nACGTACGTAC\n>b\nACGTA\n  >c\nTTTTTTT\n"
        out, keep, _, info = check(ctx, body, table, (1, 1, 0))
        assert out == body[4:] and keep.all() and info["preamble"] == 4
        # nothing kept
        out, keep, _, info = check(ctx, text, table, (99, 1, 0))
        assert out == b"" and not keep.any() and info["bytes_out"] == 0 and info["records_out"] == 0
        # the same through the ABI: *out_len = 0, nothing written
        rc, out_len, n, buf, _, _ = raw_filter(ctx, text, (99, 1, 0), 0, out_cap=len(text), cap=4)
        assert (rc, out_len, n) == (0, 0, 4) and (buf == 0xA5).all()
        # an empty text
        out, keep, rows, info = check(ctx, b"", table, (1, 1, 0))
        assert out == b"" and keep.shape == (0,) and rows.shape == (0, 5) and info["records"] == 0 and info["preamble"] == 0
        rc, out_len, n, _, _, _ = raw_filter(ctx, b"", (1, 1, 0), 0, out_cap=0, cap=0)
        assert (rc, out_len, n) == (0, 0, 0)
        # one header without a newline
        for invert, want in ((False, b""), (True, b">only")):
            out, keep, rows, info = check(ctx, b">only", table, (1, 1, 0), invert)
            assert out == want and keep.tolist() == [invert] and rows.tolist() == [[0] * 5] and info["preamble"] == 0
        # blanks only: all preamble, no record, either way
        for invert in (False, True):
            blanks = b"  \n\t\r\n \x0b\x0c\n***\n"
            out, keep, rows, info = check(ctx, blanks, table, (1, 1, 0), invert)
            assert out == b"" and keep.shape == (0,) and info["preamble"] == len(blanks) and info["records"] == 0
        # headless and nothing else
        out, keep, _, info = check(ctx, b"ACGTACGTAC", table, (1, 1, 0))
        assert out == b"ACGTACGTAC" and keep.tolist() == [True] and info["headless"] == 1 and info["preamble"] == 0


# -------------------------------------------------------------------------------------------------- the raw ABI
def raw_filter(ctx, text: bytes, rule, flags: int, out_cap: int, cap: int, with_rows: bool = True, with_keep: bool = True,
               rule_ptr="given"):
    """mk_filter_text with guarded buffers: (rc, *out_len, *nrows, out, rows, keep); 0xA5 / 0xA5A5 where nothing was written."""
    out = np.full(out_cap + 64, 0xA5, dtype=np.uint8)
    rows = np.full((cap + 1, 5), 0xA5A5, dtype=np.uint64)
    keep = np.full(cap + 1, 0xA5, dtype=np.uint8)
    out_len, n = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    r = native.FilterRule(*rule, 0) if rule is not None else None
    rc = native.lib().mk_filter_text(ctx._h, text, len(text), 0, flags, ctypes.byref(r) if r is not None else None, out.ctypes.data, out_cap,
                                     ctypes.byref(out_len), rows.ctypes.data if with_rows else None,
                                     keep.ctypes.data if with_keep else None, cap, ctypes.byref(n), None)
    return rc, out_len.value, n.value, out, rows, keep


def test_caps_and_null_buffers():
    k = 31
    text = shapes(k, False)[0]
    rule = RULES[0]
    w_out, w_keep, w_rows, _ = shapes_expected(k, False, rule, False)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        rc, out_len, n, out, rows, keep = raw_filter(ctx, text, rule, 0, len(w_out), len(w_rows))
        assert (rc, out_len, n) == (0, len(w_out), len(w_rows))
        assert out[:out_len].tobytes() == w_out and (out[out_len:] == 0xA5).all()
        assert rows[:n].tolist() == w_rows and (rows[n] == 0xA5A5).all() and keep[:n].tolist() == w_keep and keep[n] == 0xA5
        # out one byte short: the needed size, nothing past the cap
        rc, out_len, n, out, rows, keep = raw_filter(ctx, text, rule, 0, len(w_out) - 1, len(w_rows))
        assert (rc, out_len, n) == (RANGE, len(w_out), len(w_rows)) and (out[len(w_out) - 1:] == 0xA5).all()
        assert "out has room" in ctx._L.mk_last_error(ctx._h).decode()
        # rows short by one
        rc, out_len, n, out, rows, keep = raw_filter(ctx, text, rule, 0, len(w_out), len(w_rows) - 1)
        assert (rc, out_len, n) == (RANGE, len(w_out), len(w_rows)) and (rows[len(w_rows) - 1:] == 0xA5A5).all()
        assert (keep[len(w_rows) - 1:] == 0xA5).all()
        # rows or keep NULL, or both with cap = 0
        rc, out_len, n, out, rows, keep = raw_filter(ctx, text, rule, 0, len(w_out), len(w_rows), with_rows=False)
        assert (rc, out_len, n) == (0, len(w_out), len(w_rows)) and keep[:n].tolist() == w_keep and (rows == 0xA5A5).all()
        rc, out_len, n, out, rows, keep = raw_filter(ctx, text, rule, 0, len(w_out), len(w_rows), with_keep=False)
        assert (rc, out_len, n) == (0, len(w_out), len(w_rows)) and rows[:n].tolist() == w_rows and (keep == 0xA5).all()
        rc, out_len, n, out, rows, keep = raw_filter(ctx, text, rule, 0, len(w_out), 0, with_rows=False, with_keep=False)
        assert (rc, out_len, n) == (0, len(w_out), len(w_rows)) and out[:out_len].tobytes() == w_out


def test_errors():
    k = 31
    text = shapes(k, False)[0]
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        table = ctx.to_dict()
        err = lambda: ctx._L.mk_last_error(ctx._h).decode()
        for rule, word in (((0, 1, 0), "at_least"), ((1, 0, 0), "min_hits"), ((1, 1, 1_000_001), "min_ppm")):
            rc = raw_filter(ctx, text, rule, 0, len(text), 1000)[0]
            assert rc == ARG and word in err() and err().startswith("mk_filter_text")
            with pytest.raises(native.MercatHipError) as e:
                ctx.filter(text, *rule)
            assert e.value.code == ARG and word in str(e.value)
        assert raw_filter(ctx, text, None, 0, len(text), 1000)[0] == ARG and "rule" in err()
        for flags in (4, 8, 1 << 31, 2 | 16):
            assert raw_filter(ctx, text, (1, 1, 0), flags, len(text), 1000)[0] == ARG and "flag" in err()
        assert raw_filter(ctx, text, (1, 1, 0), native.FILTER_FOLD, len(text), 1000)[0] == ARG  # (not a canonical context)
        # a byte >= 0x80: refused in a sequence line, fine in a header line
        with pytest.raises(native.NonAsciiInput):
            ctx.filter(b">a\nACGT\xc3\xa9ACGT\n")
        assert ctx.filter(b">a \xc3\xa9\nACGT\n", invert=True)[0] == b">a \xc3\xa9\nACGT\n"
        # an open chunk
        assert ctx._L.mk_chunk_begin(ctx._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            ctx.filter(text)
        assert e.value.code == STATE
        assert ctx._L.mk_chunk_end(ctx._h, 1) == 0
        stats = ctx.stats()
        check(ctx, text, table, RULES[0], want=shapes_expected(k, False, RULES[0], False))
        after = ctx.stats()
        assert all(after[f] == stats[f] for f in ("raw_bytes", "symbols", "windows", "exotic_windows", "chunks", "survivors"))
        assert ctx.to_dict() == table


# ---------------------------------------------------------------------------------------------- the device call
@pytest.mark.parametrize("out_lead", [0, 5])
def test_filter_device(out_lead):
    import torch
    k, lead = 31, 1
    text = shapes(k, True)[0]
    rule = RULES[1]
    w_out, w_keep, w_rows, _ = shapes_expected(k, True, rule, False)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
        assert (d_text.data_ptr() + lead) % 16 == 1

        def run(out_cap, cap):
            d_out = torch.full((out_lead + out_cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            d_rows = torch.full((cap + 1, 5), -1, dtype=torch.int64, device="cuda")
            d_keep = torch.full((cap + 1,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            n, out_len, st = ctypes.c_size_t(0), ctypes.c_size_t(0), native.Filter()
            r = native.FilterRule(*rule, 0)
            rc = ctx._L.mk_filter_device(ctx._h, d_text.data_ptr() + lead, len(text), 0, ctypes.byref(r), d_out.data_ptr() + out_lead,
                                         out_cap, ctypes.byref(out_len), d_rows.data_ptr(), d_keep.data_ptr(), cap, ctypes.byref(n),
                                         ctypes.byref(st))
            return (rc, out_len.value, n.value, d_out.cpu().numpy(), d_rows.cpu().numpy().view(np.uint64), d_keep.cpu().numpy(),
                    st.as_dict())

        rc, out_len, n, out, rows, keep, info = run(len(w_out), len(w_rows))
        assert (rc, out_len, n) == (0, len(w_out), len(w_rows))
        assert out[out_lead:out_lead + out_len].tobytes() == w_out
        assert (out[:out_lead] == 0xA5).all() and (out[out_lead + out_len:] == 0xA5).all()
        assert rows[:n].tolist() == w_rows and (rows[n] == np.uint64(2**64 - 1)).all()
        assert keep[:n].tolist() == w_keep and keep[n] == 0xA5
        assert info["bytes_out"] == len(w_out) and info["records_out"] == sum(w_keep) and info["pieces"] == 1
        rc, out_len, n, out, rows, keep, _ = run(len(w_out) - 1, len(w_rows))
        assert (rc, out_len, n) == (RANGE, len(w_out), len(w_rows)) and (out[out_lead + len(w_out) - 1:] == 0xA5).all()
        rc, out_len, n, out, rows, keep, _ = run(len(w_out), len(w_rows) - 1)
        assert (rc, out_len, n) == (RANGE, len(w_out), len(w_rows))
        assert (rows[len(w_rows) - 1:] == np.uint64(2**64 - 1)).all() and (keep[len(w_rows) - 1:] == 0xA5).all()
        # the Python wrapper
        d_out = torch.zeros(len(text), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        info = ctx.filter_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr(), len(text), at_least=rule[0], min_hits=rule[1],
                                 min_ppm=rule[2])
        assert d_out.cpu().numpy()[:info["bytes_out"]].tobytes() == w_out and info["records"] == len(w_rows)


# --------------------------------------------------------------------------------------------- other key shapes
def nt_small(seed: int) -> bytes:
    rng = random.Random(seed)
    recs = [">r%d x\n%s\n" % (i, wrap(dna(rng, rng.randrange(30, 260)), 70)) for i in range(60)]
    recs.insert(7, ">odd\n" + "ACGTTGCANGGATCCATGNAacgtACGGT*CAGT" * 6 + "\n>empty\n")
    return "".join(recs).encode()


def aa_small(seed: int) -> bytes:
    rng = random.Random(seed)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    recs = [">p%d\n%s\n" % (i, wrap("".join(rng.choice(letters) for _ in range(rng.randrange(10, 200))), 60)) for i in range(50)]
    recs.insert(9, ">odd\nMKV-LLAX*BZJUOacdeMKVLLAGGHHWWYYPPQQRRSSTTVVMKVLLAAGGHHWWYY.PPQQRRSSTTVVKKLL\n>empty\n")
    return "".join(recs).encode()


KEY_SHAPES = [("nt", NT, 40), ("aa", AA, 3), ("aa", AA, 14), ("raw", RAW, 9)]


@pytest.mark.parametrize("kind,alphabet,k", KEY_SHAPES, ids=["%s_k%d" % (s[0], s[2]) for s in KEY_SHAPES])
def test_other_key_shapes(kind, alphabet, k):
    text = (aa_small if kind == "aa" else nt_small)(3)
    cut = text.index(b">", len(text) // 2)
    source = text[cut:] + text[cut:text.index(b">", 3 * len(text) // 4)]  # the second half; its first records twice
    table = table_of(source, k)
    with native.Counter(k, alphabet) as ctx:
        ctx.count_chunk(source, 1)
        for rule in ((1, 1, 0), (2, 2, 900_000)):
            for invert in (False, True):
                out, keep, _, _ = check(ctx, text, table, rule, invert)
                assert 0 < keep.sum() < len(keep)


def test_canonical_fold():
    k = 31
    rng = random.Random(5)
    reads = [dna(rng, 150) for _ in range(40)]
    source = "".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(reads[:20])).encode()
    text = "".join(">f%d\n%s\n>r%d\n%s\n" % (i, r, i, r.translate(COMP)[::-1]) for i, r in enumerate(reads)).encode()
    folded = cpu_ref.canonical_fold(table_of(source, k))
    with native.Counter(k, NT, canonical=True) as ctx:
        ctx.count_chunk(source, 1)
        out, keep, _, info = check(ctx, text, folded, (1, 1, 1_000_000), folded_table=True)  # fold=None: as the context counts
        assert keep.tolist() == [True] * 40 + [False] * 40 and info["folded"] > 0
        check(ctx, text, folded, (1, 1, 1_000_000), True, fold=True, folded_table=True)
        check(ctx, text, folded, (1, 1, 600_000), fold=False)  # taken as they stand: the windows of the other strand miss


# ------------------------------------------------------------------------------------------------ files and CLI
def fastq_text(seed: int, n: int):
    """(FASTQ text, the FASTA fq2fa makes of it): four-line records, quality strings that begin with '>' and '@'."""
    rng = random.Random(seed)
    fq, fa = [], []
    for i in range(n):
        seq = dna(rng, rng.randrange(20, 90))
        qual = (">" if i % 3 == 0 else "@" if i % 3 == 1 else "I") + "".join(rng.choice("!#>@FI+") for _ in range(len(seq) - 1))
        fq.append("@read%d len=%d\n%s\n+%s\n%s\n" % (i, len(seq), seq, "read%d" % i if i % 2 else "", qual))
        fa.append(">read%d len=%d\n%s\n" % (i, len(seq), seq))
    return "".join(fq).encode(), "".join(fa).encode()


def test_filter_reads_fasta_gz_fastq(tmp_path):
    k = 11
    fq, fa = fastq_text(11, 120)
    source = fa[: fa.index(b">", len(fa) // 2)]
    table = table_of(source, k)
    (tmp_path / "r.fna").write_bytes(fa)
    (tmp_path / "r.fna.gz").write_bytes(gzip.compress(fa))
    (tmp_path / "r.fastq").write_bytes(fq)
    (tmp_path / "r.fq.gz").write_bytes(gzip.compress(fq))
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(source, 1)
        for invert in (False, True):
            w_out, w_keep, _, _ = expected(fa, table, k, (1, 2, 500_000), invert)
            assert 0 < sum(w_keep) < len(w_keep)
            for name in ("r.fna", "r.fna.gz", "r.fastq", "r.fq.gz"):
                for dest in ("o.fna", "o.fna.gz"):
                    res = kmers.filter_reads(ctx, tmp_path / name, tmp_path / dest, 1, 2, 0.5, invert)
                    data = (tmp_path / dest).read_bytes()
                    if dest.endswith(".gz"):
                        assert data[:2] == b"\x1f\x8b"
                        data = gzip.decompress(data)
                    assert data == w_out, (name, dest)
                    assert res == {"records": len(w_keep), "kept": sum(w_keep), "bytes_in": len(fa), "bytes_out": len(w_out)}
            # a property that needs no oracle: every record of the written file satisfies the rule (or fails it)
            rows = ctx.screen(tmp_path / "o.fna", 1)
            assert len(rows) == sum(w_keep) and all(matched(r, (1, 2, 500_000)) != invert for r in rows.tolist())
        with pytest.raises(ValueError):
            kmers.filter_reads(ctx, tmp_path / "r.fna", tmp_path / "x.fna", min_frac=1.5)
        assert not (tmp_path / "x.fna").exists()


@pytest.mark.parametrize("keep_flag", ["matched", "unmatched", None])
def test_cli_filter(tmp_path, keep_flag):
    k = 7
    rng = random.Random(3)
    samples = {"one": "".join(">a%d\n%s\n" % (i, dna(rng, 60)) for i in range(6)), "two": "".join(">b%d\n%s\n" % (i, dna(rng, 60)) for i in range(6))}
    for base, data in samples.items():
        (tmp_path / (base + ".fna")).write_text(data)
    one, two = (ref_records(samples[b].encode()) for b in ("one", "two"))
    reads = (">from one\n%s\n>from two\n%s\n  >neither\n%s\n>short\nACG\n>both\n%s\n%s\n" %
             (one[1][1][5:45], two[4][1][:30], dna(rng, 40), one[0][1][:20], two[0][1][:20])).encode()
    (tmp_path / "reads.fa").write_bytes(reads)
    out = tmp_path / "out"
    argv = ["-i", str(tmp_path / "one.fna"), str(tmp_path / "two.fna"), "-k", str(k), "-c", "1", "-skipclean", "-o", str(out),
            "-filter", str(tmp_path / "reads.fa"), "-filter_hits", "2"]
    assert cli.main(argv + (["-filter_keep", keep_flag] if keep_flag else [])) == 0
    word = keep_flag or "unmatched"
    for base, data in samples.items():
        table = table_of(data.encode(), k)
        want = expected(reads, table, k, (1, 2, 0), word == "unmatched")
        path = out / "filter_nucleotide" / ("%s_%s.fna" % (base, word))
        assert path.read_bytes() == want[0] and 0 < sum(want[1]) < 5
        with native.Counter(k, NT) as ctx:
            ctx.count_chunk(data.encode(), 1)
            rows = ctx.screen(path, 1)
            assert len(rows) == sum(want[1]) and all(matched(r, (1, 2, 0)) != (word == "unmatched") for r in rows.tolist())
    assert sorted(p.name for p in (out / "filter_nucleotide").iterdir()) == ["one_%s.fna" % word, "two_%s.fna" % word]
    assert not (out / "filter_protein").exists()
