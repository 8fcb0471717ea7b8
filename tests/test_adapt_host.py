"""mk_fastq_adapt_* without a GPU: the rule of tests/adapt_rule.py on hand examples whose answers are written out, the
panel packer read back through the layout include/mercat_hip.h documents, the adapter reader, the header, the bindings,
the report writers and the command line's refusals."""
import ctypes as C
import gzip
import inspect
import re

import numpy as np
import pytest

import adapt_rule as rule
from conftest import GOLDEN, ROOT
from mercat2_amd import cli, kmers, native, report

HEADER = (ROOT / "include" / "mercat_hip.h").read_text()
TRU = b"AGATCGGAAGAGC"  # 13 bases: 10 % of them is one mismatch
NO = rule.NO_HIT
ARG, RANGE = -1, -7


def fq(*seqs, nl=b"\n"):
    return b"".join(b"@r%d" % i + nl + s + nl + b"+" + nl + b"I" * len(s) + nl for i, s in enumerate(seqs))


def rows_of(seqs, adapters, mates=None, **kw):
    return rule.run(fq(*seqs), adapters, mates, **kw)["rows"]


# ---------------------------------------------------------------------------------------------------- the rule
def test_hand_examples_of_the_hit():
    t6 = b"T" * 6
    assert rows_of([t6 + TRU + b"TT"], [TRU]) == [(21, 6, 0, 13, 0)]                       # internal, whole adapter
    assert rows_of([t6 + TRU], [TRU]) == [(19, 6, 0, 13, 0)]                                # the adapter ends the read
    assert rows_of([b"T" * 8 + TRU[:10]], [TRU]) == [(18, 8, 0, 10, 0)]                     # it runs off the end: overlap 10
    assert rows_of([b"T" * 8 + TRU[:8]], [TRU]) == [(16, 8, 0, 8, 0)]                       # overlap exactly min_overlap
    assert rows_of([b"T" * 8 + TRU[:7]], [TRU]) == [(15, 15, NO, 0, 0)]                     # one base fewer: no hit
    assert rows_of([b"T" * 8 + TRU[:7]], [TRU], min_overlap=7) == [(15, 8, 0, 7, 0)]
    assert rows_of([TRU + b"TTTT"], [TRU]) == [(17, 0, 0, 13, 0)]                           # at 0: nothing is kept
    assert rows_of([b"", b"T", TRU[:7]], [TRU]) == [(0, 0, NO, 0, 0), (1, 1, NO, 0, 0), (7, 7, NO, 0, 0)]
    assert rows_of([TRU[:7]], [TRU[:7]], min_overlap=7) == [(7, 0, 0, 7, 0)]
    # an adapter shorter than min_overlap is never admissible
    assert rows_of([t6 + b"ACGTACG" + t6], [b"ACGTACG"]) == [(19, 19, NO, 0, 0)]


def test_hand_examples_of_the_mismatches():
    t6 = b"T" * 6
    one, two = b"AGATCGGTAGAGC", b"AGTTCGGTAGAGC"   # TRU with base 7, and bases 2 and 7, replaced
    assert rows_of([t6 + one + b"TT"], [TRU]) == [(21, 6, 0, 13, 1)]          # 1 * 10^6 <= 100000 * 13
    assert rows_of([t6 + two + b"TT"], [TRU]) == [(21, 21, NO, 0, 0)]         # 2 * 10^6 > 1300000
    assert rows_of([t6 + two + b"TT"], [TRU], max_err_ppm=153847) == [(21, 6, 0, 13, 2)]   # 2 * 10^6 <= 153847 * 13 = 2000011
    assert rows_of([t6 + two + b"TT"], [TRU], max_err_ppm=153846) == [(21, 21, NO, 0, 0)]  # 153846 * 13 = 1999998
    assert rows_of([t6 + one + b"TT"], [TRU], max_err_ppm=0) == [(21, 21, NO, 0, 0)]
    # the overlap, not the adapter, sets the budget: 9 of 13 bases admit no mismatch at 10 %, 10 admit one
    assert rows_of([b"T" * 8 + b"AGATCGGTA"], [TRU]) == [(17, 17, NO, 0, 0)]
    assert rows_of([b"T" * 8 + b"AGATCGGTAG"], [TRU]) == [(18, 8, 0, 10, 1)]
    # a read N mismatches, an adapter N is free, and both fold
    assert rows_of([t6 + b"AGATCGGNAGAGC"], [TRU]) == [(19, 6, 0, 13, 1)]
    assert rows_of([t6 + b"AGATCGGNAGAGC"], [TRU], max_err_ppm=0) == [(19, 19, NO, 0, 0)]
    assert rows_of([t6 + b"AGATCGGNAGAGC", t6 + one, t6 + b"AGATCGG.AGAGC"], [b"AGATCGGNAGAGC"], max_err_ppm=0) == [
        (19, 6, 0, 13, 0), (19, 6, 0, 13, 0), (19, 6, 0, 13, 0)]
    assert rows_of([b"tttttt" + TRU.lower() + b"tt"], [TRU], max_err_ppm=0) == [(21, 6, 0, 13, 0)]
    assert rows_of([t6 + TRU], [b"agatcggaagagc"], max_err_ppm=0) == [(19, 6, 0, 13, 0)]
    # only X and X | 0x20 fold to X: '!' (0x21) and 0xC1 share 'A''s low bits and are no A
    assert rows_of([t6 + b"!GATCGGAAGAGC"], [TRU], max_err_ppm=0) == [(19, 19, NO, 0, 0)]
    assert rows_of([t6 + bytes([ord("A") | 0x80]) + TRU[1:]], [TRU], max_err_ppm=0) == [(19, 19, NO, 0, 0)]


def test_hand_examples_of_the_choice():
    long_, c8 = TRU + b"ACAC", b"C" * 8
    read = b"T" * 5 + long_
    assert rows_of([read], [long_, TRU]) == [(22, 5, 0, 17, 0)]       # both admissible at 5: the lower index
    assert rows_of([read], [TRU, long_]) == [(22, 5, 0, 13, 0)]
    assert rows_of([read], [TRU, TRU, long_]) == [(22, 5, 0, 13, 0)]  # duplicates: the lowest
    # the leftmost position wins over the lower index
    far = b"T" * 10 + TRU + b"T" * 17 + c8
    assert rows_of([far], [c8, TRU]) == [(48, 10, 1, 13, 0)]
    assert rows_of([far], [c8, b"GGGGGGGG"]) == [(48, 40, 0, 8, 0)]
    got = rule.run(fq(far, read, b"T" * 30), [c8, TRU, long_])
    assert got["hits"] == [0, 2, 0] and got["keep"] == [1, 1, 1]


def test_classes_pairs_and_the_bytes_that_come_out():
    cut, clean = b"T" * 6 + TRU, b"T" * 19
    text = fq(cut, cut, clean, cut, TRU + b"T", clean, TRU, TRU)
    # a class-2 adapter never cuts a first mate; class 3 cuts both; unpaired every read is of class 1
    two = rule.run(text, [TRU], [2], paired=1)
    assert [r[1] for r in two["rows"]] == [19, 6, 19, 6, 14, 19, 13, 0] and two["hits"] == [3]
    assert two["keep"] == [1, 1, 1, 1, 1, 1, 2, 0] and two["figures"]["orphans"] == 1 and two["figures"]["dropped_short"] == 1
    both = rule.run(text, [TRU], [3], paired=1)
    assert [r[1] for r in both["rows"]] == [6, 6, 19, 6, 0, 19, 0, 0] and both["keep"] == [1, 1, 1, 1, 0, 2, 0, 0]
    assert rule.run(text, [TRU], [2])["hits"] == [0] and rule.run(text, [TRU], [1])["hits"] == [6]
    orphans = rule.run(text, [TRU], [3], paired=1, which=2)
    recs = [b"".join(r) for r in rule.records(text)[0]]
    assert orphans["out"] == recs[5] and orphans["keep"] == both["keep"]
    assert both["out"] == b"@r0\nTTTTTT\n+\nIIIIII\n" * 1 + b"@r1\nTTTTTT\n+\nIIIIII\n" + recs[2] + b"@r3\nTTTTTT\n+\nIIIIII\n"
    f = both["figures"]
    assert (f["records"], f["records_out"], f["records_trimmed"], f["dropped_short"], f["orphans"], f["bases_in"], f["bases_out"],
            f["bytes_out"], f["lines"]) == (8, 4, 3, 3, 1, 135, 37, len(both["out"]), 32)
    # min_len drops what is shorter; 0 still drops an emptied read
    assert rule.run(text, [TRU], min_len=7)["keep"] == [0, 0, 1, 0, 0, 1, 0, 0]
    assert rule.run(text, [TRU], min_len=6)["keep"] == [1, 1, 1, 1, 0, 1, 0, 0]
    # CR LF: an untouched record byte for byte, a cut one with '\n' behind the cut lines; an open end gets its '\n'
    crlf = b"@a x\r\n" + cut + b"\r\n+a\r\n" + b"I" * 19 + b"\r\n@b\r\n" + clean + b"\r\n+\r\n" + b"J" * 19
    got = rule.run(crlf, [TRU])
    assert got["out"] == b"@a x\r\nTTTTTT\n+a\r\nIIIIII\n@b\r\n" + clean + b"\r\n+\r\n" + b"J" * 19 + b"\n"
    assert got["rows"] == [(19, 6, 0, 13, 0), (19, 19, NO, 0, 0)]


def test_the_rule_refuses_what_the_call_refuses():
    text = fq(b"ACGT" * 5, b"ACGT" * 5, b"ACGT" * 5)
    for kw in (dict(min_overlap=0), dict(min_overlap=129), dict(max_err_ppm=1000001), dict(which=2), dict(which=0), dict(which=3, paired=1)):
        with pytest.raises(rule.AdaptError) as e:
            rule.run(text, [TRU], **kw)
        assert e.value.code == rule.ERR_ARG
    for adapters, mates, named in (([], None, None), ([TRU] * 1025, None, None), ([TRU, b""], None, 1), ([b"A" * 129], None, 0),
                                   ([TRU, TRU, b"ACGU"], None, 2), ([TRU], [0], 0), ([TRU, TRU], [1, 4], 1)):
        with pytest.raises(rule.AdaptError) as e:
            rule.run(text, adapters, mates)
        assert (e.value.code, e.value.adapter) == (rule.ERR_ARG, named)
    with pytest.raises(rule.AdaptError) as e:
        rule.run(text, [TRU], paired=1)
    assert e.value.code == rule.ERR_RANGE
    with pytest.raises(rule.AdaptError) as e:
        rule.run(text, [TRU], cap=2)
    assert e.value.code == rule.ERR_RANGE and e.value.counts == (3, 2)
    for bad, record, kind in ((b">r\nAC\n+\nII\n", 0, "at"), (text + b"@r\nAC\n-\nII\n", 3, "plus"), (text + b"@r\nAC\n+\nIII\n", 3, "length"),
                              (text + b"@r\nAC\n", 3, "incomplete")):
        with pytest.raises(rule.AdaptError) as e:
            rule.run(bad, [TRU])
        assert (e.value.code, e.value.record, e.value.kind) == (rule.ERR_UNSUPPORTED, record, kind)
    assert rule.run(text + b"\n\n\n", [TRU])["out"] == text and rule.run(b"", [TRU])["out"] == b""
    assert rule.run(b"@r\nAC\n+\n !\n", [TRU])["out"] == b"@r\nAC\n+\n !\n"  # qualities are carried, never read


# ------------------------------------------------------------------------------------------ mk_adapters_pack
def raw_pack(seqs, mates=None, A=None, cap=None, words=True):
    """mk_adapters_pack: (rc, words, nwords, message)."""
    bases = np.frombuffer(b"".join(seqs), np.uint8).copy() if seqs else np.zeros(1, np.uint8)
    lengths = np.array([len(s) for s in seqs] or [0], np.uint32)
    A = len(seqs) if A is None else A
    if A > len(seqs):  # (a panel longer than the lists: one base each, so that only the count is wrong)
        bases, lengths = np.full(A, ord("A"), np.uint8), np.ones(A, np.uint32)
    m = None if mates is None else np.array(mates, np.uint8)
    cap = 1 + 9 * max(A, 1) if cap is None else cap
    out = np.full(cap + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
    nwords, err = C.c_size_t(77), C.create_string_buffer(200)
    rc = native.lib().mk_adapters_pack(bases.ctypes.data, lengths.ctypes.data, m.ctypes.data if m is not None else None, A,
                                       out.ctypes.data if words else None, cap if words else 0, C.byref(nwords), err, 200)
    return rc, out, nwords.value, err.value.decode()


def decode(words):
    """[(bases, class, first)] of a packed panel, by the layout the header documents."""
    words = [int(w) for w in words]
    out = []
    for a in range(words[0]):
        w = words[1 + 9 * a: 10 + 9 * a]
        m, cls, first = w[0] & 0xFF, (w[0] >> 8) & 0xFF, w[0] >> 32
        seq = bytearray()
        for j in range(m):
            code = (w[1 + j // 32] >> (2 * (j % 32))) & 3
            care = (w[5 + j // 32] >> (2 * (j % 32))) & 1
            seq.append(b"ACGT"[code] if care else ord("N"))
            assert care or code == 0
        # nothing behind the last base, nothing on the odd bits of the care plane
        for j in range(m, 128):
            assert (w[1 + j // 32] >> (2 * (j % 32))) & 3 == 0 and (w[5 + j // 32] >> (2 * (j % 32))) & 3 == 0
        assert all(c & 0xAAAAAAAAAAAAAAAA == 0 for c in w[5:9])
        out.append((bytes(seq), cls, first))
    return out


def test_the_packed_panel_reads_back():
    rng = np.random.default_rng(1)
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgtn", np.uint8)
    seqs = [bytes(rng.choice(alphabet, n)) for n in (1, 31, 32, 33, 63, 64, 65, 127, 128)]
    seqs[3] = b"N" * 33
    seqs[5] = b"T" * 63 + b"N"   # the last base of a word a wildcard
    mates = [1, 2, 3, 1, 2, 3, 1, 2, 3]
    rc, words, nwords, msg = raw_pack(seqs, mates)
    assert (rc, nwords, msg) == (0, 1 + 9 * 9, "") and (words[nwords:] == 0xA5A5A5A5A5A5A5A5).all()
    assert decode(words) == [(s.upper(), m, a) for a, (s, m) in enumerate(zip(seqs, mates))]
    assert any(b"N" in s.upper() for s in seqs) and any(s != s.upper() for s in seqs)
    # mates NULL: all class 1; the binding gives the same words
    rc, words, nwords, msg = raw_pack(seqs)
    assert rc == 0 and [c for _, c, _ in decode(words)] == [1] * 9
    bases, lengths, m, _ = native.adapter_arrays(seqs)
    assert native.pack_adapters(bases, lengths, m).tolist() == words[:nwords].tolist()
    # first: the lowest index with the same folded bases and the same class
    dup = [b"ACGTN", b"acgtn", b"ACGTA", b"ACGTN", b"ACGT", b"ACGTN"]
    rc, words, nwords, msg = raw_pack(dup, [1, 1, 1, 2, 1, 2])
    assert rc == 0 and [f for _, _, f in decode(words)] == [0, 0, 2, 3, 4, 3]
    # the literal words of one small panel
    rc, words, nwords, msg = raw_pack([b"ACGTN", b"TTTT"], [3, 2])
    assert words[:nwords].tolist() == [2, 0x305, 0xE4, 0, 0, 0, 0x55, 0, 0, 0, (1 << 32) | 0x204, 0xFF, 0, 0, 0, 0x55, 0, 0, 0]


def test_the_packer_sizes_and_refuses():
    rc, words, nwords, msg = raw_pack([TRU, TRU], words=False)
    assert (rc, nwords) == (0, 19)
    rc, words, nwords, msg = raw_pack([TRU, TRU], cap=18)
    assert (rc, nwords) == (RANGE, 19) and "19 words" in msg and (words == 0xA5A5A5A5A5A5A5A5).all()
    for seqs, mates, A, phrase in (([], None, 0, "0 adapters"), ([TRU], None, 1025, "1025 adapters"), ([TRU, b""], None, None, "adapter 1 has 0 bases"),
                                   ([b"A" * 129], None, None, "adapter 0 has 129 bases"), ([TRU, TRU, b"ACGU"], None, None, "adapter 2 holds the byte 0x55 at base 3"),
                                   ([TRU, b"AC-T"], None, None, "adapter 1 holds the byte 0x2D at base 2"), ([TRU], [0], None, "adapter 0 has mate class 0"),
                                   ([TRU, TRU], [1, 4], None, "adapter 1 has mate class 4")):
        rc, words, nwords, msg = raw_pack(seqs, mates, A)
        assert (rc, nwords) == (ARG, 0) and phrase in msg, msg
        assert (words == 0xA5A5A5A5A5A5A5A5).all()
    assert raw_pack([b"A" * 128] * 1024)[0] == 0
    with pytest.raises(native.MercatHipError) as e:
        native.pack_adapters(np.frombuffer(b"ACGX", np.uint8), np.array([4], np.uint32))
    assert e.value.code == ARG and "adapter 0" in str(e.value)


def test_adapter_arrays_merge_the_two_lists():
    bases, lengths, mates, seqs = native.adapter_arrays(["ACGT", b"TTTT", "ACGT"], ["GGGG", "TTTT"])
    assert seqs == ["ACGT", "TTTT", "GGGG"] and mates.tolist() == [1, 3, 2] and lengths.tolist() == [4, 4, 4]
    assert bases.tobytes() == b"ACGTTTTTGGGG" and lengths.dtype == np.uint32 and mates.dtype == np.uint8
    assert native.adapter_arrays(["AC"])[2].tolist() == [1]
    assert dict(native.ILLUMINA_ADAPTERS) == {"TruSeq": "AGATCGGAAGAGC", "Nextera": "CTGTCTCTTATACACATCT", "small_RNA": "TGGAATTCTCGGGTGCCAAGG"}
    with pytest.raises(ValueError):
        native.Counter.fastq_adapt(None, b"", ["ACGT"], adapters2=["ACGT"])  # (before the library or a GPU is touched)


# ------------------------------------------------------------------------------------------------- read_adapters
def test_read_adapters(tmp_path):
    text = b">one first adapter \t\nACGT \nacgt\t\t\n\n>two\r\nNNAC\r\nGT\n>three\nTTTT"
    (tmp_path / "a.fna").write_bytes(text)
    with gzip.open(tmp_path / "a.fna.gz", "wb") as fh:
        fh.write(text)
    for name in ("a.fna", "a.fna.gz"):
        assert native.read_adapters(tmp_path / name) == (["one", "two", "three"], ["ACGTacgt", "NNACGT", "TTTT"])
    (tmp_path / "bad.fna").write_bytes(b">ok\nACGT\n>odd one\nAC\nGU\n")
    with pytest.raises(ValueError) as e:
        native.read_adapters(tmp_path / "bad.fna")
    assert "'odd'" in str(e.value) and "record 1 " in str(e.value) and "0x55" in str(e.value)
    assert native.read_adapters(tmp_path / "bad.fna", check=False)[1] == ["ACGT", "ACGU"]
    (tmp_path / "hollow.fna").write_bytes(b">empty\n>full\nAC\n>last\n")
    assert native.read_adapters(tmp_path / "hollow.fna") == (["full"], ["AC"])
    for raw in (b"", b"ACGT\n>x\nAC\n", b">only a name\n"):
        (tmp_path / "none.fna").write_bytes(raw)
        with pytest.raises(ValueError):
            native.read_adapters(tmp_path / "none.fna")


def test_read_adapters_on_the_reference_panel():
    path = GOLDEN / "adapters" / "adapter.fna"
    names, seqs = native.read_adapters(path, check=False)
    assert len(names) == len(seqs) == 425 and len(set(seqs)) == 376 and max(len(s) for s in seqs) <= 128
    assert names[0] == "Illumina_Single_End_Adapter1" and seqs[0] == "GATCGGAAGAGCTCGTATGCCGTCTTCTGCTTG"
    odd = [(n, s) for n, s in zip(names, seqs) if set(s) - set("ACGTNacgtn")]
    assert odd == [("BC6", "3TTCTGAAGTTCCTGGGTCTTGAAC")]
    with pytest.raises(ValueError) as e:
        native.read_adapters(path)
    assert "'BC6'" in str(e.value) and "0x33" in str(e.value)


# ----------------------------------------------------------------------------------------- header and bindings
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            ctype, rest = stmt.split(" ", 1)
            out += [(ctype, f.strip()) for f in rest.split(",")]
    return out


def test_header_declares_the_calls():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in ("mk_adapters_pack", "mk_fastq_adapt_text", "mk_fastq_adapt_device"):
        assert name in native.ABI_SYMBOLS and getattr(native.lib(), name) is not None
    args = re.search(r"int mk_fastq_adapt_text\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "fastq", "n", "piece_bytes", "bases", "lengths", "mates", "A", "opt", "cap", "keep", "rows", "hits", "out", "out_cap",
        "out_len", "nrec", "st"]
    args = re.search(r"int mk_fastq_adapt_device\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "d_fastq", "n", "bases", "lengths", "mates", "A", "opt", "cap", "d_keep", "d_rows", "d_hits", "d_out", "out_cap", "out_len",
        "nrec", "st"]
    args = re.search(r"int mk_adapters_pack\((.*?)\);", code, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["bases", "lengths", "mates", "A", "words", "words_cap", "nwords", "err",
                                                                   "err_cap"]
    assert len(native.lib().mk_fastq_adapt_text.argtypes) == 18 and len(native.lib().mk_fastq_adapt_device.argtypes) == 17
    assert len(native.lib().mk_adapters_pack.argtypes) == 9
    assert native.lib().mk_version().decode().split()[1].split(".")[0] == str(native.MK_ABI)


def test_bound_structs_match_the_header():
    fields = _struct_fields("mk_adapt_opt_t")
    assert [f for _, f in fields] == ["min_overlap", "max_err_ppm", "min_len", "paired", "which"]
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.AdaptOpt._fields_] and C.sizeof(native.AdaptOpt) == 20
    fields = _struct_fields("mk_fastq_adapt_t")
    assert [f for _, f in fields] == ["records", "records_out", "records_trimmed", "dropped_short", "orphans", "bases_in", "bases_out",
                                      "bytes_out", "lines", "s_copy", "s_index", "s_scan", "s_place", "s_gather", "s_write"]
    assert [(CTYPE[t], f) for t, f in fields] == [(t, f) for f, t in native.FastqAdapt._fields_]
    assert [getattr(native.FastqAdapt, f).offset for _, f in fields] == [8 * i for i in range(15)] and C.sizeof(native.FastqAdapt) == 120


def test_python_layers_are_there():
    assert list(inspect.signature(native.Counter.fastq_adapt).parameters)[1:] == [
        "path_or_bytes", "adapters", "adapters2", "min_overlap", "max_err", "min_len", "paired", "which", "piece_bytes", "info"]
    d = {k: p.default for k, p in inspect.signature(native.Counter.fastq_adapt).parameters.items()}
    assert (d["adapters2"], d["min_overlap"], d["max_err"], d["min_len"], d["paired"], d["which"], d["piece_bytes"], d["info"]) == (
        None, 8, 0.1, 0, False, 1, 0, None)
    assert callable(native.Counter.fastq_adapt_device) and "panel" in native.Counter.fastq_adapt.__doc__
    opt = native.adapt_options(max_err=0.25, paired=True, which=2)
    assert (opt.min_overlap, opt.max_err_ppm, opt.min_len, opt.paired, opt.which) == (8, 250000, 0, 1, 2)
    for bad in (dict(max_err=1.5), dict(min_len=-1), dict(min_overlap=1 << 32)):
        with pytest.raises(ValueError):
            native.adapt_options(**bad)
    names = list(inspect.signature(kmers.adapt_reads).parameters)
    assert names[:4] == ["file", "out_path", "adapters", "adapters2"]
    assert {"min_overlap", "max_err", "min_len", "paired", "tsv_path", "summary_path", "mate_file", "out_path2", "singles_path", "device",
            "keep_text"} <= set(names)
    for bad in (("reads.fna", "out.fastq"), ("reads.fastq", "out.fastq", None, ["ACGT"])):
        with pytest.raises(ValueError):  # (before any call of the library)
            kmers.adapt_reads(*bad)


def test_the_reports():
    got = rule.run(fq(b"T" * 6 + TRU, b"T" * 19, TRU + b"T"), [b"C" * 8, TRU])
    tsv = report.format_adapt_tsv(["r0", "r1", "r2"], got["rows"], got["keep"], ["polyC", "TruSeq"])
    assert tsv == (b"record\tlength\tkept\tadapter\toverlap\tmismatches\tkeep\nr0\t19\t6\tTruSeq\t13\t0\t1\nr1\t19\t19\t-\t0\t0\t1\n"
                   b"r2\t14\t0\tTruSeq\t13\t0\t0\n")
    text = report.format_adapt_summary(got["figures"], got["hits"], ["polyC", "TruSeq"])
    assert text == b"metric\tbefore\tafter\nreads\t3\t2\nbases\t52\t25\ntrimmed\t\t1\ndropped_short\t\t1\norphans\t\t0\nadapter:TruSeq\t\t2\n"
    with pytest.raises(ValueError):
        report.format_adapt_tsv(["r0"], got["rows"], got["keep"], ["polyC", "TruSeq"])


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture()
def files(tmp_path):
    (tmp_path / "s.fna").write_bytes(b">a\nACGTACGTAC\n")
    (tmp_path / "r.fastq").write_bytes(b"@a\nACGTACGTAC\n+\nIIIIIIIIII\n")
    (tmp_path / "panel.fna").write_bytes(b">p1\nACGTACGTAA\n>p2\nTTTTGGGGCC\nAA\n")
    (tmp_path / "bad.fna").write_bytes(b">p1\nACGTACGTAA\n>p2\nTTTTGG-GCC\n")
    (tmp_path / "long.fna").write_bytes(b">p1\n" + b"A" * 129 + b"\n")
    return tmp_path


def parse(files, inputs, *extra):
    return cli.parseargs(list(inputs) + ["-k", "5", "-o", str(files / "out")] + [str(x) for x in extra])[0]


def test_cli_accepts_adapt(files):
    args = parse(files, ["-i", str(files / "r.fastq")], "-adapt")
    assert args.adapt == "" and args.adapters is None and args.adapt_overlap is None and args.qtrim is None
    args = parse(files, ["-i", str(files / "s.fna"), str(files / "r.fastq")], "-adapt", files / "panel.fna", "-adapt_overlap", 5,
                 "-adapt_err", 0.2, "-adapt_len", 30, "-qtrim", "-skipclean")
    assert args.adapters == [("p1", "ACGTACGTAA"), ("p2", "TTTTGGGGCCAA")]
    assert (args.adapt_overlap, args.adapt_err, args.adapt_len, args.qtrim) == (5, 0.2, 30, 20)
    assert parse(files, ["-i", str(files / "r.fastq")]).adapt is None


def test_the_help_says_what_the_default_overlap_is_for(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parseargs(["-h"])
    help_ = " ".join(capsys.readouterr().out.split())
    assert e.value.code == 0 and "-adapt_overlap" in help_ and "panel of hundreds of adapters" in help_ and "not fastp's" in help_


@pytest.mark.parametrize("extra,message", [
    (["-adapt_overlap", 10], "-adapt_overlap needs -adapt"),
    (["-adapt_err", 0.2], "-adapt_err needs -adapt"),
    (["-adapt_len", 10], "-adapt_len needs -adapt"),
    (["-qtrim", "-adapt_len", 10], "-adapt_len needs -adapt"),
    (["-adapt", "-adapt_overlap", 0], "-adapt_overlap 0: must lie in 1..128"),
    (["-adapt", "-adapt_overlap", 129], "-adapt_overlap 129: must lie in 1..128"),
    (["-adapt", "-adapt_err", 1.5], "-adapt_err 1.5: must lie in 0..1"),
    (["-adapt", "-adapt_len", -1], "-adapt_len -1"),
    (["-adapt", "nowhere.fna"], "file 'nowhere.fna' is not valid"),
])
def test_cli_refuses(files, capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], *extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_refuses_a_bad_panel_and_adapt_without_fastq_input(files, capsys):
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], "-adapt", files / "bad.fna")
    assert e.value.code == 2 and "'p2'" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "r.fastq")], "-adapt", files / "long.fna")
    assert e.value.code == 2 and "at most 128 bases" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        parse(files, ["-i", str(files / "s.fna")], "-adapt")
    assert e.value.code == 2 and "no input is a FASTQ file" in capsys.readouterr().err
    assert cli.classify(files / "r.fastq", True) == ("nucleotide", "r")
