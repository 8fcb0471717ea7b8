"""Texts that put every construct of the input language on every seam of the text kernels, and plain restatements
to compare with.  A helper module (like setop_rule.py): nothing here touches the library or a GPU.

The text kernels cut their input into fixed units and carry a small state from one unit to the next:

    kernel group      unit sizes (bytes)                      scan
    fast parser       16 / 1024 / 8192 (FP_SUB * 1024) / 32768   1024 threads, entries read in batches of 8
    general parser    32 (PB) / 2048 / 8192 (PTILE)              1024 threads
    FASTQ pre-pass    16 / 1024 / 4096 (FQ_TILE)                 1024 threads, apply grid at most 2048 tiles
    clean passes      16                                         grid cap 4096 x 256 x 16

tests/test_text_edges_host.py pins this table to the sources and checks that every generator places what it claims;
tests/test_gpu_text_edges.py counts the texts on the GPU."""
import functools
import random
import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "mercat2_amd" / "csrc"

FAST_UNITS = (16, 1024, 8192, 32768)      # lane, 64 lanes, wave (FP_SUB sub-steps), workgroup
GENERAL_UNITS = (32, 2048, 8192)          # thread, wave, tile
FASTQ_UNITS = (16, 1024, 4096)            # lane, wave, tile
CLEAN_UNITS = (16,)
SCAN_THREADS = 1024                       # one workgroup stitches the units: more units than this -> several per thread
FASTQ_APPLY_GRID = 2048
FAST_WAVE = FAST_UNITS[2]


def source_defines() -> dict:
    """The macros of the .hip sources that the unit table follows from."""
    out = {}
    for fname, names in (("mk_fparse.hip", ("FP_SUB", "FP_THREADS")), ("mk_parse.hip", ("PT", "PB")),
                         ("mk_fastq.hip", ("FQ_TILE", "FQ_THREADS"))):
        text = (CSRC / fname).read_text()
        for name in names:
            found = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)u?\s" % name, text, flags=re.M)
            assert len(found) == 1, (fname, name, found)
            out[name] = int(found[0])
    return out


# ----------------------------------------------------------------------------- building blocks
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SEP = 0  # what parse_stream() writes where a header line starts (the value never enters a comparison with the GPU)

FEATURES = {
    "lf": b"\n",
    "crlf": b"\r\n",
    "cr": b"\r",
    "lf3": b"\n\n\n",
    "header": b"\n>h x\n",                    # a header line that starts at the seam (shift -1)
    "header_quirky": b"\n>a >b *c\td\n",      # a header line holding '>', '*' and blanks
    # a line start matters only to a '>': the one byte whose meaning hangs on "the previous byte was CR" is the '>' behind it
    "cr_header": b"\r>h x\r",                 # shift -1: CR the last byte of a unit, '>' the first of the next
    "crlf_header": b"\r\n>h x\r\n",           # shift -1: CR the last byte, LF the first; shift -2: '>' the first
    "gt_inner": b">",                         # '>' inside a sequence line
    "star": b"*",
    "N": b"N",
    "lower": b"a",
}
BYREF_FEATURES = ("gt_inner", "N", "lower")   # kept characters outside ACGT: the windows over them go by reference
SHIFTS = (-17, -16, -15, -2, -1, 0, 1, 2, 15, 16, 17)
SWEEP_TOTAL = 96 * 1024 + 40


def bases(n: int, seed: int) -> bytes:
    return _ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def base_text(total: int, seed: int = 0, header_every: int = 7) -> bytes:
    """Random ACGT with a line end every 61 bytes; every 7th line starts with '>rNNN' (and is a header line)."""
    out = _ACGT[np.random.default_rng(seed).integers(0, 4, total)].copy()
    out[60::61] = 10
    for line in range(0, total // 61 + 1, header_every):
        head = b">r%03d" % (line // 7 % 1000)
        at = 61 * line
        take = min(len(head), total - at)
        out[at:at + take] = np.frombuffer(head[:take], dtype=np.uint8)
    return out.tobytes()


def plant_positions(flen: int, shift: int, unit: int, total: int, first: int = 0) -> list:
    """Where planted() writes a feature of flen bytes: B + shift for every multiple B of unit from `first` on and below
    total (where it fits)."""
    return [b + shift for b in range(first, total, unit) if b + shift >= 0 and b + shift + flen <= total]


def plant(text: bytes, feature: bytes, shift: int, unit: int, first: int = 0) -> bytes:
    out = bytearray(text)
    for at in plant_positions(len(feature), shift, unit, len(text), first):
        out[at:at + len(feature)] = feature
    return bytes(out)


def planted(feature: str, shift: int, unit: int, total: int = SWEEP_TOTAL, seed: int = 0) -> bytes:
    return plant(base_text(total, seed), FEATURES[feature], shift, unit)


INNER_BLANK_AT = 91  # the middle of base_text()'s first sequence line (bytes 61..120); no sweep plants there


def with_inner_blank(text: bytes, at: int = INNER_BLANK_AT) -> bytes:
    """The same text with ONE blank inside a sequence line: the fast parser hands the chunk to the general one."""
    assert all(text[j] in b"ACGT" for j in (at - 1, at, at + 1)), at
    return text[:at] + b" " + text[at + 1:]


def records(nbytes: int, seed: int) -> bytes:
    """At least nbytes of ordinary irregular records: lengths 0..300, wrapped at 70, some headers with a description."""
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < nbytes:
        n = rng.randrange(0, 300)
        seq = bases(n, seed * 100003 + i)
        rec = (b">q%d some text\n" % i if rng.random() < 0.5 else b">q%d\n" % i) + b"".join(seq[j:j + 70] + b"\n" for j in range(0, n, 70))
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)


def header_filler(n: int) -> bytes:
    """n bytes of header text: blanks, '>', '*', 'N' and lower case, which mean nothing inside a header line."""
    unit = b"hdr text > with *stars*\tand N "
    return (unit * (n // len(unit) + 1))[:n]


# ----------------------------------------------------------------------------- the parsed stream, restated
def _line_classes(text: bytes):
    """Per byte: is a line end, starts a header line, lies in a header line, is a blank outside header lines."""
    b = np.frombuffer(text, dtype=np.uint8)
    nl = (b == 10) | (b == 13)
    line_start = np.empty(b.size, dtype=bool)
    line_start[:1] = True
    line_start[1:] = nl[:-1]
    hstart = line_start & (b == ord(">"))
    last = np.maximum.accumulate(np.where(nl | hstart, np.arange(b.size), -1))  # the last line end or header start at or before i
    in_header = (last >= 0) & hstart[np.maximum(last, 0)]
    return b, nl, hstart, in_header, (b <= 0x20) & ~nl & ~in_header


def takes_general_parser(text: bytes) -> bool:
    """Does the text hold a blank (a byte <= 0x20 that ends no line) outside header lines?  The fast parser then hands
    the chunk to the general one: parse_retries counts 1 for it."""
    return bool(len(text)) and bool(np.any(_line_classes(text)[4]))


def parse_stream(text: bytes):
    """(stream, kept) for a text WITHOUT blanks in sequence lines: what the parsers emit -- every byte outside header
    lines that is no line end and no '*', and one SEP where a header line starts -- and the mask of the bytes kept."""
    if not text:
        return b"", np.zeros(0, dtype=bool)
    b, nl, hstart, in_header, blank = _line_classes(text)
    assert not np.any(blank), "parse_stream is for texts without blanks in sequence lines"
    kept = (~in_header & ~nl & (b != ord("*"))) | hstart
    return np.where(hstart, SEP, b)[kept].astype(np.uint8).tobytes(), kept


def emitted_per_unit(text: bytes, unit: int) -> list:
    """Bytes of the parsed stream that come from each unit-sized piece of the text."""
    _, kept = parse_stream(text)
    return np.add.reduceat(kept.astype(np.int64), np.arange(0, len(text), unit)).tolist()


# ----------------------------------------------------------------------------- output-side seams of the emit pass
RESIDUES_R = tuple(range(64))
RESIDUES_E = (0, 1, 15, 16, 17, 63, 64, 65)
_RES_BODY = 5000


def residue_text(r: int, e: int) -> bytes:
    """Wave 1 (the first 8 KiB) emits a constant + r bytes; a header line that begins inside it runs through wave 2,
    which emits nothing; wave 3 emits exactly e bytes (the end of that header line, e - 1 bases, a header that runs into
    wave 4; e = 0: the first header line covers wave 3 as well).  So the output offset at the end of a wave walks
    through every residue mod 64, waves emit 0 bytes and fewer than 16, and a packed word is shared by three waves."""
    first = b">h\n" + bases(r, 1000 + r) + b"\n" + _res_body()
    assert len(first) < FAST_WAVE - 100
    close = 3 * FAST_WAVE + 40 if e == 0 else 2 * FAST_WAVE + 100  # where the long header line ends
    text = first + b">" + header_filler(close - len(first) - 1) + b"\n"
    if e:
        text += bases(e - 1, 2000 + e) + b"\n"
        text += b">" + header_filler(3 * FAST_WAVE + 40 - len(text) - 1) + b"\n"
    text += _res_tail()
    assert len(text) < 40 * 1024
    return text


@functools.lru_cache(maxsize=None)
def _res_body() -> bytes:
    return records(_RES_BODY, 5)


@functools.lru_cache(maxsize=None)
def _res_tail() -> bytes:
    return records(2000, 6)


# ----------------------------------------------------------------------------- every byte value
ALL_BYTES = tuple(v for v in range(0x21, 0x7F) if v not in (ord(">"), ord("*")))
_RUN = 40  # longer than every k the byte-value tests count with


def all_bytes_text(inner_blank: bool = False) -> bytes:
    """Every byte 0x21..0x7E except '>' and '*' in a sequence line: once between ACGT runs longer than k, once as the
    first and once as the last byte of a line.  inner_blank: one blank inside the first sequence line."""
    out = []
    for i, v in enumerate(ALL_BYTES):
        ch = bytes([v])
        run = [bases(_RUN, 7000 + 4 * i + j) for j in range(4)]
        out.append(b">b%02x\n" % v + run[0] + ch + run[1] + b"\n" + ch + run[2] + b"\n" + run[3] + ch + b"\n")
    text = b"".join(out)
    if inner_blank:
        at = text.index(b"\n") + 1 + _RUN // 2
        text = with_inner_blank(text, at)
    return text


# ----------------------------------------------------------------------------- where the text ends
END_TAILS = {"seq": b"\nGATTACAGATC", "seq_nl": b"\nGATTACAGAT\n", "header": b"\n>tail of it"}


def end_texts(seams=FAST_UNITS) -> dict:
    """Texts of seam + s bytes, s = -1, 0, 1, that end in a sequence line without and with a final newline, and in a
    header line."""
    out = {}
    for seam in seams:
        for s in (-1, 0, 1):
            total = seam + s
            for name, tail in END_TAILS.items():
                out["%d:%+d:%s" % (seam, s, name)] = base_text(total - len(tail), seam) + tail
    return out


# ----------------------------------------------------------------------------- blank runs (general parser)
BLANK_RUNS = (1, 31, 32, 33, 4096)
BLANK_AFTER = ("base", "eol", "eof")


def blank_seam(unit: int) -> int:
    """The first multiple of unit with room for half the longest run and a line start in front of it."""
    room = BLANK_RUNS[-1] // 2 + 200
    return (room + unit - 1) // unit * unit


def blank_run_start(run: int, unit: int) -> int:
    return blank_seam(unit) - (run + 1) // 2


def blank_run_text(run: int, unit: int, after: str) -> bytes:
    """A run of blanks inside a sequence line that crosses a multiple of unit (a run of 1 is the last byte in front of
    it), followed by a base (the run is kept), by the line end (it is trimmed) or by the end of the text."""
    start = blank_run_start(run, unit)
    pre = base_text(start - 30, run)[:-1] + b"\n" + bases(30, run + 1)
    blanks = (b" \t" * (run // 2 + 1))[:run]
    text = pre + blanks
    if after == "base":
        text += bases(40, run + 2) + b"\n" + records(300, run)
    elif after == "eol":
        text += b"\n" + records(300, run)
    else:
        assert after == "eof"
    return text


# ----------------------------------------------------------------------------- long header lines, many units
def _digits(out, at, numbers, width):
    for d in range(width):
        out[at + d] = 48 + (numbers // 10 ** (width - 1 - d)) % 10


def irregular_fasta(total: int, seed: int) -> np.ndarray:
    """About total bytes of records '>rNNNNNNN' with one sequence line of 0..400 bases read from a 100 kbp genome (so the
    table stays small); 10 % of the records end their lines with CRLF; '*' and 'N' over 0.2 % of the bases."""
    rng = np.random.default_rng(seed)
    genome = _ACGT[rng.integers(0, 4, 100_000)]
    nrec = total // 200 + 16
    length = rng.integers(0, 401, nrec)
    nlen = np.where(rng.random(nrec) < 0.1, 2, 1)
    rec_len = 9 + nlen + length + nlen
    start = np.concatenate(([0], np.cumsum(rec_len)[:-1]))
    out = np.full(int(rec_len.sum()), 10, dtype=np.uint8)
    out[start] = ord(">")
    out[start + 1] = ord("r")
    _digits(out, start + 2, np.arange(nrec), 7)
    crlf = nlen == 2
    out[start[crlf] + 9] = 13
    out[(start + 9 + nlen + length)[crlf]] = 13
    ramp = np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length)
    out[np.repeat(start + 9 + nlen, length) + ramp] = genome[np.repeat(rng.integers(0, genome.size - 400, nrec), length) + ramp]
    odd = rng.integers(0, out.size, out.size // 500)
    odd = odd[np.isin(out[odd], _ACGT)]
    out[odd] = np.where(rng.random(odd.size) < 0.5, ord("*"), ord("N")).astype(np.uint8)
    return out


def plant_header(out: np.ndarray, a: int, b: int):
    """Bytes [a, b) become a line end, a header line and its line end."""
    out[a] = 10
    out[a + 1] = ord(">")
    out[a + 2:b - 1] = np.frombuffer(header_filler(b - a - 3), dtype=np.uint8)
    out[b - 1] = 10


def late_inner_blank(out: np.ndarray, near: int) -> int:
    """One blank over a base between two bases, at the first such place from `near` on; returns where."""
    ok = np.isin(out[near - 1:near + 4096], _ACGT)
    at = near + int(np.flatnonzero(ok[:-2] & ok[1:-1] & ok[2:])[0])
    out[at] = 32
    return at


KIB, MIB = 1024, 1024 * 1024
CARRY_540K = ((500 * KIB, 530 * KIB),)  # waves 62..66 of 68: the carry crosses the scan's first ballot word while set
CARRY_9M = ((MIB - 24 * KIB, MIB + 24 * KIB),           # a ballot-word crossing with two waves per scan thread
            (1945 * KIB + 7, 1945 * KIB + 7 + 1229 * KIB),  # set through the whole ballot word of threads 128..191
            (5 * MIB + 300 * KIB + 3000, 5 * MIB + 320 * KIB + 3000))


@functools.lru_cache(maxsize=None)
def long_carry_texts() -> dict:
    """name -> (text, parse_retries a context counts it with, the planted header lines as (a, b) byte ranges)."""
    small = irregular_fasta(540 * KIB, 21)[:540 * KIB].copy()
    for a, b in CARRY_540K:
        plant_header(small, a, b)
    big = irregular_fasta(9 * MIB, 22)[:9 * MIB].copy()
    for a, b in CARRY_9M:
        plant_header(big, a, b)
    small_b, big_b = small.copy(), big.copy()
    late_inner_blank(small_b, 535 * KIB)
    late_inner_blank(big_b, 8 * MIB + 700 * KIB)
    return {"540k-fast": (small.tobytes(), 0, CARRY_540K), "540k-general": (small_b.tobytes(), 1, CARRY_540K),
            "9m-fast": (big.tobytes(), 0, CARRY_9M), "9m-general": (big_b.tobytes(), 1, CARRY_9M)}


# ----------------------------------------------------------------------------- FASTQ
def fq_ref(raw: bytes):
    """(text, stats) of `sed -n '1~4s/^@/>/p;2~4p'` read back with universal newlines, restated: lines split on '\\n' and
    numbered from 1; line 4i+1 is kept with '@' -> '>' if it starts with '@' and dropped otherwise, line 4i+2 is kept;
    stats are the lines, the reads (kept headers), the dropped headers, the length of the text and the CRLF pairs of the
    kept lines."""
    lines = raw.split(b"\n")
    closed = lines[-1] == b""  # the text ends in '\n' (or is empty): no line follows
    if closed:
        lines.pop()
    out, reads, dropped, crlf = [], 0, 0, 0
    for i, line in enumerate(lines):
        whole = line + b"\n" if closed or i < len(lines) - 1 else line
        if i % 4 == 0:
            if not line.startswith(b"@"):
                dropped += 1
                continue
            reads += 1
            whole = b">" + whole[1:]
        elif i % 4 != 1:
            continue
        crlf += whole.count(b"\r\n")
        out.append(whole.replace(b"\r\n", b"\n").replace(b"\r", b"\n"))
    text = b"".join(out)
    return text, {"lines": len(lines), "reads": reads, "headers_dropped": dropped, "fasta_bytes": len(text), "crlf": crlf}


_QUAL = b"I#5F@>+I5#FI"
FQ_TILE = FASTQ_UNITS[2]
FQ_SWEEP_TOTAL = 10 * FQ_TILE + 40


def fastq_record(i: int, n: int, seed: int, nl: bytes = b"\n", head: bytes = None, plus: bytes = b"+") -> bytes:
    rng = np.random.default_rng(seed * 7919 + i)
    qual = np.frombuffer(_QUAL, dtype=np.uint8)[rng.integers(0, len(_QUAL), n)].tobytes()
    return (b"@q%d d" % i if head is None else head) + nl + bases(n, seed * 104729 + i) + nl + plus + nl + qual + nl


def fastq_records(nbytes: int, seed: int, at_least: bool = True) -> bytes:
    """Whole irregular FASTQ records (0..200 bases, 10 % CRLF, '+' lines with and without a name): the first that reach
    nbytes, or (at_least = False) the last that stay below."""
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < nbytes:
        rec = fastq_record(i, rng.randrange(0, 200), seed, b"\r\n" if rng.random() < 0.1 else b"\n",
                           plus=b"+q%d" % i if rng.random() < 0.3 else b"+")
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out if at_least else out[:-1])


def fastq_base(total: int, seed: int) -> bytes:
    """Irregular FASTQ records cut at total bytes."""
    return fastq_records(total, seed)[:total]


def fastq_planted(feature: str, shift: int, unit: int = FQ_TILE, total: int = FQ_SWEEP_TOTAL, seed: int = 3) -> bytes:
    return plant(fastq_base(total, seed), FEATURES[feature], shift, unit)


def _fastq_until(target: int, seed: int, last_line: int = 3, nl: bytes = b"\n") -> bytes:
    """Whole records, the last of which ends its line number last_line (0 header .. 3 quality) exactly at byte `target`
    (with nl as its line end) and carries on behind it."""
    text = fastq_records(target - 400, seed, at_least=False)
    rec = fastq_record(9999, 100, seed, nl, head=b"@q9999 ")
    ends, at = [], 0
    for _ in range(4):
        at = rec.index(b"\n", at) + 1
        ends.append(at)
    pad = target - len(text) - ends[last_line]       # make the header line that much longer
    assert pad >= 0
    return text + fastq_record(9999, 100, seed, nl, head=b"@q9999 " + b"x" * pad)


FASTQ_NAMES = ("at-first-in-tile", "crlf-split-header", "crlf-split-sequence", "crlf-split-plus", "crlf-split-quality",
               "long-header-without-at", "long-sequence", "long-plus", "long-quality-with-at", "extra-lines", "missing-lines")


@functools.lru_cache(maxsize=None)
def fastq_texts() -> dict:
    """The named FASTQ cases (FASTQ_NAMES); each value is a whole FASTQ text."""
    t = FQ_TILE
    out = {}
    # '@' as the first byte of a tile after a tile ending in '\n'
    out["at-first-in-tile"] = _fastq_until(t, 11, 3) + fastq_records(3000, 12)
    # CR as the last byte of a tile, LF the first of the next: on kept lines (header, sequence) and dropped ones
    for name, line in (("crlf-split-header", 0), ("crlf-split-sequence", 1), ("crlf-split-plus", 2), ("crlf-split-quality", 3)):
        out[name] = _fastq_until(t + 1, 13 + line, line, b"\r\n") + fastq_records(3000, 14)
    # lines of 20 KiB of each kind
    n = 20 * KIB
    long_seq, long_qual = bases(n, 31), (b"@" + _QUAL * (n // len(_QUAL) + 1))[:n]
    pre, post = fastq_records(1500, 15), fastq_records(6000, 16)
    out["long-header-without-at"] = pre + b"q " + header_filler(n) + b"\n" + b"ACGTTGCATTGACC\n+\nIIIIIIIIIIIIII\n" + post
    out["long-sequence"] = pre + b"@long\n" + long_seq + b"\n+\n" + long_qual + b"\n" + post
    out["long-plus"] = pre + b"@long\nACGTTGCATTGACC\n+" + header_filler(n) + b"\nIIIIIIIIIIIIII\n" + post
    out["long-quality-with-at"] = pre + b"@long\n" + long_seq[:n // 2] + b"\n+\n" + long_qual + b"\n" + post
    # missing and extra lines: the phase drifts through all four values
    parts = [fastq_records(2500, 40 + i) for i in range(6)]
    out["extra-lines"] = parts[0] + b"\n" + parts[1] + b"extra\n" + parts[2] + b"@extra\n" + parts[3] + b"\n" + parts[4]
    missing = [p.split(b"\n")[:-1] for p in parts]
    for i, drop in enumerate((0, 1, 2, 3, 1, 2)):
        del missing[i][4 * 3 + drop]
    out["missing-lines"] = b"".join(ln + b"\n" for m in missing for ln in m)
    return out


@functools.lru_cache(maxsize=None)
def fastq_big(total: int = 9 * MIB, seed: int = 51) -> bytes:
    """About 9 MiB of irregular FASTQ (0..300 bases; sequences and qualities read from short genomes, so the table stays
    small): more than 1024 tiles (the scan's threads take several each) and more than 2048 (the apply pass's workgroups
    take a second tile).  Five blocks; the lines between them shift the line number through every phase, and three of
    them are 20 KiB long -- tiles without a line end, whose class the scan carries from entry to entry of one thread: a
    line 4i+1 with '@' (kept), a line 4i+2 (kept), a line 4i+1 without '@' (dropped)."""
    rng = np.random.default_rng(seed)
    genome = _ACGT[rng.integers(0, 4, 100_000)]
    qgenome = np.frombuffer(_QUAL, dtype=np.uint8)[rng.integers(0, len(_QUAL), 50_000)]
    blocks = []
    for blk in range(5):
        nrec = total // 5 // 314 + 1
        length = rng.integers(0, 301, nrec)
        rec_len = 14 + 2 * length
        start = np.concatenate(([0], np.cumsum(rec_len)[:-1]))
        out = np.full(int(rec_len.sum()), 10, dtype=np.uint8)
        out[start] = ord("@")
        out[start + 1] = ord("r")
        _digits(out, start + 2, np.arange(nrec) + blk * nrec, 7)
        ramp = np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length)
        out[np.repeat(start + 10, length) + ramp] = genome[np.repeat(rng.integers(0, genome.size - 300, nrec), length) + ramp]
        out[start + 11 + length] = ord("+")
        out[np.repeat(start + 13 + length, length) + ramp] = qgenome[np.repeat(rng.integers(0, qgenome.size - 300, nrec), length) + ramp]
        blocks.append(out.tobytes())
    long = genome[:20 * KIB].tobytes()
    return b"".join((blocks[0], FASTQ_BIG_JOINS[0] % long, blocks[1], FASTQ_BIG_JOINS[1] % long, blocks[2],
                     FASTQ_BIG_JOINS[2] % long, blocks[3], FASTQ_BIG_JOINS[3], blocks[4]))


# between the blocks (each block is whole records): phase 0 -> 1 -> 2 -> 1 -> 0
FASTQ_BIG_JOINS = (b"@%s\n", b"%s\n", b"\n\nq%s\n", b"\n\n\n")


# ----------------------------------------------------------------------------- clean mode
CLEAN_RUNS = (1, 2, 40)
CLEAN_RESIDUES = (15, 0, 1)
CLEAN_FEATURES = {"N": b"N", "NN": b"NN", "N40": b"N" * 40}
CLEAN_SHIFTS = (-1, 0, 1, 16)
CLEAN_TOTAL = 24 * KIB + 40


def clean_runs_text() -> bytes:
    """One record whose N runs of 1, 2 and 40 bytes start, and others end, at offsets = 15, 0, 1 mod 16 of the parsed
    stream (the separator of the record is offset 0, its j-th base offset 1 + j), wrapped at 70 with CRLF on some lines;
    then records with lower case, runs across line ends, a leading and a trailing run, and a record of N alone."""
    seq = bytearray(bases(16 * 10 * 20, 61))
    slot = 0
    for run in CLEAN_RUNS:
        for res in CLEAN_RESIDUES:
            for at_end in (False, True):
                off = 160 * (slot + 1) + res - (run if at_end else 0)  # stream offset of the run's first byte
                seq[off - 1:off - 1 + run] = b"N" * run
                slot += 1
    lines = [bytes(seq[j:j + 70]) for j in range(0, len(seq), 70)]
    first = b">c runs at stream offsets\n" + b"".join(ln + (b"\r\n" if i % 5 == 4 else b"\n") for i, ln in enumerate(lines))
    rest = (b">d lower case\nacgtnnacgtNNacgtACGTNacgtacgtacgtacgtnACGT\n"
            b">e across line ends\n" + bases(50, 62) + b"NNN\nNN" + bases(33, 63) + b"\nN\n" + bases(40, 64) + b"N\n"
            b">f leading and trailing\nNNN" + bases(77, 65) + b"NNNNN\n>g only N\nNNNNNNNNNNNNNNNNNNNN\n>h empty\n"
            b">i plain\n" + bases(64, 66) + b"\n" + bases(11, 67) + b"\n")
    return first + rest


CLEAN_UNIT = 1024       # the planted runs sit around the multiples of 1 KiB from the first on: line 0, the text's only
CLEAN_NAMES = ("runs",) + tuple("%s%+d" % (name, shift) for name in CLEAN_FEATURES for shift in CLEAN_SHIFTS)  # header line, stays


@functools.lru_cache(maxsize=None)
def clean_texts() -> dict:
    """Texts for clean mode (CLEAN_NAMES): within what the GPU mode accepts (no blanks in sequence lines, no inner '>',
    no 0x7F).  The planted ones are ONE record: a header line, then 24 KiB of sequence lines with a run at every 1 KiB."""
    out = {"runs": clean_runs_text()}
    for name, feat in CLEAN_FEATURES.items():
        for shift in CLEAN_SHIFTS:
            out["%s%+d" % (name, shift)] = plant(base_text(CLEAN_TOTAL, 71, header_every=1 << 30), feat, shift, CLEAN_UNIT, first=CLEAN_UNIT)
    return out


def stream_runs(stream: bytes) -> list:
    """(start, end) of every run of 'N' in a parsed stream."""
    return [(m.start(), m.end()) for m in re.finditer(rb"N+", stream)]
