"""FASTA texts whose header lines stand on the seams of the record placement (mercat2_amd/csrc/mk_recordplace.h:
fl_tiles_k / fl_scan_k / fl_starts_k) and whose emitted records stand on the seams of the output gathers (fl_gather_k /
fl_edges_k there, tr_gather_k / tr_edges_k and tr_hend_k in mk_trimwalk.h), with plain restatements of where they stand.
A helper module (like walk_seams.py and text_edges.py): nothing here touches the library or a GPU.

    kernel group   unit sizes (bytes)                                               of
    placement      16 (one load) / 32 (a lane, FL_RUN) / 2048 (a wave) / 8192       the RAW text
                   (a workgroup's tile, FL_SPAN); sc_tile_scan: 1024 threads
    gathers        16 (a lane's chunk) / 1024 (a wave's store) / 4096 (a wave)      the OUTPUT
                   / 16384 (a workgroup); the last 32 bytes of a source by bytes

The key control: k = 5 and a table of exactly the 32 5-mers over {A, C}.  A record whose bases are all A or C is matched
(every window a hit), one over {G, T} is unmatched, one with fewer than 5 bases has no windows: what a call keeps, drops
or cuts is chosen record by record, and the smallest record is 2 bytes.  Filter keeps the unmatched records under invert
(as they stand); trim keeps a record's leading run of A / C (five or more) behind its header line.

tests/test_record_seams_host.py checks that every text places what is claimed here; tests/test_gpu_record_place.py runs
them through filter, trim, normalize, correct and the pairs call."""
import functools
import itertools
import random
import re
from pathlib import Path

import filter_rule
import trim_rule

CSRC = Path(__file__).resolve().parent.parent / "mercat2_amd" / "csrc"

K = 5
HIGH = 5                     # the count of every table entry
FILTER_RULE = (1, 1, 0)      # (at_least, min_hits, min_ppm): matched iff one window is a hit
TRIM_AT_LEAST = 2            # HIGH is enough, an absent window is low
UNITS = (16, 32, 2048, 8192)  # one 16-byte load, a lane's run (FL_RUN), a wave, a tile (FL_SPAN) of the raw text
SHIFTS = tuple(range(-3, 4))
OUT_SEAMS = (1024, 4096, 16384)  # a wave's store, a wave, a workgroup of the output (FL_CHUNKS = TR_CHUNKS = 4)
SCAN_THREADS = 1024
BLANKS = b" \t\x0b\x0c\x1c\x1d\x1e\x1f"  # mk_is_blank
OPENING = ("lf", "blank1", "blank2", "blank33", "cr", "crlf")           # a '>' that opens a header line
INERT = ("in_header", "after_base", "after_blanks", "after_star")      # a '>' that opens nothing
FORMS = OPENING + INERT
JUNK = b"=?\xbe>;<x"  # header bytes: what a borrow or carry slip of the SWAR test would take for '>', and '>' itself
LENGTHS = tuple(itertools.chain(range(1, 34), range(47, 50), range(1023, 1026), range(4095, 4098), range(16383, 16386),
                                range(20479, 20482)))
RUNS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 1000)
MODES = ("filter", "trim")
MIN_KEPT = {"filter": 2, "trim": K + 3}  # output bytes of the smallest record a mode keeps: ">\n"; ">\n", K bases, LF
MIN_DROP = {"filter": K + 3, "trim": 2}  # raw bytes of the smallest record a mode drops


def source_defines() -> dict:
    """The macros the unit table follows from."""
    place = (CSRC / "mk_recordplace.h").read_text()
    walk = (CSRC / "mk_trimwalk.h").read_text()
    out = {"FL_RUN": int(re.search(r"^#define FL_RUN (\d+)\s", place, flags=re.M).group(1)),
           "FL_CHUNKS": int(re.search(r"^#define FL_CHUNKS (\d+)\s", place, flags=re.M).group(1)),
           "TR_CHUNKS": int(re.search(r"^#define TR_CHUNKS (\d+)\s", walk, flags=re.M).group(1))}
    assert re.search(r"^#define FL_SPAN \(256 \* FL_RUN\)\s", place, flags=re.M)
    return out


@functools.lru_cache(maxsize=None)
def table() -> dict:
    return {"".join(p): HIGH for p in itertools.product("AC", repeat=K)}


def table_tsv() -> bytes:
    return b"".join(b"%s\t%d\n" % (key.encode(), c) for key, c in table().items())


def _draw(rng, letters: bytes, n: int) -> bytes:
    return bytes(rng.choice(letters) for _ in range(n))


def _junk(rng, n: int) -> bytes:
    return _draw(rng, JUNK, n)


def _blanks(at: int, n: int) -> bytes:
    return bytes(BLANKS[(at + i) % len(BLANKS)] for i in range(n))


# ----------------------------------------------------------------------------- placement
@functools.lru_cache(maxsize=None)
def placement():
    """(text, ((U, d, form, position of the '>'), ...)): for every unit U, every d in SHIFTS and every form a '>' at raw
    byte m * U + d.  Records alternate matched and unmatched from the first to the last, so every start is a kept/dropped
    boundary of the plain and of the inverted output.  The header lines that pad a record to its place carry JUNK, with
    '>>>>' in one aligned 4-byte word."""
    rng = random.Random(11)
    out = bytearray()
    placed = []
    count = [0, 0]  # records, blanks handed out

    def letters():  # opens a record
        count[0] += 1
        return b"AC" if count[0] % 2 else b"GT"

    def blanks(n):
        count[1] += n
        return _blanks(count[1], n)

    def filler(total, term=b"\n"):
        """One record of exactly ``total`` bytes: a header line of JUNK, one sequence line that ends in ``term``; now and
        then a sequence line in front of it that starts with '=' or '?' (kept characters: the only place where a byte
        next to '>' in value stands where a '>' would open a line)."""
        ab = letters()
        s = min(rng.randrange(K, 40), total - 2 - len(term))
        h = total - 2 - s - len(term)
        assert s >= K and h >= 0, total
        extra = b""
        if h >= 10 and rng.random() < 0.4:
            extra = bytes([rng.choice(b"=?")]) + _draw(rng, ab, 3) + b"\n"
            h -= len(extra)
        junk = bytearray(_junk(rng, h))
        at = len(out) + 1
        i = -at % 4
        if i + 4 <= h:
            junk[i:i + 4] = b">>>>"
        out.extend(b">" + bytes(junk) + b"\n" + extra + _draw(rng, ab, s) + term)

    def fill_to(pos, term=b"\n"):
        while pos - len(out) > 300:
            filler(rng.randrange(40, 200))
        filler(pos - len(out), term)

    def feature(form, t):
        """The bytes in front of the '>' at t and the record it stands in."""
        if form in OPENING:
            lead = {"blank1": 1, "blank2": 2, "blank33": 33}.get(form, 0)
            fill_to(t - lead, {"cr": b"\r", "crlf": b"\r\n"}.get(form, b"\n"))
            out.extend(blanks(lead))
            ab = letters()
            out.extend(b">p" + _junk(rng, rng.randrange(0, 7)) + b"\n" + _draw(rng, ab, rng.randrange(K, 30)) + b"\n")
            return
        lead = {"in_header": 3, "after_base": 9, "after_blanks": 11, "after_star": 4}[form]
        fill_to(t - lead)
        ab = letters()
        if form == "in_header":
            out.extend(b">ab>cd\n" + _draw(rng, ab, 9) + b"\n")
        elif form == "after_base":
            out.extend(b">h\n" + _draw(rng, ab, 6) + b">" + _draw(rng, ab, 6) + b"\n")
        elif form == "after_blanks":
            out.extend(b">h\n" + _draw(rng, ab, 6) + blanks(2) + b">" + _draw(rng, ab, 6) + b"\n")
        else:
            out.extend(b">h\n*>" + _draw(rng, ab, 8) + b"\n")

    def place(unit, d, form):
        lead = {"blank1": 1, "blank2": 2, "blank33": 33, "in_header": 3, "after_base": 9, "after_blanks": 11, "after_star": 4}.get(form, 0)
        m = (len(out) + lead + 64 - d) // unit + 1
        # a true seam of its kind: a 16 that is no 32, a 32 that is no 2048, a 2048 that is no 8192
        while (unit == 16 and m % 2 == 0) or (unit == 32 and m % 64 == 0) or (unit == 2048 and m % 4 == 0):
            m += 1
        t = m * unit + d
        feature(form, t)
        assert out[t] == ord(">")
        placed.append((unit, d, form, t))

    jobs = {unit: [(d, form) for form in FORMS for d in SHIFTS] for unit in UNITS}
    for unit in UNITS:
        rng.shuffle(jobs[unit])
    for i in range(len(FORMS) * len(SHIFTS)):
        for unit in UNITS:
            place(unit, *jobs[unit][i])
    filler(77)
    return bytes(out), tuple(placed)


def placement_text() -> bytes:
    return placement()[0]


# ----------------------------------------------------------------------------- the end of the text
TAIL_ENDS = {"gt_last": b">", "bare": b">t", "cr": b">t\r", "crlf": b">t\r\n", "seq": b">t\nACACA", "seq_lf": b">t\nCACAC\n"}
TAIL_BASE = 96  # three lanes of the start kernels


@functools.lru_cache(maxsize=None)
def tail_texts() -> dict:
    """{name: text}: "<ending>_<r>" is the same short text padded to TAIL_BASE + r bytes, r = 0 .. 31, that ends in
    TAIL_ENDS[ending] -- a header line in (or, where the ending is longer than r, just in front of) the final partial run
    of 32; and the texts that start in '>', in blanks and '>', and without a header line."""
    out = {}
    for r in range(32):
        for name, end in TAIL_ENDS.items():
            pad = TAIL_BASE + r - len(end) - 11 - 3 - 7
            out["%s_%d" % (name, r)] = b">a\nACACACA\n>b" + (b"=?\xbe>" * pad)[:pad] + b"\nGTGTGT\n" + end
    rest = b">a\nACACA\n>b\nGTGTG\n>c\nCCCCC\n"
    out["gt_first"] = rest
    out["blanks_gt_first"] = b" \t\x1f" + rest
    out["blanks40_gt_first"] = _blanks(0, 40) + rest
    out["headless"] = b"ACACAC\n>b\nGTGTGT\n>c\nAACCA\n"
    out["headless_short"] = b"AC\n>b\nACACA\n"
    out["gt_only"] = b">"
    return out


# ----------------------------------------------------------------------------- gathers
def kept_record(rng, nbytes: int, mode: str) -> bytes:
    """A record of which ``mode`` emits exactly ``nbytes``: filter (inverted) the record as it stands, trim its header
    line, its leading A / C and one LF."""
    assert nbytes >= MIN_KEPT[mode], (mode, nbytes)
    if mode == "filter":
        if nbytes >= 5 and rng.random() < 0.5:
            s = rng.randrange(1, min(nbytes - 3, 12) + 1)
            return b">" + _junk(rng, nbytes - s - 3) + b"\n" + _draw(rng, b"GT" if s >= K else b"ACGT", s) + b"\n"
        return b">" + _junk(rng, nbytes - 2) + b"\n"
    p = rng.randrange(K, nbytes - 2)  # the header line keeps two bytes or more
    h = nbytes - p - 1
    term = rng.choice((b"\n", b"\n", b"\r", b"\r\n"))
    if h - 1 - len(term) < 0:
        term = b"\n"
    return b">" + _junk(rng, h - 1 - len(term)) + term + _draw(rng, b"AC", p) + _draw(rng, b"GT", rng.choice((0, 0, 1, 3, 6))) + b"\n"


def dropped_record(rng, nbytes: int, mode: str) -> bytes:
    """A record of ``nbytes`` raw bytes of which ``mode`` emits nothing."""
    assert nbytes >= MIN_DROP[mode], (mode, nbytes)
    if mode == "filter":
        s = rng.randrange(K, min(nbytes - 3, 20) + 1)
        return b">" + _junk(rng, nbytes - s - 3) + b"\n" + _draw(rng, b"AC", s) + b"\n"
    if nbytes >= 4 and rng.random() < 0.7:
        s = rng.randrange(1, min(nbytes - 3, 20) + 1)
        return b">" + _junk(rng, nbytes - s - 3) + b"\n" + _draw(rng, b"GT" if s >= K else b"ACGT", s) + b"\n"
    return b">" + _junk(rng, nbytes - 2) + b"\n"


def _sizes(rng, total: int, lo: int, hi: int):
    """``total`` split into sizes of lo .. hi."""
    out = []
    while total:
        n = min(total, rng.randrange(lo, hi + 1))
        if 0 < total - n < lo:
            n = total - lo if total - lo >= lo else total
        out.append(n)
        total -= n
    return out


def _lengths(mode: str) -> dict:
    out = {}
    for L in LENGTHS:
        rng = random.Random(100_000 + L)
        if L < MIN_KEPT[mode]:
            if L == 1 and mode == "filter":  # a '>' alone, the last byte of the text
                out["len_1"] = dropped_record(rng, 12, mode) + b">"
            continue
        t = [dropped_record(rng, rng.randrange(MIN_DROP[mode], 30), mode)]
        for n in _sizes(rng, L, MIN_KEPT[mode], max(200, MIN_KEPT[mode])) if L > 40 else [L]:
            t.append(kept_record(rng, n, mode))
            if rng.random() < 0.5:
                t.append(dropped_record(rng, rng.randrange(MIN_DROP[mode], 30), mode))
        out["len_%d" % L] = b"".join(t)
    return out


def boundaries(mode: str, shift: int):
    """(text, [(source offset, output offset) of every kept record]): kept records of MIN_KEPT .. 40 output bytes; a dropped
    record in front of each is sized so that every pair (source offset mod 16, output offset mod 16) occurs at a record
    start, and a record starts exactly at OUT_SEAMS[i] + shift."""
    rng = random.Random(7000 + shift + (50 if mode == "trim" else 0))
    lo, hi = MIN_KEPT[mode], 40
    targets = [s + shift for s in OUT_SEAMS]
    need = {(a, b) for a in range(16) for b in range(16)}
    text, at, starts, extra = bytearray(), 0, [], 24
    while targets or extra:
        wanted = [a for a in range(16) if (a, at % 16) in need]
        gap = (rng.choice(wanted) - len(text)) % 16 if wanted else rng.randrange(16)
        if gap or rng.random() < 0.3:
            while gap < MIN_DROP[mode]:
                gap += 16
            text += dropped_record(rng, gap, mode)
        n = max(rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1))
        if len(starts) % 40 in (7, 8):  # the smallest and the largest, now and then
            n = lo if len(starts) % 40 == 7 else hi
        if targets:
            t = targets[0] - at
            n = t if t <= hi else min(n, t - lo)
        else:
            extra -= 1
        starts.append((len(text), at))
        need.discard((len(text) % 16, at % 16))
        text += kept_record(rng, n, mode)
        at += n
        if targets and at == targets[0]:
            targets.pop(0)
    text += dropped_record(rng, 20, mode)
    starts.append((len(text), at))  # the end of the last kept record, where no record starts
    return bytes(text), starts


def _minimal(mode: str) -> dict:
    rng = random.Random(31)
    lo = MIN_KEPT[mode]
    run = lambda n, count: b"".join(kept_record(rng, n, mode) for _ in range(count))
    mixed = b"".join(kept_record(rng, lo + i % 2, mode) for i in range(100))
    # a headless first record of 2 bytes: no windows, so filter (inverted) keeps it and trim drops it
    text = b"A\n" + run(lo, 200) + dropped_record(rng, 12, mode) + run(lo + 1, 100) + mixed + dropped_record(rng, 9, mode) + run(lo, 40)
    return {"minimal": text}


def _dropped_runs(mode: str) -> dict:
    out = {}
    for n in RUNS:
        rng = random.Random(500 + n)
        drops = lambda: b"".join(dropped_record(rng, MIN_DROP[mode] + i % 3, mode) for i in range(n))
        out["drops_%d" % n] = drops() + kept_record(rng, 21, mode) + drops() + kept_record(rng, 37, mode) + drops()
        # the run in front of the LAST row, kept: fl_record_from has to step onto row nrows - 1 itself, n + 1 rows from the
        # chunk's first record and n rows from the record that ends inside the chunk
        out["drops_last_%d" % n] = kept_record(rng, 21, mode) + drops() + kept_record(rng, 37, mode)
    return out


def _last32(mode: str) -> dict:
    out = {}
    for size in (10, 24, 40):
        for res in range(16):
            for newline in (True, False):
                rng = random.Random(1000 * size + 2 * res + newline)
                # without its last LF filter emits one byte less of the record; trim writes the LF all the same
                last = kept_record(rng, size + (1 if mode == "filter" and not newline else 0), mode)
                if not newline:
                    assert last.endswith(b"\n")
                    last = last[:-1]
                head = kept_record(rng, 19, mode)
                pad = 40 + (res - len(head) - 40 - len(last)) % 16
                text = head + dropped_record(rng, pad, mode) + last
                assert len(text) % 16 == res and len(text) >= 64
                out["last_%d_%d_%s" % (size, res, "lf" if newline else "bare")] = text
    return out


def _long_record(mode: str) -> dict:
    rng = random.Random(9)
    t = [(kept_record if i % 2 else dropped_record)(rng, rng.randrange(8, 41), mode) for i in range(100)]
    seq = _draw(rng, b"GT" if mode == "filter" else b"AC", 50_000)
    t.append(b">long\n" + b"".join(seq[i:i + 61] + b"\n" for i in range(0, len(seq), 61)))
    t += [dropped_record(rng, 11, mode), kept_record(rng, 23, mode)]
    return {"long": b"".join(t)}


@functools.lru_cache(maxsize=None)
def gather_cases(mode: str) -> dict:
    """{family: {name: text}} for "filter" (kept under invert; the plain output is the complement) or "trim"."""
    assert mode in MODES
    return {"lengths": _lengths(mode),
            "boundaries": {"bound_%+d" % s: boundaries(mode, s)[0] for s in (-1, 0, 1)},
            "minimal": _minimal(mode),
            "dropped_runs": _dropped_runs(mode),
            "last32": _last32(mode),
            "long": _long_record(mode)}


def emitted(text: bytes, mode: str) -> bytes:
    """What ``mode`` emits of a gather text, by its rule."""
    if mode == "filter":
        return filter_rule.expected(text, table(), K, FILTER_RULE, True)[0]
    return trim_rule.expected(text, table(), K, TRIM_AT_LEAST)[0]


def header_alone_text() -> bytes:
    """Header lines alone (2 and 3 bytes: eight to a chunk of what mk_correct_* writes, none with an LF of its own) and
    records shorter than k between ordinary ones, some of those with one base that is neither A nor C."""
    rng = random.Random(77)
    t = []
    for i in range(40):
        t.append(b">o%d\n" % i + _draw(rng, b"AC", 9) + (b"G" if i % 3 == 0 else b"C") + _draw(rng, b"AC", 9 + i % 7) + b"\n")
        t.append(b">\n" * (1 + i % 9) if i % 2 else b">x\n" * (1 + i % 5))
        t.append(b">s\n" + _draw(rng, b"ACGT", 1 + i % 4) + b"\n")
        if i % 4 == 0:
            t.append(b">\r\n>\r")
    return b"".join(t) + b">"


# ----------------------------------------------------------------------------- more tiles than the scan has threads
MANY_SEAM = SCAN_THREADS * UNITS[3]  # the first raw byte of tile 1024: with two tiles a thread, thread 512's first
MANY_LINE = 4001


@functools.lru_cache(maxsize=None)
def many_tiles():
    """(text, [(first byte, header line, sequence)]): about 130 records that cycle through four sequences of about 65 000
    bases (two over {A, C}, one over {G, T}, one over all four) on lines of MANY_LINE, with record starts at
    MANY_SEAM - 1, MANY_SEAM + 1 and MANY_SEAM + 8192."""
    rng = random.Random(5)
    seqs = [_draw(rng, b"AC", 65_003), _draw(rng, b"GT", 65_001), _draw(rng, b"AC", 64_999), _draw(rng, b"ACGT", 65_007)]
    wrapped = [b"".join(s[i:i + MANY_LINE] + b"\n" for i in range(0, len(s), MANY_LINE)) for s in seqs]
    parts, recs, at = [], [], 0

    def add(header, seq, body):
        nonlocal at
        recs.append((at, header, seq))
        parts.append(header + body)
        at += len(header) + len(body)

    i = 0
    while at + 70_000 < MANY_SEAM - 1:
        add(b">r%d\n" % i, seqs[i % 4], wrapped[i % 4])
        i += 1
    add(b">pad " + b"=?>\xbe" * ((MANY_SEAM - 1 - at - 6) // 4) + b"x" * ((MANY_SEAM - 1 - at - 6) % 4) + b"\n", b"", b"")
    add(b">\n", b"", b"")                                    # MANY_SEAM - 1
    short = _draw(rng, b"AC", UNITS[3] - 1 - 3 - 1)
    add(b">s\n", short, short + b"\n")                       # MANY_SEAM + 1, ends where the next tile starts
    assert at == MANY_SEAM + UNITS[3]
    while at < MANY_SEAM + 200_000:
        add(b">r%d\n" % i, seqs[i % 4], wrapped[i % 4])
        i += 1
    return b"".join(parts), recs


def many_tiles_text() -> bytes:
    return many_tiles()[0]


@functools.lru_cache(maxsize=None)
def many_tiles_expected() -> dict:
    """What filter (plain and inverted) and trim give for many_tiles(), a record's row and kept length computed once per
    distinct sequence."""
    text, recs = many_tiles()
    row_of, kept_of = {}, {}
    for _, _, seq in recs:
        if seq not in row_of:
            row_of[seq] = filter_rule.ref_rows(b">x\n" + seq + b"\n", table(), K, 1)[0]
            kept_of[seq] = trim_rule.kept_of(seq, table(), K, TRIM_AT_LEAST)
    ends = [at for at, _, _ in recs[1:]] + [len(text)]
    rows = [row_of[seq] for _, _, seq in recs]
    match = [filter_rule.matched(r, FILTER_RULE) for r in rows]
    kept = [kept_of[seq] for _, _, seq in recs]
    raws = [text[at:end] for (at, _, _), end in zip(recs, ends)]
    return {"rows": rows, "matched": match, "kept": kept, "distinct": len(row_of),
            "plain": b"".join(raw for raw, m in zip(raws, match) if m), "inverted": b"".join(raw for raw, m in zip(raws, match) if not m),
            "trim": b"".join(header + seq[:n] + b"\n" for (_, header, seq), n in zip(recs, kept) if n)}
