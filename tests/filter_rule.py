"""The rule of mk_filter_* (include/mercat_hip.h) restated over Python bytes and a dict: what the tests compare
Counter.filter with.  Nothing here touches the library.

A record's row is plain Python over ``dict.get(window, 0)`` on the reference's line loop, its byte range comes from a
regular expression over the raw text that knows nothing of the parser, and the rule is applied in Python integers."""
import io
import re

COMP = str.maketrans("ACGT", "TGCA")
# a header line: '>' with only blanks between it and the line's start (after LF or CR, or at the start of the text)
HEADER_LINE = re.compile(rb"(?:^|(?<=[\n\r]))[ \t\x0b\x0c\x1c-\x1f]*>")


def ref_records(text: bytes):
    """[(headed, sequence)] by the reference's line loop (lib/mercat2_kmers.py:49-69): text mode, strip(),
    startswith('>'), replace('*', '').  Sequence in front of the first header is a record of its own (headed False)."""
    recs = []
    for line in io.TextIOWrapper(io.BytesIO(text), encoding="latin-1", newline=None):
        line = line.strip()
        if line.startswith(">"):
            recs.append([True, ""])
        else:
            piece = line.replace("*", "")
            if not recs and piece:
                recs.append([False, ""])
            if recs:
                recs[-1][1] += piece
    return recs


def ref_rows(text: bytes, table: dict, k: int, at_least: int = 1, fold: bool = False):
    rows = []
    for _, seq in ref_records(text):
        counts = []
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if fold and set(w) <= set("ACGT"):
                w = min(w, w.translate(COMP)[::-1])
            counts.append(table.get(w, 0))
        rows.append([len(counts), sum(1 for c in counts if c >= at_least), sum(counts) % (1 << 64),
                     min(counts, default=0), max(counts, default=0)])
    return rows


def ref_ranges(text: bytes):
    """([(first byte, end)] per record, preamble): the header lines of the RAW text; row 0 from byte 0 when the line loop
    says the text starts without a header."""
    starts = [m.start() for m in HEADER_LINE.finditer(text)]
    recs = ref_records(text)
    headless = bool(recs) and not recs[0][0]
    assert len(recs) == len(starts) + (1 if headless else 0)
    if headless:
        starts = [0] + starts
    preamble = starts[0] if starts else len(text)
    return list(zip(starts, starts[1:] + [len(text)])), preamble


def matched(row, rule) -> bool:
    windows, hits = row[0], row[1]
    return windows > 0 and hits >= rule[1] and hits * 1_000_000 >= rule[2] * windows


def expected(text: bytes, table: dict, k: int, rule, invert: bool, fold: bool = False):
    rows = ref_rows(text, table, k, rule[0], fold)
    ranges, preamble = ref_ranges(text)
    keep = [matched(r, rule) != invert for r in rows]
    return b"".join(text[a:b] for (a, b), kp in zip(ranges, keep) if kp), keep, rows, preamble
