"""Restatement of mk_fastq_dedup_* (include/mercat_hip.h) over Python bytes: the duplicate reads of a FASTQ text by a dict
keyed by the key bytes -- out, keep, rows, levels and the figures, errors included.  The lines, records and checks are
those of fastq_select_rule.py (split on '\\n' only; '@', '+', equal lengths, a text that ends inside a record).  Nothing
here calls the library, and no hash of the library's is known here."""
import numpy as np

from fastq_select_rule import content, lines, records

ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -7, -8
PHRASE = {"at": "does not start with '@'", "plus": "does not start with '+'", "length": "differ in length",
          "incomplete": "the text ends inside it"}
MAX_HIGH = 1 << 20
FIGURES = ("records", "records_out", "distinct", "duplicates", "max_copies", "bases_in", "bases_out", "bytes_out", "lines")


class DedupError(Exception):
    def __init__(self, code, record=None, kind=None, counts=None):
        super().__init__("code %d record %r kind %r counts %r" % (code, record, kind, counts))
        self.code, self.record, self.kind, self.counts = code, record, kind, counts


def check(text):
    """None, or (record, kind) of the lowest malformed record and the first check it fails."""
    recs, trailing = records(text)
    for r, (head, seq, plus, qual) in enumerate(recs):
        if not head.startswith(b"@"):
            return r, "at"
        if not plus.startswith(b"+"):
            return r, "plus"
        if len(content(seq)) != len(content(qual)):
            return r, "length"
    if any(t != b"\n" for t in trailing):
        return len(recs), "incomplete"
    return None


def key(seq_line, prefix):
    seq = content(seq_line)
    return seq[:prefix] if prefix else seq


def run(text, prefix=0, paired=0, which=1, high=100, cap=None):
    """What a call that succeeds gives: "out" (bytes), "keep" (uint8 a record), "rows" ((records, 2) uint64: length,
    first), "levels" ((high + 2,) uint64) and "figures"; DedupError otherwise (arguments, then the record count against
    cap -- None for a call without keep and rows --, then an odd count with paired, then the lowest malformed record)."""
    if paired not in (0, 1) or which not in (1, 2) or not 1 <= high <= MAX_HIGH:
        raise DedupError(ERR_ARG)
    recs, _ = records(text)
    n = len(recs)
    if cap is not None and n > cap:
        raise DedupError(ERR_RANGE, counts=(n, cap))
    if paired and n % 2:
        raise DedupError(ERR_RANGE, counts=(n,))
    bad = check(text)
    if bad:
        raise DedupError(ERR_UNSUPPORTED, bad[0], bad[1])
    per = 2 if paired else 1
    first_of, size = {}, {}
    first = np.zeros(n, np.uint64)
    for u in range(n // per):
        k = tuple(key(recs[per * u + m][1], prefix) for m in range(per))
        f = first_of.setdefault(k, u)
        size[f] = size.get(f, 0) + 1
        for m in range(per):
            first[per * u + m] = per * f + m
    keep = (first == np.arange(n, dtype=np.uint64)).astype(np.uint8)
    length = np.array([len(content(rec[1])) for rec in recs], np.uint64)
    emitted = [r for r in range(n) if (1 if keep[r] else 2) == which]
    out = []
    for r in emitted:
        whole = b"".join(recs[r])
        out.append(whole if whole.endswith(b"\n") else whole + b"\n")
    levels = np.zeros(high + 2, np.uint64)
    for c in size.values():
        levels[min(c, high + 1)] += 1
    out = b"".join(out)
    figures = dict(records=n, records_out=len(emitted), distinct=len(size), duplicates=int(n - keep.sum()),
                   max_copies=max(size.values()) if size else 0, bases_in=int(length.sum()),
                   bases_out=int(length[emitted].sum()) if emitted else 0, bytes_out=len(out), lines=len(lines(text)))
    return {"out": out, "keep": keep, "rows": np.stack([length, first], axis=1) if n else np.zeros((0, 2), np.uint64),
            "levels": levels, "figures": figures}
