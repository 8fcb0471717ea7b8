"""Plain-Python restatement of mk_fastq_select_* (include/mercat_hip.h) over Python bytes: the 4-line records of a
FASTQ text, their well-formedness, and the bytes a keep / kept decision leaves of them -- errors included.  Also the
two-file helpers mk_fq_interleave / mk_fq_split_pairs.  Nothing here calls the library."""

ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -7, -8
# what the parser does not count among a sequence line's kept characters: the bytes str.strip() removes (LF ends the line
# and is none of them) and '*'
NOT_KEPT = frozenset([9, 11, 12, 13, 28, 29, 30, 31, 32, ord("*")])
# a word of the library's message for every kind of failure
PHRASE = {"at": "does not start with '@'", "plus": "does not start with '+'", "length": "differ in length",
          "blank": "holds a blank or a '*'", "kept": "more than its sequence holds", "incomplete": "the text ends inside it"}


class SelectError(Exception):
    def __init__(self, code, record=None, kind=None, counts=None):
        super().__init__("code %d record %r kind %r counts %r" % (code, record, kind, counts))
        self.code, self.record, self.kind, self.counts = code, record, kind, counts


def lines(text):
    """The lines of the text, each with its '\\n' (split on '\\n' only; a last line without one is a line)."""
    parts = bytes(text).split(b"\n")
    out = [p + b"\n" for p in parts[:-1]]
    if parts[-1]:
        out.append(parts[-1])
    return out


def records(text):
    """([the four lines of every complete record], [the up to three lines behind the last of them])."""
    ls = lines(text)
    n = len(ls) // 4
    return [ls[4 * i:4 * i + 4] for i in range(n)], ls[4 * n:]


def content(line):
    """A line without its '\\n' and without one trailing '\\r'."""
    if line.endswith(b"\n"):
        line = line[:-1]
    if line.endswith(b"\r"):
        line = line[:-1]
    return line


def check(text, kept_given, kept=None):
    """None, or (record, kind) of the lowest malformed record and the first check it fails."""
    recs, trailing = records(text)
    for r, (head, seq, plus, qual) in enumerate(recs):
        if not head.startswith(b"@"):
            return r, "at"
        if not plus.startswith(b"+"):
            return r, "plus"
        if len(content(seq)) != len(content(qual)):
            return r, "length"
        if kept_given and any(b in NOT_KEPT for b in content(seq)):
            return r, "blank"
        if kept is not None and int(kept[r]) > len(content(seq)):
            return r, "kept"
    if any(t != b"\n" for t in trailing):
        return len(recs), "incomplete"
    return None


def expected(text, keep=None, kept=None, which=1, nrec=None):
    """The bytes mk_fastq_select_* writes, or SelectError.  nrec None: the length of the arrays (the text's own count
    when there are none)."""
    recs, _ = records(text)
    if keep is not None and which not in (1, 2):
        raise SelectError(ERR_ARG)
    if nrec is None:
        nrec = len(keep) if keep is not None else len(kept) if kept is not None else len(recs)
    if nrec != len(recs):
        raise SelectError(ERR_RANGE, counts=(len(recs), nrec))
    bad = check(text, kept is not None, kept)
    if bad:
        raise SelectError(ERR_RANGE if bad[1] == "kept" else ERR_UNSUPPORTED, bad[0], bad[1])
    out = []
    for r, (head, seq, plus, qual) in enumerate(recs):
        if keep is not None and int(keep[r]) != which:
            continue
        if kept is None:
            rec = head + seq + plus + qual
            out.append(rec if rec.endswith(b"\n") else rec + b"\n")
        elif int(kept[r]) > 0:
            n = int(kept[r])
            out.append(head + content(seq)[:n] + b"\n" + plus + content(qual)[:n] + b"\n")
    return b"".join(out)


def figures(text, keep=None, kept=None, which=1):
    """records, records_out, records_trimmed, bases_out, bytes_out, lines of a call that succeeds."""
    recs, _ = records(text)
    out = trimmed = bases = 0
    for r, (head, seq, plus, qual) in enumerate(recs):
        if keep is not None and int(keep[r]) != which:
            continue
        if kept is not None and int(kept[r]) == 0:
            continue
        L = len(content(seq))
        n = L if kept is None else int(kept[r])
        out, trimmed, bases = out + 1, trimmed + (1 if n < L else 0), bases + n
    return {"records": len(recs), "records_out": out, "records_trimmed": trimmed, "bases_out": bases,
            "bytes_out": len(expected(text, keep, kept, which)), "lines": len(lines(text))}


def cuts(text, piece):
    """Where mk_fastq_cuts cuts: behind a line 4j once the piece holds `piece` bytes, strictly inside the text."""
    out, at, start = [], 0, 0
    for i, line in enumerate(lines(text)):
        at += len(line)
        if i % 4 == 3 and at < len(text) and at - start >= piece:
            out.append(at)
            start = at
    return out


def _whole_records(text):
    recs, trailing = records(text)
    if any(t != b"\n" for t in trailing):
        raise SelectError(ERR_UNSUPPORTED, len(recs), "incomplete")
    out = [b"".join(r) for r in recs]
    return [r if r.endswith(b"\n") else r + b"\n" for r in out]


def interleave(a, b):
    ra, rb = _whole_records(a), _whole_records(b)
    if len(ra) != len(rb):
        raise SelectError(ERR_RANGE, counts=(len(ra), len(rb)))
    return b"".join(x + y for x, y in zip(ra, rb))


def split(text):
    recs = _whole_records(text)
    if len(recs) % 2:
        raise SelectError(ERR_RANGE, counts=(len(recs),))
    return b"".join(recs[0::2]), b"".join(recs[1::2])
