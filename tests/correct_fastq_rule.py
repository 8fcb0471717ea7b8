"""Plain-Python restatement of mk_correct_fastq_* (include/mercat_hip.h) over Python bytes and a dict: the 4-line
records of a FASTQ text (fastq_select_rule), their checks, the FASTA view fq2fa gives of them, the view check, and
mk_correct_*'s rule (correct_rule.correct_seq) applied to every sequence line with the patches -- and new_qual -- put
into a copy of the text.  Nothing here calls the library."""
import correct_rule
import fastq_select_rule as fsr
import trim_rule

ERR_ARG, ERR_NON_ASCII, ERR_UNSUPPORTED = -1, -5, -8


class CorrectFastqError(Exception):
    def __init__(self, code, record=None, kind=None, counts=None):
        super().__init__("code %d record %r kind %r counts %r" % (code, record, kind, counts))
        self.code, self.record, self.kind, self.counts = code, record, kind, counts


def view(text):
    """The FASTA view of a text whose records pass the checks, byte offsets kept: the '@' of line 4r made '>', every
    byte of lines 4r + 2 and 4r + 3 made a newline, a header line that does not start with '@' made newlines too."""
    out = []
    for i, line in enumerate(fsr.lines(text)):
        if i % 4 == 0:
            out.append(b">" + line[1:] if line.startswith(b"@") else b"\n" * len(line))
        elif i % 4 == 1:
            out.append(line)
        else:
            out.append(b"\n" * len(line))
    return b"".join(out)


def parsed(text):
    """[(offset of the header line, kept characters)] of a FASTA text as trim_rule.records reads it (-1: headless)."""
    recs, at = [], 0
    for line in trim_rule._LINE.findall(bytes(text)):
        stripped = line.strip(trim_rule._BLANKS)
        if stripped.startswith(b">"):
            recs.append([at, b""])
        else:
            piece = stripped.replace(b"*", b"")
            if not recs and piece:
                recs.append([-1, b""])
            if recs:
                recs[-1][1] += piece
        at += len(line)
    return recs


def view_check(text):
    """None, or (record, "view") for the lowest record the parser reads differently, or (None, "counts") when only the
    record counts differ."""
    recs, _ = fsr.records(text)
    seen = parsed(view(text))
    at = 0
    for r, rec in enumerate(recs):
        if r < len(seen) and (seen[r][0] != at or seen[r][1] != fsr.content(rec[1])):
            return r, "view"
        at += sum(len(x) for x in rec)
    if len(seen) != len(recs):
        return None, "counts"
    return None


def expected(text, table, k, at_least, new_qual=0, fold=False):
    """(output bytes, [(runs, fixed, ambiguous, unfixable) per record]) or CorrectFastqError."""
    text = bytes(text)
    if at_least < 1 or (new_qual and not 33 <= new_qual <= 126) or not 0 <= new_qual < 1 << 32:
        raise CorrectFastqError(ERR_ARG)
    bad = fsr.check(text, True)
    if bad:
        raise CorrectFastqError(ERR_UNSUPPORTED, bad[0], bad[1])
    recs, _ = fsr.records(text)
    if any(b >= 0x80 for rec in recs for b in fsr.content(rec[1])):
        raise CorrectFastqError(ERR_NON_ASCII)
    bad = view_check(text)
    if bad:
        raise CorrectFastqError(ERR_UNSUPPORTED, bad[0], bad[1], (len(parsed(view(text))), len(recs)))
    out, rows, at = bytearray(text), [], 0
    for head, seq, plus, qual in recs:
        s = fsr.content(seq)
        fixed_seq, row = correct_rule.correct_seq(s, table, k, at_least, fold)
        rows.append(row)
        s_at, q_at = at + len(head), at + len(head) + len(seq) + len(plus)
        for j, (a, b) in enumerate(zip(s, fixed_seq)):
            if a != b:
                out[s_at + j] = b
                if new_qual:
                    out[q_at + j] = new_qual
        at += len(head) + len(seq) + len(plus) + len(qual)
    return bytes(out), rows


def figures(text, rows):
    """lines, records, patched / fixed, bytes_out of a call that succeeds."""
    fixed = sum(r[1] for r in rows)
    return {"lines": len(fsr.lines(text)), "records": len(rows), "patched": fixed, "fixed": fixed, "bytes_out": len(text),
            "runs": sum(r[0] for r in rows), "ambiguous": sum(r[2] for r in rows), "unfixable": sum(r[3] for r in rows)}
