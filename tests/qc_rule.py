"""Restatement of mk_fastq_qc_* (include/mercat_hip.h) over Python bytes: the per-cycle and per-read quality-control tables
of a FASTQ text, rows and the figures -- errors included.  The records and the checks are those of qtrim_rule.py; the
tables are added up with numpy (bincount over flat indices), so 20 000 reads take well under a second.  Nothing here calls
the library."""
import numpy as np

from fastq_select_rule import content, lines, records

ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -7, -8
PHRASE = {"at": "does not start with '@'", "plus": "does not start with '+'", "length": "differ in length",
          "qual": "holds a character below the phred base", "incomplete": "the text ends inside it"}
MAX_POS, QBINS, GC_BINS = 16384, 96, 101
OPT = dict(max_pos=512, phred_base=33, paired=0)
TABLES = ("pos_qual", "pos_base", "read_len", "read_qual", "read_gc")

BASE_CLASS = np.full(256, 5, np.int64)  # of seq[i] | 0x20
for _k, _ch in enumerate(b"acgtn"):
    BASE_CLASS[_ch] = _k


class QcError(Exception):
    def __init__(self, code, record=None, kind=None, counts=None):
        super().__init__("code %d record %r kind %r counts %r" % (code, record, kind, counts))
        self.code, self.record, self.kind, self.counts = code, record, kind, counts


def options(**kw):
    """The options of a call: OPT with kw over it."""
    bad = set(kw) - set(OPT)
    if bad:
        raise TypeError("unknown option %r" % sorted(bad))
    return dict(OPT, **kw)


def shapes(max_pos, paired):
    c = 2 if paired else 1
    return {"pos_qual": (c, max_pos + 1, QBINS), "pos_base": (c, max_pos + 1, 8), "read_len": (c, max_pos + 2),
            "read_qual": (c, QBINS), "read_gc": (c, GC_BINS)}


def check(text, phred_base):
    """None, or (record, kind) of the lowest malformed record and the first check it fails."""
    recs, trailing = records(text)
    bad = None
    for r, (head, seq, plus, qual) in enumerate(recs):
        if not head.startswith(b"@"):
            bad = r, "at"
        elif not plus.startswith(b"+"):
            bad = r, "plus"
        elif len(content(seq)) != len(content(qual)):
            bad = r, "length"
        if bad:
            break
    # the lowest quality line in front of that record that holds a byte below the base
    quals = [content(rec[3]) for rec in (recs if bad is None else recs[:bad[0]])]
    lens = np.array([len(q) for q in quals], np.int64)
    if lens.sum():
        low = np.frombuffer(b"".join(quals), np.uint8) < phred_base
        hits = np.flatnonzero(low)
        if len(hits):
            return int(np.repeat(np.arange(len(quals)), lens)[hits[0]]), "qual"
    if bad:
        return bad
    if any(t != b"\n" for t in trailing):
        return len(recs), "incomplete"
    return None


def run(text, cap=None, **kw):
    """What a call that succeeds gives: the five tables (uint64 arrays of shapes()), "rows" ((records, 4): length, qsum,
    gc, n) and "figures"; QcError otherwise (arguments, then the record count against cap -- the room of rows, None for a
    call without rows --, then an odd count with paired, then the lowest malformed record)."""
    o = options(**kw)
    if o["phred_base"] not in (33, 64) or not 1 <= o["max_pos"] <= MAX_POS or o["paired"] not in (0, 1):
        raise QcError(ERR_ARG)
    recs, _ = records(text)
    n = len(recs)
    if cap is not None and n > cap:
        raise QcError(ERR_RANGE, counts=(n, cap))
    if o["paired"] and n % 2:
        raise QcError(ERR_RANGE, counts=(n,))
    bad = check(text, o["phred_base"])
    if bad:
        raise QcError(ERR_UNSUPPORTED, bad[0], bad[1])
    P, C = o["max_pos"], 2 if o["paired"] else 1
    seq = np.frombuffer(b"".join(content(rec[1]) for rec in recs), np.uint8).astype(np.int64)
    q = np.frombuffer(b"".join(content(rec[3]) for rec in recs), np.uint8).astype(np.int64) - o["phred_base"]
    L = np.array([len(content(rec[1])) for rec in recs], np.int64)
    of = np.repeat(np.arange(n, dtype=np.int64), L)              # the record of every base
    i = np.arange(len(q), dtype=np.int64) - np.repeat(np.cumsum(L) - L, L)  # its cycle
    cls = (of & 1) if o["paired"] else np.zeros_like(of)
    p, v, b = np.minimum(i, P), np.minimum(q, QBINS - 1), BASE_CLASS[seq | 0x20]
    rcls = (np.arange(n, dtype=np.int64) & 1) if o["paired"] else np.zeros(n, np.int64)
    count = lambda flat, shape: np.bincount(flat, minlength=int(np.prod(shape))).astype(np.uint64).reshape(shape)
    sh = shapes(P, o["paired"])
    out = {"pos_qual": count((cls * (P + 1) + p) * QBINS + v, sh["pos_qual"]),
           "pos_base": count((cls * (P + 1) + p) * 8 + b, sh["pos_base"]),
           "read_len": count(rcls * (P + 2) + np.minimum(L, P + 1), sh["read_len"])}
    per_read = lambda w: np.rint(np.bincount(of, weights=w, minlength=n)).astype(np.int64) if n else np.zeros(0, np.int64)
    qsum, gc, nn = per_read(q), per_read((b == 1) | (b == 2)), per_read(b == 4)
    some = L > 0
    Ls = L[some]
    out["read_qual"] = count(rcls[some] * QBINS + np.minimum(qsum[some] // Ls, QBINS - 1), sh["read_qual"])
    out["read_gc"] = count(rcls[some] * GC_BINS + (200 * gc[some] + Ls) // (2 * Ls), sh["read_gc"])
    out["rows"] = np.stack([L, qsum, gc, nn], axis=1).astype(np.uint64) if n else np.zeros((0, 4), np.uint64)
    of_class = [L[rcls == c] for c in (0, 1)]
    out["figures"] = dict(records=n, lines=len(lines(text)), bases=int(L.sum()),
                          min_len=[int(x.min()) if len(x) else 0 for x in of_class],
                          max_len=[int(x.max()) if len(x) else 0 for x in of_class])
    return out
