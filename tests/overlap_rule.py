"""Plain-Python restatement of mk_fastq_overlap_* (include/mercat_hip.h) over Python bytes: the overlap of every pair of
an interleaved FASTQ text -- mate 1 against the reverse complement of mate 2 at every offset, in the rule's order -- the
cut or the merged read, the bytes that come out, keep, rows and the figures, errors included.  Nothing here calls the
library."""
import functools

from adapt_rule import PHRASE, check, fold  # (PHRASE: for the tests that read an error's message)
from fastq_select_rule import content, lines, records

ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -7, -8
NO_HIT = 0xFFFFFFFF
MAX_BASES = 512
TRIM, MERGE = 0, 1
OPT = dict(mode=MERGE, min_overlap=30, max_mismatch=5, max_err_ppm=200000, min_len=0, which=1)
ACGT = b"ACGT"
COMP = {65: 84, 67: 71, 71: 67, 84: 65}


class OverlapError(Exception):
    def __init__(self, code, record=None, kind=None, counts=None):
        super().__init__("code %d record %r kind %r counts %r" % (code, record, kind, counts))
        self.code, self.record, self.kind, self.counts = code, record, kind, counts


def options(**kw):
    """The options of a call: OPT with kw over it."""
    bad = set(kw) - set(OPT)
    if bad:
        raise TypeError("unknown option %r" % sorted(bad))
    return dict(OPT, **kw)


def comp(b):
    """The complement of a folded byte: A <-> T, C <-> G, anything else N."""
    return COMP.get(b, 78)


def revcomp(s):
    """rc of the notation: rc[j] = comp(fold(s[L - 1 - j]))."""
    return bytes(comp(fold(b)) for b in reversed(s))


def overlap_of(d, L1, L2):
    """(lo, hi): the overlap of candidate d in mate 1's positions."""
    return max(d, 0), min(L1, d + L2)


def candidates(L1, L2, min_overlap):
    """The offsets in the rule's order: 0, 1, 2, ... while ov >= min_overlap, then -1, -2, ... while ov >= min_overlap."""
    for step, d in ((1, 0), (-1, -1)):
        while True:
            lo, hi = overlap_of(d, L1, L2)
            if hi - lo < min_overlap:
                break
            yield d
            d += step


def mismatches(s1, rc, d, limit=None):
    """(ov, mm) of candidate d: s1 folded, rc as revcomp gives it.  With limit the count stops at the first mismatch
    beyond it: the candidate is then not admissible, and the count says only that."""
    lo, hi = overlap_of(d, len(s1), len(rc))
    mm = 0
    for p in range(lo, hi):
        if not (s1[p] in ACGT and s1[p] == rc[p - d]):
            mm += 1
            if limit is not None and mm > limit:
                break
    return hi - lo, mm


@functools.lru_cache(maxsize=None)
def find(s1, s2, min_overlap, max_mismatch, max_err_ppm):
    """(d, fragment, overlap, mismatches) of the first admissible candidate, or None.  (Kept: a test asks for the same
    pairs in both modes.)"""
    if len(s1) > MAX_BASES or len(s2) > MAX_BASES:
        return None
    f1, rc = bytes(fold(b) for b in s1), revcomp(s2)
    for d in candidates(len(s1), len(s2), min_overlap):
        ov, mm = mismatches(f1, rc, d, max_mismatch)
        if ov >= min_overlap and mm <= max_mismatch and mm * 1000000 <= max_err_ppm * ov:
            return d, d + len(s2), ov, mm
    return None


def merged(s1, q1, s2, q2, d):
    """(sequence, quality) of the merged read of a pair whose hit is d."""
    rc, rq = revcomp(s2), bytes(reversed(q2))
    L1, F = len(s1), d + len(s2)
    seq, qual = bytearray(), bytearray()
    for p in range(F):
        if p < d:
            base, q = s1[p], q1[p]
        elif p >= L1:
            base, q = rc[p - d], rq[p - d]
        else:
            a, b, qa, qb = s1[p], rc[p - d], q1[p], rq[p - d]
            a_ok, b_ok = fold(a) in ACGT, b in ACGT
            if a_ok and b_ok and fold(a) == b:
                base, q = a, max(qa, qb)
            elif a_ok != b_ok:
                base, q = (a, qa) if a_ok else (b, qb)
            elif qb > qa:
                base, q = b, qb
            else:
                base, q = a, qa
        seq.append(base)
        qual.append(q)
    return bytes(seq), bytes(qual)


def whole(rec):
    rec = b"".join(rec)
    return rec if rec.endswith(b"\n") else rec + b"\n"


def run(text, cap=None, **kw):
    """What a call that succeeds gives: {"out", "keep", "rows", "figures"}; OverlapError otherwise (options, then the
    record count against cap, then an odd count, then the lowest malformed record)."""
    o = options(**kw)
    if o["mode"] not in (TRIM, MERGE) or not 1 <= o["min_overlap"] <= MAX_BASES or not 0 <= o["max_err_ppm"] <= 1000000:
        raise OverlapError(ERR_ARG)
    if o["which"] != 1 and not (o["which"] == 2 and o["mode"] == MERGE):
        raise OverlapError(ERR_ARG)
    recs, _ = records(text)
    if cap is not None and len(recs) > cap:
        raise OverlapError(ERR_RANGE, counts=(len(recs), cap))
    if len(recs) % 2:
        raise OverlapError(ERR_RANGE, counts=(len(recs),))
    bad = check(text)
    if bad:
        raise OverlapError(ERR_UNSUPPORTED, bad[0], bad[1])
    floor = max(o["min_len"], 1)
    rows, keep, out = [], [], []
    f = dict(records=len(recs), pairs=len(recs) // 2, pairs_hit=0, pairs_merged=0, pairs_trimmed=0, dropped_short=0, skipped_long=0,
             records_out=0, records_trimmed=0, bases_in=0, bases_out=0, lines=len(lines(text)))
    for p in range(len(recs) // 2):
        (h1, l1, p1, y1), (h2, l2, p2, y2) = recs[2 * p], recs[2 * p + 1]
        s1, q1, s2, q2 = content(l1), content(y1), content(l2), content(y2)
        f["bases_in"] += len(s1) + len(s2)
        f["skipped_long"] += len(s1) > MAX_BASES or len(s2) > MAX_BASES
        hit = find(s1, s2, o["min_overlap"], o["max_mismatch"], o["max_err_ppm"])
        if hit is None:
            rows += [(len(s1), len(s1), NO_HIT, 0, 0), (len(s2), len(s2), NO_HIT, 0, 0)]
            k = 1 if o["mode"] == TRIM else 2
        else:
            d, F, ov, mm = hit
            rows += [(len(s1), min(len(s1), F), F, ov, mm), (len(s2), min(len(s2), F), F, ov, mm)]
            f["pairs_hit"] += 1
            k = 1 if F >= floor else 0
            f["dropped_short"] += k == 0
            f["pairs_merged"] += o["mode"] == MERGE and k == 1
            f["pairs_trimmed"] += o["mode"] == TRIM and k == 1 and (F < len(s1) or F < len(s2))
        keep += [k, k]
        if k != o["which"]:
            continue
        if o["mode"] == MERGE and k == 1:
            seq, qual = merged(s1, q1, s2, q2, d)
            out.append(h1 + seq + b"\n" + p1 + qual + b"\n")
            f["records_out"] += 1
            f["records_trimmed"] += 1
            f["bases_out"] += len(seq)
            continue
        for r in (2 * p, 2 * p + 1):
            head, seq, plus, qual = recs[r]
            L, kept = rows[r][:2]
            if o["mode"] == MERGE or kept == L:
                out.append(whole(recs[r]))
                kept = L
            else:
                out.append(head + content(seq)[:kept] + b"\n" + plus + content(qual)[:kept] + b"\n")
                f["records_trimmed"] += 1
            f["records_out"] += 1
            f["bases_out"] += kept
    out = b"".join(out)
    f["bytes_out"] = len(out)
    return {"out": out, "keep": keep, "rows": rows, "figures": f}


def seen_by_the_count(text, mode, **kw):
    """The text the steps behind the overlap step see: the trimmed pairs (trim), or the merged reads followed by the
    unmerged pairs (merge)."""
    if mode == TRIM:
        return run(text, mode=TRIM, **kw)["out"]
    return run(text, mode=MERGE, which=1, **kw)["out"] + run(text, mode=MERGE, which=2, **kw)["out"]

