"""Plain-Python restatement of mk_fastq_adapt_* (include/mercat_hip.h) over Python bytes: the leftmost admissible 3'
adapter of every read of a FASTQ text, byte by byte, the cut, the pair rule, the bytes that come out, rows, hits and the
figures -- errors included.  Nothing here calls the library."""
from fastq_select_rule import content, lines, records
from qtrim_rule import pair_keep

ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -7, -8
NO_HIT = 0xFFFFFFFF
PHRASE = {"at": "does not start with '@'", "plus": "does not start with '+'", "length": "differ in length",
          "incomplete": "the text ends inside it"}
OPT = dict(min_overlap=8, max_err_ppm=100000, min_len=0, paired=0, which=1)


class AdaptError(Exception):
    def __init__(self, code, record=None, kind=None, counts=None, adapter=None):
        super().__init__("code %d record %r kind %r counts %r adapter %r" % (code, record, kind, counts, adapter))
        self.code, self.record, self.kind, self.counts, self.adapter = code, record, kind, counts, adapter


def options(**kw):
    """The options of a call: OPT with kw over it."""
    bad = set(kw) - set(OPT)
    if bad:
        raise TypeError("unknown option %r" % sorted(bad))
    return dict(OPT, **kw)


def fold(b):
    """A byte with a .. z folded to upper case."""
    return b - 32 if 97 <= b <= 122 else b


def check_adapters(adapters, mates):
    """The adapters as upper-case bytes and their classes, or AdaptError(ERR_ARG) naming the first one refused."""
    if not 1 <= len(adapters) <= 1024:
        raise AdaptError(ERR_ARG)
    mates = [1] * len(adapters) if mates is None else list(mates)
    out = []
    for a, (seq, cls) in enumerate(zip(adapters, mates)):
        seq = bytes(fold(b) for b in seq)
        if not 1 <= len(seq) <= 128 or cls not in (1, 2, 3) or any(b not in b"ACGTN" for b in seq):
            raise AdaptError(ERR_ARG, adapter=a)
        out.append(seq)
    return out, mates


def mismatches(s, i, adapter, max_err_ppm=None):
    """(ov, mism) of the adapter at position i of the read s (folded bytes).  With max_err_ppm the count stops at the
    first mismatch beyond what that rate admits (mism <= max_err_ppm * ov // 1000000 is the admissibility test in
    integers): the adapter is then not admissible, and the count says only that."""
    ov = min(len(adapter), len(s) - i)
    limit = ov if max_err_ppm is None else max_err_ppm * ov // 1000000
    mism = 0
    for j in range(ov):
        if adapter[j] != 78 and adapter[j] != s[i + j]:
            mism += 1
            if mism > limit:
                break
    return ov, mism


def find(s, adapters, mates, cls, min_overlap, max_err_ppm):
    """(cut, adapter, overlap, mismatches) of the read s of mate class cls: the smallest i with an admissible adapter and
    the lowest adapter admissible there; (len(s), NO_HIT, 0, 0) without one."""
    s = bytes(fold(b) for b in s)
    for i in range(len(s)):
        if len(s) - i < min_overlap:
            break
        for a, adapter in enumerate(adapters):
            if not mates[a] & cls:
                continue
            if min(len(adapter), len(s) - i) < min_overlap:
                continue
            ov, mism = mismatches(s, i, adapter, max_err_ppm)
            if ov >= min_overlap and mism * 1000000 <= max_err_ppm * ov:
                return i, a, ov, mism
    return len(s), NO_HIT, 0, 0


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


def run(text, adapters, mates=None, cap=None, **kw):
    """What a call that succeeds gives: {"out", "keep", "rows", "hits", "figures"}; AdaptError otherwise (options, then
    the adapters, then the record count against cap, then an odd count with paired, then the lowest malformed record)."""
    o = options(**kw)
    if not 1 <= o["min_overlap"] <= 128 or not 0 <= o["max_err_ppm"] <= 1000000:
        raise AdaptError(ERR_ARG)
    if o["which"] not in (1, 2) or (o["which"] == 2 and not o["paired"]):
        raise AdaptError(ERR_ARG)
    adapters, mates = check_adapters(adapters, mates)
    recs, _ = records(text)
    if cap is not None and len(recs) > cap:
        raise AdaptError(ERR_RANGE, counts=(len(recs), cap))
    if o["paired"] and len(recs) % 2:
        raise AdaptError(ERR_RANGE, counts=(len(recs),))
    bad = check(text)
    if bad:
        raise AdaptError(ERR_UNSUPPORTED, bad[0], bad[1])
    rows, hits = [], [0] * len(adapters)
    for r, (head, seq, plus, qual) in enumerate(recs):
        s = content(seq)
        cut, a, ov, mism = find(s, adapters, mates, 2 if o["paired"] and r % 2 else 1, o["min_overlap"], o["max_err_ppm"])
        rows.append((len(s), cut, a, ov, mism))
        if a != NO_HIT:
            hits[a] += 1
    passes = [row[1] >= max(o["min_len"], 1) for row in rows]
    keep = pair_keep(passes, o["paired"])
    out = []
    f = dict(records=len(recs), records_out=0, records_trimmed=0, dropped_short=passes.count(False), orphans=keep.count(2),
             bases_in=sum(r[0] for r in rows), bases_out=0, lines=len(lines(text)))
    for r, (head, seq, plus, qual) in enumerate(recs):
        L, cut = rows[r][:2]
        if keep[r] != o["which"]:
            continue
        if cut == L:
            rec = head + seq + plus + qual
            out.append(rec if rec.endswith(b"\n") else rec + b"\n")
        else:
            out.append(head + content(seq)[:cut] + b"\n" + plus + content(qual)[:cut] + b"\n")
            f["records_trimmed"] += 1
        f["records_out"] += 1
        f["bases_out"] += cut
    out = b"".join(out)
    f["bytes_out"] = len(out)
    return {"out": out, "keep": keep, "rows": rows, "hits": hits, "figures": f}
