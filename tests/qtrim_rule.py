"""Plain-Python restatement of mk_fastq_qtrim_* (include/mercat_hip.h) over Python bytes: the running-sum quality
trimming of BWA -q / cutadapt -q 5',3' at both ends of every read of a FASTQ text, the span filters behind it, the pair
rule, the bytes that come out, rows, hist and the figures -- errors included.  Nothing here calls the library."""
from fastq_select_rule import content, lines, records

ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -7, -8
NO_LIMIT = 0xFFFFFFFF  # max_n: no limit
PHRASE = {"at": "does not start with '@'", "plus": "does not start with '+'", "length": "differ in length",
          "qual": "holds a character below the phred base", "incomplete": "the text ends inside it"}
OPT = dict(phred_base=33, cut_front=0, cut_back=20, min_len=0, max_n=NO_LIMIT, low_q=0, max_low_ppm=1000000, min_mean_q=0,
           paired=0, which=1)


class QtrimError(Exception):
    def __init__(self, code, record=None, kind=None, counts=None):
        super().__init__("code %d record %r kind %r counts %r" % (code, record, kind, counts))
        self.code, self.record, self.kind, self.counts = code, record, kind, counts


def options(**kw):
    """The options of a call: OPT with kw over it."""
    bad = set(kw) - set(OPT)
    if bad:
        raise TypeError("unknown option %r" % sorted(bad))
    return dict(OPT, **kw)


def cut(q, cut_front, cut_back):
    """(start, stop) of the quality values q (integers, the phred base taken off)."""
    L = len(q)
    s = best = start = 0
    for i in range(L):
        s += cut_front - q[i]
        if s < 0:
            break
        if s > best:
            best, start = s, i + 1
    s = best = 0
    stop = L
    for i in range(L - 1, -1, -1):
        s += cut_back - q[i]
        if s < 0:
            break
        if s > best:
            best, stop = s, i
    if start >= stop:
        start = stop = 0
    return start, stop


def judge(seq, q, start, stop, o):
    """(reason or None, n, low, qsum) of the span [start, stop): the first filter that applies names the reason."""
    kept = stop - start
    n = sum(1 for b in seq[start:stop] if b in b"Nn")
    low = sum(1 for v in q[start:stop] if v < o["low_q"])
    qsum = sum(q[start:stop])
    if kept < max(o["min_len"], 1):
        return "short", n, low, qsum
    if n > o["max_n"]:
        return "n", n, low, qsum
    if low * 1000000 > o["max_low_ppm"] * kept:
        return "lowq", n, low, qsum
    if qsum < o["min_mean_q"] * kept:
        return "meanq", n, low, qsum
    return None, n, low, qsum


def check(text, phred_base):
    """None, or (record, kind) of the lowest malformed record and the first check it fails."""
    recs, trailing = records(text)
    for r, (head, seq, plus, qual) in enumerate(recs):
        if not head.startswith(b"@"):
            return r, "at"
        if not plus.startswith(b"+"):
            return r, "plus"
        if len(content(seq)) != len(content(qual)):
            return r, "length"
        if any(b < phred_base for b in content(qual)):
            return r, "qual"
    if any(t != b"\n" for t in trailing):
        return len(recs), "incomplete"
    return None


def pair_keep(passes, paired):
    """keep[r] of the pass bits: unpaired the bit; paired 1 both mates, 2 only r, 0 otherwise."""
    if not paired:
        return [1 if p else 0 for p in passes]
    return [0 if not p else 1 if passes[r ^ 1] else 2 for r, p in enumerate(passes)]


def run(text, cap=None, **kw):
    """What a call that succeeds gives: {"out", "keep", "rows", "hist", "reasons", "figures"}; QtrimError otherwise
    (arguments, then the record count against cap, then an odd count with paired, then the lowest malformed record)."""
    o = options(**kw)
    if o["phred_base"] not in (33, 64) or not 0 <= o["cut_front"] <= 93 or not 0 <= o["cut_back"] <= 93:
        raise QtrimError(ERR_ARG)
    if o["which"] not in (1, 2) or (o["which"] == 2 and not o["paired"]) or o["max_low_ppm"] > 1000000:
        raise QtrimError(ERR_ARG)
    recs, _ = records(text)
    if cap is not None and len(recs) > cap:
        raise QtrimError(ERR_RANGE, counts=(len(recs), cap))
    if o["paired"] and len(recs) % 2:
        raise QtrimError(ERR_RANGE, counts=(len(recs),))
    bad = check(text, o["phred_base"])
    if bad:
        raise QtrimError(ERR_UNSUPPORTED, bad[0], bad[1])
    rows, reasons, spans = [], [], []
    hist = [0] * 512
    for head, seq, plus, qual in recs:
        s, q = content(seq), [b - o["phred_base"] for b in content(qual)]
        start, stop = cut(q, o["cut_front"], o["cut_back"])
        reason, n, low, qsum = judge(s, q, start, stop, o)
        rows.append((len(s), start, stop - start, n, low, qsum))
        reasons.append(reason)
        spans.append(q[start:stop])
        for v in q:
            hist[v] += 1
    keep = pair_keep([r is None for r in reasons], o["paired"])
    out = []
    f = dict(records=len(recs), records_out=0, records_trimmed=0, dropped_short=0, dropped_n=0, dropped_lowq=0, dropped_meanq=0,
             orphans=keep.count(2), bases_in=sum(r[0] for r in rows), bases_out=0, lines=len(lines(text)))
    for r, (head, seq, plus, qual) in enumerate(recs):
        L, start, kept = rows[r][:3]
        if reasons[r]:
            f["dropped_" + reasons[r]] += 1
        if keep[r] != o["which"]:
            continue
        if start == 0 and kept == L:
            rec = head + seq + plus + qual
            out.append(rec if rec.endswith(b"\n") else rec + b"\n")
        else:
            out.append(head + content(seq)[start:start + kept] + b"\n" + plus + content(qual)[start:start + kept] + b"\n")
            f["records_trimmed"] += 1
        f["records_out"] += 1
        f["bases_out"] += kept
        for v in spans[r]:
            hist[256 + v] += 1
    out = b"".join(out)
    f["bytes_out"] = len(out)
    return {"out": out, "keep": keep, "rows": rows, "hist": hist, "reasons": reasons, "figures": f}


def pair_cuts(text, piece):
    """Where mk_fastq_pair_cuts cuts: behind a line 8j once the piece holds `piece` bytes, strictly inside the text."""
    out, at, start = [], 0, 0
    for i, line in enumerate(lines(text)):
        at += len(line)
        if i % 8 == 7 and at < len(text) and at - start >= piece:
            out.append(at)
            start = at
    return out
