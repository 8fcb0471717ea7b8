"""The rule of mk_correct_* (include/mercat_hip.h) restated over Python bytes and a dict: what the tests compare
Counter.correct with.  Nothing here touches the library.  The text is read as tests/trim_rule.py reads it, a window's
count is trim_rule.count_of."""
import trim_rule

BASES = b"ACGT"


def runs_of(weak):
    """[(a, b)]: the maximal intervals of True in ``weak``."""
    out, a = [], None
    for j, w in enumerate(list(weak) + [False]):
        if w and a is None:
            a = j
        elif not w and a is not None:
            out.append((a, j - 1))
            a = None
    return out


def candidate_of(a: int, b: int, windows: int, k: int):
    """The position a run [a, b] of a record of ``windows`` windows names, or None."""
    n = b - a + 1
    if a == 0 and b == windows - 1:
        return None
    if a == 0:
        return b if n <= k else None
    if b == windows - 1:
        return a + k - 1 if n <= k else None
    return b if n == k else None


def weak_of(seq: bytes, table: dict, k: int, at_least: int, fold: bool):
    return [trim_rule.count_of(table, seq[j:j + k], fold) < at_least for j in range(len(seq) - k + 1)]


def judge(seq: bytes, a: int, b: int, p: int, table: dict, k: int, at_least: int, fold: bool):
    """The viable alternatives at p for the run [a, b]: bytes of ACGT other than seq[p]."""
    viable = []
    for x in BASES:
        if x == seq[p]:
            continue
        changed = seq[:p] + bytes([x]) + seq[p + 1:]
        if all(trim_rule.count_of(table, changed[j:j + k], fold) >= at_least for j in range(a, b + 1)):
            viable.append(x)
    return viable


def correct_seq(seq: bytes, table: dict, k: int, at_least: int, fold: bool = False, only=None):
    """(corrected characters, (runs, fixed, ambiguous, unfixable)): every run judged against ``seq`` as it came, the fixes
    applied together.  only: the index of the one run to apply (the others are judged and counted, not applied)."""
    runs = runs_of(weak_of(seq, table, k, at_least, fold))
    windows = len(seq) - k + 1
    out = bytearray(seq)
    fixed = ambiguous = unfixable = 0
    for i, (a, b) in enumerate(runs):
        p = candidate_of(a, b, windows, k)
        if p is None:
            continue
        assert a <= p < a + k and b <= p  # every window of the run holds p
        viable = judge(seq, a, b, p, table, k, at_least, fold)
        if len(viable) == 1:
            fixed += 1
            if only is None or only == i:
                out[p] = viable[0]
        elif viable:
            ambiguous += 1
        else:
            unfixable += 1
    return bytes(out), (len(runs), fixed, ambiguous, unfixable)


def expected(text: bytes, table: dict, k: int, at_least: int, fold: bool = False):
    """(output bytes, [(runs, fixed, ambiguous, unfixable) per record]): every record is its header line, then -- if it
    has characters -- those on one line and one LF."""
    out, rows = [], []
    for header, seq in trim_rule.records(text):
        fixed_seq, row = correct_seq(seq, table, k, at_least, fold)
        rows.append(row)
        out.append(header + (fixed_seq + b"\n" if fixed_seq else b""))
    return b"".join(out), rows
