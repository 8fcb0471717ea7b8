"""The rule of tests/orf_rule.py restated on numpy, for texts of megabases: the same signature and the same result as
orf_rule.expected, a few hundred times faster.  Nothing here touches the library.  tests/test_orf_scale_host.py
compares the two restatements with each other; orf_rule.py stays the definition.

Per record, strand and class: codes by a 256-entry table, codon indices by reshaping to (n, 3), stops by flatnonzero,
stretches as the gaps between them (the empty ones included), the first start of a stretch by searchsorted; then one
sort by (right end, strand).  Like the plain rule the reverse strand is done on a reverse-complemented copy and its
coordinates turned round afterwards."""
import re

import numpy as np

from orf_rule import _BLANKS, _LINE, ALT, CODON_TABLE, MINUS, PLUS, START

_NAME = re.compile(rb"[^\x00-\x20]*")  # a header's bytes up to the first one <= 0x20
_CODE = np.full(256, 4, dtype=np.uint8)  # A 0, C 1, G 2, T and U 3 in either case, every other byte 4
for _i, _letters in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
    for _b in _letters:
        _CODE[_b] = _i
_AMINO = np.frombuffer(CODON_TABLE.encode() + b"X", dtype=np.uint8)  # index 64: a codon with a byte that is no base
_STOP = ord("*")


def records(text: bytes):
    """orf_rule.records, with a record's lines joined once at its end: that one appends line by line, which on a record
    of megabases copies the record once a line."""
    recs = []
    for line in _LINE.findall(bytes(text)):
        stripped = line.strip(_BLANKS)
        if stripped.startswith(b">"):
            recs.append([stripped[1:], []])
        else:
            piece = stripped.replace(b"*", b"")
            if not recs and piece:
                recs.append([b"", []])
            if recs:
                recs[-1][1].append(piece)
    return [(_NAME.match(head).group(), b"".join(pieces)) for head, pieces in recs]


def codon_indices(cs: np.ndarray, c: int) -> np.ndarray:
    """16 c1 + 4 c2 + c3 of every codon of class c of the coded string cs, 64 where one of the three is no base."""
    n = max(0, (len(cs) - c) // 3)
    tri = cs[c:c + 3 * n].reshape(n, 3).astype(np.intp)
    idx = 16 * tri[:, 0] + 4 * tri[:, 1] + tri[:, 2]
    idx[(tri > 3).any(axis=1)] = 64
    return idx


def record_orfs(seq: bytes, min_aa: int = 32, flags: int = 0):
    """(begin, aa, frame -- three int64 arrays in the rule's order --, [amino acids as bytes])."""
    assert min_aa >= 1
    assert not (flags & ALT) or (flags & START)
    assert not ((flags & PLUS) and (flags & MINUS))
    L = len(seq)
    fwd = _CODE[np.frombuffer(seq, dtype=np.uint8)]
    rev = np.where(fwd < 4, 3 - fwd, 4).astype(np.uint8)[::-1]
    starts = [14] + ([46, 62] if flags & ALT else [])  # ATG; GTG TTG
    strings = []  # the translation of every (strand, class) that is looked at
    cols = [[] for _ in range(7)]  # right end, strand, begin, aa, frame, index into strings, first codon
    for strand, cs in ((0, fwd), (1, rev)):
        if (strand == 0 and flags & MINUS) or (strand == 1 and flags & PLUS):
            continue
        for c in range(3):
            idx = codon_indices(cs, c)
            amino = _AMINO[idx]
            stops = np.flatnonzero(amino == _STOP)
            first = np.concatenate(([0], stops + 1))      # stretch i holds the codons [first[i], end[i])
            end = np.concatenate((stops, [len(idx)]))
            opens = first                                  # (the order goes by the stretch, not by what a start leaves of it)
            if flags & START:
                at_start = np.flatnonzero(np.isin(idx, starts))
                j = np.searchsorted(at_start, first)       # the first start at or behind the stretch's first codon
                padded = np.concatenate((at_start, [len(idx)]))
                first = np.minimum(padded[j], end)         # (none inside the stretch: nothing is left of it)
            keep = end - first >= min_aa
            first, end, opens = first[keep], end[keep], opens[keep]
            a, b = c + 3 * first, c + 3 * end              # in the coordinates of cs
            cols[0].append(b if strand == 0 else L - (c + 3 * opens))
            cols[1].append(np.full(len(a), strand))
            cols[2].append(a if strand == 0 else L - b)
            cols[3].append(end - first)
            cols[4].append(np.full(len(a), (1 if strand == 0 else 4) + c))
            cols[5].append(np.full(len(a), len(strings)))
            cols[6].append(first)
            strings.append(amino.tobytes())
    right, strand, begin, aa, frame, which, first = (np.concatenate(col).astype(np.int64) for col in cols)
    order = np.lexsort((strand, right))
    key = right[order] * 2 + strand[order]
    assert (key[1:] > key[:-1]).all()  # one ORF a closing (position, strand)
    which, first, aa = which[order], first[order], aa[order]
    aas = [strings[w][f:f + n] for w, f, n in zip(which.tolist(), first.tolist(), aa.tolist())]
    return begin[order], aa, frame[order], aas


def expected_np(text: bytes, min_aa: int = 32, start: bool = False, alt_starts: bool = False, strand: str = "both"):
    """(output bytes, the rows as an (n, 4) uint64 array: record, begin, aa, frame) of a whole text."""
    flags = (START if start else 0) | (ALT if alt_starts else 0) | {"both": 0, "plus": PLUS, "minus": MINUS}[strand]
    out, rows = [], [np.zeros((0, 4), dtype=np.uint64)]
    for r, (name, seq) in enumerate(records(text)):
        begin, aa, frame, aas = record_orfs(seq, min_aa, flags)
        head = b">" + name
        out.extend(head + b"_%d_%d_%d\n" % (b + 1, f, n) + s + b"\n" for n, (b, f, s) in enumerate(zip(begin.tolist(), frame.tolist(), aas), 1))
        rows.append(np.stack((np.full(len(aa), r, dtype=np.int64), begin, aa, frame), axis=1).astype(np.uint64))
    return b"".join(out), np.concatenate(rows)


def expected(text: bytes, min_aa: int = 32, start: bool = False, alt_starts: bool = False, strand: str = "both"):
    """(output bytes, [[record, begin, aa, frame]]) of a whole text: orf_rule.expected."""
    out, rows = expected_np(text, min_aa, start, alt_starts, strand)
    return out, rows.tolist()
