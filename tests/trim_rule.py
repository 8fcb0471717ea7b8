"""The rule of mk_trim_* (include/mercat_hip.h) restated over Python bytes and a dict: what the tests compare
Counter.trim with.  Nothing here touches the library.

The text is read by the reference's line loop (lib/mercat2_kmers.py:49-69, as tests/test_gpu_track.ref_records does):
lines end at LF, CR LF or a lone CR; a line whose stripped form starts with '>' opens a record; every other line gives
``line.strip().replace("*", "")`` to the record it stands in -- to a leading record without a header line if none is
open yet.  Here the lines keep their bytes, because an emitted record starts with its header line as it stands."""
import re

_LINE = re.compile(rb"[^\r\n]*(?:\r\n|\r|\n)|[^\r\n]+")
_BLANKS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"  # what str.strip() removes from ASCII text
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def records(text: bytes):
    """[(header line with its terminator -- b"" for the headless record --, kept characters)] in text order."""
    recs = []
    for line in _LINE.findall(bytes(text)):
        stripped = line.strip(_BLANKS)
        if stripped.startswith(b">"):
            recs.append([line, b""])
        else:
            piece = stripped.replace(b"*", b"")
            if not recs and piece:
                recs.append([b"", b""])
            if recs:
                recs[-1][1] += piece
    return [(header, seq) for header, seq in recs]


def count_of(table: dict, window: bytes, fold: bool) -> int:
    if fold and set(window) <= set(b"ACGT"):
        window = min(window, window.translate(_COMP)[::-1])
    return table.get(window.decode("latin-1"), 0)


def kept_of(seq: bytes, table: dict, k: int, at_least: int, min_len: int = 0, fold: bool = False) -> int:
    """Characters a record keeps: all of them without a low window; j + k - 1 with the first low window at j >= 1; none
    with j = 0 or without windows; none if fewer than max(min_len, k) would remain."""
    windows = len(seq) - k + 1
    if windows <= 0:
        return 0
    kept = len(seq)
    for j in range(windows):
        if count_of(table, seq[j:j + k], fold) < at_least:
            kept = j + k - 1 if j else 0
            break
    return kept if kept >= max(min_len, k) else 0


def expected(text: bytes, table: dict, k: int, at_least: int, min_len: int = 0, fold: bool = False):
    """(output bytes, [kept per record]): an emitted record is its header line, its first kept characters and one LF."""
    out, kept = [], []
    for header, seq in records(text):
        n = kept_of(seq, table, k, at_least, min_len, fold)
        kept.append(n)
        if n:
            out.append(header + seq[:n] + b"\n")
    return b"".join(out), kept
