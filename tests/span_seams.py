"""Texts whose runs of windows end on the seams of the queue scatter's analysis (mk_sk_scatterq_k), and a plain
restatement of the symbol stream they make.  A helper module (like walk_seams.py): nothing here touches the library or a GPU.

The parsed stream holds one separator where a header line starts, then the kept characters: in a text of one record on
one line, base b sits at stream position b + 1 and window 0 is invalid (it holds the separator).  An analysis thread owns
the 32 windows that start at stream positions 32 t .. 32 t + 31, a wave 64 threads, a sub-tile 512 threads, a tile two or
three sub-tiles.  tests/test_span_seams_host.py checks that the texts place what is claimed here;
tests/test_gpu_span_records.py counts them on the GPU."""
import functools

import numpy as np

R, WAVE, SUBT = 32, 64, 512
SHIFTS = (-1, 0, 1, 31, 33)
SPANS_OF_WINDOWS = (R * WAVE * 3, R * SUBT * 3)  # 3 waves; 3 sub-tiles: a tile seam at thread 1024 (two sub-tiles) and 1536
N_ENDS = (R * 70 + 31, R * 70 + 32, R * 128)     # last invalid window: window 31 of a thread, window 0 of the next, window 0 of a wave's first thread
HOMOPOLYMER = 5000


def one_line(bases) -> bytes:
    return b">s\n" + bytes(bases) + b"\n"


def stream_of(text: bytes):
    """(sym 0..3, bad) of a one-record, one-line text: the separator, then the bases (N is kept, and bad)."""
    head, seq, rest = text.split(b"\n")
    assert head.startswith(b">") and rest == b""
    raw = np.frombuffer(seq, dtype=np.uint8)
    code = np.full(256, -1, dtype=np.int64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    sym = np.concatenate(([-1], code[raw]))
    bad = sym < 0
    sym[bad] = 0
    return sym, bad


@functools.lru_cache(maxsize=None)
def seam_texts(k: int):
    """[(name, text)].  'w<L><d>': random bases whose LAST valid window starts at stream position L + d - 1, so that
    with d = 0 it is window 31 of the last thread before the seam at L windows, with d = -1 the window before it, with
    d = 1 window 0 of the thread behind the seam.  'N@<p>': a single N at stream position p, which makes the windows
    p - k + 1 .. p invalid.  'homopolymer': A x 5000."""
    rng = np.random.default_rng(1234 + k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    texts = []
    for windows in SPANS_OF_WINDOWS:
        for d in SHIFTS:
            # stream length 1 + bases; the last window starts at 1 + bases - k = windows + d - 1
            texts.append(("w%d%+d" % (windows, d), one_line(acgt[rng.integers(0, 4, windows + d + k - 2)])))
    base = acgt[rng.integers(0, 4, R * WAVE * 3 + k - 2)]
    for at in N_ENDS:
        text = base.copy()
        text[at - 1] = ord("N")  # base at - 1 is stream position at
        texts.append(("N@%d" % at, one_line(text)))
    texts.append(("homopolymer", one_line(b"A" * HOMOPOLYMER)))
    return texts
