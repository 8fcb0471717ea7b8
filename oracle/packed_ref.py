"""numpy restatements for the running-table tests (test infrastructure only).

- mk_mix64 (mercat2_amd/csrc/mk_common.h), its inverse, and home128 (mk_table.hip): hostile key sets are built by
  choosing where a key's probe sequence starts and solving for the key.
- A vectorised k-mer counter over 2-bit packed windows of synthetic reads (fixed-length, one-line ACGT records, as
  native.synth_reads writes them): the same table as the C oracle for such text, fast enough for tens of millions of
  distinct keys.  Keys are one word for k <= 32 (2 k bits, right-aligned) and (hi, lo) for 33 <= k <= 64 (bases 0..31
  in hi, the rest in lo, both left-aligned) -- the packing of the engine's tables, so key order is k-mer text order.
"""
from typing import List, Sequence, Tuple

import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1
MIX_M1 = 0xBF58476D1CE4E5B9
MIX_M2 = 0x94D049BB133111EB
POLY_B = 0x9E3779B97F4A7C15
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _u(x) -> np.ndarray:
    return np.asarray(x, dtype=U64)


def mix64(x) -> np.ndarray:
    """mk_mix64, element-wise (uint64 arithmetic wraps as on the device)."""
    x = _u(x).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(30)
        x *= U64(MIX_M1)
        x ^= x >> U64(27)
        x *= U64(MIX_M2)
        x ^= x >> U64(31)
    return x


def _unxorshift(y: np.ndarray, s: int) -> np.ndarray:
    x = y.copy()
    for _ in range(64 // s + 1):  # (each round fixes s more of the top bits)
        x = y ^ (x >> U64(s))
    return x


def unmix64(y) -> np.ndarray:
    """The inverse of mk_mix64: unmix64(mix64(x)) == x."""
    x = _u(y).copy()
    with np.errstate(over="ignore"):
        x = _unxorshift(x, 31)
        x *= U64(pow(MIX_M2, -1, 1 << 64))
        x = _unxorshift(x, 27)
        x *= U64(pow(MIX_M1, -1, 1 << 64))
        x = _unxorshift(x, 30)
    return x


def home128(hi, lo, mask: int) -> np.ndarray:
    """Home slot of a two-word key in a table of mask + 1 slots (mk_table.hip home128)."""
    with np.errstate(over="ignore"):
        return mix64(_u(hi) ^ mix64(_u(lo) + U64(POLY_B))) & U64(mask)


def hi_for_mix(lo, mixed) -> np.ndarray:
    """The hi word that gives a key with this lo the value ``mixed`` of mix64(hi ^ mix64(lo + B)), the number whose low
    bits home128 keeps."""
    with np.errstate(over="ignore"):
        return unmix64(mixed) ^ mix64(_u(lo) + U64(POLY_B))


# ----------------------------------------------------------------------------------------------- packed keys -> text
def decode64(keys, k: int, bits: int = 2) -> np.ndarray:
    """(rows, k) uint8 text of one-word keys (nucleotides: ACGT; bits = 5: 'A' + code)."""
    keys = _u(keys)
    out = np.empty((keys.size, k), dtype=np.uint8)
    m = U64((1 << bits) - 1)
    for j in range(k):
        code = (keys >> U64(bits * (k - 1 - j))) & m
        out[:, j] = ACGT[code] if bits == 2 else (code + U64(ord("A"))).astype(np.uint8)
    return out


def decode128(hi, lo, k: int) -> np.ndarray:
    """(rows, k) uint8 text of two-word nucleotide keys."""
    hi, lo = _u(hi), _u(lo)
    out = np.empty((hi.size, k), dtype=np.uint8)
    for j in range(k):
        w, s = (hi, 62 - 2 * j) if j < 32 else (lo, 62 - 2 * (j - 32))
        out[:, j] = ACGT[(w >> U64(s)) & U64(3)]
    return out


# ------------------------------------------------------------------------------------------------------- reductions
def reduce_rows(words: Sequence[np.ndarray], counts: np.ndarray) -> Tuple[List[np.ndarray], np.ndarray]:
    """Sum the counts of equal keys (one or two key words, compared in order) and drop rows whose sum is 0: the
    distinct keys in ascending order and their sums.  This is np.unique plus a sum per key, for keys of two words."""
    counts = _u(counts)
    if counts.size == 0:
        return [np.zeros(0, U64) for _ in words], np.zeros(0, U64)
    order = np.lexsort(tuple(reversed([_u(w) for w in words]))) if len(words) > 1 else np.argsort(words[0], kind="stable")
    ws = [_u(w)[order] for w in words]
    new = np.zeros(counts.size, dtype=bool)
    new[0] = True
    for w in ws:
        new[1:] |= w[1:] != w[:-1]
    first = np.flatnonzero(new)
    sums = np.add.reduceat(counts[order], first).astype(U64)
    keep = sums != 0
    return [w[first][keep] for w in ws], sums[keep]


# --------------------------------------------------------------------------------------------------- the counter
def read_codes(text: bytes) -> np.ndarray:
    """(reads, L) 2-bit codes of a text of fixed-length one-line ACGT records ('>name' line, sequence line); raises
    AssertionError for any other form (the counter below is only exact for that form)."""
    buf = np.frombuffer(text, dtype=np.uint8)
    assert buf.size and buf[0] == ord(">") and buf[-1] == ord("\n"), "not a FASTA text ending in a newline"
    nl = np.flatnonzero(buf == ord("\n"))
    assert nl.size % 2 == 0, "records are not header line + one sequence line"
    starts = np.concatenate(([0], nl[:-1] + 1))
    seq_lo, seq_hi = starts[1::2], nl[1::2]
    assert np.all(buf[starts[0::2]] == ord(">")) and not np.any(buf[seq_lo] == ord(">")), "headers and sequences do not alternate"
    lens = seq_hi - seq_lo
    L = int(lens[0])
    assert np.all(lens == L), "reads are not of one length"
    idx = seq_lo[:, None] + np.arange(L)[None, :]
    seq = buf[idx]
    lut = np.full(256, 255, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    codes = lut[seq]
    assert not np.any(codes == 255), "a read holds a symbol other than A, C, G, T"
    return codes


def _windows(codes: np.ndarray, k: int, first: int, n: int, left: int) -> np.ndarray:
    """Keys of bases first..first+n-1 of every window, packed 2 bits a base, shifted left by 2 * left bits."""
    W = codes.shape[1] - k + 1
    key = np.zeros((codes.shape[0], W), dtype=U64)
    for j in range(first, first + n):
        key <<= U64(2)
        key |= codes[:, j:j + W]
    if left:
        key <<= U64(2 * left)
    return key.reshape(-1)


def window_keys(codes: np.ndarray, k: int, canonical: bool = False) -> List[np.ndarray]:
    """Every window's key: [keys] for k <= 32, [hi, lo] for 33 <= k <= 64; with ``canonical`` the smaller of the key and
    the key of its reverse complement."""
    assert 1 <= k <= 64 and codes.shape[1] >= k

    def fwd(c):
        if k <= 32:
            return [_windows(c, k, 0, k, 0)]
        return [_windows(c, k, 0, 32, 0), _windows(c, k, 32, k - 32, 64 - k)]

    f = fwd(codes)
    if not canonical:
        return f
    # window i of the reverse complement read is the reverse complement of window W-1-i of the read
    r = [w.reshape(codes.shape[0], -1)[:, ::-1].reshape(-1) for w in fwd(np.ascontiguousarray(3 - codes[:, ::-1]))]
    if k <= 32:
        return [np.minimum(f[0], r[0])]
    take_r = (r[0] < f[0]) | ((r[0] == f[0]) & (r[1] < f[1]))
    return [np.where(take_r, r[0], f[0]), np.where(take_r, r[1], f[1])]


def unique_counts(words: Sequence[np.ndarray]) -> Tuple[List[np.ndarray], np.ndarray]:
    """reduce_rows with every count 1 -- the distinct keys in ascending order and how often each occurs -- fast enough
    for ~10^8 windows: one unstable sort of the first word (one-word keys: of the keys themselves), then the runs of
    equal first words, and only they, put in order of the second word."""
    if len(words) == 1:
        s = np.sort(_u(words[0]))
        h, rest = s, []
    else:
        order = np.argsort(_u(words[0]))
        h = _u(words[0])[order]
        l_ = _u(words[1])[order]
        del order
        eq = h[1:] == h[:-1]
        multi = np.zeros(h.size, dtype=bool)
        multi[1:] |= eq
        multi[:-1] |= eq
        idx = np.flatnonzero(multi)
        # (the runs keep their places: h is sorted, so sorting the subset by (h, l) only reorders inside each run)
        l_[idx] = l_[idx][np.lexsort((l_[idx], h[idx]))]
        rest = [l_]
    if h.size == 0:
        return [h] + rest, np.zeros(0, U64)
    new = np.ones(h.size, dtype=bool)
    new[1:] = h[1:] != h[:-1]
    for w in rest:
        new[1:] |= w[1:] != w[:-1]
    first = np.flatnonzero(new)
    counts = np.diff(np.append(first, h.size)).astype(U64)
    return [h[first]] + [w[first] for w in rest], counts


def count_chunk(text: bytes, k: int, min_count: int, canonical: bool = False) -> Tuple[List[np.ndarray], np.ndarray]:
    """One chunk's table, filtered by its own min_count: (key words, counts) in key order."""
    keys, counts = unique_counts(window_keys(read_codes(text), k, canonical))
    keep = counts >= U64(max(min_count, 1))
    return [w[keep] for w in keys], counts[keep]


def merge_tables(tables: Sequence[Tuple[List[np.ndarray], np.ndarray]]) -> Tuple[List[np.ndarray], np.ndarray]:
    """The sum of filtered chunk tables (no filter after the sum: cpu_ref.merge_counts)."""
    nw = len(tables[0][0])
    words = [np.concatenate([t[0][i] for t in tables]) for i in range(nw)]
    return reduce_rows(words, np.concatenate([t[1] for t in tables]))


def count_sample(texts: Sequence[bytes], k: int, min_count: int, canonical: bool = False) -> Tuple[List[np.ndarray], np.ndarray]:
    """Chunks counted one by one, each filtered by min_count, then summed -- a sample as the reference counts it."""
    return merge_tables([count_chunk(t, k, min_count, canonical) for t in texts])


def count_sample_c1(texts: Sequence[bytes], k: int) -> Tuple[List[np.ndarray], np.ndarray]:
    """count_sample(texts, k, 1) in one reduction: with min_count 1 the per-chunk filter keeps every row, so the sum of
    the chunk tables is the count of all the windows together (for samples of 10^8 windows)."""
    parts = [window_keys(read_codes(t), k) for t in texts]
    words = [np.concatenate([p[i] for p in parts]) for i in range(len(parts[0]))]
    del parts
    return unique_counts(words)


def as_text(keys: Sequence[np.ndarray], k: int) -> np.ndarray:
    """(rows, k) uint8 text of packed nucleotide keys, in the key order given."""
    return decode64(keys[0], k) if len(keys) == 1 else decode128(keys[0], keys[1], k)
