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


# ------------------------------------------------------------------------------------ hostile keys for the LDS tables
# Restatements of the slot hashes of the per-chunk LDS count kernels, and solvers that return distinct keys sharing a
# kernel's bucket, its home slot and every split bit.  All arithmetic is on uint64 arrays.
M32 = 0xFFFFFFFF
M24 = 0xFFFFFF
SK_M = 11                                   # minimizer length (mk_skmer_dev.h)
SK_ORDER_MUL, SK_ORDER_ADD = 0x9277B5, 0x2C5A3D
# the one 11-mer whose minimizer order (the low 22 bits of sk_order_raw) is 0: every window that holds it is filed under it
M_STAR = (-SK_ORDER_ADD * pow(SK_ORDER_MUL, -1, 1 << 22)) % (1 << 22)
CNT_SLOTS, SKC_SLOTS, SK2C_SLOTS, SK2P_SLOTS = 8192, 8192, 6144, 2048


def umul24(a, b) -> np.ndarray:
    """__umul24: the low 32 bits of the product of the low 24 bits of each operand."""
    with np.errstate(over="ignore"):
        return ((_u(a) & U64(M24)) * (_u(b) & U64(M24))) & U64(M32)


def sk_order_raw(mm) -> np.ndarray:
    """mk_skmer_dev.h sk_order_raw (32 bits; minimizers are compared on the low 22)."""
    return (umul24(mm, SK_ORDER_MUL) + U64(SK_ORDER_ADD)) & U64(M32)


def sk_bucket(mm, p1_log2: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return ((_u(mm) * U64(0xC2B2AE3D)) & U64(M32)) >> U64(32 - p1_log2)


def _three(w) -> np.ndarray:
    """The three 24-bit multiplies of skc_hash over one 64-bit word."""
    w = _u(w)
    return umul24(w & U64(M32), 0x9E3779) ^ umul24((w >> U64(24)) & U64(M32), 0x85EBCB) ^ umul24(w >> U64(48), 0xC2B2AF)


def skc_hash(key) -> np.ndarray:
    """mk_skcount.hip skc_hash: bits 31..19 pick the slot (8192 slots), bits 15..0 the sub-range."""
    return _three(key)


def skc_home(h) -> np.ndarray:
    return _u(h) >> U64(19)


def _sk2_pre(hi, lo) -> np.ndarray:
    hi, lo = _u(hi), _u(lo)
    return (_three(hi) ^ umul24(lo & U64(M32), 0x27D4EB) ^ umul24((lo >> U64(24)) & U64(M32), 0x165667) ^
            umul24(lo >> U64(48), 0x2C1B3D))


def sk2c_hash(hi, lo) -> np.ndarray:
    """mk_skmer2.hip sk2c_hash."""
    h = _sk2_pre(hi, lo)
    return h ^ (h >> U64(15))


def sk2c_home(h) -> np.ndarray:
    return (_u(h) * U64(SK2C_SLOTS)) >> U64(32)


def rotr64(x, r: int) -> np.ndarray:
    x = _u(x)
    return (x >> U64(r)) | (x << U64(64 - r))


def sk2p_hash(hi, lo) -> np.ndarray:
    """mk_skmer2.hip sk2p_hash: the 128 key bits folded to 64 (hi ^ rotr(lo, 23)), then skc_hash's multiplies."""
    h = _three(_u(hi) ^ rotr64(lo, 23))
    return h ^ (h >> U64(15))


def part_hash_fields(key, p1_log2: int):
    """mk_part.hip: (bucket, 24-bit split field, home slot) of a one-word key."""
    h = mix64(key)
    return h >> U64(64 - p1_log2), (h >> U64(64 - p1_log2 - 24)) & U64(M24), h & U64(CNT_SLOTS - 1)


def _deposit(i: np.ndarray, positions: Sequence[int]) -> np.ndarray:
    """The bits of i (t = 0, 1, ..) placed at positions[t] of a 64-bit word."""
    out = np.zeros(i.size, dtype=U64)
    for t, p in enumerate(positions):
        out |= ((i >> U64(t)) & U64(1)) << U64(p)
    return out


def _free_positions(fixed_mask: int, skip: int) -> List[int]:
    return [b for b in range(64) if not (fixed_mask >> b) & 1 and not (skip >> b) & 1]


def skc_hostile(k: int, n: int, offset: int = 0, same_home: bool = True, seed: int = 1) -> np.ndarray:
    """Up to n distinct one-word k-mer keys (12 <= k <= 32) with M_STAR at bases offset..offset+10 -- one minimizer, so
    one bucket at any p1 -- and equal skc_hash bits 15..0 (the sub-range at every split level); with same_home also
    equal bits 31..19 (the home slot).  Bits 24..39 of the key (bases k-20..k-13) must be free: they are solved for."""
    assert 12 <= k <= 32 and 0 <= offset <= k - SK_M
    mshift = 2 * (k - SK_M - offset)
    fixed = ((1 << 22) - 1) << mshift
    base = M_STAR << mshift
    solve = 0xFFFF << 24
    assert not fixed & solve, "M_STAR would cover the solved bits"
    keymask = (1 << (2 * k)) - 1
    free = [b for b in _free_positions(fixed | ~keymask & ((1 << 64) - 1), solve)]
    rng = np.random.default_rng(seed)
    target = int(rng.integers(0, 1 << 32))
    binv = pow(0x85EBCB, -1, 1 << 16)
    got, total = [], 0
    step = 1 << 22
    for start in range(0, 1 << len(free), step):
        i = np.arange(start, min(start + step, 1 << len(free)), dtype=U64)
        key = _deposit(i, free) | U64(base)
        with np.errstate(over="ignore"):
            x = (((skc_hash(key) ^ U64(target)) & U64(0xFFFF)) * U64(binv)) & U64(0xFFFF)
        key = key | (x << U64(24))
        h = skc_hash(key)
        ok = (h & U64(0xFFFF)) == U64(target & 0xFFFF)
        if same_home:
            ok &= (h >> U64(19)) == U64(target >> 19)
        got.append(key[ok])
        total += int(ok.sum())
        if total >= n:
            break
    keys = np.unique(np.concatenate(got))
    return keys[:n]


def sk2c_hostile(k: int, n: int, seed: int = 2) -> Tuple[np.ndarray, np.ndarray]:
    """Up to n distinct two-word keys (33 <= k <= 64) with M_STAR at bases 0..10 and one value of sk2c_hash: one
    bucket, one home slot, one sub-range at every split level.  Bits 0..23 of hi are enumerated, bits 24..41 solved,
    the rest of the key (lo) drawn once."""
    assert 33 <= k <= 64
    rng = np.random.default_rng(seed)
    lo_bits = 2 * (k - 32)
    lo = U64((int.from_bytes(rng.bytes(8), "little") >> (64 - lo_bits)) << (64 - lo_bits))
    hi_base = U64(M_STAR << 42)
    target = int(rng.integers(0, 1 << 32))
    binv = pow(0x85EBCB, -1, 1 << 18)
    got, total = [], 0
    step = 1 << 22
    for start in range(0, 1 << 24, step):
        h0 = np.arange(start, start + step, dtype=U64)
        hi = hi_base | h0
        # pre-mix value without the middle piece's product: the product must make up the rest
        rest = _sk2_pre(hi, np.full(hi.size, lo)) ^ umul24((hi >> U64(24)) & U64(M32), 0x85EBCB)
        with np.errstate(over="ignore"):
            need = rest ^ U64(target)
            # middle piece = hi bits 24..47: bits 42..47 are M_STAR's, bits 24..41 (x) are solved from the low 18 bits
            top = (hi >> U64(24)) & U64(0xFC0000)
            x = (((need - umul24(top, 0x85EBCB)) & U64((1 << 18) - 1)) * U64(binv)) & U64((1 << 18) - 1)
        hi = hi | (x << U64(24))
        ok = _sk2_pre(hi, np.full(hi.size, lo)) == U64(target)
        got.append(hi[ok])
        total += int(ok.sum())
        if total >= n:
            break
    his = np.unique(np.concatenate(got))[:n]
    return his, np.full(his.size, lo)


def sk2p_hostile(k: int, n: int, seed: int = 3) -> Tuple[np.ndarray, np.ndarray]:
    """n distinct two-word keys (33 <= k <= 64) with one value of sk2p_hash and M_STAR at bases 0..10:
    (hi ^ rotr(d, 23), lo ^ d) for d on lo bits that the key uses and that rotr moves below hi bit 42."""
    assert 33 <= k <= 64
    rng = np.random.default_rng(seed)
    lo_low = max(23, 128 - 2 * k)  # (d below bit 23 would rotate into M_STAR's bits of hi)
    width = 64 - lo_low
    assert (1 << width) >= n
    hi0 = U64((M_STAR << 42) | int(rng.integers(0, 1 << 42)))
    lo0 = U64((int.from_bytes(rng.bytes(8), "little") >> (128 - 2 * k)) << (128 - 2 * k))
    d = rng.choice(1 << min(width, 40), size=n, replace=False).astype(U64) << U64(lo_low)
    return np.full(n, hi0) ^ rotr64(d, 23), np.full(n, lo0) ^ d


def part_hostile(k: int, n: int, fixed_top: int = 37, same_home: bool = True, seed: int = 4) -> np.ndarray:
    """Up to n distinct protein keys (5-bit codes A..Z, 6 <= k <= 12) whose mk_mix64 shares its top fixed_top bits
    (the bucket and split field at p1_log2 <= fixed_top - 24) and, with same_home, its low 13 bits (the LDS home slot
    of mk_part_count_k): keys are unmix64 of the values with the other bits free, kept when they are valid k-mers."""
    assert 6 <= k <= 12
    rng = np.random.default_rng(seed)
    top = int(rng.integers(0, 1 << fixed_top)) << (64 - fixed_top)
    low = int(rng.integers(0, CNT_SLOTS)) if same_home else 0
    free = list(range(13 if same_home else 0, 64 - fixed_top))
    got, total = [], 0
    step = 1 << 22
    for start in range(0, 1 << len(free), step):
        i = np.arange(start, min(start + step, 1 << len(free)), dtype=U64)
        key = unmix64(_deposit(i, free) | U64(top | low))
        ok = key < U64(1 << (5 * k))
        for j in range(k):
            ok &= ((key >> U64(5 * j)) & U64(31)) <= U64(25)
        got.append(key[ok])
        total += int(ok.sum())
        if total >= n:
            break
    return np.unique(np.concatenate(got))[:n]


def hostile_fasta(rows: np.ndarray, reps: Sequence[int], background: bytes = b"", tag: str = "h") -> bytes:
    """One record per occurrence: key i ((rows, k) uint8 text) written reps[i] times, each as a record of its own, the
    background records (FASTA text) between them."""
    recs = []
    for i, r in enumerate(reps):
        line = b">%s%d\n%s\n" % (tag.encode(), i, rows[i].tobytes())
        recs.append(line * int(r))
    half = len(recs) // 2
    return b"".join(recs[:half]) + background + b"".join(recs[half:])
