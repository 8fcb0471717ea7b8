"""Texts and keys that put the rows kept as text -- every window the engine cannot pack -- on the seams of the code that
carries them: the by-reference count kernel, the text table and its arena, the row sort and gather, the host merge of
packed and text rows.  A helper module (like text_edges.py): nothing here touches the library or a GPU.

    unit                                        size    where
    window starts a thread (RB)                 32      mk_count_byref_k: p0 = thread * RB
    threads a workgroup                         256     its launch (8192 window starts a workgroup)
    positions a bitmap word                     64      the EXOTIC skip over the bad-symbol bitmap
    bits of a position in a slot (REF_POS_BITS) 40      tag << 40 | position; the row index of mk_rows_by_slot_k
    bytes a sort word                           8       mk_row_word_k / mk_sort_rows: ceil(k / 8) big-endian words
    bytes a gather step                         64      mk_rows_gather_k: a wave copies a row 64 bytes at a time

The plain rule is the seq[i:i+k] dictionary of oracle.cpu_ref, filtered per chunk and summed; from the same records this
module counts the windows a context cannot pack (by_reference_windows).  tests/test_text_rows_host.py pins the table to
the sources and proves that every builder places what it claims; tests/test_gpu_text_rows.py counts on the GPU."""
import functools
import re

import numpy as np

import text_edges as te
from oracle import c_oracle, cpu_ref

RB = 32
WORKGROUP = 256
BITMAP_WORD = 64
REF_POS_BITS = 40
SORT_WORD = 8
GATHER_STEP = 64


def source_units() -> dict:
    """What the sources say about the table above."""
    count = (te.CSRC / "mk_count.hip").read_text()
    sort = (te.CSRC / "mk_sort.hip").read_text()
    out = {}
    for name in ("RB", "REF_POS_BITS"):
        found = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)u?\s" % name, count, flags=re.M)
        assert len(found) == 1, (name, found)
        out[name] = int(found[0])
    kernel = count[count.index("void mk_count_byref_k"):count.index("// ----------------------------------------------------------------- packed by-reference")]
    out["byref_launch_bounds"] = int(re.search(r"__launch_bounds__\((\d+)\)\s+void mk_count_byref_k", count).group(1))
    out["byref_block"] = sorted({int(x) for pair in re.findall(
        r"mk_count_byref_k<(?:true|false)>\), dim3\(\(unsigned\)div_up\(threads, (\d+)\)\), dim3\((\d+)\)", count) for x in pair})
    out["bitmap_shift"] = sorted(set(re.findall(r"(?:>>|<<) (\d+)", kernel[kernel.index("if (EXOTIC && work)"):kernel.index("work = any")])))
    row_word = sort[sort.index("void mk_row_word_k"):sort.index("int mk_sort_rows")]
    out["sort_word"] = sorted(set(int(x) for x in re.findall(r"\b(\d+) \* (?:\(size_t\))?word", row_word)))
    out["sort_words"] = "(k + 7) / 8" in sort
    gather = sort[sort.index("void mk_rows_gather_k"):sort.index("int mk_launch_rows_by_slot")]
    out["gather_step"] = [int(x) for x in re.findall(r"b \+= (\d+)", gather)]
    out["row_index_bits"] = [int(x) for x in re.findall(r"\(1ull << (\d+)\) - 1", sort[sort.index("void mk_rows_by_slot_k"):sort.index("void mk_rows_gather_k")])]
    return out


# ----------------------------------------------------------------------------- contexts and their alphabets
NT2, AA5, RAW = "nt2", "aa5", "raw"
K_SETS = {NT2: (1, 7, 8, 21, 31, 32, 33, 63, 64, 65, 90, 200),
          RAW: (1, 5, 31, 32, 33, 100),
          AA5: (3, 5, 8, 13, 25, 26, 40)}
CASES = [(a, k) for a in (NT2, RAW, AA5) for k in K_SETS[a]]
CASE_IDS = ["%s-%d" % c for c in CASES]
LETTERS = {NT2: b"ACGT", AA5: bytes(range(ord("A"), ord("Z") + 1)), RAW: b""}
FILL = {NT2: b"ACGT", RAW: b"ACGT", AA5: b"ACDEFGHIKLMPQRSTVWY"}   # what "random in-alphabet symbols" draws from (no N)
EXOTIC = {NT2: b"N", RAW: b"N", AA5: b"x"}                          # the exotic byte where one will do
EXOTICS = {NT2: b"N", RAW: b"N", AA5: b"x-1"}                       # where several are placed: taken in turn
MAX_PACKED_K = {NT2: 64, AA5: 25, RAW: 0}


def packs(alphabet: str, k: int) -> bool:
    """Does a context of this shape pack any window?  (Otherwise every window goes by reference: RAW, NT2 k > 64,
    AA5 k > 25 -- mk_create's mode.)"""
    return k <= MAX_PACKED_K[alphabet]


def letters_of(alphabet: str, k: int) -> bytes:
    """The characters a context of this shape packs: its alphabet, or none where it packs nothing."""
    return LETTERS[alphabet] if packs(alphabet, k) else b""


def fill(alphabet: str, n: int, seed: int) -> bytes:
    src = np.frombuffer(FILL[alphabet], dtype=np.uint8)
    return src[np.random.default_rng(seed).integers(0, src.size, n)].tobytes()


# ----------------------------------------------------------------------------- the plain rule
def records_of(text: bytes) -> list:
    """The parsed stream restated plainly: the records joined by one separator (text in front of the first header line
    is a record of its own), cut at the separators again."""
    stream, _ = te.parse_stream(text)
    return stream.split(bytes([te.SEP]))


def stream_of(text: bytes) -> bytes:
    return te.parse_stream(text)[0]


def window_counts(text: bytes, k: int, letters: bytes) -> tuple:
    """(all windows, windows that hold at least one character outside `letters`) of one chunk."""
    allowed = np.frombuffer(letters, dtype=np.uint8)
    windows = odd = 0
    for rec in records_of(text):
        n = len(rec) - k + 1
        if n <= 0:
            continue
        bad = ~np.isin(np.frombuffer(rec, dtype=np.uint8), allowed)
        run = np.concatenate(([0], np.cumsum(bad)))
        windows += n
        odd += int(np.count_nonzero(run[k:] - run[:-k]))
    return windows, odd


def by_reference_windows(chunks, k: int, alphabet: str) -> tuple:
    """(stats()["windows"], stats()["exotic_windows"]) after these chunks."""
    got = [window_counts(t, k, letters_of(alphabet, k)) for t in chunks]
    return sum(g[0] for g in got), sum(g[1] for g in got)


def table_of(chunks, k: int, c: int, big: bool = False) -> dict:
    """The expected table: every chunk's dictionary with its own filter, summed."""
    one = c_oracle.count_dict if big else cpu_ref.count_text
    return cpu_ref.merge_counts(one(t, k, c) for t in chunks)


def is_text_key(key: str, letters: bytes) -> bool:
    ok = set(letters.decode())
    return any(ch not in ok for ch in key)


def text_rows_of(table: dict, k: int, alphabet: str) -> dict:
    letters = letters_of(alphabet, k)
    return {key: n for key, n in table.items() if is_text_key(key, letters)}


def as_arrays(table: dict, k: int):
    """(rows, k) uint8 and counts uint64 in Python's sorted() order: what export() must return."""
    keys = sorted(table)
    kmers = np.frombuffer("".join(keys).encode("ascii"), dtype=np.uint8).reshape(len(keys), k) if keys else np.zeros((0, k), np.uint8)
    return kmers, np.array([table[key] for key in keys], dtype=np.uint64)


def clean_text(text: bytes) -> bool:
    """No blanks (every byte is a line end or 0x21..0x7E), no '*', no empty line, and no '>' but as the first byte of a line."""
    lines = text.split(b"\n")
    return all(0x21 <= b <= 0x7E for line in lines for b in line) and b"*" not in text and b"\n\n" not in text and \
        text[:1] != b"\n" and all(b">" not in line[1:] for line in lines)


# ----------------------------------------------------------------------------- packed keys, decoded
def decode_two_words(hi: int, lo: int, k: int, alphabet: str) -> str:
    """A two-word packed key as its text (mk_decode_row restated): nucleotides left-aligned, two bits a base, base 32 the
    top of lo; amino acids the number sum(code * 32^(k-1-j)) with code = letter - 'A'."""
    if alphabet == AA5:
        x = (hi << 64) | lo
        return "".join(chr(65 + ((x >> (5 * (k - 1 - j))) & 31)) for j in range(k))
    x = (hi << 64) | lo
    return "".join("ACGT"[(x >> (126 - 2 * j)) & 3] for j in range(k))


def encode_two_words(key: str, alphabet: str) -> tuple:
    k = len(key)
    if alphabet == AA5:
        x = sum((ord(ch) - 65) << (5 * (k - 1 - j)) for j, ch in enumerate(key))
    else:
        x = sum("ACGT".index(ch) << (126 - 2 * j) for j, ch in enumerate(key))
    return x >> 64, x & ((1 << 64) - 1)


# ----------------------------------------------------------------------------- 1: one exotic byte at every bitmap residue
SINGLE_STEP = 193     # = 1 mod 64 (and mod 32): 64 bytes that far apart take every residue, whatever the first one's
SINGLE_COUNT = 64
SINGLE_FIRST = 100


def single_positions() -> list:
    """Offsets inside the record of single_exotic_text's exotic bytes."""
    return [SINGLE_FIRST + SINGLE_STEP * i for i in range(SINGLE_COUNT)]


def single_exotic_text(alphabet: str, k: int, twice: bool = False) -> bytes:
    """One long record (one line) of random in-alphabet symbols with a single exotic byte ('N'; AA5: 'x', '-', '1' in turn)
    every 193 symbols, 64 of them; k + 40 symbols behind the last.  twice: the record two times in one text."""
    at = single_positions()
    seq = bytearray(fill(alphabet, at[-1] + k + 40, 300 + k))
    for i, p in enumerate(at):
        seq[p] = EXOTICS[alphabet][i % len(EXOTICS[alphabet])]
    rec = b">one_exotic_byte_every_193\n" + bytes(seq) + b"\n"
    return rec + rec if twice else rec


# ----------------------------------------------------------------------------- 2: runs of one character
PLACES = ("start", "end", "whole", "mid", "against")
LONG_RUN = 4000
RUN_VARIANTS = ("plain", "wrapped", "cut")


def run_lengths(k: int, long: bool = None) -> tuple:
    """The run lengths of a context; long = True: the longest alone, False: the others."""
    short = tuple(sorted({n for n in (k - 1, k, k + 1, k + 2, 2 * k, 31, 32, 33, 63, 64, 65, 96) if n > 0}))
    return short + (LONG_RUN,) if long is None else ((LONG_RUN,) if long else short)


def run_parts(variant: str) -> tuple:
    """The texts of one character and variant: (place, long) -- one text a place for the runs up to 96 and 2k, one a
    place for the run of 4000, so that every text stays a few hundred KB."""
    return tuple((place, long) for place in (PLACES if variant != "cut" else ("whole", "mid")) for long in (False, True))


def run_chars(alphabet: str) -> bytes:
    """N and n everywhere; A in RAW contexts, where it is as exotic as any."""
    return b"NnA" if alphabet == RAW else b"Nn"


def _other(ch: int) -> int:
    return {ord("N"): ord("n"), ord("n"): ord("N"), ord("A"): ord("N")}[ch]


class RunText:
    """A text built record by record, with the offset of everything placed in the parsed stream."""

    def __init__(self, alphabet, seed):
        self.alphabet, self.seed = alphabet, seed
        self.parts, self.at, self.placed, self.nrec = [], 0, [], 0

    def spacer_for(self, residue, lead=0):
        """How many fill symbols put a run `lead` symbols further on at this stream residue mod 32."""
        return (residue - (self.at + 1 + lead)) % RB

    def record(self, pieces, wrap=0, cut=None):
        """pieces: (bytes, label or None); a label records (label, stream offset, length).  wrap: line length (0: one line).
        cut: (piece index, offset): a header line there, so a separator lies inside that piece."""
        self.parts.append(b">r%d\n" % self.nrec)
        self.nrec += 1
        self.at += 1
        seq = b""
        for i, (data, label) in enumerate(pieces):
            if cut and cut[0] == i:
                head, tail = data[:cut[1]], data[cut[1]:]
                if label:
                    self.placed.append((label, self.at + len(seq), len(head)))
                seq += head
                self._lines(seq, wrap)
                self.at += len(seq) + 1
                self.parts.append(b">r%d_cut\n" % self.nrec)
                self.nrec += 1
                seq = b""
                if label:
                    self.placed.append((label, self.at, len(tail)))
                seq += tail
                continue
            if label:
                self.placed.append((label, self.at + len(seq), len(data)))
            seq += data
        self._lines(seq, wrap)
        self.at += len(seq)

    def _lines(self, seq, wrap):
        if not seq:
            return
        if not wrap:
            self.parts.append(seq + b"\n")
        else:
            self.parts.extend(seq[j:j + wrap] + b"\n" for j in range(0, len(seq), wrap))

    def text(self):
        return b"".join(self.parts)


@functools.lru_cache(maxsize=4)
def run_text(alphabet: str, k: int, ch: int, variant: str, place: str, long: bool):
    """(text, placed runs) for runs of the byte ch at one place of PLACES: the first thing of a record, the last, the
    whole record, between random symbols, or directly in front of an equally long run of another exotic character.
    Every length of run_lengths(k, long) starts at every stream residue mod 32.  A spacer of 0..31 random symbols in
    front of the run (or, where the run leads its record, at the end of the record before) sets the residue.
    variant "wrapped": the same records over lines of 60.  variant "cut" ("mid" and "whole"): a header line inside the
    run, at a third of its length."""
    wrap = 60 if variant == "wrapped" else 0
    t = RunText(alphabet, k)
    flank = k + 3
    seed = [1000 * k + ch + 100_000 * PLACES.index(place) + 1_000_000 * long]

    def rnd(n):
        seed[0] += 1
        return fill(alphabet, n, seed[0])

    assert (place, long) in run_parts(variant)
    for length in run_lengths(k, long):
        run = bytes([ch]) * length
        for r in range(RB):
            label = (place, length, r)
            cut = None
            if place in ("start", "whole"):
                # the residue of a record's first symbol is set by the record before: pad that one
                pad = (r - (t.at + 3)) % RB  # (that record's separator, pad + 1 symbols, this record's separator)
                t.record([(rnd(pad + 1), None)], wrap)
                pieces = [(run, label)] + ([(rnd(flank), None)] if place == "start" else [])
                if variant == "cut" and length > 1:
                    cut = (0, max(1, length // 3))
            elif place == "end":
                pieces = [(rnd(flank + t.spacer_for(r, lead=flank)), None), (run, label)]
            elif place == "mid":
                pieces = [(rnd(flank + t.spacer_for(r, lead=flank)), None), (run, label), (rnd(flank), None)]
                if variant == "cut" and length > 1:
                    cut = (1, max(1, length // 3))
            else:
                pieces = [(rnd(flank + t.spacer_for(r, lead=flank)), None), (run, label),
                          (bytes([_other(ch)]) * length, ("other", length, r)), (rnd(flank), None)]
            t.record(pieces, wrap, cut)
    return t.text(), tuple(t.placed)


# ----------------------------------------------------------------------------- 3: the end of the stream
END_LENGTHS = ("k-1", "k", "k+1", "k+31")


def end_length(name: str, k: int) -> int:
    return {"k-1": k - 1, "k": k, "k+1": k + 1, "k+31": k + 31}[name]


def end_text(alphabet: str, k: int, name: str, residue: int, newline: bool) -> bytes:
    """A filler record, then a last record of k - 1, k, k + 1 or k + 31 symbols whose last byte is exotic (k = 1: of its header line alone); the filler's
    length makes the whole parsed stream `residue` symbols long mod 32.  newline: the text ends in a line end."""
    n = end_length(name, k)
    base = k + 40
    filler = base + (residue - (2 + n + base)) % RB
    odd = EXOTICS[alphabet]
    last = fill(alphabet, n, 7 * k + n)[:max(n - 1, 0)] + (odd[residue % len(odd):][:1] if n else b"")
    text = b">filler\n" + fill(alphabet, filler, 11 * k + residue) + b"\n>last" + (b"\n" + last if n else b"")
    return text + b"\n" if newline else text


def short_only_text(alphabet: str, k: int) -> bytes:
    """One record of k - 1 symbols, the last exotic: no window at all."""
    return b">short\n" + (fill(alphabet, k - 2, k) + EXOTIC[alphabet] + b"\n" if k > 1 else b"")


# ----------------------------------------------------------------------------- 4: survivors and their tables
SURVIVOR_SHAPES = ((NT2, 33), (NT2, 40), (NT2, 64), (AA5, 13), (AA5, 25))


def survivor_text(alphabet: str, k: int, c: int) -> bytes:
    """Records of k + 4 symbols that differ in ONE place only: 'ACGT' in the middle (all four windows are packed,
    two-word keys), 'ACG' + the exotic byte, and 'acgt'.  c = 1: each once.  c = 2: eight base records, every pattern of
    once / twice over the three variants."""
    out, patterns = [], [(1, 1, 1)] if c == 1 else [(a, b, d) for a in (1, 2) for b in (1, 2) for d in (1, 2)]
    for i, times in enumerate(patterns):
        base = bytearray(fill(alphabet, k + 4, 50 * k + i))
        mid = (k + 4) // 2 - 2
        for variant, n in zip((b"ACGT", b"ACG" + EXOTIC[alphabet], b"acgt"), times):
            base[mid:mid + 4] = variant
            out.extend([b">s%d_%d\n" % (i, variant[3]) + bytes(base) + b"\n"] * n)
    return b"".join(out)


# ----------------------------------------------------------------------------- 5: the text table grows
GROW_SHAPES = ((NT2, 21), (NT2, 40), (RAW, 9), (NT2, 90))
GROW_CHUNKS = 8
GROW_FIRST = 500


def _unit(k: int, seed_bytes: np.ndarray, i: int) -> bytes:
    """k - 1 random bases, one N, k - 1 random bases: k windows, every one over the N."""
    a = seed_bytes[i * 2 * (k - 1):(i * 2 + 1) * (k - 1)].tobytes()
    b = seed_bytes[(i * 2 + 1) * (k - 1):(i * 2 + 2) * (k - 1)].tobytes()
    return a + b"N" + b


@functools.lru_cache(maxsize=2)
def grow_chunks(alphabet: str, k: int, c: int) -> tuple:
    """Eight chunks; chunk j brings about 500 * 2^j exotic windows that no chunk before it holds (units of k of them:
    random bases around one N, each unit a record) and repeats every unit of the chunks before.
    c = 1: everything once.  c = 2: a chunk holds its new units twice (kept); of the old ones those with an even number
    twice (kept, added) and the others once (dropped by this chunk's filter); and a few units of its own once, which the
    next chunk holds once again: two occurrences in the sample, none kept."""
    per = [max(1, GROW_FIRST * (1 << j) // k) for j in range(GROW_CHUNKS)]
    total = sum(per) + GROW_CHUNKS * 10
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(900 + k).integers(0, 4, (total + 1) * 2 * (k - 1) + 8)]
    units = [b">u%d\n" % i + _unit(k, bases, i) + b"\n" for i in range(total)]
    singles = [units[sum(per) + 10 * j:sum(per) + 10 * (j + 1)] for j in range(GROW_CHUNKS)]
    plain = b">plain\n" + te.bases(200, 77) + b"\n"
    chunks, first = [], 0
    for j in range(GROW_CHUNKS):
        old, new = units[:first], units[first:first + per[j]]
        if c == 1:
            parts = old + new
        else:
            parts = [u for i, u in enumerate(old) for _ in range(2 - i % 2)] + new + new + singles[j] + (singles[j - 1] if j else [])
        chunks.append(plain + b"".join(parts))
        first += per[j]
    return tuple(chunks)


def growth_model(new_rows_per_chunk) -> tuple:
    """(arena re-reservations that keep content, table rebuilds) of mk_grow_run_ref fed with these survivors per chunk:
    the arena takes max(need, twice its rows), the table pow2(4 * need) slots once 2 * need exceeds them."""
    cap = slots = rows = kept = rebuilt = 0
    for survivors, new in new_rows_per_chunk:
        need = rows + survivors
        if need > cap:
            kept += 1 if rows else 0
            cap = max(need, 2 * cap)
        if 2 * need > slots:
            rebuilt += 1 if rows else 0
            slots = 1 << max(0, (4 * need - 1).bit_length())
        rows += new
    return kept, rebuilt


# ----------------------------------------------------------------------------- 6: the order of text rows
ORDER_KS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129)
KEY_BYTES = bytes(b for b in range(0x21, 0x7F) if b != ord("*"))
ORDER_PAIR_BYTES = (0, 7, 8, 9, 63, 64, 65)
ORDER_PAIRS = 8   # pairs a byte: rows that compare equal keep the order they were stored in, which may be the right one
ORDER_COUNTS = (7, 1234567890, 12345678901234567890)   # 1, 10 and 20 digits


def order_keys(k: int) -> tuple:
    """(keys in import order, pairs): 3000 random keys over '!'..'~' without '*', 400 over 'A' and 'B' alone (rows that
    agree in long prefixes, so that every word decides somewhere), and pairs of keys that differ in ONE byte only --
    byte 0, the last, 7, 8, 9, 63, 64, 65 where k has them, eight pairs each -- all distinct, shuffled."""
    rng = np.random.default_rng(4000 + k)
    src = np.frombuffer(KEY_BYTES, dtype=np.uint8)
    keys = {src[row].tobytes() for row in rng.integers(0, src.size, (3000, k))}
    keys |= {np.frombuffer(b"AB", dtype=np.uint8)[row].tobytes() for row in rng.integers(0, 2, (400, k))}
    pairs = []
    for at in sorted({b for b in ORDER_PAIR_BYTES + (k - 1,) if b < k}):
        for _ in range(ORDER_PAIRS):
            base = bytearray(src[rng.integers(0, src.size, k)].tobytes())
            lo, hi = bytes(base[:at]) + b"5" + bytes(base[at + 1:]), bytes(base[:at]) + b"6" + bytes(base[at + 1:])
            pairs.append((at, lo, hi))
            keys |= {lo, hi}
    keys = sorted(keys)
    order = rng.permutation(len(keys))
    return tuple(keys[i] for i in order), tuple(pairs)


def order_table(keys) -> dict:
    return {key.decode("ascii"): ORDER_COUNTS[i % 3] for i, key in enumerate(keys)}


def key_rows(keys, k: int) -> np.ndarray:
    return np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), k)


# ----------------------------------------------------------------------------- 7: text rows between packed rows
MERGE_SHAPES = ((NT2, 5), (NT2, 21), (NT2, 40), (AA5, 5))
MERGE_SEEDS = (1, 2)
MOVE_SHAPES = ((NT2, 21), (RAW, 9), (NT2, 40), (AA5, 5))   # 8: text rows moved between contexts, merge_text(.., MOVE_SEED)
MOVE_SEED = 3
MERGE_ODD = b"-09Nat~"   # below 'A': '-', digits; between 'G' and 'T': 'N'; above 'Z': lower case, '~'


def merge_text(alphabet: str, k: int, seed: int) -> bytes:
    """Records of in-alphabet symbols -- the first an 'ACGGT'-like stretch over A, C, G and T, so that packed keys start
    with every one of them -- and the same records with ONE byte replaced by each of '-', '0', '9', 'N', 'a', 't', '~' at
    the first place, in the middle and at the last: text keys in front of, between and behind the packed ones.  Every
    record is there twice or three times, and a common record (seed 0) is in every such text."""
    out = []
    for s in (0, seed):
        for i in range(6):
            rec = b"ACGGTTGCA"[:max(1, min(9, k))] * 2 + fill(alphabet, 2 * k + 5, 100 * s + 7 * k + i)
            out.append((b">m%d\n" % i + rec + b"\n") * (2 + i % 2))
            for ch in MERGE_ODD:
                for at in (0, len(rec) // 2, len(rec) - 1):
                    odd = rec[:at] + bytes([ch]) + rec[at + 1:]
                    out.append(b">m%d_%d_%d\n" % (i, ch, at) + odd + b"\n")
    return b"".join(out)
