"""FASTA texts that take the ORF calls (mercat2_amd/csrc/mk_orf.hip) past the sizes at which their kernels change
path, with what tests/orf_rule_np.py gives for them.  A helper module (like record_seams.py): nothing here touches the
library or a GPU.

    path                                                   from                          text
    or_carry_k: more than one tile a thread                CARRY_THREADS + 1 tiles       dense(T), far(T, .)
    a carry that crosses hundreds of tiles                 --                            far(T, .)
    or_name_k / or_len_k: a lane takes a second item       LANES + 1 records / ORFs      many()
    or_gather_k: a workgroup inside one ORF                2 x GATHER_BYTES residues     far(T, .)

The stream of a piece holds its kept characters and one separator a header line; it has ceil((seq_len + 1) / SPAN)
tiles, the position behind its last byte included.  A headed first record begins at stream position 1.  Every figure
above is read from the source.  tests/test_orf_scale_host.py checks that every text is what is claimed here;
tests/test_gpu_orf_scale.py runs them."""
import functools
import re
from pathlib import Path

import numpy as np

import orf_rule_np

CSRC = Path(__file__).resolve().parent.parent / "mercat2_amd" / "csrc"


@functools.lru_cache(maxsize=None)
def source_figures() -> dict:
    """The sizes the thresholds follow from."""
    src = (CSRC / "mk_orf.hip").read_text()
    pieces = (CSRC / "mk_tsvpieces.h").read_text()
    run = int(re.search(r"^#define OR_RUN (\d+)\b", src, re.M).group(1))
    assert re.search(r"^#define OR_SPAN \(256 \* OR_RUN\)", src, re.M)
    carry = int(re.search(r"\(or_carry_k<START>\), dim3\(1\), dim3\((\d+)\)", src).group(1))
    per = re.search(r"const size_t per = \(ntiles \+ (\d+)\) / (\d+);", src)
    assert (int(per.group(1)), int(per.group(2))) == (carry - 1, carry)  # a thread owns ceil(ntiles / carry) tiles
    name = re.search(r"or_name_k, dim3\(grid_for\(nrows, (\d+), (\d+)\)\), dim3\((\d+)\)", src)
    length = re.search(r"or_len_k, dim3\(grid_for\(norfs \+ 1, (\d+), (\d+)\)\), dim3\((\d+)\)", src)
    assert name.group(1) == name.group(3) and length.group(1) == length.group(3) and name.groups() == length.groups()
    chunks = int(re.search(r"^#define OR_CHUNKS (\d+)\b", src, re.M).group(1))
    assert "dim3((unsigned)div_up((size_t)nbody, 256 * OR_CHUNKS)), dim3(256)" in src
    assert re.search(r"^#define TL_DEFAULT_PIECE \(\(size_t\)16 << 20\)", pieces, re.M)
    return {"RUN": run, "SPAN": 256 * run, "CARRY_THREADS": carry, "LANES": int(name.group(1)) * int(name.group(2)),
            "GATHER_BYTES": 256 * 16 * chunks, "DEFAULT_PIECE": 16 << 20}


SPAN = source_figures()["SPAN"]
CARRY_THREADS = source_figures()["CARRY_THREADS"]
LANES = source_figures()["LANES"]
GATHER_BYTES = source_figures()["GATHER_BYTES"]
DEFAULT_PIECE = source_figures()["DEFAULT_PIECE"]
# tiles: one, two, two and three a thread of or_carry_k; at CARRY_THREADS + 1 half of the threads own none
DENSE_TILES = (CARRY_THREADS, CARRY_THREADS + 1, CARRY_THREADS + 2, 2 * CARRY_THREADS + 1)
FAR_TILES = (CARRY_THREADS + 1, 2 * CARRY_THREADS + 1)
FAR_VARIANTS = ("stops", "starts", "blocked", "closed")
NEAR = 199  # the second start of residue g lies in tile NEAR + g
MODES = (dict(), dict(start=True), dict(start=True, alt_starts=True), dict(strand="plus"), dict(strand="minus"),
         dict(start=True, strand="minus"), dict(start=True, alt_starts=True, strand="plus"))  # those of test_gpu_orf.py


def tiles_of(text: bytes) -> int:
    """The tiles of the ORF scan for a text that begins with a header line, as one piece."""
    assert text.startswith(b">")
    recs = orf_rule_np.records(text)
    seq_len = sum(len(s) for _, s in recs) + len(recs)
    return -(-(seq_len + 1) // SPAN)


def per_thread(tiles: int) -> int:
    return -(-tiles // CARRY_THREADS)


def _draw(seed: int, letters: bytes, n: int) -> np.ndarray:
    return np.frombuffer(letters, dtype=np.uint8)[np.random.RandomState(seed).randint(0, len(letters), n)]


def _wrap(seq: np.ndarray, width: int) -> bytes:
    """The sequence on lines of ``width``, each with its LF."""
    full = len(seq) // width
    lines = np.full((full, width + 1), 10, dtype=np.uint8)
    lines[:, :width] = seq[:full * width].reshape(full, width)
    rest = seq[full * width:].tobytes()
    return lines.tobytes() + (rest + b"\n" if rest else b"")


# ----------------------------------------------------------------------------- dense: closings everywhere
DENSE_SHORT = 40  # bases of the record behind the long one


@functools.lru_cache(maxsize=None)
def dense(tiles: int) -> bytes:
    """One headed record of random ACGT whose stream, with a second record of DENSE_SHORT bases behind it, has exactly
    ``tiles`` tiles; the second record's separator stands in the last tile, where the record's begin and the separator
    sum of the carry change once more."""
    n = (tiles - 1) * SPAN + 100 - (DENSE_SHORT + 3)  # separator, n bases, separator, DENSE_SHORT bases, the end: + 100
    return (b">dense %d\n" % tiles + _wrap(_draw(1000 + tiles, b"ACGT", n), 80)
            + b">short\n" + _draw(2000 + tiles, b"ACGT", DENSE_SHORT).tobytes() + b"\n")


# ----------------------------------------------------------------------------- far: a carry crosses every tile
# A word with the neighbours it is planted with: none of the five-letter strings holds a second stop or start of either
# strand (the alternative ones included) in any frame, whatever G or C stands around it.
FWD_STOP, ATG, CAT = b"GTAAG", b"GATGC", b"GCATC"
REV_STOPS = (b"GTTAC", b"GCTAC", b"GTCAG")  # TTA CTA TCA


def _at(base: int, k: int, g: int) -> int:
    """The k-th slot behind record position ``base`` (30 apart), moved on to a position of residue g."""
    q = base + 30 * k
    return q + (g - q) % 3


@functools.lru_cache(maxsize=None)
def far_plan(tiles: int, variant: str) -> dict:
    """{kind: [record position of the word of residue 0, 1, 2]} of what far() plants.  Tile t of the stream begins at
    record position t * SPAN - 1."""
    assert variant in FAR_VARIANTS and tiles > NEAR + 6
    last = (tiles - 1) * SPAN
    plan = {"fwd_stop_0": [_at(300, g, g) for g in range(3)], "rev_stop_0": [_at(600, g, g) for g in range(3)]}
    if variant != "stops":
        plan["atg_first"] = [_at(SPAN + 500, g, g) for g in range(3)]
        plan["cat_first"] = [_at(SPAN + 900, g, g) for g in range(3)]
        plan["atg_last"] = [_at((NEAR + g) * SPAN + 700, g, g) for g in range(3)]
        plan["cat_last"] = [_at((NEAR + g) * SPAN + 1100, g, g) for g in range(3)]
    if variant == "blocked":  # a stop between the two starts of the forward strand, one behind the last of the reverse
        plan["fwd_stop_mid"] = [_at(100 * SPAN + 50, g, g) for g in range(3)]
        plan["rev_stop_behind"] = [_at((NEAR + 4) * SPAN + 50, g, g) for g in range(3)]
    if variant == "closed":
        plan["fwd_stop_end"] = [_at(last + 5, g, g) for g in range(3)]
        plan["rev_stop_end"] = [_at(last + 95, g, g) for g in range(3)]
    return plan


FAR_TAIL = 200  # stream positions of the last tile that the record reaches


@functools.lru_cache(maxsize=None)
def far_bases(tiles: int) -> int:
    return (tiles - 1) * SPAN + FAR_TAIL - 2  # separator, the bases, the end


@functools.lru_cache(maxsize=None)
def far(tiles: int, variant: str) -> bytes:
    """One headed record over G and C, which holds no stop and no start in any frame, with the words of far_plan planted
    by hand: in every variant a forward and a reverse stop for each residue in tile 0, so that six stretches cross every
    tile behind it."""
    seq = _draw(3000 + tiles, b"GC", far_bases(tiles)).copy()
    for kind, places in far_plan(tiles, variant).items():
        for g, q in enumerate(places):
            word = FWD_STOP if kind.startswith("fwd_stop") else REV_STOPS[g] if kind.startswith("rev_stop") else ATG if kind.startswith("atg") else CAT
            seq[q - 1:q + 4] = np.frombuffer(word, dtype=np.uint8)
    return b">far %d %s\n" % (tiles, variant.encode()) + _wrap(seq, 61)


# ----------------------------------------------------------------------------- many: more records and ORFs than lanes
MANY_POOL = ((b"", b""), (b"a", b"GC"), (b"bc", b"GCG"), (b"d.e", b"CGGCC"), (b"f", b"GCCGCG"), (b"", b"CGCGGCGC"),
             (b"gh", b"GGCCGCGCC"), (b"ijk", b"GCTAAGGCC"))
MANY_RECORDS = LANES + 24


def _pool_text(i: int) -> bytes:
    name, seq = MANY_POOL[i % len(MANY_POOL)]
    return b">" + name + b"\n" + (seq + b"\n" if seq else b"")


@functools.lru_cache(maxsize=None)
def many() -> bytes:
    """MANY_RECORDS records that cycle through MANY_POOL."""
    cycle = b"".join(_pool_text(i) for i in range(len(MANY_POOL)))
    whole, rest = divmod(MANY_RECORDS, len(MANY_POOL))
    return cycle * whole + b"".join(_pool_text(i) for i in range(rest))


# ----------------------------------------------------------------------------- expectations
def _frozen(out: bytes, rows: np.ndarray):
    rows.setflags(write=False)
    return out, rows


@functools.lru_cache(maxsize=None)
def dense_expected(tiles: int, **mode):
    """(bytes, rows as an (n, 4) uint64 array) of dense(tiles) at min_aa 1."""
    return _frozen(*orf_rule_np.expected_np(dense(tiles), 1, **mode))


@functools.lru_cache(maxsize=None)
def far_expected(tiles: int, variant: str, **mode):
    return _frozen(*orf_rule_np.expected_np(far(tiles, variant), 1, **mode))


@functools.lru_cache(maxsize=None)
def many_expected():
    """(bytes, rows) of many() at min_aa 1, stop to stop.  An output record does not hold its record's number, so the
    bytes are the pool's outputs joined in order and the rows the pool's rows with the record column filled in; the
    rule runs once a pool entry."""
    pool = len(MANY_POOL)
    outs, rows = [], []
    for i in range(pool):
        out, r = orf_rule_np.expected_np(_pool_text(i), 1)
        assert (r[:, 0] == 0).all()
        r = r.copy()
        r[:, 0] = i
        outs.append(out)
        rows.append(r)
    whole, rest = divmod(MANY_RECORDS, pool)
    cycle = np.concatenate(rows)
    full = np.tile(cycle, (whole, 1))
    full[:, 0] += np.repeat(np.arange(whole, dtype=np.uint64) * np.uint64(pool), len(cycle))
    tail = np.concatenate(rows[:rest] + [np.zeros((0, 4), dtype=np.uint64)])
    tail[:, 0] += np.uint64(whole * pool)
    return _frozen(b"".join(outs) * whole + b"".join(outs[:rest]), np.concatenate((full, tail)))


def figures(text_records: int, out: bytes, rows: np.ndarray) -> dict:
    """What mk_orf_t says of the result."""
    return {"records": text_records, "orfs": len(rows), "bytes_out": len(out), "residues": int(rows[:, 2].sum()),
            "longest": int(rows[:, 2].max()) if len(rows) else 0,
            "per_frame": [int(np.count_nonzero(rows[:, 3] == f)) for f in range(1, 7)]}
