"""A FASTA text whose record boundaries stand on the seams of the lane walk (mercat2_amd/csrc/mk_screenwalk.h), and a
plain restatement of where they stand.  A helper module (like text_edges.py): nothing here touches the library or a GPU.

The walk cuts the parsed stream -- the kept characters, and one separator where a header line starts -- into units: a
lane's run of 32 window starts, a wave's 2048, a workgroup's tile of 8192.  A lane reads k - 1 symbols past its run, a
tile stages that halo, the record a run starts in comes from a prefix over lanes, waves and tiles.  Write U for a unit
and d for the distance of a separator from a multiple of U: seam_text(k) puts a separator at m * U + d for every U and
every d in -(k + 1) .. k + 1, with records of k + 1 symbols or more on both sides, and again with a record shorter than
k - 1 in front (all d at the wave seam, a few at the tile seam): a record that ends inside the symbols that fill a key.

tests/test_walk_seams_host.py checks that the text places what is claimed here; tests/test_gpu_screen.py and
tests/test_gpu_track.py walk it on the GPU with both sinks."""
import functools
import random

UNITS = (32, 2048, 8192)  # lane run (SC_RUN), wave, tile (SC_SPAN)
TILE = UNITS[2]
LONG_TILES = 3            # the long record is longer than this many tiles: wherever it starts, it covers two whole ones
SHORT_RUN = 320           # records of k .. k + 3 symbols in a row: the lanes of a wave end in different records


def shifts(k: int):
    return range(-(k + 1), k + 2)


def tile_short_shifts(k: int):
    """The tile seams that are also made with a short record in front."""
    return (-(k + 1), -1, 0, 1, k - 1, k + 1)


def targets(k: int) -> dict:
    """{stream position of a separator: whether the record in front of it is short}, all beyond the run of short records
    in the first two tiles.  Tile t (t = 2, 3, ...) holds one tile seam, three wave seams and 28 lane seams; the shifts
    cycle through each kind."""
    ds = list(shifts(k))
    tile_jobs = [(d, False) for d in ds] + [(d, True) for d in tile_short_shifts(k)]
    wave_jobs = [(d, short) for short in (False, True) for d in ds]
    lane_jobs = [(d, False) for d in ds]
    out, nw, nl = {}, 0, 0
    for t, (d, short) in enumerate(tile_jobs, start=2):
        base = t * TILE
        out[base + d] = short
        for w in (1, 2, 3):
            dw, sw = wave_jobs[nw % len(wave_jobs)]
            out[base + w * UNITS[1] + dw] = sw
            nw += 1
        for j in range(1, 32):  # every 256 symbols, the wave seams left out
            if j % 8:
                out[base + j * 256 + lane_jobs[nl % len(lane_jobs)][0]] = False
                nl += 1
    assert nw >= len(wave_jobs) and nl >= len(lane_jobs) and len(out) == len(tile_jobs) + nw + nl
    return out


@functools.lru_cache(maxsize=None)
def seam_records(k: int, seed: int = 1):
    """[(name, sequence)] of the text, in order."""
    rng = random.Random(1000 * seed + k)
    dna = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    recs = []
    pos = 0  # the stream position of the next record's separator

    def add(n):
        nonlocal pos
        recs.append(("r%d" % len(recs), dna(n)))
        pos += 1 + n

    for i in range(SHORT_RUN):
        add(k + i % 4)
    assert pos < 2 * TILE - 4 * k
    want = targets(k)
    for i, p in enumerate(sorted(want)):
        short = i % (k - 1) if want[p] else None  # 0 .. k - 2 symbols: a header behind a header among them
        room = p - pos - 1 - (0 if short is None else short + 1)
        assert room >= k + 1, (p, pos)
        add(room)
        if short is not None:
            add(short)
        assert pos == p
    add(2 * k + 5)  # behind the last seam
    add(LONG_TILES * TILE + 123)
    recs[-1] = ("long", recs[-1][1])
    add(k + 2)
    return recs


def _wrap(seq: str, width: int) -> str:
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


@functools.lru_cache(maxsize=None)
def seam_text(k: int, seed: int = 1) -> bytes:
    """The records as FASTA, sequence lines of 70; starts with a header line, so record i's separator is the i-th."""
    return "".join(">%s\n%s" % (name, _wrap(seq, 70)) for name, seq in seam_records(k, seed)).encode()


@functools.lru_cache(maxsize=None)
def other_text(k: int, seed: int = 1) -> bytes:
    """Another text that shares half of the long record: a table of it gives hits and misses."""
    rng = random.Random(77 * seed + k)
    long_seq = dict(seam_records(k, seed))["long"]
    return (">x\n" + _wrap("".join(rng.choice("ACGT") for _ in range(5_000)), 70) + ">y\n" + _wrap(long_seq[:len(long_seq) // 2], 80)).encode()


def separators(records):
    """[(stream position, symbols of the record in front, symbols of the record behind)] for every separator of a text
    that starts with a header line, from its [(name, sequence)]: one separator a record, then its kept characters."""
    out, pos = [], 0
    for i, (_, seq) in enumerate(records):
        out.append((pos, len(records[i - 1][1]) if i else None, len(seq)))
        pos += 1 + len(seq)
    return out, pos
