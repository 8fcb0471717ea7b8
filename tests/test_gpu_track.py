"""Per-window k-mer counts of reads against the GPU tables (mk_track_text / mk_track_device, Counter.track*,
kmers.track_reads, report.write_track_*, -track).  Expected values never come from the code under test: the table is a dict
made by the CPU oracle (or crafted counts loaded with Counter.load_tsv), the records of the text come from the
reference's own line loop written out below, a track is ``[table.get(w, 0) for each window]`` in plain Python and the
median is ``sorted(v)[len(v) // 2]``.  Equality is exact everywhere.

(A RAW context with k above SC_LDS_MAX_K = 16385 walks the stream without the LDS span: a record long enough for one
window makes every lane step through 16 K symbols and the oracle hash 16 KiB strings, so that instantiation of
tk_probe_k -- the walk of mk_screenwalk.h with LDS = false -- is covered by its compile alone, as sc_probe_k's is.)"""
import ctypes
import functools
import io
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

import walk_seams
from conftest import read_input
from mercat2_amd import cli, kmers, native, report
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE, NON_ASCII, RANGE = -1, -4, -5, -7
COMP = str.maketrans("ACGT", "TGCA")
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def ref_records(text: bytes):
    """[(name, sequence)] by the reference's line loop (lib/mercat2_kmers.py:49-69): text mode, strip(), startswith('>'),
    replace('*', '').  Records with an empty sequence are kept; sequence in front of the first header is a record named
    ''."""
    recs = []
    for line in io.TextIOWrapper(io.BytesIO(text), encoding="latin-1", newline=None):
        line = line.strip()
        if line.startswith(">"):
            words = line[1:].split()
            recs.append([words[0] if words else "", ""])
        else:
            piece = line.replace("*", "")
            if not recs and piece:
                recs.append(["", ""])
            if recs:
                recs[-1][1] += piece
    return [(name, seq) for name, seq in recs]


def expected_tracks(text: bytes, table: dict, k: int, fold: bool = False):
    """One list of counts per record."""
    tracks = []
    for _, seq in ref_records(text):
        counts = []
        for i in range(len(seq) - k + 1):
            w = seq[i:i + k]
            if fold and set(w) <= set("ACGT"):
                w = min(w, w.translate(COMP)[::-1])
            counts.append(table.get(w, 0))
        tracks.append(counts)
    return tracks


def rows_of(tracks, at_least=1):
    return [[len(v), sum(1 for c in v if c >= at_least), sum(v) % (1 << 64), min(v, default=0), max(v, default=0)] for v in tracks]


def median_of(v):
    return sorted(v)[len(v) // 2] if v else 0


def check(ctx, text: bytes, table: dict, at_least: int = 1, fold=None, folded_table: bool = False, sat32: bool = False,
          tracks=None, **kw):
    """Counter.track against the oracle: counts, offsets, rows (also against Counter.screen) and median."""
    info = {}
    counts, offsets, rows, med = ctx.track(text, at_least, fold=fold, sat32=sat32, median=True, info=info, **kw)
    if tracks is None:
        tracks = expected_tracks(text, table, ctx.k, folded_table)
    clip = (lambda c: min(c, M32)) if sat32 else (lambda c: c)
    flat = [clip(c) for v in tracks for c in v]
    dtype = np.uint32 if sat32 else np.uint64
    assert counts.dtype == dtype and med.dtype == dtype and offsets.dtype == np.uint64 and rows.dtype == np.uint64
    assert offsets.tolist() == [0] + np.cumsum([len(v) for v in tracks], dtype=np.uint64).tolist()
    assert counts.tolist() == flat
    assert rows.tolist() == rows_of(tracks, at_least)
    assert rows.tolist() == ctx.screen(text, at_least, fold=fold, **kw).tolist()
    assert med.tolist() == [median_of([clip(c) for c in v]) for v in tracks]
    assert info["records"] == len(tracks) and info["bytes"] == len(text) and info["windows_out"] == len(flat) == info["windows"]
    assert info["packed_windows"] + info["text_windows"] == info["windows"]
    assert info["saturated"] == sum(1 for v in tracks for c in v if sat32 and c > M32)
    return (counts, offsets, rows, med), info


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def wrap(seq, width):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


# --------------------------------------------------------------------------------------------- record shapes
@functools.lru_cache(maxsize=None)
def shapes_text(k: int, headless: bool) -> bytes:
    """Every record shape of the issue in one text; ends in a header."""
    rng = random.Random(1000 * k)
    long_seq = dna(rng, 40_011)
    t = [dna(random.Random(k + 1), k + 2) + "\n" if headless else "  \n\t\n \x0b\n"]
    t += [">km1 a b\n" + dna(rng, k - 1) + "\n", ">k\n" + dna(rng, k) + "\n", "  >kp1\tx\n" + dna(rng, k + 1) + "\n"]
    t += [">h1\n>h2\n" + dna(rng, k + 3) + "\n", ">\n" + dna(rng, k + 1) + "\n"]
    t += [">wrapped\n" + wrap(dna(rng, 3 * k + 5), 7)]
    s = dna(rng, 2 * k + 4)
    t += [">crlf\r\n" + s[:5] + "\r\n" + s[5:] + "\r\n", ">cr\r" + dna(rng, k + 2) + "\r" + dna(rng, 3) + "\r"]
    s = dna(rng, k + 6)
    t += [">star\n" + s[:3] + "*" + s[3:] + "**\n*\n", ">blank\n  " + dna(rng, 5) + " \t" + dna(rng, k + 1) + "  \n"]
    t += [">s%d\n%s\n" % (i, dna(rng, k + i % 4)) for i in range(300)]  # many records in one lane's run, in one wave
    t += [">long\n" + wrap(long_seq, 60)]                                # lanes, waves, tiles: the halo, the tile's write range
    t += [">t%d\n%s\n" % (i, dna(rng, k + 1 + i)) for i in range(3)]
    t += [">copy of a piece of long\n" + long_seq[17_000:17_000 + 2 * k] + "\n", ">last one"]
    return "".join(t).encode()


@functools.lru_cache(maxsize=None)
def other_text(k: int) -> bytes:
    """Another text that shares half of the long record: a table of it gives hits and misses."""
    rng = random.Random(77 + k)
    long_seq = [r for r in ref_records(shapes_text(k, False)) if r[0] == "long"][0][1]
    return (">x\n" + wrap(dna(rng, 5_000), 70) + ">y\n" + wrap(long_seq[:20_000], 80)).encode()


@functools.lru_cache(maxsize=None)
def table_of(text: bytes, k: int, c: int = 1) -> dict:
    return cpu_ref.count_text(text, k, c)


@functools.lru_cache(maxsize=None)
def shapes_tracks(k: int, headless: bool, own: bool):
    text = shapes_text(k, headless)
    return expected_tracks(text, table_of(text if own else other_text(k), k), k)


@pytest.mark.parametrize("own", [True, False], ids=["own_table", "other_table"])
@pytest.mark.parametrize("headless", [False, True], ids=["blanks_first", "headless"])
@pytest.mark.parametrize("k", [5, 31])
def test_record_shapes(k, headless, own):
    text = shapes_text(k, headless)
    source = text if own else other_text(k)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(source, 1)
        (counts, offsets, rows, med), info = check(ctx, text, None, tracks=shapes_tracks(k, headless, own))
        assert info["headless"] == (1 if headless else 0) and info["pieces"] == 1
        names = [name for name, _ in ref_records(text)]
        at = names.index("km1")
        assert np.diff(offsets)[at:at + 5].tolist() == [0, 1, 2, 0, 4]  # k - 1, k, k + 1; a header behind a header
        assert int(np.diff(offsets)[names.index("long")]) == 40_011 - k + 1 > 4 * 8192  # (several workgroup tiles)
        assert names[-1] == "last" and offsets[-1] == offsets[-2] == len(counts)
        if own:
            assert counts.min() >= 1
        elif k == 31:  # (nearly every 5-mer is in any table) runs of hits and runs of misses
            changes = np.count_nonzero(np.diff((counts > 0).astype(np.int8)))
            assert 0 < np.count_nonzero(counts) < len(counts) and changes > 2
        check(ctx, text, None, at_least=2, tracks=shapes_tracks(k, headless, own))


def test_pieces():
    k = 31
    text = shapes_text(k, True)
    tracks = shapes_tracks(k, True, False)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        whole, info = check(ctx, text, None, tracks=tracks)
        # (the long record is two thirds of the text and is never split: its piece is as long as it is)
        five, info5 = check(ctx, text, None, tracks=tracks, piece_bytes=len(text) // 12)
        small, info_s = check(ctx, text, None, tracks=tracks, piece_bytes=1024)  # far below the long record
        assert info["pieces"] == 1 and 4 <= info5["pieces"] <= 6 and info_s["pieces"] > 8
        for a, b, c in zip(whole, five, small):
            assert a.tolist() == b.tolist() == c.tolist()
        assert info5["headless"] == info_s["headless"] == 1
        sat, info32 = check(ctx, text, None, tracks=tracks, sat32=True, piece_bytes=len(text) // 12)
        assert info32["pieces"] == info5["pieces"] and sat[1].tolist() == whole[1].tolist()


# --------------------------------------------------------------------------------------- the walk's own seams
@functools.lru_cache(maxsize=None)
def seam_tracks(k: int):
    return expected_tracks(walk_seams.seam_text(k), table_of(walk_seams.other_text(k), k), k)


@pytest.mark.parametrize("sat32", [False, True], ids=["u64", "sat32"])
@pytest.mark.parametrize("k", [5, 31])
def test_walk_seams(k, sat32):
    """Record boundaries on every lane, wave and tile seam of the walk (tests/walk_seams.py), in one piece and in many:
    counts, offsets, rows and medians."""
    text, tracks = walk_seams.seam_text(k), seam_tracks(k)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(walk_seams.other_text(k), 1)
        one, info = check(ctx, text, None, sat32=sat32, tracks=tracks)
        many, info_p = check(ctx, text, None, sat32=sat32, tracks=tracks, piece_bytes=len(text) // 12)
        assert info["pieces"] == 1 and info_p["pieces"] > 8
        assert one[0].min() < one[0].max() and info["packed_windows"] == info["windows"]
        if k == 31:  # (nearly every 5-mer is in any table) hits and misses
            assert 0 < np.count_nonzero(one[0]) < len(one[0])
        assert max(len(v) for v in tracks) > 3 * walk_seams.TILE - k


# ------------------------------------------------------------------------------------------------- key kinds
def nt_text(seed: int) -> bytes:
    reads = native.synth_reads(300, seed, 120, 150, seed + 1).tobytes()
    return reads + (b">side\nACG" + b"T" * 75 + b"GCA\n>odd\n" + b"ACGTTGCANGGATCCATGNAacgtACGGT*CAGT" * 12 +
                    b"\n>lower\nacgtacgtacgtnnnnACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGATCGATCGACTAGCTAGCTAGCATGCATGCCCATAGAGACCAGATTTAGAG\n")


def aa_text(seed: int) -> bytes:
    rng = random.Random(seed)
    letters = "ACDEFGHIKLMNPQRSTVWY"
    recs = [">p%d\n%s\n" % (i, wrap("".join(rng.choice(letters) for _ in range(rng.randrange(20, 400))), 60)) for i in range(40)]
    recs.append(">odd\nMKV-LLAX*BZJUOacdeMKVLLAGGHHWWYYPPQQRRSSTTVVMKVLLAAGGHHWWYY.PPQQRRSSTTVVKKLL\n")
    return "".join(recs).encode()


KINDS = [("nt", NT, k) for k in (12, 32, 33, 63)] + [("aa", AA, k) for k in (5, 13)] + [("raw", RAW, 9)]


@pytest.mark.parametrize("kind,alphabet,k", KINDS, ids=["%s_k%d" % (s[0], s[2]) for s in KINDS])
def test_key_kinds(kind, alphabet, k):
    text = (aa_text if kind == "aa" else nt_text)(3)
    # the table: the first half of the text, the run of T, and a piece of the record that holds bytes outside the alphabets
    source = text[: len(text) // 2] + b"\n>side\nACG" + b"T" * 75 + b"GCA\n>x\n" + \
        (b"MKV-LLAX*BZJUOacdeMKVLLAGGHHWWYYPPQQRR" if kind == "aa" else b"ACGTTGCANGGATCCATGNAacgtACGGT*CAGT" * 3) + b"\n"
    table = table_of(source, k)
    with native.Counter(k, alphabet) as ctx:
        ctx.count_chunk(source, 1)
        (counts, offsets, _, _), info = check(ctx, text, table)
        assert 0 < np.count_nonzero(counts) < len(counts)
        if alphabet == RAW:
            assert info["packed_windows"] == 0
        else:  # N, lower-case runs, '-', '.': packed and by-reference windows alternate inside a record
            assert info["text_windows"] > 0 and info["packed_windows"] > 0
        if kind == "nt" and k == 32:  # the run of T: the key kept beside the one-word table
            side = [i for i, (name, _) in enumerate(ref_records(text)) if name == "side"][0]
            want = table["T" * 32]
            assert want >= 2 and counts[int(offsets[side]):int(offsets[side + 1])].tolist().count(want) >= 75 - 32 + 1
        check(ctx, text, table, sat32=True)


# -------------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize("k", [31, 63])
def test_fold(k):
    rng = random.Random(k)
    read = dna(rng, 150)
    source = nt_text(5) + (">r\n%s\n" % read).encode()
    text = nt_text(5)[:9_000] + ("\n>fwd\n%s\n>rev\n%s\n>n\n%sN%s\n" % (read, read.translate(COMP)[::-1], read[:70], read[70:])).encode()
    folded = cpu_ref.canonical_fold(table_of(source, k))
    with native.Counter(k, NT, canonical=True) as ctx:
        ctx.count_chunk(source, 1)
        (counts, offsets, _, med), info = check(ctx, text, folded, folded_table=True)  # fold=None: as the context counts
        names = [name for name, _ in ref_records(text)]
        fwd, rev, n = (counts[int(offsets[i]):int(offsets[i + 1])].tolist() for i in (names.index(x) for x in ("fwd", "rev", "n")))
        assert fwd == rev[::-1] and min(fwd) >= 1 and len(fwd) == 150 - k + 1
        assert len(n) == 151 - k + 1 and n.count(0) >= k - 1  # the windows over the N are not folded, and absent
        assert info["folded"] > 0
        check(ctx, text, folded, fold=False)  # taken as they stand: the windows of the other strand miss
    with native.Counter(k, NT) as plain:  # a plain table, folding asked for: refused as screen refuses it
        with pytest.raises(native.MercatHipError) as e:
            plain.track(text, fold=True)
        assert e.value.code == ARG


# ---------------------------------------------------------------------------------------------- 64 bit, SAT32
def _table_text(counts) -> bytes:
    """A count table at k = 12, nucleotide: row i is the i-th 12-mer in base-4 order with counts[i]."""
    n = len(counts)
    digits = (np.arange(n, dtype=np.int64)[:, None] >> (2 * np.arange(11, -1, -1))) & 3
    keys = np.frombuffer(b"ACGT", dtype=np.uint8)[digits].view("S12").ravel().tolist()
    return keys, b"".join(b"%s\t%d\n" % (key, c) for key, c in zip(keys, counts))


def test_64_bit_counts_and_sat32():
    big = [M32, 1 << 32, 1 << 63, M64]
    keys, table_text = _table_text(list(range(1, 201)) + big)
    table = {key.decode(): c for key, c in zip(keys, list(range(1, 201)) + big)}
    b0, b1, b2, b3 = (key.decode() for key in keys[200:])
    # "mixed": the four among ordinary windows; "huge" and "two": records whose median is one of the large values (the
    # second window of "two" is absent: [2^64 - 1, 0] sorted is [0, 2^64 - 1], element 1) -- the sort's end_bit
    text = (">mixed\n" + keys[5].decode() + b0 + keys[77].decode() + b1 + "GG" + b2 + keys[150].decode() + b3 + "\n" +
            ">huge\n" + b2 + "\n>two\n" + b3 + b3[-1] + "\n>small\n" + keys[9].decode() + keys[10].decode() + "\n").encode()
    with native.Counter(12, NT) as ctx:
        assert ctx.load_tsv(table_text)["rows"] == 204
        tracks = expected_tracks(text, table, 12)
        assert sum(1 for v in tracks for c in v if c > M32) == 3 + 1 + 1 and sum(v.count(M32) for v in tracks) == 1
        (counts, _, rows, med), info = check(ctx, text, table)
        assert med[1] == 1 << 63 and int(rows[0][4]) == M64 and info["saturated"] == 0
        (counts, _, rows, med), info = check(ctx, text, table, sat32=True)
        assert med[1] == M32 and info["saturated"] == 5 and int(rows[0][4]) == M64  # (the rows are the screen's: not clipped)
        # the four once each
        once = (">a\n" + b0 + "\n>b\n" + b1 + "\n>c\n" + b2 + "\n>d\n" + b3 + "\n").encode()
        (counts, _, _, med), info = check(ctx, once, table, sat32=True)
        assert counts.tolist() == [M32] * 4 == med.tolist() and info["saturated"] == 3
        (counts, _, _, med), info = check(ctx, once, table)
        assert counts.tolist() == big == med.tolist()


# ---------------------------------------------------------------------------------------------- median seams
def test_median_seams():
    k = 5
    rng = random.Random(9)
    base = dna(rng, 400)
    table = table_of((">t\n" + base + "\n>u\n" + "ACGTA" * 9 + "\n").encode(), k)
    recs = [base[i:i + k - 1 + w] for i, w in ((0, 0), (10, 1), (20, 2), (30, 3), (40, 4), (50, 37))]
    recs += ["ACGTA" * 5 + "ACGT", "A" * 30, base[100:300]]  # ..., absent windows only, a longer one
    text = "".join(">m%d\n%s\n" % (i, s) for i, s in enumerate(recs)).encode()
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk((">t\n" + base + "\n>u\n" + "ACGTA" * 9 + "\n").encode(), 1)
        (counts, offsets, rows, med), info = check(ctx, text, table)
        assert np.diff(offsets)[:5].tolist() == [0, 1, 2, 3, 4] and med[0] == 0 and info["s_median"] > 0
        assert len(set(counts[int(offsets[7]):int(offsets[8])].tolist())) == 1  # a record with all counts equal
        # median=False: a guarded median buffer stays as it was, nothing of the median runs
        n = len(recs)
        guard = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        got = _raw(ctx, text, len(counts), n, median=False)
        assert got["rc"] == 0 and got["st"].s_median == 0 and got["counts"][:len(counts)].tolist() == counts.tolist()
        assert (got["median"] == guard).all()
    # the 40 011-base record -- one large segment -- beside 300 tiny ones in one sort: test_record_shapes


# ------------------------------------------------------------------------------------------------ capacities
GUARD = 0xA5A5A5A5A5A5A5A5


def _raw(ctx, text: bytes, counts_cap: int, cap: int, flags: int = 0, at_least: int = 1, median: bool = True, null_counts: bool = False,
         piece_bytes: int = 0):
    """mk_track_text into 0xA5-guarded buffers one element longer than the capacities it is told."""
    counts = np.full(counts_cap + 1, GUARD, dtype=np.uint64)
    offsets = np.full(cap + 2, GUARD, dtype=np.uint64)
    med = np.full(cap + 1, GUARD, dtype=np.uint64)
    rows = np.full((cap + 1, 5), GUARD, dtype=np.uint64)
    nwin, n, st = ctypes.c_size_t(0), ctypes.c_size_t(0), native.Track()
    rc = native.lib().mk_track_text(ctx._h, text, len(text), piece_bytes, flags, at_least, None if null_counts else counts.ctypes.data,
                                    counts_cap, ctypes.byref(nwin), offsets.ctypes.data, med.ctypes.data if median else None,
                                    rows.ctypes.data, cap, ctypes.byref(n), ctypes.byref(st))
    return {"rc": rc, "nwindows": nwin.value, "nrows": n.value, "counts": counts, "offsets": offsets, "median": med, "rows": rows, "st": st}


def test_capacities():
    k, text = 31, shapes_text(31, False)
    tracks = shapes_tracks(31, False, True)
    flat = [c for v in tracks for c in v]
    nw, nr = len(flat), len(tracks)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(text, 1)
        for piece_bytes in (0, len(text) // 12):
            # exactly enough: everything written, the element past each capacity untouched
            got = _raw(ctx, text, nw, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["nwindows"], got["nrows"]) == (0, nw, nr) and got["st"].windows_out == nw
            assert got["counts"][:nw].tolist() == flat and got["counts"][nw] == GUARD
            assert got["offsets"][:nr + 1].tolist() == [0] + np.cumsum([len(v) for v in tracks]).tolist() and got["offsets"][nr + 1] == GUARD
            assert got["median"][:nr].tolist() == [median_of(v) for v in tracks] and got["median"][nr] == GUARD
            assert got["rows"][:nr].tolist() == rows_of(tracks) and (got["rows"][nr] == GUARD).all()
            # counts_cap one short: the needed size, nothing past the cap
            got = _raw(ctx, text, nw - 1, nr, piece_bytes=piece_bytes)
            assert (got["rc"], got["nwindows"], got["nrows"]) == (RANGE, nw, nr) and got["counts"][nw - 1] == GUARD
            assert "windows" in ctx._L.mk_last_error(ctx._h).decode()
            # cap one short
            got = _raw(ctx, text, nw, nr - 1, piece_bytes=piece_bytes)
            assert (got["rc"], got["nwindows"], got["nrows"]) == (RANGE, nw, nr)
            assert (got["rows"][nr - 1] == GUARD).all() and got["median"][nr - 1] == GUARD and got["offsets"][nr] == GUARD
            # the sizing call
            got = _raw(ctx, text, 0, 0, null_counts=True, piece_bytes=piece_bytes)
            assert (got["rc"], got["nwindows"], got["nrows"]) == (RANGE, nw, nr)
            assert got["offsets"][1] == GUARD and (got["rows"] == GUARD).all()
        # offsets, median and rows all NULL: cap is ignored
        counts = np.full(nw + 1, GUARD, dtype=np.uint64)
        nwin, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = native.lib().mk_track_text(ctx._h, text, len(text), 0, 0, 1, counts.ctypes.data, nw, ctypes.byref(nwin), None, None, None, 0,
                                        ctypes.byref(n), None)
        assert (rc, nwin.value, n.value) == (0, nw, nr) and counts[:nw].tolist() == flat and counts[nw] == GUARD
        # an empty text; a text of headers only
        got = _raw(ctx, b"", 0, 0)
        assert (got["rc"], got["nwindows"], got["nrows"]) == (0, 0, 0) and got["offsets"][0] == 0 and got["offsets"][1] == GUARD
        c, o, r, m = ctx.track(b"", median=True)
        assert (len(c), o.tolist(), r.shape, len(m)) == (0, [0], (0, 5), 0)
        c, o, r, m = ctx.track(b">a\n>b x\n\n>c", median=True)
        assert (len(c), o.tolist(), r.tolist(), m.tolist()) == (0, [0] * 4, [[0] * 5] * 3, [0] * 3)


# ------------------------------------------------------------------------------------------ errors and state
def test_errors_and_state():
    k, text = 31, shapes_text(31, False)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(text, 1)
        before, size, stats = ctx.to_dict(), ctx.rows(), ctx.stats()
        screen = ctx.screen(text, 2).tolist()
        check(ctx, text, None, tracks=shapes_tracks(31, False, True))
        assert ctx.rows() == size and ctx.to_dict() == before and ctx.screen(text, 2).tolist() == screen
        after = ctx.stats()
        assert all(after[f] == stats[f] for f in ("raw_bytes", "symbols", "windows", "exotic_windows", "chunks", "survivors"))
        got = _raw(ctx, text, 1 << 16, 512, flags=4)
        assert got["rc"] == ARG and "flag" in ctx._L.mk_last_error(ctx._h).decode() and got["counts"][0] == GUARD
        got = _raw(ctx, text, 1 << 16, 512, at_least=0)
        assert got["rc"] == ARG and "at_least" in ctx._L.mk_last_error(ctx._h).decode()
        with pytest.raises(native.NonAsciiInput):
            ctx.track(b">a\nACGT\xc3\xa9ACGT\n")
        assert ctx.track(b">a \xc3\xa9\nACGT\n")[2].tolist() == [[0, 0, 0, 0, 0]]
        assert ctx._L.mk_chunk_begin(ctx._h) == 0
        with pytest.raises(native.MercatHipError) as e:
            ctx.track(text)
        assert e.value.code == STATE
        assert ctx._L.mk_chunk_end(ctx._h, 1) == 0
        assert ctx.to_dict() == before


# ------------------------------------------------------------------------------------------------ device call
@pytest.mark.parametrize("sat32", [False, True], ids=["u64", "sat32"])
def test_track_device_agrees(sat32):
    import torch
    k, text = 31, shapes_text(31, True)
    lead = 3
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(other_text(k), 1)
        counts, offsets, rows, med = ctx.track(text, 2, sat32=sat32, median=True)
        assert counts.tolist() == [c for v in shapes_tracks(31, True, False) for c in v]
        nw, nr = len(counts), len(rows)
        # every buffer starts 8 bytes (sat32: counts and median 4) behind a 16-byte boundary: aligned to its elements only
        edt, one = (torch.int32, 4) if sat32 else (torch.int64, 8)
        d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
        d_counts = torch.full((nw + 2,), -1, dtype=edt, device="cuda")
        d_offsets = torch.full((nr + 3,), -1, dtype=torch.int64, device="cuda")
        d_med = torch.full((nr + 2,), -1, dtype=edt, device="cuda")
        d_rows = torch.full((nr + 1, 5), -1, dtype=torch.int64, device="cuda")
        for t in (d_counts, d_offsets, d_med):
            assert t.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        info = ctx.track_device(d_text.data_ptr() + lead, len(text), d_counts.data_ptr() + one, nw, d_offsets.data_ptr() + 8,
                                d_med.data_ptr() + one, d_rows.data_ptr(), nr, 2, sat32=sat32)
        udt = np.uint32 if sat32 else np.uint64
        got_c, got_o, got_m = d_counts.cpu().numpy().view(udt), d_offsets.cpu().numpy().view(np.uint64), d_med.cpu().numpy().view(udt)
        got_r = d_rows.cpu().numpy().view(np.uint64)
        ones = udt(M32 if sat32 else M64)
        assert info["records"] == nr and info["windows_out"] == nw
        assert got_c[1:nw + 1].tolist() == counts.tolist() and got_c[0] == ones == got_c[nw + 1]
        assert got_o[1:nr + 2].tolist() == offsets.tolist() and got_o[0] == M64 == got_o[nr + 2]
        assert got_m[1:nr + 1].tolist() == med.tolist() and got_m[0] == ones == got_m[nr + 1]
        assert got_r[:nr].tolist() == rows.tolist() and (got_r[nr] == M64).all()
        with pytest.raises(native.MercatHipError) as e:
            ctx.track_device(d_text.data_ptr() + lead, len(text), d_counts.data_ptr() + one, nw - 1, 0, 0, 0, 0, 2, sat32=sat32)
        assert e.value.code == RANGE


# ---------------------------------------------------------------------------------------------- above the ABI
def _tsv_rows(path: Path, k: int) -> dict:
    lines = path.read_bytes().split(b"\n")[1:]
    return {line[:k].decode(): int(line[k + 1:]) for line in lines if line}


def _write(path: Path, data: bytes) -> Path:
    path.write_bytes(data)
    return path


def test_track_reads_fasta_and_fastq():
    edge = read_input("edge_reads.fna")
    table = table_of(edge, 5)
    with native.Counter(5, NT) as ctx:
        ctx.count_chunk(edge, 1)
        names, counts, offsets, rows, med = kmers.track_reads(ctx, GOLDEN / "inputs" / "edge_reads.fna")
        tracks = expected_tracks(edge, table, 5)
        assert names == [name for name, _ in ref_records(edge)]
        assert counts.tolist() == [c for v in tracks for c in v] and rows.tolist() == rows_of(tracks)
        assert offsets.tolist() == [0] + np.cumsum([len(v) for v in tracks]).tolist() and med.tolist() == [median_of(v) for v in tracks]
    table = _tsv_rows(GOLDEN / "tsv" / "ref_Test_R1_k5_c10.tsv", 5)
    with native.Counter(5, NT) as ctx:
        ctx.count_chunk(read_input("Test_R1.fna.gz"), 10)
        assert ctx.to_dict() == table
        names, counts, offsets, rows, med = kmers.track_reads(ctx, GOLDEN / "inputs" / "Test_R1.fastq.gz", sat32=True)
        fasta = read_input("Test_R1.fna.gz")
        recs = ref_records(fasta)
        assert names == [name for name, _ in recs] and len(names) > 10 and counts.dtype == np.uint32
        assert len(counts) == sum(max(0, len(seq) - 4) for _, seq in recs) == int(offsets[-1])
        for i in (0, 1, len(recs) // 2, len(recs) - 1):  # a spot check of records against the oracle
            want = [table.get(recs[i][1][j:j + 5], 0) for j in range(len(recs[i][1]) - 4)]
            assert counts[int(offsets[i]):int(offsets[i + 1])].tolist() == want and int(med[i]) == median_of(want)
        assert kmers.track_reads(ctx, GOLDEN / "inputs" / "Test_R1.fastq.gz", median=False)[4] is None


def test_cli_track(tmp_path):
    old = tmp_path / "old" / "tsv_nucleotide"
    old.mkdir(parents=True)
    shutil.copyfile(GOLDEN / "tsv" / "ref_Test_R1_k5_c10.tsv", old / "Test_R1_counts.tsv")
    table = _tsv_rows(GOLDEN / "tsv" / "ref_Test_R1_k5_c10.tsv", 5)
    data = b">r1 first\nACGTACGTTTGACCA\nGGATC\n>r2\nACG\n>r3\nNNNNNNNACGTA\n"
    reads = _write(tmp_path / "reads.fna", data)
    tracks = expected_tracks(data, table, 5)
    names = [name for name, _ in ref_records(data)]
    offsets = [0] + np.cumsum([len(v) for v in tracks]).tolist()
    flat = np.array([c for v in tracks for c in v], dtype=np.uint64)
    for extra in ([], ["-track_sat32"]):
        out = tmp_path / ("out%d" % len(extra))
        assert cli.main(["-tsv", str(tmp_path / "old"), "-k", "5", "-track", str(reads), "-o", str(out)] + extra) == 0
        assert (out / "track_nucleotide" / "Test_R1_track.txt").read_bytes() == report.format_track_txt(names, flat, offsets)
        want = b"record\twindows\tmedian\tsum\tmin\tmax\n"
        for name, v in zip(names, tracks):
            want += b"%s\t%d\t%d\t%d\t%d\t%d\n" % (name.encode(), len(v), median_of(v), sum(v), min(v, default=0), max(v, default=0))
        assert (out / "track_nucleotide" / "Test_R1_median.tsv").read_bytes() == want
        assert not (out / "track_protein").exists()
    assert b">r2\n\n" in report.format_track_txt(names, flat, offsets)
