"""No GPU: the numpy restatement of the ORF rule (tests/orf_rule_np.py) against the plain one (tests/orf_rule.py), and
that the texts of tests/orf_scale.py are what they claim to be: their tile counts, the thresholds they pass, and that
ORFs lie across the tile boundaries of the dense texts, so that a wrong carry cannot hide."""
import random

import numpy as np
import pytest

import orf_rule as rule
import orf_rule_np as rule_np
import orf_scale as scale
from test_gpu_orf import MODES

ALPHABETS = ("ACGT", "ACGTN", "GC", "ACGTacgtUuRY", "AT", "ATG")


def test_modes_are_those_of_the_gpu_tests():
    assert list(scale.MODES) == MODES


# ----------------------------------------------------------------------------- the rule on numpy
def random_text(rng, letters: str) -> bytes:
    parts = []
    if rng.random() < 0.3:  # a headless record
        parts.append("".join(rng.choice(letters) for _ in range(rng.randrange(1, 40))) + "\n")
    for i in range(rng.randrange(1, 9)):
        n = rng.choice((0, 1, 2, 3, 4, 5, rng.randrange(6, 60), rng.randrange(60, 400)))
        seq = "".join(rng.choice(letters) for _ in range(n))
        width = rng.choice((7, 60, 1000))
        eol = rng.choice(("\n", "\n", "\r\n", "\r"))
        parts.append(">%s%s\n" % (rng.choice(("r%d" % i, "", "n%%d x", "a_b c")), rng.choice(("", " rest"))))
        parts.append("".join(seq[j:j + width] + eol for j in range(0, n, width)))
    return "".join(parts).encode()


@pytest.mark.parametrize("letters", ALPHABETS)
def test_numpy_rule_is_the_rule(letters):
    rng = random.Random(41 + len(letters))
    for trial in range(10):
        text = random_text(rng, letters)
        assert rule_np.records(text) == rule.records(text)
        for mode in MODES:
            for min_aa in (1, 2, 7):
                assert rule_np.expected(text, min_aa, **mode) == rule.expected(text, min_aa, **mode), (text, mode, min_aa)
    for text in (b"", b"\n\n", b">only\n", b"ACG", b">a\nAC\n>b\n\n>c\nTAA\n", b">s\nATGTAAATG\n", b">r\nCATTTACAT\n"):
        for mode in MODES:
            assert rule_np.expected(text, 1, **mode) == rule.expected(text, 1, **mode), (text, mode)


def test_numpy_rule_on_three_tiles():
    """A text of more than three tiles with '*', CR LF and lower case in it, in every mode."""
    rng = random.Random(43)
    seq = "".join(rng.choice("ACGTacgtN") for _ in range(3 * scale.SPAN + 500))
    starred = seq[:5000] + "*" + seq[5000:20000] + "**" + seq[20000:]
    text = (">three tiles\r\n" + "".join(starred[i:i + 70] + "\r\n" for i in range(0, len(starred), 70))
            + ">tail\n" + seq[:90].lower() + "\n*\n").encode()
    assert scale.tiles_of(text) == 4 and b"*" in text and b"\r\n" in text
    for mode in MODES:
        assert rule_np.expected(text, 1, **mode) == rule.expected(text, 1, **mode), mode
    assert rule_np.expected(text, 32) == rule.expected(text, 32)
    out, rows = rule_np.expected_np(text, 1)
    assert rows.dtype == np.uint64 and rows.tolist() == rule.expected(text, 1)[1]


# ----------------------------------------------------------------------------- the texts
def test_thresholds_follow_the_source():
    f = scale.source_figures()
    assert f["SPAN"] == 256 * f["RUN"] and f["RUN"] % 3 == 0
    assert scale.DENSE_TILES == (f["CARRY_THREADS"], f["CARRY_THREADS"] + 1, f["CARRY_THREADS"] + 2, 2 * f["CARRY_THREADS"] + 1)
    assert [scale.per_thread(t) for t in scale.DENSE_TILES] == [1, 2, 2, 3]
    assert [scale.per_thread(t) for t in scale.FAR_TILES] == [2, 3]
    # at CARRY_THREADS + 1 tiles, two a thread: one thread owns a single tile and all behind it none
    t = scale.CARRY_THREADS + 1
    owned = [max(0, min(t, (i + 1) * 2) - i * 2) for i in range(scale.CARRY_THREADS)]
    assert owned.count(2) == scale.CARRY_THREADS // 2 and owned.count(1) == 1 and owned.count(0) == scale.CARRY_THREADS // 2 - 1


@pytest.mark.parametrize("tiles", scale.DENSE_TILES)
def test_dense_has_its_tiles(tiles):
    text = scale.dense(tiles)
    assert scale.tiles_of(text) == tiles and len(text) + 2 < scale.DEFAULT_PIECE
    recs = rule_np.records(text)
    assert [name for name, _ in recs] == [b"dense", b"short"] and len(recs[1][1]) == scale.DENSE_SHORT
    assert (tiles - 1) * scale.SPAN <= 1 + len(recs[0][1]) < tiles * scale.SPAN  # the second separator: in the last tile
    assert set(recs[0][1]) == set(b"ACGT")


@pytest.mark.parametrize("tiles", scale.DENSE_TILES)
def test_dense_cannot_hide_a_carry_error(tiles):
    """Stop to stop at min_aa 1: at every tile boundary ORFs of at least 3 of the 6 frames lie across it (begin <
    boundary < end in stream coordinates), and every frame lies across at least 80 % of the boundaries.  (Three seeds of
    the 257-tile text gave at least 4 frames at every boundary and 86 to 96 % a frame; at min_aa 32 about half of the
    boundaries have no ORF across them, which is why the dense texts are compared at min_aa 1.)"""
    out, rows = scale.dense_expected(tiles)
    rows = rows[rows[:, 0] == 0].astype(np.int64)
    bounds = np.arange(1, tiles) * scale.SPAN
    across = np.zeros((6, len(bounds)), dtype=bool)
    for f in range(6):
        mine = rows[rows[:, 3] == f + 1]
        begin = 1 + mine[:, 1]  # the record begins at stream position 1
        end = begin + 3 * mine[:, 2]
        order = np.argsort(begin)
        begin, end = begin[order], end[order]
        i = np.searchsorted(begin, bounds, side="left") - 1  # the last ORF of the frame that begins in front of the boundary
        across[f] = (i >= 0) & (end[np.maximum(i, 0)] > bounds)
    assert across.sum(axis=0).min() >= 3
    assert across.mean(axis=1).min() >= 0.8
    assert len(rows) > 80_000 * tiles // 257


@pytest.mark.parametrize("tiles", scale.FAR_TILES)
def test_far_texts(tiles):
    L = scale.far_bases(tiles)
    last = (tiles - 1) * scale.SPAN - 1  # the record position at which the last tile begins
    for variant in scale.FAR_VARIANTS:
        text = scale.far(tiles, variant)
        assert scale.tiles_of(text) == tiles and len(text) + 2 < scale.DEFAULT_PIECE
        (name, seq), = rule_np.records(text)
        assert name == b"far" and len(seq) == L
        plan = scale.far_plan(tiles, variant)
        at = sorted(q for places in plan.values() for q in places)
        assert all(b - a >= 8 for a, b in zip(at, at[1:]))  # no planted word touches another
        assert all(sorted(q % 3 for q in places) == [0, 1, 2] for places in plan.values())
        assert set(np.flatnonzero(~np.isin(np.frombuffer(seq, dtype=np.uint8), list(b"GC"))).tolist()) <= {q + d for q in at for d in range(3)}
        assert all(q + 1 < scale.SPAN for kind in ("fwd_stop_0", "rev_stop_0") for q in plan[kind])  # tile 0
        stop_rows = scale.far_expected(tiles, variant)[1].astype(np.int64)
        start_rows = scale.far_expected(tiles, variant, start=True)[1].astype(np.int64)
        long_rows = stop_rows[stop_rows[:, 2] > 2 * scale.GATHER_BYTES]
        ends = lambda r: r[:, 1] + 3 * r[:, 2]
        if variant in ("stops", "starts"):  # six stretches from tile 0 to the record's end
            assert sorted(long_rows[:, 3].tolist()) == [1, 2, 3, 4, 5, 6]
            assert (long_rows[:, 1] < scale.SPAN).all() and (ends(long_rows) >= L - 2).all()
            assert (long_rows[:, 2] > (tiles - 1) * scale.SPAN // 3 - 400).all()
        if variant == "stops":
            assert len(start_rows) == 0
        if variant == "starts":  # the first ATG and the last CAT win, a few hundred tiles from the closing
            assert sorted(start_rows[:, 3].tolist()) == [1, 2, 3, 4, 5, 6]
            fwd, rev = start_rows[start_rows[:, 3] < 4], start_rows[start_rows[:, 3] >= 4]
            assert sorted(fwd[:, 1].tolist()) == sorted(plan["atg_first"]) and (ends(fwd) >= L - 2).all()
            assert sorted(ends(rev).tolist()) == sorted(q + 3 for q in plan["cat_last"]) and (rev[:, 1] < scale.SPAN).all()
            assert all(scale.SPAN <= q + 1 < 2 * scale.SPAN for q in plan["atg_first"] + plan["cat_first"])
            assert sorted((q + 1) // scale.SPAN for q in plan["cat_last"]) == [scale.NEAR, scale.NEAR + 1, scale.NEAR + 2]
            assert start_rows[:, 2].min() > 2 * scale.GATHER_BYTES
        if variant == "blocked":  # the last CAT lies in front of a later stop: the record's end calls nothing of the reverse strand
            fwd, rev = start_rows[start_rows[:, 3] < 4], start_rows[start_rows[:, 3] >= 4]
            assert sorted(ends(rev).tolist()) == sorted(q + 3 for q in plan["cat_last"])
            assert sorted(fwd[:, 1].tolist()) == sorted(plan["atg_first"] + plan["atg_last"])
            assert sorted(ends(fwd).tolist())[:3] == sorted(plan["fwd_stop_mid"]) and (np.sort(ends(fwd))[3:] >= L - 2).all()
            assert min(plan["rev_stop_behind"]) > max(plan["cat_last"]) and max(plan["rev_stop_behind"]) + 1 < (tiles - 1) * scale.SPAN
        if variant == "closed":  # all six closings are stops in the last tile
            assert all(q >= last for kind in ("fwd_stop_end", "rev_stop_end") for q in plan[kind])
            assert sorted(long_rows[:, 3].tolist()) == [1, 2, 3, 4, 5, 6]
            fwd, rev = long_rows[long_rows[:, 3] < 4], long_rows[long_rows[:, 3] >= 4]
            assert sorted(ends(fwd).tolist()) == sorted(plan["fwd_stop_end"])
            assert sorted(ends(rev).tolist()) == sorted(plan["rev_stop_end"])
            fwd, rev = start_rows[start_rows[:, 3] < 4], start_rows[start_rows[:, 3] >= 4]
            assert sorted(fwd[:, 1].tolist()) == sorted(plan["atg_first"]) and sorted(ends(fwd).tolist()) == sorted(plan["fwd_stop_end"])
            assert sorted(ends(rev).tolist()) == sorted(q + 3 for q in plan["cat_last"])


def test_many_passes_both_thresholds_in_one_piece():
    text = scale.many()
    assert len(text) + 2 < scale.DEFAULT_PIECE
    assert text.count(b">") == scale.MANY_RECORDS > scale.LANES
    pool = len(scale.MANY_POOL)
    head = b"".join(scale._pool_text(i) for i in range(2 * pool + 3))
    assert text.startswith(head) and rule.records(head) == [scale.MANY_POOL[i % pool] for i in range(2 * pool + 3)]
    assert sorted({len(name) for name, _ in scale.MANY_POOL}) == [0, 1, 2, 3]
    assert all(len(seq) <= 9 for _, seq in scale.MANY_POOL) and min(len(seq) for _, seq in scale.MANY_POOL) == 0
    whole, rest = divmod(scale.MANY_RECORDS, pool)
    seq_len = whole * sum(len(s) + 1 for _, s in scale.MANY_POOL) + sum(len(s) + 1 for _, s in scale.MANY_POOL[:rest])
    assert -(-(seq_len + 1) // scale.SPAN) > 2 * scale.CARRY_THREADS  # three tiles a thread of the carry kernel, too
    out, rows = scale.many_expected()
    assert len(rows) > scale.LANES and rows.shape[1] == 4
    per_record = np.bincount(rows[:, 0].astype(np.int64), minlength=scale.MANY_RECORDS)
    assert len(per_record) == scale.MANY_RECORDS and per_record.min() == 0 and 2 <= np.median(per_record) <= 6
    assert (np.diff(rows[:, 0].astype(np.int64)) >= 0).all() and int(rows[-1, 0]) >= scale.MANY_RECORDS - pool
    assert out.count(b">") == len(rows)
    # the shortcut is the rule: on the first cycles and a ragged tail
    small = b"".join(scale._pool_text(i) for i in range(3 * pool + 5))
    w_out, w_rows = rule.expected(small, 1)
    assert out.startswith(w_out) and rows[:len(w_rows)].tolist() == w_rows
