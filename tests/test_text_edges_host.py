"""The seam texts of tests/text_edges.py, checked on the host (no GPU): the unit table is what the sources define, every
generator places what it claims, and the restatements the GPU tests compare with agree with each other on these
texts before the GPU is asked."""
import hashlib
import json

import numpy as np
import pytest

import text_edges as te
from conftest import GOLDEN
from mercat2_amd import native
from oracle import c_oracle, clean_ref, cpu_ref

FQ = json.loads((GOLDEN / "fastq.json").read_text())


def test_unit_table_is_what_the_sources_define():
    """A retuned kernel fails here rather than leaving the sweeps aimed at the wrong offsets.  What this does NOT see: the
    16 bytes a lane loads are written into the kernels as literals, not as a macro, so the 16 (and the 64 lanes of a wave)
    are taken as given here; and the scan's 1024 threads, the FASTQ grid's 2048 and the clean grid's 4096 are found as
    source text (the launch lines), so reformatting one of those lines fails this test without any retune."""
    d = te.source_defines()
    assert te.FAST_UNITS == (16, 64 * 16, d["FP_SUB"] * 1024, d["FP_THREADS"] // 64 * d["FP_SUB"] * 1024)
    assert te.GENERAL_UNITS == (d["PB"], 64 * d["PB"], d["PT"] * d["PB"])
    assert te.FASTQ_UNITS == (16, 64 * 16, d["FQ_TILE"]) and d["FQ_TILE"] == d["FQ_THREADS"] * 16
    fastq = (te.CSRC / "mk_fastq.hip").read_text()
    assert "tiles < %d ? tiles : %d" % (te.FASTQ_APPLY_GRID, te.FASTQ_APPLY_GRID) in fastq
    for fname in ("mk_fparse.hip", "mk_parse.hip", "mk_fastq.hip"):
        assert "dim3(1), dim3(%d)" % te.SCAN_THREADS in (te.CSRC / fname).read_text(), fname
    assert "g > 4096" in (te.CSRC / "mk_clean.hip").read_text()


# ----------------------------------------------------------------------------- planted features
@pytest.mark.parametrize("feature", list(te.FEATURES))
def test_planted_features_sit_at_every_seam(feature):
    feat = te.FEATURES[feature]
    for unit in (te.FAST_UNITS[1], te.GENERAL_UNITS[1]):
        base = te.base_text(te.SWEEP_TOTAL, 0)
        for shift in te.SHIFTS:
            text = te.planted(feature, shift, unit)
            at = te.plant_positions(len(feat), shift, unit, len(text))
            assert len(text) == te.SWEEP_TOTAL and len(at) >= te.SWEEP_TOTAL // unit - 1
            assert all(text[p:p + len(feat)] == feat for p in at)
            assert {p - shift for p in at} >= set(range(unit, te.SWEEP_TOTAL - 64, unit))  # every seam inside the text
            spans = np.zeros(len(text), dtype=bool)
            for p in at:
                spans[p:p + len(feat)] = True
            assert not np.any((np.frombuffer(text, dtype=np.uint8) != np.frombuffer(base, dtype=np.uint8)) & ~spans)  # nothing else
            blank = te.with_inner_blank(text)
            assert blank[te.INNER_BLANK_AT] == 0x20 and len(blank) == len(text)
            assert sum(1 for x, y in zip(blank, text) if x != y) == 1
    # the larger units are multiples of the swept one, so their seams are among the planted ones
    assert all(u % te.FAST_UNITS[1] == 0 for u in te.FAST_UNITS[2:]) and te.GENERAL_UNITS[2] % te.GENERAL_UNITS[1] == 0
    assert te.SWEEP_TOTAL > 2 * te.FAST_UNITS[3]
    # the +-16 shifts sit on lane seams that are no 1 KiB seams; 32-byte thread seams of the general parser likewise
    assert all((1024 + s) % 16 == 0 and (1024 + s) % 1024 for s in (-16, 16))
    if feature == "gt_inner":  # most of them are inside sequence lines (a few fall on line starts and open header lines)
        text = te.planted(feature, 1, 1024)
        stream, _ = te.parse_stream(text)
        assert stream.count(b">") > 40


@pytest.mark.parametrize("feature", list(te.FEATURES))
def test_two_restatements_agree_on_one_text_per_feature(feature):
    for shift, unit in ((-1, 1024), (0, 2048)):
        text = te.planted(feature, shift, unit, 24 * 1024 + 40)
        for k in (5, 31):
            assert cpu_ref.count_text(text, k, 1) == c_oracle.count_dict(text, k, 1), (shift, k)
    text = te.with_inner_blank(te.planted(feature, -1, 2048, 24 * 1024 + 40))
    assert cpu_ref.count_text(text, 31, 1) == c_oracle.count_dict(text, 31, 1)


def test_two_restatements_agree_on_every_byte_value():
    for blank in (False, True):
        text = te.all_bytes_text(blank)
        for k in (5, 31, 33):
            assert cpu_ref.count_text(text, k, 1) == c_oracle.count_dict(text, k, 1), (blank, k)


def test_all_bytes_text_holds_every_value_in_every_place():
    text = te.all_bytes_text()
    lines = text.split(b"\n")
    assert len(te.ALL_BYTES) == 0x7F - 0x21 - 2 and text.count(b" ") == 0
    for v in te.ALL_BYTES:
        ch = bytes([v])
        rec = lines[lines.index(b">b%02x" % v) + 1:][:3]
        assert rec[0][te._RUN:te._RUN + 1] == ch and len(rec[0]) == 2 * te._RUN + 1
        assert rec[1][:1] == ch and rec[2][-1:] == ch
        assert all(set(part) <= set(b"ACGT") for part in (rec[0][:te._RUN], rec[0][te._RUN + 1:], rec[1][1:], rec[2][:-1]))
    blank = te.all_bytes_text(True)
    assert blank.count(b" ") == 1 and len(blank) == len(text)
    at = blank.index(b" ")
    assert blank[at - 1] in b"ACGT" and blank[at + 1] in b"ACGT" and blank[:at].count(b"\n") == 1


# ----------------------------------------------------------------------------- residues, ends, blank runs
def test_residue_texts_walk_the_wave_end_offset_through_every_residue():
    ends = {e: set() for e in te.RESIDUES_E}
    for e in te.RESIDUES_E:
        for r in te.RESIDUES_R:
            text = te.residue_text(r, e)
            assert len(text) < 40 * 1024
            got = te.emitted_per_unit(text, te.FAST_WAVE)
            assert got[1] == 0 and got[2] == e and len(got) >= 4 and got[3] > 100, (r, e, got)
            assert got[0] == te.emitted_per_unit(te.residue_text(0, e), te.FAST_WAVE)[0] + r
            ends[e].add(got[0] % 64)
    assert all(seen == set(range(64)) for seen in ends.values())
    # a packed word (64 symbols) shared by three waves: wave 3 adds fewer than 64 bytes to a word wave 1 began
    assert any(0 < e < 64 for e in te.RESIDUES_E)


def test_end_texts_end_where_they_say():
    texts = te.end_texts()
    assert len(texts) == len(te.FAST_UNITS) * 3 * 3
    for name, text in texts.items():
        seam, s, kind = name.split(":")
        assert len(text) == int(seam) + int(s) and text.endswith(te.END_TAILS[kind]), name
    assert {len(t) for t in texts.values()} == {u + s for u in te.FAST_UNITS for s in (-1, 0, 1)}


def test_blank_runs_cross_their_seams():
    for unit in te.GENERAL_UNITS:
        seam = te.blank_seam(unit)
        assert seam % unit == 0
        for run in te.BLANK_RUNS:
            start = te.blank_run_start(run, unit)
            for after in te.BLANK_AFTER:
                text = te.blank_run_text(run, unit, after)
                assert set(text[start:start + run]) <= set(b" \t") and text[start - 1] in b"ACGT"
                assert start < seam <= start + run  # the run holds the last byte in front of the seam; its end lies behind
                assert b"\n" not in text[start - 30:start] and text[start - 31:start - 30] == b"\n"
                rest = text[start + run:]
                assert {"base": rest[:1] in (b"A", b"C", b"G", b"T"), "eol": rest[:1] == b"\n", "eof": rest == b""}[after]
    assert te.blank_seam(32) % 2048 and te.blank_seam(2048) % 8192  # seams of the smaller unit alone


def test_two_restatements_agree_on_blank_runs():
    for after in te.BLANK_AFTER:
        text = te.blank_run_text(33, 32, after)
        assert cpu_ref.count_text(text, 31, 1) == c_oracle.count_dict(text, 31, 1), after


# ----------------------------------------------------------------------------- long header lines
def test_long_carry_texts_hold_their_header_lines():
    texts = te.long_carry_texts()
    assert sorted(texts) == ["540k-fast", "540k-general", "9m-fast", "9m-general"]
    for name, (text, retries, headers) in texts.items():
        assert len(text) == (540 * te.KIB if name.startswith("540k") else 9 * te.MIB)
        assert text.count(b" ") - sum(text[a:b].count(b" ") for a, b in headers) == retries  # (blanks: header lines, + one)
        for a, b in headers:
            assert text[a:a + 2] == b"\n>" and text[b - 1:b] == b"\n"
            assert b"\n" not in text[a + 1:b - 1] and b"\r" not in text[a + 1:b - 1]
        if retries == 0:
            te.parse_stream(text)  # no blank outside header lines
    # which units the header lines cover: fast-parser waves 62..66 of the small text (scan thread = wave, ballot word = 64)
    (a, b), = te.CARRY_540K
    assert a // te.FAST_WAVE < 64 <= (b - 1) // te.FAST_WAVE and (540 * te.KIB + te.FAST_WAVE - 1) // te.FAST_WAVE <= te.SCAN_THREADS
    # the large text: two units per scan thread in both parsers, a ballot word of the fast parser's scan is 1 MiB
    assert te.SCAN_THREADS < 9 * te.MIB // te.FAST_WAVE <= 2 * te.SCAN_THREADS and te.GENERAL_UNITS[2] == te.FAST_WAVE
    word = 64 * 2 * te.FAST_WAVE
    (a1, b1), (a2, b2), (a3, b3) = te.CARRY_9M
    assert a1 // word + 1 == (b1 - 1) // word and b1 - a1 == 48 * te.KIB
    assert (b2 - 1) // word - a2 // word == 2 and b2 - a2 > 1.2 * te.MIB
    assert b3 - a3 == 20 * te.KIB
    big = texts["9m-fast"][0]
    assert 0.08 < big.count(b"\r\n") / big.count(b"\n") < 0.12 and big.count(b"*") > 1000 and big.count(b"N") > 1000


# ----------------------------------------------------------------------------- FASTQ
def test_fastq_restatement_gives_the_recorded_sed_output():
    assert len(FQ["edge"]) >= 20
    for name, case in FQ["edge"].items():
        text, _ = te.fq_ref(case["text"].encode())
        assert hashlib.sha256(text).hexdigest() == case["sha256"], name


def _all_fastq_texts():
    out = dict(te.fastq_texts())
    for feature in te.FEATURES:
        for shift in te.SHIFTS:
            out["%s%+d" % (feature, shift)] = te.fastq_planted(feature, shift)
    out["big"] = te.fastq_big()
    return out


def test_fastq_restatement_equals_the_host_conversion_on_every_text():
    for name, raw in _all_fastq_texts().items():
        assert te.fq_ref(raw) == native.fq2fa(raw), name


def test_fastq_texts_take_both_parsers():
    """The GPU tests assert which parser counted a FASTQ text; the answer comes from the converted text.  Both happen."""
    named = {name: te.takes_general_parser(te.fq_ref(raw)[0]) for name, raw in te.fastq_texts().items()}
    assert named["extra-lines"] and named["missing-lines"] and not named["at-first-in-tile"] and not named["long-sequence"]
    swept = [te.takes_general_parser(te.fq_ref(te.fastq_planted(f, s))[0]) for f in te.FEATURES for s in te.SHIFTS]
    assert 30 < sum(swept) < len(swept) - 30
    assert not te.takes_general_parser(te.fq_ref(te.fastq_big())[0])
    assert te.takes_general_parser(b">a\nAC GT\n") and te.takes_general_parser(b">a\nACGT \n") and not te.takes_general_parser(b">a b\nACGT\r\n")


def test_fastq_texts_place_what_they_claim():
    t = te.FQ_TILE
    texts = te.fastq_texts()
    assert tuple(texts) == te.FASTQ_NAMES
    a = texts["at-first-in-tile"]
    assert a[t - 1:t + 1] == b"\n@" and a[:t].count(b"\n") % 4 == 0
    kept = {"crlf-split-header": True, "crlf-split-sequence": True, "crlf-split-plus": False, "crlf-split-quality": False}
    for name, keep in kept.items():
        raw = texts[name]
        assert raw[t - 1:t + 1] == b"\r\n", name
        line = raw[:t].count(b"\n") % 4
        assert (line in (0, 1)) == keep, name
        # cut behind the split pair, the conversion counts it exactly when the line is kept
        assert te.fq_ref(raw[:t + 1])[1]["crlf"] - te.fq_ref(raw[:t - 1])[1]["crlf"] == int(keep), name
    for name, line_no in (("long-header-without-at", 0), ("long-sequence", 1), ("long-plus", 2), ("long-quality-with-at", 3)):
        lines = texts[name].split(b"\n")
        long = [i for i, ln in enumerate(lines) if len(ln) >= 20 * te.KIB]
        assert line_no in [i % 4 for i in long], name
        i = [i for i in long if i % 4 == line_no][0]
        assert lines[i][:1] == {0: b"q", 1: lines[i][:1], 2: b"+", 3: b"@"}[line_no]
    assert te.fq_ref(texts["long-header-without-at"])[1]["headers_dropped"] == 1
    for name in ("extra-lines", "missing-lines"):
        raw = texts[name]
        starts = np.flatnonzero(np.frombuffer(b"\n" + raw, dtype=np.uint8)[:-1] == 10)
        phases = {int(np.searchsorted(starts, p, side="right") - 1) % 4 for p in range(len(raw)) if raw[p:p + 2] == b"@q" and (p == 0 or raw[p - 1] == 10)}
        assert phases == {0, 1, 2, 3}, name  # record headers at every phase of the line number
    for feature, feat in te.FEATURES.items():
        for shift in te.SHIFTS:
            raw = te.fastq_planted(feature, shift)
            at = te.plant_positions(len(feat), shift, t, len(raw))
            assert len(raw) == te.FQ_SWEEP_TOTAL and len(at) >= 9 and all(raw[p:p + len(feat)] == feat for p in at)
    big = te.fastq_big()
    tiles = (len(big) + t - 1) // t
    assert tiles > te.FASTQ_APPLY_GRID > te.SCAN_THREADS and tiles <= 2 * te.FASTQ_APPLY_GRID
    st = te.fq_ref(big)[1]
    assert st["reads"] > 5000 and st["headers_dropped"] > 10000  # in phase and out of it
    lines = big.split(b"\n")
    long = [(i % 4, ln[:1]) for i, ln in enumerate(lines) if len(ln) >= 20 * te.KIB]
    assert [ph for ph, _ in long] == [0, 1, 0] and long[0][1] == b"@" and long[2][1] == b"q"  # kept, kept, dropped
    assert lines[-1] == b"" and lines[-5][:2] == b"@r" and (len(lines) - 5) % 4 == 0          # the last block is in phase again


# ----------------------------------------------------------------------------- clean mode
def test_clean_texts_are_accepted_and_hold_their_runs():
    texts = te.clean_texts()
    assert tuple(texts) == te.CLEAN_NAMES and len(texts) == 1 + len(te.CLEAN_FEATURES) * len(te.CLEAN_SHIFTS)
    for name, raw in texts.items():
        stream, _ = te.parse_stream(raw)  # (asserts: no blank in a sequence line)
        headers = stream.count(bytes([te.SEP]))
        assert raw[:1] == b">" and headers >= 1 and raw.count(b">") == headers and b"\x7f" not in raw, name  # every '>' starts a header line
        runs = te.stream_runs(stream)
        assert len(runs) >= 18, name
        for toupper in (False, True):
            cleaned = clean_ref.clean_text(raw.decode(), toupper)[0]  # accepted: no exception
            # something is left to count, and the rewrite cut a record at every run
            assert len(cleaned) > len(raw) // 2 and cleaned.count("\n>") + 1 == headers + len(runs), (name, toupper)
    stream, _ = te.parse_stream(texts["runs"])
    runs = te.stream_runs(stream)
    for n in te.CLEAN_RUNS:
        assert {a % 16 for a, b in runs if b - a == n} >= set(te.CLEAN_RESIDUES), n
        assert {b % 16 for a, b in runs if b - a == n} >= set(te.CLEAN_RESIDUES), n
    for name, feat in te.CLEAN_FEATURES.items():
        for shift in te.CLEAN_SHIFTS:
            raw = texts["%s%+d" % (name, shift)]
            at = te.plant_positions(len(feat), shift, te.CLEAN_UNIT, len(raw), first=te.CLEAN_UNIT)
            assert len(at) >= 23 and min(at) > 61 and all(raw[p:p + len(feat)] == feat for p in at)
            assert raw.count(b"N") == len(at) * len(feat) and raw[:5] == b">r000"
            stream, _ = te.parse_stream(raw)
            assert len(te.stream_runs(stream)) == len(at) >= 23, (name, shift)  # every planted run is in the parsed stream
