"""The texts of tests/record_seams.py place what they claim: every header line recomputed from the raw bytes by the
regular expression and by the reference's line loop (tests/filter_rule.py, tests/trim_rule.py), then the coverage of the
placement's seams in the raw text and of the gathers' seams in the output.  No GPU, no library."""
import pytest

import filter_rule
import norm_rule
import record_seams as rs
import trim_rule

NL = b"\n\r"


def starts_of(text: bytes):
    return [m.start() for m in filter_rule.HEADER_LINE.finditer(text)]


def test_units_are_the_sources():
    d = rs.source_defines()
    assert rs.UNITS == (16, d["FL_RUN"], 64 * d["FL_RUN"], 256 * d["FL_RUN"])
    assert d["FL_CHUNKS"] == d["TR_CHUNKS"] and rs.OUT_SEAMS == (64 * 16, 64 * 16 * d["FL_CHUNKS"], 256 * 16 * d["FL_CHUNKS"])
    assert len(rs.table()) == 32 and all(set(key) <= set("AC") and len(key) == rs.K for key in rs.table())
    assert set(rs.BLANKS) == {c for c in range(256) if chr(c).isspace() and c < 128} - set(NL)  # str.strip()'s, less the line ends


# ----------------------------------------------------------------------------------------------- placement
def test_placement_covers_every_unit_shift_and_form():
    text, placed = rs.placement()
    assert len(text) >= 3 * rs.UNITS[3] and len(text) < 1_000_000
    assert {(u, d, f) for u, d, f, _ in placed} == {(u, d, f) for u in rs.UNITS for d in rs.SHIFTS for f in rs.FORMS}
    opens = {m.end() - 1: m.start() for m in filter_rule.HEADER_LINE.finditer(text)}  # the '>' of a header line -> its line's start
    for unit, d, form, t in placed:
        m, rem = divmod(t - d, unit)
        assert rem == 0 and m >= 1 and text[t] == ord(">"), (unit, d, form)
        if unit == 16:
            assert m % 2  # inside a lane, between its two loads
        before = text[:t]
        if form in rs.OPENING:
            line = opens[t]
            assert set(text[line:t]) <= set(rs.BLANKS)
            if form == "lf":
                assert line == t and before.endswith(b"\n") and not before.endswith(b"\r\n")
            elif form == "cr":
                assert line == t and before.endswith(b"\r")
            elif form == "crlf":
                assert line == t and before.endswith(b"\r\n")
            else:
                b = int(form[5:])
                assert t - line == b and text[line - 1] == 10
                if unit >= 32 and b == 33:
                    # the line starts in the previous lane; for d >= 0 in the previous wave / tile
                    assert line // 32 < t // 32 and (unit == 32 or (line // unit < t // unit) == (d >= 0))
        else:
            assert t not in opens
            if form == "in_header":
                assert any(s < t for s in opens if s > t - 4) and 10 not in text[t - 3:t] and 13 not in text[t - 3:t]
            elif form == "after_base":
                assert text[t - 1] in b"ACGT"
            elif form == "after_blanks":
                assert text[t - 1] in rs.BLANKS and text[t - 2] in rs.BLANKS and text[t - 3] in b"ACGT"
            else:
                assert text[t - 1] == ord("*") and text[t - 2] == 10
    # every blank of mk_is_blank stands in front of an opening '>' somewhere, and every one right behind a line start
    assert {text[t - 1] for _, _, f, t in placed if f.startswith("blank")} == set(rs.BLANKS)
    # for the tile: a line that starts in the previous tile
    assert any(opens[t] // 8192 < t // 8192 for u, _, f, t in placed if u == 8192 and f == "blank33")
    assert any(opens[t] // 32 < t // 32 for u, _, f, t in placed if u == 32 and f in ("blank1", "blank2"))
    # CR and LF on either side of a seam of every unit
    for unit in rs.UNITS:
        assert any(f == "crlf" and d == 1 and text[t - 2] == 13 and (t - 1) % unit == 0 for u, d, f, t in placed if u == unit)


def test_placement_records_and_header_bytes():
    text = rs.placement_text()
    ranges, preamble = filter_rule.ref_ranges(text)  # (asserts that the regular expression and the line loop agree)
    assert preamble == 0 and ranges[0][0] == 0
    assert [a for a, _ in ranges] == starts_of(text)
    assert b"".join(raw for raw, _ in norm_rule.records(text)) == text
    keep = filter_rule.expected(text, rs.table(), rs.K, rs.FILTER_RULE, False)[1]
    assert len(keep) > 2000 and all(a != b for a, b in zip(keep, keep[1:]))  # every start a kept/dropped boundary
    # what the SWAR test must not take for '>', in header lines that full lanes read; four '>' in one aligned word
    headers = [(a, text[a:a + len(h)]) for (a, _), (h, _) in zip(ranges, trim_rule.records(text))]
    for byte in b"=?\xbe":
        assert any(byte in h for _, h in headers)
    assert sum(1 for a, h in headers for i in range(len(h) - 3) if h[i:i + 4] == b">>>>" and (a + i) % 4 == 0) > 100
    assert all(c < 128 for _, seq in trim_rule.records(text) for c in seq)
    assert text.count(b"\n=") > 100 and text.count(b"\n?") > 100  # sequence lines: no byte next to '>' in value opens a record
    kept = trim_rule.expected(text, rs.table(), rs.K, rs.TRIM_AT_LEAST)[1]
    assert sum(1 for n in kept if n) > 1000 and sum(1 for n in kept if not n) > 1000


# ----------------------------------------------------------------------------------------------- the end of the text
def test_tail_texts():
    texts = rs.tail_texts()
    for r in range(32):
        for name, end in rs.TAIL_ENDS.items():
            text = texts["%s_%d" % (name, r)]
            assert len(text) == rs.TAIL_BASE + r and text.endswith(end) and text.startswith(b">")
            starts = starts_of(text)
            assert len(starts) == 3 and starts[-1] == len(text) - len(end)
            if len(end) <= r:  # the last header line's '>' in the final partial run, which is read by bytes
                assert starts[-1] >= len(text) - r
            filter_rule.ref_ranges(text)
        assert texts["gt_last_%d" % r][-1] == ord(">")
    assert all(any(len(end) <= r for end in rs.TAIL_ENDS.values()) for r in range(1, 32))
    # tr_hend_k at the end of the text: no terminator, a lone CR, CR LF
    ends = {trim_rule.records(texts["%s_5" % name])[-1][0] for name in rs.TAIL_ENDS}
    assert {b">", b">t", b">t\r", b">t\r\n", b">t\n"} == ends
    assert texts["gt_first"][0] == ord(">") and starts_of(texts["gt_first"])[0] == 0
    for name in ("blanks_gt_first", "blanks40_gt_first"):  # the look-back runs to byte 0
        first = texts[name].index(b">")
        assert first in (3, 40) and set(texts[name][:first]) <= set(rs.BLANKS) and starts_of(texts[name])[0] == 0
    for name in ("headless", "headless_short"):
        assert not filter_rule.ref_records(texts[name])[0][0] and filter_rule.ref_ranges(texts[name])[0][0][0] == 0
    assert texts["gt_only"] == b">"


# ----------------------------------------------------------------------------------------------- gathers
@pytest.mark.parametrize("mode", rs.MODES)
def test_gather_lengths(mode):
    cases = rs.gather_cases(mode)["lengths"]
    for L in rs.LENGTHS:
        if L < rs.MIN_KEPT[mode] and not (L == 1 and mode == "filter"):
            continue  # (no record of trim's is shorter than ">\n", k bases and an LF)
        assert len(rs.emitted(cases["len_%d" % L], mode)) == L, L
    assert len(cases) == (len(rs.LENGTHS) if mode == "filter" else len([L for L in rs.LENGTHS if L >= rs.MIN_KEPT["trim"]]))


def kept_starts(text: bytes, mode: str):
    """[(source offset of the record's first byte, output offset)] of the records ``mode`` emits, and the output's length."""
    out, at = [], 0
    if mode == "filter":
        ranges, _ = filter_rule.ref_ranges(text)
        keep = filter_rule.expected(text, rs.table(), rs.K, rs.FILTER_RULE, True)[1]
        for (a, b), kp in zip(ranges, keep):
            if kp:
                out.append((a, at))
                at += b - a
    else:
        ranges, _ = filter_rule.ref_ranges(text)
        for (a, _), (header, seq) in zip(ranges, trim_rule.records(text)):
            n = trim_rule.kept_of(seq, rs.table(), rs.K, rs.TRIM_AT_LEAST)
            if n:
                out.append((a, at, len(header), n))
                at += len(header) + n + 1
    return out, at


@pytest.mark.parametrize("mode", rs.MODES)
def test_gather_boundaries(mode):
    seams = set()
    for shift in (-1, 0, 1):
        text, claimed = rs.boundaries(mode, shift)
        assert text == rs.gather_cases(mode)["boundaries"]["bound_%+d" % shift]
        found, total = kept_starts(text, mode)
        assert [(f[0], f[1]) for f in found] == claimed[:-1] and total == claimed[-1][1] == len(rs.emitted(text, mode))
        assert 550 <= len(found) <= 900
        sizes = [b[1] - a[1] for a, b in zip(found, found[1:])]
        assert min(sizes) == rs.MIN_KEPT[mode] and max(sizes) == 40
        assert {(f[0] % 16, f[1] % 16) for f in found} == {(a, b) for a in range(16) for b in range(16)}
        seams |= {f[1] for f in found}
        if mode == "trim":  # the header segment, the stream segment and the LF each start at every residue of a chunk
            assert {f[1] % 16 for f in found} == {(f[1] + f[2]) % 16 for f in found} == {(f[1] + f[2] + f[3]) % 16 for f in found} == set(range(16))
    assert {s + d for s in rs.OUT_SEAMS for d in (-1, 0, 1)} <= seams


@pytest.mark.parametrize("mode", rs.MODES)
def test_gather_small_records_runs_tails_and_the_long_record(mode):
    cases = rs.gather_cases(mode)
    lo = rs.MIN_KEPT[mode]
    # minimal records: 16 // lo to a chunk, in a row; a headless first record of 2 bytes
    text = cases["minimal"]["minimal"]
    found, total = kept_starts(text, mode)
    sizes = [b[1] - a[1] for a, b in zip(found, found[1:])]
    assert sizes[:150].count(lo) >= 149 and sizes.count(lo + 1) >= 100 and total == len(rs.emitted(text, mode))
    assert text.startswith(b"A\n>") and not filter_rule.ref_records(text)[0][0]
    assert (found[0][0] == 0) == (mode == "filter")
    # dropped runs: at the start, behind a kept record that ends inside a chunk, at the very end
    for n in rs.RUNS:
        text = cases["dropped_runs"]["drops_%d" % n]
        found, total = kept_starts(text, mode)
        ranges, _ = filter_rule.ref_ranges(text)
        assert len(found) == 2 and len(ranges) == 3 * n + 2 and (found[1][1] % 16, total % 16) == (21 % 16, 58 % 16)
        index = [i for i, (a, _) in enumerate(ranges) if a in (found[0][0], found[1][0])]
        assert index == [n, 2 * n + 1]
        text = cases["dropped_runs"]["drops_last_%d" % n]  # the run in front of the last row, which is kept
        found, total = kept_starts(text, mode)
        ranges, _ = filter_rule.ref_ranges(text)
        assert len(found) == 2 and len(ranges) == n + 2 and (found[0][0], found[1][0]) == (0, ranges[-1][0]) and total == 58
    # the last record kept: shorter than 16, 16 .. 32, longer; every residue of n; with and without the last newline
    seen = set()
    for name, text in cases["last32"].items():
        found, total = kept_starts(text, mode)
        ranges, _ = filter_rule.ref_ranges(text)
        assert found[-1][0] == ranges[-1][0] and total == len(rs.emitted(text, mode)) and len(text) >= 64
        size = total - found[-1][1]
        assert size == int(name.split("_")[1]) and text.endswith(b"\n") == name.endswith("_lf")
        seen.add((0 if size < 16 else 1 if size <= 32 else 2, len(text) % 16, text.endswith(b"\n")))
    assert len(seen) == 3 * 16 * 2
    # one long record of more than 48 KiB of output behind 100 short ones
    text = cases["long"]["long"]
    found, total = kept_starts(text, mode)
    sizes = [b[1] - a[1] for a, b in zip(found, found[1:] + [(0, total)])]
    at = sizes.index(max(sizes))
    assert max(sizes) > 48 * 1024 and at == 50 and len(found) == 52 and len(filter_rule.ref_ranges(text)[0]) == 103


def test_header_alone_text():
    text = rs.header_alone_text()
    recs = trim_rule.records(text)
    filter_rule.ref_ranges(text)
    alone = [len(h) for h, seq in recs if not seq]
    assert alone.count(2) > 80 and alone.count(3) > 40 and recs[-1] == (b">", b"")
    assert sum(1 for _, seq in recs if 0 < len(seq) < rs.K) == 40 and sum(1 for _, seq in recs if len(seq) >= 2 * rs.K) == 40
    run = best = 0
    for h, seq in recs:
        run = run + 1 if (h == b">\n" and not seq) else 0
        best = max(best, run)
    assert best >= 8  # a whole chunk of them


# ----------------------------------------------------------------------------------------------- many tiles
def test_many_tiles_text():
    text, recs = rs.many_tiles()
    assert len(text) > 8 << 20 and len(text) > rs.SCAN_THREADS * rs.UNITS[3]
    symbols = sum(len(seq) + 1 for _, _, seq in recs)
    assert symbols > rs.SCAN_THREADS * 8192  # (SC_SPAN: tests/test_walk_seams_host.py pins it)
    assert 125 <= len(recs) <= 140 and len({seq for _, _, seq in recs if len(seq) > 60_000}) == 4
    # the records are where the builder says: every '>' of the text, the pad line's own aside, opens one
    at, found = text.find(b">"), []
    while at >= 0:
        if at == 0 or text[at - 1] == 10:
            found.append(at)
        at = text.find(b">", at + 1)
    assert found == [a for a, _, _ in recs]
    for (a, header, seq), end in zip(recs, found[1:] + [len(text)]):
        assert text[a:a + len(header)] == header and header.endswith(b"\n") and header.count(b"\n") == 1
        body = text[a + len(header):end]
        assert body.replace(b"\n", b"") == seq and (not seq or body.endswith(b"\n")) and b"\r" not in body and b"*" not in body
    starts = set(found)
    assert {rs.MANY_SEAM - 1, rs.MANY_SEAM + 1, rs.MANY_SEAM + 8192} <= starts
    want = rs.many_tiles_expected()
    assert want["distinct"] == 6  # the four long sequences, the short one, none: each computed once
    assert len(want["plain"]) + len(want["inverted"]) == len(text)
    assert 0 < sum(want["matched"]) < len(recs) and 0 < sum(1 for n in want["kept"] if n) < sum(want["matched"])
    # the cache is no shortcut: two records recomputed from their own bytes
    for i in (1, len(recs) - 1):
        a, end = found[i], (found[i + 1] if i + 1 < len(found) else len(text))
        assert filter_rule.ref_rows(text[a:end], rs.table(), rs.K, 1) == [want["rows"][i]]
        assert trim_rule.expected(text[a:end], rs.table(), rs.K, rs.TRIM_AT_LEAST)[1] == [want["kept"][i]]
