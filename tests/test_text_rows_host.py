"""The texts and keys of tests/text_rows.py, checked on the host (no GPU): the unit table is what the sources define,
every builder places what its docstring claims -- at the stream residues it claims, the parsed stream restated plainly as
the records joined by one separator -- and the two references the GPU tests compare with agree on every one of these
texts before the GPU is asked."""
import numpy as np
import pytest

import text_edges as te
import text_rows as tr
from oracle import c_oracle, cpu_ref


def plain_stream(text: bytes) -> bytes:
    """The parsed stream once more, without text_edges: lines; a line that starts with '>' ends a record; the others,
    joined, are the record; one 0 byte where a header line stood."""
    out = []
    for line in text.split(b"\n"):
        if line[:1] == b">":
            out.append(b"\0")
        else:
            out.append(line.replace(b"*", b""))
    return b"".join(out)


def test_unit_table_is_what_the_sources_define():
    """A retuned kernel fails here rather than leaving the builders aimed at the wrong residues.  The 64 positions of a
    bitmap word, the 8 bytes of a sort word and the 64 bytes of a gather step are literals in the kernels: they are
    found as source text, so rewriting those lines fails this test without any retune."""
    u = tr.source_units()
    assert (u["RB"], u["REF_POS_BITS"]) == (tr.RB, tr.REF_POS_BITS)
    assert u["byref_launch_bounds"] == tr.WORKGROUP and u["byref_block"] == [tr.WORKGROUP]
    assert u["bitmap_shift"] == ["6"] and 1 << 6 == tr.BITMAP_WORD
    assert u["sort_word"] == [tr.SORT_WORD] and u["sort_words"]
    assert u["gather_step"] == [tr.GATHER_STEP]
    assert u["row_index_bits"] == [tr.REF_POS_BITS]
    # what the builders take from the table
    assert tr.SINGLE_STEP % tr.BITMAP_WORD == 1 and tr.SINGLE_STEP % tr.RB == 1 and tr.SINGLE_COUNT == tr.BITMAP_WORD
    assert tr.LONG_RUN > 3 * tr.RB * 32 and tr.LONG_RUN // tr.RB > 64   # more threads than a wave inside one run
    assert {tr.SORT_WORD - 1, tr.SORT_WORD, tr.SORT_WORD + 1, tr.GATHER_STEP - 1, tr.GATHER_STEP, tr.GATHER_STEP + 1, 0} == set(tr.ORDER_PAIR_BYTES)
    assert {k % tr.SORT_WORD for k in tr.ORDER_KS} >= {0, 1, 7} and max(tr.ORDER_KS) > 2 * tr.GATHER_STEP  # a third gather trip


def test_the_rule_counts_the_windows_of_the_plain_dictionary():
    """window_counts against the dictionary itself: all windows, and those whose key holds a character outside the letters."""
    text = b"ACGTNACGTacgtAC-GT\n>h\nNN\n>i\nACGNACGTTTGA\nCCA\n"
    assert tr.records_of(text) == [b"ACGTNACGTacgtAC-GT", b"NN", b"ACGNACGTTTGACCA"]
    for letters in (b"ACGT", tr.LETTERS[tr.AA5], b""):
        for k in (1, 2, 3, 5, 15, 16):
            table = cpu_ref.count_text(text, k, 1)
            odd = sum(n for key, n in table.items() if tr.is_text_key(key, letters))
            assert tr.window_counts(text, k, letters) == (sum(table.values()), odd), (letters, k)
    assert tr.window_counts(text, 3, b"") == (16 + 0 + 13,) * 2
    assert not tr.packs(tr.NT2, 65) and tr.packs(tr.NT2, 64) and tr.packs(tr.AA5, 25) and not tr.packs(tr.AA5, 26) and not tr.packs(tr.RAW, 1)


def test_packed_keys_decode_as_the_engine_lays_them_out():
    assert tr.decode_two_words(0x1B << 56, 0, 4, tr.NT2) == "ACGT"
    key = "ACGT" * 8 + "T" + "A" * 7
    hi, lo = tr.encode_two_words(key, tr.NT2)
    assert hi == 0x1B1B1B1B1B1B1B1B and lo == 3 << 62 and tr.decode_two_words(hi, lo, 40, tr.NT2) == key
    assert tr.encode_two_words("BA", tr.AA5) == (0, 32) and tr.decode_two_words(0, 32 * 32 + 25, 3, tr.AA5) == "BAZ"
    for alphabet, k in tr.SURVIVOR_SHAPES:
        key = tr.fill(alphabet, k, k).decode()
        assert tr.decode_two_words(*tr.encode_two_words(key, alphabet), k, alphabet) == key


def _agree(texts, k, c=1):
    for label, text in texts:
        assert tr.clean_text(text), label
        assert plain_stream(text) == tr.stream_of(text), label
        assert cpu_ref.count_text(text, k, c) == c_oracle.count_dict(text, k, c), (label, k, c)


# ----------------------------------------------------------------------------- 1
@pytest.mark.parametrize("alphabet,k", tr.CASES, ids=tr.CASE_IDS)
def test_single_exotic_bytes_take_every_residue(alphabet, k):
    text = tr.single_exotic_text(alphabet, k)
    stream = tr.stream_of(text)
    odd = tr.EXOTICS[alphabet]
    at = [i for i, b in enumerate(stream) if b in odd]
    assert [stream[p] for p in at] == [odd[i % len(odd)] for i in range(64)]
    assert at == [1 + p for p in tr.single_positions()] and len(at) == 64
    assert {p % 64 for p in at} == set(range(64)) and {p % 32 for p in at} == set(range(32))
    assert set(stream[1:]) - set(odd) <= set(tr.FILL[alphabet]) and len(stream) - at[-1] > k + 32
    windows, odd = tr.window_counts(text, k, tr.letters_of(alphabet, k))
    if tr.packs(alphabet, k):  # each exotic byte spoils k windows (they are 193 apart: no window holds two for k <= 193)
        assert odd == 64 * k and windows > odd
    else:
        assert odd == windows
    twice = tr.single_exotic_text(alphabet, k, twice=True)
    assert twice == text + text
    _agree([("once", text), ("twice", twice)], k)
    assert cpu_ref.count_text(twice, k, 2) == c_oracle.count_dict(twice, k, 2)


# ----------------------------------------------------------------------------- 2
@pytest.mark.parametrize("alphabet,k", tr.CASES, ids=tr.CASE_IDS)
def test_runs_start_at_every_residue_in_every_place(alphabet, k):
    for ch in tr.run_chars(alphabet):
        for variant, place_, long in [(v, p, g) for v in tr.RUN_VARIANTS for p, g in tr.run_parts(v)]:
            text, placed = tr.run_text(alphabet, k, ch, variant, place_, long)
            stream = tr.stream_of(text)
            assert tr.clean_text(text) and plain_stream(text) == stream, (ch, variant, place_, long)
            assert len(text) < 400_000
            seen = {}
            for (place, length, r), at, n in placed:
                want = ch if place != "other" else tr._other(ch)
                assert stream[at:at + n] == bytes([want]) * n, (variant, place, length, r)
                if place == "other":
                    assert stream[at - 1] == ch
                    continue
                seen.setdefault((place, length), []).append((r, at, n))
            assert set(seen) == {(place_, n) for n in tr.run_lengths(k, long)}
            for (place, length), runs in seen.items():
                first = {}
                for r, at, n in runs:  # the first piece of every run (a cut run has two)
                    first.setdefault(r, (at, n))
                assert set(first) == set(range(tr.RB)) and all(at % tr.RB == r for r, (at, _) in first.items()), (variant, place, length)
                for r, at, n in runs:
                    before, behind = stream[at - 1], stream[at + n] if at + n < len(stream) else te.SEP
                    if variant == "cut":
                        assert n in (max(1, length // 3), length - max(1, length // 3)) or length == 1
                        assert te.SEP in (before, behind) if length > 1 else True  # a separator lies inside the run
                    elif place == "start":
                        assert before == te.SEP and behind in tr.FILL[alphabet]
                    elif place == "end":
                        assert before in tr.FILL[alphabet] and behind == te.SEP
                    elif place == "whole":
                        assert before == te.SEP and behind == te.SEP
                    elif place == "mid":
                        assert before in tr.FILL[alphabet] and behind in tr.FILL[alphabet]
                    else:
                        assert before in tr.FILL[alphabet] and behind == tr._other(ch)
            if variant == "wrapped":
                assert max(len(line) for line in text.split(b"\n")) == 60
                assert tr.records_of(text) == tr.records_of(tr.run_text(alphabet, k, ch, "plain", place_, long)[0])
            table = cpu_ref.count_text(text, k, 1)
            assert table == c_oracle.count_dict(text, k, 1), (ch, variant)
            if ch in b"Nn":  # (the fill has no N: the rows of one character come from the placed runs alone)
                for c in (ch, tr._other(ch)):
                    runs = [n for (place, _, _), _, n in placed if (place == "other") == (c != ch)]
                    assert table.get(chr(c) * k, 0) == sum(n - k + 1 for n in runs if n >= k), (variant, c)


# ----------------------------------------------------------------------------- 3
@pytest.mark.parametrize("alphabet,k", tr.CASES, ids=tr.CASE_IDS)
def test_end_texts_end_where_they_say(alphabet, k):
    texts = []
    for name in tr.END_LENGTHS:
        n = tr.end_length(name, k)
        seen = set()
        for r in range(tr.RB):
            for newline in (True, False):
                text = tr.end_text(alphabet, k, name, r, newline)
                stream = tr.stream_of(text)
                assert len(stream) % tr.RB == r and text.endswith(b"\n") == newline
                last = tr.records_of(text)[-1]
                assert len(last) == n and (n == 0 or last[-1] == tr.EXOTICS[alphabet][r % len(tr.EXOTICS[alphabet])])
                assert text.count(b">") == 2 and len(tr.records_of(text)[1]) >= k + 40
                seen.add(len(stream) % tr.RB)
                texts.append(((name, r, newline), text))
        assert seen == set(range(tr.RB))
    _agree(texts, k)
    short = tr.short_only_text(alphabet, k)
    assert tr.clean_text(short) and len(tr.records_of(short)[-1]) == k - 1 and cpu_ref.count_text(short, k, 1) == {}
    assert c_oracle.count_dict(short, k, 1) == {}


# ----------------------------------------------------------------------------- 4
@pytest.mark.parametrize("alphabet,k", tr.SURVIVOR_SHAPES)
def test_survivor_texts_differ_in_one_place(alphabet, k):
    letters = tr.letters_of(alphabet, k)
    assert letters  # two-word packed keys
    for c in (1, 2):
        text = tr.survivor_text(alphabet, k, c)
        recs = tr.records_of(text)[1:]
        assert all(len(r) == k + 4 for r in recs)
        groups = {}
        for r in recs:
            mid = (k + 4) // 2 - 2
            groups.setdefault(r[:mid] + r[mid + 4:], []).append(r[mid:mid + 4])
        odd = b"ACG" + tr.EXOTIC[alphabet]
        assert len(groups) == (1 if c == 1 else 8)
        for got in groups.values():
            assert set(got) == {b"ACGT", odd, b"acgt"}
        if c == 2:
            assert sorted(tuple(g.count(v) for v in (b"ACGT", odd, b"acgt")) for g in groups.values()) == \
                sorted((a, b, d) for a in (1, 2) for b in (1, 2) for d in (1, 2))
        table = cpu_ref.count_text(text, k, c)
        text_rows = tr.text_rows_of(table, k, alphabet)
        assert 0 < len(text_rows) < len(table)           # both tables get rows
        if c == 2:
            assert len(table) < len(cpu_ref.count_text(text, k, 1))  # and the filter drops some of each
        _agree([((alphabet, k, c), text)], k, c)


# ----------------------------------------------------------------------------- 5
@pytest.mark.parametrize("alphabet,k", tr.GROW_SHAPES)
def test_grow_chunks_double_the_text_rows(alphabet, k):
    for c in (1, 2):
        chunks = tr.grow_chunks(alphabet, k, c)
        assert len(chunks) == tr.GROW_CHUNKS and all(tr.clean_text(t) and len(t) < 1_000_000 for t in chunks)
        seen, steps, summed = set(), [], {}
        for j, text in enumerate(chunks):
            table = c_oracle.count_dict(text, k, c)
            assert table == cpu_ref.count_text(text, k, c)
            rows = tr.text_rows_of(table, k, alphabet)
            new = set(rows) - seen
            if c == 1:
                assert seen <= set(rows)  # every text row so far is there again
                assert 0.7 * tr.GROW_FIRST * 2 ** j <= len(new) <= 1.1 * tr.GROW_FIRST * 2 ** j + 200, (j, len(new))  # (+ the plain record, where nothing packs)
            steps.append((len(rows), len(new)))
            seen |= set(rows)
            summed = cpu_ref.merge_counts([summed, table])
        assert 100_000 <= len(seen) <= 140_000
        kept, rebuilt = tr.growth_model(steps)
        assert kept >= 3 and 4 <= rebuilt <= 7, (kept, rebuilt)
        if c == 2:
            once = cpu_ref.merge_counts(c_oracle.count_dict(t, k, 1) for t in chunks)
            twice_apart = [key for key, n in once.items() if n == 2 and key not in summed]
            assert len(twice_apart) >= 7 * 10 * k // 2  # once in each of two chunks: in no chunk's table
            assert min(summed.values()) == 2 and max(summed.values()) > 8


# ----------------------------------------------------------------------------- 6
@pytest.mark.parametrize("k", tr.ORDER_KS)
def test_order_keys_hold_their_pairs(k):
    keys, pairs = tr.order_keys(k)
    assert len(set(keys)) == len(keys) and all(len(key) == k and set(key) <= set(tr.KEY_BYTES) for key in keys)
    assert len(keys) >= (3000 if k > 2 else 90) and list(keys) != sorted(keys)
    assert [at for at, _, _ in pairs] == [b for b in sorted({b for b in tr.ORDER_PAIR_BYTES + (k - 1,) if b < k}) for _ in range(tr.ORDER_PAIRS)]
    assert k == 1 or all(len({lo for at, lo, _ in pairs if at == b}) == tr.ORDER_PAIRS for b in {at for at, _, _ in pairs})
    for at, lo, hi in pairs:
        assert lo in keys and hi in keys and [i for i in range(k) if lo[i] != hi[i]] == [at] and lo < hi
    table = tr.order_table(keys)
    assert {len(str(n)) for n in table.values()} == ({1, 10, 20} if len(keys) >= 3 else set())
    assert max(table.values()) < 1 << 64
    if k >= 9:   # rows that agree in their first sort word and differ later
        assert sum(1 for a, b in zip(sorted(keys), sorted(keys)[1:]) if a[:8] == b[:8]) > 50


# ----------------------------------------------------------------------------- 7
@pytest.mark.parametrize("alphabet,k", tr.MERGE_SHAPES)
def test_merge_texts_put_text_keys_around_the_packed_ones(alphabet, k):
    texts = [tr.merge_text(alphabet, k, seed) for seed in tr.MERGE_SEEDS]
    tables = [cpu_ref.count_text(t, k, 1) for t in texts]
    _agree([((alphabet, k, i), t) for i, t in enumerate(texts)], k)
    for table in tables:
        rows = sorted(table)
        kind = [tr.is_text_key(key, tr.letters_of(alphabet, k)) for key in rows]
        assert kind[0] and kind[-1]                                   # text rows in front of and behind every packed row
        flips = sum(1 for a, b in zip(kind, kind[1:]) if a != b)
        assert flips >= 6                                             # and between them, several times
        firsts = {key[0] for key, odd in zip(rows, kind) if odd}
        assert firsts >= set("-09at~") | (set("N") if alphabet == tr.NT2 else set())
        assert {key[0] for key, odd in zip(rows, kind) if not odd} >= set("ACGT")
        assert {key[-1] for key, odd in zip(rows, kind) if odd} >= set("-09at~")
    assert set(tables[0]) & set(tables[1]) and set(tables[0]) - set(tables[1]) and set(tables[1]) - set(tables[0])


# ----------------------------------------------------------------------------- 8
@pytest.mark.parametrize("alphabet,k", tr.MOVE_SHAPES)
def test_move_text_holds_text_rows_of_every_count(alphabet, k):
    text = tr.merge_text(alphabet, k, tr.MOVE_SEED)
    _agree([((alphabet, k), text)], k)
    rows = tr.text_rows_of(cpu_ref.count_text(text, k, 1), k, alphabet)
    assert len(rows) > 100 and (tr.packs(alphabet, k) or len(rows) == len(cpu_ref.count_text(text, k, 1)))
