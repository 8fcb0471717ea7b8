"""The rows kept as text at their seams (tests/text_rows.py makes the texts and keys and states the rule; DESIGN section 7
lists the seams): the by-reference count kernel with its skip, its run compression and its end of stream, the text
table under growth, the row sort and gather, the host merge with the packed rows, and the calls that move text rows
between contexts.  Every comparison is exact: tables against the seq[i:i+k] dictionary filtered per chunk and summed
(the C oracle, which tests/test_text_rows_host.py proves equal to the Python one on every text used here), order against
Python's sorted(), TSV bytes against cpu_ref.tsv_text.  Every count also asserts stats()["windows"] and
stats()["exotic_windows"]: the by-reference kernel took exactly the windows the context cannot pack."""
import numpy as np
import pytest

import text_rows as tr
from mercat2_amd import native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

ALPHABET = {tr.NT2: native.ALPHABET_NT2, tr.AA5: native.ALPHABET_AA5, tr.RAW: native.ALPHABET_RAW}


def counter(alphabet, k):
    return native.Counter(k, ALPHABET[alphabet])


def assert_table(ctx, want: dict, label):
    """export() is the table in sorted() order, rows() its size."""
    want_k, want_c = tr.as_arrays(want, ctx.k)
    assert ctx.rows() == len(want), (label, "rows", ctx.rows(), len(want))
    kmers, counts = ctx.export()
    assert kmers.shape == want_k.shape, (label, "rows exported", kmers.shape, want_k.shape)
    if not (np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)):
        got = dict(zip((bytes(r).decode("ascii", "replace") for r in kmers), counts.tolist()))
        wrong = sorted(key for key in set(got) | set(want) if got.get(key) != want.get(key))
        assert not wrong, (label, "counts differ", len(wrong), [(key, got.get(key), want.get(key)) for key in wrong[:4]])
        assert False, (label, "order differs")


def counted(ctx, alphabet, chunks, c, label):
    """The chunks counted from empty, against the rule: the table, and who took which windows."""
    ctx.reset()
    before = ctx.stats()
    for text in chunks:
        ctx.count_chunk(text, c)
    after = ctx.stats()
    windows, by_ref = tr.by_reference_windows(chunks, ctx.k, alphabet)
    assert after["windows"] - before["windows"] == windows, (label, "windows")
    assert after["exotic_windows"] - before["exotic_windows"] == by_ref, (label, "windows taken by reference")
    want = tr.table_of(chunks, ctx.k, c, big=True)
    assert_table(ctx, want, label)
    return want


def tsv_bytes(ctx, tmp_path, name="s"):
    path = tmp_path / ("%s_counts.tsv" % name)
    if path.exists():
        path.unlink()
    rows = ctx.write_tsv(path, name)
    return rows, (path.read_bytes() if path.exists() else None)


# ----------------------------------------------------------------------------- 1
@pytest.mark.parametrize("alphabet,k", tr.CASES, ids=tr.CASE_IDS)
def test_one_exotic_byte_at_every_bitmap_residue(alphabet, k):
    """64 single exotic bytes 193 symbols apart: every residue mod 64 and mod 32 of the stream.  The first and last
    window over each byte start in other threads and other bitmap words than the byte lies in; both masks of the skip,
    its (hi - 1) >> 6 bound and a thread's last window (start p0 + 31, last byte hi - 1) decide whether they are seen."""
    text, twice = tr.single_exotic_text(alphabet, k), tr.single_exotic_text(alphabet, k, twice=True)
    with counter(alphabet, k) as ctx:
        counted(ctx, alphabet, [text], 1, "one chunk")
        counted(ctx, alphabet, [text, text], 1, "two chunks")
        counted(ctx, alphabet, [twice], 2, "the record twice, c = 2")


# ----------------------------------------------------------------------------- 2
@pytest.mark.parametrize("alphabet,k", tr.CASES, ids=tr.CASE_IDS)
def test_runs_of_one_character(alphabet, k):
    """Runs of N, n (RAW: and A) of k - 1 .. 4000 symbols at every residue mod 32, leading, ending and filling a record,
    between symbols and against a run of another character (one text a place, and one for the run of 4000); over lines
    of 60; with a header line inside.  'N' * k is
    ONE row with the sum of L - k + 1 (same, held, both flushes, the hand-over between threads inside a run)."""
    with counter(alphabet, k) as ctx:
        for ch in tr.run_chars(alphabet):
            for variant in tr.RUN_VARIANTS:
                for place, long in tr.run_parts(variant):
                    text, _ = tr.run_text(alphabet, k, ch, variant, place, long)
                    counted(ctx, alphabet, [text], 1, (chr(ch), variant, place, long))


# ----------------------------------------------------------------------------- 3
@pytest.mark.parametrize("alphabet,k", tr.CASES, ids=tr.CASE_IDS)
def test_the_end_of_the_stream(alphabet, k, tmp_path):
    """A last record of k - 1, k, k + 1 and k + 31 symbols that ends in an exotic byte, the stream's length at every
    residue mod 32, with and without a final newline (p0 + k <= n and the clamp of `last`); and a text without a window."""
    with counter(alphabet, k) as ctx:
        for name in tr.END_LENGTHS:
            for residue in range(tr.RB):
                for newline in (True, False):
                    counted(ctx, alphabet, [tr.end_text(alphabet, k, name, residue, newline)], 1, (name, residue, newline))
        assert counted(ctx, alphabet, [tr.short_only_text(alphabet, k)], 1, "shorter than k") == {}
        assert tsv_bytes(ctx, tmp_path) == (0, None)


# ----------------------------------------------------------------------------- 4
def packed_rows_on_device(ctx, alphabet):
    import torch
    n, w = ctx.rows(), ctx.words_per_key()
    assert w == 2
    keys = torch.zeros((n + 1) * w, dtype=torch.int64, device="cuda:0")
    cnts = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    rows = ctx.export_pairs_device(keys.data_ptr(), cnts.data_ptr(), n + 1)
    words = keys.cpu().numpy().view(np.uint64)[:rows * w].reshape(rows, w).tolist()
    counts = cnts.cpu().numpy().view(np.uint64)[:rows].tolist()
    table = {tr.decode_two_words(hi, lo, ctx.k, alphabet): cnt for (hi, lo), cnt in zip(words, counts)}
    assert len(table) == rows
    return table


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("alphabet,k", tr.SURVIVOR_SHAPES)
def test_survivors_go_to_the_right_table(alphabet, k, c):
    """Two-word contexts: windows that differ in one character only -- ...ACGT..., ...ACGN..., ...acgt... -- go to the
    packed table or to the text table by their bytes; with c = 2 each variant survives or not on its own."""
    text = tr.survivor_text(alphabet, k, c)
    with counter(alphabet, k) as ctx:
        want = counted(ctx, alphabet, [text], c, (alphabet, k, c))
        text_rows = tr.text_rows_of(want, k, alphabet)
        packed = {key: n for key, n in want.items() if key not in text_rows}
        assert text_rows and packed
        kmers, counts = ctx.export_exotic()
        want_k, want_c = tr.as_arrays(text_rows, k)
        assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)
        assert packed_rows_on_device(ctx, alphabet) == packed
        assert ctx.to_dict() == want


# ----------------------------------------------------------------------------- 5
@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("alphabet,k", tr.GROW_SHAPES)
def test_text_table_grows_over_chunks(alphabet, k, c):
    """Eight chunks that double the text rows, every earlier one counted again: the text table is rebuilt about five
    times (HomeRef) and the arena re-reserved with its rows kept (the host test replays mk_grow_run_ref's arithmetic on
    these chunks); c = 2: rows once in each of two chunks are dropped, rows twice in one chunk kept."""
    chunks = tr.grow_chunks(alphabet, k, c)
    summed = {}
    with counter(alphabet, k) as ctx:
        before = ctx.stats()
        for j, text in enumerate(chunks):
            ctx.count_chunk(text, c)
            summed = cpu_ref.merge_counts([summed, tr.table_of([text], k, c, big=True)])
            assert ctx.rows() == len(summed), ("rows after chunk", j)
        after = ctx.stats()
        windows, by_ref = tr.by_reference_windows(chunks, k, alphabet)
        assert (after["windows"] - before["windows"], after["exotic_windows"] - before["exotic_windows"]) == (windows, by_ref)
        assert len(tr.text_rows_of(summed, k, alphabet)) >= 100_000
        assert_table(ctx, summed, (alphabet, k, c))


# ----------------------------------------------------------------------------- 6
@pytest.mark.parametrize("k", tr.ORDER_KS)
def test_order_of_text_rows(k, tmp_path):
    """Chosen keys imported in shuffled order, three batches: the partial last sort word (k = 1, 7, 9, 15, 17, 63, 65,
    129), the pass order of the least-significant-word-first sort (pairs that differ in one byte of one word only, rows
    over two letters that agree in long prefixes), the row index of mk_rows_by_slot_k, and the second and third trip of
    the gather's 64-byte loop (k = 65, 129)."""
    keys, _ = tr.order_keys(k)
    table = tr.order_table(keys)
    counts = np.array([table[key.decode("ascii")] for key in keys], dtype=np.uint64)
    with counter(tr.RAW, k) as ctx:
        third = (len(keys) + 2) // 3
        for a in range(0, len(keys), third):
            ctx.import_exotic(tr.key_rows(keys[a:a + third], k), counts[a:a + third])
        assert_table(ctx, table, k)
        want_k, want_c = tr.as_arrays(table, k)
        kmers, got_c = ctx.export_exotic()
        assert np.array_equal(kmers, want_k) and np.array_equal(got_c, want_c)
        rows, data = tsv_bytes(ctx, tmp_path)
        assert rows == len(table) and data == cpu_ref.tsv_text("s", table).encode("ascii")


# ----------------------------------------------------------------------------- 7
def merged_text(ctxs, names):
    kmers, matrix = native.merged_export(ctxs)
    assert sorted(names) == list(names)
    return "k-mer\t" + "\t".join(names) + "\n" + "".join(
        bytes(row).decode("ascii") + "\t" + "\t".join(str(n) for n in line) + "\n" for row, line in zip(kmers, matrix.tolist()))


@pytest.mark.parametrize("alphabet,k", tr.MERGE_SHAPES)
def test_text_rows_merge_between_packed_rows(alphabet, k, tmp_path):
    """Text keys that sort in front of ('-', digits), between ('N' between G and T) and behind (lower case, '~') the packed
    keys of a dense, a one-word, a two-word and a protein table: merged_rows' memcmp walk, write_view_tsv, and the union
    of two such tables."""
    texts = [tr.merge_text(alphabet, k, seed) for seed in tr.MERGE_SEEDS]
    with counter(alphabet, k) as a, counter(alphabet, k) as b:
        tables = {}
        for name, ctx, text in (("a", a, texts[0]), ("b", b, texts[1])):
            want = counted(ctx, alphabet, [text], 1, (alphabet, k, name))
            assert ctx.to_dict() == want
            rows, data = tsv_bytes(ctx, tmp_path, name)
            assert rows == len(want) and data == cpu_ref.tsv_text(name, want).encode("ascii"), name
            tables[name] = want
        assert merged_text([a, b], ["a", "b"]) == cpu_ref.union_tsv_text(tables)


# ----------------------------------------------------------------------------- 8
@pytest.mark.parametrize("alphabet,k", tr.MOVE_SHAPES)
def test_moving_text_rows_between_contexts(alphabet, k):
    """export_exotic -> import_exotic into an empty context and into one that holds half of the rows (counts add, only
    the other half are new rows), merge_from of overlapping tables, filter_min(3) over counts 1..5, reset() and reuse:
    each against the same arithmetic on dictionaries."""
    text = tr.merge_text(alphabet, k, tr.MOVE_SEED)
    with counter(alphabet, k) as src, counter(alphabet, k) as dst, counter(alphabet, k) as other:
        want = counted(src, alphabet, [text], 1, "source")
        text_rows = tr.text_rows_of(want, k, alphabet)
        packed = {key: n for key, n in want.items() if key not in text_rows}
        kmers, counts = src.export_exotic()
        want_k, want_c = tr.as_arrays(text_rows, k)
        assert np.array_equal(kmers, want_k) and np.array_equal(want_c, counts) and len(text_rows) > 100
        # into an empty context
        dst.import_exotic(kmers, counts)
        assert_table(dst, text_rows, "into an empty context")
        # once more, every second row: counts add, no new row
        dst.import_exotic(kmers[::2], counts[::2])
        half = {key: n for key, n in zip(sorted(text_rows)[::2], want_c[::2].tolist())}
        assert_table(dst, cpu_ref.merge_counts([text_rows, half]), "into a context that holds the rows")
        # a context that holds half of the rows takes all of them: the other half are new
        other.import_exotic(kmers[1::2], counts[1::2] * np.uint64(3))
        assert other.rows() == len(kmers[1::2])
        other.import_exotic(kmers, counts)
        odd = {key: 3 * n for key, n in zip(sorted(text_rows)[1::2], want_c[1::2].tolist())}
        assert_table(other, cpu_ref.merge_counts([text_rows, odd]), "into a context that holds half")
        # merge_from: all rows of src (packed ones too) into `other`
        other.merge_from(src)
        assert_table(other, cpu_ref.merge_counts([text_rows, odd, want]), "merge_from")
        assert_table(src, want, "merge_from left its source alone")
        # filter_min(3) over counts 1..5 as imported
        dst.reset()
        fives = np.arange(len(kmers), dtype=np.uint64) % np.uint64(5) + np.uint64(1)
        dst.import_exotic(kmers, fives)
        imported = dict(zip(sorted(text_rows), fives.tolist()))
        assert set(imported.values()) == {1, 2, 3, 4, 5}
        dst.filter_min(3)
        assert_table(dst, {key: n for key, n in imported.items() if n >= 3}, "filter_min(3) over counts 1..5")
        # and over those counts with a chunk's own added (2 and up; packed rows beside the text rows)
        dst.reset()
        dst.import_exotic(kmers, fives)
        dst.count_chunk(text, 1)
        summed = cpu_ref.merge_counts([dict(zip(sorted(text_rows), fives.tolist())), want])
        assert_table(dst, summed, "import, then a chunk")
        dst.filter_min(3)
        kept = {key: n for key, n in summed.items() if n >= 3}
        assert 0 < len(tr.text_rows_of(kept, k, alphabet)) < len(text_rows)
        assert_table(dst, kept, "filter_min(3) after a chunk")
        # reset and reuse
        dst.reset()
        assert dst.rows() == 0 and dst.export_exotic()[0].shape[0] == 0
        counted(dst, alphabet, [text], 1, "after reset")
