"""K-mer panels looked up in the GPU tables (mk_lookup / mk_lookup_device / mk_lookup_text / mk_lookup_file, Counter.lookup*,
native.lookup_multi, report.write_query_tsv, -query).  The expected answer of a lookup is ``table.get(key, 0)``: from the
count tables the reference made, from ``to_dict()`` of the same context, or from the CPU oracle."""
import ctypes
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

from conftest import read_input
from mercat2_amd import cli, kmers, native, report
from mercat2_amd.chunker import chunk_offsets
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE, NON_ASCII, RANGE = -1, -4, -5, -7


def _rows(path: Path, k: int):
    """(keys, counts) of a committed count table, by the row rules of the header: k key bytes, a tab, the count."""
    lines = path.read_bytes().split(b"\n")[1:]
    if lines[-1] == b"":
        lines.pop()
    assert all(line[k:k + 1] == b"\t" for line in lines)
    return [line[:k] for line in lines], [int(line[k + 1:]) for line in lines]


def _absent_variant(key: bytes, taken: set, rng: random.Random) -> bytes:
    """key with one byte changed so that the table lacks it."""
    for _ in range(200):
        at = rng.randrange(len(key))
        new = key[:at] + bytes([rng.choice(b"ACGTNKXacgt*_ ")]) + key[at + 1:]
        if new != key and new not in taken:
            return new
    raise AssertionError("no absent variant of %r" % key)


# ------------------------------------------------------------------------------- tables the reference made
# table -> (the golden input it came from, alphabet, min_count, chunk bytes)
REFERENCE = {
    "ref_RW1_clean_k5_c10": ("RW1_clean.fna.gz", NT, 10, 0),
    "ref_RW1_pro_k5_c10": ("RW1_pro.faa.gz", AA, 10, 0),
    "ref_RW1_fgs_k5_c10": ("RW1_fgs.faa.gz", AA, 10, 0),
    "ref_Test_R1_k5_c10": ("Test_R1.fna.gz", NT, 10, 0),
    "ref_DJ_pro_k5_c10_s1": ("DJ_pro.faa.gz", AA, 10, 1 << 20),
    "A_k31_c1": ("A.fasta", NT, 1, 0),
    "Scaffolds_with-NNN_k5_c10": ("Scaffolds_with-NNN.fna.gz", NT, 10, 0),
    "edge_ws_k3_c1": ("edge_ws.fa", NT, 1, 0),
    "edge_ws_k5_c1": ("edge_ws.fa", NT, 1, 0),
    "edge_ws_k31_c1": ("edge_ws.fa", NT, 1, 0),
    "edge_lengths_k32_c2": ("edge_lengths.fa", NT, 2, 0),
    "edge_protein_k3_c2": ("edge_protein.faa", AA, 2, 0),
}


@pytest.mark.parametrize("name", sorted(REFERENCE))
def test_reference_tables(name):
    source, alphabet, c, chunk = REFERENCE[name]
    path = GOLDEN / "tsv" / (name + ".tsv")
    k = native.tsv_shape(path)["k"]
    keys, counts = _rows(path, k)
    taken = set(keys)
    rng = random.Random(name)
    absent = [_absent_variant(key, taken, rng) for key in keys]
    with native.Counter(k, alphabet) as counted, native.Counter(k, alphabet) as loaded:
        data = read_input(source)  # counted as the reference counted it: -s 1 cuts the inflated text into 1 MiB chunks
        offs = chunk_offsets(data, chunk) if chunk and len(data) >= chunk else [0, len(data)]
        for a, b in zip(offs[:-1], offs[1:]):
            counted.count_chunk(memoryview(data)[a:b], c)
        loaded.load_tsv(path)
        for ctx in (counted, loaded):
            got, info = ctx.lookup_text(path)
            assert got.tolist() == counts
            assert info["header"] == 1 and info["keys"] == info["found"] == len(keys) and info["lines"] == len(keys) + 1
            assert info["packed_keys"] + info["text_keys"] == len(keys) and info["bytes"] == path.stat().st_size
            assert ctx.lookup(keys).tolist() == counts
            assert not ctx.lookup(absent).any()
            if name.startswith("Scaffolds"):
                assert info["text_keys"] > 0 and any(b"N" in key for key in keys)
            if name == "edge_lengths_k32_c2":
                assert ctx.lookup([b"T" * 32]).tolist() == [338] == [counts[keys.index(b"T" * 32)]]
            if name.startswith("edge_ws"):
                odd = [i for i, key in enumerate(keys) if b"\t" in key or b" " in key]
                # (blanks at every k; tabs at k = 3 and 5: no 31 bytes of edge_ws.fa that hold a tab are a key)
                assert any(b" " in keys[i] for i in odd) and any(b"\t" in keys[i] for i in odd) == (k < 31)
                assert all(got[i] == counts[i] > 0 for i in odd)


# ------------------------------------------------------------------------------------ every table shape
def _synth() -> bytes:
    # (the last record holds bytes outside both alphabets: keys kept as text in every packed context)
    return native.synth_reads(30_000, 3, 1_500, 150, 4).tobytes() + b">odd\n" + b"ACGTTGCANGGATCCATGNAacgtACGGT*CA" * 8 + b"\n"


SHAPES = [("nt", NT, k) for k in (3, 21, 31, 32, 33, 63, 64, 70)] + [("aa", AA, k) for k in (3, 5, 12, 13, 25)] + [("raw", RAW, 9)]


def _device_lookup(ctx, keys, fold=None):
    import torch
    flat = np.frombuffer(b"".join(keys), dtype=np.uint8)
    d_keys = torch.from_numpy(flat.copy()).cuda()
    d_out = torch.full((len(keys),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    info = ctx.lookup_device(d_keys.data_ptr(), len(keys), d_out.data_ptr(), fold)
    return d_out.cpu().numpy().view(np.uint64), info


@pytest.mark.parametrize("kind,alphabet,k", SHAPES, ids=["%s_k%d" % (s[0], s[2]) for s in SHAPES])
def test_every_table_shape_against_to_dict(kind, alphabet, k):
    rng = random.Random(k * 7 + alphabet)
    with native.Counter(k, alphabet) as ctx:
        ctx.count_chunk(_synth(), 1)
        table = {key.encode(): n for key, n in ctx.to_dict().items()}
        present = sorted(table)
        if len(present) > 200_000:
            present = rng.sample(present, 200_000)
        letters = b"ACGTN" if k < 12 else b"ACGT"
        absent = []
        while len(absent) < len(present):
            key = bytes(rng.choice(letters) for _ in range(k))
            if key not in table:
                absent.append(key)
        panel = present + absent
        panel += rng.choices(panel, k=len(panel) // 10 + 1)  # duplicates
        rng.shuffle(panel)
        want = [table.get(key, 0) for key in panel]
        info = {}
        assert ctx.lookup(panel, info=info).tolist() == want
        got_dev, info_dev = _device_lookup(ctx, panel)
        assert got_dev.tolist() == want
        got_text, info_text = ctx.lookup_text(b"\n".join(panel) + b"\n")
        assert got_text.tolist() == want
        for i in (info, info_dev, info_text):
            assert i["keys"] == len(panel) and i["found"] == sum(1 for n in want if n)
            assert i["packed_keys"] + i["text_keys"] == len(panel) and i["folded"] == 0
            if alphabet == RAW or k == 70:
                assert i["text_keys"] == len(panel)
            else:
                assert i["text_keys"] == sum(1 for key in panel if not set(key) <= (set(b"ACGT") if alphabet == NT else set(range(65, 91))))
        assert info_text["header"] == 0 and info_text["pieces"] == 1 and info_text["lines"] == len(panel)
        assert any(b"N" in key and table.get(key) for key in panel)  # (keys kept as text are among the ones found)
        some = [key.decode() for key in panel[:5]]
        assert kmers.lookup_kmers(ctx, some) == {key: table.get(key.encode(), 0) for key in some}


# -------------------------------------------------------------------------------------------- canonical
def _rc(key: bytes) -> bytes:
    return key.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


@pytest.mark.parametrize("k", [31, 63])
def test_canonical_fold(k):
    rng = random.Random(k)
    with native.Counter(k, NT, canonical=True) as ctx:
        ctx.count_chunk(_synth(), 1)
        table = {key.encode(): n for key, n in ctx.to_dict().items()}
        acgt = [key for key in sorted(table) if set(key) <= set(b"ACGT")]
        keys = rng.sample(acgt, 3000) + [key for key in table if b"N" in key][:20]
        keys += [bytes(rng.choice(b"ACGT") for _ in range(k)) for _ in range(500)]  # absent either way round
        turned = [_rc(key) if set(key) <= set(b"ACGT") else key for key in keys]
        want = [table.get(min(key, _rc(key)) if set(key) <= set(b"ACGT") else key, 0) for key in keys]
        info = {}
        assert ctx.lookup(keys, fold=True).tolist() == want == ctx.lookup(keys).tolist()  # (None: the context is canonical)
        assert ctx.lookup(turned, fold=True, info=info).tolist() == want
        assert info["folded"] == sum(1 for key in turned if set(key) <= set(b"ACGT") and _rc(key) < key)
        assert _device_lookup(ctx, turned, True)[0].tolist() == want
        assert ctx.lookup_text(b"\n".join(turned), fold=True)[0].tolist() == want
        # as they stand: the other strand of a canonical key is not in the table
        assert ctx.lookup(turned, fold=False).tolist() == [table.get(key, 0) for key in turned]
        assert ctx.lookup([_rc(key) for key in acgt[:200] if _rc(key) not in table], fold=False).sum() == 0


def test_fold_is_refused_where_it_means_nothing():
    with native.Counter(5, AA) as aa, native.Counter(31, NT) as plain:
        for ctx in (aa, plain):
            with pytest.raises(native.MercatHipError) as e:
                ctx.lookup([b"A" * ctx.k], fold=True)
            assert e.value.code == ARG and "MK_LOOKUP_FOLD" in str(e.value)
            with pytest.raises(native.MercatHipError) as e:
                ctx.lookup_text(b"A" * ctx.k + b"\n", fold=True)
            assert e.value.code == ARG
            assert ctx.lookup([b"A" * ctx.k]).tolist() == [0]


def test_key_arrays_are_taken_as_bytes_or_refused():
    with native.Counter(5, NT) as ctx:
        ctx.load_tsv(GOLDEN / "tsv" / "ref_RW1_clean_k5_c10.tsv")
        keys = [key.encode() for key in sorted(ctx.to_dict())[:7]] + [b"NNNNN"]
        want = ctx.lookup(keys).tolist()
        assert min(want[:7]) > 0
        flat = np.frombuffer(b"".join(keys), dtype=np.uint8)
        for form in (np.array(keys, dtype="S5"), flat, flat.reshape(-1, 5), np.repeat(np.array(keys, dtype="S5"), 2)[::2]):
            assert ctx.lookup(form).tolist() == want
        for bad in (flat.astype(np.int64), np.array(keys, dtype="S6"), flat.astype(np.float32)):
            with pytest.raises(TypeError):
                ctx.lookup(bad)
        with pytest.raises(ValueError):
            ctx.lookup(flat[:-1])


# ----------------------------------------------------------------------------------------------- pieces
def _pieces_of(text: bytes, piece: int, k: int) -> int:
    """How many pieces the pinned double buffer cuts the text into (the rule of mk_load_tsv)."""
    piece = min(max(piece, 2 * (k + 24)), 1 << 30)
    pos, carry, eof, n = 0, b"", False, 0
    while not (eof and not carry):
        have, carry = carry, b""
        if not eof:
            got = text[pos:pos + piece - len(have)]
            pos += len(got)
            eof = len(got) < piece - len(have)
            have += got
        if not have:
            break
        if not eof:
            carry = have[have.rfind(b"\n") + 1:]
        n += 1
    return n


def test_pieces_give_the_same_counts():
    k = 31
    rng = random.Random(5)
    with native.Counter(k, NT) as ctx:
        ctx.count_chunk(_synth(), 1)
        table = {key.encode(): n for key, n in ctx.to_dict().items()}
        keys = rng.sample(sorted(table), 1500) + [bytes(rng.choice(b"ACGTN") for _ in range(k)) for _ in range(1500)]
        rng.shuffle(keys)
        text = b"k-mer\tpanel\n" + b"".join(key + (b"\t%d\n" % rng.randrange(10 ** rng.randrange(1, 20)) if i % 3 else b"\n")
                                            for i, key in enumerate(keys))
        want = [table.get(key, 0) for key in keys]
        first_rows = len(b"k-mer\tpanel\n") + 32  # a piece that ends right behind the '\n' of data row 0 (which has no count)
        assert text[first_rows - 1:first_rows] == b"\n"
        for piece in (1, 2 * (k + 24), 111, 127, first_rows + 2 * (k + 24), 1000, 4096, 4097, len(text) - 1, len(text), len(text) + 1, 0):
            got, info = ctx.lookup_text(text, piece_bytes=piece)
            assert got.tolist() == want, piece
            assert info["keys"] == len(keys) and info["header"] == 1 and info["lines"] == len(keys) + 1 and info["bytes"] == len(text)
            assert info["pieces"] == (_pieces_of(text, piece, k) if piece else 1), piece
        assert ctx.lookup_text(text[:-1])[0].tolist() == want  # (the last line may lack its '\n')


# --------------------------------------------------------------------------------------------- refusals
REFUSED = [
    ("key_too_short", b"AAAAA\nACGT\nCCCCC\n", RANGE, "line 2"),
    ("key_too_long", b"AAAAA\nCCCCC\nACGTAC\n", RANGE, "line 3"),
    ("carriage_return", b"AAAAA\nACGTA\r\n", RANGE, "line 2"),
    ("empty_line", b"AAAAA\n\nCCCCC\n", RANGE, "line 2"),
    ("count_not_digits", b"AAAAA\nACGTA\tabc\n", RANGE, "line 2"),
    ("count_21_digits", b"AAAAA\t7\nCCCCC\nACGTA\t123456789012345678901\n", RANGE, "line 3"),
    ("count_beyond_64_bits", b"AAAAA\nACGTA\t18446744073709551616\n", RANGE, "line 2"),
    ("tab_and_nothing", b"AAAAA\nACGTA\t\n", RANGE, "line 2"),
    ("byte_above_ascii", b"AAAAA\nAC\xc3\xa9A\n", NON_ASCII, "line 2"),
    ("header_then_bad", b"k-mer\tx\nAAAAA\nAAAA\n", RANGE, "line 3"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refusals_name_the_line_and_leave_the_table(case):
    _, text, code, line = case
    with native.Counter(5, NT) as ctx:
        ctx.load_tsv(GOLDEN / "tsv" / "Scaffolds_with-NNN_k5_c10.tsv")
        before = ctx.to_dict()
        with pytest.raises(native.MercatHipError) as e:
            ctx.lookup_text(text)
        assert e.value.code == code and line + ":" in str(e.value)
        with pytest.raises(native.MercatHipError) as e:  # the same in a later piece
            ctx.lookup_text(b"ACGTA\t1\n" * 40 + text.split(b"\n", 1)[1], piece_bytes=64)
        assert e.value.code == code and "line %d:" % (int(line.split()[1]) + 39) in str(e.value)
        assert ctx.to_dict() == before and ctx.lookup([b"AAAAA"]).tolist() == [before["AAAAA"]]


def test_non_ascii_key_and_small_cap():
    L = native.lib()
    with native.Counter(5, NT) as ctx:
        ctx.load_tsv(GOLDEN / "tsv" / "ref_RW1_clean_k5_c10.tsv")
        before = ctx.to_dict()
        with pytest.raises(native.NonAsciiInput) as e:
            ctx.lookup([b"AAAAA", b"ACGTA", b"AC\xffTA"])
        assert e.value.code == NON_ASCII and "key 2" in str(e.value)
        three = [key.encode() for key in sorted(before)[:3]]
        text = three[0] + b"\n" + three[1] + b"\t3\n" + three[2] + b"\n"
        counts = np.full(8, 12345, dtype=np.uint64)
        rows, st = ctypes.c_size_t(0), native.Lookup()
        rc = L.mk_lookup_text(ctx._h, text, len(text), 0, 0, counts.ctypes.data, 1, ctypes.byref(rows), ctypes.byref(st))
        assert rc == RANGE and rows.value == 3 and (counts[1:] == 12345).all()
        rc = L.mk_lookup_text(ctx._h, text, len(text), 0, 0, counts.ctypes.data, 3, ctypes.byref(rows), ctypes.byref(st))
        assert rc == 0 and rows.value == 3 and counts[:3].tolist() == [before[key.decode()] for key in three]
        assert (counts[3:] == 12345).all() and st.keys == 3 and st.found == 3
        assert ctx.to_dict() == before


# -------------------------------------------------------------------------------------------- read-only
def test_lookups_leave_the_table_as_it_was():
    with native.Counter(31, NT) as ctx:
        ctx.count_chunk(_synth(), 1)
        before = (ctx.rows(), ctx.export(), ctx.alpha_stats())
        keys = [bytes(row) for row in before[1][0][:2000]] + [b"N" * 31, b"A" * 31]
        for _ in range(3):
            ctx.lookup(keys)
            ctx.lookup_text(b"\n".join(keys))
        after = (ctx.rows(), ctx.export(), ctx.alpha_stats())
        # (sum_clnc too: it is added in an order the table fixes, so an unchanged table gives the same bits)
        assert before[0] == after[0] and before[2] == after[2]
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()


@pytest.mark.parametrize("alphabet,k", [(NT, 3), (NT, 31), (NT, 63), (AA, 13), (RAW, 9), (NT, 70)])
def test_empty_context_answers_zero(alphabet, k):
    with native.Counter(k, alphabet) as ctx:
        keys = [b"A" * k, b"ACGTN"[:1] * (k - 1) + b"N", b"T" * k]
        assert ctx.lookup(keys).tolist() == [0, 0, 0]
        got, info = ctx.lookup_text(b"\n".join(keys))
        assert got.tolist() == [0, 0, 0] and info["found"] == 0 and info["keys"] == 3
        assert ctx.lookup([]).tolist() == [] and ctx.lookup_text(b"")[0].tolist() == []
        assert ctx.rows() == 0


def test_lookup_right_after_fused_chunks():
    """Chunks whose count kernel puts the survivors into the running table itself, row totals read back without waiting:
    a lookup that follows at once sees the final counts."""
    data = native.synth_reads(60_000, 21, 120_000, 150, 22).tobytes()
    offs = [0] + [int(x) for x in native.chunk_cuts(data, 4_000_000)] + [len(data)]
    assert len(offs) > 4
    with native.Counter(31, NT) as ctx:
        for a, b in zip(offs[:-1], offs[1:]):
            ctx.count_chunk(memoryview(data)[a:b], 2)
        start = data.index(b"\n", offs[-2]) + 1  # the first read of the last chunk
        probe = [data[j:j + 31] for j in range(start, start + 100)] + [b"A" * 31]
        got = ctx.lookup(probe).tolist()
        assert ctx.stats()["fused_chunks"] == len(offs) - 2
        table = ctx.to_dict()
        assert got == [table.get(key.decode(), 0) for key in probe] and min(got[:-1]) > 0


# -------------------------------------------------------------------------------------------- spread tables
def test_lookup_multi_over_key_ranges():
    data = native.synth_reads(50_000, 3, 4_000, 150, 4).tobytes()
    half = data.index(b">", len(data) // 2)
    rng = random.Random(1)
    ctxs = [native.Counter(31, NT) for _ in range(2)]
    try:
        ctxs[0].count_chunk(data[:half], 1)
        ctxs[1].count_chunk(data[half:], 1)
        native.merge_devices(ctxs, native.MERGE_RANGES | native.MERGE_BALANCED)
        kmers_, counts = native.export_multi(ctxs)
        whole = {bytes(row): int(n) for row, n in zip(kmers_, counts)}
        assert all(c.rows() for c in ctxs)
        panel = rng.sample(sorted(whole), 5000) + [bytes(rng.choice(b"ACGT") for _ in range(31)) for _ in range(5000)]
        rng.shuffle(panel)
        assert native.lookup_multi(ctxs, panel).tolist() == [whole.get(key, 0) for key in panel]
    finally:
        for c in ctxs:
            c.close()


# -------------------------------------------------------------------------------------------------- CLI
def _query_table(names, tables, keys) -> bytes:
    lines = ["k-mer\t" + "\t".join(names) + "\n"]
    out = [lines[0].encode()]
    for key in keys:
        out.append(key + b"".join(b"\t%d" % tables[name].get(key, 0) for name in names) + b"\n")
    return b"".join(out)


def test_cli_query_from_loaded_tables(tmp_path):
    old = tmp_path / "old"
    (old / "tsv_nucleotide").mkdir(parents=True)
    (old / "tsv_protein").mkdir()
    placed = {"RW1": ("tsv_nucleotide", "ref_RW1_clean_k5_c10"), "Test_R1": ("tsv_nucleotide", "ref_Test_R1_k5_c10"),
              "RW1_pro": ("tsv_protein", "ref_RW1_pro_k5_c10")}
    tables = {}
    for sample, (folder, name) in placed.items():
        shutil.copyfile(GOLDEN / "tsv" / (name + ".tsv"), old / folder / (sample + "_counts.tsv"))
        tables[sample] = dict(zip(*_rows(GOLDEN / "tsv" / (name + ".tsv"), 5)))
    keys = sorted(tables["RW1"])[:40] + sorted(tables["RW1_pro"])[100:140] + [b"NNNNN", b"A\tG A", b"ZZZZZ", b"ACGTA", b"ACGTA"]
    panel = tmp_path / "panel.txt"
    panel.write_bytes(b"".join(key + (b"\t9\n" if i % 2 else b"\n") for i, key in enumerate(keys)))
    out = tmp_path / "out"
    assert cli.main(["-tsv", str(old), "-k", "5", "-query", str(panel), "-o", str(out)]) == 0
    assert (out / "query_Nucleotide.tsv").read_bytes() == _query_table(["RW1", "Test_R1"], tables, keys)
    assert (out / "query_protein.tsv").read_bytes() == _query_table(["RW1_pro"], tables, keys)
    # a panel row of another length ends the run with its line
    panel.write_bytes(b"ACGTA\nACGTAC\n")
    with pytest.raises(SystemExit) as e:
        cli.main(["-tsv", str(old), "-k", "5", "-query", str(panel), "-o", str(tmp_path / "out2")])
    assert "line 2" in str(e.value)


def test_cli_query_for_a_counted_sample(tmp_path):
    data = (GOLDEN / "inputs" / "A.fasta").read_bytes()
    table = {key.encode(): n for key, n in cpu_ref.count_text(data, 5, 2).items()}
    keys = sorted(table)[::7] + [b"NNNNN", b"acgta"]
    panel = tmp_path / "panel.txt"
    panel.write_bytes(b"k-mer\tA_Count\n" + b"\n".join(keys))  # (a header, and no line end behind the last key)
    out = tmp_path / "out"
    assert cli.main(["-i", str(GOLDEN / "inputs" / "A.fasta"), "-k", "5", "-c", "2", "-skipclean", "-query", str(panel), "-o", str(out)]) == 0
    assert (out / "query_Nucleotide.tsv").read_bytes() == _query_table(["A"], {"A": table}, keys)
    # the same table through the report layer, by hand
    with native.Counter(5, NT) as ctx:
        ctx.count_chunk(data, 2)
        assert report.write_query_tsv({"A": ctx}, panel, tmp_path / "again.tsv") == len(keys)
    assert (tmp_path / "again.tsv").read_bytes() == (out / "query_Nucleotide.tsv").read_bytes()
