"""Two GPU tables combined by key (mk_table_op, Counter.combine, report.write_against_tsvs, -against).  The expected
table never comes from the code under test: it is setop_rule.combine -- the rule of the header over Python dicts -- of
rows parsed from committed TSVs, of the ``to_dict()`` of the input contexts, or of counts written into crafted text."""
import functools
from pathlib import Path

import numpy as np
import pytest

import setop_rule
from setop_rule import M64, OPS
from mercat2_amd import cli, native

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
NT, AA, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW
ARG, STATE = -1, -4


def _snapshot(ctx):
    keys, counts = ctx.export()
    return keys.copy(), counts.copy()


def _unchanged(ctx, snap) -> bool:
    keys, counts = ctx.export()
    return np.array_equal(keys, snap[0]) and np.array_equal(counts, snap[1])


def _check(a, b, da, db, op, min_a=1, min_b=1, into=None):
    """a.combine(b, op) against the rule over the two dicts; returns (the result context, its dict, info)."""
    info = {}
    dst = a.combine(b, op, min_a, min_b, into=into, info=info)
    try:
        assert into is None or dst is into
        want = setop_rule.combine(da, db, op, min_a, min_b)
        got = dst.to_dict()
        assert got == want, (op, min_a, min_b, len(got), len(want))
        assert dst.rows() == len(want)
        for field, value in setop_rule.figures(da, db, op, min_a, min_b, want).items():
            assert info[field] == value, (op, field, info[field], value)
        assert info["packed_out"] + info["text_out"] == info["rows_out"]
        assert info["op"] == native.OPS[op] and info["s_scan"] >= 0 and info["s_total"] >= info["s_scan"]
    except BaseException:
        if into is None:
            dst.close()
        raise
    return dst, got, info


def _all_ops(a, b, da, db, min_a=1, min_b=1):
    """Every op in both argument orders into one reused result context; the inputs are what they were after each."""
    snap_a, snap_b = _snapshot(a), _snapshot(b)
    with native.Counter(a.k, a.alphabet, canonical=a.canonical) as dst:
        for op in OPS:
            _check(a, b, da, db, op, min_a, min_b, into=dst)
            assert _unchanged(a, snap_a) and _unchanged(b, snap_b), op
            _check(b, a, db, da, op, min_b, min_a, into=dst)
            assert _unchanged(a, snap_a) and _unchanged(b, snap_b), op
    assert a.to_dict() == da and b.to_dict() == db


# ------------------------------------------------------------------------------- tables the reference made
def _table(name: str, k: int) -> dict:
    lines = (GOLDEN / "tsv" / (name + ".tsv")).read_bytes().split(b"\n")[1:]
    if lines[-1] == b"":
        lines.pop()
    assert all(line[k:k + 1] == b"\t" for line in lines)
    return {line[:k].decode("ascii"): int(line[k + 1:]) for line in lines}


# (first, second, alphabet) -> rows of each, in both, only in the first, ca > cb, min != left
PAIRS = {
    "nt_k5": ("Scaffolds_with-NNN_k5_c10", "ref_RW1_clean_k5_c10", NT, (2112, 828, 828, 1284, 1907, 623)),
    "aa_k5": ("ref_DJ_pro_k5_c10_s10", "ref_DJ_pro_k5_c10_s1", AA, (10362, 2532, 2532, 7830, 10097, 2267)),
}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_tables_the_reference_made(pair):
    first, second, alphabet, figures = PAIRS[pair]
    da, db = _table(first, 5), _table(second, 5)
    both = set(da) & set(db)
    low, left = setop_rule.combine(da, db, "min"), setop_rule.combine(da, db, "left")
    assert (len(da), len(db), len(both), len(set(da) - set(db)), sum(1 for key, c in da.items() if c > db.get(key, 0)),
            sum(1 for key in both if low[key] != left[key])) == figures
    if pair == "nt_k5":  # dense bins plus rows kept as text: every one of the 4^5 bins is a row, the other 1088 rows are text
        assert sum(1 for key in da if set(key) - set("ACGT")) == len(da) - 4 ** 5 == 1088
    with native.Counter(5, alphabet) as a, native.Counter(5, alphabet) as b:
        a.load_tsv(GOLDEN / "tsv" / (first + ".tsv"))
        b.load_tsv(GOLDEN / "tsv" / (second + ".tsv"))
        _all_ops(a, b, da, db)
        if pair == "aa_k5":
            assert any(c < 50 for c in db.values()) and any(c >= 50 for c in db.values())
            assert any(c < 20 for c in da.values()) and any(c >= 20 for c in da.values())
            _all_ops(a, b, da, db, min_b=50)
            _all_ops(a, b, da, db, min_a=20)


# ------------------------------------------------------------------------------------ every table shape
ODD = b">odd\n" + b"ACGTTGCANGGATCCATGNAacgtACGGT*CA" * 8 + b"\n"
ODD_A = b">odd_a\n" + b"GGNTTACCAnnGTCATGCAtgcaTTGACNGA" * 8 + b"\n"   # only A has it
ODD_B = b">odd_b\n" + b"CANGTTGGAccNTGACAGTCagtcNCAAGTC" * 8 + b"\n"   # only B has it: text keys b holds and a lacks
POLY_T = b">polyT\n" + b"T" * 40 + b"\n"


def _text_a() -> bytes:
    return native.synth_reads(30_000, 3, 1_500, 150, 4).tobytes() + POLY_T * 3 + ODD + ODD_A


def _text_b(poly_t: bool = True) -> bytes:
    return native.synth_reads(30_000, 3, 1_500, 150, 5).tobytes() + (POLY_T if poly_t else b"") + ODD + ODD_B


SHAPES = [("nt", NT, k) for k in (3, 21, 31, 32, 33, 63, 64, 70)] + [("aa", AA, k) for k in (3, 5, 12, 13, 25)] + [("raw", RAW, 9)]


def _is_packed(kind: str, k: int, key: str) -> bool:
    """Where a key lives is decided by the key alone (the header's rule for mk_lookup)."""
    if kind == "nt":
        return k <= 64 and not set(key) - set("ACGT")
    if kind == "aa":
        return k <= 25 and all("A" <= ch <= "Z" for ch in key)
    return False


def _three_ways(da, db, keep):
    ka, kb = {key for key in da if keep(key)}, {key for key in db if keep(key)}
    return ka & kb, ka - kb, kb - ka


@pytest.mark.parametrize("kind,alphabet,k", SHAPES, ids=["%s_k%d" % (s[0], s[2]) for s in SHAPES])
def test_every_table_shape(kind, alphabet, k):
    with native.Counter(k, alphabet) as a, native.Counter(k, alphabet) as b:
        a.count_chunk(_text_a(), 1)
        b.count_chunk(_text_b(), 1)
        da, db = a.to_dict(), b.to_dict()
        has_packed = (kind == "nt" and k <= 64) or (kind == "aa" and k <= 25)
        if has_packed:
            shared, only_a, only_b = _three_ways(da, db, lambda key: _is_packed(kind, k, key))
            if kind == "nt" and k == 3:  # every one of the 4^3 keys occurs in both texts: no packed key can be in one alone
                assert len(shared) == 4 ** 3 and not only_a and not only_b
                assert any(da[key] > db[key] for key in shared) and any(da[key] < db[key] for key in shared)
            else:
                assert shared and only_a and only_b
        assert all(_three_ways(da, db, lambda key: not _is_packed(kind, k, key)))  # every shape keeps text rows here
        _all_ops(a, b, da, db)
        if kind == "nt" and k == 32:  # the key kept beside the one-word table
            side = "T" * 32
            assert da[side] == 27 and db[side] == 9
            b.reset()
            b.count_chunk(_text_b(poly_t=False), 1)
            db = b.to_dict()
            assert side not in db
            with native.Counter(k, alphabet) as dst:
                _, only, _ = _check(a, b, da, db, "only", into=dst)
                assert only[side] == 27
                _, left, _ = _check(a, b, da, db, "left", into=dst)
                assert side not in left
            _all_ops(a, b, da, db)


# ------------------------------------------------------------------------------------ small and degenerate
def _tsv(table: dict) -> bytes:
    return "".join("%s\t%d\n" % (key, c) for key, c in table.items()).encode()


def _key(k: int, i: int) -> str:
    return "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(k))


@pytest.mark.parametrize("k", [31, 40])
def test_small_and_degenerate(k):
    x, y, z = _key(k, 5), _key(k, 77), _key(k, 1234)
    cases = [
        ({}, {x: 3}), ({x: 3}, {}), ({}, {}),
        ({x: 3}, {x: 5}), ({x: 3}, {y: 5}),
        ({x: M64}, {x: 1}),                       # sum wraps to 0: no row; max keeps 2^64 - 1
        ({x: M64, y: 2}, {x: 1, z: M64}),
        ({x: 7, y: 2}, {x: 7, y: 3}),             # diff with equal counts: no row
    ]
    for da, db in cases:
        with native.Counter(k, NT) as a, native.Counter(k, NT) as b:
            if da:
                a.load_tsv(_tsv(da))
            if db:  # (else never allocated)
                b.load_tsv(_tsv(db))
            assert a.to_dict() == da and b.to_dict() == db
            _all_ops(a, b, da, db)
    assert setop_rule.combine({x: M64}, {x: 1}, "sum") == {} and setop_rule.combine({x: M64}, {x: 1}, "max") == {x: M64}
    assert setop_rule.combine({x: 7}, {x: 7}, "diff") == {}
    da, db = {x: 3, y: 9, z: 1}, {x: 4, y: 1}
    with native.Counter(k, NT) as a, native.Counter(k, NT) as b:
        a.load_tsv(_tsv(da))
        b.load_tsv(_tsv(db))
        _all_ops(a, a, da, da)                    # a is b
        _all_ops(a, b, da, db, min_a=10)          # thresholds that empty one side
        _all_ops(a, b, da, db, min_b=5)
        _all_ops(a, b, da, db, min_a=2, min_b=2)
        _all_ops(a, b, da, db, min_a=M64, min_b=M64)


# ------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("k", [31, 63])
def test_identities(k):
    with native.Counter(k, NT) as a, native.Counter(k, NT) as b, native.Counter(k, NT) as copy:
        a.count_chunk(_text_a(), 1)
        b.count_chunk(_text_b(), 1)
        da = a.to_dict()
        copy.merge_from(a)
        copy.merge_from(b)

        def result(x, y, op):
            with x.combine(y, op) as dst:
                return dst.to_dict()
        assert result(a, b, "sum") == copy.to_dict()
        assert result(a, a, "min") == da and result(a, a, "only") == {}
        left, only = result(a, b, "left"), result(a, b, "only")
        assert left and only and not set(left) & set(only) and dict(left, **only) == da
        assert result(a, b, "min") == result(b, a, "min")
        ab, ba = result(a, b, "diff"), result(b, a, "diff")
        assert ab and ba and not set(ab) & set(ba)


# ----------------------------------------------------------------------- the result is an ordinary context
@pytest.mark.parametrize("kind,alphabet,k", [("nt", NT, 5), ("nt", NT, 31), ("nt", NT, 63), ("raw", RAW, 9)])
def test_the_result_is_an_ordinary_context(kind, alphabet, k, tmp_path):
    with native.Counter(k, alphabet) as a, native.Counter(k, alphabet) as b, native.Counter(k, alphabet) as again:
        a.count_chunk(_text_a(), 1)
        b.count_chunk(_text_b(), 1)
        da, db = a.to_dict(), b.to_dict()
        with a.combine(b, "diff") as dst:
            d = dst.to_dict()
            assert d == setop_rule.combine(da, db, "diff") and d
            counts = np.array(list(d.values()), dtype=np.uint64)
            bins = dst.histo(100)
            assert int(bins.sum()) == len(d) and (bins == np.bincount(np.minimum(counts, 101).astype(np.int64), minlength=102)).all()
            alpha = dst.alpha_stats()
            assert alpha["observed"] == len(d) and alpha["total"] == int(counts.sum())
            keys = sorted(d)[:2000] + sorted(set(db) - set(d))[:200]
            assert dst.lookup(keys).tolist() == [d.get(key, 0) for key in keys]
            read = _text_a().split(b"\n")[1].decode("ascii")
            windows = [read[i:i + k] for i in range(len(read) - k + 1)]
            got = [d.get(w, 0) for w in windows]
            row = dst.screen((">r\n%s\n" % read).encode())
            assert row.tolist() == [[len(windows), sum(1 for c in got if c), sum(got), min(got), max(got)]]
            assert dst.write_tsv(tmp_path / "d.tsv", "d") == len(d)
            again.load_tsv(tmp_path / "d.tsv")
            assert again.to_dict() == d
            dst.count_chunk(_text_b(), 1)                      # further counting into it
            more = dict(d)
            for key, c in db.items():
                more[key] = more.get(key, 0) + c
            assert dst.to_dict() == more and dst.rows() == len(more)
            assert a.combine(b, "diff", into=dst) is dst        # a second time replaces, and does not add
            assert dst.to_dict() == d and dst.rows() == len(d)


# ------------------------------------------------------------------------------------------- refusals
def _code(call) -> int:
    with pytest.raises(native.MercatHipError) as e:
        call()
    return e.value.code


def test_refusals():
    L = native.lib()
    x = _key(31, 9)
    with native.Counter(31, NT) as a, native.Counter(31, NT) as b, native.Counter(31, NT) as dst:
        a.load_tsv(_tsv({x: 3}))
        b.load_tsv(_tsv({x: 5}))
        assert _code(lambda: a.combine(b, "min", into=a)) == ARG
        assert _code(lambda: a.combine(b, "min", into=b)) == ARG
        for other in (native.Counter(30, NT), native.Counter(31, RAW), native.Counter(31, NT, canonical=True)):
            with other:
                assert _code(lambda: a.combine(b, "min", into=other)) == ARG
                assert _code(lambda: a.combine(other, "min", into=dst)) == ARG
        assert _code(lambda: a.combine(b, 6, into=dst)) == ARG
        assert _code(lambda: a.combine(b, -1, into=dst)) == ARG
        assert _code(lambda: a.combine(b, "min", min_other=0, into=dst)) == ARG
        assert _code(lambda: a.combine(b, "min", min_self=0, into=dst)) == ARG
        with pytest.raises(ValueError):
            a.combine(b, "xor", into=dst)
        assert L.mk_table_op(dst._h, a._h, b._h, native.OP_MIN, 1, 1, None) == 0 and dst.to_dict() == {x: 3}  # (st may be NULL)
        # an open chunk in an input
        assert L.mk_chunk_begin(b._h) == 0
        assert _code(lambda: a.combine(b, "min", into=dst)) == STATE
        assert _code(lambda: b.combine(a, "min", into=dst)) == STATE
        assert L.mk_chunk_end(b._h, 1) == 0
        # a spoiled input: a later piece of a table is refused (tests/test_gpu_tsv_load.py)
        lines = [("%s\t%d" % (_key(31, i), 1 + i % 9)).encode() for i in range(6000)]
        lines.insert(5500, _key(31, 1).encode() + b"\t5x")
        with native.Counter(31, NT) as bad:
            with pytest.raises(native.MercatHipError):
                bad.load_tsv(b"\n".join(lines) + b"\n", piece_bytes=8192)
            assert _code(bad.rows) == STATE
            assert _code(lambda: a.combine(bad, "min", into=dst)) == STATE
            assert _code(lambda: bad.combine(a, "min", into=dst)) == STATE
        # a dst that shares, or lends, a table
        with native.Counter(31, NT) as sharer:
            sharer.share_table(dst)
            assert _code(lambda: a.combine(b, "min", into=dst)) == STATE
            assert _code(lambda: a.combine(b, "min", into=sharer)) == STATE
            sharer.share_table(None)
        assert a.combine(b, "max", into=dst).to_dict() == {x: 5}
        assert a.to_dict() == {x: 3} and b.to_dict() == {x: 5}


# -------------------------------------------------------------------------------------------------- CLI
def test_cli_against(tmp_path):
    folder, out, again = tmp_path / "in", tmp_path / "out", tmp_path / "again"
    (folder / "tsv_nucleotide").mkdir(parents=True)
    samples = {"s1": _table("Scaffolds_with-NNN_k5_c10", 5), "s2": _table("ref_Test_R1_k5_c10", 5),
               "s3": _table("ref_RW1_clean_k5_c10", 5)}
    background = samples["s3"]
    for name, table in samples.items():
        (folder / "tsv_nucleotide" / (name + "_counts.tsv")).write_bytes(("k-mer\t%s_Count\n" % name).encode() + _tsv(table))
    bg = GOLDEN / "tsv" / "ref_RW1_clean_k5_c10.tsv"
    assert cli.main(["-tsv", str(folder), "-k", "5", "-against", str(bg), "-op", "only", "-o", str(out)]) == 0
    wrote = out / "against" / "tsv_nucleotide"
    for name, table in samples.items():
        want = setop_rule.combine(table, background, "only")
        path = wrote / (name + "_counts.tsv")
        if not want:  # (an empty result writes no file: s3 against itself, and s2, whose k-mers the background all holds)
            assert name in ("s2", "s3") and not path.exists()
            continue
        assert name == "s1"
        lines = path.read_bytes().split(b"\n")
        assert lines[0] == ("k-mer\t%s_Count" % name).encode() and lines[-1] == b""
        assert {l[:5].decode(): int(l[6:]) for l in lines[1:-1]} == want
    assert cli.main(["-tsv", str(out / "against"), "-k", "5", "-o", str(again)]) == 0
    assert (again / "tsv_nucleotide" / "s1_counts.tsv").read_bytes() == (wrote / "s1_counts.tsv").read_bytes()
    assert sorted(p.name for p in (again / "tsv_nucleotide").iterdir()) == ["s1_counts.tsv"]
