"""Paired reads filtered, trimmed and normalised with the pair as the unit (mk_pairs_text / mk_pairs_device,
Counter.pairs*, kmers.*_reads(paired=...)).  The oracle never is the code under test: every mate's own result comes from
the UNPAIRED call on the same text (Counter.filter / trim / normalize: keep, kept, median, rows), the pair rule is restated
here in plain Python, and the bytes of a record are cut from the text by tests/norm_rule.py and tests/trim_rule.py.  The
tables are counted from the tests' own texts.  Equality is exact everywhere."""
import ctypes
import functools
import random

import numpy as np
import pytest

import norm_rule
import trim_rule
from mercat2_amd import kmers, native

pytestmark = pytest.mark.gpu
NT = native.ALPHABET_NT2
ARG, RANGE = -1, -7
FILTER, TRIM, NORM = native.PAIRS_FILTER, native.PAIRS_TRIM, native.PAIRS_NORM
KINDS = "GHBST"  # good (count 5), high (count 40), bad (absent), short (fewer than k characters), trimmed in the middle
LETTERS = {"G": "AC", "H": "AG", "B": "GT"}
FILTER_RULE = dict(at_least=2, min_hits=1, min_ppm=1_000_000)  # every k-mer occurs at least twice
TRIM_RULE = dict(at_least=2, min_len=0)
NORM_RULE = dict(target=8, min_depth=3, seed=7)


def seq_of(rng, kind: str, k: int, n: int) -> str:
    if kind == "S":
        return "".join(rng.choice("ACGT") for _ in range(rng.randrange(0, k)))
    if kind == "T":  # the first 60 % as a good read's, the rest as a bad one's
        cut = max(k + 2, (6 * n) // 10)
        return "".join(rng.choice("AC") for _ in range(cut)) + "".join(rng.choice("GT") for _ in range(n - cut))
    return "".join(rng.choice(LETTERS[kind]) for _ in range(n))


def dress(i: int, name: str, seq: str) -> str:
    """One record: the line ends, the wrapping and the blanks in front of '>' change from pair to pair."""
    nl = ("\n", "\r\n", "\r")[(i // 2) % 3]
    width = (0, 20, 33)[(i // 6) % 3]
    lines = [seq[j:j + width] for j in range(0, len(seq), width)] if width and seq else [seq]
    return ("  " if i % 5 == 3 else "") + ">" + name + nl + nl.join(lines) + nl


@functools.lru_cache(maxsize=None)
def pairs_case(k: int, headless: bool = False):
    """(interleaved text, source text to count the table from): every ordered combination of the five kinds as a pair,
    twice, in changing dress; optionally a headless good read as the first mate; the last record without a line end."""
    rng = random.Random(100 * k + headless)
    recs, source = [], []
    combos = [(a, b) for a in KINDS for b in KINDS] * 2
    rng.shuffle(combos)
    for p, combo in enumerate(combos):
        for m, kind in enumerate(combo):
            seq = seq_of(rng, kind, k, rng.randrange(k + 20, k + 90))
            recs.append((kind, "p%d/%d %s" % (p, m + 1, kind), seq))
            if kind in "GH":
                source += [seq] * (5 if kind == "G" else 40)
            if kind == "T":
                source += [seq[:max(k + 2, (6 * len(seq)) // 10)]] * 5
    text = "".join(dress(i, name, seq) for i, (_, name, seq) in enumerate(recs))
    if headless:
        text = recs[0][2] + "\n" + text[len(dress(0, recs[0][1], recs[0][2])):]
    text = text.rstrip("\r\n")
    return text.encode(), "".join(">s\n%s\n" % s for s in source).encode()


def opened(k: int, source: bytes, canonical: bool = False):
    ctx = native.Counter(k, NT, canonical=canonical)
    ctx.count_chunk(source, 1)
    return ctx


def oracle(ctx, text: bytes, op: int, both=False, invert=False, fold=None, **rule):
    """{"out", "singles", "keep", "own", "rows", "passed"} from the unpaired call and the pair rule."""
    k = ctx.k
    raws = [raw for raw, _ in norm_rule.records(text)]
    if op == FILTER:
        _, matched, rows = ctx.filter(text, rule["at_least"], rule["min_hits"], rule["min_ppm"], fold=fold)
        own, extra, emitted = matched.tolist(), None, raws
        passed = [(a and b) if both else (a or b) for a, b in zip(own[0::2], own[1::2])]
    elif op == TRIM:
        _, kept, rows = ctx.trim(text, rule["at_least"], rule["min_len"], fold=fold)
        own, extra = (kept > 0).tolist(), kept
        emitted = [header + seq[:int(n)] + b"\n" for (header, seq), n in zip(trim_rule.records(text), kept)]
        passed = [a and b for a, b in zip(own[0::2], own[1::2])]
    else:
        _, _, med, rows = ctx.normalize(text, rule["target"], rule["min_depth"], rule["seed"], fold=fold)
        extra, emitted, passed = med, raws, []
        for p in range(len(raws) // 2):
            depths = [int(med[r]) for r in (2 * p, 2 * p + 1) if rows[r, 0] > 0 and med[r] >= rule["min_depth"]]
            d = min(depths) if depths else None
            passed.append(d is not None and (d <= rule["target"] or norm_rule.u_of(rule["seed"], 2 * p) * d < rule["target"] << 32))
        own = [x for x in passed for _ in (0, 1)]
    assert len(raws) == len(own) == len(emitted) == rows.shape[0] and len(raws) % 2 == 0
    keep = []
    for r, o in enumerate(own):
        emit = passed[r // 2] != invert
        keep.append(1 if emit else 2 if (o and not passed[r // 2] and not invert) else 0)
    return {"out": b"".join(e for e, kp in zip(emitted, keep) if kp == 1), "singles": b"".join(e for e, kp in zip(emitted, keep) if kp == 2),
            "keep": keep, "own": extra, "rows": rows, "passed": passed, "own_flags": own}


def check(ctx, text: bytes, op: int, both=False, invert=False, singles=True, fold=None, piece_bytes=0, want=None, **rule):
    """Counter.pairs against the oracle: out, singles, keep, own (kept / median), rows and the figures."""
    want = want or oracle(ctx, text, op, both, invert, fold, **rule)
    info = {}
    out, sg, keep, own, rows = ctx.pairs(text, op, both=both, invert=invert, singles=singles and not invert, fold=fold,
                                         piece_bytes=piece_bytes, info=info, **rule)
    assert keep.dtype == np.uint8 and keep.tolist() == want["keep"]
    assert out == want["out"]
    assert rows.tolist() == want["rows"].tolist()
    if op == FILTER:
        assert own is None
    else:
        assert own.dtype == (np.uint64 if op == TRIM else np.uint32) and own.tolist() == want["own"].tolist()
    if singles and not invert:
        assert sg == want["singles"]
    else:
        assert sg is None
    emitted = [raw for raw, _ in norm_rule.records(out)]
    assert len(emitted) % 2 == 0 and len(emitted) == want["keep"].count(1) == info["records_out"] == 2 * info["pairs_out"]
    assert info["records"] == len(want["keep"]) == 2 * info["pairs"] and info["bytes"] == len(text)
    assert info["bytes_out"] == len(out) and info["bytes_singles"] == len(want["singles"]) and info["singles_out"] == want["keep"].count(2)
    assert info["preamble"] == norm_rule.preamble(text)
    screen = {}
    ctx.screen(text, rule.get("at_least", max(rule.get("min_depth", 0), 1)), fold=fold, info=screen)
    for name in ("records", "windows", "hits", "packed_windows", "text_windows", "folded", "bytes", "headless"):
        assert info[name] == screen[name], name
    return (out, sg, keep, own, rows), info, want


def combos_of(want):
    return {(a, b) for a, b in zip(want["own_flags"][0::2], want["own_flags"][1::2])}


# --------------------------------------------------------------------------------------------- the three ops
@pytest.mark.parametrize("headless", [False, True], ids=["headers", "headless"])
@pytest.mark.parametrize("k", [5, 31])
def test_filter_pairs(k, headless):
    text, source = pairs_case(k, headless)
    with opened(k, source) as ctx:
        _, info, want = check(ctx, text, FILTER, **FILTER_RULE)
        assert combos_of(want) == {(False, False), (False, True), (True, False), (True, True)}
        assert info["headless"] == (1 if headless else 0) and 0 < info["pairs_out"] < info["pairs"] and info["singles_out"] == 0
        _, info_b, want_b = check(ctx, text, FILTER, both=True, **FILTER_RULE)
        # (a pair that passes under "either" alone has exactly one matching mate: the orphan under "both")
        assert 0 < info_b["pairs_out"] < info["pairs_out"] and info_b["singles_out"] == info["pairs_out"] - info_b["pairs_out"]
        (out_i, _, keep_i, _, _), info_i, _ = check(ctx, text, FILTER, invert=True, **FILTER_RULE)
        assert info_i["pairs_out"] + info["pairs_out"] == info["pairs"]
        assert len(out_i) + info["bytes_out"] + info["preamble"] == len(text)  # the two outputs partition the records
        check(ctx, text, FILTER, both=True, invert=True, **FILTER_RULE)
        check(ctx, text, FILTER, both=True, singles=False, **FILTER_RULE)  # the orphans are only counted
        check(ctx, text, FILTER, at_least=1, min_hits=3, min_ppm=0)


@pytest.mark.parametrize("headless", [False, True], ids=["headers", "headless"])
@pytest.mark.parametrize("k", [5, 31])
def test_trim_pairs(k, headless):
    text, source = pairs_case(k, headless)
    with opened(k, source) as ctx:
        (out, sg, keep, kept, rows), info, want = check(ctx, text, TRIM, **TRIM_RULE)
        assert combos_of(want) == {(False, False), (False, True), (True, False), (True, True)}
        assert 0 < info["pairs_out"] < info["pairs"] and info["singles_out"] > 0
        # the mates keep their own lengths: some emitted pairs hold a trimmed mate beside an untrimmed one
        full = rows[:, 0] + (k - 1)
        assert any(keep[r] == 1 and 0 < kept[r] < full[r] and kept[r ^ 1] == full[r ^ 1] for r in range(len(keep)))
        # kept is the mate's own figure whatever became of the pair: an orphan has one; a mate whose first window is low
        # keeps nothing
        assert any(keep[r] == 2 and kept[r] > 0 and kept[r ^ 1] == 0 for r in range(len(keep)))
        assert any(kept[r] == 0 and rows[r, 0] > 0 for r in range(len(keep)))
        unpaired = {}
        ctx.trim(text, info=unpaired, **TRIM_RULE)
        for name in ("records_trimmed", "records_dropped", "bases_in", "bases_out"):
            assert info[name] == unpaired[name], name
        check(ctx, text, TRIM, singles=False, **TRIM_RULE)
        check(ctx, text, TRIM, at_least=2, min_len=k + 30)


@pytest.mark.parametrize("headless", [False, True], ids=["headers", "headless"])
@pytest.mark.parametrize("k", [5, 31])
def test_normalize_pairs(k, headless):
    text, source = pairs_case(k, headless)
    # (at k = 5 the reads share their few k-mers: a good read's depth is in the hundreds, a high one's above a thousand)
    rule = NORM_RULE if k > 5 else dict(target=400, min_depth=3, seed=7)
    target, min_depth = rule["target"], rule["min_depth"]
    with opened(k, source) as ctx:
        (_, sg, keep, med, rows), info, want = check(ctx, text, NORM, **rule)
        assert sg == b"" and info["singles_out"] == 0 and 2 not in keep.tolist()
        assert 0 < info["pairs_out"] < info["pairs"]
        # every class of mate occurs: short, low, within the target, above it
        eligible = [(rows[r, 0] > 0 and med[r] >= min_depth) for r in range(len(keep))]
        assert {(a, b) for a, b in zip(eligible[0::2], eligible[1::2])} == {(False, False), (False, True), (True, False), (True, True)}
        assert info["records_short"] > 0 and info["records_low"] > 0 and info["records_over"] > 0
        unpaired = {}
        ctx.normalize(text, info=unpaired, **rule)
        for name in ("records_short", "records_low", "records_over"):
            assert info[name] == unpaired[name], name
        # a deep mate beside a shallow eligible one passes without a draw; beside a short or low one it is drawn for
        deep = [r for r in range(len(keep)) if eligible[r] and med[r] > target]
        assert any(not eligible[r ^ 1] for r in deep)
        assert any(eligible[r ^ 1] and med[r ^ 1] <= target and keep[r] == 1 for r in deep)
        _, info_i, _ = check(ctx, text, NORM, invert=True, **rule)
        assert info_i["pairs_out"] + info["pairs_out"] == info["pairs"] and info_i["records_thinned"] == info["records_thinned"]
        check(ctx, text, NORM, target=target, min_depth=0, seed=1)  # khmer's -p: either mate at or under the cutoff keeps the pair


# ------------------------------------------------------------------------------------------------- the draw
def test_the_draw_is_the_first_mates():
    k, depth, target, seed, npairs = 31, 80, 20, 11, 96
    rng = random.Random(4)
    reads = [seq_of(rng, "G", k, 70) for _ in range(2 * npairs)]
    text = "".join(">d%d\n%s\n" % (i, r) for i, r in enumerate(reads)).encode()
    source = "".join(">s\n%s\n" % r for r in reads for _ in range(depth)).encode()
    rule = [norm_rule.u_of(seed, 2 * p) * depth < target << 32 for p in range(npairs)]
    assert 10 <= sum(rule) <= 40  # (Binomial(96, 1 / 4): the case keeps some and tosses some)
    assert rule != [norm_rule.u_of(seed, 2 * p + 1) * depth < target << 32 for p in range(npairs)]
    assert rule != [norm_rule.u_of(seed, p) * depth < target << 32 for p in range(npairs)]
    with opened(k, source) as ctx:
        (out, _, keep, med, _), info, want = check(ctx, text, NORM, target=target, min_depth=0, seed=seed)
        assert set(med.tolist()) == {depth} and want["passed"] == rule and keep.tolist() == [int(x) for x in rule for _ in (0, 1)]
        assert info["records_over"] == 2 * npairs and info["records_thinned"] == 2 * (npairs - sum(rule))
        again, _, _ = check(ctx, text, NORM, target=target, min_depth=0, seed=seed, piece_bytes=64)
        assert again[0] == out and again[2].tolist() == keep.tolist()
        other, _, _ = check(ctx, text, NORM, target=target, min_depth=0, seed=seed + 1)
        assert other[2].tolist() != keep.tolist()


# --------------------------------------------------------------------------------------------------- pieces
@functools.lru_cache(maxsize=None)
def pieces_case(k: int):
    """pairs_case and, in front of it, pairs of which a mate is longer than the smallest piece: as a first mate (a piece of
    one record, which has to grow) and as a second."""
    text, source = pairs_case(k)
    rng = random.Random(9)
    long_a, long_b = seq_of(rng, "G", k, 700), seq_of(rng, "T", k, 500)
    head = ">long/1\n%s\n>long/2\n%s\n>m/1\n%s\n>m/2\n%s\n" % (long_a, seq_of(rng, "G", k, 40), seq_of(rng, "B", k, 50), long_b)
    return head.encode() + text, source + (">s\n%s\n" % long_a).encode() * 5 + (">s\n%s\n" % long_b[:300]).encode() * 5


@pytest.mark.parametrize("op,rule", [(FILTER, FILTER_RULE), (TRIM, TRIM_RULE), (NORM, NORM_RULE)], ids=["filter", "trim", "norm"])
def test_nothing_depends_on_piece_bytes(op, rule):
    k = 31
    text, source = pieces_case(k)
    n_records = len(norm_rule.records(text))
    with opened(k, source) as ctx:
        one, info, want = check(ctx, text, op, both=op == FILTER, **rule)
        assert info["pieces"] == 1
        pieces = {}
        for piece_bytes in (64, 200, 1000, len(text) - 30, len(text) + 1):
            got, info_p, _ = check(ctx, text, op, both=op == FILTER, piece_bytes=piece_bytes, want=want, **rule)
            assert got[0] == one[0] and got[1] == one[1]
            pieces[piece_bytes] = info_p["pieces"]
            for name in ("pairs_out", "singles_out", "records_trimmed", "records_dropped", "bases_in", "bases_out",
                         "records_short", "records_low", "records_over", "records_thinned"):
                assert info_p[name] == info[name], name
        # the smallest piece holds about one record: many natural cuts fall between mates
        assert pieces[64] > n_records // 8 and pieces[200] > 1 and pieces[len(text) + 1] == 1
        # the cuts the unpaired call makes at that size do fall between mates (or the case shows nothing)
        ends = np.cumsum([len(raw) for raw, _ in norm_rule.records(text)]).tolist()
        cuts, at = [], 0
        for r, end in enumerate(ends):
            if end - at >= 2 * (k + 24):
                cuts.append(r + 1)
                at = end
        assert any(c % 2 for c in cuts)


# ------------------------------------------------------------------------------------- fold, two-word keys
def test_canonical_context():
    k = 31
    text, source = pairs_case(k)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    flipped = b"".join(header + (seq.translate(comp)[::-1] if r % 3 == 0 else seq) + b"\n"
                       for r, (header, seq) in enumerate(trim_rule.records(text + b"\n")))
    with opened(k, source, canonical=True) as ctx:
        _, info, want = check(ctx, flipped, TRIM, **TRIM_RULE)  # fold=None: as the context counts
        assert info["folded"] > 0 and 0 < info["pairs_out"] < info["pairs"]
        _, _, plain = check(ctx, flipped, TRIM, fold=False, **TRIM_RULE)
        assert plain["keep"] != want["keep"]
        check(ctx, flipped, FILTER, both=True, **FILTER_RULE)
        check(ctx, flipped, NORM, **NORM_RULE)


def test_two_word_keys():
    k = 33
    text, source = pairs_case(k)
    with opened(k, source) as ctx:
        for op, rule in ((FILTER, FILTER_RULE), (TRIM, TRIM_RULE), (NORM, NORM_RULE)):
            _, info, _ = check(ctx, text, op, **rule)
            assert 0 < info["pairs_out"] < info["pairs"]
            check(ctx, text, op, piece_bytes=64, **rule)


# --------------------------------------------------------------------------------------------------- errors
def raw_call(ctx, text: bytes, op=TRIM, flags=0, out_cap=None, sg_cap=None, cap=None, null_rule=False, piece_bytes=0,
             with_singles=True, rule=None):
    """mk_pairs_text into 0xA5-guarded buffers one element longer than the capacities it is told."""
    n_rec = text.count(b">") + 1
    out_cap = len(text) + 1 if out_cap is None else out_cap
    sg_cap = len(text) + 1 if sg_cap is None else sg_cap
    cap = n_rec if cap is None else cap
    held = np.frombuffer(text, dtype=np.uint8)
    out = np.full(out_cap + 1, 0xA5, dtype=np.uint8)
    sg = np.full(sg_cap + 1, 0xA5, dtype=np.uint8)
    keep = np.full(cap + 1, 0xA5, dtype=np.uint8)
    kept = np.full(cap + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    med = np.full(cap + 1, 0xA5A5A5A5, dtype=np.uint32)
    rows = np.full((cap + 1, 5), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    r = rule or native.PairsRule(op, 0, native.FilterRule(2, 1, 1_000_000, 0), native.TrimRule(2, 0), native.NormRule(8, 3, 7))
    n, out_len, sg_len, st = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), native.Pairs()
    rc = ctx._L.mk_pairs_text(ctx._h, held.ctypes.data if len(text) else None, len(text), piece_bytes, flags,
                              None if null_rule else ctypes.byref(r), out.ctypes.data, out_cap, ctypes.byref(out_len),
                              sg.ctypes.data if with_singles else None, sg_cap if with_singles else 0, ctypes.byref(sg_len),
                              keep.ctypes.data, kept.ctypes.data, med.ctypes.data, rows.ctypes.data, cap, ctypes.byref(n), ctypes.byref(st))
    return {"rc": rc, "out": out, "singles": sg, "keep": keep, "kept": kept, "median": med, "rows": rows, "nrows": n.value,
            "out_len": out_len.value, "singles_len": sg_len.value, "error": ctx._L.mk_last_error(ctx._h).decode()}


def test_errors():
    k = 31
    text, source = pairs_case(k)
    odd = text[:text.rindex(b">")]
    n_odd = len(norm_rule.records(odd))
    assert n_odd % 2 == 1
    with opened(k, source) as ctx:
        for piece_bytes in (0, 64):
            got = raw_call(ctx, odd, piece_bytes=piece_bytes)
            assert got["rc"] == RANGE and str(n_odd) in got["error"] and "odd" in got["error"]
            assert (got["out_len"], got["singles_len"], got["nrows"]) == (0, 0, n_odd)
        got = raw_call(ctx, b">only\n" + b"AC" * 40 + b"\n")
        assert got["rc"] == RANGE and "1 records" in got["error"]
        for flags, op, word in ((native.PAIRS_INVERT, TRIM, "INVERT"), (native.PAIRS_BOTH, TRIM, "BOTH"), (native.PAIRS_BOTH, NORM, "BOTH"),
                                (native.PAIRS_INVERT, FILTER, "singles"), (8, FILTER, "flag"), (16, TRIM, "flag"), (1 << 31, NORM, "flag"),
                                (0, 3, "op"), (0, -1, "op")):
            got = raw_call(ctx, text, op=op, flags=flags)
            assert got["rc"] == ARG and word in got["error"], (flags, op)
            assert (got["out"] == 0xA5).all() and (got["keep"] == 0xA5).all()
        assert raw_call(ctx, text, op=FILTER, flags=native.PAIRS_INVERT, with_singles=False)["rc"] == 0
        got = raw_call(ctx, text, null_rule=True)
        assert got["rc"] == ARG and "rule" in got["error"]
        for rule, word in ((native.PairsRule(FILTER, 0, native.FilterRule(1, 0, 0, 0)), "min_hits"),
                           (native.PairsRule(TRIM, 0, native.FilterRule(1, 1, 0, 0), native.TrimRule(0, 0)), "at_least"),
                           (native.PairsRule(NORM, 0, native.FilterRule(1, 1, 0, 0), native.TrimRule(1, 0), native.NormRule(0, 0, 0)), "target")):
            got = raw_call(ctx, text, rule=rule)
            assert got["rc"] == ARG and word in got["error"]
        with pytest.raises(native.MercatHipError) as e:
            ctx.pairs(odd, "trim")
        assert e.value.code == RANGE
        with pytest.raises(ValueError):
            ctx.pairs(text, "sort")
        # no record: success with empty outputs
        for empty in (b"", b"\n  \n"):
            out, sg, keep, kept, rows = ctx.pairs(empty, "trim", singles=True)
            assert (out, sg, keep.tolist(), kept.tolist(), rows.shape) == (b"", b"", [], [], (0, 5))


@pytest.mark.parametrize("piece_bytes", [0, 64])
def test_capacities(piece_bytes):
    k = 31
    text, source = pairs_case(k)
    with opened(k, source) as ctx:
        want = oracle(ctx, text, TRIM, **TRIM_RULE)
        no, ns, nr = len(want["out"]), len(want["singles"]), len(want["keep"])
        assert no > 16 and ns > 16
        full = raw_call(ctx, text, out_cap=no, sg_cap=ns, cap=nr, piece_bytes=piece_bytes)
        assert full["rc"] == 0 and (full["out_len"], full["singles_len"], full["nrows"]) == (no, ns, nr)
        assert full["out"][:no].tobytes() == want["out"] and full["out"][no] == 0xA5
        assert full["singles"][:ns].tobytes() == want["singles"] and full["singles"][ns] == 0xA5
        assert full["keep"][:nr].tolist() == want["keep"] and full["keep"][nr] == 0xA5
        assert full["kept"][:nr].tolist() == want["own"].tolist() and full["kept"][nr] == 0xA5A5A5A5A5A5A5A5
        assert full["rows"][:nr].tolist() == want["rows"].tolist() and (full["rows"][nr] == 0xA5A5A5A5A5A5A5A5).all()
        assert (full["median"] == 0xA5A5A5A5).all()  # (ignored by TRIM)
        for short in ("out", "singles", "rows", "all"):
            oc, sc, cp = no - (short in ("out", "all")), ns - (short in ("singles", "all")), nr - (short in ("rows", "all"))
            got = raw_call(ctx, text, out_cap=oc, sg_cap=sc, cap=cp, piece_bytes=piece_bytes)
            assert got["rc"] == RANGE, short
            assert (got["out_len"], got["singles_len"], got["nrows"]) == (no, ns, nr), short  # the exact needed sizes
            assert got["out"][oc] == 0xA5 and got["singles"][sc] == 0xA5 and got["keep"][cp] == 0xA5
            assert got["kept"][cp] == 0xA5A5A5A5A5A5A5A5 and (got["rows"][cp] == 0xA5A5A5A5A5A5A5A5).all()
        sizing = raw_call(ctx, text, out_cap=0, sg_cap=0, cap=0, piece_bytes=piece_bytes)
        assert sizing["rc"] == RANGE and (sizing["out_len"], sizing["singles_len"], sizing["nrows"]) == (no, ns, nr)


# ---------------------------------------------------------------------------------------------- device call
@pytest.mark.parametrize("op,rule", [(FILTER, FILTER_RULE), (TRIM, TRIM_RULE), (NORM, NORM_RULE)], ids=["filter", "trim", "norm"])
def test_pairs_device_agrees(op, rule):
    import torch
    k = 31
    text, source = pairs_case(k)
    lead, out_lead = 3, 5  # the text and the outputs at odd addresses
    with opened(k, source) as ctx:
        (w_out, w_sg, w_keep, w_own, w_rows), _, _ = check(ctx, text, op, both=op == FILTER, **rule)
        no, ns, nr = len(w_out), len(w_sg), len(w_keep)
        d_text = torch.from_numpy(np.frombuffer(b"#" * lead + text, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((out_lead + no + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_sg = torch.full((out_lead + ns + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_keep = torch.full((nr + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        d_kept = torch.full((nr + 1,), -1, dtype=torch.int64, device="cuda")
        d_med = torch.full((nr + 1,), -1, dtype=torch.int32, device="cuda")
        d_rows = torch.full((nr + 1, 5), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        info = ctx.pairs_device(d_text.data_ptr() + lead, len(text), op, d_out.data_ptr() + out_lead, no, d_sg.data_ptr() + out_lead, ns,
                                d_keep.data_ptr(), d_kept.data_ptr(), d_med.data_ptr(), d_rows.data_ptr(), nr, both=op == FILTER, **rule)
        assert (info["bytes_out"], info["bytes_singles"], info["records"], info["pieces"]) == (no, ns, nr, 1)
        got, got_sg = d_out.cpu().numpy(), d_sg.cpu().numpy()
        assert got[out_lead:out_lead + no].tobytes() == w_out and (got[:out_lead] == 0xA5).all() and (got[out_lead + no:] == 0xA5).all()
        assert got_sg[out_lead:out_lead + ns].tobytes() == w_sg and (got_sg[:out_lead] == 0xA5).all() and (got_sg[out_lead + ns:] == 0xA5).all()
        assert d_keep.cpu().numpy()[:nr].tolist() == w_keep.tolist() and int(d_keep[nr]) == 0xA5
        assert d_rows.cpu().numpy().view(np.uint64)[:nr].tolist() == w_rows.tolist() and (d_rows[nr] == -1).all().item()
        if op == TRIM:
            assert d_kept.cpu().numpy().view(np.uint64)[:nr].tolist() == w_own.tolist() and int(d_kept[nr]) == -1
        if op == NORM:
            assert d_med.cpu().numpy().view(np.uint32)[:nr].tolist() == w_own.tolist() and int(d_med[nr]) == -1
        odd_end = text.rindex(b">")
        with pytest.raises(native.MercatHipError) as e:  # one piece: an odd count is refused
            ctx.pairs_device(d_text.data_ptr() + lead, odd_end, op, d_out.data_ptr(), no, **rule)
        assert e.value.code == RANGE and "odd" in str(e.value)
        with pytest.raises(native.MercatHipError) as e:
            ctx.pairs_device(d_text.data_ptr() + lead, len(text), op, d_out.data_ptr(), no - 1, **rule)
        assert e.value.code == RANGE
        with pytest.raises(native.MercatHipError) as e:
            ctx.pairs_device(d_text.data_ptr() + lead, len(text), op, d_out.data_ptr(), no, kept_ptr=d_kept.data_ptr() + 4, cap=nr, **rule)
        assert e.value.code == ARG


# ------------------------------------------------------------------------------------------------ two files
def test_two_files(tmp_path, inputs_dir):
    """tests/golden/inputs/D_paired_1.fasta and D_paired_2.fasta.  The two files hold 93 and 53 records: as they stand
    they are no pairs and are refused with both counts; the first 53 records of the first file are the mates of the
    second file's by position, which is all that defines a pair."""
    k = 11
    one, two = (inputs_dir / "D_paired_1.fasta").read_bytes(), (inputs_dir / "D_paired_2.fasta").read_bytes()
    recs1, recs2 = [raw for raw, _ in norm_rule.records(one)], [raw for raw, _ in norm_rule.records(two)]
    assert (len(recs1), len(recs2)) == (93, 53)
    source = b"".join(raw[:len(raw) * 2 // 3] + b"\n" for raw in recs1[0::2] + recs2[1::3])  # most reads lose their end, some all
    with opened(k, source) as ctx:
        with pytest.raises(native.MercatHipError) as e:
            kmers.trim_reads(ctx, inputs_dir / "D_paired_1.fasta", tmp_path / "x_1.fa", mate_file=inputs_dir / "D_paired_2.fasta",
                             out_path2=tmp_path / "x_2.fa")
        assert e.value.code == RANGE and "93" in str(e.value) and "53" in str(e.value)
        (tmp_path / "r1.fasta").write_bytes(b"".join(recs1[:53]))
        both = b"".join(a + b for a, b in zip(recs1[:53], recs2))
        assert native.interleave(b"".join(recs1[:53]), two) == both
        want = oracle(ctx, both, TRIM, at_least=1, min_len=0)
        assert 0 < want["keep"].count(1) < 106 and want["keep"].count(2) > 0
        res = kmers.trim_reads(ctx, tmp_path / "r1.fasta", tmp_path / "out_1.fa", at_least=1, mate_file=inputs_dir / "D_paired_2.fasta",
                               out_path2=tmp_path / "out_2.fa", singles_path=tmp_path / "singles.fa.gz", tsv_path=tmp_path / "trim.tsv")
        out1, out2 = (tmp_path / "out_1.fa").read_bytes(), (tmp_path / "out_2.fa").read_bytes()
        e1, e2 = trim_rule.records(out1), trim_rule.records(out2)
        emitted = trim_rule.records(want["out"])
        assert len(e1) == len(e2) == want["keep"].count(1) // 2 and e1 == emitted[0::2] and e2 == emitted[1::2]
        # the same pairs in the same order: the headers left are those of the mates by position
        heads1, heads2 = [r.split(b"\n")[0] for r in recs1[:53]], [r.split(b"\n")[0] for r in recs2]
        passed = [p for p in range(53) if want["passed"][p]]
        assert [h.rstrip(b"\n") for h, _ in e1] == [heads1[p] for p in passed] and [h.rstrip(b"\n") for h, _ in e2] == [heads2[p] for p in passed]
        assert native.interleave(out1, out2) == want["out"]
        import gzip
        assert gzip.open(tmp_path / "singles.fa.gz", "rb").read() == want["singles"]
        assert (res["records"], res["pairs"], res["pairs_kept"], res["singles"]) == (106, 53, len(e1), want["keep"].count(2))
        lines = (tmp_path / "trim.tsv").read_bytes().split(b"\n")
        assert lines[0] == b"record\tlength\tkept\temitted\tpair" and len(lines) == 108
        assert [ln.split(b"\t")[3] for ln in lines[1:-1]] == [(b"0", b"pair", b"single")[x] for x in want["keep"]]
        # interleaved in, interleaved out
        (tmp_path / "both.fa").write_bytes(both)
        res_i = kmers.trim_reads(ctx, tmp_path / "both.fa", tmp_path / "both_out.fa", at_least=1, paired=True)
        assert (tmp_path / "both_out.fa").read_bytes() == want["out"] and res_i["pairs_kept"] == res["pairs_kept"]
        with pytest.raises(ValueError):
            kmers.trim_reads(ctx, tmp_path / "both.fa", tmp_path / "z.fa", out_path2=tmp_path / "z2.fa")


# ---------------------------------------------------------------------------------------------- side effects
def test_the_context_is_left_as_it_was():
    k = 31
    text, source = pairs_case(k)
    with opened(k, source) as ctx:
        before, size, stats = ctx.to_dict(), ctx.rows(), ctx.stats()
        for op, rule in ((FILTER, FILTER_RULE), (TRIM, TRIM_RULE), (NORM, NORM_RULE)):
            ctx.pairs(text, op, singles=True, piece_bytes=64, **rule)
        assert ctx.rows() == size and ctx.to_dict() == before
        after = ctx.stats()
        for name in ("kmers_total", "chunks", "bytes_in"):
            if name in stats:
                assert after[name] == stats[name], name
        assert {n: v for n, v in after.items() if isinstance(v, int)} == {n: v for n, v in stats.items() if isinstance(v, int)}


# ------------------------------------------------------------------------------------------------------ the CLI
def test_cli_paired(tmp_path):
    """-trim with two files and -singles, -filter with -paired and -filter_pair both, -norm with -paired: the files
    written are what the Counter calls give for the sample's table."""
    from mercat2_amd import cli
    k = 11
    text, source = pairs_case(k)
    text += b"\n"
    (tmp_path / "s.fna").write_bytes(source)
    (tmp_path / "both.fa").write_bytes(text)
    one, two = native.split_pairs(text)
    (tmp_path / "r1.fa").write_bytes(one)
    (tmp_path / "r2.fa").write_bytes(two)
    base = ["-i", str(tmp_path / "s.fna"), "-k", str(k), "-c", "1", "-skipclean"]
    # (-paired and a mate flag do not go together: two runs)
    assert cli.main(base + ["-o", str(tmp_path / "out1"), "-trim", str(tmp_path / "r1.fa"), "-trim_mate", str(tmp_path / "r2.fa"),
                            "-singles"]) == 0
    assert cli.main(base + ["-o", str(tmp_path / "out2"), "-paired", "-singles", "-filter", str(tmp_path / "both.fa"), "-filter_pair", "both",
                            "-filter_keep", "matched", "-filter_min", "2", "-norm", str(tmp_path / "both.fa"), "-norm_target", "8",
                            "-norm_min", "3", "-norm_seed", "7"]) == 0
    with opened(k, source) as ctx:
        trim = oracle(ctx, text, TRIM, **TRIM_RULE)
        folder = tmp_path / "out1" / "trim_nucleotide"
        assert sorted(p.name for p in folder.iterdir()) == ["s_singles.fna", "s_trim.tsv", "s_trimmed_1.fna", "s_trimmed_2.fna"]
        assert native.interleave((folder / "s_trimmed_1.fna").read_bytes(), (folder / "s_trimmed_2.fna").read_bytes()) == trim["out"]
        assert (folder / "s_singles.fna").read_bytes() == trim["singles"] != b""
        lines = (folder / "s_trim.tsv").read_bytes().split(b"\n")
        assert lines[0] == b"record\tlength\tkept\temitted\tpair" and lines[3].split(b"\t")[4] == b"1"
        filt = oracle(ctx, text, FILTER, both=True, at_least=2, min_hits=1, min_ppm=0)
        folder = tmp_path / "out2" / "filter_nucleotide"
        assert sorted(p.name for p in folder.iterdir()) == ["s_matched.fna", "s_singles.fna"]
        assert (folder / "s_matched.fna").read_bytes() == filt["out"] != b"" and (folder / "s_singles.fna").read_bytes() == filt["singles"]
        norm = oracle(ctx, text, NORM, **NORM_RULE)
        folder = tmp_path / "out2" / "norm_nucleotide"
        assert sorted(p.name for p in folder.iterdir()) == ["s_kept.fna", "s_norm.tsv", "s_singles.fna"]
        assert (folder / "s_kept.fna").read_bytes() == norm["out"] != b"" and (folder / "s_singles.fna").read_bytes() == b""
        lines = (folder / "s_norm.tsv").read_bytes().split(b"\n")
        assert lines[0] == b"record\twindows\tmedian\tkept\tpair" and [ln.split(b"\t")[3] for ln in lines[1:-1]] == [b"%d" % x for x in norm["keep"]]
        res = kmers.normalize_read_pairs(ctx, tmp_path / "r1.fa", tmp_path / "n_1.fa", 8, 3, 7, mate_file=tmp_path / "r2.fa",
                                         out_path2=tmp_path / "n_2.fa")
        assert native.interleave((tmp_path / "n_1.fa").read_bytes(), (tmp_path / "n_2.fa").read_bytes()) == norm["out"]
        assert res["pairs"] == 50 and res["pairs_kept"] == norm["keep"].count(1) // 2
