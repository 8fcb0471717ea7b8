"""mk_lookup and mk_screen probe the tables alike (the step of LkStep, mk_tableview.h): a key asked for as a key and the
same key screened as a FASTA record of exactly k symbols -- one window -- give the same count, and that count is what
the exported table says.  The expected values come from ``to_dict()`` alone (the export path: neither kernel under test),
through plain Python; the shapes are the smallest that reach every branch of the step."""
import functools
import random

import pytest

from mercat2_amd import native

pytestmark = pytest.mark.gpu
NT, AA = native.ALPHABET_NT2, native.ALPHABET_AA5
COMP = str.maketrans("ACGT", "TGCA")
AMINO = "ACDEFGHIKLMNPQRSTVWY"
LK_PER = 4  # keys a lane takes a trip (mk_tableview.h, the library as built)
SIZES = (1, 255, LK_PER * 256 + 1)  # a lane with fewer than LK_PER keys; a second stride of the grid

# name -> (alphabet, k, canonical context, fold, which keys lead the panel)
CASES = {
    "nt31_one_word": (NT, 31, False, False, "packed"),
    "nt31_canonical_fold": (NT, 31, True, True, "packed"),
    "nt31_canonical_no_fold": (NT, 31, True, False, "packed"),
    "nt31_text_keys": (NT, 31, False, False, "text"),     # a byte outside the alphabet: the by-reference table
    "nt32_side_key": (NT, 32, False, False, "side"),      # 32 x 'T' packs to all ones: kept beside the table
    "nt63_two_word": (NT, 63, False, False, "packed"),
    "nt63_canonical_fold": (NT, 63, True, True, "packed"),
    "nt63_canonical_no_fold": (NT, 63, True, False, "packed"),
    "aa5_one_word": (AA, 5, False, False, "packed"),
    "aa13_two_word": (AA, 13, False, False, "packed"),
    # dense bins start at 15 bits a key: protein k = 5 is a one-word hash table, these two are bins
    "aa3_dense_bins": (AA, 3, False, False, "packed"),
    "nt5_dense_bins": (NT, 5, False, False, "packed"),
}


def _letters(rng, alphabet, n):
    return "".join(rng.choice("ACGT" if alphabet == NT else AMINO) for _ in range(n))


def _odd(alphabet: int) -> str:
    return "N" if alphabet == NT else "1"


@functools.lru_cache(maxsize=None)
def _source(alphabet: int, k: int) -> bytes:
    """What the table is counted from: a few records, a run of T longer than k, a record with bytes outside the alphabet."""
    rng = random.Random(100 * k + alphabet)
    odd = _odd(alphabet)
    s = _letters(rng, alphabet, 3 * k + 40)
    recs = [_letters(rng, alphabet, 700), _letters(rng, alphabet, 2 * k + 7), "T" * (k + 8),
            s[:k + 3] + odd + s[k + 3:2 * k + 9] + odd + odd + s[2 * k + 9:]]
    return "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)).encode()


def _windows(text: bytes, k: int):
    for rec in text.decode().split(">")[1:]:
        seq = rec.split("\n", 1)[1].replace("\n", "")
        for i in range(len(seq) - k + 1):
            yield seq[i:i + k]


def _pool(name: str):
    """The keys of the case, SIZES[-1] of them: present and absent ones in turn, keys kept as text first, and in front of
    them the key the case is about."""
    alphabet, k, _, _, lead = CASES[name]
    rng = random.Random(name)
    letters, odd = set("ACGT" if alphabet == NT else AMINO), _odd(alphabet)
    seen = list(dict.fromkeys(_windows(_source(alphabet, k), k)))
    present = [w for w in seen if odd in w] + [w for w in seen if set(w) <= letters]
    absent = []
    for i in range(4 * SIZES[-1]):  # (a random 5-mer may well be in the table: it stays out)
        w = _letters(rng, alphabet, k)
        if lead == "text" or i % 7 == 3:
            w = w[:k // 2] + odd + w[k // 2 + 1:]
        if w not in seen and w not in absent:
            absent.append(w)
    if lead == "text":
        present = [w for w in present if odd in w]
    assert present and absent and odd in present[0]
    pool = (["T" * k] if lead == "side" else []) + [w for pair in zip(present, absent) for w in pair] + absent[len(present):]
    while len(pool) < SIZES[-1]:  # (few keys of the kind, or of this k: asked for again)
        pool += pool
    return pool[:SIZES[-1]]


def _canon(w: str) -> str:
    return min(w, w.translate(COMP)[::-1]) if set(w) <= set("ACGT") else w


@pytest.mark.parametrize("name", sorted(CASES))
def test_lookup_and_screen_agree_with_the_export(name):
    alphabet, k, canonical, fold, lead = CASES[name]
    pool = _pool(name)
    with native.Counter(k, alphabet, canonical=canonical) as ctx:
        ctx.count_chunk(_source(alphabet, k), 1)
        table = ctx.to_dict()
        assert table and all(len(key) == k for key in table)
        if lead == "side":
            assert table["T" * k] == 9  # (the run of k + 8)
        for n in SIZES:
            keys = pool[:n]
            want = [table.get(_canon(w) if fold else w, 0) for w in keys]  # the dict decides, nothing else
            if n > 1:
                assert any(want) and not all(want)
                assert any(c for w, c in zip(keys, want) if _odd(alphabet) in w)  # a key kept as text that is there
            info_l, info_s = {}, {}
            got = ctx.lookup(keys, fold=fold, info=info_l).tolist()
            rows = ctx.screen("".join(">%d\n%s\n" % (i, w) for i, w in enumerate(keys)).encode(), 1, fold=fold, info=info_s).tolist()
            print(name, n, "found", info_l["found"], "hits", info_s["hits"], "text keys", info_l["text_keys"])
            assert got == want
            assert rows == [[1, 1 if c else 0, c, c, c] for c in want]
            assert info_l["keys"] == info_s["windows"] == info_s["records"] == n
            assert info_l["found"] == info_s["hits"] == sum(1 for c in want if c)
            assert info_l["text_keys"] == info_s["text_windows"] and info_l["packed_keys"] == info_s["packed_windows"]
            assert info_l["folded"] == info_s["folded"]
