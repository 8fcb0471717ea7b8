"""The closed forms of mercat2_amd/diversity.py fed with EXACT moments (tests/alpha_moments.py) against the oracle's
restatement of scikit-bio's functions on the count column itself (oracle/alpha_ref.py): whatever differs here is the
closed forms' doing, not a kernel's.  No kernel is launched."""
import random

import pytest

import alpha_moments as am
from mercat2_amd import diversity
from oracle import alpha_ref

SEEDS = {1: 60, 2: 60, 3: 60, 4: 60, 5: 60, 8: 60, 50: 30, 100: 30, 300: 30, 1000: 25, 5000: 25}  # per kind: 3000 tables
TIED = ("dominance", "simpson")


def _closed(counts):
    return diversity.alpha_from_stats(am.exact_moments(counts))


def test_closed_forms_print_what_the_oracle_prints(capsys):
    """Six kinds of table at eleven row counts.  A table is left out -- for dominance and simpson only -- when the two
    differ there AND its dominance is an exact decimal tie (decided in integers): the reference's float sum of (c/n)^2
    and the one division of the closed form may then round to different sides, which no moment can repair.  At most 1 %
    of a row count's tables."""
    bad, report = [], []
    assert sum(SEEDS.values()) * len(am.KINDS) >= 3000 and sorted(SEEDS) == am.ROWS
    for rows in am.ROWS:
        cases = left_out = 0
        for kind in am.KINDS:
            for seed in range(SEEDS[rows]):
                counts = am.table(kind, rows, random.Random("%s/%d/%d" % (kind, rows, seed)))
                assert len(counts) == rows and min(counts) >= 1
                got, want = _closed(counts), alpha_ref.alpha_table(counts)
                differ = [m for m in alpha_ref.METRICS if got[m] != want[m]]
                cases += 1
                if differ and set(differ) <= set(TIED) and am.dominance_is_exact_tie(counts):
                    left_out += 1
                elif differ:
                    bad.append((kind, rows, seed, [(m, got[m], want[m]) for m in differ]))
        report.append("rows %5d: %d of %d tables left out as exact ties (%.2f %%)" % (rows, left_out, cases, 100.0 * left_out / cases))
        assert left_out * 100 <= cases, report[-1]
    with capsys.disabled():
        print("\n" + "\n".join(report))
    assert not bad, (len(bad), bad[:5])


def test_the_tie_rule_and_its_example():
    """[7, 5, 8]: sum c^2 / n^2 = 138 / 400 = 0.345 exactly.  The float sum of (c/n)^2 lands above it, the division
    below: the limit DESIGN 8c documents.  Everything but dominance and simpson still agrees."""
    assert am.dominance_is_exact_tie([7, 5, 8]) and not am.dominance_is_exact_tie([7, 5, 9])
    assert am.dominance_is_exact_tie([1, 3])  # 0.625, and exact in float64 on both routes
    assert _closed([1, 3]) == alpha_ref.alpha_table([1, 3])
    got, want = _closed([7, 5, 8]), alpha_ref.alpha_table([7, 5, 8])
    assert (want["dominance"], got["dominance"]) == ("0.35", "0.34")
    assert {m for m in alpha_ref.METRICS if got[m] != want[m]} <= set(TIED)


@pytest.mark.parametrize("count", [1, 2, 7, 1000, (1 << 40) + 1, (1 << 64) - 1])
def test_one_row_prints_minus_zero(count):
    """-(1 * ln 1) / ln 2 is -0.0, and round(-0.0, 2) prints as '-0.0'."""
    got = _closed([count])
    assert got["shannon"] == "-0.0" == alpha_ref.alpha_table([count])["shannon"]
    assert got == alpha_ref.alpha_table([count])


@pytest.mark.parametrize("counts", [[1, 1], [1, 2], [5, 5], [1, 1 << 40], [1 << 40, 1], [1, (1 << 64) - 2], [3, 1 << 62]])
def test_two_rows_never_print_a_negative_shannon(counts):
    """Every term -p ln p of two rows is positive: '0.0' at the least, never '-0.0'."""
    got = _closed(counts)
    assert not got["shannon"].startswith("-") and got["shannon"] == alpha_ref.alpha_table(counts)["shannon"]


def test_all_singletons():
    got = _closed([1, 1, 1])
    assert got["ace"] == "NA" and got["fisher_alpha"] == "NA" and got == alpha_ref.alpha_table([1, 1, 1])
    assert got["shannon"] == "1.58" and got["goods_coverage"] == "0.0" and got["chao1"] == "6.0"


@pytest.mark.parametrize("counts,chao1,ci", [
    ([1, 1, 1, 2, 2, 5, 9], "8.0", "[7.09, 17.68]"),      # singletons and doubletons
    ([2, 2, 3, 5, 9], "5.0", "[5, 5.62]"),                # s = 0: the Poisson form, lower end clipped at observed
    ([1, 1, 1, 3, 5, 10], "9.0", "[6.37, 30.6]"),         # d = 0
    ([3, 4, 5, 9], "4.0", "[4, 4.31]"),                   # both 0
    ([1, 2, 3], "3.0", "NA"),                             # one singleton: chao1 == observed, the log of 1 + var / 0
])
def test_chao1_ci_branches(counts, chao1, ci):
    assert not am.dominance_is_exact_tie(counts)
    got = _closed(counts)
    assert got == alpha_ref.alpha_table(counts)
    assert (got["chao1"], got["chao1_ci"]) == (chao1, ci)
