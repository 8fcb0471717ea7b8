"""native.pair_stats_matrix (mk_beta.hip) and native.gram_matrix (mk_gram.hip) at the edges of their launch plan:
tests/pair_moments.py names the shapes and the plan property each exists for (tests/test_pair_moments_host.py proves
by plan() that each still reaches it), and gives the exact integers, the canb / seuc references and their derived bounds.

For every case: all integer fields equal the reference, canb and seuc are within the bounds (seuc is left out only
under a flagged constant row; counts of 2^53 and more keep a relative 1e-9), the Gram matrix equals the reference and
the pair kernel's dot (two kernels, one answer), and a second call gives the same bytes in the f64 fields.

Every case prints its worst canb / seuc error in units of the bound (pytest -s): DESIGN 8i records the largest."""
import numpy as np
import pytest

from mercat2_amd import native

import pair_moments as pm

pytestmark = pytest.mark.gpu

SHAPES = [(r, n) for r, n, _ in pm.CASES]


def _check(rows, n, pattern):
    ref = pm.reference(rows, n, pattern)
    m, want = ref["matrix"], ref["ints"]
    got = native.pair_stats_matrix(m)
    pm.same_ints(got, want)
    gram = native.gram_matrix(m)
    assert gram == want["dot"]
    assert gram == got["dot"]
    if ref["small"]:
        worst = pm.check_f64(got, m, want, ref["canb"], ref["seuc"])
    else:
        worst = pm.check_f64(got, m, want)
    print("pair shape %s %-24s canb %.4f seuc %.4f of the bound" % (pm.case_id(rows, n), pattern, worst["canb"], worst["seuc"]))
    again = native.pair_stats_matrix(m)
    assert again["canb"].tobytes() == got["canb"].tobytes()
    assert again["seuc"].tobytes() == got["seuc"].tobytes()
    pm.same_ints(again, want)
    return got


@pytest.mark.parametrize("rows,n", SHAPES, ids=[pm.case_id(*s) for s in SHAPES])
def test_plan_edges(rows, n):
    got = _check(rows, n, "base")
    assert got["constant_row"] == (n == 1)


@pytest.mark.parametrize("rows,n", pm.SMALL, ids=[pm.case_id(*s) for s in pm.SMALL])
@pytest.mark.parametrize("pattern", [p for p in pm.PATTERNS if p.startswith("2^32")])
def test_switch_between_the_product_paths(rows, n, pattern):
    """Every count at most 2^32 - 1 with rows of (2^32 - 1)^2 that carry out of 64 bits in the 32 x 32 path; then one
    cell of 2^32, which alone sends the whole matrix through the 64 x 64 path."""
    _check(rows, n, pattern)


@pytest.mark.parametrize("rows,n", [s for s in pm.SMALL if s[0] <= 256], ids=[pm.case_id(*s) for s in pm.SMALL if s[0] <= 256])
def test_counts_up_to_2_62(rows, n):
    """Counts up to 2^62 - 1 in eight rows, below 2^59 in the others, so that every 128-bit sum stays below 2^128 (the
    kernels add modulo 2^128; 256 squares of 2^62 would not fit).  Integers exact; canb and seuc to 1e-9 against float64,
    because counts of 2^53 and more round when they are converted."""
    assert not pm.reference(rows, n, "large")["small"]
    _check(rows, n, "large")


@pytest.mark.parametrize("rows,n", pm.SMALL, ids=[pm.case_id(*s) for s in pm.SMALL])
def test_zero_column(rows, n):
    got = _check(rows, n, "zero column")
    z = n // 2
    assert got["sums"][z] == 0 and not got["both"][z].any() and all(v == 0 for v in got["dot"][z])


@pytest.mark.parametrize("rows,n", pm.SMALL, ids=[pm.case_id(*s) for s in pm.SMALL])
def test_twin_columns(rows, n):
    got = _check(rows, n, "twin columns")
    assert got["l1"][0][n - 1] == 0 and got["neq"][0, n - 1] == 0 and got["cheb"][0, n - 1] == 0
    assert got["canb"][0, n - 1] == 0.0 and got["canb"][n - 1, 0] == 0.0


@pytest.mark.parametrize("rows,n", pm.SMALL, ids=[pm.case_id(*s) for s in pm.SMALL])
def test_constant_row_is_flagged(rows, n):
    got = _check(rows, n, "constant row")
    assert got["constant_row"]


@pytest.mark.parametrize("n", [1, 2, 23, 300])
def test_no_rows(n):
    m = np.zeros((0, n), dtype=np.uint64)
    got = native.pair_stats_matrix(m)
    pm.same_ints(got, pm.exact_ints(m))
    assert not got["canb"].any() and not got["seuc"].any() and not got["constant_row"]
    assert native.gram_matrix(m) == [[0] * n for _ in range(n)]
