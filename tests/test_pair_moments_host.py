"""tests/pair_moments.py checked on the host: its exact statistics against brute-force Python ints, exact rationals and
scipy's pdist; its plan() against the properties every named case claims (a case that stops reaching its path after a
constant of mk_beta.hip / mk_gram.hip changes fails here, not silently); and its canb / seuc bounds against plain float64
evaluations in three summation orders, so that the inputs of tests/test_gpu_pair_shapes.py let a correct kernel pass."""
import numpy as np
import pytest

import pair_moments as pm

SHAPES = [(r, n) for r, n, _ in pm.CASES]
F64_PATTERNS = [p for p in pm.PATTERNS if p != "large"]


# ------------------------------------------------------------------------------------------ the reference itself
def _tiny(seed):
    rng = np.random.default_rng(seed)
    rows, n = int(rng.integers(1, 9)), int(rng.integers(1, 8))
    top = [4, 1000, 1 << 33, 1 << 62][seed % 4]
    m = rng.integers(0, top, (rows, n), dtype=np.uint64)
    m[rng.random((rows, n)) < 0.3] = 0
    return m


@pytest.mark.parametrize("seed", range(24))
def test_exact_ints_equal_brute_force(seed):
    m = _tiny(seed)
    got, want = pm.exact_ints(m), pm.brute_ints(m)
    for key in pm.INTS:
        g = got[key].tolist() if isinstance(got[key], np.ndarray) else got[key]
        assert g == want[key], key
    assert pm.xtx(m) == want["dot"]


@pytest.mark.parametrize("seed", range(24))
def test_f64_references_equal_exact_rationals(seed):
    """The long double sums, rounded to float64, are within one ulp of the exact rational sums rounded once."""
    m = _tiny(seed)
    if m.shape[1] < 2:
        return
    canb, seuc = pm.f64_refs(m)
    want_c, want_s = pm._f64_refs_fractions(m)
    assert np.all(np.abs(canb - want_c) <= 2 * pm.U * want_c)
    if np.isnan(want_s).any():
        assert pm.exact_ints(m)["constant_row"] and np.isnan(seuc[0, 1])
    else:
        assert np.all(np.abs(seuc - want_s) <= 2 * pm.U * want_s)


def test_long_double_of_a_large_int_is_exact():
    for v in (0, 1, (1 << 64) - 1, (1 << 63) + 1, ((1 << 64) - 1) << 60):
        assert int(pm._ld(v)) == v


@pytest.mark.parametrize("seed", range(12))
def test_reference_against_scipy_pdist(seed):
    """Small counts, n < 8: scipy's cityblock, chebyshev, hamming and sqeuclidean sums are exact in float64; canberra and
    seuclidean are float64 sums of the same terms (seuclidean's square root and its square here: 3 more roundings)."""
    distance = pytest.importorskip("scipy.spatial.distance")
    rng = np.random.default_rng(100 + seed)
    rows, n = int(rng.integers(2, 40)), int(rng.integers(2, 8))
    m = rng.integers(0, 50, (rows, n), dtype=np.uint64)
    pm._mend_constant_rows(m, 0)
    ints = pm.exact_ints(m)
    assert not ints["constant_row"]
    canb, seuc = pm.f64_refs(m)
    obs = m.T.astype(np.float64)
    sq = distance.squareform
    assert sq(distance.pdist(obs, "cityblock")).tolist() == [[float(v) for v in r] for r in ints["l1"]]
    assert np.array_equal(sq(distance.pdist(obs, "chebyshev")), ints["cheb"].astype(np.float64))
    assert np.array_equal(np.rint(sq(distance.pdist(obs, "hamming")) * rows), ints["neq"].astype(np.float64))
    dot = np.array(ints["dot"], dtype=np.float64)
    assert np.array_equal(sq(distance.pdist(obs, "sqeuclidean")), np.diag(dot)[:, None] + np.diag(dot)[None, :] - 2 * dot)
    assert np.all(np.abs(sq(distance.pdist(obs, "canberra")) - canb) <= pm.canb_bound(rows, canb))
    got = sq(distance.pdist(obs, "seuclidean", V=obs.var(axis=0, ddof=1))) ** 2
    assert np.all(np.abs(got - seuc) <= pm.seuc_bound(m, seuc) + 4 * pm.U * seuc)


# ------------------------------------------------------------------------------------------ the plan
def test_plan_of_documented_shapes():
    """The figures DESIGN 8i quotes."""
    assert [pm.plan(1, n, "pair")["G"] for n in (1, 2, 3, 15, 16, 22, 23)] == [256, 85, 42, 2, 1, 1, 1]
    assert pm.plan(1, 23, "pair")["tiles"] == 2 and pm.plan(1, 23, "pair")["last_tile"] == 20
    assert pm.plan(1, 2, "pair")["busy"] == 255 and pm.plan(1, 16, "pair")["busy"] == 136
    assert pm.plan(144, 300, "pair")["R"] == 13 and pm.plan(144, 300, "pair")["tiles"] == 177
    assert pm.plan(106, 257, "pair")["tiles"] == 130 and pm.plan(4081, 100, "gram")["tiles"] == 20
    assert pm.plan(256 * 512 + 1, 2, "gram")["gx"] == 257 and pm.plan(8, 8, "pair")["G"] == 7


@pytest.mark.parametrize("rows,n,props", pm.CASES, ids=[pm.case_id(r, n) for r, n, _ in pm.CASES])
def test_case_has_the_properties_it_claims(rows, n, props):
    assert props
    for name in props:
        kinds, holds = pm.PROPERTIES[name]
        for kind in kinds:
            assert holds(pm.plan(rows, n, kind)), (name, kind, pm.plan(rows, n, kind))


@pytest.mark.parametrize("name", sorted(pm.PROPERTIES))
def test_every_property_is_hit_for_each_kernel(name):
    kinds, holds = pm.PROPERTIES[name]
    for kind in kinds:
        assert [1 for rows, n, props in pm.CASES if name in props and holds(pm.plan(rows, n, kind))], (name, kind)


def test_every_shape_has_no_constant_row():
    """seuc is compared for every shape: only n = 1 (no pair at all) cannot avoid a constant row."""
    for rows, n in SHAPES + pm.SMALL:
        assert pm.exact_ints(pm.matrix(rows, n))["constant_row"] == (n == 1), (rows, n)
        m = pm.matrix(rows, n)
        assert int(m.max()) < (1 << 16)
        assert m.size < 500 or 0.25 < float((m == 0).mean()) < 0.42


def test_patterns_are_what_they_say():
    for rows, n in pm.SMALL:
        m = pm.matrix(rows, n, "2^32-1")
        assert int(m.max()) == (1 << 32) - 1 and int(((m[:, 0] == m.max()) & (m[:, n - 1] == m.max())).sum()) >= 5
        for w, (r, c) in zip(pm.WIDE_CELLS, [(0, 0), (0, n - 1), (rows - 1, 0), (rows - 1, n - 1)]):
            m = pm.matrix(rows, n, "2^32 at " + w)
            assert int(m[r, c]) == 1 << 32 and int((m >= (1 << 32)).sum()) == 1
            assert int(((m[:, 0] == (1 << 32) - 1) & (m[:, n - 1] == (1 << 32) - 1)).sum()) >= 5
        assert not pm.matrix(rows, n, "zero column")[:, n // 2].any()
        m = pm.matrix(rows, n, "twin columns")
        assert np.array_equal(m[:, 0], m[:, n - 1])
        assert pm.exact_ints(pm.matrix(rows, n, "constant row"))["constant_row"]
        for p in ("zero column", "twin columns"):
            assert pm.exact_ints(pm.matrix(rows, n, p))["constant_row"] == (n <= (2 if p == "twin columns" else 1)), (rows, n, p)
        if rows <= 256:
            m = pm.matrix(rows, n, "large")
            assert int(m.max()) == (1 << 62) - 1 and max(max(r) for r in pm.xtx(m)) < 1 << 128


# ------------------------------------------------------------------------------------------ the bounds
def _float64_pass(m, order):
    """canb and seuc as the kernels compute them, in float64: the row variance by mean and squared deviations (summed
    left to right), 1 / V, the product; the rows added first to last, last to first, or by numpy's pairwise sum."""
    F = m.astype(np.float64)
    rows, n = F.shape
    mean = np.cumsum(F, axis=1)[:, -1] / n
    q = np.cumsum((F - mean[:, None]) ** 2, axis=1)[:, -1]
    with np.errstate(all="ignore"):
        inv = 1.0 / (q / (n - 1))
    if order == "reversed":
        F, inv = F[::-1], inv[::-1]
    total = (lambda a: a.sum(axis=0)) if order == "numpy" else (lambda a: np.cumsum(a, axis=0)[-1])
    canb, seuc = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        d = F - F[:, i:i + 1]
        s = F + F[:, i:i + 1]
        with np.errstate(all="ignore"):
            canb[i] = total(np.where(s > 0, np.abs(d) / np.where(s > 0, s, 1.0), 0.0))
            seuc[i] = total(d * d * inv[:, None])
    np.fill_diagonal(canb, 0)
    np.fill_diagonal(seuc, 0)
    return {"canb": canb, "seuc": seuc}


def _inside(rows, n, pattern):
    ref = pm.reference(rows, n, pattern)
    assert ref["small"]
    for order in ("sequential", "reversed", "numpy"):
        got = _float64_pass(ref["matrix"], order)
        worst = pm.check_f64(got, ref["matrix"], ref["ints"], ref["canb"], ref["seuc"])
        assert worst["canb"] <= 1 and worst["seuc"] <= 1


@pytest.mark.parametrize("rows,n", [s for s in SHAPES if s[1] > 1], ids=[pm.case_id(*s) for s in SHAPES if s[1] > 1])
def test_float64_stays_inside_the_bounds(rows, n):
    _inside(rows, n, "base")


@pytest.mark.parametrize("pattern", F64_PATTERNS)
def test_float64_stays_inside_the_bounds_small_shapes(pattern):
    for rows, n in pm.SMALL:
        if n > 1:
            _inside(rows, n, pattern)


def test_bound_catches_one_lost_row():
    """The bounds are tight enough to see a single row dropped from a sum of 4081."""
    ref = pm.reference(102 * 40 + 1, 100)
    got = _float64_pass(ref["matrix"][:-1], "sequential")
    with pytest.raises(AssertionError):
        pm.check_f64(got, ref["matrix"], ref["ints"], ref["canb"], ref["seuc"])


def test_near_constant_rows_of_large_counts_need_the_second_term():
    """Rows of about 2^40 with spread 1, n = 3 (the mean rounds): the two-pass variance is off by some 3e8 u, far more than
    (rows + n + 8) u and more than the relative 1e-9 of a float64 reference, and inside a (1 + k)."""
    rng = np.random.default_rng(7)
    m = (np.uint64(1 << 40) + rng.integers(0, 2, (500, 3), dtype=np.uint64)).astype(np.uint64)
    pm._mend_constant_rows(m, 0)
    ints = pm.exact_ints(m)
    assert not ints["constant_row"] and pm.seuc_a(m) > 1e8 * pm.U
    got = _float64_pass(m, "sequential")
    _, seuc = pm.f64_refs(m)
    off = ~np.eye(3, dtype=bool)
    assert (np.abs(got["seuc"] - seuc)[off] / seuc[off]).max() > 1e-9
    pm.check_f64(got, m, ints)
