"""The per-pair statistics of mk_pair_stats / mk_gram (include/mercat_hip.h, mk_beta.hip, mk_gram.hip) restated over a
rows x n uint64 matrix, the launch plan of both kernels restated from their constants, and the named shapes the
tests draw: what tests/test_pair_moments_host.py, tests/test_gpu_pair_shapes.py, tests/test_gpu_join_edges.py,
tests/test_gpu_beta.py and tests/test_gpu_pca.py compare the library with.  Nothing here touches the library.

Integers are exact: numpy int64 where nothing can overflow, Python ints otherwise.  ``canb`` and ``seuc`` are summed in
numpy.longdouble where it carries 64 bits (else in exact rationals), ``seuc`` from exact integers:
(x - y)^2 n (n - 1) / D_r with D_r = n sum x^2 - (sum x)^2, so the reference never rounds a variance.

The bounds, u = 2^-53, every count below 2^53 so that int -> f64 and x - y are exact:

  canb  a term fl(|x - y| / fl(x + y)) carries at most 3 roundings (2 here), the rows terms are non-negative and are
        added in some order; additions of a zero are exact, so a term passes through at most rows - 1 rounded
        additions: |got - ref| <= gamma(rows + 2) ref <= (rows + 4) u ref   (gamma(k) = k u / (1 - k u) <= (k + 2) u
        for k < 2^27).
  seuc  1 / V_r: mean^ = fl(S^ / n) = mean + d; q^ = fl sum fl(x_i - mean^)^2 = (q + n d^2)(1 + t), |t| <= gamma(n + 2),
        because sum (x_i - mean) = 0 takes the cross term out exactly; n d^2 / q = (d / mean)^2 S^2 / D.  |d| <= u mean
        when every row sum is below 2^53 (S^ is exact), else <= n u mean.  Then the divisions by n - 1 and into 1, the
        square of x - y and the product: 4 more roundings, and rows - 1 additions:
        |got - ref| <= [k + a (1 + k)] ref, k = (rows + n + 8) u, a = c^2 u^2 max_r S_r^2 / D_r, c = 1 or n as above.
  Both get the reference's own error on top: (rows + 4) eps of the long double (2^-64: rows u / 2048).
Counts of 2^53 and more round on conversion; those tables keep a relative 1e-9 against float64 (``close_enough``)."""
import fractions
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)
LD_OK = LD_EPS <= 2.0 ** -63
INTS = ("dot", "l1", "cheb", "neq", "both", "sums", "rows", "constant_row")

# mk_beta.hip:29-31 (kThreads, kLdsBytes, kGridTarget) and mk_gram.hip:18-20 (kPairTile, kLdsBytes, kGridTarget);
# the plan itself: PairAcc::init mk_beta.hip:189-193, 202, PairAcc::add :228-229, 235; GramAcc::init mk_gram.hip:124-126,
# 135, GramAcc::add :156-157, 163
THREADS, LDS_BYTES, GRID_TARGET, R_MAX, WG_REDUCE_FROM, WG_THREADS = 256, 32768, 2048, 512, 64, 256


def plan(rows: int, n: int, kind: str) -> dict:
    """The launch of one add() of ``rows`` x ``n``: kind "pair" (mk_beta_pair_k) or "gram" (mk_gram_k)."""
    assert kind in ("pair", "gram") and n >= 1
    P = n * (n + 1) // 2
    if kind == "pair":
        T = min(P, THREADS)
        G = THREADS // T
        R = max(1, min(R_MAX, LDS_BYTES // (8 * (n + 1))))
    else:
        T, G = THREADS, 1
        R = max(1, min(R_MAX, LDS_BYTES // (8 * n)))
    tiles = -(-P // T)
    ws_blocks = max(1, GRID_TARGET // tiles)
    blocks = -(-rows // R)
    gx = min(ws_blocks, blocks)
    return {"P": P, "T": T, "G": G, "tiles": tiles, "R": R, "ws_blocks": ws_blocks, "blocks": blocks, "gx": gx,
            "tail": rows - (blocks - 1) * R if rows else 0, "strides": blocks > ws_blocks,
            "wg_reduce": gx >= WG_REDUCE_FROM, "wg_strided": gx > WG_THREADS, "n": n,
            "busy": min(P, T) * G if tiles == 1 else THREADS, "last_tile": P - (tiles - 1) * T}


# property -> (the kernels it exists for, predicate over plan())
PROPERTIES = {
    "tail rows < G": (("pair",), lambda p: p["G"] > 1 and 0 < p["tail"] < p["G"]),
    "tail rows = G": (("pair",), lambda p: p["G"] > 1 and p["tail"] == p["G"]),
    "tail rows > G, no multiple": (("pair",), lambda p: p["G"] > 1 and p["tail"] > p["G"] and p["tail"] % p["G"] != 0),
    "G = 256": (("pair",), lambda p: p["G"] == 256),
    "G = 85, one idle lane": (("pair",), lambda p: p["G"] == 85 and p["busy"] == 255),
    "G = 2, 16 idle lanes": (("pair",), lambda p: p["G"] == 2 and p["busy"] == 240),
    "G = 1, 120 idle lanes": (("pair", "gram"), lambda p: p["G"] == 1 and p["tiles"] == 1 and p["P"] == 136),
    "one-row tail block": (("pair", "gram"), lambda p: p["blocks"] > 1 and p["tail"] == 1),
    "one tile, nearly full": (("pair", "gram"), lambda p: p["tiles"] == 1 and p["P"] >= 250),
    "last tile nearly empty": (("pair", "gram"), lambda p: p["tiles"] > 1 and p["last_tile"] <= 20),
    "gx = 63, reduce_k": (("pair", "gram"), lambda p: p["gx"] == 63 and not p["wg_reduce"] and not p["strides"]),
    "gx = 64, reduce_wg_k": (("pair", "gram"), lambda p: p["gx"] == 64 and p["wg_reduce"] and not p["strides"]),
    "reduce_wg_k strided": (("pair", "gram"), lambda p: p["wg_strided"]),
    "grid-stride, G > 1": (("pair",), lambda p: p["strides"] and p["G"] > 1),
    "grid-stride and reduce_wg_k": (("pair", "gram"), lambda p: p["strides"] and p["wg_reduce"] and p["tiles"] > 1),
    "grid-stride and reduce_k": (("pair", "gram"), lambda p: p["strides"] and not p["wg_reduce"] and p["tiles"] > 100),
    "n past 256": (("pair", "gram"), lambda p: p["n"] > 256 and p["tiles"] > 100),
}

# the named shapes: (rows, n, the properties the case exists for)
CASES = [
    (1, 1, ["G = 256", "tail rows < G"]),
    (255, 1, ["G = 256", "tail rows < G"]),
    (256, 1, ["G = 256", "tail rows = G"]),
    (257, 1, ["G = 256", "tail rows > G, no multiple"]),
    (513, 1, ["G = 256", "tail rows < G", "one-row tail block"]),
    (84, 2, ["G = 85, one idle lane", "tail rows < G"]),
    (85, 2, ["G = 85, one idle lane", "tail rows = G"]),
    (86, 2, ["G = 85, one idle lane", "tail rows > G, no multiple"]),
    (513, 2, ["G = 85, one idle lane", "tail rows < G", "one-row tail block"]),
    (513, 3, ["tail rows < G", "one-row tail block"]),
    (700, 15, ["G = 2, 16 idle lanes"]),
    (700, 16, ["G = 1, 120 idle lanes"]),
    (300, 22, ["one tile, nearly full"]),
    (300, 23, ["last tile nearly empty"]),
    (63 * 512, 2, ["gx = 63, reduce_k"]),
    (63 * 512 + 1, 2, ["gx = 64, reduce_wg_k", "one-row tail block"]),
    (256 * 512 + 1, 2, ["reduce_wg_k strided", "one-row tail block"]),
    (2048 * 512 + 1, 2, ["grid-stride, G > 1", "reduce_wg_k strided"]),
    (102 * 40 + 1, 100, ["grid-stride and reduce_wg_k"]),
    (144, 300, ["grid-stride and reduce_k", "n past 256"]),
    (106, 257, ["n past 256"]),
]
# the shapes the further count patterns are applied to (rows <= 256 among them for the counts up to 2^62)
SMALL = [(6, 3), (255, 1), (257, 1), (86, 2), (513, 2), (256, 3), (700, 15), (300, 23)]
WIDE_CELLS = ["row 0, column 0", "row 0, column n-1", "last row, column 0", "last row, column n-1"]
PATTERNS = ["base", "2^32-1"] + ["2^32 at " + w for w in WIDE_CELLS] + ["large", "zero column", "twin columns",
                                                                         "constant row"]


def case_id(rows: int, n: int) -> str:
    return "%dx%d" % (rows, n)


def _mend_constant_rows(m: np.ndarray, col: int) -> None:
    """Rows that hold one value in every column get another one in column ``col`` (the lowest bit flipped)."""
    if m.shape[1] > 1:
        flat = np.flatnonzero((m == m[:, :1]).all(axis=1))
        m[flat, col] ^= np.uint64(1)


def _draw(rng, rows: int, n: int, top: int) -> np.ndarray:
    m = rng.integers(1, top, (rows, n), dtype=np.uint64)
    m[rng.random((rows, n)) < 1 / 3] = 0
    return m


def matrix(rows: int, n: int, pattern: str = "base") -> np.ndarray:
    """The seeded rows x n uint64 matrix of a case.  "base": counts below 2^16, about a third of the cells zero, no
    constant row (n > 1).  The others start from it."""
    rng = np.random.default_rng([rows, n, PATTERNS.index(pattern)])
    m = _draw(rng, rows, n, 1 << 16)
    _mend_constant_rows(m, n - 1)
    if pattern == "base" or not rows:
        return m
    if pattern.startswith("2^32"):
        m = _draw(rng, rows, n, 1 << 32)
        picked = rng.choice(rows, min(rows, 7), replace=False)
        for col in {0, n - 1}:
            m[picked, col] = np.uint64((1 << 32) - 1)  # (five rows of (2^32 - 1)^2 already carry out of 64 bits)
        if n > 2:  # (n = 1, 2: the picked rows are constant, so seuc is compared in the other patterns only)
            _mend_constant_rows(m, 1)
        if pattern != "2^32-1":
            where = pattern[len("2^32 at "):]
            m[0 if where.startswith("row 0") else rows - 1, 0 if where.endswith("column 0") else n - 1] = np.uint64(1 << 32)
            if n > 2:
                _mend_constant_rows(m, 1)
    elif pattern == "large":
        # counts up to 2^62 in 8 rows (8 squares below 2^124), below 2^59 in the others (at most 248 squares below 2^118):
        # every 128-bit sum of products stays below 2^127 + 2^126, which the kernels (sums modulo 2^128) need
        assert rows <= 256
        m = _draw(rng, rows, n, 1 << 59)
        big = rng.choice(rows, min(rows, 8), replace=False)
        m[big] = _draw(rng, big.size, n, 1 << 62)
        m[big[0], 0] = np.uint64((1 << 62) - 1)
        m[::3] >>= rng.integers(0, 59, m[::3].shape, dtype=np.uint64)
        m[big[0], 0] = np.uint64((1 << 62) - 1)
    elif pattern == "zero column":
        m[:, n // 2] = 0
        _mend_constant_rows(m, 0 if n // 2 else n - 1)
    elif pattern == "twin columns":
        m[:, n - 1] = m[:, 0]
        if n > 2:
            _mend_constant_rows(m, 1)
    elif pattern == "constant row":
        m[rows // 2] = m[rows // 2, 0] + np.uint64(7)
    return m


# ------------------------------------------------------------------------------------------ exact integers
def xtx(matrix_) -> list:
    """X^T X as nested lists of Python ints."""
    m = np.asarray(matrix_, dtype=np.uint64)
    n = m.shape[1]
    if not m.size:
        return [[0] * n for _ in range(n)]
    top = int(m.max())
    o = m.astype(np.int64) if top * top * m.shape[0] < (1 << 62) else m.astype(object)
    return [[int(v) for v in r] for r in o.T.dot(o)]


def exact_ints(X) -> dict:
    """dot, l1, sums as Python ints; cheb, neq, both as uint64 arrays; rows; constant_row."""
    X = np.asarray(X, dtype=np.uint64)
    rows, n = X.shape
    top = int(X.max()) if X.size else 0
    O = X.astype(np.int64) if top * top * max(rows, 1) < (1 << 62) else X.astype(object)
    l1 = np.zeros((n, n), dtype=object)
    cheb, neq, both = (np.zeros((n, n), dtype=np.uint64) for _ in range(3))
    for i in range(n):
        if not rows:
            break
        d = np.abs(O - O[:, i:i + 1])
        l1[i] = [int(v) for v in d.sum(axis=0)]
        cheb[i] = d.max(axis=0)
        neq[i] = (X != X[:, i:i + 1]).sum(axis=0)
        both[i] = ((X != 0) & (X[:, i:i + 1] != 0)).sum(axis=0)
    return {"dot": xtx(X), "l1": [[int(v) for v in r] for r in l1], "cheb": cheb, "neq": neq, "both": both,
            "sums": [int(v) for v in O.sum(axis=0)] if rows else [0] * n, "rows": rows,
            "constant_row": bool(n and rows and (X == X[:, :1]).all(axis=1).any())}


def brute_ints(X) -> dict:
    """The same over Python ints, one cell at a time (tiny matrices: what exact_ints is checked against)."""
    X = [[int(v) for v in r] for r in X]
    n = len(X[0]) if X else 0
    f = lambda fn: [[fn(i, j) for j in range(n)] for i in range(n)]
    return {"dot": f(lambda i, j: sum(r[i] * r[j] for r in X)), "l1": f(lambda i, j: sum(abs(r[i] - r[j]) for r in X)),
            "cheb": f(lambda i, j: max([abs(r[i] - r[j]) for r in X], default=0)),
            "neq": f(lambda i, j: sum(r[i] != r[j] for r in X)), "both": f(lambda i, j: sum(bool(r[i] and r[j]) for r in X)),
            "sums": [sum(r[i] for r in X) for i in range(n)], "rows": len(X),
            "constant_row": any(len(set(r)) == 1 for r in X)}


# ------------------------------------------------------------------------------------------ canb, seuc
def _ld(v: int):
    """A Python int as a long double (limbs of 48 bits, so that no step goes through float64)."""
    out, shift = LD(0), 0
    limbs = []
    while v:
        limbs.append((v & ((1 << 48) - 1), shift))
        v >>= 48
        shift += 48
    for limb, s in reversed(limbs):
        out = out + np.ldexp(LD(limb), s)
    return out


def row_moments(X):
    """(S_r, D_r) per row, exact: the row sum and n sum x^2 - (sum x)^2 (int64 arrays, or object arrays of Python ints)."""
    X = np.asarray(X, dtype=np.uint64)
    n = X.shape[1]
    top = int(X.max()) if X.size else 0
    O = X.astype(np.int64) if top * top * n * n < (1 << 62) else X.astype(object)
    S = O.sum(axis=1)
    return S, n * (O * O).sum(axis=1) - S * S


def _f64_refs_fractions(X):
    X = [[int(v) for v in r] for r in X]
    n = len(X[0])
    S = [sum(r) for r in X]
    D = [n * sum(v * v for v in r) - s * s for r, s in zip(X, S)]
    F = fractions.Fraction
    canb, seuc = np.zeros((n, n)), np.zeros((n, n))
    const = any(d == 0 for d in D)
    for i in range(n):
        for j in range(n):
            if i != j:
                canb[i, j] = float(sum(F(abs(r[i] - r[j]), r[i] + r[j]) for r in X if r[i] + r[j]))
                seuc[i, j] = np.nan if const else float(sum(F((r[i] - r[j]) ** 2 * n * (n - 1), d) for r, d in zip(X, D)))
    return canb, seuc


def f64_refs(X):
    """(canb, seuc) as n x n float64, each the reference sum rounded once; seuc is NaN off the diagonal when a row is
    constant (D_r = 0) and n > 1."""
    X = np.asarray(X, dtype=np.uint64)
    rows, n = X.shape
    if not rows or n < 2:
        return np.zeros((n, n)), np.zeros((n, n))
    if not LD_OK:
        return _f64_refs_fractions(X)
    _, D = row_moments(X)
    Dl = D.astype(LD) if D.dtype != object else np.array([_ld(int(d)) for d in D], dtype=LD)
    const = bool((Dl == 0).any())
    w = LD(n * (n - 1)) / np.where(Dl == 0, LD(1), Dl)
    L = X.astype(LD)  # (exact: 64 bits)
    canb, seuc = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        d = np.abs(L - L[:, i:i + 1])
        s = L + L[:, i:i + 1]
        canb[i] = (d / np.where(s > 0, s, LD(1))).sum(axis=0).astype(np.float64)
        seuc[i] = (d * d * w[:, None]).sum(axis=0).astype(np.float64)
    np.fill_diagonal(canb, 0)
    np.fill_diagonal(seuc, 0)
    if const:
        seuc[~np.eye(n, dtype=bool)] = np.nan
    return canb, seuc


def small_counts(X) -> bool:
    """Every count is below 2^53: the derived bounds hold."""
    X = np.asarray(X, dtype=np.uint64)
    return not X.size or int(X.max()) < (1 << 53)


def canb_bound(rows: int, ref):
    return ((rows + 4) * U + (rows + 4) * LD_EPS) * np.asarray(ref, dtype=np.float64)


def seuc_a(X) -> float:
    """a = c^2 u^2 max_r S_r^2 / D_r over the rows that are not constant (rounded up)."""
    X = np.asarray(X, dtype=np.uint64)
    n = X.shape[1]
    S, D = row_moments(X)
    if not len(S):
        return 0.0
    if D.dtype == object:
        worst = float(max([fractions.Fraction(int(s) * int(s), int(d)) for s, d in zip(S, D) if d], default=0))
    else:
        Sl, Dl = S.astype(LD), D.astype(LD)
        worst = float(np.max(np.where(Dl > 0, Sl * Sl / np.where(Dl > 0, Dl, LD(1)), LD(0))))
    c = 1 if int(S.max()) < (1 << 53) else n
    return float(np.nextafter(np.nextafter(worst, np.inf) * (c * U) ** 2, np.inf))


def seuc_bound(X, ref):
    X = np.asarray(X)
    rows, n = X.shape
    k = (rows + n + 8) * U
    return (k + seuc_a(X) * (1 + k) + (rows + 4) * LD_EPS) * np.asarray(ref, dtype=np.float64)


def close_enough(got, want) -> bool:
    """The relative 1e-9 (absolute below 1) that tables with counts of 2^53 and more keep."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))))


def float64_refs(X):
    """canb, seuc in plain numpy float64 (scipy's own arithmetic): the reference for counts of 2^53 and more."""
    X = np.asarray(X, dtype=np.uint64)
    rows, n = X.shape
    F = X.astype(np.float64)
    canb, seuc = np.zeros((n, n)), np.zeros((n, n))
    var = F.var(axis=1, ddof=1) if n > 1 and rows else np.ones(rows)
    for i in range(n):
        with np.errstate(all="ignore"):
            s = F + F[:, i:i + 1]
            canb[i] = np.where(s > 0, np.abs(F - F[:, i:i + 1]) / np.where(s > 0, s, 1), 0).sum(axis=0)
            seuc[i] = ((F - F[:, i:i + 1]) ** 2 / var[:, None]).sum(axis=0)
    np.fill_diagonal(canb, 0)
    np.fill_diagonal(seuc, 0)
    return canb, seuc


def exact(X) -> dict:
    """The dict ``native.pair_stats_matrix(X)`` returns: exact integers, canb / seuc in float64 as numpy computes them
    (what the 1e-9 comparisons of tests/test_gpu_beta.py use)."""
    out = exact_ints(X)
    out["canb"], out["seuc"] = float64_refs(X)
    return out


@functools.lru_cache(maxsize=None)
def reference(rows: int, n: int, pattern: str = "base") -> dict:
    """Everything a test needs of one named case, computed once: the matrix, the exact integers, the f64 references
    and their bounds (None where the counts reach 2^53)."""
    m = matrix(rows, n, pattern)
    m.setflags(write=False)
    out = {"matrix": m, "ints": exact_ints(m), "small": small_counts(m)}
    if out["small"]:
        out["canb"], out["seuc"] = f64_refs(m)
        out["canb_bound"] = canb_bound(rows, out["canb"])
        out["seuc_bound"] = None if out["ints"]["constant_row"] else seuc_bound(m, out["seuc"])
    else:
        out["canb"], out["seuc"] = float64_refs(m)
    return out


def check_f64(got: dict, X, ints: dict, canb=None, seuc=None) -> dict:
    """Assert got["canb"], got["seuc"] against the references of X (computed here unless given); returns the worst
    error of each in units of its bound.  The one comparison left out is seuc under a constant row."""
    X = np.asarray(X, dtype=np.uint64)
    rows, n = X.shape
    worst = {"canb": 0.0, "seuc": 0.0}
    if not small_counts(X):
        wc, ws = float64_refs(X)
        assert close_enough(got["canb"], wc), "canb"
        if not ints["constant_row"]:
            assert close_enough(got["seuc"], ws), "seuc"
        return worst
    if canb is None:
        canb, seuc = f64_refs(X)
    for key, ref, bound in (("canb", canb, canb_bound(rows, canb)),
                            ("seuc", seuc, None if ints["constant_row"] else seuc_bound(X, seuc))):
        if bound is None:
            continue
        err = np.abs(np.asarray(got[key], dtype=np.float64) - ref)
        with np.errstate(all="ignore"):
            worst[key] = float(np.nan_to_num(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0), initial=0.0)))
        assert np.all(err <= bound), (key, float(err.max()), worst[key])
    return worst


def same_ints(got: dict, want: dict) -> None:
    for key in INTS:
        g, w = got[key], want[key]
        if isinstance(g, np.ndarray) or isinstance(w, np.ndarray):
            assert np.array_equal(np.asarray(g, dtype=np.uint64), np.asarray(w, dtype=np.uint64)), key
        else:
            assert g == w, key
