"""The moments of mk_alpha_stats (include/mercat_hip.h) restated exactly over a list of Python ints, and the seeded
tables the alpha tests draw: what tests/test_alpha_moments_host.py and tests/test_gpu_alpha_moments.py compare
``diversity.alpha_from_stats`` and ``Counter.alpha_stats`` with.  Nothing here touches the library.

Integers stay Python ints.  ``sum_sq`` is the exact sum of squares rounded to float64 once.  ``sum_clnc`` is summed at 50
decimal digits over the DISTINCT counts (sum of m(v) * v * ln v, m = rows that hold v) and rounded once: the tables below
take their counts from a palette of at most 2000 values, so a reference costs 2000 logarithms whatever its rows."""
import collections
import decimal
import random

U = 2.0 ** -53          # unit roundoff of float64
MASK64 = (1 << 64) - 1
PALETTE = 2000
KINDS = ["1..3", "1..11", "pareto(1.1)", "10..999", "1..2^40", "singletons, doubletons, three large"]
ROWS = [1, 2, 3, 4, 5, 8, 50, 100, 300, 1000, 5000]

_CTX = decimal.Context(prec=50)


def sum_squares(counts) -> int:
    return sum(int(c) * int(c) for c in counts if c)


def exact_moments(counts) -> dict:
    """The dict ``Counter.alpha_stats()`` returns, for these counts (zeros are no rows)."""
    mult = collections.Counter(int(c) for c in counts if c)
    clnc = decimal.Decimal(0)
    for v, m in mult.items():
        if v > 1:
            clnc = _CTX.add(clnc, _CTX.multiply(m * v, _CTX.ln(decimal.Decimal(v))))
    return {"observed": sum(mult.values()), "total": sum(v * m for v, m in mult.items()) & MASK64,
            "freq": [0] + [mult.get(i, 0) for i in range(1, 11)],
            "sum_sq": float(sum(v * v * m for v, m in mult.items())), "sum_clnc": float(clnc)}


def clnc_bound(rows: int, ref: float) -> float:
    """|got - ref| allowed for a float64 sum of ``rows`` terms fl(d * fl(ln d)), d = fl(count), added in any order:
    (rows - 1) u for the additions of non-negative terms, and per term the conversion, the product and a logarithm
    good to 1 ulp (what the device library documents for its float64 log)."""
    return (rows + 8) * U * ref


def dominance_is_exact_tie(counts) -> bool:
    """Sum c^2 / n^2 lies exactly between two neighbours of two decimals: 200 * sum c^2 / n^2 is an odd integer."""
    n2 = sum(counts) ** 2
    q, r = divmod(200 * sum_squares(counts), n2)
    return r == 0 and q % 2 == 1


def table(kind: str, rows: int, rng: random.Random) -> list:
    """``rows`` counts of one of KINDS, drawn from a palette of at most PALETTE values."""
    if kind == KINDS[5]:
        large = [rng.randrange(1000, 1_000_000) for _ in range(3)]
        small = max(0, rows - 3)
        ones = rng.randint(0, small)
        out = large[:min(3, rows)] + [1] * ones + [2] * (small - ones)
        rng.shuffle(out)
        return out
    draw = {KINDS[0]: lambda: rng.randint(1, 3), KINDS[1]: lambda: rng.randint(1, 11),
            KINDS[2]: lambda: int(rng.paretovariate(1.1)), KINDS[3]: lambda: rng.randint(10, 999),
            KINDS[4]: lambda: rng.randint(1, 1 << 40)}[kind]
    palette = [draw() for _ in range(min(rows, PALETTE))]
    return [rng.choice(palette) for _ in range(rows)]
