"""The rule of mk_table_op (include/mercat_hip.h) restated over Python dicts: what the GPU tests compare
Counter.combine with.  Nothing here touches the library."""
M64 = (1 << 64) - 1
OPS = ("min", "max", "sum", "left", "only", "diff")

F = {
    "min": lambda ca, cb: min(ca, cb),
    "max": lambda ca, cb: max(ca, cb),
    "sum": lambda ca, cb: (ca + cb) & M64,
    "left": lambda ca, cb: ca if cb else 0,
    "only": lambda ca, cb: 0 if cb else ca,
    "diff": lambda ca, cb: ca - cb if ca > cb else 0,
}


def combine(a: dict, b: dict, op: str, min_a: int = 1, min_b: int = 1) -> dict:
    """For every key in a or b: ca, cb its counts, 0 where absent; a count below its threshold is first taken as 0; the
    result holds the key with f(ca, cb), and no row where that is 0."""
    out = {}
    for key in set(a) | set(b):
        ca, cb = a.get(key, 0), b.get(key, 0)
        ca, cb = (ca if ca >= min_a else 0), (cb if cb >= min_b else 0)
        f = F[op](ca, cb)
        if f:
            out[key] = f
    return out


def figures(a: dict, b: dict, op: str, min_a: int = 1, min_b: int = 1, out: dict = None) -> dict:
    """The fields of mk_table_op_t that follow from the tables alone (``out``: combine's result, if at hand)."""
    ka = {key for key, c in a.items() if c and c >= min_a}
    kb = {key for key, c in b.items() if c and c >= min_b}
    if out is None:
        out = combine(a, b, op, min_a, min_b)
    return {"rows_a": len(ka), "rows_b": len(kb), "both": len(ka & kb), "rows_out": len(out),
            "total_out": sum(out.values()) & M64, "passes": 2 if op in ("max", "sum") else 1}
