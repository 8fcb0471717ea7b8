"""The rule of mk_norm_* (include/mercat_hip.h) restated over Python bytes and a dict: what the tests compare
Counter.normalize with.  Nothing here touches the library.

The text is read by the line loop of tests/trim_rule.py (the reference's: lines end at LF, CR LF or a lone CR; a line
whose stripped form starts with '>' opens a record; every other line gives ``line.strip().replace("*", "")`` to the record
it stands in).  Here every record also keeps its raw bytes -- from the first byte of its header line to the byte in
front of the next record's header line -- because an emitted record is copied as it stands.  Lines in front of the first
record that hold no kept character are the preamble and belong to no record."""
import trim_rule

M64 = (1 << 64) - 1
CLIP = (1 << 32) - 1


def records(text: bytes):
    """[(raw bytes, kept characters)] in text order.  The headless record runs from byte 0 (the blank lines in front of
    its first kept character are its own); b"".join of the raw bytes is the text minus its preamble."""
    recs, front = [], b""
    for line in trim_rule._LINE.findall(bytes(text)):
        stripped = line.strip(trim_rule._BLANKS)
        if stripped.startswith(b">"):
            recs.append([line, b""])
            continue
        piece = stripped.replace(b"*", b"")
        if not recs and piece:
            recs.append([front, b""])
        if recs:
            recs[-1][0] += line
            recs[-1][1] += piece
        else:
            front += line
    return [(raw, seq) for raw, seq in recs]


def preamble(text: bytes) -> int:
    """Bytes in front of the first header line of a text that is not headless (all of a text without records)."""
    return len(text) - sum(len(raw) for raw, _ in records(text))


def counts_of(seq: bytes, table: dict, k: int, fold: bool = False):
    return [trim_rule.count_of(table, seq[j:j + k], fold) for j in range(len(seq) - k + 1)]


def median_of(counts) -> int:
    """Element windows // 2 of min(count, 2^32 - 1) sorted ascending; 0 without windows."""
    return sorted(min(c, CLIP) for c in counts)[len(counts) // 2] if counts else 0


def u_of(seed: int, r: int) -> int:
    """The upper 32 bits of splitmix64 of record r under seed."""
    z = (seed + (r + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) >> 32


def kept_of(windows: int, med: int, r: int, target: int, min_depth: int = 0, seed: int = 0) -> bool:
    return windows > 0 and med >= min_depth and (med <= target or u_of(seed, r) * med < target << 32)


def expected(text: bytes, table: dict, k: int, target: int, min_depth: int = 0, seed: int = 0, invert: bool = False, fold: bool = False):
    """{"out", "keep", "median", "windows", and the five record counts of mk_norm_t}."""
    assert 1 <= target <= CLIP and 0 <= min_depth <= CLIP
    res = {"out": [], "keep": [], "median": [], "windows": [], "records_out": 0, "records_short": 0, "records_low": 0,
           "records_over": 0, "records_thinned": 0}
    for r, (raw, seq) in enumerate(records(text)):
        counts = counts_of(seq, table, k, fold)
        med = median_of(counts)
        kept = kept_of(len(counts), med, r, target, min_depth, seed)
        emit = kept != invert
        res["median"].append(med)
        res["windows"].append(len(counts))
        res["keep"].append(emit)
        if emit:
            res["out"].append(raw)
        res["records_out"] += emit
        res["records_short"] += not counts
        res["records_low"] += bool(counts) and med < min_depth
        over = bool(counts) and med >= min_depth and med > target
        res["records_over"] += over
        res["records_thinned"] += over and not kept
    res["out"] = b"".join(res["out"])
    return res
