"""The flat parse lane (mk_fparse.hip mk_fparse_flat, mk_chunk.hip process_chunk_fast): read files -- one header line
and one sequence line per record -- are packed at their raw-text positions by one kernel; anything else is refused and
parsed again by the three-kernel parser.  Every text is counted with the lane on and with MK_FP_FLAT=0, k = 21 and 31,
c = 1 unless stated.  Each case checks (a) the table against oracle.cpu_ref.count_text, (b) table, symbols and
windows of the two arms against each other, (c) flat_chunks / flat_refused / parse_retries.

One lane is 16 bytes, one sub-step 1 KiB, one wave 8 KiB, one workgroup 32 KiB; a wave takes its entry state from
the 1 KiB of text in front of it (WINDOW).  The texts assert that they place what they claim."""
import numpy as np
import pytest

import text_edges as te
from mercat2_amd import native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

LANE, SUB, W, WG = te.FAST_UNITS
WINDOW = SUB
KS = (21, 31)
EDGES = (LANE * 37, 3 * SUB, W, WG)  # a lane edge inside a sub-step, a sub-step edge inside a wave, a wave edge, a workgroup edge
STAT_KEYS = ("symbols", "windows", "flat_chunks", "flat_refused", "parse_retries", "exotic_windows", "fused_chunks")


# ----------------------------------------------------------------------------- the texts
def read(i: int, seed: int, n: int = 100, head: bytes = None, nl: bytes = b"\n") -> bytes:
    return (b">r%d" % i if head is None else head) + nl + te.bases(n, seed * 1009 + i) + nl


def grow(text: bytes, target: int, seed: int) -> bytes:
    """text and whole 100-base reads behind it, exactly `target` bytes: the last header line is as long as it takes."""
    out, size, i = [text], len(text), 0
    assert target - size >= 120
    while target - size > 240:
        out.append(read(i, seed))
        size += len(out[-1])
        i += 1
    out.append(read(i, seed, head=b">" + b"p" * (target - size - 103)))
    text = b"".join(out)
    assert len(text) == target
    return text


PLACES = {
    # name -> (bytes in front of the edge, what is planted there)
    "inside-header": (20, lambda s: b">" + te.header_filler(49) + b"\n" + te.bases(100, s) + b"\n"),
    "inside-sequence": (60, lambda s: b">s\n" + te.bases(100, s) + b"\n"),
    "on-gt": (0, lambda s: b">g\n" + te.bases(100, s) + b"\n"),
    "behind-line-end": (10, lambda s: b">h2345678\n" + te.bases(100, s) + b"\n"),
}


def edge_text(place: str, begin: int = 0) -> bytes:
    """Reads with the construct of PLACES[place] at every edge of EDGES, as a kernel sees them that reads the text
    `begin` bytes behind a 16-byte boundary."""
    front, plant = PLACES[place]
    text = b""
    for n, edge in enumerate(EDGES):
        text = grow(text, edge - begin - front, 10 * n + 1) + plant(50 + n)
    text += b"".join(read(i, 77) for i in range(12))
    b, nl, hstart, in_header, _ = te._line_classes(text)
    for edge in EDGES:
        at = edge - begin  # the unit's first byte
        if place == "inside-header":
            assert in_header[at - 1] and in_header[at] and not hstart[at]
        elif place == "inside-sequence":
            assert text[at - 1] in b"ACGT" and text[at] in b"ACGT"
        elif place == "on-gt":
            assert hstart[at] and nl[at - 1]
        else:
            assert nl[at - 1] and in_header[at - 2] and text[at] in b"ACGT"
    assert len(text) < 40 * 1024
    return text


def plain(nbytes: int, seed: int) -> bytes:
    return b"".join(read(i, seed) for i in range(nbytes // 107 + 1))


def two_line(seed: int, first: int = 60) -> bytes:
    return b">two\n" + te.bases(first, seed) + b"\n" + te.bases(60, seed + 1) + b"\n"


# ----------------------------------------------------------------------------- counting both ways
@pytest.fixture(scope="module")
def ctxs():
    made = {k: native.Counter(k, native.ALPHABET_NT2) for k in KS}
    yield made
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def device_buf():
    import torch
    return torch.zeros(64 * 1024 + 64, dtype=torch.uint8, device="cuda")


def count_once(ctx, chunks, flat, monkeypatch, c=1, device=None):
    """(table, stats) of the chunks counted into the context from empty (after a reset: the lane is tried afresh)."""
    monkeypatch.setenv("MK_FP_FLAT", "1" if flat else "0")
    ctx.reset()
    before = ctx.stats()
    for text in chunks:
        if device is None:
            ctx.count_chunk(text, c)
        else:
            import torch
            buf, begin = device
            buf[:16] = ord(">")  # garbage in front of the chunk, inside its first 16-byte piece
            buf[begin:begin + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            assert buf.data_ptr() % 16 == 0
            ctx.count_device(buf.data_ptr() + begin, len(text), c)
    table = ctx.to_dict()
    after = ctx.stats()
    return table, {key: after[key] - before[key] for key in STAT_KEYS}


def both_arms(ctx, chunks, monkeypatch, flat_chunks, flat_refused, retries=0, c=1, want=None, device=None, label=None):
    """(a), (b), (c) for one context.  Returns the stats of the flat arm."""
    if isinstance(chunks, bytes):
        chunks = [chunks]
    if want is None:
        want = cpu_ref.merge_counts(cpu_ref.count_text(text, ctx.k, c) for text in chunks)
    got, stats = count_once(ctx, chunks, True, monkeypatch, c, device)
    got_off, stats_off = count_once(ctx, chunks, False, monkeypatch, c, device)
    print(label, ctx.k, "flat", stats, "MK_FP_FLAT=0", stats_off)
    assert got == want, (label, ctx.k, "flat arm differs from the oracle")
    assert got_off == want, (label, ctx.k, "MK_FP_FLAT=0 arm differs from the oracle")
    assert (stats["symbols"], stats["windows"]) == (stats_off["symbols"], stats_off["windows"]), (label, ctx.k)
    assert (stats["flat_chunks"], stats["flat_refused"]) == (flat_chunks, flat_refused), (label, ctx.k, stats)
    assert (stats_off["flat_chunks"], stats_off["flat_refused"]) == (0, 0), (label, ctx.k, stats_off)
    assert stats["parse_retries"] == retries and stats_off["parse_retries"] == retries, (label, ctx.k)
    return stats


def accepted(ctxs, text, monkeypatch, **kw):
    return [both_arms(ctxs[k], text, monkeypatch, 1, 0, **kw) for k in KS]


def refused(ctxs, text, monkeypatch, **kw):
    return [both_arms(ctxs[k], text, monkeypatch, 0, 1, **kw) for k in KS]


# ----------------------------------------------------------------------------- accepted texts
@pytest.mark.parametrize("place", list(PLACES))
def test_reads_on_every_edge(ctxs, monkeypatch, place):
    """A lane, a sub-step, a wave and a workgroup begin inside a header line, inside a sequence line, exactly on a '>'
    and exactly behind a header's line end."""
    accepted(ctxs, edge_text(place), monkeypatch, label=place)


@pytest.mark.parametrize("begin", [1, 7, 15])
def test_unaligned_device_pointer(ctxs, monkeypatch, device_buf, begin):
    """The chunk `begin` bytes behind a 16-byte boundary of device memory: the packed positions count from that boundary.
    Lengths one off a multiple of 16 bytes, of 1 KiB and of 8 KiB as the kernel sees them."""
    whole = edge_text("inside-header", begin)
    for n in (LANE * 601 - begin - 1, SUB * 11 - begin + 1, W * 2 - begin - 1, W * 2 - begin, len(whole)):
        accepted(ctxs, whole[:n], monkeypatch, device=(device_buf, begin), label=(begin, n))


ENDS = {
    "no-last-line-end": lambda: plain(3 * W, 3)[:-1],
    "bare-header-last": lambda: plain(3 * W, 4) + b">last header, no line end",
    "gt-alone": lambda: plain(W - 300, 5) + b">\n" + te.bases(100, 6) + b"\n" + plain(W, 7),
    "quirky-headers": lambda: b"".join(read(i, 8, head=b">a%d >b *c\td  e" % i) for i in range(3 * W // 120)),
    "crlf": lambda: b"".join(read(i, 9, nl=b"\r\n") for i in range(3 * W // 109)),
    "empty-line-between-records": lambda: b"".join(read(i, 10) + (b"\n" if i % 3 == 0 else b"") for i in range(3 * W // 108)),
    "empty-line-behind-header": lambda: b"".join(read(i, 11, head=b">e%d\n" % i if i % 3 == 0 else None) for i in range(3 * W // 108)),
}


@pytest.mark.parametrize("name", list(ENDS))
def test_line_shapes_the_lane_takes(ctxs, monkeypatch, name):
    text = ENDS[name]()
    assert 3 * 1024 <= len(text) <= 40 * 1024 and not te.takes_general_parser(text)
    if name == "no-last-line-end":
        assert text[-1] in b"ACGT"
    if name == "bare-header-last":
        assert te._line_classes(text)[3][-1]
    if name == "gt-alone":
        assert b"\n>\n" in text
    if name == "quirky-headers":
        assert text.count(b" >b *c\t") > 100
    if name == "crlf":
        assert text.count(b"\r\n") == 2 * text.count(b">") and text.count(b"\n") == text.count(b"\r\n")
    if name == "empty-line-between-records":
        assert text.count(b"\n\n>") > 50
    if name == "empty-line-behind-header":
        assert text.count(b"\n\nA") + text.count(b"\n\nC") + text.count(b"\n\nG") + text.count(b"\n\nT") > 50
    accepted(ctxs, text, monkeypatch, label=name)


# ----------------------------------------------------------------------------- refused texts
def _two_line_cases():
    body = plain(3 * W + 2000, 20)
    at = body.index(b">r5\n")
    first = body[:at] + two_line(21) + body[at:]
    last = body + two_line(22) + plain(300, 23)
    seam = grow(b"", 2 * W - 5 - 61, 24) + two_line(25) + plain(W, 26)  # '>two\n' + 60 bases + '\n': the line end is byte 2 W - 1
    return {"first-wave": first, "last-wave": last, "line-ends-on-wave-end": seam}


@pytest.mark.parametrize("name", ["first-wave", "last-wave", "line-ends-on-wave-end"])
def test_two_line_record_is_refused(ctxs, monkeypatch, name):
    text = _two_line_cases()[name]
    at = text.index(b">two\n")
    if name == "first-wave":
        assert text[at - 1] == 10 and at + 130 < SUB
    if name == "last-wave":
        assert at // W == (len(text) - 1) // W and at // W >= 3
    if name == "line-ends-on-wave-end":
        assert text[2 * W - 1] == 10 and text[2 * W - 2] in b"ACGT" and text[2 * W] in b"ACGT"
    refused(ctxs, text, monkeypatch, label=name)


def test_star_inside_a_sequence_is_refused(ctxs, monkeypatch):
    text = bytearray(plain(3 * W, 30))
    at = next(j for j in range(W + 2000, W + 2300) if all(text[i] in b"ACGT" for i in range(j - 3, j + 4)))
    text[at] = ord("*")
    refused(ctxs, bytes(text), monkeypatch)
    # ('*' as the last or the first byte of a sequence line breaks no run: the lane takes it)
    text = bytearray(plain(3 * W, 31))
    at = next(j for j in range(W + 2000, W + 2300) if text[j + 1] == 10 and text[j + 2] == ord(">"))
    text[at] = ord("*")
    at = next(j for j in range(2 * W, 2 * W + 300) if text[j - 1] == 10 and text[j] in b"ACGT")
    text[at] = ord("*")
    accepted(ctxs, bytes(text), monkeypatch, label="star at line ends")


@pytest.mark.parametrize("where", ["front-of-a-wave", "inside-a-wave"])
@pytest.mark.parametrize("what", ["header", "sequence"])
def test_line_longer_than_the_window_is_refused(ctxs, monkeypatch, what, where):
    """A header line, and a one-line record, longer than WINDOW bytes.  Covering the WINDOW bytes in front of wave 2, the
    wave finds no header-line start to take its state from; inside a wave it leaves a whole sub-step without one, which
    is refused all the same: whether a text is taken does not hang on where its lines fall against the waves."""
    long = (b">" + te.header_filler(WINDOW + 200) + b"\n" + te.bases(100, 40) + b"\n") if what == "header" else \
        (b">long\n" + te.bases(WINDOW + 200, 41) + b"\n")
    at = 2 * W - WINDOW - 100 if where == "front-of-a-wave" else 2 * W + SUB - 100
    text = grow(b"", at, 42) + long + plain(W, 43)
    hstart = te._line_classes(text)[2]
    assert hstart[at] and not hstart[at + 100:at + 100 + WINDOW].any() and (at + 100) % SUB == 0
    assert (at + 100 + WINDOW) % W == (0 if where == "front-of-a-wave" else 2 * SUB)
    refused(ctxs, text, monkeypatch, label=(what, where))
    # (the longest line that leaves no sub-step without a header-line start however it falls: SUB bytes with its line end)
    text = grow(b"", at + 50, 44) + b">" + te.header_filler(SUB - 103) + b"\n" + te.bases(100, 45) + b"\n" + plain(W, 46)
    hstart = np.flatnonzero(te._line_classes(text)[2])
    assert np.diff(hstart).max() == SUB
    accepted(ctxs, text, monkeypatch, label=(what, where, "record of one sub-step"))


def test_wrapped_fasta_tries_the_lane_once_per_sample(ctxs, monkeypatch):
    """Three chunks of wrapped FASTA in one context: the first is refused, the others do not try; after reset() the lane
    is tried again."""
    chunks = [te.records(5000, 50 + i) for i in range(3)]
    assert all(not te.takes_general_parser(x) for x in chunks)
    for k in KS:
        ctx = ctxs[k]
        both_arms(ctx, chunks, monkeypatch, 0, 1, label="wrapped")
        monkeypatch.setenv("MK_FP_FLAT", "1")
        ctx.reset()
        before = ctx.stats()
        ctx.count_chunk(chunks[0], 1)
        ctx.count_chunk(chunks[1], 1)
        mid = ctx.stats()
        ctx.reset()
        ctx.count_chunk(chunks[2], 1)
        ctx.count_chunk(plain(5000, 53), 1)
        after = ctx.stats()
        assert mid["flat_refused"] - before["flat_refused"] == 1 and after["flat_refused"] - mid["flat_refused"] == 1
        assert after["flat_chunks"] == before["flat_chunks"] and after["chunks"] - before["chunks"] == 4


# ----------------------------------------------------------------------------- other cases
def test_blank_inside_a_sequence_line_takes_the_general_lane(ctxs, monkeypatch):
    text = bytearray(plain(3 * W, 60))
    at = next(j for j in range(W + 100, W + 400) if all(text[i] in b"ACGT" for i in (j - 1, j, j + 1)))
    text[at] = 32
    text = bytes(text)
    assert te.takes_general_parser(text)
    for k in KS:
        both_arms(ctxs[k], text, monkeypatch, 0, 0, retries=1)


def test_reads_with_n(ctxs, monkeypatch):
    """Symbols outside the alphabet: the second parse rewrites stream, packed words and bitmap densely for the
    by-reference kernel; packed rows and rows kept as text are the oracle's."""
    text = bytearray(edge_text("inside-sequence"))
    for at in (700, W - 3, W + 2000, WG + 5):
        at = next(j for j in range(at, at + 300) if text[j] in b"ACGT" and text[j - 1] in b"ACGT")
        text[at] = ord("N")
    text = bytes(text)
    stats = both_arms(ctxs[31], text, monkeypatch, 1, 0)
    assert stats["exotic_windows"] > 0
    table = cpu_ref.count_text(text, 31, 1)
    assert any("N" in key for key in table) and any("N" not in key for key in table)


def test_fused_upsert_leaves_a_refused_chunk_out(ctxs, monkeypatch):
    """min_count 2: the second chunk's count kernel upserts into the running table itself; that chunk holds a two-line
    record near its end, so its flat launch is refused -- nothing of that launch is in the table."""
    one = plain(2 * W, 70)
    first = one + one + plain(W, 71)
    second = one + plain(W, 72) + one + two_line(73) + two_line(73) + plain(200, 74)
    for k in KS:
        want = cpu_ref.merge_counts([cpu_ref.count_text(first, k, 2), cpu_ref.count_text(second, k, 2)])
        assert want and max(want.values()) >= 4
        stats = both_arms(ctxs[k], [first, second], monkeypatch, 1, 1, c=2, want=want, label="fused")
        assert stats["fused_chunks"] >= 1, stats


def test_two_word_keys_and_canonical(monkeypatch):
    """k = 63 (two-word keys) and canonical counting read the same flat layout."""
    take, refuse = edge_text("inside-header"), _two_line_cases()["line-ends-on-wave-end"]
    with native.Counter(63, native.ALPHABET_NT2) as ctx:
        both_arms(ctx, take, monkeypatch, 1, 0, label="k63")
        both_arms(ctx, refuse, monkeypatch, 0, 1, label="k63 refused")
    with native.Counter(31, native.ALPHABET_NT2, canonical=True) as ctx:
        for text, chunks_, refused_ in ((take, 1, 0), (refuse, 0, 1)):
            want = cpu_ref.canonical_fold(cpu_ref.count_text(text, 31, 1))
            both_arms(ctx, text, monkeypatch, chunks_, refused_, want=want, label="canonical")


def test_header_share_guard(monkeypatch):
    """The lane is decided per sample from the symbols per raw byte of the last full chunk (at least 1 MiB): a context
    that knows nothing tries it; MK_FP_FLAT_SHARE moves the threshold."""
    text = plain((1 << 20) + 5000, 90)
    share = 100 * text.count(b">") / len(text)
    assert 0.90 < share < 0.96
    want = cpu_ref.count_text(text, 21, 1)
    monkeypatch.setenv("MK_FP_FLAT", "1")
    with native.Counter(21, native.ALPHABET_NT2) as ctx:
        seen = []
        for threshold in ("0.99", "0.99", None, "0.5"):
            if threshold is None:
                monkeypatch.delenv("MK_FP_FLAT_SHARE", raising=False)
            else:
                monkeypatch.setenv("MK_FP_FLAT_SHARE", threshold)
            ctx.reset()
            ctx.count_chunk(text, 1)
            assert ctx.to_dict() == want, threshold
            seen.append(ctx.stats()["flat_chunks"])
        assert seen == [1, 1, 2, 3] and ctx.stats()["flat_refused"] == 0, seen
