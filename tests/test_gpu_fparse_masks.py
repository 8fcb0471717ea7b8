"""The fast parser's emit pass on the masks the summary pass stored (mk_fparse.hip): every text is counted with the
stored masks (MK_FP_CLASSIC=0) and with every mask computed again (MK_FP_CLASSIC=1), k = 21 and k = 31, c = 1.  Each
case checks (a) the table against oracle.cpu_ref.count_text, (b) table and stats of the two arms against each other,
(c) the parse_retries expected.

One wave is 8 KiB, one sub-step 1 KiB, one lane 16 bytes.  What decides the path of a wave is restated here from the
text (wave_facts): its entry state (the byte before it lies in a header line) and `conv`, the number of leading
sub-steps up to the one that holds the wave's first line end; the texts assert that they place what they claim."""
import numpy as np
import pytest

import text_edges as te
from mercat2_amd import native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

W, SUB = te.FAST_WAVE, te.FAST_UNITS[1]
KS = (21, 31)
STAT_KEYS = ("symbols", "records", "windows", "parse_retries")


# ----------------------------------------------------------------------------- the texts
def reads(nbytes: int, seed: int, tag: bytes = b"r") -> bytes:
    """Exactly nbytes of records '>tagN' + one line of 100 bases; the last line is as long as it takes and ends the text
    with a line end."""
    assert nbytes >= 16
    out, size, i = [], 0, 0
    while nbytes - size > 240:
        out.append(b">%s%d\n" % (tag, i) + te.bases(100, seed * 1009 + i) + b"\n")
        size += len(out[-1])
        i += 1
    head = b">%s%d\n" % (tag, i)
    out.append(head + te.bases(nbytes - size - len(head) - 1, seed * 1009 + i) + b"\n")
    return b"".join(out)


def plain_reads(nbytes: int, seed: int) -> bytes:
    """About nbytes of 100-base reads; a record whose successor's header line would reach a multiple of 8 KiB gets a
    longer header line, so that every wave starts inside a sequence line."""
    out, size, i = [], 0, 0
    while size < nbytes:
        head = b">p%d\n" % i
        nxt = size + len(head) + 101
        if nxt % W > W - 32 or nxt % W == 0:
            head = b">p%d %s\n" % (i, b"x" * 40)
        out.append(head + te.bases(100, seed * 1013 + i) + b"\n")
        size += len(out[-1])
        i += 1
    return b"".join(out)


def header_at(front: int, length: int, seed: int, tail: int = 3000, filler=None, after: bytes = b"") -> bytes:
    """`front` bytes of reads, a header line of `length` bytes and its line end, `after`, then `tail` bytes of reads."""
    body = (filler or (lambda n: b"h" * n))(length - 1)
    return reads(front, seed) + b">" + body + b"\n" + after + reads(tail, seed + 1, b"t")


def wave_facts(text: bytes, begin: int = 0) -> list:
    """(entry state, conv) of every wave of the text placed `begin` bytes behind a 16-byte boundary."""
    b, nl, _, in_header, _ = te._line_classes(text)
    out = []
    for start in range(0, begin + len(text), W):
        at = start - begin  # the wave's first byte, as an index into the text
        state = int(at > 0 and bool(in_header[at - 1]))
        ends = np.flatnonzero(nl[max(at, 0):at + W]) + max(at, 0) - at
        out.append((state, min(int(ends[0]) // SUB + 1, W // SUB) if len(ends) else W // SUB))
    return out


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


def count_once(ctx, text, classic, monkeypatch, device=None):
    """(table, stats) of the text counted from empty.  It is counted twice and the second count is the one returned: how
    the scatter cuts a chunk into records follows what the chunk before it listed (mk_ctx::items_hint), so `records`
    compares only between counts that follow the same text."""
    monkeypatch.setenv("MK_FP_CLASSIC", "1" if classic else "0")
    if device is not None:
        import torch
        buf, begin = device
        buf[:16] = ord(">")  # garbage in front of the chunk, inside its first 16-byte piece
        buf[begin:begin + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0
    for turn in ("primes the hints", "counts"):
        ctx.reset()
        before = ctx.stats()
        if device is None:
            ctx.count_chunk(text, 1)
        else:
            ctx.count_device(buf.data_ptr() + begin, len(text), 1)
        table = ctx.to_dict()
        after = ctx.stats()
        stats = {key: after[key] - before[key] for key in STAT_KEYS + ("exotic_windows",)}
        print("   ", "classic" if classic else "masks", turn, stats)
    return table, stats


def both_arms(ctxs, text, retries, monkeypatch, device=None, label=None):
    """(a), (b), (c) for k = 21 and 31; retries: the expected parse_retries, or None for 'at least one'.  Returns the
    stats of the masks arm per k."""
    seen = {}
    for k in KS:
        want = cpu_ref.count_text(text, k, 1)
        got, stats = count_once(ctxs[k], text, False, monkeypatch, device)
        got_c, stats_c = count_once(ctxs[k], text, True, monkeypatch, device)
        print(label, k, "masks", stats, "classic", stats_c)
        assert got == want, (label, k, "masks arm differs from the oracle")
        assert got_c == want, (label, k, "classic arm differs from the oracle")
        assert stats == stats_c, (label, k)
        if retries is None:
            assert stats["parse_retries"] >= 1, (label, k)
        else:
            assert stats["parse_retries"] == retries, (label, k)
        seen[k] = stats
    return seen


# ----------------------------------------------------------------------------- the cases
def test_plain_reads(ctxs, monkeypatch):
    """Every wave starts in a sequence line: stored masks throughout."""
    text = plain_reads(5 * W - 100, 1)
    facts = wave_facts(text)
    assert len(facts) == 5 and all(state == 0 for state, _ in facts)
    both_arms(ctxs, text, 0, monkeypatch)


@pytest.mark.parametrize("over", [1, 15, 16, 17, SUB, SUB + 1])
def test_header_across_a_wave_start(ctxs, monkeypatch, over):
    """`over` bytes of a header line (its line end the last of them) lie in wave 2: 1, 15, 16, 17 (a lane seam), the whole
    of sub-step 0, and one byte of sub-step 1."""
    text = header_at(2 * W - 30, 30 + over - 1, 2, tail=2 * W)
    assert text[2 * W + over - 1] == 10 and text[2 * W - 30] == ord(">")
    facts = wave_facts(text)
    assert len(facts) in (4, 5) and facts[2] == (1, 2 if over > SUB else 1) and facts[1][0] == 0
    both_arms(ctxs, text, 0, monkeypatch, label=over)


@pytest.mark.parametrize("length,convs", [(SUB + 1, [2]), (3 * SUB, [3]), (3 * SUB + 1, [4]), (W, [8]), (20 * SUB, [8, 8, 4])],
                         ids=["1k+1", "3k", "3k+1", "8k", "20k"])
def test_long_headers(ctxs, monkeypatch, length, convs):
    """A header line of `length` bytes (line end not counted) that starts one byte in front of wave 1: its line end is
    byte length - 1 of that wave.  8 KiB: a whole wave inside the header line but for its last byte; 20 KiB: two waves
    in a row without a line end.  (Starting in front of the wave, a line of 3 KiB ends in sub-step 2 at the latest,
    conv = 3; one byte more gives 4.)"""
    text = header_at(W - 1, length, 3, tail=W + 500)
    facts = wave_facts(text)
    assert 3 <= len(facts) <= 6 and [f for f in facts if f[0]] == [(1, c) for c in convs], facts
    both_arms(ctxs, text, 0, monkeypatch, label=length)


@pytest.mark.parametrize("over", [12, 40, SUB + 300])
def test_blanks_in_header_lines_across_a_wave_start(ctxs, monkeypatch, over):
    """Blanks and tabs in a header line on both sides of a wave start: under entry state 0 -- the one the stored masks
    assume -- those behind it look like blanks in sequence text.  The fast parser keeps the chunk."""
    text = header_at(W - 200, 200 + over - 1, 4, tail=2 * W, filler=te.header_filler) + b">z a\tb\n" + te.bases(80, 5) + b"\n"
    b = np.frombuffer(text, dtype=np.uint8)
    assert (b[W - 200:W] <= 0x20).any() and (b[W:W + over - 1] <= 0x20).any() and text[W + over - 1] == 10
    facts = wave_facts(text)
    assert facts[1] == (1, (over - 1) // SUB + 1) and not te.takes_general_parser(text)
    both_arms(ctxs, text, 0, monkeypatch, label=over)


@pytest.mark.parametrize("where", ["wave0", "same-sub-step", "later-sub-step"])
def test_blank_in_a_sequence_line(ctxs, monkeypatch, where):
    """A blank inside a sequence line: in wave 0; in a wave entered inside a header line, behind its first line end in
    the same sub-step (computed again by the emit pass) and in a later one (the summary pass's word for it)."""
    text = bytearray(header_at(W - 50, 50 + 199, 6, tail=2 * W, filler=te.header_filler))
    assert wave_facts(bytes(text))[1] == (1, 1) and text[W + 199] == 10
    at = {"wave0": 300, "same-sub-step": W + 200 + 60, "later-sub-step": W + 3 * SUB + 10}[where]
    at = next(j for j in range(at, at + 300) if all(text[i] in b"ACGT" for i in (j - 1, j, j + 1)))
    text[at] = 32
    text = bytes(text)
    assert te.takes_general_parser(text) and (at < W or at // SUB == W // SUB + (0 if where == "same-sub-step" else 3))
    both_arms(ctxs, text, None, monkeypatch, label=where)


ODD_TOTAL = 4 * W + 40
ODD = {
    "star": lambda: te.planted("star", 5, SUB, ODD_TOTAL),
    "crlf": lambda: te.planted("crlf", -1, SUB, ODD_TOTAL),
    "crlf-header": lambda: te.planted("crlf_header", -2, SUB, ODD_TOTAL),
    "empty-lines": lambda: te.planted("lf3", -1, SUB, ODD_TOTAL),
    "gt-mid-line": lambda: te.planted("gt_inner", 3, SUB, ODD_TOTAL),
    "ends-without-newline": lambda: header_at(W - 9, 40, 7, tail=2 * W)[:-1],
    "ends-in-header": lambda: header_at(W - 9, 40, 8, tail=2 * W) + b">cut " + b"h" * (W + 77),
}


@pytest.mark.parametrize("name", list(ODD))
def test_odd_line_shapes(ctxs, monkeypatch, name):
    text = ODD[name]()
    assert 3 * W <= len(text) <= 6 * W and not te.takes_general_parser(text)
    if name == "ends-without-newline":
        assert text[-1] in b"ACGT"
    if name == "ends-in-header":
        assert wave_facts(text)[-1] == (1, 8)
    both_arms(ctxs, text, 0, monkeypatch, label=name)


LENGTHS = (16 * 1601 - 1, 16 * 1601 + 1, SUB * 27 - 1, SUB * 27 + 1, W * 4 - 1, W * 4 + 1)


@pytest.mark.parametrize("begin", [1, 7, 15])
def test_unaligned_starts_and_lengths(ctxs, monkeypatch, device_buf, begin):
    """The chunk `begin` bytes behind a 16-byte boundary of device memory; lengths one off a multiple of 16 bytes, of
    1 KiB and of 8 KiB; a header line with blanks across the second wave start as the kernel sees it."""
    whole = header_at(W - begin - 20, 20 + 36, 9, tail=4 * W, filler=te.header_filler)
    for n in LENGTHS:
        text = whole[:n]
        assert wave_facts(text, begin)[1] == (1, 1)
        both_arms(ctxs, text, 0, monkeypatch, device=(device_buf, begin), label=(begin, n))


def test_bytes_from_0x80_on(ctxs, monkeypatch):
    """In a header line (one across a wave start, one inside a wave) they mean nothing; in a sequence line the chunk is
    refused (refuse_non_ascii, mk_chunk.hip) whichever way the masks come about, and the context stays usable."""
    accent = "café 中文 ".encode("utf-8")
    text = header_at(W - 60, 60 + 30, 10, tail=2 * W, filler=lambda n: accent * (n // len(accent)) + b"x" * (n % len(accent)),
                     after=b">q " + accent + b"\n" + te.bases(90, 11) + b"\n")
    assert wave_facts(text)[1] == (1, 1) and max(text[W - 60:W]) >= 0x80 and max(text[W:W + 29]) >= 0x80
    both_arms(ctxs, text, 0, monkeypatch)
    for at in (500, 2 * W + 4000):  # wave 0; a wave without header bytes >= 0x80
        at = next(j for j in range(at, at + 300) if all(text[i] in b"ACGT" for i in (j - 1, j, j + 1, j + 2)))
        bad = text[:at] + "é".encode("utf-8") + text[at + 2:]
        for k in KS:
            for classic in (False, True):
                monkeypatch.setenv("MK_FP_CLASSIC", "1" if classic else "0")
                ctxs[k].reset()
                with pytest.raises(native.NonAsciiInput):
                    ctxs[k].count_chunk(bad, 1)
                ctxs[k].reset()
                ctxs[k].count_chunk(b">r\n" + te.bases(40, 12) + b"\n", 1)
                assert ctxs[k].to_dict() == cpu_ref.count_text(b">r\n" + te.bases(40, 12) + b"\n", k, 1)


def test_by_reference_second_parse(ctxs, monkeypatch):
    """An N in a read: the chunk is parsed a second time with the stream written, for the by-reference kernel."""
    text = bytearray(header_at(W - 12, 12 + 99, 13, tail=2 * W, filler=te.header_filler))
    for at in (700, W + 2000, 2 * W + 5):
        at = next(j for j in range(at, at + 300) if text[j] in b"ACGT" and text[j - 1] in b"ACGT")
        text[at] = ord("N")
    text = bytes(text)
    assert wave_facts(text)[1] == (1, 1)
    seen = both_arms(ctxs, text, 0, monkeypatch)
    assert all(stats["exotic_windows"] > 0 for stats in seen.values()), "the by-reference re-parse did not run"
