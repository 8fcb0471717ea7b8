"""The text kernels at their lane, wave, tile and scan seams (tests/text_edges.py makes the texts; DESIGN section 7 lists
the seams): the fast parser with its fused pack, the general parser it falls back to, the FASTQ pre-pass and the clean
passes, each against the C oracle (clean mode: the removeN restatement, then the find_kmers restatement), exactly.
Everything is counted with c = 1, so that every window shows.  Every sweep asserts which parser ran."""
import numpy as np
import pytest

import text_edges as te
from mercat2_amd import native
from oracle import c_oracle, clean_ref, cpu_ref

pytestmark = pytest.mark.gpu

NT2, AA5, RAW = native.ALPHABET_NT2, native.ALPHABET_AA5, native.ALPHABET_RAW


@pytest.fixture(scope="module")
def ctx_of():
    """One context per (k, alphabet, mode), made when first asked for; callers reset() it between texts."""
    made = {}

    def get(k, alphabet=NT2, mode=None, toupper=False):
        key = (k, alphabet, mode, toupper)
        if key not in made:
            ctx = native.Counter(k, alphabet)
            if mode == "fastq":
                ctx.set_fastq(True)
            elif mode == "clean":
                ctx.set_clean(True, toupper)
            made[key] = ctx
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


def counted(ctx, text, retries, feed=None, label=None):
    """The table of one text, counted from empty; the parser that ran is the one the text was built for."""
    ctx.reset()
    before = ctx.stats()
    (feed or (lambda: ctx.count_chunk(text, 1)))()
    after = ctx.stats()
    assert after["parse_retries"] - before["parse_retries"] == retries, ("the other parser ran", label)
    return {"exotic": after["exotic_windows"] - before["exotic_windows"]}


class DeviceText:
    """A text placed in device memory at a chosen misalignment, garbage in front of it (test_count_device_unaligned_offsets)."""

    def __init__(self, cap):
        import torch
        self.torch = torch
        self.buf = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")

    def feed(self, ctx, text, off):
        torch = self.torch
        self.buf[:16] = ord(">")
        self.buf[off:off + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        return lambda: ctx.count_device(self.buf.data_ptr() + off, len(text), 1)


@pytest.fixture(scope="module")
def device_text():
    return DeviceText(64 * 1024)


def host_and_device(ctx, text, want, retries, device_text, label):
    """Fed from the host, then from device memory 1 and 15 bytes past a 16-byte boundary."""
    counted(ctx, text, retries)
    assert ctx.to_dict() == want, (label, "host")
    for off in (1, 15):
        counted(ctx, text, retries, device_text.feed(ctx, text, off))
        assert ctx.to_dict() == want, (label, "device + %d" % off)


# ----------------------------------------------------------------------------- fast parser sweep
FAST_CONFIGS = {"nt2-k31": (NT2, 31),    # fused pack, the parsed stream is not written
                "nt2-k40": (NT2, 40),    # two-word keys
                "aa5-k5": (AA5, 5),      # stream written, mk_pack_aa_* with its 16- and 4-byte loads
                "raw-k9": (RAW, 9)}      # every window by reference


@pytest.mark.parametrize("feature", list(te.FEATURES))
@pytest.mark.parametrize("config", list(FAST_CONFIGS))
def test_fast_parser_feature_on_every_seam(ctx_of, config, feature):
    """A feature at B + shift for every multiple B of 1 KiB in 96 KiB (every lane, sub-step, wave and workgroup seam of
    mk_fparse.hip is among them; shifts +-16 are lane seams alone)."""
    alphabet, k = FAST_CONFIGS[config]
    ctx = ctx_of(k, alphabet)
    for shift in te.SHIFTS:
        text = te.planted(feature, shift, te.FAST_UNITS[1])
        seen = counted(ctx, text, 0)
        assert ctx.to_dict() == c_oracle.count_dict(text, k, 1), (config, feature, shift)
        if alphabet == NT2 and feature in te.BYREF_FEATURES:
            assert seen["exotic"] > 0, "the by-reference re-parse did not run"


# ----------------------------------------------------------------------------- residues, byte values, ends
@pytest.mark.parametrize("e", te.RESIDUES_E)
def test_emit_pass_output_residues(ctx_of, device_text, e):
    """The wave-end output offset at every residue mod 64, a wave that emits nothing, one that emits e bytes."""
    ctx = ctx_of(31)
    for r in te.RESIDUES_R:
        text = te.residue_text(r, e)
        host_and_device(ctx, text, c_oracle.count_dict(text, 31, 1), 0, device_text, (r, e))


@pytest.mark.parametrize("inner_blank", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("k", [5, 11, 31, 33])
def test_every_byte_value_through_both_packers(ctx_of, device_text, k, inner_blank):
    """Every sequence byte 0x21..0x7E through the fused pack's v_perm comparison (fast parser) and through mk_pack_nt's four
    equality tests (one inner blank: general parser, then mk_pack_nt)."""
    text = te.all_bytes_text(inner_blank)
    host_and_device(ctx_of(k), text, c_oracle.count_dict(text, k, 1), int(inner_blank), device_text, (k, inner_blank))


@pytest.mark.parametrize("seam", te.FAST_UNITS)
def test_text_ends_at_a_seam(ctx_of, device_text, seam):
    """Texts of seam - 1, seam and seam + 1 bytes that end in a sequence line (with and without a newline) and in a header."""
    texts = te.end_texts((seam,))
    assert len(texts) == 9
    for k in (5, 31):
        for name, text in texts.items():
            host_and_device(ctx_of(k), text, c_oracle.count_dict(text, k, 1), 0, device_text, (k, name))


# ----------------------------------------------------------------------------- general parser sweep
GENERAL_CONFIGS = {"nt2-k31": (NT2, 31), "aa5-k5": (AA5, 5)}


@pytest.mark.parametrize("feature", list(te.FEATURES))
@pytest.mark.parametrize("config", list(GENERAL_CONFIGS))
def test_general_parser_feature_on_every_seam(ctx_of, config, feature):
    """The planted texts at multiples of 2 KiB (every thread, wave and tile seam of mk_parse.hip) with one inner blank in
    the first sequence line: the fast parser stands back, once."""
    alphabet, k = GENERAL_CONFIGS[config]
    ctx = ctx_of(k, alphabet)
    for shift in te.SHIFTS:
        text = te.with_inner_blank(te.planted(feature, shift, te.GENERAL_UNITS[1]))
        counted(ctx, text, 1)
        assert ctx.to_dict() == c_oracle.count_dict(text, k, 1), (config, feature, shift)


@pytest.mark.parametrize("after", te.BLANK_AFTER)
@pytest.mark.parametrize("unit", te.GENERAL_UNITS)
def test_blank_runs_across_general_parser_seams(ctx_of, unit, after):
    """Runs of 1..4096 blanks inside a sequence line across a 32-byte, 2 KiB and 8 KiB seam: kept when a base follows
    (blank_is_inner looks across the seam), trimmed in front of the line end and at the end of the text."""
    ctx = ctx_of(31)
    for run in te.BLANK_RUNS:
        text = te.blank_run_text(run, unit, after)
        counted(ctx, text, 1)
        assert ctx.to_dict() == c_oracle.count_dict(text, 31, 1), (unit, run, after)


# ----------------------------------------------------------------------------- carry and scan regimes
@pytest.mark.parametrize("name", ["540k-fast", "540k-general", "9m-fast", "9m-general"])
def test_long_header_lines_carry_across_scan_words(ctx_of, name):
    """Header lines of 20 KiB .. 1.2 MiB: the 'inside a header line' carry crosses ballot words of mk_fparse_scan while
    set (540 KiB: one wave per scan thread; 9 MiB: two, the loops over more than one entry per thread in both parsers'
    scans), with irregular records, CRLF, '*' and 'N' around them."""
    text, retries, _ = te.long_carry_texts()[name]
    ctx = ctx_of(31)
    counted(ctx, text, retries)
    kmers, counts = ctx.export()
    want_k, want_c = c_oracle.count(text, 31, 1)
    assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)


# ----------------------------------------------------------------------------- FASTQ
def fastq_counted(ctx, raw, label):
    """One FASTQ text counted from empty; returns the converted text.  Which parser ran follows from the CONVERTED text:
    a blank outside its header lines (a planted line end may cut an '@q7 d' line in two, a drifting line number may keep
    a quality line) sends the chunk to the general parser, once; without one the fast parser does it all."""
    conv, stats = te.fq_ref(raw)
    counted(ctx, raw, int(te.takes_general_parser(conv)), label=label)
    assert ctx.fastq_stats() == stats, label
    return conv


def fastq_check(ctx, raw, k, label):
    conv = fastq_counted(ctx, raw, label)
    assert ctx.to_dict() == c_oracle.count_dict(conv, k, 1), label


@pytest.mark.parametrize("name", te.FASTQ_NAMES)
def test_fastq_named_seam_cases(ctx_of, name):
    fastq_check(ctx_of(31, NT2, "fastq"), te.fastq_texts()[name], 31, name)


@pytest.mark.parametrize("feature", list(te.FEATURES))
@pytest.mark.parametrize("k", [31, 5])
def test_fastq_feature_on_every_tile_seam(ctx_of, k, feature):
    """The features at B + shift for every multiple B of the pre-pass's 4 KiB tile, on irregular FASTQ records: whatever
    they do to the line numbering, the table and the figures are those of the converted text."""
    ctx = ctx_of(k, NT2, "fastq")
    for shift in te.SHIFTS:
        fastq_check(ctx, te.fastq_planted(feature, shift), k, (feature, shift))


def test_fastq_more_tiles_than_scan_threads_and_apply_workgroups(ctx_of):
    """9 MiB: the scan's threads take three tiles each, the apply pass's workgroups a second tile (the other s_last parity)."""
    ctx = ctx_of(31, NT2, "fastq")
    conv = fastq_counted(ctx, te.fastq_big(), "big")
    kmers, counts = ctx.export()
    want_k, want_c = c_oracle.count(conv, 31, 1)
    assert np.array_equal(kmers, want_k) and np.array_equal(counts, want_c)


# ----------------------------------------------------------------------------- clean mode
@pytest.mark.parametrize("toupper", [False, True], ids=["asis", "toupper"])
@pytest.mark.parametrize("name", te.CLEAN_NAMES)
def test_clean_mode_runs_at_stream_seams(ctx_of, name, toupper):
    """N runs of 1, 2 and 40 bytes that start and end at parsed-stream offsets = 15, 0, 1 mod 16 ("runs"), and that start
    at -1, 0, 1 and 16 bytes from every multiple of 1 KiB of the raw text (the others): the table of the cleaned text, and
    the runs where split_sequenceN cuts (test_runs_are_where_split_sequenceN_cuts)."""
    raw = te.clean_texts()[name]
    cleaned = clean_ref.clean_text(raw.decode(), toupper)[0]
    stream, _ = te.parse_stream(raw)
    first = stream.find(bytes([te.SEP]))
    stream = stream[first:] if first >= 0 else b""   # text in front of the first header line is dropped
    runs = te.stream_runs(stream)                    # runs of upper-case N (a lower-case n is no cut, -toupper or not)
    headers = stream.count(bytes([te.SEP]))
    gc = sum(stream.count(ch) for ch in ((b"G", b"C", b"g", b"c") if toupper else (b"G", b"C")))
    assert headers >= 1 and len(runs) >= (18 if name == "runs" else 23) and len(cleaned) > len(raw) // 2  # (nothing here is empty)
    for k in (5, 31):
        ctx = ctx_of(k, NT2, "clean", toupper)
        ctx.reset()
        ctx.count_chunk(raw, 1)
        assert ctx.to_dict() == cpu_ref.count_text(cleaned.encode(), k, 1), (name, k)
        st = ctx.clean_stats()
        starts, ends = ctx.clean_runs()
        assert list(zip(starts.tolist(), ends.tolist())) == runs, (name, k)
        n_bytes = sum(b - a for a, b in runs)
        assert st["n_runs"] == len(runs) and st["n_bytes"] == n_bytes and st["header_lines"] == headers, (name, k)
        assert st["symbols"] == len(stream) - headers - n_bytes and st["gc_count"] == gc, (name, k)
        assert st["n_runs"] == sum(1 for ln in cleaned.split("\n") if ln.startswith(">")) - headers
