"""FASTQ mode on the GPU (mk_set_fastq): raw FASTQ counted exactly as find_kmers counts the text MerCat2's fq2fa makes
of it (lib/mercat2_fasta.py:175-198), and the CLI's -skipclean FASTQ path built on it."""
import gzip
import hashlib
import json
import os
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN
from mercat2_amd import cli, native
from mercat2_amd.harness import run_raw_fastq, run_text
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

FQ = json.loads((GOLDEN / "fastq.json").read_text())
EXPECTED = json.loads((GOLDEN / "expected.json").read_text())
KS = (3, 21, 31, 33, 63)


def _r1() -> bytes:
    return gzip.open(GOLDEN / "inputs" / "Test_R1.fastq.gz", "rb").read()


def _digest(ctx, base):
    kmers, counts = ctx.export()
    k = ctx.k
    flat = kmers.tobytes().decode("ascii")
    text = "k-mer\t%s_Count\n" % base + "".join("%s\t%d\n" % (flat[i * k:(i + 1) * k], int(c)) for i, c in enumerate(counts))
    return {"rows": int(counts.size), "sum": int(counts.sum()), "sha256": hashlib.sha256(text.encode()).hexdigest()}


def _count_fastq(ctx, raw: bytes, c: int) -> dict:
    ctx.reset()
    ctx.count_chunk(raw, c)
    return ctx.to_dict()


def _fuzz_set():
    """Seeded FASTQ-like texts: records with quirks (CRLF, lone CR, blank lines, '>' / '@' / blanks at line starts,
    '*', N, missing or extra lines), several of them longer than one 4 KiB tile of the pre-pass."""
    rng = random.Random(7)
    out = []
    for i in range(160):
        recs = []
        for _ in range(rng.randrange(1, 12 if i < 120 else 160)):
            n = rng.randrange(0, 180)
            seq = "".join(rng.choice("ACGT" if rng.random() < 0.9 else "ACGTN*acgt >\r") for _ in range(n))
            head = rng.choice(["@r%d x" % i, "@r", " @r", "r", ">r", "@", ""])
            plus = rng.choice(["+", "+r", "@+", ">", ""])
            qual = "".join(rng.choice("I#@>+ ") for _ in range(n))
            lines = [head, seq, plus, qual]
            if rng.random() < 0.1:
                lines.insert(rng.randrange(0, 4), "")
            if rng.random() < 0.05:
                lines.pop(rng.randrange(0, len(lines)))
            recs.append(lines)
        nl = rng.choice(["\n", "\n", "\r\n"])
        text = nl.join(l for r in recs for l in r)
        if rng.random() < 0.7:
            text += nl
        out.append(text.encode())
    return out


def test_test_r1_raw_fastq_matches_the_reference_tables():
    raw = _r1()
    for k in (3, 5, 21, 31):
        with native.Counter(k) as ctx:
            ctx.set_fastq(True)
            for c in (1, 10):
                ctx.reset()
                ctx.count_chunk(raw, c)
                want = EXPECTED["Test_R1.fna.gz|k%d|c%d" % (k, c)]   # made by the reference's own find_kmers
                assert _digest(ctx, "Test_R1") == {x: want[x] for x in ("rows", "sum", "sha256")}, (k, c)


def test_edge_cases_and_fuzz_equal_the_oracle_on_the_converted_text():
    cases = []
    for name, case in FQ["edge"].items():
        raw = case["text"].encode()
        conv, _ = native.fq2fa(raw)
        assert hashlib.sha256(conv).hexdigest() == case["sha256"], name  # the sed pipeline's text (make_fastq_golden.py)
        cases.append((name, raw, conv))
    cases += [("fuzz%d" % i, raw, native.fq2fa(raw)[0]) for i, raw in enumerate(_fuzz_set())]
    for k in KS:
        with native.Counter(k) as ctx:
            ctx.set_fastq(True)
            for name, raw, conv in cases:
                for c in ((1, 2) if name.startswith("fuzz") and len(raw) > 4096 else (1,)):
                    assert _count_fastq(ctx, raw, c) == cpu_ref.count_text(conv, k, c), (name, k, c)


def test_canonical_fastq_mode():
    cases = [_r1()] + [raw for raw in _fuzz_set()[100:]]
    for k in (3, 21, 31, 33, 63):
        with native.Counter(k, canonical=True) as ctx:
            ctx.set_fastq(True)
            for raw in cases:
                conv, _ = native.fq2fa(raw)
                assert _count_fastq(ctx, raw, 1) == cpu_ref.canonical_fold(cpu_ref.count_text(conv, k, 1)), k


def test_fastq_stats_equal_the_host_conversion():
    cases = [_r1()] + [c["text"].encode() for c in FQ["edge"].values()] + _fuzz_set()[::7]
    with native.Counter(21) as ctx:
        ctx.set_fastq(True)
        for raw in cases:
            ctx.reset()
            assert ctx.fastq_stats() == {"lines": 0, "reads": 0, "headers_dropped": 0, "fasta_bytes": 0, "crlf": 0}
            ctx.count_chunk(raw, 1)
            assert ctx.fastq_stats() == native.fq2fa(raw)[1], raw[:200]
        # summed over the chunks since the reset, every chunk a file of its own
        ctx.reset()
        a, b = cases[0], cases[-1]
        ctx.count_chunk(a, 1)
        ctx.count_chunk(b, 1)
        sa, sb = native.fq2fa(a)[1], native.fq2fa(b)[1]
        assert ctx.fastq_stats() == {n: sa[n] + sb[n] for n in sa}


def _synth_fastq(reads: int, seed: int) -> bytes:
    fa = native.synth_reads(2_000_000, seed, reads, 150, seed + 1).tobytes()
    lines = fa.split(b"\n")[:-1]
    rng = np.random.default_rng(seed)
    qual = rng.integers(33, 75, size=(reads, 150), dtype=np.uint8)
    out = []
    for i in range(reads):
        out.append(b"@" + lines[2 * i][1:] + b" 1:N:0:ACGTACGT+TTGACCAA sample=%d" % (i % 97))
        out.append(lines[2 * i + 1])
        out.append(b"+")
        out.append(qual[i].tobytes())
    return b"\n".join(out) + b"\n"


def test_a_million_reads_equal_the_c_oracle():
    from oracle import c_oracle
    raw = _synth_fastq(1_000_000, 11)
    conv, st = native.fq2fa(raw)
    assert st["reads"] == 1_000_000
    with native.Counter(31) as ctx:
        ctx.set_fastq(True)
        ctx.count_chunk(raw, 2)
        kmers, counts = ctx.export()
        assert ctx.fastq_stats() == st
    wk, wc = c_oracle.count(conv, 31, 2)
    assert np.array_equal(kmers, wk) and np.array_equal(counts, wc)


def test_mode_rules():
    with native.Counter(21) as ctx:
        ctx.set_clean(True)
        with pytest.raises(native.MercatHipError) as e:
            ctx.set_fastq(True)
        assert e.value.code == -1
        ctx.set_clean(False)
        ctx.set_fastq(True)
        with pytest.raises(native.MercatHipError) as e:
            ctx.set_clean(True)
        assert e.value.code == -1
    with native.Counter(5, native.ALPHABET_AA5) as ctx:
        with pytest.raises(native.MercatHipError) as e:
            ctx.set_fastq(True)
        assert e.value.code == -1


def test_caller_memory_is_refused_and_reset_keeps_the_mode(tmp_path):
    import torch
    raw = b"@r\nACGTACGTAC\n+\n@@@@>>>>II\n"
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with native.Counter(5) as ctx:
        ctx.set_fastq(True)
        with pytest.raises(native.MercatHipError) as e:
            ctx.count_device(buf.data_ptr(), len(raw), 1)
        assert e.value.code == -4
        src = tmp_path / "r.fq"
        src.write_bytes(raw)
        with pytest.raises(native.MercatHipError) as e:
            native.count_file([ctx], src, 0, 1)
        assert e.value.code == -4
        ctx.reset()
        ctx.count_chunk(raw, 1)   # still FASTQ: the quality line is not counted
        assert ctx.to_dict() == cpu_ref.count_text(b">r\nACGTACGTAC\n", 5, 1)


def test_a_pooled_context_counts_fasta_after_fastq(tmp_path):
    from mercat2_amd import harness
    harness.release_pool()
    raw = _r1()
    fa = gzip.open(GOLDEN / "inputs" / "Test_R1.fna.gz", "rb").read()
    assert run_raw_fastq("Test_R1", raw, tmp_path / "a.tsv", 5, 10, 100 << 20, report=lambda l: None) is not None
    assert (tmp_path / "a.tsv").read_text() == cpu_ref.tsv_text("Test_R1", cpu_ref.count_text(fa, 5, 10))
    assert len(harness._POOL.get((5, native.ALPHABET_NT2, 0, False), [])) == 1   # the context went back to the pool
    other = (GOLDEN / "inputs" / "A.fasta").read_bytes()
    run_text("A", other, tmp_path / "b.tsv", 5, 1, alphabet=native.ALPHABET_NT2, report=lambda l: None)
    assert (tmp_path / "b.tsv").read_text() == cpu_ref.tsv_text("A", cpu_ref.count_text(other, 5, 1))


@pytest.mark.parametrize("name", ["Test_R1.fastq.gz", "Test_R1.fastq"])
def test_cli_counts_fastq_with_skipclean(tmp_path, capsys, name):
    src = tmp_path / name
    if name.endswith(".gz"):
        shutil.copy(GOLDEN / "inputs" / name, src)
    else:
        src.write_bytes(_r1())
    out = tmp_path / "res"
    assert cli.main(["-i", str(src), "-k", "5", "-skipclean", "-o", str(out)]) == 0
    assert "Significant k-mers: 642" in capsys.readouterr().out
    assert (out / "tsv_nucleotide" / "Test_R1_counts.tsv").read_text() == (GOLDEN / "tsv" / "ref_Test_R1_k5_c10.tsv").read_text()
    # the reference's rows; only the first header field differs (the release that made that run wrote 'kmer', the
    # current source writes the TSVs' own 'k-mer': tests/test_gpu_report.py)
    got = (out / "combined_Nucleotide.tsv").read_text().splitlines()
    ref = (GOLDEN / "report" / "Test_R1_combined_Nucleotide.tsv").read_text().splitlines()
    assert got[0] == "k-mer\tTest_R1" and ref[0] == "kmer\tTest_R1"
    assert got[1:] == ref[1:] and len(got) == 643
    assert gzip.open(out / "clean" / "Test_R1.fna.gz", "rb").read() == gzip.open(GOLDEN / "inputs" / "Test_R1.fna.gz", "rb").read()


def test_cli_folder_mixing_fastq_and_fasta(tmp_path):
    folder = tmp_path / "in"
    folder.mkdir()
    shutil.copy(GOLDEN / "inputs" / "Test_R1.fastq.gz", folder / "Test_R1.fastq.gz")
    (folder / "reads2.fq").write_bytes(FQ["edge"]["crlf"]["text"].encode() * 40)
    shutil.copy(GOLDEN / "inputs" / "A.fasta", folder / "A.fasta")
    shutil.copy(GOLDEN / "inputs" / "RW1.fna.gz", folder / "RW1.fna.gz")
    out = tmp_path / "res"
    assert cli.main(["-f", str(folder), "-k", "4", "-c", "3", "-n", "4", "-skipclean", "-o", str(out)]) == 0
    for fname, base in [("Test_R1.fastq.gz", "Test_R1"), ("reads2.fq", "reads2"), ("A.fasta", "A"), ("RW1.fna.gz", "RW1")]:
        data = (gzip.open if fname.endswith(".gz") else open)(folder / fname, "rb").read()
        if fname.endswith((".fq", ".fastq", ".fastq.gz")):
            data, _ = native.fq2fa(data)
            assert gzip.open(out / "clean" / f"{base}.fna.gz", "rb").read() == data
        assert (out / "tsv_nucleotide" / f"{base}_counts.tsv").read_text() == cpu_ref.tsv_text(base, cpu_ref.count_text(data, 4, 3)), fname
    assert sorted(os.listdir(out / "clean")) == ["Test_R1.fna.gz", "reads2.fna.gz"]


def _cli_s1(tmp_path, raw: bytes, name: str, k: int, c: int):
    src = tmp_path / name
    src.write_bytes(raw)
    out = tmp_path / ("res_" + name)
    assert cli.main(["-i", str(src), "-k", str(k), "-c", str(c), "-s", "1", "-skipclean", "-o", str(out), "-debug"]) == 0
    conv, _ = native.fq2fa(raw)
    gz = out / "clean" / "big.fna.gz"
    assert gzip.open(gz, "rb").read() == conv
    chunked = os.stat(gz).st_size >= (1 << 20)
    want = cpu_ref.count_sample_text(conv, k, c, 1) if chunked else cpu_ref.count_text(conv, k, c)
    tsv = out / "tsv_nucleotide" / "big_counts.tsv"
    assert (tsv.read_text() if tsv.exists() else "") == (cpu_ref.tsv_text("big", want) if want else "")
    return chunked


def test_cli_fastq_chunked_by_its_fna_gz(tmp_path):
    raw = _synth_fastq(40_000, 21)   # ~6 M bases: the .gz passes 1 MiB
    assert _cli_s1(tmp_path, raw, "big.fastq", 11, 2) is True


def test_cli_fastq_near_the_limit_counts_both_candidates(tmp_path):
    # converted text just above 1 MiB: its .gz (a quarter of it) decides "whole" only when it is complete
    raw = _synth_fastq(6_000, 31)
    assert 1 << 20 < len(native.fq2fa(raw)[0]) < 2 << 20
    assert _cli_s1(tmp_path, raw, "big.fq", 11, 2) is False


def test_cli_still_refuses_fastq_without_skipclean(tmp_path):
    fq = tmp_path / "reads.fastq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    with pytest.raises(SystemExit) as e:
        cli.main(["-i", str(fq), "-k", "5", "-o", str(tmp_path / "y")])
    assert "-skipclean" in str(e.value)
