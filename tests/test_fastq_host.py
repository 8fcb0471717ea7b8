"""FASTQ input on the host (no GPU): mk_fq2fa against MerCat2's own conversion -- fq2fa's `sed -n
'1~4s/^@/>/p;2~4p'` pipeline read back in universal-newline text mode (lib/mercat2_fasta.py:175-198), run live --
and the layers above it (fasta.fq2fa, the CLI's classify)."""
import gzip
import hashlib
import io
import json
import os
import random
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

from conftest import GOLDEN
from mercat2_amd import cli, fasta, native

FQ = json.loads((GOLDEN / "fastq.json").read_text())
needs_sed = pytest.mark.skipif(shutil.which("sed") is None, reason="the reference pipeline needs sed")


def sed_fq2fa(data: bytes) -> bytes:
    out = subprocess.run(["sed", "-n", "1~4s/^@/>/p;2~4p"], input=data, stdout=subprocess.PIPE, check=True,
                         env=dict(os.environ, LC_ALL="C")).stdout
    return io.TextIOWrapper(io.BytesIO(out), encoding="utf-8", newline=None).read().encode("utf-8")


def stats_of(data: bytes) -> dict:
    """The conversion's figures, restated line by line."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    reads = dropped = crlf = 0
    for i, line in enumerate(lines):
        ph = i % 4
        if ph == 0:
            if line.startswith(b"@"):
                reads += 1
            else:
                dropped += 1
                continue
        elif ph != 1:
            continue
        last = i == len(lines) - 1 and not data.endswith(b"\n")
        crlf += line.endswith(b"\r") and not last
    return {"lines": len(lines), "reads": reads, "headers_dropped": dropped, "crlf": crlf}


def _r1():
    return gzip.open(GOLDEN / "inputs" / "Test_R1.fastq.gz", "rb").read()


def test_fixtures_are_the_recorded_copies():
    assert hashlib.sha256((GOLDEN / "inputs" / "Test_R1.fastq.gz").read_bytes()).hexdigest() == FQ["Test_R1.fastq.gz"]["sha256"]
    tsv = GOLDEN / "report" / "Test_R1_combined_Nucleotide.tsv"
    assert hashlib.sha256(tsv.read_bytes()).hexdigest() == FQ["Test_R1_combined_Nucleotide.tsv"]["sha256"]


def test_test_r1_converts_to_the_references_fna():
    text, st = native.fq2fa(_r1())
    assert text == gzip.open(GOLDEN / "inputs" / "Test_R1.fna.gz", "rb").read()  # the reference's clean/Test_R1.fna.gz
    assert hashlib.sha256(text).hexdigest() == FQ["Test_R1.fastq.gz"]["fasta_sha256"]
    assert st == {"lines": 1000, "reads": 250, "headers_dropped": 0, "fasta_bytes": len(text), "crlf": 0}


@needs_sed
def test_test_r1_matches_the_sed_pipeline():
    raw = _r1()
    assert native.fq2fa(raw)[0] == sed_fq2fa(raw)


def test_edge_cases_match_the_recorded_sed_output():
    assert len(FQ["edge"]) >= 20
    for name, case in FQ["edge"].items():
        raw = case["text"].encode()
        text, st = native.fq2fa(raw)
        assert hashlib.sha256(text).hexdigest() == case["sha256"], name
        assert st == dict(stats_of(raw), fasta_bytes=len(text)), name


@needs_sed
def test_edge_cases_match_the_sed_pipeline_live():
    for name, case in FQ["edge"].items():
        raw = case["text"].encode()
        assert native.fq2fa(raw)[0] == sed_fq2fa(raw), name


@needs_sed
def test_random_texts_match_the_sed_pipeline():
    rng = random.Random(20261015)
    alphabet = b"@>+ACGTN* \r\n"
    for i in range(2000):
        n = rng.randrange(0, 80)
        raw = bytes(rng.choice(alphabet) for _ in range(n))
        text, st = native.fq2fa(raw)
        assert text == sed_fq2fa(raw), raw
        assert st == dict(stats_of(raw), fasta_bytes=len(text)), raw


def test_non_ascii_follows_the_fasta_rule():
    ok, _ = native.fq2fa("@r é\nACGT\n+\nééII\n".encode())  # header line and dropped lines: passed / dropped
    assert ok == "@r é\nACGT\n".replace("@", ">").encode()
    with pytest.raises(native.NonAsciiInput):
        native.fq2fa("@r\nACéGT\n+\nIIIII\n".encode())
    # a kept sequence line that starts with '>' is a header of the converted text
    assert native.fq2fa("@r\n>é\n+\nII\n".encode())[0] == ">r\n>é\n".encode()


def _wt_size(path: Path, text: bytes) -> int:
    """What the reference's writer leaves: gzip.open(p, 'wt') fed line by line (the member is named after the file)."""
    path.parent.mkdir(parents=True, exist_ok=True)
    with gzip.open(path, "wt") as w:
        for line in io.TextIOWrapper(io.BytesIO(text), encoding="utf-8", newline=None):
            w.write(line)
    return os.stat(path).st_size


@pytest.mark.parametrize("name", ["Test_R1.fastq.gz", "Test_R1.fastq"])
def test_fasta_fq2fa_writes_the_fna_gz(tmp_path, name):
    src = tmp_path / name
    if name.endswith(".gz"):
        shutil.copy(GOLDEN / "inputs" / name, src)
    else:
        src.write_bytes(_r1())
    path = fasta.fq2fa(str(src), str(tmp_path / "clean"), "Test_R1")
    assert path == os.path.abspath(tmp_path / "clean" / "Test_R1.fna.gz")
    text = gzip.open(path, "rb").read()
    assert text == native.fq2fa(_r1())[0]
    assert os.stat(path).st_size == _wt_size(tmp_path / "ref" / "Test_R1.fna.gz", text)


def test_fq2fa_background_holds_the_text_and_writes_the_file(tmp_path):
    raw = _r1()
    with ThreadPoolExecutor(1) as ex:
        path, fut, holder = fasta.fq2fa_background(Path("Test_R1.fastq.gz"), raw, tmp_path / "clean", "Test_R1", ex, limit=1 << 20)
        size, st = fut.result()
    assert path == (tmp_path / "clean" / "Test_R1.fna.gz").absolute()
    assert holder["ready"].is_set() and holder["decision"].wait() is False
    assert holder["text"] == gzip.open(path, "rb").read() == native.fq2fa(raw)[0]
    assert size == os.stat(path).st_size and st["reads"] == 250


def test_classify_takes_fastq_with_skipclean():
    for name, base in [("a.fq", "a"), ("a.fastq", "a"), ("s.R1.fq.gz", "s.R1"), ("Test_R1.fastq.gz", "Test_R1")]:
        assert cli.classify(Path(name), True) == ("nucleotide", base)
        with pytest.raises(SystemExit) as e:
            cli.classify(Path(name))
        assert "-skipclean" in str(e.value)
    assert cli.classify(Path("x.fna.gz")) == ("nucleotide", "x")
    assert cli.classify(Path("x.faa"), True) == ("protein", "x")
    assert cli.classify(Path("x.txt"), True) == (None, None)
