#!/usr/bin/env python3
"""Golden vectors of the FASTQ path (MerCat2's fq2fa, lib/mercat2_fasta.py:175-198).

Run only in the build container, where /root/reference is mounted and GNU sed is installed:

    python tests/golden/make_fastq_golden.py

It copies two data files of the reference and records what the reference's own conversion -- `sed -n
'1~4s/^@/>/p;2~4p'` read back in universal-newline text mode -- makes of them and of synthetic edge cases.  Nothing
of the reference's source text is stored.  The GPU box has no /root/reference: tests read only what this script
committed.

Outputs
  inputs/Test_R1.fastq.gz                 data/Test_R1.fastq.gz (the reads of results/2023-11-29/test-qc*)
  report/Test_R1_combined_Nucleotide.tsv  results/2023-11-29/test-qc_gz/combined_Nucleotide.tsv (-k 5 -c 10)
  fastq.json                              sha256 of both copies and of the converted text of Test_R1; the edge cases
                                          {name: {"text": FASTQ text, "sha256": of the sed pipeline's text, "bytes"}}
"""
import gzip
import hashlib
import io
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent

REC = "@a x\nACGTACGTAC\n+\nIIIIIIIIII\n"
EDGE = {
    "header_space_at": REC + " @r\nGGGGCCCCAA\n+\nIIIIIIIIII\n" + REC,
    "header_no_at": REC + "r\nGGGGCCCCAA\n+\nIIIIIIIIII\n" + REC,
    "seq_gt": "@a\n>ACGTACGT\n+\nIIIIIIIII\n@b\nACGTTTGACC\n+\nIIIIIIIIII\n",
    "seq_space_gt": "@a\n >x ACGTAC\n+\nIIIIIIIIII\n@b\nACGTTTGACC\n+\nIIIIIIIIII\n",
    "plus_qual_at_gt": "@a\nACGTACGTAA\n@plus\n>qual\n@b\nACGTTTACGT\n+\n@@@@@@@@@@\n@c\nGGGACGTACC\n>\n>>>>>>>>>>\n",
    "crlf": "@a x\r\nACGTACGTAC\r\n+\r\nIIIIIIIIII\r\n@b\r\nGGCCATACGT\r\n+\r\nIIIIIIIIII\r\n",
    "crlf_no_final_nl": "@a x\r\nACGTACGTAC\r\n+\r\nIIIIIIIIII\r\n@b\r\nGGCCATACGT\r",
    "lone_cr": "@a\nACGTA\rCGTACG\n+\nIIIIIIIIIII\n@b\rACGTTT\nCCGGTAACGT\n+\nIIIIIIIIII\n",
    "empty_lines": "@a\nACGTACGT\n\n+\nIIIIIIII\n@b\nACGTACGT\n+\nIIIIIIII\n\n@c\nGGGGACGT\n+\nIIIIIIII\n",
    "empty_line_first": "\n@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGTACGT\n+\nIIIIIIII\n",
    "one_line": "@a",
    "one_line_nl": "@a\n",
    "two_lines": "@a\nACGTACGTAC",
    "three_lines": "@a\nACGTACGTAC\n+",
    "empty": "",
    "no_final_nl_0": REC + "@b",
    "no_final_nl_1": REC + "@b\nACGTTTACGA",
    "no_final_nl_2": REC + "@b\nACGTTTACGA\n+",
    "no_final_nl_3": REC + "@b\nACGTTTACGA\n+\nIIIIIIIIII",
    "star": "@a\nAC*GTAC**GTACGT\n+\nIIIIIIIIIIIIIII\n@b\n*ACGTACGT*\n+\nIIIIIIIIII\n",
    "ns_kept": "@a\nACGTNNACGTACGTN\n+\nIIIIIIIIIIIIIII\n",
    "lower_case": "@a\nacgtACGTacgtAC\n+\nIIIIIIIIIIIIII\n",
}


def sed_fq2fa(data: bytes) -> bytes:
    """The reference's conversion: sed's output read back as text (universal newlines), written out as UTF-8."""
    out = subprocess.run(["sed", "-n", "1~4s/^@/>/p;2~4p"], input=data, stdout=subprocess.PIPE, check=True,
                         env=dict(os.environ, LC_ALL="C")).stdout
    return io.TextIOWrapper(io.BytesIO(out), encoding="utf-8", newline=None).read().encode("utf-8")


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def main() -> None:
    src = REF / "data" / "Test_R1.fastq.gz"
    shutil.copyfile(src, HERE / "inputs" / "Test_R1.fastq.gz")
    tsv = REF / "results" / "2023-11-29" / "test-qc_gz" / "combined_Nucleotide.tsv"
    shutil.copyfile(tsv, HERE / "report" / "Test_R1_combined_Nucleotide.tsv")
    fq = gzip.open(src, "rb").read()
    assert fq == (REF / "data" / "Test_R1.fastq").read_bytes()
    conv = sed_fq2fa(fq)
    # the reference's own converted file of that run (already a fixture: inputs/Test_R1.fna.gz)
    assert conv == gzip.open(REF / "results" / "2023-11-29" / "test-qc_gz" / "clean" / "Test_R1.fna.gz", "rb").read()
    doc = {
        "Test_R1.fastq.gz": {"sha256": sha((HERE / "inputs" / "Test_R1.fastq.gz").read_bytes()), "text_sha256": sha(fq),
                             "fasta_sha256": sha(conv), "fasta_bytes": len(conv)},
        "Test_R1_combined_Nucleotide.tsv": {"sha256": sha(tsv.read_bytes()), "k": 5, "c": 10},
        "edge": {},
    }
    for name, text in EDGE.items():
        out = sed_fq2fa(text.encode())
        doc["edge"][name] = {"text": text, "sha256": sha(out), "bytes": len(out)}
    (HERE / "fastq.json").write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print("wrote", HERE / "fastq.json")


if __name__ == "__main__":
    main()
