"""Drop-in for MerCat2's ``mercat2_kmers`` module (lib/mercat2_kmers.py).

``find_kmers(file, kmer, min_count)`` keeps the reference's signature and result (a dict
``{kmer_string: count}`` holding the k-mers whose count in THIS file is >= min_count,
lib/mercat2_kmers.py:32-78) but counts on the GPU through libmercat_hip.so.
"""
from __future__ import annotations

import gzip
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

from . import native

PROTEIN_SUFFIXES = (".faa", ".faa.gz")


def read_fasta_bytes(file: Union[str, Path]) -> bytes:
    """Raw (decompressed) bytes of a FASTA; gzip iff the last suffix is '.gz', exactly the
    reference's test (lib/mercat2_kmers.py:47)."""
    p = Path(file)
    if p.suffix == ".gz":
        with gzip.open(p, "rb") as fh:
            return fh.read()
    return p.read_bytes()


def read_head(file: Union[str, Path], n: int = 4096) -> bytes:
    """The first ``n`` (decompressed) bytes of a FASTA, to pick the alphabet from."""
    p = Path(file)
    with (gzip.open(p, "rb") if p.suffix == ".gz" else open(p, "rb")) as fh:
        return fh.read(n)


def map_fasta(file: Union[str, Path]):
    """Buffer over the (decompressed) bytes of a FASTA without an extra copy where possible:
    plain files are memory-mapped (the engine copies straight from the page cache to the GPU),
    '.gz' files are inflated into memory.  Returns an object supporting the buffer protocol."""
    import mmap
    p = Path(file)
    if p.suffix == ".gz":
        return read_fasta_bytes(p)
    size = p.stat().st_size
    if size == 0:
        return b""
    with open(p, "rb") as fh:
        return mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)


def guess_alphabet(file: Union[str, Path], data: Optional[bytes] = None) -> int:
    """Pick the packed fast path. Correctness never depends on it: characters outside the
    chosen alphabet are still counted exactly (by the by-reference kernel)."""
    name = str(file).lower()
    if name.endswith(PROTEIN_SUFFIXES):
        return native.ALPHABET_AA5
    if data is not None and len(data):
        # chunk files written by the Chunker lose the '.gz' but keep '.faa'; anything else:
        # sniff the first sequence lines
        seq = b"".join(l for l in bytes(data[:4096]).splitlines() if l and not l.startswith(b">"))
        if seq:
            acgt = sum(seq.count(c) for c in (b"A", b"C", b"G", b"T", b"N", b"a", b"c", b"g", b"t", b"n"))
            if acgt < 0.9 * len(seq):
                return native.ALPHABET_AA5
    return native.ALPHABET_NT2


def calculateKmerCount(seq: str, kmer: int, device: int = 0) -> Dict[str, int]:
    """Reference helper of the same name (lib/mercat2_kmers.py:10-28): all k-mers of ONE
    sequence string, no filter.  The string is counted as it stands (no stripping, '*' kept),
    so it is fed as a single-line record and must not hold characters the FASTA parser acts on."""
    data = seq.encode("ascii")
    if data != data.strip() or any(c in data for c in b"\r\n*") or data.startswith(b">"):
        raise ValueError("calculateKmerCount: sequence holds FASTA control characters")
    with native.Counter(kmer, guess_alphabet("", b">s\n" + data), device) as ctx:
        ctx.count_chunk(b">s\n" + data + b"\n", 0)
        return ctx.to_dict()


def find_kmers(file: Path, kmer: int, min_count: int, *, device: int = 0, alphabet: Optional[int] = None) -> Dict[str, int]:
    """Calculates the k-mer count in a fasta file (same contract as the reference).

    Parameters:
        file (Path): path to a fasta file (plain or .gz) to scan for k-mers.
        kmer (int): k-mer length.
        min_count (int): minimum count of k-mers found to be considered significant.

    Returns:
        dict: {k-mer string: count} for every k-mer with count >= min_count in this file.
    """
    if alphabet is None:
        alphabet = guess_alphabet(file, read_head(file))
    with native.Counter(kmer, alphabet, device) as ctx:
        native.count_file([ctx], file, 0, min_count)  # the whole file is one chunk
        return ctx.to_dict()


def lookup_kmers(table: "native.Counter", kmers) -> Dict[str, int]:
    """{k-mer: count} of the given k-mers (str, each of the table's k) in a table that is still on the GPU -- 0 for a
    k-mer it lacks -- without exporting it: what ``find_kmers(...)[kmer]`` answers, for a handful of keys."""
    kmers = list(kmers)
    return dict(zip(kmers, table.lookup(kmers).tolist()))


FASTQ_SUFFIXES = (".fq", ".fastq", ".fq.gz", ".fastq.gz")
_BLANKS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"  # what str.strip() removes from ASCII text


def record_names(text: bytes) -> List[str]:
    """The names of a FASTA text's records, in order, as the screen calls number them: a record per header line -- a
    line whose first non-blank character is '>', find_kmers' test after line.strip() (lib/mercat2_kmers.py:51-52) --
    named by the first word behind the '>' ("" for none), and a leading "" when sequence stands in front of the first
    header line.  Lines end at "\n", "\r\n" or a lone "\r", as text mode reads them."""
    names: List[str] = []
    headless = False
    for line in bytes(text).splitlines():
        line = line.strip(_BLANKS)
        if line.startswith(b">"):
            words = line[1:].decode("utf-8", "replace").split()
            names.append(words[0] if words else "")
        elif not names and not headless and line.replace(b"*", b""):
            headless = True
    return ([""] if headless else []) + names


def record_lengths(text: bytes) -> List[int]:
    """The kept characters of every record of a FASTA text, numbered as ``record_names`` numbers them: what find_kmers
    joins of the record's lines (line.strip(), '*' removed)."""
    lengths: List[int] = []
    headless = 0
    for line in bytes(text).replace(b"\r\n", b"\n").replace(b"\r", b"\n").split(b"\n"):
        line = line.strip(_BLANKS)
        if line.startswith(b">"):
            lengths.append(0)
        elif lengths:
            lengths[-1] += len(line) - line.count(b"*")
        else:
            headless += len(line) - line.count(b"*")
    return ([headless] if headless else []) + lengths


def screen_reads(table: "native.Counter", file: Union[str, Path], at_least: int = 1) -> Tuple[List[str], "native.np.ndarray"]:
    """(names, array) of every record of a FASTA or FASTQ file screened against a table that is still on the GPU
    (Counter.screen): array[i] = (windows, hits, sum, min, max) of record i -- its k-mers, how many of them the table
    holds ``at_least`` times, and the sum, smallest and largest of their counts.  A '.gz' file is inflated on the host;
    a FASTQ file ('.fq' / '.fastq', plain or '.gz') is first converted as MerCat2's fq2fa converts it (mk_fq2fa).  A
    canonical table folds the windows."""
    text = read_fasta_bytes(file)
    if str(file).lower().endswith(FASTQ_SUFFIXES):
        text, _ = native.fq2fa(text)
    names = record_names(text)
    rows = table.screen(text, at_least)
    if len(names) != rows.shape[0]:
        raise RuntimeError("screen_reads: %d header names for %d records" % (len(names), rows.shape[0]))
    return names, rows


def track_reads(table: "native.Counter", file: Union[str, Path], at_least: int = 1, sat32: bool = False, median: bool = True):
    """(names, counts, offsets, rows, median) of every record of a FASTA or FASTQ file tracked against a table that is
    still on the GPU (Counter.track): counts[offsets[i] : offsets[i + 1]] are the counts of record i's k-mers in the order
    they stand in the read (0 for one the table lacks), rows[i] its screen row (windows, hits, sum, min, max) and
    median[i] element windows // 2 of its sorted counts -- khmer's median k-mer abundance -- or None without ``median``.
    ``sat32``: uint32 counts clipped at 2^32 - 1, half the bytes.  The file is read exactly as screen_reads reads it:
    '.gz' inflated on the host, a FASTQ file first converted as MerCat2's fq2fa converts it (mk_fq2fa).  A canonical
    table folds the windows."""
    text = read_fasta_bytes(file)
    if str(file).lower().endswith(FASTQ_SUFFIXES):
        text, _ = native.fq2fa(text)
    names = record_names(text)
    counts, offsets, rows, med = table.track(text, at_least, sat32=sat32, median=median)
    if len(names) != rows.shape[0]:
        raise RuntimeError("track_reads: %d header names for %d records" % (len(names), rows.shape[0]))
    return names, counts, offsets, rows, med


def orf_names(text: bytes) -> List[bytes]:
    """The names of a FASTA text's records as Counter.orfs writes them in front of an ORF's coordinates: per header line
    (``record_names``' test) the bytes behind its '>' up to the first byte <= 0x20, and a leading b"" when sequence
    stands in front of the first header line."""
    names: List[bytes] = []
    headless = False
    for line in bytes(text).replace(b"\r\n", b"\n").replace(b"\r", b"\n").split(b"\n"):
        line = line.strip(_BLANKS)
        if line.startswith(b">"):
            end = 1
            while end < len(line) and line[end] > 0x20:
                end += 1
            names.append(line[1:end])
        elif not names and not headless and line.replace(b"*", b""):
            headless = True
    return ([b""] if headless else []) + names


def orf_reads(file: Union[str, Path, bytes], out_path: Union[str, Path, None], min_aa: int = 32, start: bool = False,
              alt_starts: bool = False, strand: str = "both", tsv_path: Union[str, Path, None] = None, device: int = 0) -> Dict[str, object]:
    """The open reading frames of a nucleotide FASTA or FASTQ file ('.gz' inflated, FASTQ converted by mk_fq2fa; or the
    FASTA text itself as bytes, for a caller that holds it already), called on the GPU and written as protein FASTA to
    ``out_path`` (gzip level 1 if it ends in '.gz'; None: not written).  Counter.orfs has the rule: six-frame
    stop-to-stop ORFs of ``min_aa`` codons or more, from the first ATG with ``start`` (GTG and TTG too with
    ``alt_starts``), ``strand`` "both", "plus" or "minus".  This stands where MerCat2 runs prodigal or FragGeneScan; it
    is that stated rule, not a gene caller.  ``tsv_path``: one line per ORF (report.write_orf_tsv).  No table is read: the
    call opens a small context of its own on ``device``.  Returns the mk_orf_t figures, without the timings."""
    text = bytes(file) if isinstance(file, (bytes, bytearray, memoryview)) else _reads_text(file)
    info: Dict[str, object] = {}
    with native.Counter(5, native.ALPHABET_NT2, device=device) as ctx:
        out, rows = ctx.orfs(text, min_aa=min_aa, start=start, alt_starts=alt_starts, strand=strand, info=info)
    if out_path is not None:
        _write_reads(out_path, out)
    if tsv_path is not None:
        from .report import write_orf_tsv
        write_orf_tsv(tsv_path, orf_names(text), rows)
    return {name: value for name, value in info.items() if not name.startswith("s_")}


def _reads_text(file: Union[str, Path]) -> bytes:
    """A FASTA or FASTQ file as the read-writing calls read it: '.gz' inflated, FASTQ converted by mk_fq2fa."""
    text = read_fasta_bytes(file)
    if str(file).lower().endswith(FASTQ_SUFFIXES):
        text, _ = native.fq2fa(text)
    return text


def _write_reads(path: Union[str, Path], data: bytes) -> None:
    """gzip (level 1) if the name ends in '.gz', plain bytes otherwise."""
    if str(path).lower().endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as fh:
            fh.write(data)
    else:
        with open(path, "wb") as fh:
            fh.write(data)


def _pairs_text(file, mate_file) -> bytes:
    """The interleaved text of a paired run: the file itself, or -- with ``mate_file`` -- both files read as above and
    interleaved on the host (native.interleave: off the GPU path, one more pass over both texts)."""
    text = _reads_text(file)
    return text if mate_file is None else native.interleave(text, _reads_text(mate_file))


def _write_pairs(out: bytes, singles: Optional[bytes], out_path, out_path2, singles_path) -> None:
    """Interleaved to ``out_path``, or split on the host into ``out_path`` and ``out_path2``; the orphans to
    ``singles_path`` where that is given."""
    if out_path2 is None:
        _write_reads(out_path, out)
    else:
        first, second = native.split_pairs(out)
        _write_reads(out_path, first)
        _write_reads(out_path2, second)
    if singles_path is not None:
        _write_reads(singles_path, singles or b"")


def _is_paired(paired, mate_file, out_path2, singles_path) -> bool:
    if not (paired or mate_file is not None):
        if out_path2 is not None or singles_path is not None:
            raise ValueError("out_path2 and singles_path go with paired reads only (paired=True or mate_file)")
        return False
    return True


def _fastq_texts(what: str, file, mate_file=None) -> Tuple[bytes, bytes]:
    """(raw, fasta) of a ``fastq_out`` run: the raw FASTQ text -- with ``mate_file`` both raw texts interleaved on the host
    (native.interleave_fastq) -- and the FASTA view mk_fq2fa gives of it, which the deciding call reads.  ValueError for
    a file without a FASTQ suffix, and for a text in which fq2fa drops a header line: record r of the FASTA view would
    no longer be record r of the FASTQ text."""
    for f in (file, mate_file):
        if f is not None and not str(f).lower().endswith(FASTQ_SUFFIXES):
            raise ValueError("%s: fastq_out needs FASTQ input (%s), not %s" % (what, " / ".join(FASTQ_SUFFIXES), f))
    raw = read_fasta_bytes(file)
    if mate_file is not None:
        raw = native.interleave_fastq(raw, read_fasta_bytes(mate_file))
    text, st = native.fq2fa(raw)
    if st["headers_dropped"] > 0:
        raise ValueError("%s: fastq_out needs every FASTQ record to start with '@'; %d header line(s) of %s do not, and "
                         "fq2fa drops them" % (what, st["headers_dropped"], file))
    return raw, text


def _write_fastq(table: "native.Counter", raw: bytes, keep, kept, out_path, out_path2=None, singles_path=None) -> int:
    """The decision of a call on the FASTA view applied to the raw FASTQ text (Counter.fastq_select) and written as
    _write_pairs writes FASTA: ``out_path``, or split into ``out_path`` and ``out_path2``; the orphans (keep == 2) to
    ``singles_path``.  Returns the bytes of the main output."""
    out = table.fastq_select(raw, keep, kept, which=1)
    if out_path2 is None:
        _write_reads(out_path, out)
    else:
        first, second = native.split_pairs_fastq(out)
        _write_reads(out_path, first)
        _write_reads(out_path2, second)
    if singles_path is not None:
        _write_reads(singles_path, table.fastq_select(raw, keep, kept, which=2) if keep is not None else b"")
    return len(out)


def filter_reads(table: "native.Counter", file: Union[str, Path], out_path: Union[str, Path], at_least: int = 1, min_hits: int = 1,
                 min_frac: float = 0.0, invert: bool = False, paired: bool = False, mate_file: Union[str, Path, None] = None,
                 out_path2: Union[str, Path, None] = None, singles_path: Union[str, Path, None] = None,
                 both: bool = False, fastq_out: bool = False) -> Dict[str, int]:
    """The records of a FASTA or FASTQ file that match a table still on the GPU (Counter.filter), written to ``out_path``
    -- gzip (level 1) if that name ends in '.gz', plain bytes otherwise; with ``invert`` the records that do not match.  A
    record matches iff at least ``min_hits`` of its k-mers occur ``at_least`` times in the table and they are at least
    ``min_frac`` (0..1) of its k-mers.  The file is read as screen_reads reads it: '.gz' inflated on the host, a FASTQ
    file ('.fq' / '.fastq', plain or '.gz') first converted as MerCat2's fq2fa converts it (mk_fq2fa) -- so the output is
    always FASTA, the text MerCat2 itself counts, and the qualities are gone.  The records are copied byte for byte, in
    order.  A canonical table folds the windows.  Returns {"records", "kept", "bytes_in", "bytes_out"}.
    Paired reads (``paired``: the file is interleaved; or ``mate_file``: the second file of the pair, read the same way
    and interleaved with the first on the host): the pair is the unit (Counter.filter_pairs) -- it is written iff either
    mate matches, with ``both`` iff both do.  The output is interleaved in ``out_path``, or split into ``out_path`` and
    ``out_path2``; ``singles_path`` receives the matching mates of pairs that fail under ``both``.  The result gains
    {"pairs", "pairs_kept", "singles"}.
    ``fastq_out``: the input (and the mate file) must be FASTQ, and the same records are written as FASTQ, qualities
    included, byte for byte (Counter.fastq_select applies the decision to the raw text); "bytes_out" counts those bytes.
    The FASTA output of the deciding call is computed and thrown away."""
    min_ppm = native.ppm_of_fraction(min_frac)
    if fastq_out:
        is_paired = _is_paired(paired, mate_file, out_path2, singles_path)
        raw, text = _fastq_texts("filter_reads", file, mate_file)
        info = {}
        if is_paired:
            _, _, keep, _, _ = table.filter_pairs(text, at_least, min_hits, min_ppm, both, invert, singles=singles_path is not None, info=info)
            done = {"records": int(keep.shape[0]), "kept": int(info["records_out"]), "bytes_in": len(text), "bytes_out": 0,
                    "pairs": int(info["pairs"]), "pairs_kept": int(info["pairs_out"]), "singles": int(info["singles_out"])}
        else:
            _, keep, _ = table.filter(text, at_least, min_hits, min_ppm, invert)
            done = {"records": int(keep.shape[0]), "kept": int(keep.sum()), "bytes_in": len(text), "bytes_out": 0}
        done["bytes_out"] = _write_fastq(table, raw, keep, None, out_path, out_path2, singles_path)
        return done
    if _is_paired(paired, mate_file, out_path2, singles_path):
        text = _pairs_text(file, mate_file)
        info: Dict[str, int] = {}
        out, singles, keep, _, _ = table.filter_pairs(text, at_least, min_hits, min_ppm, both, invert,
                                                      singles=singles_path is not None, info=info)
        _write_pairs(out, singles, out_path, out_path2, singles_path)
        return {"records": int(keep.shape[0]), "kept": int(info["records_out"]), "bytes_in": len(text), "bytes_out": len(out),
                "pairs": int(info["pairs"]), "pairs_kept": int(info["pairs_out"]), "singles": int(info["singles_out"])}
    text = read_fasta_bytes(file)
    if str(file).lower().endswith(FASTQ_SUFFIXES):
        text, _ = native.fq2fa(text)
    out, keep, _ = table.filter(text, at_least, min_hits, min_ppm, invert)
    if str(out_path).lower().endswith(".gz"):
        with gzip.open(out_path, "wb", compresslevel=1) as fh:
            fh.write(out)
    else:
        with open(out_path, "wb") as fh:
            fh.write(out)
    return {"records": int(keep.shape[0]), "kept": int(keep.sum()), "bytes_in": len(text), "bytes_out": len(out)}


def trim_reads(table: "native.Counter", file: Union[str, Path], out_path: Union[str, Path], at_least: int = 2,
               min_len: int = 0, tsv_path: Union[str, Path, None] = None, paired: bool = False,
               mate_file: Union[str, Path, None] = None, out_path2: Union[str, Path, None] = None,
               singles_path: Union[str, Path, None] = None, fastq_out: bool = False) -> Dict[str, int]:
    """The records of a FASTA or FASTQ file, each cut in front of its first k-mer that a table still on the GPU holds fewer
    than ``at_least`` times (Counter.trim: khmer's trim_on_abundance), written to ``out_path`` -- gzip (level 1) if that
    name ends in '.gz', plain bytes otherwise.  A record of which fewer than max(``min_len``, k) characters remain is
    dropped.  The file is read as filter_reads reads it: '.gz' inflated on the host, a FASTQ file first converted as
    MerCat2's fq2fa converts it (mk_fq2fa) -- so the output is always FASTA: the header line as it stands, the kept
    characters on one line.  A canonical table folds the windows.  Returns {"records", "kept", "trimmed", "dropped",
    "bases_in", "bases_out", "bytes_out"}.  With ``tsv_path`` every record's name, length and kept characters are written
    there too (report.write_trim_tsv).
    Paired reads (``paired``: the file is interleaved; or ``mate_file``: the second file of the pair, read the same way
    and interleaved with the first on the host): the pair is the unit (Counter.trim_pairs) -- both mates are written,
    each at its own trimmed length, iff both keep something.  The output is interleaved in ``out_path``, or split into
    ``out_path`` and ``out_path2``; ``singles_path`` receives the mates that keep something while their mate does not.
    "kept" then counts the records written in pairs and the result gains {"pairs", "pairs_kept", "singles"}.
    ``fastq_out``: the input (and the mate file) must be FASTQ, and the same records are written as FASTQ, the quality
    line cut wherever the sequence line is (Counter.fastq_select applies the kept lengths to the raw text); "bytes_out"
    counts those bytes.  The FASTA output of the deciding call is computed and thrown away; the TSV is unchanged."""
    if fastq_out:
        is_paired = _is_paired(paired, mate_file, out_path2, singles_path)
        raw, text = _fastq_texts("trim_reads", file, mate_file)
        info = {}
        if is_paired:
            _, _, keep, kept, _ = table.trim_pairs(text, at_least, min_len, singles=singles_path is not None, info=info)
        else:
            keep = None
            _, kept, _ = table.trim(text, at_least, min_len, info=info)
        if tsv_path is not None:
            from .report import write_trim_tsv
            if is_paired:
                write_trim_tsv(tsv_path, record_names(text), record_lengths(text), kept, keep)
            else:
                write_trim_tsv(tsv_path, record_names(text), record_lengths(text), kept)
        done = {"records": int(kept.shape[0]), "kept": int(info["records_out"]), "trimmed": int(info["records_trimmed"]),
                "dropped": int(info["records_dropped"]), "bases_in": int(info["bases_in"]), "bases_out": int(info["bases_out"]),
                "bytes_out": _write_fastq(table, raw, keep, kept, out_path, out_path2, singles_path)}
        if is_paired:
            done.update({"pairs": int(info["pairs"]), "pairs_kept": int(info["pairs_out"]), "singles": int(info["singles_out"])})
        return done
    if _is_paired(paired, mate_file, out_path2, singles_path):
        text = _pairs_text(file, mate_file)
        info: Dict[str, int] = {}
        out, singles, keep, kept, _ = table.trim_pairs(text, at_least, min_len, singles=singles_path is not None, info=info)
        _write_pairs(out, singles, out_path, out_path2, singles_path)
        if tsv_path is not None:
            from .report import write_trim_tsv
            write_trim_tsv(tsv_path, record_names(text), record_lengths(text), kept, keep)
        return {"records": int(kept.shape[0]), "kept": int(info["records_out"]), "trimmed": int(info["records_trimmed"]),
                "dropped": int(info["records_dropped"]), "bases_in": int(info["bases_in"]), "bases_out": int(info["bases_out"]),
                "bytes_out": len(out), "pairs": int(info["pairs"]), "pairs_kept": int(info["pairs_out"]),
                "singles": int(info["singles_out"])}
    text = read_fasta_bytes(file)
    if str(file).lower().endswith(FASTQ_SUFFIXES):
        text, _ = native.fq2fa(text)
    info: Dict[str, int] = {}
    out, kept, _ = table.trim(text, at_least, min_len, info=info)
    if str(out_path).lower().endswith(".gz"):
        with gzip.open(out_path, "wb", compresslevel=1) as fh:
            fh.write(out)
    else:
        with open(out_path, "wb") as fh:
            fh.write(out)
    if tsv_path is not None:
        from .report import write_trim_tsv
        write_trim_tsv(tsv_path, record_names(text), record_lengths(text), kept)
    return {"records": int(kept.shape[0]), "kept": int(info["records_out"]), "trimmed": int(info["records_trimmed"]),
            "dropped": int(info["records_dropped"]), "bases_in": int(info["bases_in"]), "bases_out": int(info["bases_out"]),
            "bytes_out": len(out)}


def correct_reads(table: "native.Counter", file: Union[str, Path], out_path: Union[str, Path], at_least: int = 2, rounds: int = 1,
                  tsv_path: Union[str, Path, None] = None, mate_file: Union[str, Path, None] = None,
                  out_path2: Union[str, Path, None] = None) -> Dict[str, int]:
    """The records of a FASTA or FASTQ file with their isolated substitutions corrected against a table still on the GPU
    (Counter.correct: a run of k-mers the table holds fewer than ``at_least`` times, shaped as one wrong base shapes it,
    is repaired iff exactly one other base makes all of them solid), written to ``out_path`` -- gzip (level 1) if that
    name ends in '.gz', plain bytes otherwise.  Every record is written.  The file is read as filter_reads reads it:
    '.gz' inflated on the host, a FASTQ file first converted as MerCat2's fq2fa converts it (mk_fq2fa) -- so the output
    is always FASTA: the header line as it stands, the characters on one line.  ``rounds`` > 1 corrects the output
    again: a fix can free a neighbouring run.  A canonical table folds the windows.  Returns {"records", "runs", "fixed",
    "ambiguous", "unfixable", "bases", "bytes_out"}: "runs" of the first round, the others summed over the rounds.  With
    ``tsv_path`` every record's name, length and those four figures are written there too (report.write_correct_tsv).
    With ``mate_file`` the two files are interleaved on the host (native.interleave), corrected as one text and split
    again into ``out_path`` and ``out_path2`` (interleaved in ``out_path`` without the latter): every record is
    written, so pairs stay pairs."""
    if rounds < 1:
        raise ValueError("correct_reads: rounds must be 1 or more")
    if mate_file is None and out_path2 is not None:
        raise ValueError("correct_reads: out_path2 goes with mate_file only")
    first = text = _reads_text(file) if mate_file is None else _pairs_text(file, mate_file)
    fix = None
    for _ in range(rounds):
        text, step, _ = table.correct(text, at_least)
        if fix is None:
            fix = step.copy()
        else:
            fix[:, 1:] += step[:, 1:]
    if mate_file is None:
        _write_reads(out_path, text)
    else:
        _write_pairs(text, None, out_path, out_path2, None)
    lengths = record_lengths(first)
    if tsv_path is not None:
        from .report import write_correct_tsv
        write_correct_tsv(tsv_path, record_names(first), lengths, fix)
    total = [int(v) for v in fix.sum(axis=0, dtype="uint64")]
    return {"records": int(fix.shape[0]), "runs": total[0], "fixed": total[1], "ambiguous": total[2], "unfixable": total[3],
            "bases": int(sum(lengths)), "bytes_out": len(text)}


def correct_reads_fastq(table: "native.Counter", file: Union[str, Path], out_path: Union[str, Path], at_least: int = 2, rounds: int = 1,
                        tsv_path: Union[str, Path, None] = None, mate_file: Union[str, Path, None] = None,
                        out_path2: Union[str, Path, None] = None, new_qual=0) -> Dict[str, int]:
    """correct_reads with FASTQ out, qualities included (correct_reads keeps the arguments it has).  The input -- and the
    mate -- must be FASTQ ('.gz' inflated on the host); the text is read on the GPU as it stands (Counter.correct_fastq)
    and written back byte for byte but for the fixed bases, so the FASTA output is never built.  ``new_qual`` (an int,
    or one character; 0: none) is written over the quality of every fixed base.  ``rounds`` > 1 corrects the FASTQ
    output again.  With ``mate_file`` the two files are interleaved on the host (native.interleave_fastq), corrected in
    one call and split again (native.split_pairs_fastq) into ``out_path`` and ``out_path2`` (interleaved in ``out_path``
    without the latter).  The returned figures and the TSV are correct_reads' for the same file: names and lengths are
    those of the FASTA view mk_fq2fa gives of the reads; "bytes_out" counts the FASTQ bytes.  ValueError for input
    without a FASTQ suffix; MercatHipError (MK_ERR_UNSUPPORTED) for a malformed record."""
    if rounds < 1:
        raise ValueError("correct_reads_fastq: rounds must be 1 or more")
    if mate_file is None and out_path2 is not None:
        raise ValueError("correct_reads_fastq: out_path2 goes with mate_file only")
    for f in (file, mate_file):
        if f is not None and not str(f).lower().endswith(FASTQ_SUFFIXES):
            raise ValueError("correct_reads_fastq: needs FASTQ input (%s), not %s" % (" / ".join(FASTQ_SUFFIXES), f))
    qual = native.quality_byte(new_qual)
    if qual and not 33 <= qual <= 126:
        raise ValueError("correct_reads_fastq: new_qual %r is no printable quality character ('!'..'~')" % (new_qual,))
    raw = read_fasta_bytes(file)
    if mate_file is not None:
        raw = native.interleave_fastq(raw, read_fasta_bytes(mate_file))
    first, _ = native.fq2fa(raw)
    fix = None
    for _ in range(rounds):
        raw, step, _ = table.correct_fastq(raw, at_least, qual)
        if fix is None:
            fix = step.copy()
        else:
            fix[:, 1:] += step[:, 1:]
    if mate_file is None or out_path2 is None:
        _write_reads(out_path, raw)
    else:
        one, two = native.split_pairs_fastq(raw)
        _write_reads(out_path, one)
        _write_reads(out_path2, two)
    lengths = record_lengths(first)
    if tsv_path is not None:
        from .report import write_correct_tsv
        write_correct_tsv(tsv_path, record_names(first), lengths, fix)
    total = [int(v) for v in fix.sum(axis=0, dtype="uint64")]
    return {"records": int(fix.shape[0]), "runs": total[0], "fixed": total[1], "ambiguous": total[2], "unfixable": total[3],
            "bases": int(sum(lengths)), "bytes_out": len(raw)}


def normalize_reads(table: "native.Counter", file: Union[str, Path], out_path: Union[str, Path], target: int = 20,
                    min_depth: int = 0, seed: int = 0, invert: bool = False, tsv_path: Union[str, Path, None] = None) -> Dict[str, int]:
    """The records of a FASTA or FASTQ file thinned to depth ``target`` against a table still on the GPU that has been
    counted from all of them (Counter.normalize: BBNorm's plan with khmer's median k-mer abundance as the depth), written to
    ``out_path`` -- gzip (level 1) if that name ends in '.gz', plain bytes otherwise.  A record without k-mers or of depth
    below ``min_depth`` is dropped, one of depth at most ``target`` is kept, a deeper one is kept with probability
    target / depth by a draw that depends only on ``seed`` and the record's index; with ``invert`` the records that are
    not kept are written instead.  The file is read as filter_reads reads it: '.gz' inflated on the host, a FASTQ file
    first converted as MerCat2's fq2fa converts it (mk_fq2fa) -- so the output is always FASTA, the records byte for byte
    and in order, and the qualities are gone.  A canonical table folds the windows.  Returns {"records", "kept", "short",
    "low", "over", "thinned", "bytes_out"} ("kept": the records written).  With ``tsv_path`` every record's name,
    k-mers, depth and fate are written there too (report.write_norm_tsv).  Paired reads: normalize_read_pairs.  FASTQ
    out, with the qualities: normalize_reads_fastq."""
    text = read_fasta_bytes(file)
    if str(file).lower().endswith(FASTQ_SUFFIXES):
        text, _ = native.fq2fa(text)
    info: Dict[str, int] = {}
    out, keep, med, rows = table.normalize(text, target, min_depth, seed, invert, info=info)
    if str(out_path).lower().endswith(".gz"):
        with gzip.open(out_path, "wb", compresslevel=1) as fh:
            fh.write(out)
    else:
        with open(out_path, "wb") as fh:
            fh.write(out)
    if tsv_path is not None:
        from .report import write_norm_tsv
        write_norm_tsv(tsv_path, record_names(text), rows[:, 0], med, keep)
    return {"records": int(keep.shape[0]), "kept": int(info["records_out"]), "short": int(info["records_short"]),
            "low": int(info["records_low"]), "over": int(info["records_over"]), "thinned": int(info["records_thinned"]),
            "bytes_out": len(out)}


def normalize_reads_fastq(table: "native.Counter", file: Union[str, Path], out_path: Union[str, Path], target: int = 20,
                          min_depth: int = 0, seed: int = 0, invert: bool = False, tsv_path: Union[str, Path, None] = None) -> Dict[str, int]:
    """normalize_reads with FASTQ out (what ``fastq_out=True`` is to filter_reads, trim_reads and normalize_read_pairs;
    normalize_reads keeps the arguments it has).  The input must be FASTQ, and the records normalize_reads would write are
    written as FASTQ, qualities included, byte for byte (Counter.fastq_select applies the decision to the raw text);
    "bytes_out" counts those bytes.  The FASTA output of the deciding call is computed and thrown away; the figures and
    the TSV are normalize_reads'."""
    raw, text = _fastq_texts("normalize_reads_fastq", file)
    info: Dict[str, int] = {}
    _, keep, med, rows = table.normalize(text, target, min_depth, seed, invert, info=info)
    if tsv_path is not None:
        from .report import write_norm_tsv
        write_norm_tsv(tsv_path, record_names(text), rows[:, 0], med, keep)
    return {"records": int(keep.shape[0]), "kept": int(info["records_out"]), "short": int(info["records_short"]),
            "low": int(info["records_low"]), "over": int(info["records_over"]), "thinned": int(info["records_thinned"]),
            "bytes_out": _write_fastq(table, raw, keep, None, out_path)}


def normalize_read_pairs(table: "native.Counter", file: Union[str, Path], out_path: Union[str, Path], target: int = 20,
                         min_depth: int = 0, seed: int = 0, invert: bool = False, tsv_path: Union[str, Path, None] = None,
                         mate_file: Union[str, Path, None] = None, out_path2: Union[str, Path, None] = None,
                         singles_path: Union[str, Path, None] = None, fastq_out: bool = False) -> Dict[str, int]:
    """normalize_reads for paired reads (the paired form of filter_reads and trim_reads is an argument of theirs;
    normalize_reads keeps the arguments it has).  ``file`` is interleaved, or -- with ``mate_file`` -- the first of two
    files that are read as normalize_reads reads one and interleaved on the host.  The pair is the unit
    (Counter.normalize_pairs): its depth is that of its shallowest mate that has k-mers and reaches ``min_depth``, its
    draw that of its first mate.  The output is interleaved in ``out_path``, or split into ``out_path`` and
    ``out_path2``; normalisation has no orphans, so a ``singles_path`` is written empty.  Returns normalize_reads' figures
    ("kept": the records written) and {"pairs", "pairs_kept", "singles"}; the TSV gains the column ``pair``.
    ``fastq_out``: FASTQ in (the mate file too), the same records out as FASTQ with their qualities (Counter.fastq_select
    applies the decision to the raw text); the FASTA output of the deciding call is computed and thrown away."""
    if fastq_out:
        raw, text = _fastq_texts("normalize_read_pairs", file, mate_file)
        info = {}
        _, _, keep, med, rows = table.normalize_pairs(text, target, min_depth, seed, invert, info=info)
        if tsv_path is not None:
            from .report import write_norm_tsv
            write_norm_tsv(tsv_path, record_names(text), rows[:, 0], med, keep, paired=True)
        return {"records": int(keep.shape[0]), "kept": int(info["records_out"]), "short": int(info["records_short"]),
                "low": int(info["records_low"]), "over": int(info["records_over"]), "thinned": int(info["records_thinned"]),
                "bytes_out": _write_fastq(table, raw, keep, None, out_path, out_path2, singles_path),
                "pairs": int(info["pairs"]), "pairs_kept": int(info["pairs_out"]), "singles": int(info["singles_out"])}
    text = _pairs_text(file, mate_file)
    info: Dict[str, int] = {}
    out, _, keep, med, rows = table.normalize_pairs(text, target, min_depth, seed, invert, info=info)
    _write_pairs(out, b"", out_path, out_path2, singles_path)
    if tsv_path is not None:
        from .report import write_norm_tsv
        write_norm_tsv(tsv_path, record_names(text), rows[:, 0], med, keep, paired=True)
    return {"records": int(keep.shape[0]), "kept": int(info["records_out"]), "short": int(info["records_short"]),
            "low": int(info["records_low"]), "over": int(info["records_over"]), "thinned": int(info["records_thinned"]),
            "bytes_out": len(out), "pairs": int(info["pairs"]), "pairs_kept": int(info["pairs_out"]),
            "singles": int(info["singles_out"])}


def fastq_names(raw: bytes) -> List[str]:
    """The names of a FASTQ text's 4-line records, in order: the first word behind the '@' of line 4r ("" for none)."""
    lines = raw.count(b"\n") + (1 if raw and not raw.endswith(b"\n") else 0)
    heads = raw.split(b"\n")[0::4][: lines // 4]
    return [(h[1:].split() or [b""])[0].decode("utf-8", "replace") for h in heads]


def qtrim_reads(file: Union[str, Path, bytes], out_path: Union[str, Path, None], cut_back: int = 20, cut_front: int = 0, min_len: int = 0,
                max_n: Optional[int] = None, low_q: int = 0, max_low_frac: float = 1.0, min_mean_q: int = 0, phred_base: int = 33,
                paired: bool = False, tsv_path: Union[str, Path, None] = None, summary_path: Union[str, Path, None] = None,
                mate_file: Union[str, Path, None] = None, out_path2: Union[str, Path, None] = None,
                singles_path: Union[str, Path, None] = None, device: int = 0, keep_text: bool = False) -> Dict[str, object]:
    """The reads of a FASTQ file ('.fq' / '.fastq', plain or '.gz'; or the FASTQ text itself as bytes, for a caller that
    holds it already) quality-trimmed and filtered on the GPU
    (Counter.fastq_qtrim has the rule and the options: BWA's / cutadapt's running-sum cut at both ends, then length, N,
    low-quality share and mean quality), written as FASTQ to ``out_path`` -- gzip (level 1) if that name ends in '.gz'.
    This stands where MerCat2 runs fastp; its result is this stated rule's, not fastp's (no adapter removal).  No table
    is read: the call opens a small context of its own on ``device``.
    Paired reads (``paired``: the file is interleaved; or ``mate_file``: the second file, interleaved with the first on
    the host by native.interleave_fastq): a pair is written iff both mates pass, interleaved to ``out_path`` or split
    into ``out_path`` and ``out_path2``; ``singles_path`` receives the reads that pass while their mate does not (a
    second call with which = 2).  ``tsv_path``: every record's name, row and keep value (report.write_qtrim_tsv);
    ``summary_path``: reads, bases, Q20 / Q30 bases and mean quality before and after, and the drop counts
    (report.write_qtrim_summary).  Returns the mk_fastq_qtrim_t figures, "hist" (2 x 256) and, with ``keep_text``, the
    main output under "text" (interleaved for pairs)."""
    is_paired = _is_paired(paired, mate_file, out_path2, singles_path)
    is_text = isinstance(file, (bytes, bytearray, memoryview))
    for f in (None if is_text else file, mate_file):
        if f is not None and not str(f).lower().endswith(FASTQ_SUFFIXES):
            raise ValueError("qtrim_reads: needs FASTQ input (%s), not %s" % (" / ".join(FASTQ_SUFFIXES), f))
    raw = bytes(file) if is_text else read_fasta_bytes(file)
    if mate_file is not None:
        raw = native.interleave_fastq(raw, read_fasta_bytes(mate_file))
    opts = dict(cut_back=cut_back, cut_front=cut_front, min_len=min_len, max_n=max_n, low_q=low_q, max_low_frac=max_low_frac,
                min_mean_q=min_mean_q, phred_base=phred_base, paired=is_paired)
    info: Dict[str, object] = {}
    with native.Counter(5, native.ALPHABET_NT2, device=device) as ctx:
        out, keep, rows, hist = ctx.fastq_qtrim(raw, which=1, info=info, **opts)
        singles = ctx.fastq_qtrim(raw, which=2, **opts)[0] if singles_path is not None else None
    if out_path is not None:
        if out_path2 is None:
            _write_reads(out_path, out)
        else:
            first, second = native.split_pairs_fastq(out)
            _write_reads(out_path, first)
            _write_reads(out_path2, second)
    if singles_path is not None:
        _write_reads(singles_path, singles or b"")
    if tsv_path is not None:
        from .report import write_qtrim_tsv
        write_qtrim_tsv(tsv_path, fastq_names(raw), rows, keep)
    if summary_path is not None:
        from .report import write_qtrim_summary
        write_qtrim_summary(summary_path, info, hist)
    done: Dict[str, object] = {name: value for name, value in info.items() if not name.startswith("s_")}
    done["hist"] = hist
    if keep_text:
        done["text"] = out
    return done


def qc_reads(file: Union[str, Path, bytes], out_prefix: Union[str, Path, None] = None, max_pos: int = 512, phred_base: int = 33,
             paired: bool = False, mate_file: Union[str, Path, None] = None, device: int = 0) -> Dict[str, object]:
    """The quality-control tables of a FASTQ file ('.fq' / '.fastq', plain or '.gz'; or the FASTQ text itself as bytes,
    for a caller that holds it already), reduced on the GPU (Counter.fastq_qc has the rule and the tables: per cycle the
    bases of every quality value and of every base class, per read its length, mean quality and GC share).  This stands
    where MerCat2 runs fastqc; the figures are that stated rule's, not fastqc's (no plots, no duplication levels, no
    verdicts).  No table is read: the call opens a small context of its own on ``device``.
    Paired reads (``paired``: the file is interleaved; or ``mate_file``: the second file, interleaved with the first on
    the host by native.interleave_fastq): every table has a class a mate.  ``out_prefix``: the tables are also written as
    ``<out_prefix>_cycles.tsv``, ``_quality.tsv``, ``_gc.tsv``, ``_length.tsv`` and ``_summary.tsv``
    (report.write_qc_files).  Returns the tables and, under their names, the mk_fastq_qc_t figures."""
    is_text = isinstance(file, (bytes, bytearray, memoryview))
    for f in (None if is_text else file, mate_file):
        if f is not None and not str(f).lower().endswith(FASTQ_SUFFIXES):
            raise ValueError("qc_reads: needs FASTQ input (%s), not %s" % (" / ".join(FASTQ_SUFFIXES), f))
    raw = bytes(file) if is_text else read_fasta_bytes(file)
    if mate_file is not None:
        raw = native.interleave_fastq(raw, read_fasta_bytes(mate_file))
    info: Dict[str, object] = {}
    with native.Counter(5, native.ALPHABET_NT2, device=device) as ctx:
        done: Dict[str, object] = ctx.fastq_qc(raw, max_pos=max_pos, phred_base=phred_base, paired=bool(paired or mate_file is not None),
                                               info=info)
    if out_prefix is not None:
        from .report import write_qc_files
        write_qc_files(out_prefix, done)
    done.update({name: value for name, value in info.items() if not name.startswith("s_")})
    return done


def fastq_keys(raw: bytes, prefix: int = 0) -> List[bytes]:
    """The keys of a FASTQ text's 4-line records as Counter.fastq_dedup compares them: line 4r + 1 without one trailing
    '\\r', cut to ``prefix`` bytes where that is not 0."""
    lines = raw.count(b"\n") + (1 if raw and not raw.endswith(b"\n") else 0)
    seqs = raw.split(b"\n")[1::4][: lines // 4]
    seqs = [s[:-1] if s.endswith(b"\r") else s for s in seqs]
    return [s[:prefix] for s in seqs] if prefix else seqs


def dedup_reads(file: Union[str, Path, bytes], out_path: Union[str, Path, None], prefix: int = 0, paired: bool = False,
                keep: str = "unique", high: int = 100, over_frac: float = 0.001, tsv_path: Union[str, Path, None] = None,
                summary_path: Union[str, Path, None] = None, levels_path: Union[str, Path, None] = None,
                over_path: Union[str, Path, None] = None, mate_file: Union[str, Path, None] = None,
                out_path2: Union[str, Path, None] = None, device: int = 0, keep_text: bool = False) -> Dict[str, object]:
    """The reads of a FASTQ file ('.fq' / '.fastq', plain or '.gz'; or the FASTQ text itself as bytes, for a caller that
    holds it already) without their duplicates, found on the GPU (Counter.fastq_dedup has the rule: reads whose sequence
    bytes -- with ``prefix`` their first ``prefix`` bases -- are equal form a cluster, and its first record over the
    whole text stays), written as FASTQ to ``out_path`` -- gzip (level 1) if that name ends in '.gz'.  ``keep``:
    "unique" writes the first of every cluster, "duplicate" the records a run removes.  This stands where fastp --dedup
    or clumpify dedupe would; it is exact (no hash decides), case and N count as they stand, no reverse complement is
    tried.  No table is read: the call opens a small context of its own on ``device``.
    Paired reads (``paired``: the file is interleaved; or ``mate_file``: the second file, interleaved with the first on
    the host by native.interleave_fastq): the unit is the pair, equal iff both mates are; the output is interleaved to
    ``out_path`` or split into ``out_path`` and ``out_path2``.  ``tsv_path``: every record's name, length, first, copies
    and keep value (report.write_dedup_tsv); ``levels_path``: the duplication levels; ``summary_path``: units, distinct,
    duplicates, rate, largest cluster, bases before and after; ``over_path``: the clusters that hold at least
    ``over_frac`` of the units (and two of them), by copies descending, then first ascending, at most 1000, with the
    sequence read from the text at their first record -- host work on a handful of rows.  Returns the mk_fastq_dedup_t
    figures, "levels", "over" and, with ``keep_text``, the output under "text" (interleaved for pairs)."""
    if keep not in ("unique", "duplicate"):
        raise ValueError("dedup_reads: keep must be 'unique' or 'duplicate', not %r" % (keep,))
    is_paired = _is_paired(paired, mate_file, out_path2, None)
    is_text = isinstance(file, (bytes, bytearray, memoryview))
    for f in (None if is_text else file, mate_file):
        if f is not None and not str(f).lower().endswith(FASTQ_SUFFIXES):
            raise ValueError("dedup_reads: needs FASTQ input (%s), not %s" % (" / ".join(FASTQ_SUFFIXES), f))
    raw = bytes(file) if is_text else read_fasta_bytes(file)
    if mate_file is not None:
        raw = native.interleave_fastq(raw, read_fasta_bytes(mate_file))
    np = native.np
    info: Dict[str, object] = {}
    with native.Counter(5, native.ALPHABET_NT2, device=device) as ctx:
        out, kept, rows, levels = ctx.fastq_dedup(raw, prefix=prefix, paired=is_paired, which=1, high=high, info=info)
        if keep == "duplicate":
            out = ctx.fastq_dedup(raw, prefix=prefix, paired=is_paired, which=2, high=high)[0]
    if out_path is not None:
        if out_path2 is None:
            _write_reads(out_path, out)
        else:
            first, second = native.split_pairs_fastq(out)
            _write_reads(out_path, first)
            _write_reads(out_path2, second)
    # cluster sizes per record: one integer a record, which left the GPU anyway
    step = 2 if is_paired else 1
    units = len(rows) // step
    first = rows[:, 1].astype(np.int64)
    unit_first = first[::step] // step
    copies = np.repeat(np.bincount(unit_first, minlength=max(units, 1))[unit_first], step) if units else np.zeros(0, np.int64)
    from . import report
    over = report.dedup_over(copies, rows, is_paired, over_frac)
    names = fastq_names(raw) if tsv_path is not None or over_path is not None else None
    if tsv_path is not None:
        report.write_dedup_tsv(tsv_path, names, rows, kept, copies)
    if levels_path is not None:
        report.write_dedup_levels(levels_path, levels, units)
    if summary_path is not None:
        report.write_dedup_summary(summary_path, info, is_paired)
    if over_path is not None:
        report.write_dedup_over(over_path, over, names, fastq_keys(raw, prefix), units, is_paired)
    done: Dict[str, object] = {name: value for name, value in info.items() if not name.startswith("s_")}
    done["levels"] = levels
    done["over"] = over
    if keep_text:
        done["text"] = out
    return done


def _named_adapters(adapters) -> Tuple[List[str], List[str]]:
    """(names, seqs) of ``adapters``: None (native.ILLUMINA_ADAPTERS), a FASTA file (native.read_adapters), (name, seq)
    pairs, or plain sequences, which are named by themselves."""
    if adapters is None:
        adapters = native.ILLUMINA_ADAPTERS
    if isinstance(adapters, (str, Path)):
        return native.read_adapters(adapters)
    names, seqs = [], []
    for a in adapters:
        name, seq = a if isinstance(a, tuple) else (None, a)
        seq = seq.decode("latin-1") if isinstance(seq, (bytes, bytearray)) else str(seq)
        names.append(seq if name is None else str(name))
        seqs.append(seq)
    return names, seqs


def adapt_reads(file: Union[str, Path, bytes], out_path: Union[str, Path, None], adapters=None, adapters2=None, min_overlap: int = 8,
                max_err: float = 0.1, min_len: int = 0, paired: bool = False, tsv_path: Union[str, Path, None] = None,
                summary_path: Union[str, Path, None] = None, mate_file: Union[str, Path, None] = None,
                out_path2: Union[str, Path, None] = None, singles_path: Union[str, Path, None] = None, device: int = 0,
                keep_text: bool = False) -> Dict[str, object]:
    """The reads of a FASTQ file ('.fq' / '.fastq', plain or '.gz'; or the FASTQ text itself as bytes) with their 3'
    adapters removed on the GPU (Counter.fastq_adapt has the rule: the leftmost position at which an adapter matches the
    rest of the read, or runs off its end, over ``min_overlap`` bases within ``max_err`` mismatches a base; no indels),
    written as FASTQ to ``out_path`` -- gzip (level 1) if that name ends in '.gz'.  This is the first job of the fastp
    run MerCat2 starts; its result is this stated rule's, not fastp's.  ``adapters``: None (native.ILLUMINA_ADAPTERS:
    TruSeq, Nextera, small RNA), a FASTA file, (name, sequence) pairs or sequences; ``adapters2``: the same for second
    mates (pairs only).  The default overlap of 8 is set for a panel of hundreds of adapters, not for one.  No table is
    read: the call opens a small context of its own on ``device``.
    Paired reads (``paired``: the file is interleaved; or ``mate_file``: the second file): a pair is written iff both
    mates keep max(``min_len``, 1) bases, interleaved to ``out_path`` or split into ``out_path`` and ``out_path2``;
    ``singles_path`` receives the reads that pass while their mate does not.  ``tsv_path``: every record's name, row and
    keep value (report.write_adapt_tsv); ``summary_path``: reads and bases before and after, reads trimmed and dropped,
    and the hits of every adapter that has any (report.write_adapt_summary).  Returns the mk_fastq_adapt_t figures,
    "hits", "adapter_names" and, with ``keep_text``, the main output under "text" (interleaved for pairs)."""
    is_paired = _is_paired(paired, mate_file, out_path2, singles_path)
    is_text = isinstance(file, (bytes, bytearray, memoryview))
    for f in (None if is_text else file, mate_file):
        if f is not None and not str(f).lower().endswith(FASTQ_SUFFIXES):
            raise ValueError("adapt_reads: needs FASTQ input (%s), not %s" % (" / ".join(FASTQ_SUFFIXES), f))
    if adapters2 is not None and not is_paired:
        raise ValueError("adapt_reads: adapters2 are searched in second mates: needs paired reads")
    names, seqs = _named_adapters(adapters)
    names2, seqs2 = _named_adapters(adapters2) if adapters2 is not None else ([], None)
    raw = bytes(file) if is_text else read_fasta_bytes(file)
    if mate_file is not None:
        raw = native.interleave_fastq(raw, read_fasta_bytes(mate_file))
    opts = dict(min_overlap=min_overlap, max_err=max_err, min_len=min_len, paired=is_paired)
    info: Dict[str, object] = {}
    with native.Counter(5, native.ALPHABET_NT2, device=device) as ctx:
        out, keep, rows, hits = ctx.fastq_adapt(raw, seqs, seqs2, which=1, info=info, **opts)
        singles = ctx.fastq_adapt(raw, seqs, seqs2, which=2, **opts)[0] if singles_path is not None else None
    # the panel holds every distinct sequence once: its names are those of the first record that has it
    first_name: Dict[str, str] = {}
    for name, seq in zip(names + names2, seqs + (seqs2 or [])):
        first_name.setdefault(seq, name)
    panel_names = [first_name[seq] for seq in info.pop("adapters")]
    if out_path is not None:
        if out_path2 is None:
            _write_reads(out_path, out)
        else:
            first, second = native.split_pairs_fastq(out)
            _write_reads(out_path, first)
            _write_reads(out_path2, second)
    if singles_path is not None:
        _write_reads(singles_path, singles or b"")
    if tsv_path is not None:
        from .report import write_adapt_tsv
        write_adapt_tsv(tsv_path, fastq_names(raw), rows, keep, panel_names)
    if summary_path is not None:
        from .report import write_adapt_summary
        write_adapt_summary(summary_path, info, hits, panel_names)
    done: Dict[str, object] = {name: value for name, value in info.items() if not name.startswith("s_")}
    done["hits"] = hits
    done["adapter_names"] = panel_names
    if keep_text:
        done["text"] = out
    return done


def overlap_reads(file: Union[str, Path, bytes], out_path: Union[str, Path, None], mode: str = "merge", min_overlap: int = 30,
                  max_mismatch: int = 5, max_err: float = 0.2, min_len: int = 0, mate_file: Union[str, Path, None] = None,
                  out_path2: Union[str, Path, None] = None, unmerged_path: Union[str, Path, None] = None,
                  unmerged_path2: Union[str, Path, None] = None, tsv_path: Union[str, Path, None] = None,
                  summary_path: Union[str, Path, None] = None, device: int = 0, keep_text: bool = False) -> Dict[str, object]:
    """The paired reads of a FASTQ file ('.fq' / '.fastq', plain or '.gz'; or the FASTQ text itself as bytes) trimmed or
    merged by the overlap of their mates on the GPU (Counter.fastq_overlap has the rule: mate 1 against the reverse
    complement of mate 2, the first offset whose overlap has ``min_overlap`` bases within ``max_mismatch`` mismatches and
    ``max_err`` mismatches a base; no indels).  ``file`` is interleaved, or -- with ``mate_file`` -- the first of two
    files, interleaved on the host (native.interleave_fastq).  This is the paired-end half of the fastp run MerCat2
    starts; its result is this stated rule's, not fastp's.  No table is read: the call opens a small context of its own
    on ``device``.
    ``mode`` "trim": every pair with an overlap is cut to its fragment -- adapter removal without a panel -- and written
    with the others, interleaved to ``out_path`` or split into ``out_path`` and ``out_path2``; a pair whose fragment is
    shorter than max(``min_len``, 1) is dropped.  ``mode`` "merge": every pair with an overlap becomes one read in
    ``out_path``; the pairs without one are written as they stand (a second call with which = 2) to ``unmerged_path``,
    interleaved, or split into ``unmerged_path`` and ``unmerged_path2``.  Outputs are gzip (level 1) where the name ends
    in '.gz'.  ``tsv_path``: every record's name, row and keep value (report.write_overlap_tsv); ``summary_path``: pairs,
    hits, merged / trimmed / dropped / skipped pairs, bases before and after and the pairs of every fragment length
    (report.write_overlap_summary), counted on the host from the rows.  Returns the mk_fastq_overlap_t figures,
    "fragments" ({fragment length: pairs}) and, with ``keep_text``, the main output under "text" and, in merge mode, the
    unmerged pairs under "unmerged"."""
    if mode not in native.OVERLAP_MODES:
        raise ValueError("overlap_reads: mode %r: must be 'trim' or 'merge'" % (mode,))
    merging = mode == "merge"
    if merging and out_path2 is not None:
        raise ValueError("overlap_reads: merged reads are one file: out_path2 goes with mode 'trim'")
    if not merging and (unmerged_path is not None or unmerged_path2 is not None):
        raise ValueError("overlap_reads: unmerged_path goes with mode 'merge': mode 'trim' writes every pair it keeps to out_path")
    if unmerged_path2 is not None and unmerged_path is None:
        raise ValueError("overlap_reads: unmerged_path2 needs unmerged_path")
    is_text = isinstance(file, (bytes, bytearray, memoryview))
    for f in (None if is_text else file, mate_file):
        if f is not None and not str(f).lower().endswith(FASTQ_SUFFIXES):
            raise ValueError("overlap_reads: needs FASTQ input (%s), not %s" % (" / ".join(FASTQ_SUFFIXES), f))
    opts = dict(mode=mode, min_overlap=min_overlap, max_mismatch=max_mismatch, max_err=max_err, min_len=min_len)
    native.overlap_options(**opts)  # (a refused value is refused before a file is read)
    raw = bytes(file) if is_text else read_fasta_bytes(file)
    if mate_file is not None:
        raw = native.interleave_fastq(raw, read_fasta_bytes(mate_file))
    info: Dict[str, object] = {}
    with native.Counter(5, native.ALPHABET_NT2, device=device) as ctx:
        out, keep, rows = ctx.fastq_overlap(raw, which=1, info=info, **opts)
        unmerged = ctx.fastq_overlap(raw, which=2, **opts)[0] if merging and (unmerged_path is not None or keep_text) else None

    def write(text, path, path2):
        if path is None:
            return
        if path2 is None:
            _write_reads(path, text)
        else:
            first, second = native.split_pairs_fastq(text)
            _write_reads(path, first)
            _write_reads(path2, second)
    write(out, out_path, out_path2)
    if merging:
        write(unmerged or b"", unmerged_path, unmerged_path2)
    from .report import overlap_fragments, write_overlap_summary, write_overlap_tsv
    fragments = overlap_fragments(rows)
    if tsv_path is not None:
        write_overlap_tsv(tsv_path, fastq_names(raw), rows, keep)
    if summary_path is not None:
        write_overlap_summary(summary_path, info, fragments)
    done: Dict[str, object] = {name: value for name, value in info.items() if not name.startswith("s_")}
    done["fragments"] = fragments
    if keep_text:
        done["text"] = out
        if merging:
            done["unmerged"] = unmerged or b""
    return done
