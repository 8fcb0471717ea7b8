"""Drop-in for the table-merging step of lib/mercat2_report.py (``merge_tsv``, lines 98-156, and
``merge_tsv_T``, lines 160-194): the combined sample x k-mer table that feeds the reference's plots
and PCA, and its transpose that beta diversity reads.

``merge_counters`` builds it straight from the samples' tables on the GPU (no TSV re-read);
``merge_tsv`` keeps the reference's signature (a dict of TSV paths) by loading the files into engine
tables first (``Counter.load_tsv``: parsed and inserted on the GPU).  Header ``<first column>\\t<sorted names>``, then one row per k-mer.

Which rows: the reference's streaming merge looks for the next k-mer only among the samples that advanced in
the current step and writes a sample's pending count under the k-mer at hand whenever its own key is not
greater (lib/mercat2_report.py:131-150) -- a key held only by samples that did not advance gets no row of its
own and its count lands in a later row.  ``merge_tsv`` (the reference's name) and the CLI write exactly those
rows (``as_reference=True``), so the file is the one MerCat2 writes; ``as_reference=False`` gives the true union
(every k-mer of any sample, 0 where a sample lacks it).  For tables that share nearly all their keys -- k = 5
over genomes, the reference's committed runs -- the two are the same.  ``merge_tsv_T`` has no such quirk.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

from . import native


def merge_counters(counters: Dict[str, "native.Counter"], out_file, first_column: str = "k-mer",
                   as_reference: bool = True) -> int:
    """Write the combined table of ``{sample name: Counter}``; returns the number of rows written."""
    names = sorted(counters.keys())
    if not names:
        raise ValueError("merge_counters: no samples")
    return native.write_merged_tsv([counters[n] for n in names], names, out_file, first_column, as_reference)


def merge_counters_T(counters: Dict[str, "native.Counter"], out_file) -> int:
    """The transposed table (samples as rows) of ``{sample name: Counter}``; returns the number of k-mer columns.
    Columns are in sorted k-mer order (the reference's order is that of a Python set: arbitrary)."""
    names = sorted(counters.keys())
    if not names:
        raise ValueError("merge_counters_T: no samples")
    return native.write_merged_tsv_T([counters[n] for n in names], names, out_file)


def format_query_tsv(names: Sequence[str], keys: Sequence[bytes], columns: Sequence[Sequence[int]]) -> bytes:
    """The text of a query table: ``k-mer\t<name>...`` then one ``<key>\t<count>...`` line per panel row, in panel order,
    duplicates kept, ``\n`` line ends.  ``columns[j][i]`` is the count of ``keys[i]`` in sample ``names[j]``; the key
    bytes are written as they stand (a key may hold a tab or a blank)."""
    out = [b"k-mer\t" + "\t".join(names).encode() + b"\n"]
    for i, key in enumerate(keys):
        out.append(bytes(key) + b"".join(b"\t%d" % int(col[i]) for col in columns) + b"\n")
    return b"".join(out)


def panel_keys(panel_path, k: int, header: bool) -> list:
    """The keys of a panel in text form (mk_lookup_file's row rules: k key bytes a line, whatever follows them is a
    tab and a count), line 1 left out when it is a header."""
    with open(panel_path, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [line[:k] for line in lines[1 if header else 0:]]


def write_query_tsv(counters: Dict[str, "native.Counter"], panel_path, out_path, fold: bool = False) -> int:
    """How often every k-mer of the panel at ``panel_path`` occurs in each sample of ``{sample name: Counter}``: the panel
    is looked up once per sample in the table on the GPU (``Counter.lookup_text``), the table written to ``out_path`` with
    the names sorted as the combined table sorts them.  Returns the number of panel rows.  MercatHipError (the message
    names the line) for a malformed panel row."""
    names = sorted(counters.keys())
    if not names:
        raise ValueError("write_query_tsv: no samples")
    columns, info = [], None
    for name in names:
        counts, info = counters[name].lookup_text(panel_path, fold=fold)
        columns.append(counts)
    keys = panel_keys(panel_path, counters[names[0]].k, bool(info["header"]))
    if any(len(col) != len(keys) for col in columns):
        raise RuntimeError("write_query_tsv: the panel changed while it was looked up")
    with open(out_path, "wb") as fh:
        fh.write(format_query_tsv(names, keys, columns))
    return len(keys)


def format_histo(bins, full: bool = False) -> bytes:
    """The text of an abundance histogram (``Counter.histo``): one ``<abundance> <k-mers>`` line per bin, a single blank
    between the two, ascending, ``\n`` line ends -- the layout ``jellyfish histo -h HIGH`` documents.  bins[i] is the
    number of distinct k-mers that occur i times, the last bin (abundance high + 1) those that occur more often.  Bins
    that are zero are left out unless ``full`` (bin 0 is never written: no row has count 0)."""
    return b"".join(b"%d %d\n" % (i, int(n)) for i, n in enumerate(bins) if i and (full or int(n)))


def write_histo_files(counters: Dict[str, "native.Counter"], folder, high: int = 10000) -> Dict[str, object]:
    """``<folder>/<name>_histo.txt`` (``format_histo``) for every sample of ``{sample name: Counter}``, each histogram
    reduced in the table on the GPU (``Counter.histo``).  Returns ``{name: bins}``."""
    os.makedirs(folder, exist_ok=True)
    out = {}
    for name in counters:
        out[name] = counters[name].histo(high)
        with open(os.path.join(folder, f"{name}_histo.txt"), "wb") as fh:
            fh.write(format_histo(out[name]))
    return out


def format_histo_tsv(names: Sequence[str], columns: Sequence[Sequence[int]]) -> bytes:
    """The cohort's histograms side by side: ``count\t<name>...``, then one tab-separated row per abundance at which any
    sample's bin is not zero, ascending, the overflow row (abundance high + 1) last.  ``columns[j]`` are the bins of
    ``names[j]``, all of one length."""
    out = [b"count\t" + "\t".join(names).encode() + b"\n"]
    for i in range(1, len(columns[0]) if columns else 0):
        if any(int(col[i]) for col in columns):
            out.append(b"%d" % i + b"".join(b"\t%d" % int(col[i]) for col in columns) + b"\n")
    return b"".join(out)


def write_histo_tsv(counters: Dict[str, "native.Counter"], out_file, high: int = 10000, bins: Optional[dict] = None) -> int:
    """The histograms of ``{sample name: Counter}`` as one table (``format_histo_tsv``), the names in the order given.
    ``bins``: histograms already at hand (``write_histo_files``' result), else they are computed.  Returns the number
    of rows written."""
    names = list(counters.keys())
    if not names:
        raise ValueError("write_histo_tsv: no samples")
    columns = [bins[name] if bins is not None else counters[name].histo(high) for name in names]
    text = format_histo_tsv(names, columns)
    with open(out_file, "wb") as fh:
        fh.write(text)
    return text.count(b"\n") - 1


def format_screen_tsv(names: Sequence[str], array) -> bytes:
    """``record\twindows\thits\tsum\tmin\tmax``, then one line per record: its name and the five integers of its row
    (kmers.screen_reads / Counter.screen)."""
    if len(names) != len(array):
        raise ValueError("format_screen_tsv: %d names for %d rows" % (len(names), len(array)))
    out = [b"record\t" + "\t".join(native.SCREEN_COLUMNS).encode() + b"\n"]
    for name, row in zip(names, array):
        out.append(name.encode() + b"".join(b"\t%d" % int(v) for v in row) + b"\n")
    return b"".join(out)


def write_screen_tsv(path, names: Sequence[str], array) -> int:
    """``format_screen_tsv`` written to ``path``; returns the number of records."""
    text = format_screen_tsv(names, array)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def format_track_txt(names: Sequence[str], counts, offsets) -> bytes:
    """The layout of a FASTA .qual file: a ``>name`` line, then one line with the counts of the record's k-mers in read
    order, separated by single spaces -- an empty line for a record without windows (kmers.track_reads / Counter.track)."""
    if len(names) + 1 != len(offsets):
        raise ValueError("format_track_txt: %d names for %d offsets" % (len(names), len(offsets)))
    out = []
    for i, name in enumerate(names):
        values = counts[int(offsets[i]): int(offsets[i + 1])].tolist()
        out.append(b">" + name.encode() + b"\n" + " ".join(map(str, values)).encode() + b"\n")
    return b"".join(out)


def write_track_txt(path, names: Sequence[str], counts, offsets) -> int:
    """``format_track_txt`` written to ``path``; returns the number of records."""
    text = format_track_txt(names, counts, offsets)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def format_track_median_tsv(names: Sequence[str], rows, median) -> bytes:
    """``record\twindows\tmedian\tsum\tmin\tmax``, then one line per record (kmers.track_reads): its name, its k-mers,
    the median of their counts, and their sum, smallest and largest from its screen row."""
    if len(names) != len(rows) or len(names) != len(median):
        raise ValueError("format_track_median_tsv: %d names for %d rows and %d medians" % (len(names), len(rows), len(median)))
    out = [b"record\twindows\tmedian\tsum\tmin\tmax\n"]
    for name, row, med in zip(names, rows, median):
        out.append(name.encode() + b"\t%d\t%d\t%d\t%d\t%d\n" % (int(row[0]), int(med), int(row[2]), int(row[3]), int(row[4])))
    return b"".join(out)


def write_track_median_tsv(path, names: Sequence[str], rows, median) -> int:
    """``format_track_median_tsv`` written to ``path``; returns the number of records."""
    text = format_track_median_tsv(names, rows, median)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


_EMITTED = (b"0", b"pair", b"single")  # keep[r] of Counter.pairs


def format_trim_tsv(names: Sequence[str], lengths, kept, keep=None) -> bytes:
    """``record\tlength\tkept``, then one line per record (kmers.trim_reads / Counter.trim): its name, the characters it
    came with and those it keeps (0: dropped).  A paired run (``keep``: Counter.trim_pairs' 0 / 1 / 2 a record) adds the
    columns ``emitted`` -- ``0``, ``pair`` or ``single``; ``kept`` stays the mate's own figure -- and ``pair``, the pair's
    index."""
    if len(names) != len(lengths) or len(names) != len(kept) or (keep is not None and len(keep) != len(names)):
        raise ValueError("format_trim_tsv: %d names for %d lengths and %d kept" % (len(names), len(lengths), len(kept)))
    if keep is None:
        out = [b"record\tlength\tkept\n"]
        for name, length, k in zip(names, lengths, kept):
            out.append(name.encode() + b"\t%d\t%d\n" % (int(length), int(k)))
        return b"".join(out)
    out = [b"record\tlength\tkept\temitted\tpair\n"]
    for r, (name, length, k, e) in enumerate(zip(names, lengths, kept, keep)):
        out.append(name.encode() + b"\t%d\t%d\t%s\t%d\n" % (int(length), int(k), _EMITTED[int(e)], r // 2))
    return b"".join(out)


def write_trim_tsv(path, names: Sequence[str], lengths, kept, keep=None) -> int:
    """``format_trim_tsv`` written to ``path``; returns the number of records."""
    text = format_trim_tsv(names, lengths, kept, keep)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def format_orf_tsv(names: Sequence[str], rows) -> bytes:
    """``record\tname\tbegin\tend\tstrand\tframe\taa``, then one line per ORF (kmers.orf_reads / Counter.orfs): the number
    of its record in the text, that record's name (``names[record]``), where it lies on the forward strand -- 0-based,
    half open, ``end - begin == 3 * aa`` --, ``+`` for frames 1 to 3 and ``-`` for 4 to 6, the frame and its amino
    acids."""
    out = [b"record\tname\tbegin\tend\tstrand\tframe\taa\n"]
    for row in rows:
        record, begin, aa, frame = (int(v) for v in row)
        if not 0 <= record < len(names):
            raise ValueError("format_orf_tsv: record %d of %d names" % (record, len(names)))
        name = names[record]
        name = name if isinstance(name, bytes) else name.encode()
        out.append(b"%d\t%s\t%d\t%d\t%s\t%d\t%d\n" % (record, name, begin, begin + 3 * aa, b"+" if frame < 4 else b"-", frame, aa))
    return b"".join(out)


def write_orf_tsv(path, names: Sequence[str], rows) -> int:
    """``format_orf_tsv`` written to ``path``; returns the number of ORFs."""
    text = format_orf_tsv(names, rows)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(rows)


def format_correct_tsv(names: Sequence[str], lengths, fix) -> bytes:
    """``record\tlength\truns\tfixed\tambiguous\tunfixable``, then one line per record (kmers.correct_reads /
    Counter.correct): its name, its characters and the four columns of its ``fix`` row."""
    if len(names) != len(lengths) or len(names) != len(fix):
        raise ValueError("format_correct_tsv: %d names for %d lengths and %d fix rows" % (len(names), len(lengths), len(fix)))
    out = [b"record\tlength\truns\tfixed\tambiguous\tunfixable\n"]
    for name, length, row in zip(names, lengths, fix):
        runs, fixed, ambiguous, unfixable = (int(v) for v in row)
        out.append(name.encode() + b"\t%d\t%d\t%d\t%d\t%d\n" % (int(length), runs, fixed, ambiguous, unfixable))
    return b"".join(out)


def write_correct_tsv(path, names: Sequence[str], lengths, fix) -> int:
    """``format_correct_tsv`` written to ``path``; returns the number of records."""
    text = format_correct_tsv(names, lengths, fix)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def format_norm_tsv(names: Sequence[str], windows, median, kept, paired: bool = False) -> bytes:
    """``record\twindows\tmedian\tkept``, then one line per record (kmers.normalize_reads / Counter.normalize): its name,
    its k-mers, the median of their counts and 1 where the record was written, 0 where not.  A ``paired`` run adds a last
    column ``pair``, the pair's index."""
    if not len(names) == len(windows) == len(median) == len(kept):
        raise ValueError("format_norm_tsv: %d names for %d windows, %d medians and %d kept" % (len(names), len(windows), len(median), len(kept)))
    out = [b"record\twindows\tmedian\tkept\tpair\n" if paired else b"record\twindows\tmedian\tkept\n"]
    for r, (name, w, m, k) in enumerate(zip(names, windows, median, kept)):
        out.append(name.encode() + b"\t%d\t%d\t%d" % (int(w), int(m), 1 if k else 0) + (b"\t%d\n" % (r // 2) if paired else b"\n"))
    return b"".join(out)


def write_norm_tsv(path, names: Sequence[str], windows, median, kept, paired: bool = False) -> int:
    """``format_norm_tsv`` written to ``path``; returns the number of records."""
    text = format_norm_tsv(names, windows, median, kept, paired)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def write_against_tsvs(tables: Dict[str, "native.Counter"], against, op, out_dir, min_other: int = 1) -> Dict[str, int]:
    """For every sample of ``{sample name: Counter}``, ``sample op against`` (Counter.combine, keys compared as they
    stand) written as ``out_dir/<sample>_counts.tsv`` with Counter.write_tsv; a sample whose result is empty writes no
    file, as everywhere.  ``against``: a Counter, or the path of a counts TSV (a Jellyfish / KMC dump) of the samples'
    k-mer length, which is loaded once per device the tables are on.  A count of ``against`` below ``min_other`` is
    taken as absent.  Returns {sample name: rows of its result}."""
    os.makedirs(out_dir, exist_ok=True)
    loaded = {}  # device -> the background table there
    rows = {}
    try:
        for name, table in tables.items():
            other = against
            if not isinstance(against, native.Counter):
                if table.device not in loaded:
                    loaded[table.device] = native.Counter(table.k, table.alphabet, table.device, canonical=table.canonical)
                    loaded[table.device].load_tsv(against)
                other = loaded[table.device]
            with table.combine(other, op, 1, min_other) as result:
                rows[name] = result.rows()
                if rows[name]:
                    result.write_tsv(os.path.join(out_dir, f"{name}_counts.tsv"), name)
    finally:
        for c in loaded.values():
            c.close()
    return rows


def _first_header_field(path, shape: dict) -> Optional[str]:
    """The first field of a count table's header line (the combined table's first column title); None without one."""
    if not shape["header"]:
        return None
    with open(path, "rb") as fh:
        return fh.readline().decode().split("\t")[0]


def merge_tsv_T(tsv_list: Dict[str, os.PathLike], out_file: os.PathLike, *, device: int = 0) -> None:
    """merge_tsv_T(tsv_list, out_file) of lib/mercat2_report.py:160-194 (same arguments): ``sample`` + one column per
    k-mer of any sample, one row per sample (sorted names), 0 where a sample lacks the k-mer."""
    _merge_files(tsv_list, out_file, device, transposed=True)


def merge_tsv(tsv_list: Dict[str, os.PathLike], out_file: os.PathLike, *, device: int = 0) -> None:
    """merge_tsv(tsv_list, out_file) of lib/mercat2_report.py:98-156 (same arguments)."""
    _merge_files(tsv_list, out_file, device, transposed=False)


def _merge_files(tsv_list, out_file, device: int, transposed: bool) -> None:
    names = sorted(tsv_list.keys())
    header: Optional[str] = None
    ctxs = []
    try:
        # one alphabet and one k for all tables of the call: those of the first file that has rows
        shapes = [native.tsv_shape(tsv_list[name]) for name in names]
        first = next((s for s in shapes if s["k"]), None)
        k, alphabet = (first["k"], first["alphabet"]) if first else (1, native.ALPHABET_RAW)
        if names:
            header = _first_header_field(tsv_list[names[0]], shapes[0])
        for name, shape in zip(names, shapes):
            c = native.Counter(k, alphabet, device)
            ctxs.append(c)
            if shape["k"]:
                c.load_tsv(tsv_list[name])
        if transposed:
            native.write_merged_tsv_T(ctxs, names, out_file)
        else:
            native.write_merged_tsv(ctxs, names, out_file, header or "k-mer", as_reference=True)
    finally:
        for c in ctxs:
            c.close()


def format_qtrim_tsv(names: Sequence[str], rows, keep) -> bytes:
    """``record\tlength\tstart\tkept\tn\tlow\tqsum\tkeep``, then one line per record (kmers.qtrim_reads /
    Counter.fastq_qtrim): its name, the six columns of its row and its keep value."""
    if len(names) != len(rows) or len(names) != len(keep):
        raise ValueError("format_qtrim_tsv: %d names for %d rows and %d keep values" % (len(names), len(rows), len(keep)))
    out = [b"record\tlength\tstart\tkept\tn\tlow\tqsum\tkeep\n"]
    for name, row, k in zip(names, rows, keep):
        out.append(name.encode() + b"\t%d\t%d\t%d\t%d\t%d\t%d" % tuple(int(v) for v in row) + b"\t%d\n" % int(k))
    return b"".join(out)


def write_qtrim_tsv(path, names: Sequence[str], rows, keep) -> int:
    """``format_qtrim_tsv`` written to ``path``; returns the number of records."""
    text = format_qtrim_tsv(names, rows, keep)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def format_qtrim_summary(figures: Dict[str, int], hist) -> bytes:
    """``metric\tbefore\tafter`` over reads, bases, q20_bases, q30_bases and mean_quality -- from the call's figures and
    its two histograms (hist[0][v]: bases of quality v in the text, hist[1][v]: in the emitted spans) -- then the four
    drop counts and the orphans, which have no "before".  The mean is written with four decimals."""
    def side(h, reads):
        bases = sum(int(c) for c in h)
        q20 = sum(int(c) for v, c in enumerate(h) if v >= 20)
        q30 = sum(int(c) for v, c in enumerate(h) if v >= 30)
        mean = sum(v * int(c) for v, c in enumerate(h)) / bases if bases else 0.0
        return [b"%d" % reads, b"%d" % bases, b"%d" % q20, b"%d" % q30, b"%.4f" % mean]
    before, after = side(hist[0], int(figures["records"])), side(hist[1], int(figures["records_out"]))
    out = [b"metric\tbefore\tafter\n"]
    for name, b, a in zip((b"reads", b"bases", b"q20_bases", b"q30_bases", b"mean_quality"), before, after):
        out.append(name + b"\t" + b + b"\t" + a + b"\n")
    for name in ("dropped_short", "dropped_n", "dropped_lowq", "dropped_meanq", "orphans"):
        out.append(name.encode() + b"\t\t%d\n" % int(figures[name]))
    return b"".join(out)


def write_qtrim_summary(path, figures: Dict[str, int], hist) -> None:
    """``format_qtrim_summary`` written to ``path``."""
    with open(path, "wb") as fh:
        fh.write(format_qtrim_summary(figures, hist))


def format_adapt_tsv(names: Sequence[str], rows, keep, adapter_names: Sequence[str]) -> bytes:
    """``record\tlength\tkept\tadapter\toverlap\tmismatches\tkeep``, then one line per record (kmers.adapt_reads /
    Counter.fastq_adapt): its name, its row -- the adapter by its name, ``-`` without a hit -- and its keep value."""
    if len(names) != len(rows) or len(names) != len(keep):
        raise ValueError("format_adapt_tsv: %d names for %d rows and %d keep values" % (len(names), len(rows), len(keep)))
    out = [b"record\tlength\tkept\tadapter\toverlap\tmismatches\tkeep\n"]
    for name, row, k in zip(names, rows, keep):
        length, kept, adapter, overlap, mism = (int(v) for v in row)
        which = "-" if adapter == 0xFFFFFFFF else adapter_names[adapter]
        out.append(name.encode() + b"\t%d\t%d\t" % (length, kept) + which.encode() + b"\t%d\t%d\t%d\n" % (overlap, mism, int(k)))
    return b"".join(out)


def write_adapt_tsv(path, names: Sequence[str], rows, keep, adapter_names: Sequence[str]) -> int:
    """``format_adapt_tsv`` written to ``path``; returns the number of records."""
    text = format_adapt_tsv(names, rows, keep, adapter_names)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def format_adapt_summary(figures: Dict[str, int], hits, adapter_names: Sequence[str]) -> bytes:
    """``metric\tbefore\tafter`` over reads and bases, then trimmed (emitted reads that were cut), dropped_short and
    orphans, which have no "before", then ``adapter:<name>`` with the reads it cut (emitted or not) for every adapter
    that cut any, in panel order."""
    out = [b"metric\tbefore\tafter\n",
           b"reads\t%d\t%d\n" % (int(figures["records"]), int(figures["records_out"])),
           b"bases\t%d\t%d\n" % (int(figures["bases_in"]), int(figures["bases_out"]))]
    for name, key in (("trimmed", "records_trimmed"), ("dropped_short", "dropped_short"), ("orphans", "orphans")):
        out.append(name.encode() + b"\t\t%d\n" % int(figures[key]))
    for name, h in zip(adapter_names, hits):
        if int(h):
            out.append(b"adapter:" + name.encode() + b"\t\t%d\n" % int(h))
    return b"".join(out)


def write_adapt_summary(path, figures: Dict[str, int], hits, adapter_names: Sequence[str]) -> None:
    """``format_adapt_summary`` written to ``path``."""
    with open(path, "wb") as fh:
        fh.write(format_adapt_summary(figures, hits, adapter_names))


def format_overlap_tsv(names: Sequence[str], rows, keep) -> bytes:
    """``record\tlength\tkept\tfragment\toverlap\tmismatches\tkeep``, then one line per record (kmers.overlap_reads /
    Counter.fastq_overlap): its name, its row -- the fragment ``-`` without a hit -- and its keep value."""
    if len(names) != len(rows) or len(names) != len(keep):
        raise ValueError("format_overlap_tsv: %d names for %d rows and %d keep values" % (len(names), len(rows), len(keep)))
    out = [b"record\tlength\tkept\tfragment\toverlap\tmismatches\tkeep\n"]
    for name, row, k in zip(names, rows, keep):
        length, kept, fragment, overlap, mism = (int(v) for v in row)
        frag = b"-" if fragment == 0xFFFFFFFF else b"%d" % fragment
        out.append(name.encode() + b"\t%d\t%d\t" % (length, kept) + frag + b"\t%d\t%d\t%d\n" % (overlap, mism, int(k)))
    return b"".join(out)


def write_overlap_tsv(path, names: Sequence[str], rows, keep) -> int:
    """``format_overlap_tsv`` written to ``path``; returns the number of records."""
    text = format_overlap_tsv(names, rows, keep)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def overlap_fragments(rows) -> Dict[int, int]:
    """{fragment length: pairs} over the pairs with a hit, in ascending order, from Counter.fastq_overlap's rows (the
    row of every first mate)."""
    counts: Dict[int, int] = {}
    for row in rows[0::2]:
        fragment = int(row[2])
        if fragment != 0xFFFFFFFF:
            counts[fragment] = counts.get(fragment, 0) + 1
    return dict(sorted(counts.items()))


def format_overlap_summary(figures: Dict[str, int], fragments: Dict[int, int]) -> bytes:
    """``metric\tbefore\tafter`` over reads and bases, then the pair counts, which have no "before" -- pairs, hits, merged,
    trimmed, dropped_short, skipped_long -- then ``fragment\tpairs`` and one line per fragment length that occurs."""
    out = [b"metric\tbefore\tafter\n",
           b"reads\t%d\t%d\n" % (int(figures["records"]), int(figures["records_out"])),
           b"bases\t%d\t%d\n" % (int(figures["bases_in"]), int(figures["bases_out"]))]
    for name, key in (("pairs", "pairs"), ("hits", "pairs_hit"), ("merged", "pairs_merged"), ("trimmed", "pairs_trimmed"),
                      ("dropped_short", "dropped_short"), ("skipped_long", "skipped_long")):
        out.append(name.encode() + b"\t\t%d\n" % int(figures[key]))
    out.append(b"fragment\tpairs\n")
    for fragment, pairs in fragments.items():
        out.append(b"%d\t%d\n" % (int(fragment), int(pairs)))
    return b"".join(out)


def write_overlap_summary(path, figures: Dict[str, int], fragments: Dict[int, int]) -> None:
    """``format_overlap_summary`` written to ``path``."""
    with open(path, "wb") as fh:
        fh.write(format_overlap_summary(figures, fragments))


# ---- the quality-control tables of Counter.fastq_qc / kmers.qc_reads as TSVs: pure Python over the arrays.  ``mate``: 0 for
# ---- a text read as one class, 1 and 2 for the mates of a paired one
def _qc_mates(qc) -> list:
    classes = len(qc["read_len"])
    return [(c, c + 1 if classes == 2 else 0) for c in range(classes)]


def qc_percentile(hist, x: int) -> int:
    """The smallest value v with 100 * (hist[0] + .. + hist[v]) >= x * sum(hist); 0 for an empty histogram."""
    total, cum = sum(int(n) for n in hist), 0
    for v, n in enumerate(hist):
        cum += int(n)
        if total and 100 * cum >= x * total:
            return v
    return 0


def qc_mean(hist) -> float:
    """sum(v * hist[v]) / sum(hist); 0.0 for an empty histogram."""
    total = sum(int(n) for n in hist)
    return sum(v * int(n) for v, n in enumerate(hist)) / total if total else 0.0


def format_qc_cycles(qc) -> bytes:
    """``mate\tcycle\tbases\tmean\tp10\tq1\tmedian\tq3\tp90\tA\tC\tG\tT\tN\tother``, one line per mate and row of
    pos_qual / pos_base that holds a base: the cycle counted from 1 (the row that collects the cycles behind max_pos = P
    is written ``>P``), its bases, their mean quality with two decimals, the qualities at 10, 25, 50, 75 and 90 per cent
    (qc_percentile) and the bases of each class."""
    out = [b"mate\tcycle\tbases\tmean\tp10\tq1\tmedian\tq3\tp90\tA\tC\tG\tT\tN\tother\n"]
    for c, mate in _qc_mates(qc):
        P = len(qc["pos_qual"][c]) - 1
        for p in range(P + 1):
            hist = [int(n) for n in qc["pos_qual"][c][p]]
            bases = sum(hist)
            if not bases:
                continue
            cycle = b">%d" % P if p == P else b"%d" % (p + 1)
            marks = tuple(qc_percentile(hist, x) for x in (10, 25, 50, 75, 90))
            out.append(b"%d\t" % mate + cycle + b"\t%d\t%.2f" % (bases, qc_mean(hist)) + b"\t%d\t%d\t%d\t%d\t%d" % marks +
                       b"\t%d\t%d\t%d\t%d\t%d\t%d\n" % tuple(int(n) for n in qc["pos_base"][c][p][:6]))
    return b"".join(out)


def format_qc_quality(qc) -> bytes:
    """``mate\tmean_quality\treads``: the reads of every mean quality (rounded down) that occurs."""
    out = [b"mate\tmean_quality\treads\n"]
    for c, mate in _qc_mates(qc):
        out += [b"%d\t%d\t%d\n" % (mate, m, int(n)) for m, n in enumerate(qc["read_qual"][c]) if int(n)]
    return b"".join(out)


def format_qc_gc(qc) -> bytes:
    """``mate\tgc\treads``: the reads of every GC share in per cent (rounded half up), all 101 lines a mate."""
    out = [b"mate\tgc\treads\n"]
    for c, mate in _qc_mates(qc):
        out += [b"%d\t%d\t%d\n" % (mate, g, int(n)) for g, n in enumerate(qc["read_gc"][c])]
    return b"".join(out)


def format_qc_length(qc) -> bytes:
    """``mate\tlength\treads``: the reads of every length that occurs; the last bin, the reads longer than max_pos = P,
    is written ``>P``."""
    out = [b"mate\tlength\treads\n"]
    for c, mate in _qc_mates(qc):
        P = len(qc["read_len"][c]) - 2
        for l, n in enumerate(qc["read_len"][c]):
            if int(n):
                out.append(b"%d\t" % mate + (b">%d" % P if l == P + 1 else b"%d" % l) + b"\t%d\n" % int(n))
    return b"".join(out)


def format_qc_summary(qc) -> bytes:
    """``metric`` and a column a mate (``all`` for a text read as one class, else ``mate1`` and ``mate2``): reads, bases,
    empty_reads, min_length, mean_length (two decimals), max_length (a length behind max_pos = P is written ``>P``),
    gc_percent (two decimals, of all bases), n_bases, q20_bases, q30_bases, mean_quality (two decimals)."""
    mates = _qc_mates(qc)
    cols = []
    for c, _ in mates:
        lens = [int(n) for n in qc["read_len"][c]]
        P = len(lens) - 2
        name = lambda l: b">%d" % P if l == P + 1 else b"%d" % l
        seen = [l for l, n in enumerate(lens) if n]
        quals = [sum(int(row[v]) for row in qc["pos_qual"][c]) for v in range(len(qc["pos_qual"][c][0]))]
        kinds = [sum(int(row[k]) for row in qc["pos_base"][c]) for k in range(6)]
        reads, bases = sum(lens), sum(quals)
        cols.append([b"%d" % reads, b"%d" % bases, b"%d" % lens[0], name(seen[0]) if seen else b"0",
                     b"%.2f" % (bases / reads if reads else 0.0), name(seen[-1]) if seen else b"0",
                     b"%.2f" % (100.0 * (kinds[1] + kinds[2]) / bases if bases else 0.0), b"%d" % kinds[4],
                     b"%d" % sum(quals[20:]), b"%d" % sum(quals[30:]), b"%.2f" % qc_mean(quals)])
    out = [b"metric\t" + (b"all" if len(mates) == 1 else b"mate1\tmate2") + b"\n"]
    for i, metric in enumerate((b"reads", b"bases", b"empty_reads", b"min_length", b"mean_length", b"max_length", b"gc_percent",
                                b"n_bases", b"q20_bases", b"q30_bases", b"mean_quality")):
        out.append(metric + b"".join(b"\t" + col[i] for col in cols) + b"\n")
    return b"".join(out)


QC_FILES = {"cycles": format_qc_cycles, "quality": format_qc_quality, "gc": format_qc_gc, "length": format_qc_length,
            "summary": format_qc_summary}


def write_qc_files(prefix, qc) -> list:
    """``<prefix>_cycles.tsv``, ``_quality.tsv``, ``_gc.tsv``, ``_length.tsv`` and ``_summary.tsv`` of the tables of
    Counter.fastq_qc; returns the paths."""
    paths = []
    for name, fmt in QC_FILES.items():
        paths.append("%s_%s.tsv" % (prefix, name))
        with open(paths[-1], "wb") as fh:
            fh.write(fmt(qc))
    return paths


# ---- -dedup: duplicate reads (kmers.dedup_reads / Counter.fastq_dedup) ----
DEDUP_OVER_LIMIT = 1000  # rows of _overrepresented.tsv at most


def dedup_copies(rows, paired: bool = False) -> list:
    """copies[r]: the units (reads, or pairs with ``paired``) of the cluster of record r, from the ``first`` column of
    Counter.fastq_dedup's rows (pure Python; kmers.dedup_reads counts with numpy)."""
    firsts = [int(row[1]) for row in rows]
    size: Dict[int, int] = {}
    for r, f in enumerate(firsts):
        if not paired or not r & 1:
            size[f] = size.get(f, 0) + 1
    return [size[f - (f & 1) if paired else f] for f in firsts]


def dedup_over(copies, rows, paired: bool = False, over_frac: float = 0.001, limit: int = DEDUP_OVER_LIMIT) -> list:
    """[(first record, copies)] of the over-represented clusters: those that hold at least ``over_frac`` of the units
    and more than one of them, by copies descending, then by first ascending, ``limit`` of them at most.  With
    ``paired`` the first record is the pair's first mate."""
    step = 2 if paired else 1
    units = len(rows) // step
    found = [(int(rows[r][1]), int(copies[r])) for r in range(0, len(rows), step) if int(rows[r][1]) == r]
    found = [(f, n) for f, n in found if n > 1 and n >= over_frac * units]
    found.sort(key=lambda x: (-x[1], x[0]))
    return found[:limit]


def format_dedup_tsv(names: Sequence[str], rows, keep, copies) -> bytes:
    """``record\tlength\tfirst\tcopies\tkeep``, then one line per record (kmers.dedup_reads / Counter.fastq_dedup): its
    name, its length, the name of the record that stands for it, the size of its cluster and its keep value."""
    if len(names) != len(rows) or len(names) != len(keep) or len(names) != len(copies):
        raise ValueError("format_dedup_tsv: %d names for %d rows, %d keep values and %d copies" %
                         (len(names), len(rows), len(keep), len(copies)))
    out = [b"record\tlength\tfirst\tcopies\tkeep\n"]
    for name, row, k, n in zip(names, rows, keep, copies):
        out.append(name.encode() + b"\t%d\t" % int(row[0]) + names[int(row[1])].encode() + b"\t%d\t%d\n" % (int(n), int(k)))
    return b"".join(out)


def write_dedup_tsv(path, names: Sequence[str], rows, keep, copies) -> int:
    """``format_dedup_tsv`` written to ``path``; returns the number of records."""
    text = format_dedup_tsv(names, rows, keep, copies)
    with open(path, "wb") as fh:
        fh.write(text)
    return len(names)


def format_dedup_levels(levels, units: int) -> bytes:
    """``copies\tsequences\treads\tpercent_of_reads``: for every level 1 .. high that occurs the clusters of that many
    copies, the units they hold and their share of all ``units`` (reads, or pairs) with four decimals; the last row,
    always written, is ``>high``: its units are those the other rows do not hold."""
    high = len(levels) - 2
    share = lambda n: b"%.4f" % (100.0 * n / units if units else 0.0)
    out, held = [b"copies\tsequences\treads\tpercent_of_reads\n"], 0
    for i in range(1, high + 1):
        if int(levels[i]):
            n = i * int(levels[i])
            held += n
            out.append(b"%d\t%d\t%d\t" % (i, int(levels[i]), n) + share(n) + b"\n")
    out.append(b">%d\t%d\t%d\t" % (high, int(levels[high + 1]), int(units) - held) + share(int(units) - held) + b"\n")
    return b"".join(out)


def write_dedup_levels(path, levels, units: int) -> None:
    """``format_dedup_levels`` written to ``path``."""
    with open(path, "wb") as fh:
        fh.write(format_dedup_levels(levels, units))


def format_dedup_summary(figures: Dict[str, int], paired: bool = False) -> bytes:
    """``metric\tvalue``: reads (``pairs`` with ``paired``), distinct, duplicates (units that are not the first of their
    cluster), duplication_rate (duplicates / units, six decimals), largest_cluster, bases_before and bases_after -- from
    the mk_fastq_dedup_t figures of a call with which = 1."""
    units = int(figures["records"]) // (2 if paired else 1)
    dup = units - int(figures["distinct"])
    rows = [(b"pairs" if paired else b"reads", b"%d" % units), (b"distinct", b"%d" % int(figures["distinct"])),
            (b"duplicates", b"%d" % dup), (b"duplication_rate", b"%.6f" % (dup / units if units else 0.0)),
            (b"largest_cluster", b"%d" % int(figures["max_copies"])), (b"bases_before", b"%d" % int(figures["bases_in"])),
            (b"bases_after", b"%d" % int(figures["bases_out"]))]
    return b"metric\tvalue\n" + b"".join(k + b"\t" + v + b"\n" for k, v in rows)


def write_dedup_summary(path, figures: Dict[str, int], paired: bool = False) -> None:
    """``format_dedup_summary`` written to ``path``."""
    with open(path, "wb") as fh:
        fh.write(format_dedup_summary(figures, paired))


def format_dedup_over(over, names: Sequence[str], seqs: Sequence[bytes], units: int, paired: bool = False) -> bytes:
    """``first\tcopies\tpercent\tsequence`` (and ``sequence2`` with ``paired``): one line per (first record, copies) of
    ``over`` (dedup_over, whose order is kept): the name of the first record, the copies, their share of all ``units``
    with four decimals, and the key of that record (of both mates); ``seqs[r]`` is the key of record r."""
    out = [b"first\tcopies\tpercent\tsequence" + (b"\tsequence2" if paired else b"") + b"\n"]
    for first, n in over:
        out.append(names[first].encode() + b"\t%d\t%.4f\t" % (n, 100.0 * n / units if units else 0.0) + bytes(seqs[first]) +
                   (b"\t" + bytes(seqs[first + 1]) if paired else b"") + b"\n")
    return b"".join(out)


def write_dedup_over(path, over, names: Sequence[str], seqs: Sequence[bytes], units: int, paired: bool = False) -> int:
    """``format_dedup_over`` written to ``path``; returns the number of rows."""
    with open(path, "wb") as fh:
        fh.write(format_dedup_over(over, names, seqs, units, paired))
    return len(over)
