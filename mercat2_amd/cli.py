"""Command line of the counting path, flag-compatible with bin/mercat2.py (lines 41-50, 68-79,
207-215, 253-283, 312-346, 411-448 of the reference): -i/-f/-k/-n/-c/-s/-o/-replace.

The count phase and what stands directly in front of and behind it: inputs are
FASTA (nucleotide or protein; plain or .gz); nucleotide inputs go through removeN first unless
-skipclean is given (bin/mercat2.py:239-244), exactly as in the reference; the combined tables are
written after counting.  -tsv DIR takes the samples of an earlier output folder (its
tsv_<type>/<sample>_counts.tsv files) as they are: their tables are loaded onto the GPU instead of being counted, so a
cohort grows by one sample, or gets its -pca / -union reports, without recounting.  FASTQ input (.fq, .fastq, plain or .gz) is taken with -skipclean: MerCat2 then
converts it with fq2fa only (lib/mercat2_fasta.py:175-198) into clean/<base>.fna.gz and counts that as a
nucleotide sample; here the GPU counts the raw reads the same way while the file is written.  Without
-skipclean MerCat2 trims the reads with fastp first, a tool this engine does not run: refused, unless -qtrim puts the
engine's own quality trimming in that place (below).  With -pca and
more than three samples of a type, pca_<type>/pca.tsv is computed from the tables still on the GPU
(bin/mercat2.py:170-181, lib/mercat2_figures.py:206-291; mercat2_amd/pca.py): exact PCA, no plots.  The diversity
reports are written from the tables on the GPU too (mercat2_amd/diversity.py): the 21 beta-diversity matrices per
sample type (report/diversity/<metric>-Nucleotide.tsv, report/beta_diversity/<metric>-protein.tsv; no heatmaps;
skipped beyond 4096 samples), each sample's alpha metrics (report/diversity/<type>-<sample>.tsv) and, with two or
more samples, report/diversity-<type>.tsv.  -query FILE writes query_<type>.tsv: the count of every k-mer of a panel in every
sample, looked up in those tables (mk_lookup_file).  -histo [HIGH] writes every sample's abundance histogram
(histo_<type>/<sample>_histo.txt, histo_<type>.tsv), reduced in those tables (mk_histo).  -screen FILE writes, for every
sample of FILE's type, screen_<type>/<sample>_screen.tsv: per record of FILE its k-mers, how many of them the sample's table
holds, and how abundant they are (mk_screen_text).  -filter FILE writes, for every sample of FILE's type,
filter_<type>/<sample>_<matched|unmatched>.fna (.faa): the records of FILE that share k-mers with the sample's table, or those
that do not, copied out on the GPU (mk_filter_text).  -track FILE writes, for every sample of FILE's type,
track_<type>/<sample>_track.txt -- per record of FILE the count of every one of its k-mers in the sample's table, in read
order -- and track_<type>/<sample>_median.tsv with the median of those counts (mk_track_text).  -trim FILE writes, for every
sample of FILE's type, trim_<type>/<sample>_trimmed.fna (.faa): every record of FILE cut in front of its first k-mer the
sample's table holds fewer than -trim_min times, as khmer's filter-abund trims (mk_trim_text), and
trim_<type>/<sample>_trim.tsv with every record's length and what it keeps.  -correct FILE writes, for every nucleotide
sample, correct_<type>/<sample>_corrected.fna: every record of FILE with the single wrong bases put right that the sample's
table can name -- a run of k-mers held fewer than -correct_min times, shaped as one substitution shapes it, and exactly one
base that makes them all solid (mk_correct_text) -- and correct_<type>/<sample>_correct.tsv with every record's runs and what
became of them; -correct_mate FILE2 corrects two files of mates together and writes ..._1 and ..._2; -correct_fastq reads a
FASTQ FILE on the GPU as it stands and writes correct_<type>/<sample>_corrected.fastq, the same text with the fixed bases and
the qualities where they were (mk_correct_fastq_text), -correct_qual C writing C over the quality of every fixed base.
-norm FILE writes, for every sample of FILE's
type, norm_<type>/<sample>_<kept|tossed>.fna (.faa): the records of FILE thinned to depth -norm_target by the median of their
k-mers' counts in the sample's table -- digital normalisation, BBNorm's count-first plan with khmer's depth (mk_norm_text) --
and norm_<type>/<sample>_norm.tsv with every record's k-mers, depth and fate.  Paired reads: with -paired the FILE of
-filter, -trim and -norm is interleaved, with -filter_mate / -trim_mate / -norm_mate FILE2 the pair comes in two files
(interleaved on the host, written back as ..._1 and ..._2); either way a pair is written or left out as a whole
(mk_pairs_text), -filter_pair says whether one matching mate is enough, -singles also writes <sample>_singles.fna (.faa)
and the per-record TSVs gain the pair's index.  -fastq_out makes -filter, -trim and -norm of a FASTQ FILE write FASTQ with
the qualities (.fastq in place of .fna; mk_fastq_select_text).  -against FILE -op OP writes, for every sample of FILE's type,
against/tsv_<type>/<sample>_counts.tsv: the sample's table combined by key with the count table FILE on the GPU
(mk_table_op) -- a folder a next run takes with -tsv.  -qtrim [Q] takes FASTQ input with or without -skipclean and, where
MerCat2 would run fastp, trims and filters the reads on the GPU by a stated rule (mk_fastq_qtrim_text: the running-sum
quality cut of BWA -q / cutadapt -q at the 3' end, with -qtrim_front at the 5' end too, then -qtrim_len, -qtrim_n,
-qtrim_low / -qtrim_low_frac and -qtrim_mean): qtrim/<sample>_qtrim.fastq holds the reads that are then counted,
qtrim/<sample>_qtrim.tsv every read's length, cut and verdict, qtrim/<sample>_summary.tsv reads, bases, Q20 / Q30 bases and
mean quality before and after.  The result is that rule's, not fastp's: no adapters are removed by it.  -adapt [FILE] does
that, before -qtrim where both are given, again by a stated rule (mk_fastq_adapt_text: the 3' adapter search of cutadapt -a
--no-indels at its leftmost admissible position, over -adapt_overlap bases within -adapt_err mismatches a base, reads left
shorter than -adapt_len dropped) against the adapters of the FASTA FILE or, without one, Illumina's TruSeq, Nextera and
small-RNA adapters: adapt/<sample>_adapt.fastq holds the reads that -qtrim and the count then see, adapt/<sample>_adapt.tsv
every read's length, cut, adapter, overlap and mismatches, adapt/<sample>_summary.tsv reads and bases before and after and
the hits of each adapter.  -overlap trim|merge does the paired-end half of that fastp run, before -adapt and -qtrim: every
FASTQ input is interleaved pairs (or, with -overlap_mate FILE2, the first of two files), mate 1 is laid against the reverse
complement of mate 2 (mk_fastq_overlap_text: the first offset, longest overlap first and read-through last, with -overlap_min
bases within -overlap_diff mismatches and -overlap_err mismatches a base), and a pair that overlaps is cut to its fragment
-- adapters gone without a panel -- or merged into one read with a consensus over the overlap; overlap/<sample>_overlap.fastq,
or _merged.fastq and _unmerged.fastq, hold what -adapt, -qtrim and the count then see, overlap/<sample>_overlap.tsv every
read's length, cut, fragment, overlap and mismatches, overlap/<sample>_summary.tsv the pair counts and the fragment lengths.
Indels (in adapters and in the overlap), 5' and anchored adapters, quality-aware correction of unmerged mates (fastp -c) and
poly-G trimming stay out.  -qc [MAXPOS] stands where MerCat2 runs fastqc, on the reads as read and again on the trimmed
reads: for every FASTQ sample (which still needs -skipclean or one of the steps above) the GPU reduces the text to per-cycle
and per-read tables (mk_fastq_qc_text: at every cycle the bases of every quality value and of A, C, G, T, N and anything
else, cycles from MAXPOS on in one row; per read its length, mean quality and GC share), written as
qc/<sample>_raw_cycles.tsv (bases, mean, percentiles and composition a cycle), _quality.tsv, _gc.tsv, _length.tsv and
_summary.tsv, and as qc/<sample>_clean_*.tsv from what the count sees where -overlap, -adapt or -qtrim ran.  -qc_paired or
-overlap gives every figure per mate (the clean stage only while mates still alternate: not after -overlap merge, -adapt or
-qtrim); -qc_phred sets the offset.  The figures are that stated rule's, not fastqc's: adapter and k-mer content, position
grouping and verdicts stay out.  -dedup takes FASTQ input with or without -skipclean and removes duplicate reads on the GPU
first of all, before -overlap, -adapt and -qtrim (trimming makes copies of one fragment differ in length): reads whose
sequence bytes are equal -- with -dedup_prefix N their first N bases -- form a cluster and the first of it stays
(mk_fastq_dedup_text: exact, case and N as they stand, no reverse complement; a hash only chooses where to look); with
-dedup_paired, or whenever -overlap is given, the unit is the pair and both mates must be equal (-overlap_mate FILE2 is then
interleaved once in front of -dedup).  dedup/<sample>_dedup.fastq holds what the later steps and the count see,
dedup/<sample>_dedup.tsv every read's length, first, copies and keep value, _levels.tsv the clusters of 1 .. -dedup_high
copies and of more (fastqc's duplication levels), _summary.tsv the duplication rate, _overrepresented.tsv the clusters that
hold at least -dedup_over of the reads (at most 1000).  With -qc the raw stage is the text in front of -dedup.  -orf stands where MerCat2
runs -prod / -fgs: the six-frame stop-to-stop ORFs (mk_orf_text: at least MIN_AA codons; -orf_start from the first ATG,
-orf_alt GTG and TTG too; -orf_strand) of the text the nucleotide count sees -- the cleaned text, the raw text with
-skipclean, fq2fa's text for FASTQ after -dedup / -overlap / -adapt / -qtrim -- are called on the GPU, written to
orf/<sample>_orf.faa and orf/<sample>_orf.tsv, and counted as the protein sample <sample>_orf with everything a protein
sample gets.  It is a stated rule, not a gene caller: gene models, RBS scoring, other translation tables, M for alternative
starts, partial-gene flags, the resolution of nested or overlapping ORFs and frameshift-aware calling stay out, and so does
a separate k for the ORFs.  QC plots, prodigal and FragGeneScanRs themselves (-prod / -fgs), the HTML report and plots belong
to the reference's other layers: their flags are accepted where they change nothing here (-lowmem, -debug,
-category_file) and refused with a clear message where the run would need that layer's output (-prod, -fgs).
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import timeit
from pathlib import Path

from . import __version__
from .fasta import _write_clean_gz, fq2fa_background, fq2fa_text, removeN_background, removeN_text
from .kmers import read_fasta_bytes
from .harness import load_table, run_raw_clean, run_raw_fastq, run_sample, run_text
from .report import (merge_counters, merge_counters_T, write_against_tsvs, write_histo_files, write_histo_tsv, write_query_tsv,
                     write_screen_tsv, write_track_median_tsv, write_track_txt)

FILTER_KEEP = ("matched", "unmatched")
NORM_KEEP = ("kept", "tossed")
FILTER_PAIR = ("either", "both")


def paired_outputs(args, name: str, folder, stem: str, base: str, ext: str) -> dict:
    """The arguments of kmers.filter_reads / trim_reads / normalize_reads that say where the reads of call ``name`` go:
    ``folder/<stem>.<ext>`` for single reads and interleaved pairs, ``<stem>_1`` and ``<stem>_2`` with a mate file,
    ``<base>_singles`` with -singles.  With -fastq_out the extension is ``fastq`` and the call is told to write FASTQ."""
    fastq = {"fastq_out": True} if getattr(args, "fastq_out", False) else {}
    if fastq:
        ext = "fastq"
    if not args.pairs_of[name]:
        return {"out_path": folder / f"{stem}.{ext}", **fastq}
    mate = getattr(args, f"{name}_mate")
    kw = {"out_path": folder / (f"{stem}_1.{ext}" if mate else f"{stem}.{ext}"), "paired": True, "mate_file": mate,
          "out_path2": folder / f"{stem}_2.{ext}" if mate else None, **fastq}
    if args.singles:
        kw["singles_path"] = folder / f"{base}_singles.{ext}"
    return kw
AGAINST_OPS = ("min", "max", "sum", "left", "only", "diff")  # native.OPS, for the parser (which loads no library)

FILE_EXT_FASTQ = [".fq", ".fastq", ".fq.gz", ".fastq.gz"]

FILE_EXT_NUCLEOTIDE = [".fasta", ".fa", ".fna", ".ffn", ".fasta.gz", ".fa.gz", ".fna.gz", ".ffn.gz"]
FILE_EXT_PROTEIN = [".faa", ".faa.gz"]


def parseargs(argv=None):
    p = argparse.ArgumentParser(description="MerCat2 k-mer counting on MI355X (count phase only)")
    p.add_argument("-i", required=False, default=list(), help="path to input file", nargs="+")
    p.add_argument("-f", type=str, required=False, help="path to folder containing input files")
    p.add_argument("-tsv", default=list(), nargs="+", metavar="DIR",
                   help="earlier output folder(s), or tsv_nucleotide / tsv_protein folders themselves: every <sample>_counts.tsv "
                        "in them is a sample whose table is loaded as it is, not counted again (-c does not apply to it); "
                        "-k must be the tables' k-mer length")
    p.add_argument("-query", type=str, required=False, metavar="FILE",
                   help="a panel of k-mers, one a line (a '\\t<count>' behind a key is ignored: a counts TSV or a Jellyfish / KMC "
                        "dump is a panel): for every sample type, query_<type>.tsv with the count of every panel k-mer in "
                        "every sample, looked up in the tables on the GPU; with -canonical a k-mer is looked up under "
                        "min(k-mer, reverse complement)")
    p.add_argument("-histo", type=int, nargs="?", const=10000, default=None, metavar="HIGH",
                   help="the abundance histogram of every sample (what Jellyfish calls histo), reduced in the tables on the "
                        "GPU: histo_<type>/<sample>_histo.txt, one '<abundance> <k-mers>' line per abundance that occurs, "
                        "k-mers counted more than HIGH times [10000, at most 1048576] together under HIGH + 1, and "
                        "histo_<type>.tsv with all samples side by side.  It describes the tables the run ends with: with "
                        "-c 10 the bins below 10 are empty by construction -- a spectrum for choosing -c is made with -c 1")
    p.add_argument("-screen", type=str, required=False, metavar="FILE",
                   help="a FASTA or FASTQ file (plain or .gz) of reads or contigs to screen against the tables on the GPU: for "
                        "every sample of FILE's type (by its extension, as -i inputs are sorted), "
                        "screen_<type>/<sample>_screen.tsv with one line per record of FILE: its k-mers (windows), how many "
                        "of them the sample holds at least -screen_min times (hits), and the sum, smallest and largest of "
                        "their counts; with -canonical the k-mers are folded")
    p.add_argument("-screen_min", type=int, default=1, metavar="N", help="-screen: a k-mer is a hit from this count on [1]")
    p.add_argument("-filter", type=str, required=False, metavar="FILE",
                   help="a FASTA or FASTQ file (plain or .gz) of reads or contigs to filter against the tables on the GPU: for "
                        "every sample of FILE's type, filter_<type>/<sample>_<matched|unmatched>.fna (.faa for protein) with "
                        "the records of FILE that match the sample's table, or those that do not (-filter_keep), byte for "
                        "byte and in order.  A FASTQ file is first converted as MerCat2's fq2fa converts it, so the output is "
                        "FASTA, the text MerCat2 itself counts; with -canonical the k-mers are folded")
    p.add_argument("-track", type=str, required=False, metavar="FILE",
                   help="a FASTA or FASTQ file (plain or .gz) of reads or contigs to track against the tables on the GPU: for "
                        "every sample of FILE's type (nucleotide / protein by its extension; FASTQ is nucleotide), "
                        "track_<type>/<sample>_track.txt with, per record of FILE, a '>name' line and one line of the counts "
                        "of its k-mers in the sample, in read order (0: absent), and track_<type>/<sample>_median.tsv with "
                        "each record's k-mers, the median of their counts, and their sum, smallest and largest")
    p.add_argument("-track_sat32", action="store_true", help="-track: 32-bit counts, clipped at 2^32 - 1 (half the bytes moved)")
    p.add_argument("-trim", type=str, required=False, metavar="FILE",
                   help="a FASTA or FASTQ file (plain or .gz) of reads to trim against the tables on the GPU: for every sample "
                        "of FILE's type, trim_<type>/<sample>_trimmed.fna (.faa for protein) with every record of FILE cut in "
                        "front of its first k-mer the sample holds fewer than -trim_min times -- its header line, then what it "
                        "keeps on one line; a record that keeps fewer than -trim_len characters is dropped -- and "
                        "trim_<type>/<sample>_trim.tsv with 'record, length, kept' per record.  A FASTQ file is first "
                        "converted as MerCat2's fq2fa converts it, so the output is FASTA; with -canonical the k-mers are folded")
    p.add_argument("-trim_min", type=int, default=None, metavar="N",
                   help="-trim: a k-mer is low below this count [2, the default cutoff of khmer's filter-abund]")
    p.add_argument("-trim_len", type=int, default=None, metavar="N", help="-trim: drop a record that keeps fewer characters [k]")
    p.add_argument("-correct", type=str, required=False, metavar="FILE",
                   help="a nucleotide FASTA or FASTQ file (plain or .gz) of reads to correct against the tables on the GPU: for "
                        "every sample of FILE's type, correct_<type>/<sample>_corrected.fna with every record of FILE -- its "
                        "header line, then its characters on one line -- in which each base that alone makes a run of k-mers "
                        "rarer than -correct_min, and that exactly one other base repairs, is replaced by that base, and "
                        "correct_<type>/<sample>_correct.tsv with 'record, length, runs, fixed, ambiguous, unfixable' per "
                        "record.  A FASTQ file is first converted as MerCat2's fq2fa converts it, so the output is FASTA; "
                        "with -canonical the k-mers are folded; -k at most 64")
    p.add_argument("-correct_min", type=int, default=None, metavar="N", help="-correct: a k-mer is weak below this count [2]")
    p.add_argument("-correct_rounds", type=int, default=None, metavar="N",
                   help="-correct: correct the output again, N passes in all [1]")
    p.add_argument("-correct_mate", type=str, default=None, metavar="FILE2",
                   help="-correct: the second file of paired reads (FILE the first); every record is written, to "
                        "..._corrected_1 and ..._corrected_2")
    p.add_argument("-correct_fastq", action="store_true",
                   help="-correct: FILE (and -correct_mate FILE2) is FASTQ and is written as FASTQ, byte for byte but for the "
                        "corrected bases, the qualities kept: correct_<type>/<sample>_corrected.fastq (..._corrected_1.fastq and "
                        "..._corrected_2.fastq with a mate) beside the same _correct.tsv (mk_correct_fastq_text)")
    p.add_argument("-correct_qual", type=str, default=None, metavar="C",
                   help="-correct_fastq: the quality character written under every corrected base, one of '!'..'~' "
                        "(Lighter's -newQual) [the qualities stay]")
    p.add_argument("-norm", type=str, required=False, metavar="FILE",
                   help="a FASTA or FASTQ file (plain or .gz) of reads to thin against the tables on the GPU (digital "
                        "normalisation; the table should have been counted from these reads): for every sample of FILE's type, "
                        "norm_<type>/<sample>_<kept|tossed>.fna (.faa for protein) with the records of FILE whose depth -- the "
                        "median of their k-mers' counts in the sample -- is at least -norm_min, all of them up to depth "
                        "-norm_target and a share target / depth of the deeper ones, byte for byte and in order, or the "
                        "records left out (-norm_keep), and norm_<type>/<sample>_norm.tsv with 'record, windows, median, "
                        "kept' per record.  A FASTQ file is first converted as MerCat2's fq2fa converts it, so the output is "
                        "FASTA; with -canonical the k-mers are folded")
    p.add_argument("-norm_target", type=int, default=None, metavar="N",
                   help="-norm: the depth to thin to [20, the default cutoff of khmer's normalize-by-median]")
    p.add_argument("-norm_min", type=int, default=None, metavar="N", help="-norm: drop a record whose depth is below N [0]")
    p.add_argument("-norm_seed", type=int, default=None, metavar="N", help="-norm: the seed of the draws [0]")
    p.add_argument("-norm_keep", type=str, default=None, choices=NORM_KEEP,
                   help="-norm: write the records that are kept, or those that are tossed [kept]")
    p.add_argument("-paired", action="store_true",
                   help="-filter, -trim, -norm: FILE holds paired reads, interleaved (records 2p and 2p + 1 are mates, by "
                        "position): a pair is written or left out as a whole, so the output is interleaved again [False]")
    p.add_argument("-filter_mate", type=str, default=None, metavar="FILE2",
                   help="-filter: the second file of paired reads (FILE the first); implies paired, writes ..._1 and ..._2")
    p.add_argument("-trim_mate", type=str, default=None, metavar="FILE2",
                   help="-trim: the second file of paired reads (FILE the first); implies paired, writes ..._1 and ..._2")
    p.add_argument("-norm_mate", type=str, default=None, metavar="FILE2",
                   help="-norm: the second file of paired reads (FILE the first); implies paired, writes ..._1 and ..._2")
    p.add_argument("-filter_pair", type=str, default=None, choices=FILTER_PAIR,
                   help="-filter on paired reads: a pair matches if either mate does, or only if both do [either]")
    p.add_argument("-singles", action="store_true",
                   help="paired reads: also write <sample>_singles.fna, the reads that pass on their own in a pair that does not")
    p.add_argument("-fastq_out", action="store_true",
                   help="-filter, -trim, -norm (with -paired, the mate options and -singles too): FILE is FASTQ and the reads are "
                        "written as FASTQ with their qualities -- the quality line cut wherever -trim cuts the sequence -- to "
                        "the same names with .fastq in place of .fna (mk_fastq_select_text).  Not with -correct")
    p.add_argument("-filter_min", type=int, default=None, metavar="N", help="-filter: a k-mer is a hit from this count on [1]")
    p.add_argument("-filter_hits", type=int, default=None, metavar="N", help="-filter: a record matches from this many hits on [1]")
    p.add_argument("-filter_frac", type=float, default=None, metavar="F",
                   help="-filter: ... and only if at least this fraction (0..1) of its k-mers are hits [0]")
    p.add_argument("-filter_keep", type=str, default=None, choices=FILTER_KEEP,
                   help="-filter: write the records that match, or those that do not [unmatched, as BBDuk's out]")
    p.add_argument("-against", type=str, required=False, metavar="FILE",
                   help="a count table -- a counts TSV, or a Jellyfish / KMC dump -- of k-mer length -k to combine every sample "
                        "with by key, in the tables on the GPU (needs -op): for every sample of FILE's type (nucleotide or "
                        "protein, by its keys), against/tsv_<type>/<sample>_counts.tsv holds 'sample OP FILE', so that "
                        "-tsv <out>/against feeds the result to a next run.  Keys are compared as they stand: with "
                        "-canonical FILE must hold canonical keys")
    p.add_argument("-op", type=str, required=False, choices=AGAINST_OPS,
                   help="-against: per k-mer, with a the sample's count and b FILE's (0 where absent), the result holds min: "
                        "min(a, b), the shared k-mers; max: max(a, b); sum: a + b; left: a where FILE holds the k-mer; only: a "
                        "where FILE lacks it; diff: a - b where that is positive -- and no row where that is 0")
    p.add_argument("-against_min", type=int, default=1, metavar="N",
                   help="-against: a count of FILE below N is taken as absent [1]")
    p.add_argument("-k", type=int, required=True,
                   help="kmer length (with -orf the same k serves the nucleotide samples and their ORFs, as with MerCat2's -prod: "
                        "a protein k such as 3 to 7 is meant then)")
    p.add_argument("-n", type=int, default=os.cpu_count() or 1,
                   help="no of cores [auto detect]: samples read (inflated) and counted concurrently, at most 8")
    p.add_argument("-c", type=int, default=10, help="minimum kmer count [10]")
    p.add_argument("-s", type=int, default=100, required=False, help="Split into x MB files. [100]")
    p.add_argument("-o", type=str, default="mercat_results", required=False, help="Output folder")
    p.add_argument("-replace", action="store_true", help="Replace existing output directory [False]")
    p.add_argument("-skipclean", action="store_true", help="skip trimming of the sequences [False]")
    p.add_argument("-qtrim", type=int, nargs="?", const=20, default=None, metavar="Q",
                   help="FASTQ input, with or without -skipclean: trim and filter the reads on the GPU before they are counted. "
                        "This stands where MerCat2 runs fastp, and its result is not fastp's: every read is cut at its 3' end "
                        "by the running sum of Q - quality (BWA -q, cutadapt -q; no adapter removal, no sliding window) "
                        "[Q = 20]; writes qtrim/<sample>_qtrim.fastq, _qtrim.tsv and _summary.tsv")
    p.add_argument("-qtrim_front", type=int, default=None, metavar="Q", help="-qtrim: cut the 5' end the same way with this cutoff [0: not cut]")
    p.add_argument("-qtrim_len", type=int, default=None, metavar="N", help="-qtrim: drop a read of which fewer than N bases remain [1]")
    p.add_argument("-qtrim_n", type=int, default=None, metavar="N", help="-qtrim: drop a read whose remaining bases hold more than N 'N' [no limit]")
    p.add_argument("-qtrim_low", type=int, default=None, metavar="Q", help="-qtrim: a remaining base below quality Q is low [0: off]")
    p.add_argument("-qtrim_low_frac", type=float, default=None, metavar="F",
                   help="-qtrim: drop a read of whose remaining bases more than this fraction (0..1) are low; needs -qtrim_low [1]")
    p.add_argument("-qtrim_mean", type=int, default=None, metavar="Q", help="-qtrim: drop a read whose remaining bases average below Q [0: off]")
    p.add_argument("-qtrim_phred", type=int, default=None, choices=(33, 64), help="-qtrim: the offset of the quality characters [33]")
    p.add_argument("-adapt", type=str, nargs="?", const="", default=None, metavar="FILE",
                   help="FASTQ input, with or without -skipclean: remove 3' adapters from the reads on the GPU before -qtrim and the "
                        "count see them. The first job of the fastp run MerCat2 starts, as a stated rule that is not fastp's: a read "
                        "is cut at the leftmost position where an adapter matches the rest of it, or runs off its end (no indels; "
                        "-overlap finds adapters by the mates' overlap). FILE: a FASTA file of up to 1024 adapters of up to 128 bases [the Illumina TruSeq, "
                        "Nextera and small-RNA adapters]; writes adapt/<sample>_adapt.fastq, _adapt.tsv and _summary.tsv")
    p.add_argument("-adapt_overlap", type=int, default=None, metavar="N",
                   help="-adapt: the fewest bases an adapter must cover [8: set for a panel of hundreds of adapters, which at "
                        "cutadapt's 3 for one adapter would cut the end of most adapter-free reads by chance]")
    p.add_argument("-adapt_err", type=float, default=None, metavar="F", help="-adapt: mismatches allowed, as a fraction (0..1) of the overlap [0.1]")
    p.add_argument("-adapt_len", type=int, default=None, metavar="N", help="-adapt: drop a read of which fewer than N bases remain [1]")
    p.add_argument("-overlap", type=str, default=None, choices=("trim", "merge"),
                   help="FASTQ input, with or without -skipclean: every FASTQ input is taken as interleaved pairs, whose mates are "
                        "laid over each other on the GPU before -adapt, -qtrim and the count see them. The paired-end half of the "
                        "fastp run MerCat2 starts, as a stated rule that is not fastp's (indels in the overlap, quality-aware correction "
                        "of unmerged mates -- fastp -c -- and poly-G trimming stay out). trim: a pair that overlaps is cut to its fragment (adapter removal without a panel); "
                        "writes overlap/<sample>_overlap.fastq. merge: it becomes one read with a consensus over the overlap; "
                        "writes overlap/<sample>_merged.fastq and _unmerged.fastq, and the count sees both. Either way "
                        "overlap/<sample>_overlap.tsv and _summary.tsv")
    p.add_argument("-overlap_min", type=int, default=None, metavar="N", help="-overlap: the fewest bases the mates must share [30]")
    p.add_argument("-overlap_diff", type=int, default=None, metavar="N", help="-overlap: mismatches an overlap may hold [5]")
    p.add_argument("-overlap_err", type=float, default=None, metavar="F",
                   help="-overlap: and mismatches allowed as a fraction (0..1) of the overlap [0.2]")
    p.add_argument("-overlap_len", type=int, default=None, metavar="N", help="-overlap: drop a pair whose fragment has fewer than N bases [1]")
    p.add_argument("-overlap_mate", type=str, default=None, metavar="FILE2",
                   help="-overlap with exactly one FASTQ input: that file holds the first mates and FILE2 the second")
    p.add_argument("-toupper", action="store_true", help="convert all input sequences to uppercase [False]")
    # flags of the reference's other layers (bin/mercat2.py:45-58)
    p.add_argument("-prod", action="store_true", help="(MerCat2: ORF calling with prodigal) not part of this engine")
    p.add_argument("-fgs", action="store_true", help="(MerCat2: ORF calling with FragGeneScanRs) not part of this engine")
    p.add_argument("-orf", type=int, nargs="?", const=32, default=None, metavar="MIN_AA",
                   help="nucleotide input: call the six-frame stop-to-stop ORFs of at least MIN_AA codons [32] of the text the "
                        "count sees on the GPU, where MerCat2 runs prodigal (-prod) or FragGeneScanRs (-fgs) -- a stated rule, what "
                        "OrfM and getorf do, not a gene caller; writes orf/<sample>_orf.faa and orf/<sample>_orf.tsv and counts "
                        "the protein sample <sample>_orf with the same -k (a protein k such as 3 to 7 is meant)")
    p.add_argument("-orf_start", action="store_true", help="-orf: an ORF begins at the first ATG of its stop-to-stop stretch")
    p.add_argument("-orf_alt", action="store_true", help="-orf_start: GTG and TTG start too (translated as they stand, not as M)")
    p.add_argument("-orf_strand", choices=["both", "plus", "minus"], default=None, help="-orf: the strand(s) to call [both]")
    p.add_argument("-lowmem", action="store_true",
                   help="(MerCat2: incremental PCA beyond 1000 samples) accepted, no effect: the PCA here is exact, and is not "
                        "computed for more than 1000 samples")
    p.add_argument("-pca", action="store_true",
                   help="write pca_<type>/pca.tsv (three principal components per sample, exact PCA) for every sample type "
                        "with more than 3 samples; no plots")
    p.add_argument("-debug", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("-category_file", type=str, required=False, help=argparse.SUPPRESS)
    p.add_argument("-gpus", type=int, default=None,
                   help="number of GPUs to use, devices 0..N-1 [all visible]: a sample that is chunked (-s) has its chunks spread "
                        "over them (chunk i on GPU i mod N, tables summed by peer copies); small samples go one per GPU")
    p.add_argument("-qc", type=int, nargs="?", const=512, default=None, metavar="MAXPOS",
                   help="FASTQ input: quality control of the reads on the GPU where MerCat2 runs fastqc -- per cycle the quality "
                        "distribution and the base composition, per read the length, mean quality and GC share, as a stated rule "
                        "that is not fastqc's (no plots, duplication levels, adapter or k-mer content, verdicts). Cycles from "
                        "MAXPOS on share one row [512]. Writes qc/<sample>_raw_cycles.tsv, _quality.tsv, _gc.tsv, _length.tsv and "
                        "_summary.tsv from the text as read and, where -overlap, -adapt or -qtrim ran, qc/<sample>_clean_*.tsv "
                        "from the reads the count sees")
    p.add_argument("-qc_phred", type=int, default=None, choices=(33, 64), help="-qc: the offset of the quality characters [33]")
    p.add_argument("-qc_paired", action="store_true", help="-qc: the FASTQ inputs are interleaved pairs: every figure per mate")
    p.add_argument("-dedup", action="store_true",
                   help="FASTQ input, with or without -skipclean: remove duplicate reads on the GPU before -overlap, -adapt, -qtrim "
                        "and the count see them -- reads whose sequence bytes are equal form a cluster and the first stays (a "
                        "stated rule: exact, case and N as they stand, no reverse complement). Writes dedup/<sample>_dedup.fastq, "
                        "_dedup.tsv, _levels.tsv, _summary.tsv and _overrepresented.tsv")
    p.add_argument("-dedup_prefix", type=int, default=None, metavar="N", help="-dedup: compare only the first N bases of a read [0: whole reads]")
    p.add_argument("-dedup_paired", action="store_true",
                   help="-dedup: the FASTQ inputs are interleaved pairs and a pair is a duplicate iff both mates are (implied by -overlap)")
    p.add_argument("-dedup_high", type=int, default=None, metavar="N", help="-dedup: the duplication levels written one by one [100]")
    p.add_argument("-dedup_over", type=float, default=None, metavar="F",
                   help="-dedup: a sequence is over-represented from this fraction (0..1) of the reads on [0.001]")
    p.add_argument("-gpu", type=int, default=None, help="use exactly this one HIP device (overrides -gpus)")
    p.add_argument("-streams", type=int, default=None,
                   help="engine contexts counting chunks concurrently [2 for one-word keys, else 1]")
    p.add_argument("-union", action="store_true",
                   help="combined_<type>.tsv as the true union of the samples' tables (one row per k-mer in any sample). Default: "
                        "the rows MerCat2's merge_tsv writes, whose streaming loop leaves out or misplaces k-mers that not "
                        "all samples share (combined_<type>_T.tsv is always the union)")
    p.add_argument("-canonical", action="store_true",
                   help="EXTENSION (not MerCat2 behaviour): count min(kmer, reverse complement) for nucleotide input")
    p.add_argument("--version", "-v", action="version", version=f"mercat2_amd {__version__}")
    args = p.parse_args(argv)
    if not args.i and not args.f and not args.tsv:
        p.error("Please provide either an input file (-i) or an input folder (-f)")
    for filename in args.i:
        if not os.path.isfile(filename):
            p.error(f"file '{filename}' is not valid.\n")
    if args.f and not os.path.isdir(args.f):
        p.error(f"folder {args.f} is not valid.\n")
    if args.query and not os.path.isfile(args.query):
        p.error(f"file '{args.query}' is not valid.\n")
    qtrim_flags = ("qtrim_front", "qtrim_len", "qtrim_n", "qtrim_low", "qtrim_low_frac", "qtrim_mean", "qtrim_phred")
    if args.qtrim is None:
        for flag in qtrim_flags:
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -qtrim")
    else:
        given = list(args.i)
        if args.f and os.path.isdir(args.f):
            given += sorted(os.listdir(args.f))
        if not any(fastq_ext(Path(name)) for name in given):
            p.error(f"-qtrim trims FASTQ reads ({' / '.join(FILE_EXT_FASTQ)}); no input is a FASTQ file")
        for flag, value in (("qtrim", args.qtrim), ("qtrim_front", args.qtrim_front), ("qtrim_low", args.qtrim_low),
                            ("qtrim_mean", args.qtrim_mean)):
            if value is not None and not 0 <= value <= 93:
                p.error(f"-{flag} {value}: must lie in 0..93")
        for flag in ("qtrim_len", "qtrim_n"):
            if getattr(args, flag) is not None and not 0 <= getattr(args, flag) < 1 << 32:
                p.error(f"-{flag} {getattr(args, flag)}: must lie in 0..2^32 - 1")
        if args.qtrim_low_frac is not None and not 0.0 <= args.qtrim_low_frac <= 1.0:
            p.error(f"-qtrim_low_frac {args.qtrim_low_frac}: must lie in 0..1")
        if args.qtrim_low_frac is not None and not args.qtrim_low:
            p.error("-qtrim_low_frac needs -qtrim_low Q: no base is low without it")
    if not args.dedup:
        for flag in ("dedup_prefix", "dedup_high", "dedup_over"):
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -dedup")
        if args.dedup_paired:
            p.error("-dedup_paired needs -dedup")
    else:
        given = list(args.i)
        if args.f and os.path.isdir(args.f):
            given += sorted(os.listdir(args.f))
        if not any(fastq_ext(Path(name)) for name in given):
            p.error(f"-dedup removes duplicate FASTQ reads ({' / '.join(FILE_EXT_FASTQ)}); no input is a FASTQ file")
        if args.dedup_prefix is not None and not 0 <= args.dedup_prefix < 1 << 32:
            p.error(f"-dedup_prefix {args.dedup_prefix}: must lie in 0..2^32 - 1")
        if args.dedup_high is not None and not 1 <= args.dedup_high <= 1 << 20:
            p.error(f"-dedup_high {args.dedup_high}: must lie in 1..{1 << 20}")
        if args.dedup_over is not None and not 0.0 <= args.dedup_over <= 1.0:
            p.error(f"-dedup_over {args.dedup_over}: must lie in 0..1")
    if args.qc is None:
        if args.qc_phred is not None:
            p.error("-qc_phred needs -qc")
        if args.qc_paired:
            p.error("-qc_paired needs -qc")
    else:
        given = list(args.i)
        if args.f and os.path.isdir(args.f):
            given += sorted(os.listdir(args.f))
        if not any(fastq_ext(Path(name)) for name in given):
            p.error(f"-qc looks at FASTQ reads ({' / '.join(FILE_EXT_FASTQ)}); no input is a FASTQ file")
        if not 1 <= args.qc <= 16384:
            p.error(f"-qc {args.qc}: must lie in 1..16384")
    args.adapters = None
    if args.adapt is None:
        for flag in ("adapt_overlap", "adapt_err", "adapt_len"):
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -adapt")
    else:
        given = list(args.i)
        if args.f and os.path.isdir(args.f):
            given += sorted(os.listdir(args.f))
        if not any(fastq_ext(Path(name)) for name in given):
            p.error(f"-adapt trims FASTQ reads ({' / '.join(FILE_EXT_FASTQ)}); no input is a FASTQ file")
        if args.adapt_overlap is not None and not 1 <= args.adapt_overlap <= 128:
            p.error(f"-adapt_overlap {args.adapt_overlap}: must lie in 1..128")
        if args.adapt_err is not None and not 0.0 <= args.adapt_err <= 1.0:
            p.error(f"-adapt_err {args.adapt_err}: must lie in 0..1")
        if args.adapt_len is not None and not 0 <= args.adapt_len < 1 << 32:
            p.error(f"-adapt_len {args.adapt_len}: must lie in 0..2^32 - 1")
        if args.adapt:
            if not os.path.isfile(args.adapt):
                p.error(f"file '{args.adapt}' is not valid.\n")
            from .native import read_adapters
            try:
                names, seqs = read_adapters(args.adapt)
            except ValueError as e:
                p.error(f"-adapt: {e}")
            if len(set(seqs)) > 1024 or max(len(s) for s in seqs) > 128:
                p.error(f"-adapt {args.adapt}: at most 1024 distinct adapters of at most 128 bases each")
            args.adapters = list(zip(names, seqs))
    if args.overlap is None:
        for flag in ("overlap_min", "overlap_diff", "overlap_err", "overlap_len", "overlap_mate"):
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -overlap")
    else:
        given = list(args.i)
        if args.f and os.path.isdir(args.f):
            given += sorted(os.listdir(args.f))
        reads = [name for name in given if fastq_ext(Path(name))]
        if not reads:
            p.error(f"-overlap lays the mates of FASTQ pairs over each other ({' / '.join(FILE_EXT_FASTQ)}); no input is a FASTQ file")
        if args.overlap_min is not None and not 1 <= args.overlap_min <= 512:
            p.error(f"-overlap_min {args.overlap_min}: must lie in 1..512")
        if args.overlap_err is not None and not 0.0 <= args.overlap_err <= 1.0:
            p.error(f"-overlap_err {args.overlap_err}: must lie in 0..1")
        for flag in ("overlap_diff", "overlap_len"):
            if getattr(args, flag) is not None and not 0 <= getattr(args, flag) < 1 << 32:
                p.error(f"-{flag} {getattr(args, flag)}: must lie in 0..2^32 - 1")
        if args.overlap_mate is not None:
            if len(reads) != 1:
                p.error(f"-overlap_mate names the second file of exactly one FASTQ input; {len(reads)} are given (interleave them)")
            if not os.path.isfile(args.overlap_mate):
                p.error(f"file '{args.overlap_mate}' is not valid.\n")
            if not fastq_ext(Path(args.overlap_mate)):
                p.error(f"-overlap_mate {args.overlap_mate}: needs a FASTQ file ({' / '.join(FILE_EXT_FASTQ)})")
    if args.histo is not None and not 1 <= args.histo <= 1 << 20:
        p.error(f"-histo {args.histo}: HIGH must lie in 1..{1 << 20}")
    args.screen_kind = None
    if args.screen:
        if not os.path.isfile(args.screen):
            p.error(f"file '{args.screen}' is not valid.\n")
        args.screen_kind = classify(Path(args.screen).expanduser().absolute(), True)[0]
        if not args.screen_kind:
            p.error(f"-screen {args.screen}: the extension names neither a nucleotide, a protein nor a FASTQ file")
    if not 1 <= args.screen_min < 1 << 64:
        p.error(f"-screen_min {args.screen_min}: must be 1 or more")
    args.track_kind = None
    if args.track:
        if not os.path.isfile(args.track):
            p.error(f"file '{args.track}' is not valid.\n")
        args.track_kind = classify(Path(args.track).expanduser().absolute(), True)[0]
        if not args.track_kind:
            p.error(f"-track {args.track}: the extension names neither a nucleotide, a protein nor a FASTQ file")
    elif args.track_sat32:
        p.error("-track_sat32 needs -track FILE")
    args.trim_kind = None
    if not args.trim:
        for flag in ("trim_min", "trim_len"):
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -trim FILE")
    else:
        if not os.path.isfile(args.trim):
            p.error(f"file '{args.trim}' is not valid.\n")
        args.trim_kind = classify(Path(args.trim).expanduser().absolute(), True)[0]
        if not args.trim_kind:
            p.error(f"-trim {args.trim}: the extension names neither a nucleotide, a protein nor a FASTQ file")
        args.trim_min = 2 if args.trim_min is None else args.trim_min
        if not 1 <= args.trim_min < 1 << 64:
            p.error(f"-trim_min {args.trim_min}: must be 1 or more")
        if args.trim_len is not None and not 1 <= args.trim_len < 1 << 64:
            p.error(f"-trim_len {args.trim_len}: must be 1 or more")
        args.trim_len = args.trim_len or 0  # (0: the k-mer length)
    args.correct_kind = None
    if not args.correct:
        for flag in ("correct_min", "correct_rounds", "correct_mate", "correct_qual"):
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -correct FILE")
        if args.correct_fastq:
            p.error("-correct_fastq needs -correct FILE")
    else:
        if not os.path.isfile(args.correct):
            p.error(f"file '{args.correct}' is not valid.\n")
        args.correct_kind = classify(Path(args.correct).expanduser().absolute(), True)[0]
        if not args.correct_kind:
            p.error(f"-correct {args.correct}: the extension names neither a nucleotide nor a FASTQ file")
        if args.correct_kind == "protein":
            p.error(f"-correct {args.correct}: a protein file; the correction rule is defined for nucleotide reads only")
        if args.k > 64:
            p.error(f"-correct needs -k of at most 64, not {args.k}")
        args.correct_min = 2 if args.correct_min is None else args.correct_min
        if not 1 <= args.correct_min < 1 << 64:
            p.error(f"-correct_min {args.correct_min}: must be 1 or more")
        args.correct_rounds = 1 if args.correct_rounds is None else args.correct_rounds
        if not 1 <= args.correct_rounds <= 64:
            p.error(f"-correct_rounds {args.correct_rounds}: must lie in 1..64")
        if args.correct_mate is not None:
            if not os.path.isfile(args.correct_mate):
                p.error(f"file '{args.correct_mate}' is not valid.\n")
            if classify(Path(args.correct_mate).expanduser().absolute(), True)[0] != args.correct_kind:
                p.error(f"-correct_mate {args.correct_mate}: not the type of -correct {args.correct}")
        if args.correct_fastq:
            for f in (args.correct, args.correct_mate):
                if f is not None and not str(f).lower().endswith(tuple(FILE_EXT_FASTQ)):
                    p.error(f"-correct_fastq with {f}: not a FASTQ file ({' / '.join(FILE_EXT_FASTQ)}); there are no qualities "
                            "to keep")
        if args.correct_qual is not None:
            if not args.correct_fastq:
                p.error("-correct_qual needs -correct_fastq")
            if len(args.correct_qual) != 1 or not "!" <= args.correct_qual <= "~":
                p.error(f"-correct_qual {args.correct_qual!r}: one printable character in '!'..'~'")
    args.norm_kind = None
    if not args.norm:
        for flag in ("norm_target", "norm_min", "norm_seed", "norm_keep"):
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -norm FILE")
    else:
        if not os.path.isfile(args.norm):
            p.error(f"file '{args.norm}' is not valid.\n")
        args.norm_kind = classify(Path(args.norm).expanduser().absolute(), True)[0]
        if not args.norm_kind:
            p.error(f"-norm {args.norm}: the extension names neither a nucleotide, a protein nor a FASTQ file")
        args.norm_target = 20 if args.norm_target is None else args.norm_target
        if not 1 <= args.norm_target < 1 << 32:
            p.error(f"-norm_target {args.norm_target}: must lie in 1..2^32 - 1")
        args.norm_min = 0 if args.norm_min is None else args.norm_min
        if not 0 <= args.norm_min < 1 << 32:
            p.error(f"-norm_min {args.norm_min}: must lie in 0..2^32 - 1")
        args.norm_seed = 0 if args.norm_seed is None else args.norm_seed
        if not 0 <= args.norm_seed < 1 << 64:
            p.error(f"-norm_seed {args.norm_seed}: must lie in 0..2^64 - 1")
        args.norm_keep = args.norm_keep or "kept"
    args.filter_kind = None
    if not args.filter:
        for flag in ("filter_min", "filter_hits", "filter_frac", "filter_keep"):
            if getattr(args, flag) is not None:
                p.error(f"-{flag} needs -filter FILE")
    else:
        if not os.path.isfile(args.filter):
            p.error(f"file '{args.filter}' is not valid.\n")
        args.filter_kind = classify(Path(args.filter).expanduser().absolute(), True)[0]
        if not args.filter_kind:
            p.error(f"-filter {args.filter}: the extension names neither a nucleotide, a protein nor a FASTQ file")
        args.filter_min = 1 if args.filter_min is None else args.filter_min
        args.filter_hits = 1 if args.filter_hits is None else args.filter_hits
        args.filter_frac = 0.0 if args.filter_frac is None else args.filter_frac
        args.filter_keep = args.filter_keep or "unmatched"
        if not 1 <= args.filter_min < 1 << 64:
            p.error(f"-filter_min {args.filter_min}: must be 1 or more")
        if not 1 <= args.filter_hits < 1 << 64:
            p.error(f"-filter_hits {args.filter_hits}: must be 1 or more")
        if not 0.0 <= args.filter_frac <= 1.0:  # (the rule kmers.filter_reads applies: native.ppm_of_fraction)
            p.error(f"-filter_frac {args.filter_frac}: must lie in 0..1")
    # paired reads: -paired (FILE is interleaved) or a mate file a call; both make the pair the unit
    mates = {name: getattr(args, f"{name}_mate") for name in ("filter", "trim", "norm")}
    for name, mate in mates.items():
        if mate is None:
            continue
        if not getattr(args, name):
            p.error(f"-{name}_mate needs -{name} FILE")
        if args.paired:
            p.error(f"-paired says FILE is interleaved: it does not go with -{name}_mate")
        if not os.path.isfile(mate):
            p.error(f"file '{mate}' is not valid.\n")
        if classify(Path(mate).expanduser().absolute(), True)[0] != getattr(args, f"{name}_kind"):
            p.error(f"-{name}_mate {mate}: not the type of -{name} {getattr(args, name)}")
    if args.paired and not (args.filter or args.trim or args.norm):
        p.error("-paired needs -filter, -trim or -norm FILE")
    args.pairs_of = {name: bool(getattr(args, name)) and (args.paired or mates[name] is not None) for name in mates}
    if args.filter_pair is not None and not args.pairs_of["filter"]:
        p.error("-filter_pair needs -filter FILE with -paired or -filter_mate")
    args.filter_pair = args.filter_pair or "either"
    if args.singles:
        if not any(args.pairs_of.values()):
            p.error("-singles needs -paired or a mate file")
        if args.pairs_of["filter"] and args.filter_keep != "matched":
            p.error("-singles with -filter needs -filter_keep matched: the pairs that do not pass have no orphans")
        if args.pairs_of["norm"] and args.norm_keep != "kept":
            p.error("-singles with -norm needs -norm_keep kept")
    if args.fastq_out:  # refused before anything runs: the qualities must exist, and must still fit the bases
        if not (args.filter or args.trim or args.norm):
            p.error("-fastq_out needs -filter, -trim or -norm FILE")
        if args.correct:
            p.error("-fastq_out does not go with -correct: corrected bases no longer go with the qualities they came with")
        for name in ("filter", "trim", "norm"):
            file = getattr(args, name)
            if not file:
                continue
            if getattr(args, f"{name}_kind") == "protein":
                p.error(f"-fastq_out with -{name} {file}: a protein file has no qualities to keep")
            for f in (file, mates[name]):
                if f is not None and not str(f).lower().endswith(tuple(FILE_EXT_FASTQ)):
                    p.error(f"-fastq_out with -{name} {f}: not a FASTQ file ({' / '.join(FILE_EXT_FASTQ)}); there are no "
                            "qualities to write")
    args.against_kind = None
    if args.op and not args.against:
        p.error("-op needs -against FILE")
    if args.against:
        if not args.op:
            p.error("-against needs -op {%s}" % ",".join(AGAINST_OPS))
        if not os.path.isfile(args.against):
            p.error(f"file '{args.against}' is not valid.\n")
        if not 1 <= args.against_min < 1 << 64:
            p.error(f"-against_min {args.against_min}: must be 1 or more")
        from . import native
        try:
            shape = native.tsv_shape(args.against)
        except native.MercatHipError as e:
            p.error(f"-against {args.against}: {e}")
        if shape["k"] != args.k:
            p.error(f"-k {args.k}: '{args.against}' holds {shape['k']}-mers")
        if shape["alphabet"] == native.ALPHABET_RAW:
            p.error(f"-against {args.against}: its keys are neither nucleotide (ACGT) nor protein (A-Z) k-mers")
        args.against_kind = "nucleotide" if shape["alphabet"] == native.ALPHABET_NT2 else "protein"
    args.loaded = {"nucleotide": {}, "protein": {}}  # sample -> its count table, per type (-tsv)
    for d in args.tsv:
        if not os.path.isdir(d):
            p.error(f"folder {d} is not valid.\n")
        found = loaded_tables(Path(d))
        for kind in found:
            args.loaded[kind].update(found[kind])
    for kind in args.loaded:
        for base, path in args.loaded[kind].items():
            from . import native
            k = native.tsv_shape(path)["k"]
            if k and k != args.k:
                p.error(f"-k {args.k}: '{path}' holds {k}-mers")
    if args.orf is None and (args.orf_start or args.orf_alt or args.orf_strand is not None):
        p.error("-orf_start / -orf_alt / -orf_strand need -orf")
    if args.orf is not None and args.orf < 1:
        p.error("-orf MIN_AA must be 1 or more")
    if args.orf_alt and not args.orf_start:
        p.error("-orf_alt needs -orf_start")
    if args.orf is not None:  # refused here, before anything runs
        samples, _ = input_samples(args)
        if not samples["nucleotide"]:
            p.error("-orf calls the ORFs of nucleotide samples: no nucleotide input file is given")
        for base in samples["nucleotide"]:
            if f"{base}_orf" in samples["protein"] or f"{base}_orf" in args.loaded["protein"]:
                p.error(f"-orf: the ORFs of '{base}' are counted as the protein sample '{base}_orf', which is given as an input already")
    if args.prod or args.fgs:
        p.error("-prod / -fgs call ORFs with prodigal / FragGeneScanRs before counting amino-acid k-mers; that layer is "
                "not part of this engine: run the ORF caller and pass its .faa output with -i / -f")
    return args, p


def loaded_tables(folder: Path) -> dict:
    """{"nucleotide": {sample: path}, "protein": {...}}: the <sample>_counts.tsv files of an output folder's
    tsv_nucleotide / tsv_protein, or of such a folder itself."""
    found = {"nucleotide": {}, "protein": {}}
    folder = Path(os.path.abspath(os.path.expanduser(folder)))
    for kind in found:
        sub = folder if folder.name == f"tsv_{kind}" else folder / f"tsv_{kind}"
        if sub.is_dir():
            for name in sorted(os.listdir(sub)):
                if name.endswith("_counts.tsv") and (sub / name).is_file():
                    found[kind][name[: -len("_counts.tsv")]] = sub / name
    return found


def write_diversity(tables, out: Path, kind: str) -> None:
    """The reference's diversity reports of one sample type (bin/mercat2.py:351-361, 451-461, 479-499), from the tables
    still on the GPU: beta diversity into report/diversity (nucleotide) or report/beta_diversity (protein), one alpha
    file per sample, and with two or more samples the merged report/diversity-<type>.tsv."""
    from .diversity import compute_alpha_diversity, compute_beta_diversity, merge_alpha
    label = "Nucleotide" if kind == "nucleotide" else "protein"
    report = out / "report"
    compute_beta_diversity(label, tables, report / ("diversity" if kind == "nucleotide" else "beta_diversity"))
    (report / "diversity").mkdir(parents=True, exist_ok=True)
    files = {}
    for base in sorted(tables):
        files[base] = report / "diversity" / f"{'nucleotide' if kind == 'nucleotide' else label}-{base}.tsv"
        compute_alpha_diversity(base, tables[base], files[base])
    if len(files) >= 2:
        merge_alpha(files, report / f"diversity-{label}.tsv")


def fastq_ext(path: Path) -> str:
    """The FASTQ extension of the name ('' for none), the longest that matches, as the reference picks it."""
    suffixes = path.suffixes
    ext = ""
    for i in reversed(range(len(suffixes))):
        cand = "".join(suffixes[i:])
        if cand in FILE_EXT_FASTQ:
            ext = cand
    return ext


def classify(path: Path, skipclean: bool = False):
    """(type, basename) by the reference's extension tables (bin/mercat2.py:26-28, 264-283).  A FASTQ name is a
    nucleotide sample with ``skipclean`` (MerCat2 converts it with fq2fa and counts that); without it MerCat2 trims the
    reads with fastp first, which this engine does not run: SystemExit."""
    suffixes = path.suffixes
    ext = ""
    for i in reversed(range(len(suffixes))):
        cand = "".join(suffixes[i:])
        if cand in FILE_EXT_NUCLEOTIDE + FILE_EXT_PROTEIN:
            ext = cand
    if not ext:
        fq = fastq_ext(path)
        if fq and skipclean:
            return "nucleotide", path.name[: -len(fq)]
        if fq:
            raise SystemExit(f"'{path.name}': without -skipclean MerCat2 trims FASTQ reads with fastp, which is not part of "
                             "this engine; -skipclean counts the reads untrimmed (fq2fa only), as MerCat2 does with "
                             "-skipclean or when fastp is not installed")
        return None, None
    base = path.name[: -len(ext)]
    return ("protein" if ext in FILE_EXT_PROTEIN else "nucleotide"), base


def orf_samples(args, samples: dict, cleaned: dict, clean_paths: dict, out: Path, devices) -> None:
    """-orf: for every nucleotide sample the ORFs of the text its count saw -- the file under clean/ (once its writer has
    finished), or with -skipclean the FASTA file itself -- called by kmers.orf_reads, which writes orf/<sample>_orf.faa and
    orf/<sample>_orf.tsv; the .faa joins ``samples["protein"]`` as <sample>_orf."""
    from . import kmers, native
    folder = out / "orf"
    folder.mkdir(parents=True, exist_ok=True)
    start = timeit.default_timer()
    total = 0
    for idx, (base, f) in enumerate(samples["nucleotide"].items()):
        job = cleaned.get(base)
        if job is not None:
            job[2].result()  # (the clean file is complete)
        faa = folder / f"{base}_orf.faa"
        try:
            done = kmers.orf_reads(read_fasta_bytes(clean_paths.get(base, f)), faa, min_aa=args.orf, start=args.orf_start,
                                   alt_starts=args.orf_alt, strand=args.orf_strand or "both", tsv_path=folder / f"{base}_orf.tsv",
                                   device=devices[idx % len(devices)])
        except native.MercatHipError as e:
            raise SystemExit(f"-orf '{f.name}': {e}")
        total += done["orfs"]
        samples["protein"][f"{base}_orf"] = faa
    print(f"orf/: {total} ORFs of at least {args.orf} codons in {len(samples['nucleotide'])} sample(s): "
          f"{round(timeit.default_timer() - start, 2)} seconds")


def input_samples(args):
    """(samples, fastq) of the input files: {"nucleotide": {sample: file}, "protein": {...}} by ``classify``, and the
    nucleotide samples given as FASTQ (-skipclean: fq2fa, then counted)."""
    files = [Path(f) for f in args.i]
    if args.f:
        folder = Path(os.path.abspath(os.path.expanduser(args.f)))
        files += [folder / name for name in sorted(os.listdir(folder)) if (folder / name).is_file()]
    samples = {"nucleotide": {}, "protein": {}}
    fastq = set()
    for f in files:
        kind, base = classify(f.expanduser().absolute(),
                              args.skipclean or args.dedup or args.qtrim is not None or args.adapt is not None or args.overlap is not None)
        if kind:
            samples[kind][base] = f
            if fastq_ext(f):
                fastq.add(base)
            else:
                fastq.discard(base)
    return samples, fastq


def qtrim_sample(args, f: Path, raw, out: Path, base: str, device: int) -> bytes:
    """-qtrim: the reads of FASTQ sample ``base`` (``raw``: its bytes if they are in memory already, else None and ``f``
    is read) trimmed and filtered on GPU ``device`` by kmers.qtrim_reads, which writes qtrim/<base>_qtrim.fastq,
    _qtrim.tsv and _summary.tsv; returns the trimmed text, which is counted in the raw reads' place."""
    from . import kmers, native
    folder = out / "qtrim"
    folder.mkdir(parents=True, exist_ok=True)
    try:
        done = kmers.qtrim_reads(
            f if raw is None else raw, folder / f"{base}_qtrim.fastq", cut_back=args.qtrim, cut_front=args.qtrim_front or 0,
            min_len=args.qtrim_len or 0, max_n=args.qtrim_n, low_q=args.qtrim_low or 0,
            max_low_frac=1.0 if args.qtrim_low_frac is None else args.qtrim_low_frac, min_mean_q=args.qtrim_mean or 0,
            phred_base=args.qtrim_phred or 33, tsv_path=folder / f"{base}_qtrim.tsv", summary_path=folder / f"{base}_summary.tsv",
            device=device, keep_text=True)
    except native.MercatHipError as e:
        raise SystemExit(f"-qtrim '{f.name}': {e}")
    return done["text"]


def adapt_sample(args, f: Path, raw, out: Path, base: str, device: int) -> bytes:
    """-adapt: the reads of FASTQ sample ``base`` (``raw``: its bytes if they are in memory already, else None and ``f``
    is read) with their 3' adapters removed on GPU ``device`` by kmers.adapt_reads, which writes
    adapt/<base>_adapt.fastq, _adapt.tsv and _summary.tsv; returns the text that is left, which -qtrim and the count see
    in the raw reads' place."""
    from . import kmers, native
    folder = out / "adapt"
    folder.mkdir(parents=True, exist_ok=True)
    try:
        done = kmers.adapt_reads(
            f if raw is None else raw, folder / f"{base}_adapt.fastq", adapters=args.adapters,
            min_overlap=8 if args.adapt_overlap is None else args.adapt_overlap, max_err=0.1 if args.adapt_err is None else args.adapt_err,
            min_len=args.adapt_len or 0, tsv_path=folder / f"{base}_adapt.tsv", summary_path=folder / f"{base}_summary.tsv",
            device=device, keep_text=True)
    except native.MercatHipError as e:
        raise SystemExit(f"-adapt '{f.name}': {e}")
    return done["text"]


def overlap_sample(args, f: Path, raw, out: Path, base: str, device: int, interleaved: bool = False) -> bytes:
    """-overlap: the pairs of FASTQ sample ``base`` (``raw``: its bytes if they are in memory already, else None and ``f``
    is read; interleaved, or the first mates with -overlap_mate) trimmed or merged by the overlap of their mates on GPU
    ``device`` by kmers.overlap_reads, which writes overlap/<base>_overlap.fastq (trim) or _merged.fastq and
    _unmerged.fastq (merge), _overlap.tsv and _summary.tsv; returns the text that -adapt, -qtrim and the count see in the
    raw reads' place: the trimmed pairs, or the merged reads followed by the unmerged pairs.  ``interleaved``: ``raw`` holds
    both files of -overlap_mate already."""
    from . import kmers, native
    folder = out / "overlap"
    folder.mkdir(parents=True, exist_ok=True)
    merging = args.overlap == "merge"
    try:
        done = kmers.overlap_reads(
            f if raw is None else raw, folder / (f"{base}_merged.fastq" if merging else f"{base}_overlap.fastq"), mode=args.overlap,
            min_overlap=30 if args.overlap_min is None else args.overlap_min, max_mismatch=5 if args.overlap_diff is None else args.overlap_diff,
            max_err=0.2 if args.overlap_err is None else args.overlap_err, min_len=args.overlap_len or 0,
            mate_file=None if interleaved else args.overlap_mate,
            unmerged_path=folder / f"{base}_unmerged.fastq" if merging else None, tsv_path=folder / f"{base}_overlap.tsv",
            summary_path=folder / f"{base}_summary.tsv", device=device, keep_text=True)
    except (native.MercatHipError, ValueError) as e:
        raise SystemExit(f"-overlap '{f.name}': {e}")
    return done["text"] + done["unmerged"] if merging else done["text"]


def dedup_sample(args, f: Path, raw, out: Path, base: str, paired: bool, device: int, timings=None) -> bytes:
    """-dedup: the reads of FASTQ sample ``base`` (``raw``: its bytes if they are in memory already, else None and ``f``
    is read; with ``paired`` interleaved pairs) without their duplicates, found on GPU ``device`` by kmers.dedup_reads,
    which writes dedup/<base>_dedup.fastq, _dedup.tsv, _levels.tsv, _summary.tsv and _overrepresented.tsv; returns the
    text that is left, which the later steps and the count see in the raw reads' place.  ``timings``, if given, has the
    seconds added to its "dedup_s"."""
    from . import kmers, native
    folder = out / "dedup"
    folder.mkdir(parents=True, exist_ok=True)
    t0 = timeit.default_timer()
    try:
        done = kmers.dedup_reads(
            f if raw is None else raw, folder / f"{base}_dedup.fastq", prefix=args.dedup_prefix or 0, paired=paired,
            high=100 if args.dedup_high is None else args.dedup_high, over_frac=0.001 if args.dedup_over is None else args.dedup_over,
            tsv_path=folder / f"{base}_dedup.tsv", summary_path=folder / f"{base}_summary.tsv",
            levels_path=folder / f"{base}_levels.tsv", over_path=folder / f"{base}_overrepresented.tsv", device=device, keep_text=True)
    except native.MercatHipError as e:
        raise SystemExit(f"-dedup '{f.name}': {e}")
    if timings is not None:
        timings["dedup_s"] = timings.get("dedup_s", 0.0) + timeit.default_timer() - t0
    return done["text"]


def qc_sample(args, f: Path, text: bytes, out: Path, base: str, stage: str, paired: bool, device: int, timings=None) -> None:
    """-qc: the quality-control tables of ``text``, the reads of FASTQ sample ``base`` at ``stage`` ("raw": as read;
    "clean": as the count sees them), reduced on GPU ``device`` by kmers.qc_reads, which writes
    qc/<base>_<stage>_cycles.tsv, _quality.tsv, _gc.tsv, _length.tsv and _summary.tsv.  ``timings``, if given, has the
    seconds added to its "qc_s"."""
    from . import kmers, native
    folder = out / "qc"
    folder.mkdir(parents=True, exist_ok=True)
    t0 = timeit.default_timer()
    try:
        kmers.qc_reads(text, folder / f"{base}_{stage}", max_pos=args.qc, phred_base=args.qc_phred or 33, paired=paired, device=device)
    except native.MercatHipError as e:
        raise SystemExit(f"-qc '{f.name}' ({stage}): {e}")
    if timings is not None:
        timings["qc_s"] = timings.get("qc_s", 0.0) + timeit.default_timer() - t0


def prepared_reads(args, f: Path, raw, out: Path, base: str, device: int, timings=None) -> bytes:
    """The reads of FASTQ sample ``base`` as the count sees them: through -dedup, then -overlap, then -adapt, then
    -qtrim, where given (duplicates are looked for in the reads as sequenced: trimming makes copies of one fragment
    differ in length).  -dedup takes pairs with -dedup_paired or -overlap; with -overlap_mate both files are interleaved
    once, on the host, in front of it, and -overlap then gets that text.  With -qc the two places where MerCat2 runs
    fastqc: the text as read (with -overlap_mate both files, interleaved), and, where one of those steps ran, what it
    left.  The raw stage is per mate with -qc_paired or -overlap; the clean stage too, unless mates no longer alternate in
    it: after -overlap merge, and after -adapt or -qtrim, which judge every read on its own, and after a -dedup of single reads (one of pairs drops whole pairs)."""
    qc = args.qc is not None
    steps = args.dedup or args.overlap is not None or args.adapt is not None or args.qtrim is not None
    paired = qc and (args.qc_paired or args.overlap is not None)
    interleaved = False
    if args.dedup and args.overlap is not None and args.overlap_mate is not None:
        from . import native
        raw = native.interleave_fastq(read_fasta_bytes(f) if raw is None else raw, read_fasta_bytes(args.overlap_mate))
        interleaved = True
    if qc:
        raw = read_fasta_bytes(f) if raw is None else raw
        text = raw
        if args.overlap is not None and args.overlap_mate is not None and not interleaved:
            from . import native
            text = native.interleave_fastq(raw, read_fasta_bytes(args.overlap_mate))
        qc_sample(args, f, text, out, base, "raw", paired, device, timings)
        del text
    if args.dedup:
        raw = dedup_sample(args, f, raw, out, base, args.dedup_paired or args.overlap is not None, device, timings)
    if args.overlap is not None:
        raw = overlap_sample(args, f, raw, out, base, device, interleaved)
    if args.adapt is not None:
        raw = adapt_sample(args, f, raw, out, base, device)
    if args.qtrim is not None:
        raw = qtrim_sample(args, f, raw, out, base, device)
    raw = read_fasta_bytes(f) if raw is None else raw
    if qc and steps:
        alternate = args.overlap != "merge" and args.adapt is None and args.qtrim is None and (
            not args.dedup or args.dedup_paired or args.overlap is not None)  # (-dedup of single reads drops single reads)
        qc_sample(args, f, raw, out, base, "clean", paired and alternate, device, timings)
    return raw


def count_converted(base: str, holder: dict, fut, tsv: Path, args, devices, home: int, lines: list, tables: dict, t: dict) -> None:
    """The table of a sample whose text a background job rewrites (removeN) or converts (fq2fa) and writes as a level-9
    .gz, counted from the text in memory: the reference cuts the REWRITTEN file, and its size on disk decides
    (bin/mercat2.py:101) -- without waiting for the whole gzip: a DEFLATE stream only grows, so "chunked" is known the
    moment its bytes pass -s MiB.  Until that is known, both tables are counted (milliseconds each) and the size picks one."""
    limit = args.s * 1024 * 1024
    holder["ready"].wait()
    if "text" not in holder:
        fut.result()  # (the rewrite failed: its exception surfaces here, as it would in MerCat2)
    text = holder.pop("text")
    decision = holder["decision"]
    kw = dict(device=home, streams=args.streams, canonical=args.canonical, timings=t)
    # the .gz cannot be larger than the text plus the stored-block overhead zlib falls back to
    certain_whole = args.s <= 0 or len(text) + len(text) // 1000 + 4096 < limit
    chunked = False if certain_whole else decision.wait(0)
    if chunked is not None:
        run_text(base, text, tsv, args.k, args.c, args.s, chunked, devices=devices if chunked else None,
                 report=lines.append, keep=tables, **kw)
        return
    # not known yet: count BOTH tables now, publish the one the size selects
    t_wait = timeit.default_timer()
    cand = {}
    for name, ch in (("whole", False), ("chunked", True)):
        lc, kc = [], {}
        run_text(base, text, str(tsv) + "." + name, args.k, args.c, args.s, ch, devices=devices if ch else None,
                 report=lc.append, keep=kc, **kw)
        cand[ch] = (str(tsv) + "." + name, lc, kc)
    del text
    chunked = decision.wait()
    if chunked is None:
        fut.result()  # (the gzip writer failed)
    t["decide_s"] = timeit.default_timer() - t_wait
    path_, lc, kc = cand[bool(chunked)]
    if os.path.exists(path_):
        os.replace(path_, tsv)
    lines.extend(lc)
    tables.update(kc)
    other_path, _, other_keep = cand[not chunked]
    if os.path.exists(other_path):
        os.unlink(other_path)
    for ctx_ in other_keep.values():
        ctx_.close()


def main(argv=None) -> int:
    args, parser = parseargs(argv)
    out = Path(args.o)
    if out.exists():
        if args.replace:
            shutil.rmtree(out)
        else:
            parser.error(f"Output folder exists, please specify another folder or use the flag '-replace' to override the files. '{out}'")
    out.mkdir(0o777, True, True)
    from . import native
    visible = native.device_count()
    if visible < 1:
        raise SystemExit("mercat2_amd: no HIP device is visible (this engine has no CPU fallback)")
    if args.gpu is not None:
        if not 0 <= args.gpu < visible:
            parser.error(f"-gpu {args.gpu}: {visible} device(s) visible")
        devices = [args.gpu]
    else:
        want = visible if args.gpus is None else args.gpus
        if not 1 <= want <= visible:
            parser.error(f"-gpus {want}: {visible} device(s) visible")
        devices = list(range(want))
    print(f"\nStarting mercat2_amd v{__version__} with k-mer {args.k} on GPU{'s' if len(devices) > 1 else ''} "
          f"{','.join(str(d) for d in devices)}\n")
    if args.query:  # a malformed panel ends the run here, not after the counting: looked up once in an empty table
        try:
            with native.Counter(args.k, native.ALPHABET_NT2, device=devices[0]) as empty:
                empty.lookup_text(args.query)
        except native.MercatHipError as e:
            raise SystemExit(f"-query {args.query}: {e}")
    samples, fastq = input_samples(args)
    for kind in samples:
        both = sorted(set(samples[kind]) & set(args.loaded[kind]))
        if both:
            parser.error(f"sample '{both[0]}' is given both as an input file and as a table to load (-tsv)")

    from concurrent.futures import ThreadPoolExecutor
    # ---- "Loading files" (bin/mercat2.py:229-298): nucleotide FASTA goes through removeN unless -skipclean, FASTQ
    # through fq2fa.  The text rewrite is native and fast; the level-9 gzip of clean/<base>_clean.fna.gz or
    # clean/<base>.fna.gz is not (~1.5 MB/s), so the files are written by background threads while the counting below
    # already runs on the text in memory.
    print("Loading files")
    load_start = timeit.default_timer()
    clean = not args.skipclean
    clean_paths = {}  # base -> the file under clean/ that holds the text the count saw (-orf reads it back)
    cleaned = {}  # base -> [clean file, raw bytes (until counted), future of (.gz size, stats), holder of the cleaned text, timings]
    gz_writers = ThreadPoolExecutor(max(1, min(int(args.n), 16)))
    to_load = {b: f for b, f in samples["nucleotide"].items() if clean or b in fastq}
    home_of = {b: devices[i % len(devices)] for i, b in enumerate(samples["nucleotide"])}  # (the GPU that counts the sample, below)
    if to_load:
        import threading
        budget = [8 << 30]  # bytes of input held in memory between loading and counting; samples beyond it are read when counted
        budget_lock = threading.Lock()

        def load(item):
            base, f = item
            t = {}
            with budget_lock:
                room = budget[0] > 0
                budget[0] -= os.stat(f).st_size * (4 if str(f).endswith(".gz") else 1)
            if not room:
                return base, None
            t0 = timeit.default_timer()
            raw = read_fasta_bytes(f)
            t["read_s"] = timeit.default_timer() - t0
            steps = args.qtrim is not None or args.adapt is not None or args.overlap is not None
            if base in fastq and (steps or args.dedup or args.qc is not None):
                t0 = timeit.default_timer()
                raw = prepared_reads(args, f, raw, out, base, home_of[base], timings=t)
                if steps:
                    t["qtrim_s"] = timeit.default_timer() - t0 - t.get("qc_s", 0.0) - t.get("dedup_s", 0.0)
            if base in fastq:
                path, fut, holder = fq2fa_background(f, raw, out / "clean", base, gz_writers, timings=t, limit=args.s * 1024 * 1024)
            else:
                path, fut, holder = removeN_background(f, raw, out / "clean", args.toupper, gz_writers, timings=t,
                                                       limit=args.s * 1024 * 1024)
            return base, [path, raw, fut, holder, t]
        with ThreadPoolExecutor(max(1, min(int(args.n), 8, len(to_load)))) as pool:
            for base, job in pool.map(load, to_load.items()):
                cleaned[base] = job
    print(f"Time to load {len(samples['nucleotide']) + len(samples['protein'])} files: {round(timeit.default_timer() - load_start, 2)} seconds")

    for kind in ("nucleotide", "protein"):
        if kind == "protein" and args.orf is not None:  # the ORFs of the nucleotide samples join the protein samples
            orf_samples(args, samples, cleaned, clean_paths, out, devices)
        if not samples[kind] and not args.loaded[kind]:
            continue
        print("Processing Nucleotides" if kind == "nucleotide" else "Processing protein")
        tsv_dir = out / f"tsv_{kind}"
        tsv_dir.mkdir(parents=True, exist_ok=True)
        start = timeit.default_timer()
        # Samples are independent (bin/mercat2.py:336-339).  A '.gz' sample is bound by its one inflating
        # thread, so up to -n samples (at most 8) are in flight at once, each with its own contexts; the
        # lines the reference prints per sample are kept and shown in sample order.
        tables = {}  # sample -> its table, kept on the GPU for the combined table

        workers = max(1, min(int(args.n), max(8, 2 * len(devices)), len(samples[kind])))
        threads = max(2, 16 // workers)  # reader/decoder threads per sample: about 16 in all

        def one(numbered):
            idx, (base, f) = numbered
            lines = []
            # Several GPUs: a sample that is chunked spreads its chunks over all of them (run_sample /
            # run_text deal chunk i to GPU i mod N); a sample that is one chunk stays on ONE GPU, the samples taking
            # the GPUs in turn (no exchange at all) -- the reference's one Ray task per sample (bin/mercat2.py:336-339)
            home = devices[idx % len(devices)]
            t = {}
            t0 = timeit.default_timer()
            tsv = tsv_dir / f"{base}_counts.tsv"
            if kind == "nucleotide" and base in fastq:
                limit = args.s * 1024 * 1024
                if cleaned[base] is None:  # (not loaded up front: the conversion, its file, then the count)
                    text, _ = fq2fa_text(prepared_reads(args, f, None, out, base, home, timings=t))
                    os.makedirs(out / "clean", exist_ok=True)
                    size = _write_clean_gz(out / "clean" / f"{base}.fna.gz", text, t)
                    clean_paths[base] = out / "clean" / f"{base}.fna.gz"
                    chunked = args.s > 0 and size >= limit
                    run_text(base, text, tsv, args.k, args.c, args.s, chunked, device=home, devices=devices if chunked else None,
                             streams=args.streams, canonical=args.canonical, report=lines.append, keep=tables, timings=t)
                    del text
                else:
                    clean_file, raw, fut, holder, t_load = cleaned[base]
                    clean_paths[base] = clean_file
                    # the table straight from the raw reads, counted as fq2fa leaves them (rewritten in place on the GPU),
                    # while the conversion and the level-9 gzip of clean/<base>.fna.gz run in the background
                    done = run_raw_fastq(base, raw, tsv, args.k, args.c, limit, device=home, canonical=args.canonical,
                                         report=lines.append, keep=tables, timings=t)
                    cleaned[base][1] = raw = None
                    if done is not None:
                        holder["drop"]()
                    else:  # the sample may be chunked: count the converted text
                        count_converted(base, holder, fut, tsv, args, devices, home, lines, tables, t)
                    t.update(t_load)
            elif kind == "nucleotide" and clean:
                limit = args.s * 1024 * 1024
                if cleaned[base] is None:  # (not loaded up front: the rewrite, its file, then the count, one after the other)
                    clean_file, _gc, text = removeN_text(f, out / "clean", args.toupper, timings=t)
                    clean_paths[base] = clean_file
                    chunked = args.s > 0 and os.stat(clean_file).st_size >= limit
                    run_text(base, text, tsv, args.k, args.c, args.s, chunked, device=home, devices=devices if chunked else None,
                             streams=args.streams, canonical=args.canonical, report=lines.append, keep=tables, timings=t)
                    del text
                    t_load = {}
                else:
                    clean_file, raw, fut, holder, t_load = cleaned[base]
                    clean_paths[base] = clean_file
                    # the table straight from the raw text, counted as removeN leaves it (N runs cut records: the GPU finds
                    # them in the parser's pass), while the rewrite and the level-9 gzip of the clean file run in the background
                    done = run_raw_clean(base, raw, tsv, args.k, args.c, args.toupper, limit, device=home, canonical=args.canonical,
                                         report=lines.append, keep=tables, timings=t)
                    cleaned[base][1] = raw = None
                    if done is not None:
                        holder["drop"]()
                    else:
                        # the sample may be chunked (the reference cuts the CLEANED file, bin/mercat2.py:101, 243), or holds
                        # text whose rewrite the GPU does not reproduce: count the text the host rewrite produced
                        count_converted(base, holder, fut, tsv, args, devices, home, lines, tables, t)
                t.update(t_load)
            else:
                run_sample(base, f, tsv, args.k, args.c, args.s, device=home,
                           devices=[home] + [d for d in devices if d != home], streams=args.streams, canonical=args.canonical,
                           report=lines.append, keep=tables, threads=threads if workers > 1 else 0, timings=t)
            if args.debug:
                t["total_s"] = timeit.default_timer() - t0
                lines.append(f"[debug] {base}: " + " ".join(f"{k_}={v:.3f}" if isinstance(v, float) else f"{k_}={v}" for k_, v in sorted(t.items())))
            return lines
        if workers == 1:
            results = map(one, enumerate(samples[kind].items()))
        else:
            pool = ThreadPoolExecutor(workers)
            results = pool.map(one, enumerate(samples[kind].items()))
        for lines in results:
            for line in lines:
                print(line)
        print(f"Time to count {args.k}-mers: {round(timeit.default_timer() - start, 2)} seconds")
        # -tsv: tables of an earlier run, loaded as they are; they take the GPUs in turn like small counted samples, and are
        # written to this run's tsv_<type>/ too, so that the output is a complete result folder
        if args.loaded[kind]:
            start = timeit.default_timer()
            print(f"Loading {len(args.loaded[kind])} count table(s): they are already filtered, -c {args.c} is not applied to them")
            alphabet = native.ALPHABET_NT2 if kind == "nucleotide" else native.ALPHABET_AA5
            for idx, (base, path) in enumerate(args.loaded[kind].items(), len(samples[kind])):
                load_table(base, path, args.k, alphabet, devices[idx % len(devices)], tables, canonical=args.canonical)
                if base in tables:
                    tables[base].write_tsv(tsv_dir / f"{base}_counts.tsv", base)
            print(f"Time to load {len(args.loaded[kind])} tables: {round(timeit.default_timer() - start, 2)} seconds")
        # combined_<type>.tsv: what createFigures writes first (bin/mercat2.py:146-150, merge_tsv), here
        # straight from the tables; samples without significant k-mers are left out, as there
        try:
            if tables:
                stem = "combined_Nucleotide" if kind == "nucleotide" else "combined_protein"
                rows = merge_counters(tables, out / (stem + ".tsv"), as_reference=not args.union)
                union_rows = merge_counters_T(tables, out / (stem + "_T.tsv"))  # bin/mercat2.py:154-157, read by beta diversity
                if rows != union_rows:
                    print(f"Note: {stem}.tsv has {rows} rows, the samples hold {union_rows} different k-mers: MerCat2's merge_tsv "
                          f"leaves out or misplaces k-mers that not all samples share; {stem}_T.tsv is the full table, and "
                          f"-union writes {stem}.tsv that way too")
                if args.pca:  # bin/mercat2.py:170-181, from the tables still on the GPU
                    from .pca import cli_pca
                    cli_pca(tables, out, "Nucleotide" if kind == "nucleotide" else "protein")
                write_diversity(tables, out, kind)
                if args.query:  # from the tables still on the GPU
                    try:
                        n = write_query_tsv(tables, args.query, out / ("query_" + stem[len("combined_"):] + ".tsv"),
                                            fold=args.canonical and kind == "nucleotide")
                    except native.MercatHipError as e:
                        raise SystemExit(f"-query {args.query}: {e}")
                    print(f"query_{stem[len('combined_'):]}.tsv: {n} panel k-mers in {len(tables)} sample(s)")
                if args.screen and args.screen_kind == kind:  # from the tables still on the GPU
                    from .kmers import screen_reads
                    (out / f"screen_{kind}").mkdir(parents=True, exist_ok=True)
                    for base in sorted(tables):
                        try:
                            names, rows = screen_reads(tables[base], args.screen, args.screen_min)
                        except native.MercatHipError as e:
                            raise SystemExit(f"-screen {args.screen}: {e}")
                        write_screen_tsv(out / f"screen_{kind}" / f"{base}_screen.tsv", names, rows)
                    print(f"screen_{kind}/: {len(names)} records of {os.path.basename(args.screen)} screened against "
                          f"{len(tables)} sample(s)")
                if args.filter and args.filter_kind == kind:  # from the tables still on the GPU
                    from .kmers import filter_reads
                    (out / f"filter_{kind}").mkdir(parents=True, exist_ok=True)
                    ext = "faa" if kind == "protein" else "fna"
                    kept = {}
                    for base in sorted(tables):
                        try:
                            where = paired_outputs(args, "filter", out / f"filter_{kind}", f"{base}_{args.filter_keep}", base, ext)
                            if args.pairs_of["filter"]:
                                where["both"] = args.filter_pair == "both"
                            res = filter_reads(tables[base], args.filter, at_least=args.filter_min, min_hits=args.filter_hits,
                                               min_frac=args.filter_frac, invert=args.filter_keep == "unmatched", **where)
                        except native.MercatHipError as e:
                            raise SystemExit(f"-filter {args.filter}: {e}")
                        except ValueError as e:  # (-fastq_out: a header line that fq2fa drops)
                            if not args.fastq_out:
                                raise
                            raise SystemExit(f"-filter {args.filter}: {e}")
                        kept[base] = res["kept"]
                    print(f"filter_{kind}/: {res['records']} records of {os.path.basename(args.filter)} filtered against "
                          f"{len(tables)} sample(s), {args.filter_keep} records written: " +
                          ", ".join(f"{base} {n}" for base, n in kept.items()))
                if args.track and args.track_kind == kind:  # from the tables still on the GPU
                    from .kmers import track_reads
                    (out / f"track_{kind}").mkdir(parents=True, exist_ok=True)
                    tracked = (0, 0)  # (records and k-mers are those of FILE at this k: the same for every sample)
                    for base in sorted(tables):
                        try:
                            names, counts, offsets, rows, med = track_reads(tables[base], args.track, sat32=args.track_sat32)
                        except native.MercatHipError as e:
                            raise SystemExit(f"-track {args.track}: {e}")
                        write_track_txt(out / f"track_{kind}" / f"{base}_track.txt", names, counts, offsets)
                        write_track_median_tsv(out / f"track_{kind}" / f"{base}_median.tsv", names, rows, med)
                        tracked = (len(names), len(counts))
                    print(f"track_{kind}/: the {tracked[1]} k-mers of the {tracked[0]} records of {os.path.basename(args.track)} "
                          f"tracked against each of {len(tables)} sample(s)")
                if args.trim and args.trim_kind == kind:  # from the tables still on the GPU
                    from .kmers import trim_reads
                    (out / f"trim_{kind}").mkdir(parents=True, exist_ok=True)
                    ext = "faa" if kind == "protein" else "fna"
                    kept = {}
                    for base in sorted(tables):
                        try:
                            res = trim_reads(tables[base], args.trim, at_least=args.trim_min, min_len=args.trim_len,
                                             tsv_path=out / f"trim_{kind}" / f"{base}_trim.tsv",
                                             **paired_outputs(args, "trim", out / f"trim_{kind}", f"{base}_trimmed", base, ext))
                        except native.MercatHipError as e:
                            raise SystemExit(f"-trim {args.trim}: {e}")
                        except ValueError as e:  # (-fastq_out: a header line that fq2fa drops)
                            if not args.fastq_out:
                                raise
                            raise SystemExit(f"-trim {args.trim}: {e}")
                        kept[base] = (res["kept"], res["trimmed"])
                    print(f"trim_{kind}/: {res['records']} records of {os.path.basename(args.trim)} trimmed against "
                          f"{len(tables)} sample(s), records written (of them cut): " +
                          ", ".join(f"{base} {n} ({t})" for base, (n, t) in kept.items()))
                if args.correct and args.correct_kind == kind:  # from the tables still on the GPU
                    from .kmers import correct_reads, correct_reads_fastq
                    folder = out / f"correct_{kind}"
                    folder.mkdir(parents=True, exist_ok=True)
                    fixed = {}
                    for base in sorted(tables):
                        mate = args.correct_mate
                        try:
                            if args.correct_fastq:
                                res = correct_reads_fastq(tables[base], args.correct,
                                                          folder / (f"{base}_corrected_1.fastq" if mate else f"{base}_corrected.fastq"),
                                                          at_least=args.correct_min, rounds=args.correct_rounds,
                                                          tsv_path=folder / f"{base}_correct.tsv", mate_file=mate,
                                                          out_path2=folder / f"{base}_corrected_2.fastq" if mate else None,
                                                          new_qual=args.correct_qual or 0)
                                fixed[base] = (res["fixed"], res["runs"])
                                continue
                            res = correct_reads(tables[base], args.correct, folder / (f"{base}_corrected_1.fna" if mate else f"{base}_corrected.fna"),
                                                at_least=args.correct_min, rounds=args.correct_rounds,
                                                tsv_path=folder / f"{base}_correct.tsv", mate_file=mate,
                                                out_path2=folder / f"{base}_corrected_2.fna" if mate else None)
                        except native.MercatHipError as e:
                            raise SystemExit(f"-correct {args.correct}: {e}")
                        fixed[base] = (res["fixed"], res["runs"])
                    print(f"correct_{kind}/: {res['records']} records of {os.path.basename(args.correct)} corrected against "
                          f"{len(tables)} sample(s), bases replaced (of weak runs): " +
                          ", ".join(f"{base} {n} ({t})" for base, (n, t) in fixed.items()))
                if args.norm and args.norm_kind == kind:  # from the tables still on the GPU
                    from .kmers import normalize_read_pairs, normalize_reads, normalize_reads_fastq
                    (out / f"norm_{kind}").mkdir(parents=True, exist_ok=True)
                    ext = "faa" if kind == "protein" else "fna"
                    kept = {}
                    for base in sorted(tables):
                        try:
                            where = paired_outputs(args, "norm", out / f"norm_{kind}", f"{base}_{args.norm_keep}", base, ext)
                            run = normalize_read_pairs if where.pop("paired", False) else normalize_reads
                            if run is normalize_reads and where.pop("fastq_out", False):
                                run = normalize_reads_fastq
                            res = run(tables[base], args.norm, target=args.norm_target, min_depth=args.norm_min,
                                      seed=args.norm_seed, invert=args.norm_keep == "tossed",
                                      tsv_path=out / f"norm_{kind}" / f"{base}_norm.tsv", **where)
                        except native.MercatHipError as e:
                            raise SystemExit(f"-norm {args.norm}: {e}")
                        except ValueError as e:  # (-fastq_out: a header line that fq2fa drops)
                            if not args.fastq_out:
                                raise
                            raise SystemExit(f"-norm {args.norm}: {e}")
                        kept[base] = (res["kept"], res["thinned"])
                    print(f"norm_{kind}/: {res['records']} records of {os.path.basename(args.norm)} thinned to depth "
                          f"{args.norm_target} against {len(tables)} sample(s), {args.norm_keep} records written (thinned out): " +
                          ", ".join(f"{base} {n} ({t})" for base, (n, t) in kept.items()))
                if args.against and args.against_kind == kind:  # from the tables still on the GPU
                    try:
                        rows = write_against_tsvs({base: tables[base] for base in sorted(tables)}, args.against, args.op,
                                                  out / "against" / f"tsv_{kind}", args.against_min)
                    except native.MercatHipError as e:
                        raise SystemExit(f"-against {args.against}: {e}")
                    print(f"against/tsv_{kind}/: {len(tables)} sample(s) {args.op} {os.path.basename(args.against)}, "
                          f"{sum(1 for n in rows.values() if n)} with rows left")
                if args.histo is not None:  # from the tables still on the GPU
                    ordered = {base: tables[base] for base in sorted(tables)}
                    bins = write_histo_files(ordered, out / f"histo_{kind}", args.histo)
                    n = write_histo_tsv(ordered, out / f"histo_{kind}.tsv", args.histo, bins=bins)
                    print(f"histo_{kind}.tsv: {n} abundances up to {args.histo} (and above) in {len(tables)} sample(s)")
        finally:
            for t in tables.values():
                t.close()
    # the clean files must be complete before the run ends
    wait_start = timeit.default_timer()
    for base, job in cleaned.items():
        if job is not None:
            job[2].result()  # (an error of the rewrite -- e.g. a record to be split without a name: IndexError, as in MerCat2 -- surfaces here)
    gz_writers.shutdown()
    if cleaned and args.debug:
        print(f"[debug] waited {round(timeit.default_timer() - wait_start, 2)} s more for the clean/*.fna.gz writers (gzip level 9)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
