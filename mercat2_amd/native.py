"""ctypes binding of libmercat_hip.so (C ABI: include/mercat_hip.h).

The library is looked up next to this file (it is built in-tree by
``__graft_entry__.build()`` / ``make -C mercat2_amd/csrc``).  A missing library or a missing
HIP device raises -- nothing here or above falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

ALPHABET_NT2, ALPHABET_AA5, ALPHABET_RAW = 0, 1, 2
MODE_NAMES = {0: "dense", 1: "hash64", 2: "hash128", 3: "byref"}

MK_OK = 0
ERR_NAMES = {-1: "MK_ERR_ARG", -2: "MK_ERR_HIP", -3: "MK_ERR_NOMEM", -4: "MK_ERR_STATE",
             -5: "MK_ERR_NON_ASCII", -6: "MK_ERR_IO", -7: "MK_ERR_RANGE", -8: "MK_ERR_UNSUPPORTED"}

# every symbol include/mercat_hip.h declares (tests check the library exports each of them)
ABI_SYMBOLS = [
    "mk_create", "mk_destroy", "mk_last_error", "mk_reset", "mk_set_canonical", "mk_chunk_begin", "mk_chunk_feed",
    "mk_chunk_feed_device", "mk_chunk_end", "mk_count_device", "mk_export_size", "mk_export",
    "mk_write_tsv", "mk_export_pairs_device", "mk_import_pairs_device", "mk_export_exotic",
    "mk_import_exotic", "mk_words_per_key", "mk_merge_from", "mk_set_profiling", "mk_get_stats", "mk_reset_stats",
    "mk_chunk_cuts", "mk_synth_reads", "mk_version", "mk_count_file", "mk_stream_cuts",
    "mk_merged_export", "mk_write_merged_tsv", "mk_trim", "mk_alpha_stats", "mk_gunzip", "mk_crc32_of", "mk_gunzip_parallel",
    "mk_filter_min", "mk_remove_n", "mk_free", "mk_write_merged_tsv_t", "mk_write_merged_tsv_as_reference",
    "mk_owner_bounds", "mk_plan_contexts", "mk_bucket_rows_device", "mk_import_rows_device", "mk_merge_devices",
    "mk_export_size_multi", "mk_export_multi", "mk_write_tsv_multi", "mk_record_cuts", "mk_sample_keys", "mk_dense_bins_device",
    "mk_device_count", "mk_reset_for", "mk_textwrap", "mk_set_clean", "mk_clean_stats", "mk_clean_runs",
    "mk_export_stats", "mk_share_table", "mk_set_fastq", "mk_fastq_stats", "mk_fq2fa", "mk_gram", "mk_gram_matrix",
    "mk_pair_stats", "mk_pair_stats_matrix", "mk_load_tsv", "mk_load_tsv_text", "mk_tsv_shape",
    "mk_lookup", "mk_lookup_device", "mk_lookup_text", "mk_lookup_file", "mk_histo", "mk_histo_device",
    "mk_screen_text", "mk_screen_device", "mk_table_op", "mk_filter_text", "mk_filter_device",
    "mk_track_text", "mk_track_device", "mk_trim_text", "mk_trim_device", "mk_correct_text", "mk_correct_device",
    "mk_orf_text", "mk_orf_device",
    "mk_correct_fastq_text", "mk_correct_fastq_device", "mk_norm_text", "mk_norm_device",
    "mk_pairs_text", "mk_pairs_device", "mk_interleave", "mk_split_pairs", "mk_host_error",
    "mk_fastq_select_text", "mk_fastq_select_device", "mk_fastq_cuts", "mk_fq_interleave", "mk_fq_split_pairs",
    "mk_fastq_qtrim_text", "mk_fastq_qtrim_device", "mk_fastq_pair_cuts",
    "mk_adapters_pack", "mk_fastq_adapt_text", "mk_fastq_adapt_device",
    "mk_fastq_overlap_text", "mk_fastq_overlap_device",
    "mk_fastq_qc_text", "mk_fastq_qc_device",
    "mk_fastq_dedup_text", "mk_fastq_dedup_device",
]
MK_ABI = 6  # the number mk_version() must announce: struct layouts and signatures of include/mercat_hip.h as bound below
MERGE_RANGES, MERGE_GATHER, MERGE_BALANCED, MERGE_RCCL = 0, 1, 2, 4
LOOKUP_FOLD = 1
SCREEN_FOLD = 1
FILTER_FOLD, FILTER_INVERT = 1, 2
TRACK_FOLD, TRACK_SAT32 = 1, 2
TRIM_FOLD = 1
CORRECT_FOLD = 1
NORM_FOLD, NORM_INVERT = 1, 2
PAIRS_FILTER, PAIRS_TRIM, PAIRS_NORM = 0, 1, 2  # mk_pairs_rule_t.op
PAIRS_OPS = {"filter": PAIRS_FILTER, "trim": PAIRS_TRIM, "norm": PAIRS_NORM}
PAIRS_FOLD, PAIRS_INVERT, PAIRS_BOTH = 1, 2, 4
MEDIAN_SELECT_MIN = 16384  # MK_MEDIAN_SELECT_MIN: a record of more windows has its median selected, not sorted
# mk_table_op: f(ca, cb) per key (include/mercat_hip.h)
OP_MIN, OP_MAX, OP_SUM, OP_LEFT, OP_ONLY, OP_DIFF = range(6)
OPS = {"min": OP_MIN, "max": OP_MAX, "sum": OP_SUM, "left": OP_LEFT, "only": OP_ONLY, "diff": OP_DIFF}
SCREEN_COLUMNS = ("windows", "hits", "sum", "min", "max")  # mk_screen_row_t: the columns of Counter.screen's array


class MercatHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "MK_ERR"), code, message))
        self.code = code


class NonAsciiInput(MercatHipError, UnicodeDecodeError.__base__):  # ValueError family, like a decode error
    pass


class CleanUnsupported(MercatHipError):
    """Clean mode (Counter.set_clean): the text holds something whose rewrite by removeN the GPU does not reproduce;
    nothing was counted -- count the text mk_remove_n produces instead."""


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("raw_bytes", "symbols", "windows", "exotic_windows", "chunks",
                                           "survivors", "rows", "table_slots")] + \
               [("mode", C.c_int32), ("profiled", C.c_int32)] + \
               [(n, C.c_double) for n in ("ms_parse", "ms_pack", "ms_count", "ms_exotic", "ms_filter", "ms_export")] + \
               [(n, C.c_uint64) for n in ("n_parse", "n_pack", "n_count", "n_exotic", "n_filter", "n_export")] + \
               [("ms_part", C.c_double), ("n_part", C.c_uint64), ("records", C.c_uint64), ("distinct", C.c_uint64),
                ("part_retries", C.c_uint64), ("part_reused", C.c_uint64), ("fused_chunks", C.c_uint64), ("fuse_spilled", C.c_uint64), ("parse_retries", C.c_uint64),
                ("split_exhausted", C.c_uint64), ("flat_chunks", C.c_uint64), ("flat_refused", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FileStats(C.Structure):
    """mk_file_stats_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("disk_bytes", "text_bytes", "chunks")] +
                [(n, C.c_int32) for n in ("gz", "chunked", "members", "threads", "contexts", "devices", "split_pieces", "pad_")] +
                [(n, C.c_double) for n in ("s_wait_io", "s_wait_gpu", "s_total", "s_merge",
                                           "s_setup", "s_scan", "s_feed", "s_retire", "s_drain")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad_"}


class ExportStats(C.Structure):
    """mk_export_stats_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("rows", "bytes")] +
                [(n, C.c_double) for n in ("s_sort", "s_d2h", "s_format", "s_write", "s_total")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TsvLoad(C.Structure):
    """mk_tsv_load_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("bytes", "lines", "rows", "packed_rows", "text_rows", "zero_rows", "new_rows")] +
                [("header", C.c_int32), ("pieces", C.c_int32)] +
                [(n, C.c_double) for n in ("s_read", "s_parse", "s_import", "s_total")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Lookup(C.Structure):
    """mk_lookup_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("bytes", "lines", "keys", "found", "packed_keys", "text_keys", "folded")] +
                [("header", C.c_int32), ("pieces", C.c_int32)] +
                [(n, C.c_double) for n in ("s_read", "s_probe", "s_total")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ScreenRow(C.Structure):
    """mk_screen_row_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint64) for n in SCREEN_COLUMNS]


class Screen(C.Structure):
    """mk_screen_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("bytes", "records", "windows", "hits", "packed_windows", "text_windows", "folded")] +
                [("headless", C.c_int32), ("pieces", C.c_int32)] +
                [(n, C.c_double) for n in ("s_read", "s_parse", "s_probe", "s_total")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FilterRule(C.Structure):
    """mk_filter_rule_t (include/mercat_hip.h)."""
    _fields_ = [("at_least", C.c_uint64), ("min_hits", C.c_uint64), ("min_ppm", C.c_uint32), ("reserved", C.c_uint32)]


class Filter(C.Structure):
    """mk_filter_t (include/mercat_hip.h)."""
    _fields_ = ([("screen", Screen)] + [(n, C.c_uint64) for n in ("records_out", "bytes_out", "preamble")] +
                [(n, C.c_double) for n in ("s_place", "s_gather", "s_write")])

    def as_dict(self):
        d = self.screen.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:]})
        return d


class Track(C.Structure):
    """mk_track_t (include/mercat_hip.h)."""
    _fields_ = ([("screen", Screen)] + [(n, C.c_uint64) for n in ("windows_out", "saturated")] +
                [(n, C.c_double) for n in ("s_place", "s_track", "s_median", "s_write")])

    def as_dict(self):
        d = self.screen.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:]})
        return d


class TrimRule(C.Structure):
    """mk_trim_rule_t (include/mercat_hip.h)."""
    _fields_ = [("at_least", C.c_uint64), ("min_len", C.c_uint64)]


class Trim(C.Structure):
    """mk_trim_t (include/mercat_hip.h)."""
    _fields_ = ([("screen", Screen)] +
                [(n, C.c_uint64) for n in ("records_out", "records_trimmed", "records_dropped", "bases_in", "bases_out",
                                           "bytes_out", "preamble")] +
                [(n, C.c_double) for n in ("s_place", "s_first", "s_gather", "s_write")])

    def as_dict(self):
        d = self.screen.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:]})
        return d


ORF_START, ORF_ALT, ORF_PLUS, ORF_MINUS = 1, 2, 4, 8  # MK_ORF_*
ORF_STRANDS = {"both": 0, "plus": ORF_PLUS, "minus": ORF_MINUS}
ORF_COLUMNS = ("record", "begin", "aa", "frame")  # the columns of Counter.orfs' rows
# the standard code, index 16 c1 + 4 c2 + c3 with A 0, C 1, G 2, T 3 (include/mercat_hip.h)
CODON_TABLE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
ORF_ROW_DTYPE = np.dtype([("record", "<u8"), ("begin", "<u8"), ("aa", "<u4"), ("frame", "<u4")])  # mk_orf_row_t


class OrfOpt(C.Structure):
    """mk_orf_opt_t (include/mercat_hip.h)."""
    _fields_ = [("min_aa", C.c_uint32), ("flags", C.c_uint32)]


class Orf(C.Structure):
    """mk_orf_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("bytes", "records", "bases", "orfs", "residues", "bytes_out", "longest")] +
                [("per_frame", C.c_uint64 * 6), ("preamble", C.c_uint64), ("headless", C.c_int32), ("pieces", C.c_int32)] +
                [(n, C.c_double) for n in ("s_read", "s_parse", "s_find", "s_place", "s_emit", "s_write", "s_total")])

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["per_frame"] = [int(v) for v in self.per_frame]
        return d


def orf_options(min_aa: int = 32, start: bool = False, alt_starts: bool = False, strand: str = "both") -> "OrfOpt":
    """mk_orf_opt_t of Counter.orfs' arguments; ValueError for a min_aa no uint32 holds, a strand that is none of
    "both", "plus", "minus", or alt_starts without start."""
    if strand not in ORF_STRANDS:
        raise ValueError("strand %r: must be 'both', 'plus' or 'minus'" % (strand,))
    if alt_starts and not start:
        raise ValueError("alt_starts needs start")
    if not 0 <= int(min_aa) <= 0xFFFFFFFF:
        raise ValueError("min_aa %r does not fit mk_orf_opt_t" % (min_aa,))
    return OrfOpt(int(min_aa), (ORF_START if start else 0) | (ORF_ALT if alt_starts else 0) | ORF_STRANDS[strand])


def orf_rows(raw: np.ndarray) -> np.ndarray:
    """mk_orf_row_t records as the (n, 4) uint64 array Counter.orfs returns: record, begin, aa, frame."""
    out = np.empty((raw.size, 4), dtype=np.uint64)
    for j, name in enumerate(ORF_COLUMNS):
        out[:, j] = raw[name]
    return out


class CorrectRule(C.Structure):
    """mk_correct_rule_t (include/mercat_hip.h)."""
    _fields_ = [("at_least", C.c_uint64), ("reserved", C.c_uint64)]


# mk_correct_row_t: the columns of Counter.correct's ``fix`` array, and the same row as a structured dtype
CORRECT_COLUMNS = ("runs", "fixed", "ambiguous", "unfixable")
CorrectRow = np.dtype([(n, np.uint32) for n in CORRECT_COLUMNS])


class Correct(C.Structure):
    """mk_correct_t (include/mercat_hip.h)."""
    _fields_ = ([("screen", Screen)] +
                [(n, C.c_uint64) for n in ("records", "runs", "candidates", "fixed", "ambiguous", "unfixable", "bases",
                                           "bytes_out", "preamble")] +
                [(n, C.c_double) for n in ("s_place", "s_track", "s_runs", "s_try", "s_gather", "s_write")])

    def as_dict(self):
        d = self.screen.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:]})
        return d


class CorrectFastqRule(C.Structure):
    """mk_correct_fastq_rule_t (include/mercat_hip.h)."""
    _fields_ = [("at_least", C.c_uint64), ("new_qual", C.c_uint32), ("reserved", C.c_uint32)]


class CorrectFastq(C.Structure):
    """mk_correct_fastq_t (include/mercat_hip.h)."""
    _fields_ = ([("correct", Correct)] + [(n, C.c_uint64) for n in ("lines", "patched")] +
                [(n, C.c_double) for n in ("s_copy", "s_index", "s_patch")])

    def as_dict(self):
        d = self.correct.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:]})
        return d


def quality_byte(new_qual) -> int:
    """new_qual of mk_correct_fastq_rule_t from an int or a one-character str / bytes (0: the qualities stay)."""
    if isinstance(new_qual, str):
        new_qual = new_qual.encode("latin-1")
    if isinstance(new_qual, (bytes, bytearray)):
        if len(new_qual) != 1:
            raise ValueError("new_qual %r: one character" % (new_qual,))
        return new_qual[0]
    return int(new_qual)


class NormRule(C.Structure):
    """mk_norm_rule_t (include/mercat_hip.h)."""
    _fields_ = [("target", C.c_uint64), ("min_depth", C.c_uint64), ("seed", C.c_uint64)]


class Norm(C.Structure):
    """mk_norm_t (include/mercat_hip.h)."""
    _fields_ = ([("screen", Screen)] +
                [(n, C.c_uint64) for n in ("records_out", "records_short", "records_low", "records_over", "records_thinned",
                                           "bytes_out", "preamble")] +
                [(n, C.c_double) for n in ("s_place", "s_track", "s_median", "s_gather", "s_write")])

    def as_dict(self):
        d = self.screen.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:]})
        return d


class PairsRule(C.Structure):
    """mk_pairs_rule_t (include/mercat_hip.h)."""
    _fields_ = [("op", C.c_int32), ("reserved", C.c_int32), ("filter", FilterRule), ("trim", TrimRule), ("norm", NormRule)]


class Pairs(C.Structure):
    """mk_pairs_t (include/mercat_hip.h)."""
    _fields_ = ([("screen", Screen)] +
                [(n, C.c_uint64) for n in ("pairs", "pairs_out", "records_out", "singles_out", "bytes_out", "bytes_singles",
                                           "preamble", "records_trimmed", "records_dropped", "bases_in", "bases_out",
                                           "records_short", "records_low", "records_over", "records_thinned")] +
                [(n, C.c_double) for n in ("s_place", "s_walk", "s_median", "s_gather", "s_write")])

    def as_dict(self):
        d = self.screen.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:]})
        return d


class FastqSelect(C.Structure):
    """mk_fastq_select_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("records", "records_out", "records_trimmed", "bases_out", "bytes_out", "lines")] +
                [(n, C.c_double) for n in ("s_copy", "s_index", "s_place", "s_gather", "s_write")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class QtrimOpt(C.Structure):
    """mk_qtrim_opt_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("phred_base", "cut_front", "cut_back", "min_len", "max_n", "low_q", "max_low_ppm",
                                          "min_mean_q", "paired", "which")]


class FastqQtrim(C.Structure):
    """mk_fastq_qtrim_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("records", "records_out", "records_trimmed", "dropped_short", "dropped_n", "dropped_lowq",
                                           "dropped_meanq", "orphans", "bases_in", "bases_out", "bytes_out", "lines")] +
                [(n, C.c_double) for n in ("s_copy", "s_index", "s_scan", "s_place", "s_gather", "s_write")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


QTRIM_COLUMNS = ("length", "start", "kept", "n", "low", "qsum")  # the columns of Counter.fastq_qtrim's rows
QTRIM_NO_LIMIT = 0xFFFFFFFF  # mk_qtrim_opt_t.max_n: no limit


def qtrim_options(cut_back: int = 20, cut_front: int = 0, min_len: int = 0, max_n=None, low_q: int = 0, max_low_frac: float = 1.0,
                  min_mean_q: int = 0, phred_base: int = 33, paired: bool = False, which: int = 1) -> "QtrimOpt":
    """mk_qtrim_opt_t of Counter.fastq_qtrim's arguments; ValueError for one that no uint32 holds or a fraction outside
    0..1 (the library checks the ranges the rule sets)."""
    vals = dict(phred_base=phred_base, cut_front=cut_front, cut_back=cut_back, min_len=min_len,
                max_n=QTRIM_NO_LIMIT if max_n is None else max_n, low_q=low_q, max_low_ppm=ppm_of_fraction(max_low_frac),
                min_mean_q=min_mean_q, paired=1 if paired else 0, which=which)
    for name, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s %r: must lie in 0..2^32-1" % (name, v))
    return QtrimOpt(**{name: int(v) for name, v in vals.items()})


QC_MAX_POS, QC_QBINS, QC_GC_BINS = 16384, 96, 101  # MK_QC_MAX_POS, MK_QC_QBINS; the bins of read_gc
QC_TABLES = ("pos_qual", "pos_base", "read_len", "read_qual", "read_gc")  # the tables of Counter.fastq_qc, in mk_qc_out_t's order
QC_COLUMNS = ("length", "qsum", "gc", "n")  # the columns of Counter.fastq_qc's rows
QC_BASES = ("A", "C", "G", "T", "N", "other")  # the base classes: columns 0 .. 5 of pos_base


class QcOpt(C.Structure):
    """mk_qc_opt_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("phred_base", "max_pos", "paired")]


class QcOut(C.Structure):
    """mk_qc_out_t (include/mercat_hip.h): host or device addresses, 0 for no rows."""
    _fields_ = [(n, C.c_void_p) for n in QC_TABLES + ("rows",)]


class FastqQc(C.Structure):
    """mk_fastq_qc_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("records", "lines", "bases")] + [("min_len", C.c_uint64 * 2), ("max_len", C.c_uint64 * 2)] +
                [(n, C.c_double) for n in ("s_copy", "s_index", "s_reads", "s_cycles", "s_write")])

    def as_dict(self):
        return {n: list(getattr(self, n)) if n in ("min_len", "max_len") else getattr(self, n) for n, _ in self._fields_}


def qc_options(max_pos: int = 512, phred_base: int = 33, paired: bool = False) -> "QcOpt":
    """mk_qc_opt_t of Counter.fastq_qc's arguments; ValueError for one that no uint32 holds (the library checks the
    ranges the rule sets)."""
    vals = dict(phred_base=phred_base, max_pos=max_pos, paired=1 if paired else 0)
    for name, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s %r: must lie in 0..2^32-1" % (name, v))
    return QcOpt(**{name: int(v) for name, v in vals.items()})


def qc_shapes(max_pos: int, paired: bool) -> Dict[str, tuple]:
    """The shapes of the five tables of Counter.fastq_qc (uint64 each) for ``max_pos`` = P and C = 2 classes with
    ``paired``, else 1."""
    c, p = (2 if paired else 1), int(max_pos)
    return {"pos_qual": (c, p + 1, QC_QBINS), "pos_base": (c, p + 1, 8), "read_len": (c, p + 2), "read_qual": (c, QC_QBINS),
            "read_gc": (c, QC_GC_BINS)}


DEDUP_MAX_HIGH = 1 << 20  # MK_DEDUP_MAX_HIGH
DEDUP_COLUMNS = ("length", "first")  # the columns of Counter.fastq_dedup's rows


class DedupOpt(C.Structure):
    """mk_dedup_opt_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("prefix", "paired", "which", "high")]


class FastqDedup(C.Structure):
    """mk_fastq_dedup_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("records", "records_out", "distinct", "duplicates", "max_copies", "slots", "probes",
                                           "compares", "bases_in", "bases_out", "bytes_out", "lines")] +
                [(n, C.c_double) for n in ("s_plan", "s_copy", "s_index", "s_scan", "s_key", "s_insert", "s_place", "s_gather",
                                           "s_levels", "s_write")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def dedup_options(prefix: int = 0, paired: bool = False, which: int = 1, high: int = 100) -> "DedupOpt":
    """mk_dedup_opt_t of Counter.fastq_dedup's arguments; ValueError for one that no uint32 holds (the library checks the
    ranges the rule sets)."""
    vals = dict(prefix=prefix, paired=1 if paired else 0, which=which, high=high)
    for name, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s %r: must lie in 0..2^32-1" % (name, v))
    return DedupOpt(**{name: int(v) for name, v in vals.items()})


class AdaptOpt(C.Structure):
    """mk_adapt_opt_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("min_overlap", "max_err_ppm", "min_len", "paired", "which")]


class FastqAdapt(C.Structure):
    """mk_fastq_adapt_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("records", "records_out", "records_trimmed", "dropped_short", "orphans", "bases_in",
                                           "bases_out", "bytes_out", "lines")] +
                [(n, C.c_double) for n in ("s_copy", "s_index", "s_scan", "s_place", "s_gather", "s_write")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ADAPT_COLUMNS = ("length", "kept", "adapter", "overlap", "mismatches")  # the columns of Counter.fastq_adapt's rows
ADAPT_NO_HIT = 0xFFFFFFFF  # the adapter column of a read without a hit
ADAPT_PANEL_STRIDE = 9  # 64-bit words an adapter in mk_adapters_pack's panel, behind the one word that holds A
# the 3' adapters of the common Illumina library kits, as cutadapt's and fastp's manuals give them
ILLUMINA_ADAPTERS = (("TruSeq", "AGATCGGAAGAGC"), ("Nextera", "CTGTCTCTTATACACATCT"), ("small_RNA", "TGGAATTCTCGGGTGCCAAGG"))


def adapt_options(min_overlap: int = 8, max_err: float = 0.1, min_len: int = 0, paired: bool = False, which: int = 1) -> "AdaptOpt":
    """mk_adapt_opt_t of Counter.fastq_adapt's arguments; ValueError for one that no uint32 holds or an error rate outside
    0..1 (the library checks the ranges the rule sets)."""
    vals = dict(min_overlap=min_overlap, max_err_ppm=ppm_of_fraction(max_err), min_len=min_len, paired=1 if paired else 0, which=which)
    for name, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s %r: must lie in 0..2^32-1" % (name, v))
    return AdaptOpt(**{name: int(v) for name, v in vals.items()})


class OverlapOpt(C.Structure):
    """mk_overlap_opt_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("mode", "min_overlap", "max_mismatch", "max_err_ppm", "min_len", "which")]


class FastqOverlap(C.Structure):
    """mk_fastq_overlap_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("records", "pairs", "pairs_hit", "pairs_merged", "pairs_trimmed", "dropped_short", "skipped_long",
                                           "records_out", "records_trimmed", "bases_in", "bases_out", "bytes_out", "lines")] +
                [(n, C.c_double) for n in ("s_copy", "s_index", "s_scan", "s_place", "s_gather", "s_write")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


OVERLAP_COLUMNS = ("length", "kept", "fragment", "overlap", "mismatches")  # the columns of Counter.fastq_overlap's rows
OVERLAP_NO_HIT = 0xFFFFFFFF  # the fragment column of a pair without a hit
OVERLAP_MAX_BASES = 512  # MK_OVERLAP_MAX_BASES: a pair with a longer mate is not tested
OVERLAP_MODES = {"trim": 0, "merge": 1}


def overlap_options(mode="merge", min_overlap: int = 30, max_mismatch: int = 5, max_err: float = 0.2, min_len: int = 0,
                    which: int = 1) -> "OverlapOpt":
    """mk_overlap_opt_t of Counter.fastq_overlap's arguments; ValueError for a mode that is neither "trim" nor "merge" (0
    and 1 are taken too), a value that no uint32 holds or an error rate outside 0..1 (the library checks the ranges the
    rule sets)."""
    if mode in OVERLAP_MODES:
        mode = OVERLAP_MODES[mode]
    elif isinstance(mode, str) or isinstance(mode, bool):
        raise ValueError("mode %r: must be 'trim' or 'merge'" % (mode,))
    vals = dict(mode=mode, min_overlap=min_overlap, max_mismatch=max_mismatch, max_err_ppm=ppm_of_fraction(max_err), min_len=min_len,
                which=which)
    for name, v in vals.items():
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s %r: must lie in 0..2^32-1" % (name, v))
    return OverlapOpt(**{name: int(v) for name, v in vals.items()})


def read_adapters(path, check: bool = True) -> Tuple[list, list]:
    """(names, seqs) of the FASTA file ``path`` (plain or '.gz', records of any number of lines): the first word behind
    every '>' and the record's bases as str, blanks and tabs at line ends stripped.  A '>' line with no bases behind it
    is no record.  ValueError for a file without records and, with ``check``, naming the first record that holds a byte
    outside ACGTNacgtn (``check`` False: the records as they stand)."""
    import gzip
    with (gzip.open(path, "rb") if str(path).lower().endswith(".gz") else open(path, "rb")) as fh:
        raw = fh.read()
    names, seqs = [], []
    for line in raw.split(b"\n"):
        line = line.rstrip(b" \t\r")
        if line.startswith(b">"):
            if names and not seqs[-1]:
                names.pop()
                seqs.pop()
            names.append((line[1:].split() or [b""])[0].decode("utf-8", "replace"))
            seqs.append(b"")
        elif line:
            if not names:
                raise ValueError("read_adapters: %s does not start with a '>' line" % (path,))
            seqs[-1] += line
    if names and not seqs[-1]:
        names.pop()
        seqs.pop()
    if not names:
        raise ValueError("read_adapters: %s holds no record" % (path,))
    for i, (name, seq) in enumerate(zip(names, seqs)):
        bad = seq.translate(None, b"ACGTNacgtn")
        if bad and check:
            raise ValueError("read_adapters: record %d ('%s') of %s holds the byte 0x%02X: adapters are of ACGTN" % (i, name, path, bad[0]))
    return names, [s.decode("latin-1") for s in seqs]


def adapter_arrays(adapters, adapters2=None):
    """(bases, lengths, mates, seqs) as mk_fastq_adapt_* take them, of sequences (str or bytes) for first mates and
    unpaired reads (``adapters``) and for second mates (``adapters2``): every distinct sequence once, in the order of
    its first appearance, with class 1, 2 or -- where both lists hold it -- 3.  ``seqs``: those sequences as str."""
    as_bytes = lambda a: a.encode() if isinstance(a, str) else bytes(a)
    order, cls = [], {}
    for group, bit in ((adapters or (), 1), (adapters2 or (), 2)):
        for a in group:
            a = as_bytes(a)
            if a not in cls:
                order.append(a)
            cls[a] = cls.get(a, 0) | bit
    bases = np.frombuffer(b"".join(order), dtype=np.uint8).copy() if order else np.zeros(0, np.uint8)
    lengths = np.array([len(a) for a in order], dtype=np.uint32)
    mates = np.array([cls[a] for a in order], dtype=np.uint8)
    return bases, lengths, mates, [a.decode("latin-1") for a in order]


def pack_adapters(bases, lengths, mates=None) -> np.ndarray:
    """mk_adapters_pack: the packed panel (uint64 words; include/mercat_hip.h has the layout) of the adapters whose
    characters stand back to back in ``bases`` (uint8) with ``lengths`` (uint32) and mate classes ``mates`` (uint8, None:
    all 1).  Host code: no GPU is needed.  MercatHipError with the library's message for a refused panel."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    if mates is not None:
        mates = np.ascontiguousarray(mates, dtype=np.uint8)
    A = int(lengths.shape[0])
    words = np.zeros(1 + ADAPT_PANEL_STRIDE * max(min(A, 1024), 1), dtype=np.uint64)
    nwords, err = C.c_size_t(0), C.create_string_buffer(256)
    rc = lib().mk_adapters_pack(bases.ctypes.data, lengths.ctypes.data, mates.ctypes.data if mates is not None else None, A,
                                words.ctypes.data, words.shape[0], C.byref(nwords), err, 256)
    if rc:
        raise MercatHipError(rc, err.value.decode())
    return words[: nwords.value]


def ppm_of_fraction(min_frac: float) -> int:
    """min_ppm of mk_filter_rule_t for "at least this fraction of the record's k-mers are hits": round(min_frac * 10^6);
    ValueError outside 0..1 (and for a NaN)."""
    f = float(min_frac)
    if not 0.0 <= f <= 1.0:
        raise ValueError("min_frac %r: must lie in 0..1" % (min_frac,))
    return int(round(f * 1_000_000))


class Histo(C.Structure):
    """mk_histo_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("distinct", "total", "max_count", "over_rows", "over_total", "slots")] +
                [(n, C.c_double) for n in ("s_scan", "s_total")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TableOp(C.Structure):
    """mk_table_op_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("rows_a", "rows_b", "both", "rows_out", "total_out", "packed_out", "text_out", "slots")] +
                [("passes", C.c_int32), ("op", C.c_int32)] +
                [(n, C.c_double) for n in ("s_scan", "s_total")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CleanGpu(C.Structure):
    """mk_clean_gpu_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint64) for n in ("raw_bytes", "symbols", "gc_count", "n_bytes", "n_runs", "header_lines", "last_runs")]


class FastqStats(C.Structure):
    """mk_fastq_stats_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint64) for n in ("lines", "reads", "headers_dropped", "fasta_bytes", "crlf")]


class MergeStats(C.Structure):
    """mk_merge_stats_t (include/mercat_hip.h)."""
    _fields_ = ([(n, C.c_uint64) for n in ("rows_in", "rows_out", "rows_moved", "bytes_moved", "max_owned")] +
                [(n, C.c_int32) for n in ("contexts", "devices", "peer_direct", "rccl")] +
                [(n, C.c_double) for n in ("s_bucket", "s_copy", "s_import", "s_total")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad_"}


class CleanStats(C.Structure):
    """mk_clean_stats_t (include/mercat_hip.h)."""
    _fields_ = [(n, C.c_uint64) for n in ("gc_count", "total_length", "records", "split_records", "pieces", "n_runs")] + \
               [("unsupported_record", C.c_int64)]


class AlphaStats(C.Structure):
    """mk_alpha_t (include/mercat_hip.h)."""
    _fields_ = [("observed", C.c_uint64), ("total", C.c_uint64), ("freq", C.c_uint64 * 11),
                ("sum_sq", C.c_double), ("sum_clnc", C.c_double)]


_LIB: Optional[C.CDLL] = None


def library_path() -> Path:
    return Path(os.environ.get("MERCAT_HIP_LIB", Path(__file__).resolve().parent / "libmercat_hip.so"))


def lib() -> C.CDLL:
    """Load libmercat_hip.so once; raise if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not path.exists():
        raise MercatHipError(-2, "HIP extension %s is missing: build it with `python -c 'import __graft_entry__ as g; "
                                 "g.build()'` or `make -C mercat2_amd/csrc` (there is no CPU fallback)" % path)
    L = C.CDLL(str(path))
    vp, u8p, u64p, szp = C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)
    sig = {
        "mk_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "mk_destroy": (None, [vp]),
        "mk_last_error": (C.c_char_p, [vp]),
        "mk_reset": (C.c_int, [vp]),
        "mk_reset_for": (C.c_int, [vp, C.c_uint64]),
        "mk_set_canonical": (C.c_int, [vp, C.c_int]),
        "mk_set_clean": (C.c_int, [vp, C.c_int, C.c_int]),
        "mk_clean_stats": (C.c_int, [vp, C.POINTER(CleanGpu)]),
        "mk_clean_runs": (C.c_int, [vp, u64p, u64p, C.c_size_t, szp]),
        "mk_set_fastq": (C.c_int, [vp, C.c_int]),
        "mk_fastq_stats": (C.c_int, [vp, C.POINTER(FastqStats)]),
        "mk_fq2fa": (C.c_int, [u8p, C.c_size_t, C.POINTER(C.c_void_p), szp, C.POINTER(FastqStats)]),
        "mk_chunk_begin": (C.c_int, [vp]),
        "mk_chunk_feed": (C.c_int, [vp, u8p, C.c_size_t]),
        "mk_chunk_feed_device": (C.c_int, [vp, u8p, C.c_size_t]),
        "mk_chunk_end": (C.c_int, [vp, C.c_uint64]),
        "mk_count_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint64]),
        "mk_export_size": (C.c_int, [vp, szp]),
        "mk_export": (C.c_int, [vp, u8p, u64p, C.c_size_t]),
        "mk_write_tsv": (C.c_int, [vp, C.c_char_p, C.c_char_p, szp]),
        "mk_export_stats": (C.c_int, [vp, C.POINTER(ExportStats)]),
        "mk_export_pairs_device": (C.c_int, [vp, u64p, u64p, C.c_size_t, szp]),
        "mk_import_pairs_device": (C.c_int, [vp, u64p, u64p, C.c_size_t]),
        "mk_export_exotic": (C.c_int, [vp, u8p, u64p, C.c_size_t, szp]),
        "mk_import_exotic": (C.c_int, [vp, u8p, u64p, C.c_size_t]),
        "mk_words_per_key": (C.c_int, [vp]),
        "mk_merge_from": (C.c_int, [vp, vp]),
        "mk_share_table": (C.c_int, [vp, vp]),
        "mk_set_profiling": (C.c_int, [vp, C.c_int]),
        "mk_get_stats": (C.c_int, [vp, C.POINTER(Stats)]),
        "mk_reset_stats": (C.c_int, [vp]),
        "mk_chunk_cuts": (C.c_int, [u8p, C.c_size_t, C.c_uint64, u64p, C.c_size_t, szp]),
        "mk_synth_reads": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32,
                                     C.c_uint64, u8p, C.c_size_t, szp]),
        "mk_version": (C.c_char_p, []),
        "mk_count_file": (C.c_int, [C.POINTER(vp), C.c_int, C.c_char_p, C.c_uint64, C.c_uint64, C.c_int,
                                    C.POINTER(FileStats)]),
        "mk_merged_export": (C.c_int, [C.POINTER(vp), C.c_int, u8p, u64p, C.c_size_t, szp]),
        "mk_write_merged_tsv": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p, szp]),
        "mk_write_merged_tsv_as_reference": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p, szp]),
        "mk_write_merged_tsv_t": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(C.c_char_p), C.c_char_p, szp]),
        "mk_trim": (C.c_int, [vp]),
        "mk_filter_min": (C.c_int, [vp, C.c_uint64]),
        "mk_remove_n": (C.c_int, [u8p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), szp, C.POINTER(CleanStats)]),
        "mk_free": (None, [C.c_void_p]),
        "mk_textwrap": (C.c_int, [u8p, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), szp]),
        "mk_alpha_stats": (C.c_int, [vp, C.POINTER(AlphaStats)]),
        "mk_gunzip_parallel": (C.c_int, [u8p, C.c_size_t, u8p, C.c_size_t, C.c_int, C.c_size_t, szp, C.POINTER(C.c_int)]),
        "mk_crc32_of": (C.c_uint32, [u8p, C.c_size_t, C.c_uint32]),
        "mk_gunzip": (C.c_int, [u8p, C.c_size_t, u8p, C.c_size_t, C.c_size_t, szp, C.POINTER(C.c_int)]),
        "mk_stream_cuts": (C.c_int, [u8p, C.c_size_t, C.c_uint64, C.c_size_t, u64p, C.c_size_t, szp]),
        "mk_record_cuts": (C.c_int, [u8p, C.c_size_t, C.c_uint64, C.c_size_t, u64p, C.c_size_t, szp]),
        "mk_owner_bounds": (C.c_int, [C.c_int, C.c_int, u64p]),
        "mk_plan_contexts": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]),
        "mk_bucket_rows_device": (C.c_int, [vp, u64p, C.c_int, u64p, C.c_size_t, u64p]),
        "mk_import_rows_device": (C.c_int, [vp, u64p, C.c_size_t]),
        "mk_merge_devices": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(MergeStats)]),
        "mk_device_count": (C.c_int, []),
        "mk_sample_keys": (C.c_int, [vp, C.c_size_t, u64p, C.c_size_t, szp]),
        "mk_dense_bins_device": (C.c_int, [vp, u64p, C.c_size_t, C.c_int]),
        "mk_export_size_multi": (C.c_int, [C.POINTER(vp), C.c_int, szp]),
        "mk_export_multi": (C.c_int, [C.POINTER(vp), C.c_int, u8p, u64p, C.c_size_t]),
        "mk_write_tsv_multi": (C.c_int, [C.POINTER(vp), C.c_int, C.c_char_p, C.c_char_p, szp]),
        "mk_gram": (C.c_int, [C.POINTER(vp), C.c_int, C.c_size_t, u64p, szp]),
        "mk_gram_matrix": (C.c_int, [C.c_int, u64p, C.c_size_t, C.c_int, u64p]),
        "mk_pair_stats": (C.c_int, [C.POINTER(vp), C.c_int, C.c_size_t, C.c_void_p, u64p, szp, u64p]),
        "mk_pair_stats_matrix": (C.c_int, [C.c_int, u64p, C.c_size_t, C.c_int, C.c_void_p, u64p, u64p]),
        "mk_load_tsv": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(TsvLoad)]),
        "mk_load_tsv_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(TsvLoad)]),
        "mk_tsv_shape": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
        "mk_lookup": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, u64p, C.POINTER(Lookup)]),
        "mk_lookup_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, u64p, C.POINTER(Lookup)]),
        "mk_lookup_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, u64p, C.c_size_t, szp, C.POINTER(Lookup)]),
        "mk_lookup_file": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_uint, u64p, C.c_size_t, szp, C.POINTER(Lookup)]),
        "mk_histo": (C.c_int, [vp, C.c_uint64, u64p, C.POINTER(Histo)]),
        "mk_histo_device": (C.c_int, [vp, C.c_uint64, u64p, C.POINTER(Histo)]),
        "mk_screen_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint64, C.c_void_p, C.c_size_t, szp,
                                     C.POINTER(Screen)]),
        "mk_screen_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.c_uint64, C.c_void_p, C.c_size_t, szp, C.POINTER(Screen)]),
        "mk_filter_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(FilterRule), C.c_void_p, C.c_size_t, szp,
                                     C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Filter)]),
        "mk_filter_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.POINTER(FilterRule), C.c_void_p, C.c_size_t, szp,
                                       C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Filter)]),
        "mk_track_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint64, C.c_void_p, C.c_size_t, szp,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Track)]),
        "mk_track_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.c_uint64, C.c_void_p, C.c_size_t, szp,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Track)]),
        "mk_trim_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(TrimRule), C.c_void_p, C.c_size_t, szp,
                                   C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Trim)]),
        "mk_trim_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.POINTER(TrimRule), C.c_void_p, C.c_size_t, szp,
                                     C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Trim)]),
        "mk_orf_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.POINTER(OrfOpt), C.c_void_p, C.c_size_t, szp,
                                  C.c_void_p, C.c_size_t, szp, C.POINTER(Orf)]),
        "mk_orf_device": (C.c_int, [vp, u8p, C.c_size_t, C.POINTER(OrfOpt), C.c_void_p, C.c_size_t, szp,
                                    C.c_void_p, C.c_size_t, szp, C.POINTER(Orf)]),
        "mk_correct_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(CorrectRule), C.c_void_p, C.c_size_t, szp,
                                      C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Correct)]),
        "mk_correct_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.POINTER(CorrectRule), C.c_void_p, C.c_size_t, szp,
                                        C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Correct)]),
        "mk_correct_fastq_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(CorrectFastqRule), C.c_void_p,
                                            C.c_size_t, szp, C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(CorrectFastq)]),
        "mk_correct_fastq_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.POINTER(CorrectFastqRule), C.c_void_p, C.c_size_t,
                                              szp, C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(CorrectFastq)]),
        "mk_norm_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(NormRule), C.c_void_p, C.c_size_t, szp,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Norm)]),
        "mk_norm_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.POINTER(NormRule), C.c_void_p, C.c_size_t, szp,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp, C.POINTER(Norm)]),
        "mk_table_op": (C.c_int, [vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(TableOp)]),
        "mk_pairs_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(PairsRule), C.c_void_p, C.c_size_t, szp,
                                    C.c_void_p, C.c_size_t, szp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp,
                                    C.POINTER(Pairs)]),
        "mk_pairs_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_uint, C.POINTER(PairsRule), C.c_void_p, C.c_size_t, szp,
                                      C.c_void_p, C.c_size_t, szp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp,
                                      C.POINTER(Pairs)]),
        "mk_interleave": (C.c_int, [u8p, C.c_size_t, u8p, C.c_size_t, C.c_void_p, C.c_size_t, szp, szp]),
        "mk_split_pairs": (C.c_int, [u8p, C.c_size_t, C.c_void_p, C.c_size_t, szp, C.c_void_p, C.c_size_t, szp, szp]),
        "mk_host_error": (C.c_char_p, []),
        "mk_fastq_select_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint,
                                           C.c_void_p, C.c_size_t, szp, C.POINTER(FastqSelect)]),
        "mk_fastq_select_device": (C.c_int, [vp, u8p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint,
                                             C.c_void_p, C.c_size_t, szp, C.POINTER(FastqSelect)]),
        "mk_fastq_cuts": (C.c_int, [u8p, C.c_size_t, C.c_uint64, u64p, C.c_size_t, szp]),
        "mk_fastq_pair_cuts": (C.c_int, [u8p, C.c_size_t, C.c_uint64, u64p, C.c_size_t, szp]),
        "mk_fastq_qtrim_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.POINTER(QtrimOpt), C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, szp, szp, C.POINTER(FastqQtrim)]),
        "mk_fastq_qtrim_device": (C.c_int, [vp, u8p, C.c_size_t, C.POINTER(QtrimOpt), C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_size_t, szp, szp, C.POINTER(FastqQtrim)]),
        "mk_adapters_pack": (C.c_int, [u8p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, szp, C.c_char_p, C.c_size_t]),
        "mk_fastq_adapt_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, u8p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(AdaptOpt),
                                          C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp, szp,
                                          C.POINTER(FastqAdapt)]),
        "mk_fastq_adapt_device": (C.c_int, [vp, u8p, C.c_size_t, u8p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(AdaptOpt),
                                            C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, szp, szp,
                                            C.POINTER(FastqAdapt)]),
        "mk_fastq_overlap_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.POINTER(OverlapOpt), C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, szp, szp, C.POINTER(FastqOverlap)]),
        "mk_fastq_overlap_device": (C.c_int, [vp, u8p, C.c_size_t, C.POINTER(OverlapOpt), C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_size_t, szp, szp, C.POINTER(FastqOverlap)]),
        "mk_fastq_qc_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.POINTER(QcOpt), C.c_size_t, C.POINTER(QcOut), szp,
                                       C.POINTER(FastqQc)]),
        "mk_fastq_qc_device": (C.c_int, [vp, u8p, C.c_size_t, C.POINTER(QcOpt), C.c_size_t, C.POINTER(QcOut), szp, C.POINTER(FastqQc)]),
        "mk_fastq_dedup_text": (C.c_int, [vp, u8p, C.c_size_t, C.c_size_t, C.POINTER(DedupOpt), C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, szp, szp, C.POINTER(FastqDedup)]),
        "mk_fastq_dedup_device": (C.c_int, [vp, u8p, C.c_size_t, C.POINTER(DedupOpt), C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_size_t, szp, szp, C.POINTER(FastqDedup)]),
        "mk_fq_interleave": (C.c_int, [u8p, C.c_size_t, u8p, C.c_size_t, C.c_void_p, C.c_size_t, szp, szp]),
        "mk_fq_split_pairs": (C.c_int, [u8p, C.c_size_t, C.c_void_p, C.c_size_t, szp, C.c_void_p, C.c_size_t, szp, szp]),
    }
    L.mk_version.restype = C.c_char_p
    ver = (L.mk_version() or b"").decode()
    try:
        abi = int(ver.split()[1].split(".")[0])
    except (IndexError, ValueError):
        abi = -1
    if abi != MK_ABI:
        raise MercatHipError(-4, "%s announces '%s' but this binding is written for ABI %d: rebuild the library "
                                 "(make -C mercat2_amd/csrc) -- struct layouts would not match" % (path, ver, MK_ABI))
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _LIB = L
    return L


def _buf_ptr(data) -> Tuple[int, int, object]:
    """(address, nbytes, keepalive) of a bytes-like object without copying."""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        return a.ctypes.data, a.nbytes, a
    mv = memoryview(data)
    if mv.nbytes == 0:
        return 0, 0, None
    a = np.frombuffer(mv, dtype=np.uint8)  # works for read-only buffers (bytes, mmap) too
    return a.__array_interface__["data"][0], a.nbytes, a


def _big_u8(n: int) -> np.ndarray:
    """Writable uint8 buffer from an anonymous mmap.  (np.empty madvises huge pages for large
    blocks, which makes the first touch of every page very slow in some sandboxes.)"""
    import mmap
    if n == 0:
        return np.empty(0, dtype=np.uint8)
    return np.frombuffer(mmap.mmap(-1, n), dtype=np.uint8)


def _fastq_in(path_or_bytes, count: bool = True) -> Tuple[int, int, object, int]:
    """(address, nbytes, keepalive, records) of a FASTQ text given as a path to a plain file or as bytes: its 4-line
    records, lines split on '\\n', a last line without one counting as a line (0 where ``count`` is off)."""
    if isinstance(path_or_bytes, (str, os.PathLike)):
        with open(path_or_bytes, "rb") as fh:
            path_or_bytes = fh.read()
    addr, size, held = _buf_ptr(path_or_bytes)
    if not count:
        return addr, size, held, 0
    nl = int(np.count_nonzero(held == 10)) if size else 0
    return addr, size, held, (nl + (1 if size and held[-1] != 10 else 0)) // 4


def _fastq_out(size: int) -> np.ndarray:
    """The output array of a call that writes records of a text of ``size`` bytes: at most one newline longer."""
    return np.empty(size + 1, dtype=np.uint8)


# ------------------------------------------------------------------------------ host helpers
def chunk_cuts(text, chunksize: int) -> np.ndarray:
    """Offsets at which the reference Chunker would start chunks 1.. (lib/mercat2_Chunker.py:39-59)."""
    L = lib()
    addr, n, keep = _buf_ptr(text)
    need = C.c_size_t(0)
    cap = 64
    while True:
        cuts = np.empty(cap, dtype=np.uint64)
        rc = L.mk_chunk_cuts(addr, n, int(chunksize), cuts.ctypes.data, cap, C.byref(need))
        if rc == MK_OK:
            return cuts[: need.value].copy()
        if rc != -7:
            raise MercatHipError(rc, "mk_chunk_cuts")
        cap = need.value


def remove_n(text, toupper: bool = False) -> Tuple[bytes, dict]:
    """mk_remove_n: (cleaned FASTA text, mk_clean_stats_t fields).  IndexError for a record to be split whose header is
    empty (as the reference raises it), NonAsciiInput for a byte >= 0x80 in a sequence line."""
    L = lib()
    addr, n, keep = _buf_ptr(text)
    out, out_len, st = C.c_void_p(), C.c_size_t(0), CleanStats()
    rc = L.mk_remove_n(addr, n, 1 if toupper else 0, C.byref(out), C.byref(out_len), C.byref(st))
    if rc == -7:
        raise IndexError("list index out of range")  # header.split()[0] of an empty header (lib/mercat2_fasta.py:40-41)
    if rc == -5:
        raise NonAsciiInput(rc, "record %d holds sequence byte(s) >= 0x80 (non-ASCII sequence text is not supported)" % st.unsupported_record)
    if rc:
        raise MercatHipError(rc, "mk_remove_n")
    try:
        data = C.string_at(out, out_len.value) if out.value else b""
    finally:
        if out.value:
            L.mk_free(out)
    return data, {n_: int(getattr(st, n_)) for n_, _ in st._fields_}


def fq2fa(raw) -> Tuple[bytes, dict]:
    """mk_fq2fa: (the text MerCat2's fq2fa writes into <base>.fna.gz, uncompressed; mk_fastq_stats_t fields) of a whole
    FASTQ text.  NonAsciiInput for a byte >= 0x80 in a line of the converted text that is not a header line."""
    L = lib()
    addr, n, keep = _buf_ptr(raw)
    out, out_len, st = C.c_void_p(), C.c_size_t(0), FastqStats()
    rc = L.mk_fq2fa(addr, n, C.byref(out), C.byref(out_len), C.byref(st))
    if rc == -5:
        raise NonAsciiInput(rc, "the converted FASTQ text holds sequence byte(s) >= 0x80 (non-ASCII sequence text is not supported)")
    if rc:
        raise MercatHipError(rc, "mk_fq2fa")
    try:
        data = C.string_at(out, out_len.value) if out_len.value else b""
    finally:
        if out.value:
            L.mk_free(out)
    return data, {n_: int(getattr(st, n_)) for n_, _ in st._fields_}


def _host_error(rc: int, what: str) -> MercatHipError:
    return MercatHipError(rc, (lib().mk_host_error() or b"").decode("utf-8", "replace") or what)


def interleave(a, b) -> bytes:
    """mk_interleave: record i of FASTA text ``a``, then record i of ``b`` (the R1 / R2 files of paired reads), records
    delimited as Counter.filter delimits them, on the host.  The preambles are dropped and a last record without a line
    end gets a newline.  MercatHipError (MK_ERR_RANGE) when the texts hold different numbers of records."""
    L = lib()
    a1, n1, k1 = _buf_ptr(a)
    a2, n2, k2 = _buf_ptr(b)
    out = np.empty(n1 + n2 + 2, dtype=np.uint8)
    out_len, pairs = C.c_size_t(0), C.c_size_t(0)
    rc = L.mk_interleave(a1, n1, a2, n2, out.ctypes.data, out.size, C.byref(out_len), C.byref(pairs))
    if rc:
        raise _host_error(rc, "mk_interleave")
    return out[: out_len.value].tobytes()


def split_pairs(text) -> Tuple[bytes, bytes]:
    """mk_split_pairs: (records 0, 2, 4, ...; records 1, 3, 5, ...) of an interleaved FASTA text, byte for byte, on the
    host.  MercatHipError (MK_ERR_RANGE) for an odd number of records."""
    L = lib()
    addr, n, keep = _buf_ptr(text)
    o1, o2 = np.empty(max(n, 1), dtype=np.uint8), np.empty(max(n, 1), dtype=np.uint8)
    l1, l2, pairs = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = L.mk_split_pairs(addr, n, o1.ctypes.data, n, C.byref(l1), o2.ctypes.data, n, C.byref(l2), C.byref(pairs))
    if rc:
        raise _host_error(rc, "mk_split_pairs")
    return o1[: l1.value].tobytes(), o2[: l2.value].tobytes()


def interleave_fastq(a, b) -> bytes:
    """mk_fq_interleave: record i of FASTQ text ``a``, then record i of ``b`` (the R1 / R2 files of paired reads), on the
    host.  Records are the 4-line records of Counter.fastq_select; a last record without a newline gets one.
    MercatHipError (MK_ERR_RANGE) when the texts hold different numbers of records, (MK_ERR_UNSUPPORTED) when one ends
    inside a record."""
    L = lib()
    a1, n1, k1 = _buf_ptr(a)
    a2, n2, k2 = _buf_ptr(b)
    out = np.empty(n1 + n2 + 2, dtype=np.uint8)
    out_len, pairs = C.c_size_t(0), C.c_size_t(0)
    rc = L.mk_fq_interleave(a1, n1, a2, n2, out.ctypes.data, out.size, C.byref(out_len), C.byref(pairs))
    if rc:
        raise _host_error(rc, "mk_fq_interleave")
    return out[: out_len.value].tobytes()


def split_pairs_fastq(text) -> Tuple[bytes, bytes]:
    """mk_fq_split_pairs: (records 0, 2, 4, ...; records 1, 3, 5, ...) of an interleaved FASTQ text, on the host.
    MercatHipError (MK_ERR_RANGE) for an odd number of records."""
    L = lib()
    addr, n, keep = _buf_ptr(text)
    o1, o2 = np.empty(n + 1, dtype=np.uint8), np.empty(n + 1, dtype=np.uint8)
    l1, l2, pairs = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = L.mk_fq_split_pairs(addr, n, o1.ctypes.data, n + 1, C.byref(l1), o2.ctypes.data, n + 1, C.byref(l2), C.byref(pairs))
    if rc:
        raise _host_error(rc, "mk_fq_split_pairs")
    return o1[: l1.value].tobytes(), o2[: l2.value].tobytes()


def fastq_cuts(text, piece: int, pairs: bool = False) -> np.ndarray:
    """Where Counter.fastq_select cuts a FASTQ text into pieces (mk_fastq_cuts): behind a line 4j once a piece holds
    ``piece`` bytes.  ``pairs``: where Counter.fastq_qtrim cuts paired reads (mk_fastq_pair_cuts): behind a line 8j."""
    L = lib()
    scan = L.mk_fastq_pair_cuts if pairs else L.mk_fastq_cuts
    addr, n, keep = _buf_ptr(text)
    need = C.c_size_t(0)
    cap = 64
    while True:
        cuts = np.empty(cap, dtype=np.uint64)
        rc = scan(addr, n, int(piece), cuts.ctypes.data, cap, C.byref(need))
        if rc == MK_OK:
            return cuts[: need.value].copy()
        if rc != -7:
            raise MercatHipError(rc, "mk_fastq_cuts")
        cap = need.value


def _select_arrays(keep, kept) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], int]:
    """keep as uint8, kept as uint64 (each or both None) and the number of records they speak of (-1: neither given)."""
    keep = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8, copy=False)).reshape(-1)
    kept = None if kept is None else np.ascontiguousarray(np.asarray(kept).astype(np.uint64, copy=False)).reshape(-1)
    if keep is not None and kept is not None and len(keep) != len(kept):
        raise ValueError("keep speaks of %d records, kept of %d" % (len(keep), len(kept)))
    return keep, kept, (len(keep) if keep is not None else len(kept) if kept is not None else -1)


def textwrap_lines(text, width: int = 80) -> list:
    """mk_textwrap: the lines the library's restatement of textwrap.wrap gives (bytes each)."""
    L = lib()
    addr, n, keep = _buf_ptr(text)
    out, out_len = C.c_void_p(), C.c_size_t(0)
    rc = L.mk_textwrap(addr, n, int(width), C.byref(out), C.byref(out_len))
    if rc:
        raise MercatHipError(rc, "mk_textwrap")
    try:
        data = C.string_at(out, out_len.value) if out.value else b""
    finally:
        if out.value:
            L.mk_free(out)
    return data.split(b"\n")[:-1] if data else []


_COLUMN_CAP = 4096  # bytes kept for a count table's column title


def tsv_shape(path) -> dict:
    """mk_tsv_shape: {"k": key length of the first data row (0: none), "header": line 1 is not a data row, "column": its
    second field, "alphabet": ALPHABET_NT2 / ALPHABET_AA5 / ALPHABET_RAW by the keys of the first 4096 rows} of a count
    table in text form.  No GPU is touched."""
    L = lib()
    k, header, hint = C.c_int(0), C.c_int(0), C.c_int(0)
    column = C.create_string_buffer(_COLUMN_CAP)
    rc = L.mk_tsv_shape(os.fsencode(str(path)), C.byref(k), C.byref(header), C.byref(hint), column, _COLUMN_CAP)
    if rc:
        raise MercatHipError(rc, (L.mk_last_error(None) or b"").decode())
    return {"k": k.value, "header": bool(header.value), "column": column.value.decode("utf-8", "replace"), "alphabet": hint.value}


def counter_from_tsv(path, alphabet: Optional[int] = None, device: int = 0, canonical: bool = False) -> Tuple["Counter", dict]:
    """(Counter, info): a new context of the table's key length holding the rows of the count table at ``path``
    (Counter.load_tsv); ``info`` is load_tsv's result.  ``alphabet`` None: the hint of tsv_shape.  A table without a
    data row gives an empty context of k = 1.  The caller closes the Counter."""
    shape = tsv_shape(path)
    if alphabet is None:
        alphabet = shape["alphabet"]
    ctx = Counter(max(1, shape["k"]), alphabet, device, canonical=canonical and alphabet == ALPHABET_NT2)
    try:
        info = ctx.load_tsv(path) if shape["k"] else dict(TsvLoad().as_dict(), column=shape["column"])
    except BaseException:
        ctx.close()
        raise
    return ctx, info


def default_streams(k: int, alphabet: int) -> int:
    """Contexts that pay off per GPU: a second one fills the gaps between the kernels of a chunk when
    keys are one word (nucleotide k <= 32, protein k <= 12: measured +18 % on S2); with two-word keys
    (33..64-mers) the long LDS-bound count kernels of two contexts only get in each other's way
    (measured -30 % at k = 63), and the by-reference modes gain nothing."""
    one_word = (alphabet == ALPHABET_NT2 and k <= 32) or (alphabet == ALPHABET_AA5 and k <= 12)
    return 2 if one_word else 1


def gunzip(gz, cap: int, block: int = 4 << 20) -> Tuple[bytes, int]:
    """(text, members) of a gzip file held in memory, through the file reader's own decoder (mk_gunzip)."""
    L = lib()
    addr, n, keep = _buf_ptr(gz)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    written, members = C.c_size_t(0), C.c_int(0)
    rc = L.mk_gunzip(addr, n, out.ctypes.data, cap, int(block), C.byref(written), C.byref(members))
    if rc:
        raise MercatHipError(rc, "mk_gunzip")
    return out[: written.value].tobytes(), members.value


def gunzip_parallel(gz, cap: int, threads: int = 4, piece: int = 1 << 20) -> Tuple[bytes, int]:
    """(text, members) through the parallel decoder (mk_gunzip_parallel)."""
    L = lib()
    addr, n, keep = _buf_ptr(gz)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    written, members = C.c_size_t(0), C.c_int(0)
    rc = L.mk_gunzip_parallel(addr, n, out.ctypes.data, cap, int(threads), int(piece), C.byref(written), C.byref(members))
    if rc:
        raise MercatHipError(rc, "mk_gunzip_parallel")
    return out[: written.value].tobytes(), members.value


def stream_cuts(text, chunksize: int, block: int) -> np.ndarray:
    """chunk_cuts through the streaming scanner of mk_count_file, the text handed over ``block`` bytes
    at a time; raises if the scanner lost, repeated or misplaced a byte."""
    L = lib()
    addr, n, keep = _buf_ptr(text)
    need = C.c_size_t(0)
    cap = 64
    while True:
        cuts = np.empty(cap, dtype=np.uint64)
        rc = L.mk_stream_cuts(addr, n, int(chunksize), int(block), cuts.ctypes.data, cap, C.byref(need))
        if rc == MK_OK:
            return cuts[: need.value].copy()
        if rc != -7:
            raise MercatHipError(rc, "mk_stream_cuts")
        cap = need.value


def record_cuts(text, piece: int, block: int = 1 << 20) -> np.ndarray:
    """Where mk_count_file cuts one filter unit that it spreads over several GPUs (mk_record_cuts): pieces of at
    least ``piece`` bytes that end where a record starts."""
    L = lib()
    addr, n, keep = _buf_ptr(text)
    need = C.c_size_t(0)
    cap = 64
    while True:
        cuts = np.empty(cap, dtype=np.uint64)
        rc = L.mk_record_cuts(addr, n, int(piece), int(block), cuts.ctypes.data, cap, C.byref(need))
        if rc == MK_OK:
            return cuts[: need.value].copy()
        if rc != -7:
            raise MercatHipError(rc, "mk_record_cuts")
        cap = need.value


def device_count() -> int:
    """HIP devices this process sees (mk_device_count)."""
    return int(lib().mk_device_count())


def owner_bounds(key_bits: int, n: int) -> list:
    """mk_owner_bounds: first key of owner 1..n-1 when [0, 2^key_bits) is cut into n equal ranges."""
    out = np.zeros(max(1, n - 1), dtype=np.uint64)
    rc = lib().mk_owner_bounds(int(key_bits), int(n), out.ctypes.data)
    if rc:
        raise MercatHipError(rc, "mk_owner_bounds")
    return [int(x) for x in out[: n - 1]]


def plan_contexts(devices: Sequence[int], streams: int) -> list:
    """mk_plan_contexts: device of every context, in creation order, so that mk_count_file's "chunk i -> ctxs[i mod
    nctx]" means device devices[i mod ndev] with the chunks of a device taking turns on its streams."""
    nd = len(devices)
    arr = (C.c_int * nd)(*[int(d) for d in devices])
    out = (C.c_int * (nd * int(streams)))()
    rc = lib().mk_plan_contexts(arr, nd, int(streams), out)
    if rc:
        raise MercatHipError(rc, "mk_plan_contexts")
    return list(out)


def _ctx_array(ctxs: Sequence["Counter"]):
    return (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])


def merge_devices(ctxs: Sequence["Counter"], flags: int = MERGE_RANGES) -> dict:
    """mk_merge_devices: sum the running tables of contexts on several GPUs (or several on one) in this process.
    MERGE_RANGES: ctxs[i] ends up with key range i; MERGE_GATHER: everything in ctxs[0]."""
    st = MergeStats()
    rc = lib().mk_merge_devices(_ctx_array(ctxs), len(ctxs), int(flags), C.byref(st))
    if rc:
        ctxs[0]._check(rc)
    return st.as_dict()


def rows_multi(ctxs: Sequence["Counter"]) -> int:
    n = C.c_size_t(0)
    rc = lib().mk_export_size_multi(_ctx_array(ctxs), len(ctxs), C.byref(n))
    if rc:
        ctxs[0]._check(rc)
    return n.value


def export_multi(ctxs: Sequence["Counter"]) -> Tuple[np.ndarray, np.ndarray]:
    """mk_export_multi: the sorted table of contexts that hold ascending key ranges (after MERGE_RANGES)."""
    rows = rows_multi(ctxs)
    kmers = np.empty((rows, ctxs[0].k), dtype=np.uint8)
    counts = np.empty(rows, dtype=np.uint64)
    rc = lib().mk_export_multi(_ctx_array(ctxs), len(ctxs), kmers.ctypes.data, counts.ctypes.data, rows)
    if rc:
        ctxs[0]._check(rc)
    return kmers, counts


def write_tsv_multi(ctxs: Sequence["Counter"], path, basename: str) -> int:
    n = C.c_size_t(0)
    rc = lib().mk_write_tsv_multi(_ctx_array(ctxs), len(ctxs), os.fsencode(str(path)), basename.encode(), C.byref(n))
    if rc:
        ctxs[0]._check(rc)
    return n.value


def count_file(ctxs: Sequence["Counter"], path, chunk_bytes: int, min_count: int, threads: int = 0) -> dict:
    """mk_count_file: read (inflate) ``path``, apply the Chunker rule iff its on-disk size is >=
    chunk_bytes > 0, count every chunk with its own min_count filter on the contexts in turn (they may sit on
    several GPUs: plan_contexts) and leave the sum in ctxs[0].  Returns the mk_file_stats_t fields."""
    L = lib()
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    st = FileStats()
    rc = L.mk_count_file(arr, len(ctxs), os.fsencode(str(path)), int(chunk_bytes), int(min_count), int(threads),
                         C.byref(st))
    if rc:
        ctxs[0]._check(rc)
    return st.as_dict()


def merged_export(ctxs: Sequence["Counter"]) -> Tuple[np.ndarray, np.ndarray]:
    """(kmers (rows, k) uint8, matrix (rows, len(ctxs)) uint64): every k-mer of any sample in sorted
    order with its count per sample, 0 where absent (mk_merged_export)."""
    L = lib()
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    rows = C.c_size_t(0)
    ctxs[0]._check(L.mk_merged_export(arr, len(ctxs), None, None, 0, C.byref(rows)))
    kmers = np.empty((rows.value, ctxs[0].k), dtype=np.uint8)
    matrix = np.empty((rows.value, len(ctxs)), dtype=np.uint64)
    if rows.value:
        ctxs[0]._check(L.mk_merged_export(arr, len(ctxs), kmers.ctypes.data, matrix.ctypes.data, rows.value, C.byref(rows)))
    return kmers, matrix


def write_merged_tsv(ctxs: Sequence["Counter"], names: Sequence[str], path, first_column: str = "k-mer",
                     as_reference: bool = False) -> int:
    """mk_write_merged_tsv: the combined table of merge_tsv (lib/mercat2_report.py:98-156) from the tables -- the true
    union, or with ``as_reference`` the rows exactly as the reference's streaming loop writes them (see the header)."""
    L = lib()
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    cn = (C.c_char_p * len(names))(*[n.encode() for n in names])
    rows = C.c_size_t(0)
    fn = L.mk_write_merged_tsv_as_reference if as_reference else L.mk_write_merged_tsv
    ctxs[0]._check(fn(arr, len(ctxs), cn, first_column.encode(), os.fsencode(str(path)), C.byref(rows)))
    return rows.value


def write_merged_tsv_T(ctxs: Sequence["Counter"], names: Sequence[str], path) -> int:
    """mk_write_merged_tsv_t: the file merge_tsv_T (lib/mercat2_report.py:160-194) writes, columns sorted."""
    L = lib()
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    cn = (C.c_char_p * len(names))(*[n.encode() for n in names])
    rows = C.c_size_t(0)
    ctxs[0]._check(L.mk_write_merged_tsv_t(arr, len(ctxs), cn, os.fsencode(str(path)), C.byref(rows)))
    return rows.value


def _gram_ints(g: np.ndarray, n: int) -> list:
    """n x n nested lists of Python ints from n*n {lo, hi} uint64 pairs."""
    g = g.reshape(n, n, 2)
    return [[int(g[i, j, 0]) | (int(g[i, j, 1]) << 64) for j in range(n)] for i in range(n)]


def gram(ctxs: Sequence["Counter"], slab_rows: int = 0) -> Tuple[list, int]:
    """mk_gram: (G, rows): the exact Gram matrix X X^T (n x n nested lists of Python ints) of the samples' count
    columns over the union of their k-mers (X = merged_export's matrix, transposed), and the number of union rows.
    ``slab_rows`` caps the union rows held on the device at once (0: from free memory)."""
    n = len(ctxs)
    g = np.zeros(2 * n * n, dtype=np.uint64)
    rows = C.c_size_t(0)
    rc = lib().mk_gram(_ctx_array(ctxs), n, int(slab_rows), g.ctypes.data, C.byref(rows))
    if rc:
        ctxs[0]._check(rc)
    return _gram_ints(g, n), rows.value


def gram_matrix(matrix: np.ndarray, device: int = 0) -> list:
    """mk_gram_matrix: the exact X^T X (n x n nested lists of Python ints) of a dense rows x n count matrix."""
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    if m.ndim != 2 or m.shape[1] < 1:
        raise ValueError("gram_matrix: a rows x n matrix with n >= 1 is needed")
    n = m.shape[1]
    g = np.zeros(2 * n * n, dtype=np.uint64)
    L = lib()
    rc = L.mk_gram_matrix(int(device), m.ctypes.data if m.size else None, m.shape[0], n, g.ctypes.data)
    if rc:
        raise MercatHipError(rc, (L.mk_last_error(None) or b"").decode())
    return _gram_ints(g, n)


# mk_pair_t (include/mercat_hip.h): the per-pair statistics beta diversity needs
PAIR_DTYPE = np.dtype([("dot", "<u8", 2), ("l1", "<u8", 2), ("cheb", "<u8"), ("neq", "<u8"), ("both", "<u8"),
                       ("canb", "<f8"), ("seuc", "<f8")])
PAIR_CONSTANT_ROW = 1


def _pair_result(out: np.ndarray, sums: np.ndarray, n: int, rows: int, flags: int) -> dict:
    out = out.reshape(n, n)
    wide = lambda a: [[int(a[i, j, 0]) | (int(a[i, j, 1]) << 64) for j in range(n)] for i in range(n)]
    return {"dot": wide(out["dot"]), "l1": wide(out["l1"]), "cheb": out["cheb"].copy(), "neq": out["neq"].copy(),
            "both": out["both"].copy(), "canb": out["canb"].copy(), "seuc": out["seuc"].copy(),
            "sums": [int(sums[2 * i]) | (int(sums[2 * i + 1]) << 64) for i in range(n)], "rows": int(rows),
            "constant_row": bool(flags & PAIR_CONSTANT_ROW)}


def pair_stats(ctxs: Sequence["Counter"], slab_rows: int = 0) -> dict:
    """mk_pair_stats: the per-pair statistics of the samples' count columns over the union of their k-mers.
    Returns {"dot", "l1": n x n nested lists of Python ints; "cheb", "neq", "both": n x n uint64 arrays; "canb",
    "seuc": n x n float64 arrays; "sums": the n column sums (Python ints); "rows": union rows; "constant_row": some
    row holds the same count in every sample}.  ``slab_rows`` as for ``gram``."""
    n = len(ctxs)
    out = np.zeros(n * n, dtype=PAIR_DTYPE)
    sums = np.zeros(2 * n, dtype=np.uint64)
    rows = C.c_size_t(0)
    flags = np.zeros(1, dtype=np.uint64)
    rc = lib().mk_pair_stats(_ctx_array(ctxs), n, int(slab_rows), out.ctypes.data, sums.ctypes.data, C.byref(rows),
                             flags.ctypes.data)
    if rc:
        ctxs[0]._check(rc)
    return _pair_result(out, sums, n, rows.value, int(flags[0]))


def pair_stats_matrix(matrix: np.ndarray, device: int = 0) -> dict:
    """mk_pair_stats_matrix: ``pair_stats`` of a dense rows x n count matrix (counts below 2^63)."""
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    if m.ndim != 2 or m.shape[1] < 1:
        raise ValueError("pair_stats_matrix: a rows x n matrix with n >= 1 is needed")
    n = m.shape[1]
    out = np.zeros(n * n, dtype=PAIR_DTYPE)
    sums = np.zeros(2 * n, dtype=np.uint64)
    flags = np.zeros(1, dtype=np.uint64)
    L = lib()
    rc = L.mk_pair_stats_matrix(int(device), m.ctypes.data if m.size else None, m.shape[0], n, out.ctypes.data,
                                sums.ctypes.data, flags.ctypes.data)
    if rc:
        raise MercatHipError(rc, (L.mk_last_error(None) or b"").decode())
    return _pair_result(out, sums, n, m.shape[0], int(flags[0]))


def lookup_multi(ctxs: Sequence["Counter"], keys, fold: Optional[bool] = None) -> np.ndarray:
    """The counts of ``keys`` in a table spread over ``ctxs`` by key range (after merge_devices with MERGE_RANGES): every
    key has one owner there, so the answer is the sum of the contexts' lookups."""
    total = None
    for c in ctxs:
        got = c.lookup(keys, fold)
        total = got if total is None else total + got
    return total if total is not None else np.zeros(0, dtype=np.uint64)


def histo_multi(ctxs: Sequence["Counter"], high: int = 10000) -> np.ndarray:
    """The abundance histogram (Counter.histo) of a table spread over ``ctxs`` by key range (after merge_devices with
    MERGE_RANGES): every key has one owner there, so the sum of the contexts' histograms is the table's.  Wrong for
    contexts whose key sets overlap: a key two of them hold is two rows here, each under its own partial count."""
    total = np.zeros(int(high) + 2, dtype=np.uint64)
    for c in ctxs:
        total += c.histo(high)
    return total


def synth_reads(genome_len: int, genome_seed: int, reads: int, read_len: int, read_seed: int,
                sub_ppm: int = 0, first_index: int = 0) -> np.ndarray:
    """Deterministic synthetic FASTA reads as a uint8 array."""
    L = lib()
    size = C.c_size_t(0)
    rc = L.mk_synth_reads(genome_len, genome_seed, reads, read_len, read_seed, sub_ppm, first_index, None, 0, C.byref(size))
    if rc:
        raise MercatHipError(rc, "mk_synth_reads(size)")
    out = _big_u8(size.value)
    rc = L.mk_synth_reads(genome_len, genome_seed, reads, read_len, read_seed, sub_ppm, first_index,
                          out.ctypes.data, out.nbytes, C.byref(size))
    if rc:
        raise MercatHipError(rc, "mk_synth_reads")
    return out


# ----------------------------------------------------------------------------------- context
class Counter:
    """One GPU counting context for a fixed (alphabet, k): wraps mk_ctx."""

    def __init__(self, k: int, alphabet: int = ALPHABET_NT2, device: int = 0, canonical: bool = False):
        self._L = lib()
        self._h = C.c_void_p()
        self.k, self.alphabet, self.device = int(k), int(alphabet), int(device)
        rc = self._L.mk_create(self.device, self.alphabet, self.k, C.byref(self._h))
        if rc:
            msg = self._L.mk_last_error(None)
            raise MercatHipError(rc, msg.decode() if msg else "mk_create")
        self.canonical = False
        if canonical:
            self.set_canonical(True)

    # -- plumbing
    def _check(self, rc: int):
        if rc:
            msg = self._L.mk_last_error(self._h)
            text = msg.decode() if msg else ""
            raise (NonAsciiInput if rc == -5 else CleanUnsupported if rc == -8 else MercatHipError)(rc, text)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.mk_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- counting
    def set_canonical(self, on: bool):
        """Opt-in extension (not reference behaviour): count min(kmer, reverse complement)."""
        self._check(self._L.mk_set_canonical(self._h, 1 if on else 0))
        self.canonical = bool(on)

    def set_clean(self, on: bool, toupper: bool = False):
        """Count RAW nucleotide FASTA as removeN would leave it (mk_set_clean): N runs cut records, text in front of the
        first header is dropped, -toupper applies after the cut.  One chunk per file; CleanUnsupported when the text
        holds something the GPU does not reproduce."""
        self._check(self._L.mk_set_clean(self._h, 1 if on else 0, 1 if toupper else 0))

    def clean_stats(self) -> dict:
        st = CleanGpu()
        self._check(self._L.mk_clean_stats(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def clean_runs(self) -> Tuple[np.ndarray, np.ndarray]:
        """The N runs of the last chunk as (starts, ends) in the parsed stream (mk_clean_runs)."""
        n = C.c_size_t(0)
        self._check(self._L.mk_clean_runs(self._h, None, None, 0, C.byref(n)))
        a, b = np.empty(n.value, dtype=np.uint64), np.empty(n.value, dtype=np.uint64)
        if n.value:
            self._check(self._L.mk_clean_runs(self._h, a.ctypes.data, b.ctypes.data, n.value, C.byref(n)))
        return a, b

    def set_fastq(self, on: bool):
        """Count every chunk fed from now on as raw FASTQ, as MerCat2's fq2fa leaves it (mk_set_fastq): one file per
        chunk, rewritten in place on the GPU before the parser.  Nucleotide alphabet; not with clean mode."""
        self._check(self._L.mk_set_fastq(self._h, 1 if on else 0))

    def fastq_stats(self) -> dict:
        """mk_fastq_stats_t fields summed over the chunks counted in FASTQ mode since the last reset."""
        st = FastqStats()
        self._check(self._L.mk_fastq_stats(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def reset(self, expect_rows: int = 0):
        """Forget the running table; with ``expect_rows`` also size it for about that many keys if that is less than
        it has now (mk_reset_for: an owner about to take in its 1/N of a merged table)."""
        if expect_rows:
            self._check(self._L.mk_reset_for(self._h, int(expect_rows)))
        else:
            self._check(self._L.mk_reset(self._h))

    def count_chunk(self, data, min_count: int):
        """One reference find_kmers call: count ``data`` (raw FASTA bytes), keep >= min_count,
        add the survivors into the running table."""
        addr, n, keep = _buf_ptr(data)
        self._check(self._L.mk_chunk_begin(self._h))
        try:
            if n:
                self._check(self._L.mk_chunk_feed(self._h, addr, n))
        except Exception:
            self._L.mk_chunk_end(self._h, 0)
            raise
        self._check(self._L.mk_chunk_end(self._h, int(min_count)))

    def count_device(self, ptr: int, nbytes: int, min_count: int):
        """Count FASTA bytes already resident in this GPU's memory (ptr = device address)."""
        self._check(self._L.mk_count_device(self._h, ptr, int(nbytes), int(min_count)))

    def load_tsv(self, path_or_bytes, piece_bytes: int = 0) -> dict:
        """Insert-add a count table in text form -- a path, or the text itself as bytes -- into the running table
        (mk_load_tsv / mk_load_tsv_text): "<k key bytes>\\t<count>" rows, with or without a header line.  Returns the
        mk_tsv_load_t fields plus "column", the header's second field.  MercatHipError (MK_ERR_RANGE, the message names
        the line) for a malformed row, NonAsciiInput for a byte >= 0x80."""
        st = TsvLoad()
        column = C.create_string_buffer(_COLUMN_CAP)
        if isinstance(path_or_bytes, (str, os.PathLike)):
            rc = self._L.mk_load_tsv(self._h, os.fsencode(str(path_or_bytes)), int(piece_bytes), column, _COLUMN_CAP, C.byref(st))
        else:
            addr, n, keep = _buf_ptr(path_or_bytes)
            rc = self._L.mk_load_tsv_text(self._h, addr, n, int(piece_bytes), column, _COLUMN_CAP, C.byref(st))
        self._check(rc)
        d = st.as_dict()
        d["column"] = column.value.decode("utf-8", "replace")
        return d

    # -- lookups: keys in, counts out (0 = absent), in the order asked; the table is only read
    def _fold_flag(self, fold: Optional[bool]) -> int:
        """fold None: fold iff the context is canonical."""
        if fold is None:
            fold = self.canonical
        return LOOKUP_FOLD if fold else 0

    def _key_rows(self, keys) -> np.ndarray:
        """(rows, k) uint8 from a list of str / bytes of length k, or a (rows, k) / flat uint8 array."""
        if isinstance(keys, np.ndarray):
            if keys.dtype == np.dtype("S%d" % self.k):
                keys = np.ascontiguousarray(keys).view(np.uint8)
            if keys.dtype != np.uint8:  # (no silent cast: an int64 array would wrap into bytes nobody meant)
                raise TypeError("lookup: a key array is uint8 or S%d, not %s" % (self.k, keys.dtype))
            a = np.ascontiguousarray(keys).reshape(-1)
        else:
            items = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in keys]
            if any(len(x) != self.k for x in items):
                raise ValueError("lookup: every key must be %d bytes long" % self.k)
            a = np.frombuffer(b"".join(items), dtype=np.uint8)
        if a.size % self.k:
            raise ValueError("lookup: the keys are not a multiple of %d bytes" % self.k)
        return a.reshape(-1, self.k)

    def lookup(self, keys, fold: Optional[bool] = None, info: Optional[dict] = None) -> np.ndarray:
        """mk_lookup: the count of every key in the running table (uint64, 0 = absent), in the order asked.  ``keys``: a
        list of str / bytes of length k, or a (rows, k) / flat uint8 array.  ``fold`` None: fold iff the context is
        canonical (MK_LOOKUP_FOLD).  ``info``, if given, receives the mk_lookup_t fields."""
        a = self._key_rows(keys)
        counts = np.zeros(a.shape[0], dtype=np.uint64)
        st = Lookup()
        self._check(self._L.mk_lookup(self._h, a.ctypes.data if a.size else None, a.shape[0], self._fold_flag(fold),
                                      counts.ctypes.data if a.size else None, C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return counts

    def lookup_device(self, ptr: int, rows: int, out_ptr: int, fold: Optional[bool] = None) -> dict:
        """mk_lookup_device: ``rows`` keys of k bytes at device address ``ptr`` -> uint64 counts at device address
        ``out_ptr`` (both on this context's GPU).  Returns the mk_lookup_t fields."""
        st = Lookup()
        self._check(self._L.mk_lookup_device(self._h, ptr, int(rows), self._fold_flag(fold), out_ptr, C.byref(st)))
        return st.as_dict()

    def lookup_text(self, path_or_bytes, piece_bytes: int = 0, fold: Optional[bool] = None) -> Tuple[np.ndarray, dict]:
        """mk_lookup_file / mk_lookup_text: (counts, info) of a panel in text form -- a path, or the text itself as bytes
        -- one key a line, a "\t<count>" behind it ignored, so a counts TSV is a panel as it stands.  info: the
        mk_lookup_t fields.  MercatHipError (MK_ERR_RANGE, the message names the line) for a malformed row."""
        is_path = isinstance(path_or_bytes, (str, os.PathLike))
        if is_path:
            size = os.stat(path_or_bytes).st_size
        else:
            addr, size, keep = _buf_ptr(path_or_bytes)
        cap = size // (self.k + 1) + 1  # (a row is at least k bytes and a line end)
        counts = np.zeros(cap, dtype=np.uint64)
        rows, st = C.c_size_t(0), Lookup()
        flags = self._fold_flag(fold)
        if is_path:
            rc = self._L.mk_lookup_file(self._h, os.fsencode(str(path_or_bytes)), int(piece_bytes), flags, counts.ctypes.data,
                                        cap, C.byref(rows), C.byref(st))
        else:
            rc = self._L.mk_lookup_text(self._h, addr, size, int(piece_bytes), flags, counts.ctypes.data, cap, C.byref(rows),
                                        C.byref(st))
        self._check(rc)
        return counts[: rows.value], st.as_dict()

    # -- the abundance spectrum: bins[i] = distinct k-mers that occur i times; the table is only read
    def histo(self, high: int = 10000, info: Optional[dict] = None) -> np.ndarray:
        """mk_histo: uint64 array of ``high + 2`` bins -- bins[c] = rows whose count is c (1 <= c <= high), bins[high + 1] =
        rows whose count is above ``high``, bins[0] = 0.  ``info``, if given, receives the mk_histo_t fields (distinct,
        total, max_count, over_rows, over_total, slots, s_scan, s_total)."""
        bins = np.zeros(max(0, int(high)) + 2, dtype=np.uint64)
        st = Histo()
        self._check(self._L.mk_histo(self._h, int(high), bins.ctypes.data, C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return bins

    def histo_device(self, high: int, out_ptr: int) -> dict:
        """mk_histo_device: the same ``high + 2`` uint64 bins written at device address ``out_ptr`` (on this context's
        GPU).  Returns the mk_histo_t fields."""
        st = Histo()
        self._check(self._L.mk_histo_device(self._h, int(high), out_ptr, C.byref(st)))
        return st.as_dict()

    # -- screening: FASTA text in, one row {windows, hits, sum, min, max} a record out; the table is only read
    def screen(self, path_or_bytes, at_least: int = 1, fold: Optional[bool] = None, piece_bytes: int = 0,
               info: Optional[dict] = None) -> np.ndarray:
        """mk_screen_text: a (records, 5) uint64 array, columns SCREEN_COLUMNS -- per record of the FASTA text (a path to a
        plain file, or the text itself as bytes) its k-length windows, how many of them the table holds ``at_least``
        times, and the sum, smallest and largest of their counts (an absent k-mer counts 0).  One row per header line,
        in order, and a leading one for sequence in front of the first header (info["headless"]).  ``fold`` None: fold
        iff the context is canonical (MK_SCREEN_FOLD).  ``info``, if given, receives the mk_screen_t fields."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, keep = _buf_ptr(path_or_bytes)
        cap = (int(np.count_nonzero(keep == ord(">"))) if size else 0) + 1  # (a record is a header line, or the text in front)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        n, st = C.c_size_t(0), Screen()
        self._check(self._L.mk_screen_text(self._h, addr, size, int(piece_bytes), SCREEN_FOLD if self._fold_flag(fold) else 0,
                                           int(at_least), rows.ctypes.data, cap, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return rows[: n.value]

    def screen_device(self, ptr: int, nbytes: int, out_ptr: int, cap: int, at_least: int = 1, fold: Optional[bool] = None) -> dict:
        """mk_screen_device: ``nbytes`` of FASTA text (whole records) at device address ``ptr`` -> rows of five uint64
        (SCREEN_COLUMNS) at device address ``out_ptr`` with room for ``cap`` of them, both on this context's GPU.  Returns
        the mk_screen_t fields; "records" is the number of rows written."""
        n, st = C.c_size_t(0), Screen()
        self._check(self._L.mk_screen_device(self._h, ptr, int(nbytes), SCREEN_FOLD if self._fold_flag(fold) else 0, int(at_least),
                                             out_ptr, int(cap), C.byref(n), C.byref(st)))
        return st.as_dict()

    # -- filtering: FASTA text in, the bytes of the matched (or unmatched) records out; the table is only read
    def _filter_flags(self, fold: Optional[bool], invert: bool) -> int:
        return (FILTER_FOLD if self._fold_flag(fold) else 0) | (FILTER_INVERT if invert else 0)

    def filter(self, path_or_bytes, at_least: int = 1, min_hits: int = 1, min_ppm: int = 0, invert: bool = False,
               fold: Optional[bool] = None, piece_bytes: int = 0, info: Optional[dict] = None) -> Tuple[bytes, np.ndarray, np.ndarray]:
        """mk_filter_text: (out, keep, rows) -- ``out`` the bytes of the records of the FASTA text (a path to a plain file,
        or the text itself as bytes) that match the rule, in text order and byte for byte; with ``invert`` of those that
        do not.  A record matches iff it has windows, at least ``min_hits`` of them are hits (count >= ``at_least``) and
        hits * 10^6 >= ``min_ppm`` * windows.  ``keep``: one bool per record, True where it was emitted; ``rows``: the
        (records, 5) uint64 array Counter.screen gives for the same text.  ``fold`` None: fold iff the context is
        canonical.  ``info``, if given, receives the mk_filter_t fields (those of mk_screen_t beside them)."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, held = _buf_ptr(path_or_bytes)
        cap = (int(np.count_nonzero(held == ord(">"))) if size else 0) + 1  # (a record is a header line, or the text in front)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        keep = np.zeros(cap, dtype=np.uint8)
        out = np.empty(max(size, 1), dtype=np.uint8)  # (the output is never longer than the text)
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Filter()
        rule = FilterRule(int(at_least), int(min_hits), int(min_ppm), 0)
        self._check(self._L.mk_filter_text(self._h, addr, size, int(piece_bytes), self._filter_flags(fold, invert), C.byref(rule),
                                           out.ctypes.data, size, C.byref(out_len), rows.ctypes.data, keep.ctypes.data, cap,
                                           C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), keep[: n.value].astype(bool), rows[: n.value]

    def filter_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, rows_ptr: int = 0, keep_ptr: int = 0, cap: int = 0,
                      at_least: int = 1, min_hits: int = 1, min_ppm: int = 0, invert: bool = False,
                      fold: Optional[bool] = None) -> dict:
        """mk_filter_device: ``nbytes`` of FASTA text (whole records) at device address ``ptr`` -> the bytes of the emitted
        records at device address ``out_ptr`` (room for ``out_cap``), and, where given, the rows (five uint64 a record) at
        ``rows_ptr`` and one keep byte a record at ``keep_ptr`` with room for ``cap`` records each -- all on this context's
        GPU.  Returns the mk_filter_t fields: "bytes_out" bytes were written, "records" rows."""
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Filter()
        rule = FilterRule(int(at_least), int(min_hits), int(min_ppm), 0)
        self._check(self._L.mk_filter_device(self._h, ptr, int(nbytes), self._filter_flags(fold, invert), C.byref(rule), out_ptr or None,
                                             int(out_cap), C.byref(out_len), rows_ptr or None, keep_ptr or None, int(cap), C.byref(n),
                                             C.byref(st)))
        return st.as_dict()

    # -- a decision applied to the FASTQ text it was taken for: the kept records out with their qualities; no table is read
    def _check_select(self, rc: int):
        if rc:
            msg = self._L.mk_last_error(self._h)
            raise MercatHipError(rc, msg.decode() if msg else "")

    def fastq_select(self, path_or_bytes, keep=None, kept=None, which: int = 1, piece_bytes: int = 0,
                     info: Optional[dict] = None) -> bytes:
        """mk_fastq_select_text: the records of the FASTQ text (a path to a plain file, or the text itself as bytes) that a
        decision keeps, as FASTQ.  ``keep``: one value per record (Counter.filter's / normalize's booleans, Counter.pairs'
        0 / 1 / 2), a record is emitted iff keep[r] == ``which`` (1: the main output, 2: the orphans).  ``kept``: one
        length per record (Counter.trim's), a record is emitted iff kept[r] > 0, its sequence and quality lines cut to
        kept[r] bytes.  Either may be None; with both None the text is validated and copied.  The arrays are coerced to
        uint8 / uint64 and must speak of exactly the text's 4-line records.  MercatHipError: MK_ERR_UNSUPPORTED for a
        malformed record (the message names it), MK_ERR_RANGE for another record count or a kept[r] longer than its read.
        ``info``, if given, receives the mk_fastq_select_t fields."""
        keep, kept, nrec = _select_arrays(keep, kept)
        addr, size, held, own = _fastq_in(path_or_bytes, count=nrec < 0)
        if nrec < 0:  # (neither array: the text's own count)
            nrec = own
        out = _fastq_out(size)
        out_len, st = C.c_size_t(0), FastqSelect()
        self._check_select(self._L.mk_fastq_select_text(
            self._h, addr, size, int(piece_bytes), keep.ctypes.data if keep is not None else None,
            kept.ctypes.data if kept is not None else None, nrec, int(which), out.ctypes.data, size + 1, C.byref(out_len), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes()

    def fastq_select_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, nrec: int, keep_ptr: int = 0, kept_ptr: int = 0,
                            which: int = 1) -> dict:
        """mk_fastq_select_device: ``nbytes`` of FASTQ text (``nrec`` whole records) at device address ``ptr`` -> the
        emitted records at device address ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice) under one
        keep byte a record at ``keep_ptr`` and one uint64 length a record at ``kept_ptr`` (aligned to 8), each optional
        -- all on this context's GPU.  Returns the mk_fastq_select_t fields: "bytes_out" bytes were written."""
        out_len, st = C.c_size_t(0), FastqSelect()
        self._check_select(self._L.mk_fastq_select_device(self._h, ptr, int(nbytes), keep_ptr or None, kept_ptr or None, int(nrec),
                                                          int(which), out_ptr or None, int(out_cap), C.byref(out_len), C.byref(st)))
        return st.as_dict()

    # -- quality trimming and read filtering of a FASTQ text (what MerCat2 leaves to fastp); no table is read
    def fastq_qtrim(self, path_or_bytes, cut_back: int = 20, cut_front: int = 0, min_len: int = 0, max_n=None, low_q: int = 0,
                    max_low_frac: float = 1.0, min_mean_q: int = 0, phred_base: int = 33, paired: bool = False, which: int = 1,
                    piece_bytes: int = 0, info: Optional[dict] = None):
        """mk_fastq_qtrim_text: (out, keep, rows, hist) of the FASTQ text (a path to a plain file, or the text itself as
        bytes).  Every read is cut at its 3' end by the running sum of ``cut_back`` - q (BWA -q, cutadapt -q) and at its
        5' end by that of ``cut_front`` - q (0: that end stays), then dropped if the span left is shorter than
        max(``min_len``, 1), holds more than ``max_n`` N (None: no limit), more than ``max_low_frac`` of its bases below
        ``low_q`` (0: off), or a mean quality below ``min_mean_q`` (0: off).  ``paired``: records 2p and 2p + 1 are mates;
        keep is 1 where both pass, 2 for a read whose mate fails, else 0; ``which`` = 2 writes those orphans.  ``out``: the
        emitted records as FASTQ bytes; ``keep``: uint8 a record; ``rows``: (records, 6) uint64, QTRIM_COLUMNS; ``hist``:
        (2, 256) uint64, the bases of every quality value in the text and in the emitted spans.  MercatHipError:
        MK_ERR_UNSUPPORTED for a malformed record (the message names it), MK_ERR_RANGE for an odd record count with
        ``paired``.  ``info``, if given, receives the mk_fastq_qtrim_t fields."""
        opt = qtrim_options(cut_back, cut_front, min_len, max_n, low_q, max_low_frac, min_mean_q, phred_base, paired, which)
        addr, size, held, cap = _fastq_in(path_or_bytes)
        out = _fastq_out(size)
        keep, rows, hist = np.zeros(cap, dtype=np.uint8), np.zeros((cap, 6), dtype=np.uint64), np.zeros((2, 256), dtype=np.uint64)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqQtrim()
        self._check_select(self._L.mk_fastq_qtrim_text(
            self._h, addr, size, int(piece_bytes), C.byref(opt), cap, keep.ctypes.data, rows.ctypes.data, hist.ctypes.data,
            out.ctypes.data, size + 1, C.byref(out_len), C.byref(nrec), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), keep[: nrec.value], rows[: nrec.value], hist

    def fastq_qtrim_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, cap: int = 0, keep_ptr: int = 0, rows_ptr: int = 0,
                           hist_ptr: int = 0, **options) -> dict:
        """mk_fastq_qtrim_device: ``nbytes`` of FASTQ text at device address ``ptr`` -> the emitted records at device
        address ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice) and, where given, one keep byte a
        record at ``keep_ptr``, six uint64 a record at ``rows_ptr`` (room for ``cap`` records each) and 512 uint64 at
        ``hist_ptr`` (both aligned to 8) -- all on this context's GPU.  ``options``: those of Counter.fastq_qtrim.
        Returns the mk_fastq_qtrim_t fields: "bytes_out" bytes were written, "records" rows."""
        opt = qtrim_options(**options)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqQtrim()
        self._check_select(self._L.mk_fastq_qtrim_device(self._h, ptr, int(nbytes), C.byref(opt), int(cap), keep_ptr or None,
                                                         rows_ptr or None, hist_ptr or None, out_ptr or None, int(out_cap),
                                                         C.byref(out_len), C.byref(nrec), C.byref(st)))
        return st.as_dict()

    # -- per-cycle quality control of a FASTQ text (what MerCat2 asks fastqc for); no table is read
    def fastq_qc(self, path_or_bytes, max_pos: int = 512, phred_base: int = 33, paired: bool = False, rows: bool = False,
                 piece_bytes: int = 0, info: Optional[dict] = None) -> Dict[str, "np.ndarray"]:
        """mk_fastq_qc_text: the quality-control tables of the FASTQ text (a path to a plain file, or the text itself as
        bytes), uint64 arrays under their names: "pos_qual" (C, P + 1, 96): the bases of every quality value at every
        cycle, row P = ``max_pos`` collecting the cycles from P on and bin 95 the values from 95 on; "pos_base" (C, P + 1,
        8): the same for the base classes QC_BASES; "read_len" (C, P + 2): the reads of every length, the last bin those
        longer than P; "read_qual" (C, 96): the reads by their mean quality, rounded down; "read_gc" (C, 101): the reads
        by their GC share in percent, rounded half up.  ``paired``: records 2p and 2p + 1 are mates and C = 2 classes,
        else C = 1.  ``rows``: also "rows", (records, 4) uint64, QC_COLUMNS.  MercatHipError: MK_ERR_UNSUPPORTED for a
        malformed record (the message names it), MK_ERR_RANGE for an odd record count with ``paired``.  ``info``, if
        given, receives the mk_fastq_qc_t fields."""
        opt = qc_options(max_pos, phred_base, paired)
        if not 1 <= opt.max_pos <= QC_MAX_POS:  # (before the tables are sized by it)
            raise MercatHipError(-1, "mk_fastq_qc_text: max_pos must be 1 .. %d" % QC_MAX_POS)
        addr, size, held, cap = _fastq_in(path_or_bytes, count=rows)
        got = {name: np.zeros(shape, dtype=np.uint64) for name, shape in qc_shapes(opt.max_pos, bool(opt.paired)).items()}
        if rows:
            got["rows"] = np.zeros((cap, 4), dtype=np.uint64)
        out = QcOut(**{name: a.ctypes.data for name, a in got.items()})
        nrec, st = C.c_size_t(0), FastqQc()
        self._check_select(self._L.mk_fastq_qc_text(self._h, addr, size, int(piece_bytes), C.byref(opt), cap, C.byref(out),
                                                    C.byref(nrec), C.byref(st)))
        if rows:
            got["rows"] = got["rows"][: nrec.value]
        if info is not None:
            info.update(st.as_dict())
        return got

    def fastq_qc_device(self, ptr: int, nbytes: int, pos_qual_ptr: int, pos_base_ptr: int, read_len_ptr: int, read_qual_ptr: int,
                        read_gc_ptr: int, rows_ptr: int = 0, cap: int = 0, **options) -> dict:
        """mk_fastq_qc_device: ``nbytes`` of FASTQ text at device address ``ptr`` -> the five tables of Counter.fastq_qc
        at the device addresses given (uint64, the sizes of qc_shapes, zeroed by the call) and, where ``rows_ptr`` is
        given, four uint64 a record there (room for ``cap`` records) -- all aligned to 8, all on this context's GPU.
        ``options``: max_pos, phred_base, paired.  Returns the mk_fastq_qc_t fields."""
        opt = qc_options(**options)
        out = QcOut(pos_qual_ptr or None, pos_base_ptr or None, read_len_ptr or None, read_qual_ptr or None, read_gc_ptr or None,
                    rows_ptr or None)
        nrec, st = C.c_size_t(0), FastqQc()
        self._check_select(self._L.mk_fastq_qc_device(self._h, ptr, int(nbytes), C.byref(opt), int(cap), C.byref(out), C.byref(nrec),
                                                      C.byref(st)))
        return st.as_dict()

    # -- duplicate reads of a FASTQ text (fastp --dedup, fastqc's duplication levels); no table is read
    def fastq_dedup(self, path_or_bytes, prefix: int = 0, paired: bool = False, which: int = 1, high: int = 100, piece_bytes: int = 0,
                    info: Optional[dict] = None):
        """mk_fastq_dedup_text: (out, keep, rows, levels) of the FASTQ text (a path to a plain file, or the text itself as
        bytes).  Reads whose sequence bytes are equal (``prefix`` > 0: whose first ``prefix`` bases are) form a cluster;
        ``paired``: records 2p and 2p + 1 are mates and pairs equal in both mates do.  The first of a cluster, over the
        whole text, is kept.  ``out``: the kept records (``which`` = 2: the others) as FASTQ bytes, whole; ``keep``:
        uint8 a record; ``rows``: (records, 2) uint64, DEDUP_COLUMNS: the length and the record that stands for this one;
        ``levels``: (high + 2,) uint64: the clusters of i copies, the last those of more than ``high``.  MercatHipError:
        MK_ERR_UNSUPPORTED for a malformed record (the message names it), MK_ERR_RANGE for an odd record count with
        ``paired``.  ``info``, if given, receives the mk_fastq_dedup_t fields."""
        opt = dedup_options(prefix, paired, which, high)
        if not 1 <= opt.high <= DEDUP_MAX_HIGH:  # (before levels is sized by it)
            raise MercatHipError(-1, "mk_fastq_dedup_text: high must lie in 1 .. 2^20")
        addr, size, held, cap = _fastq_in(path_or_bytes)
        out = _fastq_out(size)
        keep, rows = np.zeros(cap, dtype=np.uint8), np.zeros((cap, 2), dtype=np.uint64)
        levels = np.zeros(opt.high + 2, dtype=np.uint64)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqDedup()
        self._check_select(self._L.mk_fastq_dedup_text(
            self._h, addr, size, int(piece_bytes), C.byref(opt), cap, keep.ctypes.data, rows.ctypes.data, levels.ctypes.data,
            out.ctypes.data, size + 1, C.byref(out_len), C.byref(nrec), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), keep[: nrec.value], rows[: nrec.value], levels

    def fastq_dedup_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, cap: int = 0, keep_ptr: int = 0, rows_ptr: int = 0,
                           levels_ptr: int = 0, **options) -> dict:
        """mk_fastq_dedup_device: ``nbytes`` of FASTQ text at device address ``ptr`` -> the emitted records at device
        address ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice) and, where given, one keep byte a
        record at ``keep_ptr``, two uint64 a record at ``rows_ptr`` (room for ``cap`` records each) and high + 2 uint64
        at ``levels_ptr`` (both aligned to 8) -- all on this context's GPU.  ``options``: prefix, paired, which, high.
        Returns the mk_fastq_dedup_t fields: "bytes_out" bytes were written, "records" rows."""
        opt = dedup_options(**options)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqDedup()
        self._check_select(self._L.mk_fastq_dedup_device(self._h, ptr, int(nbytes), C.byref(opt), int(cap), keep_ptr or None,
                                                         rows_ptr or None, levels_ptr or None, out_ptr or None, int(out_cap),
                                                         C.byref(out_len), C.byref(nrec), C.byref(st)))
        return st.as_dict()

    # -- 3' adapter removal from the reads of a FASTQ text (the first job of the fastp run MerCat2 starts); no table is read
    def fastq_adapt(self, path_or_bytes, adapters, adapters2=None, min_overlap: int = 8, max_err: float = 0.1, min_len: int = 0,
                    paired: bool = False, which: int = 1, piece_bytes: int = 0, info: Optional[dict] = None):
        """mk_fastq_adapt_text: (out, keep, rows, hits) of the FASTQ text (a path to a plain file, or the text itself as
        bytes).  Every read is cut at the leftmost position at which one of ``adapters`` (sequences over ACGTN, str or
        bytes, each of 1..128 bases, at most 1024) matches what is left of the read, or runs off its end, over at least
        ``min_overlap`` bases with at most ``max_err`` x overlap mismatches (no indels; an adapter N matches anything, a
        read N nothing but that); of several adapters there, the first listed.  The default overlap of 8 is set for a
        panel of hundreds of adapters: 3, cutadapt's for one adapter, would cut the end of most adapter-free reads by
        chance.  A read of which fewer than max(``min_len``, 1) bases remain is dropped.  ``paired``: records 2p and 2p +
        1 are mates, ``adapters`` are searched in first mates and ``adapters2`` (which needs ``paired``) in second mates;
        keep is 1 where both pass, 2 for a read whose mate is dropped, else 0; ``which`` = 2 writes those orphans.
        ``out``: the emitted records as FASTQ bytes; ``keep``: uint8 a record; ``rows``: (records, 5) uint64,
        ADAPT_COLUMNS, the adapter column indexing info["adapters"] (ADAPT_NO_HIT without a hit); ``hits``: uint64 an
        adapter, the records it cut.  MercatHipError: MK_ERR_ARG for a refused panel or option, MK_ERR_UNSUPPORTED for a
        malformed record (the message names it), MK_ERR_RANGE for an odd record count with ``paired``.  ``info``, if
        given, receives the mk_fastq_adapt_t fields and "adapters", the panel's sequences in index order."""
        if adapters2 is not None and not paired:
            raise ValueError("fastq_adapt: adapters2 are searched in second mates: needs paired")
        opt = adapt_options(min_overlap, max_err, min_len, paired, which)
        bases, lengths, mates, seqs = adapter_arrays(adapters, adapters2)
        addr, size, held, cap = _fastq_in(path_or_bytes)
        out = _fastq_out(size)
        keep, rows, hits = np.zeros(cap, dtype=np.uint8), np.zeros((cap, 5), dtype=np.uint64), np.zeros(len(seqs), dtype=np.uint64)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqAdapt()
        self._check_select(self._L.mk_fastq_adapt_text(
            self._h, addr, size, int(piece_bytes), bases.ctypes.data, lengths.ctypes.data, mates.ctypes.data, len(seqs), C.byref(opt), cap,
            keep.ctypes.data, rows.ctypes.data, hits.ctypes.data, out.ctypes.data, size + 1, C.byref(out_len), C.byref(nrec), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
            info["adapters"] = seqs
        return out[: out_len.value].tobytes(), keep[: nrec.value], rows[: nrec.value], hits

    def fastq_adapt_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, adapters, adapters2=None, cap: int = 0,
                           keep_ptr: int = 0, rows_ptr: int = 0, hits_ptr: int = 0, **options) -> dict:
        """mk_fastq_adapt_device: ``nbytes`` of FASTQ text at device address ``ptr`` -> the emitted records at device
        address ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice) and, where given, one keep byte a
        record at ``keep_ptr``, five uint64 a record at ``rows_ptr`` (room for ``cap`` records each) and one uint64 an
        adapter at ``hits_ptr`` (both aligned to 8) -- all on this context's GPU.  ``adapters``, ``adapters2`` and
        ``options``: those of Counter.fastq_adapt.  Returns the mk_fastq_adapt_t fields: "bytes_out" bytes were written,
        "records" rows."""
        if adapters2 is not None and not options.get("paired"):
            raise ValueError("fastq_adapt_device: adapters2 are searched in second mates: needs paired")
        opt = adapt_options(**options)
        bases, lengths, mates, seqs = adapter_arrays(adapters, adapters2)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqAdapt()
        self._check_select(self._L.mk_fastq_adapt_device(self._h, ptr, int(nbytes), bases.ctypes.data, lengths.ctypes.data,
                                                         mates.ctypes.data, len(seqs), C.byref(opt), int(cap), keep_ptr or None,
                                                         rows_ptr or None, hits_ptr or None, out_ptr or None, int(out_cap),
                                                         C.byref(out_len), C.byref(nrec), C.byref(st)))
        return st.as_dict()

    # -- mate-overlap detection in interleaved pairs: panel-free adapter removal, or merging; no table is read
    def fastq_overlap(self, path_or_bytes, mode="merge", min_overlap: int = 30, max_mismatch: int = 5, max_err: float = 0.2,
                      min_len: int = 0, which: int = 1, piece_bytes: int = 0, info: Optional[dict] = None):
        """mk_fastq_overlap_text: (out, keep, rows) of the interleaved FASTQ text (a path to a plain file, or the text
        itself as bytes): records 2p and 2p + 1 are mates.  Mate 1 is laid against the reverse complement of mate 2 at
        every offset -- mates that do not read through first, the longest overlap first, then read-through -- and the
        first offset whose overlap has at least ``min_overlap`` bases, at most ``max_mismatch`` mismatches and at most
        ``max_err`` x overlap of them is the hit; it gives the fragment length (include/mercat_hip.h has the rule in
        full; the defaults are fastp's 30 / 5 / 20 %; a pair with a mate above OVERLAP_MAX_BASES is not tested).
        ``mode`` "trim": both mates of a pair with a hit are cut to the fragment (adapter removal without a panel), a
        pair whose fragment is shorter than max(``min_len``, 1) is dropped; keep is 1 or 0.  ``mode`` "merge": a pair
        with a hit becomes one read, mate 1 then what mate 2 adds, with a consensus over the overlap (the base of the
        higher quality byte, a base of ACGT before any other); keep is 1 for a merged pair, 0 for one dropped as short,
        2 without a hit, and ``which`` = 2 writes those unmerged pairs as they stand.  ``out``: the emitted records as
        FASTQ bytes; ``keep``: uint8 a record; ``rows``: (records, 5) uint64, OVERLAP_COLUMNS (fragment OVERLAP_NO_HIT
        without a hit).  MercatHipError: MK_ERR_ARG for a refused option, MK_ERR_UNSUPPORTED for a malformed record (the
        message names it), MK_ERR_RANGE for an odd record count.  ``info``, if given, receives the mk_fastq_overlap_t
        fields."""
        opt = overlap_options(mode, min_overlap, max_mismatch, max_err, min_len, which)
        addr, size, held, cap = _fastq_in(path_or_bytes)
        out = _fastq_out(size)
        keep, rows = np.zeros(cap, dtype=np.uint8), np.zeros((cap, 5), dtype=np.uint64)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqOverlap()
        self._check_select(self._L.mk_fastq_overlap_text(
            self._h, addr, size, int(piece_bytes), C.byref(opt), cap, keep.ctypes.data, rows.ctypes.data, out.ctypes.data, size + 1,
            C.byref(out_len), C.byref(nrec), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), keep[: nrec.value], rows[: nrec.value]

    def fastq_overlap_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, cap: int = 0, keep_ptr: int = 0, rows_ptr: int = 0,
                             **options) -> dict:
        """mk_fastq_overlap_device: ``nbytes`` of interleaved FASTQ text at device address ``ptr`` -> the emitted records
        at device address ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice) and, where given, one keep
        byte a record at ``keep_ptr`` and five uint64 a record at ``rows_ptr`` (aligned to 8; room for ``cap`` records
        each) -- all on this context's GPU.  The text is not modified: a merging call works on a copy.  ``options``:
        those of Counter.fastq_overlap.  Returns the mk_fastq_overlap_t fields: "bytes_out" bytes were written,
        "records" rows."""
        opt = overlap_options(**options)
        out_len, nrec, st = C.c_size_t(0), C.c_size_t(0), FastqOverlap()
        self._check_select(self._L.mk_fastq_overlap_device(self._h, ptr, int(nbytes), C.byref(opt), int(cap), keep_ptr or None,
                                                           rows_ptr or None, out_ptr or None, int(out_cap), C.byref(out_len),
                                                           C.byref(nrec), C.byref(st)))
        return st.as_dict()

    # -- tracking: FASTA text in, the count under every window out (and the median a record); the table is only read
    def _track_flags(self, fold: Optional[bool], sat32: bool) -> int:
        return (TRACK_FOLD if self._fold_flag(fold) else 0) | (TRACK_SAT32 if sat32 else 0)

    def track(self, path_or_bytes, at_least: int = 1, fold: Optional[bool] = None, sat32: bool = False, median: bool = False,
              piece_bytes: int = 0, info: Optional[dict] = None):
        """mk_track_text: (counts, offsets, rows, median_or_None) of the FASTA text (a path to a plain file, or the text
        itself as bytes).  ``counts[offsets[r] + j]`` is the count of window j of record r -- the k bytes that start at
        the record's j-th kept character, 0 for a k-mer the table lacks -- ``offsets`` has records + 1 entries and
        ``rows`` is the (records, 5) uint64 array Counter.screen gives for the same text and ``at_least``.  ``median``:
        also element windows // 2 of every record's sorted counts (0 without windows).  ``sat32``: counts and median are
        uint32, clipped at 2^32 - 1 (info["saturated"] of them), else uint64.  ``fold`` None: fold iff the context is
        canonical.  ``info``, if given, receives the mk_track_t fields (those of mk_screen_t beside them)."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, held = _buf_ptr(path_or_bytes)
        cap = (int(np.count_nonzero(held == ord(">"))) if size else 0) + 1  # (a record is a header line, or the text in front)
        dtype = np.uint32 if sat32 else np.uint64
        counts = np.empty(max(size, 1), dtype=dtype)  # (an upper bound: a window starts at a kept character; untouched pages cost nothing)
        offsets = np.zeros(cap + 1, dtype=np.uint64)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        med = np.zeros(cap, dtype=dtype) if median else None
        n, nwin, st = C.c_size_t(0), C.c_size_t(0), Track()
        self._check(self._L.mk_track_text(self._h, addr, size, int(piece_bytes), self._track_flags(fold, sat32), int(at_least),
                                          counts.ctypes.data, size, C.byref(nwin), offsets.ctypes.data,
                                          med.ctypes.data if median else None, rows.ctypes.data, cap, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return counts[: nwin.value], offsets[: n.value + 1], rows[: n.value], (med[: n.value] if median else None)

    def track_device(self, ptr: int, nbytes: int, counts_ptr: int, counts_cap: int, offsets_ptr: int = 0, median_ptr: int = 0,
                     rows_ptr: int = 0, cap: int = 0, at_least: int = 1, fold: Optional[bool] = None, sat32: bool = False) -> dict:
        """mk_track_device: ``nbytes`` of FASTA text (whole records) at device address ``ptr`` -> the counts at device
        address ``counts_ptr`` (room for ``counts_cap`` elements: uint64, or uint32 with ``sat32``) and, where given,
        ``cap`` + 1 uint64 offsets at ``offsets_ptr``, the medians at ``median_ptr`` and the rows (five uint64 a record) at
        ``rows_ptr`` with room for ``cap`` records each -- all on this context's GPU, each aligned to its elements.
        Returns the mk_track_t fields: "windows_out" elements were written, "records" rows."""
        n, nwin, st = C.c_size_t(0), C.c_size_t(0), Track()
        self._check(self._L.mk_track_device(self._h, ptr, int(nbytes), self._track_flags(fold, sat32), int(at_least),
                                            counts_ptr or None, int(counts_cap), C.byref(nwin), offsets_ptr or None,
                                            median_ptr or None, rows_ptr or None, int(cap), C.byref(n), C.byref(st)))
        return st.as_dict()

    # -- trimming: FASTA text in, every record cut in front of its first low-abundance k-mer out; the table is only read
    def trim(self, path_or_bytes=None, at_least: int = 2, min_len: int = 0, fold: Optional[bool] = None, piece_bytes: int = 0,
             info: Optional[dict] = None):
        """Without arguments, mk_trim: free the per-chunk working memory, keep the running table; returns None.
        With a text, mk_trim_text: (out, kept, rows) of the FASTA text (a path to a plain file, or the text itself as bytes).  A
        record is cut in front of the last character of its first k-mer the table holds fewer than ``at_least`` times
        (khmer's trim_on_abundance); ``kept[r]`` is the number of characters record r keeps -- 0, and the record is not
        emitted, when its first k-mer is low, when it has no k-mer, or when fewer than max(``min_len``, k) remain.
        ``out``: the emitted records in order, each its header line as it stands, then the kept characters on one line
        and a newline.  ``rows``: the (records, 5) uint64 array Counter.screen gives for the same text and ``at_least``.
        ``fold`` None: fold iff the context is canonical.  ``info``, if given, receives the mk_trim_t fields (those of
        mk_screen_t beside them)."""
        if path_or_bytes is None:
            self._check(self._L.mk_trim(self._h))
            return None
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, held = _buf_ptr(path_or_bytes)
        cap = (int(np.count_nonzero(held == ord(">"))) if size else 0) + 1  # (a record is a header line, or the text in front)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        kept = np.zeros(cap, dtype=np.uint64)
        out = np.empty(size + 1, dtype=np.uint8)  # (the output is at most one newline longer than the text)
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Trim()
        rule = TrimRule(int(at_least), int(min_len))
        self._check(self._L.mk_trim_text(self._h, addr, size, int(piece_bytes), TRIM_FOLD if self._fold_flag(fold) else 0,
                                         C.byref(rule), out.ctypes.data, size + 1, C.byref(out_len), kept.ctypes.data,
                                         rows.ctypes.data, cap, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), kept[: n.value], rows[: n.value]

    def trim_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, kept_ptr: int = 0, rows_ptr: int = 0, cap: int = 0,
                    at_least: int = 2, min_len: int = 0, fold: Optional[bool] = None) -> dict:
        """mk_trim_device: ``nbytes`` of FASTA text (whole records) at device address ``ptr`` -> the trimmed records at
        device address ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice) and, where given, one uint64 of
        kept characters a record at ``kept_ptr`` and the rows (five uint64 a record) at ``rows_ptr`` with room for
        ``cap`` records each -- all on this context's GPU, the last two aligned to 8.  Returns the mk_trim_t fields:
        "bytes_out" bytes were written, "records" rows."""
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Trim()
        rule = TrimRule(int(at_least), int(min_len))
        self._check(self._L.mk_trim_device(self._h, ptr, int(nbytes), TRIM_FOLD if self._fold_flag(fold) else 0, C.byref(rule),
                                           out_ptr or None, int(out_cap), C.byref(out_len), kept_ptr or None, rows_ptr or None,
                                           int(cap), C.byref(n), C.byref(st)))
        return st.as_dict()

    # -- ORF calling: nucleotide FASTA text in, its six-frame ORFs out as protein FASTA; no table is read
    def orfs(self, path_or_bytes, min_aa: int = 32, start: bool = False, alt_starts: bool = False, strand: str = "both",
             piece_bytes: int = 0, info: Optional[dict] = None):
        """mk_orf_text: (out, rows) of the FASTA text (a path to a plain file, or the text itself as bytes).  ``out``: one
        protein record per ORF of ``min_aa`` codons or more -- '>' name '_' begin+1 '_' frame '_' rank, then the amino
        acids on one line -- in the order (record, right end, forward before reverse).  Stop-to-stop by default;
        ``start``: from the first ATG of a stretch on (``alt_starts``: GTG and TTG too).  ``strand`` "both", "plus" or
        "minus".  ``rows``: (n, 4) uint64: record, begin (0-based, forward strand), aa, frame (1-3 forward, 4-6
        reverse).  The sizes come from a sizing call first.  ``info``, if given, receives the mk_orf_t fields."""
        opt = orf_options(min_aa, start, alt_starts, strand)
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, held = _buf_ptr(path_or_bytes)
        out_len, n, st = C.c_size_t(0), C.c_size_t(0), Orf()
        rc = self._L.mk_orf_text(self._h, addr, size, int(piece_bytes), C.byref(opt), None, 0, C.byref(out_len), None, 0,
                                 C.byref(n), C.byref(st))
        if rc != -7:
            self._check(rc)  # (MK_OK: nothing to write)
        out = np.empty(max(out_len.value, 1), dtype=np.uint8)
        raw = np.zeros(max(n.value, 1), dtype=ORF_ROW_DTYPE)
        if rc:
            self._check(self._L.mk_orf_text(self._h, addr, size, int(piece_bytes), C.byref(opt), out.ctypes.data, out_len.value,
                                            C.byref(out_len), raw.ctypes.data, n.value, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), orf_rows(raw[: n.value])

    def orfs_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, rows_ptr: int = 0, cap: int = 0, **options) -> dict:
        """mk_orf_device: ``nbytes`` of FASTA text (whole records) at device address ``ptr`` -> the protein records at
        device address ``out_ptr`` (room for ``out_cap``) and, where given, the mk_orf_row_t rows (24 bytes each) at
        ``rows_ptr`` (aligned to 8) with room for ``cap`` -- all on this context's GPU.  ``options``: those of
        orf_options.  Returns the mk_orf_t fields; with too little room MercatHipError (MK_ERR_RANGE) whose ``needed``
        holds the sizes (out_len, norfs)."""
        opt = orf_options(**options)
        out_len, n, st = C.c_size_t(0), C.c_size_t(0), Orf()
        rc = self._L.mk_orf_device(self._h, ptr, int(nbytes), C.byref(opt), out_ptr or None, int(out_cap), C.byref(out_len),
                                   rows_ptr or None, int(cap), C.byref(n), C.byref(st))
        if rc == -7:
            msg = self._L.mk_last_error(self._h)
            err = MercatHipError(rc, msg.decode() if msg else "")
            err.needed = (out_len.value, n.value)
            raise err
        self._check(rc)
        return st.as_dict()

    # -- correcting: FASTA text in, every record with its isolated substitutions put right out; the table is only read
    def correct(self, path_or_bytes, at_least: int = 2, fold: Optional[bool] = None, piece_bytes: int = 0,
                info: Optional[dict] = None):
        """mk_correct_text: (out, fix, rows) of the FASTA text (a path to a plain file, or the text itself as bytes).  A
        maximal run of k-mers the table holds fewer than ``at_least`` times that has the shape one substituted base
        leaves -- k of them inside a record, up to k at either end -- names that base; it is replaced iff exactly one
        other base of ACGT makes every k-mer of the run solid (include/mercat_hip.h has the rule).  ``out``: every record
        in order, its header line as it stands, then its characters on one line and a newline.  ``fix``: a (records, 4)
        uint32 array, CORRECT_COLUMNS a record (``fix.view(CorrectRow)`` names them): its weak runs and those fixed,
        ambiguous and unfixable.  ``rows``: the (records, 5) uint64 array Counter.screen gives for the same, uncorrected
        text and ``at_least``.  Nucleotide contexts with k <= 64 only.  ``fold`` None: fold iff the context is
        canonical.  ``info``, if given, receives the mk_correct_t fields (those of mk_screen_t beside them)."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, held = _buf_ptr(path_or_bytes)
        cap = (int(np.count_nonzero(held == ord(">"))) if size else 0) + 1  # (a record is a header line, or the text in front)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        fix = np.zeros((cap, len(CORRECT_COLUMNS)), dtype=np.uint32)
        out = np.empty(size + 1, dtype=np.uint8)  # (the output is at most one newline longer than the text)
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Correct()
        rule = CorrectRule(int(at_least), 0)
        self._check(self._L.mk_correct_text(self._h, addr, size, int(piece_bytes), CORRECT_FOLD if self._fold_flag(fold) else 0,
                                            C.byref(rule), out.ctypes.data, size + 1, C.byref(out_len), fix.ctypes.data,
                                            rows.ctypes.data, cap, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), fix[: n.value], rows[: n.value]

    def correct_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, fix_ptr: int = 0, rows_ptr: int = 0, cap: int = 0,
                       at_least: int = 2, fold: Optional[bool] = None) -> dict:
        """mk_correct_device: ``nbytes`` of FASTA text (whole records) at device address ``ptr`` -> the corrected records at
        device address ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice) and, where given, four uint32 a
        record at ``fix_ptr`` and the rows (five uint64 a record) at ``rows_ptr`` with room for ``cap`` records each --
        all on this context's GPU, the last two aligned to 8.  Returns the mk_correct_t fields: "bytes_out" bytes were
        written, "records" rows."""
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Correct()
        rule = CorrectRule(int(at_least), 0)
        self._check(self._L.mk_correct_device(self._h, ptr, int(nbytes), CORRECT_FOLD if self._fold_flag(fold) else 0,
                                              C.byref(rule), out_ptr or None, int(out_cap), C.byref(out_len), fix_ptr or None,
                                              rows_ptr or None, int(cap), C.byref(n), C.byref(st)))
        return st.as_dict()

    # -- correcting FASTQ: the text in, the same text out with the fixes in its sequence lines and the qualities kept
    def _check_correct_fastq(self, rc: int):
        if rc:
            msg = self._L.mk_last_error(self._h)
            raise (NonAsciiInput if rc == -5 else MercatHipError)(rc, msg.decode() if msg else "")

    def correct_fastq(self, path_or_bytes, at_least: int = 2, new_qual=0, fold: Optional[bool] = None, piece_bytes: int = 0,
                      info: Optional[dict] = None):
        """mk_correct_fastq_text: (out, fix, rows) of the FASTQ text (a path to a plain file, or the text itself as bytes).
        ``out`` is the text byte for byte -- CR LF, an open last record and trailing empty lines included -- but for the
        base of every run Counter.correct would fix in the FASTA view native.fq2fa gives of it; ``fix`` and ``rows`` are
        Counter.correct's for that view.  ``new_qual`` (an int, or one character as str or bytes; 0: none) is written
        over the quality of every fixed base.  MercatHipError: MK_ERR_UNSUPPORTED for a malformed record or a sequence
        line the parser reads differently (the message names the record).  Nucleotide contexts with k <= 64 only.
        ``fold`` None: fold iff the context is canonical.  ``info``, if given, receives the mk_correct_fastq_t fields
        (those of mk_correct_t and mk_screen_t beside them)."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, held = _buf_ptr(path_or_bytes)
        nl = int(np.count_nonzero(held == 10)) if size else 0
        cap = (nl + 1) // 4 + 1  # (a record is four lines; a last line without '\n' is a line)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        fix = np.zeros((cap, len(CORRECT_COLUMNS)), dtype=np.uint32)
        out = np.empty(max(size, 1), dtype=np.uint8)
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), CorrectFastq()
        rule = CorrectFastqRule(int(at_least), quality_byte(new_qual), 0)
        self._check_correct_fastq(self._L.mk_correct_fastq_text(
            self._h, addr, size, int(piece_bytes), CORRECT_FOLD if self._fold_flag(fold) else 0, C.byref(rule), out.ctypes.data,
            size, C.byref(out_len), fix.ctypes.data, rows.ctypes.data, cap, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), fix[: n.value], rows[: n.value]

    def correct_fastq_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, fix_ptr: int = 0, rows_ptr: int = 0,
                             cap: int = 0, at_least: int = 2, new_qual=0, fold: Optional[bool] = None) -> dict:
        """mk_correct_fastq_device: ``nbytes`` of FASTQ text at device address ``ptr`` -> the corrected text (``nbytes``
        bytes) at device address ``out_ptr`` (room for ``out_cap``; ``out_ptr`` == ``ptr`` corrects in place, any other
        overlap is refused) and, where given, four uint32 a record at ``fix_ptr`` and the rows (five uint64 a record) at
        ``rows_ptr`` with room for ``cap`` records each -- all on this context's GPU, the last two aligned to 8.  Returns
        the mk_correct_fastq_t fields: "bytes_out" bytes were written, "records" rows."""
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), CorrectFastq()
        rule = CorrectFastqRule(int(at_least), quality_byte(new_qual), 0)
        self._check_correct_fastq(self._L.mk_correct_fastq_device(
            self._h, ptr, int(nbytes), CORRECT_FOLD if self._fold_flag(fold) else 0, C.byref(rule), out_ptr or None, int(out_cap),
            C.byref(out_len), fix_ptr or None, rows_ptr or None, int(cap), C.byref(n), C.byref(st)))
        return st.as_dict()

    # -- normalising: FASTA text in, the records thinned to a target depth out; the table is only read
    def _norm_flags(self, fold: Optional[bool], invert: bool) -> int:
        return (NORM_FOLD if self._fold_flag(fold) else 0) | (NORM_INVERT if invert else 0)

    def normalize(self, path_or_bytes, target: int, min_depth: int = 0, seed: int = 0, invert: bool = False,
                  fold: Optional[bool] = None, piece_bytes: int = 0, info: Optional[dict] = None):
        """mk_norm_text: (out, keep, median, rows) of the FASTA text (a path to a plain file, or the text itself as bytes).
        The depth of a record is the median of its k-mers' counts in the table (khmer's; uint32, clipped at 2^32 - 1:
        ``median``).  A record is kept iff it has k-mers, its depth is at least ``min_depth`` and either at most
        ``target`` or a draw that depends only on ``seed`` and the record's index falls below target / depth (BBNorm's
        plan: the table has been counted from all the reads beforehand).  ``out``: the kept records -- with ``invert``
        all the others -- in text order and byte for byte, as Counter.filter emits them; ``keep``: one bool per record,
        True where it was emitted; ``rows``: the (records, 5) uint64 array Counter.screen gives for the same text and
        at_least = max(min_depth, 1).  ``fold`` None: fold iff the context is canonical.  ``info``, if given, receives the
        mk_norm_t fields (those of mk_screen_t beside them)."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        addr, size, held = _buf_ptr(path_or_bytes)
        cap = (int(np.count_nonzero(held == ord(">"))) if size else 0) + 1  # (a record is a header line, or the text in front)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        keep = np.zeros(cap, dtype=np.uint8)
        med = np.zeros(cap, dtype=np.uint32)
        out = np.empty(max(size, 1), dtype=np.uint8)  # (the output is never longer than the text)
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Norm()
        rule = NormRule(int(target), int(min_depth), int(seed))
        self._check(self._L.mk_norm_text(self._h, addr, size, int(piece_bytes), self._norm_flags(fold, invert), C.byref(rule),
                                         out.ctypes.data, size, C.byref(out_len), med.ctypes.data, keep.ctypes.data,
                                         rows.ctypes.data, cap, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        return out[: out_len.value].tobytes(), keep[: n.value].astype(bool), med[: n.value], rows[: n.value]

    def normalize_device(self, ptr: int, nbytes: int, out_ptr: int, out_cap: int, target: int, median_ptr: int = 0, keep_ptr: int = 0,
                         rows_ptr: int = 0, cap: int = 0, min_depth: int = 0, seed: int = 0, invert: bool = False,
                         fold: Optional[bool] = None) -> dict:
        """mk_norm_device: ``nbytes`` of FASTA text (whole records) at device address ``ptr`` -> the emitted records at
        device address ``out_ptr`` (room for ``out_cap``; ``nbytes`` always suffice) and, where given, one uint32 median a
        record at ``median_ptr`` (aligned to 4), one keep byte a record at ``keep_ptr`` and the rows (five uint64 a record,
        aligned to 8) at ``rows_ptr`` with room for ``cap`` records each -- all on this context's GPU.  Returns the
        mk_norm_t fields: "bytes_out" bytes were written, "records" rows."""
        n, out_len, st = C.c_size_t(0), C.c_size_t(0), Norm()
        rule = NormRule(int(target), int(min_depth), int(seed))
        self._check(self._L.mk_norm_device(self._h, ptr, int(nbytes), self._norm_flags(fold, invert), C.byref(rule), out_ptr or None,
                                           int(out_cap), C.byref(out_len), median_ptr or None, keep_ptr or None, rows_ptr or None,
                                           int(cap), C.byref(n), C.byref(st)))
        return st.as_dict()

    # -- paired reads: interleaved FASTA text in, the pairs that pass out; the table is only read
    def _pairs_rule(self, op, at_least, min_hits, min_ppm, min_len, target, min_depth, seed) -> PairsRule:
        code = PAIRS_OPS.get(op, op) if isinstance(op, str) else op
        if isinstance(code, str):
            raise ValueError("op %r: one of %s" % (op, ", ".join(PAIRS_OPS)))
        if at_least is None:
            at_least = 2 if code == PAIRS_TRIM else 1
        return PairsRule(int(code), 0, FilterRule(int(at_least), int(min_hits), int(min_ppm), 0), TrimRule(int(at_least), int(min_len)),
                         NormRule(int(target), int(min_depth), int(seed)))

    def _pairs_flags(self, fold: Optional[bool], invert: bool, both: bool) -> int:
        return (PAIRS_FOLD if self._fold_flag(fold) else 0) | (PAIRS_INVERT if invert else 0) | (PAIRS_BOTH if both else 0)

    def pairs(self, path_or_bytes, op, at_least: Optional[int] = None, min_hits: int = 1, min_ppm: int = 0, min_len: int = 0,
              target: int = 1, min_depth: int = 0, seed: int = 0, both: bool = False, invert: bool = False, singles: bool = False,
              fold: Optional[bool] = None, piece_bytes: int = 0, info: Optional[dict] = None):
        """mk_pairs_text: (out, singles, keep, own, rows) of an INTERLEAVED FASTA text (a path to a plain file, or the text
        itself as bytes): records 2p and 2p + 1 are the mates of pair p, by position.  ``op`` "filter", "trim" or "norm"
        (or PAIRS_FILTER / PAIRS_TRIM / PAIRS_NORM) with that call's own arguments (``at_least`` None: 1, for trim 2).
        Every mate gets the unpaired call's result -- ``rows``, and ``own``: None for filter, ``kept`` (uint64) for trim,
        ``median`` (uint32) for norm -- and the pair passes as a whole: filter iff either mate matches (``both``: both),
        trim iff both mates keep something, norm iff the shallowest eligible mate passes the depth rule with the draw of
        the first mate's index.  ``out``: both mates of every passing pair (``invert``: of every other pair), each as the
        unpaired call emits it.  ``singles``: with ``singles`` the bytes of the orphans -- records that pass on their own
        in a pair that does not -- else None.  ``keep``: uint8 a record, 0 not emitted, 1 in out, 2 an orphan.  An odd
        number of records is MercatHipError (MK_ERR_RANGE).  ``info``, if given, receives the mk_pairs_t fields."""
        if isinstance(path_or_bytes, (str, os.PathLike)):
            with open(path_or_bytes, "rb") as fh:
                path_or_bytes = fh.read()
        rule = self._pairs_rule(op, at_least, min_hits, min_ppm, min_len, target, min_depth, seed)
        addr, size, held = _buf_ptr(path_or_bytes)
        cap = (int(np.count_nonzero(held == ord(">"))) if size else 0) + 1  # (a record is a header line, or the text in front)
        rows = np.zeros((cap, len(SCREEN_COLUMNS)), dtype=np.uint64)
        keep = np.zeros(cap, dtype=np.uint8)
        kept = np.zeros(cap, dtype=np.uint64) if rule.op == PAIRS_TRIM else None
        med = np.zeros(cap, dtype=np.uint32) if rule.op == PAIRS_NORM else None
        out = np.empty(size + 1, dtype=np.uint8)  # (the output is at most one newline longer than the text)
        sg = np.empty(size + 1, dtype=np.uint8) if singles else None
        n, out_len, sg_len, st = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), Pairs()
        self._check(self._L.mk_pairs_text(self._h, addr, size, int(piece_bytes), self._pairs_flags(fold, invert, both), C.byref(rule),
                                          out.ctypes.data, size + 1, C.byref(out_len), sg.ctypes.data if singles else None,
                                          size + 1 if singles else 0, C.byref(sg_len), keep.ctypes.data,
                                          kept.ctypes.data if kept is not None else None, med.ctypes.data if med is not None else None,
                                          rows.ctypes.data, cap, C.byref(n), C.byref(st)))
        if info is not None:
            info.update(st.as_dict())
        own = kept[: n.value] if kept is not None else med[: n.value] if med is not None else None
        return (out[: out_len.value].tobytes(), sg[: sg_len.value].tobytes() if singles else None, keep[: n.value], own,
                rows[: n.value])

    def pairs_device(self, ptr: int, nbytes: int, op, out_ptr: int, out_cap: int, singles_ptr: int = 0, singles_cap: int = 0,
                     keep_ptr: int = 0, kept_ptr: int = 0, median_ptr: int = 0, rows_ptr: int = 0, cap: int = 0,
                     at_least: Optional[int] = None, min_hits: int = 1, min_ppm: int = 0, min_len: int = 0, target: int = 1,
                     min_depth: int = 0, seed: int = 0, both: bool = False, invert: bool = False, fold: Optional[bool] = None) -> dict:
        """mk_pairs_device: ``nbytes`` of interleaved FASTA text (whole pairs) at device address ``ptr`` -> the passing
        pairs at ``out_ptr`` (room for ``out_cap``; ``nbytes`` + 1 always suffice), the orphans at ``singles_ptr`` where
        given, and, where given, one keep byte, one uint64 of kept characters (trim), one uint32 median (norm) and the
        rows (five uint64) a record with room for ``cap`` records each -- all on this context's GPU, kept and rows
        aligned to 8, median to 4.  Returns the mk_pairs_t fields."""
        rule = self._pairs_rule(op, at_least, min_hits, min_ppm, min_len, target, min_depth, seed)
        n, out_len, sg_len, st = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), Pairs()
        self._check(self._L.mk_pairs_device(self._h, ptr, int(nbytes), self._pairs_flags(fold, invert, both), C.byref(rule),
                                            out_ptr or None, int(out_cap), C.byref(out_len), singles_ptr or None, int(singles_cap),
                                            C.byref(sg_len), keep_ptr or None, kept_ptr or None, median_ptr or None, rows_ptr or None,
                                            int(cap), C.byref(n), C.byref(st)))
        return st.as_dict()

    def filter_pairs(self, path_or_bytes, at_least: int = 1, min_hits: int = 1, min_ppm: int = 0, both: bool = False,
                     invert: bool = False, singles: bool = False, fold: Optional[bool] = None, piece_bytes: int = 0,
                     info: Optional[dict] = None):
        """Counter.filter with the pair as the unit: Counter.pairs(op="filter")."""
        return self.pairs(path_or_bytes, PAIRS_FILTER, at_least=at_least, min_hits=min_hits, min_ppm=min_ppm, both=both, invert=invert,
                          singles=singles, fold=fold, piece_bytes=piece_bytes, info=info)

    def trim_pairs(self, path_or_bytes, at_least: int = 2, min_len: int = 0, singles: bool = False, fold: Optional[bool] = None,
                   piece_bytes: int = 0, info: Optional[dict] = None):
        """Counter.trim with the pair as the unit: Counter.pairs(op="trim")."""
        return self.pairs(path_or_bytes, PAIRS_TRIM, at_least=at_least, min_len=min_len, singles=singles, fold=fold,
                          piece_bytes=piece_bytes, info=info)

    def normalize_pairs(self, path_or_bytes, target: int, min_depth: int = 0, seed: int = 0, invert: bool = False,
                        fold: Optional[bool] = None, piece_bytes: int = 0, info: Optional[dict] = None):
        """Counter.normalize with the pair as the unit: Counter.pairs(op="norm")."""
        return self.pairs(path_or_bytes, PAIRS_NORM, target=target, min_depth=min_depth, seed=seed, invert=invert, fold=fold,
                          piece_bytes=piece_bytes, info=info)

    # -- results
    def rows(self) -> int:
        n = C.c_size_t(0)
        self._check(self._L.mk_export_size(self._h, C.byref(n)))
        return n.value

    def export(self) -> Tuple[np.ndarray, np.ndarray]:
        """(kmers as a (rows, k) uint8 array, counts uint64) in sorted order."""
        rows = self.rows()
        kmers = np.empty((rows, self.k), dtype=np.uint8)
        counts = np.empty(rows, dtype=np.uint64)
        self._check(self._L.mk_export(self._h, kmers.ctypes.data, counts.ctypes.data, rows))
        return kmers, counts

    def to_dict(self) -> dict:
        kmers, counts = self.export()
        if kmers.shape[0] == 0:
            return {}
        flat = kmers.tobytes().decode("ascii")
        k = self.k
        return dict(zip((flat[i:i + k] for i in range(0, len(flat), k)), counts.tolist()))

    def write_tsv(self, path, basename: str) -> int:
        n = C.c_size_t(0)
        self._check(self._L.mk_write_tsv(self._h, os.fsencode(str(path)), basename.encode(), C.byref(n)))
        return n.value

    def export_stats(self) -> dict:
        """Where the last export / write_tsv of this context spent its time (mk_export_stats)."""
        st = ExportStats()
        self._check(self._L.mk_export_stats(self._h, C.byref(st)))
        return st.as_dict()

    # -- multi-GPU plumbing (device pointers come from torch tensors)
    def export_pairs_device(self, keys_ptr: int, counts_ptr: int, cap: int) -> int:
        n = C.c_size_t(0)
        self._check(self._L.mk_export_pairs_device(self._h, keys_ptr, counts_ptr, cap, C.byref(n)))
        return n.value

    def import_pairs_device(self, keys_ptr: int, counts_ptr: int, rows: int):
        self._check(self._L.mk_import_pairs_device(self._h, keys_ptr, counts_ptr, rows))

    def bucket_rows_device(self, bounds: Sequence[int], rows_ptr: int, cap_rows: int) -> list:
        """mk_bucket_rows_device: the table's rows grouped by owner (len(bounds)+1 owners) as interleaved
        {key word(s), count} rows in the device buffer at rows_ptr; returns the rows per owner."""
        n = len(bounds) + 1
        b = np.array(list(bounds) + [0], dtype=np.uint64)
        counts = np.zeros(n, dtype=np.uint64)
        self._check(self._L.mk_bucket_rows_device(self._h, b.ctypes.data, n, rows_ptr, int(cap_rows), counts.ctypes.data))
        return [int(x) for x in counts]

    def sample_keys(self, stride: int, cap: int = 1 << 16) -> np.ndarray:
        """About one in ``stride`` rows: the first word of their keys (mk_sample_keys), uint64, in no order."""
        out = np.empty(cap, dtype=np.uint64)
        n = C.c_size_t(0)
        self._check(self._L.mk_sample_keys(self._h, int(max(1, stride)), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].copy()

    def dense_bins_device(self, bins_ptr: int, nbins: int, store: bool):
        """Dense mode: copy the bins out to / in from a device buffer (mk_dense_bins_device)."""
        self._check(self._L.mk_dense_bins_device(self._h, bins_ptr, int(nbins), 1 if store else 0))

    def import_rows_device(self, rows_ptr: int, rows: int):
        self._check(self._L.mk_import_rows_device(self._h, rows_ptr, int(rows)))

    def words_per_key(self) -> int:
        """64-bit words per packed key in export_pairs_device / import_pairs_device (mk_words_per_key)."""
        return int(self._L.mk_words_per_key(self._h))

    def alpha_stats(self) -> dict:
        """Moments of the count column, reduced on the GPU (mk_alpha_stats)."""
        a = AlphaStats()
        self._check(self._L.mk_alpha_stats(self._h, C.byref(a)))
        return {"observed": int(a.observed), "total": int(a.total), "freq": [int(x) for x in a.freq],
                "sum_sq": float(a.sum_sq), "sum_clnc": float(a.sum_clnc)}

    def filter_min(self, min_count: int):
        """Drop rows whose count is below ``min_count`` (the filter of a one-chunk sample counted in pieces)."""
        self._check(self._L.mk_filter_min(self._h, int(min_count)))

    def merge_from(self, other: "Counter"):
        """Add every row of ``other`` (same GPU, alphabet, k) into this context, on the device."""
        self._check(self._L.mk_merge_from(self._h, other._h))

    def combine(self, other: "Counter", op, min_self: int = 1, min_other: int = 1, into: Optional["Counter"] = None,
                info: Optional[dict] = None) -> "Counter":
        """mk_table_op: this table and ``other``'s combined by key on the GPU.  For every key of either, with ca / cb its
        count here / there (0 where absent, and where below ``min_self`` / ``min_other``), the result holds f(ca, cb)
        where that is not 0: ``op`` "min" (keys in both, the smaller count), "max", "sum", "left" (this table's rows
        whose key ``other`` holds), "only" (those it lacks), "diff" (ca - cb where positive) -- a name of OPS or its
        code.  Keys are compared as they stand.  Both inputs are only read (``other`` may be ``self``).  Returns
        ``into`` -- a third context of the same k, alphabet, device and canonical mode, emptied first -- or a new
        Counter of that kind, which the caller closes.  ``info``, if given, receives the mk_table_op_t fields."""
        if isinstance(op, str):
            if op not in OPS:
                raise ValueError("combine: op must be one of %s" % ", ".join(OPS))
            op = OPS[op]
        dst = into if into is not None else Counter(self.k, self.alphabet, self.device, canonical=self.canonical)
        st = TableOp()
        rc = self._L.mk_table_op(dst._h, self._h, other._h, int(op), int(min_self), int(min_other), C.byref(st))
        if rc:
            try:
                dst._check(rc)
            finally:
                if into is None:
                    dst.close()
        if info is not None:
            info.update(st.as_dict())
        return dst

    def share_table(self, owner: Optional["Counter"]):
        """From now on this context's count kernels put the survivors of its chunks into ``owner``'s running table (same
        GPU, alphabet, k; mk_share_table); ``None``: back to its own.  Sum with ``owner.merge_from(self)`` as before."""
        self._check(self._L.mk_share_table(self._h, owner._h if owner is not None else None))

    def export_exotic(self) -> Tuple[np.ndarray, np.ndarray]:
        n = C.c_size_t(0)
        self._check(self._L.mk_export_exotic(self._h, None, None, 0, C.byref(n)))
        kmers = np.empty((n.value, self.k), dtype=np.uint8)
        counts = np.empty(n.value, dtype=np.uint64)
        if n.value:
            self._check(self._L.mk_export_exotic(self._h, kmers.ctypes.data, counts.ctypes.data, n.value, C.byref(n)))
        return kmers, counts

    def import_exotic(self, kmers: np.ndarray, counts: np.ndarray):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint8)
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size:
            self._check(self._L.mk_import_exotic(self._h, kmers.ctypes.data, counts.ctypes.data, counts.size))

    # -- stats
    def set_profiling(self, on: bool):
        self._check(self._L.mk_set_profiling(self._h, 1 if on else 0))

    def stats(self) -> dict:
        s = Stats()
        self._check(self._L.mk_get_stats(self._h, C.byref(s)))
        d = s.as_dict()
        d["mode_name"] = MODE_NAMES.get(d["mode"], "?")
        return d

    def reset_stats(self):
        self._check(self._L.mk_reset_stats(self._h))
