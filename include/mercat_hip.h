/* mercat_hip.h -- C ABI of libmercat_hip.so: the MI355X (gfx950) k-mer counting engine that
 * stands in for MerCat2's counting path.
 *
 * Drop-in boundary (reference file:line, relative to the reference checkout):
 *   find_kmers(file, kmer, min_count) -> {kmer: count}      lib/mercat2_kmers.py:32-78
 *   run_mercat2(basename, files, out_file, kmer, min_count) bin/mercat2.py:115-137
 *   chunk_files / Chunker.stream_delim                      bin/mercat2.py:86-106, lib/mercat2_Chunker.py:39-59
 * The Python host layer (mercat2_amd/) mirrors those three callables on top of this ABI with
 * ctypes; INTEGRATION.md shows the stub a MerCat2 maintainer would add.
 *
 * Conventions: every function returns an int status (MK_OK == 0, negative = error); the text
 * of the last error of a context is mk_last_error(ctx).  The caller owns every buffer it
 * passes in or receives into; a context owns its device memory and its HIP stream.  A context
 * is not thread-safe; different contexts may be used from different host threads.  There is
 * no CPU fallback anywhere behind this ABI: without a usable HIP device mk_create fails.
 */
#ifndef MERCAT_HIP_H
#define MERCAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MK_OK 0
#define MK_ERR_ARG (-1)       /* bad argument (k < 1, unknown alphabet, null pointer, ...) */
#define MK_ERR_HIP (-2)       /* a HIP runtime call failed (message has the call and hipError) */
#define MK_ERR_NOMEM (-3)     /* device or host allocation failed */
#define MK_ERR_STATE (-4)     /* call sequence error (feed outside begin/end, ...) */
#define MK_ERR_NON_ASCII (-5) /* a SEQUENCE line holds bytes >= 0x80: the reference would decode them as
                                 multi-byte characters; refused rather than counted wrongly.  Header lines
                                 may hold any bytes: they never enter a k-mer */
#define MK_ERR_IO (-6)        /* file could not be written */
#define MK_ERR_RANGE (-7)     /* caller buffer too small / value out of range */
#define MK_ERR_UNSUPPORTED (-8) /* clean mode (mk_set_clean): the chunk holds text whose rewrite by removeN the GPU does not
                                 reproduce (a blank inside a sequence line, a '>' that does not start a header line, a
                                 0x7F byte); nothing of the chunk was counted -- count the text mk_remove_n produces instead.
                                 mk_fastq_select_* / mk_fastq_qtrim_* / mk_fq_interleave / mk_fq_split_pairs: a FASTQ record is malformed (its
                                 first line lacks the '@', its third the '+', its sequence and quality lines differ in
                                 length, its sequence line holds a blank or '*' while kept[] is given, or the text ends
                                 inside it); the message names the record and the check, nothing was written.
                                 mk_correct_fastq_*: the same, and a sequence line the parser reads differently */

/* Alphabets select the packed fast path; they never restrict the input.  Windows holding a
 * symbol outside the alphabet are still counted, exactly, by the by-reference kernel
 * (the reference counts "any character": lib/mercat2_kmers.py:56-60). */
#define MK_ALPHABET_NT2 0 /* A C G T -> 2-bit codes 0..3 (ASCII order)            */
#define MK_ALPHABET_AA5 1 /* 'A'..'Z' -> 5-bit codes 0..25 (ASCII order)          */
#define MK_ALPHABET_RAW 2 /* no packing: every window by reference (any k, any text) */

typedef struct mk_ctx mk_ctx;

/* Counters of one context, cumulative since mk_create / mk_reset_stats. */
typedef struct mk_stats_t {
  uint64_t raw_bytes;      /* FASTA bytes fed                                               */
  uint64_t symbols;        /* sequence characters kept by the parser (the "bases")          */
  uint64_t windows;        /* length-k windows counted (all paths)                          */
  uint64_t exotic_windows; /* of those, windows no packed kernel takes: counted byte-wise    */
  uint64_t chunks;         /* chunks ended                                                  */
  uint64_t survivors;      /* chunk-table entries that passed their chunk's min_count       */
  uint64_t rows;           /* distinct k-mers now in the running (merged) table             */
  uint64_t table_slots;    /* slots (or dense bins) of the chunk table of the last chunk    */
  int32_t mode;            /* 0 dense-LDS, 1 hash64 (one-word packed keys), 2 hash128 (nucleotide 33..64-mers:
                              two-word packed keys), 3 by-reference on bytes only                 */
  int32_t profiled;        /* 1 when per-kernel HIP-event timing is on (mk_set_profiling)   */
  /* HIP-event time per kernel family, milliseconds, and launches (only when profiled) */
  double ms_parse, ms_pack, ms_count, ms_exotic, ms_filter, ms_export;
  uint64_t n_parse, n_pack, n_count, n_exotic, n_filter, n_export;
  /* partition stage (bucket histogram + scan + scatter) that feeds the LDS count kernel;
   * ms_count / n_count are the count kernel alone */
  double ms_part;
  uint64_t n_part;
  uint64_t records;  /* super-k-mer records written (0 on other paths) */
  uint64_t distinct; /* distinct packed keys seen per chunk, summed over chunks */
  uint64_t part_retries; /* chunks partitioned twice: the sampled bucket sizes were too small somewhere */
  uint64_t part_reused;  /* chunks that inherited the bucket regions of the chunk before them (no histogram, no scan) */
  uint64_t fused_chunks; /* chunks whose count kernel put the survivors into the running table itself (ABI 4)        */
  uint64_t fuse_spilled; /* ... survivors of those it set aside instead (table filling up), imported afterwards        */
  uint64_t parse_retries; /* chunks parsed a second time by the general parser (a blank inside a sequence line)           */
  uint64_t split_exhausted; /* sub-ranges of the LDS count kernels that reached the last split level (every hash bit used):
                               counted by probing the whole table (ABI 5)                                                     */
  uint64_t flat_chunks;  /* chunks counted through the flat parse lane (read files: packed in place, one kernel)              */
  uint64_t flat_refused; /* flat launches refused (the text is not one line per record): parsed again by the fast parser     */
} mk_stats_t;

/* ---- lifetime ------------------------------------------------------------------------- */
/* One context per GPU and per (alphabet, k).  Replaces the per-task state of
 * countKmers/find_kmers (bin/mercat2.py:112-114). */
int mk_create(int device, int alphabet, int k, mk_ctx** out);
/* HIP devices this process sees (0 when there is none or the runtime cannot start): the GPUs a host may spread a
 * sample's chunks over, or give one small sample each (bin/mercat2.py:217 sizes its Ray pool by -n the same way). */
int mk_device_count(void);
void mk_destroy(mk_ctx* ctx);
const char* mk_last_error(const mk_ctx* ctx);
/* Forget the running (merged) table: start the next sample (run_mercat2's `kmers = dict()`,
 * bin/mercat2.py:117). */
int mk_reset(mk_ctx* ctx);
/* mk_reset that also sizes the (emptied) packed table for about expect_rows distinct keys when that is less than its
 * present size: what an owner does between handing its rows out and taking in the rows of its own key range
 * (1/N of the table: a table that fits the caches takes the imports several times faster). */
int mk_reset_for(mk_ctx* ctx, uint64_t expect_rows);
/* Opt-in extension, NOT reference behaviour (the reference counts forward-strand substrings,
 * lib/mercat2_kmers.py:56-60): with on != 0 every ACGT-only window is counted under
 * min(kmer, reverse-complement(kmer)).  Windows holding other characters keep their own text.
 * Nucleotide alphabet only; call before the first chunk of a sample (or right after mk_reset).
 * Nucleotide k <= 64.  One-word keys (k <= 32) file a window under min(11-mer, its reverse complement) of its
 * minimizer; two-word keys (33 <= k <= 64) under the smallest canonical 11-mer among the candidates of the window's
 * first and last 32 bases -- the set the two strands share.  k > 64 and the raw alphabet count text, which has no
 * complement: MK_ERR_ARG. */
int mk_set_canonical(mk_ctx* ctx, int on);

/* removeN's effect on the count, on the GPU (lib/mercat2_fasta.py:53-119; MerCat2 runs it on every nucleotide FASTA
 * before counting, bin/mercat2.py:239-244): with on != 0 the chunks fed from now on are RAW FASTA and are counted as
 * if removeN had rewritten them first -- every run of upper-case 'N' cuts its record (no window spans or holds it),
 * text in front of the first header line is not counted, and with toupper != 0 lower-case letters count as their
 * upper-case forms (a lower-case 'n' then is an 'N' that IS counted, as in the reference, which splits before it
 * upper-cases).  The N scan shares the parser's and packer's pass over the text; the table does not wait for the
 * rewritten file.  Nucleotide alphabet, one chunk per file (a sample the reference would chunk is cut on the CLEANED
 * text: count mk_remove_n's output for those).  A chunk the mode cannot reproduce is refused with MK_ERR_UNSUPPORTED
 * and nothing of it is counted. */
int mk_set_clean(mk_ctx* ctx, int on, int toupper);
typedef struct mk_clean_gpu_t {
  uint64_t raw_bytes;    /* bytes of the chunks counted in clean mode since mk_reset                              */
  uint64_t symbols;      /* sequence characters kept (N runs excluded): the total_length removeN divides by,
                            without the header lines of split records                                            */
  uint64_t gc_count;     /* 'G' + 'C' among them AFTER -toupper if it is on, header lines of split records not
                            included: NOT the reference's "GC Content" figure, which counts before upper-casing and
                            includes those header lines (lib/mercat2_fasta.py:92-113; mk_remove_n reports that one) */
  uint64_t n_bytes;      /* upper-case 'N' bytes removed                                                         */
  uint64_t n_runs;       /* runs of N = cuts = pieces added                                                      */
  uint64_t header_lines; /* records                                                                             */
  uint64_t last_runs;    /* runs of the last chunk (mk_clean_runs lists them)                                    */
} mk_clean_gpu_t;
int mk_clean_stats(mk_ctx* ctx, mk_clean_gpu_t* out);
/* The N runs of the last chunk as [starts[i], ends[i]) in the parsed stream (kept characters in order, one separator
 * per header line: the stream the k-mer windows slide over), ascending; *n = how many (cap values fit).  A chunk with
 * more than 65536 runs is not listed: MK_ERR_RANGE, *n = 0 (mk_clean_stats still counts them).  What split_sequenceN
 * cuts at (lib/mercat2_fasta.py:35-38). */
int mk_clean_runs(mk_ctx* ctx, uint64_t* starts, uint64_t* ends, size_t cap, size_t* n);

/* FASTQ input as MerCat2 counts it with -skipclean (fq2fa, lib/mercat2_fasta.py:175-198: `sed -n '1~4s/^@/>/p;2~4p'`
 * read back in universal-newline text mode, written to <base>.fna.gz).  Lines are split on '\n' only and numbered
 * across the text: line 4i+1 is kept, its '@' made a '>', when it starts with '@' and dropped otherwise; line 4i+2 is
 * kept as it stands; lines 4i+3 and 4i+4 are dropped; the text read back turns '\r\n' and a lone '\r' into '\n'. */
typedef struct mk_fastq_stats_t {
  uint64_t lines;           /* lines of the FASTQ text (a last line without '\n' is one)                 */
  uint64_t reads;           /* lines 4i+1 kept (header lines of the converted text)                     */
  uint64_t headers_dropped; /* lines 4i+1 that do not start with '@'                                    */
  uint64_t fasta_bytes;     /* size of the converted text                                               */
  uint64_t crlf;            /* '\r\n' pairs of kept lines, each one '\n' in the converted text           */
} mk_fastq_stats_t;
/* With on != 0 every chunk fed from now on (mk_chunk_feed / mk_chunk_feed_device) is raw FASTQ text, a file of its own
 * that starts at line 1, and is counted exactly as find_kmers counts the text fq2fa makes of it.  The chunk is rewritten
 * in place before the parser (dropped lines become line ends, the kept '@' a '>'), so text already on the device is
 * refused by mk_count_device (MK_ERR_STATE), and so is mk_count_file.  Nucleotide alphabet only; not together with clean
 * mode (MK_ERR_ARG).  mk_reset keeps the mode and zeroes the stats. */
int mk_set_fastq(mk_ctx* ctx, int on);
/* The conversion's figures summed over the chunks counted in FASTQ mode since mk_reset (mk_fq2fa's for the same text). */
int mk_fastq_stats(mk_ctx* ctx, mk_fastq_stats_t* out);

/* ---- one chunk = one find_kmers call (lib/mercat2_kmers.py:32-78) ------------------------ */
int mk_chunk_begin(mk_ctx* ctx);
/* Append raw FASTA bytes (host memory) of the current chunk; may be called repeatedly, the
 * pieces are concatenated.  The buffer may be reused on return. */
int mk_chunk_feed(mk_ctx* ctx, const uint8_t* text, size_t n);
/* Same, from device memory of this context's GPU (used when the text is already in HBM). */
int mk_chunk_feed_device(mk_ctx* ctx, const uint8_t* d_text, size_t n);
/* Parse + pack + count the chunk, keep entries with count >= min_count
 * (lib/mercat2_kmers.py:73-76) and add them into the running table
 * (the dict sum of bin/mercat2.py:121-127). */
int mk_chunk_end(mk_ctx* ctx, uint64_t min_count);
/* Count a chunk in place from device memory without the staging copy (begin+feed+end).
 * d_text must stay valid until the call returns. */
int mk_count_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, uint64_t min_count);

/* ---- one file of a sample, from disk: chunk_files + a countKmers task per chunk + the dict sum
 *      (bin/mercat2.py:86-106, 112-127), with the file reading of find_kmers
 *      (lib/mercat2_kmers.py:47-50) and no chunk files ------------------------------------ */
typedef struct mk_file_stats_t {
  uint64_t disk_bytes; /* size of the file on disk                                           */
  uint64_t text_bytes; /* (inflated) bytes read and fed                                      */
  uint64_t chunks;     /* chunks counted (1 when the file was not chunked)                   */
  int32_t gz;          /* 1: the file was inflated (last suffix ".gz")                        */
  int32_t chunked;     /* 1: disk_bytes >= chunk_bytes, the Chunker rule was applied         */
  int32_t members;     /* gzip members seen                                                  */
  int32_t threads;     /* reader threads used                                                */
  int32_t contexts;    /* contexts that counted chunks                                       */
  int32_t devices;     /* GPUs those contexts are on                                         */
  int32_t split_pieces;/* > 0: the file was one filter unit counted in that many pieces on several GPUs, filtered after the sum */
  int32_t pad_;
  double s_wait_io;    /* seconds the dispatching thread waited for file blocks              */
  double s_wait_gpu;   /* seconds it waited for a context to finish its previous chunk       */
  double s_total;      /* wall seconds of the call                                           */
  double s_merge;      /* of those, the sum of the contexts' tables at the end                */
  /* (ABI 4) where the dispatching thread's time went; s_setup + s_wait_io + s_wait_gpu + s_scan + s_feed + s_retire +
   * s_drain + s_merge ~= s_total */
  double s_setup;      /* open, ring (pinned memory), worker and reader threads started       */
  double s_scan;       /* the Chunker rule applied to the blocks                              */
  double s_feed;       /* inside the host-to-device copy calls                                */
  double s_retire;     /* waiting for copies out of ring blocks the readers want back         */
  double s_drain;      /* after the last block: copies, readers and the last chunks' counting */
} mk_file_stats_t;
/* Reads `path` (gzip iff its name ends in ".gz", as the reference decides), splits it as
 * Chunker(path, dest, chunk_bytes, '>') would iff its on-disk size is >= chunk_bytes > 0
 * (chunk_bytes == 0: never), counts every chunk with its own min_count filter and adds the
 * survivors to the running table of ctxs[0].  With nctx > 1 (same alphabet, k, canonical mode; on one
 * GPU or on several: mk_plan_contexts gives the order) chunk i goes to ctxs[i mod nctx] and is counted
 * there, filtered on its own, concurrently with the reading; at the end the contexts of one GPU are summed
 * on that GPU, the GPUs' tables are summed into ctxs[0] (mk_merge_devices, MK_MERGE_GATHER) and the other
 * contexts are reset.  A file that is NOT chunked (one filter unit, lib/mercat2_kmers.py:73-76) but large
 * (>= 64 MiB of text) is, with contexts on several GPUs, cut into one piece per context at record starts
 * (mk_record_cuts), the pieces are counted unfiltered, summed, and min_count is applied to the sum
 * (single-chunk sample).  st->split_pieces says so.  threads = reader
 * threads (<= 0: pick): plain files are read, BGZF blocks and -- from 16 MiB on -- ordinary gzip
 * streams are decoded by that many threads; 1 decodes a gzip stream front to back.  st may be NULL. */
int mk_count_file(mk_ctx* const* ctxs, int nctx, const char* path, uint64_t chunk_bytes, uint64_t min_count,
                  int threads, mk_file_stats_t* st);

/* ---- result of the sample: sorted(kmers.items()) (bin/mercat2.py:130-133) --------------- */
int mk_export_size(mk_ctx* ctx, size_t* rows);
/* kmers: rows*k ASCII bytes (no terminators), counts: rows values; both caller-allocated.
 * Rows are in Python sorted(str) order == byte-wise order. */
int mk_export(mk_ctx* ctx, uint8_t* kmers, uint64_t* counts, size_t rows_cap);
/* Writes "k-mer\t{basename}_Count\n" + rows; writes NO file and sets *rows = 0 when the
 * table is empty (bin/mercat2.py:128-137). */
int mk_write_tsv(mk_ctx* ctx, const char* path, const char* basename, size_t* rows);

/* Where the last mk_export / mk_write_tsv of this context spent its time (the sorted() + print loop of
 * bin/mercat2.py:130-133 is as expensive as the counting for the reference: 17 s + 13 s at 7.7 M rows). */
typedef struct mk_export_stats_t {
  uint64_t rows;     /* rows exported (packed + kept as text)                                         */
  uint64_t bytes;    /* bytes of TSV text written (0 for mk_export)                                   */
  double s_sort;     /* device: compaction of the table + radix sort of the packed keys, waited for   */
  double s_d2h;      /* sorted rows to the host (+ the rows kept as text, sorted on the device)         */
  double s_format;   /* host: keys decoded to text, counts to decimal, merged with the text rows       */
  double s_write;    /* host: inside write(2) (the file is written while it is formatted)               */
  double s_total;
} mk_export_stats_t;
int mk_export_stats(mk_ctx* ctx, mk_export_stats_t* out);

/* ---- a count table in text form back into the running table: the inverse of mk_write_tsv (ABI 6) ------------
 * The tsv_<type>/<sample>_counts.tsv files are what MerCat2 users keep; loaded, they feed every call below that works
 * from tables (mk_write_merged_tsv*, mk_gram, mk_pair_stats, mk_alpha_stats) without counting the reads again.
 * Lines end in '\n' (the last one may lack it).  A data row is exactly k key bytes (k of the context; any ASCII byte but
 * '\n': the reference counts any character, and a key it wrote may hold a '\t' -- with k known the row is still
 * unambiguous), '\t', 1..20 decimal digits whose value fits 64 bits.  Line 1 is a
 * header iff it is not a data row, so "k-mer\t<name>_Count" files and the header-less "kmer\tcount" dumps of Jellyfish
 * and KMC both load; column receives the header's second field ("" without a header; column may be NULL).  Rows need
 * not be sorted.  A byte >= 0x80 anywhere behind the header: MK_ERR_NON_ASCII.  Anything else malformed -- a key of
 * another length, no tab, an empty count, a non-digit, a count above 2^64 - 1, '\r', an empty line (bytes after the
 * last '\n' are a line; nothing after it is none) -- MK_ERR_RANGE; mk_last_error names the 1-based line.
 * The load is an insert-add: a key listed twice, or a second text loaded into the same context, adds up (counts wrap
 * at 2^64 like every sum of the tables).  Keys are taken AS THEY STAND: a canonical context (mk_set_canonical) does not
 * fold a loaded key onto its reverse complement -- a table written by a canonical context holds canonical keys already.
 * Rows with count 0 are skipped.  Keys inside the context's alphabet go to its packed table (dense bins, one- or
 * two-word keys; the 32 x 'T' key beside the one-word table), the others -- in a by-reference context all -- are kept as
 * text, exactly where counting puts them.
 * The text travels to the device in pieces of piece_bytes (0: pick; at least two rows, at most 1 GiB), cut at line
 * ends, through a pinned double buffer: memory is bounded whatever the file's size.  A piece is validated completely
 * before any of its rows is imported: a text that fits one piece and is refused leaves the context as it was.  A
 * refusal in a later piece leaves the pieces before in the table: the context then refuses every call with
 * MK_ERR_STATE until mk_reset, as after a refused chunk. */
typedef struct mk_tsv_load_t {
  uint64_t bytes, lines;      /* text consumed, lines seen (header included)              */
  uint64_t rows;              /* data rows parsed                                          */
  uint64_t packed_rows;       /* ... that went to the packed table (or dense bins)         */
  uint64_t text_rows;         /* ... kept as text (a byte outside the alphabet; by-reference contexts: all) */
  uint64_t zero_rows;         /* rows with count 0: skipped, never inserted                */
  uint64_t new_rows;          /* distinct keys the table gained                            */
  int32_t header;             /* 1: the first line was a header                            */
  int32_t pieces;             /* pieces the text was loaded in                             */
  /* seconds: host time reading (copying) the text into the pinned buffer; device time of the line-start and row
   * kernels; device time of table growth and the import kernels; wall time of the call */
  double s_read, s_parse, s_import, s_total;
} mk_tsv_load_t;
int mk_load_tsv(mk_ctx* ctx, const char* path, size_t piece_bytes, char* column, size_t column_cap, mk_tsv_load_t* st);
int mk_load_tsv_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, char* column, size_t column_cap,
                     mk_tsv_load_t* st);
/* Host helper, no GPU: what a table in text form looks like, for choosing the context to load it into.  *k = key
 * length of the first data row, up to the line's last tab (0: no data row), *header = 1 when line 1 is not a data row of any key length, column
 * = its second field, *alphabet_hint = MK_ALPHABET_NT2 when every key among the first 4096 rows is ACGT only, else
 * MK_ALPHABET_AA5 when they are 'A'..'Z' only, else MK_ALPHABET_RAW.  Only a hint: any table loads into any context of
 * its k, keys outside the alphabet are kept as text.  Errors: mk_last_error(NULL). */
int mk_tsv_shape(const char* path, int* k, int* header, int* alphabet_hint, char* column, size_t column_cap);

/* ---- keys in, counts out: how often does this k-mer, or this panel of marker k-mers, occur in the sample whose table
 *      the context holds (what Jellyfish calls `query`), answered on the GPU without exporting the table (ABI 6.1) ----
 * counts[i] is the count of key i in the running table, 0 when the table lacks it, in the order asked; a key asked
 * twice is answered twice.
 * The table is only READ: mk_export_size, the export and every later call give what they gave before the lookup.  The
 * call first makes the table final as mk_export_size does (pending row totals folded, read-backs landed) and drains
 * the context's stream; the caller must not count into the table meanwhile.  A sharer (mk_share_table) looks in its
 * OWN table.  A context that holds part of a refused chunk answers MK_ERR_STATE.
 * Where a key is probed is decided by the key alone, exactly as counting and mk_load_tsv place it: a key inside the
 * context's alphabet in the packed table (dense bins by index; the one-word table, with the 32 x 'T' key kept beside
 * it; the two-word tables of nucleotide 33..64-mers and protein 13..25-mers), any other key -- and every key of an
 * MK_ALPHABET_RAW context, or of one whose k is beyond the packed tables -- in the by-reference table.  An
 * in-alphabet key is never searched among the rows kept as text.
 * Key bytes may be any ASCII byte (in the text form: any but '\n'; a '\t' too); a byte >= 0x80 is MK_ERR_NON_ASCII.
 * MK_LOOKUP_FOLD: an ACGT-only key is looked up under min(key, reverse complement), the key a canonical context
 * (mk_set_canonical) files it under; keys holding other bytes are never folded.  Only for a canonical nucleotide context
 * with k <= 64, MK_ERR_ARG anywhere else.  Without the flag keys are taken as they stand, as mk_load_tsv takes them.
 * mk_lookup: rows * k key bytes in host memory; mk_lookup_device: keys and counts in DEVICE memory of the context's GPU.
 * mk_lookup_text / mk_lookup_file: a panel in text form (a plain file, not .gz).  Lines end in '\n' (the last may lack
 * it).  A row is exactly k key bytes, then the end of the line or '\t' and 1..20 decimal digits that fit 64 bits, which
 * are ignored: a counts TSV, or a Jellyfish / KMC dump, is a panel as it stands.  Line 1 is a header iff it is neither
 * form; it is skipped (st->header).  Anything else malformed -- a key of another length, '\r', an empty line, bytes
 * behind the key that are not a tab and digits -- is MK_ERR_RANGE, mk_last_error names the 1-based line.  counts[i]
 * belongs to data row i (the header not counted), *rows = data rows.  With cap too small: MK_ERR_RANGE, the needed size
 * in *rows, nothing written past cap.  The text travels in pieces of piece_bytes through a pinned double buffer, with
 * the defaults and limits of mk_load_tsv: memory is bounded whatever the panel's size. */
#define MK_LOOKUP_FOLD 1u   /* look an ACGT-only key up under min(key, reverse complement) */
typedef struct mk_lookup_t {
  uint64_t bytes, lines;     /* text consumed / lines seen (0 for the non-text calls)            */
  uint64_t keys;             /* keys looked up                                                    */
  uint64_t found;            /* ... with a count above zero                                       */
  uint64_t packed_keys;      /* ... that were probed in the packed table / dense bins             */
  uint64_t text_keys;        /* ... probed in the by-reference table (a byte outside the alphabet) */
  uint64_t folded;           /* keys replaced by their reverse complement (MK_LOOKUP_FOLD)        */
  int32_t header, pieces;
  /* seconds: host time moving the keys towards the device (the text form: filling the pinned halves); HIP-event time of
   * the kernels; wall time of the call */
  double s_read, s_probe, s_total;
} mk_lookup_t;
int mk_lookup(mk_ctx* ctx, const uint8_t* kmers, size_t rows, unsigned flags, uint64_t* counts, mk_lookup_t* st);
int mk_lookup_device(mk_ctx* ctx, const uint8_t* d_kmers, size_t rows, unsigned flags, uint64_t* d_counts, mk_lookup_t* st);
int mk_lookup_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, uint64_t* counts,
                   size_t cap, size_t* rows, mk_lookup_t* st);
int mk_lookup_file(mk_ctx* ctx, const char* path, size_t piece_bytes, unsigned flags, uint64_t* counts, size_t cap,
                   size_t* rows, mk_lookup_t* st);

/* ---- the abundance spectrum of a table: how many distinct k-mers occur once, twice, ... (what Jellyfish calls `histo`,
 *      KMC its histogram), reduced on the GPU in one pass over the table, without exporting it ----
 * bins has high + 2 words: bins[c] = rows whose count is c, for 1 <= c <= high; bins[high + 1] = rows whose count is
 * above high (Jellyfish's rule for -h); bins[0] stays 0, so that bins[i] is abundance i.  1 <= high <= 2^20, MK_ERR_ARG
 * otherwise.  A row is a key whose count is not zero: a dense bin never hit, or a keyed slot that counts 0, is none.
 * Counts are 64-bit and every step is an integer add: the answer is exact whatever the order (a count of 2^64 - 1 lands
 * in the overflow bin); total and over_total are sums modulo 2^64, as mk_alpha_stats' total is.
 * The contract is that of mk_lookup: the table is only READ and a repeated call gives the same answer; the call first
 * makes the table final (pending row totals folded) and works on the context's stream, which is idle when it returns;
 * a context that holds part of a refused chunk, or an open chunk, answers MK_ERR_STATE; an empty table gives all-zero
 * bins and MK_OK.  A sharer (mk_share_table) answers as it does for mk_alpha_stats and mk_lookup: for its OWN tables,
 * not the owner's -- the rows its chunks put into the owner's table are in the owner's histogram.
 * mk_histo: bins in host memory; mk_histo_device: bins in DEVICE memory of the context's GPU.  st may be NULL. */
typedef struct mk_histo_t {
  uint64_t distinct;    /* rows: the sum of the bins                                            */
  uint64_t total;       /* sum of the counts                                                    */
  uint64_t max_count;   /* the largest count (0: no rows)                                       */
  uint64_t over_rows;   /* rows whose count is above high: bins[high + 1]                       */
  uint64_t over_total;  /* sum of their counts                                                  */
  uint64_t slots;       /* table slots (dense bins) read                                        */
  double s_scan, s_total; /* seconds: HIP-event time of the kernel(s); wall time of the call   */
} mk_histo_t;
int mk_histo(mk_ctx* ctx, uint64_t high, uint64_t* bins, mk_histo_t* st);
int mk_histo_device(mk_ctx* ctx, uint64_t high, uint64_t* d_bins, mk_histo_t* st);

/* ---- sequences in, per-record k-mer hits and abundance out: how many of this read's k-mers are in the table, and how
 *      abundant are they (Jellyfish `query -s`, BBDuk-style screening, abundance filtering), answered on the GPU from
 *      the text itself: one byte per base travels, not k ----
 * The text is FASTA and is read exactly as counting reads it (the general parser: strip(), universal newlines, '*'
 * removed, wrapped lines joined, any ASCII character kept); a byte >= 0x80 in a sequence line is MK_ERR_NON_ASCII, header
 * lines may hold any bytes.  Clean mode and FASTQ mode of the context do NOT apply: they rewrite chunks on their way into
 * the count and this call never enters that path -- the text is read as FASTA as it stands (convert FASTQ with mk_fq2fa).
 * Records are the stretches of kept characters between header lines: one row per header line, in text order, a header
 * without sequence included (windows = 0); one leading row when kept characters stand in front of the first header
 * (st->headless = 1).  *nrows = records.  With cap too small: MK_ERR_RANGE, the needed size in *nrows, nothing written
 * past cap.
 * A record of L kept characters has max(0, L - k + 1) windows; no window spans two records.  Each window is probed where
 * mk_lookup would probe the same k bytes: inside the alphabet in the packed table (dense bins, the one-word table with
 * the 32 x 'T' key beside it, the two-word tables), any other window -- every window of an MK_ALPHABET_RAW context or of
 * a k beyond the packed tables -- in the by-reference table.  MK_SCREEN_FOLD has the meaning and the restriction of
 * MK_LOOKUP_FOLD.  at_least >= 1 (0: MK_ERR_ARG).  All sums are integer adds: the rows are exact whatever the order.
 * The table is only READ, under mk_lookup's rules: it is made final first, an open chunk or a context that holds part of
 * a refused chunk is MK_ERR_STATE, a sharer screens against its OWN table, the stream is idle afterwards; the export,
 * mk_export_stats and the counting figures of mk_get_stats are what they were.  The context's chunk buffers serve as
 * scratch.
 * mk_screen_text: text in host memory, moved to the device in pieces of about piece_bytes (0: pick; limits of
 * mk_load_tsv) that are cut where a record starts (the rule of mk_record_cuts: no record is split, a record longer than
 * a piece makes its piece that long); the rows of a piece follow those of the piece before.  mk_screen_device: text and
 * rows in DEVICE memory of the context's GPU, one piece.  st may be NULL. */
#define MK_SCREEN_FOLD 1u   /* fold every ACGT-only window onto min(window, reverse complement) */
typedef struct mk_screen_row_t { /* one per record, in text order */
  uint64_t windows;  /* k-length windows of the record: max(0, L - k + 1), L = kept characters          */
  uint64_t hits;     /* windows whose k-mer's count in the table is >= at_least                         */
  uint64_t sum;      /* sum of the counts of all windows (modulo 2^64)                                   */
  uint64_t min, max; /* smallest / largest count over the windows (an absent k-mer is 0); both 0 when windows == 0 */
} mk_screen_row_t;
typedef struct mk_screen_t {
  uint64_t bytes;            /* text consumed                                                       */
  uint64_t records;          /* rows                                                                */
  uint64_t windows, hits;    /* summed over the records                                             */
  uint64_t packed_windows;   /* windows probed in the packed table / dense bins                     */
  uint64_t text_windows;     /* windows probed in the by-reference table                            */
  uint64_t folded;           /* windows replaced by their reverse complement (MK_SCREEN_FOLD)       */
  int32_t headless, pieces;  /* 1: a leading record without a header line; pieces the text went in  */
  /* seconds: host time inside the copies towards the device; HIP-event time of the parser and the record scan; of the
   * probe kernels; wall time of the call */
  double s_read, s_parse, s_probe, s_total;
} mk_screen_t;
int mk_screen_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, uint64_t at_least,
                   mk_screen_row_t* rows, size_t cap, size_t* nrows, mk_screen_t* st);
int mk_screen_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, unsigned flags, uint64_t at_least,
                     mk_screen_row_t* d_rows, size_t cap, size_t* nrows, mk_screen_t* st);

/* ---- sequences in, the matched (or the unmatched) records out: the reads themselves, filtered on the GPU by what
 *      mk_screen_* finds for them (BBDuk's outm / out, kmc_tools filter, khmer's filter-abund) ----
 * The text is read, cut into records and probed exactly as mk_screen_text does it: same parser, same rows, same
 * mk_screen_t figures (st->screen; its s_total is the wall time of this whole call), same opening rules and errors --
 * the table only read and made final first, MK_ERR_STATE with an open chunk or a refused one, MK_ERR_NON_ASCII, the fold
 * rule (MK_FILTER_FOLD = MK_SCREEN_FOLD), pieces cut by mk_record_cuts, device text of any alignment, the stream idle
 * afterwards and the counting figures untouched.
 * Bytes of a record: from the first byte of its header LINE (the byte after the nearest LF or CR in front of the '>', or
 * the first byte of the text: leading blanks of the line belong to the record) to the byte in front of the next
 * record's header line, or the end of the text.  The headless record (st->screen.headless) runs from byte 0.  Otherwise
 * the bytes in front of the first header line are the preamble (st->preamble): they hold no kept character and belong
 * to no record.  The records partition the text minus its preamble.
 * Rule: hits counts the windows whose count is >= at_least, as in screen.  A record is MATCHED iff windows > 0 and
 * hits >= min_hits and hits * 1000000 >= min_ppm * windows (128-bit integers); a record without windows never is.
 * "every k-mer occurs at least N times" is {N, 1, 1000000}.  at_least and min_hits >= 1, min_ppm <= 1000000, reserved
 * is ignored; a NULL rule, a value out of range or an unknown flag bit is MK_ERR_ARG and the message names it.
 * Output: the bytes of the matched records -- with MK_FILTER_INVERT of the unmatched ones -- in text order, byte for
 * byte: nothing is re-wrapped, the preamble goes to neither, *out_len <= n.  keep[r] = 1 iff record r was emitted;
 * rows[r] is its screen row.  rows and keep may each be NULL (cap is ignored when both are).  With out_cap or cap too
 * small: MK_ERR_RANGE, the needed sizes in *out_len and *nrows, nothing written past either -- every piece is still
 * walked to learn them.  st may be NULL.
 * mk_filter_text: host memory in and out, piece by piece (each piece's output is appended to out by its copy back).
 * mk_filter_device: text, out, rows and keep in DEVICE memory of the context's GPU, one piece. */
#define MK_FILTER_FOLD   1u   /* = MK_SCREEN_FOLD */
#define MK_FILTER_INVERT 2u   /* emit the unmatched records */
typedef struct mk_filter_rule_t {
  uint64_t at_least, min_hits;
  uint32_t min_ppm, reserved;
} mk_filter_rule_t;
typedef struct mk_filter_t {
  mk_screen_t screen;                 /* as mk_screen_* fills it for the same text                              */
  uint64_t records_out, bytes_out;    /* records emitted, their bytes                                          */
  uint64_t preamble;                  /* bytes in front of the first header line of a text that is not headless */
  /* seconds: HIP-event time of the record starts, the decision and the scan; of the gather; host time in the copies back */
  double s_place, s_gather, s_write;
} mk_filter_t;
int mk_filter_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_filter_rule_t* rule,
                   uint8_t* out, size_t out_cap, size_t* out_len,
                   mk_screen_row_t* rows, uint8_t* keep, size_t cap, size_t* nrows, mk_filter_t* st);
int mk_filter_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, unsigned flags, const mk_filter_rule_t* rule,
                     uint8_t* d_out, size_t out_cap, size_t* out_len,
                     mk_screen_row_t* d_rows, uint8_t* d_keep, size_t cap, size_t* nrows, mk_filter_t* st);

/* ---- sequences in, the count under every k-mer window out: the vector mk_screen_* folds into five numbers a record,
 *      position by position (Jellyfish `query -s`, a k-mer coverage track along a contig, the first window whose count
 *      drops), and the median of every record's counts (khmer's count-median, the decision of normalize-by-median) ----
 * Text, records, windows, probing, fold, opening rules and errors are mk_screen_*'s, word for word: same parser, same
 * rows (rows[r] is the screen row of record r for the same text and at_least), same mk_screen_t figures (st->screen; its
 * s_total is the wall time of this whole call), the table only read and made final first, MK_ERR_STATE with an open
 * chunk or a refused one, MK_ERR_NON_ASCII, the fold rule (MK_TRACK_FOLD = MK_SCREEN_FOLD), pieces cut by
 * mk_record_cuts, device text of any alignment, the stream idle afterwards, the counting figures and the export
 * untouched.
 * Record r has rows[r].windows windows; window j starts at the record's j-th kept character.  counts[offsets[r] + j] is
 * the count mk_lookup would return for those k bytes -- under min(window, reverse complement) with MK_TRACK_FOLD -- 0
 * when the k-mer is absent.  offsets[0] = 0, offsets[r + 1] = offsets[r] + rows[r].windows, offsets[nrows] = *nwindows:
 * offsets needs cap + 1 entries, and they number the whole call, not a piece.  median[r] is element windows / 2 of the
 * record's counts sorted ascending, as stored (so clipped under MK_TRACK_SAT32) -- khmer's rule -- and 0 for a record
 * without windows.  With MK_TRACK_SAT32 counts and median are uint32_t, min(count, 2^32 - 1), and st->saturated counts
 * the elements clipped; without it both are uint64_t.
 * offsets, median and rows may each be NULL (cap is ignored when all three are); with median NULL nothing of the median
 * runs.  counts_cap is in elements.  With counts_cap or cap too small: MK_ERR_RANGE, the needed sizes in *nwindows and
 * *nrows, nothing written past either -- every piece is still walked to learn them (counts = NULL, counts_cap = 0 is the
 * sizing call).  An unknown flag bit or at_least == 0 is MK_ERR_ARG and the message names it.  st may be NULL.
 * mk_track_text: host memory in and out, piece by piece (each piece's counts are appended to counts by its copy back).
 * mk_track_device: text, counts, offsets, median and rows in DEVICE memory of the context's GPU, one piece; the text at
 * any address, the others aligned to their elements (MK_ERR_ARG otherwise); the median takes fewer than 2^32 windows. */
#define MK_TRACK_FOLD  1u   /* = MK_SCREEN_FOLD */
#define MK_TRACK_SAT32 2u   /* counts (and medians) are uint32_t, min(count, 2^32 - 1) */
/* How the median is found is no part of its definition: a record of more than this many windows is not sorted, its
 * median is found by radix selection over its counts where they lie (a contig costs four reads of its counts, not a
 * sort of one segment); the size from which selection was never slower on the MI355X. */
#ifndef MK_MEDIAN_SELECT_MIN   /* (an A/B build of the library may set another) */
#define MK_MEDIAN_SELECT_MIN 16384u
#endif
typedef struct mk_track_t {
  mk_screen_t screen;          /* as mk_screen_* fills it for the same text and at_least */
  uint64_t windows_out;        /* elements written to counts */
  uint64_t saturated;          /* elements clipped by MK_TRACK_SAT32 */
  /* seconds: HIP-event time of the offsets scan; of the track kernel; of the sort and the pick; host time in the copies back */
  double s_place, s_track, s_median, s_write;
} mk_track_t;
int mk_track_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, uint64_t at_least,
                  void* counts, size_t counts_cap, size_t* nwindows,
                  uint64_t* offsets, void* median, mk_screen_row_t* rows, size_t cap, size_t* nrows, mk_track_t* st);
int mk_track_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, unsigned flags, uint64_t at_least,
                    void* d_counts, size_t counts_cap, size_t* nwindows,
                    uint64_t* d_offsets, void* d_median, mk_screen_row_t* d_rows, size_t cap, size_t* nrows, mk_track_t* st);

/* ---- sequences in, every record cut in front of its first low-abundance k-mer out: what one scans mk_track_*'s counts
 *      for, done where the counts are (khmer's trim_on_abundance / filter-abund, the error trimming in front of an
 *      assembly or a second count) ----
 * Text, records, windows, probing, fold, opening rules and errors are mk_screen_*'s, word for word: same parser, same
 * rows (rows[r] is the screen row of record r for the same text and rule->at_least), same mk_screen_t figures
 * (st->screen; its s_total is the wall time of this whole call), the table only read and made final first, MK_ERR_STATE
 * with an open chunk or a refused one, MK_ERR_NON_ASCII, the fold rule (MK_TRIM_FOLD = MK_SCREEN_FOLD), pieces cut by
 * mk_record_cuts, the stream idle afterwards, the counting figures and the export untouched.
 * Rule: a window is LOW when its count -- the one mk_lookup returns for those k bytes, folded under MK_TRIM_FOLD, 0 for
 * an absent k-mer -- is below at_least.  Record r has L kept characters and rows[r].windows windows; j is the index of
 * its first low window.  No low window: kept[r] = L.  j >= 1: kept[r] = j + k - 1 (the characters in front of the last
 * one of window j).  j = 0, or no window at all: kept[r] = 0.  Then kept[r] < max(min_len, k) gives kept[r] = 0
 * (min_len 0 means k).  A record is emitted iff kept[r] > 0.  kept numbers the records of the whole call, not a piece.
 * Output: the emitted records in text order, each as the bytes of its header LINE as they stand -- from the first byte of
 * the line (mk_filter_*'s record start, leading blanks included) through its terminator LF, CR LF or lone CR; none for
 * the headless record -- then its first kept[r] kept characters on one line and one LF.  The sequence comes from the
 * parsed stream, so it is exactly what was probed: '*' removed, lines stripped and joined.  Nothing of the preamble
 * (st->preamble, as in mk_filter_t) is emitted.  *out_len <= n + 1; for a text of one-line, LF-terminated records of
 * which none is trimmed or dropped the output is the input byte for byte.
 * at_least >= 1; a NULL rule, at_least == 0 or an unknown flag bit is MK_ERR_ARG and the message names it.  kept and
 * rows may each be NULL (cap is ignored when both are).  With out_cap or cap too small: MK_ERR_RANGE, the needed sizes
 * in *out_len and *nrows, nothing written past either -- every piece is still walked to learn them (out = NULL,
 * out_cap = 0 is the sizing call).  st may be NULL.
 * mk_trim_text: host memory in and out, piece by piece (each piece's output is appended to out by its copy back).
 * mk_trim_device: text, out, kept and rows in DEVICE memory of the context's GPU, one piece; text and out at any
 * address, d_kept and d_rows aligned to 8 (MK_ERR_ARG otherwise). */
#define MK_TRIM_FOLD 1u          /* = MK_SCREEN_FOLD */
typedef struct mk_trim_rule_t { uint64_t at_least, min_len; } mk_trim_rule_t;
typedef struct mk_trim_t {
  mk_screen_t screen;                                      /* as mk_screen_* fills it for the same text and at_least */
  uint64_t records_out, records_trimmed, records_dropped;  /* emitted; emitted shorter than they came; not emitted */
  uint64_t bases_in, bases_out, bytes_out;                 /* kept characters of all records; emitted; output bytes */
  uint64_t preamble;                                       /* bytes in front of the first header line of a text that is not headless */
  /* seconds: HIP-event time of the record starts and header ends; of the first-low walk; of the gather (the decision
   * and its scan run between the two and are in none); host time in the copies back */
  double s_place, s_first, s_gather, s_write;
} mk_trim_t;
int mk_trim_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_trim_rule_t* rule,
                 uint8_t* out, size_t out_cap, size_t* out_len, uint64_t* kept, mk_screen_row_t* rows, size_t cap,
                 size_t* nrows, mk_trim_t* st);
int mk_trim_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, unsigned flags, const mk_trim_rule_t* rule,
                   uint8_t* d_out, size_t out_cap, size_t* out_len, uint64_t* d_kept, mk_screen_row_t* d_rows, size_t cap,
                   size_t* nrows, mk_trim_t* st);

/* ---- nucleotide sequences in, their open reading frames out as protein FASTA: six-frame stop-to-stop ORF calling (what
 *      OrfM and getorf do in front of a protein k-mer profile), optionally from the first start codon.  No gene model, no
 *      RBS, no scoring: this is not prodigal. ----
 * Text, records and kept characters are mk_screen_*'s: same parser, lines stripped and joined, '*' removed, a header
 * line without sequence is a record, a leading headless record is allowed, MK_ERR_NON_ASCII as there, pieces cut by
 * mk_record_cuts (nothing depends on piece_bytes).  Any context of the device serves: alphabet and k do not matter, the
 * table is neither read nor changed, the chunk buffers are scratch, a spoiled context or an open chunk is MK_ERR_STATE,
 * the stream is idle afterwards and the counting figures are untouched.
 * Rule: s[0..L) are a record's kept characters; A a -> 0, C c -> 1, G g -> 2, T t U u -> 3, every other byte "other".
 * For t = s and then its reverse complement (complementing keeps "other") and each class c in 0, 1, 2, codon i covers
 * t[c + 3i, c + 3i + 3) for i < (L - c) / 3.  A codon with an "other" byte translates to X and is neither stop nor
 * start; any other by the standard code, index 16 c1 + 4 c2 + c3 in
 *   KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF
 * Stops are TAA TAG TGA.  A stretch is a maximal run of non-stop codons of one class; the record's ends close stretches
 * too.  Default: the ORF is the stretch.  MK_ORF_START: the stretch from its first ATG on (with MK_ORF_ALT also GTG and
 * TTG, translated as they stand); a stretch without a start yields nothing.  An ORF of fewer than min_aa codons is
 * dropped.  Coordinates are on the forward strand, half open: an ORF [a', b') of the reverse complement is
 * [L - b', L - a').  begin is the left end, aa the number of codons, frame 1 + c forward and 4 + c reverse.  Order: by
 * (record, right end in forward coordinates of the stretch the ORF was cut from, forward before reverse); n is the ORF's
 * 1-based rank within its record in that order.  MK_ORF_PLUS / MK_ORF_MINUS restrict the strand; ranks count what is
 * emitted.
 * Output, per ORF: '>' name '_' begin+1 '_' frame '_' n LF, the aa amino acids on one line, LF.  name: the bytes of the
 * record's header line behind its '>' up to the first byte <= 0x20 or the end of the line; empty for the headless
 * record.  No stop character is written.  rows[i] = {record (numbered over the whole call), begin, aa, frame}.
 * A NULL opt, min_aa == 0, an unknown flag, MK_ORF_ALT without MK_ORF_START, or MK_ORF_PLUS with MK_ORF_MINUS is
 * MK_ERR_ARG and the message names it.  out and rows may each be NULL (cap is ignored without rows).  With out_cap or
 * cap too small: MK_ERR_RANGE, the needed sizes in *out_len and *norfs, nothing written past either -- every piece is
 * still walked to learn them (out = NULL, out_cap = 0 is the sizing call; the output can be longer than the input).
 * mk_orf_text: host memory in and out, piece by piece.  mk_orf_device: text, out and rows in DEVICE memory of the
 * context's GPU, one piece; text and out at any address, d_rows aligned to 8 (MK_ERR_ARG otherwise). */
#define MK_ORF_START 1u
#define MK_ORF_ALT   2u   /* only with START, else MK_ERR_ARG */
#define MK_ORF_PLUS  4u
#define MK_ORF_MINUS 8u
typedef struct mk_orf_opt_t { uint32_t min_aa, flags; } mk_orf_opt_t;
typedef struct mk_orf_row_t { uint64_t record, begin; uint32_t aa, frame; } mk_orf_row_t;   /* 24 bytes */
typedef struct mk_orf_t {
  /* input bytes, records, kept characters; ORFs, their amino acids, output bytes, the longest ORF's codons, ORFs per
   * frame 1..6; bytes in front of the first header line of a text that is not headless */
  uint64_t bytes, records, bases, orfs, residues, bytes_out, longest, per_frame[6], preamble;
  int32_t headless, pieces;
  /* seconds: host time in the copies in; HIP-event time of the parse and record scan; of the ORF scan (tile summaries,
   * carries, count, rows); of the record starts, names, lengths and their scan; of the gather; host time in the copies
   * back; wall time of the call */
  double s_read, s_parse, s_find, s_place, s_emit, s_write, s_total;
} mk_orf_t;
int mk_orf_text  (mk_ctx* ctx, const uint8_t* text,   size_t n, size_t piece_bytes, const mk_orf_opt_t* opt,
                  uint8_t* out,   size_t out_cap, size_t* out_len, mk_orf_row_t* rows,   size_t cap, size_t* norfs, mk_orf_t* st);
int mk_orf_device(mk_ctx* ctx, const uint8_t* d_text, size_t n,                     const mk_orf_opt_t* opt,
                  uint8_t* d_out, size_t out_cap, size_t* out_len, mk_orf_row_t* d_rows, size_t cap, size_t* norfs, mk_orf_t* st);

/* ---- sequences in, every isolated substitution the table can name put right out: k-mer-spectrum error correction
 *      where the counts are (the conservative "spectral alignment" step of Musket, Lighter, BFC and Quake; with
 *      abundance trimming and normalisation the third standard step in front of an assembly or a second count) ----
 * Text, records, kept characters, windows, probing, fold, opening rules, pieces and errors are mk_screen_*'s, word for
 * word, as for mk_trim_*: same parser, same rows (rows[r] is the screen row of record r of the UNCORRECTED text for
 * rule->at_least), same mk_screen_t figures (st->screen; its s_total is the wall time of this whole call), MK_ERR_STATE
 * with an open chunk or a refused one, MK_ERR_NON_ASCII, the fold rule (MK_CORRECT_FOLD = MK_SCREEN_FOLD), pieces cut by
 * mk_record_cuts, the stream idle afterwards, the counting figures and the export untouched.  The rule is defined for
 * nucleotide contexts with packed keys only (MK_ALPHABET_NT2, k <= 64): any other context is MK_ERR_ARG.
 * Rule: record r has the kept characters s[0..L) and W = L - k + 1 windows; c[j] is the count mk_lookup returns for
 * the k bytes s[j..j+k), folded under MK_CORRECT_FOLD, 0 for an absent k-mer.  Window j is WEAK iff c[j] < at_least.  A
 * RUN is a maximal interval [a, b] of weak windows, n = b - a + 1 of them.  A run has at most one candidate position p:
 *   a == 0 and b == W - 1    none (nothing in the record is solid)
 *   a == 0, n <= k           p = b             (an error in the first k characters)
 *   b == W - 1, n <= k       p = a + k - 1     (an error in the last k characters)
 *   interior, n == k         p = b             (= a + k - 1: the one character all k windows hold)
 *   anything else            none
 * The alternatives at p are the bases of A C G T other than the byte s[p]: three, or four where s[p] is none of them (an
 * N, a lower-case letter).  An alternative x is VIABLE iff every window of the run has a count >= at_least with s[p]
 * replaced by x -- mk_lookup's count of those k bytes again; a window that still holds a byte outside ACGT is looked up
 * as text.  Exactly one viable alternative: s[p] becomes it (FIXED).  Two or more: AMBIGUOUS, none: UNFIXABLE, and the
 * record stays as it is there.  Every run is judged against the record as it came, and all fixes are applied together:
 * the windows a candidate tests are exactly the windows that hold its p, and none of them belongs to another run or
 * holds another run's p, because a solid window lies between two runs -- so neither the order of the runs nor that of
 * the records, pieces or lanes reaches the result.  One pass; a second pass is a second call on the output.
 * Output: EVERY record of the text, in text order, each as the bytes of its header LINE as they stand (mk_trim_*'s: from
 * the first byte of the line through its terminator; none for the headless record), then, if L > 0, its L characters on
 * one line and one LF; a record without characters is its header line alone.  Nothing of the preamble (st->preamble)
 * is emitted.  *out_len <= n + 1; a text of one-line, LF-terminated records in which nothing is fixed comes back byte
 * for byte.  fix[r] counts record r's runs and, of those with a candidate, the fixed, ambiguous and unfixable ones:
 * runs - fixed - ambiguous - unfixable runs had a shape without a candidate.  fix numbers the records of the whole call.
 * at_least >= 1 and reserved == 0; a NULL rule, a value out of range or an unknown flag bit is MK_ERR_ARG and the
 * message names it.  The result is exact for every at_least up to 2^64 - 1.  fix and rows may each be NULL (cap is
 * ignored when both are).  With out_cap or cap too small: MK_ERR_RANGE, the needed sizes in *out_len and *nrows, nothing
 * written past either -- every piece is still walked to learn them (out = NULL, out_cap = 0 is the sizing call).  st may
 * be NULL.
 * mk_correct_text: host memory in and out, piece by piece (each piece's output is appended to out by its copy back).
 * mk_correct_device: text, out, fix and rows in DEVICE memory of the context's GPU, one piece; text and out at any
 * address, d_fix and d_rows aligned to 8 (MK_ERR_ARG otherwise). */
#define MK_CORRECT_FOLD 1u       /* = MK_SCREEN_FOLD */
typedef struct mk_correct_rule_t { uint64_t at_least, reserved; } mk_correct_rule_t;
typedef struct mk_correct_row_t { uint32_t runs, fixed, ambiguous, unfixable; } mk_correct_row_t;
typedef struct mk_correct_t {
  mk_screen_t screen;                                      /* as mk_screen_* fills it for the same text and at_least */
  uint64_t records;                                        /* records emitted: all of them */
  uint64_t runs, candidates;                               /* weak runs; those whose shape names a position */
  uint64_t fixed, ambiguous, unfixable;                    /* the candidates by outcome: they add up to candidates */
  uint64_t bases, bytes_out;                               /* kept characters of all records; output bytes */
  uint64_t preamble;                                       /* bytes in front of the first header line of a text that is not headless */
  /* seconds: HIP-event time of the placement (record starts, header ends, window offsets); of the track kernel; of the
   * run kernel; of the try kernel and the patches; of the gather (the lengths and their scan run between the two and
   * are in none); host time in the copies back */
  double s_place, s_track, s_runs, s_try, s_gather, s_write;
} mk_correct_t;
int mk_correct_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_correct_rule_t* rule,
                    uint8_t* out, size_t out_cap, size_t* out_len, mk_correct_row_t* fix, mk_screen_row_t* rows, size_t cap,
                    size_t* nrows, mk_correct_t* st);
int mk_correct_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, unsigned flags, const mk_correct_rule_t* rule,
                      uint8_t* d_out, size_t out_cap, size_t* out_len, mk_correct_row_t* d_fix, mk_screen_row_t* d_rows, size_t cap,
                      size_t* nrows, mk_correct_t* st);

/* ---- FASTQ in, the same FASTQ out with the correction above applied and the qualities kept: the text is read on the
 *      device as it stands, and because every record is emitted and a fix replaces one byte by one byte, the output is
 *      the input with at most one byte per fixed run changed (what Lighter, Musket and BFC hand to an assembler, a mapper
 *      or a second correction pass) ----
 * Lines and records are mk_fastq_select_*'s, word for word: lines are split on '\n' only and numbered across the whole
 * text, a last line without '\n' is a line, record r is lines 4r .. 4r + 3, and the up to 3 lines behind the last
 * complete record are tolerated only if they are all empty (otherwise the text ends inside a record).  *nrows is the
 * number of records.
 * Record checks, on the device, for every record, before anything is parsed; a failure is MK_ERR_UNSUPPORTED and the
 * message names the lowest failing record, numbered over the whole call, and the first check it fails, in this order:
 *   line 4r starts with '@';  line 4r + 2 starts with '+';
 *   the sequence line 4r + 1 and the quality line 4r + 3 are equally long, one trailing '\r' not counted on either;
 *   the sequence line, without its trailing '\r', holds no '*' and none of the bytes str.strip() removes.
 * Rule: the FASTA view of the text is mk_fq2fa's -- here the text copied on the device and rewritten in place ('@' of
 * line 4r made '>', every byte of lines 4r + 2 and 4r + 3 made '\n', nothing moved) -- and mk_correct_*'s rule is
 * applied to that view, word for word: fix, rows, MK_CORRECT_FOLD, the context restrictions (MK_ERR_ARG), MK_ERR_STATE
 * and MK_ERR_NON_ASCII are as there, and fix[r] and rows[r] are exactly what mk_correct_text returns for
 * mk_fq2fa(text).  st->correct is filled as there for the view, with bytes_out = n, preamble = 0 and s_gather = 0.
 * View check: after the parse it is checked, per record, that the parser found exactly the text's records, each where
 * its header line starts, and counted as record r's characters exactly the bytes of its sequence line.  A sequence line
 * that the parser reads differently -- one that starts with '>', say, is a header line of the view -- is
 * MK_ERR_UNSUPPORTED; the message names the lowest such record, or gives both record counts when only they differ.
 * Nothing is patched before this check has been read back clean.
 * Output: the n input bytes as they stand -- CR LF stays, a last record without '\n' stays open, trailing lines stay --
 * but for every FIXED run the byte of its p, at offset p of the sequence line, is the fixing base, and where
 * rule->new_qual != 0 the byte at the same offset of the quality line is new_qual (Lighter's -newQual).  st->patched
 * counts the sequence bytes changed (= st->correct.fixed).  *out_len = n on success; on any error 0, except that
 * out_cap < n is MK_ERR_RANGE with *out_len = n, decided before any work (out = NULL, out_cap = 0 is the sizing call)
 * and that cap below the record count is MK_ERR_RANGE with *out_len = n and the count in *nrows, as for mk_correct_*.
 * at_least >= 1, reserved == 0, new_qual 0 or in 33..126; a NULL rule, a value out of range or an unknown flag bit is
 * MK_ERR_ARG.  The table is only read; the counting figures, the export and what mk_fastq_stats reports stay untouched.
 * mk_correct_fastq_text: host memory in and out; pieces end behind a line 4j once they hold piece_bytes (mk_fastq_cuts;
 * 0: the default, and the limits, of the screen calls).  out is written once, after the last piece has passed its
 * checks: on an error it holds what it held.  Output, fix, rows and messages do not depend on piece_bytes for a text
 * with at most one kind of fault; of a malformed record, a sequence line the parser reads differently and a byte
 * >= 0x80 in different records, the one in the earliest piece is reported, so which it is may depend on piece_bytes.
 * mk_correct_fastq_device: everything in DEVICE memory of the context's GPU, one piece; text and out at any address,
 * d_fix and d_rows aligned to 8.  d_out == d_fastq corrects in place; any other overlap is MK_ERR_ARG.  d_out is not
 * written before every check has passed. */
typedef struct mk_correct_fastq_rule_t { uint64_t at_least; uint32_t new_qual; uint32_t reserved; } mk_correct_fastq_rule_t;
typedef struct mk_correct_fastq_t {
  mk_correct_t correct;                 /* as mk_correct_* fills it for the FASTA view of the same text */
  uint64_t lines, patched;              /* lines of the text; bytes changed in sequence lines (= correct.fixed) */
  /* seconds: host time in the copies to the device; HIP-event time of the line index and the record checks; of the view
   * check and the patch */
  double s_copy, s_index, s_patch;
} mk_correct_fastq_t;
int mk_correct_fastq_text(mk_ctx* ctx, const uint8_t* fastq, size_t n, size_t piece_bytes, unsigned flags,
                          const mk_correct_fastq_rule_t* rule, uint8_t* out, size_t out_cap, size_t* out_len, mk_correct_row_t* fix,
                          mk_screen_row_t* rows, size_t cap, size_t* nrows, mk_correct_fastq_t* st);
int mk_correct_fastq_device(mk_ctx* ctx, const uint8_t* d_fastq, size_t n, unsigned flags, const mk_correct_fastq_rule_t* rule,
                            uint8_t* d_out, size_t out_cap, size_t* out_len, mk_correct_row_t* d_fix, mk_screen_row_t* d_rows,
                            size_t cap, size_t* nrows, mk_correct_fastq_t* st);

/* ---- sequences in, the reads thinned to a target depth out: digital normalisation by the median mk_track_* computes,
 *      decided and applied where the counts are (BBNorm's plan with khmer's normalize-by-median depth; with abundance
 *      trimming the other standard step in front of an assembly or a second count) ----
 * Text, records, windows, probing, fold, opening rules, pieces and errors are mk_screen_*'s, word for word, as for
 * mk_trim_*: same parser, same rows, same mk_screen_t figures (st->screen; its s_total is the wall time of this whole
 * call), MK_ERR_STATE with an open chunk or a refused one, MK_ERR_NON_ASCII, the fold rule (MK_NORM_FOLD =
 * MK_SCREEN_FOLD), pieces cut by mk_record_cuts, the stream idle afterwards, the counting figures and the export
 * untouched.  The table is only read: it has been counted from all the reads beforehand -- count first, then keep every
 * read with probability target / depth, which is BBNorm's plan -- and the depth of a read is khmer's: the median of its
 * k-mers' counts.  khmer's streaming normalize-by-median is NOT this: there the table grows from the reads that were
 * kept, so a read's fate depends on the reads in front of it, the result on their order, and the procedure is serial by
 * definition.  Here every record is decided on its own, from a table that does not change, so pieces and lanes may take
 * them in any order.
 * med[r] is mk_track_*'s median under MK_TRACK_SAT32: element windows / 2 of min(count, 2^32 - 1) over the record's
 * windows sorted ascending, 0 for a record without windows; it is returned as median[r].  Record r is KEPT iff
 * windows > 0 and med >= min_depth and (med <= target, or else u(r) * med < target << 32).  r is the record's index over
 * the WHOLE CALL, not over a piece, and u(r) is the upper 32 bits of splitmix64:
 *   z = seed + (r + 1) * 0x9E3779B97F4A7C15 (mod 2^64); z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31
 * so a record of depth med > target is kept with probability target / med, the same records for the same seed.  Both
 * products fit in 64 bits: 1 <= target <= 2^32 - 1 and min_depth <= 2^32 - 1.  A target of 0, a target or min_depth of
 * 2^32 or more, a NULL rule or an unknown flag bit is MK_ERR_ARG and the message names it.
 * Output: the kept records -- with MK_NORM_INVERT every record that is not kept, records without windows included -- in
 * text order, byte for byte as mk_filter_* emits a record: from the first byte of its header line to the byte in front
 * of the next record's header line, the headless record from byte 0.  The preamble (st->preamble) goes to neither;
 * *out_len <= n.  keep[r] = 1 iff record r was emitted; rows[r] is its screen row for at_least = max(min_depth, 1).
 * median, keep and rows may each be NULL (cap is ignored when all three are).  With out_cap or cap too small:
 * MK_ERR_RANGE, the needed sizes in *out_len and *nrows, nothing written past either -- every piece is still walked to
 * learn them.  The output does not depend on piece_bytes.  st may be NULL.
 * mk_norm_text: host memory in and out, piece by piece.  mk_norm_device: text, out, median, keep and rows in DEVICE
 * memory of the context's GPU, one piece; text and out at any address, d_median aligned to 4 and d_rows to 8
 * (MK_ERR_ARG otherwise).  As with mk_track_*'s median, a piece of 2^32 windows or more is refused (MK_ERR_ARG). */
#define MK_NORM_FOLD   1u   /* = MK_SCREEN_FOLD */
#define MK_NORM_INVERT 2u   /* emit the records that are NOT kept (BBNorm's outt) */
typedef struct mk_norm_rule_t { uint64_t target, min_depth, seed; } mk_norm_rule_t;
typedef struct mk_norm_t {
  mk_screen_t screen;      /* as mk_screen_* fills it for the same text and at_least = max(min_depth, 1) */
  /* emitted; windows == 0; med < min_depth; med > target; of those, not kept */
  uint64_t records_out, records_short, records_low, records_over, records_thinned;
  uint64_t bytes_out, preamble;
  /* seconds: HIP-event time of the placement (window offsets, record starts); of the track kernel; of the median; of
   * the gather (the decision and its scan run between the two and are in none); host time in the copies back */
  double s_place, s_track, s_median, s_gather, s_write;
} mk_norm_t;
int mk_norm_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_norm_rule_t* rule,
                 uint8_t* out, size_t out_cap, size_t* out_len, uint32_t* median, uint8_t* keep, mk_screen_row_t* rows,
                 size_t cap, size_t* nrows, mk_norm_t* st);
int mk_norm_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, unsigned flags, const mk_norm_rule_t* rule,
                   uint8_t* d_out, size_t out_cap, size_t* out_len, uint32_t* d_median, uint8_t* d_keep,
                   mk_screen_row_t* d_rows, size_t cap, size_t* nrows, mk_norm_t* st);

/* ---- paired reads: mk_filter_*, mk_trim_* and mk_norm_* with the PAIR as the unit, so that no read is ever emitted
 *      without its mate among the pairs (khmer's -p, BBDuk's and BBNorm's pair handling; what `megahit --12` and
 *      `spades --12` read) ----
 * The text is INTERLEAVED: records 2p and 2p + 1 of the whole call are the mates a and b of pair p.  Mates are defined
 * by position only; names are not compared.  The headless record, if any, is record 0 and so a first mate.  Text,
 * records, windows, probing, fold, opening rules, errors and argument checks are mk_screen_*'s, as for the unpaired call
 * of the same op (rule->op; only that op's member of the rule is read and checked as that call checks it).  The
 * per-record results are the unpaired call's, own to each mate: rows[r] for every op (at_least = filter.at_least,
 * trim.at_least, max(norm.min_depth, 1)), kept[r] for TRIM -- always the mate's own figure --, median[r] for NORM.
 *   FILTER  own[r] = matched by mk_filter_*'s rule.  The pair passes iff own[a] | own[b]; with MK_PAIRS_BOTH iff
 *           own[a] & own[b].
 *   TRIM    own[r] = kept[r] > 0.  The pair passes iff own[a] & own[b]; the mates keep their own trimmed lengths.
 *   NORM    a mate is eligible iff windows > 0 and med >= min_depth; D = the smallest med over the eligible mates.  The
 *           pair passes iff a mate is eligible and (D <= target or u(2p) * D < target << 32), u being mk_norm_*'s draw
 *           at the first mate's index over the whole call.  With min_depth = 0 this is khmer's -p rule: the pair is kept
 *           if either mate is at or under the cutoff.  own[r] = 1 iff the pair passes.
 * out: both mates of every passing pair -- with MK_PAIRS_INVERT of every pair that does not pass -- in text order, each
 * record byte for byte as the unpaired op emits it (mk_filter_*'s bytes for FILTER and NORM, mk_trim_*'s for TRIM): the
 * output is itself interleaved and holds an even number of records.  singles (optional, singles_cap bytes of room): the
 * records with own = 1 whose pair did not pass -- TRIM's orphans, the matched mates under MK_PAIRS_BOTH; NORM has none --
 * emitted the same way, in text order; with singles NULL they are only counted and *singles_len tells their bytes.  A
 * singles buffer together with MK_PAIRS_INVERT is MK_ERR_ARG.  keep[r]: 0 = not emitted, 1 = emitted in out, 2 = an
 * orphan (emitted in singles where that is given).  kept (TRIM) and median (NORM) are ignored by the other ops.  keep,
 * kept, median and rows may each be NULL (cap is ignored when all are).
 * With out_cap, singles_cap or cap too small: MK_ERR_RANGE, the needed sizes in *out_len, *singles_len and *nrows,
 * nothing written past any -- every piece is still walked.  An ODD number of records over the whole call is
 * MK_ERR_RANGE: mk_last_error names the count, *out_len = *singles_len = 0 and the contents of the buffers are
 * unspecified.  No record is success with empty outputs.  An unknown op, an unknown flag bit, MK_PAIRS_INVERT with TRIM,
 * MK_PAIRS_BOTH with TRIM or NORM, or a NULL rule is MK_ERR_ARG.
 * mk_pairs_text: host memory, piece by piece; no piece ends between mates (a piece that holds an odd number of records
 * hands its last one to the next piece; one that holds a single record grows to the next cut), so out, singles and
 * every array are independent of piece_bytes; st->screen counts every record once.  mk_pairs_device: everything in
 * DEVICE memory of the context's GPU, one piece; text, out and singles at any address, d_kept and d_rows aligned to 8,
 * d_median to 4 (MK_ERR_ARG otherwise).  The counting figures and the export are untouched. */
#define MK_PAIRS_FILTER 0
#define MK_PAIRS_TRIM   1
#define MK_PAIRS_NORM   2
#define MK_PAIRS_FOLD   1u  /* = MK_SCREEN_FOLD */
#define MK_PAIRS_INVERT 2u  /* FILTER, NORM: emit the pairs that do not pass.  TRIM: MK_ERR_ARG */
#define MK_PAIRS_BOTH   4u  /* FILTER only: a pair passes iff BOTH mates match (default: either).  Else MK_ERR_ARG */
typedef struct mk_pairs_rule_t {
  int32_t op, reserved;
  mk_filter_rule_t filter;
  mk_trim_rule_t trim;
  mk_norm_rule_t norm;
} mk_pairs_rule_t;
typedef struct mk_pairs_t {
  mk_screen_t screen;                  /* as mk_screen_* fills it for the same text and the op's at_least */
  uint64_t pairs, pairs_out;           /* pairs of the text; pairs emitted in out */
  uint64_t records_out, singles_out;   /* records in out (2 * pairs_out); orphans (emitted in singles where that is given) */
  uint64_t bytes_out, bytes_singles, preamble;
  /* per record, as mk_trim_t and mk_norm_t have them; records_dropped: kept[r] == 0; records_thinned: mates above the
   * target whose pair did not pass */
  uint64_t records_trimmed, records_dropped, bases_in, bases_out;
  uint64_t records_short, records_low, records_over, records_thinned;
  /* seconds: HIP-event time of the placement; of the op's walk (TRIM: first-low, NORM: track; FILTER: none); of the
   * median; of the gathers; host time in the copies back */
  double s_place, s_walk, s_median, s_gather, s_write;
} mk_pairs_t;
int mk_pairs_text(mk_ctx* ctx, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_pairs_rule_t* rule,
                  uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* singles, size_t singles_cap, size_t* singles_len,
                  uint8_t* keep, uint64_t* kept, uint32_t* median, mk_screen_row_t* rows, size_t cap, size_t* nrows,
                  mk_pairs_t* st);
int mk_pairs_device(mk_ctx* ctx, const uint8_t* d_text, size_t n, unsigned flags, const mk_pairs_rule_t* rule,
                    uint8_t* d_out, size_t out_cap, size_t* out_len, uint8_t* d_singles, size_t singles_cap, size_t* singles_len,
                    uint8_t* d_keep, uint64_t* d_kept, uint32_t* d_median, mk_screen_row_t* d_rows, size_t cap, size_t* nrows,
                    mk_pairs_t* st);
/* Two files (R1 / R2) are served on the HOST, off the hot path: plain C++, no GPU.  mk_interleave writes record i of
 * text1, then record i of text2, records delimited as mk_filter_* delimits them (a header line is one whose first
 * non-blank byte is '>'); the preambles are dropped; a record whose last byte is neither LF nor CR -- only a text's last
 * record can be -- gets one LF.  Texts with a headless record are MK_ERR_ARG; different record counts are MK_ERR_RANGE
 * and mk_host_error gives both counts.  *out_len <= n1 + n2 + 2; with cap too small MK_ERR_RANGE and the needed size in
 * *out_len (out = NULL, cap = 0 is the sizing call).  mk_split_pairs is the inverse for an interleaved text with an
 * even record count (odd: MK_ERR_RANGE): record 2p goes to out1, record 2p + 1 to out2, byte for byte. */
int mk_interleave(const uint8_t* text1, size_t n1, const uint8_t* text2, size_t n2, uint8_t* out, size_t cap, size_t* out_len,
                  size_t* npairs);
int mk_split_pairs(const uint8_t* text, size_t n, uint8_t* out1, size_t cap1, size_t* len1, uint8_t* out2, size_t cap2,
                   size_t* len2, size_t* npairs);
const char* mk_host_error(void); /* the message of this thread's last failed mk_interleave / mk_split_pairs / mk_fq_* */
/* The FASTQ analogues, for the R1 / R2 files of reads whose qualities are to be kept (mk_fastq_select_*): records are the
 * 4-line records defined there -- lines split on '\n' only, record i is lines 4i .. 4i + 3, nothing of a line is looked
 * at.  mk_fq_interleave writes record i of text1, then record i of text2, byte for byte; a last record without '\n' gets
 * one; empty lines behind the last complete record are dropped, 1 to 3 trailing lines that are not all empty are
 * MK_ERR_UNSUPPORTED (the text ends inside a record).  Different record counts are MK_ERR_RANGE and mk_host_error gives
 * both.  *out_len <= n1 + n2 + 2; with cap too small MK_ERR_RANGE and the needed size in *out_len (out = NULL, cap = 0 is
 * the sizing call).  mk_fq_split_pairs is the inverse for an interleaved text with an even record count (odd:
 * MK_ERR_RANGE): record 2p goes to out1, record 2p + 1 to out2; *len1, *len2 <= n + 1. */
int mk_fq_interleave(const uint8_t* text1, size_t n1, const uint8_t* text2, size_t n2, uint8_t* out, size_t cap, size_t* out_len,
                     size_t* npairs);
int mk_fq_split_pairs(const uint8_t* text, size_t n, uint8_t* out1, size_t cap1, size_t* len1, uint8_t* out2, size_t cap2,
                      size_t* len2, size_t* npairs);

/* ---- a decision applied to the FASTQ text it was taken for: the records mk_filter_*, mk_norm_* and mk_pairs_* keep and
 *      the lengths mk_trim_* leaves, written as FASTQ with their qualities (what khmer, BBDuk and BBNorm hand to an
 *      assembler, a mapper or a second correction pass) ----
 * Those calls read the FASTA view mk_fq2fa gives of a FASTQ text; record r there is record r here as long as every header
 * line starts with '@' (the first check below).  The decision arrays may come from them or from the caller.  The tables
 * are not read: the counting figures and the export stay untouched; an open chunk is MK_ERR_STATE as for the screen
 * calls; the stream is idle afterwards.
 * Lines and records: lines are fq2fa's -- split on '\n' only, numbered across the whole text; a last line without '\n' is
 * a line.  Record r is lines 4r .. 4r + 3.  The text must hold exactly nrec records, else MK_ERR_RANGE and the message
 * gives both counts (this is checked first).  The up to 3 lines behind the last complete record are tolerated only if
 * they are all empty; otherwise they are a malformed record (the text ends inside it).
 * Well-formedness, checked on the device for every record, emitted or not; a failure is MK_ERR_UNSUPPORTED, the message
 * names the lowest offending record index (over the whole call) and the first check it fails, in this order:
 *   line 4r starts with '@' (otherwise fq2fa drops that header and the FASTA view's record numbers no longer match);
 *   line 4r + 2 starts with '+';
 *   the sequence line 4r + 1 and the quality line 4r + 3 are equally long, one trailing '\r' not counted on either;
 *   only when kept is given: the sequence line, without its trailing '\r', holds no '*' and none of the bytes str.strip()
 *     removes (blank, tab, VT, FF, CR, 0x1C..0x1F) -- its bytes are then exactly the parser's kept characters that kept[r]
 *     counts;
 *   only when kept is given: kept[r] <= the sequence length L.  This one is MK_ERR_RANGE.
 * Selection: record r is emitted iff (keep == NULL or keep[r] == which) and (kept == NULL or kept[r] > 0).  which = 1 is
 * the main output, 2 the orphans of mk_pairs_*; any other value is MK_ERR_ARG; which is ignored when keep is NULL.  With
 * both arrays NULL the call validates and copies the whole text.
 * Output with kept == NULL: the emitted records in text order, each the bytes [start of line 4r, start of line 4r + 4)
 * byte for byte (CR LF stays CR LF); a last record without its final '\n' gets one, so that outputs can always be
 * concatenated.  Output with kept given: line 4r as it stands through its '\n'; the first kept[r] bytes of the sequence
 * line and one '\n'; line 4r + 2 as it stands through its '\n'; the first kept[r] bytes of the quality line and one '\n'
 * -- for an untrimmed LF-terminated record the input byte for byte.  *out_len <= n + 1 in both modes.
 * out = NULL, out_cap = 0 is the sizing call.  With out_cap too small: MK_ERR_RANGE, the needed size in *out_len, nothing
 * written past the buffer -- every piece is still walked to learn it.  On every other error *out_len = 0.  n == 0 with
 * nrec == 0 is success with empty output.  st may be NULL.
 * mk_fastq_select_text: host memory in and out, piece by piece: pieces end behind a line 4j once they hold piece_bytes
 * (mk_fastq_cuts; 0: the default, and the limits, of the screen calls; a record longer than that makes its piece grow);
 * each piece copies its own slice of keep and kept to the device.  Output, errors and the record indices in messages do
 * not depend on piece_bytes.
 * mk_fastq_select_device: everything in DEVICE memory of the context's GPU, one piece; text and out at any address,
 * d_kept aligned to 8 (MK_ERR_ARG otherwise). */
typedef struct mk_fastq_select_t {
  uint64_t records, records_out, records_trimmed; /* of the text; emitted; emitted with kept[r] below the sequence length */
  uint64_t bases_out, bytes_out, lines;           /* sequence bytes emitted; output bytes; lines of the text            */
  /* seconds: host time in the copies to the device (text, keep, kept); HIP-event time of the line index; of the checks,
   * the decision and its scan; of the gather; host time in the copies back */
  double s_copy, s_index, s_place, s_gather, s_write;
} mk_fastq_select_t;
int mk_fastq_select_text(mk_ctx* ctx, const uint8_t* fastq, size_t n, size_t piece_bytes,
                         const uint8_t* keep, const uint64_t* kept, size_t nrec, unsigned which,
                         uint8_t* out, size_t out_cap, size_t* out_len, mk_fastq_select_t* st);
int mk_fastq_select_device(mk_ctx* ctx, const uint8_t* d_fastq, size_t n,
                           const uint8_t* d_keep, const uint64_t* d_kept, size_t nrec, unsigned which,
                           uint8_t* d_out, size_t out_cap, size_t* out_len, mk_fastq_select_t* st);

/* ---- quality trimming and read filtering of a FASTQ text: the step MerCat2 hands to fastp, here as a stated rule -- the
 *      running-sum trimming of BWA -q and cutadapt -q 5',3' at both ends, then the span filters of fastp and cutadapt
 *      (length, N count, share of low-quality bases, mean quality) -- read, decided, cut and gathered on the GPU ----
 * Lines, records, the tolerated trailing empty lines and the checks are mk_fastq_select_*'s (no kept: the byte check of
 * the sequence line is not made), in that order, with one more behind them (kind 5): a byte of the quality line, one
 * trailing '\r' not counted, below phred_base ("its quality line holds a character below the phred base").  The lowest
 * record wins, then the lowest kind; all are MK_ERR_UNSUPPORTED.  The tables are not read; an open chunk is MK_ERR_STATE.
 * Trimming of a read of L bases, q[i] = qual[i] - phred_base, all sums signed 64-bit:
 *   5': s = best = start = 0; for i = 0 .. L-1: s += cut_front - q[i]; stop at the first s < 0; whenever s > best
 *       (strictly): best = s, start = i + 1.
 *   3': on the same untrimmed read: s = best = 0, stop = L; for i = L-1 .. 0: s += cut_back - q[i]; stop at the first
 *       s < 0; whenever s > best (strictly): best = s, stop = i.
 *   start >= stop: start = stop = 0.  kept = stop - start.  (A cutoff of 0 never trims; ties cut less.)
 * Filters over [start, stop), the first that applies names the reason: short: kept < max(min_len, 1); n: more than max_n
 * of the span's bases are 'N' or 'n'; lowq: low * 1000000 > max_low_ppm * kept, low = span bases with q < low_q (0: off);
 * meanq: qsum < min_mean_q * kept (0: off).  A record none drops passes.
 * paired: records 2p and 2p + 1 are mates (an odd count is MK_ERR_RANGE): keep[r] = 1 if both pass, 2 if only r passes,
 * 0 otherwise; unpaired keep[r] is the pass bit.  Record r is emitted iff keep[r] == which (1, or 2 with paired only).
 * Output, in text order: a record with start == 0 and kept == L whole, byte for byte (a forced '\n' where the text ends
 * without one); any other as the header line as it stands, seq[start:stop] and '\n', the '+' line as it stands,
 * qual[start:stop] and '\n'.  rows[r] (every record): length, start, kept, n, low, qsum (the last three over the span).
 * hist[v]: bases of quality value v over all records; hist[256 + v]: over the emitted spans.
 * cap: the records keep and rows have room for; a text with more is MK_ERR_RANGE with the count in *nrec (checked first;
 * not when both are NULL).  keep, rows, hist may each be NULL.  out = NULL, out_cap = 0 is the sizing call; out_cap too
 * small is MK_ERR_RANGE with the needed size in *out_len (keep, rows and hist are then complete); on every other error
 * *out_len = 0.  *out_len <= n + 1.
 * mk_fastq_qtrim_text: host memory, piece by piece as mk_fastq_select_text (with paired a piece ends behind an even
 * record: mk_fastq_pair_cuts); nothing depends on piece_bytes.  mk_fastq_qtrim_device: everything in DEVICE memory of
 * the context's GPU, one piece of at most 2^32 - 1 bytes (more: MK_ERR_RANGE, before anything is read; the text call's
 * pieces are smaller); text and out at any address, d_rows and d_hist aligned to 8 (MK_ERR_ARG otherwise). */
typedef struct mk_qtrim_opt_t {
  uint32_t phred_base;          /* 33 or 64 (else MK_ERR_ARG)                                                          */
  uint32_t cut_front, cut_back; /* 0 .. 93; 0: that end is not trimmed                                                 */
  uint32_t min_len, max_n;      /* max_n ~0: no limit                                                                  */
  uint32_t low_q, max_low_ppm;  /* max_low_ppm 0 .. 1000000                                                            */
  uint32_t min_mean_q;
  uint32_t paired, which;
} mk_qtrim_opt_t;
typedef struct mk_fastq_qtrim_t {
  uint64_t records, records_out, records_trimmed; /* of the text; emitted; emitted and cut                             */
  uint64_t dropped_short, dropped_n, dropped_lowq, dropped_meanq; /* records by the filter that dropped them           */
  uint64_t orphans;                               /* records with keep[r] == 2                                         */
  uint64_t bases_in, bases_out, bytes_out, lines; /* sequence bytes of the text; emitted; output bytes; lines          */
  /* seconds: host time in the copies to the device; HIP-event time of the line index; of the quality scan; of the
   * decision and its prefix sum; of the gather; host time in the copies back */
  double s_copy, s_index, s_scan, s_place, s_gather, s_write;
} mk_fastq_qtrim_t;
int mk_fastq_qtrim_text(mk_ctx* ctx, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_qtrim_opt_t* opt, size_t cap,
                        uint8_t* keep, uint64_t* rows, uint64_t* hist, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                        mk_fastq_qtrim_t* st);
int mk_fastq_qtrim_device(mk_ctx* ctx, const uint8_t* d_fastq, size_t n, const mk_qtrim_opt_t* opt, size_t cap, uint8_t* d_keep,
                          uint64_t* d_rows, uint64_t* d_hist, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec,
                          mk_fastq_qtrim_t* st);

/* ---- 3' adapter removal from the reads of a FASTQ text: the first job of the fastp run MerCat2 starts, here as a stated
 *      rule -- the 3' adapter search of cutadapt -a ... --no-indels, reduced to the leftmost admissible position -- read,
 *      decided, cut and gathered on the GPU.  Qualities are carried along and never interpreted ----
 * Lines, records, the tolerated trailing empty lines, the checks and their messages are mk_fastq_select_*'s without kept
 * ('@', '+', equal lengths, a text that ends inside a record); all MK_ERR_UNSUPPORTED, the lowest record wins.  The tables
 * are not read; an open chunk is MK_ERR_STATE.
 * Adapters: A of them, 1 .. 1024, each of 1 .. 128 bases over ACGTN (lower case folded; any other byte is MK_ERR_ARG and
 * the message names the adapter), bases[] their characters back to back, lengths[a] their lengths, mates[a] their mate
 * class: 1 first mates and unpaired reads, 2 second mates, 3 both (mates == NULL: all 1).  Without paired every record
 * is of class 1; with paired record 2p is of class 1 and record 2p + 1 of class 2.
 * A read's sequence line content s has L bytes (one trailing '\r' taken off), a .. z folded to upper case; a byte that is
 * then none of A, C, G, T mismatches every adapter base but N; an adapter N matches any byte.  For position i in 0 .. L-1
 * and adapter a of m bases: ov = min(m, L - i); mism = the number of j < ov with adapter[j] != 'N' and adapter[j] !=
 * fold(s[i + j]); a is admissible at i iff its class covers the record, ov >= min_overlap and mism * 1000000 <=
 * max_err_ppm * ov (64-bit integers).  The hit is the smallest i that has an admissible adapter, and of those admissible
 * there the lowest index.  cut = i, or L without a hit; the read keeps s[:cut] and qual[:cut].  A read with cut <
 * max(min_len, 1) is dropped as short.  paired, which and keep[r] are mk_fastq_qtrim_*'s: keep[r] = 1 if both mates pass, 2
 * if only r passes, 0 otherwise (unpaired: the pass bit); record r is emitted iff keep[r] == which; an odd record count
 * with paired is MK_ERR_RANGE.
 * Output, in text order: a record with cut == L whole, byte for byte (a forced '\n' where the text ends without one); any
 * other as the header line as it stands, s[:cut] and '\n', the '+' line as it stands, qual[:cut] and '\n'.
 * rows[r] (every record, five uint64): length, kept, adapter, overlap, mismatches -- adapter the index of the hit, or
 * 0xFFFFFFFF with overlap = mismatches = 0.  hits[a] (A uint64): the records whose hit is adapter a, emitted or not.
 * cap, the sizing call, out_cap too small, *nrec, *out_len, the order of the errors and NULL keep / rows / hits are
 * mk_fastq_qtrim_*'s (options, then the panel, are checked first).  mk_fastq_adapt_device: one piece of at most 2^32 - 1
 * bytes, text and out at any address, d_rows and d_hits aligned to 8 (MK_ERR_ARG otherwise); bases, lengths and mates are
 * host memory in both calls.
 * mk_adapters_pack: host code, no GPU: validates the adapters and writes the packed panel the scan kernel reads, 1 + 9 A
 * 64-bit words (*nwords; words = NULL sizes; words_cap too small is MK_ERR_RANGE; err, if given, receives the message):
 *   words[0] = A; adapter a is the nine words at 1 + 9 a:
 *   [0]      length (bits 0 .. 7) | class << 8 | first << 32 -- first: the lowest index of an adapter with the same bases
 *            (after folding) and the same class, a itself if there is none before it; the kernel compares only those with
 *            first == a, which leaves the reported index the lowest
 *   [1..4]   codes: base j is the two bits at 2 (j % 32) of word 1 + j / 32: A 0, C 1, G 2, T 3 (N: 0)
 *   [5..8]   the wildcard plane, inverted ("care"): bit 2 (j % 32) of word 5 + j / 32 is set iff base j is not N
 *   all bits behind the adapter's last base are 0. */
typedef struct mk_adapt_opt_t {
  uint32_t min_overlap; /* 1 .. 128 (else MK_ERR_ARG)                                                                  */
  uint32_t max_err_ppm; /* 0 .. 1000000                                                                                */
  uint32_t min_len, paired, which;
} mk_adapt_opt_t;
typedef struct mk_fastq_adapt_t {
  uint64_t records, records_out, records_trimmed; /* of the text; emitted; emitted and cut                             */
  uint64_t dropped_short, orphans;                /* records dropped as short; records with keep[r] == 2               */
  uint64_t bases_in, bases_out, bytes_out, lines; /* sequence bytes of the text; emitted; output bytes; lines          */
  /* seconds: host time in the copies to the device; HIP-event time of the line index; of the adapter scan; of the
   * decision and its prefix sum; of the gather; host time in the copies back */
  double s_copy, s_index, s_scan, s_place, s_gather, s_write;
} mk_fastq_adapt_t;
int mk_adapters_pack(const uint8_t* bases, const uint32_t* lengths, const uint8_t* mates, size_t A, uint64_t* words, size_t words_cap,
                     size_t* nwords, char* err, size_t err_cap);
int mk_fastq_adapt_text(mk_ctx* ctx, const uint8_t* fastq, size_t n, size_t piece_bytes, const uint8_t* bases, const uint32_t* lengths,
                        const uint8_t* mates, size_t A, const mk_adapt_opt_t* opt, size_t cap, uint8_t* keep, uint64_t* rows,
                        uint64_t* hits, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec, mk_fastq_adapt_t* st);
int mk_fastq_adapt_device(mk_ctx* ctx, const uint8_t* d_fastq, size_t n, const uint8_t* bases, const uint32_t* lengths,
                          const uint8_t* mates, size_t A, const mk_adapt_opt_t* opt, size_t cap, uint8_t* d_keep, uint64_t* d_rows,
                          uint64_t* d_hits, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec, mk_fastq_adapt_t* st);

/* ---- mate-overlap detection in paired reads: the other half of the fastp run MerCat2 starts -- panel-free adapter removal
 *      (mode 0) and merging of overlapping mates into one read (mode 1; fastp -m, PEAR, BBMerge) -- here as a stated rule,
 *      which is not fastp's: read, decided, cut or merged and gathered on the GPU.  Quality bytes are compared as bytes: no
 *      phred base is involved ----
 * The text is interleaved FASTQ: records 2p and 2p + 1 are mates, by position; an odd count is MK_ERR_RANGE.  Lines,
 * records, the tolerated trailing empty lines, the checks and their messages are mk_fastq_select_*'s without kept ('@',
 * '+', equal lengths, a text that ends inside a record); all MK_ERR_UNSUPPORTED, the lowest record wins.  The tables are
 * not read; an open chunk is MK_ERR_STATE.
 * Notation: s1, q1 (L1 bytes) and s2, q2 (L2 bytes) are the contents of the mates' sequence and quality lines (one
 * trailing '\r' taken off); fold maps a .. z to upper case; comp maps A <-> T and C <-> G on folded bytes and anything else
 * to N; rc[j] = comp(fold(s2[L2 - 1 - j])), rq[j] = q2[L2 - 1 - j].
 * Candidates: an offset d puts rc[j] under s1[d + j].  Fragment length F = d + L2; overlap = mate-1 positions [max(d, 0),
 * min(L1, F)), ov of them; mm = the overlap positions p at which fold(s1[p]) and rc[p - d] are not both of ACGT and equal
 * (an N in either mate is a mismatch).  d is admissible iff ov >= min_overlap and mm <= max_mismatch and mm * 1000000 <=
 * max_err_ppm * ov (integers).  Order: d = 0, 1, 2, ... while ov >= min_overlap, then d = -1, -2, ... while ov >=
 * min_overlap; the first admissible candidate is the hit (the order of fastp's overlap analysis: the longest overlap of
 * mates that do not read through first, then read-through).  fastp's defaults are min_overlap 30, max_mismatch 5,
 * max_err_ppm 200000.  A pair with L1 or L2 above MK_OVERLAP_MAX_BASES is not tested: it has no hit and counts in
 * skipped_long.
 * rows[r] (every record, five uint64, the same in both modes): length, kept, fragment, overlap, mismatches.  With a hit
 * kept = min(length, F) and the last three are equal for both mates; without one kept = length, fragment = 0xFFFFFFFF,
 * overlap = mismatches = 0.
 * mode 0 (trim): with a hit each mate is cut to its first kept bases (mate 2's adapter is at its 3' end too).  A pair
 * with a hit and F < max(min_len, 1) is dropped: keep = 0 for both mates (dropped_short); every other pair has keep = 1.
 * which must be 1.  Output: both mates of every kept pair, in text order: an uncut record whole, byte for byte (a forced
 * '\n' where the text ends without one), a cut record as mk_fastq_adapt_* emits one (the header line as it stands,
 * s[:kept] and '\n', the '+' line as it stands, qual[:kept] and '\n').
 * mode 1 (merge): a pair with a hit and F >= max(min_len, 1) is merged: keep = 1 for both mates; with a hit and a shorter
 * F it is dropped: keep = 0 (dropped_short); without a hit keep = 2.  which = 1 writes one record a merged pair: mate 1's
 * header line as it stands, the merged sequence and '\n', mate 1's '+' line as it stands, the merged quality and '\n'.
 * which = 2 writes both mates of every keep == 2 pair, byte for byte (the forced '\n' as above).  The merged read covers
 * positions p in [0, F):
 *   p < d: s1[p], q1[p];   p >= L1: rc[p - d], rq[p - d];
 *   in the overlap, the folded bytes equal and of ACGT: s1[p] as it stands with the larger of the two quality bytes;
 *   in the overlap otherwise: a byte of ACGT (after folding) wins over one that is not, then the higher quality byte
 *   wins, then mate 1; the winner's base (s1[p] as it stands, or rc[p - d]) goes out with its own quality.
 * Figures: pairs = records / 2; pairs_hit; pairs_merged (mode 1: keep 1), pairs_trimmed (mode 0: kept pairs with a hit
 * of which a mate was cut); dropped_short, skipped_long (pairs); records_out, records_trimmed (emitted; emitted and not
 * byte for byte: cut, or merged), bases_in (all records), bases_out (emitted).
 * cap, the sizing call (out = NULL, out_cap = 0), out_cap too small (MK_ERR_RANGE with the needed size in *out_len, keep
 * and rows complete), *nrec, the order of the errors (options first) and NULL keep / rows are mk_fastq_adapt_*'s.
 * *out_len <= n + 1 in both modes.  mk_fastq_overlap_text: host memory, piece by piece; pieces end behind a line 8j
 * (mk_fastq_pair_cuts), nothing depends on piece_bytes.  mk_fastq_overlap_device: everything in DEVICE memory, one piece
 * of at most 2^32 - 1 bytes (more: MK_ERR_RANGE before anything is read), text and out at any address, d_rows aligned to
 * 8 (MK_ERR_ARG otherwise).  d_fastq is never modified: a merging call (mode 1, which 1) works on a copy of its own, whose
 * time is in s_copy.
 * MK_ERR_ARG: mode not 0 / 1; min_overlap outside 1 .. MK_OVERLAP_MAX_BASES; max_err_ppm above 1000000; which not 1,
 * except 2 with mode 1. */
#define MK_OVERLAP_MAX_BASES 512
typedef struct mk_overlap_opt_t {
  uint32_t mode;         /* 0 trim, 1 merge                                                                            */
  uint32_t min_overlap;  /* 1 .. MK_OVERLAP_MAX_BASES                                                                  */
  uint32_t max_mismatch; /* mismatches an overlap may hold                                                             */
  uint32_t max_err_ppm;  /* 0 .. 1000000: and per million overlap bases                                                */
  uint32_t min_len, which;
} mk_overlap_opt_t;
typedef struct mk_fastq_overlap_t {
  uint64_t records, pairs, pairs_hit, pairs_merged, pairs_trimmed, dropped_short, skipped_long;
  uint64_t records_out, records_trimmed, bases_in, bases_out, bytes_out, lines;
  /* seconds: host time in the copies to the device (and the device call's own copy of a text it merges in); HIP-event
   * time of the line index; of the pair scan; of the decision, the merge writer and the prefix sum; of the gather; host
   * time in the copies back */
  double s_copy, s_index, s_scan, s_place, s_gather, s_write;
} mk_fastq_overlap_t;
int mk_fastq_overlap_text(mk_ctx* ctx, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_overlap_opt_t* opt, size_t cap,
                          uint8_t* keep, uint64_t* rows, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                          mk_fastq_overlap_t* st);
int mk_fastq_overlap_device(mk_ctx* ctx, const uint8_t* d_fastq, size_t n, const mk_overlap_opt_t* opt, size_t cap, uint8_t* d_keep,
                            uint64_t* d_rows, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec, mk_fastq_overlap_t* st);

/* ---- per-cycle quality control of a FASTQ text: the figures MerCat2 asks fastqc for, before and after trimming -- where
 *      along the read the quality falls and the base composition drifts, and per read its length, mean quality and GC
 *      share -- reduced on the GPU from the text, as a stated rule.  No plots, no duplication or over-represented
 *      sequences, no adapter or k-mer content, no position grouping and no verdicts: nothing here is fastqc's number ----
 * Lines, records and the tolerated trailing empty lines are mk_fastq_qtrim_*'s; one trailing '\r' is taken off the
 * sequence line and off the quality line, as there.  The checks are its own, in its order: '@', '+', equal lengths, a text
 * that ends inside a record, and kind 5: a byte of the quality line below phred_base ("its quality line holds a character
 * below the phred base").  The lowest record wins, then the lowest kind; all are MK_ERR_UNSUPPORTED with the same
 * phrases.  No table is read; an open chunk is MK_ERR_STATE.
 * Options: phred_base 33 or 64; max_pos = P in 1 .. MK_QC_MAX_POS; paired 0 or 1; anything else is MK_ERR_ARG.  With
 * paired, record r belongs to class c = r & 1 and an odd record count is MK_ERR_RANGE; without, c = 0.  C = the number of
 * classes, 1 or 2.
 * Base i of a record of L bases has q[i] = qual[i] - phred_base (>= 0; a negative value is the kind-5 error), the bin
 * v[i] = min(q[i], MK_QC_QBINS - 1), the base class b[i] of seq[i] | 0x20: 'a' 0, 'c' 1, 'g' 2, 't' 3, 'n' 4, anything
 * else 5, and the row p[i] = min(i, P): row P collects every cycle from P on.
 * The tables, all uint64, exact, zeroed by the call, all required (a NULL one is MK_ERR_ARG):
 *   pos_qual[c][p][v]   C x (P + 1) x 96: bases of class c, row p, quality bin v
 *   pos_base[c][p][k]   C x (P + 1) x 8: bases of class c, row p, base class k; columns 6 and 7 stay 0
 *   read_len[c][l]      C x (P + 2): records of length l for l <= P; index P + 1: the records longer than P
 *   read_qual[c][m]     C x 96: records with L > 0 by m = min(qsum / L, 95), integer division, qsum = the sum of the
 *                       unclipped q[i]
 *   read_gc[c][g]       C x 101: records with L > 0 by g = (200 gc + L) / (2 L), integer division (rounds half up), gc =
 *                       the bases of class 1 or 2
 * rows[r], optional (NULL: none): four uint64 a record: length, qsum, gc, n (the bases of class 4).  cap: the records rows
 * has room for; a text with more is MK_ERR_RANGE with the count in *nrec (checked first; not when rows is NULL).
 * mk_fastq_qc_t: min_len and max_len per class, both 0 for a class without records.
 * mk_fastq_qc_text: host memory, piece by piece (with paired a piece ends behind an even record: mk_fastq_pair_cuts); the
 * tables are accumulated on the device over all pieces and copied back once; nothing depends on piece_bytes.
 * mk_fastq_qc_device: everything in DEVICE memory of the context's GPU (the mk_qc_out_t itself is host memory, its
 * pointers device memory), one piece of at most 2^32 - 1 bytes (more: MK_ERR_RANGE, before anything is read); the text at
 * any address, the tables and rows aligned to 8 (MK_ERR_ARG otherwise).  Both leave the tables unspecified on any error. */
#define MK_QC_MAX_POS 16384
#define MK_QC_QBINS 96
typedef struct mk_qc_opt_t {
  uint32_t phred_base; /* 33 or 64 (else MK_ERR_ARG) */
  uint32_t max_pos;    /* P: 1 .. MK_QC_MAX_POS      */
  uint32_t paired;     /* 0 or 1                     */
} mk_qc_opt_t;
typedef struct mk_qc_out_t {
  uint64_t* pos_qual;
  uint64_t* pos_base;
  uint64_t* read_len;
  uint64_t* read_qual;
  uint64_t* read_gc;
  uint64_t* rows; /* or NULL */
} mk_qc_out_t;
typedef struct mk_fastq_qc_t {
  uint64_t records, lines, bases; /* of the text; bases: sequence bytes */
  uint64_t min_len[2], max_len[2];
  /* seconds: host time in the copies to the device; HIP-event time of the line index; of the per-read kernel; of the
   * per-cycle kernel; host time in the copies back */
  double s_copy, s_index, s_reads, s_cycles, s_write;
} mk_fastq_qc_t;
int mk_fastq_qc_text(mk_ctx* ctx, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_qc_opt_t* opt, size_t cap,
                     const mk_qc_out_t* out, size_t* nrec, mk_fastq_qc_t* st);
int mk_fastq_qc_device(mk_ctx* ctx, const uint8_t* d_fastq, size_t n, const mk_qc_opt_t* opt, size_t cap, const mk_qc_out_t* d_out,
                       size_t* nrec, mk_fastq_qc_t* st);

/* ---- duplicate reads of a FASTQ text: what fastp --dedup, clumpify dedupe and seqkit rmdup -s remove and fastqc's
 *      duplication levels report, here as a stated rule -- reads (or pairs) whose key BYTES are equal form a cluster, the
 *      one of lowest index stays -- found, decided and gathered on the GPU.  Exact: a hash only chooses where to look ----
 * Lines, records, the tolerated trailing empty lines, the one trailing '\r' taken off the sequence and quality lines and
 * the checks with their messages are mk_fastq_qtrim_*'s without kind 5 (qualities are never interpreted): '@', '+', equal
 * lengths, a text that ends inside a record.  The lowest record wins, then the lowest kind; all are MK_ERR_UNSUPPORTED.
 * The tables are not read; an open chunk is MK_ERR_STATE.
 * Key of a read of L bases: the bytes seq[0 : L] with prefix = 0, else seq[0 : min(L, prefix)], as they stand ('a' is not
 * 'A', 'N' is a byte like any other, no reverse complement).  An empty read has the empty key.
 * Unit: unpaired the record, its key the read's; paired the pair (2p, 2p + 1), its key the ordered pair of the mates' keys
 * (equal iff both first mates and both second mates are equal, lengths included; an odd record count is MK_ERR_RANGE).
 * Units with equal keys form a cluster; its first is the unit of lowest index over the whole call, its copies its size.
 * rows[r] = {L, first}: first = the record that plays r's part in the first unit of r's cluster (r itself for a first
 * occurrence; paired 2p' + (r & 1)).  keep[r] = 1 iff first == r, else 0.  Record r is emitted iff keep[r] == 1 with
 * which = 1 (the uniques) or keep[r] == 0 with which = 2 (the duplicates); any other which is MK_ERR_ARG.
 * Output, in text order: the emitted records whole, byte for byte (a forced '\n' where the text ends without one).
 * levels[high + 2], zeroed by the call: levels[i] = clusters of i copies for 1 <= i <= high, levels[high + 1] = those of
 * more, levels[0] = 0.  high in 1 .. MK_DEDUP_MAX_HIGH (else MK_ERR_ARG).
 * cap, *nrec, the sizing call (out = NULL, out_cap = 0), MK_ERR_RANGE with the needed size in *out_len, *out_len <= n + 1:
 * mk_fastq_qtrim_*'s.  keep, rows and levels may each be NULL.
 * mk_fastq_dedup_text: host memory, piece by piece (with paired a piece ends behind an even record); the text of all pieces
 * stays on the device for the length of the call (a copy in the last piece may equal a read of the first), so the call
 * needs about n bytes and 64 to 112 more a record of device memory; a failed allocation is MK_ERR_NOMEM and the message
 * gives the bytes.  Nothing depends on piece_bytes, on scheduling or on the hash function: two runs give identical bytes.
 * mk_fastq_dedup_device: everything in DEVICE memory of the context's GPU, one piece of at most 2^32 - 1 bytes (more:
 * MK_ERR_RANGE, before anything is read); text and out at any address, d_rows and d_levels aligned to 8 (MK_ERR_ARG
 * otherwise).  The text is never written. */
#define MK_DEDUP_MAX_HIGH (1u << 20)
typedef struct mk_dedup_opt_t {
  uint32_t prefix; /* 0: whole reads; else the first `prefix` bases are the key */
  uint32_t paired; /* 0 or 1                                                    */
  uint32_t which;  /* 1: emit the uniques; 2: emit the duplicates               */
  uint32_t high;   /* 1 .. MK_DEDUP_MAX_HIGH                                    */
} mk_dedup_opt_t;
typedef struct mk_fastq_dedup_t {
  uint64_t records, records_out;  /* of the text; emitted                                                              */
  uint64_t distinct, duplicates;  /* clusters (pairs with paired); records with keep[r] == 0                           */
  uint64_t max_copies, slots;     /* the largest cluster, in units; slots of the call's table                          */
  uint64_t probes, compares;      /* diagnostics: probe steps beyond the first; key bytes compared                     */
  uint64_t bases_in, bases_out, bytes_out, lines; /* sequence bytes of the text; emitted; output bytes; lines          */
  /* seconds: host time counting lines and sizing the call's state; host time in the copies to the device; HIP-event time
   * of the line index; of keys and inserts together, and of each; of the decision and its prefix sum; of the gather; of
   * the pass over the table; host time in the copies back */
  double s_plan, s_copy, s_index, s_scan, s_key, s_insert, s_place, s_gather, s_levels, s_write;
} mk_fastq_dedup_t;
int mk_fastq_dedup_text(mk_ctx* ctx, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_dedup_opt_t* opt, size_t cap,
                        uint8_t* keep, uint64_t* rows, uint64_t* levels, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                        mk_fastq_dedup_t* st);
int mk_fastq_dedup_device(mk_ctx* ctx, const uint8_t* d_fastq, size_t n, const mk_dedup_opt_t* opt, size_t cap, uint8_t* d_keep,
                          uint64_t* d_rows, uint64_t* d_levels, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec,
                          mk_fastq_dedup_t* st);

/* ---- several samples side by side: merge_tsv (lib/mercat2_report.py:98-156) from the tables --- */
/* The combined table of n samples (contexts with the same k; each on its own GPU or all on one):
 * every k-mer present in any of them, in sorted(str) order, with its count in each sample (0 where
 * absent).  kmers: rows*k bytes, matrix: rows*n counts, row-major, both caller-allocated; call with
 * kmers = matrix = NULL to get *rows. */
int mk_merged_export(mk_ctx* const* ctxs, int n, uint8_t* kmers, uint64_t* matrix, size_t rows_cap, size_t* rows);
/* The same as the file merge_tsv writes: "<first_column>\t<names[0]>\t...\n" then one line per k-mer.
 * names are the column titles, in the order of ctxs (the reference sorts the sample names). */
int mk_write_merged_tsv(mk_ctx* const* ctxs, int n, const char* const* names, const char* first_column,
                        const char* path, size_t* rows);
/* The same file with the rows exactly as merge_tsv's streaming loop produces them: that loop looks for the next k-mer
 * only among the samples that advanced in the current step and writes a sample's pending count under the k-mer at
 * hand whenever its own key is not greater (lib/mercat2_report.py:131-150), so a key held only by samples that did
 * not advance gets no row of its own and its count lands in a later row.  Tables that share (nearly) all their keys
 * -- k = 5 over genomes, the reference's committed runs -- come out the same either way. */
int mk_write_merged_tsv_as_reference(mk_ctx* const* ctxs, int n, const char* const* names, const char* first_column,
                                     const char* path, size_t* rows);
/* merge_tsv_T (lib/mercat2_report.py:160-194), the transposed table beta diversity reads (bin/mercat2.py:354-355):
 * "sample\t<k-mer>\t...\n", then "<names[s]>\t<count>...\n" per sample.  The reference orders the k-mer columns
 * as a Python set iterates (not reproducible); here they are in sorted(str) order.  *rows = k-mer columns. */
int mk_write_merged_tsv_t(mk_ctx* const* ctxs, int n, const char* const* names, const char* path, size_t* rows);
/* ---- sample PCA (MerCat2 -pca, lib/mercat2_figures.py:206-291): the exact Gram matrix the host centres and
 *      decomposes (mercat2_amd/pca.py) ------------------------------------------------------------------------ */
/* Exact Gram matrix of n samples' count columns over the union of their k-mers (X X^T, X = the table
 * mk_merged_export gives without as_reference).  gram: n*n pairs of uint64 {lo, hi} (128-bit), row-major.
 * Same k, alphabet and canonical mode; contexts on any devices (joined on ctxs[0]'s device); 1 <= n <= 4096.
 * slab_rows: cap on the union rows held on the device at once (0 = pick from free memory).
 * *rows = union rows (n_features). */
int mk_gram(mk_ctx* const* ctxs, int n, size_t slab_rows, uint64_t* gram, size_t* rows);
/* The same for a dense rows x n uint64 matrix in host memory (row-major, as mk_merged_export returns it).
 * Errors: mk_last_error(NULL). */
int mk_gram_matrix(int device, const uint64_t* matrix, size_t rows, int n, uint64_t* gram);
/* ---- beta diversity (lib/mercat2_diversity.py:56-105: scipy's pdist of the dense combined_<type>_T.tsv, 21
 *      metrics): the per-pair reductions every metric is a closed form of (mercat2_amd/diversity.py) ---------- */
/* Statistics of the pair (x, y) of two samples' count columns over the d union rows.  The diagonal (x = y) has
 * dot = Q_i (sum of squares), both = z_i (rows with a count above zero), everything else 0. */
typedef struct mk_pair_t {
  uint64_t dot[2]; /* sum x*y, 128-bit {lo, hi} */
  uint64_t l1[2];  /* sum |x - y|, 128-bit {lo, hi} */
  uint64_t cheb;   /* max |x - y| */
  uint64_t neq;    /* rows with x != y */
  uint64_t both;   /* rows with x != 0 and y != 0 */
  double canb;     /* sum over rows with x + y > 0 of |x - y| / (x + y), in f64 as scipy computes it */
  double seuc;     /* sum (x - y)^2 / V_r, V_r = variance of row r's n counts (ddof = 1), in f64 */
} mk_pair_t;
#define MK_PAIR_CONSTANT_ROW 1u /* flags: some union row holds the same count in all n samples (V_r = 0) */
/* out: n*n mk_pair_t, both triangles; sums: n pairs of uint64 {lo, hi}, the 128-bit column sums S_i; *rows = union
 * rows (d); *flags: MK_PAIR_CONSTANT_ROW.  Same contexts, join and slab_rows as mk_gram; counts below 2^63.
 * Integer fields do not depend on slab_rows, launch shape or device; f64 fields are reduced in a fixed order
 * (the same bits for the same input, device and slab_rows). */
int mk_pair_stats(mk_ctx* const* ctxs, int n, size_t slab_rows, mk_pair_t* out, uint64_t* sums, size_t* rows,
                  uint64_t* flags);
/* The same for a dense rows x n uint64 matrix in host memory (row-major).  Errors: mk_last_error(NULL). */
int mk_pair_stats_matrix(int device, const uint64_t* matrix, size_t rows, int n, mk_pair_t* out, uint64_t* sums,
                         uint64_t* flags);
/* ---- alpha diversity of a sample: the moments of its count column (lib/mercat2_diversity.py:13-53
 *      computes nine scikit-bio metrics from exactly these), reduced on the GPU ------------------
 * A row is a key whose count is not zero.  The integer fields are exact, total modulo 2^64.  sum_sq is added up in
 * integers (192 bits: no table can overflow them) and converted once.  sum_clnc is a float64 sum of fl(c) * ln(fl(c))
 * in an order the table's layout fixes and no launch changes -- no floating-point atomics: an unchanged table answers
 * with the same bits every time; within (rows + 8) * 2^-53 of the true sum, relative, whatever the layout.
 * A sharer (mk_share_table) answers for its OWN tables, the owner for every row its table holds. */
typedef struct mk_alpha_t {
  uint64_t observed; /* rows (distinct k-mers)                                   */
  uint64_t total;    /* sum of the counts, modulo 2^64                           */
  uint64_t freq[11]; /* freq[i], i = 1..10: rows whose count is i (freq[0] unused) */
  double sum_sq;     /* sum of count^2: exact, rounded once                      */
  double sum_clnc;   /* sum of count * ln(count): same table, same bits          */
} mk_alpha_t;
int mk_alpha_stats(mk_ctx* ctx, mk_alpha_t* out);

/* Free the per-chunk working memory of a context and keep its running table (for samples that wait
 * for mk_merged_export while others are being counted). */
int mk_trim(mk_ctx* ctx);

/* ---- multi-GPU merge plumbing (replaces ray.get + dict sum across workers) -------------- */
/* Packed-key view of the running table for exchange over RCCL: *rows entries sorted by key
 * into caller-provided DEVICE buffers.  d_keys holds mk_words_per_key(ctx) 64-bit words per row,
 * row after row (1 for dense/hash64; 2 for hash128: {hi, lo}, hi = bases 0..31, lo = the rest,
 * both left-aligned, so (hi, lo) order is the byte order of the k-mer text); cap counts rows.
 * By-reference (exotic) rows are exchanged through mk_export_exotic / mk_import_exotic. */
int mk_export_pairs_device(mk_ctx* ctx, uint64_t* d_keys, uint64_t* d_counts, size_t cap, size_t* rows);
/* insert-add (key,count) pairs from DEVICE buffers into the running table (same layout; the same key
 * may come more than once, e.g. rows received from several ranks). */
int mk_import_pairs_device(mk_ctx* ctx, const uint64_t* d_keys, const uint64_t* d_counts, size_t rows);
int mk_export_exotic(mk_ctx* ctx, uint8_t* kmers, uint64_t* counts, size_t cap, size_t* rows);
int mk_import_exotic(mk_ctx* ctx, const uint8_t* kmers, const uint64_t* counts, size_t rows);
int mk_words_per_key(const mk_ctx* ctx);
/* Add every row of src's running table into dst's (both on the same GPU, same alphabet, k and
 * canonical mode); src is left unchanged.  Lets a host deal the chunks of one sample to several
 * contexts (= HIP streams) that count concurrently and sum them at the end, on the device. */
int mk_merge_from(mk_ctx* dst, mk_ctx* src);

/* Several contexts of ONE GPU, one running table (round 4): from now on the count kernels of ctx put the survivors of its
 * chunks straight into owner's table (fused launches, one-word keys; whatever ctx still merges on its own -- a new
 * context's first chunk, rows kept as text -- stays in ctx's table).  Sum as before at the end: mk_merge_from(owner, ctx)
 * now finds little to add.  owner == NULL: ctx goes back to its own table.  Same GPU, alphabet, k, canonical mode; one
 * level deep.  The caller orders mk_reset(owner) against the sharers' chunks (reset the owner first). */
int mk_share_table(mk_ctx* ctx, mk_ctx* owner);

/* ---- one process, several GPUs: the Ray fan-out of a sample's chunks over workers and the dict sum of their
 *      results (bin/mercat2.py:119-127, 336-339) with the workers being the GPUs of one node ------------- */
/* Equal key ranges: bounds[i-1] = first key (first 64-bit word of the packed key, key_bits wide: bits*k for
 * one-word keys, 64 for two-word keys) owned by owner i, i = 1..n-1; owner 0 starts at 0.  Host helper. */
int mk_owner_bounds(int key_bits, int n, uint64_t* bounds);
/* The order in which to create contexts for ndev devices with `streams` contexts each, so that mk_count_file's
 * rule "chunk i goes to ctxs[i mod nctx]" sends chunk i to device devices[i mod ndev] and successive
 * chunks of one device to its different streams: ctx_device[j] = devices[j mod ndev], j < ndev*streams.  Host helper. */
int mk_plan_contexts(const int* devices, int ndev, int streams, int* ctx_device);
/* The rows of the running table grouped by owner (owner of a row = number of bounds <= the first word of its
 * key; n owners, n-1 ascending bounds), written to the DEVICE buffer d_rows as interleaved rows of
 * mk_words_per_key()+1 words {key word(s), count}, owner after owner; counts[j] (HOST, n values) = rows of owner j.
 * One pass for the histogram, one for the rows: no sort.  d_rows == NULL: only the counts.  The table is unchanged.
 * Dense bins travel as {bin, count}; rows kept as text are not included (mk_export_exotic). */
int mk_bucket_rows_device(mk_ctx* ctx, const uint64_t* bounds, int n, uint64_t* d_rows, size_t cap_rows, uint64_t* counts);
/* insert-add interleaved rows (that layout) from a DEVICE buffer of this context's GPU into the running table. */
int mk_import_rows_device(mk_ctx* ctx, const uint64_t* d_rows, size_t rows);

/* About one in `stride` rows of the running table -- the first word of their keys, in no order -- into the HOST
 * buffer out (cap values; *n = how many): the sample owner bounds with about equal rows per owner are made of
 * (SURVEY 8e "optionally sampled splitters").  The table is hashed, so every stride-th slot is a uniform sample. */
int mk_sample_keys(mk_ctx* ctx, size_t stride, uint64_t* out, size_t cap, size_t* n);
/* Dense mode (k * bits <= 15): the bins as one array of nbins = 4^k / 32^k counts, copied out to (store = 0) or in
 * from (store != 0) a DEVICE buffer of this context's GPU -- several GPUs sum dense tables with one reduce of that
 * array instead of exchanging rows. */
int mk_dense_bins_device(mk_ctx* ctx, uint64_t* d_bins, size_t nbins, int store);

#define MK_MERGE_RANGES 0   /* afterwards ctxs[i] holds exactly the rows of key range i: the concatenation of the
                               contexts' sorted exports, in order, is the sorted table (mk_*_multi below)        */
#define MK_MERGE_GATHER 1   /* afterwards ctxs[0] holds every row and the others are empty                        */
#define MK_MERGE_BALANCED 2 /* (with RANGES) owner bounds from a sample of the keys (about equal rows per owner)
                               instead of equal key ranges                                                        */
#define MK_MERGE_RCCL 4     /* the segments travel by grouped ncclSend / ncclRecv (RCCL over xGMI; one communicator per
                               GPU, made on first use) instead of peer copies; MK_ERR_UNSUPPORTED when librccl.so cannot
                               be loaded                                                                          */
typedef struct mk_merge_stats_t {
  uint64_t rows_in;      /* rows of all contexts before the merge (the same key counted once per context) */
  uint64_t rows_out;     /* rows of all contexts after it (distinct keys)                                  */
  uint64_t rows_moved;   /* rows copied between different contexts                                          */
  uint64_t bytes_moved;  /* ... in bytes                                                                    */
  uint64_t max_owned;    /* rows of the fullest owner afterwards                                            */
  int32_t contexts, devices;
  int32_t peer_direct;   /* device pairs with direct peer access (xGMI) among the pairs that exchanged rows */
  int32_t rccl;          /* 1: the rows travelled over RCCL (MK_MERGE_RCCL)                                  */
  double s_bucket, s_copy, s_import, s_total; /* wall seconds of the phases */
} mk_merge_stats_t;
/* Sum the running tables of n contexts (same alphabet, k, canonical mode; on n different GPUs, or several on one)
 * in this one process: every context groups its rows by owner (mk_bucket_rows_device), the segments go straight
 * to their owners' GPUs (peer copies: each pair of GPUs has its own xGMI link, all pairs at once), every owner
 * insert-adds what it received.  Rows kept as text end up in ctxs[0].  st may be NULL. */
int mk_merge_devices(mk_ctx* const* ctxs, int n, int flags, mk_merge_stats_t* st);
/* sorted(kmers.items()) of a table spread over n contexts by key range (after MK_MERGE_RANGES): every context
 * sorts its own range on its own GPU, at once; the host concatenates in order.  Same outputs as mk_export_size /
 * mk_export / mk_write_tsv.  MK_ERR_STATE if the contexts' ranges are not ascending and disjoint. */
int mk_export_size_multi(mk_ctx* const* ctxs, int n, size_t* rows);
int mk_export_multi(mk_ctx* const* ctxs, int n, uint8_t* kmers, uint64_t* counts, size_t rows_cap);
int mk_write_tsv_multi(mk_ctx* const* ctxs, int n, const char* path, const char* basename, size_t* rows);

/* Drop the rows of the running table whose count is below min_count.  For a sample that is ONE chunk
 * (one filter unit, lib/mercat2_kmers.py:73-76) but was counted in pieces without a filter -- its records
 * split over several GPUs -- and merged: the filter comes after the merge. */
int mk_filter_min(mk_ctx* ctx, uint64_t min_count);

/* ---- two tables combined by key on the GPU (KMC's `kmc_tools simple`, the Jellyfish merge variants): drop a sample's
 *      k-mers that a background table holds, keep those a marker table holds, the shared k-mers with the smaller count,
 *      one sample's counts minus another's -- one streaming read of a and one probe of b per row, nothing exported ----
 * One rule defines every op.  For every key in a or b, ca and cb are its counts there, 0 where absent.  A count below
 * min_a (respectively min_b) is first taken as 0.  dst receives the key with count f(ca, cb), and no row where that is
 * 0; a SUM that wraps to 0 is therefore no row.  min_a, min_b >= 1: 0 is MK_ERR_ARG, and so is an unknown op.
 * a and b are only READ, under mk_lookup's rules: made final first, a context that holds part of a refused chunk or an
 * open chunk is MK_ERR_STATE, a sharer (mk_share_table) answers for its OWN tables, a repeated call gives the same
 * result.  a == b is allowed.  dst is a third context (dst == a or dst == b: MK_ERR_ARG) of the same device, alphabet,
 * k and canonical mode as a and b (else MK_ERR_ARG); a dst that shares or lends a table, or has an open chunk, is
 * MK_ERR_STATE.  dst is emptied as mk_reset does, then filled; afterwards it is an ordinary context: the exports,
 * mk_write_tsv, mk_lookup, mk_histo, mk_screen_*, mk_alpha_stats and further counting or loading into it all work.
 * Keys are taken as they stand (no folding), as mk_load_tsv takes them.  Every table shape is combined on the GPU: dense
 * bins elementwise, the one-word table (f of the two counts of the 32 x 'T' key kept beside it: on the host), the
 * two-word tables, and the rows kept as text -- a's bytes from a's arena, probed in b's by-reference table, stored in
 * dst's.  A packed row is probed only in b's packed table and a text row only in b's text table: where a key lives is
 * decided by the key alone.  A table never allocated has no slots and answers 0.  All arithmetic is integer: the result
 * is exact whatever the order.  When the call fails after dst was emptied, dst is left empty.  st may be NULL. */
#define MK_OP_MIN   0  /* min(ca, cb): keys in both, the smaller count (KMC intersect)      */
#define MK_OP_MAX   1  /* max(ca, cb): keys in either                                       */
#define MK_OP_SUM   2  /* ca + cb modulo 2^64: keys in either (what mk_merge_from adds up)  */
#define MK_OP_LEFT  3  /* cb ? ca : 0: a's rows whose key b holds, a's counts               */
#define MK_OP_ONLY  4  /* cb ? 0 : ca: a's rows whose key b lacks (KMC kmers_subtract)      */
#define MK_OP_DIFF  5  /* ca > cb ? ca - cb : 0 (KMC counters_subtract)                     */
typedef struct mk_table_op_t {
  uint64_t rows_a, rows_b;   /* rows of a / of b at or above their threshold                          */
  uint64_t both;             /* keys so present in both                                               */
  uint64_t rows_out;         /* rows of dst                                                           */
  uint64_t total_out;        /* sum of their counts (modulo 2^64)                                     */
  uint64_t packed_out, text_out; /* ... in the packed table / kept as text                            */
  uint64_t slots;            /* table slots (dense bins) read                                         */
  int32_t passes;            /* 1, or 2: MAX and SUM also probe a for every row of b                  */
  int32_t op;
  double s_scan, s_total;    /* seconds: HIP-event time of the kernels; wall time of the call         */
} mk_table_op_t;
int mk_table_op(mk_ctx* dst, mk_ctx* a, mk_ctx* b, int op, uint64_t min_a, uint64_t min_b, mk_table_op_t* st);

/* ---- statistics / profiling ----------------------------------------------------------- */
int mk_set_profiling(mk_ctx* ctx, int on);
int mk_get_stats(mk_ctx* ctx, mk_stats_t* out);
int mk_reset_stats(mk_ctx* ctx);

/* ---- host helpers (no GPU needed) ------------------------------------------------------- */
/* Virtual Chunker (lib/mercat2_Chunker.py:39-59): byte offsets into `text` (decompressed file
 * bytes) at which the reference would start chunk 1, 2, ...: a line that contains '>' starts
 * a new chunk once the newline-normalised bytes written to the current chunk are >=
 * chunksize.  cuts[0..*ncuts) ascending; chunk i is [cuts[i-1], cuts[i]) with cuts[-1] = 0
 * and cuts[ncuts] = n.  Returns MK_ERR_RANGE (and the needed size in *ncuts) if cap is short. */
int mk_chunk_cuts(const uint8_t* text, size_t n, uint64_t chunksize, uint64_t* cuts, size_t cap, size_t* ncuts);
/* The same cuts computed by the streaming scanner mk_count_file uses, with the text handed over
 * `block` bytes at a time (a self-check for tests: MK_ERR_STATE if the scanner lost, repeated or
 * misplaced a byte). */
int mk_stream_cuts(const uint8_t* text, size_t n, uint64_t chunksize, size_t block, uint64_t* cuts, size_t cap,
                   size_t* ncuts);
/* Where mk_count_file cuts ONE filter unit (a file below the chunk size) that it spreads over several GPUs: pieces
 * of at least `piece` bytes, each ending where a record starts -- a line whose first non-blank byte is '>', what
 * find_kmers takes for a header (lib/mercat2_kmers.py:51-52); a line that merely contains '>' is not one.
 * Through the streaming scanner, `block` bytes at a time, self-checked like mk_stream_cuts. */
int mk_record_cuts(const uint8_t* text, size_t n, uint64_t piece, size_t block, uint64_t* cuts, size_t cap, size_t* ncuts);
/* Where mk_fastq_select_text cuts a FASTQ text into pieces: behind a line 4j (lines split on '\n' only, numbered across
 * the text) once a piece holds `piece` bytes, so that no 4-line record is split and a record longer than `piece` makes
 * its piece grow.  Only '\n' is counted; nothing else of the text is looked at.  cuts[0..*ncuts) ascending, strictly
 * inside the text; piece i is [cuts[i-1], cuts[i]) with cuts[-1] = 0 and cuts[ncuts] = n.  MK_ERR_RANGE (and the needed
 * size in *ncuts) if cap is short. */
int mk_fastq_cuts(const uint8_t* text, size_t n, uint64_t piece, uint64_t* cuts, size_t cap, size_t* ncuts);
/* The same for mk_fastq_qtrim_text with paired reads: a piece ends behind a line 8j, so that the mates 2p and 2p + 1 stay
 * in one piece; a pair longer than `piece` makes its piece grow. */
int mk_fastq_pair_cuts(const uint8_t* text, size_t n, uint64_t piece, uint64_t* cuts, size_t cap, size_t* ncuts);
/* The file reader's own gzip decoder (csrc/mk_inflate.h) over a whole '.gz' file held in memory,
 * producing `block` bytes per step as the reader does, every member's CRC-32 and length checked.
 * A self-check for tests (against zlib): out must hold the whole text (cap bytes).
 * MK_ERR_IO: corrupt or not gzip, MK_ERR_RANGE: truncated, MK_ERR_NOMEM: cap too small. */
int mk_gunzip(const uint8_t* gz, size_t n, uint8_t* out, size_t cap, size_t block, size_t* written, int* members);
/* The same through the parallel decoder (csrc/mk_pgunzip.h): `threads` pieces of `piece_bytes` compressed
 * bytes are decoded at once, each from a block start found by search, and stitched together. */
int mk_gunzip_parallel(const uint8_t* gz, size_t n, uint8_t* out, size_t cap, int threads, size_t piece_bytes,
                       size_t* written, int* members);
/* zlib's crc32(seed, p, n) as the gzip reader computes it (carry-less multiplies; csrc/mk_crc32.h). */
uint32_t mk_crc32_of(const uint8_t* p, size_t n, uint32_t seed);
/* removeN (lib/mercat2_fasta.py:53-119 with split_sequenceN :21-49), the rewrite MerCat2 applies to every
 * nucleotide FASTA before counting (bin/mercat2.py:239-244): records holding 'N' are cut at every run of N
 * into ">{name}_{i} {info}" pieces re-wrapped at 80 columns, the others are written back line by line;
 * toupper != 0 upper-cases sequence lines on output.  text = the (decompressed) file; *out receives a
 * malloc'ed buffer with the cleaned text (release it with mk_free), st the figures GC content is made of.
 * MK_ERR_RANGE: a record to be split has an empty header (the reference raises IndexError).  A sequence to be
 * split that holds blanks, tabs or hyphens is wrapped by the standard library's word rules, as textwrap.wrap does it
 * for the reference (restated in csrc/mk_host.cpp, checked against textwrap itself: mk_textwrap).  Header lines may
 * hold any bytes; a byte >= 0x80 in a SEQUENCE line is MK_ERR_NON_ASCII (st->unsupported_record names the record),
 * as in the counting calls. */
typedef struct mk_clean_stats_t {
  uint64_t gc_count;      /* 'G' + 'C' as the reference counts them (header lines of split records included) */
  uint64_t total_length;  /* the length it divides by: GC content = 100 * gc_count / total_length            */
  uint64_t records, split_records, pieces, n_runs;
  int64_t unsupported_record; /* -1, or the index of the first record this function does not rewrite */
} mk_clean_stats_t;
int mk_remove_n(const uint8_t* text, size_t n, int toupper, uint8_t** out, size_t* out_len, mk_clean_stats_t* st);
/* fq2fa (see mk_set_fastq) on a whole FASTQ text held in memory: *out receives the converted text exactly as it stands,
 * uncompressed, in MerCat2's <base>.fna.gz (malloc'ed: release it with mk_free), st its figures.  A byte >= 0x80 in a
 * line of the converted text that is not a header line is MK_ERR_NON_ASCII (*out stays NULL), as in the counting
 * calls; header lines may hold any bytes.  (The reference decodes the text as UTF-8 and raises UnicodeDecodeError on
 * invalid UTF-8 in a kept line; this function does not check that.) */
int mk_fq2fa(const uint8_t* text, size_t n, uint8_t** out, size_t* out_len, mk_fastq_stats_t* st);
void mk_free(void* p);
/* textwrap.wrap(text, width) of CPython 3.10 for ASCII text, as mk_remove_n applies it to the pieces of a split
 * sequence: the lines, each followed by '\n', in a malloc'ed buffer (mk_free).  A self-check for tests. */
int mk_textwrap(const uint8_t* text, size_t n, size_t width, uint8_t** out, size_t* out_len);
/* Deterministic synthetic reads: genome of `genome_len` iid ACGT from
 * splitmix64(genome_seed); `reads` reads of `read_len` from uniform starts, reverse-complemented
 * on a coin flip, per-base substitution with probability sub_ppm/1e6, all from
 * splitmix64(read_seed); records ">r{i}\n{seq}\n" with i starting at first_index.
 * Writes at most cap bytes to out (host) and the size to *written (call with out = NULL to size). */
int mk_synth_reads(uint64_t genome_len, uint64_t genome_seed, uint64_t reads, uint32_t read_len,
                   uint64_t read_seed, uint32_t sub_ppm, uint64_t first_index, uint8_t* out, size_t cap,
                   size_t* written);
const char* mk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MERCAT_HIP_H */
