// mk_chunk.hip -- the chunk pipeline behind mk_chunk_end / mk_count_device.  Host code only.
//
// Chunk pipeline == one reference find_kmers call (lib/mercat2_kmers.py:32-78):
//   raw bytes -> parse -> [pack] -> count (dense | hash64 | by-reference) -> keep count >= min_count
//   -> add into the running table (the dict sum of run_mercat2, bin/mercat2.py:121-127).
// Two lanes: process_chunk_fast (one read-back: nucleotide 12 <= k <= 64) and process_chunk (every other shape, and the
// fallback of the first).  What both do alike is the steps below, each called by both.
#include "mk_common.h"
#include <algorithm>
#include <cstddef>
#include <cstdio>

typedef unsigned long long u64;

#define MK_RETRY_GENERAL 1  // (internal) the speculative lane met input it does not handle: take the general path
#define MK_RETRY_DENSE 2    // (internal) the flat parse was refused: the speculative lane again, with the three-kernel parser

// The flat lane (mk_fparse.hip) is worth taking on read files: the scatter walks every raw position, header bytes
// included, so long header lines cost it more than the parser saves.  symbols / raw bytes of the last full chunk below
// this share: the lane is not taken (measured: profiles/fparse_flat.md; MK_FP_FLAT_SHARE overrides it).
#define MK_FLAT_MIN_SHARE 0.70
// share < 0: nothing is known about the input yet -- try the lane.
static bool flat_lane_wanted(bool enabled, double share, double min_share) { return enabled && (share < 0.0 || share >= min_share); }

// ------------------------------------------------------------------- steps of both lanes
// seq / bad / codes for a chunk of n raw bytes (the kernels read the true seq_len on the device)
static int reserve_chunk_buffers(mk_ctx* c, size_t n) {
  int rc;
  if ((rc = mk_buf_reserve(c, c->seq, n + 256)) != MK_OK) return rc;
  if (c->mode == MK_MODE_BYREF) return MK_OK;  // (nothing is packed)
  const size_t bad_words = n / 64 + 4;
  const size_t code_words = c->alphabet == MK_ALPHABET_NT2 ? 2 * bad_words : (bad_words * 64 + 11) / 12;
  if ((rc = mk_buf_reserve(c, c->bad, (bad_words + 2) * 8)) != MK_OK) return rc;
  return mk_buf_reserve(c, c->codes, (code_words + 8) * 8);
}

static int refuse_non_ascii(mk_ctx* c) {
  const MkChunkInfo* h = c->h_info;
  if (!h->non_ascii) return MK_OK;
  c->err = "input holds " + std::to_string(h->non_ascii) +
           " sequence byte(s) >= 0x80 (non-ASCII sequence text is not supported; the chunk was not counted)";
  return MK_ERR_NON_ASCII;
}

// A bucket (or survivor) region sized from the sampled histogram was too small: the kernels stopped short of writing
// past it (a fused count kernel that met the flag stopped before its first bucket: the running table is as it was).
// Partition and count again from the exact histogram, with the launcher that counted; the exact pass is never fused
// and hands its survivors over through their regions.
typedef int (*CountLauncher)(mk_ctx* c, size_t seq_len, uint64_t min_count, bool exact);
static int repartition_exactly(mk_ctx* c, size_t seq_len, u64 min_count, CountLauncher count) {
  MkChunkInfo* h = c->h_info;
  if (!h->part_overflow) return MK_OK;
  if (!c->part_sampled) { c->err = "partition overflow without sampling (internal error)"; return MK_ERR_STATE; }
  if (mk_env_set("MK_VERBOSE")) fprintf(stderr, "[mk] sampled partition too small (where=%llu: 1 records total, 2 survivors total, 4 a bucket, 8 a survivor region): exact pass\n", h->part_overflow);
  // (the fields the partitioned kernels own; what the by-reference kernel added for odd windows stays)
  h->windows = h->records = h->distinct = h->survivors = h->side = h->errors = h->part_overflow = 0;
  MK_HIP(hipMemcpyAsync(c->info.p, h, sizeof(MkChunkInfo), hipMemcpyHostToDevice, c->stream));
  c->st.part_retries += 1;
  int rc = count(c, seq_len, min_count, /*exact=*/true);
  if (rc) return rc;
  if ((rc = mk_pull_info(c)) != MK_OK) return rc;
  if (h->part_overflow) { c->err = "partition overflow after the exact pass (internal error: nothing was counted)"; return MK_ERR_STATE; }
  return MK_OK;
}

// The two-word pre-filter (mk_skmer2.hip mk_sk2_countp_k) met a bucket whose keys share every bit of its hash, which no
// split tells apart: the chunk is counted again by the exact kernel (as a partition that overflowed is: the fields the
// partitioned kernels own start from zero; split_exhausted keeps what the pre-filter met).
static int recount_pre_void(mk_ctx* c, size_t seq_len, u64 min_count) {
  MkChunkInfo* h = c->h_info;
  if (!h->pre_void) return MK_OK;
  if (mk_env_set("MK_VERBOSE")) fprintf(stderr, "[mk] pre-filter could not split %llu bucket(s): exact count\n", h->pre_void);
  h->windows = h->records = h->distinct = h->survivors = h->side = h->errors = h->part_overflow = h->pre_void = 0;
  MK_HIP(hipMemcpyAsync(c->info.p, h, sizeof(MkChunkInfo), hipMemcpyHostToDevice, c->stream));
  int rc = mk_launch_count_superkmer2(c, seq_len, min_count, /*exact=*/true);
  if (rc) return rc;
  if ((rc = mk_pull_info(c)) != MK_OK) return rc;
  if (h->part_overflow || h->pre_void) { c->err = "exact count after the pre-filter overflowed (internal error: nothing was counted)"; return MK_ERR_STATE; }
  return MK_OK;
}

// A fused count kernel has upserted part of a chunk that is then refused: that cannot be taken back, so the context (and
// the table's owner, when the launch went into a shared table) refuses everything but a reset until it gets one.
static void spoil(mk_ctx* c, mk_ctx* t) {
  c->spoiled = true;
  t->spoiled = true;
  c->err += " -- the running table holds part of the refused chunk: mk_reset before anything else";
}

// What the last count launch's read-back decides: the pre-filter's exact recount (two-word keys), the split counter,
// and MK_ERR_RANGE for a chunk whose kernel met a bucket it cannot split.
static int finish_count(mk_ctx* c, size_t seq_len, u64 min_count, bool two) {
  const MkChunkInfo* h = c->h_info;
  int rc;
  if (two && (rc = recount_pre_void(c, seq_len, min_count)) != MK_OK) return rc;
  c->st.split_exhausted += h->split_exhausted;
  if (h->errors) {
    c->err = "counting kernel reported " + std::to_string(h->errors) + " unrecoverable condition(s) (bucket too large to split)";
    return MK_ERR_RANGE;
  }
  c->part_dirty = false;  // the count kernel ran to its end: every cursor is back at its region's start
  return MK_OK;
}

// Room in the running tables for what the chunk is about to import: packed survivors and rows kept as text.
static int grow_for_survivors(mk_ctx* c, size_t packed, size_t by_ref) {
  int rc;
  if (c->mode == MK_MODE_HASH64 && packed && (rc = mk_grow_run64(c, c->run_rows + packed)) != MK_OK) return rc;
  if (by_ref && (rc = mk_grow_run_ref(c, c->run_ref_rows + by_ref)) != MK_OK) return rc;
  // two-word keys: survivors of the partitioned kernel, or (unpartitioned path) of the by-reference chunk table,
  // whose clean rows are packed on their way into the running table
  if (c->mode == MK_MODE_HASH128 && (packed || by_ref) && (rc = mk_grow_run128(c, c->run128_rows + packed + by_ref)) != MK_OK) return rc;
  return MK_OK;
}

// The chunk's survivors, laid out per bucket region by the count kernel, into the running table.
static int import_survivor_regions(mk_ctx* c, bool two) {
  const size_t p1 = (size_t)1 << c->p1_log2;
  const uint64_t *keys = (const uint64_t*)c->surv_keys.p, *cnts = (const uint64_t*)c->surv_cnts.p;
  const SkMeta m = sk_meta(c->part_meta.p, p1, 1);  // (kstart and nsurv lie where they do whatever the regions per bucket)
  const uint64_t *kstart = (const uint64_t*)m.kstart, *nsurv = (const uint64_t*)m.nsurv;
  mk_prof_begin(c, MK_K_FILTER);
  const int rc = two ? mk_launch_import128_regions(c, keys, (const uint64_t*)c->surv_keys2.p, cnts, kstart, nsurv, p1)
                     : mk_launch_import_regions(c, keys, cnts, kstart, nsurv, p1, (size_t)c->h_info->survivors);
  mk_prof_end(c);
  return rc;
}

// What the next chunk plans with (partitioned paths).  full_chunk: this chunk is long enough for its windows per
// distinct key to stand for the sample's (process_chunk_fast says when it is not).
static void note_hints(mk_ctx* c, size_t seq_len, bool full_chunk) {
  const MkChunkInfo* h = c->h_info;
  if (h->distinct && full_chunk) { c->dup_hint = (double)h->windows / (double)h->distinct; c->dup_known = true; }
  if (h->records) {
    c->nk_hint = (double)(h->windows + h->exotic) / (double)h->records;
    c->items_hint = (double)h->records * 32.0 / (double)(seq_len ? seq_len : 1);
  }
}

static void add_chunk_stats(mk_ctx* c, size_t n, u64 min_count) {
  const MkChunkInfo* h = c->h_info;
  c->st.raw_bytes += n;
  c->st.symbols += h->symbols;
  c->st.windows += h->windows + h->exotic;
  c->st.exotic_windows += h->exotic;
  c->st.chunks += 1;
  c->st.records += h->records;
  c->st.distinct += h->distinct;
  c->st.survivors += h->survivors + h->survivors_ref + ((h->side && h->side >= min_count) ? 1 : 0);
}

// ----------------------------------------------------------------------- the one-read-back lane
// The partitioned nucleotide paths (one-word keys 18 <= k <= 32, two-word keys 33 <= k <= 64) with ONE host
// read-back per chunk instead of three.  Everything up to the count kernel is launched on the assumption that the
// fast parser will do (no blank inside a sequence line) and with buffers and grids sized from the raw length (the
// kernels read the true seq_len on the device); the one read-back after the count kernel tells whether that held
// (otherwise MK_RETRY_GENERAL), whether symbols outside the alphabet need the by-reference kernel (then it runs
// now: one more read-back, rare), and how many rows survive; the merge is launched and its row totals are copied
// back without waiting -- they are added up when the next read-back (or mk_settle()) has passed them.
static int process_chunk_fast(mk_ctx* c, const uint8_t* d_raw, size_t n, u64 min_count) {
  int rc;
  const size_t begin = (size_t)((uintptr_t)d_raw & 15);
  const uint8_t* d_al = d_raw - begin;
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
  if ((rc = reserve_chunk_buffers(c, n)) != MK_OK) return rc;
  // The flat lane: decided at a sample's first chunk (the hints downstream then see one kind of length throughout) and
  // given up until mk_reset by a refused launch.  MK_FP_FLAT=0 is the A/B switch.
  const bool flat_on = mk_env_int("MK_FP_FLAT", 1) != 0;
  if (c->flat_lane == 0) c->flat_lane = flat_lane_wanted(flat_on, c->flat_share, mk_env_double("MK_FP_FLAT_SHARE", MK_FLAT_MIN_SHARE)) ? 1 : -1;
  const bool flat = flat_on && c->flat_lane > 0;
  // (the parsed stream itself is not written: only the by-reference kernel reads it, and that runs only when the chunk
  // holds characters outside the alphabet -- the chunk is then parsed once more with the stream, below)
  if ((rc = flat ? mk_launch_fparse_flat(c, d_al, begin, n)
                 : mk_launch_fparse(c, d_al, begin, n, /*fuse_pack_nt=*/true, /*write_seq=*/false)) != MK_OK) return rc;
  const size_t n_pos = flat ? begin + n : n;  // positions the kernels downstream walk at most
  const bool two = c->mode == MK_MODE_HASH128;
  c->rtab_chunk_slots = 0;
  c->surv_regions = 0;
  c->ctab_slots = 0;
  // Fused upsert (mk_skcount.hip): from a sample's second chunk on the count kernel puts the survivors into the running
  // table itself -- no import kernel, no waiting for their number.  The table is sized HERE for what the chunk before
  // kept, twice over; the kernel spills what a table that fills up all the same cannot take, and that is imported below.
  c->fuse_cap = 0;
  if (!two && min_count >= 2 && c->surv_hint_ok && !mk_env_set("MK_NO_FUSE")) {
    const unsigned long long per_bucket = c->surv_hint >> 13;  // (8192 buckets on chunks of this size; smaller chunks: fewer of both)
    const int cap = per_bucket <= 110 ? 512 : (per_bucket <= 360 ? 1024 : 0);
    if (cap) {
      if ((rc = mk_settle(c)) != MK_OK) return rc;  // (run_rows must be what the table holds)
      // Which table: the owner's when this context shares one (mk_share_table) AND that table has room for what this
      // chunk is expected to add -- only the owner ever replaces its table (it sizes it for its sharers as well), a sharer
      // that finds it too small upserts into its own for this chunk; the sum at the end is the same.
      mk_ctx* t = table_of_ctx(c);
      // (what this chunk is expected to add: the last full chunk's survivors -- late in a sample most of them are keys
      // the table already holds; the spill list takes what a bad guess leaves no room for)
      const size_t expect = (size_t)c->surv_hint + 4096;
      if (t != c) {
        std::shared_lock<std::shared_mutex> rd(t->table_mu);
        if (t->run_slots < 1024 || 2 * (t->run_rows + expect) > t->run_slots) t = c;
      }
      if (t == c && (rc = mk_grow_run64(c, c->run_rows + expect * (1 + c->n_sharers))) != MK_OK) return rc;
      c->fuse_target = t;
      c->fuse_cap = cap;
    }
  }
  {
    // (a launch into ANOTHER context's table reads its pointer and size under that table's lock: see mk_share_table)
    mk_ctx* t = c->fuse_cap ? c->fuse_target : c;
    std::shared_lock<std::shared_mutex> rd(t->table_mu, std::defer_lock);
    if (t != c) rd.lock();
    rc = two ? mk_launch_count_superkmer2(c, n_pos, min_count) : mk_launch_count_superkmer(c, n_pos, min_count);  // (seq_len <= n_pos)
  }
  c->fuse_cap = 0;
  if (rc) return rc;
  if ((rc = mk_pull_info(c)) != MK_OK) return rc;  // the one read-back
  MkChunkInfo* h = c->h_info;
  if (flat && (h->parse_fallback & MK_FP_REFUSED)) {  // not one line per record: this sample is parsed densely from here on
    c->st.flat_refused += 1;
    c->flat_lane = -1;
    // (a refused launch left the running table alone: the fused kernel returned at its abort test, which reads the whole
    // word, and the survivors of an unfused one are imported further down.  A wave that found no state to start from
    // may have taken a header line's blanks for a sequence line's: whether the text holds such blanks is the dense
    // parser's to say)
    return MK_RETRY_DENSE;
  }
  if (h->parse_fallback) { c->st.parse_retries += 1; return MK_RETRY_GENERAL; }
  if ((rc = refuse_non_ascii(c)) != MK_OK) return rc;
  const size_t seq_len = (size_t)h->seq_len;  // (flat lane: raw positions)
  // (the exact passes read the packed words and the bitmap in the coordinates of the launch that overflowed: they run
  // before the second parse below rewrites both)
  if ((rc = repartition_exactly(c, seq_len, min_count, two ? mk_launch_count_superkmer2 : mk_launch_count_superkmer)) != MK_OK) return rc;
  if ((rc = finish_count(c, seq_len, min_count, two)) != MK_OK) {
    if (h->errors && !two && c->fused_last) spoil(c, c->fuse_target ? c->fuse_target : c);
    return rc;
  }
  if (h->bad_symbols) {  // windows holding a symbol outside the alphabet: by reference, now
    // the by-reference kernel reads the parsed stream, which the first parse did not write: parse again (the raw text
    // is still there), this time with the stream -- the chunk's counters stand (the second parse adds to them again
    // -- kept bytes >= 0x80 -- so they are set aside and put back).  It also writes the packed words and the bitmap,
    // which nobody reads after it but the by-reference kernel: that needs the bitmap in the stream's coordinates, which
    // the flat lane's is not, and the stream's own length on the device (MkChunkInfo's first word: not put back).
    static_assert(offsetof(MkChunkInfo, seq_len) == 0, "the counters put back below are everything behind seq_len");
    if ((rc = mk_buf_reserve(c, c->ex_tmp, sizeof(MkChunkInfo) + 64)) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(c->ex_tmp.p, c->info.p, sizeof(MkChunkInfo), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = mk_launch_fparse(c, d_al, begin, n, /*fuse_pack_nt=*/flat, /*write_seq=*/true)) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync((char*)c->info.p + sizeof(u64), (const char*)c->ex_tmp.p + sizeof(u64), sizeof(MkChunkInfo) - sizeof(u64),
                          hipMemcpyDeviceToDevice, c->stream));
    const u64 bound = std::min<u64>((u64)seq_len, h->bad_symbols * (u64)c->k);
    c->rtab_chunk_slots = pow2_at_least(2 * (size_t)bound);
    if ((rc = mk_buf_reserve(c, c->rtab_chunk, c->rtab_chunk_slots * sizeof(MkSlot))) != MK_OK) return rc;
    if ((rc = mk_clear_table(c, MK_TABLE_REF, c->rtab_chunk.p, c->rtab_chunk_slots)) != MK_OK) return rc;
    if ((rc = mk_launch_count_byref(c, seq_len, true)) != MK_OK) return rc;  // (the grid covers seq_len; the kernel reads the stream's length)
    if ((rc = mk_launch_count_survivors(c, min_count)) != MK_OK) return rc;
    if ((rc = mk_pull_info(c)) != MK_OK) return rc;
  }
  const bool fused_done = !two && c->fused_last;  // (of the launch that counted: the exact pass is never fused)
  if (fused_done) {
    mk_ctx* t = c->fuse_target ? c->fuse_target : c;  // (counted by the kernel, in the same read-back; the table may be another context's)
    t->run_rows += (size_t)h->new_rows;
    h->new_rows = 0;
    c->st.fused_chunks += 1;
    c->st.fuse_spilled += h->spilled;
    // (what is launched below adds to the device's copy again, and that copy is read back later: start it from zero.
    // Nearly always nothing is: no spill, no rows kept as text -- then neither this fill nor that read-back is issued:
    // two of the five tiny device operations a chunk cost besides its kernels)
    if (h->spilled || h->survivors_ref)
      MK_HIP(hipMemsetAsync(&((MkChunkInfo*)c->info.p)->new_rows, 0, sizeof(unsigned long long), c->stream));
    if (h->spilled) {  // the table was filling up: what the kernel set aside goes in now, into a table with room
      if ((rc = mk_grow_run64(c, c->run_rows + (size_t)h->spilled)) != MK_OK) return rc;
      if ((rc = mk_launch_import_pairs(c, (const uint64_t*)c->surv_keys.p, (const uint64_t*)c->surv_cnts.p, (size_t)h->spilled)) != MK_OK) return rc;
    }
  }
  // (a fused launch has put its survivors in already)
  if ((rc = grow_for_survivors(c, fused_done ? 0 : (size_t)h->survivors, (size_t)h->survivors_ref)) != MK_OK) return rc;
  if (h->survivors && seq_len && !fused_done && (rc = import_survivor_regions(c, two)) != MK_OK) return rc;
  if ((rc = mk_launch_accumulate(c, min_count)) != MK_OK) return rc;  // (survivors of the by-reference chunk table, if any)
  // the merge's row totals: copied back, not waited for (a fused launch that set nothing aside has reported them already)
  if (!fused_done || h->spilled || h->survivors_ref) {
    MK_HIP(hipMemcpyAsync(c->h_info + 1, c->info.p, sizeof(MkChunkInfo), hipMemcpyDeviceToHost, c->stream));
    c->pending_rows = true;
  }
  if (h->side && h->side >= min_count) c->run_side += h->side;
  // (hints for the next chunk come from FULL chunks: a sample's short last chunk -- a third of the coverage, half the
  // windows per distinct key, a fraction of the survivors -- made the first chunk of the next sample plan two sub-range
  // passes per bucket, 480 instead of 305 us, and would size the fused launch's table for nothing)
  const bool full_chunk = !c->dup_known || seq_len * 4 >= c->part_prev_len * 3;
  if (full_chunk && n >= ((size_t)1 << 20)) c->flat_share = (double)h->symbols / (double)n;  // (the flat lane's guard, next sample)
  if (flat) c->st.flat_chunks += 1;
  if (!two && (full_chunk || !c->surv_hint_ok)) { c->surv_hint = h->survivors; c->surv_hint_ok = true; }
  note_hints(c, seq_len, full_chunk);
  if (mk_env_set("MK_VERBOSE"))
    fprintf(stderr, "[mk] chunk (one read-back): raw=%zu seq=%zu windows=%llu records=%llu distinct=%llu survivors=%llu p1=2^%d dup=%.2f nk=%.2f fused=%d spilled=%llu rows=%zu slots=%zu\n",
            n, seq_len, (unsigned long long)h->windows, (unsigned long long)h->records, (unsigned long long)h->distinct,
            (unsigned long long)h->survivors, c->p1_log2, c->dup_hint, c->nk_hint, fused_done ? 1 : 0, (unsigned long long)h->spilled,
            (size_t)c->run_rows, c->run_slots);
  c->st.table_slots = c->rtab_chunk_slots;
  add_chunk_stats(c, n, min_count);
  return MK_OK;
}

// --------------------------------------------------------------------------- the general lane
// d_raw may be unaligned: the fast parser reads from the 16-byte boundary below it and ignores the
// bytes in front; only the (rare) general-parser fallback needs an aligned copy.
static int process_chunk(mk_ctx* c, const uint8_t* d_raw, size_t n, u64 min_count) {
  int rc;
  bool known_blank = false;
  if (c->clean_mode) {  // (one read-back more than the speculative lane: the chunk must be known to be reproducible BEFORE it is merged)
    if (d_raw != (const uint8_t*)c->raw.p) { c->err = "clean mode rewrites the text in place: feed it (mk_chunk_feed), do not pass caller memory"; return MK_ERR_STATE; }
    MK_HIP(hipSetDevice(c->device));
    if ((rc = mk_launch_clean_pre(c, (uint8_t*)c->raw.p, n)) != MK_OK) return rc;
  }
  if (c->fastq_mode) {  // (in place, before the parser: everything after it -- the speculative lane included -- reads FASTA)
    if (d_raw != (const uint8_t*)c->raw.p) { c->err = "FASTQ mode rewrites the text in place: feed it (mk_chunk_feed), do not pass caller memory"; return MK_ERR_STATE; }
    MK_HIP(hipSetDevice(c->device));
    if ((rc = mk_launch_fastq_pre(c, (uint8_t*)c->raw.p, n)) != MK_OK) return rc;
  }
  if (!c->clean_mode && c->alphabet == MK_ALPHABET_NT2 && n && n < 0xFE000000ull &&
      ((c->mode == MK_MODE_HASH64 && c->k >= MK_SK_MIN_K && c->k <= 32) || c->mode == MK_MODE_HASH128)) {
    rc = process_chunk_fast(c, d_raw, n, min_count);
    if (rc == MK_RETRY_DENSE) rc = process_chunk_fast(c, d_raw, n, min_count);  // (flat_lane is off now)
    if (rc != MK_RETRY_GENERAL) return rc;
    known_blank = true;  // (the fast parser has just said so: straight to the general one)
  }
  if ((rc = mk_settle(c)) != MK_OK) return rc;
  const size_t begin = (size_t)((uintptr_t)d_raw & 15);
  const uint8_t* d_al = d_raw - begin;
  MkChunkInfo* h = c->h_info;
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
  if ((rc = reserve_chunk_buffers(c, n)) != MK_OK) return rc;
  const bool packed = c->mode != MK_MODE_BYREF;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const bool fast = attempt == 0 && !known_blank;
    const bool fused = fast && packed && c->alphabet == MK_ALPHABET_NT2;  // the nt pack rides on the parser's LDS image
    if (!fast && begin) {  // aligned copy for the general transducer
      if ((rc = mk_buf_reserve(c, c->raw, n + 64)) != MK_OK) return rc;
      MK_HIP(hipMemcpyAsync(c->raw.p, d_raw, n, hipMemcpyDeviceToDevice, c->stream));
      d_raw = (const uint8_t*)c->raw.p;
    }
    if ((rc = fast ? mk_launch_fparse(c, d_al, begin, n, fused) : mk_launch_parse(c, d_raw, n)) != MK_OK) return rc;
    if (packed && !fused && (rc = mk_launch_pack(c, n)) != MK_OK) return rc;
    if (c->clean_mode && (rc = mk_launch_clean_post(c, n)) != MK_OK) return rc;
    if ((rc = mk_pull_info(c)) != MK_OK) return rc;
    if (c->clean_mode) {
      const u64* m = c->h_clean;  // first header | '>' bytes | marker bytes in the input | N bytes | runs | G+C | starts | ends
      const u64 headers = h->seq_len - h->symbols;
      const char* why = h->parse_fallback ? "a blank inside a sequence line"
                        : m[2]            ? "a 0x7F byte in the text, or blanks in front of the first header"
                        : m[1] != headers ? "a '>' that does not start a header line"
                                          : nullptr;
      if (why) {
        c->err = std::string("clean mode: ") + why + " (removeN's rewrite of such text is not reproduced on the GPU; nothing was counted)";
        return MK_ERR_UNSUPPORTED;
      }
      c->clean_raw += n;
      c->clean_headers += headers;
      c->clean_n_bytes += m[3];
      c->clean_n_runs += m[4];
      c->clean_gc += m[5];
      c->clean_symbols += h->symbols - m[3];
      c->clean_last_runs = m[4];
      h->symbols -= m[3];  // (the N bytes are separators now)
      break;
    }
    if (!fast || !h->parse_fallback) break;
    c->st.parse_retries += 1;
    // a blank inside a sequence line: the general transducer handles strip() exactly
    MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
  }
  if ((rc = refuse_non_ascii(c)) != MK_OK) return rc;
  const size_t seq_len = (size_t)h->seq_len;
  const u64 bad_symbols = h->bad_symbols;

  // chunk tables
  c->rtab_chunk_slots = 0;
  const bool partitioned = c->mode == MK_MODE_HASH64;
  c->surv_regions = 0;
  c->ctab_slots = c->mode == MK_MODE_DENSE ? c->ctab_slots : 0;
  // partitioned path: no global chunk table (32-bit record indices in the scatter's LDS: chunks below 4 G symbols)
  const bool sk2 = c->mode == MK_MODE_HASH128 && c->alphabet == MK_ALPHABET_NT2 && seq_len < 0xFFFFFF00ull;
  if (c->mode == MK_MODE_HASH128 && c->canonical && !sk2) {
    c->err = "canonical counting of 33..64-mers needs the partitioned path (chunk of 4 G symbols or more)";
    return MK_ERR_RANGE;
  }
  if (c->mode == MK_MODE_BYREF || (c->mode == MK_MODE_HASH128 && !sk2)) {
    c->rtab_chunk_slots = pow2_at_least(2 * seq_len);
  } else if (bad_symbols) {
    const u64 bound = std::min<u64>((u64)seq_len, bad_symbols * (u64)c->k);
    c->rtab_chunk_slots = pow2_at_least(2 * (size_t)bound);
  }
  if (c->rtab_chunk_slots) {
    if ((rc = mk_buf_reserve(c, c->rtab_chunk, c->rtab_chunk_slots * sizeof(MkSlot))) != MK_OK) return rc;
    if ((rc = mk_clear_table(c, MK_TABLE_REF, c->rtab_chunk.p, c->rtab_chunk_slots)) != MK_OK) return rc;
  }
  c->st.table_slots = (c->mode == MK_MODE_BYREF || c->mode == MK_MODE_HASH128) ? c->rtab_chunk_slots : c->ctab_slots;

  // count
  if (c->mode == MK_MODE_DENSE) rc = mk_launch_count_dense(c, seq_len);
  else if (partitioned) {
    // (the super-k-mer scatter keeps 32-bit record indices in LDS)
    const bool sk = c->alphabet == MK_ALPHABET_NT2 && c->k >= MK_SK_MIN_K && c->k <= 32 && seq_len < 0xFE000000ull;
    // (keys of 16..26 bits -- nucleotide 8 <= k <= 11, protein k = 4, 5 -- are counted by direct index: mk_bin.hip)
    const bool binned = !sk && mk_binned_takes(c) && seq_len < 0xFFFFFF00ull;
    rc = sk ? mk_launch_count_superkmer(c, seq_len, min_count)
            : (binned ? mk_launch_count_binned(c, seq_len, min_count) : mk_launch_count_partitioned(c, seq_len, min_count));
  }
  else if (c->mode == MK_MODE_HASH128) rc = sk2 ? mk_launch_count_superkmer2(c, seq_len, min_count) : mk_launch_count_ref128(c, seq_len);
  if (rc) return rc;
  // by reference, byte-wise: every window (raw mode) or only those holding a symbol outside the alphabet
  if (c->rtab_chunk_slots && (c->mode != MK_MODE_HASH128 || bad_symbols) &&
      (rc = mk_launch_count_byref(c, seq_len, packed)) != MK_OK) return rc;

  // filter (per chunk!) + merge
  if ((rc = mk_launch_count_survivors(c, min_count)) != MK_OK) return rc;
  if ((rc = mk_pull_info(c)) != MK_OK) return rc;
  if ((rc = repartition_exactly(c, seq_len, min_count, sk2 ? mk_launch_count_superkmer2 : mk_launch_count_superkmer)) != MK_OK) return rc;
  if ((rc = finish_count(c, seq_len, min_count, sk2)) != MK_OK) return rc;
  if ((rc = grow_for_survivors(c, (size_t)h->survivors, (size_t)h->survivors_ref)) != MK_OK) return rc;
  if (sk2 && c->surv_regions == 2 && seq_len && h->survivors && (rc = import_survivor_regions(c, true)) != MK_OK) return rc;
  if (partitioned && h->survivors) {
    if (c->surv_regions) rc = import_survivor_regions(c, false);
    else {  // (a chunk's survivors from the direct-index / 8-byte-key paths: each key once)
      mk_prof_begin(c, MK_K_FILTER);
      rc = mk_launch_import_pairs(c, (const uint64_t*)c->surv_keys.p, (const uint64_t*)c->surv_cnts.p, (size_t)h->survivors, true);
      mk_prof_end(c);
    }
    if (rc) return rc;
  }
  if ((rc = mk_launch_accumulate(c, min_count)) != MK_OK) return rc;
  if ((rc = mk_pull_info(c)) != MK_OK) return rc;
  mk_add_packed_rows(c, (size_t)h->new_rows);
  c->run_ref_rows += (size_t)h->new_rows_ref;
  if (h->side && h->side >= min_count) c->run_side += h->side;
  if (partitioned || sk2) note_hints(c, seq_len, /*full_chunk=*/true);  // (this lane takes dup_hint from every chunk)

  if (mk_env_set("MK_VERBOSE"))
    fprintf(stderr, "[mk] chunk: raw=%zu seq=%zu windows=%llu records=%llu distinct=%llu survivors=%llu new_rows=%llu p1=2^%d dup=%.2f nk=%.2f\n", n, seq_len,
            (unsigned long long)h->windows, (unsigned long long)h->records, (unsigned long long)h->distinct,
            (unsigned long long)h->survivors, (unsigned long long)h->new_rows, c->p1_log2, c->dup_hint, c->nk_hint);
  add_chunk_stats(c, n, min_count);
  return MK_OK;
}

// ---------------------------------------------------------------------------- the ABI calls
extern "C" int mk_chunk_end(mk_ctx* c, uint64_t min_count) {
  if (!c) return MK_ERR_ARG;
  if (!c->in_chunk) { c->err = "mk_chunk_end: no open chunk"; return MK_ERR_STATE; }
  c->in_chunk = false;
  int rc = process_chunk(c, (const uint8_t*)c->raw.p, c->raw_len, min_count);
  c->raw_len = 0;
  return rc;
}

extern "C" int mk_count_device(mk_ctx* c, const uint8_t* d_text, size_t n, uint64_t min_count) {
  if (!c) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_count_device");
  if (c->in_chunk) { c->err = "mk_count_device: a chunk is open"; return MK_ERR_STATE; }
  if (n && !d_text) { c->err = "mk_count_device: d_text is NULL"; return MK_ERR_ARG; }
  if (c->fastq_mode) { c->err = "mk_count_device: FASTQ mode rewrites the text in place: feed it (mk_chunk_feed_device)"; return MK_ERR_STATE; }
  if (!c->clean_mode) return process_chunk(c, d_text, n, min_count);
  int rc = mk_chunk_begin(c);
  if (!rc) rc = mk_chunk_feed_device(c, d_text, n);
  if (rc) { c->in_chunk = false; return rc; }
  return mk_chunk_end(c, min_count);
}
