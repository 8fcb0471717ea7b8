// mk_common.h -- shared declarations of the MI355X k-mer engine (internal, not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <atomic>
#include <chrono>
#include <mutex>
#include <shared_mutex>
#include <vector>
#include "../../include/mercat_hip.h"
#include "mk_env.h"

// ------------------------------------------------------------------------------------------
// Device data layout (all in HBM, owned by the context)
//
//   raw      u8[n]            the chunk's FASTA bytes as fed
//   seq      u8[<=n]          parsed stream: kept sequence characters, records separated by
//                             one SEP byte ('\n' can never be a kept character)
//   codes    u64[...]         packed symbols, MSB first: 32 x 2-bit (nt) or 12 x 5-bit (aa,
//                             bits 63..4) per word
//   bad      u64[...]         1 bit per symbol (LSB first): symbol outside the alphabet, a
//                             separator, or beyond the end of seq
//   table    Slot[2^m]        open-addressed, linear probing, 16-byte slots {key, count}
//   table128 Slot128[2^m]     32-byte slots {hi, lo, count, pad} for 33..64-mers
//   bins     u64[4^k | 32^k]  dense histogram (small k)
// ------------------------------------------------------------------------------------------

// Smallest nucleotide k that takes the super-k-mer partition (mk_skmer.hip): k - 10 minimizer candidates per window.
// Round 3: 12 (measured on an S2 chunk, Gbases/s against the 8-byte-key partition: k = 12 50 / 42, 14 74 / 47, 16 90 / 46,
// 17 96 / 21; round 2 started at 18).
#define MK_SK_MIN_K 12
#define MK_SEP 0x0Au
#define MK_EMPTY 0xFFFFFFFFFFFFFFFFull

struct __attribute__((aligned(16))) MkSlot {
  unsigned long long key;
  unsigned long long cnt;
};

// Running table of two-word keys (nucleotide 33..64-mers: hi = bases 0..31, lo = the rest, left-aligned).
// There is no 128-bit compare-and-swap, so the COUNT word is the slot's state: 0 = free,
// MK_LOCK128 = claimed, key words being written, anything else = the count (key words final).
#define MK_LOCK128 0xFFFFFFFFFFFFFFFFull
struct __attribute__((aligned(32))) MkSlot128 {
  unsigned long long hi;
  unsigned long long lo;
  unsigned long long cnt;
  unsigned long long pad;
};

// Device-side scalars of one chunk (one struct in HBM, read back once per chunk).
struct MkChunkInfo {
  unsigned long long seq_len;       // bytes in seq (symbols + separators)
  unsigned long long symbols;       // kept sequence characters
  unsigned long long non_ascii;     // kept (sequence) bytes >= 0x80; header lines may hold any bytes
  unsigned long long bad_symbols;   // kept characters outside the alphabet
  unsigned long long windows;       // windows counted by the packed/dense path
  unsigned long long exotic;        // windows counted by mk_count_byref_k: those no packed kernel takes (a character outside the alphabet; every window in MK_MODE_BYREF)
  unsigned long long survivors;     // packed entries passing min_count (this chunk)
  unsigned long long survivors_ref; // by-reference entries passing min_count
  unsigned long long side;          // count of the one key that equals MK_EMPTY (all-T 32-mer)
  unsigned long long new_rows;      // rows added to the running table by this chunk
  unsigned long long new_rows_ref;
  unsigned long long distinct;      // distinct packed keys seen in this chunk (partitioned path)
  unsigned long long errors;        // non-zero: a kernel hit a condition it cannot handle
  unsigned long long parse_fallback;  // fast parser: MK_FP_BLANK (a blank in a sequence line: re-parse generally) | MK_FP_REFUSED
  unsigned long long records;       // super-k-mer records written (partitioned nt path)
  unsigned long long part_overflow; // a bucket region sized from a sampled histogram was too small: partition again, exactly
  unsigned long long spilled;       // fused upsert (mk_skcount.hip): survivors written to the spill list instead of the running table
  unsigned long long split_exhausted; // sub-ranges counted (or found void) with every split bit used: the whole LDS table probed
  unsigned long long pre_void;      // two-word pre-filter (mk_skmer2.hip): buckets it could not split far enough (count them exactly)
};

#define MK_FP_BLANK 1u    // MkChunkInfo::parse_fallback: the fast parsers' one assumption failed (mk_fparse.hip)
#define MK_FP_REFUSED 2u  // ... the flat lane's rule failed: the text is not one line per record (mk_fparse_flat)

enum MkMode { MK_MODE_DENSE = 0, MK_MODE_HASH64 = 1, MK_MODE_HASH128 = 2, MK_MODE_BYREF = 3 };
enum MkKernelId { MK_K_PARSE = 0, MK_K_PACK, MK_K_COUNT, MK_K_EXOTIC, MK_K_FILTER, MK_K_EXPORT, MK_K_PART, MK_K_NUM };

// 64-bit finaliser (splitmix64 / murmur3 style): bijective, mixes every input bit into every
// output bit -- used to pick the home slot of a packed key.
__host__ __device__ static inline unsigned long long mk_mix64(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

#define MK_POLY_B 0x9E3779B97F4A7C15ull  // odd multiplier of the rolling polynomial hash

struct MkDevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// Wall-clock seconds since t0 = MkClock::now(): the s_total / s_read figures of the read-only calls.
typedef std::chrono::steady_clock MkClock;
static inline double mk_since(MkClock::time_point t0) { return std::chrono::duration<double>(MkClock::now() - t0).count(); }

struct mk_ctx;
// ---- host plumbing shared by the host-only files (mk_api / mk_chunk / mk_export / mk_combine / mk_tableops / mk_multi) ----
// mk_api.hip: growable device buffers
int mk_buf_reserve(mk_ctx* c, MkDevBuf& b, size_t bytes, bool keep = false);
// mk_api.hip, for mk_ingest.hip: append host bytes to the open chunk without waiting for the copy
// (the source must stay untouched until the context's stream has passed it) unless wait is set
int mk_feed_host_async(mk_ctx* c, const uint8_t* p, size_t n, bool wait);
int mk_reserve_raw(mk_ctx* c, size_t bytes);
// mk_api.hip: MK_ERR_STATE (and the message) when the context holds part of a refused chunk (mk_ctx::spoiled), else MK_OK
int mk_refuse_spoiled(mk_ctx* c, const char* what);
// mk_api.hip: mk_last_error(NULL), for calls that have no context
void mk_set_global_error(const std::string& msg);
// mk_api.hip: row totals and the chunk's scalars
int mk_settle(mk_ctx* c);     // fold row totals that were read back without waiting; before anything reads run_rows & co.
int mk_pull_info(mk_ctx* c);  // MkChunkInfo -> h_info, stream idle afterwards
// mk_api.hip: the running table of this kind (MkTableKind) replaced by one of `slots` slots that holds its rows -- with
// kept, only the rows with count >= min_count, *kept of them.  The caller holds whatever lock the table needs.
int mk_rebuild_table(mk_ctx* c, int kind, size_t slots, uint64_t min_count = 0, size_t* kept = nullptr);
// mk_api.hip: room in a running table for need_rows keys in all (mk_grow_run: for more_rows further packed keys)
int mk_grow_run64(mk_ctx* c, size_t need_rows);
int mk_grow_run128(mk_ctx* c, size_t need_rows);
int mk_grow_run_ref(mk_ctx* c, size_t need_rows);
int mk_grow_run(mk_ctx* c, size_t more_rows);

// mk_api.hip: how a read-only call on the tables opens (mk_lookup*, mk_screen*, the inputs of mk_table_op): the
// arguments, then the table made final and the context's stream drained; *fold = the fold flag was given (and may be)
int lk_open(mk_ctx* c, const char* what, unsigned flags, bool* fold);

struct MkEventPair {
  hipEvent_t a, b;
  int id;
};

struct mk_ctx {
  int device = 0;
  int alphabet = 0;
  int k = 0;
  int bits = 0;           // bits per symbol (2, 5, 0 for raw)
  int syms_per_word = 0;  // 32, 12
  int mode = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool in_chunk = false;
  // a fused count kernel upserted part of a chunk that was then refused: the running table holds part of it, and every
  // call but mk_reset / mk_reset_for / mk_destroy is refused until a reset clears it
  std::atomic<bool> spoiled{false};
  bool profile = false;

  // chunk staging
  MkDevBuf raw;
  size_t raw_len = 0;
  MkDevBuf seq, codes, bad;
  MkDevBuf tile_maps;   // parse scratch
  MkDevBuf info;        // MkChunkInfo on device
  MkChunkInfo* h_info = nullptr;  // pinned host copy (two structs: [1] receives the read-back that is not waited for)
  bool pending_rows = false;      // h_info[1] holds (or will hold, once the stream has passed the copy) the row totals
                                  // of the last chunk's merge, not yet added to run_rows / run128_rows / run_ref_rows

  // chunk tables
  MkDevBuf ctab;        // MkSlot[] (hash64) / MkSlot128[] (hash128) / u64 bins (dense)
  size_t ctab_slots = 0;
  MkDevBuf rtab_chunk;  // by-reference chunk table MkSlot[] (key = tag|pos)
  size_t rtab_chunk_slots = 0;

  // running (merged) tables
  MkDevBuf run;         // same layout as ctab (dense: u64 bins)
  size_t run_slots = 0;
  // (run_rows / run128_rows are atomic: an owner's count is added to by its sharers' host threads -- mk_share_table)
  std::atomic<size_t> run_rows{0};
  unsigned long long run_side = 0;  // count of the MK_EMPTY-valued key
  MkDevBuf run_ref;     // by-reference running table MkSlot[] (key = tag|arena index)
  size_t run_ref_slots = 0;
  size_t run_ref_rows = 0;
  MkDevBuf arena;       // k bytes per by-reference row
  size_t arena_rows_cap = 0;
  MkDevBuf run128;      // MkSlot128[]: packed two-word keys (mode MK_MODE_HASH128), u64 counts
  size_t run128_slots = 0;
  std::atomic<size_t> run128_rows{0};

  // partitioned counting (hash64): keys bucketed by hash, counted per bucket in LDS
  MkDevBuf part;        // u64 keys, bucket after bucket
  MkDevBuf part_meta;   // u64 hist[P1] | start[P1+1] | cursor[P1]
  MkDevBuf surv_keys, surv_cnts;  // (key,count) survivors of the chunk
  MkDevBuf surv_keys2;            // second key word of the survivors (33..64-mers)
  int p1_log2 = 10;
  double dup_hint = 1.0;  // windows per distinct key seen in the previous chunk
  bool dup_known = false; // ... of THIS sample (mk_reset forgets it)
  int canonical = 0;      // opt-in: count min(kmer, revcomp) (nt only)
  bool part_sampled = false;  // the last super-k-mer partition sized its buckets from a sample
  // bucket regions of the previous chunk kept for the next one (mk_skmer.hip): same size, same min_count, no overflow
  bool part_reuse_ok = false;
  bool part_dirty = false;    // a partition was launched and its chunk has not been seen to end well (cursors may be anywhere)
  size_t part_prev_len = 0;
  int part_prev_p1 = 0;
  int part_nseg = 1;            // regions per bucket of the last one-word partition (1, or 8: one per XCD)
  unsigned long long part_prev_minc = 0;
  int part_cooldown = 0;      // chunks that size their buckets afresh after a chunk overflowed inherited regions
  int surv_regions = 0;   // survivors of the last chunk are laid out per bucket (kstart/nsurv in part_meta)
  double nk_hint = 8.0;   // windows per super-k-mer record seen in the previous chunk
  double items_hint = 0;  // records per analysis thread (32 positions) seen in the previous chunk; 0 = not known yet
  // fused upsert (mk_skcount.hip): the count kernel puts a chunk's survivors into the running table itself
  int fuse_cap = 0;                   // list entries per sweep the NEXT count launch may use (0: survivors go to their regions)
  bool fused_last = false;            // the last count launch was a fused one
  unsigned long long surv_hint = 0;   // survivors of the previous chunk of this sample
  bool surv_hint_ok = false;
  // flat lane (mk_fparse.hip mk_fparse_flat): decided at a sample's first chunk, kept until mk_reset
  int flat_lane = 0;          // 0 not decided yet, 1 taken, -1 not taken (the guard said no, or a launch was refused)
  double flat_share = -1.0;   // symbols per raw byte of the last full chunk; < 0: not known yet
  // one table for several contexts of a device (mk_share_table): the fused launches of this context upsert into the owner's
  mk_ctx* share_owner = nullptr;
  mk_ctx* fuse_target = nullptr;      // the context whose table the NEXT / last fused launch of this one upserts into (this or share_owner)
  std::vector<mk_ctx*> sharers;       // contexts whose fused launches upsert into THIS context's table (changed under table_mu)
  std::atomic<size_t> n_sharers{0};   // sharers.size(), for readers that do not hold table_mu
  std::shared_mutex table_mu;         // shared: a launch reads run.p / run_slots; exclusive: the table is replaced (grown) or cleared

  // export scratch
  MkDevBuf ex_keys, ex_cnts, ex_keys2, ex_cnts2, ex_tmp;
  MkDevBuf ex128, ex128_out;  // two-word rows: compacted {hi, lo, count} + sort scratch; sorted rows for the host

  // clean mode (mk_clean.hip): the raw file is counted as removeN would leave it
  int clean_mode = 0, clean_upper = 0;
  MkDevBuf clean_meta, clean_runs;
  unsigned long long* h_clean = nullptr;   // pinned: the 8 meta words of the last chunk
  unsigned long long clean_n_runs = 0, clean_n_bytes = 0, clean_gc = 0, clean_symbols = 0, clean_raw = 0, clean_headers = 0;
  unsigned long long clean_last_runs = 0;  // runs of the last chunk (listed in clean_runs up to its capacity)

  // FASTQ mode (mk_fastq.hip): every chunk is raw FASTQ, counted as fq2fa leaves it
  int fastq_mode = 0;
  MkDevBuf fastq_stats;  // 8 words summed over the chunks since mk_reset (mk_fastq.hip)
  MkDevBuf fastq_tiles;  // per 4 KiB tile: entering line number and class | summary

  // multi-GPU merge staging (mk_multi.hip): rows grouped by owner going out, rows received from the peers,
  // owner bounds + histogram + cursors
  MkDevBuf xfer_out, xfer_in, xfer_meta;

  // pinned block ring of mk_count_file (mk_ingest.hip), kept between files
  void* ingest_ring = nullptr;
  size_t ingest_ring_bytes = 0;
  // two blocks the TSV text is copied out through (mk_write_tsv): ordinary (cached) memory, registered with the driver --
  // the CPU READS these, and it read hipHostMalloc'ed memory at 3.5 GB/s
  void* tsv_pin = nullptr;
  size_t tsv_pin_bytes = 0;

  // stats
  mk_stats_t st{};
  mk_export_stats_t ex_st{};  // of the last mk_export / mk_write_tsv (mk_export_stats)
  std::vector<MkEventPair> events;
  std::vector<hipEvent_t> event_pool;
};

#define MK_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e__ = (call);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      c->err = std::string(#call) + ": " + hipGetErrorString(e__);                           \
      return MK_ERR_HIP;                                                                     \
    }                                                                                        \
  } while (0)

// A section of the context's stream timed by a pair of events (the s_probe / s_scan / s_parse figures of the read-only
// calls): begin(), the launches, end(), the caller's read-backs and its sync, then add_to().  The events die with it,
// on every path.
struct MkTimed {
  mk_ctx* c;
  hipEvent_t ev[2] = {nullptr, nullptr};
  explicit MkTimed(mk_ctx* c_) : c(c_) {}
  MkTimed(const MkTimed&) = delete;
  MkTimed& operator=(const MkTimed&) = delete;
  ~MkTimed() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int begin() {
    for (auto& e : ev)
      if (!e) MK_HIP(hipEventCreate(&e));
    MK_HIP(hipEventRecord(ev[0], c->stream));
    return MK_OK;
  }
  int end() {
    MK_HIP(hipEventRecord(ev[1], c->stream));
    return MK_OK;
  }
  int add_to(double& seconds) {  // (once the stream has passed end())
    float ms = 0.f;
    MK_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    seconds += ms * 1e-3;
    return MK_OK;
  }
};

// How an ABI entry point opens: refuse a spoiled context, fold pending row totals.  Both return from the caller.
#define MK_REFUSE_SPOILED(c, what)                                                           \
  do {                                                                                       \
    const int rs__ = mk_refuse_spoiled((c), (what));                                         \
    if (rs__) return rs__;                                                                   \
  } while (0)
#define MK_SETTLE(c)                                                                         \
  do {                                                                                       \
    const int rc__ = mk_settle(c);                                                           \
    if (rc__) return rc__;                                                                   \
  } while (0)

static inline size_t div_up(size_t a, size_t b) { return (a + b - 1) / b; }
static inline unsigned grid_for(size_t items, unsigned per_block = 256, unsigned cap = 1u << 20) {
  size_t g = div_up(items, per_block);
  if (g > cap) g = cap;
  if (g == 0) g = 1;
  return (unsigned)g;
}
static inline size_t pow2_at_least(size_t v) {
  size_t p = 1024;
  while (p < v) p <<= 1;
  return p;
}
static inline void buf_free(MkDevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}
// the context whose running table the fused launches of c upsert into (mk_share_table)
static inline mk_ctx* table_of_ctx(mk_ctx* c) { return c->share_owner ? c->share_owner : c; }

// The packed running table of a context.  (MK_TABLE_REF, the by-reference table beside it, is never what table_of names.)
enum MkTableKind { MK_TABLE_NONE = 0, MK_TABLE_ONE = 1, MK_TABLE_TWO = 2, MK_TABLE_DENSE = 3, MK_TABLE_REF = 4 };
struct TableRef {
  int kind = MK_TABLE_NONE;
  const void* p = nullptr;
  size_t slots = 0;
  size_t rows = 0;  // rows the host knows of (dense: unknown, bins)
};
static inline TableRef table_of(const mk_ctx* c) {
  TableRef t;
  if (c->mode == MK_MODE_HASH64 && c->run_slots) { t.kind = MK_TABLE_ONE; t.p = c->run.p; t.slots = c->run_slots; t.rows = c->run_rows; }
  else if (c->mode == MK_MODE_HASH128 && c->run128_slots) { t.kind = MK_TABLE_TWO; t.p = c->run128.p; t.slots = c->run128_slots; t.rows = c->run128_rows; }
  else if (c->mode == MK_MODE_DENSE) { t.kind = MK_TABLE_DENSE; t.p = c->run.p; t.slots = c->run_slots; t.rows = c->run_slots; }
  return t;
}
// n keys were new to the packed table (dense bins have no new keys: their kernels leave n at 0)
static inline void mk_add_packed_rows(mk_ctx* c, size_t n) { (c->mode == MK_MODE_HASH128 ? c->run128_rows : c->run_rows) += n; }
// rows of the hashed tables: the packed ones (with the one key kept beside the one-word table), and all of them
static inline size_t mk_packed_rows(const mk_ctx* c) { return c->run_rows + (c->run_side ? 1 : 0) + c->run128_rows; }
static inline size_t mk_total_rows(const mk_ctx* c) { return mk_packed_rows(c) + c->run_ref_rows; }

// A sample's rows on the host (mk_export.hip), for mk_combine.hip
struct ExportView {
  std::vector<unsigned long long> pkeys, pcnts;  // packed rows, sorted by key (two-word keys: pkeys holds {hi, lo} pairs)
  int words = 1;                                 // 64-bit words per packed key
  size_t packed_rows() const { return pcnts.size(); }
  std::vector<uint8_t> rstr;                     // by-reference rows: k bytes each, arena order
  std::vector<unsigned long long> rcnt;          // counts in arena order
  std::vector<unsigned long long> rorder;        // arena rows sorted by string
};
int mk_build_view(mk_ctx* c, ExportView& v);  // every row of c's running tables, sorted (settles first; fills c->ex_st)
void mk_decode_row(const mk_ctx* c, const ExportView& v, size_t i, uint8_t* out);  // packed row i -> its k characters

// ---- kernel launchers (each in its own translation unit) ---------------------------------
// parse: raw[n] -> seq, info (seq_len, symbols, non_ascii)
int mk_launch_parse(mk_ctx* c, const uint8_t* d_raw, size_t n);
// fast parse (mk_fparse.hip): same output; sets info.parse_fallback when its assumption fails
int mk_launch_fparse(mk_ctx* c, const uint8_t* d_raw, size_t begin, size_t len, bool fuse_pack_nt, bool write_seq = true);
// flat lane: packed words and bad bitmap at raw-text positions; sets MK_FP_REFUSED when the text is not one line per record
int mk_launch_fparse_flat(mk_ctx* c, const uint8_t* d_raw, size_t begin, size_t len);
// pack: seq -> codes, bad (+ info.bad_symbols)
int mk_launch_pack(mk_ctx* c, size_t seq_cap);
// counting
int mk_launch_count_dense(mk_ctx* c, size_t seq_cap);
int mk_launch_count_byref(mk_ctx* c, size_t seq_cap, bool exotic_only);
// nt 33..64-mers without bad symbols: by reference with packed hashing/compare (mode MK_MODE_HASH128)
int mk_launch_count_ref128(mk_ctx* c, size_t seq_len);
// partitioned hash64 path: windows -> hash buckets -> per-bucket LDS tables -> survivors (count >= min_count)
int mk_launch_count_partitioned(mk_ctx* c, size_t seq_len, uint64_t min_count);
// super-k-mer form of the same (nt, 18 <= k <= 32): mk_skmer.hip
int mk_launch_count_superkmer(mk_ctx* c, size_t seq_len, uint64_t min_count, bool exact = false);
// mk_skmer.hip: bucket regions (records and survivors) from an exact or sampled histogram, in one kernel
bool mk_part_inherit(mk_ctx* c, size_t seq_len, int p1_log2, uint64_t min_count, bool sampled, bool exact);  // mk_skmer.hip
// part_meta of the super-k-mer paths, in 64-bit words: hist[p1] | start[p1 + 1] | cursor[p1] (packed 32-bit record indices in
// the space of p1 words) | khist[p1] | kstart[p1 + 1] | [p1] (a cursor array the 8-byte-key path uses) | nsurv[p1], padded
// to 7 p1 + 16; with nine regions per bucket (nseg > 1, one-word keys) start[9 p1 + 1] and cursor[9 p1] follow there
// and the two single-region arrays stay unused.
struct SkMeta {
  unsigned long long *hist, *start;
  unsigned* cursor;
  unsigned long long *khist, *kstart, *nsurv;
};
inline size_t sk_meta_words(size_t p1, int nseg) { return 7 * p1 + 16 + (nseg > 1 ? 14 * p1 + 8 : 0); }
inline size_t sk_meta_cleared_words(size_t p1) { return 7 * p1 + 8; }  // what a fresh partition zeroes: the scan writes the regions
inline SkMeta sk_meta(void* part_meta, size_t p1, int nseg) {
  SkMeta m;
  m.hist = (unsigned long long*)part_meta;
  m.start = m.hist + p1;
  m.cursor = (unsigned*)(m.start + p1 + 1);
  m.khist = m.start + p1 + 1 + p1;
  m.kstart = m.khist + p1;
  m.nsurv = m.kstart + p1 + 1 + p1;
  if (nseg > 1) {
    m.start = m.hist + sk_meta_words(p1, 1);
    m.cursor = (unsigned*)(m.start + 9 * p1 + 8);
  }
  return m;
}
// what both super-k-mer launchers plan a chunk with (mk_skmer.hip)
int sk_p1_log2(size_t seq_len, int max_log2, size_t bucket_syms);  // buckets: 256 .. 2^max_log2, about bucket_syms symbols each
int sk_sample_log2(size_t seq_len, bool exact);                    // bucket sizes from one analysis thread in 2^this
unsigned long long sk_surv_div(uint64_t min_count);                // a bucket of m k-mers has <= ceil(m / this) survivors
size_t sk_surv_cap(size_t seq_len, size_t p1, unsigned long long surv_div, int sample_log2);  // survivor buffer, in entries
struct SkQueueShape { bool three; unsigned qcap; };  // sub-tiles per tile of the queue scatters (2 or 3), items per wave queue
SkQueueShape sk_queue_shape(const mk_ctx* c);
void mk_launch_sk_scan(mk_ctx* c, const unsigned long long* hist, const unsigned long long* khist, unsigned long long* start,
                       unsigned* cursor, unsigned long long* kstart, int p1_log2, int sample_log2, int nkmax,
                       unsigned long long surv_div, unsigned long long part_cap, unsigned long long surv_cap, float sigmas,
                       int nseg);  // nseg: regions per bucket (1, or 8: one per XCD, mk_skmer.hip)
// mk_skcount.hip: the count kernel of the one-word super-k-mer path over the bucket regions the scatter filled
int mk_launch_sk_count(mk_ctx* c, const unsigned long long* start, unsigned* cursor, const unsigned long long* kstart,
                       unsigned long long* nsurv, uint64_t min_count, size_t p1, int nseg);
// nt 33 <= k <= 64, two-word keys: mk_skmer2.hip; survivors {hi,lo,count} per bucket region
int mk_launch_count_superkmer2(mk_ctx* c, size_t seq_len, uint64_t min_count, bool exact = false);
// tables (mk_table.hip); kind: MkTableKind
int mk_clear_table(mk_ctx* c, int kind, void* t, size_t slots);  // every slot free (MK_TABLE_DENSE: every bin zero)
int mk_launch_count_survivors(mk_ctx* c, uint64_t min_count);
// mk_sort.hip: arena rows (k bytes each) in byte order; *d_order = row indices, sorted (lives in c->ex_cnts2)
int mk_sort_rows(mk_ctx* c, const uint8_t* d_arena, size_t rows, int k, uint64_t** d_order);
int mk_launch_rows_by_slot(mk_ctx* c, const uint64_t* slot_keys, const uint64_t* slot_cnts, size_t rows, uint64_t* cnt_by_row, uint64_t* d_bad);
int mk_launch_rows_gather(mk_ctx* c, const uint8_t* arena, const uint64_t* order, const uint64_t* cnt_by_row, size_t rows, int k,
                          uint8_t* out_rows, uint64_t* out_cnts);
// The alpha moments of every table of c (mk_alpha_k<View>): *records records of AL_WORDS words in c->ex_tmp, one per
// workgroup, the tables in mk_each_table order and a table's workgroups in block order.
enum { AL_ROWS = 0, AL_TOTAL = 1, AL_SQ = 2 /* 3 words, low first */, AL_CLNC = 5 /* a double */, AL_FREQ = 5 /* + count, 1..10 */, AL_WORDS = 16 };
int mk_launch_alpha(mk_ctx* c, size_t* records);
int mk_launch_accumulate(mk_ctx* c, uint64_t min_count);
// every row of another one-word table (same device) added into c's running table; *new_rows counts the new keys
int mk_launch_merge_table64(mk_ctx* c, const MkSlot* from, size_t from_slots);
// the rows of one table into a fresh one (mk_rebuild_k); d_kept: only rows with count >= min_count, counted there
int mk_launch_rebuild(mk_ctx* c, int kind, const void* from, size_t from_slots, void* to, size_t to_slots, uint64_t min_count,
                      uint64_t* d_kept);
// rows as columns (two-word keys: {hi, lo} interleaved) -> the packed table; distinct: a chunk's survivors, each key once
int mk_launch_import_pairs(mk_ctx* c, const uint64_t* d_keys, const uint64_t* d_counts, size_t rows, bool distinct = false);
int mk_launch_import_regions(mk_ctx* c, const uint64_t* d_keys, const uint64_t* d_counts, const uint64_t* kstart,
                             const uint64_t* nsurv, size_t p1, size_t survivors);
int mk_launch_import_ref(mk_ctx* c, const uint8_t* d_kmers, const uint64_t* d_counts, size_t rows);
// two-word keys: survivors {hi, lo, count} per bucket region -> run128
int mk_launch_import128_regions(mk_ctx* c, const uint64_t* hi, const uint64_t* lo, const uint64_t* cnts, const uint64_t* kstart,
                                const uint64_t* nsurv, size_t p1);
// mk_table_op: one scan of x's tables with y's probed, the rows into dst's (mk_setop_k); tallies per table in d_out
enum { MK_SO_ROWS_A = 0, MK_SO_ROWS_B, MK_SO_BOTH, MK_SO_ROWS_OUT, MK_SO_TOTAL_OUT, MK_SO_WORDS = 8 };
int mk_launch_setop(mk_ctx* dst, const mk_ctx* x, const mk_ctx* y, bool scan_b, int op, bool insert, uint64_t min_x, uint64_t min_y,
                    uint64_t* d_out, uint64_t* slots);
int mk_launch_refilter_dense(mk_ctx* c, uint64_t* bins, size_t nbins, uint64_t min_count);
int mk_launch_compact128(mk_ctx* c, const MkSlot128* t, size_t slots, uint64_t* hi, uint64_t* lo, uint64_t* cnts, size_t cap,
                         uint64_t* d_cursor);
// mk_sort.hip: rows {hi[i], lo[i], cnt[i]} -> sorted by (hi, lo): keys2_out = {hi, lo} interleaved, cnts_out; scratch = 4 * n words
int mk_sort_pairs128(mk_ctx* c, const uint64_t* hi, const uint64_t* lo, const uint64_t* cnts, size_t n, int lo_bits,
                     uint64_t* scratch, uint64_t* keys2_out, uint64_t* cnts_out);
// export helpers
int mk_launch_compact(mk_ctx* c, const MkSlot* t, size_t slots, uint64_t* d_keys, uint64_t* d_counts, size_t cap,
                      uint64_t* d_cursor);
int mk_sort_pairs(mk_ctx* c, const uint64_t* keys_in, const uint64_t* vals_in, uint64_t* keys_out, uint64_t* vals_out,
                  size_t n, int key_bits);
// mk_binsort.hip: a one-word table of `rows` rows straight to sorted columns (rows binned by key prefix, bins sorted in
// LDS); *d_scal = two device words for the caller's read-back: rows found, bins too large to sort (then: the library sort)
bool mk_binsort_takes(size_t rows);
int mk_binsort_export(mk_ctx* c, const MkSlot* t, size_t slots, size_t rows, int key_bits, uint64_t* keys_out,
                      uint64_t* cnts_out, const uint64_t** d_scal);

// mk_table.hip: interleaved rows {key word(s), count} -> running table (dense: {bin, count})
int mk_launch_import_rows(mk_ctx* c, const uint64_t* d_rows, size_t rows);

// mk_bin.hip: keys of 16..26 bits counted by direct index
bool mk_binned_takes(const mk_ctx* c);
int mk_launch_count_binned(mk_ctx* c, size_t seq_len, uint64_t min_count);
// mk_tsv.hip: sorted device rows -> TSV text in c->seq
int mk_launch_tsv_format(mk_ctx* c, const uint64_t* d_keys, const uint64_t* d_cnts, size_t rows, int words, uint64_t* d_len,
                         uint64_t* d_off, size_t* text_bytes);
// mk_clean.hip
int mk_launch_clean_pre(mk_ctx* c, uint8_t* d_raw, size_t n);
int mk_launch_clean_post(mk_ctx* c, size_t seq_cap);
// mk_fastq.hip
int mk_fastq_clear(mk_ctx* c);
int mk_launch_fastq_pre(mk_ctx* c, uint8_t* d_raw, size_t n);

void mk_prof_begin(mk_ctx* c, int id);
void mk_prof_end(mk_ctx* c);
