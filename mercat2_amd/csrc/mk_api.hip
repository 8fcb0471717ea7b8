// mk_api.hip -- the C ABI (include/mercat_hip.h): the context.  Buffers, lifetime and reset, the mode setters, shared
// tables, the chunk feed, running-table growth, mk_trim, alpha diversity, stats.
// The chunk pipeline is mk_chunk.hip, the exports mk_export.hip, the combined tables of several samples mk_combine.hip,
// the table-to-table operations mk_tableops.hip.
#include "mk_common.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

typedef unsigned long long u64;

static thread_local std::string g_err;  // errors that have no context to live in

// ------------------------------------------------------------------------------ buffers
int mk_buf_reserve(mk_ctx* c, MkDevBuf& b, size_t bytes, bool keep) {
  if (bytes <= b.cap) return MK_OK;
  size_t want = bytes;
  if (keep && b.cap) want = std::max(bytes, b.cap + b.cap / 2);
  want = (want + 255) & ~(size_t)255;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    c->err = "hipMalloc(" + std::to_string(want) + " bytes): " + hipGetErrorString(e);
    return MK_ERR_NOMEM;
  }
  if (b.p) {
    if (keep) {
      e = hipMemcpyAsync(p, b.p, b.cap, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) {
        (void)hipFree(p);
        c->err = std::string("hipMemcpy (grow): ") + hipGetErrorString(e);
        return MK_ERR_HIP;
      }
    } else {
      (void)hipStreamSynchronize(c->stream);
    }
    (void)hipFree(b.p);
  }
  b.p = p;
  b.cap = want;
  return MK_OK;
}

// ---------------------------------------------------------------------------- profiling
static hipEvent_t get_event(mk_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void mk_prof_begin(mk_ctx* c, int id) {
  if (!c->profile) return;
  MkEventPair p{get_event(c), get_event(c), id};
  (void)hipEventRecord(p.a, c->stream);
  c->events.push_back(p);
}

void mk_prof_end(mk_ctx* c) {
  if (!c->profile || c->events.empty()) return;
  (void)hipEventRecord(c->events.back().b, c->stream);
}

static void prof_collect(mk_ctx* c) {
  if (c->events.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  double* ms[MK_K_NUM] = {&c->st.ms_parse, &c->st.ms_pack, &c->st.ms_count, &c->st.ms_exotic, &c->st.ms_filter, &c->st.ms_export, &c->st.ms_part};
  uint64_t* nn[MK_K_NUM] = {&c->st.n_parse, &c->st.n_pack, &c->st.n_count, &c->st.n_exotic, &c->st.n_filter, &c->st.n_export, &c->st.n_part};
  for (auto& p : c->events) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
      *ms[p.id] += t;
      *nn[p.id] += 1;
    }
    c->event_pool.push_back(p.a);
    c->event_pool.push_back(p.b);
  }
  c->events.clear();
}

// ----------------------------------------------------------------------------- lifetime
// "mercat_hip <abi>.<minor> (gfx950)": the ABI number changes whenever a struct or a signature of include/mercat_hip.h does
// (native.py checks it against its own MK_ABI before it trusts the struct layouts)
extern "C" const char* mk_version(void) { return "mercat_hip 6.1 (gfx950)"; }

extern "C" int mk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n < 0 ? 0 : n;
}

extern "C" const char* mk_last_error(const mk_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }
void mk_set_global_error(const std::string& msg) { g_err = msg; }  // (mk_gram.hip: calls without a context)

extern "C" int mk_words_per_key(const mk_ctx* c) { return c ? (c->mode == MK_MODE_HASH128 ? 2 : 1) : 0; }

// Row totals of the last merge that were read back without waiting (mk_chunk.hip process_chunk_fast): add them up. Only call
// when the stream is known to have passed that copy.
static void fold_pending(mk_ctx* c) {
  if (!c->pending_rows) return;
  const MkChunkInfo* p = c->h_info + 1;
  mk_add_packed_rows(c, (size_t)p->new_rows);
  c->run_ref_rows += (size_t)p->new_rows_ref;
  c->pending_rows = false;
}

int mk_pull_info(mk_ctx* c) {
  if (c->clean_mode && c->clean_meta.p) MK_HIP(hipMemcpyAsync(c->h_clean, c->clean_meta.p, 8 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(c->h_info, c->info.p, sizeof(MkChunkInfo), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  fold_pending(c);  // (the stream is idle: whatever was in flight has landed)
  return MK_OK;
}

// Before anything reads run_rows & co.
int mk_settle(mk_ctx* c) {
  if (!c->pending_rows) return MK_OK;
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipStreamSynchronize(c->stream));
  fold_pending(c);
  return MK_OK;
}

// (mk_ctx::spoiled is set by the chunk pipeline, mk_chunk.hip, and cleared by a reset)
int mk_refuse_spoiled(mk_ctx* c, const char* what) {
  if (!c->spoiled) return MK_OK;
  c->err = std::string(what) + ": the running table holds part of a refused chunk (mk_reset first)";
  return MK_ERR_STATE;
}

// How every read-only call on the tables opens (mk_lookup*, mk_screen*, the inputs of mk_table_op): the arguments, then
// the table made final as mk_export_size makes it (pending row totals folded, read-backs landed) and the context's
// stream drained.  (MK_SCREEN_FOLD is MK_LOOKUP_FOLD.)
int lk_open(mk_ctx* c, const char* what, unsigned flags, bool* fold) {
  MK_REFUSE_SPOILED(c, what);
  if (c->in_chunk) { c->err = std::string(what) + ": a chunk is open"; return MK_ERR_STATE; }
  if (flags & ~MK_LOOKUP_FOLD) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  *fold = (flags & MK_LOOKUP_FOLD) != 0;
  if (*fold && !(c->canonical && c->alphabet == MK_ALPHABET_NT2 && c->k <= 64)) {
    c->err = std::string(what) + ": MK_LOOKUP_FOLD takes a canonical nucleotide context with k <= 64";
    return MK_ERR_ARG;
  }
  size_t rows = 0;
  const int rc = mk_export_size(c, &rows);
  if (rc != MK_OK) return rc;
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipStreamSynchronize(c->stream));
  return MK_OK;
}

extern "C" int mk_create(int device, int alphabet, int k, mk_ctx** out) {
  if (!out) { g_err = "mk_create: out is NULL"; return MK_ERR_ARG; }
  *out = nullptr;
  if (k < 1 || k > (1 << 20)) { g_err = "mk_create: k must be in [1, 2^20]"; return MK_ERR_ARG; }
  if (alphabet != MK_ALPHABET_NT2 && alphabet != MK_ALPHABET_AA5 && alphabet != MK_ALPHABET_RAW) {
    g_err = "mk_create: unknown alphabet";
    return MK_ERR_ARG;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_err = std::string("mk_create: no HIP device (") + (e == hipSuccess ? "0 devices" : hipGetErrorString(e)) +
            "); this engine has no CPU fallback";
    return MK_ERR_HIP;
  }
  if (device < 0 || device >= ndev) { g_err = "mk_create: device index out of range"; return MK_ERR_ARG; }
  mk_ctx* c = new (std::nothrow) mk_ctx();
  if (!c) { g_err = "mk_create: out of host memory"; return MK_ERR_NOMEM; }
  c->device = device;
  c->alphabet = alphabet;
  c->k = k;
  c->bits = alphabet == MK_ALPHABET_NT2 ? 2 : (alphabet == MK_ALPHABET_AA5 ? 5 : 0);
  c->syms_per_word = alphabet == MK_ALPHABET_NT2 ? 32 : 12;
  const long kb = (long)k * c->bits;
  c->mode = (c->bits == 0) ? MK_MODE_BYREF : (kb <= 15 ? MK_MODE_DENSE : (kb <= 64 ? MK_MODE_HASH64 : MK_MODE_BYREF));
  if (alphabet == MK_ALPHABET_NT2 && k >= 33 && k <= 64) c->mode = MK_MODE_HASH128;  // packed by-reference
  // amino acids, 13 <= k <= 25: 5 k <= 125 bits, the same two-word tables (mk_count_ref128aa_k)
  if (alphabet == MK_ALPHABET_AA5 && k >= 13 && k <= 25) c->mode = MK_MODE_HASH128;
  c->st.mode = c->mode;
  int rc = MK_OK;
  auto fail = [&](int code, const std::string& msg) {
    g_err = msg;
    mk_destroy(c);
    return code;
  };
  if ((e = hipSetDevice(device)) != hipSuccess) return fail(MK_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
    return fail(MK_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  // What a new context assumes about its first chunk (later chunks go by the chunk before): two windows per distinct key,
  // five per record.  The count kernels plan their sub-range passes from it; a bucket that does not fit is split anyway.
  // (1 and 8 -- every window a new key, full records -- made the first chunk of a read set take eight passes per bucket,
  // 1.35 ms instead of 0.3.)
  c->dup_hint = 2.0;
  c->nk_hint = 5.0;
  if ((e = hipHostMalloc((void**)&c->h_info, 2 * sizeof(MkChunkInfo) + 8 * sizeof(u64), hipHostMallocDefault)) != hipSuccess)
    return fail(MK_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  c->h_clean = (u64*)(c->h_info + 2);
  if ((rc = mk_buf_reserve(c, c->info, sizeof(MkChunkInfo) + 64)) != MK_OK) return fail(rc, c->err);
  if (c->mode == MK_MODE_DENSE) {
    const size_t bytes = ((size_t)1 << kb) * sizeof(u64);
    if ((rc = mk_buf_reserve(c, c->ctab, bytes)) != MK_OK) return fail(rc, c->err);
    if ((rc = mk_buf_reserve(c, c->run, bytes)) != MK_OK) return fail(rc, c->err);
    (void)hipMemsetAsync(c->ctab.p, 0, bytes, c->stream);
    (void)hipMemsetAsync(c->run.p, 0, bytes, c->stream);
    c->ctab_slots = c->run_slots = (size_t)1 << kb;
  }
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return fail(MK_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  *out = c;
  return MK_OK;
}

extern "C" void mk_destroy(mk_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->share_owner) (void)mk_share_table(c, nullptr);
  std::vector<mk_ctx*> sharers;
  { std::shared_lock<std::shared_mutex> rd(c->table_mu); sharers = c->sharers; }
  for (mk_ctx* s : sharers) (void)mk_share_table(s, nullptr);  // (their rows in this table go with it)
  for (auto& p : c->events) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto& e : c->event_pool) (void)hipEventDestroy(e);
  MkDevBuf* all[] = {&c->raw, &c->seq, &c->codes, &c->bad, &c->tile_maps, &c->info, &c->ctab, &c->rtab_chunk, &c->run,
                     &c->run_ref, &c->arena, &c->run128, &c->ex128, &c->ex128_out, &c->ex_keys, &c->ex_cnts, &c->ex_keys2, &c->ex_cnts2, &c->ex_tmp, &c->part, &c->part_meta, &c->surv_keys, &c->surv_cnts, &c->surv_keys2,
                     &c->xfer_out, &c->xfer_in, &c->xfer_meta, &c->clean_meta, &c->clean_runs, &c->fastq_stats, &c->fastq_tiles};
  for (auto* b : all) buf_free(*b);
  if (c->h_info) (void)hipHostFree(c->h_info);
  if (c->ingest_ring) (void)hipHostFree(c->ingest_ring);
  if (c->tsv_pin) { (void)hipHostUnregister(c->tsv_pin); free(c->tsv_pin); }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// (mk_share_table, below)
static void drain_table_users(mk_ctx* t) {  // (t->table_mu is held exclusively: nobody can launch into the table meanwhile)
  (void)hipStreamSynchronize(t->stream);
  for (mk_ctx* s : t->sharers) (void)hipStreamSynchronize(s->stream);
}

// expect_rows != 0: the packed table is also SIZED for about that many distinct keys when that is less than it has now
// (never more: growing is what the imports do) -- after a merge across GPUs an owner keeps 1/N of the rows, and a table
// that fits the caches takes the imports several times faster than the sample-sized one it had
static int reset_impl(mk_ctx* c, size_t expect_rows) {
  if (!c) return MK_ERR_ARG;
  MK_HIP(hipSetDevice(c->device));
  if (c->pending_rows) { MK_HIP(hipStreamSynchronize(c->stream)); c->pending_rows = false; }
  // (a table other contexts launch into: nobody launches while it is cleared, and what was launched has finished.  The
  // ORDER of a sharer's chunks against this reset is the caller's: reset the owner before the sharers count the next sample)
  std::unique_lock<std::shared_mutex> table_lock(c->table_mu);
  if (!c->sharers.empty()) drain_table_users(c);
  if (expect_rows && c->mode != MK_MODE_DENSE) {
    const size_t want = pow2_at_least(4 * expect_rows);
    if (c->run_slots > want) c->run_slots = want;
    if (c->run128_slots > want) c->run128_slots = want;
  }
  int rc;
  if ((rc = mk_clear_table(c, c->mode == MK_MODE_DENSE ? MK_TABLE_DENSE : MK_TABLE_ONE, c->run.p, c->run_slots)) != MK_OK) return rc;
  if ((rc = mk_clear_table(c, MK_TABLE_REF, c->run_ref.p, c->run_ref_slots)) != MK_OK) return rc;
  if ((rc = mk_clear_table(c, MK_TABLE_TWO, c->run128.p, c->run128_slots)) != MK_OK) return rc;
  c->run_rows = 0;
  c->run_ref_rows = 0;
  c->run128_rows = 0;
  c->run_side = 0;
  c->spoiled = false;
  c->in_chunk = false;
  c->raw_len = 0;
  c->part_reuse_ok = false;  // (a new sample sizes its own bucket regions: nothing is inherited across samples)
  c->dup_known = false;
  c->flat_lane = 0;  // (the next sample decides for itself, from the share of symbols this one's text had: flat_share stays)
  // (surv_hint stays, like dup_hint and nk_hint: a context that is reset counts the next sample, and the survivors of the
  // last sample's last full chunk are the best guess there is for its first chunk -- the fused launch spills what a wrong
  // guess leaves no room for.  Only a new context has no guess and hands its first chunk's survivors over through regions.)
  c->fuse_cap = 0;
  c->clean_n_runs = c->clean_n_bytes = c->clean_gc = c->clean_symbols = c->clean_raw = c->clean_headers = c->clean_last_runs = 0;
  if (c->fastq_stats.p && (rc = mk_fastq_clear(c)) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  return MK_OK;
}
extern "C" int mk_reset(mk_ctx* c) { return reset_impl(c, 0); }
extern "C" int mk_reset_for(mk_ctx* c, uint64_t expect_rows) { return reset_impl(c, (size_t)(expect_rows ? expect_rows : 1)); }

extern "C" int mk_set_canonical(mk_ctx* c, int on) {
  if (!c) return MK_ERR_ARG;
  MK_SETTLE(c);
  if (on && c->alphabet != MK_ALPHABET_NT2) { c->err = "mk_set_canonical: only the nucleotide alphabet has a reverse complement"; return MK_ERR_ARG; }
  if (on && c->mode != MK_MODE_DENSE && c->mode != MK_MODE_HASH64 && c->mode != MK_MODE_HASH128) {
    c->err = "mk_set_canonical: canonical counting is implemented for nucleotide k <= 64 (two-word keys: on the partitioned path only)";
    return MK_ERR_ARG;
  }
  c->part_reuse_ok = false;  // (bucket regions sized in the other mode are not inherited)
  if (c->in_chunk || c->run_rows || c->run_ref_rows || c->run128_rows || c->run_side || c->st.chunks) {
    if ((on != 0) != (c->canonical != 0) && (c->run_rows || c->run_ref_rows || c->run128_rows || c->run_side || c->in_chunk)) {
      c->err = "mk_set_canonical: the running table already holds rows counted in the other mode (mk_reset first)";
      return MK_ERR_STATE;
    }
  }
  c->canonical = on ? 1 : 0;
  return MK_OK;
}

extern "C" int mk_set_clean(mk_ctx* c, int on, int toupper) {
  if (!c) return MK_ERR_ARG;
  if (on && c->alphabet != MK_ALPHABET_NT2) { c->err = "mk_set_clean: removeN applies to nucleotide FASTA (bin/mercat2.py:276)"; return MK_ERR_ARG; }
  if (on && c->fastq_mode) { c->err = "mk_set_clean: FASTQ mode is on (MerCat2 does not run removeN on converted FASTQ)"; return MK_ERR_ARG; }
  if (c->in_chunk) { c->err = "mk_set_clean: a chunk is open"; return MK_ERR_STATE; }
  c->clean_mode = on ? 1 : 0;
  c->clean_upper = (on && toupper) ? 1 : 0;
  return MK_OK;
}

extern "C" int mk_set_fastq(mk_ctx* c, int on) {
  if (!c) return MK_ERR_ARG;
  if (on && c->alphabet != MK_ALPHABET_NT2) { c->err = "mk_set_fastq: FASTQ is counted as a nucleotide sample (bin/mercat2.py:290-293)"; return MK_ERR_ARG; }
  if (on && c->clean_mode) { c->err = "mk_set_fastq: clean mode is on (MerCat2 does not run removeN on converted FASTQ)"; return MK_ERR_ARG; }
  if (c->in_chunk) { c->err = "mk_set_fastq: a chunk is open"; return MK_ERR_STATE; }
  MK_HIP(hipSetDevice(c->device));
  if (on && !c->fastq_stats.p) {
    int rc = mk_fastq_clear(c);
    if (rc) return rc;
  }
  c->fastq_mode = on ? 1 : 0;
  return MK_OK;
}

extern "C" int mk_fastq_stats(mk_ctx* c, mk_fastq_stats_t* out) {
  if (!c || !out) return MK_ERR_ARG;
  u64 w[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // lines | kept headers | dropped headers | kept bytes | '\r\n' pairs (mk_fastq.hip)
  if (c->fastq_stats.p) {
    MK_HIP(hipSetDevice(c->device));
    MK_HIP(hipMemcpyAsync(w, c->fastq_stats.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
  }
  out->lines = w[0];
  out->reads = w[1];
  out->headers_dropped = w[2];
  out->fasta_bytes = w[3] - w[4];
  out->crlf = w[4];
  return MK_OK;
}

extern "C" int mk_clean_stats(mk_ctx* c, mk_clean_gpu_t* out) {
  if (!c || !out) return MK_ERR_ARG;
  out->raw_bytes = c->clean_raw;
  out->symbols = c->clean_symbols;
  out->gc_count = c->clean_gc;
  out->n_bytes = c->clean_n_bytes;
  out->n_runs = c->clean_n_runs;
  out->header_lines = c->clean_headers;
  out->last_runs = c->clean_last_runs;
  return MK_OK;
}

extern "C" int mk_clean_runs(mk_ctx* c, uint64_t* starts, uint64_t* ends, size_t cap, size_t* n) {
  if (!c || !n || (cap && (!starts || !ends))) return MK_ERR_ARG;
  // (the kernel lists run starts and run ends apart, each up to the lists' capacity: past it the two lists would not
  // hold the same runs, and pairing them by rank would invent intervals -- refuse instead of returning a wrong list)
  if ((size_t)c->clean_last_runs > ((size_t)1 << 16)) {
    *n = 0;
    c->err = "mk_clean_runs: the last chunk holds " + std::to_string(c->clean_last_runs) + " runs of N, more than the 65536 the list keeps";
    return MK_ERR_RANGE;
  }
  const size_t kept = (size_t)c->clean_last_runs;
  *n = kept;
  if (!kept || !cap) return MK_OK;
  MK_HIP(hipSetDevice(c->device));
  std::vector<u64> a(kept), b(kept);
  MK_HIP(hipMemcpyAsync(a.data(), c->clean_runs.p, kept * 8, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(b.data(), (const u64*)c->clean_runs.p + ((size_t)1 << 16), kept * 8, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  std::sort(a.begin(), a.end());  // (written in the order the waves got to them)
  std::sort(b.begin(), b.end());
  for (size_t i = 0; i < kept && i < cap; ++i) { starts[i] = a[i]; ends[i] = b[i]; }
  return MK_OK;
}

// ------------------------------------------------------------- one running table for several contexts of a GPU
// The chunks of a sample are dealt to several contexts of one GPU (HIP streams: one's kernels fill the other's gaps), and
// up to round 3 every context summed its survivors into a table of its own, the tables were summed table to table at
// the end (canonical S2: ~1 ms of the step for the second context's 9.9 M rows).  With fused launches (mk_skcount.hip)
// every access to a running table from a count kernel is an atomic, so the kernels of several streams can upsert into
// ONE table.  mk_share_table(ctx, owner): from now on the fused launches of ctx put their survivors into owner's table;
// whatever ctx still merges on its own (a new context's first chunk, spills, rows kept as text) stays in ctx's table and
// is summed at the end as before (mk_merge_from), only it is small now.  Locking: a launch that uses a shared table
// reads its pointer and size under the table's lock (shared); growing or clearing the table takes the lock exclusively,
// waits for the streams of all contexts that launch into it, and only then replaces it.
extern "C" int mk_share_table(mk_ctx* c, mk_ctx* owner) {
  if (!c || c == owner) return MK_ERR_ARG;
  if (owner) { const int rs_ = mk_refuse_spoiled(owner, "mk_share_table"); if (rs_) { c->err = owner->err; return rs_; } }
  MK_REFUSE_SPOILED(c, "mk_share_table");
  if (c->in_chunk) { c->err = "mk_share_table: a chunk is open"; return MK_ERR_STATE; }
  if (c->share_owner == owner) return MK_OK;
  if (c->share_owner) {  // leave the table it launched into
    mk_ctx* old = c->share_owner;
    std::unique_lock<std::shared_mutex> wr(old->table_mu);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    old->sharers.erase(std::remove(old->sharers.begin(), old->sharers.end(), c), old->sharers.end());
    old->n_sharers = old->sharers.size();
    c->share_owner = nullptr;
    c->fuse_target = nullptr;
  }
  if (!owner) return MK_OK;
  if (owner->share_owner || c->n_sharers) { c->err = "mk_share_table: tables are shared one level deep (the owner must own its table, a sharer cannot be an owner)"; return MK_ERR_ARG; }
  if (owner->device != c->device || owner->alphabet != c->alphabet || owner->k != c->k || owner->canonical != c->canonical || owner->mode != c->mode) {
    c->err = "mk_share_table: contexts differ in device, alphabet, k or canonical mode";
    return MK_ERR_ARG;
  }
  if (c->mode != MK_MODE_HASH64) { c->err = "mk_share_table: only one-word hashed tables are shared"; return MK_ERR_ARG; }
  // (the owner may have plain-store imports in flight, chosen while it had no sharers: they finish before this context
  // can launch into the table -- mk_launch_import_regions / mk_launch_import_pairs choose under the shared lock)
  std::unique_lock<std::shared_mutex> wr(owner->table_mu);
  (void)hipSetDevice(owner->device);
  drain_table_users(owner);
  owner->sharers.push_back(c);
  owner->n_sharers = owner->sharers.size();
  c->share_owner = owner;
  return MK_OK;
}

// ----------------------------------------------------------------------------- chunk feed
extern "C" int mk_chunk_begin(mk_ctx* c) {
  if (!c) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_chunk_begin");
  if (c->in_chunk) { c->err = "mk_chunk_begin: a chunk is already open"; return MK_ERR_STATE; }
  c->in_chunk = true;
  c->raw_len = 0;
  return MK_OK;
}

static int feed(mk_ctx* c, const uint8_t* p, size_t n, hipMemcpyKind kind) {
  if (!c) return MK_ERR_ARG;
  if (!c->in_chunk) { c->err = "mk_chunk_feed: no open chunk (call mk_chunk_begin)"; return MK_ERR_STATE; }
  if (n == 0) return MK_OK;
  if (!p) { c->err = "mk_chunk_feed: text is NULL"; return MK_ERR_ARG; }
  MK_HIP(hipSetDevice(c->device));
  int rc = mk_buf_reserve(c, c->raw, c->raw_len + n + 64, true);
  if (rc) return rc;
  MK_HIP(hipMemcpyAsync((uint8_t*)c->raw.p + c->raw_len, p, n, kind, c->stream));
  if (kind == hipMemcpyHostToDevice) MK_HIP(hipStreamSynchronize(c->stream));  // caller may reuse its buffer
  c->raw_len += n;
  return MK_OK;
}

int mk_feed_host_async(mk_ctx* c, const uint8_t* p, size_t n, bool wait) {
  if (!c || !c->in_chunk) return MK_ERR_STATE;
  if (n == 0) return MK_OK;
  MK_HIP(hipSetDevice(c->device));
  int rc = mk_buf_reserve(c, c->raw, c->raw_len + n + 64, true);
  if (rc) return rc;
  MK_HIP(hipMemcpyAsync((uint8_t*)c->raw.p + c->raw_len, p, n, hipMemcpyHostToDevice, c->stream));
  if (wait) MK_HIP(hipStreamSynchronize(c->stream));
  c->raw_len += n;
  return MK_OK;
}

int mk_reserve_raw(mk_ctx* c, size_t bytes) {
  MK_HIP(hipSetDevice(c->device));
  return mk_buf_reserve(c, c->raw, bytes, true);
}

extern "C" int mk_chunk_feed(mk_ctx* c, const uint8_t* text, size_t n) { return feed(c, text, n, hipMemcpyHostToDevice); }
extern "C" int mk_chunk_feed_device(mk_ctx* c, const uint8_t* d_text, size_t n) {
  return feed(c, d_text, n, hipMemcpyDeviceToDevice);
}

// ------------------------------------------------------------------------ running tables
// Slots of a running table that has to take need_rows rows: the next power of two above 2.5 x (load 20-40 % after a
// growth, 50 % before the next; rounds 1-2 took 4 x).  Compaction, table-to-table sums and clears scan the slots, so a
// table twice as sparse costs every sample ~0.15 ms.
static size_t run_slots_for(size_t need_rows) { return pow2_at_least(need_rows * 5 / 2); }

// The running table of one kind replaced by a fresh one of `slots` slots that holds its rows (all of them, or with kept
// those that pass min_count).  Whoever may launch into the old table has been dealt with by the caller.
int mk_rebuild_table(mk_ctx* c, int kind, size_t slots, uint64_t min_count, size_t* kept) {
  MkDevBuf& run = kind == MK_TABLE_TWO ? c->run128 : kind == MK_TABLE_REF ? c->run_ref : c->run;
  size_t& run_slots = kind == MK_TABLE_TWO ? c->run128_slots : kind == MK_TABLE_REF ? c->run_ref_slots : c->run_slots;
  u64* d_kept = kept ? (u64*)((char*)c->info.p + sizeof(MkChunkInfo)) : nullptr;
  u64 h_kept = 0;
  MkDevBuf nb;
  int rc = mk_buf_reserve(c, nb, slots * (kind == MK_TABLE_TWO ? sizeof(MkSlot128) : sizeof(MkSlot)));
  if (rc) return rc;
  if ((rc = mk_clear_table(c, kind, nb.p, slots)) != MK_OK) return rc;
  if (kept) MK_HIP(hipMemsetAsync(d_kept, 0, 8, c->stream));
  if ((rc = mk_launch_rebuild(c, kind, run.p, run_slots, nb.p, slots, min_count, (uint64_t*)d_kept)) != MK_OK) return rc;
  if (kept) MK_HIP(hipMemcpyAsync(&h_kept, d_kept, 8, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  buf_free(run);
  run = nb;
  run_slots = slots;
  if (kept) *kept = (size_t)h_kept;
  return MK_OK;
}

// (the shared table is only replaced under its lock -- a sharer may attach at any time, mk_share_table -- and with the
// streams of the contexts that launch into it drained; the other two tables are never shared)
int mk_grow_run64(mk_ctx* c, size_t need_rows) {
  std::unique_lock<std::shared_mutex> wr(c->table_mu);
  if (2 * need_rows <= c->run_slots) return MK_OK;
  if (!c->sharers.empty()) drain_table_users(c);
  return mk_rebuild_table(c, MK_TABLE_ONE, run_slots_for(need_rows));
}

int mk_grow_run128(mk_ctx* c, size_t need_rows) {
  if (2 * need_rows <= c->run128_slots) return MK_OK;
  return mk_rebuild_table(c, MK_TABLE_TWO, pow2_at_least(4 * need_rows));
}

int mk_grow_run_ref(mk_ctx* c, size_t need_rows) {
  if (need_rows > c->arena_rows_cap) {
    const size_t rows = std::max(need_rows, c->arena_rows_cap * 2);
    const int rc = mk_buf_reserve(c, c->arena, rows * (size_t)c->k + 64, true);
    if (rc) return rc;
    c->arena_rows_cap = rows;
  }
  if (2 * need_rows <= c->run_ref_slots) return MK_OK;
  return mk_rebuild_table(c, MK_TABLE_REF, pow2_at_least(4 * need_rows));
}

int mk_grow_run(mk_ctx* c, size_t more_rows) {
  if (c->mode == MK_MODE_HASH64) return mk_grow_run64(c, c->run_rows + more_rows);
  if (c->mode == MK_MODE_HASH128) return mk_grow_run128(c, c->run128_rows + more_rows);
  return MK_OK;  // dense bins are allocated once; by-reference rows have their own table
}

// ------------------------------------------------------------------------ alpha diversity
extern "C" int mk_alpha_stats(mk_ctx* c, mk_alpha_t* out) {
  if (!c || !out) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_alpha_stats");
  if (c->in_chunk) { c->err = "mk_alpha_stats: a chunk is open"; return MK_ERR_STATE; }
  MK_HIP(hipSetDevice(c->device));
  int rc;
  size_t records = 0;
  if ((rc = mk_launch_alpha(c, &records)) != MK_OK) return rc;
  std::vector<u64> h(records * AL_WORDS);
  if (records) MK_HIP(hipMemcpyAsync(h.data(), c->ex_tmp.p, h.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  memset(out, 0, sizeof *out);
  // Integers are added as integers -- sum c^2 in 192 bits: 128 for the low words, the carries out of them counted --
  // and sum c ln c record by record, as the records lie: the order is the table's, not the launch's.
  unsigned __int128 sq = 0;
  u64 sq_top = 0;
  const auto add_sq = [&](unsigned __int128 v) { sq += v; sq_top += sq < v; };
  for (size_t r = 0; r < records; ++r) {
    const u64* rec = &h[r * AL_WORDS];
    out->observed += rec[AL_ROWS];
    out->total += rec[AL_TOTAL];
    for (int i = 1; i <= 10; ++i) out->freq[i] += rec[AL_FREQ + i];
    add_sq(((unsigned __int128)rec[AL_SQ + 1] << 64) | rec[AL_SQ]);
    sq_top += rec[AL_SQ + 2];
    double clnc;
    memcpy(&clnc, &rec[AL_CLNC], 8);
    out->sum_clnc += clnc;
  }
  if (c->run_side) {  // the one key that lives beside the packed table (32 x 'T')
    const u64 v = c->run_side;
    out->observed += 1;
    out->total += v;
    if (v <= 10) out->freq[v] += 1;
    add_sq((unsigned __int128)v * v);
    out->sum_clnc += (double)v * log((double)v);
  }
  // One rounding.  Above 2^128 the low word moves into a sticky bit, far below the 53 bits that are kept.
  if (!sq_top) out->sum_sq = (double)sq;
  else out->sum_sq = ldexp((double)((((unsigned __int128)sq_top << 64) | (u64)(sq >> 64)) | ((u64)sq != 0)), 64);
  return MK_OK;
}

// Give back the per-chunk working memory (raw text, packed words, partition and survivor buffers,
// chunk tables); the running table stays, so the sample can still be exported or merged. The
// buffers come back on the next chunk.
extern "C" int mk_trim(mk_ctx* c) {
  if (!c) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_trim");
  MK_SETTLE(c);
  if (c->in_chunk) { c->err = "mk_trim: a chunk is open"; return MK_ERR_STATE; }
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipStreamSynchronize(c->stream));
  MkDevBuf* scratch[] = {&c->raw, &c->seq, &c->codes, &c->bad, &c->tile_maps, &c->ctab, &c->rtab_chunk, &c->part,
                         &c->surv_keys, &c->surv_cnts, &c->surv_keys2, &c->ex_keys, &c->ex_cnts, &c->ex_keys2, &c->ex_cnts2, &c->ex_tmp, &c->ex128, &c->ex128_out,
                         &c->xfer_out, &c->xfer_in};
  for (auto* b : scratch)
    if (!(b == &c->ctab && c->mode == MK_MODE_DENSE)) buf_free(*b);  // the dense bins are allocated once, at mk_create
  if (c->mode != MK_MODE_DENSE) c->ctab_slots = 0;
  c->rtab_chunk_slots = 0;
  c->part_reuse_ok = false;
  if (c->ingest_ring) { (void)hipHostFree(c->ingest_ring); c->ingest_ring = nullptr; c->ingest_ring_bytes = 0; }
  return MK_OK;
}

// ----------------------------------------------------------------------------------- stats
extern "C" int mk_set_profiling(mk_ctx* c, int on) {
  if (!c) return MK_ERR_ARG;
  prof_collect(c);
  c->profile = on != 0;
  c->st.profiled = c->profile ? 1 : 0;
  return MK_OK;
}

extern "C" int mk_get_stats(mk_ctx* c, mk_stats_t* out) {
  if (!c || !out) return MK_ERR_ARG;
  MK_SETTLE(c);
  (void)hipSetDevice(c->device);
  prof_collect(c);
  c->st.mode = c->mode;
  if (c->mode != MK_MODE_DENSE) c->st.rows = mk_total_rows(c);
  *out = c->st;
  return MK_OK;
}

extern "C" int mk_reset_stats(mk_ctx* c) {
  if (!c) return MK_ERR_ARG;
  prof_collect(c);
  const int mode = c->st.mode, prof = c->st.profiled;
  c->st = mk_stats_t{};
  c->st.mode = mode;
  c->st.profiled = prof;
  return MK_OK;
}
