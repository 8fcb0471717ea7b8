// mk_lookup.hip -- keys in, counts out: the read-only counterpart of the upserts (mk_lookup*, include/mercat_hip.h).
//
// What Jellyfish calls `query`: how often does this k-mer, or this panel of marker k-mers, occur in the sample whose
// table the context holds?  One kernel serves the contiguous form (row i starts at i * k) and the line form (a panel in
// text form, one key a line, its starts from the loader's line-start passes): per key it validates the row, classifies
// and packs the key as counting and mk_load_tsv place it (tl_pack_key), folds it onto its reverse complement if asked,
// probes the one table the key can live in (LkStep, mk_tableview.h) and writes counts[row].  No lists, no ranks: order is the row index.  The text form travels through the loader's piece pipeline
// (TlPieces, mk_tsvpieces.h) with the probe as the last stage of a piece where the loader has its import.
#include "mk_tsvpieces.h"
#include "mk_tableview.h"
#include <algorithm>

// LINES: row i is line i of a piece (line_start from tl_emit_k; rows = the lines looked at, at most cap), a key and
// then nothing or "\t<count>"; else row i is the k bytes at i * k and there are `rows` of them.
template <int KEYS, bool FOLD, bool LINES, int PER>
__global__ void __launch_bounds__(256) lk_probe_k(const uint8_t* __restrict__ text, const unsigned* __restrict__ line_start,
                                                  u64 rows, unsigned cap, int k, int bits, LkTables t,
                                                  u64* __restrict__ counts, TlStatus* __restrict__ st) {
  u64 n = rows;
  if (LINES) {
    const u64 lines = st->lines;
    n = lines < (u64)cap ? lines : (u64)cap;
  }
  u64 found = 0, packed = 0, textk = 0, folded = 0;
  LkStep<KEYS, PER> p;
  const u64 stride = (u64)gridDim.x * 256u;
  for (u64 first = (u64)blockIdx.x * 256u + threadIdx.x; first < n; first += stride * PER) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const u64 i = first + (u64)j * stride;
      p.clear(j);
      if (i >= n) continue;
      size_t s = (size_t)i * (size_t)k;
      bool ok = true;
      if (LINES) {
        s = line_start[i];
        const unsigned len = line_start[i + 1] - 1 - (unsigned)s;  // without the '\n'
        u64 ignored;
        ok = len == (unsigned)k || (len >= (unsigned)k + 2 && len <= (unsigned)k + 21 && text[s + k] == '\t' &&
                                    tl_count_field(text + s + k + 1, len - (unsigned)k - 1, ignored));
        if (!ok) atomicMin(&st->bad_line, i);  // (rare: the panel is refused)
      } else {
        unsigned high = 0;
        for (int q = 0; q < k; ++q) high |= text[s + q];
        if (high & 0x80u) { atomicMin(&st->bad_byte, i); ok = false; }  // (the line form: tl_count_k has looked)
      }
      if (!ok) continue;
      u64 a, b;
      if (tl_pack_key<KEYS>(text + s, k, bits, a, b)) {
        ++packed;
        if (FOLD) folded += p.fold(a, b, k) ? 1 : 0;
        p.issue(j, t, a, b);
      } else {
        ++textk;
        p.issue(j, t, BytesAt{text + s}, k);
      }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const u64 i = first + (u64)j * stride;
      if (i >= n) continue;
      const u64 cnt = p.finish(j, t);
      found += cnt ? 1 : 0;
      counts[i] = cnt;
    }
  }
  block_add(&st->found, found);
  block_add(&st->packed, packed);
  block_add(&st->text, textk);
  block_add(&st->folded, folded);
  if (p.locked) atomicAdd(&st->locked, 1ull);  // (cannot happen on a quiescent table)
}

// ------------------------------------------------------------------------------------------ host side
// The probe kernel over `rows` contiguous keys (line_start == nullptr) or over the lines of a piece, on c->stream.
static int lk_launch(mk_ctx* c, const uint8_t* d_text, const unsigned* line_start, u64 rows, unsigned cap, bool fold,
                     u64* d_counts, TlStatus* d_st) {
  const LkTables t = lk_tables(c);
  const int keys = tl_keys_of(c);
  const unsigned grid = grid_for(div_up(line_start ? (size_t)cap : (size_t)rows, LK_PER), 256, 8192);
#define LK_GO(K, F, L) hipLaunchKernelGGL((lk_probe_k<K, F, L, LK_PER>), dim3(grid), dim3(256), 0, c->stream, d_text, line_start, rows, \
                                          cap, c->k, c->bits, t, d_counts, d_st)
#define LK_FORM(K, F) do { if (line_start) LK_GO(K, F, true); else LK_GO(K, F, false); } while (0)
  // (lk_open: only nucleotide keys of one or two words fold)
  if (keys == TL_ONE_WORD) { if (fold) LK_FORM(TL_ONE_WORD, true); else LK_FORM(TL_ONE_WORD, false); }
  else if (keys == TL_TWO_WORD_NT) { if (fold) LK_FORM(TL_TWO_WORD_NT, true); else LK_FORM(TL_TWO_WORD_NT, false); }
  else if (keys == TL_TWO_WORD_AA) LK_FORM(TL_TWO_WORD_AA, false);
  else LK_FORM(TL_TEXT_ONLY, false);
#undef LK_FORM
#undef LK_GO
  MK_HIP(hipGetLastError());
  return MK_OK;
}

static int lk_locked(mk_ctx* c, const char* what) {
  c->err = std::string(what) + ": a slot of the table was being claimed: something counts into it during the lookup";
  return MK_ERR_STATE;
}

// `rows` contiguous keys in device memory probed, the figures added to out; first_key: the index of key 0 in the
// caller's list, for the message.  The stream is idle afterwards.
static int lk_rows(mk_ctx* c, const char* what, const uint8_t* d_kmers, size_t rows, size_t first_key, bool fold, u64* d_counts,
                   mk_lookup_t& out) {
  int rc;
  if ((rc = mk_buf_reserve(c, c->ex_tmp, sizeof(TlStatus))) != MK_OK) return rc;
  TlStatus* d_st = (TlStatus*)c->ex_tmp.p;
  MkTimed probe(c);
  TlStatus h{};
  MK_HIP(hipMemsetAsync(d_st, 0xFF, 16, c->stream));
  MK_HIP(hipMemsetAsync((char*)d_st + 16, 0, sizeof(TlStatus) - 16, c->stream));
  if ((rc = probe.begin()) != MK_OK || (rc = lk_launch(c, d_kmers, nullptr, (u64)rows, 0, fold, d_counts, d_st)) != MK_OK ||
      (rc = probe.end()) != MK_OK)
    return rc;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if (h.bad_byte != ~0ull) {
    c->err = std::string(what) + ": key " + std::to_string(first_key + h.bad_byte) + " holds a byte >= 0x80 (only ASCII keys are counted)";
    return MK_ERR_NON_ASCII;
  }
  if (h.locked) return lk_locked(c, what);
  out.keys += rows;
  out.found += h.found;
  out.packed_keys += h.packed;
  out.text_keys += h.text;
  out.folded += h.folded;
  return probe.add_to(out.s_probe);
}

extern "C" int mk_lookup_device(mk_ctx* c, const uint8_t* d_kmers, size_t rows, unsigned flags, uint64_t* d_counts, mk_lookup_t* st) {
  if (!c) return MK_ERR_ARG;
  const auto t0 = MkClock::now();
  if (rows && (!d_kmers || !d_counts)) { c->err = "mk_lookup_device: NULL buffer"; return MK_ERR_ARG; }
  bool fold = false;
  int rc = lk_open(c, "mk_lookup_device", flags, &fold);
  if (rc != MK_OK) return rc;
  mk_lookup_t out{};
  if (rows && (rc = lk_rows(c, "mk_lookup_device", d_kmers, rows, 0, fold, (u64*)d_counts, out)) != MK_OK) return rc;
  out.s_total = mk_since(t0);
  if (st) *st = out;
  return MK_OK;
}

// Keys in host memory: through two device buffers of the call, LK_BATCH bytes of keys at a time.
#define LK_BATCH ((size_t)64 << 20)
extern "C" int mk_lookup(mk_ctx* c, const uint8_t* kmers, size_t rows, unsigned flags, uint64_t* counts, mk_lookup_t* st) {
  if (!c) return MK_ERR_ARG;
  const auto t0 = MkClock::now();
  if (rows && (!kmers || !counts)) { c->err = "mk_lookup: NULL buffer"; return MK_ERR_ARG; }
  bool fold = false;
  int rc = lk_open(c, "mk_lookup", flags, &fold);
  if (rc != MK_OK) return rc;
  mk_lookup_t out{};
  const size_t k = (size_t)c->k, per = std::min(rows, std::max<size_t>(1, LK_BATCH / k));
  MkDevBuf d_keys, d_cnts;
  rc = [&]() -> int {
    int r;
    if (!rows) return MK_OK;
    if ((r = mk_buf_reserve(c, d_keys, per * k)) != MK_OK || (r = mk_buf_reserve(c, d_cnts, per * 8)) != MK_OK) return r;
    for (size_t at = 0; at < rows; at += per) {
      const size_t n = std::min(per, rows - at);
      const auto t1 = MkClock::now();
      MK_HIP(hipMemcpyAsync(d_keys.p, kmers + at * k, n * k, hipMemcpyHostToDevice, c->stream));
      out.s_read += mk_since(t1);
      if ((r = lk_rows(c, "mk_lookup", (const uint8_t*)d_keys.p, n, at, fold, (u64*)d_cnts.p, out)) != MK_OK) return r;
      MK_HIP(hipMemcpyAsync(counts + at, d_cnts.p, n * 8, hipMemcpyDeviceToHost, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
    }
    return MK_OK;
  }();
  (void)hipStreamSynchronize(c->stream);
  buf_free(d_keys);
  buf_free(d_cnts);
  if (rc != MK_OK) return rc;
  out.s_total = mk_since(t0);
  if (st) *st = out;
  return MK_OK;
}

// ---- the text form: the loader's pieces, probed instead of imported
struct LkText : TlPieces {
  mk_lookup_t out{};
  bool fold;
  uint64_t* counts;
  size_t cap;
  u64 rows_seen = 0;
  MkDevBuf* d_counts[2] = {&hold(), &hold()};
  LkText(mk_ctx* c_, TlSource src_, const char* what_, bool fold_, uint64_t* counts_, size_t cap_)
      : TlPieces(c_, src_, what_, true), fold(fold_), counts(counts_), cap(cap_) {}

  int reserve() override {
    int rc = MK_OK;
    for (auto* b : d_counts)
      if ((rc = mk_buf_reserve(c, *b, cap_rows * 8)) != MK_OK) return rc;
    return rc;
  }

  int enqueue_rows(int b, const uint8_t* text, const unsigned* line_start, unsigned cap_lines, TlStatus* st) override {
    return lk_launch(c, text, line_start, 0, cap_lines, fold, (u64*)d_counts[b]->p, st);
  }

  // The counts of a well formed piece go to the caller, as far as there is room (the rows are counted to the end).
  int accept(int b, const TlStatus& st, const MkChunkInfo&) override {
    if (st.locked) return lk_locked(c, what);
    if (st.lines != st.packed + st.text)
      return fail(MK_ERR_STATE, "the probe kernel lost rows (" + std::to_string(st.lines) + " lines, " +
                                    std::to_string(st.packed + st.text) + " keys)");
    if (rows_seen < cap && st.lines) {
      const size_t n = (size_t)std::min<u64>(st.lines, cap - rows_seen);
      MK_HIP(hipMemcpyAsync(counts + rows_seen, d_counts[b]->p, n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    rows_seen += st.lines;
    out.found += st.found;
    out.packed_keys += st.packed;
    out.text_keys += st.text;
    out.folded += st.folded;
    return MK_OK;
  }
};

static int lk_text(mk_ctx* c, const char* what, TlSource src, size_t total_hint, size_t piece_bytes, unsigned flags,
                   uint64_t* counts, size_t cap, size_t* rows, mk_lookup_t* st) {
  const auto t0 = MkClock::now();
  LkText L(c, src, what, false, counts, cap);  // (owns the file from here on)
  if (cap && !counts) { c->err = std::string(what) + ": counts is NULL"; return MK_ERR_ARG; }
  int rc = lk_open(c, what, flags, &L.fold);
  if (rc == MK_OK && (rc = L.setup(piece_bytes, total_hint)) == MK_OK) rc = L.run();
  (void)hipStreamSynchronize(c->stream);  // (the last piece's counts have landed)
  if (rc != MK_OK) return rc;
  if (rows) *rows = (size_t)L.rows_seen;
  if (L.rows_seen > cap) {
    c->err = std::string(what) + ": the panel holds " + std::to_string(L.rows_seen) + " rows, counts has room for " + std::to_string(cap);
    return MK_ERR_RANGE;
  }
  L.out.bytes = L.bytes;
  L.out.lines = L.lines_seen;
  L.out.keys = L.rows_seen;
  L.out.header = L.header;
  L.out.pieces = L.pieces;
  L.out.s_read = L.s_read;
  L.out.s_probe = L.s_parse;
  L.out.s_total = mk_since(t0);
  if (st) *st = L.out;
  return MK_OK;
}

extern "C" int mk_lookup_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, uint64_t* counts,
                              size_t cap, size_t* rows, mk_lookup_t* st) {
  if (!c) return MK_ERR_ARG;
  if (n && !text) { c->err = "mk_lookup_text: text is NULL"; return MK_ERR_ARG; }
  TlSource src;
  src.mem = text;
  src.n = n;
  return lk_text(c, "mk_lookup_text", src, n, piece_bytes, flags, counts, cap, rows, st);
}

extern "C" int mk_lookup_file(mk_ctx* c, const char* path, size_t piece_bytes, unsigned flags, uint64_t* counts, size_t cap,
                              size_t* rows, mk_lookup_t* st) {
  if (!c) return MK_ERR_ARG;
  if (!path) { c->err = "mk_lookup_file: path is NULL"; return MK_ERR_ARG; }
  TlSource src;
  size_t hint = 0;
  const int rc = tl_open(c, "mk_lookup_file", path, &src, &hint);
  if (rc != MK_OK) return rc;
  return lk_text(c, "mk_lookup_file", src, hint, piece_bytes, flags, counts, cap, rows, st);
}
