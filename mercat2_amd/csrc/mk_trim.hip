// mk_trim.hip -- sequences in, every record cut in front of its first low-abundance k-mer out (mk_trim_text /
// mk_trim_device, include/mercat_hip.h): khmer's trim_on_abundance on the GPU, where the text, the parsed stream and the
// rows already are.
//
// A piece goes through sc_piece (mk_screenpiece.h: parse, record scan, probe) and leaves its rows on the device.  Then
//   fl_tiles_k / fl_scan_k / fl_starts_k   start[r]: the first byte of every row's header line in the RAW text
//                                          (mk_recordplace.h), under the filter's guard: the header lines found must be
//                                          the parser's separators
//   tk_starts_k                            sstart[r]: where the row's symbols start in the parsed stream (mk_screenwalk.h)
//   tr_hend_k                              a lane per record: hlen[r], the bytes of its header line, terminator included
//   tr_first_k                             the walk of mk_screenwalk.h with a sink that keeps, per record, the smallest
//                                          index of a window whose count is below at_least: first_low[r], ~0 where none
//                                          is.  Skipped for a piece whose every window is a hit.
//   tr_decide_k                            a lane per record: kept[r] by the rule, len[r] = hlen + kept + 1 or 0
//   rocprim::exclusive_scan                dst[r], dst[nrows] = the piece's output length
//   tr_gather_k (tr_edges_k)               fl_gather_k's form -- a lane owns 16 aligned output bytes, a wave instruction
//                                          writes 1 KiB, one search of dst[] per wave -- with two sources a record: the
//                                          header line from the raw text, the kept symbols from the stream, then one LF
#include "mk_recordplace.h"
#include "mk_screenwalk.h"
#include <rocprim/device/device_scan.hpp>

struct TrStatus {  // device memory, read back once a piece (fl: what the start kernels found)
  FlStatus fl;
  u64 records_out, records_trimmed, bases_out;
  u64 disagree;  // records whose first_low contradicts their row
  u64 outside;   // low windows the walk met in a record, or at an index, the placement did not count
};

// hlen[r] = bytes of row r's header line: from start[r] through its terminator (LF, CR LF or a lone CR), or to the end
// of the text.  A headless row 0 has none.  A start outside the text (the host's guard reports what caused it) reads
// nothing.
__global__ void __launch_bounds__(256) tr_hend_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ start, size_t nrows,
                                                 int headless, u64* __restrict__ hlen) {
  mk_for_each(nrows, [&](size_t r) {
    const u64 s = start[r];
    if ((headless && r == 0) || s >= n) { hlen[r] = 0; return; }
    u64 p = s;
    while (p < n && !mk_is_nl(text[p])) ++p;
    if (p < n) p += (text[p] == 13u && p + 1 < n && text[p + 1] == 10u) ? 2 : 1;
    hlen[r] = p - s;
  });
}

// The sink of the walk that looks for the first low window of every record.  best: the smallest record-relative index
// of a low window of the record the lane is in (its positions ascend: the first it meets).  It leaves for first_low[r]
// by atomicMin where the record ends among the lane's window starts; what the lane still holds when its run ends
// belongs to the record it ends in (tr_first_k).
struct TrSink {
  const u64* __restrict__ sstart;
  const mk_screen_row_t* __restrict__ rows;
  u64* __restrict__ first_low;
  u64 row_base, nrows, at_least;
  u64 at_rid0 = ~0ull, ahead = 0;  // the record the lane's run started in; its symbols in front of the run
  u64 best = ~0ull, outside = 0;
  __device__ __forceinline__ void begin(u64 rid, u64 at) {
    const u64 r = rid - row_base;
    if (r < nrows && sstart[r] <= at) ahead = at - sstart[r];
    at_rid0 = rid;
  }
  // One record can span millions of lanes: the atomic is issued only where the candidate is below what a plain load
  // shows (the value only falls, so a stale read costs an atomic, never a result).
  __device__ __forceinline__ void flush(u64 rid) {
    if (best == ~0ull) return;
    const u64 r = rid - row_base;
    if (r < nrows && best < rows[r].windows) {
      if (best < first_low[r]) atomicMin((unsigned long long*)&first_low[r], (unsigned long long)best);
    } else ++outside;
    best = ~0ull;
  }
  __device__ __forceinline__ void record_end(u64 rid) { flush(rid); }
  __device__ __forceinline__ void window(u64 rid, unsigned pos, u64 cnt) {
    if (cnt < at_least && best == ~0ull) best = (rid == at_rid0 ? ahead : 0) + pos;
  }
};

// Grid, arguments and dynamic LDS of sc_probe_k.
template <int KEYS, bool FOLD, bool LDS>
__global__ void __launch_bounds__(256) tr_first_k(const uint8_t* __restrict__ seq, u64 seq_len, const u64* __restrict__ tile_pre,
                                                  u64 row_base, int k, int bits, u64 at_least, LkTables t,
                                                  const u64* __restrict__ sstart, const mk_screen_row_t* __restrict__ rows, u64 nrows,
                                                  u64* __restrict__ first_low, TrStatus* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_seq[];  // sc_span_bytes(k)
  TrSink sink{sstart, rows, first_low, row_base, nrows, at_least};
  ScWalked n;
  const u64 rid = sc_walk<KEYS, FOLD, LDS>(s_seq, seq, seq_len, tile_pre, k, bits, t, sink, n);
  // The whole wave ends in one record (the normal case inside a contig): the smallest of the wave, one lane flushes.
  if (__all(rid == __shfl(rid, 0))) {
    for (int d = 32; d > 0; d >>= 1) {
      const u64 o = __shfl_down(sink.best, d);
      sink.best = o < sink.best ? o : sink.best;
    }
    if (threadIdx.x & 63) sink.best = ~0ull;
  }
  sink.flush(rid);
  block_add(&st->outside, sink.outside);
}

// A lane per record (and one for the slot behind the last, whose length is 0 so that the scan ends in the total).
__global__ void __launch_bounds__(256) tr_decide_k(const mk_screen_row_t* __restrict__ rows, const u64* __restrict__ first_low,
                                                   const u64* __restrict__ hlen, size_t nrows, u64 k, u64 min_len,
                                                   u64* __restrict__ kept, u64* __restrict__ len, TrStatus* __restrict__ st) {
  u64 out = 0, trimmed = 0, bases = 0, bad = 0;
  mk_for_each(nrows + 1, [&](size_t r) {
    if (r == nrows) { len[r] = 0; return; }
    const u64 windows = rows[r].windows, hits = rows[r].hits, fl = first_low[r];
    const bool none = fl == ~0ull;
    bad += (none != (hits == windows)) ? 1 : 0;
    bad += (!none && fl >= windows) ? 1 : 0;
    const u64 L = windows ? windows + k - 1 : 0;  // (a record without windows keeps nothing, whatever it holds)
    u64 kp = none ? L : (fl ? fl + k - 1 : 0);
    if (kp > L) kp = L;  // (only with a disagreement, which the host reports)
    if (kp < (min_len > k ? min_len : k)) kp = 0;
    kept[r] = kp;
    len[r] = kp ? hlen[r] + kp + 1 : 0;
    out += kp ? 1 : 0;
    trimmed += (kp && kp < L) ? 1 : 0;
    bases += kp;
  });
  block_add(&st->records_out, out);
  block_add(&st->records_trimmed, trimmed);
  block_add(&st->bases_out, bases);
  block_add(&st->disagree, bad);
}

// What the gather knows of a record: where its output starts, its two sources and their lengths.
struct TrRec {
  u64 at, hsrc, h, ssrc, body;  // dst[r]; start[r], hlen[r]; sstart[r], hlen[r] + kept[r]: the LF stands at offset body
};
struct TrPlace {
  const uint8_t* __restrict__ text;
  u64 n;
  const uint8_t* __restrict__ seq;
  u64 seq_len;
  const u64* __restrict__ start;
  const u64* __restrict__ sstart;
  const u64* __restrict__ hlen;
  const u64* __restrict__ kept;
  const u64* __restrict__ dst;
  size_t nrows;
  __device__ __forceinline__ TrRec rec(size_t r) const {
    const u64 h = hlen[r];
    return TrRec{dst[r], start[r], h, sstart[r], h + kept[r]};
  }
};

// Chunks, rounds and the search as in fl_gather_k.  A chunk is filled segment by segment: up to 16 bytes of the header
// line (raw text), of the kept symbols (stream), or the LF, masked to what the segment still has and shifted to their
// place; the record after an LF is r + 1, or the next emitted one.  An emitted record holds k + 1 bytes or more, so a
// chunk sees at most sixteen segments.
#define TR_CHUNKS 4
__global__ void __launch_bounds__(256) tr_gather_k(TrPlace p, u64 head, u64 nbody, uint8_t* __restrict__ out) {
  const u64 g0 = fl_first_lane((((u64)blockIdx.x * 256 + threadIdx.x) >> 6) * (64 * TR_CHUNKS));
  if (g0 >= nbody) return;
  size_t r = fl_record_of(p.dst, 0, p.nrows - 1, head + 16 * g0);
  for (int j = 0; j < TR_CHUNKS; ++j) {
    const u64 g = g0 + j * 64 + (threadIdx.x & 63);
    if (g >= nbody) break;
    const u64 o0 = head + 16 * g;
    r = fl_record_from(p.dst, r, p.nrows, o0);
    TrRec c = p.rec(r);
    unsigned __int128 v = 0;
    for (unsigned b = 0;;) {  // b: bytes of the chunk filled
      const u64 q = o0 + b - c.at;  // (at most body: the record holds byte o0 + b)
      unsigned __int128 seg;
      u64 left;
      if (q < c.h) { seg = fl_load16(p.text, p.n, c.hsrc + q); left = c.h - q; }
      else if (q < c.body) { seg = fl_load16(p.seq, p.seq_len, c.ssrc + (q - c.h)); left = c.body - q; }
      else { seg = 10u; left = 1; }
      const unsigned m = left < 16 - b ? (unsigned)left : 16 - b;
      if (m < 16) seg &= (((unsigned __int128)1) << (8 * m)) - 1;
      v |= seg << (8 * b);
      b += m;
      if (b == 16) break;
      if (q + m <= c.body) continue;  // (the LF was not among them: the same record goes on)
      ++r;  // the record ended inside the chunk (bytes follow: an emitted record does)
      if (p.dst[r + 1] == p.dst[r]) r = fl_record_from(p.dst, r, p.nrows, o0 + b);
      c = p.rec(r);
    }
    const u64 v0 = (u64)v, v1 = (u64)(v >> 64);
    *reinterpret_cast<uint4*>(out + o0) = make_uint4((unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32));
  }
}

// The bytes in front of the first aligned 16 of the output (head of them) and behind the last (from tail_at on): a lane
// a byte, at most 15 + 15.
__global__ void __launch_bounds__(64) tr_edges_k(TrPlace p, u64 head, u64 tail_at, u64 out_len, uint8_t* __restrict__ out) {
  u64 o;
  if (threadIdx.x < 16) o = threadIdx.x < head ? threadIdx.x : out_len;
  else if (threadIdx.x < 32) o = tail_at + (threadIdx.x - 16);
  else return;
  if (o >= out_len) return;
  const TrRec c = p.rec(fl_record_of(p.dst, 0, p.nrows - 1, o));
  const u64 q = o - c.at;
  out[o] = q < c.h ? p.text[c.hsrc + q] : q < c.body ? p.seq[c.ssrc + (q - c.h)] : (uint8_t)10;
}

// ------------------------------------------------------------------------------------------ host side
struct TrCall {
  mk_trim_rule_t rule;
  uint8_t* out;       // where the output goes (text call: host memory, device call: device memory), out_cap bytes of room
  size_t out_cap;
  uint64_t* kept;     // the caller's, or nullptr; cap of each
  mk_screen_row_t* rows;
  size_t cap;
  bool device;        // out / kept / rows are device memory
  MkDevBuf d_rows, meta, scan_tmp, stage;
  MkTimed place, first, gather;
  mk_trim_t st{};
  size_t bytes_out = 0;  // of all pieces so far, written or not
  TrCall(mk_ctx* c, const mk_trim_rule_t& r, uint8_t* o, size_t oc, uint64_t* kp, mk_screen_row_t* rw, size_t cp, bool dev)
      : rule(r), out(o), out_cap(oc), kept(kp), rows(rw), cap(cp), device(dev), place(c), first(c), gather(c) {}
  ~TrCall() {
    for (MkDevBuf* b : {&d_rows, &meta, &scan_tmp, &stage}) buf_free(*b);
  }
};

static int tr_launch_first(ScCall& s, const u64* sstart, const mk_screen_row_t* d_rows, size_t nrows, u64* first_low, TrStatus* d_st) {
  mk_ctx* c = s.c;
  const LkTables t = lk_tables(c);
  const unsigned grid = (unsigned)div_up(s.last.seq_len, SC_SPAN);
  sc_dispatch_walk(s, [&](auto keys, auto fold, auto lds) {
    hipLaunchKernelGGL((tr_first_k<decltype(keys)::value, decltype(fold)::value, decltype(lds)::value>), dim3(grid), dim3(256),
                       decltype(lds)::value ? sc_span_bytes(c->k) : 0, c->stream, (const uint8_t*)c->seq.p, (u64)s.last.seq_len,
                       s.last.tile_pre, s.last.row_base, c->k, c->bits, s.at_least, t, sstart, d_rows, (u64)nrows, first_low, d_st);
    return MK_OK;
  });
  MK_HIP(hipGetLastError());
  return MK_OK;
}

// What follows sc_piece for a piece of n bytes whose rows start at row `first` of the call and whose windows are all
// hits iff all_hits: placement, the first low window, decision, gather, and the copies to the caller's buffers where
// they have room.  The stream is idle afterwards.
static int tr_piece(ScCall& s, TrCall& f, size_t n, size_t first, bool all_hits) {
  mk_ctx* c = s.c;
  int rc;
  const size_t nrows = s.last.nrows;
  if (!nrows) {  // (no header line, no kept character)
    f.st.preamble += n;
    return MK_OK;
  }
  const uint8_t* text = s.last.text;
  const mk_screen_row_t* d_rows = s.last.d_rows;
  const size_t ntiles = div_up(n, FL_SPAN), seq_len = s.last.seq_len;
  const int headless = s.last.headless ? 1 : 0;
  // meta: TrStatus (64) | start[nrows + 1] | len[nrows + 1] | dst[nrows + 1] | sstart | hlen | first_low | kept [nrows]
  //       each | tile_pre[ntiles] | tile_cnt[ntiles]
  static_assert(sizeof(TrStatus) <= 64, "TrStatus");
  if ((rc = mk_buf_reserve(c, f.meta, 64 + (3 * (nrows + 1) + 4 * nrows + ntiles) * sizeof(u64) + ntiles * sizeof(unsigned))) != MK_OK) return rc;
  TrStatus* d_st = (TrStatus*)f.meta.p;
  u64* start = (u64*)((char*)f.meta.p + 64);
  u64* len = start + nrows + 1;
  u64* dst = len + nrows + 1;
  u64* sstart = dst + nrows + 1;
  u64* hlen = sstart + nrows;
  u64* first_low = hlen + nrows;
  u64* d_kept = first_low + nrows;
  u64* tile_pre = d_kept + nrows;
  unsigned* tile_cnt = (unsigned*)(tile_pre + ntiles);
  size_t tmp = 0;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  MK_HIP(hipMemsetAsync(d_st, 0, sizeof(TrStatus), c->stream));
  MK_HIP(hipMemsetAsync(start, 0xFF, (nrows + 1) * sizeof(u64), c->stream));  // (a start no header line gives reads as outside the text)
  MK_HIP(hipMemsetAsync(sstart, 0xFF, nrows * sizeof(u64), c->stream));
  MK_HIP(hipMemsetAsync(first_low, 0xFF, nrows * sizeof(u64), c->stream));
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fl_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fl_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, (u64)n, nrows, headless,
                     start, &d_st->fl);
  hipLaunchKernelGGL(fl_starts_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, (const u64*)tile_pre, (u64)headless,
                     nrows, start);
  hipLaunchKernelGGL(tr_hend_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, text, (u64)n, (const u64*)start, nrows,
                     headless, hlen);
  if (seq_len)
    hipLaunchKernelGGL(tk_starts_k, dim3((unsigned)div_up(seq_len, SC_SPAN)), dim3(256), 0, c->stream, (const uint8_t*)c->seq.p,
                       (u64)seq_len, s.last.tile_pre, s.last.row_base, nrows, sstart);
  MK_HIP(hipGetLastError());
  if ((rc = f.place.end()) != MK_OK) return rc;

  if (!all_hits && seq_len) {
    if ((rc = f.first.begin()) != MK_OK) return rc;
    if ((rc = tr_launch_first(s, sstart, d_rows, nrows, first_low, d_st)) != MK_OK) return rc;
    if ((rc = f.first.end()) != MK_OK) return rc;
  }
  // (the lengths are only added up before the guards below have passed: no address is made of them)
  hipLaunchKernelGGL(tr_decide_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, (const u64*)first_low,
                     (const u64*)hlen, nrows, (u64)c->k, (u64)f.rule.min_len, d_kept, len, d_st);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  TrStatus h{};
  u64 piece_out = 0, start0 = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&start0, start, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (!all_hits && seq_len && (rc = f.first.add_to(f.st.s_first)) != MK_OK) return rc;
  if (h.fl.headers + headless != nrows) {
    c->err = std::string(s.what) + ": " + std::to_string(h.fl.headers) + " header lines in the text, " +
             std::to_string(nrows - headless) + " in the parsed stream (internal error)";
    return MK_ERR_STATE;
  }
  if (h.disagree || h.outside) {
    c->err = std::string(s.what) + ": the first low window of " + std::to_string(h.disagree) + " record(s) contradicts their rows, " +
             std::to_string(h.outside) + " low window(s) outside the placement (internal error)";
    return MK_ERR_STATE;
  }
  if (start0 > n || piece_out > n - start0 + 1) {
    c->err = std::string(s.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.preamble += start0;
  f.st.records_out += h.records_out;
  f.st.records_trimmed += h.records_trimmed;
  f.st.records_dropped += nrows - h.records_out;
  f.st.bases_in += seq_len - (nrows - headless);  // (the stream: the kept characters and one separator a header line)
  f.st.bases_out += h.bases_out;
  const size_t at = f.bytes_out;
  f.bytes_out += (size_t)piece_out;

  // kept and rows of the piece, where the caller has room for them
  if (first + nrows <= f.cap) {
    const auto t1 = MkClock::now();
    const hipMemcpyKind kind = f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + first, d_rows, nrows * sizeof(mk_screen_row_t), kind, c->stream));
    if (f.kept) MK_HIP(hipMemcpyAsync(f.kept + first, d_kept, nrows * sizeof(u64), kind, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }
  if (!piece_out || f.bytes_out > f.out_cap) return MK_OK;  // (no room: the call goes on adding up and answers MK_ERR_RANGE)

  // the gather: into the caller's device memory, or into a staging buffer that is copied to the host
  uint8_t* d_out = f.out + at;
  if (!f.device) {
    if ((rc = mk_buf_reserve(c, f.stage, (size_t)piece_out)) != MK_OK) return rc;
    d_out = (uint8_t*)f.stage.p;
  }
  const TrPlace p{text, (u64)n, (const uint8_t*)c->seq.p, (u64)seq_len, start, sstart, hlen, d_kept, dst, nrows};
  const u64 head = std::min<u64>((16 - ((uintptr_t)d_out & 15)) & 15, piece_out);
  const u64 nbody = (piece_out - head) / 16, tail_at = head + 16 * nbody;
  if ((rc = f.gather.begin()) != MK_OK) return rc;
  if (nbody)
    hipLaunchKernelGGL(tr_gather_k, dim3((unsigned)div_up((size_t)nbody, 256 * TR_CHUNKS)), dim3(256), 0, c->stream, p, head, nbody, d_out);
  if (head || tail_at < piece_out) hipLaunchKernelGGL(tr_edges_k, dim3(1), dim3(64), 0, c->stream, p, head, tail_at, piece_out, d_out);
  MK_HIP(hipGetLastError());
  if ((rc = f.gather.end()) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.gather.add_to(f.st.s_gather)) != MK_OK) return rc;
  if (!f.device) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(f.out + at, d_out, (size_t)piece_out, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }
  return MK_OK;
}

// sc_piece, then tr_piece with what that piece added to the call's windows and hits.
static int tr_both(ScCall& s, TrCall& f, const uint8_t* d_piece, size_t len, size_t first) {
  const u64 w0 = s.out.windows, h0 = s.out.hits;
  const int rc = sc_piece(s, d_piece, len, nullptr, ~(size_t)0, &f.d_rows, nullptr);
  return rc != MK_OK ? rc : tr_piece(s, f, len, first, s.out.windows - w0 == s.out.hits - h0);
}

// How both calls check their own arguments, open as the screen calls open, and end; body(s): the pieces.
template <class Body>
static int tr_run(mk_ctx* c, const char* what, unsigned flags, const mk_trim_rule_t* rule, TrCall* f, size_t* out_len, size_t* nrows,
                  mk_trim_t* st, Body&& body) {
  if (!rule) { c->err = std::string(what) + ": rule is NULL"; return MK_ERR_ARG; }
  if (flags & ~MK_TRIM_FOLD) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  if (rule->at_least < 1) { c->err = std::string(what) + ": at_least must be 1 or more"; return MK_ERR_ARG; }
  const size_t cap = (f->rows || f->kept) ? f->cap : ~(size_t)0;
  f->cap = cap;
  int rc = sc_run(c, what, flags & MK_TRIM_FOLD, rule->at_least, cap, nrows, &f->st.screen, [&](ScCall& s) { return body(s); });
  if (rc != MK_OK && rc != MK_ERR_RANGE) return rc;
  if (out_len) *out_len = f->bytes_out;
  if (rc != MK_OK) return rc;
  if (f->bytes_out > f->out_cap) {
    c->err = std::string(what) + ": the output holds " + std::to_string(f->bytes_out) + " bytes, out has room for " + std::to_string(f->out_cap);
    return MK_ERR_RANGE;
  }
  f->st.bytes_out = f->bytes_out;
  if (st) *st = f->st;
  return MK_OK;
}

extern "C" int mk_trim_device(mk_ctx* c, const uint8_t* d_text, size_t n, unsigned flags, const mk_trim_rule_t* rule, uint8_t* d_out,
                              size_t out_cap, size_t* out_len, uint64_t* d_kept, mk_screen_row_t* d_rows, size_t cap, size_t* nrows,
                              mk_trim_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (out_cap && !d_out)) { c->err = "mk_trim_device: NULL buffer"; return MK_ERR_ARG; }
  if (((uintptr_t)d_kept | (uintptr_t)d_rows) & 7) { c->err = "mk_trim_device: kept and rows must be aligned to 8"; return MK_ERR_ARG; }
  TrCall f(c, rule ? *rule : mk_trim_rule_t{}, d_out, out_cap, d_kept, d_rows, cap, true);
  return tr_run(c, "mk_trim_device", flags, rule, &f, out_len, nrows, st,
                [&](ScCall& s) -> int { return n ? tr_both(s, f, d_text, n, 0) : MK_OK; });
}

extern "C" int mk_trim_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_trim_rule_t* rule,
                            uint8_t* out, size_t out_cap, size_t* out_len, uint64_t* kept, mk_screen_row_t* rows, size_t cap,
                            size_t* nrows, mk_trim_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (out_cap && !out)) { c->err = "mk_trim_text: NULL buffer"; return MK_ERR_ARG; }
  TrCall f(c, rule ? *rule : mk_trim_rule_t{}, out, out_cap, kept, rows, cap, false);
  return tr_run(c, "mk_trim_text", flags, rule, &f, out_len, nrows, st, [&](ScCall& s) -> int {
    return sc_text_pieces(s, text, n, piece_bytes,
                          [&](const uint8_t* d_piece, size_t len) -> int { return tr_both(s, f, d_piece, len, s.rows_seen); });
  });
}
