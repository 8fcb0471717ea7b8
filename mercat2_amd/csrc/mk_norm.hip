// mk_norm.hip -- sequences in, the reads thinned to a target depth out (mk_norm_text / mk_norm_device,
// include/mercat_hip.h): digital normalisation by the median of every record's k-mer counts, the consumer on the GPU of
// what mk_track_* computes.  The counts never leave the device: the answer is one bit a record and a text shorter than
// the input.
//
// A piece goes through sc_piece (mk_screenpiece.h: parse, record scan, probe) and leaves its rows on the device.  Then
//   tk_lens_k + scan, tk_starts_k          woff[], sstart[]: the track's placement (mk_trackwalk.h, mk_screenwalk.h);
//   tk_longest_k                           whether the piece holds a long record
//   fl_tiles_k / fl_scan_k / fl_starts_k   start[r]: the filter's record starts in the RAW text (mk_recordplace.h), under
//                                          its guard: the header lines found must be the parser's separators
//   tk_probe_k<..., uint32_t>              the track kernel, into device scratch
//   tk_median                              med[r]: sorted and picked, or selected for a long record (mk_trackwalk.h)
//   nm_decide_k                            a lane a record: its class, keep[r], the kept length, the five record counts,
//                                          and the records whose median contradicts their row
//   rocprim::exclusive_scan                dst[r], dst[nrows] = the piece's output length
//   fl_emit: fl_gather_k (fl_edges_k)      the filter's output under another decision (mk_recordplace.h)
#include "mk_recordplace.h"
#include "mk_trackwalk.h"

struct NmStatus {  // device memory, read back once a piece (fl: what the start kernels found; its records_out: emitted)
  FlStatus fl;
  u64 records_short, records_low, records_over, records_thinned;
  u64 disagree;  // records whose median contradicts their row
};

// A lane per record (and one for the slot behind the last, whose length is 0 so that the scan ends in the total).
// first: the index over the whole call of the piece's row 0.
__global__ void __launch_bounds__(256) nm_decide_k(const mk_screen_row_t* __restrict__ rows, const u64* __restrict__ start,
                                                   const uint32_t* __restrict__ med, size_t nrows, u64 first, u64 target, u64 min_depth,
                                                   u64 seed, bool invert, uint8_t* __restrict__ keep, u64* __restrict__ len,
                                                   NmStatus* __restrict__ st) {
  u64 out = 0, n_short = 0, n_low = 0, n_over = 0, n_thin = 0, bad = 0;
  mk_for_each(nrows + 1, [&](size_t r) {
    if (r == nrows) { len[r] = 0; return; }
    const u64 windows = rows[r].windows, m = med[r];
    const u64 clip = 0xFFFFFFFFull;  // (the row's counts are not clipped, the median's are)
    const u64 low_end = rows[r].min < clip ? rows[r].min : clip, top = rows[r].max < clip ? rows[r].max : clip;
    bad += (windows ? (m < low_end || m > top) : m != 0) ? 1 : 0;
    const bool is_short = windows == 0, low = !is_short && m < min_depth, over = !is_short && !low && m > target;
    const bool kept = !is_short && !low && (!over || nm_u(seed, first + r) * m < (target << 32));
    const bool emit = kept != invert;
    keep[r] = emit ? 1 : 0;
    len[r] = emit ? start[r + 1] - start[r] : 0;
    out += emit ? 1 : 0;
    n_short += is_short ? 1 : 0;
    n_low += low ? 1 : 0;
    n_over += over ? 1 : 0;
    n_thin += (over && !kept) ? 1 : 0;
  });
  block_add(&st->fl.records_out, out);
  block_add(&st->records_short, n_short);
  block_add(&st->records_low, n_low);
  block_add(&st->records_over, n_over);
  block_add(&st->records_thinned, n_thin);
  block_add(&st->disagree, bad);
}

// ------------------------------------------------------------------------------------------ host side
struct NmCall {
  mk_norm_rule_t rule;
  bool invert;
  FlEmit emit;          // where the output goes
  uint32_t* median;     // the caller's, or nullptr; cap of each
  uint8_t* keep;
  mk_screen_row_t* rows;
  size_t cap;
  bool device;          // out / median / keep / rows are device memory
  MkDevBuf d_rows, d_keep, d_med, counts, meta, scan_tmp;
  TkMedian med;
  MkTimed place, track, sort;
  mk_norm_t st{};
  NmCall(mk_ctx* c, const mk_norm_rule_t& r, bool inv, uint8_t* o, size_t oc, uint32_t* md, uint8_t* kp, mk_screen_row_t* rw, size_t cp,
         bool dev)
      : rule(r), invert(inv), emit(c, o, oc, dev), median(md), keep(kp), rows(rw), cap(cp), device(dev), place(c), track(c), sort(c) {}
  ~NmCall() {
    for (MkDevBuf* b : {&d_rows, &d_keep, &d_med, &counts, &meta, &scan_tmp}) buf_free(*b);
  }
};

// What follows sc_piece for a piece of n bytes whose rows start at row `first` of the call: placement, the track into
// scratch, the medians, the decision, the gather, and the copies to the caller's buffers where they have room.  The
// stream is idle afterwards.
static int nm_piece(ScCall& s, NmCall& f, size_t n, size_t first) {
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
  // meta: NmStatus (64) | TkStatus (32) | start | len | dst | wlen | woff [nrows + 1] each | sstart[nrows] |
  //       tile_pre[ntiles] | tile_cnt[ntiles]
  static_assert(sizeof(NmStatus) <= 64 && sizeof(TkStatus) <= 32, "NmStatus");
  if ((rc = mk_buf_reserve(c, f.meta, 96 + (5 * (nrows + 1) + nrows + ntiles) * sizeof(u64) + ntiles * sizeof(unsigned))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, f.d_keep, nrows)) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, f.d_med, nrows * sizeof(uint32_t))) != MK_OK) return rc;
  NmStatus* d_st = (NmStatus*)f.meta.p;
  TkStatus* d_tk = (TkStatus*)((char*)f.meta.p + 64);
  u64* start = (u64*)((char*)f.meta.p + 96);
  u64* len = start + nrows + 1;
  u64* dst = len + nrows + 1;
  u64* wlen = dst + nrows + 1;
  u64* woff = wlen + nrows + 1;
  u64* sstart = woff + nrows + 1;
  u64* tile_pre = sstart + nrows;
  unsigned* tile_cnt = (unsigned*)(tile_pre + ntiles);
  uint8_t* d_keep = (uint8_t*)f.d_keep.p;
  uint32_t* d_med = (uint32_t*)f.d_med.p;
  size_t tmp = 0;  // (both scans are of nrows + 1 uint64_t)
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  MK_HIP(hipMemsetAsync(f.meta.p, 0, 96, c->stream));
  MK_HIP(hipMemsetAsync(start, 0xFF, (nrows + 1) * sizeof(u64), c->stream));  // (a start no header line gives reads as outside the text)
  MK_HIP(hipMemsetAsync(sstart, 0xFF, nrows * sizeof(u64), c->stream));
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(tk_lens_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, nrows, wlen, d_tk);
  if (seq_len)
    hipLaunchKernelGGL(tk_starts_k, dim3((unsigned)div_up(seq_len, SC_SPAN)), dim3(256), 0, c->stream, (const uint8_t*)c->seq.p,
                       (u64)seq_len, s.last.tile_pre, s.last.row_base, nrows, sstart);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)wlen, woff, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  hipLaunchKernelGGL(tk_longest_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, (const u64*)woff, nrows, d_tk);
  hipLaunchKernelGGL(fl_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fl_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, (u64)n, nrows, headless,
                     start, &d_st->fl);
  hipLaunchKernelGGL(fl_starts_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, (const u64*)tile_pre, (u64)headless,
                     nrows, start);
  MK_HIP(hipGetLastError());
  if ((rc = f.place.end()) != MK_OK) return rc;
  NmStatus h{};
  TkStatus ht{};
  u64 total = 0, start0 = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&ht, d_tk, sizeof ht, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&total, woff + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&start0, start, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (h.fl.headers + headless != nrows) {
    c->err = std::string(s.what) + ": " + std::to_string(h.fl.headers) + " header lines in the text, " +
             std::to_string(nrows - headless) + " in the parsed stream (internal error)";
    return MK_ERR_STATE;
  }
  if (total > seq_len) {
    c->err = std::string(s.what) + ": more windows in the rows of a piece than symbols in its stream (internal error)";
    return MK_ERR_STATE;
  }
  if (total >> 32) {
    c->err = std::string(s.what) + ": the median takes pieces of fewer than 2^32 windows";
    return MK_ERR_ARG;
  }

  // the track into scratch, the medians
  if ((rc = mk_buf_reserve(c, f.counts, std::max<size_t>((size_t)total * sizeof(uint32_t), 16))) != MK_OK) return rc;
  uint32_t* d_counts = (uint32_t*)f.counts.p;
  if (total) {
    if ((rc = f.track.begin()) != MK_OK) return rc;
    if ((rc = tk_launch_probe<uint32_t>(s, woff, sstart, nrows, total, d_counts, d_tk)) != MK_OK) return rc;
    if ((rc = f.track.end()) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(&ht, d_tk, sizeof ht, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if ((rc = f.track.add_to(f.st.s_track)) != MK_OK) return rc;
    if (ht.written != total) {
      c->err = std::string(s.what) + ": the track kernel wrote " + std::to_string(ht.written) + " of " + std::to_string(total) +
               " windows (internal error)";
      return MK_ERR_STATE;
    }
  }
  if ((rc = f.sort.begin()) != MK_OK) return rc;
  if ((rc = tk_median<uint32_t>(c, f.med, d_counts, woff, nrows, total, std::min<u64>(ht.max_count, 0xFFFFFFFFull), ht.longest, d_med)) != MK_OK) return rc;
  if ((rc = f.sort.end()) != MK_OK) return rc;

  // (the lengths are only added up before the guards below have passed: no address is made of them)
  hipLaunchKernelGGL(nm_decide_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, (const u64*)start,
                     (const uint32_t*)d_med, nrows, (u64)first, (u64)f.rule.target, (u64)f.rule.min_depth, (u64)f.rule.seed, f.invert,
                     d_keep, len, d_st);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  u64 piece_out = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.sort.add_to(f.st.s_median)) != MK_OK) return rc;
  if (h.disagree) {
    c->err = std::string(s.what) + ": the median of " + std::to_string(h.disagree) + " record(s) contradicts their rows (internal error)";
    return MK_ERR_STATE;
  }
  if (start0 > n || piece_out > n - start0) {
    c->err = std::string(s.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.preamble += start0;
  f.st.records_out += h.fl.records_out;
  f.st.records_short += h.records_short;
  f.st.records_low += h.records_low;
  f.st.records_over += h.records_over;
  f.st.records_thinned += h.records_thinned;

  // median, keep and rows of the piece, where the caller has room for them
  if (first + nrows <= f.cap) {
    const auto t1 = MkClock::now();
    const hipMemcpyKind kind = f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + first, d_rows, nrows * sizeof(mk_screen_row_t), kind, c->stream));
    if (f.keep) MK_HIP(hipMemcpyAsync(f.keep + first, d_keep, nrows, kind, c->stream));
    if (f.median) MK_HIP(hipMemcpyAsync(f.median + first, d_med, nrows * sizeof(uint32_t), kind, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }
  return fl_emit(s, f.emit, start, dst, n, nrows, piece_out, f.st.s_gather, f.st.s_write);
}

// How both calls check their own arguments, open as the screen calls open, and end; body(s): the pieces.
template <class Body>
static int nm_run(mk_ctx* c, const char* what, unsigned flags, const mk_norm_rule_t* rule, NmCall* f, size_t* out_len, size_t* nrows,
                  mk_norm_t* st, Body&& body) {
  if (!rule) { c->err = std::string(what) + ": rule is NULL"; return MK_ERR_ARG; }
  if (flags & ~(MK_NORM_FOLD | MK_NORM_INVERT)) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  if (rule->target < 1 || rule->target > 0xFFFFFFFFull) { c->err = std::string(what) + ": target must lie in 1..2^32 - 1"; return MK_ERR_ARG; }
  if (rule->min_depth > 0xFFFFFFFFull) { c->err = std::string(what) + ": min_depth must be below 2^32"; return MK_ERR_ARG; }
  const size_t cap = (f->rows || f->keep || f->median) ? f->cap : ~(size_t)0;
  f->cap = cap;
  int rc = sc_run(c, what, flags & MK_NORM_FOLD, std::max<uint64_t>(rule->min_depth, 1), cap, nrows, &f->st.screen,
                  [&](ScCall& s) { return body(s); });
  if (rc != MK_OK && rc != MK_ERR_RANGE) return rc;
  if (out_len) *out_len = f->emit.bytes_out;
  if (rc != MK_OK) return rc;
  if (f->emit.bytes_out > f->emit.out_cap) {
    c->err = std::string(what) + ": the output holds " + std::to_string(f->emit.bytes_out) + " bytes, out has room for " +
             std::to_string(f->emit.out_cap);
    return MK_ERR_RANGE;
  }
  f->st.bytes_out = f->emit.bytes_out;
  if (st) *st = f->st;
  return MK_OK;
}

extern "C" int mk_norm_device(mk_ctx* c, const uint8_t* d_text, size_t n, unsigned flags, const mk_norm_rule_t* rule, uint8_t* d_out,
                              size_t out_cap, size_t* out_len, uint32_t* d_median, uint8_t* d_keep, mk_screen_row_t* d_rows, size_t cap,
                              size_t* nrows, mk_norm_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (out_cap && !d_out)) { c->err = "mk_norm_device: NULL buffer"; return MK_ERR_ARG; }
  if (((uintptr_t)d_median & 3) || ((uintptr_t)d_rows & 7)) {
    c->err = "mk_norm_device: median must be aligned to 4 and rows to 8";
    return MK_ERR_ARG;
  }
  NmCall f(c, rule ? *rule : mk_norm_rule_t{}, (flags & MK_NORM_INVERT) != 0, d_out, out_cap, d_median, d_keep, d_rows, cap, true);
  return nm_run(c, "mk_norm_device", flags, rule, &f, out_len, nrows, st, [&](ScCall& s) -> int {
    if (!n) return MK_OK;
    const int rc = sc_piece(s, d_text, n, nullptr, ~(size_t)0, &f.d_rows, nullptr);
    return rc != MK_OK ? rc : nm_piece(s, f, n, 0);
  });
}

extern "C" int mk_norm_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_norm_rule_t* rule,
                            uint8_t* out, size_t out_cap, size_t* out_len, uint32_t* median, uint8_t* keep, mk_screen_row_t* rows,
                            size_t cap, size_t* nrows, mk_norm_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (out_cap && !out)) { c->err = "mk_norm_text: NULL buffer"; return MK_ERR_ARG; }
  NmCall f(c, rule ? *rule : mk_norm_rule_t{}, (flags & MK_NORM_INVERT) != 0, out, out_cap, median, keep, rows, cap, false);
  return nm_run(c, "mk_norm_text", flags, rule, &f, out_len, nrows, st, [&](ScCall& s) -> int {
    return sc_text_pieces(s, text, n, piece_bytes, [&](const uint8_t* d_piece, size_t len) -> int {
      const size_t first = s.rows_seen;
      const int rc = sc_piece(s, d_piece, len, nullptr, ~(size_t)0, &f.d_rows, nullptr);
      return rc != MK_OK ? rc : nm_piece(s, f, len, first);
    });
  });
}
