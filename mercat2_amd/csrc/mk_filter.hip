// mk_filter.hip -- sequences in, the matched (or the unmatched) records out (mk_filter_text / mk_filter_device,
// include/mercat_hip.h): what mk_screen_* finds for every record of a FASTA text decides whether the record's bytes are
// copied to the output, on the GPU, where the text and the rows already are.
//
// A piece goes through sc_piece (mk_screenpiece.h: parse, record scan, probe) and leaves its rows on the device.  Then
//   fl_tiles_k / fl_scan_k / fl_starts_k   (mk_recordplace.h, shared with mk_trim.hip) the header lines of the RAW text:
//                                          start[r] for every row, start[nrows] = n.
//                                          Only a '>' byte pays for the look back over blanks to a newline.  The header
//                                          lines found must be the parser's separators: that guard (fl_piece) is the
//                                          only link between the two views of the text.
//   fl_decide_k                            a lane per record: keep[r] from its row and the rule, the kept length
//   rocprim::exclusive_scan                dst[r], dst[nrows] = the piece's output length
//   fl_emit: fl_gather_k (fl_edges_k)      (mk_recordplace.h, shared with mk_norm.hip: the same output under another
//                                          decision) the only kernel that moves text: output-driven, a lane owns 16 aligned output
//                                          bytes at a time, finds their record by search in dst[], reads the (unaligned)
//                                          source and issues one 16-byte store.  No atomics, no byte stores but for the
//                                          at most 15 + 15 bytes in front of and behind the aligned body.
#include "mk_recordplace.h"
#include "mk_tableview.h"
#include <rocprim/device/device_scan.hpp>

// A lane per record (and one for the slot behind the last, whose length is 0 so that the scan ends in the total).
__global__ void __launch_bounds__(256) fl_decide_k(const mk_screen_row_t* __restrict__ rows, const u64* __restrict__ start, size_t nrows,
                                                   u64 min_hits, u64 min_ppm, bool invert, uint8_t* __restrict__ keep,
                                                   u64* __restrict__ len, FlStatus* __restrict__ st) {
  u64 kept = 0;
  mk_for_each(nrows + 1, [&](size_t r) {
    if (r == nrows) { len[r] = 0; return; }
    const u64 windows = rows[r].windows, hits = rows[r].hits;
    const bool matched = windows > 0 && hits >= min_hits &&
                         (unsigned __int128)hits * 1000000u >= (unsigned __int128)min_ppm * windows;
    const bool k = matched != invert;
    keep[r] = k ? 1 : 0;
    len[r] = k ? start[r + 1] - start[r] : 0;
    kept += k ? 1 : 0;
  });
  block_add(&st->records_out, kept);
}

// ------------------------------------------------------------------------------------------ host side
struct FlCall {
  mk_filter_rule_t rule;
  bool invert;
  FlEmit emit;        // where the output goes
  mk_screen_row_t* rows;  // the caller's, or nullptr; cap of each
  uint8_t* keep;
  size_t cap;
  bool device;        // out / rows / keep are device memory
  MkDevBuf d_rows, d_keep, meta, scan_tmp;
  MkTimed place;
  mk_filter_t st{};
  FlCall(mk_ctx* c, const mk_filter_rule_t& r, bool inv, uint8_t* o, size_t oc, mk_screen_row_t* rw, uint8_t* kp, size_t cp, bool dev)
      : rule(r), invert(inv), emit(c, o, oc, dev), rows(rw), keep(kp), cap(cp), device(dev), place(c) {}
  ~FlCall() {
    for (MkDevBuf* b : {&d_rows, &d_keep, &meta, &scan_tmp}) buf_free(*b);
  }
};

// What follows sc_piece for a piece of n bytes whose rows start at row `first` of the call: record starts, decision,
// placement, gather, and the copies to the caller's buffers where they have room.  The stream is idle afterwards.
static int fl_piece(ScCall& s, FlCall& f, size_t n, size_t first) {
  mk_ctx* c = s.c;
  int rc;
  const size_t nrows = s.last.nrows;
  if (!nrows) {  // (no header line, no kept character)
    f.st.preamble += n;
    return MK_OK;
  }
  const uint8_t* text = s.last.text;
  const mk_screen_row_t* d_rows = s.last.d_rows;
  const size_t ntiles = div_up(n, FL_SPAN);
  // meta: FlStatus (16) | start[nrows + 1] | len[nrows + 1] | dst[nrows + 1] | tile_pre[ntiles] | tile_cnt[ntiles]
  if ((rc = mk_buf_reserve(c, f.meta, 16 + (3 * (nrows + 1) + ntiles) * sizeof(u64) + ntiles * sizeof(unsigned))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, f.d_keep, nrows)) != MK_OK) return rc;
  FlStatus* d_st = (FlStatus*)f.meta.p;
  u64* start = (u64*)((char*)f.meta.p + 16);
  u64* len = start + nrows + 1;
  u64* dst = len + nrows + 1;
  u64* tile_pre = dst + nrows + 1;
  unsigned* tile_cnt = (unsigned*)(tile_pre + ntiles);
  uint8_t* d_keep = (uint8_t*)f.d_keep.p;
  size_t tmp = 0;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  MK_HIP(hipMemsetAsync(d_st, 0, sizeof(FlStatus), c->stream));
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fl_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fl_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, (u64)n, nrows,
                     s.last.headless ? 1 : 0, start, d_st);
  hipLaunchKernelGGL(fl_starts_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, (const u64*)tile_pre,
                     (u64)(s.last.headless ? 1 : 0), nrows, start);
  MK_HIP(hipGetLastError());
  // (the lengths are only added up before the guard below has compared the two views: no address is made of them)
  hipLaunchKernelGGL(fl_decide_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, (const u64*)start, nrows,
                     (u64)f.rule.min_hits, (u64)f.rule.min_ppm, f.invert, d_keep, len, d_st);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = f.place.end()) != MK_OK) return rc;
  FlStatus h{};
  u64 piece_out = 0, start0 = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&start0, start, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (h.headers + (s.last.headless ? 1 : 0) != nrows) {
    c->err = std::string(s.what) + ": " + std::to_string(h.headers) + " header lines in the text, " +
             std::to_string(nrows - (s.last.headless ? 1 : 0)) + " in the parsed stream (internal error)";
    return MK_ERR_STATE;
  }
  if (piece_out > n - start0) {
    c->err = std::string(s.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.preamble += start0;
  f.st.records_out += h.records_out;
  // rows and keep of the piece, where the caller has room for them
  if (first + nrows <= f.cap) {
    const auto t1 = MkClock::now();
    const hipMemcpyKind kind = f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + first, d_rows, nrows * sizeof(mk_screen_row_t), kind, c->stream));
    if (f.keep) MK_HIP(hipMemcpyAsync(f.keep + first, d_keep, nrows, kind, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }
  return fl_emit(s, f.emit, start, dst, n, nrows, piece_out, f.st.s_gather, f.st.s_write);
}

// How both calls check their own arguments, open as the screen calls open, and end; body(s, f): the pieces.
template <class Body>
static int fl_run(mk_ctx* c, const char* what, unsigned flags, const mk_filter_rule_t* rule, FlCall* f, size_t* out_len,
                  size_t* nrows, mk_filter_t* st, Body&& body) {
  if (!rule) { c->err = std::string(what) + ": rule is NULL"; return MK_ERR_ARG; }
  if (flags & ~(MK_FILTER_FOLD | MK_FILTER_INVERT)) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  if (rule->min_hits < 1) { c->err = std::string(what) + ": min_hits must be 1 or more"; return MK_ERR_ARG; }
  if (rule->min_ppm > 1000000u) { c->err = std::string(what) + ": min_ppm must lie in 0..1000000"; return MK_ERR_ARG; }
  const size_t cap = (f->rows || f->keep) ? f->cap : ~(size_t)0;
  f->cap = cap;
  int rc = sc_run(c, what, flags & MK_FILTER_FOLD, rule->at_least, cap, nrows, &f->st.screen, [&](ScCall& s) { return body(s); });
  if (rc != MK_OK && rc != MK_ERR_RANGE) return rc;
  if (out_len) *out_len = f->emit.bytes_out;
  if (rc != MK_OK) return rc;
  if (f->emit.bytes_out > f->emit.out_cap) {
    c->err = std::string(what) + ": the output holds " + std::to_string(f->emit.bytes_out) + " bytes, out has room for " + std::to_string(f->emit.out_cap);
    return MK_ERR_RANGE;
  }
  f->st.bytes_out = f->emit.bytes_out;
  if (st) *st = f->st;
  return MK_OK;
}

extern "C" int mk_filter_device(mk_ctx* c, const uint8_t* d_text, size_t n, unsigned flags, const mk_filter_rule_t* rule,
                                uint8_t* d_out, size_t out_cap, size_t* out_len, mk_screen_row_t* d_rows, uint8_t* d_keep, size_t cap,
                                size_t* nrows, mk_filter_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (out_cap && !d_out)) { c->err = "mk_filter_device: NULL buffer"; return MK_ERR_ARG; }
  FlCall f(c, rule ? *rule : mk_filter_rule_t{}, (flags & MK_FILTER_INVERT) != 0, d_out, out_cap, d_rows, d_keep, cap, true);
  return fl_run(c, "mk_filter_device", flags, rule, &f, out_len, nrows, st, [&](ScCall& s) -> int {
    if (!n) return MK_OK;
    const int rc = sc_piece(s, d_text, n, nullptr, ~(size_t)0, &f.d_rows, nullptr);
    return rc != MK_OK ? rc : fl_piece(s, f, n, 0);
  });
}

extern "C" int mk_filter_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_filter_rule_t* rule,
                              uint8_t* out, size_t out_cap, size_t* out_len, mk_screen_row_t* rows, uint8_t* keep, size_t cap,
                              size_t* nrows, mk_filter_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (out_cap && !out)) { c->err = "mk_filter_text: NULL buffer"; return MK_ERR_ARG; }
  FlCall f(c, rule ? *rule : mk_filter_rule_t{}, (flags & MK_FILTER_INVERT) != 0, out, out_cap, rows, keep, cap, false);
  return fl_run(c, "mk_filter_text", flags, rule, &f, out_len, nrows, st, [&](ScCall& s) -> int {
    return sc_text_pieces(s, text, n, piece_bytes, [&](const uint8_t* d_piece, size_t len) -> int {
      const size_t first = s.rows_seen;
      const int rc = sc_piece(s, d_piece, len, nullptr, ~(size_t)0, &f.d_rows, nullptr);
      return rc != MK_OK ? rc : fl_piece(s, f, len, first);
    });
  });
}
