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
//   tr_emit: tr_gather_k (tr_edges_k)      fl_gather_k's form -- a lane owns 16 aligned output bytes, a wave instruction
//                                          writes 1 KiB, one search of dst[] per wave -- with two sources a record: the
//                                          header line from the raw text, the kept symbols from the stream, then one LF
// The kernels and tr_emit live in mk_trimwalk.h, shared with mk_pairs.hip.
#include "mk_trimwalk.h"

// ------------------------------------------------------------------------------------------ host side
struct TrCall {
  mk_trim_rule_t rule;
  FlEmit emit;        // where the output goes
  uint64_t* kept;     // the caller's, or nullptr; cap of each
  mk_screen_row_t* rows;
  size_t cap;
  bool device;        // out / kept / rows are device memory
  MkDevBuf d_rows, meta, scan_tmp;
  MkTimed place, first;
  mk_trim_t st{};
  TrCall(mk_ctx* c, const mk_trim_rule_t& r, uint8_t* o, size_t oc, uint64_t* kp, mk_screen_row_t* rw, size_t cp, bool dev)
      : rule(r), emit(c, o, oc, dev), kept(kp), rows(rw), cap(cp), device(dev), place(c), first(c) {}
  ~TrCall() {
    for (MkDevBuf* b : {&d_rows, &meta, &scan_tmp}) buf_free(*b);
  }
};

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

  // kept and rows of the piece, where the caller has room for them
  if (first + nrows <= f.cap) {
    const auto t1 = MkClock::now();
    const hipMemcpyKind kind = f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + first, d_rows, nrows * sizeof(mk_screen_row_t), kind, c->stream));
    if (f.kept) MK_HIP(hipMemcpyAsync(f.kept + first, d_kept, nrows * sizeof(u64), kind, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }
  const TrPlace p{text, (u64)n, (const uint8_t*)c->seq.p, (u64)seq_len, start, sstart, hlen, d_kept, dst, nrows};
  return tr_emit(s, f.emit, p, piece_out, f.st.s_gather, f.st.s_write);
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
