// mk_track.hip -- sequences in, the count under every k-mer window out (mk_track_text / mk_track_device,
// include/mercat_hip.h): what mk_screen_* folds into five numbers a record, written out position by position, and --
// where asked for -- the median of every record's counts.
//
// A piece goes through sc_piece (mk_screenpiece.h: parse, record scan, probe) and leaves its rows on the device.  Then
//   tk_lens_k + rocprim::exclusive_scan     woff[r] = windows of the piece's records in front of r, woff[nrows] = all of
//                                           them; the largest count of the piece beside it (the sort's end_bit)
//   tk_starts_k                             sstart[r] = where record r starts in the stream: a lane of the walk knows how
//                                           far it is from the last separator IT saw, not from the record's
//   tk_probe_k                              the hot path: the walk of mk_screenwalk.h over the same stream and the same
//                                           tile prefixes, its sink positional -- window j of record r goes to
//                                           woff[r] + j, j = (the lane's place - sstart[r]) + its own count.  Inside a
//                                           tile those places are one contiguous range (only separators and the first
//                                           k - 1 symbols of a record give no window), so the tile's counts are gathered
//                                           in LDS, addressed by their place modulo the tile, and the range leaves in
//                                           whole-wave stores.  (Every lane storing its own elements was 19 to 49 %
//                                           slower: DESIGN 8p, profiles/track_probe.md.)
//   tk_median                               (median only) the short records' counts sorted a segment a record and picked,
//                                           the long records' medians selected in place
//   tk_offsets_k                            offsets of the piece, the windows of the pieces before it added
// Placement, the track kernel and the median are mk_trackwalk.h, shared with mk_norm.hip.
#include "mk_trackwalk.h"

__global__ void __launch_bounds__(256) tk_offsets_k(const u64* __restrict__ woff, size_t n, u64 add, u64* __restrict__ out) {
  mk_for_each(n, [&](size_t r) { out[r] = woff[r] + add; });
}

// ------------------------------------------------------------------------------------------ host side
struct TkCall {
  bool sat32, device;
  void* counts;        // the caller's (text call: host memory, device call: device memory), counts_cap elements of room
  size_t counts_cap;
  uint64_t* offsets;   // each the caller's or nullptr; cap rows (cap + 1 offsets)
  void* median;
  mk_screen_row_t* rows;
  size_t cap;
  MkDevBuf d_rows, meta, scan_tmp, stage, small;
  TkMedian med;
  MkTimed place, track, sort;
  mk_track_t st{};
  size_t windows_seen = 0;  // of all pieces so far, written or not
  TkCall(mk_ctx* c, bool s32, bool dev, void* cn, size_t cc, uint64_t* of, void* md, mk_screen_row_t* rw, size_t cp)
      : sat32(s32), device(dev), counts(cn), counts_cap(cc), offsets(of), median(md), rows(rw), cap(cp), place(c), track(c), sort(c) {}
  ~TkCall() {
    for (MkDevBuf* b : {&d_rows, &meta, &scan_tmp, &stage, &small}) buf_free(*b);
  }
};

// What follows sc_piece for a piece whose rows start at row `first` of the call: placement, the track kernel, the
// median, and the copies to the caller's buffers where they have room.  The stream is idle afterwards.
template <class E>
static int tk_piece(ScCall& s, TkCall& f, size_t first) {
  mk_ctx* c = s.c;
  int rc;
  const size_t nrows = s.last.nrows;
  if (!nrows) return MK_OK;
  const mk_screen_row_t* d_rows = s.last.d_rows;
  // meta: TkStatus (32) | wlen[nrows + 1] | woff[nrows + 1] | sstart[nrows]
  if ((rc = mk_buf_reserve(c, f.meta, 32 + (3 * nrows + 2) * sizeof(u64))) != MK_OK) return rc;
  TkStatus* d_st = (TkStatus*)f.meta.p;
  u64* wlen = (u64*)((char*)f.meta.p + 32);
  u64* woff = wlen + nrows + 1;
  u64* sstart = woff + nrows + 1;
  size_t tmp = 0;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)wlen, woff, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  MK_HIP(hipMemsetAsync(d_st, 0, sizeof(TkStatus), c->stream));
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(tk_lens_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, nrows, wlen, d_st);
  if (s.last.seq_len)
    hipLaunchKernelGGL(tk_starts_k, dim3((unsigned)div_up(s.last.seq_len, SC_SPAN)), dim3(256), 0, c->stream, (const uint8_t*)c->seq.p,
                       (u64)s.last.seq_len, s.last.tile_pre, s.last.row_base, nrows, sstart);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)wlen, woff, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if (f.median) {
    hipLaunchKernelGGL(tk_longest_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, (const u64*)woff, nrows, d_st);
    MK_HIP(hipGetLastError());
  }
  if ((rc = f.place.end()) != MK_OK) return rc;
  TkStatus h{};
  u64 total = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&total, woff + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (total > s.last.seq_len) {
    c->err = std::string(s.what) + ": more windows in the rows of a piece than symbols in its stream (internal error)";
    return MK_ERR_STATE;
  }
  const size_t at = f.windows_seen;
  f.windows_seen += (size_t)total;
  const bool rows_fit = first + nrows <= f.cap;

  // rows and offsets of the piece, where the caller has room for them
  const hipMemcpyKind kind = f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (rows_fit && (f.rows || f.offsets)) {
    u64* d_off = f.device ? (u64*)f.offsets + first : nullptr;
    if (f.offsets && !f.device) {
      if ((rc = mk_buf_reserve(c, f.small, (nrows + 1) * sizeof(u64))) != MK_OK) return rc;
      d_off = (u64*)f.small.p;
    }
    if (f.offsets) {
      hipLaunchKernelGGL(tk_offsets_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, (const u64*)woff, nrows + 1, (u64)at, d_off);
      MK_HIP(hipGetLastError());
    }
    const auto t1 = MkClock::now();
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + first, d_rows, nrows * sizeof(mk_screen_row_t), kind, c->stream));
    if (f.offsets && !f.device) MK_HIP(hipMemcpyAsync(f.offsets + first, d_off, (nrows + 1) * sizeof(u64), kind, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }
  if (f.windows_seen > f.counts_cap) return MK_OK;  // (no room: the call goes on adding up and answers MK_ERR_RANGE)
  if (f.median && total >> 32) {
    c->err = std::string(s.what) + ": the median takes pieces of fewer than 2^32 windows";
    return MK_ERR_ARG;
  }

  // the track kernel: into the caller's device memory, or into a staging buffer that is copied to the host
  E* d_out = (E*)f.counts + at;
  if (!f.device) {
    if ((rc = mk_buf_reserve(c, f.stage, std::max<size_t>((size_t)total * sizeof(E), 16))) != MK_OK) return rc;
    d_out = (E*)f.stage.p;
  }
  if (total) {
    if ((rc = f.track.begin()) != MK_OK) return rc;
    if ((rc = tk_launch_probe<E>(s, woff, sstart, nrows, total, d_out, d_st)) != MK_OK) return rc;
    if ((rc = f.track.end()) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if ((rc = f.track.add_to(f.st.s_track)) != MK_OK) return rc;
    if (h.written != total) {
      c->err = std::string(s.what) + ": the track kernel wrote " + std::to_string(h.written) + " of " + std::to_string(total) +
               " windows (internal error)";
      return MK_ERR_STATE;
    }
    f.st.saturated += h.saturated;
  }
  E* d_med = nullptr;
  if (f.median && rows_fit) {
    d_med = (E*)f.median + first;
    if (!f.device) {
      if ((rc = mk_buf_reserve(c, f.small, std::max((nrows + 1) * sizeof(u64), nrows * sizeof(E)))) != MK_OK) return rc;
      d_med = (E*)f.small.p;
    }
    if ((rc = f.sort.begin()) != MK_OK) return rc;
    const u64 mx = sizeof(E) == 4 && h.max_count > 0xFFFFFFFFull ? 0xFFFFFFFFull : h.max_count;
    if ((rc = tk_median<E>(c, f.med, d_out, woff, nrows, total, mx, h.longest, d_med)) != MK_OK) return rc;
    if ((rc = f.sort.end()) != MK_OK) return rc;
    MK_HIP(hipStreamSynchronize(c->stream));
    if ((rc = f.sort.add_to(f.st.s_median)) != MK_OK) return rc;
  }
  if (!f.device) {
    const auto t1 = MkClock::now();
    if (total) MK_HIP(hipMemcpyAsync((E*)f.counts + at, d_out, (size_t)total * sizeof(E), hipMemcpyDeviceToHost, c->stream));
    if (d_med) MK_HIP(hipMemcpyAsync((E*)f.median + first, d_med, nrows * sizeof(E), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }
  return MK_OK;
}

// How both calls check their own arguments, open as the screen calls open, and end; body(s): the pieces.
template <class Body>
static int tk_run(mk_ctx* c, const char* what, unsigned flags, uint64_t at_least, TkCall* f, size_t* nwindows, size_t* nrows,
                  mk_track_t* st, Body&& body) {
  if (flags & ~(MK_TRACK_FOLD | MK_TRACK_SAT32)) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  const size_t cap = (f->rows || f->offsets || f->median) ? f->cap : ~(size_t)0;
  f->cap = cap;
  int rc = sc_run(c, what, flags & MK_TRACK_FOLD, at_least, cap, nrows, &f->st.screen, [&](ScCall& s) -> int {
    if (f->offsets) {  // (offsets[0] of a text without records)
      if (f->device) MK_HIP(hipMemsetAsync(f->offsets, 0, sizeof(u64), c->stream));
      else f->offsets[0] = 0;
    }
    return body(s);
  });
  if (rc != MK_OK && rc != MK_ERR_RANGE) return rc;
  if (nwindows) *nwindows = f->windows_seen;
  if (rc != MK_OK) return rc;
  if (f->windows_seen > f->counts_cap) {
    c->err = std::string(what) + ": the text holds " + std::to_string(f->windows_seen) + " windows, counts has room for " +
             std::to_string(f->counts_cap);
    return MK_ERR_RANGE;
  }
  f->st.windows_out = f->windows_seen;
  if (st) *st = f->st;
  return MK_OK;
}

extern "C" int mk_track_device(mk_ctx* c, const uint8_t* d_text, size_t n, unsigned flags, uint64_t at_least, void* d_counts,
                               size_t counts_cap, size_t* nwindows, uint64_t* d_offsets, void* d_median, mk_screen_row_t* d_rows,
                               size_t cap, size_t* nrows, mk_track_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (counts_cap && !d_counts)) { c->err = "mk_track_device: NULL buffer"; return MK_ERR_ARG; }
  const bool sat32 = (flags & MK_TRACK_SAT32) != 0;
  if (((uintptr_t)d_counts | (uintptr_t)d_median) & (sat32 ? 3 : 7) || ((uintptr_t)d_offsets | (uintptr_t)d_rows) & 7) {
    c->err = "mk_track_device: a buffer is not aligned to its elements";
    return MK_ERR_ARG;
  }
  TkCall f(c, sat32, true, d_counts, counts_cap, d_offsets, d_median, d_rows, cap);
  return tk_run(c, "mk_track_device", flags, at_least, &f, nwindows, nrows, st, [&](ScCall& s) -> int {
    if (!n) return MK_OK;
    const int rc = sc_piece(s, d_text, n, nullptr, ~(size_t)0, &f.d_rows, nullptr);
    if (rc != MK_OK) return rc;
    return sat32 ? tk_piece<uint32_t>(s, f, 0) : tk_piece<u64>(s, f, 0);
  });
}

extern "C" int mk_track_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, uint64_t at_least,
                             void* counts, size_t counts_cap, size_t* nwindows, uint64_t* offsets, void* median,
                             mk_screen_row_t* rows, size_t cap, size_t* nrows, mk_track_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (counts_cap && !counts)) { c->err = "mk_track_text: NULL buffer"; return MK_ERR_ARG; }
  const bool sat32 = (flags & MK_TRACK_SAT32) != 0;
  TkCall f(c, sat32, false, counts, counts_cap, offsets, median, rows, cap);
  return tk_run(c, "mk_track_text", flags, at_least, &f, nwindows, nrows, st, [&](ScCall& s) -> int {
    return sc_text_pieces(s, text, n, piece_bytes, [&](const uint8_t* d_piece, size_t len) -> int {
      const size_t first = s.rows_seen;
      const int rc = sc_piece(s, d_piece, len, nullptr, ~(size_t)0, &f.d_rows, nullptr);
      if (rc != MK_OK) return rc;
      return sat32 ? tk_piece<uint32_t>(s, f, first) : tk_piece<u64>(s, f, first);
    });
  });
}
