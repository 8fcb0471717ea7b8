// mk_pairs.hip -- interleaved paired reads in, the pairs that pass out (mk_pairs_text / mk_pairs_device,
// include/mercat_hip.h): mk_filter_*, mk_trim_* and mk_norm_* with the pair as the unit.  Records 2p and 2p + 1 of the
// call are the mates of pair p; every mate gets the unpaired call's own result, one more kernel joins them.
//
// A piece goes through sc_piece (mk_screenpiece.h) and leaves its rows on the device; `all` rows, of which the first
// `nrows` (an even number) are decided here: a piece of a host text that holds an odd number of records hands its last
// one on to the next piece (pr_text_pieces).  Then, by op,
//   placement      fl_tiles_k / fl_scan_k / fl_starts_k (start[]: every op); tr_hend_k, tk_starts_k (TRIM); tk_lens_k +
//                  scan, tk_starts_k, tk_longest_k (NORM) -- over all rows: they describe the piece
//   the op's walk  TRIM: tr_first_k, then tr_decide_k (kept[r] and the mate's own output length);  NORM: tk_probe_k into
//                  scratch, then tk_median (med[r]);  FILTER: none, the row is the result
//   pr_decide_k    a lane a PAIR: the two own results, the pair rule, keep[] and the two length arrays (out, singles);
//                  the pair counters, NORM's per-record counters and its contradiction count
//   exclusive scan + the op's emitter (fl_emit or tr_emit), once for out and, where a singles buffer was given and the
//                  piece has orphans, once more for singles
// Nothing that moves text or walks the stream is new: mk_recordplace.h, mk_trimwalk.h, mk_trackwalk.h.
//
// pr_decide_k reads two 40-byte rows a lane.  They are adjacent, so a wave's loads cover 5 KiB without a gap and every
// cache line fetched is used whole; the kernel reads 40 MB a million records, once, against a walk that probes 120 M
// windows.  The rows are not staged through LDS: there is no reuse between lanes to pay for the barrier.
#include "mk_trimwalk.h"
#include "mk_trackwalk.h"
#include <memory>

struct PrStatus {  // device memory, read back a piece
  FlStatus fl;     // (headers: what the start kernels found)
  u64 pairs_out, singles_out, bytes_singles;
  u64 records_short, records_low, records_over, records_thinned;
  u64 disagree;    // NORM: records whose median contradicts their row
};

struct PrRule {
  int op;
  bool both, invert;
  u64 min_hits, min_ppm;          // FILTER
  u64 target, min_depth, seed;    // NORM
};

// A lane per pair (and one for the slot behind the last record, whose lengths are 0 so that the scans end in the
// totals).  nrows is even.  ownlen, kept: TRIM's (tr_decide_k); med: NORM's; first: the index over the whole call of
// the piece's row 0 (even).
static __global__ void __launch_bounds__(256) pr_decide_k(PrRule q, const mk_screen_row_t* __restrict__ rows, const u64* __restrict__ start,
                                                          const u64* __restrict__ ownlen, const u64* __restrict__ kept,
                                                          const uint32_t* __restrict__ med, size_t nrows, u64 first,
                                                          uint8_t* __restrict__ keep, u64* __restrict__ len_out, u64* __restrict__ len_sg,
                                                          PrStatus* __restrict__ st) {
  u64 pairs_out = 0, singles = 0, sg_bytes = 0, n_short = 0, n_low = 0, n_over = 0, n_thin = 0, bad = 0;
  mk_for_each(nrows / 2 + 1, [&](size_t p) {
    const size_t r0 = 2 * p;
    if (r0 >= nrows) { len_out[nrows] = 0; len_sg[nrows] = 0; return; }
    bool own[2], pass;
    u64 l[2];
    if (q.op == MK_PAIRS_TRIM) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        own[i] = kept[r0 + i] > 0;
        l[i] = ownlen[r0 + i];
      }
      pass = own[0] && own[1];
    } else if (q.op == MK_PAIRS_FILTER) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const u64 windows = rows[r0 + i].windows, hits = rows[r0 + i].hits;
        own[i] = windows > 0 && hits >= q.min_hits && (unsigned __int128)hits * 1000000u >= (unsigned __int128)q.min_ppm * windows;
        l[i] = start[r0 + i + 1] - start[r0 + i];
      }
      pass = q.both ? (own[0] && own[1]) : (own[0] || own[1]);
    } else {
      u64 depth = ~0ull;  // D: the smallest median of the eligible mates
      unsigned over = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const mk_screen_row_t& row = rows[r0 + i];
        const u64 windows = row.windows, m = med[r0 + i];
        const u64 clip = 0xFFFFFFFFull;  // (the row's counts are not clipped, the median's are)
        const u64 low_end = row.min < clip ? row.min : clip, top = row.max < clip ? row.max : clip;
        bad += (windows ? (m < low_end || m > top) : m != 0) ? 1 : 0;
        const bool is_short = windows == 0, low = !is_short && m < q.min_depth;
        if (!is_short && !low) {
          depth = m < depth ? m : depth;
          over += m > q.target ? 1 : 0;
        }
        n_short += is_short ? 1 : 0;
        n_low += low ? 1 : 0;
        l[i] = start[r0 + i + 1] - start[r0 + i];
      }
      pass = depth != ~0ull && (depth <= q.target || nm_u(q.seed, first + r0) * depth < (q.target << 32));
      own[0] = own[1] = pass;
      n_over += over;
      n_thin += pass ? 0 : over;
    }
    const bool emit = pass != q.invert;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool single = own[i] && !pass && !q.invert;
      keep[r0 + i] = emit ? 1 : single ? 2 : 0;
      len_out[r0 + i] = emit ? l[i] : 0;
      len_sg[r0 + i] = single ? l[i] : 0;
      singles += single ? 1 : 0;
      sg_bytes += single ? l[i] : 0;
    }
    pairs_out += emit ? 1 : 0;
  });
  block_add(&st->pairs_out, pairs_out);
  block_add(&st->singles_out, singles);
  block_add(&st->bytes_singles, sg_bytes);
  if (q.op == MK_PAIRS_NORM) {
    block_add(&st->records_short, n_short);
    block_add(&st->records_low, n_low);
    block_add(&st->records_over, n_over);
    block_add(&st->records_thinned, n_thin);
    block_add(&st->disagree, bad);
  }
}

// ------------------------------------------------------------------------------------------ host side
struct PrCall {
  mk_pairs_rule_t rule;
  unsigned flags;
  FlEmit out, singles;  // where the two outputs go (singles: no room at all when the caller gave no buffer)
  bool want_singles;
  uint8_t* keep;        // the caller's, or nullptr; cap of each
  uint64_t* kept;
  uint32_t* median;
  mk_screen_row_t* rows;
  size_t cap;
  bool device;          // out / singles / keep / kept / median / rows are device memory
  MkDevBuf d_rows, d_rows_back, d_keep, d_med, counts, meta, scan_tmp;
  TkMedian med;
  MkTimed place, walk, sort;
  std::unique_ptr<ScCall> one;  // the screen of a record handed on, alone (pr_text_pieces): its buffers serve every piece
  mk_pairs_t st{};
  bool odd = false;     // the call's last piece ended in a first mate
  size_t records = 0;
  PrCall(mk_ctx* c, const mk_pairs_rule_t& r, unsigned fl, uint8_t* o, size_t oc, uint8_t* sg, size_t sc, uint8_t* kp, uint64_t* kt,
         uint32_t* md, mk_screen_row_t* rw, size_t cp, bool dev)
      : rule(r), flags(fl), out(c, o, oc, dev), singles(c, sg, sg ? sc : 0, dev), want_singles(sg != nullptr), keep(kp), kept(kt),
        median(md), rows(rw), cap(cp), device(dev), place(c), walk(c), sort(c) {}
  ~PrCall() {
    for (MkDevBuf* b : {&d_rows, &d_rows_back, &d_keep, &d_med, &counts, &meta, &scan_tmp}) buf_free(*b);
  }
};

// What follows sc_piece for a piece of n bytes whose rows start at row `first` (even) of the call and whose windows are
// all hits iff all_hits.  last: no piece follows.  *back = the bytes at the piece's end that were NOT decided and go to
// the next piece: its last record where the piece holds an odd number of them, the whole piece where it holds a single
// one (nothing has been added to the call then, the screen figures aside).  The stream is idle afterwards.
static int pr_piece(ScCall& s, PrCall& f, size_t n, size_t first, bool all_hits, bool last, size_t* back) {
  mk_ctx* c = s.c;
  int rc;
  *back = 0;
  const size_t all = s.last.nrows;
  if (!all) {  // (no header line, no kept character)
    f.st.preamble += n;
    return MK_OK;
  }
  if ((all & 1) && last) { f.odd = true; return MK_OK; }
  if (all == 1) { *back = n; return MK_OK; }
  const size_t nrows = all & ~(size_t)1;
  const int op = f.rule.op;
  const uint8_t* text = s.last.text;
  const mk_screen_row_t* d_rows = s.last.d_rows;
  const size_t ntiles = div_up(n, FL_SPAN), seq_len = s.last.seq_len;
  const int headless = s.last.headless ? 1 : 0;
  // meta: PrStatus (128) | TrStatus (64) | TkStatus (32) | start | len_out | len_sg | dst [all + 1] each |
  //       tile_pre[ntiles] | the op's own arrays | tile_cnt[ntiles]
  static_assert(sizeof(PrStatus) <= 128 && sizeof(TrStatus) <= 64 && sizeof(TkStatus) <= 32, "PrStatus");
  const size_t own_words = op == MK_PAIRS_TRIM ? 4 * all + (all + 1) : op == MK_PAIRS_NORM ? 2 * (all + 1) + all : 0;
  if ((rc = mk_buf_reserve(c, f.meta, 224 + (4 * (all + 1) + ntiles + own_words) * sizeof(u64) + ntiles * sizeof(unsigned))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, f.d_keep, nrows)) != MK_OK) return rc;
  PrStatus* d_st = (PrStatus*)f.meta.p;
  TrStatus* d_tr = (TrStatus*)((char*)f.meta.p + 128);
  TkStatus* d_tk = (TkStatus*)((char*)f.meta.p + 192);
  u64* start = (u64*)((char*)f.meta.p + 224);
  u64* len_out = start + all + 1;
  u64* len_sg = len_out + all + 1;
  u64* dst = len_sg + all + 1;
  u64* tile_pre = dst + all + 1;
  u64* own = tile_pre + ntiles;
  u64 *sstart = nullptr, *hlen = nullptr, *first_low = nullptr, *d_kept = nullptr, *ownlen = nullptr, *wlen = nullptr, *woff = nullptr;
  if (op == MK_PAIRS_TRIM) {
    sstart = own; hlen = sstart + all; first_low = hlen + all; d_kept = first_low + all; ownlen = d_kept + all;
  } else if (op == MK_PAIRS_NORM) {
    wlen = own; woff = wlen + all + 1; sstart = woff + all + 1;
  }
  unsigned* tile_cnt = (unsigned*)(own + own_words);
  uint8_t* d_keep = (uint8_t*)f.d_keep.p;
  uint32_t* d_med = nullptr;
  if (op == MK_PAIRS_NORM) {
    if ((rc = mk_buf_reserve(c, f.d_med, nrows * sizeof(uint32_t))) != MK_OK) return rc;
    d_med = (uint32_t*)f.d_med.p;
  }
  size_t tmp = 0;  // (every scan is of at most all + 1 uint64_t)
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len_out, dst, 0ull, all + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  // ---- placement: over all rows of the piece
  MK_HIP(hipMemsetAsync(f.meta.p, 0, 224, c->stream));
  MK_HIP(hipMemsetAsync(start, 0xFF, (all + 1) * sizeof(u64), c->stream));  // (a start no header line gives reads as outside the text)
  if (sstart) MK_HIP(hipMemsetAsync(sstart, 0xFF, all * sizeof(u64), c->stream));
  if (first_low) MK_HIP(hipMemsetAsync(first_low, 0xFF, all * sizeof(u64), c->stream));
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fl_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fl_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, (u64)n, all, headless,
                     start, &d_st->fl);
  hipLaunchKernelGGL(fl_starts_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, (const u64*)tile_pre, (u64)headless,
                     all, start);
  if (op == MK_PAIRS_TRIM)
    hipLaunchKernelGGL(tr_hend_k, dim3(grid_for(all, 256, 4096)), dim3(256), 0, c->stream, text, (u64)n, (const u64*)start, all, headless,
                       hlen);
  if (op == MK_PAIRS_NORM)
    hipLaunchKernelGGL(tk_lens_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, nrows, wlen, d_tk);
  if (sstart && seq_len)
    hipLaunchKernelGGL(tk_starts_k, dim3((unsigned)div_up(seq_len, SC_SPAN)), dim3(256), 0, c->stream, (const uint8_t*)c->seq.p,
                       (u64)seq_len, s.last.tile_pre, s.last.row_base, all, sstart);
  MK_HIP(hipGetLastError());
  if (op == MK_PAIRS_NORM) {
    MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)wlen, woff, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
    hipLaunchKernelGGL(tk_longest_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, (const u64*)woff, nrows, d_tk);
    MK_HIP(hipGetLastError());
  }
  if ((rc = f.place.end()) != MK_OK) return rc;
  const bool walk_first = op == MK_PAIRS_TRIM && !all_hits && seq_len;
  if (walk_first) {
    if ((rc = f.walk.begin()) != MK_OK) return rc;
    if ((rc = tr_launch_first(s, sstart, d_rows, all, first_low, d_tr)) != MK_OK) return rc;
    if ((rc = f.walk.end()) != MK_OK) return rc;
  }
  PrStatus h{};
  TrStatus htr{};
  TkStatus ht{};
  u64 total = 0, start0 = 0, decided_end = 0;  // decided_end: start[nrows], the end of the piece or the start of the record handed on
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&start0, start, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&decided_end, start + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (op == MK_PAIRS_NORM) {
    MK_HIP(hipMemcpyAsync(&ht, d_tk, sizeof ht, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipMemcpyAsync(&total, woff + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  }
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (walk_first && (rc = f.walk.add_to(f.st.s_walk)) != MK_OK) return rc;
  if (h.fl.headers + headless != all) {
    c->err = std::string(s.what) + ": " + std::to_string(h.fl.headers) + " header lines in the text, " +
             std::to_string(all - headless) + " in the parsed stream (internal error)";
    return MK_ERR_STATE;
  }
  if (start0 > decided_end || decided_end > n || (nrows == all) != (decided_end == n)) {
    c->err = std::string(s.what) + ": the record starts of a piece do not ascend to its end (internal error)";
    return MK_ERR_STATE;
  }

  // ---- the op's own per-record step
  if (op == MK_PAIRS_NORM) {
    if (total > seq_len) {
      c->err = std::string(s.what) + ": more windows in the rows of a piece than symbols in its stream (internal error)";
      return MK_ERR_STATE;
    }
    if (total >> 32) {
      c->err = std::string(s.what) + ": the median takes pieces of fewer than 2^32 windows";
      return MK_ERR_ARG;
    }
    if ((rc = mk_buf_reserve(c, f.counts, std::max<size_t>((size_t)total * sizeof(uint32_t), 16))) != MK_OK) return rc;
    uint32_t* d_counts = (uint32_t*)f.counts.p;
    if (total) {
      if ((rc = f.walk.begin()) != MK_OK) return rc;
      if ((rc = tk_launch_probe<uint32_t>(s, woff, sstart, nrows, total, d_counts, d_tk)) != MK_OK) return rc;
      if ((rc = f.walk.end()) != MK_OK) return rc;
      MK_HIP(hipMemcpyAsync(&ht, d_tk, sizeof ht, hipMemcpyDeviceToHost, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      if ((rc = f.walk.add_to(f.st.s_walk)) != MK_OK) return rc;
      if (ht.written != total) {
        c->err = std::string(s.what) + ": the track kernel wrote " + std::to_string(ht.written) + " of " + std::to_string(total) +
                 " windows (internal error)";
        return MK_ERR_STATE;
      }
    }
    if ((rc = f.sort.begin()) != MK_OK) return rc;
    if ((rc = tk_median<uint32_t>(c, f.med, d_counts, woff, nrows, total, std::min<u64>(ht.max_count, 0xFFFFFFFFull), ht.longest, d_med)) != MK_OK) return rc;
    if ((rc = f.sort.end()) != MK_OK) return rc;
  }
  if (op == MK_PAIRS_TRIM)
    hipLaunchKernelGGL(tr_decide_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, (const u64*)first_low,
                       (const u64*)hlen, nrows, (u64)c->k, (u64)f.rule.trim.min_len, d_kept, ownlen, d_tr);

  // ---- the pair (the lengths are only added up before the guards below have passed: no address is made of them)
  const PrRule q{op, (f.flags & MK_PAIRS_BOTH) != 0, (f.flags & MK_PAIRS_INVERT) != 0, (u64)f.rule.filter.min_hits,
                 (u64)f.rule.filter.min_ppm, (u64)f.rule.norm.target, (u64)f.rule.norm.min_depth, (u64)f.rule.norm.seed};
  hipLaunchKernelGGL(pr_decide_k, dim3(grid_for(nrows / 2 + 1, 256, 4096)), dim3(256), 0, c->stream, q, d_rows, (const u64*)start,
                     (const u64*)ownlen, (const u64*)d_kept, (const uint32_t*)d_med, nrows, (u64)first, d_keep, len_out, len_sg, d_st);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len_out, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  u64 piece_out = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&htr, d_tr, sizeof htr, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if (op == MK_PAIRS_NORM && (rc = f.sort.add_to(f.st.s_median)) != MK_OK) return rc;
  if (h.disagree) {
    c->err = std::string(s.what) + ": the median of " + std::to_string(h.disagree) + " record(s) contradicts their rows (internal error)";
    return MK_ERR_STATE;
  }
  if (htr.disagree || htr.outside) {
    c->err = std::string(s.what) + ": the first low window of " + std::to_string(htr.disagree) + " record(s) contradicts their rows, " +
             std::to_string(htr.outside) + " low window(s) outside the placement (internal error)";
    return MK_ERR_STATE;
  }
  // (a trimmed record is no longer than it was, but for the LF a text's last record may gain)
  if (piece_out + h.bytes_singles > decided_end - start0 + (op == MK_PAIRS_TRIM ? 1 : 0)) {
    c->err = std::string(s.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.preamble += start0;
  f.st.pairs += nrows / 2;
  f.st.pairs_out += h.pairs_out;
  f.st.singles_out += h.singles_out;
  if (op == MK_PAIRS_TRIM) {
    f.st.records_trimmed += htr.records_trimmed;
    f.st.records_dropped += nrows - htr.records_out;
    f.st.bases_in += seq_len - (all - headless);  // (the stream: the kept characters and one separator a header line)
    f.st.bases_out += htr.bases_out;
  }
  f.st.records_short += h.records_short;
  f.st.records_low += h.records_low;
  f.st.records_over += h.records_over;
  f.st.records_thinned += h.records_thinned;

  // the arrays of the piece, where the caller has room for them
  if (first + nrows <= f.cap) {
    const auto t1 = MkClock::now();
    const hipMemcpyKind kind = f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + first, d_rows, nrows * sizeof(mk_screen_row_t), kind, c->stream));
    if (f.keep) MK_HIP(hipMemcpyAsync(f.keep + first, d_keep, nrows, kind, c->stream));
    if (f.kept && d_kept) MK_HIP(hipMemcpyAsync(f.kept + first, d_kept, nrows * sizeof(u64), kind, c->stream));
    if (f.median && d_med) MK_HIP(hipMemcpyAsync(f.median + first, d_med, nrows * sizeof(uint32_t), kind, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }

  // ---- the two outputs: the op's emitter under the pair's lengths
  auto emit = [&](FlEmit& e, u64 bytes) -> int {
    if (op != MK_PAIRS_TRIM) return fl_emit(s, e, start, dst, n, nrows, bytes, f.st.s_gather, f.st.s_write);
    const TrPlace p{text, (u64)n, (const uint8_t*)c->seq.p, (u64)seq_len, start, sstart, hlen, d_kept, dst, nrows};
    return tr_emit(s, e, p, bytes, f.st.s_gather, f.st.s_write);
  };
  if ((rc = emit(f.out, piece_out)) != MK_OK) return rc;
  if (f.want_singles && h.bytes_singles) {
    u64 piece_sg = 0;
    MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len_sg, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
    MK_HIP(hipMemcpyAsync(&piece_sg, dst + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (piece_sg != h.bytes_singles) {
      c->err = std::string(s.what) + ": the singles of a piece do not add up (internal error)";
      return MK_ERR_STATE;
    }
    if ((rc = emit(f.singles, piece_sg)) != MK_OK) return rc;
  } else f.singles.bytes_out += (size_t)h.bytes_singles;
  *back = n - (size_t)decided_end;
  return MK_OK;
}

// sc_piece, then pr_piece with what that piece added to the call's windows and hits.
static int pr_both(ScCall& s, PrCall& f, const uint8_t* d_piece, size_t len, bool last, size_t* back) {
  const size_t first = s.rows_seen;
  const u64 w0 = s.out.windows, h0 = s.out.hits;
  const int rc = sc_piece(s, d_piece, len, nullptr, ~(size_t)0, &f.d_rows, nullptr);
  return rc != MK_OK ? rc : pr_piece(s, f, len, first, s.out.windows - w0 == s.out.hits - h0, last, back);
}

// A host text in pieces (sc_piece_ends) none of which ends between mates.  A piece that holds an odd number of records
// hands its last one on: the next piece starts at that record, whose start came back with the placement's read-back.
// What sc_piece counted for it -- it was parsed and probed with its piece -- is taken off the call's screen figures
// again, measured by one more sc_piece over that record alone, so that every record counts once.  A piece that holds a
// single record grows to the next cut and what it counted is dropped whole.
static int pr_text_pieces(ScCall& s, PrCall& f, const uint8_t* text, size_t n, size_t piece_bytes) {
  mk_ctx* c = s.c;
  if (!n) return MK_OK;
  std::vector<uint64_t> ends;
  int r = sc_piece_ends(s, text, n, piece_bytes, ends);
  if (r != MK_OK) return r;
  auto upload = [&](size_t at, size_t len) -> int {
    const int rc = mk_buf_reserve(c, c->raw, len + 64);
    if (rc != MK_OK) return rc;
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(c->raw.p, text + at, len, hipMemcpyHostToDevice, c->stream));
    s.out.s_read += mk_since(t1);
    return MK_OK;
  };
  size_t at = 0;
  for (const uint64_t end : ends) {
    if ((size_t)end <= at) continue;
    const size_t len = (size_t)end - at;
    const mk_screen_t before = s.out;
    const size_t rows_before = s.rows_seen;
    size_t back = 0;
    if ((r = upload(at, len)) != MK_OK) return r;
    if ((r = pr_both(s, f, (const uint8_t*)c->raw.p, len, (size_t)end == n, &back)) != MK_OK) return r;
    if (back == len) {  // a single record: the piece grows
      const mk_screen_t now = s.out;
      s.out = before;
      s.out.s_read = now.s_read; s.out.s_parse = now.s_parse; s.out.s_probe = now.s_probe;
      s.rows_seen = rows_before;
      continue;
    }
    if (back) {
      if (!f.one) f.one.reset(new ScCall{c, s.what, s.fold, s.at_least});
      ScCall& one = *f.one;
      one.out = mk_screen_t{};
      one.rows_seen = 0;
      if ((r = upload((size_t)end - back, back)) != MK_OK) return r;
      if ((r = sc_piece(one, (const uint8_t*)c->raw.p, back, nullptr, ~(size_t)0, &f.d_rows_back, nullptr)) != MK_OK) return r;
      if (one.rows_seen != 1 || one.last.headless || one.out.windows > s.out.windows || one.out.hits > s.out.hits) {
        c->err = std::string(s.what) + ": the record handed to the next piece does not parse as one record (internal error)";
        return MK_ERR_STATE;
      }
      s.rows_seen -= 1;
      s.out.bytes -= back;
      s.out.windows -= one.out.windows;
      s.out.hits -= one.out.hits;
      s.out.packed_windows -= one.out.packed_windows;
      s.out.text_windows -= one.out.text_windows;
      s.out.folded -= one.out.folded;
      s.out.s_read += one.out.s_read;
      s.out.s_parse += one.out.s_parse;
      s.out.s_probe += one.out.s_probe;
      if (f.rule.op == MK_PAIRS_TRIM) f.st.bases_in -= one.last.seq_len - 1;  // (its symbols; the stream holds one separator more)
    }
    at = (size_t)end - back;
  }
  return MK_OK;
}

// How both calls check their arguments -- the op's rule as the unpaired call of that op checks it --, open as the
// screen calls open, and end; body(s): the pieces.
template <class Body>
static int pr_run(mk_ctx* c, const char* what, const mk_pairs_rule_t* rule, PrCall* f, size_t* out_len, size_t* singles_len,
                  size_t* nrows, mk_pairs_t* st, Body&& body) {
  const unsigned flags = f->flags;
  if (!rule) { c->err = std::string(what) + ": rule is NULL"; return MK_ERR_ARG; }
  if (flags & ~(MK_PAIRS_FOLD | MK_PAIRS_INVERT | MK_PAIRS_BOTH)) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  const int op = rule->op;
  if (op != MK_PAIRS_FILTER && op != MK_PAIRS_TRIM && op != MK_PAIRS_NORM) { c->err = std::string(what) + ": unknown op"; return MK_ERR_ARG; }
  if ((flags & MK_PAIRS_INVERT) && op == MK_PAIRS_TRIM) { c->err = std::string(what) + ": MK_PAIRS_INVERT does not go with MK_PAIRS_TRIM"; return MK_ERR_ARG; }
  if ((flags & MK_PAIRS_BOTH) && op != MK_PAIRS_FILTER) { c->err = std::string(what) + ": MK_PAIRS_BOTH goes with MK_PAIRS_FILTER only"; return MK_ERR_ARG; }
  if ((flags & MK_PAIRS_INVERT) && f->want_singles) { c->err = std::string(what) + ": a singles buffer does not go with MK_PAIRS_INVERT"; return MK_ERR_ARG; }
  uint64_t at_least = 0;
  if (op == MK_PAIRS_FILTER) {
    if (rule->filter.min_hits < 1) { c->err = std::string(what) + ": min_hits must be 1 or more"; return MK_ERR_ARG; }
    if (rule->filter.min_ppm > 1000000u) { c->err = std::string(what) + ": min_ppm must lie in 0..1000000"; return MK_ERR_ARG; }
    at_least = rule->filter.at_least;
  } else if (op == MK_PAIRS_TRIM) {
    if (rule->trim.at_least < 1) { c->err = std::string(what) + ": at_least must be 1 or more"; return MK_ERR_ARG; }
    at_least = rule->trim.at_least;
  } else {
    if (rule->norm.target < 1 || rule->norm.target > 0xFFFFFFFFull) { c->err = std::string(what) + ": target must lie in 1..2^32 - 1"; return MK_ERR_ARG; }
    if (rule->norm.min_depth > 0xFFFFFFFFull) { c->err = std::string(what) + ": min_depth must be below 2^32"; return MK_ERR_ARG; }
    at_least = std::max<uint64_t>(rule->norm.min_depth, 1);
  }
  if (op != MK_PAIRS_TRIM) f->kept = nullptr;
  if (op != MK_PAIRS_NORM) f->median = nullptr;
  const size_t cap = (f->rows || f->keep || f->kept || f->median) ? f->cap : ~(size_t)0;
  f->cap = cap;
  int rc = sc_run(c, what, flags & MK_PAIRS_FOLD, at_least, cap, nrows, &f->st.screen, [&](ScCall& s) {
    const int r = body(s);
    f->records = s.rows_seen;
    return r;
  });
  if (rc != MK_OK && rc != MK_ERR_RANGE) return rc;
  if (f->odd) {
    if (out_len) *out_len = 0;
    if (singles_len) *singles_len = 0;
    c->err = std::string(what) + ": the text holds " + std::to_string(f->records) + " records, an odd number: no interleaved pairs";
    return MK_ERR_RANGE;
  }
  if (out_len) *out_len = f->out.bytes_out;
  if (singles_len) *singles_len = f->singles.bytes_out;
  if (rc != MK_OK) return rc;
  if (f->out.bytes_out > f->out.out_cap) {
    c->err = std::string(what) + ": the output holds " + std::to_string(f->out.bytes_out) + " bytes, out has room for " +
             std::to_string(f->out.out_cap);
    return MK_ERR_RANGE;
  }
  if (f->want_singles && f->singles.bytes_out > f->singles.out_cap) {
    c->err = std::string(what) + ": the singles hold " + std::to_string(f->singles.bytes_out) + " bytes, singles has room for " +
             std::to_string(f->singles.out_cap);
    return MK_ERR_RANGE;
  }
  f->st.records_out = 2 * f->st.pairs_out;
  f->st.bytes_out = f->out.bytes_out;
  f->st.bytes_singles = f->singles.bytes_out;
  if (st) *st = f->st;
  return MK_OK;
}

extern "C" int mk_pairs_device(mk_ctx* c, const uint8_t* d_text, size_t n, unsigned flags, const mk_pairs_rule_t* rule, uint8_t* d_out,
                               size_t out_cap, size_t* out_len, uint8_t* d_singles, size_t singles_cap, size_t* singles_len,
                               uint8_t* d_keep, uint64_t* d_kept, uint32_t* d_median, mk_screen_row_t* d_rows, size_t cap, size_t* nrows,
                               mk_pairs_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (out_cap && !d_out)) { c->err = "mk_pairs_device: NULL buffer"; return MK_ERR_ARG; }
  if ((((uintptr_t)d_kept | (uintptr_t)d_rows) & 7) || ((uintptr_t)d_median & 3)) {
    c->err = "mk_pairs_device: kept and rows must be aligned to 8, median to 4";
    return MK_ERR_ARG;
  }
  PrCall f(c, rule ? *rule : mk_pairs_rule_t{}, flags, d_out, out_cap, d_singles, singles_cap, d_keep, d_kept, d_median, d_rows, cap, true);
  return pr_run(c, "mk_pairs_device", rule, &f, out_len, singles_len, nrows, st, [&](ScCall& s) -> int {
    size_t back = 0;
    return n ? pr_both(s, f, d_text, n, true, &back) : MK_OK;
  });
}

extern "C" int mk_pairs_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_pairs_rule_t* rule,
                             uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* singles, size_t singles_cap, size_t* singles_len,
                             uint8_t* keep, uint64_t* kept, uint32_t* median, mk_screen_row_t* rows, size_t cap, size_t* nrows,
                             mk_pairs_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (out_cap && !out)) { c->err = "mk_pairs_text: NULL buffer"; return MK_ERR_ARG; }
  PrCall f(c, rule ? *rule : mk_pairs_rule_t{}, flags, out, out_cap, singles, singles_cap, keep, kept, median, rows, cap, false);
  return pr_run(c, "mk_pairs_text", rule, &f, out_len, singles_len, nrows, st,
                [&](ScCall& s) -> int { return pr_text_pieces(s, f, text, n, piece_bytes); });
}
