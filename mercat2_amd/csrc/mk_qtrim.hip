// mk_qtrim.hip -- quality trimming and read filtering of a FASTQ text (mk_fastq_qtrim_text / mk_fastq_qtrim_device,
// include/mercat_hip.h has the rule): the qualities that every other read call only carries along are read here, the
// reads cut at both ends by the running sums of BWA -q / cutadapt -q, judged by length, N, low-quality share and mean
// quality, and the survivors gathered as FASTQ -- on the GPU, by mk_fqselect.hip's scheme:
//   fs_index_open / fs_index_lines<false>        the line index (mk_fqindex.h), unchanged.
//   qt_scan_k                16 lanes a record, four records a wave.  A lane owns one aligned 16-byte granule of the
//                            quality line a pass (fs_load), a pass is the 256 bytes of its row of lanes.  The lane sums
//                            its cut - q, a DPP row scan gives every lane the sum in front of it, the lane walks its 16
//                            bytes for its first negative sum and its first maximum, and ballot / a DPP row maximum pick
//                            the first stopped lane and the best in front of it.  Sum, best, its place and the stopped
//                            flag are carried from pass to pass (64-bit; inside a pass 32-bit differences from them
//                            suffice), so a 150-base read is one pass on registers and a 70 000-base read a loop of its
//                            row.  The 3' sweep is the mirror image from the last pass down.  Then the span's low / qsum /
//                            bad-byte walk, the sequence line's N count on its own aligned granules, the verdict, the
//                            mate's verdict from the neighbouring row (mates share a wave), and both histograms: runs of
//                            equal values are counted in registers and added to the workgroup's LDS histogram, which is
//                            flushed once with vector atomics.  No loop trusts a byte of the text: all bounds come
//                            from line[].
//   qt_decide_k              a lane per record: the checks of fs_decide_k, keep[r] from the verdicts of both mates, the
//                            counters, and four segments a record: whole = {record, -, -, -}, cut = {header line,
//                            seq[start:stop] '\n', plus line, qual[start:stop] '\n'}; unused ones have length 0.
//   rocprim::exclusive_scan  over 4 nrec + 1 lengths; the status is read back once before any address is made of them.
//   fs_gather_k / fs_edges_k the gather of mk_fqindex.h, which steps over segments of length 0.
// QtLine, qt_record, fq_segments and the host's piece loop are mk_fqpiece.h's, shared with mk_adapt.hip.
#include "mk_fqpiece.h"

#define FS_QUAL 5  // a quality byte below the phred base (behind FS_KEPT)

struct QtStatus {  // device memory, behind the FsStatus of the piece
  u64 dropped_short, dropped_n, dropped_lowq, dropped_meanq, orphans, bases_in;
};
struct QtOpt {
  int base, cut_front, cut_back;
  unsigned min_len, max_n, low_q, max_low_ppm, min_mean_q, paired, which;
};
enum { QT_PASSES = 0, QT_SHORT = 1, QT_N = 2, QT_LOWQ = 3, QT_MEANQ = 4, QT_FAILED = 5 };

// DPP over a row of 16 lanes: the inclusive prefix sum, and the sum / maximum of the row in every lane of it (row_ror:
// every lane has a source, whole rows are active or idle together).
__device__ __forceinline__ int qt_row_scan_incl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  return v;
}
__device__ __forceinline__ int qt_row_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);  // row_ror:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false);
  return v;
}
__device__ __forceinline__ unsigned qt_row_max(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false));
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false));
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false));
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false));
  return v;
}

// What a sweep carries from pass to pass (the same in all 16 lanes of the row).
struct QtSweep {
  long long s, best;
  u64 at;  // 5': start; 3': stop
  bool stopped;
};

// One pass of a sweep over the row's 256 bytes: cutv - q of every content byte added in index order (BACK: from the
// highest down), the first sum below 0 stops, the first sum above the best so far in front of that is the new best.
// Differences from the carried sum stay inside +-256 * 222, the carried thresholds are clamped far outside that.
template <bool BACK>
__device__ __forceinline__ void qt_sweep(const FsSeg& c, long long i0, long long pass0, u64 L, int cutv, int base, unsigned j, unsigned row,
                                         QtSweep& w) {
  int total = 0;
#pragma unroll
  for (unsigned b = 0; b < 16; ++b) {
    const bool valid = (u64)(i0 + b) < L;
    total += valid ? cutv - ((int)QT_BYTE(c, b) - base) : 0;
  }
  const int incl = qt_row_scan_incl(total), all = qt_row_sum(total);
  int sr = BACK ? all - incl : incl - total;
  const long long lim = 1ll << 30;
  const int negt = (int)(w.s > lim ? -lim : -w.s);                         // sr < negt: the sum is below 0
  const int over = (int)(w.best - w.s > lim ? lim : w.best - w.s);         // sr > over: the sum is above the best
  int mx = INT_MIN, stopb = -1;
  unsigned mxb = 0;
#pragma unroll
  for (unsigned bb = 0; bb < 16; ++bb) {
    const unsigned b = BACK ? 15 - bb : bb;
    const bool valid = (u64)(i0 + b) < L;
    sr += valid ? cutv - ((int)QT_BYTE(c, b) - base) : 0;
    const bool live = valid && stopb < 0;
    if (live && sr < negt) stopb = (int)b;
    else if (live && sr > mx) { mx = sr; mxb = b; }
  }
  const unsigned stops = (unsigned)(__ballot(stopb >= 0) >> (16 * row)) & 0xFFFFu;
  const unsigned stoplane = !stops ? 0u : BACK ? 31u - (unsigned)__clz(stops) : (unsigned)__ffs(stops) - 1u;
  const bool counts = !stops || (BACK ? j >= stoplane : j <= stoplane);
  const unsigned pos = 16 * j + mxb;
  const unsigned key = counts && mx != INT_MIN ? ((unsigned)(mx + 65536) << 8) | (BACK ? pos : 255u - pos) : 0u;
  const unsigned top = qt_row_max(key);
  if (top) {
    const int v = (int)(top >> 8) - 65536;
    const unsigned p = BACK ? top & 255u : 255u - (top & 255u);
    if (v > over) {
      w.best = w.s + v;
      w.at = (u64)(pass0 + p) + (BACK ? 0 : 1);
    }
  }
  w.s += all;
  w.stopped = stops != 0;
}

// Adds the content bytes of the lane's granule with index in [lo, hi) to hist[value]: a run of equal values is one add.
__device__ __forceinline__ void qt_hist(const FsSeg& c, long long i0, u64 lo, u64 hi, int base, unsigned* hist) {
  int cur = 0;
  unsigned cnt = 0;
#pragma unroll
  for (unsigned b = 0; b < 16; ++b) {
    const u64 i = (u64)(i0 + b);
    const int v = (int)QT_BYTE(c, b) - base;
    if (i >= lo && i < hi && v >= 0) {
      if (v != cur && cnt) {
        atomicAdd(&hist[cur], cnt);
        cnt = 0;
      }
      cur = v;
      ++cnt;
    }
  }
  if (cnt) atomicAdd(&hist[cur], cnt);
}

__device__ __forceinline__ unsigned qt_verdict(const QtOpt& o, u64 kept, u64 nn, u64 low, u64 qsum) {
  if (kept < (o.min_len > 1u ? o.min_len : 1u)) return QT_SHORT;
  if (nn > o.max_n) return QT_N;
  if (low * 1000000ull > (u64)o.max_low_ppm * kept) return QT_LOWQ;
  if (qsum < (u64)o.min_mean_q * kept) return QT_MEANQ;
  return QT_PASSES;
}

// rows[6 r ..]: length, start, kept, n, low, qsum; verdict[r]: QT_PASSES, the filter that drops it, or QT_FAILED for a
// record that fails a check (qt_decide_k names the first three, the quality byte is named here).  hist: 512 counters;
// the workgroup's own are 32-bit and flushed once, which the hosts' limit on a piece (below 2^32 bytes) makes safe.
// The grid has a multiple of four rows, and pieces start at even records: mates sit in neighbouring rows of one wave.
static __global__ void __launch_bounds__(256) qt_scan_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ line, size_t nrec,
                                                        QtOpt o, u64* __restrict__ rows, uint8_t* __restrict__ verdict,
                                                        u64* __restrict__ hist, FsStatus* __restrict__ st) {
  __shared__ unsigned s_hist[512];
  s_hist[threadIdx.x] = 0;
  s_hist[threadIdx.x + 256] = 0;
  __syncthreads();
  const unsigned j = threadIdx.x & 15u, row = (threadIdx.x >> 4) & 3u;
  const size_t per_grid = (size_t)gridDim.x * (256 / QT_GROUP);
  // (the loop's condition is the wave's: its four rows go round together and meet at the mate exchange)
  for (size_t r4 = (size_t)blockIdx.x * (256 / QT_GROUP) + ((threadIdx.x >> 6) << 2); r4 < nrec; r4 += per_grid) {
    const size_t r = r4 + row;
    unsigned v = QT_FAILED;
    u64 L = 0, start = 0, stop = 0, nn = 0, low = 0, qsum = 0;
    QtLine ql{0, 0};
    FsSeg q0{};
    if (r < nrec) {
      const QtRecord rec = qt_record(text, line, r);
      if (rec.fail < 0) {
        L = rec.ls;
        ql = QtLine{rec.l3, L};
        const unsigned np = ql.passes();
        q0 = ql.load(text, n, 0, j);
        QtSweep f{0, 0, 0, false}, b{0, 0, L, false};
        if (o.cut_front)
          for (unsigned p = 0; p < np && !f.stopped; ++p)
            qt_sweep<false>(p ? ql.load(text, n, p, j) : q0, ql.i0(p, j), ql.i0(p, 0), L, o.cut_front, o.base, j, row, f);
        if (o.cut_back)
          for (unsigned p = np; p-- > 0 && !b.stopped;)
            qt_sweep<true>(p ? ql.load(text, n, p, j) : q0, ql.i0(p, j), ql.i0(p, 0), L, o.cut_back, o.base, j, row, b);
        start = f.at;
        stop = b.at;
        if (start >= stop) start = stop = 0;
        // the span's low and qsum, every byte against the phred base, and the histogram of all bases
        unsigned bad = 0;
        for (unsigned p = 0; p < np; ++p) {
          const FsSeg c = p ? ql.load(text, n, p, j) : q0;
          const long long i0 = ql.i0(p, j);
          unsigned acc = 0;  // low << 20 | qsum of the lane: at most 16 and 16 * 222
#pragma unroll
          for (unsigned bb = 0; bb < 16; ++bb) {
            const u64 i = (u64)(i0 + bb);
            const int qv = (int)QT_BYTE(c, bb) - o.base;
            bad |= (i < L && qv < 0) ? 1u : 0u;
            if (i >= start && i < stop) acc += (unsigned)qv + (qv < (int)o.low_q ? 1u << 20 : 0u);
          }
          qt_hist(c, i0, 0, L, o.base, s_hist);
          const unsigned sum = (unsigned)qt_row_sum((int)acc);
          low += sum >> 20;
          qsum += sum & 0xFFFFFu;
        }
        bad = qt_row_max(bad);
        // the span's N on the sequence line's own granules
        const QtLine sl{rec.l1, L};
        if (stop > start)
          for (unsigned p = (unsigned)(((rec.l1 & 15) + start) / QT_PASS); p <= (unsigned)(((rec.l1 & 15) + stop - 1) / QT_PASS); ++p) {
            const FsSeg c = sl.load(text, n, p, j);
            const long long i0 = sl.i0(p, j);
            unsigned cnt = 0;
#pragma unroll
            for (unsigned bb = 0; bb < 16; ++bb) {
              const u64 i = (u64)(i0 + bb);
              cnt += (i >= start && i < stop && (QT_BYTE(c, bb) | 0x20u) == 'n') ? 1u : 0u;
            }
            nn += (unsigned)qt_row_sum((int)cnt);
          }
        if (bad) {
          if (j == 0) atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | FS_QUAL));
        } else {
          v = qt_verdict(o, stop - start, nn, low, qsum);
        }
      }
      const u64 mine = j == 0 ? L : j == 1 ? start : j == 2 ? stop - start : j == 3 ? nn : j == 4 ? low : qsum;
      if (j < 6) rows[6 * r + j] = mine;
      if (j == 0) verdict[r] = (uint8_t)v;
    }
    // the mate's verdict: the row beside this one (a record behind the last has QT_FAILED)
    const unsigned mate = (unsigned)__shfl_xor((int)v, 16);
    const bool emit = v == QT_PASSES && (o.paired ? (mate == QT_PASSES ? 1u : 2u) : 1u) == o.which;
    if (emit)
      for (unsigned p = (unsigned)(((ql.a & 15) + start) / QT_PASS); p <= (unsigned)(((ql.a & 15) + stop - 1) / QT_PASS); ++p)
        qt_hist(p ? ql.load(text, n, p, j) : q0, ql.i0(p, j), start, stop, o.base, s_hist + 256);
  }
  __syncthreads();
  if (s_hist[threadIdx.x]) atomicAdd((unsigned long long*)&hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
  if (s_hist[threadIdx.x + 256]) atomicAdd((unsigned long long*)&hist[threadIdx.x + 256], (unsigned long long)s_hist[threadIdx.x + 256]);
}

// A lane per record (and one for the slot behind the last segment).  Record r is lines 4r .. 4r + 3; its segments are
// 4r .. 4r + 3.
static __global__ void __launch_bounds__(256) qt_decide_k(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t nrec, QtOpt o,
                                                          const u64* __restrict__ rows, const uint8_t* __restrict__ verdict,
                                                          uint8_t* __restrict__ keep, u64* __restrict__ seg_src, u64* __restrict__ len,
                                                          FsStatus* __restrict__ st, QtStatus* __restrict__ qs) {
  u64 n_out = 0, n_trimmed = 0, n_bases = 0, n_in = 0, n_short = 0, n_n = 0, n_lowq = 0, n_meanq = 0, n_orphans = 0;
  mk_for_each(nrec + 1, [&](size_t r) {
    if (r == nrec) {
      seg_src[4 * nrec] = 0;
      len[4 * nrec] = 0;
      return;
    }
    const QtRecord q = qt_record(text, line, r);
    if (q.fail >= 0) atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | (unsigned)q.fail));
    const unsigned v = verdict[r];
    unsigned k = v == QT_PASSES ? 1u : 0u;
    if (k && o.paired) k = ((r ^ 1) < nrec && verdict[r ^ 1] == QT_PASSES) ? 1u : 2u;
    keep[r] = (uint8_t)k;
    const u64 L = rows[6 * r], start = rows[6 * r + 1], kept = rows[6 * r + 2];
    n_in += q.fail < 0 ? L : 0;
    n_short += v == QT_SHORT;
    n_n += v == QT_N;
    n_lowq += v == QT_LOWQ;
    n_meanq += v == QT_MEANQ;
    n_orphans += k == 2u;
    u64 s[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    if (q.fail < 0 && k && k == o.which) {
      n_trimmed += fq_segments(q, L, start, kept, s, m) ? 1 : 0;
      n_out += 1;
      n_bases += kept;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      seg_src[4 * r + i] = s[i];
      len[4 * r + i] = m[i];
    }
  });
  block_add(&st->records_out, n_out);
  block_add(&st->records_trimmed, n_trimmed);
  block_add(&st->bases_out, n_bases);
  block_add(&qs->bases_in, n_in);
  block_add(&qs->dropped_short, n_short);
  block_add(&qs->dropped_n, n_n);
  block_add(&qs->dropped_lowq, n_lowq);
  block_add(&qs->dropped_meanq, n_meanq);
  block_add(&qs->orphans, n_orphans);
}


// ------------------------------------------------------------------------------------------ host side
static const char* qt_kind(unsigned kind) { return kind == FS_QUAL ? "its quality line holds a character below the phred base" : fs_kind(kind); }

// What mk_fqpiece.h's piece loop asks of a call.  Side: the histogram in device memory, the caller's (device call) or
// the call's own buffer.
struct QtPolicy {
  typedef QtOpt Opt;
  typedef QtStatus Status;
  typedef mk_fastq_qtrim_t Stats;
  struct Side { u64* d_hist; };
  static constexpr size_t ROW = 6;
  static bool paired(const QtOpt& o) { return o.paired != 0; }
  static const char* kind(unsigned k) { return qt_kind(k); }
  static void scan(FqCall<QtPolicy>& f, const uint8_t* d_text, size_t n, const u64* line, size_t nrec, u64* d_rows, uint8_t* d_verdict,
                   FsStatus* d_st) {
    hipLaunchKernelGGL(qt_scan_k, dim3(grid_for(nrec, 256 / QT_GROUP, 1u << 16)), dim3(256), 0, f.c->stream, d_text, (u64)n, line, nrec, f.o,
                       d_rows, d_verdict, f.side.d_hist, d_st);
  }
  static void decide(FqCall<QtPolicy>& f, const uint8_t* d_text, const u64* line, size_t nrec, const u64* d_rows, const uint8_t* d_verdict,
                     uint8_t* d_keep, u64* seg_src, u64* len, FsStatus* d_st, QtStatus* d_qs) {
    hipLaunchKernelGGL(qt_decide_k, dim3(grid_for(nrec + 1, 256, 4096)), dim3(256), 0, f.c->stream, d_text, line, nrec, f.o, d_rows,
                       d_verdict, d_keep, seg_src, len, d_st, d_qs);
  }
  static void add(mk_fastq_qtrim_t& st, const QtStatus& q) {
    st.bases_in += q.bases_in;
    st.dropped_short += q.dropped_short;
    st.dropped_n += q.dropped_n;
    st.dropped_lowq += q.dropped_lowq;
    st.dropped_meanq += q.dropped_meanq;
    st.orphans += q.orphans;
  }
};
typedef FqCall<QtPolicy> QtCall;

// The options as the kernels take them, or the message of the first one out of range.
static const char* qt_options(const mk_qtrim_opt_t* opt, QtOpt& o) {
  if (!opt) return "opt is NULL";
  if (opt->phred_base != 33 && opt->phred_base != 64) return "phred_base must be 33 or 64";
  if (opt->cut_front > 93 || opt->cut_back > 93) return "cut_front and cut_back must be 0 .. 93";
  if (opt->max_low_ppm > 1000000) return "max_low_ppm must be 0 .. 1000000";
  if (opt->which != 1 && !(opt->which == 2 && opt->paired)) return "which must be 1 (the main output) or, with paired, 2 (the orphans)";
  o.base = (int)opt->phred_base;
  o.cut_front = (int)opt->cut_front;
  o.cut_back = (int)opt->cut_back;
  o.min_len = opt->min_len;
  o.max_n = opt->max_n;
  o.low_q = opt->low_q > 256 ? 256 : opt->low_q;
  o.max_low_ppm = opt->max_low_ppm;
  o.min_mean_q = opt->min_mean_q;
  o.paired = opt->paired ? 1 : 0;
  o.which = opt->which;
  return nullptr;
}

// fq_run with the histogram zeroed before the pieces and, for the text call, copied to h_hist (host memory) behind them.
template <class Body>
static int qt_run(QtCall& f, u64* h_hist, size_t* out_len, size_t* nrec, mk_fastq_qtrim_t* st, Body&& body) {
  mk_ctx* c = f.c;
  return fq_run(
      f, out_len, nrec, st,
      [&]() -> int {
        if (!f.side.d_hist) {
          int rc = mk_buf_reserve(c, f.side_buf, 512 * sizeof(u64));
          if (rc != MK_OK) return rc;
          f.side.d_hist = (u64*)f.side_buf.p;
        }
        MK_HIP(hipMemsetAsync(f.side.d_hist, 0, 512 * sizeof(u64), c->stream));
        return MK_OK;
      },
      body,
      [&]() -> int {
        if (!h_hist) return MK_OK;
        const auto t1 = MkClock::now();
        MK_HIP(hipMemcpyAsync(h_hist, f.side.d_hist, 512 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
        f.st.s_write += mk_since(t1);
        return MK_OK;
      });
}

extern "C" int mk_fastq_qtrim_device(mk_ctx* c, const uint8_t* d_fastq, size_t n, const mk_qtrim_opt_t* opt, size_t cap, uint8_t* d_keep,
                                     uint64_t* d_rows, uint64_t* d_hist, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec,
                                     mk_fastq_qtrim_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_fastq) || (out_cap && !d_out)) { c->err = "mk_fastq_qtrim_device: NULL buffer"; return MK_ERR_ARG; }
  // (a workgroup of qt_scan_k counts the bases it sees in 32-bit LDS counters: fewer than 2^32 of them in a piece)
  if (n > 0xFFFFFFFFull) { c->err = "mk_fastq_qtrim_device: the text is one piece, which holds at most 2^32 - 1 bytes"; return MK_ERR_RANGE; }
  if (((uintptr_t)d_rows | (uintptr_t)d_hist) & 7) { c->err = "mk_fastq_qtrim_device: d_rows and d_hist must be aligned to 8"; return MK_ERR_ARG; }
  QtOpt o{};
  if (const char* msg = qt_options(opt, o)) { c->err = std::string("mk_fastq_qtrim_device: ") + msg; return MK_ERR_ARG; }
  QtCall f(c, "mk_fastq_qtrim_device", o, (d_keep || d_rows) ? cap : ~(size_t)0, d_keep, (u64*)d_rows, d_out, out_cap, true);
  f.side.d_hist = (u64*)d_hist;
  return qt_run(f, nullptr, out_len, nrec, st, [&]() -> int { return fq_device_body(f, d_fastq, n); });
}

extern "C" int mk_fastq_qtrim_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_qtrim_opt_t* opt, size_t cap,
                                   uint8_t* keep, uint64_t* rows, uint64_t* hist, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                                   mk_fastq_qtrim_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_fastq_qtrim_text: NULL buffer"; return MK_ERR_ARG; }
  QtOpt o{};
  if (const char* msg = qt_options(opt, o)) { c->err = std::string("mk_fastq_qtrim_text: ") + msg; return MK_ERR_ARG; }
  QtCall f(c, "mk_fastq_qtrim_text", o, (keep || rows) ? cap : ~(size_t)0, keep, (u64*)rows, out, out_cap, false);
  return qt_run(f, (u64*)hist, out_len, nrec, st, [&]() -> int { return fq_text_body(f, fastq, n, piece_bytes); });
}
