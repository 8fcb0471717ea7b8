// mk_qtrim.hip -- quality trimming and read filtering of a FASTQ text (mk_fastq_qtrim_text / mk_fastq_qtrim_device,
// include/mercat_hip.h has the rule): the qualities that every other read call only carries along are read here, the
// reads cut at both ends by the running sums of BWA -q / cutadapt -q, judged by length, N, low-quality share and mean
// quality, and the survivors gathered as FASTQ -- on the GPU, by mk_fqselect.hip's scheme:
//   fs_tiles_k / fs_scan_k / fs_lines_k<false>   the line index (mk_fqindex.h), unchanged.
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
#include "mk_fqindex.h"

#define FS_QUAL 5  // a quality byte below the phred base (behind FS_KEPT)
#define QT_GROUP 16u
#define QT_PASS (QT_GROUP * 16u)

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

// A line's content [a, a + L) seen through aligned granules: pass p, lane j owns the 16 bytes at (a & ~15) + 256 p + 16 j,
// whose byte b is content index i0 + b.  A granule that holds no byte of the content is not loaded.
struct QtLine {
  u64 a, L;
  __device__ __forceinline__ unsigned passes() const { return (unsigned)(((a & 15) + L + QT_PASS - 1) / QT_PASS); }
  __device__ __forceinline__ long long i0(unsigned p, unsigned j) const { return (long long)p * QT_PASS + 16 * j - (long long)(a & 15); }
  __device__ __forceinline__ FsSeg load(const uint8_t* __restrict__ text, u64 n, unsigned p, unsigned j) const {
    const long long i = i0(p, j);
    if (i + 16 <= 0 || i >= (long long)L) {
      FsSeg s;
      s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0;
      s.len = 0;
      s.nlmask = 0;
      return s;
    }
    return fs_load(text, n, (a & ~(u64)15) + (u64)p * QT_PASS + 16 * j);
  }
};
#define QT_BYTE(c, b) (((c).w[(b) >> 2] >> (8 * ((b)&3))) & 0xFFu)

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

// The lines of record r and what the checks on them say: the contents of the sequence line [l1, l1 + ls) and of the
// quality line [l3, l3 + lq), one trailing '\r' taken off each.
struct QtRecord {
  u64 l0, l1, l2, l3, l4, ls, lq;
  bool has_nl;  // the last line ends in '\n'
  int fail;
};
__device__ __forceinline__ QtRecord qt_record(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t r) {
  QtRecord q;
  q.l0 = line[4 * r]; q.l1 = line[4 * r + 1]; q.l2 = line[4 * r + 2]; q.l3 = line[4 * r + 3]; q.l4 = line[4 * r + 4];
  q.ls = q.l2 - 1 - q.l1;
  const bool seq_cr = q.ls > 0 && text[q.l2 - 2] == 13u;
  q.ls -= seq_cr ? 1 : 0;
  q.has_nl = text[q.l4 - 1] == 10u;
  q.lq = q.l4 - (q.has_nl ? 1 : 0) - q.l3;
  const bool qual_cr = q.lq > 0 && text[q.l3 + q.lq - 1] == 13u;
  q.lq -= qual_cr ? 1 : 0;
  q.fail = text[q.l0] != '@' ? FS_AT : text[q.l2] != '+' ? FS_PLUS : q.ls != q.lq ? FS_LENGTH : -1;
  return q;
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
      if (start == 0 && kept == L) {
        s[0] = q.l0 | (q.has_nl ? 0 : FS_FORCE);
        m[0] = q.l4 - q.l0 + (q.has_nl ? 0 : 1);
      } else {
        s[0] = q.l0;
        m[0] = q.l1 - q.l0;
        s[1] = (q.l1 + start) | FS_FORCE;
        m[1] = kept + 1;
        s[2] = q.l2;
        m[2] = q.l3 - q.l2;
        s[3] = (q.l3 + start) | FS_FORCE;
        m[3] = kept + 1;
        n_trimmed += 1;
      }
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
struct QtCall {
  mk_ctx* c;
  const char* what;
  QtOpt o;
  size_t limit;   // records the caller's arrays hold
  uint8_t* keep;  // the caller's arrays (host memory for the text call, device memory for the device call), or nullptr
  u64* rows;
  u64* d_hist;  // device memory: the caller's (device call) or `hist`
  uint8_t* out;
  size_t out_cap;
  bool device;
  MkDevBuf tiles, meta, scan_tmp, stage, hist;
  MkTimed index, scan, place, gather;
  mk_fastq_qtrim_t st{};
  size_t records = 0, bytes_out = 0;  // of all pieces so far
  int bad_rc = MK_OK;                 // the first record that failed a check (pieces come in text order)
  std::string bad_msg;
  QtCall(mk_ctx* c_, const char* w, const QtOpt& o_, size_t lim, uint8_t* kp, u64* rw, uint8_t* ot, size_t oc, bool dev)
      : c(c_), what(w), o(o_), limit(lim), keep(kp), rows(rw), d_hist(nullptr), out(ot), out_cap(oc), device(dev), index(c_), scan(c_),
        place(c_), gather(c_) {}
  ~QtCall() {
    for (MkDevBuf* b : {&tiles, &meta, &scan_tmp, &stage, &hist}) buf_free(*b);
  }
  bool counting_only() const { return bad_rc != MK_OK || records > limit; }
};

static const char* qt_kind(unsigned kind) { return kind == FS_QUAL ? "its quality line holds a character below the phred base" : fs_kind(kind); }

// One piece of n > 0 bytes at d_text (device memory, 16-byte aligned, whole records -- whole pairs with paired -- but for
// what trails in the last piece).  Its records are added to f.records either way.  The stream is idle afterwards.
static int qt_piece(QtCall& f, const uint8_t* d_text, size_t n) {
  mk_ctx* c = f.c;
  int rc;
  const size_t ntiles = div_up(n, FS_TILE);
  // tiles: FsStatus | QtStatus | tile_pre[ntiles] | tile_cnt[ntiles]
  if ((rc = mk_buf_reserve(c, f.tiles, sizeof(FsStatus) + sizeof(QtStatus) + ntiles * (sizeof(u64) + sizeof(unsigned)))) != MK_OK) return rc;
  FsStatus* d_st = (FsStatus*)f.tiles.p;
  QtStatus* d_qs = (QtStatus*)(d_st + 1);
  u64* tile_pre = (u64*)(d_qs + 1);
  unsigned* tile_cnt = (unsigned*)(tile_pre + ntiles);
  struct { FsStatus s; QtStatus q; } h{};
  h.s.bad = FS_NONE;
  MK_HIP(hipMemcpyAsync(d_st, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
  if ((rc = f.index.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fs_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fs_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.index.end()) != MK_OK) return rc;
  uint8_t tail[4] = {0, 0, 0, 0};
  const size_t ntail = std::min<size_t>(n, 4);
  u64 newlines = 0;
  MK_HIP(hipMemcpyAsync(&newlines, &d_st->newlines, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(tail + (4 - ntail), d_text + (n - ntail), ntail, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.index.add_to(f.st.s_index)) != MK_OK) return rc;
  const u64 lines = newlines + (tail[3] != '\n' ? 1 : 0);
  const size_t nrec = (size_t)(lines / 4), first = f.records;
  const unsigned trailing = (unsigned)(lines & 3);
  f.st.lines += lines;
  f.records += nrec;
  // what trails behind the last complete record: `trailing` empty lines are that many '\n' behind a '\n' (or the text's start)
  bool trail_ok = true;
  for (unsigned i = 0; i < trailing && trail_ok; ++i) trail_ok = tail[3 - i] == '\n';
  if (trailing && trail_ok && n > trailing) trail_ok = tail[3 - trailing] == '\n';
  if (f.counting_only()) return MK_OK;
  const auto fail_trailing = [&]() {
    f.bad_rc = MK_ERR_UNSUPPORTED;
    f.bad_msg = std::string(f.what) + ": record " + std::to_string(first + nrec) + " is malformed: the text ends inside it (" +
                std::to_string(trailing) + " of its 4 lines)";
    return MK_OK;
  };
  if (!nrec) return trail_ok ? MK_OK : fail_trailing();

  // meta: line[4 nrec + 1] | seg_src[nseg + 1] | len[nseg + 1] | dst[nseg + 1] | rows[6 nrec] | verdict[nrec] | keep[nrec]
  const size_t nseg = 4 * nrec, nidx = 4 * nrec;
  if ((rc = mk_buf_reserve(c, f.meta, (nidx + 1 + 3 * (nseg + 1) + 6 * nrec) * sizeof(u64) + 2 * nrec)) != MK_OK) return rc;
  u64* line = (u64*)f.meta.p;
  u64* seg_src = line + nidx + 1;
  u64* len = seg_src + nseg + 1;
  u64* dst = len + nseg + 1;
  u64* d_rows = dst + nseg + 1;
  uint8_t* d_verdict = (uint8_t*)(d_rows + 6 * nrec);
  uint8_t* d_keep = d_verdict + nrec;
  if (f.device && f.rows) d_rows = f.rows + 6 * first;
  if (f.device && f.keep) d_keep = f.keep + first;
  size_t tmp = 0;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, nseg + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  if ((rc = f.index.begin()) != MK_OK) return rc;
  const int end_is_n = lines == nidx ? 1 : 0;  // (no line 4 nrec starts: the last record ends with the text)
  hipLaunchKernelGGL(fs_lines_k<false>, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_text, (u64)n, (const u64*)tile_pre, (u64)nidx,
                     end_is_n, line, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.index.end()) != MK_OK) return rc;
  if ((rc = f.scan.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(qt_scan_k, dim3(grid_for(nrec, 256 / QT_GROUP, 1u << 16)), dim3(256), 0, c->stream, d_text, (u64)n, (const u64*)line, nrec,
                     f.o, d_rows, d_verdict, f.d_hist, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.scan.end()) != MK_OK) return rc;
  if ((rc = f.place.begin()) != MK_OK) return rc;
  // (the lengths are only added up before the status below has been read: no address is made of them)
  hipLaunchKernelGGL(qt_decide_k, dim3(grid_for(nrec + 1, 256, 4096)), dim3(256), 0, c->stream, d_text, (const u64*)line, nrec, f.o,
                     (const u64*)d_rows, (const uint8_t*)d_verdict, d_keep, seg_src, len, d_st, d_qs);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nseg + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = f.place.end()) != MK_OK) return rc;
  u64 piece_out = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nseg, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.index.add_to(f.st.s_index)) != MK_OK) return rc;
  if ((rc = f.scan.add_to(f.st.s_scan)) != MK_OK) return rc;
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (h.s.bad != FS_NONE) {
    f.bad_rc = MK_ERR_UNSUPPORTED;
    f.bad_msg = std::string(f.what) + ": record " + std::to_string(first + (size_t)(h.s.bad >> 3)) + " is malformed: " +
                qt_kind((unsigned)(h.s.bad & 7));
    return MK_OK;
  }
  if (!trail_ok) return fail_trailing();
  if (piece_out > (u64)n + 1) {
    c->err = std::string(f.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.records_out += h.s.records_out;
  f.st.records_trimmed += h.s.records_trimmed;
  f.st.bases_out += h.s.bases_out;
  f.st.bases_in += h.q.bases_in;
  f.st.dropped_short += h.q.dropped_short;
  f.st.dropped_n += h.q.dropped_n;
  f.st.dropped_lowq += h.q.dropped_lowq;
  f.st.dropped_meanq += h.q.dropped_meanq;
  f.st.orphans += h.q.orphans;
  if (!f.device && (f.keep || f.rows)) {
    const auto t1 = MkClock::now();
    if (f.keep) MK_HIP(hipMemcpyAsync(f.keep + first, d_keep, nrec, hipMemcpyDeviceToHost, c->stream));
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + 6 * first, d_rows, 6 * nrec * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }

  // the gather: into the caller's device memory, or into a staging buffer that is copied to the host.  Without room the
  // call goes on adding up and answers MK_ERR_RANGE at its end.
  const size_t at = f.bytes_out;
  f.bytes_out += (size_t)piece_out;
  if (!piece_out || f.bytes_out > f.out_cap) return MK_OK;
  uint8_t* d_out = f.out + at;
  if (!f.device) {
    if ((rc = mk_buf_reserve(c, f.stage, (size_t)piece_out)) != MK_OK) return rc;
    d_out = (uint8_t*)f.stage.p;
  }
  const u64 head = std::min<u64>((16 - ((uintptr_t)d_out & 15)) & 15, piece_out);
  const u64 nbody = (piece_out - head) / 16, tail_at = head + 16 * nbody;
  if ((rc = f.gather.begin()) != MK_OK) return rc;
  if (nbody)
    hipLaunchKernelGGL(fs_gather_k, dim3((unsigned)div_up((size_t)nbody, 256 * FS_CHUNKS)), dim3(256), 0, c->stream, d_text, (u64)n,
                       (const u64*)seg_src, (const u64*)dst, nseg, head, nbody, d_out);
  if (head || tail_at < piece_out)
    hipLaunchKernelGGL(fs_edges_k, dim3(1), dim3(64), 0, c->stream, d_text, (u64)n, (const u64*)seg_src, (const u64*)dst, nseg, head,
                       tail_at, piece_out, d_out);
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

// How both calls check their arguments, open and end; body(): the pieces.  h_hist: where the text call wants the
// histogram (host memory).
template <class Body>
static int qt_run(QtCall& f, u64* h_hist, size_t* out_len, size_t* nrec, mk_fastq_qtrim_t* st, Body&& body) {
  mk_ctx* c = f.c;
  MK_REFUSE_SPOILED(c, f.what);
  if (c->in_chunk) { c->err = std::string(f.what) + ": a chunk is open"; return MK_ERR_STATE; }
  if (!out_len) { c->err = std::string(f.what) + ": out_len is NULL"; return MK_ERR_ARG; }
  *out_len = 0;
  if (nrec) *nrec = 0;
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipStreamSynchronize(c->stream));
  int rc;
  if (!f.d_hist) {
    if ((rc = mk_buf_reserve(c, f.hist, 512 * sizeof(u64))) != MK_OK) return rc;
    f.d_hist = (u64*)f.hist.p;
  }
  MK_HIP(hipMemsetAsync(f.d_hist, 0, 512 * sizeof(u64), c->stream));
  rc = body();
  (void)hipStreamSynchronize(c->stream);
  if (rc != MK_OK) return rc;
  if (nrec) *nrec = f.records;
  if (f.records > f.limit) {
    c->err = std::string(f.what) + ": the text holds " + std::to_string(f.records) + " records, keep and rows have room for " +
             std::to_string(f.limit);
    return MK_ERR_RANGE;
  }
  if (f.o.paired && (f.records & 1)) {
    c->err = std::string(f.what) + ": paired, but the text holds an odd number of records (" + std::to_string(f.records) + ")";
    return MK_ERR_RANGE;
  }
  if (f.bad_rc != MK_OK) {
    c->err = f.bad_msg;
    return f.bad_rc;
  }
  if (h_hist) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(h_hist, f.d_hist, 512 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }
  *out_len = f.bytes_out;
  f.st.records = f.records;
  f.st.bytes_out = f.bytes_out;
  if (st) *st = f.st;
  if (f.bytes_out > f.out_cap) {
    c->err = std::string(f.what) + ": the output holds " + std::to_string(f.bytes_out) + " bytes, out has room for " + std::to_string(f.out_cap);
    return MK_ERR_RANGE;
  }
  return MK_OK;
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
  f.d_hist = (u64*)d_hist;
  return qt_run(f, nullptr, out_len, nrec, st, [&]() -> int {
    if (!n) return MK_OK;
    const uint8_t* d_text = d_fastq;
    if ((uintptr_t)d_text & 15) {  // (the line passes, the scan and fl_load16 load 16 aligned bytes at a time)
      int rc = mk_buf_reserve(c, c->raw, n + 64);
      if (rc != MK_OK) return rc;
      const auto t1 = MkClock::now();
      MK_HIP(hipMemcpyAsync(c->raw.p, d_fastq, n, hipMemcpyDeviceToDevice, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      f.st.s_copy += mk_since(t1);
      d_text = (const uint8_t*)c->raw.p;
    }
    return qt_piece(f, d_text, n);
  });
}

extern "C" int mk_fastq_qtrim_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_qtrim_opt_t* opt, size_t cap,
                                   uint8_t* keep, uint64_t* rows, uint64_t* hist, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                                   mk_fastq_qtrim_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_fastq_qtrim_text: NULL buffer"; return MK_ERR_ARG; }
  QtOpt o{};
  if (const char* msg = qt_options(opt, o)) { c->err = std::string("mk_fastq_qtrim_text: ") + msg; return MK_ERR_ARG; }
  QtCall f(c, "mk_fastq_qtrim_text", o, (keep || rows) ? cap : ~(size_t)0, keep, (u64*)rows, out, out_cap, false);
  return qt_run(f, (u64*)hist, out_len, nrec, st, [&]() -> int {
    if (!n) return MK_OK;
    // pieces end behind a line 4j (8j: mates stay together) once they hold `piece` bytes: the default and the limits of
    // the screen calls
    size_t piece = piece_bytes ? piece_bytes : std::min(TL_DEFAULT_PIECE, std::max<size_t>(n + 2, 4096));
    piece = std::min(std::max(piece, 2 * ((size_t)c->k + 24)), TL_MAX_PIECE);
    std::vector<uint64_t> cuts(n / piece + 2, 0);
    size_t ncuts = 0;
    if ((o.paired ? mk_fastq_pair_cuts : mk_fastq_cuts)(fastq, n, piece, cuts.data(), cuts.size(), &ncuts) != MK_OK) {
      c->err = "mk_fastq_qtrim_text: the line scanner failed (internal error)";
      return MK_ERR_STATE;
    }
    cuts.resize(ncuts);
    cuts.push_back(n);
    size_t at = 0;
    for (const uint64_t end : cuts) {
      const size_t len = (size_t)end - at;
      if (!len) continue;
      int rc = mk_buf_reserve(c, c->raw, len + 64);
      if (rc != MK_OK) return rc;
      const auto t1 = MkClock::now();
      MK_HIP(hipMemcpyAsync(c->raw.p, fastq + at, len, hipMemcpyHostToDevice, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      f.st.s_copy += mk_since(t1);
      if ((rc = qt_piece(f, (const uint8_t*)c->raw.p, len)) != MK_OK) return rc;
      at = (size_t)end;
    }
    return MK_OK;
  });
}
