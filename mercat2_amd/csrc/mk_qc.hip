// mk_qc.hip -- per-cycle quality control of a FASTQ text (mk_fastq_qc_text / mk_fastq_qc_device, include/mercat_hip.h
// has the rule): where along the read the quality falls and the base composition drifts, and per read its length, mean
// quality and GC share -- the figures fastqc gives MerCat2 before and after trimming, reduced on the GPU from the text,
// the line index and the record checks the trimming calls already have there.  Nothing is written out, so the decide /
// prefix sum / gather of mk_fqpiece.h's piece have no part here; the piece below is the line index of mk_fqindex.h
// (fs_index_open, fs_index_lines) with two kernels behind it:
//   qc_reads_k    qt_scan_k's layout: 16 lanes a record, four records a wave, a lane one aligned 16-byte granule of a
//                 line a pass, DPP row sums.  The quality line gives qsum and the bytes below the phred base, the
//                 sequence line on its own granules gc and n.  Lane 0 of the row names a failed record (atomicMin on the
//                 status word), adds the read to the workgroup's LDS histograms of length, mean quality and GC share,
//                 which are flushed once with 64-bit vector atomics (lengths from QC_LEN_LDS on go straight to global
//                 memory: long reads are few), and leaves {l1, l3, L} of the record, 32-bit (a piece is below 2^32
//                 bytes), for the kernel behind it.  L = 0 for a record that failed: that kernel steps over it.
//   qc_cycles_k   the hot path.  blockIdx.y is a tile of QC_TILE consecutive cycles, blockIdx.z the mate class,
//                 blockIdx.x strides over the records of the class; a record has a wave and a cycle a lane, so the lanes
//                 of one wave-instruction never meet on a counter, whatever the qualities are.  The workgroup's table
//                 [QC_TILE][96 + 8] of 32-bit counters (again: a piece is below 2^32 bytes) has a row stride of 105
//                 dwords: with 104, lanes 4 apart with equal qualities -- the common case -- would share a bank, 8 lanes
//                 a bank in a group of 32; an odd stride spreads the 32 over the 32 banks.  A record that ends in front
//                 of the tile costs one compare.  The tile behind the last (launched only if a read is longer than P)
//                 walks every cycle from P on into row P.  One flush a workgroup, 64-bit vector atomics, zero counters
//                 skipped.  The host sizes gridDim.y from the longest read of the piece, which qc_reads_k has found:
//                 150-base reads launch three tiles, not P / 64.
// No loop trusts a byte of the text: all bounds come from line[].
#include "mk_fqpiece.h"

#define QC_QUAL 5        // a quality byte below the phred base (behind FS_KEPT; mk_qtrim.hip's FS_QUAL)
#define QC_TILE 64u      // cycles a workgroup of qc_cycles_k owns: a lane each
#define QC_COLS (MK_QC_QBINS + 8u)
#define QC_STRIDE (QC_COLS + 1u)  // odd: see above
#define QC_BLOCK 512u    // threads of qc_cycles_k: eight records in flight on one table
#define QC_UNROLL 4      // records a wave of qc_cycles_k loads before it counts them
#define QC_LEN_LDS 512u  // read lengths below this are counted in LDS
// The grid of qc_cycles_k: at most QC_MAX_BLOCKS workgroups a piece, and at least QC_WAVE_RECORDS records a wave where the
// piece has them.  Every workgroup ends in a flush of up to 64 x 104 atomics, and a 16 MiB piece of 150-base reads is
// short work: measured on 1 M such reads, 4 or 8 records a wave cost 1.3x to 2.8x on those pieces, 64 or 256 records
// a wave or 512 workgroups 1.1x to 3.4x.
#define QC_MAX_BLOCKS 2048u
#define QC_WAVE_RECORDS 16u
#define QC_GC_BINS 101u
static_assert(QC_STRIDE % 2 == 1, "the row stride of qc_cycles_k's table must be odd");
static_assert(MK_QC_MAX_POS / QC_TILE + 1 <= 65535, "gridDim.y");

struct QcStatus {  // device memory, behind the FsStatus of the piece
  u64 bad, bases, min_len[2], max_len[2];
};
struct QcRec {  // what qc_reads_k leaves of a record: where its sequence and quality lines start, and its bases
  unsigned l1, l3, len, pad;
};
struct QcOpt {
  int base;
  unsigned P, paired;
};
struct QcTables {  // device memory
  u64 *pos_qual, *pos_base, *read_len, *read_qual, *read_gc;
};

// the sum of a row of 16 lanes in every lane of it (mk_qtrim.hip's qt_row_sum: whole rows are active or idle together)
__device__ __forceinline__ int qc_row_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);  // row_ror:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false);
  return v;
}

// rows[4 r ..]: length, qsum, gc, n (rows may be null).  Pieces start at even records: the class of record r is r & 1.
// The grid's stride is a multiple of four records, the loop's condition the wave's.
static __global__ void __launch_bounds__(256) qc_reads_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ line, size_t nrec,
                                                         QcOpt o, QcTables t, u64* __restrict__ rows, QcRec* __restrict__ rec,
                                                         QcStatus* __restrict__ st) {
  __shared__ unsigned s_len[2][QC_LEN_LDS], s_qual[2][MK_QC_QBINS], s_gc[2][QC_GC_BINS], s_min[2], s_max[2];
  for (unsigned i = threadIdx.x; i < 2 * QC_LEN_LDS; i += 256) (&s_len[0][0])[i] = 0;
  for (unsigned i = threadIdx.x; i < 2 * MK_QC_QBINS; i += 256) (&s_qual[0][0])[i] = 0;
  for (unsigned i = threadIdx.x; i < 2 * QC_GC_BINS; i += 256) (&s_gc[0][0])[i] = 0;
  if (threadIdx.x < 2) {
    s_min[threadIdx.x] = ~0u;
    s_max[threadIdx.x] = 0;
  }
  __syncthreads();
  const unsigned j = threadIdx.x & 15u, row = (threadIdx.x >> 4) & 3u;
  const size_t per_grid = (size_t)gridDim.x * (256 / QT_GROUP);
  const u64 len_bins = (u64)o.P + 2;
  u64 bases = 0;
  for (size_t r4 = (size_t)blockIdx.x * (256 / QT_GROUP) + ((threadIdx.x >> 6) << 2); r4 < nrec; r4 += per_grid) {
    const size_t r = r4 + row;
    if (r >= nrec) continue;
    const QtRecord q = qt_record(text, line, r);
    QcRec mine{(unsigned)q.l1, (unsigned)q.l3, 0u, 0u};
    if (q.fail >= 0) {
      if (j == 0) {
        atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | (unsigned)q.fail));
        rec[r] = mine;
      }
      continue;
    }
    const u64 L = q.ls;
    // the quality line: qsum, and every byte against the phred base
    const QtLine ql{q.l3, L};
    u64 qsum = 0;
    int bad = 0;
    for (unsigned p = 0, np = ql.passes(); p < np; ++p) {
      const FsSeg c = ql.load(text, n, p, j);
      const long long i0 = ql.i0(p, j);
      int acc = 0;  // of the lane: at most 16 * 222
#pragma unroll
      for (unsigned b = 0; b < 16; ++b) {
        const bool valid = (u64)(i0 + b) < L;
        const int qv = (int)QT_BYTE(c, b) - o.base;
        bad |= (valid && qv < 0) ? 1 : 0;
        acc += (valid && qv > 0) ? qv : 0;
      }
      qsum += (u64)(unsigned)qc_row_sum(acc);
    }
    bad = qc_row_sum(bad);
    // the sequence line on its own granules: gc and n
    const QtLine sl{q.l1, L};
    u64 gc = 0, nn = 0;
    for (unsigned p = 0, np = sl.passes(); p < np; ++p) {
      const FsSeg c = sl.load(text, n, p, j);
      const long long i0 = sl.i0(p, j);
      unsigned cnt = 0;  // n << 16 | gc of the lane, of the row behind the sum: at most 256 each
#pragma unroll
      for (unsigned b = 0; b < 16; ++b) {
        const bool valid = (u64)(i0 + b) < L;
        const unsigned ch = QT_BYTE(c, b) | 0x20u;
        cnt += (valid && (ch == 'c' || ch == 'g')) ? 1u : 0u;
        cnt += (valid && ch == 'n') ? 1u << 16 : 0u;
      }
      const unsigned sum = (unsigned)qc_row_sum((int)cnt);
      gc += sum & 0xFFFFu;
      nn += sum >> 16;
    }
    if (bad) {
      if (j == 0) {
        atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | QC_QUAL));
        rec[r] = mine;
      }
      continue;
    }
    if (rows && j < 4) rows[4 * r + j] = j == 0 ? L : j == 1 ? qsum : j == 2 ? gc : nn;
    if (j == 0) {
      const unsigned cls = o.paired ? (unsigned)(r & 1) : 0u;
      const u64 lb = L <= o.P ? L : (u64)o.P + 1;
      if (lb < QC_LEN_LDS) atomicAdd(&s_len[cls][lb], 1u);
      else atomicAdd((unsigned long long*)&t.read_len[cls * len_bins + lb], 1ull);
      if (L) {
        const u64 m = qsum / L, g = (200 * gc + L) / (2 * L);  // (gc <= L: g <= 100)
        atomicAdd(&s_qual[cls][m < MK_QC_QBINS - 1 ? m : MK_QC_QBINS - 1], 1u);
        atomicAdd(&s_gc[cls][g < QC_GC_BINS - 1 ? g : QC_GC_BINS - 1], 1u);
      }
      atomicMin(&s_min[cls], (unsigned)L);
      atomicMax(&s_max[cls], (unsigned)L);
      bases += L;
      mine.len = (unsigned)L;
      rec[r] = mine;
    }
  }
  __syncthreads();
  const unsigned classes = o.paired ? 2u : 1u;
  for (unsigned cls = 0; cls < classes; ++cls) {
    for (unsigned i = threadIdx.x; i < QC_LEN_LDS && i < len_bins; i += 256)
      if (s_len[cls][i]) atomicAdd((unsigned long long*)&t.read_len[cls * len_bins + i], (unsigned long long)s_len[cls][i]);
    if (threadIdx.x < MK_QC_QBINS && s_qual[cls][threadIdx.x])
      atomicAdd((unsigned long long*)&t.read_qual[cls * MK_QC_QBINS + threadIdx.x], (unsigned long long)s_qual[cls][threadIdx.x]);
    if (threadIdx.x < QC_GC_BINS && s_gc[cls][threadIdx.x])
      atomicAdd((unsigned long long*)&t.read_gc[cls * QC_GC_BINS + threadIdx.x], (unsigned long long)s_gc[cls][threadIdx.x]);
    if (threadIdx.x == 0 && s_min[cls] != ~0u) {
      atomicMin((unsigned long long*)&st->min_len[cls], (unsigned long long)s_min[cls]);
      atomicMax((unsigned long long*)&st->max_len[cls], (unsigned long long)s_max[cls]);
    }
  }
  block_add(&st->bases, bases);
}

// One base of row `row` of the workgroup's table: its quality bin and its base class.  A byte below the phred base
// (the host launches nothing over a piece that holds one) wraps to the last bin: inside the row either way.
__device__ __forceinline__ void qc_count(unsigned* __restrict__ s_tab, unsigned row, unsigned qual, unsigned base_byte, int phred) {
  const unsigned q = (unsigned)((int)qual - phred);
  const unsigned v = q < MK_QC_QBINS - 1 ? q : MK_QC_QBINS - 1;
  const unsigned ch = base_byte | 0x20u;
  const unsigned k = ch == 'a' ? 0u : ch == 'c' ? 1u : ch == 'g' ? 2u : ch == 't' ? 3u : ch == 'n' ? 4u : 5u;
  atomicAdd(&s_tab[row * QC_STRIDE + v], 1u);
  atomicAdd(&s_tab[row * QC_STRIDE + MK_QC_QBINS + k], 1u);
}

// tiles: the tiles of rows below P that the piece's longest read reaches; gridDim.y is one more where a read is longer
// than P.  Record cls + classes * k is the k-th of its class.
static __global__ void __launch_bounds__(QC_BLOCK) qc_cycles_k(const uint8_t* __restrict__ text, const QcRec* __restrict__ rec, size_t nrec,
                                                               QcOpt o, unsigned tiles, u64* __restrict__ pos_qual,
                                                               u64* __restrict__ pos_base) {
  __shared__ unsigned s_tab[QC_TILE * QC_STRIDE];
  for (unsigned i = threadIdx.x; i < QC_TILE * QC_STRIDE; i += QC_BLOCK) s_tab[i] = 0;
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u, classes = o.paired ? 2u : 1u, cls = blockIdx.z;
  const bool over = blockIdx.y >= tiles;
  const unsigned row0 = over ? o.P : blockIdx.y * QC_TILE;
  const size_t nk = nrec > cls ? (nrec - cls + classes - 1) / classes : 0;
  const size_t step = (size_t)gridDim.x * (QC_BLOCK / 64);
  const size_t k0 = (size_t)blockIdx.x * (QC_BLOCK / 64) + (threadIdx.x >> 6);
  if (!over) {
    const unsigned i = row0 + lane;  // the lane's cycle
    for (size_t k = k0; k < nk; k += QC_UNROLL * step) {
      unsigned qual[QC_UNROLL], base_byte[QC_UNROLL];
      bool on[QC_UNROLL];
#pragma unroll
      for (int u = 0; u < QC_UNROLL; ++u) {
        const size_t ku = k + (size_t)u * step;
        on[u] = false;
        qual[u] = base_byte[u] = 0;
        if (ku < nk) {
          const QcRec q = rec[cls + classes * ku];
          on[u] = i < q.len && i < o.P;
          if (on[u]) {
            qual[u] = text[(u64)q.l3 + i];
            base_byte[u] = text[(u64)q.l1 + i];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < QC_UNROLL; ++u)
        if (on[u]) qc_count(s_tab, lane, qual[u], base_byte[u], o.base);
    }
  } else {
    for (size_t k = k0; k < nk; k += step) {
      const QcRec q = rec[cls + classes * k];
      for (u64 i = (u64)o.P + lane; i < q.len; i += 64) qc_count(s_tab, 0, text[(u64)q.l3 + i], text[(u64)q.l1 + i], o.base);
    }
  }
  __syncthreads();
  const u64 table_row0 = (u64)cls * ((u64)o.P + 1) + row0;
  for (unsigned idx = threadIdx.x; idx < (over ? QC_COLS : QC_TILE * QC_COLS); idx += QC_BLOCK) {
    const unsigned r = idx / QC_COLS, col = idx % QC_COLS, cnt = s_tab[r * QC_STRIDE + col];
    if (!cnt || row0 + r > o.P) continue;
    if (col < MK_QC_QBINS) atomicAdd((unsigned long long*)&pos_qual[(table_row0 + r) * MK_QC_QBINS + col], (unsigned long long)cnt);
    else atomicAdd((unsigned long long*)&pos_base[(table_row0 + r) * 8 + (col - MK_QC_QBINS)], (unsigned long long)cnt);
  }
}


// ------------------------------------------------------------------------------------------ host side
static const char* qc_kind(unsigned kind) { return kind == QC_QUAL ? "its quality line holds a character below the phred base" : fs_kind(kind); }

static size_t qc_table_words(const QcOpt& o, size_t at[5]) {  // where the five tables start in one buffer of uint64
  const size_t C = o.paired ? 2 : 1, P = o.P;
  const size_t words[5] = {C * (P + 1) * MK_QC_QBINS, C * (P + 1) * 8, C * (P + 2), C * MK_QC_QBINS, C * QC_GC_BINS};
  size_t total = 0;
  for (int i = 0; i < 5; ++i) {
    at[i] = total;
    total += words[i];
  }
  return total;
}

struct QcCall : FsPieces {
  mk_ctx* c;
  QcOpt o;
  u64* rows;     // the caller's (host memory for the text call, device memory for the device call), or nullptr
  bool device;
  QcTables t{};
  MkDevBuf tiles, meta, tables;
  MkTimed index, reads, cycles;
  mk_fastq_qc_t st{};
  u64 mn[2] = {~0ull, ~0ull}, mx[2] = {0, 0};
  QcCall(mk_ctx* c_, const char* w, const QcOpt& o_, size_t lim, u64* rw, bool dev)
      : FsPieces{w, lim}, c(c_), o(o_), rows(rw), device(dev), index(c_), reads(c_), cycles(c_) {}
  ~QcCall() {
    for (MkDevBuf* b : {&tiles, &meta, &tables}) buf_free(*b);
  }
};

// One piece of n > 0 bytes at d_text (device memory, 16-byte aligned, below 2^32 bytes, whole records -- whole pairs with
// paired -- but for what trails in the last piece): fq_piece's line index and checks, then the two kernels.  Its records
// are added to f.records either way.  The stream is idle afterwards.
static int qc_piece(QcCall& f, const uint8_t* d_text, size_t n) {
  mk_ctx* c = f.c;
  int rc;
  static_assert(sizeof(QcStatus) <= FS_OWN_MAX && sizeof(QcStatus) % 8 == 0, "the status block of the call");
  QcStatus hq{};
  hq.bad = FS_NONE;
  hq.min_len[0] = hq.min_len[1] = ~0ull;
  FsIndex ix;
  if ((rc = fs_index_open(c, f.tiles, f.index, f.st.s_index, d_text, n, &hq, sizeof hq, ix)) != MK_OK) return rc;
  QcStatus* d_qs = (QcStatus*)ix.d_own;
  const size_t nrec = ix.nrec;
  size_t first;
  f.st.lines += ix.lines;
  if (!f.take(ix, first)) return MK_OK;

  // meta: line[4 nrec + 1] | rec[nrec] | rows[4 nrec] (the text call's, where the caller wants them)
  const size_t nidx = 4 * nrec;
  const bool own_rows = f.rows && !f.device;
  if ((rc = mk_buf_reserve(c, f.meta, (nidx + 1) * sizeof(u64) + nrec * sizeof(QcRec) + (own_rows ? 4 * nrec * sizeof(u64) : 0))) != MK_OK)
    return rc;
  u64* line = (u64*)f.meta.p;
  QcRec* d_rec = (QcRec*)(line + nidx + 1);
  u64* d_rows = own_rows ? (u64*)(d_rec + nrec) : f.rows ? f.rows + 4 * first : nullptr;

  if ((rc = fs_index_lines<false>(c, f.index, d_text, n, ix, line)) != MK_OK) return rc;
  if ((rc = f.reads.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(qc_reads_k, dim3(grid_for(nrec, 256 / QT_GROUP, 1u << 16)), dim3(256), 0, c->stream, d_text, (u64)n, (const u64*)line,
                     nrec, f.o, f.t, d_rows, d_rec, d_qs);
  MK_HIP(hipGetLastError());
  if ((rc = f.reads.end()) != MK_OK) return rc;
  MK_HIP(hipMemcpyAsync(&hq, d_qs, sizeof hq, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.index.add_to(f.st.s_index)) != MK_OK) return rc;
  if ((rc = f.reads.add_to(f.st.s_reads)) != MK_OK) return rc;
  if (f.failed(ix, first, hq.bad, qc_kind)) return MK_OK;
  f.st.bases += hq.bases;
  for (int k = 0; k < 2; ++k) {
    f.mn[k] = std::min(f.mn[k], hq.min_len[k]);
    f.mx[k] = std::max(f.mx[k], hq.max_len[k]);
  }

  // the cycles: as many tiles as the piece's longest read reaches, and the one behind them if it passes P
  const u64 longest = std::max(hq.max_len[0], hq.max_len[1]);
  if (longest) {
    const unsigned classes = f.o.paired ? 2u : 1u;
    const unsigned tiles = (unsigned)div_up((size_t)std::min<u64>(longest, f.o.P), QC_TILE);
    const unsigned gy = tiles + (longest > f.o.P ? 1u : 0u);
    const unsigned gx = grid_for(div_up(nrec, classes), (QC_BLOCK / 64) * QC_WAVE_RECORDS, std::max(1u, QC_MAX_BLOCKS / (gy * classes)));
    if ((rc = f.cycles.begin()) != MK_OK) return rc;
    hipLaunchKernelGGL(qc_cycles_k, dim3(gx, gy, classes), dim3(QC_BLOCK), 0, c->stream, d_text, (const QcRec*)d_rec, nrec, f.o, tiles,
                       f.t.pos_qual, f.t.pos_base);
    MK_HIP(hipGetLastError());
    if ((rc = f.cycles.end()) != MK_OK) return rc;
    MK_HIP(hipStreamSynchronize(c->stream));
    if ((rc = f.cycles.add_to(f.st.s_cycles)) != MK_OK) return rc;
  }
  if (own_rows) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(f.rows + 4 * first, d_rows, 4 * nrec * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }
  return MK_OK;
}

// How both calls open and end (fq_run's order): pre() readies the tables on the device, body() runs the pieces, post()
// copies back what the text call owes once the call is known to succeed.
template <class Pre, class Body, class Post>
static int qc_run(QcCall& f, size_t* nrec, mk_fastq_qc_t* st, Pre&& pre, Body&& body, Post&& post) {
  mk_ctx* c = f.c;
  int rc = fs_call(
      c, f.what,
      [&]() -> int {
        if (nrec) *nrec = 0;
        return MK_OK;
      },
      [&]() -> int {
        const int r = pre();
        return r != MK_OK ? r : body();
      });
  if (rc != MK_OK) return rc;
  if (nrec) *nrec = f.records;
  if (f.records > f.limit) {
    c->err = std::string(f.what) + ": the text holds " + std::to_string(f.records) + " records, rows has room for " + std::to_string(f.limit);
    return MK_ERR_RANGE;
  }
  if ((rc = fs_call_end(c, f.what, f.records, f.o.paired, f.bad_rc, f.bad_msg)) != MK_OK) return rc;
  if ((rc = post()) != MK_OK) return rc;
  f.st.records = f.records;
  for (int k = 0; k < 2; ++k) {
    f.st.min_len[k] = f.mn[k] == ~0ull ? 0 : f.mn[k];
    f.st.max_len[k] = f.mx[k];
  }
  if (st) *st = f.st;
  return MK_OK;
}

// The options as the kernels take them, or the message of the first one out of range.
static const char* qc_options(const mk_qc_opt_t* opt, const mk_qc_out_t* out, QcOpt& o) {
  if (!opt) return "opt is NULL";
  if (opt->phred_base != 33 && opt->phred_base != 64) return "phred_base must be 33 or 64";
  if (opt->max_pos < 1 || opt->max_pos > MK_QC_MAX_POS) return "max_pos must be 1 .. 16384";
  if (opt->paired > 1) return "paired must be 0 or 1";
  if (!out) return "out is NULL";
  if (!out->pos_qual || !out->pos_base || !out->read_len || !out->read_qual || !out->read_gc) return "a table of out is NULL (only rows may be)";
  o.base = (int)opt->phred_base;
  o.P = opt->max_pos;
  o.paired = opt->paired;
  return nullptr;
}

extern "C" int mk_fastq_qc_device(mk_ctx* c, const uint8_t* d_fastq, size_t n, const mk_qc_opt_t* opt, size_t cap, const mk_qc_out_t* d_out,
                                  size_t* nrec, mk_fastq_qc_t* st) {
  if (!c) return MK_ERR_ARG;
  if (n && !d_fastq) { c->err = "mk_fastq_qc_device: NULL buffer"; return MK_ERR_ARG; }
  // (the workgroups count the bases they see in 32-bit LDS counters, and QcRec holds 32-bit offsets)
  if (n > 0xFFFFFFFFull) { c->err = "mk_fastq_qc_device: the text is one piece, which holds at most 2^32 - 1 bytes"; return MK_ERR_RANGE; }
  QcOpt o{};
  if (const char* msg = qc_options(opt, d_out, o)) { c->err = std::string("mk_fastq_qc_device: ") + msg; return MK_ERR_ARG; }
  if (((uintptr_t)d_out->pos_qual | (uintptr_t)d_out->pos_base | (uintptr_t)d_out->read_len | (uintptr_t)d_out->read_qual |
       (uintptr_t)d_out->read_gc | (uintptr_t)d_out->rows) & 7) {
    c->err = "mk_fastq_qc_device: the tables and rows must be aligned to 8";
    return MK_ERR_ARG;
  }
  QcCall f(c, "mk_fastq_qc_device", o, d_out->rows ? cap : ~(size_t)0, (u64*)d_out->rows, true);
  f.t = QcTables{(u64*)d_out->pos_qual, (u64*)d_out->pos_base, (u64*)d_out->read_len, (u64*)d_out->read_qual, (u64*)d_out->read_gc};
  return qc_run(
      f, nrec, st,
      [&]() -> int {
        size_t at[5];
        const size_t total = qc_table_words(o, at);
        u64* const tabs[5] = {f.t.pos_qual, f.t.pos_base, f.t.read_len, f.t.read_qual, f.t.read_gc};
        for (int i = 0; i < 5; ++i) MK_HIP(hipMemsetAsync(tabs[i], 0, ((i < 4 ? at[i + 1] : total) - at[i]) * sizeof(u64), c->stream));
        return MK_OK;
      },
      [&]() -> int {
        if (!n) return MK_OK;
        const uint8_t* d_text;
        const int rc = fs_aligned_text(c, d_fastq, n, false, f.st.s_copy, &d_text);
        return rc != MK_OK ? rc : qc_piece(f, d_text, n);
      },
      [&]() -> int { return MK_OK; });
}

extern "C" int mk_fastq_qc_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_qc_opt_t* opt, size_t cap,
                                const mk_qc_out_t* out, size_t* nrec, mk_fastq_qc_t* st) {
  if (!c) return MK_ERR_ARG;
  if (n && !fastq) { c->err = "mk_fastq_qc_text: NULL buffer"; return MK_ERR_ARG; }
  QcOpt o{};
  if (const char* msg = qc_options(opt, out, o)) { c->err = std::string("mk_fastq_qc_text: ") + msg; return MK_ERR_ARG; }
  QcCall f(c, "mk_fastq_qc_text", o, out->rows ? cap : ~(size_t)0, (u64*)out->rows, false);
  size_t at[5];
  const size_t total = qc_table_words(o, at);
  u64* const host[5] = {(u64*)out->pos_qual, (u64*)out->pos_base, (u64*)out->read_len, (u64*)out->read_qual, (u64*)out->read_gc};
  return qc_run(
      f, nrec, st,
      [&]() -> int {
        int rc = mk_buf_reserve(c, f.tables, total * sizeof(u64));
        if (rc != MK_OK) return rc;
        u64* p = (u64*)f.tables.p;
        f.t = QcTables{p + at[0], p + at[1], p + at[2], p + at[3], p + at[4]};
        MK_HIP(hipMemsetAsync(p, 0, total * sizeof(u64), c->stream));
        return MK_OK;
      },
      [&]() -> int {
        if (!n) return MK_OK;
        std::vector<uint64_t> cuts;
        int rc = fs_piece_cuts(c, f.what, fastq, n, piece_bytes, o.paired, cuts);
        if (rc != MK_OK) return rc;
        size_t from = 0;
        for (const uint64_t end : cuts) {
          const size_t len = (size_t)end - from;
          if (!len) continue;
          // (a record longer than the piece grows it: the kernels' 32-bit offsets and counters end at 2^32)
          if (len > 0xFFFFFFFFull) { c->err = "mk_fastq_qc_text: a piece holds at most 2^32 - 1 bytes"; return MK_ERR_RANGE; }
          if ((rc = fs_upload_raw(c, fastq + from, len, f.st.s_copy)) != MK_OK) return rc;
          if ((rc = qc_piece(f, (const uint8_t*)c->raw.p, len)) != MK_OK) return rc;
          from = (size_t)end;
        }
        return MK_OK;
      },
      [&]() -> int {
        const auto t1 = MkClock::now();
        const u64* p = (const u64*)f.tables.p;
        for (int i = 0; i < 5; ++i)
          MK_HIP(hipMemcpyAsync(host[i], p + at[i], ((i < 4 ? at[i + 1] : total) - at[i]) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
        f.st.s_write += mk_since(t1);
        return MK_OK;
      });
}
