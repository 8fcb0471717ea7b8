// mk_screen.hip -- sequences in, per-record k-mer hits and abundance out (mk_screen_text / mk_screen_device,
// include/mercat_hip.h): the windows of every record of a FASTA text probed in the context's tables and reduced to one
// row {windows, hits, sum, min, max} a record.
//
// A piece of text goes through the general parser (mk_parse.hip) into the stream the count kernels slide over: kept
// characters, one MK_SEP where a header line starts.  The record of a position is the number of separators at or
// before it: sc_tiles_k counts them per tile, sc_scan_k (one workgroup) turns the counts into tile prefixes and the
// number of records, and the walk finishes the scan inside the workgroup.  sc_probe_k is the lane walk of
// mk_screenwalk.h with a row sink: a lane accumulates the counts of its windows while it stays in one record and adds
// them to the record's row where the record, or its run, ends.  Integer adds, min and max only: exact in any order.
#include "mk_screenwalk.h"

struct ScStatus {  // device memory, read back twice a piece: after the scan (nsep, headless), after the probe
  u64 nsep, headless;
  u64 windows, hits, packed, text, folded, locked;
};

__global__ void __launch_bounds__(256) sc_tiles_k(const uint8_t* __restrict__ seq, const MkChunkInfo* __restrict__ info,
                                                  unsigned* __restrict__ tile_cnt) {
  __shared__ unsigned s_wave[4];
  const u64 seq_len = info->seq_len, base = (u64)blockIdx.x * SC_SPAN + (u64)threadIdx.x * SC_RUN;
  unsigned n = 0;
  if (base + SC_RUN <= seq_len) {
    const uint4* p = reinterpret_cast<const uint4*>(seq + base);  // (seq is 256-byte aligned, base a multiple of 32)
#pragma unroll
    for (int i = 0; i < SC_RUN / 16; ++i) {
      const uint4 v = p[i];
      n += sc_seps_in(v.x) + sc_seps_in(v.y) + sc_seps_in(v.z) + sc_seps_in(v.w);
    }
  } else {
    for (int j = 0; j < SC_RUN && base + j < seq_len; ++j) n += seq[base + j] == MK_SEP;
  }
  n = mk_wave_sum(n);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// One workgroup: tile_pre[i] = separators in front of tile i (sc_tile_scan); their total and whether kept characters
// stand in front of the first go to st.
__global__ void __launch_bounds__(1024) sc_scan_k(const unsigned* __restrict__ tile_cnt, size_t ntiles, u64* __restrict__ tile_pre,
                                                  const uint8_t* __restrict__ seq, const MkChunkInfo* __restrict__ info,
                                                  ScStatus* __restrict__ st) {
  __shared__ u64 s_c[1024];
  const u64 nsep = sc_tile_scan(tile_cnt, ntiles, tile_pre, s_c);
  if (threadIdx.x == 0) {
    st->nsep = nsep;
    st->headless = (info->seq_len && seq[0] != MK_SEP) ? 1 : 0;
  }
}

__global__ void __launch_bounds__(256) sc_rows_init_k(mk_screen_row_t* __restrict__ rows, size_t n) {
  mk_for_each(n, [&](size_t i) { rows[i] = mk_screen_row_t{0, 0, 0, ~0ull, 0}; });
}
// (a record without windows: its min was never written)
__global__ void __launch_bounds__(256) sc_rows_final_k(mk_screen_row_t* __restrict__ rows, size_t n) {
  mk_for_each(n, [&](size_t i) { if (rows[i].windows == 0) rows[i].min = 0; });
}

// What a lane has gathered for the record it is in.
struct ScAcc {
  u64 windows = 0, hits = 0, sum = 0, mn = ~0ull, mx = 0;
  __device__ __forceinline__ void add(u64 cnt, u64 at_least) {
    ++windows;
    hits += cnt >= at_least ? 1 : 0;
    sum += cnt;
    mn = cnt < mn ? cnt : mn;
    mx = cnt > mx ? cnt : mx;
  }
  __device__ __forceinline__ void flush(mk_screen_row_t* __restrict__ rows, u64 row) {  // (nothing gathered: no row is touched)
    if (!windows) return;
    mk_screen_row_t* r = rows + row;
    atomicAdd((unsigned long long*)&r->windows, windows);
    if (hits) atomicAdd((unsigned long long*)&r->hits, hits);
    if (sum) atomicAdd((unsigned long long*)&r->sum, sum);
    atomicMin((unsigned long long*)&r->min, mn);
    if (mx) atomicMax((unsigned long long*)&r->max, mx);
    *this = ScAcc();
  }
};

// The row sink of the walk: the lane's counts go to the row of the record they belong to when the record ends.
struct ScRowSink {
  mk_screen_row_t* __restrict__ rows;
  u64 row_base, at_least;
  ScAcc acc;
  u64 hits = 0;  // of the lane's whole run, for ScStatus
  __device__ __forceinline__ void begin(u64, u64) {}
  __device__ __forceinline__ void record_end(u64 rid) { acc.flush(rows, rid - row_base); }
  __device__ __forceinline__ void window(u64, unsigned, u64 cnt) {
    hits += cnt >= at_least ? 1 : 0;
    acc.add(cnt, at_least);
  }
};

// Grid: one workgroup per tile of SC_SPAN positions.  row_base: the record number of row 0 (1, or 0 when the piece
// starts with a record that has no header line).  LDS false: KEYS == TL_TEXT_ONLY with a k whose halo LDS cannot hold.
template <int KEYS, bool FOLD, bool LDS>
__global__ void __launch_bounds__(256) sc_probe_k(const uint8_t* __restrict__ seq, u64 seq_len, const u64* __restrict__ tile_pre,
                                                  u64 row_base, int k, int bits, u64 at_least, LkTables t,
                                                  mk_screen_row_t* __restrict__ rows, ScStatus* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_seq[];  // sc_span_bytes(k)
  ScRowSink sink{rows, row_base, at_least};
  ScWalked n;
  const u64 rid = sc_walk<KEYS, FOLD, LDS>(s_seq, seq, seq_len, tile_pre, k, bits, t, sink, n);
  ScAcc& acc = sink.acc;  // what the lane holds belongs to the record it ends in
  // The whole wave ends in one record (the normal case inside a contig): reduce across it, one lane flushes -- five
  // atomics a wave on the record's row instead of 320.  (Measured, DESIGN 8m: one 100 Mbase record 2.3 ms with it, 73 ms
  // with every lane flushing for itself; 150 bp reads the same either way.)
  if (__all(rid == __shfl(rid, 0))) {
    for (int d = 32; d > 0; d >>= 1) {
      acc.windows += __shfl_down(acc.windows, d);
      acc.hits += __shfl_down(acc.hits, d);
      acc.sum += __shfl_down(acc.sum, d);
      const u64 mn = __shfl_down(acc.mn, d), mx = __shfl_down(acc.mx, d);
      acc.mn = mn < acc.mn ? mn : acc.mn;
      acc.mx = mx > acc.mx ? mx : acc.mx;
    }
    if (threadIdx.x & 63) acc.windows = 0;
  }
  acc.flush(rows, rid - row_base);
  block_add(&st->windows, n.windows);
  block_add(&st->hits, sink.hits);
  block_add(&st->packed, n.packed);
  block_add(&st->text, n.text);
  block_add(&st->folded, n.folded);
  if (n.locked) atomicAdd(&st->locked, 1ull);  // (cannot happen on a quiescent table)
}

// ------------------------------------------------------------------------------------------ host side
static int sc_launch_probe(ScCall& s, size_t seq_len, const u64* tile_pre, u64 row_base, mk_screen_row_t* d_rows, ScStatus* d_st) {
  mk_ctx* c = s.c;
  const LkTables t = lk_tables(c);
  const unsigned grid = (unsigned)div_up(seq_len, SC_SPAN);
  sc_dispatch_walk(s, [&](auto keys, auto fold, auto lds) {
    hipLaunchKernelGGL((sc_probe_k<decltype(keys)::value, decltype(fold)::value, decltype(lds)::value>), dim3(grid), dim3(256),
                       decltype(lds)::value ? sc_span_bytes(c->k) : 0, c->stream, (const uint8_t*)c->seq.p, (u64)seq_len, tile_pre,
                       row_base, c->k, c->bits, s.at_least, t, d_rows, d_st);
    return MK_OK;
  });
  MK_HIP(hipGetLastError());
  return MK_OK;
}

// The piece routine both callers share (declared in mk_screenpiece.h).
int sc_piece(ScCall& s, const uint8_t* d_text, size_t n, mk_screen_row_t* d_rows, size_t room, MkDevBuf* own,
             mk_screen_row_t* h_rows) {
  mk_ctx* c = s.c;
  int rc;
  const size_t ntiles = div_up(n, SC_SPAN);  // (the stream is no longer than the text)
  const size_t pre_off = (sizeof(ScStatus) + 15) & ~(size_t)15;
  if ((rc = mk_buf_reserve(c, s.scratch, pre_off + ntiles * (sizeof(u64) + sizeof(unsigned)) + 16)) != MK_OK) return rc;
  ScStatus* d_st = (ScStatus*)s.scratch.p;
  u64* tile_pre = (u64*)((char*)s.scratch.p + pre_off);
  unsigned* tile_cnt = (unsigned*)(tile_pre + ntiles);
  if ((rc = mk_buf_reserve(c, c->seq, n + 256)) != MK_OK) return rc;
  if ((uintptr_t)d_text & 15) {  // (the general transducer loads 16 bytes at a time)
    if ((rc = mk_buf_reserve(c, c->raw, n + 64)) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(c->raw.p, d_text, n, hipMemcpyDeviceToDevice, c->stream));
    d_text = (const uint8_t*)c->raw.p;
  }
  s.last = {d_text, nullptr, 0, false, nullptr, 0, 0};
  MkChunkInfo info{};
  ScStatus h{};
  MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
  MK_HIP(hipMemsetAsync(d_st, 0, sizeof(ScStatus), c->stream));
  if ((rc = s.parse.begin()) != MK_OK || (rc = mk_launch_parse(c, d_text, n)) != MK_OK) return rc;
  hipLaunchKernelGGL(sc_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const uint8_t*)c->seq.p, (const MkChunkInfo*)c->info.p, tile_cnt);
  hipLaunchKernelGGL(sc_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, (const uint8_t*)c->seq.p,
                     (const MkChunkInfo*)c->info.p, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = s.parse.end()) != MK_OK) return rc;
  MK_HIP(hipMemcpyAsync(&info, c->info.p, sizeof info, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = s.parse.add_to(s.out.s_parse)) != MK_OK) return rc;
  if (info.non_ascii) {
    c->err = std::string(s.what) + ": the text holds " + std::to_string(info.non_ascii) +
             " sequence byte(s) >= 0x80 (non-ASCII sequence text is not supported)";
    return MK_ERR_NON_ASCII;
  }
  const size_t nrows = (size_t)(h.nsep + h.headless);
  const size_t first = s.rows_seen;
  s.rows_seen += nrows;
  s.out.bytes += n;
  s.out.pieces += 1;
  if (h.headless) s.out.headless = 1;
  s.last.nrows = nrows;
  s.last.headless = h.headless != 0;
  // (what the parse and the scan left is the caller's with or without rows: room 0 is the call that wants no probe)
  s.last.tile_pre = tile_pre;
  s.last.seq_len = (size_t)info.seq_len;
  s.last.row_base = h.headless ? 0 : 1;
  if (!nrows || nrows > room) return MK_OK;  // (too many: the call goes on counting records and answers MK_ERR_RANGE)
  if (!d_rows) {
    if ((rc = mk_buf_reserve(c, *own, nrows * sizeof(mk_screen_row_t))) != MK_OK) return rc;
    d_rows = (mk_screen_row_t*)own->p;
  }
  s.last.d_rows = d_rows;
  if ((rc = s.probe.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(sc_rows_init_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, d_rows, nrows);
  if (info.seq_len && (rc = sc_launch_probe(s, (size_t)info.seq_len, tile_pre, h.headless ? 0 : 1, d_rows, d_st)) != MK_OK) return rc;
  hipLaunchKernelGGL(sc_rows_final_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, d_rows, nrows);
  MK_HIP(hipGetLastError());
  if ((rc = s.probe.end()) != MK_OK) return rc;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  if (h_rows) MK_HIP(hipMemcpyAsync(h_rows + first, d_rows, nrows * sizeof(mk_screen_row_t), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = s.probe.add_to(s.out.s_probe)) != MK_OK) return rc;
  if (h.locked) {
    c->err = std::string(s.what) + ": a slot of the table was being claimed: something counts into it during the call";
    return MK_ERR_STATE;
  }
  if (h.packed + h.text != h.windows) {
    c->err = std::string(s.what) + ": the probe kernel lost windows (internal error)";
    return MK_ERR_STATE;
  }
  s.out.windows += h.windows;
  s.out.hits += h.hits;
  s.out.packed_windows += h.packed;
  s.out.text_windows += h.text;
  s.out.folded += h.folded;
  return MK_OK;
}

extern "C" int mk_screen_device(mk_ctx* c, const uint8_t* d_text, size_t n, unsigned flags, uint64_t at_least,
                                mk_screen_row_t* d_rows, size_t cap, size_t* nrows, mk_screen_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (cap && !d_rows)) { c->err = "mk_screen_device: NULL buffer"; return MK_ERR_ARG; }
  return sc_run(c, "mk_screen_device", flags, at_least, cap, nrows, st,
                [&](ScCall& s) { return n ? sc_piece(s, d_text, n, d_rows, cap, nullptr, nullptr) : MK_OK; });
}

extern "C" int mk_screen_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, uint64_t at_least,
                              mk_screen_row_t* rows, size_t cap, size_t* nrows, mk_screen_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (cap && !rows)) { c->err = "mk_screen_text: NULL buffer"; return MK_ERR_ARG; }
  MkDevBuf d_rows;
  const int rc = sc_run(c, "mk_screen_text", flags, at_least, cap, nrows, st, [&](ScCall& s) -> int {
    return sc_text_pieces(s, text, n, piece_bytes, [&](const uint8_t* d_piece, size_t len) {
      const size_t room = cap > s.rows_seen ? cap - s.rows_seen : 0;
      return sc_piece(s, d_piece, len, nullptr, room, &d_rows, rows);
    });
  });
  buf_free(d_rows);
  return rc;
}
