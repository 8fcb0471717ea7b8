// mk_trimwalk.h -- a record cut in front of its first low window, found and written: what mk_trim_* (mk_trim.hip: every
// record on its own) and mk_pairs_* (mk_pairs.hip: the mates of a pair together) share; mk_correct_* (mk_correct.hip)
// takes tr_hend_k and tr_emit for records it writes whole.  tr_hend_k gives hlen[r];
// tr_first_k is the walk of mk_screenwalk.h with a sink that keeps the first low window of every record; tr_decide_k
// turns it into kept[r] and the record's output length; tr_gather_k / tr_edges_k write a record from its two sources and
// tr_emit is the tail of a piece that launches them.  The kernels that are no templates are static: every file that
// includes them launches its own copy.
#pragma once
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
static __global__ void __launch_bounds__(256) tr_hend_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ start, size_t nrows,
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
static __global__ void __launch_bounds__(256) tr_decide_k(const mk_screen_row_t* __restrict__ rows, const u64* __restrict__ first_low,
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
  u64 lf;                       // 1; 0 where kept[r] == 0: a header line alone, which only mk_correct_* emits
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
    const u64 kp = kept[r];
    return TrRec{dst[r], start[r], h, sstart[r], h + kp, kp ? 1ull : 0ull};
  }
};

// Chunks, rounds and the search as in fl_gather_k.  A chunk is filled segment by segment: up to 16 bytes of the header
// line (raw text), of the kept symbols (stream), or the LF, masked to what the segment still has and shifted to their
// place; the record after an LF is r + 1, or the next emitted one.  A record mk_trim_* emits holds k + 1 bytes or more;
// mk_correct_* emits every record, a header line alone without the LF (lf == 0), and a chunk may hold several of them.
#define TR_CHUNKS 4
static __global__ void __launch_bounds__(256) tr_gather_k(TrPlace p, u64 head, u64 nbody, uint8_t* __restrict__ out) {
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
      if (q + m < c.body + c.lf) continue;  // (the record's last byte was not among them: the same record goes on)
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
static __global__ void __launch_bounds__(64) tr_edges_k(TrPlace p, u64 head, u64 tail_at, u64 out_len, uint8_t* __restrict__ out) {
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

// fl_emit's counterpart for trimmed records: the tail of a piece whose decision has been taken and scanned.  Record r
// of p goes to [p.dst[r], p.dst[r + 1]) of the piece's piece_out (= p.dst[p.nrows], read back and checked by the
// caller) output bytes.  The gather writes into the caller's device memory, or into a staging buffer that is copied to
// the host.  Without room the call goes on adding up and answers MK_ERR_RANGE at its end.  The stream is idle afterwards.
static int tr_emit(ScCall& s, FlEmit& e, const TrPlace& p, u64 piece_out, double& s_gather, double& s_write) {
  mk_ctx* c = s.c;
  int rc;
  const size_t at = e.bytes_out;
  e.bytes_out += (size_t)piece_out;
  if (!piece_out || e.bytes_out > e.out_cap) return MK_OK;
  uint8_t* d_out = e.out + at;
  if (!e.device) {
    if ((rc = mk_buf_reserve(c, e.stage, (size_t)piece_out)) != MK_OK) return rc;
    d_out = (uint8_t*)e.stage.p;
  }
  const u64 head = std::min<u64>((16 - ((uintptr_t)d_out & 15)) & 15, piece_out);
  const u64 nbody = (piece_out - head) / 16, tail_at = head + 16 * nbody;
  if ((rc = e.gather.begin()) != MK_OK) return rc;
  if (nbody)
    hipLaunchKernelGGL(tr_gather_k, dim3((unsigned)div_up((size_t)nbody, 256 * TR_CHUNKS)), dim3(256), 0, c->stream, p, head, nbody, d_out);
  if (head || tail_at < piece_out) hipLaunchKernelGGL(tr_edges_k, dim3(1), dim3(64), 0, c->stream, p, head, tail_at, piece_out, d_out);
  MK_HIP(hipGetLastError());
  if ((rc = e.gather.end()) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = e.gather.add_to(s_gather)) != MK_OK) return rc;
  if (!e.device) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(e.out + at, d_out, (size_t)piece_out, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    s_write += mk_since(t1);
  }
  return MK_OK;
}
