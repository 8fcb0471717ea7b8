// mk_recordplace.h -- where the records of a RAW text start and how an output-driven gather finds its bytes: what
// mk_filter_* (mk_filter.hip: whole records out), mk_trim_* (mk_trim.hip: header lines and trimmed sequence out)
// and mk_norm_* (mk_norm.hip: whole records out, under another decision) share.  fl_tiles_k / fl_scan_k / fl_starts_k
// give start[r], the first byte of the header line of every row, and start[nrows] = n; fl_record_of / fl_record_from find the record of an output offset in dst[]; fl_load16 reads 16
// bytes at any address of a text; fl_gather_k / fl_edges_k copy whole records to their places and fl_emit is the tail
// of a piece that launches them.  The kernels are static: every file that includes them launches its own copy.
#pragma once
#include "mk_screenpiece.h"

#define FL_RUN 32                // text bytes a lane of the start kernels owns
#define FL_SPAN (256 * FL_RUN)   // ... a workgroup: one tile of the header scan

struct FlStatus {  // device memory, read back once a piece
  u64 headers, records_out;
};

// 0x80 in every byte of w that is '>' (exact per byte: no borrow between them)
__device__ __forceinline__ unsigned fl_gt_in(unsigned w) {
  const unsigned x = w ^ 0x3E3E3E3Eu;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// f(j, line) for the j-th header line whose '>' lies in the FL_RUN bytes at base: line = the first byte of that line.
// Returns how many there are.  A '>' opens a header line iff only blanks stand between it and the line's start.
template <class F>
__device__ __forceinline__ unsigned fl_headers_in(const uint8_t* __restrict__ text, u64 n, u64 base, F&& f) {
  unsigned cnt = 0;
  auto at = [&](u64 i) {
    u64 j = i;
    while (j > 0 && mk_is_blank(text[j - 1])) --j;
    if (j == 0 || mk_is_nl(text[j - 1])) f(cnt++, j);
  };
  if (base + FL_RUN <= n) {
    const uint4* p = reinterpret_cast<const uint4*>(text + base);  // (text is 16-byte aligned, base a multiple of 32)
#pragma unroll
    for (int i = 0; i < FL_RUN / 16; ++i) {
      const uint4 v = p[i];
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        for (unsigned m = fl_gt_in(w[q]); m; m &= m - 1) at(base + i * 16 + q * 4 + ((__ffs(m) - 1) >> 3));
    }
  } else {
    for (int j = 0; j < FL_RUN && base + j < n; ++j)
      if (text[base + j] == '>') at(base + j);
  }
  return cnt;
}

static __global__ void __launch_bounds__(256) fl_tiles_k(const uint8_t* __restrict__ text, u64 n, unsigned* __restrict__ tile_cnt) {
  __shared__ unsigned s_wave[4];
  const u64 base = (u64)blockIdx.x * FL_SPAN + (u64)threadIdx.x * FL_RUN;
  unsigned cnt = mk_wave_sum(fl_headers_in(text, n, base, [](unsigned, u64) {}));
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// One workgroup: tile_pre[i] = header lines in front of tile i (sc_tile_scan); their total goes to st.  The two starts
// no header line gives are written here: the end of the text behind the last row, byte 0 for a headless row 0.
static __global__ void __launch_bounds__(1024) fl_scan_k(const unsigned* __restrict__ tile_cnt, size_t ntiles, u64* __restrict__ tile_pre,
                                                  u64 n, size_t nrows, int headless, u64* __restrict__ start, FlStatus* __restrict__ st) {
  __shared__ u64 s_c[1024];
  const u64 headers = sc_tile_scan(tile_cnt, ntiles, tile_pre, s_c);
  if (threadIdx.x == 0) {
    st->headers = headers;
    start[nrows] = n;
    if (headless) start[0] = 0;
  }
}

// start[row_base + j] = the first byte of header line j (row_base 1: row 0 is the headless record).  A header line past
// the rows the parser counted is not written: the host's guard reports it.
static __global__ void __launch_bounds__(256) fl_starts_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ tile_pre,
                                                   u64 row_base, size_t nrows, u64* __restrict__ start) {
  __shared__ unsigned s_wave[4];
  const u64 base = (u64)blockIdx.x * FL_SPAN + (u64)threadIdx.x * FL_RUN;
  const unsigned own = fl_headers_in(text, n, base, [](unsigned, u64) {});
  const u64 first = row_base + tile_pre[blockIdx.x] + mk_block_scan_excl(own, s_wave);
  if (own)
    fl_headers_in(text, n, base, [&](unsigned j, u64 line) {
      if (first + j < nrows) start[first + j] = line;
    });
}

// The record whose output bytes hold offset o: the largest r in [lo, hi] with dst[r] <= o.  (A dropped record has
// dst[r] == dst[r + 1], so the largest such r is a kept one.)
__device__ __forceinline__ size_t fl_record_of(const u64* __restrict__ dst, size_t lo, size_t hi, u64 o) {
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (dst[mid] <= o) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ u64 fl_first_lane(u64 v) {
  return ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// The same from a record r that is known not to lie behind o's: steps of 1, 2, 4, ... records, then the search between
// the last two.  One load when o is still in r, 2 log2(d) + 1 for a record d further on.
__device__ __forceinline__ size_t fl_record_from(const u64* __restrict__ dst, size_t r, size_t nrows, u64 o) {
  size_t step = 1;
  while (r + step < nrows && dst[r + step] <= o) {
    r += step;
    step <<= 1;
  }
  return fl_record_of(dst, r, (r + step < nrows ? r + step : nrows) - 1, o);
}

// The 16 text bytes at src, which is not aligned: the two aligned 16 bytes around them, shifted together.  Within the
// last 32 bytes of the text, byte by byte; bytes behind the text read as 0.
__device__ __forceinline__ unsigned __int128 fl_load16(const uint8_t* __restrict__ text, u64 n, u64 src) {
  const u64 a = src & ~(u64)15;
  u64 y0 = 0, y1 = 0;
  if (a + 32 <= n) {
    const uint4* p = reinterpret_cast<const uint4*>(text + a);
    const uint4 lo = p[0], hi = p[1];
    u64 x0 = lo.x | ((u64)lo.y << 32), x1 = lo.z | ((u64)lo.w << 32), x2 = hi.x | ((u64)hi.y << 32);
    const u64 x3 = hi.z | ((u64)hi.w << 32);
    const unsigned s = (unsigned)(src & 15);
    if (s >= 8) { x0 = x1; x1 = x2; x2 = x3; }
    const unsigned sh = (s & 7) * 8;
    y0 = sh ? (x0 >> sh) | (x1 << (64 - sh)) : x0;
    y1 = sh ? (x1 >> sh) | (x2 << (64 - sh)) : x1;
  } else {
    for (int b = 0; b < 8; ++b) {
      if (src + b < n) y0 |= (u64)text[src + b] << (8 * b);
      if (src + 8 + b < n) y1 |= (u64)text[src + 8 + b] << (8 * b);
    }
  }
  return ((unsigned __int128)y1 << 64) | y0;
}

// Chunk g is the output bytes [head + 16 g, head + 16 g + 16), 16-byte aligned in memory; nbody of them.  A wave owns
// FL_CHUNKS KiB of them: in round j lane l takes chunk 64 j + l of the wave's, so that a store instruction of the wave
// writes 1 KiB in one piece.  The wave searches dst[] once, for the record of its first byte (the same loads in every
// lane); from there a lane steps forward (fl_record_from) to the record of each of its chunks: about six reads of 150
// bases further on each round, the same record all the way inside a contig.  A chunk is then filled record by record:
// the 16 bytes at the source (fl_load16) masked to what the record still has and shifted to their place.  One trip
// inside a record -- every chunk of a contig, nine in ten of 150-base reads -- and one more per record that starts in
// the chunk: sixteen at the most, whatever the records are.  The next record is r + 1, or, if that one is dropped, the
// next kept one, found by stepping on from it.
#define FL_CHUNKS 4
static __global__ void __launch_bounds__(256) fl_gather_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ start,
                                                          const u64* __restrict__ dst, size_t nrows, u64 head, u64 nbody,
                                                          uint8_t* __restrict__ out) {
  const u64 g0 = fl_first_lane((((u64)blockIdx.x * 256 + threadIdx.x) >> 6) * (64 * FL_CHUNKS));
  if (g0 >= nbody) return;
  size_t r = fl_record_of(dst, 0, nrows - 1, head + 16 * g0);
  for (int j = 0; j < FL_CHUNKS; ++j) {
    const u64 g = g0 + j * 64 + (threadIdx.x & 63);
    if (g >= nbody) break;
    const u64 o0 = head + 16 * g;
    r = fl_record_from(dst, r, nrows, o0);
    u64 end = dst[r + 1];
    u64 src = start[r] + (o0 - dst[r]);
    unsigned __int128 v = 0;
    for (unsigned b = 0;;) {  // b: bytes of the chunk filled
      const u64 left = end - (o0 + b);  // (1 or more: the record holds byte o0 + b)
      const unsigned m = left < 16 - b ? (unsigned)left : 16 - b;
      unsigned __int128 seg = fl_load16(text, n, src);
      if (m < 16) seg &= (((unsigned __int128)1) << (8 * m)) - 1;
      v |= seg << (8 * b);
      b += m;
      if (b == 16) break;
      ++r;  // the record ended inside the chunk (bytes follow: a kept record does)
      if (dst[r + 1] == dst[r]) r = fl_record_from(dst, r, nrows, o0 + b);
      end = dst[r + 1];
      src = start[r];
    }
    const u64 v0 = (u64)v, v1 = (u64)(v >> 64);
    *reinterpret_cast<uint4*>(out + o0) = make_uint4((unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32));
  }
}

// The bytes in front of the first aligned 16 of the output (head of them) and behind the last (from tail_at on): a lane
// a byte, at most 15 + 15.
static __global__ void __launch_bounds__(64) fl_edges_k(const uint8_t* __restrict__ text, const u64* __restrict__ start,
                                                        const u64* __restrict__ dst, size_t nrows, u64 head, u64 tail_at, u64 out_len,
                                                        uint8_t* __restrict__ out) {
  u64 o;
  if (threadIdx.x < 16) o = threadIdx.x < head ? threadIdx.x : out_len;
  else if (threadIdx.x < 32) o = tail_at + (threadIdx.x - 16);
  else return;
  if (o >= out_len) return;
  const size_t r = fl_record_of(dst, 0, nrows - 1, o);
  out[o] = text[start[r] + (o - dst[r])];
}

// ------------------------------------------------------------------------------------------ host side
// Where the records a call emits go, piece after piece.
struct FlEmit {
  uint8_t* out;       // text call: host memory, device call: device memory; out_cap bytes of room
  size_t out_cap;
  bool device;
  MkDevBuf stage;
  MkTimed gather;
  size_t bytes_out = 0;  // of all pieces so far, written or not
  FlEmit(mk_ctx* c, uint8_t* o, size_t oc, bool dev) : out(o), out_cap(oc), device(dev), gather(c) {}
  ~FlEmit() { buf_free(stage); }
};

// The tail of a piece of n bytes whose decision has been taken and scanned: record r goes to [dst[r], dst[r + 1]) of the
// piece's piece_out (= dst[nrows], which the caller has read back and checked against the text) output bytes, from
// start[r] on.  The gather writes into the caller's device memory, or into a staging buffer that is copied to the host.
// Without room the call goes on adding up and answers MK_ERR_RANGE at its end.  The stream is idle afterwards.
static int fl_emit(ScCall& s, FlEmit& e, const u64* start, const u64* dst, size_t n, size_t nrows, u64 piece_out, double& s_gather,
                   double& s_write) {
  mk_ctx* c = s.c;
  int rc;
  const uint8_t* text = s.last.text;
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
    hipLaunchKernelGGL(fl_gather_k, dim3((unsigned)div_up((size_t)nbody, 256 * FL_CHUNKS)), dim3(256), 0, c->stream, text, (u64)n, start,
                       dst, nrows, head, nbody, d_out);
  if (head || tail_at < piece_out)
    hipLaunchKernelGGL(fl_edges_k, dim3(1), dim3(64), 0, c->stream, text, start, dst, nrows, head, tail_at, piece_out, d_out);
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
