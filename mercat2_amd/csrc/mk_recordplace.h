// mk_recordplace.h -- where the records of a RAW text start and how an output-driven gather finds its bytes: what
// mk_filter_* (mk_filter.hip: whole records out) and mk_trim_* (mk_trim.hip: header lines and trimmed sequence out)
// share.  fl_tiles_k / fl_scan_k / fl_starts_k give start[r], the first byte of the header line of every row, and
// start[nrows] = n; fl_record_of / fl_record_from find the record of an output offset in dst[]; fl_load16 reads 16
// bytes at any address of a text.  The kernels are static: every file that includes them launches its own copy.
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
