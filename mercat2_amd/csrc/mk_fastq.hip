// mk_fastq.hip -- FASTQ mode (mk_set_fastq): a chunk of raw FASTQ text counted as MerCat2's fq2fa leaves it.
//
// fq2fa (lib/mercat2_fasta.py:175-198) is `sed -n '1~4s/^@/>/p;2~4p'` read back in universal-newline text mode: lines
// are split on '\n' only and numbered across the file; line 4i+1 is kept with its '@' made a '>' when it starts with
// '@' and dropped otherwise, line 4i+2 is kept as it stands, lines 4i+3 and 4i+4 are dropped.  find_kmers takes an
// empty line for nothing, and the parser already reads '\r\n' and a lone '\r' as find_kmers does, so the chunk is
// rewritten IN PLACE before the parser, with nothing moved:
//   every byte of a dropped line -> '\n';  the '@' of a kept line 4i+1 -> '>';  line 4i+2 untouched.
// What a byte needs is its line's number mod 4 (the '\n' in front of it) and, on a line 4i+1, whether that line
// started with '@' -- possibly many tiles before.  Three launches, tiles of 4 KiB (256 lanes x 16 bytes):
//   1 mk_fq_summ_k  per tile: its '\n' count and what it does to the class of the line still open at its end
//   2 mk_fq_scan_k  one workgroup composes the tiles in order: each tile's entering line number and class
//   3 mk_fq_apply_k per tile: the lanes' entering states (a scan in the workgroup), the rewrite, the stats
// A class is 0 = a line starts at the next byte, 1 = the open line started with '@', 2 = it did not.  What a piece of
// text does to the class is a map of {0, 1, 2} onto itself, kept as three 2-bit fields (composing two pieces is a
// table look-up): a piece with a '\n' maps everything to the class of its last line; a piece without one maps 0 to the
// class of its first byte and keeps 1 and 2; an empty piece is the identity.
// Stats (since mk_reset, on the device): [0] lines [1] kept headers [2] dropped headers [3] kept bytes [4] '\r\n' pairs
// in kept lines.  The text fq2fa writes is kept bytes - '\r\n' pairs long.
#include "mk_common.h"

typedef unsigned long long u64;

#define FQ_TILE 4096u
#define FQ_THREADS 256
#define FQ_ID 36u  // identity map: 0 -> 0, 1 -> 1, 2 -> 2

__device__ __forceinline__ unsigned fq_cls_at(unsigned m, unsigned s) { return (m >> (2 * s)) & 3u; }
// a first, then b
__device__ __forceinline__ unsigned fq_compose(unsigned a, unsigned b) {
  return fq_cls_at(b, fq_cls_at(a, 0)) | (fq_cls_at(b, fq_cls_at(a, 1)) << 2) | (fq_cls_at(b, fq_cls_at(a, 2)) << 4);
}

__device__ __forceinline__ unsigned fq_byte(const uint4& v, unsigned j) {
  const unsigned w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
  return (w >> (8 * (j & 3))) & 0xFFu;
}

// bit j set for every byte j of the word equal to ch (exact: no carries between bytes)
__device__ __forceinline__ unsigned fq_eq4(unsigned w, unsigned ch) {
  const unsigned x = w ^ (ch * 0x01010101u);
  const unsigned z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 in every zero byte
  return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// the lane's 16 bytes (fewer at the end of the text; past it: zero, outside the mask)
struct FqSeg {
  uint4 v;
  unsigned len, nlmask;
};

__device__ __forceinline__ FqSeg fq_load(const uint8_t* __restrict__ raw, size_t at, size_t n) {
  FqSeg s;
  if (at + 16 <= n) {
    s.v = *(const uint4*)(raw + at);
    s.len = 16;
  } else {
    unsigned w[4] = {0, 0, 0, 0};
    s.len = at < n ? (unsigned)(n - at) : 0u;
    for (unsigned j = 0; j < s.len; ++j) w[j >> 2] |= (unsigned)raw[at + j] << (8 * (j & 3));
    s.v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  s.nlmask = (fq_eq4(s.v.x, 10) | (fq_eq4(s.v.y, 10) << 4) | (fq_eq4(s.v.z, 10) << 8) | (fq_eq4(s.v.w, 10) << 12)) &
             ((1u << s.len) - 1u);
  return s;
}

// what the piece does to the class of the open line
__device__ __forceinline__ unsigned fq_map(const FqSeg& s) {
  if (!s.len) return FQ_ID;
  if (s.nlmask) {
    const unsigned p = 31u - __builtin_clz(s.nlmask);
    const unsigned t = p + 1 >= s.len ? 0u : (fq_byte(s.v, p + 1) == '@' ? 1u : 2u);
    return t | (t << 2) | (t << 4);
  }
  return (fq_byte(s.v, 0) == '@' ? 1u : 2u) | (1u << 2) | (2u << 4);
}

// inclusive scan of (newlines, map) over the workgroup's lanes in order; returns the EXCLUSIVE prefix of this lane and
// the workgroup's total
__device__ __forceinline__ void fq_block_scan(unsigned nl, unsigned m, unsigned& ex_nl, unsigned& ex_m, unsigned& tot_nl,
                                              unsigned& tot_m, unsigned* s_nl, unsigned* s_m) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned onl = __shfl_up(nl, d), om = __shfl_up(m, d);
    if ((int)lane >= d) { nl += onl; m = fq_compose(om, m); }
  }
  unsigned pnl = __shfl_up(nl, 1), pm = __shfl_up(m, 1);
  if (lane == 0) { pnl = 0; pm = FQ_ID; }
  if (lane == 63) { s_nl[wave] = nl; s_m[wave] = m; }
  __syncthreads();
  unsigned wnl = 0, wm = FQ_ID;
  for (unsigned w = 0; w < wave; ++w) { wnl += s_nl[w]; wm = fq_compose(wm, s_m[w]); }
  ex_nl = wnl + pnl;
  ex_m = fq_compose(wm, pm);
  tot_nl = 0;
  tot_m = FQ_ID;
  for (unsigned w = 0; w < FQ_THREADS / 64; ++w) { tot_nl += s_nl[w]; tot_m = fq_compose(tot_m, s_m[w]); }
  __syncthreads();  // (s_nl / s_m are reused by the next tile)
}

// summ[t] = newlines << 8 | (last byte of the tile is '\r') << 7 | map
__global__ __launch_bounds__(FQ_THREADS) void mk_fq_summ_k(const uint8_t* __restrict__ raw, size_t n, size_t tiles,
                                                            unsigned* __restrict__ summ) {
  __shared__ unsigned s_nl[FQ_THREADS / 64], s_m[FQ_THREADS / 64];
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const size_t at = t * FQ_TILE + (size_t)threadIdx.x * 16;
    const FqSeg s = fq_load(raw, at, n);
    unsigned ex_nl, ex_m, tot_nl, tot_m;
    fq_block_scan(__builtin_popcount(s.nlmask), fq_map(s), ex_nl, ex_m, tot_nl, tot_m, s_nl, s_m);
    if (threadIdx.x == FQ_THREADS - 1) {
      const unsigned cr = s.len == 16 && fq_byte(s.v, 15) == 13u;
      summ[t] = (tot_nl << 8) | (cr << 7) | tot_m;
    }
  }
}

// enter[t] = line number of the tile's first byte << 2 | class of the line open in front of it;
// stats[0] += lines of the text (a last line without '\n' is one)
__global__ __launch_bounds__(1024) void mk_fq_scan_k(const uint8_t* __restrict__ raw, size_t n, size_t tiles,
                                                      const unsigned* __restrict__ summ, u64* __restrict__ enter,
                                                      u64* __restrict__ stats) {
  __shared__ u64 s_nl[1024];
  __shared__ unsigned s_m[1024];
  const unsigned tid = threadIdx.x;
  const size_t per = (tiles + 1023) / 1024;
  const size_t a = (size_t)tid * per, b = a + per < tiles ? a + per : tiles;
  u64 nl = 0;
  unsigned m = FQ_ID;
  for (size_t t = a; t < b; ++t) { nl += summ[t] >> 8; m = fq_compose(m, summ[t] & 63u); }
  s_nl[tid] = nl;
  s_m[tid] = m;
  __syncthreads();
  for (unsigned d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan, composition in order
    u64 onl = 0;
    unsigned om = FQ_ID;
    if (tid >= d) { onl = s_nl[tid - d]; om = s_m[tid - d]; }
    __syncthreads();
    if (tid >= d) { s_nl[tid] += onl; s_m[tid] = fq_compose(om, s_m[tid]); }
    __syncthreads();
  }
  u64 line = tid ? s_nl[tid - 1] : 0;
  unsigned cls = fq_cls_at(tid ? s_m[tid - 1] : FQ_ID, 0);  // (the text starts with a line)
  for (size_t t = a; t < b; ++t) {
    enter[t] = (line << 2) | cls;
    line += summ[t] >> 8;
    cls = fq_cls_at(summ[t] & 63u, cls);
  }
  if (tid == 1023 && n) stats[0] += s_nl[1023] + (raw[n - 1] != 10u ? 1ull : 0ull);
}

__global__ __launch_bounds__(FQ_THREADS) void mk_fq_apply_k(uint8_t* __restrict__ raw, size_t n, size_t tiles,
                                                             const unsigned* __restrict__ summ,
                                                             const u64* __restrict__ enter, u64* __restrict__ stats) {
  __shared__ unsigned s_nl[FQ_THREADS / 64], s_m[FQ_THREADS / 64];
  __shared__ unsigned s_last[2][FQ_THREADS];  // (by the parity of the workgroup's tile: read after the next tile's barriers)
  unsigned reads = 0, dropped = 0, kept = 0, crlf = 0, par = 0;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x, par ^= 1) {
    const size_t at = t * FQ_TILE + (size_t)threadIdx.x * 16;
    const FqSeg s = fq_load(raw, at, n);
    s_last[par][threadIdx.x] = s.len ? fq_byte(s.v, s.len - 1) : 0u;
    unsigned ex_nl, ex_m, tot_nl, tot_m;
    fq_block_scan(__builtin_popcount(s.nlmask), fq_map(s), ex_nl, ex_m, tot_nl, tot_m, s_nl, s_m);
    // (every lane has loaded its bytes before the scan's barrier: the rewrite below cannot reach a neighbour's load)
    const u64 e = enter[t];
    u64 line = (e >> 2) + ex_nl;
    unsigned cls = fq_cls_at(ex_m, (unsigned)(e & 3));
    unsigned prev = threadIdx.x ? s_last[par][threadIdx.x - 1] : (t && ((summ[t - 1] >> 7) & 1u) ? 13u : 0u);
    unsigned w[4] = {s.v.x, s.v.y, s.v.z, s.v.w};
    bool changed = false;
    for (unsigned j = 0; j < s.len; ++j) {
      const unsigned ch = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      const bool start = cls == 0;
      if (start) cls = ch == '@' ? 1u : 2u;
      const unsigned ph = (unsigned)line & 3u;
      const bool keep = ph == 1 || (ph == 0 && cls == 1);
      reads += start && ph == 0 && cls == 1;
      dropped += start && ph == 0 && cls == 2;
      kept += keep;
      crlf += keep && ch == 10u && prev == 13u;
      const unsigned out = keep ? ((start && ph == 0) ? (unsigned)'>' : ch) : 10u;
      if (out != ch) {
        w[j >> 2] = (w[j >> 2] & ~(0xFFu << (8 * (j & 3)))) | (out << (8 * (j & 3)));
        changed = true;
      }
      if (ch == 10u) { ++line; cls = 0; }
      prev = ch;
    }
    if (changed) {
      if (s.len == 16) {
        *(uint4*)(raw + at) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (unsigned j = 0; j < s.len; ++j) raw[at + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    reads += __shfl_down(reads, d);
    dropped += __shfl_down(dropped, d);
    kept += __shfl_down(kept, d);
    crlf += __shfl_down(crlf, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (reads) atomicAdd(&stats[1], (u64)reads);
    if (dropped) atomicAdd(&stats[2], (u64)dropped);
    if (kept) atomicAdd(&stats[3], (u64)kept);
    if (crlf) atomicAdd(&stats[4], (u64)crlf);
  }
}

// the stats words, zeroed (mk_set_fastq, mk_reset)
int mk_fastq_clear(mk_ctx* c) {
  int rc = mk_buf_reserve(c, c->fastq_stats, 8 * sizeof(u64));
  if (rc) return rc;
  MK_HIP(hipMemsetAsync(c->fastq_stats.p, 0, 8 * sizeof(u64), c->stream));
  return MK_OK;
}

// before the parser: raw bytes [0, n) of the chunk (the context's own buffer), in place
int mk_launch_fastq_pre(mk_ctx* c, uint8_t* d_raw, size_t n) {
  if (!n) return MK_OK;
  const size_t tiles = (n + FQ_TILE - 1) / FQ_TILE;
  int rc = mk_buf_reserve(c, c->fastq_tiles, tiles * (sizeof(unsigned) + sizeof(u64)) + 64);
  if (rc) return rc;
  if (!c->fastq_stats.p && (rc = mk_fastq_clear(c)) != MK_OK) return rc;
  u64* enter = (u64*)c->fastq_tiles.p;
  unsigned* summ = (unsigned*)(enter + tiles);
  u64* stats = (u64*)c->fastq_stats.p;
  // (each workgroup takes tiles t, t + grid, ...: the stats are summed in registers over them, one atomic per wave and field)
  const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
  hipLaunchKernelGGL(mk_fq_summ_k, dim3(grid), dim3(FQ_THREADS), 0, c->stream, (const uint8_t*)d_raw, n, tiles, summ);
  hipLaunchKernelGGL(mk_fq_scan_k, dim3(1), dim3(1024), 0, c->stream, (const uint8_t*)d_raw, n, tiles, (const unsigned*)summ, enter, stats);
  hipLaunchKernelGGL(mk_fq_apply_k, dim3(grid), dim3(FQ_THREADS), 0, c->stream, d_raw, n, tiles, (const unsigned*)summ,
                     (const u64*)enter, stats);
  MK_HIP(hipGetLastError());
  return MK_OK;
}
