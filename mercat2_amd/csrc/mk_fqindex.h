// mk_fqindex.h -- the line index of a FASTQ text and the check of its sequence lines, shared by mk_fastq_select_*
// (mk_fqselect.hip, which has the scheme), mk_correct_fastq_* (mk_correctfq.hip) and mk_fastq_qtrim_* (mk_qtrim.hip):
// fs_tiles_k, fs_scan_k, fs_lines_k, the status word they leave, the phrases of the record checks (fs_kind), and the
// segment gather of the two calls that write records out (fs_gather_k, fs_edges_k).
#pragma once
#include "mk_recordplace.h"
#include "mk_tableview.h"
#include <rocprim/device/device_scan.hpp>

extern "C" int mk_fastq_cuts(const uint8_t* text, size_t n, uint64_t piece, uint64_t* cuts, size_t cap, size_t* ncuts);

#define FS_TILE 4096u            // text bytes a workgroup of the line passes owns: 256 lanes x 16
#define FS_FORCE (1ull << 63)    // in seg_src[s]: the segment's last output byte is '\n' whatever the source holds
#define FS_NONE (~0ull)          // FsStatus::bad: no record failed
// what failed, in the order the checks are made (the lowest record wins, then the lowest of these)
enum { FS_AT = 0, FS_PLUS = 1, FS_LENGTH = 2, FS_BLANK = 3, FS_KEPT = 4 };
// the bytes below 64 that a sequence line may not hold when kept[] counts its characters: what the parser strips or
// skips -- blanks (mk_is_blank), CR (unless it ends the line: fs_lines_k) and '*'; LF ends the line and is none of them
#define FS_BAD_BYTES ((1ull << 9) | (1ull << 11) | (1ull << 12) | (1ull << 13) | (0xFull << 28) | (1ull << 32) | (1ull << 42))

struct FsStatus {  // device memory, read back twice a piece: newlines after the scan, the rest after the decision
  u64 newlines, bad, records_out, records_trimmed, bases_out, pad;
};

// bit j set for every byte j of the word equal to ch (exact: no carries between bytes)
__device__ __forceinline__ unsigned fs_eq4(unsigned w, unsigned ch) {
  const unsigned x = w ^ (ch * 0x01010101u);
  const unsigned z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 in every zero byte
  return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// The lane's 16 bytes at `at` (a multiple of 16; fewer at the end of the text, zero behind it) and their newline mask.
struct FsSeg {
  unsigned w[4];
  unsigned len, nlmask;
};
__device__ __forceinline__ FsSeg fs_load(const uint8_t* __restrict__ text, u64 n, u64 at) {
  FsSeg s;
  if (at + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + at);
    s.w[0] = v.x; s.w[1] = v.y; s.w[2] = v.z; s.w[3] = v.w;
    s.len = 16;
  } else {
    s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0;
    s.len = at < n ? (unsigned)(n - at) : 0u;
    unsigned lo = 0, hi = 0, lo2 = 0, hi2 = 0;  // (no indexed register array: that would be scratch)
    for (unsigned j = 0; j < s.len; ++j) {
      const unsigned b = (unsigned)text[at + j] << (8 * (j & 3));
      if (j < 4) lo |= b;
      else if (j < 8) hi |= b;
      else if (j < 12) lo2 |= b;
      else hi2 |= b;
    }
    s.w[0] = lo; s.w[1] = hi; s.w[2] = lo2; s.w[3] = hi2;
  }
  s.nlmask = (fs_eq4(s.w[0], 10) | (fs_eq4(s.w[1], 10) << 4) | (fs_eq4(s.w[2], 10) << 8) | (fs_eq4(s.w[3], 10) << 12)) &
             ((1u << s.len) - 1u);
  return s;
}

static __global__ void __launch_bounds__(256) fs_tiles_k(const uint8_t* __restrict__ text, u64 n, unsigned* __restrict__ tile_cnt) {
  __shared__ unsigned s_wave[4];
  const FsSeg s = fs_load(text, n, (u64)blockIdx.x * FS_TILE + (u64)threadIdx.x * 16);
  const unsigned cnt = mk_wave_sum(__popc(s.nlmask));
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// One workgroup: tile_pre[i] = newlines in front of tile i (sc_tile_scan strides over any number of tiles); the total.
static __global__ void __launch_bounds__(1024) fs_scan_k(const unsigned* __restrict__ tile_cnt, size_t ntiles, u64* __restrict__ tile_pre,
                                                         FsStatus* __restrict__ st) {
  __shared__ u64 s_c[1024];
  const u64 total = sc_tile_scan(tile_cnt, ntiles, tile_pre, s_c);
  if (threadIdx.x == 0) st->newlines = total;
}

// line[L] = the byte behind the L-th '\n', for every line L <= nidx (= 4 * nrec) that starts inside the text; line[0] =
// 0, and line[nidx] = n where the host has found that no line nidx starts (end_is_n).  CHECK: a byte of a sequence line
// (phase 1) of a complete record that the parser would not count among the kept characters fails that record.
template <bool CHECK>
static __global__ void __launch_bounds__(256) fs_lines_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ tile_pre,
                                                         u64 nidx, int end_is_n, u64* __restrict__ line, FsStatus* __restrict__ st) {
  __shared__ unsigned s_wave[4];
  const u64 base = (u64)blockIdx.x * FS_TILE + (u64)threadIdx.x * 16;
  const FsSeg s = fs_load(text, n, base);
  const u64 first = tile_pre[blockIdx.x] + mk_block_scan_excl(__popc(s.nlmask), s_wave);  // the line open at the lane's first byte
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    line[0] = 0;
    if (end_is_n) line[nidx] = n;
  }
  u64 L = first;
  for (unsigned m = s.nlmask; m; m &= m - 1) {
    const u64 p = base + (unsigned)(__ffs(m) - 1) + 1;
    ++L;
    if (p < n && L <= nidx) line[L] = p;
  }
  if (CHECK) {
    u64 bad = FS_NONE, at = first;
#pragma unroll
    for (unsigned j = 0; j < 16; ++j) {  // (no early exit: unrolled, the words stay in registers)
      const unsigned ch = (s.w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      const bool nl = j < s.len && ch == 10u;
      bool fails = j < s.len && !nl && (at & 3) == 1 && at < nidx && ch < 64u && ((FS_BAD_BYTES >> (ch & 63u)) & 1ull);
      if (fails && ch == 13u) {  // one CR in front of the line's LF belongs to the terminator
        const unsigned next = j < 15 ? (j + 1 < s.len ? (s.w[((j + 1) & 15) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu : 0u)
                                     : (base + 16 < n ? (unsigned)text[base + 16] : 0u);
        fails = next != 10u;
      }
      const u64 mine = ((at >> 2) << 3) | FS_BLANK;
      if (fails && mine < bad) bad = mine;
      at += nl ? 1 : 0;
    }
    if (bad != FS_NONE) atomicMin((unsigned long long*)&st->bad, (unsigned long long)bad);
  }
}

// The gather of mk_fqselect.hip's scheme, shared with mk_qtrim.hip (four segments a record there).
// fl_gather_k over segments: segment s goes to [dst[s], dst[s + 1]) from seg_src[s] on; nseg of them.
#define FS_CHUNKS 4
static __global__ void __launch_bounds__(256) fs_gather_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ seg_src,
                                                          const u64* __restrict__ dst, size_t nseg, u64 head, u64 nbody,
                                                          uint8_t* __restrict__ out) {
  const u64 g0 = fl_first_lane((((u64)blockIdx.x * 256 + threadIdx.x) >> 6) * (64 * FS_CHUNKS));
  if (g0 >= nbody) return;
  size_t s = fl_record_of(dst, 0, nseg - 1, head + 16 * g0);
  for (int j = 0; j < FS_CHUNKS; ++j) {
    const u64 g = g0 + j * 64 + (threadIdx.x & 63);
    if (g >= nbody) break;
    const u64 o0 = head + 16 * g;
    s = fl_record_from(dst, s, nseg, o0);
    u64 end = dst[s + 1];
    u64 from = seg_src[s];
    u64 src = (from & ~FS_FORCE) + (o0 - dst[s]);
    unsigned __int128 v = 0;
    for (unsigned b = 0;;) {  // b: bytes of the chunk filled
      const u64 left = end - (o0 + b);  // (1 or more: the segment holds byte o0 + b)
      const unsigned m = left < 16 - b ? (unsigned)left : 16 - b;
      unsigned __int128 part = fl_load16(text, n, src);
      if (m < 16) part &= (((unsigned __int128)1) << (8 * m)) - 1;
      if ((from & FS_FORCE) && left <= 16 - b)  // the segment ends in this chunk: its last byte
        part = (part & ~(((unsigned __int128)0xFF) << (8 * (m - 1)))) | (((unsigned __int128)10) << (8 * (m - 1)));
      v |= part << (8 * b);
      b += m;
      if (b == 16) break;
      ++s;  // the segment ended inside the chunk (bytes follow: an emitted segment does)
      if (dst[s + 1] == dst[s]) s = fl_record_from(dst, s, nseg, o0 + b);
      end = dst[s + 1];
      from = seg_src[s];
      src = from & ~FS_FORCE;
    }
    const u64 v0 = (u64)v, v1 = (u64)(v >> 64);
    *reinterpret_cast<uint4*>(out + o0) = make_uint4((unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32));
  }
}

// The bytes in front of the first aligned 16 of the output (head of them) and behind the last (from tail_at on): a lane
// a byte, at most 15 + 15.
static __global__ void __launch_bounds__(64) fs_edges_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ seg_src,
                                                        const u64* __restrict__ dst, size_t nseg, u64 head, u64 tail_at, u64 out_len,
                                                        uint8_t* __restrict__ out) {
  u64 o;
  if (threadIdx.x < 16) o = threadIdx.x < head ? threadIdx.x : out_len;
  else if (threadIdx.x < 32) o = tail_at + (threadIdx.x - 16);
  else return;
  if (o >= out_len) return;
  const size_t s = fl_record_of(dst, 0, nseg - 1, o);
  const u64 from = seg_src[s], at = (from & ~FS_FORCE) + (o - dst[s]);
  const bool forced = (from & FS_FORCE) && o + 1 == dst[s + 1];
  out[o] = forced ? (uint8_t)10 : (at < n ? text[at] : (uint8_t)0);
}

static const char* fs_kind(unsigned kind) {
  switch (kind) {
    case FS_AT: return "its first line does not start with '@'";
    case FS_PLUS: return "its third line does not start with '+'";
    case FS_LENGTH: return "its sequence and quality lines differ in length";
    case FS_BLANK: return "its sequence line holds a blank or a '*' (kept[] counts the characters the parser keeps)";
    default: return "kept[r] is more than its sequence holds";
  }
}
