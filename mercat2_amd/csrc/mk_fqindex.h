// mk_fqindex.h -- what every call that reads a FASTQ text piece by piece on the GPU shares: mk_fastq_select_*
// (mk_fqselect.hip), mk_correct_fastq_* (mk_correctfq.hip), mk_fastq_qc_* (mk_qc.hip) and, through mk_fqpiece.h,
// mk_fastq_qtrim_* / mk_fastq_adapt_* / mk_fastq_overlap_* / mk_fastq_dedup_*.
//   device side   the line index (fs_tiles_k, fs_scan_k, fs_lines_k and the check of the sequence lines), the status word
//                 they leave, and the segment gather of the calls that write records out (fs_gather_k, fs_edges_k).
//   host side     the steps of a piece, each written once, beside the kernels they launch: fs_index_open (tiles, scan,
//                 the read-back, lines / records / what trails), fs_index_lines, fs_gather; the two messages of a
//                 malformed record (fs_msg_incomplete, fs_msg_malformed) and the phrases of the checks (fs_kind); the
//                 piece plan of a text call (fs_piece_cuts over tl_piece_size); the aligned copy of a device text
//                 (fs_aligned_text); how a call opens and ends (fs_call, fs_call_end, fs_out_room).
// A piece is: fs_index_open, the call's own reservations, fs_index_lines, the call's kernels, its read-back and -- where
// records are written -- fs_gather.  What differs between the calls stays with them.
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

// The gather of the calls that write records out (two segments a record in mk_fqselect.hip, four in mk_fqpiece.h):
// output-driven, a lane owns 16 aligned output bytes a round, one search a wave, fl_record_from from there, fl_load16 /
// mask / shift / OR per segment, and the last byte of a flagged segment that ends in the chunk replaced by '\n' -- the
// base behind a trimmed prefix, the '\r' of CR LF, the 0 that fl_load16 reads behind a text without final newline.  No
// atomics, plain 16-byte stores, byte stores (fs_edges_k) for the at most 15 + 15 edge bytes only.
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

// ------------------------------------------------------------------------------------------ host side
// The two messages of a malformed record: the text ends inside record `record`, or the record fails check `kind`.
static std::string fs_msg_incomplete(const char* what, size_t record, unsigned trailing) {
  return std::string(what) + ": record " + std::to_string(record) + " is malformed: the text ends inside it (" + std::to_string(trailing) +
         " of its 4 lines)";
}
static std::string fs_msg_malformed(const char* what, size_t record, const char* kind, bool malformed = true) {
  return std::string(what) + ": record " + std::to_string(record) + (malformed ? " is malformed: " : ": ") + kind;
}

// What fs_index_open leaves of a piece.  tiles: FsStatus | the call's own status block | tile_pre[ntiles] | tile_cnt[ntiles]
struct FsIndex {
  FsStatus* d_st;
  void* d_own;  // the call's own status block, directly behind *d_st
  const u64* tile_pre;
  size_t ntiles;
  u64 lines;          // of the piece: a last line without '\n' is a line
  size_t nrec;        // complete records
  unsigned trailing;  // lines behind the last of them
  bool trail_ok;      // those are empty lines
};
#define FS_OWN_MAX 64  // bytes of a call's own status block, at most

// What a call that answers for a malformed record only at its end keeps over its pieces.  Pieces come in text order:
// the first failure found is that of the lowest record.
struct FsPieces {
  const char* what;
  size_t limit;  // records the caller's arrays hold
  size_t records = 0;
  int bad_rc = MK_OK;
  std::string bad_msg;
  // once a record has failed, or the text holds more records than the arrays, the pieces are only counted
  bool counting_only() const { return bad_rc != MK_OK || records > limit; }
  int fail(int rc, std::string msg) {
    bad_rc = rc;
    bad_msg = std::move(msg);
    return MK_OK;
  }
  // The records of an opened piece, counted; first: the index of the first of them.  False: the piece is done with.
  bool take(const FsIndex& ix, size_t& first) {
    first = records;
    records += ix.nrec;
    if (counting_only()) return false;
    if (!ix.nrec && !ix.trail_ok) fail(MK_ERR_UNSUPPORTED, fs_msg_incomplete(what, first, ix.trailing));
    return ix.nrec != 0;
  }
  // What the read-back of a piece says: `bad` of its status word (kind: the phrase of a check), then what trails.
  template <class Kind>
  bool failed(const FsIndex& ix, size_t first, u64 bad, Kind&& kind) {
    if (bad != FS_NONE) fail(MK_ERR_UNSUPPORTED, fs_msg_malformed(what, first + (size_t)(bad >> 3), kind((unsigned)(bad & 7))));
    else if (!ix.trail_ok) fail(MK_ERR_UNSUPPORTED, fs_msg_incomplete(what, first + ix.nrec, ix.trailing));
    return bad_rc != MK_OK;
  }
};

// The line index of a piece of n > 0 bytes at d_text (16-byte aligned), opened: the status blocks initialised (own:
// own_bytes initial bytes of the call's, a multiple of 8, or none), the newlines of every tile counted and scanned
// inside `index`, the total and the text's last bytes read back with one synchronisation.  The stream is idle afterwards.
static int fs_index_open(mk_ctx* c, MkDevBuf& tiles, MkTimed& index, double& s_index, const uint8_t* d_text, size_t n, const void* own,
                         size_t own_bytes, FsIndex& ix) {
  int rc;
  if (own_bytes > FS_OWN_MAX || (own_bytes & 7)) { c->err = "fs_index_open: the status block of a call (internal error)"; return MK_ERR_STATE; }
  ix.ntiles = div_up(n, FS_TILE);
  if ((rc = mk_buf_reserve(c, tiles, sizeof(FsStatus) + own_bytes + ix.ntiles * (sizeof(u64) + sizeof(unsigned)))) != MK_OK) return rc;
  ix.d_st = (FsStatus*)tiles.p;
  ix.d_own = ix.d_st + 1;
  u64* tile_pre = (u64*)((char*)ix.d_own + own_bytes);
  unsigned* tile_cnt = (unsigned*)(tile_pre + ix.ntiles);
  ix.tile_pre = tile_pre;
  struct { FsStatus s; unsigned char own[FS_OWN_MAX]; } h{};
  h.s.bad = FS_NONE;
  if (own_bytes) memcpy(h.own, own, own_bytes);
  MK_HIP(hipMemcpyAsync(ix.d_st, &h, sizeof(FsStatus) + own_bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = index.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fs_tiles_k, dim3((unsigned)ix.ntiles), dim3(256), 0, c->stream, d_text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fs_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ix.ntiles, tile_pre, ix.d_st);
  MK_HIP(hipGetLastError());
  if ((rc = index.end()) != MK_OK) return rc;
  uint8_t tail[4] = {0, 0, 0, 0};
  const size_t ntail = std::min<size_t>(n, 4);
  u64 newlines = 0;
  MK_HIP(hipMemcpyAsync(&newlines, &ix.d_st->newlines, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(tail + (4 - ntail), d_text + (n - ntail), ntail, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = index.add_to(s_index)) != MK_OK) return rc;
  ix.lines = newlines + (tail[3] != '\n' ? 1 : 0);
  ix.nrec = (size_t)(ix.lines / 4);
  ix.trailing = (unsigned)(ix.lines & 3);
  // what trails behind the last complete record: `trailing` empty lines are that many '\n' behind a '\n' (or the text's start)
  ix.trail_ok = true;
  for (unsigned i = 0; i < ix.trailing && ix.trail_ok; ++i) ix.trail_ok = tail[3 - i] == '\n';
  if (ix.trailing && ix.trail_ok && n > ix.trailing) ix.trail_ok = tail[3 - ix.trailing] == '\n';
  return MK_OK;
}

// line[0 .. 4 nrec] of an opened piece (nrec > 0), inside `index`; KEPT: with the check of the sequence lines' bytes.
// more(): what else the call launches in that section.
template <bool KEPT, class More>
static int fs_index_lines(mk_ctx* c, MkTimed& index, const uint8_t* d_text, size_t n, const FsIndex& ix, u64* line, More&& more) {
  int rc;
  const u64 nidx = 4 * (u64)ix.nrec;
  if ((rc = index.begin()) != MK_OK) return rc;
  const int end_is_n = ix.lines == nidx ? 1 : 0;  // (no line 4 nrec starts: the last record ends with the text)
  hipLaunchKernelGGL(fs_lines_k<KEPT>, dim3((unsigned)ix.ntiles), dim3(256), 0, c->stream, d_text, (u64)n, ix.tile_pre, nidx, end_is_n, line,
                     ix.d_st);
  more();
  MK_HIP(hipGetLastError());
  return index.end();
}
template <bool KEPT>
static int fs_index_lines(mk_ctx* c, MkTimed& index, const uint8_t* d_text, size_t n, const FsIndex& ix, u64* line) {
  return fs_index_lines<KEPT>(c, index, d_text, n, ix, line, []() {});
}

// The gather of a piece's piece_out bytes behind the bytes_out the call has so far: into the caller's device memory, or
// (device false) into `stage` and from there to the caller's host memory.  Without room the call goes on adding up and
// answers MK_ERR_RANGE at its end (fs_out_room).  The stream is idle afterwards.
static int fs_gather(mk_ctx* c, MkTimed& gather, MkDevBuf& stage, const uint8_t* d_text, size_t n, const u64* seg_src, const u64* dst,
                     size_t nseg, u64 piece_out, uint8_t* out, size_t out_cap, bool device, size_t& bytes_out, double& s_gather,
                     double& s_write) {
  int rc;
  const size_t at = bytes_out;
  bytes_out += (size_t)piece_out;
  if (!piece_out || bytes_out > out_cap) return MK_OK;
  uint8_t* d_out = out + at;
  if (!device) {
    if ((rc = mk_buf_reserve(c, stage, (size_t)piece_out)) != MK_OK) return rc;
    d_out = (uint8_t*)stage.p;
  }
  const u64 head = std::min<u64>((16 - ((uintptr_t)d_out & 15)) & 15, piece_out);
  const u64 nbody = (piece_out - head) / 16, tail_at = head + 16 * nbody;
  if ((rc = gather.begin()) != MK_OK) return rc;
  if (nbody)
    hipLaunchKernelGGL(fs_gather_k, dim3((unsigned)div_up((size_t)nbody, 256 * FS_CHUNKS)), dim3(256), 0, c->stream, d_text, (u64)n, seg_src,
                       dst, nseg, head, nbody, d_out);
  if (head || tail_at < piece_out)
    hipLaunchKernelGGL(fs_edges_k, dim3(1), dim3(64), 0, c->stream, d_text, (u64)n, seg_src, dst, nseg, head, tail_at, piece_out, d_out);
  MK_HIP(hipGetLastError());
  if ((rc = gather.end()) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = gather.add_to(s_gather)) != MK_OK) return rc;
  if (!device) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(out + at, d_out, (size_t)piece_out, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    s_write += mk_since(t1);
  }
  return MK_OK;
}

// The piece plan of a text call: the ends of the pieces of a host text of n > 0 bytes, ascending, the last n.  A piece
// ends behind a line 4j (paired: 8j, mates stay together) once it holds tl_piece_size bytes.
static int fs_piece_cuts(mk_ctx* c, const char* what, const uint8_t* fastq, size_t n, size_t piece_bytes, bool paired,
                         std::vector<uint64_t>& cuts) {
  const size_t piece = tl_piece_size(c, piece_bytes, n);
  cuts.assign(n / piece + 2, 0);
  size_t ncuts = 0;
  if ((paired ? mk_fastq_pair_cuts : mk_fastq_cuts)(fastq, n, piece, cuts.data(), cuts.size(), &ncuts) != MK_OK) {
    c->err = std::string(what) + ": the line scanner failed (internal error)";
    return MK_ERR_STATE;
  }
  cuts.resize(ncuts);
  cuts.push_back(n);
  return MK_OK;
}

// A piece of a host text in c->raw (16-byte aligned, 64 bytes of slack).  The stream is idle afterwards.
static int fs_upload_raw(mk_ctx* c, const uint8_t* src, size_t len, double& s_copy) {
  int rc = mk_buf_reserve(c, c->raw, len + 64);
  if (rc != MK_OK) return rc;
  const auto t1 = MkClock::now();
  MK_HIP(hipMemcpyAsync(c->raw.p, src, len, hipMemcpyHostToDevice, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  s_copy += mk_since(t1);
  return MK_OK;
}

// The text of a device call where the kernels can read it: where it stands, or copied to c->raw where it is not aligned to
// 16 (the line passes, the scans and fl_load16 load 16 aligned bytes at a time) or where the call wants a copy of its own.
static int fs_aligned_text(mk_ctx* c, const uint8_t* d_fastq, size_t n, bool own_copy, double& s_copy, const uint8_t** d_text) {
  *d_text = d_fastq;
  if (!((uintptr_t)d_fastq & 15) && !own_copy) return MK_OK;
  int rc = mk_buf_reserve(c, c->raw, n + 64);
  if (rc != MK_OK) return rc;
  const auto t1 = MkClock::now();
  MK_HIP(hipMemcpyAsync(c->raw.p, d_fastq, n, hipMemcpyDeviceToDevice, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  s_copy += mk_since(t1);
  *d_text = (const uint8_t*)c->raw.p;
  return MK_OK;
}

// How a call opens: a spoiled context and an open chunk are refused, then the call's own arguments (args()), then the
// device is set and the stream idle for body(), and idle again behind it.
template <class Args, class Body>
static int fs_call(mk_ctx* c, const char* what, Args&& args, Body&& body) {
  MK_REFUSE_SPOILED(c, what);
  if (c->in_chunk) { c->err = std::string(what) + ": a chunk is open"; return MK_ERR_STATE; }
  int rc;
  if ((rc = args()) != MK_OK) return rc;
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipStreamSynchronize(c->stream));
  rc = body();
  (void)hipStreamSynchronize(c->stream);
  return rc;
}
// How it ends once its own check of the record count has passed: an odd count of paired records, then the lowest
// malformed record (the order the rule modules of the tests state).
static int fs_call_end(mk_ctx* c, const char* what, size_t records, bool paired, int bad_rc, const std::string& bad_msg) {
  if (paired && (records & 1)) {
    c->err = std::string(what) + ": paired, but the text holds an odd number of records (" + std::to_string(records) + ")";
    return MK_ERR_RANGE;
  }
  if (bad_rc != MK_OK) c->err = bad_msg;
  return bad_rc;
}
static int fs_out_room(mk_ctx* c, const char* what, size_t bytes_out, size_t out_cap) {
  if (bytes_out <= out_cap) return MK_OK;
  c->err = std::string(what) + ": the output holds " + std::to_string(bytes_out) + " bytes, out has room for " + std::to_string(out_cap);
  return MK_ERR_RANGE;
}
