// mk_tsvload.hip -- count TSVs read back into a running table: the inverse of mk_tsv.hip.
//
// A "<k key bytes>\t<decimal count>\n" table (the tsv_<type>/<sample>_counts.tsv files mk_write_tsv writes, or a
// header-less Jellyfish / KMC dump) is insert-added into the context's running table, the same sum run_mercat2 does
// over chunk results (bin/mercat2.py:121-127).  The text goes to the device in pieces cut at line ends; per piece:
//   1. line starts: newlines counted per 4 KiB tile, the tile counts scanned, every line's start written at its rank
//      (count -> scan -> emit, the shape of mk_fparse.hip; no look-back, no waiting between workgroups);
//   2. one line per lane: the row is validated, its key classified against the context's alphabet and packed into the
//      layout mk_import_pairs_device takes, its count converted; rows with a byte outside the alphabet (and every row of a
//      by-reference context) are appended to the buffers of the by-reference import;
//   3. once the host has seen that the WHOLE piece is well formed: mk_launch_import_pairs / mk_launch_import_ref.
// The host reads (or copies) piece p+1 into the other half of a pinned double buffer and a second stream copies it to
// the device while the kernels of piece p run.
#include "mk_tsvpieces.h"
#include <rocprim/device/device_scan.hpp>
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

// ---------------------------------------------------------------------------------------- line starts
// The 16 bytes of this lane (zero beyond the end of the text: neither a newline nor >= 0x80).
__device__ __forceinline__ void tl_load16(const uint8_t* __restrict__ text, size_t n, size_t pos, unsigned w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0;
  if (pos + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + pos);  // (the text starts a device allocation; pos is a multiple of 16)
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
    for (size_t j = pos; j < n; ++j) w[(j - pos) >> 2] |= (unsigned)text[j] << (8 * ((j - pos) & 3));
  }
}
// 0x80 in every byte of w that equals '\n'
__device__ __forceinline__ unsigned tl_newlines(unsigned w) {
  const unsigned x = w ^ 0x0A0A0A0Au;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

__global__ void __launch_bounds__(256) tl_count_k(const uint8_t* __restrict__ text, size_t n, unsigned* __restrict__ tile_nl,
                                                  TlStatus* __restrict__ st) {
  __shared__ unsigned s_wave[4];
  const size_t pos = (size_t)blockIdx.x * TL_TILE + (size_t)threadIdx.x * 16;
  unsigned w[4];
  tl_load16(text, n, pos, w);
  unsigned nl = 0;
  for (int q = 0; q < 4; ++q) {
    nl += __popc(tl_newlines(w[q]));
    const unsigned high = w[q] & 0x80808080u;
    if (high) atomicMin(&st->bad_byte, (u64)(pos + 4 * q + ((__ffs(high) - 1) >> 3)));  // (rare: the file is refused)
  }
  nl = mk_wave_sum(nl);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = nl;
  __syncthreads();
  if (threadIdx.x == 0) tile_nl[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// line_start[r] = offset of the first byte of line r, for r <= cap (line_start[lines] = n: every line of a piece ends
// in '\n').  tile_off = exclusive scan of tile_nl over ntiles + 1 elements: tile_off[ntiles] = lines.
__global__ void __launch_bounds__(256) tl_emit_k(const uint8_t* __restrict__ text, size_t n, const unsigned* __restrict__ tile_off,
                                                 unsigned ntiles, unsigned* __restrict__ line_start, unsigned cap,
                                                 TlStatus* __restrict__ st) {
  __shared__ unsigned s_wave[4];
  const size_t pos = (size_t)blockIdx.x * TL_TILE + (size_t)threadIdx.x * 16;
  unsigned w[4], marks[4], mine = 0;
  tl_load16(text, n, pos, w);
  for (int q = 0; q < 4; ++q) { marks[q] = tl_newlines(w[q]); mine += __popc(marks[q]); }
  const unsigned incl = mk_wave_scan_incl(mine);
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned rank = tile_off[blockIdx.x] + incl - mine;
  for (unsigned v = 0; v < (threadIdx.x >> 6); ++v) rank += s_wave[v];
  for (int q = 0; q < 4; ++q)
    for (unsigned m = marks[q]; m; m &= m - 1) {
      const unsigned byte = (unsigned)(__ffs(m) - 1) >> 3;
      ++rank;  // the line AFTER this newline
      if (rank <= cap) line_start[rank] = (unsigned)(pos + 4 * q + byte + 1);
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    line_start[0] = 0;
    st->lines = tile_off[ntiles];
  }
}

// ---------------------------------------------------------------------------------------------- rows
// One line per lane.  A data row is exactly k key bytes (any byte but '\n'; a '\t' too: the reference counts text with
// tabs in it, and its tables must load), '\t', 1..20 decimal digits whose value fits 64 bits, '\n'.  Only the first min(lines, cap) lines are looked at: cap = piece bytes / (k + 3) + 1 well
// formed rows do not fit the piece, so with more lines than that one of the first cap is malformed and is found.
// Rows are appended in no particular order (the tables sum; the export sorts): a workgroup claims its rows' places with
// one add per list.
template <int KEYS>
__global__ void __launch_bounds__(256) tl_parse_k(const uint8_t* __restrict__ text, const unsigned* __restrict__ line_start,
                                                  unsigned cap, int k, int bits, u64* __restrict__ pk_keys,
                                                  u64* __restrict__ pk_cnts, uint8_t* __restrict__ tx_keys,
                                                  u64* __restrict__ tx_cnts, TlStatus* __restrict__ st) {
  __shared__ unsigned s_np, s_nt;
  __shared__ u64 s_bp, s_bt;
  const u64 lines = st->lines;
  const unsigned nl = lines < (u64)cap ? (unsigned)lines : cap;
  u64 zeros = 0;
  for (unsigned base = blockIdx.x * 256u; base < nl; base += gridDim.x * 256u) {  // (the same trips for every lane of a workgroup)
    if (threadIdx.x == 0) { s_np = 0; s_nt = 0; }
    __syncthreads();
    const unsigned i = base + threadIdx.x;
    int kind = 0;  // 0: nothing to append, 1: packed row, 2: text row
    unsigned my = 0, s = 0;
    u64 a = 0, b = 0, cnt = 0;
    if (i < nl) {
      s = line_start[i];
      const unsigned len = line_start[i + 1] - 1 - s;  // without the '\n'
      bool ok = len >= (unsigned)k + 2 && len <= (unsigned)k + 21 && text[s + k] == '\t';
      bool in_alphabet = false;
      if (ok) {
        in_alphabet = tl_pack_key<KEYS>(text + s, k, bits, a, b);
        ok = tl_count_field(text + s + k + 1, len - (unsigned)k - 1, cnt);
      }
      if (!ok) atomicMin(&st->bad_line, (u64)i);  // (rare: the file is refused)
      else if (cnt == 0) ++zeros;
      else kind = in_alphabet ? 1 : 2;
    }
    if (kind == 1) my = atomicAdd(&s_np, 1u);
    if (kind == 2) my = atomicAdd(&s_nt, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
      s_bp = s_np ? atomicAdd(&st->packed, (u64)s_np) : 0;
      s_bt = s_nt ? atomicAdd(&st->text, (u64)s_nt) : 0;
    }
    __syncthreads();
    if (kind == 1) {
      const u64 at = s_bp + my;  // (< cap: every appended row is a well formed line of the piece)
      if (KEYS == TL_ONE_WORD) pk_keys[at] = a;
      else { pk_keys[2 * at] = a; pk_keys[2 * at + 1] = b; }
      pk_cnts[at] = cnt;
    } else if (kind == 2) {
      const u64 at = s_bt + my;
      for (int j = 0; j < k; ++j) tx_keys[at * (u64)k + j] = text[s + j];
      tx_cnts[at] = cnt;
    }
    __syncthreads();  // (s_np / s_nt are cleared at the top of the next trip)
  }
  block_add(&st->zero, zeros);
}

// The by-reference import takes rows that are distinct among themselves (mk_import_ref_k); a file may list a key twice.
// Text rows of one piece with the same k bytes are folded into the first of them to claim a slot of a scratch table
// (slot = row index): its count takes the others', theirs become 0, which the import skips.
__global__ void tl_fold_text_k(const uint8_t* __restrict__ keys, u64* __restrict__ cnts, unsigned rows, int k,
                               unsigned* __restrict__ slots, unsigned mask) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x) {
    const uint8_t* mine = keys + (size_t)i * k;
    u64 h = 0;
    for (int j = 0; j < k; ++j) h = h * MK_POLY_B + mine[j];
    unsigned slot = (unsigned)mk_mix64(h) & mask;
    for (;;) {  // (the table has at least twice as many slots as there are rows: a free one is met)
      unsigned cur = __hip_atomic_load(&slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == TL_NONE) cur = atomicCAS(&slots[slot], TL_NONE, i);
      if (cur == TL_NONE) break;  // this row stands for its key
      const uint8_t* other = keys + (size_t)cur * k;
      bool same = true;
      for (int j = 0; j < k && same; ++j) same = other[j] == mine[j];
      if (same) {
        atomicAdd(&cnts[cur], cnts[i]);  // (nobody adds to a row that lost its slot: cnts[i] is this lane's alone)
        cnts[i] = 0;
        break;
      }
      slot = (slot + 1) & mask;
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
typedef std::chrono::steady_clock TlClk;
static double tl_since(TlClk::time_point t0) { return std::chrono::duration<double>(TlClk::now() - t0).count(); }

// Is [p, p + n) (a line without its '\n') a data row?  k >= 0: of exactly k key bytes; k < 0: with a key of any length
// >= 1 that ends at the line's LAST tab (a key may hold tabs, a count cannot; *key_len receives the length).
// count_optional (k >= 0): the k key bytes alone are a row too.  why: what is wrong with it, for the message.
static bool tl_row_ok(const uint8_t* p, size_t n, long k, size_t* key_len, const char** why, bool count_optional = false) {
  const char* dummy;
  if (!why) why = &dummy;
  if (!n) { *why = "empty line"; return false; }
  if (count_optional && k >= 0 && n == (size_t)k) return true;
  const uint8_t* tab = (const uint8_t*)memrchr(p, '\t', n);
  if (!tab) { *why = count_optional ? "the key is not k bytes long" : "no tab"; return false; }
  const size_t kl = k >= 0 ? (size_t)k : (size_t)(tab - p);
  if (key_len) *key_len = kl;
  if (kl < 1 || n < kl + 1 || p[kl] != '\t') { *why = "the key is not k bytes long"; return false; }
  const size_t nd = n - kl - 1;
  if (nd < 1) { *why = "empty count"; return false; }
  u64 v = 0;
  for (size_t j = kl + 1; j < n; ++j) {
    const unsigned d = (unsigned)p[j] - '0';
    if (d > 9u) {
      *why = p[j] == '\r' ? "carriage return (lines end in '\\n' only)" : p[j] == '\t' ? "the key is not k bytes long" : "the count is not a decimal number";
      return false;
    }
    if (nd > 20 || v > (~0ull - d) / 10ull) { *why = "the count does not fit 64 bits"; return false; }
    v = v * 10ull + d;
  }
  return true;
}

// second field of a header line
static std::string tl_second_field(const uint8_t* p, size_t n) {
  const uint8_t* tab = (const uint8_t*)memchr(p, '\t', n);
  if (!tab) return std::string();
  const uint8_t* from = tab + 1;
  const uint8_t* end = (const uint8_t*)memchr(from, '\t', (size_t)(p + n - from));
  return std::string((const char*)from, (size_t)((end ? end : p + n) - from));
}

ssize_t TlSource::read(uint8_t* dst, size_t want) {
  if (fd < 0) {
    const size_t m = std::min(want, n - at);
    if (m) memcpy(dst, mem + at, m);
    at += m;
    return (ssize_t)m;
  }
  size_t got = 0;
  while (got < want) {
    const ssize_t r = ::read(fd, dst + got, want - got);
    if (r < 0) return -1;
    if (r == 0) break;
    got += (size_t)r;
  }
  return (ssize_t)got;
}

int tl_open(mk_ctx* c, const char* what, const char* path, TlSource* src, size_t* hint) {
  src->fd = ::open(path, O_RDONLY | O_CLOEXEC);
  if (src->fd < 0) { c->err = std::string(what) + ": " + path + ": " + strerror(errno); return MK_ERR_IO; }
  struct stat sb;
  *hint = (fstat(src->fd, &sb) == 0 && sb.st_size > 0) ? (size_t)sb.st_size : 0;
  return MK_OK;
}

// ---- the pieces of a text (mk_tsvpieces.h)
TlPieces::~TlPieces() {
  (void)hipSetDevice(c->device);
  if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
  (void)hipStreamSynchronize(c->stream);
  for (auto e : ev_copy) if (e) (void)hipEventDestroy(e);
  for (auto e : ev) if (e) (void)hipEventDestroy(e);
  if (pinned) (void)hipHostFree(pinned);
  MkDevBuf* all[] = {&dtext[0], &dtext[1], &tiles, &lines, &scan_tmp, &status};
  for (auto* b : all) buf_free(*b);
  for (auto& b : held) buf_free(b);
  if (src.fd >= 0) ::close(src.fd);
}

int TlPieces::fail(int code, const std::string& msg) {
  c->err = std::string(what) + ": " + msg;
  return code;
}

int TlPieces::setup(size_t piece_bytes, size_t total_hint) {
  const size_t k = (size_t)c->k;
  piece = tl_piece_size(c, piece_bytes, total_hint);
  if (2 * (k + 24) > TL_MAX_PIECE) return fail(MK_ERR_ARG, "k is too large for a table in text form");
  cap_rows = (piece + 64) / min_row() + 2;  // (a last line without its '\n' gets one: a piece may be one byte longer)
  MK_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
  for (auto& e : ev_copy) MK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : ev) MK_HIP(hipEventCreate(&e));
  const size_t half = (piece + 64 + 255) & ~(size_t)255;
  MK_HIP(hipHostMalloc((void**)&pinned, 2 * half + sizeof(TlSnap), hipHostMallocDefault));
  hbuf[0] = pinned;
  hbuf[1] = pinned + half;
  snap = (TlSnap*)(pinned + 2 * half);
  max_tiles = div_up(piece + 64, TL_TILE) + 1;
  int rc;
  for (auto& d : dtext)
    if ((rc = mk_buf_reserve(c, d, half)) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, tiles, 2 * max_tiles * sizeof(unsigned))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, lines, (cap_rows + 1) * sizeof(unsigned))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, status, sizeof(TlStatus))) != MK_OK) return rc;
  if ((rc = reserve()) != MK_OK) return rc;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, scan_tmp_bytes, (const unsigned*)nullptr, (unsigned*)nullptr, 0u, max_tiles,
                                 rocprim::plus<unsigned>(), c->stream));
  return mk_buf_reserve(c, scan_tmp, scan_tmp_bytes ? scan_tmp_bytes : 16);
}

// Read the next piece into half b: the carried bytes, then the source up to the piece size; cut at the last '\n'.
// On piece 0 the header line (line 1, if it is not a data row) is taken off.  Returns > 0 when there was nothing left.
int TlPieces::fill(int b) {
  const auto t0 = TlClk::now();
  if (copy_used[b]) MK_HIP(hipEventSynchronize(ev_copy[b]));  // (the copy that last read this half)
  uint8_t* h = hbuf[b];
  size_t have = carry.size();
  if (have) memcpy(h, carry.data(), have);
  carry.clear();
  if (!eof) {
    const ssize_t got = src.read(h + have, piece - have);
    if (got < 0) return fail(MK_ERR_IO, std::string("read: ") + strerror(errno));
    eof = (size_t)got < piece - have;
    have += (size_t)got;
    bytes += (u64)got;
  }
  s_read += tl_since(t0);
  if (!have) return 1;
  size_t plen;
  if (eof) {
    if (h[have - 1] != '\n') h[have++] = '\n';  // (the last line may lack it; the buffer has the room)
    plen = have;
  } else {
    size_t cut = have;
    while (cut && h[cut - 1] != '\n') --cut;  // (a row is short: a few bytes are looked at)
    if (!cut || have - cut > (size_t)c->k + 22) {  // (the lines of the piece in flight are not counted yet: run() names the line)
      long_line_at = (u64)std::count(h, h + cut, (uint8_t)'\n');
      return 2;
    }
    carry.assign(h + cut, h + have);
    plen = cut;
  }
  skip[b] = 0;
  if (pieces == 0) {
    const uint8_t* nl = (const uint8_t*)memchr(h, '\n', plen);
    const size_t l1 = (size_t)(nl - h);
    if (!tl_row_ok(h, l1, c->k, nullptr, nullptr, count_optional)) {
      header = 1;
      column = tl_second_field(h, l1);
      skip[b] = l1 + 1;
      lines_seen = 1;
    }
  }
  len[b] = plen - skip[b];
  ++pieces;
  return MK_OK;
}

int TlPieces::enqueue_copy(int b) {
  if (!len[b]) return MK_OK;
  MK_HIP(hipMemcpyAsync(dtext[b].p, hbuf[b] + skip[b], len[b], hipMemcpyHostToDevice, copy_stream));
  MK_HIP(hipEventRecord(ev_copy[b], copy_stream));
  copy_used[b] = true;
  return MK_OK;
}

int TlPieces::enqueue_parse(int b) {
  const size_t n = len[b];
  TlStatus* st = (TlStatus*)status.p;
  MK_HIP(hipMemsetAsync(st, 0xFF, 16, c->stream));
  MK_HIP(hipMemsetAsync((char*)st + 16, 0, sizeof(TlStatus) - 16, c->stream));
  if (n) {
    const unsigned ntiles = (unsigned)div_up(n, TL_TILE);
    const unsigned cap = (unsigned)(n / min_row() + 1);  // <= cap_rows
    unsigned* tile_nl = (unsigned*)tiles.p;
    unsigned* tile_off = tile_nl + max_tiles;
    const uint8_t* text = (const uint8_t*)dtext[b].p;
    MK_HIP(hipStreamWaitEvent(c->stream, ev_copy[b], 0));
    MK_HIP(hipEventRecord(ev[0], c->stream));
    MK_HIP(hipMemsetAsync(tile_nl + ntiles, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(tl_count_k, dim3(ntiles), dim3(256), 0, c->stream, text, n, tile_nl, st);
    MK_HIP(rocprim::exclusive_scan(scan_tmp.p, scan_tmp_bytes, (const unsigned*)tile_nl, tile_off, 0u, (size_t)ntiles + 1,
                                   rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(tl_emit_k, dim3(ntiles), dim3(256), 0, c->stream, text, n, (const unsigned*)tile_off, ntiles,
                       (unsigned*)lines.p, cap, st);
    const int rc = enqueue_rows(b, text, (const unsigned*)lines.p, cap, st);
    if (rc != MK_OK) return rc;
    MK_HIP(hipGetLastError());
    MK_HIP(hipEventRecord(ev[1], c->stream));
  }
  MK_HIP(hipMemcpyAsync(&snap->st, st, sizeof(TlStatus), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&snap->info, c->info.p, sizeof(MkChunkInfo), hipMemcpyDeviceToHost, c->stream));
  return MK_OK;
}

// 1-based number, in the whole text, of line `index` of the piece in half b, and the line itself
void TlPieces::locate(int b, u64 index, const uint8_t** p, size_t* n) const {
  const uint8_t* at = hbuf[b] + skip[b];
  const uint8_t* end = at + len[b];
  for (u64 i = 0; i < index && at < end; ++i) at = (const uint8_t*)memchr(at, '\n', (size_t)(end - at)) + 1;
  const uint8_t* nl = at < end ? (const uint8_t*)memchr(at, '\n', (size_t)(end - at)) : nullptr;
  *p = at;
  *n = nl ? (size_t)(nl - at) : 0;
}

void TlPieces::add_elapsed(double& to, hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) == hipSuccess) to += ms * 1e-3;
}

// Wait for the piece in half b, refuse it or hand its rows on.
int TlPieces::finish(int b) {
  MK_HIP(hipStreamSynchronize(c->stream));
  if (len[b]) add_elapsed(s_parse, ev[0], ev[1]);
  const TlStatus st = snap->st;
  const MkChunkInfo before = snap->info;
  const u64 none = ~0ull;
  u64 ascii_line = none;
  if (st.bad_byte != none)
    ascii_line = (u64)std::count(hbuf[b] + skip[b], hbuf[b] + skip[b] + st.bad_byte, (uint8_t)'\n');
  if (ascii_line != none && ascii_line <= st.bad_line)
    return fail(MK_ERR_NON_ASCII, "line " + std::to_string(lines_seen + ascii_line + 1) + ": byte >= 0x80 (only ASCII keys are counted)");
  if (st.bad_line != none) {
    const uint8_t* p;
    size_t n;
    const char* why = "malformed row";
    locate(b, st.bad_line, &p, &n);
    (void)tl_row_ok(p, n, c->k, nullptr, &why, count_optional);
    return fail(MK_ERR_RANGE, "line " + std::to_string(lines_seen + st.bad_line + 1) + ": " + why + " (a row is " +
                                  std::to_string(c->k) + (count_optional ? " key bytes, then nothing or a tab and a decimal count)"
                                                                         : " key bytes, a tab, a decimal count)"));
  }
  const int rc = accept(b, st, before);
  if (rc == MK_OK) lines_seen += st.lines;
  return rc;
}

int TlPieces::too_long() {
  return fail(MK_ERR_RANGE, "line " + std::to_string(lines_seen + long_line_at + 1) + ": longer than a data row of this k");
}

int TlPieces::run() {
  int rc, cur = 0;
  if ((rc = fill(0)) < 0) return rc;
  if (rc == 2) return too_long();
  if (rc > 0) return MK_OK;  // an empty text: no lines
  if ((rc = enqueue_copy(0)) != MK_OK || (rc = enqueue_parse(0)) != MK_OK) return rc;
  for (;;) {
    const int nxt = cur ^ 1;
    rc = (eof && carry.empty()) ? 1 : fill(nxt);  // (the host reads while the device parses)
    if (rc < 0) return rc;
    if (rc == 2) return (rc = finish(cur)) != MK_OK ? rc : too_long();  // (a refusal in the piece before comes first)
    const bool more = rc == 0;
    if (more && (rc = enqueue_copy(nxt)) != MK_OK) return rc;  // ... and the copy runs beside the kernels
    if ((rc = finish(cur)) != MK_OK) return rc;
    if (!more) return MK_OK;
    if ((rc = enqueue_parse(nxt)) != MK_OK) return rc;
    cur = nxt;
  }
}

// ---- the loader: a piece's rows are parsed into lists and, once the whole piece is known to be well formed, imported
struct TlLoad : TlPieces {
  mk_tsv_load_t out{};
  int words = 1, keys = TL_TEXT_ONLY;
  MkDevBuf &pk_keys = hold(), &pk_cnts = hold(), &tx_keys = hold(), &tx_cnts = hold(), &fold = hold();
  bool import_timed = false;
  bool imported = false;       // the running table holds rows of this call
  TlLoad(mk_ctx* c_, TlSource src_) : TlPieces(c_, src_, "mk_load_tsv", false) {}

  int reserve() override {
    const size_t k = (size_t)c->k;
    keys = tl_keys_of(c);
    words = c->mode == MK_MODE_HASH128 ? 2 : 1;
    int rc;
    if (keys != TL_TEXT_ONLY) {
      if ((rc = mk_buf_reserve(c, pk_keys, cap_rows * 8 * (size_t)words)) != MK_OK) return rc;
      if ((rc = mk_buf_reserve(c, pk_cnts, cap_rows * 8)) != MK_OK) return rc;
    }
    if ((rc = mk_buf_reserve(c, tx_keys, cap_rows * k + 64)) != MK_OK) return rc;
    return mk_buf_reserve(c, tx_cnts, cap_rows * 8);
  }

  int enqueue_rows(int, const uint8_t* text, const unsigned* line_start, unsigned cap, TlStatus* st) override {
    const unsigned grid = grid_for(cap, 256, 8192);
#define TL_PARSE(K) hipLaunchKernelGGL((tl_parse_k<K>), dim3(grid), dim3(256), 0, c->stream, text, line_start, cap, c->k, \
                                       c->bits, (u64*)pk_keys.p, (u64*)pk_cnts.p, (uint8_t*)tx_keys.p, (u64*)tx_cnts.p, st)
    if (keys == TL_ONE_WORD) TL_PARSE(TL_ONE_WORD);
    else if (keys == TL_TWO_WORD_NT) TL_PARSE(TL_TWO_WORD_NT);
    else if (keys == TL_TWO_WORD_AA) TL_PARSE(TL_TWO_WORD_AA);
    else TL_PARSE(TL_TEXT_ONLY);
#undef TL_PARSE
    return MK_OK;
  }

  // Hand the rows of a well formed piece to the import kernels.
  int accept(int, const TlStatus& st, const MkChunkInfo& before) override {
    if (import_timed) { add_elapsed(out.s_import, ev[2], ev[3]); import_timed = false; }
    if (st.lines != st.packed + st.text + st.zero)
      return fail(MK_ERR_STATE, "the parse kernels lost rows (" + std::to_string(st.lines) + " lines, " +
                                    std::to_string(st.packed + st.text + st.zero) + " rows)");
    out.rows += st.lines;
    out.packed_rows += st.packed;
    out.text_rows += st.text;
    out.zero_rows += st.zero;
    if (!st.packed && !st.text) return MK_OK;
    // rows the tables hold now: what the host knew at the start + what the imports of the pieces before added
    int rc = MK_OK;
    MK_HIP(hipEventRecord(ev[2], c->stream));
    if (st.packed) {
      if (c->mode == MK_MODE_HASH64) rc = mk_grow_run64(c, c->run_rows + (size_t)before.new_rows + (size_t)st.packed);
      else if (c->mode == MK_MODE_HASH128) rc = mk_grow_run128(c, c->run128_rows + (size_t)before.new_rows + (size_t)st.packed);
      if (rc) return rc;
      imported = true;
      if ((rc = mk_launch_import_pairs(c, (const uint64_t*)pk_keys.p, (const uint64_t*)pk_cnts.p, (size_t)st.packed)) != MK_OK) return rc;
    }
    if (st.text) {
      if ((rc = mk_grow_run_ref(c, c->run_ref_rows + (size_t)before.new_rows_ref + (size_t)st.text)) != MK_OK) return rc;
      if (st.text > 1) {
        const size_t slots = pow2_at_least(2 * (size_t)st.text);
        if ((rc = mk_buf_reserve(c, fold, slots * sizeof(unsigned))) != MK_OK) return rc;
        MK_HIP(hipMemsetAsync(fold.p, 0xFF, slots * sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(tl_fold_text_k, dim3(grid_for((size_t)st.text, 256, 4096)), dim3(256), 0, c->stream,
                           (const uint8_t*)tx_keys.p, (u64*)tx_cnts.p, (unsigned)st.text, c->k, (unsigned*)fold.p, (unsigned)(slots - 1));
        MK_HIP(hipGetLastError());
      }
      imported = true;
      // (the arena rows of this launch start at run_ref_rows + the counter the launches before left in info.new_rows_ref:
      // run_ref_rows itself stays as it is until the end of the call)
      if ((rc = mk_launch_import_ref(c, (const uint8_t*)tx_keys.p, (const uint64_t*)tx_cnts.p, (size_t)st.text)) != MK_OK) return rc;
    }
    MK_HIP(hipEventRecord(ev[3], c->stream));
    import_timed = true;
    return MK_OK;
  }

  // the counters of the imports -> the host's row totals (once, at the end of the call)
  int fold_rows() {
    const size_t side_before = c->run_side ? 1 : 0;
    int rc = mk_pull_info(c);
    if (rc) return rc;
    if (import_timed) { add_elapsed(out.s_import, ev[2], ev[3]); import_timed = false; }
    mk_add_packed_rows(c, (size_t)c->h_info->new_rows);
    c->run_ref_rows += (size_t)c->h_info->new_rows_ref;
    if (c->mode == MK_MODE_HASH64) c->run_side += c->h_info->side;
    out.new_rows += c->h_info->new_rows + c->h_info->new_rows_ref + ((c->run_side ? 1 : 0) - side_before);
    return MK_OK;
  }

  int load(size_t piece_bytes, size_t total_hint) {
    int rc = setup(piece_bytes, total_hint);
    if (rc != MK_OK) return rc;
    MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
    return run();
  }
};

static int tl_load(mk_ctx* c, TlSource src, size_t total_hint, size_t piece_bytes, char* column, size_t column_cap, mk_tsv_load_t* st) {
  const auto t0 = TlClk::now();
  TlLoad L{c, src};  // (owns the file from here on)
  MK_REFUSE_SPOILED(c, "mk_load_tsv");
  if (c->in_chunk) { c->err = "mk_load_tsv: a chunk is open"; return MK_ERR_STATE; }
  MK_HIP(hipSetDevice(c->device));
  MK_SETTLE(c);
  size_t dense_before = 0, dense_after = 0;
  int rc;
  if (c->mode == MK_MODE_DENSE && (rc = mk_export_size(c, &dense_before)) != MK_OK) return rc;
  rc = L.load(piece_bytes, total_hint);
  if (rc == MK_OK && column_cap && L.column.size() + 1 > column_cap && !L.imported)
    rc = L.fail(MK_ERR_RANGE, "the column name needs " + std::to_string(L.column.size() + 1) + " bytes");
  const std::string msg = c->err;
  if (L.imported) {
    // rows of this call are in the table: the host's totals follow them, whatever came afterwards
    const int rf = L.fold_rows();
    if (rc != MK_OK || rf != MK_OK) {
      c->spoiled = true;  // part of the text is in the table: every call is refused until mk_reset
      if (rc != MK_OK) c->err = msg + "; the rows of the pieces before are in the table: mk_reset";
      return rc != MK_OK ? rc : rf;
    }
  } else {
    (void)hipStreamSynchronize(c->stream);
  }
  if (rc != MK_OK) return rc;
  if (c->mode == MK_MODE_DENSE) {
    if ((rc = mk_export_size(c, &dense_after)) != MK_OK) return rc;
    L.out.new_rows = dense_after - dense_before;
  }
  if (column && column_cap) {
    const size_t m = std::min(L.column.size(), column_cap - 1);
    memcpy(column, L.column.data(), m);
    column[m] = 0;
  }
  L.out.bytes = L.bytes;
  L.out.header = L.header;
  L.out.s_read = L.s_read;
  L.out.s_parse = L.s_parse;
  L.out.lines = L.lines_seen;
  L.out.pieces = L.pieces;
  L.out.s_total = tl_since(t0);
  if (st) *st = L.out;
  return MK_OK;
}

extern "C" int mk_load_tsv_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, char* column, size_t column_cap,
                                mk_tsv_load_t* st) {
  if (!c) return MK_ERR_ARG;
  if (n && !text) { c->err = "mk_load_tsv_text: text is NULL"; return MK_ERR_ARG; }
  TlSource src;
  src.mem = text;
  src.n = n;
  return tl_load(c, src, n, piece_bytes, column, column_cap, st);
}

extern "C" int mk_load_tsv(mk_ctx* c, const char* path, size_t piece_bytes, char* column, size_t column_cap, mk_tsv_load_t* st) {
  if (!c) return MK_ERR_ARG;
  if (!path) { c->err = "mk_load_tsv: path is NULL"; return MK_ERR_ARG; }
  TlSource src;
  size_t hint = 0;
  const int rc = tl_open(c, "mk_load_tsv", path, &src, &hint);
  if (rc != MK_OK) return rc;
  return tl_load(c, src, hint, piece_bytes, column, column_cap, st);
}

// Host helper, no GPU: what a table in text form looks like, from its first rows.
extern "C" int mk_tsv_shape(const char* path, int* k, int* header, int* alphabet_hint, char* column, size_t column_cap) {
  if (!path) { mk_set_global_error("mk_tsv_shape: path is NULL"); return MK_ERR_ARG; }
  const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) { mk_set_global_error(std::string("mk_tsv_shape: ") + path + ": " + strerror(errno)); return MK_ERR_IO; }
  std::vector<uint8_t> buf((size_t)4 << 20);
  TlSource src;
  src.fd = fd;
  const ssize_t got = src.read(buf.data(), buf.size());
  ::close(fd);
  if (got < 0) { mk_set_global_error(std::string("mk_tsv_shape: ") + path + ": read failed"); return MK_ERR_IO; }
  const bool whole = (size_t)got < buf.size();
  const uint8_t *p = buf.data(), *end = p + got;
  int kk = 0, head = 0, rows = 0;
  bool nt = true, aa = true;
  std::string col;
  for (int line = 0; p < end && rows < 4096; ++line) {
    const uint8_t* nl = (const uint8_t*)memchr(p, '\n', (size_t)(end - p));
    if (!nl && !whole) break;  // (a line the buffer cuts)
    const size_t n = (size_t)((nl ? nl : end) - p);
    size_t kl = 0;
    if (line == 0 && !tl_row_ok(p, n, -1, &kl, nullptr)) {
      head = 1;
      col = tl_second_field(p, n);
    } else {
      const uint8_t* tab = (const uint8_t*)memrchr(p, '\t', n);
      kl = tab ? (size_t)(tab - p) : n;
      if (!rows) kk = (int)kl;
      for (size_t j = 0; j < kl; ++j) {
        const uint8_t ch = p[j];
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') nt = false;
        if (ch < 'A' || ch > 'Z') aa = false;
      }
      ++rows;
    }
    p = nl ? nl + 1 : end;
  }
  if (k) *k = kk;
  if (header) *header = head;
  if (alphabet_hint) *alphabet_hint = !rows ? MK_ALPHABET_RAW : nt ? MK_ALPHABET_NT2 : aa ? MK_ALPHABET_AA5 : MK_ALPHABET_RAW;
  if (column && column_cap) {
    if (col.size() + 1 > column_cap) { mk_set_global_error("mk_tsv_shape: the column name does not fit"); return MK_ERR_RANGE; }
    memcpy(column, col.c_str(), col.size() + 1);
  }
  return MK_OK;
}
