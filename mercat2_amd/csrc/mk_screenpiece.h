// mk_screenpiece.h -- what the calls share that read a text record by record against the tables: mk_screen_*
// (mk_screen.hip) reports the rows, mk_filter_* (mk_filter.hip) goes on from them to the records' bytes, mk_track_*
// (mk_track.hip) to the count under every window, mk_trim_* (mk_trim.hip) to the records cut at their first low one,
// mk_norm_* (mk_norm.hip) to the records thinned by the median of those counts, mk_correct_* (mk_correct.hip) to the
// records with their isolated substitutions put right.
// One opening (sc_run), one way of cutting a host text into pieces
// (sc_text_pieces), one piece routine (sc_piece: parse, record scan, probe -- its kernels and launches live in
// mk_screen.hip), the tile's sizes (SC_RUN, SC_SPAN, sc_span_bytes) and the one-workgroup scan that turns tile counts
// into tile prefixes (sc_tile_scan).  The lane walk over a tile is mk_screenwalk.h.
#pragma once
#include "mk_tsvpieces.h"
#include "mk_device.h"
#include <algorithm>
#include <vector>

#define SC_RUN 32                // window starts a lane owns
#define SC_SPAN (256 * SC_RUN)   // ... a workgroup: one tile of the record scan
// Home-slot loads of the one-word table a lane has in flight before it compares any: the lookup's knob.
#ifndef SC_PER
#define SC_PER LK_PER
#endif
// The span and its halo are staged in LDS up to this k (24.5 KiB); beyond it -- by-reference contexts only -- the walk
// reads the stream itself.
#define SC_LDS_MAX_K 16385

// bytes of w that equal MK_SEP (exact per byte: no borrow between them)
#ifdef __HIPCC__
__device__ __forceinline__ unsigned sc_seps_in(unsigned w) {
  const unsigned x = w ^ (MK_SEP * 0x01010101u);
  return __popc(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu));
}

// Bytes of LDS a workgroup stages: its span and the halo of k - 1 behind it, rounded up to 16.
__host__ __device__ constexpr unsigned sc_span_bytes(int k) { return (unsigned)(SC_SPAN + k - 1 + 15) & ~15u; }

// One workgroup of 1024, in the pattern of mk_parse_scan: thread t owns tiles [t * per, (t + 1) * per).  tile_pre[i] =
// what tile_cnt holds in front of tile i.  s_c: 1024 words of the caller's LDS.  Returns the total, to thread 0 only.
__device__ __forceinline__ u64 sc_tile_scan(const unsigned* __restrict__ tile_cnt, size_t ntiles, u64* __restrict__ tile_pre, u64* s_c) {
  const size_t per = (ntiles + 1023) / 1024;
  const size_t lo = (size_t)threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
  u64 mine = 0, total = 0;
  for (size_t t = lo; t < hi; ++t) mine += tile_cnt[t];
  s_c[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int t = 0; t < 1024; ++t) {
      const u64 c = s_c[t];
      s_c[t] = total;
      total += c;
    }
  __syncthreads();
  u64 run = s_c[threadIdx.x];
  for (size_t t = lo; t < hi; ++t) {
    tile_pre[t] = run;
    run += tile_cnt[t];
  }
  return total;
}
#endif

struct ScCall {
  mk_ctx* c;
  const char* what;
  bool fold;
  u64 at_least;
  MkDevBuf scratch;  // ScStatus | tile_pre[ntiles] | tile_cnt[ntiles]
  MkTimed parse{c}, probe{c};  // (the events of the first piece serve every piece)
  mk_screen_t out{};
  size_t rows_seen = 0;
  // what the last sc_piece left on the device: the text as the parser read it (16-byte aligned: the caller's bytes or
  // their copy in c->raw), its rows (nullptr: none, or no room for them), whether row 0 has no header line
  struct {
    const uint8_t* text = nullptr;
    mk_screen_row_t* d_rows = nullptr;
    size_t nrows = 0;
    bool headless = false;
    // what a further walk over the same stream (c->seq) needs of the record scan: separators in front of every tile
    // (in s.scratch), the stream's length, the record number of row 0
    const u64* tile_pre = nullptr;
    size_t seq_len = 0;
    u64 row_base = 0;
  } last;
  ~ScCall() { buf_free(scratch); }
};

// One piece of n bytes at d_text (device memory, whole records): parsed, scanned, and -- where there is room for all its
// rows -- probed into d_rows (room rows; nullptr: the call's own buffer `own`, copied to h_rows if that is given).  The
// piece's records are added to s.rows_seen either way, and s.last holds what the parse and the scan left (text, nrows,
// headless, tile_pre, seq_len, row_base) with or without rows: room 0 is the call that wants no probe (mk_orf.hip).  The
// stream is idle afterwards.
int sc_piece(ScCall& s, const uint8_t* d_text, size_t n, mk_screen_row_t* d_rows, size_t room, MkDevBuf* own, mk_screen_row_t* h_rows);

// How the calls open (lk_open's rules) and end; body: the pieces.  cap: rows the caller has room for.
template <class Body>
static int sc_run(mk_ctx* c, const char* what, unsigned flags, uint64_t at_least, size_t cap, size_t* nrows, mk_screen_t* st,
                  Body&& body) {
  const auto t0 = MkClock::now();
  ScCall s{c, what, false, at_least};
  int rc = lk_open(c, what, flags, &s.fold);
  if (rc != MK_OK) return rc;
  if (at_least < 1) { c->err = std::string(what) + ": at_least must be 1 or more"; return MK_ERR_ARG; }
  const bool profile = c->profile;  // (the parser's launches are no part of the counting figures)
  c->profile = false;
  rc = body(s);
  c->profile = profile;
  (void)hipStreamSynchronize(c->stream);
  if (rc != MK_OK) return rc;
  if (nrows) *nrows = s.rows_seen;
  if (s.rows_seen > cap) {
    c->err = std::string(what) + ": the text holds " + std::to_string(s.rows_seen) + " records, rows has room for " + std::to_string(cap);
    return MK_ERR_RANGE;
  }
  s.out.records = s.rows_seen;
  s.out.s_total = mk_since(t0);
  if (st) *st = s.out;
  return MK_OK;
}

// A host text in pieces: cut where a record starts once a piece holds piece_bytes (mk_record_cuts; the loader's default
// and limits), each copied into c->raw and handed to piece(d_piece, len).
// The ends of those pieces for a text of n > 0 bytes, ascending; the last is n.
static int sc_piece_ends(ScCall& s, const uint8_t* text, size_t n, size_t piece_bytes, std::vector<uint64_t>& cuts) {
  mk_ctx* c = s.c;
  const size_t piece = tl_piece_size(c, piece_bytes, n);
  cuts.assign(n / piece + 2, 0);
  size_t ncuts = 0;
  int r = mk_record_cuts(text, n, piece, (size_t)4 << 20, cuts.data(), cuts.size(), &ncuts);
  if (r != MK_OK) { c->err = std::string(s.what) + ": the record scanner failed (internal error)"; return MK_ERR_STATE; }
  cuts.resize(ncuts);
  cuts.push_back(n);
  return MK_OK;
}

template <class Piece>
static int sc_text_pieces(ScCall& s, const uint8_t* text, size_t n, size_t piece_bytes, Piece&& piece_fn) {
  mk_ctx* c = s.c;
  if (!n) return MK_OK;
  std::vector<uint64_t> cuts;
  int r = sc_piece_ends(s, text, n, piece_bytes, cuts);
  if (r != MK_OK) return r;
  size_t at = 0;
  for (const uint64_t end : cuts) {
    const size_t len = (size_t)end - at;
    if (!len) continue;
    if ((r = mk_buf_reserve(c, c->raw, len + 64)) != MK_OK) return r;
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(c->raw.p, text + at, len, hipMemcpyHostToDevice, c->stream));
    s.out.s_read += mk_since(t1);
    if ((r = piece_fn((const uint8_t*)c->raw.p, len)) != MK_OK) return r;
    at = (size_t)end;
  }
  return MK_OK;
}
