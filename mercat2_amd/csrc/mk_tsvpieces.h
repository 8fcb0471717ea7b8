// mk_tsvpieces.h -- a text of "<k key bytes>\t<count>\n" lines on its way to the device in pieces: what the loader
// (mk_tsvload.hip: the rows are imported) and the lookup (mk_lookup.hip: the rows are probed) share.  The pipeline --
// pinned double buffer, copy stream, line starts (tl_count_k -> scan -> tl_emit_k), the read-back of a piece's status
// and its refusals -- is TlPieces, implemented once in mk_tsvload.hip; what happens to the rows of a piece is the part
// a user of it fills in (enqueue_rows, accept).
#pragma once
#include "mk_common.h"
#include "mk_device.h"
#include "mk_tableview.h"  // TlKeys, tl_keys_of
#include <deque>

#define TL_TILE 4096u           // bytes per workgroup of the line-start passes: 256 lanes x 16 bytes
#define TL_NONE 0xFFFFFFFFu
#define TL_MAX_PIECE ((size_t)1 << 30)  // positions inside a piece are 32-bit
#define TL_DEFAULT_PIECE ((size_t)16 << 20)
// The bytes a piece of a text of n bytes holds before it is cut: piece_bytes, or (0) the default, the whole of a small
// text; never less than two of the longest rows of a table in text form, never more than 32-bit positions reach.
static inline size_t tl_piece_size(const mk_ctx* c, size_t piece_bytes, size_t n) {
  const size_t piece = piece_bytes ? piece_bytes : std::min(TL_DEFAULT_PIECE, std::max<size_t>(n + 2, 4096));
  return std::min(std::max(piece, 2 * ((size_t)c->k + 24)), TL_MAX_PIECE);
}

// what the kernels of one piece tell the host (device memory, copied back once per piece)
struct TlStatus {
  u64 bad_line;  // smallest index of a malformed line in the piece (all ones: none)
  u64 bad_byte;  // smallest offset of a byte >= 0x80 (all ones: none)
  u64 lines, packed, text, zero;
  // the lookup's: keys with a count above zero, keys replaced by their reverse complement, probes that met a slot
  // being claimed (MK_LOCK128: somebody counts into the table meanwhile)
  u64 found, folded, locked, pad;
};

// The k key bytes at `key` classified against the alphabet (bits: 2 nucleotide, 5 amino acids) and packed into the
// layout mk_import_pairs_device takes: one word, or {a, b} = {hi, lo}.  Returns whether every byte is of the alphabet
// (the words mean nothing otherwise); a by-reference context packs nothing.
template <int KEYS>
__device__ __forceinline__ bool tl_pack_key(const uint8_t* __restrict__ key, int k, int bits, u64& a, u64& b) {
  bool in_alphabet = KEYS != TL_TEXT_ONLY;
  unsigned __int128 wide = 0;
  a = b = 0;
  for (int j = 0; j < k; ++j) {
    const unsigned ch = key[j];
    unsigned code;
    if (KEYS == TL_TEXT_ONLY) continue;
    if (bits == 2) code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 99u;
    else code = (ch >= 'A' && ch <= 'Z') ? ch - 'A' : 99u;
    if (code == 99u) { in_alphabet = false; continue; }
    if (KEYS == TL_ONE_WORD) a = (a << bits) | code;
    else if (KEYS == TL_TWO_WORD_AA) wide = (wide << 5) | code;
    else if (j < 32) a |= (u64)code << (62 - 2 * j);
    else b |= (u64)code << (62 - 2 * (j - 32));
  }
  if (KEYS == TL_TWO_WORD_AA) { a = (u64)(wide >> 64); b = (u64)wide; }
  return in_alphabet;
}
// The count field of a row: n (1..20, checked by the caller) decimal digits whose value fits 64 bits.
__device__ __forceinline__ bool tl_count_field(const uint8_t* __restrict__ p, unsigned n, u64& cnt) {
  cnt = 0;
  for (unsigned j = 0; j < n; ++j) {
    const unsigned d = (unsigned)p[j] - '0';
    if (d > 9u || cnt > (~0ull - d) / 10ull) return false;
    cnt = cnt * 10ull + d;
  }
  return true;
}

struct TlSource {  // a file, or text in host memory
  int fd = -1;
  const uint8_t* mem = nullptr;
  size_t n = 0, at = 0;
  ssize_t read(uint8_t* dst, size_t want);  // up to `want` bytes into dst; less only at the end; -1: read error
};

struct TlSnap {  // pinned: the read-back of one piece
  TlStatus st;
  MkChunkInfo info;  // the context's counters after the imports of the pieces before
};

struct TlPieces {
  mk_ctx* c;
  TlSource src;
  const char* what;     // the ABI call, for messages
  bool count_optional;  // a row may end behind its key (the lookup's panels); else "\t<count>" is part of every row
  TlPieces(mk_ctx* c_, TlSource src_, const char* what_, bool count_optional_)
      : c(c_), src(src_), what(what_), count_optional(count_optional_) {}
  virtual ~TlPieces();  // (owns the file from construction on)

  // ---- what the user of the pipeline fills in
  // its device buffers for pieces of up to cap_rows rows (it gets them from hold())
  virtual int reserve() = 0;
  // the last stage of a piece, enqueued on c->stream behind tl_emit_k: the rows at line_start[0 .. min(st->lines, cap))
  virtual int enqueue_rows(int b, const uint8_t* text, const unsigned* line_start, unsigned cap, TlStatus* st) = 0;
  // the piece in half b is well formed and st (with the context's counters `before` its kernels) is on the host
  virtual int accept(int b, const TlStatus& st, const MkChunkInfo& before) = 0;

  // ---- figures of the call
  u64 bytes = 0, lines_seen = 0;
  int header = 0, pieces = 0;
  double s_read = 0, s_parse = 0;
  std::string column;  // second field of the header line

  size_t piece = 0, cap_rows = 0, max_tiles = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_copy[2] = {nullptr, nullptr}, ev[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* pinned = nullptr;
  uint8_t* hbuf[2] = {nullptr, nullptr};
  TlSnap* snap = nullptr;
  MkDevBuf dtext[2], tiles, lines, scan_tmp, status;
  std::deque<MkDevBuf> held;  // the user's buffers: freed when the call ends, after the streams have drained
  size_t scan_tmp_bytes = 0;
  // the piece in each half of the double buffer
  size_t skip[2] = {0, 0}, len[2] = {0, 0};
  std::vector<uint8_t> carry;  // the unfinished line behind the last '\n' of the piece read before
  bool eof = false, copy_used[2] = {false, false};
  u64 long_line_at = 0;  // fill() == 2: lines of its piece in front of a line longer than any data row

  MkDevBuf& hold() { held.emplace_back(); return held.back(); }  // (a deque: the reference stays good)
  size_t min_row() const { return (size_t)c->k + (count_optional ? 1 : 3); }  // bytes of the shortest row, '\n' included
  int fail(int code, const std::string& msg);
  int setup(size_t piece_bytes, size_t total_hint);
  int fill(int b);
  int enqueue_copy(int b);
  int enqueue_parse(int b);
  void locate(int b, u64 index, const uint8_t** p, size_t* n) const;
  void add_elapsed(double& to, hipEvent_t a, hipEvent_t b);
  int finish(int b);
  int too_long();
  int run();
};

// mk_tsvload.hip: open `path` as a source; *hint = its size
int tl_open(mk_ctx* c, const char* what, const char* path, TlSource* src, size_t* hint);
