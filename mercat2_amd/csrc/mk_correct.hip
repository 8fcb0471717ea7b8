// mk_correct.hip -- sequences in, every isolated substitution the table can name put right out (mk_correct_text /
// mk_correct_device, include/mercat_hip.h): the conservative k-mer-spectrum correction of Musket, Lighter, BFC and Quake
// on the GPU, where the text, the parsed stream, the rows and the count under every window already are.
//
// A piece goes through sc_piece (mk_screenpiece.h: parse, record scan, probe) and leaves its rows on the device.  Then
//   fl_tiles_k / fl_scan_k / fl_starts_k   start[r]: the first byte of every row's header line in the RAW text
//                                          (mk_recordplace.h), under the filter's guard
//   tr_hend_k, tk_starts_k                 hlen[r], sstart[r]: trim's placement (mk_trimwalk.h, mk_screenwalk.h)
//   tk_lens_k + scan, tk_probe_k           woff[], and the count under every window in device scratch: the track
//                                          (mk_trackwalk.h) -- uint32_t, saturated, while at_least fits 32 bits (the
//                                          comparison is then the same), uint64_t above
//   cr_runs_k, cr_heads_k                  a lane a window: the lane at the start of a weak run finds its record, measures
//                                          the run (k + 1 counts at most), adds to the record's runs and appends the
//                                          candidate its shape names; a lane a record for the runs that start a record
//                                          right behind a weak window
//   cr_try_k                               a wave a candidate, a lane a window of the run: the three or four alternatives
//                                          probed, "every window solid" reduced per alternative, the outcome to the record
//                                          and the patch to a list -- the stream is only read
//   cr_apply_k                             a lane a candidate: the patch into the stream
//   cr_decide_k                            a lane a record: L[r] from sstart, its output length, the guards, the totals
//   rocprim::exclusive_scan                dst[r], dst[nrows] = the piece's output length
//   tr_emit                                trim's gather with kept[r] = L[r]: header line, the characters, one LF
// A piece whose windows are all hits skips the track, cr_runs_k, cr_try_k and cr_apply_k.
//
// The candidate list holds at most as many entries as the piece has weak windows -- every candidate owns the first
// window of its run -- and the rows give that number (windows - hits) before anything is launched: no counting pass.
// ((windows + 1) / 2 bounds the runs of one record, not of a piece: records of three windows, weak solid weak, have two
// candidates each.)  Its order is the order the workgroups finished in and reaches nothing: every outcome is an integer
// added to its record, every patch a byte at a position no other candidate has.
#include "mk_correctwalk.h"

// sc_piece, then cr_piece with what that piece added to the call's windows and hits.
static int cr_both(ScCall& s, CrCall& f, const uint8_t* d_piece, size_t len, size_t first) {
  const u64 w0 = s.out.windows, h0 = s.out.hits;
  const int rc = sc_piece(s, d_piece, len, nullptr, ~(size_t)0, &f.d_rows, nullptr);
  return rc != MK_OK ? rc : cr_piece(s, f, len, first, s.out.windows - w0, s.out.hits - h0);
}

// How both calls check their own arguments, open as the screen calls open, and end; body(s): the pieces.
template <class Body>
static int cr_run(mk_ctx* c, const char* what, unsigned flags, const mk_correct_rule_t* rule, CrCall* f, size_t* out_len, size_t* nrows,
                  mk_correct_t* st, Body&& body) {
  if (!rule) { c->err = std::string(what) + ": rule is NULL"; return MK_ERR_ARG; }
  if (flags & ~MK_CORRECT_FOLD) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  if (rule->at_least < 1) { c->err = std::string(what) + ": at_least must be 1 or more"; return MK_ERR_ARG; }
  if (rule->reserved) { c->err = std::string(what) + ": reserved must be 0"; return MK_ERR_ARG; }
  if (c->alphabet != MK_ALPHABET_NT2 || c->k > 64 || tl_keys_of(c) == TL_TEXT_ONLY) {
    c->err = std::string(what) + ": takes a nucleotide context with packed keys (ALPHABET_NT2, k <= 64)";
    return MK_ERR_ARG;
  }
  const size_t cap = (f->rows || f->fix) ? f->cap : ~(size_t)0;
  f->cap = cap;
  int rc = sc_run(c, what, flags & MK_CORRECT_FOLD, rule->at_least, cap, nrows, &f->st.screen, [&](ScCall& s) { return body(s); });
  if (rc != MK_OK && rc != MK_ERR_RANGE) return rc;
  if (out_len) *out_len = f->emit.bytes_out;
  if (rc != MK_OK) return rc;
  if (f->emit.bytes_out > f->emit.out_cap) {
    c->err = std::string(what) + ": the output holds " + std::to_string(f->emit.bytes_out) + " bytes, out has room for " +
             std::to_string(f->emit.out_cap);
    return MK_ERR_RANGE;
  }
  f->st.bytes_out = f->emit.bytes_out;
  if (st) *st = f->st;
  return MK_OK;
}

extern "C" int mk_correct_device(mk_ctx* c, const uint8_t* d_text, size_t n, unsigned flags, const mk_correct_rule_t* rule, uint8_t* d_out,
                                 size_t out_cap, size_t* out_len, mk_correct_row_t* d_fix, mk_screen_row_t* d_rows, size_t cap,
                                 size_t* nrows, mk_correct_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (out_cap && !d_out)) { c->err = "mk_correct_device: NULL buffer"; return MK_ERR_ARG; }
  if (((uintptr_t)d_fix | (uintptr_t)d_rows) & 7) { c->err = "mk_correct_device: fix and rows must be aligned to 8"; return MK_ERR_ARG; }
  CrCall f(c, rule ? *rule : mk_correct_rule_t{}, d_out, out_cap, d_fix, d_rows, cap, true);
  return cr_run(c, "mk_correct_device", flags, rule, &f, out_len, nrows, st,
                [&](ScCall& s) -> int { return n ? cr_both(s, f, d_text, n, 0) : MK_OK; });
}

extern "C" int mk_correct_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, unsigned flags, const mk_correct_rule_t* rule,
                               uint8_t* out, size_t out_cap, size_t* out_len, mk_correct_row_t* fix, mk_screen_row_t* rows, size_t cap,
                               size_t* nrows, mk_correct_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (out_cap && !out)) { c->err = "mk_correct_text: NULL buffer"; return MK_ERR_ARG; }
  CrCall f(c, rule ? *rule : mk_correct_rule_t{}, out, out_cap, fix, rows, cap, false);
  return cr_run(c, "mk_correct_text", flags, rule, &f, out_len, nrows, st, [&](ScCall& s) -> int {
    return sc_text_pieces(s, text, n, piece_bytes,
                          [&](const uint8_t* d_piece, size_t len) -> int { return cr_both(s, f, d_piece, len, s.rows_seen); });
  });
}
