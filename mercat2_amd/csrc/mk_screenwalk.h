// mk_screenwalk.h -- the lane walk over one tile of the parsed stream, with the sink a template parameter, and the
// ladder that picks a walking kernel's instantiation.  sc_probe_k (mk_screen.hip) folds every window's count into the
// record's row; tk_probe_k (mk_trackwalk.h, for mk_track.hip and mk_norm.hip) writes it where its window stands;
// tr_first_k (mk_trim.hip) keeps the place of the first low one.  tk_starts_k, which tells a positional sink where every
// record starts in the stream, is here too (static: mk_track.hip, mk_trim.hip and mk_norm.hip each launch their own copy).  The walk's device code reacts to
// restructuring: a change here is measured on both kernels (profiles/screen_walk.md, DESIGN 8p "one walk").
//
// A lane owns SC_RUN consecutive window starts: it walks k - 1 + SC_RUN symbols of the workgroup's span (staged in LDS
// once, with a halo of k - 1), ROLLS the packed key one symbol at a time, keeps "symbols since the last separator" (is
// this a window?) and "symbols since the last byte outside the alphabet" (packed key or text key?) and probes where
// lk_probe_k would probe the same k bytes, SC_PER home-slot loads of the one-word table in flight.  Integer work only:
// exact in any order.  What it hands to the sink, in stream order:
//   sink.begin(rid, at)         the lane's run starts at stream position `at`, inside record rid
//   sink.record_end(rid)        a separator among the lane's window starts: record rid ends in front of it
//   sink.window(rid, pos, cnt)  a window of record rid has count cnt; it starts at the pos-th of the record's symbols THE
//                               LANE HAS SEEN: since_sep is the lane's own, so for the record its run started in the
//                               sink adds what lay in front of the run
#pragma once
#include "mk_screenpiece.h"
#include "mk_tableview.h"
#include <type_traits>

struct ScWalked {  // what a lane's walk counted
  u64 windows = 0, packed = 0, text = 0, folded = 0;
  bool locked = false;
};

// The walk of the calling lane over tile blockIdx.x (workgroups of 256).  s_seq: dynamic LDS of sc_span_bytes(k)
// (unused when LDS is false: KEYS == TL_TEXT_ONLY with a k whose halo LDS cannot hold).  Returns the
// record the lane ends in.  Every lane of the workgroup must call it (two barriers inside).
template <int KEYS, bool FOLD, bool LDS, class Sink>
__device__ __forceinline__ u64 sc_walk(uint8_t* __restrict__ s_seq, const uint8_t* __restrict__ seq, u64 seq_len,
                                       const u64* __restrict__ tile_pre, int k, int bits, const LkTables& t, Sink& sink,
                                       ScWalked& n) {
  __shared__ unsigned s_wave[4];
  const u64 base = (u64)blockIdx.x * SC_SPAN;
  if (LDS) {
    const unsigned stage = sc_span_bytes(k);
    for (unsigned i = threadIdx.x * 16u; i < stage; i += 256u * 16u) {
      if (base + i + 16 <= seq_len) *reinterpret_cast<uint4*>(s_seq + i) = *reinterpret_cast<const uint4*>(seq + base + i);
      else
        for (unsigned j = 0; j < 16; ++j) s_seq[i + j] = base + i + j < seq_len ? seq[base + i + j] : (uint8_t)MK_SEP;
    }
    __syncthreads();
  }
  // symbol at local index li of the span; positions behind the stream are separators
  auto sym_at = [&](unsigned li) -> unsigned { return LDS ? s_seq[li] : (base + li < seq_len ? seq[base + li] : MK_SEP); };

  // the record this lane's run starts in: separators in front of the tile, of the lanes before it in the workgroup
  const unsigned l0 = threadIdx.x * SC_RUN;
  unsigned own = 0;
  if (LDS) {
#pragma unroll
    for (int i = 0; i < SC_RUN / 4; ++i) own += sc_seps_in(reinterpret_cast<const unsigned*>(s_seq + l0)[i]);
  } else {
    for (int j = 0; j < SC_RUN; ++j) own += sym_at(l0 + j) == MK_SEP;
  }
  u64 rid = tile_pre[blockIdx.x] + mk_block_scan_excl(own, s_wave);
  sink.begin(rid, base + l0);

  // ---- the walk: k - 1 symbols to fill the key, then one window start a symbol
  const int kb = k * bits;
  const u64 mask1 = kb >= 64 ? ~0ull : (1ull << kb) - 1;                                       // one-word keys
  const unsigned __int128 mask_aa = (((unsigned __int128)1) << (kb > 127 ? 127 : kb)) - 1;     // protein 13..25-mers
  const int sh2 = 128 - 2 * k;                                                                 // two-word nt: the last base's place in lo
  u64 a = 0, b = 0;
  unsigned __int128 wide = 0;
  unsigned since_sep = 0, since_bad = 0;  // symbols since the last separator / the last byte outside the alphabet
  unsigned li = l0, word = 0;
  auto step = [&]() -> bool {  // takes the next symbol in; true: it is a separator
    unsigned ch;
    if (LDS) {
      if ((li & 3u) == 0) word = reinterpret_cast<const unsigned*>(s_seq)[li >> 2];
      ch = word & 0xFFu;
      word >>= 8;
    } else ch = sym_at(li);
    ++li;
    if (ch == MK_SEP) { since_sep = since_bad = 0; return true; }
    ++since_sep;
    if (KEYS == TL_TEXT_ONLY) return false;
    unsigned code;
    if (bits == 2) code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 99u;
    else code = (ch >= 'A' && ch <= 'Z') ? ch - 'A' : 99u;
    if (code == 99u) { since_bad = 0; return false; }  // (what the key holds is pushed out before it is used again)
    ++since_bad;
    if (KEYS == TL_ONE_WORD) a = ((a << bits) | code) & mask1;
    else if (KEYS == TL_TWO_WORD_AA) wide = ((wide << 5) | code) & mask_aa;
    else { a = (a << 2) | (b >> 62); b = (b << 2) | ((u64)code << sh2); }
    return false;
  };
  for (int q = 1; q < k; ++q) rid += step() ? 1 : 0;

  for (int g = 0; g < SC_RUN; g += SC_PER) {
    u64 key[SC_PER], res[SC_PER];
    ulonglong2 home[SC_PER];
    unsigned pos[SC_PER];
    bool sep[SC_PER], window[SC_PER], pending[SC_PER];
#pragma unroll
    for (int j = 0; j < SC_PER; ++j) {
      sep[j] = step();
      window[j] = !sep[j] && since_sep >= (unsigned)k;
      pos[j] = since_sep - (unsigned)k;
      pending[j] = false;
      res[j] = 0;
      if (!window[j]) continue;
      if (KEYS != TL_TEXT_ONLY && since_bad >= (unsigned)k) {
        ++n.packed;
        u64 ka = a, kb2 = b;
        if (KEYS == TL_TWO_WORD_AA) { ka = (u64)(wide >> 64); kb2 = (u64)wide; }
        if (FOLD) n.folded += LkStep<KEYS, SC_PER>::fold(ka, kb2, k) ? 1 : 0;
        // (LkStep's issue and finish, spelled out here: with the whole step sc_probe_k's s_probe was 2 to 6 % slower on
        // the MI355X, outside the spread of this form, and the cause is not known -- profiles/table_reads_refactor.md)
        if (KEYS == TL_ONE_WORD) {
          if (t.bins) res[j] = find_dense(t.bins, (size_t)t.nbins, ka);
          else if (ka == MK_EMPTY) res[j] = t.side;
          else if (t.run_slots) {
            key[j] = ka;
            home[j] = find64_home(t.run, t.run_slots - 1, ka);
            pending[j] = true;
          }
        } else if (t.run128_slots) res[j] = find128(t.run128, t.run128_slots - 1, ka, kb2, &n.locked);
      } else {
        ++n.text;
        const uint8_t* w = LDS ? s_seq + (li - (unsigned)k) : seq + base + (li - (unsigned)k);  // the window that ends here
        if (t.ref_slots) res[j] = find_ref_of(t.ref, t.ref_slots - 1, t.arena, BytesAt{w}, k);
      }
    }
#pragma unroll
    for (int j = 0; j < SC_PER; ++j) {
      if (sep[j]) {  // the record ends in front of this symbol
        sink.record_end(rid);
        ++rid;
      }
      if (!window[j]) continue;
      if (pending[j]) res[j] = find64_from(t.run, t.run_slots - 1, key[j], home[j]);
      ++n.windows;
      sink.window(rid, pos[j], res[j]);
    }
  }
  return rid;
}

// sstart[r] = the stream position of the first symbol of row r: behind its separator, 0 for a headless row 0.  The
// record scan of sc_probe_k on the stream's own tiles (tile_pre: separators in front of every tile).
static __global__ void __launch_bounds__(256) tk_starts_k(const uint8_t* __restrict__ seq, u64 seq_len, const u64* __restrict__ tile_pre,
                                                   u64 row_base, size_t nrows, u64* __restrict__ sstart) {
  __shared__ unsigned s_wave[4];
  const u64 at = (u64)blockIdx.x * SC_SPAN + (u64)threadIdx.x * SC_RUN;
  unsigned own = 0;
  for (int j = 0; j < SC_RUN && at + j < seq_len; ++j) own += seq[at + j] == MK_SEP;
  u64 rid = tile_pre[blockIdx.x] + mk_block_scan_excl(own, s_wave);
  if (blockIdx.x == 0 && threadIdx.x == 0 && row_base == 0 && nrows) sstart[0] = 0;
  if (own)
    for (int j = 0; j < SC_RUN && at + j < seq_len; ++j)
      if (seq[at + j] == MK_SEP) {
        ++rid;
        if (rid - row_base < nrows) sstart[rid - row_base] = at + j + 1;
      }
}

// The seven instantiations of a walking kernel, by the context's key kind, the call's fold and whether LDS holds the
// halo of this k: go(KEYS, FOLD, LDS), each a std::integral_constant, launches the one that serves s.
template <class Go>
static int sc_dispatch_walk(const ScCall& s, Go&& go) {
  using std::false_type;
  using std::true_type;
  const int keys = tl_keys_of(s.c);
  if (keys == TL_ONE_WORD) {
    std::integral_constant<int, TL_ONE_WORD> one;
    return s.fold ? go(one, true_type{}, true_type{}) : go(one, false_type{}, true_type{});
  }
  if (keys == TL_TWO_WORD_NT) {
    std::integral_constant<int, TL_TWO_WORD_NT> two;
    return s.fold ? go(two, true_type{}, true_type{}) : go(two, false_type{}, true_type{});
  }
  if (keys == TL_TWO_WORD_AA) return go(std::integral_constant<int, TL_TWO_WORD_AA>{}, false_type{}, true_type{});
  std::integral_constant<int, TL_TEXT_ONLY> text;
  return s.c->k <= SC_LDS_MAX_K ? go(text, false_type{}, true_type{}) : go(text, false_type{}, false_type{});
}
