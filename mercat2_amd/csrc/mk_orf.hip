// mk_orf.hip -- nucleotide records in, their six-frame open reading frames out as protein FASTA (mk_orf_text /
// mk_orf_device, include/mercat_hip.h): stop-to-stop ORF calling, optionally from the first start codon, on the GPU,
// where the text and the parsed stream already are.
//
// A piece goes through sc_piece (mk_screenpiece.h) with room for no rows: parse and record scan, no probe.  The stream
// (c->seq) holds the kept characters and one MK_SEP where a header line starts.  In STREAM coordinates both strands look
// alike: the codons of one (strand, class) are the positions of one residue mod 3 inside the record, a stop of the
// reverse strand is TTA CTA TCA read forward, and a stretch [a, b) is closed at its right end b by a stop that starts
// there or by the record's end (b = end - 2 .. end, one per residue).  So every ORF belongs to one closing (position,
// strand), and the order the rule asks for -- record, right end, forward before reverse -- is the order of the stream.
// What a closing needs from its left is a carry per (strand, residue): where the stretch began (behind the last stop, or
// at the record's start), and in start mode the first forward start and the last reverse start since then.  OR_SPAN and
// OR_RUN are multiples of 3, so the residue of a position is that of its index in a lane's run: a compile-time constant
// once the walk is unrolled, and no carry is ever indexed by a run-time value.
//   or_tiles_k     a lane walks OR_RUN positions from the empty carry; the workgroup combines its lanes: tsum[tile]
//   or_carry_k     one workgroup: carry[tile] = the initial carry combined with tsum[0 .. tile)
//   or_emit_k<.,0> the same walk, now from carry[tile] and the lanes in front: ORFs a lane closes (min_aa, strand
//                  flags applied) -> lane_cnt, tile_cnt
//   or_scan_k      one workgroup (sc_tile_scan): tile_pre, the piece's number of ORFs
//   or_emit_k<.,1> the walk once more: rows[i] and src[i] at tile_pre + the lanes in front; reclen[row] at a record's end
//   fl_tiles_k / fl_scan_k / fl_starts_k   start[r] of every header line in the raw text (mk_recordplace.h)
//   or_name_k      a lane per record: where its name starts behind the '>' and how long it is
//   or_len_k       a lane per ORF: the reverse frame (it needs the record's length), the rank within the record (a search
//                  of rows[] for the record's first ORF), the bytes of its output record
//   rocprim::exclusive_scan                dst[i], dst[norfs] = the piece's output length
//   or_gather_k (or_edges_k)               tr_gather_k's form: a lane owns 16 aligned output bytes, one search of dst[] a
//                                          wave; the name from the raw text, the decimal fields computed in the lane, the
//                                          amino acids from three stream bytes each through the 64-entry table in LDS
// Carries travel between launches only; nothing on the output is atomic.
#include "mk_recordplace.h"
#include <rocprim/device/device_scan.hpp>

#define OR_RUN 48               // stream positions a lane owns
#define OR_SPAN (256 * OR_RUN)  // ... a workgroup: one tile of the ORF scan
static_assert(OR_RUN % 3 == 0 && OR_RUN % 16 == 0, "the residue of a position must be that of its index in the run");

// Standard code, index 16 c1 + 4 c2 + c3 with A 0, C 1, G 2, T 3.
__constant__ uint8_t OR_TABLE[65] = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";
#define OR_BIT(i) (1ull << (i))
#define OR_FWD_STOPS (OR_BIT(48) | OR_BIT(50) | OR_BIT(56))   // TAA TAG TGA
#define OR_REV_STOPS (OR_BIT(60) | OR_BIT(28) | OR_BIT(52))   // TTA CTA TCA
#define OR_FWD_ATG OR_BIT(14)
#define OR_FWD_ALT (OR_BIT(46) | OR_BIT(62))                  // GTG TTG
#define OR_REV_ATG OR_BIT(19)                                 // CAT
#define OR_REV_ALT (OR_BIT(17) | OR_BIT(16))                  // CAC CAA

// The carry.  Positions are stored + 1, 0: none.
//   v[0..2], v[3..5]  where the open stretch of (forward, reverse) residue g begins
//   v[6]              where the record begins
//   v[7..9]           forward: the first start of residue g since its stretch began
//   v[10..12]         reverse: the last start of residue g (it counts only if it lies inside the open stretch)
//   v[13]             separators so far (a sum, the one value that is no position)
#define OR_NV 14
struct OrState { u64 v[OR_NV]; };

// x = p followed by x.
template <bool START>
__device__ __forceinline__ void or_combine(const OrState& p, OrState& x) {
  if (START) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      if (!x.v[g]) x.v[7 + g] = p.v[7 + g] ? p.v[7 + g] : x.v[7 + g];  // (no boundary in x: p's first start stands)
      x.v[10 + g] = p.v[10 + g] > x.v[10 + g] ? p.v[10 + g] : x.v[10 + g];
    }
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) x.v[i] = p.v[i] > x.v[i] ? p.v[i] : x.v[i];
  x.v[13] += p.v[13];
}

// Inclusive scan of x over the 256 threads of a workgroup, in thread order; s: OR_NV * 256 words of LDS, which hold every
// thread's inclusive value afterwards.  Every thread must call it.
template <bool START>
__device__ __forceinline__ void or_block_scan(OrState& x, u64* s) {
  const unsigned t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < OR_NV; ++i) s[i * 256 + t] = x.v[i];
  __syncthreads();
  for (unsigned d = 1; d < 256; d <<= 1) {
    OrState p;
    if (t >= d) {
#pragma unroll
      for (int i = 0; i < OR_NV; ++i) p.v[i] = s[i * 256 + t - d];
    }
    __syncthreads();
    if (t >= d) {
      or_combine<START>(p, x);
#pragma unroll
      for (int i = 0; i < OR_NV; ++i) s[i * 256 + t] = x.v[i];
    }
    __syncthreads();
  }
}

// A 0, C 1, G 2, T and U 3 in either case, MK_SEP 5, every other byte 4.
__device__ __forceinline__ unsigned or_code(unsigned b) {
  const unsigned l = b | 0x20u;
  return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : (l == 't' || l == 'u') ? 3u : b == MK_SEP ? 5u : 4u;
}

struct OrRule {
  u64 min_nt;       // 3 * min_aa
  unsigned strands; // bit 0: forward, bit 1: reverse
  unsigned alt;     // start mode: GTG and TTG start too
};

struct OrNoSink {
  __device__ __forceinline__ void orf(unsigned, int, u64, u64, u64, u64) {}
  __device__ __forceinline__ void record_end(u64, u64) {}
};

// The ORF that the closing at position p of (strand S, residue G) leaves, if any, to sink.orf.
template <bool START, int S, int G, class Sink>
__device__ __forceinline__ void or_close(const OrState& st, const OrRule& rule, u64 p, Sink& sink) {
  if (!(rule.strands & (1u << S))) return;
  const u64 a1 = st.v[3 * S + G];
  u64 lo = a1 - 1, hi = p;
  if (START) {
    if (S == 0) {
      if (!st.v[7 + G]) return;
      lo = st.v[7 + G] - 1;
    } else {
      if (st.v[10 + G] < a1) return;
      hi = st.v[10 + G] - 1 + 3;
    }
  }
  if (!a1 || hi < lo || hi - lo < rule.min_nt) return;
  sink.orf(S, G, lo, hi, st.v[6] - 1, st.v[13]);
}

// The tile's bytes [tile * OR_SPAN, + OR_SPAN + 16) of the stream into s_seq (OR_SPAN / 16 + 1 uint4): the halo serves the
// codons that start at the tile's last two positions.  (seq is 256-byte aligned with 256 bytes of room behind the stream;
// what lies behind seq_len is loaded where the allocation holds it and never looked at.)  Ends in a barrier.
__device__ __forceinline__ void or_stage(const uint8_t* __restrict__ seq, u64 seq_len, uint4* s_seq) {
  const u64 tile = (u64)blockIdx.x * OR_SPAN;
  for (unsigned i = threadIdx.x; i < OR_SPAN / 16 + 1; i += 256) {
    const u64 at = tile + 16ull * i;
    s_seq[i] = at <= seq_len ? *reinterpret_cast<const uint4*>(seq + at) : make_uint4(0, 0, 0, 0);
  }
  __syncthreads();
}

// Position p of residue G with the codes of p, p + 1 and p + 2.
template <bool START, int G, class Sink>
__device__ __forceinline__ void or_step(u64 p, u64 seq_len, unsigned c0, unsigned c1, unsigned c2, const OrRule& rule, u64 fstart,
                                        u64 rstart, OrState& st, Sink& sink) {
  if (p > seq_len) return;
  const bool end = c0 == 5u;                     // a separator, or the end of the stream: the record ends here
  const bool near = end || c1 == 5u || c2 == 5u; // ... or one or two positions on: this residue's stretches end here
  const bool codon = (c0 | c1 | c2) < 4u;
  const unsigned idx = (16 * c0 + 4 * c1 + c2) & 63u;
  const bool fstop = codon && ((OR_FWD_STOPS >> idx) & 1), rstop = codon && ((OR_REV_STOPS >> idx) & 1);
  if (near || fstop) or_close<START, 0, G>(st, rule, p, sink);
  if (near || rstop) or_close<START, 1, G>(st, rule, p, sink);
  if (end) {
    sink.record_end(st.v[13], p - (st.v[6] - 1));
#pragma unroll
    for (int gg = 0; gg < 3; ++gg) {
      constexpr int next = (G + 1) % 3;
      const int d = (gg - next + 3) % 3;  // the first position of residue gg behind p is p + 1 + d
      st.v[gg] = st.v[3 + gg] = p + 2 + d;
      if (START) st.v[7 + gg] = 0;
    }
    st.v[6] = p + 2;
    st.v[13] += 1;
  } else if (fstop) {
    st.v[G] = p + 4;
    if (START) st.v[7 + G] = 0;
  } else if (rstop) {
    st.v[3 + G] = p + 4;
  } else if (START && codon) {
    if (((fstart >> idx) & 1) && !st.v[7 + G]) st.v[7 + G] = p + 1;
    if ((rstart >> idx) & 1) st.v[10 + G] = p + 1;
  }
}

// The positions [base, base + OR_RUN) of the stream, and the one behind its last byte, which closes the last record like a
// separator.  lane: the run's bytes and two more, in LDS.  st: the carry in front of base, the carry behind the run
// afterwards.  base is a multiple of 3, so the residue of a position is that of its index: every carry is named at
// compile time, unrolled or not.
template <bool START, class Sink>
__device__ __forceinline__ void or_walk(const uint8_t* lane, u64 seq_len, u64 base, const OrRule& rule, OrState& st, Sink& sink) {
  if (base > seq_len) return;
  auto code_at = [&](int j) -> unsigned { return base + j < seq_len ? or_code(lane[j]) : 5u; };
  const u64 fstart = OR_FWD_ATG | (rule.alt ? OR_FWD_ALT : 0ull), rstart = OR_REV_ATG | (rule.alt ? OR_REV_ALT : 0ull);
  unsigned c0 = code_at(0), c1 = code_at(1);
  for (int j = 0; j < OR_RUN; j += 3) {
    const unsigned c2 = code_at(j + 2), c3 = code_at(j + 3), c4 = code_at(j + 4);
    or_step<START, 0>(base + j, seq_len, c0, c1, c2, rule, fstart, rstart, st, sink);
    or_step<START, 1>(base + j + 1, seq_len, c1, c2, c3, rule, fstart, rstart, st, sink);
    or_step<START, 2>(base + j + 2, seq_len, c2, c3, c4, rule, fstart, rstart, st, sink);
    c0 = c3;
    c1 = c4;
  }
}

__device__ __forceinline__ OrState or_none() {
  OrState x;
#pragma unroll
  for (int i = 0; i < OR_NV; ++i) x.v[i] = 0;
  return x;
}

// tsum[tile]: what the tile's positions do to a carry.
template <bool START>
__global__ void __launch_bounds__(256) or_tiles_k(const uint8_t* __restrict__ seq, u64 seq_len, OrRule rule, u64* __restrict__ tsum) {
  __shared__ u64 s[OR_NV * 256];
  __shared__ uint4 s_seq[OR_SPAN / 16 + 1];
  or_stage(seq, seq_len, s_seq);
  OrState x = or_none();
  OrNoSink none;
  or_walk<START>((const uint8_t*)s_seq + threadIdx.x * OR_RUN, seq_len, (u64)blockIdx.x * OR_SPAN + (u64)threadIdx.x * OR_RUN, rule, x, none);
  or_block_scan<START>(x, s);
  if (threadIdx.x == 255) {
#pragma unroll
    for (int i = 0; i < OR_NV; ++i) tsum[(size_t)blockIdx.x * OR_NV + i] = x.v[i];
  }
}

// One workgroup of 256: thread t owns tiles [t * per, (t + 1) * per).  carry[tile] = the carry at the start of the stream
// (every stretch and the record begin at their first position) combined with tsum[0 .. tile).
template <bool START>
__global__ void __launch_bounds__(256) or_carry_k(const u64* __restrict__ tsum, size_t ntiles, u64* __restrict__ carry) {
  __shared__ u64 s[OR_NV * 256];
  const size_t per = (ntiles + 255) / 256;
  const size_t lo = (size_t)threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
  auto load = [&](size_t t) {
    OrState y;
#pragma unroll
    for (int i = 0; i < OR_NV; ++i) y.v[i] = tsum[t * OR_NV + i];
    return y;
  };
  OrState x = or_none();
  for (size_t t = lo; t < hi; ++t) {
    OrState y = load(t);
    or_combine<START>(x, y);
    x = y;
  }
  or_block_scan<START>(x, s);
  OrState run = or_none();
#pragma unroll
  for (int g = 0; g < 3; ++g) run.v[g] = run.v[3 + g] = g + 1;
  run.v[6] = 1;
  if (threadIdx.x) {
    OrState y;
#pragma unroll
    for (int i = 0; i < OR_NV; ++i) y.v[i] = s[i * 256 + threadIdx.x - 1];
    or_combine<START>(run, y);
    run = y;
  }
  for (size_t t = lo; t < hi; ++t) {
#pragma unroll
    for (int i = 0; i < OR_NV; ++i) carry[t * OR_NV + i] = run.v[i];
    OrState y = load(t);
    or_combine<START>(run, y);
    run = y;
  }
}

struct OrCountSink {
  unsigned cnt = 0;
  __device__ __forceinline__ void orf(unsigned, int, u64, u64, u64, u64) { ++cnt; }
  __device__ __forceinline__ void record_end(u64, u64) {}
};

// Where the emit pass puts what it finds.  rows[i].frame of a reverse ORF is 4 until or_len_k has the record's length.
struct OrRowSink {
  mk_orf_row_t* __restrict__ rows;
  u64* __restrict__ src;     // forward: the stream position of the first codon; reverse: the one behind the last
  u64* __restrict__ reclen;  // per row of the piece
  u64 at, end, norfs, nrows, row_base, first_record;
  __device__ __forceinline__ void orf(unsigned strand, int, u64 lo, u64 hi, u64 rec_at, u64 seps) {
    if (at < end && at < norfs) {  // (always: the count pass took the same walk)
      const u64 begin = lo - rec_at;
      rows[at] = mk_orf_row_t{first_record + (seps - row_base), begin, (unsigned)((hi - lo) / 3), strand ? 4u : 1u + (unsigned)(begin % 3)};
      src[at] = strand ? hi : lo;
    }
    ++at;
  }
  __device__ __forceinline__ void record_end(u64 seps, u64 len) {
    const u64 row = seps - row_base;  // (the separator at position 0 of a text that starts with a header line ends no row)
    if (row < nrows) reclen[row] = len;
  }
};

// EMIT false: lane_cnt[tile * 256 + lane], tile_cnt[tile].  EMIT true: the rows, from tile_pre[tile] on.
template <bool START, bool EMIT>
__global__ void __launch_bounds__(256) or_emit_k(const uint8_t* __restrict__ seq, u64 seq_len, OrRule rule, const u64* __restrict__ carry,
                                                 unsigned* __restrict__ lane_cnt, unsigned* __restrict__ tile_cnt,
                                                 const u64* __restrict__ tile_pre, OrRowSink out) {
  __shared__ u64 s[OR_NV * 256];
  __shared__ unsigned s_wave[4];
  __shared__ uint4 s_seq[OR_SPAN / 16 + 1];
  or_stage(seq, seq_len, s_seq);
  const uint8_t* lane = (const uint8_t*)s_seq + threadIdx.x * OR_RUN;
  const u64 base = (u64)blockIdx.x * OR_SPAN + (u64)threadIdx.x * OR_RUN;
  OrState x = or_none();
  OrNoSink none;
  or_walk<START>(lane, seq_len, base, rule, x, none);
  or_block_scan<START>(x, s);
#pragma unroll
  for (int i = 0; i < OR_NV; ++i) x.v[i] = carry[(size_t)blockIdx.x * OR_NV + i];
  if (threadIdx.x) {
    OrState y;
#pragma unroll
    for (int i = 0; i < OR_NV; ++i) y.v[i] = s[i * 256 + threadIdx.x - 1];
    or_combine<START>(x, y);
    x = y;
  }
  if (!EMIT) {
    OrCountSink cs;
    or_walk<START>(lane, seq_len, base, rule, x, cs);
    lane_cnt[(size_t)blockIdx.x * 256 + threadIdx.x] = cs.cnt;
    const unsigned sum = mk_wave_sum(cs.cnt);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  } else {
    const unsigned own = lane_cnt[(size_t)blockIdx.x * 256 + threadIdx.x];
    out.at = tile_pre[blockIdx.x] + mk_block_scan_excl(own, s_wave);
    out.end = out.at + own;
    or_walk<START>(lane, seq_len, base, rule, x, out);
  }
}

struct OrStatus {  // device memory, read back once a piece
  FlStatus fl;
  u64 norfs, residues, longest, sumlen, names, per_frame[6];
};

static __global__ void __launch_bounds__(1024) or_scan_k(const unsigned* __restrict__ tile_cnt, size_t ntiles, u64* __restrict__ tile_pre,
                                                         OrStatus* __restrict__ st) {
  __shared__ u64 s_c[1024];
  const u64 total = sc_tile_scan(tile_cnt, ntiles, tile_pre, s_c);
  if (threadIdx.x == 0) st->norfs = total;
}

// A lane per record: nsrc[r] = the byte behind the '>' of its header line, nlen[r] = the bytes from there to the first one
// <= 0x20 or the end of the text.  A headless row 0, or a start outside the text (the host's guard reports it), has none.
static __global__ void __launch_bounds__(256) or_name_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ start, size_t nrows,
                                                        int headless, u64* __restrict__ nsrc, u64* __restrict__ nlen) {
  mk_for_each(nrows, [&](size_t r) {
    u64 p = start[r];
    if ((headless && r == 0) || p >= n) { nsrc[r] = 0; nlen[r] = 0; return; }
    while (p < n && mk_is_blank(text[p])) ++p;
    if (p < n) ++p;  // the '>'
    u64 q = p;
    while (q < n && text[q] > 0x20u) ++q;
    nsrc[r] = p;
    nlen[r] = q - p;
  });
}

__device__ __forceinline__ unsigned or_digits(u64 v) {
  unsigned d = 1;
  while (v >= 10) { v /= 10; ++d; }
  return d;
}

// A lane per ORF (and one for the slot behind the last, whose length is 0 so that the scan ends in the total).
static __global__ void __launch_bounds__(256) or_len_k(mk_orf_row_t* __restrict__ rows, size_t norfs, u64 first_record,
                                                       const u64* __restrict__ reclen, const u64* __restrict__ nlen, size_t nrows,
                                                       u64* __restrict__ rank, u64* __restrict__ len, OrStatus* __restrict__ st) {
  u64 residues = 0, sumlen = 0, names = 0, longest = 0, pf[6] = {0, 0, 0, 0, 0, 0};
  mk_for_each(norfs + 1, [&](size_t i) {
    if (i == norfs) { len[i] = 0; return; }
    const u64 record = rows[i].record, row = record - first_record, begin = rows[i].begin;
    const unsigned aa = rows[i].aa;
    unsigned frame = rows[i].frame;
    if (row >= nrows) { len[i] = 0; rank[i] = 0; return; }  // (cannot happen: the host's sum check reports it)
    if (frame >= 4) {
      frame = 4 + (unsigned)((reclen[row] - begin) % 3);
      rows[i].frame = frame;
    }
    size_t lo = 0, hi = i;  // the first ORF of this record: the smallest j with rows[j].record >= record
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (rows[mid].record < record) lo = mid + 1;
      else hi = mid;
    }
    const u64 rk = i - lo + 1;
    rank[i] = rk;
    const u64 l = 7 + nlen[row] + or_digits(begin + 1) + or_digits(rk) + aa;
    len[i] = l;
    residues += aa;
    sumlen += l;
    names += nlen[row];
    longest = aa > longest ? aa : longest;
#pragma unroll
    for (int f = 0; f < 6; ++f) pf[f] += frame == (unsigned)(f + 1) ? 1 : 0;
  });
  block_add(&st->residues, residues);
  block_add(&st->sumlen, sumlen);
  block_add(&st->names, names);
#pragma unroll
  for (int f = 0; f < 6; ++f) block_add(&st->per_frame[f], pf[f]);
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = __shfl_down(longest, d);
    longest = o > longest ? o : longest;
  }
  if ((threadIdx.x & 63) == 0 && longest) atomicMax((unsigned long long*)&st->longest, (unsigned long long)longest);
}

// What the gather knows of an ORF's output record.
struct OrRec {
  u64 at, nsrc, nl, begin1, rank, src;
  unsigned d1, d2, aa, frame;
};
struct OrPlace {
  const uint8_t* __restrict__ text;
  u64 n;
  const uint8_t* __restrict__ seq;
  u64 seq_len;
  const mk_orf_row_t* __restrict__ rows;
  const u64* __restrict__ src;
  const u64* __restrict__ rank;
  const u64* __restrict__ nsrc;
  const u64* __restrict__ nlen;
  const u64* __restrict__ dst;
  size_t norfs;
  u64 first_record;
  __device__ __forceinline__ OrRec rec(size_t i) const {
    const mk_orf_row_t r = rows[i];
    const u64 row = r.record - first_record;
    const u64 rk = rank[i];
    return OrRec{dst[i], nsrc[row], nlen[row], r.begin + 1, rk, src[i], or_digits(r.begin + 1), or_digits(rk), r.aa, r.frame};
  }
};

// decimal digit e (0: the last) of v
__device__ __forceinline__ uint8_t or_digit(u64 v, unsigned e) {
  for (; e; --e) v /= 10;
  return (uint8_t)('0' + v % 10);
}

// Byte q of the ORF's output record: '>' name '_' begin+1 '_' frame '_' rank LF amino acids LF.  tab: OR_TABLE in LDS.
__device__ __forceinline__ uint8_t or_byte(const OrPlace& p, const OrRec& c, u64 q, const uint8_t* tab) {
  if (q == 0) return '>';
  q -= 1;
  if (q < c.nl) return c.nsrc + q < p.n ? p.text[c.nsrc + q] : (uint8_t)'?';
  q -= c.nl;
  if (q == 0) return '_';
  q -= 1;
  if (q < c.d1) return or_digit(c.begin1, c.d1 - 1 - (unsigned)q);
  q -= c.d1;
  if (q == 0 || q == 2) return '_';
  if (q == 1) return (uint8_t)('0' + c.frame);
  q -= 3;
  if (q < c.d2) return or_digit(c.rank, c.d2 - 1 - (unsigned)q);
  q -= c.d2;
  if (q == 0 || q > c.aa) return 10;
  q -= 1;  // the amino acid q: three stream bytes, read backwards and complemented on the reverse strand
  unsigned c0, c1, c2;
  if (c.frame < 4) {
    const u64 s = c.src + 3 * q;
    if (s + 3 > p.seq_len) return 'X';
    c0 = or_code(p.seq[s]); c1 = or_code(p.seq[s + 1]); c2 = or_code(p.seq[s + 2]);
  } else {
    const u64 e = c.src - 3 * q;
    if (e > p.seq_len || e < 3) return 'X';
    c0 = or_code(p.seq[e - 1]); c1 = or_code(p.seq[e - 2]); c2 = or_code(p.seq[e - 3]);
    if ((c0 | c1 | c2) < 4u) { c0 = 3 - c0; c1 = 3 - c1; c2 = 3 - c2; }
  }
  return (c0 | c1 | c2) < 4u ? tab[16 * c0 + 4 * c1 + c2] : (uint8_t)'X';
}

// Chunks, rounds and the search as in tr_gather_k: a lane fills 16 aligned output bytes, ORF by ORF (every ORF's record
// holds 8 bytes or more, so the one behind i is i + 1), and stores them at once.
#define OR_CHUNKS 4
static __global__ void __launch_bounds__(256) or_gather_k(OrPlace p, u64 head, u64 nbody, uint8_t* __restrict__ out) {
  __shared__ uint8_t s_tab[64];
  if (threadIdx.x < 64) s_tab[threadIdx.x] = OR_TABLE[threadIdx.x];
  __syncthreads();
  const u64 g0 = fl_first_lane((((u64)blockIdx.x * 256 + threadIdx.x) >> 6) * (64 * OR_CHUNKS));
  if (g0 >= nbody) return;
  size_t r = fl_record_of(p.dst, 0, p.norfs - 1, head + 16 * g0);
  for (int j = 0; j < OR_CHUNKS; ++j) {
    const u64 g = g0 + j * 64 + (threadIdx.x & 63);
    if (g >= nbody) break;
    const u64 o0 = head + 16 * g;
    r = fl_record_from(p.dst, r, p.norfs, o0);
    OrRec c = p.rec(r);
    u64 end = p.dst[r + 1];
    u64 v0 = 0, v1 = 0;
#pragma unroll
    for (unsigned b = 0; b < 16; ++b) {
      const u64 o = o0 + b;
      if (o >= end && r + 1 < p.norfs) {  // (bytes follow: o < dst[norfs], so r + 1 is an ORF)
        ++r;
        c = p.rec(r);
        end = p.dst[r + 1];
      }
      const u64 x = or_byte(p, c, o - c.at, s_tab);
      if (b < 8) v0 |= x << (8 * b);
      else v1 |= x << (8 * (b - 8));
    }
    *reinterpret_cast<uint4*>(out + o0) = make_uint4((unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32));
  }
}

// The bytes in front of the first aligned 16 of the output (head of them) and behind the last (from tail_at on): a lane
// a byte, at most 15 + 15.
static __global__ void __launch_bounds__(64) or_edges_k(OrPlace p, u64 head, u64 tail_at, u64 out_len, uint8_t* __restrict__ out) {
  __shared__ uint8_t s_tab[64];
  s_tab[threadIdx.x] = OR_TABLE[threadIdx.x];
  __syncthreads();
  u64 o;
  if (threadIdx.x < 16) o = threadIdx.x < head ? threadIdx.x : out_len;
  else if (threadIdx.x < 32) o = tail_at + (threadIdx.x - 16);
  else return;
  if (o >= out_len) return;
  const OrRec c = p.rec(fl_record_of(p.dst, 0, p.norfs - 1, o));
  out[o] = or_byte(p, c, o - c.at, s_tab);
}

// ------------------------------------------------------------------------------------------ host side
struct OrCall {
  mk_orf_opt_t opt;
  OrRule rule;
  bool start;
  FlEmit emit;         // where the output goes
  mk_orf_row_t* rows;  // the caller's, or nullptr; cap of them
  size_t cap;
  bool device;         // out / rows are device memory
  size_t orfs_seen = 0;
  MkDevBuf meta, orfs, scan_tmp;
  MkTimed find, place;
  mk_orf_t st{};
  OrCall(mk_ctx* c, const mk_orf_opt_t& o, uint8_t* out, size_t oc, mk_orf_row_t* rw, size_t cp, bool dev)
      : opt(o), emit(c, out, oc, dev), rows(rw), cap(cp), device(dev), find(c), place(c) {
    rule.min_nt = 3ull * o.min_aa;
    rule.strands = (o.flags & MK_ORF_PLUS) ? 1u : (o.flags & MK_ORF_MINUS) ? 2u : 3u;
    rule.alt = (o.flags & MK_ORF_ALT) ? 1u : 0u;
    start = (o.flags & MK_ORF_START) != 0;
  }
  ~OrCall() {
    for (MkDevBuf* b : {&meta, &orfs, &scan_tmp}) buf_free(*b);
  }
};

template <class F>
static void or_mode(bool start, F&& f) {
  if (start) f(std::true_type{});
  else f(std::false_type{});
}

// What follows sc_piece (parse and record scan only) for a piece of n bytes whose records start at record `first` of the
// call.  The stream is idle afterwards.
static int or_piece(ScCall& s, OrCall& f, size_t n, size_t first) {
  mk_ctx* c = s.c;
  int rc;
  const size_t nrows = s.last.nrows;
  f.st.pieces += 1;
  if (!nrows) {  // (no header line, no kept character)
    f.st.preamble += n;
    return MK_OK;
  }
  const uint8_t* text = s.last.text;
  const uint8_t* seq = (const uint8_t*)c->seq.p;
  const size_t seq_len = s.last.seq_len;
  const int headless = s.last.headless ? 1 : 0;
  const size_t ftiles = div_up(n, FL_SPAN), otiles = div_up(seq_len + 1, OR_SPAN);
  f.st.bases += seq_len - (nrows - headless);
  // meta: OrStatus (128) | start[nrows + 1] | nsrc, nlen, reclen [nrows] each | ftile_pre[ftiles] | otile_pre[otiles] |
  //       tsum, carry [otiles * OR_NV] each | ftile_cnt[ftiles] | otile_cnt[otiles] | lane_cnt[otiles * 256]
  static_assert(sizeof(OrStatus) <= 128, "OrStatus");
  const size_t words = (nrows + 1) + 3 * nrows + ftiles + otiles + 2 * otiles * OR_NV;
  if ((rc = mk_buf_reserve(c, f.meta, 128 + words * sizeof(u64) + (ftiles + otiles + otiles * 256) * sizeof(unsigned))) != MK_OK) return rc;
  OrStatus* d_st = (OrStatus*)f.meta.p;
  u64* start = (u64*)((char*)f.meta.p + 128);
  u64* nsrc = start + nrows + 1;
  u64* nlen = nsrc + nrows;
  u64* reclen = nlen + nrows;
  u64* ftile_pre = reclen + nrows;
  u64* otile_pre = ftile_pre + ftiles;
  u64* tsum = otile_pre + otiles;
  u64* carry = tsum + otiles * OR_NV;
  unsigned* ftile_cnt = (unsigned*)(carry + otiles * OR_NV);
  unsigned* otile_cnt = ftile_cnt + ftiles;
  unsigned* lane_cnt = otile_cnt + otiles;

  MK_HIP(hipMemsetAsync(d_st, 0, sizeof(OrStatus), c->stream));
  MK_HIP(hipMemsetAsync(start, 0xFF, (nrows + 1) * sizeof(u64), c->stream));  // (a start no header line gives reads as outside the text)
  MK_HIP(hipMemsetAsync(reclen, 0, nrows * sizeof(u64), c->stream));
  OrRowSink sink{nullptr, nullptr, reclen, 0, 0, 0, (u64)nrows, s.last.row_base, (u64)first};
  if ((rc = f.find.begin()) != MK_OK) return rc;
  or_mode(f.start, [&](auto st) {
    constexpr bool START = decltype(st)::value;
    hipLaunchKernelGGL((or_tiles_k<START>), dim3((unsigned)otiles), dim3(256), 0, c->stream, seq, (u64)seq_len, f.rule, tsum);
    hipLaunchKernelGGL((or_carry_k<START>), dim3(1), dim3(256), 0, c->stream, (const u64*)tsum, otiles, carry);
    hipLaunchKernelGGL((or_emit_k<START, false>), dim3((unsigned)otiles), dim3(256), 0, c->stream, seq, (u64)seq_len, f.rule,
                       (const u64*)carry, lane_cnt, otile_cnt, (const u64*)otile_pre, sink);
  });
  hipLaunchKernelGGL(or_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)otile_cnt, otiles, otile_pre, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.find.end()) != MK_OK) return rc;
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fl_tiles_k, dim3((unsigned)ftiles), dim3(256), 0, c->stream, text, (u64)n, ftile_cnt);
  hipLaunchKernelGGL(fl_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)ftile_cnt, ftiles, ftile_pre, (u64)n, nrows, headless,
                     start, &d_st->fl);
  hipLaunchKernelGGL(fl_starts_k, dim3((unsigned)ftiles), dim3(256), 0, c->stream, text, (u64)n, (const u64*)ftile_pre, (u64)headless,
                     nrows, start);
  hipLaunchKernelGGL(or_name_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, text, (u64)n, (const u64*)start, nrows,
                     headless, nsrc, nlen);
  MK_HIP(hipGetLastError());
  if ((rc = f.place.end()) != MK_OK) return rc;
  OrStatus h{};
  u64 start0 = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&start0, start, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.find.add_to(f.st.s_find)) != MK_OK || (rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (h.fl.headers + headless != nrows) {
    c->err = std::string(s.what) + ": " + std::to_string(h.fl.headers) + " header lines in the text, " +
             std::to_string(nrows - headless) + " in the parsed stream (internal error)";
    return MK_ERR_STATE;
  }
  f.st.preamble += start0 > n ? n : start0;
  const size_t norfs = (size_t)h.norfs;
  // (a stretch holds 3 stream bytes a codon, and the stretches of one strand and residue are disjoint)
  if (norfs > 2 * (seq_len + 1)) {
    c->err = std::string(s.what) + ": more ORFs than closings in a piece (internal error)";
    return MK_ERR_STATE;
  }
  const size_t at_orf = f.orfs_seen;
  f.orfs_seen += norfs;
  if (!norfs) return MK_OK;

  // orfs: rows[norfs] | src, rank [norfs] each | len, dst [norfs + 1] each
  if ((rc = mk_buf_reserve(c, f.orfs, norfs * sizeof(mk_orf_row_t) + (4 * norfs + 2) * sizeof(u64))) != MK_OK) return rc;
  mk_orf_row_t* d_rows = (mk_orf_row_t*)f.orfs.p;
  u64* src = (u64*)(d_rows + norfs);
  u64* rank = src + norfs;
  u64* len = rank + norfs;
  u64* dst = len + norfs + 1;
  size_t tmp = 0;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, norfs + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;
  sink.rows = d_rows;
  sink.src = src;
  sink.norfs = norfs;
  if ((rc = f.find.begin()) != MK_OK) return rc;
  or_mode(f.start, [&](auto st) {
    constexpr bool START = decltype(st)::value;
    hipLaunchKernelGGL((or_emit_k<START, true>), dim3((unsigned)otiles), dim3(256), 0, c->stream, seq, (u64)seq_len, f.rule,
                       (const u64*)carry, lane_cnt, otile_cnt, (const u64*)otile_pre, sink);
  });
  MK_HIP(hipGetLastError());
  if ((rc = f.find.end()) != MK_OK) return rc;
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(or_len_k, dim3(grid_for(norfs + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, norfs, (u64)first,
                     (const u64*)reclen, (const u64*)nlen, nrows, rank, len, d_st);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, norfs + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = f.place.end()) != MK_OK) return rc;
  u64 piece_out = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + norfs, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.find.add_to(f.st.s_find)) != MK_OK || (rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  // (no address is made of the lengths before they have passed: every ORF accounted for, no more residues than the six
  // frames of the stream hold, no more name bytes than header text a record)
  if (piece_out != h.sumlen || h.residues > 2 * (u64)seq_len || h.names > (u64)norfs * n ||
      h.sumlen > h.names + h.residues + (u64)norfs * (7 + 20 + 20)) {
    c->err = std::string(s.what) + ": the lengths of a piece's ORFs do not add up (internal error)";
    return MK_ERR_STATE;
  }
  f.st.orfs += norfs;
  f.st.residues += h.residues;
  if (h.longest > f.st.longest) f.st.longest = h.longest;
  for (int i = 0; i < 6; ++i) f.st.per_frame[i] += h.per_frame[i];

  if (f.rows && at_orf + norfs <= f.cap) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(f.rows + at_orf, d_rows, norfs * sizeof(mk_orf_row_t), f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }

  // the gather: fl_emit's shape with this file's kernels
  FlEmit& e = f.emit;
  const size_t at = e.bytes_out;
  e.bytes_out += (size_t)piece_out;
  if (!piece_out || e.bytes_out > e.out_cap) return MK_OK;
  uint8_t* d_out = e.out + at;
  if (!e.device) {
    if ((rc = mk_buf_reserve(c, e.stage, (size_t)piece_out)) != MK_OK) return rc;
    d_out = (uint8_t*)e.stage.p;
  }
  const OrPlace p{text, (u64)n, seq, (u64)seq_len, d_rows, src, rank, nsrc, nlen, dst, norfs, (u64)first};
  const u64 head = std::min<u64>((16 - ((uintptr_t)d_out & 15)) & 15, piece_out);
  const u64 nbody = (piece_out - head) / 16, tail_at = head + 16 * nbody;
  if ((rc = e.gather.begin()) != MK_OK) return rc;
  if (nbody)
    hipLaunchKernelGGL(or_gather_k, dim3((unsigned)div_up((size_t)nbody, 256 * OR_CHUNKS)), dim3(256), 0, c->stream, p, head, nbody, d_out);
  if (head || tail_at < piece_out) hipLaunchKernelGGL(or_edges_k, dim3(1), dim3(64), 0, c->stream, p, head, tail_at, piece_out, d_out);
  MK_HIP(hipGetLastError());
  if ((rc = e.gather.end()) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = e.gather.add_to(f.st.s_emit)) != MK_OK) return rc;
  if (!e.device) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(e.out + at, d_out, (size_t)piece_out, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }
  return MK_OK;
}

// sc_piece with room for no rows -- parse and record scan, no probe -- then or_piece.
static int or_both(ScCall& s, OrCall& f, const uint8_t* d_piece, size_t len) {
  const size_t first = s.rows_seen;
  const int rc = sc_piece(s, d_piece, len, nullptr, 0, nullptr, nullptr);
  return rc != MK_OK ? rc : or_piece(s, f, len, first);
}

// How both calls check their own arguments, open as the screen calls open, and end; body(s): the pieces.
template <class Body>
static int or_run(mk_ctx* c, const char* what, const mk_orf_opt_t* opt, OrCall* f, size_t* out_len, size_t* norfs, mk_orf_t* st,
                  Body&& body) {
  if (!opt) { c->err = std::string(what) + ": opt is NULL"; return MK_ERR_ARG; }
  if (opt->min_aa < 1) { c->err = std::string(what) + ": min_aa must be 1 or more"; return MK_ERR_ARG; }
  if (opt->flags & ~(MK_ORF_START | MK_ORF_ALT | MK_ORF_PLUS | MK_ORF_MINUS)) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  if ((opt->flags & MK_ORF_ALT) && !(opt->flags & MK_ORF_START)) {
    c->err = std::string(what) + ": MK_ORF_ALT needs MK_ORF_START";
    return MK_ERR_ARG;
  }
  if ((opt->flags & MK_ORF_PLUS) && (opt->flags & MK_ORF_MINUS)) {
    c->err = std::string(what) + ": MK_ORF_PLUS and MK_ORF_MINUS contradict each other";
    return MK_ERR_ARG;
  }
  mk_screen_t sc{};
  const int rc = sc_run(c, what, 0, 1, ~(size_t)0, nullptr, &sc, [&](ScCall& s) { return body(s); });
  if (rc != MK_OK) return rc;
  if (out_len) *out_len = f->emit.bytes_out;
  if (norfs) *norfs = f->orfs_seen;
  if (f->emit.bytes_out > f->emit.out_cap || (f->rows && f->orfs_seen > f->cap)) {
    c->err = std::string(what) + ": the output holds " + std::to_string(f->emit.bytes_out) + " bytes and " + std::to_string(f->orfs_seen) +
             " ORFs, out has room for " + std::to_string(f->emit.out_cap) + ", rows for " + std::to_string(f->cap);
    return MK_ERR_RANGE;
  }
  f->st.bytes = sc.bytes;
  f->st.records = sc.records;
  f->st.headless = sc.headless;
  f->st.bytes_out = f->emit.bytes_out;
  f->st.s_read = sc.s_read;
  f->st.s_parse = sc.s_parse;
  f->st.s_total = sc.s_total;
  if (st) *st = f->st;
  return MK_OK;
}

extern "C" int mk_orf_device(mk_ctx* c, const uint8_t* d_text, size_t n, const mk_orf_opt_t* opt, uint8_t* d_out, size_t out_cap,
                             size_t* out_len, mk_orf_row_t* d_rows, size_t cap, size_t* norfs, mk_orf_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_text) || (out_cap && !d_out)) { c->err = "mk_orf_device: NULL buffer"; return MK_ERR_ARG; }
  if ((uintptr_t)d_rows & 7) { c->err = "mk_orf_device: rows must be aligned to 8"; return MK_ERR_ARG; }
  OrCall f(c, opt ? *opt : mk_orf_opt_t{}, d_out, out_cap, d_rows, cap, true);
  return or_run(c, "mk_orf_device", opt, &f, out_len, norfs, st, [&](ScCall& s) -> int { return n ? or_both(s, f, d_text, n) : MK_OK; });
}

extern "C" int mk_orf_text(mk_ctx* c, const uint8_t* text, size_t n, size_t piece_bytes, const mk_orf_opt_t* opt, uint8_t* out,
                           size_t out_cap, size_t* out_len, mk_orf_row_t* rows, size_t cap, size_t* norfs, mk_orf_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !text) || (out_cap && !out)) { c->err = "mk_orf_text: NULL buffer"; return MK_ERR_ARG; }
  OrCall f(c, opt ? *opt : mk_orf_opt_t{}, out, out_cap, rows, cap, false);
  return or_run(c, "mk_orf_text", opt, &f, out_len, norfs, st, [&](ScCall& s) -> int {
    return sc_text_pieces(s, text, n, piece_bytes, [&](const uint8_t* d_piece, size_t len) -> int { return or_both(s, f, d_piece, len); });
  });
}
