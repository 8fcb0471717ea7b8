// mk_overlap.hip -- mate-overlap detection in the pairs of an interleaved FASTQ text (mk_fastq_overlap_text /
// mk_fastq_overlap_device; include/mercat_hip.h has the rule): mate 1 against the reverse complement of mate 2 at every
// offset, the first admissible one in the rule's order giving the fragment length; the pairs then cut to the fragment
// (mode 0) or merged into one read with a consensus over the overlap (mode 1), the survivors gathered as FASTQ -- on the
// GPU, by mk_qtrim.hip's scheme (mk_fqpiece.h has the shared parts):
//   fs_index_open / fs_index_lines<false>        the line index (mk_fqindex.h), unchanged.
//   ov_scan_k     a wave (a workgroup of one) a pair, a lane a candidate offset, 64 candidates a block in the rule's order.
//                 All 64 lanes load: lanes 0 .. 31 the first 32 aligned 16-byte granules of mate 1's sequence line, lanes
//                 32 .. 63 those of mate 2's (QtLine: fs_load); lanes 31 and 63 also load the 33rd granule, which holds
//                 bytes of a line only where that line is long and starts late in its granule.  Every lane packs its 16
//                 bytes word-wide -- four bytes a step, no byte loop -- into 32 bits of 2-bit codes and 32 bits of an
//                 "other" plane (a byte that is not ACGT after folding), takes its right-hand neighbour's pack (one
//                 shuffle a plane) and funnel-shifts the two into the 16 bases of the CONTENT that start at base 16 k: the
//                 packed lines no longer know the address of the text.  Mate 1 goes to LDS as it is, sixteen 64-bit words
//                 a plane; mate 2 goes there reversed and complemented, placed from the top of a 512-base frame (chunk k
//                 complemented, its 2-bit groups reversed, stored as chunk 31 - k), so that rc[j] is base j + 512 - L2 of
//                 the frame whatever L2 is.  The words live in LDS and not across lanes because every lane reads mate 2
//                 at a word index of its own (its offset / 32): that is an indexed LDS read, where registers across lanes
//                 would need a ds_bpermute a word and plane (which runs on the LDS hardware as well) -- and mate 1's
//                 word is the same for all lanes, an LDS broadcast.  512 bytes a workgroup.
//                 The compare, 32 bases a step over the words the block's overlaps touch (wave-uniform bounds): each lane
//                 funnel-shifts two neighbouring words of mate 2 by its offset % 32, x = mate 1 ^ mate 2,
//                 popcount((x | x >> 1 | other1 | other2) & EVEN & avail), avail being the lane's overlap in that word.
//                 Ballot and find-first pick the first admissible lane; the pair stops at the first block that has one.
//                 No loop trusts a byte of the text: all bounds come from line[].
//   ov_decide_k   a lane a record: the checks, keep[r], the counters, and the record's four segment slots -- a pair has
//                 eight; a merged pair uses six (header 1, s1[:min(L1, F)], the tail and '\n', '+' line 1, and the same
//                 two of the qualities), the first four in mate 1's slots, the other two in mate 2's.
//   ov_merge_k    the merge writer, mode 1 / which 1 only: a wave a merged pair, a lane a base.  The gather copies bytes of
//                 the text, and a merged record needs bytes the text does not hold; so they are written INTO the text, in
//                 the call's own copy of the piece (c->raw; the device call copies its text there first): the consensus
//                 over mate 1's overlap positions in place, and rc[L1 - d ..] / rq[L1 - d ..] -- the F - L1 bases past
//                 mate 1's end -- over the front of mate 2's sequence and quality lines, which is the reverse
//                 (complement) of those very bytes: a lane swaps positions i and T - 1 - i, and the overlap reads only
//                 mate 2's bytes from T on, so no lane reads what another writes.  It runs behind ov_decide_k: nothing
//                 reads the record checks (qt_record) again after it.
//   rocprim::exclusive_scan, fs_gather_k / fs_edges_k   as in mk_qtrim.hip, through fq_piece.
#include "mk_fqpiece.h"

#define OV_NONE 0xFFFFFFFFull
#define OV_MAX MK_OVERLAP_MAX_BASES
#define OV_WORDS (OV_MAX / 32u)  // 64-bit words a plane
#define OV_EVEN 0x5555555555555555ull
#define OV_BLOCK 64u  // candidate offsets a block: a lane each
static_assert(OV_MAX == 512, "ov_scan_k loads 32 (+ 1) granules a line with half a wave: 512 bases");

struct OvStatus {  // device memory, behind the FsStatus of the piece
  u64 pairs, pairs_hit, pairs_merged, pairs_trimmed, dropped_short, skipped_long, bases_in;
};
struct OvOpt {
  unsigned mode, min_overlap, max_mismatch, max_err_ppm, min_len, which;
};
enum { OV_MISS = 0, OV_HIT = 1, OV_LONG = 2, OV_FAILED = 5 };

// 0x80 in every byte of f that equals ch (exact: no carries between bytes)
__device__ __forceinline__ unsigned ov_eq4(unsigned f, unsigned ch) {
  const unsigned x = f ^ (ch * 0x01010101u);
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
// the 2-bit groups at bits 0, 8, 16, 24 of x (nothing else set) as bits 0 .. 7
__device__ __forceinline__ unsigned ov_squeeze(unsigned x) { return (x | (x >> 6) | (x >> 12) | (x >> 18)) & 0xFFu; }

// The 16 bytes of a granule as 2-bit codes (A 0, C 1, G 2, T 3; lower case folded) and the other plane: bit 2b set for
// a byte b that is none of them.  Four bytes a step.
__device__ __forceinline__ void ov_pack16(const FsSeg& c, unsigned& codes, unsigned& other) {
  codes = 0;
  other = 0;
#pragma unroll
  for (unsigned k = 0; k < 4; ++k) {
    const unsigned f = c.w[k] & 0xDFDFDFDFu;  // (only X and X | 0x20 fold to X)
    const unsigned acgt = ov_eq4(f, 'A') | ov_eq4(f, 'C') | ov_eq4(f, 'G') | ov_eq4(f, 'T');
    codes |= ov_squeeze(((f >> 1) ^ (f >> 2)) & 0x03030303u) << (8 * k);
    other |= ov_squeeze((~acgt & 0x80808080u) >> 7) << (8 * k);
  }
}
// the sixteen 2-bit groups of x in reverse order
__device__ __forceinline__ unsigned ov_rev2(unsigned x) {
  const unsigned y = __brev(x);
  return ((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1);
}
// bits 0 .. 2t - 1, t = 0 .. 32
__device__ __forceinline__ u64 ov_below(int t) { return t >= 32 ? ~0ull : t <= 0 ? 0ull : (1ull << (2 * t)) - 1; }

// rows[5 r ..]: length, kept, fragment, overlap, mismatches; verdict[r]: OV_HIT, OV_MISS, OV_LONG (the pair was not tested:
// a mate above OV_MAX bases), or OV_FAILED for a record that fails a check (ov_decide_k names it).  Pair p is records 2p
// and 2p + 1: pieces start at even records.  A last record without a mate (the call then fails: an odd count) has no hit.
static __global__ void __launch_bounds__(64) ov_scan_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ line, size_t nrec,
                                                       OvOpt o, u64* __restrict__ rows, uint8_t* __restrict__ verdict) {
  __shared__ u64 s_c1[OV_WORDS], s_o1[OV_WORDS], s_cr[OV_WORDS], s_or[OV_WORDS];
  const unsigned lane = threadIdx.x;
  const size_t npairs = (nrec + 1) / 2;
  for (size_t p = blockIdx.x; p < npairs; p += gridDim.x) {
    const bool lone = 2 * p + 1 >= nrec;
    const QtRecord ra = qt_record(text, line, 2 * p);
    const QtRecord rb = lone ? ra : qt_record(text, line, 2 * p + 1);
    const u64 L1 = ra.fail < 0 ? ra.ls : 0, L2 = !lone && rb.fail < 0 ? rb.ls : 0;
    const bool whole = ra.fail < 0 && !lone && rb.fail < 0;
    const bool too_long = whole && (L1 > OV_MAX || L2 > OV_MAX);
    u64 frag = OV_NONE;
    unsigned hit_ov = 0, hit_mm = 0;
    __syncthreads();  // (the workgroup is this wave: the pair before has been read)
    if (whole && !too_long && L1 >= o.min_overlap && L2 >= o.min_overlap) {
      const unsigned half = lane >> 5, k = lane & 31u;
      const QtLine sl{half ? rb.l1 : ra.l1, half ? L2 : L1};
      const unsigned sh16 = 2 * (unsigned)(sl.a & 15);
      unsigned cw, ow, ce = 0, oe = 0;
      ov_pack16(sl.load(text, n, k >> 4, k & 15u), cw, ow);
      if (k == 31) ov_pack16(sl.load(text, n, 2, 0), ce, oe);
      unsigned cn = (unsigned)__shfl_down((int)cw, 1), on = (unsigned)__shfl_down((int)ow, 1);
      if (k == 31) {
        cn = ce;
        on = oe;
      }
      const unsigned cc = __funnelshift_r(cw, cn, sh16), oc = __funnelshift_r(ow, on, sh16);  // content bases 16 k .. 16 k + 15
      if (half) {
        ((unsigned*)s_cr)[31 - k] = ov_rev2(~cc);
        ((unsigned*)s_or)[31 - k] = ov_rev2(oc);
      } else {
        ((unsigned*)s_c1)[k] = cc;
        ((unsigned*)s_o1)[k] = oc;
      }
      __syncthreads();
      const int l1 = (int)L1, l2 = (int)L2, mo = (int)o.min_overlap;
      const unsigned P = (unsigned)(l1 - mo + 1), total = P + (unsigned)(l2 - mo);  // offsets 0 .. P - 1, then -1 .. -(L2 - mo)
      for (unsigned c0 = 0; c0 < total && frag == OV_NONE; c0 += OV_BLOCK) {
        const unsigned c = c0 + lane, c1 = c0 + OV_BLOCK - 1 < total ? c0 + OV_BLOCK - 1 : total - 1;
        const bool valid = c < total;
        const int d = !valid ? 0 : c < P ? (int)c : -(int)(c - P + 1);
        const int a0 = d > 0 ? d : 0, e0 = d + l2 < l1 ? d + l2 : l1;  // the overlap, in mate 1's positions
        // the words the block's overlaps touch
        int lo = 0, hi = l1;
        if (c1 < P) {
          lo = (int)c0;
          hi = (int)c1 + l2 < l1 ? (int)c1 + l2 : l1;
        } else if (c0 >= P) {
          const int f0 = l2 - (int)(c0 - P + 1);
          hi = f0 < l1 ? f0 : l1;
        }
        const int sft = (int)OV_MAX - l2 - d;  // rc[pos - d] is base pos + sft of mate 2's frame
        const int wofs = sft >> 5;
        const unsigned sh = 2 * (unsigned)(sft & 31);
        unsigned mm = 0;
        for (int w = lo >> 5; w < (hi + 31) >> 5; ++w) {
          const int wi = w + wofs;
          const bool in0 = wi >= 0 && wi < (int)OV_WORDS, in1 = wi + 1 >= 0 && wi + 1 < (int)OV_WORDS;
          const int i0 = in0 ? wi : 0, i1 = in1 ? wi + 1 : 0;
          const u64 c_lo = in0 ? s_cr[i0] : 0ull, c_hi = in1 ? s_cr[i1] : 0ull;
          const u64 o_lo = in0 ? s_or[i0] : 0ull, o_hi = in1 ? s_or[i1] : 0ull;
          const u64 xc = sh ? (c_lo >> sh) | (c_hi << (64 - sh)) : c_lo;
          const u64 xo = sh ? (o_lo >> sh) | (o_hi << (64 - sh)) : o_lo;
          const u64 avail = ov_below(e0 - 32 * w) & ~ov_below(a0 - 32 * w) & OV_EVEN;
          const u64 x = s_c1[w] ^ xc;
          mm += (unsigned)__popcll((x | (x >> 1) | s_o1[w] | xo) & avail);
        }
        const unsigned ov = (unsigned)(e0 - a0);
        const bool adm = valid && mm <= o.max_mismatch && (u64)mm * 1000000ull <= (u64)o.max_err_ppm * ov;
        const u64 got = __ballot(adm);
        if (got) {
          const int src = __ffsll((unsigned long long)got) - 1;
          frag = (u64)(__shfl(d, src) + l2);
          hit_ov = (unsigned)__shfl((int)ov, src);
          hit_mm = (unsigned)__shfl((int)mm, src);
        }
      }
    }
    const bool hit = frag != OV_NONE;
    // lanes 0 .. 4: the row of mate 1; lanes 8 .. 12: that of mate 2
    const unsigned col = lane & 7u;
    const u64 L = lane < 8 ? L1 : L2;
    const u64 mine = col == 0 ? L : col == 1 ? (hit && frag < L ? frag : L) : col == 2 ? frag : col == 3 ? (u64)hit_ov : (u64)hit_mm;
    const unsigned v = hit ? OV_HIT : too_long ? OV_LONG : OV_MISS;
    if (lane < 5) rows[5 * (2 * p) + col] = mine;
    if (lane == 5) verdict[2 * p] = (uint8_t)(ra.fail < 0 ? v : OV_FAILED);
    if (!lone) {
      if (lane >= 8 && lane < 13) rows[5 * (2 * p + 1) + col] = mine;
      if (lane == 13) verdict[2 * p + 1] = (uint8_t)(rb.fail < 0 ? v : OV_FAILED);
    }
  }
}

// A lane per record (and one for the slot behind the last segment).  Record r is lines 4r .. 4r + 3; its segments are
// 4r .. 4r + 3.  The lane of a first mate counts its pair.
static __global__ void __launch_bounds__(256) ov_decide_k(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t nrec, OvOpt o,
                                                          const u64* __restrict__ rows, const uint8_t* __restrict__ verdict,
                                                          uint8_t* __restrict__ keep, u64* __restrict__ seg_src, u64* __restrict__ len,
                                                          FsStatus* __restrict__ st, OvStatus* __restrict__ os) {
  u64 n_out = 0, n_trimmed = 0, n_bases = 0, n_in = 0, n_pairs = 0, n_hit = 0, n_merged = 0, n_ptrim = 0, n_short = 0, n_long = 0;
  const u64 floor_len = o.min_len > 1u ? o.min_len : 1u;
  mk_for_each(nrec + 1, [&](size_t r) {
    if (r == nrec) {
      seg_src[4 * nrec] = 0;
      len[4 * nrec] = 0;
      return;
    }
    const QtRecord q = qt_record(text, line, r);
    if (q.fail >= 0) atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | (unsigned)q.fail));
    const size_t r1 = r & ~(size_t)1, r2 = r1 + 1;
    const bool first = r == r1, mated = r2 < nrec;
    const unsigned v = verdict[r];
    const bool hit = v == OV_HIT;  // (then both mates passed their checks)
    const u64 L = rows[5 * r], kept = rows[5 * r + 1], F = rows[5 * r + 2];
    const bool is_short = hit && F < floor_len;
    const unsigned k = o.mode == 0 ? (is_short ? 0u : 1u) : hit ? (is_short ? 0u : 1u) : 2u;
    keep[r] = (uint8_t)k;
    n_in += q.fail < 0 ? L : 0;
    if (first && mated) {
      n_pairs += 1;
      n_hit += hit;
      n_short += is_short;
      n_long += v == OV_LONG;
      n_merged += o.mode == 1 && hit && !is_short;
      n_ptrim += o.mode == 0 && hit && !is_short && (kept < L || rows[5 * r2 + 1] < rows[5 * r2]);
    }
    u64 s[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    if (q.fail < 0 && k == o.which) {
      if (o.mode == 1 && k == 1) {  // a merged pair: six of the pair's eight slots
        const QtRecord qa = first ? q : qt_record(text, line, r1), qb = first ? qt_record(text, line, r2) : q;
        const u64 L1 = rows[5 * r1], m1 = F < L1 ? F : L1, T = F - m1;  // T: the bases past mate 1's end
        const u64 at1 = first ? qa.l1 : qa.l3, at2 = first ? qb.l1 : qb.l3;
        const unsigned i = first ? 1 : 0;
        if (first) {
          s[0] = qa.l0;
          m[0] = qa.l1 - qa.l0;
          s[3] = qa.l2;
          m[3] = qa.l3 - qa.l2;
          n_out += 1;
          n_trimmed += 1;
          n_bases += F;
        }
        s[i] = T ? at1 : (at1 | FS_FORCE);
        m[i] = T ? L1 : m1 + 1;
        s[i + 1] = T ? (at2 | FS_FORCE) : 0;
        m[i + 1] = T ? T + 1 : 0;
      } else {
        const u64 out_len = o.mode == 0 ? kept : L;
        n_trimmed += fq_segments(q, L, 0, out_len, s, m) ? 1 : 0;
        n_out += 1;
        n_bases += out_len;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      seg_src[4 * r + i] = s[i];
      len[4 * r + i] = m[i];
    }
  });
  block_add(&st->records_out, n_out);
  block_add(&st->records_trimmed, n_trimmed);
  block_add(&st->bases_out, n_bases);
  block_add(&os->bases_in, n_in);
  block_add(&os->pairs, n_pairs);
  block_add(&os->pairs_hit, n_hit);
  block_add(&os->pairs_merged, n_merged);
  block_add(&os->pairs_trimmed, n_ptrim);
  block_add(&os->dropped_short, n_short);
  block_add(&os->skipped_long, n_long);
}

__device__ __forceinline__ unsigned ov_fold(unsigned b) { return b >= 'a' && b <= 'z' ? b - 32u : b; }
__device__ __forceinline__ bool ov_acgt(unsigned f) { return f == 'A' || f == 'C' || f == 'G' || f == 'T'; }
__device__ __forceinline__ unsigned ov_comp(unsigned b) {
  const unsigned f = ov_fold(b);
  return f == 'A' ? 'T' : f == 'C' ? 'G' : f == 'G' ? 'C' : f == 'T' ? 'A' : 'N';
}

// The merge writer (above).  text is the call's own copy of the piece: no __restrict__, it is read and written.
static __global__ void __launch_bounds__(256) ov_merge_k(uint8_t* text, const u64* __restrict__ line, size_t nrec, OvOpt o,
                                                         const u64* __restrict__ rows, const uint8_t* __restrict__ verdict) {
  const unsigned lane = threadIdx.x & 63u;
  const size_t npairs = nrec / 2, per_grid = (size_t)gridDim.x * 4;
  const u64 floor_len = o.min_len > 1u ? o.min_len : 1u;
  for (size_t p = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < npairs; p += per_grid) {
    if (verdict[2 * p] != OV_HIT || verdict[2 * p + 1] != OV_HIT) continue;
    const u64 L1 = rows[10 * p], L2 = rows[10 * p + 5], F = rows[10 * p + 2];
    if (F < floor_len || L1 > OV_MAX || L2 > OV_MAX || F > L1 + L2 || F < 1) continue;  // (a hit has 1 <= F <= L1 + L2 - 1)
    const u64 a1 = line[8 * p + 1], q1 = line[8 * p + 3], a2 = line[8 * p + 5], q2 = line[8 * p + 7];
    const long long d = (long long)F - (long long)L2;
    const u64 lo = d > 0 ? (u64)d : 0, hi = F < L1 ? F : L1, T = F - hi;
    for (u64 pos = lo + lane; pos < hi; pos += 64) {
      const u64 j = F - 1 - pos;  // rc[pos - d] is the complement of s2[L2 - 1 - (pos - d)]; j >= T
      const unsigned b1 = text[a1 + pos], y1 = text[q1 + pos], y2 = text[q2 + j];
      const unsigned f1 = ov_fold(b1), b2 = ov_comp(text[a2 + j]);
      const bool ok1 = ov_acgt(f1), ok2 = ov_acgt(b2);
      unsigned base = b1, qual = y1;
      if (ok1 && ok2 && f1 == b2) {
        qual = y1 > y2 ? y1 : y2;
      } else if (ok1 != ok2 ? ok2 : y2 > y1) {
        base = b2;
        qual = y2;
      }
      text[a1 + pos] = (uint8_t)base;
      text[q1 + pos] = (uint8_t)qual;
    }
    for (u64 i = lane; 2 * i < T; i += 64) {  // the front T bytes of mate 2's lines, reversed (and complemented) in place
      const u64 j = T - 1 - i;
      const unsigned x = text[a2 + i], y = text[a2 + j], qx = text[q2 + i], qy = text[q2 + j];
      text[a2 + i] = (uint8_t)ov_comp(y);
      text[a2 + j] = (uint8_t)ov_comp(x);
      text[q2 + i] = (uint8_t)qy;
      text[q2 + j] = (uint8_t)qx;
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
// What mk_fqpiece.h's piece loop asks of a call.
struct OvPolicy {
  typedef OvOpt Opt;
  typedef OvStatus Status;
  typedef mk_fastq_overlap_t Stats;
  struct Side {};
  static constexpr size_t ROW = 5;
  static bool paired(const OvOpt&) { return true; }
  static bool merges(const OvOpt& o) { return o.mode == 1 && o.which == 1; }
  static const char* kind(unsigned k) { return fs_kind(k); }
  static void scan(FqCall<OvPolicy>& f, const uint8_t* d_text, size_t n, const u64* line, size_t nrec, u64* d_rows, uint8_t* d_verdict,
                   FsStatus*) {
    hipLaunchKernelGGL(ov_scan_k, dim3(grid_for((nrec + 1) / 2, 1, 1u << 16)), dim3(64), 0, f.c->stream, d_text, (u64)n, line, nrec, f.o, d_rows,
                       d_verdict);
  }
  static void decide(FqCall<OvPolicy>& f, const uint8_t* d_text, const u64* line, size_t nrec, const u64* d_rows, const uint8_t* d_verdict,
                     uint8_t* d_keep, u64* seg_src, u64* len, FsStatus* d_st, OvStatus* d_os) {
    hipLaunchKernelGGL(ov_decide_k, dim3(grid_for(nrec + 1, 256, 4096)), dim3(256), 0, f.c->stream, d_text, line, nrec, f.o, d_rows,
                       d_verdict, d_keep, seg_src, len, d_st, d_os);
    // (a merging call's text is its own copy: both bodies see to that)
    if (merges(f.o) && f.own == d_text && nrec >= 2)
      hipLaunchKernelGGL(ov_merge_k, dim3(grid_for(nrec / 2, 4, 1u << 14)), dim3(256), 0, f.c->stream, f.own, line, nrec, f.o, d_rows, d_verdict);
  }
  static void add(mk_fastq_overlap_t& st, const OvStatus& q) {
    st.pairs += q.pairs;
    st.pairs_hit += q.pairs_hit;
    st.pairs_merged += q.pairs_merged;
    st.pairs_trimmed += q.pairs_trimmed;
    st.dropped_short += q.dropped_short;
    st.skipped_long += q.skipped_long;
    st.bases_in += q.bases_in;
  }
};
typedef FqCall<OvPolicy> OvCall;

// The options as the kernels take them, or the message of the first one out of range.
static const char* ov_options(const mk_overlap_opt_t* opt, OvOpt& o) {
  if (!opt) return "opt is NULL";
  if (opt->mode > 1) return "mode must be 0 (trim) or 1 (merge)";
  if (opt->min_overlap < 1 || opt->min_overlap > OV_MAX) return "min_overlap must be 1 .. 512";
  if (opt->max_err_ppm > 1000000) return "max_err_ppm must be 0 .. 1000000";
  if (opt->which != 1 && !(opt->which == 2 && opt->mode == 1)) return "which must be 1 (the main output) or, with mode 1, 2 (the unmerged pairs)";
  o.mode = opt->mode;
  o.min_overlap = opt->min_overlap;
  o.max_mismatch = opt->max_mismatch;
  o.max_err_ppm = opt->max_err_ppm;
  o.min_len = opt->min_len;
  o.which = opt->which;
  return nullptr;
}

template <class Body>
static int ov_run(OvCall& f, size_t* out_len, size_t* nrec, mk_fastq_overlap_t* st, Body&& body) {
  return fq_run(f, out_len, nrec, st, []() -> int { return MK_OK; }, body, []() -> int { return MK_OK; });
}

extern "C" int mk_fastq_overlap_device(mk_ctx* c, const uint8_t* d_fastq, size_t n, const mk_overlap_opt_t* opt, size_t cap, uint8_t* d_keep,
                                       uint64_t* d_rows, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec,
                                       mk_fastq_overlap_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_fastq) || (out_cap && !d_out)) { c->err = "mk_fastq_overlap_device: NULL buffer"; return MK_ERR_ARG; }
  if (n > 0xFFFFFFFFull) { c->err = "mk_fastq_overlap_device: the text is one piece, which holds at most 2^32 - 1 bytes"; return MK_ERR_RANGE; }
  if ((uintptr_t)d_rows & 7) { c->err = "mk_fastq_overlap_device: d_rows must be aligned to 8"; return MK_ERR_ARG; }
  OvOpt o{};
  if (const char* msg = ov_options(opt, o)) { c->err = std::string("mk_fastq_overlap_device: ") + msg; return MK_ERR_ARG; }
  OvCall f(c, "mk_fastq_overlap_device", o, (d_keep || d_rows) ? cap : ~(size_t)0, d_keep, (u64*)d_rows, d_out, out_cap, true);
  // (the merge writer patches the text: the caller's stays as it is, the call works on a copy)
  return ov_run(f, out_len, nrec, st, [&]() -> int { return fq_device_body(f, d_fastq, n, OvPolicy::merges(o)); });
}

extern "C" int mk_fastq_overlap_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_overlap_opt_t* opt, size_t cap,
                                     uint8_t* keep, uint64_t* rows, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                                     mk_fastq_overlap_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_fastq_overlap_text: NULL buffer"; return MK_ERR_ARG; }
  OvOpt o{};
  if (const char* msg = ov_options(opt, o)) { c->err = std::string("mk_fastq_overlap_text: ") + msg; return MK_ERR_ARG; }
  OvCall f(c, "mk_fastq_overlap_text", o, (keep || rows) ? cap : ~(size_t)0, keep, (u64*)rows, out, out_cap, false);
  return ov_run(f, out_len, nrec, st, [&]() -> int { return fq_text_body(f, fastq, n, piece_bytes); });
}
