// mk_adapt.hip -- 3' adapter removal from the reads of a FASTQ text (mk_adapters_pack, mk_fastq_adapt_text /
// mk_fastq_adapt_device; include/mercat_hip.h has the rule and the panel's layout): every read is cut at the leftmost
// position at which an adapter of the panel matches its remainder (or runs off its end) within the error rate, the
// survivors gathered as FASTQ -- on the GPU, by mk_qtrim.hip's scheme (mk_fqpiece.h has the shared parts):
//   fs_index_open / fs_index_lines<false>        the line index (mk_fqindex.h), unchanged.
//   ad_scan_k                a wave a record, a lane a candidate position, 64 positions a block.  Lanes 0 .. 11 load the 12
//                            aligned 16-byte granules that hold the block's positions and the 128 bases behind them
//                            (QtLine: fs_load) and pack each into 32 bits of 2-bit codes and 32 bits of an "other" plane
//                            (a byte that is not ACGT after folding); every lane fetches the nine words its window
//                            touches (__shfl) and funnel-shifts them into its own 128-base window, four 64-bit words of
//                            each plane, held in registers.  Then the adapter loop, wave-uniform, the panel read through
//                            uniform (scalar) loads: 32 bases a step, x = win ^ adp, popcount of (x | x >> 1 | other) &
//                            care & avail, care being the adapter's non-N bases and avail the bases the read still has;
//                            a lane keeps its first admissible adapter.  Ballot and find-first pick the leftmost lane
//                            that has one, and the record stops at the first block with a hit.  A read longer than a
//                            block is a loop over blocks; positions with fewer than min_overlap bases behind them are
//                            never tested.  hits are counted in the workgroup's LDS and flushed once with vector
//                            atomics.  No loop trusts a byte of the text: all bounds come from line[].
//   ad_decide_k              a lane per record: the checks, keep[r] from the verdicts of both mates, the counters, and
//                            the four segments of fq_segments with start = 0.
//   rocprim::exclusive_scan, fs_gather_k / fs_edges_k   as in mk_qtrim.hip, through fq_piece.
#include "mk_fqpiece.h"

#define AD_NONE 0xFFFFFFFFu
#define AD_MAX_ADAPTERS 1024u
#define AD_MAX_BASES 128u
#define AD_STRIDE 9u  // words an adapter: header, four of codes, four of the care plane
#define AD_EVEN 0x5555555555555555ull
#define AD_BLOCK 64u  // candidate positions a block: a lane each

struct AdStatus {  // device memory, behind the FsStatus of the piece
  u64 dropped_short, orphans, bases_in;
};
struct AdOpt {
  unsigned min_overlap, max_err_ppm, min_len, paired, which;
};
enum { AD_PASSES = 0, AD_SHORT = 1, AD_FAILED = 5 };

// The 16 bytes of a granule as 2-bit codes (A 0, C 1, G 2, T 3; lower case folded) and the other plane: bit 2b set for
// a byte b that is none of them, whose code then says nothing.
__device__ __forceinline__ void ad_pack16(const FsSeg& c, unsigned& codes, unsigned& other) {
  codes = 0;
  other = 0;
#pragma unroll
  for (unsigned b = 0; b < 16; ++b) {
    const unsigned f = QT_BYTE(c, b) & 0xDFu;  // (only X and X | 0x20 fold to X)
    const bool acgt = f == 'A' || f == 'C' || f == 'G' || f == 'T';
    codes |= (((f >> 1) ^ (f >> 2)) & 3u) << (2 * b);
    other |= (acgt ? 0u : 1u) << (2 * b);
  }
}

// rows[5 r ..]: length, kept, adapter, overlap, mismatches; verdict[r]: AD_PASSES, AD_SHORT, or AD_FAILED for a record that
// fails a check (ad_decide_k names it).  panel: mk_adapters_pack's words.  hits[a]: records whose hit is adapter a; the
// workgroup's own counters are 32-bit, which the hosts' limit on a piece (below 2^32 bytes) makes safe.  Pieces start at
// even records: the parity of r is the mate.
static __global__ void __launch_bounds__(256) ad_scan_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ line, size_t nrec,
                                                        AdOpt o, const u64* __restrict__ panel, unsigned A, u64* __restrict__ rows,
                                                        uint8_t* __restrict__ verdict, u64* __restrict__ hits) {
  __shared__ unsigned s_hits[AD_MAX_ADAPTERS];
  for (unsigned i = threadIdx.x; i < AD_MAX_ADAPTERS; i += 256) s_hits[i] = 0;
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t per_grid = (size_t)gridDim.x * 4;
  for (size_t r = (size_t)blockIdx.x * 4 + wave; r < nrec; r += per_grid) {
    const QtRecord rec = qt_record(text, line, r);
    unsigned v = AD_FAILED, hit_a = AD_NONE, hit_ov = 0, hit_mm = 0;
    u64 L = 0, cut = 0;
    if (rec.fail < 0) {
      L = rec.ls;
      cut = L;
      const unsigned cls = o.paired && (r & 1) ? 2u : 1u;
      const QtLine sl{rec.l1, L};
      const u64 off = rec.l1 & 15;  // stream position t = content index + off: the stream starts at the line's first granule
      if (L >= o.min_overlap) {
        const u64 last_t = off + L - o.min_overlap;  // the last candidate
        for (u64 b = 0; b <= last_t / AD_BLOCK && hit_a == AD_NONE; ++b) {
          // granules 4 b .. 4 b + 11: the block's 64 positions and the 128 behind the last of them
          unsigned cw = 0, ow = 0;
          if (lane < 12) {
            const u64 g = 4 * b + lane;
            ad_pack16(sl.load(text, n, (unsigned)(g >> 4), (unsigned)(g & 15)), cw, ow);
          }
          const unsigned q = lane >> 4, sh = 2 * (lane & 15u);
          unsigned c[9], x[9];
#pragma unroll
          for (unsigned k = 0; k < 9; ++k) {
            c[k] = (unsigned)__shfl((int)cw, (int)(q + k));
            x[k] = (unsigned)__shfl((int)ow, (int)(q + k));
          }
          const u64 t = b * AD_BLOCK + lane;
          const bool valid = t >= off && t <= last_t;
          const u64 left = valid ? L - (t - off) : 0;
          const unsigned avail = left > AD_MAX_BASES ? AD_MAX_BASES : (unsigned)left;
          u64 win[4], oth[4], am[4];
#pragma unroll
          for (unsigned w = 0; w < 4; ++w) {
            win[w] = (u64)__funnelshift_r(c[2 * w], c[2 * w + 1], sh) | ((u64)__funnelshift_r(c[2 * w + 1], c[2 * w + 2], sh) << 32);
            oth[w] = (u64)__funnelshift_r(x[2 * w], x[2 * w + 1], sh) | ((u64)__funnelshift_r(x[2 * w + 1], x[2 * w + 2], sh) << 32);
            const unsigned nb = avail > 32 * w ? (avail - 32 * w > 32 ? 32u : avail - 32 * w) : 0u;
            am[w] = nb == 32 ? AD_EVEN : (((1ull << (2 * nb)) - 1) & AD_EVEN);
          }
          unsigned found = AD_NONE, f_ov = 0, f_mm = 0;
          for (unsigned a = 0; a < A; ++a) {
            const u64* __restrict__ p = panel + 1 + (size_t)AD_STRIDE * a;
            const u64 hd = p[0];
            const unsigned m = (unsigned)(hd & 0xFFu), acls = (unsigned)(hd >> 8) & 3u;
            if (!(acls & cls) || (unsigned)(hd >> 32) != a || m < o.min_overlap) continue;
            unsigned mm = 0;
#pragma unroll
            for (unsigned w = 0; w < 4; ++w)
              if (32 * w < m) {
                const u64 d = win[w] ^ p[1 + w];
                mm += (unsigned)__popcll((d | (d >> 1) | oth[w]) & p[5 + w] & am[w]);
              }
            const unsigned ov = m < avail ? m : avail;
            if (valid && found == AD_NONE && ov >= o.min_overlap && (u64)mm * 1000000ull <= (u64)o.max_err_ppm * ov) {
              found = a;
              f_ov = ov;
              f_mm = mm;
            }
          }
          const u64 got = __ballot(found != AD_NONE);
          if (got) {
            const int src = __ffsll((unsigned long long)got) - 1;
            hit_a = (unsigned)__shfl((int)found, src);
            hit_ov = (unsigned)__shfl((int)f_ov, src);
            hit_mm = (unsigned)__shfl((int)f_mm, src);
            cut = b * AD_BLOCK + (unsigned)src - off;
          }
        }
      }
      v = cut < (o.min_len > 1u ? o.min_len : 1u) ? AD_SHORT : AD_PASSES;
    }
    const u64 mine = lane == 0 ? L : lane == 1 ? cut : lane == 2 ? (u64)hit_a : lane == 3 ? (u64)hit_ov : (u64)hit_mm;
    if (lane < 5) rows[5 * r + lane] = mine;
    if (lane == 0) {
      verdict[r] = (uint8_t)v;
      if (hit_a != AD_NONE) atomicAdd(&s_hits[hit_a], 1u);
    }
  }
  __syncthreads();
  for (unsigned i = threadIdx.x; i < A; i += 256)
    if (s_hits[i]) atomicAdd((unsigned long long*)&hits[i], (unsigned long long)s_hits[i]);
}

// A lane per record (and one for the slot behind the last segment).  Record r is lines 4r .. 4r + 3; its segments are
// 4r .. 4r + 3.
static __global__ void __launch_bounds__(256) ad_decide_k(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t nrec, AdOpt o,
                                                          const u64* __restrict__ rows, const uint8_t* __restrict__ verdict,
                                                          uint8_t* __restrict__ keep, u64* __restrict__ seg_src, u64* __restrict__ len,
                                                          FsStatus* __restrict__ st, AdStatus* __restrict__ as) {
  u64 n_out = 0, n_trimmed = 0, n_bases = 0, n_in = 0, n_short = 0, n_orphans = 0;
  mk_for_each(nrec + 1, [&](size_t r) {
    if (r == nrec) {
      seg_src[4 * nrec] = 0;
      len[4 * nrec] = 0;
      return;
    }
    const QtRecord q = qt_record(text, line, r);
    if (q.fail >= 0) atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | (unsigned)q.fail));
    const unsigned v = verdict[r];
    unsigned k = v == AD_PASSES ? 1u : 0u;
    if (k && o.paired) k = ((r ^ 1) < nrec && verdict[r ^ 1] == AD_PASSES) ? 1u : 2u;
    keep[r] = (uint8_t)k;
    const u64 L = rows[5 * r], kept = rows[5 * r + 1];
    n_in += q.fail < 0 ? L : 0;
    n_short += v == AD_SHORT;
    n_orphans += k == 2u;
    u64 s[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    if (q.fail < 0 && k && k == o.which) {
      n_trimmed += fq_segments(q, L, 0, kept, s, m) ? 1 : 0;
      n_out += 1;
      n_bases += kept;
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
  block_add(&as->bases_in, n_in);
  block_add(&as->dropped_short, n_short);
  block_add(&as->orphans, n_orphans);
}

// ------------------------------------------------------------------------------------------ host side
extern "C" int mk_adapters_pack(const uint8_t* bases, const uint32_t* lengths, const uint8_t* mates, size_t A, uint64_t* words,
                                size_t words_cap, size_t* nwords, char* err, size_t err_cap) {
  const auto fail = [&](int rc, const std::string& msg) {
    if (err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
    return rc;
  };
  if (nwords) *nwords = 0;
  if (A < 1 || A > AD_MAX_ADAPTERS) return fail(MK_ERR_ARG, "the panel holds " + std::to_string(A) + " adapters: must be 1 .. 1024");
  if (!bases || !lengths) return fail(MK_ERR_ARG, "NULL buffer");
  const size_t need = 1 + (size_t)AD_STRIDE * A;
  std::vector<uint64_t> w(need, 0);
  w[0] = A;
  size_t at = 0;
  for (size_t a = 0; a < A; ++a) {
    const uint32_t m = lengths[a];
    const unsigned cls = mates ? mates[a] : 1u;
    if (m < 1 || m > AD_MAX_BASES)
      return fail(MK_ERR_ARG, "adapter " + std::to_string(a) + " has " + std::to_string(m) + " bases: must be 1 .. 128");
    if (cls < 1 || cls > 3) return fail(MK_ERR_ARG, "adapter " + std::to_string(a) + " has mate class " + std::to_string(cls) + ": must be 1, 2 or 3");
    uint64_t* p = w.data() + 1 + AD_STRIDE * a;
    for (uint32_t j = 0; j < m; ++j) {
      const unsigned ch = bases[at + j], f = ch & 0xDFu;
      unsigned code = 0;
      bool care = true;
      switch (f) {
        case 'A': code = 0; break;
        case 'C': code = 1; break;
        case 'G': code = 2; break;
        case 'T': code = 3; break;
        case 'N': care = false; break;
        default: {
          char hex[8];
          snprintf(hex, sizeof hex, "0x%02X", ch);
          return fail(MK_ERR_ARG, "adapter " + std::to_string(a) + " holds the byte " + hex + " at base " + std::to_string(j) +
                                      ": its bases must be of ACGTN");
        }
      }
      p[1 + j / 32] |= (uint64_t)code << (2 * (j % 32));
      if (care) p[5 + j / 32] |= 1ull << (2 * (j % 32));
    }
    at += m;
    size_t first = a;
    for (size_t b = 0; b < a && first == a; ++b) {
      const uint64_t* q = w.data() + 1 + AD_STRIDE * b;
      if ((q[0] & 0xFFFFu) == ((uint64_t)m | ((uint64_t)cls << 8)) && !memcmp(q + 1, p + 1, 8 * sizeof(uint64_t))) first = b;
    }
    p[0] = (uint64_t)m | ((uint64_t)cls << 8) | ((uint64_t)first << 32);
  }
  if (nwords) *nwords = need;
  if (!words) return MK_OK;
  if (words_cap < need) return fail(MK_ERR_RANGE, "the panel takes " + std::to_string(need) + " words, words has room for " + std::to_string(words_cap));
  memcpy(words, w.data(), need * sizeof(uint64_t));
  return MK_OK;
}

// What mk_fqpiece.h's piece loop asks of a call.  Side: the packed panel and hits[A] in device memory.
struct AdPolicy {
  typedef AdOpt Opt;
  typedef AdStatus Status;
  typedef mk_fastq_adapt_t Stats;
  struct Side { const u64* d_panel; u64* d_hits; unsigned A; };
  static constexpr size_t ROW = 5;
  static bool paired(const AdOpt& o) { return o.paired != 0; }
  static const char* kind(unsigned k) { return fs_kind(k); }
  static void scan(FqCall<AdPolicy>& f, const uint8_t* d_text, size_t n, const u64* line, size_t nrec, u64* d_rows, uint8_t* d_verdict,
                   FsStatus*) {
    hipLaunchKernelGGL(ad_scan_k, dim3(grid_for(nrec, 4, 1u << 14)), dim3(256), 0, f.c->stream, d_text, (u64)n, line, nrec, f.o, f.side.d_panel,
                       f.side.A, d_rows, d_verdict, f.side.d_hits);
  }
  static void decide(FqCall<AdPolicy>& f, const uint8_t* d_text, const u64* line, size_t nrec, const u64* d_rows, const uint8_t* d_verdict,
                     uint8_t* d_keep, u64* seg_src, u64* len, FsStatus* d_st, AdStatus* d_as) {
    hipLaunchKernelGGL(ad_decide_k, dim3(grid_for(nrec + 1, 256, 4096)), dim3(256), 0, f.c->stream, d_text, line, nrec, f.o, d_rows,
                       d_verdict, d_keep, seg_src, len, d_st, d_as);
  }
  static void add(mk_fastq_adapt_t& st, const AdStatus& q) {
    st.bases_in += q.bases_in;
    st.dropped_short += q.dropped_short;
    st.orphans += q.orphans;
  }
};
typedef FqCall<AdPolicy> AdCall;

// The options as the kernels take them, or the message of the first one out of range.
static const char* ad_options(const mk_adapt_opt_t* opt, AdOpt& o) {
  if (!opt) return "opt is NULL";
  if (opt->min_overlap < 1 || opt->min_overlap > AD_MAX_BASES) return "min_overlap must be 1 .. 128";
  if (opt->max_err_ppm > 1000000) return "max_err_ppm must be 0 .. 1000000";
  if (opt->which != 1 && !(opt->which == 2 && opt->paired)) return "which must be 1 (the main output) or, with paired, 2 (the orphans)";
  o.min_overlap = opt->min_overlap;
  o.max_err_ppm = opt->max_err_ppm;
  o.min_len = opt->min_len;
  o.paired = opt->paired ? 1 : 0;
  o.which = opt->which;
  return nullptr;
}

// The panel packed once a call (MK_ERR_ARG with the packer's message otherwise).
static int ad_panel(mk_ctx* c, const char* what, const uint8_t* bases, const uint32_t* lengths, const uint8_t* mates, size_t A,
                    std::vector<uint64_t>& words) {
  char msg[256] = "";
  size_t nwords = 0;
  words.assign(1 + (size_t)AD_STRIDE * std::min<size_t>(std::max<size_t>(A, 1), AD_MAX_ADAPTERS), 0);
  const int rc = mk_adapters_pack(bases, lengths, mates, A, words.data(), words.size(), &nwords, msg, sizeof msg);
  if (rc != MK_OK) c->err = std::string(what) + ": " + msg;
  return rc;
}

// fq_run with the panel copied to the device and hits zeroed before the pieces and, for the text call, hits copied to
// h_hits (host memory) behind them.  d_hits: the caller's device memory, or nullptr.
template <class Body>
static int ad_run(AdCall& f, const std::vector<uint64_t>& words, u64* d_hits, u64* h_hits, size_t* out_len, size_t* nrec, mk_fastq_adapt_t* st,
                  Body&& body) {
  mk_ctx* c = f.c;
  const size_t A = (size_t)words[0];
  return fq_run(
      f, out_len, nrec, st,
      [&]() -> int {
        int rc = mk_buf_reserve(c, f.side_buf, (words.size() + A) * sizeof(u64));
        if (rc != MK_OK) return rc;
        f.side.d_panel = (const u64*)f.side_buf.p;
        f.side.d_hits = d_hits ? d_hits : (u64*)f.side_buf.p + words.size();
        f.side.A = (unsigned)A;
        MK_HIP(hipMemcpyAsync(f.side_buf.p, words.data(), words.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
        MK_HIP(hipMemsetAsync(f.side.d_hits, 0, A * sizeof(u64), c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
        return MK_OK;
      },
      body,
      [&]() -> int {
        if (!h_hits) return MK_OK;
        const auto t1 = MkClock::now();
        MK_HIP(hipMemcpyAsync(h_hits, f.side.d_hits, A * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
        f.st.s_write += mk_since(t1);
        return MK_OK;
      });
}

extern "C" int mk_fastq_adapt_device(mk_ctx* c, const uint8_t* d_fastq, size_t n, const uint8_t* bases, const uint32_t* lengths,
                                     const uint8_t* mates, size_t A, const mk_adapt_opt_t* opt, size_t cap, uint8_t* d_keep, uint64_t* d_rows,
                                     uint64_t* d_hits, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec, mk_fastq_adapt_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_fastq) || (out_cap && !d_out)) { c->err = "mk_fastq_adapt_device: NULL buffer"; return MK_ERR_ARG; }
  // (a workgroup of ad_scan_k counts the records it sees in 32-bit LDS counters: fewer than 2^32 of them in a piece)
  if (n > 0xFFFFFFFFull) { c->err = "mk_fastq_adapt_device: the text is one piece, which holds at most 2^32 - 1 bytes"; return MK_ERR_RANGE; }
  if (((uintptr_t)d_rows | (uintptr_t)d_hits) & 7) { c->err = "mk_fastq_adapt_device: d_rows and d_hits must be aligned to 8"; return MK_ERR_ARG; }
  AdOpt o{};
  if (const char* msg = ad_options(opt, o)) { c->err = std::string("mk_fastq_adapt_device: ") + msg; return MK_ERR_ARG; }
  std::vector<uint64_t> words;
  int rc = ad_panel(c, "mk_fastq_adapt_device", bases, lengths, mates, A, words);
  if (rc != MK_OK) return rc;
  AdCall f(c, "mk_fastq_adapt_device", o, (d_keep || d_rows) ? cap : ~(size_t)0, d_keep, (u64*)d_rows, d_out, out_cap, true);
  return ad_run(f, words, (u64*)d_hits, nullptr, out_len, nrec, st, [&]() -> int { return fq_device_body(f, d_fastq, n); });
}

extern "C" int mk_fastq_adapt_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const uint8_t* bases,
                                   const uint32_t* lengths, const uint8_t* mates, size_t A, const mk_adapt_opt_t* opt, size_t cap, uint8_t* keep,
                                   uint64_t* rows, uint64_t* hits, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                                   mk_fastq_adapt_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_fastq_adapt_text: NULL buffer"; return MK_ERR_ARG; }
  AdOpt o{};
  if (const char* msg = ad_options(opt, o)) { c->err = std::string("mk_fastq_adapt_text: ") + msg; return MK_ERR_ARG; }
  std::vector<uint64_t> words;
  int rc = ad_panel(c, "mk_fastq_adapt_text", bases, lengths, mates, A, words);
  if (rc != MK_OK) return rc;
  AdCall f(c, "mk_fastq_adapt_text", o, (keep || rows) ? cap : ~(size_t)0, keep, (u64*)rows, out, out_cap, false);
  return ad_run(f, words, nullptr, (u64*)hits, out_len, nrec, st, [&]() -> int { return fq_text_body(f, fastq, n, piece_bytes); });
}
