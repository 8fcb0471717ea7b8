// mk_correctwalk.h -- what the correcting calls share: mk_correct_* (mk_correct.hip) emits the corrected records as FASTA,
// mk_correct_fastq_* (mk_correctfq.hip) patches the FASTQ text they came from.  The run kernels (cr_runs_k, cr_heads_k),
// the try kernel (cr_try_k), the patch into the stream (cr_apply_k), the lengths, guards and totals (cr_decide_k), and
// the host side up to the totals: cr_front (placement and the weak runs) and cr_totals.  mk_correct.hip has the scheme.
#pragma once
#include "mk_trimwalk.h"
#include "mk_trackwalk.h"

struct CrStatus {  // device memory, read back twice a piece (fl: what the start kernels found)
  FlStatus fl;
  u64 ncand;      // candidates appended (cr_runs_k)
  u64 overflow;   // candidates the list had no room for
  u64 outside;    // candidates whose p, or whose windows, lie outside their record
  u64 disagree;   // records whose runs contradict their row, or whose length in the stream contradicts its windows
  u64 locked;     // probes that met a slot being claimed (cannot happen on a quiescent table)
  u64 runs, fixed, ambiguous, unfixable, bases;
};
static_assert(sizeof(CrStatus) <= 128, "CrStatus");

struct CrCand {  // a run with a candidate: the stream positions of its first window and of p, its record, its windows
  u64 wpos, ppos;
  unsigned rec, n;
};

__device__ __forceinline__ unsigned cr_code(unsigned ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 99u; }

// The run that starts at window i of record r -- weak, its predecessor solid or another record's -- measured (k + 1
// counts at most), added to the record's runs and classified.  Returns whether its shape names a candidate: c.
template <class E>
__device__ __forceinline__ bool cr_own(const E* __restrict__ counts, const u64* __restrict__ woff, const u64* __restrict__ sstart, size_t r,
                                       u64 i, u64 at_least, u64 k, u64 seq_len, mk_correct_row_t* __restrict__ fix, CrCand& c, u64& bad) {
  const u64 w0 = woff[r], W = woff[r + 1] - w0, a = i - w0;
  u64 n = 1;  // (k + 1: longer than k, wherever it ends)
  while (n <= k && a + n < W && (u64)counts[i + n] < at_least) ++n;
  atomicAdd(&fix[r].runs, 1u);
  if (n > k) return false;
  const bool at_start = a == 0, at_end = a + n == W;
  u64 p;
  if (at_start && at_end) return false;
  else if (at_start) p = a + n - 1;
  else if (at_end) p = a + k - 1;
  else if (n == k) p = a + n - 1;
  else return false;
  const u64 ss = sstart[r];
  if (ss > seq_len || p >= W + k - 1 || W + k - 1 > seq_len - ss) { ++bad; return false; }
  c = CrCand{ss + a, ss + p, (unsigned)r, (unsigned)n};
  return true;
}

// The candidates of a workgroup appended to the list (cap entries) with one add to its length: every thread calls it.
__device__ __forceinline__ void cr_append(bool cand, const CrCand& c, CrCand* __restrict__ list, u64 cap, CrStatus* __restrict__ st, u64& over) {
  __shared__ unsigned s_cnt[4];
  __shared__ unsigned long long s_base;
  const unsigned long long m = __ballot(cand);
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_cnt[wave] = (unsigned)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned all = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    s_base = all ? atomicAdd((unsigned long long*)&st->ncand, (unsigned long long)all) : 0ull;
  }
  __syncthreads();
  if (cand) {
    u64 slot = s_base + (u64)__popcll(m & ((1ull << lane) - 1));
    for (unsigned w = 0; w < wave; ++w) slot += s_cnt[w];
    if (slot < cap) list[slot] = c;
    else ++over;
  }
}

// A lane a window of the piece (element i of counts; whole workgroups, no loop: the ballot of cr_append is of whole
// waves).  The lane whose window is weak and whose predecessor is solid, or is none, owns the run and only then looks
// for its record (a binary search of woff).  A run that starts a record behind a weak window of the record in front is
// cr_heads_k's.
template <class E>
__global__ void __launch_bounds__(256) cr_runs_k(const E* __restrict__ counts, const u64* __restrict__ woff, const u64* __restrict__ sstart,
                                                 size_t nrows, u64 total, u64 at_least, u64 k, u64 seq_len,
                                                 mk_correct_row_t* __restrict__ fix, CrCand* __restrict__ list, u64 cap,
                                                 CrStatus* __restrict__ st) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  bool cand = false;
  CrCand c{};
  u64 bad = 0, over = 0;
  if (i < total && (u64)counts[i] < at_least && (i == 0 || (u64)counts[i - 1] >= at_least))
    cand = cr_own(counts, woff, sstart, tk_record_of(woff, nrows, i), i, at_least, k, seq_len, fix, c, bad);
  cr_append(cand, c, list, cap, st, over);
  block_add(&st->outside, bad);
  block_add(&st->overflow, over);
}

// A lane a record (whole workgroups, no loop): the run at the record's first window where the window in front of it --
// the last of an earlier record -- is weak too, which cr_runs_k takes for the inside of a run.
template <class E>
__global__ void __launch_bounds__(256) cr_heads_k(const E* __restrict__ counts, const u64* __restrict__ woff, const u64* __restrict__ sstart,
                                                  size_t nrows, u64 at_least, u64 k, u64 seq_len, mk_correct_row_t* __restrict__ fix,
                                                  CrCand* __restrict__ list, u64 cap, CrStatus* __restrict__ st) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool cand = false;
  CrCand c{};
  u64 bad = 0, over = 0;
  if (r < nrows) {
    const u64 i = woff[r];
    if (woff[r + 1] > i && i > 0 && (u64)counts[i] < at_least && (u64)counts[i - 1] < at_least)
      cand = cr_own(counts, woff, sstart, r, i, at_least, k, seq_len, fix, c, bad);
  }
  cr_append(cand, c, list, cap, st, over);
  block_add(&st->outside, bad);
  block_add(&st->overflow, over);
}

// The window of a lane with s[p] replaced, byte by byte, for the text probe.
struct CrSubst {
  const uint8_t* w;
  int q;
  unsigned x;
  __device__ __forceinline__ unsigned operator()(int i) const { return i == q ? x : w[i]; }
};

// A wave a candidate, lane i window a + i of its run (n <= k <= 64).  The lane packs its window once with the two bits
// of p left empty, derives the key of every alternative from that, folds it, and has the probes of all alternatives
// issued before it compares any (LkStep); a window that holds another byte outside ACGT is probed as text.  patch[ci]:
// the byte that goes to the candidate's p, 0 for none.  The stream is only read.
template <int KEYS, bool FOLD>
__global__ void __launch_bounds__(256) cr_try_k(const uint8_t* __restrict__ seq, u64 seq_len, const CrCand* __restrict__ list, u64 ncand,
                                                int k, u64 at_least, LkTables t, mk_correct_row_t* __restrict__ fix,
                                                uint8_t* __restrict__ patch, CrStatus* __restrict__ st) {
  const u64 ci = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6;
  const unsigned lane = threadIdx.x & 63;
  if (ci >= ncand) return;  // (the whole wave)
  const CrCand c = list[ci];
  // every window of the run holds p and lies in the stream (the whole wave decides alike)
  if (c.n < 1 || c.n > (unsigned)k || k > 64 || c.ppos < c.wpos + (c.n - 1) || c.ppos > c.wpos + (u64)(k - 1) ||
      c.wpos + (c.n - 1) + (u64)k > seq_len) {
    if (lane == 0) {
      patch[ci] = 0;
      atomicAdd((unsigned long long*)&st->outside, 1ull);
    }
    return;
  }
  const unsigned orig = cr_code(seq[c.ppos]);
  bool viable[4] = {true, true, true, true};  // (a lane without a window objects to nothing)
  LkStep<KEYS, 4> p;
  if (lane < c.n) {
    const uint8_t* w = seq + c.wpos + lane;
    const int q = (int)(c.ppos - c.wpos) - (int)lane;  // p's place in this window
    u64 a = 0, b = 0;
    unsigned others = 0;  // bytes outside ACGT beside p
    for (int j = 0; j < k; ++j) {
      const unsigned code = cr_code(w[j]);
      if (j == q) continue;
      if (code == 99u) { ++others; continue; }
      if (KEYS == TL_ONE_WORD) a |= (u64)code << (2 * (k - 1 - j));
      else if (j < 32) a |= (u64)code << (62 - 2 * j);
      else b |= (u64)code << (62 - 2 * (j - 32));
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      p.clear(x);
      if ((unsigned)x == orig) continue;
      if (others) {
        p.issue(x, t, CrSubst{w, q, (unsigned)"ACGT"[x]}, k);
        continue;
      }
      u64 ka = a, kb = b;
      if (KEYS == TL_ONE_WORD) ka |= (u64)x << (2 * (k - 1 - q));
      else if (q < 32) ka |= (u64)x << (62 - 2 * q);
      else kb |= (u64)x << (62 - 2 * (q - 32));
      if (FOLD) p.fold(ka, kb, k);
      p.issue(x, t, ka, kb);
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if ((unsigned)x != orig) viable[x] = p.finish(x, t) >= at_least;
  }
  unsigned nviable = 0, which = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const bool all = __all(viable[x]);
    if ((unsigned)x != orig && all) { ++nviable; which = (unsigned)x; }
  }
  if (__any(p.locked != 0) && lane == 0) atomicAdd((unsigned long long*)&st->locked, 1ull);
  if (lane == 0) {
    patch[ci] = nviable == 1 ? (uint8_t)"ACGT"[which] : (uint8_t)0;
    atomicAdd(nviable == 1 ? &fix[c.rec].fixed : nviable ? &fix[c.rec].ambiguous : &fix[c.rec].unfixable, 1u);
  }
}

// A lane a candidate: its patch, if it has one, into the stream.  No two candidates share a p.
static __global__ void __launch_bounds__(256) cr_apply_k(const CrCand* __restrict__ list, const uint8_t* __restrict__ patch, u64 ncand,
                                                         uint8_t* __restrict__ seq, u64 seq_len) {
  mk_for_each((size_t)ncand, [&](size_t ci) {
    const uint8_t x = patch[ci];
    const u64 at = list[ci].ppos;
    if (x && at < seq_len) seq[at] = x;
  });
}

// A lane per record (and one for the slot behind the last, whose length is 0 so that the scan ends in the total):
// slen[r] = L, the record's characters in the stream -- from sstart, so that a record shorter than k is emitted whole --
// and len[r] = hlen + L + 1, or hlen alone for a record without characters.
static __global__ void __launch_bounds__(256) cr_decide_k(const mk_screen_row_t* __restrict__ rows, const u64* __restrict__ sstart,
                                                          const u64* __restrict__ hlen, const mk_correct_row_t* __restrict__ fix,
                                                          size_t nrows, u64 k, u64 seq_len, u64* __restrict__ slen, u64* __restrict__ len,
                                                          CrStatus* __restrict__ st) {
  u64 bad = 0, runs = 0, fixed = 0, amb = 0, unfix = 0, bases = 0;
  mk_for_each(nrows + 1, [&](size_t r) {
    if (r == nrows) { len[r] = 0; return; }
    const u64 ss = sstart[r], end = r + 1 < nrows ? sstart[r + 1] - 1 : seq_len;  // (the next record's separator)
    u64 L = 0;
    if (ss > seq_len || end > seq_len || end < ss) ++bad;
    else L = end - ss;
    const mk_correct_row_t f = fix[r];
    const u64 windows = rows[r].windows;
    bad += windows != (L >= k ? L - k + 1 : 0) ? 1 : 0;
    bad += ((rows[r].hits == windows) != (f.runs == 0)) ? 1 : 0;
    bad += ((u64)f.fixed + f.ambiguous + f.unfixable > f.runs) ? 1 : 0;
    slen[r] = L;
    len[r] = hlen[r] + (L ? L + 1 : 0);
    runs += f.runs;
    fixed += f.fixed;
    amb += f.ambiguous;
    unfix += f.unfixable;
    bases += L;
  });
  block_add(&st->disagree, bad);
  block_add(&st->runs, runs);
  block_add(&st->fixed, fixed);
  block_add(&st->ambiguous, amb);
  block_add(&st->unfixable, unfix);
  block_add(&st->bases, bases);
}

// ------------------------------------------------------------------------------------------ host side
struct CrCall {
  mk_correct_rule_t rule;
  FlEmit emit;             // where the output goes
  mk_correct_row_t* fix;   // the caller's, or nullptr; cap of each
  mk_screen_row_t* rows;
  size_t cap;
  bool device;             // out / fix / rows are device memory
  bool apply = true;       // the patches go into the stream (cr_apply_k); false: they stay in list / patch for the caller
  u64 ncand = 0;           // candidates of the last piece: entries of list / patch
  MkDevBuf d_rows, d_fix, meta, scan_tmp, counts, list, patch;
  MkTimed place, track, runs, tries;
  mk_correct_t st{};
  CrCall(mk_ctx* c, const mk_correct_rule_t& r, uint8_t* o, size_t oc, mk_correct_row_t* fx, mk_screen_row_t* rw, size_t cp, bool dev)
      : rule(r), emit(c, o, oc, dev), fix(fx), rows(rw), cap(cp), device(dev), place(c), track(c), runs(c), tries(c) {}
  ~CrCall() {
    for (MkDevBuf* b : {&d_rows, &d_fix, &meta, &scan_tmp, &counts, &list, &patch}) buf_free(*b);
  }
};

static int cr_launch_try(ScCall& s, const CrCand* list, u64 ncand, mk_correct_row_t* d_fix, uint8_t* patch, CrStatus* d_st) {
  mk_ctx* c = s.c;
  const LkTables t = lk_tables(c);
  const unsigned grid = (unsigned)div_up((size_t)ncand, 4);
#define CR_GO(K, F) hipLaunchKernelGGL((cr_try_k<K, F>), dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)c->seq.p, \
                                       (u64)s.last.seq_len, list, ncand, c->k, s.at_least, t, d_fix, patch, d_st)
  if (tl_keys_of(c) == TL_ONE_WORD) { if (s.fold) CR_GO(TL_ONE_WORD, true); else CR_GO(TL_ONE_WORD, false); }
  else { if (s.fold) CR_GO(TL_TWO_WORD_NT, true); else CR_GO(TL_TWO_WORD_NT, false); }  // (cr_run: no other kind gets here)
#undef CR_GO
  MK_HIP(hipGetLastError());
  return MK_OK;
}

// The weak runs of a piece of `total` windows, `weak` of them below at_least, found, tried and applied: the track into
// scratch of E, cr_runs_k and cr_heads_k, cr_try_k, cr_apply_k (with f.apply).  The stream is idle afterwards.
template <class E>
static int cr_weak(ScCall& s, CrCall& f, const u64* woff, const u64* sstart, size_t nrows, u64 total, u64 weak, mk_correct_row_t* d_fix,
                   CrStatus* d_st, TkStatus* d_tk) {
  mk_ctx* c = s.c;
  int rc;
  const size_t seq_len = s.last.seq_len;
  const u64 cap = std::min(weak, total);
  if ((rc = mk_buf_reserve(c, f.counts, (size_t)total * sizeof(E))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, f.list, (size_t)cap * sizeof(CrCand))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, f.patch, (size_t)cap)) != MK_OK) return rc;
  E* d_counts = (E*)f.counts.p;
  CrCand* list = (CrCand*)f.list.p;
  uint8_t* patch = (uint8_t*)f.patch.p;

  if ((rc = f.track.begin()) != MK_OK) return rc;
  if ((rc = tk_launch_probe<E>(s, woff, sstart, nrows, total, d_counts, d_tk)) != MK_OK) return rc;
  if ((rc = f.track.end()) != MK_OK) return rc;
  if ((rc = f.runs.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(cr_runs_k<E>, dim3((unsigned)div_up((size_t)total, 256)), dim3(256), 0, c->stream, (const E*)d_counts, woff, sstart,
                     nrows, total, (u64)s.at_least, (u64)c->k, (u64)seq_len, d_fix, list, cap, d_st);
  hipLaunchKernelGGL(cr_heads_k<E>, dim3((unsigned)div_up(nrows, 256)), dim3(256), 0, c->stream, (const E*)d_counts, woff, sstart, nrows,
                     (u64)s.at_least, (u64)c->k, (u64)seq_len, d_fix, list, cap, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.runs.end()) != MK_OK) return rc;
  CrStatus h{};
  TkStatus ht{};
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&ht, d_tk, sizeof ht, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.track.add_to(f.st.s_track)) != MK_OK || (rc = f.runs.add_to(f.st.s_runs)) != MK_OK) return rc;
  if (ht.written != total) {
    c->err = std::string(s.what) + ": the track kernel wrote " + std::to_string(ht.written) + " of " + std::to_string(total) +
             " windows (internal error)";
    return MK_ERR_STATE;
  }
  if (h.overflow || h.outside || h.ncand > cap) {
    c->err = std::string(s.what) + ": " + std::to_string(h.ncand) + " candidates for " + std::to_string(weak) + " weak windows, " +
             std::to_string(h.outside) + " outside their records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.candidates += h.ncand;
  f.ncand = h.ncand;
  if (!h.ncand) return MK_OK;
  if ((rc = f.tries.begin()) != MK_OK) return rc;
  if ((rc = cr_launch_try(s, list, h.ncand, d_fix, patch, d_st)) != MK_OK) return rc;
  if (f.apply)
    hipLaunchKernelGGL(cr_apply_k, dim3(grid_for((size_t)h.ncand, 256, 4096)), dim3(256), 0, c->stream, (const CrCand*)list,
                       (const uint8_t*)patch, h.ncand, (uint8_t*)c->seq.p, (u64)seq_len);
  MK_HIP(hipGetLastError());
  if ((rc = f.tries.end()) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  return f.tries.add_to(f.st.s_try);
}

// Where a piece's arrays lie in f.meta (cr_front lays them out; nrows + 1 entries unless said otherwise).
struct CrLay {
  CrStatus* d_st;
  u64 *start, *len, *dst, *sstart, *hlen, *slen;  // (sstart, hlen, slen: nrows entries)
  mk_correct_row_t* d_fix;
  size_t scan_bytes;  // of f.scan_tmp: a scan of nrows + 1 uint64_t
  u64 start0;         // start[0], read back
};

// What follows sc_piece for a piece of n bytes (nrows > 0 records) which holds `windows` windows, `hits` of them solid:
// placement and the weak runs.  The stream is idle afterwards.
static int cr_front(ScCall& s, CrCall& f, size_t n, u64 windows, u64 hits, CrLay& lay) {
  mk_ctx* c = s.c;
  int rc;
  const size_t nrows = s.last.nrows;
  f.ncand = 0;
  const uint8_t* text = s.last.text;
  const mk_screen_row_t* d_rows = s.last.d_rows;
  const size_t ntiles = div_up(n, FL_SPAN), seq_len = s.last.seq_len;
  const int headless = s.last.headless ? 1 : 0;
  // meta: CrStatus (128) | TkStatus (32) | start | len | dst | wlen | woff [nrows + 1] each | sstart | hlen | slen
  //       [nrows] each | tile_pre[ntiles] | tile_cnt[ntiles]
  static_assert(sizeof(TkStatus) <= 32, "TkStatus");
  if ((rc = mk_buf_reserve(c, f.meta, 160 + (5 * (nrows + 1) + 3 * nrows + ntiles) * sizeof(u64) + ntiles * sizeof(unsigned))) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, f.d_fix, nrows * sizeof(mk_correct_row_t))) != MK_OK) return rc;
  CrStatus* d_st = (CrStatus*)f.meta.p;
  TkStatus* d_tk = (TkStatus*)((char*)f.meta.p + 128);
  u64* start = (u64*)((char*)f.meta.p + 160);
  u64* len = start + nrows + 1;
  u64* dst = len + nrows + 1;
  u64* wlen = dst + nrows + 1;
  u64* woff = wlen + nrows + 1;
  u64* sstart = woff + nrows + 1;
  u64* hlen = sstart + nrows;
  u64* slen = hlen + nrows;
  u64* tile_pre = slen + nrows;
  unsigned* tile_cnt = (unsigned*)(tile_pre + ntiles);
  mk_correct_row_t* d_fix = (mk_correct_row_t*)f.d_fix.p;
  size_t tmp = 0;  // (both scans are of nrows + 1 uint64_t)
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  MK_HIP(hipMemsetAsync(f.meta.p, 0, 160, c->stream));
  MK_HIP(hipMemsetAsync(d_fix, 0, nrows * sizeof(mk_correct_row_t), c->stream));
  MK_HIP(hipMemsetAsync(start, 0xFF, (nrows + 1) * sizeof(u64), c->stream));  // (a start no header line gives reads as outside the text)
  MK_HIP(hipMemsetAsync(sstart, 0xFF, nrows * sizeof(u64), c->stream));
  if ((rc = f.place.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fl_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fl_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, (u64)n, nrows, headless,
                     start, &d_st->fl);
  hipLaunchKernelGGL(fl_starts_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, text, (u64)n, (const u64*)tile_pre, (u64)headless,
                     nrows, start);
  hipLaunchKernelGGL(tr_hend_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, text, (u64)n, (const u64*)start, nrows,
                     headless, hlen);
  hipLaunchKernelGGL(tk_lens_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, nrows, wlen, d_tk);
  if (seq_len)
    hipLaunchKernelGGL(tk_starts_k, dim3((unsigned)div_up(seq_len, SC_SPAN)), dim3(256), 0, c->stream, (const uint8_t*)c->seq.p,
                       (u64)seq_len, s.last.tile_pre, s.last.row_base, nrows, sstart);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)wlen, woff, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = f.place.end()) != MK_OK) return rc;
  CrStatus h{};
  u64 total = 0, start0 = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&total, woff + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&start0, start, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (h.fl.headers + headless != nrows) {
    c->err = std::string(s.what) + ": " + std::to_string(h.fl.headers) + " header lines in the text, " +
             std::to_string(nrows - headless) + " in the parsed stream (internal error)";
    return MK_ERR_STATE;
  }
  if (total != windows || total > seq_len) {
    c->err = std::string(s.what) + ": the rows of a piece hold " + std::to_string(total) + " windows, its probe saw " +
             std::to_string(windows) + " in a stream of " + std::to_string(seq_len) + " (internal error)";
    return MK_ERR_STATE;
  }

  if (hits != windows) {
    rc = f.rule.at_least <= 0xFFFFFFFFull ? cr_weak<uint32_t>(s, f, woff, sstart, nrows, total, windows - hits, d_fix, d_st, d_tk)
                                          : cr_weak<uint64_t>(s, f, woff, sstart, nrows, total, windows - hits, d_fix, d_st, d_tk);
    if (rc != MK_OK) return rc;
  }
  lay = CrLay{d_st, start, len, dst, sstart, hlen, slen, d_fix, tmp, start0};
  return MK_OK;
}

// cr_decide_k for the piece cr_front laid out, the scan of the output lengths where the caller gathers (piece_out: its
// total), the guards, and the piece's totals added to f.st.  The stream is idle afterwards.
static int cr_totals(ScCall& s, CrCall& f, const CrLay& lay, u64* piece_out_p) {
  mk_ctx* c = s.c;
  const size_t nrows = s.last.nrows, seq_len = s.last.seq_len;
  size_t tmp = lay.scan_bytes;
  const mk_screen_row_t* d_rows = s.last.d_rows;
  CrStatus* d_st = lay.d_st;
  u64 *len = lay.len, *dst = lay.dst, *slen = lay.slen;
  const u64 *sstart = lay.sstart, *hlen = lay.hlen;
  const mk_correct_row_t* d_fix = lay.d_fix;
  CrStatus h{};
  // (the lengths are only added up before the guards below have passed: no address is made of them)
  hipLaunchKernelGGL(cr_decide_k, dim3(grid_for(nrows + 1, 256, 4096)), dim3(256), 0, c->stream, d_rows, (const u64*)sstart,
                     (const u64*)hlen, (const mk_correct_row_t*)d_fix, nrows, (u64)c->k, (u64)seq_len, slen, len, d_st);
  MK_HIP(hipGetLastError());
  if (piece_out_p)
    MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nrows + 1, rocprim::plus<u64>(), c->stream));
  u64 piece_out = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  if (piece_out_p) MK_HIP(hipMemcpyAsync(&piece_out, dst + nrows, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if (h.locked) {
    c->err = std::string(s.what) + ": a slot of the table was being claimed: something counts into it during the call";
    return MK_ERR_STATE;
  }
  if (h.disagree || h.outside || h.fixed + h.ambiguous + h.unfixable != h.ncand) {
    c->err = std::string(s.what) + ": the runs or the length of " + std::to_string(h.disagree) + " record(s) contradict their rows, " +
             std::to_string(h.outside) + " candidate(s) outside their records, " + std::to_string(h.ncand) + " candidates with " +
             std::to_string(h.fixed + h.ambiguous + h.unfixable) + " outcomes (internal error)";
    return MK_ERR_STATE;
  }
  if (piece_out_p) *piece_out_p = piece_out;
  f.st.records += nrows;
  f.st.runs += h.runs;
  f.st.fixed += h.fixed;
  f.st.ambiguous += h.ambiguous;
  f.st.unfixable += h.unfixable;
  f.st.bases += h.bases;
  return MK_OK;
}

// fix and rows of the piece, whose rows start at row `first` of the call, where the caller has room for them.
static int cr_rows_out(ScCall& s, CrCall& f, const CrLay& lay, size_t first) {
  mk_ctx* c = s.c;
  const size_t nrows = s.last.nrows;
  const mk_screen_row_t* d_rows = s.last.d_rows;
  const mk_correct_row_t* d_fix = lay.d_fix;
  if (first + nrows <= f.cap) {
    const auto t1 = MkClock::now();
    const hipMemcpyKind kind = f.device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + first, d_rows, nrows * sizeof(mk_screen_row_t), kind, c->stream));
    if (f.fix) MK_HIP(hipMemcpyAsync(f.fix + first, d_fix, nrows * sizeof(mk_correct_row_t), kind, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (!f.device) f.st.s_write += mk_since(t1);
  }
  return MK_OK;
}

// What follows sc_piece for a piece of n bytes whose rows start at row `first` of the call and which holds `windows`
// windows, `hits` of them solid: placement, the weak runs, the lengths, the gather, and the copies to the caller's
// buffers where they have room.  The stream is idle afterwards.
static int cr_piece(ScCall& s, CrCall& f, size_t n, size_t first, u64 windows, u64 hits) {
  mk_ctx* c = s.c;
  int rc;
  const size_t nrows = s.last.nrows;
  if (!nrows) {  // (no header line, no kept character)
    f.st.preamble += n;
    return MK_OK;
  }
  CrLay lay{};
  u64 piece_out = 0;
  if ((rc = cr_front(s, f, n, windows, hits, lay)) != MK_OK) return rc;
  if ((rc = cr_totals(s, f, lay, &piece_out)) != MK_OK) return rc;
  if (lay.start0 > n || piece_out > n - lay.start0 + 1) {
    c->err = std::string(s.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.preamble += lay.start0;
  if ((rc = cr_rows_out(s, f, lay, first)) != MK_OK) return rc;
  const TrPlace p{s.last.text, (u64)n, (const uint8_t*)c->seq.p, (u64)s.last.seq_len, lay.start, lay.sstart, lay.hlen, lay.slen,
                  lay.dst, nrows};
  return tr_emit(s, f.emit, p, piece_out, f.st.s_gather, f.st.s_write);
}
