// mk_trackwalk.h -- the count under every window of a piece, placed and written, and the median of every record's
// counts: what mk_track_* (mk_track.hip: the counts go to the caller) and mk_norm_* (mk_norm.hip: the counts stay in
// device scratch, only the medians are used) share; mk_correct_* (mk_correct.hip) takes the placement and tk_probe_k for
// the counts its runs are read from.  tk_lens_k and the scan give woff[]; tk_probe_k is the walk of
// mk_screenwalk.h with the positional sink; tk_median sorts the short records' counts a segment a record
// (rocprim::segmented_radix_sort_keys, tk_pick_k) and finds the median of a LONG record -- more than
// MK_MEDIAN_SELECT_MIN windows -- by radix selection in place (tk_longest_k, tk_long_k, tk_sel_hist_k, tk_sel_pick_k).
// The kernels that are no templates are static: every file that includes them launches its own copy.
//
// Selection.  One segment of the segmented sort runs at 2.9 ns an element: a contig's median cost more
// than its track.  A long record gets an empty segment instead (wend[r] = woff[r]) and a slot: (prefix, rank) = (0,
// windows / 2) and 256 bins.  The bits the sort would sort (end_bit, rounded up to whole bytes) are fixed from the most
// significant byte down, a pass a byte: tk_sel_hist_k reads the piece's elements tile by tile, skips what is no long
// record, counts the elements whose upper bytes equal the slot's prefix by their next byte -- in LDS, then the non-zero
// bins to the slot's global bins -- and tk_sel_pick_k, a lane a slot, finds the bin that holds the rank, appends it to
// the prefix, takes the elements in front of it off the rank and clears the bins.  After the last pass the prefix is
// element `rank` of the sorted record: the median.  At most four passes over 4 bytes an element (eight for uint64_t)
// and nothing is copied.  A tile of TK_SEL_SPAN elements overlaps at most two long records, because a long record is
// longer than a tile: the one that holds its first element and the one that holds its last.
#pragma once
#include "mk_screenwalk.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

struct TkStatus {  // device memory, read back once a piece
  u64 max_count, written, saturated;
  u64 longest;  // the windows of the piece's longest record where that is a long one, else 0 (tk_longest_k)
};

// The draw of the calls that thin by the median (mk_norm.hip, mk_pairs.hip): the upper 32 bits of splitmix64 of record
// r (its index over the whole call) under seed.
__device__ __forceinline__ u64 nm_u(u64 seed, u64 r) {
  u64 z = seed + (r + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z >> 32;
}

// wlen[r] = windows of row r, wlen[nrows] = 0 (so that the scan ends in the total); the largest count of the piece.
static __global__ void __launch_bounds__(256) tk_lens_k(const mk_screen_row_t* __restrict__ rows, size_t nrows, u64* __restrict__ wlen,
                                                        TkStatus* __restrict__ st) {
  u64 mx = 0;
  mk_for_each(nrows + 1, [&](size_t r) {
    if (r == nrows) { wlen[r] = 0; return; }
    wlen[r] = rows[r].windows;
    mx = rows[r].max > mx ? rows[r].max : mx;
  });
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = __shfl_down(mx, d);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx) atomicMax((unsigned long long*)&st->max_count, mx);
}

template <class E>
__global__ void __launch_bounds__(256) tk_pick_k(const E* __restrict__ sorted, const u64* __restrict__ woff, size_t nrows,
                                                 E* __restrict__ median) {
  mk_for_each(nrows, [&](size_t r) {
    const u64 w = woff[r + 1] - woff[r];
    median[r] = w ? sorted[woff[r] + w / 2] : (E)0;
  });
}

// The positional sink of the walk.  s_out: SC_SPAN elements of LDS, element i of the piece at i % SC_SPAN; total: the
// piece's windows (woff[nrows]).  An element whose record or place lies outside what the placement counted is dropped,
// never written -- the host compares st->written with the total.
template <class E>
struct TkSink {
  E* s_out;
  const u64* __restrict__ woff;
  const u64* __restrict__ sstart;
  u64 row_base, nrows, total;
  u64 at_rid0 = ~0ull, ahead = 0;       // that record; symbols of the record the lane's run started in that lie in front of the run
  u64 at_rid = ~0ull, at_base = 0;      // the record whose woff this lane holds
  u64 first = ~0ull, last = 0, sat = 0, written = 0;
  __device__ __forceinline__ void begin(u64 rid, u64 at) {
    const u64 r = rid - row_base;
    if (r < nrows && sstart[r] <= at) ahead = at - sstart[r];
    at_rid0 = rid;
  }
  __device__ __forceinline__ void record_end(u64) {}
  __device__ __forceinline__ void window(u64 rid, unsigned pos, u64 cnt) {
    if (rid != at_rid) {
      at_rid = rid;
      const u64 r = rid - row_base;
      at_base = r < nrows ? woff[r] : total;
    }
    const u64 i = at_base + (rid == at_rid0 ? ahead : 0) + pos;  // (a record may end inside the k - 1 symbols that fill the key)
    if (i >= total) return;
    E v = (E)cnt;
    if (sizeof(E) == 4 && cnt > 0xFFFFFFFFull) { v = (E)0xFFFFFFFFu; ++sat; }
    ++written;
    s_out[i & (SC_SPAN - 1)] = v;
    if (first == ~0ull) first = i;  // (the places of a lane ascend)
    last = i + 1;
  }
};

// Grid and arguments of sc_probe_k; dynamic LDS: the span (sc_span_bytes(k), none when LDS is false), then SC_SPAN
// elements.
template <int KEYS, bool FOLD, bool LDS, class E>
__global__ void __launch_bounds__(256) tk_probe_k(const uint8_t* __restrict__ seq, u64 seq_len, const u64* __restrict__ tile_pre,
                                                  u64 row_base, int k, int bits, LkTables t, const u64* __restrict__ woff,
                                                  const u64* __restrict__ sstart, u64 nrows, u64 total, E* __restrict__ out, TkStatus* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  __shared__ unsigned long long s_lo, s_hi;
  const unsigned span_bytes = LDS ? sc_span_bytes(k) : 0u;
  if (threadIdx.x == 0) { s_lo = ~0ull; s_hi = 0; }  // (the walk's barriers stand between this and the atomics)
  TkSink<E> sink{reinterpret_cast<E*>(s_dyn + span_bytes), woff, sstart, row_base, nrows, total};
  ScWalked n;
  sc_walk<KEYS, FOLD, LDS>(s_dyn, seq, seq_len, tile_pre, k, bits, t, sink, n);
  // The tile's range: its windows are at most SC_SPAN consecutive places, so no two share an LDS element.
  if (sink.last) {
    atomicMin(&s_lo, (unsigned long long)sink.first);
    atomicMax(&s_hi, (unsigned long long)sink.last);
  }
  __syncthreads();
  const u64 lo = s_lo, hi = s_hi;
  if (hi > lo && hi - lo <= SC_SPAN)
    for (u64 i = lo + threadIdx.x; i < hi; i += 256) out[i] = sink.s_out[i & (SC_SPAN - 1)];
  else sink.written = 0;
  block_add(&st->written, sink.written);
  if (sizeof(E) == 4) block_add(&st->saturated, sink.sat);
}

// ------------------------------------------------------------------------------------------ selection
#define TK_SEL_RUN 32                     // elements a lane of the histogram kernel owns
#define TK_SEL_SPAN (256 * TK_SEL_RUN)    // ... a workgroup: one tile of the piece's elements
static_assert(MK_MEDIAN_SELECT_MIN >= TK_SEL_SPAN, "a long record must be longer than a tile of the selection");

struct TkSelStatus {  // device memory, read back once a piece
  u64 short_windows;  // windows of the records the sort still takes
  unsigned nlong, pad;
};
struct TkSlot {  // a long record's selection: the bytes fixed so far and the rank among the elements that share them
  u64 prefix, rank;
  u64 rec;
};

// The windows of the piece's longest record, from the scanned offsets, where it is a long one: what tells the host, in
// the read-back it makes anyway, whether the piece holds a long record at all.
static __global__ void __launch_bounds__(256) tk_longest_k(const u64* __restrict__ woff, size_t nrows, TkStatus* __restrict__ st) {
  u64 mx = 0;
  mk_for_each(nrows, [&](size_t r) {
    const u64 w = woff[r + 1] - woff[r];
    mx = w > mx ? w : mx;
  });
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = __shfl_down(mx, d);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx > MK_MEDIAN_SELECT_MIN) atomicMax((unsigned long long*)&st->longest, mx);
}

// A lane a record: wend[r], the end of its segment of the sort -- its start for a long record, which gets a slot.
static __global__ void __launch_bounds__(256) tk_long_k(const u64* __restrict__ woff, size_t nrows, u64* __restrict__ wend,
                                                        unsigned* __restrict__ slot_of, TkSlot* __restrict__ slots, unsigned max_slots,
                                                        TkSelStatus* __restrict__ st) {
  u64 shorts = 0;
  mk_for_each(nrows, [&](size_t r) {
    const u64 b = woff[r], w = woff[r + 1] - b;
    unsigned slot = ~0u;
    if (w > MK_MEDIAN_SELECT_MIN) {
      slot = atomicAdd(&st->nlong, 1u);
      if (slot < max_slots) slots[slot] = TkSlot{0, w / 2, (u64)r};  // (more than max_slots cannot be: they would hold more than the piece)
      else slot = ~0u;
    }
    if (slot == ~0u) shorts += w;
    slot_of[r] = slot;
    wend[r] = slot == ~0u ? b + w : b;
  });
  block_add(&st->short_windows, shorts);
}

// The record that holds element x of the piece: the largest r with woff[r] <= x (a record without windows has
// woff[r] == woff[r + 1] and is never the largest).
__device__ __forceinline__ size_t tk_record_of(const u64* __restrict__ woff, size_t nrows, u64 x) {
  size_t lo = 0, hi = nrows - 1;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (woff[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One pass of the selection over tile blockIdx.x of the piece's elements: shift = the place of the byte this pass fixes.
// An element counts for its record's slot iff its bits above that byte equal the slot's prefix.  Four consecutive
// elements a lane and round (one 16-byte load of uint32_t where `in` is aligned to 16), a wave instruction 1 KiB.  Where
// every counting lane of a wave holds the same byte -- all of them in a homopolymer or a contig the table lacks, most of
// them in the upper bytes of any record -- one lane adds the wave's number; else each lane adds 1.
template <class E>
__global__ void __launch_bounds__(256) tk_sel_hist_k(const E* __restrict__ in, const u64* __restrict__ woff, size_t nrows, u64 total,
                                                     const unsigned* __restrict__ slot_of, const TkSlot* __restrict__ slots,
                                                     unsigned* __restrict__ bins, unsigned shift) {
  __shared__ unsigned s_bin[256];
  const u64 t0 = (u64)blockIdx.x * TK_SEL_SPAN, t1 = t0 + TK_SEL_SPAN < total ? t0 + TK_SEL_SPAN : total;
  const size_t ra = tk_record_of(woff, nrows, t0), rb = tk_record_of(woff, nrows, t1 - 1);
  const bool vec = sizeof(E) == 4 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
  for (int side = 0; side < 2; ++side) {
    const size_t r = side ? rb : ra;
    if (side && rb == ra) break;
    const unsigned slot = slot_of[r];
    if (slot == ~0u) continue;  // (the same for the whole workgroup)
    const u64 lo = woff[r] > t0 ? woff[r] : t0, hi = woff[r + 1] < t1 ? woff[r + 1] : t1;
    const u64 prefix = slots[slot].prefix;
    s_bin[threadIdx.x] = 0;
    __syncthreads();
    for (int j = 0; j < TK_SEL_RUN / 4; ++j) {
      const u64 e0 = t0 + (u64)j * 1024 + threadIdx.x * 4u;
      if (__all(e0 >= hi || e0 + 4 <= lo)) continue;
      E v[4] = {0, 0, 0, 0};
      if (vec && e0 + 4 <= total) {
        const uint4 q = *reinterpret_cast<const uint4*>(in + e0);
        v[0] = (E)q.x; v[1] = (E)q.y; v[2] = (E)q.z; v[3] = (E)q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (e0 + i < total) v[i] = in[e0 + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u64 x = (u64)v[i];
        const u64 upper = shift + 8 >= 64 ? 0 : x >> (shift + 8);
        const bool on = e0 + i >= lo && e0 + i < hi && upper == prefix;
        const unsigned b = (unsigned)(x >> shift) & 255u;
        const unsigned long long m = __ballot(on);
        if (!m) continue;
        const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((int)b, __ffsll((long long)m) - 1);
        if (__all(!on || b == b0)) {
          if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&s_bin[b0], (unsigned)__popcll(m));
        } else if (on) atomicAdd(&s_bin[b], 1u);
      }
    }
    __syncthreads();
    const unsigned c = s_bin[threadIdx.x];
    if (c) atomicAdd(&bins[(size_t)slot * 256 + threadIdx.x], c);
    __syncthreads();
  }
}

// A lane a slot: the bin that holds the rank.  last: the prefix is the record's median.
template <class E>
__global__ void __launch_bounds__(256) tk_sel_pick_k(TkSlot* __restrict__ slots, unsigned nslots, unsigned* __restrict__ bins, bool last,
                                                     E* __restrict__ median) {
  mk_for_each(nslots, [&](size_t s) {
    unsigned* b = bins + s * 256;
    TkSlot t = slots[s];
    u64 before = 0;
    unsigned at = 255;
    bool found = false;
    for (unsigned i = 0; i < 256; ++i) {
      const u64 c = b[i];
      b[i] = 0;
      if (!found && before + c > t.rank) { at = i; found = true; }
      if (!found) before += c;
    }
    t.prefix = (t.prefix << 8) | at;
    t.rank -= before;
    slots[s] = t;
    if (last) median[t.rec] = (E)t.prefix;
  });
}

// ------------------------------------------------------------------------------------------ host side
template <class E>
static int tk_launch_probe(ScCall& s, const u64* woff, const u64* sstart, size_t nrows, u64 total, E* d_out, TkStatus* d_st) {
  mk_ctx* c = s.c;
  const LkTables t = lk_tables(c);
  const unsigned grid = (unsigned)div_up(s.last.seq_len, SC_SPAN);
  const int rc = sc_dispatch_walk(s, [&](auto keys, auto fold, auto lds) -> int {
    auto kern = tk_probe_k<decltype(keys)::value, decltype(fold)::value, decltype(lds)::value, E>;
    const size_t shmem = (decltype(lds)::value ? sc_span_bytes(c->k) : 0) + (size_t)SC_SPAN * sizeof(E);
    static size_t raised[64];  // per instantiation and device: the dynamic LDS the kernel has been allowed so far
    if (shmem > 64 * 1024 && shmem > raised[c->device & 63]) {
      MK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
      raised[c->device & 63] = shmem;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), shmem, c->stream, (const uint8_t*)c->seq.p, (u64)s.last.seq_len, s.last.tile_pre,
                       s.last.row_base, c->k, c->bits, t, woff, sstart, (u64)nrows, total, d_out, d_st);
    return MK_OK;
  });
  if (rc != MK_OK) return rc;
  MK_HIP(hipGetLastError());
  return MK_OK;
}

struct TkMedian {  // the median's working memory: lives as long as the call
  MkDevBuf sorted, sort_tmp, sel;
  ~TkMedian() {
    for (MkDevBuf* b : {&sorted, &sort_tmp, &sel}) buf_free(*b);
  }
};

// The medians of the piece's `total` elements at d_in (fewer than 2^32), a record r at [woff[r], woff[r + 1]), into
// d_med: the short records sorted into f.sorted, a segment a record, and picked; the long ones selected.  longest: what
// tk_longest_k left (0: no record is long); a piece without a long record goes the way it always went, launch for launch.
template <class E>
static int tk_median(mk_ctx* c, TkMedian& f, const E* d_in, const u64* woff, size_t nrows, u64 total, u64 max_count, u64 longest,
                     E* d_med) {
  int rc;
  unsigned end_bit = 1;  // (the bits the largest count of the piece has: small counts sort in one or two passes)
  while (end_bit < 8 * sizeof(E) && (max_count >> end_bit)) ++end_bit;
  const u64* wend = woff + 1;
  TkSelStatus h{total, 0, 0};
  unsigned* slot_of = nullptr;
  TkSlot* slots = nullptr;
  unsigned* bins = nullptr;
  if (longest > MK_MEDIAN_SELECT_MIN) {
    // sel: TkSelStatus (16) | wend[nrows] | slots[max_slots] | bins[max_slots][256] | slot_of[nrows]
    const size_t max_slots = (size_t)(total / ((u64)MK_MEDIAN_SELECT_MIN + 1));
    if ((rc = mk_buf_reserve(c, f.sel, 16 + nrows * sizeof(u64) + max_slots * (sizeof(TkSlot) + 256 * sizeof(unsigned)) + nrows * sizeof(unsigned))) != MK_OK) return rc;
    TkSelStatus* d_sel = (TkSelStatus*)f.sel.p;
    u64* d_wend = (u64*)((char*)f.sel.p + 16);
    slots = (TkSlot*)(d_wend + nrows);
    bins = (unsigned*)(slots + max_slots);
    slot_of = bins + max_slots * 256;
    MK_HIP(hipMemsetAsync(d_sel, 0, sizeof(TkSelStatus), c->stream));
    hipLaunchKernelGGL(tk_long_k, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, woff, nrows, d_wend, slot_of, slots,
                       (unsigned)max_slots, d_sel);
    MK_HIP(hipGetLastError());
    MK_HIP(hipMemcpyAsync(&h, d_sel, sizeof h, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (h.nlong > max_slots) { c->err = "the median: more long records than the piece can hold (internal error)"; return MK_ERR_STATE; }
    if (h.nlong) {
      wend = d_wend;
      MK_HIP(hipMemsetAsync(bins, 0, (size_t)h.nlong * 256 * sizeof(unsigned), c->stream));
    }
  }
  if (h.short_windows || !h.nlong) {
    if (total) {
      if ((rc = mk_buf_reserve(c, f.sorted, (size_t)total * sizeof(E))) != MK_OK) return rc;
      size_t tmp = 0;
      MK_HIP(rocprim::segmented_radix_sort_keys(nullptr, tmp, d_in, (E*)f.sorted.p, (unsigned)total, (unsigned)nrows, woff, wend, 0u,
                                                end_bit, c->stream));
      if ((rc = mk_buf_reserve(c, f.sort_tmp, tmp ? tmp : 16)) != MK_OK) return rc;
      MK_HIP(rocprim::segmented_radix_sort_keys(f.sort_tmp.p, tmp, d_in, (E*)f.sorted.p, (unsigned)total, (unsigned)nrows, woff, wend,
                                                0u, end_bit, c->stream));
    }
    // (a long record's pick reads an element of f.sorted that nothing wrote; its median is overwritten below)
    hipLaunchKernelGGL(tk_pick_k<E>, dim3(grid_for(nrows, 256, 4096)), dim3(256), 0, c->stream, (const E*)f.sorted.p, woff, nrows, d_med);
    MK_HIP(hipGetLastError());
  } else MK_HIP(hipMemsetAsync(d_med, 0, nrows * sizeof(E), c->stream));  // (every record with windows is long)
  if (h.nlong) {
    const unsigned grid = (unsigned)div_up((size_t)total, TK_SEL_SPAN);
    for (int pass = (int)(end_bit + 7) / 8 - 1; pass >= 0; --pass) {
      hipLaunchKernelGGL(tk_sel_hist_k<E>, dim3(grid), dim3(256), 0, c->stream, d_in, woff, nrows, total, (const unsigned*)slot_of,
                         (const TkSlot*)slots, bins, 8u * (unsigned)pass);
      hipLaunchKernelGGL(tk_sel_pick_k<E>, dim3(grid_for(h.nlong, 256, 4096)), dim3(256), 0, c->stream, slots, h.nlong, bins, pass == 0,
                         d_med);
    }
    MK_HIP(hipGetLastError());
  }
  return MK_OK;
}
