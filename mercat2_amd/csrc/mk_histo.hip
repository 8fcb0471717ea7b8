// mk_histo.hip -- the abundance spectrum of the table a context holds (mk_histo*, include/mercat_hip.h): how many
// distinct k-mers occur once, twice, ... `high` times, and how many more often (what Jellyfish calls `histo`).
//
// One kernel template over the slot views of mk_tableview.h, one launch per table the context holds (mk_each_table);
// the one key kept beside the one-word table (run_side) is added by the host.  The same pass reduces the rows, the sum
// of the counts, the largest count and the sum of the counts above `high`.  Everything is an integer add: the result is
// exact and does not depend on the order of the slots or of the workgroups.
//
// Where the bins live.  A k-mer spectrum is skewed: nearly every row of a shallow sample has count 1, most rows of a deep
// one sit within a few bins of the coverage peak.  The low HS_WINDOW bins are private to the workgroup, u32 words in
// LDS, and only those that are not zero are added to the global bins when the workgroup ends; counts from HS_WINDOW up to
// `high` are rare and go to the global bins at once; counts above `high` are counted in registers.
#include "mk_tableview.h"
#include <string.h>

// Low bins a workgroup keeps in LDS.  8 KiB a workgroup: the eight workgroups of 256 threads a CU can hold take 64 of its
// 160 KiB, so the LDS never decides how many waves read the table -- the table read is the only HBM traffic.  A u32 bin
// cannot wrap: a workgroup would have to read 2^32 slots, 32 GiB of the smallest of them, of a table that 2048 of
// them share.
#define HS_WINDOW 2048
// Every lane adds its own 1 (ds_add_u32).  Folding equal bins inside a wave first -- the first lane's bin broadcast, a
// ballot of the lanes that share it, one add of the popcount -- was built and timed: two rounds of it are within noise
// of this form on a spread spectrum and on a table of singletons only, folding every bin is 1.7x slower on the spread
// one.
#define HS_GRID 2048  // workgroups at most: eight on each of the 256 CUs

enum { HS_ROWS = 0, HS_TOTAL, HS_MAX, HS_OVER_ROWS, HS_OVER_TOTAL, HS_WORDS = 8 };

template <class View>
__global__ __launch_bounds__(256) void hs_scan_k(View v, size_t n, u64 high, u64* __restrict__ bins, u64* __restrict__ out) {
  __shared__ unsigned s_bins[HS_WINDOW];
  __shared__ unsigned long long s_out[HS_WORDS];
  for (unsigned b = threadIdx.x; b < HS_WINDOW; b += 256) s_bins[b] = 0;
  if (threadIdx.x < HS_WORDS) s_out[threadIdx.x] = 0;
  __syncthreads();
  u64 rows = 0, total = 0, top = 0, over_rows = 0, over_total = 0;
  mk_for_each(n, [&](size_t i) {
    u64 a, b, c;
    if (!v.get(i, a, b, c)) return;
    rows += 1;
    total += c;
    top = c > top ? c : top;
    if (c > high) { over_rows += 1; over_total += c; }
    else if (c < HS_WINDOW) atomicAdd(&s_bins[c], 1u);
    else atomicAdd(&bins[c], 1ull);  // HS_WINDOW <= c <= high: rare
  });
  for (int d = 32; d > 0; d >>= 1) {
    rows += __shfl_down(rows, d);
    total += __shfl_down(total, d);
    over_rows += __shfl_down(over_rows, d);
    over_total += __shfl_down(over_total, d);
    const u64 other = __shfl_down(top, d);
    top = other > top ? other : top;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s_out[HS_ROWS], (unsigned long long)rows);
    atomicAdd(&s_out[HS_TOTAL], (unsigned long long)total);
    atomicMax(&s_out[HS_MAX], (unsigned long long)top);
    atomicAdd(&s_out[HS_OVER_ROWS], (unsigned long long)over_rows);
    atomicAdd(&s_out[HS_OVER_TOTAL], (unsigned long long)over_total);
  }
  __syncthreads();
  for (unsigned b = threadIdx.x; b < HS_WINDOW; b += 256)  // (a bin that is not zero is the count of a row, <= high: within bins[])
    if (s_bins[b]) atomicAdd(&bins[b], (u64)s_bins[b]);
  if (threadIdx.x < HS_WORDS && s_out[threadIdx.x]) {
    if (threadIdx.x == HS_MAX) atomicMax(&out[HS_MAX], (u64)s_out[HS_MAX]);
    else atomicAdd(&out[threadIdx.x], (u64)s_out[threadIdx.x]);
  }
  if (threadIdx.x == 0 && s_out[HS_OVER_ROWS]) atomicAdd(&bins[high + 1], (u64)s_out[HS_OVER_ROWS]);
}

// ------------------------------------------------------------------------------------------ host side
// Every table of the context; *slots: table slots read.
static int hs_launch_all(mk_ctx* c, u64 high, u64* d_bins, u64* d_out, u64* slots) {
  return mk_each_table(c, [&](auto v, size_t n, int) -> int {
    hipLaunchKernelGGL(hs_scan_k<decltype(v)>, dim3(grid_for(n, 256, HS_GRID)), dim3(256), 0, c->stream, v, n, high, d_bins, d_out);
    MK_HIP(hipGetLastError());
    *slots += n;
    return MK_OK;
  });
}

#define HS_MAX_HIGH ((uint64_t)1 << 20)

// The histogram into d_bins (device memory of the context's GPU), or with d_bins == NULL into the context's scratch and
// from there into h_bins.
static int hs_run(mk_ctx* c, const char* what, uint64_t high, u64* d_bins, uint64_t* h_bins, mk_histo_t* st) {
  const auto t0 = MkClock::now();
  MK_REFUSE_SPOILED(c, what);
  if (c->in_chunk) { c->err = std::string(what) + ": a chunk is open"; return MK_ERR_STATE; }
  if (high < 1 || high > HS_MAX_HIGH) { c->err = std::string(what) + ": high must lie in 1 .. 2^20"; return MK_ERR_ARG; }
  if (!d_bins && !h_bins) { c->err = std::string(what) + ": bins is NULL"; return MK_ERR_ARG; }
  MK_SETTLE(c);
  MK_HIP(hipSetDevice(c->device));
  const size_t words = (size_t)high + 2;
  int rc;
  if ((rc = mk_buf_reserve(c, c->ex_tmp, (HS_WORDS + (d_bins ? 0 : words)) * sizeof(u64))) != MK_OK) return rc;
  u64* d_out = (u64*)c->ex_tmp.p;
  if (!d_bins) d_bins = d_out + HS_WORDS;
  MkTimed scan(c);
  u64 h[HS_WORDS] = {0}, slots = 0;
  double s_scan = 0;
  const u64 side = c->run_side;  // the one key kept beside the one-word table (32 x 'T')
  rc = [&]() -> int {
    int r;
    MK_HIP(hipMemsetAsync(d_out, 0, HS_WORDS * sizeof(u64), c->stream));
    MK_HIP(hipMemsetAsync(d_bins, 0, words * sizeof(u64), c->stream));
    // (its row: the low half of a cleared bin set to 1, ahead of the kernels' adds)
    if (side) MK_HIP(hipMemsetD32Async((hipDeviceptr_t)(d_bins + (side > high ? high + 1 : side)), 1, 1, c->stream));
    if ((r = scan.begin()) != MK_OK || (r = hs_launch_all(c, high, d_bins, d_out, &slots)) != MK_OK || (r = scan.end()) != MK_OK)
      return r;
    MK_HIP(hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (h_bins) MK_HIP(hipMemcpyAsync(h_bins, d_bins, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    return scan.add_to(s_scan);
  }();
  if (rc != MK_OK) { (void)hipStreamSynchronize(c->stream); return rc; }  // (nothing of the call is left in flight)
  if (!st) return MK_OK;
  memset(st, 0, sizeof *st);
  st->distinct = h[HS_ROWS] + (side ? 1 : 0);
  st->total = h[HS_TOTAL] + side;
  st->max_count = side > h[HS_MAX] ? side : h[HS_MAX];
  st->over_rows = h[HS_OVER_ROWS] + (side > high ? 1 : 0);
  st->over_total = h[HS_OVER_TOTAL] + (side > high ? side : 0);
  st->slots = slots;
  st->s_scan = s_scan;
  st->s_total = mk_since(t0);
  return MK_OK;
}

extern "C" int mk_histo(mk_ctx* c, uint64_t high, uint64_t* bins, mk_histo_t* st) {
  if (!c) return MK_ERR_ARG;
  return hs_run(c, "mk_histo", high, nullptr, bins, st);
}

extern "C" int mk_histo_device(mk_ctx* c, uint64_t high, uint64_t* d_bins, mk_histo_t* st) {
  if (!c) return MK_ERR_ARG;
  if (!d_bins) { c->err = "mk_histo_device: d_bins is NULL"; return MK_ERR_ARG; }
  return hs_run(c, "mk_histo_device", high, (u64*)d_bins, nullptr, st);
}
