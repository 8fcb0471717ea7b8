// mk_beta.hip -- per-pair statistics of n samples' count columns over the union of their k-mers: everything the
// 21 distance matrices of MerCat2's beta diversity (lib/mercat2_diversity.py:56-105, scipy's pdist through
// scikit-bio) are closed forms of.  The host finishes in n x n (mercat2_amd/diversity.py, beta_from_stats).
//
// Join: the one mk_gram uses (mk_join.h); every dense rows x n slab goes through two kernels here.
//
// Row pre-pass (one thread per union row): V_r, the variance of the row's n counts with ddof = 1 in f64 as numpy
// computes it (mean, then the sum of squared deviations), stored as 1 / V_r; a flag bit when some row holds the
// same count in all n samples (an integer compare: V_r = 0 there and seuclidean is NaN); and whether a count of
// the slab reaches 2^32.
//
// Pair kernel: a workgroup stages blocks of R contiguous rows (and their 1 / V_r) through LDS.  A pair tile holds
// T = min(P, 256) of the P = n (n + 1) / 2 pairs i <= j; the workgroup's 256 threads are G = floor(256 / T) groups
// of T, group g taking rows g, g + G, ... of each block, so a few samples still keep most lanes busy.  Each thread
// accumulates, for its pair: sum x y (the exact 32 x 32 -> 64 product when no count of the slab reaches 2^32,
// else 64 x 64 -> 128), sum |x - y| (128-bit), max |x - y|, #{x != y}, #{x != 0 and y != 0}, and in f64, as
// scipy's C loops do (convert, subtract, IEEE divide; no contraction): sum |x - y| / (x + y) over x + y > 0 and
// sum (x - y)^2 / V_r.  A diagonal pair's sum |x - y| is zero; its thread adds x there instead, which is the
// column sum S_i (taken out again by finish()).  The G groups are reduced in LDS in group order, the workgroups'
// partials by a second kernel in block order, the slabs in slab order: integer fields do not depend on the order
// at all, f64 fields are the same bits for the same input, device and slab size.  No floating-point atomics.
#include "mk_join.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;          // threads per workgroup of the pair kernel
constexpr size_t kLdsBytes = 32768;    // staged rows per block: R = kLdsBytes / (8 (n + 1))
constexpr unsigned kGridTarget = 2048; // workgroups per pair launch (row blocks x pair tiles)

static_assert(sizeof(mk_pair_t) == 72, "mk_pair_t: 7 u64 and 2 f64");

__device__ __host__ inline void pair_merge(mk_pair_t& a, const mk_pair_t& b) {
  a.dot[0] += b.dot[0];
  a.dot[1] += b.dot[1] + (a.dot[0] < b.dot[0] ? 1 : 0);
  a.l1[0] += b.l1[0];
  a.l1[1] += b.l1[1] + (a.l1[0] < b.l1[0] ? 1 : 0);
  a.cheb = a.cheb > b.cheb ? a.cheb : b.cheb;
  a.neq += b.neq;
  a.both += b.both;
  a.canb += b.canb;
  a.seuc += b.seuc;
}

// inv[r] = 1 / var(row r, ddof = 1); flags[0] |= 1 when a count reaches 2^32, flags[1] |= 1 when a row is constant
__global__ __launch_bounds__(256) void mk_beta_rows_k(const u64* __restrict__ x, size_t rows, int n, double* __restrict__ inv,
                                                     unsigned* __restrict__ flags) {
  const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  bool wide = false, same = false;
  if (r < rows) {
    const u64* row = x + r * (size_t)n;
    const u64 first = row[0];
    u64 any = 0;
    bool eq = true;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      const u64 v = row[i];
      any |= v;
      eq = eq && v == first;
      s += (double)v;
    }
    const double mean = s / (double)n;
    double q = 0.0;
    for (int i = 0; i < n; ++i) {
      const double d = (double)row[i] - mean;
      q += d * d;
    }
    inv[r] = 1.0 / (q / (double)(n - 1));  // (n = 1: NaN; pdist of one sample has no pairs)
    wide = (any >> 32) != 0;
    same = eq;
  }
  const bool lead = (threadIdx.x & (warpSize - 1)) == 0;
  if (__any(wide) && lead) atomicOr(&flags[0], 1u);
  if (__any(same) && lead) atomicOr(&flags[1], 1u);
}

// ws[blockIdx.x * P + p] = this workgroup's statistics of pair p = blockIdx.y * T + (thread % T)
template <bool WIDE>
__global__ __launch_bounds__(kThreads) void mk_beta_pair_k(const u64* __restrict__ x, const double* __restrict__ inv, size_t rows,
                                                          int n, int R, const unsigned* __restrict__ pairs, int P, int T, int G,
                                                          mk_pair_t* __restrict__ ws) {
  extern __shared__ u64 tile[];  // R x n counts, R x 1 / V_r; at the end G x T partials
  double* tinv = (double*)(tile + (size_t)R * (size_t)n);
  const int g = (int)threadIdx.x / T, pl = (int)threadIdx.x - g * T;
  const int p = blockIdx.y * T + pl;
  const bool on = g < G && p < P;
  int i = 0, j = 0;
  if (on) { const unsigned ij = pairs[p]; i = (int)(ij & 0xffffu); j = (int)(ij >> 16); }
  const bool diag = i == j;
  u64 dlo = 0, dhi = 0, llo = 0, lhi = 0, cheb = 0, neq = 0, both = 0;
  double canb = 0.0, seuc = 0.0;
  const size_t nblk = (rows + (size_t)R - 1) / (size_t)R;
  for (size_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    const size_t r0 = b * (size_t)R;
    const int rr = (int)min((size_t)R, rows - r0);
    const size_t cnt = (size_t)rr * (size_t)n;
    const u64* src = x + r0 * (size_t)n;
    for (size_t t = threadIdx.x; t < cnt; t += kThreads) tile[t] = src[t];
    for (int t = threadIdx.x; t < rr; t += kThreads) tinv[t] = inv[r0 + t];
    __syncthreads();
    if (on) {
      for (int r = g; r < rr; r += G) {
        const u64 a = tile[(size_t)r * n + i], c = tile[(size_t)r * n + j];
        if (WIDE) {
          const u64 pl_ = a * c, ph = __umul64hi(a, c);
          dlo += pl_;
          dhi += ph + (dlo < pl_ ? 1 : 0);
        } else {
          const u64 pl_ = (u64)(unsigned)a * (u64)(unsigned)c;
          dlo += pl_;
          dhi += (dlo < pl_ ? 1 : 0);
        }
        const u64 d = a > c ? a - c : c - a;
        const u64 add = diag ? a : d;
        llo += add;
        lhi += (llo < add ? 1 : 0);
        cheb = d > cheb ? d : cheb;
        neq += a != c ? 1 : 0;
        both += (a != 0 && c != 0) ? 1 : 0;
        const double fa = (double)a, fc = (double)c;
        const double den = fa + fc;
        if (den > 0.0) canb += fabs(fa - fc) / den;
        const double t = fa - fc;
        seuc += t * t * tinv[r];
      }
    }
    __syncthreads();
  }
  mk_pair_t mine;
  mine.dot[0] = dlo; mine.dot[1] = dhi; mine.l1[0] = llo; mine.l1[1] = lhi;
  mine.cheb = cheb; mine.neq = neq; mine.both = both; mine.canb = canb; mine.seuc = seuc;
  if (G == 1) {
    if (on) ws[(size_t)blockIdx.x * (size_t)P + (size_t)p] = mine;
    return;
  }
  mk_pair_t* part = (mk_pair_t*)tile;  // (the last loop ended on a barrier: the tile is free)
  if (g < G) part[threadIdx.x] = mine;
  __syncthreads();
  if (on && g == 0) {
    for (int k = 1; k < G; ++k) pair_merge(mine, part[k * T + pl]);
    ws[(size_t)blockIdx.x * (size_t)P + (size_t)p] = mine;
  }
}

// acc[p] = acc[p] + ws[0][p] + ws[1][p] + ... (one thread per pair, in block order)
__global__ __launch_bounds__(256) void mk_beta_reduce_k(const mk_pair_t* __restrict__ ws, int blocks, int P, mk_pair_t* __restrict__ acc) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
    mk_pair_t s = ws[p];
    for (int b = 1; b < blocks; ++b) pair_merge(s, ws[(size_t)b * (size_t)P + (size_t)p]);
    mk_pair_t a = acc[p];
    pair_merge(a, s);
    acc[p] = a;
  }
}

// the same with one workgroup per pair (many workgroups' partials, few pairs): strided sums, then a fixed tree
__global__ __launch_bounds__(256) void mk_beta_reduce_wg_k(const mk_pair_t* __restrict__ ws, int blocks, int P, mk_pair_t* __restrict__ acc) {
  __shared__ mk_pair_t sh[256];
  const int p = blockIdx.x, t = threadIdx.x;
  mk_pair_t s = {};
  for (int b = t; b < blocks; b += 256) pair_merge(s, ws[(size_t)b * (size_t)P + (size_t)p]);
  sh[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) pair_merge(sh[t], sh[t + w]);
    __syncthreads();
  }
  if (t == 0) {
    mk_pair_t a = acc[p];
    pair_merge(a, sh[0]);
    acc[p] = a;
  }
}

// ------------------------------------------------------------------------------------- the accumulator
template <class C>
struct PairAcc {
  C* c;
  int device = 0, n = 0, P = 0, R = 1, T = 1, G = 1, tiles = 1;
  hipStream_t stream = nullptr;
  DevBuf pairs, acc, ws, flag, inv;  // flag: u32 [0] a count of the slab reaches 2^32, [1] some row is constant
  size_t inv_rows = 0;
  int ws_blocks = 0;

  int init(C* c_, int device_, hipStream_t stream_, int n_) {
    c = c_; device = device_; stream = stream_; n = n_;
    P = n * (n + 1) / 2;
    T = std::min(P, kThreads);
    G = kThreads / T;
    tiles = (P + T - 1) / T;
    R = (int)std::max<size_t>(1, std::min<size_t>(512, kLdsBytes / (8 * ((size_t)n + 1))));
    std::vector<unsigned> h((size_t)P);
    size_t at = 0;
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j) h[at++] = (unsigned)i | ((unsigned)j << 16);
    int rc;
    if ((rc = dev_alloc(c, pairs, device, (size_t)P * 4)) != MK_OK) return rc;
    if ((rc = dev_alloc(c, acc, device, (size_t)P * sizeof(mk_pair_t))) != MK_OK) return rc;
    if ((rc = dev_alloc(c, flag, device, 16)) != MK_OK) return rc;
    ws_blocks = (int)std::max<unsigned>(1, kGridTarget / (unsigned)tiles);
    if ((rc = dev_alloc(c, ws, device, (size_t)ws_blocks * (size_t)P * sizeof(mk_pair_t))) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(pairs.p, h.data(), (size_t)P * 4, hipMemcpyHostToDevice, stream));
    MK_HIP(hipMemsetAsync(acc.p, 0, (size_t)P * sizeof(mk_pair_t), stream));
    MK_HIP(hipMemsetAsync(flag.p, 0, 16, stream));
    return MK_OK;
  }

  // acc += the statistics of the dense rows x n matrix x (device memory on this device).  The row pre-pass finds
  // the wide flag itself, so flag_set (the join's scatter already set it) changes nothing.
  int add(const u64* x, size_t rows, bool flag_set = false) {
    (void)flag_set;
    if (!rows) return MK_OK;
    MK_HIP(hipSetDevice(device));
    int rc;
    if (rows > inv_rows) {
      MK_HIP(hipStreamSynchronize(stream));  // (the buffer may still be read by the last launch)
      if ((rc = dev_alloc(c, inv, device, rows * 8)) != MK_OK) return rc;
      inv_rows = rows;
    }
    MK_HIP(hipMemsetAsync(flag.p, 0, 4, stream));
    mk_beta_rows_k<<<grid1(rows), 256, 0, stream>>>(x, rows, n, inv.as<double>(), flag.as<unsigned>());
    MK_HIP(hipGetLastError());
    unsigned wide = 0;
    MK_HIP(hipMemcpyAsync(&wide, flag.p, 4, hipMemcpyDeviceToHost, stream));
    MK_HIP(hipStreamSynchronize(stream));
    const size_t nblk = (rows + (size_t)R - 1) / (size_t)R;
    const unsigned gx = (unsigned)std::min<size_t>((size_t)ws_blocks, nblk);
    const dim3 grid(gx, (unsigned)tiles);
    const size_t lds = std::max<size_t>((size_t)R * ((size_t)n + 1) * 8, (size_t)kThreads * sizeof(mk_pair_t));
    if (wide) mk_beta_pair_k<true><<<grid, kThreads, lds, stream>>>(x, inv.as<double>(), rows, n, R, pairs.as<unsigned>(), P, T, G, ws.as<mk_pair_t>());
    else mk_beta_pair_k<false><<<grid, kThreads, lds, stream>>>(x, inv.as<double>(), rows, n, R, pairs.as<unsigned>(), P, T, G, ws.as<mk_pair_t>());
    MK_HIP(hipGetLastError());
    if (gx >= 64) mk_beta_reduce_wg_k<<<(unsigned)P, 256, 0, stream>>>(ws.as<mk_pair_t>(), (int)gx, P, acc.as<mk_pair_t>());
    else mk_beta_reduce_k<<<std::min<unsigned>(grid1((size_t)P), 1024), 256, 0, stream>>>(ws.as<mk_pair_t>(), (int)gx, P, acc.as<mk_pair_t>());
    MK_HIP(hipGetLastError());
    return MK_OK;
  }

  // the full symmetric n x n matrix, the 128-bit column sums {lo, hi} and the flag word
  int finish(mk_pair_t* out, uint64_t* sums, uint64_t* flags) {
    std::vector<mk_pair_t> h((size_t)P);
    unsigned f[4] = {0, 0, 0, 0};
    MK_HIP(hipSetDevice(device));
    MK_HIP(hipMemcpyAsync(h.data(), acc.p, (size_t)P * sizeof(mk_pair_t), hipMemcpyDeviceToHost, stream));
    MK_HIP(hipMemcpyAsync(f, flag.p, 16, hipMemcpyDeviceToHost, stream));
    MK_HIP(hipStreamSynchronize(stream));
    size_t at = 0;
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j, ++at) {
        mk_pair_t v = h[at];
        if (i == j) {  // l1 holds S_i; the f64 sums of a sample with itself are 0 (and NaN for n = 1)
          sums[2 * (size_t)i] = v.l1[0];
          sums[2 * (size_t)i + 1] = v.l1[1];
          v.l1[0] = v.l1[1] = 0;
          v.canb = 0.0;
          v.seuc = 0.0;
        }
        out[(size_t)i * n + j] = v;
        out[(size_t)j * n + i] = v;
      }
    *flags = f[1] ? MK_PAIR_CONSTANT_ROW : 0;
    return MK_OK;
  }
};

}  // namespace

extern "C" int mk_pair_stats_matrix(int device, const uint64_t* matrix, size_t rows, int n, mk_pair_t* out, uint64_t* sums,
                                    uint64_t* flags) {
  Sink sink;
  Sink* c = &sink;
  auto fail = [&](int rc) { mk_set_global_error(sink.err); return rc; };
  if (n < 1 || n > kMaxN || !out || !sums || !flags || (rows && !matrix)) {
    sink.err = "mk_pair_stats_matrix: bad argument (1 <= n <= 4096)";
    return fail(MK_ERR_ARG);
  }
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) {
    (void)hipGetLastError();
    sink.err = "mk_pair_stats_matrix: no such device";
    return fail(MK_ERR_ARG);
  }
  if (hipSetDevice(device) != hipSuccess) { sink.err = "mk_pair_stats_matrix: hipSetDevice failed"; return fail(MK_ERR_HIP); }
  hipStream_t stream = nullptr;
  if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { sink.err = "mk_pair_stats_matrix: hipStreamCreate failed"; return fail(MK_ERR_HIP); }
  int rc;
  {
    PairAcc<Sink> g;
    rc = g.init(c, device, stream, n);
    if (!rc) rc = add_host_rows(c, g, (const u64*)matrix, rows, std::max<size_t>(1, (size_t)(256u << 20) / (8 * (size_t)n)));
    if (!rc) rc = g.finish(out, sums, flags);
  }
  (void)hipStreamDestroy(stream);
  return rc ? fail(rc) : MK_OK;
}

extern "C" int mk_pair_stats(mk_ctx* const* ctxs, int n, size_t slab_rows, mk_pair_t* out, uint64_t* sums, size_t* rows,
                             uint64_t* flags) {
  if (!ctxs || n < 1 || !ctxs[0] || !out || !sums || !rows || !flags) return MK_ERR_ARG;
  PairAcc<mk_ctx> g;
  int rc;
  if ((rc = join_union(ctxs, n, slab_rows, g, rows, "mk_pair_stats")) != MK_OK) return rc;
  return g.finish(out, sums, flags);
}
