// mk_gram.hip -- exact Gram matrix G = X X^T of n samples' count columns over the union of their k-mers: the
// one pass over the tables that MerCat2's -pca needs (lib/mercat2_figures.py:206-291 fits a PCA on the dense
// combined_<type>_T.tsv; centring and the eigen-decomposition of the n x n G are done on the host, mercat2_amd/pca.py).
//
// Join: every context's packed table is gathered as sorted keys on its own device (mk_export_pairs_device), copied
// to ctxs[0]'s device, and cut into key-range slabs of at most slab_rows entries (so at most slab_rows union rows).
// A slab's entries are gathered, radix sorted by key (rocPRIM), marked at segment heads, numbered by a scan and
// scattered into a dense rows x n slab of counts.  By-reference (text) rows are joined on the host by a sort of the
// strings (they are k-mers outside the alphabet: few) and go through the same Gram kernel as dense rows.
//
// Gram kernel: a tall, skinny X^T X over the dense slab.  A workgroup stages blocks of R contiguous rows through LDS;
// each thread owns one (i <= j) pair of the upper triangle (pair tiles of 256 over grid.y) and keeps a 128-bit sum.
// Per-workgroup sums go to a workspace, a second kernel adds them into the running 128-bit accumulators (integer
// sums: the result does not depend on the order or the launch shape).  Products are exact for any u64 count: a
// 32 x 32 -> 64 path when no count of the slab reaches 2^32 (one v_mad_u64_u32 and a carry), else the full
// 64 x 64 -> 128 product.
#include "mk_common.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

typedef unsigned long long u64;

namespace {

constexpr int kPairTile = 256;         // threads (pairs) per workgroup
constexpr size_t kLdsBytes = 32768;    // staged rows per block: R = kLdsBytes / (8 n)
constexpr int kMaxN = 4096;            // (R >= 1)
constexpr unsigned kGridTarget = 2048; // workgroups per Gram launch (row blocks x pair tiles)

struct Sink {  // where MK_HIP puts its message when there is no context
  std::string err;
};

struct DevBuf {  // device memory of one Gram call, freed on every path out
  void* p = nullptr;
  int device = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) { (void)hipSetDevice(device); (void)hipFree(p); p = nullptr; }
  }
  template <class T> T* as() const { return (T*)p; }
};

template <class C>
int dev_alloc(C* c, DevBuf& b, int device, size_t bytes) {
  b.release();
  b.device = device;
  MK_HIP(hipSetDevice(device));
  hipError_t e = hipMalloc(&b.p, bytes ? bytes : 16);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    c->err = "mk_gram: hipMalloc of " + std::to_string(bytes) + " bytes failed";
    return MK_ERR_NOMEM;
  }
  return MK_OK;
}

// ---------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void mk_gram_wide_k(const u64* __restrict__ x, size_t count, unsigned* __restrict__ flag) {
  u64 acc = 0;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < count; t += (size_t)gridDim.x * blockDim.x)
    acc |= x[t];
  if (__any((acc >> 32) != 0) && (threadIdx.x & (warpSize - 1)) == 0) atomicOr(flag, 1u);
}

// ws[blockIdx.x][p] = sum over this workgroup's rows of x[r][i] * x[r][j], (i, j) = pairs[p], as {lo, hi}
template <bool WIDE>
__global__ __launch_bounds__(kPairTile) void mk_gram_k(const u64* __restrict__ x, size_t rows, int n, int R,
                                                      const unsigned* __restrict__ pairs, int P, u64* __restrict__ ws) {
  extern __shared__ u64 tile[];  // R x n
  const int p = blockIdx.y * kPairTile + threadIdx.x;
  int i = 0, j = 0;
  if (p < P) { const unsigned ij = pairs[p]; i = (int)(ij & 0xffffu); j = (int)(ij >> 16); }
  u64 lo = 0, hi = 0;
  const size_t nblk = (rows + (size_t)R - 1) / (size_t)R;
  for (size_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    const size_t r0 = b * (size_t)R;
    const int rr = (int)min((size_t)R, rows - r0);
    const size_t cnt = (size_t)rr * (size_t)n;
    const u64* src = x + r0 * (size_t)n;  // the block's rows are contiguous: one coalesced sweep
    for (size_t t = threadIdx.x; t < cnt; t += kPairTile) tile[t] = src[t];
    __syncthreads();
    if (p < P) {
      const u64* a = tile + i;
      const u64* c = tile + j;
      for (int r = 0; r < rr; ++r, a += n, c += n) {
        if (WIDE) {
          const u64 pl = a[0] * c[0], ph = __umul64hi(a[0], c[0]);
          lo += pl;
          hi += ph + (lo < pl ? 1 : 0);
        } else {
          const u64 pl = (u64)(unsigned)a[0] * (u64)(unsigned)c[0];
          lo += pl;
          hi += (lo < pl ? 1 : 0);
        }
      }
    }
    __syncthreads();
  }
  if (p < P) {
    u64* w = ws + 2 * ((size_t)blockIdx.x * (size_t)P + (size_t)p);
    w[0] = lo;
    w[1] = hi;
  }
}

// acc[p] += sum over blocks of ws[b][p] (128-bit, with carries)
__global__ __launch_bounds__(256) void mk_gram_reduce_k(const u64* __restrict__ ws, int blocks, int P, u64* __restrict__ acc) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
    u64 lo = acc[2 * (size_t)p], hi = acc[2 * (size_t)p + 1];
    for (int b = 0; b < blocks; ++b) {
      const u64* w = ws + 2 * ((size_t)b * (size_t)P + (size_t)p);
      lo += w[0];
      hi += w[1] + (lo < w[0] ? 1 : 0);
    }
    acc[2 * (size_t)p] = lo;
    acc[2 * (size_t)p + 1] = hi;
  }
}

// the same with one workgroup per pair (many workgroups' partial sums, few pairs): a strided sum per thread, then a tree
__global__ __launch_bounds__(256) void mk_gram_reduce_wg_k(const u64* __restrict__ ws, int blocks, int P, u64* __restrict__ acc) {
  __shared__ u64 slo[256], shi[256];
  const int p = blockIdx.x, t = threadIdx.x;
  u64 lo = 0, hi = 0;
  for (int b = t; b < blocks; b += 256) {
    const u64* w = ws + 2 * ((size_t)b * (size_t)P + (size_t)p);
    lo += w[0];
    hi += w[1] + (lo < w[0] ? 1 : 0);
  }
  slo[t] = lo;
  shi[t] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const u64 a = slo[t + s], l = slo[t] + a;
      shi[t] += shi[t + s] + (l < a ? 1 : 0);
      slo[t] = l;
    }
    __syncthreads();
  }
  if (t == 0) {
    const u64 l = acc[2 * (size_t)p] + slo[0];
    acc[2 * (size_t)p + 1] += shi[0] + (l < slo[0] ? 1 : 0);
    acc[2 * (size_t)p] = l;
  }
}

// out[q * n + s] = number of keys of sample s that are <= q-th query key (binary search in its sorted keys)
__global__ __launch_bounds__(256) void mk_gram_upper_k(const u64* const* __restrict__ keys, const u64* __restrict__ rows,
                                                      int n, int words, const u64* __restrict__ q, int nq, u64* __restrict__ out) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= (size_t)nq * (size_t)n) return;
  const int s = (int)(t % (size_t)n);
  const size_t qi = t / (size_t)n;
  const u64 qh = words == 2 ? q[2 * qi] : 0, ql = words == 2 ? q[2 * qi + 1] : q[qi];
  const u64* k = keys[s];
  size_t lo = 0, hi = rows[s];
  while (lo < hi) {  // first index whose key is > q
    const size_t mid = lo + (hi - lo) / 2;
    bool le;
    if (words == 2) le = k[2 * mid] < qh || (k[2 * mid] == qh && k[2 * mid + 1] <= ql);
    else le = k[mid] <= ql;
    if (le) lo = mid + 1; else hi = mid;
  }
  out[t] = lo;
}

// the slab's entries: sample s contributes its rows [beg[s], beg[s] + pre[s+1] - pre[s]); entry e gets its key
// (one word, or hi / lo apart), its count, its sample, and e itself as the sort value
__global__ __launch_bounds__(256) void mk_gram_gather_k(const u64* const* __restrict__ keys, const u64* const* __restrict__ cnts,
                                                       const u64* __restrict__ beg, const u64* __restrict__ pre, int n, int words,
                                                       size_t E, u64* __restrict__ khi, u64* __restrict__ klo,
                                                       u64* __restrict__ cnt, unsigned* __restrict__ smp, u64* __restrict__ idx) {
  const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e >= E) return;
  int lo = 0, hi = n;  // the last s with pre[s] <= e
  while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (pre[mid] <= e) lo = mid; else hi = mid; }
  const int s = lo;
  const size_t r = beg[s] + (e - pre[s]);
  if (words == 2) { khi[e] = keys[s][2 * r]; klo[e] = keys[s][2 * r + 1]; }
  else klo[e] = keys[s][r];
  cnt[e] = cnts[s][r];
  smp[e] = (unsigned)s;
  idx[e] = e;
}

__global__ __launch_bounds__(256) void mk_gram_take_k(const u64* __restrict__ from, const u64* __restrict__ idx, size_t E,
                                                     u64* __restrict__ to) {
  const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e < E) to[e] = from[idx[e]];
}

// head[e] = 1 where the sorted key differs from the one before
__global__ __launch_bounds__(256) void mk_gram_heads_k(const u64* __restrict__ hi, const u64* __restrict__ lo, int words, size_t E,
                                                      u64* __restrict__ head) {
  const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e >= E) return;
  bool h = e == 0 || lo[e] != lo[e - 1];
  if (words == 2 && e) h = h || hi[e] != hi[e - 1];
  head[e] = h ? 1 : 0;
}

// dense[row(e)][sample] = count; a sample holds a key at most once, so no two entries share a cell
__global__ __launch_bounds__(256) void mk_gram_scatter_k(const u64* __restrict__ rowid, const u64* __restrict__ idx,
                                                        const u64* __restrict__ cnt, const unsigned* __restrict__ smp, int n,
                                                        size_t E, u64* __restrict__ dense, unsigned* __restrict__ wide) {
  const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  u64 v = 0;
  if (e < E) {
    const u64 src = idx[e];
    v = cnt[src];
    dense[(rowid[e] - 1) * (size_t)n + smp[src]] = v;
  }
  if (__any((v >> 32) != 0) && (threadIdx.x & (warpSize - 1)) == 0) atomicOr(wide, 1u);
}

static unsigned grid1(size_t items) { return (unsigned)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, 1u << 30)); }

// ------------------------------------------------------------------------------------- the accumulator
template <class C>
struct GramAcc {
  C* c;
  int device = 0, n = 0, P = 0, R = 1, tiles = 1;
  hipStream_t stream = nullptr;
  DevBuf pairs, acc, ws, flag;
  int ws_blocks = 0;

  int init(C* c_, int device_, hipStream_t stream_, int n_) {
    c = c_; device = device_; stream = stream_; n = n_;
    P = n * (n + 1) / 2;
    tiles = (P + kPairTile - 1) / kPairTile;
    R = (int)std::max<size_t>(1, std::min<size_t>(512, kLdsBytes / (8 * (size_t)n)));
    std::vector<unsigned> h((size_t)P);
    size_t at = 0;
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j) h[at++] = (unsigned)i | ((unsigned)j << 16);
    int rc;
    if ((rc = dev_alloc(c, pairs, device, (size_t)P * 4)) != MK_OK) return rc;
    if ((rc = dev_alloc(c, acc, device, (size_t)P * 16)) != MK_OK) return rc;
    if ((rc = dev_alloc(c, flag, device, 16)) != MK_OK) return rc;
    ws_blocks = (int)std::max<unsigned>(1, kGridTarget / (unsigned)tiles);
    if ((rc = dev_alloc(c, ws, device, (size_t)ws_blocks * (size_t)P * 16)) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(pairs.p, h.data(), (size_t)P * 4, hipMemcpyHostToDevice, stream));
    MK_HIP(hipMemsetAsync(acc.p, 0, (size_t)P * 16, stream));
    return MK_OK;
  }

  // acc += X^T X of the dense rows x n matrix x (device memory on this device); flag_set: the flag already tells
  // whether a count of x reaches 2^32 (set by whoever wrote x), else one pass over x finds out
  int add(const u64* x, size_t rows, bool flag_set = false) {
    if (!rows) return MK_OK;
    MK_HIP(hipSetDevice(device));
    const size_t count = rows * (size_t)n;
    if (!flag_set) {
      MK_HIP(hipMemsetAsync(flag.p, 0, 4, stream));
      mk_gram_wide_k<<<std::min<unsigned>(grid1(count), 2048), 256, 0, stream>>>(x, count, flag.as<unsigned>());
      MK_HIP(hipGetLastError());
    }
    unsigned wide = 0;
    MK_HIP(hipMemcpyAsync(&wide, flag.p, 4, hipMemcpyDeviceToHost, stream));
    MK_HIP(hipStreamSynchronize(stream));
    const size_t nblk = (rows + (size_t)R - 1) / (size_t)R;
    const unsigned gx = (unsigned)std::min<size_t>((size_t)ws_blocks, nblk);
    const dim3 grid(gx, (unsigned)tiles);
    const size_t lds = (size_t)R * (size_t)n * 8;
    if (wide) mk_gram_k<true><<<grid, kPairTile, lds, stream>>>(x, rows, n, R, pairs.as<unsigned>(), P, ws.as<u64>());
    else mk_gram_k<false><<<grid, kPairTile, lds, stream>>>(x, rows, n, R, pairs.as<unsigned>(), P, ws.as<u64>());
    MK_HIP(hipGetLastError());
    if (gx >= 64) mk_gram_reduce_wg_k<<<(unsigned)P, 256, 0, stream>>>(ws.as<u64>(), (int)gx, P, acc.as<u64>());
    else mk_gram_reduce_k<<<std::min<unsigned>(grid1((size_t)P), 1024), 256, 0, stream>>>(ws.as<u64>(), (int)gx, P, acc.as<u64>());
    MK_HIP(hipGetLastError());
    return MK_OK;
  }

  // the full symmetric n x n {lo, hi} matrix
  int finish(uint64_t* gram) {
    std::vector<u64> h((size_t)P * 2);
    MK_HIP(hipSetDevice(device));
    MK_HIP(hipMemcpyAsync(h.data(), acc.p, (size_t)P * 16, hipMemcpyDeviceToHost, stream));
    MK_HIP(hipStreamSynchronize(stream));
    size_t at = 0;
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j, ++at) {
        for (int w = 0; w < 2; ++w) {
          gram[2 * ((size_t)i * n + j) + w] = h[2 * at + w];
          gram[2 * ((size_t)j * n + i) + w] = h[2 * at + w];
        }
      }
    return MK_OK;
  }
};

// host rows x n matrix -> acc, through a device buffer of at most cap_rows rows at a time
template <class C>
int add_host_rows(C* c, GramAcc<C>& g, const u64* m, size_t rows, size_t cap_rows) {
  if (!rows) return MK_OK;
  const size_t step = std::max<size_t>(1, std::min(rows, cap_rows));
  DevBuf d;
  int rc;
  if ((rc = dev_alloc(c, d, g.device, step * (size_t)g.n * 8)) != MK_OK) return rc;
  for (size_t r0 = 0; r0 < rows; r0 += step) {
    const size_t rr = std::min(step, rows - r0);
    MK_HIP(hipMemcpyAsync(d.p, m + r0 * (size_t)g.n, rr * (size_t)g.n * 8, hipMemcpyHostToDevice, g.stream));
    if ((rc = g.add(d.as<u64>(), rr)) != MK_OK) return rc;
    MK_HIP(hipStreamSynchronize(g.stream));  // (d is overwritten by the next step)
  }
  return MK_OK;
}

typedef unsigned __int128 u128;

}  // namespace

void mk_set_global_error(const std::string& msg);  // mk_api.hip: mk_last_error(NULL)

extern "C" int mk_gram_matrix(int device, const uint64_t* matrix, size_t rows, int n, uint64_t* gram) {
  Sink sink;
  Sink* c = &sink;
  auto fail = [&](int rc) { mk_set_global_error(sink.err); return rc; };
  if (n < 1 || n > kMaxN || !gram || (rows && !matrix)) { sink.err = "mk_gram_matrix: bad argument (1 <= n <= 4096)"; return fail(MK_ERR_ARG); }
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) {
    (void)hipGetLastError();
    sink.err = "mk_gram_matrix: no such device";
    return fail(MK_ERR_ARG);
  }
  if (hipSetDevice(device) != hipSuccess) { sink.err = "mk_gram_matrix: hipSetDevice failed"; return fail(MK_ERR_HIP); }
  hipStream_t stream = nullptr;
  if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { sink.err = "mk_gram_matrix: hipStreamCreate failed"; return fail(MK_ERR_HIP); }
  int rc;
  {
    GramAcc<Sink> g;
    rc = g.init(c, device, stream, n);
    if (!rc) rc = add_host_rows(c, g, (const u64*)matrix, rows, std::max<size_t>(1, (size_t)(256u << 20) / (8 * (size_t)n)));
    if (!rc) rc = g.finish(gram);
  }
  (void)hipStreamDestroy(stream);
  return rc ? fail(rc) : MK_OK;
}

extern "C" int mk_gram(mk_ctx* const* ctxs, int n, size_t slab_rows, uint64_t* gram, size_t* rows_out) {
  if (!ctxs || n < 1 || !ctxs[0] || !gram || !rows_out) return MK_ERR_ARG;
  for (int j_ = 0; j_ < n; ++j_) if (ctxs[j_] && ctxs[j_]->spoiled) { ctxs[0]->err = "mk_gram: a context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  mk_ctx* c = ctxs[0];
  if (n > kMaxN) { c->err = "mk_gram: at most 4096 samples"; return MK_ERR_ARG; }
  for (int s = 0; s < n; ++s) {
    const mk_ctx* o = ctxs[s];
    if (!o) { c->err = "mk_gram: a context is NULL"; return MK_ERR_ARG; }
    if (o->k != c->k || o->alphabet != c->alphabet || o->canonical != c->canonical) {
      c->err = "mk_gram: contexts differ in k, alphabet or canonical mode";
      return MK_ERR_ARG;
    }
    if (o->in_chunk) { c->err = "mk_gram: a chunk is open"; return MK_ERR_STATE; }
  }
  int rc;
  const int dev0 = c->device;
  for (int s = 0; s < n; ++s)
    if ((rc = mk_settle(ctxs[s])) != MK_OK) { if (s) c->err = ctxs[s]->err; return rc; }
  MK_HIP(hipSetDevice(dev0));
  GramAcc<mk_ctx> g;
  if ((rc = g.init(c, dev0, c->stream, n)) != MK_OK) return rc;

  // ---- packed rows: sorted keys per sample, on dev0
  int words = 0;
  std::vector<DevBuf> keys((size_t)n), cnts((size_t)n);
  std::vector<u64> rows((size_t)n, 0);
  for (int s = 0; s < n; ++s) {
    mk_ctx* o = ctxs[s];
    if (o->mode == MK_MODE_BYREF) continue;
    const int w = mk_words_per_key(o);
    if (words && w != words) { c->err = "mk_gram: contexts differ in key width"; return MK_ERR_ARG; }
    words = w;
    const size_t cap = o->mode == MK_MODE_DENSE ? o->run_slots : o->run_rows + (o->run_side ? 1 : 0) + o->run128_rows;
    if (!cap) continue;
    DevBuf k_, c_;
    if ((rc = dev_alloc(c, k_, o->device, cap * 8 * (size_t)w)) != MK_OK) return rc;
    if ((rc = dev_alloc(c, c_, o->device, cap * 8)) != MK_OK) return rc;
    size_t got = 0;
    if ((rc = mk_export_pairs_device(o, k_.as<uint64_t>(), c_.as<uint64_t>(), cap, &got)) != MK_OK) {
      if (s) c->err = o->err;
      return rc;
    }
    rows[s] = got;
    if (o->device == dev0) {
      std::swap(keys[s].p, k_.p); keys[s].device = dev0;
      std::swap(cnts[s].p, c_.p); cnts[s].device = dev0;
    } else {  // to ctxs[0]'s device (hipMemcpyPeer stages through the host where there is no direct path)
      if ((rc = dev_alloc(c, keys[s], dev0, got * 8 * (size_t)w)) != MK_OK) return rc;
      if ((rc = dev_alloc(c, cnts[s], dev0, got * 8)) != MK_OK) return rc;
      if (got) {
        MK_HIP(hipMemcpyPeer(keys[s].p, dev0, k_.p, o->device, got * 8 * (size_t)w));
        MK_HIP(hipMemcpyPeer(cnts[s].p, dev0, c_.p, o->device, got * 8));
      }
    }
  }
  MK_HIP(hipSetDevice(dev0));
  size_t total = 0;
  for (int s = 0; s < n; ++s) total += rows[s];
  size_t union_rows = 0;

  if (total) {
    // slab cap (entries, hence union rows): from free memory unless given
    size_t cap = slab_rows;
    if (!cap) {
      size_t fr = 0, tot = 0;
      MK_HIP(hipMemGetInfo(&fr, &tot));
      cap = std::max<size_t>(1, (fr / 2) / (112 + 8 * (size_t)n));
      cap = std::min<size_t>(cap, (size_t)1 << 28);
    }
    // key range [first, last] of the union, as 128-bit numbers
    auto key_at = [&](int s, size_t r, u128* out) -> int {
      u64 h[2] = {0, 0};
      MK_HIP(hipMemcpy(h, keys[s].as<u64>() + r * (size_t)words, 8 * (size_t)words, hipMemcpyDeviceToHost));
      *out = words == 2 ? (((u128)h[0] << 64) | h[1]) : (u128)h[0];
      return MK_OK;
    };
    u128 kmin = ~(u128)0, kmax = 0;
    for (int s = 0; s < n; ++s) {
      if (!rows[s]) continue;
      u128 a, b;
      if ((rc = key_at(s, 0, &a)) != MK_OK || (rc = key_at(s, rows[s] - 1, &b)) != MK_OK) return rc;
      kmin = std::min(kmin, a);
      kmax = std::max(kmax, b);
    }
    // device tables of the samples' arrays
    std::vector<const u64*> hk((size_t)n), hc((size_t)n);
    for (int s = 0; s < n; ++s) { hk[s] = keys[s].as<u64>(); hc[s] = cnts[s].as<u64>(); }
    DevBuf d_keys, d_cnts, d_rows;
    if ((rc = dev_alloc(c, d_keys, dev0, 8 * (size_t)n)) || (rc = dev_alloc(c, d_cnts, dev0, 8 * (size_t)n)) ||
        (rc = dev_alloc(c, d_rows, dev0, 8 * (size_t)n)))
      return rc;
    MK_HIP(hipMemcpy(d_keys.p, hk.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
    MK_HIP(hipMemcpy(d_cnts.p, hc.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
    MK_HIP(hipMemcpy(d_rows.p, rows.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
    // per-sample entry counts <= each query key
    auto upper = [&](const std::vector<u128>& q, std::vector<u64>& out) -> int {
      const size_t nq = q.size();
      std::vector<u64> hq(nq * (size_t)words);
      for (size_t i = 0; i < nq; ++i) {
        if (words == 2) { hq[2 * i] = (u64)(q[i] >> 64); hq[2 * i + 1] = (u64)q[i]; }
        else hq[i] = (u64)q[i];
      }
      DevBuf dq, dout;
      int r_;
      if ((r_ = dev_alloc(c, dq, dev0, hq.size() * 8)) || (r_ = dev_alloc(c, dout, dev0, nq * (size_t)n * 8))) return r_;
      MK_HIP(hipMemcpyAsync(dq.p, hq.data(), hq.size() * 8, hipMemcpyHostToDevice, c->stream));
      mk_gram_upper_k<<<grid1(nq * (size_t)n), 256, 0, c->stream>>>(d_keys.as<const u64*>(), d_rows.as<u64>(), n, words,
                                                                    dq.as<u64>(), (int)nq, dout.as<u64>());
      MK_HIP(hipGetLastError());
      out.resize(nq * (size_t)n);
      MK_HIP(hipMemcpyAsync(out.data(), dout.p, out.size() * 8, hipMemcpyDeviceToHost, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      return MK_OK;
    };
    // ranges (ends[t-1], ends[t]] (the first from kmin), bisected until each holds <= cap entries or one key;
    // the first cut is an even split of [kmin, kmax] into about 2 * total / cap parts (mk_owner_bounds' style)
    std::vector<u128> ends;
    std::vector<u64> ub;  // ends.size() x n
    {
      const u128 span = kmax - kmin;
      const size_t parts = std::min<size_t>(4096, std::max<size_t>(1, 2 * total / cap));
      for (size_t i = 1; i < parts; ++i) {
        const u128 e = kmin + span / parts * i;
        if (ends.empty() || e > ends.back()) ends.push_back(e);
      }
      if (ends.empty() || ends.back() < kmax) ends.push_back(kmax);
      if ((rc = upper(ends, ub)) != MK_OK) return rc;
    }
    auto entries = [&](size_t t, const std::vector<u64>& u) {
      size_t e = 0;
      for (int s = 0; s < n; ++s) e += u[t * n + s] - (t ? u[(t - 1) * n + s] : 0);
      return e;
    };
    for (;;) {
      std::vector<u128> mids;
      std::vector<size_t> at;
      for (size_t t = 0; t < ends.size(); ++t) {
        const u128 lo = t ? ends[t - 1] + 1 : kmin;
        if (entries(t, ub) > cap && ends[t] > lo) { mids.push_back(lo + (ends[t] - lo) / 2); at.push_back(t); }
      }
      if (mids.empty()) break;
      std::vector<u64> um;
      if ((rc = upper(mids, um)) != MK_OK) return rc;
      std::vector<u128> e2;
      std::vector<u64> u2;
      size_t m = 0;
      for (size_t t = 0; t < ends.size(); ++t) {
        if (m < at.size() && at[m] == t) {
          e2.push_back(mids[m]);
          u2.insert(u2.end(), um.begin() + m * n, um.begin() + (m + 1) * n);
          ++m;
        }
        e2.push_back(ends[t]);
        u2.insert(u2.end(), ub.begin() + t * n, ub.begin() + (t + 1) * n);
      }
      ends.swap(e2);
      ub.swap(u2);
    }
    // slabs: consecutive ranges while they fit
    std::vector<size_t> slab_end;  // index into ends of each slab's last range
    size_t biggest = 0;
    {
      size_t acc = 0;
      for (size_t t = 0; t < ends.size(); ++t) {
        const size_t e = entries(t, ub);
        if (acc && acc + e > cap) { slab_end.push_back(t - 1); biggest = std::max(biggest, acc); acc = 0; }
        acc += e;
      }
      slab_end.push_back(ends.size() - 1);
      biggest = std::max(biggest, acc);
    }
    // slab buffers, sized for the largest slab
    const size_t E_max = std::max<size_t>(1, biggest);
    DevBuf khi, klo, khi2, klo2, cnt, smp, idx, idx2, head, rowid, dense, tmp, d_beg, d_pre;
    if ((rc = dev_alloc(c, klo, dev0, E_max * 8)) || (rc = dev_alloc(c, klo2, dev0, E_max * 8)) ||
        (rc = dev_alloc(c, cnt, dev0, E_max * 8)) || (rc = dev_alloc(c, smp, dev0, E_max * 4)) ||
        (rc = dev_alloc(c, idx, dev0, E_max * 8)) || (rc = dev_alloc(c, idx2, dev0, E_max * 8)) ||
        (rc = dev_alloc(c, head, dev0, E_max * 8)) || (rc = dev_alloc(c, rowid, dev0, E_max * 8)) ||
        (rc = dev_alloc(c, dense, dev0, std::min(E_max, cap) * 8 * (size_t)n + 8)) ||
        (rc = dev_alloc(c, d_beg, dev0, 8 * (size_t)n)) || (rc = dev_alloc(c, d_pre, dev0, 8 * ((size_t)n + 1))))
      return rc;
    if (words == 2 && ((rc = dev_alloc(c, khi, dev0, E_max * 8)) || (rc = dev_alloc(c, khi2, dev0, E_max * 8)))) return rc;
    size_t tmp_sort = 0, tmp_scan = 0;
    MK_HIP(rocprim::radix_sort_pairs((void*)nullptr, tmp_sort, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                     (const unsigned long long*)nullptr, (unsigned long long*)nullptr, E_max, 0u, 64u, c->stream));
    MK_HIP(rocprim::inclusive_scan((void*)nullptr, tmp_scan, (const u64*)nullptr, (u64*)nullptr, E_max, rocprim::plus<u64>(), c->stream));
    const size_t tmp_bytes = std::max(tmp_sort, tmp_scan);
    if ((rc = dev_alloc(c, tmp, dev0, tmp_bytes)) != MK_OK) return rc;

    size_t first = 0;
    std::vector<u64> beg((size_t)n), pre((size_t)n + 1);
    for (size_t sl = 0; sl < slab_end.size(); ++sl) {
      const size_t last = slab_end[sl];
      pre[0] = 0;
      for (int s = 0; s < n; ++s) {
        beg[s] = first ? ub[(first - 1) * n + s] : 0;
        pre[s + 1] = pre[s] + (ub[last * n + s] - beg[s]);
      }
      const size_t E = pre[n];
      const u128 hi_key = ends[last];
      first = last + 1;
      if (!E) continue;
      MK_HIP(hipMemcpyAsync(d_beg.p, beg.data(), 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
      MK_HIP(hipMemcpyAsync(d_pre.p, pre.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
      mk_gram_gather_k<<<grid1(E), 256, 0, c->stream>>>(d_keys.as<const u64*>(), d_cnts.as<const u64*>(), d_beg.as<u64>(),
                                                         d_pre.as<u64>(), n, words, E, khi.as<u64>(), klo.as<u64>(),
                                                         cnt.as<u64>(), smp.as<unsigned>(), idx.as<u64>());
      MK_HIP(hipGetLastError());
      // sort by key (LSD radix sorts are stable: two-word keys by lo, then by hi), values = entry numbers
      const u64* s_hi = nullptr;
      const u64* s_lo = nullptr;
      const u64* s_idx = nullptr;
      if (words == 1) {
        unsigned bits = 1;
        while (bits < 64 && (hi_key >> bits) != 0) ++bits;
        MK_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_sort, (const unsigned long long*)klo.p, (unsigned long long*)klo2.p,
                                         (const unsigned long long*)idx.p, (unsigned long long*)idx2.p, E, 0u, bits, c->stream));
        s_lo = klo2.as<u64>();
        s_idx = idx2.as<u64>();
      } else {
        MK_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_sort, (const unsigned long long*)klo.p, (unsigned long long*)klo2.p,
                                         (const unsigned long long*)idx.p, (unsigned long long*)idx2.p, E, 0u, 64u, c->stream));
        mk_gram_take_k<<<grid1(E), 256, 0, c->stream>>>(khi.as<u64>(), idx2.as<u64>(), E, khi2.as<u64>());
        MK_HIP(hipGetLastError());
        MK_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_sort, (const unsigned long long*)khi2.p, (unsigned long long*)khi.p,
                                         (const unsigned long long*)idx2.p, (unsigned long long*)idx.p, E, 0u, 64u, c->stream));
        // (khi: sorted hi words; lo words in the final order, for the head test)
        mk_gram_take_k<<<grid1(E), 256, 0, c->stream>>>(klo.as<u64>(), idx.as<u64>(), E, klo2.as<u64>());
        MK_HIP(hipGetLastError());
        s_hi = khi.as<u64>();
        s_lo = klo2.as<u64>();
        s_idx = idx.as<u64>();
      }
      mk_gram_heads_k<<<grid1(E), 256, 0, c->stream>>>(s_hi, s_lo, words, E, head.as<u64>());
      MK_HIP(hipGetLastError());
      MK_HIP(rocprim::inclusive_scan(tmp.p, tmp_scan, head.as<u64>(), rowid.as<u64>(), E, rocprim::plus<u64>(), c->stream));
      u64 U = 0;
      MK_HIP(hipMemcpyAsync(&U, rowid.as<u64>() + (E - 1), 8, hipMemcpyDeviceToHost, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      if (U > std::min(E_max, cap) && U > 1) { c->err = "mk_gram: a slab holds more union rows than its buffer"; return MK_ERR_STATE; }
      MK_HIP(hipMemsetAsync(dense.p, 0, U * 8 * (size_t)n, c->stream));
      MK_HIP(hipMemsetAsync(g.flag.p, 0, 4, c->stream));
      mk_gram_scatter_k<<<grid1(E), 256, 0, c->stream>>>(rowid.as<u64>(), s_idx, cnt.as<u64>(), smp.as<unsigned>(), n, E,
                                                          dense.as<u64>(), g.flag.as<unsigned>());
      MK_HIP(hipGetLastError());
      if ((rc = g.add(dense.as<u64>(), U, /*flag_set=*/true)) != MK_OK) return rc;
      union_rows += U;
    }
  }

  // ---- by-reference rows: joined on the host (sorted strings of every sample, merged), then the same kernel
  {
    const size_t k = (size_t)c->k;
    std::vector<std::vector<uint8_t>> str((size_t)n);
    std::vector<std::vector<u64>> cn((size_t)n);
    size_t any = 0;
    for (int s = 0; s < n; ++s) {
      size_t r = 0;
      if ((rc = mk_export_exotic(ctxs[s], nullptr, nullptr, 0, &r)) != MK_OK) { if (s) c->err = ctxs[s]->err; return rc; }
      if (!r) continue;
      str[s].resize(r * k);
      cn[s].resize(r);
      if ((rc = mk_export_exotic(ctxs[s], str[s].data(), (uint64_t*)cn[s].data(), r, &r)) != MK_OK) { if (s) c->err = ctxs[s]->err; return rc; }
      any += r;
    }
    if (any) {
      std::vector<size_t> pos((size_t)n, 0);
      std::vector<u64> m;
      size_t mrows = 0;
      for (;;) {  // k-way merge of the sorted rows
        const uint8_t* best = nullptr;
        for (int s = 0; s < n; ++s)
          if (pos[s] < cn[s].size() && (!best || memcmp(str[s].data() + pos[s] * k, best, k) < 0)) best = str[s].data() + pos[s] * k;
        if (!best) break;
        std::vector<uint8_t> key(best, best + k);
        m.resize((mrows + 1) * (size_t)n, 0);
        for (int s = 0; s < n; ++s)
          if (pos[s] < cn[s].size() && memcmp(str[s].data() + pos[s] * k, key.data(), k) == 0) {
            m[mrows * (size_t)n + s] = cn[s][pos[s]];
            ++pos[s];
          }
        ++mrows;
      }
      MK_HIP(hipSetDevice(dev0));
      const size_t step = slab_rows ? slab_rows : std::max<size_t>(1, (size_t)(256u << 20) / (8 * (size_t)n));
      if ((rc = add_host_rows(c, g, m.data(), mrows, step)) != MK_OK) return rc;
      union_rows += mrows;
    }
  }
  if ((rc = g.finish(gram)) != MK_OK) return rc;
  *rows_out = union_rows;
  return MK_OK;
}
