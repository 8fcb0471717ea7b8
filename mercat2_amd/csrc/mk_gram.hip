// mk_gram.hip -- exact Gram matrix G = X X^T of n samples' count columns over the union of their k-mers: the
// one pass over the tables that MerCat2's -pca needs (lib/mercat2_figures.py:206-291 fits a PCA on the dense
// combined_<type>_T.tsv; centring and the eigen-decomposition of the n x n G are done on the host, mercat2_amd/pca.py).
//
// Join: mk_join.h (shared with mk_pair_stats, mk_beta.hip): key-range slabs of the union, each scattered into a
// dense rows x n slab of counts that goes through the Gram kernel; by-reference rows are joined on the host.
//
// Gram kernel: a tall, skinny X^T X over the dense slab.  A workgroup stages blocks of R contiguous rows through LDS;
// each thread owns one (i <= j) pair of the upper triangle (pair tiles of 256 over grid.y) and keeps a 128-bit sum.
// Per-workgroup sums go to a workspace, a second kernel adds them into the running 128-bit accumulators (integer
// sums: the result does not depend on the order or the launch shape).  Products are exact for any u64 count: a
// 32 x 32 -> 64 path when no count of the slab reaches 2^32 (one v_mad_u64_u32 and a carry), else the full
// 64 x 64 -> 128 product.
#include "mk_join.h"

namespace {

constexpr int kPairTile = 256;         // threads (pairs) per workgroup
constexpr size_t kLdsBytes = 32768;    // staged rows per block: R = kLdsBytes / (8 n)
constexpr unsigned kGridTarget = 2048; // workgroups per Gram launch (row blocks x pair tiles)

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

}  // namespace

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
  GramAcc<mk_ctx> g;
  int rc;
  if ((rc = join_union(ctxs, n, slab_rows, g, rows_out, "mk_gram")) != MK_OK) return rc;
  return g.finish(gram);
}
