// mk_join.h -- the union join of n samples' tables that mk_gram (mk_gram.hip) and mk_pair_stats (mk_beta.hip) share.
//
// Every context's packed table is gathered as sorted keys on its own device (mk_export_pairs_device), copied to
// ctxs[0]'s device, and cut into key-range slabs of at most slab_rows entries (so at most slab_rows union rows).
// A slab's entries are gathered, radix sorted by key (rocPRIM), marked at segment heads, numbered by a scan and
// scattered into a dense rows x n slab of counts, which goes to the accumulator's add().  By-reference (text) rows
// are joined on the host by a sort of the strings (they are k-mers outside the alphabet: few) and go to add() too.
//
// An accumulator Acc has: int init(C* c, int device, hipStream_t stream, int n); int add(const u64* x, size_t rows,
// bool flag_set); members device, stream, n and a DevBuf flag whose first u32 the scatter sets when a count of the
// slab reaches 2^32 (add(..., flag_set = true) may rely on it).
#pragma once
#include "mk_common.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

typedef unsigned long long u64;

namespace {

constexpr int kMaxN = 4096;  // samples per join (mk_gram, mk_pair_stats)

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
    c->err = "mk_join: hipMalloc of " + std::to_string(bytes) + " bytes failed";
    return MK_ERR_NOMEM;
  }
  return MK_OK;
}

// ------------------------------------------------------------------------------------- join kernels
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

// host rows x n matrix -> acc, through a device buffer of at most cap_rows rows at a time
template <class C, class Acc>
int add_host_rows(C* c, Acc& g, const u64* m, size_t rows, size_t cap_rows) {
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

// validate and settle the contexts, g.init on ctxs[0]'s device, join; *rows_out = union rows.  who: the entry
// point's name, for messages
template <class Acc>
int join_union(mk_ctx* const* ctxs, int n, size_t slab_rows, Acc& g, size_t* rows_out, const char* who) {
  const std::string W(who);
  if (!ctxs || n < 1 || !ctxs[0] || !rows_out) return MK_ERR_ARG;
  for (int j_ = 0; j_ < n; ++j_) if (ctxs[j_] && ctxs[j_]->spoiled) { ctxs[0]->err = W + ": a context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  mk_ctx* c = ctxs[0];
  if (n > kMaxN) { c->err = W + ": at most 4096 samples"; return MK_ERR_ARG; }
  for (int s = 0; s < n; ++s) {
    const mk_ctx* o = ctxs[s];
    if (!o) { c->err = W + ": a context is NULL"; return MK_ERR_ARG; }
    if (o->k != c->k || o->alphabet != c->alphabet || o->canonical != c->canonical) {
      c->err = W + ": contexts differ in k, alphabet or canonical mode";
      return MK_ERR_ARG;
    }
    if (o->in_chunk) { c->err = W + ": a chunk is open"; return MK_ERR_STATE; }
  }
  int rc;
  const int dev0 = c->device;
  for (int s = 0; s < n; ++s)
    if ((rc = mk_settle(ctxs[s])) != MK_OK) { if (s) c->err = ctxs[s]->err; return rc; }
  MK_HIP(hipSetDevice(dev0));
  if ((rc = g.init(c, dev0, c->stream, n)) != MK_OK) return rc;

  // ---- packed rows: sorted keys per sample, on dev0
  int words = 0;
  std::vector<DevBuf> keys((size_t)n), cnts((size_t)n);
  std::vector<u64> rows((size_t)n, 0);
  for (int s = 0; s < n; ++s) {
    mk_ctx* o = ctxs[s];
    if (o->mode == MK_MODE_BYREF) continue;
    const int w = mk_words_per_key(o);
    if (words && w != words) { c->err = W + ": contexts differ in key width"; return MK_ERR_ARG; }
    words = w;
    const size_t cap = o->mode == MK_MODE_DENSE ? o->run_slots : mk_packed_rows(o);
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
      if (U > std::min(E_max, cap) && U > 1) { c->err = W + ": a slab holds more union rows than its buffer"; return MK_ERR_STATE; }
      MK_HIP(hipMemsetAsync(dense.p, 0, U * 8 * (size_t)n, c->stream));
      MK_HIP(hipMemsetAsync(g.flag.p, 0, 4, c->stream));
      mk_gram_scatter_k<<<grid1(E), 256, 0, c->stream>>>(rowid.as<u64>(), s_idx, cnt.as<u64>(), smp.as<unsigned>(), n, E,
                                                          dense.as<u64>(), (unsigned*)g.flag.p);
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
  *rows_out = union_rows;
  return MK_OK;
}

}  // namespace
