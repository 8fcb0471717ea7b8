// mk_binsort.hip -- a one-word running table as sorted (key, count) rows in four launches: the export's own sort.
//
// Packed keys are right-aligned and compare as unsigned integers (mk_sort.hip), so the top B of a key's key_bits bits
// name a bin, and the bins in order, each sorted, are the table in order.  The table is read twice and the rows
// cross HBM twice (the library's radix sort moves them nine times, profiles/export_sort.md):
//
//   bs_count_k   every workgroup reads a slice of BS_SLICE slots, counts its rows per bin in LDS, adds the bins it met
//   bs_scan_k    bin starts = exclusive scan of the 2^B counts; the total; bins of more than BS_SMALL rows listed,
//                bins of more than BS_CAP rows counted
//   bs_place_k   the same slices again (still in L2 / Infinity Cache): a row's rank within (workgroup, bin) from an LDS
//                counter, one global add per (workgroup, bin) reserves the range, {key, count} stored as one pair
//   bs_sort_*_k  one workgroup per bin: a counting sort on the next 10 bits puts the pairs into LDS, each finds its place
//                among the one or two rows that share those bits (keys are distinct: no stability needed); keys and
//                counts go to the two output columns at the bin's start
//
// Nothing waits for another workgroup.  A bin over BS_CAP rows is left alone and counted: the caller reads that
// number with the row total and takes the export again through the library sort (mk_export.hip).
#include "mk_common.h"
#include "mk_device.h"

// Rows of the mean bin at most (B grows until rows >> B is no larger): (362, 724] keeps a bin and its spread within
// one power of two, which is what the network pads to (profiles/export_sort.md has the other sizes tried).
#ifndef BS_MEAN_MAX
#define BS_MEAN_MAX 724
#endif
constexpr int BS_MAX_BITS = 14;       // 2^14 LDS counters = 64 KB
constexpr unsigned BS_CAP = 8192;     // rows one workgroup sorts in LDS: 128 KB of the 160
constexpr unsigned BS_SMALL = 2048;   // rows of the common class: 32 KB, several workgroups a CU
constexpr int BS_T = 1024;            // threads of the count / scan / place workgroups
constexpr int BS_PER = 16;            // slots a thread holds in registers
constexpr size_t BS_SLICE = (size_t)BS_T * BS_PER;
static_assert(BS_SLICE <= 65536, "bs_place_k packs a row's rank within its slice into 16 bits");
constexpr unsigned BS_BIG_GRID = 256;
constexpr int BS_EPT = 8;             // pairs a thread of a bin sort holds in registers
constexpr int BS_SMALL_T = BS_SMALL / BS_EPT;
static_assert(BS_SMALL_T * BS_EPT == BS_SMALL && BS_T * BS_EPT == BS_CAP, "a bin fits the registers of its workgroup");
constexpr int BS_SMALL_SBITS = 10, BS_BIG_SBITS = 12;  // key bits below the bin's that name a run (small: 36.9 KB of LDS, four workgroups a CU)
constexpr unsigned BS_RUN_MAX = 16;   // rows of a run the counting sort takes

bool mk_binsort_takes(size_t rows) { return rows <= ((size_t)(BS_CAP / 4) << BS_MAX_BITS); }

static int bs_bits(size_t rows, int key_bits) {
  int b = 0;
  while (b < BS_MAX_BITS && b < key_bits && (rows >> b) > BS_MEAN_MAX) ++b;
  return b;
}

__device__ __forceinline__ bool bs_occupied(const ulonglong2& s) { return s.x != MK_EMPTY && s.y != 0; }  // mk_compact_k's rule

// this workgroup's slice in registers, slot j * BS_T + thread of it in s[j] (free beyond the table's end)
__device__ __forceinline__ void bs_load_slice(const MkSlot* __restrict__ t, size_t slots, ulonglong2 (&s)[BS_PER]) {
  const size_t base = (size_t)blockIdx.x * BS_SLICE + threadIdx.x;
#pragma unroll
  for (int j = 0; j < BS_PER; ++j) {
    const size_t i = base + (size_t)j * BS_T;
    s[j] = i < slots ? reinterpret_cast<const ulonglong2*>(t)[i] : make_ulonglong2(MK_EMPTY, 0);
  }
}

// Exclusive prefix sum over a workgroup of THREADS in thread order (mk_block_scan_excl for any size).  s_wave: THREADS / 64
// words.  One barrier inside: every thread must call it.
template <int THREADS>
__device__ __forceinline__ unsigned bs_block_scan_excl(unsigned own, unsigned* s_wave) {
  const unsigned incl = mk_wave_scan_incl(own);
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned pre = incl - own;
  for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) pre += s_wave[w];
  return pre;
}

// shift = key_bits - B and mask = 2^B - 1 (B = 0: shift 0, mask 0)
__global__ __launch_bounds__(BS_T) void bs_count_k(const MkSlot* __restrict__ t, size_t slots, int shift, unsigned mask,
                                                   unsigned* __restrict__ counts) {
  extern __shared__ unsigned s_hist[];  // 2^B
  for (unsigned b = threadIdx.x; b <= mask; b += BS_T) s_hist[b] = 0;
  __syncthreads();
  ulonglong2 s[BS_PER];
  bs_load_slice(t, slots, s);
#pragma unroll
  for (int j = 0; j < BS_PER; ++j)
    if (bs_occupied(s[j])) atomicAdd(&s_hist[(unsigned)(s[j].x >> shift) & mask], 1u);
  __syncthreads();
  for (unsigned b = threadIdx.x; b <= mask; b += BS_T) {
    const unsigned n = s_hist[b];
    if (n) atomicAdd(&counts[b], n);
  }
}

// scal: [0] rows of the table, [1] bins over BS_CAP rows, [2] entries of big[]
__global__ __launch_bounds__(BS_T) void bs_scan_k(u64* __restrict__ scal, const unsigned* __restrict__ counts,
                                                  unsigned* __restrict__ start, unsigned* __restrict__ cursor,
                                                  unsigned* __restrict__ big, unsigned nb) {
  __shared__ unsigned s_wave[BS_T / 64];
  __shared__ unsigned s_nbig, s_nover;
  const unsigned per = (nb + BS_T - 1) / BS_T, b0 = threadIdx.x * per;
  if (threadIdx.x == 0) s_nbig = s_nover = 0;
  unsigned sum = 0;
  for (unsigned j = 0; j < per; ++j)
    if (b0 + j < nb) sum += counts[b0 + j];
  unsigned pre = bs_block_scan_excl<BS_T>(sum, s_wave);
  for (unsigned j = 0; j < per; ++j) {
    const unsigned b = b0 + j;
    if (b >= nb) break;
    const unsigned n = counts[b];
    start[b] = pre;
    cursor[b] = pre;
    pre += n;
    if (n > BS_CAP) atomicAdd(&s_nover, 1u);
    else if (n > BS_SMALL) big[atomicAdd(&s_nbig, 1u)] = b;
  }
  __syncthreads();
  if (threadIdx.x == BS_T - 1) scal[0] = pre;  // (threads past the last bin hold the total as well)
  if (threadIdx.x == 0) { scal[1] = s_nover; scal[2] = s_nbig; }
}

// cap: pairs `out` has room for (the rows the host knows of; a table that holds more is reported, not written past)
__global__ __launch_bounds__(BS_T) void bs_place_k(const MkSlot* __restrict__ t, size_t slots, int shift, unsigned mask,
                                                   unsigned* __restrict__ cursor, ulonglong2* __restrict__ out, size_t cap) {
  extern __shared__ unsigned s_hist[];  // 2^B: rows of this slice per bin, then where the slice's rows of the bin go
  for (unsigned b = threadIdx.x; b <= mask; b += BS_T) s_hist[b] = 0;
  __syncthreads();
  ulonglong2 s[BS_PER];
  unsigned rank[BS_PER / 2];  // of slot j within its (slice, bin): below BS_SLICE <= 2^16, two to a register
  bs_load_slice(t, slots, s);
#pragma unroll
  for (int j = 0; j < BS_PER; ++j) {
    const unsigned r = bs_occupied(s[j]) ? atomicAdd(&s_hist[(unsigned)(s[j].x >> shift) & mask], 1u) : 0u;
    rank[j >> 1] = (j & 1) ? rank[j >> 1] | (r << 16) : r;
  }
  __syncthreads();
  // one range per (workgroup, bin), four reservations of a thread in flight together
  for (unsigned b0 = threadIdx.x; b0 <= mask; b0 += 4 * BS_T) {
    unsigned n[4], at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) n[u] = b0 + u * BS_T <= mask ? s_hist[b0 + u * BS_T] : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) at[u] = n[u] ? atomicAdd(&cursor[b0 + u * BS_T], n[u]) : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (n[u]) s_hist[b0 + u * BS_T] = at[u];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < BS_PER; ++j)
    if (bs_occupied(s[j])) {
      const size_t pos = (size_t)s_hist[(unsigned)(s[j].x >> shift) & mask] + ((rank[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
      if (pos < cap) out[pos] = s[j];
    }
}

// LDS of one bin sort: the bin's pairs, 2^SBITS run counters, the scan's words, "a run is too long"
template <int THREADS, int SBITS>
struct BsBinLds {
  ulonglong2 s[THREADS * BS_EPT];
  unsigned hist[1u << SBITS];
  unsigned wave[THREADS / 64];
  unsigned crowded;
};

// The n <= THREADS * BS_EPT pairs in[start ..] sorted by key into keys / cnts[start ..]; rem: the key bits below the
// bin's.  The next SBITS bits of a key name its run.  A counting sort puts the pairs into LDS run after run (in no
// order within a run); then every pair finds its place within its run by counting the smaller keys of the run -- a
// run of evenly spread keys holds a row or two.  A bin with a run of more than BS_RUN_MAX rows takes a bitonic network
// instead (padded to a power of two with MK_EMPTY, the key no table holds).  Every thread of the workgroup calls it.
template <int THREADS, int SBITS>
__device__ __forceinline__ void bs_sort_bin(const ulonglong2* __restrict__ in, unsigned n, size_t start, int rem,
                                            u64* __restrict__ keys, u64* __restrict__ cnts, size_t cap,
                                            BsBinLds<THREADS, SBITS>& l) {
  constexpr unsigned NS = 1u << SBITS, HPT = NS / THREADS;
  static_assert(HPT * THREADS == NS, "every thread scans HPT counters");
  const int sb = rem < SBITS ? rem : SBITS, sshift = rem - sb;
  const unsigned smask = (1u << sb) - 1;
  for (unsigned h = threadIdx.x; h < NS; h += THREADS) l.hist[h] = 0;
  if (threadIdx.x == 0) l.crowded = 0;
  ulonglong2 e[BS_EPT];
#pragma unroll
  for (int j = 0; j < BS_EPT; ++j) {
    const unsigned i = j * THREADS + threadIdx.x;
    e[j] = i < n && start + i < cap ? in[start + i] : make_ulonglong2(MK_EMPTY, 0);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < BS_EPT; ++j)
    if (j * THREADS + threadIdx.x < n) atomicAdd(&l.hist[(unsigned)(e[j].x >> sshift) & smask], 1u);
  __syncthreads();
  unsigned c[HPT], sum = 0, most = 0;
#pragma unroll
  for (unsigned u = 0; u < HPT; ++u) {
    c[u] = l.hist[threadIdx.x * HPT + u];
    sum += c[u];
    most = c[u] > most ? c[u] : most;
  }
  if (most > BS_RUN_MAX) l.crowded = 1;
  unsigned pre = bs_block_scan_excl<THREADS>(sum, l.wave);
#pragma unroll
  for (unsigned u = 0; u < HPT; ++u) {
    l.hist[threadIdx.x * HPT + u] = pre;
    pre += c[u];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < BS_EPT; ++j)
    if (j * THREADS + threadIdx.x < n) l.s[atomicAdd(&l.hist[(unsigned)(e[j].x >> sshift) & smask], 1u)] = e[j];
  __syncthreads();  // hist[r] is now where run r ends, and run r + 1 begins
  if (!l.crowded) {
    for (unsigned p = threadIdx.x; p < n; p += THREADS) {
      const ulonglong2 a = l.s[p];
      const unsigned r = (unsigned)(a.x >> sshift) & smask, end = l.hist[r];
      unsigned at = r ? l.hist[r - 1] : 0u;
      for (unsigned q = at; q < end; ++q) at += l.s[q].x < a.x ? 1u : 0u;
      if (start + at < cap) { keys[start + at] = a.x; cnts[start + at] = a.y; }
    }
    return;
  }
  unsigned m = 64;
  while (m < n) m <<= 1;
  for (unsigned i = n + threadIdx.x; i < m; i += THREADS) l.s[i] = make_ulonglong2(MK_EMPTY, 0);
  __syncthreads();
  for (unsigned k = 2; k <= m; k <<= 1)
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      for (unsigned x = threadIdx.x; x < m / 2; x += THREADS) {
        const unsigned i = ((x & ~(j - 1)) << 1) | (x & (j - 1)), h = i | j;  // the pair (i, i + j) of this step
        const ulonglong2 a = l.s[i], b = l.s[h];
        if ((a.x > b.x) == ((i & k) == 0)) { l.s[i] = b; l.s[h] = a; }
      }
      __syncthreads();
    }
  for (unsigned i = threadIdx.x; i < n; i += THREADS)
    if (start + i < cap) { keys[start + i] = l.s[i].x; cnts[start + i] = l.s[i].y; }
}

__global__ __launch_bounds__(BS_SMALL_T) void bs_sort_small_k(const ulonglong2* __restrict__ in, const unsigned* __restrict__ counts,
                                                              const unsigned* __restrict__ start, int rem, u64* __restrict__ keys,
                                                              u64* __restrict__ cnts, size_t cap) {
  __shared__ __attribute__((aligned(16))) BsBinLds<BS_SMALL_T, BS_SMALL_SBITS> l;
  const unsigned n = counts[blockIdx.x];
  if (n == 0 || n > BS_SMALL) return;
  bs_sort_bin<BS_SMALL_T, BS_SMALL_SBITS>(in, n, start[blockIdx.x], rem, keys, cnts, cap, l);
}

// the listed bins (BS_SMALL < rows <= BS_CAP): none in a table whose keys spread evenly
__global__ __launch_bounds__(BS_T) void bs_sort_big_k(const ulonglong2* __restrict__ in, const unsigned* __restrict__ counts,
                                                      const unsigned* __restrict__ start, const unsigned* __restrict__ big,
                                                      const u64* __restrict__ scal, int rem, u64* __restrict__ keys,
                                                      u64* __restrict__ cnts, size_t cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_big[];
  BsBinLds<BS_T, BS_BIG_SBITS>& l = *reinterpret_cast<BsBinLds<BS_T, BS_BIG_SBITS>*>(s_big);
  const unsigned nbig = (unsigned)scal[2];
  for (unsigned e = blockIdx.x; e < nbig; e += gridDim.x) {
    const unsigned b = big[e];
    bs_sort_bin<BS_T, BS_BIG_SBITS>(in, counts[b], start[b], rem, keys, cnts, cap, l);
    __syncthreads();
  }
}

// The rows of table t (the host counts `rows` of them), sorted, into keys_out / cnts_out.  *d_scal: two words on the
// device for the caller's read-back, [0] the rows found, [1] the bins left unsorted (then the columns hold no result).
int mk_binsort_export(mk_ctx* c, const MkSlot* t, size_t slots, size_t rows, int key_bits, uint64_t* keys_out,
                      uint64_t* cnts_out, const uint64_t** d_scal) {
  const int bits = bs_bits(rows, key_bits);
  const unsigned nb = 1u << bits, mask = nb - 1;
  const int shift = bits ? key_bits - bits : 0;
  int rc;
  // scal[4] | counts | start | cursor | big, and the rows as pairs
  if ((rc = mk_buf_reserve(c, c->ex_tmp, 32 + 4 * (size_t)nb * 4)) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, c->ex_keys, rows * 16 + 64)) != MK_OK) return rc;
  u64* scal = (u64*)c->ex_tmp.p;
  unsigned* counts = (unsigned*)(scal + 4);
  unsigned *start = counts + nb, *cursor = start + nb, *big = cursor + nb;
  ulonglong2* pairs = (ulonglong2*)c->ex_keys.p;
  MK_HIP(hipMemsetAsync(scal, 0, 32 + (size_t)nb * 4, c->stream));
  const unsigned grid = (unsigned)div_up(slots, BS_SLICE);
  hipLaunchKernelGGL(bs_count_k, dim3(grid), dim3(BS_T), nb * 4, c->stream, t, slots, shift, mask, counts);
  hipLaunchKernelGGL(bs_scan_k, dim3(1), dim3(BS_T), 0, c->stream, scal, (const unsigned*)counts, start, cursor, big, nb);
  hipLaunchKernelGGL(bs_place_k, dim3(grid), dim3(BS_T), nb * 4, c->stream, t, slots, shift, mask, cursor, pairs, rows);
  const int rem = key_bits - bits;
  hipLaunchKernelGGL(bs_sort_small_k, dim3(nb), dim3(BS_SMALL_T), 0, c->stream, (const ulonglong2*)pairs, (const unsigned*)counts,
                     (const unsigned*)start, rem, (u64*)keys_out, (u64*)cnts_out, rows);
  const size_t big_lds = sizeof(BsBinLds<BS_T, BS_BIG_SBITS>);
  MK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bs_sort_big_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds));
  hipLaunchKernelGGL(bs_sort_big_k, dim3(BS_BIG_GRID), dim3(BS_T), big_lds, c->stream, (const ulonglong2*)pairs,
                     (const unsigned*)counts, (const unsigned*)start, (const unsigned*)big, (const u64*)scal, rem, (u64*)keys_out,
                     (u64*)cnts_out, rows);
  MK_HIP(hipGetLastError());
  *d_scal = (const uint64_t*)scal;
  return MK_OK;
}
