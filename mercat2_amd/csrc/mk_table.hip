// mk_table.hip -- chunk-table -> running-table kernels.
//
// Replaces (a) the per-file min_count filter of find_kmers (lib/mercat2_kmers.py:73-76: keep a
// key iff its count IN THIS FILE/CHUNK is >= min_count) and (b) run_mercat2's merge of the
// surviving dicts (bin/mercat2.py:121-127: kmers[k] += v).  The filter is applied per chunk,
// before the merge -- there is no post-merge filter in the reference (SURVEY.md trap T2).
#include "mk_common.h"
#include "mk_device.h"
#include "mk_tableview.h"
#include <type_traits>

// Every kernel of this file is launched like this: 256 threads a workgroup, on the context's stream.
template <class... A>
static int launch(mk_ctx* c, void (*kernel)(A...), unsigned grid, std::common_type_t<A>... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, c->stream, args...);
  MK_HIP(hipGetLastError());
  return MK_OK;
}

// ----------------------------------------------------------------------------------- clear
__global__ void mk_clear_slots_k(MkSlot* __restrict__ t, size_t slots) {
  const ulonglong2 e = make_ulonglong2(MK_EMPTY, 0ull);
  mk_for_each(slots, [&](size_t i) { reinterpret_cast<ulonglong2*>(t)[i] = e; });
}

// A free MkSlot holds the key MK_EMPTY; a free MkSlot128 and an empty bin are all zero bits.
int mk_clear_table(mk_ctx* c, int kind, void* t, size_t slots) {
  if (!slots) return MK_OK;
  if (kind == MK_TABLE_TWO) MK_HIP(hipMemsetAsync(t, 0, slots * sizeof(MkSlot128), c->stream));
  else if (kind == MK_TABLE_DENSE) MK_HIP(hipMemsetAsync(t, 0, slots * sizeof(u64), c->stream));
  else return launch(c, mk_clear_slots_k, grid_for(slots, 256, 16384), (MkSlot*)t, slots);
  return MK_OK;
}

// ------------------------------------------------------------------------------ survivors
__global__ void mk_count_survivors_k(const MkSlot* __restrict__ t, size_t slots, u64 min_count, u64* __restrict__ out) {
  u64 mine = 0;
  mk_for_each(slots, [&](size_t i) {
    ulonglong2 s = reinterpret_cast<const ulonglong2*>(t)[i];
    mine += ((s.x != MK_EMPTY) & (s.y >= min_count)) ? 1 : 0;  // (no short cut: the slot stays one 16-byte load)
  });
  block_add(out, mine);
}

int mk_launch_count_survivors(mk_ctx* c, uint64_t min_count) {
  MkChunkInfo* info = (MkChunkInfo*)c->info.p;
  if (!c->rtab_chunk_slots) return MK_OK;
  return launch(c, mk_count_survivors_k, grid_for(c->rtab_chunk_slots, 256, 8192), (const MkSlot*)c->rtab_chunk.p,
                c->rtab_chunk_slots, min_count, &info->survivors_ref);
}

// ------------------------------------------------------------------- running table: hash64
// A key's probe sequence starts at a mixing hash of the key (mask = slots - 1, a power of two).
// Returns true when the key was new to the table.  (Its read-only counterpart: find64, mk_tableview.h.)
__device__ __forceinline__ bool upsert64(MkSlot* __restrict__ table, u64 mask, u64 key, u64 add) {
  u64 slot = mk_mix64(key) & mask;
  for (;;) {
    u64 cur = table[slot].key;
    bool fresh = false;
    if (cur == MK_EMPTY) {
      cur = atomicCAS(&table[slot].key, MK_EMPTY, key);
      if (cur == MK_EMPTY) { cur = key; fresh = true; }
    }
    if (cur == key) {
      atomicAdd(&table[slot].cnt, add);
      return fresh;
    }
    slot = (slot + 1) & mask;
  }
}

// The same for keys that are DISTINCT within the launch and that no other launch adds to at the same time -- the
// survivors of one chunk: every key sits in exactly one bucket and is emitted once.  Then only the CLAIM of a free slot
// races (two new keys may want it: compare-and-swap); the count of a slot that holds the key is this lane's alone and
// is read and written with plain accesses -- one 16-byte load and one 8-byte store per key instead of a load and an
// atomic add that the L2 has to serialise (canonical S2: 2.2 M survivors per chunk; the merge was a third of the step).
__device__ __forceinline__ bool upsert64_distinct(MkSlot* __restrict__ table, u64 mask, u64 key, u64 add) {
  u64 slot = mk_mix64(key) & mask;
  for (;;) {
    const ulonglong2 s = *reinterpret_cast<const ulonglong2*>(&table[slot]);
    u64 cur = s.x;
    if (cur == key) {
      table[slot].cnt = s.y + add;
      return false;
    }
    if (cur == MK_EMPTY) {
      cur = atomicCAS(&table[slot].key, MK_EMPTY, key);
      if (cur == MK_EMPTY) {
        table[slot].cnt = add;  // (the slot was cleared: its count is zero, and it is this key's from now on)
        return true;
      }
      if (cur == key) {  // (cannot happen for distinct keys; kept exact anyway)
        atomicAdd(&table[slot].cnt, add);
        return false;
      }
    }
    slot = (slot + 1) & mask;
  }
}

// ------------------------------------------------------------- running table: two-word keys
// Insert-add of one {hi, lo} key (protocol: MkSlot128 in mk_common.h).  A lane that claims a slot writes the
// key words and publishes the count inside the loop iteration in which it won, so lanes of the same wave that
// meet MK_LOCK128 and look again cannot starve it.  Returns true when the key was new.  (home128 and the read-only
// counterpart, find128: mk_tableview.h.)

// Ordering without cache maintenance: every access to a slot's words is an agent-scope atomic (sc1: performed at the
// device's point of coherence, per-location coherent across the XCDs' L2s by themselves).  The claimer's two key stores
// are write-through; `s_waitcnt vmcnt(0)` holds the publishing store back until both have been acknowledged.  A C++
// release store / acquire fence at agent scope would do the same job with `buffer_wbl2 sc1` / `buffer_inv sc1` -- a
// write-back and an invalidation of the XCD's whole L2 -- per NEW ROW and per probe: measured on 2.1 M new rows
// (protein 13-mers, tools/aa128_probe.py) 5.3 ms against 0.6 ms for the merge kernel.
// The fast form leans on two gfx9-family facts: stores are counted in vmcnt (gfx10+ counts them in vscnt, which this wait
// would not cover) and sc1 accesses are served at the device's point of coherence.  Any other target takes the C++ form.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__) && !defined(MK_UPSERT128_FENCES)
#define MK_UPSERT128_FENCES 1
#endif
#ifdef MK_UPSERT128_FENCES  // (A/B builds: the C++ memory-order form)
#define MK_PUBLISH128(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT)
#define MK_ACQUIRE128() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#else
#define MK_PUBLISH128(p, v)                                                        \
  do {                                                                             \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                               \
    __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      \
  } while (0)
#define MK_ACQUIRE128() asm volatile("" ::: "memory")
#endif
__device__ __forceinline__ bool upsert128(MkSlot128* __restrict__ t, u64 mask, u64 hi, u64 lo, u64 add) {
  u64 slot = home128(hi, lo, mask);
  bool done = false, fresh = false;
  while (!done) {
    u64 st = __hip_atomic_load(&t[slot].cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (st == 0) {
      st = atomicCAS(&t[slot].cnt, 0ull, MK_LOCK128);
      if (st == 0) {
        __hip_atomic_store(&t[slot].hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&t[slot].lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        MK_PUBLISH128(&t[slot].cnt, add);
        done = true;
        fresh = true;
      }
    }
    if (!done && st != MK_LOCK128) {  // a published slot: its key words are final
      MK_ACQUIRE128();
      const u64 h2 = __hip_atomic_load(&t[slot].hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const u64 l2 = __hip_atomic_load(&t[slot].lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (h2 == hi && l2 == lo) {
        atomicAdd(&t[slot].cnt, add);
        done = true;
      } else {
        slot = (slot + 1) & mask;
      }
    }
  }
  return fresh;
}

// ---- where rows go: put(a, b, count) -> the key was new to the table ---------------------------------------------
// The all-ones key (32 x 'T') cannot live in the one-word table (it is the free-slot mark): wherever it stands in
// the rows -- rows received from several peers are a concatenation of sorted segments -- its count goes
// to *side (the context keeps that one key beside the table).
// DISTINCT: the plain-store upsert, for keys that are distinct within the launch (a chunk's survivors: every key is
// counted in one bucket) into a table nobody else writes meanwhile.
template <bool DISTINCT>
struct Sink64 {
  MkSlot* run;
  u64 mask;
  u64* side;
  static constexpr int W = 1;
  static constexpr bool COUNTS = true;
  __device__ __forceinline__ bool put(u64 key, u64, u64 cnt) const {
    if (key == MK_EMPTY) { atomicAdd(side, cnt); return false; }
    return DISTINCT ? upsert64_distinct(run, mask, key, cnt) : upsert64(run, mask, key, cnt);
  }
};
struct Sink128 {
  MkSlot128* run;
  u64 mask;
  static constexpr int W = 2;
  static constexpr bool COUNTS = true;
  __device__ __forceinline__ bool put(u64 hi, u64 lo, u64 cnt) const { return upsert128(run, mask, hi, lo, cnt); }
};
struct SinkBins {  // (a bin is never new: these instances count no rows)
  u64* bins;
  size_t nbins;
  static constexpr int W = 1;
  static constexpr bool COUNTS = false;
  __device__ __forceinline__ bool put(u64 bin, u64, u64 cnt) const {
    if (bin < nbins) atomicAdd(&bins[bin], cnt);
    return false;
  }
};

// Every row of a source (mk_tableview.h: columns, interleaved rows, another table's slots) into a sink.
template <class Source, class Sink>
__global__ void mk_import_k(Source src, size_t rows, Sink sink, u64* __restrict__ new_rows) {
  u64 fresh = 0;
  mk_for_each(rows, [&](size_t i) {
    u64 a, b, cnt;
    if (src.get(i, a, b, cnt)) fresh += sink.put(a, b, cnt) ? 1 : 0;
  });
  if constexpr (Sink::COUNTS) block_add(new_rows, fresh);
}

// Survivors laid out per bucket: bucket b holds nsurv[b] rows {ka, (kb,) cnts} from kstart[b] on. One wave per bucket.
template <class Sink>
__global__ void mk_import_regions_k(const u64* __restrict__ ka, const u64* __restrict__ kb, const u64* __restrict__ cnts,
                                    const u64* __restrict__ kstart, const u64* __restrict__ nsurv, size_t p1, Sink sink,
                                    u64* __restrict__ new_rows) {
  u64 fresh = 0;
  const int lane = threadIdx.x & 63;
  for (size_t b = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < p1; b += (size_t)gridDim.x * (blockDim.x >> 6)) {
    const u64 base = kstart[b], n = nsurv[b];
    for (u64 i = lane; i < n; i += 64) fresh += sink.put(ka[base + i], Sink::W == 2 ? kb[base + i] : 0, cnts[base + i]) ? 1 : 0;
  }
  block_add(new_rows, fresh);
}

static Sink128 sink128(mk_ctx* c) { return Sink128{(MkSlot128*)c->run128.p, (u64)(c->run128_slots - 1)}; }
template <bool DISTINCT>
static Sink64<DISTINCT> sink64(mk_ctx* c) {
  return Sink64<DISTINCT>{(MkSlot*)c->run.p, (u64)(c->run_slots - 1), &((MkChunkInfo*)c->info.p)->side};
}
static SinkBins sink_bins(mk_ctx* c) { return SinkBins{(u64*)c->run.p, (size_t)1 << (c->bits * c->k)}; }

int mk_launch_import_regions(mk_ctx* c, const uint64_t* d_keys, const uint64_t* d_counts, const uint64_t* kstart,
                             const uint64_t* nsurv, size_t p1, size_t survivors) {
  MkChunkInfo* info = (MkChunkInfo*)c->info.p;
  // (few workgroups, each wave walking several buckets: every workgroup ends with one add to the same counter, and
  // adds to one address are serialised by the L2 at ~4 ns each)
  // Many survivors per bucket (-c 1, canonical keys: a bucket keeps a thousand keys, each upsert is two dependent
  // round trips to HBM): every bucket gets its own wave at once -- the kernel is bound by requests in flight.
  const unsigned cap = survivors > 64 * p1 ? 4096u : 512u;
  // (the plain-store form is chosen and enqueued under the table's lock, shared: a context that attaches as a sharer
  // meanwhile -- mk_share_table, the lock exclusive -- drains this stream before its first launch into the table)
  std::shared_lock<std::shared_mutex> rd(c->table_mu);
  const u64 *keys = (const u64*)d_keys, *cnts = (const u64*)d_counts, *ks = (const u64*)kstart, *ns = (const u64*)nsurv;
  // (with sharers the counts are added with atomics: other contexts' count kernels upsert into the table at the same time)
  if (c->n_sharers)
    return launch(c, mk_import_regions_k<Sink64<false>>, grid_for(p1 * 64, 256, cap), keys, nullptr, cnts, ks, ns, p1,
                  sink64<false>(c), &info->new_rows);
  return launch(c, mk_import_regions_k<Sink64<true>>, grid_for(p1 * 64, 256, cap), keys, nullptr, cnts, ks, ns, p1,
                sink64<true>(c), &info->new_rows);
}

// Survivors of the partitioned 33..64-mer path: {hi, lo, count} per bucket region.
int mk_launch_import128_regions(mk_ctx* c, const uint64_t* hi, const uint64_t* lo, const uint64_t* cnts, const uint64_t* kstart,
                                const uint64_t* nsurv, size_t p1) {
  MkChunkInfo* info = (MkChunkInfo*)c->info.p;
  return launch(c, mk_import_regions_k<Sink128>, grid_for(p1 * 64, 256, 512), (const u64*)hi, (const u64*)lo, (const u64*)cnts,
                (const u64*)kstart, (const u64*)nsurv, p1, sink128(c), &info->new_rows);
}

// Rows as columns: keys (two-word keys: {hi, lo} interleaved) + counts.  Another context's or rank's table, where the
// same key may come more than once, or (distinct) a chunk's survivors from the direct-index and the 8-byte-key paths.
int mk_launch_import_pairs(mk_ctx* c, const uint64_t* d_keys, const uint64_t* d_counts, size_t rows, bool distinct) {
  if (!rows) return MK_OK;
  u64* new_rows = &((MkChunkInfo*)c->info.p)->new_rows;
  const Cols64 cols{(const u64*)d_keys, (const u64*)d_counts};
  if (c->mode == MK_MODE_HASH128)
    return launch(c, mk_import_k<Cols128, Sink128>, grid_for(rows, 256, 8192), Cols128{cols.keys, cols.cnts}, rows, sink128(c), new_rows);
  if (c->mode == MK_MODE_DENSE) return launch(c, mk_import_k<Cols64, SinkBins>, grid_for(rows), cols, rows, sink_bins(c), new_rows);
  std::shared_lock<std::shared_mutex> rd(c->table_mu);  // (the plain-store form: see mk_launch_import_regions)
  if (distinct && c->mode == MK_MODE_HASH64 && !c->n_sharers)
    return launch(c, mk_import_k<Cols64, Sink64<true>>, grid_for(rows, 256, 8192), cols, rows, sink64<true>(c), new_rows);
  return launch(c, mk_import_k<Cols64, Sink64<false>>, grid_for(rows, 256, 8192), cols, rows, sink64<false>(c), new_rows);
}

// Interleaved rows {key word(s), count} (dense: {bin, count}).
int mk_launch_import_rows(mk_ctx* c, const uint64_t* d_rows, size_t rows) {
  if (!rows) return MK_OK;
  u64* new_rows = &((MkChunkInfo*)c->info.p)->new_rows;
  const Rows64 rows2{(const ulonglong2*)d_rows};
  if (c->mode == MK_MODE_DENSE) return launch(c, mk_import_k<Rows64, SinkBins>, grid_for(rows), rows2, rows, sink_bins(c), new_rows);
  if (c->mode == MK_MODE_HASH64)
    return launch(c, mk_import_k<Rows64, Sink64<false>>, grid_for(rows, 256, 8192), rows2, rows, sink64<false>(c), new_rows);
  if (c->mode == MK_MODE_HASH128)
    return launch(c, mk_import_k<Rows128, Sink128>, grid_for(rows, 256, 8192), Rows128{(const u64*)d_rows}, rows, sink128(c), new_rows);
  c->err = "import of packed rows: the context has no packed table";
  return MK_ERR_STATE;
}

// Every row of another one-word table (same device) summed into c's.
int mk_launch_merge_table64(mk_ctx* c, const MkSlot* from, size_t from_slots) {
  if (!from_slots) return MK_OK;
  return launch(c, mk_import_k<View64, Sink64<false>>, grid_for(from_slots, 256, 2048), View64{from}, from_slots, sink64<false>(c),
                &((MkChunkInfo*)c->info.p)->new_rows);
}

// ------------------------------------------------------------------- running table: dense
__global__ void mk_accumulate_dense_k(u64* __restrict__ chunk, size_t nbins, u64 min_count, u64* __restrict__ run) {
  mk_for_each(nbins, [&](size_t i) {
    u64 v = chunk[i];
    if (v >= min_count && v) run[i] += v;
    chunk[i] = 0;
  });
}
__global__ void mk_refilter_dense_k(u64* __restrict__ bins, size_t nbins, u64 min_count) {
  mk_for_each(nbins, [&](size_t i) {
    if (bins[i] < min_count) bins[i] = 0;
  });
}
int mk_launch_refilter_dense(mk_ctx* c, uint64_t* bins, size_t nbins, uint64_t min_count) {
  return launch(c, mk_refilter_dense_k, grid_for(nbins), (u64*)bins, nbins, min_count);
}

// --------------------------------------------------------------- running table: by reference
// Running slot key = (tag << 40) | arena row; the k bytes of row r live at arena[r*k .. r*k+k).
// Arena bytes written in this launch are read by other workgroups of the same launch, so they
// are read with agent-scope loads (never from a stale L1 line).
__device__ __forceinline__ unsigned ld_u8_agent(const uint8_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The k-mer text comes through an accessor get(i) -> byte i, so the same code serves text held in
// memory (chunk stream, staging buffer: BytesAt, mk_tableview.h) and text decoded on the fly from packed keys.
// (poly_hash_of and the read-only counterpart of upsert_ref_of, find_ref: mk_tableview.h.)
struct Key128Text {  // 2-bit packed, left-aligned {hi, lo}: base i of the k-mer
  u64 hi, lo;
  __device__ __forceinline__ unsigned operator()(int i) const {
    const unsigned code = (unsigned)((i < 32 ? hi >> (62 - 2 * i) : lo >> (62 - 2 * (i - 32))) & 3u);
    return (unsigned)"ACGT"[code];
  }
};

__device__ __forceinline__ u64 poly_hash(const uint8_t* __restrict__ s, int k) { return poly_hash_of(BytesAt{s}, k); }

template <class Get>
__device__ __forceinline__ bool upsert_ref_of(MkSlot* __restrict__ run, u64 mask, uint8_t* __restrict__ arena, const Get& get,
                                              int k, u64 add, u64 arena_base, u64* __restrict__ new_rows) {
  const u64 h = poly_hash_of(get, k);
  const u64 tag = (h >> 41) << REF_POS_BITS;
  u64 slot = h & mask;
  u64 my_row = MK_EMPTY;
  for (;;) {
    u64 cur = __hip_atomic_load(&run[slot].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == MK_EMPTY) {
      if (my_row == MK_EMPTY) {
        my_row = arena_base + atomicAdd(new_rows, 1ull);
        uint8_t* dst = arena + my_row * (u64)k;
        for (int i = 0; i < k; ++i)
          __hip_atomic_store(dst + i, (uint8_t)get(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (the row's bytes are write-through stores; they are acknowledged before the slot that names the row is claimed.
        // A __threadfence() here is a write-back and an invalidation of the XCD's L2 per NEW ROW: see upsert128)
#ifdef MK_UPSERT128_FENCES
        __threadfence();
#else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
      }
      cur = atomicCAS(&run[slot].key, MK_EMPTY, tag | my_row);
      if (cur == MK_EMPTY) {
        atomicAdd(&run[slot].cnt, add);
        return true;
      }
    }
    if ((cur & ~REF_POS_MASK) == tag && my_row == MK_EMPTY) {
      const uint8_t* other = arena + (cur & REF_POS_MASK) * (u64)k;
      bool same = true;
      for (int i = 0; i < k && same; ++i) same = ld_u8_agent(other + i) == get(i);
      if (same) {
        atomicAdd(&run[slot].cnt, add);
        return false;
      }
    }
    slot = (slot + 1) & mask;
  }
}

__device__ __forceinline__ bool upsert_ref(MkSlot* __restrict__ run, u64 mask, uint8_t* __restrict__ arena,
                                           const uint8_t* __restrict__ str, int k, u64 add, u64 arena_base,
                                           u64* __restrict__ new_rows) {
  return upsert_ref_of(run, mask, arena, BytesAt{str}, k, add, arena_base, new_rows);
}

// Survivors of the by-reference chunk table -> running by-reference table. Within one launch
// every inserted string is distinct (they come from distinct chunk slots), so once a thread
// has reserved an arena row (my_row) its string is known to be new and it only looks for a
// free slot.
// run128 != nullptr (contexts of nucleotide 33..64-mers): a surviving row whose k bytes are all ACGT is a
// packed two-word key and goes to the packed table (every such key lives there and only there); rows
// holding other characters stay text.
__global__ void mk_accumulate_ref_k(const MkSlot* __restrict__ from, size_t slots, u64 min_count,
                                    const uint8_t* __restrict__ seq, int k, MkSlot* __restrict__ run, u64 run_mask,
                                    uint8_t* __restrict__ arena, u64 arena_base, u64* __restrict__ new_rows,
                                    MkSlot128* __restrict__ run128, u64 run128_mask, u64* __restrict__ new_rows128, int aa) {
  u64 fresh128 = 0;  // (one add per workgroup at the end: a counter every new row adds to is serialised by the L2, ~4 ns a row)
  mk_for_each(slots, [&](size_t i) {
    ulonglong2 s = reinterpret_cast<const ulonglong2*>(from)[i];
    if (s.x != MK_EMPTY && s.y >= min_count && s.y != 0) {
      const uint8_t* str = seq + (s.x & REF_POS_MASK);
      bool packed = run128 != nullptr;
      u64 hi = 0, lo = 0;
      if (packed && aa) {  // amino acids: the key is the number sum(code_j * 32^(k-1-j)), code = letter - 'A' (mk_count.hip)
        unsigned __int128 v = 0;
        for (int j = 0; j < k && packed; ++j) {
          const unsigned ch = str[j];
          if (ch < 'A' || ch > 'Z') packed = false;
          else v = (v << 5) | (unsigned __int128)(ch - 'A');
        }
        hi = (u64)(v >> 64);
        lo = (u64)v;
      } else if (packed) {
        for (int j = 0; j < k && packed; ++j) {
          const unsigned ch = str[j];
          const unsigned code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
          if (code > 3u) packed = false;
          else if (j < 32) hi |= (u64)code << (62 - 2 * j);
          else lo |= (u64)code << (62 - 2 * (j - 32));
        }
      }
      if (packed) fresh128 += upsert128(run128, run128_mask, hi, lo, s.y) ? 1 : 0;
      else upsert_ref(run, run_mask, arena, str, k, s.y, arena_base, new_rows);
    }
  });
  if (run128) block_add(new_rows128, fresh128);
}

// Strings from a staging buffer (rows*k bytes), e.g. rows received from another GPU. Distinct
// among themselves as well (they are rows of one table).
__global__ void mk_import_ref_k(const uint8_t* __restrict__ strs, const u64* __restrict__ cnts, size_t rows, int k,
                                MkSlot* __restrict__ run, u64 run_mask, uint8_t* __restrict__ arena, u64 arena_base,
                                u64* __restrict__ new_rows) {
  mk_for_each(rows, [&](size_t i) {
    if (cnts[i]) upsert_ref(run, run_mask, arena, strs + i * (size_t)k, k, cnts[i], arena_base, new_rows);
  });
}

int mk_launch_import_ref(mk_ctx* c, const uint8_t* d_kmers, const uint64_t* d_counts, size_t rows) {
  if (!rows) return MK_OK;
  MkChunkInfo* info = (MkChunkInfo*)c->info.p;
  return launch(c, mk_import_ref_k, grid_for(rows, 256, 8192), d_kmers, (const u64*)d_counts, rows, c->k, (MkSlot*)c->run_ref.p,
                (u64)(c->run_ref_slots - 1), (uint8_t*)c->arena.p, (u64)c->run_ref_rows, &info->new_rows_ref);
}

// Filter + merge of the chunk tables into the running tables (capacities already ensured).
int mk_launch_accumulate(mk_ctx* c, uint64_t min_count) {
  MkChunkInfo* info = (MkChunkInfo*)c->info.p;
  int rc = MK_OK;
  mk_prof_begin(c, MK_K_FILTER);
  if (c->mode == MK_MODE_DENSE) {
    const size_t nbins = (size_t)1 << (c->bits * c->k);
    rc = launch(c, mk_accumulate_dense_k, grid_for(nbins), (u64*)c->ctab.p, nbins, min_count, (u64*)c->run.p);
  }
  if (rc == MK_OK && c->rtab_chunk_slots && c->h_info->survivors_ref)
    rc = launch(c, mk_accumulate_ref_k, grid_for(c->rtab_chunk_slots, 256, 8192), (const MkSlot*)c->rtab_chunk.p,
                c->rtab_chunk_slots, min_count, (const uint8_t*)c->seq.p, c->k, (MkSlot*)c->run_ref.p,
                (u64)(c->run_ref_slots - 1), (uint8_t*)c->arena.p, (u64)c->run_ref_rows, &info->new_rows_ref,
                c->mode == MK_MODE_HASH128 ? (MkSlot128*)c->run128.p : (MkSlot128*)nullptr,
                (u64)(c->run128_slots ? c->run128_slots - 1 : 0), &info->new_rows, c->alphabet == MK_ALPHABET_AA5 ? 1 : 0);
  mk_prof_end(c);
  return rc;
}

// ------------------------------------------------------------------------------- rebuild
// A row that is final into a fresh table where it is not yet: claim the first free slot from its home on.
__device__ __forceinline__ void place(MkSlot* __restrict__ to, u64 to_mask, u64 slot, u64 key, u64, u64 cnt) {
  for (;;) {
    if (atomicCAS(&to[slot].key, MK_EMPTY, key) == MK_EMPTY) {
      to[slot].cnt = cnt;
      break;
    }
    slot = (slot + 1) & to_mask;
  }
}
__device__ __forceinline__ void place(MkSlot128* __restrict__ to, u64 to_mask, u64 slot, u64 hi, u64 lo, u64 cnt) {
  for (;;) {
    if (atomicCAS(&to[slot].cnt, 0ull, cnt) == 0ull) {
      to[slot].hi = hi;
      to[slot].lo = lo;
      break;
    }
    slot = (slot + 1) & to_mask;
  }
}
// Home slot of a row, by table: the key's hash; by reference, the hash of the arena row the key names.
struct Home64 {
  __device__ __forceinline__ u64 operator()(u64 key, u64, u64 mask) const { return mk_mix64(key) & mask; }
};
struct Home128 {
  __device__ __forceinline__ u64 operator()(u64 hi, u64 lo, u64 mask) const { return home128(hi, lo, mask); }
};
struct HomeRef {
  const uint8_t* arena;
  int k;
  __device__ __forceinline__ u64 operator()(u64 key, u64, u64 mask) const {
    return poly_hash(arena + (key & REF_POS_MASK) * (u64)k, k) & mask;
  }
};

// The rows of a table into a fresh one.  Re-insert after growth: every slot that holds a key (the rows are distinct and,
// by reference, their bytes final).  FILTER: only the rows with count >= min_count (the post-merge filter of a
// single-chunk sample split over several ranks); *kept counts them.
template <class View, class Slot, class Home, bool FILTER>
__global__ void mk_rebuild_k(View from, size_t slots, Slot* __restrict__ to, u64 to_mask, Home home, u64 min_count,
                             u64* __restrict__ kept) {
  u64 mine = 0;
  mk_for_each(slots, [&](size_t i) {
    u64 a, b, cnt;
    if (!(FILTER ? from.get(i, a, b, cnt) && cnt >= min_count : from.keyed(i, a, b, cnt))) return;
    ++mine;
    place(to, to_mask, home(a, b, to_mask), a, b, cnt);
  });
  if constexpr (FILTER) block_add(kept, mine);
}

template <bool FILTER, class View, class Slot, class Home>
static int launch_rebuild(mk_ctx* c, View from, size_t from_slots, Slot* to, size_t to_slots, Home home, uint64_t min_count,
                          uint64_t* d_kept) {
  return launch(c, mk_rebuild_k<View, Slot, Home, FILTER>, grid_for(from_slots, 256, 8192), from, from_slots, to, to_slots - 1, home,
                min_count, (u64*)d_kept);
}
// d_kept != nullptr: keep the rows with count >= min_count and count them there; else every keyed slot.
int mk_launch_rebuild(mk_ctx* c, int kind, const void* from, size_t from_slots, void* to, size_t to_slots, uint64_t min_count,
                      uint64_t* d_kept) {
  if (!from_slots) return MK_OK;
  const View64 v1{(const MkSlot*)from};
  const View128 v2{(const MkSlot128*)from};
  if (kind == MK_TABLE_REF)  // (only ever grown: mk_filter_min filters the rows kept as text on the host)
    return launch_rebuild<false>(c, v1, from_slots, (MkSlot*)to, to_slots, HomeRef{(const uint8_t*)c->arena.p, c->k}, 0, nullptr);
  if (kind == MK_TABLE_TWO)
    return d_kept ? launch_rebuild<true>(c, v2, from_slots, (MkSlot128*)to, to_slots, Home128{}, min_count, d_kept)
                  : launch_rebuild<false>(c, v2, from_slots, (MkSlot128*)to, to_slots, Home128{}, 0, nullptr);
  return d_kept ? launch_rebuild<true>(c, v1, from_slots, (MkSlot*)to, to_slots, Home64{}, min_count, d_kept)
                : launch_rebuild<false>(c, v1, from_slots, (MkSlot*)to, to_slots, Home64{}, 0, nullptr);
}

// --------------------------------------------------------------------------------- compact
// Occupied slots of a table -> (keys, counts) in arbitrary order; *cursor counts them.
// Each workgroup owns a contiguous slice: pass 1 counts its rows, ONE cursor atomic reserves the
// output range, pass 2 (slice is L2-hot) places the rows with a wave-aggregated LDS cursor.
__global__ __launch_bounds__(256) void mk_compact_k(const MkSlot* __restrict__ t, size_t slots, u64* __restrict__ keys,
                                                    u64* __restrict__ cnts, size_t cap, u64* __restrict__ cursor) {
  __shared__ unsigned s_n;
  __shared__ u64 s_base;
  const size_t per = (slots + gridDim.x - 1) / gridDim.x;
  const size_t lo = (size_t)blockIdx.x * per, hi = lo + per < slots ? lo + per : slots;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  unsigned mine = 0;
  for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const ulonglong2 s = reinterpret_cast<const ulonglong2*>(t)[i];
    mine += (s.x != MK_EMPTY && s.y != 0) ? 1u : 0u;
  }
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    s_base = s_n ? atomicAdd(cursor, (u64)s_n) : 0ull;
    s_n = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const size_t rounds = (hi > lo ? hi - lo + blockDim.x - 1 : 0) / blockDim.x;
  for (size_t r = 0; r < rounds; ++r) {
    const size_t i = lo + r * blockDim.x + threadIdx.x;
    ulonglong2 s = make_ulonglong2(MK_EMPTY, 0);
    if (i < hi) s = reinterpret_cast<const ulonglong2*>(t)[i];
    const bool keep = s.x != MK_EMPTY && s.y != 0;
    const u64 m = __ballot(keep);
    if (m) {
      unsigned at = 0;
      if (lane == 0) at = atomicAdd(&s_n, (unsigned)__popcll(m));
      const u64 pos = s_base + __shfl(at, 0) + __popcll(m & ((1ull << lane) - 1));
      if (keep && pos < cap) { keys[pos] = s.x; cnts[pos] = s.y; }
    }
  }
}

int mk_launch_compact(mk_ctx* c, const MkSlot* t, size_t slots, uint64_t* d_keys, uint64_t* d_counts, size_t cap,
                      uint64_t* d_cursor) {
  if (!slots) return MK_OK;
  return launch(c, mk_compact_k, grid_for(slots, 256, 8192), t, slots, (u64*)d_keys, (u64*)d_counts, cap, (u64*)d_cursor);
}

// Two-word keys: occupied slots -> {hi, lo, count} in arbitrary order; *cursor counts them (wave-aggregated cursor).
__global__ __launch_bounds__(256) void mk_compact128_k(const MkSlot128* __restrict__ t, size_t slots, u64* __restrict__ hi,
                                                       u64* __restrict__ lo, u64* __restrict__ cnts, size_t cap,
                                                       u64* __restrict__ cursor) {
  const int lane = threadIdx.x & 63;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t rounds = (slots + stride - 1) / stride;
  for (size_t r = 0; r < rounds; ++r) {
    const size_t i = r * stride + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    ulonglong4 s = make_ulonglong4(0, 0, 0, 0);
    if (i < slots) s = reinterpret_cast<const ulonglong4*>(t)[i];
    const bool keep = s.z != 0;
    const u64 m = __ballot(keep);
    if (m) {
      u64 at = 0;
      if (lane == 0) at = atomicAdd(cursor, (u64)__popcll(m));
      const u64 pos = __shfl(at, 0) + __popcll(m & ((1ull << lane) - 1));
      if (keep && pos < cap) { hi[pos] = s.x; lo[pos] = s.y; cnts[pos] = s.z; }
    }
  }
}

int mk_launch_compact128(mk_ctx* c, const MkSlot128* t, size_t slots, uint64_t* hi, uint64_t* lo, uint64_t* cnts, size_t cap,
                         uint64_t* d_cursor) {
  if (!slots) return MK_OK;
  return launch(c, mk_compact128_k, grid_for(slots, 256, 4096), t, slots, (u64*)hi, (u64*)lo, (u64*)cnts, cap, (u64*)d_cursor);
}

// ------------------------------------------------------------------- alpha-diversity moments
// One pass over the running table(s): everything the nine alpha metrics of lib/mercat2_diversity.py:13-53 need from the
// count column.  A workgroup leaves one record of AL_WORDS words (mk_common.h): rows, sum c, sum c^2 as a 192-bit
// integer (a square takes 128 bits, and no table has 2^64 rows), sum c ln c as a double, the rows with count 1..10.
// Nothing is added in floating point but sum c ln c, and that in a fixed order: a lane adds its slots in ascending
// order, the lanes of a wave fold by the shuffle tree, thread 0 adds the waves in wave order, the host adds the records
// in the order they lie.  No atomic touches a double: the same table gives the same bits.
struct AlphaSums {
  u64 rows = 0, total = 0, sq0 = 0, sq1 = 0, sq2 = 0;
  double clnc = 0;
  __device__ __forceinline__ void add_sq(u64 lo, u64 hi, u64 top) {  // 192-bit add, carries by hand
    sq0 += lo;
    u64 carry = sq0 < lo;
    sq1 += hi;
    u64 carry2 = sq1 < hi;
    sq1 += carry;
    carry2 += sq1 < carry;
    sq2 += top + carry2;
  }
  __device__ __forceinline__ void add(u64 r, u64 t, u64 lo, u64 hi, u64 top, double cl) {
    rows += r;
    total += t;
    add_sq(lo, hi, top);
    clnc += cl;
  }
};
__device__ __forceinline__ void alpha_take(u64 c, AlphaSums& s, unsigned* s_freq) {
  if (!c) return;
  const double d = (double)c;
  s.add(1, c, c * c, __umul64hi(c, c), 0, d * log(d));
  if (c <= 10) atomicAdd(&s_freq[c], 1u);
}
template <class View>
__global__ __launch_bounds__(256) void mk_alpha_k(View v, size_t n, u64* __restrict__ out) {
  __shared__ unsigned s_freq[11];
  __shared__ u64 s_wave[4][5];
  __shared__ double s_clnc[4];
  if (threadIdx.x < 11) s_freq[threadIdx.x] = 0;
  __syncthreads();
  AlphaSums s;
  mk_for_each(n, [&](size_t i) {  // (every thread adds its slots in ascending order)
    u64 a, b, cnt;
    if (v.keyed(i, a, b, cnt)) alpha_take(cnt, s, s_freq);
  });
  for (int d = 32; d > 0; d >>= 1)
    s.add(__shfl_down(s.rows, d), __shfl_down(s.total, d), __shfl_down(s.sq0, d), __shfl_down(s.sq1, d), __shfl_down(s.sq2, d),
          __shfl_down(s.clnc, d));
  if ((threadIdx.x & 63) == 0) {
    u64* w = s_wave[threadIdx.x >> 6];
    w[0] = s.rows; w[1] = s.total; w[2] = s.sq0; w[3] = s.sq1; w[4] = s.sq2;
    s_clnc[threadIdx.x >> 6] = s.clnc;
  }
  __syncthreads();
  u64* rec = out + (size_t)blockIdx.x * AL_WORDS;  // every word of the record is written: nothing to clear beforehand
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) s.add(s_wave[w][0], s_wave[w][1], s_wave[w][2], s_wave[w][3], s_wave[w][4], s_clnc[w]);
    rec[AL_ROWS] = s.rows; rec[AL_TOTAL] = s.total;
    rec[AL_SQ] = s.sq0; rec[AL_SQ + 1] = s.sq1; rec[AL_SQ + 2] = s.sq2;
    rec[AL_CLNC] = (u64)__double_as_longlong(s.clnc);
  }
  if (threadIdx.x >= 1 && threadIdx.x <= 10) rec[AL_FREQ + threadIdx.x] = s_freq[threadIdx.x];
}

int mk_launch_alpha(mk_ctx* c, size_t* records) {
  const auto grid = [](size_t n) { return grid_for(n, 256, 1024); };
  size_t all = 0, at = 0;
  (void)mk_each_table(c, [&](auto, size_t n, int) { all += grid(n); return MK_OK; });
  *records = all;
  if (!all) return MK_OK;
  int rc;
  if ((rc = mk_buf_reserve(c, c->ex_tmp, all * AL_WORDS * sizeof(u64))) != MK_OK) return rc;
  u64* out = (u64*)c->ex_tmp.p;
  return mk_each_table(c, [&](auto v, size_t n, int) {
    u64* recs = out + at * AL_WORDS;
    at += grid(n);
    return launch(c, mk_alpha_k<decltype(v)>, grid(n), v, n, recs);
  });
}

// ------------------------------------------------------------------ two tables combined by key (mk_table_op)
// ---- the OTHER table asked for the key a view hands out: probe(a, b) -> its count there, 0 when absent; each holds the
// fields of the other context's LkTables that it reads.  A table that was never allocated has no slots and answers 0.  The inputs are final (lk_open): in the two-word table an all-ones
// count word is a count.
struct Probe64 {
  const MkSlot* t;
  u64 slots;
  __device__ __forceinline__ u64 operator()(u64 key, u64) const { return slots ? find64(t, slots - 1, key) : 0; }
};
struct Probe128 {
  const MkSlot128* t;
  u64 slots;
  __device__ __forceinline__ u64 operator()(u64 hi, u64 lo) const { return slots ? find128(t, slots - 1, hi, lo, nullptr) : 0; }
};
struct ProbeBins {
  const u64* bins;
  size_t nbins;
  __device__ __forceinline__ u64 operator()(u64 bin, u64) const { return find_dense(bins, nbins, bin); }
};
// Rows kept as text: the view hands out the slot key (tag | arena row) of the table it walks; the row's k bytes, in
// THAT table's arena (from), are what the other table is asked for and what the sink stores.
struct ProbeRef {
  const MkSlot* ref;
  u64 slots;
  const uint8_t *arena, *from;
  int k;
  __device__ __forceinline__ u64 operator()(u64 key, u64) const {
    return slots ? find_ref_of(ref, slots - 1, arena, BytesAt{from + (key & REF_POS_MASK) * (u64)k}, k) : 0;
  }
};
// Two-word keys that are distinct within the launch and new to the table: the first free slot from the key's home on
// is claimed with the count, as the rebuild places a row (no key is compared, no slot waited for: upsert128 would take
// a count of 2^64 - 1 in a slot on its way for MK_LOCK128 and spin).
struct SinkPlace128 {
  MkSlot128* run;
  u64 mask;
  __device__ __forceinline__ bool put(u64 hi, u64 lo, u64 cnt) const {
    place(run, mask, home128(hi, lo, mask), hi, lo, cnt);
    return true;
  }
};
struct SinkRef {
  MkSlot* run;
  u64 mask;
  uint8_t* arena;
  const uint8_t* from;
  int k;
  u64* new_rows;  // (the arena's row cursor: the table was emptied, rows are handed out from 0)
  __device__ __forceinline__ bool put(u64 key, u64, u64 cnt) const {
    return upsert_ref(run, mask, arena, from + (key & REF_POS_MASK) * (u64)k, k, cnt, 0, new_rows);
  }
};

// One table walked through its view (x), the other probed (y), f into the sink: the kernel of mk_table_op, once for
// every table shape.  mk_import_k with a probe between the view and the sink, and with the call's five tallies, which
// that kernel has no place for.
//   SO_SCAN_A  x = a, y = b: every row of a at or above min_a; f(ca, cb) where that is not 0.
//   SO_SCAN_B  x = b, y = a: the rows of b at or above min_b are counted; with `insert` (MAX, SUM: f(0, cb) != 0) a is
//              probed and f(0, cb) goes in for the keys a lacks at or above min_a -- keys the first scan has not met.
//              Without it nothing is probed: the scan only counts rows_b.
//   SO_SCAN_AB dense bins, where slot i is the same key in both: one elementwise pass does all of it.
// Keys coming out of one table are distinct, and those of SO_SCAN_B are distinct from those of SO_SCAN_A: the sinks
// never add to a row, and whatever order the rows arrive in, the table's content is the same.
enum { SO_SCAN_A = 0, SO_SCAN_B = 1, SO_SCAN_AB = 2 };
template <int SCAN, class View, class Probe, class Sink>
__global__ void mk_setop_k(View v, size_t n, Probe probe, Sink sink, int op, int insert, u64 min_x, u64 min_y,
                           u64* __restrict__ out) {
  u64 rows_x = 0, rows_y = 0, both = 0, rows_out = 0, total_out = 0;
  mk_for_each(n, [&](size_t i) {
    u64 a, b, cx;
    if (!(SCAN == SO_SCAN_AB ? v.keyed(i, a, b, cx) : v.get(i, a, b, cx))) return;
    if (cx < min_x) cx = 0;
    if (SCAN != SO_SCAN_AB && !cx) return;
    rows_x += cx ? 1 : 0;
    if (SCAN == SO_SCAN_B && !insert) return;
    u64 cy = probe(a, b);
    if (cy < min_y) cy = 0;
    if (SCAN == SO_SCAN_B && cy) return;  // (a holds it: the first scan has dealt with the key)
    rows_y += cy ? 1 : 0;
    both += (cx && cy) ? 1 : 0;
    const u64 f = SCAN == SO_SCAN_B ? setop_f(op, 0, cx) : setop_f(op, cx, cy);
    if (!f) return;
    rows_out += 1;
    total_out += f;
    sink.put(a, b, f);
  });
  block_add(&out[SCAN == SO_SCAN_B ? MK_SO_ROWS_B : MK_SO_ROWS_A], rows_x);
  if (SCAN == SO_SCAN_AB) block_add(&out[MK_SO_ROWS_B], rows_y);
  if (SCAN != SO_SCAN_B) block_add(&out[MK_SO_BOTH], both);
  block_add(&out[MK_SO_ROWS_OUT], rows_out);
  block_add(&out[MK_SO_TOTAL_OUT], total_out);
}

template <int SCAN, class View, class Probe, class Sink>
static int launch_setop(mk_ctx* dst, View v, size_t n, Probe probe, Sink sink, int op, bool insert, u64 min_x, u64 min_y, u64* d_out) {
  return launch(dst, mk_setop_k<SCAN, View, Probe, Sink>, grid_for(n, 256, 8192), v, n, probe, sink, op, insert ? 1 : 0, min_x, min_y, d_out);
}

// One scan of mk_table_op on dst's stream: x's tables walked (scan_b: x is b, else a), y's probed, the rows into dst's
// tables, which are empty or hold the first scan's rows and have room for every row this scan can add.  The packed
// table's tallies go to d_out[0 .. MK_SO_WORDS), those of the rows kept as text to the MK_SO_WORDS words behind them;
// *slots: table slots read.
int mk_launch_setop(mk_ctx* dst, const mk_ctx* x, const mk_ctx* y, bool scan_b, int op, bool insert, uint64_t min_x, uint64_t min_y,
                    uint64_t* d_out_, uint64_t* slots) {
  u64* d_out = (u64*)d_out_;
  MkChunkInfo* info = (MkChunkInfo*)dst->info.p;
  const LkTables tx = lk_tables(x), ty = lk_tables(y);  // (the same mode: mk_table_op has compared alphabet and k)
  int rc = MK_OK;
#define SO_GO(VIEW, N, PROBE, SINK, OUT)                                                                                     \
  do {                                                                                                                     \
    rc = scan_b ? launch_setop<SO_SCAN_B>(dst, VIEW, N, PROBE, SINK, op, insert, min_x, min_y, OUT)                          \
                : launch_setop<SO_SCAN_A>(dst, VIEW, N, PROBE, SINK, op, insert, min_x, min_y, OUT);                         \
    *slots += N;                                                                                                           \
  } while (0)
  if (x->mode == MK_MODE_DENSE) {
    if (!scan_b) {  // (the one elementwise pass)
      rc = launch_setop<SO_SCAN_AB>(dst, ViewDense{tx.bins}, tx.nbins, ProbeBins{ty.bins, ty.nbins}, sink_bins(dst), op, true, min_x, min_y, d_out);
      *slots += tx.nbins + ty.nbins;
    }
  } else if (tx.run_slots) {
    SO_GO(View64{tx.run}, tx.run_slots, (Probe64{ty.run, ty.run_slots}), sink64<true>(dst), d_out);
  } else if (tx.run128_slots) {
    SO_GO(View128{tx.run128}, tx.run128_slots, (Probe128{ty.run128, ty.run128_slots}),
          (SinkPlace128{(MkSlot128*)dst->run128.p, (u64)(dst->run128_slots - 1)}), d_out);
  }
  if (rc == MK_OK && tx.ref_slots) {
    const ProbeRef probe{ty.ref, ty.ref_slots, ty.arena, tx.arena, x->k};
    const SinkRef sink{(MkSlot*)dst->run_ref.p, (u64)(dst->run_ref_slots - 1), (uint8_t*)dst->arena.p, tx.arena, x->k, &info->new_rows_ref};
    SO_GO(View64{tx.ref}, tx.ref_slots, probe, sink, d_out + MK_SO_WORDS);
  }
#undef SO_GO
  return rc;
}
