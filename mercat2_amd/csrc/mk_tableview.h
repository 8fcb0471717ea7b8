// mk_tableview.h -- the running tables and the rows that travel between them, each behind one call shape, for the
// kernels of mk_table.hip and mk_multi.hip:  get(i, a, b, cnt) -> "there is a row at i": key word(s) a (and b, 0 for
// one-word keys) and its count.
#pragma once
#include "mk_common.h"
#include "mk_device.h"

// f(i) for every i < n, the grid's threads striding over them together.  The workgroup size comes from the builtin:
// inside a helper, blockDim.x compiles to the general form (which of the grid's workgroups is a partial one?), a
// dependent load and seven instructions ahead of every loop that the kernels did not have when they spelled the loop
// out -- every launch here is of whole workgroups.  Start and stride are locals, computed once.
template <class F>
__device__ __forceinline__ void mk_for_each(size_t n, F&& f) {
  const size_t wg = __builtin_amdgcn_workgroup_size_x(), stride = (size_t)gridDim.x * wg;
  for (size_t i = (size_t)blockIdx.x * wg + threadIdx.x; i < n; i += stride) f(i);
}

// ---- the three packed running tables seen as "slot i -> (occupied, key word(s), count)" ------------------------
// get: the slot holds a row (a key and a count that is not zero).  keyed: the slot holds a key, whatever its count --
// what the rebuild after growth carries over and the alpha moments look at (they skip a count of zero themselves).
struct View64 {
  const MkSlot* t;
  static constexpr int W = 1;
  __device__ __forceinline__ bool keyed(size_t i, u64& a, u64& b, u64& c) const {
    const ulonglong2 s = reinterpret_cast<const ulonglong2*>(t)[i];
    a = s.x; b = 0; c = s.y;
    return s.x != MK_EMPTY;
  }
  __device__ __forceinline__ bool get(size_t i, u64& a, u64& b, u64& c) const { return keyed(i, a, b, c) && c != 0; }
};
struct View128 {  // (the count word is the slot's state: a free slot has no key)
  const MkSlot128* t;
  static constexpr int W = 2;
  __device__ __forceinline__ bool get(size_t i, u64& a, u64& b, u64& c) const {
    const ulonglong4 s = reinterpret_cast<const ulonglong4*>(t)[i];
    a = s.x; b = s.y; c = s.z;
    return s.z != 0;
  }
  __device__ __forceinline__ bool keyed(size_t i, u64& a, u64& b, u64& c) const { return get(i, a, b, c); }
};
struct ViewDense {  // (every bin is a key)
  const u64* bins;
  static constexpr int W = 1;
  __device__ __forceinline__ bool keyed(size_t i, u64& a, u64& b, u64& c) const {
    a = (u64)i; b = 0; c = bins[i];
    return true;
  }
  __device__ __forceinline__ bool get(size_t i, u64& a, u64& b, u64& c) const { return keyed(i, a, b, c) && c != 0; }
};

// ---- rows on their way into a table: row i -> (count is not zero, key word(s), count) -------------------------
struct Cols64 {  // two columns
  const u64 *keys, *cnts;
  __device__ __forceinline__ bool get(size_t i, u64& a, u64& b, u64& c) const {
    a = keys[i]; b = 0; c = cnts[i];
    return c != 0;
  }
};
struct Cols128 {  // {hi, lo} interleaved + counts
  const u64 *keys2, *cnts;
  __device__ __forceinline__ bool get(size_t i, u64& a, u64& b, u64& c) const {
    a = keys2[2 * i]; b = keys2[2 * i + 1]; c = cnts[i];
    return c != 0;
  }
};
// Interleaved rows {key, count} / {hi, lo, count}: the layout rows travel in between GPUs (mk_multi.hip,
// mercat2_amd/dist.py), so that a row's words move side by side and are read with one access.
struct Rows64 {
  const ulonglong2* rows2;
  __device__ __forceinline__ bool get(size_t i, u64& a, u64& b, u64& c) const {
    const ulonglong2 r = rows2[i];
    a = r.x; b = 0; c = r.y;
    return c != 0;
  }
};
struct Rows128 {
  const u64* rows3;
  __device__ __forceinline__ bool get(size_t i, u64& a, u64& b, u64& c) const {
    a = rows3[3 * i]; b = rows3[3 * i + 1]; c = rows3[3 * i + 2];
    return c != 0;
  }
};

// ---- where a key's probe sequence starts, per table (the upserts of mk_table.hip and the probes below) ----------
// one-word keys: mk_mix64(key) & mask.  Two-word keys:
__device__ __forceinline__ u64 home128(u64 hi, u64 lo, u64 mask) { return mk_mix64(hi ^ mk_mix64(lo + MK_POLY_B)) & mask; }
// By reference: running slot key = (tag << 40) | arena row, home and tag from the polynomial hash of the k bytes,
// which come through an accessor get(i) -> byte i.
#define REF_POS_BITS 40
#define REF_POS_MASK ((1ull << REF_POS_BITS) - 1)
struct BytesAt {
  const uint8_t* p;
  __device__ __forceinline__ unsigned operator()(int i) const { return p[i]; }
};
template <class Get>
__device__ __forceinline__ u64 poly_hash_of(const Get& get, int k) {
  u64 h = 0;
  for (int i = 0; i < k; ++i) h = h * MK_POLY_B + get(i);
  return mk_mix64(h);
}

// ---- read-only probes of a QUIESCENT running table: the home slot and probe order of the upserts, loads only, ending
// at the key (its count) or at a free slot (0).  Nothing writes the table meanwhile, so plain loads will do.
// One-word table: the slot is one 16-byte load.  `first` is the home slot, already loaded (find64_home: so that a lane
// can have the loads of several keys in flight before it compares any).
__device__ __forceinline__ ulonglong2 find64_home(const MkSlot* __restrict__ t, u64 mask, u64 key) {
  return reinterpret_cast<const ulonglong2*>(t)[mk_mix64(key) & mask];
}
__device__ __forceinline__ u64 find64_from(const MkSlot* __restrict__ t, u64 mask, u64 key, ulonglong2 first) {
  u64 slot = mk_mix64(key) & mask;
  ulonglong2 s = first;
  for (;;) {  // (the table is never full: a free slot is met)
    if (s.x == key) return s.y;
    if (s.x == MK_EMPTY) return 0;
    slot = (slot + 1) & mask;
    s = reinterpret_cast<const ulonglong2*>(t)[slot];
  }
}
__device__ __forceinline__ u64 find64(const MkSlot* __restrict__ t, u64 mask, u64 key) {
  return find64_from(t, mask, key, find64_home(t, mask, key));
}
// Two-word table: the count word is the slot's state, 0 = free.  MK_LOCK128 cannot be met on a quiescent table:
// *locked is set and the probe ends (a state error for the caller, not a spin).  locked == nullptr: the caller vouches
// that the table is final, and an all-ones count word is what it can only be there, a count of 2^64 - 1 (mk_table_op).
__device__ __forceinline__ u64 find128(const MkSlot128* __restrict__ t, u64 mask, u64 hi, u64 lo, bool* locked) {
  u64 slot = home128(hi, lo, mask);
  for (;;) {
    const ulonglong4 s = reinterpret_cast<const ulonglong4*>(t)[slot];
    if (s.z == 0) return 0;
    if (s.z == MK_LOCK128 && locked) { *locked = true; return 0; }
    if (s.x == hi && s.y == lo) return s.z;
    slot = (slot + 1) & mask;
  }
}
// By-reference table: the tag first, the arena bytes only on a tag match.
template <class Get>
__device__ __forceinline__ u64 find_ref_of(const MkSlot* __restrict__ run, u64 mask, const uint8_t* __restrict__ arena,
                                           const Get& get, int k) {
  const u64 h = poly_hash_of(get, k);
  const u64 tag = (h >> 41) << REF_POS_BITS;
  u64 slot = h & mask;
  for (;;) {
    const ulonglong2 s = reinterpret_cast<const ulonglong2*>(run)[slot];
    if (s.x == MK_EMPTY) return 0;
    if ((s.x & ~REF_POS_MASK) == tag) {
      const uint8_t* other = arena + (s.x & REF_POS_MASK) * (u64)k;
      bool same = true;
      for (int i = 0; i < k && same; ++i) same = other[i] == get(i);
      if (same) return s.y;
    }
    slot = (slot + 1) & mask;
  }
}
// Dense bins: one indexed load.
__device__ __forceinline__ u64 find_dense(const u64* __restrict__ bins, size_t nbins, u64 bin) { return bin < nbins ? bins[bin] : 0; }

// ---- the tables of one context, as a probing kernel sees them (mk_lookup.hip, mk_screen.hip); a table that was never
// allocated has no slots
struct LkTables {
  const MkSlot* run;          // one-word keys
  u64 run_slots;
  u64 side;                   // count of the one key kept beside it (32 x 'T' == MK_EMPTY)
  const u64* bins;            // dense mode: the bins instead
  u64 nbins;
  const MkSlot128* run128;    // two-word keys
  u64 run128_slots;
  const MkSlot* ref;          // keys kept as text
  u64 ref_slots;
  const uint8_t* arena;
};
static inline LkTables lk_tables(const mk_ctx* c) {
  LkTables t{};
  if (c->mode == MK_MODE_DENSE) { t.bins = (const u64*)c->run.p; t.nbins = c->run_slots; }
  else if (c->mode == MK_MODE_HASH64) { t.run = (const MkSlot*)c->run.p; t.run_slots = c->run_slots; t.side = c->run_side; }
  else if (c->mode == MK_MODE_HASH128) { t.run128 = (const MkSlot128*)c->run128.p; t.run128_slots = c->run128_slots; }
  t.ref = (const MkSlot*)c->run_ref.p;
  t.ref_slots = c->run_ref_slots;
  t.arena = (const uint8_t*)c->arena.p;
  return t;
}
