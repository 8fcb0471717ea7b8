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

// ---- the tables of one context, as a reading kernel sees them: the one place where the context's buffers are given
// their types.  A table that was never allocated has no slots.
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

// f(view, slots, kind: MkTableKind) for every table the context holds -- the dense bins or else the one-word table, then
// the by-reference table, then the two-word table, each only if it has slots -- until one answers other than MK_OK.
// (The one key kept beside the one-word table is no slot: whoever walks the tables adds run_side itself.)
template <class F>
static inline int mk_each_table(const mk_ctx* c, F&& f) {
  const LkTables t = lk_tables(c);
  int rc = MK_OK;
  if (c->mode == MK_MODE_DENSE) rc = f(ViewDense{t.bins}, (size_t)t.nbins, MK_TABLE_DENSE);
  else if (t.run_slots) rc = f(View64{t.run}, (size_t)t.run_slots, MK_TABLE_ONE);
  if (rc == MK_OK && t.ref_slots) rc = f(View64{t.ref}, (size_t)t.ref_slots, MK_TABLE_REF);
  if (rc == MK_OK && t.run128_slots) rc = f(View128{t.run128}, (size_t)t.run128_slots, MK_TABLE_TWO);
  return rc;
}

// The kind of key a context packs: one word, two words (nucleotide 33..64-mers; amino acid 13..25-mers), or none -- every
// key is kept as text.
enum TlKeys { TL_ONE_WORD = 0, TL_TWO_WORD_NT = 1, TL_TWO_WORD_AA = 2, TL_TEXT_ONLY = 3 };
static inline int tl_keys_of(const mk_ctx* c) {
  return c->mode == MK_MODE_BYREF ? TL_TEXT_ONLY
         : c->mode != MK_MODE_HASH128 ? TL_ONE_WORD
         : c->alphabet == MK_ALPHABET_NT2 ? TL_TWO_WORD_NT : TL_TWO_WORD_AA;
}

// A probe is a dependent random 16-byte read: a lane that looks one key up after the other waits a full trip to HBM per
// key.  PER keys a lane: the home-slot loads of all of them are issued before any is compared (one-word table).  The
// knob of mk_lookup.hip; the windows of mk_screen.hip take as many (SC_PER).
// (A/B builds: -DLK_PER=1 is the one-key-a-lane form tools/lookup_probe.py's figures are compared with.)
#ifndef LK_PER
#define LK_PER 4
#endif

// ---- one key looked up by a kernel that has PER keys a lane in flight (lk_probe_k; sc_probe_k takes the fold).  KEYS: the kind of the
// context's packed keys.  j is a constant under #pragma unroll: the arrays live in registers.
//   fold    the key onto its reverse complement where that is smaller (one-word and two-word nucleotide keys)
//   issue   a packed key: dense bins and the two-word table answer at once, the all-ones one-word key is the one kept
//           beside its table, any other one-word key has its home slot loaded and is left pending, so that a lane has
//           the loads of all its keys in flight before it compares any
//   issue   a key kept as text, its k bytes through an accessor: the by-reference table answers at once
//   finish  the count, a pending key's probe brought to its end
// locked: a slot of the two-word table was being claimed (cannot happen on a quiescent table; the caller reports it).
// A word, not a bool: as a bool it is a lane mask in two scalar registers across the whole loop, and the two-word
// instances of both kernels spill scalars for it.
template <int KEYS, int PER>
struct LkStep {
  u64 key[PER], res[PER];
  ulonglong2 home[PER];
  bool pending[PER];
  unsigned locked = 0;

  static __device__ __forceinline__ bool fold(u64& a, u64& b, int k) {
    if (KEYS == TL_TWO_WORD_NT) return mk_canon128(a, b, k);
    const u64 rc = mk_revcomp2(a, k);
    const bool turned = rc < a;
    if (turned) a = rc;
    return turned;
  }
  __device__ __forceinline__ void clear(int j) { pending[j] = false; res[j] = 0; }
  __device__ __forceinline__ void issue(int j, const LkTables& t, u64 a, u64 b) {
    if (KEYS == TL_ONE_WORD) {
      if (t.bins) res[j] = find_dense(t.bins, (size_t)t.nbins, a);
      else if (a == MK_EMPTY) res[j] = t.side;
      else if (t.run_slots) {
        key[j] = a;
        home[j] = find64_home(t.run, t.run_slots - 1, a);
        pending[j] = true;
      }
    } else if (t.run128_slots) {
      bool met = false;
      res[j] = find128(t.run128, t.run128_slots - 1, a, b, &met);
      locked |= met ? 1u : 0u;
    }
  }
  template <class Get>
  __device__ __forceinline__ void issue(int j, const LkTables& t, const Get& get, int k) {
    if (t.ref_slots) res[j] = find_ref_of(t.ref, t.ref_slots - 1, t.arena, get, k);
  }
  __device__ __forceinline__ u64 finish(int j, const LkTables& t) {
    if (pending[j]) res[j] = find64_from(t.run, t.run_slots - 1, key[j], home[j]);
    return res[j];
  }
};

// ---- f(ca, cb) of mk_table_op (include/mercat_hip.h): in mk_setop_k, where op is uniform over the launch, and on the
// host for the one key kept beside the one-word table
__host__ __device__ static inline u64 setop_f(int op, u64 ca, u64 cb) {
  switch (op) {
    case MK_OP_MIN: return ca < cb ? ca : cb;
    case MK_OP_MAX: return ca > cb ? ca : cb;
    case MK_OP_SUM: return ca + cb;
    case MK_OP_LEFT: return cb ? ca : 0;
    case MK_OP_ONLY: return cb ? 0 : ca;
    default: return ca > cb ? ca - cb : 0;  // MK_OP_DIFF
  }
}
