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
