// mk_dedup.hip -- duplicate reads of a FASTQ text (mk_fastq_dedup_text / mk_fastq_dedup_device, include/mercat_hip.h
// has the rule): reads, or pairs, whose key bytes are equal form a cluster, and the one of lowest index over the whole
// call stays.  The line index, the piece loop, the prefix sum and the gather are mk_fqpiece.h's; new here is a hash table
// keyed by a variable-length sequence, which is held by reference: a slot names a unit, and the unit's key is read from
// the text, which therefore stays on the device for the length of the call.
//   dd_key_k      qt_scan_k's layout: 16 lanes a record, four records a wave, a lane an aligned 16-byte granule of the
//                 sequence line a pass.  The hash is sum(byte[i] * M^(i + 16)) mod 2^64 over the content positions i of
//                 the key, mixed with its length: a lane forms its 16 terms by Horner's rule, multiplies by the power of
//                 its first position, a DPP row reduction adds the lanes.  A function of the key bytes alone: the same
//                 read at every alignment of its line hashes alike.  Writes ref[record] = {offset of the key in the
//                 resident text, length, hash bits} and the unit's hash (mates share a wave; the pair's hash mixes both
//                 in order), rows[r].length, and names a failed record.
//   dd_insert_k   16 lanes a unit.  Probes linearly from hash & (slots - 1); lane 0 claims an empty word by
//                 compare-and-swap with {hash tag, global unit index}.  On an occupied word the tag inside the word is
//                 compared first, then the lengths and hash bits of ref[], then the key bytes 16 a lane, ANDed over the
//                 row.  Everything read about an occupant is inside the word or was written by an earlier launch (ref[]
//                 and the text); nothing is stored beside the word after the CAS, no lane waits for another wave, and the
//                 probe loop ends after `slots` steps (a full table is a status bit, MK_ERR_STATE on the host).
//                 On the unit's slot: atomicMin(first), atomicAdd(copies), slot_of[unit] for the next kernel.
//   dd_decide_k   a lane a record, behind the piece's inserts: first[] is final for every unit up to the piece's end
//                 (earlier pieces hold lower indices).  keep, rows[r].first, the segments (whole records), the counts.
//   dd_levels_k   once a call: one pass over the slots, mk_histo's shape (LDS bins for the low levels).
#include "mk_fqpiece.h"
#include "mk_env.h"
#include <memory>
#include <string.h>

#define DD_EMPTY (~0ull)
#define DD_UNIT_BITS 40  // a word: the tag (the hash's top 24 bits) above the global unit index
#define DD_UNIT_MASK ((1ull << DD_UNIT_BITS) - 1)
#define DD_MUL MK_POLY_B  // M: odd
#define DD_WINDOW 1024    // levels a workgroup of dd_levels_k keeps in LDS

struct DdRef {  // one a record of the call, by global record number
  u64 off;      // of its key in the resident text
  unsigned len, hbits;
};
struct DdStatus {  // device memory, behind the FsStatus of the piece
  u64 bases_in, duplicates, probes, compares, full;
};
struct DdOpt {
  unsigned prefix, paired, which, high;
  u64 hmask;  // MK_DEDUP_HASH_BITS: the bits of every hash that are kept
};
struct DdStats : mk_fastq_dedup_t {  // (what fq_piece counts beside the caller's figures)
  uint64_t records_trimmed, full;
};

static constexpr u64 dd_pow_c(unsigned e) {
  u64 r = 1, s = DD_MUL;
  for (; e; e >>= 1, s *= s)
    if (e & 1) r *= s;
  return r;
}
static constexpr u64 DD_M256 = dd_pow_c(256);

// M^e for e in 0 .. 511.
__device__ __forceinline__ u64 dd_pow(unsigned e) {
  u64 r = 1, s = DD_MUL;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if ((e >> k) & 1u) r *= s;
    s *= s;
  }
  return r;
}
// The sum of a row of 16 lanes modulo 2^64, in every lane of it (row_ror; whole rows are active or idle together).
#define DD_ROR_ADD(v, ctrl)                                                                                  \
  v += ((u64)(unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((v) >> 32), ctrl, 0xf, 0xf, false) << 32) | \
       (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v), ctrl, 0xf, 0xf, false)
__device__ __forceinline__ u64 dd_row_sum(u64 v) {
  DD_ROR_ADD(v, 0x128);  // row_ror:8
  DD_ROR_ADD(v, 0x124);
  DD_ROR_ADD(v, 0x122);
  DD_ROR_ADD(v, 0x121);
  return v;
}
__device__ __forceinline__ u64 dd_rotl(u64 x, int s) { return (x << s) | (x >> (64 - s)); }

// uhash[u]: the hash of unit u of the piece (record u, or the pair (2u, 2u + 1)); first: the global number of the piece's
// record 0; base: the offset of the piece's text in the resident text.  The grid has a multiple of four rows, and pieces
// start at even records: mates sit in neighbouring rows of one wave.  Loads: QtLine's, aligned granules that hold a byte
// of the key, each inside [0, n) of the piece (fs_load reads a granule that the text ends in byte by byte).
static __global__ void __launch_bounds__(256) dd_key_k(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ line, size_t nrec,
                                                       DdOpt o, u64 first, u64 base, DdRef* __restrict__ ref, u64* __restrict__ uhash,
                                                       u64* __restrict__ rows, FsStatus* __restrict__ st, DdStatus* __restrict__ qs) {
  const unsigned j = threadIdx.x & 15u, row = (threadIdx.x >> 4) & 3u;
  const size_t per_grid = (size_t)gridDim.x * (256 / QT_GROUP);
  u64 bases = 0;
  for (size_t r4 = (size_t)blockIdx.x * (256 / QT_GROUP) + ((threadIdx.x >> 6) << 2); r4 < nrec; r4 += per_grid) {
    const size_t r = r4 + row;
    u64 h = 0;
    if (r < nrec) {
      const QtRecord rec = qt_record(text, line, r);
      if (rec.fail >= 0 && j == 0) atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | (unsigned)rec.fail));
      const u64 L = rec.ls, K = (o.prefix && o.prefix < L) ? o.prefix : L;
      const QtLine sl{rec.l1, K};
      const unsigned np = sl.passes();
      const u64 lane_pow = dd_pow(16u * j + 16u - (unsigned)(rec.l1 & 15));  // M^(i0 + 16) of pass 0: exponent 1 .. 256
      u64 sum = 0, pass_pow = 1;
      for (unsigned p = 0; p < np; ++p) {
        const FsSeg c = sl.load(text, n, p, j);
        const long long i0 = sl.i0(p, j);
        u64 acc = 0;
#pragma unroll
        for (int b = 15; b >= 0; --b) acc = acc * DD_MUL + ((u64)(i0 + b) < K ? (u64)QT_BYTE(c, b) : 0ull);
        sum += pass_pow * lane_pow * acc;
        pass_pow *= DD_M256;
      }
      sum = dd_row_sum(sum);
      h = mk_mix64(sum ^ (K * 0xD6E8FEB86659FD93ull)) & o.hmask;
      if (j == 0) {
        DdRef x;
        x.off = base + rec.l1;
        x.len = (unsigned)K;
        x.hbits = (unsigned)h;
        ref[first + r] = x;
        rows[2 * r] = L;
        bases += L;
      }
    }
    if (o.paired) {  // (the row beside this one; a record behind the last has h = 0)
      const u64 mate = (u64)__shfl_xor((unsigned long long)h, 16);
      h = mk_mix64(h * 0x9FB21C651E98DF25ull + dd_rotl(mate, 29)) & o.hmask;
      if (j == 0 && r < nrec && !(r & 1)) uhash[r >> 1] = h;
    } else if (j == 0 && r < nrec) {
      uhash[r] = h;
    }
  }
  block_add(&qs->bases_in, bases);
}

// Whether the keys of x and y are the same bytes: lane j compares bytes [16 j + 256 t, + 16) of them (fl_load16: any
// address, nothing read behind text_n), the row ANDs.  Row-uniform arguments, whole rows call it.
__device__ __forceinline__ bool dd_equal(const uint8_t* __restrict__ text, u64 text_n, const DdRef x, const DdRef y, unsigned j, unsigned row,
                                         u64& compares) {
  if (x.len != y.len || x.hbits != y.hbits) return false;
  compares += x.len;
  bool differ = false;
  for (u64 i = 16ull * j; i < x.len; i += QT_PASS) {
    const u64 left = x.len - i;
    unsigned __int128 d = fl_load16(text, text_n, x.off + i) ^ fl_load16(text, text_n, y.off + i);
    if (left < 16) d &= (((unsigned __int128)1) << (8 * left)) - 1;
    differ |= d != 0;
  }
  return ((unsigned)(__ballot(differ) >> (16 * row)) & 0xFFFFu) == 0;
}

// Unit u of the piece is unit ufirst + u of the call; per: records a unit (1, or 2 with paired).  word[] and first[] were
// set to all ones and copies[] to 0 before the call's first piece; ref[] of every unit up to this piece's end and the text
// come from earlier launches.
static __global__ void __launch_bounds__(256) dd_insert_k(const uint8_t* __restrict__ text, u64 text_n, const DdRef* __restrict__ ref,
                                                          const u64* __restrict__ uhash, size_t nunits, u64 ufirst, unsigned per,
                                                          u64* __restrict__ word, u64* __restrict__ firstv, u64* __restrict__ copies,
                                                          u64 slots, u64* __restrict__ slot_of, DdStatus* __restrict__ qs) {
  const unsigned j = threadIdx.x & 15u, row = (threadIdx.x >> 4) & 3u;
  const size_t per_grid = (size_t)gridDim.x * (256 / QT_GROUP);
  u64 probes = 0, compares = 0, full = 0;
  for (size_t u4 = (size_t)blockIdx.x * (256 / QT_GROUP) + ((threadIdx.x >> 6) << 2); u4 < nunits; u4 += per_grid) {
    const size_t u = u4 + row;
    if (u >= nunits) continue;
    const u64 g = ufirst + u, h = uhash[u], tag = h >> DD_UNIT_BITS, mine = (tag << DD_UNIT_BITS) | g;
    const DdRef a0 = ref[g * per], a1 = ref[g * per + (per - 1)];
    u64 slot = h & (slots - 1), found = DD_EMPTY;
    for (u64 step = 0; step < slots; ++step) {
      u64 w = 0;
      if (j == 0) {
        w = __hip_atomic_load(&word[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == DD_EMPTY) {
          w = atomicCAS((unsigned long long*)&word[slot], (unsigned long long)DD_EMPTY, (unsigned long long)mine);
          if (w == DD_EMPTY) w = mine;
        }
      }
      w = (u64)__shfl((unsigned long long)w, (int)(16 * row), 64);
      bool same = w == mine;
      if (!same && (w >> DD_UNIT_BITS) == tag) {
        const u64 occ = w & DD_UNIT_MASK;
        same = dd_equal(text, text_n, ref[occ * per], a0, j, row, compares);
        if (same && per == 2) same = dd_equal(text, text_n, ref[occ * per + 1], a1, j, row, compares);
      }
      if (same) {
        found = slot;
        break;
      }
      ++probes;
      slot = (slot + 1) & (slots - 1);
    }
    if (j == 0) {
      if (found != DD_EMPTY) {
        atomicMin((unsigned long long*)&firstv[found], (unsigned long long)g);
        atomicAdd((unsigned long long*)&copies[found], 1ull);
      } else {
        full = 1;
      }
      slot_of[u] = found != DD_EMPTY ? found : 0;
    }
  }
  block_add(&qs->probes, j == 0 ? probes : 0);
  block_add(&qs->compares, j == 0 ? compares : 0);
  block_add(&qs->full, j == 0 ? full : 0);
}

// A lane per record (and one for the slot behind the last segment).  Record r is lines 4r .. 4r + 3; its segments are
// 4r .. 4r + 3, of which a whole record uses the first.
static __global__ void __launch_bounds__(256) dd_decide_k(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t nrec, DdOpt o,
                                                          u64 first, const u64* __restrict__ slot_of, const u64* __restrict__ firstv,
                                                          u64* __restrict__ rows, uint8_t* __restrict__ keep, u64* __restrict__ seg_src,
                                                          u64* __restrict__ len, FsStatus* __restrict__ st, DdStatus* __restrict__ qs) {
  u64 n_out = 0, n_bases = 0, n_dup = 0;
  mk_for_each(nrec + 1, [&](size_t r) {
    if (r == nrec) {
      seg_src[4 * nrec] = 0;
      len[4 * nrec] = 0;
      return;
    }
    const QtRecord q = qt_record(text, line, r);
    const u64 fu = firstv[slot_of[o.paired ? r >> 1 : r]];
    const u64 fr = o.paired ? 2 * fu + (r & 1) : fu;
    const bool k = fr == first + r;
    keep[r] = k ? 1 : 0;
    rows[2 * r + 1] = fr;
    n_dup += k ? 0 : 1;
    const u64 L = rows[2 * r];
    u64 s[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    if (q.fail < 0 && (k ? 1u : 2u) == o.which) {
      fq_segments(q, L, 0, L, s, m);
      n_out += 1;
      n_bases += L;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      seg_src[4 * r + i] = s[i];
      len[4 * r + i] = m[i];
    }
  });
  block_add(&st->records_out, n_out);
  block_add(&st->bases_out, n_bases);
  block_add(&qs->duplicates, n_dup);
}

// levels (or nullptr) and out[0] = clusters, out[1] = the largest: mk_histo's pass over a table.
static __global__ void __launch_bounds__(256) dd_levels_k(const u64* __restrict__ word, const u64* __restrict__ copies, size_t slots, u64 high,
                                                          u64* __restrict__ levels, u64* __restrict__ out) {
  __shared__ unsigned s_bins[DD_WINDOW];
  __shared__ unsigned long long s_top;
  for (unsigned b = threadIdx.x; b < DD_WINDOW; b += 256) s_bins[b] = 0;
  if (threadIdx.x == 0) s_top = 0;
  __syncthreads();
  u64 clusters = 0, top = 0;
  mk_for_each(slots, [&](size_t i) {
    if (word[i] == DD_EMPTY) return;
    const u64 c = copies[i], bin = c > high ? high + 1 : c;
    clusters += 1;
    top = c > top ? c : top;
    if (bin < DD_WINDOW) atomicAdd(&s_bins[bin], 1u);
    else if (levels) atomicAdd((unsigned long long*)&levels[bin], 1ull);
  });
  for (int d = 32; d > 0; d >>= 1) {
    const u64 other = __shfl_down((unsigned long long)top, d);
    top = other > top ? other : top;
  }
  if ((threadIdx.x & 63) == 0 && top) atomicMax(&s_top, (unsigned long long)top);
  block_add(&out[0], clusters);  // (its barriers order s_top and s_bins too)
  if (threadIdx.x == 0 && s_top) atomicMax((unsigned long long*)&out[1], s_top);
  if (levels)  // (a bin that is not zero is min(copies, high + 1) of a slot: within levels[])
    for (unsigned b = threadIdx.x; b < DD_WINDOW; b += 256)
      if (s_bins[b]) atomicAdd((unsigned long long*)&levels[b], (unsigned long long)s_bins[b]);
}

// ------------------------------------------------------------------------------------------ host side
// The state of a call: the resident text, ref[], the table, and per piece the units' hashes and slots.
struct DdSide {
  MkDevBuf res, refs, table, unit, lev;
  const uint8_t* text = nullptr;  // the resident text: res.p (text call), or the one piece where it stands (device call)
  u64 text_n = 0;
  size_t expect = 0;       // records the call will see at most (text call: from the host's line count)
  size_t cap_records = 0;  // records ref[] has room for; 0: nothing is set up yet
  u64 slots = 0;
  u64 *word = nullptr, *first = nullptr, *copies = nullptr, *d_levels = nullptr, *d_out = nullptr;
  std::unique_ptr<MkTimed> key, insert;
  bool timed = false;
  int rc = MK_OK;
  ~DdSide() {
    for (MkDevBuf* b : {&res, &refs, &table, &unit, &lev}) buf_free(*b);
  }
};

struct DdPolicy {
  typedef DdOpt Opt;
  typedef DdStatus Status;
  typedef DdStats Stats;
  typedef DdSide Side;
  static constexpr size_t ROW = 2;
  static bool paired(const DdOpt& o) { return o.paired != 0; }
  static const char* kind(unsigned k) { return fs_kind(k); }
  // ref[] and the table, once, sized by the records the call will hold (at most half the slots used); per piece the
  // units' hashes and slots.
  static int ready(FqCall<DdPolicy>& f, const uint8_t* d_text, size_t n, size_t nrec) {
    mk_ctx* c = f.c;
    DdSide& s = f.side;
    int rc;
    if (f.device) {
      s.text = d_text;
      s.text_n = n;
    }
    if (!s.cap_records) {
      const auto t0 = MkClock::now();
      const size_t records = std::max(s.expect, f.records);
      const size_t units = f.o.paired ? (records + 1) / 2 : records;
      if (units > DD_UNIT_MASK) { c->err = std::string(f.what) + ": more than 2^40 - 1 units"; return MK_ERR_RANGE; }
      s.slots = pow2_at_least(2 * units);
      if ((rc = mk_buf_reserve(c, s.refs, (records + 2) * sizeof(DdRef))) != MK_OK) return rc;
      if ((rc = mk_buf_reserve(c, s.table, 3 * (size_t)s.slots * sizeof(u64))) != MK_OK) return rc;
      s.word = (u64*)s.table.p;
      s.first = s.word + s.slots;
      s.copies = s.first + s.slots;
      MK_HIP(hipMemsetAsync(s.refs.p, 0, (records + 2) * sizeof(DdRef), c->stream));
      MK_HIP(hipMemsetAsync(s.word, 0xFF, 2 * (size_t)s.slots * sizeof(u64), c->stream));
      MK_HIP(hipMemsetAsync(s.copies, 0, (size_t)s.slots * sizeof(u64), c->stream));
      s.cap_records = records;
      f.st.slots = s.slots;
      f.st.s_plan += mk_since(t0);
    }
    if (f.records > s.cap_records) {
      c->err = std::string(f.what) + ": the text holds more records than its lines were counted for (internal error)";
      return MK_ERR_STATE;
    }
    return mk_buf_reserve(c, s.unit, 2 * nrec * sizeof(u64));
  }
  static void scan(FqCall<DdPolicy>& f, const uint8_t* d_text, size_t n, const u64* line, size_t nrec, u64* d_rows, uint8_t*, FsStatus* d_st) {
    DdSide& s = f.side;
    hipStream_t q = f.c->stream;
    DdStatus* d_qs = (DdStatus*)(d_st + 1);  // (fq_piece's layout: the Status behind the FsStatus)
    const size_t first = f.records - nrec, per = f.o.paired ? 2 : 1, nunits = (nrec + per - 1) / per;
    u64* uhash = (u64*)s.unit.p;
    u64* slot_of = uhash + nrec;
    if (s.rc == MK_OK) s.rc = s.key->begin();
    hipLaunchKernelGGL(dd_key_k, dim3(grid_for(nrec, 256 / QT_GROUP, 1u << 16)), dim3(256), 0, q, d_text, (u64)n, line, nrec, f.o, (u64)first,
                       (u64)(d_text - s.text), (DdRef*)s.refs.p, uhash, d_rows, d_st, d_qs);
    if (s.rc == MK_OK) s.rc = s.key->end();
    if (s.rc == MK_OK) s.rc = s.insert->begin();
    hipLaunchKernelGGL(dd_insert_k, dim3(grid_for(nunits, 256 / QT_GROUP, 1u << 16)), dim3(256), 0, q, s.text, s.text_n, (const DdRef*)s.refs.p,
                       (const u64*)uhash, nunits, (u64)(first / per), (unsigned)per, s.word, s.first, s.copies, s.slots, slot_of, d_qs);
    if (s.rc == MK_OK) s.rc = s.insert->end();
    s.timed = true;
  }
  static void decide(FqCall<DdPolicy>& f, const uint8_t* d_text, const u64* line, size_t nrec, const u64* d_rows, const uint8_t*,
                     uint8_t* d_keep, u64* seg_src, u64* len, FsStatus* d_st, DdStatus* d_qs) {
    const DdSide& s = f.side;
    // (rows[r].first is written here, behind the inserts: the piece loop hands the rows on as what the scan left)
    hipLaunchKernelGGL(dd_decide_k, dim3(grid_for(nrec + 1, 256, 4096)), dim3(256), 0, f.c->stream, d_text, line, nrec, f.o,
                       (u64)(f.records - nrec), (const u64*)((u64*)s.unit.p + nrec), (const u64*)s.first, const_cast<u64*>(d_rows), d_keep,
                       seg_src, len, d_st, d_qs);
  }
  static void add(DdStats& st, const DdStatus& q) {
    st.bases_in += q.bases_in;
    st.duplicates += q.duplicates;
    st.probes += q.probes;
    st.compares += q.compares;
    st.full += q.full;
  }
};
typedef FqCall<DdPolicy> DdCall;

// What follows every piece (the stream is idle): the two halves of s_scan, and the status bit of a table found full.
static int dd_after_piece(DdCall& f) {
  mk_ctx* c = f.c;
  DdSide& s = f.side;
  if (s.rc != MK_OK) return s.rc;
  if (s.timed) {
    int rc;
    if ((rc = s.key->add_to(f.st.s_key)) != MK_OK || (rc = s.insert->add_to(f.st.s_insert)) != MK_OK) return rc;
    s.timed = false;
  }
  if (f.st.full) { c->err = std::string(f.what) + ": the table of the call is full (internal error)"; return MK_ERR_STATE; }
  return MK_OK;
}

// The options as the kernels take them, or the message of the first one out of range.
static const char* dd_options(const mk_dedup_opt_t* opt, DdOpt& o) {
  if (!opt) return "opt is NULL";
  if (opt->paired > 1) return "paired must be 0 or 1";
  if (opt->which != 1 && opt->which != 2) return "which must be 1 (the uniques) or 2 (the duplicates)";
  if (opt->high < 1 || opt->high > MK_DEDUP_MAX_HIGH) return "high must lie in 1 .. 2^20";
  o.prefix = opt->prefix;
  o.paired = opt->paired;
  o.which = opt->which;
  o.high = opt->high;
  const long long b = mk_env_int("MK_DEDUP_HASH_BITS", 64);
  o.hmask = b >= 64 ? ~0ull : b <= 0 ? 0ull : (1ull << b) - 1;
  return nullptr;
}

// fq_run with the levels zeroed before the pieces and made, with distinct and max_copies, behind them; for the text
// call copied to h_levels (host memory).  The caller's figures are st's on success and on a short out.
template <class Body>
static int dd_run(DdCall& f, u64* h_levels, size_t* out_len, size_t* nrec, mk_fastq_dedup_t* st, Body&& body) {
  mk_ctx* c = f.c;
  DdSide& s = f.side;
  const size_t words = (size_t)f.o.high + 2;
  DdStats got{};
  const int rc = fq_run(
      f, out_len, nrec, &got,
      [&]() -> int {
        s.key.reset(new MkTimed(c));
        s.insert.reset(new MkTimed(c));
        int r = mk_buf_reserve(c, s.lev, (2 + (s.d_levels ? 0 : words)) * sizeof(u64));
        if (r != MK_OK) return r;
        s.d_out = (u64*)s.lev.p;
        const bool own = !s.d_levels;
        if (own) s.d_levels = s.d_out + 2;
        MK_HIP(hipMemsetAsync(s.d_out, 0, (2 + (own ? words : 0)) * sizeof(u64), c->stream));
        if (!own) MK_HIP(hipMemsetAsync(s.d_levels, 0, words * sizeof(u64), c->stream));
        return MK_OK;
      },
      body,
      [&]() -> int {
        u64 h[2] = {0, 0};
        if (s.cap_records) {
          MkTimed levels(c);
          int r;
          if ((r = levels.begin()) != MK_OK) return r;
          hipLaunchKernelGGL(dd_levels_k, dim3(grid_for((size_t)s.slots, 256, 2048)), dim3(256), 0, c->stream, (const u64*)s.word,
                             (const u64*)s.copies, (size_t)s.slots, (u64)f.o.high, s.d_levels, s.d_out);
          MK_HIP(hipGetLastError());
          if ((r = levels.end()) != MK_OK) return r;
          MK_HIP(hipMemcpyAsync(h, s.d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
          MK_HIP(hipStreamSynchronize(c->stream));
          if ((r = levels.add_to(f.st.s_levels)) != MK_OK) return r;
        }
        f.st.distinct = h[0];
        f.st.max_copies = h[1];
        if (h_levels) {
          const auto t1 = MkClock::now();
          MK_HIP(hipMemcpyAsync(h_levels, s.d_levels, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
          MK_HIP(hipStreamSynchronize(c->stream));
          f.st.s_write += mk_since(t1);
        }
        return MK_OK;
      });
  if (st && (rc == MK_OK || (rc == MK_ERR_RANGE && *out_len))) *st = got;
  return rc;
}

extern "C" int mk_fastq_dedup_device(mk_ctx* c, const uint8_t* d_fastq, size_t n, const mk_dedup_opt_t* opt, size_t cap, uint8_t* d_keep,
                                     uint64_t* d_rows, uint64_t* d_levels, uint8_t* d_out, size_t out_cap, size_t* out_len, size_t* nrec,
                                     mk_fastq_dedup_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_fastq) || (out_cap && !d_out)) { c->err = "mk_fastq_dedup_device: NULL buffer"; return MK_ERR_ARG; }
  // (DdRef holds a 32-bit key length)
  if (n > 0xFFFFFFFFull) { c->err = "mk_fastq_dedup_device: the text is one piece, which holds at most 2^32 - 1 bytes"; return MK_ERR_RANGE; }
  if (((uintptr_t)d_rows | (uintptr_t)d_levels) & 7) { c->err = "mk_fastq_dedup_device: d_rows and d_levels must be aligned to 8"; return MK_ERR_ARG; }
  DdOpt o{};
  if (const char* msg = dd_options(opt, o)) { c->err = std::string("mk_fastq_dedup_device: ") + msg; return MK_ERR_ARG; }
  DdCall f(c, "mk_fastq_dedup_device", o, (d_keep || d_rows) ? cap : ~(size_t)0, d_keep, (u64*)d_rows, d_out, out_cap, true);
  f.side.d_levels = (u64*)d_levels;
  return dd_run(f, nullptr, out_len, nrec, st, [&]() -> int {
    // (the table is sized by the line count of the one piece: DdPolicy::ready)
    const int rc = fq_device_body(f, d_fastq, n);
    return rc != MK_OK ? rc : dd_after_piece(f);
  });
}

extern "C" int mk_fastq_dedup_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const mk_dedup_opt_t* opt, size_t cap,
                                   uint8_t* keep, uint64_t* rows, uint64_t* levels, uint8_t* out, size_t out_cap, size_t* out_len, size_t* nrec,
                                   mk_fastq_dedup_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_fastq_dedup_text: NULL buffer"; return MK_ERR_ARG; }
  DdOpt o{};
  if (const char* msg = dd_options(opt, o)) { c->err = std::string("mk_fastq_dedup_text: ") + msg; return MK_ERR_ARG; }
  if (levels) memset(levels, 0, ((size_t)o.high + 2) * sizeof(uint64_t));
  DdCall f(c, "mk_fastq_dedup_text", o, (keep || rows) ? cap : ~(size_t)0, keep, (u64*)rows, out, out_cap, false);
  return dd_run(f, (u64*)levels, out_len, nrec, st, [&]() -> int {
    if (!n) return MK_OK;
    DdSide& s = f.side;
    // the pieces of fq_text_body, and beside the pass that cuts them the line count that sizes ref[] and the table
    const auto t0 = MkClock::now();
    std::vector<uint64_t> cuts;
    int rc = fs_piece_cuts(c, f.what, fastq, n, piece_bytes, o.paired, cuts);
    if (rc != MK_OK) return rc;
    size_t newlines = 0;  // (a memchr walk: 33 ms for 314 MB where std::count, which this build does not vectorise, took 79)
    for (const uint8_t *p = fastq, *end = fastq + n; (p = (const uint8_t*)memchr(p, '\n', (size_t)(end - p))) != nullptr; ++p) ++newlines;
    s.expect = (newlines + (fastq[n - 1] != '\n' ? 1 : 0)) / 4;
    // every piece at an offset aligned to 16 of one buffer (the line kernels load aligned granules), 64 bytes of slack
    const size_t res_bytes = n + 16 * cuts.size() + 64;
    f.st.s_plan += mk_since(t0);
    if ((rc = mk_buf_reserve(c, s.res, res_bytes)) != MK_OK) {
      if (rc == MK_ERR_NOMEM) c->err = "mk_fastq_dedup_text: the resident text (" + std::to_string(res_bytes) + " bytes): " + c->err;
      return rc;
    }
    s.text = (const uint8_t*)s.res.p;
    s.text_n = res_bytes;
    size_t from = 0, at = 0;
    for (const uint64_t end : cuts) {
      const size_t len = (size_t)end - from;
      if (!len) continue;
      if (len > 0xFFFFFFFFull) { c->err = "mk_fastq_dedup_text: a piece holds at most 2^32 - 1 bytes"; return MK_ERR_RANGE; }
      const auto t1 = MkClock::now();
      MK_HIP(hipMemcpyAsync((uint8_t*)s.res.p + at, fastq + from, len, hipMemcpyHostToDevice, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      f.st.s_copy += mk_since(t1);
      if ((rc = fq_piece(f, s.text + at, len)) != MK_OK) return rc;
      if ((rc = dd_after_piece(f)) != MK_OK) return rc;
      from = (size_t)end;
      at = (at + len + 15) & ~(size_t)15;
    }
    return MK_OK;
  });
}
