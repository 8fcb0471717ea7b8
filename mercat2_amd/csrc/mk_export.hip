// mk_export.hip -- a context's running tables as sorted rows: mk_export*, mk_write_tsv and its two writers, the exports of
// one table spread over several contexts, and the device-side / text-row exports the multi-GPU merge moves rows with.
// Host code only.
//
// Export == sorted(kmers.items()) + the TSV print loop (bin/mercat2.py:128-137).
#include "mk_common.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

typedef unsigned long long u64;
using Clk = std::chrono::steady_clock;
static double since(Clk::time_point t) { return std::chrono::duration<double>(Clk::now() - t).count(); }

// --------------------------------------------------------------------------------- gather
static int gather_packed(mk_ctx* c, ExportView& v, u64* d_keys_out, u64* d_cnts_out, size_t cap, size_t* rows_out,
                         bool to_host) {
  int rc;
  size_t rows = 0;
  const auto t_gather = Clk::now();
  if (c->mode == MK_MODE_DENSE) {
    const size_t nbins = c->run_slots;
    std::vector<u64> bins(nbins);
    MK_HIP(hipMemcpyAsync(bins.data(), c->run.p, nbins * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nbins; ++i)
      if (bins[i]) { v.pkeys.push_back(i); v.pcnts.push_back(bins[i]); }
    rows = v.pkeys.size();
    if (!to_host) {
      if (rows > cap) { c->err = "export: device buffers too small"; return MK_ERR_RANGE; }
      if (rows) {
        MK_HIP(hipMemcpyAsync(d_keys_out, v.pkeys.data(), rows * 8, hipMemcpyHostToDevice, c->stream));
        MK_HIP(hipMemcpyAsync(d_cnts_out, v.pcnts.data(), rows * 8, hipMemcpyHostToDevice, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
      }
    }
  } else if (c->mode == MK_MODE_HASH64 || c->mode == MK_MODE_HASH128) {
    const bool two = c->mode == MK_MODE_HASH128;
    const size_t w = two ? 2 : 1;  // words per key
    v.words = (int)w;
    rows = two ? c->run128_rows : c->run_rows;
    const size_t side = !two && c->run_side ? 1 : 0;
    if (!to_host && rows + side > cap) { c->err = "export: device buffers too small"; return MK_ERR_RANGE; }
    if (rows) {
      u64* ok = d_keys_out;
      u64* oc = d_cnts_out;
      if (to_host) {  // sorted rows for the host: keys, then counts
        MkDevBuf& kb = two ? c->ex128_out : c->ex_keys2;
        if ((rc = mk_buf_reserve(c, kb, (two ? 3 : 1) * rows * 8 + 64)) != MK_OK) return rc;
        if (!two && (rc = mk_buf_reserve(c, c->ex_cnts2, rows * 8 + 64)) != MK_OK) return rc;
        ok = (u64*)kb.p;
        oc = two ? ok + 2 * rows : (u64*)c->ex_cnts2.p;
      }
      // one-word tables: rows binned by key prefix, the bins sorted in LDS (mk_binsort.hip); the others, and a table
      // with a bin too large for that, by the library sort
      bool binned = !two && mk_binsort_takes(rows) && mk_env_int("MK_EXPORT_LIBSORT", 0) == 0;
      u64 got[2] = {0, 0};  // rows found; bins the binned sort left alone
      auto t_sort = t_gather;
      for (;;) {
        const u64* d_got = nullptr;
        mk_prof_begin(c, MK_K_EXPORT);
        if (binned) {
          if ((rc = mk_binsort_export(c, (const MkSlot*)c->run.p, c->run_slots, rows, c->bits * c->k, (uint64_t*)ok, (uint64_t*)oc,
                                      (const uint64_t**)&d_got)) != MK_OK) return rc;
        } else {
          // compacted rows: one-word keys | counts; two-word hi | lo | count + 4 n words of sort scratch
          if ((rc = two ? mk_buf_reserve(c, c->ex128, 7 * rows * 8 + 64) : mk_buf_reserve(c, c->ex_keys, rows * 8 + 64)) != MK_OK) return rc;
          if (!two && (rc = mk_buf_reserve(c, c->ex_cnts, rows * 8 + 64)) != MK_OK) return rc;
          u64* k0 = (u64*)(two ? c->ex128.p : c->ex_keys.p);
          u64* cn = two ? k0 + 2 * rows : (u64*)c->ex_cnts.p;
          u64* d_cursor = (u64*)((char*)c->info.p + sizeof(MkChunkInfo));
          MK_HIP(hipMemsetAsync(d_cursor, 0, 8, c->stream));
          if ((rc = two ? mk_launch_compact128(c, (const MkSlot128*)c->run128.p, c->run128_slots, (uint64_t*)k0, (uint64_t*)(k0 + rows),
                                               (uint64_t*)cn, rows, (uint64_t*)d_cursor)
                        : mk_launch_compact(c, (const MkSlot*)c->run.p, c->run_slots, (uint64_t*)k0, (uint64_t*)cn, rows,
                                            (uint64_t*)d_cursor)) != MK_OK) return rc;
          if ((rc = two ? mk_sort_pairs128(c, (const uint64_t*)k0, (const uint64_t*)(k0 + rows), (const uint64_t*)cn, rows,
                                           2 * (c->k - 32), (uint64_t*)(cn + rows), (uint64_t*)ok, (uint64_t*)oc)
                        : mk_sort_pairs(c, (const uint64_t*)k0, (const uint64_t*)cn, (uint64_t*)ok, (uint64_t*)oc, rows,
                                        c->bits * c->k)) != MK_OK) return rc;
          d_got = d_cursor;
        }
        mk_prof_end(c);
        if (to_host) {
          MK_HIP(hipStreamSynchronize(c->stream));  // (so that sort and copy are timed apart: ~10 us)
          c->ex_st.s_sort += since(t_sort);
          v.pkeys.resize(w * rows);
          v.pcnts.resize(rows);
          MK_HIP(hipMemcpyAsync(v.pkeys.data(), ok, w * rows * 8, hipMemcpyDeviceToHost, c->stream));
          MK_HIP(hipMemcpyAsync(v.pcnts.data(), oc, rows * 8, hipMemcpyDeviceToHost, c->stream));
        }
        MK_HIP(hipMemcpyAsync(got, d_got, binned ? 16 : 8, hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
        if (!(binned && got[0] == rows && got[1])) break;
        binned = false;  // (keys crowded under one prefix: the whole export again)
        t_sort = Clk::now();
      }
      if (got[0] != rows) {
        c->err = std::string("export: ") + (two ? "two-word table" : "table") + " holds " + std::to_string(got[0]) + " rows, expected " + std::to_string(rows);
        return MK_ERR_STATE;
      }
    }
    if (side) {  // the all-ones key (32 x 'T'): the largest key, so it goes last
      if (to_host) { v.pkeys.push_back(MK_EMPTY); v.pcnts.push_back(c->run_side); }
      else {
        u64 kk = MK_EMPTY, cc = c->run_side;
        MK_HIP(hipMemcpyAsync(d_keys_out + rows, &kk, 8, hipMemcpyHostToDevice, c->stream));
        MK_HIP(hipMemcpyAsync(d_cnts_out + rows, &cc, 8, hipMemcpyHostToDevice, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
      }
      rows += 1;
    }
  }
  if (rows_out) *rows_out = rows;
  return MK_OK;
}

static int gather_ref(mk_ctx* c, ExportView& v, bool sorted) {
  const size_t rows = c->run_ref_rows;
  if (!rows) return MK_OK;
  int rc;
  const size_t k = (size_t)c->k;
  if ((rc = mk_buf_reserve(c, c->ex_keys, rows * 8 + 64)) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, c->ex_cnts, rows * 8 + 64)) != MK_OK) return rc;
  u64* d_cursor = (u64*)((char*)c->info.p + sizeof(MkChunkInfo));
  MK_HIP(hipMemsetAsync(d_cursor, 0, 16, c->stream));  // [0] rows compacted, [1] rows with a bad index
  if ((rc = mk_launch_compact(c, (const MkSlot*)c->run_ref.p, c->run_ref_slots, (uint64_t*)c->ex_keys.p,
                              (uint64_t*)c->ex_cnts.p, rows, (uint64_t*)d_cursor)) != MK_OK) return rc;
  // counts by arena row (the slots know their row), on the device
  if ((rc = mk_buf_reserve(c, c->surv_cnts, rows * 8 + 64)) != MK_OK) return rc;
  if ((rc = mk_launch_rows_by_slot(c, (const uint64_t*)c->ex_keys.p, (const uint64_t*)c->ex_cnts.p, rows,
                                   (uint64_t*)c->surv_cnts.p, (uint64_t*)d_cursor + 1)) != MK_OK) return rc;
  u64 got[2] = {0, 0};
  v.rstr.resize(rows * k);
  v.rcnt.resize(rows);
  v.rorder.resize(rows);
  for (size_t i = 0; i < rows; ++i) v.rorder[i] = i;
  if (sorted) {
    // rows in byte order: radix sort of the row indices, then the rows and counts gathered in that order
    // on the device, so that the host walks them front to back
    uint64_t* d_order = nullptr;
    if ((rc = mk_sort_rows(c, (const uint8_t*)c->arena.p, rows, c->k, &d_order)) != MK_OK) return rc;
    if ((rc = mk_buf_reserve(c, c->surv_keys, rows * k + 64)) != MK_OK) return rc;
    if ((rc = mk_launch_rows_gather(c, (const uint8_t*)c->arena.p, d_order, (const uint64_t*)c->surv_cnts.p, rows, c->k,
                                    (uint8_t*)c->surv_keys.p, (uint64_t*)c->ex_keys.p)) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(v.rstr.data(), c->surv_keys.p, rows * k, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipMemcpyAsync(v.rcnt.data(), c->ex_keys.p, rows * 8, hipMemcpyDeviceToHost, c->stream));
  } else {
    MK_HIP(hipMemcpyAsync(v.rstr.data(), c->arena.p, rows * k, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipMemcpyAsync(v.rcnt.data(), c->surv_cnts.p, rows * 8, hipMemcpyDeviceToHost, c->stream));
  }
  MK_HIP(hipMemcpyAsync(got, d_cursor, 16, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if (got[0] != rows || got[1] != 0) {
    c->err = "export: by-reference table holds " + std::to_string(got[0]) + " rows (" + std::to_string(got[1]) +
             " with a corrupt row index), expected " + std::to_string(rows);
    return MK_ERR_STATE;
  }
  return MK_OK;
}

static inline void decode_key(const mk_ctx* c, u64 key, uint8_t* out) {
  const int k = c->k;
  if (c->alphabet == MK_ALPHABET_NT2) {
    for (int j = k - 1; j >= 0; --j) { out[j] = "ACGT"[key & 3]; key >>= 2; }
  } else {
    for (int j = k - 1; j >= 0; --j) { out[j] = (uint8_t)('A' + (key & 31)); key >>= 5; }
  }
}

// packed row i of a view -> its k characters
void mk_decode_row(const mk_ctx* c, const ExportView& v, size_t i, uint8_t* out) {
  if (v.words == 1) { decode_key(c, v.pkeys[i], out); return; }
  const u64 hi = v.pkeys[2 * i], lo = v.pkeys[2 * i + 1];  // left-aligned: base j < 32 in hi, the rest in lo
  const int k = c->k;
  if (c->alphabet == MK_ALPHABET_AA5) {  // amino acids: the number sum(code_j * 32^(k-1-j)) in (hi, lo)
    unsigned __int128 x = ((unsigned __int128)hi << 64) | lo;
    for (int j = k - 1; j >= 0; --j) { out[j] = (uint8_t)('A' + (unsigned)(x & 31)); x >>= 5; }
    return;
  }
  for (int j = 0; j < 32; ++j) out[j] = "ACGT"[(hi >> (62 - 2 * j)) & 3];
  for (int j = 32; j < k; ++j) out[j] = "ACGT"[(lo >> (62 - 2 * (j - 32))) & 3];
}

// Visit every row in sorted(str) order: a 2-way merge of the packed rows (decoded on the fly)
// and the by-reference rows.
template <class F>
static void merged_rows(const mk_ctx* c, const ExportView& v, F&& f) {
  const size_t k = (size_t)c->k, np = v.packed_rows(), nr = v.rorder.size();
  std::vector<uint8_t> buf(k ? k : 1);
  size_t i = 0, j = 0;
  bool have = false;
  while (i < np || j < nr) {
    if (i < np && !have) { mk_decode_row(c, v, i, buf.data()); have = true; }
    bool take_packed;
    if (i >= np) take_packed = false;
    else if (j >= nr) take_packed = true;
    else take_packed = memcmp(buf.data(), v.rstr.data() + v.rorder[j] * k, k) < 0;
    if (take_packed) { f(buf.data(), v.pcnts[i]); ++i; have = false; }
    else { f(v.rstr.data() + v.rorder[j] * k, v.rcnt[v.rorder[j]]); ++j; }
  }
}

int mk_build_view(mk_ctx* c, ExportView& v) {
  MK_HIP(hipSetDevice(c->device));
  MK_SETTLE(c);
  const auto t0 = Clk::now();
  c->ex_st = mk_export_stats_t{};
  int rc = gather_packed(c, v, nullptr, nullptr, 0, nullptr, true);
  if (rc) return rc;
  rc = gather_ref(c, v, true);
  // (s_sort was added up inside; the rest of the gathering is the copies to the host)
  c->ex_st.s_d2h = since(t0) - c->ex_st.s_sort;
  c->ex_st.s_total = c->ex_st.s_sort + c->ex_st.s_d2h;
  c->ex_st.rows = v.packed_rows() + v.rorder.size();
  return rc;
}

extern "C" int mk_export_stats(mk_ctx* c, mk_export_stats_t* out) {
  if (!c || !out) return MK_ERR_ARG;
  *out = c->ex_st;
  return MK_OK;
}

extern "C" int mk_export_size(mk_ctx* c, size_t* rows) {
  if (!c || !rows) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_export_size");
  MK_SETTLE(c);
  if (c->mode == MK_MODE_DENSE) {
    ExportView v;
    MK_HIP(hipSetDevice(c->device));
    int rc = gather_packed(c, v, nullptr, nullptr, 0, nullptr, true);
    if (rc) return rc;
    *rows = v.packed_rows() + c->run_ref_rows;
  } else {
    *rows = mk_total_rows(c);
  }
  c->st.rows = *rows;
  return MK_OK;
}

extern "C" int mk_export(mk_ctx* c, uint8_t* kmers, uint64_t* counts, size_t rows_cap) {
  if (!c) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_export");
  ExportView v;
  int rc = mk_build_view(c, v);
  if (rc) return rc;
  const size_t rows = v.packed_rows() + v.rorder.size();
  if (rows > rows_cap) { c->err = "mk_export: rows_cap too small"; return MK_ERR_RANGE; }
  if (rows && (!kmers || !counts)) { c->err = "mk_export: NULL output"; return MK_ERR_ARG; }
  const size_t k = (size_t)c->k;
  size_t at = 0;
  const auto t_f = Clk::now();
  merged_rows(c, v, [&](const uint8_t* s, u64 n) {
    memcpy(kmers + at * k, s, k);
    counts[at] = n;
    ++at;
  });
  c->ex_st.s_format = since(t_f);
  c->ex_st.s_total += c->ex_st.s_format;
  return MK_OK;
}

// The table written from the device: compaction and sort as for any export, the rows formatted by a kernel (mk_tsv.hip),
// the text copied out through two pinned blocks while the one before is written to the file.  For tables whose rows are
// all packed keys (no rows kept as text: those are merged in on the host, write_view_tsv).
static int write_tsv_from_device(mk_ctx* c, const char* path, const char* basename, size_t* rows_out) {
  MK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = mk_settle(c)) != MK_OK) return rc;
  const auto t0 = Clk::now();
  c->ex_st = mk_export_stats_t{};
  const int words = c->mode == MK_MODE_HASH128 ? 2 : 1;
  size_t cap = 0;
  if (c->mode == MK_MODE_DENSE) cap = c->run_slots;
  else if (c->mode == MK_MODE_HASH64) cap = c->run_rows + 1;
  else cap = c->run128_rows;
  if (rows_out) *rows_out = 0;
  if (!cap) return MK_OK;
  MkDevBuf& kb = c->mode == MK_MODE_HASH128 ? c->ex128_out : c->ex_keys2;
  if ((rc = mk_buf_reserve(c, kb, (cap * (size_t)words + cap) * 8 + 64)) != MK_OK) return rc;  // keys, then counts
  u64* d_keys = (u64*)kb.p;
  u64* d_cnts = d_keys + cap * (size_t)words;
  ExportView v;
  size_t rows = 0;
  if ((rc = gather_packed(c, v, d_keys, d_cnts, cap, &rows, /*to_host=*/false)) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  c->ex_st.s_sort = since(t0);
  c->ex_st.rows = rows;
  if (rows_out) *rows_out = rows;
  if (!rows) return MK_OK;  // bin/mercat2.py:135-137: no file when nothing survives
  const auto t1 = Clk::now();
  // offsets and lengths: two scratch arrays of rows + 1 words (the compaction's buffers are free again)
  if ((rc = mk_buf_reserve(c, c->ex_keys, (rows + 1) * 8 + 64)) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, c->ex_cnts, (rows + 1) * 8 + 64)) != MK_OK) return rc;
  size_t text = 0;
  if ((rc = mk_launch_tsv_format(c, (const uint64_t*)d_keys, (const uint64_t*)d_cnts, rows, words, (uint64_t*)c->ex_keys.p,
                                 (uint64_t*)c->ex_cnts.p, &text)) != MK_OK) return rc;
  // two registered blocks, kept with the context
  const size_t piece = (size_t)8 << 20;
  if (c->tsv_pin_bytes < 2 * piece) {
    void* p = aligned_alloc(4096, 2 * piece);
    if (!p) { c->err = "mk_write_tsv: out of host memory"; return MK_ERR_NOMEM; }
    memset(p, 0, 2 * piece);  // (touched before it is pinned)
    const hipError_t he0 = hipHostRegister(p, 2 * piece, hipHostRegisterDefault);
    if (he0 != hipSuccess) { free(p); c->err = std::string("hipHostRegister: ") + hipGetErrorString(he0); return MK_ERR_HIP; }
    c->tsv_pin = p;
    c->tsv_pin_bytes = 2 * piece;
  }
  char* pin[2] = {(char*)c->tsv_pin, (char*)c->tsv_pin + piece};
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (auto& e : ev) MK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  FILE* f = fopen(path, "wb");
  if (!f) {
    for (auto& e : ev) (void)hipEventDestroy(e);
    c->err = std::string("mk_write_tsv: cannot open ") + path;
    return MK_ERR_IO;
  }
  setvbuf(f, nullptr, _IONBF, 0);  // (whole blocks: no second copy through stdio's buffer)
  const std::string head = std::string("k-mer\t") + basename + "_Count\n";
  double s_write = 0, s_wait = 0;
  auto timed_write = [&](const void* p, size_t n) {
    const auto tw = Clk::now();
    const size_t put = fwrite(p, 1, n, f);
    s_write += since(tw);
    return put == n;
  };
  bool ok = timed_write(head.data(), head.size());
  const size_t npieces = (text + piece - 1) / piece;
  hipError_t he = hipSuccess;
  for (size_t i = 0; i <= npieces && ok && he == hipSuccess; ++i) {
    if (i < npieces) {  // copy piece i out while piece i - 1 is written
      const size_t a = i * piece, n = std::min(piece, text - a);
      he = hipMemcpyAsync(pin[i & 1], (const char*)c->seq.p + a, n, hipMemcpyDeviceToHost, c->stream);
      if (he == hipSuccess) he = hipEventRecord(ev[i & 1], c->stream);
    }
    if (i > 0 && he == hipSuccess) {
      const size_t a = (i - 1) * piece, n = std::min(piece, text - a);
      const auto tw = Clk::now();
      he = hipEventSynchronize(ev[(i - 1) & 1]);
      s_wait += since(tw);
      if (he == hipSuccess) ok = timed_write(pin[(i - 1) & 1], n);
    }
  }
  (void)hipStreamSynchronize(c->stream);
  for (auto& e : ev) (void)hipEventDestroy(e);
  const auto tc = Clk::now();
  const bool bad_close = fclose(f) != 0;
  s_write += since(tc);
  const double all = since(t1);
  c->ex_st.bytes = head.size() + text;
  c->ex_st.s_write = s_write;
  c->ex_st.s_d2h = s_wait;
  c->ex_st.s_format = all - s_write - s_wait;  // (lengths, scan, fill kernel and what the loop itself costs)
  c->ex_st.s_total = since(t0);
  if (he != hipSuccess) { c->err = std::string("mk_write_tsv: copy of the text: ") + hipGetErrorString(he); return MK_ERR_HIP; }
  if (!ok || bad_close) { c->err = std::string("mk_write_tsv: write failed: ") + path; return MK_ERR_IO; }
  return MK_OK;
}

// The table written by the host: the packed rows decoded and merged with the rows kept as text.
static int write_view_tsv(mk_ctx* c, const ExportView& v, const char* path, const char* basename, size_t* rows_out) {
  const size_t rows = v.packed_rows() + v.rorder.size();
  if (rows_out) *rows_out = rows;
  if (!rows) return MK_OK;  // bin/mercat2.py:135-137: no file when nothing survives
  FILE* f = fopen(path, "wb");
  if (!f) { c->err = std::string("mk_write_tsv: cannot open ") + path; return MK_ERR_IO; }
  std::vector<char> out;
  out.reserve(1 << 22);
  const size_t k = (size_t)c->k;
  const auto t_f = Clk::now();
  double s_write = 0;
  uint64_t bytes = 0;
  auto flush = [&]() {
    if (!out.empty()) {
      const auto tw = Clk::now();
      fwrite(out.data(), 1, out.size(), f);
      s_write += since(tw);
      bytes += out.size();
      out.clear();
    }
  };
  const std::string head = std::string("k-mer\t") + basename + "_Count\n";
  out.insert(out.end(), head.begin(), head.end());
  merged_rows(c, v, [&](const uint8_t* s, u64 n) {
    out.insert(out.end(), (const char*)s, (const char*)s + k);
    out.push_back('\t');
    char num[24];
    int len = 0;
    do { num[len++] = (char)('0' + n % 10); n /= 10; } while (n);
    while (len) out.push_back(num[--len]);
    out.push_back('\n');
    if (out.size() > (1u << 22) - 4096 - k) flush();
  });
  flush();
  const bool bad = ferror(f) != 0;
  const auto tc = Clk::now();
  const bool bad_close = fclose(f) != 0;
  s_write += since(tc);
  c->ex_st.bytes = bytes;
  c->ex_st.s_write = s_write;
  c->ex_st.s_format = since(t_f) - s_write;
  c->ex_st.s_total += c->ex_st.s_format + s_write;
  if (bad_close || bad) { c->err = std::string("mk_write_tsv: write failed: ") + path; return MK_ERR_IO; }
  return MK_OK;
}

extern "C" int mk_write_tsv(mk_ctx* c, const char* path, const char* basename, size_t* rows_out) {
  if (!c || !path || !basename) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_write_tsv");
  MK_SETTLE(c);
  if (c->mode != MK_MODE_BYREF && c->run_ref_rows == 0 && c->bits != 0)
    return write_tsv_from_device(c, path, basename, rows_out);
  ExportView v;
  int rc = mk_build_view(c, v);
  if (rc) return rc;
  return write_view_tsv(c, v, path, basename, rows_out);
}

// ----------------------------------------------------- one table spread over several contexts by key range
// After mk_merge_devices(MK_MERGE_RANGES) context i holds the rows of key range i.  Every context sorts its own
// rows on its own GPU (one host thread each), the host concatenates the packed rows in context order and merges
// the few rows kept as text into them.
static int build_view_multi(mk_ctx* const* ctxs, int n, ExportView& all) {
  if (!ctxs || n < 1 || !ctxs[0]) return MK_ERR_ARG;
  for (int j_ = 0; j_ < n; ++j_) if (ctxs[j_] && ctxs[j_]->spoiled) { ctxs[0]->err = "multi export: a context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  mk_ctx* c0 = ctxs[0];
  for (int j = 0; j < n; ++j) {
    if (!ctxs[j]) { c0->err = "multi export: a context is NULL"; return MK_ERR_ARG; }
    if (ctxs[j]->k != c0->k || ctxs[j]->alphabet != c0->alphabet || ctxs[j]->mode != c0->mode) {
      c0->err = "multi export: contexts differ in alphabet or k";
      return MK_ERR_ARG;
    }
    if (ctxs[j]->in_chunk) { c0->err = "multi export: a chunk is open"; return MK_ERR_STATE; }
  }
  std::vector<ExportView> views((size_t)n);
  std::vector<int> rcs((size_t)n, MK_OK);
  {
    std::vector<std::thread> th;
    for (int j = 1; j < n; ++j) th.emplace_back([&, j] { rcs[j] = mk_build_view(ctxs[j], views[j]); });
    rcs[0] = mk_build_view(ctxs[0], views[0]);
    for (auto& t : th) t.join();
  }
  for (int j = 0; j < n; ++j)
    if (rcs[j]) { if (j) c0->err = ctxs[j]->err; return rcs[j]; }
  all.words = views[0].words;
  const size_t w = (size_t)all.words, k = (size_t)c0->k;
  size_t np = 0, nr = 0;
  for (auto& v : views) { np += v.packed_rows(); nr += v.rorder.size(); }
  all.pkeys.reserve(np * w);
  all.pcnts.reserve(np);
  for (int j = 0; j < n; ++j) {
    const ExportView& v = views[j];
    if (!v.packed_rows()) continue;
    if (!all.pcnts.empty()) {  // ranges ascending and disjoint: last key so far < first key of this context
      const u64* a = all.pkeys.data() + all.pkeys.size() - w;
      const u64* b = v.pkeys.data();
      const bool less = w == 1 ? a[0] < b[0] : (a[0] < b[0] || (a[0] == b[0] && a[1] < b[1]));
      if (!less) {
        c0->err = "multi export: context " + std::to_string(j) + " does not continue the key ranges of the contexts before it "
                  "(call mk_merge_devices with MK_MERGE_RANGES first)";
        return MK_ERR_STATE;
      }
    }
    all.pkeys.insert(all.pkeys.end(), v.pkeys.begin(), v.pkeys.end());
    all.pcnts.insert(all.pcnts.end(), v.pcnts.begin(), v.pcnts.end());
  }
  if (nr) {  // rows kept as text (after a merge they all sit in ctxs[0]; accept them anywhere): one sorted list
    all.rstr.reserve(nr * k);
    for (auto& v : views)
      for (size_t i = 0; i < v.rorder.size(); ++i) {
        all.rstr.insert(all.rstr.end(), v.rstr.begin() + v.rorder[i] * k, v.rstr.begin() + (v.rorder[i] + 1) * k);
        all.rcnt.push_back(v.rcnt[v.rorder[i]]);
      }
    all.rorder.resize(nr);
    for (size_t i = 0; i < nr; ++i) all.rorder[i] = i;
    std::sort(all.rorder.begin(), all.rorder.end(), [&](u64 x, u64 y) { return memcmp(all.rstr.data() + x * k, all.rstr.data() + y * k, k) < 0; });
    for (size_t i = 1; i < nr; ++i)
      if (memcmp(all.rstr.data() + all.rorder[i - 1] * k, all.rstr.data() + all.rorder[i] * k, k) == 0) {
        c0->err = "multi export: the same text row in two contexts (merge the contexts first)";
        return MK_ERR_STATE;
      }
  }
  return MK_OK;
}

extern "C" int mk_export_size_multi(mk_ctx* const* ctxs, int n, size_t* rows) {
  if (!ctxs || n < 1 || !rows) return MK_ERR_ARG;
  for (int j_ = 0; j_ < n; ++j_) if (ctxs[j_] && ctxs[j_]->spoiled) { if (ctxs[0]) ctxs[0]->err = "mk_export_size_multi: a context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  size_t total = 0;
  for (int j = 0; j < n; ++j) {
    size_t r = 0;
    int rc = mk_export_size(ctxs[j], &r);
    if (rc) { if (j && ctxs[0] && ctxs[j]) ctxs[0]->err = ctxs[j]->err; return rc; }
    total += r;
  }
  *rows = total;
  return MK_OK;
}

extern "C" int mk_export_multi(mk_ctx* const* ctxs, int n, uint8_t* kmers, uint64_t* counts, size_t rows_cap) {
  ExportView v;
  int rc = build_view_multi(ctxs, n, v);
  if (rc) return rc;
  mk_ctx* c = ctxs[0];
  const size_t rows = v.packed_rows() + v.rorder.size();
  if (rows > rows_cap) { c->err = "mk_export_multi: rows_cap too small"; return MK_ERR_RANGE; }
  if (rows && (!kmers || !counts)) { c->err = "mk_export_multi: NULL output"; return MK_ERR_ARG; }
  const size_t k = (size_t)c->k;
  size_t at = 0;
  merged_rows(c, v, [&](const uint8_t* s, u64 cnt) {
    memcpy(kmers + at * k, s, k);
    counts[at] = cnt;
    ++at;
  });
  return MK_OK;
}

extern "C" int mk_write_tsv_multi(mk_ctx* const* ctxs, int n, const char* path, const char* basename, size_t* rows_out) {
  if (!path || !basename) return MK_ERR_ARG;
  ExportView v;
  int rc = build_view_multi(ctxs, n, v);
  if (rc) return rc;
  return write_view_tsv(ctxs[0], v, path, basename, rows_out);
}

// ------------------------------------------------------------------- multi-GPU plumbing
// (what comes back in: mk_import_pairs_device / mk_import_exotic, mk_tableops.hip)
extern "C" int mk_export_pairs_device(mk_ctx* c, uint64_t* d_keys, uint64_t* d_counts, size_t cap, size_t* rows) {
  if (!c || !rows) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_export_pairs_device");
  MK_SETTLE(c);
  if (c->mode == MK_MODE_BYREF) { *rows = 0; return MK_OK; }  // rows travel as text (mk_export_exotic)
  MK_HIP(hipSetDevice(c->device));
  ExportView v;
  return gather_packed(c, v, (u64*)d_keys, (u64*)d_counts, cap, rows, false);
}

extern "C" int mk_export_exotic(mk_ctx* c, uint8_t* kmers, uint64_t* counts, size_t cap, size_t* rows) {
  if (!c || !rows) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_export_exotic");
  MK_HIP(hipSetDevice(c->device));
  MK_SETTLE(c);
  ExportView v;
  int rc = gather_ref(c, v, true);
  if (rc) return rc;
  *rows = v.rorder.size();
  if (!kmers && !counts) return MK_OK;  // size query
  if (*rows > cap) { c->err = "mk_export_exotic: cap too small"; return MK_ERR_RANGE; }
  const size_t k = (size_t)c->k;
  for (size_t i = 0; i < v.rorder.size(); ++i) {
    memcpy(kmers + i * k, v.rstr.data() + v.rorder[i] * k, k);
    counts[i] = v.rcnt[v.rorder[i]];
  }
  return MK_OK;
}
