// mk_combine.hip -- the combined table of several samples (one context each): mk_merged_export and the
// mk_write_merged_tsv* writers.  Host code only; every sample's sorted rows come from mk_build_view (mk_export.hip).
#include "mk_common.h"
#include <cstdio>
#include <cstring>

typedef unsigned long long u64;

// ------------------------------------------------------------- combined table of several samples
// merge_tsv (lib/mercat2_report.py:98-156) from the tables themselves: a k-way merge of the samples'
// sorted rows (each: device radix sort of the packed keys + by-reference rows, as for mk_export).
namespace {
struct RowIter {  // the rows of one sample in sorted(str) order
  const mk_ctx* c;
  const ExportView* v;
  size_t i = 0, j = 0;
  std::vector<uint8_t> buf;
  const uint8_t* cur = nullptr;
  u64 cnt = 0;
  RowIter(const mk_ctx* c_, const ExportView* v_) : c(c_), v(v_), buf((size_t)c_->k + 1) {}
  bool next() {
    const size_t k = (size_t)c->k, np = v->packed_rows(), nr = v->rorder.size();
    if (i >= np && j >= nr) { cur = nullptr; return false; }
    bool take_packed;
    if (i < np) mk_decode_row(c, *v, i, buf.data());
    if (i >= np) take_packed = false;
    else if (j >= nr) take_packed = true;
    else take_packed = memcmp(buf.data(), v->rstr.data() + v->rorder[j] * k, k) < 0;
    if (take_packed) { cur = buf.data(); cnt = v->pcnts[i]; ++i; }
    else { cur = v->rstr.data() + v->rorder[j] * k; cnt = v->rcnt[v->rorder[j]]; ++j; }
    return true;
  }
};

// f(kmer, counts[n]) for every k-mer present in any sample, in sorted order; absent = 0.
// as_reference: the rows exactly as merge_tsv's streaming loop produces them (lib/mercat2_report.py:128-152).  That
// loop picks the next k-mer only among the samples that ADVANCED in the current step (:131, :149-150) and, for a
// sample whose current key is not greater than the k-mer being written, writes that sample's count whatever its
// key is (:137-140).  So a key held only by samples that did not advance is never written as a row of its own: its
// count lands in a later row.  With as_reference the same rows come out (tables that share nearly all their keys --
// k = 5 on genomes -- are not affected); without it the table is the true union.
template <class F>
int merged_samples(mk_ctx* const* ctxs, int n, F&& f, bool as_reference = false) {
  if (!ctxs || n < 1 || !ctxs[0]) return MK_ERR_ARG;
  mk_ctx* c0 = ctxs[0];
  for (int s = 0; s < n; ++s) {
    if (!ctxs[s]) { c0->err = "merged table: a context is NULL"; return MK_ERR_ARG; }
    if (ctxs[s]->k != c0->k) { c0->err = "merged table: contexts differ in k"; return MK_ERR_ARG; }
    if (ctxs[s]->in_chunk) { c0->err = "merged table: a chunk is open"; return MK_ERR_STATE; }
  }
  std::vector<ExportView> views((size_t)n);
  std::vector<RowIter> it;
  it.reserve((size_t)n);
  for (int s = 0; s < n; ++s) {
    int rc = mk_build_view(ctxs[s], views[s]);
    if (rc) { if (s) c0->err = ctxs[s]->err; return rc; }
    it.emplace_back(ctxs[s], &views[s]);
    it.back().next();
  }
  const size_t k = (size_t)c0->k;
  std::vector<u64> row((size_t)n);
  std::vector<uint8_t> key(k + 1);
  if (as_reference) {
    const uint8_t* best = nullptr;
    for (int s = 0; s < n; ++s)
      if (it[s].cur && (!best || memcmp(it[s].cur, best, k) < 0)) best = it[s].cur;
    if (!best) return MK_OK;
    memcpy(key.data(), best, k);
    std::vector<uint8_t> next(k + 1);
    for (;;) {
      bool have_next = false;
      for (int s = 0; s < n; ++s) {
        if (!it[s].cur || memcmp(it[s].cur, key.data(), k) > 0) { row[s] = 0; continue; }
        row[s] = it[s].cnt;  // (whatever this sample's key is: see above)
        it[s].next();
        if (it[s].cur && (!have_next || memcmp(it[s].cur, next.data(), k) < 0)) { memcpy(next.data(), it[s].cur, k); have_next = true; }
      }
      f(key.data(), row.data());
      if (!have_next) break;
      key.swap(next);
    }
    return MK_OK;
  }
  for (;;) {
    const uint8_t* best = nullptr;
    for (int s = 0; s < n; ++s)
      if (it[s].cur && (!best || memcmp(it[s].cur, best, k) < 0)) best = it[s].cur;
    if (!best) break;
    memcpy(key.data(), best, k);
    for (int s = 0; s < n; ++s) {
      if (it[s].cur && memcmp(it[s].cur, key.data(), k) == 0) { row[s] = it[s].cnt; it[s].next(); }
      else row[s] = 0;
    }
    f(key.data(), row.data());
  }
  return MK_OK;
}
}  // namespace

extern "C" int mk_merged_export(mk_ctx* const* ctxs, int n, uint8_t* kmers, uint64_t* matrix, size_t rows_cap, size_t* rows) {
  if (!rows) return MK_ERR_ARG;
  for (int j_ = 0; ctxs && j_ < n; ++j_) if (ctxs[j_] && ctxs[j_]->spoiled) { ctxs[0]->err = "merged table: a context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  size_t at = 0;
  bool short_cap = false;
  const size_t k = ctxs && ctxs[0] ? (size_t)ctxs[0]->k : 0;
  int rc = merged_samples(ctxs, n, [&](const uint8_t* s, const u64* counts) {
    if (kmers && matrix) {
      if (at < rows_cap) {
        memcpy(kmers + at * k, s, k);
        memcpy(matrix + at * (size_t)n, counts, (size_t)n * sizeof(u64));
      } else short_cap = true;
    }
    ++at;
  });
  if (rc) return rc;
  *rows = at;
  if (short_cap) { ctxs[0]->err = "mk_merged_export: rows_cap too small"; return MK_ERR_RANGE; }
  return MK_OK;
}

static int write_merged(mk_ctx* const* ctxs, int n, const char* const* names, const char* first_column, const char* path,
                        size_t* rows_out, bool as_reference) {
  if (!ctxs || n < 1 || !ctxs[0] || !names || !first_column || !path) return MK_ERR_ARG;
  for (int j_ = 0; j_ < n; ++j_) if (ctxs[j_] && ctxs[j_]->spoiled) { ctxs[0]->err = "merged table: a context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  mk_ctx* c = ctxs[0];
  FILE* f = fopen(path, "wb");
  if (!f) { c->err = std::string("mk_write_merged_tsv: cannot open ") + path; return MK_ERR_IO; }
  std::vector<char> out;
  out.reserve(1 << 22);
  auto flush = [&]() {
    if (!out.empty()) fwrite(out.data(), 1, out.size(), f);
    out.clear();
  };
  {
    std::string head = first_column;
    for (int s = 0; s < n; ++s) { head += '\t'; head += names[s] ? names[s] : ""; }
    head += '\n';
    out.insert(out.end(), head.begin(), head.end());
  }
  const size_t k = (size_t)c->k;
  size_t rows = 0;
  int rc = merged_samples(ctxs, n, [&](const uint8_t* s, const u64* counts) {
    out.insert(out.end(), (const char*)s, (const char*)s + k);
    for (int q = 0; q < n; ++q) {
      out.push_back('\t');
      u64 v = counts[q];
      char num[24];
      int len = 0;
      do { num[len++] = (char)('0' + v % 10); v /= 10; } while (v);
      while (len) out.push_back(num[--len]);
    }
    out.push_back('\n');
    ++rows;
    if (out.size() > (1u << 22) - 4096 - k - 24 * (size_t)n) flush();
  }, as_reference);
  flush();
  const bool bad = ferror(f) != 0;
  if (fclose(f) != 0 || bad) { c->err = std::string("mk_write_merged_tsv: write failed: ") + path; return MK_ERR_IO; }
  if (rc) return rc;
  if (rows_out) *rows_out = rows;
  return MK_OK;
}
extern "C" int mk_write_merged_tsv(mk_ctx* const* ctxs, int n, const char* const* names, const char* first_column,
                                   const char* path, size_t* rows_out) {
  return write_merged(ctxs, n, names, first_column, path, rows_out, false);
}
extern "C" int mk_write_merged_tsv_as_reference(mk_ctx* const* ctxs, int n, const char* const* names, const char* first_column,
                                                const char* path, size_t* rows_out) {
  return write_merged(ctxs, n, names, first_column, path, rows_out, true);
}

// merge_tsv_T (lib/mercat2_report.py:160-194): the same matrix with samples as rows: "sample\t<k-mers>\n", then one
// line per sample.  The reference lists the k-mer columns in the iteration order of a Python set (different in
// every process); here they are sorted.  Consumers address columns by label (bin/mercat2.py:354-355).
extern "C" int mk_write_merged_tsv_t(mk_ctx* const* ctxs, int n, const char* const* names, const char* path, size_t* rows_out) {
  if (!ctxs || n < 1 || !ctxs[0] || !names || !path) return MK_ERR_ARG;
  for (int j_ = 0; j_ < n; ++j_) if (ctxs[j_] && ctxs[j_]->spoiled) { ctxs[0]->err = "merged table: a context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  mk_ctx* c = ctxs[0];
  const size_t k = (size_t)c->k;
  std::vector<uint8_t> kmers;
  std::vector<u64> matrix;  // rows x n
  int rc = merged_samples(ctxs, n, [&](const uint8_t* s, const u64* counts) {
    kmers.insert(kmers.end(), s, s + k);
    matrix.insert(matrix.end(), counts, counts + n);
  });
  if (rc) return rc;
  const size_t rows = k ? kmers.size() / k : 0;
  FILE* f = fopen(path, "wb");
  if (!f) { c->err = std::string("mk_write_merged_tsv_t: cannot open ") + path; return MK_ERR_IO; }
  std::vector<char> out;
  out.reserve(1 << 22);
  auto flush = [&]() {
    if (!out.empty()) fwrite(out.data(), 1, out.size(), f);
    out.clear();
  };
  const char* head = "sample";
  out.insert(out.end(), head, head + 6);
  for (size_t r = 0; r < rows; ++r) {
    out.push_back('\t');
    out.insert(out.end(), (const char*)kmers.data() + r * k, (const char*)kmers.data() + (r + 1) * k);
    if (out.size() > (1u << 22) - 4096 - k) flush();
  }
  out.push_back('\n');
  for (int s = 0; s < n; ++s) {
    const char* nm = names[s] ? names[s] : "";
    out.insert(out.end(), nm, nm + strlen(nm));
    for (size_t r = 0; r < rows; ++r) {
      out.push_back('\t');
      u64 v = matrix[r * (size_t)n + (size_t)s];
      char num[24];
      int len = 0;
      do { num[len++] = (char)('0' + v % 10); v /= 10; } while (v);
      while (len) out.push_back(num[--len]);
      if (out.size() > (1u << 22) - 4096) flush();
    }
    out.push_back('\n');
  }
  flush();
  const bool bad = ferror(f) != 0;
  if (fclose(f) != 0 || bad) { c->err = std::string("mk_write_merged_tsv_t: write failed: ") + path; return MK_ERR_IO; }
  if (rows_out) *rows_out = rows;
  return MK_OK;
}
