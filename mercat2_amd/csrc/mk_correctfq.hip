// mk_correctfq.hip -- FASTQ text in, the same text out with every isolated substitution the table can name put right and
// the qualities where they were (mk_correct_fastq_text / mk_correct_fastq_device, include/mercat_hip.h).  The output
// has the input's length: every record is emitted and a fix replaces one byte by one byte, so nothing is gathered --
// the raw text is indexed once, its FASTA view (mk_launch_fastq_pre: in place, nothing moved, a base at byte x of the
// text is at byte x of the view) goes through the correcting call's own steps, and the patches those leave go into the
// raw bytes.
//
// A piece of n bytes (16-byte aligned, in c->raw):
//   fs_index_open, fs_index_lines<true>         the line index (mk_fqindex.h) with the check of the sequence lines' bytes
//   cq_check_k                                  a lane per record: '@', '+', the two lengths, from five line[] entries and
//                                               a few bytes; atomicMin(record << 3 | check) as fs_decide_k.  Read back
//                                               here: a text that fails is not parsed.
//   mk_launch_fastq_pre                         c->raw becomes the view (into a stats word of the call, not the context's)
//   sc_piece, cr_front, cr_totals               mk_correct_*'s piece through cr_try_k, its guards and totals
//                                               (mk_correctwalk.h); cr_apply_k is not launched -- no total reads the
//                                               stream's bytes -- and neither are the scan and the gather
//   cq_view_k                                   a lane per record: the parser found the record where the index has it
//                                               (start[r] == line[4r]) and read exactly the sequence line's bytes
//                                               (slen[r]).  Read back here: nothing is patched before it is clean.
//   cq_patch_k                                  a lane per candidate with a patch: one byte store into the raw text at
//                                               line[4r + 1] + (ppos - sstart[r]) and, with new_qual, one at line[4r + 3] +
//                                               the same.  No two candidates share a p: no atomics.
#include "mk_correctwalk.h"
#include "mk_fqindex.h"

struct CqStatus {  // device memory: what cq_view_k and cq_patch_k found
  u64 bad;         // the lowest record the parser read differently (FS_NONE: none)
  u64 patched;     // sequence bytes written
  u64 outside;     // patches that would have fallen outside their line or the text
  u64 pad;
};

// The length of the line [a, b) whose '\n', if it has one, is byte b - 1, one trailing '\r' not counted.
__device__ __forceinline__ u64 cq_line_len(const uint8_t* __restrict__ text, u64 a, u64 b, bool has_nl) {
  u64 len = b - (has_nl ? 1 : 0) - a;
  if (len > 0 && text[a + len - 1] == 13u) --len;
  return len;
}

// A lane per record of the raw text: the checks fs_decide_k makes, in its order, and its status word.
static __global__ void __launch_bounds__(256) cq_check_k(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t nrec,
                                                         FsStatus* __restrict__ st) {
  mk_for_each(nrec, [&](size_t r) {
    const u64 l0 = line[4 * r], l1 = line[4 * r + 1], l2 = line[4 * r + 2], l3 = line[4 * r + 3], l4 = line[4 * r + 4];
    // sequence line [l1, l2): its '\n' is there (a line follows it); quality line [l3, l4): the text may end without one
    const u64 ls = cq_line_len(text, l1, l2, true), lq = cq_line_len(text, l3, l4, text[l4 - 1] == 10u);
    int fail = -1;
    if (text[l0] != '@') fail = FS_AT;
    else if (text[l2] != '+') fail = FS_PLUS;
    else if (ls != lq) fail = FS_LENGTH;
    if (fail >= 0) atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | (unsigned)fail));
  });
}

// A lane per record that both the index and the parser have (nboth = min of the two counts): the parser's record r
// starts where line 4r starts and its characters in the stream number the sequence line's bytes.
static __global__ void __launch_bounds__(256) cq_view_k(const uint8_t* __restrict__ view, const u64* __restrict__ line,
                                                        const u64* __restrict__ start, const u64* __restrict__ slen, size_t nboth,
                                                        CqStatus* __restrict__ st) {
  mk_for_each(nboth, [&](size_t r) {
    const u64 l1 = line[4 * r + 1], l2 = line[4 * r + 2];
    if (start[r] != line[4 * r] || slen[r] != cq_line_len(view, l1, l2, true))
      atomicMin((unsigned long long*)&st->bad, (unsigned long long)r);
  });
}

// A lane per candidate: its patch, if it has one, into the raw text, and new_qual (if not 0) under it.
static __global__ void __launch_bounds__(256) cq_patch_k(const CrCand* __restrict__ list, const uint8_t* __restrict__ patch, u64 ncand,
                                                         const u64* __restrict__ line, const u64* __restrict__ sstart,
                                                         const u64* __restrict__ slen, size_t nrec, u64 n, unsigned new_qual,
                                                         uint8_t* __restrict__ out, CqStatus* __restrict__ st) {
  // (the loop of mk_for_each spelled out: a byte store may alias anything a lambda holds by reference, and the two
  // counters went to scratch for it)
  u64 done = 0, bad = 0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t ci = (size_t)blockIdx.x * 256 + threadIdx.x; ci < (size_t)ncand; ci += stride) {
    const uint8_t x = patch[ci];
    if (!x) continue;
    const u64 ppos = list[ci].ppos;
    const size_t r = list[ci].rec;
    bool ok = r < nrec && ppos >= sstart[r] && ppos - sstart[r] < slen[r];
    u64 at = 0, qat = 0;
    if (ok) {
      const u64 off = ppos - sstart[r];
      at = line[4 * r + 1] + off;
      qat = line[4 * r + 3] + off;
      ok = at < n && qat < n;
    }
    if (ok) {
      out[at] = x;
      if (new_qual) out[qat] = (uint8_t)new_qual;
    }
    done += ok ? 1 : 0;
    bad += ok ? 0 : 1;
  }
  block_add(&st->patched, done);
  block_add(&st->outside, bad);
}

// ------------------------------------------------------------------------------------------ host side
struct CqCall {
  mk_ctx* c;
  const char* what;
  unsigned new_qual;
  MkDevBuf tiles, lines, stats, cq, stage;
  MkTimed index, patch;
  mk_correct_fastq_t st{};
  size_t records = 0;  // FASTQ records of the pieces so far
  CqCall(mk_ctx* c_, const char* w, unsigned q) : c(c_), what(w), new_qual(q), index(c_), patch(c_) {}
  ~CqCall() {
    for (MkDevBuf* b : {&tiles, &lines, &stats, &cq, &stage}) buf_free(*b);
  }
};

// One piece of n > 0 raw bytes in d_view (c->raw: 16-byte aligned, whole records but for what trails in the last piece),
// which becomes the view.  d_dst: where the corrected bytes go (device memory); it holds the raw bytes already unless
// d_src is given, which is then copied there once every check has passed.  The stream is idle afterwards.
static int cq_piece(ScCall& s, CrCall& f, CqCall& q, uint8_t* d_view, size_t n, uint8_t* d_dst, const uint8_t* d_src) {
  mk_ctx* c = s.c;
  int rc;
  FsIndex ix;
  if ((rc = fs_index_open(c, q.tiles, q.index, q.st.s_index, d_view, n, nullptr, 0, ix)) != MK_OK) return rc;
  FsStatus* d_st = ix.d_st;
  const size_t nrec = ix.nrec, first = q.records;
  q.st.lines += ix.lines;
  q.records += nrec;
  // (a failed check ends the call at once: no piece behind it is parsed)
  const auto fail_trailing = [&]() {
    c->err = fs_msg_incomplete(q.what, first + nrec, ix.trailing);
    return MK_ERR_UNSUPPORTED;
  };
  if (!nrec) {  // (empty lines only: nothing to parse; the piece counts among the bytes read as any other)
    if (!ix.trail_ok) return fail_trailing();
    s.out.bytes += n;
    s.out.pieces += 1;
    if (d_src) MK_HIP(hipMemcpyAsync(d_dst, d_src, n, hipMemcpyDeviceToDevice, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    return MK_OK;
  }

  const size_t nidx = 4 * nrec;
  if ((rc = mk_buf_reserve(c, q.lines, (nidx + 1) * sizeof(u64))) != MK_OK) return rc;
  u64* line = (u64*)q.lines.p;
  rc = fs_index_lines<true>(c, q.index, d_view, n, ix, line, [&]() {
    hipLaunchKernelGGL(cq_check_k, dim3(grid_for(nrec, 256, 4096)), dim3(256), 0, c->stream, (const uint8_t*)d_view, (const u64*)line, nrec, d_st);
  });
  if (rc != MK_OK) return rc;
  FsStatus h;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = q.index.add_to(q.st.s_index)) != MK_OK) return rc;
  if (h.bad != FS_NONE) {
    c->err = fs_msg_malformed(q.what, first + (size_t)(h.bad >> 3), fs_kind((unsigned)(h.bad & 7)));
    return MK_ERR_UNSUPPORTED;
  }
  if (!ix.trail_ok) return fail_trailing();

  // the view, in place; its figures go to a word of the call: what mk_fastq_stats reports is the counting path's alone
  std::swap(c->fastq_stats, q.stats);
  rc = mk_launch_fastq_pre(c, d_view, n);
  std::swap(c->fastq_stats, q.stats);
  if (rc != MK_OK) return rc;

  // mk_correct_*'s piece on the view, through cr_try_k and the totals
  const u64 w0 = s.out.windows, h0 = s.out.hits;
  if ((rc = sc_piece(s, d_view, n, nullptr, ~(size_t)0, &f.d_rows, nullptr)) != MK_OK) return rc;
  const size_t nrows = s.last.nrows;
  const auto fail_counts = [&]() {
    c->err = std::string(q.what) + ": the FASTA view of a piece holds " + std::to_string(nrows) + " records, its FASTQ text " +
             std::to_string(nrec) + ": the parser does not read every record as its four lines";
    return MK_ERR_UNSUPPORTED;
  };
  if (!nrows) return fail_counts();
  CrLay lay{};
  if ((rc = cr_front(s, f, n, s.out.windows - w0, s.out.hits - h0, lay)) != MK_OK) return rc;
  if ((rc = cr_totals(s, f, lay, nullptr)) != MK_OK) return rc;

  if ((rc = mk_buf_reserve(c, q.cq, sizeof(CqStatus))) != MK_OK) return rc;
  CqStatus* d_cq = (CqStatus*)q.cq.p;
  CqStatus hq{};
  hq.bad = FS_NONE;
  MK_HIP(hipMemcpyAsync(d_cq, &hq, sizeof hq, hipMemcpyHostToDevice, c->stream));
  if ((rc = q.patch.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(cq_view_k, dim3(grid_for(std::min(nrec, nrows), 256, 4096)), dim3(256), 0, c->stream, (const uint8_t*)d_view,
                     (const u64*)line, (const u64*)lay.start, (const u64*)lay.slen, std::min(nrec, nrows), d_cq);
  MK_HIP(hipGetLastError());
  if ((rc = q.patch.end()) != MK_OK) return rc;
  MK_HIP(hipMemcpyAsync(&hq, d_cq, sizeof hq, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = q.patch.add_to(q.st.s_patch)) != MK_OK) return rc;
  if (hq.bad != FS_NONE) {
    c->err = std::string(q.what) + ": record " + std::to_string(first + (size_t)hq.bad) +
             ": the parser does not read its sequence line as that line's bytes (a line that starts with '>' is a header line of "
             "the FASTA view)";
    return MK_ERR_UNSUPPORTED;
  }
  if (nrows != nrec) return fail_counts();
  if ((rc = cr_rows_out(s, f, lay, first)) != MK_OK) return rc;

  // every check has passed: the raw bytes to their place, the patches into them
  if (d_src) MK_HIP(hipMemcpyAsync(d_dst, d_src, n, hipMemcpyDeviceToDevice, c->stream));
  if (f.ncand) {
    if ((rc = q.patch.begin()) != MK_OK) return rc;
    hipLaunchKernelGGL(cq_patch_k, dim3(grid_for((size_t)f.ncand, 256, 4096)), dim3(256), 0, c->stream, (const CrCand*)f.list.p,
                       (const uint8_t*)f.patch.p, f.ncand, (const u64*)line, (const u64*)lay.sstart, (const u64*)lay.slen, nrec, (u64)n,
                       q.new_qual, d_dst, d_cq);
    MK_HIP(hipGetLastError());
    if ((rc = q.patch.end()) != MK_OK) return rc;
    MK_HIP(hipMemcpyAsync(&hq, d_cq, sizeof hq, hipMemcpyDeviceToHost, c->stream));
  }
  MK_HIP(hipStreamSynchronize(c->stream));
  if (f.ncand && (rc = q.patch.add_to(q.st.s_patch)) != MK_OK) return rc;
  if (hq.outside) {
    c->err = std::string(q.what) + ": " + std::to_string(hq.outside) + " patch(es) outside their sequence lines (internal error)";
    return MK_ERR_STATE;
  }
  q.st.patched += hq.patched;
  return MK_OK;
}

// How both calls check their own arguments, open as the screen calls open, and end; body(s): the pieces.
template <class Body>
static int cq_run(mk_ctx* c, unsigned flags, const mk_correct_fastq_rule_t* rule, size_t n, size_t out_cap, CrCall* f, CqCall* q,
                  size_t* out_len, size_t* nrows, mk_correct_fastq_t* st, Body&& body) {
  const char* what = q->what;
  if (out_len) *out_len = 0;
  if (!rule) { c->err = std::string(what) + ": rule is NULL"; return MK_ERR_ARG; }
  if (flags & ~MK_CORRECT_FOLD) { c->err = std::string(what) + ": unknown flag"; return MK_ERR_ARG; }
  if (rule->at_least < 1) { c->err = std::string(what) + ": at_least must be 1 or more"; return MK_ERR_ARG; }
  if (rule->reserved) { c->err = std::string(what) + ": reserved must be 0"; return MK_ERR_ARG; }
  if (rule->new_qual && (rule->new_qual < 33 || rule->new_qual > 126)) {
    c->err = std::string(what) + ": new_qual must be 0 or a printable quality character (33..126)";
    return MK_ERR_ARG;
  }
  if (c->alphabet != MK_ALPHABET_NT2 || c->k > 64 || tl_keys_of(c) == TL_TEXT_ONLY) {
    c->err = std::string(what) + ": takes a nucleotide context with packed keys (ALPHABET_NT2, k <= 64)";
    return MK_ERR_ARG;
  }
  if (out_cap < n) {  // (the output has the input's length: known before any work)
    if (out_len) *out_len = n;
    return fs_out_room(c, what, n, out_cap);
  }
  f->cap = (f->rows || f->fix) ? f->cap : ~(size_t)0;
  f->apply = false;
  const int rc = sc_run(c, what, flags & MK_CORRECT_FOLD, rule->at_least, f->cap, nrows, &f->st.screen, [&](ScCall& s) { return body(s); });
  if (rc == MK_ERR_RANGE && out_len) *out_len = n;
  if (rc != MK_OK) return rc;
  if (q->st.patched != f->st.fixed) {
    c->err = std::string(what) + ": " + std::to_string(q->st.patched) + " bytes patched for " + std::to_string(f->st.fixed) +
             " fixed runs (internal error)";
    return MK_ERR_STATE;
  }
  if (out_len) *out_len = n;
  f->st.bytes_out = n;
  q->st.correct = f->st;
  if (st) *st = q->st;
  return MK_OK;
}

extern "C" int mk_correct_fastq_device(mk_ctx* c, const uint8_t* d_fastq, size_t n, unsigned flags, const mk_correct_fastq_rule_t* rule,
                                       uint8_t* d_out, size_t out_cap, size_t* out_len, mk_correct_row_t* d_fix, mk_screen_row_t* d_rows,
                                       size_t cap, size_t* nrows, mk_correct_fastq_t* st) {
  if (!c) return MK_ERR_ARG;
  if (out_len) *out_len = 0;
  if ((n && !d_fastq) || (out_cap && !d_out)) { c->err = "mk_correct_fastq_device: NULL buffer"; return MK_ERR_ARG; }
  if (((uintptr_t)d_fix | (uintptr_t)d_rows) & 7) { c->err = "mk_correct_fastq_device: fix and rows must be aligned to 8"; return MK_ERR_ARG; }
  if (d_out && d_out != d_fastq && out_cap >= n && (uintptr_t)d_out < (uintptr_t)d_fastq + n && (uintptr_t)d_fastq < (uintptr_t)d_out + n) {
    c->err = "mk_correct_fastq_device: d_out overlaps d_fastq (d_out == d_fastq corrects in place)";
    return MK_ERR_ARG;
  }
  const mk_correct_rule_t cr{rule ? rule->at_least : 0, 0};
  CrCall f(c, cr, nullptr, 0, d_fix, d_rows, cap, true);
  CqCall q(c, "mk_correct_fastq_device", rule ? rule->new_qual : 0);
  return cq_run(c, flags, rule, n, out_cap, &f, &q, out_len, nrows, st, [&](ScCall& s) -> int {
    if (!n) return MK_OK;
    const uint8_t* d_view;  // (always the call's own copy: it becomes the view)
    const int rc = fs_aligned_text(c, d_fastq, n, true, q.st.s_copy, &d_view);
    return rc != MK_OK ? rc : cq_piece(s, f, q, (uint8_t*)c->raw.p, n, d_out, d_out != d_fastq ? d_fastq : nullptr);
  });
}

extern "C" int mk_correct_fastq_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, unsigned flags,
                                     const mk_correct_fastq_rule_t* rule, uint8_t* out, size_t out_cap, size_t* out_len,
                                     mk_correct_row_t* fix, mk_screen_row_t* rows, size_t cap, size_t* nrows, mk_correct_fastq_t* st) {
  if (!c) return MK_ERR_ARG;
  if (out_len) *out_len = 0;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_correct_fastq_text: NULL buffer"; return MK_ERR_ARG; }
  const mk_correct_rule_t cr{rule ? rule->at_least : 0, 0};
  CrCall f(c, cr, nullptr, 0, fix, rows, cap, false);
  CqCall q(c, "mk_correct_fastq_text", rule ? rule->new_qual : 0);
  return cq_run(c, flags, rule, n, out_cap, &f, &q, out_len, nrows, st, [&](ScCall& s) -> int {
    if (!n) return MK_OK;
    // The corrected pieces stay on the device until the last has passed its checks: out is written once, or not at all.
    std::vector<uint64_t> cuts;
    int rc = fs_piece_cuts(c, q.what, fastq, n, piece_bytes, false, cuts);
    if (rc != MK_OK) return rc;
    rc = mk_buf_reserve(c, q.stage, n);
    if (rc != MK_OK) return rc;
    uint8_t* stage = (uint8_t*)q.stage.p;
    size_t at = 0;
    for (const uint64_t end : cuts) {
      const size_t len = (size_t)end - at;
      if (!len) continue;
      if ((rc = mk_buf_reserve(c, c->raw, len + 64)) != MK_OK) return rc;
      const auto t1 = MkClock::now();
      MK_HIP(hipMemcpyAsync(stage + at, fastq + at, len, hipMemcpyHostToDevice, c->stream));
      MK_HIP(hipMemcpyAsync(c->raw.p, stage + at, len, hipMemcpyDeviceToDevice, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      q.st.s_copy += mk_since(t1);
      if ((rc = cq_piece(s, f, q, (uint8_t*)c->raw.p, len, stage + at, nullptr)) != MK_OK) return rc;
      at = (size_t)end;
    }
    if (s.rows_seen > f.cap) return MK_OK;  // (MK_ERR_RANGE: out stays as it is)
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(out, stage, n, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
    return MK_OK;
  });
}
