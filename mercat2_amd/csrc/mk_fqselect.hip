// mk_fqselect.hip -- a decision about the records of a FASTQ text applied to that text, qualities included
// (mk_fastq_select_text / mk_fastq_select_device, include/mercat_hip.h): keep[r] of mk_filter_* / mk_norm_* / mk_pairs_*
// and kept[r] of mk_trim_* were taken on the FASTA view fq2fa gives of the reads; here the 4-line records themselves are
// checked, chosen, cut -- the quality line wherever the sequence line is -- and gathered, on the GPU.  The tables are
// not read.
//
// A piece of n bytes (16-byte aligned: the caller's bytes or their copy in c->raw) goes through the steps of
// mk_fqindex.h, with two segments a record and a decision kernel of this call's own:
//   fs_index_open, fs_index_lines   with kept given the line pass also flags blanks and '*' on sequence lines
//   fs_decide_k                     a lane per record: the checks on '@', '+', the two lengths and kept[r] from line[] and
//                                   five bytes of text; keep / kept / which; the record's one or two segments {source,
//                                   length, force a '\n' as the last byte}.
//   rocprim::exclusive_scan         dst[s], dst[2 * nrec] = the piece's output length.  The status is read back here,
//                                   once, and no address is made of a length before it has been seen to be clean.
//   fs_gather
#include "mk_fqindex.h"

// A lane per record (and one for the slot behind the last segment, whose length is 0 so that the scan ends in the
// total).  Record r is lines 4r .. 4r + 3; its segments are 2r and 2r + 1.  Whole: one segment, the record's bytes (with
// a forced '\n' behind them where the text ends without one).  Cut (kept given, and the bytes differ from the input's):
// header line through the sequence prefix, plus line through the quality prefix, each with a forced '\n' as its last
// byte.  A record that fails a check gets no segment.
static __global__ void __launch_bounds__(256) fs_decide_k(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t nrec,
                                                          const uint8_t* __restrict__ keep, const u64* __restrict__ kept, unsigned which,
                                                          u64* __restrict__ seg_src, u64* __restrict__ len, FsStatus* __restrict__ st) {
  u64 n_out = 0, n_trimmed = 0, n_bases = 0;
  mk_for_each(nrec + 1, [&](size_t r) {
    if (r == nrec) {
      seg_src[2 * nrec] = 0;
      len[2 * nrec] = 0;
      return;
    }
    const u64 l0 = line[4 * r], l1 = line[4 * r + 1], l2 = line[4 * r + 2], l3 = line[4 * r + 3], l4 = line[4 * r + 4];
    // sequence line [l1, l2): its '\n' is there (a line follows it); quality line [l3, l4): the text may end without one
    u64 ls = l2 - 1 - l1, lq;
    const bool seq_cr = ls > 0 && text[l2 - 2] == 13u;
    ls -= seq_cr ? 1 : 0;
    const bool has_nl = text[l4 - 1] == 10u;
    lq = l4 - (has_nl ? 1 : 0) - l3;
    const bool qual_cr = lq > 0 && text[l3 + lq - 1] == 13u;
    lq -= qual_cr ? 1 : 0;
    const u64 want = kept ? kept[r] : ls;
    int fail = -1;
    if (text[l0] != '@') fail = FS_AT;
    else if (text[l2] != '+') fail = FS_PLUS;
    else if (ls != lq) fail = FS_LENGTH;
    else if (want > ls) fail = FS_KEPT;
    if (fail >= 0) atomicMin((unsigned long long*)&st->bad, (unsigned long long)(((u64)r << 3) | (unsigned)fail));
    const bool emit = fail < 0 && (!keep || keep[r] == which) && (!kept || want > 0);
    u64 s0 = 0, n0 = 0, s1 = 0, n1 = 0;
    if (emit) {
      if (!kept) {
        s0 = l0 | (has_nl ? 0 : FS_FORCE);
        n0 = l4 - l0 + (has_nl ? 0 : 1);
      } else if (want == ls && !seq_cr && !qual_cr && has_nl) {
        s0 = l0;
        n0 = l4 - l0;
      } else {
        s0 = l0 | FS_FORCE;
        n0 = l1 + want + 1 - l0;
        s1 = l2 | FS_FORCE;
        n1 = l3 + want + 1 - l2;
      }
      n_out += 1;
      n_trimmed += want < ls ? 1 : 0;
      n_bases += want;
    }
    seg_src[2 * r] = s0;
    len[2 * r] = n0;
    seg_src[2 * r + 1] = s1;
    len[2 * r + 1] = n1;
  });
  block_add(&st->records_out, n_out);
  block_add(&st->records_trimmed, n_trimmed);
  block_add(&st->bases_out, n_bases);
}

// ------------------------------------------------------------------------------------------ host side
struct FsCall : FsPieces {  // (limit: the records the caller announced)
  mk_ctx* c;
  const uint8_t* keep;  // the caller's arrays (host memory for the text call, device memory for the device call), or nullptr
  const u64* kept;
  unsigned which;
  uint8_t* out;
  size_t out_cap;
  bool device;
  MkDevBuf tiles, meta, d_keep, d_kept, scan_tmp, stage;
  MkTimed index, place, gather;
  mk_fastq_select_t st{};
  size_t bytes_out = 0;  // of all pieces so far
  FsCall(mk_ctx* c_, const char* w, const uint8_t* kp, const u64* kt, size_t nr, unsigned wh, uint8_t* o, size_t oc, bool dev)
      : FsPieces{w, nr}, c(c_), keep(kp), kept(kt), which(wh), out(o), out_cap(oc), device(dev), index(c_), place(c_), gather(c_) {}
  ~FsCall() {
    for (MkDevBuf* b : {&tiles, &meta, &d_keep, &d_kept, &scan_tmp, &stage}) buf_free(*b);
  }
};

// One piece of n > 0 bytes at d_text (device memory, 16-byte aligned, whole records but for what trails in the last
// piece).  Its records are added to f.records either way.  The stream is idle afterwards.
static int fs_piece(FsCall& f, const uint8_t* d_text, size_t n) {
  mk_ctx* c = f.c;
  int rc;
  FsIndex ix;
  if ((rc = fs_index_open(c, f.tiles, f.index, f.st.s_index, d_text, n, nullptr, 0, ix)) != MK_OK) return rc;
  FsStatus* d_st = ix.d_st;
  const size_t nrec = ix.nrec;
  size_t first;
  f.st.lines += ix.lines;
  if (!f.take(ix, first)) return MK_OK;

  // meta: line[4 nrec + 1] | seg_src[nseg + 1] | len[nseg + 1] | dst[nseg + 1]
  const size_t nseg = 2 * nrec, nidx = 4 * nrec;
  if ((rc = mk_buf_reserve(c, f.meta, (nidx + 1 + 3 * (nseg + 1)) * sizeof(u64))) != MK_OK) return rc;
  u64* line = (u64*)f.meta.p;
  u64* seg_src = line + nidx + 1;
  u64* len = seg_src + nseg + 1;
  u64* dst = len + nseg + 1;
  size_t tmp = 0;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, nseg + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;
  // the piece's own slice of the caller's arrays
  const uint8_t* d_keep = f.keep ? f.keep + first : nullptr;
  const u64* d_kept = f.kept ? f.kept + first : nullptr;
  if (!f.device && (f.keep || f.kept)) {
    if (f.keep && (rc = mk_buf_reserve(c, f.d_keep, nrec)) != MK_OK) return rc;
    if (f.kept && (rc = mk_buf_reserve(c, f.d_kept, nrec * sizeof(u64))) != MK_OK) return rc;
    const auto t1 = MkClock::now();
    if (f.keep) MK_HIP(hipMemcpyAsync(f.d_keep.p, f.keep + first, nrec, hipMemcpyHostToDevice, c->stream));
    if (f.kept) MK_HIP(hipMemcpyAsync(f.d_kept.p, f.kept + first, nrec * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_copy += mk_since(t1);
    d_keep = f.keep ? (const uint8_t*)f.d_keep.p : nullptr;
    d_kept = f.kept ? (const u64*)f.d_kept.p : nullptr;
  }

  if ((rc = d_kept ? fs_index_lines<true>(c, f.index, d_text, n, ix, line) : fs_index_lines<false>(c, f.index, d_text, n, ix, line)) != MK_OK)
    return rc;
  if ((rc = f.place.begin()) != MK_OK) return rc;
  // (the lengths are only added up before the status below has been read: no address is made of them)
  hipLaunchKernelGGL(fs_decide_k, dim3(grid_for(nrec + 1, 256, 4096)), dim3(256), 0, c->stream, d_text, (const u64*)line, nrec, d_keep,
                     d_kept, f.which, seg_src, len, d_st);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nseg + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = f.place.end()) != MK_OK) return rc;
  u64 piece_out = 0;
  FsStatus h;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nseg, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.index.add_to(f.st.s_index)) != MK_OK) return rc;
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (h.bad != FS_NONE && (h.bad & 7) == FS_KEPT)  // (a kept[r] that is too long is the caller's mistake, not the text's)
    return f.fail(MK_ERR_RANGE, fs_msg_malformed(f.what, first + (size_t)(h.bad >> 3), fs_kind(FS_KEPT), false));
  if (f.failed(ix, first, h.bad, fs_kind)) return MK_OK;
  if (piece_out > (u64)n + 1) {
    c->err = std::string(f.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.records_out += h.records_out;
  f.st.records_trimmed += h.records_trimmed;
  f.st.bases_out += h.bases_out;
  return fs_gather(c, f.gather, f.stage, d_text, n, seg_src, dst, nseg, piece_out, f.out, f.out_cap, f.device, f.bytes_out, f.st.s_gather,
                   f.st.s_write);
}

// How both calls check their arguments, open and end; body(): the pieces.
template <class Body>
static int fs_run(FsCall& f, size_t* out_len, mk_fastq_select_t* st, Body&& body) {
  mk_ctx* c = f.c;
  int rc = fs_call(
      c, f.what,
      [&]() -> int {
        if (!out_len) { c->err = std::string(f.what) + ": out_len is NULL"; return MK_ERR_ARG; }
        *out_len = 0;
        if (f.which != 1 && f.which != 2) { c->err = std::string(f.what) + ": which must be 1 (the main output) or 2 (the orphans)"; return MK_ERR_ARG; }
        return MK_OK;
      },
      body);
  if (rc != MK_OK) return rc;
  if (f.records != f.limit) {
    c->err = std::string(f.what) + ": the text holds " + std::to_string(f.records) + " records, the caller announced " + std::to_string(f.limit);
    return MK_ERR_RANGE;
  }
  if ((rc = fs_call_end(c, f.what, f.records, false, f.bad_rc, f.bad_msg)) != MK_OK) return rc;
  *out_len = f.bytes_out;
  if ((rc = fs_out_room(c, f.what, f.bytes_out, f.out_cap)) != MK_OK) return rc;
  f.st.records = f.records;
  f.st.bytes_out = f.bytes_out;
  if (st) *st = f.st;
  return MK_OK;
}

extern "C" int mk_fastq_select_device(mk_ctx* c, const uint8_t* d_fastq, size_t n, const uint8_t* d_keep, const uint64_t* d_kept, size_t nrec,
                                      unsigned which, uint8_t* d_out, size_t out_cap, size_t* out_len, mk_fastq_select_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !d_fastq) || (out_cap && !d_out)) { c->err = "mk_fastq_select_device: NULL buffer"; return MK_ERR_ARG; }
  if ((uintptr_t)d_kept & 7) { c->err = "mk_fastq_select_device: d_kept must be aligned to 8"; return MK_ERR_ARG; }
  FsCall f(c, "mk_fastq_select_device", d_keep, (const u64*)d_kept, nrec, d_keep ? which : 1u, d_out, out_cap, true);
  return fs_run(f, out_len, st, [&]() -> int {
    if (!n) return MK_OK;
    const uint8_t* d_text;
    const int rc = fs_aligned_text(c, d_fastq, n, false, f.st.s_copy, &d_text);
    return rc != MK_OK ? rc : fs_piece(f, d_text, n);
  });
}

extern "C" int mk_fastq_select_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const uint8_t* keep, const uint64_t* kept,
                                    size_t nrec, unsigned which, uint8_t* out, size_t out_cap, size_t* out_len, mk_fastq_select_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_fastq_select_text: NULL buffer"; return MK_ERR_ARG; }
  FsCall f(c, "mk_fastq_select_text", keep, (const u64*)kept, nrec, keep ? which : 1u, out, out_cap, false);
  return fs_run(f, out_len, st, [&]() -> int {
    if (!n) return MK_OK;
    std::vector<uint64_t> cuts;
    int rc = fs_piece_cuts(c, f.what, fastq, n, piece_bytes, false, cuts);
    if (rc != MK_OK) return rc;
    size_t at = 0;
    for (const uint64_t end : cuts) {
      const size_t len = (size_t)end - at;
      if (!len) continue;
      if ((rc = fs_upload_raw(c, fastq + at, len, f.st.s_copy)) != MK_OK) return rc;
      if ((rc = fs_piece(f, (const uint8_t*)c->raw.p, len)) != MK_OK) return rc;
      at = (size_t)end;
    }
    return MK_OK;
  });
}
