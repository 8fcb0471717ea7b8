// mk_fqselect.hip -- a decision about the records of a FASTQ text applied to that text, qualities included
// (mk_fastq_select_text / mk_fastq_select_device, include/mercat_hip.h): keep[r] of mk_filter_* / mk_norm_* / mk_pairs_*
// and kept[r] of mk_trim_* were taken on the FASTA view fq2fa gives of the reads; here the 4-line records themselves are
// checked, chosen, cut -- the quality line wherever the sequence line is -- and gathered, on the GPU.  The tables are
// not read.
//
// A piece of n bytes (16-byte aligned: the caller's bytes or their copy in c->raw):
//   fs_tiles_k / fs_scan_k   the tiling of mk_fastq.hip (256 lanes x 16 bytes, a newline mask a lane): '\n' per tile, then
//                            one workgroup turns the counts into prefixes (sc_tile_scan: any number of tiles) and leaves
//                            the total.  The host reads it back with the text's last bytes: lines, records, and whether
//                            what trails behind the last complete record is empty lines only.
//   fs_lines_k               line[L] = first byte of line L for L <= 4 * nrec (the end slot is n when no such line
//                            starts).  With kept given the same pass knows every byte's line phase and flags blanks and
//                            '*' on sequence lines: atomicMin of (record << 3 | FS_BLANK) into the status word.
//   fs_decide_k              a lane per record: the checks on '@', '+', the two lengths and kept[r] from line[] and five
//                            bytes of text; keep / kept / which; the record's one or two segments {source, length,
//                            force a '\n' as the last byte}.
//   rocprim::exclusive_scan  dst[s], dst[2 * nrec] = the piece's output length.  The status is read back here, once, and
//                            no address is made of a length before it has been seen to be clean.
//   fs_gather_k (fs_edges_k) (in mk_fqindex.h: mk_qtrim.hip gathers with them too)
//                            fl_gather_k's scheme (mk_recordplace.h) over segments: output-driven, a lane owns 16 aligned
//                            output bytes a round, one search a wave, fl_record_from from there, fl_load16 / mask /
//                            shift / OR per segment, and the last byte of a flagged segment that ends in the chunk
//                            replaced by '\n' -- the base behind a trimmed prefix, the '\r' of CR LF, the 0 that
//                            fl_load16 reads behind a text without final newline.  No atomics, plain 16-byte stores,
//                            byte stores for the at most 15 + 15 edge bytes only.
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
struct FsCall {
  mk_ctx* c;
  const char* what;
  const uint8_t* keep;  // the caller's arrays (host memory for the text call, device memory for the device call), or nullptr
  const u64* kept;
  size_t nrec;
  unsigned which;
  uint8_t* out;
  size_t out_cap;
  bool device;
  MkDevBuf tiles, meta, d_keep, d_kept, scan_tmp, stage;
  MkTimed index, place, gather;
  mk_fastq_select_t st{};
  size_t records = 0, bytes_out = 0;  // of all pieces so far
  // the first record that failed a check (pieces come in text order: the first found is the lowest)
  int bad_rc = MK_OK;
  std::string bad_msg;
  FsCall(mk_ctx* c_, const char* w, const uint8_t* kp, const u64* kt, size_t nr, unsigned wh, uint8_t* o, size_t oc, bool dev)
      : c(c_), what(w), keep(kp), kept(kt), nrec(nr), which(wh), out(o), out_cap(oc), device(dev), index(c_), place(c_), gather(c_) {}
  ~FsCall() {
    for (MkDevBuf* b : {&tiles, &meta, &d_keep, &d_kept, &scan_tmp, &stage}) buf_free(*b);
  }
  // once a record has failed, or the text holds more records than the arrays, the pieces are only counted
  bool counting_only() const { return bad_rc != MK_OK || records > nrec; }
};

// One piece of n > 0 bytes at d_text (device memory, 16-byte aligned, whole records but for what trails in the last
// piece).  Its records are added to f.records either way.  The stream is idle afterwards.
static int fs_piece(FsCall& f, const uint8_t* d_text, size_t n) {
  mk_ctx* c = f.c;
  int rc;
  const size_t ntiles = div_up(n, FS_TILE);
  // tiles: FsStatus (48) | tile_pre[ntiles] | tile_cnt[ntiles]
  if ((rc = mk_buf_reserve(c, f.tiles, sizeof(FsStatus) + ntiles * (sizeof(u64) + sizeof(unsigned)))) != MK_OK) return rc;
  FsStatus* d_st = (FsStatus*)f.tiles.p;
  u64* tile_pre = (u64*)((char*)f.tiles.p + sizeof(FsStatus));
  unsigned* tile_cnt = (unsigned*)(tile_pre + ntiles);
  FsStatus h{};
  h.bad = FS_NONE;
  MK_HIP(hipMemcpyAsync(d_st, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
  if ((rc = f.index.begin()) != MK_OK) return rc;
  hipLaunchKernelGGL(fs_tiles_k, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_text, (u64)n, tile_cnt);
  hipLaunchKernelGGL(fs_scan_k, dim3(1), dim3(1024), 0, c->stream, (const unsigned*)tile_cnt, ntiles, tile_pre, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.index.end()) != MK_OK) return rc;
  uint8_t tail[4] = {0, 0, 0, 0};
  const size_t ntail = std::min<size_t>(n, 4);
  u64 newlines = 0;
  MK_HIP(hipMemcpyAsync(&newlines, &d_st->newlines, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(tail + (4 - ntail), d_text + (n - ntail), ntail, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.index.add_to(f.st.s_index)) != MK_OK) return rc;
  const u64 lines = newlines + (tail[3] != '\n' ? 1 : 0);
  const size_t nrec = (size_t)(lines / 4), first = f.records;
  const unsigned trailing = (unsigned)(lines & 3);
  f.st.lines += lines;
  f.records += nrec;
  // what trails behind the last complete record: `trailing` empty lines are that many '\n' behind a '\n' (or the text's start)
  bool trail_ok = true;
  for (unsigned i = 0; i < trailing && trail_ok; ++i) trail_ok = tail[3 - i] == '\n';
  if (trailing && trail_ok && n > trailing) trail_ok = tail[3 - trailing] == '\n';
  if (f.counting_only()) return MK_OK;
  const auto fail_trailing = [&]() {
    f.bad_rc = MK_ERR_UNSUPPORTED;
    f.bad_msg = std::string(f.what) + ": record " + std::to_string(first + nrec) + " is malformed: the text ends inside it (" +
                std::to_string(trailing) + " of its 4 lines)";
    return MK_OK;
  };
  if (!nrec) return trail_ok ? MK_OK : fail_trailing();

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

  if ((rc = f.index.begin()) != MK_OK) return rc;
  const int end_is_n = lines == nidx ? 1 : 0;  // (no line 4 nrec starts: the last record ends with the text)
  if (d_kept)
    hipLaunchKernelGGL(fs_lines_k<true>, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_text, (u64)n, (const u64*)tile_pre, (u64)nidx,
                       end_is_n, line, d_st);
  else
    hipLaunchKernelGGL(fs_lines_k<false>, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_text, (u64)n, (const u64*)tile_pre, (u64)nidx,
                       end_is_n, line, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.index.end()) != MK_OK) return rc;
  if ((rc = f.place.begin()) != MK_OK) return rc;
  // (the lengths are only added up before the status below has been read: no address is made of them)
  hipLaunchKernelGGL(fs_decide_k, dim3(grid_for(nrec + 1, 256, 4096)), dim3(256), 0, c->stream, d_text, (const u64*)line, nrec, d_keep,
                     d_kept, f.which, seg_src, len, d_st);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nseg + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = f.place.end()) != MK_OK) return rc;
  u64 piece_out = 0;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nseg, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.index.add_to(f.st.s_index)) != MK_OK) return rc;
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (h.bad != FS_NONE) {
    const unsigned kind = (unsigned)(h.bad & 7);
    f.bad_rc = kind == FS_KEPT ? MK_ERR_RANGE : MK_ERR_UNSUPPORTED;
    f.bad_msg = std::string(f.what) + ": record " + std::to_string(first + (size_t)(h.bad >> 3)) +
                (kind == FS_KEPT ? ": " : " is malformed: ") + fs_kind(kind);
    return MK_OK;
  }
  if (!trail_ok) return fail_trailing();
  if (piece_out > (u64)n + 1) {
    c->err = std::string(f.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.records_out += h.records_out;
  f.st.records_trimmed += h.records_trimmed;
  f.st.bases_out += h.bases_out;

  // the gather: into the caller's device memory, or into a staging buffer that is copied to the host.  Without room the
  // call goes on adding up and answers MK_ERR_RANGE at its end.
  const size_t at = f.bytes_out;
  f.bytes_out += (size_t)piece_out;
  if (!piece_out || f.bytes_out > f.out_cap) return MK_OK;
  uint8_t* d_out = f.out + at;
  if (!f.device) {
    if ((rc = mk_buf_reserve(c, f.stage, (size_t)piece_out)) != MK_OK) return rc;
    d_out = (uint8_t*)f.stage.p;
  }
  const u64 head = std::min<u64>((16 - ((uintptr_t)d_out & 15)) & 15, piece_out);
  const u64 nbody = (piece_out - head) / 16, tail_at = head + 16 * nbody;
  if ((rc = f.gather.begin()) != MK_OK) return rc;
  if (nbody)
    hipLaunchKernelGGL(fs_gather_k, dim3((unsigned)div_up((size_t)nbody, 256 * FS_CHUNKS)), dim3(256), 0, c->stream, d_text, (u64)n,
                       (const u64*)seg_src, (const u64*)dst, nseg, head, nbody, d_out);
  if (head || tail_at < piece_out)
    hipLaunchKernelGGL(fs_edges_k, dim3(1), dim3(64), 0, c->stream, d_text, (u64)n, (const u64*)seg_src, (const u64*)dst, nseg, head,
                       tail_at, piece_out, d_out);
  MK_HIP(hipGetLastError());
  if ((rc = f.gather.end()) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.gather.add_to(f.st.s_gather)) != MK_OK) return rc;
  if (!f.device) {
    const auto t1 = MkClock::now();
    MK_HIP(hipMemcpyAsync(f.out + at, d_out, (size_t)piece_out, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }
  return MK_OK;
}

// How both calls check their arguments, open and end; body(): the pieces.
template <class Body>
static int fs_run(FsCall& f, size_t* out_len, mk_fastq_select_t* st, Body&& body) {
  mk_ctx* c = f.c;
  MK_REFUSE_SPOILED(c, f.what);
  if (c->in_chunk) { c->err = std::string(f.what) + ": a chunk is open"; return MK_ERR_STATE; }
  if (!out_len) { c->err = std::string(f.what) + ": out_len is NULL"; return MK_ERR_ARG; }
  *out_len = 0;
  if (f.which != 1 && f.which != 2) { c->err = std::string(f.what) + ": which must be 1 (the main output) or 2 (the orphans)"; return MK_ERR_ARG; }
  MK_HIP(hipSetDevice(c->device));
  MK_HIP(hipStreamSynchronize(c->stream));
  int rc = body();
  (void)hipStreamSynchronize(c->stream);
  if (rc != MK_OK) return rc;
  if (f.records != f.nrec) {
    c->err = std::string(f.what) + ": the text holds " + std::to_string(f.records) + " records, the caller announced " + std::to_string(f.nrec);
    return MK_ERR_RANGE;
  }
  if (f.bad_rc != MK_OK) {
    c->err = f.bad_msg;
    return f.bad_rc;
  }
  *out_len = f.bytes_out;
  if (f.bytes_out > f.out_cap) {
    c->err = std::string(f.what) + ": the output holds " + std::to_string(f.bytes_out) + " bytes, out has room for " + std::to_string(f.out_cap);
    return MK_ERR_RANGE;
  }
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
    const uint8_t* d_text = d_fastq;
    if ((uintptr_t)d_text & 15) {  // (the line passes and fl_load16 load 16 aligned bytes at a time)
      int rc = mk_buf_reserve(c, c->raw, n + 64);
      if (rc != MK_OK) return rc;
      const auto t1 = MkClock::now();
      MK_HIP(hipMemcpyAsync(c->raw.p, d_fastq, n, hipMemcpyDeviceToDevice, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      f.st.s_copy += mk_since(t1);
      d_text = (const uint8_t*)c->raw.p;
    }
    return fs_piece(f, d_text, n);
  });
}

extern "C" int mk_fastq_select_text(mk_ctx* c, const uint8_t* fastq, size_t n, size_t piece_bytes, const uint8_t* keep, const uint64_t* kept,
                                    size_t nrec, unsigned which, uint8_t* out, size_t out_cap, size_t* out_len, mk_fastq_select_t* st) {
  if (!c) return MK_ERR_ARG;
  if ((n && !fastq) || (out_cap && !out)) { c->err = "mk_fastq_select_text: NULL buffer"; return MK_ERR_ARG; }
  FsCall f(c, "mk_fastq_select_text", keep, (const u64*)kept, nrec, keep ? which : 1u, out, out_cap, false);
  return fs_run(f, out_len, st, [&]() -> int {
    if (!n) return MK_OK;
    // pieces end behind a line 4j once they hold `piece` bytes: the default and the limits of the screen calls
    size_t piece = piece_bytes ? piece_bytes : std::min(TL_DEFAULT_PIECE, std::max<size_t>(n + 2, 4096));
    piece = std::min(std::max(piece, 2 * ((size_t)c->k + 24)), TL_MAX_PIECE);
    std::vector<uint64_t> cuts(n / piece + 2, 0);
    size_t ncuts = 0;
    if (mk_fastq_cuts(fastq, n, piece, cuts.data(), cuts.size(), &ncuts) != MK_OK) {
      c->err = "mk_fastq_select_text: the line scanner failed (internal error)";
      return MK_ERR_STATE;
    }
    cuts.resize(ncuts);
    cuts.push_back(n);
    size_t at = 0;
    for (const uint64_t end : cuts) {
      const size_t len = (size_t)end - at;
      if (!len) continue;
      int rc = mk_buf_reserve(c, c->raw, len + 64);
      if (rc != MK_OK) return rc;
      const auto t1 = MkClock::now();
      MK_HIP(hipMemcpyAsync(c->raw.p, fastq + at, len, hipMemcpyHostToDevice, c->stream));
      MK_HIP(hipStreamSynchronize(c->stream));
      f.st.s_copy += mk_since(t1);
      if ((rc = fs_piece(f, (const uint8_t*)c->raw.p, len)) != MK_OK) return rc;
      at = (size_t)end;
    }
    return MK_OK;
  });
}
