// mk_fqpiece.h -- what the calls that read a FASTQ text, judge every record by a scan kernel of their own and write the
// survivors, whole or cut, share: mk_fastq_qtrim_* (mk_qtrim.hip), mk_fastq_adapt_* (mk_adapt.hip), mk_fastq_overlap_*
// (mk_overlap.hip) and mk_fastq_dedup_* (mk_dedup.hip).  mk_fastq_qc_* (mk_qc.hip) takes the device side only.
//   device side   QtLine (a line's content seen through aligned 16-byte granules), qt_record (the lines of a record and
//                 its checks), fq_segments (the four segments of an emitted record from its span).
//   host side     FqCall<P> (the state of a call), fq_piece<P> (one piece: mk_fqindex.h's steps -- fs_index_open,
//                 fs_index_lines, fs_gather -- around P::scan, P::decide and the prefix sum), fq_run (fs_call, the check
//                 of the record count, fs_call_end, fs_out_room), fq_device_body / fq_text_body (the one piece of a
//                 device call over fs_aligned_text, the pieces of a text call over fs_piece_cuts).
// A policy P names what differs:
//   Opt, Status (device counters behind the FsStatus of a piece), Stats (the call's mk_fastq_*_t), Side (what the scan
//   kernel reads or writes beside the text), ROW (uint64 a row),
//   paired(o), kind(k) (the phrase of a failed check), scan(...), decide(...), add(stats, status); optionally ready(...)
//   (what a piece sets up once its records are counted: mk_dedup.hip's table).
#pragma once
#include "mk_fqindex.h"

#define QT_GROUP 16u
#define QT_PASS (QT_GROUP * 16u)

// A line's content [a, a + L) seen through aligned granules: pass p, lane j owns the 16 bytes at (a & ~15) + 256 p + 16 j,
// whose byte b is content index i0 + b.  A granule that holds no byte of the content is not loaded.
struct QtLine {
  u64 a, L;
  __device__ __forceinline__ unsigned passes() const { return (unsigned)(((a & 15) + L + QT_PASS - 1) / QT_PASS); }
  __device__ __forceinline__ long long i0(unsigned p, unsigned j) const { return (long long)p * QT_PASS + 16 * j - (long long)(a & 15); }
  __device__ __forceinline__ FsSeg load(const uint8_t* __restrict__ text, u64 n, unsigned p, unsigned j) const {
    const long long i = i0(p, j);
    if (i + 16 <= 0 || i >= (long long)L) {
      FsSeg s;
      s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0;
      s.len = 0;
      s.nlmask = 0;
      return s;
    }
    return fs_load(text, n, (a & ~(u64)15) + (u64)p * QT_PASS + 16 * j);
  }
};
#define QT_BYTE(c, b) (((c).w[(b) >> 2] >> (8 * ((b)&3))) & 0xFFu)

// The lines of record r and what the checks on them say: the contents of the sequence line [l1, l1 + ls) and of the
// quality line [l3, l3 + lq), one trailing '\r' taken off each.
struct QtRecord {
  u64 l0, l1, l2, l3, l4, ls, lq;
  bool has_nl;  // the last line ends in '\n'
  int fail;
};
__device__ __forceinline__ QtRecord qt_record(const uint8_t* __restrict__ text, const u64* __restrict__ line, size_t r) {
  QtRecord q;
  q.l0 = line[4 * r]; q.l1 = line[4 * r + 1]; q.l2 = line[4 * r + 2]; q.l3 = line[4 * r + 3]; q.l4 = line[4 * r + 4];
  q.ls = q.l2 - 1 - q.l1;
  const bool seq_cr = q.ls > 0 && text[q.l2 - 2] == 13u;
  q.ls -= seq_cr ? 1 : 0;
  q.has_nl = text[q.l4 - 1] == 10u;
  q.lq = q.l4 - (q.has_nl ? 1 : 0) - q.l3;
  const bool qual_cr = q.lq > 0 && text[q.l3 + q.lq - 1] == 13u;
  q.lq -= qual_cr ? 1 : 0;
  q.fail = text[q.l0] != '@' ? FS_AT : text[q.l2] != '+' ? FS_PLUS : q.ls != q.lq ? FS_LENGTH : -1;
  return q;
}

// The four segments of an emitted record whose span is [start, start + kept) of its L bases: whole = {record, -, -, -},
// cut = {header line, seq[span] '\n', plus line, qual[span] '\n'}; unused ones have length 0.  True for a cut record.
__device__ __forceinline__ bool fq_segments(const QtRecord& q, u64 L, u64 start, u64 kept, u64 s[4], u64 m[4]) {
  if (start == 0 && kept == L) {
    s[0] = q.l0 | (q.has_nl ? 0 : FS_FORCE);
    m[0] = q.l4 - q.l0 + (q.has_nl ? 0 : 1);
    return false;
  }
  s[0] = q.l0;
  m[0] = q.l1 - q.l0;
  s[1] = (q.l1 + start) | FS_FORCE;
  m[1] = kept + 1;
  s[2] = q.l2;
  m[2] = q.l3 - q.l2;
  s[3] = (q.l3 + start) | FS_FORCE;
  m[3] = kept + 1;
  return true;
}

// ------------------------------------------------------------------------------------------ host side
template <class P>
struct FqCall : FsPieces {
  mk_ctx* c;
  typename P::Opt o;
  uint8_t* keep;  // the caller's arrays (host memory for the text call, device memory for the device call), or nullptr
  u64* rows;
  uint8_t* out;
  size_t out_cap;
  bool device;
  typename P::Side side;
  uint8_t* own = nullptr;  // the piece's text where it is the call's own copy (c->raw), which a policy may patch; else nullptr
  MkDevBuf tiles, meta, scan_tmp, stage, side_buf;
  MkTimed index, scan, place, gather;
  typename P::Stats st{};
  size_t bytes_out = 0;  // of all pieces so far
  FqCall(mk_ctx* c_, const char* w, const typename P::Opt& o_, size_t lim, uint8_t* kp, u64* rw, uint8_t* ot, size_t oc, bool dev)
      : FsPieces{w, lim}, c(c_), o(o_), keep(kp), rows(rw), out(ot), out_cap(oc), device(dev), side{}, index(c_), scan(c_), place(c_),
        gather(c_) {}
  ~FqCall() {
    for (MkDevBuf* b : {&tiles, &meta, &scan_tmp, &stage, &side_buf}) buf_free(*b);
  }
};

// P::ready(f, d_text, n, nrec), where a policy has one: what it sets up once a piece's record count is known and before
// its kernels run (records f.records - nrec .. f.records - 1); an error ends the call.  A policy without one is not asked.
template <class P>
static auto fq_ready(FqCall<P>& f, const uint8_t* d_text, size_t n, size_t nrec, int) -> decltype(P::ready(f, d_text, n, nrec)) {
  return P::ready(f, d_text, n, nrec);
}
template <class P>
static int fq_ready(FqCall<P>&, const uint8_t*, size_t, size_t, long) { return MK_OK; }

// One piece of n > 0 bytes at d_text (device memory, 16-byte aligned, whole records -- whole pairs with paired -- but for
// what trails in the last piece).  Its records are added to f.records either way.  The stream is idle afterwards.
template <class P>
static int fq_piece(FqCall<P>& f, const uint8_t* d_text, size_t n) {
  typedef typename P::Status Status;
  constexpr size_t ROW = P::ROW;
  mk_ctx* c = f.c;
  int rc;
  static_assert(sizeof(Status) <= FS_OWN_MAX && sizeof(Status) % 8 == 0, "the status block of a policy");
  const Status zero{};
  FsIndex ix;
  if ((rc = fs_index_open(c, f.tiles, f.index, f.st.s_index, d_text, n, &zero, sizeof zero, ix)) != MK_OK) return rc;
  FsStatus* d_st = ix.d_st;
  Status* d_qs = (Status*)ix.d_own;
  const size_t nrec = ix.nrec;
  size_t first;
  f.st.lines += ix.lines;
  if (!f.take(ix, first)) return MK_OK;
  if ((rc = fq_ready(f, d_text, n, nrec, 0)) != MK_OK) return rc;

  // meta: line[4 nrec + 1] | seg_src[nseg + 1] | len[nseg + 1] | dst[nseg + 1] | rows[ROW nrec] | verdict[nrec] | keep[nrec]
  const size_t nseg = 4 * nrec, nidx = 4 * nrec;
  if ((rc = mk_buf_reserve(c, f.meta, (nidx + 1 + 3 * (nseg + 1) + ROW * nrec) * sizeof(u64) + 2 * nrec)) != MK_OK) return rc;
  u64* line = (u64*)f.meta.p;
  u64* seg_src = line + nidx + 1;
  u64* len = seg_src + nseg + 1;
  u64* dst = len + nseg + 1;
  u64* d_rows = dst + nseg + 1;
  uint8_t* d_verdict = (uint8_t*)(d_rows + ROW * nrec);
  uint8_t* d_keep = d_verdict + nrec;
  if (f.device && f.rows) d_rows = f.rows + ROW * first;
  if (f.device && f.keep) d_keep = f.keep + first;
  size_t tmp = 0;
  MK_HIP(rocprim::exclusive_scan((void*)nullptr, tmp, (const u64*)len, dst, 0ull, nseg + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = mk_buf_reserve(c, f.scan_tmp, tmp ? tmp : 16)) != MK_OK) return rc;

  if ((rc = fs_index_lines<false>(c, f.index, d_text, n, ix, line)) != MK_OK) return rc;
  if ((rc = f.scan.begin()) != MK_OK) return rc;
  P::scan(f, d_text, n, (const u64*)line, nrec, d_rows, d_verdict, d_st);
  MK_HIP(hipGetLastError());
  if ((rc = f.scan.end()) != MK_OK) return rc;
  if ((rc = f.place.begin()) != MK_OK) return rc;
  // (the lengths are only added up before the status below has been read: no address is made of them)
  P::decide(f, d_text, (const u64*)line, nrec, (const u64*)d_rows, (const uint8_t*)d_verdict, d_keep, seg_src, len, d_st, d_qs);
  MK_HIP(hipGetLastError());
  MK_HIP(rocprim::exclusive_scan(f.scan_tmp.p, tmp, (const u64*)len, dst, 0ull, nseg + 1, rocprim::plus<u64>(), c->stream));
  if ((rc = f.place.end()) != MK_OK) return rc;
  u64 piece_out = 0;
  struct { FsStatus s; Status q; } h;
  MK_HIP(hipMemcpyAsync(&h, d_st, sizeof h, hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipMemcpyAsync(&piece_out, dst + nseg, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  MK_HIP(hipStreamSynchronize(c->stream));
  if ((rc = f.index.add_to(f.st.s_index)) != MK_OK) return rc;
  if ((rc = f.scan.add_to(f.st.s_scan)) != MK_OK) return rc;
  if ((rc = f.place.add_to(f.st.s_place)) != MK_OK) return rc;
  if (f.failed(ix, first, h.s.bad, P::kind)) return MK_OK;
  if (piece_out > (u64)n + 1) {
    c->err = std::string(f.what) + ": the output of a piece is longer than its records (internal error)";
    return MK_ERR_STATE;
  }
  f.st.records_out += h.s.records_out;
  f.st.records_trimmed += h.s.records_trimmed;
  f.st.bases_out += h.s.bases_out;
  P::add(f.st, h.q);
  if (!f.device && (f.keep || f.rows)) {
    const auto t1 = MkClock::now();
    if (f.keep) MK_HIP(hipMemcpyAsync(f.keep + first, d_keep, nrec, hipMemcpyDeviceToHost, c->stream));
    if (f.rows) MK_HIP(hipMemcpyAsync(f.rows + ROW * first, d_rows, ROW * nrec * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    f.st.s_write += mk_since(t1);
  }
  return fs_gather(c, f.gather, f.stage, d_text, n, seg_src, dst, nseg, piece_out, f.out, f.out_cap, f.device, f.bytes_out, f.st.s_gather,
                   f.st.s_write);
}

// How both kinds of call check their arguments, open and end; pre(): what the call sets up on the device before the first
// piece; body(): the pieces; post(): what it copies back once the call is known to succeed.
template <class P, class Pre, class Body, class Post>
static int fq_run(FqCall<P>& f, size_t* out_len, size_t* nrec, typename P::Stats* st, Pre&& pre, Body&& body, Post&& post) {
  mk_ctx* c = f.c;
  int rc = fs_call(
      c, f.what,
      [&]() -> int {
        if (!out_len) { c->err = std::string(f.what) + ": out_len is NULL"; return MK_ERR_ARG; }
        *out_len = 0;
        if (nrec) *nrec = 0;
        return MK_OK;
      },
      [&]() -> int {
        const int r = pre();
        return r != MK_OK ? r : body();
      });
  if (rc != MK_OK) return rc;
  if (nrec) *nrec = f.records;
  if (f.records > f.limit) {
    c->err = std::string(f.what) + ": the text holds " + std::to_string(f.records) + " records, keep and rows have room for " +
             std::to_string(f.limit);
    return MK_ERR_RANGE;
  }
  if ((rc = fs_call_end(c, f.what, f.records, P::paired(f.o), f.bad_rc, f.bad_msg)) != MK_OK) return rc;
  if ((rc = post()) != MK_OK) return rc;
  *out_len = f.bytes_out;
  f.st.records = f.records;
  f.st.bytes_out = f.bytes_out;
  if (st) *st = f.st;
  return fs_out_room(c, f.what, f.bytes_out, f.out_cap);
}

// The one piece of a device call: the text where it stands or its aligned copy (own_copy: the call patches its text).
template <class P>
static int fq_device_body(FqCall<P>& f, const uint8_t* d_fastq, size_t n, bool own_copy = false) {
  if (!n) return MK_OK;
  const uint8_t* d_text;
  int rc = fs_aligned_text(f.c, d_fastq, n, own_copy, f.st.s_copy, &d_text);
  if (rc != MK_OK) return rc;
  if (d_text != d_fastq) f.own = (uint8_t*)f.c->raw.p;
  return fq_piece(f, d_text, n);
}

// The pieces of a text call (fs_piece_cuts), each uploaded to c->raw.
template <class P>
static int fq_text_body(FqCall<P>& f, const uint8_t* fastq, size_t n, size_t piece_bytes) {
  mk_ctx* c = f.c;
  if (!n) return MK_OK;
  std::vector<uint64_t> cuts;
  int rc = fs_piece_cuts(c, f.what, fastq, n, piece_bytes, P::paired(f.o), cuts);
  if (rc != MK_OK) return rc;
  size_t at = 0;
  for (const uint64_t end : cuts) {
    const size_t len = (size_t)end - at;
    if (!len) continue;
    if ((rc = fs_upload_raw(c, fastq + at, len, f.st.s_copy)) != MK_OK) return rc;
    f.own = (uint8_t*)c->raw.p;
    if ((rc = fq_piece(f, (const uint8_t*)c->raw.p, len)) != MK_OK) return rc;
    at = (size_t)end;
  }
  return MK_OK;
}
