// mk_tableops.hip -- rows going INTO a running table from outside a chunk, and table-to-table operations: the imports
// of the multi-GPU merge (mk_import_pairs_device, mk_import_exotic; their exports are in mk_export.hip), mk_filter_min,
// mk_merge_from, mk_table_op.  Host code only.
#include "mk_tableview.h"  // setop_f
#include <cstring>

extern "C" int mk_import_pairs_device(mk_ctx* c, const uint64_t* d_keys, const uint64_t* d_counts, size_t rows) {
  if (!c) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_import_pairs_device");
  if (!rows) return MK_OK;
  MK_SETTLE(c);
  if (c->mode == MK_MODE_BYREF) { c->err = "mk_import_pairs_device: context has no packed table"; return MK_ERR_STATE; }
  MK_HIP(hipSetDevice(c->device));
  int rc;
  MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
  // (two-word keys: d_keys holds {hi, lo} per row; one-word keys: the all-ones key travels as an ordinary pair, anywhere
  // in the rows: the kernel sets it aside)
  if ((rc = mk_grow_run(c, rows)) != MK_OK) return rc;
  if ((rc = mk_launch_import_pairs(c, d_keys, d_counts, rows)) != MK_OK) return rc;
  if ((rc = mk_pull_info(c)) != MK_OK) return rc;
  mk_add_packed_rows(c, (size_t)c->h_info->new_rows);
  if (c->mode == MK_MODE_HASH64) c->run_side += c->h_info->side;
  return MK_OK;
}

extern "C" int mk_import_exotic(mk_ctx* c, const uint8_t* kmers, const uint64_t* counts, size_t rows) {
  if (!c) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_import_exotic");
  if (!rows) return MK_OK;
  if (!kmers || !counts) return MK_ERR_ARG;
  MK_HIP(hipSetDevice(c->device));
  MK_SETTLE(c);
  int rc;
  const size_t k = (size_t)c->k;
  if ((rc = mk_buf_reserve(c, c->ex_keys2, rows * k + 64)) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, c->ex_cnts2, rows * 8 + 64)) != MK_OK) return rc;
  MK_HIP(hipMemcpyAsync(c->ex_keys2.p, kmers, rows * k, hipMemcpyHostToDevice, c->stream));
  MK_HIP(hipMemcpyAsync(c->ex_cnts2.p, counts, rows * 8, hipMemcpyHostToDevice, c->stream));
  MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
  if ((rc = mk_grow_run_ref(c, c->run_ref_rows + rows)) != MK_OK) return rc;
  if ((rc = mk_launch_import_ref(c, (const uint8_t*)c->ex_keys2.p, (const uint64_t*)c->ex_cnts2.p, rows)) != MK_OK) return rc;
  if ((rc = mk_pull_info(c)) != MK_OK) return rc;
  c->run_ref_rows += (size_t)c->h_info->new_rows_ref;
  return MK_OK;
}

// Drop every row of the running table whose count is below min_count: the filter of a sample that is ONE
// chunk but was counted in pieces (record ranges on several GPUs, unfiltered) and merged
// (lib/mercat2_kmers.py:73-76 applies it once per file).
extern "C" int mk_filter_min(mk_ctx* c, uint64_t min_count) {
  if (!c) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(c, "mk_filter_min");
  MK_SETTLE(c);
  if (c->in_chunk) { c->err = "mk_filter_min: a chunk is open"; return MK_ERR_STATE; }
  if (min_count <= 1) return MK_OK;
  MK_HIP(hipSetDevice(c->device));
  int rc;
  size_t kept = 0;
  if (c->mode == MK_MODE_DENSE) {
    if ((rc = mk_launch_refilter_dense(c, (uint64_t*)c->run.p, c->run_slots, min_count)) != MK_OK) return rc;
  } else if (c->mode == MK_MODE_HASH64 && c->run_slots) {
    if ((rc = mk_rebuild_table(c, MK_TABLE_ONE, c->run_slots, min_count, &kept)) != MK_OK) return rc;
    c->run_rows = kept;
    if (c->run_side < min_count) c->run_side = 0;
  } else if (c->mode == MK_MODE_HASH128 && c->run128_slots) {
    if ((rc = mk_rebuild_table(c, MK_TABLE_TWO, c->run128_slots, min_count, &kept)) != MK_OK) return rc;
    c->run128_rows = kept;
  }
  if (c->run_ref_rows) {  // rows kept as text (few): through the host
    size_t n = 0;
    if ((rc = mk_export_exotic(c, nullptr, nullptr, 0, &n)) != MK_OK) return rc;
    std::vector<uint8_t> km(n * (size_t)c->k + 1), km2;
    std::vector<uint64_t> cn(n + 1), cn2;
    if ((rc = mk_export_exotic(c, km.data(), cn.data(), n, &n)) != MK_OK) return rc;
    for (size_t i = 0; i < n; ++i)
      if (cn[i] >= min_count) {
        km2.insert(km2.end(), km.begin() + i * (size_t)c->k, km.begin() + (i + 1) * (size_t)c->k);
        cn2.push_back(cn[i]);
      }
    if ((rc = mk_clear_table(c, MK_TABLE_REF, c->run_ref.p, c->run_ref_slots)) != MK_OK) return rc;
    c->run_ref_rows = 0;
    if (!cn2.empty() && (rc = mk_import_exotic(c, km2.data(), cn2.data(), cn2.size())) != MK_OK) return rc;
  }
  MK_HIP(hipStreamSynchronize(c->stream));
  return MK_OK;
}

extern "C" int mk_merge_from(mk_ctx* dst, mk_ctx* src) {
  if (!dst || !src || dst == src) return MK_ERR_ARG;
  MK_REFUSE_SPOILED(dst, "mk_merge_from");
  if (src->spoiled) { dst->err = "mk_merge_from: the source context holds part of a refused chunk (mk_reset it first)"; return MK_ERR_STATE; }
  mk_ctx* c = dst;
  if (dst->device != src->device || dst->alphabet != src->alphabet || dst->k != src->k || dst->canonical != src->canonical) {
    c->err = "mk_merge_from: contexts differ in device, alphabet, k or canonical mode";
    return MK_ERR_ARG;
  }
  if (dst->in_chunk || src->in_chunk) { c->err = "mk_merge_from: a chunk is open"; return MK_ERR_STATE; }
  MK_HIP(hipSetDevice(dst->device));
  int rc;
  // both streams idle before one context's kernels touch the other's buffers (whatever the mode: the export of src
  // writes into dst's survivor buffers, which dst's own merge kernels may still be reading)
  if ((rc = mk_settle(src)) != MK_OK) { dst->err = src->err; return rc; }
  if ((rc = mk_settle(dst)) != MK_OK) return rc;
  MK_HIP(hipStreamSynchronize(src->stream));
  MK_HIP(hipStreamSynchronize(dst->stream));
  if (src->mode == MK_MODE_HASH64) {
    // table to table, on the device: no compaction, no sort (the rows' order does not matter for a sum)
    if (src->run_rows) {
      if ((rc = mk_grow_run64(dst, dst->run_rows + src->run_rows)) != MK_OK) return rc;
      MK_HIP(hipMemsetAsync(dst->info.p, 0, sizeof(MkChunkInfo), dst->stream));
      if ((rc = mk_launch_merge_table64(dst, (const MkSlot*)src->run.p, src->run_slots)) != MK_OK) return rc;
      if ((rc = mk_pull_info(dst)) != MK_OK) return rc;
      dst->run_rows += (size_t)dst->h_info->new_rows;
    }
    dst->run_side += src->run_side;
  } else if (src->mode == MK_MODE_DENSE || src->mode == MK_MODE_HASH128) {
    size_t cap = 0;
    if ((rc = mk_export_size(src, &cap)) != MK_OK) { dst->err = src->err; return rc; }
    cap += 1;
    if ((rc = mk_buf_reserve(dst, dst->surv_keys, cap * 8 * (size_t)mk_words_per_key(src) + 64)) != MK_OK) return rc;
    if ((rc = mk_buf_reserve(dst, dst->surv_cnts, cap * 8 + 64)) != MK_OK) return rc;
    size_t rows = 0;
    if ((rc = mk_export_pairs_device(src, (uint64_t*)dst->surv_keys.p, (uint64_t*)dst->surv_cnts.p, cap, &rows)) != MK_OK) {
      dst->err = src->err;
      return rc;
    }
    if (rows && (rc = mk_import_pairs_device(dst, (const uint64_t*)dst->surv_keys.p, (const uint64_t*)dst->surv_cnts.p, rows)) != MK_OK)
      return rc;
  }
  if (src->run_ref_rows) {
    size_t n = 0;
    if ((rc = mk_export_exotic(src, nullptr, nullptr, 0, &n)) != MK_OK) { dst->err = src->err; return rc; }
    std::vector<uint8_t> km(n * (size_t)src->k + 1);
    std::vector<uint64_t> cn(n + 1);
    if ((rc = mk_export_exotic(src, km.data(), cn.data(), n, &n)) != MK_OK) { dst->err = src->err; return rc; }
    if ((rc = mk_import_exotic(dst, km.data(), cn.data(), n)) != MK_OK) return rc;
  }
  return MK_OK;
}

// ------------------------------------------------------------------------------- two tables combined by key
extern "C" int mk_table_op(mk_ctx* dst, mk_ctx* a, mk_ctx* b, int op, uint64_t min_a, uint64_t min_b, mk_table_op_t* st) {
  const auto t0 = MkClock::now();
  if (!dst || !a || !b) return MK_ERR_ARG;
  mk_ctx* c = dst;
  if (dst == a || dst == b) { c->err = "mk_table_op: dst must be a third context"; return MK_ERR_ARG; }
  if (op < MK_OP_MIN || op > MK_OP_DIFF) { c->err = "mk_table_op: unknown op"; return MK_ERR_ARG; }
  if (!min_a || !min_b) { c->err = "mk_table_op: min_a and min_b are at least 1"; return MK_ERR_ARG; }
  for (const mk_ctx* o : {a, b})
    if (dst->device != o->device || dst->alphabet != o->alphabet || dst->k != o->k || dst->canonical != o->canonical) {
      c->err = "mk_table_op: contexts differ in device, alphabet, k or canonical mode";
      return MK_ERR_ARG;
    }
  if (dst->share_owner || dst->n_sharers) { c->err = "mk_table_op: dst shares or lends a table (mk_share_table)"; return MK_ERR_STATE; }
  if (dst->in_chunk) { c->err = "mk_table_op: a chunk is open in dst"; return MK_ERR_STATE; }
  int rc;
  bool fold;
  // the inputs as every read-only call opens them: not spoiled, no open chunk, made final, their streams drained
  for (mk_ctx* o : {a, b})
    if ((rc = lk_open(o, "mk_table_op", 0, &fold)) != MK_OK) { dst->err = o->err; return rc; }
  if ((rc = mk_reset(dst)) != MK_OK) return rc;
  const bool two = op == MK_OP_MAX || op == MK_OP_SUM;  // f(0, cb) != 0: b's own keys go in as well
  // Room in dst for every row the scans can add, BEFORE the launches: nothing grows under a kernel.  (One more than
  // the rows: a table with slots and no rows is still walked, and its sink wants a table.)
  const size_t packed = (size_t)a->run_rows + a->run128_rows + (two ? (size_t)b->run_rows + b->run128_rows : 0);
  const size_t text = a->run_ref_rows + (two ? b->run_ref_rows : 0);
  if ((rc = mk_grow_run(dst, packed + 1)) != MK_OK) return rc;
  if ((a->run_ref_slots || (two && b->run_ref_slots)) && (rc = mk_grow_run_ref(dst, text + 1)) != MK_OK) return rc;
  if ((rc = mk_buf_reserve(c, c->ex_tmp, 2 * MK_SO_WORDS * sizeof(u64))) != MK_OK) return rc;
  u64* d_out = (u64*)c->ex_tmp.p;
  MkTimed scan(c);
  u64 h[2 * MK_SO_WORDS] = {0}, slots = 0;
  double s_scan = 0;
  rc = [&]() -> int {
    int r;
    MK_HIP(hipMemsetAsync(d_out, 0, sizeof h, c->stream));
    MK_HIP(hipMemsetAsync(c->info.p, 0, sizeof(MkChunkInfo), c->stream));
    // (b is walked for the one-pass ops too, without a probe or an insert: rows_b is a figure of the call)
    if ((r = scan.begin()) != MK_OK ||
        (r = mk_launch_setop(dst, a, b, false, op, true, min_a, min_b, (uint64_t*)d_out, (uint64_t*)&slots)) != MK_OK ||
        (r = mk_launch_setop(dst, b, a, true, op, two, min_b, min_a, (uint64_t*)d_out, (uint64_t*)&slots)) != MK_OK ||
        (r = scan.end()) != MK_OK)
      return r;
    MK_HIP(hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if ((r = mk_pull_info(dst)) != MK_OK) return r;  // (the arena rows handed out; the stream is idle afterwards)
    return scan.add_to(s_scan);
  }();
  if (rc != MK_OK) { (void)hipStreamSynchronize(c->stream); (void)mk_reset(dst); return rc; }
  const u64* ht = h + MK_SO_WORDS;  // the rows kept as text
  if (c->h_info->new_rows_ref != ht[MK_SO_ROWS_OUT]) {
    (void)mk_reset(dst);
    c->err = "mk_table_op: the rows kept as text and their arena rows differ";
    return MK_ERR_STATE;
  }
  // the one key kept beside the one-word table (32 x 'T'): f of the two side counts, as mk_histo adds it
  u64 sa = 0, sb = 0, sf = 0;
  if (dst->mode == MK_MODE_HASH64) {
    sa = a->run_side >= min_a ? a->run_side : 0;
    sb = b->run_side >= min_b ? b->run_side : 0;
    sf = setop_f(op, sa, sb);
    dst->run_side = sf;
  }
  mk_add_packed_rows(dst, dst->mode == MK_MODE_DENSE ? 0 : (size_t)h[MK_SO_ROWS_OUT]);
  dst->run_ref_rows = (size_t)ht[MK_SO_ROWS_OUT];
  if (!st) return MK_OK;
  memset(st, 0, sizeof *st);
  st->rows_a = h[MK_SO_ROWS_A] + ht[MK_SO_ROWS_A] + (sa ? 1 : 0);
  st->rows_b = h[MK_SO_ROWS_B] + ht[MK_SO_ROWS_B] + (sb ? 1 : 0);
  st->both = h[MK_SO_BOTH] + ht[MK_SO_BOTH] + (sa && sb ? 1 : 0);
  st->packed_out = h[MK_SO_ROWS_OUT] + (sf ? 1 : 0);
  st->text_out = ht[MK_SO_ROWS_OUT];
  st->rows_out = st->packed_out + st->text_out;
  st->total_out = h[MK_SO_TOTAL_OUT] + ht[MK_SO_TOTAL_OUT] + sf;
  st->slots = slots;
  st->passes = two ? 2 : 1;
  st->op = op;
  st->s_scan = s_scan;
  st->s_total = mk_since(t0);
  return MK_OK;
}
