"""Counting runs that push the running table where the host's sizing guess is wrong: a sample whose chunks alternate
between low and high diversity, so that the table sized before a fused launch (mk_chunk.hip process_chunk_fast, from the
chunk before) fills up during it and the count kernel spills (mk_skcount.hip) -- without MK_FUSE_MAX_PROBE -- and the
same chunks over one table shared by several contexts, each driven by its own thread; and S2e at full chunk size
(100 MiB chunks with 1 % substitutions at -c 1: the non-fused region import, buckets that overflow the count kernels'
LDS tables into sub-range passes, and tens of millions of rows in the running table).

The reference is oracle/packed_ref: a numpy counter over the packed windows of the synthetic reads, each chunk filtered
on its own and the tables summed (what cpu_ref.merge_counts does with the oracle's dicts; tests/test_packed_ref.py pins
it to the C oracle).  The C oracle itself is too slow for tens of millions of windows."""
import functools
import os
import threading

import numpy as np
import pytest

from mercat2_amd import native
from oracle import packed_ref as pr

pytestmark = pytest.mark.gpu

READS = 133_000   # per low chunk, 150 bp: ~21 MB of text, 16 M windows
HIGH_READS = 138_000  # 4 % more: a high chunk does not inherit the bucket regions of the low chunk before it (mk_part_inherit
                      # takes -2 %..+1 %), whose regions it would overflow -- the exact second pass is never fused
LOW_GENOME = 50_000
HIGH_GENOME = 1_000_000  # ~20x coverage: ~1 M survivors, 122 a bucket -- below the 360 that keep the NEXT chunk fused


@functools.lru_cache(maxsize=None)
def chunk_text(kind: str, i: int) -> bytes:
    """Low-diversity chunks: reads of one 50 kbp genome; high-diversity chunks: reads of a 1 Mbp genome of their own.
    Every chunk is a full chunk for the host's hints (at least 3/4 of the one before)."""
    if kind == "L":
        return native.synth_reads(LOW_GENOME, 500, READS, 150, 600 + i, 0, i * READS).tobytes()
    return native.synth_reads(HIGH_GENOME, 700 + i, HIGH_READS, 150, 800 + i, 0, i * HIGH_READS).tobytes()


@functools.lru_cache(maxsize=None)
def chunk_table(kind: str, i: int, k: int, canonical: bool):
    """One chunk's unfiltered table (the filter is applied by the caller)."""
    return pr.count_chunk(chunk_text(kind, i), k, 1, canonical)


def sample_reference(chunks, k, c, canonical):
    parts = []
    for kind, i in chunks:
        keys, counts = chunk_table(kind, i, k, canonical)
        keep = counts >= np.uint64(c)
        parts.append(([w[keep] for w in keys], counts[keep]))
    return pr.merge_tables(parts)


def check(ctx, k, ref):
    keys, counts = ref
    got_k, got_c = ctx.export()
    assert got_k.shape[0] == counts.size, (got_k.shape[0], counts.size)
    assert np.array_equal(got_c, counts)
    assert np.array_equal(got_k, pr.as_text(keys, k))


def device_rows_sorted(ctx):
    """The table's packed rows as mk_export_pairs_device leaves them in HBM, put in key order on the GPU (torch sorts;
    an unsigned order is the signed order of the words with the top bit flipped): ([key words], counts) on the host."""
    import torch
    n, w = ctx.rows(), ctx.words_per_key()
    keys = torch.empty((n + 1) * w, dtype=torch.int64, device="cuda:0")
    cnts = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    assert ctx.export_pairs_device(keys.data_ptr(), cnts.data_ptr(), n + 1) == n
    keys = keys[:n * w].view(n, w)
    top = torch.tensor(-(1 << 63), dtype=torch.int64, device="cuda:0")
    order = None
    for col in reversed(range(w)):  # (least significant word first; stable sorts)
        kc = torch.bitwise_xor(keys[:, col] if order is None else keys[order, col], top)
        o = torch.sort(kc, stable=True)[1]
        order = o if order is None else order[o]
        del kc
    out = [keys[order, i].cpu().numpy().view(np.uint64) for i in range(w)]
    return out, cnts[:n][order].cpu().numpy().view(np.uint64)


SHIFT = [("L", 0), ("H", 0), ("L", 1), ("H", 1)]


@pytest.mark.parametrize("k,canonical", [(31, False), (31, True), (32, False)], ids=["k31", "k31canon", "k32"])
def test_diversity_shift_spills_without_the_switch(k, canonical):
    """Low, high, low, high: every high chunk comes after a chunk with ~50 k survivors, so its fused launch meets a table
    sized for a twentieth of what it brings and sets the rest aside (fuse_spilled > 0); the host imports the spill."""
    assert "MK_FUSE_MAX_PROBE" not in os.environ
    for c in (2, 3):
        with native.Counter(k, native.ALPHABET_NT2, device=0, canonical=canonical) as ctx:
            for kind, i in SHIFT:
                ctx.count_chunk(chunk_text(kind, i), c)
            st = ctx.stats()
            check(ctx, k, sample_reference(SHIFT, k, c, canonical))
        assert st["fused_chunks"] >= 2 and st["fuse_spilled"] > 0 and st["part_retries"] == 0, (c, st)


def _table(chunks, k=31, c=2):
    return sample_reference(chunks, k, c, False)


def test_shared_table_owner_too_small_then_taken():
    """Step by step, so that the table each chunk went to is known: a sharer whose fused launch finds the owner's table
    too small for what it expects upserts into its own (the owner's table is unchanged); after the owner has grown its
    table (a spilling high chunk), another sharer's fused launch goes into the owner's table (the owner's export holds
    that chunk's counts, the sharer's own table does not)."""
    k, c = 31, 2
    ctxs = [native.Counter(k, native.ALPHABET_NT2, device=0) for _ in range(3)]
    owner, s1, s2 = ctxs
    try:
        for s in (s1, s2):
            s.share_table(owner)
        owner.count_chunk(chunk_text("L", 0), c)     # (a new context: not fused; the table is sized for ~100 k rows)
        check(owner, k, _table([("L", 0)]))
        s1.count_chunk(chunk_text("L", 1), c)        # (not fused: its own table)
        # fused; it expects ~100 k new rows, the owner's 262 k slots hold 100 k already: too small -- its own table
        s1.count_chunk(chunk_text("H", 1), c)
        assert s1.stats()["fused_chunks"] == 1
        check(s1, k, _table([("L", 1), ("H", 1)]))
        check(owner, k, _table([("L", 0)]))
        owner.count_chunk(chunk_text("H", 0), c)     # fused, spills, the table grows to millions of slots
        st = owner.stats()
        assert st["fused_chunks"] == 1 and st["fuse_spilled"] > 0, st
        check(owner, k, _table([("L", 0), ("H", 0)]))
        s2.count_chunk(chunk_text("L", 1), c)        # (not fused: its own table)
        s2.count_chunk(chunk_text("L", 2), c)        # fused, ~100 k expected into ~2 M of 8 M slots: the owner's table
        assert s2.stats()["fused_chunks"] == 1
        check(owner, k, _table([("L", 0), ("H", 0), ("L", 2)]))
        check(s2, k, _table([("L", 1)]))
        for s in (s1, s2):
            owner.merge_from(s)
        check(owner, k, _table([("L", 0), ("H", 0), ("L", 1), ("H", 1), ("L", 1), ("L", 2)]))
    finally:
        for s in (s1, s2):
            s.share_table(None)
        for x in ctxs:
            x.close()


def test_shared_table_threads_and_resets():
    """The chunks dealt to three contexts of one GPU that share the first one's table (mk_share_table), each driven by its
    own thread, for three samples in a row with reset() between them: the owner takes an unfused first chunk and a
    spilling high chunk while the sharers run fused launches.  Which table each of those goes to depends on timing
    (test_shared_table_owner_too_small_then_taken pins both cases down); whatever it is, after each sample the merged
    table equals the reference, and every context's rows() equals the length of its own export (the export checks the
    row count it was told)."""
    k, c = 31, 2
    deal = [[("L", 0), ("H", 0)], [("L", 1), ("L", 2), ("H", 1)], [("H", 2), ("L", 0), ("H", 0)]]
    ref = sample_reference([x for d in deal for x in d], k, c, False)
    ctxs = [native.Counter(k, native.ALPHABET_NT2, device=0) for _ in range(3)]
    try:
        for s in ctxs[1:]:
            s.share_table(ctxs[0])
        for sample in range(3):
            lists = [deal[0]] + (deal[1:] if sample % 2 == 0 else deal[:0:-1])
            errors = []

            def drive(ctx, chunks):
                try:
                    for kind, i in chunks:
                        ctx.count_chunk(chunk_text(kind, i), c)
                except Exception as e:  # (re-raised in the main thread)
                    errors.append(e)

            threads = [threading.Thread(target=drive, args=(x, l_)) for x, l_ in zip(ctxs, lists)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            stats = [x.stats() for x in ctxs]
            for x in ctxs:
                kmers, counts = x.export()
                assert x.rows() == counts.size
            for x in ctxs[1:]:
                ctxs[0].merge_from(x)
            check(ctxs[0], k, ref)
            assert sum(st["fused_chunks"] for st in stats) >= 3, stats
            if sample == 0:
                assert stats[0]["fuse_spilled"] > 0, stats[0]
            for x in ctxs:  # (the owner first: its sharers count the next sample into the cleared table)
                x.reset()
                x.reset_stats()
    finally:
        for s in ctxs[1:]:
            s.share_table(None)
        for x in ctxs:
            x.close()


# ------------------------------------------------------------------------------------------------ S2e at full size
S2E_READS = (100 << 20) // 161  # 150 bp reads, ~161 bytes a record: 100 MiB chunks
S2E_GENOME = 100_000_000
SKC_TARGET = 8192 * 40 // 100   # mk_skcount.hip: LDS slots x SKC_TARGET_PCT -- keys a one-word bucket pass is planned for
SK2C_SLOTS = 6144               # mk_skmer2.hip: the two-word count kernel's LDS table


@pytest.mark.parametrize("k,lds_keys", [(31, SKC_TARGET), (63, SK2C_SLOTS)], ids=["k31", "k63"])
def test_s2e_full_size_chunks(k, lds_keys):
    """Two 100 MiB chunks of 150 bp reads with 1 % substitutions (S2e) at -c 1: nothing is fused (-c 1 hands every
    chunk's survivors over through their regions), a bucket holds more distinct keys on average than the count
    kernel's LDS table is planned for (sub-range passes), and the table of ~10^8 rows equals the reference bit for bit.
    (The reference takes one reduction over all windows: at -c 1 the per-chunk filter keeps every row.)"""
    texts = [native.synth_reads(S2E_GENOME, 31, S2E_READS, 150, 32 + i, 10_000, i * S2E_READS).tobytes() for i in range(2)]
    assert all(abs(len(t) - (100 << 20)) < (1 << 20) for t in texts)
    with native.Counter(k, native.ALPHABET_NT2, device=0) as ctx:
        for t in texts:
            ctx.count_chunk(t, 1)
        st = ctx.stats()
        assert st["chunks"] == 2 and st["fused_chunks"] == 0, st
        assert st["distinct"] / 8192 / 2 > lds_keys, st
        ref_k, ref_c = pr.count_sample_c1(texts, k)
        del texts
        assert ctx.rows() == ref_c.size > 100_000_000
        # every row, bit for bit: the packed keys and counts the device holds, in key order
        got_k, got_c = device_rows_sorted(ctx)
        assert all(np.array_equal(a, b) for a, b in zip(got_k, ref_k)) and np.array_equal(got_c, ref_c)
        del got_k, got_c
        # and the sorted text export of the same table: every count in its place, the text of one row in 997
        ek, ec = ctx.export()
        assert np.array_equal(ec, ref_c)
        at = np.arange(0, ref_c.size, 997)
        assert np.array_equal(ek[at], pr.as_text([w[at] for w in ref_k], k))
