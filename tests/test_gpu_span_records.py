"""Super-k-mer records that span analysis-thread boundaries (mk_sk_scatterq_k, MK_SK_SPAN).

The queue scatter of one-word keys (12 <= k <= 32) lets a run of windows that share their minimizer go on from one
analysis thread's 32 windows into the next thread's, inside a wave, instead of cutting it there; MK_SK_SPAN=0 keeps the
cut at every thread.  Any partition of the windows into records of one minimizer each gives the same counts: every table
here must be the C oracle's, with the switch on and off, and with it on the chunk must hold fewer records.
"""
import functools
import importlib.util

import pytest

import span_seams
from conftest import ROOT
from mercat2_amd import native
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPANS = ("1", "0")


@functools.lru_cache(maxsize=None)
def _payload():
    data = native.synth_reads(300_000, 5, 70_000, 150, 6).tobytes()
    low = b">poly\n" + b"A" * 20_000 + b"\n>n\n" + (b"ACGTTGCAAGGCTTAACGGATCCATGCAAGTCCN" * 1500) + b"\n"
    return data + low


@functools.lru_cache(maxsize=None)
def _want(k, c, canon):
    from oracle import c_oracle
    if not canon:
        return c_oracle.count_dict(_payload(), k, c)
    folded = cpu_ref.canonical_fold(c_oracle.count_dict(_payload(), k, 0))  # min(key, reverse complement)
    return {key: n for key, n in folded.items() if n >= c}


def _count(data, k, c, canon=False, chunks=1):
    with native.Counter(k, native.ALPHABET_NT2, canonical=canon) as ctx:
        for _ in range(chunks):
            ctx.count_chunk(data, c)
        return ctx.to_dict(), ctx.stats()


@pytest.mark.parametrize("k,c,canon", [(31, 1, False), (21, 2, False), (12, 2, False), (32, 2, False), (32, 1, True),
                                       (14, 1, True), (18, 3, False)])
def test_same_tables_with_the_switch_on_and_off(monkeypatch, k, c, canon):
    """Reads, a poly-A record and a short repeat with an N in every copy: the oracle's table either way."""
    for span in SPANS:
        monkeypatch.setenv("MK_SK_SPAN", span)
        got, _ = _count(_payload(), k, c, canon)
        assert got == _want(k, c, canon), (k, c, canon, span)


@functools.lru_cache(maxsize=None)
def _sim():
    spec = importlib.util.spec_from_file_location("span_records_sim", ROOT / "tools" / "span_records_sim.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("subt", ["2", "3"])
@pytest.mark.parametrize("k", [31, 12])
def test_runs_end_at_every_seam(monkeypatch, k, subt):
    """The texts of tests/span_seams.py (tests/test_span_seams_host.py checks what they place): the last run ends at,
    before and behind a thread seam that is also a wave seam and, in the longer texts, a sub-tile and a tile seam of
    both shapes; an invalid stretch ends at window 31 of a thread, at window 0 of the next and at window 0 of a wave's
    first thread; a homopolymer.  The oracle's table, and exactly as many records as the restated lane arithmetic of
    tools/span_records_sim.py lists for the same stream (a wave whose records do not fit its queue walks, un-spanned:
    most waves at k = 12), so that restatement cannot drift from the kernel unnoticed."""
    from oracle import c_oracle
    monkeypatch.setenv("MK_SKQ_SUBT", subt)
    for name, text in span_seams.seam_texts(k):
        want, records = c_oracle.count_dict(text, k, 1), {}
        valid, minpos = _sim().windows(*span_seams.stream_of(text), k)
        for span in SPANS:
            monkeypatch.setenv("MK_SK_SPAN", span)
            got, st = _count(text, k, 1)
            assert got == want, (k, subt, name, span)
            records[span] = st["records"]
            listed = len(_sim().kernel_records(valid, minpos, 8, int(span), qcap=376 if subt == "3" else 512))
            print("k=%d subt=%s %s MK_SK_SPAN=%s: records %d, restated %d" % (k, subt, name, span, st["records"], listed))
            assert st["records"] == listed, (k, subt, name, span)
        assert records["1"] <= records["0"], (k, subt, name, records)


MIXED = [{"MK_SKQ_CAP": "0"}, {"MK_SKQ_CAP": "300"}, {}] + \
        [{"MK_NKMAX": n, "MK_SAMPLE_MIN": "0"} for n in ("1", "3", "5", "12", "31")] + \
        [{"MK_SAMPLE_MIN": "1"}, {"MK_SAMPLE_MIN": "1", "MK_XSEG": "0"}]


@pytest.mark.parametrize("env", MIXED, ids=["-".join("%s=%s" % kv for kv in e.items()) or "product" for e in MIXED])
@pytest.mark.parametrize("k,c", [(21, 2), (31, 1)])
def test_walking_waves_next_to_spanning_ones(monkeypatch, k, c, env):
    """Queues cut down so that some or all waves walk their runs thread by thread (un-spanned), other record length
    limits, sampled bucket sizes with nine regions and with one: same tables, and no more exact second partitions
    with the switch on than off (the histogram counts the un-spanned records: an upper bound per bucket)."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    retries = {}
    for span in SPANS:
        monkeypatch.setenv("MK_SK_SPAN", span)
        got, st = _count(_payload(), k, c)
        assert got == _want(k, c, False), (k, c, env, span)
        retries[span] = st["part_retries"]
    assert retries["1"] <= retries["0"], (k, c, env, retries)


# records / windows of the chunk below as the commit before the switch partitions it (measured on an MI355X, three runs
# alike: 2 298 764 records, 12 000 000 windows; with the switch on 2 097 462, 0.9124 of them)
PARENT_RECORDS_PER_WINDOW = 2_298_764 / 12_000_000


def test_the_records_really_went_away(monkeypatch):
    """Not a timing: the chunk holds the same windows in at most 0.94 times the records (the CPU model,
    tools/span_records_sim.py, says 0.913; wave seams and a small input's walked waves take the rest), and with the
    switch off the records are the ones the scatter listed before it had the switch."""
    data = native.synth_reads(1_000_000, 3, 100_000, 150, 4).tobytes()
    st = {}
    for span in SPANS:
        monkeypatch.setenv("MK_SK_SPAN", span)
        with native.Counter(31, native.ALPHABET_NT2) as ctx:
            ctx.count_chunk(data, 1)
            st[span] = ctx.stats()
        print("MK_SK_SPAN=%s: windows %d records %d retries %d" % (span, st[span]["windows"], st[span]["records"], st[span]["part_retries"]))
    assert st["1"]["windows"] == st["0"]["windows"] > 0
    assert st["1"]["records"] <= 0.94 * st["0"]["records"], (st["1"]["records"], st["0"]["records"])
    off = st["0"]["records"] / st["0"]["windows"]
    assert abs(off - PARENT_RECORDS_PER_WINDOW) <= 0.005 * PARENT_RECORDS_PER_WINDOW, (off, PARENT_RECORDS_PER_WINDOW)


def test_three_equal_chunks_inherit_regions_from_spanning_chunks(monkeypatch):
    """The hints of the second and third chunk come from a chunk that spanned, and they inherit its regions."""
    monkeypatch.setenv("MK_SK_SPAN", "1")
    got, st = _count(_payload(), 31, 1, chunks=3)
    assert got == {key: 3 * n for key, n in _want(31, 1, False).items()}
    assert st["part_reused"] >= 1, st["part_reused"]
