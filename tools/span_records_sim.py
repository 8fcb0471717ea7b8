#!/usr/bin/env python3
"""CPU model of the super-k-mer records the queue scatter (mk_sk_scatterq_k) writes, by where runs are cut.

A run = consecutive valid windows whose minimizer (the 11-mer with the smallest order hash, leftmost on ties) sits
at the same place.  The scatter cuts a run into records of at most `cap` windows, counted from the run's start, and
besides at every multiple of `cut` windows of the symbol stream: 32 = at every analysis thread (MK_SK_SPAN=0),
2048 = at wave ends only (MK_SK_SPAN=1), 0 = never.

  python tools/span_records_sim.py            the table of profiles/span_records.md (20 000 random reads of 150 bp)
  python tools/span_records_sim.py --check    (and tests/test_span_seams_host.py, on fewer reads) also replays the kernel's own lane arithmetic (sk_span_out, sk_span_in,
                                              sk_cut_starts with a seed, the hand-back of `ext`) on the same stream,
                                              for several k and caps, and compares it record for record with the model
"""
import argparse

import numpy as np

M = 11
R = 32


def stream(reads, length, seed):
    """Symbols 0..3 and a bad flag per symbol: `reads` random reads, one separator (bad) after each."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 4, size=(reads, length + 1), dtype=np.int64)
    bad = np.zeros((reads, length + 1), dtype=bool)
    bad[:, length] = True
    sym[:, length] = 0
    return sym.ravel(), bad.ravel()


def windows(sym, bad, k):
    """valid[p], minpos[p] (absolute position of window p's minimizer) for every window start p."""
    n = sym.size
    w = k - M + 1
    mm = np.zeros(n - M + 1, dtype=np.int64)
    for i in range(M):
        mm = (mm << 2) | sym[i:n - M + 1 + i]
    order = (mm * 0x9277B5 + 0x2C5A3D) & ((1 << 22) - 1)  # sk_order_hash: a bijection of the 11-mer
    nwin = n - k + 1
    best = order[:nwin].copy()
    for i in range(1, w):
        np.minimum(best, order[i:nwin + i], out=best)
    rel = np.zeros(nwin, dtype=np.int64)  # leftmost candidate that has the smallest hash
    found = np.zeros(nwin, dtype=bool)
    for i in range(w):
        hit = ~found & (order[i:nwin + i] == best)
        rel[hit] = i
        found |= hit
    minpos = np.arange(nwin) + rel
    csum = np.concatenate(([0], np.cumsum(bad)))
    valid = (csum[k:k + nwin] - csum[:nwin]) == 0
    return valid, minpos


def model_records(valid, minpos, cut, cap):
    """(start, windows) of every record: runs cut at multiples of `cut` (0: never), then every `cap` from the piece's start."""
    n = valid.size
    start = valid.copy()
    start[1:] &= ~(valid[:-1] & (minpos[1:] == minpos[:-1]))
    if cut:
        start[::cut] |= valid[::cut]
    out = []
    idx = np.flatnonzero(start)
    ends = np.flatnonzero(~valid)
    for a, nxt in zip(idx, np.append(idx[1:], n)):
        j = np.searchsorted(ends, a)
        b = min(nxt, ends[j] if j < ends.size else n)
        while a < b:
            t = min(cap, b - a)
            out.append((a, t))
            a += t
    return out


# ---- the kernel's arithmetic, lane by lane (32-bit masks as Python ints)
def cut_starts(starts, valid, nkmax, seed=0):
    if nkmax >= R:
        return starts | seed
    cont = valid & ~starts & 0xFFFFFFFF
    a, ln = cont, 1
    while 2 * ln <= nkmax:
        a &= a << ln
        ln *= 2
    if ln < nkmax:
        a &= a << (nkmax - ln)
    a &= 0xFFFFFFFF
    s2 = starts | seed
    c = (s2 << nkmax) & a
    while c:
        s2 |= c
        c = (c << nkmax) & a
    return s2


def ffs0(x):
    return (x & -x).bit_length() - 1


def kernel_records(valid, minpos, nkmax, span, wave=64, qcap=1 << 30):
    """(start, windows) of every record as mk_sk_scatterq_k lists them.  qcap: a wave whose spanned records do not fit
    its queue walks its threads' own, un-spanned runs instead (376 items with three sub-tiles, 512 with two)."""
    n = valid.size
    nthr = (n + R - 1) // R
    recip = 65535 // nkmax + 1
    out = []
    lanes = []
    for t in range(nthr):
        p0 = t * R
        v = s = 0
        pos = [0] * R
        prev = 64
        for j in range(R):
            p = p0 + j
            ok = p < n and bool(valid[p])
            best = int(minpos[p]) - p0 if p < n else 0
            pos[j] = best & 63
            if ok and pos[j] != prev:
                s |= 1 << j
            if ok:
                v |= 1 << j
            prev = pos[j] if ok else 64
        lanes.append((v, s, pos))
    for w0 in range(0, nthr, wave):
        ws = lanes[w0:w0 + wave]
        s2s, mine = [], []
        for i, (v, s, pos) in enumerate(ws):
            st2, seed = s, 0
            if span and i > 0:
                pv, ps, ppos = ws[i - 1]
                clz = 32 - ps.bit_length()
                inn = (pv >> 31) | (ppos[31] << 1) | ((clz + 1) << 7)
                ends = (s & ~1 | ~v) & 0xFFFFFFFF
                if (inn & 1) and (v & 1) and ends and pos[0] + R == ((inn >> 1) & 63):
                    st2 &= ~1
                    c = inn >> 7
                    phase = c - ((c * recip) >> 16) * nkmax
                    assert phase == c % nkmax
                    j0 = nkmax - phase if phase else 0
                    seed = (1 << j0) if j0 < ffs0(ends) else 0
            s2 = cut_starts(st2, v, nkmax, seed)
            s2s.append(s2)
            mine.append(ffs0((s2 | ~v) & 0xFFFFFFFF) if (s & ~st2 & 1) else 0)
        if sum(bin(x).count("1") for x in s2s) > qcap:  # the walking fallback, taken by the whole wave
            s2s, mine = [cut_starts(s, v, nkmax) for v, s, _ in ws], [0] * len(ws)
        for i, (v, s, pos) in enumerate(ws):
            ext = mine[i + 1] if i + 1 < len(ws) else 0
            todo = s2s[i]
            while todo:
                j = ffs0(todo)
                todo &= todo - 1
                stop = (s2s[i] | ~v) & ~((2 << j) - 1) & 0xFFFFFFFF
                nk = (ffs0(stop) if stop else R + ext) - j
                assert 1 <= nk <= nkmax, (nk, nkmax)
                out.append(((w0 + i) * R + j, nk))
    return out


def table(k, cap, reads, length, seed):
    sym, bad = stream(reads, length, seed)
    valid, minpos = windows(sym, bad, k)
    nwin = int(valid.sum())
    print("k = %d, cap %d, %d reads of %d bp: %d windows" % (k, cap, reads, length, nwin))
    print("| cuts | records | windows / record | records at the cap |")
    print("|---|---|---|---|")
    for name, cut in (("every 32 windows (MK_SK_SPAN=0)", 32), ("every 2048 windows (wave ends only, MK_SK_SPAN=1)", 2048), ("never", 0)):
        recs = model_records(valid, minpos, cut, cap)
        assert sum(t for _, t in recs) == nwin
        full = sum(1 for _, t in recs if t == cap)
        print("| %s | %d | %.2f | %.1f %% |" % (name, len(recs), nwin / len(recs), 100.0 * full / len(recs)))


def check(reads, length, seed, ks=(31, 12, 21, 32)):
    for k in ks:
        sym, bad = stream(reads, length, seed)
        sym[5000:9000] = 0  # a homopolymer
        sym[12000:12000 + 34 * 40] = np.tile(sym[100:134], 40)  # a short repeat
        valid, minpos = windows(sym, bad, k)
        for cap in (1, 3, 5, 8, 12, 31):
            if cap > 62 - k:
                continue
            for span, cut in ((0, 32), (1, 2048)):
                got = sorted(kernel_records(valid, minpos, cap, span))
                want = sorted(model_records(valid, minpos, cut, cap))
                assert got == want, (k, cap, span, len(got), len(want))
        print("k = %d: the lane arithmetic lists the model's records, span on and off" % k)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--cap", type=int, default=8)
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    table(a.k, a.cap, a.reads, a.length, a.seed)
    if a.check:
        check(400, a.length, a.seed)
