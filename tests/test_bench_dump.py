"""bench.py --dump-outputs on the CPU: dump_outputs given export buffers as a timed step leaves them (sorted rows of every
owner at the head of a larger buffer) writes them exactly, within the size limit, and samples the same rows every time."""
import numpy as np
import pytest
import torch

import bench


def _owners(words, rows_per_owner, seed=1):
    """Export buffers of owners holding ascending key ranges: (keys, counts, rows) with junk past the rows."""
    rng = np.random.default_rng(seed)
    total = sum(rows_per_owner)
    keys = np.sort(rng.choice(1 << 62, size=total * words, replace=False)).reshape(total, words).astype(np.int64)
    keys[:, 0] |= np.int64(1 << 62)  # high bits set: the split into 32-bit halves must keep them
    counts = rng.integers(1, 1 << 32, size=total, dtype=np.int64)
    parts, first = [], 0
    for r in rows_per_owner:
        k = torch.full(((r + 5) * words,), -1, dtype=torch.int64)
        c = torch.full((r + 5,), -1, dtype=torch.int64)
        k[: r * words] = torch.from_numpy(keys[first:first + r].reshape(-1))
        c[:r] = torch.from_numpy(counts[first:first + r])
        parts.append((k, c, r))
        first += r
    return parts, keys.view(np.uint64), counts


def _join(halves):
    return (halves[:, 0::2].astype(np.uint64) << np.uint64(32)) | halves[:, 1::2].astype(np.uint64)


def _load(d, name):
    a = np.load(d / (name + ".npy"))
    assert a.dtype == np.float64
    return a


@pytest.mark.parametrize("words", [1, 2])
def test_whole_table_is_written_exactly(tmp_path, words):
    parts, keys, counts = _owners(words, [300, 0, 211])
    n = bench.dump_outputs(str(tmp_path), parts, words)
    assert n == 511
    assert np.array_equal(_join(_load(tmp_path, "keys")), keys)
    assert np.array_equal(_load(tmp_path, "counts"), counts.astype(np.float64))
    assert _load(tmp_path, "summary").tolist() == [511, float(counts.sum())]
    assert not (tmp_path / "index.npy").exists()


@pytest.mark.parametrize("words", [1, 2])
def test_large_table_is_a_fixed_sample_within_the_limit(tmp_path, words):
    parts, keys, counts = _owners(words, [5000, 7000])
    budget = 40_000
    runs = []
    for i in range(2):
        d = tmp_path / str(i)
        n = bench.dump_outputs(str(d), parts, words, budget=budget, suffix="_rank3")
        assert 0 < n < 12000
        assert sum(f.stat().st_size for f in d.iterdir()) <= budget
        idx = _load(d, "index_rank3").astype(np.int64)
        assert idx.shape == (n,) and np.all(np.diff(idx) > 0) and idx[-1] < 12000
        assert np.array_equal(_join(_load(d, "keys_rank3")), keys[idx])
        assert np.array_equal(_load(d, "counts_rank3"), counts[idx].astype(np.float64))
        assert _load(d, "summary_rank3").tolist() == [12000, float(counts.sum())]
        runs.append(idx)
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.gpu
def test_bench_dumps_the_table_of_its_last_step(tmp_path):
    """bench.py itself on a small sample (one chunk): the dumped table is the table a Counter makes of the same reads."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from mercat2_amd import native
    genome, reads = 1_000_000, 200_000
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MK_BENCH_EXTRA")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--reads", str(reads),
                        "--genome", str(genome), "--no-cpu", "--no-file-leg", "--no-configs", "--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    # a plain run (no --full) measures nothing after its timed steps
    assert line["full"] is False and "verified_rows" not in line and "measured_stream_copy" not in line["roofline"]
    data = native.synth_reads(genome, bench.GENOME_SEED, reads, bench.READ_LEN, bench.READ_SEED).tobytes()
    with native.Counter(bench.K, native.ALPHABET_NT2, device=0) as ctx:
        ctx.count_chunk(data, bench.MIN_COUNT)
        kmers, counts = ctx.export()
    assert line["rows"] == counts.shape[0] > 0
    codes = np.zeros(256, dtype=np.uint64)
    codes[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint64)
    want = np.zeros(counts.shape[0], dtype=np.uint64)
    for j in range(bench.K):  # one-word keys: 2 bits per base, the first base in the highest bits
        want = (want << np.uint64(2)) | codes[kmers[:, j]]
    assert np.array_equal(_join(_load(tmp_path, "keys")), want[:, None])
    assert np.array_equal(_load(tmp_path, "counts"), counts.astype(np.float64))
    assert _load(tmp_path, "summary").tolist() == [counts.shape[0], float(counts.sum())]
