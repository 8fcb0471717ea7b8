"""The seam texts of tests/span_seams.py place what they claim, and the Python restatement of the queue scatter's lane
arithmetic in tools/span_records_sim.py lists the records of its plain model.  No GPU."""
import importlib.util

import numpy as np
import pytest

import span_seams
from conftest import ROOT
from test_gpu_screen import ref_records


def load_sim():
    spec = importlib.util.spec_from_file_location("span_records_sim", ROOT / "tools" / "span_records_sim.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _valid(text, k):
    sym, bad = span_seams.stream_of(text)
    csum = np.concatenate(([0], np.cumsum(bad)))
    return (csum[k:] - csum[:-k]) == 0  # valid[p]: the window that starts at stream position p


@pytest.mark.parametrize("k", [31, 12])
def test_seam_texts_place_what_they_claim(k):
    texts = dict(span_seams.seam_texts(k))
    for name, text in texts.items():
        (_, seq), = ref_records(text)  # one record; the stream is its separator and its sequence
        sym, bad = span_seams.stream_of(text)
        assert len(sym) == 1 + len(seq) and bad[0] and int(bad.sum()) == 1 + seq.count("N")
    for windows in span_seams.SPANS_OF_WINDOWS:
        last = {d: int(np.flatnonzero(_valid(texts["w%d%+d" % (windows, d)], k))[-1]) for d in span_seams.SHIFTS}
        assert last == {d: windows + d - 1 for d in span_seams.SHIFTS}
        # the seam at `windows` is a thread's, a wave's and (the longer texts) a sub-tile's and, with three sub-tiles, a tile's
        assert windows % (span_seams.R * span_seams.WAVE) == 0
        assert (last[0] % 32, last[-1] % 32, last[1] % 32, last[31] % 32, last[33] % 32) == (31, 30, 0, 30, 0)
    assert span_seams.SPANS_OF_WINDOWS[1] == 3 * span_seams.R * span_seams.SUBT  # beyond thread 512, 1024 and up to 1536
    ends = []
    for at in span_seams.N_ENDS:
        valid = _valid(texts["N@%d" % at], k)
        gone = np.flatnonzero(~valid[1:]) + 1  # (window 0 holds the separator)
        assert gone.tolist() == list(range(at - k + 1, at + 1))
        assert valid[at + 1] and valid[at - k]
        ends.append((at % 32, (at // 32) % 64))
    # the last invalid window is window 31 of a thread (the next thread's window 0 is valid and is handed an invalid
    # window 31), window 0 of a thread, and window 0 of a wave's first thread
    assert [e[0] for e in ends] == [31, 0, 0] and ends[0][1] != 63 and ends[1][1] != 0 and ends[2][1] == 0
    assert _valid(texts["homopolymer"], k)[1:].all() and len(texts["homopolymer"]) == span_seams.HOMOPOLYMER + 4


def test_lane_arithmetic_lists_the_models_records():
    """tools/span_records_sim.py --check, on fewer reads: the hand-on word, the seeded cut and the hand-back of the
    restated kernel give the records of the model (runs cut at wave ends, capped from their true start)."""
    load_sim().check(120, 150, 1, ks=(31, 12))


@pytest.mark.parametrize("k", [31, 12])
def test_lane_arithmetic_on_the_seam_texts(k):
    sim = load_sim()
    for name, text in span_seams.seam_texts(k):
        if name.startswith("w%d" % span_seams.SPANS_OF_WINDOWS[1]) and not name.endswith("+0"):
            continue  # (one of the long texts is enough here)
        valid, minpos = sim.windows(*span_seams.stream_of(text), k)
        for span, cut in ((0, 32), (1, 2048)):
            assert sorted(sim.kernel_records(valid, minpos, 8, span)) == sorted(sim.model_records(valid, minpos, cut, 8)), (name, span)
