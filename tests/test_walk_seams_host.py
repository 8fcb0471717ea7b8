"""The seam text of tests/walk_seams.py places what it claims: every separator's stream position recomputed from the
reference's line loop (ref_records of tests/test_gpu_screen.py), then the coverage of the walk's seams.  No GPU."""
import re

import pytest

import walk_seams
from conftest import ROOT
from test_gpu_screen import ref_records


def test_units_are_the_sources():
    text = (ROOT / "mercat2_amd" / "csrc" / "mk_screenpiece.h").read_text()
    run = int(re.search(r"^#define SC_RUN (\d+)\s", text, flags=re.M).group(1))
    assert re.search(r"^#define SC_SPAN \(256 \* SC_RUN\)\s", text, flags=re.M)
    assert walk_seams.UNITS == (run, 64 * run, 256 * run) and walk_seams.TILE == 256 * run


@pytest.mark.parametrize("k", [5, 31])
def test_seam_coverage(k):
    text = walk_seams.seam_text(k)
    assert len(text) < 2_000_000 and text.startswith(b">")
    records = ref_records(text)
    assert records == walk_seams.seam_records(k)
    seps, total = walk_seams.separators(records)
    assert len(seps) == len(records) == text.count(b">")

    def instances(unit, d):
        """(front, behind) of every separator at m * unit + d, m * unit a true multiple inside the stream."""
        return [(front, behind) for pos, front, behind in seps
                if (pos - d) % unit == 0 and 1 <= (pos - d) // unit and (pos - d) < total and front is not None]

    for unit in walk_seams.UNITS:
        for d in walk_seams.shifts(k):
            found = instances(unit, d)
            assert any(front >= k + 1 and behind >= k + 1 for front, behind in found), (unit, d)
    # a record that ends inside the symbols that fill the key: shorter than k - 1, in front of a wave or tile seam
    for d in walk_seams.shifts(k):
        assert any(front < k - 1 for front, _ in instances(walk_seams.UNITS[1], d)), d
    for d in walk_seams.tile_short_shifts(k):
        assert any(front < k - 1 for front, _ in instances(walk_seams.TILE, d)), d
    assert any(front == 0 for _, front, _ in seps[1:])  # a header line behind a header line
    # one record over more than two whole tiles; 64 records or more of k .. k + 3 symbols in a row
    assert max(len(seq) for _, seq in records) > 3 * walk_seams.TILE
    run = best = 0
    for _, seq in records:
        run = run + 1 if k <= len(seq) <= k + 3 else 0
        best = max(best, run)
    assert best >= 64
    # the other text shares half of the long record, and only half
    long_seq = dict(records)["long"]
    assert ref_records(walk_seams.other_text(k))[1][1] == long_seq[:len(long_seq) // 2]
