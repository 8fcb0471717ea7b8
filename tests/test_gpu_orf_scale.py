"""The ORF calls (mk_orf_text / mk_orf_device) past the sizes at which their kernels change path: or_carry_k with two
and three tiles a thread, carries that cross hundreds of tiles, or_name_k / or_len_k lanes that take a second item,
gather workgroups that lie inside one ORF.  The texts and their thresholds are tests/orf_scale.py (checked without a
GPU in tests/test_orf_scale_host.py); every expectation is tests/orf_rule_np.py, the rule on numpy, computed once a
process.  Equality is exact everywhere: bytes, rows and every figure."""
import numpy as np
import pytest

import orf_scale as scale
from mercat2_amd import native

pytestmark = pytest.mark.gpu
FIGURES = ("records", "orfs", "bytes_out", "residues", "longest", "per_frame")


@pytest.fixture(scope="module")
def ctx():
    with native.Counter(5, native.ALPHABET_NT2) as c:
        yield c


def check(ctx, text: bytes, want, records: int, bases: int, piece_bytes: int = 0, **mode):
    """Counter.orfs at min_aa 1 against the expectation: bytes, rows and the figures."""
    info = {}
    out, rows = ctx.orfs(text, min_aa=1, piece_bytes=piece_bytes, info=info, **mode)
    w_out, w_rows = want
    assert rows.dtype == np.uint64 and rows.shape == w_rows.shape
    assert np.array_equal(rows, w_rows)
    assert out == w_out
    fig = scale.figures(records, w_out, w_rows)
    assert {key: info[key] for key in FIGURES} == fig
    assert info["bytes"] == len(text) and info["bases"] == bases and info["headless"] == 0
    if not piece_bytes:
        assert info["pieces"] == 1
    return info


def dense_bases(tiles: int) -> int:
    return (tiles - 1) * scale.SPAN + 100 - 3  # the stream without its two separators and the position behind its end


# ------------------------------------------------------------------------------------------ closings everywhere
@pytest.mark.parametrize("mode", scale.MODES, ids=lambda m: "-".join("%s=%s" % kv for kv in sorted(m.items())) or "stop")
def test_dense_two_tiles_a_thread_every_mode(ctx, mode):
    """CARRY_THREADS + 1 tiles: the serial fold, the prefix from the thread in front, the second walk, and threads
    without a tile."""
    tiles = scale.DENSE_TILES[1]
    assert scale.per_thread(tiles) == 2
    info = check(ctx, scale.dense(tiles), scale.dense_expected(tiles, **mode), 2, dense_bases(tiles), **mode)
    assert info["orfs"] > 10_000


@pytest.mark.parametrize("mode", [dict(), dict(start=True, alt_starts=True)], ids=["stop", "alt"])
@pytest.mark.parametrize("tiles", [scale.DENSE_TILES[0], scale.DENSE_TILES[2], scale.DENSE_TILES[3]])
def test_dense_one_two_and_three_tiles_a_thread(ctx, tiles, mode):
    check(ctx, scale.dense(tiles), scale.dense_expected(tiles, **mode), 2, dense_bases(tiles), **mode)


def test_dense_from_small_pieces(ctx):
    """piece_bytes far below the long record: its piece grows to hold it, and the result is the same."""
    tiles = scale.DENSE_TILES[1]
    info = check(ctx, scale.dense(tiles), scale.dense_expected(tiles), 2, dense_bases(tiles), piece_bytes=1 << 20)
    assert 1 <= info["pieces"] <= 2


# ------------------------------------------------------------------------------------------ carries that travel far
@pytest.mark.parametrize("variant", scale.FAR_VARIANTS)
@pytest.mark.parametrize("tiles", scale.FAR_TILES)
def test_far(ctx, tiles, variant):
    """Six stretches from tile 0 to the last tile; the first forward and the last reverse start hundreds of tiles in
    front of their closing; a start shut out by a later stop; the closings as stops in the last tile.  Every ORF has
    about a million residues, so all but a few gather workgroups lie inside one."""
    text = scale.far(tiles, variant)
    for mode in (dict(), dict(start=True)):
        info = check(ctx, text, scale.far_expected(tiles, variant, **mode), 1, scale.far_bases(tiles), **mode)
        if not mode or variant != "stops":
            assert info["longest"] > 2 * scale.GATHER_BYTES


def test_far_device_call(ctx):
    """mk_orf_device at two alignments of the text and an unaligned out, with sentinels around out and rows."""
    import torch
    tiles = scale.FAR_TILES[0]
    text = scale.far(tiles, "starts")
    for lead, mode in ((0, dict(start=True)), (5, dict(start=True)), (5, dict())):
        w_out, w_rows = scale.far_expected(tiles, "starts", **mode)
        no, nr = len(w_out), len(w_rows)
        out_lead = 16 + 3 + 4 * lead
        host = np.frombuffer(b"#" * lead + text + b"#" * 9, dtype=np.uint8).copy()
        d_text = torch.from_numpy(host).cuda()
        d_out = torch.full((out_lead + no + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rows = torch.full(((nr + 1) * 24,), 0xA5, dtype=torch.uint8, device="cuda")
        assert d_out.data_ptr() % 16 == 0 and d_rows.data_ptr() % 8 == 0 and out_lead % 16
        torch.cuda.synchronize()
        info = ctx.orfs_device(d_text.data_ptr() + lead, len(text), d_out.data_ptr() + out_lead, no, d_rows.data_ptr(), nr, min_aa=1, **mode)
        got = d_out.cpu().numpy()
        assert {key: info[key] for key in FIGURES} == scale.figures(1, w_out, w_rows) and info["pieces"] == 1
        assert got[out_lead:out_lead + no].tobytes() == w_out
        assert (got[:out_lead] == 0xA5).all() and (got[out_lead + no:] == 0xA5).all()  # the sentinels around out
        raw = d_rows.cpu().numpy()
        assert np.array_equal(native.orf_rows(raw[:nr * 24].view(native.ORF_ROW_DTYPE)), w_rows) and (raw[nr * 24:] == 0xA5).all()
        assert (d_text.cpu().numpy() == host).all()  # the input is unmodified


# ------------------------------------------------------------------------------------------ more items than lanes
def many_bases() -> int:
    whole, rest = divmod(scale.MANY_RECORDS, len(scale.MANY_POOL))
    return whole * sum(len(s) for _, s in scale.MANY_POOL) + sum(len(s) for _, s in scale.MANY_POOL[:rest])


def test_many_records_and_orfs_in_one_piece(ctx):
    """More records and more ORFs than or_name_k and or_len_k have lanes: a lane takes a second item, its sums hold
    several before they are added up, and the rank search runs over millions of rows."""
    want = scale.many_expected()
    assert len(want[1]) > scale.LANES and scale.MANY_RECORDS > scale.LANES
    check(ctx, scale.many(), want, scale.MANY_RECORDS, many_bases())


def test_many_records_from_pieces(ctx):
    info = check(ctx, scale.many(), scale.many_expected(), scale.MANY_RECORDS, many_bases(), piece_bytes=1 << 20)
    assert info["pieces"] > 5
