"""The row-window walk continued into stage 3 (bugseg_debug_stage3_windows, host only): from the rows of the
60 x 80 stage-3 output that the 128 -> 64 upsampling block reads, back through ENet's last stage-3 blocks.
Checked against the kernels' read footprints restated here: every row a consumer reads lies inside its
producer's window, the plain-tile windows are whole tile rows from their first row, the row-dilated ones
exactly the rows needed, and the walk stops where a window stops running fewer rows than the full launch."""
import itertools

import pytest

from bugcar_image_segmentation_amd import _native as N

H8 = 60
# ENet's stage-3 tail on a 60 x 80 grid at B = 64, nearest the decoder first:
# (asymmetric, dilation, row-dilated tiles, rows the full-frame launch computes, rows per windowed tile row)
B37 = (0, 16, 1, 16 * 1 * 4, 4)     # 3.7: 16 row phases x one 4 x 80 tile
B36 = (1, 1, 0, 3 * 20, 16)         # 3.6: asymmetric, 20 x 16 tiles full-frame, 16 x 16 windowed
B35 = (0, 8, 1, 8 * 2 * 4, 4)       # 3.5: 8 row phases x two 4 x 80 tiles
B34 = (0, 1, 0, 3 * 20, 20)         # 3.4: regular, 20 x 16 tiles
TAIL = [B37, B36, B35, B34]
# The class-row spans below, of a 480-row frame: the bench calibration's [239, 479), the whole frame, the
# near-field strip [400, 480) (whose windows reach block 3.5 and beyond) and the upper half [0, 240).


@pytest.fixture(autouse=True)
def _lib(native_lib):
    return native_lib


def _reach(blk):
    return 2 if blk[0] else blk[1]          # the asymmetric block's 5x1 conv; a 3x3 block's dilation


def _up_rows(span):
    """rows of the stage-3 output the 128 -> 64 block reads for a class-row span (op 0 of the decoder's six)"""
    return N.row_windows(480, 640, span[0], span[1], 8, 16)[0]


def _rows_run(blk, y0, y1):
    """(rows a windowed launch of blk runs for needed rows [y0, y1), the end of its window)"""
    if blk[2]:
        return y1 - y0, y1
    run = -(-(y1 - y0) // blk[4]) * blk[4]
    return run, min(y0 + run, H8)


def _check(blocks, y0, y1):
    wins = N.stage3_windows(H8, y0, y1, blocks)
    need = (y0, y1)                          # what the consumer of the block at hand reads
    for blk, (a, b) in zip(blocks, wins):
        assert 0 <= a < b <= H8 and (a, b) != (0, H8)
        assert a == need[0] and b >= need[1], "a window starts at the first needed row and covers the last"
        run, end = _rows_run(blk, *need)
        assert b == end
        assert run < blk[3], "a windowed launch runs fewer rows than the full-frame one"
        need = (max(a - _reach(blk), 0), min(b + _reach(blk), H8))
    m = len(wins)
    if m < len(blocks):
        # the first block left whole: its window would be the frame, or would save nothing, or has no windowed form
        blk = blocks[m]
        run, _ = _rows_run(blk, *need)
        pow2 = blk[1] & (blk[1] - 1) == 0
        assert need == (0, H8) or run >= blk[3] or (blk[2] and not pow2) or (not blk[2] and blk[1] != 1)
    return wins


def test_the_bench_span_windows_blocks_37_and_36():
    y0, y1 = _up_rows((239, 479))
    assert (y0, y1) == (28, 60)
    # 3.7 runs the 32 rows the upsampling block reads, 3.6 three 16-row tile rows from row 28 - 16
    assert _check([B37, B36], y0, y1) == [(28, 60), (12, 60)]
    # further back 3.5 would run 50 of its 64 row slots; 3.4 needs rows [2, 60): three 20-row tile rows, the
    # full launch's count, so the walk stops there
    assert _check(TAIL, y0, y1) == [(28, 60), (12, 60), (10, 60)]


def test_the_whole_frame_is_not_windowed():
    assert _up_rows((0, 480)) == (0, 60)
    assert _check(TAIL, 0, 60) == []


def test_a_near_field_strip_reaches_block_35_and_beyond():
    y0, y1 = _up_rows((400, 480))
    assert (y0, y1) == (48, 60)
    assert _check(TAIL, y0, y1) == [(48, 60), (32, 60), (30, 60), (22, 60)]


def test_the_upper_half():
    y0, y1 = _up_rows((0, 240))
    assert (y0, y1) == (0, 41)
    # 3.6 would need rows [0, 57): four 16-row tile rows, more than the full launch's 60 rows
    assert _check(TAIL, y0, y1) == [(0, 41)]


@pytest.mark.parametrize("order", list(itertools.permutations(range(4), 2)) + [(0, 1, 2, 3), (3, 2, 1, 0), (1, 1), (0, 0, 0)])
def test_any_order_of_blocks_gets_the_right_windows_or_none(order):
    """The rule comes from the descriptors, not from the blocks' places: every order of them, every window."""
    blocks = [TAIL[i] for i in order]
    edges = [0, 1, 2, 11, 12, 15, 16, 17, 28, 31, 32, 44, 47, 48, 58, 59, 60]
    for y0, y1 in itertools.combinations(edges, 2):
        _check(blocks, y0, y1)


def test_forms_without_a_windowed_kernel_stop_the_walk():
    y0, y1 = 28, 60
    assert N.stage3_windows(H8, y0, y1, [(0, 2, 0, 64, 16), B36]) == []         # plain tiles of a dilated block
    assert N.stage3_windows(H8, y0, y1, [(0, 12, 1, 64, 4), B36]) == []         # a dilation that is no power of two
    assert N.stage3_windows(H8, y0, y1, [B37, (1, 1, 0, 60, 0)]) == [(28, 60)]  # no windowed tile form picked
    assert N.stage3_windows(H8, y0, y1, []) == []


def test_bad_arguments_are_refused():
    for args in [(0, 0, 1), (60, -1, 10), (60, 10, 10), (60, 10, 61)]:
        with pytest.raises(ValueError):
            N.stage3_windows(*args, [B37])
