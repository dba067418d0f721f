"""The row-windowed forward's stage-3 windows (include/bugseg.h bugseg_enet_forward_bgr_rows), by
the method of tests/test_gpu_row_window.py and as bit-exact: with the activation arena poisoned in between,
a windowed forward's rows inside every window equal the full forward's — the class rows and the output rows
of each windowed stage-3 block — and no launch writes a row outside its window.

fp32, B = 2, 480 x 640: the smallest shape with all 16 row phases of dilation 16 on 60 rows. The picker takes
the 8 x 16 asymmetric form there; BUGSEG_BNECK_VARIANT_ASYM=0 forces the 16 x 16 form a large batch runs."""
import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import synthetic
from bugcar_image_segmentation_amd.models import ENET
from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline

pytestmark = pytest.mark.gpu

B, H, W = 2, 480, 640
# the bench calibration's span; a near-field strip (row phases with no row in the window); a band that ends
# above the image's last row (the t0 halo below the window is real data, not the image edge); one odd row
WINDOWS = [(239, 479), (400, 480), (100, 300), (333, 334)]
POISON = 0xFF


@pytest.fixture(scope="module")
def frames(gpu):
    return (torch.from_numpy(synthetic.road_frames(B, H, W, seed=5)).to(gpu),
            torch.from_numpy(synthetic.uniform_frames(B, H, W, seed=6)).to(gpu))


def _block_outputs(ctx, ops, es):
    outs = {}
    for op in ops:
        t = torch.empty((B, H // 8, W // 8, 128 * es), dtype=torch.uint8, device="cuda")
        ctx.read_block_output(op, t)
        outs[op] = t
    torch.cuda.synchronize()
    return outs


def _run(ctx, A, other, rows, es, expect_windows):
    kind = N.OUT_CLASS3_U8
    n = ctx.plan_info(B, H, W, kind, bgr_input=True)[0]
    ref = torch.full((B, H, W), 255, dtype=torch.uint8, device=A.device)
    ctx.forward_bgr(A, B, H, W, kind, ref)
    wins = ctx.plan_windows(rows)
    print(f"rows {rows}: stage-3 windows (op, y0, y1, variant, tiles per frame) {wins}")
    assert (len(wins) > 0) == expect_windows
    ops = [w[0] for w in wins]
    # the blocks' full-frame outputs: the forward stopped before the 128 -> 64 block, which overwrites one of them
    ctx.forward_bgr_ops(A, B, H, W, kind, ref, 0, n - 6)
    want = _block_outputs(ctx, ops, es)
    ctx.forward_bgr(other, B, H, W, kind, ref.clone())      # another input's activations in the arena ...
    ctx.poison_arena(POISON)                                # ... then the fill: nothing stale is correct
    out = torch.full((B, H, W), 255, dtype=torch.uint8, device=A.device)
    # launch by launch: a block's output buffer holds an earlier block's output before its launch (the arena's
    # two activation buffers alternate), so "not written" is "as it was just before the launch"
    done = 0
    for op, y0, y1, _, _ in sorted(wins):
        ctx.forward_bgr_rows(A, B, H, W, kind, out, rows, done, op)
        before = _block_outputs(ctx, [op], es)[op]
        ctx.forward_bgr_rows(A, B, H, W, kind, out, rows, op, op + 1)
        got = _block_outputs(ctx, [op], es)[op]
        done = op + 1
        assert torch.equal(got[:, y0:y1], want[op][:, y0:y1]), f"op {op}: rows [{y0}, {y1}) differ from the full forward"
        assert not torch.equal(before[:, y0:y1], want[op][:, y0:y1])
        assert torch.equal(got[:, :y0], before[:, :y0]), f"op {op}: rows above [{y0}, {y1}) were written"
        assert torch.equal(got[:, y1:], before[:, y1:]), f"op {op}: rows below [{y0}, {y1}) were written"
    ctx.forward_bgr_rows(A, B, H, W, kind, out, rows, done, -1)
    torch.cuda.synchronize()
    r0, r1 = rows
    assert torch.equal(out[:, r0:r1], ref[:, r0:r1]), f"class rows [{r0}, {r1}) differ from the full forward"
    assert bool((out[:, :r0] == 255).all()) and bool((out[:, r1:] == 255).all()), "class rows outside the window were written"
    return wins


@pytest.mark.parametrize("asym", ["picked", "16x16"])
@pytest.mark.parametrize("order", ["0", "1"])
def test_stage3_windows_equal_the_full_forward_fp32(gpu, blocks, frames, monkeypatch, order, asym):
    monkeypatch.setenv("BUGSEG_TILE_ORDER", order)
    if asym == "16x16":
        monkeypatch.setenv("BUGSEG_BNECK_VARIANT_ASYM", "0")
    ctx = ENET(weights=blocks, precision="fp32").ctx
    for rows in WINDOWS:
        wins = _run(ctx, *frames, rows, 4, True)
        if rows == (239, 479):
            # blocks 3.7 (row-dilated, 16 tiles per frame as in the full launch) and 3.6 (three tile rows of 16, or six of 8)
            assert [w[1:3] for w in wins] == [(28, 60), (12, 60)]
            assert wins[0][3:] == (2, 16)
            if asym == "16x16":
                assert wins[1][3:] == (0, 15)


def test_the_two_byte_path_keeps_its_full_stage3(gpu, blocks, frames):
    ctx = ENET(weights=blocks, precision="fp16").ctx
    _run(ctx, *frames, (239, 479), 2, False)


def test_the_switch_keeps_stage3_whole(gpu, blocks, frames, monkeypatch):
    monkeypatch.setenv("BUGSEG_ROW_WINDOW_S3", "0")
    ctx = ENET(weights=blocks, precision="fp32").ctx
    _run(ctx, *frames, (239, 479), 4, False)


CALIBRATIONS = {
    "bench 480x640": (lambda: synthetic.synthetic_bev(480, 640), (synthetic.GRID_W_M, synthetic.GRID_H_M, synthetic.CELL_M), 480, 640),
    "96x128": (lambda: synthetic.synthetic_bev(96, 128, 300, 300), (3.0, 3.0, 0.05), 96, 128),
    "240x320": (lambda: synthetic.synthetic_bev(240, 320, 600, 600), (6.0, 6.0, 0.05), 240, 320),
}


@pytest.fixture(scope="module")
def fp32_model(gpu, blocks):
    return ENET(weights=blocks, precision="fp32")


@pytest.mark.parametrize("name", list(CALIBRATIONS))
def test_pipeline_grids_equal_the_unwindowed_pipeline(gpu, fp32_model, name):
    make, grid, h, w = CALIBRATIONS[name]
    bev = make()
    win = OccupancyPipeline(fp32_model, bev, *grid, model_hw=(h, w), window_rows=True)
    full = OccupancyPipeline(fp32_model, bev, *grid, model_hw=(h, w), window_rows=False)
    fr = torch.from_numpy(synthetic.road_frames(2, h, w, seed=9)).to(gpu)
    want = full.run(fr).clone()
    want_seg = full._seg.clone()
    got = win.run(fr).clone()
    torch.cuda.synchronize()
    rows = win._source_rows(fp32_model.ctx)
    assert rows is not None, "this calibration should leave rows to skip"
    print(f"{name}: class rows {rows}, stage-3 windows {fp32_model.ctx.plan_windows(rows)}")
    assert torch.equal(got, want)
    assert torch.equal(win._seg, want_seg)
