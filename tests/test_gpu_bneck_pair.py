"""Two consecutive fp32 C = 64 regular bottlenecks as one launch (bneck_pair_kernels.hip), against the
plans without it, bit for bit.

* default weights: the paired plan's logits equal the unfused chain's (BUGSEG_NO_FUSE=1). Shapes whose stage-1
  maps leave every 12 x 16 tile ragged at the image edge (18 x 26, 16 x 24) and one with interior tiles and tiles
  whose +- 2 ring crosses exactly one edge (40 x 52); one workgroup per tile and eight workgroups walking many
  tiles; both tile orders. With the arena poisoned the spare buffer stays poison: the pair ran, and neither its
  fallbacks nor a cut pair's plain launches did.
* a forward cut into two calls anywhere in stage 1 — between the ops of a pair too — equals the whole forward.
* the plan's own launches, one by one (launch_op: what the per-kernel tables time), compute the paired forward's logits.
* where the pair's speculation on the range exponents fails (weights scaled out of the f16 window in one block of
  a pair, the undamped draw) the guarded fallbacks redo the pair: the logits equal those of the fused plan without
  pairs, and the undamped ones pass the range bar."""
import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import enet_spec, synthetic
from bugcar_image_segmentation_amd.models import ENET
from oracle import enet_oracle as eo

pytestmark = pytest.mark.gpu

SHAPES = [(2, 72, 104), (3, 64, 96), (2, 160, 208)]
POISON = 0xA5
_unfused = {}


def _bgr(B, H, W):
    return torch.from_numpy(synthetic.road_frames(B, H, W, seed=H + W)).cuda()


def _logits(ctx, bgr, first=0, last=-1, out=None):
    B, H, W = bgr.shape[:3]
    out = torch.empty((B, 15, H, W), dtype=torch.float32, device=bgr.device) if out is None else out
    if (first, last) == (0, -1):
        ctx.forward_bgr(bgr, B, H, W, N.OUT_LOGITS_F32, out)
    else:
        ctx.forward_bgr_ops(bgr, B, H, W, N.OUT_LOGITS_F32, out, first, last)
    return out


def _reference(blocks, shape, monkeypatch):
    """the unfused chain's logits, once per shape (they depend on neither the grid nor the tile order)"""
    if shape not in _unfused:
        with monkeypatch.context() as m:
            m.setenv("BUGSEG_NO_FUSE", "1")
            _unfused[shape] = _logits(ENET(weights=blocks, precision="fp32").ctx, _bgr(*shape)).clone()
    return _unfused[shape]


@pytest.mark.parametrize("order", ["0", "1"])
@pytest.mark.parametrize("grid", [None, "8"])
@pytest.mark.parametrize("shape", SHAPES)
def test_paired_plan_equals_the_unfused_chain(gpu, blocks, monkeypatch, shape, grid, order):
    want = _reference(blocks, shape, monkeypatch)
    monkeypatch.setenv("BUGSEG_TILE_ORDER", order)
    if grid:
        monkeypatch.setenv("BUGSEG_BNECK_GRID", grid)
    ctx = ENET(weights=blocks, precision="fp32").ctx
    bgr = _bgr(*shape)
    B, H, W = shape
    _logits(ctx, bgr)                                        # builds the plan
    pairs = ctx.pair_plan()
    assert [p[0] for p in pairs] == [2, 4], "blocks 1.1 + 1.2 and 1.3 + 1.4"
    th, tw = pairs[0][1:3]
    assert pairs[0][3:5] == (-(-(H // 4) // th), -(-(W // 4) // tw)) and pairs[0][6] <= 160 * 1024
    assert [p[7] for p in pairs] == [0, 1]                   # the second pair runs in the other buffers
    got = _logits(ctx, bgr).clone()
    # again over a poisoned arena, stopped behind stage 1 (later, unfused blocks use the spare buffer for themselves)
    ctx.poison_arena(POISON)
    n = ctx.plan_info(B, H, W, N.OUT_LOGITS_F32, bgr_input=True)[0]
    cut = torch.zeros_like(got)
    _logits(ctx, bgr, 0, 6, cut)
    spare = torch.empty((B, H // 4, W // 4, 64 * 4), dtype=torch.uint8, device=gpu)
    ctx.read_block_output(2, spare)                          # a pair's first block: the spare buffer
    _logits(ctx, bgr, 6, n, cut)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(cut, want)
    assert bool((spare == POISON).all()), "the pair's fallbacks or a cut pair's launches ran"


@pytest.mark.parametrize("env,prec", [({"BUGSEG_BNECK_VARIANT_C64": "2"}, "fp32"), ({"BUGSEG_BNECK_VARIANT": "0"}, "fp32"),
                                      ({"BUGSEG_NO_FUSE": "1"}, "fp32"), ({}, "fp16"), ({}, "bf16")])
def test_no_pairs_where_the_rule_says_none(gpu, blocks, monkeypatch, env, prec):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = ENET(weights=blocks, precision=prec).ctx
    _logits(ctx, _bgr(2, 72, 104))
    assert ctx.pair_plan() == []


@pytest.mark.parametrize("cut", [2, 3, 4, 5, 6])
def test_a_forward_cut_in_two_calls_equals_the_whole(gpu, blocks, cut):
    ctx = ENET(weights=blocks, precision="fp32").ctx
    bgr, other = _bgr(2, 72, 104), _bgr(2, 72, 104).flip(1)
    whole = _logits(ctx, bgr).clone()
    _logits(ctx, other)                                      # another input's activations in the arena ...
    ctx.poison_arena(POISON)                                 # ... then the fill: nothing stale is correct
    out = torch.zeros_like(whole)
    _logits(ctx, bgr, 0, cut, out)
    _logits(ctx, bgr, cut, -1, out)
    torch.cuda.synchronize()
    assert torch.equal(out, whole)


def test_the_plan_without_the_overlay_computes_the_forward(gpu, blocks):
    """What DESIGN 6.23 promises of the plan's own launches (plan_op, launch_op, the per-kernel table): issued one by
    one over a poisoned arena they compute the paired forward's logits, bit for bit, and leave the overlay alone. The
    pair's output tensor is one place, however the forward that wrote it was cut."""
    B, H, W = 2, 72, 104
    ctx = ENET(weights=blocks, precision="fp32").ctx
    bgr = _bgr(B, H, W)
    want = _logits(ctx, bgr).clone()
    whole = torch.empty((B, H // 4, W // 4, 64 * 4), dtype=torch.uint8, device=gpu)
    ctx.read_block_output(3, whole)
    ctx.poison_arena(POISON)
    out = _logits(ctx, bgr)                                  # the binding the single launches run under
    out.zero_()
    for i in range(ctx.plan_info(B, H, W, N.OUT_LOGITS_F32, bgr_input=True)[0]):
        ctx.launch_op(B, H, W, i)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert [p[0] for p in ctx.pair_plan()] == [2, 4]
    ctx.poison_arena(POISON)
    _logits(ctx, bgr, 0, 3, out)                             # the first pair cut between its blocks
    _logits(ctx, bgr, 3, -1, out)
    cut = torch.empty_like(whole)
    ctx.read_block_output(3, cut)
    torch.cuda.synchronize()
    assert torch.equal(cut, whole) and torch.equal(out, want)


def _scaled(name, unit, factor):
    bl = enet_spec.build_enet()
    u = next(b for b in bl if b.name == name).units[unit]
    u.w = (u.w.astype(np.float64) * factor).astype(np.float32)
    return bl


def _pair_vs_unpaired(bl, bgr, monkeypatch):
    """(logits of the paired plan, of the fused plan with the C = 64 form forced, which has no pairs)"""
    paired = ENET(weights=bl, precision="fp32").ctx
    got = _logits(paired, bgr)
    assert len(paired.pair_plan()) == 2
    again = _logits(paired, bgr)
    with monkeypatch.context() as m:
        m.setenv("BUGSEG_BNECK_VARIANT_C64", "2")
        plain = ENET(weights=bl, precision="fp32").ctx
        want = _logits(plain, bgr)
        assert plain.pair_plan() == []
    with monkeypatch.context() as m:
        m.setenv("BUGSEG_BNECK_GRID", "8")
        walked = _logits(ENET(weights=bl, precision="fp32").ctx, bgr)
    torch.cuda.synchronize()
    assert torch.equal(got, again) and torch.equal(got, walked)
    return got, want


# block A's exponents non-zero (the pair leaves at once); block B's alone (the pair runs, its result is redone);
# the second pair's blocks
@pytest.mark.parametrize("name,unit,factor", [("regular1_1", 0, 1e6), ("regular1_2", 1, 1e6), ("regular1_2", 0, 1e-6),
                                              ("regular1_3", 2, 1e5), ("regular1_4", 2, 1e6)])
def test_a_failed_speculation_is_redone_by_the_fallbacks(gpu, monkeypatch, name, unit, factor):
    bl = _scaled(name, unit, factor)
    got, want = _pair_vs_unpaired(bl, _bgr(2, 72, 104), monkeypatch)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want)


def test_undamped_draw_passes_the_range_bar(gpu, monkeypatch):
    bl = enet_spec.build_enet(res_gamma=(0.5, 1.5))
    B, H, W = 2, 72, 104
    bgr = synthetic.road_frames(B, H, W, seed=H + W)
    got, want = _pair_vs_unpaired(bl, torch.from_numpy(bgr).cuda(), monkeypatch)
    assert torch.equal(got, want)
    x = np.ascontiguousarray(np.moveaxis((bgr[..., ::-1] / 256.0 - eo.IMAGE_MEAN) / eo.IMAGE_STD, -1, 1))
    ties = eo.PoolTies()
    ref = eo.forward(bl, x.astype(np.float64), torch.float64, ties=ties)
    m = ENET(weights=bl, precision="fp32")
    logits = m.logits(x.astype(np.float32))                  # (the engine-input entry, as tests/test_gpu_range.py)
    assert len(m.ctx.pair_plan()) == 2
    idx = eo.engine_pool_indices(m.ctx, bl, ties, B, H, W)
    ok, msg, _ = eo.range_verdict(logits, ref, ties, idx, "undamped 72x104, paired plan")
    print(msg)
    assert ok, msg
