"""The fp32 C64 pair kernel with its memory traffic overlapped (bneck_pair_kernels.hip): block A's
residual x left in the y region by A1 and read back by A3 (BNECK_PAIR_XLDS), the next tile's x loaded during the
current tile (BNECK_PAIR_PREF). Logits byte-identical to the unfused chain on the three stage-1 grids where the new
A1 and A3 can go wrong, with 12 x 16 tiles:

* 48 x 64, B = 2: a 12 x 16 grid, exactly one tile per frame; every pixel of the +- 2 and +- 1 rings is outside the
  image, and a workgroup's next tile is another frame's or none;
* 64 x 96, B = 3: 16 x 24, 2 x 2 tiles, partial in both directions; an odd frame count against eight workgroups;
* 104 x 160, B = 2: 26 x 40, 3 x 3 tiles; tile (1, 1) has its whole +- 2 ring inside the image, every other tile
  some of it outside. (Not 104 x 136: on its 26 x 34 grid no untransposed form of the single blocks keeps 60 % of
  its tile pixels inside the image, pick_bneck_variant takes transposed ones and the plan has no pairs. 26 x 40 is
  the next grid with the same tiling that pairs.)

Each with one workgroup per tile and with eight workgroups walking many tiles (the prefetch crosses tile rows and
frames), both tile orders; the spare buffer stays poison behind stage 1 (the pair ran and no fallback did). Where the
speculation fails (a stage-1 weight scaled out of the f16 window) the early exit and the redo equal the plan without
pairs. A library built with both macros off (the serial tile) computes the same bytes, so the off paths stay alive."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import enet_spec, synthetic
from bugcar_image_segmentation_amd.models import ENET

pytestmark = pytest.mark.gpu

SHAPES = [(2, 48, 64), (3, 64, 96), (2, 104, 160)]
POISON = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_unfused = {}


def _bgr(B, H, W):
    return torch.from_numpy(synthetic.road_frames(B, H, W, seed=H + W)).cuda()


def _logits(ctx, bgr, first=0, last=-1, out=None):
    B, H, W = bgr.shape[:3]
    out = torch.empty((B, 15, H, W), dtype=torch.float32, device=bgr.device) if out is None else out
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
def test_overlapped_pair_equals_the_unfused_chain(gpu, blocks, monkeypatch, shape, grid, order):
    want = _reference(blocks, shape, monkeypatch)
    monkeypatch.setenv("BUGSEG_TILE_ORDER", order)
    if grid:
        monkeypatch.setenv("BUGSEG_BNECK_GRID", grid)
    ctx = ENET(weights=blocks, precision="fp32").ctx
    bgr = _bgr(*shape)
    B, H, W = shape
    got = _logits(ctx, bgr).clone()
    pairs = ctx.pair_plan()
    assert [p[0] for p in pairs] == [2, 4], "blocks 1.1 + 1.2 and 1.3 + 1.4"
    assert pairs[0][1:5] == (12, 16, -(-(H // 4) // 12), -(-(W // 4) // 16))
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


def _scaled(name, unit, factor):
    bl = enet_spec.build_enet()
    u = next(b for b in bl if b.name == name).units[unit]
    u.w = (u.w.astype(np.float64) * factor).astype(np.float32)
    return bl


# block A's exponents non-zero: every workgroup leaves before A1; block B's alone: the pair runs and is redone
@pytest.mark.parametrize("name,unit,factor", [("regular1_1", 0, 1e6), ("regular1_2", 1, 1e6)])
def test_a_failed_speculation_is_still_redone(gpu, monkeypatch, name, unit, factor):
    bl = _scaled(name, unit, factor)
    bgr = _bgr(3, 64, 96)
    paired = ENET(weights=bl, precision="fp32").ctx
    got = _logits(paired, bgr).clone()
    assert len(paired.pair_plan()) == 2
    with monkeypatch.context() as m:
        m.setenv("BUGSEG_BNECK_VARIANT_C64", "2")
        plain = ENET(weights=bl, precision="fp32").ctx
        want = _logits(plain, bgr)
        assert plain.pair_plan() == []
    with monkeypatch.context() as m:
        m.setenv("BUGSEG_BNECK_GRID", "8")
        walked = _logits(ENET(weights=bl, precision="fp32").ctx, bgr)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want) and torch.equal(walked, want)


_CHILD = """
import hashlib, sys, torch
sys.path.insert(0, {root!r})
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import enet_spec, synthetic
from bugcar_image_segmentation_amd.models import ENET
B, H, W = 3, 64, 96
bgr = torch.from_numpy(synthetic.road_frames(B, H, W, seed=H + W)).cuda()
ctx = ENET(weights=enet_spec.build_enet(), precision="fp32").ctx
out = torch.empty((B, 15, H, W), dtype=torch.float32, device="cuda")
ctx.forward_bgr(bgr, B, H, W, N.OUT_LOGITS_F32, out)
torch.cuda.synchronize()
assert [p[0] for p in ctx.pair_plan()] == [2, 4]
print("sha", hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest())
"""


@pytest.mark.parametrize("grid", [None, "8"])
def test_a_library_with_the_macros_off_computes_the_same(gpu, blocks, monkeypatch, grid):
    """build_native(variant, defines) with BNECK_PAIR_XLDS and BNECK_PAIR_PREF both 0, the serial tile of before:
    one compile of bneck_kernels.hip, shared by both grids (the build is incremental). The library is loaded by a
    child process, BUGSEG_LIB being read when the package is imported."""
    from bugcar_image_segmentation_amd.build import build_native
    want = _reference(blocks, (3, 64, 96), monkeypatch)
    lib = build_native(variant="pair_serial", defines=("-DBNECK_PAIR_XLDS=0", "-DBNECK_PAIR_PREF=0"),
                       only=("bneck_kernels.hip",))
    env = dict(os.environ, BUGSEG_LIB=str(lib))
    if grid:
        env["BUGSEG_BNECK_GRID"] = grid
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split("sha")[-1].strip() == hashlib.sha256(want.cpu().numpy().tobytes()).hexdigest()
