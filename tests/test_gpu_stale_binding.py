"""A forward's input and output are bound into a copy of a launch at issue time; the plan, its cached row
windows (window_plan: 8 per plan, built once per window) and the class-fused launch never hold them. These
tests keep more than one output alive and alternate inputs, output kinds and windows on one context, so a
cached launch that kept the previous call's pointer, LUT or logits pointer writes the wrong tensor or the
wrong values. (The other window tests allocate a fresh output per call, which the caching allocator may
place at the same address each time.) Everything is bit-exact: a windowed launch runs the full launch's
per-pixel arithmetic on the tiles it keeps.

96 x 128 at B = 2: three tile rows at both decoder resolutions, as in test_gpu_row_window.py.
"""
from types import SimpleNamespace

import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import synthetic
from bugcar_image_segmentation_amd.models import ENET

pytestmark = pytest.mark.gpu

B, H, W = 2, 96, 128
WIN = (41, 96)
KINDS = (N.OUT_CLASS3_U8, N.OUT_BINARY_U8, N.OUT_LOGITS_F32)


def _fill(kind, ncls, dev, b=B):
    if kind == N.OUT_LOGITS_F32:
        return torch.full((b, ncls, H, W), float("nan"), dtype=torch.float32, device=dev)
    return torch.full((b, H, W), 255, dtype=torch.uint8, device=dev)


def _same(a, b):
    """bit equality (NaN fills included)"""
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def case(request, gpu, blocks):
    """One context per precision, two inputs, and the full forward of each input and output kind (computed once,
    never written again)."""
    model = ENET(weights=blocks, precision=request.param)
    frames = {"X": torch.from_numpy(synthetic.road_frames(B, H, W, seed=5)).to(gpu),
              "Y": torch.from_numpy(synthetic.uniform_frames(B, H, W, seed=6)).to(gpu)}
    ref = {}
    for name, x in frames.items():
        for kind in KINDS:
            ref[name, kind] = _fill(kind, model.num_classes, gpu)
            model.ctx.forward_bgr(x, B, H, W, kind, ref[name, kind])
    torch.cuda.synchronize()
    r0, r1 = WIN
    for kind in KINDS:      # a stale input shows in the window's rows, and so does a stale LUT
        assert not _same(ref["X", kind][..., r0:r1, :], ref["Y", kind][..., r0:r1, :])
    assert not _same(ref["X", N.OUT_CLASS3_U8][..., r0:r1, :], ref["X", N.OUT_BINARY_U8][..., r0:r1, :])
    return SimpleNamespace(gpu=gpu, model=model, ctx=model.ctx, ncls=model.num_classes, frames=frames, ref=ref)


def _window(c, name, kind, out, rows=WIN, others=()):
    """Class rows `rows` of input `name` into `out`: those rows become the full forward's, every other row of `out`
    and every tensor of `others` stays as it was."""
    r0, r1 = rows
    before = [t.clone() for t in (out, *others)]
    c.ctx.forward_bgr_rows(c.frames[name], B, H, W, kind, out, rows)
    torch.cuda.synchronize()
    what = f"window {rows} of {name}, kind {kind}"
    assert _same(out[..., r0:r1, :], c.ref[name, kind][..., r0:r1, :]), f"{what}: rows differ from the full forward"
    assert _same(out[..., :r0, :], before[0][..., :r0, :]), f"{what}: rows above were written"
    assert _same(out[..., r1:, :], before[0][..., r1:, :]), f"{what}: rows below were written"
    for t, b in zip(others, before[1:]):
        assert _same(t, b), f"{what}: another live output was written"


def test_two_live_outputs_each_get_their_own_call(case):
    c = case
    a, b = _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu), _fill(N.OUT_BINARY_U8, c.ncls, c.gpu)
    assert a.data_ptr() != b.data_ptr()
    _window(c, "X", N.OUT_CLASS3_U8, a, others=(b,))
    _window(c, "X", N.OUT_BINARY_U8, b, others=(a,))      # the cached class-layer launch: new pointer, new LUT
    _window(c, "Y", N.OUT_CLASS3_U8, a, others=(b,))      # ... and a new input
    assert (a[:, :WIN[0]] == 255).all() and (b[:, :WIN[0]] == 255).all()


def test_logits_and_a_class_map_alternate(case):
    c = case
    lg, a = _fill(N.OUT_LOGITS_F32, c.ncls, c.gpu), _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu)
    _window(c, "X", N.OUT_LOGITS_F32, lg, others=(a,))
    _window(c, "X", N.OUT_CLASS3_U8, a, others=(lg,))     # the cached launch must not keep logits_out
    _window(c, "Y", N.OUT_LOGITS_F32, lg, others=(a,))    # ... nor cls_out and the LUT
    _window(c, "Y", N.OUT_BINARY_U8, a, others=(lg,))


def test_a_window_evicted_from_the_cache_is_rebuilt_right(case):
    c = case
    windows = [WIN, (32, 96), (64, 96), (30, 50), (95, 96), (0, 10), (10, 60), (20, 90), (50, 70), (5, 96)]
    assert len(set(windows)) == 10                        # two more than the cache holds
    for k, rows in enumerate(windows):
        _window(c, "XY"[k & 1], N.OUT_CLASS3_U8, _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu), rows)
    out = _fill(N.OUT_BINARY_U8, c.ncls, c.gpu)
    _window(c, "Y", N.OUT_BINARY_U8, out, windows[0])
    _window(c, "X", N.OUT_BINARY_U8, out, windows[-1])    # still cached


def test_a_full_forward_after_a_windowed_one_writes_every_row(case):
    c = case
    a = _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu)
    _window(c, "X", N.OUT_CLASS3_U8, a)
    full = _fill(N.OUT_BINARY_U8, c.ncls, c.gpu)
    c.ctx.forward_bgr(c.frames["Y"], B, H, W, N.OUT_BINARY_U8, full)
    torch.cuda.synchronize()
    assert _same(full, c.ref["Y", N.OUT_BINARY_U8])
    # the profiling hook replays the full class layer for that forward's binding, not the window's
    n = c.ctx.plan_info(B, H, W, N.OUT_BINARY_U8, bgr_input=True)[0]
    kept = a.clone()
    full.fill_(255)
    c.ctx.launch_op(B, H, W, n - 1)
    torch.cuda.synchronize()
    assert _same(full, c.ref["Y", N.OUT_BINARY_U8])
    assert _same(a, kept)


def test_a_shape_change_drops_the_cached_windows(case):
    c = case
    _window(c, "X", N.OUT_CLASS3_U8, _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu))
    x3 = torch.from_numpy(synthetic.road_frames(3, H, W, seed=7)).to(c.gpu)
    ref3 = _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu, 3)
    c.ctx.forward_bgr(x3, 3, H, W, N.OUT_CLASS3_U8, ref3)             # rebuilds the plan
    out3 = _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu, 3)
    c.ctx.forward_bgr_rows(x3, 3, H, W, N.OUT_CLASS3_U8, out3, WIN)
    torch.cuda.synchronize()
    r0, r1 = WIN
    assert (ref3 != 255).all()
    assert _same(out3[:, r0:r1], ref3[:, r0:r1]) and (out3[:, :r0] == 255).all()
    _window(c, "Y", N.OUT_CLASS3_U8, _fill(N.OUT_CLASS3_U8, c.ncls, c.gpu))   # and back: rebuilt again
