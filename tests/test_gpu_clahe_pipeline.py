"""OccupancyPipeline(clahe=True): image_processing_utils.clahe on the camera-size frames before the resize and
the segmenter. Its grids equal, bit for bit, those of the same pipeline with clahe=False run on
clahe_device(frames) (which tests/test_gpu_clahe.py pins to tests/clahe_ref.py): eager, captured, sharded,
windowed, through run_host, with the road filter, and with a reduced-width DeepLabV3. After a windowed run
_seg completes the class maps from the enhanced frames, and clahe=False changes nothing.

64 x 96 model input, camera frames of 80 x 120 (resized) and 64 x 96 (not), B = 4, darkened synthetic road
scenes; synthetic_bev(64, 96, 200, 200), a 2 m x 2 m grid of 0.05 m cells. References are computed once per
configuration and shared, read-only."""
import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import deeplab_spec as S
from bugcar_image_segmentation_amd import enet_spec, synthetic
from bugcar_image_segmentation_amd.image_processing_utils import clahe_device
from bugcar_image_segmentation_amd.models import ENET, DeepLabV3, class_lut3, class_lut_binary
from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline
from deeplab_balanced import balance_logits

pytestmark = pytest.mark.gpu

H, W, B = 64, 96, 4
CAMERAS = [(80, 120), (64, 96)]
WARP = (200, 200)
GRID = (2.0, 2.0, 0.05)
NCLS = 21
_CACHE = {}


def _blocks():
    if "blocks" not in _CACHE:
        _CACHE["blocks"] = enet_spec.build_enet()
    return _CACHE["blocks"]


def _frames(hw):
    """Dusk: road scenes at 30 % of their brightness, (B, H0, W0, 3) u8, read-only."""
    if hw not in _CACHE:
        f = (synthetic.road_frames(B, *hw, seed=17).astype(np.float64) * 0.3).astype(np.uint8)
        f.setflags(write=False)
        _CACHE[hw] = f
    return _CACHE[hw]


def _dev(gpu, hw):
    return torch.from_numpy(np.array(_frames(hw))).to(gpu)


def _enet_pipe(**kw):
    kw.setdefault("model_hw", (H, W))
    return OccupancyPipeline(ENET(weights=_blocks(), precision="fp32"), synthetic.synthetic_bev(H, W, *WARP), *GRID, **kw)


def _want(gpu, hw, make=_enet_pipe, **kw):
    """The grids (and whole class maps) of the clahe=False pipeline run on clahe_device(frames)."""
    key = ("want", hw, make.__name__, tuple(sorted(kw.items())))
    if key not in _CACHE:
        enh = clahe_device(_dev(gpu, hw))
        pipe = make(**dict(kw, window_rows=False))
        grids = pipe.run(enh).cpu().numpy()
        seg = pipe._seg.cpu().numpy()
        grids.setflags(write=False)
        seg.setflags(write=False)
        _CACHE[key] = (grids, seg)
    return _CACHE[key]


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
def test_the_case_is_not_vacuous(gpu, hw):
    dev = _dev(gpu, hw)
    enh = clahe_device(dev)
    changed = int((enh != dev).any(dim=-1).sum())
    assert changed > dev[..., 0].numel() // 2, "clahe leaves most of the dusk frames as they are"
    raw = _enet_pipe(window_rows=False)
    raw.run(dev)
    grids, seg = _want(gpu, hw)
    differ = int((raw._seg.cpu().numpy() != seg).sum())
    print(hw, "pixels changed by clahe:", changed, "class-map pixels that differ:", differ)
    assert differ > 0, "the segmenter sees no difference between the raw and the enhanced frames"


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
@pytest.mark.parametrize("kw", [dict(), dict(window_rows=False), dict(streams=2), dict(streams=2, chain_forwards=True),
                                dict(streams=2, shard_offset=5), dict(ros_layout=True)], ids=str)
def test_eager(gpu, hw, kw):
    dev = _dev(gpu, hw)
    pipe = _enet_pipe(clahe=True, **kw)
    want = _want(gpu, hw, **{k: v for k, v in kw.items() if k == "ros_layout"})[0]
    got = pipe.run(dev).cpu().numpy()
    assert got.dtype == np.int8 and np.array_equal(got, want)
    assert np.array_equal(dev.cpu().numpy(), _frames(hw))                     # the caller's frames are untouched
    assert np.array_equal(pipe._clahe[2].cpu().numpy(), clahe_device(dev).cpu().numpy())
    assert np.array_equal(pipe.run(dev).cpu().numpy(), want)


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
@pytest.mark.parametrize("streams,warm", [(1, False), (2, False), (2, True)])
def test_captured(gpu, hw, streams, warm):
    dev = torch.zeros((B, *hw, 3), dtype=torch.uint8, device=gpu)
    pipe = _enet_pipe(clahe=True, streams=streams)
    replay, out = pipe.capture(dev, warm=warm)
    dev.copy_(_dev(gpu, hw))
    replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(out.cpu().numpy(), _want(gpu, hw)[0])


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
@pytest.mark.parametrize("streams", [1, 2])
def test_windowed_run_keeps_the_enhanced_frames(gpu, hw, streams):
    """After a windowed run _seg re-runs the forward on the frames it kept: with clahe=True those are the
    enhanced frames (and they are not enhanced a second time)."""
    dev = _dev(gpu, hw)
    pipe = _enet_pipe(clahe=True, window_rows=True, streams=streams)
    grids, seg = _want(gpu, hw)
    assert np.array_equal(pipe.run(dev).cpu().numpy(), grids)
    assert pipe._windowed and pipe._seg_partial is not None, "this calibration reads every row: nothing was windowed"
    partial = pipe._seg_raw.cpu().numpy()
    assert not np.array_equal(partial, seg)
    assert np.array_equal(pipe._seg.cpu().numpy(), seg)


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
def test_run_host(gpu, hw):
    pipe = _enet_pipe(clahe=True)
    want = _want(gpu, hw)[0]
    got = pipe.run_host(np.array(_frames(hw)))
    assert got.dtype == np.int8 and np.array_equal(got, want)
    assert np.array_equal(pipe.run_host(np.array(_frames(hw))), want)


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
@pytest.mark.parametrize("streams", [1, 2])
def test_with_the_road_filter(gpu, hw, streams):
    want = _want(gpu, hw, binary=True, road_filter=True)[0]
    pipe = _enet_pipe(clahe=True, binary=True, road_filter=True, streams=streams)
    assert np.array_equal(pipe.run(_dev(gpu, hw)).cpu().numpy(), want)


def _dl_net():
    if "net" not in _CACHE:
        probe = synthetic.road_frames(2, 65, 97, seed=39)[..., ::-1]
        _CACHE["net"] = balance_logits(S.build_deeplab(width=0.25, crop=(65, 97), num_classes=NCLS), np.ascontiguousarray(probe))
    return _CACHE["net"]


def _dl_pipe(**kw):
    model = DeepLabV3(net=_dl_net(), precision="fp32")
    model.class_lut = class_lut3(NCLS, [c for c in range(NCLS) if c % 3 == 1], [c for c in range(NCLS) if c % 3 == 2]) \
        if not kw.get("binary") else class_lut_binary(NCLS, [c for c in range(NCLS) if c % 3])
    kw.setdefault("model_hw", (H, W))
    return OccupancyPipeline(model, synthetic.synthetic_bev(H, W, *WARP), *GRID, **kw)


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
@pytest.mark.parametrize("streams", [1, 2])
def test_deeplab(gpu, hw, streams):
    dev = _dev(gpu, hw)
    grids, seg = _want(gpu, hw, make=_dl_pipe)
    pipe = _dl_pipe(clahe=True, streams=streams)
    assert np.array_equal(pipe.run(dev).cpu().numpy(), grids)
    assert np.array_equal(pipe._seg.cpu().numpy(), seg)
    replay, out = pipe.capture(dev)
    replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(out.cpu().numpy(), grids)


@pytest.mark.parametrize("hw", CAMERAS, ids=str)
@pytest.mark.parametrize("streams", [1, 2])
def test_without_clahe_nothing_changes(gpu, hw, streams):
    dev = _dev(gpu, hw)
    off = _enet_pipe(clahe=False, streams=streams)
    got = off.run(dev).cpu().numpy()
    assert np.array_equal(got, _enet_pipe(streams=streams).run(dev).cpu().numpy())
    assert off._clahe is None and not off.clahe
