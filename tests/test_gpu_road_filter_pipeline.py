"""OccupancyPipeline(road_filter=True): contour_noise_removal between the segmenter and the rasteriser. The
grids equal the C rasteriser (oracle.ocv_c, binary variant) run on brute(class map) of tests/road_filter_ref.py,
bit for bit, where the class maps come from a separate engine; with road_filter=False they equal the existing
binary path's. References are computed once and shared, read-only.

ENet case: 104 x 136 (k = 2), synthetic_bev(104, 136, 300, 300), a 3 m x 3 m grid of 0.05 m cells, B = 4, fp32.
The default synthetic weights call ~17 % of the pixels road, in specks the filter drops entirely; with 0.2 added
to the class layer's bias of the two road classes (checked on the CPU with oracle.enet_oracle: 26 % road) the
filter keeps a filled region in three of the four frames and drops everything in the fourth.
DeepLab case: geometry "a" of tests/test_gpu_deeplab_pipeline.py (crop 65 x 97, width 0.25, class_lut_binary)."""
import numpy as np
import pytest
import torch

import road_filter_ref as R
from bugcar_image_segmentation_amd import deeplab_spec as S
from bugcar_image_segmentation_amd import enet_spec, synthetic
from bugcar_image_segmentation_amd.models import ENET, DeepLabV3, class_lut_binary
from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline
from deeplab_balanced import balance_logits
from oracle import ocv_c

pytestmark = pytest.mark.gpu

H, W, B = 104, 136, 4
WARP = (300, 300)
GRID = (3.0, 3.0, 0.05)
_CACHE = {}


def _blocks():
    if "blocks" not in _CACHE:
        blocks = enet_spec.build_enet()
        blocks[-1].units[0].b[:2] += 0.2          # the road and lane-marking classes (models.py:79-80)
        _CACHE["blocks"] = blocks
    return _CACHE["blocks"]


def _bev(hw=(H, W), warp=WARP, laserscan=False):
    bev = synthetic.synthetic_bev(*hw, *warp)
    bev.laserscan_like_occupancy_grid = laserscan
    return bev


def _frames():
    if "frames" not in _CACHE:
        f = synthetic.road_frames(B, H, W, seed=0)
        f.setflags(write=False)
        _CACHE["frames"] = f
    return _CACHE["frames"]


def _oracle(bev, warp, grid, seg, laserscan=False):
    args = (bev._bev_matrix, *warp, 1.0, *grid)
    if laserscan:
        pairs = [ocv_c.create_occupancy_grid_binary_laserscan(s, *args) for s in seg]
        return np.stack([np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])])
    return np.stack([ocv_c.create_occupancy_grid_binary(s, *args) for s in seg])


def _enet_ref(gpu):
    """(predict_binary maps of a separate ENET, their brute filter), read-only."""
    if "enet" not in _CACHE:
        ref = ENET(weights=_blocks(), precision="fp32")
        seg = ref.predict_binary(ENET.preprocess_device(torch.from_numpy(np.array(_frames())).to(gpu), width=W, height=H))
        flt = np.stack([R.brute(s) for s in seg])
        seg.setflags(write=False)
        flt.setflags(write=False)
        _CACHE["enet"] = (seg, flt)
    return _CACHE["enet"]


def _want(gpu, filtered=True, laserscan=False):
    key = ("want", filtered, laserscan)
    if key not in _CACHE:
        seg, flt = _enet_ref(gpu)
        g = _oracle(_bev(), WARP, GRID, flt if filtered else seg, laserscan)
        g.setflags(write=False)
        _CACHE[key] = g
    return _CACHE[key]


def _pipe(laserscan=False, **kw):
    return OccupancyPipeline(ENET(weights=_blocks(), precision="fp32"), _bev(laserscan=laserscan), *GRID,
                             model_hw=(H, W), binary=True, **kw)


def test_the_case_is_not_vacuous(gpu):
    seg, flt = _enet_ref(gpu)
    live = [i for i in range(B) if flt[i].any() and not np.array_equal(flt[i], seg[i])]
    print("road fraction in", seg.mean(axis=(1, 2)).round(3).tolist(), "out", flt.mean(axis=(1, 2)).round(3).tolist())
    assert live, "no frame whose filtered map is neither empty nor its input"
    assert not np.array_equal(_want(gpu, True), _want(gpu, False))


@pytest.mark.parametrize("streams", [1, 2])
def test_enet_grids_equal_rasterised_brute(gpu, streams):
    dev = torch.from_numpy(np.array(_frames())).to(gpu)
    pipe = _pipe(road_filter=True, streams=streams)
    got = pipe.run(dev).cpu().numpy()
    assert got.dtype == np.int8 and np.array_equal(got, _want(gpu))
    # full-frame forwards whatever window_rows says: the class maps are whole, the filtered maps brute's
    seg, flt = _enet_ref(gpu)
    assert pipe._source_rows(pipe._ctxs[0]) is None
    assert np.array_equal(pipe._seg_raw.cpu().numpy(), seg) and np.array_equal(pipe._road[1].cpu().numpy(), flt)
    assert np.array_equal(pipe.run(dev).cpu().numpy(), _want(gpu))


@pytest.mark.parametrize("streams", [1, 2])
def test_enet_first_call_captured(gpu, streams):
    dev = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=gpu)
    pipe = _pipe(road_filter=True, streams=streams)
    replay, out = pipe.capture(dev, warm=False)
    dev.copy_(torch.from_numpy(np.array(_frames())).to(gpu))
    replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(out.cpu().numpy(), _want(gpu))


def test_capture_runs_no_finalizer(gpu):
    """capture() collects dead reference cycles before the capture begins and keeps the cyclic collector off
    while the stream captures (a finalizer that destroys a context or frees pinned memory there ends the
    capture or the process), then restores it. The probe's finalizer only records where it ran."""
    import gc
    seen = []

    class Probe:
        def __init__(self):
            self.me = self                      # a cycle: only the cyclic collector frees it

        def __del__(self):
            seen.append(bool(torch.cuda.is_current_stream_capturing()))

    class Churn:
        """Allocations inside run() that would trip the collector's thresholds during the capture."""
        def __init__(self, pipe):
            self.pipe, self.inner = pipe, pipe._run_shard

        def __call__(self, *a, **kw):
            late = Probe()                      # becomes garbage while the stream captures
            del late
            junk = [[i] for i in range(5000)]   # far past the youngest generation's threshold
            del junk
            return self.inner(*a, **kw)

    dev = torch.from_numpy(np.array(_frames())).to(gpu)
    pipe = _pipe(road_filter=True)
    pipe.run(dev)
    Probe()
    pipe._run_shard = Churn(pipe)
    assert gc.isenabled()
    replay, out = pipe.capture(dev, warm=False)
    assert gc.isenabled()
    gc.collect()
    assert len(seen) == 2 and seen == [False, False], seen
    replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(out.cpu().numpy(), _want(gpu))


def test_enet_run_host(gpu):
    pipe = _pipe(road_filter=True)
    got = pipe.run_host(np.array(_frames()))
    assert got.dtype == np.int8 and np.array_equal(got, _want(gpu))
    assert np.array_equal(pipe.run_host(np.array(_frames())), _want(gpu))


@pytest.mark.parametrize("streams", [1, 2])
def test_enet_laserscan_pair(gpu, streams):
    dev = torch.from_numpy(np.array(_frames())).to(gpu)
    got = _pipe(laserscan=True, road_filter=True, streams=streams).run(dev).cpu().numpy()
    want = _want(gpu, True, laserscan=True)
    assert got.shape == want.shape and got.shape[0] == 2 and np.array_equal(got, want)


@pytest.mark.parametrize("streams", [1, 2])
def test_without_the_filter_nothing_changes(gpu, streams):
    dev = torch.from_numpy(np.array(_frames())).to(gpu)
    off = _pipe(road_filter=False, streams=streams)
    got = off.run(dev).cpu().numpy()
    assert np.array_equal(got, _want(gpu, False))
    assert np.array_equal(got, _pipe(streams=streams).run(dev).cpu().numpy())
    assert off._road is None and off.window_rows


# ---------------------------------------------------------------- DeepLabV3, geometry "a"
NCLS = 21
DL = dict(crop=(65, 97), warp=(200, 200), grid=(2.0, 2.0, 0.05))
LUTB = class_lut_binary(NCLS, [c for c in range(NCLS) if c % 3])     # two thirds of the balanced classes are road


def _dl_net():
    if "net" not in _CACHE:
        probe = synthetic.road_frames(2, *DL["crop"], seed=39)[..., ::-1]
        _CACHE["net"] = balance_logits(S.build_deeplab(width=0.25, crop=DL["crop"], num_classes=NCLS),
                                       np.ascontiguousarray(probe))
    return _CACHE["net"]


@pytest.mark.parametrize("streams,Bd", [(1, 2), (2, 3)])
def test_deeplab_grids_equal_rasterised_brute(gpu, streams, Bd):
    f = synthetic.road_frames(Bd, *DL["crop"], seed=40)
    ref = DeepLabV3(net=_dl_net(), precision="fp32")
    seg = LUTB[ref.predict(np.ascontiguousarray(f[..., ::-1]))]
    flt = np.stack([R.brute(s) for s in seg])
    bev = _bev(DL["crop"], DL["warp"])
    want = _oracle(bev, DL["warp"], DL["grid"], flt)
    print("road fraction in", seg.mean(axis=(1, 2)).round(3).tolist(), "out", flt.mean(axis=(1, 2)).round(3).tolist())
    assert any(x.any() and not np.array_equal(x, s) for x, s in zip(flt, seg))       # the filter does something here
    model = DeepLabV3(net=_dl_net(), precision="fp32")
    model.class_lut = LUTB
    pipe = OccupancyPipeline(model, bev, *DL["grid"], binary=True, road_filter=True, streams=streams)
    dev = torch.from_numpy(f).to(gpu)
    assert np.array_equal(pipe.run(dev).cpu().numpy(), want)
    assert np.array_equal(pipe._seg_raw.cpu().numpy(), seg) and np.array_equal(pipe._road[1].cpu().numpy(), flt)
    replay, out = pipe.capture(dev)
    replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(out.cpu().numpy(), want)
