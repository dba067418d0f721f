"""hostio.HostStream: NumPy BGR frames in, NumPy int8 grids out (the reference's host-to-host loop,
models.py:42-44 -> bev.py:244-246) through pinned slots, with the copies on their own streams beside
the captured step. Every comparison is bit for bit against a separate eager OccupancyPipeline on its
own ENET fed the same frames as a device tensor; references are computed once and shared, read-only.
No test asserts a time or a rate."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import synthetic
from bugcar_image_segmentation_amd.hostio import HostStream
from bugcar_image_segmentation_amd.models import ENET
from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W, B = 96, 128, 4
GRID = (3.0, 3.0, 0.05)
_FRAMES, _REF_PIPES, _REFS = {}, {}, {}


def _bev(laserscan=False):
    bev = synthetic.synthetic_bev(H, W, 300, 300)
    bev.laserscan_like_occupancy_grid = laserscan
    return bev


def _frames(seed, hw=(H, W)):
    """Batch `seed` of the test frames (a different seed per batch), read-only."""
    key = (seed, hw)
    if key not in _FRAMES:
        f = synthetic.road_frames(B, hw[0], hw[1], seed=100 + seed)
        f.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def _pipe(blocks, prec="fp32", streams=1, ros=False, binary=False, laserscan=False):
    return OccupancyPipeline(ENET(weights=blocks, precision=prec), _bev(laserscan), *GRID, model_hw=(H, W),
                             streams=streams, ros_layout=ros, binary=binary)


def _ref(gpu, blocks, seed, prec="fp32", hw=(H, W), ros=False, binary=False, laserscan=False):
    """The device path's grids for batch `seed`: an eager pipeline of its own (one per configuration)."""
    cfg = (prec, ros, binary, laserscan)
    key = cfg + (hw, seed)
    if key not in _REFS:
        if cfg not in _REF_PIPES:
            _REF_PIPES[cfg] = _pipe(blocks, prec, 1, ros, binary, laserscan)
        g = _REF_PIPES[cfg].run(torch.from_numpy(np.array(_frames(seed, hw))).to(gpu)).cpu().numpy()
        g.setflags(write=False)
        _REFS[key] = g
    return _REFS[key]


@pytest.mark.parametrize("depth,graph,streams,prec", [
    (1, True, 1, "fp32"), (1, False, 1, "fp32"), (1, True, 2, "fp16"),
    (2, True, 1, "fp32"), (2, True, 2, "fp32"), (2, False, 2, "fp32"), (2, True, 2, "fp16"), (2, False, 1, "fp16"),
    (3, True, 1, "fp32"), (3, True, 2, "fp32"), (3, False, 1, "fp16"), (3, True, 1, "fp16"),
])
def test_slot_reuse(gpu, blocks, depth, graph, streams, prec):
    """Seven batches through one stream with `depth` steps kept in flight: every slot is reused at
    least twice, and every get() is its own batch's grids."""
    n = 7
    want = [_ref(gpu, blocks, k, prec) for k in range(n)]
    got, seqs = [], []
    with HostStream(_pipe(blocks, prec, streams), B, depth=depth, graph=graph) as hs:
        assert hs.grid_shape == want[0].shape
        for k in range(n):
            if hs.outstanding == depth:
                got.append(hs.get(copy=True))
            seqs.append(hs.put(_frames(k)))
        assert hs.outstanding == min(depth, n)
        while hs.outstanding:
            got.append(hs.get(copy=True))
    assert seqs == list(range(n))
    assert len(got) == n
    for k in range(n):
        assert got[k].dtype == np.int8 and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("depth", [1, 2])
def test_in_place_feeding_with_scribbling(gpu, blocks, depth):
    """The caller writes into next_frames() and, right after put(), scribbles over the buffer
    next_frames() hands out next: that call must have waited for the slot's copy-in (depth 1: the
    very copy just enqueued), so no step ever sees the scribble."""
    n = 5
    want = [_ref(gpu, blocks, k) for k in range(n)]
    # (the check can see a scribble: an all-0xFF batch gives other grids than any of the batches)
    white = _REF_PIPES[("fp32", False, False, False)].run(torch.full((B, H, W, 3), 0xFF, dtype=torch.uint8, device=gpu))
    assert not any(np.array_equal(white.cpu().numpy(), w) for w in want)
    got = []
    with HostStream(_pipe(blocks), B, depth=depth) as hs:
        for k in range(n):
            if hs.outstanding == depth:
                got.append(hs.get(copy=True))
            buf = hs.next_frames()
            assert buf.shape == (B, H, W, 3) and buf.dtype == np.uint8
            buf[...] = _frames(k)
            hs.put()
            hs.next_frames().fill(0xFF)
        while hs.outstanding:
            got.append(hs.get(copy=True))
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("depth", [2, 3])
def test_result_lifetime(gpu, blocks, depth):
    """The view get() returns stays unchanged through depth - 1 further put()s (none reuses its slot)."""
    with HostStream(_pipe(blocks), B, depth=depth) as hs:
        hs.put(_frames(0))
        view = hs.get()
        assert np.shares_memory(view, hs._pin_grids[0].numpy())
        snap = view.copy()
        assert np.array_equal(snap, _ref(gpu, blocks, 0))
        for k in range(1, depth):
            hs.put(_frames(k))
        later = [hs.get(copy=True) for _ in range(1, depth)]       # those steps ran to their copy-outs
        assert np.array_equal(view, snap)
        for k in range(1, depth):
            assert np.array_equal(later[k - 1], _ref(gpu, blocks, k)), k


def test_resize_path(gpu, blocks):
    hw = (131, 170)                                   # not the model resolution: the pipeline's resize runs
    n = 3
    got = []
    with HostStream(_pipe(blocks), B, frame_hw=hw, depth=2) as hs:
        assert hs.next_frames().shape == (B,) + hw + (3,)
        got = list(hs.map(_frames(k, hw) for k in range(n)))
    for k in range(n):
        assert np.array_equal(got[k], _ref(gpu, blocks, k, hw=hw)), k


def test_ros_layout(gpu, blocks):
    want = [_ref(gpu, blocks, k, ros=True) for k in range(3)]
    with _pipe(blocks, ros=True).host_stream(B) as hs:
        got = list(hs.map(_frames(k) for k in range(3)))
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("streams", [1, 2])
def test_binary_laserscan_pair(gpu, blocks, streams):
    """binary=True with the laserscan-like calibration: the result is the reference's pair, (2, B, ...)."""
    want = [_ref(gpu, blocks, k, binary=True, laserscan=True) for k in range(3)]
    assert want[0].ndim == 4 and want[0].shape[:2] == (2, B)
    with _pipe(blocks, streams=streams, binary=True, laserscan=True).host_stream(B) as hs:
        assert hs.grid_shape == want[0].shape
        got = list(hs.map(_frames(k) for k in range(3)))
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k


def test_errors_enqueue_nothing(gpu, blocks):
    with HostStream(_pipe(blocks), B, depth=2) as hs:
        with pytest.raises(RuntimeError):                          # underrun
            hs.get()
        for bad in (np.zeros((B + 1, H, W, 3), np.uint8), np.zeros((B, H, W, 3), np.float32),
                    np.zeros((B, H, W), np.uint8), np.zeros((B, W, H, 3), np.uint8)):
            with pytest.raises(ValueError):
                hs.put(bad)
        assert hs.steps_put == 0 and hs.outstanding == 0
        assert hs.put(_frames(0)) == 0 and hs.put(_frames(1)) == 1
        with pytest.raises(RuntimeError):                          # overrun: put number depth + 1
            hs.put(_frames(2))
        with pytest.raises(RuntimeError):
            hs.put()
        with pytest.raises(ValueError):                            # a full ring and a wrong array: still refused
            hs.put(np.zeros((B, H, W, 3), np.int8))
        assert hs.steps_put == 2 and hs.outstanding == 2
        # the refused calls left the slots alone: the two results are batches 0 and 1
        assert np.array_equal(hs.get(), _ref(gpu, blocks, 0))
        assert hs.put(_frames(2)) == 2                             # after a fetch that slot may be put again
        assert np.array_equal(hs.get(), _ref(gpu, blocks, 1))
        assert np.array_equal(hs.get(), _ref(gpu, blocks, 2))
        with pytest.raises(RuntimeError):
            hs.get()
    with pytest.raises(RuntimeError):                              # closed
        hs.put(_frames(0))
    with pytest.raises(ValueError):
        HostStream(_pipe(blocks), B, depth=0)


def test_run_host_and_map(gpu, blocks):
    pipe = _pipe(blocks)
    for k in (0, 1, 0):                                            # the cached depth-1 stream is reused
        g = pipe.run_host(_frames(k))
        assert g.flags.owndata and g.dtype == np.int8
        assert np.array_equal(g, _ref(gpu, blocks, k))
    assert len(pipe._host) == 1
    hw = (131, 170)                                                # another camera resolution: its own stream
    assert np.array_equal(pipe.run_host(_frames(0, hw)), _ref(gpu, blocks, 0, hw=hw))
    assert np.array_equal(pipe.run_host(_frames(2)), _ref(gpu, blocks, 2))
    for bad in (np.zeros((B, H, W), np.uint8), np.zeros((B, H, W, 3), np.float32)):
        with pytest.raises(ValueError):
            pipe.run_host(bad)
    with pytest.raises(ValueError):                                # run keeps refusing host tensors
        pipe.run(torch.from_numpy(np.array(_frames(0))))
    with pipe.host_stream(B, depth=2) as hs:
        out = list(hs.map(_frames(k) for k in range(5)))
        assert hs.outstanding == 0
    assert len(out) == 5
    for k in range(5):
        assert out[k].flags.owndata and np.array_equal(out[k], _ref(gpu, blocks, k)), k


def test_buffers_are_pinned(gpu, blocks):
    with HostStream(_pipe(blocks), B, depth=2) as hs:
        assert len(hs._pin_frames) == 2 and len(hs._pin_grids) == 2
        for s in range(2):
            assert hs._pin_frames[s].is_pinned() and hs._pin_grids[s].is_pinned()
            assert hs._pin_frames[s].shape == hs._dev_frames[s].shape and hs._dev_frames[s].is_cuda
            assert hs._pin_grids[s].shape == hs._dev_grids[s].shape and hs._dev_grids[s].dtype == torch.int8
        # what the caller sees are views of those buffers
        assert np.shares_memory(hs.next_frames(), hs._pin_frames[0].numpy())
        hs.put(_frames(0))
        assert np.shares_memory(hs.next_frames(), hs._pin_frames[1].numpy())
        assert np.shares_memory(hs.get(), hs._pin_grids[0].numpy())


def test_bench_host_io_runs(gpu):
    cmd = [sys.executable, "bench_host_io.py", "--batch", "4", "--height", "96", "--width", "128",
           "--steps", "3", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=220)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(line))
    for k in ("device_fps", "host_fps", "host_fps_staged", "copy_in_ms", "copy_out_ms", "step_ms", "host_over_device"):
        assert isinstance(line[k], float) and math.isfinite(line[k]) and line[k] > 0, (k, line[k])
    for k in ("device_ms", "host_stream_ms", "host_api_ms"):
        v = line["latency_b1"][k]
        assert isinstance(v, float) and math.isfinite(v) and v > 0, (k, v)
