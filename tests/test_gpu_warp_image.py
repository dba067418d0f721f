"""warp_image on the device (bev_warp_image_kernel in csrc/bev_kernels.hip) against cv2.warpPerspective as
oracle/ocv_np.py restates it, per channel, and the 8-bit BGR -> gray formula (tests/hough_ref.py warp_image), bit
for bit: 1 and 3 channels and gray over the three geometries of the reference-glue fixtures (the bench calibration
among them), a matrix that leaves part of the result outside the source, a singular matrix; batches, views at odd
offsets, capture, refusals."""
import gc
import json
import os

import numpy as np
import pytest
import torch

import hough_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd.bev import bev_transform_tools
from bugcar_image_segmentation_amd.synthetic import road_frames, synthetic_bev

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_glue.npz")


def make_bev(in_shape, out_shape, M):
    b = bev_transform_tools(list(in_shape), list(out_shape), (0.0, 100.0), 50.0, 1.0, 0.0, False)
    b._bev_matrix = np.asarray(M, np.float64).reshape(3, 3)
    return b


def geometries():
    with np.load(FIX, allow_pickle=False) as z:
        out = {}
        for g in ("bench", "small_neg", "small_odd"):
            d = json.loads(bytes(z[f"{g}/json"]).decode())
            out[g] = make_bev(d["input image size"], d["output image size"], d["bev matrix"])
    out["outside"] = make_bev((37, 53), (90, 61), [[1.5, 0.2, -20.0], [0.1, 1.4, 9.0], [0.0, 0.0, 1.0]])
    out["singular"] = make_bev((37, 53), (40, 30), [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, 0.25, 1.0]])
    return out


GEO = geometries()


def frames_for(b, n, seed):
    return road_frames(n, int(b.input_width), int(b.input_height), seed=seed)


def ref(b, frame, gray=False):
    return R.warp_image(frame, b._bev_matrix, (int(b.after_warp_width), int(b.after_warp_height)), gray=gray)


def diff(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {bad[0]}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


@pytest.mark.parametrize("g", list(GEO), ids=str)
def test_three_channels_gray_and_one_channel(gpu, g):
    b = GEO[g]
    n = 1 if g == "bench" else 3
    fr = frames_for(b, n, seed=11)
    x = torch.from_numpy(fr).to(gpu)
    bgr = b.warp_image_device(x).cpu().numpy()
    gray = b.warp_image_device(x, gray=True).cpu().numpy()
    one = b.warp_image_device(x[..., 1].contiguous()).cpu().numpy()
    h, w = int(b.after_warp_height), int(b.after_warp_width)
    assert bgr.shape == (n, h, w, 3) and gray.shape == (n, h, w) and one.shape == (n, h, w)
    for i in range(n):
        want = ref(b, fr[i])
        diff(bgr[i], want, f"{g} frame {i}, 3 channels")
        diff(gray[i], ref(b, fr[i], gray=True), f"{g} frame {i}, gray")
        diff(one[i], want[:, :, 1], f"{g} frame {i}, 1 channel")
    if g == "outside":
        assert 0.1 < (ref(b, np.full_like(fr[0], 255))[:, :, 0] == 0).mean() < 0.9        # the border is in the result
    if g == "singular":
        assert (bgr[0] == fr[0][0, 0]).all()                 # every pixel samples the source's corner, as OpenCV's


def test_single_frames_and_the_host_form(gpu):
    b = GEO["small_neg"]
    fr = frames_for(b, 1, seed=5)[0]
    want = ref(b, fr)
    x = torch.from_numpy(fr).to(gpu)
    diff(b.warp_image_device(x)[0].cpu().numpy(), want, "(r, c, 3)")
    diff(b.warp_image_device(x[:, :, 0].contiguous())[0].cpu().numpy(), want[:, :, 0], "(r, c)")
    for arg in (fr, torch.from_numpy(fr), x):
        got = b.warp_image(arg)
        assert isinstance(got, np.ndarray) and got.flags.owndata
        diff(got, want, "host form")
    diff(b.warp_image(fr, gray=True), ref(b, fr, gray=True), "host form, gray")
    diff(b.warp_image(np.asfortranarray(fr[:, :, 2])), want[:, :, 2], "host form, one channel")


def test_batch_larger_than_a_threads_frames_and_odd_offsets(gpu):
    b = GEO["small_odd"]
    n = 19                                                   # three frame groups, the last with 3
    fr = frames_for(b, n, seed=2)
    want = np.stack([ref(b, f) for f in fr])
    want_gray = np.stack([ref(b, f, gray=True) for f in fr])
    size = fr.size
    for off_in, off_out in ((1, 3), (7, 5)):
        src = torch.zeros(size + 16, dtype=torch.uint8, device=gpu)
        x = src[off_in:off_in + size].view(fr.shape)
        x.copy_(torch.from_numpy(fr))
        dst = torch.full((want.size + 16,), 0x55, dtype=torch.uint8, device=gpu)
        out = dst[off_out:off_out + want.size].view(want.shape)
        assert x.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
        assert b.warp_image_device(x, out=out) is out
        diff(out.cpu().numpy(), want, f"offsets {off_in}, {off_out}")
        d = dst.cpu().numpy()
        assert (d[:off_out] == 0x55).all() and (d[off_out + want.size:] == 0x55).all()
        dstg = torch.full((want_gray.size + 16,), 0x55, dtype=torch.uint8, device=gpu)
        outg = dstg[off_out:off_out + want_gray.size].view(want_gray.shape)
        b.warp_image_device(x, gray=True, out=outg)
        diff(outg.cpu().numpy(), want_gray, f"gray, offsets {off_in}, {off_out}")
        d = dstg.cpu().numpy()
        assert (d[:off_out] == 0x55).all() and (d[off_out + want_gray.size:] == 0x55).all()


def test_side_stream_capture_and_replay(gpu):
    b = GEO["small_neg"]
    fa, fb = frames_for(b, 2, seed=8), frames_for(b, 2, seed=9)
    x = torch.from_numpy(fa).to(gpu)
    out = torch.zeros((2, int(b.after_warp_height), int(b.after_warp_width)), dtype=torch.uint8, device=gpu)
    N.shared_context(gpu.index)
    gc.collect()
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            b.warp_image_device(x, gray=True, out=out)
    finally:
        gc.enable()
    x.copy_(torch.from_numpy(fb))
    graph.replay()
    torch.cuda.synchronize(gpu)
    want = np.stack([ref(b, f, gray=True) for f in fb])
    assert not np.array_equal(want, np.stack([ref(b, f, gray=True) for f in fa]))
    diff(out.cpu().numpy(), want, "replay")
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        got = b.warp_image_device(x)
    st.synchronize()
    diff(got.cpu().numpy(), np.stack([ref(b, f) for f in fb]), "side stream")


def test_refusals_launch_nothing(gpu):
    b = GEO["small_neg"]
    r, c, h, w = int(b.input_width), int(b.input_height), int(b.after_warp_height), int(b.after_warp_width)
    ctx = N.shared_context(gpu.index)
    x = torch.full((2, r, c, 3), 9, dtype=torch.uint8, device=gpu)
    out = torch.full((2, h, w, 3), 7, dtype=torch.uint8, device=gpu)
    good = b.warp_params()

    def params(**kw):
        p = b.warp_params()
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    buf = torch.full((x.numel() + out.numel(),), 7, dtype=torch.uint8, device=gpu)
    xin = buf[:x.numel()].view(x.shape)
    bad = [dict(channels=2), dict(channels=0), dict(channels=4), dict(channels=1, gray=1), dict(gray=2), dict(B=0), dict(B=-1),
           dict(p=params(in_rows=0)), dict(p=params(in_cols=-1)), dict(p=params(warp_w=0)), dict(p=params(warp_h=0)),
           dict(p=params(in_rows=1 << 15, in_cols=1 << 15)), dict(p=params(warp_w=1 << 15, warp_h=1 << 15)),
           dict(x=xin, out=buf[x.numel() - 1:x.numel() - 1 + out.numel()].view(out.shape)), dict(out=x)]
    for case in bad:
        with pytest.raises(ValueError):
            ctx.warp_image(case.get("x", x), case.get("B", 2), case.get("channels", 3), case.get("p", good), case.get("gray", 0),
                           case.get("out", out))
    sh = N.stream_handle(None)
    assert ctx.lib.bugseg_bev_warp_image(ctx.h, None, 2, 3, good, 0, out.data_ptr(), sh) == N.EINVAL
    assert ctx.lib.bugseg_bev_warp_image(ctx.h, x.data_ptr(), 2, 3, None, 0, out.data_ptr(), sh) == N.EINVAL
    assert ctx.lib.bugseg_bev_warp_image(ctx.h, x.data_ptr(), 2, 3, good, 0, None, sh) == N.EINVAL
    torch.cuda.synchronize(gpu)
    assert bool((out == 7).all()) and bool((x == 9).all()) and bool((buf == 7).all())
    # the Python surface
    for t in (x.cpu(), x.to(torch.int8), x[:, :, :, :2], x[:, :, :c - 1], x[0, 0], x[:0]):
        with pytest.raises((ValueError, AssertionError)):
            b.warp_image_device(t)
    with pytest.raises(ValueError):
        b.warp_image_device(x[..., 0].contiguous(), gray=True)
    for o in (out[:1], out.to(torch.int8), torch.empty((2, h, w), dtype=torch.uint8, device=gpu)):
        with pytest.raises(ValueError):
            b.warp_image_device(x, out=o)
    # the fixtures' "bench" geometry is bench.py's calibration: 480 x 640 -> 1000 x 1000
    bench = synthetic_bev().warp_params()
    assert (bench.in_rows, bench.in_cols, bench.warp_w, bench.warp_h) == (480, 640, 1000, 1000)
    assert list(bench.M) == list(GEO["bench"].warp_params().M)
