"""contour_noise_removal on the device (csrc/road_kernels.hip) against the brute restatement of its pinned
semantics (tests/road_filter_ref.py), bit for bit: every structured case at every shape (k = 1: the closing
is the identity; widths that are no multiple of 4 or 64; the even k = 2; k = 3, 5, 9), uniform noise, batches
against single frames, and the call's run-time properties (repeatable, independent of the workspace's
contents, any stream, capturable on its first call, refusals launch nothing)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import road_filter_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import image_processing_utils as ipu

pytestmark = pytest.mark.gpu

ALL_SHAPES = R.SHAPES + [(60, 50)]


def run(maps, dev, **kw):
    t = torch.from_numpy(np.array(maps)).to(dev)
    return ipu.contour_noise_removal_device(t, **kw).cpu().numpy()


@pytest.mark.parametrize("h,w", ALL_SHAPES, ids=lambda v: str(v))
def test_every_case_as_one_batch(gpu, h, w):
    names, maps, ref = R.cases_with_ref(h, w)
    got = run(maps, gpu)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    for i, name in enumerate(names):
        bad = np.count_nonzero(got[i] != ref[i])
        assert bad == 0, f"{name} at {h}x{w}: {bad} pixels differ, first at {np.argwhere(got[i] != ref[i])[0]}"


@pytest.mark.parametrize("h,w", ALL_SHAPES, ids=lambda v: str(v))
def test_every_case_as_a_single_frame(gpu, h, w):
    names, maps, ref = R.cases_with_ref(h, w)
    for i, name in enumerate(names):
        got = run(maps[i], gpu)
        assert got.shape == (1, h, w)
        assert np.array_equal(got[0], ref[i]), f"{name} at {h}x{w}"


def test_batch_of_five_equals_five_singles(gpu):
    h, w = 100, 120
    names, maps, ref = R.cases_with_ref(h, w)
    pick = [names.index(n) for n in ("scene", "noise_0.6", "nest5", "serpentine", "values_0_255")]
    got = run(maps[pick], gpu)
    for j, i in enumerate(pick):
        assert np.array_equal(got[j], run(maps[i], gpu)[0]) and np.array_equal(got[j], ref[i]), names[i]


def test_reference_signature(gpu):
    h, w = 150, 200
    names, maps, ref = R.cases_with_ref(h, w)
    i = names.index("values_0_255")
    out = ipu.contour_noise_removal(np.array(maps[i]))
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.owndata and np.array_equal(out, ref[i])
    assert np.array_equal(ipu.contour_noise_removal(torch.from_numpy(np.array(maps[i]))), ref[i])
    i = names.index("scene")
    assert np.array_equal(ipu.contour_noise_removal(maps[i].astype(np.int64)), ref[i])
    from bugcar_image_segmentation_amd import models
    assert np.array_equal(models.contour_noise_removal(np.array(maps[i])), ref[i])


@pytest.fixture(scope="module")
def noisy():
    h, w = 100, 120
    names, maps, ref = R.cases_with_ref(h, w)
    pick = [names.index(n) for n in ("noise_0.6", "scene", "spiral")]
    return maps[pick], ref[pick]


def test_two_calls_are_identical(gpu, noisy):
    maps, ref = noisy
    a, b = run(maps, gpu), run(maps, gpu)
    assert np.array_equal(a, b) and np.array_equal(a, ref)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_workspace_contents_do_not_matter(gpu, noisy, fill):
    maps, ref = noisy
    B, h, w = maps.shape
    p = ipu.road_filter_params(h, w)
    ctx = N.shared_context(gpu.index)
    n = int(ctx.lib.bugseg_road_filter_workspace_bytes(ctypes.byref(p), B))
    assert n >= B * h * w * 17
    ws = torch.full((n,), fill, dtype=torch.uint8, device=gpu)
    seg = torch.from_numpy(np.array(maps)).to(gpu)
    out = torch.empty_like(seg)
    ctx.road_filter(seg, B, p, out, workspace=ws)
    assert np.array_equal(out.cpu().numpy(), ref)


def test_side_stream(gpu, noisy):
    maps, ref = noisy
    seg = torch.from_numpy(np.array(maps)).to(gpu)
    torch.cuda.synchronize(gpu)
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        out = ipu.contour_noise_removal_device(seg)
    st.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


def test_first_call_at_a_shape_captured_and_replayed(gpu):
    h, w = 57, 71                                   # a shape no other test uses, on a context of its own
    a = R.noise(h, w, 0.62, 21)
    b = R._scene(h, w, 5)
    ctx = N.Context(gpu.index, N.FP32)
    p = ipu.road_filter_params(h, w)
    seg = torch.from_numpy(a).to(gpu).unsqueeze(0).contiguous()
    out = torch.zeros_like(seg)
    gc.collect()                                    # no finalizer of an earlier test's garbage inside the capture
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            ctx.road_filter(seg, 1, p, out)
    finally:
        gc.enable()
    seg.copy_(torch.from_numpy(b).to(gpu).unsqueeze(0))
    graph.replay()
    torch.cuda.synchronize(gpu)
    want = R.brute(b)
    assert want.any() and not np.array_equal(want, R.brute(a))
    assert np.array_equal(out[0].cpu().numpy(), want)
    ctx.close()


def test_refusals_launch_nothing(gpu):
    h, w, B = 50, 64, 2
    ctx = N.shared_context(gpu.index)
    seg = torch.ones((B, h, w), dtype=torch.uint8, device=gpu)
    out = torch.full((B, h, w), 7, dtype=torch.uint8, device=gpu)
    good = ipu.road_filter_params(h, w)
    ws = torch.empty(int(ctx.lib.bugseg_road_filter_workspace_bytes(ctypes.byref(good), B)), dtype=torch.uint8, device=gpu)

    def params(**kw):
        p = ipu.road_filter_params(h, w)
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    bad = [dict(B=0), dict(B=-1), dict(p=params(k=0)), dict(p=params(k=65)), dict(p=params(y_top=-1)),
           dict(p=params(y_top=h)), dict(p=params(min_count=0)), dict(p=params(rows=1 << 16, cols=1 << 15)),
           dict(workspace=ws[:ws.numel() - 512]), dict(out=seg)]
    for case in bad:
        with pytest.raises(N.BugsegError) as e:
            ctx.road_filter(seg, case.get("B", B), case.get("p", good), case.get("out", out),
                            workspace=case.get("workspace", ws))
        assert e.value.code == N.EINVAL, case
    # a NULL workspace
    rc = ctx.lib.bugseg_road_filter(ctx.h, seg.data_ptr(), B, ctypes.byref(good), out.data_ptr(), None, 0,
                                    N.stream_handle(None))
    assert rc == N.EINVAL and b"workspace" in ctx.lib.bugseg_last_error(ctx.h)
    torch.cuda.synchronize(gpu)
    assert bool((out == 7).all()) and bool((seg == 1).all())
    ctx.road_filter(seg, B, good, out, workspace=ws)
    assert bool((out == 1).all())
