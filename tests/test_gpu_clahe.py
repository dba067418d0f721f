"""clahe on the device (csrc/clahe_kernels.hip) against the restatement of its pinned semantics
(tests/clahe_ref.py), bit for bit: the two colour stages over 2^20 triples, the tile look-up tables and the
full call at every shape (clip at its floor, divisible and padded sides, the smallest frame, 480 x 640) as a
batch and as single frames, other grids and clip limits, the reference's signature, and the call's run-time
properties (repeatable, independent of the workspace's contents, any stream, capturable on its first call,
refusals launch nothing)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import clahe_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import image_processing_utils as ipu

pytestmark = pytest.mark.gpu

BIG = (480, 640, ("scene", "noise"))


def stage(dev, frames, which, p=None, out_shape=None):
    """One debug stage over (B, h, w, 3) frames -> NumPy."""
    f = torch.from_numpy(np.array(frames)).to(dev)
    B, h, w = f.shape[:3]
    p = p if p is not None else ipu.clahe_params(h, w)
    out = torch.zeros(out_shape if out_shape is not None else tuple(f.shape), dtype=torch.uint8, device=dev)
    N.shared_context(dev.index).clahe(f, B, p, out, stage=which)
    return out.cpu().numpy()


def luts_of(dev, frames, clip_limit=3.0, tile_grid=(8, 8)):
    B, h, w = frames.shape[:3]
    p = ipu.clahe_params(h, w, clip_limit, tile_grid)
    return stage(dev, frames, 1, p, (B, tile_grid[1], tile_grid[0], 256))


def run(dev, frames, **kw):
    return ipu.clahe_device(torch.from_numpy(np.array(frames)).to(dev), **kw).cpu().numpy()


def describe(got, want, names):
    for i, name in enumerate(names):
        bad = np.argwhere(got[i] != want[i])
        if len(bad):
            at = tuple(bad[0])
            return f"{name}: {len(bad)} values differ, first at {at}: {got[i][at]} for {want[i][at]}"
    return ""


@pytest.fixture(scope="module")
def million():
    """1024 x 1024 triples: the lattice and the greys over the first rows, seeded random ones after them."""
    return R.triples(1 << 20, seed=5).reshape(1, 1024, 1024, 3)


def test_stage_0_bgr_to_lab(gpu, million):
    got = stage(gpu, million, 0)
    want = R.bgr_to_lab(million)
    assert np.array_equal(got, want), describe(got, want, ["triples"])


def test_stage_2_lab_to_bgr(gpu, million):
    got = stage(gpu, million, 2)
    want = R.lab_to_bgr(million)
    assert np.array_equal(got, want), describe(got, want, ["triples"])
    # out-of-gamut triples clamp: the extremes of a and b are in the lattice
    corner = want[0, 0, :216].reshape(-1)
    assert (corner == 0).any() and (corner == 255).any()


def test_stages_on_an_unaligned_view_and_a_partial_group(gpu, million):
    """Frames whose address is no multiple of 4 take the byte path, and a pixel count that is no multiple of 4
    ends in a partial group."""
    flat = torch.from_numpy(np.ascontiguousarray(million.reshape(-1)[: 3 * 33 * 35 + 1])).to(gpu)
    f = flat[1:].view(1, 33, 35, 3)
    assert f.data_ptr() % 4 == 1
    out = torch.zeros(3 * 33 * 35 + 3, dtype=torch.uint8, device=gpu)
    N.shared_context(gpu.index).clahe(f, 1, ipu.clahe_params(33, 35), out[3:].view(1, 33, 35, 3), stage=0)
    src = million.reshape(-1)[1: 3 * 33 * 35 + 1].reshape(1, 33, 35, 3)
    assert np.array_equal(out[3:].view(1, 33, 35, 3).cpu().numpy(), R.bgr_to_lab(src)) and bool((out[:3] == 0).all())
    got = stage(gpu, src, 0)                                    # aligned, 1155 pixels: 288 groups and 3 more
    assert np.array_equal(got, R.bgr_to_lab(src))
    assert np.array_equal(run(gpu, src), R.clahe(src[0])[None])


SHAPE_CASES = [(h, w, None) for (h, w) in R.SHAPES] + [BIG]


@pytest.mark.parametrize("h,w,only", SHAPE_CASES, ids=lambda v: str(v))
def test_luts_and_full_call_as_one_batch(gpu, h, w, only):
    names, fr, luts, outs = R.cases_with_ref(h, w, only=only)
    got = luts_of(gpu, fr)
    assert got.shape == luts.shape and np.array_equal(got, luts), describe(got, luts, names)
    got = run(gpu, fr)
    assert got.dtype == np.uint8 and got.shape == outs.shape
    assert np.array_equal(got, outs), describe(got, outs, names)


@pytest.mark.parametrize("h,w,only", SHAPE_CASES, ids=lambda v: str(v))
def test_luts_and_full_call_as_single_frames(gpu, h, w, only):
    names, fr, luts, outs = R.cases_with_ref(h, w, only=only)
    for i, name in enumerate(names):
        assert np.array_equal(luts_of(gpu, fr[i:i + 1])[0], luts[i]), f"{name} at {h}x{w}: look-up tables"
        got = run(gpu, fr[i])
        assert got.shape == (1, h, w, 3)
        assert np.array_equal(got[0], outs[i]), f"{name} at {h}x{w}: " + describe(got, outs[i:i + 1], [name])


def test_uniform_frame_gives_identical_luts(gpu):
    names, fr, luts, outs = R.cases_with_ref(50, 70)
    got = luts_of(gpu, fr[names.index("grey")][None])[0]
    assert (got == got[0, 0]).all()


@pytest.mark.parametrize("clip_limit,tile_grid", [(2.0, (4, 2)), (40.0, (8, 8))], ids=lambda v: str(v))
def test_other_grids_and_clip_limits(gpu, clip_limit, tile_grid):
    names, fr, luts, outs = R.cases_with_ref(72, 104, clip_limit, tile_grid)
    got = luts_of(gpu, fr, clip_limit, tile_grid)
    assert np.array_equal(got, luts), describe(got, luts, names)
    got = run(gpu, fr, clip_limit=clip_limit, tile_grid=tile_grid)
    assert np.array_equal(got, outs), describe(got, outs, names)
    base = R.cases_with_ref(72, 104)[3]
    assert not np.array_equal(outs, base)                       # the arguments matter


def test_launches_3_and_4_compose_the_call(gpu):
    names, fr, luts, outs = R.cases_with_ref(64, 70)
    f = torch.from_numpy(np.array(fr)).to(gpu)
    B = f.shape[0]
    p = ipu.clahe_params(64, 70)
    ctx = N.shared_context(gpu.index)
    ws = torch.zeros(int(ctx.lib.bugseg_clahe_workspace_bytes(ctypes.byref(p), B)), dtype=torch.uint8, device=gpu)
    assert ws.numel() == B * 64 * 256
    ctx.clahe(f, B, p, None, stage=3, workspace=ws)
    assert np.array_equal(ws.cpu().numpy().reshape(luts.shape), luts)
    out = torch.zeros_like(f)
    ctx.clahe(f, B, p, out, stage=4, workspace=ws)
    assert np.array_equal(out.cpu().numpy(), outs)


def test_reference_signature(gpu):
    names, fr, luts, outs = R.cases_with_ref(120, 160)
    i = names.index("scene")
    a = np.array(fr[i])
    out = ipu.clahe(a)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == a.shape and out.flags.owndata
    assert np.array_equal(out, outs[i]) and np.array_equal(a, fr[i])
    assert np.array_equal(ipu.clahe(torch.from_numpy(a)), outs[i])
    assert np.array_equal(ipu.clahe(torch.from_numpy(a).to(gpu)), outs[i])


@pytest.fixture(scope="module")
def some():
    names, fr, luts, outs = R.cases_with_ref(50, 70)
    pick = [names.index(n) for n in ("noise", "scene", "primaries")]
    return fr[pick], outs[pick]


def test_two_calls_are_identical(gpu, some):
    fr, outs = some
    a, b = run(gpu, fr), run(gpu, fr)
    assert np.array_equal(a, b) and np.array_equal(a, outs)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_workspace_contents_do_not_matter(gpu, some, fill):
    fr, outs = some
    B, h, w = fr.shape[:3]
    p = ipu.clahe_params(h, w)
    ctx = N.shared_context(gpu.index)
    n = int(ctx.lib.bugseg_clahe_workspace_bytes(ctypes.byref(p), B))
    assert n >= B * 64 * 256
    ws = torch.full((n,), fill, dtype=torch.uint8, device=gpu)
    f = torch.from_numpy(np.array(fr)).to(gpu)
    out = torch.empty_like(f)
    ctx.clahe(f, B, p, out, workspace=ws)
    assert np.array_equal(out.cpu().numpy(), outs)


def test_side_stream(gpu, some):
    fr, outs = some
    f = torch.from_numpy(np.array(fr)).to(gpu)
    torch.cuda.synchronize(gpu)
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        out = ipu.clahe_device(f)
    st.synchronize()
    assert np.array_equal(out.cpu().numpy(), outs)


def test_first_call_of_a_context_captured_and_replayed(gpu):
    """A context of its own: its conversion tables are uploaded inside the capture."""
    names, fr, luts, outs = R.cases_with_ref(50, 70)
    a, b = names.index("noise"), names.index("scene")
    ctx = N.Context(gpu.index, N.FP32)
    p = ipu.clahe_params(50, 70)
    f = torch.from_numpy(np.array(fr[a:a + 1])).to(gpu)
    out = torch.zeros_like(f)
    ws = torch.zeros(int(ctx.lib.bugseg_clahe_workspace_bytes(ctypes.byref(p), 1)), dtype=torch.uint8, device=gpu)
    gc.collect()                                    # no finalizer of an earlier test's garbage inside the capture
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            ctx.clahe(f, 1, p, out, workspace=ws)
    finally:
        gc.enable()
    f.copy_(torch.from_numpy(np.array(fr[b:b + 1])).to(gpu))
    graph.replay()
    torch.cuda.synchronize(gpu)
    assert not np.array_equal(outs[a], outs[b])
    assert np.array_equal(out[0].cpu().numpy(), outs[b])
    del graph
    ctx.close()


def test_refusals_launch_nothing(gpu):
    h, w, B = 50, 70, 2
    ctx = N.shared_context(gpu.index)
    f = torch.full((B, h, w, 3), 9, dtype=torch.uint8, device=gpu)
    out = torch.full((B, h, w, 3), 7, dtype=torch.uint8, device=gpu)
    good = ipu.clahe_params(h, w)
    ws = torch.full((int(ctx.lib.bugseg_clahe_workspace_bytes(ctypes.byref(good), B)),), 5, dtype=torch.uint8, device=gpu)

    def params(**kw):
        p = ipu.clahe_params(h, w)
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(p=params(tiles_x=0)), dict(p=params(tiles_y=17)),
           dict(p=params(rows=15)), dict(p=params(cols=15)), dict(p=params(clip_limit=0.0)),
           dict(p=params(clip_limit=-3.0)), dict(p=params(clip_limit=float("nan"))),
           dict(p=params(clip_limit=float("inf"))), dict(p=params(rows=1 << 15, cols=1 << 15)),
           dict(workspace=ws[:ws.numel() - 256]), dict(out=f), dict(out=f.view(-1)[3:]), dict(workspace=out.view(-1))]
    for case in bad:
        with pytest.raises(N.BugsegError) as e:
            ctx.clahe(f, case.get("B", B), case.get("p", good), case.get("out", out), workspace=case.get("workspace", ws))
        assert e.value.code == N.EINVAL and "clahe" in str(e.value), case
    for st in (-1, 5):
        with pytest.raises(N.BugsegError) as e:
            ctx.clahe(f, B, good, out, stage=st, workspace=ws)
        assert e.value.code == N.EINVAL
    # a NULL workspace
    rc = ctx.lib.bugseg_clahe_bgr(ctx.h, f.data_ptr(), B, ctypes.byref(good), out.data_ptr(), None, 0, N.stream_handle(None))
    assert rc == N.EINVAL and b"workspace" in ctx.lib.bugseg_last_error(ctx.h)
    assert ctx.lib.bugseg_clahe_workspace_bytes(ctypes.byref(params(tiles_x=0)), B) == 0
    torch.cuda.synchronize(gpu)
    assert bool((out == 7).all()) and bool((f == 9).all()) and bool((ws == 5).all())
    ctx.clahe(f, B, good, out, workspace=ws)
    want = R.clahe(np.full((h, w, 3), 9, np.uint8))
    assert np.array_equal(out.cpu().numpy(), np.stack([want, want]))
