"""find_quad on the device (csrc/quad_kernels.hip) against the NumPy restatement of its pinned semantics
(tests/quad_ref.py), bit for bit: status, threshold, area, root, corners and moments of find_tile_device and the
moments of the second bugseg_quad_moments pass, on every case at every shape; find_tile's float corners to 1e-9 px;
and the call's run-time properties (a batch of mixed statuses equals its frames one by one, views at odd offsets,
repeatable, independent of the workspace's contents, any stream, capturable, refusals launch nothing)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import quad_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import calibration as C

pytestmark = pytest.mark.gpu

INTS = ("status", "threshold", "area", "root", "corners", "moments")


def args_of(p):
    return dict(bright=p["bright"], threshold=p["threshold"], min_area=p["min_area"], band=p["band"])


def want_of(refs):
    w = {k: R.stacked(refs, k) for k in ("threshold", "area", "root", "corners", "moments")}
    w["status"] = R.stacked(refs, "status0")
    return w


def check(got, refs, what, names=None):
    want = want_of(refs)
    for k in INTS:
        g = got[k].cpu().numpy()
        assert g.dtype == (np.int64 if k == "moments" else np.int32) and g.shape == want[k].shape, (what, k)
        bad = np.argwhere(g != want[k])
        assert bad.size == 0, f"{what}: {k} differs first at {bad[0].tolist()}" + (f" ({names[bad[0][0]]})" if names else "") + \
            f": {g[tuple(bad[0])]} for {want[k][tuple(bad[0])]}"


def check_host(got, refs, what):
    assert np.array_equal(got["status"], R.stacked(refs, "status")), what
    assert np.array_equal(got["coarse"], R.stacked(refs, "corners")) and np.array_equal(got["area"], R.stacked(refs, "area")), what
    assert np.array_equal(got["threshold"], R.stacked(refs, "threshold")) and np.array_equal(got["counts"], R.stacked(refs, "counts")), what
    assert got["corners"].dtype == np.float64 and np.abs(got["corners"] - R.stacked(refs, "refined")).max() <= 1e-9, what


def second_pass(x, refs, p):
    """bugseg_quad_moments with the restatement's rounded corners against the restatement's second moments."""
    c2 = torch.from_numpy(R.stacked(refs, "corners2")).to(x.device)
    a = args_of(p)
    a.pop("band")
    got = C.quad_moments_device(x, c2, p["band"][1], **a).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, R.stacked(refs, "moments2"))


@pytest.mark.parametrize("which", R.GROUPS)
@pytest.mark.parametrize("h,w", R.SHAPES, ids=lambda v: str(v))
def test_every_case_as_one_batch(gpu, h, w, which):
    names, frames, p, refs = R.group(h, w, which)
    x = torch.from_numpy(np.array(frames)).to(gpu)
    check(C.find_tile_device(x, **args_of(p)), refs, f"{which} at {h}x{w}", names)
    second_pass(x, refs, p)
    check_host(C.find_tile(x, **args_of(p)), refs, f"{which} at {h}x{w}")


def test_camera_sized_frames(gpu):
    names, frames, p, refs = R.big_group()
    x = torch.from_numpy(np.array(frames)).to(gpu)
    check(C.find_tile_device(x, **args_of(p)), refs, "480x640", names)
    second_pass(x, refs, p)
    check_host(C.find_tile(np.array(frames), **args_of(p)), refs, "480x640")


@pytest.fixture(scope="module")
def mixed():
    """99 x 130 (two tiles wide, seven high): frames of every status, and their reference."""
    names, frames, p, refs = R.group(99, 130, "grey")
    assert {r["status0"] for r in refs} == {R.OK, R.NO_TILE, R.DEGENERATE}
    return np.array(frames), p, refs


def test_batch_of_mixed_statuses_equals_singles(gpu, mixed):
    im, p, refs = mixed
    check(C.find_tile_device(torch.from_numpy(im).to(gpu), **args_of(p)), refs, "batch")
    for j in range(len(im)):
        check(C.find_tile_device(torch.from_numpy(im[j]).to(gpu), **args_of(p)), refs[j:j + 1], f"frame {j}")
    back = im[::-1].copy()
    check(C.find_tile_device(torch.from_numpy(back).to(gpu), **args_of(p)), refs[::-1], "reversed batch")


def test_views_at_odd_byte_offsets(gpu, mixed):
    im, p, refs = mixed
    n = im.size
    for off in (1, 3, 7):
        src = torch.zeros(n + 16, dtype=torch.uint8, device=gpu)
        x = src[off:off + n].view(im.shape)
        x.copy_(torch.from_numpy(im))
        assert x.data_ptr() % 2 == 1 and x.is_contiguous()
        check(C.find_tile_device(x, **args_of(p)), refs, f"offset {off}")
    names, frames, pb, rb = R.group(50, 67, "bgr")
    src = torch.zeros(frames.size + 16, dtype=torch.uint8, device=gpu)
    x = src[5:5 + frames.size].view(frames.shape)
    x.copy_(torch.from_numpy(np.array(frames)))
    check(C.find_tile_device(x, **args_of(pb)), rb, "BGR at offset 5")


def test_two_calls_are_identical(gpu, mixed):
    im, p, refs = mixed
    x = torch.from_numpy(im).to(gpu)
    a, b = C.find_tile_device(x, **args_of(p)), C.find_tile_device(x, **args_of(p))
    check(a, refs, "first")
    for k in INTS:
        assert torch.equal(a[k], b[k]), k


def outputs(B, gpu, fill):
    o = [torch.full((B,), fill, dtype=torch.int32, device=gpu) for _ in range(4)]
    o.append(torch.full((B, 4, 2), fill, dtype=torch.int32, device=gpu))
    o.append(torch.full((B, 4, 6), fill, dtype=torch.int64, device=gpu))
    return o


@pytest.mark.parametrize("fill", [0xFF, 0x00, 0x01])
def test_workspace_contents_do_not_matter(gpu, mixed, fill):
    im, p, refs = mixed
    B, h, w = im.shape
    qp = C.quad_params(h, w, channels=1, **args_of(p))
    ctx = N.shared_context(gpu.index)
    ws = torch.full((int(ctx.lib.bugseg_quad_workspace_bytes(ctypes.byref(qp), B)),), fill, dtype=torch.uint8, device=gpu)
    x = torch.from_numpy(im).to(gpu)
    o = outputs(B, gpu, -3)
    ctx.find_quad(x, B, qp, *o, workspace=ws)
    check(dict(zip(INTS, o)), refs, f"workspace filled with {fill:#x}")
    ws.fill_(fill)
    mom = torch.full((B, 4, 6), -3, dtype=torch.int64, device=gpu)
    ctx.quad_moments(x, B, qp, p["band"][1], torch.from_numpy(R.stacked(refs, "corners2")).to(gpu), mom, workspace=ws)
    assert np.array_equal(mom.cpu().numpy(), R.stacked(refs, "moments2"))


def test_side_stream(gpu, mixed):
    im, p, refs = mixed
    x = torch.from_numpy(im).to(gpu)
    C.find_tile_device(x, **args_of(p))
    torch.cuda.synchronize(gpu)
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        got = C.find_tile_device(x, **args_of(p))
    st.synchronize()
    check(got, refs, "side stream")


def test_captured_and_replayed_after_the_input_changed(gpu):
    h, w = 57, 71                                   # a shape no other test uses, on a context of its own
    p = R.params(h, w)
    a = R.render(h, w, R.scaled("tilted", h, w), 60, 200, 4.0, 5)
    b = R.from_mask(R.masks(h, w)["diamond"], seed=6)
    ra, rb = R.find_tile(a, p), R.find_tile(b, p)
    assert ra["status0"] == R.OK and rb["status0"] == R.OK and not np.array_equal(ra["corners"], rb["corners"])
    ctx = N.Context(gpu.index, N.FP32)
    qp = C.quad_params(h, w, channels=1)
    x = torch.from_numpy(a).to(gpu).unsqueeze(0).contiguous()
    o = outputs(1, gpu, 0)
    ws = torch.empty(int(ctx.lib.bugseg_quad_workspace_bytes(ctypes.byref(qp), 1)), dtype=torch.uint8, device=gpu)
    gc.collect()                                    # no finalizer of an earlier test's garbage inside the capture
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            ctx.find_quad(x, 1, qp, *o, workspace=ws)
    finally:
        gc.enable()
    x.copy_(torch.from_numpy(b).to(gpu).unsqueeze(0))
    graph.replay()
    torch.cuda.synchronize(gpu)
    check(dict(zip(INTS, o)), [rb], "replay")
    ctx.close()


def test_refusals_launch_nothing(gpu):
    h, w, B = 20, 70, 2
    ctx = N.shared_context(gpu.index)
    x = torch.from_numpy(np.stack([R.from_mask(R.masks(h, w)["rect"], seed=s) for s in (1, 2)])).to(gpu)
    good = C.quad_params(h, w, channels=1)
    o = outputs(B, gpu, 7)
    c2 = torch.full((B, 4, 2), 7, dtype=torch.int32, device=gpu)
    ws = torch.zeros(int(ctx.lib.bugseg_quad_workspace_bytes(ctypes.byref(good), B)), dtype=torch.uint8, device=gpu)

    def params(**kw):
        p = C.quad_params(h, w, channels=1)
        for name, v in kw.items():
            if name == "band":
                p.band[0], p.band[1] = v
            else:
                setattr(p, name, v)
        return p

    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(p=params(rows=2)), dict(p=params(cols=2)), dict(p=params(rows=4097)),
           dict(p=params(cols=4097)), dict(p=params(rows=0)), dict(p=params(channels=0)), dict(p=params(channels=2)),
           dict(p=params(channels=4)), dict(p=params(min_area=0)), dict(p=params(band=(65, 2))), dict(p=params(band=(3, -1))),
           dict(workspace=ws[:ws.numel() - 512])]
    for case in bad:
        for stage in (None, 0, 11):
            with pytest.raises(N.BugsegError) as e:
                ctx.find_quad(x, case.get("B", B), case.get("p", good), *o, stage=stage, workspace=case.get("workspace", ws))
            assert e.value.code == N.EINVAL, (stage, case)
        with pytest.raises(N.BugsegError) as e:
            ctx.quad_moments(x, case.get("B", B), case.get("p", good), 2, c2, o[5], workspace=case.get("workspace", ws))
        assert e.value.code == N.EINVAL, case
        assert ctx.lib.bugseg_quad_workspace_bytes(ctypes.byref(case.get("p", good)), case.get("B", B)) == 0 or "workspace" in case
    for band in (-1, 65):
        with pytest.raises(N.BugsegError):
            ctx.quad_moments(x, B, good, band, c2, o[5], workspace=ws)
    for stage in (-1, 12):
        with pytest.raises(N.BugsegError):
            ctx.find_quad(x, B, good, *o, stage=stage, workspace=ws)
    # overlapping buffers: the moments inside the workspace, status and threshold sharing a word, the frames inside the workspace
    with pytest.raises(N.BugsegError):
        ctx.find_quad(x, B, good, *o[:5], ws[:B * 24 * 8].view(torch.int64).view(B, 4, 6), workspace=ws)
    both = torch.full((B + 1,), 7, dtype=torch.int32, device=gpu)
    with pytest.raises(N.BugsegError):
        ctx.find_quad(x, B, good, both[:B], both[1:], *o[2:], workspace=ws)
    with pytest.raises(N.BugsegError):
        ctx.find_quad(ws[:B * h * w].view(B, h, w), B, good, *o, workspace=ws)
    with pytest.raises(N.BugsegError):
        ctx.quad_moments(x, B, good, 2, c2, c2.view(torch.int64), workspace=ws)      # the moments start where the corners do
    # a misaligned moments buffer, NULL arguments
    odd = torch.full((B * 24 * 2 + 1,), 7, dtype=torch.int32, device=gpu)
    with pytest.raises(N.BugsegError):
        ctx.find_quad(x, B, good, *o[:5], odd[1:], workspace=ws)
    for k in range(7):
        a = [x] + o
        a[k] = None
        with pytest.raises(N.BugsegError):
            ctx.find_quad(a[0], B, good, *a[1:], workspace=ws)
    with pytest.raises(N.BugsegError):
        ctx.quad_moments(x, B, good, 2, None, o[5], workspace=ws)
    rc = ctx.lib.bugseg_find_quad(ctx.h, x.data_ptr(), B, ctypes.byref(good), *[t.data_ptr() for t in o], None, 0, N.stream_handle(None))
    assert rc == N.EINVAL and b"workspace" in ctx.lib.bugseg_last_error(ctx.h)
    torch.cuda.synchronize(gpu)
    assert all(bool((t == 7).all()) for t in o + [c2, both, odd]) and bool((ws == 0).all())
    ctx.find_quad(x, B, good, *o, workspace=ws)
    refs = [R.find_tile(f, R.params(h, w)) for f in x.cpu().numpy()]
    assert all(r["status0"] == R.OK for r in refs)
    check(dict(zip(INTS, o)), refs, "after the refusals")


def test_device_entry_refusals(gpu):
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=gpu)
    for bad in (x.cpu(), x.to(torch.int8), x[0, 0], x[:0], x[:, :2], torch.zeros((1, 1, 8, 8, 3), dtype=torch.uint8, device=gpu),
                torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=gpu)):
        with pytest.raises(ValueError):
            C.find_tile_device(bad)
    for kw in (dict(threshold=255), dict(min_area=0), dict(band=(70, 2)), dict(band=3)):
        with pytest.raises(ValueError):
            C.find_tile_device(x, **kw)
    with pytest.raises(ValueError):
        C.quad_moments_device(x, torch.zeros((2, 4, 2), dtype=torch.int64, device=gpu), 2)
    with pytest.raises(ValueError):
        C.find_tile(np.zeros((8, 8), np.float32))
