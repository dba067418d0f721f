"""The Hough transform on the device (csrc/hough_kernels.hip) against the NumPy restatement of its pinned semantics
(tests/hough_ref.py), bit for bit: lines as float32 bit patterns, counts, peaks and the stage-0 accumulators on every
structured case at every shape, parameter set, threshold and max_lines; the camera-sized frame whose peaks exceed
any LDS sort; peak finding and selection alone on hand-made accumulators; and the call's run-time properties
(batches with empty frames, views at odd offsets, repeatable, independent of the workspace's contents, any stream,
capturable, refusals launch nothing)."""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

import hough_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import image_processing_utils as ipu

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(got, want, what):
    lines, counts, peaks = (t.cpu().numpy() for t in got)
    assert lines.dtype == np.float32 and counts.dtype == np.int32 and peaks.dtype == np.int32
    assert np.array_equal(peaks, want[2]), f"{what}: peaks {peaks.tolist()} for {want[2].tolist()}"
    assert np.array_equal(counts, want[1]), f"{what}: counts {counts.tolist()} for {want[1].tolist()}"
    bad = np.argwhere(bits(lines) != bits(want[0]))
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0]}: {lines[tuple(bad[0])]} for {want[0][tuple(bad[0])]}"


def stage0(ctx, x, p, trig):
    B = x.shape[0]
    acc = torch.full((B, p.numangle + 2, p.numrho + 2), 0x55555555, dtype=torch.int32, device=x.device)
    ctx.hough(x, B, p, trig, None, None, None, stage=0, acc=acc)
    return acc.cpu().numpy()


def stage1(ctx, acc, p):
    B = acc.shape[0]
    lines = torch.full((B, p.max_lines, 2), 7.0, dtype=torch.float32, device=acc.device)
    counts = torch.full((B,), -1, dtype=torch.int32, device=acc.device)
    peaks = torch.full((B,), -1, dtype=torch.int32, device=acc.device)
    ctx.hough(None, B, p, None, lines, counts, peaks, stage=1, acc=acc)
    return lines, counts, peaks


@pytest.mark.parametrize("k", range(len(R.PARAM_SETS)), ids=lambda k: f"set{k}")
@pytest.mark.parametrize("h,w", R.SHAPES, ids=lambda v: str(v))
def test_every_case_as_one_batch(gpu, h, w, k):
    rho, theta, lo, hi = R.PARAM_SETS[k]
    par, tab, acc = R.accumulators(h, w, k)
    x = torch.from_numpy(np.array(R.images(h, w))).to(gpu)
    ctx = N.shared_context(gpu.index)
    p = ipu.hough_params(h, w, rho, theta, 0, 1, lo, hi)
    got_acc = stage0(ctx, x, p, ipu.hough_trig_device(gpu, p))
    for i, name in enumerate(R.CASE_NAMES):
        assert np.array_equal(got_acc[i], acc[i]), f"accumulator of {name} at {h}x{w}, set {k}"
    for thr in R.thresholds(h, w):
        for ml in R.MAX_LINES:
            got = ipu.hough_lines_device(x, rho, theta, thr, ml, lo, hi)
            assert got[0].shape == (len(R.CASE_NAMES), ml, 2)
            check(got, R.cases_with_ref(h, w, k, thr, ml), f"{h}x{w}, set {k}, threshold {thr}, max_lines {ml}")


@pytest.mark.parametrize("h,w", [(17, 65), (100, 100)], ids=lambda v: str(v))
def test_every_case_as_a_single_frame(gpu, h, w):
    rho, theta, lo, hi = R.PARAM_SETS[0]
    thr = R.thresholds(h, w)[1]
    want = R.cases_with_ref(h, w, 0, thr, 3)
    for i, name in enumerate(R.CASE_NAMES):
        got = ipu.hough_lines_device(torch.from_numpy(np.array(R.images(h, w)[i])).to(gpu), rho, theta, thr, 3, lo, hi)
        check(got, tuple(a[i:i + 1] for a in want[:3]), f"{name} at {h}x{w}")


@pytest.mark.parametrize("ml", R.BIG_CASE["max_lines"])
def test_camera_sized_frame_with_more_peaks_than_any_sort_holds(gpu, ml):
    par, acc = R.big_accumulator()
    rho, theta, lo, hi = R.PARAM_SETS[0]
    thr = R.BIG_CASE["threshold"]
    x = torch.from_numpy(np.array(R.big_edges())).to(gpu).unsqueeze(0)
    lines, count, peaks, votes = R.select(acc, par, thr, ml)
    assert peaks == R.BIG_CASE["peaks"] and count == ml
    check(ipu.hough_lines_device(x, rho, theta, thr, ml, lo, hi),
          (lines[None], np.array([count], np.int32), np.array([peaks], np.int32)), f"480x640, max_lines {ml}")
    if ml == R.MAX_LINES_CAP:
        p = ipu.hough_params(*R.BIG, rho, theta, thr, ml, lo, hi)
        got = stage0(N.shared_context(gpu.index), x, p, ipu.hough_trig_device(gpu, p))
        assert np.array_equal(got[0], acc)
        with pytest.raises(ValueError, match=str(R.BIG_CASE["peaks"])):
            ipu.hough_lines(np.array(R.big_edges()), rho, theta, thr)


@pytest.mark.parametrize("geo", R.HAND_GEOMETRIES, ids=lambda v: str(v))
def test_peaks_and_selection_alone_on_hand_made_accumulators(gpu, geo):
    rows, cols, div = geo
    par = R.hand_params(*geo)
    accs = R.hand_accumulators(*geo)
    ctx = N.shared_context(gpu.index)
    a = torch.from_numpy(np.array(accs)).to(gpu)
    for thr in (0, 4):
        for ml in (1, 5, R.MAX_LINES_CAP):
            p = ipu.hough_params(rows, cols, 1.0, math.pi / div, thr, ml)
            assert (p.numangle, p.numrho) == (par["numangle"], par["numrho"])
            res = [R.select(x, par, thr, ml) for x in accs]
            want = (np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32))
            check(stage1(ctx, a, p), want, f"{geo}, threshold {thr}, max_lines {ml}")
            i = R.HAND_NAMES.index("checker_equal")
            check(stage1(ctx, a[i:i + 1].contiguous(), p), tuple(v[i:i + 1] for v in want), f"{geo} checkerboard alone")


@pytest.fixture(scope="module")
def mixed():
    """Different frames with empty ones between them, and their reference at threshold 12, max_lines 5."""
    h, w = 48, 80
    pick = [R.CASE_NAMES.index(n) for n in ("empty", "edges", "empty", "noise", "parallel", "empty", "full", "corners")]
    want = R.cases_with_ref(h, w, 0, 12, 5)
    return np.array(R.images(h, w)[pick]), tuple(a[pick] for a in want[:3])


ARGS = (1.0, math.pi / 180, 12, 5)


def test_batch_with_empty_frames_equals_singles(gpu, mixed):
    im, want = mixed
    assert (want[2] == 0).sum() >= 3 and (want[2] > 5).sum() >= 2 and len(set(want[2].tolist())) >= 4
    check(ipu.hough_lines_device(torch.from_numpy(im).to(gpu), *ARGS), want, "batch")
    for j in range(len(im)):
        check(ipu.hough_lines_device(torch.from_numpy(im[j]).to(gpu), *ARGS), tuple(a[j:j + 1] for a in want), f"frame {j}")


def test_views_at_odd_byte_offsets(gpu, mixed):
    im, want = mixed
    B, h, w = im.shape
    n = B * h * w
    for off in (1, 3, 7):
        src = torch.zeros(n + 16, dtype=torch.uint8, device=gpu)
        x = src[off:off + n].view(B, h, w)
        x.copy_(torch.from_numpy(im))
        assert x.data_ptr() % 2 == 1 and x.is_contiguous()
        check(ipu.hough_lines_device(x, *ARGS), want, f"offset {off}")


def test_two_calls_are_identical(gpu, mixed):
    im, want = mixed
    x = torch.from_numpy(im).to(gpu)
    a, b = ipu.hough_lines_device(x, *ARGS), ipu.hough_lines_device(x, *ARGS)
    check(a, want, "first")
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("fill", [0xFF, 0x00, 0x01])
def test_workspace_contents_do_not_matter(gpu, mixed, fill):
    im, want = mixed
    B, h, w = im.shape
    p = ipu.hough_params(h, w, *ARGS)
    ctx = N.shared_context(gpu.index)
    ws = torch.full((int(ctx.lib.bugseg_hough_workspace_bytes(ctypes.byref(p), B)),), fill, dtype=torch.uint8, device=gpu)
    x = torch.from_numpy(im).to(gpu)
    lines = torch.full((B, 5, 2), 3.0, dtype=torch.float32, device=gpu)
    counts, peaks = torch.full((B,), -1, dtype=torch.int32, device=gpu), torch.full((B,), -1, dtype=torch.int32, device=gpu)
    ctx.hough(x, B, p, ipu.hough_trig_device(gpu, p), lines, counts, peaks, workspace=ws)
    check((lines, counts, peaks), want, f"workspace filled with {fill:#x}")


def test_side_stream(gpu, mixed):
    im, want = mixed
    x = torch.from_numpy(im).to(gpu)
    ipu.hough_lines_device(x, *ARGS)
    torch.cuda.synchronize(gpu)
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        got = ipu.hough_lines_device(x, *ARGS)
    st.synchronize()
    check(got, want, "side stream")


def test_captured_and_replayed_after_the_input_changed(gpu):
    h, w = 57, 71                                   # a shape no other test uses, on a context of its own
    rho, theta, thr, ml = 1.0, math.pi / 180, 6, 9
    a, b = R.canny_ref.canny(R.canny_ref.scene(h, w, seed=1), 50, 150), R.canny_ref.canny(R.canny_ref.scene(h, w, seed=2), 50, 150)
    ctx = N.Context(gpu.index, N.FP32)
    p = ipu.hough_params(h, w, rho, theta, thr, ml)
    trig = ipu.hough_trig_device(gpu, p)            # before the capture
    x = torch.from_numpy(a).to(gpu).unsqueeze(0).contiguous()
    lines = torch.zeros((1, ml, 2), dtype=torch.float32, device=gpu)
    counts, peaks = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(int(ctx.lib.bugseg_hough_workspace_bytes(ctypes.byref(p), 1)), dtype=torch.uint8, device=gpu)
    gc.collect()                                    # no finalizer of an earlier test's garbage inside the capture
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            ctx.hough(x, 1, p, trig, lines, counts, peaks, workspace=ws)
    finally:
        gc.enable()
    x.copy_(torch.from_numpy(b).to(gpu).unsqueeze(0))
    graph.replay()
    torch.cuda.synchronize(gpu)
    wa, wb = R.hough(a, rho, theta, thr, ml), R.hough(b, rho, theta, thr, ml)
    assert wb[1] > 0 and not np.array_equal(bits(wa[0]), bits(wb[0]))
    check((lines, counts, peaks), (wb[0][None], np.array([wb[1]], np.int32), np.array([wb[2]], np.int32)), "replay")
    ctx.close()


def test_refusals_launch_nothing(gpu):
    h, w, B = 20, 70, 2
    ctx = N.shared_context(gpu.index)
    x = torch.zeros((B, h, w), dtype=torch.uint8, device=gpu)
    x[:, :, w // 2] = 255
    good = ipu.hough_params(h, w, 1.0, math.pi / 180, 10, 4)
    trig = ipu.hough_trig_device(gpu, good)
    lines = torch.full((B, 4, 2), 7.0, dtype=torch.float32, device=gpu)
    counts, peaks = torch.full((B,), 7, dtype=torch.int32, device=gpu), torch.full((B,), 7, dtype=torch.int32, device=gpu)
    acc = torch.full((B, good.numangle + 2, good.numrho + 2), 7, dtype=torch.int32, device=gpu)
    ws = torch.zeros(int(ctx.lib.bugseg_hough_workspace_bytes(ctypes.byref(good), B)), dtype=torch.uint8, device=gpu)

    def params(**kw):
        p = ipu.hough_params(h, w, 1.0, math.pi / 180, 10, 4)
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    bad = [dict(B=0), dict(B=-1), dict(B=65536), dict(p=params(rows=0)), dict(p=params(cols=0)), dict(p=params(rows=65536)),
           dict(p=params(numrho=good.numrho + 1)), dict(p=params(numrho=good.numrho - 1)), dict(p=params(numrho=0)),
           dict(p=params(numangle=0)), dict(p=params(numangle=65537)), dict(p=params(max_lines=0)), dict(p=params(max_lines=4097)),
           dict(p=params(rho=0.0)), dict(p=params(rho=-1.0)), dict(p=params(rho=float("inf"))), dict(p=params(theta=0.0)),
           dict(p=params(theta=float("nan"))), dict(p=params(min_theta=float("inf"))),
           dict(p=params(rows=3413, cols=3413, numrho=13653)), dict(p=params(rows=40000, cols=40000, numrho=160001)),
           dict(workspace=ws[:ws.numel() - 512])]
    for stg in (None, 0, 1):
        for case in bad:
            with pytest.raises(N.BugsegError) as e:
                ctx.hough(x, case.get("B", B), case.get("p", good), trig, lines, counts, peaks, stage=stg, acc=acc,
                          workspace=case.get("workspace", ws))
            assert e.value.code == N.EINVAL, (stg, case)
    # overlapping buffers: the lines inside the workspace, counts and peaks sharing a word, the image inside the lines
    n = B * 4 * 2 * 4
    with pytest.raises(N.BugsegError):
        ctx.hough(x, B, good, trig, ws[:n].view(torch.float32).view(B, 4, 2), counts, peaks, workspace=ws)
    both = torch.full((B + 1,), 7, dtype=torch.int32, device=gpu)
    with pytest.raises(N.BugsegError):
        ctx.hough(x, B, good, trig, lines, both[:B], both[1:], workspace=ws)
    with pytest.raises(N.BugsegError):
        ctx.hough(ws[:B * h * w].view(B, h, w), B, good, trig, lines, counts, peaks, workspace=ws)
    with pytest.raises(N.BugsegError) as e:
        ctx.hough(x, B, good, trig, lines, counts, peaks, stage=2, acc=acc, workspace=ws)
    assert e.value.code == N.EINVAL
    # NULL arguments
    sh = N.stream_handle(None)
    for args in ((None, trig.data_ptr(), lines.data_ptr(), counts.data_ptr(), peaks.data_ptr(), ws.data_ptr(), ws.numel()),
                 (x.data_ptr(), None, lines.data_ptr(), counts.data_ptr(), peaks.data_ptr(), ws.data_ptr(), ws.numel()),
                 (x.data_ptr(), trig.data_ptr(), None, counts.data_ptr(), peaks.data_ptr(), ws.data_ptr(), ws.numel()),
                 (x.data_ptr(), trig.data_ptr(), lines.data_ptr(), None, peaks.data_ptr(), ws.data_ptr(), ws.numel()),
                 (x.data_ptr(), trig.data_ptr(), lines.data_ptr(), counts.data_ptr(), None, ws.data_ptr(), ws.numel()),
                 (x.data_ptr(), trig.data_ptr(), lines.data_ptr(), counts.data_ptr(), peaks.data_ptr(), None, 0)):
        rc = ctx.lib.bugseg_hough_lines(ctx.h, args[0], B, ctypes.byref(good), *args[1:], sh)
        assert rc == N.EINVAL, args
    assert b"workspace" in ctx.lib.bugseg_last_error(ctx.h)
    torch.cuda.synchronize(gpu)
    assert bool((lines == 7.0).all()) and bool((counts == 7).all()) and bool((peaks == 7).all()) and bool((acc == 7).all())
    assert bool((ws == 0).all()) and bool((both == 7).all())
    ctx.hough(x, B, good, trig, lines, counts, peaks, workspace=ws)
    want = R.hough(x[0].cpu().numpy(), 1.0, math.pi / 180, 10, 4)
    assert want[1] >= 1 and want[0][0, 0] == w // 2 and want[0][0, 1] == 0
    check((lines, counts, peaks), (np.stack([want[0]] * 2), np.array([want[1]] * 2, np.int32), np.array([want[2]] * 2, np.int32)), "after the refusals")


def test_device_entry_refusals(gpu):
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=gpu)
    for bad in (x.cpu(), x.to(torch.int8), x.unsqueeze(0), x[0, 0], x[:0]):
        with pytest.raises(ValueError):
            ipu.hough_lines_device(bad, 1, math.pi / 180, 3)
    for kw in (dict(rho=0), dict(theta=float("nan")), dict(max_lines=0), dict(max_lines=4097), dict(min_theta=2.0, max_theta=1.0)):
        a = dict(rho=1, theta=math.pi / 180, threshold=3)
        a.update(kw)
        with pytest.raises(ValueError):
            ipu.hough_lines_device(x, **a)


def test_host_form(gpu):
    h, w = 48, 80
    par, tab, acc = R.accumulators(h, w, 0)
    i = R.CASE_NAMES.index("edges")
    im = np.array(R.images(h, w)[i])
    lines, count, peaks, _ = R.select(acc[i], par, 12, R.MAX_LINES_CAP)
    assert 0 < count == peaks
    got = ipu.hough_lines(im, 1.0, math.pi / 180, 12)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (count, 1, 2) and got.flags.owndata
    assert np.array_equal(bits(got[:, 0]), bits(lines[:count]))
    assert np.array_equal(bits(ipu.hough_lines(torch.from_numpy(im).to(gpu), 1.0, math.pi / 180, 12)), bits(got))
    assert ipu.hough_lines(im, 1.0, math.pi / 180, h * w) is None
    assert ipu.hough_lines(np.zeros((h, w), np.uint8), 1.0, math.pi / 180, 0) is None
