"""The device confusion matrix (csrc/eval_kernels.hip, evaluate.py) against the NumPy
restatement (tests/evaluate_ref.py), exact on every integer, at the smallest shapes where the kernel can go
wrong: below one vector, a ragged end, several workgroups, every path (vectors, bytes, resampling), every
number of private copies of the bins (C = 64 has two, C = 1 to 21 sixteen)."""
import gc
import json
import os

import numpy as np
import pytest
import torch

import evaluate_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import evaluate as E

pytestmark = pytest.mark.gpu

_CASES = {}


def cases():
    """evaluate_ref.gpu_cases() with its expected accumulators, computed once and shared read-only."""
    if not _CASES:
        for name, pred, gt, C, pl, gl in R.gpu_cases():
            want = R.accumulator(pred, gt, C, pl, gl)
            for a in (pred, gt, want):
                a.setflags(write=False)
            _CASES[name] = (pred, gt, C, pl, gl, want)
    return _CASES


def dev(gpu, a):
    return torch.from_numpy(np.array(a)).to(gpu)


def run(gpu, pred, gt, C, pl=None, gl=None, out=None):
    return E.confusion_device(dev(gpu, pred), dev(gpu, gt), C, pred_lut=pl, gt_lut=gl, out=out)


@pytest.mark.parametrize("C", R.CLASSES)
def test_shapes_and_contents(gpu, C):
    n = 0
    for name, (pred, gt, c, pl, gl, want) in cases().items():
        if c != C or name.split("-")[0] not in R.CONTENTS:
            continue
        got = run(gpu, pred, gt, C).cpu().numpy()
        assert got.dtype == np.int64 and got.shape == (C * C + 1,)
        assert np.array_equal(got, want), name
        assert got.sum() == gt.size, name
        n += 1
    assert n == len(R.SHAPES) * len(R.CONTENTS)


@pytest.mark.parametrize("name", ["gt-ignore", "pred-lut3", "pred-binary"])
def test_tables(gpu, name):
    pred, gt, C, pl, gl, want = cases()[name]
    got = run(gpu, pred, gt, C, pl, gl).cpu().numpy()
    assert np.array_equal(got, want) and got.sum() == gt.size
    assert 0 < got[-1] < gt.size or name == "pred-binary"


@pytest.mark.parametrize("name", ["resample-12x20-to-30x50", "resample-30x50-to-12x20", "resample-5x122-to-3x14"])
def test_nearest_rule(gpu, name):
    pred, gt, C, pl, gl, want = cases()[name]
    got = run(gpu, pred, gt, C).cpu().numpy()
    assert np.array_equal(got, want) and got.sum() == gt.size


def test_nearest_rule_is_the_integer_one_where_doubles_differ(gpu):
    """44 label columns (and rows) against 30: at index 22 the integer rule reads source 15, the
    double-precision expression floor(22 * (30 / 44.)) reads 14 (evaluate_ref.differing_ratio)."""
    pred, gt, C, pl, gl, want = cases()["resample-30x30-to-44x44"]
    assert R.nearest_index(44, 30)[22] == 15 and R.nearest_index_double(44, 30)[22] == 14
    ys, xs = R.nearest_index_double(44, 30), R.nearest_index_double(44, 30)
    other = R.accumulator(np.ascontiguousarray(pred[:, ys][:, :, xs]), gt, C)
    assert not np.array_equal(other, want)                   # the two rules give different matrices on this input
    assert np.array_equal(run(gpu, pred, gt, C).cpu().numpy(), want)


def test_views_at_odd_byte_offsets(gpu):
    pred, gt, C, pl, gl, want = cases()["random-31x64-C15"]
    B, h, w = gt.shape
    n = B * h * w
    # contiguous maps that start at odd bytes: equally far from a 16-byte boundary (vectors behind a head of
    # bytes, a tail of bytes) and not (bytes only)
    for off_p, off_g in ((1, 1), (3, 19), (5, 2), (7, 0), (0, 13)):
        bp = torch.zeros(n + 32, dtype=torch.uint8, device=gpu)
        bg = torch.zeros(n + 32, dtype=torch.uint8, device=gpu)
        p, g = bp[off_p:off_p + n].view(B, h, w), bg[off_g:off_g + n].view(B, h, w)
        p.copy_(dev(gpu, pred))
        g.copy_(dev(gpu, gt))
        assert p.is_contiguous() and g.is_contiguous() and (p.data_ptr() % 16, g.data_ptr() % 16) == (off_p % 16, off_g % 16)
        assert np.array_equal(E.confusion_device(p, g, C).cpu().numpy(), want), (off_p, off_g)
    # rows and columns sliced out of larger maps: the base and the row pitch are odd
    big_p = torch.full((B, h + 3, w + 5), 9, dtype=torch.uint8, device=gpu)
    big_g = torch.full((B, h + 3, w + 5), 9, dtype=torch.uint8, device=gpu)
    p, g = big_p[:, 1:1 + h, 2:2 + w], big_g[:, 2:2 + h, 1:1 + w]
    p.copy_(dev(gpu, pred))
    g.copy_(dev(gpu, gt))
    assert not p.is_contiguous() and p.stride(1) % 2 == 1 and p.data_ptr() % 2 == 1 and g.data_ptr() % 2 == 1
    assert np.array_equal(E.confusion_device(p, g, C).cpu().numpy(), want)


@pytest.mark.parametrize("B", [1, 3])
def test_batch_equals_the_sum_of_single_frames(gpu, B):
    rng = np.random.default_rng(B)
    pred, gt = rng.integers(0, 17, (B, 7, 33), dtype=np.uint8), rng.integers(0, 17, (B, 7, 33), dtype=np.uint8)
    whole = run(gpu, pred, gt, 15).cpu().numpy()
    singles = sum(run(gpu, pred[i], gt[i], 15).cpu().numpy() for i in range(B))      # (h, w) maps
    assert np.array_equal(whole, singles) and np.array_equal(whole, R.accumulator(pred, gt, 15))


def test_accumulation_invariant_and_repeatability(gpu):
    a, b = cases()["random-50x50-C21"], cases()["halves-50x50-C21"]
    out = torch.zeros(21 * 21 + 1, dtype=torch.int64, device=gpu)
    assert run(gpu, a[0], a[1], 21, out=out) is out
    run(gpu, b[0], b[1], 21, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(got, a[5] + b[5])
    assert got.sum() == a[1].size + b[1].size                  # every label pixel seen is counted once
    # the same calls again give the same bits
    again = torch.zeros_like(out)
    run(gpu, a[0], a[1], 21, out=again)
    run(gpu, b[0], b[1], 21, out=again)
    assert torch.equal(again, out)
    # a start that is not zero is kept
    out2 = torch.full_like(out, 5)
    run(gpu, a[0], a[1], 21, out=out2)
    assert np.array_equal(out2.cpu().numpy(), a[5] + 5)


def test_side_stream(gpu):
    pred, gt, C, pl, gl, want = cases()["checkerboard-31x64-C15"]
    p, g = dev(gpu, pred), dev(gpu, gt)
    torch.cuda.synchronize(gpu)
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        out = E.confusion_device(p, g, C)
    st.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_first_call_captured_and_replayed_twice(gpu):
    h, w, C = 37, 53, 9                                        # a shape and a class count no other test uses
    rng = np.random.default_rng(5)
    pred, gt = rng.integers(0, C + 1, (2, h, w), dtype=np.uint8), rng.integers(0, C + 1, (2, h, w), dtype=np.uint8)
    ctx = N.Context(gpu.index, N.FP32)                         # a context of its own: its first call
    params = E.confusion_params((h, w), (h, w), C)
    p, g = dev(gpu, pred), dev(gpu, gt)
    acc = torch.zeros(C * C + 1, dtype=torch.int64, device=gpu)
    gc.collect()                                               # no finalizer of an earlier test's garbage inside the capture
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            ctx.confusion(p, g, 2, params, acc)
    finally:
        gc.enable()
    torch.cuda.synchronize(gpu)
    assert int(acc.sum()) == 0                                 # capturing ran nothing
    want = R.accumulator(pred, gt, C)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(acc.cpu().numpy(), 2 * want)
    ctx.close()


def test_refusals_launch_nothing(gpu):
    h, w, B, C = 6, 10, 2, 3
    ctx = N.shared_context(gpu.index)
    x = torch.ones((B, h, w), dtype=torch.uint8, device=gpu)
    out = torch.full((C * C + 1,), 7, dtype=torch.int64, device=gpu)
    good = E.confusion_params((h, w), (h, w), C)

    def params(**kw):
        p = E.confusion_params((h, w), (h, w), C)
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    bad = [dict(B=0), dict(B=-1), dict(p=params(num_classes=0)), dict(p=params(num_classes=65)), dict(p=params(gt_rows=0)),
           dict(p=params(pred_cols=0)), dict(p=params(gt_cols=-4)),
           dict(p=params(gt_rows=1 << 16, gt_cols=1 << 15)), dict(p=params(pred_rows=1 << 16, pred_cols=1 << 15)),
           dict(B=1 << 20, p=params(gt_rows=1 << 6, gt_cols=1 << 6, pred_rows=1 << 6, pred_cols=1 << 6)),
           dict(B=1, p=params(gt_rows=1 << 16, gt_cols=1, pred_rows=1 << 15, pred_cols=1))]
    for case in bad:
        with pytest.raises(N.BugsegError) as e:
            ctx.confusion(x, x, case.get("B", B), case.get("p", good), out)
        assert e.value.code == N.EINVAL, case
    # a NULL argument, an accumulator that is not 8-byte aligned
    import ctypes
    rc = ctx.lib.bugseg_confusion(ctx.h, x.data_ptr(), None, B, ctypes.byref(good), out.data_ptr(), N.stream_handle(None))
    assert rc == N.EINVAL and b"NULL" in ctx.lib.bugseg_last_error(ctx.h)
    rc = ctx.lib.bugseg_confusion(ctx.h, x.data_ptr(), x.data_ptr(), B, ctypes.byref(good), out.data_ptr() + 4,
                                  N.stream_handle(None))
    assert rc == N.EINVAL and b"aligned" in ctx.lib.bugseg_last_error(ctx.h)
    # the public entry: every check before any device work, `out` untouched
    for bad_call in (lambda: E.confusion_device(x, x, 65, out=out), lambda: E.confusion_device(x, x, 0, out=out),
                     lambda: E.confusion_device(x, x[:1], C, out=out), lambda: E.confusion_device(x.cpu(), x, C, out=out),
                     lambda: E.confusion_device(x.to(torch.int32), x, C, out=out),
                     lambda: E.confusion_device(x, x, C, pred_lut=np.zeros(255, np.uint8), out=out),
                     lambda: E.confusion_device(x, x, C, out=out[:-1]), lambda: E.confusion_device(x, x, C, out=out.to(torch.int32)),
                     lambda: E.confusion_device(x[:, :0], x[:, :0], C, out=out), lambda: E.confusion_device(x[:0], x[:0], C, out=out)):
        with pytest.raises(ValueError):
            bad_call()
    torch.cuda.synchronize(gpu)
    assert bool((out == 7).all())
    E.confusion_device(x, x, C, out=out)
    want = np.full(C * C + 1, 7, dtype=np.int64)
    want[1 * C + 1] += B * h * w
    assert np.array_equal(out.cpu().numpy(), want)


def test_camera_sized_frames(gpu):
    pred, gt, C, pl, gl, want = cases()["camera"]
    assert gt.shape == (4, 480, 640) and C == 15
    got = run(gpu, pred, gt, C).cpu().numpy()
    assert np.array_equal(got, want) and got.sum() == gt.size


def test_uniform_batch_does_not_overflow_a_workgroups_bins(gpu):
    """B = 8 uniform 480 x 640 maps: one bin takes all 2,457,600 pixels."""
    gt = torch.full((8, 480, 640), 4, dtype=torch.uint8, device=gpu)
    pred = torch.full((8, 480, 640), 11, dtype=torch.uint8, device=gpu)
    got = E.confusion_device(pred, gt, 15).cpu().numpy()
    want = np.zeros(15 * 15 + 1, dtype=np.int64)
    want[4 * 15 + 11] = 2457600
    assert np.array_equal(got, want)


def test_int8_grids_of_the_reference_glue_geometries(gpu):
    """Evaluator.for_grids() on the fixture's grids: the laserscan-like grids as predictions against the plain
    ones as labels, int8 as the rasteriser writes them, one update per geometry and all of them summed."""
    fix = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_glue.npz")
    ev = E.Evaluator.for_grids()
    assert ev.num_classes == 3
    total = np.zeros(10, dtype=np.int64)
    with np.load(fix, allow_pickle=False) as z:
        for g in ("bench", "small_neg", "small_odd"):
            gt, pred = z[f"{g}/plain/occgrid"], z[f"{g}/ls/occgrid"]
            assert gt.dtype == np.int8 and pred.dtype == np.int8 and json.loads(bytes(z[f"{g}/json"]).decode())
            want = R.accumulator(pred, gt, 3, E.grid_lut(), E.grid_lut())
            assert 0 < want[-1] < gt.size and want.sum() == gt.size     # the fixture's maps hold other bytes too: skipped
            one = E.Evaluator.for_grids()
            one.update(torch.from_numpy(pred).to(gpu), torch.from_numpy(gt).to(gpu))      # int8 device tensors
            assert np.array_equal(one.confusion(), R.matrix(want, 3)) and one.skipped() == want[-1]
            ev.update(pred, gt)                                                          # NumPy arrays, copied up
            total += want
    assert np.array_equal(ev.confusion(), R.matrix(total, 3)) and ev.skipped() == total[-1]
    got, ref = ev.metrics(), R.metrics(R.matrix(total, 3))
    for k in ref:
        np.testing.assert_allclose(np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64), rtol=1e-12, atol=0, equal_nan=True)
    # a byte that is no grid value is skipped
    odd = np.array([[[-1, 0, 100, 50]]], dtype=np.int8)
    ev.reset()
    ev.update(odd, odd)
    assert np.array_equal(ev.confusion(), np.eye(3, dtype=np.int64)) and ev.skipped() == 1


def test_evaluator_update_reset_and_metrics(gpu):
    a, b = cases()["random-31x64-C15"], cases()["gt-ignore"]
    ev = E.Evaluator(15, gt_lut=R.gt_ignore_lut())
    ev.update(dev(gpu, a[0]), dev(gpu, a[1]))
    ev.update(b[0], b[1])
    want = R.accumulator(a[0], a[1], 15, None, R.gt_ignore_lut()) + b[5]
    assert np.array_equal(ev.confusion(), R.matrix(want, 15)) and ev.skipped() == want[-1]
    got, ref = ev.metrics(), R.metrics(R.matrix(want, 15))
    for k in ref:
        np.testing.assert_allclose(np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64), rtol=1e-12, atol=0, equal_nan=True)
    ev.reset()
    assert not ev.confusion().any() and ev.skipped() == 0
    assert np.isnan(ev.metrics()["miou"])
