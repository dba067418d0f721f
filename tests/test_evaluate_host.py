"""Host side of the device evaluation (evaluate.py): the metrics, the parameter checks, the
table builders, and the NumPy restatement (tests/evaluate_ref.py) against torch.bincount on the CPU for every
case the GPU tests use. No GPU."""
import numpy as np
import pytest
import torch

import evaluate_ref as R
from bugcar_image_segmentation_amd import evaluate as E


def same_metrics(a, b, rtol=1e-12):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_allclose(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), rtol=rtol, atol=0,
                                   equal_nan=True, err_msg=k)


def test_metrics_perfect():
    m = np.diag([5, 7, 11]).astype(np.int64)
    r = E.metrics(m)
    assert np.array_equal(r["iou"], [1.0, 1.0, 1.0]) and r["miou"] == 1.0 and r["pixel_accuracy"] == 1.0
    assert np.array_equal(r["class_accuracy"], [1.0, 1.0, 1.0]) and r["fw_iou"] == 1.0 and r["pixels"] == 23
    same_metrics(r, R.metrics(m))


def test_metrics_all_wrong():
    m = np.array([[0, 4], [6, 0]], dtype=np.int64)
    r = E.metrics(m)
    assert np.array_equal(r["iou"], [0.0, 0.0]) and r["miou"] == 0.0 and r["pixel_accuracy"] == 0.0
    assert np.array_equal(r["class_accuracy"], [0.0, 0.0]) and r["fw_iou"] == 0.0
    same_metrics(r, R.metrics(m))


def test_metrics_absent_class_is_nan_and_left_out_of_miou():
    m = np.array([[3, 1, 0], [2, 4, 0], [0, 0, 0]], dtype=np.int64)
    r = E.metrics(m)
    assert np.isnan(r["iou"][2]) and np.isnan(r["class_accuracy"][2])
    assert r["iou"][0] == 3 / 6 and r["iou"][1] == 4 / 7
    assert r["miou"] == np.mean([3 / 6, 4 / 7])
    assert r["pixel_accuracy"] == 7 / 10
    assert r["fw_iou"] == pytest.approx(4 / 10 * 3 / 6 + 6 / 10 * 4 / 7, rel=1e-15)
    same_metrics(r, R.metrics(m))
    # a class that is only predicted has IoU 0 (its union is not empty) and no class accuracy
    m2 = np.array([[3, 0, 2], [0, 4, 0], [0, 0, 0]], dtype=np.int64)
    r2 = E.metrics(m2)
    assert r2["iou"][2] == 0.0 and np.isnan(r2["class_accuracy"][2]) and r2["miou"] == np.mean([3 / 5, 1.0, 0.0])
    same_metrics(r2, R.metrics(m2))


def test_metrics_empty_is_nan_not_an_exception():
    r = E.metrics(np.zeros((4, 4), dtype=np.int64))
    assert np.isnan(r["iou"]).all() and np.isnan(r["class_accuracy"]).all()
    assert all(np.isnan(r[k]) for k in ("miou", "pixel_accuracy", "mean_class_accuracy", "fw_iou")) and r["pixels"] == 0
    same_metrics(r, R.metrics(np.zeros((4, 4))))
    with pytest.raises(ValueError):
        E.metrics(np.zeros((3, 4)))


def test_metrics_agree_with_the_restatement_on_random_matrices():
    rng = np.random.default_rng(0)
    for C in (1, 2, 15, 21, 64):
        m = rng.integers(0, 1 << 40, (C, C), dtype=np.int64)
        m[rng.integers(0, C)] = 0
        same_metrics(E.metrics(m), R.metrics(m))


def test_confusion_params_refusals():
    ident = np.arange(256, dtype=np.uint8)
    for C in (0, -1, 65, 1.5, 1000):
        with pytest.raises(ValueError, match="num_classes"):
            E.confusion_params((4, 4), (4, 4), C)
    for pred_hw, gt_hw in (((0, 4), (4, 4)), ((4, 0), (4, 4)), ((4, 4), (0, 4)), ((4, 4), (4, -2))):
        with pytest.raises(ValueError, match="empty"):
            E.confusion_params(pred_hw, gt_hw, 3)
    for bad in (ident[:255], ident.astype(np.int16), ident.astype(np.int8), np.zeros((2, 128), np.uint8), list(range(255))):
        with pytest.raises(ValueError, match="256 uint8"):
            E.confusion_params((4, 4), (4, 4), 3, pred_lut=bad)
        with pytest.raises(ValueError, match="256 uint8"):
            E.confusion_params((4, 4), (4, 4), 3, gt_lut=bad)
    with pytest.raises(ValueError):
        E.Evaluator(65)                          # refused before any device is asked for
    with pytest.raises(ValueError):
        E.Evaluator(3, pred_lut=ident[:10])


def test_confusion_params_fields():
    lut = R.lut3_of_15()
    p = E.confusion_params((12, 20), (30, 50), 3, pred_lut=lut)
    assert (p.pred_rows, p.pred_cols, p.gt_rows, p.gt_cols, p.num_classes) == (12, 20, 30, 50, 3)
    assert np.array_equal(np.frombuffer(bytes(p.pred_lut), np.uint8), lut)
    assert np.array_equal(np.frombuffer(bytes(p.gt_lut), np.uint8), np.arange(256))
    for C in (1, 64):
        assert E.confusion_params((1, 1), (1, 1), C).num_classes == C


def test_table_builders():
    from bugcar_image_segmentation_amd.models import class_lut3, class_lut_binary
    assert np.array_equal(E.identity_lut(), np.arange(256))
    assert np.array_equal(E.class_lut(class_lut3(15, (0, 1), (2, 9))), R.lut3_of_15())
    assert np.array_equal(E.class_lut(class_lut_binary(15, (0, 1))), R.binary_of_15())
    assert np.array_equal(E.class_lut([1, 0], fill=7), [1, 0] + [7] * 254)
    for bad in ([], [300], [-1], np.zeros((2, 2), np.uint8), [0.5]):
        with pytest.raises(ValueError):
            E.class_lut(bad)
    g = E.ignore_lut([3, 255])
    assert g[3] == E.SKIP and g[255] == E.SKIP and g[4] == 4 and g.dtype == np.uint8
    assert np.array_equal(E.ignore_lut([3], base=E.class_lut(np.arange(15, dtype=np.uint8))), R.gt_ignore_lut())
    with pytest.raises(ValueError):
        E.ignore_lut([256])
    gl = E.grid_lut()
    assert (gl[255], gl[0], gl[100]) == (0, 1, 2) and (np.delete(gl, [0, 100, 255]) == E.SKIP).all()
    grid = np.array([-1, 0, 100, 50], dtype=np.int8)
    assert np.array_equal(gl[grid.view(np.uint8)], [0, 1, 2, E.SKIP])


def torch_accumulator(pred, gt, C, pred_lut, gt_lut):
    """The cross-check: what a user would write with torch on the CPU. The nearest rule is restated here with
    torch integer division, the tables with torch indexing."""
    p, g = torch.from_numpy(pred).long(), torch.from_numpy(gt).long()
    gh, gw = g.shape[1:]
    ph, pw = p.shape[1:]
    ys = torch.clamp(torch.div(torch.arange(gh) * ph, gh, rounding_mode="floor"), max=ph - 1)
    xs = torch.clamp(torch.div(torch.arange(gw) * pw, gw, rounding_mode="floor"), max=pw - 1)
    p = p[:, ys][:, :, xs]
    if pred_lut is not None:
        p = torch.from_numpy(pred_lut).long()[p]
    if gt_lut is not None:
        g = torch.from_numpy(gt_lut).long()[g]
    ok = (g < C) & (p < C)
    acc = torch.bincount(g[ok] * C + p[ok], minlength=C * C)
    return torch.cat([acc, (~ok).sum().reshape(1)]).numpy()


def test_restatement_equals_torch_bincount_on_every_gpu_case():
    n = 0
    for name, pred, gt, C, pl, gl in R.gpu_cases():
        want = R.accumulator(pred, gt, C, pl, gl)
        assert want.sum() == gt.size, name
        assert np.array_equal(want, torch_accumulator(pred, gt, C, pl, gl)), name
        n += 1
    assert n == len(R.CLASSES) * len(R.SHAPES) * len(R.CONTENTS) + 3 + 4 + 1


def test_the_named_ratio_where_the_double_rule_differs():
    # 44 label columns against 30 prediction columns: 22 * 30 // 44 = 15, but 22 * (30 / 44.) = 14.999999999999998
    assert R.differing_ratio() == (44, 30, 22)
    assert R.nearest_index(44, 30)[22] == 15 and R.nearest_index_double(44, 30)[22] == 14
    # and the rule is the identity for equal sizes, and never leaves the source
    for n in (1, 7, 640):
        assert np.array_equal(R.nearest_index(n, n), np.arange(n))
    for nd, ns in ((30, 12), (12, 30), (14, 122), (1, 9), (9, 1)):
        i = R.nearest_index(nd, ns)
        assert i.min() >= 0 and i.max() <= ns - 1 and (np.diff(i) >= 0).all()
