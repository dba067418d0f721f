"""NumPy restatement of the device evaluation, written out independently of
bugcar_image_segmentation_amd/evaluate.py: the tables, the integer nearest rule, np.bincount, the metrics.
There is no reference program for this feature; this file is the tests' oracle, and test_evaluate_host.py
checks it against torch.bincount on the CPU."""
from __future__ import annotations

import numpy as np


def nearest_index(n_dst: int, n_src: int) -> np.ndarray:
    """Source index of each of n_dst positions: min(i * n_src // n_dst, n_src - 1), exact in integers."""
    i = np.arange(n_dst, dtype=np.int64)
    return np.minimum(i * n_src // n_dst, n_src - 1)


def nearest_index_double(n_dst: int, n_src: int) -> np.ndarray:
    """What OpenCV's INTER_NEAREST computes instead: min(floor(i * (n_src / n_dst)), n_src - 1) in doubles."""
    i = np.arange(n_dst, dtype=np.float64)
    return np.minimum(np.floor(i * (float(n_src) / float(n_dst))).astype(np.int64), n_src - 1)


def resample(pred: np.ndarray, gt_hw) -> np.ndarray:
    """(B, ph, pw) -> (B, gh, gw) by the integer nearest rule; the identity when the shapes are equal."""
    ys, xs = nearest_index(gt_hw[0], pred.shape[1]), nearest_index(gt_hw[1], pred.shape[2])
    return pred[:, ys][:, :, xs]


def accumulator(pred, gt, C: int, pred_lut=None, gt_lut=None) -> np.ndarray:
    """int64 [C * C + 1]: the matrix row by row (rows = labels), then the skipped pixels."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.dtype == np.int8:
        pred = pred.view(np.uint8)
    if gt.dtype == np.int8:
        gt = gt.view(np.uint8)
    assert pred.dtype == np.uint8 and gt.dtype == np.uint8
    if pred.ndim == 2:
        pred = pred[None]
    if gt.ndim == 2:
        gt = gt[None]
    assert pred.shape[0] == gt.shape[0]
    p = resample(pred, gt.shape[1:]).astype(np.int64)
    g = gt.astype(np.int64)
    if pred_lut is not None:
        p = np.asarray(pred_lut, dtype=np.int64)[p]
    if gt_lut is not None:
        g = np.asarray(gt_lut, dtype=np.int64)[g]
    ok = (g < C) & (p < C)
    acc = np.zeros(C * C + 1, dtype=np.int64)
    acc[: C * C] = np.bincount(g[ok] * C + p[ok], minlength=C * C)
    acc[C * C] = int((~ok).sum())
    return acc


def matrix(acc, C: int) -> np.ndarray:
    return np.asarray(acc)[: C * C].reshape(C, C)


def metrics(m) -> dict:
    """The figures, class by class in plain loops (float64)."""
    m = np.asarray(m, dtype=np.float64)
    C = m.shape[0]
    nan = float("nan")
    total = float(m.sum())
    iou, acc = np.full(C, nan), np.full(C, nan)
    for c in range(C):
        tp, row, col = m[c, c], m[c, :].sum(), m[:, c].sum()
        if row + col - tp > 0:
            iou[c] = tp / (row + col - tp)
        if row > 0:
            acc[c] = tp / row
    seen = [v for v in iou if not np.isnan(v)]
    lab = [v for v in acc if not np.isnan(v)]
    fw = nan
    if total > 0:
        fw = float(sum(m[c, :].sum() / total * iou[c] for c in range(C) if m[c, :].sum() > 0))
    return {"iou": iou, "miou": float(np.mean(seen)) if seen else nan,
            "pixel_accuracy": float(np.trace(m) / total) if total > 0 else nan,
            "class_accuracy": acc, "mean_class_accuracy": float(np.mean(lab)) if lab else nan,
            "fw_iou": fw, "pixels": int(total)}


# ---------------------------------------------------------------- the cases the GPU tests use
SHAPES = [(1, 1), (1, 17), (7, 33), (16, 16), (31, 64), (50, 50)]
CONTENTS = ["uniform", "checkerboard", "random", "halves"]
CLASSES = [1, 2, 15, 21, 64]


def content(kind: str, B: int, h: int, w: int, C: int, seed: int) -> np.ndarray:
    """A (B, h, w) u8 map with values below C + 2: the two values C and C + 1 (where they occur) are out of
    range and land in the skipped slot."""
    rng = np.random.default_rng(seed)
    top = C + 2 if C < 64 else C          # C = 64 keeps every value a class, so the whole matrix is in play
    if kind == "uniform":
        return np.full((B, h, w), int(rng.integers(0, C)), dtype=np.uint8)
    if kind == "checkerboard":
        a, b = (int(v) for v in rng.integers(0, top, 2))
        yy, xx = np.mgrid[0:h, 0:w]
        return np.broadcast_to(np.where((yy + xx) % 2 == 0, a, b).astype(np.uint8), (B, h, w)).copy()
    if kind == "random":
        return rng.integers(0, top, (B, h, w), dtype=np.uint8)
    if kind == "halves":
        a, b = (int(v) for v in rng.integers(0, top, 2))
        m = np.full((B, h, w), a, dtype=np.uint8)
        m[:, :, w // 2:] = b
        return m
    raise ValueError(kind)


def pair(kind: str, B: int, h: int, w: int, C: int, seed: int):
    """(pred, gt) of one case: the label map has the content, the prediction the same content from another
    seed with a band of rows copied from the labels, so that the diagonal and the rest are both filled."""
    gt = content(kind, B, h, w, C, seed)
    pred = content(kind, B, h, w, C, seed + 1000)
    pred[:, : h // 2] = gt[:, : h // 2]
    return pred, gt


def differing_ratio(limit: int = 64):
    """The first (n_dst, n_src, i), n_src < n_dst <= limit, where the double-precision nearest index differs
    from the integer one; None if there is none."""
    for n_dst in range(2, limit + 1):
        for n_src in range(1, n_dst):
            a, b = nearest_index(n_dst, n_src), nearest_index_double(n_dst, n_src)
            d = np.nonzero(a != b)[0]
            if d.size:
                return n_dst, n_src, int(d[0])
    return None


def lut3_of_15() -> np.ndarray:
    """models.py:56-58 as a 256-entry prediction table: ids 0, 1 -> 1 (road), 2, 9 -> 0 (flat), the other ENet
    ids -> 2, bytes past 14 -> 255 (skipped)."""
    lut = np.full(256, 255, dtype=np.uint8)
    lut[:15] = 2
    lut[[2, 9]] = 0
    lut[[0, 1]] = 1
    return lut


def binary_of_15() -> np.ndarray:
    """models.py:79-80: ids 0, 1 -> 1, the other ENet ids -> 0, bytes past 14 -> 255 (skipped)."""
    lut = np.full(256, 255, dtype=np.uint8)
    lut[:15] = 0
    lut[[0, 1]] = 1
    return lut


def gt_ignore_lut() -> np.ndarray:
    """A label table with ignore labels: ids 0..14 themselves, 3 and 255 ignored, and (as datasets with a
    'void' id above the classes do) 19 ignored; every other byte also maps past the classes."""
    lut = np.full(256, 255, dtype=np.uint8)
    lut[:15] = np.arange(15)
    lut[3] = 255
    return lut


def gpu_cases():
    """Every (name, pred, gt, C, pred_lut, gt_lut) the GPU tests compare with accumulator(): the shape x content
    x class grid at B = 2, the table cases, the resampling cases, the camera-sized case. test_evaluate_host.py
    runs the same list against torch.bincount on the CPU."""
    seed = 0
    for C in CLASSES:
        for h, w in SHAPES:
            for kind in CONTENTS:
                seed += 1
                pred, gt = pair(kind, 2, h, w, C, seed)
                yield f"{kind}-{h}x{w}-C{C}", pred, gt, C, None, None
    rng = np.random.default_rng(77)
    gt = rng.integers(0, 21, (2, 31, 64), dtype=np.uint8)
    gt[0, :3] = 255
    pred = rng.integers(0, 16, (2, 31, 64), dtype=np.uint8)
    yield "gt-ignore", pred, gt, 15, None, gt_ignore_lut()
    g3 = rng.integers(0, 3, (2, 31, 64), dtype=np.uint8)
    yield "pred-lut3", pred, g3, 3, lut3_of_15(), None
    yield "pred-binary", pred, (g3 & 1).astype(np.uint8), 2, binary_of_15(), None
    for (ph, pw), (gh, gw) in (((12, 20), (30, 50)), ((30, 50), (12, 20)), ((30, 30), (44, 44)), ((5, 122), (3, 14))):
        p = rng.integers(0, 15, (3, ph, pw), dtype=np.uint8)
        g = rng.integers(0, 17, (3, gh, gw), dtype=np.uint8)
        yield f"resample-{ph}x{pw}-to-{gh}x{gw}", p, g, 15, None, None
    pred, gt = pair("random", 4, 480, 640, 15, 4242)
    gt[:, 200:280] = 3                       # and uniform bands, as class maps have
    pred[:, 240:300] = 3
    yield "camera", pred, gt, 15, None, None
