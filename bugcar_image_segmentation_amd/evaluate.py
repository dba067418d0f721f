"""Evaluation of segmenters on the device: batched confusion matrix, IoU and accuracy.

The reference's README names `evaluate_model.py` ("to evaluate the accuracy of this ENET model",
README.md:14); the script is not in the snapshot, so there is nothing to restate. This module does the
job: predicted u8 class maps and u8 label maps, both in device memory, go through one kernel
(csrc/eval_kernels.hip, bugseg_confusion) that adds into an int64 accumulator of C * C + 1 words on the
device. No class map reaches the host; the host reads the accumulator once, when the matrix is asked for,
and `metrics` turns it into IoU and accuracy figures in float64.

    confusion[g, p]  label pixels whose label maps to class g and whose prediction maps to class p
    skipped          label pixels whose label or prediction maps to no class (a byte >= C after its table)

Evaluation is at the labels' resolution. Where the prediction has another shape it is read at the integer
nearest position sy = min(y * ph // gh, ph - 1), sx = min(x * pw // gw, pw - 1).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

MAX_CLASSES = 64
SKIP = 255            # a table entry no evaluation has as a class (C <= 64): the pixel is counted as skipped


# ---------------------------------------------------------------- tables
def identity_lut() -> np.ndarray:
    """Byte b -> class b."""
    return np.arange(256, dtype=np.uint8)


def class_lut(table, fill: int = SKIP) -> np.ndarray:
    """A table of n <= 256 entries (models.class_lut3 / class_lut_binary give such, one byte per class id of
    a network) -> the 256-entry table the kernel takes: bytes past the table map to `fill` (skipped)."""
    t = np.asarray(table)
    if t.ndim != 1 or not 1 <= t.shape[0] <= 256:
        raise ValueError("a class table holds 1..256 entries")
    if t.dtype != np.uint8:
        if not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() > 255:
            raise ValueError("class table entries must be bytes (0..255)")
        t = t.astype(np.uint8)
    if int(fill) != fill or not 0 <= fill <= 255:
        raise ValueError("fill must be a byte (0..255)")
    lut = np.full(256, int(fill), dtype=np.uint8)
    lut[: t.shape[0]] = t
    return lut


def ignore_lut(ignore, base=None) -> np.ndarray:
    """`base` (default: the identity) with every id of `ignore` sent to SKIP: a label table for datasets
    that mark unlabelled pixels with ids such as 255 or 19."""
    lut = identity_lut() if base is None else _lut256("base", base).copy()
    for v in ignore:
        k = int(v)
        if k != v or not 0 <= k <= 255:
            raise ValueError(f"ignore id {v!r} is not a byte (0..255)")
        lut[k] = SKIP
    return lut


def grid_lut() -> np.ndarray:
    """Occupancy grid bytes (int8 cells read as uint8) -> {unknown, free, occupied}: 255 (-1) -> 0, 0 -> 1,
    100 -> 2, every other byte -> SKIP."""
    lut = np.full(256, SKIP, dtype=np.uint8)
    lut[255], lut[0], lut[100] = 0, 1, 2
    return lut


def _lut256(name: str, lut) -> np.ndarray:
    a = np.asarray(lut)
    if a.dtype != np.uint8 or a.shape != (256,):
        raise ValueError(f"{name} must be 256 uint8 values, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


# ---------------------------------------------------------------- the kernel's parameters
def confusion_params(pred_hw, gt_hw, num_classes, pred_lut=None, gt_lut=None) -> N.ConfusionParams:
    """bugseg_confusion_params, with every check before any device work: ValueError for num_classes outside
    1..64, an empty map, a table that is not 256 uint8 values. None is the identity table."""
    C = int(num_classes)
    if C != num_classes or not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"num_classes must be 1..{MAX_CLASSES}, got {num_classes!r}")
    ph, pw = (int(v) for v in pred_hw)
    gh, gw = (int(v) for v in gt_hw)
    if ph < 1 or pw < 1:
        raise ValueError(f"the prediction map is empty: {ph} x {pw}")
    if gh < 1 or gw < 1:
        raise ValueError(f"the label map is empty: {gh} x {gw}")
    pl = identity_lut() if pred_lut is None else _lut256("pred_lut", pred_lut)
    gl = identity_lut() if gt_lut is None else _lut256("gt_lut", gt_lut)
    p = N.ConfusionParams()
    p.pred_rows, p.pred_cols, p.gt_rows, p.gt_cols, p.num_classes = ph, pw, gh, gw, C
    p.pred_lut[:] = pl.tolist()
    p.gt_lut[:] = gl.tolist()
    return p


def _maps(name: str, t) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint8, torch.int8):
        raise ValueError(f"{name} must be a uint8 (or int8) device tensor")
    if t.dtype == torch.int8:
        t = t.view(torch.uint8)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f"{name} must have shape (B, h, w) or (h, w)")
    return t.contiguous()


def confusion_device(pred: torch.Tensor, gt: torch.Tensor, num_classes, *, pred_lut=None, gt_lut=None,
                     out: torch.Tensor | None = None, params: N.ConfusionParams | None = None) -> torch.Tensor:
    """(B, ph, pw) or (ph, pw) predictions against (B, gh, gw) or (gh, gw) labels, uint8 device tensors (int8
    grids are read as uint8) -> the int64 device tensor [C * C + 1]: the matrix row by row (rows = labels),
    then the skipped pixels. On the current stream; nothing synchronises. `out` is added into when given (a
    contiguous int64 tensor of that size on the maps' device) and is a new zeroed tensor otherwise. `params`:
    a confusion_params() result for these shapes, classes and tables, to save building it per call."""
    p_, g_ = _maps("pred", pred), _maps("gt", gt)
    if p_.device != g_.device:
        raise ValueError(f"pred is on {p_.device}, gt on {g_.device}")
    if p_.shape[0] != g_.shape[0]:
        raise ValueError(f"pred holds {p_.shape[0]} frames, gt {g_.shape[0]}")
    B = int(g_.shape[0])
    if params is None:
        params = confusion_params(p_.shape[1:], g_.shape[1:], num_classes, pred_lut, gt_lut)
    elif (params.pred_rows, params.pred_cols, params.gt_rows, params.gt_cols, params.num_classes) != \
            (*p_.shape[1:], *g_.shape[1:], int(num_classes)):
        raise ValueError("params were built for other shapes or another class count")
    if B < 1:
        raise ValueError("the maps hold no frame")
    n = int(num_classes) ** 2 + 1
    if out is None:
        out = torch.zeros(n, dtype=torch.int64, device=g_.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (n,) or out.dtype != torch.int64 \
            or not out.is_contiguous() or out.device != g_.device:
        raise ValueError(f"out must be a contiguous int64 tensor of shape {(n,)} on {g_.device}")
    with torch.cuda.device(g_.device):
        N.shared_context(g_.device.index).confusion(p_, g_, B, params, out, torch.cuda.current_stream(g_.device))
    return out


# ---------------------------------------------------------------- host metrics
def metrics(confusion) -> dict:
    """Figures of a (C, C) confusion matrix (rows = labels), in float64. With TP the diagonal, row the row
    sums (label pixels per class) and col the column sums (predicted pixels per class):
      iou[c] = TP / (row + col - TP), NaN where the class is in neither map; miou: the mean of the others
      pixel_accuracy = sum(TP) / sum; class_accuracy[c] = TP / row (NaN for a class without label pixels);
      mean_class_accuracy: the mean of the others; fw_iou = sum over classes with label pixels of row / sum * iou.
    An empty matrix gives NaN everywhere, not an exception."""
    m = np.asarray(confusion)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError(f"a confusion matrix is square, got {m.shape}")
    m = m.astype(np.float64)
    tp, row, col = np.diag(m), m.sum(axis=1), m.sum(axis=0)
    total = m.sum()
    union = row + col - tp
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, tp / union, nan)
        acc = np.where(row > 0, tp / row, nan)
    seen, labelled = union > 0, row > 0
    return {
        "iou": iou,
        "miou": float(iou[seen].mean()) if seen.any() else nan,
        "pixel_accuracy": float(tp.sum() / total) if total > 0 else nan,
        "class_accuracy": acc,
        "mean_class_accuracy": float(acc[labelled].mean()) if labelled.any() else nan,
        "fw_iou": float((row[labelled] / total * iou[labelled]).sum()) if total > 0 else nan,
        "pixels": int(total),
    }


# ---------------------------------------------------------------- the evaluator
class Evaluator:
    """A confusion matrix that lives on the device and grows by `update` / `update_frames` calls, none of
    which synchronises; `confusion()`, `skipped()` and `metrics()` read it back."""

    def __init__(self, num_classes, pred_lut=None, gt_lut=None, device: int | None = None):
        confusion_params((1, 1), (1, 1), num_classes, pred_lut, gt_lut)        # every check, before any device work
        N.require_gpu()
        self.num_classes = int(num_classes)
        self.pred_lut = identity_lut() if pred_lut is None else _lut256("pred_lut", pred_lut).copy()
        self.gt_lut = identity_lut() if gt_lut is None else _lut256("gt_lut", gt_lut).copy()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.acc = torch.zeros(self.num_classes ** 2 + 1, dtype=torch.int64, device=self.device)
        self._params: dict = {}
        self._bufs: dict = {}

    @classmethod
    def for_grids(cls, device: int | None = None) -> "Evaluator":
        """The 3-class evaluator of occupancy grids (unknown, free, occupied; grid_lut on both sides): the
        grids of a predicted map against the grids of a labelled map. int8 grids are taken as they are."""
        return cls(3, pred_lut=grid_lut(), gt_lut=grid_lut(), device=device)

    def _up(self, name: str, x) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            if x.is_cuda and x.device != self.device:
                raise ValueError(f"{name} is on {x.device}, but the evaluator accumulates on {self.device}")
            t = x
        else:
            a = np.ascontiguousarray(x)
            if a.dtype not in (np.uint8, np.int8):
                raise ValueError(f"{name} must be uint8 (or int8), got {a.dtype}")
            t = torch.from_numpy(a)
        return t if t.is_cuda else t.to(self.device)

    def update(self, pred, gt) -> None:
        """Add (B, ph, pw) or (ph, pw) predictions against (B, gh, gw) or (gh, gw) labels: uint8 (or int8)
        device tensors, or NumPy arrays, which are copied up first."""
        p_, g_ = _maps("pred", self._up("pred", pred)), _maps("gt", self._up("gt", gt))
        key = (tuple(p_.shape[1:]), tuple(g_.shape[1:]))
        if key not in self._params:
            self._params[key] = confusion_params(*key, self.num_classes, self.pred_lut, self.gt_lut)
        confusion_device(p_, g_, self.num_classes, out=self.acc, params=self._params[key])

    def _buf(self, key, shape):
        t = self._bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._bufs[key] = torch.empty(shape, dtype=torch.uint8, device=self.device)
        return t

    def predict_classes(self, model, frames_bgr, model_hw=None) -> torch.Tensor:
        """What update_frames evaluates: (B, H0, W0, 3) uint8 BGR frames (device, or host and copied up) ->
        the model's (B, H, W) u8 class map on the device, in a buffer this evaluator owns and reuses. An ENET
        gives its 15 class ids (OUT_CLASS15_U8), a DeepLabV3 class_lut[class id]. (H, W) = model_hw, by
        default an ENET's INPUT_HEIGHT x INPUT_WIDTH and a DeepLabV3's crop; frames of another size are
        resized to it first (models.py:87)."""
        from .models import ENET, DeepLabV3, _as_device_tensor
        dl = isinstance(model, DeepLabV3)
        if not dl and not isinstance(model, ENET):
            raise ValueError("model must be an ENET or a DeepLabV3")
        if dl and model.class_lut is None:
            raise ValueError("a DeepLabV3 model needs its class_lut set (models.class_lut3 / class_lut_binary): "
                             "there is no default mapping of an arbitrary label set to the rasteriser's classes")
        if model.ctx.device != self.device.index:
            raise ValueError(f"the model runs on cuda:{model.ctx.device}, but the evaluator accumulates on {self.device}")
        x = _as_device_tensor(frames_bgr, torch.uint8, self.device.index)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"expected BGR uint8 frames (B, H, W, 3), got {tuple(x.shape)}")
        B, H0, W0 = (int(v) for v in x.shape[:3])
        if model_hw is None:
            model_hw = model._spec.crop_hw(model.net) if dl else (ENET.INPUT_HEIGHT, ENET.INPUT_WIDTH)
        H, W = int(model_hw[0]), int(model_hw[1])
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            if (H0, W0) != (H, W):
                small = self._buf(("frames", id(model)), (B, H, W, 3))
                N.shared_context(self.device.index).preprocess(x, B, H0, W0, H, W, N.PRE_BGR_U8, small, stream)
                x = small
            seg = self._buf(("seg", id(model)), (B, H, W))
            if dl:
                model.predict_classes_device(x, bgr=True, out=seg)
            else:
                model.ctx.forward_bgr(x, B, H, W, N.OUT_CLASS15_U8, seg, stream)
        return seg

    def update_frames(self, model, frames_bgr, labels, model_hw=None) -> None:
        """Run `model` on BGR frames and add its class maps against `labels` ((B, gh, gw) uint8): the forward
        to u8 classes (predict_classes) feeds the kernel directly, so no class map reaches the host and the
        whole call can be captured (after one call outside the capture: a DeepLabV3 builds its plan on the
        first call at a batch size, which allocates and synchronises). A DeepLabV3 without a class_lut is
        refused, as OccupancyPipeline refuses it."""
        self.update(self.predict_classes(model, frames_bgr, model_hw), labels)

    def reset(self) -> None:
        self.acc.zero_()

    def confusion(self) -> np.ndarray:
        """Synchronises: the (C, C) int64 matrix, rows = labels, columns = predictions."""
        C = self.num_classes
        return self.acc[: C * C].cpu().numpy().reshape(C, C).copy()

    def skipped(self) -> int:
        """Synchronises: label pixels seen whose label or prediction mapped to no class."""
        return int(self.acc[-1].item())

    def metrics(self) -> dict:
        return metrics(self.confusion())

    def reduce(self, group=None) -> None:
        """Sum the accumulators of all ranks, in place on every rank (one all-reduce)."""
        from .distributed import reduce_confusion
        reduce_confusion(self.acc, group)
