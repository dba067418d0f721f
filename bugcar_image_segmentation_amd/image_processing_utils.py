"""image_processing_utils.py of the reference, on the native engine: `contour_noise_removal`
(image_processing_utils.py:4-44), the clean-up of a binary road map between `ENET.predict_binary` and
`create_occupancy_grid_binary`. The reference's `clahe`, `find_intersection_line` and `create_skeleton`
are not provided.

What it computes is stated in DESIGN.md §6.16: the map is closed with a k x k square, and of the closed
map's regions only the road regions that reach the bottom tenth of the image are kept, their small holes
filled. The reference does this on the host with OpenCV (morphologyEx, findContours, one fillPoly per
contour); here it is a fixed sequence of integer kernels over a batch (csrc/road_kernels.hip), bit-exact
against the restatement in tests/road_filter_ref.py. There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

LENGTH_RATIO = 0.1        # image_processing_utils.py:19
MASK_AREA_THRESH = 0.4    # image_processing_utils.py:31
MIN_SIDE = 50


def road_filter_params(h: int, w: int) -> N.RoadFilterParams:
    """The host arithmetic of image_processing_utils.py:6-8, 19-27, 31, 38 in the reference's own Python
    float expressions: k = int(min(h, w) / 50), y_top = int(h * (1 - 0.1)), mask_area = w * (h - y_top);
    a filled contour is kept when its band count is > mask_area * 0.4, i.e. >= floor(mask_area * 0.4) + 1.

    h >= 50 and w >= 50, otherwise ValueError. Below that k is 0 (an empty structuring element, which
    OpenCV treats in its own way), and the reference's `cnt.shape[0] > 2` filter
    (image_processing_utils.py:13), which the device form does not apply, could matter: it drops the
    components that are a single pixel or a straight one-pixel line. With h >= 50 the band has r >= 5
    rows of w >= 50 columns, so a kept contour needs more than 0.4 r w band pixels, which is at least 2 w
    and at least 20 r, while a single pixel has 1 and a one-pixel line at most max(w, r) of them: no such
    component can be kept, with the filter or without it."""
    h, w = int(h), int(w)
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError(f"contour_noise_removal needs a map of at least {MIN_SIDE} x {MIN_SIDE}, got {h} x {w}")
    min_length = min(h, w)
    k = int(min_length / 50)
    y_top = int(h * (1 - LENGTH_RATIO))
    mask_area = (w - 0) * (h - y_top)
    thresh = mask_area * MASK_AREA_THRESH
    p = N.RoadFilterParams()
    p.rows, p.cols, p.k, p.y_top = h, w, k, y_top
    p.min_count = int(np.floor(thresh)) + 1
    return p


def contour_noise_removal_device(segmaps: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Batched contour_noise_removal on device tensors: (B, h, w) or (h, w) uint8 maps (any non-zero
    value is road) -> (B, h, w) uint8 in {0, 1}, on the current stream. `out` must not overlap the input."""
    if not isinstance(segmaps, torch.Tensor) or not segmaps.is_cuda or segmaps.dtype != torch.uint8:
        raise ValueError("segmaps must be a uint8 device tensor")
    seg = segmaps if segmaps.dim() == 3 else segmaps.unsqueeze(0)
    if seg.dim() != 3:
        raise ValueError("segmaps must have shape (B, h, w) or (h, w)")
    seg = seg.contiguous()
    B, h, w = seg.shape
    p = road_filter_params(h, w)
    if B < 1:
        raise ValueError("segmaps holds no frame")
    if out is None:
        out = torch.empty((B, h, w), dtype=torch.uint8, device=seg.device)
    elif tuple(out.shape) != (B, h, w) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != seg.device:
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {(B, h, w)} on {seg.device}")
    with torch.cuda.device(seg.device):
        N.shared_context(seg.device.index).road_filter(seg, B, p, out, torch.cuda.current_stream(seg.device))
    return out


def contour_noise_removal(segmap):
    """image_processing_utils.py:4-44: an (h, w) map (NumPy array or torch tensor, any integer or bool
    dtype; non-zero = road) -> an owned NumPy uint8 (h, w) map in {0, 1}."""
    if isinstance(segmap, torch.Tensor):
        t = segmap
    else:
        t = torch.from_numpy(np.ascontiguousarray(segmap))
    if t.dim() != 2:
        raise ValueError("segmap must have shape (h, w)")       # image_processing_utils.py:6 unpacks two
    road_filter_params(*t.shape)                                # the size check, before any device work
    N.require_gpu()
    if t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8)
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return contour_noise_removal_device(t)[0].cpu().numpy().copy()      # owned: no torch storage behind it
