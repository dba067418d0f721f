"""image_processing_utils.py of the reference, on the native engine: `contour_noise_removal`
(image_processing_utils.py:4-44), the clean-up of a binary road map between `ENET.predict_binary` and
`create_occupancy_grid_binary`, and `clahe` (image_processing_utils.py:46-61), the contrast fix applied to a
camera frame before `ENET.preprocess`, `find_intersection_line` (image_processing_utils.py:63-91) and
`create_skeleton` (image_processing_utils.py:95-105) with the `cv2.Canny` it needs (`canny`, `canny_device`).

What contour_noise_removal computes is stated in DESIGN.md §6.16: the map is closed with a k x k square, and
of the closed map's regions only the road regions that reach the bottom tenth of the image are kept, their
small holes filled. The reference does this on the host with OpenCV (morphologyEx, findContours, one fillPoly
per contour); here it is a fixed sequence of integer kernels over a batch (csrc/road_kernels.hip), bit-exact
against the restatement in tests/road_filter_ref.py.

What clahe computes is stated in DESIGN.md §6.18: BGR -> Lab in 8 bits, contrast-limited adaptive histogram
equalisation of L over an 8 x 8 grid of tiles with clipLimit 3.0, Lab -> BGR. The reference does this with
cv2.cvtColor and cv2.createCLAHE; here it is two launches over a batch (csrc/clahe_kernels.hip), bit-exact
against the restatement in tests/clahe_ref.py.

What canny computes is stated in DESIGN.md §6.19: 3 x 3 Sobel with the border replicated, |dx| + |dy|,
non-maximum suppression, hysteresis between two thresholds (cv2.Canny with apertureSize 3 and L2gradient
False, the only form the reference uses). Here it is five launches over a batch (csrc/canny_kernels.hip),
bit-exact against the restatements in tests/canny_ref.py. create_skeleton is the outline of the camera's field
of view in the occupancy grid: the edges of the grid of an all-free map. find_intersection_line is host
arithmetic. There is no CPU fallback for the device functions.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

def _device_batch(t, name: str, bgr: bool = False):
    """What every *_device function does first: `t`, a uint8 device tensor of one frame or a batch of them
    (frames are (h, w), or (h, w, 3) when `bgr`), as a contiguous batch -> (batch, (B, h, w))."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
        raise ValueError(f"{name} must be a uint8 device tensor")
    nd = 4 if bgr else 3
    b = t if t.dim() == nd else t.unsqueeze(0)
    if b.dim() != nd or (bgr and b.shape[3] != 3):
        raise ValueError(f"{name} must have shape " + ("(B, h, w, 3) or (h, w, 3)" if bgr else "(B, h, w) or (h, w)"))
    b = b.contiguous()
    return b, tuple(b.shape[:3])


def _out_like(batch: torch.Tensor, name: str, out):
    """After the parameter checks: refuse an empty batch, then check `out` against the batch or allocate it."""
    if batch.shape[0] < 1:
        raise ValueError(f"{name} holds no frame")
    if out is None:
        return torch.empty_like(batch)
    if tuple(out.shape) != tuple(batch.shape) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != batch.device:
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(batch.shape)} on {batch.device}")
    return out


def _host_call(t: torch.Tensor, device_fn, *args):
    """The host wrappers' tail, after their checks: one frame to the current device, through `device_fn`, back
    as an owned NumPy array (no torch storage behind it)."""
    N.require_gpu()
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return device_fn(t, *args)[0].cpu().numpy().copy()


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
    seg, (B, h, w) = _device_batch(segmaps, "segmaps")
    p = road_filter_params(h, w)
    out = _out_like(seg, "segmaps", out)
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
    if t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8)
    return _host_call(t, contour_noise_removal_device)


CLAHE_CLIP_LIMIT = 3.0          # image_processing_utils.py:53
CLAHE_TILE_GRID = (8, 8)        # image_processing_utils.py:53, (tiles_x, tiles_y)
CLAHE_MAX_TILES = 16


def clahe_params(h: int, w: int, clip_limit: float = CLAHE_CLIP_LIMIT, tile_grid=CLAHE_TILE_GRID) -> N.ClaheParams:
    """bugseg_clahe_params for (h, w) frames, with the checks the library makes, before any device work:
    ValueError for a grid outside [1, 16] per side, a side smaller than twice its tile count (the reflected
    border of a frame that the grid does not divide needs that room), a clip limit that is not positive and
    finite."""
    h, w = int(h), int(w)
    try:
        tx, ty = (int(v) for v in tile_grid)
    except (TypeError, ValueError):
        raise ValueError(f"tile_grid must be (tiles_x, tiles_y), got {tile_grid!r}") from None
    if not (1 <= tx <= CLAHE_MAX_TILES and 1 <= ty <= CLAHE_MAX_TILES):
        raise ValueError(f"clahe tiles must be in [1, {CLAHE_MAX_TILES}] per side, got {tx} x {ty}")
    if h < 2 * ty or w < 2 * tx:
        raise ValueError(f"clahe needs a frame of at least {2 * ty} x {2 * tx} for a {tx} x {ty} grid, got {h} x {w}")
    c = float(clip_limit)
    if not (0.0 < c <= float(np.finfo(np.float32).max) and np.float32(c) > 0):      # (the struct holds a float32)
        raise ValueError(f"clip_limit must be positive and finite, got {clip_limit!r}")
    p = N.ClaheParams()
    p.rows, p.cols, p.tiles_x, p.tiles_y, p.clip_limit = h, w, tx, ty, c
    return p


def clahe_device(frames: torch.Tensor, out: torch.Tensor | None = None, clip_limit: float = CLAHE_CLIP_LIMIT,
                 tile_grid=CLAHE_TILE_GRID) -> torch.Tensor:
    """Batched clahe on device tensors: (B, h, w, 3) or (h, w, 3) uint8 BGR frames -> (B, h, w, 3) uint8 BGR,
    on the current stream. `out` must not overlap the input."""
    f, (B, h, w) = _device_batch(frames, "frames", bgr=True)
    p = clahe_params(h, w, clip_limit, tile_grid)
    out = _out_like(f, "frames", out)
    with torch.cuda.device(f.device):
        N.shared_context(f.device.index).clahe(f, B, p, out, torch.cuda.current_stream(f.device))
    return out


def clahe(img):
    """image_processing_utils.py:46-61: an (h, w, 3) uint8 BGR frame (NumPy array or torch tensor) -> an owned
    NumPy uint8 (h, w, 3) BGR frame."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
        raise ValueError("img must be an (h, w, 3) uint8 BGR frame")     # cv2.COLOR_BGR2LAB of 8-bit input
    clahe_params(t.shape[0], t.shape[1])                        # the size check, before any device work
    return _host_call(t, clahe_device)


CANNY_LOW, CANNY_HIGH = 50, 150         # image_processing_utils.py:104


def canny_params(h: int, w: int, threshold1, threshold2, apertureSize: int = 3, L2gradient: bool = False) -> N.CannyParams:
    """bugseg_canny_params for (h, w) images, with every check before any device work: ValueError for an
    aperture other than 3, the L2 gradient, an empty image, a threshold that is NaN or infinite. The struct
    holds low = floor(threshold1) and high = floor(threshold2), swapped if low > high (DESIGN.md §6.19,
    step 1), clamped to the int32 range (no magnitude exceeds 2040, so the clamp changes no result)."""
    h, w = int(h), int(w)
    if apertureSize != 3:
        raise ValueError(f"canny supports apertureSize 3 only, got {apertureSize!r}")
    if L2gradient:
        raise ValueError("canny supports L2gradient=False only")
    if h < 1 or w < 1:
        raise ValueError(f"canny needs an image of at least 1 x 1, got {h} x {w}")
    t = []
    for v in (threshold1, threshold2):
        f = float(v)
        if not np.isfinite(f):
            raise ValueError(f"canny thresholds must be finite, got {v!r}")
        t.append(int(min(max(np.floor(f), -2.0 ** 31), 2.0 ** 31 - 1)))
    low, high = t
    if low > high:
        low, high = high, low
    p = N.CannyParams()
    p.rows, p.cols, p.low, p.high = h, w, low, high
    return p


def canny_device(images: torch.Tensor, threshold1, threshold2, out: torch.Tensor | None = None) -> torch.Tensor:
    """Batched cv2.Canny(image, threshold1, threshold2) on device tensors: (B, h, w) or (h, w) uint8 images
    -> (B, h, w) uint8 in {0, 255}, on the current stream. `out` must not overlap the input."""
    im, (B, h, w) = _device_batch(images, "images")
    p = canny_params(h, w, threshold1, threshold2)
    out = _out_like(im, "images", out)
    with torch.cuda.device(im.device):
        N.shared_context(im.device.index).canny(im, B, p, out, torch.cuda.current_stream(im.device))
    return out


def canny(img, threshold1, threshold2, apertureSize: int = 3, L2gradient: bool = False):
    """cv2.Canny(img, threshold1, threshold2, apertureSize=3, L2gradient=False): an (h, w) uint8 image (NumPy
    array or torch tensor) -> an owned NumPy uint8 (h, w) edge map in {0, 255}."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dim() != 2 or t.dtype != torch.uint8:
        raise ValueError("img must be an (h, w) uint8 image")            # cv2.Canny's 8-bit single-channel input
    canny_params(t.shape[0], t.shape[1], threshold1, threshold2, apertureSize, L2gradient)   # before any device work
    return _host_call(t, canny_device, threshold1, threshold2)


def find_intersection_line(line1, line2):
    """image_processing_utils.py:63-91, host arithmetic: each line is two points ((x1, y1), (x2, y2)); the
    result is the NumPy pair (x, y) where they meet, or None. A line is a x + b y = c with b = -1,
    a = (y2 - y1) / (x2 - x1), c = (x1 y2 - x2 y1) / (x2 - x1); a vertical line is a = 1, b = 0, c = x1.

    As in the reference, None is returned whenever the two a are equal: for parallel lines and two vertical
    lines, and also for a vertical line against a line of slope 1 (both have a = 1), although those two meet."""
    first, second = _line_abc(line1), _line_abc(line2)
    if first[0] == second[0]:
        return None
    return np.linalg.solve(np.array([first[:2], second[:2]]), np.array([first[2], second[2]]))


def _line_abc(line):
    """(a, b, c) of a x + b y = c through the two points of `line`, in find_intersection_line's convention."""
    (px, py), (qx, qy) = line[0], line[1]
    run = qx - px
    if run == 0:
        return 1, 0, px                                  # vertical: x = px
    return (qy - py) / run, -1, (px * qy - qx * py) / run


def create_skeleton(perspective_transformer, input_shape, occupancy_grid_width_in_m, occupancy_grid_height_in_m,
                    cell_size_in_m):
    """image_processing_utils.py:95-105 with a call shape that works: the reference passes
    create_occupancy_grid seven arguments, five of them attributes the transformer does not have; here they
    are create_occupancy_grid's three real ones. input_shape = (width, height) of the segmentation map. The
    occupancy grid of an all-free (height, width) map is built on the device, its int8 cells are read as uint8
    (unknown, -1, becomes 255) and canny_device(., 50, 150) outlines the camera's field of view in it; only the
    result leaves the device -> NumPy uint8 (h, w) in {0, 255}. A map shape that the transformer was not
    calibrated for fails its own assertion."""
    width, height = input_shape
    N.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    free_img = torch.ones((int(height), int(width)), dtype=torch.uint8, device=dev)      # image_processing_utils.py:97
    occ_grid = perspective_transformer.create_occupancy_grid_device(free_img, occupancy_grid_width_in_m,
                                                                    occupancy_grid_height_in_m, cell_size_in_m)
    edges = canny_device(occ_grid.contiguous().view(torch.uint8), CANNY_LOW, CANNY_HIGH)
    return edges[0].cpu().numpy().copy()      # owned: no torch storage behind it
