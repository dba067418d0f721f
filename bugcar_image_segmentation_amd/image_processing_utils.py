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

What hough_lines computes is stated in DESIGN.md §6.21: cv2.HoughLines' standard transform, the step between
canny and find_intersection_line. Here it is three launches over a batch (csrc/hough_kernels.hip), bit-exact
against the restatements in tests/hough_ref.py; the sines and cosines come from one host function of the library.
"""
from __future__ import annotations

import ctypes

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


HOUGH_MAX_LINES = 4096          # the most lines one call stores per frame (the select's LDS sort)
HOUGH_MAX_SIDE, HOUGH_MAX_NUMRHO, HOUGH_MAX_NUMANGLE = 65535, 13651, 65536      # include/bugseg.h


def hough_params(h: int, w: int, rho, theta, threshold, max_lines, min_theta=0.0, max_theta=np.pi) -> N.HoughParams:
    """bugseg_hough_params for (h, w) images, with every check before any device work.
    rho and theta are rounded to float32 first; numangle = floor((max_theta - min_theta) / theta) + 1 in double,
    less one if numangle > 1 and |pi - (numangle - 1) theta| < theta / 2; numrho = cvRound((2 (w + h) + 1) / rho)
    in double. ValueError for: an empty image or a side above 65535; rho or theta that is not positive and finite
    as float32; min_theta or max_theta not finite, max_theta < min_theta; a threshold that is no finite number
    (it is floored and clamped to int32); max_lines outside 1..4096; numrho below 1 or above 13651, numangle above
    65536, (numangle + 2) (numrho + 2) of 2^31 or more."""
    h, w = int(h), int(w)
    if not (1 <= h <= HOUGH_MAX_SIDE and 1 <= w <= HOUGH_MAX_SIDE):
        raise ValueError(f"hough needs an image of 1 x 1 to {HOUGH_MAX_SIDE} x {HOUGH_MAX_SIDE}, got {h} x {w}")
    with np.errstate(over="ignore"):
        r32, t32, m32 = np.float32(float(rho)), np.float32(float(theta)), np.float32(float(min_theta))
    if not (np.isfinite(r32) and r32 > 0 and np.isfinite(t32) and t32 > 0):
        raise ValueError(f"rho and theta must be positive and finite as float32, got {rho!r}, {theta!r}")
    lo, hi = float(min_theta), float(max_theta)
    if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(m32)) or hi < lo:
        raise ValueError(f"min_theta and max_theta must be finite with max_theta >= min_theta, got {min_theta!r}, {max_theta!r}")
    thr = float(threshold)
    if not np.isfinite(thr):
        raise ValueError(f"threshold must be finite, got {threshold!r}")
    if isinstance(max_lines, bool) or int(max_lines) != max_lines or not 1 <= int(max_lines) <= HOUGH_MAX_LINES:
        raise ValueError(f"max_lines must be an integer in [1, {HOUGH_MAX_LINES}], got {max_lines!r}")
    t, r = float(t32), float(r32)
    angles = np.floor((hi - lo) / t) + 1.0
    rhos = np.rint((2.0 * (w + h) + 1.0) / r)
    if angles > HOUGH_MAX_NUMANGLE + 1:
        raise ValueError(f"theta {theta!r} gives more than {HOUGH_MAX_NUMANGLE} angles")
    numangle = int(angles)
    if numangle > 1 and abs(np.pi - (numangle - 1) * t) < t / 2:
        numangle -= 1
    if numangle > HOUGH_MAX_NUMANGLE:
        raise ValueError(f"theta {theta!r} gives more than {HOUGH_MAX_NUMANGLE} angles")
    if not 1 <= rhos <= HOUGH_MAX_NUMRHO:
        raise ValueError(f"rho {rho!r} gives {rhos:.0f} accumulator columns for {h} x {w}; 1 to {HOUGH_MAX_NUMRHO} are supported")
    numrho = int(rhos)
    if (numangle + 2) * (numrho + 2) >= 2 ** 31:
        raise ValueError("the accumulator has 2^31 cells or more")
    p = N.HoughParams()
    p.rows, p.cols, p.numangle, p.numrho = h, w, numangle, numrho
    p.threshold = int(min(max(np.floor(thr), -2.0 ** 31), 2.0 ** 31 - 1))
    p.max_lines = int(max_lines)
    p.rho, p.theta, p.min_theta = float(r32), float(t32), float(m32)
    return p


_hough_trig_tables: dict = {}       # (device, numangle, rho, theta, min_theta) -> the device copy of the trig table


def hough_trig_host(p: N.HoughParams) -> np.ndarray:
    """bugseg_hough_trig: the (2, numangle) float32 table of p, cosines / rho then sines / rho. Host only."""
    tab = np.empty((2, p.numangle), np.float32)
    N.check(N.load_library().bugseg_hough_trig(ctypes.byref(p), tab.ctypes.data))
    return tab


def hough_trig_device(device: torch.device, p: N.HoughParams) -> torch.Tensor:
    """The device copy of p's trig table, made on first use per (device, parameters) and kept for the process's
    life (a captured graph may hold its address; a table is 8 bytes per angle). Making it copies from the host,
    so the first call with new parameters must come before a capture: inside one it raises RuntimeError."""
    key = (device.index, p.numangle, float(p.rho), float(p.theta), float(p.min_theta))
    t = _hough_trig_tables.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("hough: call once with these parameters before capturing (the trig table is uploaded on first use)")
        t = torch.from_numpy(hough_trig_host(p).reshape(-1)).to(device)
        t = _hough_trig_tables.setdefault(key, t)
    return t


def hough_lines_device(images: torch.Tensor, rho, theta, threshold, max_lines: int = 256, min_theta=0.0, max_theta=np.pi):
    """Batched cv2.HoughLines(image, rho, theta, threshold, min_theta=, max_theta=) on device tensors: (B, h, w) or
    (h, w) uint8 images, any non-zero byte is an edge -> (lines, counts, peaks) on the current stream: lines
    (B, max_lines, 2) float32 (rho, theta), strongest first, zero from row counts[b] on; counts (B,) int32 =
    min(peaks, max_lines); peaks (B,) int32, the peaks found. Nothing is read back: the call does not synchronise."""
    im, (B, h, w) = _device_batch(images, "images")
    p = hough_params(h, w, rho, theta, threshold, max_lines, min_theta, max_theta)
    if B < 1:
        raise ValueError("images holds no frame")
    trig = hough_trig_device(im.device, p)
    with torch.cuda.device(im.device):
        lines = torch.empty((B, p.max_lines, 2), dtype=torch.float32, device=im.device)
        counts = torch.empty((B,), dtype=torch.int32, device=im.device)
        peaks = torch.empty((B,), dtype=torch.int32, device=im.device)
        N.shared_context(im.device.index).hough(im, B, p, trig, lines, counts, peaks, torch.cuda.current_stream(im.device))
    return lines, counts, peaks


def hough_lines(img, rho, theta, threshold, min_theta=0.0, max_theta=np.pi):
    """cv2.HoughLines(img, rho, theta, threshold, min_theta=0, max_theta=pi), the standard transform: an (h, w)
    uint8 image (NumPy array or torch tensor) -> an owned NumPy float32 (N, 1, 2) array of (rho, theta), strongest
    first, or None when no line passes. cv2 returns every peak; one call here stores at most 4096, so a frame with
    more raises ValueError naming the count: nothing is cut off silently."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dim() != 2 or t.dtype != torch.uint8:
        raise ValueError("img must be an (h, w) uint8 image")
    hough_params(t.shape[0], t.shape[1], rho, theta, threshold, HOUGH_MAX_LINES, min_theta, max_theta)    # before any device work
    N.require_gpu()
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    lines, counts, peaks = hough_lines_device(t, rho, theta, threshold, HOUGH_MAX_LINES, min_theta, max_theta)
    found, n = int(peaks[0]), int(counts[0])
    if found > HOUGH_MAX_LINES:
        raise ValueError(f"the image has {found} lines above the threshold; at most {HOUGH_MAX_LINES} can be returned: raise the threshold")
    if n == 0:
        return None
    return lines[0, :n].cpu().numpy().reshape(n, 1, 2).copy()


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
