"""The calibration the reference's README starts with (`python3 calibration.py`: "Press C to calibrate, and S to save
the matrix into a json file") without the key presses: camera frames that show the calibration tile in, the tile's
image corners (`tile_coords`) and the solved bird's-eye matrix out; the caller saves with `bev.save_to_JSON`.

  quad_params          bugseg_quad_params for a frame size, with every check before any device work
  find_tile_device     find_quad on the device (csrc/quad_kernels.hip): per frame status, threshold,
                       area, root, the four coarse corners and the moments of the region's boundary along each
                       side; no synchronisation, capturable
  refine               host, float64: a total-least-squares line per side from the moments, corners where adjacent
                       lines meet
  find_tile            two passes: find_tile_device and refine, then the moments again in a narrower band around
                       the refined sides (bugseg_quad_moments) and refine again
  order_tile_corners   the order bev.calculate_transform_matrix pairs with its target points
  solve, calibrate     the per-corner median over the frames -> tile_coords -> the matrix, as a report

What the device computes is integer-exact and bit for bit the restatement in tests/quad_ref.py. There is no CPU
fallback for it.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N

OK, NO_TILE, DEGENERATE = 0, 1, 2          # include/bugseg.h BUGSEG_QUAD_*
MAX_SIDE, MIN_SIDE, MAX_BAND = 4096, 3, 64
DEFAULT_BAND = (3, 2)


def quad_params(h: int, w: int, bright: bool = True, threshold=None, min_area=None, band=DEFAULT_BAND, channels: int = 3) -> N.QuadParams:
    """bugseg_quad_params for (h, w) frames. bright: the tile is brighter than its surroundings. threshold: None for
    Otsu's threshold per frame, or a fixed one in 0..254. min_area defaults to max(16, h * w // 1000): a tile smaller
    than a thousandth of the frame (or 16 pixels) has sides too short to fit. band = (first pass, second pass): the
    half-width in pixels of the strip along a side whose boundary points the side takes. ValueError for a side
    outside 3..4096, a threshold outside 0..254, min_area below 1, a band outside 0..64, channels not 1 or 3."""
    h, w = int(h), int(w)
    if not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
        raise ValueError(f"find_tile needs frames of {MIN_SIDE} x {MIN_SIDE} to {MAX_SIDE} x {MAX_SIDE}, got {h} x {w}")
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, got {channels!r}")
    if threshold is not None and (isinstance(threshold, bool) or int(threshold) != threshold or not 0 <= int(threshold) <= 254):
        raise ValueError(f"threshold must be None or an integer in [0, 254], got {threshold!r}")
    area = max(16, h * w // 1000) if min_area is None else min_area
    if isinstance(area, bool) or int(area) != area or not 1 <= int(area) < 2 ** 31:
        raise ValueError(f"min_area must be a positive integer, got {min_area!r}")
    try:
        b0, b1 = (int(v) for v in band)
    except (TypeError, ValueError):
        raise ValueError(f"band must be (first pass, second pass), got {band!r}") from None
    if not (0 <= b0 <= MAX_BAND and 0 <= b1 <= MAX_BAND):
        raise ValueError(f"band must be in [0, {MAX_BAND}], got {band!r}")
    p = N.QuadParams()
    p.rows, p.cols, p.channels, p.bright = h, w, int(channels), int(bool(bright))
    p.threshold = -1 if threshold is None else int(threshold)
    p.min_area = int(area)
    p.band[0], p.band[1] = b0, b1
    return p


def _device_frames(frames):
    """uint8 device frames as a contiguous batch -> (batch, channels). (B, r, c, 3) and (r, c, 3) are BGR, (B, r, c)
    and (r, c) grey; a three-dimensional tensor whose last dimension is 3 is one BGR frame."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
        raise ValueError("frames must be a uint8 device tensor")
    if frames.dim() == 4 and frames.shape[3] == 3:
        f, ch = frames, 3
    elif frames.dim() == 3 and frames.shape[2] == 3:
        f, ch = frames.unsqueeze(0), 3
    elif frames.dim() == 3:
        f, ch = frames, 1
    elif frames.dim() == 2:
        f, ch = frames.unsqueeze(0), 1
    else:
        raise ValueError(f"frames must have shape (B, r, c, 3), (r, c, 3), (B, r, c) or (r, c), got {tuple(frames.shape)}")
    return f.contiguous(), ch


def find_tile_device(frames: torch.Tensor, bright: bool = True, threshold=None, min_area=None, band=DEFAULT_BAND) -> dict:
    """find_quad on uint8 device frames ((B, r, c, 3) or (r, c, 3) BGR, (B, r, c) or (r, c) grey) on the current
    stream -> {"status", "threshold", "area", "root": (B,) int32, "corners": (B, 4, 2) int32 (x, y) in cyclic order,
    "moments": (B, 4, 6) int64} device tensors. Nothing is read back: the call does not synchronise."""
    f, ch = _device_frames(frames)
    B, h, w = f.shape[:3]
    p = quad_params(h, w, bright, threshold, min_area, band, ch)
    if B < 1:
        raise ValueError("frames holds no frame")
    with torch.cuda.device(f.device):
        i32 = dict(dtype=torch.int32, device=f.device)
        out = {k: torch.empty((B,), **i32) for k in ("status", "threshold", "area", "root")}
        out["corners"] = torch.empty((B, 4, 2), **i32)
        out["moments"] = torch.empty((B, 4, 6), dtype=torch.int64, device=f.device)
        N.shared_context(f.device.index).find_quad(f, B, p, out["status"], out["threshold"], out["area"], out["root"],
                                                   out["corners"], out["moments"], torch.cuda.current_stream(f.device))
    return out


def quad_moments_device(frames: torch.Tensor, corners2: torch.Tensor, band_px: int, bright: bool = True, threshold=None,
                        min_area=None) -> torch.Tensor:
    """bugseg_quad_moments: the side moments of the frames' tile regions for the doubled integer corners `corners2`
    ((B, 4, 2) int32 device tensor), in a band of `band_px` pixels -> (B, 4, 6) int64, on the current stream."""
    f, ch = _device_frames(frames)
    B, h, w = f.shape[:3]
    p = quad_params(h, w, bright, threshold, min_area, (band_px, band_px), ch)
    if not isinstance(corners2, torch.Tensor) or corners2.device != f.device or corners2.dtype != torch.int32 or \
            tuple(corners2.shape) != (B, 4, 2):
        raise ValueError(f"corners2 must be an int32 tensor of shape {(B, 4, 2)} on {f.device}")
    if B < 1:
        raise ValueError("frames holds no frame")
    with torch.cuda.device(f.device):
        mom = torch.empty((B, 4, 6), dtype=torch.int64, device=f.device)
        N.shared_context(f.device.index).quad_moments(f, B, p, int(band_px), corners2.contiguous(), mom,
                                                      torch.cuda.current_stream(f.device))
    return mom


def _fit_line(m):
    """The total-least-squares line through the points whose sums are m = (n, SX, SY, SXX, SXY, SYY): (mean, unit
    direction of the scatter's principal axis). The scatter n SXX - SX^2, ... is formed in exact integers."""
    n, sx, sy, sxx, sxy, syy = (int(v) for v in m)
    a, b, c = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
    th = 0.5 * math.atan2(2.0 * b, float(a - c))
    return (sx / n, sy / n), (math.cos(th), math.sin(th))


def refine(corners2, moments, min_points: int = 8):
    """Pure NumPy, float64. corners2 (B, 4, 2) doubled integer corners, moments (B, 4, 6) the sums of the points of
    side i (from corner i to corner i + 1) -> (status (B,) int32, corners (B, 4, 2) float64 in pixels). Per side the
    total-least-squares line (the mean, and the principal axis of the 2 x 2 scatter); corner i is where the lines of
    sides i - 1 and i meet, halved into pixel units. A side with fewer than min_points points (at least 2), or two
    adjacent lines with |sin| of their angle below 1e-6, gives DEGENERATE and the frame's corners2 / 2."""
    c2 = np.asarray(corners2).reshape(-1, 4, 2)
    mom = np.asarray(moments).reshape(-1, 4, 6)
    if len(c2) != len(mom):
        raise ValueError("corners2 and moments hold different numbers of frames")
    need = max(2, int(min_points))
    status = np.zeros(len(c2), np.int32)
    out = c2.astype(np.float64) / 2
    for f in range(len(c2)):
        if any(int(mom[f, i, 0]) < need for i in range(4)):
            status[f] = DEGENERATE
            continue
        lines = [_fit_line(mom[f, i]) for i in range(4)]
        pts = []
        for i in range(4):
            (p, u), (q, v) = lines[i - 1], lines[i]
            den = u[0] * v[1] - u[1] * v[0]
            if abs(den) < 1e-6:
                break
            s = ((q[0] - p[0]) * v[1] - (q[1] - p[1]) * v[0]) / den
            pts.append(((p[0] + s * u[0]) / 2, (p[1] + s * u[1]) / 2))
        if len(pts) < 4:
            status[f] = DEGENERATE
        else:
            out[f] = pts
    return status, out


def _to_device(frames):
    t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
    if t.dtype != torch.uint8 or t.dim() not in (2, 3, 4) or (t.dim() == 4 and t.shape[3] != 3):
        raise ValueError("frames must be uint8 of shape (B, r, c, 3), (r, c, 3), (B, r, c) or (r, c)")
    N.require_gpu()
    return t if t.is_cuda else t.to(torch.device("cuda", torch.cuda.current_device()))


def find_tile(frames, bright: bool = True, threshold=None, min_area=None, band=DEFAULT_BAND, min_points: int = 8) -> dict:
    """The host form, two passes (and two synchronisations: calibration is a one-shot). frames: NumPy array or torch
    tensor, the shapes of find_tile_device -> NumPy arrays {"status" (B,) int32 (OK, NO_TILE, DEGENERATE), "corners"
    (B, 4, 2) float64 (x, y) in cyclic order (the coarse corners where the status is not OK), "coarse" (B, 4, 2)
    int32, "area", "threshold" (B,) int32, "counts" (B, 4) int64: the second pass's points per side}."""
    t = _to_device(frames)
    dev = find_tile_device(t, bright, threshold, min_area, band)
    status = dev["status"].cpu().numpy()
    coarse = dev["corners"].cpu().numpy()
    st1, c1 = refine(2 * coarse, dev["moments"].cpu().numpy(), min_points)
    good = (status == OK) & (st1 == OK)
    corners2 = np.where(good[:, None, None], np.rint(2 * c1), 0).astype(np.int32)
    mom2 = quad_moments_device(t, torch.from_numpy(corners2).to(t.device), int(band[1]), bright, threshold, min_area).cpu().numpy()
    st2, c2 = refine(corners2, mom2, min_points)
    final = np.where(status != OK, status, np.where(st1 != OK, st1, st2)).astype(np.int32)
    # (refine returns its input, halved, where it fails: the coarse corners in pass one, the rounded ones in pass two)
    corners = np.where(good[:, None, None], c2, np.where((status == OK)[:, None, None], c1, coarse.astype(np.float64)))
    return {"status": final, "corners": corners, "coarse": coarse, "area": dev["area"].cpu().numpy(),
            "threshold": dev["threshold"].cpu().numpy(), "counts": np.where(good[:, None], mom2[:, :, 0], 0)}


def order_tile_corners(corners) -> np.ndarray:
    """Four image corners (4, 2), any order -> the order bev.calculate_transform_matrix pairs with its target points:
    the two corners with the larger image y first (near the vehicle), left before right, then the other two, left
    before right.

    Derivation. calculate_transform_matrix puts its target square through bev.order_points_counter_clockwise with an
    axis that starts at the square's centre and points along the vehicle's x rotated by yaw. That function turns the
    points by -yaw about the centre, calls a point `right` when its turned y is negative and `left` otherwise, and
    returns the left points by ascending turned x, then the right ones likewise. In the bird's-eye image y grows
    downwards, towards the vehicle, so at yaw 0 `left` is the near side of the square (y at or below the centre) and
    `right` the far side, and ascending x is left to right: near-left, near-right, far-left, far-right. Turning by
    yaw keeps every corner of the square in its quadrant about the centre as long as |yaw| < pi / 4, so the four
    names, and the order, hold for those yaws; and a camera that looks forward maps the near side to larger image y
    and left to smaller image x."""
    c = np.asarray(corners, np.float64).reshape(4, 2)
    by_y = sorted(range(4), key=lambda i: (-c[i, 1], c[i, 0]))
    near, far = sorted(by_y[:2], key=lambda i: c[i, 0]), sorted(by_y[2:], key=lambda i: c[i, 0])
    return c[near + far]


def solve(bev, corners, status, order=None) -> dict:
    """Pure host. corners (B, 4, 2) and status (B,) as find_tile returns them -> the report {"tile_coords" (4, 2): the
    per-corner median over the frames with status OK, each put through order_tile_corners first so that the frames'
    corners correspond; "frames_used": their indices; "spread_px": the largest distance of any used frame's corner
    from the median; "matrix": bev.calculate_transform_matrix(tile_coords), which also stores it in `bev`}.
    ValueError without a frame of status OK, and for |bev.yaw| >= pi / 4 unless `order` is given: a permutation of
    (0, 1, 2, 3), tile_coords[i] = the ordered corner order[i]."""
    c = np.asarray(corners, np.float64).reshape(-1, 4, 2)
    st = np.asarray(status).reshape(-1)
    if len(st) != len(c):
        raise ValueError("corners and status hold different numbers of frames")
    if order is None:
        if not abs(float(bev.yaw)) < math.pi / 4:
            raise ValueError("order_tile_corners holds for |yaw| < pi / 4 only: pass order=, a permutation of (0, 1, 2, 3)")
        order = (0, 1, 2, 3)
    elif sorted(int(v) for v in order) != [0, 1, 2, 3]:
        raise ValueError(f"order must be a permutation of (0, 1, 2, 3), got {order!r}")
    used = [int(i) for i in np.flatnonzero(st == OK)]
    if not used:
        raise ValueError("no frame shows a tile (no status is OK)")
    each = np.stack([order_tile_corners(c[i]) for i in used])
    tile = order_tile_corners(np.median(each, axis=0))[[int(v) for v in order]]
    each = each[:, [int(v) for v in order]]
    spread = float(np.linalg.norm(each - tile[None], axis=2).max())
    M = bev.calculate_transform_matrix(tile)
    return {"tile_coords": tile, "frames_used": used, "spread_px": spread, "matrix": M}


def calibrate(bev, frames, line_check: bool = False, order=None, **find_args) -> dict:
    """find_tile on the frames (of the size `bev` was made for), then solve: the report of solve, with find_tile's
    "status" added; `bev` holds the new matrix afterwards and the caller saves it with bev.save_to_JSON. With
    line_check the first used frame then goes through line_test.check_straight_lines with the new matrix: its report
    is added as "line_check" and its spread as "line_spread"."""
    t = _to_device(frames)
    f, _ = _device_frames(t)
    bev._check_shape(f.shape[1:3])
    found = find_tile(t, **find_args)
    rep = solve(bev, found["corners"], found["status"], order)
    rep["status"] = found["status"]
    if line_check:
        from . import line_test
        rep["line_check"] = line_test.check_straight_lines(bev, f[rep["frames_used"][0]])
        rep["line_spread"] = rep["line_check"]["spread"]
    return rep
