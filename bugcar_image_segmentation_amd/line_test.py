"""The check the reference's README names but does not ship (test_straight_line.py: "see for yourself if the
bev_matrix is functioning as intended"), as a number instead of a look: a camera frame with straight parallel
markings (lane lines, the calibration tiles' edges) is warped into the bird's-eye view, its edges are found and
the straight lines through them; seen through a correct matrix the lines are parallel, so their angles agree.

  straight_lines_device   warp_image_device(gray) -> canny_device -> hough_lines_device, all on the device, no
                          synchronisation: the whole chain can be captured as one graph (after one call outside
                          the capture, which uploads the Hough trig table)
  straight_line_report    host arithmetic on the lines: per frame the strongest line's angle and the largest
                          angular distance of any line from it (`spread`, radians, 0 for parallel lines)
  check_straight_lines    the one-call host form

The Hough threshold defaults to THRESHOLD_FRACTION of the warped image's shorter side: a line must be supported
by edge pixels along more than a quarter of it, which a lane marking that crosses the view is and the short
edges of texture and noise are not.
"""
from __future__ import annotations

import numpy as np
import torch

from . import image_processing_utils as ipu

THRESHOLD_FRACTION = 0.25


def default_threshold(bev) -> int:
    """int(THRESHOLD_FRACTION * min(after_warp_height, after_warp_width))."""
    return int(THRESHOLD_FRACTION * min(int(bev.after_warp_height), int(bev.after_warp_width)))


def straight_lines_device(bev, frames: torch.Tensor, canny=(50, 150), rho=1.0, theta=np.pi / 180, threshold=None,
                          max_lines: int = 64):
    """frames: uint8 device tensor, (B, r, c, 3) or (r, c, 3) BGR (or (B, r, c), (r, c): already grey), (r, c) the
    size `bev` was calibrated for -> hough_lines_device's (lines, counts, peaks) of the warped frames' Canny
    edges, on the current stream."""
    f, ch = bev._frame_batch(frames)
    gray = bev.warp_image_device(f, gray=ch == 3)
    edges = ipu.canny_device(gray, canny[0], canny[1])
    thr = default_threshold(bev) if threshold is None else threshold
    return ipu.hough_lines_device(edges, rho, theta, thr, max_lines)


def straight_line_report(lines, counts) -> list[dict]:
    """Per frame of (lines (B, max_lines, 2), counts (B,)) (tensors or arrays): {"count": the lines stored,
    "theta0": the strongest line's angle (None without a line), "deviation": per line d = min(|theta - theta0|,
    pi - |theta - theta0|) as float64, "spread": max d (None without a line)}. An angle and the same angle plus
    pi are one direction, hence the second term."""
    ln = np.asarray(lines.cpu() if isinstance(lines, torch.Tensor) else lines, dtype=np.float64)
    cn = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    if ln.ndim != 3 or ln.shape[2] != 2 or cn.shape != (ln.shape[0],):
        raise ValueError("lines must be (B, max_lines, 2) and counts (B,)")
    out = []
    for b in range(ln.shape[0]):
        n = int(cn[b])
        if not 0 <= n <= ln.shape[1]:
            raise ValueError(f"counts[{b}] = {n} is outside 0..{ln.shape[1]}")
        if n == 0:
            out.append({"count": 0, "theta0": None, "deviation": np.zeros(0), "spread": None})
            continue
        th = ln[b, :n, 1]
        a = np.abs(th - th[0])
        d = np.minimum(a, np.pi - a)
        out.append({"count": n, "theta0": float(th[0]), "deviation": d, "spread": float(d.max())})
    return out


def check_straight_lines(bev, frame, canny=(50, 150), rho=1.0, theta=np.pi / 180, threshold=None, max_lines: int = 64) -> dict:
    """One (r, c, 3) BGR or (r, c) grey uint8 frame (NumPy array or torch tensor) -> its straight_line_report
    entry, with "lines" (the (count, 2) float32 (rho, theta) array) and "peaks" (the lines found before max_lines
    cut them) added."""
    from . import _native as N
    t = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
    if t.dtype != torch.uint8 or not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)):
        raise ValueError("frame must be an (r, c, 3) or (r, c) uint8 image")
    bev._check_shape(t.shape[:2])
    N.require_gpu()
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    lines, counts, peaks = straight_lines_device(bev, t, canny, rho, theta, threshold, max_lines)
    rep = straight_line_report(lines, counts)[0]
    rep["lines"] = lines[0, :rep["count"]].cpu().numpy().copy()
    rep["peaks"] = int(peaks[0])
    return rep
