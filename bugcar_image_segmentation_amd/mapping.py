"""A rolling local map on the device: what a user of the occupancy-grid publisher does next with B
consecutive grids. Each grid comes with the odometry pose (x, y, yaw) of its base point in a fixed world frame; one
launch (csrc/map_kernels.hip, bugseg_map_fuse) fuses the batch in time order into a world-aligned log-odds map that
scrolls with the vehicle, and emits that map as the nav_msgs/OccupancyGrid payload.

  compose              the pose of a camera's grid from the vehicle's pose and the camera's mount
  place_window         where the window lies for a batch of poses (the last finite one, floor semantics)
  pose_record          poses -> the integer update record the device reads: float64 on the host, nothing but
                       integers after it
  build_lut            the int8 table from log-odds to the payload, "ternary" or "probability"
  map_params           bugseg_map_params, with every check before any device work
  occupancy_msg        the OccupancyGrid message of a payload
  LocalMap             the device-resident map: update, set_poses / fuse / capture, reset, state, to_msg

What the device computes is integer-exact and bit for bit the restatement in tests/map_ref.py. There is no CPU
fallback for it.
"""
from __future__ import annotations

import gc
import math

import numpy as np
import torch

from . import _native as N

MAX_SIDE, MAX_B = 4096, 4096
UNOBSERVED = -32768                        # include/bugseg.h BUGSEG_MAP_UNOBSERVED
RECORD_HEADER, RECORD_FRAME = 8, 4         # include/bugseg.h BUGSEG_MAP_RECORD_*
MAX_CELLS = 2 ** 30                        # |x|, |y| / cell_m of a pose: every device sum stays far inside int64
FRAC = 16                                  # fraction bits of the record
MODES = ("ternary", "probability")
RING = 4                                   # pinned copies of the record that may be on their way to the device


def compose(vehicle_pose, mount_pose) -> np.ndarray:
    """The world pose of a grid's base point from the vehicle's world pose and the base point's pose in the vehicle's
    frame (the camera's mount): (x, y, yaw) arrays of any equal or broadcastable leading shape -> float64 (..., 3)."""
    v = np.asarray(vehicle_pose, np.float64)
    m = np.asarray(mount_pose, np.float64)
    if v.shape[-1:] != (3,) or m.shape[-1:] != (3,):
        raise ValueError("poses are (..., 3) arrays of (x, y, yaw)")
    c, s = np.cos(v[..., 2]), np.sin(v[..., 2])
    return np.stack([v[..., 0] + c * m[..., 0] - s * m[..., 1], v[..., 1] + s * m[..., 0] + c * m[..., 1],
                     v[..., 2] + m[..., 2]], axis=-1)


def _poses(poses) -> np.ndarray:
    p = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
    try:
        p = np.ascontiguousarray(p, np.float64)
    except (TypeError, ValueError):
        raise ValueError("poses must be a (B, 3) array of (x, y, yaw)") from None
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"poses must be a (B, 3) array of (x, y, yaw), got shape {p.shape}")
    if not 1 <= p.shape[0] <= MAX_B:
        raise ValueError(f"a batch holds 1..{MAX_B} grids, got {p.shape[0]}")
    return p


def _size(size_cells, what="size_cells"):
    try:
        a, b = size_cells
        if isinstance(a, bool) or isinstance(b, bool) or int(a) != a or int(b) != b:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be two integers, got {size_cells!r}") from None
    a, b = int(a), int(b)
    if not (1 <= a <= MAX_SIDE and 1 <= b <= MAX_SIDE):
        raise ValueError(f"{what}: every side must be in 1..{MAX_SIDE}, got {a} x {b}")
    return a, b


def _cell(cell_m) -> float:
    try:
        c = float(cell_m)
    except (TypeError, ValueError):
        raise ValueError(f"cell_m must be a positive length in metres, got {cell_m!r}") from None
    if not (math.isfinite(c) and c > 0):
        raise ValueError(f"cell_m must be a positive length in metres, got {cell_m!r}")
    return c


def place_window(poses, size_cells, cell_m, origin=None):
    """The window's origin (wx0, wy0) in world cells for a batch: wx0 = floor(x / cell_m) - Wm // 2 and wy0 =
    floor(y / cell_m) - Hm // 2 for the last finite pose of the batch; without one, `origin` (the window stays where
    it is), and before the first placement (origin None) the window of the pose (0, 0)."""
    Hm, Wm = _size(size_cells)
    cell = _cell(cell_m)
    p = _poses(poses)
    ok = np.flatnonzero(np.isfinite(p).all(axis=1))
    if len(ok) == 0:
        return (-(Wm // 2), -(Hm // 2)) if origin is None else (int(origin[0]), int(origin[1]))
    x, y = p[ok[-1], 0] / cell, p[ok[-1], 1] / cell
    if not (abs(x) <= MAX_CELLS and abs(y) <= MAX_CELLS):
        raise ValueError(f"a pose lies more than 2^30 cells from the world's origin: ({p[ok[-1], 0]}, {p[ok[-1], 1]}) m")
    return int(math.floor(x)) - Wm // 2, int(math.floor(y)) - Hm // 2


def pose_record(poses, size_cells, cell_m, origin=None, fresh=True):
    """The update record of a batch (include/bugseg.h): int64 words, a header of 8 and 4 per frame -> (record, new
    origin). origin is where the window lies now ((wx0, wy0), None before the first placement) and fresh whether
    nothing stored is to be kept; the new origin comes from place_window. Per frame, in float64, with c, s = cos,
    sin(yaw), X0 = wx0 + 1/2 - x / cell_m and Y0 = wy0 + 1/2 - y / cell_m:

        C = rint(c 2^16)   S = rint(s 2^16)   Ox = rint((c X0 + s Y0) 2^16)   Oy = rint((-s X0 + c Y0) 2^16)

    so that the centre of window cell (i, j) lies (C j + S i + Ox) / 2^16 cells in front of the grid's base point
    and (-S j + C i + Oy) / 2^16 cells to its left. A frame whose pose is not finite gets C = S = 0, which no yaw
    gives: the device skips it. Against float geometry a coordinate is off by less than (Wm + Hm) 2^-17 cells: C and
    S by at most 2^-17 each, times at most Wm - 1 and Hm - 1, and the offset by at most 2^-17."""
    Hm, Wm = _size(size_cells)
    cell = _cell(cell_m)
    p = _poses(poses)
    wx0, wy0 = place_window(p, (Hm, Wm), cell, origin)
    prev = (wx0, wy0) if origin is None else (int(origin[0]), int(origin[1]))
    rec = np.zeros(RECORD_HEADER + RECORD_FRAME * len(p), np.int64)
    rec[:5] = (wx0, wy0, prev[0], prev[1], int(bool(fresh) or origin is None))
    ok = np.isfinite(p).all(axis=1)
    q = np.where(ok[:, None], p, 0.0)
    if (np.abs(q[:, :2]) / cell > MAX_CELLS).any():
        raise ValueError("a pose lies more than 2^30 cells from the world's origin")
    c, s = np.cos(q[:, 2]), np.sin(q[:, 2])
    X0, Y0 = wx0 + 0.5 - q[:, 0] / cell, wy0 + 0.5 - q[:, 1] / cell
    one = float(1 << FRAC)
    fr = np.stack([np.rint(c * one), np.rint(s * one), np.rint((c * X0 + s * Y0) * one),
                   np.rint((-s * X0 + c * Y0) * one)], axis=1).astype(np.int64)
    fr[~ok] = 0
    rec[RECORD_HEADER:] = fr.reshape(-1)
    return rec, (wx0, wy0)


def _levels(l_occ, l_free, l_min, l_max):
    for name, v in (("l_occ", l_occ), ("l_free", l_free), ("l_min", l_min), ("l_max", l_max)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    l_occ, l_free, l_min, l_max = int(l_occ), int(l_free), int(l_min), int(l_max)
    if not (UNOBSERVED < l_min < 0 < l_max <= 32767):
        raise ValueError(f"needs -32768 < l_min < 0 < l_max <= 32767, got l_min {l_min}, l_max {l_max}")
    if l_occ < 1 or l_free < 1 or l_occ >= 2 ** 31 or l_free >= 2 ** 31:
        raise ValueError(f"l_occ and l_free must be at least 1 (and fit an int), got {l_occ}, {l_free}")
    return l_occ, l_free, l_min, l_max


def build_lut(mode="ternary", l_occ=85, l_free=40, l_min=-200, l_max=350, occ_threshold=None, free_threshold=None) -> np.ndarray:
    """int8 (l_max - l_min + 1,): the payload of log-odds L is lut[L - l_min]. "ternary": 100 for L >= occ_threshold
    (default l_occ: one occupied observation), 0 for L <= free_threshold (default -l_free), -1 between them.
    "probability": rint(100 / (1 + exp(-L / 100))), log-odds in hundredths of a nat."""
    l_occ, l_free, l_min, l_max = _levels(l_occ, l_free, l_min, l_max)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    L = np.arange(l_min, l_max + 1, dtype=np.int64)
    if mode == "probability":
        if occ_threshold is not None or free_threshold is not None:
            raise ValueError("thresholds belong to mode 'ternary'")
        return np.rint(100.0 / (1.0 + np.exp(-L / 100.0))).astype(np.int8)
    occ = l_occ if occ_threshold is None else occ_threshold
    free = -l_free if free_threshold is None else free_threshold
    for name, v in (("occ_threshold", occ), ("free_threshold", free)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not int(free) < int(occ):
        raise ValueError(f"free_threshold {free} must lie below occ_threshold {occ}")
    return np.where(L >= int(occ), 100, np.where(L <= int(free), 0, -1)).astype(np.int8)


def map_params(size_cells, grid_hw, ros_layout=False, l_occ=85, l_free=40, l_min=-200, l_max=350, cull=True) -> N.MapParams:
    """bugseg_map_params for an Hm x Wm window and h x w grids. ValueError for a side outside 1..4096 and for
    levels outside -32768 < l_min < 0 < l_max <= 32767, l_occ, l_free >= 1."""
    Hm, Wm = _size(size_cells)
    h, w = _size(grid_hw, "grid_hw")
    l_occ, l_free, l_min, l_max = _levels(l_occ, l_free, l_min, l_max)
    p = N.MapParams()
    p.map_rows, p.map_cols, p.grid_rows, p.grid_cols = Hm, Wm, h, w
    p.ros_layout, p.cull = int(bool(ros_layout)), int(bool(cull))
    p.l_occ, p.l_free, p.l_min, p.l_max = l_occ, l_free, l_min, l_max
    return p


def occupancy_msg(data, origin_cells, cell_m, stamp=None, frame_id="map"):
    """The nav_msgs/OccupancyGrid of a payload (Hm, Wm) int8 in window order (occgrid_to_ros's message types: the
    real ones where ROS is installed): width Wm, height Hm, resolution cell_m, origin (wx0 cell_m, wy0 cell_m, 0)
    with the identity orientation, data row by row."""
    from . import occgrid_to_ros as O
    d = np.asarray(data)
    if d.ndim != 2 or d.dtype != np.int8:
        raise ValueError("data must be an int8 (Hm, Wm) array")
    cell = _cell(cell_m)
    msg = O.OccupancyGrid()
    msg.header = O.Header()
    msg.header.frame_id = frame_id
    msg.header.stamp = O._now() if stamp is None else stamp
    msg.info = O.MapMetaData()
    msg.info.resolution = cell
    msg.info.width, msg.info.height = int(d.shape[1]), int(d.shape[0])
    msg.info.origin = O.Pose()
    msg.info.origin.position = O.Point()
    msg.info.origin.position.x = origin_cells[0] * cell
    msg.info.origin.position.y = origin_cells[1] * cell
    msg.info.origin.position.z = 0.0
    msg.info.origin.orientation = O.Quaternion()
    msg.info.origin.orientation.x = msg.info.origin.orientation.y = msg.info.origin.orientation.z = 0.0
    msg.info.origin.orientation.w = 1.0
    msg.info.map_load_time = O._now()
    msg.data = d.reshape(-1).tolist()
    return msg


class LocalMap:
    """The device-resident map. size_cells = (Hm, Wm) window cells of cell_m metres, axes aligned to the world:
    window cell (i, j) is world cell (wx0 + j, wy0 + i). grid_hw = (h, w): the grids are int8 (B, h, w), forward up
    and the base point at the bottom centre as the rasteriser writes them, or with ros_layout (B, w, h) in ROS data
    order. State: one int16 of log-odds per cell, -32768 for a cell never observed, stored as a torus so that
    scrolling moves nothing.

      update(grids, poses)   set_poses, then fuse: the payload, int8 (Hm, Wm), a device tensor owned by the map
      set_poses(poses)       places the window and sends the record up: a pinned copy and an asynchronous transfer
                             on the current stream, no synchronisation. It advances the map's window, so every call
                             is followed by exactly one fuse or one replay, on the same stream
      fuse(grids)            the launch alone, reading the record last sent; may be captured
      capture(grids)         the launch on this grid buffer as a graph -> replay
      reset()                the map is fresh again; the state buffer is not touched, and need not be

    Any refusal raises before anything is launched."""

    def __init__(self, size_cells, cell_m, grid_hw, ros_layout=False, mode="ternary", l_occ=85, l_free=40, l_min=-200,
                 l_max=350, occ_threshold=None, free_threshold=None, cull=True, device=None):
        self.size_cells = _size(size_cells)
        self.cell_m = _cell(cell_m)
        self.grid_hw = _size(grid_hw, "grid_hw")
        self.ros_layout = bool(ros_layout)
        self.mode = mode
        lut = build_lut(mode, l_occ, l_free, l_min, l_max, occ_threshold, free_threshold)
        self._params = map_params(self.size_cells, self.grid_hw, ros_layout, l_occ, l_free, l_min, l_max, cull)
        N.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self._ctx = N.shared_context(self.device.index)
        Hm, Wm = self.size_cells
        words = RECORD_HEADER + RECORD_FRAME * MAX_B
        with torch.cuda.device(self.device):
            self._state = torch.empty((Hm, Wm), dtype=torch.int16, device=self.device)
            self._out = torch.full((Hm, Wm), -1, dtype=torch.int8, device=self.device)
            self._lut = torch.from_numpy(lut).to(self.device)
            self._rec = torch.zeros(words, dtype=torch.int64, device=self.device)
            self._ring = [torch.zeros(words, dtype=torch.int64).pin_memory() for _ in range(RING)]
        self._sent = [None] * RING     # per pinned copy, the event behind its transfer
        self._turn = 0
        self._origin = None            # (wx0, wy0) once the window has been placed
        self._fresh = True
        self._frames = 0               # frames of the record last sent

    # ---- what the map is
    @property
    def origin_cells(self):
        """(wx0, wy0): the world cell of window cell (0, 0)."""
        Hm, Wm = self.size_cells
        return (-(Wm // 2), -(Hm // 2)) if self._origin is None else self._origin

    @property
    def origin_m(self):
        """The world position in metres of the window's first cell's corner: the OccupancyGrid origin."""
        wx0, wy0 = self.origin_cells
        return wx0 * self.cell_m, wy0 * self.cell_m

    @property
    def state_buffer(self) -> torch.Tensor:
        """The torus storage itself, int16 (Hm, Wm): world cell (X, Y) in slot (Y mod Hm, X mod Wm). For tests and
        diagnostics; state() is the readable form."""
        return self._state

    def state(self) -> torch.Tensor:
        """The log-odds in window order, int16 (Hm, Wm), a new device tensor: -32768 where nothing was observed."""
        if self._fresh or self._origin is None:
            return torch.full(self.size_cells, UNOBSERVED, dtype=torch.int16, device=self.device)
        Hm, Wm = self.size_cells
        wx0, wy0 = self._origin
        return torch.roll(self._state, shifts=(-(wy0 % Hm), -(wx0 % Wm)), dims=(0, 1))

    def reset(self) -> None:
        """Forget everything: the next update keeps nothing stored. The window stays where it is until then."""
        self._fresh = True

    # ---- updates
    def _grids(self, grids) -> torch.Tensor:
        h, w = self.grid_hw
        shape = (w, h) if self.ros_layout else (h, w)
        if not isinstance(grids, torch.Tensor) or grids.dtype != torch.int8 or grids.device != self.device:
            raise ValueError(f"grids must be an int8 tensor on {self.device}")
        if grids.dim() != 3 or tuple(grids.shape[1:]) != shape:
            raise ValueError(f"grids must have shape (B, {shape[0]}, {shape[1]}), got {tuple(grids.shape)}")
        if not 1 <= grids.shape[0] <= MAX_B:
            raise ValueError(f"a batch holds 1..{MAX_B} grids, got {grids.shape[0]}")
        if not grids.is_contiguous():
            raise ValueError("grids must be contiguous")
        return grids

    def set_poses(self, poses) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_poses inside a stream capture: a graph would replay the transfer of this one record; "
                               "capture fuse() alone and call set_poses before every replay")
        rec, origin = pose_record(poses, self.size_cells, self.cell_m, self._origin, self._fresh)
        k = self._turn
        self._turn = (k + 1) % RING
        if self._sent[k] is not None:
            self._sent[k].synchronize()     # (waits only when RING transfers are still on their way)
        n = len(rec)
        self._ring[k][:n] = torch.from_numpy(rec)
        st = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            # stream order keeps a record in flight whole: the transfer runs behind the launch that reads the last one
            self._rec[:n].copy_(self._ring[k][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        self._sent[k] = ev
        self._origin, self._fresh, self._frames = origin, False, (n - RECORD_HEADER) // RECORD_FRAME

    def fuse(self, grids) -> torch.Tensor:
        g = self._grids(grids)
        if g.shape[0] != self._frames:
            raise ValueError(f"the record last sent is for {self._frames} grids, got {g.shape[0]}")
        with torch.cuda.device(self.device):
            self._ctx.map_fuse(g, g.shape[0], self._params, self._rec, self._state, self._lut, self._out,
                               torch.cuda.current_stream(self.device))
        return self._out

    def update(self, grids, poses) -> torch.Tensor:
        g = self._grids(grids)
        if len(_poses(poses)) != g.shape[0]:
            raise ValueError(f"{g.shape[0]} grids need as many poses")
        self.set_poses(poses)
        return self.fuse(g)

    def capture(self, grids):
        """The launch on this grid buffer, recorded as a graph -> replay. replay() fuses whatever the buffer holds
        with the record set_poses sent last (for as many grids), into the tensor update returns; the buffer must
        stay alive and keep its address. Nothing runs during the capture and the map is not changed by it."""
        g = self._grids(grids)
        self._frames = g.shape[0]
        gc.collect()
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                self.fuse(g)
        finally:
            if gc_was_on:
                gc.enable()
        def replay():
            if self._frames != g.shape[0]:
                raise ValueError(f"the record last sent is for {self._frames} grids, the graph fuses {g.shape[0]}")
            graph.replay()
            return self._out

        return replay

    def to_msg(self, stamp=None, frame_id="map"):
        """The nav_msgs/OccupancyGrid of the map as the last update left it (occupancy_msg); synchronises."""
        return occupancy_msg(self._out.cpu().numpy(), self.origin_cells, self.cell_m, stamp, frame_id)
