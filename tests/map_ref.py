"""The rolling local map restated, by two routes that share nothing but the integer update record
they take as input (mapping.pose_record builds it; include/bugseg.h describes it):

  fuse_np     vectorised NumPy in int64; the state travels as a window-ordered array that is cut and pasted when
              the window moves
  fuse_walk   a walk over the window cell by cell in Python integers; the state travels as a dictionary from world
              cell to log-odds

Neither knows of the torus the device stores its state in. Also here: the look-up tables restated, a synthetic
world with a wall for the end-to-end check, and the cases the host and GPU tests share.
"""
from __future__ import annotations

import functools
import math

import numpy as np

UNOBS = -32768
HDR, FRM = 8, 4
DEFAULTS = dict(l_occ=85, l_free=40, l_min=-200, l_max=350)


def lut_ref(mode, l_occ=85, l_free=40, l_min=-200, l_max=350, occ_threshold=None, free_threshold=None):
    occ = l_occ if occ_threshold is None else occ_threshold
    free = -l_free if free_threshold is None else free_threshold
    out = []
    for L in range(l_min, l_max + 1):
        if mode == "probability":
            out.append(int(round(100.0 / (1.0 + math.exp(-L / 100.0)))))
        else:
            out.append(100 if L >= occ else 0 if L <= free else -1)
    return np.array(out, np.int8)


def config(grid_hw, ros=False, mode="ternary", **levels):
    lv = dict(DEFAULTS)
    thr = {k: levels.pop(k) for k in ("occ_threshold", "free_threshold") if k in levels}
    lv.update(levels)
    return dict(h=grid_hw[0], w=grid_hw[1], ros=bool(ros), lut=lut_ref(mode, **lv, **thr), **lv)


def to_ros(grids):
    """(B, h, w) plain grids -> (B, w, h) in ROS data order, G[::-1, ::-1].T per grid."""
    return np.ascontiguousarray(np.asarray(grids)[:, ::-1, ::-1].transpose(0, 2, 1))


def carry(prev, rec, size):
    """The state a window starts an update with: `prev` (window order of the previous origin, or None) moved to the
    new origin; what was not in the previous window, and everything when the record says fresh, is unobserved."""
    Hm, Wm = size
    wx0, wy0, px0, py0, fresh = (int(v) for v in rec[:5])
    new = np.full((Hm, Wm), UNOBS, np.int16)
    if fresh or prev is None:
        return new
    dx, dy = wx0 - px0, wy0 - py0                  # new cell (i, j) was cell (i + dy, j + dx)
    i0, i1, j0, j1 = max(0, -dy), min(Hm, Hm - dy), max(0, -dx), min(Wm, Wm - dx)
    if i0 < i1 and j0 < j1:
        new[i0:i1, j0:j1] = prev[i0 + dy:i1 + dy, j0 + dx:j1 + dx]
    return new


def fuse_np(prev, rec, grids, size, cfg):
    """-> (state int16 (Hm, Wm) in window order, payload int8 (Hm, Wm))."""
    Hm, Wm = size
    h, w = cfg["h"], cfg["w"]
    rec = np.asarray(rec, np.int64)
    L = carry(prev, rec, size).astype(np.int64)
    i, j = np.mgrid[0:Hm, 0:Wm].astype(np.int64)
    half = np.int64(w) << 15
    for k in range(len(grids)):
        C, S, Ox, Oy = rec[HDR + FRM * k:HDR + FRM * k + 4]
        if C == 0 and S == 0:
            continue
        xq, yq = C * j + S * i + Ox, -S * j + C * i + Oy
        fx = xq >> 16
        g = np.asarray(grids[k])
        if cfg["ros"]:
            c = (yq + half) >> 16
            hit = (fx >= 0) & (fx < h) & (c >= 0) & (c < w)
            v = g[np.where(hit, c, 0), np.where(hit, fx, 0)]
        else:
            c = (half - yq) >> 16
            hit = (fx >= 0) & (fx < h) & (c >= 0) & (c < w)
            v = g[np.where(hit, h - 1 - fx, 0), np.where(hit, c, 0)]
        v = np.where(hit, v.astype(np.int64), -1)
        base = np.where(L == UNOBS, 0, L)
        L = np.where(v == 100, np.clip(base + cfg["l_occ"], cfg["l_min"], cfg["l_max"]),
                     np.where(v == 0, np.clip(base - cfg["l_free"], cfg["l_min"], cfg["l_max"]), L))
    seen = L != UNOBS
    out = np.where(seen, cfg["lut"][np.where(seen, L - cfg["l_min"], 0)], -1).astype(np.int8)
    return L.astype(np.int16), out


def fuse_walk(prev, rec, grids, size, cfg):
    """The same, cell by cell in Python integers."""
    Hm, Wm = size
    h, w = cfg["h"], cfg["w"]
    r = [int(v) for v in rec]
    wx0, wy0, px0, py0, fresh = r[:5]
    old = {}
    if not fresh and prev is not None:
        for i, row in enumerate(np.asarray(prev).tolist()):
            for j, val in enumerate(row):
                old[(px0 + j, py0 + i)] = val
    frames = [(k, r[HDR + FRM * k:HDR + FRM * k + 4]) for k in range(len(grids))]
    frames = [(np.asarray(grids[k]).tolist(), f) for k, f in frames if f[0] != 0 or f[1] != 0]
    lut = cfg["lut"].tolist()
    lo, hi, up, down = cfg["l_min"], cfg["l_max"], cfg["l_occ"], cfg["l_free"]
    state = [[UNOBS] * Wm for _ in range(Hm)]
    out = [[-1] * Wm for _ in range(Hm)]
    for i in range(Hm):
        for j in range(Wm):
            L = old.get((wx0 + j, wy0 + i), UNOBS)
            for g, (C, S, Ox, Oy) in frames:
                fx = (C * j + S * i + Ox) >> 16
                yq = -S * j + C * i + Oy
                if fx < 0 or fx >= h:
                    continue
                if cfg["ros"]:
                    c = (yq + (w << 15)) >> 16
                    if c < 0 or c >= w:
                        continue
                    v = g[c][fx]
                else:
                    c = ((w << 15) - yq) >> 16
                    if c < 0 or c >= w:
                        continue
                    v = g[h - 1 - fx][c]
                if v == 100:
                    L = min(max((0 if L == UNOBS else L) + up, lo), hi)
                elif v == 0:
                    L = min(max((0 if L == UNOBS else L) - down, lo), hi)
            state[i][j] = L
            if L != UNOBS:
                out[i][j] = lut[L - lo]
    return np.array(state, np.int16), np.array(out, np.int8)


# ---- a synthetic world for the end-to-end check: free ground with a wall two cells thick
WALL_X = (14, 15)                 # world cells X of the wall
WALL_Y = (-30, 30)                # its extent in Y, half-open


def world_value(X, Y):
    X, Y = np.asarray(X), np.asarray(Y)
    wall = (X >= WALL_X[0]) & (X <= WALL_X[1]) & (Y >= WALL_Y[0]) & (Y < WALL_Y[1])
    return np.where(wall, 100, 0).astype(np.int8)


def sample_world(pose, grid_hw, cell_m, rng=None, flip=0.1, drop=0.2):
    """The grid a sensor at `pose` gives: every cell's centre looked up in the world (float64 geometry); with `rng`,
    a share `flip` of the cells then reports the opposite and a share `drop` nothing."""
    h, w = grid_hw
    row, col = np.mgrid[0:h, 0:w]
    xf, yl = (h - 1 - row + 0.5), (w / 2.0 - col - 0.5)
    c, s = math.cos(pose[2]), math.sin(pose[2])
    X = np.floor(pose[0] / cell_m + c * xf - s * yl).astype(np.int64)
    Y = np.floor(pose[1] / cell_m + s * xf + c * yl).astype(np.int64)
    g = world_value(X, Y)
    if rng is not None:
        u = rng.uniform(size=g.shape)
        g = np.where(u < flip, 100 - g, np.where(u < flip + drop, -1, g)).astype(np.int8)
    return g


def wall_trajectory(n=24, seed=0):
    """Poses that drive towards the wall on a gentle curve, in metres and radians (cell_m = 0.5)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)
    x = -6.0 + 9.0 * t + rng.uniform(-0.05, 0.05, n)
    y = 2.0 * np.sin(2.0 * t) + rng.uniform(-0.05, 0.05, n)
    yaw = 0.5 * np.cos(2.0 * t) + rng.uniform(-0.02, 0.02, n)
    return np.stack([x, y, yaw], axis=1)


# ---- the shared cases. A case: a window, a grid shape, and steps: one (grids (B, h, w) plain layout, poses (B, 3))
# per update. cell_m is 0.5 everywhere.
CELL_M = 0.5
SMALL = dict(size=(24, 20), grid_hw=(12, 9))       # odd w: the base point sits in the middle of a cell
MID = dict(size=(33, 47), grid_hw=(16, 16))
BIG = dict(size=(256, 256), grid_hw=(200, 200))


def _rand_grids(rng, B, hw, p=(0.3, 0.4, 0.3)):
    return rng.choice(np.array([-1, 0, 100], np.int8), size=(B,) + tuple(hw), p=p)


def _case(name, shape, steps, **kw):
    return dict(name=name, size=shape["size"], grid_hw=shape["grid_hw"], steps=steps, kw=kw)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261021)
    out = []
    nan, inf = float("nan"), float("inf")

    def poses(*rows):
        return np.array(rows, np.float64)

    def step(shape, ps, **kw):
        return (_rand_grids(rng, len(ps), shape["grid_hw"], **kw), np.asarray(ps, np.float64))

    for shape, tag in ((SMALL, "small"), (MID, "mid")):
        for yname, yaw in (("yaw0", 0.0), ("yaw90", math.pi / 2), ("yaw180", math.pi), ("yaw-135", -3 * math.pi / 4),
                           ("yaw_any", 0.7391)):
            out.append(_case(f"{tag}_{yname}", shape, [step(shape, poses((0.31, -0.17, yaw), (0.83, 0.12, yaw), (1.44, 0.29, yaw)))]))
        out.append(_case(f"{tag}_negative_world", shape, [step(shape, poses((-37.3, -12.9, 0.4), (-37.0, -12.6, 0.5)))]))
        a = (1.2, 0.7, 0.3)
        # (the first update of the scroll cases looks four ways, so that observed cells reach the window's edges and
        # a scroll of a few cells both keeps cells and clears cells)
        around = poses(*[(a[0], a[1], a[2] + q * math.pi / 2) for q in range(4)])
        back = -0.3 if tag == "small" else -3.3                      # 3 cells back in x; 9 in the wider window
        out.append(_case(f"{tag}_scroll_zero", shape, [step(shape, around), step(shape, poses(a, a))]))
        out.append(_case(f"{tag}_scroll_x", shape, [step(shape, around), step(shape, poses((back, 0.7, 0.3),))]))
        out.append(_case(f"{tag}_scroll_y", shape, [step(shape, around), step(shape, poses((1.2, 1.9, 0.3),))]))
        out.append(_case(f"{tag}_scroll_xy", shape, [step(shape, around), step(shape, poses((2.2, 2.3, 0.2),)),
                                                     step(shape, poses((0.1, 3.9, -0.4),))]))
        out.append(_case(f"{tag}_scroll_far", shape, [step(shape, around), step(shape, poses((90.0, -70.0, 1.0),))]))
        out.append(_case(f"{tag}_frame_outside", shape, [step(shape, poses(a, (400.0, 400.0, 0.2), (1.5, 0.6, 0.4)))]))
        out.append(_case(f"{tag}_nonfinite_mid", shape, [step(shape, poses(a, (nan, 0.0, 0.0), (1.5, 0.6, 0.4)))]))
        out.append(_case(f"{tag}_nonfinite_end", shape, [step(shape, poses(a, (1.5, 0.6, 0.4), (0.0, inf, 0.0))),
                                                         step(shape, poses((nan, nan, nan),))]))
        out.append(_case(f"{tag}_all_unknown", shape, [step(shape, poses(a, a)),
                                                       (np.full((2,) + shape["grid_hw"], -1, np.int8), poses(a, a))]))
        out.append(_case(f"{tag}_b1", shape, [step(shape, poses(a))]))
        tr = np.stack([np.linspace(0.013, 3.0, 70), 0.007 + np.linspace(0.0, 1.0, 70) ** 2, np.linspace(0.0, 0.8, 70)], axis=1)
        out.append(_case(f"{tag}_b70", shape, [step(shape, tr)]))
        out.append(_case(f"{tag}_three_updates", shape, [step(shape, tr[0:5]), step(shape, tr[30:35]), step(shape, tr[65:70])]))
        out.append(_case(f"{tag}_probability", shape, [step(shape, tr[0:9]), step(shape, tr[20:29])], mode="probability"))
        out.append(_case(f"{tag}_levels", shape, [step(shape, tr[0:9]), step(shape, tr[9:18])], l_occ=30000, l_free=7,
                         l_min=-32767, l_max=32767, occ_threshold=1, free_threshold=-8))
        full = lambda v: np.full((1,) + shape["grid_hw"], v, np.int8)
        up, down = [full(100)] * 6 + [full(0)] * 3, [full(0)] * 3 + [full(100)] * 6
        for nm, seq in (("clamp_occ_then_free", up), ("clamp_free_then_occ", down),
                        ("clamp_down", [full(0)] * 7 + [full(100)])):
            out.append(_case(f"{tag}_{nm}", shape, [(np.concatenate(seq), np.repeat(poses(a), len(seq), axis=0))]))
    tr = np.stack([np.linspace(-20.0, 20.0, 8), 8.0 * np.sin(np.linspace(0.0, 2.0, 8)), np.linspace(0.3, -0.9, 8)], axis=1)
    out.append(_case("big", BIG, [step(BIG, tr)]))
    return tuple(out)


def ties(rec, size, w):
    """How many (frame, window cell) pairs put a cell centre exactly on a boundary between two grid columns. Only
    there do the two layouts differ: floor(w / 2 - yl) and w - 1 - floor(yl + w / 2) are the same number unless
    yl + w / 2 is whole. Where a case has none, ROS-layout input must give what plain input gives."""
    i, j = np.mgrid[0:size[0], 0:size[1]].astype(np.int64)
    n = 0
    for k in range((len(rec) - HDR) // FRM):
        C, S, _, Oy = (np.int64(v) for v in rec[HDR + FRM * k:HDR + FRM * k + 4])
        if C != 0 or S != 0:
            n += int((((-S * j + C * i + Oy + (np.int64(w) << 15)) & 0xFFFF) == 0).sum())
    return n


def run_case(c, pose_record, route=fuse_np, ros=False):
    """A case through a route, update by update -> [(record, state in window order, payload)]. pose_record is
    mapping.pose_record: the routes start from the integers it gives."""
    cfg = config(c["grid_hw"], ros=ros, **c["kw"])
    origin, prev, res = None, None, []
    for grids, poses in c["steps"]:
        rec, origin = pose_record(poses, c["size"], CELL_M, origin, prev is None)
        prev, out = route(prev, rec, to_ros(grids) if ros else grids, c["size"], cfg)
        res.append((rec, prev, out))
    return res


def wall_agreement(pose_record, seed, route=fuse_np, size=(64, 64), grid_hw=(24, 17), batch=8):
    """The end-to-end check: noisy grids sampled from the world along wall_trajectory(seed), fused batch by batch ->
    (observed cells, the share of them whose ternary payload is the world's value, observed wall cells, the share
    of those that read occupied)."""
    rng = np.random.default_rng(1000 + seed)
    tr = wall_trajectory(seed=seed)
    cfg = config(grid_hw)
    origin, prev, out = None, None, None
    for s0 in range(0, len(tr), batch):
        ps = tr[s0:s0 + batch]
        grids = np.stack([sample_world(p, grid_hw, CELL_M, rng) for p in ps])
        rec, origin = pose_record(ps, size, CELL_M, origin, prev is None)
        prev, out = route(prev, rec, grids, size, cfg)
    i, j = np.mgrid[0:size[0], 0:size[1]]
    truth = world_value(origin[0] + j, origin[1] + i)
    seen, wall = out != -1, truth == 100
    return (int(seen.sum()), float((out[seen] == truth[seen]).mean()), int((seen & wall).sum()),
            float((out[seen & wall] == 100).mean()))


def case(name):
    return next(c for c in cases() if c["name"] == name)
