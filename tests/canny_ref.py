"""Canny as DESIGN.md §6.19 pins it (cv2.Canny, apertureSize 3, L2gradient False), restated twice in NumPy,
independently of each other and of the device code, and the inputs the tests share.

  canny(img, t1, t2)         vectorised: padded slices for Sobel and the suppression, hysteresis by growing the
                             strong pixels into the candidates until nothing changes
  canny_loops(img, t1, t2)   one pixel at a time with an explicit stack, the shape of OpenCV's own loop: a
                             strong pixel is pushed when it is found, the stack flood turns the weak
                             8-neighbours of every popped pixel into edges
  nms(img, low, high)        the map of launch 0: 2 strong, 0 weak, 1 none (with the magnitude and gradients)
  hysteresis(map)            edges of a map (any byte other than 2 and 0 is none)

|dx| + |dy| is always even (dx + dy = 2 (se - nw + e - w + s - n)), so a magnitude of low + 1 or high + 1
does not exist for the even thresholds 50 and 150: the `ramp` case holds 48, 50, 52 and 148, 150, 152.
"""
from __future__ import annotations

import functools
import math

import numpy as np

TG22 = 13573            # int(tan(22.5 deg) * 2^15 + 0.5)
STRONG, WEAK, NONE = 2, 0, 1
THRESHOLDS = [(50, 150), (150, 50), (0, 0), (-1, 5000), (49.9, 150.9)]


def thresholds(t1, t2):
    """Step 1: floor, then swap if low > high."""
    low, high = int(math.floor(t1)), int(math.floor(t2))
    return (high, low) if low > high else (low, high)


# ---------------------------------------------------------------- vectorised
def sobel(img):
    p = np.pad(img.astype(np.int64), 1, mode="edge")
    nw, n, ne = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    w, e = p[1:-1, :-2], p[1:-1, 2:]
    sw, s, se = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    return (ne + 2 * e + se) - (nw + 2 * w + sw), (sw + 2 * s + se) - (nw + 2 * n + ne)


def direction_classes(dx, dy):
    """0: y < tg22x (left / right), 1: y > tg67x (up / down), 2: diagonal with s = +1, 3: diagonal with s = -1."""
    x, y = np.abs(dx), np.abs(dy) << 15
    tg22x = x * TG22
    tg67x = tg22x + (x << 16)
    s_neg = (dx ^ dy) < 0
    return np.where(y < tg22x, 0, np.where(y > tg67x, 1, np.where(s_neg, 3, 2)))


def nms(img, low, high, full=False):
    dx, dy = sobel(img)
    m = np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1)                                   # zero outside the image
    c = mp[1:-1, 1:-1]
    left, right, up, down = mp[1:-1, :-2], mp[1:-1, 2:], mp[:-2, 1:-1], mp[2:, 1:-1]
    ul, ur, dl, dr = mp[:-2, :-2], mp[:-2, 2:], mp[2:, :-2], mp[2:, 2:]
    cls = direction_classes(dx, dy)
    peak = np.where(cls == 0, (c > left) & (c >= right),
                    np.where(cls == 1, (c > up) & (c >= down),
                             np.where(cls == 2, (c > ul) & (c > dr), (c > ur) & (c > dl))))
    peak &= m > low
    out = np.where(peak, np.where(m > high, STRONG, WEAK), NONE).astype(np.uint8)
    return (out, m, dx, dy, cls) if full else out


def hysteresis(mp):
    cand = (mp == STRONG) | (mp == WEAK)
    edge = mp == STRONG
    while True:
        g = np.pad(edge, 1)
        grown = (g[:-2, :-2] | g[:-2, 1:-1] | g[:-2, 2:] | g[1:-1, :-2] | g[1:-1, 2:] | g[2:, :-2] | g[2:, 1:-1]
                 | g[2:, 2:] | edge) & cand
        if np.array_equal(grown, edge):
            return (edge * 255).astype(np.uint8)
        edge = grown


def canny(img, t1, t2):
    low, high = thresholds(t1, t2)
    return hysteresis(nms(img, low, high))


# ---------------------------------------------------------------- one pixel at a time
def nms_loops(img, low, high):
    H, W = img.shape
    px = img.tolist()

    def at(r, c):
        return px[min(max(r, 0), H - 1)][min(max(c, 0), W - 1)]

    dxs = [[0] * W for _ in range(H)]
    dys = [[0] * W for _ in range(H)]
    mag = [[0] * (W + 2) for _ in range(H + 2)]         # a zero frame of one pixel
    for r in range(H):
        for c in range(W):
            dx = at(r - 1, c + 1) + 2 * at(r, c + 1) + at(r + 1, c + 1) - at(r - 1, c - 1) - 2 * at(r, c - 1) - at(r + 1, c - 1)
            dy = at(r + 1, c - 1) + 2 * at(r + 1, c) + at(r + 1, c + 1) - at(r - 1, c - 1) - 2 * at(r - 1, c) - at(r - 1, c + 1)
            dxs[r][c], dys[r][c] = dx, dy
            mag[r + 1][c + 1] = abs(dx) + abs(dy)
    out = np.full((H, W), NONE, np.uint8)
    for r in range(H):
        for c in range(W):
            m = mag[r + 1][c + 1]
            if not m > low:
                continue
            dx, dy = dxs[r][c], dys[r][c]
            x, y = abs(dx), abs(dy) << 15
            tg22x = x * TG22
            tg67x = tg22x + (x << 16)
            if y < tg22x:
                ok = m > mag[r + 1][c] and m >= mag[r + 1][c + 2]
            elif y > tg67x:
                ok = m > mag[r][c + 1] and m >= mag[r + 2][c + 1]
            else:
                s = -1 if (dx ^ dy) < 0 else 1
                ok = m > mag[r][c + 1 - s] and m > mag[r + 2][c + 1 + s]
            if ok:
                out[r, c] = STRONG if m > high else WEAK
    return out


def hysteresis_loops(mp):
    H, W = mp.shape
    m = np.pad(np.where((mp == STRONG) | (mp == WEAK), mp, NONE).astype(np.uint8), 1, constant_values=NONE).tolist()
    stack = [(r, c) for r in range(1, H + 1) for c in range(1, W + 1) if m[r][c] == STRONG]
    while stack:
        r, c = stack.pop()
        for rr, cc in ((r - 1, c - 1), (r - 1, c), (r - 1, c + 1), (r, c - 1), (r, c + 1), (r + 1, c - 1), (r + 1, c), (r + 1, c + 1)):
            if m[rr][cc] == WEAK:
                m[rr][cc] = STRONG
                stack.append((rr, cc))
    return ((np.array(m, np.uint8)[1:-1, 1:-1] == STRONG) * 255).astype(np.uint8)


def canny_loops(img, t1, t2):
    low, high = thresholds(t1, t2)
    return hysteresis_loops(nms_loops(img, low, high))


# ---------------------------------------------------------------- the inputs the tests share
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 3), (17, 65), (33, 131), (48, 80), (100, 100)]
BIG = (480, 640)
CASE_NAMES = ("scene", "noise", "constant", "step_x", "step_y", "step_diag", "step_anti", "line", "ramp", "plateau",
              "tangent")


@functools.lru_cache(maxsize=None)
def scene(h, w, seed=0):
    """Gaussian blobs of both signs on a grey ground, with noise: closed contours of every orientation whose
    gradient runs from below the low threshold to above the high one. Made once per shape (the camera-sized
    one takes seconds) and shared read-only."""
    rng = np.random.default_rng(7000 + 131 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 110.0)
    for _ in range(max(3, h * w // 250)):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        sy, sx = rng.uniform(2.0, 7.0), rng.uniform(2.0, 7.0)
        amp = rng.uniform(25, 140) * rng.choice((-1.0, 1.0))
        img += amp * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
    img += rng.normal(0.0, 4.0, size=(h, w))
    res = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    res.setflags(write=False)
    return res


def ramp(h, w):
    """Stripes three columns wide on black; the height of stripe j in row r is base_j or base_j + 1. Beside a
    stripe's edge dx = d[r-1] + 2 d[r] + d[r+1] and |dy| = |d[r+1] - d[r-1]|, so heights around 12.5 and 37.5
    put magnitudes on 48, 50, 52 and 148, 150, 152."""
    img = np.zeros((h, w), np.uint8)
    base = (12, 37, 11, 38, 13, 36, 12, 37)
    r = np.arange(h)
    for j in range((w + 5) // 6):
        d = base[j % len(base)] + ((r * (j % 3 + 1) + j) // 2) % 2
        img[:, 6 * j + 3:6 * j + 6] = d[:, None]
    return img


def plateau(h, w):
    """Linear ramps: along x in the top half (slopes 7, 13, 0 over runs of 8 columns), along y in the bottom
    half. Inside a run the magnitude is constant: only the first pixel of a plateau can pass `>` on one side and
    `>=` on the other."""
    slopes = np.array([7, 13, 0, 20, 7, 7, 0, 13])
    n = max(h, w)
    prof = np.concatenate([[0], np.cumsum(slopes[(np.arange(n - 1) // 8) % len(slopes)])]) % 256
    tri = np.minimum(prof, 255 - prof) * 2                              # no wrap-around step
    img = np.zeros((h, w), np.int64)
    img[:h // 2] = tri[None, :w]
    img[h // 2:] = tri[:h, None][h // 2:]
    return np.clip(img, 0, 255).astype(np.uint8)


def _tangent_with(h, w, sharp, phase):
    """Four bands, each a soft edge whose normal makes 22.5, 67.5, 112.5, 157.5 degrees with the x axis."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w))
    bw = max(1, -(-w // 4))
    for k, deg in enumerate((22.5, 67.5, 112.5, 157.5)):
        t = math.radians(deg)
        x0 = k * bw + bw / 2.0
        d = (xx - x0) * math.cos(t) + (yy - h / 2.0) * math.sin(t) + phase
        band = 128.0 + 110.0 * np.tanh(d / sharp)
        img[:, k * bw:(k + 1) * bw] = band[:, k * bw:(k + 1) * bw]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def near_boundary_counts(img, low):
    """Per side of the tg22x and the tg67x boundary: the pixels with m > low whose |dy| 2^15 lies within a
    sixteenth of the boundary value on that side -> (below 22, above 22, below 67, above 67)."""
    dx, dy = sobel(img)
    m = np.abs(dx) + np.abs(dy)
    x, y = np.abs(dx), np.abs(dy) << 15
    tg22x = x * TG22
    tg67x = tg22x + (x << 16)
    on = m > low
    return (int((on & (y < tg22x) & (y >= tg22x - tg22x // 16)).sum()), int((on & (y >= tg22x) & (y <= tg22x + tg22x // 16)).sum()),
            int((on & (y <= tg67x) & (y >= tg67x - tg67x // 16)).sum()), int((on & (y > tg67x) & (y <= tg67x + tg67x // 16)).sum()))


def tangent(h, w):
    """The soft edges whose gradients lie closest around both direction boundaries, by search over the
    edge's width and phase: the choice with the largest smallest count of near_boundary_counts."""
    best, best_img = -1, None
    for sharp in (1.5, 2.5, 4.0):
        for phase in (0.0, 0.37):
            img = _tangent_with(h, w, sharp, phase)
            score = min(near_boundary_counts(img, 50))
            if score > best:
                best, best_img = score, img
    return best_img


@functools.lru_cache(maxsize=None)
def images(h, w):
    """(len(CASE_NAMES), h, w) u8, in the order of CASE_NAMES; made once per shape and shared read-only."""
    rng = np.random.default_rng(4000 + 31 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    line = np.zeros((h, w), np.uint8)
    line[h // 2, :] = 255
    line[:, w // 3] = 255
    a = [scene(h, w), rng.integers(0, 256, size=(h, w), dtype=np.uint8), np.full((h, w), 93, np.uint8),
         ((xx >= w // 2) * 255).astype(np.uint8), ((yy >= h // 2) * 255).astype(np.uint8),
         ((xx + yy >= (h + w) // 2) * 255).astype(np.uint8), ((xx - yy >= (w - h) // 2) * 255).astype(np.uint8),
         line, ramp(h, w), plateau(h, w), tangent(h, w)]
    res = np.stack(a)
    res.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def cases_with_ref(h, w, t1=50, t2=150, only=None):
    """-> (names, images (n, h, w), maps (n, h, w), edges (n, h, w)) by the vectorised restatement, computed
    once per argument set and shared read-only."""
    names = CASE_NAMES if only is None else tuple(only)
    im = images(h, w)[[CASE_NAMES.index(n) for n in names]]
    low, high = thresholds(t1, t2)
    maps = np.stack([nms(i, low, high) for i in im])
    edges = np.stack([hysteresis(m) for m in maps])
    res = (names, im, maps, edges)
    for a in res[1:]:
        a.setflags(write=False)
    return res


def kind_counts(img, t1=50, t2=150):
    """What a frame exercises: candidates per direction class, strong, weak kept, weak dropped."""
    low, high = thresholds(t1, t2)
    mp, m, dx, dy, cls = nms(img, low, high, full=True)
    edges = hysteresis(mp)
    c = (mp != NONE)
    return {"left_right": int((c & (cls == 0)).sum()), "up_down": int((c & (cls == 1)).sum()),
            "diag_pos": int((c & (cls == 2)).sum()), "diag_neg": int((c & (cls == 3)).sum()),
            "strong": int((mp == STRONG).sum()), "weak_kept": int(((mp == WEAK) & (edges == 255)).sum()),
            "weak_dropped": int(((mp == WEAK) & (edges == 0)).sum())}


# ---------------------------------------------------------------- hand-made maps for the hysteresis alone
MAP_SHAPES = [(48, 200), (33, 131)]
MAP_NAMES = ("spiral_strong_last", "spiral_no_strong", "staircase", "two_chains", "checkerboard", "all_weak", "all_none",
             "all_strong", "random_a", "random_b")


def _spiral(h, w):
    """A rectangular spiral of weak pixels from (0, 0) inwards, one empty row or column between its arms: one
    path, so one component."""
    mp = np.full((h, w), NONE, np.uint8)
    r, c, dr, dc, turns = 0, 0, 0, 1, 0
    mp[0, 0] = WEAK
    while turns < 2:
        nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        if 0 <= nr < h and 0 <= nc < w and mp[nr, nc] != WEAK and not (0 <= ar < h and 0 <= ac < w and mp[ar, ac] == WEAK):
            r, c, turns = nr, nc, 0
            mp[r, c] = WEAK
        else:
            dr, dc, turns = dc, -dr, turns + 1
    return mp


def maps(h, w):
    """(len(MAP_NAMES), h, w) u8 maps, in the order of MAP_NAMES."""
    rng = np.random.default_rng(9000 + 17 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    sp = _spiral(h, w)
    last = np.argwhere(sp == WEAK)[-1]                   # the raster-last pixel of the spiral
    sp_s = sp.copy()
    sp_s[last[0], last[1]] = STRONG
    # a pure diagonal through (15, 63), (16, 64): the corners of the labelling tiles (16 x 64), crossed by a short
    # anti-diagonal through (16, 65), (17, 64); the strong pixel is the diagonal's last. A parallel diagonal eight
    # columns on holds no strong pixel
    stair = np.full((h, w), NONE, np.uint8)
    diag = (yy - 16) == (xx - 64)
    stair[diag] = WEAK
    stair[((yy - 16) == 1 - (xx - 64)) & (np.abs(xx - 64) <= 3)] = WEAK
    stair[(yy - 16) == (xx - 72)] = WEAK
    stair[tuple(np.argwhere(diag)[-1])] = STRONG
    # two chains one "none" pixel apart, crossing tile borders in both directions; only the first is strong
    two = np.full((h, w), NONE, np.uint8)
    zig = (xx // 3) % 2
    two[(yy == h // 2 - 2 + zig)] = WEAK
    two[(yy == h // 2 + 1 + zig)] = WEAK
    two[h // 2 - 2 + zig[0, w - 1], w - 1] = STRONG
    # a checkerboard of weak pixels (8-connected through its diagonals), one strong pixel
    chk = np.where((yy + xx) % 2 == 0, WEAK, NONE).astype(np.uint8)
    chk[h - 1, (h - 1) % 2] = STRONG
    res = [sp_s, sp, stair, two, chk, np.full((h, w), WEAK, np.uint8), np.full((h, w), NONE, np.uint8),
           np.full((h, w), STRONG, np.uint8)]
    for _ in range(2):
        u = rng.random((h, w))
        # near the 8-neighbour site percolation threshold: large twisted components; the other bytes stand
        # for "none" in every value
        mp = rng.integers(3, 256, size=(h, w)).astype(np.uint8)
        mp[u < 0.25] = NONE
        mp[u >= 0.62] = WEAK
        mp[rng.random((h, w)) < 0.002] = STRONG
        res.append(mp)
    return np.stack(res)


@functools.lru_cache(maxsize=None)
def maps_with_ref(h, w):
    mp = maps(h, w)
    edges = np.stack([hysteresis(m) for m in mp])
    mp.setflags(write=False)
    edges.setflags(write=False)
    return MAP_NAMES, mp, edges
