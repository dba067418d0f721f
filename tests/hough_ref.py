"""The standard Hough transform as DESIGN.md §6.21 pins it (cv2.HoughLines), restated twice in NumPy / Python,
independently of each other and of the device code, the inputs the tests share, and the reference of warp_image.

  hough(img, ...)         vectorised: one pass per angle over all set pixels in float32 arrays, a histogram per
                          angle, the peak test on shifted slices, one lexsort
  hough_loops(img, ...)   the pixel, angle and peak loops written out in Python floats. A product of two float32
                          values is exact in double and a sum of two is rounded once more to float32 without a
                          second error (53 >= 2 * 24 + 2 bits), so f32(.) after each operation gives the float32
                          result. For the camera-sized frame (`rows=True`) the angle loop alone is an array
                          operation; the pixel and peak loops stay
  trig(par)               the table: a float32 angle stepped in float32, math.cos / math.sin in double

Both return (lines (max_lines, 2) float32, count, peaks, votes of the stored lines).
"""
from __future__ import annotations

import functools
import math
import struct

import numpy as np

import canny_ref

MAX_LINES_CAP = 4096


def f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


# ---------------------------------------------------------------- parameters and the table
def params(h, w, rho, theta, min_theta=0.0, max_theta=math.pi):
    rho32, theta32 = f32(rho), f32(theta)
    numangle = int(math.floor((max_theta - min_theta) / theta32)) + 1
    if numangle > 1 and abs(math.pi - (numangle - 1) * theta32) < theta32 / 2:
        numangle -= 1
    q = (2 * (w + h) + 1) / rho32
    numrho = int(math.floor(q))
    frac = q - numrho
    if frac > 0.5 or (frac == 0.5 and numrho % 2 == 1):            # cvRound: half to even
        numrho += 1
    return dict(h=h, w=w, rho=rho32, theta=theta32, min_theta=f32(min_theta), numangle=numangle, numrho=numrho)


def trig(par):
    """(2, numangle) float32: cos(ang) / rho, then sin(ang) / rho."""
    irho = np.float32(1.0) / np.float32(par["rho"])
    ang = np.float32(par["min_theta"])
    step = np.float32(par["theta"])
    tab = np.empty((2, par["numangle"]), np.float32)
    for n in range(par["numangle"]):
        tab[0, n] = np.float32(math.cos(float(ang)) * float(irho))
        tab[1, n] = np.float32(math.sin(float(ang)) * float(irho))
        ang = np.float32(ang + step)
    return tab


# ---------------------------------------------------------------- vectorised
def accumulate(img, par, tab=None):
    tab = trig(par) if tab is None else tab
    A, R = par["numangle"], par["numrho"]
    acc = np.zeros((A + 2, R + 2), np.int32)
    ys, xs = np.nonzero(img)
    xf, yf = xs.astype(np.float32), ys.astype(np.float32)
    half = (R - 1) // 2
    for n in range(A):
        s = xf * tab[0, n] + yf * tab[1, n]                         # float32 arrays: every operation rounds
        assert s.dtype == np.float32
        r = np.rint(s).astype(np.int64) + half
        r = r[(r >= 0) & (r < R)]
        acc[n + 1] += np.bincount(r + 1, minlength=R + 2).astype(np.int32)
    return acc


def select(acc, par, threshold, max_lines):
    """Peaks of a bordered accumulator, ordered, cut, decoded."""
    A, R = par["numangle"], par["numrho"]
    a = acc[1:-1, 1:-1].astype(np.int64)
    left, right = acc[1:-1, :-2], acc[1:-1, 2:]
    up, down = acc[:-2, 1:-1], acc[2:, 1:-1]
    pk = (a > threshold) & (a > left) & (a >= right) & (a > up) & (a >= down)
    n, r = np.nonzero(pk)
    idx = (n + 1) * (R + 2) + r + 1
    votes = a[n, r]
    order = np.lexsort((idx, -votes))
    return _decode(idx[order], votes[order], par, max_lines)


def _decode(idx, votes, par, max_lines):
    R = par["numrho"]
    peaks = len(idx)
    count = min(peaks, max_lines)
    idx, votes = np.asarray(idx[:count], np.int64), np.asarray(votes[:count], np.int64)
    n, r = idx // (R + 2) - 1, idx % (R + 2) - 1
    lines = np.zeros((max_lines, 2), np.float32)
    centre = np.float32(R - 1) * np.float32(0.5)
    lines[:count, 0] = (r.astype(np.float32) - centre) * np.float32(par["rho"])
    lines[:count, 1] = np.float32(par["min_theta"]) + n.astype(np.float32) * np.float32(par["theta"])
    return lines, count, peaks, votes


def hough(img, rho, theta, threshold, max_lines, min_theta=0.0, max_theta=math.pi):
    par = params(img.shape[0], img.shape[1], rho, theta, min_theta, max_theta)
    return select(accumulate(img, par), par, threshold, max_lines)


# ---------------------------------------------------------------- loops
def accumulate_loops(img, par, tab=None, rows=False):
    tab = trig(par) if tab is None else tab
    A, R = par["numangle"], par["numrho"]
    H, W = img.shape
    half = (R - 1) // 2
    acc = [[0] * (R + 2) for _ in range(A + 2)]
    px = img.tolist()
    if rows:
        cos, sin = tab[0].copy(), tab[1].copy()
        cells = np.zeros((A + 2) * (R + 2), np.int64)
        base = (np.arange(A) + 1) * (R + 2) + 1
        for i in range(H):
            row = px[i]
            for j in range(W):
                if row[j]:
                    r = np.rint(np.float32(j) * cos + np.float32(i) * sin).astype(np.int64) + half
                    ok = (r >= 0) & (r < R)
                    cells[(base + r)[ok]] += 1                        # (one cell per angle: no repeated index)
        return cells.reshape(A + 2, R + 2).astype(np.int32)
    tc, ts = [float(v) for v in tab[0]], [float(v) for v in tab[1]]
    pack, unpack = struct.Struct("f").pack, struct.Struct("f").unpack
    for i in range(H):
        row = px[i]
        for j in range(W):
            if not row[j]:
                continue
            for n in range(A):
                xc = unpack(pack(j * tc[n]))[0]
                ys = unpack(pack(i * ts[n]))[0]
                s = unpack(pack(xc + ys))[0]
                r = round(s) + half                                    # Python's round: half to even
                if 0 <= r < R:
                    acc[n + 1][r + 1] += 1
    return np.array(acc, np.int32)


def select_loops(acc, par, threshold, max_lines):
    A, R = par["numangle"], par["numrho"]
    g = np.asarray(acc).tolist()
    found = []
    for n in range(A):
        cur, above, below = g[n + 1], g[n], g[n + 2]
        for r in range(R):
            a = cur[r + 1]
            if a > threshold and a > cur[r] and a >= cur[r + 2] and a > above[r + 1] and a >= below[r + 1]:
                found.append((-a, (n + 1) * (R + 2) + r + 1))
    found.sort()
    return _decode([i for _, i in found], [-v for v, _ in found], par, max_lines)


def hough_loops(img, rho, theta, threshold, max_lines, min_theta=0.0, max_theta=math.pi, rows=False):
    par = params(img.shape[0], img.shape[1], rho, theta, min_theta, max_theta)
    return select_loops(accumulate_loops(img, par, rows=rows), par, threshold, max_lines)


# ---------------------------------------------------------------- the inputs the tests share
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (17, 65), (33, 131), (48, 80), (100, 100)]
BIG = (480, 640)
# (rho, theta, min_theta, max_theta)
PARAM_SETS = [(1.0, math.pi / 180, 0.0, math.pi), (2.0, math.pi / 180, 0.0, math.pi), (0.5, math.pi / 90, 0.0, math.pi),
              (1.0, math.pi / 360, 0.0, math.pi), (1.0, math.pi / 180, math.pi / 4, 3 * math.pi / 4)]
MAX_LINES = (1, 3, MAX_LINES_CAP)
CASE_NAMES = ("empty", "corners", "full", "row", "column", "diagonal", "antidiagonal", "parallel", "noise", "edges")
BIG_CASE = dict(threshold=20, peaks=24367, pixels=113363, max_votes=379, max_lines=(MAX_LINES_CAP, 7))


def thresholds(h, w):
    """0, a middle value, one no cell can pass (a cell has at most h * w votes)."""
    return (0, max(1, min(h, w) // 2), h * w)


@functools.lru_cache(maxsize=None)
def images(h, w):
    """(len(CASE_NAMES), h, w) u8 in the order of CASE_NAMES; set pixels hold 255 except where noted."""
    rng = np.random.default_rng(9000 + 37 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    z = lambda: np.zeros((h, w), np.uint8)
    corners = z()
    corners[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = (255, 1, 128, 7)        # any non-zero byte counts
    row, col, diag, anti, par = z(), z(), z(), z(), z()
    row[h // 2, :] = 255
    col[:, w // 3] = 200
    diag[yy == xx] = 255
    anti[yy == (min(h, w) - 1 - xx)] = 255
    par[:, w // 2] = 255
    par[:, min(w - 1, w // 2 + 1)] = 255
    noise = (rng.random((h, w)) < 0.12).astype(np.uint8) * rng.integers(1, 256, size=(h, w), dtype=np.uint8)
    edges = canny_ref.canny(canny_ref.scene(h, w), 50, 150)
    res = np.stack([z(), corners, np.full((h, w), 255, np.uint8), row, col, diag, anti, par, noise, edges])
    res.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def accumulators(h, w, k):
    """-> (par, table, accumulators (len(CASE_NAMES), numangle + 2, numrho + 2)) of images(h, w) under PARAM_SETS[k],
    by the vectorised restatement; computed once and shared read-only."""
    rho, theta, lo, hi = PARAM_SETS[k]
    par = params(h, w, rho, theta, lo, hi)
    tab = trig(par)
    acc = np.stack([accumulate(im, par, tab) for im in images(h, w)])
    acc.setflags(write=False)
    return par, tab, acc


@functools.lru_cache(maxsize=None)
def cases_with_ref(h, w, k, threshold, max_lines):
    """-> (lines (n, max_lines, 2), counts (n,), peaks (n,), votes per image) of images(h, w)."""
    par, tab, acc = accumulators(h, w, k)
    res = [select(a, par, threshold, max_lines) for a in acc]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32),
            [r[3] for r in res])


@functools.lru_cache(maxsize=None)
def big_edges():
    """The Canny edges (50, 150) of canny_ref's 480 x 640 noise frame."""
    h, w = BIG
    e = canny_ref.canny(canny_ref.images(h, w)[canny_ref.CASE_NAMES.index("noise")], 50, 150)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def big_accumulator():
    h, w = BIG
    rho, theta, lo, hi = PARAM_SETS[0]
    par = params(h, w, rho, theta, lo, hi)
    acc = accumulate(big_edges(), par)
    acc.setflags(write=False)
    return par, acc


def halfway_votes(img, par, tab):
    """How many (pixel, angle) pairs land exactly half-way between two integers before cvRound."""
    ys, xs = np.nonzero(img)
    xf, yf = xs.astype(np.float32), ys.astype(np.float32)
    n = 0
    for a in range(par["numangle"]):
        s = (xf * tab[0, a] + yf * tab[1, a]).astype(np.float64)
        n += int((s - np.floor(s) == 0.5).sum())
    return n


# ---------------------------------------------------------------- hand-made accumulators (stage 1)
# (rows, cols, theta divisor): numrho = 2 (rows + cols) + 1 at rho 1, numangle = the divisor
HAND_GEOMETRIES = [(1, 1, 4), (3, 4, 6), (3, 4, 45), (20, 20, 180)]
HAND_NAMES = ("plateau_h2", "plateau_h3", "plateau_v2", "plateau_v3", "scattered_ties", "corners", "checker_equal",
              "checker_ramp", "random", "zero")


def hand_params(rows, cols, div):
    par = params(rows, cols, 1.0, math.pi / div)
    assert par["numangle"] == div and par["numrho"] == 2 * (rows + cols) + 1, par
    return par


@functools.lru_cache(maxsize=None)
def hand_accumulators(rows, cols, div):
    """(len(HAND_NAMES), numangle + 2, numrho + 2) int32 with a zero border."""
    par = hand_params(rows, cols, div)
    A, R = par["numangle"], par["numrho"]
    rng = np.random.default_rng(100 * A + R)
    out = []

    def blank():
        return np.zeros((A + 2, R + 2), np.int32)

    def inner(a):
        return a[1:-1, 1:-1]

    n_mid, r_mid = A // 2, R // 2
    for horizontal, length in ((True, 2), (True, 3), (False, 2), (False, 3)):
        a = blank()
        v = inner(a)
        if horizontal:
            v[n_mid, max(0, r_mid - 1):max(0, r_mid - 1) + length] = 9       # only the leftmost passes
            v[0, 0:length] = 4
        else:
            v[max(0, n_mid - 1):max(0, n_mid - 1) + length, r_mid] = 9       # only the uppermost passes
            v[0:length, R - 1] = 4
        out.append(a)
    a = blank()                                              # equal votes, visited in an order that is not the index order
    v = inner(a)
    cells = [(n, r) for n in range(0, A, 2) for r in range((n // 2) % 2, R, 2)]
    for k, (n, r) in enumerate(cells):
        v[n, r] = 5 if k % 3 else 8
    out.append(a)
    a = blank()                                              # the first and last angle and rho
    v = inner(a)
    v[0, 0], v[0, R - 1], v[A - 1, 0], v[A - 1, R - 1] = 3, 4, 4, 6
    out.append(a)
    nn, rr = np.mgrid[0:A, 0:R]
    a = blank()                                              # ceil(A R / 2) peaks, all equal
    inner(a)[(nn + rr) % 2 == 0] = 5
    out.append(a)
    a = blank()                                              # the same cells, votes that grow against the index
    inner(a)[(nn + rr) % 2 == 0] = (1 + (A * R - (nn * R + rr)) // 3)[(nn + rr) % 2 == 0]
    out.append(a)
    a = blank()
    inner(a)[:] = rng.integers(0, 6, size=(A, R))
    out.append(a)
    out.append(blank())
    res = np.stack(out)
    res.setflags(write=False)
    return res


# ---------------------------------------------------------------- warp_image
def warp_image(frame, M, dsize, gray=False):
    """cv2.warpPerspective(frame, M, dsize) per channel (oracle.ocv_np.warp_perspective), then, with gray,
    cv2.cvtColor(., COLOR_BGR2GRAY) in 8 bits: (1868 b + 9617 g + 4899 r + 8192) >> 14."""
    from oracle import ocv_np
    f = np.asarray(frame)
    if f.ndim == 2:
        assert not gray
        return ocv_np.warp_perspective(f, M, dsize)
    ch = [ocv_np.warp_perspective(np.ascontiguousarray(f[:, :, c]), M, dsize).astype(np.int64) for c in range(3)]
    if gray:
        return ((1868 * ch[0] + 9617 * ch[1] + 4899 * ch[2] + 8192) >> 14).astype(np.uint8)
    return np.stack(ch, axis=2).astype(np.uint8)
