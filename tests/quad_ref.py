"""NumPy restatement of find_quad and of calibration.refine, written from the semantics alone.

  grey, otsu, foreground     stages a, b
  choose / choose_brute      stages c, d: the tile's region as (root, area, mask). `choose` labels by neighbour
                             minima with pointer jumping; `choose_brute` asks scipy.ndimage.label (3 x 3 structure)
  corners / corners_brute    stage e: vectorised arg-maxima over the region's pixels in raster order;
                             `corners_brute` walks the sorted pixel list in Python integers
  moments                    stage f, for any doubled corners
  find_quad                  a .. f for one frame -> a dict of the device's outputs
  refine, find_tile          the host's line fits and the two-pass form
  render, rendered, group    the renderer, the rendered accuracy cases and the cases of the GPU tests, by group

Coordinates: pixel (x, y) covers [x - 1/2, x + 1/2] x [y - 1/2, y + 1/2]; the crack between pixels x and x + 1
lies at x + 1/2, doubled: 2 x + 1.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

OK, NO_TILE, DEGENERATE = 0, 1, 2
MAX_COORD2 = 16384


def params(h, w, bright=True, threshold=None, min_area=None, band=(3, 2)):
    return {"rows": h, "cols": w, "bright": bool(bright), "threshold": threshold,
            "min_area": max(16, h * w // 1000) if min_area is None else min_area, "band": tuple(band)}


# ---------------------------------------------------------------- a, b
def grey(frame):
    f = np.asarray(frame)
    if f.ndim == 2:
        return f.astype(np.uint8)
    b, g, r = (f[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def otsu_values(g):
    """v(t) for t = 0..255 (None where a side is empty), float64, in the pinned operation order."""
    hist = np.bincount(g.ravel(), minlength=256).astype(np.int64)
    out = []
    for t in range(256):
        n0, n1 = int(hist[:t + 1].sum()), int(hist[t + 1:].sum())
        if n0 == 0 or n1 == 0:
            out.append(None)
            continue
        s0 = int((hist[:t + 1] * np.arange(t + 1)).sum())
        s1 = int((hist[t + 1:] * np.arange(t + 1, 256)).sum())
        d = np.float64(s0) / np.float64(n0) - np.float64(s1) / np.float64(n1)
        out.append(np.float64(n0) * np.float64(n1) * d * d)
    return out


def otsu(g):
    """-> the first t with the largest v, or -1 for a frame of one grey level."""
    best, bv = -1, None
    for t, v in enumerate(otsu_values(g)):
        if v is not None and (bv is None or v > bv):
            best, bv = t, v
    return best


def otsu_margin(g):
    """(best v - second best v) / best v over the distinct splits: the tests ask their Otsu inputs for more than 1e-9.
    A t whose bin is empty splits the pixels as t - 1 does: the same four integers go through the same operations,
    so its v is the same bits on any machine and the first such t wins; only distinct splits can differ by rounding."""
    hist = np.bincount(g.ravel(), minlength=256)
    vs = sorted((v for t, v in enumerate(otsu_values(g)) if v is not None and hist[t] > 0), reverse=True)
    if len(vs) < 2 or vs[0] == 0:
        return np.inf
    return float((vs[0] - vs[1]) / vs[0])


def foreground(g, t, bright):
    if t < 0:
        return np.zeros(g.shape, bool)
    return g > t if bright else g <= t


# ---------------------------------------------------------------- c, d
def _pick(cands):
    """cands: (area, root) pairs -> the largest area, the lowest root on a tie, or None."""
    return min(cands, key=lambda c: (-c[0], c[1])) if cands else None


def choose(fg, min_area):
    h, w = fg.shape
    n = h * w
    lab = np.where(fg, np.arange(n).reshape(h, w), n).astype(np.int64)
    while True:
        prev = lab.copy()
        pad = np.full((h + 2, w + 2), n, np.int64)
        pad[1:-1, 1:-1] = lab
        m = lab
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                m = np.minimum(m, pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
        lab = np.where(fg, m, n)
        flat = np.append(lab.ravel(), n)
        for _ in range(4):
            flat = flat[flat]
        lab = flat[:n].reshape(h, w)
        if np.array_equal(lab, prev):
            break
    roots = lab[fg]
    area = np.bincount(roots, minlength=n + 1)
    edge = np.zeros((h, w), bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    touching = set(np.unique(lab[fg & edge]).tolist())
    best = _pick([(int(area[r]), int(r)) for r in np.unique(roots) if int(r) not in touching and area[r] >= min_area])
    if best is None:
        return None
    return best[1], best[0], lab == best[1]


def choose_brute(fg, min_area):
    from scipy import ndimage
    lab, k = ndimage.label(fg, structure=np.ones((3, 3), int))
    cands = {}
    for i in range(1, k + 1):
        m = lab == i
        if m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any() or int(m.sum()) < min_area:
            continue
        cands[(int(m.sum()), int(np.flatnonzero(m)[0]))] = m
    best = _pick(list(cands))
    if best is None:
        return None
    return best[1], best[0], cands[best]


# ---------------------------------------------------------------- e
def _order(c, c3, edge):
    out = []
    for i in range(3):
        out.append(c[i])
        if i == edge:
            out.append(c3)
    return out


def corners(mask, root):
    """-> (status, [(x, y)] * 4 in cyclic order), zeros unless OK."""
    w = mask.shape[1]
    ys, xs = np.nonzero(mask)                       # raster order: argmax's first maximum is the lowest index
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    zero = [(0, 0)] * 4

    def far(px, py):
        i = int(np.argmax((xs - px) ** 2 + (ys - py) ** 2))
        return int(xs[i]), int(ys[i])

    c0 = far(root % w, root // w)
    c1 = far(*c0)

    def cross(a, b, px, py):
        return (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])

    i = int(np.argmax(np.abs(cross(c0, c1, xs, ys))))
    c2 = (int(xs[i]), int(ys[i]))
    s = cross(c0, c1, *c2)
    if s == 0:
        return DEGENERATE, zero
    tri = [c0, c1, c2]
    out = np.stack([cross(tri[e], tri[(e + 1) % 3], xs, ys) * (-1 if s > 0 else 1) for e in range(3)])
    val = out.max(axis=0)
    i = int(np.argmax(val))
    if val[i] <= 0:
        return DEGENERATE, zero
    c3 = (int(xs[i]), int(ys[i]))
    edge = int(np.argmax(out[:, i]))
    quad = _order(tri, c3, edge)
    if len(set(quad)) < 4:
        return DEGENERATE, zero
    return OK, quad


def corners_brute(mask, root):
    w = mask.shape[1]
    pix = sorted(int(p) for p in np.flatnonzero(mask))
    pts = [(p % w, p // w) for p in pix]
    zero = [(0, 0)] * 4

    def first_max(vals):
        best = 0
        for i, v in enumerate(vals):
            if v > vals[best]:
                best = i
        return best

    def cross(a, b, p):
        return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])

    r = (root % w, root // w)
    c0 = pts[first_max([(p[0] - r[0]) ** 2 + (p[1] - r[1]) ** 2 for p in pts])]
    c1 = pts[first_max([(p[0] - c0[0]) ** 2 + (p[1] - c0[1]) ** 2 for p in pts])]
    c2 = pts[first_max([abs(cross(c0, c1, p)) for p in pts])]
    s = cross(c0, c1, c2)
    if s == 0:
        return DEGENERATE, zero
    tri = [c0, c1, c2]
    sign = -1 if s > 0 else 1

    def outward(p):
        return [sign * cross(tri[e], tri[(e + 1) % 3], p) for e in range(3)]

    vals = [max(outward(p)) for p in pts]
    i = first_max(vals)
    if vals[i] <= 0:
        return DEGENERATE, zero
    c3 = pts[i]
    o = outward(c3)
    quad = _order(tri, c3, o.index(max(o)))
    if len(set(quad)) < 4:
        return DEGENERATE, zero
    return OK, quad


# ---------------------------------------------------------------- f
def cracks(mask):
    """The doubled crack points of a region, (N, 2) int64 (X, Y)."""
    h, w = mask.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = mask
    pts = []
    for dx, dy in ((0, -1), (-1, 0), (1, 0), (0, 1)):
        nb = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        ys, xs = np.nonzero(mask & ~nb)
        pts.append(np.stack([2 * xs + dx, 2 * ys + dy], axis=1))
    return np.concatenate(pts).astype(np.int64)


def moments(mask, corners2, band):
    """(4, 6) int64: n, sum X, sum Y, sum XX, sum XY, sum YY per side of the doubled corners."""
    out = np.zeros((4, 6), np.int64)
    if mask is None:
        return out
    pts = cracks(mask)
    X, Y = pts[:, 0], pts[:, 1]
    c = [(int(v[0]), int(v[1])) for v in np.asarray(corners2).reshape(4, 2)]
    for i in range(4):
        a, b = c[i], c[(i + 1) % 4]
        if a == b or max(abs(v) for v in a + b) > MAX_COORD2:
            continue
        ux, uy = b[0] - a[0], b[1] - a[1]
        vx, vy = X - a[0], Y - a[1]
        len2 = ux * ux + uy * uy
        cr = ux * vy - uy * vx
        dt = 8 * (ux * vx + uy * vy)
        take = (cr * cr <= (2 * band) ** 2 * len2) & (len2 <= dt) & (dt <= 7 * len2)
        x, y = X[take], Y[take]
        out[i] = [take.sum(), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()]
    return out


def find_quad(frame, p, brute=False):
    """One frame -> {"status", "threshold", "area", "root", "corners" (4, 2) int32, "moments" (4, 6) int64, "mask"}."""
    g = grey(frame)
    fixed = p["threshold"] is not None and 0 <= p["threshold"] <= 254
    t = int(p["threshold"]) if fixed else otsu(g)
    res = {"status": NO_TILE, "threshold": t, "area": 0, "root": -1, "corners": np.zeros((4, 2), np.int32),
           "moments": np.zeros((4, 6), np.int64), "mask": None}
    reg = (choose_brute if brute else choose)(foreground(g, t, p["bright"]), p["min_area"])
    if reg is None:
        return res
    res["root"], res["area"], res["mask"] = reg
    res["status"], quad = (corners_brute if brute else corners)(reg[2], reg[0])
    if res["status"] == OK:
        res["corners"] = np.array(quad, np.int32)
        res["moments"] = moments(reg[2], 2 * res["corners"], p["band"][0])
    return res


# ---------------------------------------------------------------- the host's part
def fit_line(m):
    """(point, unit direction) of the total-least-squares line through the sums m, or None for fewer than 2 points.
    The scatter is formed exactly (rationals), its principal axis by a symmetric eigen-decomposition."""
    n, sx, sy, sxx, sxy, syy = (int(v) for v in m)
    if n < 2:
        return None
    mx, my = Fraction(sx, n), Fraction(sy, n)
    S = np.array([[float(sxx - n * mx * mx), float(sxy - n * mx * my)],
                  [float(sxy - n * mx * my), float(syy - n * my * my)]])
    wv, vec = np.linalg.eigh(S)
    return np.array([float(mx), float(my)]), vec[:, 1]


def refine(corners2, mom, min_points=8):
    """One frame: doubled corners (4, 2) and moments (4, 6) -> (status, corners (4, 2) float64 in pixels)."""
    coarse = np.asarray(corners2, np.float64).reshape(4, 2) / 2
    lines = []
    for i in range(4):
        if int(mom[i][0]) < min_points:
            return DEGENERATE, coarse
        lines.append(fit_line(mom[i]))
    out = np.zeros((4, 2))
    for i in range(4):
        (p, u), (q, v) = lines[i - 1], lines[i]
        if abs(u[0] * v[1] - u[1] * v[0]) < 1e-6:
            return DEGENERATE, coarse
        # p + s u = q + r v
        s, _ = np.linalg.solve(np.array([[u[0], -v[0]], [u[1], -v[1]]]), q - p)
        out[i] = (p + s * u) / 2
    return OK, out


def find_tile(frame, p, min_points=8):
    """The two-pass host form for one frame -> find_quad's dict with "refined" (4, 2) float64, "corners2" (the doubled
    integers of the second pass), "moments2", "counts" (the second pass's points per side) and "status0" added; status
    updated."""
    r = find_quad(frame, p)
    r["status0"] = r["status"]                      # the device's status: the passes below can only lower an OK
    r["refined"] = r["corners"].astype(np.float64)
    r["corners2"] = np.zeros((4, 2), np.int32)
    r["moments2"] = np.zeros((4, 6), np.int64)
    r["counts"] = np.zeros(4, np.int64)
    if r["status"] != OK:
        return r
    st, c = refine(2 * r["corners"], r["moments"], min_points)
    if st == OK:
        r["corners2"] = np.rint(2 * c).astype(np.int32)
        r["moments2"] = moments(r["mask"], r["corners2"], p["band"][1])
        r["counts"] = r["moments2"][:, 0].copy()
        st, c = refine(r["corners2"], r["moments2"], min_points)
    r["status"], r["refined"] = st, c
    return r


# ---------------------------------------------------------------- renderer and shared cases
def render(h, w, quad, bg=60, fg=200, sigma=4.0, seed=0, blobs=(), bgr=False, holes=()):
    """A convex quad (float corners, either orientation) 4 x 4 supersampled onto an h x w frame of level bg, foreground
    level fg, blobs / holes: (x0, y0, x1, y1) pixel rectangles (half-open) set to fg / bg, then seeded Gaussian noise
    (per channel for BGR), rounded and clipped."""
    q = np.asarray(quad, np.float64).reshape(4, 2)
    sub = (np.arange(4) + 0.5) / 4 - 0.5
    X = (np.arange(w)[:, None] + sub[None, :]).reshape(-1)
    Y = (np.arange(h)[:, None] + sub[None, :]).reshape(-1)
    gx, gy = np.meshgrid(X, Y)
    area2 = sum(q[i][0] * q[(i + 1) % 4][1] - q[(i + 1) % 4][0] * q[i][1] for i in range(4))
    inside = np.ones(gx.shape, bool)
    for i in range(4):
        a, b = q[i], q[(i + 1) % 4]
        c = (b[0] - a[0]) * (gy - a[1]) - (b[1] - a[1]) * (gx - a[0])
        inside &= (c >= 0) if area2 > 0 else (c <= 0)
    cov = inside.reshape(h, 4, w, 4).mean(axis=(1, 3))
    img = bg + (fg - bg) * cov
    for x0, y0, x1, y1 in blobs:
        img[y0:y1, x0:x1] = fg
    for x0, y0, x1, y1 in holes:
        img[y0:y1, x0:x1] = bg
    rng = np.random.default_rng(seed)
    shape = (h, w, 3) if bgr else (h, w)
    noisy = (img[..., None] if bgr else img) + rng.normal(0.0, sigma, shape) if sigma > 0 else np.broadcast_to(img[..., None] if bgr else img, shape)
    return np.clip(np.rint(noisy), 0, 255).astype(np.uint8)


QUADS = {
    "wide": ((120, 160), [(52.3, 70.6), (108.9, 72.2), (131.4, 104.7), (30.2, 101.3)]),
    "tilted": ((120, 160), [(60.3, 30.6), (100.9, 50.2), (85.4, 98.7), (40.2, 80.3)]),
    "small": ((48, 64), [(20.3, 18.6), (44.9, 19.2), (54.4, 38.7), (10.2, 37.3)]),
    "camera": ((480, 640), [(250.3, 300.6), (410.9, 305.2), (480.4, 420.7), (170.2, 410.3)]),
    "foreshortened": ((480, 640), [(300.3, 200.6), (340.9, 201.2), (520.4, 440.7), (120.2, 430.3)]),
}
SEEDS = (0, 1, 2)


def standard_blobs(h, w):
    """One bright blob in the top-left corner (off the border, smaller than any tile) and one touching the bottom border."""
    return ((2, 2, 2 + w // 12, 2 + h // 12), (int(0.85 * w), h - h // 12, int(0.97 * w), h))


@functools.lru_cache(maxsize=None)
def rendered(name, seed, bgr=False):
    (h, w), quad = QUADS[name]
    f = render(h, w, quad, 60, 200, 4.0, seed, standard_blobs(h, w), bgr)
    f.setflags(write=False)
    return f


def match_error(found, truth):
    """Each found corner's nearest true corner -> (the true indices, the largest distance)."""
    found, truth = np.asarray(found, np.float64), np.asarray(truth, np.float64)
    d = np.linalg.norm(found[:, None, :] - truth[None, :, :], axis=2)
    return d.argmin(axis=1).tolist(), float(d.min(axis=1).max())


# ---------------------------------------------------------------- the cases of the GPU tests
SHAPES = [(48, 64), (50, 67), (99, 130), (120, 160)]
BIG = (480, 640)
UNIT = {name: [(x / w, y / h) for x, y in quad] for name, ((h, w), quad) in QUADS.items()}


def scaled(name, h, w):
    return [(x * w, y * h) for x, y in UNIT[name]]


def from_mask(mask, bg=60, fg=200, sigma=4.0, seed=0, bgr=False):
    """A frame with level fg where mask is set and bg elsewhere, plus seeded Gaussian noise (per channel for BGR)."""
    img = np.where(mask, float(fg), float(bg))
    rng = np.random.default_rng(seed)
    if bgr:
        img = np.repeat(img[..., None], 3, axis=2)
    if sigma > 0:
        img = img + rng.normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def masks(h, w):
    """Hand-made regions, by name."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {}
    rect = (yy >= h // 4) & (yy < 3 * h // 4) & (xx >= w // 5) & (xx < 4 * w // 5)
    out["rect"] = rect
    r = min(h, w) // 3
    out["diamond"] = np.abs(xx - w // 2) + np.abs(yy - h // 2) <= r
    holes = rect.copy()
    holes[h // 2, w // 2] = False
    holes[h // 4 + 3:h // 4 + 3 + h // 8, w // 5 + 4:w // 5 + 4 + w // 8] = False
    out["holes"] = holes
    a, b = h // 5, w // 5
    equal = np.zeros((h, w), bool)
    equal[2:2 + a, w - 3 - b:w - 3] = True                     # the upper right one holds the lower root
    equal[h - 3 - a:h - 3, 3:3 + b] = True
    out["equal"] = equal
    border = np.zeros((h, w), bool)
    border[1:h - 1, 0:w // 2] = True                           # larger, but it touches the left border
    border[h // 3:2 * h // 3, w // 2 + 4:w - 4] = True
    out["border"] = border
    none = np.zeros((h, w), bool)
    none[h - h // 4:h, 0:w] = True
    none[4:7, 5:8] = True                                      # 9 pixels: below any min_area
    out["none"] = none
    k = min(h, w) // 3
    out["triangle"] = (yy >= 5) & (yy <= 5 + k) & (xx >= 7) & (xx - 7 <= yy - 5)
    return out


GROUPS = ("grey", "bgr", "dark", "fixed")


@functools.lru_cache(maxsize=None)
def group(h, w, which):
    """-> (names, frames (B, h, w[, 3]) uint8, params, [find_tile(frame) for every frame]); cached, do not write."""
    m = masks(h, w)
    blobs = standard_blobs(h, w)
    if which == "grey":
        p = params(h, w)
        fr = {"wide": render(h, w, scaled("wide", h, w), 60, 200, 4.0, 0, blobs),
              "foreshortened": render(h, w, scaled("foreshortened", h, w), 60, 200, 4.0, 2, blobs),
              "uniform": np.full((h, w), 77, np.uint8)}
        for i, name in enumerate(("rect", "diamond", "holes", "equal", "border", "none", "triangle")):
            fr[name] = from_mask(m[name], seed=10 + i)
        for name, (shape, _) in QUADS.items():                  # the accuracy test's own frames of this size
            if shape == (h, w):
                fr["rendered " + name] = rendered(name, 0)
    elif which == "bgr":
        p = params(h, w)
        fr = {"tilted": render(h, w, scaled("tilted", h, w), 60, 200, 4.0, 1, blobs, bgr=True),
              "rect": from_mask(m["rect"], seed=20, bgr=True),
              "uniform": np.full((h, w, 3), 200, np.uint8),
              "coloured": from_mask(m["diamond"], seed=21, bgr=True) // np.array([1, 2, 3], np.uint8)}
    elif which == "dark":
        p = params(h, w, bright=False)
        fr = {"wide": render(h, w, scaled("wide", h, w), 200, 60, 4.0, 3),
              "rect": from_mask(m["rect"], 200, 60, seed=30), "triangle": from_mask(m["triangle"], 200, 60, seed=31)}
    else:
        p = params(h, w, threshold=150, band=(4, 1))
        fr = {"wide": render(h, w, scaled("wide", h, w), 60, 200, 4.0, 4, blobs),
              "rect": from_mask(m["rect"], sigma=0.0), "diamond": from_mask(m["diamond"], sigma=0.0)}
    names = list(fr)
    frames = np.stack([fr[n] for n in names])
    frames.setflags(write=False)
    return names, frames, p, [find_tile(f, p) for f in frames]


@functools.lru_cache(maxsize=None)
def big_group():
    """The one camera-sized case: the foreshortened trapezoid (BGR) and the camera quad's grey values as BGR."""
    h, w = BIG
    p = params(h, w)
    frames = np.stack([rendered("foreshortened", 0, True), np.repeat(rendered("camera", 1)[..., None], 3, axis=2)])
    frames.setflags(write=False)
    return ["foreshortened", "camera"], frames, p, [find_tile(f, p) for f in frames]


def stacked(refs, key):
    return np.stack([np.asarray(r[key]) for r in refs])
