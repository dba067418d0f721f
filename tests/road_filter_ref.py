"""Helper of the road-filter tests (not collected): two restatements of contour_noise_removal's pinned
semantics (image_processing_utils.py:4-44), written independently of each other with NumPy
and scipy.ndimage, and the case builders the tests share.

`brute` treats every contour separately, as the reference's loop does: per region it builds the filled
contour as a mask (flood from outside the region), counts its band pixels, and the output is the even-odd
fill of all kept contours with their outlines drawn. `tree` follows the nesting rule: one label image, the
parent of a region is the region above its raster-first pixel, counts are summed up the tree.
Neither uses OpenCV: the semantics are pinned to no OpenCV run."""
from __future__ import annotations

import functools

import numpy as np
from scipy import ndimage

S8 = np.ones((3, 3), bool)
S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)

SHAPES = [(50, 64), (53, 50), (50, 67), (99, 130), (100, 120), (150, 200), (256, 512), (480, 640)]


def host_params(h, w):
    """(k, y_top, min_count) in the reference's own float expressions (image_processing_utils.py:7-8, 22, 27, 38)."""
    min_length = min(h, w)
    k = int(min_length / 50)
    y_top = int(h * (1 - 0.1))
    mask_area = (w - 0) * (h - y_top)
    thresh = mask_area * 0.4
    n = 0
    while not n > thresh:      # the smallest integer count that passes `count > thresh`
        n += 1
    return k, y_top, n


# ------------------------------------------------------------------ closing, two ways
def close_shifts(seg, k):
    """OR then AND over the k x k offsets -a .. k-1-a (a = k // 2), taps outside the image ignored."""
    fg = np.asarray(seg) != 0
    h, w = fg.shape
    a = k // 2

    def sweep(src, neutral, op):
        acc = np.full((h, w), neutral, bool)
        pad = np.full((h + 2 * k, w + 2 * k), neutral, bool)
        pad[k:k + h, k:k + w] = src
        for i in range(k):
            for j in range(k):
                acc = op(acc, pad[k + i - a:k + i - a + h, k + j - a:k + j - a + w])
        return acc

    d = sweep(fg, False, np.logical_or)
    return sweep(d, True, np.logical_and)


def close_filters(seg, k):
    """The same with scipy's rank filters: footprint k x k whose centre sits at index a, constant borders that
    are neutral for each pass."""
    fg = (np.asarray(seg) != 0).astype(np.uint8)
    a = k // 2
    # scipy centres a size-k window at index k // 2 and origin shifts it: window [x - k//2 - o, ...]; ours is
    # [x - a, x - a + k), so o = 0
    d = ndimage.maximum_filter(fg, size=(k, k), mode="constant", cval=0, origin=0) if k > 1 else fg
    c = ndimage.minimum_filter(d, size=(k, k), mode="constant", cval=1, origin=0) if k > 1 else d
    assert a == k // 2
    return c.astype(bool)


# ------------------------------------------------------------------ brute: every contour on its own
def _enclosed(region, structure):
    """region plus everything it encloses: the complement of what is reachable from outside the (padded)
    image through non-region pixels under `structure`."""
    rest = np.pad(~region, 1, constant_values=True)
    lab, _ = ndimage.label(rest, structure=structure)
    return ~(lab == lab[0, 0])[1:-1, 1:-1]


def brute(seg, params=None):
    seg = np.asarray(seg)
    h, w = seg.shape
    k, y_top, min_count = params if params is not None else host_params(h, w)
    c = close_shifts(seg, k)
    band = np.zeros((h, w), bool)
    band[y_top:] = True
    parity = np.zeros((h, w), np.int32)
    outline = np.zeros((h, w), bool)

    def crop(sl):
        return (slice(max(sl[0].start - 1, 0), min(sl[0].stop + 1, h)), slice(max(sl[1].start - 1, 0), min(sl[1].stop + 1, w)))

    fl, nf = ndimage.label(c, structure=S8)
    for i, sl in enumerate(ndimage.find_objects(fl)):
        sl = crop(sl)
        comp = fl[sl] == i + 1
        # the filled outer contour: the component and all it encloses (4-connected flood of the rest from outside)
        filled = _enclosed(comp, S4)
        if np.count_nonzero(filled & band[sl]) >= min_count:
            parity[sl] += filled
            outline[sl] |= comp & ~ndimage.binary_erosion(comp, structure=S8, border_value=0)
    bl, nb = ndimage.label(~c, structure=S4)
    edge = np.zeros((h, w), bool)
    edge[0] = edge[-1] = True
    edge[:, 0] = edge[:, -1] = True
    outside = set(np.unique(bl[edge & ~c]).tolist())
    for i, sl in enumerate(ndimage.find_objects(bl)):
        if i + 1 in outside:
            continue                    # no hole: findContours gives it no contour
        sl = crop(sl)
        hole = bl[sl] == i + 1
        # the filled hole contour: it runs over the road pixels that bound the hole (4-neighbours of it that
        # the hole does not enclose), so the polygon covers them, the hole and all the hole encloses
        inner = _enclosed(hole, S8)
        ringpx = ndimage.binary_dilation(hole, structure=S4) & ~inner
        poly = inner | ringpx
        if np.count_nonzero(poly & band[sl]) >= min_count:
            parity[sl] += poly
            outline[sl] |= ringpx
    return (((parity & 1) == 1) | outline).astype(np.uint8)


# ------------------------------------------------------------------ tree: the nesting rule
def tree(seg, params=None):
    seg = np.asarray(seg)
    h, w = seg.shape
    k, y_top, min_count = params if params is not None else host_params(h, w)
    c = close_filters(seg, k)
    fl, nf = ndimage.label(c, structure=S8)
    bl, nb = ndimage.label(~c, structure=S4)
    node = np.where(c, fl - 1, nf + bl - 1).astype(np.int64)      # one id per region, components first
    n = nf + nb
    flat = node.ravel()
    first = np.full(n, h * w, np.int64)
    np.minimum.at(first, flat, np.arange(h * w))
    is_fg = np.arange(n) < nf
    outside = np.zeros(n, bool)
    for border in (node[0], node[-1], node[:, 0], node[:, -1]):
        outside[border] = True
    outside &= ~is_fg
    parent = np.full(n, -1, np.int64)
    for v in range(n):
        if outside[v] or first[v] < w:
            continue
        p = flat[first[v] - w]
        if not outside[p]:
            parent[v] = p
    band = np.bincount(flat[y_top * w:], minlength=n).astype(np.int64)
    # ring(H): band pixels of H's parent with a 4-neighbour in H, once per (pixel, H)
    ring = np.zeros(n, np.int64)
    pairs = set()
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ys, xs = np.nonzero(c[y_top:])
        ys = ys + y_top
        ny, nx = ys + dy, xs + dx
        ok = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
        ys, xs, ny, nx = ys[ok], xs[ok], ny[ok], nx[ok]
        bg = ~c[ny, nx]
        for y, x, hh in zip(ys[bg], xs[bg], node[ny[bg], nx[bg]]):
            if not outside[hh] and parent[hh] == node[y, x]:
                pairs.add((int(y) * w + int(x), int(hh)))
    for _, hh in pairs:
        ring[hh] += 1
    sub = band.copy()
    for v in np.argsort(-first):            # a parent's first pixel precedes its children's
        if parent[v] >= 0:
            sub[parent[v]] += sub[v]
    qual = np.where(is_fg, sub >= min_count, (sub + ring >= min_count) & ~outside)
    res = np.zeros(n, np.uint8)
    for v in np.argsort(first):             # top-down: a node's parent is resolved before it
        if qual[v]:
            res[v] = 1 if is_fg[v] else 0
        elif parent[v] >= 0:
            res[v] = res[parent[v]]
    return res[node].astype(np.uint8)


# ------------------------------------------------------------------ case builders
def _band_block(h, w, target, x0=2):
    """A block in the band rows with exactly `target` band pixels: full columns from x0, the last pixels missing
    from the right end of its top row (a staircase, which the closing leaves alone)."""
    k, y_top, _ = host_params(h, w)
    r = h - y_top
    bw = -(-target // r)
    x0 += 2 * k                    # (a gap narrower than k to the image border would be closed)
    top = y_top - (k % 2 == 0)     # (an even k shifts the closed map one pixel down and right)
    m = np.zeros((h, w), np.uint8)
    m[top:, x0:x0 + bw] = 1
    e = bw * r - target
    if e:
        m[top, x0 + bw - e:x0 + bw] = 0
    assert int(close_shifts(m, k)[y_top:].sum()) == target and x0 + bw + 1 < w
    return m


def _ring_hole(h, w, target):
    """A wide block with a hole inside the band whose own pixels plus ring count exactly `target` band pixels."""
    k, y_top, mc = host_params(h, w)
    r = h - y_top
    m = np.zeros((h, w), np.uint8)
    m[y_top - 2:, 1:w - 1] = 1
    hw = -(-mc // r)               # hw * r + 2 (r - 2) band pixels to start with: fewer than 3 r above mc
    x0 = 4
    hole = np.zeros((h, w), bool)
    hole[y_top + 1:h - 1, x0:x0 + hw] = True
    band = np.zeros((h, w), bool)
    band[y_top:] = True
    for step in range(hw - 2 * k - 2):
        total = np.count_nonzero((hole | ndimage.binary_dilation(hole, structure=S4)) & band)
        if total == target:
            m[hole] = 0
            return m
        assert total > target
        hole[y_top + 1, x0 + step] = False
    raise AssertionError("no hole with that count")


def _spiral(h, w, pitch):
    """A one-pixel road line winding inwards clockwise, `pitch` between turns: one long component."""
    m = np.zeros((h, w), np.uint8)
    o = pitch - 1                  # off the image border by more than the closing fills
    y, x, dy, dx = o, o, 0, 1
    top, bot, left, right = o, h - 1 - o, o, w - 1 - o
    while right - left >= pitch and bot - top >= pitch:
        if dx == 1:
            m[y, x:right + 1] = 1
            x, top = right, top + pitch
        elif dy == 1:
            m[y:bot + 1, x] = 1
            y, right = bot, right - pitch
        elif dx == -1:
            m[y, left:x + 1] = 1
            x, bot = left, bot - pitch
        else:
            m[top:y + 1, x] = 1
            y, left = top, left + pitch
        dy, dx = dx, -dy
    return m


def _serpentine(h, w, pitch):
    """Road walls every `pitch` rows, each open at alternate ends beside a side column: the background is one
    long snake of corridors, the road two interleaved combs."""
    m = np.zeros((h, w), np.uint8)
    t = 1 + (pitch % 2)            # pitch = k + 1: an even k shifts the closed map right, two columns leave one
    m[:, 0] = 1
    m[:, w - t:] = 1
    gap = pitch - 1
    for n, y in enumerate(range(pitch, h, pitch)):
        m[y] = 1
        if n % 2:
            m[y, 1:1 + gap] = 0
        else:
            m[y, w - t - gap:w - t] = 0
    return m


def _scene(h, w, seed):
    """A trapezoid road to the bottom edge with holes in it and false islands beside and above it."""
    rng = np.random.default_rng(seed)
    k, y_top, _ = host_params(h, w)
    m = np.zeros((h, w), np.uint8)
    top = h // 3
    for y in range(top, h):
        f = (y - top) / max(1, h - 1 - top)
        half = int(w * (0.08 + 0.38 * f))
        cx = w // 2 + int(rng.integers(-1, 2))
        m[y, max(0, cx - half):min(w, cx + half)] = 1
    for _ in range(12):
        s = int(rng.integers(1, 3 * k + 4))
        y, x = int(rng.integers(0, h - s)), int(rng.integers(0, w - s))
        m[y:y + s, x:x + s] = 1 - m[y + s // 2, x + s // 2]
    salt = rng.random((h, w)) < 0.01
    m[salt] ^= 1
    return m


def noise(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def shape_cases(h, w):
    """name -> (h, w) uint8 map: the structured cases at one shape."""
    k, y_top, mc = host_params(h, w)
    r = h - y_top
    g = k + 2                      # a gap or a wall this wide survives the closing
    cases = {}
    cases["zeros"] = np.zeros((h, w), np.uint8)
    cases["ones"] = np.ones((h, w), np.uint8)
    bw = -(-mc // r)
    two = np.zeros((h, w), np.uint8)
    two[y_top - 3:, :bw + 2] = 1      # (two columns to spare: an even k shifts the closed map by one)
    two[y_top - 3:, w - bw - 2:] = 1
    assert w - 2 * bw - 4 > k + 1
    cases["two_blocks"] = two
    cases["block_min_count_minus_1"] = _band_block(h, w, mc - 1)
    cases["block_min_count"] = _band_block(h, w, mc)
    sm = np.zeros((h, w), np.uint8)
    sm[h // 2:, 2:w - 2] = 1
    sm[h // 2 + g:h // 2 + 2 * g, w // 2:w // 2 + g] = 0
    cases["small_hole"] = sm
    cases["ring_hole_open"] = _ring_hole(h, w, mc)
    cases["ring_hole_filled"] = _ring_hole(h, w, mc - 1)
    # a hole wide enough to qualify, with an island; a small hole with an island
    isl = np.zeros((h, w), np.uint8)
    isl[h // 4:, 1:w - 1] = 1
    t = 1 + (k % 2 == 0)           # (an even k shifts the closed map one pixel down: two rows leave one)
    isl[h // 4 + g:h - t, 1 + g:w - 1 - g] = 0
    isl[h - t - 2 * g:h - t - g, w // 2:w // 2 + g] = 1
    cases["island_in_open_hole"] = isl
    isl2 = np.zeros((h, w), np.uint8)
    isl2[h // 4:, 1:w - 1] = 1
    y0, x0 = h // 4 + g, w // 2 - 2 * g
    isl2[y0:y0 + 3 * g, x0:x0 + 3 * g] = 0
    isl2[y0 + g:y0 + 2 * g, x0 + g:x0 + 2 * g] = 1
    cases["island_in_filled_hole"] = isl2
    # five levels: road, hole, road, hole, road, insets of g, the outer hole spanning the band
    nest = np.zeros((h, w), np.uint8)
    t, b, l, rr = h // 8, h, 1, w - 1
    for lev in range(5):
        nest[t:b, l:rr] = 1 - (lev & 1)
        t, b, l, rr = t + g, b - (g if lev else 1), l + g, rr - g
    assert b - t >= 1 and rr - l >= 1
    cases["nest5"] = nest
    nest2 = np.zeros((h, w), np.uint8)
    t, b, l, rr = h // 2 - 5 * g, h // 2 + 5 * g, w // 2 - 5 * g, w // 2 + 5 * g
    nest2[h // 2:, 1:w - 1] = 1
    for lev in range(1, 6):
        nest2[max(t, 0):b, l:rr] = 1 - (lev & 1)
        t, b, l, rr = t + g, b - g, l + g, rr - g
    cases["nest5_small"] = nest2
    bd = np.zeros((h, w), np.uint8)
    bd[0:g, w // 3:2 * w // 3] = 1
    bd[h // 3:h // 2, 0:g] = 1
    bd[h // 3:h // 2, w - g:] = 1
    bd[y_top - 2:, 0:w] = 1
    cases["borders"] = bd
    fr = np.zeros((h, w), np.uint8)
    fr[:g] = fr[-g:] = 1
    fr[:, :g] = fr[:, -g:] = 1
    cases["frame"] = fr
    co = np.ones((h, w), np.uint8)
    co[h - 1, w - 1] = 0
    co[0, 0] = 0
    cases["corner_pixels"] = co
    foot = np.ones((h, w), np.uint8)
    foot[h // 2:h // 2 + 2 * g, w // 2:w // 2 + 2 * g] = 0       # an inner room ...
    foot[h // 2:, w // 2:w // 2 + k] = 0                          # ... with a k-wide foot on the bottom row
    cases["foot_to_border"] = foot
    dp = np.zeros((h, w), np.uint8)
    dp[h // 3:h, 0:w // 2] = 1
    dp[h // 3 + 1:h // 3 + 1 + 2 * g, w // 2 - 1 - 2 * g:w // 2 - 1] = 0   # a pocket one pixel inside the block's corner ...
    dp[h // 3, w // 2 - 1] = 0                                             # ... and the corner pixel itself: diagonal only
    cases["diagonal_pocket"] = dp
    db = np.zeros((h, w), np.uint8)
    db[y_top - 1:, 0:bw + 2] = 1
    db[y_top - 1 - 2 * g:y_top - 1, bw + 2:bw + 2 + 2 * g] = 1
    cases["diagonal_blobs"] = db
    cases["serpentine"] = _serpentine(h, w, k + 1)
    cases["spiral"] = _spiral(h, w, k + 2)
    cases["scene"] = _scene(h, w, 7)
    sc = _scene(h, w, 11).astype(np.int64) * np.random.default_rng(3).integers(1, 256, (h, w))
    cases["values_0_255"] = sc.astype(np.uint8)
    return cases


def joined_blobs(h, w, gap):
    """A block in the band with a blob `gap` pixels left of it and one `gap` pixels above it."""
    k, y_top, mc = host_params(h, w)
    m = np.zeros((h, w), np.uint8)
    x0 = w // 3
    m[y_top - 4:, x0:w - 2] = 1
    m[y_top - 4:y_top + 2, x0 - gap - 6:x0 - gap] = 1
    m[y_top - 4 - gap - 6:y_top - 4 - gap, x0 + 10:x0 + 20] = 1
    return m


CORNERS = [(16, 64), (32, 64), (48, 64)]       # (y, x) of the first pixel of a labelling tile (16 x 64 tiles)
CORNER_SHAPES = ((50, 67), (99, 130))          # k = 1: the closing is the identity, one-pixel lines survive it


def corner_diagonal_parts(ne):
    """Per corner of CORNERS: (the staircase's pixel at the corner, the 2 x 2 blob above the staircase as slices).
    ne False: the staircase runs down to the right, its only link across the corner is (y - 1, x - 1) -> (y, x);
    ne True: down to the left, the link is (y - 1, x) -> (y, x - 1)."""
    parts = []
    for cy, cx in CORNERS:
        at = (cy, cx - 1) if ne else (cy, cx)
        xe = cx + 2 if ne else cx - 3          # the column of the staircase's top end, three rows up
        parts.append((at, (slice(cy - 5, cy - 3), slice(xe - 1, xe + 1))))
    return parts


def corner_diagonals(h, w, ne):
    """One-pixel diagonal staircases of five pixels across the tile corners CORNERS, each from a blob above it
    down to a trunk column that a connector row joins to a band block large enough to be kept: a blob is in the
    output only through the diagonal link across its corner."""
    k, y_top, mc = host_params(h, w)
    assert k == 1 and h >= 50 and w >= 67
    m = np.zeros((h, w), np.uint8)
    bw = -(-mc // (h - y_top)) + 2
    assert 20 < bw < 56
    m[y_top:, :bw] = 1                         # the band block
    m[40:y_top, 20] = 1                        # up from it ...
    trunk = 61 if ne else 66
    m[40, 20:trunk + 1] = 1                    # ... along the connector row, between the second and third staircase ...
    m[17:50, trunk] = 1                        # ... to the trunk, which the low end of every staircase touches
    for (cy, cx), (_, blob) in zip(CORNERS, corner_diagonal_parts(ne)):
        for t in range(-3, 2):
            m[cy + t, cx - 1 - t if ne else cx + t] = 1
        m[blob] = 1
    return m


NOISE = [(50, 64, 0.3, 1), (50, 64, 0.5, 2), (50, 64, 0.6, 3), (50, 64, 0.7, 4),
         (60, 50, 0.3, 5), (60, 50, 0.5, 6), (60, 50, 0.6, 7), (60, 50, 0.7, 8), (100, 120, 0.6, 9)]


@functools.lru_cache(maxsize=None)
def cases_with_ref(h, w):
    """(names, stacked maps (n, h, w), stacked brute results), computed once per shape."""
    cs = shape_cases(h, w)
    if (h, w) in ((100, 120), (150, 200)):
        k = host_params(h, w)[0]
        cs["blobs_joined"] = joined_blobs(h, w, k - 1)
        cs["blobs_apart"] = joined_blobs(h, w, k)
    if (h, w) in CORNER_SHAPES:
        cs["corner_diagonals_nw"] = corner_diagonals(h, w, False)
        cs["corner_diagonals_ne"] = corner_diagonals(h, w, True)
    for nh, nw, d, seed in NOISE:
        if (nh, nw) == (h, w):
            cs[f"noise_{d}"] = noise(h, w, d, seed)
    names = list(cs)
    maps = np.stack([cs[n] for n in names])
    ref = np.stack([brute(m) for m in maps])
    maps.setflags(write=False)
    ref.setflags(write=False)
    return names, maps, ref
