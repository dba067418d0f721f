"""Calibration on the CPU: the two routes of the restatement of DESIGN.md §6.22 (tests/quad_ref.py) agree on every
case the GPU tests use and those cases are not vacuous; calibration.refine, order_tile_corners and solve on hand-made
inputs; quad_params' defaults and refusals; the accuracy of the scheme on the rendered cases; and the round trip
through a known bird's-eye matrix. No GPU."""
import math

import numpy as np
import pytest

import quad_ref as R
from bugcar_image_segmentation_amd import calibration as C
from bugcar_image_segmentation_amd import synthetic
from bugcar_image_segmentation_amd.bev import order_points_counter_clockwise


def same_integers(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("status", "threshold", "area", "root", "corners", "moments"))


def device_view(r):
    """find_tile's dict as find_quad returned it."""
    return dict(r, status=r["status0"])


@pytest.mark.parametrize("which", R.GROUPS)
@pytest.mark.parametrize("h,w", R.SHAPES, ids=lambda v: str(v))
def test_the_two_routes_agree(h, w, which):
    names, frames, p, refs = R.group(h, w, which)
    for name, f, r in zip(names, frames, refs):
        assert same_integers(R.find_quad(f, p, brute=True), device_view(r)), name


def test_the_two_routes_agree_on_the_camera_sized_frames():
    names, frames, p, refs = R.big_group()
    for name, f, r in zip(names, frames, refs):
        assert r["status"] == R.OK, name
        assert same_integers(R.find_quad(f, p, brute=True), device_view(r)), name


def test_the_cases_are_not_vacuous():
    for h, w in R.SHAPES:
        names, frames, p, refs = R.group(h, w, "grey")
        by = dict(zip(names, refs))
        m = R.masks(h, w)
        # the exact rectangle: c0 and c1 are opposite corners, c2 ties between the other two and the lower index wins
        x0, x1, y0, y1 = w // 5, 4 * w // 5 - 1, h // 4, 3 * h // 4 - 1
        assert by["rect"]["corners"].tolist() == [[x1, y1], [x0, y1], [x0, y0], [x1, y0]]
        assert by["rect"]["root"] == y0 * w + x0 and by["rect"]["area"] == int(m["rect"].sum())
        # the trapezoid: c1 is c0's neighbour (the long base), so the fourth corner is not inserted between them
        c = by["foreshortened"]["corners"]
        assert by["foreshortened"]["status0"] == R.OK and abs(int(c[0][1]) - int(c[1][1])) <= 4, c.tolist()
        assert by["holes"]["area"] < by["rect"]["area"] and by["holes"]["moments"][:, 0].sum() > by["rect"]["moments"][:, 0].sum()
        a, b = h // 5, w // 5
        assert by["equal"]["area"] == a * b and by["equal"]["root"] == 2 * w + (w - 3 - b)        # the upper right one
        assert by["border"]["area"] == int(m["border"][:, w // 2:].sum()) < int(m["border"][:, :w // 2].sum())
        assert by["none"]["status0"] == R.NO_TILE and by["none"]["threshold"] >= 0
        assert by["triangle"]["status0"] == R.DEGENERATE and by["triangle"]["area"] == int(m["triangle"].sum())
        assert by["uniform"]["status0"] == R.NO_TILE and by["uniform"]["threshold"] == -1
        assert {r["status0"] for r in refs} == {R.OK, R.NO_TILE, R.DEGENERATE}
        assert by["diamond"]["status"] == R.OK and by["rect"]["status"] == R.OK
        for which in R.GROUPS:
            assert any(r["status"] == R.OK for r in R.group(h, w, which)[3]), which


@pytest.mark.parametrize("h,w", R.SHAPES + [R.BIG], ids=lambda v: str(v))
def test_otsu_inputs_have_one_best_threshold(h, w):
    groups = [R.big_group()] if (h, w) == R.BIG else [R.group(h, w, g) for g in ("grey", "bgr", "dark")]
    for names, frames, p, refs in groups:
        for name, f in zip(names, frames):
            assert R.otsu_margin(R.grey(f)) > 1e-9, name


def test_otsu_by_hand():
    g = np.array([[10] * 6 + [20] * 2 + [200] * 4], np.uint8)
    # t = 10: d = 10 - 140, v = 6 * 6 * 16900; t = 20: d = 12.5 - 200, v = 8 * 4 * 35156.25
    v = R.otsu_values(g)
    assert v[9] is None and v[10] == 608400.0 and v[19] == 608400.0 and v[20] == 1125000.0 and v[199] == 1125000.0 and v[200] is None
    assert R.otsu(g) == 20 and R.otsu(np.full((3, 3), 9, np.uint8)) == -1
    assert R.grey(np.array([[[10, 200, 100]]], np.uint8))[0, 0] == (18680 + 1923400 + 489900 + 8192) >> 14


# ---------------------------------------------------------------- the host functions on hand-made inputs
def rectangle_moments(x0, y0, x1, y1):
    """The crack points of the pixel rectangle [x0, x1] x [y0, y1] and its doubled pixel corners, cyclic."""
    mask = np.zeros((y1 + 6, x1 + 6), bool)
    mask[y0:y1 + 1, x0:x1 + 1] = True
    c2 = 2 * np.array([[x1, y1], [x0, y1], [x0, y0], [x1, y0]])
    return mask, c2


def test_refine_gives_an_exact_rectangle_its_exact_sides():
    mask, c2 = rectangle_moments(5, 4, 44, 23)
    mom = R.moments(mask, c2, 3)
    # a side runs between pixel centres, 39 and 19 px: its middle three quarters hold the cracks of pixels 10 .. 39
    # of the 40 along x and 7 .. 20 of the 20 along y
    assert mom[:, 0].tolist() == [30, 14, 30, 14]
    want = np.array([[44.5, 23.5], [4.5, 23.5], [4.5, 3.5], [44.5, 3.5]])
    for fn in (lambda a, b: C.refine(a[None], b[None]), lambda a, b: tuple(np.asarray(v)[None] for v in R.refine(a, b))):
        st, c = fn(c2, mom)
        assert st.tolist() == [C.OK] and np.abs(c[0] - want).max() < 1e-12
    # a side short of points, and a frame of zeros, are DEGENERATE and come back as they went in, halved
    st, c = C.refine(np.stack([c2, c2, np.zeros((4, 2), int)]), np.stack([mom, mom, np.zeros((4, 6), int)]), min_points=16)
    assert st.tolist() == [C.DEGENERATE] * 3 and np.array_equal(c[0], c2 / 2) and not c[2].any()
    # parallel adjacent lines
    par = mom.copy()
    par[1] = par[0]
    par[1][2] += 10 * par[1][0]                                      # the same points 5 px lower (sum Y only: means move)
    par[1][4] += 10 * par[1][1]
    par[1][5] += 20 * par[0][2] + 100 * par[1][0]
    assert C.refine(c2[None], par[None])[0].tolist() == [C.DEGENERATE]
    assert R.refine(c2, par)[0] == R.DEGENERATE
    with pytest.raises(ValueError):
        C.refine(np.zeros((2, 4, 2)), np.zeros((1, 4, 6)))


def test_refine_agrees_with_the_restatement_on_the_rendered_cases():
    for name in R.QUADS:
        r = R.find_tile(R.rendered(name, 0), R.params(*R.QUADS[name][0]))
        st, c = C.refine((2 * r["corners"])[None], r["moments"][None])
        st2, c2 = C.refine(r["corners2"][None], r["moments2"][None])
        assert st.tolist() == [C.OK] and st2.tolist() == [C.OK]
        assert np.array_equal(np.rint(2 * c[0]).astype(np.int32), r["corners2"])
        assert np.abs(c2[0] - r["refined"]).max() < 1e-9


def target_points(bev):
    """What calculate_transform_matrix pairs tile_coords with, and the same points before its ordering."""
    mh = bev.tile_length / bev.cm_per_px
    t = np.array([bev.after_warp_width / 2 + bev.dist2target[0] / bev.cm_per_px, bev.after_warp_height - bev.dist2target[1] / bev.cm_per_px])
    rot = np.array([[math.cos(bev.yaw), -math.sin(bev.yaw)], [math.sin(bev.yaw), math.cos(bev.yaw)]])
    pts = np.array([rot @ p for p in ([mh / 2, mh / 2], [mh / 2, -mh / 2], [-mh / 2, -mh / 2], [-mh / 2, mh / 2])]) + t
    axis = np.stack([t, rot @ np.array([100.0, 0.0]) + t])
    return order_points_counter_clockwise(pts.copy(), axis), pts


@pytest.mark.parametrize("yaw", [0.0, 0.3, -0.3, 0.78, -0.78])
def test_order_tile_corners_is_the_order_of_the_target_points(yaw):
    bev = round_trip_bev()
    bev.yaw = yaw
    ordered, pts = target_points(bev)
    for perm in ([0, 1, 2, 3], [2, 0, 3, 1], [3, 2, 1, 0], [1, 3, 0, 2]):
        assert np.array_equal(C.order_tile_corners(pts[perm]), ordered), perm
    near_left, near_right, far_left, far_right = ordered
    assert near_left[1] > far_left[1] and near_right[1] > far_right[1] and near_left[0] < near_right[0] and far_left[0] < far_right[0]


def test_solve_takes_the_median_of_the_good_frames_and_reports_the_spread():
    bev = round_trip_bev()
    base = np.array([[30.0, 90.0], [120.0, 91.0], [60.0, 70.0], [95.0, 69.0]])      # near-left, near-right, far-left, far-right
    cyc = [1, 0, 2, 3]                                                               # a cyclic order, as find_tile gives
    frames = np.stack([base[cyc] + d for d in (0.0, 0.5, -0.25, 40.0, 0.125)])
    frames[4] = np.roll(frames[4], 2, axis=0)                                        # another start of the cycle
    status = np.array([C.OK, C.OK, C.OK, C.DEGENERATE, C.OK])
    rep = C.solve(bev, frames, status)
    assert rep["frames_used"] == [0, 1, 2, 4]
    assert np.array_equal(rep["tile_coords"], base + 0.0625)                         # the median of 0, .5, -.25, .125
    assert rep["spread_px"] == pytest.approx(math.hypot(0.4375, 0.4375), abs=1e-12)
    ordered, _ = target_points(bev)
    q = np.c_[rep["tile_coords"], np.ones(4)] @ rep["matrix"].T
    assert np.abs(q[:, :2] / q[:, 2:] - ordered).max() < 1e-4 and rep["matrix"] is bev._bev_matrix
    swapped = C.solve(bev, frames, status, order=(1, 0, 3, 2))
    assert np.array_equal(swapped["tile_coords"], (base + 0.0625)[[1, 0, 3, 2]])


def test_solve_refusals():
    bev = round_trip_bev()
    c = np.zeros((2, 4, 2))
    with pytest.raises(ValueError, match="no frame"):
        C.solve(bev, c, np.array([C.NO_TILE, C.DEGENERATE]))
    with pytest.raises(ValueError):
        C.solve(bev, c, np.array([C.OK]))
    with pytest.raises(ValueError, match="permutation"):
        C.solve(bev, c, np.array([C.OK, C.OK]), order=(0, 1, 2, 2))
    for yaw in (math.pi / 4, -1.0, 2.0):
        bev.yaw = yaw
        with pytest.raises(ValueError, match="yaw"):
            C.solve(bev, c + np.arange(8).reshape(4, 2), np.array([C.OK, C.OK]))
        C.solve(bev, c + np.array([[0, 9], [9, 9], [1, 0], [8, 0]]), np.array([C.OK, C.OK]), order=(0, 1, 2, 3))


def test_quad_params_defaults_and_refusals():
    p = C.quad_params(480, 640)
    assert (p.rows, p.cols, p.channels, p.bright, p.threshold, p.min_area, tuple(p.band)) == (480, 640, 3, 1, -1, 307, (3, 2))
    assert C.quad_params(48, 64).min_area == 16 and C.quad_params(48, 64, min_area=5, threshold=0, bright=False, band=(0, 64)).min_area == 5
    for h, w in R.SHAPES:
        assert C.quad_params(h, w).min_area == R.params(h, w)["min_area"]
    for kw in (dict(h=2), dict(w=2), dict(h=4097), dict(w=4097), dict(threshold=255), dict(threshold=-1), dict(threshold=1.5),
               dict(min_area=0), dict(band=(3,)), dict(band=(65, 2)), dict(band=(3, -1)), dict(channels=2)):
        a = dict(h=48, w=64)
        a.update(kw)
        with pytest.raises(ValueError):
            C.quad_params(**a)


# ---------------------------------------------------------------- accuracy of the scheme (the restatement alone)
ACCURACY_BOUND_PX = 0.75        # between the scheme's 0.47 px and the 1.48 px of moments over inner pixel centres


def test_accuracy_on_the_rendered_cases():
    """Measured here: the coarse corners are 0.92 to 6.90 px off, one refinement pass gives up to 0.94 px, two passes
    0.470 px at the worst (the 48 x 64 quad)."""
    worst = 0.0
    for name, ((h, w), quad) in R.QUADS.items():
        for seed in R.SEEDS:
            r = R.find_tile(R.rendered(name, seed), R.params(h, w))
            assert r["status"] == R.OK, (name, seed)
            idx, err = R.match_error(r["refined"], quad)
            _, coarse = R.match_error(r["corners"], quad)
            print(f"{name} seed {seed}: coarse {coarse:.3f} px, refined {err:.3f} px")
            assert sorted(idx) == [0, 1, 2, 3], (name, seed, idx)
            assert err < coarse, (name, seed, err, coarse)
            worst = max(worst, err)
    print(f"worst refined corner: {worst:.3f} px")
    assert worst <= ACCURACY_BOUND_PX


# ---------------------------------------------------------------- round trip through a known matrix
RT_SEEDS = (0, 1, 2, 3)
RT_MEASURED_BEV_PX = 0.384       # what the restatement gives on these four frames (0.143 px in the image)
RT_BOUND_BEV_PX = 2 * RT_MEASURED_BEV_PX      # a factor 2 for the noise seeds not drawn


def round_trip_bev():
    """120 x 160 -> 200 x 200 with a 30 cm tile 25 cm ahead: its image is a trapezoid well inside the frame."""
    bev = synthetic.synthetic_bev(120, 160, 200, 200)
    bev.dist2target, bev.tile_length = (0.0, 25.0), 30.0
    return bev


def round_trip_truth():
    """-> (the bev with its known matrix, the tile's true image corners in calculate_transform_matrix's order, the
    target points)."""
    bev = round_trip_bev()
    ordered, _ = target_points(bev)
    q = np.c_[ordered, np.ones(4)] @ np.linalg.inv(bev._bev_matrix).T
    return bev, q[:, :2] / q[:, 2:], ordered


def round_trip_frames(bgr=False):
    _, img, _ = round_trip_truth()
    cyc = img[[0, 1, 3, 2]]                                   # near-left, near-right, far-right, far-left: convex order
    return np.stack([R.render(120, 160, cyc, 60, 200, 4.0, s, R.standard_blobs(120, 160), bgr) for s in RT_SEEDS])


def test_round_trip_through_a_known_matrix():
    bev, img, target = round_trip_truth()
    assert img.min() > 8 and (img[:, 0] < 152).all() and (img[:, 1] < 112).all()
    known = bev._bev_matrix.copy()
    refs = [R.find_tile(f, R.params(120, 160)) for f in round_trip_frames()]
    rep = C.solve(bev, np.stack([r["refined"] for r in refs]), np.array([r["status"] for r in refs]))
    assert rep["frames_used"] == list(range(len(RT_SEEDS)))
    q = np.c_[img, np.ones(4)] @ rep["matrix"].T
    err = float(np.linalg.norm(q[:, :2] / q[:, 2:] - target, axis=1).max())
    print(f"round trip: tile_coords {np.linalg.norm(rep['tile_coords'] - img, axis=1).max():.3f} px off in the image, "
          f"{err:.3f} px in the bird's-eye view, spread {rep['spread_px']:.3f} px")
    assert err <= RT_BOUND_BEV_PX
    assert not np.array_equal(known, rep["matrix"])
