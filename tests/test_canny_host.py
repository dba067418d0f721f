"""Canny on the CPU: the two NumPy restatements of DESIGN.md §6.19 (tests/canny_ref.py) agree on every case the
GPU tests use, those cases are not vacuous (every direction class, strong, weak kept and weak dropped pixels; the
magnitudes at the thresholds; gradients on both sides of both direction boundaries), canny_params' floor, swap
and refusals, find_intersection_line on hand-computed cases and, wherever cv2 can be imported, the restatement
against OpenCV itself. No GPU."""
import numpy as np
import pytest

import canny_ref as R
from bugcar_image_segmentation_amd import image_processing_utils as ipu


@pytest.mark.parametrize("h,w", R.SHAPES, ids=lambda v: str(v))
def test_the_two_restatements_agree(h, w):
    im = R.images(h, w)
    for t1, t2 in R.THRESHOLDS:
        low, high = R.thresholds(t1, t2)
        for name, x in zip(R.CASE_NAMES, im):
            mp = R.nms(x, low, high)
            assert np.array_equal(mp, R.nms_loops(x, low, high)), (name, t1, t2)
            assert np.array_equal(R.hysteresis(mp), R.hysteresis_loops(mp)), (name, t1, t2)
    assert np.array_equal(R.canny(im[0], 49.9, 150.9), R.canny_loops(im[0], 49.9, 150.9))


def test_the_two_restatements_agree_on_the_camera_sized_frames():
    """The references of test_gpu_canny.py's 480 x 640 frames come from the vectorised restatement; the loops
    check them here, maps and edges."""
    h, w = R.BIG
    names, im, maps, edges = R.cases_with_ref(h, w, only=("scene", "noise"))
    assert names == ("scene", "noise")
    for name, x, mp, e in zip(names, im, maps, edges):
        by_loops = R.nms_loops(x, 50, 150)
        assert np.array_equal(by_loops, mp), name
        assert np.array_equal(R.hysteresis_loops(by_loops), e), name
        assert e.any() and ((mp == R.WEAK) & (e == 0)).any(), name          # edges, and weak pixels dropped


@pytest.mark.parametrize("h,w", R.MAP_SHAPES, ids=lambda v: str(v))
def test_the_two_floods_agree_on_the_hand_made_maps(h, w):
    names, mp, edges = R.maps_with_ref(h, w)
    for i, name in enumerate(names):
        assert np.array_equal(R.hysteresis_loops(mp[i]), edges[i]), name
    cand = (mp == R.STRONG) | (mp == R.WEAK)
    kept = edges == 255
    assert not (kept & ~cand).any()
    i = names.index("spiral_strong_last")
    assert (mp[i] == R.STRONG).sum() == 1 and cand[i].sum() > 2 * (h + w) and np.array_equal(kept[i], cand[i])
    assert tuple(np.argwhere(mp[i] == R.STRONG)[0]) == tuple(np.argwhere(cand[i])[-1])       # its raster-last pixel
    i = names.index("spiral_no_strong")
    assert cand[i].sum() > 2 * (h + w) and not kept[i].any()
    i = names.index("staircase")
    assert kept[i, 15, 63] and kept[i, 16, 64] and kept[i, 16, 65] and kept[i, 17, 64]       # through a tile corner
    assert cand[i, 16, 72] and not kept[i, 16, 72]                                           # the parallel one
    i = names.index("two_chains")
    assert kept[i].sum() * 2 == cand[i].sum() and kept[i].any()
    i = names.index("checkerboard")
    assert np.array_equal(kept[i], cand[i]) and (mp[i] == R.STRONG).sum() == 1
    assert not kept[names.index("all_weak")].any() and not kept[names.index("all_none")].any()
    assert kept[names.index("all_strong")].all()
    for n in ("random_a", "random_b"):
        i = names.index(n)
        assert 0 < kept[i].sum() < cand[i].sum()
        assert ((mp[i] > 2).sum()) > 0                   # "none" in other bytes than 1


@pytest.mark.parametrize("h,w", [(17, 65), (48, 80), (33, 131), (100, 100), R.BIG], ids=lambda v: str(v))
def test_the_scene_holds_pixels_of_every_kind(h, w):
    counts = R.kind_counts(R.scene(h, w))
    print(counts)
    assert all(v > 0 for v in counts.values()), counts
    if (h, w) != (17, 65):
        assert all(v >= 100 for v in counts.values()), counts


@pytest.mark.parametrize("h,w", [(17, 65), (48, 80), (33, 131), (100, 100)], ids=lambda v: str(v))
def test_the_structured_cases_sit_where_they_should(h, w):
    im = dict(zip(R.CASE_NAMES, R.images(h, w)))
    mp, m, dx, dy, cls = R.nms(im["ramp"], 50, 150, full=True)
    assert (m % 2 == 0).all()
    for v in (48, 50, 52, 148, 150, 152):
        assert (m == v).any(), v
    # a pixel with m = 50 is never a candidate at low = 50 and one with m = 150 never strong at high = 150
    assert (mp[m == 50] == R.NONE).all() and (mp[m == 150] != R.STRONG).all()
    assert (mp[m == 52] != R.NONE).any() and (mp[m == 152] == R.STRONG).any()
    assert min(R.near_boundary_counts(im["tangent"], 50)) >= 16, R.near_boundary_counts(im["tangent"], 50)
    # plateaus: neighbours of equal non-zero magnitude along x and along y, and the `>` / `>=` pair keeps one
    _, m, _, _, cls = R.nms(im["plateau"], 50, 150, full=True)
    assert ((m[:, 1:] == m[:, :-1]) & (m[:, 1:] > 50) & (cls[:, 1:] == 0)).any()
    assert ((m[1:] == m[:-1]) & (m[1:] > 50) & (cls[1:] == 1)).any()
    ex = R.canny(im["step_x"], 50, 150)
    assert (ex[:, w // 2 - 1] == 255).all() and ex.sum() == 255 * h         # the left pixel of the equal pair
    ey = R.canny(im["step_y"], 50, 150)
    assert (ey[h // 2 - 1] == 255).all() and ey.sum() == 255 * w            # the upper one
    assert not R.canny(im["constant"], 0, 0).any()
    assert R.canny(im["step_diag"], 50, 150).any() and R.canny(im["step_anti"], 50, 150).any()


def test_canny_params_floor_swap_and_refusals():
    def lh(*a, **kw):
        p = ipu.canny_params(*a, **kw)
        return p.rows, p.cols, p.low, p.high

    assert lh(48, 80, 50, 150) == (48, 80, 50, 150)
    assert lh(48, 80, 150, 50) == (48, 80, 50, 150)
    assert lh(1, 1, 49.9, 150.9) == (1, 1, 49, 150)
    assert lh(3, 2, -0.5, 5000) == (3, 2, -1, 5000)
    assert lh(3, 2, 7.99, -7.01) == (3, 2, -8, 7)
    assert lh(3, 2, 0, 0) == (3, 2, 0, 0)
    assert lh(3, 2, 1e30, -1e30) == (3, 2, -2 ** 31, 2 ** 31 - 1)
    assert lh(3, 2, 50, 150, apertureSize=3, L2gradient=False) == (3, 2, 50, 150)
    for t1, t2 in R.THRESHOLDS:
        assert lh(5, 5, t1, t2)[2:] == R.thresholds(t1, t2)
    for bad in [dict(apertureSize=5), dict(apertureSize=7), dict(apertureSize=1), dict(L2gradient=True)]:
        with pytest.raises(ValueError):
            ipu.canny_params(48, 80, 50, 150, **bad)
    for bad in [(0, 80, 50, 150), (48, 0, 50, 150), (-1, 5, 50, 150), (48, 80, float("nan"), 150),
                (48, 80, 50, float("nan")), (48, 80, float("inf"), 150), (48, 80, 50, float("-inf"))]:
        with pytest.raises(ValueError):
            ipu.canny_params(*bad)


def test_canny_refuses_what_is_no_grey_image_before_any_device_work():
    for bad in (np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.float32), np.zeros((8,), np.uint8)):
        with pytest.raises(ValueError):
            ipu.canny(bad, 50, 150)
    with pytest.raises(ValueError):
        ipu.canny(np.zeros((8, 8), np.uint8), 50, 150, apertureSize=5)
    with pytest.raises(ValueError):
        ipu.canny(np.zeros((8, 8), np.uint8), 50, 150, L2gradient=True)
    with pytest.raises(ValueError):
        ipu.canny(np.zeros((8, 8), np.uint8), float("nan"), 150)


def test_find_intersection_line_by_hand():
    f = ipu.find_intersection_line
    # y = x and y = -x + 4 meet in (2, 2)
    got = f([(0, 0), (1, 1)], [(0, 4), (4, 0)])
    assert isinstance(got, np.ndarray) and got.shape == (2,) and np.allclose(got, (2.0, 2.0), rtol=0, atol=1e-12)
    # y = 2 x + 1 and y = -0.5 x + 6 meet in (2, 5)
    assert np.allclose(f([(0, 1), (1, 3)], [(0, 6), (4, 4)]), (2.0, 5.0), rtol=0, atol=1e-12)
    # one vertical line, x = 3, against y = 2 x + 1, either way round: (3, 7)
    assert np.allclose(f([(3, -5), (3, 9)], [(0, 1), (1, 3)]), (3.0, 7.0), rtol=0, atol=1e-12)
    assert np.allclose(f([(0, 1), (1, 3)], [(3, 0), (3, 1)]), (3.0, 7.0), rtol=0, atol=1e-12)
    # a horizontal line, y = 4, against x = -2
    assert np.allclose(f([(0, 4), (10, 4)], [(-2, 0), (-2, 1)]), (-2.0, 4.0), rtol=0, atol=1e-12)
    # parallel lines, two vertical lines
    assert f([(0, 0), (2, 1)], [(0, 3), (4, 5)]) is None
    assert f([(1, 0), (1, 5)], [(2, 0), (2, 5)]) is None
    assert f([(0, 0), (1, 1)], [(0, 0), (1, 1)]) is None
    # the reference's quirk: a vertical line has a = 1, and so has a line of slope 1: None although they meet
    assert f([(3, 0), (3, 1)], [(0, 0), (5, 5)]) is None
    assert f([(0, 2), (1, 3)], [(7, 0), (7, 9)]) is None
    # integer and float inputs give the same answer; NumPy arrays are taken too
    a = f([(0, 0), (3, 1)], [(0, 5), (2, 0)])
    b = f([(0.0, 0.0), (3.0, 1.0)], [(0.0, 5.0), (2.0, 0.0)])
    c = f(np.array([[0, 0], [3, 1]]), np.array([[0, 5], [2, 0]]))
    # y = x / 3 and y = -2.5 x + 5: x = 30 / 17, y = 10 / 17
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.allclose(a, (30 / 17, 10 / 17), rtol=0, atol=1e-12)


def test_opencv_agrees_with_the_restatement():
    """Settles the recalled points (DESIGN.md §2 "canny: unpinned against cv2") wherever OpenCV is installed."""
    cv2 = pytest.importorskip("cv2")
    for (h, w) in R.SHAPES:
        for name, x in zip(R.CASE_NAMES, R.images(h, w)):
            for t1, t2 in R.THRESHOLDS:
                got = cv2.Canny(np.array(x), t1, t2, apertureSize=3, L2gradient=False)
                assert np.array_equal(got, R.canny(x, t1, t2)), (h, w, name, t1, t2)
