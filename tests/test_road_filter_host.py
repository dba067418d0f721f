"""contour_noise_removal on the CPU: the two restatements of its pinned semantics agree on every case the GPU
tests use (tests/road_filter_ref.py), the case builders build what their names say, and the host arithmetic
of road_filter_params is the reference's (image_processing_utils.py:6-8, 19-27, 31, 38). No GPU."""
import numpy as np
import pytest
from scipy import ndimage

import road_filter_ref as R
from bugcar_image_segmentation_amd import image_processing_utils as ipu

ALL_SHAPES = R.SHAPES + [(60, 50)]


@pytest.mark.parametrize("h,w", ALL_SHAPES, ids=lambda v: str(v))
def test_brute_equals_tree(h, w):
    names, maps, ref = R.cases_with_ref(h, w)
    for name, m, want in zip(names, maps, ref):
        got = R.tree(m)
        assert got.dtype == np.uint8 and got.shape == (h, w)
        assert np.array_equal(got, want), f"{name} at {h}x{w}: {np.count_nonzero(got != want)} pixels differ"


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 9])
def test_the_two_closings_agree(k):
    rng = np.random.default_rng(k)
    for d in (0.2, 0.5, 0.8):
        m = rng.random((37, 41)) < d
        assert np.array_equal(R.close_shifts(m, k), R.close_filters(m, k))


@pytest.mark.parametrize("h,w", R.SHAPES, ids=lambda v: str(v))
def test_cases_are_what_they_say(h, w):
    names, maps, ref = R.cases_with_ref(h, w)
    k, y_top, mc = R.host_params(h, w)
    case = dict(zip(names, zip(maps, ref)))

    def closed(name):
        return R.close_shifts(case[name][0], k)

    assert not case["zeros"][1].any() and case["ones"][1].all()
    m, out = case["two_blocks"]
    assert ndimage.label(closed("two_blocks"), structure=R.S8)[1] == 2 and np.array_equal(out, closed("two_blocks"))
    for name, kept in (("block_min_count_minus_1", False), ("block_min_count", True)):
        c = closed(name)
        assert np.count_nonzero(c[y_top:]) == mc - 1 + kept, name
        assert out_equals(case[name][1], c if kept else np.zeros_like(c)), name
    c = closed("small_hole")
    assert ndimage.label(~c, structure=R.S4)[1] == 2 and np.array_equal(case["small_hole"][1], ndimage.binary_fill_holes(c))
    c = closed("ring_hole_open")
    assert ndimage.label(~c, structure=R.S4)[1] == 2 and np.array_equal(case["ring_hole_open"][1], c)
    c = closed("ring_hole_filled")
    assert ndimage.label(~c, structure=R.S4)[1] == 2
    assert np.array_equal(case["ring_hole_filled"][1], ndimage.binary_fill_holes(c))
    # the island in the open hole is dropped (the map keeps the outer region only), the one in the small hole reads 1
    c = closed("island_in_open_hole")
    lab, n = ndimage.label(c, structure=R.S8)
    assert n == 2
    assert np.array_equal(case["island_in_open_hole"][1], lab == lab[h // 4 + 2, 3])
    c = closed("island_in_filled_hole")
    assert ndimage.label(c, structure=R.S8)[1] == 2
    assert np.array_equal(case["island_in_filled_hole"][1], ndimage.binary_fill_holes(c))
    for name in ("nest5", "nest5_small"):
        c = closed(name)
        assert ndimage.label(c, structure=R.S8)[1] == 3 and ndimage.label(~c, structure=R.S4)[1] == 3, name
    # a background pixel in the image corner is outside, not a hole: it is not filled
    if k == 1:
        out = case["corner_pixels"][1]
        assert out[0, 0] == 0 and out[h - 1, w - 1] == 0 and out.sum() == h * w - 2
    c = closed("foot_to_border")
    assert ndimage.label(~c, structure=R.S4)[1] == 1 and np.array_equal(case["foot_to_border"][1], c)
    # the pocket touches the outside only diagonally: 4-connected it is a region of its own, 8-connected not
    c = closed("diagonal_pocket")
    assert ndimage.label(~c, structure=R.S4)[1] == 2 and ndimage.label(~c, structure=R.S8)[1] == 1
    py, px = h // 3 + 1 + k + 2, w // 2 - 1 - k - 2                            # the pocket's centre: a hole, filled
    assert not c[py, px] and case["diagonal_pocket"][1][py, px] == 1
    # the two blobs touch only diagonally: 8-connected one component, and the upper one is kept with the lower
    c = closed("diagonal_blobs")
    assert ndimage.label(c, structure=R.S8)[1] == 1 and (k > 1 or ndimage.label(c, structure=R.S4)[1] == 2)
    assert np.array_equal(case["diagonal_blobs"][1], c)
    for name, nfg in (("serpentine", 2), ("spiral", 1)):
        c = closed(name)
        assert ndimage.label(c, structure=R.S8)[1] == nfg and ndimage.label(~c, structure=R.S4)[1] == 1, name
    if "blobs_joined" in case:
        assert ndimage.label(closed("blobs_joined"), structure=R.S8)[1] == 1
        assert ndimage.label(closed("blobs_apart"), structure=R.S8)[1] == 3
    assert case["values_0_255"][0].max() > 1


@pytest.mark.parametrize("ne", [False, True], ids=["nw", "ne"])
@pytest.mark.parametrize("h,w", R.CORNER_SHAPES, ids=lambda v: str(v))
def test_corner_diagonals_hang_on_the_link_across_the_corner(h, w, ne):
    names, maps, ref = R.cases_with_ref(h, w)
    name = "corner_diagonals_ne" if ne else "corner_diagonals_nw"
    m, out = maps[names.index(name)], ref[names.index(name)]
    assert R.host_params(h, w)[0] == 1 and np.array_equal(out, m)          # one component, kept whole
    for (y, x), blob in R.corner_diagonal_parts(ne):
        assert (y, x + ne) in R.CORNERS
        # the staircase's pixel at the corner and the one before it lie in diagonally opposite tiles, and no
        # straight neighbour stands in for the diagonal
        py, px = y - 1, x + 1 if ne else x - 1
        assert y % 16 == 0 and {x % 64, px % 64} == {0, 63}
        assert m[y, x] and m[py, px] and not m[y, px] and not m[py, x]
        assert out[blob].all()
        cut = m.copy()
        cut[y, x] = 0
        got = R.brute(cut)
        assert not got[blob].any(), f"the blob above corner {(y, x + ne)} does not depend on the link across it"
        assert got[h - 1, 0] == 1                                           # (the band block stays)


def out_equals(out, mask):
    return np.array_equal(out.astype(bool), mask.astype(bool))


def test_noise_gives_many_regions():
    names, maps, ref = R.cases_with_ref(50, 64)
    case = dict(zip(names, zip(maps, ref)))
    m, out = case["noise_0.3"]
    assert ndimage.label(m, structure=R.S8)[1] + ndimage.label(m == 0, structure=R.S4)[1] > 100 and not out.any()
    m, out = case["noise_0.6"]
    assert out.any() and not np.array_equal(out, m)


# (h, w) -> (k, y_top, min_count), worked by hand from the reference's expressions
PARAMS = {
    (50, 50): (1, 45, 101),        # mask_area 250, * 0.4 = 100.0 exactly: > 100 means >= 101
    (100, 120): (2, 90, 481),      # 1200 * 0.4 = 480.0
    (150, 200): (3, 135, 1201),    # 3000 * 0.4 = 1200.0
    (256, 512): (5, 230, 5325),    # 13312 * 0.4 = 5324.8
    (480, 640): (9, 432, 12289),   # 30720 * 0.4 = 12288.0
    (53, 50): (1, 47, 121),        # 300 * 0.4 = 120.0
    (51, 67): (1, 45, 161),        # 402 * 0.4 = 160.8: not an integer
    (99, 51): (1, 89, 205),        # 510 * 0.4 = 204.0
}


@pytest.mark.parametrize("hw", list(PARAMS), ids=lambda v: str(v))
def test_road_filter_params(hw):
    h, w = hw
    p = ipu.road_filter_params(h, w)
    assert (p.rows, p.cols) == (h, w)
    assert (p.k, p.y_top, p.min_count) == PARAMS[hw]
    assert (p.k, p.y_top, p.min_count) == R.host_params(h, w)
    # the reference's own test, count > mask_area * 0.4, flips exactly at min_count
    thresh = (w * (h - int(h * (1 - 0.1)))) * 0.4
    assert p.min_count > thresh and not (p.min_count - 1 > thresh)


@pytest.mark.parametrize("hw", [(49, 64), (64, 49), (10, 10), (0, 50)])
def test_small_maps_are_refused(hw):
    with pytest.raises(ValueError):
        ipu.road_filter_params(*hw)
    with pytest.raises(ValueError):
        ipu.contour_noise_removal(np.zeros(hw, np.uint8))


def test_models_imports_it_as_the_reference_does():
    from bugcar_image_segmentation_amd import models
    assert models.contour_noise_removal is ipu.contour_noise_removal


def test_pipeline_refuses_the_filter_without_binary():
    from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline
    with pytest.raises(ValueError, match="binary"):
        OccupancyPipeline(None, None, 1.0, 1.0, 0.1, road_filter=True, binary=False)
