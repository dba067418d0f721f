"""create_skeleton (image_processing_utils.py:95-105 with a working call shape) on the device: for the three
geometries of the reference-glue fixtures (tests/golden/ref_glue.npz) it equals the Canny restatement
(tests/canny_ref.py) of the oracle's occupancy grid of an all-ones map, read as uint8, at 50 / 150."""
import json
import os

import numpy as np
import pytest

import canny_ref as R
from bugcar_image_segmentation_amd import image_processing_utils as ipu
from bugcar_image_segmentation_amd.bev import bev_transform_tools
from oracle import ocv_np

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_glue.npz")
GEOMS = ("bench", "small_neg", "small_odd")


@pytest.fixture(scope="module")
def fx():
    with np.load(FIX, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def geometry(fx, g, tmp_path):
    d = json.loads(bytes(fx[f"{g}/json"]).decode())
    d["is_laserscan"] = False
    p = tmp_path / f"{g}.json"
    p.write_text(json.dumps(d))
    gw, gh, cell = (float(v) for v in fx[f"{g}/grid"])
    return d, bev_transform_tools.fromJSON(str(p)), (gw, gh, cell)


@pytest.mark.parametrize("g", GEOMS)
def test_skeleton_equals_canny_of_the_oracles_grid(gpu, fx, g, tmp_path):
    d, bev, grid = geometry(fx, g, tmp_path)
    rows, cols = fx[f"{g}/segmaps"][0].shape
    M = np.asarray(d["bev matrix"], np.float64).reshape(3, 3)
    aw, ah = d["output image size"]
    occ = ocv_np.create_occupancy_grid(np.ones((rows, cols), np.uint8), M, aw, ah, d["cm_per_px"], *grid)
    assert occ.dtype == np.int8
    as_u8 = occ.astype(np.uint8)
    assert set(np.unique(as_u8)) <= {0, 100, 255}
    want = R.canny(as_u8, 50, 150)
    got = ipu.create_skeleton(bev, (cols, rows), *grid)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.flags.owndata and got.shape == occ.shape
    assert np.array_equal(got, want), f"{g}: {np.count_nonzero(got != want)} pixels differ"
    assert np.array_equal(want, R.canny_loops(as_u8, 50, 150))
    if g == "bench":
        assert got.any() and set(np.unique(got)) == {0, 255}


def test_a_wrong_input_shape_fails_the_transformers_assertion(gpu, fx, tmp_path):
    d, bev, grid = geometry(fx, "small_odd", tmp_path)
    rows, cols = fx["small_odd/segmaps"][0].shape
    with pytest.raises(AssertionError, match="segmap"):
        ipu.create_skeleton(bev, (cols + 1, rows), *grid)
    if rows != cols:
        with pytest.raises(AssertionError, match="segmap"):
            ipu.create_skeleton(bev, (rows, cols), *grid)            # (height, width) where (width, height) is due
