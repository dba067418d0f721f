"""calibration.calibrate end to end on the device: rendered frames of a tile seen through a known bird's-eye matrix
(the round-trip geometry of tests/test_quad_host.py) -> the report must be what calibration.solve makes of the
restatement's detections (tests/quad_ref.py), the saved JSON must load to the same matrix, the line check must
report, and frames without a tile must raise."""
import numpy as np
import pytest
import torch

import quad_ref as R
import test_quad_host as H
from bugcar_image_segmentation_amd import calibration as C
from bugcar_image_segmentation_amd.bev import bev_transform_tools

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    """The BGR frames (B = 4, one noise seed each) and what solve makes of the restatement's detections."""
    frames = H.round_trip_frames(bgr=True)
    refs = [R.find_tile(f, R.params(120, 160)) for f in frames]
    assert all(r["status"] == R.OK for r in refs)
    bev = H.round_trip_bev()
    rep = C.solve(bev, np.stack([r["refined"] for r in refs]), np.array([r["status"] for r in refs]))
    return frames, rep


def test_calibrate_equals_solve_on_the_restatement(gpu, expected, tmp_path):
    frames, want = expected
    bev, img, target = H.round_trip_truth()
    rep = C.calibrate(bev, frames)
    assert rep["frames_used"] == want["frames_used"] == [0, 1, 2, 3] and rep["status"].tolist() == [C.OK] * 4
    assert np.abs(rep["tile_coords"] - want["tile_coords"]).max() <= 1e-9
    # calculate_transform_matrix rounds tile_coords to float32 first: equal roundings give the same matrix bit for bit;
    # a corner within 1e-9 of a rounding boundary may move by one float32 step (2^-17 px below 128), which the tile's
    # magnification into the bird's-eye view (below 4) keeps under 1e-3 px there
    if np.array_equal(rep["tile_coords"].astype(np.float32), want["tile_coords"].astype(np.float32)):
        assert np.array_equal(rep["matrix"], want["matrix"])
    q, qw = (np.c_[img, np.ones(4)] @ m.T for m in (rep["matrix"], want["matrix"]))
    assert np.abs(q[:, :2] / q[:, 2:] - qw[:, :2] / qw[:, 2:]).max() <= 1e-3
    assert abs(rep["spread_px"] - want["spread_px"]) <= 1e-9
    assert np.linalg.norm(q[:, :2] / q[:, 2:] - target, axis=1).max() <= H.RT_BOUND_BEV_PX
    path = tmp_path / "bev.json"
    bev.save_to_JSON(str(path))
    back = bev_transform_tools.fromJSON(str(path))
    assert np.array_equal(back._bev_matrix, np.asarray(rep["matrix"])) and np.array_equal(back._bev_matrix, bev._bev_matrix)
    # device tensors and grey frames go the same way
    dev = C.calibrate(H.round_trip_bev(), torch.from_numpy(frames).to(gpu))
    assert np.array_equal(dev["tile_coords"], rep["tile_coords"]) and np.array_equal(dev["matrix"], rep["matrix"])
    one = C.calibrate(H.round_trip_bev(), R.grey(frames[2]))
    assert one["frames_used"] == [0] and one["spread_px"] == 0.0


def test_line_check_reports(gpu, expected):
    frames, want = expected
    rep = C.calibrate(H.round_trip_bev(), frames, line_check=True)
    assert np.abs(rep["tile_coords"] - want["tile_coords"]).max() <= 1e-9
    assert set(rep["line_check"]) >= {"count", "theta0", "spread", "lines", "peaks"} and rep["line_spread"] == rep["line_check"]["spread"]


def test_no_tile_raises(gpu):
    bev = H.round_trip_bev()
    known = bev._bev_matrix.copy()
    with pytest.raises(ValueError, match="no frame"):
        C.calibrate(bev, np.full((3, 120, 160, 3), 90, np.uint8))
    with pytest.raises(ValueError, match="no frame"):
        C.calibrate(bev, R.from_mask(R.masks(120, 160)["none"], seed=1))
    assert np.array_equal(bev._bev_matrix, known)
    with pytest.raises(AssertionError):
        C.calibrate(bev, np.zeros((2, 48, 64), np.uint8))
    with pytest.raises(ValueError, match="yaw"):
        steep = H.round_trip_bev()
        steep.yaw = 1.0
        C.calibrate(steep, H.round_trip_frames()[:1])
