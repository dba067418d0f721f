"""mapping.LocalMap on the device (csrc/map_kernels.hip): the payload and state() bit for bit the
restatement in tests/map_ref.py, on the cases the host test shares: a 24 x 20 window with 12 x 9 grids (odd w: a
half-cell centre), 33 x 47 with 16 x 16, and one case of 256 x 256 with 200 x 200 grids at B = 8. References are
computed once per case and layout and shared, read-only."""
import functools
import gc
import math

import numpy as np
import pytest
import torch

import map_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import mapping as M

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in R.cases()]


@functools.lru_cache(maxsize=None)
def _ref(name, ros=False):
    res = R.run_case(R.case(name), M.pose_record, R.fuse_np, ros)
    for _, s, o in res:
        s.setflags(write=False)
        o.setflags(write=False)
    return res


def _map(c, gpu, ros=False, **kw):
    return M.LocalMap(c["size"], R.CELL_M, c["grid_hw"], ros_layout=ros, device=gpu.index, **dict(c["kw"], **kw))


def _dev(grids, gpu, ros=False):
    return torch.from_numpy(R.to_ros(grids) if ros else np.ascontiguousarray(grids)).to(gpu)


def _check(lm, out, want, what):
    _, state, payload = want
    got_out, got_state = out.cpu().numpy(), lm.state().cpu().numpy()
    assert got_out.dtype == np.int8 and got_state.dtype == np.int16
    assert np.array_equal(got_out, payload), f"{what}: {int((got_out != payload).sum())} payload cells differ"
    assert np.array_equal(got_state, state), f"{what}: {int((got_state != state).sum())} states differ"


def _run(c, lm, gpu, ros=False):
    for n, ((grids, poses), want) in enumerate(zip(c["steps"], _ref(c["name"], ros))):
        _check(lm, lm.update(_dev(grids, gpu, ros), poses), want, f"{c['name']} update {n}")


@pytest.mark.parametrize("name", CASES)
def test_bit_for_bit(gpu, name):
    c = R.case(name)
    lm = _map(c, gpu)
    _run(c, lm, gpu)
    wx0, wy0 = (int(v) for v in _ref(name)[-1][0][:2])
    assert lm.origin_cells == (wx0, wy0) and lm.origin_m == (wx0 * R.CELL_M, wy0 * R.CELL_M)


@pytest.mark.parametrize("name", CASES)
def test_ros_layout(gpu, name):
    c = R.case(name)
    _run(c, _map(c, gpu, ros=True), gpu, ros=True)
    if not sum(R.ties(rec, c["size"], c["grid_hw"][1]) for rec, _, _ in _ref(name)):
        # no cell centre on a column boundary: ROS-layout input gives what plain input gives
        for (_, sa, oa), (_, sb, ob) in zip(_ref(name), _ref(name, True)):
            assert np.array_equal(sa, sb) and np.array_equal(oa, ob)


@pytest.mark.parametrize("name", ["small_b70", "mid_three_updates", "mid_frame_outside", "mid_scroll_xy", "big"])
def test_without_culling(gpu, name):
    c = R.case(name)
    _run(c, _map(c, gpu, cull=False), gpu)


def test_order_dependence_on_the_device(gpu):
    c, d = R.case("small_clamp_occ_then_free"), R.case("small_clamp_free_then_occ")
    a, b = _map(c, gpu), _map(d, gpu)
    _run(c, a, gpu)
    _run(d, b, gpu)
    sa, sb = a.state().cpu().numpy(), b.state().cpu().numpy()
    assert set(sa[sa != R.UNOBS].tolist()) == {230} and set(sb[sb != R.UNOBS].tolist()) == {350}


@pytest.mark.parametrize("name", ["small_b70", "big"])
def test_grids_at_an_odd_byte_offset(gpu, name):
    c = R.case(name)
    lm = _map(c, gpu)
    grids, poses = c["steps"][0]
    buf = torch.zeros(grids.size + 1, dtype=torch.int8, device=gpu)
    g = buf[1:].view(grids.shape)
    g.copy_(_dev(grids, gpu))
    assert g.data_ptr() % 2 == 1
    _check(lm, lm.update(g, poses), _ref(name)[0], name)


@pytest.mark.parametrize("name", ["small_three_updates", "mid_scroll_xy"])
def test_poisoned_state_and_reset(gpu, name):
    c = R.case(name)
    lm = _map(c, gpu)
    lm.state_buffer.fill_(0x5A5A)
    _run(c, lm, gpu)
    lm.state_buffer.fill_(-21846)
    lm.reset()
    assert (lm.state().cpu().numpy() == R.UNOBS).all()
    _run(c, lm, gpu)                                   # from the beginning: nothing of the poison, nothing of the first run


def test_side_stream(gpu):
    c = R.case("mid_three_updates")
    lm = _map(c, gpu)
    side = torch.cuda.Stream(device=gpu)
    dev = [_dev(g, gpu) for g, _ in c["steps"]]
    torch.cuda.synchronize(gpu)
    outs = []
    with torch.cuda.stream(side):
        for g, (_, poses) in zip(dev, c["steps"]):
            outs.append(lm.update(g, poses).clone())
    side.synchronize()
    for o, (_, _, payload) in zip(outs, _ref(c["name"])):
        assert np.array_equal(o.cpu().numpy(), payload)
    assert np.array_equal(lm.state().cpu().numpy(), _ref(c["name"])[-1][1])


def test_two_identical_runs(gpu):
    c = R.case("big")
    got = []
    for _ in range(2):
        lm = _map(c, gpu)
        out = lm.update(_dev(c["steps"][0][0], gpu), c["steps"][0][1])
        got.append((out.cpu().numpy(), lm.state().cpu().numpy(), lm.state_buffer.cpu().numpy()))
    assert all(np.array_equal(x, y) for x, y in zip(*got))


def test_three_updates_in_a_row(gpu):
    c = R.case("small_three_updates")
    assert len(c["steps"]) == 3
    _run(c, _map(c, gpu), gpu)


@pytest.mark.parametrize("name", ["small_three_updates", "mid_three_updates"])
def test_capture_and_back_to_back_replays(gpu, name):
    """set_poses + replay three times with nothing between them: no record may be overwritten while the launch that
    reads it is still to run."""
    c = R.case(name)
    lm = _map(c, gpu)
    dev = [_dev(g, gpu) for g, _ in c["steps"]]
    buf = torch.zeros_like(dev[0])
    replay = lm.capture(buf)
    assert (lm.state().cpu().numpy() == R.UNOBS).all()           # capturing ran nothing
    torch.cuda.synchronize(gpu)
    outs = []
    for g, (_, poses) in zip(dev, c["steps"]):
        buf.copy_(g, non_blocking=True)
        lm.set_poses(poses)
        outs.append(replay().clone())
    torch.cuda.synchronize(gpu)
    for o, (_, _, payload) in zip(outs, _ref(name)):
        assert np.array_equal(o.cpu().numpy(), payload)
    assert np.array_equal(lm.state().cpu().numpy(), _ref(name)[-1][1])
    with pytest.raises(ValueError):
        lm.set_poses(c["steps"][0][1][:2])
        replay()


def test_pipeline_and_map_in_one_graph(gpu, blocks):
    from bugcar_image_segmentation_amd import synthetic
    from bugcar_image_segmentation_amd.models import ENET
    from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline
    H, W, B = 64, 96, 4

    def pipe(**kw):
        return OccupancyPipeline(ENET(weights=blocks, precision="fp32"), synthetic.synthetic_bev(H, W, 200, 200), 2.0, 2.0, 0.05,
                                 model_hw=(H, W), **kw)

    frames = torch.from_numpy(synthetic.road_frames(B, H, W, seed=17)).to(gpu)
    poses = np.array([[0.02 * k, 0.01 * k * k, 0.1 * k] for k in range(B)])
    for ros in (False, True):
        p = pipe(ros_layout=ros)
        eager = p.local_map((96, 80))
        assert eager.grid_hw == (40, 40) and eager.cell_m == 0.05 and eager.ros_layout == ros
        grids = p.run(frames)
        want = eager.update(grids, poses).cpu().numpy()
        want_state = eager.state().cpu().numpy()
        # against the restatement too, from the grids the pipeline made
        rec, _ = M.pose_record(poses, (96, 80), 0.05)
        state, payload = R.fuse_np(None, rec, grids.cpu().numpy(), (96, 80), R.config((40, 40), ros=ros))
        assert np.array_equal(want, payload) and np.array_equal(want_state, state)
        seen = int((state != R.UNOBS).sum())
        print("ros" if ros else "plain", "observed cells:", seen)
        assert seen > 100

        q = pipe(ros_layout=ros)
        lm = q.local_map((96, 80))
        buf = torch.zeros_like(frames)
        q.run(buf)                                          # plans and tables are built outside the capture
        lm.set_poses(poses)
        gc.collect()                                         # (no finalizer inside the capture: pipeline.capture)
        torch.cuda.synchronize(gpu)
        graph = torch.cuda.CUDAGraph()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                out = lm.fuse(q.run(buf))
        finally:
            gc.enable()
        buf.copy_(frames)
        lm.reset()
        lm.set_poses(poses)
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(lm.state().cpu().numpy(), want_state)
    with pytest.raises(ValueError, match="pair"):
        bev = synthetic.synthetic_bev(H, W, 200, 200)
        bev.laserscan_like_occupancy_grid = True
        OccupancyPipeline(ENET(weights=blocks, precision="fp32"), bev, 2.0, 2.0, 0.05, model_hw=(H, W), binary=True).local_map((96, 80))


def test_message(gpu):
    c = R.case("small_negative_world")
    lm = _map(c, gpu)
    _run(c, lm, gpu)
    msg = lm.to_msg(stamp=12, frame_id="odom")
    rec, _, payload = _ref(c["name"])[-1]
    assert (msg.info.height, msg.info.width, msg.info.resolution) == (24, 20, R.CELL_M)
    assert (msg.info.origin.position.x, msg.info.origin.position.y) == (int(rec[0]) * R.CELL_M, int(rec[1]) * R.CELL_M)
    assert list(msg.data) == payload.reshape(-1).tolist() and msg.header.frame_id == "odom"


def test_python_refusals_launch_nothing(gpu):
    c = R.case("small_b1")
    lm = _map(c, gpu)
    grids, poses = c["steps"][0]
    good = _dev(grids, gpu)
    bad = [(good.to(torch.uint8), poses), (good.cpu(), poses), (good[:, :, :8], poses), (good[0], poses),
           (good.expand(2, -1, -1), poses), (good, np.zeros((2, 3))), (good, np.zeros((1, 2))),
           (torch.zeros((1, 24, 9), dtype=torch.int8, device=gpu)[:, ::2], poses)]
    for g, p in bad:
        with pytest.raises(ValueError):
            lm.update(g, p)
    with pytest.raises(ValueError):
        lm.fuse(good)                                       # no record was ever sent
    assert lm.origin_cells == (-10, -12) and (lm.state().cpu().numpy() == R.UNOBS).all()
    _run(c, lm, gpu)                                        # and the map is as new


def test_abi_refusals_launch_nothing(gpu):
    c = R.case("small_b1")
    grids, poses = c["steps"][0]
    g = _dev(grids, gpu)
    ctx = N.shared_context(gpu.index)
    rec = torch.from_numpy(M.pose_record(poses, c["size"], R.CELL_M)[0]).to(gpu)
    lut = torch.from_numpy(M.build_lut()).to(gpu)
    state = torch.full(c["size"], 1234, dtype=torch.int16, device=gpu)
    out = torch.full(c["size"], 77, dtype=torch.int8, device=gpu)
    both = torch.zeros(2048, dtype=torch.int8, device=gpu)

    class At:                                  # an address no tensor view can have
        def __init__(self, address):
            self.address = address

        def data_ptr(self):
            return self.address

    def params(**kw):
        return M.map_params(c["size"], c["grid_hw"], **kw)

    def tweak(**kw):
        p = params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    calls = [(None, 1, params(), rec, state, lut, out), (g, 1, params(), None, state, lut, out),
             (g, 1, params(), rec, None, lut, out), (g, 1, params(), rec, state, None, out),
             (g, 1, params(), rec, state, lut, None), (g, 0, params(), rec, state, lut, out),
             (g, 4097, params(), rec, state, lut, out)]
    for kw in (dict(map_rows=0), dict(map_cols=4097), dict(grid_rows=0), dict(grid_cols=4097), dict(l_min=0),
               dict(l_min=-32768), dict(l_max=0), dict(l_max=32768), dict(l_occ=0), dict(l_free=0), dict(ros_layout=2),
               dict(cull=-1)):
        calls.append((g, 1, tweak(**kw), rec, state, lut, out))
    calls.append((g, 1, params(), At(rec.data_ptr() + 4), state, lut, out))                                # record 4 bytes off
    calls.append((g, 1, params(), rec, At(both.data_ptr() + 1), lut, out))                                 # odd state address
    calls.append((g, 1, params(), rec, both[:960].view(torch.int16), lut, both[900:1380]))                 # state over out
    calls.append((g, 1, params(), rec, state, lut, g.view(-1)[:1]))                                        # out over the grids
    for n, (gg, B, p, r, s, l, o) in enumerate(calls):
        with pytest.raises(N.BugsegError) as e:
            ctx.map_fuse(gg, B, p, r, s, l, o, torch.cuda.current_stream(gpu))
        assert e.value.code == N.EINVAL, (n, str(e.value))
    torch.cuda.synchronize(gpu)
    assert (state == 1234).all() and (out == 77).all() and (both == 0).all()
    ctx.map_fuse(g, 1, params(), rec, state, lut, out, torch.cuda.current_stream(gpu))                     # the good call
    assert np.array_equal(out.cpu().numpy(), _ref(c["name"])[0][2])


def test_compose_feeds_two_cameras(gpu):
    """Poses are per grid: two cameras with different mounts are one batch, in time order."""
    c = R.case("mid_b1")
    rng = np.random.default_rng(3)
    vehicle = np.array([[0.2 * k, 0.05 * k, 0.1 * k] for k in range(4)])
    mounts = [(0.8, 0.0, 0.0), (-0.6, 0.0, math.pi)]
    poses = np.stack([M.compose(v, m) for v in vehicle for m in mounts])
    grids = R._rand_grids(rng, len(poses), c["grid_hw"])
    lm = _map(c, gpu)
    out = lm.update(_dev(grids, gpu), poses)
    rec, _ = M.pose_record(poses, c["size"], R.CELL_M)
    _check(lm, out, (rec,) + R.fuse_np(None, rec, grids, c["size"], R.config(c["grid_hw"])), "two cameras")
