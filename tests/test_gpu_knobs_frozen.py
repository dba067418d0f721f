"""A context holds the BUGSEG_* knobs it was created under (csrc/knobs.h): changing the
environment afterwards changes nothing for it, not even when a new shape forces a plan rebuild."""
import ctypes

import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import deeplab_resnet as R
from bugcar_image_segmentation_amd import synthetic
from bugcar_image_segmentation_amd.models import ENET, DeepLabV3
from test_knobs import DEFAULTS

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(64, 96), (72, 104)]       # the second forces a plan rebuild
LATER = {"BUGSEG_NO_FUSE": "1", "BUGSEG_BNECK_GRID": "8", "BUGSEG_CLS_CONV": "1", "BUGSEG_INIT_TABLE": "1",
         "BUGSEG_TILE_ORDER": "0"}


@pytest.fixture
def clean_env(gpu, monkeypatch):
    for name in DEFAULTS:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _logits(model, bgr):
    _, H, W = bgr.shape[:3]
    out = torch.empty((B, model.num_classes, H, W), dtype=torch.float32, device=bgr.device)
    model.ctx.forward_bgr(bgr, B, H, W, N.OUT_LOGITS_F32, out)
    torch.cuda.synchronize()
    return out


def _plan(model, H, W):
    n = model.ctx.plan_info(B, H, W, N.OUT_LOGITS_F32, bgr_input=True)[0]
    return n, [model.ctx.plan_op(B, H, W, i)[0] for i in range(n)]


@pytest.fixture(scope="module")
def frames(gpu):
    return [torch.from_numpy(synthetic.road_frames(B, H, W, seed=H)).to(gpu) for H, W in SHAPES]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_a_clean_context_ignores_later_settings(clean_env, blocks, frames, prec):
    model, fresh = ENET(weights=blocks, precision=prec), ENET(weights=blocks, precision=prec)
    want = _logits(fresh, frames[1])
    want_plan = _plan(fresh, *SHAPES[1])
    _logits(model, frames[0])
    for name, value in LATER.items():
        clean_env.setenv(name, value)
    got = _logits(model, frames[1])
    n, tags = _plan(model, *SHAPES[1])
    assert n == want_plan[0] < 88, "the plan was rebuilt under the later environment"
    assert tags == want_plan[1]
    assert torch.equal(got, want)
    assert model.ctx.knobs() == DEFAULTS


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_an_unfused_context_stays_unfused(clean_env, blocks, frames, prec):
    fresh = ENET(weights=blocks, precision=prec)
    clean_env.setenv("BUGSEG_NO_FUSE", "1")
    model = ENET(weights=blocks, precision=prec)
    _logits(model, frames[0])
    clean_env.delenv("BUGSEG_NO_FUSE")
    got = _logits(model, frames[1])
    assert _plan(model, *SHAPES[1])[0] == 88
    assert torch.equal(got, _logits(fresh, frames[1]))      # (fused and unfused plans are bit-identical)
    assert model.ctx.knobs() == {**DEFAULTS, "BUGSEG_NO_FUSE": 1}
    assert fresh.ctx.knobs() == DEFAULTS


def test_create_refuses_a_bad_knob_and_leaves_no_context(clean_env, gpu, native_lib):
    clean_env.setenv("BUGSEG_TILE_ORDER", "7")
    h = ctypes.c_void_p()
    assert native_lib.bugseg_create(gpu.index, N.FP32, ctypes.byref(h)) == N.EINVAL
    assert h.value is None
    assert "BUGSEG_TILE_ORDER=7" in native_lib.bugseg_last_error(None).decode()
    with pytest.raises(ValueError, match="BUGSEG_TILE_ORDER"):
        N.Context(gpu.index, N.FP32)
    h = ctypes.c_void_p()
    assert native_lib.bugseg_dl_create(gpu.index, N.BF16, ctypes.byref(h)) == N.EINVAL and h.value is None
    assert "BUGSEG_TILE_ORDER=7" in native_lib.bugseg_dl_last_error(None).decode()


def test_a_deeplab_context_keeps_its_grouping_choice(clean_env, gpu):
    # (test_resnet_grouped_aspp_bit_identical's net: three same-shape atrous branches)
    net = R.build_deeplab_resnet(depth=50, units=(1, 1, 1, 1), crop=97, atrous_rates=(6, 12, 18))
    x = np.random.default_rng(46).integers(0, 256, (2, 97, 90, 3), dtype=np.uint8)
    clean_env.setenv("BUGSEG_DL_GROUP", "0")
    single = DeepLabV3(net=net, precision="bf16")
    clean_env.delenv("BUGSEG_DL_GROUP")
    grouped = DeepLabV3(net=net, precision="bf16")
    assert single.ctx.knobs() == {**DEFAULTS, "BUGSEG_DL_GROUP": 0}
    assert grouped.ctx.knobs() == DEFAULTS
    a = single.predict(x)
    la = single.logits_device().cpu()
    b = grouped.predict(x)
    assert torch.equal(la, grouped.logits_device().cpu())
    assert np.array_equal(a, b)
    assert single.ctx.knobs()["BUGSEG_DL_GROUP"] == 0
