"""GPU parity of the DeepLabV3 path (BASELINE config 4) through the C ABI
(bugseg_dl_*) against the CPU oracle (oracle/deeplab_oracle.py) on the same synthetic weights.

Tolerances: fp32 mode — logits within 1e-3 absolute of the oracle (fp64 at reduced width, fp32 at
full size), class maps exact wherever the oracle's top-2 margin of the upsampled logits exceeds 2.5x the measured max
logit error (floor 1e-5; the excused near-tie count is printed and bounded);
the resize + argmax stage is checked bit-exactly against the oracle's TF-formula restatement applied
to the GPU's own logits. bf16 mode — against the oracle's bf16-storage emulation: mean |dlogit|
< 2e-2, class agreement > 98%.
"""
import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import deeplab_spec as S
from bugcar_image_segmentation_amd import deeplab_resnet as R
from bugcar_image_segmentation_amd import deeplab_xception as X
from bugcar_image_segmentation_amd.models import DeepLabV3
from oracle import deeplab_oracle as O

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3


def _frames(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _gpu_logits(model):
    L = model.logits_device().cpu().numpy()[..., :model.net.num_classes]   # (B, h, w, C)
    return L.transpose(0, 3, 1, 2)


def _check_fp32(model, net, x, ref_dtype):
    got_cls = model.predict(x)
    got = _gpu_logits(model)
    ref = O.forward(net, x, dtype=ref_dtype).numpy()
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() < LOGIT_TOL, np.abs(got - ref).max()
    # resize + argmax kernel: bit-exact on the GPU's own logits
    assert np.array_equal(got_cls, O.predict(net, x, logits=got))
    # class maps vs the oracle wherever its margin decides them
    # (the bilinear upsampling is a convex combination: its logits are within the same max error)
    err = float(np.abs(got - ref).max())
    thr = max(2.5 * err, 1e-5)
    up = O.resize_bilinear_tf(ref, *S.crop_hw(net))[:, :, :x.shape[1], :x.shape[2]]
    s = np.sort(up, axis=1)
    decided = (s[:, -1] - s[:, -2]) > thr
    ref_cls = O.predict(net, x, logits=ref)
    assert got_cls.dtype == np.int64 and got_cls.shape == x.shape[:3]
    assert np.array_equal(got_cls[decided], ref_cls[decided])
    n_exc = int(decided.size - decided.sum())
    print(f"deeplab fp32 max|dlogit| {err:.2e}; margin threshold {thr:.2e}; excused {n_exc} of {decided.size}")
    assert n_exc / decided.size <= 1e-3


@pytest.mark.parametrize("B,H,W,os_,rates", [(2, 90, 97, 8, ()), (1, 97, 97, 16, (6, 12, 18)), (3, 64, 40, 8, ())])
def test_deeplab_fp32_small(gpu, B, H, W, os_, rates):
    net = S.build_deeplab(width=0.25, crop=97, output_stride=os_, atrous_rates=rates)
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(B, H, W, B * 7 + H), torch.float64)


@pytest.mark.parametrize("crop,B,H,W", [((65, 113), 2, 60, 113), ((121, 49), 1, 100, 49)])
def test_deeplab_fp32_non_square_crop(gpu, crop, B, H, W):
    """An export whose crop_size is not square (pad to crop_h x crop_w, resize back to it)."""
    net = S.build_deeplab(width=0.25, crop=crop, atrous_rates=(2,))
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(B, H, W, 5 + H), torch.float64)
    with pytest.raises(ValueError):
        model.predict(_frames(1, crop[0] + 1, 8, 0))
    with pytest.raises(ValueError):
        model.predict(_frames(1, 8, crop[1] + 1, 0))


def test_deeplab_fp32_many_classes(gpu):
    """More than 24 (padded) classes: the per-pixel resize + argmax kernel."""
    net = S.build_deeplab(width=0.25, crop=65, num_classes=30)
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(2, 65, 50, 9), torch.float64)


def test_deeplab_fp32_full_513(gpu):
    net = S.build_deeplab()
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(1, 513, 513, 3), torch.float32)


def test_deeplab_bf16_vs_storage_emulation(gpu):
    net = S.build_deeplab(width=0.5, crop=129)
    model = DeepLabV3(net=net, precision="bf16")
    x = _frames(2, 129, 120, 11)
    got_cls = model.predict(x)
    got = _gpu_logits(model)
    ref = O.forward(net, x, bf16_storage=True).numpy()
    assert np.abs(got - ref).mean() < 2e-2
    assert (got_cls == O.predict(net, x, logits=ref)).mean() > 0.98
    assert np.array_equal(got_cls, O.predict(net, x, logits=got))


def test_deeplab_bf16_full_batch_properties(gpu):
    """Config 4 shape in the throughput mode: batch independence and run-to-run determinism."""
    model = DeepLabV3(precision="bf16")
    x = _frames(4, 513, 513, 5)
    a = model.predict_device(x).clone()
    b = model.predict_device(x)
    assert torch.equal(a, b)
    one = DeepLabV3(net=model.net, precision="bf16").predict(x[2:3])
    assert np.array_equal(a[2:3].cpu().numpy(), one)
    assert a.min() >= 0 and a.max() < model.net.num_classes


def test_deeplab_errors(gpu):
    model = DeepLabV3(net=S.build_deeplab(width=0.25, crop=65), precision="fp32")
    with pytest.raises(ValueError):
        model.predict(_frames(1, 66, 40, 0))
    with pytest.raises(ValueError):
        model.predict(np.zeros((1, 10, 10, 4), np.uint8))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_deeplab_fused_dw_bit_identical(gpu, precision):
    """The depthwise-fused projection against the default plan (separate depthwise launches)."""
    net = S.build_deeplab(width=0.5, crop=129, atrous_rates=(6,))
    x = _frames(2, 129, 129, 21)
    fused = DeepLabV3(net=net, precision=precision, fuse_dw=True)
    plain = DeepLabV3(net=net, precision=precision)
    a = fused.predict(x)
    la = fused.logits_device().cpu()
    b = plain.predict(x)
    lb = plain.logits_device().cpu()
    assert torch.equal(la, lb)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_deeplab_fused_prep_bit_identical(gpu, precision):
    """The stem forming its operand from the raw RGB bytes (default) against the separate
    dl_prep_kernel launch: the same padded, normalised values, so identical logits and classes;
    images smaller than the crop in both dimensions exercise the mean-pixel padding."""
    net = S.build_deeplab(width=0.5, crop=129, atrous_rates=(6,))
    for B, H, W in ((2, 129, 129), (3, 100, 77)):
        x = _frames(B, H, W, 31 + H)
        fused = DeepLabV3(net=net, precision=precision)
        plain = DeepLabV3(net=net, precision=precision, fuse_prep=False)
        a = fused.predict(x)
        la = fused.logits_device().cpu()
        b = plain.predict(x)
        lb = plain.logits_device().cpu()
        assert torch.equal(la, lb)
        assert np.array_equal(a, b)


@pytest.mark.parametrize("style,crop", [("slim", S.CROP), ("folded", S.CROP), ("slim", (129, 193))])
def test_deeplab_from_frozen_graphdef(gpu, tmp_path, style, crop):
    """DeepLabV3(GRAPH_PB_PATH=<frozen GraphDef>) (models.py:104-110): the imported network on the GPU
    against the NumPy GraphDef interpreter's logits (the sess.run stand-in) and the oracle; the crop
    comes from the graph (an export at another crop than 513 runs at its own)."""
    from deeplab_graph_writer import write_deeplab_graph
    from oracle import tf_graph
    net = S.build_deeplab(width=0.25, crop=crop, atrous_rates=(2, 4))
    H, W = 120, 97
    pb = tmp_path / "deeplab.pb"
    pb.write_bytes(write_deeplab_graph(net, style, H, W))
    model = DeepLabV3(str(pb), precision="fp32")
    assert S.crop_hw(model.net) == S.crop_hw(net) and len(model.net.atrous) == 2
    x = _frames(1, H, W, 11)
    _check_fp32(model, model.net, x, torch.float32)
    lg = np.transpose(tf_graph.run(pb.read_bytes(), {"ImageTensor": x}, "logits"), (0, 3, 1, 2))
    assert np.abs(_gpu_logits(model) - lg).max() < LOGIT_TOL


@pytest.mark.parametrize("gtm", ["0", "1"])
@pytest.mark.parametrize("width,crop,B", [(0.5, 129, 2), (1.0, 97, 3)])
def test_deeplab_gemm_1x1_bit_identical(gpu, monkeypatch, width, crop, B, gtm):
    """The LDS-staged GEMM kernel of the 1x1 convolutions (default in bf16) against dl_conv_kernel
    (BUGSEG_DL_GEMM=0): the same k-steps through the same MFMA in the same order and the same
    epilogue, so identical logits and class maps — over tile tails (pixel counts not a multiple of
    256), 32-channel k tails, the residual projections and the per-image-bias projection."""
    net = S.build_deeplab(width=width, crop=crop, atrous_rates=(6,))
    x = _frames(B, crop, crop - 5, 41)
    monkeypatch.setenv("BUGSEG_DL_GTM", gtm)   # 256- / 128-pixel tiles
    gemm = DeepLabV3(net=net, precision="bf16")
    a = gemm.predict(x)
    la = gemm.logits_device().cpu()
    monkeypatch.setenv("BUGSEG_DL_GEMM", "0")
    plain = DeepLabV3(net=net, precision="bf16")
    b = plain.predict(x)
    lb = plain.logits_device().cpu()
    assert torch.equal(la, lb)
    assert np.array_equal(a, b)


# ---------------------------------------------------------------- Xception-65 / DeepLabV3+
@pytest.mark.parametrize("os_,rates,decoder,B,H,W", [(16, (2, 4), True, 2, 60, 65), (8, (2,), True, 1, 65, 65),
                                                     (16, (), False, 2, 65, 50)])
def test_xception_fp32_small(gpu, os_, rates, decoder, B, H, W):
    """Reduced-width Xception (2 middle modules) against the fp64 oracle: pre-activation modules,
    conv / sum / no skips, fixed padding of the strided layers, separable ASPP, the decoder's resize +
    concat + separable convs (or none), at output stride 16 and 8 (atrous exit flow)."""
    net = X.build_deeplab_xception(width=0.25, middle=2, crop=65, output_stride=os_, atrous_rates=rates,
                                   decoder=decoder)
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(B, H, W, 3 + H), torch.float64)


def test_xception_fp32_full_width(gpu):
    """The full Xception-65 (16 middle modules, 2048-channel exit, ASPP 6/12/18, decoder) at a 129
    crop against the fp32 oracle."""
    net = X.build_deeplab_xception(crop=129)
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(1, 129, 120, 8), torch.float32)


def test_xception_non_square_and_even_crop(gpu):
    """Even crop sides: a strided layer's fixed padding (1 before) differs from SAME's (0 before)."""
    net = X.build_deeplab_xception(width=0.25, middle=1, crop=(64, 98), atrous_rates=(2,))
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(2, 64, 90, 17), torch.float64)


def test_xception_bf16_vs_storage_emulation(gpu):
    net = X.build_deeplab_xception(width=0.5, middle=4, crop=129)
    model = DeepLabV3(net=net, precision="bf16")
    x = _frames(2, 129, 120, 12)
    got_cls = model.predict(x)
    got = _gpu_logits(model)
    ref = O.forward(net, x, bf16_storage=True).numpy()
    assert np.abs(got - ref).mean() < 2e-2
    assert (got_cls == O.predict(net, x, logits=ref)).mean() > 0.98
    assert np.array_equal(got_cls, O.predict(net, x, logits=got))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_xception_fused_prep_bit_identical(gpu, precision):
    net = X.build_deeplab_xception(width=0.25, middle=2, crop=97)
    x = _frames(2, 90, 97, 5)
    fused = DeepLabV3(net=net, precision=precision)
    plain = DeepLabV3(net=net, precision=precision, fuse_prep=False)
    a = fused.predict(x)
    la = fused.logits_device().cpu()
    b = plain.predict(x)
    assert torch.equal(la, plain.logits_device().cpu())
    assert np.array_equal(a, b)


@pytest.mark.parametrize("style", ["slim", "folded"])
def test_xception_from_frozen_graphdef(gpu, tmp_path, style):
    """DeepLabV3(<frozen Xception-65 DeepLabV3+ GraphDef>): the imported network on the GPU against
    the NumPy GraphDef interpreter's logits and the oracle."""
    from deeplab_graph_writer import write_deeplab_graph
    from oracle import tf_graph
    net = X.build_deeplab_xception(width=0.25, middle=2, crop=97, atrous_rates=(2, 4))
    H, W = 90, 97
    pb = tmp_path / "deeplab.pb"
    pb.write_bytes(write_deeplab_graph(net, style, H, W))
    model = DeepLabV3(str(pb), precision="fp32")
    assert isinstance(model.net, X.DeepLabXception) and S.crop_hw(model.net) == (97, 97)
    x = _frames(1, H, W, 13)
    _check_fp32(model, model.net, x, torch.float64)
    lg = np.transpose(tf_graph.run(pb.read_bytes(), {"ImageTensor": x}, "logits"), (0, 3, 1, 2))
    assert np.abs(_gpu_logits(model) - lg).max() < LOGIT_TOL


@pytest.mark.parametrize("which", ["mobilenet", "xception"])
def test_deeplab_gemm128_bit_identical(gpu, monkeypatch, which):
    """The 128 x 128 glds GEMM of the deep, wide 1x1s (K >= 256, N >= 256: the ASPP 1x1s and
    projection, Xception's pointwise layers) against the 256 x 64 register-staged one
    (BUGSEG_DL_G128=0): the same k-steps through the same MFMA in the same order -> identical
    logits and class maps, over pixel tails, 32-channel k tails (cinP 736 = 11.5 stages),
    stored-channel tails (CS 728 < cinP), output-channel tails (cout < NP), residual and per-image-bias
    epilogues."""
    if which == "mobilenet":
        net = S.build_deeplab(width=1.0, crop=97, atrous_rates=(6,))
        x = _frames(3, 97, 90, 43)
    else:
        net = X.build_deeplab_xception(width=1.0, middle=1, crop=65)   # 728 channels: cinP 736 = 11.5 stages
        x = _frames(2, 65, 60, 44)
    a_model = DeepLabV3(net=net, precision="bf16")
    a = a_model.predict(x)
    la = a_model.logits_device().cpu()
    monkeypatch.setenv("BUGSEG_DL_G128", "0")
    b_model = DeepLabV3(net=net, precision="bf16")
    b = b_model.predict(x)
    assert torch.equal(la, b_model.logits_device().cpu())
    assert np.array_equal(a, b)


# ---------------------------------------------------------------- ResNet-v1-beta backbone (deeplab_resnet.py)
@pytest.mark.parametrize("depth,units,os_,rates,B,H,W,crop", [
    (50, (1, 2, 2, 2), 16, (2, 4), 2, 60, 65, 65),
    (101, (2, 1, 3, 3), 8, (2,), 1, 65, 65, 65),
    (50, (1, 1, 1, 1), 16, (), 3, 64, 90, (64, 98)),
])
def test_resnet_fp32_small(gpu, depth, units, os_, rates, B, H, W, crop):
    """Reduced-width ResNet-v1-beta DeepLabV3 against the fp64 oracle: the 3-conv root with the fixed
    padding of its strided conv, the 3x3 s2 SAME max pool, bottleneck units with projection / identity /
    subsampled shortcuts and the ReLU after the residual add (CONV act 3), strided and atrous 3x3s
    (output stride 16 and 8, multi-grid block 4), dense atrous ASPP; an even, non-square crop."""
    net = R.build_deeplab_resnet(depth=depth, width=0.25, units=units, crop=crop, output_stride=os_, atrous_rates=rates)
    model = DeepLabV3(net=net, precision="fp32")
    assert any(int(S.field(o, "kind")) == S.OP_MAXPOOL for o in S.lower(net, B, False)[1])
    _check_fp32(model, net, _frames(B, H, W, 21 + H), torch.float64)


def test_resnet101_fp32_full_width(gpu):
    """The full ResNet-v1-101-beta DeepLabV3 (33 units, 2048 channels, ASPP 6/12/18) at a 129 crop
    against the fp32 oracle."""
    net = R.build_deeplab_resnet(depth=101, crop=129)
    model = DeepLabV3(net=net, precision="fp32")
    _check_fp32(model, net, _frames(1, 129, 120, 23), torch.float32)


def test_resnet_bf16_vs_storage_emulation(gpu):
    net = R.build_deeplab_resnet(depth=50, width=0.5, crop=129)
    model = DeepLabV3(net=net, precision="bf16")
    x = _frames(2, 129, 120, 24)
    got_cls = model.predict(x)
    got = _gpu_logits(model)
    ref = O.forward(net, x, bf16_storage=True).numpy()
    print(f"resnet bf16 mean|d| {np.abs(got - ref).mean():.2e}, class agreement {(got_cls == O.predict(net, x, logits=ref)).mean():.5f}")
    assert np.abs(got - ref).mean() < 2e-2
    assert (got_cls == O.predict(net, x, logits=ref)).mean() > 0.98
    assert np.array_equal(got_cls, O.predict(net, x, logits=got))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resnet_fused_prep_bit_identical(gpu, precision):
    net = R.build_deeplab_resnet(depth=50, width=0.25, units=(1, 1, 1, 1), crop=97)
    x = _frames(2, 90, 97, 25)
    fused = DeepLabV3(net=net, precision=precision)
    plain = DeepLabV3(net=net, precision=precision, fuse_prep=False)
    a = fused.predict(x)
    la = fused.logits_device().cpu()
    b = plain.predict(x)
    assert torch.equal(la, plain.logits_device().cpu())
    assert np.array_equal(a, b)


def test_resnet_weight_file_round_trip(gpu, tmp_path):
    """deeplab_spec.save / DeepLabV3(<.npz>) for the ResNet form: the loaded network runs to the same
    class ids."""
    net = R.build_deeplab_resnet(depth=50, width=0.25, units=(1, 1, 2, 1), crop=65)
    p = tmp_path / "resnet.npz"
    S.save(net, p)
    x = _frames(1, 65, 60, 26)
    a = DeepLabV3(net=net, precision="fp32").predict(x)
    m = DeepLabV3(str(p), precision="fp32")
    assert isinstance(m.net, R.DeepLabResNet)
    assert np.array_equal(a, m.predict(x))


def test_resnet_from_frozen_graphdef(gpu, tmp_path):
    """DeepLabV3(<frozen ResNet-v1-beta DeepLabV3 GraphDef>): the imported network on the GPU against
    the NumPy GraphDef interpreter's logits and the oracle."""
    from deeplab_graph_writer import write_deeplab_graph
    from oracle import tf_graph
    net = R.build_deeplab_resnet(depth=50, width=0.25, units=(1, 2, 2, 2), crop=97, atrous_rates=(2, 4))
    H, W = 90, 97
    pb = tmp_path / "deeplab.pb"
    pb.write_bytes(write_deeplab_graph(net, "slim", H, W))
    model = DeepLabV3(str(pb), precision="fp32")
    assert isinstance(model.net, R.DeepLabResNet) and S.crop_hw(model.net) == (97, 97)
    x = _frames(1, H, W, 27)
    _check_fp32(model, model.net, x, torch.float64)
    lg = np.transpose(tf_graph.run(pb.read_bytes(), {"ImageTensor": x}, "logits"), (0, 3, 1, 2))
    assert np.abs(_gpu_logits(model) - lg).max() < LOGIT_TOL


@pytest.mark.parametrize("ig64", ["0", "1"])
@pytest.mark.parametrize("os_,crop,rates,B", [(16, 97, (6, 12, 18), 2), (8, 65, (2,), 3)])
def test_resnet_implicit_gemm_bit_identical(gpu, monkeypatch, os_, crop, rates, B, ig64):
    """The implicit-GEMM k x k conv on the 128 x 128 glds tile (bf16 default for dense convs with
    64-channel-aligned inputs and 128-channel-aligned outputs: the root's 64 -> 128 3x3, block 2-4's
    3x3s strided / atrous / multi-grid, the ASPP atrous branches) against dl_conv_kernel
    (BUGSEG_DL_IG=0): the same (tap, 32-channel) k-steps in the same order through the same MFMA and
    epilogue -> identical logits — over pixel tails, the fixed padding of the strided 3x3, and ASPP
    rates past the feature map (taps wholly in the zero padding)."""
    net = R.build_deeplab_resnet(depth=50, units=(1, 1, 2, 1), crop=crop, output_stride=os_, atrous_rates=rates)
    x = _frames(B, crop, crop - 4, 45)
    monkeypatch.setenv("BUGSEG_DL_IG64", ig64)   # "0": the 64-channel-output convs stay on dl_conv_kernel
    ig = DeepLabV3(net=net, precision="bf16")
    a = ig.predict(x)
    la = ig.logits_device().cpu()
    monkeypatch.setenv("BUGSEG_DL_IG", "0")
    direct = DeepLabV3(net=net, precision="bf16")
    b = direct.predict(x)
    lb = direct.logits_device().cpu()
    print(f"implicit GEMM vs direct: max|d| {(la - lb).abs().max().item():.3e}")
    assert torch.equal(la, lb)
    assert np.array_equal(a, b)


def test_resnet_grouped_aspp_bit_identical(gpu, monkeypatch):
    """The ASPP's atrous branches as one grouped launch (bugseg_dl_forward's same-shape conv runs,
    dl_gemm128_group_kernel) against one launch each (BUGSEG_DL_GROUP=0): every tile runs the same
    code on its own branch's arguments -> identical logits."""
    net = R.build_deeplab_resnet(depth=50, units=(1, 1, 1, 1), crop=97, atrous_rates=(6, 12, 18))
    x = _frames(2, 97, 90, 46)
    grouped = DeepLabV3(net=net, precision="bf16")
    a = grouped.predict(x)
    la = grouped.logits_device().cpu()
    monkeypatch.setenv("BUGSEG_DL_GROUP", "0")
    single = DeepLabV3(net=net, precision="bf16")
    b = single.predict(x)
    assert torch.equal(la, single.logits_device().cpu())
    assert np.array_equal(a, b)
