"""Evaluator.update_frames (evaluate.py): a model's forward to u8 classes feeding the confusion
kernel on the device, for the ENet with the seeded synthetic weights at 64 x 96 and for the reduced-width
DeepLabV3 of tests/test_gpu_deeplab.py (width 0.25, crop 65 x 97) with a 3-class table. The matrix must be,
bit for bit, the one confusion_device gives on the model's own class maps."""
import gc

import numpy as np
import pytest
import torch

import evaluate_ref as R
from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import deeplab_spec as S
from bugcar_image_segmentation_amd import evaluate as E
from bugcar_image_segmentation_amd import synthetic
from bugcar_image_segmentation_amd.models import ENET, DeepLabV3, class_lut3

pytestmark = pytest.mark.gpu

EH, EW = 64, 96
DH, DW, DCLS = 65, 97, 21
_MODELS = {}


def enet(blocks):
    if "enet" not in _MODELS:
        _MODELS["enet"] = ENET(weights=blocks, precision="fp32")
    return _MODELS["enet"]


def deeplab():
    if "dl" not in _MODELS:
        m = DeepLabV3(net=S.build_deeplab(width=0.25, crop=(DH, DW), num_classes=DCLS), precision="fp32")
        m.class_lut = class_lut3(DCLS, range(0, DCLS, 3), range(1, DCLS, 3))
        _MODELS["dl"] = m
    return _MODELS["dl"]


def own_classes(gpu, model, frames, hw):
    """The model's own u8 class maps of device frames already at its size, through its existing entry."""
    B = frames.shape[0]
    if isinstance(model, DeepLabV3):
        return model.predict_classes_device(frames, bgr=True)
    seg = torch.empty((B, *hw), dtype=torch.uint8, device=gpu)
    model.ctx.forward_bgr(frames, B, hw[0], hw[1], N.OUT_CLASS15_U8, seg)
    return seg


def labels_for(B, hw, C, seed):
    return np.random.default_rng(seed).integers(0, C + 1, (B, *hw), dtype=np.uint8)


@pytest.mark.parametrize("which", ["enet", "deeplab"])
def test_update_frames_equals_confusion_of_the_models_own_classes(gpu, blocks, which):
    model, hw, C = (enet(blocks), (EH, EW), 15) if which == "enet" else (deeplab(), (DH, DW), 3)
    B = 2
    frames = torch.from_numpy(synthetic.road_frames(B, *hw, seed=7)).to(gpu)
    labels = torch.from_numpy(labels_for(B, hw, C, 1)).to(gpu)
    ev = E.Evaluator(C)
    ev.update_frames(model, frames, labels, model_hw=hw)
    seg = own_classes(gpu, model, frames, hw)
    want = E.confusion_device(seg, labels, C)
    assert torch.equal(ev.acc, want)
    assert np.array_equal(ev.acc.cpu().numpy(), R.accumulator(seg.cpu().numpy(), labels.cpu().numpy(), C))
    assert int(ev.acc.sum()) == labels.numel() and ev.skipped() > 0          # the labels hold the byte C: skipped
    # labels equal to the model's own prediction: a diagonal matrix, every figure 1
    ev.reset()
    ev.update_frames(model, frames, seg.clone(), model_hw=hw)
    m = ev.confusion()
    assert m.sum() == labels.numel() and not (m - np.diag(np.diag(m))).any() and ev.skipped() == 0
    got = ev.metrics()
    assert got["miou"] == 1.0 and got["pixel_accuracy"] == 1.0 and got["fw_iou"] == pytest.approx(1.0, rel=1e-12)
    # host frames and host labels are copied up and give the same
    ev2 = E.Evaluator(C)
    ev2.update_frames(model, frames.cpu().numpy(), labels.cpu().numpy(), model_hw=hw)
    assert torch.equal(ev2.acc, want)


@pytest.mark.parametrize("which", ["enet", "deeplab"])
def test_frames_of_another_size_go_through_the_resize(gpu, blocks, which):
    model, hw, C = (enet(blocks), (EH, EW), 15) if which == "enet" else (deeplab(), (DH, DW), 3)
    B, big_hw = 2, (100, 150)
    big = torch.from_numpy(synthetic.road_frames(B, *big_hw, seed=9)).to(gpu)
    small = torch.empty((B, *hw, 3), dtype=torch.uint8, device=gpu)
    N.shared_context(gpu.index).preprocess(big, B, big_hw[0], big_hw[1], hw[0], hw[1], N.PRE_BGR_U8, small)
    seg = own_classes(gpu, model, small, hw)
    # labels at the frames' size: the class maps, at the model's size, are read by the nearest rule
    labels = torch.from_numpy(labels_for(B, big_hw, C, 2)).to(gpu)
    ev = E.Evaluator(C)
    ev.update_frames(model, big, labels, model_hw=hw)
    assert torch.equal(ev.acc, E.confusion_device(seg, labels, C))
    assert np.array_equal(ev.acc.cpu().numpy(), R.accumulator(seg.cpu().numpy(), labels.cpu().numpy(), C))


@pytest.mark.parametrize("which", ["enet", "deeplab"])
def test_update_frames_under_capture_copies_no_class_map_to_the_host(gpu, blocks, which):
    """A host copy, a synchronisation or an allocation outside the graph's pool inside a capture is an error,
    so a captured update_frames shows that the class maps go from the forward to the kernel on the device."""
    model, hw, C = (enet(blocks), (EH, EW), 15) if which == "enet" else (deeplab(), (DH, DW), 3)
    B = 2
    frames = torch.from_numpy(synthetic.road_frames(B, *hw, seed=11)).to(gpu)
    labels = torch.from_numpy(labels_for(B, hw, C, 3)).to(gpu)
    ev = E.Evaluator(C)
    ev.update_frames(model, frames, labels, model_hw=hw)            # outside: buffers, and the DeepLab's plan
    torch.cuda.synchronize(gpu)
    once = ev.acc.clone()
    assert int(once.sum()) == labels.numel()
    gc.collect()
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            ev.update_frames(model, frames, labels, model_hw=hw)
    finally:
        gc.enable()
    torch.cuda.synchronize(gpu)
    assert torch.equal(ev.acc, once)                                # capturing ran nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize(gpu)
    assert torch.equal(ev.acc, 3 * once)


def test_refusals(gpu, blocks):
    bare = DeepLabV3(net=S.build_deeplab(width=0.25, crop=(DH, DW), num_classes=DCLS), precision="fp32")
    frames = torch.zeros((1, DH, DW, 3), dtype=torch.uint8, device=gpu)
    labels = torch.zeros((1, DH, DW), dtype=torch.uint8, device=gpu)
    ev = E.Evaluator(3)
    with pytest.raises(ValueError, match="needs its class_lut set"):
        ev.update_frames(bare, frames, labels)
    with pytest.raises(ValueError, match="ENET or a DeepLabV3"):
        ev.update_frames(object(), frames, labels)
    with pytest.raises(ValueError):
        ev.update_frames(enet(blocks), frames[..., :2], labels, model_hw=(EH, EW))
    torch.cuda.synchronize(gpu)
    assert not ev.confusion().any() and ev.skipped() == 0
