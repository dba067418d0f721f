"""The DeepLab context's plan as one value, on N.DeepLabContext directly: a set_plan whose arena
cannot be allocated leaves no plan (every entry refuses as on a fresh context, nothing is launched), a new plan
starts without the old one's last forward, and a captured forward keeps its arena and weights across a re-plan."""
import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import deeplab_spec as S

pytestmark = pytest.mark.gpu
CROP, H, W = 65, 33, 40


@pytest.fixture(scope="module")
def lowered():
    """(blob, {B: (ops, bufs)}) of the reduced MobileNetV2 net in fp32; one blob serves both batch sizes."""
    net = S.build_deeplab(width=0.25, crop=CROP, atrous_rates=(2, 4))
    blob, ops1, bufs1, _ = S.lower(net, 1, False)
    blob2, ops2, bufs2, _ = S.lower(net, 2, False)
    assert blob == blob2 and len(bufs1) == 11
    return blob, {1: (ops1, bufs1), 2: (ops2, bufs2)}


def _frames(B, seed, gpu):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(gpu)


def _context(lowered, gpu, B):
    ctx = N.DeepLabContext(gpu.index, N.FP32)
    ctx.load_weights(lowered[0])
    ctx.set_plan(*lowered[1][B], B, CROP, CROP)
    return ctx


def _classes(ctx, x):
    seg = torch.empty(x.shape[:3], dtype=torch.uint8, device=x.device)
    ctx.forward_classes(x, False, x.shape[0], H, W, seg)
    torch.cuda.synchronize()
    return seg.cpu().numpy()


def _estate(call):
    with pytest.raises(N.BugsegError) as e:
        call()
    assert e.value.code == N.ESTATE


def test_failed_set_plan_leaves_no_plan(gpu, lowered):
    ops, bufs = lowered[1][1]
    ctx = _context(lowered, gpu, 1)
    x = _frames(1, 11, gpu)
    r0 = _classes(ctx, x)
    # one more buffer, unused, of the validator's own cap: a valid plan whose arena no card holds
    with pytest.raises(N.BugsegError) as e:
        ctx.set_plan(ops, np.append(bufs, np.uint64(1 << 40)), 1, CROP, CROP)
    assert e.value.code == N.ENOMEM
    seg = torch.empty((1, H, W), dtype=torch.uint8, device=gpu)
    out = torch.empty((1, H, W), dtype=torch.int64, device=gpu)
    _estate(lambda: ctx.forward(x, 1, H, W, out))
    _estate(lambda: ctx.forward_classes(x, False, 1, H, W, seg))
    _estate(lambda: ctx.classes_from_logits(1, H, W, seg))
    with pytest.raises(ValueError):
        ctx.launch_op(0)
    with pytest.raises(ValueError):
        ctx.read_buffer(7, torch.empty(64, dtype=torch.float32, device=gpu))
    ctx.set_plan(ops, bufs, 1, CROP, CROP)
    assert np.array_equal(_classes(ctx, x), r0)
    ctx.close()


def test_replan_forgets_last_forward(gpu, lowered):
    ctx = _context(lowered, gpu, 1)
    x1, x2 = _frames(1, 12, gpu), _frames(2, 13, gpu)      # (launch_op reads the last forward's frames again)
    _classes(ctx, x1)
    ctx.launch_op(0)                                       # the plan has a forward: its ops can be issued alone
    ctx.set_plan(*lowered[1][2], 2, CROP, CROP)
    seg = torch.empty((2, H, W), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="no such op / no forward yet"):
        ctx.launch_op(0)
    _estate(lambda: ctx.classes_from_logits(2, H, W, seg))
    want = _classes(ctx, x2)
    ctx.launch_op(0)
    ctx.classes_from_logits(2, H, W, seg)
    torch.cuda.synchronize()
    assert np.array_equal(seg.cpu().numpy(), want)
    ctx.close()


def test_captured_forward_survives_replan(gpu, lowered):
    ctx = _context(lowered, gpu, 1)
    x = _frames(1, 14, gpu)
    seg = torch.empty((1, H, W), dtype=torch.uint8, device=gpu)
    ctx.forward_classes(x, False, 1, H, W, seg)            # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # (captures on a side stream of its own)
        ctx.forward_classes(x, False, 1, H, W, seg)
    ctx.set_plan(*lowered[1][2], 2, CROP, CROP)            # the graph's arena is replaced, not freed
    x2 = _frames(2, 15, gpu)
    got2 = _classes(ctx, x2)
    ref = _context(lowered, gpu, 2)                        # a second context, eager throughout
    assert np.array_equal(got2, _classes(ref, x2))
    ref.set_plan(*lowered[1][1], 1, CROP, CROP)
    x.copy_(_frames(1, 16, gpu))
    want = _classes(ref, x)
    seg.fill_(255)                                         # no class id: the replay must write every byte
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(seg.cpu().numpy(), want)
    del g
    ctx.close()
    ref.close()
