"""The ENet context's weights and plan as values that change hands whole, on N.Context directly, in
fp32 at B = 1, 64 x 64: a refused weight blob keeps the loaded model and its plan; a re-plan that fails after the old
arena was retired leaves no plan (never the old ops on freed memory), and the next forward plans again; a new plan
starts without the old one's last forward. Class maps are compared byte for byte; each case has a context of its own."""
import dataclasses

import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import enet_spec, synthetic

pytestmark = pytest.mark.gpu
H = W = 64
OUT = N.OUT_CLASS15_U8


@pytest.fixture(scope="module")
def blob(blocks):
    return enet_spec.serialize(blocks)


def _context(gpu, blob):
    ctx = N.Context(gpu.index, N.FP32)
    ctx.load_weights(blob)
    return ctx


def _frames(B, gpu):
    return torch.from_numpy(synthetic.uniform_frames(B, H, W, seed=21)).to(gpu)


def _classes(ctx, x):
    seg = torch.full(x.shape[:3], 255, dtype=torch.uint8, device=x.device)      # (no class id)
    ctx.forward_bgr(x, x.shape[0], H, W, OUT, seg)
    torch.cuda.synchronize()
    return seg.cpu().numpy()


def _estate(call, text=None):
    with pytest.raises(N.BugsegError) as e:
        call()
    assert e.value.code == N.ESTATE
    assert text is None or text in str(e.value)


def _no_plan(ctx):
    """plan_op, launch_op and the pair plan refuse as before any forward: nothing of an old plan is shown or launched."""
    _estate(lambda: ctx.plan_op(1, H, W, 0), "no forward has run at these dimensions")
    _estate(lambda: ctx.launch_op(1, H, W, 0), "no forward has run at these dimensions")
    _estate(ctx.pair_plan)


def test_refused_blob_keeps_the_model(gpu, blocks, blob):
    ctx = _context(gpu, blob)
    x = _frames(1, gpu)
    a = _classes(ctx, x)
    ncls = ctx.num_classes
    assert ncls == enet_spec.NUM_CLASSES
    up = next(i for i, b in enumerate(blocks) if b.type == "up")
    bad_ref = list(blocks)
    bad_ref[up] = dataclasses.replace(blocks[up], attrs=dict(blocks[up].attrs, pool_ref=2))   # a regular block
    refused = [(blob[:-1], "weight blob: "),                                 # cut short: parse_blob refuses it
               (enet_spec.serialize(blocks[:-1]), "model must end in fullconv"),   # these two parse, and do not pack
               (enet_spec.serialize(bad_ref), "up block malformed")]
    for bad, text in refused:
        with pytest.raises(N.BugsegError, match=text) as e:
            ctx.load_weights(bad)
        assert e.value.code == N.EFORMAT
        assert ctx.num_classes == ncls
        assert ctx.plan_op(1, H, W, 0)[0] == "init"                          # the plan is still in force
        assert np.array_equal(_classes(ctx, x), a)
    ctx.close()


def test_failed_replan_leaves_no_plan(gpu, blob):
    ctx = _context(gpu, blob)
    x = _frames(2, gpu)
    a = _classes(ctx, x[:1])
    # fp32, B = 32768: the initial block's output is exactly 2^31 bytes, refused after the fill pass; the arena of
    # about 8 GiB is allocated and freed within the call (a card short of memory refuses a step earlier)
    with pytest.raises(ValueError, match="batch too large for 32-bit tensor offsets|hipMalloc of the activation arena failed"):
        ctx.plan_info(32768, H, W, OUT, True)
    _no_plan(ctx)
    assert np.array_equal(_classes(ctx, x[:1]), a)
    _classes(ctx, x)                                                         # re-plans still work: to B = 2 and back
    assert np.array_equal(_classes(ctx, x[:1]), a)
    ctx.close()


def test_arena_that_cannot_be_allocated(gpu, blob):
    ctx = _context(gpu, blob)
    x = _frames(1, gpu)
    a = _classes(ctx, x)
    with pytest.raises(ValueError, match="hipMalloc of the activation arena failed"):
        ctx.plan_info(2 ** 21, H, W, OUT, True)                              # hundreds of terabytes: nothing is allocated
    _no_plan(ctx)
    assert np.array_equal(_classes(ctx, x), a)
    ctx.close()


def test_new_plan_forgets_the_last_forward(gpu, blob):
    ctx = _context(gpu, blob)
    x = _frames(1, gpu)                                                      # (launch_op reads the last forward's frames again)
    _classes(ctx, x)
    ctx.launch_op(1, H, W, 0)                                                # the plan has a forward: an op can be issued alone
    torch.cuda.synchronize()
    ctx.plan_info(2, H, W, OUT, True)
    _estate(lambda: ctx.launch_op(2, H, W, 0), "no forward has run at these dimensions")   # none has bound the new plan
    _estate(lambda: ctx.launch_op(1, H, W, 0), "no forward has run at these dimensions")
    ctx.close()
