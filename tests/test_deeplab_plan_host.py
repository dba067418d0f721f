"""The DeepLab op record and plan, host side (no GPU): the executor's field tables
(csrc/deeplab_ops.h) equal deeplab_spec.OP_LAYOUT; the three lowerers produce the bytes they produced before the
fields had names; every lowered plan passes the executor's validation and the edits that must not are refused
with their text; the ASPP's atrous branches group as one launch only while they stay disjoint and out of place."""
import ctypes
import hashlib

import numpy as np
import pytest

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import deeplab_spec as S
from bugcar_image_segmentation_amd.deeplab_resnet import build_deeplab_resnet
from bugcar_image_segmentation_amd.deeplab_xception import build_deeplab_xception

# sha256(blob + ops.tobytes() + bufs.tobytes()) of the lowerers as they were when a record was written as a
# positional list (the commit before the field tables), and the op array's shape
LOWERED = {
    "mnv2_b2_bf16": ((58, 32), "486bc5b48347d78605299871ab8d75c47bd3a7c34ffce3b2729bd7bc5eb04738"),
    "mnv2_b1_fp32_fuse_dw": ((41, 32), "3d3d2c013a0d5261d8a954da6cda3de78794c007cc62b341c7169e47ee022506"),
    "mnv2_b1_fp32_no_fuse_prep": ((59, 32), "1cca827caf140a4050a688e3e501a87b7d117e69edfa6a2474e176f1fd32f6db"),
    "resnet_b2_bf16": ((31, 32), "2da013803715de45754fabda44fc0afc045dda57738fa8fcfdead84397705f50"),
    "resnet_b1_fp32": ((31, 32), "db5dad2cf5b51a49664621efbdc1b408f7da7b1f213c9e04b0c5dca0ba9deb41"),
    "xception_b2_bf16": ((149, 32), "0fdb8ceae38c516714b6b9c39de7b244dbc937a94fd5608e77c785c332f55285"),
}
KINDS = (S.OP_PREP, S.OP_CONV, S.OP_DW, S.OP_POOL, S.OP_ARGMAX, S.OP_RESIZE, S.OP_MAXPOOL)


@pytest.fixture(scope="module")
def plans():
    """name -> (blob, ops, bufs, B, bf16), lowered once and left unchanged (the tests edit copies)."""
    mn = S.build_deeplab(width=0.25, crop=65, atrous_rates=(2, 4))
    rn = build_deeplab_resnet(depth=50, width=0.25, units=(1, 1, 2, 1), crop=65)
    xc = build_deeplab_xception(width=0.25, crop=65)
    cases = {"mnv2_b2_bf16": (mn, 2, True, {}), "mnv2_b1_fp32_fuse_dw": (mn, 1, False, dict(fuse_dw=True)),
             "mnv2_b1_fp32_no_fuse_prep": (mn, 1, False, dict(fuse_prep=False)), "resnet_b2_bf16": (rn, 2, True, {}),
             "resnet_b1_fp32": (rn, 1, False, {}), "xception_b2_bf16": (xc, 2, True, {})}
    return {name: (*S.lower(net, B, bf16, **kw)[:3], B, bf16) for name, (net, B, bf16, kw) in cases.items()}


def check(plan, ops=None, bufs=None):
    blob, ops0, bufs0, B, bf16 = plan
    N.dl_check_plan(ops0 if ops is None else ops, bufs0 if bufs is None else bufs, B, 65, 65, N.BF16 if bf16 else N.FP32,
                    len(blob))


@pytest.mark.parametrize("kind", KINDS)
def test_executor_and_lowerer_agree_on_the_layout(native_lib, kind):
    assert N.dl_op_layout(kind) == S.OP_LAYOUT[kind]


def test_layout_bounds(native_lib):
    assert set(S.OP_LAYOUT) == set(KINDS)
    assert max(len(v) for v in S.OP_LAYOUT.values()) == len(S.OP_LAYOUT[S.OP_CONV]) == 31 == S.OP_FIELDS - 1
    for kind in (0, 8, 99, -1):
        with pytest.raises(ValueError, match=f"unknown op kind {kind}"):
            N.dl_op_layout(kind)
    buf = ctypes.create_string_buffer(8)
    assert native_lib.bugseg_dl_debug_op_layout(S.OP_CONV, buf, 8) == N.EINVAL      # a short buffer is not written past
    assert native_lib.bugseg_dl_debug_op_layout(S.OP_PREP, buf, 4) == 1 and buf.value == b"dst"
    assert native_lib.bugseg_dl_debug_op_layout(S.OP_PREP, buf, 3) == N.EINVAL


def test_op_takes_exactly_the_layouts_names():
    L = S.Lowering(1, False, 2)
    L.op(S.OP_ARGMAX, "argmax", 0, 0, logits=1, h=2, w=3, LCS=8, ncls=5)
    assert L.ops[-1] == [S.OP_ARGMAX, 1, 2, 3, 8, 5] + [0] * 26
    with pytest.raises(ValueError):
        L.op(S.OP_ARGMAX, "argmax", 0, 0, logits=1, h=2, w=3, LCS=8)                # a missing name
    with pytest.raises(ValueError):
        L.op(S.OP_ARGMAX, "argmax", 0, 0, logits=1, h=2, w=3, LCS=8, ncls=5, tap=0)   # an unknown one
    with pytest.raises(ValueError):
        L.op(99, "x", 0, 0)
    assert len(L.ops) == 1
    rec = np.asarray(L.ops[-1], np.int32)
    assert S.field(rec, "ncls") == 5 and S.field(rec, "kind") == S.OP_ARGMAX and S.field_pos(S.OP_CONV, "tap") == 31
    with pytest.raises(ValueError):
        S.field(rec, "tap")
    with pytest.raises(ValueError):                                                # a column needs records of one kind
        S.field(np.stack([rec, np.asarray([S.OP_PREP] + [0] * 31, np.int32)]), "h")


@pytest.mark.parametrize("name", sorted(LOWERED))
def test_lowering_unchanged(plans, name):
    blob, ops, bufs = plans[name][:3]
    shape, digest = LOWERED[name]
    assert ops.shape == shape and ops.dtype == np.int32 and bufs.dtype == np.uint64
    assert hashlib.sha256(blob + ops.tobytes() + bufs.tobytes()).hexdigest() == digest


@pytest.mark.parametrize("name", sorted(LOWERED))
def test_lowered_plans_validate(native_lib, plans, name):
    check(plans[name])


def test_validation_refuses(native_lib, plans):
    plan = plans["resnet_b2_bf16"]
    ops0, bufs0 = plan[1], plan[2]
    (mp,) = [i for i, o in enumerate(ops0) if S.field(o, "kind") == S.OP_MAXPOOL and S.field(o, "k") == 3]   # the root pool

    def edited(i, name, value):
        ops = ops0.copy()
        S.field(ops[i:i + 1], name)[:] = value
        return ops

    assert S.field(ops0[mp], "pad_t") < 3 and S.field(ops0[mp], "src") != S.field(ops0[mp], "dst")
    for name in ("pad_t", "pad_l"):
        with pytest.raises(ValueError, match=f"op {mp}: maxpool: padding covers the window"):
            check(plan, edited(mp, name, 3))
    with pytest.raises(ValueError, match=f"op {mp}: maxpool: in place"):
        check(plan, edited(mp, "dst", S.field(ops0[mp], "src")))
    ops = ops0.copy()
    ops[mp, 0] = 99
    with pytest.raises(ValueError, match=f"op {mp}: unknown op kind 99"):
        check(plan, ops)
    bufs = bufs0.copy()
    bufs[S.field(ops0[mp], "dst")] //= 2
    with pytest.raises(ValueError, match="too small"):
        check(plan, bufs=bufs)
    check(plan)                                                                    # the originals were not touched


def test_conv_groups(native_lib, plans):
    ops0 = plans["resnet_b2_bf16"][1]
    cat = [i for i, o in enumerate(ops0) if S.field(o, "kind") == S.OP_CONV and S.field(o, "dst") == 11]
    assert [(int(S.field(ops0[i], "kh")), int(S.field(ops0[i], "out_off"))) for i in cat] == [(1, 0), (3, 64), (3, 128), (3, 192)]
    a = cat[1]
    assert cat == [a - 1, a, a + 1, a + 2]
    want = [1] * len(ops0)
    want[a] = 3
    assert N.dl_plan_groups(ops0) == want
    three = ops0[a:a + 3]
    # the second branch on the first's channels: a grid holding both would race, so the first runs alone
    ops = ops0.copy()
    S.field(ops[a + 1:a + 2], "out_off")[:] = S.field(ops0[a], "out_off")
    assert N.dl_plan_groups(ops)[a:a + 3] == [1, 2, 1]
    # in place: never grouped
    ops = ops0.copy()
    S.field(ops[a:a + 3], "dst")[:] = S.field(three, "src")
    assert N.dl_plan_groups(ops) == [1] * len(ops0)
