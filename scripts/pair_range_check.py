"""Why the paired fp32 C64 bottleneck cannot take its exponents from a bound (CPU, oracle activations; not product code).

bneck_pair_kernels.hip runs blocks A and B of a pair (1.1+1.2, 1.3+1.4; 4.1+4.2 is shown too) in one launch, so
the tensor between them, y, is never measured before block B needs its range. The candidate rule this script
settles: a launch-uniform exponent from a rigorous bound,

    By = max(1, |s_out|) * (n3 * B1 + c3 + max|x|),    B1 = n2 * (n1 * max|x| + c1) + c2   (block A's chain)
    sy = 0 while By < 2^15, else the exponent that brings By to [2^14, 2^15)

with block B's chain started from By where the unpaired launch starts from the measured max |y|. Per pair and
input it prints block A's exponents, By against the measured max |y|, and block B's exponents both ways. On
the default weights By is ~800 x max |y| and block B's bounds leave the f16 window (B0 1e5 - 5e5, B1 2e6 - 1e7): its
exponents come out non-zero, which would change the default-weight results. Hence the kernel speculates on
exponent 0 and the guarded launches behind it check the measured maxima. The "B unpaired" column is
what that check evaluates: all 0 here, so the pair's result stands. Exit status 1 says the bound rule fails.

    python scripts/pair_range_check.py [--undamped]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bugcar_image_segmentation_amd import enet_spec, synthetic  # noqa: E402
from oracle import enet_oracle as eo  # noqa: E402

f32 = np.float32
EMAX = 40


def fold(u):
    s = np.asarray(u.gamma, np.float64) / np.sqrt(np.asarray(u.var, np.float64) + float(u.eps))
    b = (np.asarray(u.b, np.float64) - np.asarray(u.mean, np.float64)) * s + np.asarray(u.beta, np.float64)
    return np.asarray(u.w, np.float64) * s[:, None, None, None], b


def row_bound(u):
    """enet_weights.cpp range_stats + row_bound: (n, c, sw)."""
    w, b = fold(u)
    rabs = np.abs(w).reshape(w.shape[0], -1).sum(1).astype(f32)
    rbias = np.abs(b.astype(f32))
    rslope = np.maximum(f32(1), np.abs(np.asarray(u.slope, f32)))
    n = f32((rabs * rslope).max()) * f32(1.0001)
    c = f32((rbias * rslope).max()) * f32(1.0001)
    return n, c, weight_exp(float(np.abs(w).max()))


def log2f(m):
    return math.frexp(float(m))[1] - 1


def clamp(e):
    return max(-EMAX, min(EMAX, e))


def weight_exp(m):
    if not (m > 0) or not math.isfinite(m):
        return 0
    l = log2f(m)
    return 0 if -2 <= l < 15 else clamp(14 - l)


def exp_meas(m):
    if not (m > 0) or not math.isfinite(m):
        return 0
    l = log2f(m)
    return 0 if -2 <= l < 15 else clamp(14 - l)


def exp_bound(B, p):
    p = max(-2 * EMAX, min(2 * EMAX, p))
    if not (B < math.inf):
        return -EMAX
    if not (B > 0):
        return p
    l = log2f(B)
    return p if 3 <= l + p < 15 else clamp(14 - l)


def exp_y(B):
    """the candidate rule for y"""
    if not (B < math.inf):
        return -EMAX
    if not (B > 0):
        return 0
    l = log2f(B)
    return 0 if l < 15 else clamp(14 - l)


def chain(units, amx, sx):
    """bneck_range<false>: -> (exponents dict, B1)."""
    (n1, c1, sw1), (n2, c2, sw2), (_, _, sw3) = (row_bound(u) for u in units)
    e1 = sx + sw1
    B0 = f32(n1 * f32(amx) + c1)
    s0 = exp_bound(B0, e1)
    e2 = s0 + sw2
    B1 = f32(n2 * B0 + c2)
    s1 = exp_bound(B1, e2)
    e3 = s1 + sw3
    return dict(sx=sx, e1=e1, s0=s0, e2=e2, s1=s1, e3=e3), B0, B1


def inputs(name, H, W):
    if name == "road":
        return synthetic.road_frames(2, H, W, seed=5)
    return synthetic.uniform_frames(2, H, W, seed=6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--undamped", action="store_true")
    a = p.parse_args()
    blocks = enet_spec.build_enet(res_gamma=(0.5, 1.5)) if a.undamped else enet_spec.build_enet()
    pairs = (("regular1_1", "regular1_2"), ("regular1_3", "regular1_4"), ("regular4_1", "regular4_2"))
    ok = True
    for kind, H, W in (("uniform", 480, 640), ("road", 480, 640), ("road", 160, 208), ("road", 72, 104), ("road", 64, 96)):
        bgr = inputs(kind, H, W)
        x = np.moveaxis((bgr[..., ::-1] / 256.0 - eo.IMAGE_MEAN) / eo.IMAGE_STD, -1, 1)
        h = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32)
        amax_in, pools = {}, {}
        for i, b in enumerate(blocks):
            amax_in[b.name] = float(h.abs().max())
            if b.type == "initial":
                u = b.units[0]
                main = F.conv2d(h, eo._t(u.w, torch.float32), eo._t(u.b, torch.float32), stride=2, padding=1)
                k = b.attrs["pool_k"]
                y = torch.cat([main, F.max_pool2d(h, k, stride=2, padding=(k - 1) // 2)], 1)
                e = b.extra
                y = eo._bn(y, np.concatenate([u.mean, e["pool_mean"]]), np.concatenate([u.var, e["pool_var"]]),
                           np.concatenate([u.gamma, e["pool_gamma"]]), np.concatenate([u.beta, e["pool_beta"]]), u.eps, torch.float32)
                h = eo._prelu(y, np.concatenate([u.slope, e["pool_slope"]]), torch.float32)
            elif b.type == "down":
                main, idx = F.max_pool2d(h, 2, stride=2, return_indices=True)
                pools[i] = (idx, h.shape[2:])
                ext = h
                for u in b.units:
                    ext = eo._unit(ext, u, torch.float32)
                main = torch.cat([main, main.new_zeros((main.shape[0], ext.shape[1] - main.shape[1]) + main.shape[2:])], 1)
                h = eo._prelu(main + ext, b.extra["out_slope"], torch.float32)
            elif b.type == "regular":
                ext = h
                for u in b.units:
                    ext = eo._unit(ext, u, torch.float32)
                h = eo._prelu(h + ext, b.extra["out_slope"], torch.float32)
            elif b.type == "up":
                idx, size = pools[b.attrs["pool_ref"]]
                main = eo._unit(h, b.units[0], torch.float32, act=False)
                main = F.max_unpool2d(main, idx, 2, stride=2, output_size=size)
                ext = h
                for u in b.units[1:]:
                    ext = eo._unit(ext, u, torch.float32)
                h = eo._prelu(main + ext, b.extra["out_slope"], torch.float32)
            else:
                break
        by_name = {b.name: b for b in blocks}
        for na, nb in pairs:
            A, Bk = by_name[na], by_name[nb]
            amx, amy = amax_in[na], amax_in[nb]
            ea, _, B1 = chain(A.units, amx, exp_meas(amx))
            n3, c3, _ = row_bound(A.units[-1])
            so = f32(max(1.0, float(np.abs(A.extra["out_slope"]).max())))
            By = f32(so * f32(f32(n3 * B1 + c3) + f32(amx))) * f32(1.0001)
            sy = exp_y(By)
            eb_pair, B0p, B1p = chain(Bk.units, By, sy)
            eb_meas, B0m, B1m = chain(Bk.units, amy, exp_meas(amy))
            zero = not any(ea.values()) and not any(eb_pair.values()) and not any(eb_meas.values())
            ok = ok and zero
            print(f"{kind:7s} {H}x{W} {na}+{nb[-3:]}: max|x| {amx:8.3f} A {list(ea.values())}  max|y| {amy:8.3f} By {By:10.2f} "
                  f"sy {sy}  B paired {list(eb_pair.values())} (B0 {B0p:9.1f} B1 {B1p:10.1f})  "
                  f"B unpaired {list(eb_meas.values())} (B0 {B0m:8.1f} B1 {B1m:9.1f})  {'all 0' if zero else 'NON-ZERO'}")
    print("every exponent 0" if ok else "some exponent is non-zero")
    return 0 if ok or a.undamped else 1


if __name__ == "__main__":
    sys.exit(main())
