"""Benchmark of the road filter, contour_noise_removal on the device.

One process, one GPU, bench.py's shape (fp32, batch 64, 480x640, synthetic.synthetic_bev, synthetic.GRID_*).
The class maps are ENET.predict_binary of synthetic.road_frames(seed=0) with the default synthetic weights.
It prints ONE JSON line:

  filter_ms            one bugseg_road_filter call on the batch (HIP events over `steps` calls, workspace
                       allocated once), and filter_us_per_frame
  kernels              per launch of the call's eight: ms, from the differences of the timed prefixes
                       [0, 1), [0, 2), ... of the sequence (Context.road_filter(ops=...))
  alg_bytes            the filter's algorithmic traffic: the u8 map read once, the u8 map written once;
                       alg_gbs what that is per second at filter_ms, hbm_frac against the 8 TB/s HBM peak
  workspace_bytes      of the call
  step_ms_off / _on    the captured pipeline step (binary=True) without and with road_filter, frames/s beside
  cpu_ms_per_frame     the NumPy / scipy restatement (tests/road_filter_ref.tree) on `cpu_frames` of the maps,
                       cpu_threads threads; the device output of those frames is checked against it
  regions_per_frame    foreground + background regions of the closed map, mean over the CPU frames
  block_noise          the same call on maps of 12 x 12 coin-flip blocks, which keep hundreds of regions through
                       the closing (the class maps above close to a single region): ms, kernels, regions, CPU ms

Run:  python bench_road_filter.py [--batch B --height H --width W --steps K --warmup W]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X spec (bench.py's constant)
OPS = ("close", "tile", "merge", "flatten", "count", "sub", "keep", "out")


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--precision", default="fp32", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--cpu-frames", type=int, default=2)
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_road_filter {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def timed_ms(fn, steps, warmup):
    """ms per call of `fn` enqueued `steps` times on the current stream, from HIP events."""
    for _ in range(max(1, warmup)):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def step_ms(replay, steps, warmup):
    """bench.py's timed loop: warm up, synchronise, `steps` replays, synchronise."""
    for _ in range(warmup):
        replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_road_filter.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    import road_filter_ref as R
    from bugcar_image_segmentation_amd import _native as N
    from bugcar_image_segmentation_amd import enet_spec, synthetic
    from bugcar_image_segmentation_amd.image_processing_utils import road_filter_params
    from bugcar_image_segmentation_amd.models import ENET
    from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline

    H, W, B = a.height, a.width, a.batch
    blocks = enet_spec.build_enet()
    frames = torch.from_numpy(synthetic.road_frames(B, H, W, seed=0)).to(dev)
    model = ENET(weights=blocks, precision=a.precision)
    log("class maps")
    seg = model.predict_device(ENET.preprocess_device(frames, N.PRE_ENGINE, model.ctx, W, H), N.OUT_BINARY_U8).clone()

    log("filter")
    ctx = N.shared_context(0)
    p = road_filter_params(H, W)
    nws = int(ctx.lib.bugseg_road_filter_workspace_bytes(ctypes.byref(p), B))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    out = torch.empty_like(seg)
    filter_ms = timed_ms(lambda: ctx.road_filter(seg, B, p, out, workspace=ws), a.steps, a.warmup)
    prefix = [0.0] + [timed_ms(lambda n=n: ctx.road_filter(seg, B, p, out, ops=(0, n), workspace=ws), a.steps, a.warmup)
                      for n in range(1, len(OPS) + 1)]
    kernels = {name: round(prefix[i + 1] - prefix[i], 4) for i, name in enumerate(OPS)}
    ctx.road_filter(seg, B, p, out, workspace=ws)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    seg_np = seg.cpu().numpy()
    alg_bytes = 2 * B * H * W
    alg_gbs = alg_bytes / (filter_ms * 1e-3) / 1e9

    # the class maps above close to one region (the synthetic weights' road specks lie closer than k): a second
    # workload with many regions that survive the closing, 12 x 12 blocks of coin flips, another draw per frame
    log("filter, block noise")
    rng = np.random.default_rng(0)
    coarse = rng.random((B, -(-H // 12), -(-W // 12))) < 0.5
    blocks_np = np.kron(coarse, np.ones((12, 12), bool))[:, :H, :W].astype(np.uint8)
    bseg = torch.from_numpy(blocks_np).to(dev)
    blocks_ms = timed_ms(lambda: ctx.road_filter(bseg, B, p, out, workspace=ws), a.steps, a.warmup)
    bprefix = [0.0] + [timed_ms(lambda n=n: ctx.road_filter(bseg, B, p, out, ops=(0, n), workspace=ws), a.steps, a.warmup)
                       for n in range(1, len(OPS) + 1)]
    torch.cuda.synchronize()
    bgot = out[0].cpu().numpy()
    ctx.road_filter(seg, B, p, out, workspace=ws)
    torch.cuda.synchronize()

    log("CPU restatement")
    from scipy import ndimage
    nc = max(1, min(a.cpu_frames, B))
    t0 = time.perf_counter()
    ref = [R.tree(seg_np[i]) for i in range(nc)]
    cpu_ms = (time.perf_counter() - t0) / nc * 1e3
    for i in range(nc):
        if not np.array_equal(ref[i], got[i]):
            raise RuntimeError(f"device output of frame {i} differs from the CPU restatement")
    regions = []
    for i in range(nc):
        c = R.close_shifts(seg_np[i], p.k)
        regions.append(ndimage.label(c, structure=R.S8)[1] + ndimage.label(~c, structure=R.S4)[1])
    t0 = time.perf_counter()
    bref = R.tree(blocks_np[0])
    blocks_cpu_ms = (time.perf_counter() - t0) * 1e3
    if not np.array_equal(bref, bgot):
        raise RuntimeError("device output of the block-noise frame differs from the CPU restatement")
    c = R.close_shifts(blocks_np[0], p.k)
    blocks_regions = ndimage.label(c, structure=R.S8)[1] + ndimage.label(~c, structure=R.S4)[1]

    log("pipeline steps")
    bev = synthetic.synthetic_bev(H, W)
    grid = (synthetic.GRID_W_M, synthetic.GRID_H_M, synthetic.CELL_M)
    steps = {}
    for on in (False, True):
        pipe = OccupancyPipeline(ENET(weights=blocks, precision=a.precision), bev, *grid, model_hw=(H, W), binary=True,
                                 road_filter=on)
        replay, _ = pipe.capture(frames)
        steps[on] = step_ms(replay, a.steps, a.warmup)
        del pipe, replay
    res = {
        "metric": "contour_noise_removal on the device: ms per batch call (synthetic road frames through predict_binary)",
        "filter_ms": round(filter_ms, 4), "filter_us_per_frame": round(filter_ms * 1e3 / B, 3),
        "kernels": kernels, "kernels_sum_ms": round(prefix[-1], 4),
        "alg_bytes": alg_bytes, "alg_gbs": round(alg_gbs, 2), "hbm_frac": round(alg_gbs / HBM_PEAK_GBS, 5),
        "workspace_bytes": nws,
        "step_ms_off": round(steps[False], 4), "step_ms_on": round(steps[True], 4),
        "fps_off": round(B / steps[False] * 1e3, 2), "fps_on": round(B / steps[True] * 1e3, 2),
        "cpu_ms_per_frame": round(cpu_ms, 2), "cpu_frames": nc, "cpu_threads": 1,
        "regions_per_frame": round(float(np.mean(regions)), 1),
        "road_fraction_in": round(float(seg_np.mean()), 4), "road_fraction_out": round(float(got.mean()), 4),
        "block_noise": {"filter_ms": round(blocks_ms, 4), "filter_us_per_frame": round(blocks_ms * 1e3 / B, 3),
                        "kernels": {name: round(bprefix[i + 1] - bprefix[i], 4) for i, name in enumerate(OPS)},
                        "regions_per_frame": int(blocks_regions), "cpu_ms_per_frame": round(blocks_cpu_ms, 2),
                        "road_fraction_out": round(float(bgot.mean()), 4)},
        "unit": "ms", "dtype": a.precision, "steps": a.steps, "warmup": a.warmup,
        "config": {"batch": B, "height": H, "width": W, "k": p.k, "y_top": p.y_top, "min_count": p.min_count},
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
