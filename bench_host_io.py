"""Benchmark of the host-to-host flow: NumPy BGR frames in, NumPy int8 occupancy grids out.

bench.py times the step on frames already resident in HBM. The reference's loop is host to host
(models.py:42-44 feeds a NumPy frame, bev.py:244-246 returns a NumPy grid), so this script measures
what moving the frames onto the card and the grids back costs when hostio.HostStream runs the copies
beside the step. One process, one GPU, bench.py's configuration and defaults (fp32, batch 64,
480x640, synthetic.synthetic_bev, synthetic.GRID_*, uniform_frames(seed=0)). It prints ONE JSON line:

  device_fps        the captured step on device-resident frames, timed as bench.py's main loop times it
  host_fps          the same step fed through HostStream(depth=2) from pre-filled pinned slots
                    (next_frames, put, get in steady state: `steps` consecutive step completions)
  host_fps_staged   the same with put(frames=pageable_array): the host memcpy into the pinned slot included
  copy_in_ms, copy_out_ms, step_ms   per step, from HIP events, each leg run alone on its stream
  host_over_device  host_fps / device_fps
  latency_b1        at B = 1, medians of the timed calls: device_ms (captured step, device-resident frame,
                    synchronised per call), host_stream_ms (host BGR -> host grid through a depth-1
                    HostStream), host_api_ms (the drop-in ENET.preprocess -> predict -> create_occupancy_grid)

Run:  python bench_host_io.py [--batch B --height H --width W --steps K --warmup W]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--precision", default="fp32", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--streams", type=int, default=1, help="the pipeline's own frame-shard streams (bench.py --streams)")
    p.add_argument("--depth", type=int, default=2, help="slots of the timed HostStream")
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_host_io {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def device_fps(replay, B, steps, warmup):
    """bench.py's timed loop: warm up, synchronise, `steps` replays, synchronise."""
    for _ in range(warmup):
        replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        replay()
    torch.cuda.synchronize()
    return B * steps / (time.perf_counter() - t0)


def stream_fps(hs, steps, warmup, staged=None):
    """Steady state of the ring: it is primed with `depth` steps, then every iteration fetches the
    oldest step and puts a new one. The clock runs from the return of the last warm-up fetch to the
    return of the fetch `steps` later, so it spans `steps` step completions with the ring full
    throughout; the ring is drained afterwards."""
    def put():
        if staged is None:
            hs.next_frames()                   # the pre-filled slot (waits for its last copy-in, as a writer would)
            hs.put()
        else:
            hs.put(staged)
    for _ in range(hs.depth):
        put()
    for _ in range(max(1, warmup)):
        hs.get()
        put()
    t0 = time.perf_counter()
    for _ in range(steps):
        hs.get()
        put()
    el = time.perf_counter() - t0
    while hs.outstanding:
        hs.get()
    return hs.batch * steps / el


def leg_ms(stream, fn, reps):
    """ms per call of `fn` enqueued `reps` times on `stream` with nothing else running."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        fn()
        ev[0].record(stream)
        for _ in range(reps):
            fn()
        ev[1].record(stream)
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def median_ms(fn, iters):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def latency_b1(blocks, precision, bev, grid, H, W, frame_np, dev, iters):
    """One camera frame per call (the reference's loop shape, models.py:94), three ways."""
    from bugcar_image_segmentation_amd.models import ENET
    from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline
    model = ENET(weights=blocks, precision=precision)
    pipe = OccupancyPipeline(model, bev, *grid, model_hw=(H, W))
    f = torch.from_numpy(frame_np).to(dev)
    replay, _ = pipe.capture(f)

    def device():
        replay()
        torch.cuda.synchronize()
    device_ms = median_ms(device, iters)
    with pipe.host_stream(1, depth=1) as hs:
        def host_stream():
            hs.put(frame_np)
            hs.get()
        host_stream_ms = median_ms(host_stream, iters)
    # the drop-in modules as the reference's loop calls them, at this frame size
    enet = type("ENETAtFrameSize", (ENET,), {"INPUT_WIDTH": W, "INPUT_HEIGHT": H})
    api = enet(weights=blocks, precision=precision)

    def host_api():
        seg = api.predict(enet.preprocess(frame_np[0]))
        bev.create_occupancy_grid(seg[0], *grid)
    host_api_ms = median_ms(host_api, iters)
    return {"device_ms": round(device_ms, 4), "host_stream_ms": round(host_stream_ms, 4),
            "host_api_ms": round(host_api_ms, 4), "iters": iters, "frame": f"{H}x{W}", "dtype": precision}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_host_io.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    from bugcar_image_segmentation_amd import enet_spec, synthetic
    from bugcar_image_segmentation_amd.models import ENET
    from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline

    H, W, B = a.height, a.width, a.batch
    blocks = enet_spec.build_enet()
    model = ENET(weights=blocks, precision=a.precision)
    bev = synthetic.synthetic_bev(H, W)
    grid = (synthetic.GRID_W_M, synthetic.GRID_H_M, synthetic.CELL_M)
    pipe = OccupancyPipeline(model, bev, *grid, model_hw=(H, W), streams=a.streams)
    frames_np = synthetic.uniform_frames(B, H, W, seed=0)

    log("device-resident step")
    frames = torch.from_numpy(frames_np).to(dev)
    replay, grids = pipe.capture(frames)
    dfps = device_fps(replay, B, a.steps, a.warmup)
    want = grids.cpu().numpy()

    log("host stream")
    reps = max(3, min(20, a.steps))
    with pipe.host_stream(B, depth=a.depth) as hs:
        for _ in range(hs.depth):                                  # pre-fill every pinned slot
            np.copyto(hs.next_frames(), frames_np)
            hs.put()
        for _ in range(hs.depth):
            if not np.array_equal(hs.get(), want):
                raise RuntimeError("host stream grids differ from the device-resident step's")
        hfps = stream_fps(hs, a.steps, a.warmup)
        log("host stream, staged")
        sfps = stream_fps(hs, a.steps, a.warmup, staged=frames_np)
        log("legs alone")
        copy_in = leg_ms(hs._cin, lambda: hs._dev_frames[0].copy_(hs._pin_frames[0], non_blocking=True), reps)
        copy_out = leg_ms(hs._cout, lambda: hs._pin_grids[0].copy_(hs._dev_grids[0], non_blocking=True), reps)
        step = leg_ms(hs._compute, hs._steps[0], reps)
        torch.cuda.synchronize()
        frame_bytes, grid_bytes = hs._pin_frames[0].numel(), hs._pin_grids[0].numel()
    del frames, replay, grids

    log("batch-1 latency")
    lat = latency_b1(blocks, a.precision, bev, grid, H, W, frames_np[:1], dev, max(3, min(100, 5 * a.steps)))

    res = {
        "metric": "frames/sec ENet segmentation -> BEV occupancy grid, host frames in, host grids out (synthetic)",
        "device_fps": round(dfps, 2), "host_fps": round(hfps, 2), "host_fps_staged": round(sfps, 2),
        "copy_in_ms": round(copy_in, 4), "copy_out_ms": round(copy_out, 4), "step_ms": round(step, 4),
        "host_over_device": round(hfps / dfps, 4),
        "latency_b1": lat,
        "unit": "frames/s", "dtype": a.precision, "steps": a.steps, "warmup": a.warmup,
        "config": {"batch": B, "height": H, "width": W, "depth": a.depth, "streams_per_gpu": a.streams,
                   "frame_bytes_per_step": frame_bytes, "grid_bytes_per_step": grid_bytes,
                   "copy_in_gbs_alone": round(frame_bytes / (copy_in * 1e-3) / 1e9, 2),
                   "copy_out_gbs_alone": round(grid_bytes / (copy_out * 1e-3) / 1e9, 2)},
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
