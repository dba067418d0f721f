"""Benchmark of clahe on the device (image_processing_utils.py:46-61).

One process, one GPU, bench.py's shape (batch 64, 480x640, synthetic.synthetic_bev, synthetic.GRID_*). The
frames are synthetic.road_frames(seed=0) at 35 % brightness (dusk). It prints ONE JSON line and writes the
same record to --out (profiles/clahe.json):

  call_ms              one bugseg_clahe_bgr call on the batch (HIP events over `steps` calls, workspace
                       allocated once), and call_us_per_frame
  luts_ms, apply_ms    launch 1 and launch 2 alone (bugseg_debug_clahe_stage 3 and 4), each with
                       bytes     its compulsory traffic: launch 1 reads the frames once and writes the tile
                                 tables; launch 2 reads the frames and the tile tables once and writes the frames
                       gbs       what that is per second at its time, hbm_frac against the 8 TB/s HBM peak
  lab_ms, bgr_ms       the colour stages alone (stages 0 and 2: read and write the frames once)
  step_ms_off / _on    the captured pipeline step without and with clahe=True, `rounds` alternating
                       measurements each (the medians; step_ms_*_all holds every one), frames/s beside, and
                       step_slowdown = on / off
  checked_frames       device frames compared with the NumPy restatement (tests/clahe_ref.py)

Run:  python bench_clahe.py [--batch B --height H --width W --steps K --warmup W --rounds R --out PATH]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X spec (bench.py's constant)


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--pipe-steps", type=int, default=30)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--precision", default="fp32", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--check-frames", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "clahe.json"))
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.pipe_steps < 1 or a.rounds < 1:
        p.error("--steps, --pipe-steps and --rounds must be at least 1 and --warmup at least 0")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_clahe {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


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
        raise RuntimeError("bench_clahe.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    import clahe_ref as R
    from bugcar_image_segmentation_amd import _native as N
    from bugcar_image_segmentation_amd import enet_spec, synthetic
    from bugcar_image_segmentation_amd.image_processing_utils import clahe_params
    from bugcar_image_segmentation_amd.models import ENET
    from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline

    H, W, B = a.height, a.width, a.batch
    frames_np = (synthetic.road_frames(B, H, W, seed=0).astype(np.float64) * 0.35).astype(np.uint8)
    frames = torch.from_numpy(frames_np).to(dev)

    log("the call and its launches")
    ctx = N.shared_context(0)
    p = clahe_params(H, W)
    nws = int(ctx.lib.bugseg_clahe_workspace_bytes(ctypes.byref(p), B))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    out = torch.empty_like(frames)
    call_ms = timed_ms(lambda: ctx.clahe(frames, B, p, out, workspace=ws), a.steps, a.warmup)
    luts_ms = timed_ms(lambda: ctx.clahe(frames, B, p, None, stage=3, workspace=ws), a.steps, a.warmup)
    apply_ms = timed_ms(lambda: ctx.clahe(frames, B, p, out, stage=4, workspace=ws), a.steps, a.warmup)
    lab_ms = timed_ms(lambda: ctx.clahe(frames, B, p, out, stage=0), a.steps, a.warmup)
    bgr_ms = timed_ms(lambda: ctx.clahe(frames, B, p, out, stage=2), a.steps, a.warmup)
    ctx.clahe(frames, B, p, out, workspace=ws)
    torch.cuda.synchronize()
    nc = max(1, min(a.check_frames, B))
    got = out[:nc].cpu().numpy()
    for i in range(nc):
        if not np.array_equal(got[i], R.clahe(frames_np[i])):
            raise RuntimeError(f"device output of frame {i} differs from the NumPy restatement")
    nframes = B * H * W * 3
    luts_bytes, apply_bytes = nframes + nws, 2 * nframes + nws

    def rate(nbytes, ms):
        gbs = nbytes / (ms * 1e-3) / 1e9
        return {"ms": round(ms, 4), "bytes": nbytes, "gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}

    log("pipeline steps")
    blocks = enet_spec.build_enet()
    bev = synthetic.synthetic_bev(H, W)
    grid = (synthetic.GRID_W_M, synthetic.GRID_H_M, synthetic.CELL_M)
    replays = {}
    for on in (False, True):
        pipe = OccupancyPipeline(ENET(weights=blocks, precision=a.precision), bev, *grid, model_hw=(H, W), clahe=on)
        replays[on] = (pipe,) + tuple(pipe.capture(frames))
    steps = {False: [], True: []}
    for _ in range(a.rounds):                      # alternating, so that a drift of the machine hits both alike
        for on in (False, True):
            steps[on].append(step_ms(replays[on][1], a.pipe_steps, 5))
    off, on_ = statistics.median(steps[False]), statistics.median(steps[True])
    res = {
        "metric": "clahe on the device: ms per batch call (synthetic road frames at 35 % brightness)",
        "call_ms": round(call_ms, 4), "call_us_per_frame": round(call_ms * 1e3 / B, 3),
        "luts": rate(luts_bytes, luts_ms), "apply": rate(apply_bytes, apply_ms),
        "launches_sum_ms": round(luts_ms + apply_ms, 4),
        "lab_ms": round(lab_ms, 4), "bgr_ms": round(bgr_ms, 4),
        "workspace_bytes": nws, "table_bytes": 34388,
        "step_ms_off": round(off, 4), "step_ms_on": round(on_, 4), "step_slowdown": round(on_ / off, 4),
        "step_ms_off_all": [round(v, 4) for v in steps[False]], "step_ms_on_all": [round(v, 4) for v in steps[True]],
        "fps_off": round(B / off * 1e3, 2), "fps_on": round(B / on_ * 1e3, 2),
        "checked_frames": nc,
        "unit": "ms", "dtype": a.precision, "steps": a.steps, "warmup": a.warmup, "pipe_steps": a.pipe_steps,
        "rounds": a.rounds,
        "config": {"batch": B, "height": H, "width": W, "tiles_x": p.tiles_x, "tiles_y": p.tiles_y,
                   "clip_limit": p.clip_limit},
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
