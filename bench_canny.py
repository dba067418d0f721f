"""Benchmark of canny on the device (image_processing_utils.py:95-105's cv2.Canny).

One process, one GPU, batch 64, thresholds 50 / 150, two inputs:
  frames   480x640 grey road scenes (synthetic.road_frames(seed=0), the mean of the three channels)
  grids    the occupancy grids of those scenes' three-level maps under the bench calibration
           (synthetic.synthetic_bev, synthetic.GRID_*: 200x200), int8 read as uint8, as create_skeleton reads them
It prints ONE JSON line and writes the same record to --out (profiles/canny.json). Per input:

  call        one bugseg_canny call on the batch, workspace allocated once. Timing: HIP events around a window of
              back-to-back calls, at least --steps of them and as many as make the window --window-ms long;
              --repeats windows per figure, taken in turn with the other figures' windows. ms is the median
              window's time per call, ms_min and ms_max the spread, calls_per_window the window's size;
              us_per_frame; bytes = the algorithmic traffic (the input read once, the output written once);
              gbs = bytes per second at the median; hbm_frac against the 8 TB/s HBM peak, device_copy_frac and
              copy_frac against the two copies below
  nms, hyst   launch 0 alone and launches 1-4 alone (bugseg_debug_canny_stage 0 and 1; the hysteresis reads the
              map that launch 0 gave), each against the same algorithmic bytes. halves_sum_ms is the sum of
              their medians: close to the call's, not equal (each half is a run of its own launches)
  device_copy the device's copy rate: a device-to-device copy of 512 MiB, twice the Infinity Cache, so it
              runs at the rate of HBM; timed the same way in the same run
  copy        a device-to-device copy of the input to the output (the same bytes as the call's), timed the same
              way. Both buffers fit the Infinity Cache, so this is no HBM rate; launch_bound is true where
              the copy takes under 10 us, about what enqueueing one launch takes: then the figure, and
              copy_frac with it, measure launch overhead, not a copy rate
  edge_frac, candidate_frac   the share of edge pixels in the result and of candidates in the map
  checked_frames              device frames compared with the NumPy restatement (tests/canny_ref.py)

There is no threshold: nothing exists to compare against.

Run:  python bench_canny.py [--batch B --height H --width W --steps K --warmup W --repeats R --window-ms MS --out PATH]
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
LAUNCH_BOUND_MS = 0.010        # a copy quicker than this is timed by its launch, not by the bytes it moves
DEVICE_COPY_BYTES = 1 << 29    # each buffer of the large copy: twice the 256 MiB Infinity Cache


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=7, help="timed windows per figure: median, min and max are reported")
    p.add_argument("--window-ms", type=float, default=250.0, help="least length of one timed window")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--check-frames", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "canny.json"))
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.batch < 1 or a.repeats < 1 or not a.window_ms >= 0:
        p.error("--steps, --batch and --repeats must be at least 1, --warmup and --window-ms at least 0")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_canny {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def window_ms(fn, steps):
    """ms per call of `fn` enqueued `steps` times on the current stream, from HIP events."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def timed(fns, a):
    """{name: (ms per call in each of a.repeats windows, calls per window)}. Every fn is warmed up, then its
    window is sized from a first window of a.steps calls so that it lasts at least a.window_ms; the repeats go
    round the fns in turn, so that a drift of the machine touches all of them alike."""
    steps = {}
    for name, fn in fns.items():
        for _ in range(max(1, a.warmup)):
            fn()
        first = window_ms(fn, a.steps)
        steps[name] = max(a.steps, int(np.ceil(a.window_ms / max(first, 1e-6))))
    ms = {name: [] for name in fns}
    for _ in range(a.repeats):
        for name, fn in fns.items():
            ms[name].append(window_ms(fn, steps[name]))
    return {name: (ms[name], steps[name]) for name in fns}


def spread(ms):
    return {"ms": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def measure(ctx, x, big, a, R, canny_params):
    B, h, w = x.shape
    p = canny_params(h, w, 50, 150)
    nws = int(ctx.lib.bugseg_canny_workspace_bytes(ctypes.byref(p), B))
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    mp = torch.empty_like(x)
    ctx.canny(x, B, p, mp, stage=0, workspace=ws)
    t = timed({"call": lambda: ctx.canny(x, B, p, out, workspace=ws),
               "nms": lambda: ctx.canny(x, B, p, out, stage=0, workspace=ws),
               "hyst": lambda: ctx.canny(mp, B, p, out, stage=1, workspace=ws),
               "copy": lambda: out.copy_(x),
               "device_copy": lambda: big[1].copy_(big[0])}, a)
    ctx.canny(x, B, p, out, workspace=ws)
    torch.cuda.synchronize()
    nc = max(1, min(a.check_frames, B))
    got, src = out[:nc].cpu().numpy(), x[:nc].cpu().numpy()
    for i in range(nc):
        if not np.array_equal(got[i], R.canny(src[i], 50, 150)):
            raise RuntimeError(f"device output of frame {i} at {h}x{w} differs from the NumPy restatement")
    nbytes = 2 * B * h * w
    copy = spread(t["copy"][0])
    copy_gbs = nbytes / (copy["ms"] * 1e-3) / 1e9
    dev = spread(t["device_copy"][0])
    dev_gbs = 2 * big[0].numel() / (dev["ms"] * 1e-3) / 1e9
    launch_bound = copy["ms"] < LAUNCH_BOUND_MS

    def rate(name):
        r = spread(t[name][0])
        gbs = nbytes / (r["ms"] * 1e-3) / 1e9
        r.update({"calls_per_window": t[name][1], "us_per_frame": round(r["ms"] * 1e3 / B, 3), "bytes": nbytes,
                  "gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4),
                  "device_copy_frac": round(gbs / dev_gbs, 4), "copy_frac": round(gbs / copy_gbs, 4)})
        return r

    copy.update({"calls_per_window": t["copy"][1], "bytes": nbytes, "gbs": round(copy_gbs, 1),
                 "launch_bound": launch_bound})
    dev.update({"calls_per_window": t["device_copy"][1], "bytes": 2 * big[0].numel(), "gbs": round(dev_gbs, 1)})
    call, nms, hyst = rate("call"), rate("nms"), rate("hyst")
    return {"shape": [B, h, w], "call": call, "nms": nms, "hyst": hyst,
            "halves_sum_ms": round(nms["ms"] + hyst["ms"], 4), "copy": copy, "device_copy": dev,
            "workspace_bytes": nws, "edge_frac": round(float((out == 255).float().mean()), 5),
            "candidate_frac": round(float((mp != 1).float().mean()), 5), "checked_frames": nc}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_canny.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    import canny_ref as R
    from bugcar_image_segmentation_amd import _native as N
    from bugcar_image_segmentation_amd import synthetic
    from bugcar_image_segmentation_amd.image_processing_utils import canny_params

    H, W, B = a.height, a.width, a.batch
    grey = synthetic.road_frames(B, H, W, seed=0).astype(np.uint16).sum(axis=3) // 3
    frames = torch.from_numpy(grey.astype(np.uint8)).to(dev)
    bev = synthetic.synthetic_bev(H, W)
    levels = (frames // 86).contiguous()                      # three-level class maps
    grids = bev.create_occupancy_grid_device(levels, synthetic.GRID_W_M, synthetic.GRID_H_M, synthetic.CELL_M)
    grids = grids.contiguous().view(torch.uint8)
    big = torch.zeros((2, DEVICE_COPY_BYTES), dtype=torch.uint8, device=dev)
    ctx = N.shared_context(0)
    res = {"metric": "canny on the device: ms per batch call, thresholds 50 / 150", "unit": "ms"}
    for name, x in (("frames", frames), ("grids", grids)):
        log(f"{name}: {tuple(x.shape)}")
        res[name] = measure(ctx, x, big, a, R, canny_params)
    res.update({"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "window_ms": a.window_ms,
                "launch_bound_ms": LAUNCH_BOUND_MS, "hbm_peak_gbs": HBM_PEAK_GBS,
                "config": {"batch": B, "height": H, "width": W, "low": 50, "high": 150}})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
