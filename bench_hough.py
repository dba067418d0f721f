"""Benchmark of hough_lines, warp_image and the straight-line check on the device.

One process, one GPU, batch 64, rho 1, theta pi / 180, Canny thresholds 50 / 150. Inputs:
  frames   Canny edges of 480x640 grey road scenes (synthetic.road_frames(seed=0), the mean of the three channels)
  warped   Canny edges of the same scenes (BGR) warped to 1000x1000 under the bench calibration
           (synthetic.synthetic_bev) and turned grey: what the line check hands to the transform
It prints ONE JSON line and writes the same record to --out (profiles/hough.json).

  hough.<input>   call: one bugseg_hough_lines call on the batch (threshold a quarter of the shorter side,
                  max_lines 64), workspace allocated once; vote: stage 0 alone (list the pixels, vote, write the
                  accumulators: the product writes none, so this is an upper bound of its first two launches);
                  select: stage 1 alone (peaks and selection on those accumulators read from memory).
                  Timing: HIP events around a window of back-to-back calls, at least --steps of them and as many
                  as make the window --window-ms long; --repeats windows per figure, taken in turn with the other
                  figures' windows. ms is the median window's time per call, ms_min and ms_max the spread.
                  bytes = the algorithmic traffic: the edge image read once, lines, counts and peaks written once;
                  edge_frac, peaks_mean and votes (pixels x angles, the LDS atomic adds of one call without the
                  halo angles) describe the load
  warp.<form>     one bugseg_bev_warp_image call, 64 BGR frames of 480x640 to 1000x1000: bgr (3 channels out),
                  gray (1 byte out), one (1 channel in and out); bytes = frames read once + result written once
  line_check      straight_lines_device on the 64 BGR frames: warp to grey, Canny, Hough; bytes = frames read
                  once + lines, counts and peaks written once
  device_copy     a device-to-device copy of 512 MiB, twice the Infinity Cache: the device's copy rate in the same run
  checked_frames  device results compared with the NumPy restatements (tests/hough_ref.py, tests/canny_ref.py)

There is no threshold: nothing earlier exists to compare against.

Run:  python bench_hough.py [--batch B --steps K --warmup W --repeats R --window-ms MS --out PATH]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X spec (bench.py's constant)
DEVICE_COPY_BYTES = 1 << 29    # each buffer of the large copy: twice the 256 MiB Infinity Cache
RHO, THETA, MAX_LINES = 1.0, math.pi / 180, 64


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=7, help="timed windows per figure: median, min and max are reported")
    p.add_argument("--window-ms", type=float, default=250.0, help="least length of one timed window")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--check-frames", type=int, default=1)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hough.json"))
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.batch < 1 or a.repeats < 1 or not a.window_ms >= 0:
        p.error("--steps, --batch and --repeats must be at least 1, --warmup and --window-ms at least 0")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_hough {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


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


def figure(t, name, nbytes, B, dev_gbs=None):
    ms = t[name][0]
    r = {"ms": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
         "calls_per_window": t[name][1], "us_per_frame": round(float(np.median(ms)) * 1e3 / B, 3), "bytes": int(nbytes)}
    gbs = nbytes / (r["ms"] * 1e-3) / 1e9
    r.update({"gbs": round(gbs, 2), "hbm_frac": round(gbs / HBM_PEAK_GBS, 5)})
    if dev_gbs:
        r["device_copy_frac"] = round(gbs / dev_gbs, 5)
    return r


def measure_hough(ctx, ipu, edges, big, a, R):
    B, h, w = edges.shape
    thr = min(h, w) // 4
    p = ipu.hough_params(h, w, RHO, THETA, thr, MAX_LINES)
    trig = ipu.hough_trig_device(edges.device, p)
    nws = int(ctx.lib.bugseg_hough_workspace_bytes(ctypes.byref(p), B))
    ws = torch.empty(nws, dtype=torch.uint8, device=edges.device)
    lines = torch.empty((B, MAX_LINES, 2), dtype=torch.float32, device=edges.device)
    counts = torch.empty((B,), dtype=torch.int32, device=edges.device)
    peaks = torch.empty((B,), dtype=torch.int32, device=edges.device)
    acc = torch.empty((B, p.numangle + 2, p.numrho + 2), dtype=torch.int32, device=edges.device)
    ctx.hough(edges, B, p, trig, None, None, None, stage=0, acc=acc, workspace=ws)
    t = timed({"call": lambda: ctx.hough(edges, B, p, trig, lines, counts, peaks, workspace=ws),
               "vote": lambda: ctx.hough(edges, B, p, trig, None, None, None, stage=0, acc=acc, workspace=ws),
               "select": lambda: ctx.hough(None, B, p, None, lines, counts, peaks, stage=1, acc=acc, workspace=ws),
               "device_copy": lambda: big[1].copy_(big[0])}, a)
    ctx.hough(edges, B, p, trig, lines, counts, peaks, workspace=ws)
    torch.cuda.synchronize()
    nc = max(0, min(a.check_frames, B))
    for i in range(nc):
        want = R.hough(edges[i].cpu().numpy(), RHO, THETA, thr, MAX_LINES)
        got = lines[i].cpu().numpy()
        if int(counts[i]) != want[1] or int(peaks[i]) != want[2] or not np.array_equal(got.view(np.uint32), want[0].view(np.uint32)):
            raise RuntimeError(f"device lines of frame {i} at {h}x{w} differ from the NumPy restatement")
    nbytes = B * h * w + B * (MAX_LINES * 8 + 8)
    dev_ms = float(np.median(t["device_copy"][0]))
    dev_gbs = 2 * big[0].numel() / (dev_ms * 1e-3) / 1e9
    set_px = float((edges != 0).sum())
    return {"shape": [B, h, w], "threshold": thr, "max_lines": MAX_LINES, "numangle": p.numangle, "numrho": p.numrho,
            "call": figure(t, "call", nbytes, B, dev_gbs), "vote": figure(t, "vote", nbytes, B, dev_gbs),
            "select": figure(t, "select", nbytes, B, dev_gbs),
            "accumulator_bytes": int(acc.numel() * 4), "workspace_bytes": nws,
            "device_copy": figure(t, "device_copy", 2 * big[0].numel(), B),
            "edge_frac": round(set_px / (B * h * w), 5), "votes": int(set_px * p.numangle),
            "peaks_mean": round(float(peaks.float().mean()), 1), "counts_mean": round(float(counts.float().mean()), 1),
            "checked_frames": nc}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_hough.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    import canny_ref
    import hough_ref as R
    from bugcar_image_segmentation_amd import _native as N
    from bugcar_image_segmentation_amd import image_processing_utils as ipu
    from bugcar_image_segmentation_amd import line_test, synthetic

    H, W, B = 480, 640, a.batch
    bgr_np = synthetic.road_frames(B, H, W, seed=0)
    bgr = torch.from_numpy(bgr_np).to(dev)
    grey = torch.from_numpy((bgr_np.astype(np.uint16).sum(axis=3) // 3).astype(np.uint8)).to(dev)
    bev = synthetic.synthetic_bev(H, W)
    big = torch.zeros((2, DEVICE_COPY_BYTES), dtype=torch.uint8, device=dev)
    ctx = N.shared_context(0)
    res = {"metric": "hough_lines, warp_image and the line check on the device: ms per batch call", "unit": "ms"}

    edges = ipu.canny_device(grey, 50, 150)
    warped_gray = bev.warp_image_device(bgr, gray=True)
    warped_edges = ipu.canny_device(warped_gray, 50, 150)
    res["hough"] = {}
    for name, e in (("frames", edges), ("warped", warped_edges)):
        log(f"hough {name}: {tuple(e.shape)}")
        res["hough"][name] = measure_hough(ctx, ipu, e, big, a, R)

    log("warp_image")
    oh, ow = int(bev.after_warp_height), int(bev.after_warp_width)
    out3 = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=dev)
    out1 = torch.empty((B, oh, ow), dtype=torch.uint8, device=dev)
    t = timed({"bgr": lambda: bev.warp_image_device(bgr, out=out3),
               "gray": lambda: bev.warp_image_device(bgr, gray=True, out=out1),
               "one": lambda: bev.warp_image_device(grey, out=out1),
               "line_check": lambda: line_test.straight_lines_device(bev, bgr),
               "device_copy": lambda: big[1].copy_(big[0])}, a)
    dev_gbs = 2 * big[0].numel() / (float(np.median(t["device_copy"][0])) * 1e-3) / 1e9
    nin3, nin1, nout = B * H * W * 3, B * H * W, B * oh * ow
    res["warp"] = {"shape_in": [B, H, W], "shape_out": [B, oh, ow],
                   "bgr": figure(t, "bgr", nin3 + 3 * nout, B, dev_gbs), "gray": figure(t, "gray", nin3 + nout, B, dev_gbs),
                   "one": figure(t, "one", nin1 + nout, B, dev_gbs)}
    res["line_check"] = figure(t, "line_check", nin3 + B * (64 * 8 + 8), B, dev_gbs)
    res["line_check"].update({"threshold": line_test.default_threshold(bev), "max_lines": 64})
    res["device_copy"] = figure(t, "device_copy", 2 * big[0].numel(), B)
    nc = max(0, min(a.check_frames, B))
    g3 = bev.warp_image_device(bgr[:max(nc, 1)])
    torch.cuda.synchronize()
    for i in range(nc):
        M, size = bev._bev_matrix, (ow, oh)
        if not np.array_equal(g3[i].cpu().numpy(), R.warp_image(bgr_np[i], M, size)) or \
                not np.array_equal(warped_gray[i].cpu().numpy(), R.warp_image(bgr_np[i], M, size, gray=True)):
            raise RuntimeError(f"warped frame {i} differs from the NumPy restatement")
        if not np.array_equal(warped_edges[i].cpu().numpy(), canny_ref.canny(warped_gray[i].cpu().numpy(), 50, 150)):
            raise RuntimeError(f"edges of warped frame {i} differ from the NumPy restatement")
    res["warp"]["checked_frames"] = nc
    rep = line_test.straight_line_report(*line_test.straight_lines_device(bev, bgr)[:2])
    res["line_check"]["spread_median"] = round(float(np.median([r["spread"] for r in rep if r["spread"] is not None] or [0.0])), 5)
    res.update({"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "window_ms": a.window_ms,
                "hbm_peak_gbs": HBM_PEAK_GBS,
                "config": {"batch": B, "height": H, "width": W, "rho": RHO, "theta": THETA, "canny": [50, 150]}})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
