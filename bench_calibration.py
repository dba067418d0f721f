"""Benchmark of the calibration tile finder on the device: find_tile_device per launch and as a
whole, and the two-pass host form find_tile, at B = 64 frames of 480 x 640 BGR.

It prints ONE JSON line and writes the same record to --out (profiles/calibration.json).

  launches.<name>  one launch of bugseg_find_quad alone (bugseg_debug_quad_stage) on a workspace a whole call has filled
  call             one bugseg_find_quad call on the batch: two memsets and twelve launches
  find_tile        calibration.find_tile on device frames: the call above, a read-back, the host's line fits, an
                   upload, bugseg_quad_moments (launches 0..5 and 11 again), a read-back, the line fits again
  device_copy      a copy between two 512 MiB device buffers, for the rate this machine copies at today

There is no OpenCV here to compare the times with. Instead every launch stands beside `copy_ms`: the time its
compulsory bytes (what it must read and write at least once, from the shapes and the foreground count) would take
at COPY_RATE_GBS, the rate a float4 copy reaches on an MI355X (6.3 TB/s of its 8 TB/s), and `copy_frac` = copy_ms / ms.
`far_from_copy_rate` names the launches below FAR_FRAC of it. No bar is set: calibration is a one-shot.

Every step (launches, call, find_tile) runs in a child process of its own under --step-timeout seconds; after a step
that fails or runs out of time nothing more is started.

Run:  python bench_calibration.py [--batch B --steps K --warmup W --repeats R --window-ms MS --step-timeout S --out PATH]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X spec (bench.py's constant)
COPY_RATE_GBS = 6300.0         # what a float4 copy reaches of it
FAR_FRAC = 0.10
DEVICE_COPY_BYTES = 1 << 29    # each buffer of the large copy: twice the 256 MiB Infinity Cache
H, W = 480, 640
STEPS = ("launches", "call", "find_tile")
LAUNCHES = ("grey", "otsu", "tile", "merge", "flatten", "choose", "c0", "c1", "c2", "c3", "order", "moments")


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5, help="timed windows per figure: median, min and max are reported")
    p.add_argument("--window-ms", type=float, default=100.0, help="least length of one timed window")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--check-frames", type=int, default=2)
    p.add_argument("--step-timeout", type=float, default=150.0, help="seconds one step may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration.json"))
    p.add_argument("--step", choices=STEPS, help=argparse.SUPPRESS)
    p.add_argument("--step-out", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.batch < 1 or a.repeats < 1 or not a.window_ms >= 0 or not a.step_timeout > 0:
        p.error("--steps, --batch and --repeats must be at least 1, --warmup and --window-ms at least 0, --step-timeout positive")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_calibration {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def frames_np(B):
    """B BGR frames: the two camera-sized quads of tests/quad_ref.py under four noise seeds, repeated."""
    import quad_ref as R
    base = [R.rendered(name, seed, True) for seed in range(4) for name in ("camera", "foreshortened")]
    return np.stack([base[i % len(base)] for i in range(B)])


def compulsory_bytes(B, n, ch, fg, border):
    """Per launch: the bytes it must move at least once. fg: foreground pixels of the batch (they alone carry labels
    and counters); border: pixels on a labelling tile's top row or side columns."""
    g, lab = B * n, 4 * fg
    return {"grey": B * n * (ch + 1) + B * 1024, "otsu": B * 1024 + B * 8, "tile": g + 2 * lab, "merge": 5 * border,
            "flatten": g + 2 * lab, "choose": g + lab, "c0": g + lab, "c1": g + lab, "c2": g + lab, "c3": g + lab,
            "order": B * (80 + 48), "moments": g + lab + B * 192}


def step(a):
    """One step, in this process (a child of main's)."""
    import torch
    import quad_ref as R
    from bugcar_image_segmentation_amd import _native as N
    from bugcar_image_segmentation_amd import calibration as C

    if not torch.cuda.is_available():
        raise RuntimeError("bench_calibration.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B = a.batch
    fr = frames_np(B)
    x = torch.from_numpy(fr).to(dev)
    ctx = N.shared_context(0)
    p = C.quad_params(H, W)
    nws = int(ctx.lib.bugseg_quad_workspace_bytes(ctypes.byref(p), B))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    o = [torch.empty((B,), **i32) for _ in range(4)] + [torch.empty((B, 4, 2), **i32), torch.empty((B, 4, 6), dtype=torch.int64, device=dev)]
    big = torch.zeros((2, DEVICE_COPY_BYTES), dtype=torch.uint8, device=dev)

    def window_ms(fn, steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(steps):
            fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) / steps

    def timed(fns):
        steps = {}
        for name, fn in fns.items():
            for _ in range(max(1, a.warmup)):
                fn()
            steps[name] = max(a.steps, int(np.ceil(a.window_ms / max(window_ms(fn, a.steps), 1e-6))))
        ms = {name: [] for name in fns}
        for _ in range(a.repeats):
            for name, fn in fns.items():
                ms[name].append(window_ms(fn, steps[name]))
        return {name: (ms[name], steps[name]) for name in fns}

    def figure(t, name, nbytes):
        ms = t[name][0]
        med = float(np.median(ms))
        copy_ms = nbytes / (COPY_RATE_GBS * 1e9) * 1e3
        return {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls_per_window": t[name][1],
                "us_per_frame": round(med * 1e3 / B, 3), "bytes": int(nbytes), "copy_ms": round(copy_ms, 5),
                "copy_frac": round(copy_ms / med, 4)}

    whole = lambda: ctx.find_quad(x, B, p, *o, workspace=ws)
    whole()
    torch.cuda.synchronize()
    grey = R.grey(fr[:8])
    thr = o[1][:8].cpu().numpy()
    fg = int(sum(int((g > t).sum()) for g, t in zip(grey, thr)) * (B / min(B, 8)))
    yy, xx = np.mgrid[0:H, 0:W]
    border = B * int(((yy % 16 == 0) | (xx % 64 == 0) | (xx % 64 == 63)).sum())
    nb = compulsory_bytes(B, H * W, 3, fg, border)
    res = {}
    if a.step == "launches":
        fns = {name: (lambda k=k: ctx.find_quad(x, B, p, *o, stage=k, workspace=ws)) for k, name in enumerate(LAUNCHES)}
        fns["device_copy"] = lambda: big[1].copy_(big[0])
        t = timed(fns)
        res["launches"] = {name: figure(t, name, nb[name]) for name in LAUNCHES}
        res["launches_sum_ms"] = round(sum(v["ms"] for v in res["launches"].values()), 4)
        res["far_from_copy_rate"] = [n for n in LAUNCHES if res["launches"][n]["copy_frac"] < FAR_FRAC]
        res["device_copy"] = figure(t, "device_copy", 2 * DEVICE_COPY_BYTES)
        res["device_copy"]["gbs"] = round(2 * DEVICE_COPY_BYTES / (res["device_copy"]["ms"] * 1e-3) / 1e9, 1)
    elif a.step == "call":
        t = timed({"call": whole})
        res["call"] = figure(t, "call", sum(nb.values()))
        res["call"]["workspace_bytes"] = nws
        res["foreground_frac"] = round(fg / (B * H * W), 5)
        whole()
        torch.cuda.synchronize()
        nc = max(0, min(a.check_frames, B))
        for i in range(nc):
            r = R.find_tile(fr[i], R.params(H, W))
            got = [t_[i].cpu().numpy() for t_ in o]
            want = [r["status0"], r["threshold"], r["area"], r["root"], r["corners"], r["moments"]]
            if not all(np.array_equal(g, w_) for g, w_ in zip(got, want)):
                raise RuntimeError(f"device outputs of frame {i} differ from the NumPy restatement")
        res["checked_frames"] = nc
        res["status_ok"] = int((o[0] == 0).sum())
    else:
        t = timed({"find_tile": lambda: C.find_tile(x)})
        res["find_tile"] = figure(t, "find_tile", 2 * sum(nb.values()))
        found = C.find_tile(x)
        res["find_tile"]["status_ok"] = int((found["status"] == C.OK).sum())
        truth = {name: np.array(R.QUADS[name][1]) for name in ("camera", "foreshortened")}
        err = [R.match_error(found["corners"][i], truth[("camera", "foreshortened")[i % 2]])[1] for i in range(B) if found["status"][i] == C.OK]
        res["find_tile"]["worst_corner_px"] = round(max(err), 4) if err else None
    with open(a.step_out, "w") as f:
        json.dump(res, f)


def main():
    a = parse()
    if a.step:
        return step(a)
    res = {"metric": "find_quad on the device and the two-pass find_tile: ms per batch call", "unit": "ms"}
    with tempfile.TemporaryDirectory() as tmp:
        for name in STEPS:
            out = os.path.join(tmp, name + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", out, "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--window-ms", str(a.window_ms), "--batch", str(a.batch),
                   "--check-frames", str(a.check_frames)]
            log(f"step {name} (limit {a.step_timeout:.0f} s)")
            try:
                rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"bench_calibration: step {name} ran out of its {a.step_timeout:.0f} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"bench_calibration: step {name} ended with status {rc}; nothing more is started")
            with open(out) as f:
                res.update(json.load(f))
    res.update({"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "window_ms": a.window_ms,
                "hbm_peak_gbs": HBM_PEAK_GBS, "copy_rate_gbs": COPY_RATE_GBS, "far_frac": FAR_FRAC,
                "config": {"batch": a.batch, "height": H, "width": W, "channels": 3, "band": [3, 2]}})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
