"""Benchmark of the rolling local map: B = 64 grids of 200 x 200 cells fused into windows of
512 x 512 and 1024 x 1024 cells along a curved trajectory.

It prints ONE JSON line and writes the same record to --out (profiles/local_map.json).

Per window size:
  fuse            one bugseg_map_fuse launch on a record already on the device, frame culling on: the launches of
                  a captured graph of GRAPH_LAUNCHES of them, so that the device and not the host sets the pace
  fuse_no_cull    the same with culling off: every workgroup walks all B frames
  fuse_call       LocalMap.fuse called eagerly, back to back: the launch or the host's call, whichever is slower
  update          LocalMap.update: the host's pose record, its pinned copy and transfer, then the launch
  replay          set_poses and the replay of a captured launch
  device_copy     a copy between two 512 MiB device buffers, for the rate this machine copies at in this run

There is no reference routine to compare the times with. Instead every figure stands beside `copy_ms`: the time its
compulsory bytes (the grids, the record and the table read once, the state read and written once, the payload
written once) would take at the copy rate this run measured, and `copy_frac` = copy_ms / ms. No bar is set.

Every window size runs in a child process of its own under --step-timeout seconds; after a step that fails or runs
out of time nothing more is started. The payload and the state of both launches are compared with each other, and
at 512 x 512 with the NumPy restatement (tests/map_ref.py), before anything is timed.

Run:  python bench_local_map.py [--batch B --steps K --warmup W --repeats R --window-ms MS --step-timeout S --out PATH]
"""
from __future__ import annotations

import argparse
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
DEVICE_COPY_BYTES = 1 << 29    # each buffer of the large copy: twice the 256 MiB Infinity Cache
GRID = (200, 200)
CELL_M = 0.05
SIZES = (512, 1024)
GRAPH_LAUNCHES = 20
CHECK_AGAINST_REF = 512        # the restatement is run at this size only (it takes seconds per megacell)


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5, help="timed windows per figure: median, min and max are reported")
    p.add_argument("--window-ms", type=float, default=100.0, help="least length of one timed window")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--step-timeout", type=float, default=150.0, help="seconds one step may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map.json"))
    p.add_argument("--step", type=int, choices=SIZES, help=argparse.SUPPRESS)
    p.add_argument("--step-out", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or not 1 <= a.batch <= 4096 or a.repeats < 1 or not a.window_ms >= 0 or not a.step_timeout > 0:
        p.error("--steps and --repeats must be at least 1, --batch 1..4096, --warmup and --window-ms at least 0, --step-timeout positive")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_local_map {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def trajectory(B):
    """B poses 0.15 m apart on a left-hand arc of 10 m radius, heading along it: 9.6 m and 55 degrees at B = 64."""
    s = 0.15 * np.arange(B)
    yaw = s / 10.0
    return np.stack([10.0 * np.sin(yaw), 10.0 * (1.0 - np.cos(yaw)), yaw], axis=1)


def grids_np(B):
    rng = np.random.default_rng(25)
    return rng.choice(np.array([-1, 0, 100], np.int8), size=(B,) + GRID, p=(0.3, 0.5, 0.2))


def step(a):
    """One window size, in this process (a child of main's)."""
    import torch
    import map_ref as R
    from bugcar_image_segmentation_amd import mapping as M

    if not torch.cuda.is_available():
        raise RuntimeError("bench_local_map.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, size = a.batch, (a.step, a.step)
    poses, g_np = trajectory(B), grids_np(B)
    grids = torch.from_numpy(g_np).to(dev)
    maps = {name: M.LocalMap(size, CELL_M, GRID, cull=cull) for name, cull in (("fuse", True), ("fuse_no_cull", False))}
    big = torch.zeros((2, DEVICE_COPY_BYTES), dtype=torch.uint8, device=dev)

    # what is timed is first shown to be right: two updates, the second of which keeps what the first stored
    got = {}
    for name, lm in maps.items():
        lm.update(grids, poses[: B // 2].repeat(2, axis=0))
        got[name] = (lm.update(grids, poses).cpu().numpy(), lm.state().cpu().numpy())
    if not all(np.array_equal(x, y) for x, y in zip(got["fuse"], got["fuse_no_cull"])):
        raise RuntimeError("the launch with culling and the one without give different maps")
    checked = False
    if a.step == CHECK_AGAINST_REF:
        cfg, prev, origin = R.config(GRID), None, None
        for ps in (poses[: B // 2].repeat(2, axis=0), poses):
            rec, origin = M.pose_record(ps, size, CELL_M, origin, prev is None)
            prev, payload = R.fuse_np(prev, rec, g_np, size, cfg)
        if not (np.array_equal(got["fuse"][0], payload) and np.array_equal(got["fuse"][1], prev)):
            raise RuntimeError("the device's map differs from the NumPy restatement")
        checked = True
    observed = float((got["fuse"][1] != M.UNOBSERVED).mean())

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

    # the launches alone re-read the record the last update sent: same window, nothing fresh, the steady state
    def launches(lm):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(GRAPH_LAUNCHES):
                lm.fuse(grids)
        return g.replay

    fns = {name: launches(lm) for name, lm in maps.items()}
    per_call = {name: GRAPH_LAUNCHES for name in fns}
    fns["fuse_call"] = lambda: maps["fuse"].fuse(grids)
    fns["update"] = lambda: maps["fuse"].update(grids, poses)
    replay = maps["fuse"].capture(grids)

    def set_and_replay():
        maps["fuse"].set_poses(poses)
        replay()

    fns["replay"] = set_and_replay
    fns["device_copy"] = lambda: big[1].copy_(big[0])
    t = timed(fns)
    copy_ms_all = float(np.median(t["device_copy"][0]))
    copy_gbs = 2 * DEVICE_COPY_BYTES / (copy_ms_all * 1e-3) / 1e9
    cells = size[0] * size[1]
    nbytes = B * GRID[0] * GRID[1] + 8 * (M.RECORD_HEADER + M.RECORD_FRAME * B) + 551 + 5 * cells

    def figure(name):
        ms = [v / per_call.get(name, 1) for v in t[name][0]]
        med = float(np.median(ms))
        copy_ms = nbytes / (copy_gbs * 1e9) * 1e3
        return {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "launches_per_window": t[name][1] * per_call.get(name, 1),
                "us_per_grid": round(med * 1e3 / B, 3), "copy_ms": round(copy_ms, 5), "copy_frac": round(copy_ms / med, 4)}

    res = {name: figure(name) for name in ("fuse", "fuse_no_cull", "fuse_call", "update", "replay")}
    res.update({"bytes": int(nbytes), "device_copy_gbs": round(copy_gbs, 1), "observed_frac": round(observed, 4),
                "checked_against_restatement": checked, "cull_speedup": round(res["fuse_no_cull"]["ms"] / res["fuse"]["ms"], 3)})
    with open(a.step_out, "w") as f:
        json.dump({f"map{a.step}": res}, f)


def main():
    a = parse()
    if a.step:
        return step(a)
    res = {"metric": "bugseg_map_fuse: ms per batch of grids fused into the rolling local map", "unit": "ms"}
    with tempfile.TemporaryDirectory() as tmp:
        for size in SIZES:
            out = os.path.join(tmp, f"{size}.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", str(size), "--step-out", out, "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--window-ms", str(a.window_ms), "--batch", str(a.batch)]
            log(f"window {size} x {size} (limit {a.step_timeout:.0f} s)")
            try:
                rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"bench_local_map: window {size} ran out of its {a.step_timeout:.0f} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"bench_local_map: window {size} ended with status {rc}; nothing more is started")
            with open(out) as f:
                res.update(json.load(f))
    res.update({"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "window_ms": a.window_ms, "hbm_peak_gbs": HBM_PEAK_GBS,
                "config": {"batch": a.batch, "grid": list(GRID), "cell_m": CELL_M, "windows": list(SIZES),
                           "trajectory": "arc of 10 m radius, 0.15 m per grid"}})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
