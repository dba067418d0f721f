"""Benchmark of the device confusion matrix (evaluate.confusion_device).

One process, one GPU, batch 64. Label and prediction maps of equal shape unless said otherwise:
  camera   480x640, C = 15        deeplab  513x513, C = 21        grids  200x200 through Evaluator.for_grids()
each with three contents:
  uniform  one class everywhere (the worst case for contention: every pixel lands in one bin)
  road     class maps of the synthetic road scene (synthetic.road_frames(seed=0): the mean of the three channels
           cut into C levels; for the grids, the occupancy grids of those scenes' three-level maps under the
           bench calibration); the prediction is the same scene with its level borders moved
  random   uniformly random classes (the worst case for the spread over bins)
and one case `resample`: road labels at 480x640 against predictions at 256x512, C = 15.
It prints ONE JSON line and writes the same record to --out (profiles/evaluate.json). Per case:

  call           one bugseg_confusion call on the batch into a persistent accumulator. Timing as bench_canny.py:
                 HIP events around a window of back-to-back calls, at least --steps of them and as many as make
                 the window --window-ms long; --repeats windows per figure, taken in turn with the other figures'
                 windows. ms is the median window's time per call, ms_min and ms_max the spread. bytes = what the
                 call must read (every label byte and every prediction byte once); gbs = bytes per second at the
                 median; hbm_frac against the 8 TB/s HBM peak (both maps of the largest case are 39 MB and stay
                 in the 256 MiB Infinity Cache between calls, so this is a rate against the HBM roofline, not a
                 measurement of HBM traffic)
  torch_bincount what a user would write on the device without this feature, timed the same way in the same run:
                 torch.bincount(gt.long() * C + pred.long(), minlength=C * C) (behind the table look-ups for the
                 grids and the index gather for `resample`, which the kernel does inside)
  host_bincount  the same with both maps copied to the host and np.bincount there; wall time per call,
                 --host-repeats calls
  speedup_vs_torch, speedup_vs_host   baseline ms / call ms at the medians
  checked        the call's matrix equals the torch baseline's and the NumPy restatement's (tests/evaluate_ref.py)
call_floor: the same call on one 1 x 1 frame, timed the same way: what a call costs whatever the maps hold (the
Python entry and the enqueue of one launch); a case whose call time is close to it is bound by that, not by the kernel.
uniform_over_random: the ratio of the uniform content's call time to the random one's, per shape.

There is no threshold: the bar is that the call beats torch_bincount on every content.

Run:  python bench_evaluate.py [--batch B --steps K --warmup W --repeats R --window-ms MS --out PATH]
"""
from __future__ import annotations

import argparse
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


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=7, help="timed windows per figure: median, min and max are reported")
    p.add_argument("--window-ms", type=float, default=250.0, help="least length of one timed window")
    p.add_argument("--host-repeats", type=int, default=3, help="calls of the host baseline per case")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate.json"))
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.batch < 1 or a.repeats < 1 or a.host_repeats < 1 or not a.window_ms >= 0:
        p.error("--steps, --batch, --repeats and --host-repeats must be at least 1, --warmup and --window-ms at least 0")
    return a


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench_evaluate {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


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
    """{name: (ms per call in each of a.repeats windows, calls per window)}: bench_canny.py's method."""
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


def levels(grey: np.ndarray, C: int, shift: int = 0) -> np.ndarray:
    """(B, h, w) grey bytes -> class maps of C levels; shift moves the level borders."""
    return (np.clip(grey.astype(np.int32) + shift, 0, 255) * C // 256).astype(np.uint8)


def measure(name, pred, gt, C, pl, gl, a, R, E):
    """pred, gt: uint8 device maps; pl, gl: 256-entry tables or None."""
    dev = gt.device
    B, gh, gw = gt.shape
    ph, pw = pred.shape[1:]
    params = E.confusion_params((ph, pw), (gh, gw), C, pl, gl)
    acc = torch.zeros(C * C + 1, dtype=torch.int64, device=dev)
    plt = None if pl is None else torch.from_numpy(pl).to(dev).long()
    glt = None if gl is None else torch.from_numpy(gl).to(dev).long()
    ys = xs = None
    if (ph, pw) != (gh, gw):
        ys = torch.from_numpy(R.nearest_index(gh, ph)).to(dev)
        xs = torch.from_numpy(R.nearest_index(gw, pw)).to(dev)

    def call():
        E.confusion_device(pred, gt, C, out=acc, params=params)

    def torch_bincount():
        p, g = pred, gt
        if ys is not None:
            p = p[:, ys][:, :, xs]
        p, g = p.long(), g.long()
        if plt is not None:
            p, g = plt[p], glt[g]
            ok = (p < C) & (g < C)
            p, g = p[ok], g[ok]
        return torch.bincount(g.reshape(-1) * C + p.reshape(-1), minlength=C * C)

    def host_bincount():
        p, g = pred.cpu().numpy(), gt.cpu().numpy()
        if ys is not None:
            p = R.resample(p, (gh, gw))
        p, g = p.astype(np.int64), g.astype(np.int64)
        if pl is not None:
            p, g = pl.astype(np.int64)[p], gl.astype(np.int64)[g]
            ok = (p < C) & (g < C)
            p, g = p[ok], g[ok]
        return np.bincount(g.reshape(-1) * C + p.reshape(-1), minlength=C * C)

    # the three agree before anything is timed
    call()
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    want = R.accumulator(pred.cpu().numpy(), gt.cpu().numpy(), C, pl, gl)
    if not (np.array_equal(got, want) and np.array_equal(got[:-1], torch_bincount().cpu().numpy())
            and np.array_equal(got[:-1], host_bincount())):
        raise RuntimeError(f"{name}: the device matrix differs from the restatement or a baseline")
    t = timed({"call": call, "torch_bincount": torch_bincount}, a)
    host = []
    for _ in range(a.host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_bincount()
        host.append((time.perf_counter() - t0) * 1e3)
    nbytes = B * (gh * gw + (gh * gw if ys is None else ph * pw))
    r = spread(t["call"][0])
    gbs = nbytes / (r["ms"] * 1e-3) / 1e9
    r.update({"calls_per_window": t["call"][1], "us_per_frame": round(r["ms"] * 1e3 / B, 3), "bytes": nbytes,
              "gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)})
    tb = spread(t["torch_bincount"][0])
    tb["calls_per_window"] = t["torch_bincount"][1]
    hb = spread(host)
    hb["calls"] = a.host_repeats
    return {"pred_shape": [B, ph, pw], "gt_shape": [B, gh, gw], "num_classes": C, "call": r, "torch_bincount": tb,
            "host_bincount": hb, "speedup_vs_torch": round(tb["ms"] / r["ms"], 2),
            "speedup_vs_host": round(hb["ms"] / r["ms"], 1), "nonzero_bins": int((got != 0).sum()), "checked": True}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_evaluate.py needs a HIP GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    import evaluate_ref as R
    from bugcar_image_segmentation_amd import evaluate as E
    from bugcar_image_segmentation_amd import synthetic

    B = a.batch
    rng = np.random.default_rng(0)
    res = {"metric": "confusion matrix on the device: ms per batch call", "unit": "ms"}

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def grey(h, w):
        return (synthetic.road_frames(B, h, w, seed=0).astype(np.uint16).sum(axis=3) // 3).astype(np.uint8)

    for name, (h, w), C in (("camera", (480, 640), 15), ("deeplab", (513, 513), 21)):
        g = grey(h, w)
        maps = {"uniform": (np.full((B, h, w), C // 2, np.uint8), np.full((B, h, w), C // 2, np.uint8)),
                "road": (levels(g, C, 6), levels(g, C)),
                "random": (rng.integers(0, C, (B, h, w), dtype=np.uint8), rng.integers(0, C, (B, h, w), dtype=np.uint8))}
        for kind, (pred, gt) in maps.items():
            log(f"{name}/{kind}")
            res[f"{name}/{kind}"] = measure(f"{name}/{kind}", up(pred), up(gt), C, None, None, a, R, E)
    # occupancy grids, int8 read as uint8, through the tables of Evaluator.for_grids()
    g = grey(480, 640)
    bev = synthetic.synthetic_bev(480, 640)
    gargs = (synthetic.GRID_W_M, synthetic.GRID_H_M, synthetic.CELL_M)
    lut = E.grid_lut()
    vals = np.array([255, 0, 100], dtype=np.uint8)
    grids = {"uniform": (np.zeros((B, 200, 200), np.uint8), np.zeros((B, 200, 200), np.uint8)),
             "road": tuple(bev.create_occupancy_grid_device(up(levels(g, 3, s)), *gargs).contiguous().view(torch.uint8)
                           for s in (6, 0)),
             "random": (vals[rng.integers(0, 3, (B, 200, 200))], vals[rng.integers(0, 3, (B, 200, 200))])}
    for kind, (pred, gt) in grids.items():
        log(f"grids/{kind}")
        pred, gt = (x if isinstance(x, torch.Tensor) else up(x) for x in (pred, gt))
        res[f"grids/{kind}"] = measure(f"grids/{kind}", pred, gt, 3, lut, lut, a, R, E)
    log("resample")
    res["resample/road"] = measure("resample/road", up(levels(grey(256, 512), 15, 6)), up(levels(g, 15)), 15, None, None, a, R, E)
    # what a call costs whatever the maps hold: one 1 x 1 frame (the Python entry, the enqueue, one workgroup)
    one = torch.zeros((1, 1, 1), dtype=torch.uint8, device=dev)
    acc1 = torch.zeros(15 * 15 + 1, dtype=torch.int64, device=dev)
    p1 = E.confusion_params((1, 1), (1, 1), 15)
    floor = timed({"call": lambda: E.confusion_device(one, one, 15, out=acc1, params=p1)}, a)["call"]
    res["call_floor"] = dict(spread(floor[0]), calls_per_window=floor[1])
    res["uniform_over_random"] ={s: round(res[f"{s}/uniform"]["call"]["ms"] / res[f"{s}/random"]["call"]["ms"], 3)
                                  for s in ("camera", "deeplab", "grids")}
    res.update({"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "window_ms": a.window_ms,
                "hbm_peak_gbs": HBM_PEAK_GBS, "config": {"batch": B}})
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
