"""Benchmark of DeepLabV3 as the occupancy pipeline's segmenter: BGR frames in HBM -> occupancy grids.

One process, one GPU. MobileNetV2 DeepLabV3 in bf16 at 513x513, B = 64, one stream, the synthetic
calibration synthetic.synthetic_bev(513, 513) and grid synthetic.GRID_*; the seeded synthetic network and
uniform random frames (seed 0), the reference's three-class table (models.class_lut3(21, (0, 1), (2, 9))).
Three steps over the same frames, each captured as one HIP graph and timed side by side:

  pipeline          OccupancyPipeline(DeepLabV3, ...).capture: forward with the u8 + LUT final op over the
                    rows the rasteriser reads, then the rasteriser
  pipeline_full     the same with window_rows=False (the final op over the whole frame)
  composed          what a user assembled before the pipeline took DeepLab: RGB frames ->
                    DeepLabV3.predict_device (int64 ids) -> torch gather through the LUT to u8 -> Context.bev

Timing: every step is warmed up, then `--rounds` rounds visit the three steps in turn (so drift of the
shared machine lands on all of them); a visit is `--steps` graph replays between two HIP events on the
stream they run on. Reported per step: the median over the rounds of ms per step, the fastest and slowest
round, and spread = (slowest - fastest) / median. `per_op` times the pieces that differ, each alone with
HIP events (eager, repeated): the int64 final op, the gather, the u8 final op windowed and whole, the
rasteriser. `class_map_bytes` is counted from the shapes, not measured. The three steps' grids are compared
before anything is timed; the run fails if they differ.

Prints ONE JSON line and writes it to --out (default profiles/deeplab_bev.json).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20, help="graph replays per timed visit")
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=9, help="timed visits per step")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "deeplab_bev.json"))
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.rounds < 1:
        p.error("--steps and --rounds must be at least 1 and --warmup at least 0")
    return a


def timed(fn, n, stream):
    """ms per call of n calls of fn between two HIP events on `stream`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(n):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def summary(ms):
    med = statistics.median(ms)
    return {"ms_per_step": round(med, 4), "fastest": round(min(ms), 4), "slowest": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4), "rounds": [round(v, 4) for v in ms]}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deeplab_bev needs a HIP GPU: nothing here is measured without one")
    from bugcar_image_segmentation_amd import _native as N
    from bugcar_image_segmentation_amd import synthetic
    from bugcar_image_segmentation_amd.models import DeepLabV3, class_lut3
    from bugcar_image_segmentation_amd.pipeline import OccupancyPipeline

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    B = a.batch
    net = DeepLabV3(precision=a.precision).net          # the seeded synthetic MobileNetV2 network, built once
    C = net.crop
    lut = class_lut3(net.num_classes, (0, 1), (2, 9))
    grid = (synthetic.GRID_W_M, synthetic.GRID_H_M, synthetic.CELL_M)
    bgr = torch.from_numpy(synthetic.uniform_frames(B, C, C, seed=0)).to(dev)
    rgb = bgr.flip(3).contiguous()

    def pipeline(window):
        m = DeepLabV3(net=net, precision=a.precision)
        m.class_lut = lut
        pipe = OccupancyPipeline(m, synthetic.synthetic_bev(C, C), *grid, window_rows=window)
        replay, out = pipe.capture(bgr)
        return pipe, replay, out

    pipe_w, replay_w, out_w = pipeline(True)
    pipe_f, replay_f, out_f = pipeline(False)

    # the composition on the parent: predict_device -> gather + u8 -> Context.bev, as one captured step
    model_c = DeepLabV3(net=net, precision=a.precision)
    ctx_c = N.Context(0, N.FP32)
    params = synthetic.synthetic_bev(C, C).occupancy_params(*grid)
    lut_t = torch.from_numpy(lut).to(dev)
    ids = torch.empty((B, C, C), dtype=torch.int64, device=dev)
    seg_c = torch.empty((B, C, C), dtype=torch.uint8, device=dev)
    out_c = torch.empty_like(out_w)

    def composed():
        # (the stream of the moment: inside the capture it is the capturing stream, not `stream`)
        model_c.predict_device(rgb, out=ids)
        torch.index_select(lut_t, 0, ids.view(-1), out=seg_c.view(-1))
        ctx_c.bev(seg_c, B, params, out_c, torch.cuda.current_stream(dev))

    composed()
    torch.cuda.synchronize()
    graph_c = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_c):
        composed()
    steps = {"pipeline": replay_w, "pipeline_full": replay_f, "composed": graph_c.replay}

    # every replay must produce its grids itself: clear them first
    for o in (out_w, out_f, out_c):
        o.fill_(-128)
    for fn in steps.values():
        fn()
    torch.cuda.synchronize()
    if not (torch.equal(out_w, out_c) and torch.equal(out_f, out_c)):
        raise SystemExit("the three steps' grids differ: nothing timed")
    rows = pipe_w._source_rows(pipe_w._ctxs[0])

    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ms[k].append(timed(fn, a.steps, stream))

    # the pieces that differ, each alone (eager, HIP events; the logits are those of the last forward)
    reps = 20
    dl = pipe_w.model.ctx
    seg = pipe_w._seg_raw
    am = len(model_c.plan_info["per_op"]) - 1
    assert model_c.plan_info["per_op"][am][0] == "argmax"
    pieces = {
        "final_op_int64": lambda: model_c.ctx.launch_op(am, stream),
        "lut_gather_u8": lambda: torch.index_select(lut_t, 0, ids.view(-1), out=seg_c.view(-1)),
        "final_op_u8_window": lambda: dl.classes_from_logits(B, C, C, seg, rows or (0, C), stream),
        "final_op_u8_full": lambda: dl.classes_from_logits(B, C, C, seg, (0, C), stream),
        "rasteriser": lambda: ctx_c.bev(seg_c, B, params, out_c, stream),
    }
    per_op = {}
    for k, fn in pieces.items():
        fn()
        per_op[k] = round(min(timed(fn, reps, stream) for _ in range(3)) * 1e3, 2)      # us, best of 3 visits

    px = B * C * C
    wpx = B * C * ((rows[1] - rows[0]) if rows else C)
    res = {
        "metric": "ms per step, DeepLabV3 513x513 BGR frames in HBM -> occupancy grids (synthetic)",
        "unit": "ms", "higher_is_better": False, "dtype": a.precision, "batch": B, "crop": C,
        "steps_per_visit": a.steps, "warmup": a.warmup, "rounds": a.rounds,
        "timing": "HIP events around `steps` replays of each captured step; median over rounds that visit the three "
                  "steps in turn; spread = (slowest - fastest round) / median",
        "pipeline": summary(ms["pipeline"]), "pipeline_full": summary(ms["pipeline_full"]),
        "composed": summary(ms["composed"]),
        "pipeline_over_composed": round(statistics.median(ms["pipeline"]) / statistics.median(ms["composed"]), 4),
        "frames_per_s": {k: round(B / statistics.median(v) * 1e3, 1) for k, v in ms.items()},
        "window_rows": list(rows) if rows else None,
        "grids_equal": True,
        "per_op_us": per_op,
        "class_map_bytes": {"note": "counted from the shapes: bytes of class map written by the final op and read back "
                                    "(by the gather and the rasteriser, or by the rasteriser alone)",
                            "composed": px * 8 + px * 8 + px + px, "pipeline_full": px + px, "pipeline": wpx + wpx},
        "data": f"uniform u8 frames (seed 0); seeded synthetic MobileNetV2 weights (seed {net.meta.get('seed')}); "
                "class_lut3(21, (0, 1), (2, 9)); synthetic_bev(513, 513), 10 m x 10 m grid of 0.05 m cells",
    }
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
