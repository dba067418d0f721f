"""Batched, device-resident frame -> occupancy-grid path (BASELINE config 3):

    BGR u8 frames (B,H0,W0,3)  --[resize kernel, only if H0xW0 != HxW]-->  BGR u8 (B,H,W,3)
      --29 launches, one per ENet block (the initial block normalises the raw bytes as it loads
        them, argmax + 3-class remap in the class layer's epilogue)-->  u8 (B,H,W)
      --BEV rasteriser kernel-->  int8 grids (B,h,w)   [or ROS data order]

Everything stays in HBM; there is no host round trip between stages. With streams > 1 every frame
shard runs all three stages on its own context and stream. This is the
loop the reference's (absent) ROS node runs per frame (README.md:19), batched.

With a DeepLabV3 model the middle stage is its plan with the u8 final op: the resized
BGR frames go in as they are (the stem or the prep launch swaps the channels as it loads them), the
final op stores model.class_lut[class id] for the rows the rasteriser reads, and the resize and the
rasteriser run on a weightless engine context per shard.
"""
from __future__ import annotations

import gc

import numpy as np
import torch

from . import _native as N
from .bev import bev_transform_tools
from .models import ENET, DeepLabV3


class OccupancyPipeline:
    """streams > 1 splits the batch into that many frame shards, each run by its own engine context
    (own activation arena) on its own HIP stream, so the launches of different shards overlap on the
    device (one shard's compute phases beside another's memory phases). Results are identical."""

    def __init__(self, model: "ENET | DeepLabV3", bev: bev_transform_tools, grid_w_m: float, grid_h_m: float, cell_m: float,
                 model_hw: tuple[int, int] | None = None, ros_layout: bool = False, streams: int = 1,
                 binary: bool = False, stream_priority: int = 0, chain_forwards: bool = False, shard_offset: int = 0,
                 window_rows: bool = True, road_filter: bool = False, clahe: bool = False):
        """binary=True is the predict_binary + create_occupancy_grid_binary pairing (models.py:70-82,
        bev.py:97-165): class maps through the binary LUT, the binary rasteriser; in the laserscan-like
        mode its output is the reference's pair, (2, B, ...) (bev.py:164). stream_priority is the HIP
        priority of the side shards' streams (shard 0 runs on the caller's stream; lower = higher).
        chain_forwards=True starts shard i's forward when shard i-1's forward has finished, so each
        shard's BEV rasteriser runs beside the next shard's forward (only the last one is exposed)
        instead of all shards' forwards running together and their BEVs together at the end.
        shard_offset=k > 0 starts shard i+1 when shard i has reached its k-th launch (an
        event between launches k-1 and k of its forward), so the shards run different layers side by
        side instead of the same layer at the same time.
        window_rows=True computes only the class-map rows the rasteriser reads for this calibration
        (Context.bev_source_rows: for a forward-looking camera, the rows below the horizon): the decoder's
        last six launches run just the tiles those rows need (Context.forward_bgr_rows). The grids are the
        same; the rows of the internal class map that nothing samples are not computed. A calibration
        that samples the whole image, or window_rows=False, makes the full-frame calls.
        model may be a DeepLabV3 with its class_lut set (models.class_lut3 / class_lut_binary for the
        reference's conventions; binary=True only selects the binary rasteriser for what the LUT
        produces). model_hw then defaults to the net's crop and must fit inside it; every shard runs its
        own DeepLabV3.clone planned for that shard's frames; the row window applies to the final op
        alone (the ASPP image pooling needs the whole frame); shard_offset is refused.
        road_filter=True runs contour_noise_removal (image_processing_utils.py:4-44) on
        every shard's stream between the segmenter and the rasteriser: the class maps go through
        Context.road_filter into a second u8 buffer, which the rasteriser reads. Its output is a {0, 1} map,
        so it requires binary=True (ENET, or a DeepLabV3 whose LUT is class_lut_binary). The filter needs
        whole maps: a row cut off above the window would open holes and change the closing near the
        cut, so the forwards run full-frame whatever window_rows says.
        clahe=True runs image_processing_utils.clahe (image_processing_utils.py:46-61) on every
        shard's stream first, on the camera-size frames, before the resize of models.py:87: Context.clahe
        writes the enhanced frames into a pipeline-owned (B, H0, W0, 3) buffer, which the forward then reads
        (and which _seg re-runs after a windowed run). The caller's frames are not changed."""
        self.clahe = bool(clahe)
        self._clahe = None           # clahe: (its parameters, the caller's frames, the enhanced frames the forward reads)
        if road_filter and not binary:
            raise ValueError("road_filter=True needs binary=True: contour_noise_removal reads and writes a {0, 1} road map")
        self.road_filter = bool(road_filter)
        self._road = None            # road_filter: (its parameters, the filtered maps the rasteriser reads)
        self.model = model
        self._dl = isinstance(model, DeepLabV3)
        self.binary = binary
        self.bev = bev
        self.grid = (grid_w_m, grid_h_m, cell_m)
        if self._dl:
            crop = model._spec.crop_hw(model.net)
            self.H, self.W = model_hw if model_hw is not None else crop
            if self.H > crop[0] or self.W > crop[1] or self.H < 1 or self.W < 1:
                raise ValueError(f"model_hw {self.H}x{self.W} does not fit the network's {crop[0]}x{crop[1]} crop")
            if model.class_lut is None:
                raise ValueError("a DeepLabV3 model needs its class_lut set (models.class_lut3 / class_lut_binary): "
                                 "there is no default mapping of an arbitrary label set to the rasteriser's classes")
            if int(shard_offset) > 0:
                raise ValueError("shard_offset needs a forward that runs a range of launches, which DeepLabV3 lacks; "
                                 "use chain_forwards to stagger its shards")
        else:
            self.H, self.W = model_hw if model_hw is not None else (ENET.INPUT_HEIGHT, ENET.INPUT_WIDTH)
        self.ros_layout = ros_layout
        if (self.H, self.W) != (bev.input_width, bev.input_height):
            raise ValueError(f"model output {self.H}x{self.W} must equal the calibration's input image size "
                             f"{bev.input_width}x{bev.input_height} (bev.py:169)")
        if streams < 1:
            raise ValueError("streams must be >= 1")
        self.streams = streams
        self.stream_priority = stream_priority
        self.chain_forwards = chain_forwards
        self.shard_offset = int(shard_offset)
        # DeepLab: _ctxs are weightless engine contexts (resize, source rows, rasteriser: none of them
        # needs weights) and _engines the DeepLabV3 of each shard, shard 0 the caller's own
        self._ctxs = [N.Context(model.ctx.device, N.FP32)] if self._dl else [model.ctx]
        self._engines = [model] if self._dl else []
        self._streams = []
        self.window_rows = bool(window_rows) and not self.road_filter
        self._windowed = False       # the forwards of the run in progress are windowed
        self._spans = {}             # (context, calibration) -> the class-map rows the rasteriser reads
        self._x = None
        self._seg_raw = None         # the class maps as the last run left them (windowed: its rows only)
        self._seg_partial = None     # the last run was windowed: (frames, shard bounds) to complete _seg from
        self._grid = None

    def _shard_ctxs(self, dev: torch.device):
        while len(self._ctxs) < self.streams:
            if self._dl:
                c = N.Context(dev.index, N.FP32)
                self._engines.append(self.model.clone(dev.index))
            else:
                c = N.Context(dev.index, self.model.ctx.precision)
                c.load_weights(self.model.blob)
            self._ctxs.append(c)
            self._streams.append(torch.cuda.Stream(device=dev, priority=self.stream_priority))
        return self._ctxs, self._streams

    def _bounds(self, B: int):
        """Frame bounds of the shards a batch of B runs as ([0, B]: one shard on the model's own engine)."""
        if self.streams == 1 or B < self.streams:
            return [0, B]
        return [B * i // self.streams for i in range(self.streams + 1)]

    def _prepare_dl(self, B: int, dev: torch.device, may_build: bool) -> None:
        """Every shard's engine with its weights, class LUT and a plan for its share of B frames, and the
        row window of every shard's calibration. set_plan and set_class_lut allocate and synchronise the
        device, so none of this may happen while a stream is capturing: with may_build False a missing piece
        raises before any library call."""
        lut = self.model.class_lut
        if lut is None:
            raise ValueError("the model's class_lut was removed: an occupancy pipeline needs one")
        bounds = self._bounds(B)
        n = len(bounds) - 1
        todo = n > len(self._ctxs)
        for i in range(min(n, len(self._engines))):
            m = self._engines[i]
            todo = todo or m._plan_B != bounds[i + 1] - bounds[i] or not np.array_equal(m._class_lut, lut)
        if not todo:
            return
        if not may_build:
            raise RuntimeError(f"OccupancyPipeline.run inside a stream capture with no plan for a batch of {B}: planning "
                               "allocates and synchronises the device; use capture(), or run this batch size once first")
        if n > 1:
            self._shard_ctxs(dev)
        for i in range(n):
            m = self._engines[i]
            if not np.array_equal(m._class_lut, lut):
                m.class_lut = lut
            m._ensure_plan(bounds[i + 1] - bounds[i])
            self._source_rows(self._ctxs[i])

    def _bufs(self, B: int, dev: torch.device):
        if self._x is None or self._x.shape[0] != B or self._x.device != dev:
            self._x = torch.empty((B, self.H, self.W, 3), dtype=torch.uint8, device=dev)   # resized BGR
            # (zeros: the rows a windowed forward never writes are deterministic)
            self._seg_raw = torch.zeros((B, self.H, self.W), dtype=torch.uint8, device=dev)
            self._seg_partial = None
            self._grid = torch.empty(self._grid_shape(B), dtype=torch.int8, device=dev)
            if self.road_filter:
                from .image_processing_utils import road_filter_params
                self._road = (road_filter_params(self.H, self.W), torch.empty_like(self._seg_raw))
        return self._x, self._seg_raw, self._grid

    @property
    def _seg(self):
        """The whole class maps of the last run. After a windowed run the rows outside the window are
        computed first: the full forward on that run's frames, shard by shard on the contexts that ran
        them, on the current stream."""
        part, self._seg_partial = self._seg_partial, None
        if part is not None:
            frames, bounds = part
            st = torch.cuda.current_stream(frames.device)
            for i in range(len(bounds) - 1):
                s, e = bounds[i], bounds[i + 1]
                if self._dl:
                    # the final op alone over the missing rows, on the logits the shard's forward left
                    r0, r1 = self._source_rows(self._ctxs[i])
                    for rows in ((0, r0), (r1, self.H)):
                        if rows[0] < rows[1]:
                            self._engines[i].ctx.classes_from_logits(e - s, self.H, self.W, self._seg_raw[s:e], rows, st)
                    continue
                # (with clahe the frames kept are the enhanced ones: they are not enhanced again)
                self._run_forward(self._ctxs[i], frames[s:e], self._x[s:e], self._seg_raw[s:e], st, window=False,
                                  enhance=False)
        return self._seg_raw

    def _params(self):
        return self.bev.occupancy_params(*self.grid, ros_layout=self.ros_layout, binary=self.binary)

    def _grid_shape(self, B):
        p = self._params()
        shape = (B, p.occ_w, p.occ_h) if self.ros_layout else (B, p.occ_h, p.occ_w)
        return ((2,) + shape) if self.binary and p.laserscan else shape

    def run(self, frames_bgr: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        if frames_bgr.dim() != 4 or frames_bgr.shape[3] != 3 or frames_bgr.dtype != torch.uint8 or not frames_bgr.is_cuda:
            raise ValueError("frames must be a (B, H0, W0, 3) uint8 device tensor")
        B, H0, W0 = frames_bgr.shape[:3]
        if self._dl:
            self._prepare_dl(B, frames_bgr.device, may_build=not torch.cuda.is_current_stream_capturing())
        x, seg, grid = self._bufs(B, frames_bgr.device)
        if grid.shape != self._grid_shape(B):       # the calibration's laserscan flag changed
            self._grid = grid = torch.empty(self._grid_shape(B), dtype=torch.int8, device=frames_bgr.device)
        frames = frames_bgr.contiguous()
        if self.clahe:
            # every shard enhances its own frames on its own stream (_run_forward); from here on `frames` is
            # the enhanced buffer
            frames = self._clahe_bufs(frames)
        out = grid if out is None else out
        if tuple(out.shape) != tuple(grid.shape) or out.dtype != torch.int8 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int8 tensor of shape {tuple(grid.shape)}")
        p = self._params()
        self._seg_partial = None
        if self.streams == 1 or B < self.streams:
            self._run_shard(self._ctxs[0], frames, x, seg, out, p, None)
            if self._windowed:
                self._seg_partial = (frames, [0, B])
            return out
        pair = self.binary and bool(p.laserscan)
        ctxs, streams = self._shard_ctxs(frames.device)
        main = torch.cuda.current_stream(frames.device)
        ready = main.record_event()
        bounds = self._bounds(B)
        for i in range(self.streams):
            s, e = bounds[i], bounds[i + 1]
            st = main if i == 0 else streams[i - 1]
            if i:
                st.wait_event(ready)
            split_done = self.chain_forwards or (self.shard_offset > 0 and i + 1 < self.streams)
            with torch.cuda.stream(st):
                if self.shard_offset > 0 and i + 1 < self.streams:
                    self._run_forward(ctxs[i], frames[s:e], x[s:e], seg[s:e], st, split=self.shard_offset)
                    ready = self._split_event
                elif self.chain_forwards:
                    self._run_forward(ctxs[i], frames[s:e], x[s:e], seg[s:e], st)
                    ready = torch.cuda.Event()
                    ready.record(st)                  # the next shard's forward starts here
                if pair:
                    # the kernel writes a shard's pair as one contiguous (2, e - s, ...) block; the
                    # batch's pair (2, B, ...) holds it as two slabs, so stage it and copy
                    tmp = self._pair_buf(i, (2, e - s) + tuple(out.shape[2:]), out.device)
                    self._run_shard(ctxs[i], frames[s:e], x[s:e], seg[s:e], tmp, p, st, forward=not split_done)
                    out[:, s:e].copy_(tmp)
                else:
                    self._run_shard(ctxs[i], frames[s:e], x[s:e], seg[s:e], out[s:e], p, st, forward=not split_done)
        for st in streams[: self.streams - 1]:
            main.wait_stream(st)
        if self._windowed:
            self._seg_partial = (frames, bounds)
        return out

    def _clahe_bufs(self, frames):
        from .image_processing_utils import clahe_params
        old = self._clahe
        if old is None or old[2].shape != frames.shape or old[2].device != frames.device:
            enh = torch.empty_like(frames)
            self._clahe = (clahe_params(frames.shape[1], frames.shape[2]), frames, enh)
        else:
            self._clahe = (old[0], frames, old[2])
        return self._clahe[2]

    def _pair_buf(self, i, shape, dev):
        if not hasattr(self, "_pairs"):
            self._pairs = {}
        t = self._pairs.get(i)
        if t is None or tuple(t.shape) != shape or t.device != dev:
            t = self._pairs[i] = torch.empty(shape, dtype=torch.int8, device=dev)
        return t

    def capture(self, frames_bgr: torch.Tensor, out: torch.Tensor | None = None, warm: bool = True):
        """Record one ``run`` over these frame / output buffers as a HIP graph (every shard's launches
        and the stream fork / join between them) and return (replay, out): ``replay()`` re-launches the
        whole step with one call, reading whatever the frame buffer holds at that time. The buffers
        must stay alive and keep their addresses. warm=True runs the step once eagerly first;
        warm=False captures the very first call at this shape and geometry (the library allocates
        arenas and builds its tables on its own stream during the capture; only the shard contexts
        and streams are created beforehand). A DeepLabV3 pipeline prepares every shard's engine, weights,
        plan and class LUT before either form: planning must not run inside a capture."""
        dev = frames_bgr.device
        if self._dl:
            self._prepare_dl(frames_bgr.shape[0], dev, may_build=True)
        if warm:
            self.run(frames_bgr, out)
        elif self.streams > 1 and frames_bgr.shape[0] >= self.streams:
            self._shard_ctxs(dev)
        # No finalizer may run inside the capture: a dead reference cycle (a pipeline and the HostStream that
        # run_host keeps for it, say) still owns contexts, graphs and pinned buffers, and destroying those
        # synchronises the device and frees memory, which HIP refuses while a stream captures and which ends the
        # capture, or the process. The cyclic collector runs whenever allocation counts say so, so collect what
        # is dead now and keep it off until the capture has ended.
        gc.collect()
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                res = self.run(frames_bgr, out)
        finally:
            if gc_was_on:
                gc.enable()
        return graph.replay, res

    def host_stream(self, batch: int, frame_hw: tuple[int, int] | None = None, depth: int = 2, graph: bool = True):
        """A hostio.HostStream over this pipeline: pinned host frames in, pinned host grids out, the
        copies of `depth` steps in flight beside the step itself (the reference's host-to-host loop,
        models.py:42-44 -> bev.py:244-246, at the device path's speed)."""
        from .hostio import HostStream
        return HostStream(self, batch, frame_hw=frame_hw, depth=depth, graph=graph)

    def local_map(self, size_cells, **kw):
        """A mapping.LocalMap for this pipeline's grids: their cell size, shape and layout, on the
        model's device; size_cells = (Hm, Wm) and the keywords are LocalMap's. `map.update(pipe.run(frames), poses)`
        fuses a batch, and map.fuse can be captured in one graph with run. Refused for the binary laserscan output,
        whose (2, B, ...) pair is not a batch of grids."""
        p = self._params()
        if self.binary and p.laserscan:
            raise ValueError("local_map needs a batch of grids: the binary laserscan output is the reference's pair")
        from .mapping import LocalMap
        kw.setdefault("device", self._ctxs[0].device)
        return LocalMap(size_cells, self.grid[2], (p.occ_h, p.occ_w), ros_layout=self.ros_layout, **kw)

    def run_host(self, frames_np) -> np.ndarray:
        """One batch of host frames, (B, H0, W0, 3) uint8, -> its grids as an owned int8 array, through
        a depth-1 HostStream kept per (B, H0, W0) (rebuilt when the calibration or the grid changed,
        which a captured step would not see)."""
        f = np.asarray(frames_np)
        if f.ndim != 4 or f.shape[3] != 3 or f.dtype != np.uint8:
            raise ValueError("frames must be a (B, H0, W0, 3) uint8 array")
        if not hasattr(self, "_host"):
            self._host = {}
        key, stamp = tuple(f.shape[:3]), bytes(self._params())
        hit = self._host.get(key)
        if hit is None or hit[0] != stamp:
            if hit is not None:
                hit[1].close()
            hit = self._host[key] = (stamp, self.host_stream(f.shape[0], frame_hw=f.shape[1:3], depth=1))
        hit[1].put(f)
        return hit[1].get(copy=True)

    def _source_rows(self, ctx):
        """The class-map rows the rasteriser reads for the current calibration, or None for the whole
        frame (window_rows off, or nothing to skip); asked of the library once per context and calibration."""
        if not self.window_rows:
            return None
        p = self._params()
        key = (id(ctx), bytes(p))
        if key not in self._spans:
            r0, r1 = ctx.bev_source_rows(p, self.H, self.W)
            self._spans[key] = None if (r0 <= 0 and r1 >= self.H) or r0 >= r1 else (r0, r1)
        return self._spans[key]

    def _run_forward(self, ctx, frames, x, seg, stream, split=0, window=True, enhance=True):
        B, H0, W0 = frames.shape[:3]
        if self.clahe and enhance:
            # the shard's frames of the caller's batch: frames is a run of whole frames of the enhanced buffer
            cp, src, enh = self._clahe
            s = (frames.data_ptr() - enh.data_ptr()) // (H0 * W0 * 3)
            ctx.clahe(src[s:s + B], B, cp, frames, stream)
        if (H0, W0) != (self.H, self.W):
            # resize only (models.py:87); colour swap + normalisation are fused into the initial block
            ctx.preprocess(frames, B, H0, W0, self.H, self.W, N.PRE_BGR_U8, x, stream)
            frames = x
        if self._dl:
            rows = self._source_rows(ctx) if window else None
            if window:
                self._windowed = rows is not None
            engine = self._engines[self._ctxs.index(ctx)]
            engine.ctx.forward_classes(frames, True, B, self.H, self.W, seg, rows, stream)
            return
        kind = N.OUT_BINARY_U8 if self.binary else N.OUT_CLASS3_U8
        rows = self._source_rows(ctx) if window else None
        if window:
            self._windowed = rows is not None

        def ops(first, last):
            if rows is not None:
                ctx.forward_bgr_rows(frames, B, self.H, self.W, kind, seg, rows, first, last, stream)
            elif (first, last) == (0, -1):
                ctx.forward_bgr(frames, B, self.H, self.W, kind, seg, stream)
            else:
                ctx.forward_bgr_ops(frames, B, self.H, self.W, kind, seg, first, last, stream)

        if split <= 0:
            ops(0, -1)
            return
        # launches [0, split), an event (the next shard starts there), then the rest
        ops(0, split)
        self._split_event = torch.cuda.Event()
        self._split_event.record(stream)
        ops(split, -1)

    def _run_shard(self, ctx, frames, x, seg, out, p, stream, forward=True):
        if forward:
            self._run_forward(ctx, frames, x, seg, stream)
        if self.road_filter:
            # the shard's frames of the filtered buffer: seg is a run of whole frames of _seg_raw
            rp, flt = self._road
            s = (seg.data_ptr() - self._seg_raw.data_ptr()) // (self.H * self.W)
            flt = flt[s:s + frames.shape[0]]
            ctx.road_filter(seg, frames.shape[0], rp, flt, stream)
            seg = flt
        # the shard's own context: its laserscan scratch is never shared with another shard's stream
        ctx.bev(seg, frames.shape[0], p, out, stream)
