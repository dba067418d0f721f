"""Host frames in, host grids out: a pinned, double-buffered stream over one OccupancyPipeline.

The reference's loop is host to host: a NumPy BGR frame goes into `sess.run` (models.py:42-44) and a
NumPy int8 grid comes back (bev.py:244-246) for `convert_to_occupancy_grid_msg`. `HostStream` is that
flow around the device-resident step: a ring of `depth` slots, each with a pinned host frame buffer,
a device frame buffer, a device grid buffer, a pinned host grid buffer and (graph=True) one captured
step over the two device buffers. Three streams: the copy-in stream, the compute stream (the
device's current stream when the HostStream is made) and the copy-out stream; with the pipeline's own
`streams=2` that is four, and no more are created. The copies stay outside the captured graphs, so a
step's graph is the one `OccupancyPipeline.capture` records today; no kernel is added — the copy
engines run beside the existing launches.

Orderings, all by events (no device-wide synchronisation after construction):
  * a step starts after its slot's copy-in (the compute stream waits for the copy-in's event);
  * a copy-out starts after its step (the copy-out stream waits for the step's event);
  * `next_frames()` hands out a slot's pinned frame buffer only after its previous copy-in finished
    (the host waits for that event);
  * `get()` returns after the step's copy-out finished (the host waits for that event).
The rest follows from the fetch rule — `put()` refuses a slot whose previous result has not been
fetched, and fetching is FIFO: the fetch waited for the slot's copy-out, which followed its step,
which followed its copy-in, so by the time a slot is put again nothing reads its device frames and
nothing reads or writes its device grids. Slots of different steps share the compute stream, so the
pipeline's internal buffers (resized frames, class maps) are never used by two steps at once.

Single-threaded use.
"""
from __future__ import annotations

import numpy as np
import torch

from .hostio_ring import SlotRing


class HostStream:
    def __init__(self, pipe, batch: int, frame_hw: tuple[int, int] | None = None, depth: int = 2, graph: bool = True):
        """pipe: an OccupancyPipeline. batch: frames per step (fixed). frame_hw: the camera resolution
        (H0, W0), default the pipeline's model resolution; when it differs the pipeline's resize runs.
        depth: slots in the ring (>= 1) = steps that can be outstanding. graph=False launches every
        step eagerly (`pipe.run`) instead of replaying a captured graph; same results.
        The grid shape and the calibration are those of the pipeline at this moment."""
        if int(batch) != batch or batch < 1:
            raise ValueError("batch must be an integer >= 1")
        self._ring = SlotRing(depth)
        self.pipe = pipe
        self.batch = B = int(batch)
        self.depth = self._ring.depth
        self.graph = bool(graph)
        H0, W0 = (pipe.H, pipe.W) if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1]))
        if H0 < 1 or W0 < 1:
            raise ValueError("frame_hw must be positive")
        self.frame_shape = (B, H0, W0, 3)
        self.grid_shape = tuple(pipe._grid_shape(B))
        self.device = dev = torch.device("cuda", pipe.model.ctx.device)
        self._compute = torch.cuda.current_stream(dev)
        self._cin = torch.cuda.Stream(device=dev)
        self._cout = torch.cuda.Stream(device=dev)
        n = self.depth
        self._pin_frames = [torch.empty(self.frame_shape, dtype=torch.uint8, pin_memory=True) for _ in range(n)]
        self._pin_grids = [torch.empty(self.grid_shape, dtype=torch.int8, pin_memory=True) for _ in range(n)]
        self._np_frames = [t.numpy() for t in self._pin_frames]
        self._np_grids = [t.numpy() for t in self._pin_grids]
        with torch.cuda.stream(self._compute):
            self._dev_frames = [torch.zeros(self.frame_shape, dtype=torch.uint8, device=dev) for _ in range(n)]
            self._dev_grids = [torch.empty(self.grid_shape, dtype=torch.int8, device=dev) for _ in range(n)]
            self._steps = []
            if self.graph:
                for s in range(n):
                    replay, _ = pipe.capture(self._dev_frames[s], out=self._dev_grids[s])
                    self._steps.append(replay)
                # the graphs hold the addresses of the pipeline's internal buffers: keep those alive even
                # if the pipeline re-allocates its own for another batch size
                self._keep = (pipe._x, pipe._seg_raw, pipe._grid, dict(getattr(pipe, "_pairs", {})),
                              getattr(pipe, "_road", None), getattr(pipe, "_clahe", None))
        self._in_done = [torch.cuda.Event() for _ in range(n)]      # slot's copy-in finished
        self._in_used = [False] * n
        self._step_done = [torch.cuda.Event() for _ in range(n)]
        self._out_done = [torch.cuda.Event() for _ in range(n)]     # slot's copy-out finished
        self._closed = False

    # -- state -------------------------------------------------------------------------------------
    @property
    def outstanding(self) -> int:
        """Steps put and not yet fetched (at most depth)."""
        return self._ring.outstanding

    @property
    def steps_put(self) -> int:
        """Steps enqueued so far = the sequence number the next put() returns."""
        return self._ring._put

    def _check_open(self):
        if self._closed:
            raise RuntimeError("HostStream is closed")

    # -- calls -------------------------------------------------------------------------------------
    def next_frames(self) -> np.ndarray:
        """The pinned (B, H0, W0, 3) uint8 buffer the next put() sends. Returns once that slot's
        previous copy-in has finished, so the caller may overwrite it (a camera driver writes here
        directly; there is no staging copy)."""
        self._check_open()
        s = self._ring.put_slot
        if self._in_used[s]:
            self._in_done[s].synchronize()
        return self._np_frames[s]

    def put(self, frames=None) -> int:
        """Enqueue one step on the next slot: the copy-in on the copy-in stream, the step on the
        compute stream after it, the grids' copy-out on the copy-out stream after the step. With
        `frames` (a (B, H0, W0, 3) uint8 array) they are first copied into the slot's pinned buffer
        (one host memcpy); without, whatever next_frames() holds is sent. Returns the step's sequence
        number without waiting for the device. ValueError: wrong shape or dtype; RuntimeError: the
        slot's previous result has not been fetched. A refused call enqueues nothing."""
        self._check_open()
        if frames is not None:
            frames = np.asarray(frames)
            if frames.dtype != np.uint8 or tuple(frames.shape) != self.frame_shape:
                raise ValueError(f"frames must be a uint8 array of shape {self.frame_shape}, got {frames.dtype} "
                                 f"{tuple(frames.shape)}")
        if self._ring.full:
            self._ring.put()                     # raises the overrun error
        if frames is not None:
            np.copyto(self.next_frames(), frames)
        s, seq = self._ring.put()
        with torch.cuda.stream(self._cin):
            self._dev_frames[s].copy_(self._pin_frames[s], non_blocking=True)
            self._in_done[s].record(self._cin)
        self._in_used[s] = True
        self._compute.wait_event(self._in_done[s])
        with torch.cuda.stream(self._compute):
            if self.graph:
                self._steps[s]()
            else:
                self.pipe.run(self._dev_frames[s], out=self._dev_grids[s])
            self._step_done[s].record(self._compute)
        self._cout.wait_event(self._step_done[s])
        with torch.cuda.stream(self._cout):
            self._pin_grids[s].copy_(self._dev_grids[s], non_blocking=True)
            self._out_done[s].record(self._cout)
        return seq

    def get(self, copy: bool = False) -> np.ndarray:
        """The int8 grids of the oldest unfetched step, after waiting for that step's copy-out only.
        The array is a view of the slot's pinned grid buffer: valid and unchanged until the put() that
        reuses the slot (the depth-th put from the one that produced it); copy=True returns an owned
        array. RuntimeError when nothing is outstanding."""
        self._check_open()
        s, _seq = self._ring.peek()
        self._out_done[s].synchronize()
        self._ring.get()
        g = self._np_grids[s]
        return g.copy() if copy else g

    def map(self, batches):
        """Generator over an iterable of frame batches: keeps `depth` steps in flight and yields each
        step's grids in order, as owned arrays. Starts with nothing outstanding."""
        if self.outstanding:
            raise RuntimeError("map() needs a stream with no outstanding step")
        for frames in batches:
            if self._ring.full:
                yield self.get(copy=True)
            self.put(frames)
        while self.outstanding:
            yield self.get(copy=True)

    def close(self) -> None:
        """Wait for the three streams, then drop the graphs and the buffers."""
        if self._closed:
            return
        self._closed = True
        for st in (self._cin, self._compute, self._cout):
            st.synchronize()
        self._steps = []
        self._keep = None
        self._np_frames = self._np_grids = None
        self._pin_frames = self._pin_grids = self._dev_frames = self._dev_grids = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
