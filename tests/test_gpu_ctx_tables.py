"""The per-context table caches past their capacity: the BEV warp-tap tables, the laserscan
polar tables with the scratch of the scratch-owning entry, and the resize tables of bugseg_preprocess each hold
4 entries, so a 5th geometry evicts, and a table a captured graph reads must survive that. Every case runs on a
Context of its own (empty caches), eagerly and with the first geometry captured into a graph, on 48 x 64 class
maps warped to 120 x 100, grids of at most 99 cells and B = 2; the grids equal oracle.ocv_c, the resized frames
an eager result of a second fresh context, byte for byte."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bugcar_image_segmentation_amd import _native as N
from bugcar_image_segmentation_amd import synthetic
from oracle import ocv_c

pytestmark = pytest.mark.gpu
ROWS, COLS, WW, WH, B = 48, 64, 120, 100, 2
GRID = (1.0, 0.8, 0.1)                                  # 10 x 8 cells
# seven grids with seven (occ_w, occ_h): seven polar tables, and scratch that grows and shrinks
GRIDS = [(1.0, 0.8, 0.1), (0.8, 0.8, 0.1), (1.1, 0.7, 0.1), (0.7, 0.5, 0.1), (1.2, 0.9, 0.1), (0.9, 0.4, 0.1), (0.5, 0.9, 0.1)]
H, W = 96, 128                                          # the model's resolution; no source is it or twice it
SOURCES = [(131, 170), (110, 150), (101, 135), (120, 161), (143, 190), (99, 140), (125, 171)]


@functools.lru_cache(maxsize=None)
def _bev(seed):
    """Calibration `seed`: a perturbed matrix, so its tap table is one no other seed shares."""
    rng = np.random.default_rng(2000 + seed)
    bev = synthetic.synthetic_bev(ROWS, COLS, WW, WH)
    bev._bev_matrix = bev._bev_matrix @ np.array([[1 + 0.03 * rng.normal(), 0.01 * rng.normal(), 3 * rng.normal()],
                                                  [0.01 * rng.normal(), 1 + 0.03 * rng.normal(), 3 * rng.normal()],
                                                  [1e-5 * rng.normal(), 1e-5 * rng.normal(), 1.0]])
    return bev


@functools.lru_cache(maxsize=None)
def _segs(seed):
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 3, size=(B, ROWS // 4, COLS // 4)), np.ones((1, 4, 4), np.int64)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _want(seed, seg_seed, grid, laserscan):
    f = ocv_c.create_occupancy_grid_laserscan if laserscan else ocv_c.create_occupancy_grid
    return np.stack([f(s, _bev(seed)._bev_matrix, WW, WH, 1.0, *grid) for s in _segs(seg_seed)])


def _run(ctx, seed, seg, grid=GRID, laserscan=False, own_scratch=False, out=None, **fields):
    """One rasteriser call on `ctx`; own_scratch: through bugseg_bev_occgrid, whose scratch the context owns."""
    p = _bev(seed).occupancy_params(*grid, laserscan=laserscan)
    for k, v in fields.items():
        setattr(p, k, v)
    if out is None:
        out = torch.empty((B, p.occ_h, p.occ_w), dtype=torch.int8, device=seg.device)
    if own_scratch:
        N.check(ctx.lib.bugseg_bev_occgrid(ctx.h, seg.data_ptr(), B, ctypes.byref(p), out.data_ptr(),
                                           N.stream_handle(torch.cuda.current_stream(seg.device))), ctx.h)
    else:
        ctx.bev(seg, B, p, out, torch.cuda.current_stream(seg.device))
    return out


def _captured(fn):
    """fn() captured as the first call of its kind, replayed once -> the graph."""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _same(got, want):
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_bev_tables_evict_and_rebuild(gpu):
    ctx = N.Context(gpu.index)
    seg = torch.from_numpy(_segs(1)).to(gpu)
    for seed in (0, 1, 2, 3, 4, 5, 0):                  # the 5th and 6th evict; 0 went first and is rebuilt
        _same(_run(ctx, seed, seg), _want(seed, 1, GRID, False))
    ctx.close()


def test_bev_table_of_a_graph_survives_evictions(gpu):
    ctx = N.Context(gpu.index)
    seg = torch.from_numpy(_segs(1)).to(gpu)
    out = torch.empty((B,) + _want(0, 1, GRID, False).shape[1:], dtype=torch.int8, device=gpu)
    g = _captured(lambda: _run(ctx, 0, seg, out=out))
    _same(out, _want(0, 1, GRID, False))
    for seed in (1, 2, 3, 4, 5):                        # 4 and 5 evict: unpinned, the graph's table would go first
        _same(_run(ctx, seed, seg), _want(seed, 1, GRID, False))
    seg.copy_(torch.from_numpy(_segs(2)))
    g.replay()
    _same(out, _want(0, 2, GRID, False))
    _same(_run(ctx, 6, seg), _want(6, 2, GRID, False))  # a 7th: the cache grew or evicted an unpinned entry
    del g
    ctx.close()


def test_laserscan_grids_evict_polar_tables_and_regrow_scratch(gpu):
    ctx = N.Context(gpu.index)
    seg = torch.from_numpy(_segs(1)).to(gpu)
    for grid in GRIDS[:6] + GRIDS[:1]:
        _same(_run(ctx, 0, seg, grid, laserscan=True, own_scratch=True), _want(0, 1, grid, True))
    ctx.close()


def test_polar_table_of_a_graph_survives_evictions(gpu):
    ctx = N.Context(gpu.index)
    seg = torch.from_numpy(_segs(1)).to(gpu)
    out = torch.empty((B,) + _want(0, 1, GRIDS[0], True).shape[1:], dtype=torch.int8, device=gpu)
    g = _captured(lambda: _run(ctx, 0, seg, GRIDS[0], laserscan=True, out=out))
    _same(out, _want(0, 1, GRIDS[0], True))
    for grid in GRIDS[1:6]:
        _same(_run(ctx, 0, seg, grid, laserscan=True), _want(0, 1, grid, True))
    seg.copy_(torch.from_numpy(_segs(2)))
    g.replay()
    _same(out, _want(0, 2, GRIDS[0], True))
    _same(_run(ctx, 0, seg, GRIDS[6], laserscan=True), _want(0, 2, GRIDS[6], True))
    del g
    ctx.close()


def _frames(gpu, k, seed):
    return torch.from_numpy(synthetic.road_frames(B, *SOURCES[k], seed=seed)).to(gpu)


def _resized(ctx, frames, out=None):
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=frames.device)
    ctx.preprocess(frames, B, frames.shape[1], frames.shape[2], H, W, N.PRE_BGR_U8, out, torch.cuda.current_stream(frames.device))
    return out


@functools.lru_cache(maxsize=None)
def _resize_want(gpu, k, seed):
    """Source k resized by a fresh context that builds this one table only."""
    ref = N.Context(gpu.index)
    want = _resized(ref, _frames(gpu, k, seed)).cpu().numpy()
    ref.close()
    return want


def test_resize_tables_evict_and_rebuild(gpu):
    ctx = N.Context(gpu.index)
    for k in (0, 1, 2, 3, 4, 5, 0):
        _same(_resized(ctx, _frames(gpu, k, 70 + k)), _resize_want(gpu, k, 70 + k))
    ctx.close()


def test_resize_table_of_a_graph_survives_evictions(gpu):
    ctx = N.Context(gpu.index)
    buf = _frames(gpu, 0, 70)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=gpu)
    g = _captured(lambda: _resized(ctx, buf, out))
    _same(out, _resize_want(gpu, 0, 70))
    for k in (1, 2, 3, 4, 5):
        _same(_resized(ctx, _frames(gpu, k, 70 + k)), _resize_want(gpu, k, 70 + k))
    buf.copy_(_frames(gpu, 0, 80))
    g.replay()
    _same(out, _resize_want(gpu, 0, 80))
    _same(_resized(ctx, _frames(gpu, 6, 76)), _resize_want(gpu, 6, 76))
    del g
    ctx.close()


def test_a_refused_call_leaves_the_context_usable(gpu):
    ctx = N.Context(gpu.index)
    seg = torch.from_numpy(_segs(1)).to(gpu)
    with pytest.raises(ValueError, match="variant must be 0 or 1"):
        _run(ctx, 0, seg, variant=2)
    with pytest.raises(ValueError, match="bad BEV geometry"):
        _run(ctx, 0, seg, laserscan=True, own_scratch=True, warp_w=0)
    _same(_run(ctx, 0, seg), _want(0, 1, GRID, False))
    _same(_run(ctx, 0, seg, laserscan=True, own_scratch=True), _want(0, 1, GRID, True))
    ctx.close()
