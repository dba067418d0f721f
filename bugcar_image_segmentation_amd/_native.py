"""ctypes binding of libbugseg.so (include/bugseg.h).

There is no fallback: if the library is missing or no HIP device is visible, every product call
raises. torch is imported first so that the library binds to torch's already-loaded HIP runtime
(same soname libamdhip64.so.7) and torch device pointers / streams are valid for it.
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path

import torch  # noqa: F401  (must precede loading the library: shared HIP runtime)

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("BUGSEG_LIB", _PKG / "libbugseg.so"))

OK, EINVAL, ENOMEM, EHIP, EFORMAT, ESTATE = 0, -1, -2, -3, -4, -5
FP32, BF16, F16 = 0, 1, 2
OUT_LOGITS_F32, OUT_CLASS15_U8, OUT_CLASS3_U8, OUT_BINARY_U8 = 0, 1, 2, 3
PRE_ENGINE, PRE_NCHW_F64, PRE_NCHW_F32, PRE_BGR_U8 = 0, 1, 2, 3

EXPORTED = ("bugseg_version", "bugseg_create", "bugseg_destroy", "bugseg_load_weights", "bugseg_num_classes",
            "bugseg_input_bytes", "bugseg_preprocess", "bugseg_nchw_to_input", "bugseg_enet_forward",
            "bugseg_enet_forward_bgr", "bugseg_enet_forward_bgr_ops", "bugseg_enet_forward_bgr_rows",
            "bugseg_bev_source_rows", "bugseg_debug_row_windows", "bugseg_debug_poison_arena",
            "bugseg_debug_stage3_windows", "bugseg_debug_plan_windows", "bugseg_debug_read_block_output",
            "bugseg_debug_pair_walk", "bugseg_debug_pair_plan",
            "bugseg_bev_occgrid", "bugseg_bev_workspace_bytes", "bugseg_bev_occgrid_ws", "bugseg_plan_info", "bugseg_plan_op", "bugseg_plan_launch_op",
            "bugseg_last_error",
            "bugseg_road_filter_workspace_bytes", "bugseg_road_filter", "bugseg_debug_road_filter_ops",
            "bugseg_clahe_workspace_bytes", "bugseg_clahe_bgr", "bugseg_debug_clahe_stage", "bugseg_debug_clahe_table",
            "bugseg_canny_workspace_bytes", "bugseg_canny", "bugseg_debug_canny_stage", "bugseg_confusion",
            "bugseg_bev_warp_image", "bugseg_hough_trig", "bugseg_hough_workspace_bytes", "bugseg_hough_lines",
            "bugseg_debug_hough_stage",
            "bugseg_quad_workspace_bytes", "bugseg_find_quad", "bugseg_quad_moments", "bugseg_debug_quad_stage",
            "bugseg_map_fuse",
            "bugseg_dl_create", "bugseg_dl_destroy", "bugseg_dl_load_weights", "bugseg_dl_set_plan",
            "bugseg_dl_forward", "bugseg_dl_launch_op", "bugseg_dl_read_buffer", "bugseg_dl_last_error",
            "bugseg_dl_set_class_lut", "bugseg_dl_forward_classes", "bugseg_dl_classes_from_logits",
            "bugseg_debug_parse_pack", "bugseg_debug_polar_tables", "bugseg_debug_ctx_info", "bugseg_debug_tile_walk", "bugseg_debug_set_spans", "bugseg_debug_pool_indices",
            "bugseg_dl_debug_check_plan", "bugseg_dl_debug_op_layout", "bugseg_dl_debug_plan_groups",
            "bugseg_debug_knobs", "bugseg_dl_debug_knobs", "bugseg_debug_fused_forms")
DL_OP_FIELDS = 32


class BevParams(ctypes.Structure):
    _fields_ = [("M", ctypes.c_double * 9), ("in_rows", ctypes.c_int), ("in_cols", ctypes.c_int),
                ("warp_w", ctypes.c_int), ("warp_h", ctypes.c_int), ("occ_w_px", ctypes.c_int),
                ("occ_h_px", ctypes.c_int), ("occ_w", ctypes.c_int), ("occ_h", ctypes.c_int),
                ("left_x", ctypes.c_int), ("top_y", ctypes.c_int), ("ros_layout", ctypes.c_int),
                ("variant", ctypes.c_int), ("laserscan", ctypes.c_int)]


class RoadFilterParams(ctypes.Structure):
    """bugseg_road_filter_params: image_processing_utils.road_filter_params computes them."""
    _fields_ = [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("k", ctypes.c_int), ("y_top", ctypes.c_int),
                ("min_count", ctypes.c_int)]


class ClaheParams(ctypes.Structure):
    """bugseg_clahe_params: image_processing_utils.clahe_params builds and checks them."""
    _fields_ = [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("tiles_x", ctypes.c_int), ("tiles_y", ctypes.c_int),
                ("clip_limit", ctypes.c_float)]


class CannyParams(ctypes.Structure):
    """bugseg_canny_params: image_processing_utils.canny_params builds and checks them."""
    _fields_ = [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("low", ctypes.c_int), ("high", ctypes.c_int)]


class HoughParams(ctypes.Structure):
    """bugseg_hough_params: image_processing_utils.hough_params builds and checks them."""
    _fields_ = [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("numangle", ctypes.c_int), ("numrho", ctypes.c_int),
                ("threshold", ctypes.c_int), ("max_lines", ctypes.c_int), ("rho", ctypes.c_float),
                ("theta", ctypes.c_float), ("min_theta", ctypes.c_float)]


class QuadParams(ctypes.Structure):
    """bugseg_quad_params: calibration.quad_params builds and checks them."""
    _fields_ = [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("channels", ctypes.c_int), ("bright", ctypes.c_int),
                ("threshold", ctypes.c_int), ("min_area", ctypes.c_int), ("band", ctypes.c_int * 2)]


class MapParams(ctypes.Structure):
    """bugseg_map_params: mapping.map_params builds and checks them."""
    _fields_ = [("map_rows", ctypes.c_int), ("map_cols", ctypes.c_int), ("grid_rows", ctypes.c_int),
                ("grid_cols", ctypes.c_int), ("ros_layout", ctypes.c_int), ("l_occ", ctypes.c_int),
                ("l_free", ctypes.c_int), ("l_min", ctypes.c_int), ("l_max", ctypes.c_int), ("cull", ctypes.c_int)]


class ConfusionParams(ctypes.Structure):
    """bugseg_confusion_params: evaluate.confusion_params builds and checks them."""
    _fields_ = [("pred_rows", ctypes.c_int), ("pred_cols", ctypes.c_int), ("gt_rows", ctypes.c_int),
                ("gt_cols", ctypes.c_int), ("num_classes", ctypes.c_int), ("pred_lut", ctypes.c_uint8 * 256),
                ("gt_lut", ctypes.c_uint8 * 256)]


class BugsegError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bugseg error {code}: {msg}")
        self.code = code


_lib = None
_lock = threading.Lock()


def load_library(path: Path | str | None = None) -> ctypes.CDLL:
    """Load (once) and prototype libbugseg.so. Raises if it is missing."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = Path(path) if path else LIB_PATH
        if not p.exists():
            raise FileNotFoundError(f"{p} not found: build it with `python -m bugcar_image_segmentation_amd.build` "
                                    "(or __graft_entry__.build())")
        lib = ctypes.CDLL(str(p))
        vp, i, sz, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p
        proto = {
            "bugseg_version": (i, []),
            "bugseg_create": (i, [i, i, ctypes.POINTER(vp)]),
            "bugseg_destroy": (i, [vp]),
            "bugseg_load_weights": (i, [vp, vp, sz]),
            "bugseg_num_classes": (i, [vp]),
            "bugseg_input_bytes": (sz, [vp, i, i, i]),
            "bugseg_preprocess": (i, [vp, vp, i, i, i, i, i, i, vp, vp]),
            "bugseg_nchw_to_input": (i, [vp, vp, i, i, i, i, vp, vp]),
            "bugseg_enet_forward": (i, [vp, vp, i, i, i, i, vp, vp]),
            "bugseg_enet_forward_bgr": (i, [vp, vp, i, i, i, i, vp, vp]),
            "bugseg_enet_forward_bgr_ops": (i, [vp, vp, i, i, i, i, vp, i, i, vp]),
            "bugseg_enet_forward_bgr_rows": (i, [vp, vp, i, i, i, i, vp, i, i, i, i, vp]),
            "bugseg_bev_source_rows": (i, [vp, ctypes.POINTER(BevParams), i, i, ctypes.POINTER(i), ctypes.POINTER(i)]),
            "bugseg_debug_row_windows": (i, [i, i, i, i, i, i, vp]),
            "bugseg_debug_poison_arena": (i, [vp, i, vp]),
            "bugseg_debug_stage3_windows": (i, [i, i, i, i, vp, vp]),
            "bugseg_debug_plan_windows": (i, [vp, i, i, vp]),
            "bugseg_debug_read_block_output": (i, [vp, i, vp, sz, vp]),
            "bugseg_debug_pair_walk": (i, [i, vp, i, i, vp]),
            "bugseg_debug_pair_plan": (i, [vp, vp, i]),
            "bugseg_bev_occgrid": (i, [vp, vp, i, ctypes.POINTER(BevParams), vp, vp]),
            "bugseg_bev_workspace_bytes": (sz, [ctypes.POINTER(BevParams), i]),
            "bugseg_bev_occgrid_ws": (i, [vp, vp, i, ctypes.POINTER(BevParams), vp, vp, sz, vp]),
            "bugseg_plan_info": (i, [vp, i, i, i, i, i, ctypes.POINTER(i), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
            "bugseg_plan_op": (i, [vp, i, i, i, i, cp, i, ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
            "bugseg_plan_launch_op": (i, [vp, i, i, i, i, vp]),
            "bugseg_last_error": (cp, [vp]),
            "bugseg_road_filter_workspace_bytes": (sz, [ctypes.POINTER(RoadFilterParams), i]),
            "bugseg_road_filter": (i, [vp, vp, i, ctypes.POINTER(RoadFilterParams), vp, vp, sz, vp]),
            "bugseg_debug_road_filter_ops": (i, [vp, vp, i, ctypes.POINTER(RoadFilterParams), vp, vp, sz, i, i, vp]),
            "bugseg_clahe_workspace_bytes": (sz, [ctypes.POINTER(ClaheParams), i]),
            "bugseg_clahe_bgr": (i, [vp, vp, i, ctypes.POINTER(ClaheParams), vp, vp, sz, vp]),
            "bugseg_debug_clahe_stage": (i, [vp, vp, i, ctypes.POINTER(ClaheParams), i, vp, vp, sz, vp]),
            "bugseg_debug_clahe_table": (i, [i, vp, sz]),
            "bugseg_canny_workspace_bytes": (sz, [ctypes.POINTER(CannyParams), i]),
            "bugseg_canny": (i, [vp, vp, i, ctypes.POINTER(CannyParams), vp, vp, sz, vp]),
            "bugseg_debug_canny_stage": (i, [vp, vp, i, ctypes.POINTER(CannyParams), i, vp, vp, sz, vp]),
            "bugseg_confusion": (i, [vp, vp, vp, i, ctypes.POINTER(ConfusionParams), vp, vp]),
            "bugseg_bev_warp_image": (i, [vp, vp, i, i, ctypes.POINTER(BevParams), i, vp, vp]),
            "bugseg_hough_trig": (i, [ctypes.POINTER(HoughParams), vp]),
            "bugseg_hough_workspace_bytes": (sz, [ctypes.POINTER(HoughParams), i]),
            "bugseg_hough_lines": (i, [vp, vp, i, ctypes.POINTER(HoughParams), vp, vp, vp, vp, vp, sz, vp]),
            "bugseg_debug_hough_stage": (i, [vp, vp, i, ctypes.POINTER(HoughParams), vp, i, vp, vp, vp, vp, vp, sz, vp]),
            "bugseg_quad_workspace_bytes": (sz, [ctypes.POINTER(QuadParams), i]),
            "bugseg_find_quad": (i, [vp, vp, i, ctypes.POINTER(QuadParams), vp, vp, vp, vp, vp, vp, vp, sz, vp]),
            "bugseg_quad_moments": (i, [vp, vp, i, ctypes.POINTER(QuadParams), i, vp, vp, vp, sz, vp]),
            "bugseg_debug_quad_stage": (i, [vp, vp, i, ctypes.POINTER(QuadParams), i, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
            "bugseg_map_fuse": (i, [vp, vp, i, ctypes.POINTER(MapParams), vp, vp, vp, vp, vp]),
            "bugseg_dl_create": (i, [i, i, ctypes.POINTER(vp)]),
            "bugseg_dl_destroy": (i, [vp]),
            "bugseg_dl_load_weights": (i, [vp, vp, sz]),
            "bugseg_dl_set_plan": (i, [vp, vp, i, vp, i, i, i, i]),
            "bugseg_dl_forward": (i, [vp, vp, i, i, i, vp, vp]),
            "bugseg_dl_set_class_lut": (i, [vp, vp, i]),
            "bugseg_dl_forward_classes": (i, [vp, vp, i, i, i, i, vp, i, i, vp]),
            "bugseg_dl_classes_from_logits": (i, [vp, i, i, i, vp, i, i, vp]),
            "bugseg_dl_launch_op": (i, [vp, i, vp]),
            "bugseg_dl_read_buffer": (i, [vp, i, vp, sz, vp]),
            "bugseg_dl_last_error": (cp, [vp]),
            "bugseg_debug_parse_pack": (i, [vp, sz, i, ctypes.POINTER(i)]),
            "bugseg_debug_polar_tables": (i, [i, i, i, vp, sz, vp, sz, ctypes.POINTER(i), ctypes.POINTER(i)]),
            "bugseg_debug_ctx_info": (i, [vp, i, i]),
            "bugseg_debug_tile_walk": (i, [i, i, i, vp, sz, vp]),
            "bugseg_debug_set_spans": (i, [vp, vp, i]),
            "bugseg_debug_pool_indices": (i, [vp, i, i, i, i, vp, sz, ctypes.POINTER(ctypes.c_int), vp]),
            "bugseg_dl_debug_check_plan": (i, [vp, i, vp, i, i, i, i, i, sz]),
            "bugseg_dl_debug_op_layout": (i, [i, vp, i]),
            "bugseg_dl_debug_plan_groups": (i, [vp, i, vp]),
            "bugseg_debug_knobs": (i, [vp, vp, i]),
            "bugseg_dl_debug_knobs": (i, [vp, vp, i]),
            "bugseg_debug_fused_forms": (i, [vp, i]),
        }
        for name, (res, args) in proto.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _lib = lib
        return lib


def check(code: int, ctx=None) -> None:
    if code != OK:
        lib = load_library()
        msg = lib.bugseg_last_error(ctx).decode(errors="replace")
        if code == EINVAL:
            raise ValueError(msg)
        raise BugsegError(code, msg)


def knobs(ctx=None, size: int = 4096, dl: bool = False) -> dict[str, int]:
    """Test hook (bugseg_debug_knobs / bugseg_dl_debug_knobs): the BUGSEG_* run-time knobs as {name: value}:
    those the context handle `ctx` was created with, or (None; host only, no device) those of the environment
    as it is now. A bad value, or a `size`-byte buffer too small for the dump, raises ValueError."""
    lib = load_library()
    buf = ctypes.create_string_buffer(size)
    if dl:
        rc = lib.bugseg_dl_debug_knobs(ctx, buf, size)
        if rc != OK:
            raise (ValueError if rc == EINVAL else RuntimeError)(lib.bugseg_dl_last_error(ctx).decode(errors="replace"))
    else:
        check(lib.bugseg_debug_knobs(ctx, buf, size), ctx)
    return {k: int(v) for k, v in (line.split("=") for line in buf.value.decode().splitlines())}


def _dl_check(code: int) -> None:
    """A host-only bugseg_dl_debug_* hook's return code (its message: bugseg_dl_last_error(NULL))."""
    if code < 0:
        msg = load_library().bugseg_dl_last_error(None).decode(errors="replace")
        raise ValueError(msg) if code == EINVAL else BugsegError(code, msg)


def dl_op_layout(kind: int) -> tuple[str, ...]:
    """Test hook (bugseg_dl_debug_op_layout, host only): the executor's names of the fields after the kind in a
    DeepLab op record of `kind` (csrc/deeplab_ops.h); deeplab_spec.OP_LAYOUT is the writer's copy."""
    buf = ctypes.create_string_buffer(1024)
    n = load_library().bugseg_dl_debug_op_layout(int(kind), buf, len(buf))
    _dl_check(n)
    names = tuple(buf.value.decode().split(","))
    assert len(names) == n
    return names


def dl_check_plan(ops, buf_bytes, B: int, Hc: int, Wc: int, precision: int, w_bytes: int) -> None:
    """Test hook (bugseg_dl_debug_check_plan, host only): bugseg_dl_set_plan's validation; ValueError with its text."""
    import numpy as np
    o = np.ascontiguousarray(ops, dtype=np.int32)
    b = np.ascontiguousarray(buf_bytes, dtype=np.uint64)
    _dl_check(load_library().bugseg_dl_debug_check_plan(o.ctypes.data, o.shape[0], b.ctypes.data, b.shape[0], B, Hc, Wc,
                                                        precision, w_bytes))


def dl_plan_groups(ops) -> list[int]:
    """Test hook (bugseg_dl_debug_plan_groups, host only): per op, how many consecutive CONV ops from it a forward
    issues as one launch (1: alone)."""
    import numpy as np
    o = np.ascontiguousarray(ops, dtype=np.int32)
    runs = np.zeros(o.shape[0], np.int32)
    _dl_check(load_library().bugseg_dl_debug_plan_groups(o.ctypes.data, o.shape[0], runs.ctypes.data))
    return runs.tolist()


FORM_COLS = ("kind", "precision", "C", "asym", "variant", "transposed", "cin", "windowed", "lut_kind", "threads",
             "lds_bytes", "TH", "TW", "NW", "RD", "keep")


def fused_forms() -> list[dict[str, int]]:
    """Test hook (bugseg_debug_fused_forms, host only): one {column: value} row per built form of the fused
    bottleneck (kind 0) and upsampling (kind 1) kernels, columns FORM_COLS (include/bugseg.h)."""
    lib = load_library()
    n = lib.bugseg_debug_fused_forms(None, 0)
    if n < 0:
        check(n)
    rows = (ctypes.c_int32 * (n * len(FORM_COLS)))()
    if lib.bugseg_debug_fused_forms(rows, n) != n:
        raise RuntimeError("bugseg_debug_fused_forms: the form count changed between two calls")
    return [dict(zip(FORM_COLS, rows[k * len(FORM_COLS):(k + 1) * len(FORM_COLS)])) for k in range(n)]


def tile_walk(ntiles: int, grid: int, rev: int) -> list[list[int]]:
    """Test hook (bugseg_debug_tile_walk, host only): per workgroup of a `grid`-workgroup launch over
    `ntiles` tiles, the tiles it visits, in order (rev 0 ascending, 1 descending)."""
    lib = load_library()
    per_max = (ntiles + 7) // 8                 # no workgroup walks more than its XCD group's run
    seq = (ctypes.c_int32 * (grid * per_max))()
    count = (ctypes.c_int32 * grid)()
    per = lib.bugseg_debug_tile_walk(ntiles, grid, rev, seq, len(seq), count)
    if per < 0:
        check(per)
    return [list(seq[b * per:b * per + count[b]]) for b in range(grid)]


def row_windows(H: int, W: int, row0: int, row1: int, tile_rows_c64: int = 8, tile_rows_c16: int = 16) -> list[tuple[int, int]]:
    """Test hook (bugseg_debug_row_windows, host only): the half-open rows each of the forward's last six
    launches runs for class rows [row0, row1) of an H x W frame, on the launch's own grid (include/bugseg.h)."""
    lib = load_library()
    win = (ctypes.c_int32 * 12)()
    check(lib.bugseg_debug_row_windows(H, W, row0, row1, tile_rows_c64, tile_rows_c16, win))
    return [(win[2 * k], win[2 * k + 1]) for k in range(6)]


def stage3_windows(h: int, y0: int, y1: int, blocks) -> list[tuple[int, int]]:
    """Test hook (bugseg_debug_stage3_windows, host only): the output rows each stage-3 block runs when the
    128 -> 64 block reads rows [y0, y1) of the h-row stage-3 output. blocks: per block, nearest the decoder
    first, (asymmetric, dilation, row-dilated tiles, rows of its full-frame launch, rows per windowed tile row).
    The list ends where the walk stops (include/bugseg.h)."""
    lib = load_library()
    flat = [int(v) for b in blocks for v in b]
    blk = (ctypes.c_int32 * max(1, len(flat)))(*flat)
    win = (ctypes.c_int32 * max(1, 2 * len(blocks)))()
    m = lib.bugseg_debug_stage3_windows(h, y0, y1, len(blocks), blk, win)
    if m < 0:
        check(m)
    return [(win[2 * k], win[2 * k + 1]) for k in range(m)]


def pair_walk(cands, first_op: int = 0, last_op: int = -1):
    """Test hook (bugseg_debug_pair_walk, host only): the pair overlay's walk over a plan described per op by
    (candidate, grid rows, grid columns, buffer read, buffer written), for a forward over ops [first_op, last_op).
    -> (number of pairs, [(action, flip) per op]); the actions are listed in include/bugseg.h."""
    lib = load_library()
    n = len(cands)
    flat = [int(v) for c in cands for v in c]
    cand = (ctypes.c_int32 * max(1, len(flat)))(*flat)
    out = (ctypes.c_int32 * max(1, 2 * n))()
    m = lib.bugseg_debug_pair_walk(n, cand, first_op, n if last_op < 0 else last_op, out)
    if m < 0:
        check(m)
    return m, [(out[2 * k], out[2 * k + 1]) for k in range(n)]


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("bugseg needs a HIP GPU (MI355X / gfx950); none is visible — there is no CPU fallback")


def stream_handle(stream: torch.cuda.Stream | None = None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


class Context:
    """Owns one bugseg_ctx (device + precision + weights + activation arena)."""

    def __init__(self, device: int | None = None, precision: int = FP32):
        require_gpu()
        self.lib = load_library()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.precision = precision
        h = ctypes.c_void_p()
        check(self.lib.bugseg_create(self.device, precision, ctypes.byref(h)))
        self.h = h

    def close(self) -> None:
        if getattr(self, "h", None) and self.h.value:
            self.lib.bugseg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            # (destroying synchronises the device and frees memory, which would end a capture in progress:
            # a context the collector finalizes there is left to the process's end instead)
            if not torch.cuda.is_current_stream_capturing():
                self.close()
        except Exception:
            pass

    def load_weights(self, blob: bytes) -> None:
        buf = ctypes.create_string_buffer(blob, len(blob))
        check(self.lib.bugseg_load_weights(self.h, buf, len(blob)), self.h)

    @property
    def num_classes(self) -> int:
        return int(self.lib.bugseg_num_classes(self.h))

    def input_bytes(self, B: int, H: int, W: int) -> int:
        return int(self.lib.bugseg_input_bytes(self.h, B, H, W))

    def preprocess(self, bgr, B, H0, W0, H, W, layout, out, stream=None):
        check(self.lib.bugseg_preprocess(self.h, bgr.data_ptr(), B, H0, W0, H, W, layout, out.data_ptr(),
                                         stream_handle(stream)), self.h)

    def nchw_to_input(self, x, B, H, W, out, stream=None):
        check(self.lib.bugseg_nchw_to_input(self.h, x.data_ptr(), int(x.dtype == torch.float64), B, H, W,
                                            out.data_ptr(), stream_handle(stream)), self.h)

    def forward(self, x, B, H, W, out_kind, out, stream=None):
        check(self.lib.bugseg_enet_forward(self.h, x.data_ptr(), B, H, W, out_kind, out.data_ptr(),
                                           stream_handle(stream)), self.h)

    def forward_bgr(self, bgr, B, H, W, out_kind, out, stream=None):
        check(self.lib.bugseg_enet_forward_bgr(self.h, bgr.data_ptr(), B, H, W, out_kind, out.data_ptr(),
                                               stream_handle(stream)), self.h)

    def forward_bgr_ops(self, bgr, B, H, W, out_kind, out, first_op, last_op, stream=None):
        """Launches [first_op, last_op) of forward_bgr's plan only (last_op = -1: to the end)."""
        check(self.lib.bugseg_enet_forward_bgr_ops(self.h, bgr.data_ptr(), B, H, W, out_kind, out.data_ptr(),
                                                   first_op, last_op, stream_handle(stream)), self.h)

    def forward_bgr_rows(self, bgr, B, H, W, out_kind, out, rows, first_op=0, last_op=-1, stream=None):
        """forward_bgr_ops writing only output rows rows = (row0, row1) of every frame: the decoder's last
        six launches run just the tiles those rows need (bugseg_enet_forward_bgr_rows); the other rows of
        `out` are not written."""
        check(self.lib.bugseg_enet_forward_bgr_rows(self.h, bgr.data_ptr(), B, H, W, out_kind, out.data_ptr(),
                                                    int(rows[0]), int(rows[1]), first_op, last_op,
                                                    stream_handle(stream)), self.h)

    def bev_source_rows(self, params: BevParams, rows: int, cols: int) -> tuple[int, int]:
        """The half-open class-map rows the rasteriser's result depends on for these parameters
        (bugseg_bev_source_rows; builds the geometry's tap table if it is missing). (0, 0): none."""
        r0, r1 = ctypes.c_int(0), ctypes.c_int(0)
        check(self.lib.bugseg_bev_source_rows(self.h, ctypes.byref(params), rows, cols, ctypes.byref(r0),
                                              ctypes.byref(r1)), self.h)
        return r0.value, r1.value

    def poison_arena(self, byte: int, stream=None) -> None:
        """Test hook (bugseg_debug_poison_arena): fill the activation arena and pooling indices with `byte`."""
        check(self.lib.bugseg_debug_poison_arena(self.h, int(byte), ctypes.c_void_p(stream_handle(stream))), self.h)

    def plan_windows(self, rows) -> list[tuple[int, int, int, int, int]]:
        """Test hook (bugseg_debug_plan_windows): the stage-3 windows the current plan runs for class rows
        rows = (row0, row1), nearest the decoder first: (plan op, first row, end row, tile variant, tiles per frame)."""
        win = (ctypes.c_int32 * 10)()
        m = self.lib.bugseg_debug_plan_windows(self.h, int(rows[0]), int(rows[1]), win)
        if m < 0:
            check(m, self.h)
        return [tuple(win[5 * k:5 * k + 5]) for k in range(m)]

    def pair_plan(self) -> list[tuple[int, ...]]:
        """Test hook (bugseg_debug_pair_plan): the current plan's paired launches, one row each: (first op, tile rows,
        tile columns, tiles_y, tiles_x, threads, LDS bytes, flip of the first op)."""
        rows = (ctypes.c_int32 * (8 * 16))()
        m = self.lib.bugseg_debug_pair_plan(self.h, rows, 16)
        if m < 0:
            check(m, self.h)
        return [tuple(rows[8 * k:8 * k + 8]) for k in range(min(m, 16))]

    def read_block_output(self, op: int, out, stream=None) -> None:
        """Test hook (bugseg_debug_read_block_output): the output of fused bottleneck launch `op` into `out`."""
        check(self.lib.bugseg_debug_read_block_output(self.h, op, out.data_ptr(), out.numel() * out.element_size(),
                                                      ctypes.c_void_p(stream_handle(stream))), self.h)

    def _stream_ws(self, x, stream, workspace=None, size_fn=None, params=None, B=0):
        """-> (stream handle, (workspace pointer, bytes), the workspace tensor: keep it until the call is enqueued)
        for an operator on `x`'s device. The stream is `stream` or the current one; the workspace is `workspace`
        or, given size_fn, size_fn(params, B) bytes from torch's caching allocator on that stream (reuse is
        stream-ordered; under graph capture it is the graph's pool)."""
        st = stream if stream is not None else torch.cuda.current_stream(x.device)
        ws = workspace
        nws = int(size_fn(ctypes.byref(params), B)) if ws is None and size_fn is not None else 0
        if nws:
            with torch.cuda.stream(st):
                ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
        return stream_handle(st), ((0, 0) if ws is None else (ws.data_ptr(), ws.numel() * ws.element_size())), ws

    def _raise_any(self, rc: int) -> None:
        """BugsegError for any non-zero code (check() turns EINVAL into ValueError)."""
        if rc != OK:
            raise BugsegError(rc, self.lib.bugseg_last_error(self.h).decode(errors="replace"))

    def bev(self, seg, B, params: BevParams, out, stream=None):
        """bugseg_bev_occgrid_ws: the laserscan scratch comes from torch's caching allocator on the
        stream the work runs on (reuse is stream-ordered; under graph capture it is the graph's pool),
        so the library never allocates or synchronises for it."""
        sh, w, _keep = self._stream_ws(seg, stream, None, self.lib.bugseg_bev_workspace_bytes, params, B)
        check(self.lib.bugseg_bev_occgrid_ws(self.h, seg.data_ptr(), B, ctypes.byref(params), out.data_ptr(), *w, sh),
              self.h)

    def road_filter(self, seg, B, params: RoadFilterParams, out, stream=None, ops=None, workspace=None):
        """bugseg_road_filter: the workspace comes from torch's caching allocator on the stream the work
        runs on, as in bev (`workspace`: a uint8 device tensor to use instead). ops = (first, last) enqueues
        only those launches (bugseg_debug_road_filter_ops, the benchmark's per-kernel times). Any refusal,
        a bad argument included, raises BugsegError and launches nothing."""
        sh, w, _keep = self._stream_ws(seg, stream, workspace, self.lib.bugseg_road_filter_workspace_bytes, params, B)
        if ops is None:
            rc = self.lib.bugseg_road_filter(self.h, seg.data_ptr(), B, ctypes.byref(params), out.data_ptr(), *w, sh)
        else:
            rc = self.lib.bugseg_debug_road_filter_ops(self.h, seg.data_ptr(), B, ctypes.byref(params), out.data_ptr(),
                                                       *w, int(ops[0]), int(ops[1]), sh)
        self._raise_any(rc)

    def clahe(self, frames, B, params: ClaheParams, out, stream=None, stage=None, workspace=None):
        """bugseg_clahe_bgr: (B, rows, cols, 3) u8 BGR frames -> `out`, the same shape. The workspace (the tile
        look-up tables) comes from torch's caching allocator on the stream the work runs on, as in road_filter
        (`workspace`: a uint8 device tensor to use instead). stage = 0..4 enqueues that stage alone
        (bugseg_debug_clahe_stage: the tests' and the benchmark's view of the parts; `out` may be None for
        stage 3). Any refusal, a bad argument included, raises BugsegError and launches nothing."""
        size_fn = None if stage in (0, 1, 2) else self.lib.bugseg_clahe_workspace_bytes    # (stages 0-2 use none)
        sh, w, _keep = self._stream_ws(frames, stream, workspace, size_fn, params, B)
        op = 0 if out is None else out.data_ptr()
        if stage is None:
            rc = self.lib.bugseg_clahe_bgr(self.h, frames.data_ptr(), B, ctypes.byref(params), op, *w, sh)
        else:
            rc = self.lib.bugseg_debug_clahe_stage(self.h, frames.data_ptr(), B, ctypes.byref(params), int(stage), op,
                                                   *w, sh)
        self._raise_any(rc)

    def canny(self, images, B, params: CannyParams, out, stream=None, stage=None, workspace=None):
        """bugseg_canny: (B, rows, cols) u8 images -> `out`, the same shape, in {0, 255}. The workspace comes
        from torch's caching allocator on the stream the work runs on, as in road_filter (`workspace`: a uint8
        device tensor to use instead). stage = 0 or 1 enqueues that half alone (bugseg_debug_canny_stage: 0
        writes the non-maximum-suppression map to `out`, 1 reads `images` as such a map). Any refusal, a bad
        argument included, raises BugsegError and launches nothing."""
        sh, w, _keep = self._stream_ws(images, stream, workspace, self.lib.bugseg_canny_workspace_bytes, params, B)
        if stage is None:
            rc = self.lib.bugseg_canny(self.h, images.data_ptr(), B, ctypes.byref(params), out.data_ptr(), *w, sh)
        else:
            rc = self.lib.bugseg_debug_canny_stage(self.h, images.data_ptr(), B, ctypes.byref(params), int(stage),
                                                   out.data_ptr(), *w, sh)
        self._raise_any(rc)

    def confusion(self, pred, gt, B, params: ConfusionParams, acc, stream=None):
        """bugseg_confusion: (B, pred_rows, pred_cols) u8 predictions against (B, gt_rows, gt_cols) u8 labels,
        added into `acc`, an int64 device tensor of num_classes^2 + 1 words (the matrix row by row, rows =
        labels, then the skipped pixels). One launch, no workspace. Any refusal, a bad argument included,
        raises BugsegError and launches nothing."""
        sh, _, _ = self._stream_ws(gt, stream)
        self._raise_any(self.lib.bugseg_confusion(self.h, pred.data_ptr(), gt.data_ptr(), B, ctypes.byref(params),
                                                  acc.data_ptr(), sh))

    def warp_image(self, frames, B, channels, params: BevParams, gray, out, stream=None):
        """bugseg_bev_warp_image: (B, in_rows, in_cols[, 3]) u8 frames -> `out`, (B, warp_h, warp_w[, 3]) u8 (one
        byte per pixel with gray). One launch, no workspace. A bad argument raises ValueError (as bev) and
        launches nothing."""
        sh, _, _ = self._stream_ws(frames, stream)
        check(self.lib.bugseg_bev_warp_image(self.h, frames.data_ptr(), B, int(channels), ctypes.byref(params),
                                             int(gray), out.data_ptr(), sh), self.h)

    def hough(self, images, B, params: HoughParams, trig, lines, counts, peaks, stream=None, stage=None, acc=None,
              workspace=None):
        """bugseg_hough_lines: (B, rows, cols) u8 images and the device copy of the trig table -> lines
        (B, max_lines, 2) float32, counts and peaks (B,) int32. The workspace comes from torch's caching allocator
        on the stream the work runs on, as in road_filter (`workspace`: a uint8 device tensor to use instead).
        stage = 0 or 1 enqueues that half alone (bugseg_debug_hough_stage: 0 writes the accumulators to `acc`,
        1 reads them from it; the arguments a stage does not use may be None). Any refusal, a bad argument
        included, raises BugsegError and launches nothing."""
        ref = next(t for t in (images, acc, lines) if t is not None)
        sh, w, _keep = self._stream_ws(ref, stream, workspace, self.lib.bugseg_hough_workspace_bytes, params, B)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        if stage is None:
            rc = self.lib.bugseg_hough_lines(self.h, ptr(images), B, ctypes.byref(params), ptr(trig), ptr(lines),
                                             ptr(counts), ptr(peaks), *w, sh)
        else:
            rc = self.lib.bugseg_debug_hough_stage(self.h, ptr(images), B, ctypes.byref(params), ptr(trig), int(stage),
                                                   ptr(acc), ptr(lines), ptr(counts), ptr(peaks), *w, sh)
        self._raise_any(rc)

    def find_quad(self, frames, B, params: QuadParams, status, threshold, area, root, corners, moments, stream=None,
                  stage=None, workspace=None):
        """bugseg_find_quad: (B, rows, cols[, 3]) u8 frames -> status, threshold, area, root (B,) int32, corners
        (B, 4, 2) int32, moments (B, 4, 6) int64. The workspace comes from torch's caching allocator on the stream
        the work runs on, as in road_filter (`workspace`: a uint8 device tensor to use instead). stage = 0..11
        enqueues that launch alone (bugseg_debug_quad_stage: the benchmark's per-launch times). Any refusal, a bad
        argument included, raises BugsegError and launches nothing."""
        ref = next(t for t in (frames, moments, corners, status) if t is not None)
        sh, w, _keep = self._stream_ws(ref, stream, workspace, self.lib.bugseg_quad_workspace_bytes, params, B)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        outs = [ptr(t) for t in (status, threshold, area, root, corners, moments)]
        if stage is None:
            rc = self.lib.bugseg_find_quad(self.h, ptr(frames), B, ctypes.byref(params), *outs, *w, sh)
        else:
            rc = self.lib.bugseg_debug_quad_stage(self.h, ptr(frames), B, ctypes.byref(params), int(stage), *outs, *w, sh)
        self._raise_any(rc)

    def quad_moments(self, frames, B, params: QuadParams, band, corners2, moments, stream=None, workspace=None):
        """bugseg_quad_moments: the side moments of the frames' tile regions for the doubled corners `corners2`
        (B, 4, 2) int32 -> moments (B, 4, 6) int64. Workspace and refusals as find_quad."""
        sh, w, _keep = self._stream_ws(frames, stream, workspace, self.lib.bugseg_quad_workspace_bytes, params, B)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        self._raise_any(self.lib.bugseg_quad_moments(self.h, ptr(frames), B, ctypes.byref(params), int(band), ptr(corners2),
                                                     ptr(moments), *w, sh))

    def map_fuse(self, grids, B, params: MapParams, record, state, lut, out, stream=None):
        """bugseg_map_fuse: (B, h, w) int8 grids and the update record (int64 words, mapping.pose_record) -> the
        int16 torus `state` (Hm, Wm) and the int8 payload `out` (Hm, Wm). One launch, no workspace. Any refusal, a
        bad argument included, raises BugsegError and launches nothing."""
        sh, _, _ = self._stream_ws(out if out is not None else state, stream)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        self._raise_any(self.lib.bugseg_map_fuse(self.h, ptr(grids), B, ctypes.byref(params), ptr(record), ptr(state),
                                                 ptr(lut), ptr(out), sh))

    def plan_info(self, B, H, W, out_kind, bgr_input=False):
        """-> (launches, per-layer algorithmic bytes, plan compulsory bytes, flops) of one forward."""
        n = ctypes.c_int()
        lb = ctypes.c_double()
        pb = ctypes.c_double()
        fl = ctypes.c_double()
        check(self.lib.bugseg_plan_info(self.h, B, H, W, out_kind, int(bool(bgr_input)), ctypes.byref(n),
                                        ctypes.byref(lb), ctypes.byref(pb), ctypes.byref(fl)), self.h)
        return n.value, lb.value, pb.value, fl.value

    def plan_op(self, B, H, W, op):
        """Profiling hook: -> (kernel tag, per-layer algorithmic bytes, bytes the launch moves, flops)
        of launch `op` of the plan the last forward at (B, H, W) ran."""
        buf = ctypes.create_string_buffer(64)
        lb, pb, fl = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(self.lib.bugseg_plan_op(self.h, B, H, W, op, buf, 64, ctypes.byref(lb), ctypes.byref(pb),
                                      ctypes.byref(fl)), self.h)
        return buf.value.decode(), lb.value, pb.value, fl.value

    def launch_op(self, B, H, W, op, stream=None):
        """Profiling hook: enqueue launch `op` of that plan alone (its buffers must still be alive)."""
        check(self.lib.bugseg_plan_launch_op(self.h, B, H, W, op, ctypes.c_void_p(stream_handle(stream))), self.h)

    def debug_info(self, what: int, arg: int = 0) -> int:
        """Test hook (bugseg_debug_ctx_info): 0 = exact affine byte normalisation in use, 1 = fp32 range
        scaling off, 2 = weight exponent of packed convolution `arg`."""
        return int(self.lib.bugseg_debug_ctx_info(self.h, what, arg))

    def knobs(self) -> dict[str, int]:
        """The BUGSEG_* knobs this context was created with (they never change afterwards)."""
        return knobs(self.h)

    def set_spans(self, spans=None):
        """Measurement hook (bugseg_debug_set_spans): a CUDA int64 tensor of 512 words per plan op (64
        [entry, exit] slots, 64 B apart) that later launches fold their clock into (None disarms); ops
        beyond the tensor's size are never armed."""
        if spans is None:
            check(self.lib.bugseg_debug_set_spans(self.h, ctypes.c_void_p(0), 0), self.h)
            return
        if not spans.is_cuda or spans.dtype != torch.int64 or not spans.is_contiguous() or spans.numel() % 512:
            raise ValueError("spans must be a contiguous CUDA int64 tensor of 512 words per op")
        check(self.lib.bugseg_debug_set_spans(self.h, ctypes.c_void_p(spans.data_ptr()), spans.numel() // 512), self.h)

    def pool_indices(self, B: int, H: int, W: int, block: int, shape: tuple, stream=None) -> torch.Tensor:
        """Test hook (bugseg_debug_pool_indices): the pooling indices the last forward at (B, H, W) wrote
        for downsampling block `block`, as a uint8 (B, h, w, idx_cs) device tensor; shape = (h, w, idx_cs)."""
        out = torch.empty((B,) + tuple(shape), dtype=torch.uint8, device=torch.device("cuda", self.device))
        cs = ctypes.c_int(0)
        check(self.lib.bugseg_debug_pool_indices(self.h, B, H, W, block, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                                 ctypes.byref(cs), ctypes.c_void_p(stream_handle(stream))), self.h)
        if cs.value != shape[-1]:
            raise ValueError(f"index tensor has channel stride {cs.value}, not {shape[-1]}")
        return out


_shared: dict[int, Context] = {}


def shared_context(device: int | None = None) -> Context:
    """Per-device context for the weight-free ops (preprocess classmethod, BEV rasteriser)."""
    require_gpu()
    d = torch.cuda.current_device() if device is None else int(device)
    with _lock:
        c = _shared.get(d)
    if c is None:
        c = Context(d, FP32)
        with _lock:
            _shared.setdefault(d, c)
            c = _shared[d]
    return c


class DeepLabContext:
    """Owns one bugseg_dl (DeepLabV3 executor: weights + op list + activation arena), include/bugseg.h."""

    def __init__(self, device: int | None = None, precision: int = BF16):
        require_gpu()
        self.lib = load_library()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.precision = precision
        h = ctypes.c_void_p()
        self._check(self.lib.bugseg_dl_create(self.device, precision, ctypes.byref(h)), None)
        self.h = h

    def _check(self, code, h):
        if code != OK:
            msg = self.lib.bugseg_dl_last_error(h).decode(errors="replace")
            if code == EINVAL:
                raise ValueError(msg)
            raise BugsegError(code, msg)

    def close(self) -> None:
        if getattr(self, "h", None) and self.h.value:
            self.lib.bugseg_dl_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            # (destroying synchronises the device and frees memory, which would end a capture in progress:
            # a context the collector finalizes there is left to the process's end instead)
            if not torch.cuda.is_current_stream_capturing():
                self.close()
        except Exception:
            pass

    def load_weights(self, blob: bytes) -> None:
        buf = ctypes.create_string_buffer(blob, len(blob))
        self._check(self.lib.bugseg_dl_load_weights(self.h, buf, len(blob)), self.h)

    def set_plan(self, ops, buf_bytes, B: int, Hc: int, Wc: int) -> None:
        import numpy as np
        o = np.ascontiguousarray(ops, dtype=np.int32)
        assert o.ndim == 2 and o.shape[1] == DL_OP_FIELDS
        b = np.ascontiguousarray(buf_bytes, dtype=np.uint64)
        self._check(self.lib.bugseg_dl_set_plan(self.h, o.ctypes.data, o.shape[0], b.ctypes.data, b.shape[0], B, Hc, Wc),
                    self.h)

    def forward(self, rgb, B, H, W, out, stream=None):
        self._check(self.lib.bugseg_dl_forward(self.h, rgb.data_ptr(), B, H, W, out.data_ptr(), stream_handle(stream)),
                    self.h)

    def set_class_lut(self, lut) -> None:
        """bugseg_dl_set_class_lut: the byte the u8 forms store per class id (a sequence of the plan's
        class count, at most 256 entries, each 0..255), or None for the identity. Uploaded here, once;
        synchronises the device, so never inside a stream capture."""
        if lut is None:
            self._check(self.lib.bugseg_dl_set_class_lut(self.h, None, 0), self.h)
            return
        b = bytes(bytearray(int(v) for v in lut))
        buf = ctypes.create_string_buffer(b, len(b))
        self._check(self.lib.bugseg_dl_set_class_lut(self.h, buf, len(b)), self.h)

    def forward_classes(self, img, bgr, B, H, W, seg, rows=None, stream=None):
        """bugseg_dl_forward_classes: (B, H, W, 3) u8 frames (bgr: their byte order is B, G, R) -> rows
        rows = (row0, row1) (None: all) of the (B, H, W) u8 map lut[class id]; other rows are not written."""
        r0, r1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
        self._check(self.lib.bugseg_dl_forward_classes(self.h, img.data_ptr(), int(bool(bgr)), B, H, W, seg.data_ptr(),
                                                       r0, r1, stream_handle(stream)), self.h)

    def classes_from_logits(self, B, H, W, seg, rows=None, stream=None):
        """bugseg_dl_classes_from_logits: the final op alone on the last forward's logits, rows as above."""
        r0, r1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
        self._check(self.lib.bugseg_dl_classes_from_logits(self.h, B, H, W, seg.data_ptr(), r0, r1,
                                                           stream_handle(stream)), self.h)

    def knobs(self) -> dict[str, int]:
        """The BUGSEG_* knobs this context was created with (they never change afterwards)."""
        return knobs(self.h, dl=True)

    def launch_op(self, op, stream=None):
        self._check(self.lib.bugseg_dl_launch_op(self.h, op, ctypes.c_void_p(stream_handle(stream))), self.h)

    def read_buffer(self, buf, out, stream=None):
        self._check(self.lib.bugseg_dl_read_buffer(self.h, buf, out.data_ptr(), out.numel() * out.element_size(),
                                                   ctypes.c_void_p(stream_handle(stream))), self.h)
