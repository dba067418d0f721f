"""Debug: in-kernel phase clocks of the fp32 C64 pair kernel (bneck_pair_kernels.hip; a -DBUGSEG_STAMPS library).

Runs fp32 forwards at batch B, then the first pair alone (ops 2, 3 of the plan: the paired launch and its two
guards, which return at once) with the stamp buffer armed, and prints the mean shader-clock cycles of each tile
phase as wave 0 of the workgroup sees it:
  a1ld   A1's x loads, issue -> landed (with a prefetch: what is left of it at tile top)
  a1     A1's projections, t0_A (and the raw x) to LDS, barrier
  a23    A2 + A3: the 3x3, the expansion, y to LDS, barrier
  b1     B1: t0_B from y, barrier
  b23    B2 + B3: the 3x3, the expansion, the stores issued, barrier
and the HIP-event time of the three launches next to the tile count per workgroup.

usage: [BUGSEG_LIB=...] python scripts/pair_stamp_probe.py [B]   (build: python -m bugcar_image_segmentation_amd.build --stamps)"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BUGSEG_LIB", os.path.join(ROOT, "bugcar_image_segmentation_amd", "libbugseg_stamps.so"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bugcar_image_segmentation_amd import _native as N  # noqa: E402
from bugcar_image_segmentation_amd import enet_spec, synthetic  # noqa: E402
from bugcar_image_segmentation_amd.models import ENET  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
H, W = 480, 640
lib = N.load_library()
lib.bugseg_debug_set_stamps.argtypes = [ctypes.c_void_p]
m = ENET(weights=enet_spec.build_enet(), precision="fp32")
frames = torch.from_numpy(synthetic.uniform_frames(B, H, W)).cuda()
seg = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
for _ in range(3):
    m.ctx.forward_bgr(frames, B, H, W, N.OUT_CLASS3_U8, seg)
first = m.ctx.pair_plan()[0][0]
for _ in range(3):
    m.ctx.forward_bgr_ops(frames, B, H, W, N.OUT_CLASS3_U8, seg, first, first + 2)
stamps = torch.zeros(1 << 20, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
assert lib.bugseg_debug_set_stamps(ctypes.c_void_p(stamps.data_ptr())) == 0
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
m.ctx.forward_bgr_ops(frames, B, H, W, N.OUT_CLASS3_U8, seg, first, first + 2)
ev[1].record()
torch.cuda.synchronize()
assert lib.bugseg_debug_set_stamps(ctypes.c_void_p(0)) == 0
s = stamps.cpu().numpy()[:1 << 19].reshape(-1, 8)
s = s[s[:, 0] != 0]
d = np.diff(s[:, :6], axis=1).astype(np.float64)
names = ["a1ld", "a1", "a23", "b1", "b23"]
wg = s[:, 7].astype(np.int64)
per_wg = np.bincount(wg)
per_wg = per_wg[per_wg > 0]
print(f"{os.path.basename(os.environ['BUGSEG_LIB'])} B={B}: {len(s)} tiles on {len(per_wg)} WGs "
      f"({per_wg.min()}-{per_wg.max()} tiles/WG); pair + 2 guards {ev[0].elapsed_time(ev[1]) * 1e3:.1f} us; "
      f"tile {(s[:, 5] - s[:, 0]).mean():.0f} cyc (p10 {np.percentile(s[:, 5] - s[:, 0], 10):.0f}, p90 {np.percentile(s[:, 5] - s[:, 0], 90):.0f})")
print("  all tiles:   " + "  ".join(f"{nm}={d[:, k].mean():6.0f} (p90 {np.percentile(d[:, k], 90):6.0f})" for k, nm in enumerate(names)))
# a workgroup's first tile (no prefetch ahead of it, cold weights) apart from its later ones
order = np.lexsort((s[:, 0], wg))
isfirst = np.zeros(len(s), bool)
isfirst[order[np.r_[True, wg[order][1:] != wg[order][:-1]]]] = True
for nm, sel in (("first tiles", isfirst), ("later tiles", ~isfirst)):
    if sel.any():
        print(f"  {nm}: " + "  ".join(f"{n2}={d[sel, k].mean():6.0f}" for k, n2 in enumerate(names)))
