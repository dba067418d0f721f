"""A/B timing of the fp32 C64 pair launches alone (bneck_pair_kernels.hip), for libraries built with other defines
(build_native(variant, defines), loaded through BUGSEG_LIB).

Runs fp32 forwards at batch B, then the first pair alone (two plan ops: the paired launch and two guards that return
at once; its input stays what the forward left) REPS times between two events, and prints the time per pair (its guards included) next to the
SHA-256 of the class map of a whole forward, which must not differ between libraries.

usage: [BUGSEG_LIB=...] python scripts/pair_time_probe.py [B] [REPS] [--once: no timing, for counter passes]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bugcar_image_segmentation_amd import _native as N  # noqa: E402
from bugcar_image_segmentation_amd import enet_spec, synthetic  # noqa: E402
from bugcar_image_segmentation_amd.models import ENET  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args else 64
REPS = int(args[1]) if len(args) > 1 else 40
H, W = 480, 640
m = ENET(weights=enet_spec.build_enet(), precision="fp32")
frames = torch.from_numpy(synthetic.uniform_frames(B, H, W)).cuda()
seg = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
for _ in range(1 if "--once" in sys.argv else 3):
    m.ctx.forward_bgr(frames, B, H, W, N.OUT_CLASS3_U8, seg)
torch.cuda.synchronize()
sha = hashlib.sha256(seg.cpu().numpy().tobytes()).hexdigest()[:16]
pairs = m.ctx.pair_plan()
first, last = pairs[0][0], pairs[0][0] + 2
name = os.path.basename(os.environ.get("BUGSEG_LIB", "libbugseg.so"))
if "--once" in sys.argv:
    for _ in range(3):
        m.ctx.forward_bgr_ops(frames, B, H, W, N.OUT_CLASS3_U8, seg, first, last)
    torch.cuda.synchronize()
    print(f"{name}: the first pair x 3, class map {sha}")
    sys.exit(0)
best = []
for _ in range(3):
    for _ in range(5):
        m.ctx.forward_bgr_ops(frames, B, H, W, N.OUT_CLASS3_U8, seg, first, last)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(REPS):
        m.ctx.forward_bgr_ops(frames, B, H, W, N.OUT_CLASS3_U8, seg, first, last)
    ev[1].record()
    torch.cuda.synchronize()
    best.append(ev[0].elapsed_time(ev[1]) * 1e3 / REPS)
print(f"{name}: B={B} pair {pairs[0][1]}x{pairs[0][2]} / {pairs[0][5]} threads: "
      + " / ".join(f"{t:.1f}" for t in best) + f" us per pair + 2 guards; class map {sha}", flush=True)
