"""Print the compiler's resource table of the kernels in one HIP source: registers, scratch bytes, occupancy
and spilled registers per kernel (hipcc -Rpass-analysis=kernel-resource-usage; device code only, no GPU needed).

The fused bottleneck's fp32 forms sit at the SGPR limit, so small changes to scalar code (the tile walk,
DESIGN 6.10) move their VGPR count and scratch; this table is the check before a run.

usage: python scripts/kernel_resources.py [source.hip] [-DKNOB=1 ...]        (default bneck_kernels.hip)
       python scripts/kernel_resources.py --diff old.txt new.txt             (two saved tables)
"""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from bugcar_image_segmentation_amd.build import ARCH, CSRC, SOURCE_FLAGS, _hipcc  # noqa: E402

KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill")


def parse(text):
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for k in KEYS:
            m = re.search(rf"^\s*{k}( \[[^\]]*\])?: (\d+)", ln.split("remark:")[-1])
            if m and cur is not None:
                cur.setdefault(k, int(m.group(2)))
    return out


def table(src, defines):
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", f"-I{ROOT / 'include'}", f"-I{CSRC}", *defines,
           *SOURCE_FLAGS.get(Path(src).name, []), "-x", "hip", "-c", str(src), "-o", "/dev/null"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    return parse(r.stderr)


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else list(names)


def show(tab):
    print("| kernel | " + " | ".join(KEYS) + " |")
    print("|---|" + "---|" * len(KEYS))
    for name, short in zip(tab, demangle(tab)):
        print(f"| `{short.replace('bugseg::', '')}` | " + " | ".join(str(tab[name].get(k, "")) for k in KEYS) + " |")


def read_table(path):
    tab = {}
    for ln in Path(path).read_text().splitlines():
        c = [x.strip() for x in ln.strip("|").split("|")]
        if len(c) == len(KEYS) + 1 and c[0].startswith("`"):
            tab[c[0]] = dict(zip(KEYS, c[1:]))
    return tab


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--diff"]:
        a, b = read_table(args[1]), read_table(args[2])
        for k in a:
            if a[k] != b.get(k):
                print(k, a[k], "->", b.get(k))
    else:
        src = next((x for x in args if not x.startswith("-D")), "bneck_kernels.hip")
        show(table(CSRC / src if not Path(src).exists() else Path(src), [x for x in args if x.startswith("-D")]))
