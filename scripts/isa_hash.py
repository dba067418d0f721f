"""Hash the device assembly of each kernel in one HIP source (hipcc --cuda-device-only -S; no GPU needed).

The check for a change that must not move device code (retiring a compile-time knob): save the
table before and after, and --diff prints the kernels whose code differs. Per kernel, the text from its label
to its .Lfunc_end and its .amdhsa_kernel descriptor (registers, LDS, scratch) are hashed, after comments are
stripped and the function's index is taken out of its local labels, so that a kernel does not "change" because
another one ahead of it in the file did. The text is only normalised and hashed, never searched.

usage: python scripts/isa_hash.py [source.hip] [-DKNOB=1 ...] > table.txt    (default bneck_kernels.hip)
       python scripts/isa_hash.py --diff old.txt new.txt
"""
import hashlib
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from bugcar_image_segmentation_amd.build import ARCH, CSRC, SOURCE_FLAGS, _hipcc  # noqa: E402


def assembly(src, defines):
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "--cuda-device-only", "-S",
           f"-I{ROOT / 'include'}", f"-I{CSRC}", *defines, *SOURCE_FLAGS.get(Path(src).name, []),
           "-x", "hip", str(src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    return r.stdout


def normalise(lines):
    out = []
    for ln in lines:
        ln = re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", ln.split(";")[0]).strip()
        if ln:
            out.append(ln)
    return "\n".join(out)


def hashes(text):
    """{kernel symbol: hash}. A kernel is a symbol that has an .amdhsa_kernel descriptor; the compiler writes the
    descriptor between the kernel's last instruction and its .Lfunc_end, so it is part of the hashed text."""
    lines = text.splitlines()
    label = {ln.split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"\w+:", ln)}
    out = {}
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            i = label[m.group(1)]
            j = next(k for k in range(i, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
            out[m.group(1)] = hashlib.sha256(normalise(lines[i + 1:j]).encode()).hexdigest()[:16]
    return out


def read_table(path):
    return dict(ln.split() for ln in Path(path).read_text().splitlines() if len(ln.split()) == 2)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--diff"]:
        a, b = read_table(args[1]), read_table(args[2])
        moved = [s for s in a if s in b and a[s] != b[s]]
        for s in sorted(set(a) ^ set(b)):
            print("only in", args[1] if s in a else args[2], s)
        for s in moved:
            print("differs", s)
        print(f"{len(moved)} of {len(a)} kernels differ, {len(set(a) ^ set(b))} symbols unmatched")
        sys.exit(1 if moved or set(a) ^ set(b) else 0)
    src = next((x for x in args if not x.startswith("-D")), "bneck_kernels.hip")
    tab = hashes(assembly(CSRC / src if not Path(src).exists() else Path(src), [x for x in args if x.startswith("-D")]))
    for s in sorted(tab):
        print(s, tab[s])
