"""Host ASan + UBSan over the native runtime's input-parsing paths (race /
memory-error detection on the host C++ build). tests/asan/build.sh compiles the host runtime's
translation units (csrc/*.cpp) and tests/asan/asan_driver.cpp with host-only sanitizers; the driver feeds the BSG1
weight-blob parser + BN folding + packing, the DeepLab plan validator and the polar-table builder
with valid inputs, truncations and seeded corruptions. CPU only: no device is touched."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "asan" / "_build"


def _stale(target, deps):
    return not target.exists() or any(Path(d).stat().st_mtime > target.stat().st_mtime for d in deps)


@pytest.fixture(scope="module")
def driver():
    if shutil.which("/opt/rocm/bin/hipcc") is None:
        pytest.skip("hipcc not available")
    exe = OUT / "asan_driver"
    csrc = ROOT / "bugcar_image_segmentation_amd" / "csrc"
    deps = [ROOT / "tests" / "asan" / "asan_driver.cpp", ROOT / "tests" / "asan" / "build.sh", ROOT / "include" / "bugseg.h",
            *csrc.glob("*.cpp"), *csrc.glob("*.h"), *csrc.glob("*.hip")]
    if _stale(exe, deps):
        r = subprocess.run(["bash", str(ROOT / "tests" / "asan" / "build.sh"), str(OUT)], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_runtime_parsers_under_asan_ubsan(driver, tmp_path):
    from bugcar_image_segmentation_amd import deeplab_spec, enet_spec
    (tmp_path / "enet.bsg1").write_bytes(enet_spec.serialize(enet_spec.build_enet()))
    net = deeplab_spec.build_deeplab(width=0.25, crop=65)
    B, prec = 2, 1
    blob, ops, bufs, _info = deeplab_spec.lower(net, B, True)
    np.ascontiguousarray(ops, dtype=np.int32).tofile(tmp_path / "ops.i32")
    np.ascontiguousarray(bufs, dtype=np.uint64).tofile(tmp_path / "bufs.u64")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(driver), str(tmp_path / "enet.bsg1"), str(tmp_path / "ops.i32"), str(tmp_path / "bufs.u64"),
                        str(B), str(net.crop), str(net.crop), str(len(blob)), str(prec)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "asan driver ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
