"""The built forms of the fused ENet bottleneck and upsampling kernels through the host-only
entry bugseg_debug_fused_forms: every form's threads, dynamic LDS bytes and tile shape equal the table below.

The table was dumped once, from the commit before the kernels and their launchers came to share one LDS
layout: there the launcher sized each allocation with a host formula of its own, and these are that formula's
numbers (and the old launchers' thread counts and tile shapes) for every kernel that commit instantiated. It is
a record, not a mirror: a change that moves a number here changes how much LDS a launch asks for, and so how
many workgroups fit a CU. `keep` is recorded where that commit's host code had an answer (bneck_keeps_c64: the
plain symmetric C = 64 forms); None elsewhere, and not compared."""
import pytest

from bugcar_image_segmentation_amd import _native as N

# (kind, precision, C, asym, variant, transposed, cin, windowed, lut_kind, threads, lds_bytes, TH, TW, NW, RD, keep)
# kind 0 = bottleneck, 1 = upsampling (C = its output channels, cin = its input channels); precision 0 fp32, 1 bf16,
# 2 fp16; lut_kind >= 0: the C = 16 form with the class layer fused
PARENT = [
    (0, 0, 16, 0, 0, 0, 0, 0, -1, 256, 27200, 16, 16, 4, 0, None),
    (0, 0, 16, 1, 0, 0, 0, 0, -1, 256, 33168, 16, 16, 4, 0, None),
    (0, 0, 64, 0, 0, 0, 0, 0, -1, 256, 47616, 16, 16, 4, 0, 0),
    (0, 0, 64, 0, 0, 0, 16, 0, -1, 256, 36736, 16, 16, 4, 0, None),
    (0, 0, 64, 0, 1, 0, 0, 0, -1, 256, 52224, 20, 16, 4, 0, 0),
    (0, 0, 64, 0, 2, 0, 0, 0, -1, 256, 38400, 8, 16, 4, 0, 0),
    (0, 0, 64, 1, 0, 0, 0, 0, -1, 256, 61456, 16, 16, 4, 0, None),
    (0, 0, 64, 1, 1, 0, 0, 0, -1, 256, 67856, 20, 16, 4, 0, None),
    (0, 0, 64, 1, 2, 0, 0, 0, -1, 256, 48656, 8, 16, 4, 0, None),
    (0, 0, 128, 0, 0, 0, 0, 0, -1, 512, 130048, 16, 16, 8, 0, None),
    (0, 0, 128, 0, 1, 0, 0, 0, -1, 512, 141568, 20, 16, 8, 0, None),
    (0, 0, 128, 0, 1, 0, 64, 0, -1, 512, 79232, 20, 16, 8, 0, None),
    (0, 0, 128, 0, 1, 1, 0, 0, -1, 512, 141568, 20, 16, 8, 0, None),
    (0, 0, 128, 0, 2, 0, 0, 0, -1, 512, 155008, 4, 80, 8, 1, None),
    (0, 0, 128, 0, 2, 0, 0, 1, -1, 512, 155008, 4, 80, 8, 1, None),
    (0, 0, 128, 0, 3, 0, 0, 0, -1, 512, 139648, 4, 64, 8, 1, None),
    (0, 0, 128, 0, 4, 0, 0, 0, -1, 512, 107008, 8, 16, 8, 0, None),
    (0, 0, 128, 1, 0, 0, 0, 0, -1, 512, 147360, 16, 16, 8, 0, None),
    (0, 0, 128, 1, 0, 0, 0, 1, -1, 512, 147360, 16, 16, 8, 0, None),
    (0, 0, 128, 1, 1, 0, 0, 0, -1, 512, 160160, 20, 16, 8, 0, None),
    (0, 0, 128, 1, 1, 0, 0, 1, -1, 512, 160160, 20, 16, 8, 0, None),
    (0, 0, 128, 1, 4, 0, 0, 0, -1, 512, 121760, 8, 16, 8, 0, None),
    (0, 0, 128, 1, 4, 0, 0, 1, -1, 512, 121760, 8, 16, 8, 0, None),
    (0, 1, 16, 0, 0, 0, 0, 0, -1, 256, 12448, 16, 16, 4, 0, None),
    (0, 1, 16, 0, 1, 0, 0, 0, -1, 256, 13600, 20, 16, 4, 0, None),
    (0, 1, 16, 1, 0, 0, 0, 0, -1, 256, 15200, 16, 16, 4, 0, None),
    (0, 1, 64, 0, 0, 0, 0, 0, -1, 256, 25888, 16, 16, 4, 0, 1),
    (0, 1, 64, 0, 0, 0, 16, 0, -1, 256, 22688, 16, 16, 4, 0, None),
    (0, 1, 64, 0, 1, 0, 0, 0, -1, 256, 28192, 20, 16, 4, 0, 0),
    (0, 1, 64, 0, 2, 0, 0, 0, -1, 256, 24736, 8, 16, 4, 0, 1),
    (0, 1, 64, 1, 0, 0, 0, 0, -1, 256, 29856, 16, 16, 4, 0, None),
    (0, 1, 64, 1, 1, 0, 0, 0, -1, 256, 32416, 20, 16, 4, 0, None),
    (0, 1, 64, 1, 2, 0, 0, 0, -1, 256, 26272, 8, 16, 4, 0, None),
    (0, 1, 128, 0, 0, 0, 0, 0, -1, 512, 74400, 16, 16, 8, 0, None),
    (0, 1, 128, 0, 1, 0, 0, 0, -1, 512, 81312, 20, 16, 8, 0, None),
    (0, 1, 128, 0, 1, 0, 64, 0, -1, 512, 41248, 20, 16, 8, 0, None),
    (0, 1, 128, 0, 1, 1, 0, 0, -1, 512, 81312, 20, 16, 8, 0, None),
    (0, 1, 128, 0, 2, 0, 0, 0, -1, 512, 78624, 4, 80, 8, 1, None),
    (0, 1, 128, 0, 3, 0, 0, 0, -1, 512, 80160, 4, 64, 8, 1, None),
    (0, 1, 128, 0, 4, 0, 0, 0, -1, 512, 60576, 8, 16, 8, 0, None),
    (0, 1, 128, 1, 0, 0, 0, 0, -1, 512, 74784, 16, 16, 8, 0, None),
    (0, 1, 128, 1, 1, 0, 0, 0, -1, 512, 81184, 20, 16, 8, 0, None),
    (0, 1, 128, 1, 4, 0, 0, 0, -1, 512, 61984, 8, 16, 8, 0, None),
    (0, 2, 16, 0, 0, 0, 0, 0, -1, 256, 12448, 16, 16, 4, 0, None),
    (0, 2, 16, 0, 1, 0, 0, 0, -1, 256, 13600, 20, 16, 4, 0, None),
    (0, 2, 16, 1, 0, 0, 0, 0, -1, 256, 15200, 16, 16, 4, 0, None),
    (0, 2, 64, 0, 0, 0, 0, 0, -1, 256, 25888, 16, 16, 4, 0, 1),
    (0, 2, 64, 0, 0, 0, 16, 0, -1, 256, 22688, 16, 16, 4, 0, None),
    (0, 2, 64, 0, 1, 0, 0, 0, -1, 256, 28192, 20, 16, 4, 0, 0),
    (0, 2, 64, 0, 2, 0, 0, 0, -1, 256, 24736, 8, 16, 4, 0, 1),
    (0, 2, 64, 1, 0, 0, 0, 0, -1, 256, 29856, 16, 16, 4, 0, None),
    (0, 2, 64, 1, 1, 0, 0, 0, -1, 256, 32416, 20, 16, 4, 0, None),
    (0, 2, 64, 1, 2, 0, 0, 0, -1, 256, 26272, 8, 16, 4, 0, None),
    (0, 2, 128, 0, 0, 0, 0, 0, -1, 512, 74400, 16, 16, 8, 0, None),
    (0, 2, 128, 0, 1, 0, 0, 0, -1, 512, 81312, 20, 16, 8, 0, None),
    (0, 2, 128, 0, 1, 0, 64, 0, -1, 512, 41248, 20, 16, 8, 0, None),
    (0, 2, 128, 0, 1, 1, 0, 0, -1, 512, 81312, 20, 16, 8, 0, None),
    (0, 2, 128, 0, 2, 0, 0, 0, -1, 512, 78624, 4, 80, 8, 1, None),
    (0, 2, 128, 0, 3, 0, 0, 0, -1, 512, 80160, 4, 64, 8, 1, None),
    (0, 2, 128, 0, 4, 0, 0, 0, -1, 512, 60576, 8, 16, 8, 0, None),
    (0, 2, 128, 1, 0, 0, 0, 0, -1, 512, 74784, 16, 16, 8, 0, None),
    (0, 2, 128, 1, 1, 0, 0, 0, -1, 512, 81184, 20, 16, 8, 0, None),
    (0, 2, 128, 1, 4, 0, 0, 0, -1, 512, 61984, 8, 16, 8, 0, None),
    (0, 0, 16, 0, 0, 0, 0, 0, 0, 256, 64336, 16, 16, 4, 0, None),
    (0, 0, 16, 0, 0, 0, 0, 0, 1, 256, 64336, 16, 16, 4, 0, None),
    (0, 0, 16, 0, 0, 0, 0, 0, 2, 256, 64336, 16, 16, 4, 0, None),
    (0, 1, 16, 0, 0, 0, 0, 0, 0, 256, 33200, 16, 16, 4, 0, None),
    (0, 1, 16, 0, 0, 0, 0, 0, 1, 256, 33200, 16, 16, 4, 0, None),
    (0, 1, 16, 0, 0, 0, 0, 0, 2, 256, 33200, 16, 16, 4, 0, None),
    (0, 2, 16, 0, 0, 0, 0, 0, 0, 256, 33200, 16, 16, 4, 0, None),
    (0, 2, 16, 0, 0, 0, 0, 0, 1, 256, 33200, 16, 16, 4, 0, None),
    (0, 2, 16, 0, 0, 0, 0, 0, 2, 256, 33200, 16, 16, 4, 0, None),
    (1, 0, 64, 0, 0, 0, 128, 0, -1, 256, 80896, 0, 0, 4, 0, None),
    (1, 1, 64, 0, 0, 0, 128, 0, -1, 512, 48640, 0, 0, 8, 0, None),
    (1, 2, 64, 0, 0, 0, 128, 0, -1, 512, 48640, 0, 0, 8, 0, None),
    (1, 0, 16, 0, 0, 0, 64, 0, -1, 256, 21184, 0, 0, 4, 0, None),
    (1, 1, 16, 0, 0, 0, 64, 0, -1, 256, 13760, 0, 0, 4, 0, None),
    (1, 2, 16, 0, 0, 0, 64, 0, -1, 256, 13760, 0, 0, 4, 0, None),
]
KEY = slice(0, 9)
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def forms(native_lib):
    return [tuple(r[c] for c in N.FORM_COLS) for r in N.fused_forms()]


def test_forms_are_the_recorded_table(forms):
    assert len({f[KEY] for f in forms}) == len(forms), "a form is listed twice"
    got = {f[KEY]: f[9:] for f in forms}
    want = {p[KEY]: p[9:] for p in PARENT}
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        g = got[key]
        assert g[:6] == w[:6], f"form {key}: (threads, lds, TH, TW, NW, RD) {g[:6]}, recorded {w[:6]}"
        if w[6] is not None:
            assert g[6] == w[6], f"form {key}: keep {g[6]}, recorded {w[6]}"


def test_bottleneck_kernel_count(forms):
    assert sum(f[0] == 0 for f in forms) == 72
    assert sum(f[0] == 1 for f in forms) == 6


def test_lds_fits_the_cu(forms):
    for f in forms:
        assert 0 < f[10] <= LDS_LIMIT, f


def test_threads_are_whole_waves(forms):
    for f in forms:
        assert f[9] == f[13] * 64, f


def test_short_buffer_is_not_overrun(native_lib):
    import ctypes
    n = native_lib.bugseg_debug_fused_forms(None, 0)
    assert n == len(PARENT)
    buf = (ctypes.c_int32 * (3 * len(N.FORM_COLS) + 1))()
    buf[len(buf) - 1] = 0x5A5A5A5A
    assert native_lib.bugseg_debug_fused_forms(buf, 3) == n
    assert buf[len(buf) - 1] == 0x5A5A5A5A
    assert native_lib.bugseg_debug_fused_forms(None, 3) == N.EINVAL
