"""The BUGSEG_* run-time knobs (csrc/knobs.h): one reader, uniform parsing. Host only: the dump
with no context parses the environment as it is now and touches no device."""
import ctypes

import pytest

from bugcar_image_segmentation_amd import _native as N

# DESIGN.md 6.15 (-1 / 0 where the table says "unset")
DEFAULTS = {
    "BUGSEG_F32_RANGE": 1, "BUGSEG_NO_PAIR": 0, "BUGSEG_NO_FUSE": 0, "BUGSEG_BNECK_VARIANT": -1,
    "BUGSEG_BNECK_VARIANT_C128": -1, "BUGSEG_BNECK_VARIANT_C64": -1, "BUGSEG_BNECK_VARIANT_C16": -1,
    "BUGSEG_BNECK_VARIANT_ASYM": -1, "BUGSEG_BNECK2": 0, "BUGSEG_TILE_ORDER": 1, "BUGSEG_CLS_FUSE": 0,
    "BUGSEG_CLS_CONV": 0, "BUGSEG_ROW_WINDOW_S3": 1, "BUGSEG_INIT_TABLE": 0, "BUGSEG_INIT_POOL_SCAN": 0,
    "BUGSEG_BNECK_GRID": 0, "BUGSEG_BEV_F": 0, "BUGSEG_BEV_FG": 0, "BUGSEG_BEV_BAND": 1, "BUGSEG_BEV_FB": 1,
    "BUGSEG_BEV_NEAR_FIRST": 0, "BUGSEG_DL_GEMM": 1, "BUGSEG_DL_G128": 1, "BUGSEG_DL_IG": 1, "BUGSEG_DL_IG64": 1,
    "BUGSEG_DL_GTM": -1, "BUGSEG_DL_GROUP": 1,
}

# every (variable, value) the tests and scripts set
USED = [
    ("BUGSEG_F32_RANGE", "0"), ("BUGSEG_NO_PAIR", "1"), ("BUGSEG_NO_FUSE", "1"), ("BUGSEG_NO_FUSE", "0"),
    *[("BUGSEG_BNECK_VARIANT", v) for v in "01234"], ("BUGSEG_BNECK_VARIANT_C128", "5"),
    ("BUGSEG_BNECK_VARIANT_ASYM", "0"), ("BUGSEG_BNECK2", "1"), *[("BUGSEG_TILE_ORDER", v) for v in "012"],
    ("BUGSEG_CLS_FUSE", "1"), ("BUGSEG_CLS_FUSE", "0"), ("BUGSEG_CLS_CONV", "1"), ("BUGSEG_ROW_WINDOW_S3", "0"),
    ("BUGSEG_INIT_TABLE", "1"), ("BUGSEG_INIT_POOL_SCAN", "1"), ("BUGSEG_BNECK_GRID", "8"), ("BUGSEG_BNECK_GRID", "-2"),
    ("BUGSEG_BEV_F", "1"), ("BUGSEG_BEV_F", "2"), ("BUGSEG_BEV_F", "4"), ("BUGSEG_BEV_FG", "4"), ("BUGSEG_BEV_BAND", "0"),
    ("BUGSEG_BEV_FB", "2"), ("BUGSEG_BEV_NEAR_FIRST", "1"), ("BUGSEG_DL_GEMM", "0"), ("BUGSEG_DL_G128", "0"),
    ("BUGSEG_DL_IG", "0"), ("BUGSEG_DL_IG64", "0"), ("BUGSEG_DL_IG64", "1"), ("BUGSEG_DL_GTM", "0"), ("BUGSEG_DL_GTM", "1"),
    ("BUGSEG_DL_GROUP", "0"),
]


@pytest.fixture
def clean_env(native_lib, monkeypatch):
    for name in DEFAULTS:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_clean_environment_gives_the_documented_defaults(clean_env):
    assert N.knobs() == DEFAULTS
    assert N.knobs(dl=True) == DEFAULTS
    assert list(N.knobs()) == list(DEFAULTS)          # one line per knob, in the table's order


@pytest.mark.parametrize("name,value", USED)
def test_every_value_in_use_parses_to_its_field(clean_env, name, value):
    clean_env.setenv(name, value)
    assert N.knobs() == {**DEFAULTS, name: int(value)}


@pytest.mark.parametrize("name", ["BUGSEG_CLS_CONV", "BUGSEG_NO_PAIR", "BUGSEG_INIT_TABLE", "BUGSEG_INIT_POOL_SCAN"])
def test_zero_turns_a_boolean_off_and_empty_is_the_default(clean_env, name):
    clean_env.setenv(name, "0")
    assert N.knobs()[name] == 0
    clean_env.setenv(name, "")
    assert N.knobs() == DEFAULTS


@pytest.mark.parametrize("name,value", [
    ("BUGSEG_TILE_ORDER", "3"), ("BUGSEG_BEV_FB", "x"), ("BUGSEG_NO_FUSE", "yes"),
    ("BUGSEG_BEV_F", "3"), ("BUGSEG_BEV_FG", "-1"), ("BUGSEG_BNECK_GRID", "8 "), ("BUGSEG_BNECK_GRID", "99999999999"),
    ("BUGSEG_BNECK_VARIANT_C16", "2"), ("BUGSEG_DL_GTM", "2"), ("BUGSEG_CLS_CONV", "2"), ("BUGSEG_TILE_ORDER", "1.0"),
])
def test_a_bad_value_is_an_error_that_names_the_variable(clean_env, native_lib, name, value):
    clean_env.setenv(name, value)
    buf = ctypes.create_string_buffer(4096)
    assert native_lib.bugseg_debug_knobs(None, buf, 4096) == N.EINVAL
    err = native_lib.bugseg_last_error(None).decode()
    assert name in err and value in err
    assert native_lib.bugseg_dl_debug_knobs(None, buf, 4096) == N.EINVAL
    assert name in native_lib.bugseg_dl_last_error(None).decode()
    with pytest.raises(ValueError, match=name):
        N.knobs()


def test_a_small_buffer_is_an_error_and_is_not_overrun(clean_env, native_lib):
    need = len("".join(f"{k}={v}\n" for k, v in DEFAULTS.items())) + 1
    for size in (0, 1, 16, need - 1):
        buf = ctypes.create_string_buffer(b"\xaa" * 64 + b"\xaa" * need, need + 64)
        assert native_lib.bugseg_debug_knobs(None, buf, size) == N.EINVAL
        assert buf.raw[size:] == b"\xaa" * (need + 64 - size), "bytes past the given length were written"
    buf = ctypes.create_string_buffer(need)
    assert native_lib.bugseg_debug_knobs(None, buf, need) == N.OK
    assert buf.value.decode().count("\n") == len(DEFAULTS)
    assert native_lib.bugseg_debug_knobs(None, None, 4096) == N.EINVAL


def test_the_removed_knobs_are_not_read(clean_env):
    for name in ("BUGSEG_DL_GPD2", "BUGSEG_DL_G2ALL", "BUGSEG_DL_PD", "BUGSEG_DL_DWR"):
        clean_env.setenv(name, "1")
    assert N.knobs() == DEFAULTS
