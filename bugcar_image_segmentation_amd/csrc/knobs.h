// The run-time behaviour knobs (BUGSEG_* environment variables; DESIGN.md 6.15 says what each does): one record,
// read from the environment once, when a context is created (bugseg_create, bugseg_dl_create), and held there
// unchanged. Nothing after creation reads the environment; the launchers take what they need from the context's
// record. (BUGSEG_STAMPS, BUGSEG_RANGE and the like are compile-time defines, not knobs.)
#pragma once
#include <string>

#ifndef BUGSEG_TILE_ORDER_DEFAULT   // (the measurement that chose it)
#define BUGSEG_TILE_ORDER_DEFAULT 1
#endif

namespace bugseg {

// A context's other creation-time choice, its storage precision (here for the host-only code, which reads it
// without the HIP headers of bugseg_internal.h)
enum Prec { PREC_F32 = 0, PREC_BF16 = 1, PREC_F16 = 2 };
// bytes per stored element: fp32 parity mode 4; bf16 / f16 storage modes 2
inline constexpr int prec_es(int prec) { return prec == PREC_F32 ? 4 : 2; }

// X(variable after "BUGSEG_", field, default, least, greatest): every knob is a decimal integer in [least,
// greatest], a boolean one in [0, 1]; unset or empty is the default (-1, and BEV_F's 0: not set, the code chooses).
#define BUGSEG_KNOBS(X) \
    X(F32_RANGE, f32_range, 1, 0, 1) X(NO_PAIR, no_pair, 0, 0, 1) X(NO_FUSE, no_fuse, 0, 0, 1) \
    X(BNECK_VARIANT, bneck_variant, -1, 0, 5) X(BNECK_VARIANT_C128, bneck_variant_c128, -1, 0, bneck_variants(128) - 1) \
    X(BNECK_VARIANT_C64, bneck_variant_c64, -1, 0, bneck_variants(64) - 1) \
    X(BNECK_VARIANT_C16, bneck_variant_c16, -1, 0, bneck_variants(16) - 1) X(BNECK_VARIANT_ASYM, bneck_variant_asym, -1, 0, 5) \
    X(BNECK2, bneck2, 0, 0, 1) X(TILE_ORDER, tile_order, BUGSEG_TILE_ORDER_DEFAULT, 0, 2) X(CLS_FUSE, cls_fuse, 0, 0, 1) \
    X(CLS_CONV, cls_conv, 0, 0, 1) X(ROW_WINDOW_S3, row_window_s3, 1, 0, 1) X(INIT_TABLE, init_table, 0, 0, 1) \
    X(INIT_POOL_SCAN, init_pool_scan, 0, 0, 1) X(BNECK_GRID, bneck_grid, 0, INT_MIN, INT_MAX) \
    X(BEV_F, bev_f, 0, 1, 4) /* (not 3) */ X(BEV_FG, bev_fg, 0, 0, INT_MAX) X(BEV_BAND, bev_band, 1, 0, 1) \
    X(BEV_FB, bev_fb, 1, 1, 2) X(BEV_NEAR_FIRST, bev_near_first, 0, 0, 1) \
    X(DL_GEMM, dl_gemm, 1, 0, 1) X(DL_G128, dl_g128, 1, 0, 1) X(DL_IG, dl_ig, 1, 0, 1) X(DL_IG64, dl_ig64, 1, 0, 1) \
    X(DL_GTM, dl_gtm, -1, 0, 1) X(DL_GROUP, dl_group, 1, 0, 1)

struct Knobs {
#define X(name, field, def, lo, hi) int field = def;
    BUGSEG_KNOBS(X)
#undef X
};

// Fills k from the environment; false: a variable holds anything else, and err names it and its value.
bool read_knobs(Knobs &k, std::string &err);
// One NAME=value line per knob of k (nullptr: of the environment as it is now; no device is touched) into
// buf[len], NUL-terminated. -> BUGSEG_OK, or BUGSEG_EINVAL with err set (a bad value; buf too small).
int dump_knobs(const Knobs *k, char *buf, int len, std::string &err);

}  // namespace bugseg
