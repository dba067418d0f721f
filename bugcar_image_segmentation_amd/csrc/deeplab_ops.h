// The DeepLab op record (include/bugseg.h: BUGSEG_DL_OP_FIELDS int32, the kind first), one field table per
// kind. Host only. deeplab_spec.OP_LAYOUT is the writer's copy of these tables; bugseg_dl_debug_op_layout
// lets a test compare the two.
#pragma once
#include <cstring>

#include "../../include/bugseg.h"

namespace bugseg {

#define DL_PREP_FIELDS(X) X(dst)
// act: 0 none, 1 ReLU, 2 ReLU6 (before the residual add), 3 ReLU after the residual add. res, bias_img,
// dw_w_off: -1 when absent. dw_geom: stride | dil << 8 | pad_t << 16 | pad_l << 24 of the fused depthwise
// conv. nb: pixel fragments per wave (0: the launcher's 2). tap: 0 plain, 1 tap-packed, 2 tap-packed
// reading the raw u8 frames.
#define DL_CONV_FIELDS(X)                                                                                       \
    X(src) X(dst) X(res) X(Hin) X(Win) X(CS) X(Hout) X(Wout) X(kh) X(kw) X(stride) X(dil) X(pad_t) X(pad_l)     \
    X(cinP) X(NP) X(w_off) X(b_off) X(act) X(res_cs) X(out_cs) X(out_off) X(cout) X(out_f32) X(bias_img)        \
    X(bias_img_stride) X(dw_w_off) X(dw_b_off) X(dw_geom) X(nb) X(tap)
#define DL_DW_FIELDS(X)                                                                                         \
    X(src) X(dst) X(Hin) X(Win) X(C) X(Hout) X(Wout) X(stride) X(dil) X(pad_t) X(pad_l) X(w_off) X(b_off)       \
    X(act) X(in_relu)
#define DL_POOL_FIELDS(X)                                                                                       \
    X(src) X(part) X(z) X(H) X(W) X(C) X(CS) X(chunk_px) X(nchunks) X(cmid) X(cout) X(wp_off) X(bp_off)         \
    X(wq_off) X(bq_off) X(z_stride) X(y)
#define DL_ARGMAX_FIELDS(X) X(logits) X(h) X(w) X(LCS) X(ncls)
#define DL_RESIZE_FIELDS(X) X(src) X(dst) X(h) X(w) X(in_cs) X(C) X(Hout) X(Wout) X(out_cs) X(out_off)
#define DL_MAXPOOL_FIELDS(X) X(src) X(dst) X(Hin) X(Win) X(C) X(Hout) X(Wout) X(k) X(stride) X(pad_t) X(pad_l)

// K(kind constant, its value, struct, union member, field list)
#define DL_OP_KINDS(K)                                  \
    K(OP_PREP, 1, DlPrepOp, prep, DL_PREP_FIELDS)       \
    K(OP_CONV, 2, DlConvOp, conv, DL_CONV_FIELDS)       \
    K(OP_DW, 3, DlDwOp, dw, DL_DW_FIELDS)               \
    K(OP_POOL, 4, DlPoolOp, pool, DL_POOL_FIELDS)       \
    K(OP_ARGMAX, 5, DlArgmaxOp, argmax, DL_ARGMAX_FIELDS) \
    K(OP_RESIZE, 6, DlResizeOp, resize, DL_RESIZE_FIELDS) \
    K(OP_MAXPOOL, 7, DlMaxPoolOp, maxpool, DL_MAXPOOL_FIELDS)

#define DL_MEMBER(n) int n;
#define DL_NAME(n) #n ","
#define DL_STRUCT(KIND, V, T, M, FIELDS)                                                                        \
    struct T { int kind; FIELDS(DL_MEMBER) };                                                                   \
    static_assert(sizeof(T) <= 4 * BUGSEG_DL_OP_FIELDS, #T " does not fit a record");
#define DL_ENUM(KIND, V, T, M, FIELDS) KIND = V,
#define DL_UNION(KIND, V, T, M, FIELDS) T M;
#define DL_DECODE(KIND, V, T, M, FIELDS) case KIND: std::memcpy(&o.M, rec, sizeof(T)); break;
#define DL_NAMES(KIND, V, T, M, FIELDS) case KIND: return FIELDS(DL_NAME);

enum { DL_OP_KINDS(DL_ENUM) };
DL_OP_KINDS(DL_STRUCT)

// A decoded op: the member its kind names (every member begins with the kind; an unknown kind has only that).
union DlOp {
    struct { int kind; } any;
    DL_OP_KINDS(DL_UNION)
};

// The record's prefix copied into the struct of its kind.
inline DlOp dl_decode(const int32_t *rec) {
    DlOp o{};
    o.any.kind = *rec;
    switch (o.any.kind) { DL_OP_KINDS(DL_DECODE) }
    return o;
}

// "src,dst,...," : the names of a kind's fields after the kind, each followed by a comma; null for an unknown kind.
inline const char *dl_field_names(int kind) {
    switch (kind) { DL_OP_KINDS(DL_NAMES) }
    return nullptr;
}

#undef DL_MEMBER
#undef DL_NAME
#undef DL_STRUCT
#undef DL_ENUM
#undef DL_UNION
#undef DL_DECODE
#undef DL_NAMES

}  // namespace bugseg
