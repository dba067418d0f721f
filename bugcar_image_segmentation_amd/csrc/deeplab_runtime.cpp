// DeepLabV3 executor behind the C ABI (include/bugseg.h, bugseg_dl_*): SURVEY.md §8(f) row 3.
//
// The graph builder is host-side Python (deeplab_spec.py): it folds batch-norm, packs weights for
// the kernels into one blob, and lowers the network to a flat op list with buffer ids for a batch
// size. This executor owns the device copies (weights, one activation arena per plan), validates
// every op's shapes against its buffers before anything is launched, and enqueues the launches on
// the caller's stream. It knows nothing about MobileNetV2, Xception or ASPP beyond the op kinds
// (deeplab_ops.h). A plan is one value, built and validated whole and installed whole; the device
// memory follows DESIGN.md 6.26 (6.27).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "bugseg_internal.h"
#include "ctx_memory.h"
#include "deeplab_internal.h"
#include "deeplab_ops.h"
#include "../../include/bugseg.h"

using namespace bugseg;

namespace {

thread_local std::string g_dl_err;

// One forward's input and output: the frames and their channel order, and either the int64 map (seg ==
// nullptr) or the u8 class map with the output rows [row0, row1) the final op stores.
struct DlIo {
    const uint8_t *img = nullptr;
    int bgr = 0, H = 0, W = 0;
    int64_t *out = nullptr;
    uint8_t *seg = nullptr;
    int row0 = 0, row1 = 0;
};

// A lowered network at one batch size and crop, with what belongs to it: its arena and its last forward.
struct DlPlan {
    std::vector<DlOp> ops;
    std::vector<int> group_len;   // per op: > 1 at the first of that many same-shape convs run as one launch
    std::vector<size_t> buf_bytes, buf_off;
    size_t total = 0;             // arena bytes
    int B = 0, Hc = 0, Wc = 0;
    void *arena = nullptr;
    bool pinned = false;          // a launch on this arena was captured into a graph: never freed before destroy
    // the last forward's I/O (profiling hook; classes_from_logits checks its frame size)
    DlIo last;
    bool has_logits = false;      // a forward of this plan has run: its logits are in the arena
};

}  // namespace

struct bugseg_dl {
    bugseg_dl(const Knobs &k, int device) : knobs(k), mem(device) {}
    const Knobs knobs;            // the BUGSEG_* knobs as bugseg_dl_create read them (knobs.h)
    CtxMemory mem;
    int prec = 0;
    std::string err;
    void *dev_w = nullptr;
    size_t w_bytes = 0, zero_off = 0;
    bool w_pinned = false;        // as DlPlan::pinned, for dev_w
    DlPlan plan;                  // no ops: no plan
    // class LUT of the u8 final op: 256 bytes of device memory, identity until bugseg_dl_set_class_lut
    uint8_t *dev_lut = nullptr;
    int lut_n = 0;                // 0: identity (fits any class count), else the class count it was set for
};

namespace {

int dl_fail(bugseg_dl *c, int code, const std::string &m) {
    if (c) c->err = m;
    else g_dl_err = m;
    return code;
}

void *bufp(const DlPlan &p, int id) { return static_cast<char *>(p.arena) + p.buf_off[id]; }

bool in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }

// Shape / bounds validation of one op against the plan's buffers and a weight blob of w_bytes.
bool check_op(const DlPlan &p, int prec, size_t w_bytes, const DlOp &op, std::string &why) {
    const double es = prec == PREC_BF16 ? 2.0 : 4.0;
    const int B = p.B;
    auto in_w = [&](long off, long bytes) { return off >= 0 && bytes >= 0 && off + bytes <= (long)w_bytes; };
    auto buf_ok = [&](int id, double bytes) { return id >= 0 && id < (int)p.buf_bytes.size() && bytes <= (double)p.buf_bytes[id]; };
    // every field that enters integer arithmetic here or in run_op is bounded first (no overflow):
    // spatial sizes <= 16384, channels <= 8192, kernel extents <= 15, strides / dilations <= 255
    constexpr int SP = 16384, CH = 8192;
    switch (op.any.kind) {
    case OP_PREP:
        if (!buf_ok(op.prep.dst, (double)B * p.Hc * p.Wc * 8 * es)) { why = "prep: destination buffer too small"; return false; }
        return true;
    case OP_CONV: {
        const DlConvOp &o = op.conv;
        if (!in_range(o.Hin, 1, SP) || !in_range(o.Win, 1, SP) || !in_range(o.Hout, 1, SP) || !in_range(o.Wout, 1, SP) ||
            !in_range(o.kh, 1, 15) || !in_range(o.kw, 1, 15) || !in_range(o.stride, 1, 255) || !in_range(o.dil, 1, 255) ||
            !in_range(o.pad_t, 0, 255) || !in_range(o.pad_l, 0, 255) || !in_range(o.CS, 8, CH) || !in_range(o.cinP, 32, CH) ||
            !in_range(o.NP, 64, CH) || !in_range(o.res_cs, 0, CH) || !in_range(o.out_cs, 8, CH) || !in_range(o.out_off, 0, CH) ||
            !in_range(o.cout, 8, CH) || !in_range(o.bias_img_stride, 0, 1 << 20) || !in_range(o.tap, 0, 2) ||
            (double)B * o.Hout * o.Wout >= 2147483648.0) { why = "conv: field out of range"; return false; }
        if (o.CS % 8 || o.cinP % 32 || o.NP % 64 || o.act < 0 || o.act > 3 || o.cout % 8 || o.cout > o.NP || o.out_off % 8 ||
            o.out_off + o.cout > o.out_cs) { why = "conv: bad shape"; return false; }
        if (!buf_ok(o.src, (double)B * o.Hin * o.Win * o.CS * es)) { why = "conv: source buffer too small"; return false; }
        if (!buf_ok(o.dst, (double)B * o.Hout * o.Wout * o.out_cs * (o.out_f32 ? 4.0 : es))) { why = "conv: destination too small"; return false; }
        if (o.res >= 0 && (o.res_cs < o.cout || !buf_ok(o.res, (double)B * o.Hout * o.Wout * o.res_cs * es))) { why = "conv: residual too small"; return false; }
        if (o.bias_img >= 0 && (o.bias_img_stride < o.NP || !buf_ok(o.bias_img, (double)B * o.bias_img_stride * 4.0))) { why = "conv: per-image bias too small"; return false; }
        const long wk = o.tap ? (long)((o.kh * o.kw + 3) / 4) * 32 : (long)o.kh * o.kw * o.cinP;
        if (o.tap && (o.CS != 8 || o.dw_w_off >= 0)) { why = "conv: tap packing needs an 8-channel input"; return false; }
        if (!in_w(o.w_off, (long)o.NP * wk * (long)es) || !in_w(o.b_off, (long)o.NP * 4) || o.w_off % 16 || o.b_off % 16) {
            why = "conv: weights out of the blob"; return false;
        }
        if ((double)B * o.Hin * o.Win * o.CS * es >= 2147483648.0) { why = "conv: input exceeds 31-bit offsets"; return false; }
        if (o.nb != 0 && o.nb != 2 && o.nb != 4 && o.nb != 8) { why = "conv: pixel fragments per wave must be 2, 4 or 8"; return false; }
        if (o.dw_w_off >= 0) {   // depthwise-fused projection: 1x1 over the dw output grid (Hout, Wout)
            const int dws = o.dw_geom & 0xff, dwd = (o.dw_geom >> 8) & 0xff, pt = (o.dw_geom >> 16) & 0xff, pl = (o.dw_geom >> 24) & 0xff;
            if (o.kh != 1 || o.kw != 1 || o.stride != 1 || o.pad_t || o.pad_l || dws < 1 || dwd < 1 ||
                (o.Hout - 1) * dws - pt > o.Hin - 1 + 2 * dwd || (o.Wout - 1) * dws - pl > o.Win - 1 + 2 * dwd) {
                why = "conv: bad depthwise-fused geometry"; return false;
            }
            if (!in_w(o.dw_w_off, 9L * o.CS * (long)es) || !in_w(o.dw_b_off, (long)o.CS * 4) || o.dw_w_off % 16 || o.dw_b_off % 16) {
                why = "conv: depthwise weights out of the blob"; return false;
            }
        }
        return true;
    }
    case OP_DW: {
        const DlDwOp &o = op.dw;
        if (!in_range(o.Hin, 1, SP) || !in_range(o.Win, 1, SP) || !in_range(o.Hout, 1, SP) || !in_range(o.Wout, 1, SP) ||
            !in_range(o.C, 8, CH) || !in_range(o.stride, 1, 255) || !in_range(o.dil, 1, 255) || !in_range(o.pad_t, 0, 255) ||
            !in_range(o.pad_l, 0, 255) || (double)B * o.Hout * o.Wout >= 2147483648.0) { why = "dw: field out of range"; return false; }
        if (o.C % 8) { why = "dw: bad shape"; return false; }
        if (!in_range(o.act, 0, 2) || !in_range(o.in_relu, 0, 1) || (o.in_relu && o.act)) { why = "dw: bad activation flags"; return false; }
        if (o.stride != 1 && (o.stride != 2 || o.dil != 1)) { why = "dw: stride 2 with dilation (TF has no strided atrous)"; return false; }
        if (!buf_ok(o.src, (double)B * o.Hin * o.Win * o.C * es) || !buf_ok(o.dst, (double)B * o.Hout * o.Wout * o.C * es)) { why = "dw: buffer too small"; return false; }
        if ((double)B * o.Hin * o.Win * o.C * es >= 2147483648.0) { why = "dw: input exceeds 31-bit offsets"; return false; }
        if (!in_w(o.w_off, 9L * o.C * (long)es) || !in_w(o.b_off, (long)o.C * 4) || o.w_off % 16 || o.b_off % 16) { why = "dw: weights out of the blob"; return false; }
        return true;
    }
    case OP_POOL: {
        const DlPoolOp &o = op.pool;
        if (!in_range(o.H, 1, SP) || !in_range(o.W, 1, SP) || !in_range(o.CS, 1, CH)) { why = "pool: field out of range"; return false; }
        if (o.C < 1 || o.C > 2048 || o.C % 8 || o.CS < o.C || o.cmid < 1 || o.cmid > 1024 || o.cout < 1 || o.z_stride < o.cout ||
            o.chunk_px < 1 || o.nchunks < 1 || (long)o.chunk_px * o.nchunks < (long)o.H * o.W) { why = "pool: bad shape"; return false; }
        if (!buf_ok(o.src, (double)B * o.H * o.W * o.CS * es) || !buf_ok(o.part, (double)B * o.nchunks * o.C * 4.0) ||
            !buf_ok(o.z, (double)B * o.z_stride * 4.0) || !buf_ok(o.y, (double)B * o.cmid * 4.0)) { why = "pool: buffer too small"; return false; }
        if (!in_w(o.wp_off, (long)o.cmid * o.C * 4) || !in_w(o.bp_off, (long)o.cmid * 4) || !in_w(o.wq_off, (long)o.cout * o.cmid * 4) ||
            !in_w(o.bq_off, (long)o.cout * 4)) { why = "pool: weights out of the blob"; return false; }
        return true;
    }
    case OP_ARGMAX: {
        const DlArgmaxOp &o = op.argmax;
        if (!in_range(o.h, 1, SP) || !in_range(o.w, 1, SP) || !in_range(o.LCS, 1, CH)) { why = "argmax: field out of range"; return false; }
        if (o.ncls < 1 || o.LCS < o.ncls || o.LCS % 4) { why = "argmax: bad shape"; return false; }
        if (!buf_ok(o.logits, (double)B * o.h * o.w * o.LCS * 4.0)) { why = "argmax: logits buffer too small"; return false; }
        return true;
    }
    case OP_RESIZE: {
        const DlResizeOp &o = op.resize;
        if (!in_range(o.h, 1, SP) || !in_range(o.w, 1, SP) || !in_range(o.Hout, 1, SP) || !in_range(o.Wout, 1, SP) ||
            !in_range(o.in_cs, 8, CH) || !in_range(o.C, 8, CH) || !in_range(o.out_cs, 8, CH) || !in_range(o.out_off, 0, CH) ||
            (double)B * o.Hout * o.Wout * o.out_cs >= 2147483648.0) { why = "resize: field out of range"; return false; }
        if (o.C % 8 || o.in_cs % 8 || o.out_cs % 8 || o.out_off % 8 || o.C > o.in_cs || o.out_off + o.C > o.out_cs) { why = "resize: bad shape"; return false; }
        if (!buf_ok(o.src, (double)B * o.h * o.w * o.in_cs * es) || !buf_ok(o.dst, (double)B * o.Hout * o.Wout * o.out_cs * es)) {
            why = "resize: buffer too small"; return false;
        }
        return true;
    }
    case OP_MAXPOOL: {
        const DlMaxPoolOp &o = op.maxpool;
        if (!in_range(o.Hin, 1, SP) || !in_range(o.Win, 1, SP) || !in_range(o.Hout, 1, SP) || !in_range(o.Wout, 1, SP) ||
            !in_range(o.C, 8, CH) || !in_range(o.k, 1, 15) || !in_range(o.stride, 1, 255) || !in_range(o.pad_t, 0, 15) ||
            !in_range(o.pad_l, 0, 15) || (double)B * o.Hout * o.Wout * o.C >= 2147483648.0) { why = "maxpool: field out of range"; return false; }
        if (o.C % 8 || (o.Hout - 1) * o.stride - o.pad_t > o.Hin - 1 || (o.Wout - 1) * o.stride - o.pad_l > o.Win - 1) { why = "maxpool: bad shape"; return false; }
        // a first window wholly in the padding would store -inf; a strided pool in place races
        if (o.pad_t >= o.k || o.pad_l >= o.k) { why = "maxpool: padding covers the window"; return false; }
        if (o.src == o.dst) { why = "maxpool: in place"; return false; }
        if (!buf_ok(o.src, (double)B * o.Hin * o.Win * o.C * es) || !buf_ok(o.dst, (double)B * o.Hout * o.Wout * o.C * es)) {
            why = "maxpool: buffer too small"; return false;
        }
        return true;
    }
    default:
        why = "unknown op kind " + std::to_string(op.any.kind);
        return false;
    }
}

// Runs of consecutive k x k CONV ops of one shape that read the same buffer and write the same one
// (the ASPP's atrous branches, each at its channel offset of the concat): same input / output
// geometry, packing, no residual, depthwise or per-image bias, 2-byte output, not in place, and output
// channels [out_off, out_off + cout) that no two members share (one grid would race where a sequence has
// a last writer). -> per op, the length of the run starting there (1 = launched alone); a run ends before
// the first op that does not fit, which may start the next; the launcher still checks each member's form.
std::vector<int> conv_groups(const std::vector<DlOp> &ops) {
    std::vector<int> len(ops.size(), 1);
    auto alone_ok = [](const DlOp &op) {
        const DlConvOp &o = op.conv;
        return o.kind == OP_CONV && o.res < 0 && o.kh > 1 && o.kw > 1 && o.out_f32 == 0 && o.bias_img < 0 && o.dw_w_off < 0 &&
               o.tap == 0 && o.src != o.dst;
    };
    auto same = [](const DlConvOp &x, const DlConvOp &y) {
        return x.src == y.src && x.dst == y.dst && x.Hin == y.Hin && x.Win == y.Win && x.CS == y.CS && x.Hout == y.Hout &&
               x.Wout == y.Wout && x.kh == y.kh && x.kw == y.kw && x.cinP == y.cinP && x.NP == y.NP && x.out_cs == y.out_cs;
    };
    auto disjoint = [](const DlConvOp &x, const DlConvOp &y) {
        return (long)x.out_off + x.cout <= y.out_off || (long)y.out_off + y.cout <= x.out_off;
    };
    for (size_t i = 0; i < ops.size();) {
        size_t n = 1;
        auto fits = [&](const DlOp &next) {
            if (!alone_ok(next) || !same(ops[i].conv, next.conv)) return false;
            for (size_t k = 0; k < n; ++k)
                if (!disjoint(ops[i + k].conv, next.conv)) return false;
            return true;
        };
        if (alone_ok(ops[i]))
            while (i + n < ops.size() && (int)n < DL_GROUP_MAX && fits(ops[i + n])) ++n;
        if (n > 1) len[i] = (int)n;
        i += n;
    }
    return len;
}

// A plan from the ABI's arguments, for a context of precision prec holding a blob of w_bytes: every op
// validated against the buffers and the blob, the arena laid out (not allocated), the runs grouped.
// Host only. -> BUGSEG_OK, or the code with the message in `why` and `p` not to be used.
int build_plan(const int32_t *ops, int nops, const uint64_t *buf_bytes, int nbufs, int B, int Hc, int Wc, int prec,
               size_t w_bytes, DlPlan &p, std::string &why) {
    if (!ops || nops < 1 || nops > 4096 || nbufs < 1 || nbufs > 64 || !buf_bytes || B < 1 || Hc < 2 || Wc < 2 ||
        Hc > 8192 || Wc > 8192) { why = "bad plan"; return BUGSEG_EINVAL; }
    p.B = B; p.Hc = Hc; p.Wc = Wc;
    p.buf_bytes.assign(buf_bytes, buf_bytes + nbufs);
    p.buf_off.resize(nbufs);
    for (int i = 0; i < nbufs; ++i) {
        if (p.buf_bytes[i] > ((uint64_t)1 << 40)) { why = "buffer " + std::to_string(i) + " too large"; return BUGSEG_EINVAL; }
        p.buf_off[i] = p.total;
        p.total += (p.buf_bytes[i] + 255) & ~(size_t)255;
    }
    p.ops.reserve(nops);
    for (int i = 0; i < nops; ++i) {
        p.ops.push_back(dl_decode(ops + (size_t)i * BUGSEG_DL_OP_FIELDS));
        std::string w;
        if (!check_op(p, prec, w_bytes, p.ops.back(), w)) { why = "op " + std::to_string(i) + ": " + w; return BUGSEG_EINVAL; }
    }
    p.group_len = conv_groups(p.ops);
    return BUGSEG_OK;
}

// The DlConvArgs of a CONV op (run_op and the grouped launch in run_plan).
DlConvArgs conv_args(bugseg_dl *c, const DlConvOp &o, const DlIo &io) {
    const DlPlan &p = c->plan;
    const char *wb = static_cast<const char *>(c->dev_w);
    const int B = p.B;
    DlConvArgs a{};
    a.in = bufp(p, o.src);
    a.B = B; a.Hin = o.Hin; a.Win = o.Win; a.CS = o.CS;
    a.Hout = o.Hout; a.Wout = o.Wout; a.M = B * a.Hout * a.Wout;
    a.kh = o.kh; a.kw = o.kw; a.taps = a.kh * a.kw; a.stride = o.stride; a.dil = o.dil; a.pad_t = o.pad_t; a.pad_l = o.pad_l;
    a.cinP = o.cinP; a.NP = o.NP;
    a.w = wb + o.w_off;
    a.bias = reinterpret_cast<const float *>(wb + o.b_off);
    a.act = o.act;
    a.res = o.res >= 0 ? bufp(p, o.res) : nullptr;
    a.res_cs = o.res_cs;
    a.out = bufp(p, o.dst); a.out_cs = o.out_cs; a.out_off = o.out_off; a.cout = o.cout;
    a.bias_img = o.bias_img >= 0 ? static_cast<const float *>(bufp(p, o.bias_img)) : nullptr;
    a.bias_img_stride = o.bias_img_stride;
    a.in_bytes = (uint32_t)((size_t)B * a.Hin * a.Win * a.CS * (c->prec == PREC_BF16 ? 2 : 4));
    a.nb = o.nb == 8 ? 8 : o.nb == 4 ? 4 : 2;
    a.zero = wb + c->zero_off;
    a.tap_packed = o.tap != 0;
    if (o.tap == 2) { a.rgb = io.img; a.img_h = io.H; a.img_w = io.W; a.bgr = io.bgr; }   // stem with the preprocessing fused
    if (o.dw_w_off >= 0) {
        a.dw_w = wb + o.dw_w_off;
        a.dw_b = reinterpret_cast<const float *>(wb + o.dw_b_off);
        a.dw_stride = o.dw_geom & 0xff; a.dw_dil = (o.dw_geom >> 8) & 0xff;
        a.dw_pt = (o.dw_geom >> 16) & 0xff; a.dw_pl = (o.dw_geom >> 24) & 0xff;
    }
    fastdiv((uint32_t)(a.Hout * a.Wout), a.mHW, a.sHW);
    fastdiv((uint32_t)a.Wout, a.mW, a.sW);
    return a;
}

hipError_t run_op(bugseg_dl *c, const DlOp &op, const DlIo &io, hipStream_t s) {
    const DlPlan &p = c->plan;
    const char *wb = static_cast<const char *>(c->dev_w);
    const int B = p.B;
    switch (op.any.kind) {
    case OP_PREP: {
        DlPrepArgs a{io.img, B, io.H, io.W, p.Hc, p.Wc, bufp(p, op.prep.dst), io.bgr};
        return dl_launch_prep(c->prec, a, s);
    }
    case OP_CONV:
        return dl_launch_conv(c->knobs, c->prec, op.conv.out_f32 != 0, conv_args(c, op.conv, io), s);
    case OP_DW: {
        const DlDwOp &o = op.dw;
        DlDwArgs a{};
        a.in = bufp(p, o.src); a.out = bufp(p, o.dst);
        a.B = B; a.Hin = o.Hin; a.Win = o.Win; a.C = o.C; a.Hout = o.Hout; a.Wout = o.Wout;
        a.M = B * a.Hout * a.Wout; a.stride = o.stride; a.dil = o.dil; a.pad_t = o.pad_t; a.pad_l = o.pad_l;
        a.w = wb + o.w_off;
        a.in_bytes = (uint32_t)((size_t)B * a.Hin * a.Win * a.C * (c->prec == PREC_BF16 ? 2 : 4));
        a.bias = reinterpret_cast<const float *>(wb + o.b_off);
        a.act = o.act; a.in_relu = o.in_relu;
        fastdiv((uint32_t)(a.Hout * a.Wout), a.mHW, a.sHW);
        fastdiv((uint32_t)a.Wout, a.mW, a.sW);
        return dl_launch_dw(c->prec, a, s);
    }
    case OP_RESIZE: {
        const DlResizeOp &o = op.resize;
        DlResizeArgs a{};
        a.in = bufp(p, o.src); a.out = bufp(p, o.dst);
        a.B = B; a.h = o.h; a.w = o.w; a.in_cs = o.in_cs; a.C = o.C; a.Ho = o.Hout; a.Wo = o.Wout;
        a.out_cs = o.out_cs; a.out_off = o.out_off;
        a.sy = a.Ho > 1 ? (float)(a.h - 1) / (float)(a.Ho - 1) : 0.f;
        a.sx = a.Wo > 1 ? (float)(a.w - 1) / (float)(a.Wo - 1) : 0.f;
        return dl_launch_resize(c->prec, a, s);
    }
    case OP_POOL: {
        const DlPoolOp &o = op.pool;
        DlPoolArgs a{};
        a.x = bufp(p, o.src); a.part = static_cast<float *>(bufp(p, o.part)); a.z = static_cast<float *>(bufp(p, o.z));
        a.B = B; a.H = o.H; a.W = o.W; a.C = o.C; a.CS = o.CS; a.chunk_px = o.chunk_px; a.nchunks = o.nchunks;
        a.cmid = o.cmid; a.cout = o.cout;
        a.wp = reinterpret_cast<const float *>(wb + o.wp_off); a.bp = reinterpret_cast<const float *>(wb + o.bp_off);
        a.wq = reinterpret_cast<const float *>(wb + o.wq_off); a.bq = reinterpret_cast<const float *>(wb + o.bq_off);
        a.z_stride = o.z_stride;
        a.y = static_cast<float *>(bufp(p, o.y));
        return dl_launch_pool(c->prec, a, s);
    }
    case OP_MAXPOOL: {
        const DlMaxPoolOp &o = op.maxpool;
        DlMaxPoolArgs a{};
        a.in = bufp(p, o.src); a.out = bufp(p, o.dst);
        a.B = B; a.Hin = o.Hin; a.Win = o.Win; a.C = o.C; a.Hout = o.Hout; a.Wout = o.Wout;
        a.k = o.k; a.stride = o.stride; a.pad_t = o.pad_t; a.pad_l = o.pad_l;
        return dl_launch_maxpool(c->prec, a, s);
    }
    case OP_ARGMAX: {
        const DlArgmaxOp &o = op.argmax;
        DlArgmaxArgs a{};
        a.logits = static_cast<const float *>(bufp(p, o.logits));
        a.B = B; a.h = o.h; a.w = o.w; a.LCS = o.LCS; a.ncls = o.ncls;
        a.sy = p.Hc > 1 ? (float)(a.h - 1) / (float)(p.Hc - 1) : 0.f;
        a.sx = p.Wc > 1 ? (float)(a.w - 1) / (float)(p.Wc - 1) : 0.f;
        a.Ho = io.H; a.Wo = io.W; a.Hout = io.H; a.Wout = io.W;
        if (io.seg) {
            a.out8 = io.seg; a.lut = c->dev_lut; a.row0 = io.row0; a.row1 = io.row1;
            return dl_launch_argmax_u8(a, s);
        }
        a.out = io.out;
        return dl_launch_argmax(a, s);
    }
    }
    return hipErrorInvalidValue;
}

// The plan's ARGMAX op (its last one), or nullptr.
const DlOp *argmax_op(const DlPlan &p) {
    for (size_t i = p.ops.size(); i-- > 0;)
        if (p.ops[i].any.kind == OP_ARGMAX) return &p.ops[i];
    return nullptr;
}

int check_frame(bugseg_dl *c, int B, int H, int W) {
    const DlPlan &p = c->plan;
    if (B != p.B || H < 1 || W < 1 || H > p.Hc || W > p.Wc)
        return dl_fail(c, BUGSEG_EINVAL, "input (" + std::to_string(B) + ", " + std::to_string(H) + ", " + std::to_string(W) +
                                             ") does not fit the plan (B = " + std::to_string(p.B) + ", crop " +
                                             std::to_string(p.Hc) + "x" + std::to_string(p.Wc) + ")");
    return BUGSEG_OK;
}

// What the u8 final op needs beyond check_frame: a window inside the frame, a class count a byte holds
// and a LUT set for this plan's class count (one set for another plan is stale).
int check_classes(bugseg_dl *c, int H, int row0, int row1) {
    if (row0 < 0 || row1 > H || row0 >= row1)
        return dl_fail(c, BUGSEG_EINVAL, "row window [" + std::to_string(row0) + ", " + std::to_string(row1) +
                                             ") is empty or leaves [0, " + std::to_string(H) + ")");
    const DlOp *am = argmax_op(c->plan);
    if (!am) return dl_fail(c, BUGSEG_ESTATE, "the plan has no class-map op");
    const int ncls = am->argmax.ncls;
    if (ncls < 1 || ncls > 256) return dl_fail(c, BUGSEG_EINVAL, "a u8 class map holds at most 256 classes, the plan has " + std::to_string(ncls));
    if (c->lut_n != 0 && c->lut_n != ncls)
        return dl_fail(c, BUGSEG_EINVAL, "the class LUT was set for " + std::to_string(c->lut_n) + " classes, the plan has " +
                                             std::to_string(ncls));
    return BUGSEG_OK;
}

// A launch on `stream` is about to read the arena and the weights: a captured one keeps them until destroy.
hipStream_t launch_stream(bugseg_dl *c, void *stream) {
    if (stream_capturing(stream)) c->plan.pinned = c->w_pinned = true;
    return static_cast<hipStream_t>(stream);
}

// Every op of the plan on stream s (callers have validated io against the plan).
int run_plan(bugseg_dl *c, const DlIo &io, hipStream_t s) {
    DlPlan &p = c->plan;
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const int n = c->knobs.dl_group ? p.group_len[i] : 1;
        if (n > 1) {   // same-shape convs as one launch (the ASPP's atrous branches)
            DlConvGroup grp{};
            grp.n = n;
            for (int k = 0; k < n; ++k) grp.a[k] = conv_args(c, p.ops[i + k].conv, io);
            const hipError_t e = dl_launch_conv_group(c->knobs, c->prec, grp, s);
            if (e == hipSuccess) { i += n - 1; continue; }
            if (e != hipErrorNotSupported) return dl_fail(c, BUGSEG_EHIP, "grouped launch at op " + std::to_string(i) + ": " + hipGetErrorString(e));
            (void)hipGetLastError();
        }
        const hipError_t e = run_op(c, p.ops[i], io, s);
        if (e != hipSuccess) return dl_fail(c, BUGSEG_EHIP, "launch of op " + std::to_string(i) + ": " + hipGetErrorString(e));
    }
    p.last = io;
    p.has_logits = true;
    return BUGSEG_OK;
}

}  // namespace

extern "C" {

int bugseg_dl_create(int device, int precision, bugseg_dl **out) {
    if (!out || (precision != BUGSEG_FP32 && precision != BUGSEG_BF16)) return dl_fail(nullptr, BUGSEG_EINVAL, "bad argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return dl_fail(nullptr, BUGSEG_EINVAL, "no such HIP device");
    Knobs knobs;
    std::string bad;
    if (!read_knobs(knobs, bad)) return dl_fail(nullptr, BUGSEG_EINVAL, bad);
    auto *c = new bugseg_dl(knobs, device);
    c->prec = precision == BUGSEG_BF16 ? PREC_BF16 : PREC_F32;
    // the class LUT lives as long as the context: identity until one is set
    uint8_t id[256];
    for (int k = 0; k < 256; ++k) id[k] = (uint8_t)k;
    void *p = nullptr;
    if (const hipError_t e = c->mem.upload({{id, 256}}, &p)) {
        (void)hipGetLastError();
        delete c;
        return e == hipErrorOutOfMemory ? dl_fail(nullptr, BUGSEG_ENOMEM, "class LUT allocation failed")
                                        : dl_fail(nullptr, BUGSEG_EHIP, "class LUT upload failed");
    }
    c->dev_lut = static_cast<uint8_t *>(p);
    *out = c;
    return BUGSEG_OK;
}

int bugseg_dl_destroy(bugseg_dl *c) {
    if (!c) return BUGSEG_OK;
    DeviceGuard g(c->mem.device);
    (void)hipDeviceSynchronize();                     // enqueued launches may still read the context's memory
    if (c->dev_w) (void)hipFree(c->dev_w);
    if (c->plan.arena) (void)hipFree(c->plan.arena);
    if (c->dev_lut) (void)hipFree(c->dev_lut);
    delete c;                                         // the graveyard and the setup stream
    return BUGSEG_OK;
}

int bugseg_dl_load_weights(bugseg_dl *c, const void *blob, size_t bytes) {
    if (!c || !blob || bytes == 0 || bytes >= (size_t)1 << 31) return dl_fail(c, BUGSEG_EINVAL, "bad weight blob");
    DeviceGuard g(c->mem.device);
    // the old weights and the plan lowered against them go first: a failure below leaves neither
    c->mem.retire(c->dev_w, c->w_pinned);
    c->mem.retire(c->plan.arena, c->plan.pinned);
    c->dev_w = nullptr;
    c->w_bytes = c->zero_off = 0;
    c->w_pinned = false;
    c->plan = DlPlan();
    // the blob, then 256 zero bytes at a 256-B boundary (the implicit-GEMM conv's padding taps read them)
    const size_t zoff = (bytes + 255) / 256 * 256;
    const std::vector<char> zeros(zoff - bytes + 256, 0);
    void *w = nullptr;
    if (const hipError_t e = c->mem.upload({{blob, bytes}, {zeros.data(), zeros.size()}}, &w)) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? dl_fail(c, BUGSEG_ENOMEM, "weight allocation failed")
                                        : dl_fail(c, BUGSEG_EHIP, "weight upload failed");
    }
    c->dev_w = w;
    c->w_bytes = bytes;
    c->zero_off = zoff;
    return BUGSEG_OK;
}

// Test hook (host only, no device): the validation bugseg_dl_set_plan runs, for a blob of w_bytes.
int bugseg_dl_debug_check_plan(const int32_t *ops, int nops, const uint64_t *buf_bytes, int nbufs, int B, int Hc, int Wc,
                               int precision, size_t w_bytes) {
    DlPlan p;
    std::string why;
    const int rc = build_plan(ops, nops, buf_bytes, nbufs, B, Hc, Wc, precision == BUGSEG_BF16 ? PREC_BF16 : PREC_F32, w_bytes, p, why);
    return rc == BUGSEG_OK ? rc : dl_fail(nullptr, rc, why);
}

// Test hook (host only): conv_groups on unvalidated records.
int bugseg_dl_debug_plan_groups(const int32_t *ops, int nops, int32_t *len) {
    if (!ops || !len || nops < 0) return dl_fail(nullptr, BUGSEG_EINVAL, "bad argument");
    std::vector<DlOp> v;
    for (int i = 0; i < nops; ++i) v.push_back(dl_decode(ops + (size_t)i * BUGSEG_DL_OP_FIELDS));
    const std::vector<int> g = conv_groups(v);
    std::copy(g.begin(), g.end(), len);
    return BUGSEG_OK;
}

// Test hook (host only): "src,dst,..." of a kind's fields after the kind -> their count.
int bugseg_dl_debug_op_layout(int kind, char *buf, int len) {
    const char *names = dl_field_names(kind);
    if (!names) return dl_fail(nullptr, BUGSEG_EINVAL, "unknown op kind " + std::to_string(kind));
    const size_t n = std::strlen(names);   // each name is followed by a comma; the last one becomes the NUL
    if (!buf || len < (int)n) return dl_fail(nullptr, BUGSEG_EINVAL, "bad argument");
    std::memcpy(buf, names, n);
    buf[n - 1] = 0;
    return (int)std::count(names, names + n, ',');
}

int bugseg_dl_set_plan(bugseg_dl *c, const int32_t *ops, int nops, const uint64_t *buf_bytes, int nbufs, int B, int Hc, int Wc) {
    if (!c) return dl_fail(c, BUGSEG_EINVAL, "bad plan");
    if (!c->dev_w) return dl_fail(c, BUGSEG_ESTATE, "plan before weights");
    // build and validate the new plan before touching the old one
    DlPlan p;
    std::string why;
    const int rc = build_plan(ops, nops, buf_bytes, nbufs, B, Hc, Wc, c->prec, c->w_bytes, p, why);
    if (rc != BUGSEG_OK) return dl_fail(c, rc, why);
    DeviceGuard g(c->mem.device);
    // (a forward of the old plan may still be running on any stream: retire synchronises, or keeps a captured arena)
    c->mem.retire(c->plan.arena, c->plan.pinned);
    c->plan = DlPlan();
    if (hipMalloc(&p.arena, p.total) != hipSuccess) {
        (void)hipGetLastError();
        return dl_fail(c, BUGSEG_ENOMEM, "activation arena allocation failed");   // no plan now
    }
    c->plan = std::move(p);
    return BUGSEG_OK;
}

int bugseg_dl_forward(bugseg_dl *c, const uint8_t *rgb_dev, int B, int H, int W, int64_t *out_dev, void *stream) {
    if (!c || !rgb_dev || !out_dev) return dl_fail(c, BUGSEG_EINVAL, "null argument");
    if (c->plan.ops.empty()) return dl_fail(c, BUGSEG_ESTATE, "forward before set_plan");
    if (const int rc = check_frame(c, B, H, W)) return rc;
    DeviceGuard g(c->mem.device);
    DlIo io;
    io.img = rgb_dev; io.H = H; io.W = W; io.out = out_dev;
    return run_plan(c, io, launch_stream(c, stream));
}

int bugseg_dl_set_class_lut(bugseg_dl *c, const uint8_t *lut, int n) {
    if (!c) return dl_fail(c, BUGSEG_EINVAL, "null argument");
    if (!lut) {   // identity
        n = 0;
    } else {
        if (n < 1 || n > 256) return dl_fail(c, BUGSEG_EINVAL, "a class LUT has 1 to 256 entries, got " + std::to_string(n));
        const DlOp *am = argmax_op(c->plan);
        if (am && am->argmax.ncls != n)
            return dl_fail(c, BUGSEG_EINVAL, "class LUT of " + std::to_string(n) + " entries for a plan of " +
                                                 std::to_string(am->argmax.ncls) + " classes");
    }
    uint8_t host[256];
    for (int k = 0; k < 256; ++k) host[k] = lut && k < n ? lut[k] : (uint8_t)k;
    DeviceGuard g(c->mem.device);
    // a synchronous copy from pageable memory, in place (a captured graph goes on reading this table): it
    // orders after every earlier forward's reads of the old table, and leaves nothing for a later captured
    // step to copy
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(c->dev_lut, host, 256, hipMemcpyHostToDevice) != hipSuccess)
        return dl_fail(c, BUGSEG_EHIP, "class LUT upload failed");
    c->lut_n = n;
    return BUGSEG_OK;
}

int bugseg_dl_forward_classes(bugseg_dl *c, const uint8_t *img_dev, int bgr, int B, int H, int W, uint8_t *seg_dev,
                              int row0, int row1, void *stream) {
    if (!c || !img_dev || !seg_dev) return dl_fail(c, BUGSEG_EINVAL, "null argument");
    if (bgr != 0 && bgr != 1) return dl_fail(c, BUGSEG_EINVAL, "bgr must be 0 or 1");
    if (c->plan.ops.empty()) return dl_fail(c, BUGSEG_ESTATE, "forward before set_plan");
    if (const int rc = check_frame(c, B, H, W)) return rc;
    if (const int rc = check_classes(c, H, row0, row1)) return rc;
    DeviceGuard g(c->mem.device);
    DlIo io;
    io.img = img_dev; io.bgr = bgr; io.H = H; io.W = W; io.seg = seg_dev; io.row0 = row0; io.row1 = row1;
    return run_plan(c, io, launch_stream(c, stream));
}

int bugseg_dl_classes_from_logits(bugseg_dl *c, int B, int H, int W, uint8_t *seg_dev, int row0, int row1, void *stream) {
    if (!c || !seg_dev) return dl_fail(c, BUGSEG_EINVAL, "null argument");
    const DlPlan &p = c->plan;
    if (!p.has_logits) return dl_fail(c, BUGSEG_ESTATE, "classes_from_logits before a forward of this plan");
    if (const int rc = check_frame(c, B, H, W)) return rc;
    if (H != p.last.H || W != p.last.W)
        return dl_fail(c, BUGSEG_EINVAL, "the last forward ran " + std::to_string(p.last.H) + "x" + std::to_string(p.last.W) +
                                             " frames, not " + std::to_string(H) + "x" + std::to_string(W));
    if (const int rc = check_classes(c, H, row0, row1)) return rc;
    DeviceGuard g(c->mem.device);
    DlIo io = p.last;
    io.seg = seg_dev; io.row0 = row0; io.row1 = row1;
    const hipError_t e = run_op(c, *argmax_op(p), io, launch_stream(c, stream));
    return e == hipSuccess ? BUGSEG_OK : dl_fail(c, BUGSEG_EHIP, hipGetErrorString(e));
}

int bugseg_dl_launch_op(bugseg_dl *c, int op, void *stream) {
    if (!c || op < 0 || op >= (int)c->plan.ops.size() || !c->plan.last.img) return dl_fail(c, BUGSEG_EINVAL, "no such op / no forward yet");
    DeviceGuard g(c->mem.device);
    const hipError_t e = run_op(c, c->plan.ops[op], c->plan.last, launch_stream(c, stream));
    return e == hipSuccess ? BUGSEG_OK : dl_fail(c, BUGSEG_EHIP, hipGetErrorString(e));
}

int bugseg_dl_read_buffer(bugseg_dl *c, int buf, void *dst_dev, size_t bytes, void *stream) {
    if (!c || !dst_dev || !c->plan.arena || buf < 0 || buf >= (int)c->plan.buf_bytes.size() || bytes > c->plan.buf_bytes[buf])
        return dl_fail(c, BUGSEG_EINVAL, "no such buffer / too many bytes");
    DeviceGuard g(c->mem.device);
    const hipError_t e = hipMemcpyAsync(dst_dev, bufp(c->plan, buf), bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? BUGSEG_OK : dl_fail(c, BUGSEG_EHIP, hipGetErrorString(e));
}

int bugseg_dl_debug_knobs(const bugseg_dl *c, char *buf, int len) {
    std::string err;
    const int rc = dump_knobs(c ? &c->knobs : nullptr, buf, len, err);
    return rc == BUGSEG_OK ? rc : dl_fail(const_cast<bugseg_dl *>(c), rc, err);
}

const char *bugseg_dl_last_error(const bugseg_dl *c) { return c ? c->err.c_str() : g_dl_err.c_str(); }

}  // extern "C"
