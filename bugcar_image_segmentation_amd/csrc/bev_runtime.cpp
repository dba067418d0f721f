// Host side of the BEV rasteriser (bev_kernels.hip): geometry, the cached per-geometry tables (BevState) and the
// C entries. Built with the ENet runtime's flags: the polar tables and cv::invert are bit-exact host float code.
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

#include "bugseg_internal.h"
#include "bev_runtime.h"
#include "../../include/bugseg.h"

using namespace bugseg;

namespace {

int fail(bugseg_ctx *c, int code, const std::string &m) { return ctx_fail(c, code, m.c_str()); }

// ---- laserscan-like mode: cv::warpPolar's remap tables (imgwarp.cpp 4.x), built on the host once
// per geometry. Forward: polar (rho, phi) -> grid cell, phi the row of a ph x pw polar image,
// x = (float)(rho*Kmag) * cos(Kangle*phi) + cx in double, rounded to float, then half-to-even to a
// short (remap INTER_NEAREST). Inverse: grid cell -> (rho, polar row) through hal::magnitude32f /
// fastAtan32f (the AVX2 dispatch: fused polynomial) on float offsets, the BORDER_WRAP row of
// copyMakeBorder folded into the row index. -1 = outside (BORDER_TRANSPARENT).
#pragma clang fp contract(off)
const float kAtanP1 = 0.9997878412794807f * (float)(180 / 3.1415926535897932384626433832795);
const float kAtanP3 = -0.3258083974640975f * (float)(180 / 3.1415926535897932384626433832795);
const float kAtanP5 = 0.1555786518463281f * (float)(180 / 3.1415926535897932384626433832795);
const float kAtanP7 = -0.04432655554792128f * (float)(180 / 3.1415926535897932384626433832795);

float fast_atan_rad(float y, float x) {
    const float ax = std::fabs(x), ay = std::fabs(y);
    const float c = std::min(ax, ay) / (std::max(ax, ay) + (float)2.220446049250313e-16);
    const float cc = c * c;
    float a = std::fma(std::fma(std::fma(cc, kAtanP7, kAtanP5), cc, kAtanP3), cc, kAtanP1) * c;
    if (!(ax >= ay)) a = 90.f - a;
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a * (float)(3.1415926535897932384626433832795 / 180);
}

int round_short(float v) {
    const long r = std::lrint(v);
    return (int)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}

void polar_tables(int pw, int ph, double max_radius, float cx, float cy, int w, int h, std::vector<int32_t> &fmap,
                  std::vector<int32_t> &imap) {
    const double CV_2PI = 6.283185307179586476925286766559;
    const double Kangle = CV_2PI / ph, Kmag = max_radius / pw;
    fmap.resize((size_t)pw * ph);
    for (int phi = 0; phi < ph; ++phi) {
        const double KKy = Kangle * phi, cp = std::cos(KKy), sp = std::sin(KKy);
        for (int rho = 0; rho < pw; ++rho) {
            const float r = (float)(rho * Kmag);
            const float mx = (float)(r * cp + (double)cx), my = (float)(r * sp + (double)cy);
            const int sx = round_short(mx), sy = round_short(my);
            fmap[(size_t)phi * pw + rho] = ((unsigned)sx < (unsigned)w && (unsigned)sy < (unsigned)h) ? (sx | (sy << 16)) : -1;
        }
    }
    imap.resize((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const float bx = (float)x - cx, by = (float)y - cy;
            const float mag = std::sqrt(std::fma(bx, bx, by * by));
            const float ang = fast_atan_rad(by, bx);
            const double rho = mag / Kmag, phi = ang / Kangle;
            const float mx = (float)rho, my = (float)phi + 1;
            const int X = round_short(mx), Y = round_short(my);
            int32_t v = -1;
            if ((unsigned)X < (unsigned)pw && (unsigned)Y < (unsigned)(ph + 2)) {
                const int row = Y == 0 ? ph - 1 : (Y == ph + 1 ? 0 : Y - 1);
                v = X | (row << 16);
            }
            imap[(size_t)y * w + x] = v;
        }
}
#pragma clang fp contract(on)

// warpPolar dsize: (-1, -1) -> (round(L), round(L*pi)) for create_occupancy_grid (bev.py:219); the
// explicit (w, h) of create_occupancy_grid_binary (bev.py:146). False if the tables cannot hold it.
bool polar_dims(int w, int h, int variant, int &pw, int &ph) {
    const int L = std::max(w, h);
    pw = variant ? w : (int)std::lrint((double)L);
    ph = variant ? h : (int)std::lrint((double)L * 3.1415926535897932384626433832795);
    return pw > 0 && ph > 0 && pw <= 32767 && ph <= 32767 && w <= 32767 && h <= 32767;
}

// Laserscan batch scratch: cells (B*occ_h*occ_w u8, 256-B aligned) then rmin (B*ph int32).
size_t ls_cells_bytes(int B, const bugseg_bev_params *p) { return ((size_t)B * p->occ_w * p->occ_h + 255) & ~(size_t)255; }
size_t ls_workspace_bytes(int B, const bugseg_bev_params *p, int ph) {
    return ls_cells_bytes(B, p) + (size_t)B * ph * sizeof(int32_t);
}

// The polar tables (pw x ph: polar_dims) of a laserscan call, cached per grid; fills a.fmap / imap / pw / ph / hit.
int prepare_polar(bugseg_ctx *ctx, const bugseg_bev_params *p, BevArgs &a, bool cap, int pw, int ph) {
    const int w = p->occ_w, h = p->occ_h, L = std::max(w, h);
    int rc = BUGSEG_OK;
    const auto *hit = ctx_bev(ctx).polar_tabs.get(ctx_memory(ctx), {w, h, p->variant}, cap, true, &rc, [&](auto &t) -> int {
        std::vector<int32_t> fmap, imap;
        polar_tables(pw, ph, (double)L, (float)(w / 2.0 - 1), (float)h, w, h, fmap, imap);
        t.pw = pw; t.ph = ph;
        const hipError_t e = ctx_memory(ctx).upload({{fmap.data(), fmap.size() * 4}, {imap.data(), imap.size() * 4}}, &t.tab);
        if (e == hipSuccess) return BUGSEG_OK;
        if (e == hipErrorOutOfMemory) return fail(ctx, BUGSEG_ENOMEM, "polar table allocation failed");
        return fail(ctx, BUGSEG_EHIP, std::string("polar table upload: ") + hipGetErrorString(e));
    });
    if (!hit) return rc;
    a.fmap = (const int32_t *)hit->tab;
    a.imap = (const int32_t *)hit->tab + (size_t)pw * ph;
    a.pw = pw; a.ph = ph;
    a.laserscan = 1; a.hit = p->variant ? 100 : 3;
    return BUGSEG_OK;
}

// The scratch-owning entry's per-stream laserscan scratch (bugseg_bev_occgrid without a workspace). Not a
// TableCache: keyed by stream, 8 entries, the least recently used unpinned one goes, a buffer regrows in place.
int internal_scratch(bugseg_ctx *ctx, void *stream, size_t need, bool cap, void *&out) {
    BevState &bs = ctx_bev(ctx);
    CtxMemory &mem = ctx_memory(ctx);
    BevState::LsScratch *sc = nullptr;
    for (auto &x : bs.ls_scratch) if (x.stream == stream) sc = &x;
    if (!sc) {
        auto victim = bs.ls_scratch.end();
        for (auto i = bs.ls_scratch.begin(); i != bs.ls_scratch.end() && bs.ls_scratch.size() >= 8; ++i)
            if (!i->pinned && (victim == bs.ls_scratch.end() || i->used < victim->used)) victim = i;
        if (victim != bs.ls_scratch.end()) {
            mem.retire(victim->p, cap);
            bs.ls_scratch.erase(victim);
        }
        bs.ls_scratch.push_back({stream});
        sc = &bs.ls_scratch.back();
    }
    sc->used = ++bs.use_clock;
    if (need > sc->bytes) {
        // work already enqueued on this stream (or captured from it) may still use the old buffer
        mem.retire(sc->p, cap || sc->pinned);
        sc->p = nullptr; sc->bytes = 0;
        RelaxCapture relax;
        if (hipMalloc(&sc->p, need) != hipSuccess) return fail(ctx, BUGSEG_ENOMEM, "laserscan scratch allocation failed");
        sc->bytes = need;
    }
    if (cap) sc->pinned = true;
    out = sc->p;
    return BUGSEG_OK;
}

// what warp_tap (bev_kernels.hip) reads: the sizes of the source and of the warped image, the inverse matrix and
// the x-block width; every other field of `a` is zeroed. The sizes are positive (the callers check).
void warp_geometry(const bugseg_bev_params *p, BevArgs &a) {
    std::memset(&a, 0, sizeof(a));
    a.in_rows = p->in_rows; a.in_cols = p->in_cols;
    {
        // cv::invert(M) closed-form 3x3 branch (DECOMP_LU), as warpPerspective does without WARP_INVERSE_MAP
#pragma clang fp contract(off)
        const double *S = p->M;
        double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
        if (d != 0.0) {
            d = 1.0 / d;
            a.Mi[0] = (S[4] * S[8] - S[5] * S[7]) * d;
            a.Mi[1] = (S[2] * S[7] - S[1] * S[8]) * d;
            a.Mi[2] = (S[1] * S[5] - S[2] * S[4]) * d;
            a.Mi[3] = (S[5] * S[6] - S[3] * S[8]) * d;
            a.Mi[4] = (S[0] * S[8] - S[2] * S[6]) * d;
            a.Mi[5] = (S[2] * S[3] - S[0] * S[5]) * d;
            a.Mi[6] = (S[3] * S[7] - S[4] * S[6]) * d;
            a.Mi[7] = (S[1] * S[6] - S[0] * S[7]) * d;
            a.Mi[8] = (S[0] * S[4] - S[1] * S[3]) * d;
        }
    }
    const int bh0 = std::min(16, p->warp_h);
    a.bw0 = std::min(1024 / bh0, p->warp_w);
    a.warp_w = p->warp_w; a.warp_h = p->warp_h;
}

// the geometry fields of the rasteriser's arguments from the caller's parameters (checked)
int bev_geometry(bugseg_ctx *ctx, const bugseg_bev_params *p, BevArgs &a) {
    if (p->in_rows <= 0 || p->in_cols <= 0 || p->warp_w <= 0 || p->warp_h <= 0 || p->occ_w <= 0 ||
        p->occ_h <= 0 || p->occ_w_px <= 0 || p->occ_h_px <= 0)
        return fail(ctx, BUGSEG_EINVAL, "bad BEV geometry");
    if (p->variant != 0 && p->variant != 1) return fail(ctx, BUGSEG_EINVAL, "variant must be 0 or 1");
    if (p->laserscan != 0 && p->laserscan != 1) return fail(ctx, BUGSEG_EINVAL, "laserscan must be 0 or 1");
    warp_geometry(p, a);
    a.occ_w_px = p->occ_w_px; a.occ_h_px = p->occ_h_px; a.occ_w = p->occ_w; a.occ_h = p->occ_h;
    a.left_x = p->left_x; a.top_y = p->top_y;
    a.ifx = 1.0 / ((double)p->occ_w / p->occ_w_px);
    a.ify = 1.0 / ((double)p->occ_h / p->occ_h_px);
    a.ros_layout = p->ros_layout;
    a.variant = p->variant;
    return BUGSEG_OK;
}

using BevTab = decltype(BevState::bev_tabs)::Entry;

// Fills the allocated t.tab on the setup stream `s`: the kernel, then the work items and source rows from its records.
hipError_t build_bev_table(const Knobs &knobs, BevArgs &a, BevTab &t, hipStream_t s) {
    a.wtab = (uint4 *)t.tab;
    hipError_t e = launch_bev_table(a, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // only the build itself is waited for
    // the band-staged form's work items: one per (band, row part), the far bands first, whose workgroups
    // live longest and so are dispatched first (DESIGN.md "Workgroup order": 26.2 -> 23.7 us per 32 frames)
    const int nb = bev_bands(a.occ_h);
    std::vector<int4> rec((size_t)nb * BEV_BOXREC);
    std::vector<int2> items;
    if (e == hipSuccess)
        e = hipMemcpyAsync(rec.data(), (unsigned char *)t.tab + bev_records_offset(a.occ_w, a.occ_h),
                           rec.size() * sizeof(int4), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) {
        // (BUGSEG_BEV_NEAR_FIRST=1: the earlier order, nearest bands first; A/B)
        for (int i = 0; i < nb; ++i) {
            const int b = knobs.bev_near_first ? nb - 1 - i : i;
            for (int k = 0; k < std::max(1, std::min(BEV_BAND, rec[(size_t)b * BEV_BOXREC].x)); ++k) items.push_back(make_int2(b, k));
        }
        // the class-map rows the rasteriser's result depends on (bugseg_bev_source_rows): the union
        // of the bands' spans (header .z, .w; lo > hi: no tap of the band carries weight)
        int lo = 1 << 30, hi = -(1 << 30);
        for (int b = 0; b < nb; ++b) {
            const int4 h = rec[(size_t)b * BEV_BOXREC];
            if (h.z <= h.w) { lo = std::min(lo, h.z); hi = std::max(hi, h.w); }
        }
        t.row0 = lo <= hi ? std::max(lo, 0) : 0;
        t.row1 = lo <= hi ? std::min(hi + 1, a.in_rows) : 0;
        e = hipMemcpyAsync((unsigned char *)t.tab + bev_items_offset(a.occ_w, a.occ_h), items.data(),
                           items.size() * sizeof(int2), hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    t.nitems = (int)items.size();
    return e;
}

// The geometry's warp-tap table (cached; shared read-only by every call on any stream) into a.wtab / nitems,
// or null with *rc the error. cap: the caller's stream is being captured; pin: TableCache::get.
const BevTab *bev_table(bugseg_ctx *ctx, BevArgs &a, bool cap, bool pin, int *rc) {
    std::vector<unsigned char> key(sizeof(double) * 11 + sizeof(int) * 12);
    unsigned char *kp = key.data();
    auto put = [&](const void *v, size_t n) { std::memcpy(kp, v, n); kp += n; };
    put(a.Mi, sizeof(a.Mi)); put(&a.ifx, sizeof(double)); put(&a.ify, sizeof(double));
    const int ik[12] = {a.in_rows, a.in_cols, a.bw0, a.warp_w, a.warp_h, a.occ_w_px, a.occ_h_px, a.occ_w, a.occ_h,
                        a.left_x, a.top_y, 0};
    put(ik, sizeof(ik));
    if ((size_t)a.occ_h * a.occ_w * BEV_SLOTS > (size_t)1 << 31) {
        *rc = fail(ctx, BUGSEG_EINVAL, "occupancy grid too large");
        return nullptr;
    }
    const BevTab *hit = ctx_bev(ctx).bev_tabs.get(ctx_memory(ctx), key, cap, pin, rc, [&](BevTab &t) -> int {
        RelaxCapture relax;
        hipStream_t s = ctx_memory(ctx).setup_stream();
        if (!s) return fail(ctx, BUGSEG_EHIP, "could not create the table-build stream");
        if (hipMalloc(&t.tab, bev_table_bytes(a.occ_w, a.occ_h)) != hipSuccess)
            return fail(ctx, BUGSEG_ENOMEM, "BEV table allocation failed");
        const hipError_t e = build_bev_table(ctx_knobs(ctx), a, t, s);
        if (e == hipSuccess) return BUGSEG_OK;
        (void)hipFree(t.tab);
        return fail(ctx, BUGSEG_EHIP, std::string("BEV table: ") + hipGetErrorString(e));
    });
    if (hit) { a.wtab = (uint4 *)hit->tab; a.nitems = hit->nitems; }
    return hit;
}

int bev_occgrid(bugseg_ctx *ctx, const uint8_t *seg, int B, const bugseg_bev_params *p, int8_t *out, bool own_ws,
                void *ws, size_t ws_bytes, void *stream) {
    if (!ctx || !seg || !p || !out) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    if (B <= 0) return fail(ctx, BUGSEG_EINVAL, "bad BEV geometry");
    BevArgs a;
    int rc0 = bev_geometry(ctx, p, a);
    if (rc0 != BUGSEG_OK) return rc0;
    DeviceGuard g(ctx_device(ctx));
    a.seg = seg; a.B = B; a.out = out;
    int pw = 0, ph = 0;
    if (p->laserscan) {
        // check the workspace before anything is built or enqueued
        if (!polar_dims(p->occ_w, p->occ_h, p->variant, pw, ph)) return fail(ctx, BUGSEG_EINVAL, "laserscan grid too large for the polar tables");
        if (!own_ws && (!ws || ws_bytes < ls_workspace_bytes(B, p, ph)))
            return fail(ctx, BUGSEG_EINVAL, "laserscan workspace missing or smaller than bugseg_bev_workspace_bytes()");
    }
    const bool cap = stream_capturing(stream);
    if (!bev_table(ctx, a, cap, true, &rc0)) return rc0;
    if (p->laserscan) {
        int rc = prepare_polar(ctx, p, a, cap, pw, ph);
        if (rc != BUGSEG_OK) return rc;
        if (own_ws) {
            rc = internal_scratch(ctx, stream, ls_workspace_bytes(B, p, a.ph), cap, ws);
            if (rc != BUGSEG_OK) return rc;
        }
        a.cells = (uint8_t *)ws;
        a.rmin = (int32_t *)((unsigned char *)ws + ls_cells_bytes(B, p));
    }
    hipError_t e = launch_bev(ctx_knobs(ctx), a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("bev launch: ") + hipGetErrorString(e));
    return BUGSEG_OK;
}

}  // namespace

extern "C" {

int bugseg_bev_occgrid(bugseg_ctx *ctx, const uint8_t *seg, int B, const bugseg_bev_params *p, int8_t *out, void *stream) {
    return bev_occgrid(ctx, seg, B, p, out, true, nullptr, 0, stream);
}

int bugseg_bev_source_rows(bugseg_ctx *ctx, const bugseg_bev_params *p, int in_rows, int in_cols, int *row0, int *row1) {
    if (!ctx || !p || !row0 || !row1) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    if (in_rows != p->in_rows || in_cols != p->in_cols)
        return fail(ctx, BUGSEG_EINVAL, "source rows: the class map is not the size the parameters name");
    BevArgs a;
    int rc = bev_geometry(ctx, p, a);
    if (rc != BUGSEG_OK) return rc;
    DeviceGuard g(ctx_device(ctx));
    // (the entry takes no stream: it evicts as under a capture, never behind a device sync, and pins nothing)
    const BevTab *hit = bev_table(ctx, a, true, false, &rc);
    if (!hit) return rc;
    *row0 = hit->row0; *row1 = hit->row1;
    return BUGSEG_OK;
}

size_t bugseg_bev_workspace_bytes(const bugseg_bev_params *p, int B) {
    int pw, ph;
    if (!p || B <= 0 || p->occ_w <= 0 || p->occ_h <= 0 || !p->laserscan || !polar_dims(p->occ_w, p->occ_h, p->variant, pw, ph)) return 0;
    return ls_workspace_bytes(B, p, ph);
}

int bugseg_bev_occgrid_ws(bugseg_ctx *ctx, const uint8_t *seg, int B, const bugseg_bev_params *p, int8_t *out,
                          void *workspace, size_t workspace_bytes, void *stream) {
    return bev_occgrid(ctx, seg, B, p, out, false, workspace, workspace_bytes, stream);
}

int bugseg_bev_warp_image(bugseg_ctx *ctx, const uint8_t *img, int B, int channels, const bugseg_bev_params *p, int gray,
                          uint8_t *out, void *stream) {
    if (!ctx || !img || !p || !out) return fail(ctx, BUGSEG_EINVAL, "warp image: NULL argument");
    if (channels != 1 && channels != 3) return fail(ctx, BUGSEG_EINVAL, "warp image: channels must be 1 or 3");
    if ((gray != 0 && gray != 1) || (gray && channels != 3)) return fail(ctx, BUGSEG_EINVAL, "warp image: gray is 0 or 1, and 1 only with 3 channels");
    if (B < 1 || B > 65535 * BEV_WARP_FRAMES) return fail(ctx, BUGSEG_EINVAL, "warp image: B must be at least 1 (and fit the launch grid)");
    if (p->in_rows <= 0 || p->in_cols <= 0 || p->warp_w <= 0 || p->warp_h <= 0) return fail(ctx, BUGSEG_EINVAL, "warp image: an empty source or result");
    const size_t in_frame = (size_t)p->in_rows * p->in_cols * channels, out_frame = (size_t)p->warp_w * p->warp_h * (gray ? 1 : channels);
    if (in_frame > (size_t)INT_MAX || (size_t)p->warp_w * p->warp_h * 3 > (size_t)INT_MAX)
        return fail(ctx, BUGSEG_EINVAL, "warp image: a frame or a result of 2^31 bytes or more");
    if (ranges_overlap(out, out_frame * B, img, in_frame * B)) return fail(ctx, BUGSEG_EINVAL, "warp image: out_dev overlaps the input");
    BevArgs a;
    warp_geometry(p, a);
    a.B = B;
    DeviceGuard g(ctx_device(ctx));
    hipError_t e = launch_bev_warp_image(a, img, channels, gray, out, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("warp image launch: ") + hipGetErrorString(e));
    return BUGSEG_OK;
}

// test hook (host only: no device, no HIP call) — tests/asan drives it under ASan + UBSan
int bugseg_debug_polar_tables(int w, int h, int variant, int32_t *fmap, size_t fmap_n, int32_t *imap, size_t imap_n,
                              int *pw_out, int *ph_out) {
    if (w <= 0 || h <= 0 || w > 32767 || h > 32767) return fail(nullptr, BUGSEG_EINVAL, "bad grid");
    int pw, ph;
    if (!polar_dims(w, h, variant, pw, ph)) return fail(nullptr, BUGSEG_EINVAL, "grid too large for the polar tables");
    std::vector<int32_t> f, im;
    polar_tables(pw, ph, (double)std::max(w, h), (float)(w / 2.0 - 1), (float)h, w, h, f, im);
    if (pw_out) *pw_out = pw;
    if (ph_out) *ph_out = ph;
    if (fmap) std::memcpy(fmap, f.data(), std::min(fmap_n, f.size()) * sizeof(int32_t));
    if (imap) std::memcpy(imap, im.data(), std::min(imap_n, im.size()) * sizeof(int32_t));
    return BUGSEG_OK;
}

}  // extern "C"
