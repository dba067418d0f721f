// Canny edge detection (cv2.Canny, apertureSize 3, L1 gradient; create_skeleton, image_processing_utils.py:95-105)
// on the device, batched: Sobel gradient and non-maximum suppression in one launch, hysteresis as connected
// component labelling. Semantics: DESIGN.md §6.19. Everything is integer: the result does not depend on the
// order atomics land in.
//
// The host entry points (bugseg_canny*) live here beside the kernels: the runtime translation units reference
// nothing of this file (tests/asan links them without it); this file uses what bugseg_internal.h and the
// runtime export.
//
// Launch sequence of one call (fixed: nothing is read back by the host), B frames each:
//   0 nms     u8 image -> map byte per pixel: 2 strong, 0 weak, 1 none. The tile and a 2-pixel halo are staged
//             in LDS with the image border replicated; dx, dy and |dx| + |dy| of the tile and a 1-pixel ring are
//             formed there (0 outside the image) and never reach memory
//   1 tile    ccl_common.h's labelling of the candidate (strong or weak) pixels of a 16 x 64 tile in LDS,
//             8-connected. Only candidate pixels have a label: the other words of the label image are never read
//   2 merge   ccl_common.h's unions across tile borders, one thread per border pixel of a tile
//   3 mark   every strong pixel walks to its root r and stores ~r there: a negative label is a root whose
//             component holds a strong pixel
//   4 out     out[p] = 255 if p is a candidate and the label of its root is negative, else 0
// There is no flatten launch: launch 4 walks the same chain a flatten would, once, and writes no label.
//
// Workspace: 5 bytes per pixel (the map, one int32 label) plus alignment.
//
// Visibility across workgroups: the rule in ccl_common.h, which the merge and mark launches follow for every
// label word. In the mark launch a walker that meets a negative label has found its root already marked.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "bugseg_internal.h"
#include "ccl_common.h"
#include "../../include/bugseg.h"

namespace {

using namespace bugseg;

constexpr int THREADS = 256;
constexpr int NM_TH = 32, NM_TW = 64;     // nms: output tile
constexpr int NM_PH = NM_TH + 4, NM_PW = NM_TW + 4;     // pixels with the 2-pixel halo
constexpr int NM_GH = NM_TH + 2, NM_GW = NM_TW + 2;     // gradients with the 1-pixel ring
constexpr int LT_BORDER = LT_TW + 2 * (LT_TH - 1);     // merge: the pixels of a tile with a neighbour in another
constexpr int TG22 = 13573;               // int(tan(22.5 deg) * 2^15 + 0.5)
constexpr uint8_t STRONG = 2, WEAK = 0, NONE = 1;

struct CannyArgs {
    const uint8_t *img;   // (B, rows, cols)
    uint8_t *mapw;        // launch 0 writes it: map_stride bytes per frame
    const uint8_t *map;   // launches 1-4 read it: map_stride bytes per frame
    uint8_t *out;         // (B, rows, cols)
    int *label;           // workspace, per frame: n words
    size_t map_stride;
    int B, rows, cols, low, high;
    int n;                // rows * cols
    int tiles_x;          // of the launch's tiling
};

__device__ inline bool cand(uint8_t m) { return m == STRONG || m == WEAK; }

// ---------------------------------------------------------------- 0: gradient and non-maximum suppression
__global__ __launch_bounds__(THREADS) void canny_nms_kernel(CannyArgs a) {
    __shared__ uint8_t px[NM_PH * NM_PW];
    __shared__ int dxy[NM_GH * NM_GW];        // dx in the low half, dy in the high half
    __shared__ uint16_t mag[NM_GH * NM_GW];   // |dx| + |dy| <= 2040
    const int W = a.cols, H = a.rows;
    const int tyi = blockIdx.x / a.tiles_x, txi = blockIdx.x - tyi * a.tiles_x;
    const int x0 = txi * NM_TW, y0 = tyi * NM_TH;
    const uint8_t *img = a.img + (size_t)blockIdx.y * a.n;
    uint8_t *dst = a.mapw + (size_t)blockIdx.y * a.map_stride;
    const int tid = threadIdx.x;
    // rows y0 - 2 .., cols x0 - 2 .., the border replicated
    for (int i = tid; i < NM_PH * NM_PW; i += THREADS) {
        int r = i / NM_PW, c = i - r * NM_PW;
        int gy = min(max(y0 - 2 + r, 0), H - 1), gx = min(max(x0 - 2 + c, 0), W - 1);
        px[i] = img[(size_t)gy * W + gx];
    }
    __syncthreads();
    // rows y0 - 1 .., cols x0 - 1 ..
    for (int i = tid; i < NM_GH * NM_GW; i += THREADS) {
        int r = i / NM_GW, c = i - r * NM_GW;
        int gy = y0 - 1 + r, gx = x0 - 1 + c;
        const uint8_t *p = px + (r + 1) * NM_PW + c + 1;
        int nw = p[-NM_PW - 1], nn = p[-NM_PW], ne = p[-NM_PW + 1], ww = p[-1], ee = p[1];
        int sw = p[NM_PW - 1], ss = p[NM_PW], se = p[NM_PW + 1];
        int dx = (ne + 2 * ee + se) - (nw + 2 * ww + sw);
        int dy = (sw + 2 * ss + se) - (nw + 2 * nn + ne);
        bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        dxy[i] = (int)((unsigned)(dx & 0xffff) | ((unsigned)dy << 16));
        mag[i] = in ? (uint16_t)(abs(dx) + abs(dy)) : (uint16_t)0;
    }
    __syncthreads();
    for (int i = tid; i < NM_TH * NM_TW; i += THREADS) {
        int r = i / NM_TW, c = i - r * NM_TW;
        int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        const int g = (r + 1) * NM_GW + c + 1;
        const int m = mag[g];
        uint8_t v = NONE;
        if (m > a.low) {
            const int d = dxy[g];
            const int dx = (int)(short)(d & 0xffff), dy = d >> 16;
            const int x = abs(dx), y = abs(dy) << 15;
            const int tg22x = x * TG22, tg67x = tg22x + (x << 16);
            bool peak;
            if (y < tg22x) peak = m > mag[g - 1] && m >= mag[g + 1];
            else if (y > tg67x) peak = m > mag[g - NM_GW] && m >= mag[g + NM_GW];
            else {
                int s = (dx ^ dy) < 0 ? -1 : 1;
                peak = m > mag[g - NM_GW - s] && m > mag[g + NM_GW + s];
            }
            if (peak) v = m > a.high ? STRONG : WEAK;
        }
        dst[(size_t)gy * W + gx] = v;
    }
}

// ---------------------------------------------------------------- 1, 2: labelling (ccl_common.h)
// The pixels of one frame: a candidate joins its W, NW, N and NE candidate neighbours, any other pixel nothing.
struct CannyPixels {
    static constexpr bool HAS_BG = false, HAS_NONE = true;
    const uint8_t *map;
    int *label;
    int W, H;
    __device__ CannyPixels(const CannyArgs &a, size_t f)
        : map(a.map + f * a.map_stride), label(a.label + f * a.n), W(a.cols), H(a.rows) {}
    __device__ uint8_t kind(int p) const { return cand(map[p]) ? 1 : 2; }
    __device__ void store(int p, int root) const { label[p] = root; }
};

__global__ __launch_bounds__(THREADS) void canny_tile_kernel(CannyArgs a) {
    const int tyi = blockIdx.x / a.tiles_x, txi = blockIdx.x - tyi * a.tiles_x;
    label_tile<THREADS>(CannyPixels(a, blockIdx.y), txi * LT_TW, tyi * LT_TH);
}

// One thread per pixel of a tile's top row, left column and right column (LT_BORDER of them), tiles along grid x.
__global__ __launch_bounds__(THREADS) void canny_merge_kernel(CannyArgs a) {
    const long long idx = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int tile = (int)(idx / LT_BORDER), k = (int)(idx - (long long)tile * LT_BORDER);
    const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
    const int ty = k < LT_TW ? 0 : (k - LT_TW) % (LT_TH - 1) + 1;
    const int tx = k < LT_TW ? k : k < LT_TW + LT_TH - 1 ? 0 : LT_TW - 1;
    const int y = tyi * LT_TH + ty, x = txi * LT_TW + tx;
    if (y >= a.rows || x >= a.cols) return;     // (also every thread past the last tile: its y is past the frame)
    const CannyPixels px(a, blockIdx.y);
    link_border(px, px.label, x, y, tx, ty);
}

// ---------------------------------------------------------------- 3: mark the roots of strong pixels
__global__ __launch_bounds__(THREADS) void canny_mark_kernel(CannyArgs a) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const size_t f = blockIdx.y;
    if (a.map[f * a.map_stride + p] != STRONG) return;
    int *lab = a.label + f * a.n;
    int x = p;
    for (;;) {
        int q = ld_agent(lab + x);
        if (q < 0) return;                      // its root, already marked
        if (q == x) break;
        x = q;
    }
    __hip_atomic_store(lab + x, ~x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- 4: out
__global__ __launch_bounds__(THREADS) void canny_out_kernel(CannyArgs a) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const size_t f = blockIdx.y;
    uint8_t v = 0;
    if (cand(a.map[f * a.map_stride + p])) {
        const int *lab = a.label + f * a.n;
        int x = p;
        for (;;) {
            int q = lab[x];
            if (q < 0) { v = 255; break; }
            if (q == x) break;
            x = q;
        }
    }
    a.out[f * a.n + p] = v;
}

// n is checked: B * n fits an int with one more block of THREADS indices
size_t canny_ws_bytes(size_t n, int B) { return (size_t)B * (pad256(n) + 4 * n) + 256; }

bool canny_shape_ok(const bugseg_canny_params *p, int B) {
    if (B < 1 || B > 65535 || p->rows < 1 || p->cols < 1) return false;
    if ((long long)B * p->rows * (long long)p->cols > (long long)INT_MAX - THREADS ||
        (long long)p->rows * p->cols > (long long)INT_MAX - THREADS)
        return false;
    // a launch is refused by the runtime once gridDim.x * blockDim.x passes 2^32 - 1. The pixel launches stay
    // below it by the test above; the tile launches do not for frames thinner than a tile (a 1 x cols frame has
    // cols / 64 tiles of 256 threads), so such frames are refused here, with the rest, before anything is launched
    const long long nms_tiles = (long long)((p->cols + NM_TW - 1LL) / NM_TW) * ((p->rows + NM_TH - 1LL) / NM_TH);
    const long long lab_tiles = (long long)((p->cols + LT_TW - 1LL) / LT_TW) * ((p->rows + LT_TH - 1LL) / LT_TH);
    return std::max(nms_tiles, lab_tiles) * THREADS <= (long long)UINT_MAX;
}

// stage -1: the whole call; 0: launch 0 alone, the map into `out`; 1: launches 1-4 alone, `in` read as a map
int canny(bugseg_ctx *ctx, const uint8_t *in, int B, const bugseg_canny_params *p, uint8_t *out, void *ws, size_t ws_bytes,
          int stage, void *stream) {
    if (!ctx || !in || !p || !out) return ctx_fail(ctx, BUGSEG_EINVAL, "canny: NULL argument");
    if (B < 1) return ctx_fail(ctx, BUGSEG_EINVAL, "canny: B must be at least 1");
    if (B > 65535) return ctx_fail(ctx, BUGSEG_EINVAL, "canny: B above 65535");
    if (p->rows < 1 || p->cols < 1) return ctx_fail(ctx, BUGSEG_EINVAL, "canny: bad shape");
    if (!canny_shape_ok(p, B)) return ctx_fail(ctx, BUGSEG_EINVAL, "canny: B * rows * cols too large for an int32 index, or a frame's tiles for one launch grid");
    const size_t n = (size_t)p->rows * p->cols;
    if (!ws || ws_bytes < canny_ws_bytes(n, B))
        return ctx_fail(ctx, BUGSEG_EINVAL, "canny: workspace missing or smaller than bugseg_canny_workspace_bytes()");
    if (ranges_overlap(out, n * B, in, n * B)) return ctx_fail(ctx, BUGSEG_EINVAL, "canny: out_dev overlaps the input");
    DeviceGuard g(ctx_device(ctx));
    CannyArgs a;
    a.img = in; a.out = out;
    a.B = B; a.rows = p->rows; a.cols = p->cols; a.low = p->low; a.high = p->high;
    a.n = (int)n;
    unsigned char *w = align256(ws);
    a.mapw = w; a.map = w; a.map_stride = pad256(n);
    a.label = (int *)(w + (size_t)B * a.map_stride);
    if (stage == 0) { a.mapw = out; a.map_stride = n; }
    if (stage == 1) { a.map = in; a.map_stride = n; }
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(THREADS);
    const dim3 px((unsigned)((n + THREADS - 1) / THREADS), (unsigned)B);
    // tiles are numbered along grid x; canny_shape_ok passed only shapes whose tile counts, times THREADS, fit it
    // (the merge launch has fewer workgroups than the labelling launch: LT_BORDER < THREADS)
    const int ntx = (p->cols + NM_TW - 1) / NM_TW, nty = (p->rows + NM_TH - 1) / NM_TH;
    const int ltx = (p->cols + LT_TW - 1) / LT_TW, lty = (p->rows + LT_TH - 1) / LT_TH;
    const dim3 ntiles((unsigned)((long long)ntx * nty), (unsigned)B), ltiles((unsigned)((long long)ltx * lty), (unsigned)B);
    const dim3 border((unsigned)(((long long)ltx * lty * LT_BORDER + THREADS - 1) / THREADS), (unsigned)B);
    const int first = stage == 1 ? 1 : 0, last = stage == 0 ? 1 : 5;
    for (int op = first; op < last; ++op) {
        switch (op) {
        case 0: a.tiles_x = ntx; hipLaunchKernelGGL(canny_nms_kernel, ntiles, blk, 0, s, a); break;
        case 1: a.tiles_x = ltx; hipLaunchKernelGGL(canny_tile_kernel, ltiles, blk, 0, s, a); break;
        case 2: a.tiles_x = ltx; hipLaunchKernelGGL(canny_merge_kernel, border, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL(canny_mark_kernel, px, blk, 0, s, a); break;
        default: hipLaunchKernelGGL(canny_out_kernel, px, blk, 0, s, a); break;
        }
        if (int rc = launch_fail(ctx, "canny")) return rc;
    }
    return BUGSEG_OK;
}

}  // namespace

extern "C" {

size_t bugseg_canny_workspace_bytes(const bugseg_canny_params *p, int B) {
    if (!p || !canny_shape_ok(p, B)) return 0;
    return canny_ws_bytes((size_t)p->rows * p->cols, B);
}

int bugseg_canny(bugseg_ctx *ctx, const uint8_t *img_dev, int B, const bugseg_canny_params *p, uint8_t *out_dev,
                 void *workspace_dev, size_t workspace_bytes, void *stream) {
    return canny(ctx, img_dev, B, p, out_dev, workspace_dev, workspace_bytes, -1, stream);
}

int bugseg_debug_canny_stage(bugseg_ctx *ctx, const uint8_t *in_dev, int B, const bugseg_canny_params *p, int stage,
                             uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (stage != 0 && stage != 1) return bugseg::ctx_fail(ctx, BUGSEG_EINVAL, "canny: stage must be 0 or 1");
    return canny(ctx, in_dev, B, p, out_dev, workspace_dev, workspace_bytes, stage, stream);
}

}
