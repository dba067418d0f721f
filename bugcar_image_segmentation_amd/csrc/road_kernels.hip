// contour_noise_removal (image_processing_utils.py:4-44) on the device, batched: morphological closing,
// labelling of the foreground (8-connected) and background (4-connected) regions of the closed mask in one
// label image, the band / ring counts per region, the walk over the nesting of regions, the output pass.
// Semantics: DESIGN.md §6.16. Everything is integer: the result does not depend on the order atomics land in.
//
// The host entry points (bugseg_road_filter*) live here beside the kernels: the runtime translation units
// reference nothing of this file (tests/asan links them without it); this file uses what bugseg_internal.h
// and the runtime export.
//
// Launch sequence of one call (fixed: nothing is read back by the host), B frames each:
//   0 close     u8 map -> closed mask, separable OR then AND from LDS tiles with a halo
//   1 tile      ccl_common.h's labelling of a 16 x 64 tile in LDS; clears the per-root counters of its pixels
//   2 merge     ccl_common.h's unions across tile borders, one thread per pixel of the frame
//   3 flatten   label[p] = root(p)
//   4 count     band and ring counts per root, outside marks
//   5 sub       every root adds its band count to itself and its ancestors
//   6 keep      per root: the nearest qualifying node, from the root upwards
//   7 out       out[p] = keep[label[p]]
//
// Visibility across workgroups: the rule in ccl_common.h, which the merge and sub launches follow. The flatten
// launch reads labels that other workgroups overwrite with their roots: a stale read is an older, still valid,
// ancestor.
#include <hip/hip_runtime.h>

#include <climits>

#include "bugseg_internal.h"
#include "ccl_common.h"
#include "../../include/bugseg.h"

namespace {

using namespace bugseg;

constexpr int THREADS = 256;
constexpr int CL_TH = 32, CL_TW = 64;     // closing: output tile
constexpr int OUTSIDE = INT_MIN;          // sub[] of a background root that touches the image border
constexpr int N_OPS = 8;

struct RoadArgs {
    const uint8_t *seg;   // (B, rows, cols)
    uint8_t *out;         // (B, rows, cols)
    uint8_t *closed;      // workspace, per frame: npad bytes
    int *label, *band, *ring, *sub;   // workspace, per frame: n words each
    int B, rows, cols, k, y_top, min_count;
    int n;                // rows * cols
    size_t npad;          // n rounded up to 256
};

// ---------------------------------------------------------------- 0: closing
// One workgroup = one CL_TH x CL_TW output tile of one frame. a = k / 2 is the anchor of both passes: d(y, x)
// reads fg0 at offsets -a .. k-1-a, c(y, x) reads d at the same offsets. Taps outside the image are ignored
// in both passes: fg0 there is 0 (neutral for OR), d there is 1 (neutral for AND) — not the dilation of a
// zero-padded image. Two LDS images of (CL_TH + 2k - 2) x (CL_TW + 2k - 2) bytes, used alternately.
__global__ __launch_bounds__(THREADS) void road_close_kernel(RoadArgs a) {
    extern __shared__ uint8_t lds[];
    const int k = a.k, lo = k >> 1, W = a.cols, H = a.rows;
    const int C0 = CL_TW + 2 * (k - 1), R0 = CL_TH + 2 * (k - 1);
    const int C1 = CL_TW + k - 1, R1 = CL_TH + k - 1;
    uint8_t *A = lds, *Bf = lds + (size_t)R0 * C0;
    const int x0 = blockIdx.x * CL_TW, y0 = blockIdx.y * CL_TH;
    const uint8_t *seg = a.seg + (size_t)blockIdx.z * a.n;
    uint8_t *dst = a.closed + (size_t)blockIdx.z * a.npad;
    const int tid = threadIdx.x;
    // fg0 over rows y0 - 2 lo .., cols x0 - 2 lo ..
    for (int i = tid; i < R0 * C0; i += THREADS) {
        int r = i / C0, c = i - r * C0;
        int gy = y0 - 2 * lo + r, gx = x0 - 2 * lo + c;
        uint8_t v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = seg[(size_t)gy * W + gx] != 0;
        A[i] = v;
    }
    __syncthreads();
    // OR along the row: column c of Bf is image column x0 - lo + c
    for (int i = tid; i < R0 * C1; i += THREADS) {
        int r = i / C1, c = i - r * C1;
        const uint8_t *p = A + r * C0 + c;
        uint8_t v = 0;
        for (int j = 0; j < k; ++j) v |= p[j];
        Bf[r * C0 + c] = v;
    }
    __syncthreads();
    // OR down the column: row r of A is image row y0 - lo + r; d outside the image is neutral for the AND
    for (int i = tid; i < R1 * C1; i += THREADS) {
        int r = i / C1, c = i - r * C1;
        const uint8_t *p = Bf + r * C0 + c;
        uint8_t v = 0;
        for (int j = 0; j < k; ++j) v |= p[j * C0];
        int gy = y0 - lo + r, gx = x0 - lo + c;
        if (gy < 0 || gy >= H || gx < 0 || gx >= W) v = 1;
        A[r * C0 + c] = v;
    }
    __syncthreads();
    // AND along the row: column c of Bf is image column x0 + c
    for (int i = tid; i < R1 * CL_TW; i += THREADS) {
        int r = i / CL_TW, c = i - r * CL_TW;
        const uint8_t *p = A + r * C0 + c;
        uint8_t v = 1;
        for (int j = 0; j < k; ++j) v &= p[j];
        Bf[r * C0 + c] = v;
    }
    __syncthreads();
    for (int i = tid; i < CL_TH * CL_TW; i += THREADS) {
        int r = i / CL_TW, c = i - r * CL_TW;
        int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        const uint8_t *p = Bf + r * C0 + c;
        uint8_t v = 1;
        for (int j = 0; j < k; ++j) v &= p[j * C0];
        dst[(size_t)gy * W + gx] = v;
    }
}

// ---------------------------------------------------------------- 1, 2: labelling (ccl_common.h)
// The pixels of one frame: the closed mask's foreground is 8-connected, its background 4-connected.
struct RoadPixels {
    static constexpr bool HAS_BG = true, HAS_NONE = false;
    const uint8_t *closed;
    int *label, *band, *ring, *sub;
    int W, H;
    __device__ RoadPixels(const RoadArgs &a, size_t f)
        : closed(a.closed + f * a.npad), label(a.label + f * a.n), band(a.band + f * a.n), ring(a.ring + f * a.n),
          sub(a.sub + f * a.n), W(a.cols), H(a.rows) {}
    __device__ uint8_t kind(int p) const { return closed[p]; }
    __device__ void store(int p, int root) const {
        label[p] = root;
        band[p] = 0;
        ring[p] = 0;
        sub[p] = 0;
    }
};

__global__ __launch_bounds__(THREADS) void road_tile_kernel(RoadArgs a) {
    label_tile<THREADS>(RoadPixels(a, blockIdx.z), blockIdx.x * LT_TW, blockIdx.y * LT_TH);
}

// One thread per pixel of the frame: those with no neighbour in another tile leave at once.
__global__ __launch_bounds__(THREADS) void road_merge_kernel(RoadArgs a) {
    const int W = a.cols;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const int y = p / W, x = p - y * W;
    const int ty = y % LT_TH, tx = x % LT_TW;
    if (ty != 0 && tx != 0 && tx != LT_TW - 1) return;
    const RoadPixels px(a, blockIdx.y);
    link_border(px, px.label, x, y, tx, ty);
}

// ---------------------------------------------------------------- 3: flatten
__global__ __launch_bounds__(THREADS) void road_flatten_kernel(RoadArgs a) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    int *lab = a.label + (size_t)blockIdx.y * a.n;
    int x = p;
    for (;;) {
        int q = lab[x];
        if (q == x) break;
        x = q;
    }
    if (x != p) lab[p] = x;
}

// One atomic per distinct key among the wave's active lanes. Every lane of the wave must call it.
__device__ inline void wave_count(int *base, int key, bool active) {
    unsigned long long todo = __ballot(active);
    const int lane = __lane_id();
    while (todo) {
        int leader = __ffsll((long long)todo) - 1;
        int kk = __shfl(key, leader);
        unsigned long long same = __ballot(active && key == kk);
        if (lane == leader) atomicAdd(base + kk, (int)__popcll(same));
        todo &= ~same;
    }
}

// ---------------------------------------------------------------- 4: band, ring, outside
// band[r]: pixels of region r with y >= y_top. ring[h]: pixels with y >= y_top of the component above h's first
// pixel (h's parent) that have a 4-neighbour in h, once per (pixel, h). sub[r] = OUTSIDE for a background
// region with a pixel in the outermost rows or columns.
__global__ __launch_bounds__(THREADS) void road_count_kernel(RoadArgs a) {
    const int W = a.cols, H = a.rows;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    const bool in = p < a.n;
    const size_t f = blockIdx.y;
    const uint8_t *closed = a.closed + f * a.npad;
    const int *lab = a.label + f * a.n;
    int *band = a.band + f * a.n, *ring = a.ring + f * a.n, *sub = a.sub + f * a.n;
    int y = 0, x = 0, r = 0;
    uint8_t kd = 0;
    if (in) {
        y = p / W; x = p - y * W;
        r = lab[p];
        kd = closed[p];
        if (kd == 0 && (y == 0 || x == 0 || y == H - 1 || x == W - 1)) atomicOr(sub + r, OUTSIDE);
    }
    const bool inband = in && y >= a.y_top;
    wave_count(band, r, inband);
    // the (at most four) distinct background regions beside a foreground band pixel whose parent is r
    int h[4] = {-1, -1, -1, -1};
    if (inband && kd == 1) {
        if (y > 0 && closed[p - W] == 0) h[0] = lab[p - W];
        if (x > 0 && closed[p - 1] == 0) h[1] = lab[p - 1];
        if (x + 1 < W && closed[p + 1] == 0) h[2] = lab[p + 1];
        if (y + 1 < H && closed[p + W] == 0) h[3] = lab[p + W];
        if (h[1] == h[0]) h[1] = -1;
        if (h[2] == h[0] || h[2] == h[1]) h[2] = -1;
        if (h[3] == h[0] || h[3] == h[1] || h[3] == h[2]) h[3] = -1;
        for (int i = 0; i < 4; ++i)
            if (h[i] >= 0 && (h[i] < W || lab[h[i] - W] != r)) h[i] = -1;
    }
    for (int i = 0; i < 4; ++i) wave_count(ring, h[i], h[i] >= 0);
}

// ---------------------------------------------------------------- 5: sub
// Parent of a root u (its raster-first pixel): the region of the pixel above it. A hole always has one; a
// component is top level in row 0 or under an outside region. An outside region is no node.
__global__ __launch_bounds__(THREADS) void road_sub_kernel(RoadArgs a) {
    const int W = a.cols;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const size_t f = blockIdx.y;
    const uint8_t *closed = a.closed + f * a.npad;
    const int *lab = a.label + f * a.n;
    int *sub = a.sub + f * a.n;
    if (lab[p] != p) return;
    const int add = a.band[f * a.n + p];
    if (add == 0 || ld_agent(sub + p) < 0) return;
    int u = p;
    for (;;) {
        atomicAdd(sub + u, add);
        if (u < W) break;
        int b = lab[u - W];
        if (closed[u] == 1 && ld_agent(sub + b) < 0) break;
        u = b;
    }
}

// ---------------------------------------------------------------- 6: keep
// keep (stored in band[root]) = 1 when the nearest qualifying node from the root upwards is a component.
__global__ __launch_bounds__(THREADS) void road_keep_kernel(RoadArgs a) {
    const int W = a.cols;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const size_t f = blockIdx.y;
    const uint8_t *closed = a.closed + f * a.npad;
    const int *lab = a.label + f * a.n;
    const int *sub = a.sub + f * a.n, *ring = a.ring + f * a.n;
    if (lab[p] != p) return;
    int u = p, res = 0;
    for (;;) {
        int s = sub[u];
        if (s < 0) break;                       // outside: no node, nothing above
        bool fg = closed[u] == 1;
        long long cnt = fg ? (long long)s : (long long)s + ring[u];
        if (cnt >= a.min_count) { res = fg; break; }
        if (u < W) break;
        u = lab[u - W];
    }
    a.band[f * a.n + p] = res;
}

// ---------------------------------------------------------------- 7: out
__global__ __launch_bounds__(THREADS) void road_out_kernel(RoadArgs a) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const size_t f = blockIdx.y;
    a.out[f * a.n + p] = (uint8_t)a.band[f * a.n + a.label[f * a.n + p]];
}

size_t road_ws_bytes(size_t n, int B) { return (size_t)B * (pad256(n) + 4 * 4 * n) + 256; }

int road_filter(bugseg_ctx *ctx, const uint8_t *seg, int B, const bugseg_road_filter_params *p, uint8_t *out, void *ws,
                size_t ws_bytes, int first, int last, void *stream) {
    if (!ctx || !seg || !p || !out) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: NULL argument");
    if (B < 1) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: B must be at least 1");
    if (p->rows < 1 || p->cols < 1) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: bad shape");
    if (p->k < 1 || p->k > 64) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: k must be in [1, 64]");
    if (p->y_top < 0 || p->y_top >= p->rows) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: y_top must be in [0, rows)");
    if (p->min_count < 1) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: min_count must be at least 1");
    const long long n64 = (long long)p->rows * p->cols;
    // (one more block of THREADS indices must still fit an int)
    if (n64 > INT_MAX - THREADS) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: rows * cols too large for an int32 index");
    if (B > 65535) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: B above 65535");
    const size_t n = (size_t)n64;
    if (!ws || ws_bytes < road_ws_bytes(n, B))
        return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: workspace missing or smaller than bugseg_road_filter_workspace_bytes()");
    if (last < 0 || last > N_OPS) last = N_OPS;
    if (first < 0 || first > last) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: bad op range");
    if (ranges_overlap(out, n * B, seg, n * B)) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: out_dev overlaps seg_dev");
    DeviceGuard g(ctx_device(ctx));
    RoadArgs a;
    a.seg = seg; a.out = out;
    a.B = B; a.rows = p->rows; a.cols = p->cols; a.k = p->k; a.y_top = p->y_top; a.min_count = p->min_count;
    a.n = (int)n; a.npad = pad256(n);
    unsigned char *w = align256(ws);
    a.closed = w;
    a.label = (int *)(w + (size_t)B * a.npad);
    a.band = a.label + (size_t)B * n;
    a.ring = a.band + (size_t)B * n;
    a.sub = a.ring + (size_t)B * n;
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(THREADS);
    const dim3 px((unsigned)((n + THREADS - 1) / THREADS), (unsigned)B);
    const dim3 ctiles((p->cols + CL_TW - 1) / CL_TW, (p->rows + CL_TH - 1) / CL_TH, B);
    const dim3 ltiles((p->cols + LT_TW - 1) / LT_TW, (p->rows + LT_TH - 1) / LT_TH, B);
    if (ctiles.y > 65535 || ltiles.y > 65535) return ctx_fail(ctx, BUGSEG_EINVAL, "road filter: too many rows");
    const size_t lds = (size_t)2 * (CL_TH + 2 * (p->k - 1)) * (CL_TW + 2 * (p->k - 1));
    for (int op = first; op < last; ++op) {
        switch (op) {
        case 0: hipLaunchKernelGGL(road_close_kernel, ctiles, blk, lds, s, a); break;
        case 1: hipLaunchKernelGGL(road_tile_kernel, ltiles, blk, 0, s, a); break;
        case 2: hipLaunchKernelGGL(road_merge_kernel, px, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL(road_flatten_kernel, px, blk, 0, s, a); break;
        case 4: hipLaunchKernelGGL(road_count_kernel, px, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL(road_sub_kernel, px, blk, 0, s, a); break;
        case 6: hipLaunchKernelGGL(road_keep_kernel, px, blk, 0, s, a); break;
        default: hipLaunchKernelGGL(road_out_kernel, px, blk, 0, s, a); break;
        }
        if (int rc = launch_fail(ctx, "road filter")) return rc;
    }
    return BUGSEG_OK;
}

}  // namespace

extern "C" {

size_t bugseg_road_filter_workspace_bytes(const bugseg_road_filter_params *p, int B) {
    if (!p || B < 1 || p->rows < 1 || p->cols < 1 || (long long)p->rows * p->cols > INT_MAX - THREADS) return 0;
    return road_ws_bytes((size_t)p->rows * p->cols, B);
}

int bugseg_road_filter(bugseg_ctx *ctx, const uint8_t *seg_dev, int B, const bugseg_road_filter_params *p, uint8_t *out_dev,
                       void *workspace_dev, size_t workspace_bytes, void *stream) {
    return road_filter(ctx, seg_dev, B, p, out_dev, workspace_dev, workspace_bytes, 0, N_OPS, stream);
}

int bugseg_debug_road_filter_ops(bugseg_ctx *ctx, const uint8_t *seg_dev, int B, const bugseg_road_filter_params *p,
                                 uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, int first_op, int last_op,
                                 void *stream) {
    return road_filter(ctx, seg_dev, B, p, out_dev, workspace_dev, workspace_bytes, first_op, last_op, stream);
}

}
