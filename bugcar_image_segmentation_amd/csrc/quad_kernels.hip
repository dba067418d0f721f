// find_quad: the calibration tile in a camera frame, batched: grey value and histogram, Otsu's threshold, labelling
// of the foreground (8-connected, ccl_common.h), the largest region off the border, its four corners, and the
// moments of its boundary cracks along each side. Semantics: DESIGN.md §6.22. Everything but Otsu's float64
// variances is integer, every sum is of integers and every arg-max goes through a key that is unique per pixel:
// the result does not depend on the order atomics land in.
//
// The host entry points (bugseg_find_quad, bugseg_quad_moments, bugseg_debug_quad_stage) live here beside the
// kernels, as hough_kernels.hip's do.
//
// Launches of bugseg_find_quad, B frames each (nothing is read back by the host):
//    0 grey      (after one memset of the per-frame histograms and state) u8 grey image into the workspace, 256-bin
//                histogram: per-wave LDS bins, one global atomic per non-zero bin and workgroup
//    1 otsu      one workgroup per frame: the threshold, or the given one
//    2 tile      ccl_common.h's labelling of a 16 x 64 tile in LDS; clears the per-root counters of its pixels
//    3 merge     ccl_common.h's unions across tile borders
//    4 flatten   label[p] = root(p) for foreground pixels; area and border mark per root
//    5 choose    the largest admissible root: one packed 64-bit atomicMax per candidate root
//    6..9 c0..c3 one corner each: a packed 64-bit atomicMax per wave that holds a candidate
//   10 order     one thread per frame: status, cyclic order, the outputs, the doubled corners for launch 11
//   11 moments   (after one memset of the moments) the crack points of the region, six int64 sums per side
// bugseg_quad_moments runs 0 .. 5 and 11, with the corners the caller gives.
//
// Visibility across workgroups: the rule in ccl_common.h, which the merge launch follows. The flatten launch
// reads labels that other workgroups overwrite with their roots: a stale read is an older, still valid,
// ancestor. Every other word a launch reads was written by an earlier launch; the words several workgroups of a
// launch write (bins, counters, keys, sums) are only ever touched with atomics there.
//
// Limits (refused before anything is launched, BUGSEG_EINVAL): rows, cols 3 .. 4096 (a squared distance, a cross
// product and a pixel index each fit 32 bits of a key); channels 1 or 3; B 1 .. 65535 (the launch grid);
// min_area at least 1; band 0 .. 64.
//
// Workspace, per frame: the grey image (1 byte per pixel), labels and counters (4 bytes per pixel each), the
// histogram, the state.
#include <hip/hip_runtime.h>

#include <climits>

#include "bugseg_internal.h"
#include "ccl_common.h"
#include "../../include/bugseg.h"

namespace {

using namespace bugseg;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
static_assert(THREADS == 256, "launch 0 ends with one histogram bin per thread");
constexpr int GREY_PER_THREAD = 16;       // pixels a thread of launch 0 converts: fewer workgroups per histogram word
constexpr int MAX_SIDE = 4096, MIN_SIDE = 3, MAX_BAND = 64;
constexpr int MAX_COORD2 = 4 * MAX_SIDE;  // doubled corner coordinates beyond +-this: the side takes no point
constexpr unsigned BORDER = 0x80000000u;  // counter bit: the region has a pixel in the outermost rows or columns
constexpr int N_OPS = 12, OP_MOMENTS = 11, OP_REGION_END = 6;

struct FrameState {
    unsigned long long key[5];            // the chosen root, then c0 .. c3: value << 32 | (2^32 - 1 - pixel); 0: none
    int tcut;                             // foreground: grey > tcut (bright) or grey <= tcut
    int tout;                             // the threshold reported: tcut, or -1 for a frame of one grey level
    int c2[8];                            // launch 10 -> 11: the corners, doubled
};

struct QuadArgs {
    const uint8_t *img;                   // (B, rows, cols, channels)
    uint8_t *grey;                        // workspace, per frame: npad bytes
    int *label;                           // workspace, per frame: n words
    unsigned *cnt;                        // workspace, per frame: n words. At a root: area | BORDER
    int *hist;                            // workspace, per frame: 256 words
    FrameState *state;                    // workspace, per frame
    const int *corners2;                  // launch 11: (B, 4, 2) doubled corners
    int *status, *threshold, *area, *root, *corners;
    unsigned long long *moments;          // (B, 4, 6)
    int B, rows, cols, channels, bright, fixed, min_area, band;
    int n;                                // rows * cols
    size_t npad;
};

__device__ __forceinline__ bool is_fg(int g, int tcut, int bright) { return bright ? g > tcut : g <= tcut; }
__device__ __forceinline__ unsigned key_pixel(unsigned long long k) { return 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull); }
__device__ __forceinline__ unsigned long long make_key(unsigned v, int p) { return (unsigned long long)v << 32 | (0xFFFFFFFFu - (unsigned)p); }

// ---------------------------------------------------------------- 0: grey value and histogram
__global__ __launch_bounds__(THREADS) void quad_grey_kernel(QuadArgs a) {
    __shared__ int bins[WAVES * 256];
    const int tid = threadIdx.x;
    const size_t f = blockIdx.y;
    for (int i = tid; i < WAVES * 256; i += THREADS) bins[i] = 0;
    __syncthreads();
    int *mine = bins + (tid >> 6) * 256;
    const uint8_t *src = a.img + f * (size_t)a.n * a.channels;
    uint8_t *dst = a.grey + f * a.npad;
    const int base = blockIdx.x * (THREADS * GREY_PER_THREAD);
    for (int i = 0; i < GREY_PER_THREAD; ++i) {
        const int p = base + i * THREADS + tid;
        if (p >= a.n) break;
        int g;
        if (a.channels == 3) {
            const uint8_t *s = src + (size_t)p * 3;
            g = (1868 * s[0] + 9617 * s[1] + 4899 * s[2] + 8192) >> 14;      // bev_warp_image_kernel<3, true>
        } else {
            g = src[p];
        }
        dst[p] = (uint8_t)g;
        atomicAdd(mine + g, 1);
    }
    __syncthreads();
    int s = 0;
    for (int w = 0; w < WAVES; ++w) s += bins[w * 256 + tid];        // THREADS == 256: a bin per thread
    if (s) atomicAdd(a.hist + f * 256 + tid, s);
}

// ---------------------------------------------------------------- 1: threshold
// v(t) in float64, each operation rounded on its own (no product feeds an add here, and contraction is off).
__device__ __forceinline__ double otsu_v(long long n0, unsigned long long s0, long long n1, unsigned long long s1) {
#pragma clang fp contract(off)
    const double d = (double)s0 / (double)n0 - (double)s1 / (double)n1;
    return (double)n0 * (double)n1 * d * d;
}

__global__ __launch_bounds__(256) void quad_otsu_kernel(QuadArgs a) {
    __shared__ int h[256];
    __shared__ double v[256];
    __shared__ uint8_t ok[256];
    const int t = threadIdx.x;
    const size_t f = blockIdx.x;
    FrameState *st = a.state + f;
    if (a.fixed >= 0) {
        if (t == 0) { st->tcut = a.fixed; st->tout = a.fixed; }
        return;
    }
    h[t] = a.hist[f * 256 + t];
    __syncthreads();
    long long n0 = 0, n1 = 0;
    unsigned long long s0 = 0, s1 = 0;
    for (int i = 0; i < 256; ++i) {
        const long long c = h[i];
        if (i <= t) { n0 += c; s0 += (unsigned long long)(c * i); }
        else { n1 += c; s1 += (unsigned long long)(c * i); }
    }
    const bool valid = n0 > 0 && n1 > 0;
    ok[t] = valid;
    v[t] = valid ? otsu_v(n0, s0, n1, s1) : 0.0;
    __syncthreads();
    if (t == 0) {
        int best = -1;
        double bv = 0.0;
        for (int i = 0; i < 256; ++i)
            if (ok[i] && (best < 0 || v[i] > bv)) { best = i; bv = v[i]; }
        // one grey level: no foreground under either polarity
        st->tcut = best >= 0 ? best : (a.bright ? 255 : -1);
        st->tout = best;
    }
}

// ---------------------------------------------------------------- 2, 3: labelling (ccl_common.h)
struct QuadPixels {
    static constexpr bool HAS_BG = false, HAS_NONE = true;
    const uint8_t *grey;
    int *label;
    unsigned *cnt;
    int W, H, tcut, bright;
    __device__ QuadPixels(const QuadArgs &a, size_t f)
        : grey(a.grey + f * a.npad), label(a.label + f * a.n), cnt(a.cnt + f * a.n), W(a.cols), H(a.rows),
          tcut(a.state[f].tcut), bright(a.bright) {}
    __device__ uint8_t kind(int p) const { return is_fg(grey[p], tcut, bright) ? 1 : 2; }
    __device__ void store(int p, int root) const {
        label[p] = root;
        cnt[p] = 0;
    }
};

__global__ __launch_bounds__(THREADS) void quad_tile_kernel(QuadArgs a) {
    label_tile<THREADS>(QuadPixels(a, blockIdx.z), blockIdx.x * LT_TW, blockIdx.y * LT_TH);
}

__global__ __launch_bounds__(THREADS) void quad_merge_kernel(QuadArgs a) {
    const int W = a.cols;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const int y = p / W, x = p - y * W;
    const int ty = y % LT_TH, tx = x % LT_TW;
    if (ty != 0 && tx != 0 && tx != LT_TW - 1) return;
    const QuadPixels px(a, blockIdx.y);
    link_border(px, px.label, x, y, tx, ty);
}

// ---------------------------------------------------------------- 4: flatten, area, border mark
// One atomic per distinct key among the wave's active lanes (road_kernels.hip's wave_count). Every lane calls it.
__device__ inline void wave_count(unsigned *base, int key, bool active) {
    unsigned long long todo = __ballot(active);
    const int lane = __lane_id();
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int kk = __shfl(key, leader);
        const unsigned long long same = __ballot(active && key == kk);
        if (lane == leader) atomicAdd(base + kk, (unsigned)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(THREADS) void quad_flatten_kernel(QuadArgs a) {
    const int W = a.cols, H = a.rows;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    const size_t f = blockIdx.y;
    const QuadPixels px(a, f);
    bool fg = false, edge = false;
    int r = 0;
    if (p < a.n && px.kind(p) == 1) {
        fg = true;
        int x = p;
        for (;;) {
            const int q = px.label[x];
            if (q == x) break;
            x = q;
        }
        if (x != p) px.label[p] = x;
        r = x;
        const int y = p / W, xx = p - y * W;
        edge = y == 0 || xx == 0 || y == H - 1 || xx == W - 1;
    }
    wave_count(px.cnt, r, fg);
    if (edge) atomicOr(px.cnt + r, BORDER);       // (an add below bit 31 and this or commute: areas stay below 2^25)
}

// ---------------------------------------------------------------- 5: the tile's region
__global__ __launch_bounds__(THREADS) void quad_choose_kernel(QuadArgs a) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= a.n) return;
    const size_t f = blockIdx.y;
    const QuadPixels px(a, f);
    if (px.kind(p) != 1 || px.label[p] != p) return;
    const unsigned c = px.cnt[p];
    if ((c & BORDER) || c < (unsigned)a.min_area) return;
    atomicMax(&a.state[f].key[0], make_key(c, p));
}

// ---------------------------------------------------------------- 6 .. 9: corners
__device__ __forceinline__ long long cross2(int ax, int ay, int bx, int by) { return (long long)ax * by - (long long)ay * bx; }

// S = 0: c0, farthest from the root. 1: c1, farthest from c0. 2: c2, largest |cross(c1 - c0, p - c0)|.
// 3: c3, largest outward value over the triangle's three edges, candidates only where it is positive.
template <int S>
__global__ __launch_bounds__(THREADS) void quad_corner_kernel(QuadArgs a) {
    const size_t f = blockIdx.y;
    FrameState *st = a.state + f;
    const unsigned long long best = st->key[0];
    if (best == 0) return;                          // (the whole workgroup)
    if (S > 0 && st->key[S] == 0) return;
    const int W = a.cols;
    const int root = (int)key_pixel(best);
    const int p = blockIdx.x * THREADS + threadIdx.x;
    const QuadPixels px(a, f);
    unsigned long long key = 0;
    if (p < a.n && px.kind(p) == 1 && px.label[p] == root) {
        const int y = p / W, x = p - y * W;
        int q[3][2];
        q[0][0] = root % W; q[0][1] = root / W;
#pragma unroll
        for (int i = 0; i < S && i < 3; ++i) {
            const int c = (int)key_pixel(st->key[i + 1]);
            q[i][0] = c % W; q[i][1] = c / W;
        }
        if constexpr (S < 2) {
            const int dx = x - q[0][0], dy = y - q[0][1];
            key = make_key((unsigned)(dx * dx + dy * dy), p);
        } else if constexpr (S == 2) {
            const long long c = cross2(q[1][0] - q[0][0], q[1][1] - q[0][1], x - q[0][0], y - q[0][1]);
            key = make_key((unsigned)(c < 0 ? -c : c), p);
        } else {
            const long long s = cross2(q[1][0] - q[0][0], q[1][1] - q[0][1], q[2][0] - q[0][0], q[2][1] - q[0][1]);
            long long m = 0;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int *u = q[e], *w = q[(e + 1) % 3];
                long long c = cross2(w[0] - u[0], w[1] - u[1], x - u[0], y - u[1]);
                c = s > 0 ? -c : c;                 // positive: outside the triangle
                m = c > m ? c : m;
            }
            if (s != 0 && m > 0) key = make_key((unsigned)m, p);
        }
    }
    // the wave's largest key, one atomic
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if (__lane_id() == 0 && key) atomicMax(&st->key[S + 1], key);
}

// ---------------------------------------------------------------- 10: status, order, outputs
__global__ __launch_bounds__(64) void quad_order_kernel(QuadArgs a) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= a.B) return;
    FrameState *st = a.state + f;
    const int W = a.cols;
    int status = BUGSEG_QUAD_OK, area = 0, root = -1;
    int c[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, o[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    if (st->key[0] == 0) {
        status = BUGSEG_QUAD_NO_TILE;
    } else {
        area = (int)(st->key[0] >> 32);
        root = (int)key_pixel(st->key[0]);
        if (st->key[4] == 0) {
            status = BUGSEG_QUAD_DEGENERATE;
        } else {
            for (int i = 0; i < 4; ++i) {
                const int p = (int)key_pixel(st->key[i + 1]);
                c[i][0] = p % W; c[i][1] = p / W;
            }
            for (int i = 0; i < 4; ++i)
                for (int j = i + 1; j < 4; ++j)
                    if (c[i][0] == c[j][0] && c[i][1] == c[j][1]) status = BUGSEG_QUAD_DEGENERATE;
        }
    }
    if (status == BUGSEG_QUAD_OK) {
        // the edge of (c0, c1, c2) that c3 lies farthest outside of, the lowest on a tie
        const long long s = cross2(c[1][0] - c[0][0], c[1][1] - c[0][1], c[2][0] - c[0][0], c[2][1] - c[0][1]);
        int edge = 0;
        long long m = 0;
        for (int e = 0; e < 3; ++e) {
            const int *u = c[e], *w = c[(e + 1) % 3];
            long long v = cross2(w[0] - u[0], w[1] - u[1], c[3][0] - u[0], c[3][1] - u[1]);
            v = s > 0 ? -v : v;
            if (v > m) { m = v; edge = e; }
        }
        int k = 0;
        for (int i = 0; i < 3; ++i) {
            o[k][0] = c[i][0]; o[k][1] = c[i][1]; ++k;
            if (i == edge) { o[k][0] = c[3][0]; o[k][1] = c[3][1]; ++k; }
        }
    }
    a.status[f] = status;
    a.threshold[f] = st->tout;
    a.area[f] = area;
    a.root[f] = root;
    for (int i = 0; i < 4; ++i) {
        a.corners[f * 8 + 2 * i] = o[i][0];
        a.corners[f * 8 + 2 * i + 1] = o[i][1];
        st->c2[2 * i] = 2 * o[i][0];
        st->c2[2 * i + 1] = 2 * o[i][1];
    }
}

// ---------------------------------------------------------------- 11: side moments over the region's cracks
// corners2 == nullptr: the corners launch 10 left in the state.
__global__ __launch_bounds__(THREADS) void quad_moments_kernel(QuadArgs a) {
    __shared__ unsigned long long sums[24];
    const size_t f = blockIdx.y;
    const FrameState *st = a.state + f;
    const unsigned long long best = st->key[0];
    if (best == 0) return;                          // (the whole workgroup)
    const int tid = threadIdx.x;
    if (tid < 24) sums[tid] = 0;
    __syncthreads();
    const int W = a.cols, H = a.rows;
    const int root = (int)key_pixel(best);
    const int *cc = a.corners2 ? a.corners2 + f * 8 : st->c2;
    const int p = blockIdx.x * THREADS + tid;
    const QuadPixels px(a, f);
    // this pixel's crack points (at most four), doubled coordinates
    int np = 0, X[4], Y[4];
    if (p < a.n && px.kind(p) == 1 && px.label[p] == root) {
        const int y = p / W, x = p - y * W;
        const int dx[4] = {0, -1, 1, 0}, dy[4] = {-1, 0, 0, 1};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int nx = x + dx[d], ny = y + dy[d];
            bool in = nx >= 0 && nx < W && ny >= 0 && ny < H;
            if (in) {
                const int q = ny * W + nx;
                in = px.kind(q) == 1 && px.label[q] == root;
            }
            if (!in) { X[np] = 2 * x + dx[d]; Y[np] = 2 * y + dy[d]; ++np; }
        }
    }
    const bool idle = __ballot(np != 0) == 0;       // (the whole wave: most waves hold no boundary pixel)
    const long long band2 = (long long)(2 * a.band) * (2 * a.band);
    for (int s = 0; s < 4 && !idle; ++s) {
        const int ax = cc[2 * s], ay = cc[2 * s + 1], bx = cc[2 * ((s + 1) & 3)], by = cc[2 * ((s + 1) & 3) + 1];
        const bool usable = ax >= -MAX_COORD2 && ax <= MAX_COORD2 && ay >= -MAX_COORD2 && ay <= MAX_COORD2 &&
                            bx >= -MAX_COORD2 && bx <= MAX_COORD2 && by >= -MAX_COORD2 && by <= MAX_COORD2 &&
                            (ax != bx || ay != by);
        if (!usable) continue;                      // (the same for every lane)
        const long long ux = bx - ax, uy = by - ay, len2 = ux * ux + uy * uy;
        long long m[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < np; ++i) {
            const long long vx = X[i] - ax, vy = Y[i] - ay;
            const long long cr = ux * vy - uy * vx, dt = 8 * (ux * vx + uy * vy);
            if (cr * cr <= band2 * len2 && len2 <= dt && dt <= 7 * len2) {
                const long long xx = X[i], yy = Y[i];
                m[0] += 1; m[1] += xx; m[2] += yy; m[3] += xx * xx; m[4] += xx * yy; m[5] += yy * yy;
            }
        }
        if (__ballot(m[0] != 0) == 0) continue;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            long long v = m[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (__lane_id() == 0 && v) atomicAdd(&sums[s * 6 + k], (unsigned long long)v);
        }
    }
    __syncthreads();
    if (tid < 24 && sums[tid]) atomicAdd(a.moments + f * 24 + tid, sums[tid]);
}

// ---------------------------------------------------------------- host
size_t state_bytes(int B) { return pad256((size_t)B * sizeof(FrameState)); }
size_t hist_bytes(int B) { return pad256((size_t)B * 256 * sizeof(int)); }
size_t quad_ws_bytes(size_t n, int B) { return state_bytes(B) + hist_bytes(B) + (size_t)B * (pad256(n) + 8 * n) + 256; }

const char *quad_check(const bugseg_quad_params *p, int B) {
    if (B < 1 || B > 65535) return "find_quad: B must be 1 to 65535";
    if (p->rows < MIN_SIDE || p->cols < MIN_SIDE || p->rows > MAX_SIDE || p->cols > MAX_SIDE) return "find_quad: rows and cols must be 3 to 4096";
    if (p->channels != 1 && p->channels != 3) return "find_quad: channels must be 1 or 3";
    if (p->min_area < 1) return "find_quad: min_area must be at least 1";
    if (p->band[0] < 0 || p->band[0] > MAX_BAND || p->band[1] < 0 || p->band[1] > MAX_BAND) return "find_quad: band must be 0 to 64";
    return nullptr;
}

struct Outputs { int *status, *threshold, *area, *root, *corners; int64_t *moments; };

// first .. last: the launches to enqueue; corners2: given corners for launch 11 (nullptr: launch 10's)
int quad_run(bugseg_ctx *ctx, const uint8_t *img, int B, const bugseg_quad_params *p, int band, const int *corners2,
             const Outputs &o, bool find, void *ws, size_t ws_bytes, int first, int last, void *stream) {
    if (!ctx || !img || !p || !o.moments) return ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: NULL argument");
    if (find && (!o.status || !o.threshold || !o.area || !o.root || !o.corners)) return ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: NULL argument");
    if (!find && !corners2) return ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: NULL argument");
    if (const char *why = quad_check(p, B)) return ctx_fail(ctx, BUGSEG_EINVAL, why);
    if (band < 0 || band > MAX_BAND) return ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: band must be 0 to 64");
    const size_t n = (size_t)p->rows * p->cols;
    if (!ws || ws_bytes < quad_ws_bytes(n, B))
        return ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: workspace missing or smaller than bugseg_quad_workspace_bytes()");
    if (((uintptr_t)o.moments & 7)) return ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: moments_dev is not 8-byte aligned");
    struct Range { const void *p; size_t n; bool written; };
    const Range r[] = {{img, n * p->channels * B, false},
                       {corners2, (size_t)B * 8 * sizeof(int), false},
                       {o.status, (size_t)B * sizeof(int), true},
                       {o.threshold, (size_t)B * sizeof(int), true},
                       {o.area, (size_t)B * sizeof(int), true},
                       {o.root, (size_t)B * sizeof(int), true},
                       {o.corners, (size_t)B * 8 * sizeof(int), true},
                       {o.moments, (size_t)B * 24 * sizeof(int64_t), true},
                       {ws, ws_bytes, true}};
    for (size_t i = 0; i < sizeof(r) / sizeof(r[0]); ++i)
        for (size_t j = i + 1; j < sizeof(r) / sizeof(r[0]); ++j)
            if (r[i].p && r[j].p && (r[i].written || r[j].written) && ranges_overlap(r[i].p, r[i].n, r[j].p, r[j].n))
                return ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: a buffer that is written overlaps another buffer");
    DeviceGuard g(ctx_device(ctx));
    QuadArgs a = {};
    a.img = img; a.corners2 = corners2;
    a.status = o.status; a.threshold = o.threshold; a.area = o.area; a.root = o.root; a.corners = o.corners;
    a.moments = (unsigned long long *)o.moments;
    a.B = B; a.rows = p->rows; a.cols = p->cols; a.channels = p->channels; a.bright = p->bright ? 1 : 0;
    a.fixed = (p->threshold >= 0 && p->threshold <= 254) ? p->threshold : -1;
    a.min_area = p->min_area; a.band = band;
    a.n = (int)n; a.npad = pad256(n);
    unsigned char *w = align256(ws);
    a.state = (FrameState *)w;
    a.hist = (int *)(w + state_bytes(B));
    a.grey = w + state_bytes(B) + hist_bytes(B);
    a.label = (int *)(a.grey + (size_t)B * a.npad);
    a.cnt = (unsigned *)(a.label + (size_t)B * n);
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(THREADS);
    const dim3 px((unsigned)((n + THREADS - 1) / THREADS), (unsigned)B);
    const dim3 gpx((unsigned)((n + THREADS * GREY_PER_THREAD - 1) / (THREADS * GREY_PER_THREAD)), (unsigned)B);
    const dim3 ltiles((p->cols + LT_TW - 1) / LT_TW, (p->rows + LT_TH - 1) / LT_TH, B);
    for (int op = first; op < last; ++op) {
        if (!find && op >= OP_REGION_END && op < OP_MOMENTS) continue;
        switch (op) {
        case 0:
            if (hipMemsetAsync(w, 0, state_bytes(B) + hist_bytes(B), s) != hipSuccess) return launch_fail(ctx, "find_quad");
            hipLaunchKernelGGL(quad_grey_kernel, gpx, blk, 0, s, a);
            break;
        case 1: hipLaunchKernelGGL(quad_otsu_kernel, dim3((unsigned)B), dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL(quad_tile_kernel, ltiles, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL(quad_merge_kernel, px, blk, 0, s, a); break;
        case 4: hipLaunchKernelGGL(quad_flatten_kernel, px, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL(quad_choose_kernel, px, blk, 0, s, a); break;
        case 6: hipLaunchKernelGGL(quad_corner_kernel<0>, px, blk, 0, s, a); break;
        case 7: hipLaunchKernelGGL(quad_corner_kernel<1>, px, blk, 0, s, a); break;
        case 8: hipLaunchKernelGGL(quad_corner_kernel<2>, px, blk, 0, s, a); break;
        case 9: hipLaunchKernelGGL(quad_corner_kernel<3>, px, blk, 0, s, a); break;
        case 10: hipLaunchKernelGGL(quad_order_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, a); break;
        default:
            if (hipMemsetAsync(o.moments, 0, (size_t)B * 24 * sizeof(int64_t), s) != hipSuccess) return launch_fail(ctx, "find_quad");
            hipLaunchKernelGGL(quad_moments_kernel, px, blk, 0, s, a);
            break;
        }
        if (int rc = launch_fail(ctx, "find_quad")) return rc;
    }
    return BUGSEG_OK;
}

}  // namespace

extern "C" {

size_t bugseg_quad_workspace_bytes(const bugseg_quad_params *p, int B) {
    if (!p || quad_check(p, B)) return 0;
    return quad_ws_bytes((size_t)p->rows * p->cols, B);
}

int bugseg_find_quad(bugseg_ctx *ctx, const uint8_t *frames_dev, int B, const bugseg_quad_params *p, int32_t *status_dev,
                     int32_t *threshold_dev, int32_t *area_dev, int32_t *root_dev, int32_t *corners_dev, int64_t *moments_dev,
                     void *workspace_dev, size_t workspace_bytes, void *stream) {
    const Outputs o = {status_dev, threshold_dev, area_dev, root_dev, corners_dev, moments_dev};
    return quad_run(ctx, frames_dev, B, p, p ? p->band[0] : 0, nullptr, o, true, workspace_dev, workspace_bytes, 0, N_OPS, stream);
}

int bugseg_quad_moments(bugseg_ctx *ctx, const uint8_t *frames_dev, int B, const bugseg_quad_params *p, int band,
                        const int32_t *corners2_dev, int64_t *moments_dev, void *workspace_dev, size_t workspace_bytes,
                        void *stream) {
    const Outputs o = {nullptr, nullptr, nullptr, nullptr, nullptr, moments_dev};
    return quad_run(ctx, frames_dev, B, p, band, corners2_dev, o, false, workspace_dev, workspace_bytes, 0, N_OPS, stream);
}

int bugseg_debug_quad_stage(bugseg_ctx *ctx, const uint8_t *frames_dev, int B, const bugseg_quad_params *p, int stage,
                            int32_t *status_dev, int32_t *threshold_dev, int32_t *area_dev, int32_t *root_dev,
                            int32_t *corners_dev, int64_t *moments_dev, void *workspace_dev, size_t workspace_bytes,
                            void *stream) {
    if (stage < 0 || stage >= N_OPS) return bugseg::ctx_fail(ctx, BUGSEG_EINVAL, "find_quad: stage must be 0 to 11");
    const Outputs o = {status_dev, threshold_dev, area_dev, root_dev, corners_dev, moments_dev};
    return quad_run(ctx, frames_dev, B, p, p ? p->band[0] : 0, nullptr, o, true, workspace_dev, workspace_bytes, stage, stage + 1, stream);
}

}
