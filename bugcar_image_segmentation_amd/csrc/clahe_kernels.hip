// clahe (image_processing_utils.py:46-61) on the device, batched: BGR -> Lab, CLAHE on L, Lab -> BGR, in two
// launches over (B, rows, cols, 3) u8 frames. Semantics: DESIGN.md §6.18, restated in tests/clahe_ref.py.
//
//   1 luts    one workgroup per (frame, tile): the tile's BGR pixels (reflected indices serve the padding),
//             L only, a 256-bin histogram in LDS (one sub-histogram per wave), clip, redistribute, scan,
//             256 LUT bytes to the workspace (B, tiles_y, tiles_x, 256)
//   2 apply   per pixel: BGR -> Lab, L through the four neighbouring LUTs (float32, every operation rounded on
//             its own), Lab -> BGR. No Lab image ever reaches HBM.
//
// The stage functions (clahe_bgr_to_lab, clahe_tile_lut, clahe_blend, clahe_lab_to_bgr) are __device__
// functions that the two launches and the debug launches (bugseg_debug_clahe_stage) share. Everything is
// integer but the blend, whose float32 expressions use __fmul_rn / __fadd_rn (this file is also compiled with
// -ffp-contract=off, build.py): a contracted multiply-add would round once where the semantics round twice.
//
// The conversion tables (ClaheTables, 34 KB) are built once per process on the host and uploaded once per
// context (bugseg::ctx_clahe_tables). The per-pixel launch stages them in LDS; the luts launch, which needs
// only the gamma and cube-root tables, gathers from them through the cache.
// The host entry points live here beside the kernels, as road_kernels.hip's do.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "bugseg_internal.h"
#include "../../include/bugseg.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int PX = 4;                       // pixels per thread of the per-pixel launches (12 bytes: 3 dwords)
constexpr int GAMMA_SHIFT = 3, LAB_SHIFT = 12, LAB_SHIFT2 = 15;
constexpr int CBRT_N = 256 * 3 / 2 * (1 << GAMMA_SHIFT);
constexpr int F_BITS = 16, F_STEP_BITS = 6, F_BIAS = 1 << 15, F_N = 2306;
constexpr int V_BITS = 20, C_BITS = 16, G_BITS = 14;
constexpr int IG_N = (1 << G_BITS) + 1;
constexpr int MAX_TILES = 16;

struct ClaheTables {
    uint16_t gamma[256];        // round(255 * 8 * srgb_to_linear(i / 255))
    uint16_t cbrt[CBRT_N];      // round(32768 * f(i / 2040))
    int32_t lab_c[9];           // sRGB -> XYZ rows / white point, Q12
    int32_t fy[256];            // (L * 100 / 255 + 16) / 116, Q16
    int32_t y[256];             // Y of L, Q20
    int32_t f[F_N];             // finv(k / 1024 - 0.5), Q20
    int32_t rgb_c[9];           // XYZ -> sRGB columns * white point, Q16
    uint8_t inv_gamma[IG_N];    // round(255 * linear_to_srgb(i / 16384))
};

static_assert(sizeof(ClaheTables) % 4 == 0, "the tables are copied to LDS as dwords");

struct ClaheArgs {
    const uint8_t *in;          // (B, rows, cols, 3)
    uint8_t *out;               // (B, rows, cols, 3), or the LUTs for the luts launch
    uint8_t *luts;              // (B, tiles_y, tiles_x, 256)
    const ClaheTables *t;
    int B, rows, cols, tiles_x, tiles_y;
    int tile_w, tile_h;         // of the extended image
    int clip;                   // max(int(clip_limit * tile_area / 256), 1)
    float lut_scale;            // float32(255 / tile_area)
    float inv_tw, inv_th;       // 1.0f / tile_w, 1.0f / tile_h
    int n;                      // rows * cols
    int total;                  // B * n
    int mode;                   // per-pixel launches: 0 the product, 1 BGR -> Lab only, 2 Lab -> BGR only
    int dwords;                 // both frame buffers are 4-byte aligned: 12-byte groups move as 3 dwords
};

__device__ __forceinline__ int sat_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---------------------------------------------------------------- stage A
__device__ __forceinline__ int clahe_cbrt_of(const ClaheTables *t, int r, int g, int b, int row) {
    const int *c = t->lab_c + 3 * row;
    return t->cbrt[(r * c[0] + g * c[1] + b * c[2] + (1 << (LAB_SHIFT - 1))) >> LAB_SHIFT];
}

__device__ __forceinline__ int clahe_l_of_fy(int fy) {
    return sat_u8((296 * fy - ((16 * 255 * (1 << LAB_SHIFT2) + 50) / 100) + (1 << (LAB_SHIFT2 - 1))) >> LAB_SHIFT2);
}

// L alone (the luts launch needs nothing else)
__device__ __forceinline__ int clahe_bgr_to_l(const ClaheTables *t, int b, int g, int r) {
    return clahe_l_of_fy(clahe_cbrt_of(t, t->gamma[r], t->gamma[g], t->gamma[b], 1));
}

__device__ __forceinline__ void clahe_bgr_to_lab(const ClaheTables *t, int b, int g, int r, int &L, int &A, int &Bb) {
    const int R = t->gamma[r], G = t->gamma[g], Bl = t->gamma[b];
    const int fx = clahe_cbrt_of(t, R, G, Bl, 0), fy = clahe_cbrt_of(t, R, G, Bl, 1), fz = clahe_cbrt_of(t, R, G, Bl, 2);
    L = clahe_l_of_fy(fy);
    A = sat_u8((500 * (fx - fy) + 128 * (1 << LAB_SHIFT2) + (1 << (LAB_SHIFT2 - 1))) >> LAB_SHIFT2);
    Bb = sat_u8((200 * (fy - fz) + 128 * (1 << LAB_SHIFT2) + (1 << (LAB_SHIFT2 - 1))) >> LAB_SHIFT2);
}

// ---------------------------------------------------------------- stage C
// round(v * 2^16 / den), halves up, for v in [-128, 127]: the numerator is shifted positive by a multiple of
// 2 * den first, so the division truncates like a floor
__device__ __forceinline__ int clahe_q16(int v, int den) {
    const int k = 128 * (2 << F_BITS) / (2 * den) + 1;
    return (v * (2 << F_BITS) + den + k * 2 * den) / (2 * den) - k;
}

__device__ __forceinline__ int clahe_finv(const ClaheTables *t, int fq) {
    const int u = fq + F_BIAS;
    const int k = u >> F_STEP_BITS, fr = u & ((1 << F_STEP_BITS) - 1);
    const int t0 = t->f[k], t1 = t->f[k + 1];
    return t0 + (((t1 - t0) * fr + (1 << (F_STEP_BITS - 1))) >> F_STEP_BITS);
}

__device__ __forceinline__ void clahe_lab_to_bgr(const ClaheTables *t, int L, int A, int Bb, int &b, int &g, int &r) {
    const int fy = t->fy[L];
    const long long x = clahe_finv(t, fy + clahe_q16(A - 128, 500));
    const long long y = t->y[L];
    const long long z = clahe_finv(t, fy - clahe_q16(Bb - 128, 200));
    constexpr int SH = V_BITS + C_BITS - G_BITS;
    int o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int *c = t->rgb_c + 3 * ch;
        long long i = (c[0] * x + c[1] * y + c[2] * z + (1ll << (SH - 1))) >> SH;
        i = i < 0 ? 0 : (i > (1 << G_BITS) ? (1 << G_BITS) : i);
        o[ch] = t->inv_gamma[(int)i];
    }
    r = o[0]; g = o[1]; b = o[2];
}

// ---------------------------------------------------------------- stage B: the blend
__device__ __forceinline__ void clahe_axis(int c, float inv, int tiles, int &i1, int &i2, float &w1, float &w2) {
    const float tf = __fadd_rn(__fmul_rn((float)c, inv), -0.5f);
    const float t1 = floorf(tf);
    w2 = __fsub_rn(tf, t1);
    w1 = __fsub_rn(1.0f, w2);
    const int i = (int)t1;
    i1 = i < 0 ? 0 : i;
    i2 = i + 1 > tiles - 1 ? tiles - 1 : i + 1;
}

__device__ __forceinline__ int clahe_blend(const uint8_t *luts, int tiles_x, int tiles_y, float inv_tw, float inv_th, int x, int y,
                                  int v) {
    int tx1, tx2, ty1, ty2;
    float xa1, xa, ya1, ya;
    clahe_axis(x, inv_tw, tiles_x, tx1, tx2, xa1, xa);
    clahe_axis(y, inv_th, tiles_y, ty1, ty2, ya1, ya);
    const uint8_t *r1 = luts + (size_t)ty1 * tiles_x * 256 + v, *r2 = luts + (size_t)ty2 * tiles_x * 256 + v;
    const float v00 = r1[tx1 * 256], v01 = r1[tx2 * 256], v10 = r2[tx1 * 256], v11 = r2[tx2 * 256];
    const float top = __fadd_rn(__fmul_rn(v00, xa1), __fmul_rn(v01, xa));
    const float bot = __fadd_rn(__fmul_rn(v10, xa1), __fmul_rn(v11, xa));
    const float res = __fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya));
    return sat_u8((int)rintf(res));
}

// ---------------------------------------------------------------- stage B: one tile's LUT
// Called by all THREADS threads of a workgroup; thread i owns bin i. hist: WAVES sub-histograms of 256 bins,
// zeroed here, filled by the threads' atomics (a frame of one grey level lands on WAVES addresses, not one);
// red: 2 * WAVES words of scratch.
__device__ __forceinline__ void clahe_tile_lut(const ClaheArgs &a, int frame, int tile_x, int tile_y, unsigned *hist, int *red,
                                      uint8_t *dst) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) hist[w * 256 + tid] = 0;
    __syncthreads();
    const uint8_t *img = a.in + (size_t)frame * a.n * 3;
    const int area = a.tile_w * a.tile_h;
    const int x0 = tile_x * a.tile_w, y0 = tile_y * a.tile_h;
    for (int p = tid; p < area; p += THREADS) {
        const int ty = p / a.tile_w, tx = p - ty * a.tile_w;
        int y = y0 + ty, x = x0 + tx;
        if (y >= a.rows) y = 2 * (a.rows - 1) - y;          // BORDER_REFLECT_101; the pad is at most tiles <= side / 2
        if (x >= a.cols) x = 2 * (a.cols - 1) - x;
        const uint8_t *px = img + ((size_t)y * a.cols + x) * 3;
        atomicAdd(&hist[wave * 256 + clahe_bgr_to_l(a.t, px[0], px[1], px[2])], 1u);
    }
    __syncthreads();
    int h = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) h += (int)hist[w * 256 + tid];
    const int clipped = h < a.clip ? h : a.clip;
    // the excess of the whole tile
    int e = h - clipped;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) e += __shfl_xor(e, d, 64);
    if (lane == 0) red[wave] = e;
    __syncthreads();
    int excess = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) excess += red[w];
    int v = clipped + (excess >> 8);
    const int rest = excess & 255;
    if (rest > 0) {
        const int s = 256 / rest;                           // >= 1: rest <= 255
        if (tid % s == 0 && tid / s < rest) ++v;
    }
    // inclusive running sum over the 256 bins
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) red[WAVES + wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += red[WAVES + w];
    dst[tid] = (uint8_t)sat_u8((int)rintf(__fmul_rn((float)v, a.lut_scale)));
}

// ---------------------------------------------------------------- launch 1
__global__ __launch_bounds__(THREADS) void clahe_luts_kernel(ClaheArgs a) {
    __shared__ unsigned hist[WAVES * 256];
    __shared__ int red[2 * WAVES];
    const int tile = blockIdx.x, frame = blockIdx.y;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    clahe_tile_lut(a, frame, tx, ty, hist, red, a.luts + ((size_t)frame * a.tiles_x * a.tiles_y + tile) * 256);
}

// ---------------------------------------------------------------- launch 2 (and the per-pixel debug stages)
// One thread = PX consecutive pixels of the batch's flat pixel array, 12 bytes: three dword loads and stores
// when both buffers are 4-byte aligned, bytes otherwise and for the last, partial group.
__device__ __forceinline__ void clahe_group(const ClaheArgs &a, const ClaheTables *t, int g0) {
    const int cnt = a.total - g0 < PX ? a.total - g0 : PX;
    const bool wide = a.dwords && cnt == PX;
    uint8_t px[3 * PX];
    const uint8_t *src = a.in + (size_t)g0 * 3;
    if (wide) {
        const uint32_t *s4 = (const uint32_t *)src;
        uint32_t w[3] = {s4[0], s4[1], s4[2]};
        memcpy(px, w, 12);
    } else {
        for (int i = 0; i < 3 * cnt; ++i) px[i] = src[i];
    }
    int frame = g0 / a.n;
    int p = g0 - frame * a.n;
    int y = p / a.cols, x = p - y * a.cols;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        if (i < cnt) {
            int c0 = px[3 * i], c1 = px[3 * i + 1], c2 = px[3 * i + 2];
            if (a.mode == 1) {
                int L, A, Bb;
                clahe_bgr_to_lab(t, c0, c1, c2, L, A, Bb);
                c0 = L; c1 = A; c2 = Bb;
            } else if (a.mode == 2) {
                int b, g, r;
                clahe_lab_to_bgr(t, c0, c1, c2, b, g, r);
                c0 = b; c1 = g; c2 = r;
            } else {
                int L, A, Bb, b, g, r;
                clahe_bgr_to_lab(t, c0, c1, c2, L, A, Bb);
                L = clahe_blend(a.luts + (size_t)frame * a.tiles_x * a.tiles_y * 256, a.tiles_x, a.tiles_y, a.inv_tw,
                                a.inv_th, x, y, L);
                clahe_lab_to_bgr(t, L, A, Bb, b, g, r);
                c0 = b; c1 = g; c2 = r;
            }
            px[3 * i] = (uint8_t)c0; px[3 * i + 1] = (uint8_t)c1; px[3 * i + 2] = (uint8_t)c2;
            if (++x == a.cols) {
                x = 0;
                if (++y == a.rows) { y = 0; ++frame; }
            }
        }
    }
    uint8_t *dst = a.out + (size_t)g0 * 3;
    if (wide) {
        uint32_t w[3];
        memcpy(w, px, 12);
        uint32_t *d4 = (uint32_t *)dst;
        d4[0] = w[0]; d4[1] = w[1]; d4[2] = w[2];
    } else {
        for (int i = 0; i < 3 * cnt; ++i) dst[i] = px[i];
    }
}

// The conversion tables are staged in LDS once per workgroup (34 KB: four workgroups per CU), and a grid of at
// most LDS_GRID workgroups strides over the pixel groups, so a large batch amortises the staging over ~19 k
// pixels per workgroup. Gathering from the tables through the cache instead measured 2.0x slower at B = 64,
// 480 x 640.
constexpr int LDS_GRID = 1024;      // 256 CUs x the 4 workgroups whose tables fit a CU's LDS

__global__ __launch_bounds__(THREADS) void clahe_pixels_kernel(ClaheArgs a) {
    __shared__ ClaheTables lt;
    {
        const uint32_t *s4 = (const uint32_t *)a.t;
        uint32_t *d4 = (uint32_t *)&lt;
        for (int i = threadIdx.x; i < (int)(sizeof(ClaheTables) / 4); i += THREADS) d4[i] = s4[i];
    }
    __syncthreads();
    const int groups = (a.total + PX - 1) / PX;
    for (int g = blockIdx.x * THREADS + threadIdx.x; g < groups; g += gridDim.x * THREADS) clahe_group(a, &lt, g * PX);
}

// ---------------------------------------------------------------- host: the tables
double srgb_to_linear(double x) { return x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4); }
double linear_to_srgb(double x) { return x <= 0.0031308 ? 12.92 * x : 1.055 * std::pow(x, 1.0 / 2.4) - 0.055; }
double lab_f(double x) { return x < 0.008856 ? 7.787 * x + 16.0 / 116.0 : std::cbrt(x); }
double lab_finv(double f) {
    const double thresh = 7.787 * 0.008856 + 16.0 / 116.0;
    return f <= thresh ? (f - 16.0 / 116.0) / 7.787 : f * f * f;
}

const ClaheTables &host_tables() {
    static const ClaheTables tabs = [] {
        ClaheTables t;
        std::memset(&t, 0, sizeof(t));
        static const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
        static const double MI[3][3] = {{3.240479, -1.53715, -0.498535}, {-0.969256, 1.875991, 0.041556}, {0.055648, -0.204043, 1.057311}};
        static const double white[3] = {0.950456, 1.0, 1.088754};
        for (int i = 0; i < 256; ++i)
            t.gamma[i] = (uint16_t)std::nearbyint(255.0 * (1 << GAMMA_SHIFT) * srgb_to_linear(i / 255.0));
        for (int i = 0; i < CBRT_N; ++i)
            t.cbrt[i] = (uint16_t)std::nearbyint((1 << LAB_SHIFT2) * lab_f(i / (255.0 * (1 << GAMMA_SHIFT))));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                t.lab_c[3 * r + c] = (int32_t)std::nearbyint(M[r][c] / white[r] * (double)(1 << LAB_SHIFT));
                t.rgb_c[3 * r + c] = (int32_t)std::nearbyint(MI[r][c] * white[c] * (double)(1 << C_BITS));
            }
        for (int L = 0; L < 256; ++L) {
            t.fy[L] = (int32_t)(((100ll * L + 4080) * (2ll << F_BITS) + 29580) / (2 * 29580));
            const double li = L * 100.0 / 255.0, fy = (li + 16.0) / 116.0;
            t.y[L] = (int32_t)std::nearbyint((li <= 8.0 ? li / 903.3 : fy * fy * fy) * (double)(1 << V_BITS));
        }
        for (int k = 0; k < F_N; ++k) t.f[k] = (int32_t)std::nearbyint(lab_finv(k / 1024.0 - 0.5) * (double)(1 << V_BITS));
        for (int i = 0; i < IG_N; ++i)
            t.inv_gamma[i] = (uint8_t)std::nearbyint(255.0 * linear_to_srgb(i / (double)(1 << G_BITS)));
        return t;
    }();
    return tabs;
}

// ---------------------------------------------------------------- host: the call
// The shape checks every entry shares; nullptr when the parameters are usable.
const char *bad_shape(const bugseg_clahe_params *p, int B) {
    if (B < 1) return "clahe: B must be at least 1";
    if (B > 65535) return "clahe: B above 65535";
    if (p->tiles_x < 1 || p->tiles_x > MAX_TILES || p->tiles_y < 1 || p->tiles_y > MAX_TILES)
        return "clahe: tiles must be in [1, 16]";
    if (p->rows < 2 * p->tiles_y || p->cols < 2 * p->tiles_x) return "clahe: a side is smaller than twice its tile count";
    if (!(p->clip_limit > 0.f) || !std::isfinite(p->clip_limit)) return "clahe: clip_limit must be positive and finite";
    // (every byte of the batch, and one more block of pixel groups, is indexed with an int)
    if ((long long)B * p->rows * p->cols * 3 > (long long)INT_MAX - 3 * PX * THREADS)
        return "clahe: B * rows * cols * 3 too large for an int32 index";
    return nullptr;
}

size_t lut_bytes(const bugseg_clahe_params *p, int B) { return (size_t)B * p->tiles_x * p->tiles_y * 256; }

enum { STAGE_LAB = 0, STAGE_LUTS = 1, STAGE_BGR = 2, STAGE_LAUNCH1 = 3, STAGE_LAUNCH2 = 4, STAGE_ALL = 5 };

int clahe_run(bugseg_ctx *ctx, const uint8_t *in, int B, const bugseg_clahe_params *p, int stage, uint8_t *out, void *ws,
              size_t ws_bytes, void *stream) {
    using bugseg::ctx_fail;
    using bugseg::ranges_overlap;
    if (!ctx || !p) return ctx_fail(ctx, BUGSEG_EINVAL, "clahe: NULL argument");
    if (stage < 0 || stage > STAGE_ALL) return ctx_fail(ctx, BUGSEG_EINVAL, "clahe: stage must be in [0, 4]");
    const bool writes_out = stage != STAGE_LAUNCH1;
    if (!in || (writes_out && !out)) return ctx_fail(ctx, BUGSEG_EINVAL, "clahe: NULL argument");
    if (const char *why = bad_shape(p, B)) return ctx_fail(ctx, BUGSEG_EINVAL, why);
    const bool uses_ws = stage == STAGE_LAUNCH1 || stage == STAGE_LAUNCH2 || stage == STAGE_ALL;
    const size_t frames = (size_t)B * p->rows * p->cols * 3, nlut = lut_bytes(p, B);
    if (uses_ws && (!ws || ws_bytes < nlut))
        return ctx_fail(ctx, BUGSEG_EINVAL, "clahe: workspace missing or smaller than bugseg_clahe_workspace_bytes()");
    if (writes_out && ranges_overlap(in, frames, out, stage == STAGE_LUTS ? nlut : frames))
        return ctx_fail(ctx, BUGSEG_EINVAL, "clahe: out_dev overlaps the input");
    if (uses_ws && (ranges_overlap(ws, nlut, in, frames) || (writes_out && ranges_overlap(ws, nlut, out, frames))))
        return ctx_fail(ctx, BUGSEG_EINVAL, "clahe: the workspace overlaps a frame buffer");
    const void *tabs = nullptr;
    if (int rc = bugseg::ctx_clahe_tables(ctx, &host_tables(), sizeof(ClaheTables), stream, &tabs)) return rc;
    bugseg::DeviceGuard g(bugseg::ctx_device(ctx));
    ClaheArgs a;
    a.in = in; a.out = out; a.t = (const ClaheTables *)tabs;
    a.luts = stage == STAGE_LUTS ? out : (uint8_t *)ws;
    a.B = B; a.rows = p->rows; a.cols = p->cols; a.tiles_x = p->tiles_x; a.tiles_y = p->tiles_y;
    int pr = p->rows, pc = p->cols;
    if (p->cols % p->tiles_x != 0 || p->rows % p->tiles_y != 0) {
        pr += p->tiles_y - p->rows % p->tiles_y;
        pc += p->tiles_x - p->cols % p->tiles_x;
    }
    a.tile_w = pc / p->tiles_x; a.tile_h = pr / p->tiles_y;
    const int area = a.tile_w * a.tile_h;
    // (a clip of the tile's area clips nothing: capping there keeps the conversion to int defined)
    const double c = (double)p->clip_limit * area / 256.0;
    a.clip = c >= (double)area ? area : (int)c;
    if (a.clip < 1) a.clip = 1;
    a.lut_scale = (float)(255.0 / area);
    a.inv_tw = 1.0f / (float)a.tile_w; a.inv_th = 1.0f / (float)a.tile_h;
    a.n = p->rows * p->cols; a.total = B * a.n;
    a.mode = stage == STAGE_LAB ? 1 : (stage == STAGE_BGR ? 2 : 0);
    a.dwords = ((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(THREADS);
    const dim3 tiles((unsigned)(p->tiles_x * p->tiles_y), (unsigned)B);
    dim3 px((unsigned)((a.total + PX * THREADS - 1) / (PX * THREADS)));
    if (px.x > LDS_GRID) px.x = LDS_GRID;
    const bool l1 = stage == STAGE_LUTS || stage == STAGE_LAUNCH1 || stage == STAGE_ALL;
    const bool l2 = stage != STAGE_LUTS && stage != STAGE_LAUNCH1;
    for (int launch = 0; launch < 2; ++launch) {
        if (launch == 0 && l1) hipLaunchKernelGGL(clahe_luts_kernel, tiles, blk, 0, s, a);
        else if (launch == 1 && l2) hipLaunchKernelGGL(clahe_pixels_kernel, px, blk, 0, s, a);
        else continue;
        if (int rc = bugseg::launch_fail(ctx, "clahe")) return rc;
    }
    return BUGSEG_OK;
}

}  // namespace

extern "C" {

size_t bugseg_clahe_workspace_bytes(const bugseg_clahe_params *p, int B) {
    if (!p || bad_shape(p, B)) return 0;
    return lut_bytes(p, B);
}

int bugseg_clahe_bgr(bugseg_ctx *ctx, const uint8_t *bgr_dev, int B, const bugseg_clahe_params *p, uint8_t *out_dev,
                     void *workspace_dev, size_t workspace_bytes, void *stream) {
    return clahe_run(ctx, bgr_dev, B, p, STAGE_ALL, out_dev, workspace_dev, workspace_bytes, stream);
}

int bugseg_debug_clahe_stage(bugseg_ctx *ctx, const uint8_t *in_dev, int B, const bugseg_clahe_params *p, int stage,
                             uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (stage == STAGE_ALL) stage = -1;
    return clahe_run(ctx, in_dev, B, p, stage, out_dev, workspace_dev, workspace_bytes, stream);
}

int bugseg_debug_clahe_table(int which, void *dst, size_t bytes) {
    const ClaheTables &t = host_tables();
    const void *src[8] = {t.gamma, t.cbrt, t.lab_c, t.fy, t.y, t.f, t.rgb_c, t.inv_gamma};
    const size_t len[8] = {sizeof(t.gamma), sizeof(t.cbrt), sizeof(t.lab_c), sizeof(t.fy), sizeof(t.y), sizeof(t.f),
                           sizeof(t.rgb_c), sizeof(t.inv_gamma)};
    if (which < 0 || which >= 8 || !dst || bytes != len[which])
        return bugseg::ctx_fail(nullptr, BUGSEG_EINVAL, "clahe table: `which` must be in [0, 8) and `bytes` the table's size");
    std::memcpy(dst, src[which], bytes);
    return BUGSEG_OK;
}

}
