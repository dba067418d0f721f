// The standard Hough transform (cv2.HoughLines) on the device, batched: edge pixels vote for (angle, rho) cells,
// local maxima above a threshold are the lines, the strongest max_lines of them are returned in order.
// Semantics: DESIGN.md §6.21. Votes are integer adds and the keys that order the peaks are unique, so the result
// does not depend on the order atomics land in. The only floating-point arithmetic is float32 multiply and add,
// each rounded on its own: this file is built with -ffp-contract=off (build.py), and the sine and cosine come
// from a table the host makes (bugseg_hough_trig): the device evaluates no transcendental.
//
// The host entry points (bugseg_hough*) live here beside the kernels, as canny_kernels.hip's do.
//
// Launches of one call, B frames each (after one memset of the per-frame counters):
//   0 compact  the non-zero pixels of a frame as words x | y << 16, appended to the frame's list: one ballot and
//              one atomic add per wave. The list's order is free
//   1 vote     one workgroup per (frame, run of T angles). T + 2 accumulator rows of numrho + 2 int32 in LDS: the
//              angles before and after the run are voted too, so that the run's rows see their true neighbours.
//              The workgroup walks the frame's list (LDS atomic adds), then tests its T rows for peaks and
//              appends a key votes << 32 | (2^32 - 1 - index) per peak, again one atomic per wave. The
//              accumulator never reaches memory
//   2 select   one workgroup per frame: if the frame has more than max_lines keys, a radix select (8 passes of 8
//              bits, from the top) finds the max_lines-th largest key exactly; the keys at or above it (at most
//              4096) are sorted in LDS (bitonic, descending), decoded and written with counts and peaks
//
// No two cells that share a side can both be peaks (of two equal neighbours only the left, or the upper, passes;
// of two unequal ones only the larger), so a frame has at most ceil(numangle * numrho / 2) keys. Its key list has
// that many places: there is no overflow.
//
// T: the most rows for which T + 2 of them fit 80 KiB, so that two workgroups share a CU's 160 KiB of LDS (at
// 480 x 640 and rho 1 a row is 8972 bytes, T = 7: 9 rows, 80,748 bytes); where not even 3 rows fit 80 KiB, the most
// that fit 160 KiB, one workgroup per CU. At 1080 x 1920 and rho 1 a row is 24,012 bytes and T = 1: 3 rows, 72,036
// bytes, still two workgroups per CU. T is at most 30.
//
// Limits (refused before anything is launched, BUGSEG_EINVAL):
//   rows, cols   1 .. 65535 each (the packed word), B * rows * cols below 2^31 - 256
//   numrho       must be the value §6.21 defines for rows, cols and rho (votes are indexed with it), and at most
//                13651: three rows of numrho + 2 int32 must fit 160 KiB
//   numangle     1 .. 65536, and (numangle + 2) * (numrho + 2) below 2^31 (the index in a key)
//   max_lines    1 .. 4096 (the LDS sort)
//   B            1 .. 65535 (the launch grid)
//
// Workspace, per frame: the pixel list (4 bytes per pixel), the key list (8 bytes per possible key), two counters.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "bugseg_internal.h"
#include "../../include/bugseg.h"

namespace {

using namespace bugseg;

constexpr int CT = 256;       // compact: threads
constexpr int VT = 512;       // vote: threads
constexpr int ST = 1024;      // select: threads
constexpr int MAX_T = 30;
constexpr int MAX_LINES = 4096;
constexpr int MAX_NUMRHO = 13651, MAX_NUMANGLE = 65536, MAX_SIDE = 65535;
constexpr size_t LDS_SHARED = 80 * 1024, LDS_ALL = 160 * 1024;

struct HoughArgs {
    const uint8_t *img;             // (B, rows, cols)
    const int *acc_in;              // stage 1: (B, numangle + 2, numrho + 2), read in place of the votes
    int *acc_out;                   // stage 0: the same shape, written in place of the peak test
    const float *trig;              // numangle cosines / rho, then numangle sines / rho
    float *lines;                   // (B, max_lines, 2)
    int *counts, *peaks;            // (B,)
    unsigned *counters;             // workspace, per frame: listed pixels, keys
    unsigned *pix;                  // workspace, per frame: pix_stride words
    unsigned long long *keys;       // workspace, per frame: key_stride keys
    size_t pix_stride, key_stride;
    int B, rows, cols, n;           // n = rows * cols
    int numangle, numrho, threshold, max_lines, T;
    float rho, theta, min_theta;
};

// the place of the calling lane among the lanes of mask m, and the wave's first lane of m
__device__ inline unsigned rank_in(unsigned long long m) { return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// One place per lane of mask m (the same in every lane of the wave, all of them active) in a list whose length
// `count` holds: one atomic add per wave -> the calling lane's place (meaningful in the lanes of m).
__device__ inline unsigned append_places(unsigned *count, unsigned long long m) {
    unsigned base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(count, (unsigned)__popcll(m));
    return (unsigned)__shfl((int)base, 0) + rank_in(m);
}

// ---------------------------------------------------------------- 0: the non-zero pixels
__global__ __launch_bounds__(CT) void hough_compact_kernel(HoughArgs a) {
    const int p = blockIdx.x * CT + threadIdx.x;
    const size_t f = blockIdx.y;
    const bool set = p < a.n && a.img[f * a.n + p] != 0;
    const unsigned long long m = __ballot(set);
    if (m == 0) return;                             // (the whole wave)
    const unsigned at = append_places(a.counters + 2 * f, m);
    if (set) {
        const int y = p / a.cols, x = p - y * a.cols;
        a.pix[f * a.pix_stride + at] = (unsigned)x | (unsigned)y << 16;      // at < the frame's non-zero pixels <= n
    }
}

// ---------------------------------------------------------------- 1: votes and peaks
// MODE 0: the product. 1 (stage 0): the votes, then the run's rows to acc_out. 2 (stage 1): the rows from acc_in
// in place of the votes, then the peaks.
template <int MODE>
__global__ __launch_bounds__(VT) void hough_vote_kernel(HoughArgs a) {
    extern __shared__ int acc[];                    // (T + 2) x (numrho + 2): row t is angle n0 - 1 + t (all the LDS it has)
    const int W = a.numrho + 2, T = a.T;
    const int n0 = blockIdx.x * T;
    const int nt = min(T, a.numangle - n0);         // this run's angles
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const size_t frame_cells = (size_t)(a.numangle + 2) * W;
    if (MODE == 2) {
        // rows n0 .. n0 + nt + 1 of the given accumulator (whose row n + 1 is angle n)
        const int *src = a.acc_in + f * frame_cells + (size_t)n0 * W;
        for (int i = tid; i < (T + 2) * W; i += VT) acc[i] = i < (nt + 2) * W ? src[i] : 0;
        __syncthreads();
    } else {
        for (int i = tid; i < (T + 2) * W; i += VT) acc[i] = 0;
        __syncthreads();
        const unsigned cnt = a.counters[2 * f];
        const unsigned *pix = a.pix + f * a.pix_stride;
        const int half = (a.numrho - 1) / 2;
        // the rows whose angle exists: the others stay zero, as the accumulator's border
        const int t_lo = n0 == 0 ? 1 : 0, t_hi = min(T + 2, a.numangle - n0 + 1);
        const float *tc = a.trig + (n0 - 1), *ts = a.trig + a.numangle + (n0 - 1);       // read for t_lo <= t < t_hi only
        for (unsigned k = tid; k < cnt; k += VT) {
            const unsigned w = pix[k];
            const float x = (float)(w & 0xffffu), y = (float)(w >> 16);
            for (int t = t_lo; t < t_hi; ++t) {
#pragma clang fp contract(off)
                const float xc = x * tc[t], ys = y * ts[t];
                const float s = xc + ys;
                const int r = (int)__builtin_rintf(s) + half;       // cvRound: half to even
                if ((unsigned)r < (unsigned)a.numrho) atomicAdd(&acc[t * W + r + 1], 1);
            }
        }
        __syncthreads();
    }
    if (MODE == 1) {
        int *dst = a.acc_out + f * frame_cells + (size_t)(n0 + 1) * W;
        for (int i = tid; i < nt * W; i += VT) dst[i] = acc[W + i];
        return;
    }
    const int total = nt * a.numrho;
    unsigned long long *keys = a.keys + f * a.key_stride;
    for (int base = 0; base < total; base += VT) {                 // (the same trip count in every lane)
        const int i = base + tid;
        bool pk = false;
        unsigned v = 0, idx = 0;
        if (i < total) {
            const int t = i / a.numrho, r = i - t * a.numrho;
            const int *c = acc + (t + 1) * W + r + 1;
            const int av = *c;
            pk = av > a.threshold && av > c[-1] && av >= c[1] && av > c[-W] && av >= c[W];
            v = (unsigned)av;
            idx = (unsigned)((n0 + t + 1) * W + r + 1);
        }
        const unsigned long long m = __ballot(pk);
        if (m == 0) continue;
        const unsigned at = append_places(a.counters + 2 * f + 1, m);
        if (pk) keys[at] = (unsigned long long)v << 32 | (0xFFFFFFFFu - idx);   // at < ceil(numangle numrho / 2)
    }
}

// ---------------------------------------------------------------- 2: the max_lines largest keys, in order
__global__ __launch_bounds__(ST) void hough_select_kernel(HoughArgs a) {
    __shared__ unsigned long long sk[MAX_LINES];
    __shared__ unsigned hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_need, s_cnt;
    const size_t f = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned K = a.counters[2 * f + 1];
    const unsigned long long *keys = a.keys + f * a.key_stride;
    const unsigned want = min(K, (unsigned)a.max_lines);
    unsigned long long cut = 0;                     // the want-th largest key (0: every key)
    if (K > (unsigned)a.max_lines) {
        unsigned long long prefix = 0;
        unsigned need = (unsigned)a.max_lines;      // of the keys that begin with `prefix`, the need-th largest
        for (int p = 7; p >= 0; --p) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const int sh = 8 * p;
            for (unsigned base = 0; base < K; base += ST) {
                const unsigned k = base + tid;
                bool in = false;
                unsigned d = 0;
                if (k < K) {
                    const unsigned long long key = keys[k];
                    in = (p == 7 ? 0ull : key >> (sh + 8)) == prefix;
                    d = (unsigned)(key >> sh) & 255u;
                }
                const unsigned long long m = __ballot(in);
                if (m == 0) continue;
                // a wave whose keys all share the digit (the upper bytes of small vote counts) adds once
                const int first = __ffsll((long long)m) - 1;
                const unsigned d0 = (unsigned)__shfl((int)d, first);
                if (__ballot(in && d == d0) == m) {
                    if (lane == first) atomicAdd(&hist[d0], (unsigned)__popcll(m));
                } else if (in) {
                    atomicAdd(&hist[d], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {
                unsigned c = 0;
                int d = 255;
                for (; d > 0; --d) {
                    if (c + hist[d] >= need) break;
                    c += hist[d];
                }
                s_prefix = prefix << 8 | (unsigned)d;
                s_need = need - c;
            }
            __syncthreads();
            prefix = s_prefix;
            need = s_need;
        }
        cut = prefix;
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (unsigned base = 0; base < K; base += ST) {
        const unsigned k = base + tid;
        unsigned long long key = 0;
        if (k < K) key = keys[k];
        const bool keep = k < K && key >= cut;
        const unsigned long long m = __ballot(keep);
        if (m == 0) continue;
        const unsigned at = append_places(&s_cnt, m);
        if (keep && at < (unsigned)MAX_LINES) sk[at] = key;         // (keys are unique: exactly `want` are kept)
    }
    unsigned P = 1;
    while (P < want) P <<= 1;
    __syncthreads();
    for (unsigned i = want + tid; i < P; i += ST) sk[i] = 0;        // below every key
    __syncthreads();
    for (unsigned k = 2; k <= P; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = tid; i < P; i += ST) {
                const unsigned l = i ^ j;
                if (l > i) {
                    const unsigned long long x = sk[i], y = sk[l];
                    if ((i & k) == 0 ? x < y : x > y) { sk[i] = y; sk[l] = x; }
                }
            }
            __syncthreads();
        }
    }
    const unsigned W = (unsigned)a.numrho + 2;
    float *out = a.lines + f * (size_t)a.max_lines * 2;
    for (unsigned i = tid; i < (unsigned)a.max_lines; i += ST) {
        float rho = 0.0f, theta = 0.0f;
        if (i < want) {
#pragma clang fp contract(off)
            const unsigned idx = 0xFFFFFFFFu - (unsigned)(sk[i] & 0xFFFFFFFFull);
            const int n = (int)(idx / W) - 1, r = (int)(idx % W) - 1;
            const float centre = (float)(a.numrho - 1) * 0.5f;
            rho = ((float)r - centre) * a.rho;
            const float step = (float)n * a.theta;
            theta = a.min_theta + step;
        }
        out[2 * i] = rho;
        out[2 * i + 1] = theta;
    }
    if (tid == 0) {
        a.counts[f] = (int)want;
        a.peaks[f] = (int)K;
    }
}

// ---------------------------------------------------------------- host
struct Plan {
    int T;
    size_t lds, pix_stride, key_stride, counters_bytes, bytes;
};

inline long long cv_round(double v) { return (long long)std::nearbyint(v); }     // (the default rounding mode: to even)

// nullptr and the plan, or why the parameters are refused
const char *hough_plan(const bugseg_hough_params *p, int B, Plan &pl) {
    if (B < 1 || B > 65535) return "hough: B must be 1 to 65535";
    if (p->rows < 1 || p->cols < 1 || p->rows > MAX_SIDE || p->cols > MAX_SIDE) return "hough: rows and cols must be 1 to 65535";
    if ((long long)B * p->rows * (long long)p->cols > (long long)INT_MAX - CT) return "hough: B * rows * cols too large for an int32 index";
    if (!(p->rho > 0.0f) || !std::isfinite(p->rho) || !(p->theta > 0.0f) || !std::isfinite(p->theta) || !std::isfinite(p->min_theta))
        return "hough: rho and theta must be positive and finite, min_theta finite";
    if (p->max_lines < 1 || p->max_lines > MAX_LINES) return "hough: max_lines must be 1 to 4096";
    if (p->numangle < 1 || p->numangle > MAX_NUMANGLE) return "hough: numangle must be 1 to 65536";
    const double want = (2.0 * ((double)p->cols + (double)p->rows) + 1.0) / (double)p->rho;
    if (!(want < 1e9) || p->numrho < 1 || (long long)p->numrho != cv_round(want))
        return "hough: numrho is not cvRound((2 (cols + rows) + 1) / rho), or below 1";
    if (p->numrho > MAX_NUMRHO) return "hough: numrho above 13651: three accumulator rows do not fit the LDS";
    if (((long long)p->numangle + 2) * (p->numrho + 2) >= (1LL << 31)) return "hough: (numangle + 2) * (numrho + 2) must be below 2^31";
    const size_t row = (size_t)(p->numrho + 2) * sizeof(int);
    long long t = (long long)(LDS_SHARED / row) - 2;
    if (t < 1) t = (long long)(LDS_ALL / row) - 2;
    if (t < 1) return "hough: numrho above 13651: three accumulator rows do not fit the LDS";
    pl.T = (int)std::min<long long>(std::min<long long>(t, MAX_T), p->numangle);
    pl.lds = (size_t)(pl.T + 2) * row;
    const size_t n = (size_t)p->rows * p->cols;
    const size_t maxkeys = ((size_t)p->numangle * p->numrho + 1) / 2;
    pl.pix_stride = pad256(n * 4) / 4;
    pl.key_stride = pad256(maxkeys * 8) / 8;
    pl.counters_bytes = pad256((size_t)B * 2 * sizeof(unsigned));
    pl.bytes = pl.counters_bytes + (size_t)B * (pl.pix_stride * 4 + pl.key_stride * 8) + 256;
    return nullptr;
}

// stage -1: the whole call; 0: compact and vote, the accumulators into acc; 1: peaks and select on the accumulators in acc
int hough(bugseg_ctx *ctx, const uint8_t *img, int B, const bugseg_hough_params *p, const float *trig, int stage, int *acc,
          float *lines, int *counts, int *peaks, void *ws, size_t ws_bytes, void *stream) {
    if (!ctx || !p) return ctx_fail(ctx, BUGSEG_EINVAL, "hough: NULL argument");
    const bool votes = stage != 1, selects = stage != 0;
    if ((votes && (!img || !trig)) || (selects && (!lines || !counts || !peaks)) || (stage >= 0 && !acc))
        return ctx_fail(ctx, BUGSEG_EINVAL, "hough: NULL argument");
    Plan pl;
    if (const char *why = hough_plan(p, B, pl)) return ctx_fail(ctx, BUGSEG_EINVAL, why);
    if (!ws || ws_bytes < pl.bytes)
        return ctx_fail(ctx, BUGSEG_EINVAL, "hough: workspace missing or smaller than bugseg_hough_workspace_bytes()");
    const size_t n = (size_t)p->rows * p->cols;
    const size_t acc_bytes = (size_t)B * (p->numangle + 2) * (p->numrho + 2) * sizeof(int);
    struct Range { const void *p; size_t n; bool written; };
    const Range r[] = {{votes ? img : nullptr, n * B, false},
                       {votes ? trig : nullptr, (size_t)2 * p->numangle * sizeof(float), false},
                       {stage >= 0 ? acc : nullptr, acc_bytes, stage == 0},
                       {selects ? lines : nullptr, (size_t)B * p->max_lines * 2 * sizeof(float), true},
                       {selects ? counts : nullptr, (size_t)B * sizeof(int), true},
                       {selects ? peaks : nullptr, (size_t)B * sizeof(int), true},
                       {ws, ws_bytes, true}};
    for (size_t i = 0; i < sizeof(r) / sizeof(r[0]); ++i)
        for (size_t j = i + 1; j < sizeof(r) / sizeof(r[0]); ++j)
            if (r[i].p && r[j].p && (r[i].written || r[j].written) && ranges_overlap(r[i].p, r[i].n, r[j].p, r[j].n))
                return ctx_fail(ctx, BUGSEG_EINVAL, "hough: a buffer that is written overlaps another buffer");
    DeviceGuard g(ctx_device(ctx));
    HoughArgs a = {};
    a.img = img; a.acc_in = acc; a.acc_out = acc; a.trig = trig;
    a.lines = lines; a.counts = counts; a.peaks = peaks;
    unsigned char *w = align256(ws);
    a.counters = (unsigned *)w;
    a.pix = (unsigned *)(w + pl.counters_bytes);
    a.keys = (unsigned long long *)(w + pl.counters_bytes + (size_t)B * pl.pix_stride * 4);
    a.pix_stride = pl.pix_stride; a.key_stride = pl.key_stride;
    a.B = B; a.rows = p->rows; a.cols = p->cols; a.n = (int)n;
    a.numangle = p->numangle; a.numrho = p->numrho; a.threshold = p->threshold; a.max_lines = p->max_lines; a.T = pl.T;
    a.rho = p->rho; a.theta = p->theta; a.min_theta = p->min_theta;
    hipStream_t s = (hipStream_t)stream;
    const void *vote = stage < 0 ? (const void *)hough_vote_kernel<0> : stage == 0 ? (const void *)hough_vote_kernel<1>
                                                                                  : (const void *)hough_vote_kernel<2>;
    if (allow_dynamic_lds(vote) != hipSuccess) return ctx_fail(ctx, BUGSEG_EHIP, "hough: the vote kernel cannot have its LDS");
    if (hipMemsetAsync(a.counters, 0, (size_t)B * 2 * sizeof(unsigned), s) != hipSuccess) return launch_fail(ctx, "hough");
    if (stage == 0 && hipMemsetAsync(acc, 0, acc_bytes, s) != hipSuccess) return launch_fail(ctx, "hough");
    const dim3 runs((unsigned)((p->numangle + pl.T - 1) / pl.T), (unsigned)B);
    if (votes) {
        hipLaunchKernelGGL(hough_compact_kernel, dim3((unsigned)((n + CT - 1) / CT), (unsigned)B), dim3(CT), 0, s, a);
        if (int rc = launch_fail(ctx, "hough")) return rc;
    }
    if (stage < 0) hipLaunchKernelGGL(hough_vote_kernel<0>, runs, dim3(VT), pl.lds, s, a);
    else if (stage == 0) hipLaunchKernelGGL(hough_vote_kernel<1>, runs, dim3(VT), pl.lds, s, a);
    else hipLaunchKernelGGL(hough_vote_kernel<2>, runs, dim3(VT), pl.lds, s, a);
    if (int rc = launch_fail(ctx, "hough")) return rc;
    if (selects) {
        hipLaunchKernelGGL(hough_select_kernel, dim3((unsigned)B), dim3(ST), 0, s, a);
        if (int rc = launch_fail(ctx, "hough")) return rc;
    }
    return BUGSEG_OK;
}

}  // namespace

extern "C" {

int bugseg_hough_trig(const bugseg_hough_params *p, float *dst_host) {
    if (!p || !dst_host || p->numangle < 1 || p->numangle > MAX_NUMANGLE || !(p->rho > 0.0f) || !std::isfinite(p->rho) ||
        !std::isfinite(p->theta) || !std::isfinite(p->min_theta))
        return bugseg::ctx_fail(nullptr, BUGSEG_EINVAL, "hough trig: bad parameters");
    const float irho = 1.0f / p->rho;
    float ang = p->min_theta;
    for (int n = 0; n < p->numangle; ++n) {
        dst_host[n] = (float)(std::cos((double)ang) * (double)irho);
        dst_host[p->numangle + n] = (float)(std::sin((double)ang) * (double)irho);
        ang += p->theta;
    }
    return BUGSEG_OK;
}

size_t bugseg_hough_workspace_bytes(const bugseg_hough_params *p, int B) {
    Plan pl;
    if (!p || hough_plan(p, B, pl)) return 0;
    return pl.bytes;
}

int bugseg_hough_lines(bugseg_ctx *ctx, const uint8_t *img_dev, int B, const bugseg_hough_params *p, const float *trig_dev,
                       float *lines_dev, int32_t *counts_dev, int32_t *peaks_dev, void *workspace_dev, size_t workspace_bytes,
                       void *stream) {
    return hough(ctx, img_dev, B, p, trig_dev, -1, nullptr, lines_dev, counts_dev, peaks_dev, workspace_dev, workspace_bytes, stream);
}

int bugseg_debug_hough_stage(bugseg_ctx *ctx, const uint8_t *img_dev, int B, const bugseg_hough_params *p, const float *trig_dev,
                             int stage, int32_t *acc_dev, float *lines_dev, int32_t *counts_dev, int32_t *peaks_dev,
                             void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (stage != 0 && stage != 1) return bugseg::ctx_fail(ctx, BUGSEG_EINVAL, "hough: stage must be 0 or 1");
    return hough(ctx, img_dev, B, p, trig_dev, stage, acc_dev, lines_dev, counts_dev, peaks_dev, workspace_dev, workspace_bytes, stream);
}

}
