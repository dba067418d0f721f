// Evaluation of class maps on the device: the confusion matrix of predicted u8 class maps against u8 label maps,
// batched, accumulated into the caller's int64 accumulator. Semantics: DESIGN.md §6.20. Everything is integer and
// every sum is of integers: the result does not depend on the order atomics land in.
//
// The host entry point (bugseg_confusion) lives here beside the kernel, as in canny_kernels.hip: the runtime
// translation units reference nothing of this file; this file uses what bugseg_internal.h and the runtime export.
//
// One launch. acc[g * C + p] += 1 for every label pixel whose mapped label g = gt_lut[gt] and mapped prediction
// p = pred_lut[pred] are both below C; acc[C * C] += 1 for every other label pixel.
//
//   equal shapes   the B frames of both maps are one run of B * rows * cols bytes. Up to 15 bytes bring both
//                  pointers to a 16-byte boundary (they can only when both are equally far from one; else every
//                  pixel goes the byte way), then every lane loads 16 label bytes and 16 prediction bytes with
//                  one dwordx4 each; what is left behind the last whole vector goes the byte way too
//   other shapes   one label pixel per lane and step; the prediction is read at the integer nearest position
//                  sy = min(y * ph / gh, ph - 1), sx = min(x * pw / gw, pw - 1)
//
// Contention (class maps are large uniform regions: a plain atomic per pixel has all 64 lanes on one LDS word):
//   runs       a lane folds its 16 pixels into runs of equal (label, prediction) byte pairs in registers and
//              looks a pair up in the two tables only when a run ends
//   wave       the lanes whose runs end in the same step with the key and length of the first of them are served
//              by one LDS atomic of that lane (road_kernels.hip's wave_count, one round of it); the others add on
//              their own. Inside a uniform region that is one LDS atomic per wave and 1024 pixels. Further rounds,
//              and rounds that sum unequal lengths from ballots, measured slower on noisy maps
//   workgroup  every wave adds into its own copy of the bins where LDS has room (clahe_kernels.hip's
//              sub-histograms): 16 copies (one per wave) while they fit 48 KB, halved until they do (C = 64: 2), so
//              that a workgroup stays under 50 KB and two, a CU's complement of waves, fit its 160 KB
//   device     a workgroup ends with one 64-bit global atomic per non-zero bin. These are what the workgroup
//              size is chosen by: a thousand workgroups adding to one word take as long as the rest of the call,
//              so the workgroups are 1024 threads and at most 512
// A bin is a u32 and a call counts fewer than 2^31 pixels, so no bin of a workgroup can overflow.
#include <hip/hip_runtime.h>

#include <climits>

#include "bugseg_internal.h"
#include "../../include/bugseg.h"

namespace {

constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int VEC = 16;                  // pixels per lane and load
constexpr int MAX_CLASSES = 64;
constexpr int MAX_GROUPS = 512;         // two workgroups of 16 waves per CU: a CU's full complement of waves
constexpr int LDS_TABLE_WORDS = 256;     // two u16[256] tables in front of the bins
constexpr int LDS_BIN_BUDGET = 48 * 1024;
constexpr unsigned BAD = 0x8000u;        // table entry of a byte that maps to no evaluated class

struct EvalArgs {
    const uint8_t *pred, *gt;
    unsigned long long *acc;
    unsigned n_total;                    // B * gh * gw label pixels
    unsigned head, nvec;                 // equal shapes: bytes before the first vector, whole vectors
    unsigned pn, gn;                     // pixels of one prediction frame, of one label frame
    int ph, pw, gh, gw;
    int C, bins, copies;                 // bins = C * C + 1; copies a power of two
    int same;                            // the shapes are equal
    uint8_t pred_lut[256], gt_lut[256];
};

// Called by every lane of a wave in the same step. active lanes add cnt (1..16) to hist[key]; those that hold
// the first active lane's key and count are served by one atomic of that lane.
__device__ __forceinline__ void wave_emit(unsigned *hist, unsigned key, unsigned cnt, bool active) {
    const unsigned long long todo = __ballot(active);
    if (!todo) return;
    const int lane = __lane_id(), leader = __ffsll((long long)todo) - 1;
    const unsigned comb = key << 5 | cnt;
    const bool served = active && comb == (unsigned)__builtin_amdgcn_readlane((int)comb, leader);   // leader is wave-uniform
    const unsigned ns = (unsigned)__popcll(__ballot(served));
    if (lane == leader) atomicAdd(hist + key, cnt * ns);
    else if (active && !served) atomicAdd(hist + key, cnt);
}

// raw = label byte << 8 | prediction byte -> bin
__device__ __forceinline__ unsigned eval_key(const unsigned short *gl, const unsigned short *pl, unsigned raw, unsigned CC) {
    const unsigned g = gl[raw >> 8], p = pl[raw & 255];
    return ((g | p) & BAD) ? CC : g + p;
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // loaded with one dwordx4

__device__ __forceinline__ unsigned eval_raw(const u32x4 &g, const u32x4 &p, int j) {
    const int s = 8 * (j & 3);
    return ((g[j >> 2] >> s) & 255u) << 8 | ((p[j >> 2] >> s) & 255u);
}

// 16 pixels of a lane, as runs. Every lane of the wave calls it; valid: the lane holds pixels.
__device__ __forceinline__ void eval_vec(unsigned *hist, const unsigned short *gl, const unsigned short *pl, unsigned CC,
                                         const u32x4 &g, const u32x4 &p, bool valid) {
    unsigned cur = eval_raw(g, p, 0), cnt = 1;
#pragma unroll
    for (int j = 1; j < VEC; ++j) {
        const unsigned r = eval_raw(g, p, j);
        const bool end = valid && r != cur;
        unsigned key = 0;
        if (end) key = eval_key(gl, pl, cur, CC);
        wave_emit(hist, key, cnt, end);
        cnt = end ? 1 : cnt + 1;
        cur = r;
    }
    unsigned key = 0;
    if (valid) key = eval_key(gl, pl, cur, CC);
    wave_emit(hist, key, cnt, valid);
}

extern __shared__ unsigned eval_lds[];

__global__ __launch_bounds__(THREADS) void eval_confusion_kernel(EvalArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6;
    unsigned short *gl = (unsigned short *)eval_lds, *pl = gl + 256;
    unsigned *bins = eval_lds + LDS_TABLE_WORDS;
    const unsigned C = (unsigned)a.C, CC = C * C;
    if (tid < 256) {
        const unsigned g = a.gt_lut[tid], p = a.pred_lut[tid];
        gl[tid] = (unsigned short)(g < C ? g * C : BAD);
        pl[tid] = (unsigned short)(p < C ? p : BAD);
    }
    const int nwords = a.bins * a.copies;
    for (int i = tid; i < nwords; i += THREADS) bins[i] = 0;
    __syncthreads();
    unsigned *hist = bins + (wave & (a.copies - 1)) * a.bins;
    const unsigned stride = gridDim.x * THREADS;

    if (a.same) {
        const u32x4 *gv = (const u32x4 *)(a.gt + a.head), *pv = (const u32x4 *)(a.pred + a.head);
        // two vectors of each map in flight per lane. A lane past the end loads the last vector again (the
        // loop runs only when there is one) and does not count it
        for (unsigned v0 = blockIdx.x * THREADS; v0 < a.nvec; v0 += 2 * stride) {
            const unsigned va = v0 + tid, vb = va + stride;
            const bool oka = va < a.nvec, okb = vb < a.nvec;
            const unsigned ia = oka ? va : a.nvec - 1, ib = okb ? vb : a.nvec - 1;
            const u32x4 ga = gv[ia], pa = pv[ia], gb = gv[ib], pb = pv[ib];
            eval_vec(hist, gl, pl, CC, ga, pa, oka);
            if (v0 + stride < a.nvec) eval_vec(hist, gl, pl, CC, gb, pb, okb);
        }
        // the bytes in front of the first vector and behind the last
        const unsigned nbytes = a.n_total - a.nvec * VEC;
        for (unsigned k0 = blockIdx.x * THREADS; k0 < nbytes; k0 += stride) {
            const unsigned k = k0 + tid;
            const bool ok = k < nbytes;
            unsigned key = 0;
            if (ok) {
                const unsigned pos = k < a.head ? k : k + a.nvec * VEC;
                key = eval_key(gl, pl, (unsigned)a.gt[pos] << 8 | a.pred[pos], CC);
            }
            wave_emit(hist, key, 1, ok);
        }
    } else {
        for (unsigned k0 = blockIdx.x * THREADS; k0 < a.n_total; k0 += stride) {
            const unsigned k = k0 + tid;
            const bool ok = k < a.n_total;
            unsigned key = 0;
            if (ok) {
                const unsigned f = k / a.gn, r = k - f * a.gn;
                const unsigned y = r / (unsigned)a.gw, x = r - y * (unsigned)a.gw;
                unsigned sy = y * (unsigned)a.ph / (unsigned)a.gh, sx = x * (unsigned)a.pw / (unsigned)a.gw;
                sy = sy < (unsigned)a.ph - 1 ? sy : (unsigned)a.ph - 1;
                sx = sx < (unsigned)a.pw - 1 ? sx : (unsigned)a.pw - 1;
                key = eval_key(gl, pl, (unsigned)a.gt[k] << 8 | a.pred[(size_t)f * a.pn + sy * (unsigned)a.pw + sx], CC);
            }
            wave_emit(hist, key, 1, ok);
        }
    }
    __syncthreads();
    for (int b = tid; b < a.bins; b += THREADS) {
        unsigned long long s = 0;
        for (int c = 0; c < a.copies; ++c) s += bins[c * a.bins + b];
        if (s) atomicAdd(a.acc + b, s);
    }
}

}  // namespace

extern "C" {

int bugseg_confusion(bugseg_ctx *ctx, const uint8_t *pred_dev, const uint8_t *gt_dev, int B, const bugseg_confusion_params *p,
                     int64_t *acc_dev, void *stream) {
    using bugseg::ctx_fail;
    if (!ctx || !pred_dev || !gt_dev || !p || !acc_dev) return ctx_fail(ctx, BUGSEG_EINVAL, "confusion: NULL argument");
    if (B < 1) return ctx_fail(ctx, BUGSEG_EINVAL, "confusion: B must be at least 1");
    if (p->pred_rows < 1 || p->pred_cols < 1 || p->gt_rows < 1 || p->gt_cols < 1)
        return ctx_fail(ctx, BUGSEG_EINVAL, "confusion: bad shape");
    if (p->num_classes < 1 || p->num_classes > MAX_CLASSES)
        return ctx_fail(ctx, BUGSEG_EINVAL, "confusion: num_classes must be 1..64");
    // every index is a 32-bit one, with room for one more step of the whole grid behind the last pixel
    const long long lim = (long long)INT_MAX - 2LL * MAX_GROUPS * THREADS;
    const long long gn = (long long)p->gt_rows * p->gt_cols, pn = (long long)p->pred_rows * p->pred_cols;
    if (gn > lim || pn > lim || gn * B > lim || pn * B > lim)
        return ctx_fail(ctx, BUGSEG_EINVAL, "confusion: B * rows * cols too large for an int32 index");
    const bool same = p->pred_rows == p->gt_rows && p->pred_cols == p->gt_cols;
    if (!same && ((long long)p->gt_rows * p->pred_rows > lim || (long long)p->gt_cols * p->pred_cols > lim))
        return ctx_fail(ctx, BUGSEG_EINVAL, "confusion: label rows * prediction rows (or cols * cols) too large for an int32 index");
    if ((uintptr_t)acc_dev & 7) return ctx_fail(ctx, BUGSEG_EINVAL, "confusion: acc_dev is not 8-byte aligned");
    bugseg::DeviceGuard g(bugseg::ctx_device(ctx));
    EvalArgs a;
    a.pred = pred_dev; a.gt = gt_dev; a.acc = (unsigned long long *)acc_dev;
    a.n_total = (unsigned)(gn * B);
    a.pn = (unsigned)pn; a.gn = (unsigned)gn;
    a.ph = p->pred_rows; a.pw = p->pred_cols; a.gh = p->gt_rows; a.gw = p->gt_cols;
    a.C = p->num_classes;
    a.bins = a.C * a.C + 1;
    a.copies = WAVES;
    while (a.copies > 1 && (size_t)a.copies * a.bins * 4 > (size_t)LDS_BIN_BUDGET) a.copies >>= 1;
    a.same = same ? 1 : 0;
    a.head = 0; a.nvec = 0;
    unsigned steps = a.n_total;          // lane steps of the longer of the launch's loops
    if (same) {
        const unsigned mg = (unsigned)((uintptr_t)gt_dev & 15), mp = (unsigned)((uintptr_t)pred_dev & 15);
        if (mg == mp) {
            a.head = (16 - mg) & 15;
            if (a.head > a.n_total) a.head = a.n_total;
            a.nvec = (a.n_total - a.head) / VEC;
            steps = (a.nvec + 1) / 2;
            if (steps < a.n_total - a.nvec * VEC) steps = a.n_total - a.nvec * VEC;
        }
    }
    for (int i = 0; i < 256; ++i) { a.pred_lut[i] = p->pred_lut[i]; a.gt_lut[i] = p->gt_lut[i]; }
    unsigned groups = (steps + THREADS - 1) / THREADS;
    groups = groups < 1 ? 1 : groups > (unsigned)MAX_GROUPS ? (unsigned)MAX_GROUPS : groups;
    const size_t lds = (size_t)(LDS_TABLE_WORDS + a.copies * a.bins) * 4;
    hipLaunchKernelGGL(eval_confusion_kernel, dim3(groups), dim3(THREADS), lds, (hipStream_t)stream, a);
    return bugseg::launch_fail(ctx, "confusion");
}

}
