// Two consecutive fp32 (parity mode) C = 64 regular bottlenecks in ONE launch.
//
// ENet's blocks 1.1 -> 1.2, 1.3 -> 1.4 and 4.1 -> 4.2 are consecutive regular bottlenecks of one shape (3x3,
// d = 1, 64 -> 16 -> 16 -> 64). Run one launch each (bneck_kernels.hip), the first block's output y goes to HBM
// and is read straight back by the second and by nobody else: half of the bytes the two launches move. Here one
// workgroup owns a TH x 16 tile of the SECOND block's output and computes, per tile,
//   A1  t0_A = act1(W1a x + b1a)                          over tile +- 2 (0 outside the image)   -> LDS
//   A2  t1_A = act2(W2a * t0_A + b2a)                     over tile +- 1                          registers
//   A3  y    = act_out(act3(W3a t1_A + b3a) + x)          over tile +- 1, as f32                  -> LDS
//   B1  t0_B = act1(W1b y + b1b)                          over tile +- 1 (0 outside the image)   -> LDS (over t0_A)
//   B2  t1_B = act2(W2b * t0_B + b2b)                     over the tile                           registers
//   B3  out  = act_out(act3(W3b t1_B + b3b) + y)          over the tile, whole-line stores        -> HBM
// with bneck_kernel's products in bneck_kernel's order: the split-f16 MFMAs of mfma_common.h, the HL weight
// layout, t0 as hi / lo planes (bneck_kernels.hip PL), bias-initialised accumulators, PReLU as max(v, s v).
// y in LDS holds the bits the unpaired launch stores to HBM, so out is bit-identical to the two launches'.
// The tile's memory traffic runs beside its compute: A1 leaves the raw x of tile +- 1 in the y region, dead until
// A3, which takes its residual from there (BNECK_PAIR_XLDS), and the next tile's x is loaded into registers while
// A2 .. B3 of this one run (BNECK_PAIR_PREF), so B2 + B3's stores are the only global traffic a tile waits behind.
//
// Range scaling. The unpaired second launch derives its exponents from the MEASURED max |y|, which does not
// exist inside one launch, and no rigorous bound replaces it: the row-sum bound of y is ~800 x its measured
// maximum on the default weights and block B's chain from it leaves the f16 window (scripts/pair_range_check.py).
// So the pair SPECULATES that every exponent of both blocks is 0 — the unscaled instruction stream, the only
// one this kernel has — and the result is checked, not assumed:
//   * block A's exponents follow from the measured max |x| alone (bneck_range); if one is non-zero every
//     workgroup leaves before computing anything;
//   * otherwise y is exactly the unpaired y, and the launch commits max |y| to the range words the unpaired
//     first launch would commit (and max |out| to the second's);
//   * the two unpaired launches follow in their guarded form (bneck_kernels.hip bneck_guard64_kernel): they
//     evaluate both blocks' exponents from the measured max |x| and max |y| and return at once when all are
//     0 — the common case, a few microseconds — else they redo the pair's work with the scaled bodies.
// Either way the result is the unpaired plan's, bit for bit, whatever the tile grid: the decision rests on
// launch-wide maxima only.
#include <algorithm>

#include "bugseg_internal.h"
#include "mfma_common.h"

namespace bugseg {

namespace {
constexpr int PC = 64, PKS1 = 2, PKS2 = 5, PG2 = 18, PNR3 = 4;
constexpr int PK1S = PKS1 * 32 + 8, PK2S = PKS2 * 32 + 8, PK3S = 32 + 8;   // HL weight rows: 8 / 40 dwords mod 64
constexpr int PW1 = 16 * PK1S, PW2 = 16 * PK2S, PW3 = PC * PK3S;            // floats per matrix
constexpr int PWF = PW1 + PW2 + PW3;                                        // one block's weights (one run of 16-B slots)
constexpr int PCST = 4 * 16 + 3 * PC;                                       // cb1 cs1 cb2 cs2 | cb3 cs3 cso
constexpr int PBLK = PWF + PCST;                                            // one block: 26,624 B
constexpr int PZP = 8;                                                      // zero pad (masked-off B fragments)
constexpr int PYS = 68;                                                     // y pixel stride (dwords): 256 B + 16 B pad
static_assert(PYS >= PC && PYS % 4 == 0, "a y pixel is 64 floats, 16-B aligned");
// The residual x of block A over tile +- 1: 1 = A1 leaves the raw x it loaded in the (then dead) y region and A3
// reads it where it writes y; 0 = A3 re-reads it from global memory (L2)
#ifndef BNECK_PAIR_XLDS
#define BNECK_PAIR_XLDS 1
#endif
// The next tile's x in flight during the current tile: the first BNECK_PAIR_PREF fragments of every wave (0 = none,
// 1 = each wave's first, 2 = all) are loaded before A2 + A3, which touch no global memory under XLDS, and held in
// registers across the loop-end barrier; the rest in A1 as before, behind the first fragment's projection. The
// defaults by measurement. These two stay -D switches: the serial tile (both 0) is built as the
// pair_serial variant by tests/test_gpu_bneck_pair_overlap.py
#ifndef BNECK_PAIR_PREF
#define BNECK_PAIR_PREF 1
#endif
// Debug build only (-DBUGSEG_STAMPS, scripts/pair_stamp_probe.py): bneck_kernels.hip's phase clocks, here
// 0 tile top, 1 A1's loads landed, 2 A1 end, 3 A2 + A3 end, 4 B1 end, 5 B2 + B3 end (each behind its barrier)
#ifndef STAMP
#define STAMP(k) do {} while (0)
#define STAMP_WG() do {} while (0)
#endif

// The LDS map (floats): both blocks' weights and constants, the zero pad, y over tile +- 1, then the t0 region:
// t0_A over tile +- 2 as a hi and a lo plane of 8 dwords per pixel, later t0_B over tile +- 1 in the same bytes
template <int TH, int NW>
struct PairForm {
    static constexpr int TW = 16, NT = NW * 64;
    static constexpr int HWA = TW + 4, HRA = (TH + 4) * HWA;   // t0_A: width, pixels
    static constexpr int HWB = TW + 2, HRB = (TH + 2) * HWB;   // y, t0_B
    static constexpr int NFA = (HRA + 15) / 16, NFB = (HRB + 15) / 16;   // 16-pixel fragments
    static constexpr int NCA = (NFA + NW - 1) / NW, NCB = (NFB + NW - 1) / NW, NCT = (TH + NW - 1) / NW;   // per wave
    static constexpr int ZPAD = 2 * PBLK, Y = ZPAD + PZP, T0 = Y + HRB * PYS;
    static constexpr int PLOA = HRA * 8, PLOB = HRB * 8;       // the lo plane's offset from the hi plane
    static constexpr int END = T0 + 2 * PLOA;
    static constexpr size_t LDS_BYTES = (size_t)END * 4;
    static_assert(Y % 4 == 0 && T0 % 4 == 0, "every region starts on a 16-B boundary");
    static_assert(NW <= 2 * PLOA, "the range maxima fit in the t0 region");
    static_assert(LDS_BYTES <= 160 * 1024, "a CU has 160 KB of LDS");
};

__device__ __forceinline__ void ldw_hl(RawS &r, const float *p, int kq) {   // HL: hi chunk kq, lo chunk 4 + kq
    r.h = *reinterpret_cast<const uint4 *>(p + kq * 4);
    r.l = *reinterpret_cast<const uint4 *>(p + 16 + kq * 4);
}
// channels ch .. ch + 3 of plane pixel h, split as bneck_kernels.hip st4t (PL)
__device__ __forceinline__ void st4pl(float *t0, int plo, int h, int ch, float4 v) {
    const float e[4] = {v.x, v.y, v.z, v.w};
    _Float16 hh[4], ll[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hh[i] = (_Float16)e[i];
        ll[i] = (_Float16)(e[i] - (float)hh[i]);
    }
    unsigned char *b = reinterpret_cast<unsigned char *>(t0 + h * 8) + (ch >> 3) * 16 + (ch & 7) * 2;
    *reinterpret_cast<f16x4 *>(b) = (f16x4){hh[0], hh[1], hh[2], hh[3]};
    *reinterpret_cast<f16x4 *>(b + plo * 4) = (f16x4){ll[0], ll[1], ll[2], ll[3]};
}
}  // namespace

// a.a: the first block's launch arguments (x, its weights, rg: amax_in = x's range words, amax_out = y's),
// a.b: the second's (out, its weights, rg.amax_out = out's range words); the tile grid is a.a's
template <int TH, int NW>
__global__ void __launch_bounds__(NW * 64, 1) bneck_pair_kernel(const BneckPairArgs p) {
    using F = PairForm<TH, NW>;
    constexpr int TW = F::TW, HWA = F::HWA, HRA = F::HRA, HWB = F::HWB, HRB = F::HRB;
    extern __shared__ __attribute__((aligned(16))) float psm[];
    const BneckArgs &a = p.a, &b = p.b;
    span_enter(a.span);
    const int grp = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3), nslots = (int)(gridDim.x >> 3);
    const int CH = tile_walk_ch(a.ntiles);
    // a workgroup without a tile leaves before staging anything (bneck_kernels.hip)
    if (tile_walk(grp, slot, CH, a.ntiles, a.rev) < 0) {
        span_exit(a.span);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float rl = rng_lane(a.rg);                  // issued first, consumed once the staging loads are in flight
    // both blocks' weights by LDS-DMA in the HL chunk order, rows of SR 16-B slots, the last of each a pad slot
    // (bneck_kernels.hip pick()); the constants through registers
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const BneckArgs &q = k ? b : a;
        float *base_k = psm + k * PBLK;
        constexpr int SR1 = PK1S / 4, SR2 = PK2S / 4, SR3 = PK3S / 4, CPR1 = PKS1 * 8, CPR2 = PKS2 * 8, CPR3 = 8;
        constexpr int S1 = 16 * SR1, S2 = 16 * SR2, NSL = PWF / 4;
        static_assert(NSL % 64 == 0, "whole wave instructions");
        for (int base = wave * 64; base < NSL; base += F::NT) {    // wave-uniform
            const int s = base + lane;
            const uint4 *src;
            auto pick = [&](const void *w, int i, int SR, int CPR) {
                const int r = i / SR, c = i - r * SR;
                const int cs = (c & ~7) | ((c & 7) < 4 ? 2 * (c & 7) : 2 * (c & 3) + 1);
                src = (const uint4 *)w + r * CPR + (c < CPR ? cs : 0);
            };
            if (s < S1) pick(q.w1, s, SR1, CPR1);
            else if (s < S1 + S2) pick(q.w2, s - S1, SR2, CPR2);
            else pick(q.w3, s - S1 - S2, SR3, CPR3);
            __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(base_k + (size_t)base * 4), 16, 0, 0);
        }
        float *cb1 = base_k + PWF, *cs1 = cb1 + 16, *cb2 = cs1 + 16, *cs2 = cb2 + 16, *cb3 = cs2 + 16, *cs3 = cb3 + PC, *cso = cs3 + PC;
        if (tid < 16) { cb1[tid] = q.b1[tid]; cs1[tid] = q.s1[tid]; cb2[tid] = q.b2[tid]; cs2[tid] = q.s2[tid]; }
        if (tid < PC) { cb3[tid] = q.b3[tid]; cs3[tid] = q.s3[tid]; cso[tid] = q.s_out[tid]; }
    }
    if (tid < PZP) psm[F::ZPAD + tid] = 0.f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the speculation's first half: block A's exponents from the measured max |x| (every load has landed, so a
    // workgroup may leave). Block B's are checked by the guarded launches that follow, from the max |y| below
    if (bneck_range<false>(a.rg, rng_reduce(rl)).any) {
        span_exit(a.span);
        return;
    }
    __syncthreads();

    float *const zpad = psm + F::ZPAD, *const ys = psm + F::Y, *const t0 = psm + F::T0;
    const auto rxb = mkbuf(a.x, a.x_bytes);
    const auto rob = mkbuf(b.out, a.x_bytes);
    auto act = [](float4 v, const float *s) { return prelu4m(v, ld4f(s)); };   // slopes <= 1 (planned so)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float amy = 0.f, amo = 0.f;                        // max |y|, max |out| of this lane

    // one block's regions
    auto blk = [&](int k, const float *&w1, const float *&w2, const float *&w3, const float *&cb1) {
        w1 = psm + k * PBLK; w2 = w1 + PW1; w3 = w2 + PW2; cb1 = w3 + PW3;
    };
    // the 1x1 projection of one 16-pixel fragment: lane (col, kq) holds channels 8 (4 s + kq) .. + 7 of pixel col
    auto project = [&](const float *w1, const float *cb1, const RawF (&xs)[PKS1]) -> float4 {
        f32x4 acc = bias4(cb1 + kq * 4);
#pragma unroll
        for (int s = 0; s < PKS1; ++s) {
            RawS wf;
            ldw_hl(wf, w1 + col * PK1S + s * 32, kq);
            mma(acc, wf, xs[s]);
        }
        return act(f4(acc), cb1 + 16 + kq * 4);
    };
    // the 3x3 of the pixel at plane index hc (its top-left tap; plane width hw) -> the expansion's B operand
    auto middle = [&](const float *w2, const float *cb2, int hc, int hw, int plo, RawF &tf) {
        f32x4 acc = bias4(cb2 + kq * 4);
#pragma unroll
        for (int s = 0; s < PKS2; ++s) {
            const int g = s * 4 + kq;
            const int tap = g >> 1, coff = (g & 1) * 4;
            const int ky = tap / 3, kx = tap - ky * 3;
            int off = (hc + ky * hw + kx) * 8 + coff;
            asm volatile("" : "+v"(off));
            RawS xf, wf;
            xf.h = *reinterpret_cast<const uint4 *>(g < PG2 ? t0 + off : zpad);
            xf.l = *reinterpret_cast<const uint4 *>(g < PG2 ? t0 + plo + off : zpad);
            ldw_hl(wf, w2 + col * PK2S + s * 32, kq);
            mma(acc, wf, xf);
        }
        to_bop(tf, act(f4(acc), cb2 + 16 + kq * 4), zero4);
    };
    // row block r of the expansion + residual + activation
    auto expand = [&](const float *w3, const float *cb3, int r, const RawF &tf, float4 res) -> float4 {
        const int ch = r * 16 + kq * 4;
        f32x4 acc = bias4(cb3 + ch);
        RawS wf;
        ldw_hl(wf, w3 + (r * 16 + col) * PK3S, kq);
        mma(acc, wf, tf);
        const float4 v = act(f4(acc), cb3 + PC + ch);
        return act(add4(v, res), cb3 + 2 * PC + ch);
    };

    const int wword = tile_walk_mirror(grp, CH, a.ntiles, a.rev);
    // the workgroup's tile of iteration it, or -1 past its last
    auto tile_at = [&](int it) -> int {
        const int tile = grp * CH + it;
        return it < CH && tile < a.ntiles ? tile_walk_flip(wword, tile) : -1;
    };
    // a tile's origin (oy0, ox0) and its frame's byte offset
    auto origin = [&](int tile, int &oy0, int &ox0, uint32_t &xn) {
        const int txi = tile % a.tiles_x, t2 = tile / a.tiles_x;
        const int tyi = t2 % a.tiles_y, n = t2 / a.tiles_y;
        oy0 = a.oy_base + tyi * TH; ox0 = txi * TW;
        xn = (uint32_t)(n * a.H * a.W) * (uint32_t)(PC * 4);
    };
    // byte offset of channel 0 of pixel (y, x) of the frame at xn, or OOB outside the image
    auto pixn = [&](uint32_t xn, int y, int x) -> uint32_t {
        uint32_t v = xn + (__umul24((uint32_t)y, (uint32_t)a.W) + (uint32_t)x) * (uint32_t)(PC * 4);
        asm volatile("" : "+v"(v));
        return (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W ? v : OOB;
    };
    // A1's loads: x of the wave's fragments c0 .. c1 - 1 of t0_A's plane of `tile` (every offset OOB, so zeros and
    // nothing dereferenced, for tile < 0), lane (col, kq) channels 8 (4 s + kq) .. + 7 of plane pixel 16 f + col
    constexpr int NPF = BNECK_PAIR_PREF < F::NCA ? BNECK_PAIR_PREF : F::NCA;   // fragments held across the barrier
    RawF xf[F::NCA][PKS1];
    uint32_t pof[F::NCA];
    auto a1_loads = [&](int tile, int c0, int c1) {
        int oy0 = 0, ox0 = 0;
        uint32_t xn = 0;
        if (tile >= 0) origin(tile, oy0, ox0, xn);     // wave-uniform
#pragma unroll
        for (int c = 0; c < F::NCA; ++c) {
            const int f = wave + NW * c;
            if (c < c0 || c >= c1) continue;
            if (f >= F::NFA) break;                    // wave-uniform
            const int h = f * 16 + col, hy = h / HWA, hx = h - hy * HWA;
            pof[c] = h < HRA && tile >= 0 ? pixn(xn, oy0 - 2 + hy, ox0 - 2 + hx) : OOB;
#pragma unroll
            for (int s = 0; s < PKS1; ++s) bld8(xf[c][s], rxb, pof[c] == OOB ? OOB : pof[c] + (uint32_t)((s * 4 + kq) * 32));
        }
    };
    if (NPF) a1_loads(tile_at(slot), 0, NPF);
    for (int it = slot; it < CH; it += nslots) {
        const int tile = tile_at(it);
        if (tile < 0) break;
        int oy0, ox0;
        uint32_t xn;
        origin(tile, oy0, ox0, xn);
        auto pix = [&](int y, int x) -> uint32_t { return pixn(xn, y, x); };
        const float *w1, *w2, *w3, *cb1;
        STAMP(0); STAMP_WG();

        // ---- A1: t0_A over tile +- 2. Every load of the wave's fragments is issued before the first MFMA (the
        // first NPF of them by the previous tile). XLDS: the raw x of tile +- 1 goes to the y region as loaded
        blk(0, w1, w2, w3, cb1);
        a1_loads(tile, NPF, F::NCA);
#ifdef BUGSEG_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        STAMP(1);
#endif
#pragma unroll
        for (int c = 0; c < F::NCA; ++c) {
            const int f = wave + NW * c;
            if (f >= F::NFA) break;
            const int h = f * 16 + col;
            if (BNECK_PAIR_XLDS) {
                const int hy = h / HWA, hx = h - hy * HWA;
                if (hy >= 1 && hy <= TH + 2 && hx >= 1 && hx <= TW + 2) {   // inside tile +- 1 (h < HRA follows)
                    float *xq = ys + ((hy - 1) * HWB + hx - 1) * PYS + kq * 8;
#pragma unroll
                    for (int s = 0; s < PKS1; ++s) { st4(xq + s * 32, xf[c][s].a); st4(xq + s * 32 + 4, xf[c][s].b); }
                }
            }
            float4 v = project(w1, cb1, xf[c]);
            if (pof[c] == OOB) v = zero4;
            if (h < HRA) st4pl(t0, F::PLOA, h, kq * 4, v);
        }
        __syncthreads();
        STAMP(2);
        if (NPF) a1_loads(tile_at(it + nslots), 0, NPF);

        // ---- A2 + A3: y over tile +- 1 into LDS, 0 outside the image; the residual x from the y region
        // (XLDS) or re-read (L2)
#pragma unroll
        for (int c = 0; c < F::NCB; ++c) {
            const int f = wave + NW * c;
            if (f >= F::NFB) break;                   // wave-uniform
            const int q = f * 16 + col, qq = q < HRB ? q : 0;
            const int ry = qq / HWB, rx = qq - ry * HWB;
            const uint32_t po = q < HRB ? pix(oy0 - 1 + ry, ox0 - 1 + rx) : OOB;
            // XLDS: the lane reads its four residual values where it then writes y (a lane past the plane reads
            // pixel 0's and drops the result)
            uint4 res[PNR3];
#pragma unroll
            for (int r = 0; r < PNR3; ++r)
                res[r] = BNECK_PAIR_XLDS ? __builtin_bit_cast(uint4, ld4(ys + qq * PYS + r * 16 + kq * 4))
                                         : bld16(rxb, po == OOB ? OOB : po + (uint32_t)((r * 16 + kq * 4) * 4));
            RawF tf;
            middle(w2, cb1 + 32, ry * HWA + rx, HWA, F::PLOA, tf);
#pragma unroll
            for (int r = 0; r < PNR3; ++r) {
                float4 v = expand(w3, cb1 + 64, r, tf, __builtin_bit_cast(float4, res[r]));
                if (po == OOB) v = zero4;
                rng_acc4(amy, v);
                if (q < HRB) st4(ys + q * PYS + r * 16 + kq * 4, v);
            }
        }
        __syncthreads();
        STAMP(3);

        // ---- B1: t0_B over tile +- 1 from y, into the t0 region (t0_A is dead)
        blk(1, w1, w2, w3, cb1);
#pragma unroll
        for (int c = 0; c < F::NCB; ++c) {
            const int f = wave + NW * c;
            if (f >= F::NFB) break;
            const int q = f * 16 + col, qq = q < HRB ? q : 0;
            const int ry = qq / HWB, rx = qq - ry * HWB;
            const bool ok = q < HRB && (unsigned)(oy0 - 1 + ry) < (unsigned)a.H && (unsigned)(ox0 - 1 + rx) < (unsigned)a.W;
            RawF xs[PKS1];
#pragma unroll
            for (int s = 0; s < PKS1; ++s) ld8(xs[s], ys + qq * PYS + (s * 4 + kq) * 8);
            float4 v = project(w1, cb1, xs);
            if (!ok) v = zero4;
            if (q < HRB) st4pl(t0, F::PLOB, q, kq * 4, v);
        }
        __syncthreads();
        STAMP(4);

        // ---- B2 + B3: the tile's rows, residual y from LDS, whole-line stores (bneck_kernels.hip LINES): rows
        // 2u / 2u + 1 of pixels col and col ^ 8 traded across lanes 8 apart, then line u of each pixel
#pragma unroll
        for (int c = 0; c < F::NCT; ++c) {
            const int f = wave + NW * c;              // tile row
            if (f >= TH) break;                       // wave-uniform
            RawF tf;
            middle(w2, cb1 + 32, f * HWB + col, HWB, F::PLOB, tf);
            const float *yr = ys + ((f + 1) * HWB + col + 1) * PYS;
            const uint32_t po = pix(oy0 + f, ox0 + col), po_o = pix(oy0 + f, ox0 + (col ^ 8));
            const bool lo8 = col < 8;
            const uint32_t pa = lo8 ? po : po_o, pb = lo8 ? po_o : po;
#pragma unroll
            for (int u = 0; u < PNR3 / 2; ++u) {
                float4 v2[2];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int r = 2 * u + hh;
                    v2[hh] = expand(w3, cb1 + 64, r, tf, ld4(yr + r * 16 + kq * 4));
                    rng_acc4(amo, v2[hh]);
                }
                const uint4 u0 = __builtin_bit_cast(uint4, v2[0]), u1 = __builtin_bit_cast(uint4, v2[1]);
                const uint4 xs = lo8 ? u1 : u0;
                uint4 yx;
                yx.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)xs.x, 0x128, 0xf, 0xf, false);
                yx.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)xs.y, 0x128, 0xf, 0xf, false);
                yx.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)xs.z, 0x128, 0xf, 0xf, false);
                yx.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)xs.w, 0x128, 0xf, 0xf, false);
                const uint32_t cb = (uint32_t)(u * 32 + (lo8 ? 0 : 16) + kq * 4) * 4u;
                bst16o<16>(rob, pa == OOB ? OOB : pa + cb, lo8 ? u0 : yx);
                bst16o<16>(rob, pb == OOB ? OOB : pb + cb, lo8 ? yx : u1);
            }
        }
        __syncthreads();                              // the next tile writes t0 and y
        STAMP(5);
    }
    rng_commit_wg(amy, a.rg.amax_out, t0, NW);
    rng_commit_wg(amo, b.rg.amax_out, t0, NW);
    span_exit(a.span);
}

// ---- the built form: tile height and waves by measurement
constexpr int PAIR_TH = 12, PAIR_NW = 16;
using PairBuilt = PairForm<PAIR_TH, PAIR_NW>;
static const void *pair_fun() { return (const void *)bneck_pair_kernel<PAIR_TH, PAIR_NW>; }

void bneck_pair_shape(int &th, int &tw, int &threads, size_t &lds) {
    th = PAIR_TH; tw = PairBuilt::TW; threads = PairBuilt::NT; lds = PairBuilt::LDS_BYTES;
}

hipError_t launch_bneck_pair(const Knobs &k, const BneckPairArgs &a, hipStream_t s) {
    hipError_t e = allow_dynamic_lds(pair_fun());
    if (e != hipSuccess) return e;
    const int g = resident_grid(k, pair_fun(), PairBuilt::NT, PairBuilt::LDS_BYTES, a.a.ntiles);   // (bneck_kernels.hip)
    void *args[] = {const_cast<BneckPairArgs *>(&a)};
    return hipLaunchKernel(pair_fun(), dim3(g), dim3(PairBuilt::NT), args, PairBuilt::LDS_BYTES, s);
}

}  // namespace bugseg
