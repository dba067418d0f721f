// Connected-component labelling shared by road_kernels.hip and canny_kernels.hip: a lock-free union-find over
// a label image, per 16 x 64 tile in LDS, then across tile borders in memory. Semantics: DESIGN.md §6.16.
//
// Visibility across workgroups (MI355X: the L2 of one XCD is not coherent with another's, a CU's L1 is never
// refreshed by another CU's stores): inside a launch that links across workgroups (the border merge, and any
// later launch of an operator that names this rule) every word another workgroup may change is read and
// written with agent-scope atomics only; everything else a launch reads was written by an earlier launch (a
// kernel boundary makes it visible).
//
// A pixel has a kind: 0 background, 4-connected; 1 foreground, 8-connected; 2 joins nothing and gets no label.
// An operator describes its pixels with a policy P:
//   static constexpr bool HAS_BG       whether kind 0 can occur; when not, its paths fold away at compile time
//   static constexpr bool HAS_NONE     whether kind 2 can occur inside the frame (outside it, it always does)
//   int W, H                           the frame's shape
//   uint8_t kind(int p) const          the kind of pixel p = y * W + x, inside the frame
//   void store(int p, int root) const  (tile labelling only) p's label: the frame index of its region's
//                                      raster-first pixel inside the tile. Called for every pixel not of kind 2
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bugseg {

constexpr int LT_TH = 16, LT_TW = 64;     // labelling: tile (LT_TH * LT_TW labels in LDS)
constexpr int LT_N = LT_TH * LT_TW;

// ---------------------------------------------------------------- union-find
// Labels only decrease and label[x] <= x always, so the forest stays acyclic under any interleaving; the
// root of a set is its smallest index, i.e. its raster-first pixel.
__device__ inline int ld_wg(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline int ld_agent(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool LDS>
__device__ inline int uf_find(int *lab, int x) {
    for (;;) {
        int p = LDS ? ld_wg(lab + x) : ld_agent(lab + x);
        if (p == x) return x;
        x = p;
    }
}

template <bool LDS>
__device__ inline void uf_union(int *lab, int a, int b) {
    for (;;) {
        a = uf_find<LDS>(lab, a);
        b = uf_find<LDS>(lab, b);
        if (a == b) return;
        if (a > b) { int t = a; a = b; b = t; }
        int old = atomicMin(lab + b, a);   // vector atomic (LDS: ds_min, global: device scope)
        if (old == b) return;
        b = old;
    }
}

// ---------------------------------------------------------------- per-tile labelling in LDS
// The tile whose first pixel is (x0, y0), by one workgroup of THREADS threads. A pixel joins its W and N
// neighbours of the same kind, a foreground pixel its NW and NE ones too. Pixels outside the frame are of kind 2.
template <int THREADS, class P>
__device__ inline void label_tile(const P &px, int x0, int y0) {
    __shared__ int lab[LT_N];
    __shared__ uint8_t kind[LT_N];
    const int W = px.W, H = px.H;
    const int tid = threadIdx.x;
    // a tile row is one wave (LT_TW = 64 lanes): every pixel starts at the first pixel of its horizontal run,
    // found from the ballot of its kind, so no union is needed along rows
    static_assert(LT_TW == 64 && THREADS % 64 == 0, "one wave per tile row");
    for (int i = tid; i < LT_N; i += THREADS) {
        int ly = i / LT_TW, lx = i - ly * LT_TW;
        int gy = y0 + ly, gx = x0 + lx;
        uint8_t kd = (gy < H && gx < W) ? px.kind(gy * W + gx) : 2;
        unsigned long long same = __ballot(kd == 1);
        if constexpr (P::HAS_BG) {
            unsigned long long m0 = __ballot(kd == 0);
            same = kd == 1 ? same : kd == 0 ? m0 : 0ull;
        }
        unsigned long long brk = ~same & ((1ull << lx) - 1ull);       // lanes below of another kind
        int start = brk ? 64 - __clzll((long long)brk) : 0;
        kind[i] = kd;
        lab[i] = kd == 2 ? i : ly * LT_TW + start;
    }
    __syncthreads();
    // rows are joined where an overlap of two runs starts (the pixels after it hang together through both
    // rows); a diagonal only where no straight neighbour makes the same link
    for (int i = tid; i < LT_N; i += THREADS) {
        int ly = i / LT_TW, lx = i - ly * LT_TW;
        uint8_t kd = kind[i];
        if (kd == 2 || ly == 0) continue;
        uint8_t up = kind[i - LT_TW];
        bool wsame = lx > 0 && kind[i - 1] == kd;
        uint8_t nw = lx > 0 ? kind[i - LT_TW - 1] : 2;
        if (up == kd && !(wsame && nw == kd)) uf_union<true>(lab, i, i - LT_TW);
        if ((!P::HAS_BG || kd == 1) && up != 1) {
            if (nw == 1 && !wsame) uf_union<true>(lab, i, i - LT_TW - 1);
            if (lx + 1 < LT_TW && kind[i - LT_TW + 1] == 1) uf_union<true>(lab, i, i - LT_TW + 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < LT_N; i += THREADS) {
        if (kind[i] == 2) continue;
        int ly = i / LT_TW, lx = i - ly * LT_TW;
        int r = uf_find<true>(lab, i);
        int ry = r / LT_TW, rx = r - ry * LT_TW;
        px.store((y0 + ly) * W + x0 + lx, (y0 + ry) * W + x0 + rx);
    }
}

// ---------------------------------------------------------------- merge across tile borders
// Pixel (x, y) of the frame, at (tx, ty) inside its tile, joins those of its W, NW, N and NE neighbours that lie
// in another tile, under its kind's connectivity. Call it for every pixel of a tile's top row, left column and
// right column; for any other pixel it does nothing. lab: the frame's label image.
template <class P>
__device__ inline void link_border(const P &px, int *lab, int x, int y, int tx, int ty) {
    const int W = px.W, p = y * W + x;
    // As inside a tile, a straight link is made only where an overlap of two runs starts along the border
    // (after it, the pixels on either side hang together along the border, through links made in their tiles
    // or by this launch), and a diagonal only where no straight neighbour makes the same link: a uniform
    // region crossing many tiles costs one atomic per border, not one per border pixel.
    const uint8_t kd = px.kind(p);
    // (only where kind 2 occurs inside the frame: elsewhere the branch would just hold the loads below back)
    if (P::HAS_NONE && kd == 2) return;
    const uint8_t wk = x > 0 ? px.kind(p - 1) : 2, nk = y > 0 ? px.kind(p - W) : 2;
    const uint8_t nwk = (x > 0 && y > 0) ? px.kind(p - W - 1) : 2;
    // (the pixel in a tile's corner makes both links whatever its neighbours: each rule would lean on the other)
    const bool corner = tx == 0 && ty == 0;
    if (tx == 0 && wk == kd && (corner || !(nk == kd && nwk == kd))) uf_union<false>(lab, p, p - 1);
    if (ty == 0 && nk == kd && (corner || !(wk == kd && nwk == kd))) uf_union<false>(lab, p, p - W);
    if ((!P::HAS_BG || kd == 1) && y > 0 && nk != 1) {
        if ((ty == 0 || tx == 0) && nwk == 1 && wk != 1) uf_union<false>(lab, p, p - W - 1);
        if ((ty == 0 || tx == LT_TW - 1) && x + 1 < W && px.kind(p - W + 1) == 1) uf_union<false>(lab, p, p - W + 1);
    }
}

}  // namespace bugseg
