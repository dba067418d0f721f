// The rolling local map: B occupancy grids, each with the pose it was taken at, fused in time
// order into a world-aligned log-odds map that scrolls with the vehicle, and the nav_msgs/OccupancyGrid payload of
// that map. Integers only: the host turns every pose into a fixed-point record (mapping.pose_record), the device
// adds, shifts, compares and clamps. Bit for bit the restatement in tests/map_ref.py.
//
// The host entry point (bugseg_map_fuse) lives here beside the kernel, as in eval_kernels.hip: the runtime
// translation units reference nothing of this file; this file uses what bugseg_internal.h and the runtime export.
//
// One launch. A workgroup of 256 threads owns a tile of 16 rows x 64 columns of the window; a wave owns 16 x 16
// of them (lanes 4 rows x 16 columns, four cells per lane, 4 rows apart), so that whatever the yaw a wave's gather
// stays within a 16 x 16-cell patch of a grid. Every cell has one owner, and the owner alone touches the cell's
// torus slot: no atomics, no races, the same bits every run.
//
//   1  frame list   thread t tests frames t, t + 256, ...: a frame stays when it is not skipped and (with culling)
//                   when its footprint can reach the tile. Both coordinates are affine in (i, j), so their extremes
//                   over the tile lie at its corners: a frame whose forward index is negative at every corner, or
//                   at least grid_rows at every corner, or whose lateral index is so, samples nothing here and
//                   leaving it out changes nothing. The frames that stay are written to LDS in ascending order
//                   (ballot, popcount below the lane, per-wave counts): the order of fusion is the order of time
//   2  placement    a cell keeps its stored value when the map is not fresh and its world cell lay in the previous
//                   window; otherwise it starts unobserved, whatever the slot holds (no memset)
//   3  fusion       for the listed frames in order: the frame's record through uniform loads (the index comes out
//                   of LDS through readfirstlane), the two fixed-point coordinates, one byte gathered from L2,
//                   the clamped step
//   4  emission     the slot gets the new state, the payload lut[L - l_min], or -1 where nothing was ever seen
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bugseg_internal.h"
#include "../../include/bugseg.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = 64, TILE_H = 16;  // window cells of a workgroup
constexpr int WAVE_W = 16;               // columns of a wave; its lanes are 4 rows x 16 columns
constexpr int CELLS = 4;                 // cells of a lane, 4 rows apart
constexpr int MAX_SIDE = 4096, MAX_B = 4096;
constexpr int UNOBSERVED = BUGSEG_MAP_UNOBSERVED;
constexpr int HDR = BUGSEG_MAP_RECORD_HEADER, FRM = BUGSEG_MAP_RECORD_FRAME;

struct MapArgs {
    const int8_t *__restrict__ grids;
    const long long *__restrict__ rec;
    int16_t *__restrict__ state;
    const int8_t *__restrict__ lut;
    int8_t *__restrict__ out;
    int B, h, w, Hm, Wm;
    int ros, l_occ, l_free, l_min, l_max, cull;
};

__device__ __forceinline__ int floor_mod(int a, int m) {
    int r = a % m;
    return r < 0 ? r + m : r;
}

__global__ void __launch_bounds__(THREADS) map_fuse_kernel(MapArgs a) {
    __shared__ uint16_t list[MAX_B];
    __shared__ int wave_count[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * TILE_W, i0 = blockIdx.y * TILE_H;
    const long long half_w = (long long)a.w << 15;

    // 1: the frames of this tile, in order
    const int j1 = min(j0 + TILE_W, a.Wm) - 1, i1 = min(i0 + TILE_H, a.Hm) - 1;
    int n = 0;
    for (int base = 0; base < a.B; base += THREADS) {
        const int k = base + tid;
        bool keep = false;
        if (k < a.B) {
            const long long *f = a.rec + HDR + (size_t)k * FRM;
            const long long C = f[0], S = f[1], Ox = f[2], Oy = f[3];
            keep = (C | S) != 0;
            if (keep && a.cull) {
                const long long xa = C * j0 + S * i0 + Ox, xb = C * j1 + S * i0 + Ox;
                const long long xc = C * j0 + S * i1 + Ox, xd = C * j1 + S * i1 + Ox;
                const long long ya = -S * j0 + C * i0 + Oy, yb = -S * j1 + C * i0 + Oy;
                const long long yc = -S * j0 + C * i1 + Oy, yd = -S * j1 + C * i1 + Oy;
                const long long x_lo = min(min(xa, xb), min(xc, xd)), x_hi = max(max(xa, xb), max(xc, xd));
                const long long y_lo = min(min(ya, yb), min(yc, yd)), y_hi = max(max(ya, yb), max(yc, yd));
                // lateral index: plain (half_w - yl) >> 16, falling in yl; ROS (yl + half_w) >> 16, rising
                const long long c_lo = a.ros ? (y_lo + half_w) >> 16 : (half_w - y_hi) >> 16;
                const long long c_hi = a.ros ? (y_hi + half_w) >> 16 : (half_w - y_lo) >> 16;
                keep = (x_hi >> 16) >= 0 && (x_lo >> 16) < a.h && c_hi >= 0 && c_lo < a.w;
            }
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_count[wave] = __popcll(bal);
        __syncthreads();
        int off = n, tot = 0;
        for (int v = 0; v < THREADS / 64; ++v) {
            if (v < wave) off += wave_count[v];
            tot += wave_count[v];
        }
        if (keep) list[off + __popcll(bal & ((1ull << lane) - 1))] = (uint16_t)k;
        n += tot;
        __syncthreads();
    }

    // 2: this lane's cells
    const int wx0 = (int)a.rec[0], wy0 = (int)a.rec[1], px0 = (int)a.rec[2], py0 = (int)a.rec[3];
    const bool fresh = a.rec[4] != 0;
    const int j = j0 + wave * WAVE_W + (lane & 15), ib = i0 + (lane >> 4);
    const bool col_in = j < a.Wm;
    const long long gx = (long long)wx0 + j;
    const bool col_kept = !fresh && gx >= px0 && gx < (long long)px0 + a.Wm;
    const int sx = floor_mod((int)gx, a.Wm);      // (a world cell fits an int: mapping.MAX_CELLS)
    int L[CELLS];
    bool in[CELLS];
    size_t slot[CELLS];
#pragma unroll
    for (int r = 0; r < CELLS; ++r) {
        const int i = ib + 4 * r;
        in[r] = col_in && i < a.Hm;
        const long long gy = (long long)wy0 + i;
        slot[r] = (size_t)floor_mod((int)gy, a.Hm) * a.Wm + sx;
        L[r] = UNOBSERVED;
        if (in[r] && col_kept && gy >= py0 && gy < (long long)py0 + a.Hm) {
            // (a state this kernel wrote lies in the clamp's range already; the clamp keeps a buffer that something
            // else wrote from indexing past the table)
            const int kept = a.state[slot[r]];
            L[r] = kept == UNOBSERVED ? kept : min(max(kept, a.l_min), a.l_max);
        }
    }

    // 3: fusion, in the list's order (no branch around a gather: a sample out of range reads the frame's first byte
    // and is dropped, so the four loads of a lane are in flight together)
    const unsigned uh = (unsigned)a.h, uw = (unsigned)a.w;
    const size_t frame_bytes = (size_t)a.h * a.w;
    for (int t = 0; t < n; ++t) {
        const int k = __builtin_amdgcn_readfirstlane((int)list[t]);
        const long long *f = a.rec + HDR + (size_t)k * FRM;
        const long long C = f[0], S = f[1];
        long long xq = C * j + S * ib + f[2], yq = -S * j + C * ib + f[3];
        const int8_t *g = a.grids + (size_t)k * frame_bytes;
        int v[CELLS];
#pragma unroll
        for (int r = 0; r < CELLS; ++r) {
            const long long fx = xq >> 16;
            const long long col = a.ros ? (yq + half_w) >> 16 : (half_w - yq) >> 16;
            const bool hit = in[r] && fx >= 0 && fx < a.h && col >= 0 && col < a.w;
            const unsigned ux = (unsigned)fx, uc = (unsigned)col;
            const unsigned at = a.ros ? uc * uh + ux : (uh - 1u - ux) * uw + uc;     // below 2^24 on a hit
            v[r] = g[hit ? at : 0u];
            if (!hit) v[r] = -1;
            xq += 4 * S;
            yq += 4 * C;
        }
#pragma unroll
        for (int r = 0; r < CELLS; ++r) {
            const int s = (L[r] == UNOBSERVED ? 0 : L[r]) + (v[r] == 100 ? a.l_occ : -a.l_free);
            if (v[r] == 100 || v[r] == 0) L[r] = min(max(s, a.l_min), a.l_max);
        }
    }

    // 4: the slot and the payload
#pragma unroll
    for (int r = 0; r < CELLS; ++r) {
        if (!in[r]) continue;
        a.state[slot[r]] = (int16_t)L[r];
        a.out[(size_t)(ib + 4 * r) * a.Wm + j] = L[r] == UNOBSERVED ? (int8_t)-1 : a.lut[L[r] - a.l_min];
    }
}

}  // namespace

extern "C" {

int bugseg_map_fuse(bugseg_ctx *ctx, const int8_t *grids_dev, int B, const bugseg_map_params *p, const int64_t *record_dev,
                    int16_t *state_dev, const int8_t *lut_dev, int8_t *out_dev, void *stream) {
    using bugseg::ctx_fail;
    using bugseg::ranges_overlap;
    if (!ctx || !grids_dev || !p || !record_dev || !state_dev || !lut_dev || !out_dev)
        return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: NULL argument");
    if (B < 1 || B > MAX_B) return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: B must be 1..4096");
    for (int side : {p->map_rows, p->map_cols, p->grid_rows, p->grid_cols})
        if (side < 1 || side > MAX_SIDE) return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: every side must be 1..4096");
    if (!(p->l_min > UNOBSERVED && p->l_min < 0 && p->l_max > 0 && p->l_max <= 32767))
        return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: needs -32768 < l_min < 0 < l_max <= 32767");
    if (p->l_occ < 1 || p->l_free < 1) return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: l_occ and l_free must be at least 1");
    if ((p->ros_layout != 0 && p->ros_layout != 1) || (p->cull != 0 && p->cull != 1))
        return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: ros_layout and cull are 0 or 1");
    if (((uintptr_t)record_dev & 7) || ((uintptr_t)state_dev & 1))
        return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: record_dev must be 8-byte and state_dev 2-byte aligned");
    const size_t cells = (size_t)p->map_rows * p->map_cols, n_grid = (size_t)B * p->grid_rows * p->grid_cols;
    const size_t n_rec = (size_t)(HDR + FRM * B) * 8, n_lut = (size_t)(p->l_max - p->l_min + 1);
    if (ranges_overlap(state_dev, cells * 2, out_dev, cells))
        return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: state_dev overlaps out_dev");
    for (void *wr : {(void *)state_dev, (void *)out_dev}) {
        const size_t n_wr = wr == (void *)state_dev ? cells * 2 : cells;
        if (ranges_overlap(wr, n_wr, grids_dev, n_grid) || ranges_overlap(wr, n_wr, record_dev, n_rec) ||
            ranges_overlap(wr, n_wr, lut_dev, n_lut))
            return ctx_fail(ctx, BUGSEG_EINVAL, "map fuse: a written buffer overlaps an input");
    }
    bugseg::DeviceGuard g(bugseg::ctx_device(ctx));
    MapArgs a;
    a.grids = grids_dev; a.rec = (const long long *)record_dev; a.state = state_dev; a.lut = lut_dev; a.out = out_dev;
    a.B = B; a.h = p->grid_rows; a.w = p->grid_cols; a.Hm = p->map_rows; a.Wm = p->map_cols;
    a.ros = p->ros_layout; a.cull = p->cull;
    // a step of the whole span or more clamps from anywhere in [l_min, l_max], so a larger one is the same step
    const int span = p->l_max - p->l_min;
    a.l_occ = p->l_occ < span ? p->l_occ : span; a.l_free = p->l_free < span ? p->l_free : span;
    a.l_min = p->l_min; a.l_max = p->l_max;
    const dim3 grid((unsigned)((a.Wm + TILE_W - 1) / TILE_W), (unsigned)((a.Hm + TILE_H - 1) / TILE_H));
    hipLaunchKernelGGL(map_fuse_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    return bugseg::launch_fail(ctx, "map fuse");
}

}
