// What a context keeps for the BEV rasteriser's host side (bev_runtime.cpp).
#pragma once
#include <array>
#include <stdint.h>

#include "ctx_memory.h"

namespace bugseg {

struct BevState {
    // laserscan mode: polar tables by (occ_w, occ_h, variant); tab: fmap (ph*pw int32) then imap (occ_h*occ_w int32)
    struct Polar { int pw = 0, ph = 0; };
    TableCache<std::array<int, 3>, Polar> polar_tabs;
    // warp-tap tables (bev_kernels.hip bev_table_kernel) by the geometry fields of BevArgs. row0, row1: the
    // class-map rows [row0, row1) that carry weight in some tap (bugseg_bev_source_rows)
    struct Taps { int nitems = 0, row0 = 0, row1 = 0; };
    TableCache<std::vector<unsigned char>, Taps> bev_tabs;
    // laserscan batch scratch of bugseg_bev_occgrid (bugseg_bev_occgrid_ws takes the caller's): keyed by stream,
    // so that calls enqueued on different streams of one context never share intermediate buffers
    struct LsScratch { void *stream = nullptr; void *p = nullptr; size_t bytes = 0; uint64_t used = 0; bool pinned = false; };
    std::vector<LsScratch> ls_scratch;
    uint64_t use_clock = 0;
    ~BevState() { for (LsScratch &s : ls_scratch) (void)hipFree(s.p); }
};

}  // namespace bugseg
