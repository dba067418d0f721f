// The BSG1 weight blob (enet_spec.py) as one value: parsed, batch-norm folded into the convolutions in double and
// packed for the MFMA kernels ([Npad][Kpad] rows, 8-channel k groups, tap table) into the staging image of the
// context's one device allocation. Host only: no HIP call and no context (enet_weights.cpp).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "knobs.h"

namespace bugseg {

struct UnitDesc {
    int kind = 0, cout = 0, cin = 0, kh = 0, kw = 0, stride = 1, pad_h = 0, pad_w = 0, dil_h = 1, dil_w = 1, out_pad = 0;
    float eps = 0.f;
    std::vector<float> w, b, gamma, beta, mean, var, slope;
};

struct BlockDesc {
    int type = 0;
    int attrs[8] = {0};
    std::vector<UnitDesc> units;
    std::vector<std::vector<float>> extra;
};

enum { BT_INITIAL = 1, BT_REGULAR = 2, BT_DOWN = 3, BT_UP = 4, BT_FULLCONV = 5 };

// One packed convolution launch (weights resident on the device).
struct Packed {
    int Npad = 0, Kpad = 0, Ksteps = 0, nr = 0;
    int CinS = 0;      // input storage channels
    int stride = 1;    // on the GEMM grid
    int cout = 0;      // valid output channels (per phase)
    int coutP = 0;     // per-phase padded channels
    int phases = 1;
    double macs_per_px = 0;   // MACs per GEMM pixel (flop accounting)
    size_t o_w = 0, o_gtab = 0, o_bias = 0, o_s1 = 0, o_s2 = 0, o_ps = 0;
    // fp32 mode range scaling (bugseg_internal.h RangeArgs): the weights' exponent (packed w = w * 2^sw)
    // and per packed row the bound terms of its activated output: sum |w|, |bias|, max(1, |slope|)
    int sw = 0;
    std::vector<float> rabs, rbias, rslope;
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int pow2_nr(int npad) {   // 16-row fragments, rounded up to 1, 2, 4 or 8
    int nr = npad / 16;
    int p = 1;
    while (p < nr) p <<= 1;
    return p;
}
inline int cstore(int c) { return round_up(c, 8); }   // storage channels of a c-channel tensor

// weight exponent of a matrix whose largest |w| is m (the measured-tensor window of the kernels)
int range_weight_exp(double m);
// |act(W x + b)| <= n |x| + c over the rows [r0, r1) of a packed matrix (a 1e-4 margin for the f32
// arithmetic the kernels evaluate the bound in)
void row_bound(const Packed &p, int r0, int r1, float &n, float &c);

struct EnetWeights {
    int ncls = 0;
    std::vector<BlockDesc> blocks;
    std::vector<Packed> packed;
    std::vector<std::vector<int>> block_convs;   // per block: indices into packed
    std::vector<unsigned char> host_w;           // the staging image of the one device allocation
};
// parse_blob, then the packing for precision prec (Prec) under the knobs f32_range and no_pair. Writes only out,
// which is complete on true; false: why says what the blob lacks, and out is not to be used.
bool build_weights(const void *blob, size_t bytes, int prec, const Knobs &k, EnetWeights &out, std::string &why);

}  // namespace bugseg
