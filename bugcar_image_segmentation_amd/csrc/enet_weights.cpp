// The BSG1 weight blob parsed and packed (enet_weights.h): pure host arithmetic, no HIP call. bugseg_load_weights
// installs the result; bugseg_debug_parse_pack, which the stand-alone sanitizer driver feeds, only builds it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "enet_weights.h"

// the weights' exponent for the fp32 mode's split-f16 products: 0 while the largest |w| lies in the
// kernels' measured window [2^-2, 2^15) (mfma_common.h rng_exp_meas), else the exponent that brings it
// to [2^14, 2^15), clamped as the kernels clamp
int bugseg::range_weight_exp(double m) {
    if (!(m > 0) || !std::isfinite(m)) return 0;
    int e = 0;
    (void)std::frexp(m, &e);
    const int l = e - 1;
    if (l >= -2 && l < 15) return 0;
    return std::max(-40, std::min(40, 14 - l));   // (mfma_common.h RNG_EMAX)
}

void bugseg::row_bound(const Packed &p, int r0, int r1, float &n, float &c) {
    n = c = 0.f;
    for (int r = r0; r < r1 && r < (int)p.rabs.size(); ++r) {
        n = std::max(n, p.rabs[r] * p.rslope[r]);
        c = std::max(c, p.rbias[r] * p.rslope[r]);
    }
    n *= 1.0001f;
    c *= 1.0001f;
}

namespace {
using namespace bugseg;

// ---------------------------------------------------------------- blob parsing
struct Reader {
    const unsigned char *p, *end;
    bool ok = true;
    template <typename T> T get() {
        T v{};
        if (p + sizeof(T) > end) { ok = false; return v; }
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
    std::vector<float> tensor() {
        uint32_t n = get<uint32_t>();
        std::vector<float> v;
        if (!ok || (size_t)(end - p) / 4 < (size_t)n) { ok = false; return v; }   // (no pointer past the end)
        v.resize(n);
        if (n) std::memcpy(v.data(), p, (size_t)n * 4);   // (memcpy from / to NULL is UB even for 0 bytes)
        p += (size_t)n * 4;
        return v;
    }
};

bool parse_blob(const void *blob, size_t bytes, std::vector<BlockDesc> &out, int &ncls, std::string &why) {
    Reader r{(const unsigned char *)blob, (const unsigned char *)blob + bytes};
    char magic[4];
    for (int i = 0; i < 4; ++i) magic[i] = r.get<char>();
    if (!r.ok || std::memcmp(magic, "BSG1", 4) != 0) { why = "bad magic (expected BSG1)"; return false; }
    uint32_t ver = r.get<uint32_t>(), nb = r.get<uint32_t>(), nc = r.get<uint32_t>();
    if (!r.ok || ver != 1) { why = "unsupported blob version"; return false; }
    if (nb == 0 || nb > 4096 || nc == 0 || nc > 16) { why = "bad block/class count"; return false; }
    ncls = (int)nc;
    for (uint32_t b = 0; b < nb; ++b) {
        BlockDesc bd;
        bd.type = (int)r.get<uint32_t>();
        for (int i = 0; i < 8; ++i) bd.attrs[i] = r.get<int32_t>();
        uint32_t nu = r.get<uint32_t>();
        if (!r.ok || nu > 16) { why = "bad unit count"; return false; }
        for (uint32_t u = 0; u < nu; ++u) {
            UnitDesc ud;
            int32_t iv[11];
            for (int i = 0; i < 11; ++i) iv[i] = r.get<int32_t>();
            ud.kind = iv[0]; ud.cout = iv[1]; ud.cin = iv[2]; ud.kh = iv[3]; ud.kw = iv[4]; ud.stride = iv[5];
            ud.pad_h = iv[6]; ud.pad_w = iv[7]; ud.dil_h = iv[8]; ud.dil_w = iv[9]; ud.out_pad = iv[10];
            ud.eps = r.get<float>();
            ud.w = r.tensor(); ud.b = r.tensor(); ud.gamma = r.tensor(); ud.beta = r.tensor();
            ud.mean = r.tensor(); ud.var = r.tensor(); ud.slope = r.tensor();
            if (!r.ok) { why = "truncated unit"; return false; }
            if (ud.cout <= 0 || ud.cin <= 0 || ud.kh <= 0 || ud.kw <= 0 || ud.cout > 128 || ud.cin > 128 || ud.kh > 7 || ud.kw > 7) {
                why = "unit dims out of range"; return false;
            }
            const size_t nw = (size_t)ud.cout * ud.cin * ud.kh * ud.kw;
            const size_t c = (size_t)ud.cout;
            if (ud.w.size() != nw || ud.b.size() != c || ud.gamma.size() != c || ud.beta.size() != c ||
                ud.mean.size() != c || ud.var.size() != c || ud.slope.size() != c) {
                why = "unit tensor size mismatch"; return false;
            }
            bd.units.push_back(std::move(ud));
        }
        uint32_t ne = r.get<uint32_t>();
        if (!r.ok || ne > 16) { why = "bad extra count"; return false; }
        for (uint32_t e = 0; e < ne; ++e) bd.extra.push_back(r.tensor());
        if (!r.ok) { why = "truncated extras"; return false; }
        out.push_back(std::move(bd));
    }
    return true;
}

// ---------------------------------------------------------------- packing
// IEEE binary16 bits of a finite float, round to nearest even (the fp16-storage mode's weights);
// overflow to +-inf, underflow through the subnormals to +-0 — as a (_Float16) cast does
uint16_t f32_to_f16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int32_t exp = (int32_t)((u >> 23) & 0xff) - 127 + 15;
    uint32_t man = u & 0x7fffffu;
    if (((u >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (man ? 0x200u : 0u));   // inf / nan
    if (exp >= 31) return (uint16_t)(sign | 0x7c00u);
    if (exp <= 0) {                                  // subnormal half (or zero)
        if (exp < -10) return (uint16_t)sign;
        man |= 0x800000u;
        const int shift = 14 - exp;                  // 24-bit significand -> 10 + exp bits
        uint32_t h = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (h & 1u))) ++h;
        return (uint16_t)(sign | h);
    }
    uint32_t h = ((uint32_t)exp << 10) | (man >> 13);
    const uint32_t rem = man & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;   // may carry into the exponent (-> inf): correct
    return (uint16_t)(sign | h);
}
// the float value of IEEE binary16 bits (exact)
float f16_to_f32(uint16_t h) {
    const float s = (h & 0x8000u) ? -1.f : 1.f;
    const int e = (h >> 10) & 31, m = h & 1023;
    if (e == 31) return m ? std::nanf("") : s * INFINITY;
    if (e == 0) return s * std::ldexp((float)m, -24);
    return s * std::ldexp((float)(m | 1024), e - 25);
}

struct Packer {
    int prec;
    bool range;   // fp32 with Knobs::f32_range: the packed matrices carry a weight exponent (range_stats)
    std::vector<unsigned char> &buf;
    size_t push(const void *d, size_t n) {
        size_t off = round_up((int)buf.size(), 256);
        buf.resize(off + n);
        std::memcpy(buf.data() + off, d, n);
        return off;
    }
    size_t push_w(const std::vector<double> &w, int sw = 0) {
        if (prec == PREC_F16) {
            std::vector<uint16_t> h(w.size());
            for (size_t i = 0; i < w.size(); ++i) h[i] = f32_to_f16((float)w[i]);
            return push(h.data(), h.size() * 2);
        }
        if (prec == PREC_BF16) {
            std::vector<uint16_t> h(w.size());
            for (size_t i = 0; i < w.size(); ++i) {
                float f = (float)w[i];
                uint32_t u;
                std::memcpy(&u, &f, 4);
                u = u + 0x7fffu + ((u >> 16) & 1u);     // round to nearest even (weights are finite)
                h[i] = (uint16_t)(u >> 16);
            }
            return push(h.data(), h.size() * 2);
        }
        // fp32 parity mode: the split-f16 operand of mfma_common.h (RawS): per 8 consecutive k of a
        // row (rows are whole 32-k steps), the 8 hi parts f16(w) then the 8 lo parts f16(w - hi),
        // w * 2^sw rounded to f32 first (the f32 weight the exact-product path used, times the power of
        // two that brings the matrix into the split's window: range_weight_exp)
        // (rows are whole 32-k steps, so w.size() is a multiple of 8; a partial last group would be
        // zero-padded to 8, never written past the buffer)
        const double scale = std::ldexp(1.0, sw);
        std::vector<uint16_t> h((w.size() + 7) / 8 * 16, 0);
        for (size_t g = 0; g < w.size(); g += 8)
            for (size_t i = 0; i < 8 && g + i < w.size(); ++i) {
                const float f = (float)(w[g + i] * scale);
                const uint16_t hi = f32_to_f16(f);
                h[2 * g + i] = hi;
                h[2 * g + 8 + i] = f32_to_f16(f - f16_to_f32(hi));   // exact difference in f32
            }
        return push(h.data(), h.size() * 2);
    }
    size_t push_f(const std::vector<float> &v) { return push(v.data(), v.size() * 4); }
};

void bn_fold(const UnitDesc &u, std::vector<double> &scale, std::vector<double> &shift) {
    scale.resize(u.cout);
    shift.resize(u.cout);
    for (int c = 0; c < u.cout; ++c) {
        const double s = (double)u.gamma[c] / std::sqrt((double)u.var[c] + (double)u.eps);
        scale[c] = s;
        shift[c] = ((double)u.b[c] - (double)u.mean[c]) * s + (double)u.beta[c];
    }
}

int gentry(int dy, int dx, int coff) { return (dy & 0xff) | ((dx & 0xff) << 8) | (coff << 16); }

// fp32 mode range scaling: the weight exponent of the packed matrix and its rows' bound terms
// (bugseg_internal.h RangeArgs). w: the folded [Npad][Kpad] matrix; bias / slope per row.
void range_stats(Packed &p, bool scaled, const std::vector<double> &w, const std::vector<float> &bias,
                 const std::vector<float> &slope) {
    p.sw = 0;
    p.rabs.assign(p.Npad, 0.f);
    p.rbias.assign(p.Npad, 0.f);
    p.rslope.assign(p.Npad, 1.f);
    double mx = 0;
    for (int r = 0; r < p.Npad; ++r) {
        double sa = 0;
        for (int k = 0; k < p.Kpad; ++k) {
            const double v = std::fabs(w[(size_t)r * p.Kpad + k]);
            sa += v;
            mx = std::max(mx, v);
        }
        p.rabs[r] = (float)sa;
        p.rbias[r] = std::fabs(bias[r]);
        p.rslope[r] = std::max(1.f, std::fabs(slope[r]));
    }
    if (scaled) p.sw = range_weight_exp(mx);
}

// Ordinary convolution (OIHW weights) on an NHWC input with CinS storage channels.
Packed pack_conv(Packer &pk, const UnitDesc &u, int CinS, const std::vector<float> *slope2) {
    Packed p;
    const int taps = u.kh * u.kw, CG = CinS / 8;
    const int Kgroups = taps * CG;
    p.Ksteps = (Kgroups + 3) / 4;
    p.Kpad = p.Ksteps * 32;
    p.cout = u.cout;
    p.coutP = round_up(u.cout, 16);
    p.nr = pow2_nr(p.coutP);
    p.Npad = p.nr * 16;
    p.CinS = CinS;
    p.stride = u.stride;
    p.macs_per_px = (double)u.cout * u.cin * taps;
    std::vector<double> scale, shift;
    bn_fold(u, scale, shift);
    std::vector<double> w((size_t)p.Npad * p.Kpad, 0.0);
    for (int co = 0; co < u.cout; ++co)
        for (int ci = 0; ci < u.cin; ++ci)
            for (int ky = 0; ky < u.kh; ++ky)
                for (int kx = 0; kx < u.kw; ++kx) {
                    const int tap = ky * u.kw + kx;
                    w[(size_t)co * p.Kpad + tap * CinS + ci] =
                        (double)u.w[(((size_t)co * u.cin + ci) * u.kh + ky) * u.kw + kx] * scale[co];
                }
    std::vector<int> gt(p.Ksteps * 4, gentry(0, 0, 0xffff));
    for (int g = 0; g < Kgroups; ++g) {
        const int tap = g / CG, ky = tap / u.kw, kx = tap % u.kw;
        gt[g] = gentry(ky * u.dil_h - u.pad_h, kx * u.dil_w - u.pad_w, (g % CG) * 8);
    }
    std::vector<float> bias(p.Npad, 0.f), s1(p.Npad, 0.f), s2(p.Npad, 0.f), ps(p.Npad, 0.f);
    for (int c = 0; c < u.cout; ++c) {
        bias[c] = (float)shift[c];
        s1[c] = u.slope[c];
        if (slope2) s2[c] = (*slope2)[c];
    }
    range_stats(p, pk.range, w, bias, s1);
    p.o_w = pk.push_w(w, p.sw);
    p.o_gtab = pk.push(gt.data(), gt.size() * 4);
    p.o_bias = pk.push_f(bias);
    p.o_s1 = pk.push_f(s1);
    p.o_s2 = pk.push_f(s2);
    p.o_ps = pk.push_f(ps);
    return p;
}

// Two 1x1 convolutions over the same input as ONE launch (the upsampling block's main 1x1 and its
// extension branch's first 1x1, which both read the block input): rows [0, m.cout) are m's,
// rows [m.cout, m.cout + e.cout) e's, each with its own folded BN and slope. Bit-identical per output
// channel to the two separate launches when both pack to the same bias placement.
Packed pack_conv_pair(Packer &pk, const UnitDesc &m, const UnitDesc &e, int CinS) {
    UnitDesc u = m;
    u.cout = m.cout + e.cout;
    u.w.insert(u.w.end(), e.w.begin(), e.w.end());
    u.b.insert(u.b.end(), e.b.begin(), e.b.end());
    auto cat = [](std::vector<float> a, const std::vector<float> &b) { a.insert(a.end(), b.begin(), b.end()); return a; };
    // BN folds per channel (the caller requires m.eps == e.eps)
    u.gamma = cat(m.gamma, e.gamma);
    u.beta = cat(m.beta, e.beta);
    u.mean = cat(m.mean, e.mean);
    u.var = cat(m.var, e.var);
    u.slope = cat(m.slope, e.slope);
    return pack_conv(pk, u, CinS, nullptr);
}

// Stride-2 transposed convolution (IOHW weights) as a 4-phase convolution over the INPUT grid:
// output pixel (2i+a, 2j+b) = sum over taps (dy,dx) of in[i+dy][j+dx] . W[ky = a+pad-2dy][kx = b+pad-2dx]
// (PyTorch/ONNX semantics y = 2i - pad + ky). GEMM row n = phase * coutP + co.
Packed pack_tconv(Packer &pk, const UnitDesc &u, int CinS, std::string &why, int choff = 0) {
    Packed p;
    if (u.stride != 2 || u.kh != u.kw || u.pad_h != u.pad_w) { why = "tconv: only square stride-2 kernels"; return p; }
    const int k = u.kh, pad = u.pad_h;
    if (-2 - 2 * pad + k + u.out_pad != 0) { why = "tconv: output must be exactly 2x the input"; return p; }
    std::vector<int> D;
    for (int d = -3; d <= 3; ++d) {
        bool any = false;
        for (int a = 0; a < 2; ++a) { const int kk = a + pad - 2 * d; any |= kk >= 0 && kk < k; }
        if (any) D.push_back(d);
    }
    // input groups: cstore(u.cin) channels starting at channel `choff` of a CinS-channel tensor
    const int nd = (int)D.size(), taps = nd * nd, CG = round_up(u.cin, 8) / 8;
    const int Kgroups = taps * CG;
    p.Ksteps = (Kgroups + 3) / 4;
    p.Kpad = p.Ksteps * 32;
    p.cout = u.cout;
    p.coutP = round_up(u.cout, 16);
    p.phases = 4;
    p.nr = pow2_nr(4 * p.coutP);
    p.Npad = p.nr * 16;
    if (p.Npad != 4 * p.coutP || p.nr > 8) { why = "tconv: unsupported channel count"; return p; }
    p.CinS = CinS;
    p.stride = 1;
    p.macs_per_px = (double)u.cout * u.cin * k * k;       // per INPUT pixel
    std::vector<double> scale, shift;
    bn_fold(u, scale, shift);
    std::vector<double> w((size_t)p.Npad * p.Kpad, 0.0);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int ty = 0; ty < nd; ++ty)
                for (int tx = 0; tx < nd; ++tx) {
                    const int ky = a + pad - 2 * D[ty], kx = b + pad - 2 * D[tx];
                    if (ky < 0 || ky >= k || kx < 0 || kx >= k) continue;
                    const int tap = ty * nd + tx;
                    for (int co = 0; co < u.cout; ++co)
                        for (int ci = 0; ci < u.cin; ++ci)
                            w[(size_t)((a * 2 + b) * p.coutP + co) * p.Kpad + tap * CG * 8 + ci] =
                                (double)u.w[(((size_t)ci * u.cout + co) * k + ky) * k + kx] * scale[co];
                }
    std::vector<int> gt(p.Ksteps * 4, gentry(0, 0, 0xffff));
    for (int g = 0; g < Kgroups; ++g) {
        const int tap = g / CG;
        gt[g] = gentry(D[tap / nd], D[tap % nd], choff + (g % CG) * 8);
    }
    std::vector<float> bias(p.Npad, 0.f), s1(p.Npad, 0.f), s2(p.Npad, 0.f), ps(p.Npad, 0.f);
    for (int ph = 0; ph < 4; ++ph)
        for (int c = 0; c < u.cout; ++c) {
            bias[ph * p.coutP + c] = (float)shift[c];
            s1[ph * p.coutP + c] = u.slope[c];
        }
    range_stats(p, pk.range, w, bias, s1);
    p.o_w = pk.push_w(w, p.sw);
    p.o_gtab = pk.push(gt.data(), gt.size() * 4);
    p.o_bias = pk.push_f(bias);
    p.o_s1 = pk.push_f(s1);
    p.o_s2 = pk.push_f(s2);
    p.o_ps = pk.push_f(ps);
    return p;
}

// w.blocks and w.ncls (parse_blob) -> w.packed, w.block_convs, w.host_w
bool pack_all(EnetWeights &w, int prec, const Knobs &k, std::string &why) {
    Packer pk{prec, prec == PREC_F32 && k.f32_range, w.host_w};
    int cur_c = 3;
    std::vector<int> down_cin(w.blocks.size(), -1);
    for (size_t bi = 0; bi < w.blocks.size(); ++bi) {
        const BlockDesc &b = w.blocks[bi];
        std::vector<int> ids;
        auto add = [&](const Packed &p) { w.packed.push_back(p); ids.push_back((int)w.packed.size() - 1); };
        auto expect_units = [&](size_t n) { return b.units.size() == n; };
        switch (b.type) {
        case BT_INITIAL: {
            const int cin = b.attrs[0], cconv = b.attrs[1], pk_k = b.attrs[2];
            if (bi != 0 || !expect_units(1) || cin != 3 || cconv + cin > 16 || (pk_k != 2 && pk_k != 3) ||
                b.extra.size() != 6) { why = "initial block malformed"; return false; }
            const UnitDesc &u = b.units[0];
            if (u.cout != cconv || u.cin != cin || u.kh != 3 || u.kw != 3 || u.stride != 2 || u.pad_h != 1 || u.pad_w != 1) {
                why = "initial conv must be 3x3 s2 p1"; return false;
            }
            Packed p = pack_conv(pk, u, 8, nullptr);
            // pool channels [cconv, cconv+cin): BN of the concat as scale + shift, their own slope
            std::vector<float> bias(p.Npad), s1(p.Npad), ps(p.Npad, 0.f);
            std::memcpy(bias.data(), w.host_w.data() + p.o_bias, p.Npad * 4);
            std::memcpy(s1.data(), w.host_w.data() + p.o_s1, p.Npad * 4);
            const std::vector<float> &g = b.extra[0], &be = b.extra[1], &mu = b.extra[2], &va = b.extra[3],
                                     &ep = b.extra[4], &sl = b.extra[5];
            if ((int)g.size() != cin || ep.size() != 1 || (int)sl.size() != cin) { why = "initial extras malformed"; return false; }
            for (int c = 0; c < cin; ++c) {
                const double s = (double)g[c] / std::sqrt((double)va[c] + (double)ep[0]);
                ps[cconv + c] = (float)s;
                bias[cconv + c] = (float)((double)be[c] - (double)mu[c] * s);
                s1[cconv + c] = sl[c];
            }
            std::memcpy(w.host_w.data() + p.o_bias, bias.data(), p.Npad * 4);
            std::memcpy(w.host_w.data() + p.o_s1, s1.data(), p.Npad * 4);
            std::memcpy(w.host_w.data() + p.o_ps, ps.data(), p.Npad * 4);
            p.cout = cconv + cin;
            add(p);
            cur_c = cconv + cin;
            break;
        }
        case BT_DOWN: {
            const int cin = b.attrs[0], cout = b.attrs[1];
            if (!expect_units(3) || b.extra.size() != 1 || cin != cur_c || cout < cin) { why = "down block malformed"; return false; }
            const UnitDesc &u1 = b.units[0], &u2 = b.units[1], &u3 = b.units[2];
            if (u1.kh != 2 || u1.kw != 2 || u1.stride != 2 || u1.cin != cin || u2.stride != 1 || u3.kh != 1 ||
                u3.kw != 1 || u3.cout != cout || (int)b.extra[0].size() != cout) { why = "down block units malformed"; return false; }
            add(pack_conv(pk, u1, cstore(cin), nullptr));
            add(pack_conv(pk, u2, cstore(u1.cout), nullptr));
            add(pack_conv(pk, u3, cstore(u2.cout), &b.extra[0]));
            down_cin[bi] = cin;
            cur_c = cout;
            break;
        }
        case BT_REGULAR: {
            const int ch = b.attrs[0];
            if ((b.units.size() != 3 && b.units.size() != 4) || b.extra.size() != 1 || ch != cur_c) {
                why = "regular block malformed"; return false;
            }
            int c = ch;
            for (size_t i = 0; i < b.units.size(); ++i) {
                const UnitDesc &u = b.units[i];
                if (u.kind != 0 || u.cin != c || u.stride != 1) { why = "regular block unit chain malformed"; return false; }
                const bool last = i + 1 == b.units.size();
                add(pack_conv(pk, u, cstore(c), last ? &b.extra[0] : nullptr));
                c = u.cout;
            }
            if (c != ch || (int)b.extra[0].size() != ch) { why = "regular block must preserve channels"; return false; }
            break;
        }
        case BT_UP: {
            const int cin = b.attrs[0], cout = b.attrs[1], ref = b.attrs[2];
            if (!expect_units(4) || b.extra.size() != 1 || cin != cur_c || ref < 0 || ref >= (int)bi ||
                w.blocks[ref].type != BT_DOWN || down_cin[ref] != cout) { why = "up block malformed"; return false; }
            const UnitDesc &um = b.units[0], &u1 = b.units[1], &ut = b.units[2], &u2 = b.units[3];
            if (um.kh != 1 || um.cout != cout || u1.kh != 1 || ut.kind != 1 || ut.kh != 2 || u2.kh != 1 || u2.cout != cout) {
                why = "up block units malformed"; return false;
            }
            add(pack_conv(pk, um, cstore(cin), nullptr));
            add(pack_conv(pk, u1, cstore(cin), nullptr));
            Packed t = pack_tconv(pk, ut, cstore(u1.cout), why);
            if (!why.empty()) return false;
            add(t);
            add(pack_conv(pk, u2, cstore(ut.cout), &b.extra[0]));
            // ids 4 (and 5): the main 1x1 and the extension 1x1 packed as ONE matrix over the block
            // input (rows: main then extension, each with its own folded BN and slope). Used by the
            // fused upsampling kernel (up_kernels.hip), or, where that kernel is not built for the
            // shape, as one conv launch whose output the tconv reads from channel cout on (id 5) —
            // that needs a power-of-two count of 16-B chunks per pixel (the conv epilogue's staged
            // stores). Both require the two halves to fold their bias the same way (bias_in_acc).
            const int es = prec_es(prec), mc = cstore(um.cout) + cstore(u1.cout);
            const int chunks = mc * es / 16;
            const int nr_pair = pow2_nr(round_up(um.cout, 16) + round_up(u1.cout, 16));
            auto bias_acc = [](int nr) { return nr < 8; };     // mfma_common.h bias_in_acc
            const bool same_bias = bias_acc(pow2_nr(round_up(um.cout, 16))) && bias_acc(pow2_nr(round_up(u1.cout, 16)));
            if (um.cout % 16 == 0 && u1.cout % 16 == 0 && um.eps == u1.eps && same_bias) {
                add(pack_conv_pair(pk, um, u1, cstore(cin)));
                if ((chunks & (chunks - 1)) == 0 && nr_pair <= 8 && bias_acc(nr_pair) && !k.no_pair) {
                    Packed t2 = pack_tconv(pk, ut, mc, why, cstore(um.cout));
                    if (!why.empty()) return false;
                    add(t2);
                }
            }
            cur_c = cout;
            break;
        }
        case BT_FULLCONV: {
            if (!expect_units(1) || bi + 1 != w.blocks.size()) { why = "fullconv must be the last block"; return false; }
            const UnitDesc &u = b.units[0];
            if (u.kind != 1 || u.cin != cur_c || u.cout != w.ncls || u.cout > 16) { why = "fullconv malformed"; return false; }
            Packed t = pack_tconv(pk, u, cstore(cur_c), why);
            if (!why.empty()) return false;
            if (t.coutP != 16) { why = "fullconv: classes must fit 16"; return false; }
            add(t);
            cur_c = u.cout;
            break;
        }
        default:
            why = "unknown block type";
            return false;
        }
        w.block_convs.push_back(ids);
    }
    if (w.blocks.empty() || w.blocks.back().type != BT_FULLCONV) { why = "model must end in fullconv"; return false; }
    return true;
}

}  // namespace

bool bugseg::build_weights(const void *blob, size_t bytes, int prec, const Knobs &k, EnetWeights &out, std::string &why) {
    out = EnetWeights();
    why.clear();        // (pack_all reads a non-empty why as pack_tconv's refusal)
    return parse_blob(blob, bytes, out.blocks, out.ncls, why) && pack_all(out, prec, k, why);
}
