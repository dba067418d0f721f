// bugseg host runtime: the native engine behind include/bugseg.h.
//
// Replaces what the reference gets from the TensorFlow C++ runtime (GraphDef import + Session
// executor, models.py:21-44) and from OpenCV (resize / warpPerspective / morphology / resize-NN,
// models.py:87-89, bev.py:182-212):
//   * uploads the parsed and packed BSG1 weight blob (enet_weights.h) in ONE device allocation;
//   * expands the ENet block list into a launch plan per (B, H, W): one fused conv launch per
//     convolution (89 for canonical ENet), ping-pong activation buffers + per-downsample pooling
//     indices carved from ONE device arena, sized for the batch (HBM is 288 GB: the arena for
//     B=64 at 640x480 is a few GB and stays resident between calls);
//   * enqueues on the caller's stream; no host synchronisation, no allocation once a plan exists.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <variant>

#include "bugseg_internal.h"
#include "enet_weights.h"
#include "bev_runtime.h"
#include "../../include/bugseg.h"

using namespace bugseg;

// ---- launch-path caches (bugseg_internal.h)
namespace {
std::mutex g_occ_mu;
struct OccKey { int dev; const void *f; int threads; size_t lds; int val; };
std::vector<OccKey> g_occ;          // val: resident workgroups per CU; f == nullptr: the CU count
int current_device() {
    int d = 0;
    return hipGetDevice(&d) == hipSuccess ? d : 0;
}
}  // namespace
int bugseg::device_cus() {
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(g_occ_mu);
    for (const OccKey &k : g_occ)
        if (k.dev == dev && !k.f) return k.val;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    g_occ.push_back({dev, nullptr, 0, 0, n});
    return n;
}
int bugseg::occupancy_per_cu(const void *f, int threads, size_t lds) {
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(g_occ_mu);
    for (const OccKey &k : g_occ)
        if (k.dev == dev && k.f == f && k.threads == threads && k.lds == lds) return k.val;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, threads, lds) != hipSuccess || n < 0) n = 0;
    g_occ.push_back({dev, f, threads, lds, n});
    return n;
}
hipError_t bugseg::allow_dynamic_lds(const void *f) {
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(g_occ_mu);
    for (const OccKey &k : g_occ)
        if (k.dev == dev && k.f == f && k.threads == -1) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) g_occ.push_back({dev, f, -1, 0, 1});
    return e;
}

// ---- the one reader of the BUGSEG_* behaviour knobs (knobs.h) and their dump; deeplab_runtime.cpp calls them too
bool bugseg::read_knobs(Knobs &k, std::string &err) {
    k = Knobs();
    auto read = [&](const char *var, int &field, long lo, long hi) {
        const char *v = std::getenv(var);
        if (!v || !*v) return true;
        char *end = nullptr;
        const long n = std::strtol(v, &end, 10);
        const bool ok = (*v == '-' || (*v >= '0' && *v <= '9')) && !*end && n >= lo && n <= hi && !(&field == &k.bev_f && n == 3);
        if (ok) field = (int)n;
        else err = std::string(var) + "=" + v + ": not a decimal integer this knob takes (" + std::to_string(lo) + " to " + std::to_string(hi) + ")";
        return ok;
    };
#define X(name, field, def, lo, hi) if (!read("BUGSEG_" #name, k.field, lo, hi)) return false;
    BUGSEG_KNOBS(X)
#undef X
    return true;
}
int bugseg::dump_knobs(const Knobs *k, char *buf, int len, std::string &err) {
    Knobs now;
    if (!k && !read_knobs(now, err)) return BUGSEG_EINVAL;
    if (!k) k = &now;
    std::string s;
#define X(name, field, def, lo, hi) s += "BUGSEG_" #name "=" + std::to_string(k->field) + "\n";
    BUGSEG_KNOBS(X)
#undef X
    if (!buf || len <= (int)s.size()) {
        err = "the knob dump needs a buffer of " + std::to_string(s.size() + 1) + " bytes";
        return BUGSEG_EINVAL;
    }
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return BUGSEG_OK;
}

namespace {

thread_local std::string g_thread_err;

// One kernel launch of the plan: which launch_* it goes to, that call's dispatch arguments and its argument
// struct. Everything but span and rev (issue) and the forward's bindings (bind) is final once the plan is built.
struct ConvLaunch {    // launch_conv: the unfused convolutions, the initial block, the class layer
    int nr = 0, epi = 0;
    bool cls = false;  // the class layer's route: the class kernel (cls_kernels.hip), not the generic EPI_CLASSES
                       // convolution (Knobs::cls_conv, or a shape the class kernel does not take)
    ConvArgs a{};
};
struct BneckLaunch {   // launch_bneck: a fused bottleneck; cin > 0: a downsampling block (cin input channels)
    int C = 0, var = 0, cin = 0;
    bool asym = false;
    bool win = false;  // the row-windowed fp32 C = 128 kernels (BneckArgs::oy_end)
    bool cls = false;  // launch_bneck_cls: the C = 16 block with the class layer fused in (Plan::cls_fused)
    BneckArgs a{};
};
struct UpLaunch {      // launch_up: a fused upsampling block
    int cin = 0, it = 0, cout = 0;
    UpArgs a{};
};
using Launch = std::variant<ConvLaunch, BneckLaunch, UpLaunch>;

// A plan op: its full-frame launch and its accounting. Immutable between build_plan calls: a forward's input and
// output (Binding) and a row window (WinPlan) go into a copy of the launch, never into the plan.
// l is the plan's own launch, which bugseg_plan_info / _op / _launch_op describe and run; fwd is the launch as a
// forward issues it outside a whole pair, on the buffers the pair overlay leaves it (build_pairs; without pairs: l).
struct Op {
    Launch l, fwd;
    double bytes = 0, flops = 0;
    double layer_bytes = -1;   // per-layer (unfused) algorithmic bytes of the work; -1: same as bytes
    int launches = 1;          // kernel launches the op issues (every form today: one)
    int pos = 0;               // launches the plan issues before this op (build_plan): its walk direction's parity
    int fwd_odd = 0;           // that parity in a forward (build_pairs): a pair is one launch where the plan counts two
    double layer() const { return layer_bytes >= 0 ? layer_bytes : bytes; }
    const ConvLaunch *conv() const { return std::get_if<ConvLaunch>(&l); }
    const BneckLaunch *bneck() const { return std::get_if<BneckLaunch>(&l); }
    const UpLaunch *up() const { return std::get_if<UpLaunch>(&l); }
    // a fused regular bottleneck (3x3, undilated, one phase) of C channels on an h-row grid
    bool regular(int C, int h) const {
        const BneckLaunch *b = bneck();
        return b && b->C == C && !b->asym && b->cin == 0 && b->a.dt == 1 && b->a.phases == 1 && b->a.H == h;
    }
    bool up_on(int h) const { return up() && up()->a.h == h; }          // a fused upsampling block reading an h-row grid
    bool epi(int e) const { return conv() && conv()->epi == e; }
    // the class layer as the class kernel runs it (ConvLaunch::cls)
    bool class_kernel() const { return conv() && conv()->cls; }
};

// What one forward binds into the plan's first and last launch (bind): the input and its kind, the output and its kind.
struct Binding {
    const void *in = nullptr;
    bool bgr = false;
    int out_kind = 0; void *out = nullptr;
};

// Row-windowed decoder (bugseg_enet_forward_bgr_rows): the rows each of the plan's last WIN_OPS ops runs
// when only class rows [row0, row1) are wanted — in plan order the 128 -> 64 upsampling block, the two
// stage-4 bottlenecks, the 64 -> 16 upsampling block, the stage-5 bottleneck and the class layer. y0, y1:
// rows of the op's own grid, input rows for the upsampling blocks and the class layer (pointwise in their
// input grid), output rows for the bottlenecks; a bottleneck also carries the tile form picked for its
// window (pick_bneck_variant over the window's rows). l: the op's finished windowed launch (narrow), built
// once with the window; launch_op only picks it.
constexpr int WIN_OPS = 6;
struct WinOp { int y0 = 0, y1 = 0, var = 0, tr = 0, te = 1, tiles_x = 0, tiles_y = 0; Launch l; };   // te: image rows per tile row
// The walk goes on into stage 3 (stage3_windows): s3[k] is the window of the (k + 1)-th op before those six, a
// fused fp32 C = 128 bottleneck in its windowed form (launch_bneck win = true), for k < ns3 <= S3_OPS. y0, y1:
// output rows; tiles_y: tile rows per frame (a row-dilated form: of its longest row phase).
constexpr int S3_OPS = 2;
struct WinPlan {
    int row0 = 0, row1 = 0; WinOp op[WIN_OPS]; int ns3 = 0; WinOp s3[S3_OPS];
    // the windowed launch of op i of an n-op plan; null: the op runs its full-frame launch
    const Launch *launch_of(int i, int n) const {
        const int k = i - (n - WIN_OPS);
        return k >= 0 ? &op[k].l : -k - 1 < ns3 ? &s3[-k - 1].l : nullptr;
    }
};

// ---- the pair overlay (bneck_pair_kernels.hip). The plan keeps one op per block; a forward runs ops
// i and i + 1 as one paired launch where the overlay has a pair (i, i + 1) and both lie in the forward's op range.
// pair_firsts and pair_actions are the whole rule: build_pairs turns them into finished launches when the plan is
// built, enet_forward switches on the actions of its op range, and bugseg_debug_pair_walk shows the same two to the
// tests. A forced tile variant (BUGSEG_BNECK_VARIANT, BUGSEG_BNECK_VARIANT_C64) or BUGSEG_NO_FUSE=1 plans without it.
// What the walk needs of an op: ok — a fused fp32 C = 64 regular d = 1 bottleneck on an h x w grid in an untransposed
// form, before the row-windowed decoder ops; in, out — which of the arena's two activation buffers it reads and
// writes (0, 1; -1: another buffer).
struct PairCand { bool ok = false; int h = 0, w = 0, in = -1, out = -1; };
// The pairs' first ops: left to right, op i with op i + 1 when both are candidates on one grid, i + 1 reads what i
// writes and writes the buffer i reads (the arena's ping-pong).
std::vector<int> pair_firsts(const std::vector<PairCand> &c) {
    std::vector<int> f;
    for (size_t i = 0; i + 1 < c.size(); ++i) {
        const PairCand &p = c[i], &q = c[i + 1];
        if (p.ok && q.ok && p.h == q.h && p.w == q.w && p.in >= 0 && p.out >= 0 && p.in != p.out && q.in == p.out && q.out == p.in) {
            f.push_back((int)i);
            ++i;
        }
    }
    return f;
}
// What each op of an n-op plan does in a forward over ops [first_op, last_op), and where. A paired launch reads
// x where op i would and writes where op i would (the buffer of the tensor it skips), so everything after a pair
// lives in the other buffer than the plan says: flip[k] = 1. A pair cut by the op range runs as its two plain
// launches through a spare buffer — the first writes it, the second reads it and writes where the pair would — so
// where every tensor lives does not depend on how a forward was cut into calls.
enum { PA_PLAIN = 0, PA_PAIR = 1, PA_SKIP = 2, PA_LONE_FIRST = 3, PA_LONE_SECOND = 4 };
void pair_actions(int n, const std::vector<int> &firsts, int first_op, int last_op, int *act, int *flip) {
    for (int k = 0; k < n; ++k) { act[k] = PA_PLAIN; flip[k] = 0; }
    for (const int i : firsts) {
        if (i < 0 || i + 1 >= n) continue;
        const bool both = first_op <= i && i + 1 < last_op;
        act[i] = both ? PA_PAIR : PA_LONE_FIRST;
        act[i + 1] = both ? PA_SKIP : PA_LONE_SECOND;
        for (int k = i + 2; k < n; ++k) flip[k] ^= 1;
    }
}
// One pair of the overlay: the paired launch, buffers bound, and the guards of the two fallbacks behind it, which run
// the forward launches (Op::fwd) of ops first and first + 1. flip: of op first (pair_actions)
struct PairOp {
    int first = 0, flip = 0;
    BneckPairArgs args{};
    BneckGuardArgs ga{}, gb{};
};

struct Plan {
    int B = 0, H = 0, W = 0;
    std::vector<Op> ops;
    // the pair overlay (build_pairs): the pairs' first ops (pair_firsts), ascending, and pair k's launch
    std::vector<int> firsts;
    std::vector<PairOp> pairs;
    std::vector<WinPlan> wins;   // windowed forms of this plan, by window (window_plan); dropped with the plan
    size_t act_bytes = 0;        // the arena's activation and pool-index part (before the range words)
    float *words = nullptr;  // fp32 mode: RNG_SLOTS range words per measured tensor (block 0: the engine input)
    size_t words_bytes = 0;
    void *arena = nullptr;
    size_t arena_bytes = 0;
    bool pinned = false;     // a forward on this arena was captured into a graph: never freed before destroy
    std::vector<unsigned char *> idx;   // per block: its pooling-index tensor in the arena (down blocks), else null
    std::vector<size_t> idx_bytes;
    // ENet's last bottleneck (C = 16) and the class layer as ONE launch (bneck_kernels.hip, class fusion;
    // opt-in, BUGSEG_CLS_FUSE=1: measured slower, see there): possible for this plan (cls_ok: the plan ends
    // with that bottleneck feeding the class kernel; cls_fused is then that launch, its output unbound, and
    // cls_fused_fwd the same of the two ops' forward launches, Op::fwd), and
    // taken by the last forward (cls_on: a class-map output, both ops in its range). The last op then launches
    // nothing; its plan_op tag is "fused".
    bool cls_ok = false, cls_on = false;
    Launch cls_fused, cls_fused_fwd;
    Binding bound;           // the last forward's binding (in == nullptr: none since the plan was built)
    // A context's plan is a complete plan for its (B, H, W) or Plan(), never a mixture (build_plan)
    bool empty() const { return !arena; }
    bool at(int b, int h, int w) const { return arena && B == b && H == h && W == w; }
};

}  // namespace

struct bugseg_ctx {
    bugseg_ctx(const Knobs &k, int device) : knobs(k), mem(device) {}
    const Knobs knobs;                             // the BUGSEG_* knobs as bugseg_create read them (knobs.h)
    int prec = PREC_F32;
    float naff[6] = {};                            // exact affine form of the normalisation table (find_affine)
    bool naff_on = false;                          // ... found (never searched for under Knobs::init_table)
    float norm_amax = 0.f;                         // max |table| (the BGR input's range, fp32 range scaling)
    unsigned long long *spans = nullptr;           // bugseg_debug_set_spans: 512 u64 of launch-span slots per op, or null
    int spans_ops = 0;                             // ... for ops [0, spans_ops) only (the caller's buffer size)
    std::string err;
    // the model: the blob parsed and packed (enet_weights.h) and the device copy of its staging image, installed
    // together by bugseg_load_weights; loaded == false: w is empty and dev_w null
    bool loaded = false;
    EnetWeights w;
    void *dev_w = nullptr;
    void *dev_luts = nullptr;                      // [0..15] lut3, [16..31] binary, then 3x256 f64 norm lut
    Plan plan;
    CtxMemory mem;                                 // the device, the setup stream, the graveyard (ctx_memory.h)
    struct NoPayload {};
    TableCache<std::array<int, 4>, NoPayload> pre_tabs;   // preprocess resize tables (mode 2) by (H0, W0, H, W)
    BevState bev;                                  // the BEV rasteriser's tables and scratch (bev_runtime.cpp)
    void *clahe_tabs = nullptr;                    // clahe_kernels.hip's conversion tables (ctx_clahe_tables)
};

namespace {

int fail(bugseg_ctx *c, int code, const std::string &m) {
    if (c) c->err = m;
    else g_thread_err = m;
    return code;
}

// ---------------------------------------------------------------- plan
struct Shape { int H, W, C; };   // C = storage channels

ConvArgs base_args(const bugseg_ctx *ctx, const Packed &p) {
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    const unsigned char *d = (const unsigned char *)ctx->dev_w;
    a.Ksteps = p.Ksteps;
    a.Kpad = p.Kpad;
    a.Npad = p.Npad;
    a.w = d + p.o_w;
    a.gtab = (const int *)(d + p.o_gtab);
    a.bias = (const float *)(d + p.o_bias);
    a.slope1 = (const float *)(d + p.o_s1);
    a.slope2 = (const float *)(d + p.o_s2);
    a.pscale = (const float *)(d + p.o_ps);
    a.stride = p.stride;
    a.CinS = p.CinS;
    a.coutP = p.coutP;
    return a;
}

// Every PReLU slope (both slope vectors) of the packed units is <= 1: max(v, s*v) is then exact
bool slopes_le1(const bugseg_ctx *ctx, std::initializer_list<const Packed *> units) {
    for (const Packed *p : units) {
        const float *s1 = (const float *)(ctx->w.host_w.data() + p->o_s1), *s2 = (const float *)(ctx->w.host_w.data() + p->o_s2);
        for (int c = 0; c < p->Npad; ++c)
            if (!(s1[c] <= 1.f) || !(s2[c] <= 1.f)) return false;
    }
    return true;
}

// A regular block runs as ONE fused launch (bneck_kernels.hip) when its shape is one the fused
// kernel is built for and a tile variant covers the layer efficiently (pick_bneck_variant);
// otherwise as its 3-4 conv launches. BUGSEG_NO_FUSE=1 forces the unfused plan (A/B testing;
// results are bit-identical).
bool fusable_regular(const bugseg_ctx *ctx, const BlockDesc &b, const std::vector<int> &ids, int &r, int &d) {
    if (ctx->knobs.no_fuse) return false;
    // the fused kernel computes PReLU as max(v, s*v), exact only for slopes <= 1
    for (const int id : ids)
        if (!slopes_le1(ctx, {&ctx->w.packed[id]})) return false;
    const int C = b.attrs[0];
    if (C != 128 && C != 64 && C != 16) return false;
    const int nu = (int)b.units.size();
    const UnitDesc &u1 = b.units[0], &u3 = b.units[nu - 1];
    if (u1.kh != 1 || u1.kw != 1 || u1.cout != C / 4 || u3.kh != 1 || u3.kw != 1 || u3.cin != C / 4) return false;
    if (nu == 4) {
        const UnitDesc &a = b.units[1], &c = b.units[2];
        if (a.kh != 5 || a.kw != 1 || a.pad_h != 2 || a.pad_w != 0 || a.dil_h != 1 ||
            c.kh != 1 || c.kw != 5 || c.pad_h != 0 || c.pad_w != 2 || c.dil_w != 1 || a.cout != C / 4 || c.cout != C / 4)
            return false;
        r = 2; d = 1;
    } else {
        const UnitDesc &m = b.units[1];
        if (m.kh != 3 || m.kw != 3 || m.dil_h != m.dil_w || m.pad_h != m.dil_h || m.pad_w != m.dil_w || m.cout != C / 4)
            return false;
        d = m.dil_h;
        r = 1;
    }
    return true;
}

// The downsampling block in one fused launch (bneck_kernels.hip, cin > 0): ENet's two shapes
// (16 -> 64, 64 -> 128, internal cin / 4), 2x2 stride-2 projection, 3x3 middle conv, PReLU slopes
// <= 1. -> the tile variant (C64: 16x16, C128: 20x16, untransposed) or -1.
int fusable_down(const bugseg_ctx *ctx, const BlockDesc &b, const std::vector<int> &ids) {
    if (ctx->knobs.no_fuse) return -1;
    const int cin = b.attrs[0], C = b.attrs[1];
    const int v = C == 64 && cin == 16 ? 0 : C == 128 && cin == 64 ? 1 : -1;
    if (v < 0 || b.units.size() != 3) return -1;
    for (const int id : ids)
        if (!slopes_le1(ctx, {&ctx->w.packed[id]})) return -1;
    const UnitDesc &u1 = b.units[0], &u2 = b.units[1], &u3 = b.units[2];
    const int I = cin / 4;                              // ENet: internal = input channels / 4
    if (u1.kh != 2 || u1.kw != 2 || u1.stride != 2 || u1.pad_h != 0 || u1.pad_w != 0 || u1.cin != cin || u1.cout != I)
        return -1;
    if (u2.kh != 3 || u2.kw != 3 || u2.stride != 1 || u2.pad_h != 1 || u2.pad_w != 1 || u2.dil_h != 1 || u2.dil_w != 1 ||
        u2.cin != I || u2.cout != I)
        return -1;
    if (u3.kh != 1 || u3.kw != 1 || u3.cin != I || u3.cout != C) return -1;
    if (bneck_slots_per_cu(ctx->knobs, ctx->prec, C, false, v, false, cin) <= 0) return -1;
    return v;
}

// Tile variant of a fused bottleneck layer: the variant whose estimated time is least, where a
// launch costs (rounds of resident workgroups) x (per-tile cost) and the per-tile cost is the
// per-wave fragment count of the two tile phases (weights from in-kernel phase clocks of the 16x16
// C128 tile, scripts/stamp_probe.py: ~3.8k cycles per halo fragment per wave in the projection,
// ~7.5k per tile fragment per wave in the middle conv + expansion, ~4.5k fixed). Returns -1 when no
// variant keeps at least 60 % of the computed tile pixels inside the image (large dilations on small
// feature maps: the unfused launches are cheaper). BUGSEG_BNECK_VARIANT forces a variant.
int pick_bneck_variant(const bugseg_ctx *ctx, int C, bool asym, int d, int B, int H, int W, int &tiles_y, int &tiles_x,
                       int &tr, int &rdv) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->mem.device) != hipSuccess || cus <= 0) cus = 256;
    const Knobs &k = ctx->knobs;
    int force = k.bneck_variant;                                           // -1: none
    const int fc = C == 128 ? k.bneck_variant_c128 : C == 64 ? k.bneck_variant_c64 : C == 16 ? k.bneck_variant_c16 : -1;
    if (fc >= 0) force = fc;                                               // debug
    if (asym && k.bneck_variant_asym >= 0) force = k.bneck_variant_asym;   // debug
    const int R = asym ? 2 : 1;
    const int hs = (H + d - 1) / d, ws = (W + d - 1) / d;    // phase sub-image (largest phase)
    int best = -1;
    double best_cost = 0;
    for (int v = 0; v < bneck_variants(C); ++v) {
        int th, tw, nw, rd;
        bneck_shape(C, v, th, tw, nw, &rd);
        if (bneck_lds_bytes(ctx->prec, C, asym, v) > 160 * 1024) continue;
        if (rd && (asym || W > tw || d < 2)) continue;        // row-dilated tiles span the width
        const bool forced = force == v;
        for (int t = 0; t < (asym || rd ? 1 : 2); ++t) {
            const int spc = bneck_slots_per_cu(k, ctx->prec, C, asym, v, t != 0);
            if (spc <= 0) continue;                           // this orientation is not built
            const int slots = spc * cus;
            const int ty = rd ? (hs + th - 1) / th : t ? (hs + tw - 1) / tw : (hs + th - 1) / th;
            const int tx = rd ? 1 : t ? (ws + th - 1) / th : (ws + tw - 1) / tw;
            const double ntiles = (double)B * (rd ? d : d * d) * ty * tx;
            const double eff = (double)H * W / (ntiles / B * th * tw);
            const double nf1 = std::ceil((th + 2.0 * R) * (tw + (rd ? 0.0 : 2.0 * R)) / 16.0), nft = std::ceil(th * tw / 16.0);
            double tile = 3.8 * std::ceil(nf1 / nw) + 7.5 * std::ceil(nft / nw) + 4.5;
            // 2-byte C = 64: a form that re-reads its residual pays for it (PMC, round 6, B = 64: 20 x 16 reads
            // 1.45x its compulsory bytes and runs 71.8 us against 70.9 for the kept 16 x 16 form)
            if (C == 64 && !asym && ctx->prec != PREC_F32 && bneck_keeps_c64(ctx->prec, 0) && !bneck_keeps_c64(ctx->prec, v))
                tile *= 1.15;
            const double cost = std::ceil(ntiles / slots) * tile;
            if (!forced && eff < 0.6) continue;
            if (best < 0 || (forced && best != v) || cost < best_cost) {
                best = v; best_cost = cost; tiles_y = ty; tiles_x = tx; tr = t; rdv = rd;
            }
        }
        if (forced && best == v) break;
    }
    return best;
}

// Walk the network for (B, H, W), twice: run(false) computes only the buffer sizes, run(true), with the arena
// carved, the ops. run dispatches to one method per block type; wire / slopes_le1 / sums are what those share.
// Of the plan under construction (build_plan's local) the size pass fills idx_bytes and the second pass ops, from
// the idx and words build_plan carved in between.
struct Walker {
    const bugseg_ctx *ctx;
    Plan &pl;
    int B, H, W;
    size_t es;
    // buffer sizes (bytes) and pointers
    size_t szX = 0, szT = 0, szM = 0;
    unsigned char *X[2] = {nullptr, nullptr}, *T[3] = {nullptr, nullptr, nullptr}, *Mb = nullptr;
    // fp32 mode range scaling (bugseg_internal.h RangeArgs): RNG_SLOTS words per measured tensor (Plan::words), block
    // 0 for the engine input; which block holds the range of each buffer's current contents
    int nwords = 1;
    std::vector<std::pair<const void *, float *>> wmap;
    static int max_words(size_t nblocks) { return (int)(4 * nblocks + 4); }
    float *take_words() {
        float *w = pl.words && es == 4 ? pl.words + (size_t)nwords * RNG_SLOTS : nullptr;
        ++nwords;
        return w;
    }
    void wrote(const void *buf, float *w) {
        for (auto &e : wmap)
            if (e.first == buf) { e.second = w; return; }
        wmap.push_back({buf, w});
    }
    float *words_of(const void *buf) const {
        if (es != 4) return nullptr;
        if (!buf) return pl.words;                          // the engine input
        for (const auto &e : wmap)
            if (e.first == buf) return e.second;
        return nullptr;
    }

    size_t tbytes(const Shape &s) const { return (size_t)B * s.H * s.W * s.C * es; }

    // ---- the walk's state, shared by the block methods: the pass, the current activation (curp == nullptr: the
    // engine input, bound per call), the index of the block being walked, its packed units and its output buffer
    bool fill = false;
    Shape cur{0, 0, 0};
    const unsigned char *curp = nullptr;
    size_t bi = 0;
    const std::vector<int> *ids = nullptr;
    unsigned char *dst = nullptr;
    const Packed &P(int i) const { return ctx->w.packed[(size_t)(*ids)[(size_t)i]]; }
    static ConvArgs &args(Op &op) { return std::get<ConvLaunch>(op.l).a; }
    static uint32_t clamp31(size_t v) { return (uint32_t)std::min<size_t>(v, 0x7fffffff); }

    // a packed unit's weights, bias and first slope vector on the device; its second slope vector
    void wire(const Packed &p, const void *&w, const float *&b, const float *&s) const {
        const unsigned char *dw = (const unsigned char *)ctx->dev_w;
        w = dw + p.o_w; b = (const float *)(dw + p.o_bias); s = (const float *)(dw + p.o_s1);
    }
    const float *slope2(const Packed &p) const { return (const float *)((const unsigned char *)ctx->dev_w + p.o_s2); }
    // weight bytes and flops over px GEMM pixels of the block's first n units
    void sums(int n, double px, double &wb, double &fl) const {
        wb = fl = 0;
        for (int i = 0; i < n; ++i) { wb += (double)P(i).Npad * P(i).Kpad * es; fl += 2.0 * P(i).macs_per_px * px; }
    }
    // fp32 range scaling of a launch: its input's measured range; measure: its output's range is measured too
    void range_io(RangeArgs &rg, const void *in, const void *out, bool measure = true) {
        rg.amax_in = words_of(in);
        rg.off = !ctx->knobs.f32_range;
        if (!measure) return;
        rg.amax_out = take_words();
        wrote(out, rg.amax_out);
    }
    static void residual(ConvArgs &a, const void *res, Shape s, int C) {
        a.res = res; a.resH = s.H; a.resW = s.W; a.resC = C; a.resCS = s.C;
    }
    // the units of a fused bottleneck (p2b: the asymmetric block's 1x5, else p2 again)
    void wire_bneck(BneckArgs &q, const Packed &p1, const Packed &p2, const Packed &p2b, const Packed &p3) const {
        wire(p1, q.w1, q.b1, q.s1); wire(p2, q.w2, q.b2, q.s2);
        wire(p2b, q.w2b, q.b2b, q.s2b); wire(p3, q.w3, q.b3, q.s3);
        q.s_out = slope2(p3);
        q.slopes_le1 = slopes_le1(ctx, {&p1, &p2, &p2b, &p3});
        q.rg.sw[0] = p1.sw; q.rg.sw[1] = p2.sw; q.rg.sw[2] = p2b.sw; q.rg.sw[3] = p3.sw;
        row_bound(p1, 0, p1.cout, q.rg.n[0], q.rg.c[0]);
        row_bound(p2, 0, p2.cout, q.rg.n[1], q.rg.c[1]);
    }

    // one convolution launch, appended to ops
    Op &conv(const Packed &p, int epi, const void *in, Shape si, Shape sg, void *out, Shape so) {
        Op op;
        ConvLaunch &l = op.l.emplace<ConvLaunch>();
        l.nr = p.nr; l.epi = epi;
        ConvArgs &a = l.a;
        a = base_args(ctx, p);
        a.in = in; a.B = B; a.Hin = si.H; a.Win = si.W;
        a.Hg = sg.H; a.Wg = sg.W; a.M = B * sg.H * sg.W;
        a.out = out; a.Hout = so.H; a.Wout = so.W; a.outC = so.C;
        a.ntiles = (a.M + conv_tile_pixels(p.nr) - 1) / conv_tile_pixels(p.nr);
        const int epc = 16 / (int)es;
        a.stg_elems = epi == EPI_CLASSES ? 64 * 20 * 4 / (int)es      // 64 pixels x 20 floats (conv_kernels.hip CLS_STR)
                    : epi == EPI_SHUFFLE ? 64 * (so.C + epc) : 16 * (so.C + epc);
        a.slopes_le1 = slopes_le1(ctx, {&p});
        a.rg.sw[0] = p.sw;
        range_io(a.rg, in, out, out && epi != EPI_CLASSES);
        op.flops = 2.0 * p.macs_per_px * a.M;
        op.bytes = (double)B * si.H * si.W * si.C * es + (double)p.Npad * p.Kpad * es +
                   (epi == EPI_CLASSES ? 0.0 : (double)B * so.H * so.W * so.C * es);
        pl.ops.push_back(op);
        return pl.ops.back();
    }

    void initial(const BlockDesc &b) {
        Shape so{H / 2, W / 2, cstore(P(0).cout)};
        szX = std::max(szX, tbytes(so));
        if (fill) {
            ConvArgs &a = args(conv(P(0), EPI_INIT, curp, cur, so, dst, so));
            a.cconv = b.attrs[1]; a.cpool = b.attrs[0]; a.pool_k = b.attrs[2];
            a.pool_scan = ctx->knobs.init_pool_scan;
            a.CinS = 8;
        }
        cur = so;
    }

    void down(const BlockDesc &b) {
        Shape s1{cur.H / 2, cur.W / 2, cstore(P(0).cout)}, s2{s1.H, s1.W, cstore(P(1).cout)};
        Shape so{s1.H, s1.W, cstore(P(2).cout)};
        const int idxCS = cstore(b.attrs[0]);
        szT = std::max({szT, tbytes(s1), tbytes(s2)});
        szX = std::max(szX, tbytes(so));
        if (!fill) pl.idx_bytes[bi] = (size_t)B * so.H * so.W * idxCS;
        const int dv = cur.C == b.attrs[0] ? fusable_down(ctx, b, *ids) : -1;
        const Shape sp{so.H, so.W, idxCS};
        // (sizes T for the pooled-values scratch the fused form had; kept so that the arena's size does not move)
        if (dv >= 0) szT = std::max(szT, tbytes(sp));
        if (fill && dv >= 0) {
            // one launch: 2x2 projection + 3x3 + expansion + pooled main branch (pooled values
            // in registers, as the residual)
            Op op;
            BneckLaunch &l = op.l.emplace<BneckLaunch>();
            l.C = b.attrs[1]; l.var = dv; l.cin = b.attrs[0];
            BneckArgs &q = l.a;
            int th, tw, nw;
            bneck_shape(l.C, dv, th, tw, nw, nullptr);
            q.x = nullptr; q.out = dst; q.B = B; q.H = so.H; q.W = so.W;
            q.dt = 1; q.phases = 1; q.tr = 0;
            q.tiles_y = (so.H + th - 1) / th; q.tiles_x = (so.W + tw - 1) / tw;
            q.ntiles = B * q.tiles_y * q.tiles_x;
            wire_bneck(q, P(0), P(1), P(1), P(2));
            q.xin = curp;                             // (x_bytes: build_plan, as for every fused bottleneck)
            q.xin_bytes = clamp31(tbytes(cur));
            q.idx_out = pl.idx[bi]; q.idxCS = idxCS;
            q.idx_bytes = clamp31((size_t)B * so.H * so.W * idxCS);
            range_io(q.rg, curp, dst);
            const double px = (double)B * so.H * so.W;
            double wb, fl;
            sums(3, px, wb, fl);
            op.flops = fl;
            // x read once, out + indices written once
            op.bytes = (double)tbytes(cur) + (double)tbytes(so) + px * idxCS + wb;
            op.layer_bytes = (double)tbytes(cur) * 2 + 2.0 * (tbytes(s1) + tbytes(s2)) + (double)tbytes(so) +
                             px * idxCS + wb;
            pl.ops.push_back(op);
        } else if (fill) {
            conv(P(0), EPI_PLAIN, curp, cur, s1, T[0], s1);
            conv(P(1), EPI_PLAIN, T[0], s1, s2, T[1], s2);
            Op &o3 = conv(P(2), EPI_RESPOOL, T[1], s2, so, dst, so);
            residual(args(o3), curp, cur, b.attrs[0]);
            args(o3).idx_out = pl.idx[bi]; args(o3).idxCS = idxCS;
            o3.bytes += (double)B * cur.H * cur.W * cur.C * es + (double)B * so.H * so.W * idxCS;
        }
        cur = so;
    }

    void regular(const BlockDesc &b) {
        const int nu = (int)b.units.size();
        int rr = 0, dd = 1, ty = 0, tx = 0, ttr = 0, trd = 0, var = -1;
        if (fusable_regular(ctx, b, *ids, rr, dd))
            var = pick_bneck_variant(ctx, b.attrs[0], nu == 4, dd, B, cur.H, cur.W, ty, tx, ttr, trd);
        if (var >= 0) {
            // one launch: projection + middle conv + expansion + residual, internals in LDS
            szX = std::max(szX, tbytes(cur));
            if (!fill) return;
            Op op;
            BneckLaunch &l = op.l.emplace<BneckLaunch>();
            l.C = b.attrs[0]; l.asym = nu == 4; l.var = var;
            BneckArgs &q = l.a;
            const Packed &p2b = P(nu == 4 ? 2 : 1);
            q.x = curp; q.out = dst; q.B = B; q.H = cur.H; q.W = cur.W;
            q.dt = dd; q.phases = trd ? dd : dd * dd; q.tr = ttr;
            q.tiles_y = ty; q.tiles_x = tx;
            q.ntiles = B * q.phases * ty * tx;
            wire_bneck(q, P(0), P(1), p2b, P(nu - 1));
            row_bound(p2b, 0, p2b.cout, q.rg.n[2], q.rg.c[2]);
            range_io(q.rg, curp, dst);
            const double px = (double)B * cur.H * cur.W;
            double wb, fl, lb = 0;
            sums(nu, px, wb, fl);
            for (int i = 0; i < nu; ++i) lb += px * (cstore(b.units[i].cin) + cstore(b.units[i].cout)) * es;   // layer by layer
            op.flops = fl;
            op.bytes = 2.0 * px * cur.C * es + wb;             // what this launch must move
            op.layer_bytes = lb + px * cur.C * es + wb;        // + the residual re-read
            pl.ops.push_back(op);
            return;
        }
        Shape s = cur;
        const unsigned char *src = curp;
        for (int i = 0; i < nu; ++i) {
            const bool last = i + 1 == nu;
            Shape so{s.H, s.W, cstore(b.units[i].cout)};
            unsigned char *o = last ? dst : T[i % 3];
            if (!last) szT = std::max(szT, tbytes(so));
            else szX = std::max(szX, tbytes(so));
            if (fill) {
                Op &op = conv(P(i), last ? EPI_RESADD : EPI_PLAIN, src, s, so, o, so);
                if (last) {
                    residual(args(op), curp, cur, b.attrs[0]);
                    op.bytes += (double)B * cur.H * cur.W * cur.C * es;
                }
            }
            s = so;
            src = o;
        }
        cur = s;
    }

    void up(const BlockDesc &b) {
        const int ref = b.attrs[2];
        Shape sm{cur.H, cur.W, cstore(P(0).cout)}, s1{cur.H, cur.W, cstore(P(1).cout)};
        Shape st{cur.H * 2, cur.W * 2, cstore(P(2).cout)}, so{cur.H * 2, cur.W * 2, cstore(P(3).cout)};
        szM = std::max(szM, tbytes(sm));
        szT = std::max({szT, tbytes(s1), tbytes(st)});
        szX = std::max(szX, tbytes(so));
        const int cin_b = b.attrs[0], cout_b = b.attrs[1], it_b = P(1).cout;
        const int idxCS = cstore(ctx->w.blocks[(size_t)ref].attrs[0]);
        const bool fuse_up = ids->size() >= 5 && up_supported(cin_b, it_b, cout_b) && cur.C == cin_b && so.C == cout_b && !ctx->knobs.no_fuse;
        const bool pair = ids->size() == 6;
        // unfused, paired: the main and extension 1x1 outputs share one tensor (main channels first)
        Shape sp{cur.H, cur.W, pair ? sm.C + s1.C : sm.C};
        if (!fuse_up) szM = std::max(szM, tbytes(sp));
        if (fill && fuse_up) {
            // one launch: x read once, out written once, everything else in registers
            Op op;
            UpLaunch &l = op.l.emplace<UpLaunch>();
            l.cin = cin_b; l.it = it_b; l.cout = cout_b;
            UpArgs &q = l.a;
            const Packed &p1 = P(4), &p2 = P(2), &p3 = P(3);
            q.x = curp; q.idx = pl.idx[(size_t)ref]; q.out = dst;
            q.M = B * cur.H * cur.W; q.h = cur.H; q.w = cur.W;
            q.y0 = 0; q.hwin = cur.H;                 // the full frame (narrow: a window)
            q.idxCS = idxCS;
            fastdiv((uint32_t)(cur.H * cur.W), q.mHW, q.sHW);
            fastdiv((uint32_t)cur.W, q.mW, q.sW);
            wire(p1, q.w1, q.b1, q.s1);
            wire(p2, q.w2, q.b2, q.s2);
            wire(p3, q.w3, q.b3, q.s3);
            q.s_out = slope2(p3);
            q.slopes_le1 = slopes_le1(ctx, {&p1, &p2, &p3});
            q.rg.sw[0] = p1.sw; q.rg.sw[1] = p2.sw; q.rg.sw[2] = p3.sw;
            row_bound(p1, cout_b, cout_b + it_b, q.rg.n[0], q.rg.c[0]);   // the pair's e1 rows
            row_bound(p2, 0, p2.Npad, q.rg.n[1], q.rg.c[1]);
            range_io(q.rg, curp, dst);
            q.x_bytes = clamp31(tbytes(cur));
            q.idx_bytes = clamp31((size_t)B * cur.H * cur.W * idxCS);
            q.out_bytes = clamp31(tbytes(so));
            const double px = (double)B * cur.H * cur.W;
            double wb, fl;
            sums(4, px, wb, fl);
            op.flops = fl;
            op.bytes = px * cur.C * es + px * idxCS + 4.0 * px * so.C * es + wb;   // x + idx in, out
            op.layer_bytes = px * cur.C * es * 2 + px * (sm.C + s1.C) * es + px * s1.C * es + 4.0 * px * st.C * es * 2 +
                             px * sm.C * es + px * idxCS + 4.0 * px * so.C * es + wb;
            pl.ops.push_back(op);
        } else if (fill) {
            if (pair) {
                conv(P(4), EPI_PLAIN, curp, cur, sp, Mb, sp);
                conv(P(5), EPI_SHUFFLE, Mb, sp, sp, T[1], st).bytes -= (double)B * sp.H * sp.W * sm.C * es;   // reads only the extension half
            } else {
                conv(P(0), EPI_PLAIN, curp, cur, sm, Mb, sm);
                conv(P(1), EPI_PLAIN, curp, cur, s1, T[0], s1);
                conv(P(2), EPI_SHUFFLE, T[0], s1, s1, T[1], st);
            }
            Op &o2 = conv(P(3), EPI_RESUNPOOL, T[1], st, so, dst, so);
            residual(args(o2), Mb, sp, b.attrs[1]);
            args(o2).idx_in = pl.idx[(size_t)ref]; args(o2).idxCS = idxCS;
            o2.bytes += (double)B * sm.H * sm.W * sm.C * es + (double)B * sm.H * sm.W * idxCS;
        }
        cur = so;
    }

    bool fullconv(std::string &why) {
        Shape so{cur.H * 2, cur.W * 2, P(0).cout};
        if (so.H != H || so.W != W) { why = "network does not return to the input resolution"; return false; }
        if (fill) {
            ConvLaunch &l = std::get<ConvLaunch>(conv(P(0), EPI_CLASSES, curp, cur, cur, nullptr, so).l);
            l.a.ncls = ctx->w.ncls;
            l.cls = cls_supported(l.a) && !ctx->knobs.cls_conv;   // the route, decided here once
        }
        cur = so;
        return true;
    }

    // fill == false: only the buffer sizes; fill == true (the arena carved): the ops
    bool run(bool fill_, std::string &why) {
        fill = fill_;
        es = prec_es(ctx->prec);
        if (H % 8 || W % 8 || H <= 0 || W <= 0 || B <= 0) { why = "H and W must be positive multiples of 8"; return false; }
        const size_t nb = ctx->w.blocks.size();
        if (!fill) pl.idx_bytes.assign(nb, 0);
        cur = Shape{H, W, 8};
        curp = nullptr;
        int xi = 0;
        pl.ops.clear();
        nwords = 1;
        wmap.clear();
        for (bi = 0; bi < nb; ++bi) {
            const BlockDesc &b = ctx->w.blocks[bi];
            ids = &ctx->w.block_convs[bi];
            dst = X[xi];
            switch (b.type) {
            case BT_INITIAL: initial(b); break;
            case BT_DOWN: down(b); break;
            case BT_REGULAR: regular(b); break;
            case BT_UP: up(b); break;
            case BT_FULLCONV: if (!fullconv(why)) return false; break;
            }
            if (b.type != BT_FULLCONV) {
                curp = dst;
                xi ^= 1;
            }
        }
        return true;
    }
};

// Derived launch fields (conv_kernels.hip): magic divisors, buffer-descriptor sizes (every tensor
// must be addressable with 31-bit byte offsets), the staging shift. false: a tensor is too large.
bool finish_conv_args(ConvArgs &a, int epi, size_t es) {
    fastdiv((uint32_t)(a.Hg * a.Wg), a.mHWg, a.sHWg);
    fastdiv((uint32_t)a.Wg, a.mWg, a.sWg);
    a.wy0 = 0; a.wrows = a.Hg; a.orow0 = 0; a.orow1 = a.Hout;   // class kernel: the full frame
    const double in_b = (double)a.B * a.Hin * a.Win * a.CinS * es;
    const double out_b = epi == EPI_CLASSES ? 0.0 : (double)a.B * a.Hout * a.Wout * a.outC * es;
    const double res_b = a.res ? (double)a.B * a.resH * a.resW * a.resCS * es : 0.0;
    const double idx_b = a.idx_out ? (double)a.M * a.idxCS : a.idx_in ? (double)a.B * a.resH * a.resW * a.idxCS : 0.0;
    const double lim = 2147483648.0;
    if (in_b >= lim || out_b >= lim || res_b >= lim || idx_b >= lim ||
        (epi == EPI_CLASSES && (double)a.B * a.Hout * a.Wout * a.ncls * 4.0 >= 4.0 * lim))
        return false;
    a.in_bytes = (uint32_t)in_b; a.out_bytes = (uint32_t)out_b;
    a.res_bytes = (uint32_t)res_b; a.idx_bytes = (uint32_t)idx_b;
    const int epc = 16 / (int)es, cpr = a.outC / epc;
    a.cpr_sh = -1;
    if (a.outC % epc == 0 && cpr > 0 && (cpr & (cpr - 1)) == 0)
        for (a.cpr_sh = 0; (1 << a.cpr_sh) < cpr; ++a.cpr_sh) {}
    a.stage_ok = a.cpr_sh >= 0 && (epi != EPI_SHUFFLE || (a.Wg % 16 == 0 && a.M % 16 == 0));
    return true;
}

// The class-fused launch (Plan::cls_ok) of the last bottleneck q and the class layer l: q's arguments, 15 x
// 15-strided 16 x 16 tiles, no block output or range words written, l's weights and bias; the class map and
// its LUT are the forward's (bind)
Launch cls_fused_launch(const BneckLaunch &q, const ConvArgs &l) {
    BneckLaunch f = q;
    f.cls = true;
    BneckArgs &a = f.a;
    a.rg.amax_out = nullptr;
    a.tr = 0;
    a.tiles_y = (a.H + 14) / 15; a.tiles_x = (a.W + 14) / 15;
    a.ntiles = a.B * a.tiles_y * a.tiles_x;
    a.cw = l.w; a.cbias = l.bias; a.ncls = l.ncls; a.csw = l.rg.sw[0];
    a.cls_bytes = (uint32_t)((size_t)l.B * l.Hout * l.Wout);
    return f;
}

// The plan's launch l as a forward issues it where the pair overlay has flipped the activation buffers X: every
// tensor the plan puts in one of them lies in the other. The one place that knows which pointers of a launch are
// tensors in those buffers; used while the plan is built only (build_pairs).
Launch flipped(const Launch &l, unsigned char *const X[2]) {
    Launch f = l;
    auto mv = [&](auto *&p) {
        using P = std::remove_reference_t<decltype(p)>;
        if ((const void *)p == X[0]) p = (P)X[1];
        else if ((const void *)p == X[1]) p = (P)X[0];
    };
    if (ConvLaunch *c = std::get_if<ConvLaunch>(&f)) { mv(c->a.in); mv(c->a.out); mv(c->a.res); }
    else if (UpLaunch *u = std::get_if<UpLaunch>(&f)) { mv(u->a.x); mv(u->a.out); }
    else if (BneckLaunch *b = std::get_if<BneckLaunch>(&f)) { mv(b->a.x); mv(b->a.out); mv(b->a.xin); }
    return f;
}

// The pair overlay of the plan pl under construction: the pairs (Plan::firsts, Plan::pairs) and every op's
// forward launch and walk parity (Op::fwd, Op::fwd_odd), final from here on. Pairs exist in fp32, in the fused plan, with
// no C = 64 tile variant forced, where the spare buffer holds a C = 64 tensor; the decoder's last WIN_OPS ops keep their
// own (row-windowed) launches. X: the arena's two activation buffers.
void build_pairs(const bugseg_ctx *ctx, Plan &pl, unsigned char *const X[2], unsigned char *spare, size_t spare_bytes) {
    const int n = (int)pl.ops.size();
    const Knobs &k = ctx->knobs;
    if (ctx->prec == PREC_F32 && !k.no_fuse && k.bneck_variant < 0 && k.bneck_variant_c64 < 0) {
        auto buf = [&](const void *p) { return p == X[0] ? 0 : p == X[1] ? 1 : -1; };
        std::vector<PairCand> c((size_t)n);
        for (int i = 0; i < n - WIN_OPS; ++i) {
            const BneckLaunch *b = pl.ops[(size_t)i].bneck();
            if (!b || !pl.ops[(size_t)i].regular(64, b->a.H) || b->a.tr || b->cls || b->win || b->var < 0 || b->var > 2) continue;
            if (b->a.x_bytes > spare_bytes) continue;
            c[(size_t)i] = PairCand{true, b->a.H, b->a.W, buf(b->a.x), buf(b->a.out)};
        }
        pl.firsts = pair_firsts(c);
    }
    std::vector<int> act((size_t)n), flip((size_t)n);
    pair_actions(n, pl.firsts, 0, n, act.data(), flip.data());
    for (int i = 0; i < n; ++i) {
        Op &op = pl.ops[(size_t)i];
        op.fwd = flip[(size_t)i] ? flipped(op.l, X) : op.l;
        op.fwd_odd = (op.pos & 1) ^ flip[(size_t)i];
    }
    int th, tw, threads;
    size_t lds;
    bneck_pair_shape(th, tw, threads, lds);
    for (int i = 0; i < n; ++i) {
        if (act[(size_t)i] != PA_PAIR) continue;
        BneckArgs &A = std::get<BneckLaunch>(pl.ops[(size_t)i].fwd).a, &Bk = std::get<BneckLaunch>(pl.ops[(size_t)i + 1].fwd).a;
        PairOp p;
        p.first = i; p.flip = flip[(size_t)i];
        p.args.a = A; p.args.b = Bk;
        p.args.b.out = A.out;                 // where the skipped tensor would have gone
        p.args.a.tiles_y = (A.H + th - 1) / th; p.args.a.tiles_x = (A.W + tw - 1) / tw;
        p.args.a.ntiles = A.B * p.args.a.tiles_y * p.args.a.tiles_x;
        p.args.a.oy_base = 0;
        p.ga.ra = A.rg; p.ga.rb = Bk.rg; p.ga.clear = Bk.rg.amax_out;
        p.gb = p.ga; p.gb.clear = nullptr;
        pl.pairs.push_back(p);
        // outside the whole pair (a forward's op range cuts it; the pair's guarded fallbacks): block A into the spare
        // buffer, block B from it to the pair's output
        A.out = spare;
        Bk.x = spare; Bk.out = p.args.b.out;
    }
}

// The context's plan for (B, H, W): kept when it is that already, else built in a local and moved in complete
// (DESIGN 6.28). A failure before the old arena is retired (the size pass) leaves the installed plan in force; a
// failure after it (the allocation, the fill pass, the range-word count, the 31-bit sizes) leaves Plan(), with the
// new arena freed: nothing was ever enqueued on it. Retire, then allocate: a re-plan's peak memory is one arena.
bool build_plan(bugseg_ctx *ctx, int B, int H, int W, std::string &why, void *stream = nullptr) {
    if (ctx->plan.at(B, H, W)) return true;
    Plan pl;
    Walker w{ctx, pl, B, H, W};
    if (!w.run(false, why)) return false;
    auto al = [](size_t v) { return (v + 4095) / 4096 * 4096; };
    size_t total = 2 * al(w.szX) + 3 * al(w.szT) + al(w.szM);
    for (size_t s : pl.idx_bytes) total += al(s);
    pl.words_bytes = ctx->prec == PREC_F32 ? (size_t)Walker::max_words(ctx->w.blocks.size()) * RNG_SLOTS * 4 : 0;
    total += al(pl.words_bytes);
    const bool cap = stream_capturing(stream);
    RelaxCapture relax;                 // the first forward at a shape may itself be captured
    if (!ctx->plan.empty()) {
        // a forward of the old shape may still be running (or be part of a captured graph)
        ctx->mem.retire(ctx->plan.arena, cap || ctx->plan.pinned);
        ctx->plan = Plan();
    }
    if (hipMalloc(&pl.arena, total) != hipSuccess) {
        (void)hipGetLastError();            // (reported here: the next launch's check must not find it)
        why = "hipMalloc of the activation arena failed";
        return false;
    }
    auto drop = [&](const char *what) { if (what) why = what; (void)hipFree(pl.arena); return false; };
    unsigned char *p = (unsigned char *)pl.arena;
    w.X[0] = p; p += al(w.szX);
    w.X[1] = p; p += al(w.szX);
    for (int i = 0; i < 3; ++i) { w.T[i] = p; p += al(w.szT); }
    w.Mb = p; p += al(w.szM);
    pl.idx.assign(pl.idx_bytes.size(), nullptr);
    for (size_t i = 0; i < pl.idx_bytes.size(); ++i) if (pl.idx_bytes[i]) { pl.idx[i] = p; p += al(pl.idx_bytes[i]); }
    pl.words = pl.words_bytes ? (float *)p : nullptr;
    if (!w.run(true, why)) return drop(nullptr);
    if (pl.words_bytes && w.nwords > Walker::max_words(ctx->w.blocks.size())) return drop("range words: plan too long");
    for (Op &op : pl.ops) {
        bool fits = true;
        if (BneckLaunch *b = std::get_if<BneckLaunch>(&op.l)) {
            const double bytes = (double)b->a.B * b->a.H * b->a.W * b->C * w.es;
            const double in_bytes = b->cin ? 4.0 * b->a.B * b->a.H * b->a.W * b->cin * w.es : 0.0;
            fits = bytes < 2147483648.0 && in_bytes < 2147483648.0;
            if (fits) b->a.x_bytes = (uint32_t)bytes;
        } else if (ConvLaunch *c = std::get_if<ConvLaunch>(&op.l)) {
            fits = finish_conv_args(c->a, c->epi, w.es);
        }
        if (!fits) return drop("batch too large for 32-bit tensor offsets");
    }
    int issued = 0;
    for (Op &op : pl.ops) { op.pos = issued; issued += op.launches; }
    // the spare buffer: T[1] (the fused plan's launches use none of the T buffers)
    build_pairs(ctx, pl, w.X, w.T[1], al(w.szT));
    if (ctx->knobs.cls_fuse && pl.ops.size() >= 2 && pl.ops.back().class_kernel()) {
        const ConvArgs &l = pl.ops.back().conv()->a;
        const Op &q = pl.ops[pl.ops.size() - 2];
        pl.cls_ok = q.regular(16, l.Hin) && q.bneck()->a.out == l.in && l.B == q.bneck()->a.B && l.Win == q.bneck()->a.W &&
                    (double)B * l.Hout * l.Wout < 2147483648.0;
        if (pl.cls_ok) {
            pl.cls_fused = cls_fused_launch(*q.bneck(), l);
            pl.cls_fused_fwd = cls_fused_launch(std::get<BneckLaunch>(q.fwd), std::get<ConvLaunch>(pl.ops.back().fwd).a);
        }
    }
    pl.B = B; pl.H = H; pl.W = W;
    pl.arena_bytes = total;
    pl.act_bytes = total - al(pl.words_bytes);
    ctx->plan = std::move(pl);
    return true;
}

// ---------------------------------------------------------------- row windows of the decoder
// Class rows [row0, row1) of an H-row frame (0 <= row0 < row1 <= H, H % 8 == 0) -> the rows each of the
// last WIN_OPS ops must run, walked back from the class layer through the kernels' read footprints:
//   class layer (cls_kernels.hip): input pixel (y, x) makes output rows 2y, 2y + 1 from input rows y, y + 1;
//   bottlenecks (bneck_kernels.hip): whole tile rows, counted from the first row needed, reading one row
//   above and below (the 3x3 middle conv);
//   upsampling blocks (up_kernels.hip): input pixel (y, x) makes output rows 2y, 2y + 1 from input row y and
//   the pooling indices of row y alone.
// Coordinates are absolute and clamped to the image only. tile_rows(k, need0, need1) gives the image rows
// per tile row of bottleneck k for the rows it must produce. win[k] = [y0, y1) (WinOp).
template <typename F>
void row_windows(int H, int row0, int row1, F tile_rows, int (*win)[2]) {
    const int h2 = H / 2, h4 = H / 4, h8 = H / 8;
    int a = row0, b = row1;
    auto set = [&](int k) { win[k][0] = a; win[k][1] = b; };
    auto halve = [&](int h) { a >>= 1; b = std::min((b + 1) >> 1, h); };
    auto grow = [&](int h) { a = std::max(a - 1, 0); b = std::min(b + 1, h); };
    auto tiles = [&](int k, int h) {
        // whole tile rows from the first needed row on (the tile grid starts there, BneckArgs::oy_base): the
        // fewest tiles, and every row a tile computes has its inputs inside the producer's window
        const int t = std::max(1, tile_rows(k, a, b));
        b = std::min(a + (b - a + t - 1) / t * t, h);
    };
    halve(h2); set(5);
    b = std::min(b + 1, h2);                  // the class layer's dy = 1 taps
    tiles(4, h2); set(4); grow(h2);
    halve(h4); set(3);
    tiles(2, h4); set(2); grow(h4);
    tiles(1, h4); set(1); grow(h4);
    halve(h8); set(0);
}

// The walk continued into stage 3, from the rows [y0, y1) of the h-row stage-3 output that the 128 -> 64
// upsampling block reads, back through the blocks before it: blk[0] writes that output, blk[1] feeds blk[0], ...
// A block's output window is the rows its consumer reads; what it reads itself reaches `reach` rows further
// either way, clamped to the image: the dilation of a 3x3 block, 2 for the asymmetric block's 5x1 conv.
//   plain tiles (d = 1, untransposed): whole tile rows from the first needed row, as in the decoder;
//   tile_rows(k, need0, need1) gives the image rows per tile row of the form picked for those rows (0: none built);
//   row-dilated tiles (d a power of two): exactly the needed rows — every row phase starts its tiles at its
//   first needed row, and the kernel skips the fragments of rows past the window (BneckArgs::oy_end).
// The walk stops at the first block whose window is the whole frame, whose form has no windowed kernel, or whose
// window runs no fewer rows than its full-frame launch computes per frame (rows_full: tile rows x rows per
// tile row; a row-dilated form: phases x tiles_y x tile rows — the rows it runs MFMAs for, in the image or not).
// Every block before that runs the full frame, so every row a windowed tile reads was written by its producer's
// window or by a full launch. Returns the number of windowed blocks; win[k] = [y0, y1) for k below it.
struct S3Desc { int asym = 0, d = 1, rd = 0, rows_full = 0; };
template <typename F>
int stage3_windows(int h, int y0, int y1, int n, const S3Desc *blk, F tile_rows, int (*win)[2]) {
    int a = std::max(y0, 0), b = std::min(y1, h), k = 0;
    for (; k < n; ++k) {
        const S3Desc &q = blk[k];
        if (a >= b || (a == 0 && b == h) || q.d < 1) break;
        int e = b, run;
        if (q.rd) {
            if (q.asym || (q.d & (q.d - 1))) break;
            run = b - a;
        } else {
            if (q.d != 1) break;
            const int t = tile_rows(k, a, b);
            if (t <= 0) break;
            run = (b - a + t - 1) / t * t;
            e = std::min(a + run, h);
        }
        if (run >= q.rows_full) break;
        win[k][0] = a; win[k][1] = e;
        const int reach = q.asym ? 2 : q.d;
        a = std::max(a - reach, 0);
        b = std::min(e + reach, h);
    }
    return k;
}

// The full-frame launch `full` narrowed to its window w of a forward for class rows [row0, row1): the same
// arguments with the per-frame extent cut to the window's rows and its first row as an offset; walk direction,
// XCD grouping and range words as in the full launch, over the smaller count. All the window arithmetic of the
// launch path is here. s3: a stage-3 block (WinPlan::s3), which takes the windowed kernels.
Launch narrow(const Launch &full, const WinOp &w, bool s3, int row0, int row1) {
    Launch l = full;
    const int rows = w.y1 - w.y0;
    if (BneckLaunch *b = std::get_if<BneckLaunch>(&l)) {
        BneckArgs &q = b->a;
        b->var = w.var;
        b->win = s3;
        q.tr = w.tr; q.tiles_x = w.tiles_x; q.tiles_y = w.tiles_y;
        q.ntiles = q.B * q.phases * q.tiles_y * q.tiles_x;   // (the decoder's blocks: one phase)
        q.oy_base = w.y0;
        if (s3) q.oy_end = w.y1;
    } else if (UpLaunch *u = std::get_if<UpLaunch>(&l)) {
        UpArgs &q = u->a;
        q.y0 = w.y0; q.hwin = rows;
        q.M = (q.M / q.h) * rows;                            // B * rows * w
        fastdiv((uint32_t)(rows * q.w), q.mHW, q.sHW);
    } else {
        ConvArgs &q = std::get<ConvLaunch>(l).a;             // the class layer
        q.wy0 = w.y0; q.wrows = rows;
        q.M = q.B * rows * q.Wg;
        fastdiv((uint32_t)(rows * q.Wg), q.mHWg, q.sHWg);
        q.orow0 = row0; q.orow1 = row1;
    }
    return l;
}

// The windowed form of the current plan for class rows [row0, row1), cached by window; nullptr = run the
// full-frame plan: the window is the whole frame or out of range, or the plan does not end in the six
// fused launches the windows are defined for (BUGSEG_NO_FUSE, BUGSEG_CLS_CONV, BUGSEG_CLS_FUSE, a class
// layer the class kernel does not take).
const WinPlan *window_plan(bugseg_ctx *ctx, int row0, int row1) {
    Plan &pl = ctx->plan;
    if (row0 < 0 || row1 > pl.H || row0 >= row1 || (row0 == 0 && row1 == pl.H)) return nullptr;
    for (const WinPlan &w : pl.wins)
        if (w.row0 == row0 && w.row1 == row1) return &w;
    const int n = (int)pl.ops.size(), H = pl.H;
    if (n < WIN_OPS + 1 || pl.cls_ok) return nullptr;
    const Op *o = &pl.ops[(size_t)(n - WIN_OPS)];
    if (!(o[0].up_on(H / 8) && o[1].regular(64, H / 4) && o[2].regular(64, H / 4) && o[3].up_on(H / 4) &&
          o[4].regular(16, H / 2) && o[5].class_kernel() && o[5].conv()->a.Hg == H / 2))
        return nullptr;
    // the op k blocks before the 128 -> 64 block, as a fused bottleneck (null: none, or another launch form). Only
    // forwards take a window, so the windowed launches are narrowed from the forward launches (Op::fwd)
    auto s3b = [&](int k) { return n - WIN_OPS - 1 - k >= 0 ? std::get_if<BneckLaunch>(&pl.ops[(size_t)(n - WIN_OPS - 1 - k)].fwd) : nullptr; };
    // The tile form of block q for the `rows` rows it must produce, into r: the picker's choice for the window,
    // else (a thin window: none efficient enough) the full frame's. s3: among the untransposed forms with a
    // windowed kernel. -> image rows per tile row (0: no form).
    auto form = [&](const BneckLaunch &q, int rows, bool s3, WinOp &r) {
        auto built = [&](int v) { return !s3 || bneck_slots_per_cu(ctx->knobs, ctx->prec, q.C, q.asym, v, false, 0, true) > 0; };
        int ty = 0, tx = 0, tr = 0, rd = 0;
        int v = pick_bneck_variant(ctx, q.C, q.asym, 1, pl.B, rows, q.a.W, ty, tx, tr, rd);
        if (v < 0 || rd || (s3 && (tr || !built(v)))) { v = q.var; tr = s3 ? 0 : q.a.tr; }
        if (!built(v)) return 0;
        int th, tw, nw;
        bneck_shape(q.C, v, th, tw, nw, nullptr);
        r.var = v; r.tr = tr;
        r.te = tr ? tw : th;
        r.tiles_x = tr ? (q.a.W + th - 1) / th : (q.a.W + tw - 1) / tw;
        return r.te;
    };
    WinPlan w;
    w.row0 = row0; w.row1 = row1;
    int win[WIN_OPS][2];
    row_windows(H, row0, row1, [&](int k, int need0, int need1) { return form(*o[k].bneck(), need1 - need0, false, w.op[k]); }, win);
    for (int k = 0; k < WIN_OPS; ++k) {
        WinOp &r = w.op[k];
        r.y0 = win[k][0]; r.y1 = win[k][1];
        r.tiles_y = (r.y1 - r.y0 + r.te - 1) / r.te;
        r.l = narrow(o[k].fwd, r, false, row0, row1);
    }
    // on into stage 3: the ops before the 128 -> 64 block, while they are fused C = 128 bottlenecks on its input
    // grid whose form has a windowed kernel (fp32). BUGSEG_ROW_WINDOW_S3=0: the decoder's windows only (A/B)
    if (ctx->knobs.row_window_s3) {
        S3Desc blk[S3_OPS];
        int nb = 0, th[S3_OPS], tw, nw;
        for (; nb < S3_OPS; ++nb) {
            const BneckLaunch *q = s3b(nb);
            if (!(q && q->C == 128 && q->cin == 0 && q->a.H == H / 8 && q->a.W == o[0].up()->a.w)) break;
            S3Desc &d = blk[nb];
            bneck_shape(128, q->var, th[nb], tw, nw, &d.rd);
            d.asym = q->asym; d.d = q->a.dt;
            d.rows_full = d.rd ? q->a.phases * q->a.tiles_y * th[nb] : q->a.tr ? 0 : q->a.tiles_y * th[nb];
            if (d.rd && bneck_slots_per_cu(ctx->knobs, ctx->prec, 128, false, q->var, false, 0, true) <= 0) d.rows_full = 0;
        }
        int w3[S3_OPS][2];
        w.ns3 = stage3_windows(H / 8, w.op[0].y0, w.op[0].y1, nb, blk,
                               [&](int k, int need0, int need1) { return form(*s3b(k), need1 - need0, true, w.s3[k]); }, w3);
        for (int k = 0; k < w.ns3; ++k) {
            const BneckLaunch &q = *s3b(k);
            WinOp &r = w.s3[k];
            r.y0 = w3[k][0]; r.y1 = w3[k][1];
            if (blk[k].rd) {   // the full frame's form; tiles_y: of the longest row phase
                r.var = q.var; r.tr = 0; r.te = th[k]; r.tiles_x = 1;
                r.tiles_y = ((r.y1 - r.y0 + q.a.dt - 1) / q.a.dt + r.te - 1) / r.te;
            } else {
                r.tiles_y = (r.y1 - r.y0 + r.te - 1) / r.te;
            }
            r.l = narrow(q, r, true, row0, row1);
        }
    }
    if (pl.wins.size() >= 8) pl.wins.erase(pl.wins.begin());
    pl.wins.push_back(w);
    return &pl.wins.back();
}

// ---------------------------------------------------------------- preprocess tables
void linear_coeffs(int dsize, int ssize, double scale, int *ofs, short *a01) {
#pragma clang fp contract(off)
    for (int d = 0; d < dsize; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
        ofs[d] = s;
        long v0 = std::lrintf((1.f - f) * 2048.f), v1 = std::lrintf(f * 2048.f);
        a01[2 * d] = (short)std::min(32767L, std::max(-32768L, v0));
        a01[2 * d + 1] = (short)std::min(32767L, std::max(-32768L, v1));
    }
}

}  // namespace

namespace bugseg {
int ctx_fail(bugseg_ctx *ctx, int code, const char *msg) { return fail(ctx, code, msg); }
int ctx_device(const bugseg_ctx *ctx) { return ctx->mem.device; }
int launch_fail(bugseg_ctx *ctx, const char *op) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return BUGSEG_OK;
    return fail(ctx, BUGSEG_EHIP, std::string(op) + " launch: " + hipGetErrorString(e));
}
const Knobs &ctx_knobs(const bugseg_ctx *ctx) { return ctx->knobs; }
CtxMemory &ctx_memory(bugseg_ctx *ctx) { return ctx->mem; }
BevState &ctx_bev(bugseg_ctx *ctx) { return ctx->bev; }
int ctx_clahe_tables(bugseg_ctx *ctx, const void *host, size_t bytes, void *stream, const void **dev) {
    (void)stream;       // never touched: the upload runs and is waited for on the setup stream
    if (!ctx->clahe_tabs)
        if (hipError_t e = ctx->mem.upload({{host, bytes}}, &ctx->clahe_tabs))
            return fail(ctx, BUGSEG_EHIP, std::string("clahe table upload failed: ") + hipGetErrorString(e));
    *dev = ctx->clahe_tabs;
    return BUGSEG_OK;
}
}  // namespace bugseg

// =============================================================== C ABI
extern "C" {

int bugseg_version(void) { return 100; }

const char *bugseg_last_error(const bugseg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_thread_err.c_str(); }

int bugseg_create(int device, int precision, bugseg_ctx **out) {
    if (!out) return fail(nullptr, BUGSEG_EINVAL, "out is NULL");
    *out = nullptr;
    if (precision != BUGSEG_FP32 && precision != BUGSEG_BF16 && precision != BUGSEG_F16)
        return fail(nullptr, BUGSEG_EINVAL, "precision must be BUGSEG_FP32, BUGSEG_BF16 or BUGSEG_F16");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return fail(nullptr, BUGSEG_EINVAL, "no such HIP device: " + std::to_string(device));
    Knobs knobs;
    std::string bad;
    if (!read_knobs(knobs, bad)) return fail(nullptr, BUGSEG_EINVAL, bad);
    bugseg_ctx *c = new (std::nothrow) bugseg_ctx(knobs, device);
    if (!c) return fail(nullptr, BUGSEG_ENOMEM, "out of host memory");
    c->prec = precision == BUGSEG_BF16 ? PREC_BF16 : precision == BUGSEG_F16 ? PREC_F16 : PREC_F32;
    DeviceGuard g(device);
    // class remap tables (models.py:56-58 and :79-80) + the normalisation table (models.py:17-18, 91)
    unsigned char tab[32 + 3 * 256 * 8];
    const uint8_t lut3[16] = {1, 1, 0, 2, 2, 2, 2, 2, 2, 0, 2, 2, 2, 2, 2, 2};
    const uint8_t lutb[16] = {1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(tab, lut3, 16);
    std::memcpy(tab + 16, lutb, 16);
    const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
    for (int ch = 0; ch < 3; ++ch)
        for (int v = 0; v < 256; ++v) {
            const double x = ((double)v / 256.0 - mean[ch]) / stdv[ch];
            std::memcpy(tab + 32 + (ch * 256 + v) * 8, &x, 8);
            c->norm_amax = std::max(c->norm_amax, (float)std::fabs(x) * 1.0001f);
        }

    {
        // on the setup stream (never the legacy stream, which would join a capture in progress on another
        // stream), so a context may be created while a stream is capturing
        RelaxCapture relax;
        hipError_t e = c->mem.upload({{tab, sizeof(tab)}}, &c->dev_luts);
        hipStream_t s = c->mem.setup_stream();
        // bf16 / fp16: the fused initial block evaluates the table as one fmaf per byte when an f32
        // pair (a, b) near (1 / (256 std), -mean / std) reproduces all 256 stored values of a channel
        // bit for bit (searched on the device, with its own conversions: init_kernels.hip
        // naff_search_kernel) — no LDS lookups, whose data-dependent addresses conflict; fp32 keeps
        // the table. BUGSEG_INIT_TABLE=1 forces the table (A/B)
        if (e == hipSuccess && c->prec != PREC_F32 && !c->knobs.init_table) {
            float base[6];
            for (int ch = 0; ch < 3; ++ch) {
                base[ch] = (float)(1.0 / (256.0 * stdv[ch]));
                base[3 + ch] = (float)(-mean[ch] / stdv[ch]);
            }
            constexpr int N = 2 * NAFF_R + 1;
            std::vector<uint8_t> okh((size_t)3 * N * N);
            uint8_t *okd = nullptr;
            hipError_t e2 = hipMalloc(&okd, okh.size());
            if (e2 == hipSuccess) e2 = launch_naff_search(c->prec, (const double *)((const unsigned char *)c->dev_luts + 32), base, okd, s);
            if (e2 == hipSuccess) e2 = hipMemcpyAsync(okh.data(), okd, okh.size(), hipMemcpyDeviceToHost, s);
            if (e2 == hipSuccess) e2 = hipStreamSynchronize(s);
            if (okd) (void)hipFree(okd);
            bool all = e2 == hipSuccess;
            for (int ch = 0; ch < 3 && all; ++ch) {
                int best = -1, bestd = 1 << 30;
                for (int k = 0; k < N * N; ++k) {
                    const int da = k / N - NAFF_R, db = k % N - NAFF_R, d = std::max(std::abs(da), std::abs(db));
                    if (okh[(size_t)ch * N * N + k] && d < bestd) { best = k; bestd = d; }
                }
                if (best < 0) { all = false; break; }
                int32_t ia, ib;
                std::memcpy(&ia, &base[ch], 4);
                std::memcpy(&ib, &base[3 + ch], 4);
                ia += best / N - NAFF_R;
                ib += best % N - NAFF_R;
                std::memcpy(&c->naff[ch], &ia, 4);
                std::memcpy(&c->naff[3 + ch], &ib, 4);
            }
            c->naff_on = all;
        }
        if (e != hipSuccess) {
            delete c;
            return fail(nullptr, BUGSEG_EHIP, std::string("device allocation failed: ") + hipGetErrorString(e));
        }
    }
    *out = c;
    return BUGSEG_OK;
}

int bugseg_destroy(bugseg_ctx *ctx) {
    if (!ctx) return BUGSEG_OK;
    DeviceGuard g(ctx->mem.device);
    (void)hipDeviceSynchronize();
    if (ctx->dev_w) (void)hipFree(ctx->dev_w);
    if (ctx->dev_luts) (void)hipFree(ctx->dev_luts);
    if (ctx->plan.arena) (void)hipFree(ctx->plan.arena);
    if (ctx->clahe_tabs) (void)hipFree(ctx->clahe_tabs);
    delete ctx;                                       // the caches, the graveyard and the setup stream
    return BUGSEG_OK;
}

int bugseg_load_weights(bugseg_ctx *ctx, const void *blob, size_t bytes) {
    if (!ctx || !blob) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    DeviceGuard g(ctx->mem.device);
    // a refused blob changes nothing: the old model stays loaded and its plan in force
    EnetWeights w;
    std::string why;
    if (!build_weights(blob, bytes, ctx->prec, ctx->knobs, w, why)) return fail(ctx, BUGSEG_EFORMAT, "weight blob: " + why);
    // a captured graph's kernels hold pointers into the old weights and arena: then kept until destroy
    ctx->mem.retire(ctx->dev_w, ctx->plan.pinned);
    if (!ctx->plan.empty()) ctx->mem.retire(ctx->plan.arena, ctx->plan.pinned);
    ctx->dev_w = nullptr;
    ctx->plan = Plan();
    ctx->w = EnetWeights();
    ctx->loaded = false;
    // the new model goes in whole, once it is on the device; a failure leaves no weights, no plan, nothing allocated
    void *dev = nullptr;
    if (hipMalloc(&dev, w.host_w.size()) != hipSuccess ||
        hipMemcpy(dev, w.host_w.data(), w.host_w.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (dev) (void)hipFree(dev);
        return fail(ctx, BUGSEG_EHIP, "uploading weights failed");
    }
    ctx->dev_w = dev;
    ctx->w = std::move(w);
    ctx->loaded = true;
    return BUGSEG_OK;
}

int bugseg_num_classes(const bugseg_ctx *ctx) { return ctx && ctx->loaded ? ctx->w.ncls : 0; }

size_t bugseg_input_bytes(const bugseg_ctx *ctx, int B, int H, int W) {
    if (!ctx || B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * H * W * 8 * prec_es(ctx->prec);
}

int bugseg_preprocess(bugseg_ctx *ctx, const uint8_t *bgr, int B, int H0, int W0, int H, int W, int out_layout,
                      void *out, void *stream) {
    if (!ctx || !bgr || !out) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    if (B <= 0 || H0 <= 0 || W0 <= 0 || H <= 0 || W <= 0) return fail(ctx, BUGSEG_EINVAL, "bad shape");
    if (out_layout < BUGSEG_PRE_ENGINE || out_layout > BUGSEG_PRE_BGR_U8) return fail(ctx, BUGSEG_EINVAL, "bad out_layout");
    DeviceGuard g(ctx->mem.device);
    PreArgs a;
    std::memset(&a, 0, sizeof(a));
    a.bgr = bgr; a.B = B; a.H0 = H0; a.W0 = W0; a.H = H; a.W = W;
    a.lut = (const double *)((const unsigned char *)ctx->dev_luts + 32);
    a.out_layout = out_layout; a.prec = ctx->prec; a.out = out;
    a.vec_end = W * 3 - (W * 3) % 8;
    if (H0 == H && W0 == W) {
        a.mode = 0;
    } else {
        const double sx = 1.0 / ((double)W / W0), sy = 1.0 / ((double)H / H0);
        const int isx = (int)std::lrint(sx), isy = (int)std::lrint(sy);
        const double eps = 2.220446049250313e-16;
        if (std::fabs(sx - isx) < eps && std::fabs(sy - isy) < eps && isx == 2 && isy == 2) {
            a.mode = 1;
        } else {
            a.mode = 2;
            int rc = BUGSEG_OK;
            const auto *hit = ctx->pre_tabs.get(ctx->mem, {H0, W0, H, W}, stream_capturing(stream), true, &rc, [&](auto &t) -> int {
                std::vector<int> xo((size_t)W), yo((size_t)H);
                std::vector<short> xa(2 * (size_t)W), yb(2 * (size_t)H);
                linear_coeffs(W, W0, sx, xo.data(), xa.data());
                linear_coeffs(H, H0, sy, yo.data(), yb.data());
                const hipError_t e = ctx->mem.upload({{xo.data(), (size_t)W * 4}, {xa.data(), (size_t)W * 4}, {yo.data(), (size_t)H * 4},
                                                      {yb.data(), (size_t)H * 4}}, &t.tab);
                if (e == hipSuccess) return BUGSEG_OK;
                return fail(ctx, BUGSEG_EHIP, std::string("resize table upload failed: ") + hipGetErrorString(e));
            });
            if (!hit) return rc;
            unsigned char *t = (unsigned char *)hit->tab;
            a.xofs = (const int *)t;
            a.xa = (const short *)(t + (size_t)W * 4);
            a.yofs = (const int *)(t + (size_t)W * 8);
            a.yb = (const short *)(t + (size_t)W * 8 + (size_t)H * 4);
        }
    }
    hipError_t e = launch_preprocess(a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("preprocess launch: ") + hipGetErrorString(e));
    return BUGSEG_OK;
}

int bugseg_nchw_to_input(bugseg_ctx *ctx, const void *x, int is_f64, int B, int H, int W, void *out, void *stream) {
    if (!ctx || !x || !out) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    if (B <= 0 || H <= 0 || W <= 0) return fail(ctx, BUGSEG_EINVAL, "bad shape");
    DeviceGuard g(ctx->mem.device);
    NchwArgs a{x, is_f64 ? 1 : 0, B, H, W, ctx->prec, out};
    hipError_t e = launch_nchw_to_input(a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("layout launch: ") + hipGetErrorString(e));
    return BUGSEG_OK;
}

static hipError_t dispatch(const bugseg_ctx *c, const ConvLaunch &l, hipStream_t s) { return launch_conv(c->prec, l.nr, l.epi, l.a, s, l.cls); }
static hipError_t dispatch(const bugseg_ctx *c, const UpLaunch &l, hipStream_t s) { return launch_up(c->prec, l.cin, l.it, l.cout, l.a, s); }
static hipError_t dispatch(const bugseg_ctx *c, const BneckLaunch &l, hipStream_t s) {
    return l.cls ? launch_bneck_cls(c->knobs, c->prec, l.a, s)
                 : launch_bneck(c->knobs, c->prec, l.C, l.asym, l.var, l.a, s, l.cin, l.win);
}
// The tile walk direction of op i's launch (Knobs::tile_order: 0 ascending, 1 alternating from ascending (DESIGN
// 6.10), 2 descending). Alternating follows the parity of the launches issued before the op, so a single op and an
// op range walk as they do in the whole run: of the plan's own launches (Op::pos), or (fwd) of a forward's, where a
// pair is one launch (Op::fwd_odd).
static int walk_rev(const bugseg_ctx *ctx, int i, bool fwd) {
    const Op &o = ctx->plan.ops[(size_t)i];
    const int order = ctx->knobs.tile_order;
    return order == 2 ? 1 : order == 1 ? (fwd ? o.fwd_odd : o.pos & 1) : 0;
}
// Op i's launch-span slots, where bugseg_debug_set_spans armed them (mfma_common.h: 64 slots x 64 B), else null
static unsigned long long *span_slots(const bugseg_ctx *ctx, int i) {
    return ctx->spans && i < ctx->spans_ops ? ctx->spans + 512 * (size_t)i : nullptr;
}

// One launch record to its kernel, with its launch-span slots (or null) and its tile walk direction (span_slots,
// walk_rev): the one place that sets them for a single launch; launch_pair sets its three launches' from the same two.
static hipError_t issue(const bugseg_ctx *ctx, Launch &l, int rev, unsigned long long *span, hipStream_t s) {
    return std::visit([&](auto &r) {
        r.a.span = span;
        r.a.rev = rev;
        return dispatch(ctx, r, s);
    }, l);
}

// A forward's binding into a copy of a launch. first: the plan's first op (the initial block) takes the input;
// last: the class layer, or the class-fused bottleneck, takes the output.
static void bind(const bugseg_ctx *ctx, const Binding &b, bool first, bool last, Launch &l) {
    ConvLaunch *c = std::get_if<ConvLaunch>(&l);
    if (first && c) {
        c->epi = b.bgr ? EPI_INIT_BGR : EPI_INIT;
        c->a.in = b.in;
        c->a.nlut = b.bgr ? (const double *)((const unsigned char *)ctx->dev_luts + 32) : nullptr;
        c->a.naff_on = b.bgr && ctx->naff_on;   // (the exact affine form of the normalisation, where the context has one)
        std::memcpy(c->a.naff, ctx->naff, sizeof(ctx->naff));
        // fp32 range scaling: the BGR input's range is the normalisation table's (static); an engine input
        // the caller supplied is measured (block 0 of the range words)
        c->a.rg.amax_in = b.bgr ? nullptr : ctx->plan.words;
        c->a.rg.amax_static = b.bgr ? ctx->norm_amax : 0.f;
    }
    if (!last) return;
    const uint8_t *luts = (const uint8_t *)ctx->dev_luts;
    const bool logits = b.out_kind == BUGSEG_OUT_LOGITS_F32;
    uint8_t *cls_out = logits ? nullptr : (uint8_t *)b.out;
    const int lut_kind = b.out_kind == BUGSEG_OUT_CLASS3_U8 ? 1 : b.out_kind == BUGSEG_OUT_BINARY_U8 ? 2 : 0;
    const uint8_t *lut = lut_kind ? luts + 16 * (lut_kind - 1) : nullptr;
    if (BneckLaunch *f = std::get_if<BneckLaunch>(&l)) {
        f->a.cls_out = cls_out; f->a.lut = lut; f->a.lut_kind = lut_kind;
    } else if (c) {
        c->a.cls_out = cls_out; c->a.lut = lut; c->a.lut_kind = lut_kind;
        c->a.logits_out = logits ? (float *)b.out : nullptr;
    }
}

// One plan op for the last forward's binding (Plan::bound). Every record is final once the plan is built; launch_op
// only picks the op's — its windowed launch when wp (a row-windowed forward, window_plan) has one, the class-fused
// launch when the forward took it (the last op then issues nothing; nothing follows it), else the full-frame launch
// — binds a copy and issues it. fwd: the launch of a forward (Op::fwd: where the pair overlay puts the op, walking as
// the launches really issued before it alternate), not the plan's own (bugseg_plan_launch_op).
static hipError_t launch_op(const bugseg_ctx *ctx, int i, hipStream_t s, const WinPlan *wp = nullptr, bool fwd = false) {
    const Plan &pl = ctx->plan;
    const int n = (int)pl.ops.size();
    if (pl.cls_on && i + 1 == n) return hipSuccess;   // (ran within op i - 1)
    const bool fused = pl.cls_on && i + 2 == n;
    const Launch *pick = wp ? wp->launch_of(i, n) : nullptr;
    if (!pick) pick = fused ? (fwd ? &pl.cls_fused_fwd : &pl.cls_fused) : fwd ? &pl.ops[(size_t)i].fwd : &pl.ops[(size_t)i].l;
    Launch l = *pick;
    bind(ctx, pl.bound, i == 0, fused || i + 1 == n, l);
    return issue(ctx, l, walk_rev(ctx, i, fwd), span_slots(ctx, i), s);
}

// Pair p in place of ops i = p.first and i + 1: the paired launch, then the two ops' forward launches as its guarded
// fallbacks (BneckGuardArgs), which return at once unless the pair's speculation on the range exponents failed. The
// pair and the first fallback walk as op i, the second as op i + 1. Armed spans: op i's slots time the paired launch,
// op i + 1's its second fallback.
static hipError_t launch_pair(const bugseg_ctx *ctx, const PairOp &p, hipStream_t s) {
    const int i = p.first;
    const BneckLaunch &A = std::get<BneckLaunch>(ctx->plan.ops[(size_t)i].fwd), &Bk = std::get<BneckLaunch>(ctx->plan.ops[(size_t)i + 1].fwd);
    BneckPairArgs a = p.args;
    BneckArgs fa = A.a, fb = Bk.a;
    a.a.rev = fa.rev = walk_rev(ctx, i, true);
    a.a.span = span_slots(ctx, i); fa.span = nullptr;
    fb.rev = walk_rev(ctx, i + 1, true);
    fb.span = span_slots(ctx, i + 1);
    hipError_t e = launch_bneck_pair(ctx->knobs, a, s);
    if (e == hipSuccess) e = launch_bneck_guarded(ctx->knobs, A.var, fa, p.ga, s);
    if (e == hipSuccess) e = launch_bneck_guarded(ctx->knobs, Bk.var, fb, p.gb, s);
    return e;
}

static int enet_forward(bugseg_ctx *ctx, const void *in, bool bgr, int B, int H, int W, int out_kind, void *out,
                        void *stream, int first_op = 0, int last_op = -1, int row0 = 0, int row1 = 0) {
    if (!ctx || !in || !out) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    if (!ctx->loaded) return fail(ctx, BUGSEG_ESTATE, "no weights loaded");
    if (out_kind < BUGSEG_OUT_LOGITS_F32 || out_kind > BUGSEG_OUT_BINARY_U8) return fail(ctx, BUGSEG_EINVAL, "bad out_kind");
    DeviceGuard g(ctx->mem.device);
    std::string why;
    if (!build_plan(ctx, B, H, W, why, stream)) return fail(ctx, BUGSEG_EINVAL, why);
    Plan &pl = ctx->plan;
    if (stream_capturing(stream)) pl.pinned = true;
    pl.bound = Binding{in, bgr, out_kind, out};
    const int nops = (int)pl.ops.size();
    if (last_op < 0 || last_op > nops) last_op = nops;
    if (first_op < 0 || first_op > last_op) return fail(ctx, BUGSEG_EINVAL, "bad op range");
    if (pl.words && first_op == 0) {
        // every launch max-accumulates its output's range: cleared once per forward (a memset node when captured)
        hipError_t e = hipMemsetAsync(pl.words, 0, pl.words_bytes, (hipStream_t)stream);
        if (e == hipSuccess && !bgr) e = launch_amax((const float *)in, (size_t)B * H * W * 8, pl.words, (hipStream_t)stream);
        if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("range words: ") + hipGetErrorString(e));
    }
    pl.cls_on = pl.cls_ok && out_kind != BUGSEG_OUT_LOGITS_F32 && first_op <= nops - 2 && last_op == nops;
    // class rows [row0, row1) only (bugseg_enet_forward_bgr_rows); null: the full-frame launches
    const WinPlan *wp = window_plan(ctx, row0, row1);
    // what each op does in this op range (pair_actions, the walk bugseg_debug_pair_walk shows): a pair with both ops
    // in the range is one launch for ops i and i + 1, every other op its forward launch
    std::vector<int> act(2 * (size_t)nops);           // (the flips behind the actions: in the records already)
    pair_actions(nops, pl.firsts, first_op, last_op, act.data(), act.data() + nops);
    for (int i = first_op; i < last_op; ++i) {
        hipError_t e = hipSuccess;
        switch (act[(size_t)i]) {
        case PA_SKIP: break;                          // (ran within the pair)
        case PA_PAIR:
            e = launch_pair(ctx, pl.pairs[(size_t)(std::lower_bound(pl.firsts.begin(), pl.firsts.end(), i) - pl.firsts.begin())], (hipStream_t)stream);
            if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, "pair launch " + std::to_string(i) + ": " + hipGetErrorString(e));
            break;
        default:                                      // PA_PLAIN, PA_LONE_FIRST, PA_LONE_SECOND
            e = launch_op(ctx, i, (hipStream_t)stream, wp, true);
            if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, "conv launch " + std::to_string(i) + ": " + hipGetErrorString(e));
        }
    }
    return BUGSEG_OK;
}

int bugseg_enet_forward(bugseg_ctx *ctx, const void *in, int B, int H, int W, int out_kind, void *out, void *stream) {
    return enet_forward(ctx, in, false, B, H, W, out_kind, out, stream);
}

int bugseg_enet_forward_bgr(bugseg_ctx *ctx, const uint8_t *bgr, int B, int H, int W, int out_kind, void *out,
                            void *stream) {
    return enet_forward(ctx, bgr, true, B, H, W, out_kind, out, stream);
}

int bugseg_enet_forward_bgr_ops(bugseg_ctx *ctx, const uint8_t *bgr, int B, int H, int W, int out_kind, void *out,
                                int first_op, int last_op, void *stream) {
    return enet_forward(ctx, bgr, true, B, H, W, out_kind, out, stream, first_op, last_op);
}

int bugseg_enet_forward_bgr_rows(bugseg_ctx *ctx, const uint8_t *bgr, int B, int H, int W, int out_kind, void *out,
                                 int row0, int row1, int first_op, int last_op, void *stream) {
    return enet_forward(ctx, bgr, true, B, H, W, out_kind, out, stream, first_op, last_op, row0, row1);
}

// ---- test hooks (host only: no device, no HIP call) — tests/asan drives them under ASan + UBSan
int bugseg_debug_parse_pack(const void *blob, size_t bytes, int precision, int *ncls) {
    if (!blob) return fail(nullptr, BUGSEG_EINVAL, "NULL blob");
    const int prec = precision == BUGSEG_BF16 ? PREC_BF16 : precision == BUGSEG_F16 ? PREC_F16 : PREC_F32;
    EnetWeights w;                                  // (default knobs)
    std::string why;
    if (!build_weights(blob, bytes, prec, Knobs(), w, why)) return fail(nullptr, BUGSEG_EFORMAT, "weight blob: " + why);
    if (ncls) *ncls = w.ncls;
    return BUGSEG_OK;
}

int bugseg_debug_set_spans(bugseg_ctx *ctx, void *spans, int n_ops) {
    if (!ctx) return fail(ctx, BUGSEG_EINVAL, "NULL ctx");
    if (spans && n_ops <= 0) return fail(ctx, BUGSEG_EINVAL, "spans: n_ops must be positive");
    ctx->spans = (unsigned long long *)spans;
    ctx->spans_ops = spans ? n_ops : 0;
    return BUGSEG_OK;
}

int bugseg_debug_pool_indices(bugseg_ctx *ctx, int B, int H, int W, int block, void *dst, size_t bytes, int *idx_cs,
                              void *stream) {
    if (!ctx || !dst) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    if (!ctx->loaded) return fail(ctx, BUGSEG_ESTATE, "no weights loaded");
    Plan &pl = ctx->plan;
    if (!pl.at(B, H, W)) return fail(ctx, BUGSEG_ESTATE, "no forward has run at these dimensions");
    if (block < 0 || block >= (int)pl.idx.size() || !pl.idx[(size_t)block])
        return fail(ctx, BUGSEG_EINVAL, "block " + std::to_string(block) + " is not a downsampling block");
    if (bytes != pl.idx_bytes[(size_t)block])
        return fail(ctx, BUGSEG_EINVAL, "index tensor is " + std::to_string(pl.idx_bytes[(size_t)block]) + " bytes");
    if (idx_cs) *idx_cs = cstore(ctx->w.blocks[(size_t)block].attrs[0]);
    DeviceGuard g(ctx->mem.device);
    hipError_t e = hipMemcpyAsync(dst, pl.idx[(size_t)block], bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("pool indices copy: ") + hipGetErrorString(e));
    return BUGSEG_OK;
}

int bugseg_debug_tile_walk(int ntiles, int grid, int rev, int32_t *seq, size_t seq_n, int32_t *count) {
    if (!seq || !count) return fail(nullptr, BUGSEG_EINVAL, "NULL argument");
    if (ntiles <= 0 || grid <= 0 || grid % 8 || (rev != 0 && rev != 1))
        return fail(nullptr, BUGSEG_EINVAL, "tile walk: ntiles > 0, grid a positive multiple of 8, rev 0 or 1");
    // the kernels' loop (bneck_kernels.hip, conv_kernels.hip, init_kernels.hip): steps slot, + nslots, ...
    const int nslots = grid >> 3, CH = tile_walk_ch(ntiles), per = (CH + nslots - 1) / nslots;
    if (seq_n < (size_t)grid * per) return fail(nullptr, BUGSEG_EINVAL, "tile walk: seq too small");
    for (int b = 0; b < grid; ++b) {
        const int grp = b & 7, slot = b >> 3;
        int n = 0;
        for (int it = slot; it < CH; it += nslots) {
            const int tile = tile_walk(grp, it, CH, ntiles, rev);
            if (tile < 0) break;
            // the two spellings the kernels use where scalar registers are short (bneck_kernels.hip)
            if (tile_walk_at(tile_walk_base(grp, CH, ntiles, rev), it) != tile ||
                tile_walk_flip(tile_walk_mirror(grp, CH, ntiles, rev), grp * CH + it) != tile)
                return fail(nullptr, BUGSEG_ESTATE, "tile walk: the kernels' forms disagree with tile_walk");
            seq[(size_t)b * per + n++] = tile;
        }
        count[b] = n;
        for (int k = n; k < per; ++k) seq[(size_t)b * per + k] = -1;
    }
    return per;
}

int bugseg_debug_fused_forms(int32_t *rows, int n_rows) {
    if (n_rows < 0 || (!rows && n_rows > 0)) return fail(nullptr, BUGSEG_EINVAL, "fused forms: NULL rows");
    const int nb = bneck_form_rows(rows, n_rows);
    const int left = n_rows > nb ? n_rows - nb : 0;
    return nb + up_form_rows(left ? rows + (size_t)nb * FORM_COLS : nullptr, left);
}

int bugseg_debug_row_windows(int H, int W, int row0, int row1, int tile_rows_c64, int tile_rows_c16, int32_t *win) {
    (void)W;                                          // (the windows are whole rows: the width plays no part)
    if (!win) return fail(nullptr, BUGSEG_EINVAL, "NULL argument");
    if (H <= 0 || H % 8 || W <= 0 || W % 8) return fail(nullptr, BUGSEG_EINVAL, "H and W must be positive multiples of 8");
    if (row0 < 0 || row1 > H || row0 >= row1) return fail(nullptr, BUGSEG_EINVAL, "row windows: 0 <= row0 < row1 <= H");
    if (tile_rows_c64 <= 0 || tile_rows_c16 <= 0) return fail(nullptr, BUGSEG_EINVAL, "row windows: tile rows must be positive");
    int w[WIN_OPS][2];
    row_windows(H, row0, row1, [&](int k, int, int) { return k == 4 ? tile_rows_c16 : tile_rows_c64; }, w);
    for (int k = 0; k < WIN_OPS; ++k) { win[2 * k] = w[k][0]; win[2 * k + 1] = w[k][1]; }
    return BUGSEG_OK;
}

int bugseg_debug_poison_arena(bugseg_ctx *ctx, int byte, void *stream) {
    if (!ctx) return fail(ctx, BUGSEG_EINVAL, "NULL ctx");
    Plan &pl = ctx->plan;
    if (pl.empty()) return fail(ctx, BUGSEG_ESTATE, "no forward has run");
    DeviceGuard g(ctx->mem.device);
    // activations and pooling indices; the range words after them are cleared by every forward
    hipError_t e = hipMemsetAsync(pl.arena, byte & 255, pl.act_bytes, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("poison arena: ") + hipGetErrorString(e));
    return BUGSEG_OK;
}

int bugseg_debug_stage3_windows(int h, int y0, int y1, int n, const int32_t *blk, int32_t *win) {
    if (h <= 0 || y0 < 0 || y0 >= y1 || y1 > h || n < 0 || n > 16 || (n && (!blk || !win)))
        return fail(nullptr, BUGSEG_EINVAL, "bad stage-3 walk");
    S3Desc d[16];
    int te[16], w[16][2];
    for (int k = 0; k < n; ++k) {
        d[k].asym = blk[5 * k]; d[k].d = blk[5 * k + 1]; d[k].rd = blk[5 * k + 2]; d[k].rows_full = blk[5 * k + 3];
        te[k] = blk[5 * k + 4];
    }
    const int m = stage3_windows(h, y0, y1, n, d, [&](int k, int, int) { return te[k]; }, w);
    for (int k = 0; k < m; ++k) { win[2 * k] = w[k][0]; win[2 * k + 1] = w[k][1]; }
    return m;
}

int bugseg_debug_plan_windows(bugseg_ctx *ctx, int row0, int row1, int32_t *win) {
    if (!ctx || !win) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    if (ctx->plan.empty()) return fail(ctx, BUGSEG_ESTATE, "no forward has run");
    DeviceGuard g(ctx->mem.device);
    const WinPlan *wp = window_plan(ctx, row0, row1);
    if (!wp) return 0;
    const int n = (int)ctx->plan.ops.size();
    for (int k = 0; k < wp->ns3; ++k) {
        const WinOp &r = wp->s3[k];
        const int32_t v[5] = {n - WIN_OPS - 1 - k, r.y0, r.y1, r.var, r.tiles_y * r.tiles_x * std::get<BneckLaunch>(r.l).a.phases};
        std::memcpy(win + 5 * k, v, sizeof(v));
    }
    return wp->ns3;
}

int bugseg_debug_read_block_output(bugseg_ctx *ctx, int op, void *dst_dev, size_t bytes, void *stream) {
    if (!ctx || !dst_dev) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    const Plan &pl = ctx->plan;
    if (pl.empty()) return fail(ctx, BUGSEG_ESTATE, "no forward has run");
    // where a forward leaves it (Op::fwd): the other activation buffer after an odd number of pairs; a pair's first
    // block in the spare buffer (written only when the pair was cut), its second where the pair writes
    const BneckLaunch *b = op >= 0 && op < (int)pl.ops.size() ? std::get_if<BneckLaunch>(&pl.ops[(size_t)op].fwd) : nullptr;
    if (!b || bytes != b->a.x_bytes) return fail(ctx, BUGSEG_EINVAL, "not a fused bottleneck launch, or not its output's size");
    DeviceGuard g(ctx->mem.device);
    hipError_t e = hipMemcpyAsync(dst_dev, b->a.out, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, std::string("read block output: ") + hipGetErrorString(e));
    return BUGSEG_OK;
}

int bugseg_debug_pair_walk(int n, const int32_t *cand, int first_op, int last_op, int32_t *out) {
    if (n < 0 || n > 4096 || (n && (!cand || !out)) || first_op < 0 || first_op > last_op || last_op > n)
        return fail(nullptr, BUGSEG_EINVAL, "bad pair walk");
    std::vector<PairCand> c((size_t)n);
    for (int k = 0; k < n; ++k) c[(size_t)k] = PairCand{cand[5 * k] != 0, cand[5 * k + 1], cand[5 * k + 2], cand[5 * k + 3], cand[5 * k + 4]};
    const std::vector<int> firsts = pair_firsts(c);
    std::vector<int> act((size_t)n), flip((size_t)n);
    pair_actions(n, firsts, first_op, last_op, act.data(), flip.data());
    for (int k = 0; k < n; ++k) { out[2 * k] = act[(size_t)k]; out[2 * k + 1] = flip[(size_t)k]; }
    return (int)firsts.size();
}

int bugseg_debug_pair_plan(bugseg_ctx *ctx, int32_t *rows, int cap) {
    if (!ctx || cap < 0 || (cap && !rows)) return fail(ctx, BUGSEG_EINVAL, "NULL argument");
    const Plan &pl = ctx->plan;
    if (pl.empty()) return fail(ctx, BUGSEG_ESTATE, "no forward has run");
    int th, tw, threads;
    size_t lds;
    bneck_pair_shape(th, tw, threads, lds);
    for (int k = 0; k < (int)pl.pairs.size() && k < cap; ++k) {
        const PairOp &p = pl.pairs[(size_t)k];
        const int32_t v[8] = {p.first, th, tw, p.args.a.tiles_y, p.args.a.tiles_x, threads, (int32_t)lds, p.flip};
        std::memcpy(rows + 8 * k, v, sizeof(v));
    }
    return (int)pl.pairs.size();
}

int bugseg_debug_ctx_info(const bugseg_ctx *ctx, int what, int arg) {
    if (!ctx) return -1;
    switch (what) {
    case 0: return ctx->naff_on ? 1 : 0;
    case 1: return ctx->knobs.f32_range ? 0 : 1;
    case 2: return arg >= 0 && arg < (int)ctx->w.packed.size() ? ctx->w.packed[(size_t)arg].sw : -1000;
    default: return -1;
    }
}

int bugseg_debug_knobs(const bugseg_ctx *ctx, char *buf, int len) {
    std::string err;
    const int rc = dump_knobs(ctx ? &ctx->knobs : nullptr, buf, len, err);
    return rc == BUGSEG_OK ? rc : fail(const_cast<bugseg_ctx *>(ctx), rc, err);
}

int bugseg_plan_info(bugseg_ctx *ctx, int B, int H, int W, int out_kind, int bgr_input, int *n_launches, double *alg_bytes,
                     double *plan_bytes, double *flops) {
    if (!ctx) return fail(ctx, BUGSEG_EINVAL, "NULL ctx");
    if (!ctx->loaded) return fail(ctx, BUGSEG_ESTATE, "no weights loaded");
    DeviceGuard g(ctx->mem.device);
    std::string why;
    if (!build_plan(ctx, B, H, W, why)) return fail(ctx, BUGSEG_EINVAL, why);
    double lb = 0, pb = 0, fl = 0;
    for (const Op &op : ctx->plan.ops) {
        pb += op.bytes;
        lb += op.layer();
        fl += op.flops;
    }
    // final epilogue output
    const double fin = out_kind == BUGSEG_OUT_LOGITS_F32 ? (double)B * H * W * ctx->w.ncls * 4 : (double)B * H * W;
    // class fusion: the last bottleneck's output is neither written nor read back
    if (ctx->plan.cls_ok && out_kind != BUGSEG_OUT_LOGITS_F32) {
        pb -= 2.0 * std::get<BneckLaunch>(ctx->plan.cls_fused).a.x_bytes;
    }
    // raw BGR input (bugseg_enet_forward_bgr): 3 bytes per pixel instead of the 8-channel engine input
    double adj = bgr_input ? (double)B * H * W * (8.0 * prec_es(ctx->prec) - 3.0) : 0.0;
    if (n_launches) *n_launches = (int)ctx->plan.ops.size();
    if (alg_bytes) *alg_bytes = lb + fin - adj;
    if (plan_bytes) *plan_bytes = pb + fin - adj;
    if (flops) *flops = fl;
    return BUGSEG_OK;
}

int bugseg_plan_op(bugseg_ctx *ctx, int B, int H, int W, int op, char *kernel, int kernel_len, double *alg_bytes,
                   double *plan_bytes, double *flops) {
    if (!ctx) return fail(ctx, BUGSEG_EINVAL, "NULL ctx");
    if (!ctx->loaded) return fail(ctx, BUGSEG_ESTATE, "no weights loaded");
    Plan &pl = ctx->plan;
    if (!pl.at(B, H, W)) return fail(ctx, BUGSEG_ESTATE, "no forward has run at these dimensions");
    if (op < 0 || op >= (int)pl.ops.size()) return fail(ctx, BUGSEG_EINVAL, "op index out of range");
    const Op &o = pl.ops[op];
    const int nops = (int)pl.ops.size();
    auto put = [&](const std::string &tag, double lb, double pb, double fl) {
        if (kernel && kernel_len > 0) {
            std::strncpy(kernel, tag.c_str(), (size_t)kernel_len - 1);
            kernel[kernel_len - 1] = 0;
        }
        if (alg_bytes) *alg_bytes = lb;
        if (plan_bytes) *plan_bytes = pb;
        if (flops) *flops = fl;
        return BUGSEG_OK;
    };
    if (pl.cls_on && op + 1 == nops) return put("fused", 0, 0, 0);   // ran within the previous op (class fusion)
    if (pl.cls_on && op + 2 == nops) {
        // the last bottleneck and the class layer in one launch: block input in, class map out
        const Op &l = pl.ops.back();
        const double outb = o.bneck()->a.x_bytes, fin = (double)B * H * W;
        return put("bneck C16+classes 16x16", o.layer() + l.layer() + fin, o.bytes - outb + (l.bytes - outb) + fin, o.flops + l.flops);
    }
    std::string tag;
    if (const UpLaunch *u = o.up()) {
        tag = "up C" + std::to_string(u->cout);
    } else if (const BneckLaunch *b = o.bneck()) {
        int th, tw, nw;
        bneck_shape(b->C, b->var, th, tw, nw, nullptr);
        tag = std::string(b->cin ? "down C" : b->var == BNECK2_V && b->C == 128 ? "bneck2 C" : "bneck C") +
              std::to_string(b->C) + (b->asym ? " asym" : "") + " " + std::to_string(th) + "x" + std::to_string(tw);
    }
    else if (o.epi(EPI_INIT)) tag = "init";
    else if (o.class_kernel()) tag = "classes";
    else tag = "conv NR" + std::to_string(o.conv()->nr) + " E" + std::to_string(o.conv()->epi);
    double adj = 0;
    if (o.epi(EPI_INIT) && pl.bound.bgr)                  // raw BGR input: 3 B/px, not the 8-channel engine input
        adj = -(double)B * H * W * (8.0 * prec_es(ctx->prec) - 3.0);
    if (o.epi(EPI_CLASSES))                               // the output the last forward asked for
        adj = pl.bound.in && pl.bound.out_kind == BUGSEG_OUT_LOGITS_F32 ? (double)B * H * W * ctx->w.ncls * 4 : (double)B * H * W;
    return put(tag, o.layer() + adj, o.bytes + adj, o.flops);
}

int bugseg_plan_launch_op(bugseg_ctx *ctx, int B, int H, int W, int op, void *stream) {
    if (!ctx) return fail(ctx, BUGSEG_EINVAL, "NULL ctx");
    if (!ctx->loaded) return fail(ctx, BUGSEG_ESTATE, "no weights loaded");
    Plan &pl = ctx->plan;
    if (!pl.at(B, H, W) || !pl.bound.in)
        return fail(ctx, BUGSEG_ESTATE, "no forward has run at these dimensions");
    if (op < 0 || op >= (int)pl.ops.size()) return fail(ctx, BUGSEG_EINVAL, "op index out of range");
    DeviceGuard g(ctx->mem.device);
    hipError_t e = launch_op(ctx, op, (hipStream_t)stream);
    if (e != hipSuccess) return fail(ctx, BUGSEG_EHIP, "launch of op " + std::to_string(op) + ": " + hipGetErrorString(e));
    return BUGSEG_OK;
}

}  // extern "C"
