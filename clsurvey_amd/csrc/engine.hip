// Static-plan executor for the reference's feature-extractor / classifier nets:
//   [conv (any square kernel / stride / pad) (+BatchNorm2d) (+ReLU) (+max-pool)]* -> [(Dropout) Linear (+ReLU)]*
// i.e. VGGSlim and its _BN / _DROP variants (models/VGGSlim.py:27-76) and torchvision's AlexNet (models/net.py:96-125).
// 3x3 stride-1 pad-1 layers take the conv3x3.hip fast path (fused ReLU + 2x2 pool forward, fused un-pool first-layer weight gradient, one
// deferred reduction launch for all weight-gradient slabs); everything else runs through the general kernels (conv2d.hip, pool.hip,
// bn.hip).  Side inputs per layer: dropout mask rows, an extra gradient for side branches (EBLL's code layers), BatchNorm running buffers.
//
// The reference trains through nn.Sequential + autograd, one Python dispatch per op per batch (EWC/train_EWC.py:181-189).  At N=200 a
// small_VGG9 step is < 1.5 ms of MFMA work, so the op sequence is planned once and every forward / loss / backward pass is ONE call that
// enqueues its launches (17 for a small_VGG9 loss step) on the caller's stream with all ReLU backward passes fused into the
// producing backward-data kernels.  The plan holds only shapes and offsets; parameters, gradients and the activation workspace are
// caller-owned device memory (torch allocations).  clhip_net_create decides ONCE what every layer runs (choose_paths); the passes
// launch from one place per kind of launch (launch_conv_fwd, launch_conv_bwd_data, launch_wgrad, conv_layer's one_grid).
#include <vector>
#include <cstdlib>
#include <memory>
#include <new>
#include "common.hpp"

namespace {

// the kernel of a conv layer's forward or backward-data launch
enum class Conv : unsigned char {
    None,       // no launch (backward-data of layer 0)
    Direct3,    // direct f32 3x3 (conv3x3.hip)
    Wino,       // Winograd F(2x2,3x3) (wino.hip), weights transformed per pass
    Bs3,        // 3x3 on the bf16 matrix cores with split fp32 operands (bsconv.hip), weight image built per pass
    Bs5,        // 5x5 / stride 1 / padding 2 on the same (bsconv.hip)
    S2d,        // strided first layer through space-to-depth + the dense 3x3 kernels (s2dconv.hip); forward only
    Gemm,       // general gather-GEMM (conv2d.hip)
};
// weights prepared once per pass for one direction of a layer (wino_prepare / the first layer's merged grid)
enum class Img : unsigned char { None, WinoU, Bs3, Bs5 };
struct WeightImage { Img kind; size_t off; };       // off: bytes into the plan's image region (off_wino)
// weight-gradient candidates of a conv layer, tried in this order (launch_wgrad); a kernel may decline a call at run time
enum : unsigned {
    WG_BS = 1,      // bf16-split slabs (bswgrad.hip), deferred reduction
    WG_WINO = 2,    // Winograd slabs (wino.hip), deferred reduction
    WG_3X3 = 4,     // direct 3x3 kernel: slabs under the deferred reduction, else reduced right away (without it: the gather-GEMM)
    WG_BS5 = 8,     // 5x5 bf16-split (bswgrad5.hip; slabs in the plan's scratch)
    WG_S2D = 16,    // space-to-depth frames of the forward pass (s2dconv.hip)
};

struct LayerPlan {
    int type;              // 0 conv, 1 fc
    int cin, cout, relu, pool;
    long w_off, b_off;     // float offsets into the parameter / gradient arenas
    int h, w;              // conv: input spatial size
    int ks, st, pd;        // conv kernel / stride / pad
    int oh, ow;            // conv output size
    int pk, ps;            // pool window / stride
    int ph, pw;            // pooled size
    bool vgg;              // 3x3 / stride 1 / pad 1: the conv3x3.hip / wino.hip / bsconv.hip fast paths
    bool pool22;           // pooled with a 2x2 stride-2 window (pool.hip's 2-bit fast path, the fused un-pooling kernels)
    bool fused_pool;       // conv + ReLU + 2x2 pool go out as ONE forward launch that marks dead windows in the arg-max bytes: the
                           // next layer's backward-data needs no ReLU mask (CLHIP_POOL_DEAD, common.hpp)
    size_t in_elems, out_elems, pool_elems;   // per image
    size_t act_off;        // float offset of this layer's OUTPUT (post-ReLU, pre-pool) in ws
    size_t pool_off;       // float offset of pooled output
    size_t idx_off;        // byte offset of pool argmax
    int bn;                // BatchNorm2d between conv and ReLU
    long bn_w_off, bn_b_off;
    size_t z_off;          // bn: float offset of the convolution output (pre-BatchNorm) in ws
    size_t stat_off;       // bn: float offset of save_mean[cout], save_invstd[cout]
    float* rmean; float* rvar; float bn_momentum, bn_eps;
    Conv fwd, bwd;               // forward / backward-data kernel
    WeightImage img_f, img_d;    // ... and the prepared weights it reads
    unsigned wg;                 // WG_* candidates of the weight gradient
    size_t wg_off, wg_bytes;     // this layer's own weight-gradient slabs (WG_BS / WG_WINO / WG_3X3; reduced for all layers at once)
    size_t s2d_off, s2d_bytes;   // Conv::S2d: this layer's frames in the plan's space-to-depth region
    size_t scratch_need;         // the most any of this layer's launches asks of the plan's shared scratch
    const float* extra_grad;   // added to the gradient w.r.t. this layer's input (side branches: clhip_net_set_input_grad)
    const float* drop;     // dropout mask applied to this layer's INPUT (NULL = none); see clhip_net_set_dropout
    long drop_stride;      // floats between the mask rows of consecutive samples (0 = one row shared by the batch)
    int has_drop_buf;      // the masked input gets its own buffer (the un-masked activation stays readable: side branches)
    size_t drop_off;       // float offset of that buffer in ws
};

constexpr long long WINO_MIN_UNITS = 640;
constexpr long long WINO16_MIN_UNITS = 384;      // waves of the 8 x 8 variant (wino.hip, wino_conv16_kernel)
constexpr unsigned PROBE_RING = 64;
#ifndef CLHIP_EDGE_GRIDS_DEFAULT
#define CLHIP_EDGE_GRIDS_DEFAULT 1
#endif
#ifndef CLHIP_REDUCE_RIDERS_DEFAULT
#define CLHIP_REDUCE_RIDERS_DEFAULT 1
#endif
#ifndef CLHIP_OVERLAP_DEFAULT
#define CLHIP_OVERLAP_DEFAULT 0
#endif

// The environment switches of the executor, all read while a plan is created.
bool env_starts(const char* name, char c) { const char* e = std::getenv(name); return e && e[0] == c; }
bool wino_enabled() { return !env_starts("CLHIP_WINO", '0'); }           // =0: every layer off the Winograd kernels (A/B measurements, triage)
bool bs5_wgrad_enabled() { return !env_starts("CLHIP_BS_WGRAD", '0'); }  // =0: no bf16-split weight gradient on the 5x5 layers
bool s2d_enabled() { return env_starts("CLHIP_S2D", '1'); }              // =1: a strided first layer over phase planes (choose_paths)
bool fc_tail_enabled() { return !env_starts("CLHIP_FC_TAIL", '0'); }     // =0: per-layer classifier launches (the bitwise reference of the fused tail)
// CLHIP_WGRAD_OVERLAP=1 / 2 (make_resources), CLHIP_EDGE_GRIDS=0 / 1 / 2 (NetPlan::edge_grids), CLHIP_REDUCE_RIDERS=0 .. 3 (NetPlan::reduce_riders)
int overlap_mode() { return env_starts("CLHIP_WGRAD_OVERLAP", '1') ? 1 : env_starts("CLHIP_WGRAD_OVERLAP", '2') ? 2 : CLHIP_OVERLAP_DEFAULT; }
int edge_grids_mode() {
    const char* e = std::getenv("CLHIP_EDGE_GRIDS");
    return (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : CLHIP_EDGE_GRIDS_DEFAULT;
}

int reduce_riders_mode() {
    const char* e = std::getenv("CLHIP_REDUCE_RIDERS");
    return (e && e[0] >= '0' && e[0] <= '3' && !e[1]) ? e[0] - '0' : CLHIP_REDUCE_RIDERS_DEFAULT;
}
// tuning switch (tools/experiments): rider blocks of the host launch, a multiple of 256
int reduce_rider_blocks() {
    const char* e = std::getenv("CLHIP_REDUCE_RIDER_BLOCKS");
    const int v = e && e[0] ? std::atoi(e) : 0;
    return (v > 0 && v % 256 == 0 && v <= 16384) ? v : 256;
}

struct NetPlan {
    std::vector<LayerPlan> layers;
    int max_batch, in_c, in_h, in_w, n_classes;
    size_t in_elems;
    size_t scratch_bytes;    // wgrad / fc split-K scratch
    size_t wino_bytes;       // prepared weights (Winograd U, bf16-split images) of every layer: one region, filled once per pass
    size_t off_wino;
    size_t off_s2d;         // frames of the space-to-depth first layer (its own region: the phase planes of the forward pass feed the
    int s2d_fresh_n;         // weight gradient of the same pass; s2d_fresh_n = the batch they were made for, 0 = stale)
    size_t total_bytes;
    // derived offsets (bytes) inside ws
    size_t off_acts, off_idx, off_g0, off_g1, off_scratch, off_dlogits, off_loss, off_fcdz, off_wg;
    int training = 1;        // BatchNorm: batch statistics (1) or running statistics (0)
    int n_wg;                // conv layers with slabs of their own under the deferred reduction (0: every layer reduces right away)
    // classifier = trailing Linear layers [fc_first, end): fused into three launches when it fits fc_chain.hip
    int fc_first;
    bool fc_fused;
    clhip_fc_chain chain;
    size_t fcdz_floats;      // dz slots of the hidden Linear layers
    // measurement probe (clhip_net_probe): HIP events around the forward launch(es) of one layer, a ring of PROBE_RING
    // pairs so that recording never waits for the GPU
    int probe_layer = -1;
    int probe_kind;          // 0 forward, 1 backward-data, 2 weight-gradient launch(es) of probe_layer
    unsigned probe_count;
    std::vector<hipEvent_t> probe_ev;
    // layers fc_first+1 .. end forward + cross-entropy + backward-data down to dz(h1) in one launch (fc_tail_kernel); the
    // arrival counter of its last-workgroup reduction is the plan's own 4 bytes of device memory (zero between launches),
    // so a plan must not run on two streams at once (it never could: the activations live in one workspace)
    bool fc_tail, no_combo;
    unsigned* tail_counter;
    size_t off_rows;
    // CLHIP_EDGE_GRIDS (default 1): the prepared-weights launch of a pass runs as blocks of the first layer's forward grid where that
    // layer is on conv3x3_c3w64_relu_pool_kernel (net_forward_impl).  0: the launch of its own (the bitwise A/B reference);
    // 1 / 2: weight blocks at the end / at the front of the merged grid (both measured, DESIGN 9: the end is the faster side)
    int edge_grids;
    unsigned edge_count;     // merged launches issued so far (clhip_net_edge_grid_count: tests tell the merged grid from its fallback)
    // CLHIP_REDUCE_RIDERS (default 1): the weight-gradient slabs that are complete when the LAST bf16-split backward-data launch of a
    // pass is issued (layer rider_host: the lowest conv layer > 0 whose backward-data is Conv::Bs3; -1: none) are reduced by rider
    // blocks of that launch (bsconv.hip, bs_conv_riders_kernel); the reduction launch of the pass keeps what is left, the first
    // layer's slabs.  0: every slab in the reduction launch (the bitwise A/B reference); 1 / 2 / 3: riders in front of / behind /
    // spread through the convolution blocks (all measured, DESIGN 9: in front is the only order faster than the two launches)
    int reduce_riders, rider_blocks, rider_host = -1;
    unsigned rider_count;    // backward passes whose host launch carried riders (clhip_net_reduce_rider_count)
    // backward (optional, CLHIP_WGRAD_OVERLAP): the weight-gradient launches of the conv layers run on a side stream
    // next to the backward-data launch of the same layer (both only read dy)
    bool overlap;
    int overlap_mode;        // 0 off, 1 every conv layer (CLHIP_WGRAD_OVERLAP=1), 2 only layers whose launches under-fill the chip
    hipStream_t side;
    std::vector<hipEvent_t> ev_dy, ev_wg;      // per layer: dy ready (main -> side), weight gradient done (side -> main)
    ~NetPlan() {
        for (hipEvent_t e : ev_dy) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_wg) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
        if (tail_counter) (void)hipFree(tail_counter);
        for (hipEvent_t e : probe_ev) (void)hipEventDestroy(e);
    }
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t max_of(size_t a, size_t b) { return a > b ? a : b; }

// h[n][f] *= mask[n * stride + f]: nn.Dropout in training mode with a caller-drawn mask (already divided by the
// retain probability), or GEM's one-row-per-observe masks (stride 0).  HBM-bound, in place.
__global__ void drop_scale_kernel(float* __restrict__ h, const float* __restrict__ mask, long stride, int feat, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / feat, f = i - n * feat;
        h[i] *= mask[n * stride + f];
    }
}

__global__ void add_inplace_kernel(float* __restrict__ a, const float* __restrict__ b, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] += b[i];
}

int add_inplace(float* a, const float* b, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(add_inplace_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, s, a, b, n);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

__global__ void drop_copy_kernel(const float* __restrict__ h, float* __restrict__ out, const float* __restrict__ mask, long stride,
                                 int feat, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / feat, f = i - n * feat;
        out[i] = h[i] * mask[n * stride + f];
    }
}

int drop_copy(const float* h, float* out, const float* mask, long stride, size_t feat, int N, hipStream_t s) {
    const size_t total = feat * N;
    hipLaunchKernelGGL(drop_copy_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, s, h, out, mask, stride, (int)feat, total);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int drop_scale(float* h, const float* mask, long stride, size_t feat, int N, hipStream_t s) {
    const size_t total = feat * N;
    hipLaunchKernelGGL(drop_scale_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, s, h, mask, stride, (int)feat, total);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

// clhip_net_create in pieces: geometry, kernel choice, arena layout (with the classifier chain), runtime resources.
// Shapes of every layer from the descriptors; CLHIP_EINVAL for a net the plan does not cover
int plan_geometry(NetPlan& p, const clhip_layer_desc* descs, int n_layers) {
    int c = p.in_c, h = p.in_h, w = p.in_w;
    size_t feat = p.in_elems;
    bool seen_fc = false;
    for (int i = 0; i < n_layers; ++i) {
        const clhip_layer_desc& d = descs[i];
        LayerPlan L{};
        L.type = d.type; L.cin = d.cin; L.cout = d.cout; L.relu = d.relu; L.pool = d.pool; L.w_off = d.w_off; L.b_off = d.b_off;
        if (L.type == 0) {
            if (seen_fc || L.cin != c) return CLHIP_EINVAL;
            L.h = h; L.w = w;
            L.ks = d.ksize > 0 ? d.ksize : 3;
            L.st = d.ksize > 0 ? d.stride : 1;
            L.pd = d.ksize > 0 ? d.pad : 1;
            if (L.st < 1 || L.pd < 0) return CLHIP_EINVAL;
            L.oh = (h + 2 * L.pd - L.ks) / L.st + 1; L.ow = (w + 2 * L.pd - L.ks) / L.st + 1;
            if (L.oh <= 0 || L.ow <= 0) return CLHIP_EINVAL;
            L.vgg = L.ks == 3 && L.st == 1 && L.pd == 1;
            L.in_elems = (size_t)c * h * w;
            L.out_elems = (size_t)L.cout * L.oh * L.ow;
            L.bn = d.bn ? 1 : 0; L.bn_w_off = d.bn_w_off; L.bn_b_off = d.bn_b_off;
            L.bn_momentum = 0.1f; L.bn_eps = 1e-5f;
            h = L.oh; w = L.ow;
            if (L.pool) {
                L.pk = d.pool_k > 0 ? d.pool_k : 2;
                L.ps = d.pool_k > 0 ? d.pool_s : 2;
                L.pool22 = L.pk == 2 && L.ps == 2;
                if (L.ps < 1 || h < L.pk || w < L.pk) return CLHIP_EINVAL;
                if (L.pool22 && ((h & 1) || (w & 1))) return CLHIP_EINVAL;
                L.ph = (h - L.pk) / L.ps + 1; L.pw = (w - L.pk) / L.ps + 1;
                L.pool_elems = (size_t)L.cout * L.ph * L.pw;
                h = L.ph; w = L.pw;
            }
            L.fused_pool = L.vgg && !L.bn && L.pool22 && L.relu;
            c = L.cout;
            feat = (size_t)c * h * w;
        } else if (L.type == 1) {
            seen_fc = true;
            if ((size_t)L.cin != feat) return CLHIP_EINVAL;
            L.in_elems = feat; L.out_elems = (size_t)L.cout;
            L.scratch_need = clhip_fc_ws(p.max_batch, L.cin, L.cout);
            feat = L.out_elems;
        } else return CLHIP_EINVAL;
        L.has_drop_buf = (d.has_drop && i > 0) ? 1 : 0;
        p.layers.push_back(L);
    }
    p.n_classes = (int)feat;
    return 0;
}

// What conv layer `layer` runs: the kernel of each direction, the weights prepared for it, the weight-gradient candidates and the
// sizes of the regions they need.  This is the only place that decides; the passes read L.fwd / L.bwd / L.img_* / L.wg.
void choose_paths(LayerPlan& L, const clhip_layer_desc& d, int layer, int max_batch) {
    // 3x3 layers whose rows are not 16-byte aligned (AlexNet's 13x13 maps) would take the scalar-staging variant of
    // the 3x3 weight-gradient kernel with 16x4-pixel tiles (169 of 256 slots): the dense gather-GEMM is 1.8x faster
    // there (measured 83 vs 46 TFLOP/s)
    const bool wg3 = L.vgg && (L.w % 4 == 0 || L.cin * 9 <= 32);
    const size_t s = wg3 ? clhip_conv3x3_bwd_weight_ws(max_batch, L.cin, L.cout, L.h, L.w)
                         : clhip_conv2d_bwd_weight_ws(max_batch, L.cin, L.h, L.w, L.cout, L.ks, L.ks, L.st, L.pd);
    L.scratch_need = max_of(s, L.bn ? clhip_bn_ws(L.cout) : 0);
    if (wg3) { L.wg = WG_3X3; L.wg_bytes = align_up(s, 256); }
    L.fwd = L.vgg ? Conv::Direct3 : Conv::Gemm;
    L.bwd = layer == 0 ? Conv::None : L.fwd;
    if (L.vgg && !L.bn) {
        // Winograd path: 2.25x fewer matrix instructions, but a wave's work unit is 32 channels x 32 TILES (128 pixels) with 256 accumulator
        // registers, one wave per SIMD: it needs enough units to fill most of the 1024 SIMDs (measured at N = 200: 64->64 @16x16, 800 units,
        // 1.26x the direct kernel; 128->128 @8x8, 400 units, 0.8x)
        const long long tiles = (long long)max_batch * ((L.h + 1) / 2) * ((L.w + 1) / 2);
        auto units = [&](int kout) { return ((tiles + 31) / 32) * ((kout + 31) / 32); };
        // (8 x 8 maps: the 16x16x4-MFMA variant has 16-tile units, one image x 32 channels per wave)
        auto enough = [&](int kout) {
            if (units(kout) >= WINO_MIN_UNITS) return true;
            return L.h == 8 && L.w == 8 && (long long)max_batch * ((kout + 31) / 32) >= WINO16_MIN_UNITS;
        };
        const bool wino = wino_enabled();
        if (wino && clhip_internal_wino_ok(L.cin, L.cout, L.h, L.w) && enough(L.cout)) L.fwd = Conv::Wino;
        if (wino && layer > 0 && clhip_internal_wino_ok(L.cout, L.cin, L.h, L.w) && enough(L.cin)) L.bwd = Conv::Wino;
        // bf16 matrix cores with split fp32 operands (bsconv.hip) where that path is the faster one (large maps: see clhip_internal_bs_preferred;
        // CLHIP_BS=0 turns it off, =2 takes it wherever it can run); fused 2x2 pooling only exists on even maps there
        const bool even = ((L.h | L.w) & 1) == 0;
        if (clhip_internal_bs_preferred(L.cin, L.cout, L.h, L.w) && (even || !L.pool)) L.fwd = Conv::Bs3;
        if (layer > 0 && clhip_internal_bs_preferred(L.cout, L.cin, L.h, L.w) && (even || !L.pool)) L.bwd = Conv::Bs3;
        // Winograd weight gradient (wino.hip picks the tile split by the stages per block itself); its slabs live in this layer's
        // weight-gradient region (AlexNet's 13x13 layers get one for it: their direct path is the gather-GEMM, which has no slabs)
        if (wino && clhip_internal_wino_wgrad_ok(L.cin, L.cout, L.h, L.w)) {
            L.wg |= WG_WINO;
            L.wg_bytes = max_of(L.wg_bytes, align_up(clhip_internal_wino_wgrad_ws(max_batch, L.cin, L.cout, L.h, L.w), 256));
        }
        // ... or on the bf16 matrix cores with split fp32 operands (bswgrad.hip) where that is the faster launch and the layer's
        // backward is not one merged grid (BackwardPass::one_grid): its slabs live in the same region
        const bool merged = L.bwd == Conv::Wino && (L.wg & WG_WINO) && L.wg_bytes &&
                            clhip_internal_wino_pair_shape(max_batch, L.cin, L.cout, L.h, L.w, L.pool22 ? 1 : 0);
        if (!merged && clhip_internal_bs_wgrad_preferred(L.cin, L.cout, L.h, L.w, L.pool22 ? 1 : 0)) {
            const size_t bw = clhip_internal_bs_wgrad_ws(max_batch, L.cin, L.cout, L.h, L.w);
            if (bw && wg3) { L.wg |= WG_BS; L.wg_bytes = max_of(L.wg_bytes, align_up(bw, 256)); }
        }
        L.img_f.kind = L.fwd == Conv::Wino ? Img::WinoU : L.fwd == Conv::Bs3 ? Img::Bs3 : Img::None;
        L.img_d.kind = L.bwd == Conv::Wino ? Img::WinoU : L.bwd == Conv::Bs3 ? Img::Bs3 : Img::None;
    }
    // 5 x 5 / stride 1 / padding 2 layers (AlexNet's second convolution) on the bf16-split kernels
    if (!L.vgg && !L.bn && L.ks == 5 && L.st == 1 && L.pd == 2) {
        if (clhip_internal_bs5_preferred(L.cin, L.cout, L.h, L.w)) { L.fwd = Conv::Bs5; L.img_f.kind = Img::Bs5; }
        if (layer > 0 && clhip_internal_bs5_preferred(L.cout, L.cin, L.h, L.w)) { L.bwd = Conv::Bs5; L.img_d.kind = Img::Bs5; }
        // weight gradient: 372 us against the gather-GEMM's 589 at N = 128 (profiles/r06_x_bswgrad5.txt)
        const size_t w5 = bs5_wgrad_enabled() ? clhip_internal_bs5_wgrad_ws(max_batch, L.cin, L.cout, L.h, L.w) : 0;
        if (w5) { L.wg |= WG_BS5; L.scratch_need = max_of(L.scratch_need, w5); }
    }
    // AlexNet's 11 x 11 / stride-4 first layer as a dense 3x3 convolution over the 48 phase planes of the padded input
    // (s2dconv.hip), CLHIP_S2D=1.  Off by default: measured at N = 128 (profiles/r06_l_alexnet_s2d.txt) the dense kernels take
    // 159 (forward) and 192 us (weight gradient) but building the frames and cropping the output costs 64 + 62 + 45 us more —
    // 285 / 237 us against the gather-GEMM's 257 / 217; the step 4.72 against 4.69 ms.  First layer only: no backward-data.
    if (!L.vgg && !L.bn && layer == 0 && !d.has_drop) {
        const size_t sb = s2d_enabled() ? clhip_conv2d_s2d_ws(max_batch, L.cin, L.h, L.w, L.cout, L.ks, L.st, L.pd) : 0;
        if (sb) { L.fwd = Conv::S2d; L.wg |= WG_S2D; L.s2d_bytes = align_up(sb, 256); }
    }
}

size_t image_bytes(Img kind, int cin, int cout) {
    return kind == Img::WinoU ? clhip_internal_wino_ws(cin, cout) : kind == Img::Bs3 ? clhip_internal_bs_ws(cin, cout)
         : kind == Img::Bs5 ? clhip_internal_bs5_ws(cin, cout) : 0;
}

// trailing Linear layers as one clhip_fc_chain (needs the layers' act_off); fc_fused when fc_chain.hip takes it
void plan_classifier(NetPlan& p) {
    const int n_layers = (int)p.layers.size();
    p.fc_first = n_layers;
    for (int i = 0; i < n_layers; ++i) if (p.layers[i].type == 1) { p.fc_first = i; break; }
    const int nfc = n_layers - p.fc_first;
    if (nfc < 1 || nfc > CLHIP_FC_MAX) return;
    clhip_fc_chain& ch = p.chain;
    ch.n = nfc;
    size_t dzf = 0;
    for (int l = 0; l < nfc; ++l) {
        const LayerPlan& L = p.layers[p.fc_first + l];
        ch.w_off[l] = L.w_off; ch.b_off[l] = L.b_off; ch.din[l] = L.cin; ch.dout[l] = L.cout; ch.relu[l] = L.relu;
        ch.act_off[l] = L.act_off;
        ch.dz_off[l] = dzf;
        if (l < nfc - 1) dzf += (size_t)L.cout * p.max_batch;
    }
    p.fcdz_floats = dzf;
    p.fc_fused = clhip_internal_fc_chain_ok(&ch) != 0;
}

// offsets of everything in the caller's workspace: per layer inside the regions (layer order), then the regions themselves
void layout_arena(NetPlan& p) {
    const size_t N = p.max_batch;
    size_t acts = 0, idxb = 0, gmax = 0, scratch = 0, imgs = 0, wg_total = 0, s2d_total = 0;
    for (LayerPlan& L : p.layers) {
        if (L.bn) {
            L.z_off = acts; acts += L.out_elems * N;
            L.stat_off = acts; acts += align_up(2 * (size_t)L.cout, 4);
        }
        L.act_off = acts; acts += L.out_elems * N;
        if (L.type == 0 && L.pool) {
            L.pool_off = acts; acts += L.pool_elems * N;
            L.idx_off = idxb; idxb += align_up(L.pool_elems * N, 256);
        }
        if (L.has_drop_buf) { L.drop_off = acts; acts += L.in_elems * N; }
        // own slabs per layer so that ONE launch reduces them all at the end of backward (HBM is plentiful: 288 GB)
        if (L.wg & (WG_3X3 | WG_WINO)) { L.wg_off = wg_total; wg_total += L.wg_bytes; ++p.n_wg; }
        // every layer keeps its own prepared weights: ONE launch per pass fills them all
        if (L.img_f.kind != Img::None) { L.img_f.off = imgs; imgs += align_up(image_bytes(L.img_f.kind, L.cin, L.cout), 256); }
        if (L.img_d.kind != Img::None) { L.img_d.off = imgs; imgs += align_up(image_bytes(L.img_d.kind, L.cout, L.cin), 256); }
        if (L.fwd == Conv::S2d) { L.s2d_off = s2d_total; s2d_total += L.s2d_bytes; }
        scratch = max_of(scratch, L.scratch_need);
        gmax = max_of(gmax, max_of(L.in_elems, L.out_elems));
    }
    p.scratch_bytes = scratch; p.wino_bytes = imgs;
    plan_classifier(p);
    size_t off = 0;
    p.off_acts = off; off += align_up(acts * 4, 256);
    p.off_idx = off; off += align_up(idxb, 256);
    p.off_g0 = off; off += align_up(gmax * N * 4, 256);          // two ping-pong gradient buffers
    p.off_g1 = off; off += align_up(gmax * N * 4, 256);
    p.off_scratch = off; off += align_up(scratch, 256);
    p.off_wino = off; off += align_up(imgs, 256);
    p.off_dlogits = off; off += align_up(N * p.n_classes * 4, 256);
    p.off_loss = off; off += 256;
    p.off_fcdz = off;
    if (p.fc_fused) {
        off += align_up(p.fcdz_floats * 4 + 256, 256);
        p.off_rows = off;                        // per-row loss / hit of the fused classifier tail
        off += align_up(N * 8, 256);
    }
    p.off_wg = off;
    if (p.n_wg < 2 || p.n_wg > CLHIP_WGRAD_JOBS_MAX) p.n_wg = 0;
    if (p.n_wg) off += align_up(wg_total, 256);
    p.off_s2d = off; off += s2d_total;
    p.total_bytes = off;
}

// side stream and events of the weight-gradient overlap, arrival counter of the fused classifier tail: both need a device, and
// plans made on a host without one (shape tests) simply stay single-stream / keep the per-layer launches
void make_resources(NetPlan& p) {
    // Measured on small_VGG9 (N = 200): 2.59 ms per bench step with the overlap against 2.45 ms without (the two MFMA-bound kernels only
    // take slots from each other); AlexNet N = 128: 9.65 vs 9.76 ms.  Hence off unless CLHIP_WGRAD_OVERLAP=1; results are identical either
    // way (same kernels, same order per stream).  Round 2 tried the side stream for the DEEP layers only (planes of 16x16 and smaller at
    // batch 200: ~400 blocks, 1.5 per CU, SIMD time left unused) with the slab reductions still deferred: 2.125 against 2.076 ms per step —
    // the event hand-offs and the two launches taking each other's slots cost more than the idle time they fill.  So: off by default;
    // CLHIP_WGRAD_OVERLAP=1 every conv layer, =2 the deep layers only.
    const size_t n_layers = p.layers.size();
    bool any_bn = false;
    for (const LayerPlan& L : p.layers) any_bn = any_bn || L.bn;
    p.overlap_mode = overlap_mode();
    if (p.overlap_mode && !any_bn) {         // BatchNorm backward shares `scratch` with the weight-gradient launches
        if (hipStreamCreateWithFlags(&p.side, hipStreamNonBlocking) == hipSuccess) {
            p.overlap = true;
            p.ev_dy.resize(n_layers); p.ev_wg.resize(n_layers);
            for (size_t i = 0; i < n_layers && p.overlap; ++i)
                if (hipEventCreateWithFlags(&p.ev_dy[i], hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&p.ev_wg[i], hipEventDisableTiming) != hipSuccess) p.overlap = false;
        } else { (void)hipGetLastError(); p.side = nullptr; }
    }
    p.edge_grids = edge_grids_mode();
    p.reduce_riders = reduce_riders_mode();
    p.rider_blocks = reduce_rider_blocks();
    for (size_t i = n_layers; i-- > 1;)
        if (p.layers[i].type == 0 && p.layers[i].bwd == Conv::Bs3) p.rider_host = (int)i;
    const bool tail = fc_tail_enabled();
    p.no_combo = !tail;
    if (p.fc_fused && tail && clhip_internal_fc_tail_ok(&p.chain) && p.max_batch <= 1024) {
        if (hipMalloc(reinterpret_cast<void**>(&p.tail_counter), 256) == hipSuccess &&
            hipMemset(p.tail_counter, 0, 256) == hipSuccess) {
            p.fc_tail = true;
        } else {
            (void)hipGetLastError();
            if (p.tail_counter) { (void)hipFree(p.tail_counter); p.tail_counter = nullptr; }
        }
    }
}

static bool tail_usable(const NetPlan* p, const float* params, const void* ws, int N) {
    if (!p->fc_tail) return false;
    for (size_t i = p->fc_first + 1; i < p->layers.size(); ++i)
        if (p->layers[i].drop || p->layers[i].extra_grad) return false;
    const float* acts = reinterpret_cast<const float*>(static_cast<const char*>(ws) + p->off_acts);
    return aligned16(params + p->chain.w_off[1]) && aligned16(params + p->chain.w_off[2]) && aligned16(acts + p->chain.act_off[0]) &&
           aligned16(params + p->chain.b_off[0]) && (size_t)N * (p->n_classes | 1) <= 12288;        // the range in which the per-layer path uses softmax_ce_rows_lds_kernel
}

// what the launches of one pass share: the plan, the caller's buffers and stream, the regions of the workspace
struct Pass {
    NetPlan* p; const float* params; int N; void* stream; char* base; float* acts; uint8_t* idx; void* scratch;
    Pass(NetPlan* plan, const float* prm, int n, void* ws, void* st)
        : p(plan), params(prm), N(n), stream(st), base(static_cast<char*>(ws)), acts(reinterpret_cast<float*>(base + plan->off_acts)),
          idx(reinterpret_cast<uint8_t*>(base + plan->off_idx)), scratch(base + plan->off_scratch) {}
    hipStream_t s() const { return as_stream(stream); }
    float* image(const WeightImage& im) const { return reinterpret_cast<float*>(base + p->off_wino + im.off); }
};

// the prepared-weights 3x3 convolution of a layer: Winograd (wino.hip) or bf16-split (bsconv.hip), same arguments
static int plan_conv_u(Conv kind, int mode, const float* in, const float* U, const float* bias, const float* mask_src, float* out,
                       uint8_t* pool_idx, int unpool, int N, int Cin, int Cout, int H, int W, int relu, hipStream_t s) {
    return kind == Conv::Bs3 ? clhip_internal_bs_conv_u(mode, in, U, bias, mask_src, out, pool_idx, unpool, N, Cin, Cout, H, W, relu, s)
                             : clhip_internal_wino_conv_u(mode, in, U, bias, mask_src, out, pool_idx, unpool, N, Cin, Cout, H, W, relu, s);
}

// Forward launch of a conv layer: out = conv(in) + bias (+ ReLU).  pool_idx (fused_pool layers): the launch pools 2x2 as well, `out`
// is the pooled map and pool_idx receives the arg-max bytes; the pre-pool tensor is never materialised.
static int launch_conv_fwd(const Pass& c, const LayerPlan& L, const float* in, float* out, uint8_t* pool_idx, int relu) {
    const float* w = c.params + L.w_off; const float* b = c.params + L.b_off;
    switch (L.fwd) {
    case Conv::Wino: case Conv::Bs3:
        return plan_conv_u(L.fwd, 0, in, c.image(L.img_f), b, nullptr, out, pool_idx, 0, c.N, L.cin, L.cout, L.h, L.w, relu, c.s());
    case Conv::Direct3:
        return pool_idx ? clhip_conv3x3_relu_pool_fwd(in, w, b, out, pool_idx, c.N, L.cin, L.cout, L.h, L.w, c.stream)
                        : clhip_conv3x3_fwd(in, w, b, out, c.N, L.cin, L.cout, L.h, L.w, relu, c.stream);
    case Conv::Bs5:
        return clhip_internal_bs5_conv_u(0, in, c.image(L.img_f), b, nullptr, out, c.N, L.cin, L.cout, L.h, L.w, relu, c.s());
    case Conv::S2d:
        return clhip_conv2d_s2d_fwd(in, w, b, out, c.N, L.cin, L.h, L.w, L.cout, L.ks, L.st, L.pd, relu, c.base + c.p->off_s2d + L.s2d_off,
                                    L.s2d_bytes, c.stream);
    default:
        return clhip_conv2d_fwd(in, w, b, out, c.N, L.cin, L.h, L.w, L.cout, L.ks, L.ks, L.st, L.pd, relu, c.stream);
    }
}

// Backward-data launch of a conv layer (> 0): dx = conv^T(dy), masked with (xmask > 0) where xmask is given.  unpool_idx: dy is the
// POOLED gradient of a 2x2 pool and the kernel rebuilds the un-pooled tile from it and the arg-max bytes while staging
// (3x3 kernels only; they may decline a shape with CLHIP_ENOTSUP).
// ride != NULL (the plan's rider host, a Conv::Bs3 layer): the launch also reduces the slab jobs ride[0 .. n_ride) in rider blocks and
// sets *rode; where the kernel declines them (CLHIP_ENOTSUP) the plain launch goes out and *rode stays false.
static int launch_conv_bwd_data(const Pass& c, const LayerPlan& L, const float* dy, uint8_t* unpool_idx, const float* xmask, float* dx,
                                const clhip_wgrad_job* ride = nullptr, int n_ride = 0, bool* rode = nullptr) {
    const float* w = c.params + L.w_off;
    switch (L.bwd) {
    case Conv::Wino: case Conv::Bs3:
        if (ride && L.bwd == Conv::Bs3) {
            const int r = clhip_internal_bs_conv_u_riders(dy, c.image(L.img_d), xmask, dx, unpool_idx, unpool_idx ? 1 : 0, c.N, L.cout, L.cin,
                                                          L.h, L.w, ride, n_ride, c.p->reduce_riders, c.p->rider_blocks, c.s());
            if (r == 0) *rode = true;
            if (r != CLHIP_ENOTSUP) return r;
        }
        return plan_conv_u(L.bwd, 1, dy, c.image(L.img_d), nullptr, xmask, dx, unpool_idx, unpool_idx ? 1 : 0, c.N, L.cout, L.cin, L.h, L.w, 0,
                           c.s());
    case Conv::Direct3:
        return unpool_idx ? clhip_conv3x3_bwd_data_unpool(dy, unpool_idx, w, xmask, dx, c.N, L.cin, L.cout, L.h, L.w, c.stream)
                          : clhip_conv3x3_bwd_data(dy, w, xmask, dx, c.N, L.cin, L.cout, L.h, L.w, c.stream);
    case Conv::Bs5:
        return clhip_internal_bs5_conv_u(1, dy, c.image(L.img_d), nullptr, xmask, dx, c.N, L.cout, L.cin, L.h, L.w, 0, c.s());
    default:
        return clhip_conv2d_bwd_data(dy, w, xmask, dx, c.N, L.cin, L.h, L.w, L.cout, L.ks, L.ks, L.st, L.pd, c.stream);
    }
}

// Weight gradient of a conv layer from dy on stream `st`, by the layer's candidates in order; a kernel that declines the call
// (CLHIP_ENOTSUP, CLHIP_ENOSPC: alignment, 2^31 offsets, a fused un-pool on an odd map) hands over to the next.
// unpool_idx != NULL is the POOLED site (dy is the pooled gradient, see launch_conv_bwd_data): only layers with WG_3X3 come here, the
// last resort is the un-pooling direct kernel, and a CLHIP_ENOTSUP from the chain sends the caller to the un-pooled site.
// defer: slabs go to the layer's own region and *slot describes them for the one reduction launch of the pass (*job set).
static int launch_wgrad(const Pass& c, float* grads, const LayerPlan& L, const float* xin, const float* dy, const uint8_t* unpool_idx, void* st,
                        bool defer, clhip_wgrad_job* slot, bool* job) {
    NetPlan* p = c.p;
    float* dw = grads + L.w_off; float* db = grads + L.b_off;
    void* slabs = c.base + p->off_wg + L.wg_off;
    int r;
    auto declined = [&]() { return r == CLHIP_ENOTSUP || r == CLHIP_ENOSPC; };
    auto slab_kernel = [&](auto partial) {        // bswgrad.hip / wino.hip: same arguments; false: it declined, the next candidate runs
        r = partial(xin, dy, unpool_idx, dw, db, c.N, L.cin, L.cout, L.h, L.w, slabs, L.wg_bytes, as_stream(st), slot);
        if (r == 0) *job = true;
        return !declined();
    };
    // (the un-pooled site asks for a region; the pooled site does not: WG_3X3 layers always own one)
    const bool region = defer && (unpool_idx || L.wg_bytes);
    if (region && (L.wg & WG_BS) && slab_kernel(clhip_internal_bs_wgrad_partial)) return r;
    if (region && (L.wg & WG_WINO) && slab_kernel(clhip_internal_wino_wgrad_partial)) return r;
    if (defer && (L.wg & WG_3X3)) {
        *job = true;
        return clhip_internal_conv3x3_wgrad_partial(xin, dy, unpool_idx, dw, db, c.N, L.cin, L.cout, L.h, L.w, slabs, L.wg_bytes, st, slot);
    }
    if (unpool_idx)
        return clhip_conv3x3_bwd_weight_unpool(xin, dy, unpool_idx, dw, db, c.N, L.cin, L.cout, L.h, L.w, c.scratch, p->scratch_bytes, st);
    if (L.wg & WG_BS5) {
        r = clhip_internal_bs5_wgrad(xin, dy, dw, db, c.N, L.cin, L.cout, L.h, L.w, c.scratch, p->scratch_bytes, as_stream(st));
        if (!declined()) return r;
    }
    if (L.wg & WG_S2D) {                  // (the phase planes of this pass's forward are still in the layer's frames)
        const bool fresh = p->s2d_fresh_n == c.N;
        p->s2d_fresh_n = 0;
        return clhip_conv2d_s2d_bwd_weight(fresh ? nullptr : xin, dy, dw, db, c.N, L.cin, L.h, L.w, L.cout, L.ks, L.st, L.pd,
                                           c.base + p->off_s2d + L.s2d_off, L.s2d_bytes, st);
    }
    return (L.wg & WG_3X3) ? clhip_conv3x3_bwd_weight(xin, dy, dw, db, c.N, L.cin, L.cout, L.h, L.w, c.scratch, p->scratch_bytes, st)
                           : clhip_conv2d_bwd_weight(xin, dy, dw, db, c.N, L.cin, L.h, L.w, L.cout, L.ks, L.ks, L.st, L.pd, c.scratch,
                                                     p->scratch_bytes, st);
}

// prepared weights of every layer (forward set, backward-data set, or both): Winograd U images and bf16-split images
static void wino_collect(const Pass& c, bool fwd, bool bwd, std::vector<clhip_wino_wt>& jobs, std::vector<clhip_wino_wt>& bsjobs) {
    jobs.reserve(2 * c.p->layers.size());                  // (sized by the plan: a net of any depth gets every transform)
    bsjobs.reserve(2 * c.p->layers.size());
    for (const LayerPlan& L : c.p->layers) {
        auto add = [&](const WeightImage& im, int ko, int ci, int mode) {
            const float* w = c.params + L.w_off;
            switch (im.kind) {
            case Img::WinoU: jobs.push_back(clhip_wino_wt{w, c.image(im), ko, ci, mode, 0}); break;
            case Img::Bs3: bsjobs.push_back(clhip_wino_wt{w, c.image(im), ko, ci, mode, 0}); break;
            case Img::Bs5: bsjobs.push_back(clhip_wino_wt{w, c.image(im), ko, ci, mode, 5}); break;
            case Img::None: break;
            }
        };
        if (fwd) add(L.img_f, L.cout, L.cin, 0);
        if (bwd) add(L.img_d, L.cin, L.cout, 1);
    }
}

static int wino_prepare(const Pass& c, bool fwd, bool bwd) {
    std::vector<clhip_wino_wt> jobs, bsjobs;
    wino_collect(c, fwd, bwd, jobs, bsjobs);
    // (ONE launch for the Winograd U images and the bf16-split images of the pass when they fit one job table: a boundary between two
    // launches of 5 - 7 us each costs as much as either)
    return clhip_internal_weight_images(jobs.data(), (int)jobs.size(), bsjobs.data(), (int)bsjobs.size(), c.s());
}

// Forward pass; activations are kept in ws for a following backward. logits_out (optional) receives a copy of the [N][classes] logits.
// tail: 0 = every layer; 1 = stop behind the first Linear layer, the caller launches the fused tail itself (loss step);
// 2 = stop there and finish with the fused tail, forward only.
static int net_forward_impl(void* handle, const float* params, const float* x, int N, void* ws, float* logits_out,
                            void* stream, int tail, int* slabs_live = nullptr, bool prep_bwd = false) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || !params || !x || !ws || N <= 0 || N > p->max_batch) return CLHIP_EINVAL;
    const Pass c(p, params, N, ws, stream);
    float* acts = c.acts;
    // The weight images are first read by layer 1.  Where layer 0 is the fused conv + ReLU + pool launch of a 3-channel image (no
    // dropout on the input, direct kernel) the jobs ride in that launch's grid (conv3x3.hip, c3w64_relu_pool_wt_kernel),
    // which declines (CLHIP_ENOTSUP) unless the shape is conv3x3_c3w64_relu_pool_kernel's; every other plan: the launch of its own, here
    std::vector<clhip_wino_wt> edge_jobs, edge_bsjobs;
    bool edge = false;
    if (p->wino_bytes) {
        const LayerPlan& L0 = p->layers[0];
        edge = p->edge_grids && L0.fused_pool && L0.fwd == Conv::Direct3 && !L0.drop && L0.cin == 3;
        if (edge) wino_collect(c, true, prep_bwd, edge_jobs, edge_bsjobs);
        else if (const int rcw = wino_prepare(c, true, prep_bwd)) return rcw;
    }
    const float* cur = x;
    int rc;
    const size_t n_run = tail ? (size_t)p->fc_first + 1 : p->layers.size();
    int live = 0;            // split-K slabs of the first Linear layer left in `scratch` for the fused tail
    for (size_t li = 0; li < n_run; ++li) {
        const LayerPlan& L = p->layers[li];
        float* y = acts + L.act_off;
        const bool probed = (int)li == p->probe_layer && p->probe_kind == 0 && !p->probe_ev.empty();
        if (probed) (void)hipEventRecord(p->probe_ev[2 * (p->probe_count % PROBE_RING)], c.s());
        struct ProbeEnd {       // closes the pair when the layer's launches are issued (every exit of the loop body)
            NetPlan* p; bool on; hipStream_t s;
            ~ProbeEnd() { if (on) { (void)hipEventRecord(p->probe_ev[2 * (p->probe_count % PROBE_RING) + 1], s); ++p->probe_count; } }
        } probe_end{p, probed, c.s()};
        if (L.drop && L.has_drop_buf) {       // masked copy: backward reads it as this layer's input, cur stays intact
            float* dropped = acts + L.drop_off;
            rc = drop_copy(cur, dropped, L.drop, L.drop_stride, L.in_elems, N, c.s());
            if (rc) return rc;
            cur = dropped;
        } else if (L.drop) {    // li > 0: cur is the previous layer's saved output; masked in place so that backward sees h * m
            rc = drop_scale(const_cast<float*>(cur), L.drop, L.drop_stride, L.in_elems, N, c.s());
            if (rc) return rc;
        }
        if (L.type == 0) {
            // fused_pool layers: conv + bias + ReLU + 2x2 max-pool in one launch.  Every other conv layer (general geometry, BatchNorm,
            // no ReLU, other pool windows): separate conv (+bias, ReLU), BatchNorm and pool kernels
            float* pl = acts + L.pool_off;
            uint8_t* pidx = c.idx + L.idx_off;
            if (li == 0 && edge) {
                // (a forward probe on layer 0 — clhip_net_probe_kind 0 — times the merged launch, weight blocks included; with
                //  CLHIP_EDGE_GRIDS=0 the weight-image launch lies in front of the event pair: the layer-0 figure shifts by it)
                rc = clhip_internal_c3w64_pool_weight_images(cur, params + L.w_off, params + L.b_off, pl, pidx, N, L.cin, L.cout,
                                                             L.h, L.w, edge_jobs.data(), (int)edge_jobs.size(), edge_bsjobs.data(),
                                                             (int)edge_bsjobs.size(), p->edge_grids == 2, c.s());
                if (rc == 0) { ++p->edge_count; cur = pl; continue; }
                if (rc != CLHIP_ENOTSUP) return rc;
                rc = clhip_internal_weight_images(edge_jobs.data(), (int)edge_jobs.size(), edge_bsjobs.data(), (int)edge_bsjobs.size(), c.s());
                if (rc) return rc;
            }
            float* zc = L.bn ? acts + L.z_off : L.fused_pool ? pl : y;
            rc = launch_conv_fwd(c, L, cur, zc, L.fused_pool ? pidx : nullptr, L.bn ? 0 : L.relu);
            if (rc) return rc;
            if (L.fwd == Conv::S2d) p->s2d_fresh_n = N;
            if (L.bn) {
                float* st = acts + L.stat_off;
                rc = clhip_bn_fwd(zc, params + L.bn_w_off, params + L.bn_b_off, L.rmean, L.rvar, y, st, st + L.cout, N, L.cout,
                                  L.oh * L.ow, p->training, L.bn_momentum, L.bn_eps, L.relu, c.scratch, p->scratch_bytes, stream);
                if (rc) return rc;
            }
            cur = L.fused_pool ? pl : y;
            if (L.pool && !L.fused_pool) {
                rc = L.pool22 ? clhip_maxpool2_fwd(y, pl, pidx, N * L.cout, L.oh, L.ow, stream)
                              : clhip_maxpool_fwd(y, pl, pidx, N * L.cout, L.oh, L.ow, L.pk, L.ps, stream);
                if (rc) return rc;
                cur = pl;
            }
        } else {
            if (tail && (int)li == p->fc_first) {
                // the fused tail sums the split-K slabs of this layer itself (no reduction launch)
                rc = clhip_internal_fc_fwd_partial(cur, params + L.w_off, N, L.cin, L.cout, c.scratch, p->scratch_bytes, &live, c.s());
                if (rc) return rc;
            }
            if (!live) {
                rc = clhip_fc_fwd(cur, params + L.w_off, params + L.b_off, y, N, L.cin, L.cout, L.relu, c.scratch, p->scratch_bytes, stream);
                if (rc) return rc;
            }
            cur = y;
        }
    }
    if (slabs_live) *slabs_live = live;
    if (tail == 1) return 0;
    if (tail == 2) {
        rc = clhip_internal_fc_tail(&p->chain, params, acts, N, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                                    c.base + p->off_rows, p->tail_counter, 0, 0, static_cast<const float*>(c.scratch), live, c.s());
        if (rc) return rc;
        cur = acts + p->layers.back().act_off;
    }
    if (logits_out) {
        hipError_t e = hipMemcpyAsync(logits_out, cur, (size_t)N * p->n_classes * sizeof(float), hipMemcpyDeviceToDevice, c.s());
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// State of one backward pass, layer by layer from the top: the gradient in flight and its ping-pong buffer, the side stream's
// hand-offs, the slab jobs collected for the one reduction launch at the end.
struct BackwardPass {
    const Pass c;
    NetPlan* const p;
    float* const grads; const float* const dlogits;
    float* const g[2]; float* const fcdz;      // the two ping-pong gradient buffers; dz slots of the fused classifier
    const hipStream_t main_s;
    const bool ov;           // every conv layer's weight gradient on the side stream: immediate reductions
    const bool ov_small;     // only the under-filled deep layers; slabs stay deferred
    const bool defer;        // weight-gradient slabs stay in the layers' regions until one launch reduces them all
    const float* gin;        // gradient w.r.t. the current layer's output (already ReLU-masked)
    int gin_buf = -1;        // which of g[0..1] holds gin (-1: dlogits / fcdz)
    int flip = 0, taken = -1;
    hipEvent_t last_side = nullptr;                  // last weight-gradient event of the side stream: the caller's stream joins it at the end
    hipEvent_t pending[2] = {nullptr, nullptr};      // side-stream reader of g[b] that must finish before g[b] is rewritten
    clhip_wgrad_job jobs[CLHIP_WGRAD_JOBS_MAX];
    int n_jobs = 0;
    bool side_jobs = false;  // one of jobs[] was issued on the side stream: its slabs are not ordered before a main-stream launch

    BackwardPass(NetPlan* plan, const float* params, float* grads_, int N, void* ws, const float* dl, void* stream)
        : c(plan, params, N, ws, stream), p(plan), grads(grads_), dlogits(dl),
          g{reinterpret_cast<float*>(c.base + plan->off_g0), reinterpret_cast<float*>(c.base + plan->off_g1)},
          fcdz(reinterpret_cast<float*>(c.base + plan->off_fcdz)), main_s(as_stream(stream)), ov(plan->overlap && plan->overlap_mode == 1),
          ov_small(plan->overlap && plan->overlap_mode == 2), defer(plan->n_wg > 0 && !ov), gin(dl) {}

    bool side_ok(int layer) const {
        const LayerPlan& Ls = p->layers[layer];
        return ov || (ov_small && Ls.type == 0 && (Ls.wg & WG_3X3) && Ls.h * Ls.w <= 256);
    }
    // layers whose backward-data and weight gradient can go out as one grid: 3x3 layers on the Winograd kernels with deferred
    // slabs, a backward-data to compute and nothing to apply to it afterwards (clhip_internal_wino_pair decides on the shape)
    bool pair_ok(const LayerPlan& L, int layer) const {
        return defer && L.bwd == Conv::Wino && (L.wg & WG_WINO) && !(L.wg & WG_BS) && L.wg_bytes && !L.drop && !L.extra_grad && !side_ok(layer);
    }
    // next ping-pong buffer as an OUTPUT of a main-stream launch
    float* take() {
        const int bi = flip;
        flip ^= 1;
        if (pending[bi]) { (void)hipStreamWaitEvent(main_s, pending[bi], 0); pending[bi] = nullptr; }
        taken = bi;
        return g[bi];
    }
    // run `launch(stream)` (a weight-gradient launch reading dy = g[dy_buf]) on the side stream once main has produced dy
    template <class F> int on_side(int layer, int dy_buf, F&& launch) {
        if (!side_ok(layer)) return launch(c.stream);
        hipError_t e = hipEventRecord(p->ev_dy[layer], main_s);
        if (e == hipSuccess) e = hipStreamWaitEvent(p->side, p->ev_dy[layer], 0);
        if (e != hipSuccess) return (int)e;
        const int r = launch((void*)p->side);
        if (r) return r;
        e = hipEventRecord(p->ev_wg[layer], p->side);
        if (e != hipSuccess) return (int)e;
        last_side = p->ev_wg[layer];
        if (dy_buf >= 0) pending[dy_buf] = p->ev_wg[layer];
        return 0;
    }
    // what a layer applies to the gradient w.r.t. its input once backward-data has written it: dropout mask, then the side branch
    int finish_input_grad(const LayerPlan& L, float* gout) {
        if (L.drop) {
            const int rc = drop_scale(gout, L.drop, L.drop_stride, L.in_elems, c.N, main_s);
            if (rc) return rc;
        }
        return L.extra_grad ? add_inplace(gout, L.extra_grad, L.in_elems * (size_t)c.N, main_s) : 0;
    }
    int fc_layer(int i, const float* xin);
    int conv_layer(int i, const float* xin, const float* xmask);
};

int BackwardPass::fc_layer(int i, const float* xin) {
    const LayerPlan& L = p->layers[i];
    const int N = c.N;
    int rc;
    if (!p->fc_fused) {
        rc = clhip_fc_bwd_weight(xin, gin, grads + L.w_off, grads + L.b_off, N, L.cin, L.cout, c.scratch, p->scratch_bytes, c.stream);
        if (rc) return rc;
    }
    bool combo = false;
    clhip_fc_chain ch;
    if (p->fc_fused && i == p->fc_first) {
        ch = p->chain;       // inputs of the hidden layers: their masked copies where a dropout is active
        for (int l = 1; l < ch.n; ++l) {
            const LayerPlan& Ll = p->layers[p->fc_first + l];
            if (Ll.drop && Ll.has_drop_buf) ch.act_off[l - 1] = Ll.drop_off;
        }
    }
    if (i > 0) {
        // fused weight gradients (below) read the hidden layers' dz after the chain: keep them in their own slots
        float* gout;
        if (p->fc_fused && i > p->fc_first) { gout = fcdz + p->chain.dz_off[i - p->fc_first - 1]; gin_buf = -1; }
        else { gout = take(); gin_buf = taken; }
        // mask with (xin > 0): xin is a ReLU (or pooled ReLU) output
        clhip_gemm_args ga;
        const int gb = (p->fc_fused && i == p->fc_first && !p->no_combo)
                           ? clhip_internal_fc_bwd_data_args(gin, c.params + L.w_off, xin, gout, N, L.cin, L.cout, &ga) : 0;
        if (gb > 0) {
            // backward-data of the first Linear layer and every Linear layer's dW / db in ONE launch
            rc = clhip_internal_fc_bwd_combo(&ga, gb, &ch, grads, xin, N, c.acts, dlogits, fcdz, main_s);
            combo = true;
        } else {
            rc = clhip_fc_bwd_data(gin, c.params + L.w_off, xin, gout, N, L.cin, L.cout, c.scratch, p->scratch_bytes, c.stream);
        }
        if (rc) return rc;
        gin = gout;
        rc = finish_input_grad(L, gout);
        if (rc) return rc;
    }
    if (p->fc_fused && i == p->fc_first && !combo) {
        // all dz_l are in place: dW_l, db_l of every Linear layer in one launch
        rc = clhip_internal_fc_chain_wgrad(&ch, grads, xin, N, c.acts, dlogits, fcdz, main_s);
        if (rc) return rc;
    }
    return 0;
}

int BackwardPass::conv_layer(int i, const float* xin, const float* xmask) {
    const LayerPlan& L = p->layers[i];
    const int N = c.N;
    uint8_t* const pidx = c.idx + L.idx_off;
    const float* gy = gin; int gy_buf = gin_buf;       // gradient w.r.t. the conv (+ ReLU) output: gin itself, or its un-pooled form
    bool wdone = false, ddone = false;
    float* gout_d = nullptr; int gout_d_buf = -1;      // backward-data output, once taken
    int rc;
    // measurement probe around this layer's backward-data / weight-gradient launch(es) (clhip_net_probe_kind)
    auto probe_on = [&](int kind) { return i == p->probe_layer && p->probe_kind == kind && !p->probe_ev.empty(); };
    // (events go on the stream the launch is issued on: a weight-gradient launch may run on the side stream, on_side)
    auto probe_stream = [&](int kind) { return (kind == 2 && side_ok(i)) ? p->side : main_s; };
    auto probe_begin = [&](int kind) { if (probe_on(kind)) (void)hipEventRecord(p->probe_ev[2 * (p->probe_count % PROBE_RING)], probe_stream(kind)); };
    auto probe_end = [&](int kind) {
        if (probe_on(kind)) { (void)hipEventRecord(p->probe_ev[2 * (p->probe_count % PROBE_RING) + 1], probe_stream(kind)); ++p->probe_count; }
    };
    // backward-data and the weight-gradient slabs of this layer as ONE grid (wino.hip, wino_pair_kernel).  A declined shape is no
    // error: gout_d stays taken and the backward-data launch below reuses it
    auto one_grid = [&](const float* dy, uint8_t* idx_or_null) {
        gout_d = take(); gout_d_buf = taken;
        if (p->probe_kind) probe_begin(p->probe_kind);   // (kinds 1 and 2 both time the merged launch; a forward probe does not)
        const int r = clhip_internal_wino_pair(dy, idx_or_null, c.image(L.img_d), xmask, gout_d, xin, grads + L.w_off, grads + L.b_off, N, L.cin,
                                               L.cout, L.h, L.w, c.base + p->off_wg + L.wg_off, L.wg_bytes, main_s, &jobs[n_jobs]);
        if (r == 0) { wdone = ddone = true; ++n_jobs; if (p->probe_kind) probe_end(p->probe_kind); }
        return r == CLHIP_ENOTSUP ? 0 : r;
    };
    // the weight-gradient chain (launch_wgrad) on the stream of this layer; n_jobs advances when it left slabs for the deferred reduction
    auto wgrad = [&](const float* dy, uint8_t* idx_or_null, int dy_buf) {
        bool job = false;
        probe_begin(2);
        const int r = on_side(i, dy_buf, [&](void* st) { return launch_wgrad(c, grads, L, xin, dy, idx_or_null, st, defer, &jobs[n_jobs], &job); });
        if (r == 0) { wdone = true; probe_end(2); if (job) { ++n_jobs; side_jobs = side_jobs || side_ok(i); } }
        return r;
    };
    // the backward-data launch; at the plan's rider host it takes the slab jobs collected so far along (all of them issued on the
    // main stream in front of it) and they are done: the reduction launch of the pass keeps the jobs that follow
    auto bwd_data = [&](const float* dy, uint8_t* idx_or_null, float* dx) {
        const bool host = i == p->rider_host && p->reduce_riders && defer && n_jobs > 0 && !side_jobs;
        bool rode = false;
        const int r = launch_conv_bwd_data(c, L, dy, idx_or_null, xmask, dx, host ? jobs : nullptr, n_jobs, &rode);
        if (rode) { n_jobs = 0; ++p->rider_count; }
        return r;
    };
    if (L.vgg && L.pool22 && !L.bn && (L.wg & WG_3X3)) {
        // fused max-pool backward: weight gradient and backward-data both rebuild the un-pooled gradient tile from
        // the POOLED gradient + the arg-max codes while staging it, when their kernels support the shape (first
        // layer: the small-C kernel; others: the 16-byte staging paths).  The 4x larger un-pooled tensor and the
        // clhip_maxpool2_bwd launch disappear.
        if (pair_ok(L, i)) {
            rc = one_grid(gin, pidx);
            if (rc) return rc;
        }
        if (!wdone) {
            rc = wgrad(gin, pidx, gin_buf);
            if (rc && rc != CLHIP_ENOTSUP) return rc;      // CLHIP_ENOTSUP: this layer goes the un-pooled way below
        }
        if (wdone && !ddone && i > 0 && !L.drop && !L.extra_grad) {
            if (!gout_d) { gout_d = take(); gout_d_buf = taken; }
            probe_begin(1);
            rc = bwd_data(gin, pidx, gout_d);
            if (rc == 0) { ddone = true; probe_end(1); }
            else if (rc != CLHIP_ENOTSUP) return rc;
        }
    }
    if (L.pool && !(wdone && (i == 0 || ddone))) {      // somebody still needs the un-pooled gradient
        float* gout = gout_d;
        if (gout) taken = gout_d_buf; else gout = take();
        rc = L.pool22 ? clhip_maxpool2_bwd(gin, pidx, gout, N * L.cout, L.oh, L.ow, c.stream)
                      : clhip_maxpool_bwd(gin, pidx, gout, N * L.cout, L.oh, L.ow, L.pk, L.ps, c.stream);
        if (rc) return rc;
        gy = gout; gy_buf = taken;
        gout_d = nullptr;
    }
    if (L.bn) {
        // dy (w.r.t. the ReLU output) -> dz (w.r.t. the convolution output), in place; dgamma, dbeta
        const float* st = c.acts + L.stat_off;
        float* dzb = const_cast<float*>(gy);
        if (gy_buf < 0) return CLHIP_EINVAL;      // a conv layer's incoming gradient always lives in g[0..1]
        rc = clhip_bn_bwd(gy, c.acts + L.act_off, c.acts + L.z_off, c.params + L.bn_w_off, st, st + L.cout, dzb, grads + L.bn_w_off,
                          grads + L.bn_b_off, N, L.cout, L.oh * L.ow, p->training, L.relu, c.scratch, p->scratch_bytes, c.stream);
        if (rc) return rc;
    }
    if (!wdone && !L.pool && !gout_d && pair_ok(L, i)) {
        rc = one_grid(gy, nullptr);
        if (rc) return rc;
    }
    if (!wdone) {
        rc = wgrad(gy, nullptr, gy_buf);
        if (rc) return rc;
    }
    if (ddone) { gin = gout_d; gin_buf = gout_d_buf; }
    if (i == 0 || ddone) return 0;
    float* gout = gout_d;             // (taken for a merged launch that declined the shape)
    if (gout) taken = gout_d_buf; else gout = take();
    probe_begin(1);
    rc = bwd_data(gy, nullptr, gout);
    if (rc) return rc;
    probe_end(1);
    gin = gout; gin_buf = taken;
    return finish_input_grad(L, gout);
}

// Backward pass from dlogits[N][classes] (device) through the activations saved by the last clhip_net_forward on the same ws.
// Writes every parameter gradient into `grads` (same offsets as params; overwritten, not accumulated).
static int net_backward_impl(void* handle, const float* params, float* grads, const float* x, int N, void* ws,
                             const float* dlogits, void* stream, bool tail_done, bool wino_ready = false) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || !params || !grads || !x || !ws || !dlogits || N <= 0 || N > p->max_batch) return CLHIP_EINVAL;
    BackwardPass b(p, params, grads, N, ws, dlogits, stream);
    int rc;
    if (p->wino_bytes && !wino_ready) {           // a backward on its own: the forward of the same call did not transform for it
        rc = wino_prepare(b.c, false, true);
        if (rc) return rc;
    }
    for (int i = (int)p->layers.size() - 1; i >= 0; --i) {
        const LayerPlan& L = p->layers[i];
        // input of layer i = (pooled) output of layer i-1, or the image batch
        const float* xin = x;
        // ReLU mask of this layer's backward-data, (input > 0).  Not needed when the input is the pooled output of a fused
        // conv + ReLU + pool launch: its arg-max bytes mark the windows without a positive maximum (CLHIP_POOL_DEAD) and
        // the un-pooling consumers of the gradient drop them (common.hpp)
        bool masked = true;
        if (i > 0) {
            const LayerPlan& P = p->layers[i - 1];
            xin = b.c.acts + ((P.type == 0 && P.pool) ? P.pool_off : P.act_off);
            if (L.drop && L.has_drop_buf) xin = b.c.acts + L.drop_off;
            masked = !(L.type == 0 && !L.drop && P.fused_pool);
        }
        if (L.type == 1 && tail_done && i > p->fc_first) {
            // the fused tail has already left dz of this layer's input in its fcdz slot
            b.gin = b.fcdz + p->chain.dz_off[i - p->fc_first - 1]; b.gin_buf = -1;
            continue;
        }
        rc = L.type == 1 ? b.fc_layer(i, xin) : b.conv_layer(i, xin, masked ? xin : nullptr);
        if (rc) return rc;
    }
    if (b.last_side) {      // join: every slab / gradient of the side stream is complete on the caller's stream from here on
        hipError_t e = hipStreamWaitEvent(b.main_s, b.last_side, 0);
        if (e != hipSuccess) return (int)e;
    }
    return b.n_jobs ? clhip_internal_wgrad_reduce_multi(b.jobs, b.n_jobs, b.main_s) : 0;
}

}  // namespace

extern "C" {

int clhip_net_create(const clhip_layer_desc* descs, int n_layers, int max_batch, int in_c, int in_h, int in_w,
                     void** out_handle) {
    if (!descs || n_layers <= 0 || max_batch <= 0 || !out_handle) return CLHIP_EINVAL;
    std::unique_ptr<NetPlan> p(new (std::nothrow) NetPlan());
    if (!p) return CLHIP_ENOSPC;
    p->max_batch = max_batch; p->in_c = in_c; p->in_h = in_h; p->in_w = in_w;
    p->in_elems = (size_t)in_c * in_h * in_w;
    const int rc = plan_geometry(*p, descs, n_layers);
    if (rc) return rc;
    for (int i = 0; i < n_layers; ++i)
        if (p->layers[i].type == 0) choose_paths(p->layers[i], descs[i], i, max_batch);
    layout_arena(*p);
    make_resources(*p);
    *out_handle = p.release();
    return 0;
}

// Dropout in front of layer `layer` (> 0): mask is device memory, [N][in_elems] with row_stride floats between samples
// (row_stride 0: one row for the whole batch), values 0 or 1/p_retain.  NULL switches it off (eval mode).  The mask must
// stay valid and unchanged from a forward to its backward.
int clhip_net_set_dropout(void* handle, int layer, const float* mask, long row_stride) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || layer <= 0 || layer >= (int)p->layers.size() || row_stride < 0) return CLHIP_EINVAL;
    p->layers[layer].drop = mask;
    p->layers[layer].drop_stride = row_stride;
    return 0;
}

int clhip_net_set_bn(void* handle, int layer, float* running_mean, float* running_var, float momentum, float eps) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || layer < 0 || layer >= (int)p->layers.size() || !p->layers[layer].bn || !(eps > 0.f)) return CLHIP_EINVAL;
    LayerPlan& L = p->layers[layer];
    L.rmean = running_mean; L.rvar = running_var; L.bn_momentum = momentum; L.bn_eps = eps;
    return 0;
}

int clhip_net_layer_input(void* handle, int layer, size_t* ws_float_off, size_t* in_elems) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || layer <= 0 || layer >= (int)p->layers.size() || !ws_float_off || !in_elems) return CLHIP_EINVAL;
    const LayerPlan& P = p->layers[layer - 1];
    *ws_float_off = p->off_acts / sizeof(float) + ((P.type == 0 && P.pool) ? P.pool_off : P.act_off);
    *in_elems = p->layers[layer].in_elems;
    return 0;
}

int clhip_net_layer_pool_idx(void* handle, int layer, size_t* ws_byte_off, size_t* elems) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || layer < 0 || layer >= (int)p->layers.size() || !ws_byte_off || !elems) return CLHIP_EINVAL;
    const LayerPlan& L = p->layers[layer];
    if (L.type != 0 || !L.pool) return CLHIP_EINVAL;
    *ws_byte_off = p->off_idx + L.idx_off;
    *elems = L.pool_elems;
    return 0;
}

int clhip_net_edge_grid_count(void* handle) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    return p ? (int)(p->edge_count & 0x7fffffffu) : CLHIP_EINVAL;
}

int clhip_net_reduce_rider_count(void* handle) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    return p ? (int)(p->rider_count & 0x7fffffffu) : CLHIP_EINVAL;
}

int clhip_net_prepared_weights(void* handle, size_t* ws_byte_off, size_t* bytes) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || !ws_byte_off || !bytes) return CLHIP_EINVAL;
    *ws_byte_off = p->off_wino;
    *bytes = p->wino_bytes;
    return 0;
}

int clhip_net_layer_paths(void* handle, int layer) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || layer < 0 || layer >= (int)p->layers.size()) return CLHIP_EINVAL;
    const LayerPlan& L = p->layers[layer];
    if (L.type == 1) {
        // Linear layers.  bit 6: the layer's forward and backward-data run inside fc_tail_kernel (the layers behind the first
        // Linear layer of a plan that takes the tail, while none of them has a dropout mask or an extra input gradient set:
        // tail_usable's plan-side conditions; its per-call ones are the alignment of the caller's buffers and the batch).
        // bit 7: dW / db come from the fused weight-gradient launch (fc_chain_wgrad_kernel / fc_bwd_combo_kernel).
        bool tail = p->fc_tail && layer > p->fc_first;
        for (size_t i = p->fc_first + 1; tail && i < p->layers.size(); ++i)
            if (p->layers[i].drop || p->layers[i].extra_grad) tail = false;
        return (tail ? 64 : 0) | ((p->fc_fused && layer >= p->fc_first) ? 128 : 0);
    }
    // bits 0 / 1: the forward / backward-data launch reads prepared weights of the 3x3 paths (Winograd or bf16-split);
    // bits 3 / 4: it is a bf16-split kernel (bsconv.hip, 3x3 or 5x5), not Winograd
    auto dir = [](Conv k) { return (k == Conv::Wino || k == Conv::Bs3 ? 1 : 0) | (k == Conv::Bs3 || k == Conv::Bs5 ? 8 : 0); };
    // bits 2 / 5: the weight gradient is the Winograd / the bf16-split kernel (bswgrad.hip).  Both run only inside the
    // deferred-reduction scheme (BackwardPass::defer), and even then the kernel may hand single shapes back to the direct path —
    // odd maps with a fused un-pool, > 2^31-byte offsets
    const bool defer_capable = p->n_wg > 0 && !(p->overlap && p->overlap_mode == 1);
    return dir(L.fwd) | dir(L.bwd) << 1 | (((L.wg & WG_WINO) && defer_capable) ? 4 : 0) | (((L.wg & WG_BS) && defer_capable) ? 32 : 0);
}

int clhip_net_set_input_grad(void* handle, int layer, const float* extra) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || layer <= 0 || layer >= (int)p->layers.size()) return CLHIP_EINVAL;
    p->layers[layer].extra_grad = extra;
    return 0;
}

// Measurement: time the forward launch(es) of plan layer `layer` with HIP events on the stream they are issued on
// (layer < 0: off).  A backward-data probe (clhip_net_probe_kind 1) on the plan's rider host times that launch WITH its rider
// blocks (CLHIP_REDUCE_RIDERS; with 0 the slabs are reduced outside the pair) — as the layer-0 forward probe does with the weight
// blocks of the edge grid.  clhip_net_probe_read waits for the recorded launches and returns their average duration over the
// last (at most 64) forward passes, then clears the count.
int clhip_net_probe(void* handle, int layer) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || layer >= (int)p->layers.size()) return CLHIP_EINVAL;
    if (layer >= 0 && p->probe_ev.empty()) {
        std::vector<hipEvent_t> made;
        made.reserve(2 * PROBE_RING);
        for (unsigned i = 0; i < 2 * PROBE_RING; ++i) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) {
                for (hipEvent_t m : made) (void)hipEventDestroy(m);
                return CLHIP_ENOTSUP;
            }
            made.push_back(e);
        }
        p->probe_ev.swap(made);
    }
    p->probe_layer = layer;
    p->probe_kind = 0;
    p->probe_count = 0;
    return 0;
}

int clhip_net_probe_kind(void* handle, int layer, int kind) {
    if (kind < 0 || kind > 2) return CLHIP_EINVAL;
    const int rc = clhip_net_probe(handle, layer);
    if (rc == 0) static_cast<NetPlan*>(handle)->probe_kind = kind;
    return rc;
}

int clhip_net_probe_read(void* handle, float* avg_us, int* count) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || !avg_us || !count) return CLHIP_EINVAL;
    const unsigned n = p->probe_count < PROBE_RING ? p->probe_count : PROBE_RING;
    double sum = 0.0;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned slot = (p->probe_count - 1 - i) % PROBE_RING;
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(p->probe_ev[2 * slot + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, p->probe_ev[2 * slot], p->probe_ev[2 * slot + 1]);
        if (e != hipSuccess) return (int)e;
        sum += ms;
    }
    *avg_us = n ? (float)(sum / n * 1e3) : 0.f;
    *count = (int)n;
    p->probe_count = 0;
    return 0;
}

int clhip_net_set_training(void* handle, int training) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p) return CLHIP_EINVAL;
    p->training = training ? 1 : 0;
    return 0;
}

void clhip_net_destroy(void* handle) { delete static_cast<NetPlan*>(handle); }

size_t clhip_net_workspace_bytes(void* handle) { return handle ? static_cast<NetPlan*>(handle)->total_bytes : 0; }
int clhip_net_num_classes(void* handle) { return handle ? static_cast<NetPlan*>(handle)->n_classes : 0; }

int clhip_net_forward(void* handle, const float* params, const float* x, int N, void* ws, float* logits_out,
                      void* stream) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || !params || !x || !ws || N <= 0 || N > p->max_batch) return CLHIP_EINVAL;
    return net_forward_impl(handle, params, x, N, ws, logits_out, stream, tail_usable(p, params, ws, N) ? 2 : 0);
}

int clhip_net_backward(void* handle, const float* params, float* grads, const float* x, int N, void* ws,
                       const float* dlogits, void* stream) {
    return net_backward_impl(handle, params, grads, x, N, ws, dlogits, stream, false);
}

// forward + loss (+ backward when grads != NULL) in one call.
//   loss_kind 0: CrossEntropy mean   1: CrossEntropy sum   2: sum of squared logits (MAS)
int clhip_net_loss_step_slice(void* handle, const float* params, float* grads, const float* x, const int64_t* labels,
                              int N, int loss_kind, int col_off, int ncols, void* ws, float* loss_out, double* stats,
                              float* logits_out, void* stream) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || !ws || (loss_kind != 2 && !labels)) return CLHIP_EINVAL;
    char* base = static_cast<char*>(ws);
    float* dlogits = reinterpret_cast<float*>(base + p->off_dlogits);
    float* loss_dev = loss_out ? loss_out : reinterpret_cast<float*>(base + p->off_loss);
    if (!params || !x || N <= 0 || N > p->max_batch) return CLHIP_EINVAL;
    const int nc = ncols > 0 ? ncols : p->n_classes - col_off;
    if (loss_kind != 2 && nc <= 64 && col_off >= 0 && col_off + nc <= p->n_classes && tail_usable(p, params, ws, N)) {
        // first Linear layer by the GEMM launches, then ONE launch for the rest of the classifier, the loss and the
        // backward-data chain down to dz(h1); backward resumes at the first Linear layer
        if (loss_kind != 0 && loss_kind != 1) return CLHIP_EINVAL;
        int live = 0;
        int rc = net_forward_impl(handle, params, x, N, ws, nullptr, stream, 1, &live, grads != nullptr);
        if (rc) return rc;
        float* acts = reinterpret_cast<float*>(base + p->off_acts);
        rc = clhip_internal_fc_tail(&p->chain, params, acts, N, labels, loss_kind, col_off, nc, dlogits,
                                    reinterpret_cast<float*>(base + p->off_fcdz), loss_dev, stats, base + p->off_rows,
                                    p->tail_counter, 1, grads ? 1 : 0, reinterpret_cast<const float*>(base + p->off_scratch), live,
                                    as_stream(stream));
        if (rc) return rc;
        if (logits_out) {
            hipError_t e = hipMemcpyAsync(logits_out, acts + p->layers.back().act_off, (size_t)N * p->n_classes * sizeof(float),
                                          hipMemcpyDeviceToDevice, as_stream(stream));
            if (e != hipSuccess) return (int)e;
        }
        if (grads) rc = net_backward_impl(handle, params, grads, x, N, ws, dlogits, stream, true, true);
        return rc;
    }
    int rc = net_forward_impl(handle, params, x, N, ws, logits_out, stream, 0, nullptr, grads != nullptr);
    if (rc) return rc;
    const LayerPlan& last = p->layers.back();
    const float* logits = reinterpret_cast<float*>(base + p->off_acts) + last.act_off;
    if (loss_kind == 2) rc = clhip_mse_zero_sum(logits, (size_t)N * p->n_classes, dlogits, loss_dev, stream);
    else rc = clhip_softmax_ce_slice(logits, labels, N, p->n_classes, col_off, ncols > 0 ? ncols : p->n_classes - col_off,
                                     loss_kind, dlogits, loss_dev, stats, stream);
    if (rc) return rc;
    if (grads) rc = net_backward_impl(handle, params, grads, x, N, ws, dlogits, stream, false, true);
    return rc;
}

// forward (every layer: the fused fc_tail knows one slice only) + segmented loss (loss.hip) + backward: the whole step of
// an exemplar method over [current batch | exemplar chunks].
int clhip_net_loss_step_loss_segments(void* handle, const float* params, float* grads, const float* x, const int64_t* labels,
                                      const float* targets, int ld_t, int N, const clhip_loss_segment* segs, int n_segs, float T,
                                      void* ws, float* loss_out, double* stats, float* logits_out, void* stream) {
    NetPlan* p = static_cast<NetPlan*>(handle);
    if (!p || !ws || !labels || !segs || n_segs < 1 || n_segs > CLHIP_LOSS_MAX_SEGS) return CLHIP_EINVAL;
    if (!params || !x || N <= 0 || N > p->max_batch || N > CLHIP_LOSS_MAX_ROWS) return CLHIP_EINVAL;
    char* base = static_cast<char*>(ws);
    float* dlogits = reinterpret_cast<float*>(base + p->off_dlogits);
    float* loss_dev = loss_out ? loss_out : reinterpret_cast<float*>(base + p->off_loss);
    int rc = net_forward_impl(handle, params, x, N, ws, logits_out, stream, 0, nullptr, grads != nullptr);
    if (rc) return rc;
    const float* logits = reinterpret_cast<float*>(base + p->off_acts) + p->layers.back().act_off;
    rc = clhip_loss_segments(logits, labels, targets, ld_t, N, p->n_classes, segs, n_segs, T, dlogits, loss_dev, stats, stream);
    if (rc) return rc;
    if (grads) rc = net_backward_impl(handle, params, grads, x, N, ws, dlogits, stream, false, true);
    return rc;
}

int clhip_net_loss_step(void* handle, const float* params, float* grads, const float* x, const int64_t* labels,
                        int N, int loss_kind, void* ws, float* loss_out, double* stats, float* logits_out,
                        void* stream) {
    return clhip_net_loss_step_slice(handle, params, grads, x, labels, N, loss_kind, 0, 0, ws, loss_out, stats,
                                     logits_out, stream);
}

}  // extern "C"
