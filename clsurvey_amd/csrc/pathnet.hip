// PathNet parameter-side kernels — restates networks/vgg_pathnet.py (Net.forward's sum over the N modules of a layer,
// unfreeze_path) and approaches/pathnet.py:208-229 (clip_grad_norm + torch.optim.SGD over the trainable modules).
//
// Design: a PathNet layer is x_next = sum_n pool(relu(conv_{P[l,n]}(x))).  The next layer is linear in its input, so the
// sum is absorbed by its weights: conv_W(sum_m x_m) = conv_{[W W .. W]}(cat_m x_m).  A path therefore runs as a plain
// narrow net whose weights are ASSEMBLED from the modules (pack), and the gradient of a module is the sum of the packed
// gradient over the replicas of its weight (fold).  The conv / FC kernels and the engine are reused unchanged.
// Everything here is HBM-bound over a few hundred kB: three launches per batch, job tables by value, no host sync.
#include "common.hpp"

namespace {

constexpr int HB = 256;
constexpr int FOLD_MAX_BPM = 64;            // blocks per module in the fold / step launches

struct PJob { clhip_pathnet_layer l; int first_block; int n_blocks; };
struct PJobs { int n; int pad; PJob j[CLHIP_PATHNET_MAX_LAYERS]; };

__device__ __forceinline__ int job_of_block(const PJobs& J, int b) {
    int k = 0;
    for (int i = 1; i < J.n; ++i) k = (b >= J.j[i].first_block) ? i : k;
    return k;
}

// path[n] without a dynamically indexed copy of the kernel arguments in scratch
__device__ __forceinline__ int path_at(const clhip_pathnet_layer& l, int n) {
    int p = -1;
#pragma unroll
    for (int q = 0; q < CLHIP_PATHNET_MAX_N; ++q) p = (q == n && q < l.n_out) ? l.path[q] : p;
    return p;
}

__device__ __forceinline__ float pack_w(const clhip_pathnet_layer& l, const float* __restrict__ mod, unsigned i) {
    const unsigned CR = (unsigned)l.Cp * (unsigned)l.R;
    const unsigned kp = i / CR, rem = i - kp * CR;
    const unsigned cp = rem / (unsigned)l.R, r = rem - cp * (unsigned)l.R;
    const unsigned n = kp / (unsigned)l.c_out, k = kp - n * (unsigned)l.c_out;
    const unsigned m = cp / (unsigned)l.c_in, j = cp - m * (unsigned)l.c_in;
    if (n >= (unsigned)l.n_out || m >= (unsigned)l.n_in) return 0.f;
    const int p = path_at(l, (int)n);
    if (p < 0) return 0.f;
    return mod[l.w_off + (long)p * l.mod_stride + (long)((k * (unsigned)l.c_in + j) * (unsigned)l.R + r)];
}

__global__ __launch_bounds__(HB) void pathnet_pack_kernel(PJobs J, const float* __restrict__ mod, float* __restrict__ pk) {
    const PJob& jb = J.j[job_of_block(J, blockIdx.x)];
    const clhip_pathnet_layer& l = jb.l;
    const unsigned total = (unsigned)l.Kp * (unsigned)l.Cp * (unsigned)l.R;
    const unsigned stride = (unsigned)jb.n_blocks * HB, first = (unsigned)(blockIdx.x - jb.first_block) * HB + threadIdx.x;
    float* __restrict__ dw = pk + l.pw_off;
    const unsigned n4 = (((uintptr_t)dw & 15u) == 0) ? total / 4 : 0;          // 16-byte stores; the reads are gathers
    for (unsigned i = first; i < n4; i += stride)
        reinterpret_cast<float4*>(dw)[i] = make_float4(pack_w(l, mod, 4 * i), pack_w(l, mod, 4 * i + 1), pack_w(l, mod, 4 * i + 2),
                                                       pack_w(l, mod, 4 * i + 3));
    for (unsigned i = 4 * n4 + first; i < total; i += stride) dw[i] = pack_w(l, mod, i);
    float* __restrict__ db = pk + l.pb_off;
    for (unsigned i = first; i < (unsigned)l.Kp; i += stride) {
        const unsigned n = i / (unsigned)l.c_out, k = i - n * (unsigned)l.c_out;
        const int p = n < (unsigned)l.n_out ? path_at(l, (int)n) : -1;
        db[i] = p >= 0 ? mod[l.b_off + (long)p * l.mod_stride + k] : 0.f;
    }
}

// the module this block owns, or -1 when that module has no work (frozen, or in no slot of the path)
__device__ __forceinline__ int owned_module(const PJob& jb, int b, int& sub, int& bpm) {
    const clhip_pathnet_layer& l = jb.l;
    bpm = jb.n_blocks / l.M;
    const int rel = b - jb.first_block, mod = rel / bpm;
    sub = rel - mod * bpm;
    bool in_path = false;
#pragma unroll
    for (int q = 0; q < CLHIP_PATHNET_MAX_N; ++q) in_path |= (q < l.n_out && l.path[q] == mod);
    return (in_path && ((l.trainable >> mod) & 1ull)) ? mod : -1;
}

__device__ __forceinline__ double block_sum(double v, double* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = HB / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(HB) void pathnet_fold_kernel(PJobs J, const float* __restrict__ G, float* __restrict__ g,
                                                          double* __restrict__ partial) {
    __shared__ double part[HB];
    const PJob& jb = J.j[job_of_block(J, blockIdx.x)];
    const clhip_pathnet_layer& l = jb.l;
    int sub, bpm;
    const int mod = owned_module(jb, blockIdx.x, sub, bpm);
    if (mod < 0) {
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
        return;
    }
    const int JR = l.c_in * l.R, n_w = l.c_out * JR;
    const long CR = (long)l.Cp * l.R;
    double ss = 0.0;
    for (int e = sub * HB + threadIdx.x; e < n_w; e += bpm * HB) {
        const int k = e / JR, jr = e - k * JR;                     // jr = j*R + r: the replicas lie c_in*R floats apart
        float s = 0.f;
#pragma unroll
        for (int n = 0; n < CLHIP_PATHNET_MAX_N; ++n) {
            if (n < l.n_out && l.path[n] == mod) {
                const float* __restrict__ row = G + l.pw_off + (long)(n * l.c_out + k) * CR + jr;
                for (int m = 0; m < l.n_in; ++m) s += row[(long)m * JR];
            }
        }
        g[l.w_off + (long)mod * l.mod_stride + e] = s;
        ss += (double)s * (double)s;
    }
    if (sub == 0) {
        for (int k = threadIdx.x; k < l.c_out; k += HB) {
            float s = 0.f;
#pragma unroll
            for (int n = 0; n < CLHIP_PATHNET_MAX_N; ++n)
                if (n < l.n_out && l.path[n] == mod) s += G[l.pb_off + n * l.c_out + k];
            g[l.b_off + (long)mod * l.mod_stride + k] = s;
            ss += (double)s * (double)s;
        }
    }
    const double t = block_sum(ss, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(HB) void pathnet_sgd_kernel(PJobs J, float* __restrict__ theta, float* __restrict__ grad,
                                                         float* __restrict__ buf, float lr, float momentum, float wd,
                                                         float clipgrad, int first, const double* __restrict__ partial,
                                                         int n_partial) {
    __shared__ double part[HB];
    const PJob& jb = J.j[job_of_block(J, blockIdx.x)];
    const clhip_pathnet_layer& l = jb.l;
    int sub, bpm;
    const int mod = owned_module(jb, blockIdx.x, sub, bpm);
    if (mod < 0) return;
    double t = 0.0;                                               // every block: the same strided sums, the same tree
    for (int i = threadIdx.x; i < n_partial; i += HB) t += partial[i];
    const float norm = (float)sqrt(block_sum(t, part));
    const float c = clipgrad / (norm + 1e-6f);
    const float coef = c < 1.f ? c : 1.f;
    const bool mom = momentum != 0.f;
    auto one = [&](long i) {
        const float gc = grad[i] * coef;
        grad[i] = gc;
        const float th = theta[i];
        const float gv = gc + wd * th;
        float b = gv;
        if (mom) {
            if (!first) b = buf[i] * momentum + gv;
            buf[i] = b;
        }
        theta[i] = th - lr * b;
    };
    const int n_w = l.c_out * l.c_in * l.R;
    const long wb = l.w_off + (long)mod * l.mod_stride, bb = l.b_off + (long)mod * l.mod_stride;
    for (int e = sub * HB + threadIdx.x; e < n_w; e += bpm * HB) one(wb + e);
    if (sub == 0)
        for (int k = threadIdx.x; k < l.c_out; k += HB) one(bb + k);
}

bool layer_ok(const clhip_pathnet_layer& l) {
    if (l.c_out <= 0 || l.c_in <= 0 || l.R <= 0 || l.n_out <= 0 || l.n_out > CLHIP_PATHNET_MAX_N || l.n_in <= 0 ||
        l.n_in > CLHIP_PATHNET_MAX_N || l.M <= 0 || l.M > 64 || l.w_off < 0 || l.b_off < 0 || l.pw_off < 0 || l.pb_off < 0 ||
        l.mod_stride < 0)
        return false;
    if ((long)l.Kp < (long)l.n_out * l.c_out || (long)l.Cp < (long)l.n_in * l.c_in) return false;
    if ((double)l.Kp * l.Cp * l.R >= 2147483648.0) return false;
    for (int n = 0; n < l.n_out; ++n)
        if (l.path[n] >= l.M) return false;
    return true;
}

// the arenas must hold every slot the table names
bool fits(const clhip_pathnet_layer& l, size_t mod_numel, size_t packed_numel) {
    const size_t last = (size_t)(l.M - 1) * (size_t)l.mod_stride;
    return (size_t)l.w_off + last + (size_t)l.c_out * l.c_in * l.R <= mod_numel && (size_t)l.b_off + last + (size_t)l.c_out <= mod_numel &&
           (size_t)l.pw_off + (size_t)l.Kp * l.Cp * l.R <= packed_numel && (size_t)l.pb_off + (size_t)l.Kp <= packed_numel;
}

int fold_blocks(const clhip_pathnet_layer& l) {
    const size_t n = (size_t)l.c_out * l.c_in * l.R;
    size_t bpm = (n + (size_t)HB * 4 - 1) / ((size_t)HB * 4);
    if (bpm < 1) bpm = 1;
    if (bpm > FOLD_MAX_BPM) bpm = FOLD_MAX_BPM;
    return (int)bpm * l.M;
}

int fold_table(const clhip_pathnet_layer* layers, int n_layers, size_t mod_numel, size_t packed_numel, PJobs& J) {
    if (!layers || n_layers <= 0 || n_layers > CLHIP_PATHNET_MAX_LAYERS) return -1;
    J.n = n_layers; J.pad = 0;
    int blocks = 0;
    for (int i = 0; i < n_layers; ++i) {
        if (!layer_ok(layers[i]) || !fits(layers[i], mod_numel, packed_numel)) return -1;
        const int nb = fold_blocks(layers[i]);
        J.j[i] = PJob{layers[i], blocks, nb};
        blocks += nb;
    }
    return blocks;
}

}  // namespace

extern "C" {

size_t clhip_pathnet_ws(const clhip_pathnet_layer* layers, int n_layers) {
    if (!layers || n_layers <= 0 || n_layers > CLHIP_PATHNET_MAX_LAYERS) return 0;
    size_t blocks = 0;
    for (int i = 0; i < n_layers; ++i) {
        if (!layer_ok(layers[i])) return 0;
        blocks += (size_t)fold_blocks(layers[i]);
    }
    return blocks * sizeof(double);
}

int clhip_pathnet_pack_multi(const clhip_pathnet_layer* layers, int n_layers, const float* mod_theta, size_t mod_numel,
                             float* packed_theta, size_t packed_numel, void* stream) {
    if (!layers || n_layers <= 0 || n_layers > CLHIP_PATHNET_MAX_LAYERS || !mod_theta || !packed_theta) return CLHIP_EINVAL;
    PJobs J;
    J.n = n_layers; J.pad = 0;
    int blocks = 0;
    for (int i = 0; i < n_layers; ++i) {
        const clhip_pathnet_layer& l = layers[i];
        if (!layer_ok(l) || !fits(l, mod_numel, packed_numel)) return CLHIP_EINVAL;
        const size_t total = (size_t)l.Kp * l.Cp * l.R;
        size_t nb = (total + (size_t)HB * 16 - 1) / ((size_t)HB * 16);          // ~16 elements per thread
        if (nb < 1) nb = 1;
        if (nb > 2048) nb = 2048;
        J.j[i] = PJob{l, blocks, (int)nb};
        blocks += (int)nb;
    }
    hipLaunchKernelGGL(pathnet_pack_kernel, dim3(blocks), dim3(HB), 0, as_stream(stream), J, mod_theta, packed_theta);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_pathnet_fold_grads_multi(const clhip_pathnet_layer* layers, int n_layers, const float* packed_grad, size_t packed_numel,
                                   float* mod_grad, size_t mod_numel, void* ws, size_t ws_bytes, void* stream) {
    if (!packed_grad || !mod_grad || !ws) return CLHIP_EINVAL;
    PJobs J;
    const int blocks = fold_table(layers, n_layers, mod_numel, packed_numel, J);
    if (blocks <= 0 || ws_bytes < (size_t)blocks * sizeof(double)) return CLHIP_EINVAL;
    hipLaunchKernelGGL(pathnet_fold_kernel, dim3(blocks), dim3(HB), 0, as_stream(stream), J, packed_grad, mod_grad,
                       static_cast<double*>(ws));
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_pathnet_sgd_step(const clhip_pathnet_layer* layers, int n_layers, float* mod_theta, float* mod_grad, float* mod_buf,
                           size_t mod_numel, float lr, float momentum, float wd, float clipgrad, int first, const void* ws,
                           size_t ws_bytes, void* stream) {
    if (!mod_theta || !mod_grad || !mod_buf || !ws || !(clipgrad > 0.f)) return CLHIP_EINVAL;
    PJobs J;
    const int blocks = fold_table(layers, n_layers, mod_numel, (size_t)-1 / 2, J);
    if (blocks <= 0 || ws_bytes < (size_t)blocks * sizeof(double)) return CLHIP_EINVAL;
    hipLaunchKernelGGL(pathnet_sgd_kernel, dim3(blocks), dim3(HB), 0, as_stream(stream), J, mod_theta, mod_grad, mod_buf, lr,
                       momentum, wd, clipgrad, first, static_cast<const double*>(ws), blocks);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
