// iCaRL (rehearsal/model/icarl.py): herding of the exemplar sets (manage_memory :384-471) over features computed once and the
// nearest-mean-of-exemplars classifier of Net.forward (:142-186).  The loss of update_representation is loss.hip's
// segmented loss.
#include "common.hpp"

namespace {

constexpr int HERD_BLOCK = 1024;          // 16 waves, one block per class
constexpr int HERD_WAVES = HERD_BLOCK / 64;
constexpr int NME_BLOCK = 256;            // one wave per row

struct herd_table { clhip_icarl_class c[CLHIP_ICARL_MAX_CLASSES]; };

// The block of one class, shared by the two herding kernels: they differ in where mu[F] (the weighted class mean) and S[F] (sum
// of the features chosen so far) live.  r[F] = (k+1) mu - S and one `taken` bit per row of the class are in LDS.  Pick k: every
// wave walks rows wave, wave + 16, ... of the class; its lanes walk the row in float4 (or scalar) steps, d = r - f in fp32, d*d
// summed in f64, butterfly over the lanes (fixed order); the wave keeps its smallest (cost, row), the 16 candidates meet in
// LDS.  ||mu - (f + S) / (k+1)|| = ||r - f|| / (k+1): the same arg-min without a division per element.  Equal costs: the
// lowest row wins.  Thread j reads only the mu[j], S[j] it wrote itself: no fence where they are in device memory.
template <bool VEC>
__device__ __forceinline__ void herd_block(const float* __restrict__ feats, int F, const float* __restrict__ w,
                                           const clhip_icarl_class cls, int* __restrict__ ranking, float* mu, float* S, float* r,
                                           unsigned* taken) {
    const int n = cls.row_end - cls.row_begin;
    __shared__ double s_cost[HERD_WAVES];
    __shared__ int s_row[HERD_WAVES];
    __shared__ int s_win;
    const float* base = feats + (size_t)cls.row_begin * F;
    const float* wc = w + cls.row_begin;
    for (int j = threadIdx.x; j < F; j += HERD_BLOCK) {           // mu = sum_i w_i f_i, column per thread (coalesced rows), f64
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += (double)wc[i] * (double)base[(size_t)i * F + j];
        mu[j] = (float)acc;
        S[j] = 0.f;
        r[j] = (float)acc;
    }
    for (int i = threadIdx.x; i < (n + 31) / 32; i += HERD_BLOCK) taken[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < cls.k; ++k) {
        double best = INFINITY;
        int best_row = 0x7fffffff;
        for (int i = wave; i < n; i += HERD_WAVES) {
            if ((taken[i >> 5] >> (i & 31)) & 1u) continue;       // wave-uniform
            const float* f = base + (size_t)i * F;
            double acc = 0.0;
            if (VEC) {
                const float4* f4 = reinterpret_cast<const float4*>(f);
                const float4* r4 = reinterpret_cast<const float4*>(r);
                for (int j = lane; j < F / 4; j += 64) {
                    const float4 a = f4[j], b = r4[j];
                    const float d0 = b.x - a.x, d1 = b.y - a.y, d2 = b.z - a.z, d3 = b.w - a.w;
                    acc += (double)d0 * d0 + (double)d1 * d1 + (double)d2 * d2 + (double)d3 * d3;
                }
            } else {
                for (int j = lane; j < F; j += 64) {
                    const float d = r[j] - f[j];
                    acc += (double)d * d;
                }
            }
            acc = wave_sum(acc);
            if (acc < best) { best = acc; best_row = i; }         // rows ascend within a wave: the first minimum stays
        }
        if (lane == 0) { s_cost[wave] = best; s_row[wave] = best_row; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double b = s_cost[0];
            int br = s_row[0];
            for (int q = 1; q < HERD_WAVES; ++q)
                if (s_cost[q] < b || (s_cost[q] == b && s_row[q] < br)) { b = s_cost[q]; br = s_row[q]; }
            s_win = br;
            if (br != 0x7fffffff) {
                taken[br >> 5] |= 1u << (br & 31);
                ranking[cls.out_off + k] = br;
            } else {
                ranking[cls.out_off + k] = -1;                    // (k <= n is checked on the host: not reached)
            }
        }
        __syncthreads();
        const int win = s_win;
        if (win != 0x7fffffff) {
            const float* f = base + (size_t)win * F;
            const float kk = (float)(k + 2);
            for (int j = threadIdx.x; j < F; j += HERD_BLOCK) {
                const float s = S[j] + f[j];
                S[j] = s;
                r[j] = kk * mu[j] - s;
            }
        }
        __syncthreads();
    }
}

// One block per class, F <= CLHIP_ICARL_MAX_FEATS.  Dynamic LDS: mu[F], S[F], r[F], taken bits of the largest class.
template <bool VEC>
__global__ __launch_bounds__(HERD_BLOCK) void icarl_herd_kernel(const float* __restrict__ feats, int F, const float* __restrict__ w,
                                                                herd_table tab, int* __restrict__ ranking) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    herd_block<VEC>(feats, F, w, tab.c[blockIdx.x], ranking, lds, lds + F, lds + 2 * (size_t)F,
                    reinterpret_cast<unsigned*>(lds + 3 * (size_t)F));
}

// One block per class, F <= CLHIP_ICARL_MAX_FEATS_WIDE.  Only r is read in the pick loop, so only r (64 KB) and the taken bits
// of CLHIP_ICARL_MAX_CLASS_ROWS rows (8 KB) are in LDS, declared statically; mu and S of class c are ws[c][0][F], ws[c][1][F],
// touched once per pick in the update loop.
template <bool VEC>
__global__ __launch_bounds__(HERD_BLOCK) void icarl_herd_wide_kernel(const float* __restrict__ feats, int F,
                                                                     const float* __restrict__ w, herd_table tab,
                                                                     int* __restrict__ ranking, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float r[CLHIP_ICARL_MAX_FEATS_WIDE];
    __shared__ unsigned taken[CLHIP_ICARL_MAX_CLASS_ROWS / 32];
    float* mu = ws + (size_t)blockIdx.x * 2 * F;
    herd_block<VEC>(feats, F, w, tab.c[blockIdx.x], ranking, mu, mu + F, r, taken);
}

// One wave per row.  means == nullptr: the task has no exemplars yet (:146-155).
__global__ __launch_bounds__(NME_BLOCK) void icarl_nme_kernel(const float* __restrict__ feats, const float* __restrict__ means,
                                                              int N, int F, int C, int offset1, int n_outputs,
                                                              float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (NME_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= N) return;
    float* orow = out + (size_t)row * n_outputs;
    if (!means) {
        const float u = 1.0f / (float)C;
        for (int c = lane; c < n_outputs; c += 64) orow[c] = (c >= offset1 && c < offset1 + C) ? u : -10e10f;
        return;
    }
    const float* f = feats + (size_t)row * F;
    float best = INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
        const float* m = means + (size_t)c * F;
        double acc = 0.0;
        for (int j = lane; j < F; j += 64) {
            const float d = m[j] - f[j];
            acc += (double)d * d;
        }
        const float dist = (float)sqrt(wave_sum(acc));
        if (dist < best) { best = dist; arg = c; }               // the first minimum wins
    }
    for (int c = lane; c < n_outputs; c += 64) orow[c] = (c == offset1 + arg) ? 1.f : 0.f;
}

}  // namespace

extern "C" {

// The checks both herding entries share; fills the table and the row count of the largest class.
static int herd_table_fill(const float* feats, long n_rows, int F, int max_feats, const float* w, const clhip_icarl_class* classes_host,
                           int n_classes, const int* ranking, long ranking_len, herd_table* tab, int* max_rows_out) {
    if (!feats || !w || !classes_host || !ranking) return CLHIP_EINVAL;
    if (n_rows <= 0 || F <= 0 || F > max_feats || n_classes < 1 || n_classes > CLHIP_ICARL_MAX_CLASSES) return CLHIP_EINVAL;
    int max_rows = 0;
    for (int c = 0; c < n_classes; ++c) {
        const clhip_icarl_class& k = classes_host[c];
        const long n = (long)k.row_end - k.row_begin;
        if (k.row_begin < 0 || n <= 0 || k.row_end > n_rows || n > CLHIP_ICARL_MAX_CLASS_ROWS) return CLHIP_EINVAL;
        if (k.k < 0 || k.k > n || k.out_off < 0 || (long)k.out_off + k.k > ranking_len) return CLHIP_EINVAL;
        tab->c[c] = k;
        if (n > max_rows) max_rows = (int)n;
    }
    *max_rows_out = max_rows;
    return 0;
}

size_t clhip_icarl_herd_wide_ws(int n_classes, int F) {
    if (n_classes < 1 || n_classes > CLHIP_ICARL_MAX_CLASSES || F < 1 || F > CLHIP_ICARL_MAX_FEATS_WIDE) return 0;
    return (size_t)n_classes * 2 * (size_t)F * sizeof(float);
}

int clhip_icarl_herd_wide(const float* feats, long n_rows, int F, const float* w, const clhip_icarl_class* classes_host,
                          int n_classes, int* ranking, long ranking_len, void* ws, size_t ws_bytes, void* stream) {
    herd_table tab;
    int max_rows = 0;
    const int rc = herd_table_fill(feats, n_rows, F, CLHIP_ICARL_MAX_FEATS_WIDE, w, classes_host, n_classes, ranking, ranking_len, &tab,
                                   &max_rows);
    if (rc) return rc;
    if (!ws || ws_bytes < clhip_icarl_herd_wide_ws(n_classes, F)) return CLHIP_EINVAL;
    float* wsf = static_cast<float*>(ws);
    if (F % 4 == 0 && aligned16(feats))
        hipLaunchKernelGGL(icarl_herd_wide_kernel<true>, dim3(n_classes), dim3(HERD_BLOCK), 0, as_stream(stream), feats, F, w, tab, ranking,
                           wsf);
    else
        hipLaunchKernelGGL(icarl_herd_wide_kernel<false>, dim3(n_classes), dim3(HERD_BLOCK), 0, as_stream(stream), feats, F, w, tab,
                           ranking, wsf);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_icarl_herd(const float* feats, long n_rows, int F, const float* w, const clhip_icarl_class* classes_host,
                     int n_classes, int* ranking, long ranking_len, void* stream) {
    herd_table tab;
    int max_rows = 0;
    const int rc = herd_table_fill(feats, n_rows, F, CLHIP_ICARL_MAX_FEATS, w, classes_host, n_classes, ranking, ranking_len, &tab,
                                   &max_rows);
    if (rc) return rc;
    const size_t lds = 3 * (size_t)F * sizeof(float) + (size_t)((max_rows + 31) / 32) * sizeof(unsigned);
    if (F % 4 == 0 && aligned16(feats))
        hipLaunchKernelGGL(icarl_herd_kernel<true>, dim3(n_classes), dim3(HERD_BLOCK), lds, as_stream(stream), feats, F, w, tab, ranking);
    else
        hipLaunchKernelGGL(icarl_herd_kernel<false>, dim3(n_classes), dim3(HERD_BLOCK), lds, as_stream(stream), feats, F, w, tab, ranking);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_icarl_nme(const float* feats, const float* means, int N, int F, int C, int offset1, int n_outputs, float* out,
                    void* stream) {
    if (!out || N <= 0 || C <= 0 || offset1 < 0 || offset1 + C > n_outputs) return CLHIP_EINVAL;
    if (means && (!feats || F <= 0)) return CLHIP_EINVAL;
    const int rows_per_block = NME_BLOCK / 64;
    hipLaunchKernelGGL(icarl_nme_kernel, dim3((N + rows_per_block - 1) / rows_per_block), dim3(NME_BLOCK), 0, as_stream(stream), feats,
                       means, N, F, C, offset1, n_outputs, out);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
