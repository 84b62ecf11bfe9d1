// LwF objective over stacked heads for any head size and up to CLHIP_LWF_MAX_HEADS_WIDE heads (clhip_lwf_loss_wide): the
// contract and the fp32 formulas of lwf_loss_kernel (loss.hip; methods/LwF/main_LWF.py:47-76, 184-202), spread over the GPU.
//   launch 1  lwf_wide_rows_kernel   one wave per batch row, 4 waves per block, ceil(N / 4) blocks.  The lanes of a wave run
//             across the columns of a head (consecutive lanes read consecutive floats, dword accesses only: ld, ld_teacher and
//             the head offsets are arbitrary, so no row and no head is assumed 16-byte aligned) and the wave loops over the
//             heads; row maxima, sums and the arg-max are wave reductions.  The wave writes its row's gradient and leaves
//             (task, distillation, hit) of the row in ws.
//   launch 2  lwf_wide_sum_kernel    one block sums the rows of ws in a fixed lane assignment (f64 partials + butterfly, as
//             phase 2 of loss_segments_kernel) and writes loss_out2 / stats.
// No atomics and no inter-block counters: every row's numbers depend on that row alone and the row sum has one order, so the
// result does not depend on scheduling.
#include "common.hpp"

namespace {

constexpr int WIDE_ROWS_PER_BLOCK = 4;               // one wave per row
constexpr int WIDE_SUM_BLOCK = 256;
constexpr int WIDE_MAX_ROWS = 1024;

struct LwfWideHeads { int n; int off[CLHIP_LWF_MAX_HEADS_WIDE]; int size[CLHIP_LWF_MAX_HEADS_WIDE]; };

// ws: three arrays of pad4(N) dwords: task[N] (f32), dist[N] (f32), hit[N] (i32)
__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }

// (value, column) arg-max over the wave: greater value, or equal value and lower column (torch.max's tie rule)
__device__ __forceinline__ int wave_argmax(float m, int am) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    return am;
}

// One head of one row.  NARROW (C <= 64): a lane holds its one column in a register (zv, tv), every loop below runs at
// most once and nothing is read twice; otherwise the columns are re-read from cache in every pass.
template <bool NARROW>
__device__ __forceinline__ void lwf_wide_head(const float* __restrict__ z, const float* __restrict__ t, float* __restrict__ dz, int C,
                                              int lane, bool last, int distill, int y, float invN, float invT, float lam,
                                              float& task, float& dist, int& hit) {
    float zv = 0.f, tv = 0.f;
    if (NARROW && lane < C) {
        zv = z[lane];
        if (!last && distill) tv = t[lane];
    }
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const float v = NARROW ? zv : z[c];
        if (v > m) { m = v; am = c; }                // strict: the first maximum of the lane's own columns
    }
    const float gm = wave_max(m);
    if (last) {
        am = wave_argmax(m, am);
        float se = 0.f;
        for (int c = lane; c < C; c += 64) se += expf((NARROW ? zv : z[c]) - gm);
        const float lse = logf(wave_sum(se));
        float zy = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = NARROW ? zv : z[c];
            dz[c] = (expf(v - gm - lse) - (c == y ? 1.f : 0.f)) * invN;
            if (c == y) zy = v;
        }
        zy = wave_sum(zy);                           // one lane holds z[y], the others 0
        task = -(zy - gm - lse);
        hit = (am == y) ? 1 : 0;
    } else if (distill) {
        float mt = -INFINITY;
        for (int c = lane; c < C; c += 64) mt = fmaxf(mt, NARROW ? tv : t[c]);
        mt = wave_max(mt);
        float st = 0.f;
        for (int c = lane; c < C; c += 64) st += expf((NARROW ? tv : t[c]) - mt);
        st = wave_sum(st);
        float sp = 0.f, sumex = 0.f;                 // sum_j softmax(t)_j^(1/T), sum_j exp((y_j - max y)/T)
        for (int c = lane; c < C; c += 64) {
            sp += powf(expf((NARROW ? tv : t[c]) - mt) / st, invT);
            sumex += expf(((NARROW ? zv : z[c]) - gm) * invT);
        }
        sp = wave_sum(sp);
        sumex = wave_sum(sumex);
        float cross = 0.f;
        const float g = lam * invN * invT;
        for (int c = lane; c < C; c += 64) {
            const float p = powf(expf((NARROW ? tv : t[c]) - mt) / st, invT) / sp;
            const float ys = ((NARROW ? zv : z[c]) - gm) * invT;
            cross += p * ys;
            dz[c] = g * (expf(ys) / sumex - p);
        }
        dist += logf(sumex) - wave_sum(cross);
    } else {
        for (int c = lane; c < C; c += 64) dz[c] = 0.f;
    }
}

__global__ __launch_bounds__(WIDE_ROWS_PER_BLOCK * 64) void lwf_wide_rows_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ teacher, LwfWideHeads hd, int N,
    int ld, int ld_t, float T, float lam, int distill, float* __restrict__ dlogits, float* __restrict__ ws_task,
    float* __restrict__ ws_dist, int* __restrict__ ws_hit) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WIDE_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= N) return;                            // whole waves leave; the kernel has no barrier
    const float* z = logits + (size_t)row * ld;
    const float* t = teacher ? teacher + (size_t)row * ld_t : nullptr;
    float* dz = dlogits + (size_t)row * ld;
    const int y = (int)labels[row];
    const float invN = 1.f / (float)N, invT = 1.f / T;
    float task = 0.f, dist = 0.f;
    int hit = 0;
    for (int h = 0; h < hd.n; ++h) {
        const int o = hd.off[h], C = hd.size[h];
        const bool last = h == hd.n - 1;
        const float* th = (!last && distill) ? t + o : nullptr;
        if (C <= 64) lwf_wide_head<true>(z + o, th, dz + o, C, lane, last, distill, y, invN, invT, lam, task, dist, hit);
        else lwf_wide_head<false>(z + o, th, dz + o, C, lane, last, distill, y, invN, invT, lam, task, dist, hit);
    }
    // columns past the last head carry no loss: zero, as lwf_loss_kernel writes them
    for (int c = hd.off[hd.n - 1] + hd.size[hd.n - 1] + lane; c < ld; c += 64) dz[c] = 0.f;
    if (lane == 0) { ws_task[row] = task; ws_dist[row] = dist; ws_hit[row] = hit; }
}

__global__ __launch_bounds__(WIDE_SUM_BLOCK) void lwf_wide_sum_kernel(const float* __restrict__ ws_task, const float* __restrict__ ws_dist,
                                                                      const int* __restrict__ ws_hit, int N, float lam,
                                                                      float* __restrict__ loss_out, double* __restrict__ stats) {
    __shared__ double s_t[WIDE_SUM_BLOCK / 64], s_d[WIDE_SUM_BLOCK / 64];
    __shared__ int s_c[WIDE_SUM_BLOCK / 64];
    double t = 0.0, d = 0.0;
    int c = 0;
    for (int r = threadIdx.x; r < N; r += WIDE_SUM_BLOCK) { t += (double)ws_task[r]; d += (double)ws_dist[r]; c += ws_hit[r]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { t += __shfl_xor(t, o, 64); d += __shfl_xor(d, o, 64); c += __shfl_xor(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_t[threadIdx.x >> 6] = t; s_d[threadIdx.x >> 6] = d; s_c[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tt = 0.0, dd = 0.0;
        int cc = 0;
        for (int i = 0; i < WIDE_SUM_BLOCK / 64; ++i) { tt += s_t[i]; dd += s_d[i]; cc += s_c[i]; }        // fixed order
        const float tf = (float)(tt / (double)N), df = (float)((double)lam * dd / (double)N);
        loss_out[0] = tf; loss_out[1] = df;
        if (stats) { stats[0] += (double)tf; stats[1] += (double)cc; }
    }
}

}  // namespace

extern "C" {

size_t clhip_lwf_loss_wide_ws(int n_heads, int N) {
    if (n_heads < 1 || n_heads > CLHIP_LWF_MAX_HEADS_WIDE || N < 1 || N > WIDE_MAX_ROWS) return 0;
    return (size_t)3 * pad4(N) * 4;
}

int clhip_lwf_loss_wide(const float* logits, const int64_t* labels_i64, const float* teacher, const int* head_sizes, int n_heads,
                        int N, int ld, int ld_teacher, float T, float reg_lambda, int distill, float* dlogits, float* loss_out2,
                        double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !labels_i64 || !head_sizes || !dlogits || !loss_out2 || !ws) return CLHIP_EINVAL;
    if (n_heads < 1 || n_heads > CLHIP_LWF_MAX_HEADS_WIDE) return CLHIP_EINVAL;
    long long width = 0;
    for (int h = 0; h < n_heads; ++h) {
        if (head_sizes[h] <= 0) return CLHIP_EINVAL;
        width += head_sizes[h];
    }
    if (width > ld) return CLHIP_EINVAL;                                         // from here on every offset fits an int
    LwfWideHeads hd; hd.n = n_heads;
    int off = 0;
    for (int h = 0; h < CLHIP_LWF_MAX_HEADS_WIDE; ++h) {
        hd.off[h] = off; hd.size[h] = h < n_heads ? head_sizes[h] : 0;
        off += hd.size[h];
    }
    const bool distils = distill && n_heads > 1;
    if (distils && off - head_sizes[n_heads - 1] > ld_teacher) return CLHIP_EINVAL;
    if (N < 1 || N > WIDE_MAX_ROWS) return CLHIP_EINVAL;
    if (!(T > 0.f)) return CLHIP_EINVAL;
    if (distils && !teacher) return CLHIP_EINVAL;
    if (ws_bytes < clhip_lwf_loss_wide_ws(n_heads, N)) return CLHIP_ENOSPC;
    float* ws_task = static_cast<float*>(ws);
    float* ws_dist = ws_task + pad4(N);
    int* ws_hit = reinterpret_cast<int*>(ws_dist + pad4(N));
    hipLaunchKernelGGL(lwf_wide_rows_kernel, dim3((N + WIDE_ROWS_PER_BLOCK - 1) / WIDE_ROWS_PER_BLOCK), dim3(WIDE_ROWS_PER_BLOCK * 64), 0,
                       as_stream(stream), logits, labels_i64, teacher, hd, N, ld, ld_teacher, T, reg_lambda, distils ? 1 : 0, dlogits,
                       ws_task, ws_dist, ws_hit);
    CLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(lwf_wide_sum_kernel, dim3(1), dim3(WIDE_SUM_BLOCK), 0, as_stream(stream), ws_task, ws_dist, ws_hit, N, reg_lambda,
                       loss_out2, stats);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
