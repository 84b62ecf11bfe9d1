// iCaRL (rehearsal/model/icarl.py): herding of the exemplar sets (manage_memory :384-471) over features computed once, the
// CE + distillation loss of update_representation (:482-598) over one mixed batch, and the nearest-mean-of-exemplars
// classifier of Net.forward (:142-186).
#include "common.hpp"

namespace {

constexpr int HERD_BLOCK = 1024;          // 16 waves, one block per class
constexpr int HERD_WAVES = HERD_BLOCK / 64;
constexpr int LOSS_BLOCK = 1024;          // one block: fixed reduction order
constexpr int LOSS_MAX_ROWS = 1024;
constexpr int NME_BLOCK = 256;            // one wave per row

struct herd_table { clhip_icarl_class c[CLHIP_ICARL_MAX_CLASSES]; };

__device__ __forceinline__ float wmax_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wsum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wsum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wmin_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// One block per class.  LDS: mu[F] (the weighted class mean), S[F] (sum of the features chosen so far), r[F] = (k+1) mu - S,
// and one `taken` bit per row of the class.  Pick k: every wave walks rows wave, wave + 16, ... of the class; its lanes walk the
// row in float4 (or scalar) steps, d = r - f in fp32, d*d summed in f64, butterfly over the lanes (fixed order); the wave
// keeps its smallest (cost, row), the 16 candidates meet in LDS.  ||mu - (f + S) / (k+1)|| = ||r - f|| / (k+1): the same
// arg-min without a division per element.  Equal costs: the lowest row wins.
template <bool VEC>
__global__ __launch_bounds__(HERD_BLOCK) void icarl_herd_kernel(const float* __restrict__ feats, int F, const float* __restrict__ w,
                                                                herd_table tab, int* __restrict__ ranking) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const clhip_icarl_class cls = tab.c[blockIdx.x];
    const int n = cls.row_end - cls.row_begin;
    float* mu = lds;
    float* S = lds + F;
    float* r = lds + 2 * (size_t)F;
    unsigned* taken = reinterpret_cast<unsigned*>(lds + 3 * (size_t)F);
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
            acc = wsum_d(acc);
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

// Phase 1: one wave per row (rows strided over the 16 waves) computes the row's value over its class slice and keeps the
// row's softmax statistics in LDS; phase 2: one wave per segment sums its rows in f64 (fixed lane assignment + butterfly)
// and decides the segment's gate (a distillation segment whose own value is negative counts as the integer 0 of :584-587:
// no loss, no gradient); phase 3: the gradient rows; thread 0 sums the segments in order.
__global__ __launch_bounds__(LOSS_BLOCK) void icarl_loss_segments_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ targets, int ld_t, int N, int ld,
    const clhip_icarl_segment* __restrict__ segs, int n_segs, float T, float* __restrict__ dlogits, float* __restrict__ loss_out,
    double* __restrict__ stats) {
    __shared__ clhip_icarl_segment s_seg[CLHIP_CE_MAX_SEGS];
    __shared__ int s_valid[CLHIP_CE_MAX_SEGS];
    __shared__ float s_gate[CLHIP_CE_MAX_SEGS];
    __shared__ double s_part[CLHIP_CE_MAX_SEGS];
    __shared__ float s_val[LOSS_MAX_ROWS];
    __shared__ float s_zm[LOSS_MAX_ROWS], s_zl[LOSS_MAX_ROWS], s_tm[LOSS_MAX_ROWS], s_tl[LOSS_MAX_ROWS];
    __shared__ short s_rowseg[LOSS_MAX_ROWS];
    __shared__ unsigned char s_hit[LOSS_MAX_ROWS];
    __shared__ int s_bad, s_hits;
    if (threadIdx.x == 0) { s_bad = 0; s_hits = 0; }
    for (int g = threadIdx.x; g < n_segs; g += LOSS_BLOCK) {
        const clhip_icarl_segment sg = segs[g];
        s_seg[g] = sg;
        s_valid[g] = sg.row_begin >= 0 && sg.row_begin < sg.row_end && sg.row_end <= N && sg.col_off >= 0 && sg.ncols > 0 &&
                     sg.col_off + sg.ncols <= ld && (sg.kind == 0 || (sg.kind == 1 && targets && sg.col_off + sg.ncols <= ld_t));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float invT = 1.f / T;
    for (int row = wave; row < N; row += LOSS_BLOCK / 64) {
        int g = -1;                                    // first valid segment that holds the row (wave-uniform scan)
        for (int k = 0; k < n_segs; ++k)
            if (s_valid[k] && row >= s_seg[k].row_begin && row < s_seg[k].row_end) { g = k; break; }
        if (lane == 0) s_rowseg[row] = (short)g;
        if (g < 0) {
            if (lane == 0) { s_val[row] = 0.f; s_hit[row] = 0; }
            continue;
        }
        const int o = s_seg[g].col_off, C = s_seg[g].ncols;
        const float* z = logits + (size_t)row * ld + o;
        if (s_seg[g].kind == 0) {
            const int y = (int)labels[row];
            const bool ok = y >= 0 && y < C;
            float m = -INFINITY;
            int am = 0x7fffffff;
            for (int c = lane; c < C; c += 64) {
                const float v = z[c];
                if (v > m) { m = v; am = c; }
            }
            const float gm = wmax_f(m);
            am = wmin_i(m == gm ? am : 0x7fffffff);               // torch.max tie rule: lowest index
            float se = 0.f;
            for (int c = lane; c < C; c += 64) se += expf(z[c] - gm);
            const float lse = logf(wsum_f(se));
            if (lane == 0) {
                if (!ok) s_bad = 1;
                s_val[row] = ok ? -(z[y] - gm - lse) : 0.f;
                s_hit[row] = (unsigned char)(g == 0 && am == y);
                s_zm[row] = gm; s_zl[row] = lse;
            }
        } else {
            const float* tr = targets + (size_t)row * ld_t + o;
            float zm = -INFINITY, tm = -INFINITY;
            for (int c = lane; c < C; c += 64) { zm = fmaxf(zm, z[c] * invT); tm = fmaxf(tm, tr[c] * invT); }
            zm = wmax_f(zm); tm = wmax_f(tm);
            float zs = 0.f, ts = 0.f;
            for (int c = lane; c < C; c += 64) { zs += expf(z[c] * invT - zm); ts += expf(tr[c] * invT - tm); }
            const float zl = logf(wsum_f(zs)), tl = logf(wsum_f(ts));
            float kl = 0.f;                                       // sum_c p (log p - log q), p = softmax(target / T), q = softmax(z / T)
            for (int c = lane; c < C; c += 64) {
                const float lp = tr[c] * invT - tm - tl, lq = z[c] * invT - zm - zl;
                const float p = expf(lp);
                kl += p > 0.f ? p * (lp - lq) : 0.f;
            }
            kl = wsum_f(kl);
            if (lane == 0) {
                s_val[row] = kl * T * T;
                s_hit[row] = 0;
                s_zm[row] = zm; s_zl[row] = zl; s_tm[row] = tm; s_tl[row] = tl;
            }
        }
    }
    __syncthreads();
    for (int g = wave; g < n_segs; g += LOSS_BLOCK / 64) {
        double t = 0.0;
        int h = 0;
        if (s_valid[g]) {
            for (int r = s_seg[g].row_begin + lane; r < s_seg[g].row_end; r += 64) {
                if (s_rowseg[r] == g) { t += (double)s_val[r]; h += s_hit[r]; }    // a row counts for the first segment that holds it
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { t += __shfl_xor(t, off, 64); h += __shfl_xor(h, off, 64); }
        if (lane == 0) {
            double v = s_valid[g] ? t / (double)(s_seg[g].row_end - s_seg[g].row_begin) : 0.0;
            const bool off_ = s_valid[g] && s_seg[g].kind == 1 && (float)v < 0.f;
            s_gate[g] = off_ ? 0.f : 1.f;
            s_part[g] = (s_valid[g] && !off_) ? (double)s_seg[g].scale * v : 0.0;
            if (g == 0) s_hits = h;
        }
    }
    __syncthreads();
    for (int row = wave; row < N; row += LOSS_BLOCK / 64) {
        const int g = s_rowseg[row];
        float* dz = dlogits + (size_t)row * ld;
        if (g < 0 || s_gate[g] == 0.f) {
            for (int c = lane; c < ld; c += 64) dz[c] = 0.f;
            continue;
        }
        const int o = s_seg[g].col_off, C = s_seg[g].ncols;
        const float wgt = s_seg[g].scale / (float)(s_seg[g].row_end - s_seg[g].row_begin);
        const float* zr = logits + (size_t)row * ld;
        if (s_seg[g].kind == 0) {
            const int y = (int)labels[row];
            const float gm = s_zm[row], lse = s_zl[row];
            for (int c = lane; c < ld; c += 64) {
                const int cc = c - o;
                dz[c] = (cc >= 0 && cc < C) ? (expf(zr[c] - gm - lse) - (cc == y ? 1.f : 0.f)) * wgt : 0.f;
            }
        } else {
            const float* tr = targets + (size_t)row * ld_t;
            const float zm = s_zm[row], zl = s_zl[row], tm = s_tm[row], tl = s_tl[row];
            const float wT = wgt * T;                             // d/dz of T^2 KL = T (q - p)
            for (int c = lane; c < ld; c += 64) {
                const int cc = c - o;
                dz[c] = (cc >= 0 && cc < C) ? (expf(zr[c] * invT - zm - zl) - expf(tr[c] * invT - tm - tl)) * wT : 0.f;
            }
        }
    }
    if (threadIdx.x == 0) {
        double td = 0.0;
        for (int g = 0; g < n_segs; ++g) td += s_part[g];
        float t = (float)td;
        bool bad = s_bad != 0;
        for (int g = 0; g < n_segs; ++g) bad = bad || !s_valid[g];
        if (bad) t = __int_as_float(0x7fc00000);      // a malformed table or label is reported as a NaN loss
        loss_out[0] = t;
        if (stats) { stats[0] += (double)t; stats[1] += (double)s_hits; }
    }
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
        const float dist = (float)sqrt(wsum_d(acc));
        if (dist < best) { best = dist; arg = c; }               // the first minimum wins
    }
    for (int c = lane; c < n_outputs; c += 64) orow[c] = (c == offset1 + arg) ? 1.f : 0.f;
}

}  // namespace

extern "C" {

int clhip_icarl_herd(const float* feats, long n_rows, int F, const float* w, const clhip_icarl_class* classes_host,
                     int n_classes, int* ranking, long ranking_len, void* stream) {
    if (!feats || !w || !classes_host || !ranking) return CLHIP_EINVAL;
    if (n_rows <= 0 || F <= 0 || F > CLHIP_ICARL_MAX_FEATS || n_classes < 1 || n_classes > CLHIP_ICARL_MAX_CLASSES) return CLHIP_EINVAL;
    herd_table tab;
    int max_rows = 0;
    for (int c = 0; c < n_classes; ++c) {
        const clhip_icarl_class& k = classes_host[c];
        const long n = (long)k.row_end - k.row_begin;
        if (k.row_begin < 0 || n <= 0 || k.row_end > n_rows || n > CLHIP_ICARL_MAX_CLASS_ROWS) return CLHIP_EINVAL;
        if (k.k < 0 || k.k > n || k.out_off < 0 || (long)k.out_off + k.k > ranking_len) return CLHIP_EINVAL;
        tab.c[c] = k;
        if (n > max_rows) max_rows = (int)n;
    }
    const size_t lds = 3 * (size_t)F * sizeof(float) + (size_t)((max_rows + 31) / 32) * sizeof(unsigned);
    if (F % 4 == 0 && aligned16(feats))
        hipLaunchKernelGGL(icarl_herd_kernel<true>, dim3(n_classes), dim3(HERD_BLOCK), lds, as_stream(stream), feats, F, w, tab, ranking);
    else
        hipLaunchKernelGGL(icarl_herd_kernel<false>, dim3(n_classes), dim3(HERD_BLOCK), lds, as_stream(stream), feats, F, w, tab, ranking);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_icarl_loss_segments(const float* logits, const int64_t* labels_i64, const float* targets, int ld_t, int N, int ld,
                              const clhip_icarl_segment* segs, int n_segs, float T, float* dlogits, float* loss_out,
                              double* stats, void* stream) {
    if (!logits || !labels_i64 || !segs || !dlogits || !loss_out) return CLHIP_EINVAL;
    if (N <= 0 || N > LOSS_MAX_ROWS || ld <= 0 || n_segs < 1 || n_segs > CLHIP_CE_MAX_SEGS || !(T > 0.f)) return CLHIP_EINVAL;
    if (targets && ld_t <= 0) return CLHIP_EINVAL;
    hipLaunchKernelGGL(icarl_loss_segments_kernel, dim3(1), dim3(LOSS_BLOCK), 0, as_stream(stream), logits, labels_i64, targets, ld_t, N,
                       ld, segs, n_segs, T, dlogits, loss_out, stats);
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
