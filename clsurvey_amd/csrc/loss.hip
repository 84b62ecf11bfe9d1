// Loss kernels: softmax cross-entropy (mean / sum), the MAS sum-of-squares objective, LwF's stacked heads and the
// segmented CE / distillation loss of the exemplar methods.
// Tiny tensors ([N<=~1k][C<=1k]); one block, fixed reduction order => deterministic.
#include "common.hpp"

namespace {

constexpr int LOSS_BLOCK = 1024;  // 16 waves

// One wave per row, rows strided over the 16 waves of the single block.  The tensor is tiny, so
// the kernel is pure latency: rows are fetched RB at a time per wave (all loads in flight
// together) before any arithmetic, instead of one dependent round trip per row.
template <int RB>
__global__ __launch_bounds__(LOSS_BLOCK) void softmax_ce_kernel(
    const float* __restrict__ logits_full, const int64_t* __restrict__ labels, int N, int C, int reduction,
    float* __restrict__ dlogits_full, float* __restrict__ loss_out, double* __restrict__ stats, int ld, int col_off) {
    // logits_full is [N][ld]; the loss is taken over columns [col_off, col_off + C) (labels are relative to
    // the slice); dlogits outside the slice are written as 0.
    const float* logits = logits_full + col_off;
    float* dlogits = dlogits_full + col_off;
    if (ld != C) {
        for (size_t i = threadIdx.x; i < (size_t)N * ld; i += LOSS_BLOCK) {
            int c = (int)(i % ld);
            if (c < col_off || c >= col_off + C) dlogits_full[i] = 0.f;
        }
    }
    __shared__ float s_loss[16];
    __shared__ int s_corr[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float scale = reduction == 0 ? 1.f / (float)N : 1.f;
    float wl = 0.f;   // this wave's loss sum (rows in increasing order)
    int wc = 0;
    const bool narrow = C <= 64;
    for (int row0 = wave; row0 < N; row0 += 16 * RB) {
        float zr[RB];
        int yr[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            int row = row0 + 16 * b;
            zr[b] = (narrow && row < N && lane < C) ? logits[(size_t)row * ld + lane] : -INFINITY;
            yr[b] = (row < N) ? (int)labels[row] : 0;
        }
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            int row = row0 + 16 * b;
            if (row >= N) break;
            const float* z = logits + (size_t)row * ld;
            const int y = yr[b];
            float m = -INFINITY;
            int am = 0x7fffffff;
            if (narrow) {
                m = zr[b];
                am = lane < C ? lane : 0x7fffffff;
            } else {
                for (int c = lane; c < C; c += 64) {
                    float v = z[c];
                    if (v > m) { m = v; am = c; }
                }
            }
            float gm = wave_max(m);
            // first index attaining the max (torch.max tie rule: lowest index)
            const int cand = wave_min((m == gm) ? am : 0x7fffffff);
            float se = 0.f, zy;
            if (narrow) {
                float ex = lane < C ? expf(zr[b] - gm) : 0.f;
                se = wave_sum(ex);
                const float lse = logf(se);
                if (lane < C) dlogits[(size_t)row * ld + lane] = (expf(zr[b] - gm - lse) - (lane == y ? 1.f : 0.f)) * scale;
                zy = __shfl(zr[b], y, 64);
                wl += -(zy - gm - lse);
            } else {
                for (int c = lane; c < C; c += 64) se += expf(z[c] - gm);
                se = wave_sum(se);
                const float lse = logf(se);
                for (int c = lane; c < C; c += 64)
                    dlogits[(size_t)row * ld + c] = (expf(z[c] - gm - lse) - (c == y ? 1.f : 0.f)) * scale;
                zy = z[y];
                wl += -(zy - gm - lse);
            }
            wc += (cand == y) ? 1 : 0;
        }
    }
    if (lane == 0) { s_loss[wave] = wl; s_corr[wave] = wc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f; int c = 0;
        for (int i = 0; i < 16; ++i) { t += s_loss[i]; c += s_corr[i]; }
        t *= scale;
        loss_out[0] = t;
        if (stats) { stats[0] += (double)t; stats[1] += (double)c; }
    }
}

// Narrow heads (C <= 64, the 20-way task heads): one THREAD per row, no cross-lane traffic; rows are
// summed in index order by thread 0 afterwards (deterministic).  N <= 1024.
__global__ __launch_bounds__(LOSS_BLOCK) void softmax_ce_rows_kernel(
    const float* __restrict__ logits_full, const int64_t* __restrict__ labels, int N, int C, int reduction,
    float* __restrict__ dlogits_full, float* __restrict__ loss_out, double* __restrict__ stats, int ld, int col_off) {
    __shared__ float s_loss[LOSS_BLOCK];
    __shared__ unsigned char s_corr[LOSS_BLOCK];
    const int row = threadIdx.x;
    const float scale = reduction == 0 ? 1.f / (float)N : 1.f;
    float li = 0.f;
    int ok = 0;
    if (row < N) {
        const float* z = logits_full + (size_t)row * ld + col_off;
        float* dz = dlogits_full + (size_t)row * ld;
        const int y = (int)labels[row];
        float m = -INFINITY;
        int am = 0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            float v = z[c];
            if (v > m) { m = v; am = c; }
        }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(z[c] - m);
        const float lse = logf(se);
        for (int c = 0; c < ld; ++c) {
            const int cc = c - col_off;
            dz[c] = (cc >= 0 && cc < C) ? (expf(z[cc] - m - lse) - (cc == y ? 1.f : 0.f)) * scale : 0.f;
        }
        li = -(z[y] - m - lse);
        ok = (am == y);
    }
    s_loss[row] = li;
    s_corr[row] = (unsigned char)ok;
    __syncthreads();
    // fixed-order reduction: wave w sums rows w*64 .. w*64+63 with a butterfly, thread 0 adds the 16 wave sums
    __shared__ float w_loss[16];
    __shared__ int w_corr[16];
    float v = s_loss[row];
    int cc = s_corr[row];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); cc += __shfl_xor(cc, o, 64); }
    if ((threadIdx.x & 63) == 0) { w_loss[threadIdx.x >> 6] = v; w_corr[threadIdx.x >> 6] = cc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f; int c = 0;
        for (int w = 0; w < 16; ++w) { t += w_loss[w]; c += w_corr[w]; }
        t *= scale;
        loss_out[0] = t;
        if (stats) { stats[0] += (double)t; stats[1] += (double)c; }
    }
}

// Same arithmetic as softmax_ce_rows_kernel with the whole [N][ld] logit block staged through LDS: coalesced loads and
// stores instead of three latency-serialised passes of row-strided global reads (11.7 us -> a few us at 200 x 20).
constexpr int CE_LDS_FLOATS = 12288;
__global__ __launch_bounds__(LOSS_BLOCK) void softmax_ce_rows_lds_kernel(
    const float* __restrict__ logits_full, const int64_t* __restrict__ labels, int N, int C, int reduction,
    float* __restrict__ dlogits_full, float* __restrict__ loss_out, double* __restrict__ stats, int ld, int col_off) {
    __shared__ float zs[CE_LDS_FLOATS];
    __shared__ float w_loss[16];
    __shared__ int w_corr[16];
    const int lds = ld | 1;                       // odd row stride: conflict-free per-row walks
    const int total = N * ld;
    for (int e = threadIdx.x; e < total; e += LOSS_BLOCK) {
        const int r = e / ld, c = e - r * ld;
        zs[r * lds + c] = logits_full[e];
    }
    __syncthreads();
    const int row = threadIdx.x;
    const float scale = reduction == 0 ? 1.f / (float)N : 1.f;
    float li = 0.f;
    int ok = 0;
    if (row < N) {
        float* z = zs + row * lds + col_off;
        const int y = (int)labels[row];
        float m = -INFINITY;
        int am = 0;
        for (int c = 0; c < C; ++c) {
            float v = z[c];
            if (v > m) { m = v; am = c; }
        }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(z[c] - m);
        const float lse = logf(se);
        li = -(z[y] - m - lse);
        ok = (am == y);
        float* zr = zs + row * lds;
        for (int c = 0; c < ld; ++c) {
            const int cc = c - col_off;
            zr[c] = (cc >= 0 && cc < C) ? (expf(zr[c] - m - lse) - (cc == y ? 1.f : 0.f)) * scale : 0.f;
        }
    }
    float v = li;
    int cc = ok;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); cc += __shfl_xor(cc, o, 64); }
    if ((threadIdx.x & 63) == 0) { w_loss[threadIdx.x >> 6] = v; w_corr[threadIdx.x >> 6] = cc; }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += LOSS_BLOCK) {
        const int r = e / ld, c = e - r * ld;
        dlogits_full[e] = zs[r * lds + c];
    }
    if (threadIdx.x == 0) {
        float t = 0.f; int c = 0;
        for (int w = 0; w < 16; ++w) { t += w_loss[w]; c += w_corr[w]; }
        t *= scale;
        loss_out[0] = t;
        if (stats) { stats[0] += (double)t; stats[1] += (double)c; }
    }
}

__global__ __launch_bounds__(LOSS_BLOCK) void mse_zero_sum_kernel(const float* __restrict__ z, size_t n,
                                                                  float* __restrict__ dz, float* __restrict__ loss_out) {
    __shared__ float s_part[16];
    float acc = 0.f;
    for (size_t i = threadIdx.x; i < n; i += LOSS_BLOCK) {
        float v = z[i];
        acc += v * v;
        dz[i] = 2.f * v;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 16; ++i) t += s_part[i];
        loss_out[0] = t;
    }
}


// LwF objective over stacked heads (methods/LwF/main_LWF.py:47-76,184-202): logits [N][ld] hold H heads side by side
// (head h = columns off[h] .. off[h] + size[h]); the LAST head is the new task (CrossEntropy, mean), every earlier head
// h is distilled towards teacher [N][ld_t] (same column layout, the old heads only):
//   L_h = 1/N sum_rows [ log sum_j exp((y_j - max y)/T) - sum_j p_j (y_j - max y)/T ],
//   p = softmax(t - max t)^(1/T) / sum(...)                                  (distillation_loss, :47-76)
//   total = task + lambda * sum_h L_h ;  d total / d y_j = lambda / (N T) (softmax((y - max)/T)_j - p_j) on old heads.
// One thread per row (N <= 1024); rows are summed in a fixed order.  loss_out[0] = task loss (what the reference logs),
// loss_out[1] = lambda * sum_h L_h; stats += (task loss, #correct on the new head).
constexpr int LWF_MAX_HEADS = 32;
struct LwfHeads { int n; int off[LWF_MAX_HEADS]; int size[LWF_MAX_HEADS]; };

__global__ __launch_bounds__(LOSS_BLOCK) void lwf_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ teacher, LwfHeads hd, int N, int ld, int ld_t,
                                                              float T, float lam, int distill, float* __restrict__ dlogits,
                                                              float* __restrict__ loss_out, double* __restrict__ stats) {
    __shared__ float s_task[LOSS_BLOCK], s_dist[LOSS_BLOCK];
    __shared__ unsigned char s_corr[LOSS_BLOCK];
    const int row = threadIdx.x;
    float task = 0.f, dist = 0.f;
    int ok = 0;
    if (row < N) {
        const float* z = logits + (size_t)row * ld;
        float* dz = dlogits + (size_t)row * ld;
        const float invN = 1.f / (float)N;
        for (int h = 0; h < hd.n; ++h) {
            const int o = hd.off[h], C = hd.size[h];
            float m = -INFINITY; int am = 0;
            for (int c = 0; c < C; ++c) { const float v = z[o + c]; if (v > m) { m = v; am = c; } }
            if (h == hd.n - 1) {
                const int y = (int)labels[row];
                float se = 0.f;
                for (int c = 0; c < C; ++c) se += expf(z[o + c] - m);
                const float lse = logf(se);
                for (int c = 0; c < C; ++c) dz[o + c] = (expf(z[o + c] - m - lse) - (c == y ? 1.f : 0.f)) * invN;
                task = -(z[o + y] - m - lse);
                ok = (am == y);
            } else if (distill) {
                const float* t = teacher + (size_t)row * ld_t + o;
                float mt = -INFINITY;
                for (int c = 0; c < C; ++c) mt = fmaxf(mt, t[c]);
                float st = 0.f;
                for (int c = 0; c < C; ++c) st += expf(t[c] - mt);
                const float invT = 1.f / T;
                float sp = 0.f;                                   // sum_j softmax(t)_j^(1/T)
                for (int c = 0; c < C; ++c) sp += powf(expf(t[c] - mt) / st, invT);
                float sumex = 0.f;
                for (int c = 0; c < C; ++c) sumex += expf((z[o + c] - m) * invT);
                float cross = 0.f;
                const float g = lam * invN * invT;
                for (int c = 0; c < C; ++c) {
                    const float p = powf(expf(t[c] - mt) / st, invT) / sp;
                    const float ys = (z[o + c] - m) * invT;
                    cross += p * ys;
                    dz[o + c] = g * (expf(ys) / sumex - p);
                }
                dist += logf(sumex) - cross;
            } else {
                for (int c = 0; c < C; ++c) dz[o + c] = 0.f;
            }
        }
        // columns past the last head (ld > sum of the heads) carry no loss: zero, as the slice and segment kernels do
        for (int c = hd.off[hd.n - 1] + hd.size[hd.n - 1]; c < ld; ++c) dz[c] = 0.f;
    }
    s_task[row] = task; s_dist[row] = dist; s_corr[row] = (unsigned char)ok;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f, d = 0.f; int c = 0;
        for (int i = 0; i < N; ++i) { t += s_task[i]; d += s_dist[i]; c += s_corr[i]; }       // fixed order
        t /= (float)N; d = lam * d / (float)N;
        loss_out[0] = t; loss_out[1] = d;
        if (stats) { stats[0] += (double)t; stats[1] += (double)c; }
    }
}

// The segmented loss of the exemplar methods (clhip_loss_segments).  Phase 1: one wave per row (rows strided over the 16
// waves) computes the row's value over its class slice; a cross-entropy row also writes its gradient row (a slice of <= 64
// classes is loaded once and kept in registers), a distillation row keeps its softmax statistics in LDS; phase 2: one wave
// per segment sums its rows in f64 (fixed lane assignment + butterfly) and decides the segment's gate (a distillation
// segment whose own value is negative counts as the integer 0 of icarl.py:584-587: no loss, no gradient); phase 3: the
// gradient rows of the distillation segments and zeros for rows of no segment; thread 0 sums the segments in order => the
// loss does not depend on scheduling.
__global__ __launch_bounds__(LOSS_BLOCK) void loss_segments_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ targets, int ld_t, int N, int ld,
    const clhip_loss_segment* __restrict__ segs, int n_segs, float T, float* __restrict__ dlogits, float* __restrict__ loss_out,
    double* __restrict__ stats) {
    __shared__ clhip_loss_segment s_seg[CLHIP_LOSS_MAX_SEGS];
    __shared__ int s_valid[CLHIP_LOSS_MAX_SEGS];
    __shared__ float s_gate[CLHIP_LOSS_MAX_SEGS];
    __shared__ double s_part[CLHIP_LOSS_MAX_SEGS];
    __shared__ float s_val[CLHIP_LOSS_MAX_ROWS];
    __shared__ float s_zm[CLHIP_LOSS_MAX_ROWS], s_zl[CLHIP_LOSS_MAX_ROWS], s_tm[CLHIP_LOSS_MAX_ROWS], s_tl[CLHIP_LOSS_MAX_ROWS];
    __shared__ short s_rowseg[CLHIP_LOSS_MAX_ROWS];
    __shared__ unsigned char s_hit[CLHIP_LOSS_MAX_ROWS];
    __shared__ int s_bad, s_hits;
    if (threadIdx.x == 0) { s_bad = 0; s_hits = 0; }
    for (int g = threadIdx.x; g < n_segs; g += LOSS_BLOCK) {
        const clhip_loss_segment sg = segs[g];
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
        if (s_seg[g].kind == 0) {                      // never gated: the gradient row is written here, from the same loads
            const int y = (int)labels[row];
            const bool ok = y >= 0 && y < C;
            const float w = s_seg[g].scale / (float)(s_seg[g].row_end - s_seg[g].row_begin);
            float* dz = dlogits + (size_t)row * ld;
            float gm, lse, zy;
            int am;
            if (C <= 64) {                             // the task heads: ONE load of the slice, everything from registers
                const float zv = lane < C ? z[lane] : -INFINITY;
                gm = wave_max(zv);
                am = wave_min((lane < C && zv == gm) ? lane : 0x7fffffff);      // torch.max tie rule: lowest index
                lse = logf(wave_sum(lane < C ? expf(zv - gm) : 0.f));
                zy = __shfl(zv, ok ? y : 0, 64);
                for (int c0 = 0; c0 < ld; c0 += 64) {   // wave-uniform trip count: every lane takes part in the shuffle
                    const int c = c0 + lane, cc = c - o;
                    const float zc = __shfl(zv, (cc >= 0 && cc < 64) ? cc : 0, 64);
                    if (c < ld) dz[c] = (cc >= 0 && cc < C) ? (expf(zc - gm - lse) - (cc == y ? 1.f : 0.f)) * w : 0.f;
                }
            } else {
                float m = -INFINITY, se = 0.f;
                am = 0x7fffffff;
                for (int c = lane; c < C; c += 64) {
                    const float v = z[c];
                    if (v > m) { m = v; am = c; }
                }
                gm = wave_max(m);
                am = wave_min(m == gm ? am : 0x7fffffff);
                for (int c = lane; c < C; c += 64) se += expf(z[c] - gm);
                lse = logf(wave_sum(se));
                for (int c = lane; c < ld; c += 64) {
                    const int cc = c - o;
                    dz[c] = (cc >= 0 && cc < C) ? (expf(z[cc] - gm - lse) - (cc == y ? 1.f : 0.f)) * w : 0.f;
                }
                zy = ok ? z[y] : 0.f;
            }
            if (lane == 0) {
                if (!ok) s_bad = 1;
                s_val[row] = ok ? -(zy - gm - lse) : 0.f;
                s_hit[row] = (unsigned char)(g == 0 && am == y);
            }
        } else {
            const float* tr = targets + (size_t)row * ld_t + o;
            float zm = -INFINITY, tm = -INFINITY;
            for (int c = lane; c < C; c += 64) { zm = fmaxf(zm, z[c] * invT); tm = fmaxf(tm, tr[c] * invT); }
            zm = wave_max(zm); tm = wave_max(tm);
            float zs = 0.f, ts = 0.f;
            for (int c = lane; c < C; c += 64) { zs += expf(z[c] * invT - zm); ts += expf(tr[c] * invT - tm); }
            const float zl = logf(wave_sum(zs)), tl = logf(wave_sum(ts));
            float kl = 0.f;                                       // sum_c p (log p - log q), p = softmax(target / T), q = softmax(z / T)
            for (int c = lane; c < C; c += 64) {
                const float lp = tr[c] * invT - tm - tl, lq = z[c] * invT - zm - zl;
                const float p = expf(lp);
                kl += p > 0.f ? p * (lp - lq) : 0.f;
            }
            kl = wave_sum(kl);
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
        if (s_seg[g].kind == 0) continue;              // written in phase 1
        const int o = s_seg[g].col_off, C = s_seg[g].ncols;
        const float wT = s_seg[g].scale / (float)(s_seg[g].row_end - s_seg[g].row_begin) * T;      // d/dz of T^2 KL = T (q - p)
        const float* zr = logits + (size_t)row * ld;
        const float* tr = targets + (size_t)row * ld_t;
        const float zm = s_zm[row], zl = s_zl[row], tm = s_tm[row], tl = s_tl[row];
        for (int c = lane; c < ld; c += 64) {
            const int cc = c - o;
            dz[c] = (cc >= 0 && cc < C) ? (expf(zr[c] * invT - zm - zl) - expf(tr[c] * invT - tm - tl)) * wT : 0.f;
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

}  // namespace

extern "C" {

int clhip_softmax_ce_slice(const float* logits, const int64_t* labels_i64, int N, int ld, int col_off, int ncols,
                           int reduction, float* dlogits, float* loss_out, double* stats, void* stream) {
    if (!logits || !labels_i64 || !dlogits || !loss_out || N <= 0 || ncols <= 0 || col_off < 0 || col_off + ncols > ld)
        return CLHIP_EINVAL;
    if (reduction != 0 && reduction != 1) return CLHIP_EINVAL;
    if (ncols <= 64 && N <= LOSS_BLOCK && (size_t)N * (ld | 1) <= (size_t)CE_LDS_FLOATS)
        hipLaunchKernelGGL(softmax_ce_rows_lds_kernel, dim3(1), dim3(LOSS_BLOCK), 0, as_stream(stream), logits, labels_i64, N, ncols,
                           reduction, dlogits, loss_out, stats, ld, col_off);
    else if (ncols <= 64 && N <= LOSS_BLOCK && ld <= 4096)
        hipLaunchKernelGGL(softmax_ce_rows_kernel, dim3(1), dim3(LOSS_BLOCK), 0, as_stream(stream), logits, labels_i64, N, ncols,
                           reduction, dlogits, loss_out, stats, ld, col_off);
    else
        hipLaunchKernelGGL(softmax_ce_kernel<16>, dim3(1), dim3(LOSS_BLOCK), 0, as_stream(stream), logits, labels_i64, N, ncols,
                           reduction, dlogits, loss_out, stats, ld, col_off);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_softmax_ce(const float* logits, const int64_t* labels_i64, int N, int C, int reduction,
                     float* dlogits, float* loss_out, double* stats, void* stream) {
    return clhip_softmax_ce_slice(logits, labels_i64, N, C, 0, C, reduction, dlogits, loss_out, stats, stream);
}

int clhip_lwf_loss(const float* logits, const int64_t* labels_i64, const float* teacher, const int* head_sizes, int n_heads,
                   int N, int ld, int ld_teacher, float T, float reg_lambda, int distill, float* dlogits, float* loss_out2,
                   double* stats, void* stream) {
    if (!logits || !labels_i64 || !head_sizes || !dlogits || !loss_out2 || n_heads < 1 || n_heads > LWF_MAX_HEADS) return CLHIP_EINVAL;
    if (N <= 0 || N > LOSS_BLOCK || (distill && n_heads > 1 && !teacher) || T <= 0.f) return CLHIP_EINVAL;
    LwfHeads hd; hd.n = n_heads;
    int off = 0;
    for (int h = 0; h < n_heads; ++h) { if (head_sizes[h] <= 0) return CLHIP_EINVAL; hd.off[h] = off; hd.size[h] = head_sizes[h]; off += head_sizes[h]; }
    if (off > ld || (distill && n_heads > 1 && off - head_sizes[n_heads - 1] > ld_teacher)) return CLHIP_EINVAL;
    hipLaunchKernelGGL(lwf_loss_kernel, dim3(1), dim3(LOSS_BLOCK), 0, as_stream(stream), logits, labels_i64, teacher, hd, N, ld,
                       ld_teacher, T, reg_lambda, distill, dlogits, loss_out2, stats);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_mse_zero_sum(const float* logits, size_t n, float* dlogits, float* loss_out, void* stream) {
    if (!logits || !dlogits || !loss_out || n == 0) return CLHIP_EINVAL;
    hipLaunchKernelGGL(mse_zero_sum_kernel, dim3(1), dim3(LOSS_BLOCK), 0, as_stream(stream), logits, n, dlogits, loss_out);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_loss_segments(const float* logits, const int64_t* labels_i64, const float* targets, int ld_t, int N, int ld,
                        const clhip_loss_segment* segs, int n_segs, float T, float* dlogits, float* loss_out, double* stats,
                        void* stream) {
    if (!logits || !labels_i64 || !segs || !dlogits || !loss_out) return CLHIP_EINVAL;
    if (N <= 0 || N > CLHIP_LOSS_MAX_ROWS || ld <= 0 || n_segs < 1 || n_segs > CLHIP_LOSS_MAX_SEGS || !(T > 0.f)) return CLHIP_EINVAL;
    if (targets && ld_t <= 0) return CLHIP_EINVAL;
    hipLaunchKernelGGL(loss_segments_kernel, dim3(1), dim3(LOSS_BLOCK), 0, as_stream(stream), logits, labels_i64, targets, ld_t, N, ld,
                       segs, n_segs, T, dlogits, loss_out, stats);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
