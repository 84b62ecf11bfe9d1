// Rehearsal baselines (rehearsal/model/baseline_rehearsal_partial_mem.py:125-253): the step's batch assembly and the
// segmented cross-entropy that let one engine pass over [current batch | exemplar chunks] replace the reference's one
// forward / backward per exemplar chunk plus one for the current batch.
#include "common.hpp"

namespace {

constexpr int ASM_BLOCK = 256;
constexpr int ASM_VEC_PER_THREAD = 12;    // float4 per thread, all in flight at once: 48 KB per block = one 3x64x64 row
constexpr int CE_BLOCK = 1024;            // 16 waves, one block: fixed reduction order
constexpr int CE_MAX_ROWS = 1024;

// One block row per destination row (blockIdx.y), blockIdx.x walks the row in 48 KB segments.
//   rows [0, B)            x[r]                 -> x_mix[r],          y[r]        -> y_mix[r]
//   rows [B, B + eff)      x[i]                 -> store_x[row0 + i], y[i]        -> store_y[row0 + i]   (ring buffer)
//   rows [B + eff, ...)    store_x[gather[e]]   -> x_mix[B + e],      store_y[..] -> y_mix[B + e]
// A gather index outside [0, store_rows) copies nothing and writes label -1 (the caller's plan never produces one).
template <bool VEC>
__global__ __launch_bounds__(ASM_BLOCK) void rehearsal_assemble_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ y, int B, size_t row_elems, float* store_x, int64_t* store_y,
    long store_rows, long row0, int eff, const int* __restrict__ gather, int E, float* __restrict__ x_mix,
    int64_t* __restrict__ y_mix) {
    const int r = blockIdx.y;
    const float* src;
    float* dst;
    const int64_t* ysrc;
    int64_t* ydst;
    if (r < B) {
        src = x + (size_t)r * row_elems; dst = x_mix + (size_t)r * row_elems;
        ysrc = y + r; ydst = y_mix + r;
    } else if (r < B + eff) {
        const int i = r - B;
        src = x + (size_t)i * row_elems; dst = store_x + (size_t)(row0 + i) * row_elems;
        ysrc = y + i; ydst = store_y + row0 + i;
    } else {
        const int e = r - B - eff;
        const long g = gather[e];
        dst = x_mix + (size_t)(B + e) * row_elems;
        ydst = y_mix + B + e;
        if (g < 0 || g >= store_rows) {
            if (blockIdx.x == 0 && threadIdx.x == 0) *ydst = -1;
            return;
        }
        src = store_x + (size_t)g * row_elems;
        ysrc = store_y + g;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *ydst = *ysrc;
    if (VEC) {
        const size_t nvec = row_elems / 4;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        const size_t base = (size_t)blockIdx.x * ASM_BLOCK * ASM_VEC_PER_THREAD + threadIdx.x;
        float4 v[ASM_VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < ASM_VEC_PER_THREAD; ++k) {          // all loads in flight before the first store
            const size_t i = base + (size_t)k * ASM_BLOCK;
            if (i < nvec) v[k] = s4[i];
        }
#pragma unroll
        for (int k = 0; k < ASM_VEC_PER_THREAD; ++k) {
            const size_t i = base + (size_t)k * ASM_BLOCK;
            if (i < nvec) d4[i] = v[k];
        }
    } else {
        const size_t seg = (size_t)ASM_BLOCK * ASM_VEC_PER_THREAD * 4;
        const size_t end = min(row_elems, ((size_t)blockIdx.x + 1) * seg);
        for (size_t i = (size_t)blockIdx.x * seg + threadIdx.x; i < end; i += ASM_BLOCK) dst[i] = src[i];
    }
}

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// One wave per row (rows strided over the 16 waves): lanes walk the row's class slice (coalesced, any width), the whole
// [ld] dlogits row is written (0 outside the slice); a slice of <= 64 classes is loaded once and kept in registers.
// Per-row CE and hit go to LDS; then one wave per segment sums its rows (fixed lane assignment + butterfly) and thread 0
// sums the segments in order => the loss does not depend on scheduling.
__global__ __launch_bounds__(CE_BLOCK) void softmax_ce_segments_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels, int N, int ld, const clhip_ce_segment* __restrict__ segs,
    int n_segs, float* __restrict__ dlogits, float* __restrict__ loss_out, double* __restrict__ stats) {
    __shared__ clhip_ce_segment s_seg[CLHIP_CE_MAX_SEGS];
    __shared__ int s_valid[CLHIP_CE_MAX_SEGS];
    __shared__ float s_ce[CE_MAX_ROWS];
    __shared__ unsigned char s_hit[CE_MAX_ROWS];
    __shared__ double s_part[CLHIP_CE_MAX_SEGS];
    __shared__ int s_bad, s_hits;
    if (threadIdx.x == 0) { s_bad = 0; s_hits = 0; }
    for (int g = threadIdx.x; g < n_segs; g += CE_BLOCK) {
        const clhip_ce_segment sg = segs[g];
        s_seg[g] = sg;
        s_valid[g] = sg.row_begin >= 0 && sg.row_begin < sg.row_end && sg.row_end <= N && sg.col_off >= 0 && sg.ncols > 0 &&
                     sg.col_off + sg.ncols <= ld;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = wave; row < N; row += CE_BLOCK / 64) {
        int g = -1;                                    // first valid segment that holds the row (wave-uniform scan)
        for (int k = 0; k < n_segs; ++k)
            if (s_valid[k] && row >= s_seg[k].row_begin && row < s_seg[k].row_end) { g = k; break; }
        float* dz = dlogits + (size_t)row * ld;
        if (g < 0) {                                   // row outside every segment: no loss, no gradient
            for (int c = lane; c < ld; c += 64) dz[c] = 0.f;
            if (lane == 0) { s_ce[row] = 0.f; s_hit[row] = 0; }
            continue;
        }
        const int o = s_seg[g].col_off, C = s_seg[g].ncols;
        const float w = s_seg[g].scale / (float)(s_seg[g].row_end - s_seg[g].row_begin);
        const float* z = logits + (size_t)row * ld + o;
        const int y = (int)labels[row];
        const bool ok = y >= 0 && y < C;
        float m = -INFINITY, se = 0.f, lse, zy;
        int am = 0x7fffffff;
        if (C <= 64) {                                 // the task heads: ONE load of the slice, everything from registers
            const float zv = lane < C ? z[lane] : -INFINITY;
            m = zv;
            am = lane < C ? lane : 0x7fffffff;
            const float gm = wave_max_f(m);
            const int cand = wave_min_i(m == gm ? am : 0x7fffffff);     // torch.max tie rule: lowest index
            lse = logf(wave_sum_f(lane < C ? expf(zv - gm) : 0.f));
            zy = __shfl(zv, ok ? y : 0, 64);
            for (int c0 = 0; c0 < ld; c0 += 64) {       // wave-uniform trip count: every lane takes part in the shuffle
                const int c = c0 + lane, cc = c - o;
                const float zc = __shfl(zv, (cc >= 0 && cc < 64) ? cc : 0, 64);
                if (c < ld) dz[c] = (cc >= 0 && cc < C) ? (expf(zc - gm - lse) - (cc == y ? 1.f : 0.f)) * w : 0.f;
            }
            m = gm;
            am = cand;
        } else {
            for (int c = lane; c < C; c += 64) {
                const float v = z[c];
                if (v > m) { m = v; am = c; }
            }
            const float gm = wave_max_f(m);
            am = wave_min_i(m == gm ? am : 0x7fffffff);
            for (int c = lane; c < C; c += 64) se += expf(z[c] - gm);
            lse = logf(wave_sum_f(se));
            for (int c = lane; c < ld; c += 64) {
                const int cc = c - o;
                dz[c] = (cc >= 0 && cc < C) ? (expf(z[cc] - gm - lse) - (cc == y ? 1.f : 0.f)) * w : 0.f;
            }
            zy = ok ? z[y] : 0.f;
            m = gm;
        }
        if (lane == 0) {
            if (!ok) s_bad = 1;
            s_ce[row] = ok ? -(zy - m - lse) : 0.f;
            s_hit[row] = (unsigned char)(g == 0 && am == y);
        }
    }
    __syncthreads();
    // one wave per segment: lanes take rows r0 + lane, r0 + lane + 64, ... in f64, then a butterfly — a fixed order
    for (int g = wave; g < n_segs; g += CE_BLOCK / 64) {
        double t = 0.0;                                // f64 sums: the loss of a 1024-row step to ~1 ulp of f32
        int h = 0;
        if (s_valid[g]) {
            for (int r = s_seg[g].row_begin + lane; r < s_seg[g].row_end; r += 64) { t += (double)s_ce[r]; h += s_hit[r]; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { t += __shfl_xor(t, off, 64); h += __shfl_xor(h, off, 64); }
        if (lane == 0) {
            s_part[g] = s_valid[g] ? (double)s_seg[g].scale * (t / (double)(s_seg[g].row_end - s_seg[g].row_begin)) : 0.0;
            if (g == 0) s_hits = h;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double td = 0.0;
        for (int g = 0; g < n_segs; ++g) td += s_part[g];
        float t = (float)td;
        const int hits = s_hits;
        bool bad = s_bad != 0;
        for (int g = 0; g < n_segs; ++g) bad = bad || !s_valid[g];
        if (bad) t = __int_as_float(0x7fc00000);      // a malformed table or label is reported as a NaN loss
        loss_out[0] = t;
        if (stats) { stats[0] += (double)t; stats[1] += (double)hits; }
    }
}

}  // namespace

extern "C" {

int clhip_rehearsal_assemble(const float* x, const int64_t* labels_i64, int B, size_t row_elems, float* store_x,
                             int64_t* store_labels, long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                             int E, float* x_mix, int64_t* labels_mix, void* stream) {
    if (B < 0 || E < 0 || ring_rows < 0 || row_elems == 0 || store_rows < 0) return CLHIP_EINVAL;
    if (ring_rows > B) return CLHIP_EINVAL;                                      // ring rows are a prefix of x
    if ((B > 0 || ring_rows > 0) && (!x || !labels_i64)) return CLHIP_EINVAL;
    if ((B > 0 || E > 0) && (!x_mix || !labels_mix)) return CLHIP_EINVAL;
    if ((ring_rows > 0 || E > 0) && (!store_x || !store_labels)) return CLHIP_EINVAL;
    if (E > 0 && !gather_rows) return CLHIP_EINVAL;
    if (ring_rows > 0 && (ring_row0 < 0 || ring_row0 + ring_rows > store_rows)) return CLHIP_EINVAL;
    const long rows = (long)B + ring_rows + E;
    if (rows == 0) return 0;
    if (rows > 65535) return CLHIP_EINVAL;
    const bool vec = row_elems % 4 == 0 && (!x || aligned16(x)) && (!x_mix || aligned16(x_mix)) && (!store_x || aligned16(store_x));
    const size_t seg = (size_t)ASM_BLOCK * ASM_VEC_PER_THREAD * 4;
    dim3 grid((unsigned)((row_elems + seg - 1) / seg), (unsigned)rows);
    if (vec)
        hipLaunchKernelGGL(rehearsal_assemble_kernel<true>, grid, dim3(ASM_BLOCK), 0, as_stream(stream), x, labels_i64, B, row_elems,
                           store_x, store_labels, store_rows, ring_row0, ring_rows, gather_rows, E, x_mix, labels_mix);
    else
        hipLaunchKernelGGL(rehearsal_assemble_kernel<false>, grid, dim3(ASM_BLOCK), 0, as_stream(stream), x, labels_i64, B, row_elems,
                           store_x, store_labels, store_rows, ring_row0, ring_rows, gather_rows, E, x_mix, labels_mix);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_softmax_ce_segments(const float* logits, const int64_t* labels_i64, int N, int ld, const clhip_ce_segment* segs,
                              int n_segs, float* dlogits, float* loss_out, double* stats, void* stream) {
    if (!logits || !labels_i64 || !segs || !dlogits || !loss_out) return CLHIP_EINVAL;
    if (N <= 0 || N > CE_MAX_ROWS || ld <= 0 || n_segs < 1 || n_segs > CLHIP_CE_MAX_SEGS) return CLHIP_EINVAL;
    hipLaunchKernelGGL(softmax_ce_segments_kernel, dim3(1), dim3(CE_BLOCK), 0, as_stream(stream), logits, labels_i64, N, ld, segs,
                       n_segs, dlogits, loss_out, stats);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
