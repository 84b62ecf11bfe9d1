// weight_images.hpp — the prepared-weights job table of a pass and the body of one of its blocks: the Winograd U images (wino.hip) and
// the bf16-split images (bs_weight.hpp) of every layer, forward and backward-data sets.  Shared by wino.hip (wino_weight_multi_kernel,
// the launch of its own) and conv3x3.hip (c3w64_relu_pool_wt_kernel: the same blocks at one end of the first layer's forward grid), so
// that both run the same device code per job and the images hold the same bits.
#pragma once
#include "common.hpp"
#include "bs_weight.hpp"

namespace {

constexpr int WKT = 64;      // out channels per block
constexpr int WCK = 8;       // in channels per chunk
constexpr int WFP = 20;      // floats per (channel, out-channel) in the U tile: 16 frequencies + 4 pad — an 80-byte stride makes
                             // the 16-byte reads of 16 consecutive lanes land on 64 distinct LDS banks
constexpr int W_FLOATS = WCK * WKT * WFP;         // 10240 floats = 40 KB: U tile of one chunk [c][k][f]
// The lane-ordered image, behind the LDS images of the whole layer (wino_conv16g_kernel and wino_conv16_kernel load their A operands
// from it straight into registers): per (k-tile, 4-channel chunk) 16 pieces of 1 KB,
//   [out-channel half wk][row tile r][frequency quad fq][lane = 16 * (channel of the quad) + (out channel & 15)][4 frequencies]
// = what ONE buffer_load_dwordx4 of a wave of wino_conv16g_kernel wants as its A operands of 4 MFMAs: contiguous, whole lines.
constexpr int WD_FLOATS = 4 * WKT * 16;           // 4096 floats = 16 KB per (k-tile, 4-channel chunk)
constexpr int WU_FLOATS = W_FLOATS + 2 * WD_FLOATS;   // both images of an 8-channel chunk

// the four float4 of one (channel, out-channel) pair -> the LDS image and the lane-ordered image behind it
__device__ __forceinline__ void wino_u_store(float* __restrict__ U, int kts, int n_chunks, int kt, int chunk, int c_l, int k_l,
                                             const float4 (&u)[4]) {
    float4* dst = reinterpret_cast<float4*>(U + (((size_t)(kt * n_chunks + chunk) * WCK + c_l) * WKT + k_l) * WFP);
#pragma unroll
    for (int a = 0; a < 4; ++a) dst[a] = u[a];
    dst[4] = make_float4(0.f, 0.f, 0.f, 0.f);
    float* Ud = U + (size_t)kts * n_chunks * W_FLOATS;
    const int chunk4 = 2 * chunk + (c_l >> 2), q = c_l & 3, wk = k_l >> 5, r = (k_l >> 4) & 1, ti = k_l & 15;
    float4* dd = reinterpret_cast<float4*>(Ud + ((((size_t)(kt * 2 * n_chunks + chunk4) * 2 + wk) * 2 + r) * 4) * 256 + (q * 16 + ti) * 4);
#pragma unroll
    for (int a = 0; a < 4; ++a) dd[a * 64] = u[a];
}

// Several (layer, mode) pairs in ONE launch: the plan executor transforms the weights of every Winograd layer of a pass at its start
// (six ~5 us launches per pass of small_VGG9 were 3 % of the step).
constexpr int WT_JOBS = 24;
struct WtJobs { int n; int pad; clhip_wino_wt j[WT_JOBS]; int first[WT_JOBS + 1]; };      // pad: bit i = job i is a bf16-split image (bs_weight.hpp)

__device__ __forceinline__ void wino_weight_one(const float* __restrict__ w, float* __restrict__ U, int Ko, int Ci, int mode,
                                                int n_chunks, int i) {
    const int k_l = i % WKT, c_l = (i / WKT) % WCK, chunk = (i / (WKT * WCK)) % n_chunks, kt = i / (WKT * WCK * n_chunks);
    const int k = kt * WKT + k_l, c = chunk * WCK + c_l;
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            float v = 0.f;
            if (k < Ko && c < Ci)
                v = mode == 0 ? w[((size_t)k * Ci + c) * 9 + r * 3 + s] : w[((size_t)c * Ko + k) * 9 + (2 - r) * 3 + (2 - s)];
            g[r][s] = v;
        }
    float t[4][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        t[0][s] = g[0][s];
        t[1][s] = 0.5f * (g[0][s] + g[1][s] + g[2][s]);
        t[2][s] = 0.5f * (g[0][s] - g[1][s] + g[2][s]);
        t[3][s] = g[2][s];
    }
    float4 u[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
        u[a] = make_float4(t[a][0], 0.5f * (t[a][0] + t[a][1] + t[a][2]), 0.5f * (t[a][0] - t[a][1] + t[a][2]), t[a][2]);
    wino_u_store(U, (Ko + WKT - 1) / WKT, n_chunks, kt, chunk, c_l, k_l, u);
}

// the work of block `vb` (256 threads, thread `tid`) of the table — the body of wino_weight_multi_kernel.  No LDS, no barrier: a
// caller may run it on any 256 consecutive threads of a larger block.
__device__ __forceinline__ void weight_image_block(const WtJobs& J, int vb, int tid) {
    int jb = 0;
    for (int i = 1; i < J.n; ++i) jb = (vb >= J.first[i]) ? i : jb;
    const clhip_wino_wt& q = J.j[jb];
    if ((J.pad >> jb) & 1) {                 // (uniform per block) a bf16-split image of the same pass
        bs_weight_block(q, vb - J.first[jb], tid);
        return;
    }
    const int n_chunks = (q.Ci + WCK - 1) / WCK;
    const int total = ((q.Ko + WKT - 1) / WKT) * n_chunks * WCK * WKT;
    const int i = (vb - J.first[jb]) * 256 + tid;
    if (i < total) wino_weight_one(q.w, q.U, q.Ko, q.Ci, q.mode, n_chunks, i);
}

// Job table of the Winograd jobs wj[0 .. nw) followed by the bf16-split jobs bj[0 .. nb) (host arrays; either kind may be absent).
// Returns the number of 256-thread blocks, or CLHIP_EINVAL (negative); nw + nb must fit WT_JOBS.
static inline int weight_jobs_table(const clhip_wino_wt* wj, int nw, const clhip_wino_wt* bj, int nb, WtJobs& J) {
    if (nw < 0 || nb < 0 || nw + nb <= 0 || nw + nb > WT_JOBS || (nw && !wj) || (nb && !bj)) return CLHIP_EINVAL;
    J.n = nw + nb;
    J.pad = 0;
    int blocks = 0;
    for (int i = 0; i < J.n; ++i) {
        const bool is_bs = i >= nw;
        const clhip_wino_wt& q = is_bs ? bj[i - nw] : wj[i];
        if (!q.w || !q.U || q.Ko <= 0 || q.Ci <= 0) return CLHIP_EINVAL;
        J.j[i] = q;
        J.first[i] = blocks;
        if (is_bs) {
            J.pad |= 1 << i;
            blocks += bs_weight_blocks(q);
        } else {
            const int total = ((q.Ko + WKT - 1) / WKT) * ((q.Ci + WCK - 1) / WCK) * WCK * WKT;
            blocks += (total + 255) / 256;
        }
    }
    J.first[J.n] = blocks;
    return blocks;
}

}  // namespace
