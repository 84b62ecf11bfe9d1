// wgrad_reduce.hpp — the fixed-order reduction of weight-gradient split-K slabs as a block-level device function, for the
// reduction launches of conv3x3_wgrad.hip and for the rider blocks of the bf16-split backward-data launch (bsconv.hip,
// bs_conv_riders_kernel): both run the same code per 64-element unit, so dw / db do not depend on which launch reduced them.
#pragma once
#include "common.hpp"

// Fixed-order reduction of the partial slabs in ONE launch (the two tiny launches it replaces were launch-latency
// bound: 12 us per layer and pass).  Block = 64 consecutive elements x 16 split-lanes: lane j sums its contiguous
// range of splits in order (f64), the 16 partials meet in LDS and are added in order j = 0..15 — the same two-level
// association for every run, every grid size: bitwise run-to-run deterministic.
//   dw[k][c][rs] = sum_s part[s][rs][k][c] ; db[k] = sum_s part[s][9KC + k]
constexpr int RED_EL = 64, RED_J = 16, RED_V = 4;          // 64 elements x 16 split-lanes per block, 4 elements per thread
constexpr int RED_THREADS = RED_EL / RED_V * RED_J;
// (Measured and removed in round 5: 256 elements x 4 split-lanes — 1 KB of ONE slab per wave and load instruction — ran 39.1 us
// against 22.7 us for the slabs of a small_VGG9 pass, profiles/r05_wgred_wide.txt: fewer splits in flight per element.)

// One block: elements [e0, e0 + 64) of the (9KC + K)-element slab.  Thread (j, v) sums splits [j q, (j + 1) q) of the 4
// consecutive elements v (16-byte loads when every slab row is 16-byte aligned: total % 4 == 0 and `part` itself), then lane j = 0 adds the 16 partial
// sums in order: the order per element does not depend on the vector width.
template <int EL, int J>
__device__ __forceinline__ void wgrad_reduce_block(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                   int K, int C, int splits, size_t e0, double (*partial)[EL], int T = 9) {
    const size_t kc = (size_t)K * C, nw = (size_t)T * kc, total = nw + K;      // T taps per (k, c): 9, or 25 for the 5x5 slabs of bswgrad5.hip
    const int v = threadIdx.x % (EL / RED_V), j = threadIdx.x / (EL / RED_V);
    const size_t e = e0 + (size_t)v * RED_V;
    const int q = (splits + J - 1) / J;
    const int s0 = j * q, s1 = min(splits, s0 + q);
    double s[RED_V] = {0.0, 0.0, 0.0, 0.0};
    if ((total & 3) == 0 && (reinterpret_cast<uintptr_t>(part) & 15u) == 0 && e + RED_V <= total) {
        // (four slabs in flight per thread; eight were measured SLOWER — 36.7 us against 24.5 for the slabs of a small_VGG9 pass)
#pragma unroll 4
        for (int sp = s0; sp < s1; ++sp) {
            const float4 t = *reinterpret_cast<const float4*>(part + (size_t)sp * total + e);
            s[0] += (double)t.x; s[1] += (double)t.y; s[2] += (double)t.z; s[3] += (double)t.w;
        }
    } else {
        for (int sp = s0; sp < s1; ++sp)
#pragma unroll
            for (int t = 0; t < RED_V; ++t)
                if (e + t < total) s[t] += (double)part[(size_t)sp * total + e + t];
    }
#pragma unroll
    for (int t = 0; t < RED_V; ++t) partial[j][v * RED_V + t] = s[t];
    __syncthreads();
    if (threadIdx.x < EL) {
        const int el = threadIdx.x;
        const size_t ee = e0 + el;
        if (ee < total) {
            double t = 0.0;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) t += partial[jj][el];
            if (ee < nw) {
                const size_t rs = ee / kc, rem = ee - rs * kc;     // rem = k*C + c
                dw[rem * T + rs] = (float)t;
            } else if (db) {
                db[ee - nw] = (float)t;
            }
        }
    }
}

// The slabs of SEVERAL layers as one list of 64-element units (the plan executor defers them to the end of the backward pass, or
// hands them to the rider blocks of a backward-data launch).  Per job the arithmetic and its order are those of wgrad_reduce_block.
struct RedJobs {
    clhip_wgrad_job job[CLHIP_WGRAD_JOBS_MAX];
    unsigned first[CLHIP_WGRAD_JOBS_MAX + 1];       // prefix sums of blocks
    int n;
};

// unit u of the list: the job it belongs to (from first[]) and wgrad_reduce_block on its 64 elements
template <int EL, int JL>
__device__ __forceinline__ void wgrad_reduce_unit(const RedJobs& jobs, unsigned u, double (*partial)[EL]) {
    int ji = 0;
    while (ji + 1 < jobs.n && u >= jobs.first[ji + 1]) ++ji;
    const clhip_wgrad_job J = jobs.job[ji];
    wgrad_reduce_block<EL, JL>(J.part, J.dw, J.db, J.K, J.C, J.splits, (size_t)(u - jobs.first[ji]) * EL, partial, J.taps ? J.taps : 9);
}

// host side: the table of n jobs (1 .. CLHIP_WGRAD_JOBS_MAX, checked by the caller); unused entries are empty and own no unit
inline void wgrad_reduce_fill(RedJobs& r, const clhip_wgrad_job* jobs, int n) {
    r.n = n;
    r.first[0] = 0;
    for (int i = 0; i < n; ++i) {
        r.job[i] = jobs[i];
        const size_t total = (size_t)(jobs[i].taps ? jobs[i].taps : 9) * jobs[i].K * jobs[i].C + jobs[i].K;
        r.first[i + 1] = r.first[i] + (unsigned)((total + RED_EL - 1) / RED_EL);
    }
    for (int i = n; i < CLHIP_WGRAD_JOBS_MAX; ++i) { r.job[i] = clhip_wgrad_job{nullptr, nullptr, nullptr, 0, 0, 0, 0}; r.first[i + 1] = r.first[n]; }
}
