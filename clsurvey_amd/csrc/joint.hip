// Joint baseline (methods/method.py:1185-1235): one model on all tasks at once.
//   gather_tasks        a batch out of T per-task tensors by GLOBAL sample number (data/imgfolder.py:244-272
//                       ConcatDatasetDynamicLabels.__getitem__) — no merged copy of the sequence in HBM.
//   gather_tasks_u8     the same out of BYTE rows [C][plane_elems]: element e of a row, a byte v of channel (e / plane_elems) % C,
//                       becomes lut[channel][v] (the host's ToTensor -> Normalize table, clhip.h).
//   slice_argmax_count  framework/inference.py:141-149 for one batch: arg-max inside the task's output slice against the
//                       task-local label, per-class correct / total counters.
#include "common.hpp"

namespace {

constexpr int GT_BLOCK = 256;
constexpr int GT_VEC_PER_THREAD = 4;      // float4 per thread, all in flight at once: 16 KB per block, 3 blocks per 3x64x64 row
constexpr int SA_BLOCK = 256;             // 4 waves, one logits row each

// blockIdx.y = destination row, blockIdx.x walks the row in 16 KB segments.  Everything that selects the source is
// block-uniform (scalar loads of idx / the table).  A sample number outside [0, total) copies nothing and writes label -1
// (the host checks the permutation before it is uploaded; this only keeps a bad one from faulting).
__global__ __launch_bounds__(GT_BLOCK) void gather_tasks_kernel(const clhip_task_src* __restrict__ tasks, int T, size_t row_elems,
                                                                 const int64_t* __restrict__ idx, float* __restrict__ x_out,
                                                                 int64_t* __restrict__ labels_out) {
    const int r = blockIdx.y;
    const int64_t g = idx[r];
    // first task whose cumulative count exceeds g (bisect_right): lane j of every wave looks at task j (T <= 64) and the
    // counts are monotone, so it is the number of lanes that answer "not yet" — one load latency, not a chain of T
    const int lane = threadIdx.x & 63;
    const int64_t cum = lane < T ? tasks[lane].cum_rows : INT64_MAX;
    const int t = __popcll(__ballot(cum <= g));
    if (g < 0 || t >= T) {
        if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = -1;
        return;
    }
    const int64_t local = g - (t ? tasks[t - 1].cum_rows : 0);
    const float* src = tasks[t].x + (size_t)local * row_elems;
    float* dst = x_out + (size_t)r * row_elems;
    if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = tasks[t].labels[local] + tasks[t].label_shift;
    const size_t seg = (size_t)GT_BLOCK * GT_VEC_PER_THREAD * 4;          // elements per block
    if (row_elems % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
        const size_t nvec = row_elems / 4;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        const size_t base = (size_t)blockIdx.x * GT_BLOCK * GT_VEC_PER_THREAD + threadIdx.x;
        float4 v[GT_VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < GT_VEC_PER_THREAD; ++k) {                     // all loads in flight before the first store
            const size_t i = base + (size_t)k * GT_BLOCK;
            if (i < nvec) v[k] = s4[i];
        }
#pragma unroll
        for (int k = 0; k < GT_VEC_PER_THREAD; ++k) {
            const size_t i = base + (size_t)k * GT_BLOCK;
            if (i < nvec) d4[i] = v[k];
        }
    } else {
        const size_t end = min(row_elems, ((size_t)blockIdx.x + 1) * seg);
        for (size_t i = (size_t)blockIdx.x * seg + threadIdx.x; i < end; i += GT_BLOCK) dst[i] = src[i];
    }
}

// gather_tasks_kernel for byte rows.  A 16 KB segment of the output is 4096 source bytes and may cross any number of channel
// planes (plane_elems is arbitrary), so the table is read through the cache at lut[channel * 256 + byte] (3 KB for three
// channels: it stays in L1 / L2) rather than staged per block.  A thread divides ONCE, its first element -> (channel, position
// in the plane); after that it steps by the block-uniform (qc, rem) = stride / plane_elems (qc already modulo C).
// VEC: row_elems % 4 == 0 and the destination row 16-byte aligned: one float4 store per 4 elements.  Their 4 source bytes are
// one dword load when the SOURCE ROW's address is a multiple of 4 (block-uniform test of the address: every offset is one),
// 4 byte loads otherwise (an odd-sized row starts at any byte).
struct gt_pos { size_t p; int c; };                                       // position inside the plane, channel

__device__ __forceinline__ gt_pos gt_locate(size_t e, size_t plane_elems, int C) {
    const size_t pl = e / plane_elems;
    return {e - pl * plane_elems, (int)(pl % (size_t)C)};
}

__device__ __forceinline__ void gt_step(gt_pos& at, size_t rem, int qc, size_t plane_elems, int C) {
    at.p += rem;
    at.c += qc;
    if (at.p >= plane_elems) { at.p -= plane_elems; ++at.c; }
    if (at.c >= C) at.c -= C;                                             // (c + qc + 1 <= 2 C - 1)
}

__global__ __launch_bounds__(GT_BLOCK) void gather_tasks_u8_kernel(const clhip_task_src_u8* __restrict__ tasks, int T, int C,
                                                                    size_t plane_elems, const float* __restrict__ lut,
                                                                    const int64_t* __restrict__ idx, float* __restrict__ x_out,
                                                                    int64_t* __restrict__ labels_out) {
    const int r = blockIdx.y;
    const int64_t g = idx[r];
    const int lane = threadIdx.x & 63;                                     // bisect_right by ballot, as gather_tasks_kernel
    const int64_t cum = lane < T ? tasks[lane].cum_rows : INT64_MAX;
    const int t = __popcll(__ballot(cum <= g));
    if (g < 0 || t >= T) {
        if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = -1;
        return;
    }
    const size_t row_elems = (size_t)C * plane_elems;
    const int64_t local = g - (t ? tasks[t - 1].cum_rows : 0);
    typedef const uint8_t __attribute__((address_space(1))) gbyte;
    typedef const uint32_t __attribute__((address_space(1))) gu32;
    gbyte* src = (gbyte*)(tasks[t].x + (size_t)local * row_elems);
    float* dst = x_out + (size_t)r * row_elems;
    if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = tasks[t].labels[local] + tasks[t].label_shift;
    const size_t seg = (size_t)GT_BLOCK * GT_VEC_PER_THREAD * 4;          // elements per block
    if (row_elems % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const size_t nvec = row_elems / 4;
        const size_t base = (size_t)blockIdx.x * GT_BLOCK * GT_VEC_PER_THREAD + threadIdx.x;
        const bool wide = (reinterpret_cast<uintptr_t>(src) & 3u) == 0;   // block-uniform
        uint32_t u[GT_VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < GT_VEC_PER_THREAD; ++k) {                     // all loads in flight before the first store
            const size_t i = base + (size_t)k * GT_BLOCK;
            if (i < nvec) {
                if (wide) {
                    u[k] = *(gu32*)(src + 4 * i);
                } else {
                    gbyte* s = src + 4 * i;
                    u[k] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
                }
            }
        }
        gt_pos at = gt_locate(4 * base, plane_elems, C);
        const size_t stride = (size_t)GT_BLOCK * 4;
        const size_t rem = stride % plane_elems;
        const int qc = (int)((stride / plane_elems) % (size_t)C);
        float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
        for (int k = 0; k < GT_VEC_PER_THREAD; ++k) {
            const size_t i = base + (size_t)k * GT_BLOCK;
            if (i < nvec) {
                float v[4];
                gt_pos e = at;
#pragma unroll
                for (int j = 0; j < 4; ++j) {                             // (the 4 elements may cross a plane)
                    v[j] = lut[e.c * 256 + (int)((u[k] >> (8 * j)) & 255u)];
                    gt_step(e, 1, 0, plane_elems, C);
                }
                d4[i] = make_float4(v[0], v[1], v[2], v[3]);
            }
            gt_step(at, rem, qc, plane_elems, C);
        }
    } else {
        const size_t end = min(row_elems, ((size_t)blockIdx.x + 1) * seg);
        const size_t first = (size_t)blockIdx.x * seg + threadIdx.x;
        gt_pos at = gt_locate(first, plane_elems, C);
        const size_t rem = (size_t)GT_BLOCK % plane_elems;
        const int qc = (int)(((size_t)GT_BLOCK / plane_elems) % (size_t)C);
        for (size_t i = first; i < end; i += GT_BLOCK) {
            dst[i] = lut[at.c * 256 + (int)src[i]];
            gt_step(at, rem, qc, plane_elems, C);
        }
    }
}

// torch.max over a row on the CPU: the first NaN wins, otherwise the largest value, lowest position on ties.
__device__ __forceinline__ bool sa_better(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (!na && a != b) return a > b;
    return ia < ib;
}

// One wave per row: lanes stride the K columns of the slice, butterfly over (value, position), lane 0 counts.
__global__ __launch_bounds__(SA_BLOCK) void slice_argmax_count_kernel(const float* __restrict__ logits, int N, int ld,
                                                                       const int* __restrict__ cols, int K,
                                                                       const int64_t* __restrict__ labels,
                                                                       unsigned long long* __restrict__ correct,
                                                                       unsigned long long* __restrict__ total,
                                                                       unsigned long long* __restrict__ out_of_range) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (SA_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= N) return;                            // wave-uniform
    const float* z = logits + (size_t)row * ld;
    float best = -INFINITY;
    int at = 0x7fffffff;
    bool bad_col = false;
    for (int k = lane; k < K; k += 64) {
        const int c = cols[k];
        if (c < 0 || c >= ld) { bad_col = true; continue; }               // never read outside the row
        const float v = z[c];
        if (at == 0x7fffffff || sa_better(v, k, best, at)) { best = v; at = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (oa != 0x7fffffff && (at == 0x7fffffff || sa_better(ov, oa, best, at))) { best = ov; at = oa; }
    }
    const bool any_bad_col = __any(bad_col);
    if (lane == 0) {
        const int64_t y = labels[row];
        if (y < 0 || y >= K || any_bad_col) {
            atomicAdd(out_of_range, 1ULL);
        } else {
            atomicAdd(total + y, 1ULL);
            if ((int64_t)at == y) atomicAdd(correct + y, 1ULL);
        }
    }
}

}  // namespace

extern "C" {

int clhip_gather_tasks(const clhip_task_src* tasks_dev, int T, size_t row_elems, const int64_t* idx, int B, float* x_out,
                       int64_t* labels_out, void* stream) {
    if (!tasks_dev || T < 1 || T > CLHIP_MAX_TASKS || row_elems == 0 || B < 0) return CLHIP_EINVAL;
    if (B == 0) return 0;
    if (!idx || !x_out || !labels_out || B > 65535) return CLHIP_EINVAL;
    const size_t seg = (size_t)GT_BLOCK * GT_VEC_PER_THREAD * 4;
    const size_t segs = (row_elems + seg - 1) / seg;
    if (segs > 0x7fffffffull) return CLHIP_EINVAL;
    hipLaunchKernelGGL(gather_tasks_kernel, dim3((unsigned)segs, (unsigned)B), dim3(GT_BLOCK), 0, as_stream(stream), tasks_dev, T,
                       row_elems, idx, x_out, labels_out);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_gather_tasks_u8(const clhip_task_src_u8* tasks_dev, int T, int C, size_t plane_elems, const float* lut,
                          const int64_t* idx, int B, float* x_out, int64_t* labels_out, void* stream) {
    if (!tasks_dev || T < 1 || T > CLHIP_MAX_TASKS || C < 1 || plane_elems < 1 || !lut || B < 0) return CLHIP_EINVAL;
    if (plane_elems > SIZE_MAX / (size_t)C) return CLHIP_EINVAL;
    if (B == 0) return 0;
    if (!idx || !x_out || !labels_out || B > 65535) return CLHIP_EINVAL;
    const size_t seg = (size_t)GT_BLOCK * GT_VEC_PER_THREAD * 4;
    const size_t segs = ((size_t)C * plane_elems + seg - 1) / seg;
    if (segs > 0x7fffffffull) return CLHIP_EINVAL;
    hipLaunchKernelGGL(gather_tasks_u8_kernel, dim3((unsigned)segs, (unsigned)B), dim3(GT_BLOCK), 0, as_stream(stream), tasks_dev, T,
                       C, plane_elems, lut, idx, x_out, labels_out);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_slice_argmax_count(const float* logits, int N, int ld, const int* cols, int K, const int64_t* labels_i64,
                             int64_t* correct, int64_t* total, int64_t* out_of_range, void* stream) {
    if (!logits || !cols || !labels_i64 || !correct || !total || !out_of_range) return CLHIP_EINVAL;
    if (N < 0 || ld < 1 || K < 1 || K > ld) return CLHIP_EINVAL;
    if (N == 0) return 0;
    const int rows_per_block = SA_BLOCK / 64;
    hipLaunchKernelGGL(slice_argmax_count_kernel, dim3((unsigned)((N + rows_per_block - 1) / rows_per_block)), dim3(SA_BLOCK), 0,
                       as_stream(stream), logits, N, ld, cols, K, labels_i64, reinterpret_cast<unsigned long long*>(correct),
                       reinterpret_cast<unsigned long long*>(total), reinterpret_cast<unsigned long long*>(out_of_range));
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
