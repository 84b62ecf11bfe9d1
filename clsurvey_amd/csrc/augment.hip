// On-device training augmentation of the task loaders: RandomCrop + RandomHorizontalFlip of the stored, already
// normalised frames (data/recogseq_dataprep.py:53-60, data/inaturalist_dataprep.py:232-253), done inside the gather that
// assembles a batch.
//   gather_tasks_crop_flip   clhip_gather_tasks (joint.hip) with one (top, left, flip) per batch position:
//                            x_out[b, c, y, x] = frame(idx[b])[c, top + y, left + (flip ? tw - 1 - x : x)]
//                            (torchvision's crop, then hflip).  A copy: bitwise.
#include "common.hpp"

namespace {

constexpr int CF_BLOCK = 256;
constexpr int CF_BATCH = 4;               // accesses per thread in flight at once (loads first, then the stores)
constexpr int CF_SEG = 4096;              // output elements per block the host aims at (16 KB, as gather_tasks_kernel)

// blockIdx.y = batch position.  blockIdx.x = (channel, chunk of `rpb` output lines): the block's destination is one contiguous
// run of nrows * tw floats, its source a nrows x tw window of one channel plane.  Everything that selects the source is
// block-uniform (scalar loads of idx / params / the table, the division by `chunks` on the scalar unit).  Lanes run along the
// output line, so loads are coalesced whichever way the line is read; a flip only reverses the lane order inside a line.
// A thread divides ONCE (its first element -> line, column); after that it steps by the block-uniform (q, rem) = stride / tw.
// A sample number outside [0, total), top outside [0, Hs - th], left outside [0, Ws - tw] or flip outside {0, 1} copies nothing
// and writes label -1: no address outside the source frame is ever formed (the host draws valid tables; this only keeps a bad
// one from faulting).
// VEC: tw % 4 == 0 and x_out 16-byte aligned (decided on the host): one float4 store per 4 output columns.  The source line
// start is arbitrarily aligned (any left, odd Ws), so the loads are written as dwords and promise 4-byte alignment only; read in
// ascending order and mirrored in registers, the compiler fuses four of them into one 16-byte load, which the hardware takes at
// dword alignment (measured against per-dword loads in mirrored order: 45.1 vs 48.2 us at 3 x 256^2 -> 224^2, 22.0 vs 21.2 us
// at 72^2 -> 64^2, batch 200).
template <bool VEC>
__global__ __launch_bounds__(CF_BLOCK) void gather_crop_flip_kernel(const clhip_task_src* __restrict__ tasks, int T, int C, int Hs,
                                                                     int Ws, int th, int tw, int rpb, int chunks,
                                                                     const int64_t* __restrict__ idx, const int* __restrict__ params,
                                                                     float* __restrict__ x_out, int64_t* __restrict__ labels_out) {
    const int r = blockIdx.y;
    const int64_t g = idx[r];
    const int top = params[3 * r], left = params[3 * r + 1], flip = params[3 * r + 2];
    const int lane = threadIdx.x & 63;                                      // bisect_right by ballot, as gather_tasks_kernel
    const int64_t cum = lane < T ? tasks[lane].cum_rows : INT64_MAX;
    const int t = __popcll(__ballot(cum <= g));
    if (g < 0 || t >= T || top < 0 || top > Hs - th || left < 0 || left > Ws - tw || (flip != 0 && flip != 1)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = -1;
        return;
    }
    const int64_t local = g - (t ? tasks[t - 1].cum_rows : 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = tasks[t].labels[local] + tasks[t].label_shift;
    const int c = (int)blockIdx.x / chunks;
    const int y0 = ((int)blockIdx.x - c * chunks) * rpb;
    const int nrows = min(rpb, th - y0);
    // (a pointer read out of the table is generic to the compiler; it is device memory, so say so: global_load, not flat_load)
    typedef const float __attribute__((address_space(1))) gfloat;
    gfloat* src = (gfloat*)(tasks[t].x + ((size_t)local * C + c) * Hs * Ws + (size_t)(top + y0) * Ws + left);
    float* dst = x_out + (((size_t)r * C + c) * th + y0) * tw;
    const unsigned total = (unsigned)nrows * (unsigned)tw;                 // <= max(CF_SEG, tw) < 2^31
    constexpr int W = VEC ? 4 : 1;                                         // output columns per access
    const int q = (CF_BLOCK * W) / tw, rem = (CF_BLOCK * W) % tw;
    int yy = (int)(threadIdx.x * W) / tw;
    int x = (int)(threadIdx.x * W) - yy * tw;
    for (unsigned e = threadIdx.x * W; e < total; e += CF_BATCH * CF_BLOCK * W) {
        float v[CF_BATCH][W];
#pragma unroll
        for (int k = 0; k < CF_BATCH; ++k) {                               // all loads in flight before the first store
            if (e + (unsigned)k * CF_BLOCK * W < total) {
                gfloat* s = src + (size_t)yy * Ws + (flip ? tw - W - x : x);
                float a[W];
#pragma unroll
                for (int j = 0; j < W; ++j) a[j] = s[j];                   // ascending addresses; mirrored in registers
#pragma unroll
                for (int j = 0; j < W; ++j) v[k][j] = flip ? a[W - 1 - j] : a[j];
            }
            x += rem;
            yy += q;
            if (x >= tw) { x -= tw; ++yy; }
        }
#pragma unroll
        for (int k = 0; k < CF_BATCH; ++k) {
            const unsigned i = e + (unsigned)k * CF_BLOCK * W;
            if (i < total) {
                if constexpr (VEC) *reinterpret_cast<float4*>(dst + i) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
                else dst[i] = v[k][0];
            }
        }
    }
}

}  // namespace

extern "C" {

int clhip_gather_tasks_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const int64_t* idx,
                                 const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    if (!tasks_dev || T < 1 || T > CLHIP_MAX_TASKS || C < 1 || th < 1 || tw < 1 || th > Hs || tw > Ws || B < 0) return CLHIP_EINVAL;
    if (B == 0) return 0;
    if (!idx || !params || !x_out || !labels_out || B > 65535) return CLHIP_EINVAL;
    const int rpb = tw >= CF_SEG ? 1 : CF_SEG / tw;                         // output lines per block
    const int chunks = (th + rpb - 1) / rpb;
    if ((size_t)C * chunks > 0x7fffffffull) return CLHIP_EINVAL;
    const dim3 grid((unsigned)(C * chunks), (unsigned)B);
    if (tw % 4 == 0 && aligned16(x_out))
        hipLaunchKernelGGL(gather_crop_flip_kernel<true>, grid, dim3(CF_BLOCK), 0, as_stream(stream), tasks_dev, T, C, Hs, Ws, th, tw,
                           rpb, chunks, idx, params, x_out, labels_out);
    else
        hipLaunchKernelGGL(gather_crop_flip_kernel<false>, grid, dim3(CF_BLOCK), 0, as_stream(stream), tasks_dev, T, C, Hs, Ws, th, tw,
                           rpb, chunks, idx, params, x_out, labels_out);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
