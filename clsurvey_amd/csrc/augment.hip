// On-device training augmentation of the task loaders: RandomCrop + RandomHorizontalFlip of the stored, already
// normalised frames (data/recogseq_dataprep.py:53-60, data/inaturalist_dataprep.py:232-253), done inside the gather that
// assembles a batch.
//   gather_tasks_crop_flip   clhip_gather_tasks (joint.hip) with one (top, left, flip) per batch position:
//                            x_out[b, c, y, x] = frame(idx[b])[c, top + y, left + (flip ? tw - 1 - x : x)]
//                            (torchvision's crop, then hflip).  A copy: bitwise.
#include "crop_flip.hpp"

namespace {

// blockIdx.y = batch position.  blockIdx.x = (channel, chunk of `rpb` output lines): the block's destination is one contiguous
// run of nrows * tw floats, its source a nrows x tw window of one channel plane, copied by cf_copy_window (crop_flip.hpp).
// Everything that selects the source is block-uniform (scalar loads of idx / params / the table, the division by `chunks` on the
// scalar unit).
// A sample number outside [0, total), top outside [0, Hs - th], left outside [0, Ws - tw] or flip outside {0, 1} copies nothing
// and writes label -1: no address outside the source frame is ever formed (the host draws valid tables; this only keeps a bad
// one from faulting).
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
    cf_copy_window<VEC>(src, Ws, dst, (unsigned)nrows * (unsigned)tw, tw, flip);      // total <= max(CF_SEG, tw) < 2^31
}

}  // namespace

extern "C" {

int clhip_gather_tasks_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const int64_t* idx,
                                 const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    if (!tasks_dev || T < 1 || T > CLHIP_MAX_TASKS || C < 1 || th < 1 || tw < 1 || th > Hs || tw > Ws || B < 0) return CLHIP_EINVAL;
    if (B == 0) return 0;
    if (!idx || !params || !x_out || !labels_out || B > 65535) return CLHIP_EINVAL;
    const int rpb = cf_rows_per_block(tw);
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
