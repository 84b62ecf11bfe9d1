// On-device training augmentation of the task loaders: RandomCrop + RandomHorizontalFlip of the stored, already
// normalised frames (data/recogseq_dataprep.py:53-60, data/inaturalist_dataprep.py:232-253), done inside the gather that
// assembles a batch.
//   gather_tasks_crop_flip   clhip_gather_tasks (joint.hip) with one (top, left, flip) per batch position:
//                            x_out[b, c, y, x] = frame(idx[b])[c, top + y, left + (flip ? tw - 1 - x : x)]
//                            (torchvision's crop, then hflip).  A copy: bitwise.
// and RandomResizedCrop + RandomHorizontalFlip (data/tinyimgnet_dataprep.py:105-122, the cropped Tiny-ImageNet variant):
//   gather_tasks_resized_crop_flip   one (top, left, h, w, flip) per batch position: the h x w window of the frame resized to
//                            th x tw by the antialiased bilinear filter of ATen's _upsample_bilinear2d_aa (align_corners =
//                            False), then mirrored.  Separable: lines first, then columns, fp32, taps in ascending source order.
// and torchvision's RandomCrop(size, padding, fill, padding_mode) + RandomHorizontalFlip (the CIFAR-style rule; not in the
// reference's Composes, which crop a larger frame):
//   gather_tasks_pad_crop_flip   one (top, left, flip, h, w) per batch position: the window of the sample's PADDED image
//                            (constant / edge / reflect / symmetric around its h x w extent), then mirrored.  A copy: bitwise.
// All also serve BYTE frames (the ..._u8 entries; TS = clhip_task_src_u8): a stored byte v of channel c means lut[c][v], the
// ToTensor -> Normalize of the reference's Compose as a table the host computed.  The block's channel of the table is staged in
// LDS and every source element is decoded where it is loaded; everything after the load is the fp32 code, so the result is
// bitwise the fp32 entry's on the decoded frames.
#include "resized_crop.hpp"
#include <type_traits>

namespace {

template <typename TS> constexpr bool ts_u8 = std::is_same<TS, clhip_task_src_u8>::value;

// blockIdx.y = batch position.  blockIdx.x = (channel, chunk of `rpb` output lines): the block's destination is one contiguous
// run of nrows * tw floats, its source a nrows x tw window of one channel plane, copied by cf_copy_window (crop_flip.hpp).
// Everything that selects the source is block-uniform (scalar loads of idx / params / the table, the division by `chunks` on the
// scalar unit).
// A sample number outside [0, total), top outside [0, Hs - th], left outside [0, Ws - tw] or flip outside {0, 1} copies nothing
// and writes label -1: no address outside the source frame is ever formed (the host draws valid tables; this only keeps a bad
// one from faulting).
template <bool VEC, typename TS>
__global__ __launch_bounds__(CF_BLOCK) void gather_crop_flip_kernel(const TS* __restrict__ tasks, int T, int C, int Hs,
                                                                     int Ws, int th, int tw, int rpb, int chunks,
                                                                     const float* __restrict__ lut,
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
    float* dst = x_out + (((size_t)r * C + c) * th + y0) * tw;
    // (a pointer read out of the table is generic to the compiler; it is device memory, so say so: global_load, not flat_load)
    if constexpr (ts_u8<TS>) {
        __shared__ float lut_s[256];                                        // the table of channel c (CF_BLOCK == 256: one entry each)
        lut_s[threadIdx.x] = lut[c * 256 + (int)threadIdx.x];
        __syncthreads();
        typedef const uint8_t __attribute__((address_space(1))) gbyte;
        gbyte* src = (gbyte*)(tasks[t].x + ((size_t)local * C + c) * Hs * Ws + (size_t)(top + y0) * Ws + left);
        cf_copy_window<VEC>(src, Ws, dst, (unsigned)nrows * (unsigned)tw, tw, flip, cf_load_u8{lut_s});
    } else {
        typedef const float __attribute__((address_space(1))) gfloat;
        gfloat* src = (gfloat*)(tasks[t].x + ((size_t)local * C + c) * Hs * Ws + (size_t)(top + y0) * Ws + left);
        cf_copy_window<VEC>(src, Ws, dst, (unsigned)nrows * (unsigned)tw, tw, flip);  // total <= max(CF_SEG, tw) < 2^31
    }
}

// ---------------------------------------------------------------------------------------------- padded crop
// gather_crop_flip_kernel for RandomCrop(size, padding, fill, padding_mode) + flip: same grid, same block -> (channel, chunk
// of lines) split, same task selection and labels.  params rows are (top, left, flip, h, w): the window's corner in the
// UNPADDED coordinates of the sample's h x w extent (top in [-pt, h + pb - th], left in [-pl, w + pr - tw]); cf_copy_window_pad
// maps every source coordinate into the extent, so the frame is never read outside it.  The rows the header lists as bad copy
// nothing and write label -1 (64-bit compares: a bad table may hold any int32).  MODE (the padding mode) is a template argument:
// the maps compile to the mode's own two or three instructions.
template <bool VEC, int MODE, typename TS>
__global__ __launch_bounds__(CF_BLOCK) void gather_pad_crop_flip_kernel(const TS* __restrict__ tasks, int T, int C, int Hs,
                                                                         int Ws, int th, int tw, int rpb, int chunks,
                                                                         int pl, int pt, int pr, int pb,
                                                                         const float* __restrict__ fill,
                                                                         const float* __restrict__ lut,
                                                                         const int64_t* __restrict__ idx, const int* __restrict__ params,
                                                                         float* __restrict__ x_out, int64_t* __restrict__ labels_out) {
    const int r = blockIdx.y;
    const int64_t g = idx[r];
    const int top = params[5 * r], left = params[5 * r + 1], flip = params[5 * r + 2], h = params[5 * r + 3], w = params[5 * r + 4];
    const int lane = threadIdx.x & 63;                                      // bisect_right by ballot, as gather_tasks_kernel
    const int64_t cum = lane < T ? tasks[lane].cum_rows : INT64_MAX;
    const int t = __popcll(__ballot(cum <= g));
    constexpr int lim = MODE == CF_PAD_REFLECT ? 1 : 0;                     // reflect: pad <= extent - 1, symmetric: pad <= extent
    const bool one_reflection = MODE < CF_PAD_REFLECT || (max(pl, pr) <= w - lim && max(pt, pb) <= h - lim);
    if (g < 0 || t >= T || (flip != 0 && flip != 1) || h < 1 || h > Hs || w < 1 || w > Ws || top < -pt ||
        (int64_t)top > (int64_t)h + pb - th || left < -pl || (int64_t)left > (int64_t)w + pr - tw || !one_reflection) {
        if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = -1;
        return;
    }
    const int64_t local = g - (t ? tasks[t - 1].cum_rows : 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = tasks[t].labels[local] + tasks[t].label_shift;
    const int c = (int)blockIdx.x / chunks;
    const int y0 = ((int)blockIdx.x - c * chunks) * rpb;
    const int nrows = min(rpb, th - y0);
    float* dst = x_out + (((size_t)r * C + c) * th + y0) * tw;
    const float fill_c = fill[c];
    // (a pointer read out of the table is generic to the compiler; it is device memory, so say so: global_load, not flat_load)
    if constexpr (ts_u8<TS>) {
        __shared__ float lut_s[257];                                        // the table of channel c (CF_BLOCK == 256: one entry each)
        lut_s[threadIdx.x] = lut[c * 256 + (int)threadIdx.x];
        if (threadIdx.x == 0) lut_s[256] = fill_c;                          // entry 256: what a fill element decodes to
        __syncthreads();
        typedef const uint8_t __attribute__((address_space(1))) gbyte;
        gbyte* plane = (gbyte*)(tasks[t].x + ((size_t)local * C + c) * Hs * Ws);
        cf_copy_window_pad<VEC, MODE>(plane, Ws, h, w, top + y0, left, fill_c, dst, (unsigned)nrows * (unsigned)tw, tw, flip,
                                      cf_load_u8{lut_s});
    } else {
        typedef const float __attribute__((address_space(1))) gfloat;
        gfloat* plane = (gfloat*)(tasks[t].x + ((size_t)local * C + c) * Hs * Ws);
        cf_copy_window_pad<VEC, MODE>(plane, Ws, h, w, top + y0, left, fill_c, dst, (unsigned)nrows * (unsigned)tw, tw, flip);
    }
}

// ---------------------------------------------------------------------------------------------- resized crop
// blockIdx.y = batch position, blockIdx.x = (channel, chunk of `rpb` output lines) as gather_crop_flip_kernel; everything that
// selects the source is block-uniform.  The plan of the launch (rz_make_plan), the taps and the block's work, with its
// arithmetic and SUMMATION ORDER, are rz_resample_block's (resized_crop.hpp), which the exemplar assembly (rehearsal.hip) runs
// too.
// Rows the header lists as bad copy nothing and write label -1; no address outside the source frame is formed.
template <bool VEC, typename TS>
__global__ __launch_bounds__(CF_BLOCK) void gather_resized_kernel(const TS* __restrict__ tasks, int T, int C, int Hs, int Ws,
                                                                   int th, int tw, int rpb, int chunks, int nb, int wmax, int ktx_max,
                                                                   int kty_max, const float* __restrict__ lut,
                                                                   const int64_t* __restrict__ idx,
                                                                   const int* __restrict__ params, float* __restrict__ x_out,
                                                                   int64_t* __restrict__ labels_out) {
    extern __shared__ __attribute__((aligned(16))) float rz_lds[];
    const int r = blockIdx.y;
    const int64_t g = idx[r];
    const int top = params[5 * r], left = params[5 * r + 1], h = params[5 * r + 2], w = params[5 * r + 3], flip = params[5 * r + 4];
    const int lane = threadIdx.x & 63;
    const int64_t cum = lane < T ? tasks[lane].cum_rows : INT64_MAX;
    const int t = __popcll(__ballot(cum <= g));
    if (g < 0 || t >= T || h < 1 || w < 1 || top < 0 || left < 0 || top > Hs - h || left > Ws - w || (flip != 0 && flip != 1) ||
        (int64_t)h > (int64_t)CLHIP_RESIZE_MAX_RATIO * th || (int64_t)w > (int64_t)CLHIP_RESIZE_MAX_RATIO * tw) {
        if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = -1;
        return;
    }
    const int64_t local = g - (t ? tasks[t - 1].cum_rows : 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[r] = tasks[t].labels[local] + tasks[t].label_shift;
    const int c = (int)blockIdx.x / chunks;
    const int y0 = ((int)blockIdx.x - c * chunks) * rpb;
    const int nrows = min(rpb, th - y0);
    // (a pointer read out of the table is generic to the compiler; it is device memory, so say so: global_load, not flat_load)
    typedef typename std::conditional<ts_u8<TS>, const uint8_t, const float>::type __attribute__((address_space(1))) gelem;
    gelem* plane = (gelem*)(tasks[t].x + ((size_t)local * C + c) * Hs * Ws);
    const float* lut_c = nullptr;
    if constexpr (ts_u8<TS>) lut_c = lut + c * 256;
    rz_resample_block<VEC, ts_u8<TS>>(rz_lds, plane, Ws, top, left, h, w, flip, th, tw, y0, nrows, rpb, nb, wmax, ktx_max, kty_max,
                                      lut_c, x_out + (((size_t)r * C + c) * th + y0) * tw);
}

}  // namespace

// One body per pair of entries: TS selects the frames' element type, lut is NULL for floats.
template <typename TS>
static int gather_crop_flip(const TS* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const float* lut, const int64_t* idx,
                            const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    if (!tasks_dev || T < 1 || T > CLHIP_MAX_TASKS || C < 1 || th < 1 || tw < 1 || th > Hs || tw > Ws || B < 0) return CLHIP_EINVAL;
    if (ts_u8<TS> && !lut) return CLHIP_EINVAL;
    if (B == 0) return 0;
    if (!idx || !params || !x_out || !labels_out || B > 65535) return CLHIP_EINVAL;
    const int rpb = cf_rows_per_block(tw);
    const int chunks = (th + rpb - 1) / rpb;
    if ((size_t)C * chunks > 0x7fffffffull) return CLHIP_EINVAL;
    const dim3 grid((unsigned)(C * chunks), (unsigned)B);
    if (tw % 4 == 0 && aligned16(x_out))
        hipLaunchKernelGGL((gather_crop_flip_kernel<true, TS>), grid, dim3(CF_BLOCK), 0, as_stream(stream), tasks_dev, T, C, Hs, Ws,
                           th, tw, rpb, chunks, lut, idx, params, x_out, labels_out);
    else
        hipLaunchKernelGGL((gather_crop_flip_kernel<false, TS>), grid, dim3(CF_BLOCK), 0, as_stream(stream), tasks_dev, T, C, Hs, Ws,
                           th, tw, rpb, chunks, lut, idx, params, x_out, labels_out);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename TS>
static int gather_pad_crop_flip(const TS* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, int mode, int pl, int pt, int pr,
                                int pb, const float* fill, const float* lut, const int64_t* idx, const int* params, int B,
                                float* x_out, int64_t* labels_out, void* stream) {
    // (a crop larger than the frame is legal here: the padded image may hold it, and a row whose image does not is a bad row)
    if (!tasks_dev || !fill || T < 1 || T > CLHIP_MAX_TASKS || C < 1 || Hs < 1 || Ws < 1 || th < 1 || tw < 1 || B < 0)
        return CLHIP_EINVAL;
    if (Hs > CLHIP_PAD_MAX_EXTENT || Ws > CLHIP_PAD_MAX_EXTENT) return CLHIP_EINVAL;   // (2 n - 1 - s stays an int)
    if (mode < CF_PAD_CONSTANT || mode > CF_PAD_SYMMETRIC) return CLHIP_EINVAL;
    if (pl < 0 || pt < 0 || pr < 0 || pb < 0 || pl > CLHIP_PAD_MAX || pt > CLHIP_PAD_MAX || pr > CLHIP_PAD_MAX || pb > CLHIP_PAD_MAX)
        return CLHIP_EINVAL;
    if (ts_u8<TS> && !lut) return CLHIP_EINVAL;
    if (B == 0) return 0;
    if (!idx || !params || !x_out || !labels_out || B > 65535) return CLHIP_EINVAL;
    const int rpb = cf_rows_per_block(tw);
    const int chunks = (th + rpb - 1) / rpb;
    if ((size_t)C * chunks > 0x7fffffffull) return CLHIP_EINVAL;
    const dim3 grid((unsigned)(C * chunks), (unsigned)B);
    const bool vec = tw % 4 == 0 && aligned16(x_out);
#define CLHIP_PAD_LAUNCH(VEC, MODE)                                                                                                \
    hipLaunchKernelGGL((gather_pad_crop_flip_kernel<VEC, MODE, TS>), grid, dim3(CF_BLOCK), 0, as_stream(stream), tasks_dev, T, C, \
                       Hs, Ws, th, tw, rpb, chunks, pl, pt, pr, pb, fill, lut, idx, params, x_out, labels_out)
    switch (mode) {
    case CF_PAD_CONSTANT: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_CONSTANT); else CLHIP_PAD_LAUNCH(false, CF_PAD_CONSTANT); break;
    case CF_PAD_EDGE: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_EDGE); else CLHIP_PAD_LAUNCH(false, CF_PAD_EDGE); break;
    case CF_PAD_REFLECT: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_REFLECT); else CLHIP_PAD_LAUNCH(false, CF_PAD_REFLECT); break;
    default: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_SYMMETRIC); else CLHIP_PAD_LAUNCH(false, CF_PAD_SYMMETRIC); break;
    }
#undef CLHIP_PAD_LAUNCH
    CLHIP_LAUNCH_CHECK();
    return 0;
}

template <typename TS>
static int gather_resized(const TS* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const float* lut, const int64_t* idx,
                          const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    // (an output larger than the frame is an enlargement here, not an error)
    if (!tasks_dev || T < 1 || T > CLHIP_MAX_TASKS || C < 1 || Hs < 1 || Ws < 1 || th < 1 || tw < 1 || B < 0) return CLHIP_EINVAL;
    if (ts_u8<TS> && !lut) return CLHIP_EINVAL;
    if (B == 0) return 0;
    if (!idx || !params || !x_out || !labels_out || B > 65535) return CLHIP_EINVAL;
    rz_plan p;
    if (!rz_make_plan(Hs, Ws, th, tw, ts_u8<TS> ? 256 * sizeof(float) : 0, &p)) return CLHIP_ENOTSUP;   // one output line's band does not fit the LDS
    if ((size_t)C * p.chunks > 0x7fffffffull) return CLHIP_EINVAL;
    const dim3 grid((unsigned)(C * p.chunks), (unsigned)B);
    if (tw % 4 == 0 && aligned16(x_out))
        hipLaunchKernelGGL((gather_resized_kernel<true, TS>), grid, dim3(CF_BLOCK), p.lds, as_stream(stream), tasks_dev, T, C, Hs, Ws,
                           th, tw, p.rpb, p.chunks, p.nb, p.wmax, p.ktx, p.kty, lut, idx, params, x_out, labels_out);
    else
        hipLaunchKernelGGL((gather_resized_kernel<false, TS>), grid, dim3(CF_BLOCK), p.lds, as_stream(stream), tasks_dev, T, C, Hs, Ws,
                           th, tw, p.rpb, p.chunks, p.nb, p.wmax, p.ktx, p.kty, lut, idx, params, x_out, labels_out);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

// Host read-outs of the launch plans (no launch, no device): what the tests assert their geometries against.
int clhip_resized_crop_plan(int Hs, int Ws, int th, int tw, int byte_frames, int* out7) {
    if (Hs < 1 || Ws < 1 || th < 1 || tw < 1 || !out7) return CLHIP_EINVAL;
    rz_plan p;
    if (!rz_make_plan(Hs, Ws, th, tw, byte_frames ? 256 * sizeof(float) : 0, &p)) return CLHIP_ENOTSUP;   // (gather_resized's call)
    out7[0] = p.rpb; out7[1] = p.chunks; out7[2] = p.nb; out7[3] = p.wmax; out7[4] = p.ktx; out7[5] = p.kty;
    out7[6] = (int)p.lds;
    return 0;
}

int clhip_crop_rows_per_block(int tw) { return tw < 1 ? CLHIP_EINVAL : cf_rows_per_block(tw); }

int clhip_gather_tasks_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const int64_t* idx,
                                 const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    return gather_crop_flip(tasks_dev, T, C, Hs, Ws, th, tw, nullptr, idx, params, B, x_out, labels_out, stream);
}

int clhip_gather_tasks_crop_flip_u8(const clhip_task_src_u8* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const float* lut,
                                    const int64_t* idx, const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    return gather_crop_flip(tasks_dev, T, C, Hs, Ws, th, tw, lut, idx, params, B, x_out, labels_out, stream);
}

int clhip_gather_tasks_pad_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, int mode, int pl,
                                     int pt, int pr, int pb, const float* fill, const int64_t* idx, const int* params, int B,
                                     float* x_out, int64_t* labels_out, void* stream) {
    return gather_pad_crop_flip(tasks_dev, T, C, Hs, Ws, th, tw, mode, pl, pt, pr, pb, fill, nullptr, idx, params, B, x_out,
                                labels_out, stream);
}

int clhip_gather_tasks_pad_crop_flip_u8(const clhip_task_src_u8* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, int mode,
                                        int pl, int pt, int pr, int pb, const float* fill, const float* lut, const int64_t* idx,
                                        const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    return gather_pad_crop_flip(tasks_dev, T, C, Hs, Ws, th, tw, mode, pl, pt, pr, pb, fill, lut, idx, params, B, x_out, labels_out,
                                stream);
}

int clhip_gather_tasks_resized_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw,
                                         const int64_t* idx, const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    return gather_resized(tasks_dev, T, C, Hs, Ws, th, tw, nullptr, idx, params, B, x_out, labels_out, stream);
}

int clhip_gather_tasks_resized_crop_flip_u8(const clhip_task_src_u8* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw,
                                            const float* lut, const int64_t* idx, const int* params, int B, float* x_out,
                                            int64_t* labels_out, void* stream) {
    return gather_resized(tasks_dev, T, C, Hs, Ws, th, tw, lut, idx, params, B, x_out, labels_out, stream);
}

}  // extern "C"
