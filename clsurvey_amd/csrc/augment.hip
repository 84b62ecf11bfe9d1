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
// Both also serve BYTE frames (the ..._u8 entries; TS = clhip_task_src_u8): a stored byte v of channel c means lut[c][v], the
// ToTensor -> Normalize of the reference's Compose as a table the host computed.  The block's channel of the table is staged in
// LDS and every source element is decoded where it is loaded; everything after the load is the fp32 code, so the result is
// bitwise the fp32 entry's on the decoded frames.
#include "crop_flip.hpp"
#include <math.h>
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

// ---------------------------------------------------------------------------------------------- resized crop
// Host plan of one launch: output lines per block (rpb), the LDS rows (nb) and row width (wmax) its source band may take, the
// taps per axis at the largest window the frame allows, the LDS bytes.  A window is at most min(Hs, R th) x min(Ws, R tw)
// (R = CLHIP_RESIZE_MAX_RATIO; the kernel rejects larger ones), so with s = min(Hs / th, R) the source lines of rpb
// neighbouring output lines span at most s (rpb - 1) + 2 max(s, 1) + 1 lines; + 2 covers the fp32 rounding of the centres.
constexpr int RZ_LDS_AIM = 48 * 1024;      // bytes per block the plan aims at (3 blocks per CU), RZ_LDS_MAX when one line needs more
constexpr int RZ_LDS_MAX = 64 * 1024;
struct rz_plan { int rpb, chunks, nb, wmax, ktx, kty; size_t lds; };

static inline int rz_align4(int v) { return (v + 3) & ~3; }

// `extra`: LDS bytes the block takes besides (the byte entry's table).
static bool rz_make_plan(int Hs, int Ws, int th, int tw, size_t extra, rz_plan* p) {
    const double R = CLHIP_RESIZE_MAX_RATIO;
    const double sy = fmin((double)Hs / th, R), sx = fmin((double)Ws / tw, R);
    p->kty = (int)ceil(2.0 * fmax(sy, 1.0)) + 1;
    p->ktx = (int)ceil(2.0 * fmax(sx, 1.0)) + 1;
    p->wmax = (int)fmin((double)Ws, R * tw);
    for (int rpb = min(th, cf_rows_per_block(tw));; --rpb) {
        const double span = ceil(sy * (rpb - 1) + 2.0 * fmax(sy, 1.0)) + 3.0;
        const int nb = (int)fmin((double)Hs, span);
        const size_t floats = (size_t)rz_align4(nb * p->wmax) + (size_t)nb * tw + (size_t)p->ktx * tw + (size_t)p->kty * rpb;
        const size_t bytes = 4 * (floats + (size_t)tw + 2 * (size_t)rpb) + extra;
        if (bytes <= (size_t)RZ_LDS_AIM || (rpb == 1 && bytes <= (size_t)RZ_LDS_MAX)) {
            p->rpb = rpb;
            p->chunks = (th + rpb - 1) / rpb;
            p->nb = nb;
            p->lds = bytes;
            return true;
        }
        if (rpb == 1) return false;
    }
}

// Taps of output element o of an axis resized n_in -> n_out (the formula of clhip.h, fp32): lo, hi and the normalised weights
// wcol[k * stride], k < KT (0 from hi - lo on).  hi - lo <= KT and lo < n_in by the arithmetic; the clamps only keep a rounding
// surprise from reaching past the tables.
__device__ __forceinline__ void rz_taps(int o, int n_in, int n_out, int KT, float* wcol, int stride, int& lo, int& hi) {
    const float scale = (float)n_in / (float)n_out;
    const float sup = fmaxf(scale, 1.0f);
    const float c = scale * ((float)o + 0.5f);
    lo = min(max(0, (int)(c - sup + 0.5f)), n_in - 1);
    hi = max(min(min(n_in, (int)(c + sup + 0.5f)), lo + KT), lo + 1);
    float total = 0.0f;
    for (int k = 0; k < KT; ++k) {
        const float wv = lo + k < hi ? fmaxf(0.0f, 1.0f - fabsf(((float)(lo + k) - c + 0.5f) / sup)) : 0.0f;
        wcol[k * stride] = wv;
        total += wv;
    }
    for (int k = 0; k < KT; ++k) wcol[k * stride] = total > 0.0f ? wcol[k * stride] / total : 0.0f;
}

// blockIdx.y = batch position, blockIdx.x = (channel, chunk of `rpb` output lines) as gather_crop_flip_kernel; everything that
// selects the source is block-uniform.  One block:
//   0. the taps of its output lines and of all tw output columns (of column tw - 1 - x under a flip: everything after this is
//      flip-agnostic), computed on the device into LDS: wx[k][x], wy[k][line] (lanes along x / along the line: no bank conflicts)
//   1. the source band (the lines its output lines tap, all w columns of the window) global -> LDS, lanes along the source line,
//      dword loads (a line starts anywhere); byte frames: byte loads, decoded here through the channel's table (staged in LDS
//      in step 0), so raw[] holds what it holds for the decoded frames
//   2. the horizontal pass LDS -> LDS, once per source line of the band: tmp[j][x] = sum_k wx[k][x] raw[j][xlo[x] + k]
//   3. the vertical pass: out[y][x] = sum_k wy[k][y] tmp[ylo[y] - jlo + k][x], lanes along the output line, float4 when VEC
// SUMMATION ORDER (fixed; two runs are bitwise equal): both passes accumulate in fp32 by fmaf over the taps in ascending source
// index, starting from -0.0f (the identity of fp32 addition for every value, -0.0f included); a tap of weight exactly 0 is
// skipped, so nothing outside the support of the filter takes part (no 0 * inf).  A window of the output's size has one tap of
// weight exactly 1 per axis: the result is then the source value, bitwise.
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
    const int tid = threadIdx.x;

    float* raw = rz_lds;                                  // [band][w]
    float* tmp = raw + ((nb * wmax + 3) & ~3);            // [band][tw]   (16-byte aligned lines when tw % 4 == 0)
    float* wx = tmp + nb * tw;                            // [ktx_max][tw]
    float* wy = wx + ktx_max * tw;                        // [kty_max][rpb]
    int* xlo = reinterpret_cast<int*>(wy + kty_max * rpb);
    int* ylo = xlo + tw;
    int* yhi = ylo + rpb;
    float* lut_s = reinterpret_cast<float*>(yhi + rpb);   // [256], byte frames only (the plan's `extra`)
    if constexpr (ts_u8<TS>) lut_s[tid] = lut[c * 256 + tid];              // (CF_BLOCK == 256: one entry each)
    // taps this window needs (block-uniform; <= the plan's, which is made for the largest window)
    const int ktx = min(ktx_max, (int)ceilf(2.0f * fmaxf((float)w / (float)tw, 1.0f)) + 1);
    const int kty = min(kty_max, (int)ceilf(2.0f * fmaxf((float)h / (float)th, 1.0f)) + 1);

    for (int o = tid; o < tw; o += CF_BLOCK) {
        int lo, hi;
        rz_taps(flip ? tw - 1 - o : o, w, tw, ktx, wx + o, tw, lo, hi);
        xlo[o] = lo;
    }
    for (int o = tid; o < nrows; o += CF_BLOCK) {
        int lo, hi;
        rz_taps(y0 + o, h, th, kty, wy + o, rpb, lo, hi);
        ylo[o] = lo;
        yhi[o] = hi;
    }
    __syncthreads();
    const int jlo = ylo[0];                                                // (lo and hi do not decrease along an axis)
    const int band = min(yhi[nrows - 1] - jlo, nb);

    // (a pointer read out of the table is generic to the compiler; it is device memory, so say so: global_load, not flat_load)
    typedef typename std::conditional<ts_u8<TS>, const uint8_t, const float>::type __attribute__((address_space(1))) gelem;
    gelem* src = (gelem*)(tasks[t].x + ((size_t)local * C + c) * Hs * Ws + (size_t)(top + jlo) * Ws + left);
    {
        const int q = CF_BLOCK / w, rem = CF_BLOCK % w, total = band * w;  // a thread divides once, then steps (crop_flip.hpp)
        int j = tid / w, i = tid - j * w;
#pragma unroll 4
        for (int e = tid; e < total; e += CF_BLOCK) {
            if constexpr (ts_u8<TS>) raw[e] = lut_s[src[(size_t)j * Ws + i]];
            else raw[e] = src[(size_t)j * Ws + i];
            i += rem;
            j += q;
            if (i >= w) { i -= w; ++j; }
        }
    }
    __syncthreads();
    {
        const int q = CF_BLOCK / tw, rem = CF_BLOCK % tw, total = band * tw;
        int j = tid / tw, x = tid - j * tw;
        for (int e = tid; e < total; e += CF_BLOCK) {
            const float* line = raw + j * w;
            const int lo = xlo[x];
            float acc = -0.0f;
            for (int k = 0; k < ktx; ++k) {
                const float wv = wx[k * tw + x], v = line[min(lo + k, w - 1)];
                acc = wv != 0.0f ? fmaf(wv, v, acc) : acc;
            }
            tmp[e] = acc;
            x += rem;
            j += q;
            if (x >= tw) { x -= tw; ++j; }
        }
    }
    __syncthreads();
    {
        constexpr int W = VEC ? 4 : 1;                                     // output columns per thread and step
        const int n = tw / W;
        const int q = CF_BLOCK / n, rem = CF_BLOCK % n, total = nrows * n;
        int y = tid / n, x = tid - y * n;
        float* dst = x_out + (((size_t)r * C + c) * th + y0) * tw;
        for (int e = tid; e < total; e += CF_BLOCK) {
            const int j0 = ylo[y] - jlo;
            float acc[W];
#pragma unroll
            for (int m = 0; m < W; ++m) acc[m] = -0.0f;
            for (int k = 0; k < kty; ++k) {
                const float wv = wy[k * rpb + y];
                const float* line = tmp + max(min(j0 + k, band - 1), 0) * tw + x * W;
                if (wv != 0.0f) {                                          // (wave-uniform whenever a wave stays inside one line)
                    if constexpr (VEC) {
                        const float4 v = *reinterpret_cast<const float4*>(line);
                        acc[0] = fmaf(wv, v.x, acc[0]);
                        acc[1] = fmaf(wv, v.y, acc[1]);
                        acc[2] = fmaf(wv, v.z, acc[2]);
                        acc[3] = fmaf(wv, v.w, acc[3]);
                    } else {
                        acc[0] = fmaf(wv, line[0], acc[0]);
                    }
                }
            }
            if constexpr (VEC) *reinterpret_cast<float4*>(dst + (size_t)e * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else dst[e] = acc[0];
            x += rem;
            y += q;
            if (x >= n) { x -= n; ++y; }
        }
    }
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

int clhip_gather_tasks_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const int64_t* idx,
                                 const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    return gather_crop_flip(tasks_dev, T, C, Hs, Ws, th, tw, nullptr, idx, params, B, x_out, labels_out, stream);
}

int clhip_gather_tasks_crop_flip_u8(const clhip_task_src_u8* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const float* lut,
                                    const int64_t* idx, const int* params, int B, float* x_out, int64_t* labels_out, void* stream) {
    return gather_crop_flip(tasks_dev, T, C, Hs, Ws, th, tw, lut, idx, params, B, x_out, labels_out, stream);
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
