// One block's share of a resized crop + flip (the antialiased bilinear filter of clhip.h), shared by the task loaders' gather
// (augment.hip) and the exemplar batch assembly (rehearsal.hip): the host plan of a launch, the taps, and the block body.  Both
// callers run the SAME device code on a window, so their results are bitwise equal.
#pragma once
#include "crop_flip.hpp"
#include <math.h>

// Host plan of one launch: output lines per block (rpb), the LDS rows (nb) and row width (wmax) its source band may take, the
// taps per axis at the largest window the frame allows, the LDS bytes.  A window is at most min(Hs, R th) x min(Ws, R tw)
// (R = CLHIP_RESIZE_MAX_RATIO; the kernel rejects larger ones), so with s = min(Hs / th, R) the source lines of rpb
// neighbouring output lines span at most s (rpb - 1) + 2 max(s, 1) + 1 lines; + 2 covers the fp32 rounding of the centres.
constexpr int RZ_LDS_AIM = 48 * 1024;      // bytes per block the plan aims at (3 blocks per CU), RZ_LDS_MAX when one line needs more
constexpr int RZ_LDS_MAX = 64 * 1024;
struct rz_plan { int rpb, chunks, nb, wmax, ktx, kty; size_t lds; };

static inline int rz_align4(int v) { return (v + 3) & ~3; }

// `extra`: LDS bytes the block takes besides (the byte entry's table).
static inline bool rz_make_plan(int Hs, int Ws, int th, int tw, size_t extra, rz_plan* p) {
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

// One block (CF_BLOCK threads, ALL of them: the body has barriers) resamples the h x w window at (top, left) of one channel
// plane [..][Ws] (`plane`: its first element, float or byte) to output lines [y0, y0 + nrows) of a th x tw image, written as one
// contiguous run of nrows * tw floats at dst.  lds: the launch's dynamic LDS (16-byte aligned), the plan's bytes; rpb, nb,
// wmax, ktx_max, kty_max: the plan's.  The caller has checked the window (inside the frame, h <= R th, w <= R tw) and
// everything here is block-uniform.
//   0. the taps of its output lines and of all tw output columns (of column tw - 1 - x under a flip: everything after this is
//      flip-agnostic), computed on the device into LDS: wx[k][x], wy[k][line] (lanes along x / along the line: no bank conflicts)
//   1. the source band (the lines its output lines tap, all w columns of the window) global -> LDS, lanes along the source line,
//      dword loads (a line starts anywhere); byte frames (U8): byte loads, decoded here through the channel's table lut_c
//      [256] (staged in LDS in step 0), so raw[] holds what it holds for the decoded frames
//   2. the horizontal pass LDS -> LDS, once per source line of the band: tmp[j][x] = sum_k wx[k][x] raw[j][xlo[x] + k]
//   3. the vertical pass: out[y][x] = sum_k wy[k][y] tmp[ylo[y] - jlo + k][x], lanes along the output line, float4 when VEC
// SUMMATION ORDER (fixed; two runs are bitwise equal): both passes accumulate in fp32 by fmaf over the taps in ascending source
// index, starting from -0.0f (the identity of fp32 addition for every value, -0.0f included); a tap of weight exactly 0 is
// skipped, so nothing outside the support of the filter takes part (no 0 * inf).  A window of the output's size has one tap of
// weight exactly 1 per axis: the result is then the source value, bitwise.
template <bool VEC, bool U8, typename Src>
__device__ __forceinline__ void rz_resample_block(float* lds, Src plane, int Ws, int top, int left, int h, int w, int flip, int th,
                                                  int tw, int y0, int nrows, int rpb, int nb, int wmax, int ktx_max, int kty_max,
                                                  const float* __restrict__ lut_c, float* __restrict__ dst) {
    const int tid = threadIdx.x;
    float* raw = lds;                                     // [band][w]
    float* tmp = raw + ((nb * wmax + 3) & ~3);            // [band][tw]   (16-byte aligned lines when tw % 4 == 0)
    float* wx = tmp + nb * tw;                            // [ktx_max][tw]
    float* wy = wx + ktx_max * tw;                        // [kty_max][rpb]
    int* xlo = reinterpret_cast<int*>(wy + kty_max * rpb);
    int* ylo = xlo + tw;
    int* yhi = ylo + rpb;
    float* lut_s = reinterpret_cast<float*>(yhi + rpb);   // [256], byte frames only (the plan's `extra`)
    if constexpr (U8) lut_s[tid] = lut_c[tid];                             // (CF_BLOCK == 256: one entry each)
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

    Src src = plane + (size_t)(top + jlo) * Ws + left;
    {
        const int q = CF_BLOCK / w, rem = CF_BLOCK % w, total = band * w;  // a thread divides once, then steps (crop_flip.hpp)
        int j = tid / w, i = tid - j * w;
#pragma unroll 4
        for (int e = tid; e < total; e += CF_BLOCK) {
            if constexpr (U8) raw[e] = lut_s[src[(size_t)j * Ws + i]];
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
