/*
 * clhip.h — C ABI of libclhip.so: MI355X (gfx950 / CDNA4) kernels for the CLsurvey
 * per-task training + importance-weight hot path.
 *
 * The reference (Mattdl/CLsurvey) is pure Python on torch; every "kernel" it runs is an ATen
 * op reached from the files cited per entry point below (paths relative to /root/reference/src).
 * A maintainer binds this header with ctypes; no torch types cross it.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (fp32 unless the name says _u8 / _i64 / _f64)
 *   - tensors are dense NCHW / row-major exactly as torch lays them out (weights [K][C][3][3])
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     CLHIP_E* argument error. Kernels never allocate; scratch comes in through `ws`.
 */
#ifndef CLHIP_H
#define CLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the prototypes of this header are its whole dynamic symbol table (the
 * cross-translation-unit helpers of csrc/common.hpp stay inside the .so; one test hook, clhip_internal_stage_map, is exported from
 * csrc/stage_map.hpp and is not part of this API). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#define CLHIP_VISIBILITY_PUSHED 1
#endif

#define CLHIP_EINVAL (-1)   /* bad shape / null pointer */
#define CLHIP_ENOSPC (-2)   /* workspace too small */
#define CLHIP_ENOTSUP (-3)  /* shape not supported by this build */

/* Library version (major*10000 + minor*100 + patch) and the gfx arch it was built for. */
/* EBLL (methods/EBLL): the code layer of AutoEncoder (AlexNet_EBLL.py:9-26: Linear + Sigmoid), nn.MSELoss() on codes /
 * reconstructions (Finetune_SGD_EBLL.py:151, 297) with its gradient (times grad_scale) and optim.Adadelta (:497). */
int clhip_sigmoid_fwd(const float* x, float* y, size_t n, void* stream);
int clhip_sigmoid_bwd(const float* dy, const float* y, float* dx, size_t n, void* stream);
int clhip_mse_mean(const float* a, const float* b, size_t n, float grad_scale, float* da, float* loss_out, void* stream);
int clhip_adadelta_step(float* theta, const float* grad, float* square_avg, float* acc_delta, size_t n, float lr, float rho,
                        float eps, float weight_decay, void* stream);

int clhip_version(void);
const char* clhip_arch(void);

/* ------------------------------------------------------------------ convolution (MFMA fp32)
 * nn.Conv2d(C, K, 3, padding=1) (+ fused bias, ReLU) — models/VGGSlim.py:34-38.
 * y[N][K][H][W] = relu?(conv(x[N][C][H][W], w[K][C][3][3]) + b[K])
 * Size limits of every clhip_conv3x3_* entry point below up to clhip_conv3x3_bwd_weight_unpool (32-bit offsets inside one
 * image; whole tensors may exceed 2 GB): (C+32)*H*W < 2^28, (K+32)*H*W < 2^28, 9*K*C < 2^29, N*H*W < 2^31.
 * CLHIP_EINVAL beyond them, before any launch; clhip_conv3x3_bwd_weight_ws then reports 0.                */
int clhip_conv3x3_fwd(const float* x, const float* w, const float* b, float* y,
                      int N, int C, int K, int H, int W, int relu, void* stream);

/* Fused conv + bias + ReLU + 2x2/2 max-pool (VGGSlim.py:32-38): y_pool[N][K][H/2][W/2], idx_u8 = argmax
 * (0..3), or 4 for a window whose maximum after ReLU is not positive: max_pool2d backward followed by ReLU backward
 * (VGGSlim.py:32,38) passes nothing through such a window, so every consumer of the codes (`code == position`) applies
 * both, and backward-data of the NEXT layer may be called with relu_src = NULL.  The pre-pool activation is never
 * written (the first layer's would be 210 MB per batch).                                                    */
int clhip_conv3x3_relu_pool_fwd(const float* x, const float* w, const float* b, float* y_pool, uint8_t* idx_u8,
                                int N, int C, int K, int H, int W, void* stream);

/* autograd convolution_backward, data part. dx[N][C][H][W] from dy[N][K][H][W].
 * If relu_src != NULL: dx is multiplied by (relu_src > 0) — the fused ReLU backward
 * (threshold_backward) of the layer that PRODUCED this conv's input (VGGSlim.py:38).      */
int clhip_conv3x3_bwd_data(const float* dy, const float* w, const float* relu_src, float* dx,
                           int N, int C, int K, int H, int W, void* stream);

/* convolution_backward, weight + bias part. dw[K][C][3][3], db[K] (db may be NULL).
 * Deterministic: split partial sums live in `ws` (>= clhip_conv3x3_bwd_weight_ws bytes)
 * and are reduced in a fixed order (utils.set_random contract, utilities/utils.py:52-58).  */
size_t clhip_conv3x3_bwd_weight_ws(int N, int C, int K, int H, int W);
int clhip_conv3x3_bwd_weight(const float* x, const float* dy, float* dw, float* db,
                             int N, int C, int K, int H, int W, void* ws, size_t ws_bytes,
                             void* stream);

/* Backward-data of a conv whose ReLU output was 2x2-max-pooled, from the gradient w.r.t. the POOLED output + arg-max
 * codes (fused max_pool2d backward, as clhip_conv3x3_bwd_weight_unpool below).  16-byte-staging shapes only (K % 8 == 0,
 * C % 4 == 0, W % 4 == 0, whole tiles along w, aligned pointers): CLHIP_ENOTSUP otherwise.  relu_src as in
 * clhip_conv3x3_bwd_data.                                                                                      */
int clhip_conv3x3_bwd_data_unpool(const float* dy_pool, const uint8_t* idx_u8, const float* w, const float* relu_src,
                                  float* dx, int N, int C, int K, int H, int W, void* stream);

/* The same computation in two calls, for callers that defer the reduction (the plan executor reduces the slabs of
 * every layer of a backward pass in ONE launch): `_slabs` writes the per-split partial sums into ws and reports their
 * count, `_reduce` adds them in the fixed order of clhip_conv3x3_bwd_weight (bitwise the same dw / db).
 * idx_u8_or_null != NULL: dy is the POOLED gradient (see clhip_conv3x3_bwd_weight_unpool).                */
int clhip_conv3x3_bwd_weight_slabs(const float* x, const float* dy, const uint8_t* idx_u8_or_null, int N, int C, int K,
                                   int H, int W, void* ws, size_t ws_bytes, int* splits_out, void* stream);
int clhip_conv3x3_bwd_weight_reduce(const void* ws, float* dw, float* db, int K, int C, int splits, void* stream);

/* Same from the gradient w.r.t. the POOLED output + argmax (fused max_pool2d backward).  Implemented for the first-layer
 * kernel (C*9 <= 32) and for the 16-byte staging path of the general kernel (W % 4 == 0, whole tiles along w, aligned
 * pointers); returns CLHIP_ENOTSUP otherwise (callers then un-pool with clhip_maxpool2_bwd first).          */
int clhip_conv3x3_bwd_weight_unpool(const float* x, const float* dy_pool, const uint8_t* idx_u8, float* dw, float* db,
                                    int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ max-pool 2x2 stride 2
 * nn.MaxPool2d(2, 2) — models/VGGSlim.py:32. idx_u8 holds the argmax (0..3, row-major in the
 * window, first maximum wins as in ATen).  H, W are the INPUT sizes (even).  The backward kernel
 * also takes the fused kernels' code 4 ("no positive maximum": the window gets no gradient).
 * x (forward) and dx (backward) are accessed as float2: CLHIP_EINVAL unless they are 8-byte aligned. */
int clhip_maxpool2_fwd(const float* x, float* y, uint8_t* idx_u8, int NC, int H, int W, void* stream);
int clhip_maxpool2_bwd(const float* dy, const uint8_t* idx_u8, float* dx, int NC, int H, int W,
                       void* stream);

/* General k x k / stride max-pool, no padding (torchvision alexnet features[2,5,12]: MaxPool2d(3, 2), models/net.py:96-125).
 * idx = window position r*k + c of the first maximum (ATen scan order); backward gathers over the overlapping windows. */
int clhip_maxpool_fwd(const float* x, float* y, uint8_t* idx_u8, int NC, int H, int W, int k, int stride, void* stream);
int clhip_maxpool_bwd(const float* dy, const uint8_t* idx_u8, float* dx, int NC, int H, int W, int k, int stride, void* stream);

/* nn.BatchNorm2d (+ the ReLU behind it) of the '_BN' model variants (models/VGGSlim.py:27-40, models/net.py:152-156),
 * NCHW, HW = H*W.  training != 0: batch mean / biased variance, running_mean / running_var (may be NULL) moved by
 * `momentum` with the unbiased variance, as torch; training == 0: the running statistics.  save_mean / save_invstd [C]
 * are what the backward needs.  ws: clhip_bn_ws(C) bytes.  Backward: dy is the gradient w.r.t. y (post-ReLU when relu),
 * dz may alias dy; dgamma / dbeta (may be NULL) are overwritten. */
size_t clhip_bn_ws(int C);
int clhip_bn_fwd(const float* z, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                 float* save_mean, float* save_invstd, int N, int C, int HW, int training, float momentum, float eps, int relu,
                 void* ws, size_t ws_bytes, void* stream);
int clhip_bn_bwd(const float* dy, const float* y, const float* z, const float* gamma, const float* save_mean,
                 const float* save_invstd, float* dz, float* dgamma, float* dbeta, int N, int C, int HW, int training, int relu,
                 void* ws, size_t ws_bytes, void* stream);

/* General convolution (AlexNet: Conv2d(3,64,11,4,2), Conv2d(64,192,5,1,2), 3x3 pad 1 with 192/384/256 channels —
 * models/net.py:96-125 via torchvision.models.alexnet), NCHW / KCRS, zero padding `pad`, stride `stride`:
 * forward (+bias, optional ReLU), backward-data (optional ReLU mask relu_src > 0), backward-weight (+ db) with
 * caller-provided workspace of clhip_conv2d_bwd_weight_ws bytes. CLHIP_ENOTSUP if R*S > 256. */
size_t clhip_conv2d_bwd_weight_ws(int N, int C, int H, int W, int K, int R, int S, int stride, int pad);
int clhip_conv2d_fwd(const float* x, const float* w, const float* b, float* y, int N, int C, int H, int W, int K, int R, int S,
                     int stride, int pad, int relu, void* stream);
int clhip_conv2d_bwd_data(const float* dy, const float* w, const float* relu_src, float* dx, int N, int C, int H, int W, int K,
                          int R, int S, int stride, int pad, void* stream);
int clhip_conv2d_bwd_weight(const float* x, const float* dy, float* dw, float* db, int N, int C, int H, int W, int K, int R,
                            int S, int stride, int pad, void* ws, size_t ws_bytes, void* stream);

/* Weight / bias gradient of the 3x3 layer on the bf16 matrix cores with exact 3-piece fp32 splits of BOTH operands (csrc/bswgrad.hip):
 * the operator of clhip_conv3x3_wino_bwd_weight (same arguments; idx_u8 != NULL: dy is the pooled gradient [N][K][H/2][W/2] + the
 * forward pass's arg-max codes), for C % 64 == 0, K % 64 == 0, W % 16 == 0; other maps from 8 pixels wide (13 x 13!) with C % 32 == 0,
 * K % 32 == 0 and a plain dy run on the tap-split kernel of csrc/bswgrad5.hip (CLHIP_ENOTSUP otherwise).  ws:
 * clhip_conv3x3_bs_bwd_weight_ws(N, C, K, H, W) bytes of slabs, reduced in a fixed order (bitwise deterministic); 0 for a shape
 * neither kernel takes.  Order of the answers: N <= 0, a shape neither kernel takes, codes on an odd map or with a shape the 16-pixel
 * kernel does not take -> CLHIP_ENOTSUP; a NULL x / dy / dw / ws -> CLHIP_EINVAL; ws_bytes too small -> CLHIP_ENOSPC.  Per-image
 * limits: C*H*W*4 and K*H*W*4 < 2^31 - 1 on the 16-pixel kernel, N*C*H*W*4 and N*K*H*W*4 < 2^31 - 1 on the tap-split one.  Codes may
 * lie at any byte address. */
size_t clhip_conv3x3_bs_bwd_weight_ws(int N, int C, int K, int H, int W);
int clhip_conv3x3_bs_bwd_weight(const float* x, const float* dy, const uint8_t* idx_u8_or_null, float* dw, float* db, int N, int C, int K,
                                int H, int W, void* ws, size_t ws_bytes, void* stream);

/* Weight / bias gradient of the 5x5 / padding-2 convolution (AlexNet's Conv2d(64, 192, 5, padding=2), models/net.py:96-125) on the bf16
 * matrix cores with exact 3-piece fp32 splits of both operands (csrc/bswgrad5.hip): the operator of clhip_conv2d_bwd_weight(R = S = 5,
 * stride 1, pad 2), for C % 32 == 0, K % 32 == 0, W >= 8, tensors < 2 GB (CLHIP_ENOTSUP otherwise).  ws:
 * clhip_conv5x5_bs_bwd_weight_ws(N, C, K, H, W) bytes of slabs, reduced in a fixed order (bitwise deterministic). */
size_t clhip_conv5x5_bs_bwd_weight_ws(int N, int C, int K, int H, int W);
int clhip_conv5x5_bs_bwd_weight(const float* x, const float* dy, float* dw, float* db, int N, int C, int K, int H, int W, void* ws,
                                size_t ws_bytes, void* stream);

/* The same strided convolution by space-to-depth (csrc/s2dconv.hip): stride s in {2, 4}, 2 s < R <= 3 s, C s^2 <= 64, K % 64 == 0 —
 * AlexNet's Conv2d(3, 64, 11, 4, 2), models/net.py:96-125 — becomes a dense 3x3 convolution over the C s^2 phase planes of the
 * padded input and runs on clhip_conv3x3_bs_fwd / clhip_conv3x3_wino_bwd_weight over frames kept in `ws`
 * (clhip_conv2d_s2d_ws bytes; 0 = shape not taken, the entry points then return CLHIP_ENOTSUP).  Same results as
 * clhip_conv2d_fwd / clhip_conv2d_bwd_weight up to fp32 summation order.  bwd_weight with x == NULL reuses the phase planes the
 * forward call left in the same ws (same batch); there is no backward-data (the layer reads the images). */
size_t clhip_conv2d_s2d_ws(int N, int C, int H, int W, int K, int R, int stride, int pad);
int clhip_conv2d_s2d_fwd(const float* x, const float* w, const float* b, float* y, int N, int C, int H, int W, int K, int R, int stride,
                         int pad, int relu, void* ws, size_t ws_bytes, void* stream);
int clhip_conv2d_s2d_bwd_weight(const float* x_or_null, const float* dy, float* dw, float* db, int N, int C, int H, int W, int K, int R,
                                int stride, int pad, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ fully connected (MFMA fp32)
 * nn.Linear — models/VGGSlim.py:68-74.  x[M][I], w[O][I], b[O], y[M][O].                   */
/* ws: optional split-K scratch (>= clhip_fc_ws(M,I,O) bytes); NULL => no K split (slower, same result
 * up to summation order).                                                                   */
size_t clhip_fc_ws(int M, int I, int O);
int clhip_fc_fwd(const float* x, const float* w, const float* b, float* y,
                 int M, int I, int O, int relu, void* ws, size_t ws_bytes, void* stream);
/* dx[M][I] = dy[M][O] . w[O][I], optionally masked by (relu_src[M][I] > 0). */
int clhip_fc_bwd_data(const float* dy, const float* w, const float* relu_src, float* dx,
                      int M, int I, int O, void* ws, size_t ws_bytes, void* stream);
/* dw[O][I] = dy^T . x ; db[O] = column sums of dy (db may be NULL). */
int clhip_fc_bwd_weight(const float* x, const float* dy, float* dw, float* db,
                        int M, int I, int O, void* ws, size_t ws_bytes, void* stream);
/* y = relu(x) backward helper for non-fused callers: dx = dy * (y > 0). */
int clhip_relu_bwd(const float* dy, const float* y, float* dx, size_t n, void* stream);

/* ------------------------------------------------------------------ losses
 * CrossEntropyLoss (mean, reduction=0) — EWC/train_EWC.py:183; nll_loss(log_softmax, sum,
 * reduction=1) — EWC/main_EWC.py:148.  Writes loss_out[0], dlogits[N][C] (already scaled by
 * 1/N for mean) and, if stats != NULL, accumulates stats[0] += loss, stats[1] += #correct
 * (argmax == label; the running_loss / running_corrects of train_EWC.py:196-197) so the
 * host needs no per-batch .item() sync.  C <= 1024.                                         */
int clhip_softmax_ce(const float* logits, const int64_t* labels_i64, int N, int C, int reduction,
                     float* dlogits, float* loss_out, double* stats, void* stream);
/* Same over a column slice [col_off, col_off+ncols) of logits[N][ld] (labels relative to the slice; dlogits
 * outside the slice = 0): GEM's shared 200-way head, rehearsal/model/gem.py:259-263.          */
int clhip_softmax_ce_slice(const float* logits, const int64_t* labels_i64, int N, int ld, int col_off, int ncols,
                           int reduction, float* dlogits, float* loss_out, double* stats, void* stream);
/* MSELoss(size_average=False) against zeros — MAS/train_MAS.py:556-560: loss = sum(z^2),
 * dlogits = 2 z.                                                                            */
int clhip_mse_zero_sum(const float* logits, size_t n, float* dlogits, float* loss_out, void* stream);

/* LwF objective over stacked heads — LwF/main_LWF.py:47-76 (distillation_loss) and :184-202 (train_model_lwf):
 * logits [N][ld] = n_heads heads side by side (head_sizes, host array); last head = new task, CrossEntropy(mean);
 * every earlier head is distilled (temperature T) towards teacher [N][ld_teacher] (same column layout).
 * dlogits [N][ld] = d(task + reg_lambda * sum dist)/dlogits (columns past the last head = 0); loss_out2[0] = task loss, [1] = reg_lambda * sum of the
 * distillation terms; stats (optional, f64[2]) += (task loss, #correct on the new head). distill = 0: validation
 * (task loss / accuracy only, zero gradient on the old heads). N <= 1024.                                      */
int clhip_lwf_loss(const float* logits, const int64_t* labels_i64, const float* teacher, const int* head_sizes, int n_heads,
                   int N, int ld, int ld_teacher, float T, float reg_lambda, int distill, float* dlogits, float* loss_out2,
                   double* stats, void* stream);
/* The same objective (LwF/main_LWF.py:47-76, 184-202), the same contract and the same fp32 formulas for up to
 * CLHIP_LWF_MAX_HEADS_WIDE heads of any size (clhip_lwf_loss takes 32 heads and is one block with one thread per row by
 * design: a 10 x 20 layout on one CU).  Rows are spread over the GPU: one wave per row, 4 rows per block, the lanes of a wave
 * across the columns of a head (dword accesses only: no row, head or ld is assumed 16-byte aligned); each row leaves
 * (task, distillation, hit) in ws and a second one-block launch sums the rows in a fixed order (f64), so the result does not
 * depend on scheduling; no atomics.  loss_out2, stats, distill = 0, the zeros past the last head, the lowest-index arg-max rule
 * and "a single head needs no teacher" are those of clhip_lwf_loss.  ws: clhip_lwf_loss_wide_ws(n_heads, N) bytes (a multiple
 * of 16; 0 for n_heads outside 1..64 or N outside 1..1024), 4-byte aligned.
 * Refusals, in the order they are checked (a refused call launches nothing and writes nothing):
 *   CLHIP_EINVAL  logits, labels_i64, head_sizes, dlogits, loss_out2 or ws is NULL
 *   CLHIP_EINVAL  n_heads outside 1..CLHIP_LWF_MAX_HEADS_WIDE
 *   CLHIP_EINVAL  a head size <= 0
 *   CLHIP_EINVAL  the heads together wider than ld
 *   CLHIP_EINVAL  distill with more than one head and the old heads together wider than ld_teacher
 *   CLHIP_EINVAL  N outside 1..1024
 *   CLHIP_EINVAL  T <= 0 (or NaN)
 *   CLHIP_EINVAL  distill with more than one head and teacher NULL
 *   CLHIP_ENOSPC  ws_bytes < clhip_lwf_loss_wide_ws(n_heads, N)                                                          */
#define CLHIP_LWF_MAX_HEADS_WIDE 64          /* = CLHIP_MAX_TASKS */
size_t clhip_lwf_loss_wide_ws(int n_heads, int N);
int clhip_lwf_loss_wide(const float* logits, const int64_t* labels_i64, const float* teacher, const int* head_sizes, int n_heads,
                        int N, int ld, int ld_teacher, float T, float reg_lambda, int distill, float* dlogits, float* loss_out2,
                        double* stats, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ penalised optimizers
 * Weight_Regularized_SGD.step — EWC/train_EWC.py:23-86 == MAS/train_MAS.py:32-95.
 *   d = g + 2*lambda*omega*(theta - init);  d += wd*theta;
 *   buf = first ? d : momentum*buf + d;  theta -= lr*buf
 * omega == NULL  <=>  "p not in reg_params" (plain SGD, e.g. the fresh head).               */
int clhip_reg_sgd_step(float* theta, const float* grad, const float* omega, const float* init_val,
                       float* buf, size_t n, float reg_lambda, float lr, float momentum, float wd,
                       int first, void* stream);
/* diag_fisher accumulation — EWC/main_EWC.py:155: omega += grad^2 / data_len.               */
int clhip_fisher_accum(float* omega, const float* grad, size_t n, float data_len, void* stream);
/* Objective_After_SGD.step — MAS/train_MAS.py:167-173: omega = (omega*prev + |g|) / curr.   */
int clhip_mas_accum(float* omega, const float* grad, size_t n, float prev_size, float curr_size,
                    void* stream);
/* Elastic_SGD.step — SI/train_SI.py:28-126 (penalised momentum SGD + path integral w).      */
int clhip_si_step(float* theta, const float* grad, const float* omega, const float* init_val,
                  float* w, float* buf, size_t n, float reg_lambda, float lr, float momentum,
                  float wd, int first, void* stream);
/* update_reg_params — SI/train_SI.py:301-351: omega += max(w/((theta-init)^2+slack),0);
 * w = 0; init = theta.                                                                      */
int clhip_si_consolidate(float* omega, float* w, const float* theta, float* init_val, size_t n,
                         float slack, void* stream);

/* IMM_merge_models — IMM/merge.py:185-242, one parameter tensor of n_models (<= 32) task models:
 * precisions == NULL: mean-IMM  out = (sum_m theta_m) / n_models
 * else               mode-IMM  out = sum_m (precisions[m] / sum_precision) * theta_m
 * thetas / precisions are HOST arrays of device pointers.                                           */
int clhip_imm_merge(const float* const* thetas, const float* const* precisions, const float* sum_precision,
                    int n_models, size_t n, float* out, void* stream);

/* ------------------------------------------------------------------ PackNet masks (uint8, bit-exact)
 * methods/packnet/prune.py: mask value = owning task (1-based), 0 = free/pruned.
 *   finetune_mask  (:141-155)  mask[mask==0] = cur
 *   kth_abs        (:30-39)    cutoff = k-th smallest |w| over {mask==cur} (exact radix select;
 *                               k = round(prune_perc*numel) computed by the caller, k >= 1)
 *   prune          (:43-47,:64-71) mask[(|w|<=cutoff)&(mask==cur)] = 0 ; w[mask==0] = 0
 *   mask_grad_zero (:73-97)    grad[mask != cur] = 0
 *   mask_weight_zero mode 0 (:99-106 make_pruned_zero): w[mask==0]=0 ;
 *                    mode 1 (:108-118 apply_mask(idx)): w[mask==0 or mask>idx]=0
 *   packnet_sgd_step           fused do_batch tail (packnet/main.py:187-193): grads of foreign weights
 *                               -> 0, PacknetSGD.step (packnetSGD.py:35-56: weight decay masked by
 *                               grad != 0), pruned weights -> 0.  mask_u8 == NULL => plain PacknetSGD. */
int clhip_packnet_finetune_mask(uint8_t* mask_u8, size_t n, int cur, void* stream);
size_t clhip_packnet_kth_ws(void);
int clhip_packnet_kth_abs(const float* w, const uint8_t* mask_u8, size_t n, int cur, size_t k,
                          float* out_cutoff, void* ws, size_t ws_bytes, void* stream);
int clhip_packnet_prune(float* w, uint8_t* mask_u8, size_t n, int cur, const float* cutoff_dev, void* stream);
int clhip_mask_grad_zero(float* grad, const uint8_t* mask_u8, size_t n, int cur, void* stream);
int clhip_mask_weight_zero(float* w, const uint8_t* mask_u8, size_t n, int mode, int idx, void* stream);
int clhip_packnet_sgd_step(float* theta, float* grad, float* buf, const uint8_t* mask_u8, size_t n, int cur,
                           float lr, float momentum, float wd, int first, void* stream);

/* ------------------------------------------------------------------ 3x3 convolution by Winograd F(2x2, 3x3)
 * The same operators as clhip_conv3x3_fwd / _relu_pool_fwd / _bwd_data / _bwd_data_unpool (VGGSlim.py:27-40 and their
 * autograd backward) with 2.25x fewer matrix instructions per pixel: input / weight / output transforms fused into ONE
 * kernel (csrc/wino.hip), fp32, results equal to the direct kernels' up to rounding (~1e-6 of the output scale).
 * Shapes: C % 8 == 0, C >= 16, K % 32 == 0, H and W even (CLHIP_ENOTSUP otherwise: callers fall back to the direct
 * kernels).  idx_u8 != NULL on the forward: y is the 2x2-max-pooled activation [N][K][H/2][W/2] + arg-max codes;
 * idx_u8 != NULL on backward-data: dy is the gradient w.r.t. that pooled activation (fused max_pool2d backward).
 * ws: clhip_conv3x3_wino_ws(C, K) bytes (the transformed weights of this call).                              */
size_t clhip_conv3x3_wino_ws(int C, int K);
int clhip_conv3x3_wino_fwd(const float* x, const float* w, const float* b, float* y, uint8_t* idx_u8_or_null, int N, int C, int K,
                           int H, int W, int relu, void* ws, size_t ws_bytes, void* stream);
int clhip_conv3x3_wino_bwd_data(const float* dy, const uint8_t* idx_u8_or_null, const float* w, const float* relu_src, float* dx,
                                int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* dW, db of the same convolution through the Winograd weight-gradient form G^T[(A dY A^T).*(B^T d B)]G (C % 64 == 0,
 * K % 64 == 0, even H, W; CLHIP_ENOTSUP otherwise).  ws: clhip_conv3x3_wino_bwd_weight_ws(N, C, K, H, W) bytes — partial slabs in
 * the format of clhip_conv3x3_bwd_weight_slabs, summed in a fixed order (deterministic).  idx_u8 != NULL: dy is the POOLED gradient. */
size_t clhip_conv3x3_wino_bwd_weight_ws(int N, int C, int K, int H, int W);
int clhip_conv3x3_wino_bwd_weight(const float* x, const float* dy, const uint8_t* idx_u8_or_null, float* dw, float* db, int N, int C,
                                  int K, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* The whole backward of one such layer — dx (clhip_conv3x3_wino_bwd_data) and dW, db (clhip_conv3x3_wino_bwd_weight) — as ONE
 * grid: the blocks of the two launches interleaved so that blocks in their memory phases share the CUs with blocks in their matrix
 * phases (the autograd backward of one conv of VGGSlim.py:27-40; results bit-identical to the two entry points above wherever they
 * run the same kernels — every layer the VGG9 plans merge, asserted per shape in tests/test_gpu_pair.py; on 8 x 8 maps with
 * N * ceil(C / 32) > 512 and few units the stand-alone backward-data launch is the two-wave-shape instance of wino_conv16_kernel and the
 * agreement is up to fp32 summation order).  Taken for the
 * layers whose launches fill one round of blocks or less: even maps of at most 256 pixels, 16 or more wide or 8 x 8, weight gradient
 * on the pixel-split kernel, 16-byte-aligned tensors; CLHIP_ENOTSUP otherwise (nothing launched: call the two entry points).
 * ws: clhip_conv3x3_wino_bwd_ws(N, C, K, H, W) bytes.                                                                             */
size_t clhip_conv3x3_wino_bwd_ws(int N, int C, int K, int H, int W);
int clhip_conv3x3_wino_bwd(const float* x, const float* dy, const uint8_t* idx_u8_or_null, const float* w, const float* relu_src,
                           float* dx, float* dw, float* db, int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ 3x3 convolution on the bf16 matrix cores, split fp32 operands
 * The same operators again (VGGSlim.py:27-40 and their autograd backward w.r.t. the input; arguments as the _wino_ entry points)
 * in DIRECT form on v_mfma_f32_32x32x16_bf16: every fp32 operand is split exactly into three bf16 pieces, the six products
 * a_i * b_j (i + j <= 2) of each 16-deep k-step are accumulated in fp32 inside the matrix core (csrc/bsconv.hip).  Measured error
 * against fp64 = that of an fp32 fmaf chain (profiles/r05_bf16_split_dot.txt); results equal the other paths' up to fp32 rounding.
 * Non-finite inputs: an operand that is +-Inf, or so large that its leading bf16 piece rounds to Inf (|v| > 3.39e38), splits into
 * Inf + NaN residuals, so such an output is NaN where the f32 kernels give +-Inf; either way the loss is non-finite and the trainers
 * stop the attempt (train_EWC.py:204-205).
 * Shapes: C % 32 == 0, K % 64 == 0 on the forward (K % 32, C % 64 on backward-data), H, W >= 4; fused pooling on even maps only;
 * CLHIP_ENOTSUP otherwise.  ws: clhip_conv3x3_bs_ws(C, K) bytes (the weight image of this call).
 * Order of the answers: N <= 0 or a shape outside the domain -> CLHIP_ENOTSUP; a NULL x / w / y (dy / w / dx) or ws, or ws_bytes below
 * the weight image -> CLHIP_EINVAL (these entry points have no CLHIP_ENOSPC); a size beyond the limits below -> CLHIP_EINVAL; arg-max
 * codes on an odd map -> CLHIP_ENOTSUP; all of it before anything is launched.
 * Size limits (32-bit offsets inside the images of one block; the batch and whole tensors may exceed 2 GB), with Cin / Cout the
 * channels as the kernel sees them (C, K forward; K, C backward-data) and stated on the un-pooled H x W map: Cin*H*W < 2^29
 * (< 2^28 for the 3x3 entry points where W <= 8: two images per block), Cout*H*W < 2^29, and a weight image
 * (clhip_conv3x3_bs_ws / clhip_conv5x5_bs_ws of this direction) under 2^31 bytes.  The 5x5 pair below has the same limits.
 * Arg-max codes may lie at any byte address (off a 4-byte boundary the pooled forward stores them byte by byte).              */
size_t clhip_conv3x3_bs_ws(int C, int K);
int clhip_conv3x3_bs_fwd(const float* x, const float* w, const float* b, float* y, uint8_t* idx_u8_or_null, int N, int C, int K,
                         int H, int W, int relu, void* ws, size_t ws_bytes, void* stream);
int clhip_conv3x3_bs_bwd_data(const float* dy, const uint8_t* idx_u8_or_null, const float* w, const float* relu_src, float* dx,
                              int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* clhip_conv3x3_bs_bwd_data whose launch also carries `riders` extra blocks that reduce finished weight-gradient slabs while the
 * convolution blocks run (csrc/bsconv.hip, bs_conv_riders_kernel; what the plan executor does at its lowest bf16-split layer,
 * CLHIP_REDUCE_RIDERS).  Job i: `splits` slabs of taps * K * C + K floats back to back at `slabs`, complete on `stream` before the
 * call; dw [K][C][taps] and db [K] (may be NULL) receive exactly what clhip_conv3x3_bwd_weight_reduce writes (taps: 9 or 25).
 * place: 1 riders in front of the convolution blocks, 2 behind them, 3 spread through the grid; riders: a multiple of 8.
 * dx is bitwise that of clhip_conv3x3_bs_bwd_data.  Answers as there; a bad job -> CLHIP_EINVAL; n_jobs outside 1 .. 32, another
 * place, riders no positive multiple of 8 -> CLHIP_ENOTSUP, nothing launched. */
typedef struct clhip_reduce_job {
    const float* slabs;
    float* dw;
    float* db;
    int K, C, splits, taps;
} clhip_reduce_job;
int clhip_conv3x3_bs_bwd_data_riders(const float* dy, const uint8_t* idx_u8_or_null, const float* w, const float* relu_src, float* dx,
                                     int N, int C, int K, int H, int W, void* ws, size_t ws_bytes, const clhip_reduce_job* jobs,
                                     int n_jobs, int place, int riders, void* stream);
/* The same kernel with 5 x 5 taps (stride 1, padding 2): torchvision AlexNet's features[3], nn.Conv2d(64, 192, 5, padding=2) + ReLU
 * (models/net.py:96-125) and its autograd w.r.t. the input (dx *= (relu_src > 0) when relu_src != NULL).  w: [K][C][5][5].
 * C % 32 == 0, K % 64 == 0 on the forward (roles swapped on backward-data), W > 8.  ws: clhip_conv5x5_bs_ws(C, K) bytes.      */
size_t clhip_conv5x5_bs_ws(int C, int K);
int clhip_conv5x5_bs_fwd(const float* x, const float* w, const float* b, float* y, int N, int C, int K, int H, int W, int relu,
                         void* ws, size_t ws_bytes, void* stream);
int clhip_conv5x5_bs_bwd_data(const float* dy, const float* w, const float* relu_src, float* dx, int N, int C, int K, int H, int W,
                              void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ HAT gates / back-masks / HAT_SGD
 * methods/HAT/networks/vgg_hat.py, approaches/hat.py, HAT_utils.py.  Gates multiply layer outputs in the
 * reference (vgg_hat.py:104-116); here they are folded into the NEXT layer's weights
 * (W'[k][c][r] = W[k][c][r]*gate[c]) so the conv/FC kernels run unchanged on un-gated activations.
 *   hat_gate        (:121-127)  gate = sigmoid(s * emb_row)
 *   hat_scale_weight            out = w * gate_in[c]   (w viewed as [K][C][R]; gate_in NULL => copy)
 *   hat_weight_grad             dw = g_wprime * gate_in[c] ; dgate_in[c] = sum_{k,r} g_wprime * w
 *   hat_emb_grad                demb = (dgate + lamb_over_count*(1-mask_pre)) * s*a*(1-a)   (hat.py:285-299)
 *   hat_reg_sums                sums2[0] += sum gate*(1-mask_pre); sums2[1] += sum (1-mask_pre)
 *   hat_backmask    (:258-295)  out[k][c][r] = 1 - min(a_post[k], a_pre[c])   (a_pre NULL => 1 - a_post[k])
 *   hat_sgd_step    (HAT_utils.py:192-250) wd (not on embs), grad *= mask_back, embedding compensation
 *                   (smax/s)*(cosh(clamp(s*e,+-thres))+1)/(cosh(e)+1), clip_grad_norm(p, clipgrad), momentum SGD
 *   clamp           (hat.py:238-240) embeddings to +-6                                               */
int clhip_hat_gate(const float* emb_row, int n, float s, float* gate, void* stream);
int clhip_hat_scale_weight(const float* w, const float* gate_in, float* out, size_t K, size_t C, size_t R, void* stream);
int clhip_hat_weight_grad(const float* g_wprime, const float* w, const float* gate_in, float* dw, float* dgate_in,
                          int K, int C, int R, void* stream);
int clhip_hat_emb_grad(const float* dgate, const float* gate, const float* mask_pre, int n, float s,
                       float lamb_over_count, float* demb, void* stream);
int clhip_hat_reg_sums(const float* gate, const float* mask_pre, int n, double* sums2, void* stream);
int clhip_hat_backmask(const float* a_post, const float* a_pre, float* out, size_t K, size_t C, size_t R, void* stream);
size_t clhip_hat_sgd_ws(void);
int clhip_hat_sgd_step(float* theta, float* grad, float* buf, const float* mask_back, size_t n, float lr,
                       float momentum, float wd, int is_emb, int finetune, float s, float smax, float thres_cosh,
                       float clipgrad, int first, void* ws, size_t ws_bytes, void* stream);
int clhip_clamp(float* x, size_t n, float lo, float hi, void* stream);

/* The same arithmetic for a whole net per launch (job tables on the host, copied into the kernel arguments): one HAT
 * training batch is gates + regulariser sums (1 launch), W' for every layer (1), [the net's own plan], dW / dgate for every
 * gated layer (1), embedding gradients (1), HAT_SGD.step over every parameter incl. the embedding clamp (2).
 *   hat_gates_multi        gate_l = sigmoid(s * emb_row_l); sums2[0] = sum gate*(1-mask_pre), sums2[1] = sum (1-mask_pre)
 *                          and sums2[2] = their ratio (3 doubles, written, not accumulated; sums2 may be NULL)
 *   hat_scale_weights_multi  out = w * gate_in[c] per layer (gate_in NULL => copy: biases, the first layer)
 *   hat_weight_grads_multi   in place: dgate_in[c] = sum_{k,r} g*w ; g *= gate_in[c]
 *   hat_emb_grads_multi      demb[rows][n] = 0 except row t = (dgate + lamb/count*(1-mask_pre)) * s*a*(1-a); count <= 0 reads
 *                            sums2[1] on the device (no host synchronisation)
 *   hat_sgd_step_multi       HAT_utils.py:192-250 per parameter (clip_grad_norm_ is per parameter) + clamp of the embeddings to
 *                            +-thres_emb when thres_emb > 0 (hat.py:238-240); ws: clhip_hat_sgd_multi_ws(n_params) bytes   */
typedef struct { float* theta; float* grad; float* buf; const float* mask_back; size_t n; int is_emb; int reserved; } clhip_hat_param;
typedef struct { const float* emb_row; float* gate; const float* mask_pre; int n; int reserved; } clhip_hat_gate_job;
typedef struct { const float* w; const float* gate_in; float* out; size_t K, C, R; } clhip_hat_layer;
typedef struct { float* g; const float* w; const float* gate_in; float* dgate_in; int K, C, R, reserved; } clhip_hat_wgrad_job;
typedef struct { const float* dgate; const float* gate; const float* mask_pre; float* demb; int n, rows, t, reserved; } clhip_hat_emb_job;
size_t clhip_hat_sgd_multi_ws(int n_params);
int clhip_hat_sgd_step_multi(const clhip_hat_param* params, int n_params, float lr, float momentum, float wd, int finetune,
                             float s, float smax, float thres_cosh, float clipgrad, float thres_emb, int first, void* ws,
                             size_t ws_bytes, void* stream);
int clhip_hat_gates_multi(const clhip_hat_gate_job* jobs, int n_jobs, float s, double* sums2, void* stream);
int clhip_hat_scale_weights_multi(const clhip_hat_layer* layers, int n_layers, void* stream);
int clhip_hat_weight_grads_multi(const clhip_hat_wgrad_job* jobs, int n_jobs, void* stream);
int clhip_hat_emb_grads_multi(const clhip_hat_emb_job* jobs, int n_jobs, float s, float lamb, float count, const double* sums2,
                              void* stream);

/* ------------------------------------------------------------------ PathNet (networks/vgg_pathnet.py, approaches/pathnet.py)
 * A path (N of M modules per layer, summed behind ReLU / pool) runs as a plain narrow net over a PACKED arena:
 *   layer 0     Wp[n*c_out + k][j][r]            = mod[path[n]].w[k][j][r]
 *   layer l > 0 Wp[n*c_out + k][m*c_in + j][r]   = mod[path[n]].w[k][j][r]  for every m < n_in   (n_in = N of the layer before)
 *   head        n_out = 1, M = 1, path[0] = 0
 * with every packed width padded by zero rows / columns to Kp x Cp.  One table row per layer (the head is a row); all
 * offsets count floats from the arena bases handed to the call; the modules of one layer lie mod_stride floats apart
 * (weight and bias alike).  path[n] < 0: the slot contributes nothing.  trainable: bit i = module i trains
 * (vgg_pathnet.py:130-150); only modules that are trainable AND in path[0..n_out) are folded / stepped, every other
 * module's gradient, momentum and weights are left untouched.
 *   pathnet_pack_multi        module arena -> packed arena (bitwise copies, padding = 0), ONE launch
 *   pathnet_fold_grads_multi  packed gradient -> g[mod][k][j][r] = sum_{n: path[n]==mod} sum_m G[n*c_out+k][m*c_in+j][r]
 *                             (n, then m, ascending); biases over the duplicate slots; ws receives one double per block:
 *                             the sum of squares of what the block wrote (0 for a block without work)
 *   pathnet_sgd_step          clip_grad_norm(active, clipgrad) (coef = clip / (norm + 1e-6), applied when < 1; the norm is the
 *                             fixed-order sum of ws) then SGD: g += wd*p; buf = first ? g : momentum*buf + g; p -= lr*buf
 * ws: clhip_pathnet_ws(layers, n_layers) bytes, the same table for fold and step.                                            */
#define CLHIP_PATHNET_MAX_N 8
#define CLHIP_PATHNET_MAX_LAYERS 24
typedef struct {
    long w_off, b_off;          /* module 0's weight / bias in the module arenas */
    long pw_off, pb_off;        /* packed weight / bias in the packed arenas */
    long mod_stride;
    int c_out, c_in, R;         /* one module's weight is [c_out][c_in][R] */
    int n_out, n_in;            /* slots of this layer, slots of the layer before (1 for layer 0) */
    int Kp, Cp;                 /* packed weight is [Kp][Cp][R], Kp >= n_out*c_out, Cp >= n_in*c_in */
    int M;
    int path[CLHIP_PATHNET_MAX_N];
    unsigned long long trainable;
} clhip_pathnet_layer;
size_t clhip_pathnet_ws(const clhip_pathnet_layer* layers, int n_layers);
/* mod_numel / packed_numel: floats in the module / packed arenas; a table that names a slot beyond them is CLHIP_EINVAL */
int clhip_pathnet_pack_multi(const clhip_pathnet_layer* layers, int n_layers, const float* mod_theta, size_t mod_numel,
                             float* packed_theta, size_t packed_numel, void* stream);
int clhip_pathnet_fold_grads_multi(const clhip_pathnet_layer* layers, int n_layers, const float* packed_grad, size_t packed_numel,
                                   float* mod_grad, size_t mod_numel, void* ws, size_t ws_bytes, void* stream);
int clhip_pathnet_sgd_step(const clhip_pathnet_layer* layers, int n_layers, float* mod_theta, float* mod_grad, float* mod_buf,
                           size_t mod_numel, float lr, float momentum, float wd, float clipgrad, int first, const void* ws,
                           size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ static-plan net executor
 * One call per pass for VGG-style nets instead of one Python dispatch per op
 * (replaces `outputs = model(inputs); loss.backward()` of EWC/train_EWC.py:181-187,
 * EWC/main_EWC.py:147-149, MAS/train_MAS.py:549-560, framework/inference.py:52-68).
 * params / grads are flat fp32 arenas; w_off / b_off are float offsets into them.          */
typedef struct {
    int type;            /* 0: conv3x3 pad 1 (+ReLU) (+2x2 max-pool)   1: Linear (+ReLU) */
    int cin, cout;       /* channels (conv) or in/out features (fc) */
    int relu, pool;      /* pool: 0 none, 1 = a max-pool follows (pool_k x pool_k, stride pool_s; 0/0 means 2x2 stride 2) */
    long w_off, b_off;
    int ksize, stride, pad;   /* conv geometry; ksize 0 means the VGG default 3x3, stride 1, pad 1 */
    int pool_k, pool_s;
    int bn;                   /* conv layers: 1 = BatchNorm2d between the convolution and the ReLU (clhip_net_set_bn) */
    long bn_w_off, bn_b_off;  /* float offsets of the BatchNorm weight / bias in the parameter arena */
    int has_drop;             /* a dropout may be set in front of this layer (clhip_net_set_dropout): its masked input gets
                               * its own buffer, so that the un-masked activation stays readable (clhip_net_layer_input);
                               * without it the mask is applied in place */
} clhip_layer_desc;

int clhip_net_create(const clhip_layer_desc* layers, int n_layers, int max_batch, int in_c, int in_h,
                     int in_w, void** out_handle);
/* nn.Dropout of the AlexNet classifier (torchvision alexnet: classifier[0], [3]) in training mode, and GEM's per-observe
 * masks (methods/rehearsal/GEM/gem.py:166-196): the mask (values 0 or 1/p_retain, drawn by the caller) multiplies the
 * INPUT of plan layer `layer` (> 0) in forward and the gradient w.r.t. it in backward.  mask [N][in_elems] with
 * row_stride floats between samples, row_stride 0 = one row for the whole batch; NULL = off (eval mode). */
int clhip_net_set_dropout(void* handle, int layer, const float* mask, long row_stride);
/* BatchNorm buffers of plan layer `layer` (device fp32 [cout]; updated in place by training-mode forwards) and the
 * module's momentum / eps; clhip_net_set_training switches every BatchNorm layer between batch and running statistics
 * (nn.Module.train / eval). */
int clhip_net_set_bn(void* handle, int layer, float* running_mean, float* running_var, float momentum, float eps);
int clhip_net_set_training(void* handle, int training);
/* Measurement only (bench.py's roofline object): HIP events around the forward launch(es) of plan layer `layer`, recorded
 * on the stream of each clhip_net_forward / clhip_net_loss_step call into a ring of 64 pairs (layer < 0: off).
 * clhip_net_probe_read waits for the recorded launches, returns their average duration in microseconds and how many
 * passes it covers, and restarts the count. */
int clhip_net_probe(void* handle, int layer);
/* the same around the layer's backward-data (kind 1) or weight-gradient (kind 2) launch(es); kind 0 = clhip_net_probe */
int clhip_net_probe_kind(void* handle, int layer, int kind);
int clhip_net_probe_read(void* handle, float* avg_us, int* count);
/* Where the arg-max bytes of a max-pooled conv layer live after a forward: byte offset into ws and bytes per
 * sample ([cout][oh][ow], window position r*k + c, first maximum wins).  With the saved activations
 * (clhip_net_layer_input) this is every non-linear decision the backward pass will use — what a parity harness
 * needs to judge gradients independently of ReLU / arg-max near-ties.  EINVAL for layers without a pool.   */
int clhip_net_layer_pool_idx(void* handle, int layer, size_t* ws_byte_off, size_t* elems_per_sample);
/* Where the prepared weights of a pass live (Winograd U images and bf16-split images of every layer that takes such a path, written
 * at the start of each forward / stand-alone backward): byte offset into ws and size; *bytes = 0 for a plan without such layers.
 * A parity harness compares the region between two ways of launching its jobs (CLHIP_EDGE_GRIDS). */
int clhip_net_prepared_weights(void* handle, size_t* ws_byte_off, size_t* bytes);
/* How many forward passes of this plan built those weights INSIDE the first layer's forward launch (one merged grid,
 * CLHIP_EDGE_GRIDS != 0) instead of by a launch of their own; < 0 on error.  While it counts, a forward probe on layer 0
 * (clhip_net_probe_kind 0) times the merged launch, weight blocks included; with the separate launches they lie outside the pair. */
int clhip_net_edge_grid_count(void* handle);
/* How many backward passes of this plan reduced the weight-gradient slabs finished so far INSIDE the backward-data launch of the
 * plan's lowest bf16-split layer (rider blocks, CLHIP_REDUCE_RIDERS != 0; csrc/bsconv.hip) instead of leaving them to the one
 * reduction launch at the end of the pass; < 0 on error.  While it counts, a backward-data probe on that layer
 * (clhip_net_probe_kind 1) times the launch with its riders, and the reduction launch of the pass holds the remaining slabs only. */
int clhip_net_reduce_rider_count(void* handle);
/* Which kernels the plan chose for a layer (measurement harnesses time the same ones): bit 0 forward, bit 1 backward-data, bit 2
 * weight gradient through a prepared-weights path instead of the direct f32 MFMA kernels — Winograd F(2x2,3x3) (csrc/wino.hip)
 * unless bit 3 (forward) / bit 4 (backward-data) says the launch is the bf16-split kernel (csrc/bsconv.hip); bit 5: the weight
 * gradient is the bf16-split kernel (csrc/bswgrad.hip); < 0 on error.
 * Linear layers (bits 0 .. 5 are 0 for them): bit 6 (`fc_tail`) the layer's forward and backward-data run inside the fused
 * classifier tail (fc_tail_kernel, csrc/fc_chain.hip) — set for the Linear layers behind the first one of a plan that takes
 * the tail (created on a device, CLHIP_FC_TAIL != 0, max_batch <= 1024, widths inside the tail's envelope), as long as none
 * of them has a dropout mask or an extra input gradient set; a single call still runs the per-layer launches when the
 * caller's parameter / workspace pointers are not 16-byte aligned or N * (classes | 1) > 12288.  bit 7 (`fc_fused`) the
 * layer's weight and bias gradient come from the fused launch of the whole classifier (fc_chain_wgrad_kernel, or
 * fc_bwd_combo_kernel together with the first Linear layer's backward-data). */
int clhip_net_layer_paths(void* handle, int layer);

/* Side branches off a plan (EBLL's code layers on the flattened features, AlexNet_EBLL.py:110-117): the INPUT activation
 * of plan layer `layer` (> 0) lives at float offset *ws_float_off of the workspace after a forward (in_elems floats per
 * sample); `extra` ([N][in_elems], device, may be NULL = none) is added to the gradient w.r.t. that activation in the
 * following backward passes until changed. */
int clhip_net_layer_input(void* handle, int layer, size_t* ws_float_off, size_t* in_elems);
int clhip_net_set_input_grad(void* handle, int layer, const float* extra);
void clhip_net_destroy(void* handle);
size_t clhip_net_workspace_bytes(void* handle);
int clhip_net_num_classes(void* handle);
int clhip_net_forward(void* handle, const float* params, const float* x, int N, void* ws,
                      float* logits_out, void* stream);
int clhip_net_backward(void* handle, const float* params, float* grads, const float* x, int N, void* ws,
                       const float* dlogits, void* stream);
/* loss_kind 0: CE mean, 1: CE sum, 2: sum of squared logits.  grads == NULL => forward + loss only
 * (validation / test).  stats as in clhip_softmax_ce.
 * Small classifiers (Linear-ReLU-Linear-ReLU-Linear, hidden widths <= 128, <= 32 logits, no dropout inside) run
 * everything behind the first Linear layer's GEMM — split-K sum, Linear 2-3, the loss, backward-data down to the first
 * layer's output — as ONE launch, and the first layer's backward-data GEMM together with all Linear weight gradients as
 * another; results are bit-identical to the per-layer launches (CLHIP_FC_TAIL=0 at plan creation selects those).  The
 * fused launch keeps a 4-byte arrival counter in device memory owned by the plan: do not run ONE plan on two streams at
 * the same time (its activations live in one workspace, so that was never meaningful).                             */
int clhip_net_loss_step(void* handle, const float* params, float* grads, const float* x,
                        const int64_t* labels_i64, int N, int loss_kind, void* ws, float* loss_out,
                        double* stats, float* logits_out, void* stream);

/* cross-entropy over the class slice [col_off, col_off+ncols) of the shared head (ncols 0 => to the end) */
int clhip_net_loss_step_slice(void* handle, const float* params, float* grads, const float* x,
                              const int64_t* labels_i64, int N, int loss_kind, int col_off, int ncols, void* ws,
                              float* loss_out, double* stats, float* logits_out, void* stream);

/* ------------------------------------------------------------------ GEM memory gradients
 * rehearsal/model/gem.py:20-80,275-277.  G[n_tasks][ld]: one contiguous row per task.
 *   axpy        y = (assign ? 0 : y) + alpha*x : store_grad (:20-35) / accumulation over memory batches (:237-255)
 *   gem_gram    out_f64[m*m] = rows(row_idx) . rows(row_idx)^T in f64, one pass (the MM^T and M g of :70-73;
 *               its last row/column also carries the violation test g.G_tt of :275-277)
 *   gem_project out = g + sum_i v[i]*G[row_idx[i]]   (:79, written straight into the gradient arena = overwrite_grad) */
int clhip_axpy(float* y, const float* x, size_t n, float alpha, int assign, void* stream);
size_t clhip_gem_gram_ws(int m);
int clhip_gem_gram(const float* G, size_t ld, const int* row_idx_host, int m, size_t n, double* out_f64, void* ws,
                   size_t ws_bytes, void* stream);
int clhip_gem_project(const float* G, size_t ld, const int* row_idx_host, const float* v_host, int m, const float* g,
                      float* out, size_t n, void* stream);
/* project2cone2's QP itself (gem.py:58-80, quadprog.solve_qp = Goldfarb-Idnani dual active set) on the device, so that an
 * observe step never synchronises with the host:
 *   gem_qp          from clhip_gem_gram's f64 output over [memory rows..., current gradient LAST] (m rows, m - 1 <= 15
 *                   unknowns): P = 1/2 (MM^T + MM^T^T) + eps I, q = -M g, min 1/2 v^T P v - q^T v s.t. v >= margin;
 *                   v_out_f64[m - 1]; info_i32[0] = #{k : g . G_k < 0} (gem.py:275-277; 0 => v = 0), info_i32[1] = 0 ok,
 *                   1 iteration limit, 2 infeasible
 *   gem_project_dev clhip_gem_project with v and the violation count read from device memory: out = g when nothing is
 *                   violated (a no-op for out == g), else g + sum_i v[i] G[row_idx[i]]                                  */
int clhip_gem_qp(const double* gram_f64, int m, double margin, double eps, double* v_out_f64, int* info_i32, void* stream);
int clhip_gem_project_dev(const float* G, size_t ld, const int* row_idx_host, const double* v_dev_f64, const int* info_dev,
                          int m, const float* g, float* out, size_t n, void* stream);
/* The same four operations for task sequences of more than 16 tasks (GEM's own paper runs 20): up to CLHIP_GEM_WIDE_MAX rows
 * of a Gram matrix = 63 memory rows + the current gradient = CLHIP_MAX_TASKS tasks.  Semantics are those of the entries
 * above at every m in range, m <= 16 included (the Gram sums are added in another order there, so the two agree to the
 * f64 summation bound, not bit for bit); the entries above stay what a sequence of <= 16 tasks calls.
 *   gem_gram_wide    1 <= m <= 64.  The rows are cut into 16-row panels, every panel pair is one f64 matrix-core tile; f64
 *                    accumulation only, per-block tiles in ws (clhip_gem_gram_wide_ws(m) bytes, 0 for an m out of range), a
 *                    grid that depends on n alone and fixed-order sums: bitwise symmetric, and the same bits in every run.
 *                    Rows that are not selected and columns n .. ld-1 are never read.
 *   gem_qp_wide      2 <= m <= 64 (m - 1 <= 63 unknowns): the Goldfarb-Idnani steps and decisions of gem_qp on ONE workgroup,
 *                    matrices in LDS.  Same v_out_f64[m - 1] / info_i32[2] contract.  clhip_gem_qp_wide_ws(m) is 0 in this
 *                    build and ws may then be NULL; ws_bytes below what it reports is refused.
 *   gem_project_wide / gem_project_dev_wide    1 <= m <= 63 memory rows, the arithmetic of gem_project / gem_project_dev.   */
#define CLHIP_GEM_WIDE_MAX 64
size_t clhip_gem_gram_wide_ws(int m);
int clhip_gem_gram_wide(const float* G, size_t ld, const int* row_idx_host, int m, size_t n, double* out_f64, void* ws,
                        size_t ws_bytes, void* stream);
size_t clhip_gem_qp_wide_ws(int m);
int clhip_gem_qp_wide(const double* gram_f64, int m, double margin, double eps, double* v_out_f64, int* info_i32, void* ws,
                      size_t ws_bytes, void* stream);
int clhip_gem_project_wide(const float* G, size_t ld, const int* row_idx_host, const float* v_host, int m, const float* g,
                           float* out, size_t n, void* stream);
int clhip_gem_project_dev_wide(const float* G, size_t ld, const int* row_idx_host, const double* v_dev_f64, const int* info_dev,
                               int m, const float* g, float* out, size_t n, void* stream);

/* ------------------------------------------------------------------ rehearsal baselines
 * rehearsal/model/baseline_rehearsal_partial_mem.py:125-253 (observe_FT; full_mem.py is the same class): the reference runs
 * one forward / backward per exemplar chunk of every past task (:205-234) and one for the current batch (:238-247).
 * Without BatchNorm a sample's forward does not depend on the rest of the batch and the step's dropout mask rows are
 * shared by every pass (:97-111), so the step is ONE pass over [current batch | exemplar chunks] with per-row slices.
 *
 *   rehearsal_assemble  one launch, no allocation, no synchronisation; bitwise copies (16-byte vectors when row_elems % 4
 *                       == 0 and the tensors are 16-byte aligned):
 *                         x[0:B)                -> x_mix[0:B)                        (labels -> labels_mix)
 *                         x[0:ring_rows)        -> store rows [ring_row0, +ring_rows)  the ring-buffer update (:170-186)
 *                         store[gather_rows[e]] -> x_mix[B + e], e < E                the exemplar chunks (:214-234)
 *                       gather_rows (device int32[E]) hold store row indices of PAST tasks (never the ring rows).
 *                       store rows >= store_rows are not read (label -1).  B + ring_rows + E <= 65535.
 *   rehearsal_assemble_crop_flip  the same launch for a store of FRAMES [C][Hs][Ws] (the reference's memories hold paths and
 *                       every replay rebuilds the exemplar loader with the task's train transform, :215-216, gem.py:233-234, so
 *                       an exemplar gets a fresh RandomCrop + RandomHorizontalFlip at every draw); x and x_mix rows are
 *                       [C][th][tw]:
 *                         x[0:B)                          -> x_mix[0:B)                 (the loader already cropped them)
 *                         src_frames[src_idx[i]] (whole)  -> store rows [ring_row0, +ring_rows), labels_i64[i] -> store_labels
 *                         x_mix[B + e][c][y][x] = store[gather_rows[e]][c][top_e + y][left_e + (flip_e ? tw - 1 - x : x)]
 *                       src_frames: the loader's frame tensor (src_rows frames), src_idx device int64[ring_rows] the sample
 *                       numbers of the batch's first rows (the `paths` argument of the reference's observe); gather_params
 *                       device int32[E][3] of (top, left, flip) as in clhip_gather_tasks_crop_flip below.  A src_idx outside
 *                       [0, src_rows) leaves its store row untouched and writes store label -1; a gather row outside
 *                       [0, store_rows), top outside [0, Hs - th], left outside [0, Ws - tw] or flip outside {0, 1} copies
 *                       nothing and writes label -1; no address outside a frame is formed.  x_mix == NULL (E == 0 only): the
 *                       ring update alone, rows [0, B) are not copied (GEM's fill_buffer).  CLHIP_EINVAL before any launch:
 *                       the checks of clhip_rehearsal_assemble and of clhip_gather_tasks_crop_flip's geometry.  16-byte
 *                       copies of full rows / frames under the rule above; float4 stores of the cropped rows when
 *                       tw % 4 == 0 and x_mix is 16-byte aligned, loads at dword alignment.
 *   rehearsal_assemble_resized_crop_flip  rehearsal_assemble_crop_flip when the task's train transform is RandomResizedCrop +
 *                       RandomHorizontalFlip (data/tinyimgnet_dataprep.py:105-122): :215-216, gem.py:233-234 and common.py:57-72
 *                       rebuild the exemplar loader with THAT transform, so a replayed exemplar is a fresh resized window of
 *                       its stored frame.  Same arguments, same single launch (a 1-D grid of the copy rows, the ring rows and
 *                       the exemplar rows), same copy and ring rows; gather_params is device int32[E][5] of (top, left, h, w,
 *                       flip) and
 *                         x_mix[B + e] = the h x w window at (top, left) of store[gather_rows[e]], resized to th x tw and
 *                                        mirrored: the formula, taps and SUMMATION ORDER of clhip_gather_tasks_resized_crop_flip
 *                                        below, by the same device code
 *                       so the exemplar rows are BITWISE what that gather yields for a one-task table laid over the store,
 *                       idx = gather_rows and the same params, and a window with h == th and w == tw is bitwise
 *                       rehearsal_assemble_crop_flip for (top, left, flip).  The exemplar rows take E x C x chunks blocks
 *                       under that gather's plan for the frame, made once on the host; the launch carries the plan's dynamic LDS.
 *                       A src_idx outside [0, src_rows): as rehearsal_assemble_crop_flip.  An exemplar row copies nothing and
 *                       writes label -1 when its gather row is outside [0, store_rows), h < 1, w < 1, top < 0, left < 0,
 *                       top + h > Hs, left + w > Ws, flip is outside {0, 1}, or h > CLHIP_RESIZE_MAX_RATIO th or
 *                       w > CLHIP_RESIZE_MAX_RATIO tw (the gather's rule); no address outside a frame is formed.
 *                       CLHIP_EINVAL before any launch: the checks of clhip_rehearsal_assemble, and the geometry rule of
 *                       clhip_gather_tasks_resized_crop_flip (C, th, tw, Hs or Ws < 1; th > Hs is an enlargement, not an
 *                       error).  CLHIP_ENOTSUP before any launch: E > 0 and the plan does not fit the LDS (as that gather:
 *                       1000 -> 125 is not served).  With E == 0 (the ring update alone, x_mix == NULL allowed) no plan is
 *                       needed and CLHIP_ENOTSUP is never returned.  float4 stores of the exemplar rows when tw % 4 == 0 and
 *                       x_mix is 16-byte aligned, dword loads of the frames.
 *   rehearsal_assemble_pad_crop_flip  rehearsal_assemble_crop_flip when the task's train transform is torchvision's
 *                       RandomCrop(size, padding, fill, padding_mode) + RandomHorizontalFlip (the CIFAR-style rule, see
 *                       clhip_gather_tasks_pad_crop_flip below): the store holds the UNPADDED frames and a replayed exemplar is a
 *                       fresh window of its padded frame.  Same single launch (a 1-D grid of the copy rows, the ring rows and
 *                       the exemplar rows), same copy and ring rows; mode, (pl, pt, pr, pb) and fill (device float[C], output
 *                       domain) as in that gather, gather_params is device int32[E][5] of (top, left, flip, h, w), that
 *                       gather's row: the corner in the frame's unpadded coordinates, (h, w) the stored frame's valid extent, and
 *                         x_mix[B + e][c][y][x] = P(c, top + y, left + (flip ? tw - 1 - x : x))
 *                       with P the padded image of store[gather_rows[e]] as that gather defines it, by the same device code
 *                       (E x C x ceil(th / clhip_crop_rows_per_block(tw)) blocks): the exemplar rows are BITWISE what that
 *                       gather yields for a one-task table laid over the store, idx = gather_rows and the same params, and with
 *                       all pads 0 and full extents the whole launch is bitwise rehearsal_assemble_crop_flip.
 *                       A src_idx outside [0, src_rows): as rehearsal_assemble_crop_flip.  An exemplar row copies nothing and
 *                       writes label -1 when its gather row is outside [0, store_rows), flip is outside {0, 1}, h is outside
 *                       [1, Hs] or w outside [1, Ws], top is outside [-pt, h + pb - th] or left outside [-pl, w + pr - tw], or the
 *                       pads exceed the mode's limit for (h, w) (reflect: extent - 1, symmetric: extent); no address outside a
 *                       stored frame's h x w extent is formed in any mode.  CLHIP_EINVAL before any launch: the checks of
 *                       clhip_rehearsal_assemble_crop_flip except th > Hs and tw > Ws (the padded image may hold the crop), and
 *                       mode outside 0..3, a pad < 0 or > CLHIP_PAD_MAX, Hs or Ws > CLHIP_PAD_MAX_EXTENT, fill == NULL with
 *                       E > 0.  The ring-only form (x_mix == NULL, E == 0) needs no fill.  float4 stores of the exemplar rows
 *                       when tw % 4 == 0 and x_mix is 16-byte aligned; dword-aligned loads, 4 columns one wide load only when all
 *                       4 lie inside [0, w).
 *   loss_segments      segs (device, n_segs <= CLHIP_LOSS_MAX_SEGS) cover rows of logits[N][ld], N <= CLHIP_LOSS_MAX_ROWS, each
 *                       with a class slice [col_off, col_off + ncols), a scale and a kind:
 *                         kind 0  scale * mean_i CE_i over the slice against labels (relative to the slice)
 *                         kind 1  scale * T^2 * KLDiv_batchmean(log_softmax(z / T), softmax(target / T)) over the slice,
 *                                 target = targets[row][ld_t] (same row numbers as logits; targets may be NULL when no
 *                                 segment is of kind 1); a segment whose OWN value is negative (rounding, icarl.py:584-587)
 *                                 adds nothing and gets zero gradient, decided on the device.
 *                       loss = sum of the segments' values; dlogits[i] = its gradient inside the slice (kind 0: scale_g / |g|
 *                       * (softmax - onehot)), 0 outside and 0 for rows of no segment; stats[0] += loss, stats[1] += #hits
 *                       of segment 0 (arg-max, lowest index on ties).  Fixed summation order, f64 sums.  A malformed
 *                       segment or a label outside its slice makes the loss NaN.  A row that lies in several segments
 *                       (no caller produces one) counts for the first of them only.
 *                       Rehearsal baselines: every kind 0, segment 0 = the current batch with scale 1, chunk c of `count`
 *                       chunks with scale 1 / count: new_task_loss + sum_c CE_mean(c) / count (:236, :248).  iCaRL: segment 0
 *                       the current batch, every distillation chunk of kind 1 (update_representation, icarl.py:482-598).
 *   net_loss_step_loss_segments  per-layer forward (every layer, no fused tail) + loss_segments + backward in one call: the
 *                       whole step of a plan without BatchNorm.                                                         */
#define CLHIP_LOSS_MAX_ROWS 1024
#define CLHIP_LOSS_MAX_SEGS 256
typedef struct clhip_loss_segment { int row_begin; int row_end; int col_off; int ncols; float scale; int kind; } clhip_loss_segment;
int clhip_rehearsal_assemble(const float* x, const int64_t* labels_i64, int B, size_t row_elems, float* store_x,
                             int64_t* store_labels, long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                             int E, float* x_mix, int64_t* labels_mix, void* stream);
int clhip_rehearsal_assemble_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                       const float* src_frames, long src_rows, const int64_t* src_idx, float* store_frames,
                                       int64_t* store_labels, long store_rows, long ring_row0, int ring_rows,
                                       const int* gather_rows, const int* gather_params, int E, float* x_mix, int64_t* labels_mix,
                                       void* stream);
int clhip_rehearsal_assemble_resized_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                               int tw, const float* src_frames, long src_rows, const int64_t* src_idx,
                                               float* store_frames, int64_t* store_labels, long store_rows, long ring_row0,
                                               int ring_rows, const int* gather_rows, const int* gather_params, int E, float* x_mix,
                                               int64_t* labels_mix, void* stream);
int clhip_rehearsal_assemble_pad_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                           int mode, int pl, int pt, int pr, int pb, const float* fill, const float* src_frames,
                                           long src_rows, const int64_t* src_idx, float* store_frames, int64_t* store_labels,
                                           long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                                           const int* gather_params, int E, float* x_mix, int64_t* labels_mix, void* stream);
int clhip_loss_segments(const float* logits, const int64_t* labels_i64, const float* targets, int ld_t, int N, int ld,
                        const clhip_loss_segment* segs, int n_segs, float T, float* dlogits, float* loss_out, double* stats,
                        void* stream);
int clhip_net_loss_step_loss_segments(void* handle, const float* params, float* grads, const float* x,
                                      const int64_t* labels_i64, const float* targets, int ld_t, int N,
                                      const clhip_loss_segment* segs, int n_segs, float T, void* ws, float* loss_out,
                                      double* stats, float* logits_out, void* stream);

/* ------------------------------------------------------------------ Joint baseline
 * methods/method.py:1185-1235: one model trained on all tasks at once, one shared output layer, each task scored on its
 * own slice of that layer.
 *
 *   gather_tasks        a batch out of T <= CLHIP_MAX_TASKS per-task tensors WITHOUT a merged copy of the sequence
 *                       (data/imgfolder.py:244-272 ConcatDatasetDynamicLabels): tasks_dev is a DEVICE table, cum_rows the
 *                       cumulative sample counts, label_shift the class counts of the tasks before.  idx (device int64[B],
 *                       B <= 65535) holds GLOBAL sample numbers; number g belongs to the first task whose cum_rows exceeds
 *                       it.  x_out[b] = the row (bitwise; 16-byte vectors when row_elems % 4 == 0 and both rows are
 *                       16-byte aligned, scalar otherwise), labels_out[b] = label + label_shift.  A number outside
 *                       [0, cum_rows[T-1]) copies nothing and writes label -1: callers check the numbers on the host.
 *   slice_argmax_count  framework/inference.py:141-149 for one batch in one launch: row i's prediction is the position k of
 *                       the largest logits[i][cols[k]], k < K (cols: device int32[K], any order, not necessarily
 *                       contiguous; the first NaN wins, lowest k on ties — torch.max on the CPU); for a label y in [0, K)
 *                       total[y] += 1 and correct[y] += (prediction == y), integer atomics: the result does not depend on
 *                       order.  A label outside [0, K) (the reference stops with IndexError there) or a column outside
 *                       [0, ld) adds 1 to *out_of_range and nothing else for that row.  Counters accumulate over calls. */
#define CLHIP_MAX_TASKS 64
typedef struct clhip_task_src { const float* x; const int64_t* labels; int64_t cum_rows; int64_t label_shift; } clhip_task_src;
int clhip_gather_tasks(const clhip_task_src* tasks_dev, int T, size_t row_elems, const int64_t* idx, int B, float* x_out,
                       int64_t* labels_out, void* stream);
int clhip_slice_argmax_count(const float* logits, int N, int ld, const int* cols, int K, const int64_t* labels_i64,
                             int64_t* correct, int64_t* total, int64_t* out_of_range, void* stream);

/* ------------------------------------------------------------------ training augmentation of the task loaders
 * data/recogseq_dataprep.py:53-60 (the `train` split of every RecogSeq task: Resize(256) -> RandomCrop(224) ->
 * RandomHorizontalFlip -> ToTensor -> Normalize) and data/inaturalist_dataprep.py:232-253 (get_rnd_transforms, the file
 * methods/method.py:1204 asks for): crop and flip of the stored, already normalised Resize(256) frames.  Normalize is a
 * per-channel affine map and commutes with both, so the result is bitwise what that pipeline yields for the same draws.
 *
 *   gather_tasks_crop_flip   clhip_gather_tasks with one (top, left, flip) per batch position: the rows of the task table are
 *                            frames [C][Hs][Ws], params is device int32[B][3], x_out is [B][C][th][tw] and
 *                              x_out[b][c][y][x] = frame(idx[b])[c][top_b + y][left_b + (flip_b ? tw - 1 - x : x)]
 *                            (torchvision's crop, then hflip), labels_out[b] = label + label_shift.  A sample number outside
 *                            [0, cum_rows[T-1]), top outside [0, Hs - th], left outside [0, Ws - tw] or flip outside {0, 1}
 *                            copies nothing for that row and writes label -1; no address outside the source frame is formed.
 *                            Callers draw and check the table on the host.  CLHIP_EINVAL before any launch: the checks of
 *                            clhip_gather_tasks, C < 1, th or tw < 1, th > Hs, tw > Ws.  B == 0 returns 0.  float4 stores
 *                            when tw % 4 == 0 and x_out is 16-byte aligned; loads assume dword alignment only (a line starts anywhere). */
int clhip_gather_tasks_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const int64_t* idx,
                                 const int* params, int B, float* x_out, int64_t* labels_out, void* stream);

/* data/tinyimgnet_dataprep.py:105-122 (the `train` split of the cropped Tiny-ImageNet variant: RandomResizedCrop(56) ->
 * RandomHorizontalFlip -> ToTensor -> Normalize on 64 x 64 images; also the standard ImageNet training augmentation).
 *
 *   gather_tasks_resized_crop_flip   clhip_gather_tasks_crop_flip with a window that is RESIZED: params is device int32[B][5] of
 *                            (top, left, h, w, flip), the h x w window of the stored frame [C][Hs][Ws] whose top-left corner is
 *                            (top, left); x_out is [B][C][th][tw] and
 *                              x_out[b][c][y][x] = sum_j sum_i Wy[y][j] Wx[x'][i] frame(idx[b])[c][top + j][left + i]
 *                              x' = flip ? tw - 1 - x : x                 (torchvision's crop, resize, then hflip)
 *                            W is the antialiased bilinear filter of torchvision's tensor resized_crop(antialias=True), ATen's
 *                            _upsample_bilinear2d_aa with align_corners = False.  Per axis, n_in the window's and n_out the
 *                            output's extent:
 *                              scale = n_in / n_out     sup = max(scale, 1)     c = scale (i_out + 0.5)
 *                              lo = max(0, int(c - sup + 0.5))     hi = min(n_in, int(c + sup + 0.5))
 *                              w_j = max(0, 1 - |(j - c + 0.5) / sup|) for j in [lo, hi), normalised to sum 1
 *                            at most ceil(2 sup) + 1 taps.  The weights are computed on the device in fp32 from the integers.
 *                            Summation order (fixed: two runs are bitwise equal): the horizontal pass first, one fp32 value per
 *                            (source line, output column), then the vertical pass; each accumulates by fp32 fused multiply-add
 *                            over its taps in ascending source index, starting from -0.0f, and skips a tap whose weight is
 *                            exactly 0.  A window with h == th and w == tw has one tap of weight exactly 1 per axis: the result
 *                            is then bitwise that of clhip_gather_tasks_crop_flip for (top, left, flip).
 *                            Difference from the reference: PIL resizes the uint8 image and rounds to uint8 before Normalize;
 *                            here the stored normalised floats are resampled, so a value can differ by up to half a grey level
 *                            divided by the channel's std (0.5 / 255 / std).
 *                            A row copies nothing and writes label -1 when its sample number is outside [0, cum_rows[T-1]),
 *                            h < 1, w < 1, top < 0, left < 0, top + h > Hs, left + w > Ws, flip is outside {0, 1}, or
 *                            h > CLHIP_RESIZE_MAX_RATIO th or w > CLHIP_RESIZE_MAX_RATIO tw; no address outside the source
 *                            frame is formed.  CLHIP_EINVAL before any launch: the checks of clhip_gather_tasks_crop_flip
 *                            except th > Hs and tw > Ws (a window may be enlarged: 5 x 7 -> 8 x 8), and Hs < 1 or Ws < 1.
 *                            CLHIP_ENOTSUP: the source band of ONE output line at the largest window the frame allows, with
 *                            s = min(Hs / th, CLHIP_RESIZE_MAX_RATIO) about 2 max(s, 1) + 3 lines of
 *                            min(Ws, CLHIP_RESIZE_MAX_RATIO tw) + tw floats, and the tap tables do not fit 64 KB of LDS (the plan is
 *                            made for the frame, not for the windows of one batch): 512 -> 64 is served, 1000 -> 125 is not.
 *                            B == 0 returns 0.  float4 stores when tw % 4 == 0 and x_out is 16-byte aligned; dword loads.
 * CLHIP_RESIZE_MAX_RATIO: the largest supported shrink ratio max(h / th, w / tw) of a window (17 taps per axis; 64 -> 8 and
 * 256 -> 56 with room).  It bounds the LDS a block needs for its source band and its tap tables. */
#define CLHIP_RESIZE_MAX_RATIO 8
int clhip_gather_tasks_resized_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw,
                                         const int64_t* idx, const int* params, int B, float* x_out, int64_t* labels_out,
                                         void* stream);

/* torchvision's RandomCrop(size, padding, fill, padding_mode) -> RandomHorizontalFlip: the standard augmentation of the
 * CIFAR-style split benchmarks (RandomCrop(32, padding = 4) + flip), and the only translation jitter for frames already at the
 * net's input size.  The reference's own Composes do not pad (data/recogseq_dataprep.py:56-57 and
 * data/inaturalist_dataprep.py:240-241 crop a LARGER Resize(256) frame); with it a task file stores frames of the output size
 * and no margin.  It replaces F.pad of the whole task tensor on the host followed by clhip_gather_tasks_crop_flip.
 *
 *   gather_tasks_pad_crop_flip   clhip_gather_tasks_crop_flip over the PADDED image of each sample.  params is device
 *                            int32[B][5] of (top, left, flip, h, w): (h, w) the valid extent of the sample inside its stored
 *                            frame [C][Hs][Ws] (top-left anchored), (top, left) the window's corner in the sample's UNPADDED
 *                            coordinates, top in [-pt, h + pb - th] and left in [-pl, w + pr - tw] (uniform over the padded
 *                            image of (h + pt + pb) x (w + pl + pr), RandomCrop.get_params; th > Hs is legal when the padded
 *                            image holds it).  x_out is [B][C][th][tw] and
 *                              x_out[b][c][y][x] = P(c, top + y, left + (flip ? tw - 1 - x : x))      (pad, crop, then hflip)
 *                              P(c, i, j) = frame(idx[b])[c][m(i, h)][m(j, w)], or fill[c] where a map says so
 *                            m(s, n) = s inside [0, n), otherwise by mode:
 *                              0 constant   nowhere: the element is fill[c], nothing is loaded
 *                              1 edge       clamp(s, 0, n - 1)
 *                              2 reflect    -s below 0, 2 (n - 1) - s at or above n     [1,2,3,4], pad 2 -> [3,2,1,2,3,4,3,2]
 *                              3 symmetric  -s - 1 below 0, 2 n - 1 - s at or above n                    -> [2,1,1,2,3,4,4,3]
 *                            fill is device float[C] in the OUTPUT domain (the stored, normalised values), read in every mode.
 *                            A copy: bitwise.  A row copies nothing and writes label -1 when its sample number is outside
 *                            [0, cum_rows[T-1]), flip is outside {0, 1}, h is outside [1, Hs] or w outside [1, Ws], top or
 *                            left is outside its range above, or the pads exceed the mode's limit for (h, w) (reflect: every
 *                            pad <= extent - 1 on its axis, symmetric: <= extent, as torch; one reflection then suffices).
 *                            No address outside the sample's h x w extent is formed in any mode.  Callers draw and check the
 *                            table on the host.  CLHIP_EINVAL before any launch: the checks of clhip_gather_tasks, fill ==
 *                            NULL, C, Hs, Ws, th or tw < 1, Hs or Ws > CLHIP_PAD_MAX_EXTENT, mode outside 0..3, a pad < 0 or
 *                            > CLHIP_PAD_MAX.  B == 0 returns 0.  Grid, lines per block (clhip_crop_rows_per_block) and
 *                            stores as clhip_gather_tasks_crop_flip: float4 stores when tw % 4 == 0 and x_out is 16-byte
 *                            aligned, dword-aligned loads; 4 columns are one wide load only when all 4 lie inside [0, w).
 *   gather_tasks_pad_crop_flip_u8   the same for byte frames (the byte-frames section below): the frame's bytes are decoded
 *                            through the device table lut (fp32 [C][256], NULL is CLHIP_EINVAL), staged per channel in LDS;
 *                            fill STAYS float[C] in the output domain (callers pass lut[c][fill byte of c]), so the result is
 *                            bitwise the fp32 entry's on the decoded frames.  Byte loads, one dword load per 4 interior columns
 *                            only behind a test of that address. */
#define CLHIP_PAD_MAX 32767
#define CLHIP_PAD_MAX_EXTENT (1 << 30)
int clhip_gather_tasks_pad_crop_flip(const clhip_task_src* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, int mode, int pl,
                                     int pt, int pr, int pb, const float* fill, const int64_t* idx, const int* params, int B,
                                     float* x_out, int64_t* labels_out, void* stream);

/* Host read-outs of the launch plans of the window entries (the gathers above, clhip_rehearsal_assemble_*crop_flip*,
 * clhip_icarl_assemble_*crop_flip*); nothing is launched and no device is needed.  Test infrastructure: a test asserts through
 * them that a geometry still splits a channel plane into the blocks it was chosen for.
 *   resized_crop_plan     the plan every resized entry makes for frames Hs x Ws resized to th x tw (byte_frames != 0: the _u8
 *                         entries, whose blocks also hold a 1024-byte table): out7 = {rpb, chunks, nb, wmax, ktx, kty, lds_bytes}
 *                         = output lines per block, blocks per channel plane (chunks rpb >= th > (chunks - 1) rpb), the source
 *                         lines and the line width the block's LDS band holds, the taps per axis at the largest window, and the
 *                         dynamic LDS of a block (at most 48 KB, up to 64 KB only with rpb == 1).  Returns 0; CLHIP_ENOTSUP
 *                         where the entries return it (no plan; out7 is not written); CLHIP_EINVAL for an argument < 1 or
 *                         out7 == NULL.
 *   crop_rows_per_block   the output lines per block of every crop + flip entry for output width tw (blocks per channel plane:
 *                         ceil(th / that)); CLHIP_EINVAL for tw < 1. */
int clhip_resized_crop_plan(int Hs, int Ws, int th, int tw, int byte_frames, int* out7);
int clhip_crop_rows_per_block(int tw);

/* ------------------------------------------------------------------ byte frames
 * ToTensor -> Normalize, the last step of every Compose of the reference (data/recogseq_dataprep.py:53-60,
 * data/inaturalist_dataprep.py:232-277, data/tinyimgnet_dataprep.py:105-122), done inside the gathers: the task tensors hold the
 * decoded images as uint8 [n][C][H][W], a quarter of the bytes in HBM and on every gather's source side.
 *
 * MEANING.  A byte dataset is its frames plus per-channel mean and std (fp32 [C], std > 0).  It means the fp32 dataset of
 * lut[c][x], lut a [C][256] fp32 table the HOST computes once with torch on the CPU, op for op as ToTensor then Normalize do:
 *     lut[c][v] = (float(v) / 255 - mean[c]) / std[c]          (fp32: convert, div, sub, div)
 * The device never does this arithmetic: it looks the byte up.  So each entry below yields, BITWISE, what its fp32 sibling
 * yields on the decoded frames for the same idx / params; crop, flip and the antialiased resize act on the decoded values
 * exactly as the fp32 kernels do (the stated difference to PIL's uint8 rounding in the resized case is unchanged).
 *
 * The task table keeps its layout (clhip_task_src_u8 differs from clhip_task_src only in the type x points to); every entry
 * takes the DEVICE table `lut` (fp32 [C][256]) after the geometry.
 *
 *   gather_tasks_u8     clhip_gather_tasks for byte rows [C][plane_elems] (row_elems = C plane_elems):
 *                         x_out[b][e] = lut[(e / plane_elems) % C][row(idx[b])[e]]
 *                       bad rows and labels as clhip_gather_tasks.  CLHIP_EINVAL before any launch: its checks, lut == NULL,
 *                       C < 1, plane_elems < 1.  B == 0 returns 0.  float4 stores when row_elems % 4 == 0 and the destination
 *                       row is 16-byte aligned, plain stores otherwise.  Source: a row of odd size starts at any byte, so the
 *                       baseline is byte loads; the 4 bytes of a float4 are one dword load only when the source row's address
 *                       was TESTED to be a multiple of 4.  The table is read through the cache (a 16 KB output segment may
 *                       cross any number of channel planes).
 *   gather_tasks_crop_flip_u8   clhip_gather_tasks_crop_flip for byte frames, same geometry and (top, left, flip) table:
 *                         x_out[b][c][y][x] = lut[c][frame(idx[b])[c][top_b + y][left_b + (flip_b ? tw - 1 - x : x)]]
 *                       Same bad rows (nothing copied, label -1, no address outside the frame formed), same CLHIP_EINVAL
 *                       checks plus lut == NULL.  float4 stores when tw % 4 == 0 and x_out is 16-byte aligned; byte loads,
 *                       one dword load per 4 columns only behind a test of that address.  The block's channel of the table
 *                       is staged in LDS (1 KB).
 *   gather_tasks_resized_crop_flip_u8   clhip_gather_tasks_resized_crop_flip for byte frames, same geometry, (top, left, h, w,
 *                       flip) table, plan, taps, summation order and stores: the bytes are decoded through the block's channel
 *                       of the table (staged in LDS; the plan counts its 1 KB) while the source band is staged, everything
 *                       after is the fp32 entry's code.  Same bad rows, CLHIP_EINVAL checks plus lut == NULL, CLHIP_ENOTSUP
 *                       as there (with the table's 1 KB counted).  Byte loads.
 *   rehearsal_assemble_crop_flip_u8   clhip_rehearsal_assemble_crop_flip for a store of BYTE frames: src_frames and store_frames
 *                       are uint8 [rows][C][Hs][Ws], x and x_mix stay fp32 [C][th][tw] (the loader decoded the current batch):
 *                         x[0:B)                          -> x_mix[0:B)
 *                         src_frames[src_idx[i]] (whole)  -> store rows [ring_row0, +ring_rows), the C Hs Ws bytes as they are
 *                         x_mix[B + e][c][y][x] = lut[c][store[gather_rows[e]][c][top_e + y][left_e + (flip_e ? tw - 1 - x : x)]]
 *                       Bitwise the fp32 entry on the decoded store, and the stored bytes are bitwise those of the source
 *                       frames: one table (one mean / std) decodes a store.  Same bad rows (nothing copied, label -1, no
 *                       address outside a frame formed), same labels, same x_mix == NULL form, same CLHIP_EINVAL checks, plus
 *                       lut == NULL with E > 0 (a ring-only call decodes nothing and may pass NULL).  Ring rows: 48 KB
 *                       segments; 16-byte accesses only when C Hs Ws % 16 == 0 and both frame tensors are 16-byte aligned (a
 *                       frame of odd size starts at any byte), byte accesses otherwise.  Exemplar rows: as
 *                       gather_tasks_crop_flip_u8 (float4 stores when tw % 4 == 0 and x_mix is 16-byte aligned; byte loads, one
 *                       dword load per 4 columns only behind a test of that address; the block's channel of the table staged in
 *                       LDS, 1 KB).
 *   rehearsal_assemble_resized_crop_flip_u8   clhip_rehearsal_assemble_resized_crop_flip for a store of BYTE frames: frames, ring
 *                       rows and the lut rule (NULL allowed with E == 0) as rehearsal_assemble_crop_flip_u8, (top, left, h, w,
 *                       flip) rows, bad rows, CLHIP_EINVAL and CLHIP_ENOTSUP (the table's 1 KB counted in the plan) as the fp32
 *                       entry.  The bytes of the source band are decoded through the block's channel of the table as they are
 *                       staged, everything after is the fp32 code: bitwise the fp32 entry on the decoded store, and bitwise
 *                       clhip_gather_tasks_resized_crop_flip_u8 over the store.  Byte loads of the frames.
 *   rehearsal_assemble_pad_crop_flip_u8   clhip_rehearsal_assemble_pad_crop_flip for a store of BYTE frames: frames, ring rows
 *                       and the lut rule (NULL is CLHIP_EINVAL only with E > 0) as rehearsal_assemble_crop_flip_u8; mode, pads,
 *                       (top, left, flip, h, w) rows, bad rows and CLHIP_EINVAL as the fp32 entry.  fill STAYS float[C] in the
 *                       output domain (callers pass lut[c][fill byte of c]); the block's channel of the table is staged in LDS as
 *                       257 entries, the last one fill[c], and the bytes are decoded where they are loaded, as
 *                       gather_tasks_pad_crop_flip_u8 does: bitwise the fp32 entry on the decoded store, and bitwise that gather
 *                       over the store. */
typedef struct clhip_task_src_u8 { const uint8_t* x; const int64_t* labels; int64_t cum_rows; int64_t label_shift; } clhip_task_src_u8;
int clhip_gather_tasks_u8(const clhip_task_src_u8* tasks_dev, int T, int C, size_t plane_elems, const float* lut,
                          const int64_t* idx, int B, float* x_out, int64_t* labels_out, void* stream);
int clhip_gather_tasks_crop_flip_u8(const clhip_task_src_u8* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, const float* lut,
                                    const int64_t* idx, const int* params, int B, float* x_out, int64_t* labels_out, void* stream);
int clhip_gather_tasks_resized_crop_flip_u8(const clhip_task_src_u8* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw,
                                            const float* lut, const int64_t* idx, const int* params, int B, float* x_out,
                                            int64_t* labels_out, void* stream);
/* (documented with clhip_gather_tasks_pad_crop_flip above) */
int clhip_gather_tasks_pad_crop_flip_u8(const clhip_task_src_u8* tasks_dev, int T, int C, int Hs, int Ws, int th, int tw, int mode,
                                        int pl, int pt, int pr, int pb, const float* fill, const float* lut, const int64_t* idx,
                                        const int* params, int B, float* x_out, int64_t* labels_out, void* stream);
int clhip_rehearsal_assemble_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                          const float* lut, const uint8_t* src_frames, long src_rows, const int64_t* src_idx,
                                          uint8_t* store_frames, int64_t* store_labels, long store_rows, long ring_row0,
                                          int ring_rows, const int* gather_rows, const int* gather_params, int E, float* x_mix,
                                          int64_t* labels_mix, void* stream);
int clhip_rehearsal_assemble_resized_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                                  int tw, const float* lut, const uint8_t* src_frames, long src_rows,
                                                  const int64_t* src_idx, uint8_t* store_frames, int64_t* store_labels,
                                                  long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                                                  const int* gather_params, int E, float* x_mix, int64_t* labels_mix,
                                                  void* stream);
int clhip_rehearsal_assemble_pad_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                              int tw, int mode, int pl, int pt, int pr, int pb, const float* fill, const float* lut,
                                              const uint8_t* src_frames, long src_rows, const int64_t* src_idx,
                                              uint8_t* store_frames, int64_t* store_labels, long store_rows, long ring_row0,
                                              int ring_rows, const int* gather_rows, const int* gather_params, int E, float* x_mix,
                                              int64_t* labels_mix, void* stream);

/* ------------------------------------------------------------------ iCaRL
 * rehearsal/model/icarl.py: exemplar herding (manage_memory :384-471) and the nearest-mean-of-exemplars classifier of
 * Net.forward (:142-186); the loss of update_representation (:482-598) over one mixed batch is clhip_loss_segments above.
 *
 *   icarl_herd          the prioritised exemplar lists of ALL classes of a task in one launch, one workgroup per class,
 *                       over features computed ONCE (the reference recomputes them K (n/B + 1) times per class).
 *                       feats[n_rows][F] fp32 (device), w[n_rows] the per-row mean weights (device), classes_host: HOST table
 *                       of n_classes <= CLHIP_ICARL_MAX_CLASSES row ranges (checked here, passed by value): class c owns
 *                       rows [row_begin, row_end) (at most CLHIP_ICARL_MAX_CLASS_ROWS), picks k <= rows of them and writes
 *                       ranking[out_off .. out_off + k) (device int32, row numbers RELATIVE to row_begin).
 *                       mu = sum_i w_i f_i (f64 sums).  Pick k = the row not yet taken with the smallest
 *                       || mu - (f_i + S_k) / (k + 1) ||, S_k the fp32 sum of the features already chosen; evaluated as
 *                       || r - f_i ||, r = (k + 1) mu - S_k (the same quantity times k + 1: no Gram matrix, no expanded
 *                       square), differences in fp32, squares summed in f64; the lowest row wins a tie.
 *                       F <= CLHIP_ICARL_MAX_FEATS (mu, S and r live in LDS).
 *   icarl_herd_wide     the same table, launch shape and result for F <= CLHIP_ICARL_MAX_FEATS_WIDE (deep_VGG22 at 64x64,
 *                       the widest classifier input of the model table): one pick-loop body serves both entries, so the
 *                       rankings are equal bit for bit wherever both accept F.  Only r, the vector the pick loop reads, and
 *                       the taken bits are in LDS (72 KB, static); mu and S live in ws, fp32 [n_classes][2][F] in device
 *                       memory, touched once per pick by the thread that wrote them.  ws_bytes >=
 *                       clhip_icarl_herd_wide_ws(n_classes, F) = n_classes * 2 * F * 4 bytes exactly (no rounding; 0 for an
 *                       n_classes or F outside the limits); ws == NULL or too small is CLHIP_EINVAL, as every other refusal,
 *                       before any launch.  Launches on one stream may share ws.
 *   icarl_nme          out[N][n_outputs] = 0, and 1 at offset1 + argmin_c || means[c] - feats[i] || (c < C, the first
 *                       minimum wins; squares summed in f64, distances compared in fp32).  means == NULL: the task has no
 *                       exemplars yet, out = -10e10 everywhere and 1 / C inside [offset1, offset1 + C) (:146-155).        */
#define CLHIP_ICARL_MAX_CLASSES 128
#define CLHIP_ICARL_MAX_FEATS 4096
#define CLHIP_ICARL_MAX_FEATS_WIDE 16384
#define CLHIP_ICARL_MAX_CLASS_ROWS 65536
typedef struct clhip_icarl_class { int row_begin; int row_end; int k; int out_off; } clhip_icarl_class;
int clhip_icarl_herd(const float* feats, long n_rows, int F, const float* w, const clhip_icarl_class* classes_host,
                     int n_classes, int* ranking, long ranking_len, void* stream);
size_t clhip_icarl_herd_wide_ws(int n_classes, int F);
int clhip_icarl_herd_wide(const float* feats, long n_rows, int F, const float* w, const clhip_icarl_class* classes_host,
                          int n_classes, int* ranking, long ranking_len, void* ws, size_t ws_bytes, void* stream);
int clhip_icarl_nme(const float* feats, const float* means, int N, int F, int C, int offset1, int n_outputs, float* out,
                    void* stream);

/* iCaRL on augmented tasks: the assembly of one update_representation step when the store holds FRAMES.  The reference's
 * memory holds paths; every step rebuilds the exemplar loader with the task's train transform (icarl.py:560-561), so a
 * replayed exemplar is a fresh crop, while its distillation target is the row computed once at herding time (:476-479,
 * mem_class_y, read back at :566-574).
 *
 *   icarl_assemble_crop_flip   ONE launch fills the mixed batch of the step: a 1-D grid of three runs of blocks,
 *                         B x row_blocks     x[r] -> x_mix[r], labels[r] -> labels_mix[r]                  (48 KB segments)
 *                         E x crop_blocks    the th x tw window at (top, left) of store_frames[gather_rows[e]] [C][Hs][Ws],
 *                                            mirrored when flip, -> x_mix[B + e];  labels_mix[B + e] = 0   (a distillation
 *                                            row has no label: the segmented loss reads its target row)
 *                         target blocks      store_t[gather_rows[e]][0 .. n_outputs) -> t_mix[B + e][0 .. n_outputs)
 *                       gather_params: device int32[E][3] of (top, left, flip).  The window is copied by the block body of
 *                       clhip_gather_tasks_crop_flip / clhip_rehearsal_assemble_crop_flip (bitwise their result); the target
 *                       rows move in 16-byte accesses when n_outputs % 4 == 0 and store_t and t_mix are 16-byte aligned, as
 *                       floats otherwise; the copy run as clhip_rehearsal_assemble_crop_flip's.  It replaces the two launches
 *                       of the crop-mode step (clhip_rehearsal_assemble over the images, again over the target rows).
 *                       B == 0 is the cropping of stored frames alone (x, labels may be NULL); E == 0 the copy alone
 *                       (everything of the store may be NULL); B == 0 and E == 0 returns 0 at once.
 *                       A gather row outside [0, store_rows), top outside [0, Hs - th], left outside [0, Ws - tw] or flip
 *                       outside {0, 1} copies nothing, neither window nor target row, and writes label -1; no address outside
 *                       a frame or a target row is formed.
 *                       CLHIP_EINVAL before any launch: a negative B, E or store_rows; C, Hs, Ws, th, tw or n_outputs < 1;
 *                       th > Hs or tw > Ws; B > 0 without x, labels, x_mix or labels_mix; E > 0 without store_frames,
 *                       gather_rows, gather_params, store_t, x_mix, labels_mix or t_mix; B + E > 65535.
 *   icarl_assemble_resized_crop_flip   the same under RandomResizedCrop + flip: gather_params int32[E][5] of (top, left, h, w,
 *                       flip), the window resampled to th x tw by the block body of clhip_gather_tasks_resized_crop_flip under a
 *                       plan made for the frame (bitwise that gather's result).  A window may be enlarged (th > Hs is allowed).
 *                       Bad rows: that gather's rule (h or w < 1, a window outside the frame, flip outside {0, 1}, h >
 *                       CLHIP_RESIZE_MAX_RATIO th or w > CLHIP_RESIZE_MAX_RATIO tw), treated as above.  CLHIP_ENOTSUP: E > 0 and
 *                       no plan fits the LDS (clhip_gather_tasks_resized_crop_flip's limit).
 *   ..._u8              store_frames holds BYTE frames (byte frames, above): a stored byte v of channel c means lut[c][v]
 *                       (device float32 [C][256], staged per block in LDS), decoded where the window is loaded: bitwise the
 *                       fp32 entry on the decoded store.  lut may be NULL with E == 0, CLHIP_EINVAL otherwise.
 *   icarl_assemble_pad_crop_flip   the same under RandomCrop(size, padding, fill, padding_mode) + flip, the CIFAR-style train
 *                       transform (datasets/dataset_utils.py; rebuilt for the exemplar loader at icarl.py:560-561): the store
 *                       holds the UNPADDED frames and a replayed exemplar is a fresh window of its padded frame.  Same launch
 *                       shape and the same copy and target runs; mode, (pl, pt, pr, pb) and fill (device float[C], output
 *                       domain) as clhip_gather_tasks_pad_crop_flip takes them, gather_params int32[E][5] of (top, left, flip,
 *                       h, w), that gather's row: the corner in the frame's unpadded coordinates, (h, w) the frame's valid
 *                       extent.  The window is copied by the block body of clhip_gather_tasks_pad_crop_flip /
 *                       clhip_rehearsal_assemble_pad_crop_flip (bitwise their result), and with all pads 0 and full extents
 *                       the whole launch is bitwise icarl_assemble_crop_flip.
 *                       Bad rows: clhip_rehearsal_assemble_pad_crop_flip's rule (a gather row outside [0, store_rows), flip
 *                       outside {0, 1}, h outside [1, Hs] or w outside [1, Ws], top outside [-pt, h + pb - th] or left outside
 *                       [-pl, w + pr - tw], pads over the mode's limit for (h, w): reflect extent - 1, symmetric extent),
 *                       treated as above: neither window nor target row, label -1, no address formed from the row.
 *                       CLHIP_EINVAL before any launch: the checks of icarl_assemble_crop_flip except th > Hs and tw > Ws
 *                       (the padded image may hold the crop), and mode outside 0..3, a pad < 0 or > CLHIP_PAD_MAX, Hs or Ws >
 *                       CLHIP_PAD_MAX_EXTENT, fill == NULL with E > 0.  The _u8 form takes lut after fill; entry 256 of the
 *                       staged table is the decoded fill.                                                              */
int clhip_icarl_assemble_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                   const float* store_frames, long store_rows, const int* gather_rows, const int* gather_params,
                                   int E, const float* store_t, int n_outputs, float* x_mix, int64_t* labels_mix, float* t_mix,
                                   void* stream);
int clhip_icarl_assemble_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                      const float* lut, const uint8_t* store_frames, long store_rows, const int* gather_rows,
                                      const int* gather_params, int E, const float* store_t, int n_outputs, float* x_mix,
                                      int64_t* labels_mix, float* t_mix, void* stream);
int clhip_icarl_assemble_resized_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                           const float* store_frames, long store_rows, const int* gather_rows,
                                           const int* gather_params, int E, const float* store_t, int n_outputs, float* x_mix,
                                           int64_t* labels_mix, float* t_mix, void* stream);
int clhip_icarl_assemble_resized_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                              int tw, const float* lut, const uint8_t* store_frames, long store_rows,
                                              const int* gather_rows, const int* gather_params, int E, const float* store_t,
                                              int n_outputs, float* x_mix, int64_t* labels_mix, float* t_mix, void* stream);
int clhip_icarl_assemble_pad_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                       int mode, int pl, int pt, int pr, int pb, const float* fill, const float* store_frames,
                                       long store_rows, const int* gather_rows, const int* gather_params, int E,
                                       const float* store_t, int n_outputs, float* x_mix, int64_t* labels_mix, float* t_mix,
                                       void* stream);
int clhip_icarl_assemble_pad_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                          int mode, int pl, int pt, int pr, int pb, const float* fill, const float* lut,
                                          const uint8_t* store_frames, long store_rows, const int* gather_rows,
                                          const int* gather_params, int E, const float* store_t, int n_outputs, float* x_mix,
                                          int64_t* labels_mix, float* t_mix, void* stream);

#ifdef CLHIP_VISIBILITY_PUSHED
#pragma GCC visibility pop
#undef CLHIP_VISIBILITY_PUSHED
#endif

#ifdef __cplusplus
}
#endif
#endif /* CLHIP_H */
