/*
 * sequitr_hip.h -- C-ABI of libsequitr_hip.so, the MI355X (gfx950) back end of
 * the sequitr per-tile network hot path.
 *
 * The reference has NO FFI: its leaf operators are Python hooks
 * on the UNet class (sequitr/networks/unet.py:326-343) and module-level
 * functions in sequitr/networks/gan.py:44-136 that call TensorFlow.  Each entry
 * point below names the hook / function whose arithmetic it replaces; the
 * Python side that binds them with ctypes is sequitr_amd/_lib.py +
 * sequitr_amd/ops.py, and INTEGRATION.md shows the stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every function returns int: 0 = ok, negative = SQ_E*; sq_last_error()
 *     returns a thread-local message for the last failure on this thread;
 *   - all tensor pointers are DEVICE pointers (e.g. torch.Tensor.data_ptr());
 *     the caller owns every byte, kernels never allocate;
 *   - layout is NHWC, weights HWIO (kh,kw,Cin,Cout), transpose-conv weights in
 *     TensorFlow's (kh,kw,Cout,Cin);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     launches are asynchronous and graph-capturable (no sync, no malloc);
 *   - no global mutable state: one host thread per GPU process may call in.
 *
 * Numerics contract for the f32 entry points: every
 * convolution output is one f32 fmaf chain from +0, reduction order
 * (16-channel chunk, tap, channel), then "+ bias" (one rounding), then the
 * activation.  oracle/sq_oracle.c restates it; parity is bit-exact.
 */
#ifndef SEQUITR_HIP_H
#define SEQUITR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQ_OK 0
#define SQ_EINVAL (-1)   /* bad shape / null pointer / unsupported combination */
#define SQ_ELAUNCH (-2)  /* HIP reported a launch error */
#define SQ_EALIGN (-3)   /* pointer not 16-byte aligned */

/* activations */
#define SQ_ACT_NONE 0
#define SQ_ACT_RELU 1    /* UNet._activation, sequitr/networks/unet.py:142 */
#define SQ_ACT_LEAKY 2   /* k_leaky_relu_alpha, alpha 0.2, sequitr/networks/gan.py:44-46 */

/* bridges, sequitr/networks/unet.py:42,190-200 (up-scaled operand first) */
#define SQ_BRIDGE_NONE 0
#define SQ_BRIDGE_ADD 1
#define SQ_BRIDGE_MUL 2
#define SQ_BRIDGE_SUB 3

int sq_version(void);
const char *sq_last_error(void);

/*
 * conv_layer / conv_layer_1x1 hooks (sequitr/networks/unet.py:326-333) and
 * weighted_conv2d / to_image / from_image (sequitr/networks/gan.py:61-125).
 * KxK (K = 1 or 3) SAME stride-1 convolution + bias + activation.
 *   x (N,H,W,Cin)  w (K,K,Cin,Cout)  bias (Cout) or NULL  y (N,H,W,Cout)
 * wscale: runtime equalised-LR scale, w' = fl(w*wscale) (gan.py:75-79); 1.0f for the U-Net.
 * Supported: Cin in 1..8 or Cin % 16 == 0; Cout % 4 == 0, or Cout <= 7 with K == 1 and Cin % 4 == 0.
 */
int sq_conv2d_nhwc_fwd_f32(const float *x, const float *w, const float *bias, float *y,
                           int N, int H, int W, int Cin, int Cout, int K,
                           float wscale, int act, void *stream);

/*
 * max_pool_layer / pool_layer hook (sequitr/networks/unet.py:242,340-342):
 * 2x2 stride-2 VALID max pooling.  x (N,H,W,C) -> y (N,H/2,W/2,C); H,W even, C % 4 == 0.
 */
int sq_maxpool2x2_fwd_f32(const float *x, float *y, int N, int H, int W, int C, void *stream);

/* tf.layers.average_pooling2d(2,2) in the discriminator (sequitr/networks/gan.py:189-192). */
int sq_avgpool2x2_fwd_f32(const float *x, float *y, int N, int H, int W, int C, void *stream);

/*
 * conv_transpose_layer hook (sequitr/networks/unet.py:336-338) fused with the
 * bridge of up_layer (unet.py:312-319): 2x2 stride-2 transpose convolution +
 * bias, then bridge(upscale, skip).
 *   x (N,H,W,Cin)  w (2,2,Cout,Cin)  bias (Cout) or NULL
 *   skip (N,2H,2W,Cout) or NULL when bridge == SQ_BRIDGE_NONE   y (N,2H,2W,Cout)
 * Cin % 16 == 0, Cout % 4 == 0.
 */
int sq_convT2x2s2_nhwc_fwd_f32(const float *x, const float *w, const float *bias,
                               const float *skip, float *y, int N, int H, int W,
                               int Cin, int Cout, int bridge, void *stream);

/* UNet.bridge as a stand-alone op (sequitr/networks/unet.py:190-200), y = a (op) b, n elements, n % 4 == 0. */
int sq_bridge_fwd_f32(const float *a, const float *b, float *y, int64_t n, int bridge, void *stream);

/*
 * to_image head of UNet.build (sequitr/networks/unet.py:252-253) fused with the
 * prediction argmax: 1x1 conv Cin -> Cout (Cout <= 7) writes f32 logits and the
 * uint8 class mask (ties -> lowest index) in one pass.  mask may be NULL.
 */
int sq_conv1x1_argmax_fwd_f32(const float *x, const float *w, const float *bias,
                              float *logits, uint8_t *mask, int N, int H, int W,
                              int Cin, int Cout, void *stream);

/* argmax over the channel axis of (npix, C) f32 logits -> uint8, ties -> lowest index. */
int sq_argmax_u8(const float *logits, uint8_t *mask, int64_t npix, int C, void *stream);

/* pixel_norm (sequitr/networks/gan.py:49-51): y = x * rsqrt(mean_c(x^2) + eps). C % 4 == 0. */
int sq_pixelnorm_fwd_f32(const float *x, float *y, int64_t npix, int C, float eps, void *stream);

/* double_size (sequitr/networks/gan.py:133-136): nearest-neighbour 2x up-sampling. C % 4 == 0. */
int sq_upsample_nn2x_f32(const float *x, float *y, int N, int H, int W, int C, void *stream);

/*
 * Weighted softmax cross-entropy, forward + backward in one pass (SURVEY.md A.3;
 * tensor contract sequitr/networks/unet.py:395-401).
 *   logits (npix,C) f32, onehot (npix,C) u8, weights (npix) f32
 *   partials: workspace of sq_wsoftmax_ce_partials(npix) doubles (block sums, fixed order)
 *   loss: 1 double on the device = sum(partials)/npix, written by a second tiny kernel
 *   dlogits (npix,C) f32 or NULL:  w_p (softmax_c * sum(y) - y_c) * grad_scale / npix
 */
int64_t sq_wsoftmax_ce_partials(int64_t npix);
int sq_wsoftmax_ce_fwd_bwd_f32(const float *logits, const uint8_t *onehot, const float *weights,
                               int64_t npix, int C, float grad_scale, double *partials,
                               double *loss, float *dlogits, void *stream);

/* ------------------------------------------------------------------------------------------
 * Training side.  The reference trains through TensorFlow's automatic differentiation of the
 * same graph (sequitr/networks/gan.py:721,740-751; the U-Net model_fn is absent);
 * these entry points are the hand-written gradients of the forward operators above.
 * Gradient reductions use fixed-order two-stage sums (no float atomics): reproducible.
 * ---------------------------------------------------------------------------------------- */

/* dgrad filter: wt[ky][kx][co][ci] = w[K-1-ky][K-1-kx][ci][co]; then
 * dX = sq_conv2d_nhwc_fwd_f32(dY, wt, NULL, ..., Cin := Cout, Cout := Cin, act NONE). */
int sq_conv_weight_transform_f32(const float *w, float *wt, int K, int Cin, int Cout, void *stream);

/* dW (K,K,Cin,Cout) and db (Cout, may be NULL) of the KxK SAME convolution from X (N,H,W,Cin)
 * and dY (N,H,W,Cout).  Cin in 1..7 (K=3 only), 8, or Cin % 16 == 0; Cout % 4 == 0.
 * workspace: sq_conv2d_nhwc_wgrad_workspace_f32(...) bytes (returns -1 for unsupported shapes). */
int64_t sq_conv2d_nhwc_wgrad_workspace_f32(int N, int H, int W, int Cin, int Cout, int K);
int sq_conv2d_nhwc_wgrad_f32(const float *x, const float *dy, float *dw, float *db, float *workspace,
                             int N, int H, int W, int Cin, int Cout, int K, void *stream);

/* d(pre-activation) = dY * act'(.), decided from the activation OUTPUT y (y > 0 <=> pre > 0). */
int sq_act_bwd_f32(const float *dy, const float *y, float *dx, int64_t n, int act, void *stream);

/* max-pool backward: gradient to the first maximum in raster order; x (N,H,W,C) is the pool input. */
int sq_maxpool2x2_bwd_f32(const float *x, const float *dy, float *dx, int N, int H, int W, int C, void *stream);

/* dst (N,H,W,C) = scale * src (N,H/2,W/2,C) broadcast over 2x2: avg-pool backward (scale 0.25)
 * and double_size forward (scale 1).  sq_sumpool2x2: y = scale * sum of each 2x2 patch (double_size
 * backward).  Any C (2-channel images take a scalar path). */
int sq_broadcast2x2_f32(const float *src, float *dst, int N, int H, int W, int C, float scale, void *stream);
int sq_sumpool2x2_f32(const float *x, float *y, int N, int H, int W, int C, float scale, void *stream);

/* bridge backward: (da, db) from dY and the forward operands a (up-scaled) and b (skip).  n % 4 == 0; dy, da, db 16-byte
 * aligned.  a, b are read by eltwise_mul only (may be NULL otherwise) and must then be 16-byte aligned too. */
int sq_bridge_bwd_f32(const float *dy, const float *a, const float *b, float *da, float *db, int64_t n,
                      int bridge, void *stream);

/* g[n,i,j,(2a+b)*C+c] = dy[n,2i+a,2j+b,c]: makes the 2x2/s2 transpose-conv backward two 1x1 convs. */
int sq_space_to_depth2_f32(const float *dy, float *g, int N, int H, int W, int C, void *stream);

/* to_image head backward (1x1 conv, Cin in {8,16,32}, Cout <= 4): dx (may be NULL), dw (Cin,Cout), db. */
int64_t sq_conv1x1_small_bwd_workspace_f32(int64_t npix, int Cin, int Cout);
int sq_conv1x1_small_bwd_f32(const float *x, const float *w, const float *dz, float *dx, float *dw, float *db,
                             float *workspace, int64_t npix, int Cin, int Cout, void *stream);

/* tf.layers.dropout (sequitr/networks/unet.py:274-276): y = x * keep / (1 - rate).  mask (u8, n) is
 * written from a counter-based hash of (seed, index), or read when mask_given != 0.  step_dev (may be
 * NULL): device int32 whose value is folded into the seed, so a captured hipGraph draws a new mask on
 * every replay.  n % 4 == 0, rate in [0,1); x, y, dy, dx 16-byte aligned, mask 4-byte aligned (four bytes per access). */
int sq_dropout_fwd_f32(const float *x, float *y, uint8_t *mask, int64_t n, float rate, uint32_t seed,
                       int mask_given, const int32_t *step_dev, void *stream);
int sq_dropout_bwd_f32(const float *dy, const uint8_t *mask, float *dx, int64_t n, float rate, void *stream);

/* tf.train.AdamOptimizer update over a flat parameter buffer (sequitr/networks/gan.py:736-751):
 * g is first multiplied by grad_scale (1/world for data-parallel averaging); step counts from 1. */
int sq_adam_step_f32(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1,
                     float beta2, float eps, int step, float grad_scale, void *stream);
/* y += alpha * x (flat fp32): accumulates the gradient bucket over the micro-batches of one optimiser step when a
 * rank's share of the global batch is larger than one launch batch (BASELINE config 4 on fewer than 8 GPUs). */
int sq_axpy_f32(float *y, const float *x, float alpha, int64_t n, void *stream);
/* hipGraph-safe form: state = 2 x int32 in device memory {step counter, lr_t bits}; the call increments
 * the counter on the device, so a captured step replays with the right bias correction. */
int sq_adam_step_dev_f32(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1,
                         float beta2, float eps, int32_t *state, float grad_scale, void *stream);
/* its two halves, for optimisers with per-variable slots (the GAN's two AdamOptimizers, gan.py:736-751): one advance
 * of {step, lr_t} per minimize(), then one apply per tensor reading it. */
int sq_adam_advance_dev(int32_t *state, float lr, float beta1, float beta2, void *stream);
/* the same advance with a linear learning-rate warm-up evaluated ON THE DEVICE from the step counter:
 * lr_t = lr * min(1, t / warmup_steps) * sqrt(1 - beta2^t) / (1 - beta1^t); warmup_steps = 0 is sq_adam_advance_dev.
 * A captured training step walks the schedule by itself when replayed (the U-Net trainer's default: the reference's
 * learning_rate 0.01, sequitr/utils.py:289, diverges on step 2 of the 5-level net without it -- HISTORY.md section 8). */
int sq_adam_advance_warmup_dev(int32_t *state, float lr, float beta1, float beta2, int warmup_steps, void *stream);
int sq_adam_apply_dev_f32(float *p, const float *g, float *m, float *v, int64_t n, float beta1, float beta2,
                          float eps, const int32_t *state, float grad_scale, void *stream);
/* the same apply over a list of tensors in ONE launch: table (device memory, 8-byte aligned) = n_entries x
 * {p, g, m, v, element count, first chunk} as 64-bit words, chunks of sq_adam_multi_chunk() elements numbered across
 * the entries, total_chunks of them; element for element the update of sq_adam_apply_dev_f32 */
int sq_adam_multi_chunk(void);
int sq_adam_apply_multi_dev_f32(const void *table, int n_entries, int64_t total_chunks, float beta1, float beta2, float eps,
                                const int32_t *state, float grad_scale, void *stream);

/* conv_transpose_layer with a 3x3 kernel (SURVEY.md A.1 `up_kernel` = (3,3); hook at
 * sequitr/networks/unet.py:336-338): TF's conv2d_transpose(k=3, s=2, SAME) equals a SAME 3x3
 * convolution (sq_conv2d_nhwc_fwd_f32, filter = sq_conv_weight_transform_f32 of the TF (3,3,Cout,Cin)
 * kernel) of the zero-inserted input u[n,2i+1,2j+1,:] = x[n,i,j,:].  H, W are the SMALL side; C % 4 == 0.
 * sq_gather_odd2x_f32 is the adjoint (dx[n,i,j,:] = du[n,2i+1,2j+1,:]). */
int sq_zero_insert2x_f32(const float *x, float *u, int N, int H, int W, int C, void *stream);
int sq_gather_odd2x_f32(const float *du, float *dx, int N, int H, int W, int C, void *stream);

/* ------------------------------------------------------------------------------------------
 * Batch normalisation between a convolution and its activation: the optional `batch_norm` of the
 * conv_layer hook (sequitr/networks/unet.py:326-328 leaves the layer abstract; SURVEY.md A.1 pins
 * tf.layers.batch_normalization defaults: epsilon 1e-3, momentum 0.99).  x (npix, C) NHWC-flat,
 * C % 4 == 0, C <= 1024.  workspace: sq_bn_workspace_f32 bytes, 8-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_bn_workspace_f32(int64_t npix, int C);
/* batch mean and POPULATION variance per channel (tf.nn.moments); fp64 fixed-order accumulation */
int sq_bn_stats_f32(const float *x, float *mean, float *var, void *workspace, int64_t npix, int C, void *stream);
/* scale = gamma / sqrtf(var + eps), shift = fmaf(-mean, scale, beta)  (batch or moving statistics) */
int sq_bn_fold_f32(const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                   float *scale, float *shift, int C, void *stream);
/* moving -= (moving - batch) * (1 - momentum); the variance enters with Bessel's correction
 * npix/(npix-1) as TF's fused kernel does */
int sq_bn_update_moving_f32(float *moving_mean, float *moving_var, const float *mean, const float *var,
                            float momentum, int64_t npix, int C, void *stream);
/* y = act(fmaf(x, scale[c], shift[c])) */
int sq_bn_apply_f32(const float *x, const float *scale, const float *shift, float *y, int64_t npix, int C, int act,
                    void *stream);
/* gradients of y = act(BN(x)) given dy: the activation is differentiated through y_act (= y; NULL when
 * act == SQ_ACT_NONE); dx (npix,C), dgamma (C), dbeta (C). */
int sq_bn_bwd_f32(const float *x, const float *dy, const float *y_act, int act, const float *mean, const float *var,
                  const float *gamma, float eps, float *dx, float *dgamma, float *dbeta, void *workspace,
                  int64_t npix, int C, void *stream);
/* The same three passes on bf16 tensors (`batch_norm` in the bf16 training graph, BASELINE configs 3-4; hook
 * sequitr/networks/unet.py:326-328 + SURVEY.md A.1): elements are widened to f32, statistics accumulate in f64, parameters
 * and gradients of gamma / beta stay f32, y / dx are rounded to bf16 once.  fold / update_moving are the f32 entry points;
 * workspace as sq_bn_workspace_f32. */
int sq_bn_stats_bf16(const void *x, float *mean, float *var, void *workspace, int64_t npix, int C, void *stream);
int sq_bn_apply_bf16(const void *x, const float *scale, const float *shift, void *y, int64_t npix, int C, int act,
                     void *stream);
int sq_bn_bwd_bf16(const void *x, const void *dy, const void *y_act, int act, const float *mean, const float *var,
                   const float *gamma, float eps, void *dx, float *dgamma, float *dbeta, void *workspace, int64_t npix,
                   int C, void *stream);

/* ------------------------------------------------------------------------------------------
 * GAN side (sequitr/networks/gan.py).  weighted_conv2d / to_image / from_image are
 * sq_conv2d_nhwc_fwd_f32 with wscale + act; the entries below are the remaining leaf ops, their
 * gradients and the second-order pieces the WGAN-GP penalty needs (gan.py:719-729).
 * ---------------------------------------------------------------------------------------- */

/* pixel_norm gradients (gan.py:49-51): bwd: dx from (x, dy); bwd2: with v = dL/d(dx) returns
 * dg = dL/d(dy) and dx2 = dL/dx through the backward expression. */
int sq_pixelnorm_bwd_f32(const float *x, const float *dy, float *dx, int64_t npix, int C, float eps, void *stream);
int sq_pixelnorm_bwd2_f32(const float *x, const float *g, const float *v, float *dg, float *dx2, int64_t npix,
                          int C, float eps, void *stream);
/* pixel_norm backward + the backward of the activation that produced x (conv -> leaky -> pixel_norm, gan.py:90-98) in
 * one pass: dx = act'(x) * pixelnorm_bwd(x, dy) */
int sq_pixelnorm_bwd_act_f32(const float *x, const float *dy, float *dx, int64_t npix, int C, float eps, int act,
                             void *stream);
/* avg-pool backward (scale * 2x nearest up-sampling of src (N,H/2,W/2,C)) + the backward of the activation whose
 * output is `gate` (N,H,W,C): the discriminator block's conv2 -> leaky -> avg-pool tail (gan.py:171-192) */
int sq_broadcast2x2_act_bwd_f32(const float *src, const float *gate, float *dst, int N, int H, int W, int C, float scale,
                                int act, void *stream);

/* half_size / any tf.image.resize_nearest_neighbor(align_corners=True) (gan.py:128-136). */
int sq_resize_nearest_f32(const float *x, float *y, int N, int Hi, int Wi, int Ho, int Wo, int C, void *stream);

/* y = alpha*a + (1-alpha)*b: fade-in (gan.py:687-694, scalar alpha) and the real/fake interpolation
 * (gan.py:709-714, alpha_per_sample (N) != NULL, per_sample = elements per sample). */
int sq_lerp_f32(const float *a, const float *b, float *y, int64_t n, int64_t per_sample, float alpha,
                const float *alpha_per_sample, void *stream);
/* y = k*x, k = s or s_per_sample[n] (or 1-k when one_minus): the gradients of sq_lerp_f32. */
int sq_scale_f32(const float *x, float *y, int64_t n, int64_t per_sample, float s, const float *s_per_sample,
                 int one_minus, void *stream);

/* stand-alone activation (k_leaky_relu_alpha, gan.py:44-46) */
int sq_act_fwd_f32(const float *x, float *y, int64_t n, int act, void *stream);

/* out[n] = sum_i a[n,i]*b[n,i] (b == a: squared gradient norm of gan.py:722); fixed-order two-stage sum. */
int64_t sq_dot_per_sample_workspace_f32(int N);
int sq_dot_per_sample_f32(const float *a, const float *b, float *out, float *workspace, int N, int64_t per_sample,
                          void *stream);

/* minibatch stdev scalar (gan.py:204-211): sqrt(mean over positions of the batch variance).
 * workspace: 256 floats. */
int sq_mbstd_fwd_f32(const float *x, float *out, float *workspace, int N, int64_t per_sample, void *stream);
/* The discriminator's minibatch-stdev FEATURE MAP (gan.py:204-212) up to second order (two launches per call):
 * x (groups*n, per_sample) -> y (groups*n, cells) filled with its group's statistic (cells = 16: the hard-coded
 * (N,4,4,1) map); bwd: dx from (x, dy); bwd2: with v = dL/d(dx) returns ddy = dL/d(dy) and dx2 = dL/dx.  groups = 2
 * when D(Gz) and D(X) run as one stacked pass (each minibatch its own statistic). */
int64_t sq_mbstd_map_workspace(int groups);      /* bytes of the `workspace` the three calls take */
int sq_mbstd_map_fwd_f32(const float *x, float *y, float *workspace, int groups, int n, int64_t per_sample, int cells,
                         void *stream);
int sq_mbstd_map_bwd_f32(const float *x, const float *dy, float *dx, float *workspace, int groups, int n,
                         int64_t per_sample, int cells, void *stream);
int sq_mbstd_map_bwd2_f32(const float *x, const float *dy, const float *v, float *ddy, float *dx2, float *workspace,
                          int groups, int n, int64_t per_sample, int cells, void *stream);
/* the same three with the feature tensors (x, v, dx, dx2) in bf16 storage -- f32 arithmetic, results rounded once; y, dy, ddy f32 */
int sq_mbstd_map_fwd_bf16(const void *x, float *y, float *workspace, int groups, int n, int64_t per_sample, int cells, void *stream);
int sq_mbstd_map_bwd_bf16(const void *x, const float *dy, void *dx, float *workspace, int groups, int n, int64_t per_sample,
                          int cells, void *stream);
int sq_mbstd_map_bwd2_bf16(const void *x, const float *dy, const void *v, float *ddy, void *dx2, float *workspace, int groups,
                           int n, int64_t per_sample, int cells, void *stream);
/* WGAN-GP loss algebra of gan.py:715-729 in one launch: out2 = {d_loss, g_loss} from Dz, Dx (N) and gn2 (N) = squared
 * norm of dD(mix)/dmix per sample (one-sided penalty, lambda 10, eps drift 0.001 Dx^2); Dx = gn2 = NULL: g_loss only.
 * bwd: g_dloss / g_gloss = upstream gradients (device scalars, NULL = 0) -> dDz, dDx, dgn2. */
int sq_wgan_losses_fwd_f32(const float *Dz, const float *Dx, const float *gn2, float *out2, int N, void *stream);
int sq_wgan_losses_bwd_f32(const float *Dz, const float *Dx, const float *gn2, const float *g_dloss, const float *g_gloss,
                           float *dDz, float *dDx, float *dgn2, int N, void *stream);

/* Small-image batches (the 4x4 / 8x8 levels of generator_network / discriminator_network,
 * gan.py:246-316,149-240) as ONE image of R x Cc cells of pitch (H+1, W+1): m (1, R*(H+1), Cc*(W+1), C),
 * image n at cell (n / Cc, n % Cc), a zero row and column after every image = the SAME padding.  A KxK
 * (K <= 3) SAME convolution of m equals the per-image convolutions on the image cells, bit for bit. */
int sq_mosaic_pack_f32(const float *x, float *m, int N, int H, int W, int C, int R, int Cc, void *stream);
int sq_mosaic_unpack_f32(const float *m, float *y, int N, int H, int W, int C, int R, int Cc, void *stream);

/* tf.layers.dense with a long reduction and few rows (discriminator_network, gan.py:226-237: 8208 -> 512 on
 * 32..96 samples): y (M,N) = act(x (M,K) @ fl(w (K,N) * wscale) + bias), the reduction split into 64-wide
 * slices over thread blocks and the slices added in order (deterministic; not the convolution's single
 * chain).  K % 4 == 0; workspace sq_dense_workspace_f32 bytes. */
int64_t sq_dense_workspace_f32(int M, int K, int N);
int sq_dense_fwd_f32(const float *x, const float *w, const float *bias, float *y, float *workspace, int M, int K, int N,
                     float wscale, int act, void *stream);
/* its weight gradient: dW (K,N) = scale * x^T dY, db (N) or NULL = column sums of dY; x (M,K), dY (M,N), M <= 128 rows.
 * accumulate: bit 0 -- dW is added to the contents of dw, bit 1 -- db to those of db. */
int sq_dense_wgrad_f32(const float *x, const float *dy, float *dw, float *db, int M, int K, int N, float scale, int accumulate,
                       void *stream);

/* M (Ca,Cb) = sum_p a[p,:]^T b[p,:] with Ca <= 7, Cb % 4 == 0: weight gradient of to_image / from_image. */
int64_t sq_wgrad1x1_small_workspace_f32(int64_t npix, int Ca, int Cb);
int sq_wgrad1x1_small_f32(const float *a, const float *b, float *m, float *workspace, int64_t npix, int Ca, int Cb,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused inference variants of the 3x3 convolution (bit-identical to the unfused sequence).
 * ---------------------------------------------------------------------------------------- */

/* conv_layer on the concat bridge (sequitr/networks/unet.py:196-197, 321): y = act(conv(concat([xa, xb], -1)) + bias);
 * xa, xb (N,H,W,Ca) each (the up-scaled tensor first, the skip tensor second), w (K,K,2*Ca,Cout); the concatenated
 * tensor is never written.  Bit-identical to sq_conv2d_nhwc_fwd_f32 on the materialised concat. */
int sq_conv2d_concat_nhwc_fwd_f32(const float *xa, const float *xb, const float *w, const float *bias, float *y, int N,
                                  int H, int W, int Ca, int Cout, int K, int act, void *stream);

/* conv_block tail + max_pool_layer (sequitr/networks/unet.py:241-243,265-277): 3x3 conv + bias + act
 * that writes y (N,H,W,Cout) AND its 2x2 max-pool (N,H/2,W/2,Cout) from the same accumulators. */
int sq_conv3x3_pool_fwd_f32(const float *x, const float *w, const float *bias, float *y, float *pooled,
                            int N, int H, int W, int Cin, int Cout, int act, void *stream);

/* Fragment-order filter pack of an inference model's 3x3 layers on 64-channel blocks, made ONCE per model: a pure permutation
 * of the stored (3,3,Cin,Cout) weights (bits in, bits out; no scaling, no rounding).  For each (64-channel output block cb,
 * 16-channel chunk c, tap, 4-channel k-step s) it holds the 64 lanes' four A operands of one v_mfma_f32_16x16x4_f32 step as one
 * float4 per lane:  wp[((((cb * Cin/16 + c) * 9 + tap) * 4 + s) * 64 + 16 kk + li) * 4 + nb]
 *                   = w[tap][16 c + 4 s + kk][64 cb + 16 nb + li]        (li 0..15, kk 0..3, nb 0..3)
 * -- value for value what the unpacked kernel re-stages through LDS for every (tile, chunk).  Eligible: K == 3, Cin % 16 == 0,
 * Cout % 64 == 0; sq_conv_packed_filter_elems_f32 gives the element count 9 Cin Cout (-1: not eligible).
 * sq_conv2d_packed_nhwc_fwd_f32 / sq_conv3x3_pool_packed_fwd_f32 are sq_conv2d_nhwc_fwd_f32 / sq_conv3x3_pool_fwd_f32 with the
 * pack of `w` beside it (wp, or NULL): same bits.  The packed kernel (one barrier per item, halo double-buffered, A operands
 * from the pack through a register ring) runs where sq_conv_packed_takes_f32 says 1: wp given, wscale == 1, the pack eligible
 * the plan on 64-channel blocks (sq_conv_plan) and every tensor below 2 GiB, switch SQ_CONV_PACKED (0: never; read per call).  It walks the grid of the
 * unpacked 64-channel form, so sq_conv_walk_plan describes it too.  Everything else runs the unpacked entry point on w.
 * The caller keeps wp current: it is a function of w's contents at pack time. */
int64_t sq_conv_packed_filter_elems_f32(int K, int Cin, int Cout);
int sq_conv_pack_filter_f32(const float *w, float *wp, int K, int Cin, int Cout, void *stream);
int sq_conv_packed_takes_f32(int N, int H, int W, int Cin, int Cout, int K);
int sq_conv2d_packed_nhwc_fwd_f32(const float *x, const float *w, const float *wp, const float *bias, float *y, int N, int H,
                                  int W, int Cin, int Cout, int K, float wscale, int act, void *stream);
int sq_conv3x3_pool_packed_fwd_f32(const float *x, const float *w, const float *wp, const float *bias, float *y, float *pooled,
                                   int N, int H, int W, int Cin, int Cout, int act, void *stream);

/* Does sq_conv2d_nhwc_fwd_f32 (pooled = 0) / sq_conv3x3_pool_fwd_f32 (pooled = 1) at wscale == 1 run the 32 -> 32 kernel with the
 * filter held in registers (conv_r32_kernel) at this shape?  1 where K == 3, Cin == Cout == 32, act == SQ_ACT_RELU, H and W
 * multiples of 16, every tensor below 2 GiB, and the plan is the 32-channel block with 32 staged channels (sq_conv_plan: at
 * least 512 pixel tiles); switch SQ_CONV_R32 (0: never; read per call).  Same bits as the generic kernel, whose grid it walks
 * (sq_conv_walk_plan describes both).  Host only, no HIP call. */
int sq_conv_r32_takes_f32(int N, int H, int W, int Cin, int Cout, int K, int act, int pooled);

/* last conv_layer of up0 + conv_layer_1x1 + prediction (unet.py:252-253,321): 3x3 conv Cin -> 16
 * + bias + act, then the 1x1 head (16 -> head_c <= 4, HWIO head_w (1,1,16,head_c)) and the argmax
 * mask in the epilogue; the 16-channel activation never reaches HBM.  mask may be NULL. */
int sq_conv3x3_head_fwd_f32(const float *x, const float *w, const float *bias, const float *head_w,
                            const float *head_b, float *logits, uint8_t *mask, int N, int H, int W,
                            int Cin, int head_c, int act, void *stream);

/* conv_block of down0 for a 1-channel input (unet.py:238): conv1 (3x3, 1 -> 16, bias, ReLU) is
 * evaluated in LDS, conv2 (3x3, 16 -> 16, bias, ReLU) on the matrix cores; writes y (N,H,W,16) and,
 * when pooled != NULL, its 2x2 max-pool. */
int sq_conv3x3_first_block_fwd_f32(const float *x, const float *w1, const float *b1, const float *w2,
                                   const float *b2, float *y, float *pooled, int N, int H, int W,
                                   void *stream);

/* conv_transpose_layer + bridge + first conv_layer of up0 (unet.py:299-322) for the level-0 shape: the
 * transpose conv (32 -> 16 channels) and the bridge are evaluated for each tile's halo inside the 3x3
 * convolution's staging; the up-scaled / merged tensor never reaches HBM.
 *   x_low (N,H/2,W/2,32); wt (2,2,16,32) TF layout, bt (16) or NULL; skip (N,H,W,16); bridge SQ_BRIDGE_*;
 *   w (3,3,16,16), bias (16) or NULL; y (N,H,W,16) = act(conv3x3(bridge(convT(x_low) + bt, skip)) + bias).
 * Same bits as sq_convT2x2s2_nhwc_fwd_f32 followed by sq_conv2d_nhwc_fwd_f32. */
int sq_convT_conv3x3_fwd_f32(const float *x_low, const float *wt, const float *bt, const float *skip, int bridge,
                             const float *w, const float *bias, float *y, int N, int H, int W, int act, void *stream);

/* ------------------------------------------------------------------------------------------
 * bf16 path (BASELINE configs 3-5: bf16 compute, fp32 master weights and accumulation).
 * bf16 tensors are passed as void* (2-byte elements, NHWC); biases / logits / weight grads stay f32.
 * ---------------------------------------------------------------------------------------- */

/* Packed bf16 filter of the KxK conv Cin -> Cout: [Cin/KC][Cout][KP] with k = tap*KC + c, KC = 32 when
 * Cin % 32 == 0, 16 when Cin % 16 == 0, else 8 (Cin % 8 == 0); KP = K*K*KC rounded up to 32.
 * sq_conv_packed_weights_elems_bf16 gives the element count (-1: unsupported).  transform != 0 packs the dgrad filter of the forward conv
 * Cout -> Cin whose f32 HWIO weights (K,K,Cout,Cin) are passed in `w`. */
int64_t sq_conv_packed_weights_elems_bf16(int K, int Cin, int Cout);
int sq_conv_pack_weights_bf16(const float *w, void *wp, int K, int Cin, int Cout, float wscale, int transform,
                              void *stream);
/* Every pack (and plain f32 -> bf16 cast) of one optimiser step in one launch.  base: the flat fp32 parameter
 * buffer; out: one bf16 buffer; table (device, n_entries x 8 int32, n_entries <= 128):
 * {src offset in floats, dst offset in bf16 elements, K, Cin, Cout of the packed conv, transform, index of the
 * entry's first item, kind (0 = pack as sq_conv_pack_weights_bf16, 1 = plain cast of K*K*Cin*Cout values)};
 * total_items = sum of the entries' item counts (packed elements, or values for kind 1). */
int sq_conv_pack_weights_multi_bf16(const float *base, void *out, const int32_t *table, int n_entries,
                                    int total_items, void *stream);
/* the same with a factor per entry (`scales`, n_entries floats on the device) applied as sq_conv_pack_weights_bf16's
 * wscale: all filter packs of a GAN solver step in one launch */
int sq_conv_pack_weights_multi_scaled_bf16(const float *base, void *out, const int32_t *table, const float *scales,
                                           int n_entries, int total_items, void *stream);

/* conv_layer / weighted_conv2d on bf16 activations: y = act(conv(x, wp) + bias), fp32 accumulate. */
int sq_conv2d_nhwc_fwd_bf16(const void *x, const void *wp, const float *bias, void *y, int N, int H, int W,
                            int Cin, int Cout, int K, int act, void *stream);

/* "Mixed" convolution behind an f32 graph (the GAN of BASELINE config 5; weighted_conv2d, gan.py:61-99): f32
 * activations in and out, both operands rounded to bf16 (RNE) on the way into LDS, f32 accumulation on
 * v_mfma_f32_16x16x32_bf16.  wp = sq_conv_pack_weights_bf16(w, K, Cin, Cout, wscale, transform) (Cin % 8 == 0);
 * Cout % 4 == 0.  The drop-in for sq_conv2d_nhwc_fwd_f32 where the bf16 matrix rate is wanted. */
int sq_conv2d_nhwc_fwd_mixed_f32(const float *x, const void *wp, const float *bias, float *y, int N, int H, int W,
                                 int Cin, int Cout, int K, int act, void *stream);
/* dgrad of such a conv whose INPUT was the output `gate` (N,H,W,Cout) of a ReLU / leaky-ReLU (act): the result leaves through
 * that activation's backward in the epilogue, dx = gate > 0 ? v : v * slope -- the sq_act_bwd_f32 pass that followed the
 * dgrad in the GAN's first-order backward passes (gan.py:90-98 chains), same bits */
int sq_conv2d_nhwc_dgrad_actgate_mixed_f32(const float *dy, const void *wp_t, const float *gate, int act, float *dx, int N,
                                           int H, int W, int Cin, int Cout, int K, void *stream);
/* both forms on a batch of small images (Nimg, h, w, C) convolved as ONE mosaic image of R x Cc cells (sq_mosaic_pack_f32's
 * layout, 3x3 only) without building it: loads, gate and stores address the compact tensors.  gate == NULL: forward with
 * bias / act; gate != NULL: the act-gated dgrad (`act` = the gate's activation).  Same bits as pack -> conv -> unpack. */
int sq_conv2d_nhwc_mixed_mosaic_f32(const float *x, const void *wp, const float *bias, const float *gate, float *y, int Nimg,
                                    int h, int w, int Cin, int Cout, int act, int R, int Cc, void *stream);
/* its weight gradient: dW (K,K,Cin,Cout) f32, db (Cout) f32 or NULL from f32 X and f32 dY (rounded to bf16 in
 * LDS); Cin % 16 == 0, Cout % 16 == 0. */
int64_t sq_conv2d_nhwc_wgrad_workspace_mixed_f32(int N, int H, int W, int Cin, int Cout, int K);
int sq_conv2d_nhwc_wgrad_mixed_f32(const float *x, const float *dy, float *dw, float *db, float *workspace, int N,
                                   int H, int W, int Cin, int Cout, int K, void *stream);
/* the same with dW (not db) multiplied by dw_scale in the finish kernel: the gradient of an equalised-learning-rate
 * kernel is wscale * raw dW (gan.py:75-79); saves the scalar-multiply pass over every weight gradient */
int sq_conv2d_nhwc_wgrad_scaled_mixed_f32(const float *x, const float *dy, float *dw, float *db, float *workspace, int N,
                                          int H, int W, int Cin, int Cout, int K, float dw_scale, void *stream);
/* ... on a batch of small images (Nimg, h, w, C) taken as one mosaic image of R x Cc cells without building the mosaics
 * (see sq_conv2d_nhwc_mixed_mosaic_f32); workspace as for (1, R*(h+1), Cc*(w+1), Cin, Cout, K = 3) */
int sq_conv2d_nhwc_wgrad_mixed_mosaic_f32(const float *x, const float *dy, float *dw, float *db, float *workspace, int Nimg,
                                          int h, int w, int Cin, int Cout, int R, int Cc, float dw_scale, void *stream);
int sq_conv2d_nhwc_wgrad_scaled_f32(const float *x, const float *dy, float *dw, float *db, float *workspace, int N, int H,
                                    int W, int Cin, int Cout, int K, float dw_scale, void *stream);

/* first conv of down0 in the bf16 graph: f32 (N,H,W,Cin) image, Cin 1..7 -> bf16 (N,H,W,Cout), 3x3, f32 HWIO
 * weights (`num_inputs`, unet.py:131). */
int sq_conv3x3_first_fwd_bf16(const float *x, const float *w, const float *bias, void *y, int N, int H, int W,
                              int Cin, int Cout, int act, void *stream);
/* Sign masks of ReLU outputs: one bit per element in NHWC order (bit c & 7 of byte (pixel * Cout + c) >> 3, Cout % 16 == 0,
 * N*H*W*Cout/8 bytes).  The forward convs of a conv_block's conv1 (unet.py:265-270) write the mask beside their output;
 * the dgrad of conv2, which lets gradient through where conv1's ReLU was active, reads the mask instead of the tensor
 * (1/16 of the bytes).  sq_conv2d_nhwc_dgrad_maskgate_bf16 == sq_conv2d_nhwc_dgrad_gate_bf16 on the tensor, bit for bit. */
int sq_conv3x3_first_fwd_mask_bf16(const float *x, const float *w, const float *bias, void *y, void *mask, int N, int H,
                                   int W, int Cin, int Cout, int act, void *stream);
int sq_conv2d_nhwc_fwd_mask_bf16(const void *x, const void *wp, const float *bias, void *y, void *mask, int N, int H, int W,
                                 int Cin, int Cout, int K, int act, void *stream);
int sq_conv2d_nhwc_dgrad_maskgate_bf16(const void *dy, const void *wp_t, const void *mask, float scale, void *dx, int N,
                                       int H, int W, int Cin, int Cout, int K, void *stream);

/* dW (K,K,Cin,Cout) f32 and db (Cout, may be NULL) f32 from bf16 X (N,H,W,Cin) and bf16 dY (N,H,W,Cout);
 * Cin % 16 == 0, Cout % 16 == 0.  Transposing LDS reads (ds_read_b64_tr_b16) feed the MFMA. */
int64_t sq_conv2d_nhwc_wgrad_workspace_bf16(int N, int H, int W, int Cin, int Cout, int K);
int sq_conv2d_nhwc_wgrad_bf16(const void *x, const void *dy, float *dw, float *db, float *workspace, int N,
                              int H, int W, int Cin, int Cout, int K, void *stream);
/* parameter gradients of the 2x2/s2 transpose conv from x (N,H,W,Cin) bf16 and the output gradient in space-to-depth
 * form g (N,H,W,4*Cout) bf16: dW (2,2,Cout,Cin) f32, db (Cout) f32 or NULL; workspace as for the 1x1 wgrad Cin -> 4*Cout */
int sq_convT2x2s2_wgrad_bf16(const void *x, const void *g, float *dw, float *db, float *workspace, int N, int H, int W,
                             int Cin, int Cout, void *stream);

/* The concatenation in front of the discriminator's dense head (gan.py:213-226: tf.concat([conv, minibatch_stdev], -1) then
 * reshape) with bf16 features: flat f32 (npix, C + 1) = [float(conv (npix, C)), mb (npix)] in one pass, and its adjoint
 * (dconv rounded to bf16, dmb f32) -- each is the other's derivative, so the WGAN-GP second-order pass stays closed. */
int sq_head_concat_fwd_bf16(const void *conv, const float *mb, float *flat, int64_t npix, int C, void *stream);
int sq_head_concat_bwd_bf16(const float *dflat, void *dconv, float *dmb, int64_t npix, int C, void *stream);

/* bf16 <-> f32 casts (RNE), n % 4 == 0 */
int sq_cast_f32_to_bf16(const float *x, void *y, int64_t n, void *stream);
int sq_cast_bf16_to_f32(const void *x, float *y, int64_t n, void *stream);

/* bf16 variants of the streaming ops (C % 8 == 0 / n % 8 == 0): same semantics as the f32 entries */
int sq_maxpool2x2_fwd_bf16(const void *x, void *y, int N, int H, int W, int C, void *stream);
int sq_maxpool2x2_bwd_bf16(const void *x, const void *dy, void *dx, int N, int H, int W, int C, void *stream);
/* decoder junction backward in one pass (merged = bridge(up, skip), unet.py:312-319): g (N,H,W,4C) = d_up in the
 * space-to-depth layout sq_conv2d_nhwc_wgrad_bf16 / the 1x1 dgrad of the transpose conv consume, dskip
 * (N,2H,2W,C) = gradient of the skip operand.  H, W = the LOW-resolution side; up / skip needed for eltwise_mul. */
int sq_bridge_bwd_s2d_bf16(const void *dy, const void *up, const void *skip, void *g, void *dskip, int N, int H, int W,
                           int C, int bridge, void *stream);
/* max-pool backward + the other gradient of the pooled tensor (the U-Net skip path): dx = scatter(dy) + add */
int sq_maxpool2x2_bwd_add_bf16(const void *x, const void *dy, const void *add, void *dx, int N, int H, int W, int C,
                               void *stream);
/* ... and through the gate of the conv block that produced x = dropout(ReLU(.)) (unet.py:265-277): dx = x > 0 ?
 * (scatter(dy) + add) * gate_scale : 0, gate_scale = 1 / (1 - rate); 0 = no gate.  Replaces a stand-alone
 * sq_relu_scale_bwd_bf16 pass bit for bit (x is already read for the arg-max). */
int sq_maxpool2x2_bwd_add_gate_bf16(const void *x, const void *dy, const void *add, void *dx, int N, int H, int W, int C,
                                    float gate_scale, void *stream);
int sq_act_bwd_bf16(const void *dy, const void *y, void *dx, int64_t n, int act, void *stream);
/* dropout backward + the backward of the activation in front of it, one pass:
 * dx = act'(y) * (mask ? dy / (1 - rate) : 0), y = the activation output that entered the dropout */
int sq_act_dropout_bwd_bf16(const void *dy, const uint8_t *mask, const void *y, void *dx, int64_t n, float rate,
                            int act, void *stream);
/* conv + bias + act + dropout in one kernel: the mask is the counter hash of sq_dropout_fwd_bf16 over the flat
 * NHWC element index (same seed / step_dev semantics, same two roundings => same bits as the two kernels);
 * no mask tensor is written.  sq_relu_scale_bwd_bf16 is the matching backward for act == ReLU:
 * dx = y > 0 ? dy * scale : 0 with scale = 1 / (1 - rate)  (y > 0 <=> kept and active). */
int sq_conv2d_nhwc_fwd_dropout_bf16(const void *x, const void *wp, const float *bias, void *y, int N, int H, int W,
                                    int Cin, int Cout, int K, int act, float rate, uint32_t seed,
                                    const int32_t *step_dev, void *stream);
/* ... and the 2x2/s2 max pool of the result beside it (ypool (N,H/2,W/2,Cout); K = 3, H and W even; rate 0 = no dropout):
 * conv_block -> max_pool of an encoder level (unet.py:241-243, 265-277) in one kernel; ypool = sq_maxpool2x2_fwd_bf16(y) */
int sq_conv2d_nhwc_fwd_dropout_pool_bf16(const void *x, const void *wp, const float *bias, void *y, void *ypool, int N, int H,
                                         int W, int Cin, int Cout, int K, int act, float rate, uint32_t seed,
                                         const int32_t *step_dev, void *stream);
/* conv_block of down0 + max_pool_layer (unet.py:238-243, 265-277), training form, ONE launch for a single-channel f32 image
 * and 16 filters: y1 = relu(conv3x3(x, w1) + b1) and its sign mask mask1 (sq_conv3x3_first_fwd_mask_bf16's outputs, bit for
 * bit) are made per tile and never read back; y, ypool as sq_conv2d_nhwc_fwd_dropout_pool_bf16(y1, wp2, b2, relu). */
int sq_conv3x3_first_block_dropout_pool_bf16(const float *x, const float *w1, const float *b1, void *y1, void *mask1,
                                             const void *wp2, const float *b2, void *y, void *ypool, int N, int H, int W,
                                             float rate, uint32_t seed, const int32_t *step_dev, void *stream);
int sq_relu_scale_bwd_bf16(const void *dy, const void *y, void *dx, int64_t n, float scale, void *stream);
/* dX of a convolution whose input was the ReLU output `gate` (same shape as dx): sq_conv2d_nhwc_fwd_bf16 of dy
 * with the transposed packed filter, passed only where gate > 0 (the upstream ReLU backward fused in) */
int sq_conv2d_nhwc_dgrad_relu_bf16(const void *dy, const void *wp_t, const void *gate, void *dx, int N, int H, int W,
                                   int Cin, int Cout, int K, void *stream);
/* the same with a factor on what passes (backward of dropout(ReLU(.)) = `gate`): gate > 0 ? dgrad * gate_scale : 0 */
int sq_conv2d_nhwc_dgrad_gate_bf16(const void *dy, const void *wp_t, const void *gate, float gate_scale, void *dx, int N,
                                   int H, int W, int Cin, int Cout, int K, void *stream);
/* dgrad of a decoder block's first conv with the junction backward (merged = bridge(up, skip), unet.py:312-319) in
 * its epilogue: writes g (N,H/2,W/2,4*Cout) = d_up in the space-to-depth layout and dskip (N,H,W,Cout); d(merged) is
 * never stored.  Same bits as the dgrad followed by sq_bridge_bwd_s2d_bf16. */
int sq_conv2d_nhwc_dgrad_junction_bf16(const void *dy, const void *wp_t, const void *up, const void *skip, void *g,
                                       void *dskip, int N, int H, int W, int Cin, int Cout, int K, int bridge, void *stream);
int sq_bridge_fwd_bf16(const void *a, const void *b, void *y, int64_t n, int bridge, void *stream);
int sq_bridge_bwd_bf16(const void *dy, const void *a, const void *b, void *da, void *db, int64_t n, int bridge,
                       void *stream);
int sq_dropout_fwd_bf16(const void *x, void *y, uint8_t *mask, int64_t n, float rate, uint32_t seed,
                        int mask_given, const int32_t *step_dev, void *stream);
int sq_dropout_bwd_bf16(const void *dy, const uint8_t *mask, void *dx, int64_t n, float rate, void *stream);

/* conv_transpose_layer + bridge on bf16 tensors; w = bf16 copy of the (2,2,Cout,Cin) kernel, bias f32.
 * Cin % 32 == 0, Cout % 16 == 0.  The up-scaled value is rounded to bf16 before the bridge. */
int sq_convT2x2s2_nhwc_fwd_bf16(const void *x, const void *w, const float *bias, const void *skip, void *y,
                                int N, int H, int W, int Cin, int Cout, int bridge, void *stream);
/* training form of the decoder junction (unet.py:312-319): one pass writes the up-scaled tensor `up` (kept for the
 * bridge backward) AND merged = bridge(up, skip); same bits as sq_convT2x2s2_nhwc_fwd_bf16 + sq_bridge_fwd_bf16. */
int sq_convT2x2s2_bridge_both_fwd_bf16(const void *x, const void *w, const float *bias, const void *skip, void *up,
                                       void *merged, int N, int H, int W, int Cin, int Cout, int bridge, void *stream);

/* to_image head on a bf16 activation: f32 (Cin,Cout<=4) weights, f32 logits + uint8 mask (may be NULL);
 * backward: dz f32 -> dx bf16 (may be NULL), dw (Cin,Cout) f32, db f32; Cin in {16,32}, Cout <= 2. */
int sq_conv1x1_head_fwd_bf16(const void *x, const float *w, const float *bias, float *logits, uint8_t *mask,
                             int64_t npix, int Cin, int Cout, void *stream);
int64_t sq_conv1x1_head_bwd_workspace_bf16(int64_t npix, int Cin, int Cout);
int sq_conv1x1_head_bwd_bf16(const void *x, const float *w, const float *dz, void *dx, float *dw, float *db,
                             float *workspace, int64_t npix, int Cin, int Cout, void *stream);
/* gate_scale > 0: x = dropout(ReLU(.)) of the last conv block; dx leaves through that gate (x > 0 ? dx * gate_scale : 0) */
int sq_conv1x1_head_bwd_gate_bf16(const void *x, const float *w, const float *dz, void *dx, float *dw, float *db,
                                  float *workspace, int64_t npix, int Cin, int Cout, float gate_scale, void *stream);
/* to_image head + weighted softmax-CE of the training step as one forward and one backward kernel: the logits are never
 * written (sequitr/networks/unet.py:252-253 followed by the loss of SURVEY.md A.3).  forward: loss = f32 device scalar,
 * partials = sq_wsoftmax_ce_partials(npix) doubles; backward: dloss = f32 device scalar (gradient arriving at the loss),
 * workspace = sq_conv1x1_head_bwd_workspace_bf16 bytes, gate_scale as above.  Bit-identical to
 * sq_conv1x1_head_fwd_bf16 -> sq_wsoftmax_ce_fwd_bwd_f32 -> (* dloss) -> sq_conv1x1_head_bwd_gate_bf16. */
int sq_conv1x1_head_wce_fwd_bf16(const void *x, const float *w, const float *bias, const uint8_t *onehot,
                                 const float *weights, double *partials, float *loss, int64_t npix, int Cin, int Cout,
                                 void *stream);
int sq_conv1x1_head_wce_bwd_bf16(const void *x, const float *w, const float *bias, const uint8_t *onehot,
                                 const float *weights, const float *dloss, void *dx, float *dw, float *db, float *workspace,
                                 int64_t npix, int Cin, int Cout, float gate_scale, void *stream);
/* the backward pass that also leaves the LOSS (sq_conv1x1_head_wce_fwd_bf16's value, bit for bit) in `loss`: a training
 * step that runs the backward right behind the forward skips the forward kernel and its read of the level-0 activation
 * (the loss of unet.py:395-401's tensor contract is only a reported number there).  partials as in the forward. */
int sq_conv1x1_head_wce_bwd_loss_bf16(const void *x, const float *w, const float *bias, const uint8_t *onehot,
                                      const float *weights, const float *dloss, void *dx, float *dw, float *db,
                                      float *workspace, double *partials, float *loss, int64_t npix, int Cin, int Cout,
                                      float gate_scale, void *stream);

/* weight gradient of the first (Cin -> Cout, Cin 1..7) 3x3 convolution from the f32 image and a bf16 dY:
 * dW (3,3,Cin,Cout) f32, db (Cout) f32 or NULL */
int64_t sq_conv3x3_first_wgrad_workspace_bf16(int N, int H, int W, int Cin, int Cout);
int sq_conv3x3_first_wgrad_bf16(const float *x, const void *dy, float *dw, float *db, float *workspace, int N,
                                int H, int W, int Cin, int Cout, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mask -> connected components -> centroids (the step after the hot path).
 * CentroidWriter.write, sequitr/utils.py:531-578: per frame, per class c > 0,
 * scipy.ndimage.label(mask == c) (4-connectivity) and center_of_mass of every label.
 *   mask (N,H,W) uint8 class labels on the device; workspace sq_mask_centroids_workspace bytes, 16-B aligned.
 *   count (device int32): number of components found (may exceed max_out: then re-run with more room).
 *   out (max_out,5) f32 rows [frame, x = row centre, y = column centre, 0, class] in NO particular order;
 *   keys (max_out) int32 = linear index of each component's first pixel in raster order: sorting rows by
 *   (frame, class, key) gives the reference's order (scipy numbers labels by first pixel).
 * ---------------------------------------------------------------------------------------- */
int64_t sq_mask_centroids_workspace(int N, int H, int W);
int sq_mask_centroids_u8(const uint8_t *mask, int N, int H, int W, void *workspace, int32_t *count, float *out,
                         int32_t *keys, int max_out, void *stream);
/* volumetric form (CentroidWriter.write on (N,Z,X,Y) input, utils.py:511-521, after its swapaxes(1,-1)):
 * mask (N,D0,D1,D2), 6-connectivity; rows [frame, x, y, z, class] = centre along (D0, D1, D2);
 * workspace: sq_mask_centroids_workspace(N*D0, D1, D2). */
int sq_volume_centroids_u8(const uint8_t *mask, int N, int D0, int D1, int D2, void *workspace, int32_t *count,
                           float *out, int32_t *keys, int max_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Object measurements: what CentroidWriter.write's docstring promises beyond the centroid ("if the original image
 * data is provided, some image statistics are calculated", sequitr/utils.py:492-494).  Components, connectivity and
 * numbering are those of the centroid path above: 4 neighbours in a plane, 6 in a volume, two pixels linked only when
 * they carry the same class > 0, a component's root = its first pixel in raster order.
 *   mask (N,planes,H,W) uint8 class labels on the device, planes = 1 for planar masks; fewer than 2^31 elements.
 *   image: NULL, or the mask's shape in `dtype` = SQ_PIX_U8 / SQ_PIX_U16 / SQ_PIX_F32 (defined below, "Frame cleaning").
 *   workspace: sq_objects_workspace bytes (-1: too large), 16-B aligned: 8 B per pixel + 88 B per max_out.
 *   found (device int32): components before the size filter; when it exceeds max_out the rows are incomplete: re-run with
 *     max_out >= found.  count (device int32): objects kept = rows written.
 *   An object is kept iff min_area <= area <= max_area (inclusive; min_area >= 1; max_area <= 0: no upper bound).
 *   rows_i (max_out,12) int64, in NO particular order:
 *     [frame, class, key, area, lo_plane, lo_row, lo_col, hi_plane, hi_row, hi_col, isum, isumsq]
 *     key = linear index of the object's first voxel within its frame: sorting by (frame, class, key) gives the reference's
 *     order.  hi_* are exclusive (scipy.ndimage.find_objects slices).  isum / isumsq = the exact sum of x and of x*x under
 *     the object for integer images, 0 otherwise.
 *   rows_f (max_out,7) float64: [centre_plane, centre_row, centre_col, sum, sumsq, min, max]
 *     centre = (c * sum of coordinate) / (c * area) in float64, c the class: scipy.ndimage.center_of_mass(out, labels, index).
 *     sum / sumsq / min / max of the image under the object, 0 without an image.  Integer images: exact (sumsq rounded
 *     once to float64).  float32 images: sum and sumsq are float64 atomic adds of exact terms, so their last bits depend
 *     on arrival order; min / max are exact and leave NaN pixels out; a NaN pixel makes sum and sumsq NaN.
 *   slots (max_out) int32: the workspace slot of each output row, what sq_objects_relabel's rank is indexed by.
 * sq_objects_relabel reads the workspace the measure call on the same mask left behind: rank (n_slots) int32 with
 * n_slots = that call's max_out; labels (int32, the mask's shape, or NULL) = rank[slot of the pixel's object], 0 on
 * background; mask_out (uint8, or NULL) = mask where that rank is not 0, else 0.  Give rank 0 to dropped objects and the
 * 1-based position within the frame to kept ones for scipy-style label images.
 * Both return SQ_EINVAL with a message, before any launch, for null pointers, a bad dtype, min_area < 1, max_out < 1,
 * 2^31 or more elements, a workspace that is not 16-B aligned, an n_slots / shape that does not match the measure
 * call that filled the workspace, labels and mask_out both NULL.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_objects_workspace(int N, int planes, int H, int W, int max_out);
int sq_objects_measure(const uint8_t *mask, int N, int planes, int H, int W, const void *image, int dtype,
                       int64_t min_area, int64_t max_area, void *workspace, int32_t *count, int32_t *found,
                       int64_t *rows_i, double *rows_f, int32_t *slots, int max_out, void *stream);
int sq_objects_relabel(const uint8_t *mask, int N, int planes, int H, int W, const void *workspace,
                       const int32_t *rank, int n_slots, int32_t *labels, uint8_t *mask_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Shape of the measured objects: second-order coordinate sums, exposed faces, boundary voxels and the counts of the
 * 4-neighbourhood perimeter estimator (regionprops' `perimeter`), all integers defined on the mask.
 * sq_objects_shape reads the workspace the measure call on the same mask left behind, as sq_objects_relabel does:
 *   workspace, n_slots: that call's workspace and max_out;  slots, n: that call's `slots` and its count.
 *   shape_workspace: sq_objects_shape_workspace(n_slots) bytes (-1: n_slots < 1) = 104 per slot rounded up to 16, 16-B
 *     aligned; the call clears it.
 *   shape_i (n,16) int64: row i describes the object of row i of the measure call's rows_i / rows_f, in the same
 *     unsorted order, so the host applies one permutation to all three.
 * Coordinates are (p, r, c) = plane, row, column within the frame.  "Same object" = same root of the labelling.  A
 * neighbour outside the frame is not in the object; nothing connects across frames.  The columns:
 *    0- 2  s_p, s_r, s_c                       sum of p, r, c over the object's voxels (s_p = 0 when planes == 1)
 *    3- 8  s_pp, s_rr, s_cc, s_pr, s_pc, s_rc  sums of the products over the object's voxels
 *    9-11  faces_p, faces_r, faces_c           the (voxel, +/- direction along the axis) pairs whose neighbour is outside
 *                                              the frame or carries another byte; faces_p = 0 when planes == 1
 *   12     boundary                            voxels with at least one such exposed face (4 neighbours when planes == 1,
 *                                              6 otherwise)
 *   13-15  per_straight, per_diag, per_mixed   planar masks only (0 when planes > 1): with B = the object's boundary
 *          pixels, every pixel of B gets code = 1 + 2 n4 + 10 n8, n4 = its 4 edge neighbours that are in B OF THE SAME
 *          OBJECT, n8 the same for its 4 diagonal neighbours; codes 5, 7, 15, 17, 25, 27 count in per_straight, 21, 33 in
 *          per_diag, 13, 23 in per_mixed, every other code nowhere.  This is the 3 x 3 kernel [[10,2,10],[2,1,2],[10,2,10]]
 *          over the border image of one object's crop; perimeter = per_straight + per_diag sqrt(2) + per_mixed (1 + sqrt(2)) / 2.
 * planes, H and W may not exceed 65536: with fewer than 2^31 voxels per call that keeps every sum below 2^63
 * (a product of two coordinates is below 2^32), so the sums are exact and independent of the order of the atomics.
 * SQ_EINVAL with a message, before any launch and leaving shape_i untouched, for null pointers, n < 0 or n > n_slots,
 * a workspace / shape / n_slots that does not match the measure call that filled the workspace, workspaces that are
 * not 16-B aligned, planes, H or W above 65536.  n == 0 succeeds and writes nothing.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_objects_shape_workspace(int max_out);
int sq_objects_shape(const uint8_t *mask, int N, int planes, int H, int W, const void *workspace, int n_slots,
                     const int32_t *slots, int n, void *shape_workspace, int64_t *shape_i, void *stream);

/* ------------------------------------------------------------------------------------------
 * EDT weight maps (the step in front of the training hot path).
 * ImageWeightMap.pipe, sequitr/pipeline.py:475-479:
 *   d = distance_transform_edt(1 - image);  out = w0*(1-image)*exp(-(d*d)/(2 sigma^2 + 1e-99)) + image + 1
 * img (N,H,W) f32 binary label images (values 0 / 1; a pixel is a feature iff 1 - image == 0), one map per
 * image.  workspace: sq_weightmap_workspace bytes, 16-B aligned.  H, W < 30000.
 * Types as in numpy: the reference's image is float32 and w0 a Python scalar, so w0*(1-image) is the FLOAT32 product
 * fl32(fl32(w0) * fl32(1 - image)); it is widened where it meets the float64 exp(...), the rest is float64.
 *   sq_edt_sq_f32        : d2 (N,H,W) int32 = EXACT squared Euclidean distance to the nearest feature
 *                          (an image with no feature reproduces scipy's artefact: distance to index (-1, 0))
 *   sq_weightmap_edt_f32 : out64 (N,H,W) f64 as the reference computes it and / or out32 (N,H,W) f32, the
 *                          `weights` tensor the loss kernel takes (sq_wsoftmax_ce_fwd_bwd_f32)
 * ---------------------------------------------------------------------------------------- */
int64_t sq_weightmap_workspace(int N, int H, int W);
int sq_edt_sq_f32(const float *img, int32_t *d2, void *workspace, int N, int H, int W, void *stream);
int sq_weightmap_edt_f32(const float *img, double *out64, float *out32, void *workspace, int N, int H, int W,
                         double w0, double sigma, void *stream);

/* Volumetric EDT weight maps: ImageWeightMap.pipe, sequitr/pipeline.py:475-479, called on a (Z, X, Y) array, where
 * distance_transform_edt is the true 3-D Euclidean transform; dz = the depth spacing in in-plane pixels, scipy's
 * sampling = (dz, 1, 1).  img (N,D,H,W) f32 binary label volumes (a voxel is a feature iff 1 - image == 0), one map
 * per volume: the search never crosses from volume n into n +- 1.  0 < D, H, W < 30000, N*D*H*W < 2^31, dz finite
 * and > 0; workspace: sq_weightmap3d_workspace bytes (-1: the request is out of range), 16-B aligned.
 *   D3(n,z,x,y) = min over z' of A(z - z') + P(n,z',x,y), A(k) = fl(fl(k dz) fl(k dz)) in double, P = the exact planar
 *   squared distance of slice z' (infinite for a slice without a feature); a volume without any feature reproduces
 *   scipy's artefact, the distance to index (-1, 0, 0): D3 = fl(fl(((z+1) dz)^2 + x^2) + y^2).
 *   sq_edt3d_sq_f64        : d2 (N,D,H,W) f64 = D3 (for dz == 1 an exact integer)
 *   sq_weightmap3d_edt_f32 : d = sqrt(D3); out = w0*(1-image)*exp(-(d*d)/(2 sigma^2 + 1e-99)) + image + 1 in float64
 *                            except the float32 product w0*(1-image) (the reference on a float32 volume, as above),
 *                            written to out64 (N,D,H,W) and / or rounded once to out32, the `weights` tensor of the loss
 * SQ_EDT3D_LDS=0 (read per launch) runs the depth pass on global memory instead of LDS: the same result, bit for bit. */
int64_t sq_weightmap3d_workspace(int N, int D, int H, int W);
int sq_edt3d_sq_f64(const float *img, double *d2, void *workspace, int N, int D, int H, int W, double dz, void *stream);
int sq_weightmap3d_edt_f32(const float *img, double *out64, float *out32, void *workspace, int N, int D, int H, int W,
                           double w0, double sigma, double dz, void *stream);

/* ImageWeightMap2 (sequitr/pipeline.py:482-571), the per-pixel part on the device: `simplices` (nsimp,7) int32 rows
 * {tile, x0, y0, x1, y1, x2, y2} (x = row, y = column, as np.where orders them) and `longest` (nsimp) float64 = the
 * longest edge of each simplex, from scipy.spatial.Delaunay of the boundary points (host); img (N,H,W) binary f32.
 * Rasterises the simplices (point location; a pixel covered by several takes the largest value), builds the
 * pre-filter map (1024 where uncovered, 0 on foreground), applies scipy's gaussian_filter(sigma = 1) and the
 * reference's expression: float64 except w0*(1-mask), a float32 product because mask is mask.astype('float32').
 * out64 (N,H,W) and / or out32; workspace of sq_weightmap2_workspace bytes. */
int64_t sq_weightmap2_workspace(int N, int H, int W);
/* ImageWeightMap2's boundary points on the device (sequitr/pipeline.py:516-528: erosion outline of the label XOR the
 * outline of the label dilated three times, von Neumann element, border value 0): points (N,H,W) uint8, 1 = a vertex
 * of the triangulation.  img (N,H,W) binary f32. */
int sq_wm2_boundary_points_u8(const float *img, uint8_t *points, int N, int H, int W, void *stream);
/* HOST function (no GPU work): exact Delaunay triangulation of each tile's boundary points in place of
 * scipy.spatial.Delaunay (pipeline.py:531-537) -- integer predicates in 128-bit arithmetic, incremental insertion in scan
 * order, tiles on a small pool of host threads (SQ_HOST_THREADS, default 16).  xy = the (row, column) int32 pairs of
 * `nsets` tiles back to back, tile s = points offsets[s] .. offsets[s+1] (0 <= coordinate < 32768, distinct); writes
 * the (tile, x0, y0, x1, y1, x2, y2) rows and longest edges sq_weightmap2_delaunay_f32 takes.  A triangulation of n points
 * has < 2 n triangles: tile s owns rows 2 offsets[s] .. 2 offsets[s+1] - 1, written by the worker that triangulated it (no
 * second pass); the few rows a tile does not need are padding with tile = -1, which sq_weightmap2_delaunay_f32 skips.
 * Returns the number of rows = 2 * offsets[nsets] (cap must hold them), or a negative SQ_E* code. */
int64_t sq_delaunay2d_batch_i32(const int32_t *xy, const int64_t *offsets, int nsets, int32_t *simplices, double *longest,
                                int64_t cap);
int sq_weightmap2_delaunay_f32(const float *img, const int32_t *simplices, const double *longest, int nsimp, double *out64,
                               float *out32, void *workspace, int N, int H, int W, double w0, double sigma, void *stream);

/* ------------------------------------------------------------------------------------------
 * GAN operators on bf16 FEATURE tensors (BASELINE config 5 with bf16 storage; sequitr/networks/gan.py:44-136, 149-316):
 * activations and activation gradients are bf16 in HBM, every kernel computes in f32 and rounds once per stored value;
 * parameters, images (<= 4 channels), the discriminator's outputs and the losses stay f32.  C % 8 == 0 everywhere.
 *   pixel_norm (gan.py:49-51): fwd; bwd (act != NONE: x is that activation's output and dx also leaves through its
 *   backward, second rounding kept: == sq_pixelnorm_bwd_bf16(NONE) then sq_act_bwd_bf16, bit for bit); bwd2 as
 *   sq_pixelnorm_bwd2_f32.
 *   half_size by averaging / double_size (gan.py:133-136, 189-192): sumpool (scale 0.25 = average pool) and its adjoint
 *   broadcast (scale 1 = nearest-neighbour up-sampling), H and W are the LARGER tensor's size; *_act_bwd: the
 *   up-sampled gradient additionally passes the backward of the activation whose output is `gate`.
 *   to_image / from_image (gan.py:102-125) and their gradients: 1x1 convolutions between an f32 image side with
 *   <= 4 channels and a bf16 feature side -- smallin (image -> features), smallout (features -> image),
 *   wgrad1x1_small (m (Ca, C) = scale * sum_p a[p]^T b[p]; a == NULL: per-channel sums of b, from_image's bias gradient;
 *   asum != NULL: (Ca) per-channel sums of a from the same pass, to_image's bias gradient).
 *   Weights are f32 row-major (in, out), multiplied by wscale on the fly (equalised learning rate, gan.py:75-79).
 * ---------------------------------------------------------------------------------------- */
int sq_pixelnorm_fwd_bf16(const void *x, void *y, int64_t npix, int C, float eps, void *stream);
int sq_pixelnorm_bwd_bf16(const void *x, const void *dy, void *dx, int64_t npix, int C, float eps, int act, void *stream);
int sq_pixelnorm_bwd2_bf16(const void *x, const void *g, const void *v, void *dg, void *dx2, int64_t npix, int C, float eps,
                           void *stream);
int sq_sumpool2x2_bf16(const void *x, void *y, int N, int H, int W, int C, float scale, void *stream);
int sq_broadcast2x2_bf16(const void *src, void *dst, int N, int H, int W, int C, float scale, void *stream);
int sq_broadcast2x2_act_bwd_bf16(const void *src, const void *gate, void *dst, int N, int H, int W, int C, float scale,
                                 int act, void *stream);
int sq_act_fwd_bf16(const void *x, void *y, int64_t n, int act, void *stream);
int sq_conv1x1_smallin_fwd_bf16(const float *x, const float *w, const float *bias, void *y, int64_t npix, int Ca, int C,
                                float wscale, int act, void *stream);
int sq_conv1x1_smallout_fwd_bf16(const void *x, const float *w, const float *bias, float *y, int64_t npix, int C, int Co,
                                 float wscale, int act, void *stream);
int64_t sq_wgrad1x1_small_workspace_bf16(int64_t npix, int Ca, int C);
int sq_wgrad1x1_small_bf16(const float *a, const void *b, float *m, float *asum, float *workspace, int64_t npix, int Ca,
                           int C, float scale, void *stream);
/* weighted_conv2d (gan.py:61-99) on bf16 tensors: the forward is sq_conv2d_nhwc_fwd_bf16; these are the forms the
 * mixed (f32 tensor) GAN path has beside it -- the dgrad that leaves through the previous activation's backward
 * (== dgrad then sq_act_bwd_bf16, same two roundings), the small-image batch addressed as one mosaic (forward, or with
 * `gate` the gated dgrad; with a workspace the reduction over input channels is split over the grid where the launch would
 * otherwise be a handful of blocks, slices added in order by a finish kernel), and the weight gradient with the equalised-LR
 * factor in the finish kernel, plain or mosaic.
 * sq_conv2d_nhwc_wgrad_bf16 and the scaled form take channel counts that are multiples of 8 (8 mod 16: the ragged form). */
/* a discriminator block's second conv with the 2x2 average pool that follows it (gan.py:171-192) written from the same kernel:
 * y (N,H,W,Cout) and ypool (N,H/2,W/2,Cout) == sq_sumpool2x2_bf16(y, 0.25).  K = 3, even H and W. */
int sq_conv2d_nhwc_fwd_avgpool_bf16(const void *x, const void *wp, const float *bias, void *y, void *ypool, int N, int H, int W,
                                    int Cin, int Cout, int act, void *stream);
/* weighted_conv2d with norm=True (gan.py:86-97: conv -> bias -> activation -> pixel_norm, one op upstream) from one kernel:
 * y (N,H,W,Cout) = act(conv3x3(x, wp) + bias) and ynorm = pixel_norm(y, eps) of the STORED y (== sq_pixelnorm_fwd_bf16(y) up
 * to the f32 rounding of the per-pixel factor: the squares are added in another order).  One block holds all channels of a
 * pixel: Cout % 8 == 0, Cout <= 64 (the generator's 32x32 .. 256x256 levels).  y may be NULL (only ynorm is wanted). */
int sq_conv2d_nhwc_fwd_pixelnorm_bf16(const void *x, const void *wp, const float *bias, void *y, void *ynorm, int N, int H, int W,
                                      int Cin, int Cout, int act, float eps, void *stream);
int sq_conv2d_nhwc_dgrad_actgate_bf16(const void *dy, const void *wp_t, const void *gate, int act, void *dx, int N, int H,
                                      int W, int Cin, int Cout, int K, void *stream);
int sq_conv2d_nhwc_mosaic_bf16(const void *x, const void *wp, const float *bias, const void *gate, void *y, int Nimg, int h,
                               int w, int Cin, int Cout, int act, int R, int Cc, float *workspace, int64_t workspace_bytes,
                               void *stream);
/* Launch plan of the implicit-GEMM convolutions, computed on the host without a HIP call (the choices the launchers make,
 * from the same functions, under the same environment switches SQ_CONV_BF16_NARROW, SQ_CONV_STAGE32, SQ_CONV_L0, ...).
 * family: SQ_PLAN_BF16 (bf16 tensors: sq_conv2d_nhwc_fwd_bf16 and its fused forms, sq_conv2d_nhwc_mosaic_bf16),
 *         SQ_PLAN_MIXED (f32 tensors, bf16 operands: sq_conv2d_nhwc_fwd_mixed_f32, ..._dgrad_actgate_mixed_f32, ..._mixed_mosaic_f32),
 *         SQ_PLAN_F32 (the f32 v2 / level-0 kernels behind sq_conv2d_nhwc_fwd_f32, sq_conv2d_concat_nhwc_fwd_f32 with
 *         Cin = both sources' channels, sq_conv3x3_pool_fwd_f32).
 * form: SQ_PLAN_PLAIN (also the relu / dropout gates of the plain kernel), _JUNCTION, _POOL (max or average pooled copy;
 *         f32: sq_conv3x3_pool_fwd_f32), _MASK, _MASKGATE, _ACTGATE, _FIRSTBLOCK, _PIXELNORM, _CONCAT (f32).
 * act: SQ_ACT_* of the call (the level-0 kernel takes ReLU only); flags: SQ_PLAN_WSCALE when an f32 call has wscale != 1.
 * mosaic: NULL, or {R, Cc} of a mosaic call, whose (N, H, W) are then (Nimg, h, w); workspace_bytes: its split-K room (0: none).
 * out[5] = {BN channel-block width, KC input channels per chunk, gy channel blocks, S split-K slices, 1 if the f32 level-0
 * kernel takes the call (BN, KC, gy then describe that kernel: Cout, 16, 1)}.  Returns SQ_OK, or SQ_EINVAL where no kernel of
 * the family takes the call. */
#define SQ_PLAN_BF16 0
#define SQ_PLAN_MIXED 1
#define SQ_PLAN_F32 2
#define SQ_PLAN_PLAIN 0
#define SQ_PLAN_JUNCTION 1
#define SQ_PLAN_POOL 2
#define SQ_PLAN_MASK 3
#define SQ_PLAN_MASKGATE 4
#define SQ_PLAN_ACTGATE 5
#define SQ_PLAN_FIRSTBLOCK 8
#define SQ_PLAN_PIXELNORM 9
#define SQ_PLAN_CONCAT 10
#define SQ_PLAN_WSCALE 1
int sq_conv_plan(int family, int form, int N, int H, int W, int Cin, int Cout, int K, int act, int flags, const int *mosaic,
                 int64_t workspace_bytes, int *out);
/* Tile walk of the persistent f32 inference kernels, computed on the host without a HIP call from the functions the launchers
 * take their grids from.  Block b of a grid of G takes item b, b + G, b + 2G, ... (a 16 x 16 pixel tile; for the transpose
 * conv a (row tile, pixel tile) pair), so the busiest block walks ceil(items / G) of them and the idlest floor(items / G).
 * form: SQ_PLAN_PLAIN (sq_conv2d_nhwc_fwd_f32), _POOL (sq_conv3x3_pool_fwd_f32), _CONCAT (sq_conv2d_concat_nhwc_fwd_f32,
 *       Cin = both sources' channels), _FIRSTBLOCK (sq_conv3x3_first_block_fwd_f32: Cin 1, Cout 16; flags SQ_PLAN_POOLED when
 *       it also pools), _UP (sq_convT_conv3x3_fwd_f32: Cin 16, Cout 16, (N, H, W) of the output), _HEAD
 *       (sq_conv3x3_head_fwd_f32: Cout 16, head_c classes), _CONVT (sq_convT2x2s2_nhwc_fwd_f32: (N, H, W) of the input, K unused).
 * flags: SQ_PLAN_WSCALE as for sq_conv_plan, SQ_PLAN_POOLED.  The switches SQ_CONV_L0, SQ_CONV_STAGE32, SQ_CONVT_V2 and
 * SQ_CONVT_WNI act as on the launchers.
 * out[SQ_WALK_N]: [SQ_WALK_KERNEL] SQ_WALK_L0 (level-0 kernel), SQ_WALK_V2 (generic kernel), SQ_WALK_CONVT (transpose conv v2)
 * or SQ_WALK_NONE (a transpose conv the v2 kernel declines: no walk, everything else 0); [SQ_WALK_G] blocks along the walk;
 * [SQ_WALK_TMIN], [SQ_WALK_TMAX] items of the idlest / busiest block; [SQ_WALK_GX], [_GY], [_GN] the stride in tile
 * coordinates, G = gn tiles_x tiles_y + gy tiles_x + gx (the level-0 kernel is handed the triple; the generic kernel derives
 * the same one); [SQ_WALK_MTILES] row tiles of the transpose conv (4 Cout / 128); [SQ_WALK_CBLOCKS] channel blocks, each
 * walking the same tiles (gridDim.y of the generic kernel, else 1); [SQ_WALK_ITEMS] items of the walk (pixel tiles; for the
 * transpose conv row tiles x pixel tiles, item = pixel tile * mtiles + row tile); [SQ_WALK_TILEPX] pixels of a pixel tile
 * (256; transpose conv: 32, 64 or 128 consecutive input pixels).  Returns SQ_OK, or SQ_EINVAL for a call the entry point
 * would refuse. */
#define SQ_PLAN_UP 11
#define SQ_PLAN_HEAD 12
#define SQ_PLAN_CONVT 13
#define SQ_PLAN_POOLED 2
#define SQ_WALK_NONE 0
#define SQ_WALK_L0 1
#define SQ_WALK_V2 2
#define SQ_WALK_CONVT 3
#define SQ_WALK_KERNEL 0
#define SQ_WALK_G 1
#define SQ_WALK_TMIN 2
#define SQ_WALK_TMAX 3
#define SQ_WALK_GX 4
#define SQ_WALK_GY 5
#define SQ_WALK_GN 6
#define SQ_WALK_MTILES 7
#define SQ_WALK_CBLOCKS 8
#define SQ_WALK_ITEMS 9
#define SQ_WALK_TILEPX 10
#define SQ_WALK_N 11
int sq_conv_walk_plan(int form, int N, int H, int W, int Cin, int Cout, int K, int act, int flags, int head_c, int *out);
int sq_conv2d_nhwc_wgrad_scaled_bf16(const void *x, const void *dy, float *dw, float *db, float *workspace, int N, int H,
                                     int W, int Cin, int Cout, int K, float dw_scale, void *stream);
int sq_conv2d_nhwc_wgrad_mosaic_bf16(const void *x, const void *dy, float *dw, float *db, float *workspace, int Nimg, int h,
                                     int w, int Cin, int Cout, int R, int Cc, float dw_scale, void *stream);

/* Weight gradients of SEVERAL layers in one launch (+ one finish launch) per kernel block shape: the deep layers of a
 * training step are each a ~37 us launch for ~10 us of matrix work (ramp-up and the cross-wave reduction run with the chip
 * idle, and every one of a layer's ~512 blocks ends with a cross-wave reduction); sharing one grid the layers are cut into a
 * quarter as many, longer blocks.  Every item is what sq_conv2d_nhwc_wgrad_scaled_bf16 (convT_cout == 0) or
 * sq_convT2x2s2_wgrad_bf16 (convT_cout > 0: K = 1, Cout = 4 * convT_cout, dW (2,2,convT_cout,Cin)) computes, to f32 rounding
 * (the same products; more of them summed per block, fewer block partials in the fixed-order finish); run-to-run identical.
 * bf16 X (N,H,W,Cin) and dY (N,H,W,Cout), channel counts multiples of 16 (plain items: of 8, the ragged form), db may be NULL.  accumulate: bit 0 -- dW is ADDED to
 * the contents of dw, bit 1 -- db to the contents of db (a parameter used by several passes of one step: the first item
 * writes, the later ones accumulate; items naming the same destination run in item order, in separate launches).
 * The caller keeps X and dY alive until the launch has run. */
typedef struct sq_wgrad_item {
    const void *x, *dy;
    float *dw, *db;
    int32_t N, H, W, Cin, Cout, K;
    int32_t convT_cout;
    float dw_scale;
    int32_t accumulate;
    int32_t mosaic_R, mosaic_Cc;   /* > 0: X / dY are N small images (H, W <= 8) taken as one mosaic of R x Cc cells (K = 3) */
    int32_t reserved;
} sq_wgrad_item;
int64_t sq_conv2d_nhwc_wgrad_group_workspace_bf16(const sq_wgrad_item *items, int n);
int sq_conv2d_nhwc_wgrad_group_bf16(const sq_wgrad_item *items, int n, float *workspace, void *stream);

/* Launch plan of the weight gradients, computed on the host without a HIP call (the choices the launchers and the workspace
 * queries make, from the same functions, under the same environment switches SQ_WGRAD_BF16_NARROW, _MAX, _K3,
 * SQ_WGRAD_INTERLEAVE, SQ_WGRAD_GROUP_SHRINK, SQ_WGRAD_PAIR_MAJOR).
 * sq_wgrad_plan: family SQ_PLAN_BF16 (sq_conv2d_nhwc_wgrad_bf16 and its scaled / mosaic / transpose-conv forms), SQ_PLAN_MIXED
 * (sq_conv2d_nhwc_wgrad_mixed_f32 and its forms), SQ_PLAN_F32 (sq_conv2d_nhwc_wgrad_f32; Cin 1..7: the small-Cin kernel, also
 * that of sq_conv3x3_first_wgrad_bf16).  mosaic: NULL or {R, Cc}, (N, H, W) then (Nimg, h, w); convT_cout > 0: the 1x1 form of
 * sq_convT2x2s2_wgrad_bf16 with Cout = 4 * convT_cout.  out[SQ_WGP_N]:
 *   KS; NI, NO (16-channel planes of Cin / Cout per block; f32: KC input channels, BN output channels); kind (SQ_WGP_*);
 *   PF prefetch depth (tiles in flight; f32: 1); npairs channel-block pairs; gx tile ranges; tpb tiles per block (< 0: block bx
 *   takes tiles bx, bx + gx, ...); G block groups of the finish; workspace floats.
 * sq_wgrad_group_plan: out[SQ_WGP_GROUP_N] per item: the launch ("bucket") it runs in, its plan as above after the group's shrink
 * (workspace: the floats it writes), 1 if the pair-major block mapping applies, and its partials' offset in the workspace
 * (floats).  Returns the number of buckets, or SQ_EINVAL. */
#define SQ_WGP_KS 0
#define SQ_WGP_NI 1
#define SQ_WGP_NO 2
#define SQ_WGP_KIND 3
#define SQ_WGP_PF 4
#define SQ_WGP_NPAIRS 5
#define SQ_WGP_GX 6
#define SQ_WGP_TPB 7
#define SQ_WGP_G 8
#define SQ_WGP_WS 9
#define SQ_WGP_N 10
#define SQ_WGP_GROUP_N (SQ_WGP_N + 3)
#define SQ_WGP_PLAIN 0
#define SQ_WGP_MOSAIC 1
#define SQ_WGP_RAGGED 2
#define SQ_WGP_CONVT 3
#define SQ_WGP_F32 4
#define SQ_WGP_F32_SMALL 5
int sq_wgrad_plan(int family, int N, int H, int W, int Cin, int Cout, int K, const int *mosaic, int convT_cout, int64_t *out);
int sq_wgrad_group_plan(const sq_wgrad_item *items, int n, int64_t *out);

/* ------------------------------------------------------------------------------------------
 * Volumes (UNet3D inference).  Layout NDHWC: x (N,D,H,W,C).  Numerics contract -- every 3-D op is DEFINED through the
 * planar f32 entries above, so its result is pinned bit for bit by oracle/sq_oracle.c:
 *   sq_conv3d_ndhwc_fwd_f32: 3x3x3 SAME stride-1 convolution + bias + activation.  w (3,3,3,Cin,Cout) (TF conv3d layout
 *     kd,kh,kw,in,out), bias (Cout) or NULL, y (N,D,H,W,Cout).  y equals sq_conv2d_nhwc_fwd_f32 (K = 3) applied to the
 *     N*D planar images of the depth-stacked input xs[n,d,h,w, kd*Cin + c] = x[n, d+kd-1, h, w, c] (zero slices beyond
 *     the depth ends) with the stacked filter ws[kh,kw, kd*Cin + c, o] = w[kd,kh,kw,c,o]: one fmaf chain from +0 per
 *     output, reduction order
 *       Cin % 16 == 0: depth tap, 16-channel chunk, in-plane tap (raster), channel;
 *       Cin in {1,2} (a single chunk of 3*Cin): in-plane tap, depth tap, channel;
 *     then "+ bias", then the activation.  Supported: Cin in {1,2} or Cin % 16 == 0, Cout % 4 == 0, one depth slice
 *     (H*W*max(Cin,Cout) floats) < 2 GiB; whole tensors may exceed 2 GiB (SQ_C3_WINDOW addressing).
 *   sq_maxpool2x2x2_fwd_f32: 2x2x2 stride-2 VALID max pooling, the max of 8 values.  D,H,W even, C % 4 == 0.
 *   sq_convT2x2x2s2_ndhwc_fwd_f32: 2x2x2 stride-2 transpose convolution + bias, then bridge(upscale, skip).  x (N,D,H,W,Cin),
 *     w (2,2,2,Cout,Cin) (TF conv3d_transpose layout), skip / y (N,2D,2H,2W,Cout).  Output slice 2d+a equals
 *     sq_convT2x2s2_nhwc_fwd_f32 of input slice d with w[a] (bias and bridge included).  Cin % 16 == 0, Cout % 4 == 0.
 *   The 1x1x1 head + argmax, the bridges and batch-norm inference are pointwise: the planar entries on the
 *   (N*D, H, W, C) view.
 * sq_conv3d_plan: the launch plan of sq_conv3d_ndhwc_fwd_f32, computed on the host without a HIP call (the launcher calls
 *   the same function).  out[SQ_C3P_N] = {kind SQ_C3_MFMA / SQ_C3_DIRECT, BN output channels per block, KC stacked input
 *   channels per staged chunk, gx blocks over the pixel tiles (direct kernel: one per tile and 4 output slices), gy channel blocks, addressing SQ_C3_FLAT / SQ_C3_WINDOW}.  Returns SQ_OK, or
 *   SQ_EINVAL for a shape no kernel takes.
 * ---------------------------------------------------------------------------------------- */
#define SQ_C3P_KIND 0
#define SQ_C3P_BN 1
#define SQ_C3P_KC 2
#define SQ_C3P_GX 3
#define SQ_C3P_GY 4
#define SQ_C3P_ADDR 5
#define SQ_C3P_N 6
#define SQ_C3_MFMA 0
#define SQ_C3_DIRECT 1
#define SQ_C3_FLAT 0
#define SQ_C3_WINDOW 1
int sq_conv3d_plan(int N, int D, int H, int W, int Cin, int Cout, int *out);
int sq_conv3d_ndhwc_fwd_f32(const float *x, const float *w, const float *bias, float *y, int N, int D, int H, int W,
                            int Cin, int Cout, int act, void *stream);
int sq_maxpool2x2x2_fwd_f32(const float *x, float *y, int N, int D, int H, int W, int C, void *stream);
int sq_convT2x2x2s2_ndhwc_fwd_f32(const float *x, const float *w, const float *bias, const float *skip, float *y, int N,
                                  int D, int H, int W, int Cin, int Cout, int bridge, void *stream);

/* Volumes, training side (f32; UNet3DTrain).  Pointwise gradients (activation, bridge, dropout, batch norm, head, loss)
 * are the planar entries on flat views.
 *   sq_conv3d_weight_transform_f32: wt[kd][kh][kw][co][ci] = w[2-kd][2-kh][2-kw][ci][co].  The input gradient of
 *     sq_conv3d_ndhwc_fwd_f32 is DEFINED as sq_conv3d_ndhwc_fwd_f32(dY, wt, NULL, ..., Cin := Cout, Cout := Cin, act none):
 *     it inherits that entry's reduction order and oracle.  Supported where the forward takes the swapped channels:
 *     Cout % 16 == 0 or Cout in {1,2}, and Cin % 4 == 0; anything else SQ_EINVAL.
 *   sq_conv3d_ndhwc_wgrad_f32: dw (3,3,3,Cin,Cout), dw[kd,kh,kw,c,o] = sum_{n,d,h,w} x[n,d+kd-1,h+kh-1,w+kw-1,c] *
 *     dy[n,d,h,w,o] (zeros outside the volume), db[o] = sum dy[...,o] (db may be NULL): the planar weight gradient of the
 *     depth-stacked input.  Two-stage fixed-order sums, no float atomics, run-to-run bit-identical; every element of dw and
 *     db is written (dw[0], dw[2] are exact zeros at D == 1).  Supported: Cin in {1,2} or Cin % 16 == 0, Cout % 4 == 0,
 *     every tensor < 2 GiB.  workspace: sq_conv3d_ndhwc_wgrad_workspace_f32 bytes (-1: shape not taken).
 *   sq_conv3d_wgrad_plan: its launch plan, host only (the launcher and the workspace query call it).  out[SQ_WGP_N] as
 *     sq_wgrad_plan: KS 3; NI = stacked input channels per chunk (16, or 3*Cin for Cin in {1,2}); NO = output channels per
 *     block; kind SQ_WGP_F32 / SQ_WGP_F32_SMALL; PF 1; npairs = (depth tap, ci chunk, co chunk) triples (small: co groups);
 *     gx tile ranges over the N*D*tiles pixel tiles; tpb; G; workspace floats.  SQ_EINVAL for a shape no kernel takes.
 *   sq_maxpool2x2x2_bwd_f32: x the pool input (N,D,H,W,C), dy (N,D/2,H/2,W/2,C); the gradient goes to the FIRST maximum
 *     of each window in (depth, row, column) raster order, zeros elsewhere; every element of dx is written.  D,H,W even,
 *     C % 4 == 0.
 *   sq_space_to_depth2x2x2_f32: dy (N,2D,2H,2W,C) -> g (N,D,H,W,8C), g[n,d,i,j, ((2a+b)*2+e)*C + c] = dy[n,2d+a,2i+b,2j+e,c]
 *     (D,H,W the small side): the transpose conv's backward is then a planar 1x1 conv and a planar 1x1 weight gradient
 *     on the (N*D, H, W, .) views.  C % 4 == 0. */
int sq_conv3d_weight_transform_f32(const float *w, float *wt, int Cin, int Cout, void *stream);
int sq_conv3d_wgrad_plan(int N, int D, int H, int W, int Cin, int Cout, int64_t *out);
int64_t sq_conv3d_ndhwc_wgrad_workspace_f32(int N, int D, int H, int W, int Cin, int Cout);
int sq_conv3d_ndhwc_wgrad_f32(const float *x, const float *dy, float *dw, float *db, float *workspace, int N, int D, int H,
                              int W, int Cin, int Cout, void *stream);
int sq_maxpool2x2x2_bwd_f32(const float *x, const float *dy, float *dx, int N, int D, int H, int W, int C, void *stream);
int sq_space_to_depth2x2x2_f32(const float *dy, float *g, int N, int D, int H, int W, int C, void *stream);

/* ------------------------------------------------------------------------------------------
 * Tile front end: raw single-channel camera frames in HBM (OctopusData .dat memmap,
 * sequitr/dataio/octopus.py:231-245) -> ImageNorm (sequitr/pipeline.py:350-356) -> network tiles, and the
 * tile masks back to full-frame masks.
 *   sq_frame_stats     : per-frame float32 mean and std EXACTLY as numpy's np.mean / np.std of the float32
 *                        frame (8192-element chunks, pairwise blocks of 128 with 8 accumulators); H*W <= 2^24.
 *                        workspace: sq_frame_stats_workspace bytes.  frames need the alignment of their pixel type
 *                        only (a channel's slice of multi-channel planes, below).
 *   sq_frames_to_tiles : tiles (F*TR*TC, TS, TS) f32, tile (f,ty,tx) = frame f at origin (oy[ty], ox[tx]),
 *                        value (x - mean[f]) / std[f], or the plain cast when mean == std == NULL.  One kernel cuts the
 *                        tiles of this entry, of sq_frames_to_tiles_bg and of sq_frames_to_tiles_mc (C = 1 here); it
 *                        indexes tile rows in 32 bits, so all three refuse F*TR*TC*TS > 2^31 - 1 ("tile rows are out of
 *                        range") before any launch -- unreachable for TS >= 36 within 288 GB of tiles.  tiles need no
 *                        more than float alignment here: C = 1 stores scalars.
 *   sq_stitch_masks_u8 : out (F,H,W): pixel (y,x) = tile_masks[(f, ymap[y]>>16, xmap[x]>>16)][ymap[y]&0xffff][xmap[x]&0xffff]
 *
 * Multi-channel frames (bright field + fluorescence, one stack per channel: sequitr/dataio/octopus.py:321-328) are
 * CHANNEL-MAJOR PLANES on the device: channel c of frame f is a contiguous (H, W) plane at element offset
 * c * chan_stride + f * H * W, chan_stride >= F * H * W elements (a partial batch [:, :n] of a (C, B, H, W) buffer has
 * chan_stride = B * H * W).  Every per-frame entry above and under "Frame cleaning" then runs unchanged on a channel's
 * slice; per-channel statistics are (C, F) arrays, index c * F + f.
 *   sq_frames_to_tiles_mc : tiles (F*TR*TC, TS, TS, C) f32, interleaved, sq_frames_to_tiles' geometry, C = 1 .. 8, one
 *                        launch.  chan_mode is a HOST array of C int32, read before the launch; channel c of a tile is
 *                          SQ_CH_CAST    : (float)v
 *                          SQ_CH_NORM    : ((float)v - mean32[c,f]) / std32[c,f] in float32 (sq_frames_to_tiles' value)
 *                          SQ_CH_BG      : (float)r,  r = (double)x - bg(u, v) from coef[c,f,0..5] ("Frame cleaning")
 *                          SQ_CH_BG_NORM : (float)((r - mean64[c,f]) / (1e-99 + std64[c,f])) in fp64 (sq_frames_to_tiles_bg's)
 *                        with bg evaluated by rows as sq_frames_to_tiles_bg does, every multiply-add of the surface one
 *                        fused operation:  t' = fma(t, fma(c5, t, c2), c0),  b = fma(c4, t, c1),
 *                        bg = fma(s, fma(c3, s, b), t').  Channel c is what sq_frames_to_tiles / sq_frames_to_tiles_bg
 *                        give on channel c's stack: the same kernel.  All channels are read in one pixel type `dtype`; the two background
 *                        modes need SQ_PIX_F32 (the float32 frames sq_frame_outliers_f32 or a cast wrote) and H, W >= 3.
 *                        A statistics pointer may be NULL only if no channel's mode reads it.  An unknown mode or pixel
 *                        type, C outside 1 .. 8, chan_stride < F*H*W, a tile that does not fit, F*TR*TC*TS >= 2^31 and
 *                        tiles not 16-byte aligned are refused before any launch.
 * Where the reference is silent: its ImageOutliers and ImageNorm already work per channel of an (H, W, C) image
 * (sequitr/pipeline.py:174-180), its ImageBGSubtract ravels (H, W, C) against H*W rows and fails for C > 1.  Here every
 * channel gets its own fit: the single-channel contract applied per plane.
 * ---------------------------------------------------------------------------------------- */
#define SQ_PIX_U8 0
#define SQ_PIX_U16 1
#define SQ_PIX_F32 2
#define SQ_CH_CAST 0
#define SQ_CH_NORM 1
#define SQ_CH_BG 2
#define SQ_CH_BG_NORM 3
int64_t sq_frame_stats_workspace(int F, int H, int W);
int sq_frame_stats(const void *frames, int dtype, float *mean, float *stdv, void *workspace, int F, int H, int W,
                   void *stream);
int sq_frames_to_tiles(const void *frames, int dtype, const float *mean, const float *stdv, const int32_t *oy,
                       const int32_t *ox, float *tiles, int F, int H, int W, int TR, int TC, int TS, void *stream);
int sq_stitch_masks_u8(const uint8_t *tile_masks, const int32_t *ymap, const int32_t *xmap, uint8_t *out, int F, int H,
                       int W, int TR, int TC, int TS, void *stream);
int sq_frames_to_tiles_mc(const void *frames, int dtype, int64_t chan_stride, const int32_t *chan_mode, const float *mean32,
                          const float *std32, const double *coef, const double *mean64, const double *std64,
                          const int32_t *oy, const int32_t *ox, float *tiles, int F, int H, int W, int C, int TR, int TC,
                          int TS, void *stream);

/* ------------------------------------------------------------------------------------------
 * Tile views and probability stitch: test-time augmentation over the symmetries of the square, and per-pixel class
 * probabilities stitched to whole frames (sequitr_amd/frontend.py: FrameTiler.view, FrameTiler.stitch_probs,
 * segment_frames(tta=, probabilities=)).  The reference samples the same symmetries on the training side (ImageFlip's four
 * flip states, the quarter turns of ImageRotate; sequitr/pipeline.py); here a trained net is evaluated under them and its
 * logits averaged, all in HBM.
 *
 * VIEWS.  A tile batch is (N, T, T, E) float32: square tiles, E interleaved elements per pixel (C input channels or K
 * class logits), 1 <= E <= 16.  op is 0 .. 7: bit 0 mirrors axis 1, bit 1 mirrors axis 2, bit 2 transposes the two axes
 * (the role of the volume sampler's transpose bit):
 *
 *     view_op(x)[n, i, j, e] = x[n, a, b, e]
 *     (p, q) = (j, i) if op & 4 else (i, j)
 *     a = T-1-p if op & 1 else p
 *     b = T-1-q if op & 2 else q
 *
 * unview_op is the inverse, unview_op(view_op(x)) == x.  The eight ops are the dihedral group of the square, so the inverse
 * of an op is an op:  unview_op == view_op'  with  op' = op  for op in {0, 1, 2, 3, 4, 7}  (the mirrors, the half turn and
 * the two diagonal reflections are involutions),  5' = 6  and  6' = 5  (the two quarter turns).  As numpy says it, on one
 * (T, T, E) tile: op 3 is np.rot90(x, 2), op 5 is np.rot90(x, -1) (clockwise), op 6 is np.rot90(x, 1) (counter-clockwise), op 4 is
 * x.transpose(1, 0, 2), op 7 the transpose about the other diagonal.
 *
 * SETS.  tta = None: ops (0);  'flips': ops (0, 1, 2, 3), ImageFlip's four states;  'dihedral': ops (0 .. 7).  Only these,
 * so n is 1, 4 or 8: the mean is an exact scaling and the argmax of the sum is the argmax of the mean.
 *
 * MERGE.  With L_op = net.build(view_op(tiles)):
 *     acc = unview_0(L_0)
 *     acc = acc + unview_op(L_op)        for op ascending, one float32 add per element per op
 * in that order: deterministic, run-to-run identical.  mean = acc * (1/n) is exact.
 *
 * MASK.  Frame pixel (y, x) takes its owner tile and local coordinate from ymap / xmap (sq_stitch_masks_u8's maps,
 * unchanged: one owner per pixel, no seam blending).  Its class pc is the one sq_argmax_u8's loop writes for the K values
 * of acc:  best = 0;  for c = 1 .. K-1: if (acc[c] > acc[best]) best = c  -- ties go to the lowest class, NaN never wins,
 * a row that starts with NaN gives class 0.  With n = 1 the mask is sq_stitch_masks_u8 of sq_argmax_u8, byte for byte.
 *
 * PROBABILITIES.  From the same K values, in float32, contraction off:
 *     l_k = acc_k * inv_n                 inv_n = 1/n
 *     m   = l_pc
 *     e_k = expf(l_k - m)                 full-precision expf
 *     s   = e_0 + ... + e_{K-1}           in index order, starting from 0
 *     p_k = e_k / s
 * A row whose m is not finite, or that holds a NaN, gives NaN in every class.  Output is planar (F, K, H, W): SQ_PIX_F32
 * writes p_k, SQ_PIX_U8 writes (uint8) floorf(p_k * 255 + 0.5f) and 0 for NaN.  With K == 1, p = 1 where the logit is
 * finite.  Against the float64 softmax every finite p_k is within (K + 4) * 2^-23: one rounding in l - m costs at most
 * 2^-24 d e^-d <= 2^-24 / e in e_k, expf, the K - 1 adds and the divide about an ulp each on values <= 1, doubled.
 *
 *   sq_tiles_view_f32 : dst = view_op(src), or unview_op(src) when inverse != 0; dst += ... when accumulate != 0 (every
 *                       element read, changed and written by exactly one thread).  Refused before any launch, dst
 *                       untouched: a null pointer, src and dst the same or overlapping, op outside 0 .. 7, E outside
 *                       1 .. 16, T outside 1 .. 65535, N < 1 or N * T > 2^31 - 1, pointers not 16-byte aligned
 *                       (SQ_EALIGN).  Ops 0 .. 3 are row streams (16-byte accesses where E and T allow: E % 4 == 0, or
 *                       T * E % 4 == 0 with no mirror of axis 2 or E <= 2).  Ops 4 .. 7 go through a padded LDS block of
 *                       sq_tiles_view_block(E) pixels a side (32 for E <= 4, 16 above), so that loads and stores both run
 *                       along rows; SQ_TTA_LDS=0 (read per call) gathers them directly instead, with the same bits.  The
 *                       LDS form was made the default by design and has kept it by measurement: on an MI355X it is
 *                       2.1 - 2.6 x the direct gather (tools/tta_bench.py, profiles/tta_bench.json; DESIGN.md "Test-time
 *                       augmentation").  No allocation, no synchronisation: the same under graph capture.
 *   sq_stitch_probs   : mask_out (F, H, W) uint8 and / or prob_out (F, K, H, W) of prob_dtype SQ_PIX_U8 or SQ_PIX_F32
 *                       from tile_logits (F*TR*TC, TS, TS, K) = acc, as defined above.  Either output may be NULL, not
 *                       both.  K is 1 .. 16, inv_n in (0, 1]; F * H <= 2^31 - 1; tile_logits 16-byte aligned.  The maps
 *                       are trusted as sq_stitch_masks_u8 trusts them.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------- */
int sq_tiles_view_block(int E);
int sq_tiles_view_f32(const float *src, float *dst, int N, int T, int E, int op, int inverse, int accumulate, void *stream);
int sq_stitch_probs(const float *tile_logits, const int32_t *ymap, const int32_t *xmap, uint8_t *mask_out, void *prob_out,
                    int prob_dtype, float inv_n, int F, int H, int W, int TR, int TC, int TS, int K, void *stream);

/* ------------------------------------------------------------------------------------------
 * Seam blending: sq_stitch_probs with more than one tile per frame pixel (sequitr_amd/frontend.py: axis_blend,
 * FrameTiler.stitch_blend, segment_frames(blend=)).  Neighbouring tiles overlap by 2 * margin and see different context, so
 * their logits disagree a little and an owner-map stitch carries a step along every seam line; here the merged logits of
 * the overlapping tiles are mixed with integer tent weights before the argmax and the softmax.  Planar frames only: bricks
 * keep one owner per voxel.
 *
 * PER AXIS.  An axis of length L, tile T, margin m, the origins o[0 .. n-1] of the tile front end.  Tile k owns
 * [s[k], s[k+1]) with s[0] = 0, s[k] = o[k] + m for k >= 1 and s[n] = L: the runs the owner map encodes.  With a blend
 * width B the integer weight of tile k at frame coordinate p is
 *
 *     dl = p - s[k]            if k > 0      else +infinity
 *     dr = s[k+1] - 1 - p      if k < n - 1  else +infinity
 *     w_k(p) = clamp(min(dl, dr) + B + 1, 0, 2B + 1)
 *
 * B must satisfy 0 <= B <= m, 2B <= T - 2m and B <= 255.  Then: w_k(p) > 0 only inside tile k, and for k > 0 only at local
 * coordinates >= m - B (the outer m - B pixels of a tile are never used); the owner's weight is >= B + 1; the tiles with a
 * positive weight at p are consecutive and at most 3 (three where the last tile is clamped to L - T and its neighbour's run
 * is shorter than 2B: L = 53, T = 16, m = 4, B = 4 has origins 0, 8, 16, 24, 32, 37 and weight sums 10, 11, 10 at
 * p = 37, 38, 39); at a regular seam s, pixel s + j with -B <= j < B gets the weights B - j and B + j + 1, sum 2B + 1;
 * with B = 0 every pixel has its owner with weight 1 and nothing else.
 *
 * PER PIXEL.  KY and KX are the contributing tiles (positive weight) along y and x, each ascending; acc is the MERGE of
 * "Tile views and probability stitch".  In float32, contraction off:
 *
 *     S_c = +0.0f
 *     for ky in KY ascending: for kx in KX ascending:
 *         S_c = S_c + (float)(wy * wx) * acc[tile(f, ky, kx), y - oy[ky], x - ox[kx], c]
 *     Wt  = (float)(sum(wy over KY) * sum(wx over KX))        exact: < 2^24
 *     b_c = S_c / Wt
 *
 * Terms with zero weight are not read and not added: a NaN in a tile that does not contribute does not show.  A pixel
 * with one contributor goes through the same expression, b_c = (w * acc_c) / w.
 *
 * MASK is sq_argmax_u8's loop on b_0 .. b_{K-1}; PROBABILITIES the text of "Tile views and probability stitch" with
 * l_k = b_k * inv_n, its bound against the float64 softmax of those l_k unchanged.  At B = 0 both outputs are
 * sq_stitch_probs' bit for bit (w = Wt = 1; +0 + (-0) = +0 changes no comparison and no expf).
 *
 * SLOTS.  yslots / xslots are (L, 3, 2) int32 tables built on the host: per coordinate three slots of
 * (tile << 16 | local coordinate, weight), the contributors first in ascending tile order, unused slots (0, 0).
 *
 *   sq_blend_axis_slots : host only, no HIP call: fills slots (L, 3, 2) in host memory for one axis and returns the number
 *                         of tiles n, or SQ_EINVAL (slots untouched) for a null pointer, T outside 1 .. 65535, T > L,
 *                         margin outside 0 <= 2 margin < T, blend outside the range above, or more than 65535 tiles.
 *   sq_stitch_blend     : mask_out (F, H, W) uint8 and / or prob_out (F, K, H, W) of prob_dtype SQ_PIX_U8 or SQ_PIX_F32
 *                         from tile_logits (F*TR*TC, TS, TS, K) = acc, as defined above.  Either output may be NULL, not
 *                         both.  K is 1 .. 16, inv_n in (0, 1]; F * H <= 2^31 - 1; tile_logits 16-byte aligned, the slot
 *                         tables 8-byte aligned (a slot is read as one pair of words; else SQ_EINVAL).  The tables are
 *                         trusted as sq_stitch_masks_u8 trusts its maps.  One frame pixel per lane; a wave none of whose
 *                         pixels lies in a blend band reads one tile per pixel, as sq_stitch_probs does.  No allocation,
 *                         no synchronisation: the same under graph capture.
 * ---------------------------------------------------------------------------------------- */
int sq_blend_axis_slots(int L, int T, int margin, int blend, int32_t *slots);
int sq_stitch_blend(const float *tile_logits, const int32_t *yslots, const int32_t *xslots, uint8_t *mask_out, void *prob_out,
                    int prob_dtype, float inv_n, int F, int H, int W, int TR, int TC, int TS, int K, void *stream);

/* ------------------------------------------------------------------------------------------
 * Frame cleaning: the pipes the reference applies to raw microscope frames in front of ImageNorm, per whole frame,
 * in the order ImageOutliers -> ImageBlur -> ImageBGSubtract -> ImageNorm (sequitr_amd/frontend.py: FrameClean,
 * FrameTiler).
 *   sq_frame_outliers_f32 : ImageOutliers (sequitr/pipeline.py:266-295: median_filter(image, sigma), then
 *                           image[|image - med| > threshold] = med).  frames (F,H,W) SQ_PIX_* -> out (F,H,W) f32,
 *                           BIT-EXACT: x = the pixel as float32; med = the element of rank size*size/2 (0-based,
 *                           ascending) of the size x size window at offsets -(size/2) .. size-1-(size/2) along both
 *                           axes, indices outside the frame mirrored with the edge pixel repeated (i < 0 -> -i-1,
 *                           i >= L -> 2L-1-i: scipy's mode='reflect'); out = |x - med| > threshold ? med : x in
 *                           float32.  For size 2 the window is the pixel with its upper and left neighbours and med
 *                           the third smallest of the four.  size is 2 .. 5 and min(H, W) >= size (one reflection).
 *   sq_frame_bgfit_f64    : ImageBGSubtract's fit (sequitr/pipeline.py:360-401: least squares of 1, u, v, u^2, uv, v^2
 *                           over all pixels, u the column, v the row), in fp64 and in centred, scaled coordinates
 *                               s = (u - (W-1)/2) / ((W-1)/2),  t = (v - (H-1)/2) / ((H-1)/2)   (both in [-1, 1]):
 *                           coef (F,6) float64 with  bg(u, v) = c0 + c1 s + c2 t + c3 s^2 + c4 s t + c5 t^2.
 *                           It is the reference's surface (the same polynomial space); the reference inverts A^T A in
 *                           raw pixel coordinates, whose condition number grows as L^8.  Partial sums per strip of rows
 *                           go to the workspace (sq_frame_bgfit_workspace bytes) and are added in a fixed order: results
 *                           are the same bits on every run, and frame f's do not depend on F.  H, W >= 3, H*W <= 2^24.
 *   sq_frame_bg_stats_f64 : float64 mean and standard deviation (np.std's definition) of the residual
 *                           r = (double)x - bg(u, v) per frame; same workspace, same fixed-order reduction.
 *   sq_frames_to_tiles_bg : sq_frames_to_tiles' geometry on the residual (sequitr/pipeline.py:402-405, then :350-356):
 *                           (float)((r - mean[f]) / (1e-99 + stdv[f])) evaluated in fp64, or (float)r when
 *                           mean == stdv == NULL.  The reference's result after ImageBGSubtract is float64; this is
 *                           where the chain's one rounding to the network's float32 happens.  The kernel is
 *                           sq_frames_to_tiles_mc's in mode SQ_CH_BG / SQ_CH_BG_NORM with C = 1 ("Tile front end"): the
 *                           surface is evaluated by rows with every multiply-add one fused operation, as stated there.
 *   sq_frame_blur_f32     : ImageBlur (sequitr/pipeline.py:244-263: gaussian_filter(image, sigma) per channel).  frames
 *                           (F,H,W) SQ_PIX_* -> out (F,H,W) f32, never aliasing frames, BIT-EXACT with scipy's
 *                           gaussian_filter of the float32 plane, whose radius is R = int(4.0 * sigma + 0.5).  `weights`
 *                           is a HOST array of radius + 1 doubles, w[0] the centre, read before the launch and carried
 *                           in the kernel arguments by value (a captured graph replays them).  The caller computes them
 *                           in numpy float64 with scipy's own expressions (the library never calls exp: the last bit of
 *                           two libms may differ):
 *                               x = np.arange(-R, R + 1); phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
 *                               phi /= phi.sum(); w[k] = phi[R + k], k = 0 .. R
 *                           One pass along an axis of length L, for each output i:
 *                               acc = (double)a[i] * w[0]
 *                               for k = R, R-1, .. 1:  acc = acc + ((double)a[refl(i-k)] + (double)a[refl(i+k)]) * w[k]
 *                           the add, the multiply and the add three separate float64 roundings (no fused multiply-add:
 *                           the kernel is compiled with contraction off), the result rounded once to float32.  refl is
 *                           scipy's mode='reflect' repeated until the index is inside (i < 0 -> -i-1, i >= L -> 2L-1-i;
 *                           L == 1 -> 0): a frame may be far smaller than R.  The first pass runs along axis 0 (down
 *                           the columns) over the pixel cast to float32, the second along axis 1 over the float32
 *                           result of the first; that intermediate rounding is part of the definition.  radius 0
 *                           (sigma < 0.125) still multiplies by w[0] == 1.0.  One launch; the intermediate lives in LDS.
 *                           Refused before any launch: radius outside 0 .. 32 (sigma >= 8.125), a weight that is not
 *                           finite, F outside 1 .. 65535, H or W < 1, H*W > 2^24, an unknown pixel type, a null pointer.
 *                           On the device the order is ImageOutliers -> ImageBlur -> ImageBGSubtract -> ImageNorm: after
 *                           hot-pixel removal, which a blur would smear, before the fit and the statistics, which see
 *                           the blurred frame.
 * F <= 65535 (a grid dimension).
 * ---------------------------------------------------------------------------------------- */
int sq_frame_blur_f32(const void *frames, int dtype, float *out, const double *weights, int radius, int F, int H, int W,
                      void *stream);
int sq_frame_outliers_f32(const void *frames, int dtype, float *out, int F, int H, int W, int size, float threshold,
                          void *stream);
int64_t sq_frame_bgfit_workspace(int F, int H, int W);
int sq_frame_bgfit_f64(const float *frames, double *coef, void *workspace, int F, int H, int W, void *stream);
int sq_frame_bg_stats_f64(const float *frames, const double *coef, double *mean, double *stdv, void *workspace, int F,
                          int H, int W, void *stream);
int sq_frames_to_tiles_bg(const float *frames, const double *coef, const double *mean, const double *stdv,
                          const int32_t *oy, const int32_t *ox, float *tiles, int F, int H, int W, int TR, int TC, int TS,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Volume front end: raw single-channel volumes (V, Z, X, Y) in HBM -> ImageNorm per volume -> network bricks, and
 * the brick-shaped network output back into full-volume arrays (sequitr_amd/frontend.py: volume_bricks, VolumeTiler).
 * A volume has KZ x KX x KY bricks of (BZ, BX, BY) voxels, numbered (v, kz, kx, ky) row-major.  `geom` is one int32
 * array in HBM of 3 * (KZ + KX + KY) entries: the brick origins along z, x, y, then the first coordinate each brick
 * owns along z, x, y, then one past the last (absolute coordinates; the owned boxes of a volume partition it).  An axis
 * shorter than the brick has one brick at origin 0 that owns the whole axis.
 *   sq_volume_stats     : per-volume float32 mean and std EXACTLY as np.mean / np.std of the float32 volume: float32
 *                         pairwise sums per 8192-element chunk added in order, the division by nvox in double
 *                         (numpy divides by an integer count), which sq_frame_stats' float32 division equals only up
 *                         to 2^24 elements.  nvox <= 2^40; workspace: sq_volume_stats_workspace bytes.
 *   sq_volume_to_bricks : out (count, BZ, BX, BY) f32 = bricks first .. first+count-1: (x - mean[v]) / std[v], or the
 *                         plain cast when mean == std == NULL; 0.0f where the brick reaches beyond the volume.
 *   sq_bricks_scatter_* : every brick's owned box copied from bricks (count, BZ, BX, BY[, C]) into out (V, Z, X, Y[, C]);
 *                         owned boxes are disjoint, so batches may be scattered in any order.
 * count <= 65535 and BZ <= 65535 (grid dimensions).
 * ---------------------------------------------------------------------------------------- */
int64_t sq_volume_stats_workspace(int V, int64_t nvox);
int sq_volume_stats(const void *vols, int dtype, float *mean, float *stdv, void *workspace, int V, int64_t nvox,
                    void *stream);
int sq_volume_to_bricks(const void *vols, int dtype, const float *mean, const float *stdv, const int32_t *geom, float *out,
                        int V, int Z, int X, int Y, int KZ, int KX, int KY, int BZ, int BX, int BY, int64_t first,
                        int count, void *stream);
int sq_bricks_scatter_u8(const uint8_t *bricks, const int32_t *geom, uint8_t *out, int V, int Z, int X, int Y, int KZ,
                         int KX, int KY, int BZ, int BX, int BY, int64_t first, int count, void *stream);
int sq_bricks_scatter_f32(const float *bricks, const int32_t *geom, float *out, int V, int Z, int X, int Y, int KZ, int KX,
                          int KY, int BZ, int BX, int BY, int C, int64_t first, int count, void *stream);

/* ------------------------------------------------------------------------------------------
 * Volume sampler: the training counterpart of the volume front end (sequitr/pipeline.py: ImageSample crops random ROIs
 * and repeats the coordinates for labels and weights, ImageFlip mirrors, ImageRotate turns; sequitr_amd/frontend.py:
 * sample_plan, VolumeSampler).  Volumes, labels and weight maps (V, Z, X, Y[, ...]) stay in HBM; a SAMPLE PLAN is an int32
 * array (count, 5) in HBM with rows [v, oz, ox, oy, op]: the volume, the origin of a (BZ, BX, BY) box in the array's
 * (Z, X, Y) order, and a 4-bit symmetry -- bit 0 flips z, bit 1 flips x, bit 2 flips y, bit 3 transposes x and y.  As
 * numpy says it:
 *
 *     box = zero-padded crop vol[v, oz:oz+BZ, ox:ox+BX, oy:oy+BY]      # fill where the box leaves the volume
 *     if op & 8: box = box.transpose(0, 2, 1)                          # needs BX == BY
 *     if op & 1: box = box[::-1];  if op & 2: box = box[:, ::-1];  if op & 4: box = box[:, :, ::-1]
 *
 * that is out[z, x, y] = box[fz(z), a, b] with (a, b) = (fx(x), fy(y)), or (fy(y), fx(x)) under bit 3, f the identity
 * or the mirror of its axis.  The 16 ops are the group the three flips and the in-plane transpose generate; it holds
 * every in-plane quarter turn, and every op is exact (no interpolation).
 *   sq_volume_sample_f32       : raw SQ_PIX_* volumes -> out (count, BZ, BX, BY) f32 = (x - mean[v]) / std[v] (the
 *                                expression of sq_volume_to_bricks: op 0 at a brick's origin gives that brick bit for
 *                                bit), or the plain cast when mean == std == NULL; fill 0.0f.
 *   sq_volume_sample_copy      : voxels of elem_bytes in {1, 2, 3, 4, 8} bytes moved verbatim (4: the f32 weight map, C:
 *                                one-hot uint8 labels of C classes); fill zero bytes.
 *   sq_volume_sample_onehot_u8 : class-index labels (V, Z, X, Y) uint8 -> out (count, BZ, BX, BY, C) uint8,
 *                                out[..., c] = (label == c), C in 1 .. 16; fill all zero.
 * `plan` points at the first of `count` rows.  The plan is data in HBM, so the kernels trust none of it: a coordinate
 * outside the volume -- a negative origin, one beyond the volume, v outside 0 .. V-1 -- reads as fill, no load leaves
 * the volumes.  Bits of op above bit 3 are ignored.  allow_transpose != 0 requires BX == BY (refused before any launch
 * otherwise); with allow_transpose == 0 any BX, BY are taken and bit 3 is ignored.  count <= 65535 and BZ <= 65535
 * (grid dimensions).  Transposed ops go through padded LDS tiles, so that global loads and stores both run along the
 * contiguous axis; SQ_SAMPLE_LDS=0 (read per launch) gathers them directly instead, with the same bits.
 * ---------------------------------------------------------------------------------------- */
int sq_volume_sample_f32(const void *vols, int dtype, const float *mean, const float *stdv, const int32_t *plan, float *out,
                         int V, int Z, int X, int Y, int BZ, int BX, int BY, int count, int allow_transpose, void *stream);
int sq_volume_sample_copy(const void *src, int elem_bytes, const int32_t *plan, void *out, int V, int Z, int X, int Y,
                          int BZ, int BX, int BY, int count, int allow_transpose, void *stream);
int sq_volume_sample_onehot_u8(const uint8_t *labels, int C, const int32_t *plan, uint8_t *out, int V, int Z, int X, int Y,
                               int BZ, int BX, int BY, int count, int allow_transpose, void *stream);

/* ------------------------------------------------------------------------------------------
 * Brick views and probability scatter: "Tile views and probability stitch" for volumes -- test-time augmentation and class
 * probability maps for UNet3D on whole volumes (sequitr_amd/frontend.py: VolumeTiler.view, VolumeTiler.scatter_probs,
 * segment_volumes(tta=, probabilities=)).  The volume sampler trains on exactly these symmetries; here a trained net is
 * evaluated under them and its logits averaged, all in HBM.
 *
 * VIEWS.  A brick batch is (N, BZ, BX, BY, E) float32, contiguous, E interleaved elements per voxel, 1 <= E <= 16.  op is
 * the sample plan's 4-bit symmetry, the bits and the meaning of "Volume sampler": bit 0 flips z, bit 1 flips x, bit 2
 * flips y, bit 3 transposes x and y and needs BX == BY.  In numpy, per brick b of shape (BZ, BX, BY, E):
 *
 *     if op & 8: b = b.transpose(0, 2, 1, 3)
 *     if op & 1: b = b[::-1];  if op & 2: b = b[:, ::-1];  if op & 4: b = b[:, :, ::-1]
 *
 * that is view_op(b)[z, x, y, e] = b[fz(z), a, b, e] with (a, b) = (fx(x), fy(y)), or (fy(y), fx(x)) under bit 3.
 * unview_op is the inverse, and the inverse of an op is an op:  unview_op == view_op'  with
 *
 *     op   0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15
 *     op'  0  1  2  3  4  5  6  7  8  9 12 13 10 11 14 15
 *
 * (the mirrors commute and are involutions; carried through the transpose the x and y mirrors change places, so bits 1
 * and 2 swap under bit 3: 8, 9, 14, 15 are reflections about a diagonal or half turns with it, 10 <-> 12 and 11 <-> 13
 * the quarter turns).  In a slice, op >> 1 names the element of the square's group that the planar section's op names,
 * except that the planar op mirrors before it transposes: planar (bit 0, bit 1) are this section's (bit 2, bit 1) under
 * the transpose and (bit 1, bit 2) without it.
 *
 * SETS.  tta = None: ops (0);  'flips': ops (0 .. 7), the three mirrors, any brick;  'dihedral': ops (0 .. 15), requires
 * BX == BY.  So n is 1, 8 or 16, 1/n a power of two, the mean an exact scaling.
 *
 * MERGE.  With L_op = net.build(view_op(bricks)):
 *     acc = unview_0(L_0)
 *     acc = acc + unview_op(L_op)        for op ascending, one float32 add per element per op
 * in that order: deterministic, run-to-run identical.  mean = acc * (1/n) is exact.
 *
 * MASK and PROBABILITIES.  The planar section's rules, word for word, on the K values acc holds for a voxel in its owner
 * brick: the class is sq_argmax_u8's loop (ties to the lowest class, NaN never wins, a row that starts with NaN gives
 * class 0); l_k = acc_k * inv_n, m = l_pc, e_k = expf(l_k - m), s = e_0 + ... + e_{K-1} in index order, p_k = e_k / s, in
 * float32 with contraction off; a row whose m is not finite, or that holds a NaN, gives NaN in every class; SQ_PIX_U8
 * writes (uint8) floorf(p_k * 255 + 0.5f) and 0 for NaN; every finite p_k is within (K + 4) * 2^-23 of the float64
 * softmax.  The owner of a voxel comes from `geom` exactly as sq_bricks_scatter_* reads it ("Volume front end": the owned
 * boxes of a volume partition it; no seam blending).  With n = 1 the mask is sq_bricks_scatter_u8 of sq_argmax_u8, byte
 * for byte.  Probability output is planar per volume: (V, K, Z, X, Y).
 *
 *   sq_bricks_view_f32      : dst = view_op(src), or unview_op(src) when inverse != 0; dst += ... when accumulate != 0
 *                             (every element read, changed and written by exactly one thread, once).  Refused before any
 *                             launch, dst untouched: a null pointer, src and dst the same or overlapping, op outside
 *                             0 .. 15, bit 3 with BX != BY, E outside 1 .. 16, a dimension < 1, BX or BY > 65535,
 *                             N * BZ * BX > 2^31 - 1, pointers not 16-byte aligned (SQ_EALIGN).  It is sq_tiles_view_f32's
 *                             kernel family on N * BZ slices with the slice remapped under bit 0 (sq_tiles_view_f32 is its
 *                             BZ = 1, BX = BY case, instantiated with those fixed at compile time): ops 0 .. 7 are row streams, any BX, BY, with 16-byte accesses where E
 *                             and BY allow (E % 4 == 0, or BY * E % 4 == 0 with no mirror of y or E <= 2), one float
 *                             otherwise; ops 8 .. 15 go per slice through the padded LDS block of sq_tiles_view_block(E)
 *                             pixels a side, and SQ_TTA_LDS=0 (read per call) gathers them directly instead, with the same
 *                             bits.  No allocation, no synchronisation: the same under graph capture.
 *   sq_bricks_scatter_probs : for bricks first .. first+count-1 with brick_logits (count, BZ, BX, BY, K) = acc, every voxel
 *                             of each brick's owned box -- clamped into brick and volume, whatever the table says -- gets
 *                             its class in mask_out (V, Z, X, Y) uint8 and / or its K probabilities in prob_out
 *                             (V, K, Z, X, Y) of prob_dtype SQ_PIX_U8 or SQ_PIX_F32; nothing else is written, so batches
 *                             may be scattered in any order.  Either output may be NULL, not both.  K is 1 .. 16, inv_n in
 *                             (0, 1]; count <= 65535 and BZ <= 65535 (grid dimensions); brick_logits 16-byte aligned.
 *                             Refused before any launch, outputs untouched.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------- */
int sq_bricks_view_f32(const float *src, float *dst, int N, int BZ, int BX, int BY, int E, int op, int inverse,
                       int accumulate, void *stream);
int sq_bricks_scatter_probs(const float *brick_logits, const int32_t *geom, uint8_t *mask_out, void *prob_out,
                            int prob_dtype, float inv_n, int V, int Z, int X, int Y, int KZ, int KX, int KY, int BZ, int BX,
                            int BY, int K, int64_t first, int count, void *stream);

/* ------------------------------------------------------------------------------------------
 * Tile sampler: the planar twin of the volume sampler, and the one interpolating op of the pipeline -- the reference's
 * tr_augment (sequitr/networks/unet.py:348-401: per element one random angle, image and weight map rotated bilinearly,
 * labels by nearest neighbour, 1 - rotate(ones, NEAREST) added to the weights, a random crop of the network's shape,
 * one-hot labels; sequitr_amd/frontend.py: tile_sample_plan, TileSampler).  Raw frames (F, H, W) SQ_PIX_*, class-index
 * labels (F, H, W) uint8 and weight maps (F, H, W) f32 stay in HBM.  A sample is two rows in HBM:
 *     plan[k] = [f, oy, ox, 0]  int32 (the fourth entry is reserved and ignored),
 *     coef[k] = [a0, a1, a2, b0, b1, b2]  float32.
 * TensorFlow's parity is unpinned; this text is the contract.  It restates TF 1.x's angles_to_projective_transforms and
 * ImageProjectiveTransform.  For pixel (i, j) of sample k, with tiles of (TH, TW) and frames (F, H, W):
 *
 *     x = float32(ox + j);  y = float32(oy + i)
 *     sx = (a0*x + a1*y) + a2;   sy = (b0*x + b1*y) + b2     # float32, every * and + rounded on its own, no FMA
 *     read_T(r, c) = T[f, r, c] if 0 <= f < F and 0 <= r < H and 0 <= c < W else 0
 *     bilinear(T):  x0 = floor(sx), y0 = floor(sy), x1 = x0 + 1, y1 = y0 + 1
 *         top = (x1 - sx) * read_T(y0, x0) + (sx - x0) * read_T(y0, x1)
 *         bot = (x1 - sx) * read_T(y1, x0) + (sx - x0) * read_T(y1, x1)
 *         val = (y1 - sy) * top + (sy - y0) * bot
 *     nearest:  r = roundf(sy), c = roundf(sx)  (half away from zero);  inside = (r, c) in the frame and 0 <= f < F
 *     image  [k,i,j,0] = bilinear(normalised frame)
 *     onehot [k,i,j,q] = (read_labels(r, c) == q)                            # label 0 outside; label >= C: all zero
 *     weights[k,i,j,0] = bilinear(weight map) + (inside ? 0.0f : 1.0f)
 *
 * Normalised frame: a frame pixel read for the image is (float(v) - mean[f]) / std[f], sq_frames_to_tiles' expression with
 * sq_frame_stats' statistics of the whole frame, or the plain cast when mean == std == NULL; a corner outside the frame
 * reads 0.0f, the frame's mean.  ox + j and oy + i are exact integer sums, rounded once to float32.  A pixel whose sx or
 * sy is NaN, or at or beyond +-2^23, reads fill everywhere: image 0, label 0, weight 1.  No load ever leaves the arrays:
 * plan and coef are data, and the kernel trusts none of it.  The kernel knows nothing about angles; it takes any affine
 * rows (tile_sample_plan writes a rotation about the frame's centre, optionally composed with mirrors of the tile).
 *   sq_tile_sample_affine : out_image (count, TH, TW) f32, out_onehot (count, TH, TW, C) uint8, out_weights
 *                           (count, TH, TW) f32, one launch.  Each of the pairs (frames, out_image), (labels, out_onehot),
 *                           (weights, out_weights) may be NULL together, which skips that output; any other NULL, a
 *                           half-NULL pair, C outside 1 .. 16, count outside 1 .. 65535, a non-positive size or
 *                           H*W > 2^24 is refused before any launch.
 * A block owns a 32 x 32 patch of one tile, so that its source footprint is compact at any angle, and gathers the four
 * corners of every pixel directly.  With SQ_ROTATE_LDS=1 (read per launch) it stages the bounding box of the patch's
 * footprint (the four corner coordinates, plus the bilinear apron) into LDS with loads that run along the frame's rows,
 * and interpolates from there; a block whose box exceeds 48 x 48 pixels (a zooming or shearing row) still gathers
 * directly.  SQ_ROTATE_LDS=0 selects the direct gather everywhere.  Unset is the direct gather, the faster form as
 * measured (tools/tile_sampler_bench.py); both give the same bits.
 *   sq_tile_sample_affine_mc : sq_tile_sample_affine with CI image channels, 1 .. 8.  frames are channel-major planes
 *                           ("Tile front end": channel c of frame f at c * chan_stride + f * H * W, chan_stride >= F*H*W),
 *                           mean and stdv are (CI, F), out_image is (count, TH, TW, CI) interleaved.  sx, sy, the corner
 *                           indices and the bilinear weights are computed once per pixel and applied to every channel
 *                           with the same float32 expressions; labels, weights, plan, coef, the fill rules, the NaN and
 *                           +-2^23 rule, "no load ever leaves the arrays" and SQ_ROTATE_LDS are the contract above, word
 *                           for word (under SQ_ROTATE_LDS=1 the planes pass through the staging buffer one after the
 *                           other and the image is stored one channel per pass, CI floats apart; only the default
 *                           direct form was timed for this entry, tools/multichannel_bench.py).  Channel c is what
 *                           sq_tile_sample_affine gives on channel c's stack -- the same kernel: sq_tile_sample_affine
 *                           is this entry with CI == 1 and chan_stride = F*H*W.  CI outside 1 .. 8 or chan_stride < F*H*W (with
 *                           frames given) is refused before any launch, next to everything the entry above refuses.
 * ---------------------------------------------------------------------------------------- */
int sq_tile_sample_affine(const void *frames, int dtype, const float *mean, const float *stdv, const uint8_t *labels,
                          const float *weights, const int32_t *plan, const float *coef, float *out_image,
                          uint8_t *out_onehot, float *out_weights, int F, int H, int W, int TH, int TW, int C, int count,
                          void *stream);
int sq_tile_sample_affine_mc(const void *frames, int dtype, int64_t chan_stride, const float *mean, const float *stdv,
                             const uint8_t *labels, const float *weights, const int32_t *plan, const float *coef,
                             float *out_image, uint8_t *out_onehot, float *out_weights, int F, int H, int W, int CI, int TH,
                             int TW, int C, int count, void *stream);

/* ------------------------------------------------------------------------------------------
 * GAN sampler: the progressive GAN's real images, the third sampler -- the reference's input pipeline in front of its
 * discriminator (sequitr/networks/gan.py:347-407 and :682-684: every image normalised per channel by its own moments,
 * tf.nn.moments(img, axes=[0,1]) and batch_normalization(..., 1e-8); shuffled; a random crop; two random mirrors; a
 * bilinear tf.image.resize_images(..., align_corners=True) to the current level's size; sequitr_amd/frontend.py:
 * gan_sample_plan, GanSampler).  Raw image stacks (N, H, W, C), channels interleaved, C in 1 .. 4, stay in HBM.
 * TensorFlow's parity is unpinned; this text is the contract.
 *   sq_gan_image_stats : per-(image, channel) moments of SQ_PIX_U8 or SQ_PIX_U16 images, H*W <= 2^24.  The sums are EXACT
 *                        integers, S1 = sum v and S2 = sum v^2 over the n = H*W pixels in uint64, accumulated with integer
 *                        adds and integer atomics: the result does not depend on any order and is the same bits on every
 *                        run.  A finishing step computes in float64, no FMA contraction,
 *                            mean = S1 / n;   var = max(S2 / n - mean * mean, 0);   inv = 1 / sqrt(var + 1e-8)
 *                        (S1, S2 and n converted to float64, round to nearest even) and stores float32(mean) and
 *                        float32(inv) as (N, C) arrays.  The clamp matters: a nearly constant uint16 image can round the
 *                        difference below zero.  workspace: sq_gan_image_stats_workspace bytes, 8-byte aligned, cleared
 *                        by the call.  SQ_PIX_F32 is refused here: float32 pixels are sampled with the caller's own
 *                        statistics or with none.
 *   sq_gan_sample_f32  : out (count, SH, SW, C) f32 from a SAMPLE PLAN, an int32 array (count, 4) in HBM with rows
 *                        plan[k] = [n, oy, ox, bits]: the image, the origin of a (CH, CW) crop, bit 0 mirrors the crop along
 *                        x, bit 1 along y (higher bits are ignored).  One launch.  For output pixel (i, j) and channel c:
 *
 *     sy = SH > 1 ? float32(CH-1) / float32(SH-1) : 0.0f      (sx likewise from CW, SW)
 *     py = float32(i) * sy;  y0 = floor(py);  y1 = min(ceil(py), CH-1);  ly = py - y0     (x likewise)
 *     crop(r, q) = src(oy + (bits&2 ? CH-1-r : r), ox + (bits&1 ? CW-1-q : q))
 *     src(Y, X)  = (float32(v[n,Y,X,c]) - mean[n,c]) * inv[n,c]   if 0<=n<N, 0<=Y<H, 0<=X<W   else 0.0f
 *                  (plain cast when mean == inv == NULL)
 *     tl = crop(y0, x0), tr = crop(y0, x1), bl = crop(y1, x0), br = crop(y1, x1)
 *     top = tl + (tr - tl) * lx;  bot = bl + (br - bl) * lx;  out = top + (bot - top) * ly
 *
 * Every *, + and - is rounded on its own in float32, no FMA.  This restates TF 1.x ResizeBilinear with align_corners=True
 * applied to the flipped crop of the normalised image: crop -> flips -> resize is the reference's order.  With SH == CH and
 * SW == CW the lerps are 0 and the output is the normalised crop bit for bit.  The plan is data: no load leaves the arrays,
 * and a row or a corner that points outside -- n outside 0 .. N-1, a negative origin, a crop larger than the image -- reads
 * 0.0f, the image's mean.  mean and inv are (N, C) f32, sq_gan_image_stats' or the caller's own.
 * Refused before any launch: a NULL images, plan or out, a half-NULL (mean, inv) pair, C outside 1 .. 4, count outside
 * 1 .. 65535, a non-positive size, H*W > 2^24, a crop axis above 2^24, SH*SW > 2^24, count*SH*SW >= 2^31.  A pixel's C
 * channels are one load and its C floats one store where C is 1, 2 or 4, so images, out, mean and inv must be aligned to
 * C of their elements there (to one element for C = 3).
 * One thread per output pixel over the flat (k, i, j) index, stores along j; the kernel is launch- and gather-bound.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_gan_image_stats_workspace(int N, int C);
int sq_gan_image_stats(const void *images, int dtype, float *mean, float *inv, void *workspace, int N, int H, int W, int C,
                       void *stream);
int sq_gan_sample_f32(const void *images, int dtype, const float *mean, const float *inv, const int32_t *plan, float *out,
                      int N, int H, int W, int C, int CH, int CW, int SH, int SW, int count, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scoring: confusion counts of predictions against labels, both in HBM -- the counterpart of the reference's
 * sequitr/confusion.py, which hands host arrays to scikit-learn (sequitr_amd/confusion.py: confusion_counts,
 * ConfusionMeter, scores).  One streaming pass; every quantity is an integer count, so this text is exact.
 *   sq_confusion : `items` rows of `n` pixels or voxels each (a row is a tile, a whole frame or a whole volume; n is an
 *                  int64, up to 2^44).  For pixel p of item i, with C classes:
 *
 *     pc = SQ_PRED_MASK       : pred  uint8 (items, n),     pc = pred[i, p]
 *          SQ_PRED_LOGITS_F32 : pred  float32 (items, n, C), best = 0; for c = 1 .. C-1: if (z[c] > z[best]) best = c; pc = best
 *     tc = SQ_TRUTH_INDEX     : truth uint8 (items, n),     tc = truth[i, p]
 *          SQ_TRUTH_ONEHOT    : truth uint8 (items, n, C),  tc = the lowest c with truth[i, p, c] != 0; none: no class
 *     tc < C and pc < C  ?  counts[i, tc, pc] += 1  :  ignored[i] += 1
 *
 *                  The logits rule is sq_argmax_u8's loop: ties go to the lowest index, a NaN never wins a comparison (a row
 *                  that starts with NaN is class 0), and -0 == +0; for every input pc is the class sq_argmax_u8 writes, and no
 *                  mask is materialised.  An all-zero one-hot row is what the trainer's label format holds for labels >= C.
 *                  counts is int64 (items, C, C), row = truth, column = prediction (scikit-learn's convention); ignored is
 *                  int64 (items): the pixels whose truth has no class or is >= C and the mask pixels >= C.  Those touch no
 *                  counts cell, so counts[i].sum() + ignored[i] grows by exactly n per call.  The call ADDS to both arrays:
 *                  the caller zeroes them, and the batches of a stream accumulate into the same rows.  Integer adds only
 *                  (LDS and global atomics): the result depends on no order and is the same bits on every run.
 *                  Refused before any launch: a NULL pointer, an unknown kind, C outside 1 .. 16, a negative items or n,
 *                  counts or ignored not aligned to 8 bytes, logits not aligned to 4.  items == 0 or n == 0 is a no-op that
 *                  returns 0.  pred (masks) and truth may start at ANY byte address and n may be odd: see below.
 *   sq_confusion_chunk : the pixels of one item a block counts before it flushes, for this (items, n): 16384, doubled while
 *                  the call would have more than 2^22 chunks, at most 2^30.  0 for an empty call.
 * A block owns one chunk of one item -- it never straddles two -- and counts it into an LDS histogram of C*C + 1 bins of
 * 32-bit counters, 32 counters per bin so that the lanes of an LDS lane group always sit on different banks; it then issues
 * at most C*C + 1 global 64-bit atomic adds.  There is no global atomic per pixel.  Overflow bound: a block's counters see
 * at most one chunk <= 2^30 pixels between two flushes, below the 2^32 a counter holds.  Chunks beyond 65536 blocks are a
 * grid-stride loop, so any `items` is one launch.
 * Alignment: masks against index labels read 16 pixels per lane.  A block takes the pixels up to the first 16-byte boundary
 * of its pred range one per thread, then 16-byte vectors (pred aligned; truth aligned too when both bases are congruent mod
 * 16, otherwise the same load at an unaligned address), then the tail one per thread.  The other pairs walk one pixel per
 * lane and read its C floats or C bytes as the widest vector that divides a pixel and that every row base is aligned to.
 * No load leaves [base, base + items * n * bytes per pixel).
 * ---------------------------------------------------------------------------------------- */
#define SQ_PRED_MASK 0
#define SQ_PRED_LOGITS_F32 1
#define SQ_TRUTH_INDEX 0
#define SQ_TRUTH_ONEHOT 1
int64_t sq_confusion_chunk(int64_t items, int64_t n);
int sq_confusion(const void *pred, int pred_kind, const uint8_t *truth, int truth_kind, int64_t *counts, int64_t *ignored,
                 int64_t items, int64_t n, int C, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mask clean-up between "mask" and "objects": morphology, hole filling, border objects (sequitr_amd/maskops.py: morph,
 * fill_holes, clear_border, MaskCleanup; the frame jobs' `postprocess` key).  The reference has no counterpart: its
 * CentroidWriter (sequitr/utils.py:492-494) measures the raw argmax mask, and users ran scipy.ndimage on the host.  Planar
 * masks only: mask and out are (N, H, W) uint8 class labels with C classes, fewer than 2^31 elements; volumes are refused.
 * Every plane is Boolean, so every result is exact and the same bits on every run.
 *
 * Common definitions
 *   P_c = (mask == c) for c = 1 .. C-1.  Byte 0 is background.  Bytes >= C belong to no class: they are never processed,
 *   they are copied through unchanged and they are never overwritten; they count as "not background".
 *   "An object" has the centroid path's connectivity (sq_ccl.h): 4 neighbours, same class > 0.
 *   Every operation computes one processed plane Q_c per class from the INPUT mask, then merges:
 *     extensive operations (dilate, close, fill_holes -- they can add pixels):
 *         out = mask wherever mask > 0, elsewhere the smallest c whose Q_c is set, else 0.
 *         A clean-up step never changes a pixel that already carries a class or an unknown byte.
 *     anti-extensive operations (erode, open, clear_border -- they can only remove pixels):
 *         out = c where Q_c is set and mask == c, else 0; bytes >= C stay.
 *
 * sq_mask_morph_u8 : op = SQ_MORPH_ERODE / DILATE / OPEN / CLOSE, structure = SQ_MORPH_CROSS
 *   (scipy.ndimage.generate_binary_structure(2, 1)) or SQ_MORPH_SQUARE ((2, 2)), iterations r = 1 .. SQ_MORPH_MAX_ITER.
 *     Q_c = scipy.ndimage.binary_{erosion,dilation,opening,closing}(P_c, structure, iterations=r)
 *   with scipy's defaults (border_value = 0, origin 0): every one of the r (or r + r) elementary 3x3 steps sees zeros
 *   outside the frame, so erosion eats in from the frame edge and closing loses pixels near it -- harmless under the
 *   extensive merge rule for pixels that already carry a class.
 *   One launch reads the mask once and writes out once, whatever r and C are.  A block of 256 threads owns a tile of
 *   SQ_MORPH_TILE_ROWS x SQ_MORPH_TILE_COLS pixels, stages it with a halo of r (erode, dilate) or 2r (open, close) as bytes
 *   in LDS, and then per class present in the staged region: one __ballot of (byte == c) per 64-pixel row segment makes the
 *   row a 64-bit word, a 3x3 step is shifts with carry from the neighbouring words plus AND / OR with the rows above and
 *   below, between two LDS copies of the bit plane; a block's result is exact on its tile because an error at the staged
 *   region's rim travels one pixel per step and the halo is as wide as there are steps.  The classes are merged in
 *   registers and the tile is stored.  SQ_MORPH_MAX_ITER = 16 makes the widest halo 32 pixels: the staged region is at most
 *   (64 + 64) x (192 + 64) bytes = 32 KiB plus two bit planes of 4 KiB, 40 KiB of LDS per block.
 *   out must not overlap mask (a block reads its neighbours' tiles): overlap returns SQ_EINVAL.  No workspace.
 *
 * sq_mask_fill_holes_u8 : a hole of class c is a 4-connected component of ~P_c that touches none of the frame's outer rows
 *   and columns -- what scipy.ndimage.binary_fill_holes(P_c) fills.  Q_c = P_c plus the holes that qualify: all of them for
 *   max_area <= 0, otherwise those whose area is at most max_area pixels, where the area counts ALL pixels of the component,
 *   pixels of other classes and bytes >= C inside it included.  Extensive merge.  Per class: the complement plane is
 *   written, labelled with sq_ccl.h's row scan / merge / compress, the roots that own a pixel of the outer rows or columns
 *   are marked, the areas of the others are counted per root with integer atomics, and one pointwise pass writes c onto the
 *   background pixels of the qualifying components that no smaller class has taken.  The results are unique.
 *   workspace: sq_mask_fill_holes_workspace(N, H, W) bytes (-1: too large), 16-B aligned: 9 B per pixel.
 *
 * sq_mask_clear_border_u8 : removes every object that has a pixel in row 0, row H-1, column 0 or column W-1; the rest is
 *   unchanged (anti-extensive merge; bytes >= C stay).  The centroid path's labelling on the mask itself plus a flag per
 *   root.  workspace: sq_mask_clear_border_workspace(N, H, W) bytes (-1: too large), 16-B aligned: 8 B per pixel.
 *
 * All three return SQ_EINVAL with a message, before any launch, for null pointers, C < 2 or C > 256, a bad op, structure
 * or iterations, N, H or W < 1, 2^31 or more elements, a workspace that is not 16-B aligned, and out overlapping mask.
 * None reads anything back, and every call is a chain of kernel launches on `stream` and nothing else (the counts and flags
 * are cleared and the mask is copied by kernels, not by memset or memcpy calls): each can be captured in a graph and
 * replayed.  fill_holes and clear_border are the volume entries' implementation ("Volume clean-up" below) with D = 1 and
 * the four lateral faces as the border.
 * ---------------------------------------------------------------------------------------- */
#define SQ_MORPH_ERODE 0
#define SQ_MORPH_DILATE 1
#define SQ_MORPH_OPEN 2
#define SQ_MORPH_CLOSE 3
#define SQ_MORPH_CROSS 0
#define SQ_MORPH_SQUARE 1
#define SQ_MORPH_MAX_ITER 16
#define SQ_MORPH_TILE_ROWS 64
#define SQ_MORPH_TILE_COLS 192
int sq_mask_morph_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, int op, int structure, int iterations,
                     void *stream);
int64_t sq_mask_fill_holes_workspace(int N, int H, int W);
int sq_mask_fill_holes_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, int64_t max_area, void *workspace,
                          void *stream);
int64_t sq_mask_clear_border_workspace(int N, int H, int W);
int sq_mask_clear_border_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mask clean-up: splitting (sequitr_amd/maskops.py: split, the `split` step of MaskCleanup and of the frame jobs'
 * `postprocess` key).  Everything downstream of the mask calls a 4-connected component of one class "an object", so two
 * cells that touch are one object with one centroid.  sq_mask_split_u8 cuts a one-pixel line of background between the
 * parts of an object; the mask format does not change, so every consumer that runs after it sees separate objects.
 * Planar (N, H, W) uint8 masks with C classes, fewer than 2^31 elements; volumes are refused.  P_c, bytes >= C and "an
 * object" are those of "Mask clean-up" above: bytes >= C belong to no class, are copied through, are never written and
 * never propagate a label.  Only integer and Boolean arithmetic: the same bits on every run.
 *
 * Definition.  erosions r = 1 .. SQ_MORPH_MAX_ITER, structure = SQ_MORPH_CROSS or SQ_MORPH_SQUARE, reach T = 1 ..
 * SQ_SPLIT_MAX_REACH (the Python binding's default, None, means 2 r).  Per class c = 1 .. C-1:
 *   1. Seeds.   S_c = scipy.ndimage.binary_erosion(P_c, structure, iterations=r) with scipy's defaults (border_value 0: the
 *               seeds shrink away from the frame edge exactly as sq_mask_morph_u8's erode does).
 *   2. Labels.  The 4-connected components of S_c are numbered in the raster order of their first pixel
 *               (scipy.ndimage.label's order, the root order of sq_ccl.h).  L_0 = that number on seed pixels, 0 ("none")
 *               elsewhere.  Labels of different classes are never compared.
 *   3. Regrowth.  T synchronous steps.  For every pixel p with mask(p) = c and L_{t-1}(p) = 0:
 *               L_t(p) = the smallest non-zero L_{t-1}(q) over the 4 neighbours q inside the frame with mask(q) = c,
 *               or 0 when there is none.  Every other pixel keeps its label.  All reads of step t see step t-1 (Jacobi,
 *               never in place): which label a pixel takes depends on the step at which the labels arrive, not only on
 *               their order, so this is part of the definition.
 *   4. Cut.     out(p) = 0 iff L_T(p) > 0 and some 4-neighbour q inside the frame with mask(q) = mask(p) has
 *               0 < L_T(q) < L_T(p); otherwise out(p) = mask(p).  Anti-extensive: out is mask or 0 everywhere.
 * Consequences (tests/test_mask_split_cpu.py asserts them on the restatement, tests/mask_split_cases.py):
 *   - two surviving pixels with different non-zero labels are never 4-adjacent;
 *   - a component without a seed is unchanged, and a mask with at most one seed per component comes back unchanged;
 *   - pixels that T steps do not reach keep their class and may still bridge two parts: the price of a bounded T.
 * Deliberately not built: growth until nothing changes (it would need a device-to-host readback inside the frame stream and
 * could not be captured in a graph), and seeds from the Euclidean distance transform or its h-maxima.  Known limit: objects
 * whose eroded cores stay connected (three mutually overlapping disks) are not split.
 *
 * Kernels (sq_split.hip, one program with "Volume clean-up: splitting": a frame is a volume with D = 1).  A fixed chain of launches on `stream`, no host readback, no block waits on another, no
 * flag is polled: the call can be captured in a graph.
 *   seeds    : one sq_mask_morph_u8 erosion launch, all classes, into a 1 B / pixel plane of the workspace.
 *   labels   : sq_ccl.h's row scan / merge / compress on the seed plane; a label is the root's linear index + 1 (the batch
 *              is one index space, frames are never linked).  The first regrowth launch turns roots into labels as it reads.
 *   regrowth : a block of 256 threads owns a tile of SQ_SPLIT_TILE_ROWS x SQ_SPLIT_TILE_COLS pixels and stages the class
 *              bytes and the int32 labels of the tile and a halo of as many pixels as the launch runs steps, at most
 *              SQ_SPLIT_STEPS, in LDS; beyond the halo and the frame there is nothing (class 0, label 0).  Every thread
 *              owns 25 staged cells; per step it computes their new labels from LDS into registers -- the second copy a
 *              synchronous step needs -- and writes them after a barrier.  A step that changes nothing in the staged region
 *              ends the block's loop (so does every later one), which is also how a block with nothing to grow copies
 *              through.  The tile's labels go to the other global label plane; ceil(T / SQ_SPLIT_STEPS) launches
 *              ping-pong between the two planes, the last one runs the remainder.  The tile is exact because what is
 *              missing beyond the staged rim travels one pixel per step.  (64 + 16) x (64 + 16) cells x 5 B = 32 000 B of
 *              static LDS (32 256 allocated), 102 VGPRs, no spills: 4 blocks = 16 waves per CU (tools/resource_report.py:
 *              4 waves per SIMD).
 *   cut      : one pointwise pass, labels + mask -> out.
 *   SQ_SPLIT_LDS=0 (environment, read per call) runs the regrowth as one synchronous step per launch on the global planes:
 *   trivially the definition, the in-tree cross-check and the baseline of tools/mask_split_bench.py.  Same bits.
 *
 * workspace: sq_mask_split_workspace(N, H, W) = 9 N H W rounded up to 16 bytes (-1: N, H or W < 1, or 2^31 or more
 * elements): two int32 label planes and the seed plane; 16-B aligned, overlapping neither mask nor out.
 * sq_mask_split_u8 returns SQ_EINVAL with a message, before any launch, for null pointers, C < 2 or C > 256, a bad
 * structure, erosions outside 1 .. 16, reach outside 1 .. 64, N, H or W < 1, 2^31 or more elements, a workspace that is not
 * 16-B aligned or overlaps mask or out, and out overlapping mask.
 * ---------------------------------------------------------------------------------------- */
#define SQ_SPLIT_MAX_REACH 64
#define SQ_SPLIT_TILE_ROWS 64
#define SQ_SPLIT_TILE_COLS 64
#define SQ_SPLIT_STEPS 8
int64_t sq_mask_split_workspace(int N, int H, int W);
int sq_mask_split_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, int erosions, int structure, int reach,
                     void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Volume clean-up: 3-D morphology, cavities, faces (sequitr_amd/volumeops.py: morph3d, fill_cavities, clear_border3d,
 * VolumeCleanup; the volume jobs' `volume_postprocess` key).  The 3-D counterpart of "Mask clean-up" above for the masks
 * of UNet3D: mask and out are (N, D, H, W) uint8 class labels with C classes, fewer than 2^31 elements; in the jobs
 * D, H, W = Z, X, Y.  The N volumes are independent: nothing crosses from volume n into n + 1.
 *
 * "Mask clean-up" applies word for word, with voxels for pixels: P_c = (mask == c) for c = 1 .. C-1, byte 0 is background,
 * bytes >= C belong to no class, are copied through and are never written; every operation computes one processed plane
 * Q_c per class from the INPUT mask and merges with the extensive rule (dilate, close, fill_holes: out = mask wherever
 * mask > 0, elsewhere the smallest c whose Q_c is set, else 0) or the anti-extensive rule (erode, open, clear_border:
 * out = c where Q_c is set and mask == c, else 0; bytes >= C stay).  out must not overlap mask.  "An object" is a
 * 6-connected component of one class > 0: the labelling of sq_ccl.h with planes = D, scipy.ndimage.label's default 3-D
 * structure.  Every plane is Boolean: every result is exact and the same bits on every run.
 *
 * sq_volume_morph_u8 : op = SQ_MORPH_ERODE / DILATE / OPEN / CLOSE, structure = SQ_MORPH3D_CROSS
 *   (scipy.ndimage.generate_binary_structure(3, 1), 6 neighbours) or SQ_MORPH3D_CUBE ((3, 3), 26 neighbours), iterations
 *   r = 1 .. SQ_MORPH3D_MAX_ITER.
 *     Q_c = scipy.ndimage.binary_{erosion,dilation,opening,closing}(P_c, structure, iterations=r)
 *   with scipy's defaults (border_value = 0, origin 0): every one of the r (or r + r) elementary 3x3x3 steps sees zeros
 *   outside the volume on all six faces, so erosion eats in from the faces and closing loses voxels near them.
 *   One launch per call, no workspace.  A block of 256 threads owns a brick of SQ_MORPH3D_TILE_D x SQ_MORPH3D_TILE_H x
 *   SQ_MORPH3D_TILE_W voxels and keeps the bit plane of one class in LDS for the brick plus a halo of r (erode, dilate) or
 *   2r (open, close) planes and rows and of 32 columns (the staged row of 192 columns starts at a multiple of 4 and is three
 *   64-bit words), in two copies.  Per class c = 1 .. C-1 the block reads the bytes of that region once from global memory
 *   -- only the planes, rows and dword columns inside the halo it needs and inside the volume -- four rows per wave at a
 *   time through a 6 KiB byte buffer, and packs each 64-voxel row segment with one __ballot of (byte == c); for the default
 *   C = 2 that is one read of the region.  A class absent from the region skips its steps.  A cross step is the word's
 *   horizontal triple (shifts with carry from the neighbouring words) AND / OR'ed with the same word of the rows above and
 *   below and of the planes before and after; a cube step is the horizontal triple of all nine (plane +- 1, row +- 1) rows.
 *   Dilations are masked to the volume in all three axes.  The block's result is exact on its brick because an error at
 *   the staged region's rim travels one voxel per step and the halo is as wide as there are steps.  Each class's finished
 *   plane is merged into the brick in `out` at once: a thread reads its own voxels of the mask again (and, from the second
 *   class present on, what it wrote to `out` itself) and stores them, with 4-byte accesses where W % 4 == 0 and both
 *   pointers are 4-byte aligned, byte by byte otherwise; nothing of the brick is kept in registers across the steps
 *   (107 VGPRs, no spills).  A brick whose region holds no class at all is copied through.
 *   Why the cap: the halo is as wide as the number of steps in all three axes, so LDS grows with the cube of it.
 *   SQ_MORPH3D_MAX_ITER = 4 makes the widest halo 8 (open or close at r = 4): (8 + 16) x (32 + 16) rows x 3 words =
 *   27 KiB per copy, 60 KiB of static LDS per block with the byte buffer -- under 64 KiB, two blocks per CU.
 *   Larger radii: iterated erosions and iterated dilations of one plane compose exactly (erode 2 then erode 2 = erode 4),
 *   so for C = 2 two steps in a list equal one larger step.  For C > 2 this holds for erosions only: two extensive steps
 *   merge between them -- a voxel the first dilation gave to class 1 is no background for class 2 in the second -- so they
 *   differ from a single larger step.  Open and close do not compose this way at any C (open 2 twice = open 2).
 *
 * sq_volume_fill_holes_u8 : a cavity of class c is a 6-connected component of ~P_c with no voxel on any of the volume's six
 *   faces -- what scipy.ndimage.binary_fill_holes(P_c) fills on a 3-D array.  Q_c = P_c plus the cavities that qualify: all
 *   of them for max_voxels <= 0, otherwise those of at most max_voxels voxels, counting EVERY voxel of the component,
 *   voxels of other classes and bytes >= C included.  Extensive merge, the lowest class first.  The steps of
 *   sq_mask_fill_holes_u8 with rows = N D H in the row scan, planes = D in the merge and the face voxels -- 2 H W + 2 D W +
 *   2 D H per volume, those on edges more than once -- in place of the edge pixels.  D = 1 (or H = 1, or W = 1) puts every
 *   voxel on a face: nothing is filled, as with scipy.
 *   workspace: sq_volume_fill_holes_workspace(N, D, H, W) bytes (-1: too large), 16-B aligned: 9 B per voxel.
 *
 * sq_volume_clear_border_u8 : removes every object that has a voxel on a face; the rest is unchanged (anti-extensive merge;
 *   bytes >= C stay).  faces = SQ_FACES_ALL: all six faces.  faces = SQ_FACES_LATERAL: only the four faces h = 0, h = H-1,
 *   w = 0, w = W-1 -- a z-stack usually cuts cells at its first and last slice, and the user may want to keep them.
 *   workspace: sq_volume_clear_border_workspace(N, D, H, W) bytes (-1: too large), 16-B aligned: 8 B per voxel.
 *
 * All three return SQ_EINVAL with a message, before any launch and with out untouched, for null pointers, C < 2 or
 * C > 256, a bad op, structure or faces value, iterations outside 1 .. SQ_MORPH3D_MAX_ITER, N, D, H or W < 1, 2^31 or more
 * elements, a workspace that is not 16-B aligned, and out overlapping mask.  None reads anything back, and every call is a
 * chain of kernel launches on `stream` and nothing else (the counts and flags are cleared and the mask is copied by kernels,
 * not by memset or memcpy calls): each can be captured in a graph and replayed.  Not built: the 18-neighbour structure, anisotropic structuring elements.
 * ---------------------------------------------------------------------------------------- */
#define SQ_MORPH3D_CROSS 0
#define SQ_MORPH3D_CUBE 1
#define SQ_MORPH3D_MAX_ITER 4
#define SQ_MORPH3D_TILE_D 8
#define SQ_MORPH3D_TILE_H 32
#define SQ_MORPH3D_TILE_W 128
#define SQ_FACES_ALL 0
#define SQ_FACES_LATERAL 1
int sq_volume_morph_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int op, int structure,
                       int iterations, void *stream);
int64_t sq_volume_fill_holes_workspace(int N, int D, int H, int W);
int sq_volume_fill_holes_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int64_t max_voxels,
                            void *workspace, void *stream);
int64_t sq_volume_clear_border_workspace(int N, int D, int H, int W);
int sq_volume_clear_border_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int faces,
                              void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Volume clean-up: splitting (sequitr_amd/volumeops.py: split3d, the `split3d` step of VolumeCleanup and of the volume
 * jobs' `volume_postprocess` key).  Everything downstream of the volume mask calls a 6-connected component of one class
 * "an object", so two cells that touch are one object with one centroid, one row, one zone.  sq_volume_split_u8 cuts a
 * one-voxel sheet of background between the parts of an object; the mask format does not change.
 *
 * "Mask clean-up: splitting" applies word for word with voxels for pixels, except as follows.  mask and out are
 * (N, D, H, W) uint8 with C classes, fewer than 2^31 elements, the N volumes independent.  P_c, bytes >= C and "an object"
 * are those of "Volume clean-up": bytes >= C belong to no class, are copied through, are never written and conduct
 * nothing.  Only integer and Boolean arithmetic: the same bits on every run.
 *
 * Definition.  erosions r = 1 .. SQ_SPLIT3D_MAX_EROSIONS, structure = SQ_MORPH3D_CROSS, SQ_MORPH3D_CUBE,
 * SQ_SPLIT3D_PLANE_CROSS or SQ_SPLIT3D_PLANE_SQUARE, reach T = 1 .. SQ_SPLIT3D_MAX_REACH.  Per class c = 1 .. C-1:
 *   1. Seeds.   S_c = scipy.ndimage.binary_erosion(P_c, structure, iterations=r) with scipy's defaults (border value 0 on
 *               all six faces).  The structure is generate_binary_structure(3, 1) for cross and (3, 3) for cube; for the
 *               two plane structures it is generate_binary_structure(2, 1 | 2)[None], the planar erosion slice by slice
 *               (no face in z eats anything): what a z-stack with few, thick slices needs.
 *   2. Labels.  The 6-connected components of S_c, numbered in the raster order of their first voxel
 *               (scipy.ndimage.label's default 3-D structure, the labelling of sq_ccl.h with planes = D) -- also when the
 *               seeds came from a plane structure: seeds stacked along z are one seed.  L_0 = that number on seed voxels,
 *               0 ("none") elsewhere.  Labels of different classes are never compared.
 *   3. Regrowth.  T synchronous steps with the 6 neighbours inside the volume.  A voxel p with mask(p) = c and
 *               L_{t-1}(p) = 0 takes the smallest non-zero L_{t-1}(q) over its neighbours q with mask(q) = c, or stays 0
 *               when there is none.  Everything else keeps its label.  All reads of step t see step t-1.
 *   4. Cut.     out(p) = 0 iff L_T(p) > 0 and some 6-neighbour q inside the volume with mask(q) = mask(p) has
 *               0 < L_T(q) < L_T(p); otherwise out(p) = mask(p).
 * Consequences (tests/test_volume_split_cpu.py asserts them on the restatement, tests/volume_split_cases.py):
 *   - two surviving voxels with different non-zero labels are never 6-adjacent;
 *   - a component with at most one seed comes back unchanged;
 *   - voxels that T steps do not reach keep their class and may still bridge two parts;
 *   - row H-1 of slice z and row 0 of slice z+1 are not neighbours, nor are the last voxel of a row and the first of the
 *     next, nor volume n and volume n+1.
 * The Python default reach (None) is 3 r for cube and 2 r for the other three structures: a cube erosion removes a
 * Chebyshev ball, and the 6-neighbour growth needs up to 3 r steps to refill it (two touching balls of radius 8, centres 14
 * apart, r = 4: cube at reach 8 leaves a bridge, at reach 12 it splits; the other structures split at reach 8).
 * Not built: growth until nothing changes (it would need a readback inside the stream), EDT or h-maxima seeds,
 * spacing-aware (anisotropic) growth, the 18-neighbour structure.
 *
 * Kernels (sq_split.hip, the planar split's program with depth).  A fixed chain of launches on `stream`, no host readback, no memset or memcpy calls, no
 * block waits on another, no flag is polled: the call can be captured in a graph.
 *   seeds    : plane structures: one sq_mask_morph_u8 erosion launch on the (N D, H, W) view into the workspace's byte
 *              plane.  cross and cube: ceil(r / SQ_MORPH3D_MAX_ITER) launches of sq_volume_morph_u8 (erosions compose
 *              exactly at every C, see "Volume clean-up") that ping-pong between the workspace's byte plane and `out`,
 *              which is free until the cut; the chain is ordered so that the last launch lands in the workspace plane.
 *   labels   : sq_ccl.h's row scan (rows = N D H), merge with planes = D, compress; a label is the root's linear index + 1.
 *              The first regrowth launch turns roots into labels as it reads.
 *   regrowth : SQ_SPLIT3D_LDS=1 (environment, read per call): a block of 512 threads owns a brick of SQ_SPLIT3D_TILE_D x
 *              SQ_SPLIT3D_TILE_H x SQ_SPLIT3D_TILE_W voxels and stages the class bytes and the int32 labels of the brick
 *              and a halo of as many voxels as the launch runs steps, at most SQ_SPLIT3D_STEPS, on all three axes in LDS;
 *              beyond the halo and the volume there is nothing.  Every thread owns up to 17 staged cells and precomputes
 *              once which of them can still take a label and which of their 6 neighbours conduct (6 bits per cell); per
 *              step it computes their new labels from LDS into registers -- the second copy a synchronous step needs --
 *              and writes them after a barrier.  A step that changes nothing in the staged region ends the block's loop by
 *              a block-uniform vote.  The brick's labels go to the other global plane; ceil(T / SQ_SPLIT3D_STEPS) launches
 *              ping-pong between the two planes, the last one runs the remainder.  (8 + 4) x (16 + 4) x (32 + 4) = 8 640
 *              staged cells for 4 096 useful (47 %) x 5 B = 43 200 B of static LDS (43 456 allocated), 66 VGPRs, no
 *              spills: 3 blocks = 24 waves per CU (tools/resource_report.py: 6 waves per SIMD).  Measured against a halo
 *              of 4 (15 360 cells, 76 800 B, 2 blocks per CU): 2 steps per launch are 0.75-0.82x its time.
 *              SQ_SPLIT3D_LDS=0: one synchronous step per launch on the global planes, trivially the definition, the
 *              in-tree cross-check and the A/B baseline of tools/volume_split_bench.py.  Same bits.  With the variable
 *              unset the form is SQ_SPLIT3D_LDS_DEFAULT: the one that A/B measured faster (README.md has the figures).
 *   cut      : one pointwise pass, labels + mask -> out.
 *
 * workspace: sq_volume_split_workspace(N, D, H, W) = 9 N D H W rounded up to 16 bytes (-1: a dimension < 1, or 2^31 or
 * more elements): two int32 label planes and the seed plane; 16-B aligned, overlapping neither mask nor out.
 * sq_volume_split_u8 returns SQ_EINVAL with a message, before any launch and with out and the workspace untouched, for
 * null pointers, C < 2 or C > 256, a structure outside 0 .. 3, erosions outside 1 .. 16, reach outside 1 .. 64, a
 * dimension < 1, 2^31 or more elements, a workspace that is not 16-B aligned or overlaps mask or out, and out overlapping
 * mask.
 * ---------------------------------------------------------------------------------------- */
#define SQ_SPLIT3D_PLANE_CROSS 2
#define SQ_SPLIT3D_PLANE_SQUARE 3
#define SQ_SPLIT3D_MAX_EROSIONS 16
#define SQ_SPLIT3D_MAX_REACH 64
#define SQ_SPLIT3D_TILE_D 8
#define SQ_SPLIT3D_TILE_H 16
#define SQ_SPLIT3D_TILE_W 32
#define SQ_SPLIT3D_STEPS 2
#define SQ_SPLIT3D_LDS_DEFAULT 1
int64_t sq_volume_split_workspace(int N, int D, int H, int W);
int sq_volume_split_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int erosions, int structure,
                       int reach, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Label zones and the zone contact graph (sequitr_amd/analysis/neighbors.py: which cells are next to
 * which).  The reference counts neighbours per frame on the host with scipy's Voronoi / Delaunay of the centroids
 * (sequitr/analysis/neighbors.py); here the per-pixel part -- the zone of influence of every object -- and the per-pixel
 * part of the adjacency run on the device.  Planar (N, H, W) int32 images only, fewer than 2^31 elements.  Only integer
 * arithmetic: the same bits on every run.  Neither call reads anything back, waits on a flag or lets one block wait on
 * another: both can be captured in a graph.
 *
 * sq_label_zones_i32.  labels (N,H,W) int32: a pixel is a SEED of object L iff 1 <= L <= max_label; every other value,
 * negative and too-large ones included, is background and not an error.  max_distance R >= 0, 0 = unbounded.
 *   D(n,p)     = the minimum over the seeds q of frame n of the exact squared Euclidean distance |p - q|^2
 *   zones(n,p) = the smallest label among the seeds of frame n at squared distance D(n,p)
 *   d2(n,p)    = D(n,p)                                        (d2 may be NULL)
 *   With R > 0 a pixel with D > R*R gets zone 0; d2 still holds D.
 *   A frame without a seed gets zone 0 and d2 = 0x7fffffff everywhere (scipy's feature transform points such a frame at
 *   index (-1, 0); that artefact is not reproduced).  The search never crosses from frame n into n +- 1.
 * Consequences: a seed pixel lies in its own zone (D = 0 and it is the only seed there); without a reach the zones of a
 * frame with a seed cover it.  This is skimage.segmentation.expand_labels with the tie rule pinned.
 * The transform is separable and exact, the tie rule included:
 *   rows    : per pixel the distance g along the row to the nearest seed of that row (30000 = none) and the smaller label
 *             of the at most two seeds at that distance.  One wave per row over 64-pixel segments: the ballot of seed
 *             lanes, the nearest set bit to the left / right by clz / ffs with a carry between segments, the label
 *             fetched from that lane by a shuffle or from the carried value.  u16 + int32 = 6 B per pixel of workspace.
 *   columns : the lexicographic minimum over rows y' of (g(y',x)^2 + (y - y')^2, label(y',x)), searched outwards from y,
 *             lanes along x, while dy^2 <= the best distance so far -- <=, not <: an equidistant seed with a smaller label
 *             further out must still be seen.  Without d2 and with R > 0 the search also stops at dy > R; with d2 it runs
 *             on, because d2 = D beyond the reach too.  A per-frame flag spares a frame without a seed the search.
 * workspace: sq_label_zones_workspace(N, H, W) bytes = 16 ceil(N / 4) + 6 N H W rounded up to 16 (-1: N, H or W < 1, H or
 * W >= 30000, or 2^31 or more elements), 16-B aligned.
 * SQ_EINVAL with a message, before any launch: null labels, zones or workspace; N, H or W < 1; H or W >= 30000; 2^31 or
 * more elements; max_label outside 1 .. 2^21 - 1; max_distance outside 0 .. 46340 (R*R must fit an int32); a workspace
 * that is not 16-B aligned or overlaps labels, zones or d2; zones overlapping d2.
 *
 * sq_zone_graph.  zones (N,H,W) int32; values outside 1 .. max_label count as 0.
 *   stats (N, max_label + 1, 2) int64, [area, edge] per label: area = the number of pixels of the zone, edge = the number
 *       of those on the frame's outer border (first / last row or column; a corner counts once).  Row 0 stays 0.
 *   pairs (max_pairs, 4) int32 [frame, a, b, border], a < b, in no particular order: border = the number of pixel pairs
 *       (p, right neighbour) and (p, lower neighbour) within the frame in which one pixel has zone a and the other zone
 *       b, both > 0.  One row per distinct (frame, a, b) with border > 0.
 *   count (device int32): the number of rows written, at most max_pairs.
 *   dropped (device int32): 0 iff the rows are complete.  It counts the boundary runs that found no free slot in the
 *       table plus the distinct pairs that found no row; when it is not 0 the caller comes back with a larger max_pairs.
 * The call clears stats, count, dropped and its table itself.  One wave per image row, one lane per pixel: runs of equal
 * (a, b) along the row are found with a shuffle and a ballot, and the leader lane of each run makes one insert-and-add of
 * the run's length into an open-addressing table in the workspace (a 64-bit key of (frame, a, b) claimed with a
 * compare-and-swap, a 32-bit integer add for the count; the smallest power of two >= 2 max_pairs slots).  Areas and edges
 * get the same treatment: one 64-bit add per run of equal zone, never one per pixel.  A second kernel writes the rows.
 * Sums of integers: the set of rows and every count are independent of the order in which the atomics arrive.
 * workspace: sq_zone_graph_workspace(max_pairs) bytes = 12 per slot rounded up to 16 (-1: max_pairs outside 1 .. 2^28).
 * SQ_EINVAL with a message, before any launch: a null pointer; N, H or W < 1; N >= 2^21; 2^31 or more elements; max_label
 * outside 1 .. 2^21 - 1; max_pairs outside 1 .. 2^28; a workspace that is not 16-B aligned or overlaps zones or an output;
 * stats not 8-B aligned.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_label_zones_workspace(int N, int H, int W);
int sq_label_zones_i32(const int32_t *labels, int32_t *zones, int32_t *d2, int N, int H, int W, int max_label,
                       int max_distance, void *workspace, void *stream);
int64_t sq_zone_graph_workspace(int max_pairs);
int sq_zone_graph(const int32_t *zones, int N, int H, int W, int max_label, int64_t *stats, int32_t *pairs, int max_pairs,
                  int32_t *count, int32_t *dropped, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Label zones and the contact graph in volumes (sequitr_amd/analysis/neighbors.py: which cells of a z-stack are next
 * to which -- cells stacked along z are neighbours, and no slice-by-slice run shows it).  The volumetric counterpart of
 * the section above: (N, D, H, W) int32 arrays, fewer than 2^31 voxels, `dz` the depth spacing in in-plane pixels
 * (scipy's sampling = (dz, 1, 1)).  The zones are a minimum of fixed floating-point expressions, the graph is integer
 * work: the same bits on every run.  Neither call reads anything back, waits on a flag or lets one block wait on
 * another: each is a linear chain of kernels that can be captured in a graph, and whatever is cleared is cleared by a
 * kernel of the chain.
 *
 * sq_label_zones3d_i32.  labels (N,D,H,W) int32: a voxel is a SEED of object L iff 1 <= L <= max_label; every other value
 * is background and not an error.  max_distance R >= 0, 0 = unbounded.
 *   For every slice (n, z') let (P, L)(n, z', h, w) be what sq_label_zones_i32 defines for that slice alone: P the exact
 *   integer squared distance to the slice's nearest seed, L the smallest label among the slice's seeds at that distance.
 *   A slice without a seed contributes nothing.
 *   A(k) = fl(fl(k dz) fl(k dz)) in double: exactly sq_edt3d_sq_f64's A.
 *   (D3, zone)(n, z, h, w) = the lexicographic minimum over z' of (fl(A(z - z') + P(n, z', h, w)), L(n, z', h, w)),
 *   the sum being one double add.  The search never crosses from volume n into n +- 1.
 *   zones(n,p) = zone, or 0 where R > 0 and D3 > (double)R * R;   d2(n,p) = D3 everywhere (float64; d2 may be NULL).
 *   A volume without a seed gets zone 0 and d2 = +inf everywhere (scipy's feature transform points such a volume at index
 *   (-1, 0, 0), and sq_edt3d_sq_f64 reproduces that; this call does not -- the same decision as in the planar call).
 * Consequences: a seed voxel lies in its own zone; without a reach the zones of a volume with a seed cover it; for a
 * volume with a seed d2 equals sq_edt3d_sq_f64 of the seed indicator bit for bit, for every dz (the minimum of the first
 * components is the same minimum); at dz = 1, and at every dz at which each A + P is exact, the result is the all-pairs
 * definition -- the nearest seed in 3-D, the smallest label at a tie.  Where A + P rounds, ties are ties of the ROUNDED
 * sums, as written above.
 * The kernels:
 *   planar half : the row and column passes of sq_label_zones_i32 over the N*D slices, always unbounded and with d2, so
 *                 that they deliver P (0x7fffffff in a slice without a seed) and L for every voxel.  No reach bounds them.
 *   depth pass  : a block owns a strip of 32 columns of one (n, h) row with P and L of all D slices in LDS, as two arrays
 *                 of [D][32] int32 (8 B x D x 32: a 32-lane LDS group reads 32 consecutive dwords of one slice, which is
 *                 free of bank conflicts); lanes run along w and the search outwards in k runs on LDS.  A side is finished
 *                 when A(k) > best -- not sq_edt3d_sq_f64's >=: an equidistant seed with a smaller label further out must
 *                 still be seen -- and, without d2 and with R > 0, also when A(k) > R*R.  L is read only where the
 *                 candidate's distance is <= best.  Depths whose strip exceeds the device's LDS per block
 *                 (hipDeviceAttributeMaxSharedMemoryPerBlock: D > 640 at 160 KiB) take the same search on global memory;
 *                 the environment variable SQ_ZONES3D_LDS=0, read per launch, selects that form for every depth.  Both
 *                 give the same bits.
 * workspace: sq_label_zones3d_workspace(N, D, H, W) bytes = 16 ceil(N D / 4) [per-slice flags] + 3 x 16 ceil(V / 4) [P, L and
 * the row pass's labels, int32 each] + 2 V [the row pass's distances, u16] rounded up to 16, V = N D H W; -1 under
 * sq_weightmap3d_workspace's conditions (a dimension < 1, D, H or W >= 30000, or 2^31 or more voxels).  16-B aligned.
 * SQ_EINVAL with a message, before any launch: null labels, zones or workspace; a dimension < 1; D, H or W >= 30000; 2^31
 * or more voxels; max_label outside 1 .. 2^21 - 1; max_distance outside 0 .. 46340; dz not finite or <= 0; a workspace that
 * is not 16-B aligned or overlaps labels, zones or d2; zones overlapping d2; d2 not 8-B aligned.
 *
 * sq_zone_graph3d.  zones (N,D,H,W) int32; values outside 1 .. max_label count as 0.
 *   stats (N, max_label + 1, 2) int64, [voxels, face] per label: voxels = the number of voxels of the zone, face = the
 *       number of those on any of the volume's six faces (a voxel on an edge or a corner counts once).  Row 0 stays 0.
 *   pairs (max_pairs, 5) int32 [volume, a, b, lateral, axial], a < b, in no particular order: lateral = the number of voxel
 *       pairs (p, p + 1 along w) and (p, p + 1 along h) inside the volume in which one voxel has zone a and the other zone
 *       b, both > 0; axial = the same for (p, p + 1 along d).  One row per distinct (volume, a, b) with lateral + axial > 0.
 *       The two are kept apart because in an anisotropic stack a lateral face has area dz and an axial face area 1.
 *   count, dropped (device int32): as in sq_zone_graph.
 * The call clears stats, count, dropped and its table itself.  One wave per (n, d, h) row, one lane per voxel: the right
 * neighbour comes by a shuffle, the lower and the deeper one by one coalesced load each; runs of equal (a, b) per direction
 * are found with a ballot and their leader lane makes one insert-and-add into an open-addressing table in the workspace (a
 * 64-bit key of (volume, a, b) claimed with a compare-and-swap, two 32-bit integer adds per slot -- 16 B -- the smallest
 * power of two >= 2 max_pairs slots); voxels and face get one 64-bit add per run of equal zone.  A second kernel writes
 * the rows.  Plain atomics on vector memory; sums of integers: the set of rows and every count are independent of the
 * order in which the atomics arrive.
 * workspace: sq_zone_graph3d_workspace(max_pairs) bytes = 16 per slot (-1: max_pairs outside 1 .. 2^28), 16-B aligned.
 * SQ_EINVAL with a message, before any launch: a null pointer; N, D, H or W < 1; N >= 2^21; 2^31 or more voxels; max_label
 * outside 1 .. 2^21 - 1; max_pairs outside 1 .. 2^28; a workspace that is not 16-B aligned or overlaps zones or an output;
 * stats not 8-B aligned.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_label_zones3d_workspace(int N, int D, int H, int W);
int sq_label_zones3d_i32(const int32_t *labels, int32_t *zones, double *d2, int N, int D, int H, int W, int max_label,
                         int max_distance, double dz, void *workspace, void *stream);
int64_t sq_zone_graph3d_workspace(int max_pairs);
int sq_zone_graph3d(const int32_t *zones, int N, int D, int H, int W, int max_label, int64_t *stats, int32_t *pairs,
                    int max_pairs, int32_t *count, int32_t *dropped, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Label overlap and relabelling (sequitr_amd/analysis/linking.py: which object of frame t + 1 is the same cell as which
 * object of frame t).  The reference hands tracking to an external program; here the per-position part of linking by
 * overlap -- the contingency table of two label stacks -- and the rewriting of per-frame ranks into track IDs run on the
 * device.  A frame is P positions: H W pixels or D H W voxels alike.  Only integer arithmetic: the same bits on every
 * run.  Neither call reads anything back, waits on a flag or lets one block wait on another: both can be captured in a
 * graph, and whatever is cleared is cleared by a kernel of the call's own chain.
 *
 * sq_label_overlap.  a, b (N, P) int32; values outside 1 .. max_label count as 0.
 *   pairs (max_pairs, 4) int32 [n, la, lb, overlap], in no particular order: one row per distinct (n, la, lb) with la > 0
 *       and lb > 0 that occurs, overlap = the number of positions p with a[n,p] == la && b[n,p] == lb.
 *   area_a, area_b (N, max_label + 1) int64, each may be NULL: the number of positions per label in a / in b.  Row 0
 *       stays 0.
 *   count (device int32): the number of rows written, at most max_pairs.
 *   dropped (device int32): 0 iff the rows are complete, as in sq_zone_graph: it counts the runs that found no free slot
 *       in the table plus the distinct triples that found no row; when it is not 0 the caller comes back with a larger
 *       max_pairs.  The areas are complete either way.
 * labels[:-1] and labels[1:] of one contiguous (F, ...) stack are valid a and b: nothing is assumed about the alignment
 * of b beyond 4 bytes, nor about P.
 * Two forms, which give the same table:
 *   one-lane  : a wave takes 4 groups of 64 consecutive positions of a frame at a time, one lane per position, all 8 loads
 *               issued before the first is used; a group without a label in either stack (most of a frame is background)
 *               is left after one ballot.  Runs of equal (la, lb) along memory are found with a shuffle and a ballot; the
 *               run's leader lane makes one insert-and-add of the run's
 *               length into an open-addressing table in the workspace (a 64-bit key n << 42 | la << 21 | lb claimed with a
 *               compare-and-swap, a 32-bit integer add for the count; the smallest power of two >= 2 max_pairs slots).  The
 *               areas likewise: one 64-bit add per run of equal label, never one per position.
 *   four-lane : 16-byte loads, four positions per lane, 2 groups of 256 positions at a time; taken only when a and b are
 *               16-byte aligned and P % 4 == 0 (every frame then starts on 16 bytes and no quad straddles two frames).  Runs are
 *               merged inside the lane first: a lane whose four keys are equal enters the wave's run search with a weight
 *               of 4, a lane that sees a change adds its at most four runs itself.
 *   The environment variable SQ_LINK_VEC=0|1, read per call, selects the one-lane / four-lane form; without it
 *   SQ_LINK_VEC_DEFAULT holds: the one-lane form, which is the faster one with the areas, as the linker calls it (DESIGN.md
 *   has the figures; without the areas the four-lane form is).  A second kernel writes the rows.
 * Sums of integers: the set of rows and every count are independent of the order in which the atomics arrive.
 * workspace: sq_label_overlap_workspace(max_pairs) bytes = 12 per slot rounded up to 16 (-1: max_pairs outside 1 .. 2^28).
 * SQ_EINVAL with a message, before any launch: null a, b, pairs, count, dropped or workspace; N < 1, N >= 2^21, P < 1,
 * P >= 2^31 (N P >= 2^63 cannot then occur); max_label outside 1 .. 2^21 - 1; max_pairs outside 1 .. 2^28; a workspace
 * that is not 16-B aligned or overlaps an input or an output; area arrays that are not 8-B aligned.
 *
 * sq_relabel_lut_i32.  labels, out (N, P) int32; offsets (N + 1) device int64, non-decreasing within 0 .. lut_len; lut
 * (lut_len) device int32.  With L = labels[n,p]:
 *   out[n,p] = lut[offsets[n] + L - 1]   if 1 <= L <= offsets[n+1] - offsets[n],   0 otherwise.
 * The call cannot validate device data: an entry that would be read outside 0 .. lut_len - 1 reads as 0.
 * out == labels (in place) is allowed; any other overlap of out with labels, offsets or lut is refused.  A streaming
 * kernel: 16-byte loads and stores when labels and out are 16-byte aligned and P % 4 == 0, a scalar path otherwise.
 * It turns each object's per-frame rank into its track ID, so that a cell keeps one value through the movie.
 * SQ_EINVAL with a message, before any launch: null labels, out or offsets; null lut with lut_len > 0; lut_len < 0;
 * N < 1, N >= 2^21, P < 1, P >= 2^31; offsets not 8-B aligned; a refused overlap.
 * ---------------------------------------------------------------------------------------- */
#define SQ_LINK_VEC_DEFAULT 0
int64_t sq_label_overlap_workspace(int max_pairs);
int sq_label_overlap(const int32_t *a, const int32_t *b, int N, int64_t P, int max_label, int64_t *area_a, int64_t *area_b,
                     int32_t *pairs, int max_pairs, int32_t *count, int32_t *dropped, void *workspace, void *stream);
int sq_relabel_lut_i32(const int32_t *labels, int32_t *out, int N, int64_t P, const int64_t *offsets, const int32_t *lut,
                       int64_t lut_len, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SEQUITR_HIP_H */
