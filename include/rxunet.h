/* rxunet.h -- C ABI of librxunet.so: hand-written CDNA4 (gfx950) kernels for the hot path of the
 * multi-task 3-D residual-encoder U-Net (reference: /root/reference/builders/, path
 * NetworkFromConfig.forward + autograd backward).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator);
 *    nothing here allocates, frees, synchronises or retains pointers after return;
 *  - every entry point enqueues on `stream` (a hipStream_t passed as void*) and returns
 *    RX_OK (0) or a negative status; rx_last_error() gives a human-readable reason;
 *  - activations inside the engine are CHANNELS-LAST (n, z, y, x, c) in the compute dtype
 *    (RX_F32 parity mode, RX_BF16 / RX_F16 throughput modes); the boundary tensors (input
 *    image, logits) are NCDHW fp32 exactly as the reference's callers see them
 *    (train.py:195-204, dataset.py:211-220);
 *  - parameters and parameter gradients cross the boundary in PyTorch's own layouts
 *    (Conv3d (Co,Ci,kz,ky,kx), ConvTranspose3d (Ci,Co,kz,ky,kx)), fp32.
 *
 * Environment knobs (RX_*, listed in README.md) are measurement switches: the library reads each ONCE per thread, at the first
 * call that consults it, and keeps the answer -- changing one inside a running process has no effect.
 *
 * Each entry point names the torch primitive of the reference it replaces (file:line relative to
 * /root/reference).  The Python binding a maintainer would add is in INTEGRATION.md.
 */
#ifndef RXUNET_H
#define RXUNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RX_OK 0
#define RX_EINVAL (-1)      /* bad argument (null pointer, non-positive size, misaligned) */
#define RX_EUNSUPPORTED (-2) /* shape outside what the kernels cover (e.g. channels % 32 != 0) */
#define RX_ELAUNCH (-3)     /* HIP reported a launch error */
#define RX_EWORKSPACE (-4)  /* workspace too small */

typedef enum { RX_F32 = 0, RX_BF16 = 1, RX_F16 = 2 } rx_dtype;
typedef enum { RX_ACT_NONE = 0, RX_ACT_SIGMOID = 1, RX_ACT_SOFTMAX = 2 } rx_head_act;

/* channels-last activation view: element (n,z,y,x,c) lives at
 * ptr[((n*z_*y_ + ...)*x_ + x)*ld + c]; `ld` >= c lets a view address a channel slice of a wider
 * buffer (how torch.cat of decoder.py:147 is eliminated). */
typedef struct {
  void* ptr;
  int32_t n, z, y, x, c, ld;
  /* cs == 0: the c channels of a voxel are contiguous (stride ld between voxels).
   * cs != 0 ("planar concat", only the 3x3x3 stride-1 conv entry points take it, 16-bit types, ld == 32): the channels come
   * in groups of ld, group j of element (n,z,y,x) lives at ptr[j*cs + (((n*z_+z)*y_+y)*x_+x)*ld + c%ld] -- how the two
   * 32-channel halves of the full-resolution decoder.py:147 concat stay DENSE tensors (a 64-byte channel slice of a 128-byte
   * voxel costs every kernel that streams it 1.5-2x: measured 154 -> 250 us for the stride-2 conv reading it). */
  int64_t cs;
} rx_act;

int rx_abi_version(void);
const char* rx_last_error(void);
int rx_device_arch_ok(void); /* 1 iff the current device is gfx950 */
/* name of the kernel instantiation the last conv / convT entry point of this thread launched (bench attribution), or of
 * the gate kernel the last rx_se_gate_fwd / rx_se_gate_bwd chose (se_gate_fwd_kernel, se_fill_mult_kernel,
 * se_gate_bwd_small_kernel, se_gate_bwd_kernel) */
const char* rx_last_conv_kernel(void);

/* ---- parameter packing ------------------------------------------------------------------ */
/* Conv3d weight (Co,Ci,T) fp32 -> w_fwd [T][Co][Ci] and w_bwd [T][Ci][Co] (same tap order; the
 * bwd-data tap table mirrors the offsets instead), both in `dt`.  Either output
 * may be NULL.  T = kz*ky*kx. */
int rx_pack_conv_weight(rx_dtype dt, const float* w, int co, int ci, int taps, void* w_fwd, void* w_bwd,
                        void* stream);
/* ConvTranspose3d weight (Ci,Co,T) fp32 -> w_fwd [T][Co][Ci], w_bwd [T][Ci][Co] (tap order kept). */
int rx_pack_convT_weight(rx_dtype dt, const float* w, int ci, int co, int taps, void* w_fwd, void* w_bwd,
                         void* stream);
/* the same for `count` weights in ONE launch per 40 tensors (a train step re-packs every conv weight: 66 tensors at cfg2).
 * kind[i] 0: Conv3d weight (A = Co, B = Ci), 1: ConvTranspose3d weight (A = Ci, B = Co); HOST arrays of device pointers. */
int rx_pack_multi(rx_dtype dt, int count, const float* const* w, const int* kind, const int* A, const int* B,
                  const int* taps, void* const* w_fwd, void* const* w_bwd, void* stream);

/* ---- nn.Conv3d (simple_conv_blocks.py:43-51; kernel per axis in {1,3}, stride per axis in {1,2},
 *      padding (k-1)/2, dilation 1) ------------------------------------------------------- */
/* `ws`/`ws_bytes`: optional scratch for split-K (used only for the deep 4^3/8^3 layers whose natural
 * grid cannot fill 256 CUs); NULL disables split-K.  rx_conv_workspace_hint() is always enough. */
size_t rx_conv_workspace_hint(void);
int rx_conv3d_fwd(rx_dtype dt, const rx_act* x, const void* w_fwd, const float* bias, const rx_act* y,
                  const int32_t kernel[3], const int32_t stride[3], void* ws, size_t ws_bytes, void* stream);
/* the same plus the InstanceNorm statistics of y (stats[n][c] = (mean, rstd), as rx_instnorm_stats): on the persistent
 * halo kernels the sums come out of the conv epilogue (per-lane running sums, one wavefront reduction per workgroup) and y
 * is not read again; otherwise conv followed by rx_instnorm_stats.  ws >= max(rx_conv_workspace_hint(),
 * rx_instnorm_stats_workspace(y)). */
int rx_conv3d_fwd_stats(rx_dtype dt, const rx_act* x, const void* w_fwd, const float* bias, const rx_act* y,
                        const int32_t kernel[3], const int32_t stride[3], float eps, float* stats, void* ws,
                        size_t ws_bytes, void* stream);
/* dx (+)= conv_transpose(dy, w): autograd of the above w.r.t. its input */
int rx_conv3d_bwd_data(rx_dtype dt, const rx_act* dy, const void* w_bwd, const rx_act* dx,
                       const int32_t kernel[3], const int32_t stride[3], int accumulate, void* ws,
                       size_t ws_bytes, void* stream);
/* backward-data that also delivers the two means of the InstanceNorm backward of the layer whose OUTPUT gradient it completes
 * (dx = dL/d(out of that layer); in_y / in_stats / slope describe it; the layer has no residual: its LeakyReLU mask is the
 * sign of the normalised value; the caller guarantees nothing adds to dx afterwards).  On the persistent 32-channel halo
 * kernel  sum g'  and  sum g'*(y - mean)  are per-lane running sums of the epilogue (y prefetched under the MFMA loop):
 * *fused = 1, m12[n][c] = (mean g', mean g'*xhat), continue with rx_instnorm_act_bwd_apply.  Otherwise *fused = 0 and m12 is
 * untouched: continue with rx_instnorm_act_bwd. */
int rx_conv3d_bwd_data_instats(rx_dtype dt, const rx_act* dy, const void* w_bwd, const rx_act* dx,
                               const int32_t kernel[3], const int32_t stride[3], int accumulate, const rx_act* in_y,
                               const float* in_stats, float slope, float* m12, int* fused, void* ws, size_t ws_bytes,
                               void* stream);
/* dw (Co,Ci,T) fp32 = sum over voxels; workspace from rx_conv3d_bwd_weight_workspace() */
size_t rx_conv3d_bwd_weight_workspace(const rx_act* x, const rx_act* dy, const int32_t kernel[3]);
int rx_conv3d_bwd_weight(rx_dtype dt, const rx_act* x, const rx_act* dy, float* dw, const int32_t kernel[3],
                         const int32_t stride[3], void* ws, size_t ws_bytes, void* stream);

/* ---- nn.ConvTranspose3d with kernel == stride, per axis in {1,2} (decoder.py:110-113,146) -- */
int rx_convT3d_fwd(rx_dtype dt, const rx_act* x, const void* w_fwd, const float* bias, const rx_act* y,
                   const int32_t stride[3], void* ws, size_t ws_bytes, void* stream);
int rx_convT3d_bwd_data(rx_dtype dt, const rx_act* dy, const void* w_bwd, const rx_act* dx,
                        const int32_t stride[3], int accumulate, void* ws, size_t ws_bytes, void* stream);
size_t rx_convT3d_bwd_weight_workspace(const rx_act* x, const rx_act* dy, const int32_t stride[3]);
int rx_convT3d_bwd_weight(rx_dtype dt, const rx_act* x, const rx_act* dy, float* dw, const int32_t stride[3],
                          void* ws, size_t ws_bytes, void* stream);

/* ---- nn.InstanceNorm3d(affine=False, eps) + LeakyReLU(slope) + residual add
 *      (build_network_from_config.py:172,208-210; resblocks.py:106-114) ------------------- */
/* stats[n][c] = (mean, rstd) with biased variance; ws: rx_instnorm_stats_workspace() bytes */
size_t rx_instnorm_stats_workspace(const rx_act* y);
int rx_instnorm_stats(rx_dtype dt, const rx_act* y, float eps, float* stats, void* ws, size_t ws_bytes,
                      void* stream);
/* nn.Dropout3d / nn.Dropout2d (channel dropout, training mode) between a conv and its InstanceNorm
 * (simple_conv_blocks.py:57-66; build_network_from_config.py:169-170 `dropout_op_kwargs`): IN(s*y) with s = 1/(1-p) equals
 * (y - mean)/sqrt(var + eps*(1-p)^2) for a kept (n, c) plane and 0 for a dropped one -- so the caller computes the statistics
 * with eps*(1-p)^2 and this call sets rstd = 0 for the dropped planes (stats[i].rstd *= keep[i], keep[n*C+c] in {0,1}); every
 * forward and backward InstanceNorm entry point then does the right thing from `stats` alone, no pass over y. */
int rx_instnorm_stats_mask(float* stats, const float* keep, int count, void* stream);
/* out = lrelu_slope( (y-mean)*rstd + residual ); residual may be NULL; slope = 1 -> no activation */
int rx_instnorm_act_fwd(rx_dtype dt, const rx_act* y, const float* stats, const rx_act* residual,
                        const rx_act* out, float slope, void* stream);
/* stats + apply in one call: one launch when the tensor is small (<= 8^3 voxels per sample, C % 32 == 0), otherwise the two
 * calls above.  Writes stats (kept for the backward). */
int rx_instnorm_fwd(rx_dtype dt, const rx_act* y, float eps, float* stats, const rx_act* residual,
                    const rx_act* out, float slope, void* ws, size_t ws_bytes, void* stream);
/* g = dL/dout; `out` supplies the sign for the LeakyReLU mask.  out == NULL with slope != 1 means "no residual was
 * added": the mask is then the sign of the normalised value and the output tensor is not read.
 * dy = dL/dy; d_residual (optional) receives (or accumulates) g*mask.  ws as for stats. */
int rx_instnorm_act_bwd(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out,
                        float slope, const rx_act* dy, const rx_act* d_residual, int accumulate_residual,
                        void* ws, size_t ws_bytes, void* stream);

/* rx_instnorm_act_bwd for a residual-block epilogue out = lrelu(IN(y) + res) (resblocks.py:113-114) with the masked gradient
 * g' = g * lrelu'(out) written ONCE: the reduce pass stores g' into d_residual (it IS the residual's gradient; the buffer must
 * not hold earlier contributions -- d_residual == g is allowed) while it sums, the apply pass reads (g', y) only: 7 tensor
 * passes instead of 8.  pool_dy / pool_stride (optional): gradient of the AvgPool that opens the next stage's skip path
 * (resblocks.py:95), added on the fly, g <- g + pool_dy[v / stride] / prod(stride) -- replaces a preceding
 * rx_avgpool_bwd(pool_dy, g, stride, accumulate = 1).  ws as for rx_instnorm_act_bwd. */
int rx_instnorm_act_bwd_res(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out,
                            float slope, const rx_act* pool_dy, const int32_t pool_stride[3], const rx_act* d_residual,
                            const rx_act* dy, void* ws, size_t ws_bytes, void* stream);

/* second pass of rx_instnorm_act_bwd alone, with the two means m12[n][c] supplied by the caller */
int rx_instnorm_act_bwd_apply(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out,
                              float slope, const float* m12, const rx_act* dy, const rx_act* d_residual,
                              int accumulate_residual, void* stream);

/* ---- SqueezeExcite + DropPath of the residual blocks (resblocks.py:79-87,109-112 BasicBlockD; :203-212,234-240
 *      BottleneckD).  Both classes come from the un-vendored dynamic_network_architectures package: PARITY UNPINNED
 *      (restated in oracle/resenc_oracle.py).  The block output is
 *          a = lrelu( mult[n][line][c] * xhat + residual ),   mult = path_scale[n] * gate,
 *      gate = sigmoid(fc2(relu(fc1(p)))), p = (path_scale[n] * xhat).mean((2, 3)): a 5-D tensor is pooled over (z, y) and
 *      keeps x (keep_x = 1: line = x), a 4-D tensor (2-D nets, unit z axis here) over (y, x) (keep_x = 0: one line).
 *      path_scale[n] = bernoulli(keep_prob)/keep_prob of DropPath in training, NULL otherwise. -------------------- */
typedef struct {
  const float* w1; /* fc1.weight (rd, C) */
  const float* b1; /* fc1.bias (rd) */
  const float* w2; /* fc2.weight (C, rd) */
  const float* b2; /* fc2.bias (C) */
  int32_t rd;      /* reduction channels, <= 64 */
  int32_t keep_x;
} rx_se_params;
size_t rx_se_workspace(const rx_act* y);
/* line sums of y -> pooled [n][L][c] (raw line mean of xhat), hidden [n][L][rd], gate, mult [n][L][c] (all fp32, kept for
 * the backward).  se == NULL: DropPath only, mult[n][x][c] = path_scale[n] (keep_x = 1 layout), nothing else is written. */
int rx_se_gate_fwd(rx_dtype dt, const rx_act* y, const float* stats, const float* path_scale, const rx_se_params* se,
                   float* pooled, float* hidden, float* gate, float* mult, void* ws, size_t ws_bytes, void* stream);
/* out = lrelu_slope( mult * (y-mean)*rstd + residual ) */
int rx_instnorm_gate_act_fwd(rx_dtype dt, const rx_act* y, const float* stats, const float* mult, int keep_x,
                             const rx_act* residual, const rx_act* out, float slope, void* stream);
/* first backward pass: line sums of g' = g*lrelu'(out) and g'*xhat, gate backward.  Writes dadd [n][L][c] (the pooled
 * path's contribution to dL/dxhat), m12 [n][c] (the two InstanceNorm backward means) and the fc gradients
 * (dw1 (rd,C), db1 (rd), dw2 (C,rd), db2 (C); untouched when se == NULL). */
int rx_se_gate_bwd(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out, float slope,
                   const float* path_scale, const rx_se_params* se, const float* pooled, const float* hidden,
                   const float* gate, const float* mult, float* dadd, float* m12, float* dw1, float* db1, float* dw2,
                   float* db2, void* ws, size_t ws_bytes, void* stream);
/* second pass: dy = rstd*(g'*mult + dadd - m1 - xhat*m2); d_residual (+)= g' */
int rx_instnorm_gate_act_bwd(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out,
                             float slope, const float* mult, const float* dadd, const float* m12, int keep_x,
                             const rx_act* dy, const rx_act* d_residual, int accumulate_residual, void* stream);

/* ---- nn.AvgPool3d(kernel=stride, per axis in {1,2}) (resblocks.py:95) -------------------- */
int rx_avgpool_fwd(rx_dtype dt, const rx_act* x, const rx_act* y, const int32_t stride[3], void* stream);
/* rx_instnorm_act_fwd and rx_avgpool_fwd of its output in one pass (the last block of an encoder stage feeds the AvgPool of
 * the next stage's skip path, resblocks.py:95): out as above, pooled = avgpool(out), bit-identical to the two calls */
int rx_instnorm_act_pool_fwd(rx_dtype dt, const rx_act* y, const float* stats, const rx_act* residual,
                             const rx_act* out, const rx_act* pooled, const int32_t stride[3], float slope,
                             void* stream);
int rx_avgpool_bwd(rx_dtype dt, const rx_act* dy, const rx_act* dx, const int32_t stride[3], int accumulate,
                   void* stream);

/* ---- stem: first Conv3d on the NCDHW fp32 image, Cin <= 16 with Cout * Cin * taps * 4 <= 160 KB (encoder.py:84; MFMA kernels
 *      for Cin <= 4, VALU kernels with all weights in LDS above) ---- */
int rx_stem_conv_fwd(rx_dtype dt, const float* x_ncdhw, int n, int cin, int z, int y, int x, const float* w,
                     const float* bias, const rx_act* out, const int32_t kernel[3], void* stream);
/* rx_stem_conv_fwd followed by rx_instnorm_stats of its output (workspace: rx_instnorm_stats_workspace(out)); on the MFMA
 * kernel the statistics come out of the same pass.  Same (mean, rstd) either way. */
int rx_stem_conv_fwd_stats(rx_dtype dt, const float* x_ncdhw, int n, int cin, int z, int y, int x, const float* w,
                           const float* bias, const rx_act* out, const int32_t kernel[3], float eps, float* stats,
                           void* ws, size_t ws_bytes, void* stream);
size_t rx_stem_conv_bwd_weight_workspace(int cin, int cout, int taps);
int rx_stem_conv_bwd_weight(rx_dtype dt, const float* x_ncdhw, int n, int cin, int z, int y, int x,
                            const rx_act* dy, float* dw, const int32_t kernel[3], void* ws, size_t ws_bytes,
                            void* stream);

/* ---- task head: Conv3d 1x1x1 with bias to K <= 64 channels, NCDHW fp32 logits, optional
 *      eval-mode activation (decoder.py:131,151-152; build_network_from_config.py:320-323) ---- */
int rx_head_fwd(rx_dtype dt, const rx_act* x, const float* w, const float* b, int k, float* out_ncdhw,
                int act, void* stream);
size_t rx_head_bwd_workspace(const rx_act* x, int k);
int rx_head_bwd(rx_dtype dt, const float* dout_ncdhw, const rx_act* x, const float* w, int k, const rx_act* dx,
                float* dw, float* db, void* ws, size_t ws_bytes, void* stream);

/* InstanceNorm apply + LeakyReLU of the layer under a task head AND the head's 1x1x1 conv (+ eval-mode activation) in one pass:
 * the activated output is written and not re-read -- or, with out = NULL, not written at all (nobody but the head reads that
 * layer's output, and rx_instnorm_act_bwd_head rebuilds what the backward needs from y).  Same `out` bit for bit and the same
 * logits to fp32 round-off as rx_instnorm_act_fwd followed by rx_head_fwd (decoder.py:115-131,151-152).  16-bit types, k <= 4. */
int rx_instnorm_act_head_fwd(rx_dtype dt, const rx_act* y, const float* stats, const rx_act* out, float slope,
                             const float* head_w, const float* head_b, int k, float* out_ncdhw, int act, void* stream);

/* InstanceNorm + LeakyReLU backward of the layer that feeds a task head (the conv block of the last decoder stage,
 * decoder.py:115-131: no residual), with the head's data gradient formed on the fly: g[v][c] = sum_k dout[k][v] * w[k][c] is
 * never written (call rx_head_bwd with dx = NULL for dw / db).  Same dy, bit for bit, as rx_head_bwd(dx = g) followed by
 * rx_instnorm_act_bwd(g, y, stats, out = NULL, ...).  k <= 4; ws as for rx_instnorm_act_bwd.
 * head_dw (k, C) / head_db (k), optional and together (round 3): the head's OWN parameter gradients out of the same reduce pass,
 * dw[k][c] = sum dout[k][v] * lrelu(xhat)[v][c] with the activation recomputed from y and rounded as the forward stored it --
 * rx_head_bwd is then not called and rx_instnorm_act_head_fwd may be given out = NULL (the activated output of that layer, 268 MB
 * at cfg2, is neither written nor read). */
int rx_instnorm_act_bwd_head(rx_dtype dt, const float* dout_ncdhw, int k, const float* head_w, const rx_act* y,
                             const float* stats, float slope, const rx_act* dy, float* head_dw, float* head_db, void* ws,
                             size_t ws_bytes, void* stream);

/* ---- per-channel sum over (n, voxels): bias gradients ----------------------------------- */
size_t rx_channel_sum_workspace(const rx_act* x);
int rx_channel_sum(rx_dtype dt, const rx_act* x, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- task losses of the train step, single pass (reference training/losses/losses.py) ---------
 * logits / target / pred: (N, C, V) fp32, NCDHW-contiguous (V = Z*Y*X).  `loss` and `grad_loss` are DEVICE scalars
 * (no host synchronisation); `coef` carries the per-channel backward coefficients from fwd to bwd
 * (2*C floats for BCE-Dice, 1 float for masked cosine).  ws: rx_loss_workspace() bytes. */
size_t rx_loss_workspace(int n, int c, long v);
/* BCEDiceLoss(alpha, beta): alpha * BCE-with-logits on targets t*(1-2s)+s (losses.py:217-238,307-318)
 * + beta * (1 - mean_c 2 sum(p t) / max(sum(p^2)+sum(t^2), eps)), p = sigmoid(logits) (losses.py:17-43,128-138) */
int rx_bce_dice_loss_fwd(const float* logits, const float* target, int n, int c, long v, float alpha, float beta,
                         float smoothing, float eps, float* loss, float* coef, void* ws, size_t ws_bytes,
                         void* stream);
int rx_bce_dice_loss_bwd(const float* logits, const float* target, int n, int c, long v, float alpha, float beta,
                         float smoothing, const float* coef, const float* grad_loss, float* dlogits, void* stream);
/* MaskedCosineLoss (losses.py:187-215): 1 - sum(cos(pred/|pred|, t) m) / (sum(m) + 1e-8), m = |t| > 1e-6; C <= 8 */
int rx_masked_cosine_loss_fwd(const float* pred, const float* target, int n, int c, long v, float* loss, float* coef,
                              void* ws, size_t ws_bytes, void* stream);
int rx_masked_cosine_loss_bwd(const float* pred, const float* target, int n, int c, long v, const float* coef,
                              const float* grad_loss, float* dpred, void* stream);

/* ---- the other task losses of the reference's map (train.py:43-66), same pattern: single pass, device-scalar loss --------
 * Element-wise family: loss = mean or sum over all N*C*V elements of l(x, t).
 *   RX_LOSS_BCE_LOGITS  l = max(x,0) - x*ts + log1p(exp(-|x|)), ts = t*(1-2a) + a   (nn.BCEWithLogitsLoss: a = 0;
 *                       BCEWithLogitsLossLabelSmoothing, losses.py:217-238: a = smoothing; BCEWithLogitsLossZSmooth, :240-304:
 *                       a = alpha_z[z], a DEVICE table of `z` floats indexed by (index inside the V-plane) / (V / z))
 *   RX_LOSS_BCE_PROB    nn.BCELoss on probabilities, with torch's clamps (log >= -100 forward, x(1-x) >= 1e-12 backward)
 *   RX_LOSS_MSE         (x - t)^2
 * `alpha_z` may be NULL (then `smoothing` is the constant a and `z` is ignored); non-NULL needs kind BCE_LOGITS, z >= 1,
 * V % z == 0, V < 2^31.  ws: rx_loss_workspace(n, c, v) bytes.  Nothing is carried from fwd to bwd.  N*C < 65536. */
typedef enum { RX_LOSS_BCE_LOGITS = 0, RX_LOSS_BCE_PROB = 1, RX_LOSS_MSE = 2 } rx_elem_loss_kind;
typedef enum { RX_REDUCE_MEAN = 0, RX_REDUCE_SUM = 1 } rx_reduction;
int rx_elem_loss_fwd(int kind, const float* x, const float* target, int n, int c, long v, float smoothing,
                     const float* alpha_z, int z, int reduction, float* loss, void* ws, size_t ws_bytes, void* stream);
int rx_elem_loss_bwd(int kind, const float* x, const float* target, int n, int c, long v, float smoothing,
                     const float* alpha_z, int z, int reduction, const float* grad_loss, float* dx, void* stream);
/* nn.CrossEntropyLoss over the channel axis of (N, C, V) fp32 logits, 1 <= C <= 1024, N < 65536.  Exactly one of
 * `target_prob` ((N, C, V) fp32 class probabilities; mean divides by N*V) and `target_index` ((N, V) int64 class indices;
 * voxels equal to `ignore_index` -- or outside [0, C) -- contribute nothing; mean divides by the number of contributing
 * voxels, and is NaN with a zero gradient when there is none) is non-NULL.  `saved`: 2*N*V floats (N*V suffice for index
 * targets), the per-voxel log-sum-exp and target sum the backward reads; `coef`: 1 float, the backward's scale.
 * ws: rx_cross_entropy_loss_workspace() bytes. */
size_t rx_cross_entropy_loss_workspace(int n, int c, long v);
int rx_cross_entropy_loss_fwd(const float* logits, const float* target_prob, const int64_t* target_index,
                              int64_t ignore_index, int n, int c, long v, int reduction, float* loss, float* coef,
                              float* saved, void* ws, size_t ws_bytes, void* stream);
int rx_cross_entropy_loss_bwd(const float* logits, const float* target_prob, const int64_t* target_index,
                              int64_t ignore_index, int n, int c, long v, const float* coef, const float* saved,
                              const float* grad_loss, float* dlogits, void* stream);

/* ---- optimizer step fused with the weight re-pack (torch.optim.AdamW arithmetic: decoupled weight decay, bias
 *      correction; train.py:69-86 selects AdamW) -- one pass over a conv / convT weight updates p, exp_avg, exp_avg_sq
 *      and rewrites both packed copies.  `clip` is an optional DEVICE scalar multiplied into the gradient
 *      (clip_grad_norm_, train.py:227).  kind 0: Conv3d weight (Co,Ci,T); kind 1: ConvTranspose3d weight (Ci,Co,T).
 *      rx_adamw_flat: the same update for parameters that have no packed copy (stem, biases, heads). */
int rx_adamw_pack(rx_dtype dt, float* p, const float* grad, float* exp_avg, float* exp_avg_sq, const float* clip, double lr,
                  double beta1, double beta2, double eps, double weight_decay, int step, int kind, int A, int B, int taps,
                  void* w_fwd, void* w_bwd, void* stream);
int rx_adamw_flat(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, const float* clip, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, long n, void* stream);
/* Global L2 norm of a list of fp32 gradient tensors and the clip coefficient of torch.nn.utils.clip_grad_norm_(params,
 * max_norm) (train.py:227) in two launches: out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6)); the coefficient is what
 * rx_adamw_flat(_multi) / rx_adamw_pack take as `clip`.  Deterministic (fixed summation order).  `partial`: device scratch of
 * rx_grad_norm_clip_partials(count, numel) floats.  Pointer arrays are host arrays. */
long rx_grad_norm_clip_partials(int count, const long* numel);
int rx_grad_norm_clip(int count, const float* const* grad, const long* numel, float max_norm, float* partial, long partial_len,
                      float* out, void* stream);
/* the same for `count` tensors of one param group (shared hyper-parameters and step): HOST arrays of device pointers */
int rx_adamw_flat_multi(int count, float* const* p, const float* const* grad, float* const* exp_avg,
                        float* const* exp_avg_sq, const long* numel, const float* clip, double lr, double beta1,
                        double beta2, double eps, double weight_decay, int step, void* stream);
/* SGD with momentum / Nesterov (torch.optim.SGD arithmetic in fp32; train.py:70-77 selects SGD(momentum=0.9, nesterov=True)):
 *   g' = g * clip;  d = wd != 0 ? g' + wd * p : g';  buf = first ? d : momentum * buf + (1 - dampening) * d;
 *   u = nesterov ? d + momentum * buf : buf  (momentum == 0: u = d);  p -= lr * u
 * `buf` (momentum buffers) is NULL iff momentum == 0.  `first` != 0: the buffers do not exist yet -- they are written, never
 * read -- and it holds for the whole call.  `clip`: optional DEVICE scalar, as for AdamW.  nesterov needs momentum > 0 and
 * dampening == 0 (RX_EINVAL otherwise).  rx_sgd_flat_multi: `count` tensors, HOST arrays of device pointers;
 * rx_sgd_pack: one conv / convT weight (kind, A, B, taps <= 27, w_fwd, w_bwd as in rx_adamw_pack), both packed copies rewritten. */
int rx_sgd_flat_multi(int count, float* const* p, const float* const* grad, float* const* buf, const long* numel,
                      const float* clip, double lr, double momentum, double dampening, double weight_decay, int nesterov,
                      int first, void* stream);
int rx_sgd_pack(rx_dtype dt, float* p, const float* grad, float* buf, const float* clip, double lr, double momentum,
                double dampening, double weight_decay, int nesterov, int first, int kind, int A, int B, int taps, void* w_fwd,
                void* w_bwd, void* stream);

/* ---- launch programs: the launch list of a forward / backward pass, recorded once and replayed from C ------------------
 * The reference's model call is ONE Python call (`model(x)`, train.py:204; `loss.backward()`, :224) behind which the
 * framework issues its kernels natively.  A host-language loop over ~700 entry points per step costs ~8 ms of host time;
 * a program issues the same calls from C.  Between rx_prog_begin and rx_prog_end every entry point above that takes a
 * `stream` BOTH executes as usual AND appends itself -- arguments by value, rx_act / kernel / stride copied -- to the
 * program (the recording pass is an ordinary step).  Streams are recorded by index into `streams` and substituted from
 * the table given to rx_prog_run; device pointers are recorded as they are, so a program is valid as long as the buffers
 * it was recorded on live at the same addresses.  rx_prog_run(first, last) replays commands [first, last) (last < 0: to
 * the end) and returns the first non-zero status.  With `ms` != NULL (last - first floats) every command is bracketed by
 * timing events on its stream and the streams are synchronised before returning (profiling replay; the only entry point
 * that synchronises). */
typedef struct rx_prog rx_prog;
rx_prog* rx_prog_create(void);
void rx_prog_destroy(rx_prog* p);
int rx_prog_begin(rx_prog* p, void* const* streams, int n_streams);
int rx_prog_end(rx_prog* p);
int rx_prog_len(const rx_prog* p);
const char* rx_prog_cmd_name(const rx_prog* p, int i);   /* entry point of command i */
const char* rx_prog_cmd_kernel(const rx_prog* p, int i); /* kernel instantiation it dispatched at record time ("" if not a conv) */
int rx_prog_cmd_stream(const rx_prog* p, int i);         /* index into the stream table */
int rx_prog_run(rx_prog* p, int first, int last, void* const* streams, int n_streams, float* ms);
/* numbered events for cross-stream ordering (recordable like everything else): rx_stream_wait makes `stream` wait for the
 * work captured by the last rx_event_record(slot) issued before it. */
int rx_event_new(void);
/* return a slot to the library (a plan frees its slots when it is destroyed; programs that mention the slot must be destroyed
 * first).  rx_event_slots_in_use: how many slots are handed out right now (leak checks). */
int rx_event_free(int slot);
int rx_event_slots_in_use(void);
int rx_event_record(int slot, void* stream);
int rx_stream_wait(int slot, void* stream);

/* ---- streaming sliding-window inference (reference inference.py:115-157 patch loop, :166-210 overlap processing, :251-263
 *      cast; dataloading/inference_dataset.py:60-71 input normalisation).  Volumes on the device are RING SLABS: a
 *      (C, ring, Y, X) array whose ring row r holds volume row z with z % ring == r, so rows can be replaced as the window
 *      moves down Z.  `origins` is a HOST array of batch x (z, y, x) patch origins, z an absolute volume row (batch <= 32).
 *      No entry point here records itself into a launch program. ---------------------------------------------------------- */
typedef enum { RX_SW_U8 = 0, RX_SW_U16 = 1, RX_SW_F32 = 2 } rx_sw_in_dtype;
typedef enum { RX_SW_SCALE = 0, RX_SW_ZSCORE = 1 } rx_sw_norm;
typedef enum { RX_SW_BLEND_AVERAGE = 0, RX_SW_BLEND_UNIT = 1, RX_SW_BLEND_NONE = 2 } rx_sw_blend;
typedef enum { RX_SW_CAST_U8 = 0, RX_SW_CAST_U16 = 1 } rx_sw_cast;
/* fp64 scratch of the zscore statistics of rx_sw_gather */
size_t rx_sw_gather_workspace(int batch, int cin, int pz, int py, int px);
/* input slab -> out (batch, cin, pz, py, px) fp32, contiguous and 16-byte aligned.  RX_SW_SCALE: uint8 / 255, uint16 / 65535,
 * fp32 as is (fp32 division, dataset.py:179-184).  RX_SW_ZSCORE: then (v - mean) / max(std, 1e-10) per patch over all its
 * channels, population std, statistics summed in fp64 in a fixed order (ws: rx_sw_gather_workspace() bytes). */
int rx_sw_gather(int in_dtype, const void* slab, int cin, int ring, int y, int x, int batch, const int32_t* origins, int pz,
                 int py, int px, int norm, float* out, void* ws, size_t ws_bytes, void* stream);
/* one task's logits (batch, c, pz, py, px) fp32 -> act (rx_head_act, fp32, softmax over c with the max subtracted) -> for the
 * first `valid` patches, in patch order: sum (c, ring, Y, X) += weight * p and, if wsum != NULL, wsum (ring, Y, X) += weight,
 * weight a (pz, py, px) fp32 table.  Deterministic (no atomics): each destination voxel adds the patches in order.  The rows
 * [min z, max z + pz) of the batch must fit the ring. */
int rx_sw_accumulate(const float* logits, int batch, int valid, int c, int pz, int py, int px, const int32_t* origins, int act,
                     const float* weight, float* sum, float* wsum, int ring, int y, int x, void* stream);
/* volume rows [z0, z0 + rows) of the ring accumulators -> blended (c, rows, Y, X) fp32 and final (c, rows, Y, X) uint8
 * (RX_SW_CAST_U8: clip(v*255, 0, 255)) or uint16 (RX_SW_CAST_U16: clip((v+1)/2*65535, 0, 65535)), truncating.  Where wsum > 0:
 * RX_SW_BLEND_AVERAGE v = s / wsum, RX_SW_BLEND_UNIT (c == 3) v = s / (sqrt(sum s^2) + 1e-8), RX_SW_BLEND_NONE v = s; elsewhere
 * v = s.  wsum_out (optional): the weight sum of those rows.  reset 1: the rows of sum are zeroed after reading, 2: those of
 * wsum too (ring rows are then ready for the rows that follow). */
int rx_sw_finalize(float* sum, float* wsum, int c, int ring, int y, int x, int z0, int rows, int blend, int cast, int reset,
                   float* blended, void* final_out, float* wsum_out, void* stream);
/* empty-patch skipping: counts[i] = the raw voxels v of the patch at origins[i], over all cin channels, with (float)v > value (a
 * float compare: a NaN never counts; uint8 / uint16 are exact in fp32).  `origins`: n_pos x (z, y, x) in HOST memory (any n_pos
 * >= 0, handed to the kernels by value, 256 patches per launch); `counts`: n_pos uint64 on the device, 8-byte aligned, zeroed by
 * the call.  Integer adds only: exact and reproducible.  RX_EINVAL before anything is launched: an origin that leaves the slab,
 * a patch that does not fit it, rows [min z, max z + pz) that do not fit the ring, a misaligned slab or counts pointer. */
int rx_sw_occupancy(int in_dtype, const void* slab, int cin, int ring, int y, int x, int n_pos, const int32_t* origins, int pz,
                    int py, int px, float value, uint64_t* counts, void* stream);

/* ---- training augmentation on the device (reference dataloading/dataset.py:171-205; host restatement dataloading/augment.py).
 *      The image batch is contiguous fp32 (batch, c, z, y, x).  Parameters are drawn on the host and passed as ONE table per
 *      batch: `batch` rx_aug_sample records followed by a pool of 4-byte words that the records' offsets index (fp32 (z, y)
 *      factor planes, fp32 k x k filter weights in row-major tap order, int32 index tables of downscale: z source rows, then y
 *      source columns).  Every entry point takes the table twice: `host_table`, read during the call to validate every size,
 *      offset and box (a bad table returns RX_EINVAL before anything is launched), and `table`, the same bytes on the device,
 *      16-byte aligned, copied by the caller on `stream`.  A sample applies, in this order:
 *        two pointwise stages  RX_AUG_PW_AFFINE v = clip(v * pw_a + pw_b)   RX_AUG_PW_PLANE v = clip(v * pool[pw_off + z*Y + y] + pw_b)
 *                              RX_AUG_PW_NOISE  v = clip(v + pw_a * n), n standard normal: Philox4x32-10, key (key_lo, key_hi),
 *                              counter = (linear (z, y, x) index of the voxel) / 4 -- the channel is not part of it --, the top 24
 *                              bits of each output + 1 scaled by 2^-24 -> uniforms in (0, 1], Box-Muller pairs (u0, u1), (u2, u3)
 *                              -> n0 = r0 cos, n1 = r0 sin, n2 = r1 cos, n3 = r1 sin, voxel i of the quad takes n_i;
 *        one group-3 member    RX_AUG_G3_FILTER k x k correlation in the (z, y) plane, k odd in 3..21, border reflect-101, fp32
 *                              sum in row-major tap order, then clip;  RX_AUG_G3_DOWNSCALE v = src[zi[z], yi[y], x];
 *        nbox dropout boxes    (z0, y0, x0, d, h, w) inside the patch, filled with `fill`.
 *      clip is to [0, 1]; products and sums are separate fp32 operations (no FMA contraction).  Deterministic, no atomics. */
#define RX_AUG_MAX_K 21
#define RX_AUG_MAX_BOXES 4
typedef enum { RX_AUG_PW_NONE = 0, RX_AUG_PW_AFFINE = 1, RX_AUG_PW_PLANE = 2, RX_AUG_PW_NOISE = 3 } rx_aug_pw_mode;
typedef enum { RX_AUG_G3_NONE = 0, RX_AUG_G3_FILTER = 1, RX_AUG_G3_DOWNSCALE = 2 } rx_aug_g3_mode;
typedef struct {
  int32_t pw_mode[2];
  float pw_a[2], pw_b[2]; /* factor (AFFINE) or sigma (NOISE); offset */
  int32_t pw_off[2];      /* pool word of the (z, y) plane (PLANE) */
  uint32_t key_lo, key_hi;
  int32_t g3_mode, k, g3_off; /* pool word of the k*k weights or of the z + y indices */
  int32_t nbox;
  int32_t box[RX_AUG_MAX_BOXES][6];
  float fill;
  int32_t pad_; /* 160 bytes: the pool that follows stays 16-byte aligned */
} rx_aug_sample;
/* bytes of the scratch batch that samples with a group-3 member pass through */
size_t rx_aug_workspace(int batch, int c, int z, int y, int x);
/* pass 1: the pointwise stages of every sample; a sample without a group-3 member also gets its boxes and lands in `out`, the
 * others land in `scratch` (may be NULL when no sample has one).  1 read + 1 write per voxel; in != out. */
int rx_aug_pointwise(const float* in, float* out, float* scratch, size_t scratch_bytes, int batch, int c, int z, int y, int x,
                     const rx_aug_sample* host_table, const void* table, long pool_words, void* stream);
/* pass 2: the group-3 member and the boxes of the samples that have one, scratch -> out; other samples are not touched. */
int rx_aug_filter_zy(const float* scratch, float* out, int batch, int c, int z, int y, int x, const rx_aug_sample* host_table,
                     const void* table, long pool_words, void* stream);
/* test hook: the raw Philox outputs behind the noise of the first n voxels of a patch, out[i] = philox(key, i / 4)[i % 4] */
int rx_aug_philox_u32(uint64_t key, long n, uint32_t* out, void* stream);

/* ---- axis flips and 90-degree rotations on the device, with the component rule of a 3-vector field (reference
 *      training/transforms/geometric/geometry.py; host side dataloading/geometry_device.py).  One gather pass per tensor:
 *        out[b][c][o] = (+/-) in[b][cs(c)][i],   i[src_axis[d]] = flip[d] ? n_d - 1 - o_d : o_d   (d = 0, 1, 2 = z, y, x)
 *      cs(c) = ch_src[c] with the sign bit flipped where ch_neg[c] for a vector tensor (`vector` != 0, needs c == 3); cs(c) = c
 *      and no sign change otherwise.  Any chain of flips and rotations is one such record (they compose on the host).  A negated
 *      0.0 is -0.0 (the sign bit is XORed; nothing is multiplied). */
typedef struct {        /* one sample's transform, 48 bytes */
  int32_t src_axis[3];  /* output axis d (0=z,1=y,2=x) reads input axis src_axis[d]            */
  int32_t flip[3];      /* ... at coordinate flip[d] ? n_d-1-o_d : o_d                         */
  int32_t ch_src[3];    /* vector tensors: output component c reads input component ch_src[c] */
  int32_t ch_neg[3];    /* ... with its sign bit flipped if ch_neg[c]                          */
} rx_geom_sample;
/* in / out: contiguous fp32 (batch, c, z, y, x), distinct buffers.  `host_table`: `batch` records in HOST memory, read during
 * the call and handed to the kernels by value (16 samples per launch): no device table, copy, allocation or synchronisation.
 * RX_EINVAL before anything is launched: null pointers, in == out, src_axis or ch_src not a permutation of 0..2, a permutation
 * that would change the shape (extent[src_axis[d]] != extent[d]), vector with c != 3, z * y * x >= 2^31, z or y > 65535,
 * c > 4095.  One read and one write of the tensor for every record. */
int rx_geom_apply(const float* in, float* out, int batch, int c, int z, int y, int x, const rx_geom_sample* host_table,
                  int vector, void* stream);

/* ---- test-time augmentation of streaming inference: rx_sw_gather / rx_sw_accumulate with a table of one rx_geom_sample per patch
 *      slot (`ops`: `batch` records in HOST memory, handed to the kernels by value; no device table, copy or synchronisation).  One
 *      family: each _geom entry point runs the host path and the kernel body of its plain twin, with the table as the one thing
 *      added, so "with identity records, bit for bit" below holds by construction.  Both use the
 *      gather form of rx_geom_apply on the PATCH: out[o] = in[i(o)], i[src_axis[d]] = flip[d] ? n_d - 1 - o_d : o_d.
 *      rx_sw_gather_geom: output voxel o of slot b is slab voxel origin_b + i(o) (z modulo the ring), scaled and standardised as
 *      rx_sw_gather does; image channels are never permuted or negated.  With identity records it is rx_sw_gather, bit for bit.
 *      rx_sw_accumulate_geom: `ops` are the records to APPLY to the prediction (a view's inverse).  Destination voxel l of slot b
 *      adds weight[l] * q, q the activated logit at i(l) -- the activation runs over the view-frame channels first; with `vector`
 *      (needs c == 3) destination channel ch takes activated channel ch_src[ch], its sign bit flipped where ch_neg[ch] (-0.0 is
 *      kept).  The weight is indexed by the destination voxel.  Slots are added in slot order, no atomics; with identity records
 *      it is rx_sw_accumulate, bit for bit.  RX_EINVAL before anything is launched: everything rx_sw_gather / rx_sw_accumulate
 *      refuse, a null table, src_axis or ch_src not a permutation of 0..2, a permutation that would change the patch shape,
 *      vector with c != 3. */
int rx_sw_gather_geom(int in_dtype, const void* slab, int cin, int ring, int y, int x, int batch, const int32_t* origins,
                      const rx_geom_sample* ops, int pz, int py, int px, int norm, float* out, void* ws, size_t ws_bytes,
                      void* stream);
int rx_sw_accumulate_geom(const float* logits, int batch, int valid, int c, int pz, int py, int px, const int32_t* origins,
                          const rx_geom_sample* ops, int vector, int act, const float* weight, float* sum, float* wsum, int ring,
                          int y, int x, void* stream);

/* ---- label dilation on the device (reference dataloading/dataset.py: `dilate_label`, dilation(t > 0, ball(5)); host side
 *      dataloading/dilate_device.py).  Every (sample, channel) volume of a contiguous fp32 (batch, c, z, y, x) tensor on its own:
 *        out[v] = 1.0f if some voxel u with in[u] > 0.0f lies within |u - v|^2 <= radius^2, else +0.0f
 *      (a float compare: NaN, -0.0 and negatives are off).  Nothing outside the volume is on: no wrap, no reflection, the border
 *      rule of skimage's dilation and of scipy's binary_dilation.  The input is packed to one bit per voxel in `scratch` first
 *      (64 voxels of an x row to a word) and read nowhere else, so out == in is allowed.  One fp32 read and one fp32 write. */
size_t rx_dilate_workspace(int batch, int c, int z, int y, int x);
    /* bytes of scratch: batch*c*z*y*ceil(x/64) 64-bit words (0 on invalid sizes) */
/* radius 1..8; any positive z, y, x (extents below the radius and x % 64 != 0 included), z * y * x < 2^31 per sample; `scratch`
 * 8-byte aligned.  RX_EINVAL before anything is launched: null pointers, non-positive sizes, a radius out of range;
 * RX_EWORKSPACE: scratch_bytes below rx_dilate_workspace(...). */
int rx_label_dilate(const float* in, float* out, void* scratch, size_t scratch_bytes, int batch, int c, int z, int y, int x,
                    int radius, void* stream);

/* ---- box statistics on the device: what the valid-patch search asks of every candidate patch (reference helpers.py:
 *      _check_patch_chunk, find_label_bounding_box; host side dataloading/patch_search_device.py).  `vol` is a contiguous
 *      (z, y, x) device array of `dtype` (rx_sw_in_dtype: RX_SW_U8, RX_SW_U16, RX_SW_F32; anything else is RX_EINVAL), aligned
 *      to its element size.  `host_boxes` holds n_boxes records (z0, y0, x0, dz, dy, dx) in HOST memory; per box i
 *        count[i] = the number of voxels != 0 (np.count_nonzero: a NaN and a negative count, -0.0 does not)
 *        ext[i]   = (minz, maxz, miny, maxy, minx, maxx) of the voxels > 0 in BOX-LOCAL coordinates (NaN, negatives and -0.0
 *                   do not extend it); (dz, -1, dy, -1, dx, -1) when the box has no voxel > 0, the reference's empty record.
 *      For the integer dtypes the two predicates are the same.  The global bounding box of a volume is the call with one box
 *      that covers it.  The table is copied into `workspace` on `stream` (host_boxes must stay valid and unchanged until the
 *      stream is synchronised), and count / ext are initialised on the stream by the call, not by the caller.
 *      A box is cut along z -- and below a plane along y -- into chunks of whole x-rows, one workgroup each, so one volume-sized
 *      box and thousands of patch-sized ones both fill the device; a launch gives every box the chunk grid of its largest box,
 *      so keep the boxes of one call of similar size.  Rows are read with 16-byte loads between a scalar head and tail (x0 is
 *      arbitrary), reduced per lane, wave and workgroup, then merged with one integer atomic per workgroup and output word
 *      (add on the 64-bit count, min / max on the extents): the result does not depend on arrival order, a launch is
 *      bit-reproducible, and there is no floating-point arithmetic.  Voxel offsets are 64-bit: z * y * x may exceed 2^31, only
 *      z, y and x themselves are int32.  Overlapping and duplicate boxes are allowed; every box reads its own voxels.
 *      RX_EINVAL before anything is launched or copied: null pointers, non-positive z / y / x, n_boxes <= 0, an unknown dtype,
 *      a box with a non-positive extent or one that leaves the volume, vol not aligned to its element, workspace not 16-byte,
 *      count not 8-byte or ext not 4-byte aligned; RX_EWORKSPACE: workspace_bytes below rx_box_stats_workspace(n_boxes). */
size_t rx_box_stats_workspace(int n_boxes); /* bytes of the device box table, a multiple of 16 (0 for n_boxes <= 0) */
int rx_box_stats(const void* vol, int dtype, int z, int y, int x, const int32_t* host_boxes, int n_boxes, void* workspace,
                 size_t workspace_bytes, uint64_t* count, int32_t* ext, void* stream);

/* ---- raw patches -> the float32, channel-first training batch (reference dataloading/dataset.py __getitem__: astype(float32), the
 *      dtype scaling, and transpose(3, 0, 1, 2) of a channels-last normals store; host side dataloading/ingest_device.py).  `in`
 *      holds `batch` contiguous samples of `dtype` (rx_sw_in_dtype), each (z, y, x) for c == 1 or channels-last (z, y, x, c) for
 *      1 < c <= 8; `out` is contiguous fp32 (batch, c, z, y, x).  One rule per call, in float32 as numpy evaluates it (true IEEE
 *      division; the result has the bits of ingest_device.ingest_numpy):
 *        RX_INGEST_COPY         v                      (a float32 input is copied bit for bit: -0.0, NaN payloads, denormals)
 *        RX_INGEST_DIV255       v / 255                RX_INGEST_DIV65535     v / 65535
 *        RX_INGEST_NORMAL_U16   v / 32767.5 - 1        RX_INGEST_NORMAL_MUL2  v * 2 - 1
 *      Every rule takes every dtype.  One read of the input at its storage width and one fp32 write: 16-byte loads and stores
 *      between a scalar head and tail per sample (samples need no alignment beyond their element); c > 1 goes through LDS, a
 *      contiguous run of voxels in, one coalesced run per plane out.  No workspace, no copy, no synchronisation.
 *      RX_EINVAL before anything is launched: null pointers, in == out, an unknown dtype or rule, non-positive batch or extents,
 *      c > 8, z * y * x * c >= 2^31, `in` not aligned to its element or `out` not 4-byte aligned. */
typedef enum {
  RX_INGEST_COPY = 0,
  RX_INGEST_DIV255 = 1,
  RX_INGEST_DIV65535 = 2,
  RX_INGEST_NORMAL_U16 = 3,
  RX_INGEST_NORMAL_MUL2 = 4
} rx_ingest_rule;
int rx_ingest(const void* in, int dtype, float* out, int batch, int z, int y, int x, int c, int rule, void* stream);

/* ---- rotation and isotropic scaling about the patch centre on the device, with the vector rule of a 3-component field (the
 *      continuous counterpart of rx_geom_apply; host side dataloading/spatial_device.py, whose affine_numpy is the statement).
 *      One resampling pass per tensor.  For output voxel o of sample b, per axis d in (z, y, x), all in float32, one rounding per
 *      operation, nothing contracted into an fma, denormals kept:
 *        c_d = (float)(n_d - 1) * 0.5          t_d = (float)o_d - c_d
 *        p_d = ((point[3d] * t_z + point[3d+1] * t_y) + point[3d+2] * t_x) + c_d
 *      RX_AFFINE_LINEAR:  i_d = floor(p_d), f_d = p_d - i_d, the eight corners i and i + 1, lerp(a, b, f) = a + f * (b - a) along
 *                         x, then y, then z.      RX_AFFINE_NEAREST: the source index is floor(p_d + 0.5).
 *      RX_AFFINE_CONSTANT: a corner / source voxel with an index outside [0, n_d - 1] has the value `fill`;
 *      RX_AFFINE_CLAMP:    its index is clamped to [0, n_d - 1].
 *      `vector` != 0 (needs c == 3): with s the three sampled components, out_k = (vector[3k] * s_0 + vector[3k+1] * s_1) +
 *      vector[3k+2] * s_2; otherwise channels are sampled one by one.  All channels of a sample share one set of coordinates. */
typedef enum { RX_AFFINE_LINEAR = 0, RX_AFFINE_NEAREST = 1 } rx_affine_interp;
typedef enum { RX_AFFINE_CONSTANT = 0, RX_AFFINE_CLAMP = 1 } rx_affine_border;
typedef struct {      /* one sample's transform, 72 bytes */
  float point[9];     /* row-major 3 x 3, (z, y, x) axis order: output voxel offsets from the centre -> input voxel offsets */
  float vector[9];    /* row-major 3 x 3, component order: the rotation of a vector tensor's three channels           */
} rx_affine_sample;
/* in / out: contiguous fp32 (batch, c, z, y, x), distinct buffers.  `host_table`: `batch` records in HOST memory, read during
 * the call and handed to the kernels by value (16 samples per launch): no device table, copy, allocation or synchronisation.
 * No load leaves a sample, whatever the matrices hold.  RX_EINVAL before anything is launched: null pointers, in == out, an
 * unknown interp or border, vector with c != 3, a matrix entry that is not finite, z * y * x >= 2^31, z or y > 65535,
 * x > 2^24 (float32 coordinates), c > 4095.  One write of the tensor; every source voxel a brick needs is read through L1 / L2. */
int rx_affine_apply(const float* in, float* out, int batch, int c, int z, int y, int x, const rx_affine_sample* host_table,
                    int interp, int border, float fill, int vector, void* stream);

/* ---- smooth non-rigid deformation on the device, with the vector rule of a 3-component normal field (host side
 *      dataloading/elastic_device.py, whose displacement_numpy and elastic_numpy are the statement).  One resampling pass per
 *      tensor: out(o) = in(o + D(o)), D a cubic B-spline displacement field over a node lattice of pitch `spacing`:
 *      G_d = (n_d - 1) / s_d + 4 nodes along axis d of (z, y, x).  The output grid is regular, so each axis arrives as a table over
 *      its voxel indices o: idx[o] = floor(o / s) (voxel o uses nodes idx[o] .. idx[o] + 3), w[o][0..3] the uniform cubic
 *      B-spline weights at f = o / s - idx[o], dw[o][0..3] their derivatives with respect to o (evaluated in float64, rounded
 *      once).  For component c of (z, y, x) at voxel (oz, oy, ox), all float32, one rounding per operation, nothing contracted
 *      into an fma, denormals kept, every sum from its first product on, left to right:
 *        L1[c][b][k] = sum_a w_z[oz][a] * nodes[c][iz+a][iy+b][ix+k]
 *        L2[c][k]    = sum_b w_y[oy][b] * L1[c][b][k]
 *        D_c         = sum_k w_x[ox][k] * L2[c][k]                 (z, then y, then x: an L2 line serves a whole x row)
 *        E[d][e]     = the same three sums with dw on axis e and w on the other two          (dD_d / do_e)
 *        p_d = (float)o_d + D_d
 *      From p_d on the rules are rx_affine_apply's: RX_AFFINE_LINEAR / _NEAREST, RX_AFFINE_CONSTANT (`fill`) / _CLAMP, lerp along
 *      x, then y, then z.  All channels of a sample share one set of coordinates.
 *      `vector` != 0 (needs c == 3, channels (Nx, Ny, Nz)): with s the sampled components and (n_z, n_y, n_x) = (s_2, s_1, s_0),
 *        t_e = n_e + ((E[z][e] * n_z + E[y][e] * n_y) + E[x][e] * n_x)                        (a normal is a covector)
 *        q = (s_0*s_0 + s_1*s_1) + s_2*s_2     r = (t_x*t_x + t_y*t_y) + t_z*t_z     k = r > 0 ? sqrt(q / r) : 0
 *      with correctly rounded sqrt and /; output channel j is t_(x, y, z)[j] * k: the sampled length is kept, zero stays zero. */
typedef struct {         /* one axis, DEVICE pointers */
  const int32_t* idx;    /* [n]    */
  const float* w;        /* [n][4] */
  const float* dw;       /* [n][4] */
} rx_elastic_axis;
typedef struct { rx_elastic_axis z, y, x; } rx_elastic_tables;
/* in / out: contiguous fp32 (batch, c, z, y, x), distinct buffers.  `nodes`: DEVICE, fp32 (batch, 3, Gz, Gy, Gx).  `spacing` and
 * `tables`: HOST, read during the call (the pointers inside `tables` are device pointers and ride in the kernel arguments).  No
 * allocation, copy or synchronisation.  Device data cannot be validated here (the Python wrapper refuses nodes that are not
 * finite before upload); whatever nodes and tables hold, every node load is clamped into the lattice and every source load into
 * the sample.  RX_EINVAL before anything is launched: null pointers, in == out, an unknown interp or border, vector with
 * c != 3, a spacing < 8, z * y * x >= 2^31, z or y > 65535, x > 2^24 (float32 coordinates), c > 4095, batch > 65535.  One
 * write of the tensor; source voxels are read through L1 / L2; 3.2 KB of LDS whatever the lattice. */
int rx_elastic_apply(const float* in, float* out, int batch, int c, int z, int y, int x, const float* nodes, const int32_t spacing[3],
                     const rx_elastic_tables* tables, int interp, int border, float fill, int vector, void* stream);

/* ---- validation metrics on the device (host side training/metrics/metrics.py, whose seg_counts_numpy, class_counts_numpy and
 *      normal_stats_numpy are the statements).  Operands are contiguous (n, c, v) device arrays: `pred` of `pred_dtype` (rx_dtype),
 *      aligned to its element, `target` fp32, 4-byte aligned (a base that is not 16-byte aligned is fine).  Every entry point ADDS
 *      into its output buffers: the caller zeroes them once and accumulates over as many calls as it likes, with no extra kernel
 *      and no synchronisation.  One read of each operand: a row is a scalar head up to the first 16-byte boundary of the
 *      prediction, 16-byte vectors, a scalar tail; nothing outside [0, v) of a row is read; voxel offsets are 64-bit.  Integer
 *      results are reduced per lane, wave and workgroup, then merged with one 64-bit atomic add per workgroup and output word, so
 *      they do not depend on arrival order.  RX_EINVAL before anything is launched, for all of them: null pointers, non-positive
 *      n / c / v, an unknown dtype, a misaligned pointer.
 *      rx_seg_counts: binary confusion per (sample, channel).  Predicted positive is pred > thr_pred, labelled positive is
 *        target > thr_target, both IEEE float32 comparisons (a NaN is negative; a NaN threshold is RX_EINVAL).
 *        counts: int64 (n, c, 3) = (TP, FP, FN); TN is v minus their sum.
 *      rx_class_counts: multi-class confusion by arg-max over the c channels, 2 <= c <= 64 (else RX_EINVAL).  The predicted class
 *        is best = 0; for k = 1 .. c-1: if x[k] > x[best], or x[best] is a NaN and x[k] is not: best = k -- the first maximum wins
 *        and a NaN is never chosen over a number.  The label is the same rule on the fp32 target_prob (n, c, v), or
 *        target_index int64 (n, v), 8-byte aligned; exactly one of the two is non-null.  Voxels whose index equals ignore_index,
 *        or is no class at all (outside [0, c)), are skipped.  counts: int64 (n, c, 3) = per-class (TP, FP, FN): a voxel with
 *        label l predicted as p adds TP[l] if p == l, else FP[p] and FN[l].
 *      rx_normal_stats: 3-channel vector fields (n, 3, v).  In float32, one rounding per operation: the mask is
 *        sqrt((tx*tx + ty*ty) + tz*tz) > 1e-6 (the mask of MaskedCosineLoss); per masked voxel
 *        cos = dot / (max(|p|, 1e-8) * max(|t|, 1e-8)) clamped to [-1, 1], deg = acos(cos) * (180 / pi).
 *        count: int64 (n) += the masked voxels; sums: float64 (n, 2) += (sum of cos, sum of deg).  The float sums never go
 *        through an atomic: per-workgroup fp64 partials in `ws` (8-byte aligned), then a finalize that adds a sample's partials in
 *        index order, so two runs on the same input give the same bits.  RX_EWORKSPACE: ws_bytes below
 *        rx_normal_stats_workspace(n, v). */
int rx_seg_counts(const void* pred, int pred_dtype, const float* target, int n, int c, long v, float thr_pred, float thr_target,
                  int64_t* counts, void* stream);
int rx_class_counts(const void* pred, int pred_dtype, const float* target_prob, const int64_t* target_index, int64_t ignore_index,
                    int n, int c, long v, int64_t* counts, void* stream);
size_t rx_normal_stats_workspace(int n, long v); /* bytes of partials (0 for non-positive arguments) */
int rx_normal_stats(const void* pred, int pred_dtype, const float* target, int n, long v, int64_t* count, double* sums, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- surface-distance validation metrics on the device (host side training/metrics/surface.py, whose edges_numpy, edt_sq_numpy
 *      and surface_hist_numpy are the statements).  A volume is a contiguous (z, y, x) block; `n` volumes lie back to back
 *      (n = samples * channels).  Distances are in voxels, isotropic, squared, exact integers; no floating point beyond the one
 *      float32 comparison against the threshold.  Each extent is 1 .. RX_EDT_MAX_EXTENT.  No allocation, copy or synchronisation.
 *      RX_EINVAL before anything is launched, for all of them: null pointers, non-positive sizes, an extent above
 *      RX_EDT_MAX_EXTENT, a misaligned pointer, more volumes than one call's grid covers.
 *      rx_mask_edges: edges[v] = 1 where values[v] > threshold (IEEE float32; a NaN is off; a NaN threshold is RX_EINVAL) and v is
 *        on the border of its volume or one of its six face neighbours is off, else 0: mask & ~erode6(mask) with everything
 *        outside the volume off.  `values` of `dtype` (rx_dtype), aligned to its element; at most 65535 volumes.  No neighbour
 *        outside a voxel's own volume is ever read.
 *      rx_edt_sq: dist[v] = the squared Euclidean distance from v to the nearest voxel of its volume with feature != 0, or
 *        RX_EDT_NONE everywhere in a volume that has none.  Three passes, x then y then z, each
 *        g'[i] = min(RX_EDT_NONE, min_j (g[j] + (i - j)^2)) along its axis, from g = 0 on a feature and RX_EDT_NONE elsewhere; the
 *        y and z passes run in place on `dist` (int32, 4-byte aligned; `feature` must be another buffer).
 *      rx_surface_hist: over the `total` voxels of both arrays, for each voxel with edges != 0: count += 1, and unmatched += 1 if
 *        dist is RX_EDT_NONE (or no distance at all: negative), else hist[min(dist, bins - 1)] += 1.  hist: int64 (bins), count
 *        and unmatched: one int64 each, 8-byte aligned; everything is ADDED with integer atomics into buffers the caller zeroes,
 *        so the result does not depend on arrival order. */
#define RX_EDT_NONE (1 << 30)
#define RX_EDT_MAX_EXTENT 1024
int rx_mask_edges(const void* values, int dtype, float threshold, int n, int z, int y, int x, uint8_t* edges, void* stream);
int rx_edt_sq(const uint8_t* feature, int n, int z, int y, int x, int32_t* dist, void* stream);
int rx_surface_hist(const uint8_t* edges, const int32_t* dist, long total, long bins, int64_t* hist, int64_t* count, int64_t* unmatched,
                    void* stream);

/* ---- connected components of a thresholded uint8 volume (host side postprocess/components.py, whose label_numpy,
 *      component_sizes_numpy and filter_numpy are the statements).  A volume is a contiguous (z, y, x) block; `nvol` volumes lie back
 *      to back, at most 65535 of them, each of at most RX_CC_MAX_VOXELS = 2^31 - 2 voxels.  Integers only; no allocation, copy or
 *      synchronisation.  RX_EINVAL before anything is launched: null pointers, an extent of 0, more voxels or volumes than that, a
 *      connectivity other than 6, 18 or 26, a level outside 0 .. 254, a misaligned pointer.
 *      rx_cc_label: labels[v] = 0 where values[v] <= level, else 1 + the smallest linear index z*Y*X + y*X + x over the voxels of
 *        v's component of the mask values > level under `connectivity` (6 faces, 18 + edges, 26 + corners), within v's own volume.
 *        The label is a property of the mask alone: it does not depend on the order anything ran in.  `labels`: int32, 4-byte
 *        aligned, another buffer than `values`.  Up to five launches: tiles, the tile faces of each axis, roots.
 *      rx_cc_sizes: sizes (int32, nvol * voxels words) is zeroed, then sizes[volume * voxels + label - 1] += 1 for every voxel with a
 *        label in 1 .. voxels: at a component's root its voxel count, 0 everywhere else.  Integer atomics.
 *      rx_cc_filter: out[v] = values[v] where labels[v] is in 1 .. voxels and sizes[volume * voxels + labels[v] - 1] >= min_voxels,
 *        else 0.  It compares whatever `sizes` holds.  `out` may be `values`. */
#define RX_CC_MAX_VOXELS 2147483646L
int rx_cc_label(const uint8_t* values, int level, int nvol, int z, int y, int x, int connectivity, int32_t* labels, void* stream);
int rx_cc_sizes(const int32_t* labels, int nvol, long voxels, int32_t* sizes, void* stream);
int rx_cc_filter(const uint8_t* values, const int32_t* labels, const int32_t* sizes, int min_voxels, int nvol, long voxels, uint8_t* out,
                 void* stream);

/* ---- triangle mesh of a uint8 volume by surface nets (host side postprocess/isosurface.py, whose surface_nets_numpy and counts_numpy
 *      are the statements).  `values` is a contiguous (z, y, x) block, padded with 0 on every side by the kernels themselves; inside is
 *      value > level.  Cells form a (z+1, y+1, x+1) grid, cell (k, j, i) with corner 0 at voxel (k-1, j-1, i-1); a cell ROW is (k, j),
 *      `rows` = (z+1) * (y+1) of them, and a row's bits are ceil((x+1) / 64) 64-bit words.  No allocation, copy or synchronisation; no
 *      output depends on the order anything ran in.  RX_EINVAL before anything is launched: null pointers, an extent of 0 or of
 *      2^24 - 2 or more (a position is an exact float32 integer plus a fraction), more than RX_ISO_MAX_CELLS = 2^31 - 2 cells, more than
 *      2^24 - 1 bands of 4 cell planes x 8 cell rows (ceil((z+1) / 4) * ceil((y+1) / 8): one workgroup each), a level
 *      outside 0 .. 254, a cell-plane window outside the grid, a misaligned pointer.
 *      rx_iso_classify: bits[row][word] = the active flags (corners not all inside, not all outside) of the row's cells, bit l of word w
 *        cell 64 w + l; row_counts[row] = {active cells, quads the row's cells own} (int32 pairs).  Cell planes outside [k_lo, k_hi)
 *        get zeros: a slab of a larger volume leaves out the planes whose voxels it does not hold (the whole volume: 0, z + 1).
 *      rx_iso_scan: row_offsets[row] = {sum of the active cells, sum of the quads} of the rows before it (int64 pairs, 16-byte
 *        aligned), totals[0..1] = the two sums over all rows.  Three launches.
 *      rx_iso_emit: for every active cell of planes >= k_emit, in ascending linear cell index, vertices[3 * (id - v_skip)] = its
 *        (x, y, z) with z_base added to the plane (float32, the statement's bits), id = row_offsets[row][0] + its rank in the row;
 *        for every quad those cells own, in (cell, axis z / y / x) order, triangles[6 * (slot - q_skip)] = its two triangles with
 *        vertex_base added to every id.  v_skip / q_skip: row_offsets[k_emit * (y+1)], which the caller has read; a slot outside
 *        0 .. n_vertices - 1 / n_quads - 1 is not written. */
#define RX_ISO_MAX_EXTENT 16777213
#define RX_ISO_MAX_CELLS 2147483646L
int rx_iso_classify(const uint8_t* values, int level, int z, int y, int x, int k_lo, int k_hi, uint64_t* bits, int32_t* row_counts,
                    void* stream);
int rx_iso_scan(const int32_t* row_counts, long rows, int64_t* row_offsets, int64_t* totals, void* stream);
int rx_iso_emit(const uint8_t* values, int level, int z, int y, int x, int z_base, const uint64_t* bits, const int64_t* row_offsets,
                int k_emit, int64_t v_skip, int64_t q_skip, int64_t vertex_base, int64_t n_vertices, int64_t n_quads, float* vertices,
                int64_t* triangles, void* stream);

/* ---- refinement of an indexed triangle mesh: canonical vertex adjacency, Taubin smoothing passes, area-weighted vertex normals (host
 *      side postprocess/refine.py, whose adjacency_numpy, smooth_numpy and vertex_normals_numpy are the statements).  `vertices`:
 *      float32 (x, y, z) triples; `triangles`: int64 id triples; at most RX_MESH_MAX_VERTICES vertices and RX_MESH_MAX_TRIANGLES
 *      triangles, because ids, triangle indices and a vertex's corner count are held as int32.  A triangle with an id outside
 *      [0, n_vertices) takes part in nothing and sets bit 0 of `flag` (caller-zeroed).  Every vertex owns the corner SLOTS
 *      [face_offsets[v], face_offsets[v + 1]); slot s holds its triangle in faces[s] and the corner's two edge partners in raw[2 s],
 *      raw[2 s + 1].  Every output has an explicit capacity outside which nothing is stored, and every list entry read back is
 *      checked against its range before it is followed.  No float atomics; no allocation, copy or synchronisation.  RX_EINVAL
 *      before anything is launched: null or misaligned pointers, sizes outside the limits, a non-finite factor, a negative clamp.
 *      rx_mesh_count: counts[v] = the triangle corners at v (zeroed first; integer atomics).
 *      rx_mesh_scan: offsets[i] = counts[0] + .. + counts[i - 1] for i = 0 .. n (n + 1 int64 values).  Up to three launches.
 *      rx_mesh_fill: every corner takes the next slot of its vertex at `cursor` (n_vertices int32, zeroed first) and fills it;
 *        `capacity`: the slots of `faces` (raw holds 2 * capacity).  Which slot a corner gets depends on arrival.
 *      rx_mesh_canonical: per vertex, faces and raw of its slots sorted ascending; the distinct partners other than the vertex
 *        itself moved to the front of its raw slots, degrees[v] their number; boundary[v] = some partner appeared exactly once.
 *        After it, nothing depends on the order anything ran in.
 *      rx_mesh_compact: neighbours[offsets[v] + r] = raw[2 * face_offsets[v] + r] for r < offsets[v + 1] - offsets[v], where
 *        offsets = rx_mesh_scan(degrees); `capacity`: the entries of `neighbours`.
 *      rx_mesh_check_vertices: bit 0 of `flag` is set when a coordinate is not finite.
 *      rx_mesh_smooth_pass: out[v] = p + factor * (m - p), m = (sum of the neighbours' positions in list order) / float(degree), p
 *        = positions[v]; with `origin`, each component then clamped to origin[v] -+ clamp.  A vertex of degree 0, or with
 *        boundary[v] != 0 (`boundary` may be null: nothing is pinned), keeps p.  `out` is another buffer than `positions`.
 *      rx_mesh_face_vectors: face_vectors[t] = cross(pb - pa, pc - pa) of triangle t = (a, b, c); (0, 0, 0) for a dropped one.
 *      rx_mesh_vertex_normals: normals[v] = the sum of face_vectors over the vertex's slots in order, divided by its length
 *        sqrt(x*x + y*y + z*z); (0, 0, 0) where that is 0.  `capacity`: the entries of `faces`. */
#define RX_MESH_MAX_VERTICES 2147483646L
#define RX_MESH_MAX_TRIANGLES 715827882L
int rx_mesh_count(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, int32_t* counts, int32_t* flag, void* stream);
int rx_mesh_scan(const int32_t* counts, int64_t n, int64_t* offsets, void* stream);
int rx_mesh_fill(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* face_offsets, int32_t* cursor,
                 int64_t capacity, int32_t* faces, int32_t* raw, void* stream);
int rx_mesh_canonical(int64_t n_vertices, const int64_t* face_offsets, int64_t capacity, int32_t* faces, int32_t* raw, int32_t* degrees,
                      uint8_t* boundary, void* stream);
int rx_mesh_compact(int64_t n_vertices, const int64_t* face_offsets, const int32_t* raw, int64_t raw_capacity, const int64_t* offsets,
                    int64_t capacity, int32_t* neighbours, void* stream);
int rx_mesh_check_vertices(const float* vertices, int64_t n_vertices, int32_t* flag, void* stream);
int rx_mesh_smooth_pass(const float* positions, const float* origin, int64_t n_vertices, const int64_t* offsets, const int32_t* neighbours,
                        int64_t n_neighbours, const uint8_t* boundary, float factor, float clamp, float* out, void* stream);
int rx_mesh_face_vectors(const float* vertices, int64_t n_vertices, const int64_t* triangles, int64_t n_triangles, float* face_vectors,
                         void* stream);
int rx_mesh_vertex_normals(int64_t n_vertices, const int64_t* face_offsets, const int32_t* faces, int64_t capacity, const float* face_vectors,
                           int64_t n_triangles, float* normals, void* stream);

/* ---- mesh decimation by vertex clustering on a uniform grid (host side postprocess/decimate.py, whose decimate_numpy is the
 *      statement).  Sizes as in the refinement group above; n_vertices, n_clusters and n_triangles are at least 1 (the caller
 *      handles empty meshes).  Counts, cursors, flags and list entries are int32, offsets are what rx_mesh_scan returns.  Every
 *      call refuses with a status and a message before anything is launched: null or misaligned pointers, sizes outside the
 *      limits, a cell that is not finite and > 0, a table capacity that is not a power of two above n_vertices.  No float
 *      atomics; nothing is stored beyond a stated capacity; after the calls nothing depends on the order anything ran in.
 *      rx_mesh_cluster_keys: keys[v] = ((k0 + 2^20) << 42) | ((k1 + 2^20) << 21) | (k2 + 2^20), k = floor(p / cell) per component;
 *        bit 0 of `flag` is set, and the key is -1, where some |k| >= 2^20.
 *      rx_mesh_cluster_assign: open-addressing table of `capacity` slots (table_keys int64, table_min int32, both cleared here),
 *        claimed by 64-bit compare-and-swap with linear probing, at most `capacity` probes (bit 1 of `flag` on exhaustion);
 *        slot_of[v] = the slot of v's key, table_min[slot] = the smallest id with that key, first[v] = v is that id.
 *      rx_mesh_cluster_number: cluster_of[v] = rank[smallest id of v's slot], rank = rx_mesh_scan(first): the clusters numbered
 *        by ascending smallest member; rank[n_vertices] is their number.
 *      rx_mesh_cluster_count / _fill: the member counts (zeroed first), and the members of cluster c in
 *        members[member_offsets[c] .. member_offsets[c + 1]) in arrival order (`cursor`: n_clusters int32, zeroed first).
 *      rx_mesh_cluster_mean: per cluster its member list sorted ascending in place, then representatives[c] = (the sum of the
 *        members' positions in that order, from 0) / float(n).
 *      rx_mesh_cluster_nearest: best[c] = the minimum over members of (bits of d) << 32 | id, d = dx*dx + dy*dy + dz*dz to the cell
 *        centre (float(k) + 0.5f) * cell; representatives[c] = the position of that id.
 *      rx_mesh_cluster_remap: a triangle whose corners lie in three different clusters sets used[c] = 1 for each and adds 1 to
 *        counts[its smallest cluster] (both zeroed first); bit 2 of `flag`: an id outside [0, n_vertices).
 *      rx_mesh_cluster_unique: those triangles stored as (middle, largest, triangle) at entry_offsets = rx_mesh_scan(counts) of
 *        their smallest cluster (`capacity` entries of three int32), each list sorted in place, keep[t] = 1 for the first entry
 *        of every (middle, largest) run, 0 for every other triangle.
 *      rx_mesh_cluster_emit: out_triangles[keep_offsets[t]] = used_offsets[cluster of each corner] for kept t, and
 *        out_vertices[used_offsets[c]] = representatives[c] for used c, with the offsets rx_mesh_scan(keep) and rx_mesh_scan(used). */
int rx_mesh_cluster_keys(const float* vertices, int64_t n_vertices, float cell, int64_t* keys, int32_t* flag, void* stream);
int rx_mesh_cluster_assign(const int64_t* keys, int64_t n_vertices, int64_t capacity, int64_t* table_keys, int32_t* table_min, int32_t* slot_of,
                           int32_t* first, int32_t* flag, void* stream);
int rx_mesh_cluster_number(int64_t n_vertices, const int32_t* slot_of, int64_t capacity, const int32_t* table_min, const int64_t* rank,
                           int64_t* cluster_of, void* stream);
int rx_mesh_cluster_count(const int64_t* cluster_of, int64_t n_vertices, int64_t n_clusters, int32_t* counts, void* stream);
int rx_mesh_cluster_fill(const int64_t* cluster_of, int64_t n_vertices, int64_t n_clusters, const int64_t* member_offsets, int32_t* cursor,
                         int64_t capacity, int32_t* members, void* stream);
int rx_mesh_cluster_mean(const float* vertices, int64_t n_vertices, int64_t n_clusters, const int64_t* member_offsets, int32_t* members,
                         int64_t capacity, float* representatives, void* stream);
int rx_mesh_cluster_nearest(const float* vertices, const int64_t* keys, int64_t n_vertices, float cell, const int64_t* cluster_of,
                            int64_t n_clusters, uint64_t* best, float* representatives, void* stream);
int rx_mesh_cluster_remap(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* cluster_of, int64_t n_clusters,
                          int32_t* counts, int32_t* used, int32_t* flag, void* stream);
int rx_mesh_cluster_unique(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* cluster_of, int64_t n_clusters,
                           const int64_t* entry_offsets, int32_t* cursor, int64_t capacity, int32_t* entries, int32_t* keep, void* stream);
int rx_mesh_cluster_emit(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* cluster_of, int64_t n_clusters,
                         const int32_t* keep, const int64_t* keep_offsets, const int32_t* used, const int64_t* used_offsets,
                         const float* representatives, int64_t vertex_capacity, float* out_vertices, int64_t triangle_capacity,
                         int64_t* out_triangles, void* stream);

/* ---- mesh orientation against a sampled vector field (host side postprocess/orient.py, whose sample_points_numpy, unit_numpy,
 *      face_cos_numpy and side_numpy are the statements).  Sizes as in the refinement group above; n_points, n_vertices and
 *      n_triangles are at least 1 (the caller handles empty meshes).  Every float32 operation is one rounding, nothing is
 *      contracted into an fma, and there is no atomic that chooses anything: two runs give the same bytes.  Every call refuses
 *      with a status and a message before anything is launched: null or misaligned pointers, sizes outside the limits, an unknown
 *      rule, channels outside 1 .. 8, `unit` with another channel count than 3, a slab that does not lie inside z_total, a
 *      min_cos outside [0, 1).  No allocation, copy or synchronisation.
 *      rx_mesh_sample: `volume` is (channels, z_depth, y, x) contiguous, of float32 (RX_MESH_SAMPLE_COPY), uint8 (_U8) or uint16
 *        (_U16, _NORMAL_U16) values, planes [z_base, z_base + z_depth) of a volume of z_total planes; `points` float32
 *        (n_points, 3) as (x, y, z) in voxel coordinates.  out[v] (float32, `channels` values) = the trilinear sample with clamped
 *        borders: per axis i = floor(p), f = p - i, corners i and i + 1 clamped; every corner decoded first (copy: unchanged;
 *        u8: v / 255; u16: v / 65535; normal_u16: (v / 65535) * 2 - 1); lerp(u, w, f) = u + f * (w - u) along x, then y, then z.
 *        unit != 0: the three values are then divided by their length sqrt(x*x + y*y + z*z), (0, 0, 0) where that is not > 0.
 *        A point whose two clamped z indices are not both inside the slab is left untouched in `out`, so successive slab launches
 *        fill one buffer.  No load leaves the slab, whatever the coordinates hold.
 *      rx_mesh_face_cos: per triangle (a, b, c): g = cross(pb - pa, pc - pa), m = (n_a + n_b) + n_c of `vectors`,
 *        cos[t] = (g.m) / sqrt((g.g) * (m.m)), each dot three products summed left to right; side[t] = 1 where cos > min_cos,
 *        -1 where cos < -min_cos, else 0 (a NaN included); keep[t] = side[t] == want (want 0: every triangle); used[v] = 1 for
 *        the corners of a kept triangle (zeroed first; a plain store of a constant).  Bit 2 of `flag`: an id outside
 *        [0, n_vertices); such a triangle is not followed, its cos is NaN and it is not kept.
 *      rx_mesh_select_mark: used[v] = 1 for the corners of the triangles with keep[t] != 0 (zeroed first); `flag` as above.
 *      The compaction of the kept triangles and the used vertices is rx_mesh_scan over `keep` and `used`, then
 *      rx_mesh_cluster_emit with cluster_of[v] = v and n_clusters = n_vertices. */
#define RX_MESH_SAMPLE_COPY 0
#define RX_MESH_SAMPLE_U8 1
#define RX_MESH_SAMPLE_U16 2
#define RX_MESH_SAMPLE_NORMAL_U16 3
#define RX_MESH_SAMPLE_MAX_CHANNELS 8
#define RX_MESH_SAMPLE_MAX_EXTENT 16777214
int rx_mesh_sample(const void* volume, int rule, int channels, int z_base, int z_depth, int z_total, int y, int x, const float* points,
                   int64_t n_points, int unit, float* out, void* stream);
int rx_mesh_face_cos(const float* vertices, const float* vectors, int64_t n_vertices, const int64_t* triangles, int64_t n_triangles,
                     float min_cos, int want, float* cos, int8_t* side, int32_t* keep, int32_t* used, int32_t* flag, void* stream);
int rx_mesh_select_mark(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* keep, int32_t* used, int32_t* flag,
                        void* stream);

/* ---- validation preview on the device: one panel of the debug GIF (host side training/visualization/preview.py, whose
 *      panel_numpy and minmax_numpy are the statements).  `src` is ONE sample's contiguous (c, z, h, w) block of `dtype` (rx_dtype),
 *      aligned to its element (a base that is not 16-byte aligned is fine).  c == 3 draws channels 0, 1, 2 into bytes 0, 1, 2 of
 *      a pixel, each scaled by its own range; any other c draws channel 0 as grey (the same byte three times).  Kept slice j is
 *      source slice j * z_step, j < z_kept = ceil(z / z_step).  Its h x w x 3 bytes go to
 *        frames + j * frame_stride + (y0 + row) * row_stride + 3 * (x0 + col)
 *      and nothing outside that rectangle is written; nothing outside the sample is read; every offset is 64-bit.
 *      Per drawn channel and kept slice, in float32 with one rounding per operation, nothing contracted into an fma, IEEE
 *      division: v = the element (`sigmoid` != 0: v = 1.0f / (1.0f + expf(-v)), the device's expf), lo = min v, hi = max v,
 *      r = hi - lo; if every v is finite, r > 1e-6f and r is finite, the byte is trunc(((v - lo) / r) * 255.0f), else the whole
 *      slice is 127 (= trunc(0.5 * 255): a flat slice, and by this library's own rule a slice that holds a NaN or an infinity).
 *      `minmax` (nullable, 4-byte aligned): float32 (c_drawn, z_kept, 2) = (lo, hi), or (NaN, NaN) for a slice that holds a NaN
 *      or an infinity.
 *      One launch draws the panel: one workgroup per kept slice reduces lo / hi / "not finite" per lane, wave (shuffles) and
 *      workgroup (LDS) -- no atomics, so nothing depends on arrival order -- then reads its slice again (from L2) and writes the
 *      bytes.  Both passes read a scalar head up to the first 16-byte boundary of the slice of channel 0, 16-byte vectors, a scalar
 *      tail.  The bytes are staged in LDS in pixel order and stored as whole dwords wherever a destination dword lies inside a
 *      panel row (row_stride and 3 * x0 need not be multiples of 4; the rest are byte stores).  No allocation, copy or
 *      synchronisation.  RX_EINVAL before anything is launched: null src or frames, non-positive c / z / h / w / z_step, an unknown
 *      dtype, a misaligned src or minmax, negative y0 or x0, row_stride < 3 * (x0 + w), frame_stride < (y0 + h) * row_stride. */
int rx_preview_panel(const void* src, int dtype, int c, int z, int h, int w, int z_step, int sigmoid, uint8_t* frames,
                     long frame_stride, long row_stride, int y0, int x0, float* minmax, void* stream);

/* ---- mesh targets on the device: triangle meshes sliced by the z-planes of a slab into normals / label / mask volumes (host side
 *      tasks/normals/mesh_targets.py, whose slice_normals_numpy and slice_labels_numpy are the statements).  The reference paints a
 *      slice serially, so a pixel keeps its last writer, i.e. the largest (triangle, pair, step, sample): rx_mesh_slice_keys
 *      scatters that tuple as an order key with an integer atomic maximum (bit-identical run to run), and the resolve calls
 *      recompute every pixel from its winning key alone.  Geometry, shared by the three calls: slices [z0, z0 + nz) of the full
 *      w x h image, of which only the window rows [y0, y0 + wh) and columns [x0, x0 + ww) are stored; endpoint and pixel tests
 *      use the full image, so a slab or window result equals the full result cropped.  `vertices` and `normals`: DEVICE fp32
 *      (n_vertices, 3); `triangles`: DEVICE int32 (n_triangles, 3).  Device data cannot be validated here: the Python wrapper
 *      refuses non-finite vertices or normals, coordinates at or beyond 2^24 and vertex indices outside [0, n_vertices); the
 *      kernels clamp every vertex index and bound every loop regardless.  No allocation, copy or synchronisation.
 *
 *      rx_mesh_slice_keys: `keys` is the ZEROED (nz, wh, ww) key buffer: uint64 `(triangle + 1) << 26 | pair << 24 | step << 4 |
 *      sample` for normals (labels == 0; `normals` and `exp_factor` are used), uint32 `triangle + 1` for labels (labels != 0).
 *      RX_EINVAL before anything is launched: null or misaligned pointers, n_vertices outside [1, 2^31), non-positive sizes, sides
 *      above 2^24, slices outside (-2^24, 2^24), a window outside the image, more triangles than the key holds (2^38 - 2, labels
 *      2^32 - 2), an exp_factor whose int(4 * 1.2 * exp_factor + 1) samples are fewer than 2 or more than 16, an image whose
 *      diagonal allows a segment of 2^20 steps or more. */
int rx_mesh_slice_keys(int labels, const float* vertices, long n_vertices, const int32_t* triangles, long n_triangles,
                       const float* normals, int w, int h, int z0, int nz, int y0, int x0, int wh, int ww, double exp_factor,
                       void* keys, void* stream);
/* out: uint16 (nz, wh, ww, 3) channels-last codes uint16((n + 1) * 32767.5), 0 where the key is 0.  viz (optional): uint8
 * (nz, wh, ww, 3), the reference's preview byte.  mask (optional): uint8 (nz, wh, ww), 255 where any channel is non-zero.  All
 * three 4-byte aligned: a workgroup stages its pixels in LDS and stores whole dwords, bytes only for the last dword of an array. */
int rx_mesh_resolve_normals(const void* keys, const float* vertices, long n_vertices, const int32_t* triangles, long n_triangles,
                            const float* normals, int w, int h, int z0, int nz, int y0, int x0, int wh, int ww, uint16_t* out,
                            uint8_t* viz, uint8_t* mask, void* stream);
/* out: uint16 [npix] = tri_labels[key - 1] & 0xffff (DEVICE int32 [n_triangles]), 0 where the key is 0; mask (optional): uint8
 * [npix], 255 where the label is non-zero.  npix = nz * wh * ww. */
int rx_mesh_resolve_labels(const void* keys, const int32_t* tri_labels, long n_triangles, long npix, uint16_t* out, uint8_t* mask,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RXUNET_H */
