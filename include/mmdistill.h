/* mmdistill.h — C ABI of libmmdistill_hip.so (MI355X / gfx950 kernels for the MM-DistillNet distillation step).
 *
 * Drop-in boundary: the reference has no FFI; its hot path is reached through Python
 * call signatures.  Each entry point below replaces the torch/torchvision operator(s) cited above it
 * (file:line relative to the reference tree).  Conventions: extern "C", raw DEVICE pointers + sizes,
 * fp32 NHWC activations ("rows" = B*H*W pixels x C channels), last argument is the hipStream_t to
 * launch on, return 0 on success / negative errno-style code on bad arguments or launch failure,
 * the caller owns every buffer including workspaces, no hidden allocation, no host synchronisation
 * (every entry point is hipGraph-capturable).
 */
#ifndef MMDISTILL_H
#define MMDISTILL_H
#include <hip/hip_runtime_api.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MMD_ACT_NONE 0
#define MMD_ACT_SWISH 1
#define MMD_ACT_SIGMOID 2

// BiFPN fast-attention fusion node: swish(sum_i w_i * operand_i), nearest-x2 upsample and SAME max-pool fused
// (src/YetAnotherEfficientDet.py:338-390).
int mmd_bifpn_fuse_fwd(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, float* out, int B, int H, int W, int C, hipStream_t stream);

// Fusion node + its depthwise 3x3 (SeparableConvBlock.depthwise_conv) in one launch; f_out (nullable) keeps the fused
// activation for the backward.
int mmd_bifpn_node_dw_fwd(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, float* f_out, float* zd, int B, int H, int W, int C, hipStream_t stream);

// Whole BiFPN node of a frozen net in one kernel: fusion + swish + depthwise 3x3 + 1x1 conv (w_pw [C, C] as stored upstream) + bias + folded
// BatchNorm (SeparableConvBlock(norm=True) after BiFPN._forward_fast_attention's weighted sum, src/YetAnotherEfficientDet.py:150-185,338-390,
// eval mode).  -22 for a width without a kernel: ask mmd_bifpn_node_fused_supported (C in {64, 112, 160, 224}: the fpn widths of D0 / D2 / D3 / D4) and keep mmd_bifpn_node_dw_fwd + mmd_pwconv_fwd.
int mmd_bifpn_node_fused_supported(int C);
int mmd_bifpn_node_fwd_fused(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, const float* w_pw, const float* bias, const float* scale, const float* shift, float* y, int B, int H, int W, int C, hipStream_t stream);

// The same node for the TRAINABLE net in train mode: z = the raw 1x1-conv output (+ bias), stats [2C] (+)= [sum z, sum z^2] (the batch
// statistics of the node's BatchNorm, src/YetAnotherEfficientDet.py:171-176), zd = the depthwise output (read by the 1x1 conv's weight
// gradient in the backward).  C as mmd_bifpn_node_fused_supported.
int mmd_bifpn_node_fwd_fused_train(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, const float* w_pw, const float* bias, float* z, float* zd, double* stats, int B, int H, int W, int C, hipStream_t stream);

// Backward of the fusion node, part 1: dx = df*swish'(x), wdot[i] += <dx, operand_i>.
int mmd_bifpn_fuse_bwd(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* df, float* dx, float* wdot, int B, int H, int W, int C, float* d0, int acc0, float* d1, int acc1, hipStream_t stream);

// Backward of w = relu(theta)/(sum+1e-4).
// Node backward in one launch: depthwise 3x3 input gradient (from an LDS tile of dzd, the gradient w.r.t. the depthwise output)
// + fusion backward (same outputs as mmd_bifpn_fuse_bwd fed with df = dwconv^T(dzd, w_dw)); dup (nullable, needs `up`): the gradient of
// the nearest-upsampled operand [B, H/2, W/2, C] (=|+=) w_up * 2x2 block sums, written here instead of by mmd_upsample2_bwd_acc;
// dw_grad (nullable): the node's depthwise weight gradient [9, C] += , from the recomputed fused activation and the dzd tile this launch
// already holds (instead of a mmd_dwconv_bwd_weight launch over a materialised f).
int mmd_bifpn_node_dw_bwd(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, const float* dzd, float* dx, float* wdot, int B, int H, int W, int C, float* d0, int acc0, float* d1, int acc1, float* dup, int acc_up, float* dw_grad, hipStream_t stream);

// Round 3: "the writer of the last contribution to a gradient computes the BatchNorm-backward sums of the total".  Same launch as
// mmd_bifpn_node_dw_bwd; for each operand gradient it writes (d0 / d1 / dup) an optional (z, mean, invstd, sums): when this launch
// completes that gradient and the operand is the output y = BN(z) of a BatchNorm (a BiFPN node / down-channel output), sums [2C] (+)=
// [sum g, sum g*xhat], xhat = (z - mean)*invstd, over the completed gradient g - what mmd_bn_bwd_reduce(act = NONE) would compute in a
// launch of its own on the backward's serial chain (autograd of the BatchNorm in SeparableConvBlock, src/YetAnotherEfficientDet.py:171-176).
int mmd_bifpn_node_dw_bwd2(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, const float* dzd, float* dx, float* wdot, int B, int H, int W, int C, float* d0, int acc0, float* d1, int acc1, float* dup, int acc_up, float* dw_grad, const float* z0, const float* mean0, const float* invstd0, double* sums0, const float* z1, const float* mean1, const float* invstd1, double* sums1, const float* zu, const float* meanu, const float* invstdu, double* sumsu, hipStream_t stream);

// + the POOLED operand's gradient out of the same launch (round 3): dpool [B, 2H, 2W, C] += w_pool * g at the arg-max element of every output
// pixel's 3x3 / stride-2 SAME window (first maximum in scan order; a winning zero-padding element swallows the gradient - torch's max-pool
// backward, src/YetAnotherEfficientNet.py:68-104), fp32 atomics on a buffer holding zeros or the earlier contributions - instead of dx + a
// mmd_maxpool_same_bwd_acc launch.  A scattered gradient has no last writer, so the BatchNorm-backward sums of a pooled tensor are kept
// linearly: (zp, meanp, invstdp, sumsp) receive the sums of this launch's share; own bit 0 / 1 / 2: the sums of d0 / d1 / dup likewise
// cover this launch's share instead of the accumulated total.
int mmd_bifpn_node_dw_bwd3(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, const float* dzd, float* dx, float* wdot, int B, int H, int W, int C, float* d0, int acc0, float* d1, int acc1, float* dup, int acc_up, float* dw_grad, const float* z0, const float* mean0, const float* invstd0, double* sums0, const float* z1, const float* mean1, const float* invstd1, double* sums1, const float* zu, const float* meanu, const float* invstdu, double* sumsu, float* dpool, const float* zp, const float* meanp, const float* invstdp, double* sumsp, int own, hipStream_t stream);

// Round 4, "lazy" BiFPN operands of the trainable net: a node's / down-channel conv's train-mode BatchNorm (no activation) is applied by its
// CONSUMERS while they load the operand, instead of by an mmd_affine_act launch behind every producer (40 launches on the student's forward
// chain; BiFPN._forward_fast_attention, src/YetAnotherEfficientDet.py:320-392).  Operand i (order in0, in1, up, pool) then holds the RAW 1x1
// output z_i; host arrays of 4 entries describe the transforms, a null entry = plain tensor.
//   forward:  y_i = z_i * scale_i + shift_i with (scale, shift) derived in-kernel from the live batch sums op_stats4[i] [2C] (double),
//             op_gamma4[i], op_beta4[i], op_count4[i] (long long rows) - bit-identical to mmd_bn_finalize's coefficients.  C <= 160.
//   backward: op_scale4[i] / op_shift4[i] = the finalized coefficients; applied wherever the launch needs the operand's value (fused
//             activation, fusion-weight dot products, pool arg-max); gradients / BatchNorm sums are w.r.t. the BatchNorm output as before.
int mmd_bifpn_node_fwd_fused_train_lz(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, const float* w_pw, const float* bias, float* z, float* zd, double* stats, int B, int H, int W, int C, const void* op_stats4, const void* op_gamma4, const void* op_beta4, const void* op_count4, hipStream_t stream);
int mmd_bifpn_node_dw_bwd3_lz(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, const float* dzd, float* dx, float* wdot, int B, int H, int W, int C, float* d0, int acc0, float* d1, int acc1, float* dup, int acc_up, float* dw_grad, const float* z0, const float* mean0, const float* invstd0, double* sums0, const float* z1, const float* mean1, const float* invstd1, double* sums1, const float* zu, const float* meanu, const float* invstdu, double* sumsu, float* dpool, const float* zp, const float* meanp, const float* invstdp, double* sumsp, int own, const void* op_scale4, const void* op_shift4, hipStream_t stream);
// Whole-node BiFPN backward (round 4): mmd_bifpn_node_dw_bwd3_lz with the node's 1x1 conv's input gradient inside the launch (replaces
// mmd_pwconv_bwd_data_bn in front of it): dzd = BnBwd(g, z) . w_pw is computed per tile - g the gradient w.r.t. the node's BatchNorm output,
// z its raw 1x1 output [B*H*W, C], (bn_scale, bn_mean, bn_invstd) of that BatchNorm, bn_sums = [sum g, sum g xhat] over `count` rows,
// w_pw_t [C in, C out] = the conv's weight TRANSPOSED (the operand mmd_pwconv_bwd_data takes); dz_out receives the evaluated BatchNorm backward (the weight-gradient GEMM's operand), dgamma / dbeta (+)= the sums.
// C % 16 == 0, C <= 224; operand sets (in, up), (in, td, pool), (in, pool).  SeparableConvBlock backward, src/YetAnotherEfficientDet.py:150-185.
int mmd_bifpn_node_bwd_full(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, float* wdot, int B, int H, int W, int C, float* d0, int acc0, float* d1, int acc1, float* dup, int acc_up, float* dw_grad, const float* z0, const float* mean0, const float* invstd0, double* sums0, const float* z1, const float* mean1, const float* invstd1, double* sums1, const float* zu, const float* meanu, const float* invstdu, double* sumsu, float* dpool, const float* zp, const float* meanp, const float* invstdp, double* sumsp, int own, const void* op_scale4, const void* op_shift4, const float* g, const float* z, const float* bn_scale, const float* bn_mean, const float* bn_invstd, const double* bn_sums, long long count, const float* w_pw_t, float* dz_out, float* dgamma, float* dbeta, hipStream_t stream);
// mmd_bifpn_node_bwd_full picks its block shape from the launch size: with fewer than 128 64-channel blocks (the 4x4 .. 16x16 levels at B = 8)
// it runs 16-channel blocks - same results up to the order of the per-channel sums - and on launches of >= 128 blocks a pooled operand's
// scattered gradient is collected in an LDS tile of the fine map.  EXCLUSIVITY (mmd_bifpn_node_bwd_full, mmd_bifpn_node_dw_bwd3[_lz]): with the
// LDS tile the interior of `dpool` is read at block start and plainly stored at block end, so no other launch may write `dpool` while this
// one runs (every contributor to a scattered gradient on ONE stream; the engine asserts it).
// _form: the same launch with both choices made by the caller (tests, timing; per call - no process-wide state): small_below = launches with
// fewer 64-channel blocks than this take the 16-channel form (0 never, 1 << 30 always, < 0 default); pool_lds = 1 / 0 the LDS tile on / off, < 0 default.
int mmd_bifpn_node_bwd_full_form(const float* in0, const float* in1, const float* up, const float* pool, const float* theta, const float* w_dw, float* wdot, int B, int H, int W, int C, float* d0, int acc0, float* d1, int acc1, float* dup, int acc_up, float* dw_grad, const float* z0, const float* mean0, const float* invstd0, double* sums0, const float* z1, const float* mean1, const float* invstd1, double* sums1, const float* zu, const float* meanu, const float* invstdu, double* sumsu, float* dpool, const float* zp, const float* meanp, const float* invstdp, double* sumsp, int own, const void* op_scale4, const void* op_shift4, const float* g, const float* z, const float* bn_scale, const float* bn_mean, const float* bn_invstd, const double* bn_sums, long long count, const float* w_pw_t, float* dz_out, float* dgamma, float* dbeta, int small_below, int pool_lds, hipStream_t stream);

int mmd_bifpn_theta_bwd(const float* theta, const float* wdot, float* dtheta, int n, hipStream_t stream);

// d theta of every fusion node of a net in ONE launch: desc [nodes][2] = (offset of the node's theta in theta_base / dtheta_base, its
// operand count); wdot_all [nodes][4] = the dot products the node backward launches accumulated.
int mmd_bifpn_theta_bwd_batched(const float* theta_base, float* dtheta_base, const float* wdot_all, const long long* desc, int nodes, hipStream_t stream);

// dst (+)= w_idx(theta) * src (same-resolution operand gradient).
int mmd_scale_acc(const float* src, float* dst, const float* theta, int ntheta, int widx, int accumulate, long long numel, hipStream_t stream);

// Backward of nn.Upsample(scale_factor=2, nearest) (src/YetAnotherEfficientDet.py:223-226).
int mmd_upsample2_bwd_acc(const float* dx, float* dst, const float* theta, int ntheta, int widx, int accumulate, int B, int H, int W, int C, hipStream_t stream);

// MaxPool2dStaticSamePadding(3,2) forward: zero padding takes part in the max (src/YetAnotherEfficientNet.py:68-104).
int mmd_maxpool_same_fwd(const float* src, float* out, int B, int PH, int PW, int C, hipStream_t stream);

// Backward of MaxPool2dStaticSamePadding(3,2) in gather form (first maximum in scan order wins).
int mmd_maxpool_same_bwd_acc(const float* src, const float* dout, float* dst, const float* theta, int ntheta, int widx, int accumulate, int B, int PH, int PW, int C, hipStream_t stream);

// + (z, mean, invstd, sums): the BatchNorm-backward sums of the completed gradient dst when this launch is its last contribution and
// src = BN(z) (see mmd_bifpn_node_dw_bwd2).  C <= 512.
int mmd_maxpool_bwd_sums_ok(int B, int PH, int PW, int C);

int mmd_maxpool_same_bwd_acc2(const float* src, const float* dout, float* dst, const float* theta, int ntheta, int widx, int accumulate, int B, int PH, int PW, int C, const float* z, const float* mean, const float* invstd, double* sums, hipStream_t stream);

// Depthwise kxk TF-SAME conv, NHWC, fused producer BN+swish prologue, stats / eval-BN+swish / SE-pool epilogue.
// pool [B, C] (nullable, frozen nets): the squeeze-excite average pool (src/YetAnotherEfficientNet.py:470) accumulated as 64-bit fixed-point
// integers, pool[b, c] += round(2^36 * mean_hw y): integer atomics commute exactly, so a frozen net's outputs are bit-identical from run to
// run (zero the array first; mmd_se_fc_fwd_q reads it back).
// stats_ws/ws_slots (nullable/0): zeroed workspace of ws_slots*2C doubles; launches that would send > 128 blocks to one
// BatchNorm-sum address spread their f64 atomics over the slots and fold them into `stats` (workspace left zero).
// Replaces Conv2dStaticSamePadding(groups=C) (src/YetAnotherEfficientNet.py:433-435, src/YetAnotherEfficientDet.py:169-170) incl. F.pad (:51-65).
int mmd_dwconv_fwd(const float* x, const float* w, float* y, int B, int H, int W, int C, int k, int stride, const float* in_scale, const float* in_shift, int in_act, const double* in_stats, const float* in_gamma, const float* in_beta, long long in_count, const float* out_scale, const float* out_shift, int out_act, double* stats, long long* pool, double* stats_ws, int ws_slots, hipStream_t stream);

// Frozen-net MBConv front half in one kernel: expand 1x1 conv + folded BN0 + swish -> depthwise kxk/stride (TF-SAME) + folded BN1 + swish
// + squeeze-excite average pool (pool[B,Cmid] +=, nullable; Q36 fixed-point integers as for mmd_dwconv_fwd).  The 6x expanded tensor stays in LDS (MFMA -> LDS -> depthwise).
// w_expand [Cmid, Cin] as stored by the reference, w_dw tap-major [k*k, Cmid].  -22 for a geometry without a kernel: ask
// mmd_mbconv_expand_dw_supported (Cin in {16,24,32,40,48,56}, Cmid % 48 == 0, k in {3,5}, stride in {1,2}) and keep mmd_pwconv_fwd +
// mmd_dwconv_fwd otherwise.  Replaces MBConvBlock.forward's `_expand_conv`/`_bn0`/swish/`_depthwise_conv`/`_bn1`/swish/avg-pool
// in eval mode (src/YetAnotherEfficientNet.py:450-470).
int mmd_mbconv_expand_dw_supported(int Cin, int Cmid, int k, int stride);
int mmd_mbconv_expand_dw_fwd(const float* x, const float* w_expand, const float* scale0, const float* shift0, const float* w_dw, const float* scale1, const float* shift1, float* y, long long* pool, int B, int H, int W, int Cin, int Cmid, int k, int stride, hipStream_t stream);

// Input gradient of the depthwise conv.  With bn_sums (stride 1 only) the launch also accumulates the sums of the BatchNorm(+swish)
// backward that consumes dx: bn_sums[c] += sum dx*swish'(u), bn_sums[C+c] += sum dx*swish'(u)*xhat, u = bn_z*bn_scale+bn_shift,
// xhat = (bn_z-bn_mean)*bn_invstd (bn_z = that BN's forward input, same shape as dx); stats_ws/ws_slots as in mmd_dwconv_fwd.
// dw_grad (nullable; needs bn_sums): the conv's weight gradient [k*k, C] += out of the same launch, with the forward input taken as
// swish(bn_z*bn_scale+bn_shift) - what mmd_dwconv_bwd_weight computes from x = bn_z with that producer transform.
int mmd_dwconv_bwd_data(const float* dy, const float* w, float* dx, int B, int H, int W, int C, int k, int stride, const float* bn_z, const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd, double* bn_sums, double* stats_ws, int ws_slots, float* dw_grad, hipStream_t stream);

// Round 3: the same launch for an MBConv block's stride-1 depthwise conv (C >= 64) with the BatchNorm-1 (+swish) backward - including the
// squeeze-excite terms: g' = (g1 * q_gate[img,c] + q_add[img,c]) * swish'(z1*scale+shift) - evaluated on the dY operand while its tile is
// staged, instead of by mmd_bn_bwd_apply(mul_bc = gate, add_bc = dpooled) writing dz1 to HBM first; q_dgamma / q_dbeta (+)= from q_sums.
// bn_* / dw_grad: as mmd_dwconv_bwd_data (all required).  Autograd of src/YetAnotherEfficientNet.py:462-474.
int mmd_dwconv_bwd_data_bn1(const float* g1, const float* z1, const float* w, float* dx, int B, int H, int W, int C, int k, const float* q_scale, const float* q_shift, const float* q_mean, const float* q_invstd, const double* q_sums, long long q_count, const float* q_gate, const float* q_add, float* q_dgamma, float* q_dbeta, const float* bn_z, const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd, double* bn_sums, double* stats_ws, int ws_slots, float* dw_grad, hipStream_t stream);

// Weight gradient of the depthwise conv, tap-major dw[k*k, C] (+=).
int mmd_dwconv_bwd_weight(const float* x, const float* dy, float* dw, int B, int H, int W, int C, int k, int stride, const float* in_scale, const float* in_shift, int in_act, hipStream_t stream);

// Train-mode BatchNorm2d: batch statistics -> (scale, shift, mean, invstd) + running-stat update (momentum 0.01, eps 1e-3).
// Replaces nn.BatchNorm2d forward in training (call sites SURVEY 2.1).
int mmd_bn_finalize(const double* stats, long long count, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift, float* mean_out, float* invstd_out, int C, hipStream_t stream);

// All train-mode BN layers of a net finalized in one launch (running stats + saved mean/invstd for the backward);
// forward consumers derive (scale, shift) on the fly from the raw sums (in_stats/in_gamma/in_beta/in_count arguments).
int mmd_bn_finalize_all(const double* stats_flat, const float* count, const int* layer_off, const int* layer_C, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift, float* mean_out, float* invstd_out, int total, long long* num_batches_tracked, int n_layers, hipStream_t stream);

// Eval-mode BatchNorm2d folded to per-channel (scale, shift).
int mmd_bn_fold(const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps, float* scale, float* shift, int C, hipStream_t stream);

// y = act(z*scale+shift) * rowscale[image] + res : BN apply, drop-connect scaling and identity skip
// (src/YetAnotherEfficientNet.py:173-182,479-485).
int mmd_affine_act(const float* z, const float* scale, const float* shift, const double* in_stats, const float* in_gamma, const float* in_beta, long long in_count, int act, const float* rowscale, int rows_per_image, const float* res, float* y, int M, int C, hipStream_t stream);

// out[b,c] += s * sum_hw (g? g*a : a), a = act(z*scale+shift): SE global average pool (src/YetAnotherEfficientNet.py:470) and d(gate).
int mmd_chan_pool(const float* z, const float* scale, const float* shift, const double* in_stats, const float* in_gamma, const float* in_beta, long long in_count, int act, const float* g, float* out, float out_scale, int B, int rows_per_image, int C, hipStream_t stream);

// Squeeze-excite FCs: gate = sigmoid(We*swish(Wr*pooled+br)+be) (src/YetAnotherEfficientNet.py:471-474).
int mmd_se_fc_fwd(const float* pooled, const float* wr, const float* br, const float* we, const float* be, float* hpre, float* gate, int B, int C, int S, hipStream_t stream);
// The frozen nets' form: pooled_q [B, C] holds the Q36 fixed-point pool sums of mmd_dwconv_fwd / mmd_mbconv_expand_dw_fwd (value = q / 2^36).
int mmd_se_fc_fwd_q(const long long* pooled_q, const float* wr, const float* br, const float* we, const float* be, float* hpre, float* gate, int B, int C, int S, hipStream_t stream);

// Round 4, grouped frozen nets: several frozen nets of ONE architecture (the three teachers) evaluated as one batch of n_groups x
// images_per_group images - a launch covers the same layer of every net and each workgroup picks its net's parameters by the image it
// works on: group g = image / images_per_group reads its weights g * w_stride floats and its folded BatchNorm coefficients g * bn_stride
// floats behind the pointers passed in (the nets' flat parameter / coefficient buffers are laid out alike, a constant stride apart).
// mmd_set_group applies to the launches the CALLING HOST THREAD issues after it until cleared with n_groups <= 1 (thread-local descriptor:
// other threads' launches never see it); clearing returns -22 when no launch issued in between read the group, i.e. an entry point
// without a group mode ran under it (with the first net's parameters for every image).  Honoured by the frozen
// forward entry points mmd_pwconv_fwd / mmd_pwconv_fwd_pyr (LDS-tiled kernels; every group's rows are whole 128-row tiles),
// mmd_dwconv_fwd, mmd_dwconv3_pyr (forward), mmd_mbconv_expand_dw_fwd, mmd_se_fc_fwd(_q), mmd_bifpn_node_fwd_fused and mmd_bifpn_node_dw_fwd; they return -22
// for a launch form the mode does not cover (statistics, live BatchNorm prologues, bf16 storage).
int mmd_set_group(int n_groups, int images_per_group, long long w_stride, long long bn_stride);

// One pass over (z1, g1): out5[5][B][C] += (sum g1*swish(u), sum g1*swish'(u), sum g1*swish'(u)*xhat, sum swish'(u), sum swish'(u)*xhat)
// per (image, channel): d(gate) for the SE backward plus the partials of the BatchNorm-1 backward sums (autograd of
// src/YetAnotherEfficientNet.py:466-476), so the expanded tensor is not read again by a BN reduce pass.
int mmd_chan_pool_bwd(const float* z, const float* scale, const float* shift, const float* mean, const float* invstd, const float* g1, float* out5, int B, int rows_per_image, int C, hipStream_t stream);

// Backward of the squeeze-excite FCs (weight grads +=, dpooled scaled by dpool_scale = 1/HW).  With pool5 (from
// mmd_chan_pool_bwd; dgate = pool5[0]) it also finishes the BN-1 sums: bn_sums[c] += sum_b gate*pool5[1] + dpooled*pool5[3], [C+c] likewise with [2],[4].
int mmd_se_fc_bwd(const float* dgate, const float* gate, const float* hpre, const float* pooled, const float* wr, const float* we, float* dpe_ws, float* dpr_ws, float* dh_zeroed, float* dpooled, float dpool_scale, float* dwr, float* dbr, float* dwe, float* dbe, int B, int C, int S, const float* pool5, double* bn_sums, hipStream_t stream);

// Weight/bias gradients of the SE FCs alone (mmd_se_fc_bwd with dwr == NULL skips them): dpe/dpr are mmd_se_fc_bwd's workspaces.
int mmd_se_fc_wgrad(const float* dpe, const float* dpr, const float* hpre, const float* pooled, float* dwr, float* dbr, float* dwe, float* dbe, int B, int C, int S, hipStream_t stream);

// mmd_se_fc_bwd's two data-gradient kernels as ONE launch (dh is not materialised; C <= 3072): dpe_ws [B,C], dpr_ws [B,S], dpooled [B,C],
// and with pool5 / bn_sums the BatchNorm-1 backward sums, exactly as mmd_se_fc_bwd(dwr = NULL) (src/YetAnotherEfficientNet.py:469-474).
int mmd_se_fc_bwd_fused(const float* dgate, const float* gate, const float* hpre, const float* wr, const float* we, float* dpe_ws, float* dpr_ws, float* dpooled, float dpool_scale, int B, int C, int S, const float* pool5, double* bn_sums, hipStream_t stream);

// mmd_se_fc_wgrad for every squeeze-excite block of a backward segment in one launch.  desc: device array of n records of ten 8-byte fields
// {dpe, dpr, hpre, pooled, dwr, dbr, dwe, dbe (pointers), C, S (64-bit ints)}; max_cs = the largest C*S among them.
int mmd_se_fc_wgrad_batched(const void* desc, int n, int max_cs, int B, hipStream_t stream);

// BN(+swish) backward pass 1: g = (g_in*mul+add)*act'(y); per-channel sum(g), sum(g*xhat). g_out may be NULL (g not stored).
int mmd_bn_bwd_reduce(const float* g_in, const float* z, const float* scale, const float* shift, const float* mean, const float* invstd, int act, const float* mul_bc, const float* mul_b, const float* add_bc, int rows_per_image, float* g_out, double* sums, int M, int C, double* stats_ws, int ws_slots, hipStream_t stream);

// BN backward pass 2: dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); dgamma/dbeta +=. With act/mul/add given, `g` is pass 1's g_in and g is recomputed.
int mmd_bn_bwd_apply(const float* g, const float* z, const float* mean, const float* invstd, const float* gamma, const double* sums, long long count, float* dz, float* dgamma, float* dbeta, int M, int C, const float* scale, const float* shift, int act, const float* mul_bc, const float* mul_b, const float* add_bc, int rows_per_image, hipStream_t stream);

// out[c] += sum_rows a[row,c] (bias gradients).
int mmd_colsum(const float* a, float* out, int M, int C, hipStream_t stream);

// Stem 3x3/s2 TF-SAME conv lowered to rows [B*OH*OW, Kp] (src/YetAnotherEfficientNet.py:519,603); the GEMM is mmd_pwconv_fwd.
int mmd_stem_im2col(const float* x, float* col, int B, int Cin, int H, int W, int Kp, hipStream_t stream);
// Weight gradient of the stem conv without the im2col matrix (round 4; csrc/stem_wgrad.hip): dw [Cout, Kp] (+)= sum over the output pixels of
// dz[(b, oh, ow)][co] * x[b][ci][2 oh + i - pad_t][2 ow + j - pad_l] at column ci*9 + i*3 + j - autograd of Conv2dStaticSamePadding(Cin, Cout, 3, stride=2)
// (src/YetAnotherEfficientNet.py:519-523, 597-604; padding :27-65).  x [B, Cin, H, W] NCHW, dz [B*OH*OW, Cout] rows.  ws: mmd_stem_wgrad_ws_floats(Cout)
// floats of scratch (per-block partials, folded in a fixed order).  _supported -> 1 for Cin <= 8, Kp <= 80, Cout <= 48, ceil(W/2) % 64 == 0.
int mmd_stem_conv_bwd_weight_supported(int Cin, int H, int W, int Kp, int Cout);
int mmd_stem_wgrad_ws_floats(int Cout);
int mmd_stem_conv_bwd_weight(const float* x, const float* dz, float* dw, float* ws, int B, int Cin, int H, int W, int Kp, int Cout, hipStream_t stream);
// ... with the stem BatchNorm(+swish) backward in the prologue: dz = BnBwd(g, z) is evaluated while the tile is staged (never a tensor), dgamma /
// dbeta (+)= sums - autograd of `_bn0` + swish behind the stem conv (src/YetAnotherEfficientNet.py:523-524); arguments as mmd_pwconv_bwd_data_bn.
int mmd_stem_conv_bwd_weight_bn(const float* x, const float* g, const float* z, float* dw, float* ws, int B, int Cin, int H, int W, int Kp, int Cout, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, float* dgamma, float* dbeta, hipStream_t stream);

// dlogit = dprob * p * (1-p) (classifier sigmoid, src/YetAnotherEfficientDet.py:529).
int mmd_sigmoid_bwd(const float* dprob, const float* prob, float* dlogit, long long n, hipStream_t stream);

// Copy one pyramid level out of a concatenated [B, A_total, C] head tensor.
int mmd_slice_rows(const float* src, float* dst, int B, int rows, int N, long long batch_stride, long long offset, hipStream_t stream);
// ... every level in one launch, into the level-major pyramid matrix the head backward works on (the split the reference's per-level loop
// implies, src/YetAnotherEfficientDet.py:470-480 / 520-530 run backwards): dst[row0[l] + b * HW_l + r, :] = src[b * batch_stride + offsets[l] + r * N ...];
// pyr_desc as for mmd_dwconv3_pyr, offsets = one host value per level.
int mmd_slice_rows_pyr(const float* src, float* dst, const int* pyr_desc, int N, long long batch_stride, const long long* offsets, hipStream_t stream);

// MTALoss.at without the normalisation: a[b,j] = mean_c f^p (src/loss/MTALoss.py:76-77).
int mmd_mta_attention(const float* f, float* a, int rows, int C, float p, hipStream_t stream);

// Per-level MTA loss (pairwise or list mode) and d/d(student attention) (src/loss/MTALoss.py:36-74).
int mmd_mta_kl(const float* a_s, const float* a_t0, const float* a_t1, const float* a_t2, int nteachers, int B, int HW, float T, float* loss, float* da_s, float gscale, int accumulate, hipStream_t stream);

// df (+)= da * p * f^(p-1) / C.
// Every (pyramid level, teacher) pair of one step in a single launch (host arrays of device pointers: a_s[nlev], a_t[nteachers*nlev]
// teacher-major, da_s[nlev] nullable, HW[nlev]).  list_mode = 0: pairwise MTALoss calls (src/optimization/train_methods.py:341-346),
// loss[t*nlev + l], da_s[l] accumulated over teachers with atomics (zero on entry when nteachers > 1); list_mode = 1: the list form
// (src/loss/MTALoss.py:36-52), loss[l].
int mmd_mta_kl_multi(const float* const* a_s, const float* const* a_t, float* const* da_s, const int* HW, int nlev, int nteachers, int list_mode, int B, float T, float* loss, float gscale, hipStream_t stream);

int mmd_mta_attention_bwd(const float* f, const float* da, float* df, int rows, int C, float p, int accumulate, hipStream_t stream);

// AttentionLoss (src/loss/AttentionLoss.py:17-41, p = 2), every (pyramid level, teacher) pair of one step: the pairwise calls of
// ModelWithNMSLoss(.Augmented).forward (src/optimization/train_methods.py:351-358) on the raw maps of mmd_mta_attention(p = 2).
// Host arrays of device pointers as for mmd_mta_kl_multi: a_s[nlev], a_t[nteachers*nlev] teacher-major, da_s[nlev] nullable, HW[nlev].
// loss[t*nlev + l] = mean_{b,j} (ahat_s - ahat_t)^2 (stored: no zeroing needed); da_s[l] = gscale * d(sum of the losses)/d a_s, stored
// for every element of the B x HW[l] map.  ws: nteachers*nlev*B floats.  Bitwise reproducible (no float atomics; two launches).
int mmd_at_loss_multi(const float* const* a_s, const float* const* a_t, float* const* da_s, const int* HW, int nlev, int nteachers, int B, float* loss, float gscale, float* ws, hipStream_t stream);

// YetAnotherFocalLoss forward + gradients (src/loss/YetAnotherFocalLoss.py:27-190).
// boxes [B, maxg, 5] (x1,y1,x2,y2,label), nbox [B]: image b has min(nbox[b], maxg) boxes (a larger count is clamped, not an error); the
// rows at and behind that count are never read.  An anchor's box is its FIRST maximum of the IoU (duplicates: the lower index wins).
// Workspaces assign_ws int[B*A], npos_ws int[B], acc_ws double[2B] need no zeroing: all three are written before they are read.
// loss_out [2] (regression, classification), dcls / dreg (nullable: loss only) are stored for every element.  any_boxes (nullable) is
// sticky: set to 1 when the batch has a box, never cleared - the caller zeroes it once.
int mmd_focal_loss(const float* cls, const float* reg, const float* anchors, const float* boxes, const int* nbox, int maxg, int B, int A, int NC, int* assign_ws, int* npos_ws, double* acc_ws, float* loss_out, float* dcls, float* dreg, float grad_scale, int to_logit, int* any_boxes, hipStream_t stream);

// mmd_focal_loss with a selectable box regression criterion (an extension: the reference has smooth-L1 only).  Same launches, arguments,
// workspaces (need no zeroing), clamped box counts and sticky any_boxes as mmd_focal_loss; assignment, classification loss, dcls and the
// empty-batch / empty-image rules are unchanged in every mode.  box_mode: 0 = smooth-L1, identical to mmd_focal_loss (box_weight must
// be 1); 1 = GIoU (Rezatofighi et al. 2019); 2 = DIoU, 3 = CIoU (Zheng et al. 2020).  Another mode, a box_weight that is not finite or
// not > 0, or box_weight != 1 with mode 0 -> MMD_EINVAL, nothing is launched.
// Modes 1-3, per positive anchor (y1, x1, y2, x2) with size ah, aw and centre acy, acx, in fp32:
//   prediction (BBoxTransform's decode, src/YetAnotherEfficientDet.py:26-45): pcy = r0*ah + acy, pcx = r1*aw + acx,
//     ph = exp(min(r2, M))*ah, pw = exp(min(r3, M))*aw, M = log(1000/16); the gradient w.r.t. r2 / r3 is 0 where the clamp is active;
//   target: the raw box's centre (gcx, gcy), gw = max(x2 - x1, 1), gh = max(y2 - y1, 1) (the clamp of the smooth-L1 targets);
//   on the corner forms of both: I = product of the two intersection extents clamped at 0, U = pw*ph + gw*gh - I, IoU = I / (U + 1e-7),
//     cw, ch = extents of the smallest enclosing box;
//   GIoU: L = 1 - IoU + (cw*ch - U) / (cw*ch + 1e-7)
//   DIoU: L = 1 - IoU + ((pcx - gcx)^2 + (pcy - gcy)^2) / (cw^2 + ch^2 + 1e-7)
//   CIoU: DIoU's L + alpha*v, v = (4/pi^2) * (atan(gw/gh) - atan(pw/ph))^2, alpha = v / (1 - IoU + v + 1e-7), a constant in the gradient.
// Image b contributes box_weight * sum_pos L / npos[b] (0 without boxes or without positive anchors); loss_out[0] is the mean over the
// B images.  dreg = grad_scale * d loss_out[0] / d reg, analytic through the decode (exp, the min / max selections, atan), stored for
// every element: zeros for negative, ignored and out-of-range anchors.  A batch without boxes: zero losses and gradients, any_boxes
// untouched.
int mmd_focal_loss_box(const float* cls, const float* reg, const float* anchors, const float* boxes, const int* nbox, int maxg, int B, int A, int NC, int* assign_ws, int* npos_ws, double* acc_ws, float* loss_out, float* dcls, float* dreg, float grad_scale, int to_logit, int* any_boxes, int box_mode, float box_weight, hipStream_t stream);

// torch.optim.Adam step on a flat segment (src/optimization/train_methods.py:825-833, traditional.py:190).
int mmd_adam_step(float* p, const float* g, float* m, float* v, float* state, const float* hyper, const int* active, float grad_scale, long long n, hipStream_t stream);

// Adam over the whole flat buffer with the head (regressor/classifier) ranges skipped until they first receive a gradient.
int mmd_adam_step_gated(float* p, const float* g, float* m, float* v, float* state_main, float* state_head, const float* hyper, const int* head_active, long long b0, long long e0, long long b1, long long e1, long long b2, long long e2, float grad_scale, long long n, hipStream_t stream);

// The reference's other optimizers on the same flat, head-gated pass (cfg `optimizer` = SGD | Adam | AdamW,
// src/optimization/train_methods.py:808-836): mode 0 Adam, 1 AdamW, 2 SGD(momentum, weight_decay; m = momentum buffer).
// hyper6: device floats [lr, beta1, beta2, eps, weight_decay, momentum].
int mmd_opt_step_gated(int mode, float* p, const float* g, float* m, float* v, float* state_main, float* state_head, const float* hyper6, const int* head_active, long long b0, long long e0, long long b1, long long e1, long long b2, long long e2, float grad_scale, long long n, hipStream_t stream);

// hipMemsetAsync wrapper (graph-capturable zeroing of stats / gradient buffers).
int mmd_memset_async(void* p, int value, long long bytes, hipStream_t stream);

// Drop-connect scales of one step, drawn on the device (drop_connect, src/YetAnotherEfficientNet.py:173-182): out [n_skip, batch] =
// floor(keep[s] + U[0,1)) / keep[s], U from Philox4x32-10 keyed by `seed` with counter (state[0] = draws so far, element / 4).  state [2]
// (device): state[0] is advanced by the launch, state[1] != 0 = the caller injected out[] itself and the launch leaves it alone.
// Capturable: the replay loop of a captured step then issues no RNG / elementwise launches of its own.
int mmd_drop_scale(float* out, const float* keep, int n_skip, int batch, unsigned long long seed, unsigned long long* state, hipStream_t stream);

// Exponential moving average of the student's weights, one update: ema = fmaf(1 - d, p - ema, ema) per element over up to three
// (live, ema) fp32 segment pairs of n0 / n1 / n2 floats (the flat parameter buffer, the BatchNorm running means, the running variances)
// in ONE launch.  ema_state [2] (device floats, zeroed by the caller when an average starts): ema_state[0] = n, the updates done before
// this one, advanced to n + 1 by the call (exact up to 2^24); ema_state[1] = the d this update used: `decay` with warmup = 0,
// min(decay, (1 + n) / (10 + n)) with warmup != 0.  No host read: capturable, and a replay advances the counter like a call.
// The live buffers are only read; any length is allowed (float4 body, scalar tail), nothing at or behind ema[n] is written.
// A zero length or a null (live, ema) pair is an empty segment.  Every non-null segment pointer must be 16-byte aligned; a misaligned
// pointer, one null pointer of a pair with a positive length, a negative length, a null ema_state or a decay outside (0, 1)
// -> MMD_EINVAL, nothing is launched.
int mmd_ema_update(const float* p0, float* ema0, long long n0, const float* p1, float* ema1, long long n1, const float* p2, float* ema2, long long n2, float* ema_state, float decay, int warmup, hipStream_t stream);

// clip_grad_norm_ on the flat gradient buffer (src/optimization/traditional.py:184-188).
int mmd_clip_grad_norm(float* g, long long n, float max_norm, double* sumsq_ws, hipStream_t stream);

// Box decode + clip + conf threshold + class filter, ordered compaction
// (src/YetAnotherEfficientDet.py:574-602, src/utils/utils.py:123-204).
// over_scores [B, cap]: scores of the over-threshold anchors, cand [B, cap, 6]: (x1,y1,x2,y2,score,class) of those whose class is in
// valid_class_mask, both in anchor order; n_over / n_keep [B] their counts.  Rows at and behind a count are left as they were.
// Capacity: more than `cap` valid candidates in an image -> *overflow = 1, n_keep = cap, rows [0, cap) are the first cap candidates in
// anchor order.  More than `cap` over-threshold anchors alone is NOT an overflow (only over_scores[i < n_keep] is ever indexed):
// n_over = cap, over_scores holds the first cap.  Nothing is written at or behind row `cap`.
// Workspaces score_ws float[B*A], clsid_ws / flags_ws uchar[B*A] need no zeroing (every entry is written before it is read), nor do
// the outputs.  `overflow` is sticky (set, never cleared): the caller zeroes it.
int mmd_decode_filter(const float* cls, const float* reg, const float* anchors, int B, int A, int NC, float conf_threshold, unsigned long long valid_class_mask, float image_size, float* score_ws, unsigned char* clsid_ws, unsigned char* flags_ws, float* over_scores, float* cand, int* n_over, int* n_keep, int* overflow, int cap, hipStream_t stream);

// Per-teacher batched_nms + int truncation + label remap (src/utils/utils.py:205-231,285-323).
// cand / out: [B, cap, 6] rows; mask_ws: B*1024*16 words; big_ws (nullable when cap <= 1024): B * mmd_nms_ws_floats(cap) floats.
// The reference runs torchvision's NMS over EVERY over-threshold anchor (src/utils/utils.py:179-205, no cap): lists longer than
// 1024 rows take a chunked (1024 rows at a time, exact greedy) path through big_ws.
// Order: score descending, equal scores by ascending row index.  out row = (int(max(x1,0)), int(max(y1,0)), int(min(x2,S)), int(min(y2,S)),
// over_scores[row index], label_map[class]); rows of cand / over_scores at and behind n_keep[b] (clamped to cap) are never read, rows
// of out at and behind out_cnt[b] are left as they were.
// Capacity: an image with more than 1024 rows and big_ws == NULL -> *overflow = 1 and the result is the NMS of its FIRST 1024 rows in
// source order (the other rows do not take part, not even in the class offset).
// mask_ws and big_ws need no zeroing (they may hold anything, e.g. the previous step's bytes); `overflow` is sticky: the caller zeroes it.
int mmd_nms_teacher(const float* cand, const int* n_keep, const float* over_scores, const int* label_map, float nms_threshold, int inclusive, float image_size, int B, float* out, int* out_cnt, unsigned long long* mask_ws, int* overflow, int cap, float* big_ws, hipStream_t stream);

// Cross-teacher concat + nms(0.5) + drop score (src/optimization/train_methods.py:361-411).
// merge01 != 0: image 1 also takes image 0's rows, in front of its own, when both have rows (augment=True, :379-387); ignored for B = 1.
// Sources are [B, cap, 6] rows (x1,y1,x2,y2,score,label) with counts c*[B]; a count above cap is clamped to cap, rows at and behind a
// count are never read.  Class-agnostic; order: score descending, equal scores by source order, then row index (the earlier teacher wins).
// boxes [B, maxg, 5] (x1,y1,x2,y2,label) in keep order, nbox [B]; rows at and behind nbox[b] are left as they were.
// Capacity: more than maxg kept rows -> *overflow = 1, nbox = maxg, rows [0, maxg) are the first maxg kept rows.  A concatenation of
// more than 1024 rows with big_ws == NULL -> *overflow = 1 and the NMS runs over its first 1024 rows in concatenation order.
// mask_ws and big_ws need no zeroing; `overflow` is sticky: the caller zeroes it.  nteachers outside 1..3, a null source among the first
// nteachers, maxg <= 0 or cap <= 0 -> MMD_EINVAL, nothing is launched.
int mmd_nms_merge(const float* t0, const int* c0, const float* t1, const int* c1, const float* t2, const int* c2, int nteachers, float iou_threshold, int inclusive, int B, float* boxes, int* nbox, int maxg, unsigned long long* mask_ws, int* overflow, int merge01, int cap, float* big_ws, hipStream_t stream);

// The same merge over 1..4 sources (host arrays of device pointers, teacher order); the 4th source is the "augmentation" pass of
// ModelWithNMSKDListLossAugmented (src/optimization/train_methods.py:73-110).  big_ws: B * mmd_nms_ws_floats(nsrc * cap * (merge01 ? 2 : 1)).
// Same outputs, overflow conditions and workspace rules as mmd_nms_merge (same bits for nsrc <= 3); nsrc outside 1..4 or a null entry
// in srcs / cnts -> MMD_EINVAL, nothing is launched.
int mmd_nms_merge_n(const float* const* srcs, const int* const* cnts, int nsrc, float iou_threshold, int inclusive, int B, float* boxes, int* nbox, int maxg, unsigned long long* mask_ws, int* overflow, int merge01, int cap, float* big_ws, hipStream_t stream);

// Weighted box fusion (Solovyev, Wang, Gabruseva 2021) over the rows mmd_nms_merge_n gathers (same sources, counts, clamping and merge01
// rule; every gathered row remembers its source index 0..3, whichever image it came from): overlapping boxes of one label are averaged
// with their scores as weights instead of suppressed.  The rule, in fp32 with separately rounded operations (no FMA contraction):
// rows in the NMS's order (score descending, equal scores by gather index) are walked one at a time; a row joins, among the clusters
// of its own label (labels compared as stored floats), the one whose current fused box has the best IoU (the NMS's arithmetic) with
// it, provided IoU > iou_threshold (>= with inclusive != 0), the lowest cluster index on ties; joining advances the cluster in arrival
// order: w = fmaxf(score, FLT_MIN), W += w, Xk += w * xk for the four coordinates, n += 1, the source's bit is set, the fused box becomes
// Xk / W and its area (x2 - x1) * (y2 - y1) is recomputed.  Without such a cluster the row opens the next one, by the same advance from
// zeroed sums (a lone box comes out as (w * xk) / w).  After the walk the clusters with at least min_votes distinct sources go out in
// birth order: boxes [B, maxg, 5] (fused x1,y1,x2,y2, label), nbox [B], and into the nullable aux [B, maxg, 3] (W / n = mean member
// weight, n members, distinct sources); rows at and behind nbox[b] are left as they were.
// Capacity: more than maxg emitted clusters -> *overflow = 1, nbox = maxg, rows [0, maxg) are the first maxg emitted clusters.  More than
// 1024 gathered rows in an image -> *overflow = 1 and the fusion runs over its first 1024 rows in gather order (there is no chunked
// path and no global workspace: rows and clusters live in up to 86 016 B of LDS).  The outputs need no zeroing; `overflow` is sticky:
// the caller zeroes it.  nsrc outside 1..4, min_votes outside 1..nsrc, a null entry in srcs / cnts, maxg <= 0 or cap <= 0 ->
// MMD_EINVAL, nothing is launched.
int mmd_wbf_merge_n(const float* const* srcs, const int* const* cnts, int nsrc, float iou_threshold, int inclusive, int B, float* boxes, int* nbox, int maxg, float* aux, int min_votes, int* overflow, int merge01, int cap, hipStream_t stream);

// Floats per image of `big_ws` for NMS lists of up to nmax rows (0 when nmax <= 1024).  mmd_nms_merge: nmax = nteachers * cap * (merge01 ? 2 : 1).
int mmd_nms_ws_floats(int nmax);

// Rows per image the single-pass (all-in-LDS) NMS handles; the arrays' capacity itself is the run-time `cap` argument.
int mmd_pp_cap(void);

// Detection statistics of one evaluation batch, appended to a device-side record (csrc/evalstats.hip; get_batch_statistics and
// get_batch_central_distances, src/utils/utils.py:979-1136, bit for bit as mm_distillnet_amd/metrics.py computes them on the host).
// In: predictions rows [B, cap, 6] (x1,y1,x2,y2,score,class) with cnt [B], ground truth boxes [B, G, 5] (x1,y1,x2,y2,class) with
// nbox [B]; counts are clamped to [0, cap] / [0, G], rows at and behind a count are never read.
// Record, in image order then row order, behind cursor int[3] = {rows, images, classes}:
//   rec_rows [max_rows, 2] (score, class) and rec_tp [max_rows]: one row per prediction of every image that has predictions AND boxes,
//     in the given prediction order; bit k of rec_tp = true positive at IoU threshold fp32(0.5 + 0.05 k), k = 0..8 (best box by +1-pixel
//     IoU, first index on ties, each box taken once per threshold; a prediction whose class no box of the image has is never one);
//   rec_cd [max_images, 3] (sum dx, sum dy, n_boxes): one row per image, all zero for an image without boxes; the host divides;
//   rec_gt [max_gt]: the classes of every image's boxes.
// The call advances the cursor by the batch (a second small launch behind the first: calls append one after another in stream order).
// Workspace ws: B * mmd_eval_ws_floats(cap, G) floats, NULL when that is 0.  An image of up to mmd_eval_lds_cap(0) predictions and
// mmd_eval_lds_cap(1) boxes runs in LDS; a larger one runs the same algorithm through ws - any count the arrays can hold is exact.
// ws and the record need no zeroing (every entry is written before it is read); the caller zeroes `cursor` when it starts a record and
// `overflow`, which is sticky (set, never cleared).
// Capacity: a row, image or class that does not fit max_rows / max_images / max_gt -> *overflow = 1, it is dropped (the entries that
// fit are written, in order), nothing is written at or behind a capacity, and the cursor stops at the capacity.
// Null pointers (ws when the query is not 0), B, cap, G or a capacity <= 0 -> MMD_EINVAL, nothing is launched.
int mmd_eval_match(const float* rows, const int* cnt, int cap, const float* boxes, const int* nbox, int G, int B, float* rec_rows, int* rec_tp, int max_rows, float* rec_cd, int max_images, float* rec_gt, int max_gt, int* cursor, float* ws, int* overflow, hipStream_t stream);

// Floats PER IMAGE of mmd_eval_match's `ws` for arrays of cap predictions and G boxes per image: 0 when both fit the LDS path.
int mmd_eval_ws_floats(int cap, int G);

// Counts up to which mmd_eval_match keeps an image in LDS: which = 0 predictions, 1 boxes.
int mmd_eval_lds_cap(int which);

// ---- stable device-wide sort and the AP / CD table of an evaluation record (csrc/evaltable.hip)
// Items one block of the sort handles (a multiple of 64); block boundaries fall at its multiples.
int mmd_sort_tile(void);

// Bytes of mmd_sort_desc_f32's `ws` for n keys (monotone in n, never 0).  -22 for n < 0, n >= 2^31 or a size that does not fit an int.
int mmd_sort_desc_ws_bytes(long long n);

// Stable descending sort of n float32 keys, optionally grouped by a small integer class: perm_out[0..n) = the input indices ordered by
// class ascending (when cls is given), then key descending, then index ascending - np.lexsort((arange(n), -key, cls)) with -0.0 equal
// to +0.0, +-inf as numbers and every NaN key behind all others of its class, in input order.  key and cls are not modified.
// cls [n] (or NULL): integers 0 .. 255 stored as float; any other value -> *status |= 1 (sticky; the caller zeroes it) and the order of
// perm_out is unspecified (it still holds in-range indices).
// LSD radix sort, 8-bit digits, four passes over the key and one over the class, three launches per pass (per-block counts, a one-block
// scan, a stable scatter); every dependency between blocks is a kernel boundary.  ws: mmd_sort_desc_ws_bytes(n) bytes, 16-byte aligned,
// needs no zeroing.
// Null ws / status, null key / perm_out with n > 0, a misaligned pointer, n < 0 or n >= 2^31 -> -22, nothing is launched; n == 0
// succeeds without a launch.
int mmd_sort_desc_f32(const float* key, const float* cls, long long n, int* perm_out, void* ws, int* status, hipStream_t stream);

// Bytes of mmd_eval_table's `ws` (monotone in n_rows, never 0).  -22 for a negative count, a count >= 2^31 or a size that does not fit an int.
int mmd_eval_table_ws_bytes(long long n_rows, long long n_gt);

// The AP / CD table of an evaluation record (mmd_eval_match's layout; the counts are the cursor values the host has read):
// metrics.table_from_stats with predictions of equal score ranked in record order (the stable order of mmd_sort_desc_f32, cls = class).
// In: score_label [n_rows, 2] (score, class), tp [n_rows] (bit k: true positive at threshold k), cd [n_img, 3] (sum dx, sum dy,
// n_boxes), gt [n_gt] ground-truth classes.  Per ground-truth class c with n_c boxes and IoU threshold k, over the class's predictions
// by rank i: hits_i = true positives up to i, p_i = hits_i / (i + 1), r_i = hits_i / (n_c + 1e-16),
// AP = sum over the true positives of (r_i - r_(i-1)) * max_(j >= i) p_j, all in float64; a ground-truth class without predictions
// scores 0, a predicted class without ground truth is ignored.
// out double[16 + 256 * 8], every element written:
//   [0..8] mean AP over the ground-truth classes per threshold (fractions); [9..13] AP@Ave, AP@0.5, AP@0.75, CDx, CDy in percent;
//   [14] number of ground-truth classes; [15] 0;
//   [16 + 8 c ..] class c = 0 .. 255: present (0 / 1), n_gt, n_pred, precision, recall, AP, F1 at threshold 0, and a spare 0; all
//   zero for a class the ground truth does not hold.
// CDx / CDy: over the images with n_boxes > 0 the float32 quotient sum / n_boxes / image_size, averaged in float64.
// n_rows == 0: the ten APs are 0 and CDx = CDy = 100 * 100 (the reference's sentinel row).  n_rows > 0 without ground truth: NaN APs,
// as the host's empty mean.
// A class in gt or score_label that is not an integer 0 .. 255 -> *status |= 1 (sticky; the caller zeroes it), out is then unspecified.
// ws: mmd_eval_table_ws_bytes bytes, 16-byte aligned, needs no zeroing.  Null out / ws / status, a null array with a count > 0, a
// misaligned pointer or a negative count -> -22, nothing is launched.
int mmd_eval_table(const float* score_label, const int* tp, long long n_rows, const float* cd, long long n_img, const float* gt, long long n_gt, float image_size, double* out, void* ws, int* status, hipStream_t stream);

// Profiling hooks for bench.py (hipEvents on the launch stream).
int mmd_prof_is_on(int family);

int mmd_prof_dump_to(const char* path);

int mmd_prof_enable(int family, int on);

int mmd_prof_collect(int family, double* out);

// 1x1 conv as fp32 MFMA GEMM with fused producer-BN/swish/SE-gate prologue and bias/BN/act/residual/stats epilogue.
// Replaces nn.Conv2d(k=1) in Conv2dStaticSamePadding (src/YetAnotherEfficientNet.py:27-65; call sites :427,446,
// src/YetAnotherEfficientDet.py:171,238-265) + BatchNorm2d/swish that follow (:428,447,126-143).
int mmd_pwconv_fwd(const float* x, const float* w, float* y, int M, int K, int N, const float* in_scale, const float* in_shift, int in_act, const double* in_stats, const float* in_gamma, const float* in_beta, long long in_count, const float* gate, int rows_per_image, const float* bias, const float* out_scale, const float* out_shift, int out_act, const float* residual, double* stats, long long y_batch_stride, long long y_offset, double* stats_ws, int ws_slots, hipStream_t stream);

// --- feature-pyramid ("pyr") launches: the 5 levels of a shared-weight head layer in ONE launch.  pyr_desc is a HOST
// int array {n, B, H0, W0, H1, W1, ...}; level l occupies rows [row0_l, row0_l + B*H_l*W_l) of the row buffer and
// every level starts at a multiple of 128 rows; per-level BatchNorm data sit lev_stride channels apart.
// (Regressor/Classifier.forward, src/YetAnotherEfficientDet.py:463-532: conv_list shared across levels, bn_list per level.)
int mmd_pwconv_fwd_pyr(const float* x, const float* w, float* y, const int* pyr_desc, int K, int N, const float* bias, int out_act, double* stats, long long lev_stride, long long y_batch_stride, const long long* y_off_lev, hipStream_t stream);

// dw_grad (nullable; flip = 1 launches): the conv's weight gradient [9, C] += from the same launch, x operand = act(wg_x * wg_scale + wg_shift)
// with per-level coefficients lev_stride apart (what mmd_dwconv3_pyr_bwd_weight(wg_x, x, ...) computes); bn_sums (nullable, needs dw_grad
// and a swish producer): the sums of the BatchNorm(+swish) backward that consumes y - what mmd_bn_bwd_reduce_pyr(y, wg_x, ...) computes.
int mmd_dwconv3_pyr(const float* x, const float* w, float* y, const int* pyr_desc, int C, int flip, const float* in_scale, const float* in_shift, int in_act, const double* in_stats, const float* in_gamma, const float* in_beta, long long lev_stride, const float* wg_x, const float* wg_scale, const float* wg_shift, int wg_act, float* dw_grad, const float* wg_mean, const float* wg_invstd, double* bn_sums, hipStream_t stream);

int mmd_dwconv3_pyr_bwd_weight(const float* x, const float* dy, float* dw, const int* pyr_desc, int C, const float* in_scale, const float* in_shift, int in_act, long long lev_stride, hipStream_t stream);

int mmd_bn_bwd_reduce_pyr(const float* g_in, const float* z, const float* scale, const float* shift, const float* mean, const float* invstd, int act, const int* pyr_desc, long long lev_stride, float* g_out, double* sums, int C, hipStream_t stream);

int mmd_bn_bwd_apply_pyr(const float* g, const float* z, const float* mean, const float* invstd, const float* gamma, const double* sums, const int* pyr_desc, long long lev_stride, float* dz, float* dgamma, float* dbeta, int C, const float* scale, const float* shift, int act, hipStream_t stream);

// out = a + b (+ c, nullable) over a pyramid row buffer [rows, C] (the two heads' input gradients + the MTA loss' feature gradient =
// the gradient w.r.t. the last BiFPN cell's outputs), and per level l with z[l] != NULL (host arrays of n device pointers; that level's
// feature map is BN(z[l]), z[l] its own [B*H*W, C] tensor) sums[l] [2C] (+)= [sum out, sum out*xhat]: the BatchNorm-backward reduce
// passes of the five output nodes (src/YetAnotherEfficientDet.py:338-390) in the launch that completes their upstream gradient.
int mmd_pyr_add_bnsums(const float* a, const float* b, const float* c, float* out, const int* pyr_desc, int C, const float* const* z, const float* const* mean, const float* const* invstd, double* const* sums, hipStream_t stream);

// dW[N,K] += dY^T * pro(X) (autograd of the 1x1 conv weight; reference: loss.backward(), src/optimization/traditional.py:182).
int mmd_pwconv_bwd_weight(const float* dy, const float* x, float* dw, int M, int K, int N, const float* in_scale, const float* in_shift, int in_act, const float* gate, int rows_per_image, hipStream_t stream);

// All 1x1-conv weight gradients of a backward segment in ONE persistent launch + one deterministic fold (csrc/pw_wgrad_grouped.hip;
// reference: autograd of every nn.Conv2d(k=1) weight of the student, src/YetAnotherEfficientNet.py:427,446, src/YetAnotherEfficientDet.py:171,238-265).
// The caller fills dy / x / dw / in_scale / in_shift / gate / M / K / N / in_act / rows_per_image of each layer (same operand meaning as
// mmd_pwconv_bwd_weight), mmd_wgrad_plan (host) fills the rest and returns the item / tile counts and the workspace size; the planned
// table is then copied to device memory once and mmd_wgrad_grouped launched every step.  dW is WRITTEN (not accumulated), sums are
// bit-reproducible run to run (no atomics).
typedef struct MmdWgradLayer {
  const float* dy; const float* x; float* dw;
  const float* in_scale; const float* in_shift; const float* gate;
  int M, K, N; int in_act; int rows_per_image;
  int mchunk; int nsplit; int ntn, ntk; int item0; int tile0; int pad_;
  long long ws_off;
} MmdWgradLayer;
int mmd_wgrad_plan(MmdWgradLayer* layers_host, int n, int rows_per_item, int* n_items, int* n_tiles, long long* ws_floats);
int mmd_wgrad_grouped(const MmdWgradLayer* layers_dev, int n_layers, int n_items, int n_tiles, float* ws, int blocks, double flops, double bytes, hipStream_t stream);
// precision "bf16" (BASELINE configs[4]): the same launch with both operands rounded to bf16 at the MFMA input, fp32 accumulate
// (mmd_pwconv_bwd_weight_bf16's arithmetic for every layer of the table)
int mmd_wgrad_grouped_bf16(const void* layers_dev, int n_layers, int n_items, int n_tiles, float* ws, int blocks, double flops, double bytes, hipStream_t stream);
// mmd_wgrad_grouped / _bf16 with one more choice made by the caller: rows32 = 1 promises that every layer's M is a multiple of 32 (any net
// at B >= 2: the smallest map is 4 x 4) - the kernel then runs without row clamps / masks and with running operand pointers
// (57 v_cndmask + 43 address instructions per 32-row step less on a kernel whose VALU instructions are MFMA time).  rows32 = 0: as the plain entry points.
// bf16: 0 = fp32 products - with rows32 on the bf16 matrix pipe in the SPLIT form (see mmd_pwconv_fwd_form below; MMD_MFMA_F32=1 in the
// environment keeps v_mfma_f32), 1 = operands rounded to bf16 (mmd_wgrad_grouped_bf16), 2 = fp32 products on v_mfma_f32_32x32x2_f32.
int mmd_wgrad_grouped_form(const void* layers_dev, int n_layers, int n_items, int n_tiles, float* ws, int blocks, double flops, double bytes, int bf16, int rows32, hipStream_t stream);

// dX[M,K] (=|+=) dY[M,N] * W[N,K] using the transposed weight copy Wt[K,N] (autograd of the 1x1 conv input).
int mmd_pwconv_bwd_data(const float* dy, const float* wt, float* dx, int M, int K, int N, int accumulate, hipStream_t stream);

// --- bf16 mixed-precision variants of the four 1x1-conv entry points (BASELINE config 5: "bf16 mixed precision, MFMA bf16").
// Same contracts and fp32 tensors; the two MFMA operands are rounded to bf16 (round-to-nearest-even) right before
// v_mfma_f32_32x32x16_bf16, accumulation / prologue / epilogue / BatchNorm statistics stay fp32.  The reference has no
// reduced-precision path ("no AMP anywhere"); this is what torch.autocast(bf16) would make of its nn.Conv2d(k=1).
int mmd_pwconv_fwd_bf16(const float* x, const float* w, float* y, int M, int K, int N, const float* in_scale, const float* in_shift, int in_act, const double* in_stats, const float* in_gamma, const float* in_beta, long long in_count, const float* gate, int rows_per_image, const float* bias, const float* out_scale, const float* out_shift, int out_act, const float* residual, double* stats, long long y_batch_stride, long long y_offset, double* stats_ws, int ws_slots, hipStream_t stream);

// mmd_pwconv_fwd with the kernel family chosen PER CALL (round 6; replaces the process-wide mmd_pwconv_rows_mode / mmd_pwconv_longk_mode
// setters - the library keeps no global state besides the communicator): form 0 = the measured shape filters decide (what
// mmd_pwconv_fwd does), 1 = thin-K row-slab kernel (csrc/pw_rows.hip), 2 = LDS-tiled kernels only, 3 = long-K LDS-DMA kernel (csrc/pw_longk.hip),
// 4 = all-N K-sliced slab kernel (csrc/pw_slab.hip).  A family that does not support the launch falls through to the LDS-tiled kernels.
// ws / ws_floats (nullable): caller-owned workspace for the slab kernel's K slices (mmd_pwconv_slab_ws_floats floats; contents undefined
// before and after, no zeroing needed); without one a launch that would need slices keeps the LDS-tiled kernels (form 0) or is refused (form 4).
// The engine calls this with form 0; forms 1 - 4: tests and A/B timing.  Conv2dStaticSamePadding(k=1), src/YetAnotherEfficientNet.py:27-65.
// form | 16 (MMD_PW_FORM_NATIVE): fp32 products on v_mfma_f32_32x32x2_f32.  Without it the LDS-tiled kernels compute the SAME fp32 GEMM in the
// split form where K >= 64 and N > 48 (csrc/common.h): each fp32 operand value is split exactly into three bf16 pieces (round to nearest:
// x = h + m + l, both residuals exact), a * b is taken as the six largest of the nine partial products - each exact in fp32 - on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulate; the three dropped ones are at most 2^-23 |a * b| (2^-27 rms), the size of ONE 2^-24 rounding of an fp32
// accumulate.  192 matrix-pipe cycles per 16-deep k group instead of 512.  Error against float64: not above the v_mfma_f32 chain's
// (tests/test_gpu_kernels.py::test_split3_precision; measured lower on every shape).  Operands must be finite (Inf - Inf in a residual is NaN).
// MMD_MFMA_F32=1 in the environment: the whole library on v_mfma_f32 (A/B timing, bisecting).
int mmd_pwconv_fwd_form(const float* x, const float* w, float* y, int M, int K, int N, const float* in_scale, const float* in_shift, int in_act, const double* in_stats, const float* in_gamma, const float* in_beta, long long in_count, const float* gate, int rows_per_image, const float* bias, const float* out_scale, const float* out_shift, int out_act, const float* residual, double* stats, long long y_batch_stride, long long y_offset, double* stats_ws, int ws_slots, float* ws, long long ws_floats, int form, hipStream_t stream);

int mmd_pwconv_fwd_pyr_bf16(const float* x, const float* w, float* y, const int* pyr_desc, int K, int N, const float* bias, int out_act, double* stats, long long lev_stride, long long y_batch_stride, const long long* y_off_lev, hipStream_t stream);

int mmd_pwconv_bwd_weight_bf16(const float* dy, const float* x, float* dw, int M, int K, int N, const float* in_scale, const float* in_shift, int in_act, const float* gate, int rows_per_image, hipStream_t stream);

int mmd_pwconv_bwd_data_bf16(const float* dy, const float* wt, float* dx, int M, int K, int N, int accumulate, hipStream_t stream);

// --- BatchNorm backward as an operand prologue of the two gradient GEMMs of the conv in front of it (one launch and one
// [M, N] round trip less per BatchNorm on the backward's main chain).  (g, z): gradient w.r.t. the BatchNorm(+swish) output and the
// conv's raw output, both [M, N]; scale = gamma*invstd, shift = beta - mean*scale; sums[2N] = [sum g', sum g'*xhat] from
// mmd_bn_bwd_reduce (or the depthwise input-gradient epilogue); g' = g * mul_b[image] * swish'(z*scale+shift) (act = 1) - the same
// rule as mmd_bn_bwd_apply.  mmd_pwconv_bwd_data_bn side outputs (nullable): dz_out [M, N] = the evaluated BatchNorm backward, stored once
// so that the weight gradient can be the plain mmd_pwconv_bwd_weight(dz_out, x); dgamma / dbeta (+)= [sum g'*xhat, sum g'].  Autograd of nn.BatchNorm2d (train) behind nn.Conv2d(k=1): src/YetAnotherEfficientNet.py:427-428,446-447,477;
// src/YetAnotherEfficientDet.py:171-176.
int mmd_pwconv_bwd_data_bn(const float* g, const float* z, const float* wt, float* dx, int M, int K, int N, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, const float* mul_b, int rows_per_image, float* dz_out, float* dgamma, float* dbeta, hipStream_t stream);

// mmd_pwconv_bwd_data_bn with two more (optional) jobs for its epilogue.  residual (may alias dx): dx = BnBwd(g, z) * W + residual - the
// skip branch's / earlier consumers' contributions already sit in the gradient buffer.  xs_*: dx is then the COMPLETE gradient w.r.t. a
// tensor y' = BN'(xs_z) * xs_mul_b[image] (+ skip) (an MBConv block output / a tap), and xs_sums [2K] (+)= [sum g', sum g'*xhat'],
// g' = dx * xs_mul_b[image], xhat' = (xs_z - xs_mean)*xs_invstd: the reduce pass of that upstream BatchNorm's backward, without a launch of
// its own and without the scale_acc launch that added the skip gradient (src/YetAnotherEfficientNet.py:477-485).  stats_ws / ws_slots
// (nullable / 0) as in mmd_pwconv_fwd: slotted sums for launches with more than 128 row tiles.  p5_* (an MBConv project conv; not with
// residual / xs): dx = g1 is the gradient w.r.t. the gated activation, and p5_out [5][p5_B][K] (+)= what mmd_chan_pool_bwd(p5_z = z1,
// p5_scale .. p5_invstd of BatchNorm-1, g1) computes - the pooled pass of the squeeze-excite / BatchNorm-1 backward - taken from the
// output tiles instead of by a launch re-reading g1 and z1.
int mmd_pwconv_bwd_data_bn2(const float* g, const float* z, const float* wt, float* dx, int M, int K, int N, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, const float* mul_b, int rows_per_image, float* dz_out, float* dgamma, float* dbeta, const float* residual, const float* xs_z, const float* xs_mean, const float* xs_invstd, const float* xs_mul_b, int xs_rows_per_image, double* xs_sums, double* stats_ws, int ws_slots, const float* p5_z, const float* p5_scale, const float* p5_shift, const float* p5_mean, const float* p5_invstd, float* p5_out, int p5_B, hipStream_t stream);
// All-N, K-sliced slab GEMM (csrc/pw_slab.hip, round 6) for the small-M 1x1 convs whose A operand carries an arithmetic prologue (the
// student's expand-conv input gradients behind BatchNorm + swish, its project convs behind live BatchNorm + swish + gate; autograd of
// src/YetAnotherEfficientNet.py:427-447): a block owns a 32-row slab x ALL N x a slice of K, so the prologue is evaluated once per element
// instead of once per 64-wide column tile; launches with few row slabs are cut along K and the slices' partial slabs are added in slice
// order by a second launch that owns the epilogue (deterministic, no atomics).  mmd_pwconv_slab_ws_floats: workspace floats such a launch
// needs (0 = it runs unsliced, or the family does not take the shape); mmd_pwconv_bwd_data_bn2_form = mmd_pwconv_bwd_data_bn2 + workspace + form.
int mmd_pwconv_slab_ws_floats(int M, int K, int N, int bn_operand);
int mmd_pwconv_bwd_data_bn2_form(const float* g, const float* z, const float* wt, float* dx, int M, int K, int N, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, const float* mul_b, int rows_per_image, float* dz_out, float* dgamma, float* dbeta, const float* residual, const float* xs_z, const float* xs_mean, const float* xs_invstd, const float* xs_mul_b, int xs_rows_per_image, double* xs_sums, double* stats_ws, int ws_slots, const float* p5_z, const float* p5_scale, const float* p5_shift, const float* p5_mean, const float* p5_invstd, float* p5_out, int p5_B, float* ws, long long ws_floats, int form, hipStream_t stream);

int mmd_pwconv_bwd_data_bn2_bf16(const float* g, const float* z, const float* wt, float* dx, int M, int K, int N, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, const float* mul_b, int rows_per_image, float* dz_out, float* dgamma, float* dbeta, const float* residual, const float* xs_z, const float* xs_mean, const float* xs_invstd, const float* xs_mul_b, int xs_rows_per_image, double* xs_sums, double* stats_ws, int ws_slots, const float* p5_z, const float* p5_scale, const float* p5_shift, const float* p5_mean, const float* p5_invstd, float* p5_out, int p5_B, hipStream_t stream);

// Round 4: backward of an MBConv EXPAND conv with its train-mode BatchNorm-0 + swish in ONE pass over the 6x expanded gradient, for the
// thin-input high-resolution blocks (autograd of `_expand_conv` -> `_bn0` -> swish, src/YetAnotherEfficientNet.py:456-460):
//   dz0 = BnBwd0(g0, z0) evaluated once per element into LDS (never written to HBM);  dx[M, Cin] = dz0 . w[Cmid, Cin] (+ residual, may be dx);
//   dw[Cmid, Cin] += dz0^T . x[M, Cin];  dgamma / dbeta (+)= the reduce pass' sums;  optional xs_* as in mmd_pwconv_bwd_data_bn2 (dx completes
//   the gradient of an upstream BatchNorm output: xs_sums[2 Cin] (+)= its backward sums).
// Replaces mmd_pwconv_bwd_data_bn2 (which stores dz0 for the weight gradient) + the layer's entry in mmd_wgrad_grouped (which reads it back).
// mmd_mbconv_expand_bwd_supported(Cin, Cmid) -> 1 for (16, 96), (24, 144), (32, 192).
int mmd_mbconv_expand_bwd_supported(int Cin, int Cmid);
int mmd_mbconv_expand_bwd_fused(const float* g0, const float* z0, const float* x, const float* w, float* dx, const float* residual, float* dw, int M, int Cin, int Cmid, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, float* dgamma, float* dbeta, const float* xs_z, const float* xs_mean, const float* xs_invstd, const float* xs_mul_b, int xs_rows_per_image, double* xs_sums, hipStream_t stream);

int mmd_pwconv_bwd_data_bn_bf16(const float* g, const float* z, const float* wt, float* dx, int M, int K, int N, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, const float* mul_b, int rows_per_image, float* dz_out, float* dgamma, float* dbeta, hipStream_t stream);

int mmd_pwconv_bwd_weight_bn(const float* g, const float* z, const float* x, float* dw, int M, int K, int N, const float* in_scale, const float* in_shift, int in_act, const float* gate, int rows_per_image, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, const float* mul_b, int bn_rows_per_image, float* dgamma, float* dbeta, hipStream_t stream);

int mmd_pwconv_bwd_weight_bn_bf16(const float* g, const float* z, const float* x, float* dw, int M, int K, int N, const float* in_scale, const float* in_shift, int in_act, const float* gate, int rows_per_image, const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums, long long count, int act, const float* mul_b, int bn_rows_per_image, float* dgamma, float* dbeta, hipStream_t stream);

// Every 1x1 weight of the student transposed in one launch (desc rows: src_off, dst_off, R, C, first_tile).
int mmd_transpose_batched(const float* src_base, float* dst_base, const long long* desc, int n, int total_tiles, hipStream_t stream);

// dst[C,R] = src[R,C]^T (refreshes the Wt copies after an optimizer step).
int mmd_transpose2d(const float* src, float* dst, int R, int C, hipStream_t stream);

// Stem conv forward, direct: NCHW image -> NHWC rows [B*OH*OW, Cout] (Cout in {32,40,48,56,64}; 3x3, stride 2, TF-SAME; w = the [Cout, Kp] im2col weight
// layout, k = ci*9 + i*3 + j).  Epilogue: folded BN + swish (frozen nets) or raw output + BatchNorm sums (train; stats_ws/ws_slots
// as in mmd_dwconv_fwd).  src/YetAnotherEfficientNet.py:519-523,597-604.  mmd_stem_im2col + the GEMM entry points remain for the weight gradient.
int mmd_stem_conv_fwd(const float* x, const float* w, float* y, int B, int Cin, int H, int W, int Kp, int Cout, const float* out_scale, const float* out_shift, int out_act, double* stats, double* stats_ws, int ws_slots, hipStream_t stream);

// ModelWithNMSLossAugmented.merge_batch_0_1 (src/optimization/train_methods.py:291-308): out = in, except image 1 =
// log10(max(in[0]^10 + in[1]^10, 1e-7)) (the reference's literal 10th power).  per_image = C*H*W.
int mmd_audio_merge01(const float* in, float* out, long long per_image, int B, hipStream_t stream);

// ModelWithNMSLossAugmented.average_batch_0_1 (:279-289): f[image 1] = (f[image 0] + f[image 1]) / 2, in place.
int mmd_avg_image01(float* f, long long per_image, hipStream_t stream);

// ---- input preparation.  cv2 sampling rules restated (cv2 is not in the reference tree): parity with
// cv2 itself is unpinned, the kernels are pinned to oracle/input_ref.py.
// (min, max) of clamp(src, lo, hi) for the thermal min-max stretch (src/datasets/MultimodalDetection.py:196-211). dtype: 0 u8, 1 u16, 2 f32.
int mmd_image_minmax(const void* src, int dtype, long long n, float lo, float hi, float* mm, hipStream_t stream);

// Normalizer + Resizer + HWC->CHW for one image (src/datasets/transformations.py:315-330,407-433; MultimodalDetection.py:245-255):
// dst[C,S,S] = letterbox(bilinear((pre(src)*scale - mean)/std)); pre = clamp + round((v-min)*255/(max-min)) when minmax != 0.
int mmd_image_letterbox(const void* src, int dtype, int H, int W, int C, float scale, const float* mean, const float* stdv, int minmax, float lo, float hi, const float* mm, int common_size, float* dst, hipStream_t stream);

// The training-time augmentations in front of mmd_image_letterbox, for a stacked batch of one modality in ONE launch (the sample index in
// the grid): the 2-pixel column shift (src/datasets/MultimodalDetection.py:236-242,320-327) and HSVAdjust (src/datasets/transformations.py:133-190).
// src[B,H,W,C]: C = 3 uint8, or C = 1 uint16 (thermal: minmax / lo / hi as in mmd_image_letterbox, mm[B,2] = every sample's
// mmd_image_minmax of its UNSHIFTED frame) -> dst[B,C,S,S].  Row b of aug[B,5] (device) = (on, hue_deg, sat, val, shift_px):
//   shift_px > 0: source pixel (y, x) reads (y, x + shift_px) for x < W - shift_px and is 0 otherwise (0 in the stretched frame, as
//                 upstream shifts after the thermal stretch); index math, no shifted frame is written.
//   hsv != 0 and on != 0 (C = 3 only): per source pixel, before the bilinear taps: rgb/255 -> HSV, h += hue_deg wrapped into [0, 360),
//                 s = clip(sat*s, 0, 1), v = clip(val*v, 0, 1), HSV -> RGB, *255 without rounding; then (v*scale - mean)/std and the letterbox.
//   hsv == 0: the `on` column is ignored, so ONE table serves all modalities of a sample (as one HSVAdjust.__call__ draws once) and the
//                 thermal launch takes its shift from it.  hsv != 0 with C = 1: -22 (upstream's HSVAdjust fails on the 2-D thermal frame).
// cv2.cvtColor is restated from OpenCV's documented float formulas: parity with cv2 itself is UNPINNED, the kernel is held to
// tests/hsv_ref.py.  A sample whose row has on == 0 (or hsv == 0) and shift_px == 0 gets exactly the bits of mmd_image_letterbox.
// -22 before any launch: null src / aug / dst (mm with minmax), B, H, W or common_size < 1 (B, common_size > 65535), C not in {1, 3},
// minmax with C = 3.
int mmd_image_letterbox_aug_batch(const void* src, int B, int H, int W, int C, float scale, const float* mean, const float* stdv, int minmax, float lo, float hi, const float* mm, const float* aug, int hsv, int common_size, float* dst, hipStream_t stream);

// Resizer's audio branch: cv2.resize(INTER_CUBIC) of an [h,w,C] spectrogram stack to [C,S,S] (transformations.py:435-441).
int mmd_resize_cubic(const float* src, int h, int w, int C, int common_size, float* dst, hipStream_t stream);

// mmd_resize_cubic (Resizer's audio branch, transformations.py:435-441) for a batch in ONE launch: src[batch, h, w, C] ->
// dst[batch, C, S, S], the sample index in the grid; every sample's bits are those of the per-sample entry point.
int mmd_resize_cubic_batch(const float* src, int batch, int h, int w, int C, int common_size, float* dst, hipStream_t stream);

// ---- waveform front end (csrc/melspec.hip).  MultimodalDetection.merge_audios (src/datasets/MultimodalDetection.py:329-353, called per
// sample from yield_batch, :355-367) and Audio2Spectogram (src/datasets/transformations.py:251-266):
// librosa.feature.melspectrogram(sr=44100, n_fft=1024, hop_length=256, n_mels=80) of each microphone channel.  librosa's arithmetic
// is restated (it is not in the reference tree): parity with librosa itself is unpinned, the kernel is pinned to tests/melspec_ref.py.
// Frames of a center=True STFT over n_samples samples: 1 + n_samples / 256, or -22 for n_samples <= 512 (the reflect padding of 512
// samples needs more than 512).  No GPU work.
int mmd_melspec_frames(long long n_samples);

// The melspectrogram call of merge_audios (src/datasets/MultimodalDetection.py:329-353) and Audio2Spectogram
// (src/datasets/transformations.py:251-266) for all channels of one recording in ONE launch.
// out[80, T, channels] (mel, frame, channel - the order np.transpose(np.stack(...), (1, 2, 0)) gives upstream and mmd_resize_cubic
// reads), T = mmd_melspec_frames(n_samples): POWER mel spectrogram (no power_to_db, like merge_audios) of wav_a[channels, n_samples],
// or of (wav_a + wav_b) / 2 in fp32 when wav_b is not null (merge_audios, :339).  Reflect padding, periodic Hann window, 1024-point
// real FFT at hop 256, Slaney mel bank handed over in band form: row m = band_w[m * band_stride + j] on bins band_start[m] + j,
// j < band_len[m] <= band_stride (80 * band_stride <= 4096; mm_distillnet_amd.audio.mel_bands).  One launch, raw device pointers,
// no allocation; out needs no zeroing and two calls on the same input give the same bits.  -22 on null pointers / bad sizes before any launch.
int mmd_melspec_power(const float* wav_a, const float* wav_b, int channels, long long n_samples, const int* band_start, const int* band_len, const float* band_w, int band_stride, float* out, hipStream_t stream);

// mmd_melspec_power for a whole batch, and the dB map the student's stored input is (mp3_to_pkl.py:31-41: melspectrogram(...), then
// librosa.power_to_db(S, ref=np.max); stacked by MultimodalDetection.__getitem__, src/datasets/MultimodalDetection.py:219-224; the
// melspectrogram call is merge_audios', MultimodalDetection.py:329-353, and Audio2Spectogram's, transformations.py:251-266).
// wav_a[batch, channels, n_samples] (wav_b: the partner recordings of the same shape, or null) -> out[batch, 80, T, channels], the sample
// index in the grid: one launch for db = 0, and every sample's bits are those mmd_melspec_power gives that sample alone.
// db = 1: power_to_db per (sample, channel) map S[80, T] as published - ls = 10 log10(max(1e-10, S)) - 10 log10(max(1e-10, max S)),
// then max(ls, max(ls) - 80) - in fp32 with each product and the difference rounded on its own.  librosa is not in the reference tree:
// the rule is restated and pinned to tests/melspec_db_ref.py, parity with librosa's power_to_db itself is UNPINNED.  The maxima go
// through max_ws[batch * channels] (any 4-byte words; null allowed for db = 0) as unsigned atomic maxima of the float bits (power is
// >= +0), so they do not depend on the order of arrival: two calls give the same bits.  Launch sequence for db = 1: one zero-fill launch on
// max_ws, the spectrogram launch, one elementwise launch.  max_ws and out need no zeroing; no allocation, no host synchronisation
// (capturable in a hipGraph).  -22 on null pointers / bad sizes / db outside {0, 1} before any launch.
int mmd_melspec_batch(const float* wav_a, const float* wav_b, int batch, int channels, long long n_samples, const int* band_start, const int* band_len, const float* band_w, int band_stride, int db, float* max_ws, float* out, hipStream_t stream);

// The same power_to_db(S, ref=np.max) (mp3_to_pkl.py:31-41), in place, for a ready-made POWER stack x[batch, h, w, channels] (what
// Audio2Spectogram, src/datasets/transformations.py:251-266, hands on): the maximum is again per (sample, channel) map.  On the db = 0
// output of mmd_melspec_batch it gives the bits of db = 1.  Values below +0 count as 0 in the maximum (max(1e-10, .) floors them anyway).
// One zero-fill launch on max_ws[batch * channels] (needs no zeroing), one maximum launch, one elementwise launch; channels <= 1024.
// Restated from the published rule, pinned to tests/melspec_db_ref.py; parity with librosa's power_to_db itself is UNPINNED.
// -22 on null pointers / bad sizes before any launch.
int mmd_power_to_db(float* x, int batch, int h, int w, int channels, float* max_ws, hipStream_t stream);

// mmd_melspec_batch over overlapping windows read straight out of ONE recording (streaming detection, AudioDetector.detect_stream;
// the melspectrogram call is merge_audios', src/datasets/MultimodalDetection.py:329-353, the dB map mp3_to_pkl.py:31-41's):
// wav[channels, n_total], win_start[batch] (DEVICE int64 sample offsets, so one captured hipGraph serves every group of a recording),
// win_len samples per window -> out[batch, 80, T, channels], T = mmd_melspec_frames(win_len).  Window b is exactly the clip
// wav[:, win_start[b] : win_start[b] + win_len]: the reflect padding happens at the window's own two ends (edge sample not repeated)
// and never reads the recording's samples outside the window, nor before wav or past n_total; the dB maximum is per (window, channel).
// For db = 0 and db = 1 the output is bit for bit what mmd_melspec_batch gives on the materialised [batch, channels, win_len] stack of
// those slices (one kernel body; the window offset enters the base pointer only).  The table's contents cannot be checked on the
// host: a start outside [0, n_total - win_len] is the CALLER'S ERROR (the kernel clamps it into that range, so such a window is the
// wrong one but no read leaves the recording).  Launch sequence, max_ws[batch * channels] and out as mmd_melspec_batch: they need no
// zeroing, two calls give the same bits, no allocation, no host synchronisation.  -22 before any launch on null pointers, batch < 1,
// channels < 1, win_len <= 512 (too short for the padding), win_len > n_total, a bad band_stride or db outside {0, 1}.
int mmd_melspec_windows(const float* wav, int channels, long long n_total, const long long* win_start, int batch, long long win_len, const int* band_start, const int* band_len, const float* band_w, int band_stride, int db, float* max_ws, float* out, hipStream_t stream);

// mmd_melspec_windows with the recording in a RING (live streaming detection, AudioDetector.open_stream; the melspectrogram call is
// merge_audios', src/datasets/MultimodalDetection.py:329-353, the dB map mp3_to_pkl.py:31-41's): ring[channels, cap], absolute sample p
// of channel c at ring[c * cap + p % cap]; win_start[batch] (DEVICE int64) are ABSOLUTE positions counted from the session's start.
// Window b is samples win_start[b] .. win_start[b] + win_len - 1, read modulo cap; the reflect padding stays in window coordinates, so
// for db = 0 and db = 1 the output is bit for bit what mmd_melspec_windows gives for that window of the linear recording (one kernel
// body, one more mode: only the staging load's address differs - the start is reduced modulo cap once per block and every load wraps
// with one compare and one subtract).  Nothing but the window's win_len slots per channel is read.  A negative start is the CALLER'S
// ERROR (the kernel clamps it to 0: the wrong window, but no read leaves the ring); that the window's samples are still resident is
// the caller's schedule.  Launch sequence, max_ws[batch * channels] and out as mmd_melspec_windows: they need no zeroing, two calls
// give the same bits, no allocation, no host synchronisation.  -22 before any launch on the refusals of mmd_melspec_windows, and on
// win_len > cap.
int mmd_melspec_windows_ring(const float* ring, int channels, long long cap, const long long* win_start, int batch, long long win_len, const int* band_start, const int* band_len, const float* band_w, int band_stride, int db, float* max_ws, float* out, hipStream_t stream);

// mmd_melspec_windows_ring for the rings of a BANK of sessions (AudioDetector.open_bank; the melspectrogram call is merge_audios',
// src/datasets/MultimodalDetection.py:329-353, the dB map mp3_to_pkl.py:31-41's): rings[n_sessions, channels, cap], one block of
// memory, absolute sample p of channel c of session s at rings[(s * channels + c) * cap + p % cap].  win_sess[batch] (DEVICE int32)
// names the session of each window, win_start[batch] (DEVICE int64) its ABSOLUTE position in that session's recording; sessions may
// repeat and come in any order.  One kernel body, one more mode: only the row base (sess * channels + c) * cap differs, so for db = 0
// and db = 1 window b's output is bit for bit what mmd_melspec_windows_ring gives for rings + win_sess[b] * channels * cap with the
// same start.  A session outside 0 .. n_sessions-1 is the CALLER'S ERROR (the kernel clamps it into that range: the wrong window, but
// no read leaves rings); a negative start is clamped to 0 as in the ring mode.  Launch sequence, max_ws[batch * channels] and out as
// mmd_melspec_windows_ring: they need no zeroing, two calls give the same bits, no allocation, no host synchronisation.  -22 before
// any launch on the refusals of mmd_melspec_windows_ring, on a null win_sess and on n_sessions < 1.
int mmd_melspec_windows_rings(const float* rings, int n_sessions, int channels, long long cap, const int* win_sess, const long long* win_start, int batch, long long win_len, const int* band_start, const int* band_len, const float* band_w, int band_stride, int db, float* max_ws, float* out, hipStream_t stream);

// ---- sample-rate conversion and PCM decoding (csrc/resample.hip): what librosa.load(path, sr=44100) does in front of the mel
// spectrogram upstream (mp3_to_pkl.py:31; merge_audios, src/datasets/MultimodalDetection.py:335-336).
// x[rows, n_in] at sr_in -> y[rows, n_out] at sr_out, rows = batch x channels, with L / M = sr_out / sr_in in lowest terms and
// n_out = ceil(n_in * L / M):  y[t] = sum_{j < taps} B[p][j] * x[n + j - taps / 2 + 1],  n = (t * M) // L,  p = (t * M) % L,  where
// B[p][j] = h(p / L - (j - taps / 2 + 1)) is the float32 windowed-sinc bank of mm_distillnet_amd.audio.resample_bank (after the published
// design of resampy's kaiser_best, as an exact polyphase filter; the rule is the project's own, pinned to tests/resample_ref.py: parity
// with resampy / librosa themselves is UNPINNED).  x is ZERO-EXTENDED at both ends: samples outside 0 .. n_in - 1 count as 0, there is
// no reflect padding, so the first and last taps / 2 input samples' worth of output fade in and out.
// Layout of the arguments: bank[taps, L] TRANSPOSED and in OUTPUT-phase order - bank[j * L + r] = B[(r * M) % L][j] for r = t % L - so
// that neighbouring outputs read neighbouring addresses for a fixed tap; phase_off[L], phase_off[r] = (r * M) // L.  Both are DEVICE
// tables whose contents cannot be checked on the host: a wrong table is the CALLER'S ERROR (the kernel clamps what it takes from
// phase_off into the input span it staged, so such a call gives wrong samples but reads nothing outside x's row and writes nothing
// outside y's).  fp32 accumulation in tap order; one launch, plain stores, no atomics, no allocation, no host synchronisation: y needs
// no zeroing, elements behind n_out of a larger buffer are not touched, and two calls give the same bits.  Outputs are indexed as
// (period, phase), so no product t * M is formed.  Caps: L, M in 1 .. 1024, taps even in 2 .. 4096, rows <= 65535, n_in <= 2^50.
// -22 before any launch on null pointers, rows < 1, n_in < 1, L or M outside 1 .. 1024, taps odd or outside 2 .. 4096,
// n_out != ceil(n_in * L / M), or a size above the caps.
int mmd_resample_poly(const float* x, int rows, long long n_in, const float* bank, const int* phase_off, int L, int M, int taps, float* y, long long n_out, hipStream_t stream);

// A PCM WAV's frames as read from the file -> the waveforms the front end takes (detect.py --resample; upstream gets floats from
// librosa.load, mp3_to_pkl.py:31): pcm = interleaved little-endian SIGNED samples [frames, channels] of width 2, 3 or 4 bytes ->
// out[channels, frames] float32, a de-interleaving transpose staged through LDS (word reads, coalesced float stores; pcm needs no
// alignment).  16-bit: i / 2^15; 24-bit: sign-extended, i / 2^23; 32-bit: (float)i rounded to nearest, then * 2^-31 - each equal bit for
// bit to numpy.float32(i) / numpy.float32(2^k).  One launch, no allocation, no host synchronisation; out needs no zeroing and two calls
// give the same bits.  Caps: channels * width <= 16384.  -22 before any launch on null pointers, frames < 1, channels < 1, another
// width, or channels above the cap.
int mmd_pcm_to_float(const unsigned char* pcm, long long frames, int channels, int width, float* out, hipStream_t stream);

// ---- the device sample ring of live streaming detection (csrc/live.hip, AudioDetector.open_stream): chunks go in as they arrive,
// mmd_melspec_windows_ring reads windows back out.  ring[channels, cap] float32 at a fixed address; absolute sample p (int64, counted
// from the session's start) of channel c lives at ring[c * cap + p % cap].
// ring[c, (pos + i) % cap] = src[c * src_stride + i] for i < n: n samples per channel from float rows src_stride apart (src_stride > n:
// a column slice of a larger tensor).  pos is reduced modulo cap on the host and n <= cap, so a position wraps at most once: one
// compare and one subtract per store, lanes store consecutive floats (two contiguous runs where the chunk crosses the ring's end).
// One launch, plain vector stores, no atomics, no allocation, no host synchronisation; nothing outside those n positions per channel
// is touched, two calls give the same bits.  Which older sample a store overwrites is the caller's schedule
// (mm_distillnet_amd.audio.live_schedule).  Caps: channels <= 65535, cap and pos <= 2^50.  -22 before any launch on null pointers,
// channels < 1, n < 1, n > cap, pos < 0, src_stride < n, or a size above the caps.
int mmd_ring_push(const float* src, long long src_stride, int channels, long long n, float* ring, long long cap, long long pos, hipStream_t stream);

// The same for a PCM WAV's frames as read from the file: pcm = interleaved little-endian SIGNED samples [frames, channels] of width
// 2, 3 or 4 bytes (no alignment needed), decoded exactly as mmd_pcm_to_float decodes them - one tile body, the floats are bit for bit
// the same - de-interleaved through LDS and stored at ring[c, (pos + f) % cap] for f < frames.  One launch, no atomics, no allocation,
// no host synchronisation; nothing outside those positions is touched.  Caps as mmd_pcm_to_float (channels * width <= 16384) and as
// mmd_ring_push.  -22 before any launch on null pointers, frames < 1, channels < 1, another width, channels above the cap,
// frames > cap, pos < 0, or cap / pos above 2^50.
int mmd_ring_push_pcm(const unsigned char* pcm, long long frames, int channels, int width, float* ring, long long cap, long long pos, hipStream_t stream);

// Resampling for a live session whose source is not at 44.1 kHz (AudioDetector.open_stream(sample_rate=R); upstream resamples whole
// files with librosa.load(path, sr=44100), mp3_to_pkl.py:31): mmd_resample_poly's rule from a ring into a ring.  in_ring[channels,
// in_cap] holds the input-rate samples as the two writers above leave them, absolute input sample p at in_ring[c * in_cap + p % cap]
// with cap = in_cap; n_valid = input samples pushed so far.  The outputs t_lo .. t_hi-1 (absolute, at the output rate) are stored at
// out_ring[c * out_cap + t % cap] with cap = out_cap - the ring mmd_melspec_windows_ring reads.  bank, phase_off, L, M, taps as
// mmd_resample_poly takes them (the same DEVICE tables, the same caller's duty):
//   y[t] = sum_{j < taps} bank[j * L + r] * x[n + j - taps / 2 + 1],  t = q * L + r,  n = q * M + phase_off[r],
// acc = 0, then acc = fmaf(w, x, acc) for j = 0 .. taps-1 over ALL taps; x[i] enters as 0.f for i < 0 and for i >= n_valid (multiplied,
// not skipped), so every output has bit for bit the value mmd_resample_poly gives it for a recording of n_valid samples whose tail
// is in the ring - once its last input (t * M) / L + taps / 2 has been pushed, for any n_valid; before that, the value for the
// recording that ENDS at n_valid (what a flush wants).  One tile body with that kernel (csrc/resample_tile.h).  [t_lo, t_hi) need not
// be period-aligned: outputs outside it are masked.  Both moduli are taken on the host once; loads and stores wrap with one compare
// and one subtract (t_hi - t_lo <= out_cap: a store wraps once), the device divides nothing and only q * M, q * L and the row offsets
// are 64-bit.  One launch, plain vector stores, no atomics, no allocation, no host synchronisation; nothing outside those t_hi - t_lo
// slots per channel is written, nothing outside in_ring is read, two calls give the same bits.  That no input the range needs has
// been overwritten is checked as far as the host can: the range's oldest input, (t_lo * M) / L - taps / 2 + 1, must be at or behind
// n_valid - in_cap (a negative index counts like any other: a range that starts before the recording needs that much room).  Caps: channels <= 65535, L, M, taps as mmd_resample_poly, in_cap, out_cap, n_valid, t_hi <= 2^50, in_cap >=
// mmd_ring_resample_span(L, M, taps), the least input span a block stages.  -22 before any launch on null pointers, channels outside
// 1 .. 65535, L or M outside 1 .. 1024, taps odd or outside 2 .. 4096, in_cap < 1, out_cap < 1, n_valid < 0, t_lo < 0, t_hi <= t_lo,
// t_hi - t_lo > out_cap, a cap or position above 2^50, in_cap below the staged span, or an oldest input that is no longer in the ring.
int mmd_ring_resample(const float* in_ring, long long in_cap, int channels, long long n_valid, const float* bank, const int* phase_off, int L, int M, int taps, float* out_ring, long long out_cap, long long t_lo, long long t_hi, hipStream_t stream);

// The least in_cap mmd_ring_resample takes for L, M, taps: the input span (floats per channel) of a block of ONE period, taps + the
// phase offsets' spread inside a tile of <= 64 phases (at most M).  A block stages as many periods as fit in min(in_cap, 12288)
// floats, so a small ring costs blocks, never bits.  Host only, no launch; -22 on L or M outside 1 .. 1024, taps odd or outside 2 .. 4096.
int mmd_ring_resample_span(int L, int M, int taps);

// ---- one round of chunks of a BANK of sessions (csrc/live.hip, LiveBank.push_all): the ring writers and the ring resampler above for
// several rings in ONE launch each, driven by a table of descriptors in DEVICE memory (the number of entries varies per call).  The
// caller builds the table on the host, uploads it - in the same copy as the chunks - and hands over both: h_desc, the host copy, which
// the wrapper checks and sizes the grid from, and d_desc, the device copy, which the blocks read (that the two agree, and that the
// upload is ordered in front of the launch on `stream`, is the caller's duty).  blockIdx.z names the entry, the grid covers the largest
// entry, and a block outside its own entry's range returns before it touches memory.
//
// mmd_rings_push: entry e does what one mmd_ring_push / mmd_ring_push_pcm call does.  A descriptor is 64 bytes, eight int64:
//   {src_off, src_stride, n, kind, ring, cap, p0, 0} - the chunk lies src_off BYTES behind src_base (float rows: a multiple of 4, and
//   src_base 4-byte aligned); src_stride: floats between two channels' rows (float rows; >= n); n: samples per channel or frames, 1 .. cap;
//   kind: 0 = float rows [channels, n], 2 / 3 / 4 = interleaved PCM frames of that width; ring: the DEVICE ADDRESS of the destination
//   ring[channels, cap]; p0 = pos % cap, reduced on the host (0 <= p0 < cap).
// Float entries run mmd_ring_push's blocks (1024 samples of one channel, wrap once), PCM entries mmd_ring_push_pcm's (pcm_tile.h: the
// floats are mmd_pcm_to_float's), so ring[c, (pos + i) % cap] gets the bits the single calls give it.  Plain vector stores, no
// atomics, no allocation, no host synchronisation; nothing outside each entry's n slots per channel is touched.  Entries must not
// name overlapping slots of one ring.  -22 before any launch on a null src_base or table, n_desc or channels outside 1 .. 65535, and on
// any entry with a null ring, src_off < 0, n < 1, n > cap, cap > 2^50, p0 outside 0 .. cap-1, another kind, src_stride < n or a
// misaligned float chunk, channels * width above mmd_pcm_to_float's cap.
int mmd_rings_push(const void* src_base, const void* h_desc, const void* d_desc, int n_desc, int channels, hipStream_t stream);

// mmd_rings_resample: entry e does what one mmd_ring_resample call does - its own L, M, taps, bank, phase_off, rings and range, so
// sessions at different rates share the launch.  Grid (max blocks, max phase tiles, channels * n_desc), dynamic LDS the largest span
// among the entries; a block whose tile lies outside its own entry's grid returns before the first barrier.  Staging, tap loop and
// the masked, wrapped stores are mmd_ring_resample's (one tile body), so every output has the bits that call gives it.  A descriptor
// is 192 bytes and is written by mmd_rings_resample_plan alone: the arguments of mmd_ring_resample (addresses as int64) and behind
// them the launch plan made of them.  The wrapper plans every entry of h_desc anew from its arguments and refuses (-22, nothing is
// launched) an entry mmd_ring_resample would refuse - the range whose oldest input has left the ring included - or whose plan is not
// the planner's; also null tables, n_desc < 1 and channels * n_desc > 65535.
int mmd_rings_resample(const void* h_desc, const void* d_desc, int n_desc, int channels, hipStream_t stream);

// Host only, no launch: fills entry `index` (0 .. 65534) of the HOST table h_desc (192 bytes per entry) for mmd_rings_resample from
// the arguments of mmd_ring_resample; in_ring, bank, phase_off and out_ring are device addresses and are not read.  -22, the entry
// untouched, on everything mmd_ring_resample refuses.
int mmd_rings_resample_plan(void* h_desc, int index, const float* in_ring, long long in_cap, int channels, long long n_valid, const float* bank, const int* phase_off, int L, int M, int taps, float* out_ring, long long out_cap, long long t_lo, long long t_hi);

// ---- device-side detection record (csrc/stream.hip): the rows mmd_nms_teacher leaves for a group of windows, appended behind every
// group with one host copy at the end of the recording (the shape of mmd_eval_match's record).
// rows[B, cap_img, 6] / cnt[B]: decode / NMS output (counts are clamped to 0 .. cap_img).  ctl[2] (DEVICE) = {n_valid, first_window}:
// the rows of images 0 .. n_valid-1 are appended at *rec_count in image order, then the NMS output order within an image - the order
// AudioDetector.detect returns - and each appended row i gets rec_win[i] = first_window + image.  Images at or behind n_valid
// contribute nothing, whatever their counts hold (n_valid is clamped to 0 .. B).  rec_rows[rec_cap, 6], rec_win[rec_cap]; *rec_count
// (one device int32) is zeroed by the caller once per stream, and so is *rec_overflow; neither record array needs zeroing.  Offsets
// are an exclusive scan of the B counts inside the kernel (one block, no atomics): two runs give the same record.  *rec_count advances
// by the TRUE total even behind rec_cap: rows that do not fit are not written (nothing behind rec_cap is touched) and *rec_overflow = 1
// (sticky), so the host can say how many rows were needed.  -22 before any launch on null pointers, B < 1, B > 1024, cap_img < 1,
// rec_cap < 1.
int mmd_det_record_append(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, float* rec_rows, int* rec_win, int rec_cap, int* rec_count, int* rec_overflow, hipStream_t stream);

// mmd_det_record_append for a bank of sessions (AudioDetector.open_bank), whose groups mix windows of several recordings: n_valid (one
// DEVICE int32, clamped to 0 .. B) and per-image DEVICE tables win_sess[B], win_idx[B] in place of ctl.  The same scan, order, clamping
// and overflow rule; each appended row i gets rec_win[i] = win_idx[image] and rec_sess[i] = win_sess[image] (rec_sess[rec_cap] int32,
// no zeroing needed; the table's values are copied, not checked).  -22 as mmd_det_record_append.
int mmd_det_record_append_bank(const float* rows, const int* cnt, int B, int cap_img, const int* n_valid, const int* win_sess, const int* win_idx, float* rec_rows, int* rec_win, int* rec_sess, int rec_cap, int* rec_count, int* rec_overflow, hipStream_t stream);

// ---- streaming tracking (csrc/track.hip, AudioDetector.track_stream): links the rows of a group of windows to the tracks of the
// windows before - a greedy IoU tracker with a constant-velocity alpha-beta model, alpha = 1 (the rule: DESIGN.md, streaming tracking;
// tests/track_ref.py restates it in numpy float32 and gives the same bits).  rows / cnt / B / cap_img / ctl as mmd_det_record_append.
// The launch MUST PRECEDE the mmd_det_record_append of the same group on the same stream: it reads the *rec_count the append is
// about to advance (never writes it), does the same clamped exclusive scan of cnt[0 .. n_valid-1] and writes rec_track[offset + j]
// (int32: the row's track id, -1 = none) for every row the append will write at rec_rows[offset + j]; rows behind rec_cap are not
// written.  Windows run in order first_window, first_window + 1, ..; a window without rows ages the tracks.  Counts behind n_valid,
// negative and huge counts are clamped or ignored as the append does; nothing behind cnt[i] rows of image i is read.
// State, caller-owned: trk_slots int32 [max_tracks, 16], one slot per row, words 0 live (0 = free), 1 id, 2..5 x1 y1 x2 y2 (float bits),
// 6 7 vx vy (pixels per window), 8 label (float bits), 9 score, 10 hits, 11 misses, 12 last_window, 13..15 unused (never read or
// written); a freed slot's words 0..12 are zeroed.  trk_glob int32 [2] = {next_id, overflow}.  A ZERO FILL of both RESETS the tracker
// (ids start at 0 again); between the groups of one recording they are left alone.  rec_track and the record arrays need no zeroing.
// Overflow: at most 256 detections of a window take part - the first 256 in NMS output order; later rows get -1 - and an unmatched
// detection that finds no free slot among max_tracks gets -1; either sets trk_glob[1] = 1 (sticky: only a zero fill clears it).
// max_tracks 1 .. 256; a track is freed once it was missed more than max_age windows in a row; pairs need equal labels and
// iou >= iou_min; an unmatched detection starts a track when score >= birth_score (comparisons are false for NaN).
// One block of 256 threads, no atomics: two runs give the same bits.  -22 before any launch on null pointers, B < 1, B > 1024,
// cap_img < 1, rec_cap < 1, max_tracks outside 1 .. 256, max_age < 0.
int mmd_track_update(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, const int* rec_count, int rec_cap, int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age, float birth_score, hipStream_t stream);

// mmd_track_update for a bank of sessions (AudioDetector.open_bank): one tracker per session, trk_slots int32 [n_sessions, max_tracks,
// 16] and trk_glob int32 [n_sessions, 2], each session's part as mmd_track_update describes it (a zero fill of session s's part resets
// that session alone).  n_valid / win_sess[B] / win_idx[B] as mmd_det_record_append_bank, whose launch for the same group this one
// MUST PRECEDE.  One 256-thread block per session: block s walks the rows i < n_valid in row order and runs the per-window body of
// mmd_track_update (ONE __device__ function for both kernels: one rule, one rounding) for those with win_sess[i] == s, with
// win_idx[i] as the window's index (`last_window`); a session's windows must come in rising order across and inside groups.  So
// session s's state and ids are what mmd_track_update leaves after the same windows alone.  Record offsets are the clamped exclusive
// scan over ALL rows on top of *rec_count, computed by every block; the blocks write disjoint parts of rec_track.  A session with no
// row in the group is not touched: no word of its state changes, nothing ages.  A row whose session is outside 0 .. n_sessions-1
// (the CALLER'S ERROR) is tracked by no block and its rec_track entries are not written.  No atomics, plain vector stores.  -22 as
// mmd_track_update, and on n_sessions outside 1 .. 65535.
int mmd_track_update_bank(const float* rows, const int* cnt, int B, int cap_img, const int* n_valid, const int* win_sess, const int* win_idx, int n_sessions, const int* rec_count, int rec_cap, int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age, float birth_score, hipStream_t stream);

// mmd_track_update with the association rule as an argument (TrackConfig(assign=...)): assign 0 = greedy - the launch is the very
// kernel mmd_track_update launches -, 1 = optimal, anything else -22.  Every other argument, the state, the offsets, the overflow rule
// and the refusals are mmd_track_update's.  The OPTIMAL rule replaces the greedy pairing and nothing else (predict, matched-slot update,
// ageing and freeing, births and the rows' ids stay, with their rounding): T = the live slots in rising order after the predict step,
// D = the first min(n, 256) detections of the window; iou[t][d] = the float32 IoU of the greedy step with every operation rounded on
// its own (tests/track_ref.iou_matrix bit for bit); a pair is ALLOWED when the labels are equal and iou >= iou_min (false for NaN);
// W[t][d] = (double)iou[t][d] on allowed pairs and 0 elsewhere (a NaN IoU weighs 0).  The matching of MAXIMUM WEIGHT sum W is taken -
// maximum weight, not maximum cardinality: scipy.optimize.linear_sum_assignment(W, maximize=True) with the pairs that are not allowed
// dropped, float64 on the float32 IoUs as the "assign" step of mmd_mot_clear - and every pair of it is a match: all matched slots
// update from their own prediction, so their order does not matter.  Where two matchings tie, which one is taken is unspecified.  No
// live slot, no detection or no allowed pair: nothing is matched.  tests/track_assign_ref.py restates it.  The solver is mot_assign
// (csrc/mot_assign.h, shared with the tracking evaluation), run on the slots and detections that have an allowed pair at all; should it
// ever find no column (it cannot for finite costs) the window matches nothing and trk_glob[1] = 1.  One block of 256 threads, no
// atomics, no workspace: two runs give the same bits.
int mmd_track_update_assign(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, const int* rec_count, int rec_cap, int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age, float birth_score, int assign, hipStream_t stream);

// mmd_track_update_bank with the association rule as an argument: assign as mmd_track_update_assign (0: the kernel
// mmd_track_update_bank launches), everything else as mmd_track_update_bank.
int mmd_track_update_bank_assign(const float* rows, const int* cnt, int B, int cap_img, const int* n_valid, const int* win_sess, const int* win_idx, int n_sessions, const int* rec_count, int rec_cap, int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age, float birth_score, int assign, hipStream_t stream);

// ---- tracking evaluation (csrc/moteval.hip, mm_distillnet_amd/mot.py): the CLEAR-MOT counts and the identity measures of a tracked
// hypothesis record against a ground-truth record (the rule: DESIGN.md, tracking evaluation; tests/mot_ref.py restates it in numpy /
// scipy).  Both records as the host wrapper prepares them: rows float32 [n, 6] (x1, y1, x2, y2, score, label) sorted stably by
// (session, window); track int32 [n], DENSE ids 0 .. tracks_of_the_session-1 per session and side (hypothesis: -1 = no track; such a
// row can never be paired); off int32 [n_sessions * n_windows + 1]: the rows of window w of session s are off[s * n_windows + w] ..
// off[s * n_windows + w + 1] - 1.  At most 256 rows of one side in one window take part (the first 256; the HOST refuses more);
// offsets are clamped into 0 .. n, so nothing outside the arrays is read.  A pair is allowed when the labels are equal and
// iou >= iou_min (false for NaN), the IoU being the tracker's float32 expression with every operation rounded on its own
// (mmd_box_iou of csrc/moteval.hip = tests/track_ref.iou_matrix bit for bit).
//
// Bytes of mmd_mot_clear's `ws` for n_gt_tracks ground-truth tracks over all sessions (never 0).  -22 for a negative count or one
// above 2^27 - 1.
int mmd_mot_clear_ws_bytes(long long n_gt_tracks);

// CLEAR: one 256-thread block per session walks windows 0 .. n_windows-1 in order.  Per window: KEEP (a ground-truth row whose track
// was last paired with hypothesis track h keeps h when h has a row in the window, that row is free and the pair is allowed; rows in
// row order), ASSIGN (the maximum-weight matching of the allowed pairs among the rows left, weight = IoU, by the shortest augmenting
// path algorithm in float64; where two matchings tie, which one is taken is unspecified), COUNT.  gt_trk_off int32 [n_sessions + 1]:
// session s owns ground-truth tracks gt_trk_off[s] .. gt_trk_off[s + 1] - 1 of the per-track arrays; n_gt_tracks = gt_trk_off[n_sessions].
// Outputs: counts int64 [n_sessions, 8] = {n_gt, n_hyp, tp, fp, fn, idsw, frag, windows walked}; iou_sum double [n_sessions] (the sum of
// the pairs' IoUs; the order of the sum is fixed); present / matched int32 [n_gt_tracks]: windows in which the track has a row / a
// paired row.  ws: mmd_mot_clear_ws_bytes(n_gt_tracks) bytes, 8-byte aligned: per track {map, state}.  counts, iou_sum, present,
// matched and ws need no zeroing: every block initialises its session's part.  A ground-truth row whose id is outside its session's
// range (the CALLER'S ERROR) is never paired and counts as a miss.  No atomics: two runs give the same bits.  -22 before any launch on
// null pointers (a null row / track array with a row count of 0 is allowed), negative counts, counts that do not fit an int,
// n_sessions outside 1 .. 65535, n_windows < 1, n_sessions * n_windows >= 2^31 - 1.
int mmd_mot_clear(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows, const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows, const int* gt_trk_off, long long n_gt_tracks, float iou_min, long long* counts, double* iou_sum, int* present, int* matched, void* ws, hipStream_t stream);

// Identity, step 1: C[g][h] += 1 for every window in which a row of ground-truth track g and a row of hypothesis track h (>= 0) form
// an allowed pair.  One block per (window, session); integer atomicAdd, so the sums do not depend on the order of arrival.  C int32:
// session s's matrix [G_s, H_s] (G_s = gt_trk_off[s + 1] - gt_trk_off[s], H_s likewise from hyp_trk_off int32 [n_sessions + 1]), row
// major, at C + c_off[s] (c_off int64 [n_sessions]); c_total = the ints C holds.  The CALLER ZEROES C.  A session whose matrix does not
// lie inside C, and a row whose id is outside its session's range, add nothing.  max_tracks: the largest G_s or H_s.  -22 as
// mmd_mot_clear, and on c_total < 1, max_tracks outside 1 .. 1024 (the capacity of the identity measures).
int mmd_mot_id_counts(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows, const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows, const int* gt_trk_off, const int* hyp_trk_off, int max_tracks, const long long* c_off, long long c_total, float iou_min, int* C, hipStream_t stream);

// Identity, step 2: idtp int64 [n_sessions] = the weight of the maximum-weight matching of session s's C (the routine of mmd_mot_clear,
// one block per session; integer weights, so the float64 arithmetic is exact and ties do not matter); 0 for a session without tracks on
// either side, -1 for a session whose G_s or H_s is above 1024 or whose matrix does not lie inside C (the CALLER'S ERROR).  idtp needs
// no zeroing.  -22 before any launch on null pointers, n_sessions outside 1 .. 65535, c_total < 1, max_tracks outside 1 .. 1024.
int mmd_mot_id_assign(const int* C, const long long* c_off, long long c_total, const int* gt_trk_off, const int* hyp_trk_off, int n_sessions, int max_tracks, long long* idtp, hipStream_t stream);

// ---- HOTA (Luiten et al., IJCV 2021) of the same two records, in three passes (the rule: DESIGN.md, tracking evaluation, HOTA;
// tests/hota_ref.py restates it).  Records, offsets, gt_trk_off / hyp_trk_off, c_off / c_total (the cell layout of the identity
// matrix: session s's cell (g, h) is c_off[s] + g * H_s + h) and max_tracks as above.  Hypothesis rows with track -1 take no part.
// s(i, j) = mmd_box_iou (float32) of a ground-truth row and a hypothesis row of one window when the labels are equal, else 0;
// q(x) = floor(double(x) * 2^32 + 0.5); thresholds alpha_k = float32((k + 1) / 20), k = 0 .. 18; bins(s) = the number of k with
// s >= alpha_k.  gc int32 [n_gt_tracks] / tc int32 [n_hyp_tracks]: the rows of each track, at gt_trk_off[s] + g / hyp_trk_off[s] + h.
// Everything accumulated is an integer added with integer atomics, so two runs give the same bits.  Every entry point returns -22
// before any launch, without touching the device, on: null pointers (a null row / track array with a row count of 0 is allowed),
// the size errors of mmd_mot_clear, n_windows > 2^20 (P must stay below 2^52), c_total < 1 or 19 * c_total > 2^28, max_tracks outside
// 1 .. 1024, track counts that are negative or above 2^27 - 1.
//
// Pass 1, alignment: one 256-thread block per (window, session).  R_i = sum_j q(s(i, j)), C_j = sum_i q(s(i, j)); every pair with
// q(s) > 0 adds q(double(q(s)) / double(R_i + C_j - q(s))) to P[cell(g, h)], g and h the rows' tracks.  P unsigned 64-bit [c_total].
// The CALLER ZEROES P.  A session whose cells do not lie inside P adds nothing.
int mmd_hota_align(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows, const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows, const int* gt_trk_off, const int* hyp_trk_off, int max_tracks, const long long* c_off, long long c_total, unsigned long long* P, hipStream_t stream);

// Pass 2, matching: one block per (window, session).  score(i, j) = gas(g, h) * double(s(i, j)) in float64, gas = double(P) /
// (2^32 * double(gc + tc) - double(P)); ONE maximum-score assignment of the window's rows (the routine of mmd_mot_clear on
// cost = -score; where two assignments tie, which one is taken is unspecified).  Every assigned pair with b = bins(s) > 0 adds 1 to
// hist[cell(g, h) * 19 + b - 1], and for every k < b 1 to tp[s * 19 + k] and q(s) to loc[s * 19 + k].  hist int32 [c_total * 19],
// tp int64 [n_sessions, 19], loc unsigned 64-bit [n_sessions, 19].  The CALLER ZEROES hist, tp and loc.  P, gc and tc are read only.
int mmd_hota_match(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows, const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows, const int* gt_trk_off, const int* hyp_trk_off, int max_tracks, const long long* c_off, long long c_total, const unsigned long long* P, const int* gc, long long n_gt_tracks, const int* tc, long long n_hyp_tracks, int* hist, long long* tp, unsigned long long* loc, hipStream_t stream);

// Pass 3, association: one block per session.  For each of the session's cells mc[k] = hist[cell][k] + .. + hist[cell][18]; num double
// [n_sessions, 19, 3] = per k the sums over the cells with mc > 0 of mc * mc / (gc + tc - mc), mc * mc / gc, mc * mc / tc (float64; a
// strided loop over the cells and a fixed reduction tree, no atomics: two runs give the same bits).  num needs no zeroing: every
// block writes its session's 57 values, zeros for a session without cells or whose tables do not lie inside hist / gc / tc.
int mmd_hota_assoc(const int* hist, const long long* c_off, long long c_total, const int* gt_trk_off, const int* hyp_trk_off, const int* gc, long long n_gt_tracks, const int* tc, long long n_hyp_tracks, int n_sessions, int max_tracks, double* num, hipStream_t stream);


// ---- data-parallel exchange (RCCL over xGMI), SURVEY.md section 8b.  Replaces DistributedDataParallel's gradient reduction
// (src/optimization/train_methods.py:944-961): student gradients only, sum (the 1/N average rides in the optimizer pass), plus the
// MAX-reduce of head_active.  librccl is opened lazily: -38 when it is not installed.
// mmd_comm_unique_id: 128-byte rendezvous token made on rank 0 and handed to every rank by the host.
int mmd_comm_unique_id(void* out128);
int mmd_comm_init(void** comm_out, int rank, int world, const void* unique_id128);
// In place, asynchronous on `stream`; dtype 0 = float32, 1 = int32; op 0 = sum, 1 = max.
int mmd_comm_allreduce_bucket(void* comm, void* buf, long long count, int dtype, int op, hipStream_t stream);
// ranks RCCL reports for the communicator (ncclCommCount) -> *(int*)count_out
int mmd_comm_count(void* comm, void* count_out);
int mmd_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif
