/*
 * hybrid_hip.h -- C ABI of libhybrid_hip.so, the MI355X (gfx950) implementation of
 * the CNN + temporal-transformer hot path (forward and backward).
 *
 * The reference (spygaurad/Transformer-CNN-Hybrid-Network-for-Video-Processing) has NO
 * native / FFI interface: every op on its hot path is a stock torch.nn call made from
 * nn.Module.forward.  Each entry point below therefore replaces
 * the torch dispatch the cited reference line makes; INTEGRATION.md shows the ctypes
 * binding a maintainer adds on the Python side.
 *
 * Contract:
 *   - extern "C", plain pointers and sizes only; no torch types.
 *   - the CALLER owns every buffer (inputs, outputs, saved activations, workspace);
 *     the library never allocates or frees device memory.  Process-global state is limited to
 *     (i) the optional measurement hooks of hyb_profile_set (off unless set; measurement runs only),
 *     (ii) per-kernel "dynamic-LDS attribute already set on device d" bitmasks (lock-free, idempotent) and
 *     (iii) the HYB_* debug switches, each read from the environment once.
 *     None of it depends on the data or changes results.
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*) and
 *     returns immediately; no internal synchronisation; re-entrant (concurrent calls from several host threads
 *     and on several devices are allowed).
 *   - return value: 0 = success; negative = argument check failed (HYB_E_*);
 *     positive = hipError_t from a launch.  Nothing throws across the ABI.
 *   - `dtype` selects the storage/MFMA-operand type T of activations:
 *       HYB_F32  : fp32 storage, v_mfma_f32_16x16x4_f32 (exact fp32; the parity gate)
 *       HYB_BF16 : bf16 storage, v_mfma_f32_16x16x32_bf16, fp32 accumulate/statistics
 *     A second build of the SAME sources and the SAME ABI, libhybrid_hip_x3.so (-DHYB_F32_X3), gives HYB_F32 a third meaning: fp32
 *     storage, every contraction product from three bf16 MFMAs on two-term splits (x = hi + lo; csrc/hyb_common.h) -- within 1e-5 of the
 *     exact mode at 1.8 x its speed.  The Python host side selects it with compute_dtype="bf16x3" (_lib.py routes by library).
 *     Parameters (weights, biases, BN/LN affine, running stats) and parameter
 *     gradients are always fp32.
 *   - internal activation layout is NHWC with the channel count padded to a multiple
 *     of 32 ("Cp"); padded channels hold zeros.  The user-facing clip tensor stays
 *     NCHW fp32 ([B*T, C, H, W]) and is read directly by the first conv stage.
 */
#ifndef HYBRID_HIP_H_
#define HYBRID_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HYB_F32 0
#define HYB_BF16 1
/* May be OR-ed into the `dtype` of hyb_temporal_{fwd,bwd} / hyb_temporal_ce_{fwd,bwd} when dtype is HYB_F32: the last pooled map `h` (and its
 * gradient `dh`) is bf16 although the temporal part stores and computes in fp32 -- the "mixed" mode of the host side (bf16 conv stages,
 * fp32 / split-bf16 temporal part): the global-average-pool kernels read / write the other type, no cast launches.  Workspace / saved-size
 * queries take the plain dtype. */
#define HYB_H_BF16 0x100

#define HYB_E_ARG (-1)      /* bad argument (null pointer, unsupported size) */
#define HYB_E_WORKSPACE (-2) /* workspace too small */

/* ---- misc ------------------------------------------------------------------------- */
int hyb_abi_version(void);
/* bytes per element of dtype (4 or 2); HYB_E_ARG otherwise */
int hyb_dtype_size(int dtype);
/* round a channel count up to the internal padded count */
int hyb_pad_channels(int c);

/* ---- measurement hook (bench.py): time ONE kernel launch inside a real step with HIP events -----------
 * hyb_profile_set(slot, kernel_id, a, b, ev_start, ev_stop): the next launches of kernel `kernel_id` whose shape key is
 * (a, b) record hipEvent_t ev_start / ev_stop on the launch stream immediately before / after that kernel only.
 *   kernel_id 1: the conv contraction kernel of hyb_conv3x3_fwd -- conv3x3_v2_kernel (bf16, shapes with an asynchronous
 *                variant) or the first-generation conv3x3_nhwc_kernel -- (a = Cip, b = Cop as passed; forward and dgrad launches)
 *   kernel_id 2: the weight-gradient contraction kernel -- wgrad_v3_kernel / wgrad_v2_kernel or the first-generation conv3x3_wgrad_kernel --
 *                (a = Cip, b = Cop)
 *   kernel_id 4: gemm_nt_lds_kernel / gemm_nt_tall_kernel (fewer than 64 columns), the fp32 pixel-side GEMM behind hyb_conv2d_* / hyb_fct_conv_* (a = output columns, b = K as launched)
 *   kernel_id 5: flash_bwd4_dkv_kernel, the dK / dV kernel of FCT's attention backward over narrow heads (a = tokens L, b = heads)
 * slot in [0, 16).  hyb_profile_clear() removes all hooks.  The hook table is never touched unless a hook is set, and it is
 * not thread-safe (measurement runs only). */
int hyb_profile_set(int slot, int kernel_id, int a, int b, void* ev_start, void* ev_stop);
int hyb_profile_clear(void);

/* layout conversion helpers (used by tests and by in_channels > 3):
 * NCHW fp32 [N,C,H,W] <-> NHWC T [N,H,W,Cp] (padded channels written as zero). */
int hyb_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, int H, int W, int Cp, void* stream);
int hyb_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int C, int H, int W, int Cp, void* stream);
/* T <-> fp32 elementwise cast of n elements */
int hyb_cast_to_f32(int dtype, const void* src, float* dst, long long n, void* stream);
int hyb_cast_from_f32(int dtype, const float* src, void* dst, long long n, void* stream);

/* ---- conv stage pieces: replace nn.Conv2d / BatchNorm2d / ReLU / MaxPool2d ----------
 * reference: UNet.py:58 (Conv2d 3x3 pad 1 bias=False), UNet.py:59 (BatchNorm2d),
 * UNet.py:60 (ReLU), UNet.py:13 (MaxPool2d(2,2)).                                      */

/* number of T elements of a packed weight: first ? Cop*32 : Cop*9*Cip */
long long hyb_conv_packed_elems(int first, int Cip, int Cop);
/* w fp32 [Co,Ci,3,3] -> packed T.  mode 0: forward   wp[co][tap][ci]   (Cop x 9 x Cip)
 *                                  mode 1: dgrad     wp[ci][8-tap][co] (Cip x 9 x Cop)
 *                                  mode 2: first layer wp[co][k=tap*Ci+ci] (Cop x 32), Ci<=3 */
int hyb_conv_pack_weight(int dtype, int mode, const float* w, void* wp, int Co, int Ci, int Cop, int Cip, void* stream);

/* y[N,H,W,Cop] = conv3x3(x, wp), stride 1, zero pad 1.
 * first=1: x is NCHW fp32 [N,Ci,H,W] with Ci<=3 (Cip ignored), wp packed with mode 2.
 * first=0: x is NHWC T [N,H,W,Cip], wp packed with mode 0 (or mode 1 for dgrad, with
 *          Cip/Cop exchanged by the caller).
 * stats: NULL, or fp32 [2][Cop] (sum, sum of squares per output channel over N*H*W), overwritten.
 *        Computed from the fp32 accumulators as per-workgroup partial rows in `stats_partials`
 *        (caller workspace of hyb_conv_stats_workspace(Cop) bytes) summed in a fixed order:
 *        bitwise reproducible, no float atomics. */
size_t hyb_conv_stats_workspace(int Cop);
/* number of partial rows hyb_conv3x3_fwd writes for this problem (stats == NULL with stats_partials != NULL leaves only
 * the partial rows: feed them to hyb_bn_stats_finalize) */
int hyb_conv_stats_rows(int first, int N, int H, int W, int Cop);
int hyb_conv3x3_fwd(int dtype, int first, const void* x, const void* wp, void* y, float* stats, float* stats_partials,
                    int N, int H, int W, int Ci, int Cip, int Cop, void* stream);

/* BatchNorm2d statistics -> per-channel scale/shift (UNet.py:59; torch semantics:
 * training: batch mean, biased var for normalisation, running stats updated with
 * momentum and UNBIASED var, num_batches_tracked += 1; eval: running stats).
 * scale_shift fp32 [2][Cop]; mean_invstd fp32 [2][Cop] (saved for backward). */
int hyb_bn_finalize(const float* stats, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, long long* num_batches_tracked, int training, float momentum,
                    float eps, long long count, int Co, int Cop, float* scale_shift, float* mean_invstd,
                    float* running_out /* NULL: update running_mean/var/num_batches_tracked in place (nn.BatchNorm2d semantics);
                                          else fp32 [2][Co] receiving the UPDATED (mean, var) while the inputs stay untouched and
                                          num_batches_tracked is left to the caller (functional form, for torch custom ops) */,
                    void* stream);

/* training-mode shortcut: the same, computed straight from the G per-workgroup partial rows hyb_conv3x3_fwd left in
 * `stats_partials` (fixed-order sum + finalize in one launch).  G = hyb_conv_stats_rows(...). */
int hyb_bn_stats_finalize(const float* stats_partials, int G, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, long long* num_batches_tracked, float momentum, float eps, long long count,
                          int Co, int Cop, float* scale_shift, float* mean_invstd, float* running_out /* as above */, void* stream);

/* pooled[N,H/2,W/2,Cop] = maxpool2x2(relu(y*scale+shift)) (floor; H,W >= 2) */
int hyb_bn_relu_pool_fwd(int dtype, const void* y, const float* scale_shift, void* pooled,
                         int N, int H, int W, int Cop, void* stream);

/* backward of pool+relu+BN, two passes:
 *  reduce: sums[2][Cop] = (sum dy, sum dy*xhat) with dy routed through pool argmax and relu (overwritten; per-block
 *          partial rows summed in a fixed order: reproducible, no float atomics)
 *  dx    : dyraw[N,H,W,Cop] = gamma*invstd*(dy - sum_dy/count - xhat*sum_dyxhat/count) (training)
 *                             gamma*invstd*dy                                        (eval)
 *          and writes dgamma[Co] = sum dy*xhat, dbeta[Co] = sum dy. */
size_t hyb_bn_bwd_reduce_workspace(int Cop);
int hyb_bn_relu_pool_bwd_reduce(int dtype, const void* dpooled, const void* y,
                                const void* pooled /* NULL, or the forward's pooled output [N,H/2,W/2,Cop]: the sums are then formed from it
                                                      (xhat at the arg-max = (pooled - beta)/gamma where pooled > 0) without reading y */,
                                const float* scale_shift, const float* mean_invstd, float* sums, float* partials /* hyb_bn_bwd_reduce_workspace bytes */,
                                float* dgamma /* [Co] or NULL */, float* dbeta /* [Co] or NULL */,
                                int N, int H, int W, int Co, int Cop, void* stream);
int hyb_bn_relu_pool_bwd_dx(int dtype, const void* dpooled, const void* y, const float* scale_shift,
                            const float* mean_invstd, const float* gamma, const float* sums, int training,
                            long long count, void* dyraw, float* dgamma, float* dbeta,
                            int N, int H, int W, int Co, int Cop, void* stream);

/* weight gradient of the conv: dw fp32 [Co,Ci,3,3] = sum_{n,h,w} dy (x) patch(x).
 * x as in hyb_conv3x3_fwd (first selects NCHW fp32 input).  workspace: fp32 partial slabs, summed in a fixed order.
 * dw == NULL leaves only the partial slabs in the workspace (skips the final reduce). */
size_t hyb_conv3x3_wgrad_workspace(int first, int N, int H, int W, int Cip, int Cop);
int hyb_conv3x3_wgrad(int dtype, int first, const void* x, const void* dy, float* dw,
                      int N, int H, int W, int Ci, int Cip, int Co, int Cop,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- whole conv stage (Conv3x3 -> BN -> ReLU -> MaxPool), UNet.py:58-60 + :13 -------- */
size_t hyb_convstage_fwd_workspace(int dtype, int first, int Cip, int Cop);
int hyb_convstage_fwd(int dtype, int first, const void* x, const float* weight, const float* gamma,
                      const float* beta, float* running_mean, float* running_var,
                      long long* num_batches_tracked, int training, float momentum, float eps,
                      int N, int H, int W, int Ci, int Cip, int Co, int Cop,
                      void* y_raw /* [N,H,W,Cop] T, saved */, void* pooled /* [N,H/2,W/2,Cop] T */,
                      float* scale_shift /* [2][Cop] saved */, float* mean_invstd /* [2][Cop] saved */,
                      void* packed_bwd /* NULL, or hyb_convstage_packed_bwd_elems() T elements: weights packed for backward, saved */,
                      float* running_out /* NULL = in-place running statistics; else [2][Co], see hyb_bn_finalize (training only) */,
                      void* workspace, size_t workspace_bytes, void* stream);
long long hyb_convstage_packed_bwd_elems(int first, int Cip, int Cop);
/* The FIRST stage (first = 1) never materialises its raw conv output; its y_raw argument is instead an optional buffer of
 * hyb_convstage_route_elems() T elements (0 = this dtype / shape keeps no codes: pass NULL) that the forward fills with the stage's
 * pooling / ReLU routing decisions (4 bits per pooled element: which pixel of the 2x2 window is the first maximum in torch's scan order,
 * and whether the ReLU passed) and the backward, given the same buffer as y_raw, reads instead of recomputing the convolution to re-derive
 * them.  NULL on either side: the backward recomputes (same results, bit for bit). */
long long hyb_convstage_route_elems(int dtype, int N, int H, int W, int Cop);
size_t hyb_convstage_bwd_workspace(int dtype, int first, int N, int H, int W, int Cip, int Cop);
int hyb_convstage_bwd(int dtype, int first, const void* dpooled, const void* x, const void* y_raw,
                      const void* pooled /* NULL, or the stage's forward output (see hyb_bn_relu_pool_bwd_reduce) */,
                      const float* weight, const float* gamma, const float* scale_shift,
                      const float* mean_invstd, int training,
                      int N, int H, int W, int Ci, int Cip, int Co, int Cop,
                      void* dx /* [N,H,W,Cip] T, NULL when first */, float* dweight, float* dgamma, float* dbeta,
                      const void* packed_bwd /* from hyb_convstage_fwd, or NULL to repack */,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- whole conv stage, INFERENCE (eval-mode BatchNorm; new symbols only, hyb_abi_version() stays 9) ---------------------------------
 * pooled = maxpool2x2(relu(conv3x3(x, weight) * scale + shift)) with scale = gamma * rsqrt(running_var + eps), shift = beta -
 * running_mean * scale (fp32; padded channels exact zeros).  The running statistics are only read, nothing is saved for a backward.
 * bf16 storage, shapes the asynchronous conv kernels take (hyb_conv3x3_pool_fused() == 1): ONE kernel -- the affine, the ReLU and the 2x2
 * maximum are applied to the fp32 accumulators in the conv's epilogue, the raw conv output is never stored and the pooled value is
 * rounded to bf16 once.  Everything else (fp32 storage, other shapes): the conv -> hyb_bn_relu_pool_fwd pair of hyb_convstage_fwd's eval
 * mode with the raw output in the workspace: the same results as hyb_convstage_fwd(training = 0), bit for bit.
 * x / Ci / Cip / first as in hyb_convstage_fwd.  hyb_conv3x3_pool_fused is a pure host query (W = the stage's input width). */
int hyb_conv3x3_pool_fused(int dtype, int W, int Cip, int Cop);
/* hyb_conv3x3_pool_ext: pure host query (new symbol, hyb_abi_version() stays 9).  1 when hyb_convstage_fwd(training = 1) runs a non-first stage
 * of this shape with the 2x2 window extremes stored by the conv's epilogue (no full-resolution re-read for BatchNorm + ReLU + MaxPool);
 * the outputs are the same bit for bit either way. */
int hyb_conv3x3_pool_ext(int dtype, int W, int Cip, int Cop);
/* pure host query: the kernel variant a non-first hyb_conv3x3_fwd of this shape runs, 100 * family + table row (family 0 first-generation rows 0-3, 1 asynchronous ring rows 0-6, 2 k32 rows 0-1: csrc/conv_plan.h) */
int hyb_conv3x3_fwd_variant(int dtype, int N, int H, int W, int Cip, int Cop);
/* pure host query (new symbol, hyb_abi_version() stays 9): the tiles in a workgroup's run of that launch -- the asynchronous kernels are persistent, a workgroup
 * walks ceil(tiles / grid) consecutive tiles -- without (stats = 0: stats_partials == NULL) or with (stats = 1) partial statistics; 0 for the
 * first-generation kernel (one tile per workgroup) and for bad arguments */
int hyb_conv3x3_fwd_run(int dtype, int stats, int N, int H, int W, int Cip, int Cop);
/* pure host query (new symbol, hyb_abi_version() stays 9): the stage-1 twin of hyb_conv3x3_fwd_run.  Every first-stage kernel is persistent; pass =
 * 0 statistics, 1 apply + pool, 2 Gram, 3 backward of hyb_convstage_fwd / hyb_convstage_bwd(first = 1).  > 0: the 8x16-pixel blocks in a WAVE's run
 * (a wave-private kernel serves the pass: wave k of the grid walks blocks [k run, (k + 1) run), row-major inside an image; waves past the last block
 * are idle); < 0: minus the 8x32-pixel tiles in a workgroup's run (the block-level kernel); 0: the pass does not run for this dtype / shape / mode,
 * or an argument is bad.  Assumes 16-byte-aligned tensors; the HYB_S1_* switches as the process reads them. */
int hyb_stage1_run(int dtype, int pass, int training, int N, int H, int W, int Ci, int Cop);
/* pure host query: the non-first weight-gradient kernel of this shape (fused = hyb_convstage_bwd's form), 100 * generation (1, 2, 3) + input channels per workgroup (32, 64) */
int hyb_conv3x3_wgrad_variant(int dtype, int fused, int N, int H, int W, int Cip, int Cop);
size_t hyb_convstage_infer_workspace(int dtype, int first, int N, int H, int W, int Cip, int Cop);
int hyb_convstage_infer(int dtype, int first, const void* x, const float* weight, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var, float eps,
                        int N, int H, int W, int Ci, int Cip, int Co, int Cop,
                        void* pooled /* [N,H/2,W/2,Cop] T */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- frame token: global average pool over H*W (the composite's own glue) ----------- */
int hyb_gap_fwd(int dtype, const void* x /* [N,HW,Cp] */, void* feat /* [N,Cp] */, int N, int HW, int Cp, void* stream);
int hyb_gap_bwd(int dtype, const void* dfeat /* [N,Cp] */, void* dx /* [N,HW,Cp] */, int N, int HW, int Cp, void* stream);

/* ---- nn.Linear: y = x W^T + b (TransformerEncoder.pyc src L12-15, L69, L87, L107) ----
 * x [M,K] T with row stride ldx (elements), W fp32 [N,K], b fp32 [N] or NULL, y [M,N] T.
 * relu=1 applies ReLU in the epilogue (src L70 / the FFN's nn.ReLU). */
int hyb_linear_fwd(int dtype, const void* x, int ldx, const float* W, const float* b, void* y,
                   int M, int N, int K, int relu, void* stream);
/* backward: if relu, dy is first masked by (y > 0) (y = saved forward output).
 * dx [M,K] T (ldx stride; accumulate_dx=1 adds into it), dW fp32 [N,K], db fp32 [N] (both overwritten).
 * dx, dW or db may be NULL to skip.  workspace: M*N T elements (masked dy) when relu. */
int hyb_linear_bwd(int dtype, const void* x, int ldx, const float* W, const void* y, const void* dy,
                   void* dx, int accumulate_dx, float* dW, float* db, int M, int N, int K, int relu,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- attention core: TransformerEncoder.pyc src L49-62 with the head split of L22-45 --
 * q,k,v,out: [B,S,D] T (token-major; head h = feature slice [h*D/H,(h+1)*D/H), batch index
 * b*H+h).  scores = q k^T / sqrt(D) (D = d_model, quirk Q1); mask: NULL or fp32 [B,S,S],
 * row b*H+h uses mask[(b*H+h) % B] (quirk Q4: mask.repeat(H,1,1)); masked_fill(mask==0,-1e9);
 * softmax; dropout(p_drop) on the weights (src L58, counter-based RNG keyed by seed);
 * out = weights v.  Masked scores follow masked_fill in both directions: the VALUE -1e9 enters the softmax (a query whose keys are all
 * masked -- a padded frame under a valid x valid mask, a zero row of a [B,S,1] mask -- attends uniformly, 1/S per key), and NO gradient
 * reaches a masked score: such a query adds nothing to dq or dk, and dv receives 1/S of its dout.  stats: fp32 [B*H,S,2] = (row max, row sum of exp) of the scaled, masked scores -- all the backward needs to
 * recompute the probabilities (the fp32 probability matrix of the first generation is gone); pass the SAME mask, p_drop and seed
 * to the backward call.
 * Limits: S <= 64 (longer sequences: hyb_attention_long_* below; hyb_encoder_* switch by themselves), D/H a multiple of 8, <= 128. */
int hyb_attention_fwd(int dtype, const void* q, const void* k, const void* v, const float* mask,
                      void* out, float* stats, int B, int S, int D, int H, float p_drop,
                      unsigned long long seed, void* stream);
int hyb_attention_bwd(int dtype, const void* q, const void* k, const void* v, const float* mask, const float* stats,
                      const void* dout, void* dq, void* dk, void* dv, int B, int S, int D, int H,
                      float p_drop, unsigned long long seed, void* stream);
/* The same attention() for sequences of ANY length (the reference has no limit on S; TransformerEncoder.pyc src L49-62): online-softmax
 * kernels over 64-key blocks, same scale / mask / dropout semantics as above.  q, k, v: rows at stride ld_qkv elements (D for separate
 * tensors, 3 D for a packed q|k|v row), dq, dk, dv at stride ld_d; out and dout are dense [B*S, D].  lse: fp32 [B*H, S], the
 * log-sum-exp of each query's scaled, masked scores (forward output, backward input, with the forward's `out`).  seed_inc: NULL, or a
 * device counter added to the seed (graph replay).  workspace: hyb_attention_long_workspace bytes.  The core computes on fp32 operands;
 * a bf16 caller's tensors are widened into the workspace and results rounded once.  Limits: D/H a multiple of 8, <= 128; B*H <= 65535. */
size_t hyb_attention_long_workspace(int dtype, int B, int S, int D, int H);
int hyb_attention_long_fwd(int dtype, const void* q, const void* k, const void* v, int ld_qkv, const float* mask, void* out, float* lse,
                           int B, int S, int D, int H, float p_drop, unsigned long long seed, const unsigned long long* seed_inc,
                           void* workspace, size_t workspace_bytes, void* stream);
int hyb_attention_long_bwd(int dtype, const void* q, const void* k, const void* v, int ld_qkv, const float* mask, const void* out,
                           const float* lse, const void* dout, void* dq, void* dk, void* dv, int ld_d, int B, int S, int D, int H,
                           float p_drop, unsigned long long seed, const unsigned long long* seed_inc, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- LayerNorm + residual (+ scale, + dropout): src L116-117 / L120-123 ---------------
 * y = dropout_p( (LayerNorm(x)*gamma + beta + skip) * out_scale ).  stats fp32 [2][M]. */
int hyb_ln_residual_fwd(int dtype, const void* x, const void* skip, const float* gamma, const float* beta,
                        void* y, float* stats, int M, int D, float eps, float out_scale, float p_drop,
                        unsigned long long seed, void* stream);
/* dx, dskip [M,D] T; dgamma/dbeta fp32 [D] are ACCUMULATED into (one LayerNorm instance is
 * applied twice per layer, quirk Q3).  accumulate_dskip=1 adds into dskip. */
int hyb_ln_residual_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* stats,
                        void* dx, void* dskip, int accumulate_dskip, float* dgamma, float* dbeta,
                        int M, int D, float out_scale, float p_drop, unsigned long long seed, void* stream);

/* ---- whole TransformerEncoder.forward(input, mask): src L110-126 ----------------------
 * params: host array of L*14 device pointers (fp32), per layer in this order:
 *   Wq,bq,Wk,bk,Wv,bv,Wo,bo (attention_layers.i.{query,key,value,output}_layer.{weight,bias}),
 *   W1,b1,W2,b2 (feedforward_layers.i.{0,2}.{weight,bias}), ln_w, ln_b (layer_norm.i).
 * grads: same order, fp32, overwritten.  saved: caller buffer of hyb_encoder_saved_bytes.
 * attn_p = attention-weight dropout (0.1 in train mode, 0 in eval: quirk Q5);
 * layer_p = per-layer dropout (always active: quirk Q6).
 * seed_inc: NULL, or a DEVICE pointer to one 64-bit counter that the kernels add to `seed` when they run.  A launch captured
 * in a hipGraph replays with the same by-value `seed`; advancing the counter between replays (any kernel on the stream) gives
 * every replay its own dropout masks.  Pass the same pointer (and value) to the backward call of the same step. */
size_t hyb_encoder_saved_bytes(int dtype, int B, int S, int D, int Hid, int L, int H);
size_t hyb_encoder_workspace_bytes(int dtype, int B, int S, int D, int Hid, int L, int H);
int hyb_encoder_fwd(int dtype, const void* x, const float* mask, const float* const* params, void* out,
                    void* saved, int B, int S, int D, int Hid, int L, int H, float attn_p, float layer_p,
                    unsigned long long seed, const unsigned long long* seed_inc, void* stream);
int hyb_encoder_bwd(int dtype, const void* dout, const float* mask, const float* const* params,
                    float* const* grads, const void* saved, void* dx, int B, int S, int D, int Hid, int L,
                    int H, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Pure host query (new symbol, hyb_abi_version() stays 9).  hyb_gemm_longk: 1 when the encoder's token product C[Mo][No] = A[Mo][R] .
 * B[No][R]^T (bf16 in and out, `groups` products in one launch) runs on the long-K kernel: few-tile products with R >= 1024, i.e. the
 * feed-forward's second Linear, the dX of its first Linear and the dX of the Q|K|V projection when Hid / 3 D reach 1024
 * (HYB_GEMM_LONGK=0: never).  The results are the same bit for bit on either kernel. */
int hyb_gemm_longk(int dtype, int groups, int Mo, int No, int R);

/* ---- head: mean over T then Linear(d, classes) (composite's own) ---------------------- */
int hyb_head_fwd(int dtype, const void* x /* [B,S,D] T */, const float* W /* [C,D] */, const float* b,
                 float* logits /* [B,C] fp32 */, int B, int S, int D, int C, void* stream);
int hyb_head_bwd(int dtype, const void* x, const float* W, const float* dlogits /* [B,C] */,
                 void* dx /* [B,S,D] T */, float* dW, float* db, int B, int S, int D, int C, void* stream);

/* ---- loss: mean cross-entropy over the batch (composite's own) ------------------------
 * A target outside [0, C) (torch raises a device-side assert there) makes the loss and that row of dlogits NaN; nothing is
 * read out of bounds. */
int hyb_cross_entropy_fwd(const float* logits, const long long* target, float* loss /* [1] */,
                          int B, int C, void* stream);
int hyb_cross_entropy_bwd(const float* logits, const long long* target, const float* dloss /* [1] */,
                          float* dlogits, int B, int C, void* stream);

/* hyb_cross_entropy_opts_*: the same loss with torch.nn.functional.cross_entropy's options, reduction "mean" (new symbols, hyb_abi_version()
 *   stays 9).  weight [C] class weights >= 0, or NULL = all ones; has_ignore != 0: clips whose target equals ignore_index (inside or
 *   outside [0, C)) are left out; label_smoothing e in [0, 1].  With keep_b = (target_b != ignore_index), lse_b = logsumexp(logits_b):
 *     term_b = keep_b [ (1 - e) w[y_b] (lse_b - z_b[y_b]) + (e / C) sum_c w[c] (lse_b - z_b[c]) ],
 *     den = sum_b keep_b w[y_b],   loss = (sum_b term_b) / den,
 *     dlogits[b,c] = (dloss / den) keep_b [ (1 - e) w[y_b] (p_bc - [c == y_b]) + (e / C) (p_bc sum_k w[k] - w[c]) ].
 *   den == 0 (every clip ignored, or zero-weight classes only): the loss is NaN and dlogits is all zero.  A kept target outside [0, C)
 *   makes the loss and every kept row of dlogits NaN (rows of ignored clips stay 0); nothing is read out of bounds.  Numerator and den are summed in a fixed tree: results are
 *   reproducible bit for bit.  HYB_E_ARG: a NULL pointer (other than weight), has_ignore not 0 / 1, label_smoothing outside [0, 1]. */
int hyb_cross_entropy_opts_fwd(const float* logits, const long long* target, const float* weight /* [C] or NULL */,
                               long long ignore_index, int has_ignore, float label_smoothing, float* loss /* [1] */, int B, int C,
                               void* stream);
int hyb_cross_entropy_opts_bwd(const float* logits, const long long* target, const float* weight /* [C] or NULL */,
                               long long ignore_index, int has_ignore, float label_smoothing, const float* dloss /* [1] */,
                               float* dlogits, int B, int C, void* stream);

/* hyb_cross_entropy_mix_*: hyb_cross_entropy_opts_* with TWO targets per clip, the labels of a Mixup / CutMix batch (new symbols,
 *   hyb_abi_version() stays 9).  Behind `target`: target_b [B] class indices and lam [B] floats, both read on the device.  With
 *   a_b = target[b], c_b = target_b[b], l_b = lam[b], and term(b, y), d(b, y) = keep w[y] the per-clip term and den share defined above:
 *     num = sum_b [ l_b term(b, a_b) + (1 - l_b) term(b, c_b) ],   den = sum_b [ l_b d(b, a_b) + (1 - l_b) d(b, c_b) ],   loss = num / den,
 *     dlogits[b,c] = (dloss / den) [ l_b r(b, a_b, c) + (1 - l_b) r(b, c_b, c) ],  r the bracket of hyb_cross_entropy_opts_bwd's formula.
 *   Each side keeps the rules above on its own: a target equal to ignore_index drops that side, a kept target outside [0, C) poisons the
 *   loss with NaN.  l_b == 1 does not look at c_b and l_b == 0 does not look at a_b (an out-of-range index there changes nothing); an l_b
 *   outside [0, 1], NaN included, poisons den: the loss is NaN.  den == 0: NaN loss, zero gradient.  The log-sum-exp is formed once per
 *   clip; numerator and den go through the same fixed trees.  lam == 1 everywhere gives hyb_cross_entropy_opts_* bit for bit.  With a
 *   uniform lam, target_b a permutation of target and nothing ignored the loss is lam CE(z, a) + (1 - lam) CE(z, c) of
 *   torch.nn.functional.cross_entropy for any weights and smoothing.  HYB_E_ARG as for the *_opts_* family, and a NULL target_b or lam. */
int hyb_cross_entropy_mix_fwd(const float* logits, const long long* target, const long long* target_b /* [B] */, const float* lam /* [B] */,
                              const float* weight /* [C] or NULL */, long long ignore_index, int has_ignore, float label_smoothing,
                              float* loss /* [1] */, int B, int C, void* stream);
int hyb_cross_entropy_mix_bwd(const float* logits, const long long* target, const long long* target_b /* [B] */, const float* lam /* [B] */,
                              const float* weight /* [C] or NULL */, long long ignore_index, int has_ignore, float label_smoothing,
                              const float* dloss /* [1] */, float* dlogits, int B, int C, void* stream);

/* hyb_cross_entropy_dense_*: the loss on DENSE targets, one fp32 row target[b][0..C) per clip, reduction "mean", fp32 arithmetic (new
 *   symbols, hyb_abi_version() stays 9).  z = logits, t = target, w = weight [C] >= 0 or NULL = all ones, lse_b = logsumexp(z_b).
 *   kind 0, soft-target cross-entropy -- torch.nn.functional.cross_entropy(z, t, weight=w, label_smoothing=e) with class probabilities:
 *     q_bc = (1 - e) t_bc + e / C,   loss = (1 / B) sum_b sum_c w_c q_bc (lse_b - z_bc),
 *     dlogits[b,c] = (dloss / B) (softmax(z_b)_c P_b - w_c q_bc),   P_b = sum_k w_k q_bk.
 *   The divisor is B, not a weight sum (torch's rule for probability targets; the index-target families divide by den).  Rows are used
 *   as given: neither normalised nor range-checked, a NaN propagates.  A one-hot row with no weight and no smoothing gives
 *   hyb_cross_entropy_* bit for bit.
 *   kind 1, binary cross-entropy with logits -- torch.nn.functional.binary_cross_entropy_with_logits(z, t, weight=w, pos_weight=pw),
 *   pw = pos_weight [C] >= 0 or NULL = all ones, in the overflow-safe form (z = +-100 gives a finite loss and gradient):
 *     L_bc = 1 + (pw_c - 1) t_bc,   term_bc = w_c [ (1 - t_bc) z_bc + L_bc (log1p(exp(-|z_bc|)) + max(-z_bc, 0)) ],
 *     loss = (1 / (B C)) sum_bc term_bc,   dlogits[b,c] = (dloss / (B C)) w_c (L_bc sigmoid(z_bc) - pw_c t_bc).
 *   A clip's sum over classes runs in class order, the sum over clips goes through the fixed tree of the other families, the division is
 *   taken once at the end: results are reproducible bit for bit.  HYB_E_ARG, without a launch: a NULL pointer (other than weight and
 *   pos_weight), kind not 0 / 1, label_smoothing outside [0, 1] or non-zero with kind 1, pos_weight given with kind 0. */
int hyb_cross_entropy_dense_fwd(const float* logits, const float* target /* [B,C] */, const float* weight /* [C] or NULL */,
                                const float* pos_weight /* [C] or NULL */, int kind, float label_smoothing, float* loss /* [1] */, int B,
                                int C, void* stream);
int hyb_cross_entropy_dense_bwd(const float* logits, const float* target /* [B,C] */, const float* weight /* [C] or NULL */,
                                const float* pos_weight /* [C] or NULL */, int kind, float label_smoothing, const float* dloss /* [1] */,
                                float* dlogits, int B, int C, void* stream);

/* hyb_cross_entropy_focal_* / hyb_cross_entropy_asym_*: the two focusing losses for imbalanced data, reduction "mean" (new symbols,
 *   hyb_abi_version() stays 9).  fp32 arithmetic throughout; every product that feeds a sum is one fused multiply-add; a clip's sums over
 *   classes run in class order and the sum over clips goes through the fixed 256-leaf tree of the other families: results are reproducible
 *   bit for bit.  Each exponent (gamma, gamma_pos, gamma_neg) must be 0 or >= 1: between 0 and 1 the derivative of base^g is singular at
 *   base == 0, which a clipped negative reaches exactly.  Wherever an exponent is 0, x^0 is taken as 1 and its derivative as 0; x^(g-1) at
 *   g == 1 is 1.  HYB_E_ARG, without a launch: a NULL pointer (other than weight and pos_weight), an exponent that is neither 0 nor >= 1
 *   (NaN and infinity included), clip outside [0, 1).
 *   FOCAL, class-index targets y (Lin et al. 2017, softmax form).  keep_b, w, lse_b, den and the out-of-range / all-ignored rules are
 *   those of hyb_cross_entropy_opts_*; there is no label smoothing.  With mx_b = max_c z_bc, s_b = sum_c exp(z_bc - mx_b), p = softmax(z_b):
 *     u_b = (sum_{c != y} exp(z_bc - mx_b)) / s_b   -- the other classes' probability as that sum, not as 1 - p_y,
 *     term_b = keep_b w[y] u_b^gamma (lse_b - z_by),   loss = (sum_b term_b) / den,
 *     dlogits[b,c] = (dloss / den) keep_b w[y] M_b (p_bc - [c == y]),   M_b = u^gamma + gamma u^(gamma-1) p_y (lse_b - z_by).
 *   gamma == 0 gives hyb_cross_entropy_opts_* with the same weight and ignore_index (label_smoothing 0), loss and gradient bit for bit.
 *   ASYMMETRIC, dense fp32 targets t [B,C] (Ridnik et al. 2021).  With ez = exp(-|z|), sp(x) = log1p(exp(-|x|)) + max(-x, 0),
 *   p = sigmoid(z) and q = sigmoid(-z) in the overflow-safe form of hyb_cross_entropy_dense_* kind 1, m = clip:
 *     logp = -sp(z),   r = max(p - m, 0),   logn = -sp(-z) if m == 0, else log(min(q + m, 1)),
 *     base = t q + (1 - t) r,   g_t = gamma_pos t + gamma_neg (1 - t),   L = 1 + (pw_c - 1) t,
 *     cell_bc = -w_c L base^g_t (t logp + (1 - t) logn),   loss = (1 / (B C)) sum_bc cell_bc,
 *   the clip's sum formed as fma(-(w_c L), base^g_t (t logp + (1 - t) logn), sum) over c.  dlogits is (dloss / (B C)) times the derivative
 *   of exactly this expression, the focusing factor included: d r / dz = p q where p > m, else 0; d logn / dz = -p for m == 0, else
 *   -p q / min(q + m, 1) where p > m, else 0.  Soft rows are used as given (their per-cell exponent g_t may then fall between 0 and 1); a
 *   NaN propagates.  gamma_pos == gamma_neg == g with m == 0, w = 1 - alpha and pw = alpha / (1 - alpha) is the sigmoid focal loss with
 *   reduction "mean"; all three 0 is kind-1 BCE in value (another form of the same number: not bit for bit).  z = +-100 gives a finite
 *   loss and gradient. */
int hyb_cross_entropy_focal_fwd(const float* logits, const long long* target, const float* weight /* [C] or NULL */, long long ignore_index,
                                int has_ignore, float gamma, float* loss /* [1] */, int B, int C, void* stream);
int hyb_cross_entropy_focal_bwd(const float* logits, const long long* target, const float* weight /* [C] or NULL */, long long ignore_index,
                                int has_ignore, float gamma, const float* dloss /* [1] */, float* dlogits, int B, int C, void* stream);
int hyb_cross_entropy_asym_fwd(const float* logits, const float* target /* [B,C] */, const float* weight /* [C] or NULL */,
                               const float* pos_weight /* [C] or NULL */, float gamma_pos, float gamma_neg, float clip, float* loss /* [1] */,
                               int B, int C, void* stream);
int hyb_cross_entropy_asym_bwd(const float* logits, const float* target /* [B,C] */, const float* weight /* [C] or NULL */,
                               const float* pos_weight /* [C] or NULL */, float gamma_pos, float gamma_neg, float clip,
                               const float* dloss /* [1] */, float* dlogits, int B, int C, void* stream);

/* hyb_eval_metrics: the update of an accumulating classification meter, ONE launch of one 256-thread workgroup behind the logits (new
 *   symbol, hyb_abi_version() stays 9).  It ADDS into sums, counts and confusion and overwrites none of them: repeated launches, and
 *   replays of a graph that holds the launch, accumulate; the caller zeroes the three before the first.  Launches on one stream are ordered
 *   and one thread makes the final add, so there is no floating-point atomic and the sums are reproducible bit for bit.  Never synchronises.
 *   Each of the B videos has V = views rows of logits, adjacent (row b * V + v).  Its scores s [C] are
 *     V == 1: the logits;   V > 1: pbar_c = (1 / V) sum_v softmax(z_v)_c, formed in fp32 and written to scores[b].
 *   Loss, with the options of hyb_cross_entropy_opts_* (keep, w, e as defined there):
 *     V == 1: term_b and the den share w[y_b] are the criterion's own per-clip functions, so sums[0] / sums[1] is its arithmetic;
 *     V > 1:  term_b = keep_b [ (1 - e) w[y_b] (-log pbar_y) + (e / C) sum_c w[c] (-log pbar_c) ], the same den share.
 *     Terms are fp32; numerator and den are summed in double over a fixed 256-leaf tree and added once to sums[0] and sums[1].
 *   Prediction and rank (torch leaves ties open; these are this library's rules):
 *     pred = the LOWEST index among the maxima of s;   rank = #{c : s_c > s_y} + #{c < y : s_c == s_y};
 *     top-1 correct iff rank == 0 (iff pred == y), top-k correct iff rank < topk.
 *   counts: [0] videos seen (B), [1] kept, [2] top-1 correct, [3] top-k correct, [4] kept videos whose scores hold a NaN.
 *   A video whose target equals ignore_index (has_ignore set) counts in [0] and nowhere else and contributes nothing (pred is still
 *   written).  A video whose scores hold a NaN gets pred = -1, is wrong for both accuracies, has no confusion entry and, when kept,
 *   counts in [4]; its loss term is the NaN the loss functions give.  A kept target outside [0, C) makes both sums NaN as in the
 *   criterion, counts as kept and as wrong, and neither touches confusion nor reads weight out of bounds.
 *   confusion [C*C] (row = target, column = prediction; 64-bit integer adds, which commute) may be NULL, as may pred [B]; scores [B, C] is
 *   required when V > 1 and optional otherwise (V == 1: a copy of the logits).
 *   HYB_E_ARG, before any HIP call: a NULL logits, target, sums or counts; B < 1, C < 1, views < 1; topk outside [1, C]; label_smoothing
 *   outside [0, 1]; has_ignore not 0 / 1; views > 1 without scores. */
int hyb_eval_metrics(const float* logits /* [B*V, C] */, const long long* target /* [B] */, const float* weight /* [C] or NULL */,
                     long long ignore_index, int has_ignore, float label_smoothing, int topk, int views,
                     double* sums /* [2] */, long long* counts /* [5] */, long long* confusion /* [C*C] or NULL */,
                     long long* pred /* [B] or NULL */, float* scores /* [B, C] or NULL */, int B, int C, void* stream);

/* hyb_eval_multilabel: the update of an accumulating MULTI-LABEL meter, ONE launch of one 256-thread workgroup behind the logits (new
 *   symbol, hyb_abi_version() stays 9).  Like hyb_eval_metrics it ADDS into sums, counts and cells and overwrites none of them, thread t
 *   owns videos t, t + 256, .., the loss is summed in double over the fixed 256-leaf tree and one thread makes the final add: no
 *   floating-point atomic, sums reproducible bit for bit, never synchronises.  The caller zeroes sums, counts and cells before the first.
 *   Each of the B videos has V = views rows of logits, adjacent (row b * V + v), and one fp32 target row t_b [C].
 *   Scores, with the overflow-safe sigmoid of the BCE gradient, ez = exp(-|z|), sg(z) = (z >= 0 ? 1 : ez) / (1 + ez):
 *     V == 1: s_c = sg(z_c);   V > 1: s_c = (1 / V) sum_v sg(z_vc), summed in view order in fp32.  Always written to scores[b].
 *   Loss term, fp32 per video, added into sums[0] in double (the meter reports sums[0] / (videos C)):
 *     V == 1: the BCE-with-logits term of hyb_cross_entropy_dense_* (kind 1) on (z_b, t_b, weight, pos_weight): the criterion's function;
 *     V > 1:  term_b = sum_c w_c [ pw_c t_c (-L(s_c)) + (1 - t_c) (-L1(s_c)) ],  L(p) = max(log(p), -100),  L1(p) = max(log1p(-p), -100)
 *             (torch.nn.functional.binary_cross_entropy's clamp; a NaN passes through it), in class order, every product that feeds a
 *             sum an explicit fma.
 *   Labels and predictions: y_c = (t_c >= 0.5), so a NaN target is a negative label (its loss term is what the arithmetic gives);
 *     pred_c = (s_c >= threshold[c]) on the fp32 score that was written;  cells[c] = {tp, fp, fn} (64-bit integer adds, which commute).
 *   counts: [0] videos seen (B), [1] videos whose scores hold a NaN, [2] exact matches (pred_c == y_c for every c), [3] rows stored in the
 *     bank (the cursor), [4] rows dropped.
 *   A video whose scores hold a NaN counts in [1], predicts negative for every class (its positive labels become fn), is never an exact
 *   match, is stored in the bank with score -inf in every class (it ranks last), and its loss term is the NaN the arithmetic gives.
 *   Score bank (mean average precision needs every score of the validation set): when both bank pointers are given, video b of this launch
 *   goes to row r = counts[3] + b if r < capacity: its fp32 scores to bank_scores[r] and its labels y (0 / 1) to bank_labels[r].  Every
 *   thread reads the cursor before the reduction's first barrier; after the tree thread 0 alone writes counts[3] = min(cursor + B, capacity)
 *   and counts[4] += the rows that did not fit.  No atomics, the row order is the arrival order, a replayed graph appends (the cursor
 *   lives on the device), and nothing is ever written at or beyond `capacity`.  Without a bank counts[3] and counts[4] are left as they are.
 *   pred [B, C] (0 / 1) may be NULL.  The inputs (logits, target, weight, pos_weight, threshold) are only read and must not overlap
 *   anything the launch writes.
 *   HYB_E_ARG, before any HIP call: a NULL logits, target, threshold, sums, counts, cells or scores; B < 1, C < 1, views < 1,
 *   capacity < 0; exactly one of the two bank pointers given; a bank given with capacity == 0; B * views or views * C beyond int. */
int hyb_eval_multilabel(const float* logits /* [B*V, C] */, const float* target /* [B, C] */,
                        const float* weight /* [C] or NULL */, const float* pos_weight /* [C] or NULL */,
                        const float* threshold /* [C] */, int views,
                        double* sums /* [1] */, long long* counts /* [5] */, long long* cells /* [C, 3] */,
                        float* bank_scores /* [capacity, C] or NULL */, unsigned char* bank_labels /* [capacity, C] or NULL */,
                        long long capacity,
                        unsigned char* pred /* [B, C] or NULL */, float* scores /* [B, C] */,
                        int B, int C, void* stream);

/* hyb_eval_metrics_focal / hyb_eval_metrics_soft / hyb_eval_multilabel_asym: the two meters' updates under the other criteria the library
 *   trains with (new symbols, hyb_abi_version() stays 9).  Each is the launch of hyb_eval_metrics / hyb_eval_multilabel with another loss
 *   term: ONE 256-thread workgroup, thread t owns videos t, t + 256, .., fp32 terms summed in double over the fixed 256-leaf tree, one thread
 *   makes the final add (no floating-point atomic), the launch ADDS into the caller's state and never synchronises.  Scores, predictions,
 *   ranks, every counter, confusion, the tp / fp / fn cells and the bank are computed exactly as stated above -- the same statements of the
 *   same kernel body, instantiated per criterion.  Only the loss term and the form of the target differ:
 *   FOCAL (hyb_eval_metrics_focal; class indices y [B], the options and gamma of hyb_cross_entropy_focal_*):
 *     V == 1: term_b is that criterion's per-clip function, keep_b w[y] u_b^gamma (lse_b - z_by), and the den share is w[y_b]: sums[0] /
 *             sums[1] is its arithmetic.  keep, out-of-range targets and NaN scores follow the rules of hyb_eval_metrics.
 *     V > 1:  with pbar the mean softmax written to scores[b]:  ubar = sum_{c != y} pbar_c, summed in class order, not formed as 1 - pbar_y;
 *             term_b = keep_b w[y] ubar^gamma (-log pbar_y), x^0 taken as 1 (x^1 as x, x^2 as x x); the same den share.
 *     gamma == 0 gives hyb_eval_metrics with the same weight and ignore_index (label_smoothing 0), both sums bit for bit, for every V.
 *   SOFT (hyb_eval_metrics_soft; one fp32 row of class probabilities t_b [C] per video, weight and label_smoothing e of
 *   hyb_cross_entropy_dense_* kind 0; q_c = (1 - e) t_c + e / C):
 *     V == 1: term_b = sum_c w_c q_c (lse_b - z_bc), that criterion's per-clip function.
 *     V > 1:  term_b = sum_c w_c q_c (-log pbar_c), in class order from 0.f, one fma per class.
 *     Every video is kept and adds exactly 1.0 to sums[1]: the criterion's divisor is B, there is no ignore_index.  Rows are used as given.
 *     The label for top-1 / top-k / confusion is the LOWEST index among the maxima of t_b (found with a strict >, as pred is).  A row
 *     that holds a NaN has no label: the video counts as kept, is wrong for both accuracies, has no confusion entry, and its loss term
 *     is what the arithmetic gives.
 *   ASYMMETRIC (hyb_eval_multilabel_asym; weight, pos_weight, gamma_pos, gamma_neg, clip of hyb_cross_entropy_asym_*):
 *     V == 1: term_b = sum_c cell_bc, that criterion's per-clip function on (z_b, t_b), where hyb_eval_multilabel has the BCE term; the
 *             meter reports sums[0] / (videos C) as it does for BCE.
 *     V > 1:  with s_c the mean sigmoid (the score) and qbar_c = (1 / V) sum_v sg(-z_vc), its own mean in view order, never 1 - s_c:
 *             the criterion's cell with p -> s_c, q -> qbar_c and
 *               logp = max(log s_c, -100),   logn = max(log qbar_c, -100) if clip == 0, else log(min(qbar_c + clip, 1));
 *             r = max(s_c - clip, 0), base, g_t and L as there, the clip's term the same fma(-(w_c L), base^g_t (t logp + (1 - t) logn), sum)
 *             chain over c.  It is formed in the class loop that forms the scores: no further walk over the row.  All views at
 *             z = +-100 give a finite term.
 *   HYB_E_ARG, before any HIP call: everything hyb_eval_metrics / hyb_eval_multilabel refuse; an exponent that is neither 0 nor >= 1 (NaN
 *   and infinity included); clip outside [0, 1); label_smoothing outside [0, 1]. */
int hyb_eval_metrics_focal(const float* logits /* [B*V, C] */, const long long* target /* [B] */, const float* weight /* [C] or NULL */,
                           long long ignore_index, int has_ignore, float gamma, int topk, int views,
                           double* sums /* [2] */, long long* counts /* [5] */, long long* confusion /* [C*C] or NULL */,
                           long long* pred /* [B] or NULL */, float* scores /* [B, C] or NULL */, int B, int C, void* stream);
int hyb_eval_metrics_soft(const float* logits /* [B*V, C] */, const float* target /* [B, C] */, const float* weight /* [C] or NULL */,
                          float label_smoothing, int topk, int views,
                          double* sums /* [2] */, long long* counts /* [5] */, long long* confusion /* [C*C] or NULL */,
                          long long* pred /* [B] or NULL */, float* scores /* [B, C] or NULL */, int B, int C, void* stream);
int hyb_eval_multilabel_asym(const float* logits /* [B*V, C] */, const float* target /* [B, C] */,
                             const float* weight /* [C] or NULL */, const float* pos_weight /* [C] or NULL */,
                             float gamma_pos, float gamma_neg, float clip, const float* threshold /* [C] */, int views,
                             double* sums /* [1] */, long long* counts /* [5] */, long long* cells /* [C, 3] */,
                             float* bank_scores /* [capacity, C] or NULL */, unsigned char* bank_labels /* [capacity, C] or NULL */,
                             long long capacity,
                             unsigned char* pred /* [B, C] or NULL */, float* scores /* [B, C] */,
                             int B, int C, void* stream);

/* ---- model-level entry points: whole CNN backbone / whole temporal part in ONE call each way ---------------------------
 * They chain the stage-level entry points above on the caller's stream; their purpose is host time (a training step is three
 * operator calls each way), not different arithmetic: results are bit-identical to calling the stages one by one.
 *
 * hyb_backbone_*: `stages` conv stages, UNet.py:58-60 + UNet.py:13 each, in the order UNet.forward chains them (UNet.py:32-37).
 *   channels [stages+1] = {C_in (<= 4: the clip frames are read as NCHW fp32), C_1, ..., C_stages}.
 *   fwd params: HOST array of stages*5 device pointers {weight, gamma, beta, running_mean, running_var};
 *   fwd outs:   HOST array of stages*6 device pointers {y_raw (unused for stage 0), pooled, scale_shift, mean_invstd, packed_bwd,
 *               running_out}; pooled of stage s is the input of stage s+1, sizes as in hyb_convstage_fwd.
 *   BatchNorm running statistics in training mode, per stage: running_out [2][C_s] != NULL -> functional (the updated statistics are
 *               written there, running_mean / running_var are only read; see hyb_bn_finalize); running_out == NULL -> nn.BatchNorm2d's
 *               own behaviour: running_mean / running_var are updated in place and *num_batches_tracked[s] += 1 (HOST array of
 *               `stages` device pointers to 64-bit counters; the array or single entries may be NULL).
 *   bwd params: stages*2 {weight, gamma}; saved: stages*5 {y_raw, stage input (ignored for stage 0: x is passed), scale_shift,
 *               mean_invstd, packed_bwd}; grads: stages*3 {dweight, dgamma, dbeta}.  The clip tensor gets no gradient. */
size_t hyb_backbone_fwd_workspace(int dtype, int stages, const int* channels);
int hyb_backbone_fwd(int dtype, int stages, const int* channels, const float* x, const float* const* params,
                     long long* const* num_batches_tracked, int training, float momentum, float eps, int N, int H, int W,
                     void* const* outs, void* workspace, size_t workspace_bytes, void* stream);
size_t hyb_backbone_bwd_workspace(int dtype, int stages, const int* channels, int N, int H, int W);
int hyb_backbone_bwd(int dtype, int stages, const int* channels, const void* dpooled_last,
                     const void* pooled_last /* NULL, or the last stage's forward output */, const float* x, const float* const* params,
                     const void* const* saved, int training, int N, int H, int W, float* const* grads, void* workspace,
                     size_t workspace_bytes, void* stream);

/* hyb_backbone_infer: the stages of hyb_backbone_fwd for INFERENCE, chained on the caller's stream as hyb_convstage_infer would run them:
 *   one launch forms every stage's scale/shift from the running statistics, one packs every stage's forward weights, then one launch
 *   per stage (two where hyb_conv3x3_pool_fused() == 0).  channels as above; params: HOST array of stages*5 device pointers {weight, gamma,
 *   beta, running_mean, running_var}, all read-only; pooled_last [N, H/2^stages, W/2^stages, pad(C_stages)] T is the only output.
 *   The workspace holds the packed weights, the scale/shift rows, the intermediate pooled maps (two buffers, ping-pong) and, only
 *   for stages without the fused epilogue, one raw conv output. */
size_t hyb_backbone_infer_workspace(int dtype, int stages, const int* channels, int N, int H, int W);
int hyb_backbone_infer(int dtype, int stages, const int* channels, const float* x, const float* const* params, float eps,
                       int N, int H, int W, void* pooled_last, void* workspace, size_t workspace_bytes, void* stream);

/* hyb_temporal_*: frame tokens (global average pool over HW + Linear(C, D); composite's own) -> hyb_encoder_* (TransformerEncoder.pyc
 *   src L110-126) -> head (mean over S + Linear(D, classes); composite's own).  h [B*S, HW, Cp] T is the last pooled map.
 *   Saved by the caller for backward: feat [B*S, Cp] T, enc_saved (hyb_encoder_saved_bytes), enc_out [B,S,D] T; tok [B,S,D] T is scratch.
 *   bwd writes every parameter gradient and dh [B*S, HW, Cp] T. */
int hyb_temporal_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                     const float* head_w, const float* head_b, const float* mask, void* feat, void* tok, void* enc_saved,
                     void* enc_out, float* logits, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes,
                     float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* stream);
size_t hyb_temporal_bwd_workspace(int dtype, int B, int S, int HW, int Cp, int D, int Hid, int L, int H);
int hyb_temporal_bwd(int dtype, const float* dlogits, const float* token_w, const float* const* enc_params, const float* head_w,
                     const float* mask, const void* feat, const void* enc_saved, const void* enc_out, float* dtoken_w,
                     float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C,
                     int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                     const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes, void* stream);

/* hyb_temporal_ce_*: hyb_temporal_* with the mean cross-entropy loss (the composite's own loss, the harness line `loss = criterion(model(x), y)`,
 *   Model.py:56-57 / FCT.py:330-331) inside the same launches: the forward's last launch is LayerNorm + head + loss, the backward's first is
 *   loss backward + head backward + LayerNorm backward -- every dependent launch costs >= 4.6 us on this chip, and these were 8 x 512 x 8
 *   numbers in four launches each way.  target [B] class indices; loss [1]; dloss [1] = d(objective)/d(loss).
 *   ce_scratch: B + 1 floats owned by the caller, ZERO before the first call and left zero-ticketed by every call (per-clip loss terms and
 *   the ticket word the last workgroup resets); calls that share it must be stream-ordered.  Results equal hyb_temporal_* followed by
 *   hyb_cross_entropy_* bit for bit. */
int hyb_temporal_ce_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                        const float* head_w, const float* head_b, const float* mask, const long long* target, void* feat, void* tok,
                        void* enc_saved, void* enc_out, float* logits, float* loss, float* ce_scratch, int B, int S, int HW, int C, int Cp,
                        int D, int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                        const unsigned long long* seed_inc, void* stream);
int hyb_temporal_ce_bwd(int dtype, const float* dloss, const float* logits, const long long* target, const float* token_w,
                        const float* const* enc_params, const float* head_w, const float* mask, const void* feat, const void* enc_saved,
                        const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b,
                        void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p,
                        float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes,
                        void* stream);

/* hyb_temporal_ce_opts_*: hyb_temporal_ce_* with the options of hyb_cross_entropy_opts_* (same meaning, same argument checks) behind the
 *   target: the same launches, the same B + 1 floats of ce_scratch under the same rules (a buffer may serve both families), weight read
 *   when the kernels run.  Results equal hyb_temporal_* followed by hyb_cross_entropy_opts_* bit for bit; shapes the fused tail does
 *   not take run hyb_cross_entropy_opts_* as launches of their own.  (New symbols, hyb_abi_version() stays 9.) */
int hyb_temporal_ce_opts_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                             const float* head_w, const float* head_b, const float* mask, const long long* target,
                             const float* weight /* [classes] or NULL */, long long ignore_index, int has_ignore, float label_smoothing,
                             void* feat, void* tok, void* enc_saved, void* enc_out, float* logits, float* loss, float* ce_scratch, int B,
                             int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p,
                             unsigned long long seed, const unsigned long long* seed_inc, void* stream);
int hyb_temporal_ce_opts_bwd(int dtype, const float* dloss, const float* logits, const long long* target,
                             const float* weight /* [classes] or NULL */, long long ignore_index, int has_ignore, float label_smoothing,
                             const float* token_w, const float* const* enc_params, const float* head_w, const float* mask, const void* feat,
                             const void* enc_saved, const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads,
                             float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H,
                             int classes, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                             void* workspace, size_t workspace_bytes, void* stream);

/* hyb_temporal_ce_mix_*: hyb_temporal_ce_opts_* with target_b [B] and lam [B] (hyb_cross_entropy_mix_*) behind the target: the same
 *   launches, the same ce_scratch, all three read when the kernels run -- a captured call replays with new labels and new lam.  Results
 *   equal hyb_temporal_* followed by hyb_cross_entropy_mix_* bit for bit; shapes the fused tail does not take run hyb_cross_entropy_mix_*
 *   as launches of their own.  (New symbols, hyb_abi_version() stays 9.) */
int hyb_temporal_ce_mix_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                            const float* head_w, const float* head_b, const float* mask, const long long* target,
                            const long long* target_b /* [B] */, const float* lam /* [B] */,
                            const float* weight /* [classes] or NULL */, long long ignore_index, int has_ignore, float label_smoothing,
                            void* feat, void* tok, void* enc_saved, void* enc_out, float* logits, float* loss, float* ce_scratch, int B,
                            int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p,
                            unsigned long long seed, const unsigned long long* seed_inc, void* stream);
int hyb_temporal_ce_mix_bwd(int dtype, const float* dloss, const float* logits, const long long* target,
                            const long long* target_b /* [B] */, const float* lam /* [B] */,
                            const float* weight /* [classes] or NULL */, long long ignore_index, int has_ignore, float label_smoothing,
                            const float* token_w, const float* const* enc_params, const float* head_w, const float* mask, const void* feat,
                            const void* enc_saved, const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads,
                            float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H,
                            int classes, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                            void* workspace, size_t workspace_bytes, void* stream);

/* hyb_temporal_ce_dense_*: hyb_temporal_ce_* with a dense target [B, classes] and the arguments of hyb_cross_entropy_dense_* (same
 *   meaning, same argument checks) in place of the class indices: the same launches, the same B + 1 floats of ce_scratch under the same
 *   rules, target, weight and pos_weight read when the kernels run -- a captured call replays with new targets.  Results equal
 *   hyb_temporal_* followed by hyb_cross_entropy_dense_* bit for bit; shapes the fused tail does not take run hyb_cross_entropy_dense_*
 *   as launches of their own.  (New symbols, hyb_abi_version() stays 9.) */
int hyb_temporal_ce_dense_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                              const float* head_w, const float* head_b, const float* mask, const float* target /* [B,classes] */,
                              const float* weight /* [classes] or NULL */, const float* pos_weight /* [classes] or NULL */, int kind,
                              float label_smoothing, void* feat, void* tok, void* enc_saved, void* enc_out, float* logits, float* loss,
                              float* ce_scratch, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes,
                              float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* stream);
int hyb_temporal_ce_dense_bwd(int dtype, const float* dloss, const float* logits, const float* target /* [B,classes] */,
                              const float* weight /* [classes] or NULL */, const float* pos_weight /* [classes] or NULL */, int kind,
                              float label_smoothing, const float* token_w, const float* const* enc_params, const float* head_w,
                              const float* mask, const void* feat, const void* enc_saved, const void* enc_out, float* dtoken_w,
                              float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW,
                              int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p,
                              unsigned long long seed, const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes,
                              void* stream);

/* hyb_temporal_ce_focal_* / hyb_temporal_ce_asym_*: hyb_temporal_ce_opts_* / hyb_temporal_ce_dense_* with the arguments of
 *   hyb_cross_entropy_focal_* / hyb_cross_entropy_asym_* (same meaning, same argument checks) in place of theirs: the same launches, the
 *   same B + 1 floats of ce_scratch, target, weight and pos_weight read when the kernels run; the exponents and clip travel by value.
 *   Results equal hyb_temporal_* followed by the stand-alone loss bit for bit; shapes the fused tail does not take run it as launches of
 *   its own.  (New symbols, hyb_abi_version() stays 9.) */
int hyb_temporal_ce_focal_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                              const float* head_w, const float* head_b, const float* mask, const long long* target /* [B] */,
                              const float* weight /* [classes] or NULL */, long long ignore_index, int has_ignore, float gamma, void* feat,
                              void* tok, void* enc_saved, void* enc_out, float* logits, float* loss, float* ce_scratch, int B, int S, int HW,
                              int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                              const unsigned long long* seed_inc, void* stream);
int hyb_temporal_ce_focal_bwd(int dtype, const float* dloss, const float* logits, const long long* target /* [B] */,
                              const float* weight /* [classes] or NULL */, long long ignore_index, int has_ignore, float gamma,
                              const float* token_w, const float* const* enc_params, const float* head_w, const float* mask, const void* feat,
                              const void* enc_saved, const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads,
                              float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H,
                              int classes, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                              void* workspace, size_t workspace_bytes, void* stream);
int hyb_temporal_ce_asym_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                             const float* head_w, const float* head_b, const float* mask, const float* target /* [B,classes] */,
                             const float* weight /* [classes] or NULL */, const float* pos_weight /* [classes] or NULL */, float gamma_pos,
                             float gamma_neg, float clip, void* feat, void* tok, void* enc_saved, void* enc_out, float* logits, float* loss,
                             float* ce_scratch, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes,
                             float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* stream);
int hyb_temporal_ce_asym_bwd(int dtype, const float* dloss, const float* logits, const float* target /* [B,classes] */,
                             const float* weight /* [classes] or NULL */, const float* pos_weight /* [classes] or NULL */, float gamma_pos,
                             float gamma_neg, float clip, const float* token_w, const float* const* enc_params, const float* head_w,
                             const float* mask, const void* feat, const void* enc_saved, const void* enc_out, float* dtoken_w,
                             float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW,
                             int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p,
                             unsigned long long seed, const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- FCT, the reference's "Fully Convolutional Transformer" (FCT.py:24-254; SURVEY.md section 8f-1, first "next" row) -----------
 * FORWARD entry points (the backward is the next step of this row).  Arrays are NHWC fp32 with the TRUE channel count
 * ([N,H,W,C]; a pixel's channels are contiguous: the token view of the spatial attention, FCT.py:69-74, is free).  Arithmetic is
 * exact fp32 (fp32-input MFMA for the contractions). */
#define HYB_ACT_NONE 0
#define HYB_ACT_RELU 1
#define HYB_ACT_GELU 2    /* nn.GELU(): erf form, FCT.py:114 */
#define HYB_ACT_SIGMOID 3 /* FCT.py:205 */
/* y = act(conv3x3(x, w, stride 1, "same" zero padding, dilation) + b): nn.Conv2d(.., 3, 1, padding="same"[, dilation=d]) of
 * FCT.py:140-143, 110-113, 172-174, 194-196 followed by the ReLU / GELU / Sigmoid the reference applies next.  w [Co,Ci,3,3], b [Co] or NULL. */
size_t hyb_fct_conv_workspace(int N, int H, int W, int Ci, int Co);
int hyb_fct_conv_fwd(const float* x, const float* w, const float* b, float* y, float* z_out /* NULL, or the pre-activation [N,H,W,Co]
                     (kept for the GELU backward) */, int N, int H, int W, int Ci, int Co, int dilation,
                     int act, void* workspace, size_t workspace_bytes, void* stream);
/* Attention._build_projection for q, k and v in one pass (FCT.py:41-57): depthwise Conv2d(C, C, 3, padding 1, groups=C) + bias
 * -> ReLU -> LayerNorm over C.  HOST arrays of three device pointers each (q, k, v order): w [C,1,3,3], b [C] (or NULL), LayerNorm
 * weight / bias [C].  C a power of two. */
int hyb_fct_qkv_proj_fwd(const float* x, const float* const* w3, const float* const* b3, const float* const* g3, const float* const* beta3,
                         float* q, float* k, float* v, int N, int H, int W, int C, float eps, void* stream);
/* LayerNorm over C of P = N*H*W pixel rows (Transformer.layernorm, FCT.py:97-99) */
int hyb_fct_ln_fwd(const float* x, const float* g, const float* b, float* y, long long P, int C, float eps, void* stream);
/* nn.MultiheadAttention(embed_dim=C, num_heads, batch_first=True)(query=q, key=k, value=v, need_weights=False), FCT.py:37,75:
 * q, k, v, out [N, L, C]; in_w [3C, C], in_b [3C] (or NULL), out_w [C, C], out_b [C] (or NULL); softmax scale 1/sqrt(C/heads);
 * L = H*W tokens per image are streamed through an online softmax (nothing of size L x L is stored). */
size_t hyb_fct_mha_workspace(int N, int L, int C, int heads);
size_t hyb_fct_mha_saved_bytes(int N, int L, int C, int heads);
int hyb_fct_mha_fwd(const float* q, const float* k, const float* v, const float* in_w, const float* in_b, const float* out_w,
                    const float* out_b, float* out, void* saved /* NULL, or hyb_fct_mha_saved_bytes: kept by the caller for the backward */,
                    int N, int L, int C, int heads, void* workspace, size_t workspace_bytes, void* stream);
size_t hyb_fct_mha_bwd_workspace(int N, int L, int C, int heads);
int hyb_fct_mha_bwd(const float* dout, const float* q, const float* k, const float* v, const float* in_w, const float* out_w,
                    const void* saved, float* dq, float* dk, float* dv, float* din_w, float* din_b /* or NULL */, float* dout_w,
                    float* dout_b /* or NULL */, int N, int L, int C, int heads, void* workspace, size_t workspace_bytes, void* stream);
/* y = a + b (torch.add, FCT.py:96,101,127-128) */
int hyb_fct_add(const float* a, const float* b, float* y, long long n, void* stream);
/* mode 0: nn.MaxPool2d(2) (FCT.py:147), 1: nn.AvgPool2d(2,2) (FCT.py:222), 2: nn.Upsample(scale_factor=2) nearest (FCT.py:170).
 * H, W are the input sizes; pooling floors odd sizes like torch. */
int hyb_fct_resample(int mode, const float* x, float* y, int N, int H, int W, int C, void* stream);
/* torch.cat((a, b), dim=channels) (FCT.py:157,180) */
int hyb_fct_concat(const float* a, int Ca, const float* b, int Cb, float* y, long long P, void* stream);
/* DiceLoss.forward (Metrics.py:14-22) on channel 0 of NCHW pred / true [N,C,H,W]: 1 - (2 sum(p t) + smooth) / (sum p + sum t + smooth) */
size_t hyb_dice_workspace(void);
int hyb_dice_fwd(const float* pred, const float* tru, float* loss /* [1] */, int N, int C, long long HW, float smooth, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- FCT backward (autograd of the forward entry points above; all gradients overwritten, reductions in a fixed order) -----------
 * conv: saved = y for ReLU / sigmoid, the pre-activation z for GELU, ignored for NONE; dx may be NULL (first layer). */
size_t hyb_fct_conv_bwd_workspace(int N, int H, int W, int Ci, int Co);
int hyb_fct_conv_bwd(const float* dy, const float* x, const float* w, const float* saved, float* dx, float* dw, float* db /* or NULL */, int N, int H,
                     int W, int Ci, int Co, int dilation, int act, void* workspace, size_t workspace_bytes, void* stream);
size_t hyb_fct_qkv_proj_bwd_workspace(int N, int H, int W, int C);
int hyb_fct_qkv_proj_bwd(const float* x, const float* const* w3, const float* const* b3, const float* const* g3, const float* const* dq3,
                         float* dx, float* const* dw3, float* const* db3, float* const* dg3, float* const* dbeta3, int N, int H, int W,
                         int C, float eps, void* workspace, size_t workspace_bytes, void* stream);
size_t hyb_fct_ln_bwd_workspace(long long P, int C);
int hyb_fct_ln_bwd(const float* dy, const float* x, const float* g, float* dx, float* dg, float* db, long long P, int C, float eps,
                   void* workspace, size_t workspace_bytes, void* stream);
/* mode 0: MaxPool2d(2) backward (x = the pool's input [N,H,W,C]; the gradient goes to the first maximum in scan order, like torch);
 * mode 2: Upsample x2 backward (dy [N,2H,2W,C] -> dx [N,H,W,C]) */
int hyb_fct_resample_bwd(int mode, const float* dy, const float* x, float* dx, int N, int H, int W, int C, void* stream);
int hyb_fct_concat_bwd(const float* dy, float* da /* or NULL */, int Ca, float* db /* or NULL */, int Cb, long long P, void* stream);
int hyb_dice_bwd(const float* pred, const float* tru, const float* dloss, float* dpred /* NCHW like pred */, int N, int C, long long HW, float smooth,
                 void* workspace /* >= 4096 bytes */, size_t workspace_bytes, void* stream);
/* nn.Dropout in train mode (FCT.py:115,146,175): y = x * keep / (1 - p), mask from the counter-based RNG keyed by (seed + *seed_inc);
 * the backward is the same call on the gradient. */
int hyb_fct_dropout(const float* x, float* y, long long n, float p, unsigned long long seed, const unsigned long long* seed_inc, void* stream);

/* ---- clip input pipeline: torchvision's to-tensor transform on the device -----------------------------
 * dst[f][c][h][w] = src[f][h][w][c] / 255 for `frames` uint8 HWC frames (what PIL / cv2 decode to; Dataloader.py:19-23,
 * dataset.pyc src L106-113): frames cross PCIe as bytes and become the fp32 NCHW clip tensor the first conv stage reads. */
int hyb_frames_u8hwc_to_f32chw(const unsigned char* src, float* dst, long long frames, int H, int W, int C, void* stream);
/* Clip augmentation in the same pass (torchvision's Resize / RandomResizedCrop / RandomHorizontalFlip / Normalize plus temporal
 * sub-sampling, applied with ONE parameter row per clip so that all frames of a clip get the same crop and flip).  A row is
 * {y0, x0, ch, cw, flip, t0, tstride, 0}; rows live in device memory (no host value per batch: the launch can sit on the copy stream
 * behind the H2D of the rows and can be captured and replayed with new rows).  For clip b, output frame t, channel c, pixel (oy, ox):
 *   ts  = clamp(t0 + t*tstride, 0, Tin-1)
 *   oxs = flip ? Wo-1-ox : ox
 *   ny  = max((2*oy +1)*ch - Ho, 0);  iy0 = ny / (2*Ho);  ry = ny % (2*Ho);  iy1 = min(iy0+1, ch-1);  fy = float(ry) / float(2*Ho)
 *   nx  = max((2*oxs+1)*cw - Wo, 0);  ix0 = nx / (2*Wo);  rx = nx % (2*Wo);  ix1 = min(ix0+1, cw-1);  fx = float(rx) / float(2*Wo)
 *   aYX = (float) src[b][ts][y0+iyY][x0+ixX][c]
 *   top = a00 + fx*(a01-a00);   bot = a10 + fx*(a11-a10);   v = top + fy*(bot-top)
 *   out = v / 255.0f;           if (mean_invstd) out = (out - mean[c]) * invstd[c]
 * i.e. F.interpolate(crop, (Ho,Wo), mode="bilinear", align_corners=False, antialias=False) / 255, flipped, normalised: NO antialias
 * filter.  ch == Ho, cw == Wo gives bit-for-bit what hyb_frames_u8hwc_to_f32chw writes.  The kernel clamps every row before use (y0 to
 * [0, Hin-1], ch to [1, Hin-y0], the same for x0 / cw, flip read as != 0, ts as above): no row value reads outside src.
 * C <= 4; Hin, Win, Ho, Wo <= 16384. */
int hyb_clips_u8_transform(const unsigned char* src /* [B][Tin][Hin][Win][C] uint8 */,
                           const int* params        /* device, [B][8] int32, one row per CLIP */,
                           const float* mean_invstd /* device, [2][C]: mean then 1/std; or NULL = no normalisation */,
                           float* dst               /* [B][Tout][C][Ho][Wo] fp32 */,
                           int B, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream);

/* hyb_clips_u8_transform_mix: the same pass with Mixup / CutMix (new symbol, hyb_abi_version() stays 9).  `mix`: one more int32 row of 8 per
 * clip, in device memory: {partner, kind, by0, bx0, bh, bw, lam_bits, 0}.  own[b] is what hyb_clips_u8_transform writes for clip b from its
 * own params row (crop, flip, temporal window, / 255, mean / std); the partner's value own[partner] comes from the PARTNER's params row,
 * temporal window included.
 *   kind 0 (none):   out = own[b]; the partner is not read; the bits of hyb_clips_u8_transform.
 *   kind 1 (Mixup):  out = lam*own[b] + (1-lam)*own[partner] per element in fp32, after both operands' full pipelines; lam = the fp32
 *                    whose bits are lam_bits, clamped into [0, 1], a NaN counts as 1.
 *   kind 2 (CutMix): inside the box [by0, by0+bh) x [bx0, bx0+bw) of OUTPUT coordinates (the same box for every frame of the clip) the pixel
 *                    is own[partner] at the same position, outside it own[b]; no arithmetic on the values -- every output element is bit
 *                    for bit one of the two -- and a pixel gathers only the taps of the clip it comes from.  lam_bits is not read.
 * The rows are clamped before use like the params rows: partner into [0, B-1], by0 into [0, Ho] and bh into [0, Ho-by0], bx0 into [0, Wo]
 * and bw into [0, Wo-bx0], a kind outside 0..2 counts as 0: no row value reads outside src.  Same limits as hyb_clips_u8_transform. */
int hyb_clips_u8_transform_mix(const unsigned char* src /* [B][Tin][Hin][Win][C] uint8 */,
                               const int* params        /* device, [B][8] int32, one row per CLIP */,
                               const int* mix           /* device, [B][8] int32, one row per CLIP */,
                               const float* mean_invstd /* device, [2][C]: mean then 1/std; or NULL = no normalisation */,
                               float* dst               /* [B][Tout][C][Ho][Wo] fp32 */,
                               int B, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream);

/* hyb_clips_u8_transform_views: multi-view evaluation clips, V views of every source clip in one launch (new symbol, hyb_abi_version() stays
 * 9).  `params` holds V rows per SOURCE clip, adjacent: output clip r = b*V + v is what hyb_clips_u8_transform writes for row params[r] applied
 * to source clip b = r / V -- the same clamps, the same sampling rule, the same division by 255 and (x - mean) * invstd, bit for bit; nothing
 * but the source-clip index changes.  So B uint8 clips, copied to the device once, become the [B*V] rows that hyb_eval_metrics scores with
 * views = V (the mean softmax of V adjacent rows), without replicating a source byte.  The kernel walks the output frames with v fastest inside
 * (b, t): views that share a temporal window read one source frame from neighbouring workgroups; which frame a workgroup writes does not
 * change its values.  V >= 1, B*V within int; otherwise the limits of hyb_clips_u8_transform.  V == 1 is that function's output. */
int hyb_clips_u8_transform_views(const unsigned char* src /* [B][Tin][Hin][Win][C] uint8 */,
                                 const int* params        /* device, [B*V][8] int32: V rows per SOURCE clip, adjacent */,
                                 const float* mean_invstd /* device, [2][C]: mean then 1/std; or NULL = no normalisation */,
                                 float* dst               /* [B*V][Tout][C][Ho][Wo] fp32 */,
                                 int B, int V, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream);

/* hyb_clips_u8_transform_aa: the antialiased resize, torchvision's Resize(antialias=True) (new symbol, hyb_abi_version() stays 9).  Rows, views
 * and layouts are hyb_clips_u8_transform_views': V rows {y0, x0, ch, cw, flip, t0, tstride, 0} per SOURCE clip, output clip r = b*V + v from row r
 * and the bytes of clip b = r / V; V == 1 is the training / single-view case.  The clamps of a row, the temporal index ts and the flip
 * (oxs = flip ? Wo-1-ox : ox: output column ox takes the value of column Wo-1-ox) are hyb_clips_u8_transform's.  Only the resampling differs.
 * Per axis, a crop of n source positions resampled to m output positions (n = ch, m = Ho for rows; n = cw, m = Wo for columns), for output
 * index i and source index k in [0, n), all in int32 (the largest value is about 2 * 16384^2):
 *   D = 2*max(n, m);   W(i,k) = max(0, D - |(2k+1)*m - (2i+1)*n|);   S(i) = sum_k W(i,k)
 *   v   = sum_ky sum_kx Wy(oy,ky) * Wx(oxs,kx) * (float) src[b][ts][y0+ky][x0+kx][c] / (Sy(oy) * Sx(oxs))
 *   out = v / 255.0f;           if (mean_invstd) out = (out - mean[c]) * invstd[c]
 * For n > m that is F.interpolate(crop, (Ho,Wo), mode="bilinear", align_corners=False, antialias=True): a triangle filter of support n/m,
 * renormalised at the borders, at most 2*ceil(n/m)+1 taps.  For n <= m there are at most two taps with the weights (1-f, f) of
 * hyb_clips_u8_transform's rule, its border clamp expressed as renormalisation (what torch does with antialias=True when up-scaling).
 * Evaluation order in fp32: each weight is the correctly rounded quotient float(W) / float(S); the columns are summed first, the rows second,
 * each sum a chain of fused multiply-adds in ascending k.  Two consequences are part of the contract:
 *   - ch == Ho and cw == Wo (one tap of weight exactly 1 per axis): the bits of hyb_clips_u8_transform for that row, with and without mean_invstd
 *   - n == 2m on both axes (interior weights (1,3,3,1)/8): an element whose windows are not clipped by a border is fp32(N/64) / 255, N the integer
 *     weighted sum -- every partial sum is exact
 * Same limits as hyb_clips_u8_transform_views: V >= 1, B*V within int, C <= 4, Hin, Win, Ho, Wo <= 16384. */
int hyb_clips_u8_transform_aa(const unsigned char* src /* [B][Tin][Hin][Win][C] uint8 */,
                              const int* params        /* device, [B*V][8] int32: V rows per SOURCE clip, adjacent */,
                              const float* mean_invstd /* device, [2][C]: mean then 1/std; or NULL = no normalisation */,
                              float* dst               /* [B*V][Tout][C][Ho][Wo] fp32 */,
                              int B, int V, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream);

/* hyb_clips_u8_transform_photo: the same pass with colour jitter, grayscale, Gaussian noise and random erasing, with or without mixing (new
 * symbols, hyb_abi_version() stays 9).  `photo`: one more int32 row of 16 per clip, in device memory; every field is clamped by the kernel:
 *   [0] [1] [2]  brightness, contrast, saturation factor (fp32 bits): !(f >= 0) (NaN included) counts as 1, values above 16 as 16; a factor of
 *                exactly 1.0f skips its op
 *   [3]          order of the three ops, the lexicographic permutations of (B, C, S): 0 BCS, 1 BSC, 2 CBS, 3 CSB, 4 SBC, 5 SCB; outside 0..5: 0
 *   [4]          gray: != 0, every channel becomes the luma after the jitter
 *   [5]          noise sigma (fp32 bits, on the [0,1] scale): !(s > 0) is off, values above 1 count as 1
 *   [6] [7]      low, high 32 bits of the 64-bit noise seed
 *   [8..11]      erase box ey0, ex0, eh, ew in OUTPUT coordinates, clamped like the CutMix box (ey0 into [0, Ho], eh into [0, Ho-ey0], the same
 *                for ex0 / ew); eh*ew == 0: no erase
 *   [12]         erase mode: 0 "zero", 1 "black", 2 "pixel"; outside 0..2: 0
 *   [13..15]     reserved, not read
 * Per output pixel of clip b, frame t, all C channels together (C is 1 or 3), in fp32:
 *   1. v_c = the value of hyb_clips_u8_transform up to and including the division by 255
 *   2. the three ops in the row's order, each followed by a clamp to [0, 1]:
 *        brightness v = f*v;   contrast v = f*v + (1-f)*mu;   saturation v = f*v + (1-f)*L(v)
 *      L = 0.2989 r + 0.587 g + 0.114 b; for C == 1 L is the value itself, saturation and gray do nothing
 *   3. gray: v_c = L(v)
 *   4. noise: v = clamp(v + sigma*z, 0, 1), z a Box-Muller draw from the library's counter hash h(seed, idx) (splitmix64's finaliser of
 *      idx * 0x9E3779B97F4A7C15 + seed, upper 32 bits) at the element's index inside its clip e = ((t*C + c)*Ho + oy)*Wo + ox:
 *        u1 = ((h(seed, 2e) >> 8) + 1) * 2^-24;   u2 = (h(seed, 2e+1) >> 8) * 2^-24;   z = sqrt(-2 ln u1) * cos(2 pi u2)
 *      so the noise differs from frame to frame; only the geometry and the colour map are shared over a clip
 *   5. normalise: v = (v - mean[c]) * invstd[c]   (skipped when mean_invstd is NULL)
 *   6. erase, inside the box: mode 0 0.0f; mode 1 (0 - mean[c]) * invstd[c] (black; 0.0f without mean_invstd); mode 2 a Box-Muller draw at
 *      element index e + Tout*C*Ho*Wo (the same seed past the noise's range), on the normalised scale
 *   7. mix as in hyb_clips_u8_transform_mix (mix == NULL: nothing mixes): the partner's pixel is formed by steps 1-6 under the PARTNER's params
 *      and photo rows at the same output coordinates, so a mixed clip is the blend or composite of the two clips as this kernel alone would have
 *      written them; kind 0 and CutMix still do no arithmetic on the values.
 * The contrast pivot mu is per CLIP, so that all frames of a clip get the same affine map (the rule for crop and flip):
 *   mu = (sum_t luma_sums[b][t]) / (10000 * 255 * ch * cw * Tout), formed in double and rounded to fp32 once; min(fb*mu, 1) instead when
 *   brightness precedes contrast in the order.
 * That is the mean luma of the UNTOUCHED source crop over the clip's frames -- on purpose not torchvision's per-frame mean of the already
 * jittered, already resized image: it needs no pass over the output and is exact in integers.  luma_sums comes from hyb_clips_u8_luma_sums
 * with the same src, params and Tout; it may be NULL when no contrast factor other than 1 can occur (with NULL every contrast factor counts
 * as 1).  Photo rows of factors 1, sigma 0 and an empty box give the bits of hyb_clips_u8_transform / _mix.
 * C must be 1 or 3; otherwise the limits of hyb_clips_u8_transform. */
int hyb_clips_u8_transform_photo(const unsigned char* src /* [B][Tin][Hin][Win][C] uint8 */,
                                 const int* params        /* device, [B][8] int32, one row per CLIP */,
                                 const int* mix           /* device, [B][8] int32, one row per CLIP; or NULL = nothing mixes */,
                                 const int* photo         /* device, [B][16] int32, one row per CLIP */,
                                 const long long* luma_sums /* device, [B][Tout] int64 from hyb_clips_u8_luma_sums; or NULL */,
                                 const float* mean_invstd /* device, [2][C]: mean then 1/std; or NULL = no normalisation */,
                                 float* dst               /* [B][Tout][C][Ho][Wo] fp32 */,
                                 int B, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream);
/* sums[b][t] = the sum over the clamped crop box of output frame t's source frame (the params rows' clamps and temporal clamp of
 * hyb_clips_u8_transform) of 2989 R + 5870 G + 1140 B; for C == 1 of 10000 * value.  Pure integer arithmetic: exact, independent of the
 * summation order.  The call overwrites sums (it zeroes them itself, on the stream) and leaves no state behind.  C must be 1 or 3;
 * Hin, Win <= 16384. */
int hyb_clips_u8_luma_sums(const unsigned char* src /* [B][Tin][Hin][Win][C] uint8 */,
                           const int* params        /* device, [B][8] int32, one row per CLIP */,
                           long long* sums          /* device, [B][Tout] int64 */,
                           int B, int Tin, int Hin, int Win, int C, int Tout, void* stream);

/* hyb_clip_aug_u8_transform: hyb_clips_u8_transform_photo with RandAugment's ops and a hue shift in the same pass (new symbol,
 * hyb_abi_version() stays 9; the name stands outside the hyb_clips_u8_* family, whose six members tests/test_clip_job_cpu.py lists as a closed
 * set).  `aug`: one more int32 row of 32 per clip, in device memory; all frames of a clip share it:
 *   [0]        flags: bit 0 switches the geometry on
 *   [1]        n, the length of the program, clamped into 0..8
 *   [2..17]    (op, arg) x 8: the program's steps in order; only the first n are read; an op outside 0..8 counts as 0 (Identity)
 *   [18..23]   M = (a, b, c, d, e, f) as fp32 bits; a value that is not finite switches the geometry off
 *   [24..26]   fill[3] as fp32 bits, on the [0,1] scale: !(v >= 0) (NaN included) counts as 0, values above 1 as 1; C == 1 reads fill[0]
 *   [27..31]   reserved, not read
 * The pixel chain of hyb_clips_u8_transform_photo becomes
 *   1.  resample, with the geometry when it is on
 *   1a. the program: its n steps on the [0,1] value, in order
 *   2-6 jitter, gray, noise, normalise, erase, as hyb_clips_u8_transform_photo states them (photo == NULL: identity photo rows)
 *   7.  mix: the partner's pixel goes through the PARTNER's params, aug and photo rows.
 * Geometry.  M maps an output pixel to a point of the un-augmented output frame, in PIL's Image.AFFINE convention; pixel (i, j) = (oy, ox)
 * has the centre (j + 1/2, i + 1/2), everything in fp32:
 *   x = fma(a, j + 0.5f, fma(b, i + 0.5f, c));      y = fma(d, j + 0.5f, fma(e, i + 0.5f, f))
 *   !(0 <= x < Wo && 0 <= y < Ho) (a NaN is outside): the value is fill[c]; it then goes through 1a-7 like any other pixel.  Otherwise
 *   x  = Wo - x when the clip is flipped
 *   sx = (x * float(cw)) / float(Wo) - 0.5f;        sy = (y * float(ch)) / float(Ho) - 0.5f          (rounded product, quotient, difference)
 *   ix = floor(sx), fx = sx - ix;  iy = floor(sy), fy = sy - iy;    the taps ix, ix + 1 clamped into [0, cw-1], iy, iy + 1 into [0, ch-1]
 *   top = fma(fx, a01 - a00, a00);  bot = fma(fx, a11 - a10, a10);  v = fma(fy, bot - top, top) / 255.0f
 * ONE resampling of the source crop through the composite map (output pixel -> un-augmented output frame -> crop), not a second resampling of
 * the resized frame; with ch == Ho, cw == Wo and no flip it is PIL's Image.transform(AFFINE, BILINEAR, fillcolor) of the crop.  A row without the
 * geometry takes the integer taps of hyb_clips_u8_transform: with n == 0 (or only Identity steps) on top and identity photo rows (or NULL), the
 * bits of hyb_clips_u8_transform_photo, and so of hyb_clips_u8_transform and hyb_clips_u8_transform_mix.
 * The program.  q = floor(255 v + 1/2) is the byte of a value; factors are read like the photo row's (!(f >= 0) is 1, above 16 is 16) and
 * integer arguments are clamped into their ranges.  L(v) = 0.2989 r + 0.587 g + 0.114 b.
 *   0 Identity
 *   1 Invert                  v = 1 - v
 *   2 Brightness   f bits     v = clamp01(f v)
 *   3 Contrast     f bits     v = clamp01(f v + (1-f) m).  m starts as the clip's mean luma mu0 = (sum_t luma_sums[b][t]) / (10000*255*ch*cw*Tout)
 *                             (double, rounded to fp32 once) and moves with the steps in front of this one: a Brightness step makes it
 *                             min(f m, 1), an Invert step 1 - m, nothing else moves it.  luma_sums == NULL: the factor counts as 1
 *   4 Color        f bits     v = clamp01(f v + (1-f) L(v));  nothing happens at C == 1
 *   5 Posterize    bits 0..8  v = float(q & ~(2^(8-bits) - 1)) / 255.0f
 *   6 Solarize     thr 0..256 q >= thr: v = 1 - v
 *   7 SolarizeAdd  add 0..255 q < 128: v = min(1, v + float(add) / 255.0f)
 *   8 Hue          h bits     a NaN is 0, then clamped into [-1/2, 1/2]; torchvision's adjust_hue on floats; nothing happens at C == 1 or h == 0:
 *        mx = max(r,g,b); mn = min(r,g,b); cr = mx - mn; eq = (mx == mn); s = cr / (eq ? 1 : mx); d = eq ? 1 : cr
 *        rc = (mx-r)/d; gc = (mx-g)/d; bc = (mx-b)/d
 *        hh = mx == r ? bc - gc : (mx == g ? 2 + rc - bc : 4 + gc - rc);   hh = fmod(hh/6 + 1, 1);   hh = hh + h;  hh = hh - floor(hh)
 *        i = floor(6 hh); f = 6 hh - i; i = i mod 6
 *        p = clamp01(mx (1 - s)); q' = clamp01(mx (1 - s f)); t = clamp01(mx (1 - s (1 - f)))
 *        (r,g,b) = i == 0 ? (mx,t,p) : 1 ? (q',mx,p) : 2 ? (p,mx,t) : 3 ? (p,q',mx) : 4 ? (t,p,mx) : (mx,p,q')       every operation rounded, none fused
 * On values that are bytes / 255 Invert, Posterize, Solarize and SolarizeAdd give the bytes of PIL's ImageOps.invert / posterize / solarize and
 * of timm's solarize_add.  The jitter of step 2 keeps its pivot rule on the untouched mu0.
 * No row value reads outside src.  mix, photo, luma_sums and mean_invstd may be NULL.  C must be 1 or 3; otherwise the limits of
 * hyb_clips_u8_transform. */
int hyb_clip_aug_u8_transform(const unsigned char* src /* [B][Tin][Hin][Win][C] uint8 */,
                              const int* params        /* device, [B][8] int32, one row per CLIP */,
                              const int* mix           /* device, [B][8] int32, one row per CLIP; or NULL = nothing mixes */,
                              const int* photo         /* device, [B][16] int32, one row per CLIP; or NULL = identity rows */,
                              const int* aug           /* device, [B][32] int32, one row per CLIP */,
                              const long long* luma_sums /* device, [B][Tout] int64 from hyb_clips_u8_luma_sums; or NULL */,
                              const float* mean_invstd /* device, [2][C]: mean then 1/std; or NULL = no normalisation */,
                              float* dst               /* [B][Tout][C][Ho][Wo] fp32 */,
                              int B, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream);

/* ---- ResNet-bottleneck backbone `Encoder_32K` (only bytecode of it ships with the reference:
 * __pycache__/AE_256_32K.cpython-38.pyc, read as data -- `Bottleneck` src L21-53, `Encoder_32K` src L58-137).  NHWC fp32 with the
 * true channel counts, exact-fp32 arithmetic like the FCT entry points above, which these generalise.
 *
 * nn.Conv2d(Ci, Co, k, stride, padding, dilation, bias) forward / backward: the stem Conv2d(3, 64, 7, 2, 3, bias=False) (src L62),
 * the bottleneck's 1x1 / 3x3-stride-s / 1x1 (src L25-30), the down-sampling Conv2d(.., 1, stride, bias=False) (src L99-102) and the
 * tail's Conv2d(.., 3, 1, 1) with bias (src L70-88).  x [N,H,W,Ci], w [Co,Ci,k,k], y [N,Ho,Wo,Co] with torch's output size
 * floor((H + 2 pad - dilation (k-1) - 1) / stride) + 1; act / z_out / saved as for hyb_fct_conv_*, which are these at k=3, stride 1. */
size_t hyb_conv2d_workspace(int N, int H, int W, int Ci, int Co, int k, int stride, int pad, int dilation);
int hyb_conv2d_fwd(const float* x, const float* w, const float* b /* or NULL */, float* y, float* z_out /* or NULL */, int N, int H, int W, int Ci,
                   int Co, int k, int stride, int pad, int dilation, int act, void* workspace, size_t workspace_bytes, void* stream);
size_t hyb_conv2d_bwd_workspace(int N, int H, int W, int Ci, int Co, int k, int stride, int pad, int dilation);
int hyb_conv2d_bwd(const float* dy, const float* x, const float* w, const float* saved, float* dx /* or NULL */, float* dw, float* db /* or NULL */,
                   int N, int H, int W, int Ci, int Co, int k, int stride, int pad, int dilation, int act, void* workspace,
                   size_t workspace_bytes, void* stream);
/* nn.BatchNorm2d over P = N*H*W pixel rows of C channels (C % 4 == 0, C/4 a divisor of 256), optionally fused with the bottleneck's
 * `out += residual` and nn.ReLU (src L44-52): y = relu?( (x - mean) / sqrt(var + eps) * gamma + beta (+ residual) ).
 * training != 0: batch statistics (biased variance), running_mean / running_var (or NULL) updated in place with `momentum` and the
 * unbiased variance, like torch; training == 0: the running statistics normalise.  coef [4][C] (a, b, mean, invstd) is written by
 * the forward and read by the backward; y in the backward is the forward's output (ReLU mask; ignored when relu == 0) -- NULL when the
 * forward had no residual: the mask is then recomputed as fmaf(x, a, b) > 0, the forward's own expression (one array less to read). */
size_t hyb_bn2d_workspace(long long P, int C);
int hyb_bn2d_fwd(const float* x, const float* gamma, const float* beta, const float* residual /* or NULL */, float* y, float* coef,
                 float* running_mean, float* running_var, long long P, int C, float eps, float momentum, int training, int relu,
                 void* workspace, size_t workspace_bytes, void* stream);
int hyb_bn2d_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* coef, float* dx,
                 float* dresidual /* or NULL */, float* dgamma, float* dbeta, long long P, int C, int training, int relu, void* workspace,
                 size_t workspace_bytes, void* stream);
/* nn.Dropout2d(p) in train mode (src L92, L113, L136) on [N,H,W,C]: one decision per (image, channel) plane from the counter-based RNG
 * keyed by (seed + *seed_inc); the backward is the same call on the gradient. */
int hyb_dropout2d(const float* x, float* y, int N, long long HW, int C, float p, unsigned long long seed, const unsigned long long* seed_inc,
                  void* stream);

/* ---- optimizer step: torch.optim.AdamW of Model.py:153 / FCT.py:305, all tensors in one launch ---------
 * Same update as torch.optim.AdamW(betas=(beta1,beta2), eps, weight_decay, amsgrad=False, maximize=False) at step number
 * `step` (1-based).  params/grads/exp_avg/exp_avg_sq: HOST arrays of `count` device pointers (fp32 tensors of numel[i]
 * elements); state tensors are caller-owned and must be zero before step 1.  Hyper-parameters are doubles (Python floats):
 * 1 - beta etc. are formed in double and rounded to fp32 once, like torch does.
 * step_inc: NULL, or a DEVICE pointer to one 64-bit counter: the step number used is step + *step_inc, read when the kernel runs
 * (the bias corrections are then formed on the device, in double) -- lets one captured launch serve every replay of a hipGraph.
 * advance_ticket != NULL (needs step_inc): the call also adds 1 to *step_inc once every workgroup has read it (the last workgroup to
 * finish does it), so the replayed step needs no separate "counter += 1" launch.  advance_ticket is a DEVICE pointer to one 32-bit word
 * owned by the caller, zero at rest, used by this counter's advancing launches only (the launch counts its finished workgroups there and
 * leaves it zero): advancing calls on different counters -- two optimizers on two streams -- each bring their own word and never
 * interfere; two advancing calls on the SAME counter must be stream-ordered, as any two steps of one optimizer are.
 * -1 with nothing launched for a NULL array or entry or a numel[i] <= 0 ANYWHERE in the table (also past the 80 tensors of the first
 * launch), and, as every optimizer call below, for a table of 2^31 or more 4096-element chunks. */
int hyb_adamw_step(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   const long long* numel, double lr, double beta1, double beta2, double eps, double weight_decay, long long step,
                   long long* step_inc, unsigned int* advance_ticket, void* stream);

/* ---- hyper-parameters in device memory: gradient-norm clipping and learning-rate schedules under hipGraph replay -------------------
 * (New symbols only: hyb_adamw_step above is unchanged and hyb_abi_version() stays 9.)
 * hyb_adamw_step takes its hyper-parameters by value, so a captured launch keeps the values of the capture for ever.  The three calls
 * below keep them in a DEVICE block `double hyper[6]` = {lr, beta1, beta2, eps, weight_decay, max_grad_norm}, owned by the caller.
 *
 * hyb_adamw_hyper_set: writes the six values from a one-workgroup kernel that received them as kernel arguments: no staging memory, the
 * host never waits, and calling it before every step with a new lr is safe.  NOT meant to be captured into a replayed graph: a captured
 * call would rewrite the block with its capture-time values at every replay.  max_grad_norm <= 0 or +inf = no clipping. */
int hyb_adamw_hyper_set(double* hyper, double lr, double beta1, double beta2, double eps, double weight_decay, double max_grad_norm,
                        void* stream);
/* hyb_grad_norm: ONE global L2 norm over `count` fp32 gradient tensors (host array of device pointers, as hyb_adamw_step) and the clip
 * coefficient of torch.nn.utils.clip_grad_norm_(norm_type = 2): norm_out[0] = sqrt(sum g^2), norm_out[1] = min(1, max_grad_norm /
 * (norm_out[0] + 1e-6)) (1 when clipping is off; a NaN norm gives a NaN coefficient, as torch with error_if_nonfinite = False).
 * 4096-element chunks, one workgroup each, fp32 within a chunk in a fixed order (independent of the tensor's alignment), then the chunks'
 * partial sums in double in a fixed order by a one-workgroup launch: no floating-point atomics, bit-identical from run to run.
 * partials: hyb_grad_norm_workspace(count, numel) floats (= sum of ceil(numel[i] / 4096); 0 for bad arguments); no state is kept in it
 * between calls, calls sharing partials / norm_out must be stream-ordered.  More than 80 tensors = more launches, still one norm. */
size_t hyb_grad_norm_workspace(int count, const long long* numel);
int hyb_grad_norm(int count, const float* const* grads, const long long* numel, float* partials, const double* hyper,
                  float* norm_out /* [2]: total L2 norm, clip coefficient */, void* stream);
/* hyb_adamw_step_dev: the update of hyb_adamw_step with every scalar formed ON THE DEVICE from hyper[0..4] and step + (step_inc ?
 * *step_inc : 0), in double, rounded to fp32 once -- the expressions hyb_adamw_step evaluates on the host.  clip: NULL, or the norm_out
 * of hyb_grad_norm: every gradient element is multiplied by clip[1] before use (g * 1.0f is exact, so an unclipped step equals a step
 * without clipping bit for bit).  step_inc / advance_ticket as in hyb_adamw_step. */
int hyb_adamw_step_dev(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const long long* numel, const double* hyper, long long step, long long* step_inc, unsigned int* advance_ticket,
                       const float* clip /* norm_out of hyb_grad_norm, or NULL */, void* stream);

/* ---- exponential moving average of the weights, kept inside the AdamW launch ---------------------------------------------------------
 * (New symbols only; hyb_abi_version() stays 9.)  The average's two hyper-parameters live in a DEVICE block `double ema_hyper[2]` =
 * {decay, warmup}, owned by the caller, for the reason hyper[] does: a captured launch must follow a decay that changes between replays.
 *
 * hyb_adamw_ema_set: writes {decay, warmup} from a one-workgroup kernel that received them as kernel arguments (as hyb_adamw_hyper_set;
 * NOT meant to be captured).  0 <= decay < 1; warmup is 0 or 1. */
int hyb_adamw_ema_set(double* ema_hyper /* [2] */, double decay, double warmup, void* stream);
/* hyb_adamw_step_dev_ema: hyb_adamw_step_dev -- params, exp_avg and exp_avg_sq come out bit for bit as it gives them -- which also moves
 * ema[i] (fp32, numel[i] elements, never the parameter itself), in the same launch, from the parameter value it has just formed:
 *     t = step + (step_inc ? *step_inc : 0), n = t - 1;  d = warmup ? min(decay, (1 + n) / (10 + n)) : decay      (double, on the device)
 *     e <- fmaf((float)d, e, (float)(1 - d) * p_new)                                                            (decay 0: e == p_new exactly)
 * 9 x 4 bytes of traffic per parameter instead of 7 x 4.  One launch holds 64 tensors (80 without the average: a sixth pointer per tensor
 * in 4 KB of kernel arguments); more tensors = more launches, the last of which advances the counter. */
int hyb_adamw_step_dev_ema(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                           float* const* ema, const long long* numel, const double* hyper, const double* ema_hyper, long long step,
                           long long* step_inc, unsigned int* advance_ticket, const float* clip /* norm_out of hyb_grad_norm, or NULL */,
                           void* stream);

/* ---- gradient accumulation: one optimizer step over k micro-batches --------------------------------------------------------------------
 * (New symbols only; hyb_abi_version() stays 9.)  acc[i]: one fp32 accumulator of numel[i] elements per parameter, caller-owned, zero at
 * every optimizer-step boundary.  Micro-batches 1 .. k - 1 end in hyb_grad_accumulate, the k-th in hyb_adamw_step_dev_acc (after
 * hyb_grad_norm_acc when clipping).  With inv_k = (float)(1.0 / (double)k) the effective gradient of one element is
 *     G = (acc + g) * inv_k        (grads == NULL as a whole: G = acc * inv_k -- data parallelism, acc is the all-reduced bucket)
 * the sum rounded, then the product rounded (no contraction); k == 1 gives inv_k == 1.0f.
 *
 * hyb_grad_accumulate: acc[i][e] = acc[i][e] + grads[i][e] for every tensor of the table in one launch (80 tensors per launch, more
 * tensors = more launches); 4096-element chunks, 16-byte accesses where both pointers are aligned; grads is only read.  3 x 4 bytes
 * per parameter.  -1 for a NULL array or entry, acc[i] == grads[i], numel[i] <= 0, count <= 0, or a table of 2^31 or more chunks in all,
 * decided before the first launch. */
int hyb_grad_accumulate(int count, float* const* acc, const float* const* grads, const long long* numel, void* stream);
/* hyb_grad_norm_acc: hyb_grad_norm over G -- the same workspace (hyb_grad_norm_workspace), the same summation order, the same final
 * launch, so the norm equals hyb_grad_norm over a materialised G bit for bit.  acc and grads are only read. */
int hyb_grad_norm_acc(int count, const float* const* acc, const float* const* grads /* or NULL */, const long long* numel, long long k,
                      float* partials, const double* hyper, float* norm_out /* [2] */, void* stream);
/* hyb_adamw_step_dev_acc: hyb_adamw_step_dev (ema == ema_hyper == NULL) or hyb_adamw_step_dev_ema (both given) with G in place of the
 * gradient (G * clip[1] follows as there), which also stores +0.0f to every element of acc in the same launch: 9 x 4 bytes per
 * parameter, 11 x 4 with the average, and no sum, scale or memset pass.  The step number used (bias corrections, the average's warm-up)
 * is step + (step_inc ? *step_inc / k : 0), integer division: the counter counts MICRO-steps, and an advancing call adds 1 to it like
 * every other micro-step does.  76 tensors per launch, 64 with the average.  -1 also for k < 1, a NULL acc entry, acc[i] == params[i],
 * ema without ema_hyper or the reverse. */
int hyb_adamw_step_dev_acc(int count, float* const* params, const float* const* grads /* or NULL */, float* const* exp_avg,
                           float* const* exp_avg_sq, float* const* acc, float* const* ema /* or NULL */, const long long* numel,
                           const double* hyper, const double* ema_hyper /* or NULL */, long long k, long long step, long long* step_inc,
                           unsigned int* advance_ticket, const float* clip /* norm_out of hyb_grad_norm_acc, or NULL */, void* stream);

/* ---- skipping an optimizer step whose gradients are not finite, decided on the device ---------------------------------------------------
 * (New symbols only; hyb_abi_version() stays 9.)  guard: a DEVICE block `long long guard[2]` = {skip_now, skipped_total}, owned by the
 * caller, zero before the first step.  One norm call and then the AdamW calls of every parameter group, stream-ordered, make one step.
 *
 * hyb_grad_norm_guard / hyb_grad_norm_acc_guard: hyb_grad_norm / hyb_grad_norm_acc -- the same chunk launches, the same final sum in the
 * same order, norm_out bit for bit as they write it -- whose final one-workgroup launch also writes skip_now = !isfinite(norm_out[0]) and
 * adds it to skipped_total: once per step, the only place that counts.  Not finite means a NaN or infinite element, or finite elements
 * whose sum of squares overflows fp32 (a single 1e20).  hyper[5] == 0 gives the coefficient 1 as ever: the guard without clipping.
 * On a skipped step norm_out[0] holds the non-finite norm and norm_out[1] is unspecified. */
int hyb_grad_norm_guard(int count, const float* const* grads, const long long* numel, float* partials, const double* hyper,
                        float* norm_out /* [2] */, long long* guard /* [2] */, void* stream);
int hyb_grad_norm_acc_guard(int count, const float* const* acc, const float* const* grads /* or NULL */, const long long* numel, long long k,
                            float* partials, const double* hyper, float* norm_out /* [2] */, long long* guard /* [2] */, void* stream);
/* hyb_adamw_step_dev_guard: every device-path step behind one call -- acc == NULL (then k == 1 and grads != NULL): hyb_adamw_step_dev, or
 * hyb_adamw_step_dev_ema when ema and ema_hyper are given; acc != NULL: hyb_adamw_step_dev_acc -- which reads guard[] when it runs.
 *   skip_now != 0: params, exp_avg, exp_avg_sq and ema get NO stores (not a rewrite of the old values); every element of acc gets +0.0f;
 *                  an advancing call advances the counter as ever (the counter also seeds dropout: the next replay draws new masks).
 *   skip_now == 0: the update of the unguarded call, bit for bit, at the step number
 *                      step + (step_inc ? *step_inc (/ k) : 0) - skipped_total
 *                  i.e. the number of APPLIED updates: a run with a skipped step has from then on the parameters of a run that never
 *                  attempted it.
 * clip must be the norm_out the step's norm call has written (never NULL). */
int hyb_adamw_step_dev_guard(int count, float* const* params, const float* const* grads /* or NULL */, float* const* exp_avg,
                             float* const* exp_avg_sq, float* const* acc /* or NULL */, float* const* ema /* or NULL */, const long long* numel,
                             const double* hyper, const double* ema_hyper /* or NULL */, long long k, long long step, long long* step_inc,
                             unsigned int* advance_ticket, const float* clip, const long long* guard /* [2] */, void* stream);

/* ---- parameter groups: one AdamW launch for all of them -----------------------------------------------------------------------------------
 * (New symbols only; hyb_abi_version() stays 9.)  Weight decay off for biases and norm parameters, a learning rate per layer: such recipes
 * are parameter groups, and with the calls above every group is a launch of its own.  The caller's DEVICE blocks are contiguous over the
 * groups -- `double hyper[groups, 6]`, `double ema_hyper[groups, 2]`, rows as above -- so one launch can serve them all: its tensor table
 * carries one byte per tensor, the group, and a workgroup forms its scalars from the row of its tensor's group.
 *
 * hyb_adamw_step_dev_groups: every device-path step over the tensors of SEVERAL groups behind one call.  group: a HOST array of `count`
 * bytes, group[i] < groups <= 255 the parameter group of tensor i (tensors of one group need not be adjacent); hyper, ema_hyper: the BASES
 * of the blocks.  acc == NULL (then k == 1 and grads != NULL): hyb_adamw_step_dev, or hyb_adamw_step_dev_ema when ema and ema_hyper are
 * given (all groups keep the average or none does); acc != NULL: hyb_adamw_step_dev_acc.  guard == NULL: the unguarded launches, clip may
 * be NULL; guard != NULL: hyb_adamw_step_dev_guard (clip is then the step's norm_out).  Every element of every tensor comes out bit for bit
 * as the call over its group alone, with that group's rows, gives it.  The counter is advanced once, by the last launch of the call, so an
 * advancing step may span several groups.  80 tensors per launch, 72 with acc, 64 with ema.  -1 as the calls it stands for, and for
 * group == NULL, a group[i] >= groups, groups < 1 or > 255. */
int hyb_adamw_step_dev_groups(int count, float* const* params, const float* const* grads /* or NULL */, float* const* exp_avg,
                              float* const* exp_avg_sq, float* const* acc /* or NULL */, float* const* ema /* or NULL */, const long long* numel,
                              const unsigned char* group, int groups, const double* hyper /* [groups, 6] */,
                              const double* ema_hyper /* [groups, 2], or NULL */, long long k, long long step, long long* step_inc,
                              unsigned int* advance_ticket, const float* clip /* or NULL */, const long long* guard /* [2], or NULL */, void* stream);
/* hyb_adamw_hyper_set_groups: hyb_adamw_hyper_set for `count` groups and hyb_adamw_ema_set for `ema_count` groups in ONE one-workgroup
 * launch: row group[i] of hyper gets values[6 i .. 6 i + 5], row ema_group[i] of ema_hyper gets ema_values[2 i], ema_values[2 i + 1].
 * group, values, ema_group, ema_values are HOST arrays, copied into the kernel arguments before the call returns (no staging memory, nothing
 * to keep alive); more than 60 rows of a block = more launches.  Either count may be 0 (its three pointers are then not read), not both.
 * NOT meant to be captured, as the calls it stands for.  -1 for a value they refuse, a group index >= groups or listed twice in one list,
 * groups < 1 or > 255. */
int hyb_adamw_hyper_set_groups(double* hyper /* [groups, 6] */, double* ema_hyper /* [groups, 2], or NULL */, int groups, int count,
                               const unsigned char* group, const double* values /* [count, 6] */, int ema_count,
                               const unsigned char* ema_group, const double* ema_values /* [ema_count, 2] */, void* stream);

/* ---- LAMB: layer-wise trust ratios in the fused step (You et al. 2020; timm's Lamb, apex FusedLAMB without nvlamb) -------------------------
 * (New symbols only; hyb_abi_version() stays 9.)  Per tensor, at applied step t, with G the effective gradient exactly as the AdamW launch
 * forms it (acc / grads / k as in hyb_adamw_step_dev_acc, times clip[1] when clip is given):
 *     m' = m + (1 - b1)(G - m)      v' = b2 v + (1 - b2) G^2                                      (the step's own expressions)
 *     q  = (m' / (1 - b1^t)) / (sqrt(v') / sqrt(1 - b2^t) + eps)        u = q + wd p
 *     r  = |p| / |u|  if (wd != 0 or always_adapt) and |p| > 0 and |u| > 0, else 1                 (L2 norms over the tensor)
 *     p <- p - lr r u
 * which is the AdamW step of that tensor at the rate r lr: one read-only pass forms the ratios, then the AdamW launch runs with them.
 *
 * hyb_lamb_trust: the pass.  The table, group / groups / hyper, k, step, step_inc, clip and guard are those of the hyb_lamb_step_dev call
 * that follows (grads / acc / group / clip / guard may be NULL as there; group == NULL: hyper is the one row).  It stores nothing to
 * params, the moments or acc.  fp32 per element, contraction off:
 *     u = fmaf((float)wd, p, (float)(1 / (1 - b1^t)) * (m' / fmaf(sqrtf(v'), (float)(1 / sqrt(1 - b2^t)), (float)eps)))
 * then p^2 and u^2 summed like hyb_grad_norm sums g^2 -- 4096-element chunks in a fixed order, two fp32 partials per chunk, a tensor's
 * partials in double in a fixed order by a second launch (one workgroup per tensor) -- so the ratios are bit-identical from run to run.
 * trust_out: DEVICE float [count, 3], row i = {|p_i|, |u_i|, r_i} over the WHOLE table (more than 80 tensors, 72 with acc: more launches);
 * r = (float)((double)|p| / (double)|u|).  wd is read from the tensor's row of hyper when the launch runs, always_adapt (0 or 1) travels by
 * value.  With guard, the step number is less skipped_total as in the guarded step; on a skipped step trust_out is unspecified (and unread).
 * partials: hyb_lamb_trust_workspace(count, numel) floats (2 per chunk; 0 for bad arguments), no state kept in it between calls.
 * 4 x 4 bytes read per parameter, 5 x 4 with acc and grads. */
size_t hyb_lamb_trust_workspace(int count, const long long* numel);
int hyb_lamb_trust(int count, float* const* params, const float* const* grads /* or NULL */, float* const* exp_avg, float* const* exp_avg_sq,
                   float* const* acc /* or NULL */, const long long* numel, const unsigned char* group /* or NULL */, int groups,
                   const double* hyper, long long k, long long step, long long* step_inc, const float* clip /* or NULL */,
                   const long long* guard /* [2], or NULL */, int always_adapt, float* partials, float* trust_out /* [count, 3] */, void* stream);
/* hyb_lamb_step_dev: hyb_adamw_step_dev_groups -- every variant behind it, the average, accumulation, the guard, the advancing counter -- in
 * which thread 0 of a workgroup forms its tensor's decay and step size from r lr, r = trust[3 i + 2], in double, rounded once: r == 1 gives
 * the AdamW step bit for bit.  group may be NULL here (hyper / ema_hyper are then the one group's rows, groups is not read).  trust: the
 * trust_out of the hyb_lamb_trust call of this step (never NULL); on a guarded skip it is not read. */
int hyb_lamb_step_dev(int count, float* const* params, const float* const* grads /* or NULL */, float* const* exp_avg,
                      float* const* exp_avg_sq, float* const* acc /* or NULL */, float* const* ema /* or NULL */, const long long* numel,
                      const unsigned char* group /* or NULL */, int groups, const double* hyper, const double* ema_hyper /* or NULL */,
                      long long k, long long step, long long* step_inc, unsigned int* advance_ticket, const float* clip /* or NULL */,
                      const long long* guard /* [2], or NULL */, const float* trust /* [count, 3] */, void* stream);

/* ---- SGD with momentum, and LARS, in the fused step (torch.optim.SGD's rule; timm's Lars with trust_clip = False) ----------------------------
 * (New symbols only; hyb_abi_version() stays 9.)  One state tensor per parameter, the momentum buffer: the launch moves 5 x 4 bytes per
 * parameter (it reads p, g, buf and writes p, buf) where the AdamW launch moves 7 x 4.  The device block `double hyper[groups, 6]` is read
 * as {lr, momentum, dampening, lars_eps, weight_decay, max_grad_norm}: hyb_adamw_hyper_set, hyb_adamw_hyper_set_groups, hyb_adamw_ema_set,
 * the four hyb_grad_norm* and hyb_grad_accumulate serve SGD unchanged (their range checks -- columns 1 and 2 in [0, 1), column 3 >= 0 -- are
 * the ranges wanted here).
 *
 * The rule.  Per element of a tensor at applied step t -- t = step + *step_inc (/ k when accumulating) - skipped_total, the step number of
 * the AdamW launch -- with the effective gradient exactly as the AdamW launch forms it (acc / grads / k as in hyb_adamw_step_dev_acc, then
 * times clip[1] when clip is given), in fp32 with contraction off and every fused multiply-add written out:
 *     G    = eff_grad(acc, g, 1 / k) * clip
 *     d    = fmaf(wd32, p, G)                      coupled L2 decay, torch.optim.SGD's
 *     d    = r * d                                 LARS only (trust != NULL); r = trust[3 i + 2], the tensor's trust ratio
 *     buf' = (t == 1) ? d : fmaf(mu32, buf, omt32 * d)
 *     s    = nesterov ? fmaf(mu32, buf', d) : (mu32 == 0) ? d : buf'
 *     p'   = fmaf(-lr32, s, p)
 *     e'   = fmaf(d32, e, omd32 * p')              where the call keeps the average (ema, ema_hyper: as hyb_adamw_step_dev_ema)
 * mu32 = (float)momentum, omt32 = (float)(1.0 - dampening), wd32 = (float)weight_decay, lr32 = (float)lr: each rounded once from the doubles
 * of the tensor's row of hyper, by thread 0 of the workgroup when the launch runs.  At t == 1 the old buffer value does not reach the
 * result (a select, not a product with 0): a buffer full of NaNs gives buf' = d.  With momentum == 0 torch.optim.SGD keeps no buffer and
 * steps on d itself, whatever the dampening: so does this rule (s = d, again a select); the buffer is still written and never read back into p.
 *
 * hyb_sgd_step_dev: every variant behind one entry point, the arguments of hyb_adamw_step_dev_groups with ONE state table (momentum_buf),
 * `nesterov` (0 or 1, by value) and `trust` (NULL: plain SGD; else the trust_out of this step's hyb_lars_trust call, not read on a guarded
 * skip).  NULL where a call has no such thing, under the rule of the AdamW steps: grads (acc holds the whole sum), acc (then k == 1 and
 * grads != NULL), ema together with ema_hyper, group (hyper / ema_hyper are then the one group's rows, groups is not read), step_inc,
 * advance_ticket (needs step_inc), clip, guard (needs clip).  A guarded skip stores nothing to p / buf / e, stores +0.0f over the
 * accumulators and takes its ticket; the accumulators are left +0.0f by every step; the last launch of the call advances the counter.
 * 80 tensors per launch, 72 with acc and ema together.  -1 as hyb_adamw_step_dev_groups, and for a nesterov other than 0 or 1. */
int hyb_sgd_step_dev(int count, float* const* params, const float* const* grads /* or NULL */, float* const* momentum_buf,
                     float* const* acc /* or NULL */, float* const* ema /* or NULL */, const long long* numel,
                     const unsigned char* group /* or NULL */, int groups, const double* hyper, const double* ema_hyper /* or NULL */,
                     long long k, long long step, long long* step_inc, unsigned int* advance_ticket, const float* clip /* or NULL */,
                     const long long* guard /* [2], or NULL */, int nesterov, const float* trust /* [count, 3], or NULL */, void* stream);
/* hyb_lars_trust: LARS's layer-wise ratios for the hyb_sgd_step_dev call that follows (the same params / grads / acc / numel / group /
 * groups / hyper / k / clip / guard).  Per tensor, wn = |p| and gn = |G| (L2 norms, G the effective, clipped gradient above):
 *     r = trust_coeff wn / (gn + wn wd + eps)      in double from the fp32 norms, rounded once
 *     r = 1  where wn == 0 or gn == 0, and for every tensor of a group with weight_decay == 0 unless always_adapt
 * wd and eps (columns 4 and 3) are read from the tensor's row of hyper when the launch runs; trust_coeff (> 0, finite) and always_adapt
 * (0 or 1) travel by value.  A read-only pass (2 x 4 bytes per parameter, 3 x 4 with acc and grads): p^2 and G^2 summed like hyb_grad_norm
 * sums g^2 -- 4096-element chunks in a fixed order, two fp32 partials per chunk, a tensor's partials in double in a fixed order by a
 * second launch (one workgroup per tensor) -- so the ratios are bit-identical from run to run and independent of how the table is cut
 * into launches.  trust_out: DEVICE float [count, 3], row i = {wn_i, gn_i, r_i}.  On a step the guard skips, trust_out is unspecified (and
 * unread).  partials: hyb_lars_trust_workspace(count, numel) floats (2 per chunk; 0 for bad arguments), no state kept between calls.
 * -1 under the rule of the step (acc with k, guard needs clip, the group range), for trust_coeff or always_adapt out of range, and for
 * partials or trust_out NULL. */
size_t hyb_lars_trust_workspace(int count, const long long* numel);
int hyb_lars_trust(int count, float* const* params, const float* const* grads /* or NULL */, float* const* acc /* or NULL */,
                   const long long* numel, const unsigned char* group /* or NULL */, int groups, const double* hyper, long long k,
                   const float* clip /* or NULL */, const long long* guard /* [2], or NULL */, double trust_coeff, int always_adapt,
                   float* partials, float* trust_out /* [count, 3] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYBRID_HIP_H_ */
