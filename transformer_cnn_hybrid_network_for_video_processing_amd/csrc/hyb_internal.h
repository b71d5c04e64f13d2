// What the .hip files share on the HOST side outside the C ABI (include/hybrid_hip.h): one prototype per internal function (the defining
// file includes this header too: a changed signature is a compile error there, not a link-time surprise), default arguments only here, the
// helpers every workspace layout uses, the one way a switch is read.  (hyb_stage1w_* take S1Args: declared next to it, conv_first.h.)
// Workspace rule: a workspace is described ONCE, by a `struct ...Layout { size_t <offsets...>, total; }` and an inline builder that
// walks it with a take() lambda (EncLayout in model.hip is the model).  The size query returns .total, the entry point takes every
// pointer from the same struct.  Add a region in the layout function and nowhere else.
#pragma once
#include <stdlib.h>
#include "hyb_common.h"

#define HYB_TRY(call) do { int rc_ = (call); if (rc_ != 0) return rc_; } while (0)
#define HYB_HIP_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (int)e_; } while (0)

// internal "no kernel variant takes this shape: use the other path" return of hyb_conv_v2*, hyb_gemm_nt_ln, hyb_gemm_skinny_wf32 (not an ABI status)
constexpr int HYB_NO_VARIANT = -100;

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int padc(int c) { return (c + 31) / 32 * 32; }

// An environment switch, read once per call site: `static const int x = hyb_env_int("HYB_...", dflt);`
inline int hyb_env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
// The switches more than one function consults: every reader calls the accessor, so they cannot disagree.
inline int hyb_sw_conv_v2() { static const int v = hyb_env_int("HYB_CONV_V2", 1); return v; }                  // asynchronous bf16 conv3x3 (conv_v2.hip)
inline int hyb_sw_wgrad_v2() { static const int v = hyb_env_int("HYB_WGRAD_V2", 1); return v; }                // warp-specialised weight gradient
inline int hyb_sw_wgrad_v3() { static const int v = hyb_env_int("HYB_WGRAD_V3", 1); return v; }                // its third generation (fused, conv_wgrad_v3.h)
inline int hyb_sw_s1_wave() { static const int v = hyb_env_int("HYB_S1_WAVE", 1); return v; }                  // stage 1: wave-private forward passes
inline int hyb_sw_s1_wave_bwd() { static const int v = hyb_env_int("HYB_S1_WAVE_BWD", 1); return v; }          // stage 1: wave-private backward pass
inline int hyb_sw_s1_gram() { static const int v = hyb_env_int("HYB_S1_GRAM", 1); return v; }                  // stage 1: statistics from the Gram matrix
inline int hyb_sw_conv_implicit() { static const int v = hyb_env_int("HYB_CONV_IMPLICIT", 1); return v; }      // FCT: implicit-GEMM convolutions

// attention.hip
int hyb_attention_fwd_packed(int dtype, const void* qkv, const float* mask, void* out, float* stats, int B, int S, int D, int H, float p_drop,
                             unsigned long long seed, const unsigned long long* seed_inc, hipStream_t st);
int hyb_attention_bwd_packed(int dtype, const void* qkv, const float* mask, const float* stats, const void* dout, void* dqkv, int B, int S, int D, int H,
                             float p_drop, unsigned long long seed, const unsigned long long* seed_inc, hipStream_t st, int relu_out);
int hyb_flash_attention_fwd(int dtype, const void* q, const void* k, const void* v, void* out, float* lse, int N, int L, int H, int dhp, int ld, float scale,
                            hipStream_t st, int dh_true);
int hyb_flash_attention_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta_ws, void* dq,
                            void* dk, void* dv, int N, int L, int H, int dhp, int ld, float scale, hipStream_t st, int dh_true);
// bn_pool.hip
int hyb_bn_infer_affine_many(int n, const float* const* gamma, const float* const* beta, const float* const* mean, const float* const* var,
                             float* const* scale_shift, const int* Co, const int* Cop, float eps, hipStream_t st);
int hyb_bn_relu_apply_pooled(int dtype, void* pooled, const float* ss, int N, int Ho, int Wo, int Cop, hipStream_t st);
int hyb_gap_fwd_h16(const void* x, float* feat, int N, int HW, int Cp, hipStream_t st);
int hyb_gap_bwd_h16(const float* dfeat, void* dx, int N, int HW, int Cp, hipStream_t st);
// conv_first.hip
size_t hyb_stage1_fwd_workspace(int dtype, int Cop);
size_t hyb_stage1_bwd_workspace(int dtype, int Cop);
long long hyb_stage1_route_elems(int dtype, int N, int H, int W, int Cop);
int hyb_stage1_fwd(int dtype, const float* x, const float* weight, const float* gamma, const float* beta, float* running_mean, float* running_var, long long* nbt,
                   int training, float momentum, float eps, int N, int H, int W, int Ci, int Co, int Cop, void* pooled, float* scale_shift, float* mean_invstd,
                   void* packed_out, void* workspace, float* running_out, int prepacked, void* route, hipStream_t st);
int hyb_stage1_bwd(int dtype, const void* dpooled, const float* x, const float* weight, const float* gamma, const float* scale_shift, const float* mean_invstd,
                   int training, int N, int H, int W, int Ci, int Co, int Cop, float* dweight, float* dgamma, float* dbeta, const void* packed_in, void* workspace,
                   const void* route, hipStream_t st);
int hyb_stage1_infer(int dtype, const float* x, const float* weight, const float* scale_shift, int N, int H, int W, int Ci, int Co, int Cop, void* pooled,
                     void* prepacked, void* workspace, hipStream_t st);
// conv_fwd.hip
int hyb_conv_dgrad_planar_ok(int dtype, int W, int Cin_p, int Cout_p);
int hyb_conv3x3_fwd_ext(const void* x, const void* wp, void* y, float* part, void* pooled, const float* gamma, int Co, int N, int H, int W, int Cip, int Cop,
                        hipStream_t st);
int hyb_conv3x3_planar_in(const void* x, const void* wp, void* y, int N, int H, int W, int Cin_p, int Cout_p, hipStream_t st);
int hyb_conv_pack_weight_dual(int dtype, const float* w, void* wp0, void* wp1, int Co, int Ci, int Cop, int Cip, hipStream_t st);
int hyb_conv_pack_weight_many(int dtype, int n, const float* const* w, void* const* wp0, void* const* wp1, const int* Co, const int* Ci, const int* Cop,
                              const int* Cip, const float* s1_w, void* s1_wp, int s1_Co, int s1_Ci, int s1_Cop, hipStream_t st);
int hyb_conv_pack_weight_fwd_many(int dtype, int n, const float* const* w, void* const* wp0, const int* Co, const int* Ci, const int* Cop, const int* Cip,
                                  const float* s1_w, void* s1_wp, int s1_Co, int s1_Ci, int s1_Cop, hipStream_t st);
// conv_v2.hip (the plan: conv_plan.h, conv_fwd_plan of the same shape)
struct ConvFwdPlan;
int hyb_conv_v2(const ConvFwdPlan& p, const void* x, const void* wp, void* y, float* part, int N, int H, int W, int Cip, int Cop, hipStream_t st, long long xblk = 0);
int hyb_conv_v2_pool(const ConvFwdPlan& p, const void* x, const void* wp, void* pooled, const float* ss, int N, int H, int W, int Cip, int Cop, hipStream_t st);
int hyb_conv_v2_ext(const ConvFwdPlan& p, const void* x, const void* wp, void* y, float* part, void* pooled, const float* gamma, int Co, int N, int H, int W, int Cip, int Cop,
                    hipStream_t st);
// conv_wgrad.hip
int hyb_wgrad_reduce_multi(int n, const HybSlabInfo* infos, hipStream_t st);
int hyb_wgrad_v2_supported(int dtype, int W, int Cip, int Cop);
int hyb_conv3x3_wgrad_fused(int dtype, const void* x, const void* y, const void* dp, const float* ss, const float* mi, const float* gamma, const float* sums,
                            int training, long long count, void* dyraw_out, long long dyraw_blk, float* dw, int N, int H, int W, int Ci, int Cip, int Co, int Cop,
                            void* workspace, size_t workspace_bytes, hipStream_t st, HybSlabInfo* defer);
// layernorm.hip
int hyb_ln_residual_fwd_inc(int dtype, const void* x, const void* skip, const float* gamma, const float* beta, void* y, float* stats, int M, int D, float eps,
                            float out_scale, float p_drop, unsigned long long seed, const unsigned long long* seed_inc, void* stream);
int hyb_ln_bwd_rows(int M);
int hyb_ln_residual_bwd_rows(int dtype, const void* dy, const void* x, const float* gamma, const float* stats, void* dx, void* dskip, int accumulate_dskip,
                             float* part, int M, int D, float out_scale, float p_drop, unsigned long long seed, const unsigned long long* seed_inc,
                             hipStream_t st);
int hyb_ln_rows_reduce(const float* part, int rows, int D, float* dgamma, float* dbeta, hipStream_t st);
int hyb_temporal_tail_ok(int B, int S, int D, int C, int ln_rows);
// the cross-entropy loss's options as the *_opts_* entry points and kernels carry them (weight: [C] device floats, or nullptr = all ones)
struct HybCeOpts { const float* weight; long long ignore_index; int has_ignore; float label_smoothing; };
int hyb_ce_opts_ok(const HybCeOpts& o);                    // (the evaluation meter's check too)
// the second target and the mixing weight of every clip as the *_mix_* entry points and kernels carry them ([B] each, device memory)
struct HybCeMix { const long long* target_b; const float* lam; };
// a dense target as the *_dense_* entry points and kernels carry it: target [B][C] fp32 rows; kind 0: class probabilities (soft-target
// cross-entropy), kind 1: per-class binary targets (BCE with logits; pos_weight [C] or nullptr = all ones).  label_smoothing and weight
// travel in HybCeOpts (whose ignore fields are unused).
struct HybCeDense { const float* target; const float* pos_weight; int kind; };
// the focusing scalars as the *_focal_* / *_asym_* entry points and kernels carry them, by value.  Index focal: gamma (gamma_neg and clip
// are 0), beside HybCeOpts (no label smoothing).  Asymmetric: gamma is the positives' exponent, gamma_neg the negatives', clip the
// probability shift m in [0, 1), beside HybCeOpts (weight only) and a HybCeDense of kind 1 (target, pos_weight).
struct HybCeFocal { float gamma; float gamma_neg; float clip; };
// One loss, described once from the entry point to the kernel launch.  mode == the MODE template argument of temporal_tail_{fwd,bwd}_body
// and of the two meter kernels eval_metrics_kernel / eval_multilabel_kernel (layernorm.hip); the members a mode does not read stay zero.  target: class indices [B] (PLAIN, OPTS, MIX, FOCAL); the dense modes
// (SOFT = HybCeDense kind 0, BCE = kind 1, ASYM) carry theirs in d.  hyb_loss_*(): the members each family of entry points fills.
enum HybLossMode { HYB_LOSS_PLAIN = 0, HYB_LOSS_OPTS, HYB_LOSS_MIX, HYB_LOSS_SOFT, HYB_LOSS_BCE, HYB_LOSS_FOCAL, HYB_LOSS_ASYM };
struct HybLoss { int mode; const long long* target; HybCeOpts o; HybCeMix m; HybCeDense d; HybCeFocal f; };
inline bool hyb_loss_is_dense(int mode) { return mode == HYB_LOSS_SOFT || mode == HYB_LOSS_BCE || mode == HYB_LOSS_ASYM; }
inline HybLoss hyb_loss_plain(const long long* target) { return {HYB_LOSS_PLAIN, target}; }
inline HybLoss hyb_loss_opts(const long long* target, const float* weight, long long ignore_index, int has_ignore, float label_smoothing) {
    return {HYB_LOSS_OPTS, target, {weight, ignore_index, has_ignore, label_smoothing}};
}
inline HybLoss hyb_loss_mix(const long long* target, const long long* target_b, const float* lam, const float* weight, long long ignore_index,
                            int has_ignore, float label_smoothing) {
    return {HYB_LOSS_MIX, target, {weight, ignore_index, has_ignore, label_smoothing}, {target_b, lam}};
}
inline HybLoss hyb_loss_dense(const float* target, const float* weight, const float* pos_weight, int kind, float label_smoothing) {
    return {kind == 1 ? HYB_LOSS_BCE : HYB_LOSS_SOFT, nullptr, {weight, 0, 0, label_smoothing}, {}, {target, pos_weight, kind}};
}
inline HybLoss hyb_loss_focal(const long long* target, const float* weight, long long ignore_index, int has_ignore, float gamma) {
    return {HYB_LOSS_FOCAL, target, {weight, ignore_index, has_ignore, 0.f}, {}, {}, {gamma, 0.f, 0.f}};
}
inline HybLoss hyb_loss_asym(const float* target, const float* weight, const float* pos_weight, float gamma_pos, float gamma_neg, float clip) {
    return {HYB_LOSS_ASYM, nullptr, {weight, 0, 0, 0.f}, {}, {target, pos_weight, 1}, {gamma_pos, gamma_neg, clip}};
}
// the one validity rule: the mode's target is there, and its members are in the ranges include/hybrid_hip.h states
int hyb_loss_ok(const HybLoss& l);
// the stand-alone launches (ce_*_kernel) of any mode: what the hyb_cross_entropy*_{fwd,bwd} entry points are, and what the temporal part
// runs behind the head where the tail kernels do not take the shape
int hyb_loss_fwd(const HybLoss& l, const float* logits, float* loss, int B, int C, hipStream_t st);
int hyb_loss_bwd(const HybLoss& l, const float* logits, const float* dloss, float* dlogits, int B, int C, hipStream_t st);
// l != nullptr: the loss in the same one launch (forward: into loss, with ce_scratch; backward: from the saved logits and dloss);
// l == nullptr: logits only / the caller's dlogits
int hyb_temporal_tail_fwd(int dtype, const void* f, const void* x1, const float* gamma, const float* beta, void* enc_out, float* stats, int B, int S, int D,
                          float eps, float out_scale, float p_drop, unsigned long long seed, const unsigned long long* seed_inc, const float* W, const float* bias,
                          float* logits, int C, float* loss, float* ce_scratch, hipStream_t st, const HybLoss* l);
int hyb_temporal_tail_bwd(int dtype, const float* dlogits, const float* logits, const float* dloss, const float* W, const void* enc_out, const void* f,
                          const float* gamma, const float* stats, void* dx, void* dskip, float* ln_part, int ln_rows, float* head_part, int B, int S, int D, int C,
                          float out_scale, float p_drop, unsigned long long seed, const unsigned long long* seed_inc, hipStream_t st, const HybLoss* l);
// linear.hip
int hyb_linear_bwd_wt(int dtype, const void* x, int ldx, const float* W, const void* Wt, const void* y, const void* dy, void* dx, int accumulate_dx, float* dW,
                      float* db, int M, int N, int K, int relu, void* ws, size_t ws_bytes, hipStream_t st);
int hyb_gemm_nt(int dtype, int groups, const void* const* A, const void* const* B, void* const* C, const float* const* bias, int out_f32, int Mo, int No, int R,
                int lda, int ldb, int ldc, int relu, int accumulate, hipStream_t st, const void* const* Amask = nullptr, const void* const* Cmask = nullptr);
int hyb_gemm_nt_ln(int dtype, int groups, const void* x, const void* skip, const float* gamma, const float* beta, void* y, float* stats, float eps, float out_scale,
                   float p_drop, unsigned long long seed, const unsigned long long* seed_inc, const void* const* B, void* const* C, const float* const* bias,
                   int Mo, int No, int R, int ldb, int ldc, int relu, hipStream_t st);
int hyb_gemm_skinny_wf32(int dtype, const void* A, const float* Bf, void* C, const float* bias, int Mo, int No, int R, int lda, int ldb, int ldc, int relu,
                         int accumulate, int transposed_b, hipStream_t st);
bool hyb_conv_implicit_ok(int Ci, long long rows);
int hyb_conv_implicit_gemm(const float* x, const float* wp, const float* bias, float* y, int n_img, int H, int W, int Ci, int Ho, int Wo, int Co, int Kp, int k,
                           int stride, int pad, int dil, int ldy, int relu, hipStream_t st);
int hyb_linear_dw_grouped(int dtype, int groups, const void* const* dy, const void* const* mask, const void* x, float* const* dW, float* const* db, int M, int N,
                          int K, int lddy, int ldx, hipStream_t st);
int hyb_linear_dw_multi(int dtype, int groups, const void* const* dy, const void* const* mask, const void* const* x, float* const* dW, float* const* db,
                        const int* N, const int* K, const int* lddy, const int* ldx, int M, hipStream_t st, int nriders, const HybDwRider* riders);
int hyb_convert_weights(int dtype, int count, const float* const* W, void* const* Wc, void* const* Wt, const int* N, const int* K, const int* ldt, hipStream_t st);
// model.hip
int hyb_convstage_fwd_impl(int dtype, int first, const void* x, const float* weight, const float* gamma, const float* beta, float* running_mean, float* running_var,
                           long long* nbt, int training, float momentum, float eps, int N, int H, int W, int Ci, int Cip, int Co, int Cop, void* y_raw,
                           void* pooled, float* scale_shift, float* mean_invstd, void* packed_bwd, float* running_out, void* workspace, size_t workspace_bytes,
                           void* stream, const void* prepacked_fwd);
int hyb_convstage_infer_core(int dtype, int first, const void* x, const float* weight, const float* scale_shift, int N, int H, int W, int Ci, int Cip, int Co,
                             int Cop, void* pooled, const void* prepacked, void* pack_ws, void* y_raw, void* s1_ws, void* stream);
int hyb_convstage_bwd_impl(int dtype, int first, const void* dpooled, const void* x, const void* y_raw, const void* pooled, const float* weight, const float* gamma,
                           const float* scale_shift, const float* mean_invstd, int training, int N, int H, int W, int Ci, int Cip, int Co, int Cop, void* dx,
                           float* dweight, float* dgamma, float* dbeta, const void* packed_bwd, void* workspace, size_t workspace_bytes, void* stream,
                           void* slab_ws, HybSlabInfo* defer);
size_t hyb_encoder_xin_offset(int dtype, int B, int S, int D, int Hid, int H);
int hyb_encoder_fwd_impl(int dtype, const void* x, const float* mask, const float* const* params, void* out, void* saved, int B, int S, int D, int Hid, int L,
                         int H, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* stream, HybEncTail* tail);
HybEncBwdTail hyb_encoder_bwd_tail(int dtype, const float* const* params, const void* saved, void* workspace, int B, int S, int D, int Hid, int L, int H,
                                   float layer_p, unsigned long long seed);
int hyb_encoder_bwd_impl(int dtype, const void* dout, const float* mask, const float* const* params, float* const* grads, const void* saved, void* dx, int B, int S,
                         int D, int Hid, int L, int H, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* workspace,
                         size_t workspace_bytes, void* stream, const HybDwExtra* extra, int tail_done, const HybDwRider* extra_rider);
