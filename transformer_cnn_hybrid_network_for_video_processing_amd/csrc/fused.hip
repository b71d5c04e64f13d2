// Model-level entry points: the whole CNN backbone and the whole temporal part (frame tokens -> TransformerEncoder -> head) as
// ONE C call each way.  They only chain the stage-level entry points of this library on the caller's stream; what they save is
// host time: a training step becomes three operator calls each way instead of seven, which keeps the step GPU-bound.
//   hyb_backbone_{fwd,bwd} : `stages` x [Conv3x3 -> BatchNorm2d -> ReLU -> MaxPool2d]   (UNet.py:58-60 + UNet.py:13, UNet.py:32-37 order)
//   hyb_temporal_{fwd,bwd} : global-average-pool + Linear frame token (composite's own) -> TransformerEncoder.forward
//                            (TransformerEncoder.pyc src L110-126) -> mean over T + Linear head (composite's own)
#include "hyb_common.h"
#include "hyb_internal.h"

namespace {
inline size_t smax(size_t a, size_t b) { return a > b ? a : b; }

// Training forward: the per-stage scratch (reused by every stage: the stages are ordered on the stream; stage_bytes = the largest need),
// then one forward weight pack per non-first stage: all of them are written by ONE launch before the first convolution
struct BackboneFwdLayout { size_t stage_ws, stage_bytes, pack[16], total; };
inline BackboneFwdLayout backbone_fwd_layout(int dtype, int stages, const int* channels) {
    const size_t es = dtype == HYB_F32 ? 4 : 2;
    BackboneFwdLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al256(bytes); return o; };
    size_t b = 0;
    for (int s = 0; s < stages; ++s) b = smax(b, hyb_convstage_fwd_workspace(dtype, s == 0, s == 0 ? 0 : padc(channels[s]), padc(channels[s + 1])));
    L.stage_bytes = al256(b);
    L.stage_ws = take(b);
    for (int s = 1; s < stages; ++s) {
        const size_t o = take((size_t)hyb_conv_packed_elems(0, padc(channels[s]), padc(channels[s + 1])) * es);
        if (s < 16) L.pack[s] = o;                           // (the entry point takes at most 16 stages; the query sizes any count)
    }
    L.total = off;
    return L;
}

// Training backward: the per-stage scratch (stage_bytes = the largest need), two ping-pong d(stage input) buffers, then the weight-gradient
// slabs of stages 2.., which outlive their stage: their fixed-order sums are ONE launch at the end of the backward (they feed only the
// optimizer).  Up to four stages are deferred (the first ones met walking backwards); slab[s] = (size_t)-1 for a stage that is not.
struct BackboneBwdLayout { size_t stage_ws, stage_bytes, dx[2], slab[16], total; };
inline BackboneBwdLayout backbone_bwd_layout(int dtype, int stages, const int* channels, int N, int H, int W) {
    const size_t es = dtype == HYB_F32 ? 4 : 2;
    BackboneBwdLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al256(bytes); return o; };
    size_t stage = 0, dx_bytes = 0;
    for (int s = 0, h = H, w = W; s < stages; ++s, h /= 2, w /= 2) {      // (stage s works on H >> s x W >> s pixels)
        stage = smax(stage, hyb_convstage_bwd_workspace(dtype, s == 0, N, h, w, s == 0 ? 0 : padc(channels[s]), padc(channels[s + 1])));
        if (s > 0) dx_bytes = smax(dx_bytes, (size_t)N * h * w * padc(channels[s]) * es);      // d(input of stage s) = d(pooled of stage s-1)
    }
    L.stage_bytes = al256(stage);
    L.stage_ws = take(stage);
    for (int j = 0; j < 2; ++j) L.dx[j] = take(dx_bytes);
    int deferred = 0;
    for (int s = 0; s < 16; ++s) L.slab[s] = (size_t)-1;
    for (int s = stages - 1; s >= 1 && deferred < 4; --s, ++deferred) {
        const size_t o = take(hyb_conv3x3_wgrad_workspace(0, N, H >> s, W >> s, padc(channels[s]), padc(channels[s + 1])));
        if (s < 16) L.slab[s] = o;                           // (the entry point takes at most 16 stages; the query sizes any count)
    }
    L.total = off;
    return L;
}

// (the head's per-clip weight / bias gradient rows of the fused tail, [B][C*D + C] floats, are sized for the largest class count the head takes: 64)
inline size_t head_part_bytes(int B, int D) { return al256((size_t)B * ((size_t)64 * D + 64) * sizeof(float)); }

// Workspace of the temporal backward: the encoder backward's own workspace (enc_bytes of it), d(encoder output), d(tokens), d(frame features)
// with the padded channels zero (dfeat_bytes), the head's partial rows
struct TemporalBwdLayout { size_t enc_ws, enc_bytes, denc, dtok, dfeat, dfeat_bytes, head_part, total; };
inline TemporalBwdLayout temporal_bwd_layout(int dtype, int B, int S, int Cp, int D, int Hid, int L, int H) {
    const size_t es = dtype == HYB_F32 ? 4 : 2;
    const size_t M = (size_t)B * S;
    TemporalBwdLayout T;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al256(bytes); return o; };
    T.enc_bytes = al256(hyb_encoder_workspace_bytes(dtype, B, S, D, Hid, L, H));
    T.enc_ws = take(T.enc_bytes);
    T.denc = take(M * D * es);
    T.dtok = take(M * D * es);
    T.dfeat_bytes = al256(M * Cp * es);
    T.dfeat = take(T.dfeat_bytes);
    T.head_part = take(head_part_bytes(B, D));
    T.total = off;
    return T;
}
}  // namespace

extern "C" size_t hyb_backbone_fwd_workspace(int dtype, int stages, const int* channels) {
    if (stages < 1 || !channels) return 0;
    return backbone_fwd_layout(dtype, stages, channels).total;
}

extern "C" int hyb_backbone_fwd(int dtype, int stages, const int* channels, const float* x, const float* const* params,
                                long long* const* num_batches_tracked, int training, float momentum, float eps, int N, int H, int W,
                                void* const* outs, void* workspace, size_t workspace_bytes, void* stream) {
    HYB_CHECK_ARG(stages >= 1 && stages <= 16 && channels && x && params && outs && workspace && N > 0);
    HYB_CHECK_ARG(channels[0] >= 1 && channels[0] <= 4);                  // the first stage reads NCHW fp32 frames directly
    const BackboneFwdLayout lay = backbone_fwd_layout(dtype, stages, channels);
    if (workspace_bytes < lay.total) return HYB_E_WORKSPACE;
    char* ws = (char*)workspace;
    const void* in = x;
    int h = H, w = W;
    // weight packs of stages 1.. (forward layout into the workspace behind the per-stage scratch, backward layout into the caller's saved
    // packed_bwd buffers) in one launch; a stage without a packed_bwd buffer packs by itself as before
    const void* prepacked[17] = {nullptr};
    {
        const float* pw[16]; void* p0[16]; void* p1[16]; int co[16], ci[16], cop[16], cip[16];
        int n = 0;
        for (int s = 1; s < stages; ++s) {
            void* bwdpack = outs[(size_t)s * 6 + 4];
            void* fwdpack = ws + lay.pack[s];
            if (!bwdpack) continue;
            pw[n] = params[(size_t)s * 5]; p0[n] = fwdpack; p1[n] = bwdpack;
            co[n] = channels[s + 1]; ci[n] = channels[s]; cop[n] = padc(channels[s + 1]); cip[n] = padc(channels[s]);
            prepacked[s] = fwdpack;
            ++n;
        }
        // the first stage's two layouts ([2][Cop][64] at the head of its packed_bwd buffer) ride in the same launch
        void* s1pack = outs[4];
        if (s1pack) prepacked[0] = s1pack;
        if (n > 0 || s1pack)
            HYB_TRY(hyb_conv_pack_weight_many(dtype, n, pw, p0, p1, co, ci, cop, cip, params[0], s1pack, channels[1], channels[0], padc(channels[1]),
                                              (hipStream_t)stream));
    }
    for (int s = 0; s < stages; ++s) {
        HYB_CHECK_ARG(h >= 2 && w >= 2);
        const float* const* P = params + (size_t)s * 5;
        void* const* O = outs + (size_t)s * 6;
        const int Ci = channels[s], Co = channels[s + 1];
        // training: running_out (O[5]) != NULL -> functional BatchNorm (the updated statistics go there, the inputs stay untouched);
        // NULL -> nn.BatchNorm2d's own in-place update of running_mean / running_var and num_batches_tracked += 1
        HYB_TRY(hyb_convstage_fwd_impl(dtype, s == 0, in, P[0], P[1], P[2], (float*)P[3], (float*)P[4],
                                       num_batches_tracked ? num_batches_tracked[s] : nullptr, training, momentum, eps, N, h, w, Ci,
                                       s == 0 ? 0 : padc(Ci), Co, padc(Co), O[0], O[1], (float*)O[2], (float*)O[3], O[4], training ? (float*)O[5] : nullptr,
                                       ws + lay.stage_ws, lay.stage_bytes, stream, prepacked[s]));
        in = O[1];
        h /= 2; w /= 2;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Inference backbone: all stages chained on the caller's stream; one launch for every stage's scale/shift, one for every weight pack, then one
// launch per stage (stage 1: apply + pool; stages 2..: conv with the affine + ReLU + pool epilogue, or the conv -> bn_relu_pool pair where
// hyb_conv3x3_pool_fused says 0).  Workspace: scale/shift rows | weight packs | stage-1 scratch | two pooled maps (ping-pong) | one y_raw (pair only)
namespace {
struct InferLayout { size_t ss[16], pack[16], s1_ws, buf[2], y_raw, total; };
inline bool infer_layout(int dtype, int stages, const int* channels, int N, int H, int W, InferLayout& L) {
    if ((dtype != HYB_F32 && dtype != HYB_BF16) || stages < 1 || stages > 16 || !channels || N <= 0 || channels[0] < 1 || channels[0] > 4) return false;
    const size_t es = dtype == HYB_F32 ? 4 : 2;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al256(bytes); return o; };
    for (int s = 0; s < stages; ++s) {
        if (channels[s + 1] < 1) return false;
        L.ss[s] = take(2 * (size_t)padc(channels[s + 1]) * 4);
    }
    L.pack[0] = take((size_t)padc(channels[1]) * 128 * es);
    for (int s = 1; s < stages; ++s) L.pack[s] = take((size_t)hyb_conv_packed_elems(0, padc(channels[s]), padc(channels[s + 1])) * es);
    L.s1_ws = take(hyb_stage1_fwd_workspace(dtype, padc(channels[1])));
    size_t bufb[2] = {0, 0}, yraw = 0;
    int h = H, w = W;
    for (int s = 0; s < stages; ++s) {
        if (h < 2 || w < 2) return false;
        const int Cop = padc(channels[s + 1]);
        if (Cop / 8 > 256) return false;
        if (s > 0 && !hyb_conv3x3_pool_fused(dtype, w, padc(channels[s]), Cop)) yraw = smax(yraw, (size_t)N * h * w * Cop * es);
        if (s < stages - 1) bufb[s & 1] = smax(bufb[s & 1], (size_t)N * (h / 2) * (w / 2) * Cop * es);
        h /= 2; w /= 2;
    }
    L.buf[0] = take(bufb[0]);
    L.buf[1] = take(bufb[1]);
    L.y_raw = take(yraw);
    L.total = off;
    return true;
}
}  // namespace

extern "C" size_t hyb_backbone_infer_workspace(int dtype, int stages, const int* channels, int N, int H, int W) {
    InferLayout L;
    return infer_layout(dtype, stages, channels, N, H, W, L) ? L.total : 0;
}

extern "C" int hyb_backbone_infer(int dtype, int stages, const int* channels, const float* x, const float* const* params, float eps, int N, int H, int W,
                                  void* pooled_last, void* workspace, size_t workspace_bytes, void* stream) {
    HYB_CHECK_ARG(stages >= 1 && stages <= 16 && channels && x && params && pooled_last && workspace && N > 0);
    InferLayout L;
    HYB_CHECK_ARG(infer_layout(dtype, stages, channels, N, H, W, L));
    for (int s = 0; s < stages * 5; ++s) HYB_CHECK_ARG(params[s]);
    if (workspace_bytes < L.total) return HYB_E_WORKSPACE;
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    {   // every stage's scale/shift from the running statistics: one launch
        const float* g[16]; const float* b[16]; const float* m[16]; const float* v[16]; float* ss[16]; int co[16], cop[16];
        for (int s = 0; s < stages; ++s) {
            const float* const* P = params + (size_t)s * 5;
            g[s] = P[1]; b[s] = P[2]; m[s] = P[3]; v[s] = P[4]; ss[s] = (float*)(ws + L.ss[s]); co[s] = channels[s + 1]; cop[s] = padc(channels[s + 1]);
        }
        HYB_TRY(hyb_bn_infer_affine_many(stages, g, b, m, v, ss, co, cop, eps, st));
    }
    {   // every stage's forward weight pack: one launch
        const float* pw[16]; void* p0[16]; int co[16], ci[16], cop[16], cip[16];
        for (int s = 1; s < stages; ++s) {
            pw[s - 1] = params[(size_t)s * 5]; p0[s - 1] = ws + L.pack[s];
            co[s - 1] = channels[s + 1]; ci[s - 1] = channels[s]; cop[s - 1] = padc(channels[s + 1]); cip[s - 1] = padc(channels[s]);
        }
        HYB_TRY(hyb_conv_pack_weight_fwd_many(dtype, stages - 1, pw, p0, co, ci, cop, cip, params[0], ws + L.pack[0], channels[1], channels[0],
                                              padc(channels[1]), st));
    }
    const void* in = x;
    int h = H, w = W;
    for (int s = 0; s < stages; ++s) {
        const int Ci = channels[s], Co = channels[s + 1];
        void* out = s == stages - 1 ? pooled_last : (void*)(ws + L.buf[s & 1]);
        HYB_TRY(hyb_convstage_infer_core(dtype, s == 0, in, params[(size_t)s * 5], (const float*)(ws + L.ss[s]), N, h, w, Ci, s == 0 ? 0 : padc(Ci), Co,
                                         padc(Co), out, ws + L.pack[s], nullptr, ws + L.y_raw, ws + L.s1_ws, stream));
        in = out;
        h /= 2; w /= 2;
    }
    return 0;
}

extern "C" size_t hyb_backbone_bwd_workspace(int dtype, int stages, const int* channels, int N, int H, int W) {
    if (stages < 1 || !channels || N <= 0) return 0;
    return backbone_bwd_layout(dtype, stages, channels, N, H, W).total;
}

extern "C" int hyb_backbone_bwd(int dtype, int stages, const int* channels, const void* dpooled_last, const void* pooled_last, const float* x,
                                const float* const* params,
                                const void* const* saved, int training, int N, int H, int W, float* const* grads, void* workspace,
                                size_t workspace_bytes, void* stream) {
    HYB_CHECK_ARG(stages >= 1 && stages <= 16 && channels && dpooled_last && x && params && saved && grads && workspace && N > 0);
    const BackboneBwdLayout lay = backbone_bwd_layout(dtype, stages, channels, N, H, W);
    if (workspace_bytes < lay.total) return HYB_E_WORKSPACE;
    char* ws = (char*)workspace;
    void* dxbuf[2] = {ws + lay.dx[0], ws + lay.dx[1]};
    HybSlabInfo pending[4];
    int npending = 0;
    const void* dp = dpooled_last;
    for (int s = stages - 1; s >= 0; --s) {
        const float* const* P = params + (size_t)s * 2;          // weight, gamma
        const void* const* S = saved + (size_t)s * 5;            // y_raw, stage input, scale_shift, mean_invstd, packed_bwd
        float* const* G = grads + (size_t)s * 3;                 // dweight, dgamma, dbeta
        const int Ci = channels[s], Co = channels[s + 1];
        void* dx = s == 0 ? nullptr : dxbuf[s & 1];
        const void* pooled = s + 1 < stages ? saved[(size_t)(s + 1) * 5 + 1] : pooled_last;      // a stage's output is the next stage's saved input
        const bool can_defer = s > 0 && lay.slab[s] != (size_t)-1;
        HybSlabInfo info{};
        HYB_TRY(hyb_convstage_bwd_impl(dtype, s == 0, dp, s == 0 ? (const void*)x : S[1], S[0], pooled, P[0], P[1], (const float*)S[2], (const float*)S[3],
                                       training, N, H >> s, W >> s, Ci, s == 0 ? 0 : padc(Ci), Co, padc(Co), dx, G[0], G[1], G[2], S[4], ws + lay.stage_ws,
                                       lay.stage_bytes, stream, can_defer ? ws + lay.slab[s] : nullptr, can_defer ? &info : nullptr));
        if (info.S > 0) pending[npending++] = info;
        dp = dx;
    }
    if (npending > 0) HYB_TRY(hyb_wgrad_reduce_multi(npending, pending, (hipStream_t)stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
extern "C" size_t hyb_temporal_bwd_workspace(int dtype, int B, int S, int HW, int Cp, int D, int Hid, int L, int H) {
    if (B <= 0 || S <= 0 || D <= 0) return 0;
    return temporal_bwd_layout(dtype, B, S, Cp, D, Hid, L, H).total;
}

// The tail of the temporal part runs as ONE launch each way when the shapes allow (hyb_temporal_tail_ok): forward = the last layer's second
// LayerNorm + head (+ the loss when one is described), backward = (the loss backward +) head backward + that LayerNorm's backward.
// HYB_TEMPORAL_TAIL=0: the separate launches (A/B; same results up to the order of two fixed-order sums).  l: the loss (hyb_internal.h,
// HybLoss), in the tail's launch or -- shapes the tail does not take -- as hyb_loss_fwd / hyb_loss_bwd behind / in front of the head;
// nullptr: logits only / the caller's dlogits.
static int tail_enabled() { static const int env = hyb_env_int("HYB_TEMPORAL_TAIL", 1); return env; }

static int temporal_fwd_impl(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                             const float* head_w, const float* head_b, const float* mask, void* feat, void* tok, void* enc_saved,
                             void* enc_out, float* logits, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes,
                             float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc, float* loss,
                             float* ce_scratch, void* stream, const HybLoss* l) {
    HYB_CHECK_ARG(h && token_w && enc_params && head_w && feat && tok && enc_saved && enc_out && logits && B > 0 && S > 0 && HW > 0);
    HYB_CHECK_ARG(!l || (loss && ce_scratch && hyb_loss_ok(*l)));
    const int N = B * S;
    const bool h16 = (dtype & HYB_H_BF16) != 0;                 // the pooled map is bf16, everything from the frame features on is fp32
    dtype &= 0xff;
    HYB_CHECK_ARG(!h16 || dtype == HYB_F32);
    if (h16) HYB_TRY(hyb_gap_fwd_h16(h, (float*)feat, N, HW, Cp, (hipStream_t)stream));
    else HYB_TRY(hyb_gap_fwd(dtype, h, feat, N, HW, Cp, stream));
    // the tokens are written straight into the encoder's saved input slot (`tok` stays an unused scratch argument of the ABI)
    void* tok_dst = (char*)enc_saved + hyb_encoder_xin_offset(dtype, B, S, D, Hid, H);
    (void)tok;
    HYB_TRY(hyb_linear_fwd(dtype, feat, Cp, token_w, token_b, tok_dst, N, D, C, 0, stream));
    const bool tail = tail_enabled() && hyb_temporal_tail_ok(B, S, D, classes, hyb_ln_bwd_rows(N));
    HybEncTail t{};
    HYB_TRY(hyb_encoder_fwd_impl(dtype, tok_dst, mask, enc_params, enc_out, enc_saved, B, S, D, Hid, L, H, attn_p, layer_p, seed, seed_inc, stream,
                                 tail ? &t : nullptr));
    if (tail)
        return hyb_temporal_tail_fwd(dtype, t.f, t.x1, t.gamma, t.beta, enc_out, t.st2, B, S, D, t.eps, t.out_scale, t.p_drop, t.seed, seed_inc, head_w,
                                     head_b, logits, classes, loss, ce_scratch, (hipStream_t)stream, l);
    HYB_TRY(hyb_head_fwd(dtype, enc_out, head_w, head_b, logits, B, S, D, classes, stream));
    if (l) HYB_TRY(hyb_loss_fwd(*l, logits, loss, B, classes, (hipStream_t)stream));
    return 0;
}

// The seven forward entry points differ in the loss they describe and in nothing else: what they all hand on is named once.
#define HYB_TEMPORAL_FWD_COMMON                                                                                                            \
    dtype, h, token_w, token_b, enc_params, head_w, head_b, mask, feat, tok, enc_saved, enc_out, logits, B, S, HW, C, Cp, D, Hid, L, H, classes, \
        attn_p, layer_p, seed, seed_inc
extern "C" int hyb_temporal_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                                const float* head_w, const float* head_b, const float* mask, void* feat, void* tok, void* enc_saved,
                                void* enc_out, float* logits, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes,
                                float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* stream) {
    return temporal_fwd_impl(HYB_TEMPORAL_FWD_COMMON, nullptr, nullptr, stream, nullptr);
}
extern "C" int hyb_temporal_ce_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                                   const float* head_w, const float* head_b, const float* mask, const long long* target, void* feat, void* tok,
                                   void* enc_saved, void* enc_out, float* logits, float* loss, float* ce_scratch, int B, int S, int HW, int C, int Cp,
                                   int D, int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                                   const unsigned long long* seed_inc, void* stream) {
    const HybLoss l = hyb_loss_plain(target);
    return temporal_fwd_impl(HYB_TEMPORAL_FWD_COMMON, loss, ce_scratch, stream, &l);
}
extern "C" int hyb_temporal_ce_opts_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                                        const float* head_w, const float* head_b, const float* mask, const long long* target, const float* weight,
                                        long long ignore_index, int has_ignore, float label_smoothing, void* feat, void* tok, void* enc_saved,
                                        void* enc_out, float* logits, float* loss, float* ce_scratch, int B, int S, int HW, int C, int Cp, int D, int Hid,
                                        int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                                        const unsigned long long* seed_inc, void* stream) {
    const HybLoss l = hyb_loss_opts(target, weight, ignore_index, has_ignore, label_smoothing);
    return temporal_fwd_impl(HYB_TEMPORAL_FWD_COMMON, loss, ce_scratch, stream, &l);
}
extern "C" int hyb_temporal_ce_mix_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                                       const float* head_w, const float* head_b, const float* mask, const long long* target, const long long* target_b,
                                       const float* lam, const float* weight, long long ignore_index, int has_ignore, float label_smoothing, void* feat,
                                       void* tok, void* enc_saved, void* enc_out, float* logits, float* loss, float* ce_scratch, int B, int S, int HW, int C,
                                       int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                                       const unsigned long long* seed_inc, void* stream) {
    const HybLoss l = hyb_loss_mix(target, target_b, lam, weight, ignore_index, has_ignore, label_smoothing);
    return temporal_fwd_impl(HYB_TEMPORAL_FWD_COMMON, loss, ce_scratch, stream, &l);
}
extern "C" int hyb_temporal_ce_dense_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                                         const float* head_w, const float* head_b, const float* mask, const float* target, const float* weight,
                                         const float* pos_weight, int kind, float label_smoothing, void* feat, void* tok, void* enc_saved,
                                         void* enc_out, float* logits, float* loss, float* ce_scratch, int B, int S, int HW, int C, int Cp, int D,
                                         int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                                         const unsigned long long* seed_inc, void* stream) {
    const HybLoss l = hyb_loss_dense(target, weight, pos_weight, kind, label_smoothing);
    return temporal_fwd_impl(HYB_TEMPORAL_FWD_COMMON, loss, ce_scratch, stream, &l);
}
extern "C" int hyb_temporal_ce_focal_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                                         const float* head_w, const float* head_b, const float* mask, const long long* target, const float* weight,
                                         long long ignore_index, int has_ignore, float gamma, void* feat, void* tok, void* enc_saved, void* enc_out,
                                         float* logits, float* loss, float* ce_scratch, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H,
                                         int classes, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                                         void* stream) {
    const HybLoss l = hyb_loss_focal(target, weight, ignore_index, has_ignore, gamma);
    return temporal_fwd_impl(HYB_TEMPORAL_FWD_COMMON, loss, ce_scratch, stream, &l);
}
extern "C" int hyb_temporal_ce_asym_fwd(int dtype, const void* h, const float* token_w, const float* token_b, const float* const* enc_params,
                                        const float* head_w, const float* head_b, const float* mask, const float* target, const float* weight,
                                        const float* pos_weight, float gamma_pos, float gamma_neg, float clip, void* feat, void* tok, void* enc_saved,
                                        void* enc_out, float* logits, float* loss, float* ce_scratch, int B, int S, int HW, int C, int Cp, int D,
                                        int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                                        const unsigned long long* seed_inc, void* stream) {
    const HybLoss l = hyb_loss_asym(target, weight, pos_weight, gamma_pos, gamma_neg, clip);
    return temporal_fwd_impl(HYB_TEMPORAL_FWD_COMMON, loss, ce_scratch, stream, &l);
}
#undef HYB_TEMPORAL_FWD_COMMON

static int temporal_bwd_impl(int dtype, const float* dlogits, const float* logits, const float* dloss, const HybLoss* l, const float* token_w,
                             const float* const* enc_params, const float* head_w, const float* mask, const void* feat, const void* enc_saved,
                             const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b, void* dh,
                             int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p,
                             unsigned long long seed, const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes, void* stream) {
    HYB_CHECK_ARG(l ? !dlogits && logits && dloss && hyb_loss_ok(*l) : dlogits != nullptr);
    HYB_CHECK_ARG(token_w && enc_params && head_w && feat && enc_saved && enc_out && dtoken_w && enc_grads && dhead_w && dh && workspace);
    const bool h16 = (dtype & HYB_H_BF16) != 0;                 // dh is written as bf16
    dtype &= 0xff;
    HYB_CHECK_ARG(!h16 || dtype == HYB_F32);
    const TemporalBwdLayout lay = temporal_bwd_layout(dtype, B, S, Cp, D, Hid, L, H);
    if (workspace_bytes < lay.total) return HYB_E_WORKSPACE;
    const size_t es = dtype == HYB_F32 ? 4 : 2;
    const int N = B * S;
    char* ws = (char*)workspace;
    void* enc_ws = ws + lay.enc_ws;
    void *denc = ws + lay.denc, *dtok = ws + lay.dtok, *dfeat = ws + lay.dfeat;
    float* head_part = (float*)(ws + lay.head_part);
    // the token projection's weight gradient (dtok^T feat) rides in the encoder backward's final multi-matrix launch
    const bool ride = C % 8 == 0;
    const HybDwExtra tokdw{dtok, feat, dtoken_w, dtoken_b, D, C, D, Cp};
    const bool tail = tail_enabled() && dhead_b && hyb_temporal_tail_ok(B, S, D, classes, hyb_ln_bwd_rows(N)) && (ride || L <= 2);
    if (tail) {
        const HybEncBwdTail t = hyb_encoder_bwd_tail(dtype, enc_params, enc_saved, enc_ws, B, S, D, Hid, L, H, layer_p, seed);
        HYB_TRY(hyb_temporal_tail_bwd(dtype, dlogits, logits, dloss, head_w, enc_out, t.f, t.gamma, t.stats, t.dx, t.dskip, t.ln_part, t.ln_rows,
                                      head_part, B, S, D, classes, t.out_scale, t.p_drop, t.seed, seed_inc, (hipStream_t)stream, l));
        const long long cd = (long long)classes * D;
        const HybDwRider hr{head_part, dhead_w, dhead_b, B, cd + classes, cd};
        HYB_TRY(hyb_encoder_bwd_impl(dtype, nullptr, mask, enc_params, enc_grads, enc_saved, dtok, B, S, D, Hid, L, H, attn_p, layer_p, seed, seed_inc, enc_ws,
                                     lay.enc_bytes, stream, ride ? &tokdw : nullptr, 1, &hr));
    } else {
        const float* dl = dlogits;
        if (!dl) {      // cross-entropy backward as its own launch, into the head of the (not yet used) dfeat scratch
            HYB_CHECK_ARG((size_t)B * classes * sizeof(float) <= lay.dfeat_bytes);
            HYB_TRY(hyb_loss_bwd(*l, logits, dloss, (float*)dfeat, B, classes, (hipStream_t)stream));
            dl = (const float*)dfeat;
        }
        HYB_TRY(hyb_head_bwd(dtype, enc_out, head_w, dl, denc, dhead_w, dhead_b, B, S, D, classes, stream));
        HYB_TRY(hyb_encoder_bwd_impl(dtype, denc, mask, enc_params, enc_grads, enc_saved, dtok, B, S, D, Hid, L, H, attn_p, layer_p, seed, seed_inc, enc_ws,
                                     lay.enc_bytes, stream, ride ? &tokdw : nullptr, 0, nullptr));
    }
    if (Cp > C) { hipError_t e = hipMemsetAsync(dfeat, 0, (size_t)N * Cp * es, (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
    HYB_TRY(hyb_linear_bwd(dtype, feat, Cp, token_w, nullptr, dtok, dfeat, 0, ride ? nullptr : dtoken_w, ride ? nullptr : dtoken_b, N, D, C, 0, nullptr, 0,
                           stream));
    if (h16) HYB_TRY(hyb_gap_bwd_h16((const float*)dfeat, dh, N, HW, Cp, (hipStream_t)stream));
    else HYB_TRY(hyb_gap_bwd(dtype, dfeat, dh, N, HW, Cp, stream));
    return 0;
}

// ... and the seven backward ones
#define HYB_TEMPORAL_BWD_COMMON                                                                                                            \
    token_w, enc_params, head_w, mask, feat, enc_saved, enc_out, dtoken_w, dtoken_b, enc_grads, dhead_w, dhead_b, dh, B, S, HW, C, Cp, D, Hid, L, H, \
        classes, attn_p, layer_p, seed, seed_inc, workspace, workspace_bytes, stream
extern "C" int hyb_temporal_bwd(int dtype, const float* dlogits, const float* token_w, const float* const* enc_params, const float* head_w,
                                const float* mask, const void* feat, const void* enc_saved, const void* enc_out, float* dtoken_w,
                                float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C,
                                int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p, unsigned long long seed,
                                const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes, void* stream) {
    return temporal_bwd_impl(dtype, dlogits, nullptr, nullptr, nullptr, HYB_TEMPORAL_BWD_COMMON);
}
extern "C" int hyb_temporal_ce_bwd(int dtype, const float* dloss, const float* logits, const long long* target, const float* token_w,
                                   const float* const* enc_params, const float* head_w, const float* mask, const void* feat, const void* enc_saved,
                                   const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b,
                                   void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p,
                                   float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const HybLoss l = hyb_loss_plain(target);
    return temporal_bwd_impl(dtype, nullptr, logits, dloss, &l, HYB_TEMPORAL_BWD_COMMON);
}
extern "C" int hyb_temporal_ce_opts_bwd(int dtype, const float* dloss, const float* logits, const long long* target, const float* weight,
                                        long long ignore_index, int has_ignore, float label_smoothing, const float* token_w,
                                        const float* const* enc_params, const float* head_w, const float* mask, const void* feat, const void* enc_saved,
                                        const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b,
                                        void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p,
                                        float layer_p, unsigned long long seed, const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    const HybLoss l = hyb_loss_opts(target, weight, ignore_index, has_ignore, label_smoothing);
    return temporal_bwd_impl(dtype, nullptr, logits, dloss, &l, HYB_TEMPORAL_BWD_COMMON);
}
extern "C" int hyb_temporal_ce_mix_bwd(int dtype, const float* dloss, const float* logits, const long long* target, const long long* target_b,
                                       const float* lam, const float* weight, long long ignore_index, int has_ignore, float label_smoothing,
                                       const float* token_w, const float* const* enc_params, const float* head_w, const float* mask, const void* feat,
                                       const void* enc_saved, const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads,
                                       float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H,
                                       int classes, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    const HybLoss l = hyb_loss_mix(target, target_b, lam, weight, ignore_index, has_ignore, label_smoothing);
    return temporal_bwd_impl(dtype, nullptr, logits, dloss, &l, HYB_TEMPORAL_BWD_COMMON);
}
extern "C" int hyb_temporal_ce_dense_bwd(int dtype, const float* dloss, const float* logits, const float* target, const float* weight,
                                         const float* pos_weight, int kind, float label_smoothing, const float* token_w,
                                         const float* const* enc_params, const float* head_w, const float* mask, const void* feat,
                                         const void* enc_saved, const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads,
                                         float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H,
                                         int classes, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    const HybLoss l = hyb_loss_dense(target, weight, pos_weight, kind, label_smoothing);
    return temporal_bwd_impl(dtype, nullptr, logits, dloss, &l, HYB_TEMPORAL_BWD_COMMON);
}
extern "C" int hyb_temporal_ce_focal_bwd(int dtype, const float* dloss, const float* logits, const long long* target, const float* weight,
                                         long long ignore_index, int has_ignore, float gamma, const float* token_w, const float* const* enc_params,
                                         const float* head_w, const float* mask, const void* feat, const void* enc_saved, const void* enc_out,
                                         float* dtoken_w, float* dtoken_b, float* const* enc_grads, float* dhead_w, float* dhead_b, void* dh, int B, int S,
                                         int HW, int C, int Cp, int D, int Hid, int L, int H, int classes, float attn_p, float layer_p,
                                         unsigned long long seed, const unsigned long long* seed_inc, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    const HybLoss l = hyb_loss_focal(target, weight, ignore_index, has_ignore, gamma);
    return temporal_bwd_impl(dtype, nullptr, logits, dloss, &l, HYB_TEMPORAL_BWD_COMMON);
}
extern "C" int hyb_temporal_ce_asym_bwd(int dtype, const float* dloss, const float* logits, const float* target, const float* weight,
                                        const float* pos_weight, float gamma_pos, float gamma_neg, float clip, const float* token_w,
                                        const float* const* enc_params, const float* head_w, const float* mask, const void* feat,
                                        const void* enc_saved, const void* enc_out, float* dtoken_w, float* dtoken_b, float* const* enc_grads,
                                        float* dhead_w, float* dhead_b, void* dh, int B, int S, int HW, int C, int Cp, int D, int Hid, int L, int H,
                                        int classes, float attn_p, float layer_p, unsigned long long seed, const unsigned long long* seed_inc,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    const HybLoss l = hyb_loss_asym(target, weight, pos_weight, gamma_pos, gamma_neg, clip);
    return temporal_bwd_impl(dtype, nullptr, logits, dloss, &l, HYB_TEMPORAL_BWD_COMMON);
}
#undef HYB_TEMPORAL_BWD_COMMON
