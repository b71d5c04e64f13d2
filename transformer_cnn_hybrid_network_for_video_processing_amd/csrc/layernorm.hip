// LayerNorm + residual epilogue of TransformerEncoder.forward (TransformerEncoder.pyc src L116-117, L120-123):
//   y = dropout_p( (LayerNorm(x) * gamma + beta + skip) * out_scale )
// One wave per token row (D <= 2048), 8 features per lane per chunk, statistics by wave shuffles.
// Also the classifier head (mean over T + Linear) and the cross-entropy loss: tiny, one kernel each.
#include "hyb_common.h"
#include "hyb_internal.h"

namespace {

constexpr int LN_MAXC = 4;        // chunks of 8 features per lane: D <= 64*8*4 = 2048

// Latency is all this kernel has (128 rows of 512 features): every global load of a row -- x, skip, gamma, beta and the dropout counter --
// is issued before the first wait, so the kernel pays ONE memory round trip (the first version loaded skip / gamma / beta after the two
// reductions and the counter before anything else: three dependent round trips, 4.2 us hot; reductions by DPP, not ds_bpermute).
// One token row by one wave (the body of ln_residual_fwd_kernel; also called per row by temporal_tail_fwd_kernel, which is why the two
// produce the same bits).  ycopy: optional second destination (an LDS image of the row), same values.
template <typename T>
__device__ __forceinline__ void ln_fwd_row(const T* __restrict__ x, const T* __restrict__ skip, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, T* __restrict__ y, T* ycopy, float* __restrict__ stats, int M, int row,
                                           int D, float eps, float out_scale, float p_drop, unsigned long long seed,
                                           const unsigned long long* __restrict__ seed_inc, int lane) {
    const int nchunk = D >> 3;
    Vec8<T> xv[LN_MAXC], sk[LN_MAXC];
    Vec8<float> gm[LN_MAXC], bt[LN_MAXC];
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
            xv[c].load(x + (long long)row * D + ch * 8);
            sk[c].load(skip + (long long)row * D + ch * 8);
            gm[c].load(gamma + ch * 8);
            bt[c].load(beta + ch * 8);
        }
    }
    unsigned long long inc = 0;
    if (p_drop > 0.f && seed_inc) inc = *seed_inc;              // device-side step counter: the same captured launch draws a fresh mask per replay
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += xv[c].get(j);
        }
    }
    const float mean = wave_sum(sum) / (float)D;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float dlt = xv[c].get(j) - mean; var += dlt * dlt; }
        }
    }
    var = wave_sum(var) / (float)D;
    const float rstd = rsqrtf(var + eps);
    if (lane == 0) { stats[row] = mean; stats[M + row] = rstd; }
    const float inv_keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
    seed += inc;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
            Vec8<T> o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = ch * 8 + j;
                float v = ((xv[c].get(j) - mean) * rstd * gm[c].get(j) + bt[c].get(j) + sk[c].get(j)) * out_scale;
                if (p_drop > 0.f) v *= dropout_mult(seed, (unsigned long long)row * D + col, p_drop, inv_keep);
                o.set(j, v);
            }
            o.store(y + (long long)row * D + ch * 8);
            if (ycopy) o.store(ycopy + ch * 8);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ln_residual_fwd_kernel(const T* __restrict__ x, const T* __restrict__ skip,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              T* __restrict__ y, float* __restrict__ stats, int M, int D, float eps,
                                                              float out_scale, float p_drop, unsigned long long seed, const unsigned long long* __restrict__ seed_inc) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    ln_fwd_row<T>(x, skip, gamma, beta, y, nullptr, stats, M, row, D, eps, out_scale, p_drop, seed, seed_inc, lane);
}

// One token row of the LayerNorm + residual backward by one wave (the loop body of ln_residual_bwd_kernel; temporal_tail_bwd_kernel calls it
// with the row's upstream gradient in LDS: DY_LDS, dyl[D] floats holding T-rounded values -- the same for every token of a clip).
template <typename T, bool DY_LDS, bool XPRE = false>
__device__ __forceinline__ void ln_bwd_row(const T* __restrict__ dy, const float* dyl, const T* __restrict__ x, const Vec8<float> (&gmv)[LN_MAXC],
                                           const float* __restrict__ stats, T* __restrict__ dx, T* __restrict__ dskip, int accumulate_dskip,
                                           float (&dg)[LN_MAXC][8], float (&db)[LN_MAXC][8], int M, int row, int D, float out_scale, float p_drop,
                                           unsigned long long seed, float inv_keep, int lane, const Vec8<T>* xpre = nullptr) {
    // XPRE: the caller loaded the row of x already (xpre[LN_MAXC]), before it formed dyl -- one memory round trip instead of two
    const int nchunk = D >> 3;
    Vec8<T> dvv[LN_MAXC], xvv[LN_MAXC], dsv[LN_MAXC];
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {                    // every load of the row before the first wait
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
            if (DY_LDS) {
#pragma unroll
                for (int j = 0; j < 8; ++j) dvv[c].set(j, dyl[ch * 8 + j]);
            } else dvv[c].load(dy + (long long)row * D + ch * 8);
            if (XPRE) xvv[c] = xpre[c]; else xvv[c].load(x + (long long)row * D + ch * 8);
            if (accumulate_dskip) dsv[c].load(dskip + (long long)row * D + ch * 8);
        }
    }
    const float mean = stats[row], rstd = stats[M + row];
    float gl[LN_MAXC][8], xh[LN_MAXC][8];      // g = d(ln_out) * gamma ; xhat
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
            const Vec8<T>& dv = dvv[c];
            const Vec8<T>& xv = xvv[c];
            Vec8<T> ds = dsv[c];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = ch * 8 + j;
                float d = dv.get(j) * out_scale;
                if (p_drop > 0.f) d *= dropout_mult(seed, (unsigned long long)row * D + col, p_drop, inv_keep);
                const float xhat = (xv.get(j) - mean) * rstd;
                xh[c][j] = xhat;
                dg[c][j] += d * xhat;
                db[c][j] += d;
                const float g = d * gmv[c].get(j);
                gl[c][j] = g;
                s1 += g;
                s2 += g * xhat;
                ds.set(j, accumulate_dskip ? ds.get(j) + d : d);
            }
            ds.store(dskip + (long long)row * D + ch * 8);
        }
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
            Vec8<T> o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.set(j, rstd * (gl[c][j] - s1 - xh[c][j] * s2));
            o.store(dx + (long long)row * D + ch * 8);
        }
    }
}

// ROWS = false: dgamma/dbeta += block sums (float atomics; the public per-op entry point).  ROWS = true (encoder composite): the
// block writes its sums as one partial row dgamma[blockIdx][2][D] (fixed order inside the block), summed later in a fixed order.
template <typename T, bool ROWS>
__global__ __launch_bounds__(256) void ln_residual_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ stats, T* __restrict__ dx, T* __restrict__ dskip,
                                                              int accumulate_dskip, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              int M, int D, float out_scale, float p_drop, unsigned long long seed, const unsigned long long* __restrict__ seed_inc) {
    const int lane = threadIdx.x & 63;
    const int nchunk = D >> 3;
    const int total_waves = gridDim.x * 4;
    // gamma is row-independent: loaded once, together with the first row's operands (one memory round trip; see the forward kernel)
    Vec8<float> gmv[LN_MAXC];
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) { const int ch = lane + 64 * c; if (ch < nchunk) gmv[c].load(gamma + ch * 8); }
    bool seeded = false;
    float dg[LN_MAXC][8], db[LN_MAXC][8];
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) { dg[c][j] = 0.f; db[c][j] = 0.f; }
    const float inv_keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += total_waves) {
        if (!seeded) { if (p_drop > 0.f && seed_inc) seed += *seed_inc; seeded = true; }      // device-side step counter (fresh mask per replay)
        ln_bwd_row<T, false>(dy, nullptr, x, gmv, stats, dx, dskip, accumulate_dskip, dg, db, M, row, D, out_scale, p_drop, seed, inv_keep, lane);
    }
    extern __shared__ float lnred[];
    if (ROWS) {
        // per-wave slots [4][2][D] (single owner per entry), then the four waves in a fixed order
        float* mine = lnred + (threadIdx.x >> 6) * 2 * D;
#pragma unroll
        for (int c = 0; c < LN_MAXC; ++c) {
            const int ch = lane + 64 * c;
            if (ch < nchunk) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { mine[ch * 8 + j] = dg[c][j]; mine[D + ch * 8 + j] = db[c][j]; }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * D; i += blockDim.x)
            dgamma[(long long)blockIdx.x * 2 * D + i] = (lnred[i] + lnred[2 * D + i]) + (lnred[4 * D + i] + lnred[6 * D + i]);
        return;
    }
    // combine the block's 4 waves in LDS, then one atomic per feature per block
    for (int i = threadIdx.x; i < 2 * D; i += blockDim.x) lnred[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                atomicAdd(&lnred[ch * 8 + j], dg[c][j]);
                atomicAdd(&lnred[D + ch * 8 + j], db[c][j]);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        atomicAdd(dgamma + i, lnred[i]);
        atomicAdd(dbeta + i, lnred[D + i]);
    }
}

// [G rows][2][D] partial rows -> dgamma[D], dbeta[D] (overwritten), fixed order
__global__ __launch_bounds__(1024) void ln_rows_reduce_kernel(const float* __restrict__ part, int G, int D, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
    long long i; float v;
    if (!rows_reduce_1024(part, G, 2LL * D, i, v)) return;
    if (i < D) dgamma[i] = v; else dbeta[i - D] = v;
}

// mean over the S tokens of feature d of clip b: the loads are issued eight at a time (independent), the additions keep the
// order of a plain loop
template <typename T>
__device__ __forceinline__ float token_mean(const T* __restrict__ x, int b, int S, int D, int d) {
    const T* col = x + (long long)b * S * D + d;
    float s = 0.f;
    int t = 0;
    for (; t + 8 <= S; t += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = to_f32<T>(col[(long long)(t + j) * D]);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; t < S; ++t) s += to_f32<T>(col[(long long)t * D]);
    return s / (float)S;
}

// ---- head: logits[b][c] = bias[c] + sum_d mean_s(x[b][s][d]) * W[c][d] ------------------------------
template <typename T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                       float* __restrict__ logits, int S, int D, int C) {
    extern __shared__ float pooled[];          // [D]
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this wave's first class: its weight row does not depend on the tokens -- requested before the token means (a latency-bound kernel:
    // one memory round trip fewer on the critical path), up to 8 x 64 features in registers
    float w0[8];
    const bool pre = wave < C && D <= 512;
#pragma unroll
    for (int j = 0; j < 8; ++j) w0[j] = (pre && lane + 64 * j < D) ? W[(long long)wave * D + lane + 64 * j] : 0.f;
    for (int d = threadIdx.x; d < D; d += blockDim.x) pooled[d] = token_mean(x, b, S, D, d);
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        float s = 0.f;
        if (pre && c == wave) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int d = lane + 64 * j; if (d < D) s = fmaf(pooled[d], w0[j], s); }      // same order and rounding as head_logit
        } else {
            for (int d = lane; d < D; d += 64) s = fmaf(pooled[d], W[(long long)c * D + d], s);
        }
        s = wave_sum(s);
        if (lane == 0) logits[b * C + c] = s + (bias ? bias[c] : 0.f);
    }
}
// dx[b][s][d] = (1/S) sum_c dlogits[b][c] W[c][d]
template <typename T>
__global__ void head_bwd_dx_kernel(const float* __restrict__ W, const float* __restrict__ dlogits, T* __restrict__ dx, int S, int D, int C) {
    const int b = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(dlogits[b * C + c], W[(long long)c * D + d], s);      // (explicit: the same rounding in every kernel that forms this row)
        const T v = from_f32<T>(s / (float)S);
        for (int t = 0; t < S; ++t) dx[((long long)b * S + t) * D + d] = v;
    }
}
// dW[c][d] = sum_b dlogits[b][c] * mean_s x[b][s][d];  db[c] = sum_b dlogits[b][c]
// grid (D/64, C-chunks of 16), 256 threads = 64 features x 4 clip groups (clips b = group, group + 4, ...); the groups are
// combined through LDS in a fixed order
// (with dx_rider: the blocks y >= ceil(C/16) of the same launch form dx, the head's input gradient -- one launch for the whole head backward)
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_dw_kernel(const T* __restrict__ x, const float* __restrict__ dlogits, float* __restrict__ dW,
                                                          float* __restrict__ db, int B, int S, int D, int C, const float* __restrict__ W,
                                                          T* __restrict__ dx_rider, int yblocks) {
    __shared__ float red[4][16][64];
    if ((int)blockIdx.y >= yblocks) {                      // dx[b][s][d] = (1/S) sum_c dlogits[b][c] W[c][d] for this block's 64 features
        const int d = blockIdx.x * 64 + (threadIdx.x & 63);
        if (d >= D) return;
        for (int b = ((int)blockIdx.y - yblocks) * 4 + (threadIdx.x >> 6); b < B; b += 4 * ((int)gridDim.y - yblocks)) {
            float s = 0.f;
            for (int c = 0; c < C; ++c) s = fmaf(dlogits[b * C + c], W[(long long)c * D + d], s);
            const T v = from_f32<T>(s / (float)S);
            for (int t = 0; t < S; ++t) dx_rider[((long long)b * S + t) * D + d] = v;
        }
        return;
    }
    const int dl = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int d = blockIdx.x * 64 + dl;
    const int c0 = blockIdx.y * 16;
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.f;
    if (d < D) {
        for (int b = grp; b < B; b += 4) {
            const float s = token_mean(x, b, S, D, d);
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c0 + c < C) acc[c] += dlogits[b * C + c0 + c] * s;
        }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) red[grp][c][dl] = acc[c];
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * 64; i += 256) {
        const int c = i >> 6, dd = i & 63;
        if (c0 + c < C && blockIdx.x * 64 + dd < D)
            dW[(long long)(c0 + c) * D + blockIdx.x * 64 + dd] = (red[0][c][dd] + red[1][c][dd]) + (red[2][c][dd] + red[3][c][dd]);
    }
    if (db && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < C) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dlogits[b * C + threadIdx.x];
        db[threadIdx.x] = s;
    }
}

// ---- cross entropy (mean over the batch) --------------------------------------------------------------
// one clip's loss term from its C logits (any address space); shared by ce_fwd_kernel and the fused temporal tail
__device__ __forceinline__ float ce_clip_loss(const float* lg, long long t, int C) {
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lg[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lg[c] - mx);
    // an out-of-range class index (torch raises a device assert) poisons the loss instead of reading out of bounds
    return (t >= 0 && t < C) ? (logf(s) + mx) - lg[(int)t] : NAN;
}
// one clip's d(loss)/d(logits[c]) for every class c, g = dloss / B
__device__ __forceinline__ float ce_clip_dlogit(const float* lg, long long t, int C, int c, float g) {
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, lg[k]);
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(lg[k] - mx);
    const bool ok = t >= 0 && t < C;                          // out of range: NaN gradient row (see ce_clip_loss)
    return ok ? g * (expf(lg[c] - mx) / s - (c == (int)t ? 1.f : 0.f)) : NAN;
}
// mean of the per-clip terms: threads 0..255 of the calling workgroup (every thread of it must call), thread t owns clips t, t+256, ..;
// a fixed tree -- the same one whether the terms were just computed (ce_fwd_kernel) or come from other workgroups (temporal tail)
__device__ __forceinline__ void ce_tree_mean(float acc, float* part /* LDS [256] */, float* __restrict__ loss, int B) {
    if (threadIdx.x < 256) part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = part[0] / (float)B;
}
__global__ void ce_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target, float* __restrict__ loss, int B, int C) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) acc += ce_clip_loss(logits + (long long)b * C, target[b], C);
    ce_tree_mean(acc, part, loss, B);
}
__global__ void ce_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target, const float* __restrict__ dloss,
                              float* __restrict__ dlogits, int B, int C) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float g = dloss[0] / (float)B;
    const long long t = target[b];
    for (int c = 0; c < C; ++c) dlogits[b * C + c] = ce_clip_dlogit(logits + (long long)b * C, t, C, c, g);
}

// ---- cross entropy with options: class weights w (nullptr: all ones), an ignored class index, label smoothing e -------------------
// torch.nn.functional.cross_entropy's "mean":  loss = (sum_b term_b) / den,  den = sum_b keep_b w[y_b],  keep_b = (y_b != ignore),
//   term_b = keep_b [ (1 - e) w[y_b] (lse_b - z_b[y_b]) + (e / C) sum_c w[c] (lse_b - z_b[c]) ].
// The plain loss above stays its own code (its kernels are the benchmarked path); these are the same per-clip / tree scheme: every
// per-clip expression is one device function shared by the stand-alone kernels and the fused temporal tail, numerator and den each go
// through the fixed 256-leaf tree, and den -- a function of target and weight alone -- is formed by whoever needs it, forward or backward,
// with the same function: the backward divides by the forward's bits without a hand-off.
__device__ __forceinline__ float ce_w(const float* w, int c) { return w ? w[c] : 1.f; }
__device__ __forceinline__ bool ce_keep(long long t, const HybCeOpts& o) { return !(o.has_ignore && t == o.ignore_index); }
// one clip's share of den; a kept target outside [0, C) poisons it (and with it the loss and every gradient) instead of reading out of bounds
__device__ __forceinline__ float ce_clip_den(const float* w, long long t, int C, const HybCeOpts& o) {
    if (!ce_keep(t, o)) return 0.f;
    return (t >= 0 && t < C) ? ce_w(w, (int)t) : NAN;
}
__device__ __forceinline__ float ce_clip_loss_opts(const float* lg, const float* w, long long t, int C, const HybCeOpts& o) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lg[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lg[c] - mx);
    const float lse = logf(s) + mx;
    float r = (1.f - o.label_smoothing) * (ce_w(w, (int)t) * (lse - lg[(int)t]));
    if (o.label_smoothing > 0.f) {
        float sm = 0.f;
        for (int c = 0; c < C; ++c) sm += ce_w(w, c) * (lse - lg[c]);
        r += (o.label_smoothing / (float)C) * sm;
    }
    return r;
}
// one clip's d(loss)/d(logits[c]), g = dloss / den (0 when den == 0: nothing was kept, the gradient is zero)
__device__ __forceinline__ float ce_clip_dlogit_opts(const float* lg, const float* w, long long t, int C, int c, float g, const HybCeOpts& o) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, lg[k]);
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(lg[k] - mx);
    const float p = expf(lg[c] - mx) / s;
    float r = (1.f - o.label_smoothing) * (ce_w(w, (int)t) * (p - (c == (int)t ? 1.f : 0.f)));
    if (o.label_smoothing > 0.f) {
        float ws = 0.f;
        for (int k = 0; k < C; ++k) ws += ce_w(w, k);
        r += (o.label_smoothing / (float)C) * (p * ws - ce_w(w, c));
    }
    return g * r;
}
// sum of 256 leaves (thread t of the calling workgroup holds leaf t; every thread of it must call), ce_tree_mean's tree; returned to every thread
__device__ __forceinline__ float ce_tree_sum(float acc, float* part /* LDS [256] */) {
    if (threadIdx.x < 256) part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    const float r = part[0];
    __syncthreads();                                          // (part is free again)
    return r;
}
// den by the calling workgroup (>= 256 threads, all of them call): thread t owns clips t, t + 256, ..
__device__ __forceinline__ float ce_den(const long long* __restrict__ target, const float* w, int B, int C, const HybCeOpts& o, float* part) {
    float acc = 0.f;
    if (threadIdx.x < 256)
        for (int i = threadIdx.x; i < B; i += 256) acc += ce_clip_den(w, target[i], C, o);
    return ce_tree_sum(acc, part);
}
__device__ __forceinline__ float ce_loss_opts(float num, float den) { return den == 0.f ? NAN : num / den; }
__device__ __forceinline__ float ce_gscale_opts(float dloss, float den) { return den == 0.f ? 0.f : dloss / den; }

__global__ __launch_bounds__(256) void ce_opts_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target, float* __restrict__ loss,
                                                          int B, int C, HybCeOpts o) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) acc += ce_clip_loss_opts(logits + (long long)b * C, o.weight, target[b], C, o);
    const float num = ce_tree_sum(acc, part);
    const float den = ce_den(target, o.weight, B, C, o, part);
    if (threadIdx.x == 0) loss[0] = ce_loss_opts(num, den);
}
__global__ __launch_bounds__(256) void ce_opts_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                          const float* __restrict__ dloss, float* __restrict__ dlogits, int B, int C, HybCeOpts o) {
    __shared__ float part[256];
    const float g = ce_gscale_opts(dloss[0], ce_den(target, o.weight, B, C, o, part));      // every workgroup forms den for itself
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const long long t = target[b];
    for (int c = 0; c < C; ++c) dlogits[(long long)b * C + c] = ce_clip_dlogit_opts(logits + (long long)b * C, o.weight, t, C, c, g, o);
}

// ---- two targets per clip (the labels of a Mixup / CutMix batch): a_b = target[b], c_b = target_b[b], l_b = lam[b], read on the device ----
//   num = sum_b [ l_b term(b, a_b) + (1 - l_b) term(b, c_b) ],  den = sum_b [ l_b d(b, a_b) + (1 - l_b) d(b, c_b) ],  loss = num / den,
// term = ce_clip_loss_opts and d = ce_clip_den above, each side under its own ignore_index / out-of-range rule.  The log-sum-exp (and the
// smoothing sum, which does not depend on the target) is formed once per clip and serves both sides; a side is written with
// ce_clip_loss_opts' expressions, and l_b == 1 returns the a side as it stands -- not 1 * a + 0 * c -- so that lam == 1 everywhere gives the
// bits of the *_opts_* family and never looks at c_b (l_b == 0: the mirror image).  An l_b outside [0, 1] or NaN poisons den.
// (ce_side_loss / ce_side_dlogit are SECOND COPIES of the expressions in ce_clip_loss_opts / ce_clip_dlogit_opts, which keep theirs so that
// the *_opts_* kernels keep their instructions: a change to either formula must be made in both; tests/test_gpu_mix_loss.py compares
// lam == 1 and lam == 0 with the *_opts_* operators bit for bit, loss and gradient, and fails when one copy is forgotten.)
__device__ __forceinline__ float ce_side_loss(const float* lg, const float* w, long long t, int C, float lse, float sm, const HybCeOpts& o) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    float r = (1.f - o.label_smoothing) * (ce_w(w, (int)t) * (lse - lg[(int)t]));
    if (o.label_smoothing > 0.f) r += (o.label_smoothing / (float)C) * sm;
    return r;
}
__device__ __forceinline__ float ce_clip_den_mix(const float* w, long long ta, long long tc, float l, int C, const HybCeOpts& o) {
    if (!(l >= 0.f && l <= 1.f)) return NAN;
    if (l == 1.f) return ce_clip_den(w, ta, C, o);
    if (l == 0.f) return ce_clip_den(w, tc, C, o);
    return l * ce_clip_den(w, ta, C, o) + (1.f - l) * ce_clip_den(w, tc, C, o);
}
__device__ __forceinline__ float ce_clip_loss_mix(const float* lg, const float* w, long long ta, long long tc, float l, int C, const HybCeOpts& o) {
    const bool use_a = !(l == 0.f), use_c = !(l == 1.f);
    if (!((use_a && ce_keep(ta, o)) || (use_c && ce_keep(tc, o)))) return 0.f;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lg[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lg[c] - mx);
    const float lse = logf(s) + mx;
    float sm = 0.f;
    if (o.label_smoothing > 0.f)
        for (int c = 0; c < C; ++c) sm += ce_w(w, c) * (lse - lg[c]);
    if (!use_c) return ce_side_loss(lg, w, ta, C, lse, sm, o);
    if (!use_a) return ce_side_loss(lg, w, tc, C, lse, sm, o);
    return l * ce_side_loss(lg, w, ta, C, lse, sm, o) + (1.f - l) * ce_side_loss(lg, w, tc, C, lse, sm, o);
}
// one side's d(term)/d(logits[c]) before the scale g (ce_clip_dlogit_opts' expressions); p = softmax(logits)[c], ws = sum_k w[k]
__device__ __forceinline__ float ce_side_dlogit(const float* w, long long t, int C, int c, float p, float ws, const HybCeOpts& o) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    float r = (1.f - o.label_smoothing) * (ce_w(w, (int)t) * (p - (c == (int)t ? 1.f : 0.f)));
    if (o.label_smoothing > 0.f) r += (o.label_smoothing / (float)C) * (p * ws - ce_w(w, c));
    return r;
}
__device__ __forceinline__ float ce_clip_dlogit_mix(const float* lg, const float* w, long long ta, long long tc, float l, int C, int c, float g,
                                                    const HybCeOpts& o) {
    const bool use_a = !(l == 0.f), use_c = !(l == 1.f);
    if (!((use_a && ce_keep(ta, o)) || (use_c && ce_keep(tc, o)))) return 0.f;      // (rows of clips with nothing kept stay 0 whatever g is)
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, lg[k]);
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(lg[k] - mx);
    const float p = expf(lg[c] - mx) / s;
    float ws = 0.f;
    if (o.label_smoothing > 0.f)
        for (int k = 0; k < C; ++k) ws += ce_w(w, k);
    if (!use_c) return g * ce_side_dlogit(w, ta, C, c, p, ws, o);
    if (!use_a) return g * ce_side_dlogit(w, tc, C, c, p, ws, o);
    return g * (l * ce_side_dlogit(w, ta, C, c, p, ws, o) + (1.f - l) * ce_side_dlogit(w, tc, C, c, p, ws, o));
}
// den by the calling workgroup, as ce_den
__device__ __forceinline__ float ce_den_mix(const long long* __restrict__ target, const HybCeMix& m, const float* w, int B, int C, const HybCeOpts& o,
                                            float* part) {
    float acc = 0.f;
    if (threadIdx.x < 256)
        for (int i = threadIdx.x; i < B; i += 256) acc += ce_clip_den_mix(w, target[i], m.target_b[i], m.lam[i], C, o);
    return ce_tree_sum(acc, part);
}
__global__ __launch_bounds__(256) void ce_mix_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target, float* __restrict__ loss,
                                                         int B, int C, HybCeOpts o, HybCeMix m) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) acc += ce_clip_loss_mix(logits + (long long)b * C, o.weight, target[b], m.target_b[b], m.lam[b], C, o);
    const float num = ce_tree_sum(acc, part);
    const float den = ce_den_mix(target, m, o.weight, B, C, o, part);
    if (threadIdx.x == 0) loss[0] = ce_loss_opts(num, den);
}
__global__ __launch_bounds__(256) void ce_mix_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                         const float* __restrict__ dloss, float* __restrict__ dlogits, int B, int C, HybCeOpts o,
                                                         HybCeMix m) {
    __shared__ float part[256];
    const float g = ce_gscale_opts(dloss[0], ce_den_mix(target, m, o.weight, B, C, o, part));
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const long long ta = target[b], tc = m.target_b[b];
    const float l = m.lam[b];
    for (int c = 0; c < C; ++c) dlogits[(long long)b * C + c] = ce_clip_dlogit_mix(logits + (long long)b * C, o.weight, ta, tc, l, C, c, g, o);
}

// ---- dense targets: one fp32 row t_b[0..C) per clip (include/hybrid_hip.h states both definitions) ----------------------------------------
// kind 0, soft-target cross-entropy (torch's cross_entropy with class probabilities): q_c = (1 - e) t_c + e / C,
//   term_b = sum_c w_c q_c (lse_b - z_c),  loss = (sum_b term_b) / B,  dz_c = (dloss / B) (p_c P_b - w_c q_c),  P_b = sum_k w_k q_k.
// kind 1, binary cross-entropy with logits: L_c = 1 + (pw_c - 1) t_c,  sp(z) = log1p(exp(-|z|)) + max(-z, 0) (no overflow at any z),
//   term_b = sum_c w_c [ (1 - t_c) z_c + L_c sp(z_c) ],  loss = (sum_b term_b) / (B C),  dz_c = (dloss / (B C)) w_c (L_c sigmoid(z_c) - pw_c t_c).
// The sum over classes runs in class order from 0.f and every product that feeds a sum is an explicit fmaf, so a one-hot row with no weights
// and no smoothing adds exact zeros and multiplies by exact ones: kind 0 then gives the bits of ce_clip_loss / ce_clip_dlogit.  The divisor is
// B or B C, known on the host side of every kernel: no den pass.  Rows are used as given (not normalised, not range-checked; NaN propagates).
__device__ __forceinline__ float ce_soft_q(float t, float e, int C) { return fmaf(1.f - e, t, e / (float)C); }
__device__ __forceinline__ float ce_clip_loss_soft(const float* lg, const float* w, const float* t, int C, float e) {
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lg[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lg[c] - mx);
    const float lse = logf(s) + mx;
    float r = 0.f;
    for (int c = 0; c < C; ++c) r = fmaf(ce_w(w, c) * ce_soft_q(t[c], e, C), lse - lg[c], r);
    return r;
}
// one clip's d(loss)/d(logits[c]), g = dloss / B
__device__ __forceinline__ float ce_clip_dlogit_soft(const float* lg, const float* w, const float* t, int C, int c, float g, float e) {
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, lg[k]);
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(lg[k] - mx);
    const float p = expf(lg[c] - mx) / s;
    float P = 0.f;
    for (int k = 0; k < C; ++k) P = fmaf(ce_w(w, k), ce_soft_q(t[k], e, C), P);
    return g * fmaf(p, P, -(ce_w(w, c) * ce_soft_q(t[c], e, C)));
}
__device__ __forceinline__ float ce_clip_loss_bce(const float* lg, const float* w, const float* pw, const float* t, int C) {
    float r = 0.f;
    for (int c = 0; c < C; ++c) {
        const float z = lg[c], tc = t[c];
        const float L = fmaf(ce_w(pw, c) - 1.f, tc, 1.f);
        const float sp = log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.f);
        r = fmaf(ce_w(w, c), fmaf(L, sp, (1.f - tc) * z), r);
    }
    return r;
}
// one clip's d(loss)/d(logits[c]), g = dloss / (B C)
__device__ __forceinline__ float ce_clip_dlogit_bce(const float* lg, const float* w, const float* pw, const float* t, int c, float g) {
    const float z = lg[c], tc = t[c], pwc = ce_w(pw, c);
    const float L = fmaf(pwc - 1.f, tc, 1.f);
    const float ez = expf(-fabsf(z));
    const float sg = (z >= 0.f ? 1.f : ez) / (1.f + ez);
    return g * (ce_w(w, c) * fmaf(L, sg, -(pwc * tc)));
}
__device__ __forceinline__ float ce_dense_div(int B, int C, int kind) { return kind == 1 ? (float)B * (float)C : (float)B; }

__global__ __launch_bounds__(256) void ce_dense_fwd_kernel(const float* __restrict__ logits, float* __restrict__ loss, int B, int C, HybCeOpts o,
                                                           HybCeDense d) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* lg = logits + (long long)b * C;
        const float* t = d.target + (long long)b * C;
        acc += d.kind == 1 ? ce_clip_loss_bce(lg, o.weight, d.pos_weight, t, C) : ce_clip_loss_soft(lg, o.weight, t, C, o.label_smoothing);
    }
    const float num = ce_tree_sum(acc, part);
    if (threadIdx.x == 0) loss[0] = num / ce_dense_div(B, C, d.kind);
}
__global__ __launch_bounds__(256) void ce_dense_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ dloss,
                                                           float* __restrict__ dlogits, int B, int C, HybCeOpts o, HybCeDense d) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float g = dloss[0] / ce_dense_div(B, C, d.kind);
    const float* lg = logits + (long long)b * C;
    const float* t = d.target + (long long)b * C;
    for (int c = 0; c < C; ++c)
        dlogits[(long long)b * C + c] = d.kind == 1 ? ce_clip_dlogit_bce(lg, o.weight, d.pos_weight, t, c, g)
                                                    : ce_clip_dlogit_soft(lg, o.weight, t, C, c, g, o.label_smoothing);
}

// ---- focal and asymmetric losses (include/hybrid_hip.h states both definitions) ------------------------------------------------------------
// x^g and d(x^g)/dx = g x^(g-1) under the family's rules: an exponent of 0 gives exactly 1 and a derivative of exactly 0, x^(g-1) at g == 1
// is exactly 1.  (Every g the entry points take is 0 or >= 1; the per-cell exponent of a soft asymmetric row may fall between: powf then.)
__device__ __forceinline__ float ce_pow(float x, float g) { return g == 0.f ? 1.f : g == 1.f ? x : g == 2.f ? x * x : powf(x, g); }
__device__ __forceinline__ float ce_dpow(float x, float g) { return g == 0.f ? 0.f : g == 1.f ? 1.f : g * ce_pow(x, g - 1.f); }
// Index focal: term_b = keep_b w[y] u^g (lse_b - z_by), u = (sum_{c != y} exp(z_c - mx)) / s in class order -- the other classes' softmax
// mass as a sum, not 1 - p_y, which cancels for a confident clip.  keep, den, the out-of-range and all-ignored rules are ce_clip_loss_opts'
// (no label smoothing), and so are the log-sum-exp loops: u's numerator is a second accumulator in the loop that forms s -- no further pass
// over the logits, which the backward reads from global memory: a pass is a memory round trip on the tail's critical path -- and leaves s as
// it was, so g == 0 gives ce_clip_loss_opts' / ce_clip_dlogit_opts' bits ((1 - 0) * x there is x).
__device__ __forceinline__ float ce_clip_loss_focal(const float* lg, const float* w, long long t, int C, const HybCeOpts& o, float gm) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lg[c]);
    float s = 0.f, a = 0.f;
    for (int c = 0; c < C; ++c) { const float e = expf(lg[c] - mx); s += e; if (c != (int)t) a += e; }
    const float lse = logf(s) + mx;
    const float r = ce_w(w, (int)t) * (lse - lg[(int)t]);
    if (gm == 0.f) return r;
    return ce_pow(a / s, gm) * r;
}
// one clip's d(loss)/d(logits[c]), g = dloss / den:  g w[y] M (p_c - [c == y]),  M = u^gm + gm u^(gm-1) p_y (lse - z_y)
__device__ __forceinline__ float ce_clip_dlogit_focal(const float* lg, const float* w, long long t, int C, int c, float g, const HybCeOpts& o, float gm) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, lg[k]);
    const float zt = lg[(int)t];
    float s = 0.f, a = 0.f;
    for (int k = 0; k < C; ++k) { const float e = expf(lg[k] - mx); s += e; if (k != (int)t) a += e; }
    const float p = expf(lg[c] - mx) / s;
    const float r = ce_w(w, (int)t) * (p - (c == (int)t ? 1.f : 0.f));
    if (gm == 0.f) return g * r;
    const float u = a / s, py = expf(zt - mx) / s;
    const float M = fmaf(ce_dpow(u, gm) * py, (logf(s) + mx) - zt, ce_pow(u, gm));
    return g * (M * r);
}
__global__ __launch_bounds__(256) void ce_focal_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target, float* __restrict__ loss,
                                                           int B, int C, HybCeOpts o, HybCeFocal fo) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) acc += ce_clip_loss_focal(logits + (long long)b * C, o.weight, target[b], C, o, fo.gamma);
    const float num = ce_tree_sum(acc, part);
    const float den = ce_den(target, o.weight, B, C, o, part);
    if (threadIdx.x == 0) loss[0] = ce_loss_opts(num, den);
}
__global__ __launch_bounds__(256) void ce_focal_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                           const float* __restrict__ dloss, float* __restrict__ dlogits, int B, int C, HybCeOpts o,
                                                           HybCeFocal fo) {
    __shared__ float part[256];
    const float g = ce_gscale_opts(dloss[0], ce_den(target, o.weight, B, C, o, part));
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const long long t = target[b];
    for (int c = 0; c < C; ++c) dlogits[(long long)b * C + c] = ce_clip_dlogit_focal(logits + (long long)b * C, o.weight, t, C, c, g, o, fo.gamma);
}
// Asymmetric, one cell (clip b, class c): with ez = exp(-|z|), p = sigmoid(z), q = sigmoid(-z) (kind 1's overflow-safe form), m = clip,
//   logp = -sp(z),  r = max(p - m, 0),  logn = -sp(-z) if m == 0 else log(min(q + m, 1)),  base = t q + (1 - t) r,
//   gt = gamma t + gamma_neg (1 - t),  L = 1 + (pw - 1) t,  cell = a * e with a = -(w L) and e = base^gt (t logp + (1 - t) logn).
// The cell is handed out as its two factors: the clip's term is r = fmaf(a_c, e_c, r) over c in class order from 0.f, the same fmaf whether
// one thread walks the classes (the stand-alone kernel) or C lanes formed the factors and one thread adds them (the fused tail).
struct CeAsymCell { float p, q, logp, logn, r, base, gt, L; };
__device__ __forceinline__ CeAsymCell ce_asym_cell(float z, float t, float pw, const HybCeFocal& fo) {
    CeAsymCell k;
    const float ez = expf(-fabsf(z)), l1 = log1pf(ez);
    k.p = (z >= 0.f ? 1.f : ez) / (1.f + ez);
    k.q = (z >= 0.f ? ez : 1.f) / (1.f + ez);
    k.logp = -(l1 + fmaxf(-z, 0.f));
    k.r = fmaxf(k.p - fo.clip, 0.f);
    k.logn = fo.clip == 0.f ? -(l1 + fmaxf(z, 0.f)) : logf(fminf(k.q + fo.clip, 1.f));
    k.base = fmaf(t, k.q, (1.f - t) * k.r);
    k.gt = fmaf(fo.gamma, t, fo.gamma_neg * (1.f - t));
    k.L = fmaf(pw - 1.f, t, 1.f);
    return k;
}
__device__ __forceinline__ void ce_asym_factors(float z, float t, float w, float pw, const HybCeFocal& fo, float& a, float& e) {
    const CeAsymCell k = ce_asym_cell(z, t, pw, fo);
    a = -(w * k.L);
    e = ce_pow(k.base, k.gt) * fmaf(t, k.logp, (1.f - t) * k.logn);
}
__device__ __forceinline__ float ce_clip_loss_asym(const float* lg, const float* w, const float* pw, const float* t, int C, const HybCeFocal& fo) {
    float r = 0.f;
    for (int c = 0; c < C; ++c) {
        float a, e;
        ce_asym_factors(lg[c], t[c], ce_w(w, c), ce_w(pw, c), fo, a, e);
        r = fmaf(a, e, r);
    }
    return r;
}
// one clip's d(loss)/d(logits[c]), g = dloss / (B C): the derivative of the cell as written, the focusing factor included.
//   d base / dz = -t p q + (1 - t) [p > m] p q,   d logp / dz = q,   d logn / dz = -p (m == 0), else -[p > m] p q / min(q + m, 1)
__device__ __forceinline__ float ce_clip_dlogit_asym(const float* lg, const float* w, const float* pw, const float* t, int c, float g, const HybCeFocal& fo) {
    const float z = lg[c], tc = t[c];
    const CeAsymCell k = ce_asym_cell(z, tc, ce_w(pw, c), fo);
    const float pq = k.p * k.q;
    const bool open = k.p > fo.clip;                                         // the shifted probability is off its floor
    const float dbase = fmaf(tc, -pq, (1.f - tc) * (open ? pq : 0.f));
    const float dlogn = fo.clip == 0.f ? -k.p : (open ? -(pq / fminf(k.q + fo.clip, 1.f)) : 0.f);
    const float G = fmaf(tc, k.logp, (1.f - tc) * k.logn), dG = fmaf(tc, k.q, (1.f - tc) * dlogn);
    const float F = ce_pow(k.base, k.gt), dF = ce_dpow(k.base, k.gt) * dbase;
    return g * (-(ce_w(w, c) * k.L) * fmaf(dF, G, F * dG));
}
__global__ __launch_bounds__(256) void ce_asym_fwd_kernel(const float* __restrict__ logits, float* __restrict__ loss, int B, int C, HybCeOpts o,
                                                          HybCeDense d, HybCeFocal fo) {
    __shared__ float part[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256)
        acc += ce_clip_loss_asym(logits + (long long)b * C, o.weight, d.pos_weight, d.target + (long long)b * C, C, fo);
    const float num = ce_tree_sum(acc, part);
    if (threadIdx.x == 0) loss[0] = num / ce_dense_div(B, C, 1);
}
__global__ __launch_bounds__(256) void ce_asym_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ dloss, float* __restrict__ dlogits,
                                                          int B, int C, HybCeOpts o, HybCeDense d, HybCeFocal fo) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float g = dloss[0] / ce_dense_div(B, C, 1);
    for (int c = 0; c < C; ++c)
        dlogits[(long long)b * C + c] = ce_clip_dlogit_asym(logits + (long long)b * C, o.weight, d.pos_weight, d.target + (long long)b * C, c, g, fo);
}

// ---- the tail of the temporal part as ONE launch each way --------------------------------------------------------------------
// forward: the last encoder layer's second LayerNorm (+ residual, scale, dropout: src L120-123) -> mean over the clip's tokens -> Linear
// head -> (when a target is given) the clip's cross-entropy term, and the batch mean by the last workgroup to finish.  One workgroup per
// clip, a wave per token row.  Every per-row / per-clip expression is the device function the stand-alone kernels call (ln_fwd_row,
// token_mean's order, head_logit, ce_clip_loss, ce_tree_mean): the fused launch produces the bits of the four launches it replaces.
// A dependent launch costs >= 4.6 us on this chip whatever it computes: these were 4 x ~5 us for 8 x 512 x 8 numbers.
__device__ __forceinline__ float head_logit(const float* pooled, const float* __restrict__ Wrow, int D, int lane) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(pooled[d], Wrow[d], s);
    return wave_sum(s);
}

// OPTS: the loss with options (ce_clip_loss_opts; `o`, and [64] class weights in LDS behind the loss tree).  The plain instantiation is the
// code it always was: every OPTS line is compiled out of it.  nthreads / nclips are the kernel's blockDim.x / gridDim.x, read by the
// __global__ wrappers: read in here, outside a kernel, blockDim.x compiles to the general form (a select on the grid's remainder and a
// 16-bit global load of the implicit arguments) in front of the first row request instead of one scalar load of the kernel argument block.
// MODE 0: the plain loss; 1: with options (OPTS); 2: with options and two targets per clip (OPTS and MIX; `m`): every MIX line is compiled out of
// the other two.  MODE 3 / 4: a dense target of kind 0 / 1 (OPTS and DENSE; `dn`; `target` is null): the clip's target row -- and pos_weight
// for kind 1 -- ride with the up-front requests like the class weights and are staged in LDS, [64] floats each, behind wl; every DENSE line
// is compiled out of the other three.  MODE 5: index focal (OPTS and FOCAL; `fo`): ce_clip_loss_focal on thread 0 like the other index losses
// -- one power and one more accumulate per clip, not worth a hand-over -- with OPTS' two trees and den.  MODE 6: asymmetric (OPTS, DENSE and
// ASYM; kind 1's staging of the target row and pos_weight): an exponential, two logarithms and a power per cell would make thread 0's chain
// grow with C, so lane c forms cell c's two factors (ce_asym_factors), parks them over its own tl[c] / pl[c], and thread 0 runs
// ce_clip_loss_asym's fmaf chain over them in class order: the stand-alone kernel's bits.
template <typename T, int MODE>
__device__ __forceinline__ void temporal_tail_fwd_body(const T* __restrict__ f, const T* __restrict__ x1, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, T* __restrict__ enc_out, float* __restrict__ stats,
                                                       int B, int S, int D, float eps, float out_scale, float p_drop, unsigned long long seed,
                                                       const unsigned long long* __restrict__ seed_inc, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ logits, int C,
                                                       const long long* __restrict__ target, float* __restrict__ loss,
                                                       float* __restrict__ ce_scratch, int rows_in_lds, const HybCeOpts& o, const HybCeMix& m,
                                                       const HybCeDense& dn, const HybCeFocal& fo, const int nthreads,
                                                       const unsigned int nclips) {                 // (the kernel's blockDim.x, gridDim.x)
    constexpr bool OPTS = MODE >= 1, MIX = MODE == 2, DENSE = MODE == 3 || MODE == 4 || MODE == 6, BCE = MODE == 4, FOCAL = MODE == 5, ASYM = MODE == 6;
    constexpr bool PW = BCE || ASYM;
    extern __shared__ __attribute__((aligned(16))) unsigned char tail_smem[];
    float* pooled = reinterpret_cast<float*>(tail_smem);                    // [D]
    float* lg = pooled + D;                                                  // [64] this clip's logits
    float* part = lg + 64;                                                   // [256] loss tree
    float* wl = part + 256;                                                  // [64] class weights (OPTS)
    float* tl = wl + 64;                                                     // [64] the clip's target row, [64] pos_weight (DENSE)
    float* pl = tl + 64;
    T* rows = reinterpret_cast<T*>(part + 256 + (OPTS ? 64 : 0) + (DENSE ? 128 : 0));       // [S][D] when rows_in_lds
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
    const int M = B * S;
    float wreg = 1.f;                                                        // the class weights ride with the up-front requests
    if constexpr (OPTS) { if (tid < C && o.weight) wreg = o.weight[tid]; }
    float treg = 0.f, preg = 1.f;
    if constexpr (DENSE) { if (tid < C) treg = dn.target[(long long)b * C + tid]; }
    if constexpr (PW) { if (tid < C && dn.pos_weight) preg = dn.pos_weight[tid]; }
    // this wave's first class: its weight row does not depend on the tokens -- requested before the LayerNorm rows (a latency-bound kernel: one
    // memory round trip fewer on the critical path), up to 8 x 64 features in registers
    float w0[8];
    const bool pre = wave < C && D <= 512;
#pragma unroll
    for (int j = 0; j < 8; ++j) w0[j] = (pre && lane + 64 * j < D) ? W[(long long)wave * D + lane + 64 * j] : 0.f;
    const float bias0 = (pre && bias) ? bias[wave] : 0.f;
    for (int s = wave; s < S; s += nwaves)
        ln_fwd_row<T>(f, x1, gamma, beta, enc_out, rows_in_lds ? rows + (long long)s * D : nullptr, stats, M, b * S + s, D, eps, out_scale, p_drop,
                      seed, seed_inc, lane);
    if constexpr (OPTS) { if (tid < C) wl[tid] = wreg; }
    if constexpr (DENSE) { if (tid < C) tl[tid] = treg; }
    if constexpr (PW) { if (tid < C) pl[tid] = preg; }
    __syncthreads();                                                         // (also makes the rows just stored to enc_out readable by this workgroup)
    for (int d = tid; d < D; d += nthreads) {
        if (rows_in_lds) {
            float s = 0.f;
            for (int t = 0; t < S; ++t) s += to_f32<T>(rows[(long long)t * D + d]);      // token_mean's order
            pooled[d] = s / (float)S;
        } else pooled[d] = token_mean(enc_out, b, S, D, d);
    }
    __syncthreads();
    for (int c = wave; c < C; c += nwaves) {
        float s;
        if (pre && c == wave) {
            s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int d = lane + 64 * j; if (d < D) s = fmaf(pooled[d], w0[j], s); }      // head_logit's order and rounding
            s = wave_sum(s);
        } else s = head_logit(pooled, W + (long long)c * D, D, lane);
        if (lane == 0) { const float v = s + ((pre && c == wave) ? bias0 : (bias ? bias[c] : 0.f)); logits[b * C + c] = v; lg[c] = v; }
    }
    if constexpr (!DENSE) { if (!target) return; }                           // (a dense target: the loss is always asked for)
    __syncthreads();
    // ce_scratch: [B] per-clip terms, then one ticket word (zero at rest).  The term is published by an agent-scope atomic store (performed at
    // the device's coherence point, not in this XCD's L2), which has completed when vmcnt reaches 0 -- only then is the ticket taken; the last
    // workgroup reads the terms with agent-scope atomic loads.  (The release / acquire pair of the memory model would be an L2 write-back +
    // invalidate per workgroup: ~3 us each on this chip, see optim.hip -- as much as the launch this fusion removes.)
    __shared__ int s_last;
    if constexpr (ASYM) {
        if (tid < C) ce_asym_factors(lg[tid], tl[tid], wl[tid], pl[tid], fo, tl[tid], pl[tid]);
        __syncthreads();
    }
    if (tid == 0) {
        float term;
        if constexpr (ASYM) {
            term = 0.f;
            for (int c = 0; c < C; ++c) term = fmaf(tl[c], pl[c], term);
        } else if constexpr (FOCAL) term = ce_clip_loss_focal(lg, o.weight ? wl : nullptr, target[b], C, o, fo.gamma);
        else if constexpr (BCE) term = ce_clip_loss_bce(lg, o.weight ? wl : nullptr, dn.pos_weight ? pl : nullptr, tl, C);
        else if constexpr (DENSE) term = ce_clip_loss_soft(lg, o.weight ? wl : nullptr, tl, C, o.label_smoothing);
        else if constexpr (MIX) term = ce_clip_loss_mix(lg, o.weight ? wl : nullptr, target[b], m.target_b[b], m.lam[b], C, o);
        else if constexpr (OPTS) term = ce_clip_loss_opts(lg, o.weight ? wl : nullptr, target[b], C, o);
        else term = ce_clip_loss(lg, target[b], C);
        __hip_atomic_store(ce_scratch + b, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned int* ticket = reinterpret_cast<unsigned int*>(ce_scratch + B);
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == nclips - 1;
        if (s_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return;
    float acc = 0.f;
    if (tid < 256)
        for (int i = tid; i < B; i += 256) acc += __hip_atomic_load(ce_scratch + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (DENSE) {          // ce_dense_fwd_kernel's tree and division
        const float num = ce_tree_sum(acc, part);
        if (tid == 0) loss[0] = num / ce_dense_div(B, C, PW ? 1 : 0);
    } else if constexpr (OPTS) {    // ce_opts_fwd_kernel's two trees, the terms coming from the other workgroups
        const float num = ce_tree_sum(acc, part);
        float den;
        if constexpr (MIX) den = ce_den_mix(target, m, o.weight ? wl : nullptr, B, C, o, part);
        else den = ce_den(target, o.weight ? wl : nullptr, B, C, o, part);
        if (tid == 0) loss[0] = ce_loss_opts(num, den);
    } else ce_tree_mean(acc, part, loss, B);
}
template <typename T>
__global__ __launch_bounds__(512) void temporal_tail_fwd_kernel(const T* __restrict__ f, const T* __restrict__ x1, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, T* __restrict__ enc_out, float* __restrict__ stats,
                                                                 int B, int S, int D, float eps, float out_scale, float p_drop, unsigned long long seed,
                                                                 const unsigned long long* __restrict__ seed_inc, const float* __restrict__ W,
                                                                 const float* __restrict__ bias, float* __restrict__ logits, int C,
                                                                 const long long* __restrict__ target, float* __restrict__ loss,
                                                                 float* __restrict__ ce_scratch, int rows_in_lds) {
    temporal_tail_fwd_body<T, 0>(f, x1, gamma, beta, enc_out, stats, B, S, D, eps, out_scale, p_drop, seed, seed_inc, W, bias, logits, C, target, loss,
                                 ce_scratch, rows_in_lds, HybCeOpts{}, HybCeMix{}, HybCeDense{}, HybCeFocal{}, blockDim.x, gridDim.x);
}
template <typename T>
__global__ __launch_bounds__(512) void temporal_tail_fwd_opts_kernel(const T* __restrict__ f, const T* __restrict__ x1, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, T* __restrict__ enc_out, float* __restrict__ stats,
                                                                      int B, int S, int D, float eps, float out_scale, float p_drop,
                                                                      unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                                      float* __restrict__ logits, int C, const long long* __restrict__ target,
                                                                      float* __restrict__ loss, float* __restrict__ ce_scratch, int rows_in_lds,
                                                                      HybCeOpts o) {
    temporal_tail_fwd_body<T, 1>(f, x1, gamma, beta, enc_out, stats, B, S, D, eps, out_scale, p_drop, seed, seed_inc, W, bias, logits, C, target, loss,
                                 ce_scratch, rows_in_lds, o, HybCeMix{}, HybCeDense{}, HybCeFocal{}, blockDim.x, gridDim.x);
}
template <typename T>
__global__ __launch_bounds__(512) void temporal_tail_fwd_mix_kernel(const T* __restrict__ f, const T* __restrict__ x1, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, T* __restrict__ enc_out, float* __restrict__ stats,
                                                                     int B, int S, int D, float eps, float out_scale, float p_drop,
                                                                     unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                                     const float* __restrict__ W, const float* __restrict__ bias,
                                                                     float* __restrict__ logits, int C, const long long* __restrict__ target,
                                                                     float* __restrict__ loss, float* __restrict__ ce_scratch, int rows_in_lds,
                                                                     HybCeOpts o, HybCeMix m) {
    temporal_tail_fwd_body<T, 2>(f, x1, gamma, beta, enc_out, stats, B, S, D, eps, out_scale, p_drop, seed, seed_inc, W, bias, logits, C, target, loss,
                                 ce_scratch, rows_in_lds, o, m, HybCeDense{}, HybCeFocal{}, blockDim.x, gridDim.x);
}
template <typename T, int KIND>
__global__ __launch_bounds__(512) void temporal_tail_fwd_dense_kernel(const T* __restrict__ f, const T* __restrict__ x1, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, T* __restrict__ enc_out, float* __restrict__ stats,
                                                                       int B, int S, int D, float eps, float out_scale, float p_drop,
                                                                       unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                                       const float* __restrict__ W, const float* __restrict__ bias,
                                                                       float* __restrict__ logits, int C, float* __restrict__ loss,
                                                                       float* __restrict__ ce_scratch, int rows_in_lds, HybCeOpts o, HybCeDense dn) {
    temporal_tail_fwd_body<T, 3 + KIND>(f, x1, gamma, beta, enc_out, stats, B, S, D, eps, out_scale, p_drop, seed, seed_inc, W, bias, logits, C, nullptr,
                                        loss, ce_scratch, rows_in_lds, o, HybCeMix{}, dn, HybCeFocal{}, blockDim.x, gridDim.x);
}
template <typename T>
__global__ __launch_bounds__(512) void temporal_tail_fwd_focal_kernel(const T* __restrict__ f, const T* __restrict__ x1, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, T* __restrict__ enc_out, float* __restrict__ stats,
                                                                       int B, int S, int D, float eps, float out_scale, float p_drop,
                                                                       unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                                       const float* __restrict__ W, const float* __restrict__ bias,
                                                                       float* __restrict__ logits, int C, const long long* __restrict__ target,
                                                                       float* __restrict__ loss, float* __restrict__ ce_scratch, int rows_in_lds,
                                                                       HybCeOpts o, HybCeFocal fo) {
    temporal_tail_fwd_body<T, 5>(f, x1, gamma, beta, enc_out, stats, B, S, D, eps, out_scale, p_drop, seed, seed_inc, W, bias, logits, C, target, loss,
                                 ce_scratch, rows_in_lds, o, HybCeMix{}, HybCeDense{}, fo, blockDim.x, gridDim.x);
}
template <typename T>
__global__ __launch_bounds__(512) void temporal_tail_fwd_asym_kernel(const T* __restrict__ f, const T* __restrict__ x1, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, T* __restrict__ enc_out, float* __restrict__ stats,
                                                                      int B, int S, int D, float eps, float out_scale, float p_drop,
                                                                      unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                                      float* __restrict__ logits, int C, float* __restrict__ loss,
                                                                      float* __restrict__ ce_scratch, int rows_in_lds, HybCeOpts o, HybCeDense dn,
                                                                      HybCeFocal fo) {
    temporal_tail_fwd_body<T, 6>(f, x1, gamma, beta, enc_out, stats, B, S, D, eps, out_scale, p_drop, seed, seed_inc, W, bias, logits, C, nullptr, loss,
                                 ce_scratch, rows_in_lds, o, HybCeMix{}, dn, fo, blockDim.x, gridDim.x);
}

// backward: cross-entropy backward (from the saved logits, when a target is given; else the caller's dlogits) -> head backward (the
// clip's token-gradient row v = dlogits W / S; its weight / bias gradient terms as one partial row per clip) -> LayerNorm backward of the
// clip's token rows, whose upstream gradient is v for every token.  Grid (row blocks per clip, clips), four waves, a wave per token row:
// every workgroup of a clip forms the clip's dlogits and v for itself (C x D multiply-adds), the clip's head terms are split among them by
// column.  Everything a workgroup reads -- its rows of the LayerNorm input, the head weights, the token means -- is requested up front: one
// memory round trip.  Writes dx (d LN input), dskip and ln_rows affine-gradient partial rows as ln_residual_bwd_kernel<T, true> does for
// the launch it replaces (workgroup (sb, b) writes row b * nsb + sb; rows no workgroup owns are zero-filled).
// OPTS (a target is given): the loss backward with options; [64] class weights and the [256] den tree in LDS behind lnred.  MODE as in the forward;
// DENSE: [64] class weights, the clip's [64] target row and [64] pos_weight behind lnred, no den tree.  FOCAL (5) is OPTS with
// ce_clip_dlogit_focal, ASYM (6) is DENSE of kind 1 with ce_clip_dlogit_asym: a lane per class either way, as the others.
template <typename T, int MODE>
__device__ __forceinline__ void temporal_tail_bwd_body(const float* __restrict__ dlogits_in, const float* __restrict__ logits,
                                                       const long long* __restrict__ target, const float* __restrict__ dloss,
                                                       const float* __restrict__ W, const T* __restrict__ enc_out, const T* __restrict__ f,
                                                       const float* __restrict__ gamma, const float* __restrict__ stats, T* __restrict__ dx,
                                                       T* __restrict__ dskip, float* __restrict__ ln_part, int ln_rows,
                                                       float* __restrict__ head_part, int B, int S, int D, int C, int rpw, float out_scale,
                                                       float p_drop, unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                       const HybCeOpts& o, const HybCeMix& m, const HybCeDense& dn, const HybCeFocal& fo) {
    constexpr bool OPTS = MODE >= 1, MIX = MODE == 2, DENSE = MODE == 3 || MODE == 4 || MODE == 6, BCE = MODE == 4, FOCAL = MODE == 5, ASYM = MODE == 6;
    constexpr bool PW = BCE || ASYM;
    extern __shared__ __attribute__((aligned(16))) unsigned char tail_smem[];
    float* dl = reinterpret_cast<float*>(tail_smem);                         // [64]
    float* v = dl + 64;                                                      // [D] the clip's token-gradient row (T-rounded values)
    float* lnred = v + D;                                                    // [4][2][D]
    float* wl = lnred + 8 * D;                                               // [64] class weights, [256] den tree (OPTS)
    float* part = wl + 64;
    const int sb = blockIdx.x, nsb = gridDim.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = B * S, nchunk = D >> 3;
    const int s_begin = sb * rpw, s_end = s_begin + rpw < S ? s_begin + rpw : S;
    // ---- requests first
    Vec8<float> gmv[LN_MAXC];
    Vec8<T> xpre[LN_MAXC];
    const int s0 = s_begin + wave;                                           // this wave's first row
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
            gmv[c].load(gamma + ch * 8);
            if (s0 < s_end) xpre[c].load(f + (long long)(b * S + s0) * D + ch * 8);
        }
    }
    const int d_first = sb + tid * nsb;                                      // this thread's first head column: its token mean does not wait for dl
    const float pooled_first = d_first < D ? token_mean(enc_out, b, S, D, d_first) : 0.f;
    if constexpr (DENSE) {
        float* tl = wl + 64;                                                 // [64] the clip's target row, [64] pos_weight
        float* pl = tl + 64;
        if (tid < C) {
            wl[tid] = o.weight ? o.weight[tid] : 1.f;
            tl[tid] = dn.target[(long long)b * C + tid];
            if constexpr (PW) pl[tid] = dn.pos_weight ? dn.pos_weight[tid] : 1.f;
        }
        const float g = dloss[0] / ce_dense_div(B, C, PW ? 1 : 0);
        __syncthreads();
        const float* w = o.weight ? wl : nullptr;
        if constexpr (ASYM) { if (tid < C) dl[tid] = ce_clip_dlogit_asym(logits + (long long)b * C, w, dn.pos_weight ? pl : nullptr, tl, tid, g, fo); }
        else if constexpr (BCE) { if (tid < C) dl[tid] = ce_clip_dlogit_bce(logits + (long long)b * C, w, dn.pos_weight ? pl : nullptr, tl, tid, g); }
        else { if (tid < C) dl[tid] = ce_clip_dlogit_soft(logits + (long long)b * C, w, tl, C, tid, g, o.label_smoothing); }
    } else if constexpr (OPTS) {
        if (tid < C) wl[tid] = o.weight ? o.weight[tid] : 1.f;
        const float dlo = dloss[0];
        __syncthreads();
        const float* w = o.weight ? wl : nullptr;
        if constexpr (MIX) {
            const float g = ce_gscale_opts(dlo, ce_den_mix(target, m, w, B, C, o, part));
            if (tid < C) dl[tid] = ce_clip_dlogit_mix(logits + (long long)b * C, w, target[b], m.target_b[b], m.lam[b], C, tid, g, o);
        } else {
            const float g = ce_gscale_opts(dlo, ce_den(target, w, B, C, o, part));       // the forward's den: same function, same inputs
            if constexpr (FOCAL) { if (tid < C) dl[tid] = ce_clip_dlogit_focal(logits + (long long)b * C, w, target[b], C, tid, g, o, fo.gamma); }
            else { if (tid < C) dl[tid] = ce_clip_dlogit_opts(logits + (long long)b * C, w, target[b], C, tid, g, o); }
        }
    } else {
        if (tid < C) dl[tid] = target ? ce_clip_dlogit(logits + (long long)b * C, target[b], C, tid, dloss[0] / (float)B) : dlogits_in[b * C + tid];
    }
    if (p_drop > 0.f && seed_inc) seed += *seed_inc;
    __syncthreads();
    for (int d = tid; d < D; d += 256) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(dl[c], W[(long long)c * D + d], s);           // head_bwd_dx_kernel's expression
        v[d] = to_f32<T>(from_f32<T>(s / (float)S));
    }
    // the clip's head terms, columns [sb, sb + nsb, ...) of this workgroup
    float* hp = head_part + (long long)b * ((long long)C * D + C);
    for (int d = d_first; d < D; d += 256 * nsb) {
        const float pooled = d == d_first ? pooled_first : token_mean(enc_out, b, S, D, d);
        for (int c = 0; c < C; ++c) hp[(long long)c * D + d] = dl[c] * pooled;
    }
    if (sb == 0 && tid < C) hp[(long long)C * D + tid] = dl[tid];
    __syncthreads();
    float dg[LN_MAXC][8], db[LN_MAXC][8];
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) { dg[c][j] = 0.f; db[c][j] = 0.f; }
    const float inv_keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
    if (s0 < s_end) ln_bwd_row<T, true, true>(nullptr, v, f, gmv, stats, dx, dskip, 0, dg, db, M, b * S + s0, D, out_scale, p_drop, seed, inv_keep, lane, xpre);
    for (int s = s0 + 4; s < s_end; s += 4)
        ln_bwd_row<T, true, false>(nullptr, v, f, gmv, stats, dx, dskip, 0, dg, db, M, b * S + s, D, out_scale, p_drop, seed, inv_keep, lane);
    // the workgroup's partial row: per-wave slots, then the four waves in a fixed order (as ln_residual_bwd_kernel<T, true>)
    float* mine = lnred + wave * 2 * D;
#pragma unroll
    for (int c = 0; c < LN_MAXC; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { mine[ch * 8 + j] = dg[c][j]; mine[D + ch * 8 + j] = db[c][j]; }
        }
    }
    __syncthreads();
    const int prow = b * nsb + sb, nrows = B * nsb;
    for (int i = tid; i < 2 * D; i += 256) {
        ln_part[(long long)prow * 2 * D + i] = (lnred[i] + lnred[2 * D + i]) + (lnred[4 * D + i] + lnred[6 * D + i]);
        for (int r = nrows + prow; r < ln_rows; r += nrows) ln_part[(long long)r * 2 * D + i] = 0.f;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void temporal_tail_bwd_kernel(const float* __restrict__ dlogits_in, const float* __restrict__ logits,
                                                                const long long* __restrict__ target, const float* __restrict__ dloss,
                                                                const float* __restrict__ W, const T* __restrict__ enc_out, const T* __restrict__ f,
                                                                const float* __restrict__ gamma, const float* __restrict__ stats, T* __restrict__ dx,
                                                                T* __restrict__ dskip, float* __restrict__ ln_part, int ln_rows,
                                                                float* __restrict__ head_part, int B, int S, int D, int C, int rpw, float out_scale,
                                                                float p_drop, unsigned long long seed, const unsigned long long* __restrict__ seed_inc) {
    temporal_tail_bwd_body<T, 0>(dlogits_in, logits, target, dloss, W, enc_out, f, gamma, stats, dx, dskip, ln_part, ln_rows, head_part, B, S, D, C,
                                 rpw, out_scale, p_drop, seed, seed_inc, HybCeOpts{}, HybCeMix{}, HybCeDense{}, HybCeFocal{});
}
template <typename T>
__global__ __launch_bounds__(256) void temporal_tail_bwd_opts_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                                     const float* __restrict__ dloss, const float* __restrict__ W,
                                                                     const T* __restrict__ enc_out, const T* __restrict__ f,
                                                                     const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                     T* __restrict__ dx, T* __restrict__ dskip, float* __restrict__ ln_part, int ln_rows,
                                                                     float* __restrict__ head_part, int B, int S, int D, int C, int rpw,
                                                                     float out_scale, float p_drop, unsigned long long seed,
                                                                     const unsigned long long* __restrict__ seed_inc, HybCeOpts o) {
    temporal_tail_bwd_body<T, 1>(nullptr, logits, target, dloss, W, enc_out, f, gamma, stats, dx, dskip, ln_part, ln_rows, head_part, B, S, D, C, rpw,
                                 out_scale, p_drop, seed, seed_inc, o, HybCeMix{}, HybCeDense{}, HybCeFocal{});
}
template <typename T>
__global__ __launch_bounds__(256) void temporal_tail_bwd_mix_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                                    const float* __restrict__ dloss, const float* __restrict__ W,
                                                                    const T* __restrict__ enc_out, const T* __restrict__ f,
                                                                    const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                    T* __restrict__ dx, T* __restrict__ dskip, float* __restrict__ ln_part, int ln_rows,
                                                                    float* __restrict__ head_part, int B, int S, int D, int C, int rpw,
                                                                    float out_scale, float p_drop, unsigned long long seed,
                                                                    const unsigned long long* __restrict__ seed_inc, HybCeOpts o, HybCeMix m) {
    temporal_tail_bwd_body<T, 2>(nullptr, logits, target, dloss, W, enc_out, f, gamma, stats, dx, dskip, ln_part, ln_rows, head_part, B, S, D, C, rpw,
                                 out_scale, p_drop, seed, seed_inc, o, m, HybCeDense{}, HybCeFocal{});
}
template <typename T, int KIND>
__global__ __launch_bounds__(256) void temporal_tail_bwd_dense_kernel(const float* __restrict__ logits, const float* __restrict__ dloss,
                                                                      const float* __restrict__ W, const T* __restrict__ enc_out,
                                                                      const T* __restrict__ f, const float* __restrict__ gamma,
                                                                      const float* __restrict__ stats, T* __restrict__ dx, T* __restrict__ dskip,
                                                                      float* __restrict__ ln_part, int ln_rows, float* __restrict__ head_part, int B,
                                                                      int S, int D, int C, int rpw, float out_scale, float p_drop,
                                                                      unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                                      HybCeOpts o, HybCeDense dn) {
    temporal_tail_bwd_body<T, 3 + KIND>(nullptr, logits, nullptr, dloss, W, enc_out, f, gamma, stats, dx, dskip, ln_part, ln_rows, head_part, B, S, D, C,
                                        rpw, out_scale, p_drop, seed, seed_inc, o, HybCeMix{}, dn, HybCeFocal{});
}
template <typename T>
__global__ __launch_bounds__(256) void temporal_tail_bwd_focal_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                                      const float* __restrict__ dloss, const float* __restrict__ W,
                                                                      const T* __restrict__ enc_out, const T* __restrict__ f,
                                                                      const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                      T* __restrict__ dx, T* __restrict__ dskip, float* __restrict__ ln_part, int ln_rows,
                                                                      float* __restrict__ head_part, int B, int S, int D, int C, int rpw,
                                                                      float out_scale, float p_drop, unsigned long long seed,
                                                                      const unsigned long long* __restrict__ seed_inc, HybCeOpts o, HybCeFocal fo) {
    temporal_tail_bwd_body<T, 5>(nullptr, logits, target, dloss, W, enc_out, f, gamma, stats, dx, dskip, ln_part, ln_rows, head_part, B, S, D, C, rpw,
                                 out_scale, p_drop, seed, seed_inc, o, HybCeMix{}, HybCeDense{}, fo);
}
template <typename T>
__global__ __launch_bounds__(256) void temporal_tail_bwd_asym_kernel(const float* __restrict__ logits, const float* __restrict__ dloss,
                                                                     const float* __restrict__ W, const T* __restrict__ enc_out,
                                                                     const T* __restrict__ f, const float* __restrict__ gamma,
                                                                     const float* __restrict__ stats, T* __restrict__ dx, T* __restrict__ dskip,
                                                                     float* __restrict__ ln_part, int ln_rows, float* __restrict__ head_part, int B,
                                                                     int S, int D, int C, int rpw, float out_scale, float p_drop,
                                                                     unsigned long long seed, const unsigned long long* __restrict__ seed_inc,
                                                                     HybCeOpts o, HybCeDense dn, HybCeFocal fo) {
    temporal_tail_bwd_body<T, 6>(nullptr, logits, nullptr, dloss, W, enc_out, f, gamma, stats, dx, dskip, ln_part, ln_rows, head_part, B, S, D, C, rpw,
                                 out_scale, p_drop, seed, seed_inc, o, HybCeMix{}, dn, fo);
}

// ---- evaluation: an accumulating classification meter behind the logits (hyb_eval_metrics; include/hybrid_hip.h states the rules) --------
// ONE workgroup of 256 threads, thread t owns videos t, t + 256, .. as in ce_opts_fwd_kernel: evaluation batches are tens to a few hundred
// videos of a handful of classes, and a single workgroup makes the final add into the caller's block without any hand-off -- launches on
// one stream are ordered, so neither a ticket nor a floating-point atomic is needed and the sums are reproducible bit for bit.
// V == 1: the scores are the logits and the loss term is ce_clip_loss_opts / ce_clip_den themselves (a validation loss is the training
// criterion's arithmetic).  V > 1: the scores are the mean of the views' softmax rows, formed in fp32 in the video's own `scores` row (the
// owning thread's scratch), and the term is the criterion's formula with -log(pbar_c) where it has lse - z_c.
// ONE body for every criterion the meter knows, templated on the loss mode as the temporal tail is: HYB_LOSS_OPTS (hyb_eval_metrics),
// HYB_LOSS_FOCAL (hyb_eval_metrics_focal) and HYB_LOSS_SOFT (hyb_eval_metrics_soft; the target is the dense row l.d.target[b], its label the
// lowest index among the row's maxima).  Only the loss term, the den share and the form of the target differ: scores, pred, ranks,
// counters and confusion are the same statements in every instantiation.
struct HybEvalArgs {
    const float* logits; const long long* target; double* sums; long long* counts; long long* confusion; long long* pred; float* scores;
    int B, C, V, topk;
};
__device__ __forceinline__ float eval_clip_loss_probs(const float* p, const float* w, long long t, int C, const HybCeOpts& o) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    float r = (1.f - o.label_smoothing) * (ce_w(w, (int)t) * -logf(p[(int)t]));
    if (o.label_smoothing > 0.f) {
        float sm = 0.f;
        for (int c = 0; c < C; ++c) sm += ce_w(w, c) * -logf(p[c]);
        r += (o.label_smoothing / (float)C) * sm;
    }
    return r;
}
// V > 1, focal: ubar = sum_{c != y} pbar_c in class order (not 1 - pbar_y); gm == 0 returns eval_clip_loss_probs' bits at label smoothing 0
__device__ __forceinline__ float eval_clip_loss_probs_focal(const float* p, const float* w, long long t, int C, const HybCeOpts& o, float gm) {
    if (!ce_keep(t, o)) return 0.f;
    if (!(t >= 0 && t < C)) return NAN;
    const float r = ce_w(w, (int)t) * -logf(p[(int)t]);
    if (gm == 0.f) return r;
    float u = 0.f;
    for (int c = 0; c < C; ++c)
        if (c != (int)t) u += p[c];
    return ce_pow(u, gm) * r;
}
// V > 1, soft targets: ce_clip_loss_soft's chain with -log(pbar_c) where it has lse - z_c
__device__ __forceinline__ float eval_clip_loss_probs_soft(const float* p, const float* w, const float* t, int C, float e) {
    float r = 0.f;
    for (int c = 0; c < C; ++c) r = fmaf(ce_w(w, c) * ce_soft_q(t[c], e, C), -logf(p[c]), r);
    return r;
}
// a soft row's label for top-1 / top-k / confusion: the lowest index among its maxima (strict >, as pred); a row holding a NaN has none
__device__ __forceinline__ long long eval_soft_label(const float* t, int C) {
    bool has_nan = false;
    int y = 0;
    float best = t[0];
    for (int c = 0; c < C; ++c) {
        const float v = t[c];
        has_nan |= v != v;
        if (v > best) { best = v; y = c; }
    }
    return has_nan ? -1 : y;
}
template <int MODE>
__global__ __launch_bounds__(256) void eval_metrics_kernel(HybEvalArgs a, HybLoss l) {
    static_assert(MODE == HYB_LOSS_OPTS || MODE == HYB_LOSS_FOCAL || MODE == HYB_LOSS_SOFT, "the classification meter's criteria");
    const HybCeOpts& o = l.o;
    __shared__ double partd[2][256];
    __shared__ int parti[4][256];
    const int C = a.C, V = a.V;
    double num = 0.0, den = 0.0;
    int kept = 0, top1 = 0, topk = 0, nans = 0;
    for (int b = threadIdx.x; b < a.B; b += 256) {
        const float* tl = nullptr;                                              // SOFT: the video's target row
        long long t;
        if constexpr (MODE == HYB_LOSS_SOFT) {
            tl = l.d.target + (long long)b * C;
            t = eval_soft_label(tl, C);                                         // -1: no label -- kept, wrong, no confusion entry
        } else t = a.target[b];
        const float* s = a.logits + (long long)b * V * C;                       // V == 1: the scores are the logits
        float term;
        if (V > 1) {
            float* sc = a.scores + (long long)b * C;
            for (int v = 0; v < V; ++v) {
                const float* z = s + (long long)v * C;
                float mx = -INFINITY;
                for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
                float e = 0.f;
                for (int c = 0; c < C; ++c) e += expf(z[c] - mx);
                for (int c = 0; c < C; ++c) {
                    const float p = expf(z[c] - mx) / e;
                    sc[c] = v ? sc[c] + p : p;
                }
            }
            for (int c = 0; c < C; ++c) sc[c] = sc[c] / (float)V;
            s = sc;
            if constexpr (MODE == HYB_LOSS_FOCAL) term = eval_clip_loss_probs_focal(sc, o.weight, t, C, o, l.f.gamma);
            else if constexpr (MODE == HYB_LOSS_SOFT) term = eval_clip_loss_probs_soft(sc, o.weight, tl, C, o.label_smoothing);
            else term = eval_clip_loss_probs(sc, o.weight, t, C, o);
        } else {
            if constexpr (MODE == HYB_LOSS_FOCAL) term = ce_clip_loss_focal(s, o.weight, t, C, o, l.f.gamma);
            else if constexpr (MODE == HYB_LOSS_SOFT) term = ce_clip_loss_soft(s, o.weight, tl, C, o.label_smoothing);
            else term = ce_clip_loss_opts(s, o.weight, t, C, o);
            if (a.scores)
                for (int c = 0; c < C; ++c) a.scores[(long long)b * C + c] = s[c];
        }
        bool has_nan = false;
        int pred = 0;
        float best = s[0];
        for (int c = 0; c < C; ++c) {
            const float v = s[c];
            has_nan |= v != v;
            if (v > best) { best = v; pred = c; }                               // strict: the lowest index among the maxima
        }
        if (has_nan) pred = -1;
        if (a.pred) a.pred[b] = pred;
        if (!ce_keep(t, o)) continue;                                           // ignored: seen, and nothing else
        num += (double)term;
        if constexpr (MODE == HYB_LOSS_SOFT) den += 1.0;                        // the criterion's divisor is B
        else den += (double)ce_clip_den(o.weight, t, C, o);
        ++kept;
        if (has_nan) { ++nans; continue; }                                      // wrong for both accuracies, no confusion entry
        if (!(t >= 0 && t < C)) continue;                                       // kept and wrong; the sums went NaN above
        const float sy = s[(int)t];
        int rank = 0;
        for (int c = 0; c < C; ++c) rank += (s[c] > sy || (c < (int)t && s[c] == sy)) ? 1 : 0;
        top1 += rank == 0 ? 1 : 0;
        topk += rank < a.topk ? 1 : 0;
        // integer adds commute: whichever order the owning threads arrive in, the cell ends at the same value
        if (a.confusion) atomicAdd(reinterpret_cast<unsigned long long*>(a.confusion + t * C + pred), 1ull);
    }
    const int tid = threadIdx.x;
    partd[0][tid] = num; partd[1][tid] = den;
    parti[0][tid] = kept; parti[1][tid] = top1; parti[2][tid] = topk; parti[3][tid] = nans;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                                         // the fixed 256-leaf tree, in double
        if (tid < h) {
            partd[0][tid] += partd[0][tid + h]; partd[1][tid] += partd[1][tid + h];
            for (int k = 0; k < 4; ++k) parti[k][tid] += parti[k][tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {                                                             // the one add into the caller's block
        a.sums[0] += partd[0][0];
        a.sums[1] += partd[1][0];
        a.counts[0] += a.B;
        for (int k = 0; k < 4; ++k) a.counts[1 + k] += parti[k][0];
    }
}

// ---- evaluation of multi-label clips (hyb_eval_multilabel; include/hybrid_hip.h states the rules) ------------------------------------------
// The same shape as eval_metrics_kernel: ONE workgroup, thread t owns videos t, t + 256, .., the loss in double over the fixed tree, one
// thread makes the final add.  V == 1: the term is ce_clip_loss_bce itself, the criterion's function.  The score bank is appended without a
// hand-off: every thread reads the cursor counts[3] before the first barrier, video b owns row cursor + b, and thread 0 moves the cursor
// after the last barrier, when nobody reads it any more.
// ONE body for both criteria, templated on the loss mode: HYB_LOSS_BCE (hyb_eval_multilabel) and HYB_LOSS_ASYM (hyb_eval_multilabel_asym,
// `fo`).  V == 1: ce_clip_loss_asym stands where ce_clip_loss_bce does; V > 1: the asymmetric cell on the mean scores is formed in the
// class loop that forms them, so neither instantiation walks a row a fourth time.
struct HybEvalMlArgs {
    const float* logits; const float* target; const float* weight; const float* pos_weight; const float* threshold;
    double* sums; long long* counts; long long* cells; float* bank_scores; unsigned char* bank_labels; long long capacity;
    unsigned char* pred; float* scores;
    int B, C, V;
};
__device__ __forceinline__ float eval_sigmoid(float z) {                        // ce_clip_dlogit_bce's: no overflow at any z, sg(0) = 0.5
    const float ez = expf(-fabsf(z));
    return (z >= 0.f ? 1.f : ez) / (1.f + ez);
}
__device__ __forceinline__ float eval_log_floor(float l) { return l < -100.f ? -100.f : l; }      // torch's clamp: a NaN passes through
// V > 1, asymmetric: ce_asym_factors with p -> s (the mean sigmoid), q -> qb (the mean of sigmoid(-z), its own sum) and the logs floored
__device__ __forceinline__ void eval_asym_factors(float s, float qb, float t, float w, float pw, const HybCeFocal& fo, float& a, float& e) {
    const float logp = eval_log_floor(logf(s));
    const float logn = fo.clip == 0.f ? eval_log_floor(logf(qb)) : logf(fminf(qb + fo.clip, 1.f));
    const float r = fmaxf(s - fo.clip, 0.f);
    const float base = fmaf(t, qb, (1.f - t) * r);
    const float gt = fmaf(fo.gamma, t, fo.gamma_neg * (1.f - t));
    const float L = fmaf(pw - 1.f, t, 1.f);
    a = -(w * L);
    e = ce_pow(base, gt) * fmaf(t, logp, (1.f - t) * logn);
}
template <int MODE>
__global__ __launch_bounds__(256) void eval_multilabel_kernel(HybEvalMlArgs a, HybCeFocal fo) {
    static_assert(MODE == HYB_LOSS_BCE || MODE == HYB_LOSS_ASYM, "the multi-label meter's criteria");
    __shared__ double partd[256];
    __shared__ int parti[2][256];
    const int C = a.C, V = a.V;
    const bool bank = a.bank_scores != nullptr;
    const long long cursor = a.counts[3];                                       // read by every thread before the first barrier
    double num = 0.0;
    int nans = 0, exact = 0;
    // the inputs are only read here: saying so lets their loads move ahead of the stores and integer adds of the loop below (a batch of 8
    // videos is 8 lanes walking their rows alone, so what the kernel takes is its chain of dependent memory round trips)
    const float* __restrict__ logits = a.logits;
    const float* __restrict__ target = a.target;
    const float* __restrict__ weight = a.weight;
    const float* __restrict__ pos_weight = a.pos_weight;
    const float* __restrict__ threshold = a.threshold;
    for (int b = threadIdx.x; b < a.B; b += 256) {
        const float* __restrict__ z = logits + (long long)b * V * C;
        const float* __restrict__ t = target + (long long)b * C;
        float* sc = a.scores + (long long)b * C;
        // a score is NaN exactly when one of its logits is (the sigmoid of anything else lies in [0, 1], and so does a mean of those): the
        // video's NaN flag, which every prediction below needs, comes from a pass of loads alone
        bool has_nan = false;
        for (int i = 0; i < V * C; ++i) has_nan |= z[i] != z[i];
        float term = 0.f;
        if (V == 1) {
            if constexpr (MODE == HYB_LOSS_ASYM) term = ce_clip_loss_asym(z, weight, pos_weight, t, C, fo);
            else term = ce_clip_loss_bce(z, weight, pos_weight, t, C);
        }
        const long long r = cursor + b;
        const bool store = bank && r >= 0 && r < a.capacity;                    // nothing at or beyond capacity, whatever the cursor holds
        bool match = !has_nan;
        for (int c = 0; c < C; ++c) {
            float s = eval_sigmoid(z[c]);
            const float tc = t[c];
            if constexpr (MODE == HYB_LOSS_ASYM) {
                if (V > 1) {
                    float qb = eval_sigmoid(-z[c]);
                    for (int v = 1; v < V; ++v) {
                        const float zv = z[(long long)v * C + c];
                        s += eval_sigmoid(zv);
                        qb += eval_sigmoid(-zv);
                    }
                    s = s / (float)V;
                    qb = qb / (float)V;
                    float fa, fe;
                    eval_asym_factors(s, qb, tc, ce_w(weight, c), ce_w(pos_weight, c), fo, fa, fe);
                    term = fmaf(fa, fe, term);
                }
            } else if (V > 1) {
                for (int v = 1; v < V; ++v) s += eval_sigmoid(z[(long long)v * C + c]);
                s = s / (float)V;
                term = fmaf(ce_w(weight, c), fmaf(ce_w(pos_weight, c) * tc, -eval_log_floor(logf(s)), (1.f - tc) * -eval_log_floor(log1pf(-s))), term);
            }
            sc[c] = s;
            const bool y = tc >= 0.5f;                                          // a NaN target: negative
            const bool p = !has_nan && s >= threshold[c];                       // on the fp32 score just written
            if (a.pred) a.pred[(long long)b * C + c] = p ? 1 : 0;
            // integer adds commute: whichever order the owning threads arrive in, the cell ends at the same value
            if (p || y) atomicAdd(reinterpret_cast<unsigned long long*>(a.cells + 3ll * c + (p ? (y ? 0 : 1) : 2)), 1ull);
            match &= p == y;
            if (store) {
                a.bank_scores[r * C + c] = has_nan ? -INFINITY : s;
                a.bank_labels[r * C + c] = y ? 1 : 0;
            }
        }
        num += (double)term;
        nans += has_nan ? 1 : 0;
        exact += match ? 1 : 0;
    }
    const int tid = threadIdx.x;
    partd[tid] = num;
    parti[0][tid] = nans; parti[1][tid] = exact;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                                         // the fixed 256-leaf tree, in double
        if (tid < h) {
            partd[tid] += partd[tid + h];
            parti[0][tid] += parti[0][tid + h]; parti[1][tid] += parti[1][tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {                                                             // the one add into the caller's block
        a.sums[0] += partd[0];
        a.counts[0] += a.B;
        a.counts[1] += parti[0][0];
        a.counts[2] += parti[1][0];
        if (bank) {
            const long long end = cursor + a.B, stored = end < a.capacity ? end : a.capacity;
            a.counts[3] = stored;
            a.counts[4] += end - stored;
        }
    }
}

}  // namespace

extern "C" int hyb_ln_residual_fwd(int dtype, const void* x, const void* skip, const float* gamma, const float* beta, void* y, float* stats,
                                   int M, int D, float eps, float out_scale, float p_drop, unsigned long long seed, void* stream) {
    return hyb_ln_residual_fwd_inc(dtype, x, skip, gamma, beta, y, stats, M, D, eps, out_scale, p_drop, seed, nullptr, stream);
}
int hyb_ln_residual_fwd_inc(int dtype, const void* x, const void* skip, const float* gamma, const float* beta, void* y, float* stats,
                            int M, int D, float eps, float out_scale, float p_drop, unsigned long long seed, const unsigned long long* seed_inc,
                            void* stream) {
    HYB_CHECK_ARG(x && skip && gamma && beta && y && stats && M > 0 && D > 0 && D % 8 == 0 && D <= 64 * 8 * LN_MAXC && p_drop >= 0.f && p_drop < 1.f);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(hyb_cdiv(M, 4));
    if (dtype == HYB_F32)
        hipLaunchKernelGGL(ln_residual_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (const float*)skip, gamma, beta, (float*)y, stats, M, D, eps, out_scale, p_drop, seed, seed_inc);
    else if (dtype == HYB_BF16)
        hipLaunchKernelGGL(ln_residual_fwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)x, (const bf16*)skip, gamma, beta, (bf16*)y, stats, M, D, eps, out_scale, p_drop, seed, seed_inc);
    else return HYB_E_ARG;
    HYB_LAUNCH_CHECK();
    return 0;
}

extern "C" int hyb_ln_residual_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* stats, void* dx, void* dskip,
                                   int accumulate_dskip, float* dgamma, float* dbeta, int M, int D, float out_scale, float p_drop,
                                   unsigned long long seed, void* stream) {
    HYB_CHECK_ARG(dy && x && gamma && stats && dx && dskip && dgamma && dbeta && M > 0 && D > 0 && D % 8 == 0 && D <= 64 * 8 * LN_MAXC);
    hipStream_t st = (hipStream_t)stream;
    int blocks = hyb_cdiv(M, 4);
    if (blocks > 32) blocks = 32;
    const size_t lnlds = 2 * (size_t)D * sizeof(float);
    if (dtype == HYB_F32)
        hipLaunchKernelGGL((ln_residual_bwd_kernel<float, false>), dim3(blocks), dim3(256), lnlds, st, (const float*)dy, (const float*)x, gamma, stats, (float*)dx, (float*)dskip, accumulate_dskip, dgamma, dbeta, M, D, out_scale, p_drop, seed, (const unsigned long long*)nullptr);
    else if (dtype == HYB_BF16)
        hipLaunchKernelGGL((ln_residual_bwd_kernel<bf16, false>), dim3(blocks), dim3(256), lnlds, st, (const bf16*)dy, (const bf16*)x, gamma, stats, (bf16*)dx, (bf16*)dskip, accumulate_dskip, dgamma, dbeta, M, D, out_scale, p_drop, seed, (const unsigned long long*)nullptr);
    else return HYB_E_ARG;
    HYB_LAUNCH_CHECK();
    return 0;
}

// Internal (encoder composite): deterministic variant.  Writes hyb_ln_bwd_rows(M) partial rows [rows][2][D] to `part`;
// hyb_ln_rows_reduce sums any number of such rows into dgamma/dbeta (overwriting them).
int hyb_ln_bwd_rows(int M) { int b = hyb_cdiv(M, 4); return b > 32 ? 32 : b; }
int hyb_ln_residual_bwd_rows(int dtype, const void* dy, const void* x, const float* gamma, const float* stats, void* dx, void* dskip,
                             int accumulate_dskip, float* part, int M, int D, float out_scale, float p_drop, unsigned long long seed, const unsigned long long* seed_inc,
                             hipStream_t st) {
    HYB_CHECK_ARG(dy && x && gamma && stats && dx && dskip && part && M > 0 && D > 0 && D % 8 == 0 && D <= 64 * 8 * LN_MAXC);
    const int blocks = hyb_ln_bwd_rows(M);
    const size_t lnlds = 8 * (size_t)D * sizeof(float);
    if (dtype == HYB_F32)
        hipLaunchKernelGGL((ln_residual_bwd_kernel<float, true>), dim3(blocks), dim3(256), lnlds, st, (const float*)dy, (const float*)x, gamma, stats, (float*)dx, (float*)dskip, accumulate_dskip, part, (float*)nullptr, M, D, out_scale, p_drop, seed, seed_inc);
    else if (dtype == HYB_BF16)
        hipLaunchKernelGGL((ln_residual_bwd_kernel<bf16, true>), dim3(blocks), dim3(256), lnlds, st, (const bf16*)dy, (const bf16*)x, gamma, stats, (bf16*)dx, (bf16*)dskip, accumulate_dskip, part, (float*)nullptr, M, D, out_scale, p_drop, seed, seed_inc);
    else return HYB_E_ARG;
    HYB_LAUNCH_CHECK();
    return 0;
}
int hyb_ln_rows_reduce(const float* part, int rows, int D, float* dgamma, float* dbeta, hipStream_t st) {
    hipLaunchKernelGGL(ln_rows_reduce_kernel, dim3(hyb_cdiv(2 * D, 32)), dim3(1024), 0, st, part, rows, D, dgamma, dbeta);
    HYB_LAUNCH_CHECK();
    return 0;
}

// Internal (fused.hip): the temporal tail.  hyb_temporal_tail_ok: the shapes the one-workgroup-per-clip kernels take.
int hyb_temporal_tail_ok(int B, int S, int D, int C, int ln_rows) {
    return B >= 1 && B <= ln_rows && S >= 1 && D % 8 == 0 && D <= 1536 && C >= 1 && C <= 64;       // (D: 64 KB of LDS in the backward)
}
// l: the loss in the same launch, or nullptr.  One kernel wrapper per HybLossMode (`launch`, T = float / bf16): the arguments every wrapper
// takes, then the mode's own.  LDS behind the common part: [64] class weights for every mode with options, [64] + [64] target row and
// pos_weight more for the dense ones.
int hyb_temporal_tail_fwd(int dtype, const void* f, const void* x1, const float* gamma, const float* beta, void* enc_out, float* stats, int B, int S,
                          int D, float eps, float out_scale, float p_drop, unsigned long long seed, const unsigned long long* seed_inc, const float* W,
                          const float* bias, float* logits, int C, float* loss, float* ce_scratch, hipStream_t st, const HybLoss* l) {
    HYB_CHECK_ARG(f && x1 && gamma && beta && enc_out && stats && W && logits && (!l || (loss && ce_scratch && hyb_loss_ok(*l))));
    HYB_CHECK_ARG(dtype == HYB_F32 || dtype == HYB_BF16);
    const int mode = l ? l->mode : HYB_LOSS_PLAIN;
    const size_t es = dtype == HYB_F32 ? 4 : 2;
    const size_t base = ((size_t)D + 64 + 256 + (mode != HYB_LOSS_PLAIN ? 64 : 0) + (hyb_loss_is_dense(mode) ? 128 : 0)) * sizeof(float);
    const int rows_in_lds = base + (size_t)S * D * es <= 60 * 1024;
    const size_t lds = base + (rows_in_lds ? (size_t)S * D * es : 0);
    const int threads = S >= 8 ? 512 : 256;             // (1024 threads leave 128 registers per lane: the LayerNorm row spills -- measured 13 -> 24 us)
    auto launch = [&](auto t) {
        using T = decltype(t);
#define HYB_TAIL_FWD(kernel, ...)                                                                                                                 \
    hipLaunchKernelGGL(kernel, dim3(B), dim3(threads), lds, st, (const T*)f, (const T*)x1, gamma, beta, (T*)enc_out, stats, B, S, D, eps, out_scale, \
                       p_drop, seed, seed_inc, W, bias, logits, C, __VA_ARGS__)
        switch (mode) {
        case HYB_LOSS_PLAIN: HYB_TAIL_FWD(temporal_tail_fwd_kernel<T>, l ? l->target : nullptr, loss, ce_scratch, rows_in_lds); break;
        case HYB_LOSS_OPTS: HYB_TAIL_FWD(temporal_tail_fwd_opts_kernel<T>, l->target, loss, ce_scratch, rows_in_lds, l->o); break;
        case HYB_LOSS_MIX: HYB_TAIL_FWD(temporal_tail_fwd_mix_kernel<T>, l->target, loss, ce_scratch, rows_in_lds, l->o, l->m); break;
        case HYB_LOSS_SOFT: HYB_TAIL_FWD((temporal_tail_fwd_dense_kernel<T, 0>), loss, ce_scratch, rows_in_lds, l->o, l->d); break;
        case HYB_LOSS_BCE: HYB_TAIL_FWD((temporal_tail_fwd_dense_kernel<T, 1>), loss, ce_scratch, rows_in_lds, l->o, l->d); break;
        case HYB_LOSS_FOCAL: HYB_TAIL_FWD(temporal_tail_fwd_focal_kernel<T>, l->target, loss, ce_scratch, rows_in_lds, l->o, l->f); break;
        case HYB_LOSS_ASYM: HYB_TAIL_FWD(temporal_tail_fwd_asym_kernel<T>, loss, ce_scratch, rows_in_lds, l->o, l->d, l->f); break;
        }
#undef HYB_TAIL_FWD
    };
    if (dtype == HYB_F32) launch(float{});
    else launch(bf16{});
    HYB_LAUNCH_CHECK();
    return 0;
}
// l: the loss backward from the saved logits and dloss in the same launch; nullptr: the caller's dlogits.  LDS behind the common part: [64]
// class weights, target row and pos_weight for the dense modes, [64] class weights and the [256] den tree for the others with options.
int hyb_temporal_tail_bwd(int dtype, const float* dlogits, const float* logits, const float* dloss, const float* W, const void* enc_out,
                          const void* f, const float* gamma, const float* stats, void* dx, void* dskip, float* ln_part, int ln_rows,
                          float* head_part, int B, int S, int D, int C, float out_scale, float p_drop, unsigned long long seed,
                          const unsigned long long* seed_inc, hipStream_t st, const HybLoss* l) {
    HYB_CHECK_ARG((l ? !dlogits && logits && dloss && hyb_loss_ok(*l) : dlogits != nullptr) && W && enc_out && f && gamma && stats && dx && dskip && ln_part &&
                  head_part);
    HYB_CHECK_ARG(dtype == HYB_F32 || dtype == HYB_BF16);
    const int mode = l ? l->mode : HYB_LOSS_PLAIN;
    const size_t lds = (64 + 9 * (size_t)D + (hyb_loss_is_dense(mode) ? 3 * 64 : mode != HYB_LOSS_PLAIN ? 64 + 256 : 0)) * sizeof(float);
    // row blocks per clip: as many as the ln_rows partial rows allow (>= 1: hyb_temporal_tail_ok), four-row granules
    int nsb = hyb_cdiv(S, 4);
    if (nsb > ln_rows / B) nsb = ln_rows / B;
    const int rpw = hyb_cdiv(hyb_cdiv(S, nsb), 4) * 4;
    nsb = hyb_cdiv(S, rpw);
    const dim3 grid(nsb, B);
    if (lds > 64 * 1024) return HYB_E_ARG;
    auto launch = [&](auto t) {
        using T = decltype(t);
#define HYB_TAIL_BWD(kernel, ...) hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, __VA_ARGS__)
#define HYB_TAIL_BWD_COMMON                                                                                                                      \
    dloss, W, (const T*)enc_out, (const T*)f, gamma, stats, (T*)dx, (T*)dskip, ln_part, ln_rows, head_part, B, S, D, C, rpw, out_scale, p_drop, seed, \
        seed_inc
        switch (mode) {
        case HYB_LOSS_PLAIN: HYB_TAIL_BWD(temporal_tail_bwd_kernel<T>, dlogits, logits, l ? l->target : nullptr, HYB_TAIL_BWD_COMMON); break;
        case HYB_LOSS_OPTS: HYB_TAIL_BWD(temporal_tail_bwd_opts_kernel<T>, logits, l->target, HYB_TAIL_BWD_COMMON, l->o); break;
        case HYB_LOSS_MIX: HYB_TAIL_BWD(temporal_tail_bwd_mix_kernel<T>, logits, l->target, HYB_TAIL_BWD_COMMON, l->o, l->m); break;
        case HYB_LOSS_SOFT: HYB_TAIL_BWD((temporal_tail_bwd_dense_kernel<T, 0>), logits, HYB_TAIL_BWD_COMMON, l->o, l->d); break;
        case HYB_LOSS_BCE: HYB_TAIL_BWD((temporal_tail_bwd_dense_kernel<T, 1>), logits, HYB_TAIL_BWD_COMMON, l->o, l->d); break;
        case HYB_LOSS_FOCAL: HYB_TAIL_BWD(temporal_tail_bwd_focal_kernel<T>, logits, l->target, HYB_TAIL_BWD_COMMON, l->o, l->f); break;
        case HYB_LOSS_ASYM: HYB_TAIL_BWD(temporal_tail_bwd_asym_kernel<T>, logits, HYB_TAIL_BWD_COMMON, l->o, l->d, l->f); break;
        }
#undef HYB_TAIL_BWD_COMMON
#undef HYB_TAIL_BWD
    };
    if (dtype == HYB_F32) launch(float{});
    else launch(bf16{});
    HYB_LAUNCH_CHECK();
    return 0;
}

extern "C" int hyb_head_fwd(int dtype, const void* x, const float* W, const float* b, float* logits, int B, int S, int D, int C, void* stream) {
    HYB_CHECK_ARG(x && W && logits && B > 0 && S > 0 && D > 0 && C > 0);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)D * sizeof(float);
    if (dtype == HYB_F32) hipLaunchKernelGGL(head_fwd_kernel<float>, dim3(B), dim3(256), lds, st, (const float*)x, W, b, logits, S, D, C);
    else if (dtype == HYB_BF16) hipLaunchKernelGGL(head_fwd_kernel<bf16>, dim3(B), dim3(256), lds, st, (const bf16*)x, W, b, logits, S, D, C);
    else return HYB_E_ARG;
    HYB_LAUNCH_CHECK();
    return 0;
}

extern "C" int hyb_head_bwd(int dtype, const void* x, const float* W, const float* dlogits, void* dx, float* dW, float* db, int B, int S, int D,
                            int C, void* stream) {
    HYB_CHECK_ARG(x && W && dlogits && B > 0 && S > 0 && D > 0 && C > 0 && C <= 64);
    hipStream_t st = (hipStream_t)stream;
    if (dtype != HYB_F32 && dtype != HYB_BF16) return HYB_E_ARG;
    if (dx && !dW) {
        if (dtype == HYB_F32) hipLaunchKernelGGL(head_bwd_dx_kernel<float>, dim3(B), dim3(256), 0, st, W, dlogits, (float*)dx, S, D, C);
        else hipLaunchKernelGGL(head_bwd_dx_kernel<bf16>, dim3(B), dim3(256), 0, st, W, dlogits, (bf16*)dx, S, D, C);
        HYB_LAUNCH_CHECK();
    }
    if (dW) {        // one launch: weight/bias gradient blocks, and (when asked) the input-gradient blocks riding behind them
        const int yb = hyb_cdiv(C, 16), xb = dx ? hyb_cdiv(B, 4) : 0;
        if (dtype == HYB_F32) hipLaunchKernelGGL(head_bwd_dw_kernel<float>, dim3(hyb_cdiv(D, 64), yb + xb), dim3(256), 0, st, (const float*)x, dlogits, dW, db, B, S, D, C, W, (float*)dx, yb);
        else hipLaunchKernelGGL(head_bwd_dw_kernel<bf16>, dim3(hyb_cdiv(D, 64), yb + xb), dim3(256), 0, st, (const bf16*)x, dlogits, dW, db, B, S, D, C, W, (bf16*)dx, yb);
        HYB_LAUNCH_CHECK();
    }
    return 0;
}

// The loss by itself (ce_*_kernel; include/hybrid_hip.h states every definition).  hyb_loss_ok: what every entry point that carries a loss asks
// of it beyond its own non-null pointers.  hyb_ce_opts_ok: the options' ranges.  An exponent is 0 or >= 1: between, the derivative of
// base^g is singular at base == 0, which clipped negatives reach exactly.
int hyb_ce_opts_ok(const HybCeOpts& o) {
    return (o.has_ignore == 0 || o.has_ignore == 1) && o.label_smoothing >= 0.f && o.label_smoothing <= 1.f;
}
static int ce_gamma_ok(float g) { return g == 0.f || (g >= 1.f && g <= 3.0e38f); }
int hyb_loss_ok(const HybLoss& l) {
    if (hyb_loss_is_dense(l.mode) ? !l.d.target : !l.target) return 0;
    const float ls = l.o.label_smoothing;
    switch (l.mode) {
    case HYB_LOSS_PLAIN: return 1;
    case HYB_LOSS_OPTS: return hyb_ce_opts_ok(l.o);
    case HYB_LOSS_MIX: return l.m.target_b && l.m.lam && hyb_ce_opts_ok(l.o);
    case HYB_LOSS_SOFT: return l.d.kind == 0 && !l.d.pos_weight && ls >= 0.f && ls <= 1.f;
    case HYB_LOSS_BCE: return l.d.kind == 1 && ls == 0.f;
    case HYB_LOSS_FOCAL: return ls == 0.f && ce_gamma_ok(l.f.gamma) && l.f.gamma_neg == 0.f && l.f.clip == 0.f;
    case HYB_LOSS_ASYM: return l.d.kind == 1 && ls == 0.f && ce_gamma_ok(l.f.gamma) && ce_gamma_ok(l.f.gamma_neg) && l.f.clip >= 0.f && l.f.clip < 1.f;
    }
    return 0;
}
// forward: one workgroup; backward: a thread per clip
int hyb_loss_fwd(const HybLoss& l, const float* logits, float* loss, int B, int C, hipStream_t st) {
    HYB_CHECK_ARG(logits && loss && B > 0 && C > 0 && hyb_loss_ok(l));
    const dim3 grid(1), block(256);
    switch (l.mode) {
    case HYB_LOSS_PLAIN: hipLaunchKernelGGL(ce_fwd_kernel, grid, block, 0, st, logits, l.target, loss, B, C); break;
    case HYB_LOSS_OPTS: hipLaunchKernelGGL(ce_opts_fwd_kernel, grid, block, 0, st, logits, l.target, loss, B, C, l.o); break;
    case HYB_LOSS_MIX: hipLaunchKernelGGL(ce_mix_fwd_kernel, grid, block, 0, st, logits, l.target, loss, B, C, l.o, l.m); break;
    case HYB_LOSS_SOFT:
    case HYB_LOSS_BCE: hipLaunchKernelGGL(ce_dense_fwd_kernel, grid, block, 0, st, logits, loss, B, C, l.o, l.d); break;
    case HYB_LOSS_FOCAL: hipLaunchKernelGGL(ce_focal_fwd_kernel, grid, block, 0, st, logits, l.target, loss, B, C, l.o, l.f); break;
    case HYB_LOSS_ASYM: hipLaunchKernelGGL(ce_asym_fwd_kernel, grid, block, 0, st, logits, loss, B, C, l.o, l.d, l.f); break;
    }
    HYB_LAUNCH_CHECK();
    return 0;
}
int hyb_loss_bwd(const HybLoss& l, const float* logits, const float* dloss, float* dlogits, int B, int C, hipStream_t st) {
    HYB_CHECK_ARG(logits && dloss && dlogits && B > 0 && C > 0 && hyb_loss_ok(l));
    const dim3 grid(hyb_cdiv(B, 256)), block(256);
    switch (l.mode) {
    case HYB_LOSS_PLAIN: hipLaunchKernelGGL(ce_bwd_kernel, dim3(hyb_cdiv(B, 64)), dim3(64), 0, st, logits, l.target, dloss, dlogits, B, C); break;
    case HYB_LOSS_OPTS: hipLaunchKernelGGL(ce_opts_bwd_kernel, grid, block, 0, st, logits, l.target, dloss, dlogits, B, C, l.o); break;
    case HYB_LOSS_MIX: hipLaunchKernelGGL(ce_mix_bwd_kernel, grid, block, 0, st, logits, l.target, dloss, dlogits, B, C, l.o, l.m); break;
    case HYB_LOSS_SOFT:
    case HYB_LOSS_BCE: hipLaunchKernelGGL(ce_dense_bwd_kernel, grid, block, 0, st, logits, dloss, dlogits, B, C, l.o, l.d); break;
    case HYB_LOSS_FOCAL: hipLaunchKernelGGL(ce_focal_bwd_kernel, grid, block, 0, st, logits, l.target, dloss, dlogits, B, C, l.o, l.f); break;
    case HYB_LOSS_ASYM: hipLaunchKernelGGL(ce_asym_bwd_kernel, grid, block, 0, st, logits, dloss, dlogits, B, C, l.o, l.d, l.f); break;
    }
    HYB_LAUNCH_CHECK();
    return 0;
}

// The twelve entry points: each fills a HybLoss with its own arguments (hyb_internal.h) and runs the pair above.
extern "C" int hyb_cross_entropy_fwd(const float* logits, const long long* target, float* loss, int B, int C, void* stream) {
    return hyb_loss_fwd(hyb_loss_plain(target), logits, loss, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_bwd(const float* logits, const long long* target, const float* dloss, float* dlogits, int B, int C, void* stream) {
    return hyb_loss_bwd(hyb_loss_plain(target), logits, dloss, dlogits, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_opts_fwd(const float* logits, const long long* target, const float* weight, long long ignore_index, int has_ignore,
                                          float label_smoothing, float* loss, int B, int C, void* stream) {
    return hyb_loss_fwd(hyb_loss_opts(target, weight, ignore_index, has_ignore, label_smoothing), logits, loss, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_opts_bwd(const float* logits, const long long* target, const float* weight, long long ignore_index, int has_ignore,
                                          float label_smoothing, const float* dloss, float* dlogits, int B, int C, void* stream) {
    return hyb_loss_bwd(hyb_loss_opts(target, weight, ignore_index, has_ignore, label_smoothing), logits, dloss, dlogits, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_mix_fwd(const float* logits, const long long* target, const long long* target_b, const float* lam, const float* weight,
                                         long long ignore_index, int has_ignore, float label_smoothing, float* loss, int B, int C, void* stream) {
    return hyb_loss_fwd(hyb_loss_mix(target, target_b, lam, weight, ignore_index, has_ignore, label_smoothing), logits, loss, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_mix_bwd(const float* logits, const long long* target, const long long* target_b, const float* lam, const float* weight,
                                         long long ignore_index, int has_ignore, float label_smoothing, const float* dloss, float* dlogits, int B, int C,
                                         void* stream) {
    return hyb_loss_bwd(hyb_loss_mix(target, target_b, lam, weight, ignore_index, has_ignore, label_smoothing), logits, dloss, dlogits, B, C,
                        (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_dense_fwd(const float* logits, const float* target, const float* weight, const float* pos_weight, int kind,
                                           float label_smoothing, float* loss, int B, int C, void* stream) {
    return hyb_loss_fwd(hyb_loss_dense(target, weight, pos_weight, kind, label_smoothing), logits, loss, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_dense_bwd(const float* logits, const float* target, const float* weight, const float* pos_weight, int kind,
                                           float label_smoothing, const float* dloss, float* dlogits, int B, int C, void* stream) {
    return hyb_loss_bwd(hyb_loss_dense(target, weight, pos_weight, kind, label_smoothing), logits, dloss, dlogits, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_focal_fwd(const float* logits, const long long* target, const float* weight, long long ignore_index, int has_ignore,
                                           float gamma, float* loss, int B, int C, void* stream) {
    return hyb_loss_fwd(hyb_loss_focal(target, weight, ignore_index, has_ignore, gamma), logits, loss, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_focal_bwd(const float* logits, const long long* target, const float* weight, long long ignore_index, int has_ignore,
                                           float gamma, const float* dloss, float* dlogits, int B, int C, void* stream) {
    return hyb_loss_bwd(hyb_loss_focal(target, weight, ignore_index, has_ignore, gamma), logits, dloss, dlogits, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_asym_fwd(const float* logits, const float* target, const float* weight, const float* pos_weight, float gamma_pos,
                                          float gamma_neg, float clip, float* loss, int B, int C, void* stream) {
    return hyb_loss_fwd(hyb_loss_asym(target, weight, pos_weight, gamma_pos, gamma_neg, clip), logits, loss, B, C, (hipStream_t)stream);
}
extern "C" int hyb_cross_entropy_asym_bwd(const float* logits, const float* target, const float* weight, const float* pos_weight, float gamma_pos,
                                          float gamma_neg, float clip, const float* dloss, float* dlogits, int B, int C, void* stream) {
    return hyb_loss_bwd(hyb_loss_asym(target, weight, pos_weight, gamma_pos, gamma_neg, clip), logits, dloss, dlogits, B, C, (hipStream_t)stream);
}

// The classification meter's update (eval_metrics_kernel<mode>): one launch of one workgroup that ADDS into sums / counts / confusion.  The
// three entry points describe their criterion as a HybLoss (hyb_internal.h) and meet here: one set of checks, hyb_loss_ok included, one launch.
static int eval_metrics_launch(const HybLoss& l, const float* logits, int topk, int views, double* sums, long long* counts, long long* confusion,
                               long long* pred, float* scores, int B, int C, void* stream) {
    HYB_CHECK_ARG(logits && sums && counts && B >= 1 && C >= 1 && views >= 1 && topk >= 1 && topk <= C && hyb_ce_opts_ok(l.o) && hyb_loss_ok(l));
    HYB_CHECK_ARG(views == 1 || scores);
    HYB_CHECK_ARG((long long)B * views <= 0x7fffffffll);
    const HybEvalArgs a{logits, l.target, sums, counts, confusion, pred, scores, B, C, views, topk};
    switch (l.mode) {
    case HYB_LOSS_OPTS: hipLaunchKernelGGL(eval_metrics_kernel<HYB_LOSS_OPTS>, dim3(1), dim3(256), 0, (hipStream_t)stream, a, l); break;
    case HYB_LOSS_FOCAL: hipLaunchKernelGGL(eval_metrics_kernel<HYB_LOSS_FOCAL>, dim3(1), dim3(256), 0, (hipStream_t)stream, a, l); break;
    case HYB_LOSS_SOFT: hipLaunchKernelGGL(eval_metrics_kernel<HYB_LOSS_SOFT>, dim3(1), dim3(256), 0, (hipStream_t)stream, a, l); break;
    default: return HYB_E_ARG;
    }
    HYB_LAUNCH_CHECK();
    return 0;
}
extern "C" int hyb_eval_metrics(const float* logits, const long long* target, const float* weight, long long ignore_index, int has_ignore,
                                float label_smoothing, int topk, int views, double* sums, long long* counts, long long* confusion,
                                long long* pred, float* scores, int B, int C, void* stream) {
    return eval_metrics_launch(hyb_loss_opts(target, weight, ignore_index, has_ignore, label_smoothing), logits, topk, views, sums, counts, confusion,
                               pred, scores, B, C, stream);
}
extern "C" int hyb_eval_metrics_focal(const float* logits, const long long* target, const float* weight, long long ignore_index, int has_ignore,
                                      float gamma, int topk, int views, double* sums, long long* counts, long long* confusion, long long* pred,
                                      float* scores, int B, int C, void* stream) {
    return eval_metrics_launch(hyb_loss_focal(target, weight, ignore_index, has_ignore, gamma), logits, topk, views, sums, counts, confusion, pred,
                               scores, B, C, stream);
}
extern "C" int hyb_eval_metrics_soft(const float* logits, const float* target, const float* weight, float label_smoothing, int topk, int views,
                                     double* sums, long long* counts, long long* confusion, long long* pred, float* scores, int B, int C,
                                     void* stream) {
    return eval_metrics_launch(hyb_loss_dense(target, weight, nullptr, 0, label_smoothing), logits, topk, views, sums, counts, confusion, pred, scores,
                               B, C, stream);
}

// The multi-label meter's update (eval_multilabel_kernel<mode>): one launch of one workgroup that ADDS into sums / counts / cells and appends
// to the bank.  Both entry points describe their criterion as a HybLoss and meet here.
static int eval_multilabel_launch(const HybLoss& l, const float* logits, const float* threshold, int views, double* sums, long long* counts,
                                  long long* cells, float* bank_scores, unsigned char* bank_labels, long long capacity, unsigned char* pred,
                                  float* scores, int B, int C, void* stream) {
    HYB_CHECK_ARG(logits && threshold && sums && counts && cells && scores && B >= 1 && C >= 1 && views >= 1 && capacity >= 0 && hyb_loss_ok(l));
    HYB_CHECK_ARG((bank_scores != nullptr) == (bank_labels != nullptr) && (!bank_scores || capacity > 0));
    HYB_CHECK_ARG((long long)B * views <= 0x7fffffffll && (long long)views * C <= 0x7fffffffll);
    const HybEvalMlArgs a{logits, l.d.target, l.o.weight, l.d.pos_weight, threshold, sums, counts, cells, bank_scores, bank_labels, capacity, pred,
                          scores, B, C, views};
    switch (l.mode) {
    case HYB_LOSS_BCE: hipLaunchKernelGGL(eval_multilabel_kernel<HYB_LOSS_BCE>, dim3(1), dim3(256), 0, (hipStream_t)stream, a, l.f); break;
    case HYB_LOSS_ASYM: hipLaunchKernelGGL(eval_multilabel_kernel<HYB_LOSS_ASYM>, dim3(1), dim3(256), 0, (hipStream_t)stream, a, l.f); break;
    default: return HYB_E_ARG;
    }
    HYB_LAUNCH_CHECK();
    return 0;
}
extern "C" int hyb_eval_multilabel(const float* logits, const float* target, const float* weight, const float* pos_weight, const float* threshold,
                                   int views, double* sums, long long* counts, long long* cells, float* bank_scores,
                                   unsigned char* bank_labels, long long capacity, unsigned char* pred, float* scores, int B, int C,
                                   void* stream) {
    return eval_multilabel_launch(hyb_loss_dense(target, weight, pos_weight, 1, 0.f), logits, threshold, views, sums, counts, cells, bank_scores,
                                  bank_labels, capacity, pred, scores, B, C, stream);
}
extern "C" int hyb_eval_multilabel_asym(const float* logits, const float* target, const float* weight, const float* pos_weight, float gamma_pos,
                                        float gamma_neg, float clip, const float* threshold, int views, double* sums, long long* counts,
                                        long long* cells, float* bank_scores, unsigned char* bank_labels, long long capacity,
                                        unsigned char* pred, float* scores, int B, int C, void* stream) {
    return eval_multilabel_launch(hyb_loss_asym(target, weight, pos_weight, gamma_pos, gamma_neg, clip), logits, threshold, views, sums, counts, cells,
                                  bank_scores, bank_labels, capacity, pred, scores, B, C, stream);
}
