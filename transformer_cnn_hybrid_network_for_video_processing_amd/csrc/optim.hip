// AdamW step over all parameter tensors of the model in ONE launch (the step right after the hot path;
// the reference's optimizer is torch.optim.AdamW, Model.py:153 / FCT.py:305).  Same update as torch.optim.AdamW
// (decoupled weight decay, bias correction, amsgrad = False, maximize = False):
//     p <- p * (1 - lr*wd);  m <- m + (1-b1)(g - m);  v <- b2*v + (1-b2) g^2;
//     p <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The tensor table travels in the kernel arguments (up to 80 tensors per launch), a workgroup owns 4096 consecutive elements
// of one tensor and finds it by scanning the table's chunk offsets; HBM-bound: 7 x 4 bytes per parameter (9 x 4 in the variant that also keeps
// an exponential moving average of the weights, hyb_adamw_step_dev_ema: 64 tensors per launch).
// Gradient accumulation over k micro-batches: hyb_grad_accumulate (acc += g, 3 x 4 bytes per parameter) ends micro-batches 1 .. k - 1,
// hyb_adamw_step_dev_acc ends the k-th: it steps on (acc + g) / k and leaves acc zeroed (9 x 4 bytes, 11 x 4 with the average) -- no
// separate sum, scale or memset pass.
// The non-finite guard: hyb_grad_norm_guard / hyb_grad_norm_acc_guard also decide, on the device, whether the step is skipped (the norm is not
// finite), and hyb_adamw_step_dev_guard reads the decision: a skipped step stores nothing to the model.
// Parameter groups: hyb_adamw_step_dev_groups serves the tensors of ALL groups from one launch -- the table carries one byte per tensor, its
// group, and thread 0 of a workgroup forms its scalars from that group's row of the device blocks hyper[groups, 6] / ema_hyper[groups, 2];
// hyb_adamw_hyper_set_groups writes the rows of several groups in one launch.
// LAMB: hyb_lamb_trust forms every tensor's trust ratio r = |p| / |u| on the device (a read-only chunk pass and a one-workgroup-per-tensor
// final launch, 4 x 4 bytes read per parameter), hyb_lamb_step_dev is the AdamW launch at the rate r * lr per tensor (LAMB, below).
// SGD: hyb_sgd_step_dev is torch.optim.SGD's rule (momentum, dampening, Nesterov, coupled weight decay) in a launch of the same shape with one
// state tensor, 5 x 4 bytes per parameter; hyb_lars_trust forms LARS's layer-wise ratios for it (SGD with momentum, and LARS, below).
#include <algorithm>
#include <type_traits>

#include "hyb_common.h"
#include "hyb_internal.h"

namespace {

constexpr int ADAM_MAX = 80, ADAM_CHUNK = 4096;

struct AdamTensor { float* p; const float* g; float* m; float* v; long long n; };
struct AdamArgs {
    AdamTensor t[ADAM_MAX];
    int chunk_begin[ADAM_MAX + 1];
    int count;
    float decay, omb1, beta2, omb2, eps, step_size, inv_sqrt_bc2;      // omb = 1 - beta, formed in double on the host like torch does
    // device-side step counter (hipGraph replays): when step_inc != NULL the bias corrections are formed on the device, in double,
    // from step + *step_inc
    const long long* step_inc;
    long long* advance;          // NULL, or = step_inc: the last workgroup to finish adds 1 to it (every workgroup has read it by then)
    unsigned int* ticket;        // the caller's ticket word of THIS counter (zero at rest): workgroups finished in the running launch
    long long step;
    double lr, beta1d, beta2d;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a, float step_size, float inv_sqrt_bc2) {
    p *= a.decay;
    m = m + a.omb1 * (g - m);
    v = a.beta2 * v + a.omb2 * g * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + a.eps;
    p -= step_size * (m / denom);
}

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
    __shared__ float s_corr[2];
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if ((int)blockIdx.x >= a.chunk_begin[i]) ti = i;
    const AdamTensor t = a.t[ti];
    const long long base = (long long)(blockIdx.x - a.chunk_begin[ti]) * ADAM_CHUNK;
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0);
    constexpr int NK = ADAM_CHUNK / (256 * 4);
    // a full, aligned chunk (all but each tensor's last): its 16 loads are issued BEFORE the bias corrections are formed (two double-
    // precision pow() on one thread, ~2 us) -- the kernel used to start every workgroup with that, then run four load -> store rounds
    const bool full = vec && base + ADAM_CHUNK <= t.n;
    f32x4 p[NK], m[NK], v[NK], g[NK];
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            p[k] = *reinterpret_cast<const f32x4*>(t.p + i); m[k] = *reinterpret_cast<const f32x4*>(t.m + i);
            v[k] = *reinterpret_cast<const f32x4*>(t.v + i); g[k] = *reinterpret_cast<const f32x4*>(t.g + i);
        }
    }
    float step_size = a.step_size, inv_sqrt_bc2 = a.inv_sqrt_bc2;
    if (a.step_inc) {                                          // uniform branch: every thread reaches the barrier
        if (threadIdx.x == 0) {
            const double tt = (double)(a.step + *a.step_inc);
            s_corr[0] = (float)(a.lr / (1.0 - pow(a.beta1d, tt)));
            s_corr[1] = (float)(1.0 / sqrt(1.0 - pow(a.beta2d, tt)));
        }
        __syncthreads();
        step_size = s_corr[0]; inv_sqrt_bc2 = s_corr[1];
    }
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) { float pj = p[k][j], mj = m[k][j], vj = v[k][j]; adam_one(pj, g[k][j], mj, vj, a, step_size, inv_sqrt_bc2); p[k][j] = pj; m[k][j] = mj; v[k][j] = vj; }
            *reinterpret_cast<f32x4*>(t.p + i) = p[k]; *reinterpret_cast<f32x4*>(t.m + i) = m[k]; *reinterpret_cast<f32x4*>(t.v + i) = v[k];
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            if (i >= t.n) break;
            if (vec && i + 4 <= t.n) {
                f32x4 pp = *reinterpret_cast<f32x4*>(t.p + i), mm = *reinterpret_cast<f32x4*>(t.m + i), vv = *reinterpret_cast<f32x4*>(t.v + i);
                const f32x4 gg = *reinterpret_cast<const f32x4*>(t.g + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) { float pj = pp[j], mj = mm[j], vj = vv[j]; adam_one(pj, gg[j], mj, vj, a, step_size, inv_sqrt_bc2); pp[j] = pj; mm[j] = mj; vv[j] = vj; }
                *reinterpret_cast<f32x4*>(t.p + i) = pp; *reinterpret_cast<f32x4*>(t.m + i) = mm; *reinterpret_cast<f32x4*>(t.v + i) = vv;
            } else {
                for (long long e = i; e < i + 4 && e < t.n; ++e) adam_one(t.p[e], t.g[e], t.m[e], t.v[e], a, step_size, inv_sqrt_bc2);
            }
        }
    }
    // Thread 0 consumed the counter's value before the barrier at the top, so its read is complete here; the ticket only orders "every
    // workgroup has read" before the one write, which needs no fence (a release fence per workgroup costs an L2 write-back each: measured
    // 38 -> 126 us for this kernel).  The relaxed atomic is performed at the L2, in order per address.
    if (a.advance && threadIdx.x == 0) {
        if (__hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *a.advance += 1;
        }
    }
}

// ---- hyper-parameters on the device (hyb_adamw_hyper_set / hyb_grad_norm / hyb_adamw_step_dev) ------------------------------------------
// A captured launch freezes its by-value arguments, so a learning-rate schedule under hipGraph replay needs the hyper-parameters in device
// memory: double hyper[6] = {lr, beta1, beta2, eps, weight_decay, max_grad_norm}, rewritten between replays by the one-workgroup kernel below
// (the values travel as ITS kernel arguments: no staging buffer to reuse too early, nothing for the host to wait on).
constexpr int HYPER_N = 6;
struct HyperVals { double v[HYPER_N]; };

__global__ __launch_bounds__(64) void hyper_set_kernel(double* hyper, HyperVals h) {
    double x = h.v[0];                                             // (selects, not an indexed read: the arguments stay in registers)
#pragma unroll
    for (int i = 1; i < HYPER_N; ++i) x = (int)threadIdx.x == i ? h.v[i] : x;
    if (threadIdx.x < HYPER_N) hyper[threadIdx.x] = x;
}

// Global L2 norm of all gradient tensors + torch's clip coefficient, bit-reproducible: no floating-point atomics, every order fixed.
//   grad_norm_kernel, one workgroup per 4096-element chunk: a thread squares-and-adds its 16 elements in index order (fmaf; the same
//   element -> thread -> order mapping as adamw_kernel whether the tensor is 16-byte aligned or not), wave_sum, the four wave totals pairwise
//   in index order -> partials[chunk];
//   grad_norm_final_kernel, ONE workgroup in a launch of its own: partials[0 .. total) in double -- thread t takes t, t + 256, ... ascending,
//   thread 0 adds the 256 thread sums in ascending order -- then the norm and the coefficient.
// The second launch IS the cross-workgroup hand-off.  The in-launch form (partial store, release fetch_add on a ticket at agent scope, acquire
// fence and final sum in the workgroup that finishes last) was built and measured first: 38.6 us per call against 11.7 us for these two launches
// on the model's 27.3 MB of gradients (scripts/micro/grad_norm_handoff.hip) -- every workgroup's release is an L2 write-back, the cost adamw_kernel's
// note below its ticket records too -- so it costs far more than the 4.6 us of one dependent launch and was dropped.
struct GradNormArgs {
    const float* g[ADAM_MAX];
    long long n[ADAM_MAX];
    int chunk_begin[ADAM_MAX + 1];
    int count;
    int chunk_offset;                     // index of this launch's first chunk among all chunks of the call (more than 80 tensors = several launches)
    float* partials;
};
// hyb_grad_norm_acc: the norm of the effective gradient of an accumulated step, G = (acc + g) * inv_k (g[] all NULL: G = acc * inv_k)
struct GradNormAccArgs : GradNormArgs {
    const float* acc[ADAM_MAX];
    float inv_k;
};
static_assert(sizeof(GradNormAccArgs) <= 4096, "the tensor table travels in the kernel arguments");

// Which gradient a launch works on.  GRAD_PLAIN: g.  GRAD_ACC_G: G = (acc + g) * inv_k, the sum rounded, then the product rounded (no
// contraction; inv_k == 1.0f for k == 1).  GRAD_ACC: G = acc * inv_k (data parallelism: acc is the all-reduced bucket, there is no g).
// (named constants of type int, not an unnamed enum: a kernel's template arguments are part of its mangled name, and the host and device
// passes number unnamed types differently, so the launch would not find the kernel)
constexpr int GRAD_PLAIN = 0, GRAD_ACC_G = 1, GRAD_ACC = 2;
template <int MODE> __device__ __forceinline__ float eff_grad(float acc, float g, float inv_k) {
#pragma clang fp contract(off)
    if constexpr (MODE == GRAD_PLAIN) return g;
    else if constexpr (MODE == GRAD_ACC) return acc * inv_k;
    else { const float sum = acc + g; return sum * inv_k; }
}

// one chunk's sum of squares; every thread of the workgroup must call it, thread 0 gets the result
template <int MODE = GRAD_PLAIN, typename Args = GradNormArgs> __device__ __forceinline__ float grad_chunk_sumsq(const Args& a, float* s_wave /* [4] */) {
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if ((int)blockIdx.x >= a.chunk_begin[i]) ti = i;
    const float* __restrict__ g = a.g[ti];
    const long long n = a.n[ti];
    const long long base = (long long)(blockIdx.x - a.chunk_begin[ti]) * ADAM_CHUNK;
    constexpr int NK = ADAM_CHUNK / (256 * 4);
    float s = 0.f;
    if constexpr (MODE == GRAD_PLAIN) {
        if ((((uintptr_t)g & 15) == 0) && base + ADAM_CHUNK <= n) {
            f32x4 v[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) v[k] = *reinterpret_cast<const f32x4*>(g + base + ((long long)k * 256 + threadIdx.x) * 4);
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_fmaf(v[k][j], v[k][j], s);
        } else {
#pragma unroll 1
            for (int k = 0; k < NK; ++k) {
                const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
                for (long long e = i; e < i + 4 && e < n; ++e) s = __builtin_fmaf(g[e], g[e], s);
            }
        }
    } else {                                                      // the same elements in the same order, each formed by eff_grad first
        constexpr bool HAS_G = MODE != GRAD_ACC;
        const float* __restrict__ acc = a.acc[ti];
        const float inv_k = a.inv_k;
        if (((((uintptr_t)g | (uintptr_t)acc) & 15) == 0) && base + ADAM_CHUNK <= n) {
            f32x4 v[HAS_G ? NK : 1], w[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
                if constexpr (HAS_G) v[k] = *reinterpret_cast<const f32x4*>(g + i);
                w[k] = *reinterpret_cast<const f32x4*>(acc + i);
            }
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = eff_grad<MODE>(w[k][j], HAS_G ? v[k][j] : 0.f, inv_k);
                    s = __builtin_fmaf(x, x, s);
                }
        } else {
#pragma unroll 1
            for (int k = 0; k < NK; ++k) {
                const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
                for (long long e = i; e < i + 4 && e < n; ++e) {
                    const float x = eff_grad<MODE>(acc[e], HAS_G ? g[e] : 0.f, inv_k);
                    s = __builtin_fmaf(x, x, s);
                }
            }
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
    __syncthreads();
    return (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// partials[0 .. total) -> norm_out; every thread of the (one) workgroup must call it, thread 0 gets the norm back.  LOAD(i) reads partials[i].
template <typename Load> __device__ __forceinline__ float grad_norm_finish(Load load, int total, const double* hyper, float* norm_out, double* s_sum /* [256] */) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < total; i += 8 * 256) {          // eight loads in flight (one workgroup: pure latency), added in index order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i + j * 256 < total ? load(i + j * 256) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (double)v[j];
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    float norm = 0.f;
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int i = 0; i < 256; ++i) sum += s_sum[i];
        norm = (float)sqrt(sum);
        const double mx = hyper[5];
        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1); a NaN norm stays a NaN coefficient
        double coef = 1.0;
        if (mx > 0.0 && mx < (double)INFINITY) { coef = mx / ((double)norm + 1e-6); coef = coef > 1.0 ? 1.0 : coef; }
        norm_out[0] = norm;
        norm_out[1] = (float)coef;
    }
    return norm;
}

__global__ __launch_bounds__(256) void grad_norm_kernel(GradNormArgs a) {
    __shared__ float s_wave[4];
    const float s = grad_chunk_sumsq(a, s_wave);
    if (threadIdx.x == 0) a.partials[a.chunk_offset + blockIdx.x] = s;
}

template <int MODE> __global__ __launch_bounds__(256) void grad_norm_acc_kernel(GradNormAccArgs a) {
    __shared__ float s_wave[4];
    const float s = grad_chunk_sumsq<MODE>(a, s_wave);
    if (threadIdx.x == 0) a.partials[a.chunk_offset + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_norm_final_kernel(const float* partials, int total, const double* hyper, float* norm_out) {
    __shared__ double s_sum[256];
    grad_norm_finish([partials](int i) { return partials[i]; }, total, hyper, norm_out, s_sum);
}

// ---- the non-finite guard (hyb_grad_norm_guard / hyb_grad_norm_acc_guard / hyb_adamw_step_dev_guard) -------------------------------------
// A step whose global gradient norm is not finite (a NaN or an infinite element, or finite elements whose sum of squares overflows fp32)
// must leave the model as it was: the host never looks at the gradients, and a captured launch cannot be left out, so the decision is taken
// here.  long long guard[2] = {skip_now, skipped_total}, device memory owned by the caller and zero before the first step.  The final norm
// launch -- one workgroup, once per optimizer step however many parameter groups follow -- is the only writer: the same sum, the same
// norm_out, then skip_now = !isfinite(norm) and skipped_total += skip_now, plain stores from thread 0 like norm_out's.  Every AdamW launch
// of the step reads both words (adamw_dev_kernel, GUARD).
__global__ __launch_bounds__(256) void grad_norm_final_guard_kernel(const float* partials, int total, const double* hyper, float* norm_out,
                                                                    long long* guard) {
    __shared__ double s_sum[256];
    const float norm = grad_norm_finish([partials](int i) { return partials[i]; }, total, hyper, norm_out, s_sum);
    if (threadIdx.x == 0) {
        const long long skip = (__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u ? 1ll : 0ll;      // exponent all ones: inf or NaN
        guard[0] = skip;
        guard[1] += skip;
    }
}

// adamw_kernel with every scalar formed on the device: from hyper[] and step + *step_inc by thread 0, in double, rounded once -- the same
// expressions, in the same precision, as hyb_adamw_step forms on the host (and as adamw_kernel's own step_inc branch).  clip: NULL, or the
// norm_out of grad_norm_kernel: every gradient element is multiplied by clip[1] first (g * 1.0f is exact: an unclipped step is the plain step).
struct AdamScalars { float decay, omb1, beta2, omb2, eps, step_size, inv_sqrt_bc2, clip; };
template <int N> struct AdamDevTable {
    AdamTensor t[N];
    int chunk_begin[N + 1];
    int count;
    const double* hyper;
    const long long* step_inc;
    long long* advance;
    unsigned int* ticket;
    long long step;
    const float* clip;
};
using AdamDevArgs = AdamDevTable<ADAM_MAX>;
// The same launch keeping an exponential moving average of the weights (hyb_adamw_step_dev_ema): a sixth pointer per tensor.  80 entries
// of 48 bytes would not fit the 4 KB of kernel arguments, so this variant's table holds 64.
constexpr int ADAM_EMA_MAX = 64;
struct AdamEmaArgs : AdamDevTable<ADAM_EMA_MAX> {
    float* e[ADAM_EMA_MAX];
    const double* ema_hyper;     // device double [2] = {decay, warmup (0 or 1)}, written by hyb_adamw_ema_set
};
// The accumulated step (hyb_adamw_step_dev_acc): one more pointer per tensor, the accumulator, and k.  76 entries without the average, 64 with.
constexpr int ADAM_ACC_MAX = 76, ADAM_EMA_ACC_MAX = 64;
struct AdamAccArgs : AdamDevTable<ADAM_ACC_MAX> {
    float* acc[ADAM_ACC_MAX];
    long long k;                 // micro-batches per optimizer step; the step number is step + *step_inc / k (the counter counts micro-steps)
    float inv_k;                 // (float)(1.0 / (double)k)
};
struct AdamEmaAccArgs : AdamDevTable<ADAM_EMA_ACC_MAX> {
    float* e[ADAM_EMA_ACC_MAX];
    const double* ema_hyper;
    float* acc[ADAM_EMA_ACC_MAX];
    long long k;
    float inv_k;
};
static_assert(sizeof(AdamArgs) <= 4096 && sizeof(AdamDevArgs) <= 4096 && sizeof(AdamEmaArgs) <= 4096 && sizeof(AdamAccArgs) <= 4096 &&
              sizeof(AdamEmaAccArgs) <= 4096, "the tensor table travels in the kernel arguments");
// The guarded launches (hyb_adamw_step_dev_guard): the same tables with one more pointer, the guard block.  Types of their own -- the
// unguarded kernels' arguments stay as they are.
template <typename Base> struct AdamGuarded : Base { const long long* guard; };
static_assert(sizeof(AdamGuarded<AdamDevArgs>) <= 4096 && sizeof(AdamGuarded<AdamEmaArgs>) <= 4096 && sizeof(AdamGuarded<AdamAccArgs>) <= 4096 &&
              sizeof(AdamGuarded<AdamEmaAccArgs>) <= 4096, "the tensor table travels in the kernel arguments");
// The grouped launches (hyb_adamw_step_dev_groups): one byte per tensor, the index of its parameter group; hyper and ema_hyper are the BASES
// of the blocks double [groups, 6] and double [groups, 2], of which a workgroup reads the row of its tensor's group.  Types of their own
// again, with the members of the tables above under the same names (e / acc hold one unused entry in the variants without them; guard is
// read by the guarded instantiations only).  The accumulating table gives up four tensors for the bytes: 72, not 76.
constexpr int ADAM_GROUPS_MAX = 255;                               // group indices are bytes; 255 itself is not one
template <bool EMA, bool ACCUM> struct AdamGroupArgs : AdamDevTable<EMA ? 64 : ACCUM ? 72 : ADAM_MAX> {
    static constexpr int MAX = EMA ? 64 : ACCUM ? 72 : ADAM_MAX;
    unsigned char group[MAX];
    float* e[EMA ? MAX : 1];
    const double* ema_hyper;
    float* acc[ACCUM ? MAX : 1];
    long long k;
    float inv_k;
    const long long* guard;
};
static_assert(sizeof(AdamGroupArgs<false, false>) <= 4096 && sizeof(AdamGroupArgs<true, false>) <= 4096 && sizeof(AdamGroupArgs<false, true>) <= 4096 &&
              sizeof(AdamGroupArgs<true, true>) <= 4096, "the tensor table travels in the kernel arguments");

// adam_one with every fused multiply-add written out, so that the device path computes what adamw_kernel computes as the compiler contracts
// it (test_unclipped_equals_no_clipping: bit-equal to the plain launch).  adamw_kernel's 16-byte groups end in p = fma(p, decay, -(step * q)),
// its element-wise remainder -- which stores p * decay first -- in p = fma(-step, q, p * decay); VEC says which of the two this element takes.
template <bool VEC> __device__ __forceinline__ void adam_dev_one(float& p, float g, float& m, float& v, const AdamScalars& a) {
#pragma clang fp contract(off)
    g = g * a.clip;
    m = __builtin_fmaf(a.omb1, g - m, m);
    v = __builtin_fmaf(a.beta2, v, (a.omb2 * g) * g);
    const float q = m / __builtin_fmaf(sqrtf(v), a.inv_sqrt_bc2, a.eps);
    p = VEC ? __builtin_fmaf(p, a.decay, -(a.step_size * q)) : __builtin_fmaf(-a.step_size, q, p * a.decay);
}

// e <- d * e + (1 - d) * p_new: the product rounded, then one fused multiply-add (d == 0: e == p_new exactly, whatever e held)
__device__ __forceinline__ float adam_ema_one(float e, float p_new, float d32, float omd32) {
#pragma clang fp contract(off)
    return __builtin_fmaf(d32, e, omd32 * p_new);
}

// the step number: step + *step_inc; the accumulated step (ACCUM, a.k micro-steps per optimizer step): step + *step_inc / k.  skipped (the
// guarded launch: guard[1]) is the number of steps, among those that step and the counter count, that were attempted but not applied: bias
// correction and the average's warm-up go by the number of APPLIED updates.
template <bool ACCUM, typename Args> __device__ __forceinline__ long long adam_step_number(const Args& a, long long skipped) {
    if constexpr (ACCUM) return a.step + (a.step_inc ? *a.step_inc / a.k : 0ll) - skipped;
    else return a.step + (a.step_inc ? *a.step_inc : 0ll) - skipped;
}

// (hyper: the six values of the tensor's parameter group -- a.hyper itself, or in a grouped launch the group's row of the block)
// LAMB: the tensor's trust ratio r scales the rate -- decay and step_size are formed from r * lr, still in double and rounded once; every
// other instantiation reads hyper[0] as it always did (r is not looked at), and r == 1.0 gives AdamW's doubles.
template <bool ACCUM = false, bool LAMB = false, typename Args> __device__ __forceinline__ void adam_dev_scalars(const Args& a, const double* hyper, float* out /* [8] */, long long skipped = 0ll, double r = 1.0) {
#pragma clang fp contract(off)                                    // 1.0 - lr * wd: a product rounded, then a difference, as on the host (no fma)
    const double lr = LAMB ? r * hyper[0] : hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4];
    const double tt = (double)adam_step_number<ACCUM>(a, skipped);
    const double prod = lr * wd;
    out[0] = (float)(1.0 - prod);
    out[1] = (float)(1.0 - b1);
    out[2] = (float)b2;
    out[3] = (float)(1.0 - b2);
    out[4] = (float)eps;
    out[5] = (float)(lr / (1.0 - pow(b1, tt)));
    out[6] = (float)(1.0 / sqrt(1.0 - pow(b2, tt)));
    out[7] = a.clip ? a.clip[1] : 1.0f;
}

// the average's decay at step t = step + *step_inc (n = t - 1 updates so far): d = warmup ? min(decay, (1 + n) / (10 + n)) : decay, in double;
// d and 1 - d are rounded to fp32 once each
template <bool ACCUM = false, typename Args> __device__ __forceinline__ void adam_ema_scalars(const Args& a, const double* ema_hyper, float* out /* [2] */, long long skipped = 0ll) {
#pragma clang fp contract(off)
    const double decay = ema_hyper[0];
    const double n = (double)(adam_step_number<ACCUM>(a, skipped) - 1ll);
    double d = decay;
    if (ema_hyper[1] != 0.0) {
        const double w = (1.0 + n) / (10.0 + n);
        d = w < decay ? w : decay;
    }
    out[0] = (float)d;
    out[1] = (float)(1.0 - d);
}

template <bool EMA, int ACC> using AdamDevTableArgs =
    std::conditional_t<ACC != GRAD_PLAIN, std::conditional_t<EMA, AdamEmaAccArgs, AdamAccArgs>, std::conditional_t<EMA, AdamEmaArgs, AdamDevArgs>>;
template <bool EMA, int ACC, bool GUARD = false, bool GROUPS = false> using AdamwDevKernelArgs =
    std::conditional_t<GROUPS, AdamGroupArgs<EMA, ACC != GRAD_PLAIN>, std::conditional_t<GUARD, AdamGuarded<AdamDevTableArgs<EMA, ACC>>, AdamDevTableArgs<EMA, ACC>>>;
// The LAMB launches (hyb_lamb_step_dev): any of the tables above with the trust block of hyb_lamb_trust -- float [3] per tensor of the WHOLE
// call, {|p|, |u|, r} -- and the index of the slice's first tensor in it.  Types of their own once more: every table above stays as it is.
template <typename Base> struct AdamLamb : Base { const float* trust; int first; };
static_assert(sizeof(AdamLamb<AdamDevArgs>) <= 4096 && sizeof(AdamLamb<AdamEmaArgs>) <= 4096 && sizeof(AdamLamb<AdamAccArgs>) <= 4096 &&
              sizeof(AdamLamb<AdamEmaAccArgs>) <= 4096 && sizeof(AdamLamb<AdamGuarded<AdamDevArgs>>) <= 4096 && sizeof(AdamLamb<AdamGuarded<AdamEmaArgs>>) <= 4096 &&
              sizeof(AdamLamb<AdamGuarded<AdamAccArgs>>) <= 4096 && sizeof(AdamLamb<AdamGuarded<AdamEmaAccArgs>>) <= 4096 &&
              sizeof(AdamLamb<AdamGroupArgs<false, false>>) <= 4096 && sizeof(AdamLamb<AdamGroupArgs<true, false>>) <= 4096 &&
              sizeof(AdamLamb<AdamGroupArgs<false, true>>) <= 4096 && sizeof(AdamLamb<AdamGroupArgs<true, true>>) <= 4096,
              "the tensor table travels in the kernel arguments");
template <bool EMA, int ACC, bool GUARD = false, bool GROUPS = false, bool LAMB = false> using AdamDevKernelArgs =
    std::conditional_t<LAMB, AdamLamb<AdamwDevKernelArgs<EMA, ACC, GUARD, GROUPS>>, AdamwDevKernelArgs<EMA, ACC, GUARD, GROUPS>>;

// the counter's one read (thread 0, in front of the barrier) is complete in every workgroup that has taken a ticket: see adamw_kernel
template <typename Args> __device__ __forceinline__ void adam_dev_advance(const Args& a) {
    if (a.advance && threadIdx.x == 0) {
        if (__hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *a.advance += 1;
        }
    }
}

// EMA = false: hyb_adamw_step_dev, the launch as it always was.  EMA = true: hyb_adamw_step_dev_ema -- the same body, and where it holds a new
// parameter value in a register it also moves that parameter's average (2 x 4 more bytes per parameter, no second pass over the weights).
// ACC != GRAD_PLAIN: hyb_adamw_step_dev_acc -- the same body again on the effective gradient G of an accumulated step (eff_grad: the
// accumulator is one more 16-byte load per group, issued with the others), which also stores +0.0f over the accumulator it has read;
// GRAD_ACC: there is no g (t.g is NULL and never read).
// GUARD: hyb_adamw_step_dev_guard -- thread 0 reads guard[] = {skip_now, skipped_total} in the scalar phase.  skip_now: the workgroup forms
// no scalars and stores nothing to p / m / v / e (not even their old values); it stores +0.0f over the accumulators (ACCUM: the poison must
// not stay in them) and takes its ticket, so the counter -- which also seeds dropout -- advances as after an applied step.  Otherwise the
// same body with the step number less skipped_total.
// GROUPS: hyb_adamw_step_dev_groups -- the table holds the tensors of several parameter groups, and thread 0 reads the hyper-parameters from
// the row of ITS tensor's group (a.group[ti]) where the other launches read the one row they were given.  Nothing else differs: every
// element comes out as the launch over its group alone gives it.
// LAMB: hyb_lamb_step_dev -- thread 0 also reads its tensor's trust ratio r = trust[3 (first + ti) + 2], which hyb_lamb_trust has formed for
// this very step, and forms decay and step_size from r * lr (adam_dev_scalars): p - lr r u = p (1 - (r lr) wd) - (r lr / (1 - b1^t)) m' /
// (sqrt(v') / sqrt(1 - b2^t) + eps), so the element loop is AdamW's, and r == 1.0f gives AdamW's step bit for bit.  On a guarded skip the trust
// block is not read.
template <bool EMA, int ACC = GRAD_PLAIN, bool GUARD = false, bool GROUPS = false, bool LAMB = false> __global__ __launch_bounds__(256)
void adamw_dev_kernel(AdamDevKernelArgs<EMA, ACC, GUARD, GROUPS, LAMB> a) {
    constexpr bool ACCUM = ACC != GRAD_PLAIN, HAS_G = ACC != GRAD_ACC;
    __shared__ float s_sc[EMA ? 10 : 8];
    __shared__ int s_skip;
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if ((int)blockIdx.x >= a.chunk_begin[i]) ti = i;
    const AdamTensor t = a.t[ti];
    float* te = nullptr;
    if constexpr (EMA) te = a.e[ti];
    float* ta = nullptr;
    float inv_k = 1.f;
    if constexpr (ACCUM) { ta = a.acc[ti]; inv_k = a.inv_k; }
    const long long base = (long long)(blockIdx.x - a.chunk_begin[ti]) * ADAM_CHUNK;
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v | (uintptr_t)te | (uintptr_t)ta) & 15) == 0);
    constexpr int NK = ADAM_CHUNK / (256 * 4);
    const bool full = vec && base + ADAM_CHUNK <= t.n;            // as in adamw_kernel: a full chunk's 16 loads go out before the scalar work
    f32x4 p[NK], m[NK], v[NK], g[HAS_G ? NK : 1], ea[EMA ? NK : 1], ac[ACCUM ? NK : 1];
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            p[k] = *reinterpret_cast<const f32x4*>(t.p + i); m[k] = *reinterpret_cast<const f32x4*>(t.m + i);
            v[k] = *reinterpret_cast<const f32x4*>(t.v + i);
            if constexpr (HAS_G) g[k] = *reinterpret_cast<const f32x4*>(t.g + i);
            if constexpr (EMA) ea[k] = *reinterpret_cast<const f32x4*>(te + i);
            if constexpr (ACCUM) ac[k] = *reinterpret_cast<const f32x4*>(ta + i);
        }
    }
    if (threadIdx.x == 0) {
        long long skipped = 0ll;
        bool skip = false;
        if constexpr (GUARD) { skip = a.guard[0] != 0ll; skipped = a.guard[1]; s_skip = skip ? 1 : 0; }
        if (!skip) {
            const double* hyper = a.hyper;
            if constexpr (GROUPS) hyper += HYPER_N * (int)a.group[ti];
            if constexpr (LAMB) adam_dev_scalars<ACCUM, true>(a, hyper, s_sc, skipped, (double)a.trust[3ll * (a.first + ti) + 2]);
            else adam_dev_scalars<ACCUM>(a, hyper, s_sc, skipped);
            if constexpr (EMA) {
                const double* ema_hyper = a.ema_hyper;
                if constexpr (GROUPS) ema_hyper += 2 * (int)a.group[ti];
                adam_ema_scalars<ACCUM>(a, ema_hyper, s_sc + 8, skipped);
            }
        }
    }
    __syncthreads();
    if constexpr (GUARD) {
        if (s_skip) {                                              // uniform over the workgroup (and over the launch)
            if constexpr (ACCUM) {
#pragma unroll 1
                for (int k = 0; k < NK; ++k) {
                    const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
                    if (i >= t.n) break;
                    if (vec && i + 4 <= t.n) *reinterpret_cast<f32x4*>(ta + i) = f32x4{0.f, 0.f, 0.f, 0.f};
                    else for (long long e = i; e < i + 4 && e < t.n; ++e) ta[e] = 0.f;
                }
            }
            adam_dev_advance(a);
            return;
        }
    }
    const AdamScalars sc{s_sc[0], s_sc[1], s_sc[2], s_sc[3], s_sc[4], s_sc[5], s_sc[6], s_sc[7]};
    float d32 = 0.f, omd32 = 0.f;
    if constexpr (EMA) { d32 = s_sc[8]; omd32 = s_sc[9]; }
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = p[k][j], mj = m[k][j], vj = v[k][j];
                adam_dev_one<true>(pj, eff_grad<ACC>(ACCUM ? ac[k][j] : 0.f, HAS_G ? g[k][j] : 0.f, inv_k), mj, vj, sc);
                p[k][j] = pj; m[k][j] = mj; v[k][j] = vj;
                if constexpr (EMA) ea[k][j] = adam_ema_one(ea[k][j], pj, d32, omd32);
            }
            *reinterpret_cast<f32x4*>(t.p + i) = p[k]; *reinterpret_cast<f32x4*>(t.m + i) = m[k]; *reinterpret_cast<f32x4*>(t.v + i) = v[k];
            if constexpr (EMA) *reinterpret_cast<f32x4*>(te + i) = ea[k];
            if constexpr (ACCUM) *reinterpret_cast<f32x4*>(ta + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            if (i >= t.n) break;
            if (vec && i + 4 <= t.n) {
                f32x4 pp = *reinterpret_cast<f32x4*>(t.p + i), mm = *reinterpret_cast<f32x4*>(t.m + i), vv = *reinterpret_cast<f32x4*>(t.v + i);
                f32x4 gg{}, ee{}, aa{};
                if constexpr (HAS_G) gg = *reinterpret_cast<const f32x4*>(t.g + i);
                if constexpr (EMA) ee = *reinterpret_cast<const f32x4*>(te + i);
                if constexpr (ACCUM) aa = *reinterpret_cast<const f32x4*>(ta + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pj = pp[j], mj = mm[j], vj = vv[j];
                    adam_dev_one<true>(pj, eff_grad<ACC>(aa[j], gg[j], inv_k), mj, vj, sc);
                    pp[j] = pj; mm[j] = mj; vv[j] = vj;
                    if constexpr (EMA) ee[j] = adam_ema_one(ee[j], pj, d32, omd32);
                }
                *reinterpret_cast<f32x4*>(t.p + i) = pp; *reinterpret_cast<f32x4*>(t.m + i) = mm; *reinterpret_cast<f32x4*>(t.v + i) = vv;
                if constexpr (EMA) *reinterpret_cast<f32x4*>(te + i) = ee;
                if constexpr (ACCUM) *reinterpret_cast<f32x4*>(ta + i) = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (long long e = i; e < i + 4 && e < t.n; ++e) {
                    if constexpr (ACCUM) {
                        const float ae = ta[e];
                        ta[e] = 0.f;
                        adam_dev_one<false>(t.p[e], eff_grad<ACC>(ae, HAS_G ? t.g[e] : 0.f, inv_k), t.m[e], t.v[e], sc);
                    } else {
                        adam_dev_one<false>(t.p[e], t.g[e], t.m[e], t.v[e], sc);
                    }
                    if constexpr (EMA) te[e] = adam_ema_one(te[e], t.p[e], d32, omd32);
                }
            }
        }
    }
    adam_dev_advance(a);
}

// ---- LAMB: layer-wise trust ratios (hyb_lamb_trust / hyb_lamb_step_dev; You et al. 2020, as timm's Lamb and apex's FusedLAMB without nvlamb) ------
// Per tensor r = |p| / |u| with u = q + wd p, q the bias-corrected Adam direction of THIS step, so the ratio needs m' and v' before the step
// stores them.  lamb_trust_kernel is a read-only chunk pass that forms them exactly as the step will -- the scalars of adam_dev_scalars at
// the same step number, the expressions of adam_dev_one -- and then, in fp32 with contraction off,
//     q = m' / fmaf(sqrtf(v'), inv_sqrt_bc2, eps)            (adam_dev_one's q)
//     u = fmaf(wd32, p, inv_bc1 * q)                          wd32 = (float)wd, inv_bc1 = (float)(1.0 / (1.0 - pow(b1, t))), both rounded once
// and sums p^2 and u^2 as grad_chunk_sumsq sums g^2: a thread's 16 elements in index order with fmaf (the mapping of adamw_dev_kernel, whether
// the tensor is 16-byte aligned or not), wave_sum, the four wave totals pairwise -> partials[2 chunk], partials[2 chunk + 1].  That form of u
// is the contract: the ratios are bit-identical from run to run and independent of how the table is cut into launches.
// lamb_trust_final_kernel, one workgroup per tensor in a launch of its own (the hand-off: see the note on grad_norm above), adds the
// tensor's partials in double in grad_norm_finish's order and writes trust_out[i] = {|p|, |u|, r}.  No floating-point atomics anywhere.
template <bool ACCUM> struct LambTrustArgs : AdamDevTable<ACCUM ? 72 : ADAM_MAX> {      // (advance and ticket stay NULL: nothing is stepped)
    static constexpr int MAX = ACCUM ? 72 : ADAM_MAX;
    unsigned char group[MAX];
    const float* acc[ACCUM ? MAX : 1];
    long long k;
    float inv_k;
    const long long* guard;      // NULL, or the guard block: the step number is less skipped_total, as in the guarded step
    int chunk_offset;            // index of this launch's first chunk among all chunks of the call
    float* partials;
};
static_assert(sizeof(LambTrustArgs<false>) <= 4096 && sizeof(LambTrustArgs<true>) <= 4096, "the tensor table travels in the kernel arguments");

__device__ __forceinline__ void lamb_trust_one(float p, float g, float m, float v, const AdamScalars& a, float inv_bc1, float wd32, float& sp, float& su) {
#pragma clang fp contract(off)
    g = g * a.clip;
    m = __builtin_fmaf(a.omb1, g - m, m);
    v = __builtin_fmaf(a.beta2, v, (a.omb2 * g) * g);
    const float q = m / __builtin_fmaf(sqrtf(v), a.inv_sqrt_bc2, a.eps);
    const float u = __builtin_fmaf(wd32, p, inv_bc1 * q);
    sp = __builtin_fmaf(p, p, sp);
    su = __builtin_fmaf(u, u, su);
}

template <int ACC, bool GROUPS> __global__ __launch_bounds__(256) void lamb_trust_kernel(LambTrustArgs<ACC != GRAD_PLAIN> a) {
    constexpr bool ACCUM = ACC != GRAD_PLAIN, HAS_G = ACC != GRAD_ACC;
    __shared__ float s_sc[10];
    __shared__ float s_wave[8];
    __shared__ int s_skip;
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if ((int)blockIdx.x >= a.chunk_begin[i]) ti = i;
    const AdamTensor t = a.t[ti];
    const float* ta = nullptr;
    float inv_k = 1.f;
    if constexpr (ACCUM) { ta = a.acc[ti]; inv_k = a.inv_k; }
    const long long base = (long long)(blockIdx.x - a.chunk_begin[ti]) * ADAM_CHUNK;
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v | (uintptr_t)ta) & 15) == 0);
    constexpr int NK = ADAM_CHUNK / (256 * 4);
    const bool full = vec && base + ADAM_CHUNK <= t.n;            // as in adamw_dev_kernel: a full chunk's loads go out before the scalar work
    f32x4 p[NK], m[NK], v[NK], g[HAS_G ? NK : 1], ac[ACCUM ? NK : 1];
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            p[k] = *reinterpret_cast<const f32x4*>(t.p + i); m[k] = *reinterpret_cast<const f32x4*>(t.m + i);
            v[k] = *reinterpret_cast<const f32x4*>(t.v + i);
            if constexpr (HAS_G) g[k] = *reinterpret_cast<const f32x4*>(t.g + i);
            if constexpr (ACCUM) ac[k] = *reinterpret_cast<const f32x4*>(ta + i);
        }
    }
    if (threadIdx.x == 0) {
        long long skipped = 0ll;
        bool skip = false;
        if (a.guard) { skip = a.guard[0] != 0ll; skipped = a.guard[1]; }
        s_skip = skip ? 1 : 0;
        if (!skip) {
#pragma clang fp contract(off)
            const double* hyper = a.hyper;
            if constexpr (GROUPS) hyper += HYPER_N * (int)a.group[ti];
            adam_dev_scalars<ACCUM>(a, hyper, s_sc, skipped);
            s_sc[8] = (float)(1.0 / (1.0 - pow(hyper[1], (double)adam_step_number<ACCUM>(a, skipped))));
            s_sc[9] = (float)hyper[4];
        }
    }
    __syncthreads();
    float* out = a.partials + 2ll * (a.chunk_offset + (int)blockIdx.x);
    if (s_skip) {                                                  // a skipped step reads no trust value: zeros (r = 1), and no pass over poison
        if (threadIdx.x == 0) { out[0] = 0.f; out[1] = 0.f; }
        return;
    }
    const AdamScalars sc{s_sc[0], s_sc[1], s_sc[2], s_sc[3], s_sc[4], s_sc[5], s_sc[6], s_sc[7]};
    const float inv_bc1 = s_sc[8], wd32 = s_sc[9];
    float sp = 0.f, su = 0.f;
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                lamb_trust_one(p[k][j], eff_grad<ACC>(ACCUM ? ac[k][j] : 0.f, HAS_G ? g[k][j] : 0.f, inv_k), m[k][j], v[k][j], sc, inv_bc1, wd32, sp, su);
    } else {
#pragma unroll 1
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            for (long long e = i; e < i + 4 && e < t.n; ++e)
                lamb_trust_one(t.p[e], eff_grad<ACC>(ACCUM ? ta[e] : 0.f, HAS_G ? t.g[e] : 0.f, inv_k), t.m[e], t.v[e], sc, inv_bc1, wd32, sp, su);
        }
    }
    sp = wave_sum(sp);
    su = wave_sum(su);
    if ((threadIdx.x & 63) == 0) { s_wave[threadIdx.x >> 6] = sp; s_wave[4 + (threadIdx.x >> 6)] = su; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        out[1] = (s_wave[4] + s_wave[5]) + (s_wave[6] + s_wave[7]);
    }
}

// The final launch serves up to 760 tensors: an int and a byte per tensor in the kernel arguments.
constexpr int LAMB_FINAL_MAX = 760;
struct LambFinalArgs {
    int chunk_begin[LAMB_FINAL_MAX + 1];      // tensor first + i owns the chunks chunk_begin[i] .. chunk_begin[i + 1] of the whole call
    unsigned char group[LAMB_FINAL_MAX];      // its row of hyper (all zero: hyper is the one row)
    int first;
    int always_adapt;
    const float* partials;
    const double* hyper;
    float* trust_out;
};
static_assert(sizeof(LambFinalArgs) <= 4096, "the tensor table travels in the kernel arguments");

__global__ __launch_bounds__(256) void lamb_trust_final_kernel(LambFinalArgs a) {
    __shared__ double s_sum[2][256];
    const int c0 = a.chunk_begin[blockIdx.x], c1 = a.chunk_begin[blockIdx.x + 1];
    double sp = 0.0, su = 0.0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += 256) {         // thread t takes t, t + 256, ... ascending
        sp += (double)a.partials[2ll * c];
        su += (double)a.partials[2ll * c + 1];
    }
    s_sum[0][threadIdx.x] = sp;
    s_sum[1][threadIdx.x] = su;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tp = 0.0, tu = 0.0;
        for (int i = 0; i < 256; ++i) { tp += s_sum[0][i]; tu += s_sum[1][i]; }      // the 256 thread sums in ascending order
        const float w_norm = (float)sqrt(tp), u_norm = (float)sqrt(tu);
        const double wd = a.hyper[HYPER_N * (int)a.group[blockIdx.x] + 4];
        const bool adapt = (wd != 0.0 || a.always_adapt != 0) && w_norm > 0.f && u_norm > 0.f;
        float* out = a.trust_out + 3ll * (a.first + (int)blockIdx.x);
        out[0] = w_norm;
        out[1] = u_norm;
        out[2] = adapt ? (float)((double)w_norm / (double)u_norm) : 1.0f;
    }
}

__global__ __launch_bounds__(64) void ema_set_kernel(double* ema_hyper, double decay, double warmup) {
    if (threadIdx.x < 2) ema_hyper[threadIdx.x] = threadIdx.x == 0 ? decay : warmup;
}

// hyb_adamw_hyper_set_groups: the rows of several groups of hyper[groups, 6] and of ema_hyper[groups, 2] from ONE one-workgroup launch.  The
// values travel in the kernel arguments as hyb_adamw_hyper_set's do; 60 rows of each block fit the 4 KB.  A group appears at most once in
// each list (checked by the caller), so no two threads write one word.
constexpr int HYPER_SET_MAX = 60;
struct HyperSetArgs {
    double* hyper;
    double* ema_hyper;
    int n, ema_n;
    double v[HYPER_SET_MAX * HYPER_N];
    double ema_v[HYPER_SET_MAX * 2];
    unsigned char group[HYPER_SET_MAX], ema_group[HYPER_SET_MAX];
};
static_assert(sizeof(HyperSetArgs) <= 4096, "the values travel in the kernel arguments");

__global__ __launch_bounds__(256) void hyper_set_groups_kernel(HyperSetArgs a) {
    for (int i = threadIdx.x; i < a.n * HYPER_N; i += 256) a.hyper[HYPER_N * (int)a.group[i / HYPER_N] + i % HYPER_N] = a.v[i];
    for (int i = threadIdx.x; i < a.ema_n * 2; i += 256) a.ema_hyper[2 * (int)a.ema_group[i / 2] + i % 2] = a.ema_v[i];
}

// ---- gradient accumulation ----------------------------------------------------------------------------------------------------------------
// acc += g over the whole tensor table in one launch: what ends micro-batches 1 .. k - 1 of an accumulated step.  The chunk -> tensor -> thread
// mapping of adamw_dev_kernel; a full aligned chunk issues its eight 16-byte loads before the first add.
struct AccumArgs {
    float* acc[ADAM_MAX];
    const float* g[ADAM_MAX];
    long long n[ADAM_MAX];
    int chunk_begin[ADAM_MAX + 1];
    int count;
};
static_assert(sizeof(AccumArgs) <= 4096, "the tensor table travels in the kernel arguments");

__global__ __launch_bounds__(256) void grad_accumulate_kernel(AccumArgs a) {
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if ((int)blockIdx.x >= a.chunk_begin[i]) ti = i;
    float* __restrict__ acc = a.acc[ti];
    const float* __restrict__ g = a.g[ti];
    const long long n = a.n[ti];
    const long long base = (long long)(blockIdx.x - a.chunk_begin[ti]) * ADAM_CHUNK;
    const bool vec = ((((uintptr_t)acc | (uintptr_t)g) & 15) == 0);
    constexpr int NK = ADAM_CHUNK / (256 * 4);
    if (vec && base + ADAM_CHUNK <= n) {
        f32x4 x[NK], y[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            x[k] = *reinterpret_cast<const f32x4*>(acc + i); y[k] = *reinterpret_cast<const f32x4*>(g + i);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) *reinterpret_cast<f32x4*>(acc + base + ((long long)k * 256 + threadIdx.x) * 4) = x[k] + y[k];
    } else {
#pragma unroll 1
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            if (i >= n) break;
            if (vec && i + 4 <= n) {
                *reinterpret_cast<f32x4*>(acc + i) = *reinterpret_cast<const f32x4*>(acc + i) + *reinterpret_cast<const f32x4*>(g + i);
            } else {
                for (long long e = i; e < i + 4 && e < n; ++e) acc[e] = acc[e] + g[e];
            }
        }
    }
}

// ---- SGD with momentum, and LARS (hyb_sgd_step_dev / hyb_lars_trust; torch.optim.SGD's rule, timm's Lars without trust clipping) ---------------
// One state tensor per parameter, the momentum buffer: 5 x 4 bytes per parameter where AdamW moves 7 x 4.  The hyper row is the same block,
// read as {lr, momentum, dampening, lars_eps, weight_decay, max_grad_norm}; thread 0 rounds mu32 = (float)momentum, omt32 = (float)(1.0 -
// dampening), wd32 and lr32 once each from its doubles.  Per element at applied step t (adam_step_number), fp32, contraction off, every fused
// multiply-add written out:
//     G    = eff_grad(acc, g, inv_k) * clip
//     d    = fmaf(wd32, p, G)                      coupled L2 decay
//     d    = r * d                                 LARS: r is the tensor's trust ratio (r == 1.0f: the SGD step bit for bit)
//     buf' = t == 1 ? d : fmaf(mu32, buf, omt32 * d)            a select: whatever the buffer held before the first step never reaches buf'
//     s    = nesterov ? fmaf(mu32, buf', d) : mu32 == 0 ? d : buf'      (without momentum torch.optim.SGD steps on d: dampening is not applied)
//     p'   = fmaf(-lr32, s, p)
//     e'   = adam_ema_one(e, p', d32, omd32)
// The table is one type per (EMA, ACCUM) with every optional member in it (group, guard, trust are read by the instantiations that have
// them): 80 tensors per launch, 72 with the average and the accumulators.
struct SgdTensor { float* p; const float* g; float* b; long long n; };
template <bool EMA, bool ACCUM> struct SgdArgs {
    static constexpr int MAX = EMA && ACCUM ? 72 : ADAM_MAX;
    SgdTensor t[MAX];
    int chunk_begin[MAX + 1];
    int count;
    const double* hyper;
    const long long* step_inc;
    long long* advance;
    unsigned int* ticket;
    long long step;
    const float* clip;
    unsigned char group[MAX];
    float* e[EMA ? MAX : 1];
    const double* ema_hyper;
    float* acc[ACCUM ? MAX : 1];
    long long k;
    float inv_k;
    int nesterov;                // 0 or 1, by value: uniform over the launch
    const long long* guard;
    const float* trust;          // LARS: the trust block of hyb_lars_trust, float [3] per tensor of the WHOLE call, and the index of the
    int first;                   // slice's first tensor in it
};
static_assert(sizeof(SgdArgs<false, false>) <= 4096 && sizeof(SgdArgs<true, false>) <= 4096 && sizeof(SgdArgs<false, true>) <= 4096 &&
              sizeof(SgdArgs<true, true>) <= 4096, "the tensor table travels in the kernel arguments");

struct SgdScalars { float mu, omt, wd, lr, clip, r; bool first, nesterov, plain; };      // plain: mu32 == 0, the step is d itself

template <bool LARS> __device__ __forceinline__ void sgd_dev_one(float& p, float g, float& b, const SgdScalars& a) {
#pragma clang fp contract(off)
    g = g * a.clip;
    float d = __builtin_fmaf(a.wd, p, g);
    if constexpr (LARS) d = a.r * d;
    const float nb = a.first ? d : __builtin_fmaf(a.mu, b, a.omt * d);
    const float s = a.nesterov ? __builtin_fmaf(a.mu, nb, d) : a.plain ? d : nb;
    b = nb;
    p = __builtin_fmaf(-a.lr, s, p);
}

// adamw_dev_kernel's frame around sgd_dev_one: the chunk -> tensor -> thread mapping, a full chunk's 16-byte loads in front of the scalar
// phase, the 16-byte path with its 4-element and element-wise remainders, the accumulator stored +0.0f, the guard's skip (no store to
// p / buf / e, accumulators zeroed, ticket taken) and adam_dev_advance on the call's last launch.
template <bool EMA, int ACC = GRAD_PLAIN, bool GUARD = false, bool GROUPS = false, bool LARS = false> __global__ __launch_bounds__(256)
void sgd_dev_kernel(SgdArgs<EMA, ACC != GRAD_PLAIN> a) {
    constexpr bool ACCUM = ACC != GRAD_PLAIN, HAS_G = ACC != GRAD_ACC;
    __shared__ float s_sc[8];
    __shared__ int s_flag[2];                                      // skip, t == 1
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if ((int)blockIdx.x >= a.chunk_begin[i]) ti = i;
    const SgdTensor t = a.t[ti];
    float* te = nullptr;
    if constexpr (EMA) te = a.e[ti];
    float* ta = nullptr;
    float inv_k = 1.f;
    if constexpr (ACCUM) { ta = a.acc[ti]; inv_k = a.inv_k; }
    const long long base = (long long)(blockIdx.x - a.chunk_begin[ti]) * ADAM_CHUNK;
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.b | (uintptr_t)te | (uintptr_t)ta) & 15) == 0);
    constexpr int NK = ADAM_CHUNK / (256 * 4);
    const bool full = vec && base + ADAM_CHUNK <= t.n;
    f32x4 p[NK], b[NK], g[HAS_G ? NK : 1], ea[EMA ? NK : 1], ac[ACCUM ? NK : 1];
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            p[k] = *reinterpret_cast<const f32x4*>(t.p + i); b[k] = *reinterpret_cast<const f32x4*>(t.b + i);
            if constexpr (HAS_G) g[k] = *reinterpret_cast<const f32x4*>(t.g + i);
            if constexpr (EMA) ea[k] = *reinterpret_cast<const f32x4*>(te + i);
            if constexpr (ACCUM) ac[k] = *reinterpret_cast<const f32x4*>(ta + i);
        }
    }
    if (threadIdx.x == 0) {
        long long skipped = 0ll;
        bool skip = false;
        if constexpr (GUARD) { skip = a.guard[0] != 0ll; skipped = a.guard[1]; }
        s_flag[0] = skip ? 1 : 0;
        if (!skip) {
#pragma clang fp contract(off)
            const double* hyper = a.hyper;
            if constexpr (GROUPS) hyper += HYPER_N * (int)a.group[ti];
            s_sc[0] = (float)hyper[1];
            s_sc[1] = (float)(1.0 - hyper[2]);
            s_sc[2] = (float)hyper[4];
            s_sc[3] = (float)hyper[0];
            s_sc[4] = a.clip ? a.clip[1] : 1.0f;
            s_sc[5] = 1.0f;
            if constexpr (LARS) s_sc[5] = a.trust[3ll * (a.first + ti) + 2];
            s_flag[1] = adam_step_number<ACCUM>(a, skipped) == 1ll ? 1 : 0;
            if constexpr (EMA) {
                const double* ema_hyper = a.ema_hyper;
                if constexpr (GROUPS) ema_hyper += 2 * (int)a.group[ti];
                adam_ema_scalars<ACCUM>(a, ema_hyper, s_sc + 6, skipped);
            }
        }
    }
    __syncthreads();
    if constexpr (GUARD) {
        if (s_flag[0]) {                                           // uniform over the workgroup (and over the launch)
            if constexpr (ACCUM) {
#pragma unroll 1
                for (int k = 0; k < NK; ++k) {
                    const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
                    if (i >= t.n) break;
                    if (vec && i + 4 <= t.n) *reinterpret_cast<f32x4*>(ta + i) = f32x4{0.f, 0.f, 0.f, 0.f};
                    else for (long long e = i; e < i + 4 && e < t.n; ++e) ta[e] = 0.f;
                }
            }
            adam_dev_advance(a);
            return;
        }
    }
    const SgdScalars sc{s_sc[0], s_sc[1], s_sc[2], s_sc[3], s_sc[4], s_sc[5], s_flag[1] != 0, a.nesterov != 0, s_sc[0] == 0.f};
    float d32 = 0.f, omd32 = 0.f;
    if constexpr (EMA) { d32 = s_sc[6]; omd32 = s_sc[7]; }
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = p[k][j], bj = b[k][j];
                sgd_dev_one<LARS>(pj, eff_grad<ACC>(ACCUM ? ac[k][j] : 0.f, HAS_G ? g[k][j] : 0.f, inv_k), bj, sc);
                p[k][j] = pj; b[k][j] = bj;
                if constexpr (EMA) ea[k][j] = adam_ema_one(ea[k][j], pj, d32, omd32);
            }
            *reinterpret_cast<f32x4*>(t.p + i) = p[k]; *reinterpret_cast<f32x4*>(t.b + i) = b[k];
            if constexpr (EMA) *reinterpret_cast<f32x4*>(te + i) = ea[k];
            if constexpr (ACCUM) *reinterpret_cast<f32x4*>(ta + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            if (i >= t.n) break;
            if (vec && i + 4 <= t.n) {
                f32x4 pp = *reinterpret_cast<f32x4*>(t.p + i), bb = *reinterpret_cast<f32x4*>(t.b + i);
                f32x4 gg{}, ee{}, aa{};
                if constexpr (HAS_G) gg = *reinterpret_cast<const f32x4*>(t.g + i);
                if constexpr (EMA) ee = *reinterpret_cast<const f32x4*>(te + i);
                if constexpr (ACCUM) aa = *reinterpret_cast<const f32x4*>(ta + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pj = pp[j], bj = bb[j];
                    sgd_dev_one<LARS>(pj, eff_grad<ACC>(aa[j], gg[j], inv_k), bj, sc);
                    pp[j] = pj; bb[j] = bj;
                    if constexpr (EMA) ee[j] = adam_ema_one(ee[j], pj, d32, omd32);
                }
                *reinterpret_cast<f32x4*>(t.p + i) = pp; *reinterpret_cast<f32x4*>(t.b + i) = bb;
                if constexpr (EMA) *reinterpret_cast<f32x4*>(te + i) = ee;
                if constexpr (ACCUM) *reinterpret_cast<f32x4*>(ta + i) = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (long long e = i; e < i + 4 && e < t.n; ++e) {
                    float ge = 0.f, ae = 0.f;
                    if constexpr (HAS_G) ge = t.g[e];
                    if constexpr (ACCUM) { ae = ta[e]; ta[e] = 0.f; }
                    sgd_dev_one<LARS>(t.p[e], eff_grad<ACC>(ae, ge, inv_k), t.b[e], sc);
                    if constexpr (EMA) te[e] = adam_ema_one(te[e], t.p[e], d32, omd32);
                }
            }
        }
    }
    adam_dev_advance(a);
}

// LARS: per tensor r = trust_coeff |p| / (|G| + wd |p| + eps), G the effective, clipped gradient of THIS step.  lars_trust_kernel is a
// read-only chunk pass over p and G (2 x 4 bytes per parameter, 3 x 4 when accumulating) that sums p^2 and G^2 as grad_chunk_sumsq sums g^2:
// a thread's 16 elements in index order with fmaf (the mapping of sgd_dev_kernel, aligned or not), wave_sum, the four wave totals pairwise
// -> partials[2 chunk], partials[2 chunk + 1]; it needs no hyper-parameter, only the clip coefficient and the guard's decision.
// lars_trust_final_kernel, one workgroup per tensor in a launch of its own (the hand-off: see the note on grad_norm above), adds the
// tensor's partials in double in lamb_trust_final_kernel's order and writes trust_out[i] = {|p|, |G|, r}; weight_decay and lars_eps are
// read from the tensor's row of hyper there.  Bit-identical from run to run, independent of how the table is sliced.
struct LarsTrustArgs {
    const float* p[ADAM_MAX];
    const float* g[ADAM_MAX];
    const float* acc[ADAM_MAX];
    long long n[ADAM_MAX];
    int chunk_begin[ADAM_MAX + 1];
    int count;
    float inv_k;
    const float* clip;
    const long long* guard;      // NULL, or the guard block: a skipped step reads no trust value
    int chunk_offset;            // index of this launch's first chunk among all chunks of the call
    float* partials;
};
static_assert(sizeof(LarsTrustArgs) <= 4096, "the tensor table travels in the kernel arguments");

__device__ __forceinline__ void lars_trust_one(float p, float g, float clip, float& sp, float& sg) {
#pragma clang fp contract(off)
    g = g * clip;
    sp = __builtin_fmaf(p, p, sp);
    sg = __builtin_fmaf(g, g, sg);
}

template <int ACC> __global__ __launch_bounds__(256) void lars_trust_kernel(LarsTrustArgs a) {
    constexpr bool ACCUM = ACC != GRAD_PLAIN, HAS_G = ACC != GRAD_ACC;
    __shared__ float s_clip;
    __shared__ float s_wave[8];
    __shared__ int s_skip;
    int ti = 0;
    for (int i = 1; i < a.count; ++i)
        if ((int)blockIdx.x >= a.chunk_begin[i]) ti = i;
    const float* __restrict__ tp = a.p[ti];
    const float* __restrict__ tg = a.g[ti];
    const float* __restrict__ ta = a.acc[ti];
    const long long n = a.n[ti];
    const float inv_k = a.inv_k;
    const long long base = (long long)(blockIdx.x - a.chunk_begin[ti]) * ADAM_CHUNK;
    const bool vec = ((((uintptr_t)tp | (uintptr_t)tg | (uintptr_t)ta) & 15) == 0);
    constexpr int NK = ADAM_CHUNK / (256 * 4);
    const bool full = vec && base + ADAM_CHUNK <= n;
    f32x4 p[NK], g[HAS_G ? NK : 1], ac[ACCUM ? NK : 1];
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            p[k] = *reinterpret_cast<const f32x4*>(tp + i);
            if constexpr (HAS_G) g[k] = *reinterpret_cast<const f32x4*>(tg + i);
            if constexpr (ACCUM) ac[k] = *reinterpret_cast<const f32x4*>(ta + i);
        }
    }
    if (threadIdx.x == 0) {
        const bool skip = a.guard && a.guard[0] != 0ll;
        s_skip = skip ? 1 : 0;
        s_clip = !skip && a.clip ? a.clip[1] : 1.0f;
    }
    __syncthreads();
    float* out = a.partials + 2ll * (a.chunk_offset + (int)blockIdx.x);
    if (s_skip) {                                                  // zeros (r = 1), and no pass over poison
        if (threadIdx.x == 0) { out[0] = 0.f; out[1] = 0.f; }
        return;
    }
    const float clip = s_clip;
    float sp = 0.f, sg = 0.f;
    if (full) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                lars_trust_one(p[k][j], eff_grad<ACC>(ACCUM ? ac[k][j] : 0.f, HAS_G ? g[k][j] : 0.f, inv_k), clip, sp, sg);
    } else {
#pragma unroll 1
        for (int k = 0; k < NK; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            for (long long e = i; e < i + 4 && e < n; ++e) {
                float ge = 0.f, ae = 0.f;
                if constexpr (HAS_G) ge = tg[e];
                if constexpr (ACCUM) ae = ta[e];
                lars_trust_one(tp[e], eff_grad<ACC>(ae, ge, inv_k), clip, sp, sg);
            }
        }
    }
    sp = wave_sum(sp);
    sg = wave_sum(sg);
    if ((threadIdx.x & 63) == 0) { s_wave[threadIdx.x >> 6] = sp; s_wave[4 + (threadIdx.x >> 6)] = sg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        out[1] = (s_wave[4] + s_wave[5]) + (s_wave[6] + s_wave[7]);
    }
}

struct LarsFinalArgs {
    int chunk_begin[LAMB_FINAL_MAX + 1];      // tensor first + i owns the chunks chunk_begin[i] .. chunk_begin[i + 1] of the whole call
    unsigned char group[LAMB_FINAL_MAX];      // its row of hyper (all zero: hyper is the one row)
    int first;
    int always_adapt;
    double trust_coeff;
    const float* partials;
    const double* hyper;
    float* trust_out;
};
static_assert(sizeof(LarsFinalArgs) <= 4096, "the tensor table travels in the kernel arguments");

__global__ __launch_bounds__(256) void lars_trust_final_kernel(LarsFinalArgs a) {
    __shared__ double s_sum[2][256];
    const int c0 = a.chunk_begin[blockIdx.x], c1 = a.chunk_begin[blockIdx.x + 1];
    double sp = 0.0, sg = 0.0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += 256) {         // thread t takes t, t + 256, ... ascending
        sp += (double)a.partials[2ll * c];
        sg += (double)a.partials[2ll * c + 1];
    }
    s_sum[0][threadIdx.x] = sp;
    s_sum[1][threadIdx.x] = sg;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        double tp = 0.0, tg = 0.0;
        for (int i = 0; i < 256; ++i) { tp += s_sum[0][i]; tg += s_sum[1][i]; }      // the 256 thread sums in ascending order
        const float w_norm = (float)sqrt(tp), g_norm = (float)sqrt(tg);
        const double* hyper = a.hyper + HYPER_N * (int)a.group[blockIdx.x];
        const double eps = hyper[3], wd = hyper[4];
        const bool adapt = (wd != 0.0 || a.always_adapt != 0) && w_norm > 0.f && g_norm > 0.f;
        const double decayed = (double)w_norm * wd;
        float* out = a.trust_out + 3ll * (a.first + (int)blockIdx.x);
        out[0] = w_norm;
        out[1] = g_norm;
        out[2] = adapt ? (float)(a.trust_coeff * (double)w_norm / (((double)g_norm + decayed) + eps)) : 1.0f;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// Every entry point below works on a table of `count` tensors.  Three helpers are all of them share: table_ok (the table is sound),
// for_each_slice (the table in launches of at most a kernel's capacity) and, for the device-path steps, one descriptor (AdamStep) with one
// validity rule (adam_step_ok) and one dispatch (adam_step_launch).  Nothing is launched before the whole call has been checked.

// count > 0, numel and every listed array given, no NULL entry, every numel positive, and the chunks of the whole table fit an int (the
// kernels index them with one)
template <typename... T> bool table_ok(int count, const long long* numel, const T* const*... arrays) {
    if (count <= 0 || !numel || !(arrays && ...)) return false;
    long long chunks = 0;
    for (int i = 0; i < count; ++i) {                                // (the sum in long long, tested as it grows: no tensor can wrap it)
        if (numel[i] <= 0 || !(arrays[i] && ...) || (chunks += (numel[i] - 1) / ADAM_CHUNK + 1) >= (1ll << 31)) return false;
    }
    return true;
}

// The table in slices of at most `capacity` tensors: launch(first, n, chunk_begin, last) gets tensors [first, first + n), chunk_begin[0 .. n]
// (tensor first + i owns the workgroups chunk_begin[i] .. chunk_begin[i + 1] of the slice's launch) and whether this is the call's last slice
// (the one that advances a counter).  Stops at the first non-zero status.
template <typename Launch> int for_each_slice(int count, const long long* numel, int capacity, Launch&& launch) {
    for (int first = 0; first < count; first += capacity) {
        const int n = count - first < capacity ? count - first : capacity;
        int chunk_begin[ADAM_MAX + 1] = {};
        for (int i = 0; i < n; ++i) chunk_begin[i + 1] = chunk_begin[i] + hyb_cdiv(numel[first + i], ADAM_CHUNK);
        const int rc = launch(first, n, chunk_begin, first + capacity >= count);
        if (rc != 0) return rc;
    }
    return 0;
}

template <typename Kernel, typename Args> int launch_chunks(Kernel kernel, const Args& a, void* stream) {
    hipLaunchKernelGGL(kernel, dim3(a.chunk_begin[a.count]), dim3(256), 0, (hipStream_t)stream, a);
    HYB_LAUNCH_CHECK();
    return 0;
}

// What any device-path step call is, in the order of hyb_adamw_step_dev_groups' parameters.  NULL where a call has no such thing: grads (the
// accumulators hold the whole sum), acc (k == 1), ema and ema_hyper (no average), group (one group: hyper / ema_hyper are its rows, not the
// blocks' bases), ticket (the counter does not advance), clip, guard.
struct AdamStep {
    int count;
    float* const* params; const float* const* grads; float* const* exp_avg; float* const* exp_avg_sq; float* const* acc; float* const* ema;
    const long long* numel;
    const unsigned char* group; int groups;
    const double* hyper; const double* ema_hyper;
    long long k, step; long long* step_inc; unsigned int* ticket;
    const float* clip; const long long* guard;
    const float* trust;          // NULL: AdamW.  The trust block of hyb_lamb_trust, float [count, 3]: the LAMB step (hyb_lamb_step_dev)
    // The SGD calls (hyb_sgd_step_dev, hyb_lars_trust) are the same descriptor: exp_avg is the momentum buffer, exp_avg_sq stays NULL, trust
    // is hyb_lars_trust's block.  RULE_LARS_PASS: the read-only pass, which takes no state table at all.
    int rule;
    int nesterov;
};
constexpr int RULE_ADAM = 0, RULE_SGD = 1, RULE_LARS_PASS = 2;

// the one rule; an entry point adds only what its own prototype promises (hyb_adamw_step_dev: grads, ...)
bool adam_step_ok(const AdamStep& s) {
    const bool tables = s.rule == RULE_ADAM ? table_ok(s.count, s.numel, s.params, s.exp_avg, s.exp_avg_sq)
                      : s.rule == RULE_SGD  ? table_ok(s.count, s.numel, s.params, s.exp_avg) : table_ok(s.count, s.numel, s.params);
    if (!tables || !s.hyper || s.step < 1 || s.k < 1 || !(s.acc || (s.k == 1 && s.grads)) || (s.nesterov != 0 && s.nesterov != 1) ||
        (s.ema != nullptr) != (s.ema_hyper != nullptr) || (s.ticket && !s.step_inc) || (s.guard && !s.clip) ||
        (s.group && (s.groups < 1 || s.groups > ADAM_GROUPS_MAX))) return false;     // (the LAMB calls take group or NULL: the range is the rule's)
    for (int i = 0; i < s.count; ++i)
        if ((s.grads && !s.grads[i]) || (s.acc && (!s.acc[i] || s.acc[i] == s.params[i])) || (s.ema && (!s.ema[i] || s.ema[i] == s.params[i])) ||
            (s.group && (int)s.group[i] >= s.groups)) return false;
    return true;
}

// one instantiation of adamw_dev_kernel over the whole table; the last launch of the call advances the counter
template <bool EMA, int ACC, bool GUARD, bool GROUPS, bool LAMB> int adamw_dev_launch(const AdamStep& s, void* stream) {
    using Args = AdamDevKernelArgs<EMA, ACC, GUARD, GROUPS, LAMB>;
    return for_each_slice(s.count, s.numel, (int)(sizeof(Args::t) / sizeof(AdamTensor)), [&](int first, int n, const int* chunk_begin, bool last) {
        Args a{};
        for (int i = 0; i < n; ++i) {
            a.t[i] = AdamTensor{s.params[first + i], ACC == GRAD_ACC ? nullptr : s.grads[first + i], s.exp_avg[first + i], s.exp_avg_sq[first + i], s.numel[first + i]};
            if constexpr (EMA) a.e[i] = s.ema[first + i];
            if constexpr (ACC != GRAD_PLAIN) a.acc[i] = s.acc[first + i];
            if constexpr (GROUPS) a.group[i] = s.group[first + i];
        }
        std::copy(chunk_begin, chunk_begin + n + 1, a.chunk_begin);
        a.count = n;
        a.hyper = s.hyper; a.step_inc = s.step_inc; a.step = s.step; a.clip = s.clip;
        if constexpr (EMA) a.ema_hyper = s.ema_hyper;
        if constexpr (ACC != GRAD_PLAIN) { a.k = s.k; a.inv_k = (float)(1.0 / (double)s.k); }
        if constexpr (GUARD) a.guard = s.guard;
        if constexpr (LAMB) { a.trust = s.trust; a.first = first; }
        a.advance = (s.ticket && last) ? s.step_inc : nullptr;
        a.ticket = s.ticket;
        return launch_chunks(adamw_dev_kernel<EMA, ACC, GUARD, GROUPS, LAMB>, a, stream);
    });
}

// (ema, acc and grads, guard, group, trust) given or not -> the 2 x 3 x 2 x 2 x 2 instantiations
template <typename F> int with_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
int adam_step_launch(const AdamStep& s, void* stream) {
    return with_flag(s.ema != nullptr, [&](auto ema) { return with_flag(s.guard != nullptr, [&](auto guard) { return with_flag(s.group != nullptr, [&](auto groups) {
        return with_flag(s.trust != nullptr, [&](auto lamb) {
            constexpr bool EMA = decltype(ema)::value, GUARD = decltype(guard)::value, GROUPS = decltype(groups)::value, LAMB = decltype(lamb)::value;
            if (!s.acc) return adamw_dev_launch<EMA, GRAD_PLAIN, GUARD, GROUPS, LAMB>(s, stream);
            if (s.grads) return adamw_dev_launch<EMA, GRAD_ACC_G, GUARD, GROUPS, LAMB>(s, stream);
            return adamw_dev_launch<EMA, GRAD_ACC, GUARD, GROUPS, LAMB>(s, stream);
        });
    }); }); });
}

int adam_step(const AdamStep& s, void* stream) {
    HYB_CHECK_ARG(adam_step_ok(s));
    return adam_step_launch(s, stream);
}

// The trust pass of the step that `s` describes (no average, no ticket: nothing is stepped): the chunk launches over the table in slices,
// then the final launches, one workgroup per tensor.
template <int ACC, bool GROUPS> int lamb_trust_launch(const AdamStep& s, int always_adapt, float* partials, float* trust_out, void* stream) {
    using Args = LambTrustArgs<ACC != GRAD_PLAIN>;
    int total = 0;
    const int rc = for_each_slice(s.count, s.numel, Args::MAX, [&](int first, int n, const int* chunk_begin, bool) {
        Args a{};
        for (int i = 0; i < n; ++i) {
            a.t[i] = AdamTensor{s.params[first + i], ACC == GRAD_ACC ? nullptr : s.grads[first + i], s.exp_avg[first + i], s.exp_avg_sq[first + i], s.numel[first + i]};
            if constexpr (ACC != GRAD_PLAIN) a.acc[i] = s.acc[first + i];
            if constexpr (GROUPS) a.group[i] = s.group[first + i];
        }
        std::copy(chunk_begin, chunk_begin + n + 1, a.chunk_begin);
        a.count = n;
        a.hyper = s.hyper; a.step_inc = s.step_inc; a.step = s.step; a.clip = s.clip;
        a.k = s.k; a.inv_k = (float)(1.0 / (double)s.k);
        a.guard = s.guard;
        a.chunk_offset = total;
        a.partials = partials;
        total += chunk_begin[n];
        return launch_chunks(lamb_trust_kernel<ACC, GROUPS>, a, stream);
    });
    if (rc != 0) return rc;
    for (int first = 0, chunk = 0; first < s.count; first += LAMB_FINAL_MAX) {
        LambFinalArgs f{};
        const int n = s.count - first < LAMB_FINAL_MAX ? s.count - first : LAMB_FINAL_MAX;
        for (int i = 0; i < n; ++i) {
            f.chunk_begin[i] = chunk;
            chunk += hyb_cdiv(s.numel[first + i], ADAM_CHUNK);
            if constexpr (GROUPS) f.group[i] = s.group[first + i];
        }
        f.chunk_begin[n] = chunk;
        f.first = first; f.always_adapt = always_adapt; f.partials = partials; f.hyper = s.hyper; f.trust_out = trust_out;
        hipLaunchKernelGGL(lamb_trust_final_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, f);
        HYB_LAUNCH_CHECK();
    }
    return 0;
}

int lamb_trust_call(const AdamStep& s, int always_adapt, float* partials, float* trust_out, void* stream) {
    HYB_CHECK_ARG(adam_step_ok(s) && !s.ema && !s.ticket && (always_adapt == 0 || always_adapt == 1) && partials && trust_out);
    return with_flag(s.group != nullptr, [&](auto groups) {
        constexpr bool GROUPS = decltype(groups)::value;
        if (!s.acc) return lamb_trust_launch<GRAD_PLAIN, GROUPS>(s, always_adapt, partials, trust_out, stream);
        if (s.grads) return lamb_trust_launch<GRAD_ACC_G, GROUPS>(s, always_adapt, partials, trust_out, stream);
        return lamb_trust_launch<GRAD_ACC, GROUPS>(s, always_adapt, partials, trust_out, stream);
    });
}

// one instantiation of sgd_dev_kernel over the whole table; the last launch of the call advances the counter
template <bool EMA, int ACC, bool GUARD, bool GROUPS, bool LARS> int sgd_dev_launch(const AdamStep& s, void* stream) {
    using Args = SgdArgs<EMA, ACC != GRAD_PLAIN>;
    return for_each_slice(s.count, s.numel, Args::MAX, [&](int first, int n, const int* chunk_begin, bool last) {
        Args a{};
        for (int i = 0; i < n; ++i) {
            a.t[i] = SgdTensor{s.params[first + i], ACC == GRAD_ACC ? nullptr : s.grads[first + i], s.exp_avg[first + i], s.numel[first + i]};
            if constexpr (EMA) a.e[i] = s.ema[first + i];
            if constexpr (ACC != GRAD_PLAIN) a.acc[i] = s.acc[first + i];
            if constexpr (GROUPS) a.group[i] = s.group[first + i];
        }
        std::copy(chunk_begin, chunk_begin + n + 1, a.chunk_begin);
        a.count = n;
        a.hyper = s.hyper; a.step_inc = s.step_inc; a.step = s.step; a.clip = s.clip; a.ema_hyper = s.ema_hyper;
        a.k = s.k; a.inv_k = (float)(1.0 / (double)s.k);
        a.nesterov = s.nesterov; a.guard = s.guard; a.trust = s.trust; a.first = first;
        a.advance = (s.ticket && last) ? s.step_inc : nullptr;
        a.ticket = s.ticket;
        return launch_chunks(sgd_dev_kernel<EMA, ACC, GUARD, GROUPS, LARS>, a, stream);
    });
}

// (ema, acc and grads, guard, group, trust) given or not -> the 2 x 3 x 2 x 2 x 2 instantiations; nesterov is an argument
int sgd_step(const AdamStep& s, void* stream) {
    HYB_CHECK_ARG(s.rule == RULE_SGD && adam_step_ok(s));
    return with_flag(s.ema != nullptr, [&](auto ema) { return with_flag(s.guard != nullptr, [&](auto guard) { return with_flag(s.group != nullptr, [&](auto groups) {
        return with_flag(s.trust != nullptr, [&](auto lars) {
            constexpr bool EMA = decltype(ema)::value, GUARD = decltype(guard)::value, GROUPS = decltype(groups)::value, LARS = decltype(lars)::value;
            if (!s.acc) return sgd_dev_launch<EMA, GRAD_PLAIN, GUARD, GROUPS, LARS>(s, stream);
            if (s.grads) return sgd_dev_launch<EMA, GRAD_ACC_G, GUARD, GROUPS, LARS>(s, stream);
            return sgd_dev_launch<EMA, GRAD_ACC, GUARD, GROUPS, LARS>(s, stream);
        });
    }); }); });
}

// The trust pass of the SGD step that `s` describes: the chunk launches over the table in slices, then the final launches, one workgroup
// per tensor.
int lars_trust_call(const AdamStep& s, double trust_coeff, int always_adapt, float* partials, float* trust_out, void* stream) {
    HYB_CHECK_ARG(s.rule == RULE_LARS_PASS && adam_step_ok(s) && trust_coeff > 0.0 && trust_coeff < (double)INFINITY &&
                  (always_adapt == 0 || always_adapt == 1) && partials && trust_out);
    int total = 0;
    const int rc = for_each_slice(s.count, s.numel, ADAM_MAX, [&](int first, int n, const int* chunk_begin, bool) {
        LarsTrustArgs a{};
        for (int i = 0; i < n; ++i) {
            a.p[i] = s.params[first + i]; a.n[i] = s.numel[first + i];
            a.g[i] = s.grads ? s.grads[first + i] : nullptr;
            a.acc[i] = s.acc ? s.acc[first + i] : nullptr;
        }
        std::copy(chunk_begin, chunk_begin + n + 1, a.chunk_begin);
        a.count = n;
        a.inv_k = (float)(1.0 / (double)s.k);
        a.clip = s.clip; a.guard = s.guard;
        a.chunk_offset = total;
        a.partials = partials;
        total += chunk_begin[n];
        if (!s.acc) return launch_chunks(lars_trust_kernel<GRAD_PLAIN>, a, stream);
        return s.grads ? launch_chunks(lars_trust_kernel<GRAD_ACC_G>, a, stream) : launch_chunks(lars_trust_kernel<GRAD_ACC>, a, stream);
    });
    if (rc != 0) return rc;
    for (int first = 0, chunk = 0; first < s.count; first += LAMB_FINAL_MAX) {
        LarsFinalArgs f{};
        const int n = s.count - first < LAMB_FINAL_MAX ? s.count - first : LAMB_FINAL_MAX;
        for (int i = 0; i < n; ++i) {
            f.chunk_begin[i] = chunk;
            chunk += hyb_cdiv(s.numel[first + i], ADAM_CHUNK);
            if (s.group) f.group[i] = s.group[first + i];
        }
        f.chunk_begin[n] = chunk;
        f.first = first; f.always_adapt = always_adapt; f.trust_coeff = trust_coeff; f.partials = partials; f.hyper = s.hyper; f.trust_out = trust_out;
        hipLaunchKernelGGL(lars_trust_final_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, f);
        HYB_LAUNCH_CHECK();
    }
    return 0;
}

// The four norm entry points: acc == NULL is the plain norm of grads (k == 1), acc given the norm of (acc + grads) / k, or of acc / k without
// grads; guard given: the final launch that also takes the skip decision.  The same chunk launches, the same final sum.
int grad_norm_call(int count, const float* const* acc, const float* const* grads, const long long* numel, long long k, float* partials,
                   const double* hyper, float* norm_out, long long* guard, void* stream) {
    HYB_CHECK_ARG((!acc ? table_ok(count, numel, grads) : grads ? table_ok(count, numel, acc, grads) : table_ok(count, numel, acc)) && k >= 1 &&
                  partials && hyper && norm_out);
    int total = 0;
    const int rc = for_each_slice(count, numel, ADAM_MAX, [&](int first, int n, const int* chunk_begin, bool) {
        GradNormAccArgs a{};
        for (int i = 0; i < n; ++i) {
            a.g[i] = grads ? grads[first + i] : nullptr; a.n[i] = numel[first + i];
            if (acc) a.acc[i] = acc[first + i];
        }
        std::copy(chunk_begin, chunk_begin + n + 1, a.chunk_begin);
        a.count = n;
        a.chunk_offset = total;
        a.partials = partials;
        a.inv_k = (float)(1.0 / (double)k);
        total += chunk_begin[n];
        if (!acc) return launch_chunks(grad_norm_kernel, static_cast<const GradNormArgs&>(a), stream);
        return grads ? launch_chunks(grad_norm_acc_kernel<GRAD_ACC_G>, a, stream) : launch_chunks(grad_norm_acc_kernel<GRAD_ACC>, a, stream);
    });
    if (rc != 0) return rc;
    if (guard) hipLaunchKernelGGL(grad_norm_final_guard_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, total, hyper, norm_out, guard);
    else hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, total, hyper, norm_out);
    HYB_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// The by-value step.  The WHOLE table is checked before the first launch -- a NULL entry or a numel <= 0 in a later slice (past the 80th
// tensor) is refused with nothing stepped -- and so is a table whose chunks do not fit an int, as by every entry point of this file.
extern "C" int hyb_adamw_step(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                              const long long* numel, double lr, double beta1, double beta2, double eps, double weight_decay, long long step,
                              long long* step_inc, unsigned int* advance_ticket, void* stream) {
    HYB_CHECK_ARG(table_ok(count, numel, params, grads, exp_avg, exp_avg_sq) && step >= 1 && lr >= 0.0 && (!advance_ticket || step_inc));
    // every scalar is formed in double from the caller's doubles and rounded once, as torch does with its Python floats
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamArgs scalars{};
    scalars.decay = (float)(1.0 - lr * weight_decay);
    scalars.omb1 = (float)(1.0 - beta1); scalars.beta2 = (float)beta2; scalars.omb2 = (float)(1.0 - beta2); scalars.eps = (float)eps;
    scalars.step_size = (float)(lr / bc1);
    scalars.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    scalars.step_inc = step_inc; scalars.step = step; scalars.lr = lr; scalars.beta1d = beta1; scalars.beta2d = beta2;
    scalars.ticket = advance_ticket;
    return for_each_slice(count, numel, ADAM_MAX, [&](int first, int n, const int* chunk_begin, bool last) {
        AdamArgs a = scalars;
        for (int i = 0; i < n; ++i) a.t[i] = AdamTensor{params[first + i], grads[first + i], exp_avg[first + i], exp_avg_sq[first + i], numel[first + i]};
        std::copy(chunk_begin, chunk_begin + n + 1, a.chunk_begin);
        a.count = n;
        a.advance = (advance_ticket && last) ? step_inc : nullptr;            // the last launch of the call advances the counter
        return launch_chunks(adamw_kernel, a, stream);
    });
}

// acc += grads.  The chunks of the WHOLE table must fit an int, checked before the first launch (not slice by slice, after earlier slices
// have been added).
extern "C" int hyb_grad_accumulate(int count, float* const* acc, const float* const* grads, const long long* numel, void* stream) {
    HYB_CHECK_ARG(table_ok(count, numel, acc, grads));
    for (int i = 0; i < count; ++i) HYB_CHECK_ARG(acc[i] != grads[i]);
    return for_each_slice(count, numel, ADAM_MAX, [&](int first, int n, const int* chunk_begin, bool) {
        AccumArgs a{};
        for (int i = 0; i < n; ++i) { a.acc[i] = acc[first + i]; a.g[i] = grads[first + i]; a.n[i] = numel[first + i]; }
        std::copy(chunk_begin, chunk_begin + n + 1, a.chunk_begin);
        a.count = n;
        return launch_chunks(grad_accumulate_kernel, a, stream);
    });
}

extern "C" size_t hyb_grad_norm_workspace(int count, const long long* numel) {
    if (count <= 0 || !numel) return 0;
    size_t chunks = 0;
    for (int i = 0; i < count; ++i) {
        if (numel[i] <= 0) return 0;
        chunks += (size_t)hyb_cdiv(numel[i], ADAM_CHUNK);
    }
    return chunks;
}

extern "C" int hyb_grad_norm(int count, const float* const* grads, const long long* numel, float* partials, const double* hyper,
                             float* norm_out, void* stream) {
    return grad_norm_call(count, nullptr, grads, numel, 1, partials, hyper, norm_out, nullptr, stream);
}

extern "C" int hyb_grad_norm_guard(int count, const float* const* grads, const long long* numel, float* partials, const double* hyper,
                                   float* norm_out, long long* guard, void* stream) {
    HYB_CHECK_ARG(guard);
    return grad_norm_call(count, nullptr, grads, numel, 1, partials, hyper, norm_out, guard, stream);
}

extern "C" int hyb_grad_norm_acc(int count, const float* const* acc, const float* const* grads, const long long* numel, long long k, float* partials,
                                 const double* hyper, float* norm_out, void* stream) {
    HYB_CHECK_ARG(acc);
    return grad_norm_call(count, acc, grads, numel, k, partials, hyper, norm_out, nullptr, stream);
}

extern "C" int hyb_grad_norm_acc_guard(int count, const float* const* acc, const float* const* grads, const long long* numel, long long k,
                                       float* partials, const double* hyper, float* norm_out, long long* guard, void* stream) {
    HYB_CHECK_ARG(acc && guard);
    return grad_norm_call(count, acc, grads, numel, k, partials, hyper, norm_out, guard, stream);
}

// ---- the five device-path steps: each states what its own prototype requires, fills the descriptor and forwards -------------------------------
extern "C" int hyb_adamw_step_dev(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                  const long long* numel, const double* hyper, long long step, long long* step_inc,
                                  unsigned int* advance_ticket, const float* clip, void* stream) {
    HYB_CHECK_ARG(grads);
    return adam_step({count, params, grads, exp_avg, exp_avg_sq, nullptr, nullptr, numel, nullptr, 0, hyper, nullptr, 1, step, step_inc, advance_ticket, clip, nullptr}, stream);
}

extern "C" int hyb_adamw_step_dev_ema(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                      float* const* ema, const long long* numel, const double* hyper, const double* ema_hyper, long long step,
                                      long long* step_inc, unsigned int* advance_ticket, const float* clip, void* stream) {
    HYB_CHECK_ARG(grads && ema && ema_hyper);
    return adam_step({count, params, grads, exp_avg, exp_avg_sq, nullptr, ema, numel, nullptr, 0, hyper, ema_hyper, 1, step, step_inc, advance_ticket, clip, nullptr}, stream);
}

extern "C" int hyb_adamw_step_dev_acc(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                      float* const* acc, float* const* ema, const long long* numel, const double* hyper, const double* ema_hyper,
                                      long long k, long long step, long long* step_inc, unsigned int* advance_ticket, const float* clip, void* stream) {
    HYB_CHECK_ARG(acc);
    return adam_step({count, params, grads, exp_avg, exp_avg_sq, acc, ema, numel, nullptr, 0, hyper, ema_hyper, k, step, step_inc, advance_ticket, clip, nullptr}, stream);
}

// every variant of the device-path step behind one entry point: acc == NULL (k == 1) is the plain step, with or without the average
extern "C" int hyb_adamw_step_dev_guard(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                        float* const* acc, float* const* ema, const long long* numel, const double* hyper, const double* ema_hyper,
                                        long long k, long long step, long long* step_inc, unsigned int* advance_ticket, const float* clip,
                                        const long long* guard, void* stream) {
    HYB_CHECK_ARG(guard && clip);
    return adam_step({count, params, grads, exp_avg, exp_avg_sq, acc, ema, numel, nullptr, 0, hyper, ema_hyper, k, step, step_inc, advance_ticket, clip, guard}, stream);
}

// the same variants over the tensors of several parameter groups: hyper / ema_hyper are the bases of the blocks, group[i] picks tensor i's row
extern "C" int hyb_adamw_step_dev_groups(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                         float* const* acc, float* const* ema, const long long* numel, const unsigned char* group, int groups,
                                         const double* hyper, const double* ema_hyper, long long k, long long step, long long* step_inc,
                                         unsigned int* advance_ticket, const float* clip, const long long* guard, void* stream) {
    HYB_CHECK_ARG(group && groups >= 1 && groups <= ADAM_GROUPS_MAX);
    return adam_step({count, params, grads, exp_avg, exp_avg_sq, acc, ema, numel, group, groups, hyper, ema_hyper, k, step, step_inc, advance_ticket, clip, guard}, stream);
}

// ---- LAMB: the trust pass, then the step that reads it -- the same descriptor, group or not ---------------------------------------------------
extern "C" size_t hyb_lamb_trust_workspace(int count, const long long* numel) { return 2 * hyb_grad_norm_workspace(count, numel); }

extern "C" int hyb_lamb_trust(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                              float* const* acc, const long long* numel, const unsigned char* group, int groups, const double* hyper, long long k,
                              long long step, long long* step_inc, const float* clip, const long long* guard, int always_adapt, float* partials,
                              float* trust_out, void* stream) {
    return lamb_trust_call({count, params, grads, exp_avg, exp_avg_sq, acc, nullptr, numel, group, groups, hyper, nullptr, k, step, step_inc, nullptr, clip, guard, nullptr},
                           always_adapt, partials, trust_out, stream);
}

extern "C" int hyb_lamb_step_dev(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                 float* const* acc, float* const* ema, const long long* numel, const unsigned char* group, int groups,
                                 const double* hyper, const double* ema_hyper, long long k, long long step, long long* step_inc,
                                 unsigned int* advance_ticket, const float* clip, const long long* guard, const float* trust, void* stream) {
    HYB_CHECK_ARG(trust);
    return adam_step({count, params, grads, exp_avg, exp_avg_sq, acc, ema, numel, group, groups, hyper, ema_hyper, k, step, step_inc, advance_ticket, clip, guard, trust}, stream);
}

// ---- SGD and LARS: the same descriptor with one state table, checked by the same rule -----------------------------------------------------------
extern "C" int hyb_sgd_step_dev(int count, float* const* params, const float* const* grads, float* const* momentum_buf, float* const* acc,
                                float* const* ema, const long long* numel, const unsigned char* group, int groups, const double* hyper,
                                const double* ema_hyper, long long k, long long step, long long* step_inc, unsigned int* advance_ticket,
                                const float* clip, const long long* guard, int nesterov, const float* trust, void* stream) {
    return sgd_step({count, params, grads, momentum_buf, nullptr, acc, ema, numel, group, groups, hyper, ema_hyper, k, step, step_inc, advance_ticket, clip, guard,
                     trust, RULE_SGD, nesterov}, stream);
}

extern "C" size_t hyb_lars_trust_workspace(int count, const long long* numel) { return 2 * hyb_grad_norm_workspace(count, numel); }

extern "C" int hyb_lars_trust(int count, float* const* params, const float* const* grads, float* const* acc, const long long* numel,
                              const unsigned char* group, int groups, const double* hyper, long long k, const float* clip, const long long* guard,
                              double trust_coeff, int always_adapt, float* partials, float* trust_out, void* stream) {
    return lars_trust_call({count, params, grads, nullptr, nullptr, acc, nullptr, numel, group, groups, hyper, nullptr, k, 1, nullptr, nullptr, clip, guard, nullptr,
                            RULE_LARS_PASS, 0}, trust_coeff, always_adapt, partials, trust_out, stream);
}

// ---- the uploads of the device blocks -----------------------------------------------------------------------------------------------------------
extern "C" int hyb_adamw_hyper_set(double* hyper, double lr, double beta1, double beta2, double eps, double weight_decay, double max_grad_norm,
                                   void* stream) {
    HYB_CHECK_ARG(hyper && lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0 &&
                  max_grad_norm == max_grad_norm);
    const HyperVals h{{lr, beta1, beta2, eps, weight_decay, max_grad_norm}};
    hipLaunchKernelGGL(hyper_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper, h);
    HYB_LAUNCH_CHECK();
    return 0;
}

extern "C" int hyb_adamw_ema_set(double* ema_hyper, double decay, double warmup, void* stream) {
    HYB_CHECK_ARG(ema_hyper && decay >= 0.0 && decay < 1.0 && (warmup == 0.0 || warmup == 1.0));
    hipLaunchKernelGGL(ema_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ema_hyper, decay, warmup);
    HYB_LAUNCH_CHECK();
    return 0;
}

extern "C" int hyb_adamw_hyper_set_groups(double* hyper, double* ema_hyper, int groups, int count, const unsigned char* group, const double* values,
                                          int ema_count, const unsigned char* ema_group, const double* ema_values, void* stream) {
    HYB_CHECK_ARG(groups >= 1 && groups <= ADAM_GROUPS_MAX && count >= 0 && ema_count >= 0 && count + ema_count > 0 &&
                  (count == 0 || (hyper && group && values)) && (ema_count == 0 || (ema_hyper && ema_group && ema_values)));
    bool seen[ADAM_GROUPS_MAX] = {}, ema_seen[ADAM_GROUPS_MAX] = {};
    for (int i = 0; i < count; ++i) {
        const double* v = values + (long long)HYPER_N * i;          // the checks of hyb_adamw_hyper_set, and no group twice
        HYB_CHECK_ARG((int)group[i] < groups && !seen[group[i]] && v[0] >= 0.0 && v[1] >= 0.0 && v[1] < 1.0 && v[2] >= 0.0 && v[2] < 1.0 && v[3] >= 0.0 &&
                      v[4] >= 0.0 && v[5] == v[5]);
        seen[group[i]] = true;
    }
    for (int i = 0; i < ema_count; ++i) {
        const double* v = ema_values + 2ll * i;                     // the checks of hyb_adamw_ema_set
        HYB_CHECK_ARG((int)ema_group[i] < groups && !ema_seen[ema_group[i]] && v[0] >= 0.0 && v[0] < 1.0 && (v[1] == 0.0 || v[1] == 1.0));
        ema_seen[ema_group[i]] = true;
    }
    for (int first = 0; first < count || first < ema_count; first += HYPER_SET_MAX) {        // more than 60 rows of a block: more launches
        HyperSetArgs a{};
        a.hyper = hyper; a.ema_hyper = ema_hyper;
        a.n = count - first < 0 ? 0 : count - first < HYPER_SET_MAX ? count - first : HYPER_SET_MAX;
        a.ema_n = ema_count - first < 0 ? 0 : ema_count - first < HYPER_SET_MAX ? ema_count - first : HYPER_SET_MAX;
        for (int i = 0; i < a.n; ++i) {
            a.group[i] = group[first + i];
            for (int j = 0; j < HYPER_N; ++j) a.v[HYPER_N * i + j] = values[(long long)HYPER_N * (first + i) + j];
        }
        for (int i = 0; i < a.ema_n; ++i) {
            a.ema_group[i] = ema_group[first + i];
            a.ema_v[2 * i] = ema_values[2ll * (first + i)]; a.ema_v[2 * i + 1] = ema_values[2ll * (first + i) + 1];
        }
        hipLaunchKernelGGL(hyper_set_groups_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
        HYB_LAUNCH_CHECK();
    }
    return 0;
}

