// Clip augmentation on the device (DESIGN.md "Clip augmentation on the device"): crop, bilinear resize, horizontal flip, temporal
// sub-sampling, ToTensor and mean/std normalisation in the one kernel that expands a batch's uint8 HWC frames into the fp32
// [B,Tout,C,Ho,Wo] clip tensor.  One parameter row {y0, x0, ch, cw, flip, t0, tstride, 0} per CLIP, read from device memory: all
// frames of a clip get the same crop and flip, the launch takes no per-batch host value, and a captured launch replays with new rows.
//
// Sampling rule (include/hybrid_hip.h states it in full): source index and fraction from integer arithmetic -- for output row oy of a
// crop ch rows high, n = max((2 oy + 1) ch - Ho, 0), i0 = n / (2 Ho), frac = float(n % (2 Ho)) / float(2 Ho) -- which is
// F.interpolate(bilinear, align_corners=False, antialias=False) without a rounded coordinate; then two horizontal lerps, one vertical
// lerp, a DIVISION by 255 (ToTensor's arithmetic) and (x - mean) * (1/std).
//
// Access pattern: a lane owns VEC = 4 consecutive output pixels of one row (Wo % 4 == 0 and a 16-byte aligned dst; VEC = 1 otherwise)
// and writes them as one 16-byte store per channel plane, so a wave writes 1 KiB of consecutive floats per plane.  The four taps of a pixel
// are gathered straight from global memory as bytes: neighbouring lanes read neighbouring (down-scale: strided) bytes of the same two
// source rows, which the vector L1 serves; no LDS, no barrier.  blockIdx.x walks the (row, quad) positions of a frame, blockIdx.y the
// output frames, so the clip index, its parameter row and the clamps are wave-uniform.
#include "hyb_common.h"

namespace {
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (TWO COPIES OF THE RULE: this body and clip_row / clip_taps / clip_pixel below state the same clamps and the same arithmetic.  Calling the
// helpers from here changed this kernel's instruction schedule, and its instantiations are to stay as they were, so the body keeps its
// inline copy.  A change to a clamp or a rounding must be made in both places; tests/test_gpu_mix_transform.py (kind-0 rows and CutMix
// against this kernel with torch.equal) is what catches a copy that was forgotten.)
template <int VEC>
__global__ __launch_bounds__(256) void clips_u8_transform_kernel(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                                 const float* __restrict__ mean_invstd, float* __restrict__ dst, long long frames,
                                                                 int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo) {
    const int Wq = Wo / VEC;
    const unsigned pos = blockIdx.x * 256u + threadIdx.x;            // (oy, quad) inside a frame: Ho * Wq <= 2^28
    if (pos >= (unsigned)(Ho * Wq)) return;
    const int oy = (int)(pos / (unsigned)Wq), ox0 = ((int)pos - oy * Wq) * VEC;
    const long long frame_bytes = (long long)Hin * Win * C;
    for (long long f = blockIdx.y; f < frames; f += gridDim.y) {
        const long long b = f / Tout;
        const int t = (int)(f - b * Tout);
        const int* p = params + b * 8;
        // the rows come from device memory and were never seen by the host: clamp, so that no value reads outside src
        const int y0 = clampi(p[0], 0, Hin - 1), x0 = clampi(p[1], 0, Win - 1);
        const int ch = clampi(p[2], 1, Hin - y0), cw = clampi(p[3], 1, Win - x0);
        const bool flip = p[4] != 0;
        long long ts = (long long)p[5] + (long long)t * p[6];
        ts = ts < 0 ? 0 : (ts > Tin - 1 ? Tin - 1 : ts);
        const unsigned char* fb = src + (b * Tin + ts) * frame_bytes;

        // (every operand is non-negative after the max: unsigned division, the shorter sequence)
        const unsigned ny = (unsigned)max((2 * oy + 1) * ch - Ho, 0);               // <= 2 * 16384 * 16384 = 2^29
        const unsigned qy = ny / (2u * Ho), ry = ny - qy * (2u * Ho);
        const int iy0 = (int)qy, iy1 = min(iy0 + 1, ch - 1);
        const float fy = (float)ry / (float)(2 * Ho);
        const unsigned row0 = (unsigned)(((y0 + iy0) * Win + x0) * C), row1 = (unsigned)(((y0 + iy1) * Win + x0) * C);      // < 2^30: byte offsets inside one frame
        unsigned c0[VEC], c1[VEC];
        float fx[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int oxs = flip ? Wo - 1 - (ox0 + j) : ox0 + j;
            const unsigned nx = (unsigned)max((2 * oxs + 1) * cw - Wo, 0);
            const unsigned qx = nx / (2u * Wo), rx = nx - qx * (2u * Wo);
            const int ix0 = (int)qx, ix1 = min(ix0 + 1, cw - 1);
            fx[j] = (float)rx / (float)(2 * Wo);
            c0[j] = (unsigned)(ix0 * C);
            c1[j] = (unsigned)(ix1 * C);
        }
        float* out = dst + (f * C * Ho + oy) * (long long)Wo + ox0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= C) break;
            float v[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float a00 = (float)fb[row0 + c0[j] + c], a01 = (float)fb[row0 + c1[j] + c];
                const float a10 = (float)fb[row1 + c0[j] + c], a11 = (float)fb[row1 + c1[j] + c];
                const float top = a00 + fx[j] * (a01 - a00), bot = a10 + fx[j] * (a11 - a10);
                float o = (top + fy * (bot - top)) / 255.0f;         // ToTensor divides by 255 (not a multiply by 1/255)
                if (mean_invstd) o = (o - mean_invstd[c]) * mean_invstd[C + c];
                v[j] = o;
            }
            float* oc = out + (long long)c * Ho * Wo;
            if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(oc) = f32x4{v[0], v[1], v[2], v[3]};
            else oc[0] = v[0];
        }
    }
}

// ---- Mixup / CutMix (hyb_clips_u8_transform_mix).  The kernel above stays as it was written, instruction for instruction; the functions
// below restate its steps, expression for expression, for the kernel that needs them twice per pixel (own clip and partner) -- a second copy
// of the rule, see the note above clips_u8_transform_kernel: change both or neither.
// One clip's parameter row for output frame t as the kernel uses it: clamped (the rows come from device memory and were never seen by
// the host: no value reads outside src), with the address of the source frame.  Wave-uniform.
struct ClipRow { int y0, x0, ch, cw; bool flip; const unsigned char* fb; };
__device__ __forceinline__ ClipRow clip_row(const unsigned char* __restrict__ src, const int* __restrict__ params, long long b, int t, int Tin, int Hin,
                                            int Win, long long frame_bytes) {
    const int* p = params + b * 8;
    ClipRow r;
    r.y0 = clampi(p[0], 0, Hin - 1); r.x0 = clampi(p[1], 0, Win - 1);
    r.ch = clampi(p[2], 1, Hin - r.y0); r.cw = clampi(p[3], 1, Win - r.x0);
    r.flip = p[4] != 0;
    long long ts = (long long)p[5] + (long long)t * p[6];
    ts = ts < 0 ? 0 : (ts > Tin - 1 ? Tin - 1 : ts);
    r.fb = src + (b * Tin + ts) * frame_bytes;
    return r;
}
// The taps of a lane's VEC pixels (oy, ox0 .. ox0 + VEC - 1) in clip row r: byte offsets inside the frame and the two fractions
template <int VEC>
struct ClipTaps { unsigned row0, row1, c0[VEC], c1[VEC]; float fy, fx[VEC]; };
template <int VEC>
__device__ __forceinline__ ClipTaps<VEC> clip_taps(const ClipRow& r, int oy, int ox0, int Win, int C, int Ho, int Wo) {
    ClipTaps<VEC> k;
    // (every operand is non-negative after the max: unsigned division, the shorter sequence)
    const unsigned ny = (unsigned)max((2 * oy + 1) * r.ch - Ho, 0);               // <= 2 * 16384 * 16384 = 2^29
    const unsigned qy = ny / (2u * Ho), ry = ny - qy * (2u * Ho);
    const int iy0 = (int)qy, iy1 = min(iy0 + 1, r.ch - 1);
    k.fy = (float)ry / (float)(2 * Ho);
    k.row0 = (unsigned)(((r.y0 + iy0) * Win + r.x0) * C);                           // < 2^30: byte offsets inside one frame
    k.row1 = (unsigned)(((r.y0 + iy1) * Win + r.x0) * C);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const int oxs = r.flip ? Wo - 1 - (ox0 + j) : ox0 + j;
        const unsigned nx = (unsigned)max((2 * oxs + 1) * r.cw - Wo, 0);
        const unsigned qx = nx / (2u * Wo), rx = nx - qx * (2u * Wo);
        const int ix0 = (int)qx, ix1 = min(ix0 + 1, r.cw - 1);
        k.fx[j] = (float)rx / (float)(2 * Wo);
        k.c0[j] = (unsigned)(ix0 * C);
        k.c1[j] = (unsigned)(ix1 * C);
    }
    return k;
}
// One output value: four byte taps, two horizontal lerps, one vertical, ToTensor, Normalize
__device__ __forceinline__ float clip_pixel(const unsigned char* __restrict__ fb, unsigned row0, unsigned row1, unsigned c0, unsigned c1, float fx, float fy,
                                            int c, int C, const float* __restrict__ mean_invstd) {
    const float a00 = (float)fb[row0 + c0 + c], a01 = (float)fb[row0 + c1 + c];
    const float a10 = (float)fb[row1 + c0 + c], a11 = (float)fb[row1 + c1 + c];
    const float top = a00 + fx * (a01 - a00), bot = a10 + fx * (a11 - a10);
    float o = (top + fy * (bot - top)) / 255.0f;         // ToTensor divides by 255 (not a multiply by 1/255)
    if (mean_invstd) o = (o - mean_invstd[c]) * mean_invstd[C + c];
    return o;
}

// Mixup / CutMix in the same pass (include/hybrid_hip.h, hyb_clips_u8_transform_mix): one more row {partner, kind, by0, bx0, bh, bw, lam_bits, 0}
// per clip.  The clip index, the partner, the kind and the box are wave-uniform; only "is this pixel inside the box" varies per lane.
// kind 0 and CutMix do no arithmetic on the values: a pixel takes the taps of the ONE clip it comes from (selected per pixel, so a quad
// that straddles a box edge is right) and goes through clip_pixel once -- the bits of the plain kernel.  Mixup gathers both clips.
template <int VEC>
__global__ __launch_bounds__(256) void clips_u8_transform_mix_kernel(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                                     const int* __restrict__ mix, const float* __restrict__ mean_invstd,
                                                                     float* __restrict__ dst, long long frames, int B, int Tin, int Hin, int Win, int C,
                                                                     int Tout, int Ho, int Wo) {
    const int Wq = Wo / VEC;
    const unsigned pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= (unsigned)(Ho * Wq)) return;
    const int oy = (int)(pos / (unsigned)Wq), ox0 = ((int)pos - oy * Wq) * VEC;
    const long long frame_bytes = (long long)Hin * Win * C;
    for (long long f = blockIdx.y; f < frames; f += gridDim.y) {
        const long long b = f / Tout;
        const int t = (int)(f - b * Tout);
        const int* m = mix + b * 8;
        // the mix rows are clamped like the parameter rows: a kind outside 0..2 is 0, the partner is a clip of this batch, the box lies in the output
        int kind = m[1];
        if (kind < 0 || kind > 2) kind = 0;
        const ClipRow r = clip_row(src, params, b, t, Tin, Hin, Win, frame_bytes);
        const ClipTaps<VEC> k = clip_taps<VEC>(r, oy, ox0, Win, C, Ho, Wo);
        ClipRow pr = r;
        ClipTaps<VEC> pk = k;
        if (kind != 0) {                                         // (kind 0 does not read the partner)
            pr = clip_row(src, params, (long long)clampi(m[0], 0, B - 1), t, Tin, Hin, Win, frame_bytes);      // the partner's own row, temporal window included
            pk = clip_taps<VEC>(pr, oy, ox0, Win, C, Ho, Wo);
        }
        float lam = 1.f;
        bool in[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) in[j] = false;
        if (kind == 1) {
            lam = __int_as_float(m[6]);
            lam = !(lam <= 1.f) ? 1.f : (lam < 0.f ? 0.f : lam);        // into [0, 1]; a NaN counts as 1
        } else if (kind == 2) {
            const int by0 = clampi(m[2], 0, Ho), bx0 = clampi(m[3], 0, Wo);
            const int bh = clampi(m[4], 0, Ho - by0), bw = clampi(m[5], 0, Wo - bx0);
            const bool inrow = oy >= by0 && oy < by0 + bh;
#pragma unroll
            for (int j = 0; j < VEC; ++j) in[j] = inrow && ox0 + j >= bx0 && ox0 + j < bx0 + bw;
        }
        float* out = dst + (f * C * Ho + oy) * (long long)Wo + ox0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= C) break;
            float v[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if (kind == 1) {
                    const float own = clip_pixel(r.fb, k.row0, k.row1, k.c0[j], k.c1[j], k.fx[j], k.fy, c, C, mean_invstd);
                    const float oth = clip_pixel(pr.fb, pk.row0, pk.row1, pk.c0[j], pk.c1[j], pk.fx[j], pk.fy, c, C, mean_invstd);
                    v[j] = lam * own + (1.f - lam) * oth;
                } else {
                    const bool q = in[j];
                    v[j] = clip_pixel(q ? pr.fb : r.fb, q ? pk.row0 : k.row0, q ? pk.row1 : k.row1, q ? pk.c0[j] : k.c0[j], q ? pk.c1[j] : k.c1[j],
                                      q ? pk.fx[j] : k.fx[j], q ? pk.fy : k.fy, c, C, mean_invstd);
                }
            }
            float* oc = out + (long long)c * Ho * Wo;
            if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(oc) = f32x4{v[0], v[1], v[2], v[3]};
            else oc[0] = v[0];
        }
    }
}
}  // namespace

extern "C" int hyb_clips_u8_transform(const unsigned char* src, const int* params, const float* mean_invstd, float* dst, int B, int Tin, int Hin,
                                      int Win, int C, int Tout, int Ho, int Wo, void* stream) {
    HYB_CHECK_ARG(src && params && dst && B > 0 && Tin > 0 && Hin > 0 && Win > 0 && C > 0 && Tout > 0 && Ho > 0 && Wo > 0);
    HYB_CHECK_ARG(C <= 4 && Hin <= 16384 && Win <= 16384 && Ho <= 16384 && Wo <= 16384);      // the rule's integer products stay below 2^31
    const long long frames = (long long)B * Tout;
    const unsigned gy = (unsigned)(frames < 65535 ? frames : 65535);
    const bool vec = Wo % 4 == 0 && ((unsigned long long)dst & 15) == 0;
    const int per_frame = Ho * (vec ? Wo / 4 : Wo);
    const dim3 grid(hyb_cdiv(per_frame, 256), gy);
    if (vec)
        hipLaunchKernelGGL(clips_u8_transform_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, src, params, mean_invstd, dst, frames, Tin, Hin, Win,
                           C, Tout, Ho, Wo);
    else
        hipLaunchKernelGGL(clips_u8_transform_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, params, mean_invstd, dst, frames, Tin, Hin, Win,
                           C, Tout, Ho, Wo);
    HYB_LAUNCH_CHECK();
    return 0;
}

extern "C" int hyb_clips_u8_transform_mix(const unsigned char* src, const int* params, const int* mix, const float* mean_invstd, float* dst, int B, int Tin,
                                          int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream) {
    HYB_CHECK_ARG(src && params && mix && dst && B > 0 && Tin > 0 && Hin > 0 && Win > 0 && C > 0 && Tout > 0 && Ho > 0 && Wo > 0);
    HYB_CHECK_ARG(C <= 4 && Hin <= 16384 && Win <= 16384 && Ho <= 16384 && Wo <= 16384);
    const long long frames = (long long)B * Tout;
    const unsigned gy = (unsigned)(frames < 65535 ? frames : 65535);
    const bool vec = Wo % 4 == 0 && ((unsigned long long)dst & 15) == 0;
    const int per_frame = Ho * (vec ? Wo / 4 : Wo);
    const dim3 grid(hyb_cdiv(per_frame, 256), gy);
    if (vec)
        hipLaunchKernelGGL(clips_u8_transform_mix_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, src, params, mix, mean_invstd, dst, frames, B, Tin,
                           Hin, Win, C, Tout, Ho, Wo);
    else
        hipLaunchKernelGGL(clips_u8_transform_mix_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, params, mix, mean_invstd, dst, frames, B, Tin,
                           Hin, Win, C, Tout, Ho, Wo);
    HYB_LAUNCH_CHECK();
    return 0;
}
