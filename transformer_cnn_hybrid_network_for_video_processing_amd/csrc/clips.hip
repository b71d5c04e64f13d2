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
