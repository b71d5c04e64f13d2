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
//
// Four kernels share the rule: the plain kernel, the mix kernel (Mixup / CutMix), the photo kernel (colour jitter, noise, erasing) and the
// views kernel (V evaluation views of every source clip, hyb_clips_u8_transform_views); a fifth, the aug kernel (RandAugment's ops and a hue
// shift, hyb_clip_aug_u8_transform), puts an affine map in front of the rule and a program of pointwise steps behind it.  The plain, mix, photo and luma kernels are to keep
// their instruction schedules: a new variant is a new kernel built from clip_row / clip_taps / clip_pixel, not a change to one of them.
// The antialiased resize (hyb_clips_u8_transform_aa, the last kernel of the file) has a rule and an access pattern of its own: a separable
// triangle filter through LDS, with barriers.
//
// The host side is at the end of the file and is written once for the six transforms: an entry point fills a HybClipJob (kind, pointers,
// extents), hyb_clip_ok is the one validity rule -- a shared body and a table row per kind -- and hyb_clip_launch the one launch rule: frames,
// the 16-byte store condition, the grid and one switch over the kinds.  A new variant is a kind, a row in the check and a case in the launch.
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

// ---- Multi-view evaluation (hyb_clips_u8_transform_views): V parameter rows per SOURCE clip, output clip b * V + v from row b * V + v and the
// bytes of clip b.  The pixel is the plain kernel's, through the helpers above: one gather, clip_pixel once -- its bits.
// The walk over the B * V * Tout output frames is re-ordered: position g of the walk is (b, t, v) with v fastest, i.e. output frame
// (b * V + v) * Tout + t.  ClipTransform.sample_views orders a clip's rows window-major with crops and flips inside, so neighbouring v of one t
// are the crops of ONE temporal window: they read the same source frame, and workgroups dispatched one after the other find its bytes in the
// L2.  In output order the second reader of a source frame would come Tout frames of workgroups later.  Which frame a workgroup writes does not
// change what it writes; b, v, t and the row stay wave-uniform.
template <int VEC>
__global__ __launch_bounds__(256) void clips_u8_transform_views_kernel(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                                       const float* __restrict__ mean_invstd, float* __restrict__ dst,
                                                                       long long frames, int V, int Tin, int Hin, int Win, int C, int Tout, int Ho,
                                                                       int Wo) {
    const int Wq = Wo / VEC;
    const unsigned pos = blockIdx.x * 256u + threadIdx.x;            // (oy, quad) inside a frame: Ho * Wq <= 2^28
    if (pos >= (unsigned)(Ho * Wq)) return;
    const int oy = (int)(pos / (unsigned)Wq), ox0 = ((int)pos - oy * Wq) * VEC;
    const long long frame_bytes = (long long)Hin * Win * C;
    for (long long g = blockIdx.y; g < frames; g += gridDim.y) {
        const long long bt = g / V;
        const int v = (int)(g - bt * V);
        const long long b = bt / Tout;                               // the source clip
        const int t = (int)(bt - b * Tout);
        const long long row = b * V + v;                             // the output clip and its parameter row
        // clip_row reads row `b` of the rows it is given and frame (b, ts) of src: hand it the rows shifted so that its row b is row `row`
        const ClipRow r = clip_row(src, params + (row - b) * 8, b, t, Tin, Hin, Win, frame_bytes);
        const ClipTaps<VEC> k = clip_taps<VEC>(r, oy, ox0, Win, C, Ho, Wo);
        float* out = dst + ((row * Tout + t) * C * Ho + oy) * (long long)Wo + ox0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= C) break;
            float val[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) val[j] = clip_pixel(r.fb, k.row0, k.row1, k.c0[j], k.c1[j], k.fx[j], k.fy, c, C, mean_invstd);
            float* oc = out + (long long)c * Ho * Wo;
            if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(oc) = f32x4{val[0], val[1], val[2], val[3]};
            else oc[0] = val[0];
        }
    }
}

// ---- Photometric augmentation and erasing (hyb_clips_u8_transform_photo; include/hybrid_hip.h has the rule in full).  The two kernels above
// stay as they were written; clip_unit below is clip_pixel up to and including the division by 255 -- a THIRD copy of that arithmetic, see
// the note above clips_u8_transform_kernel: change all or none.  tests/test_gpu_photo.py (identity rows against both kernels above with
// torch.equal) is what catches a copy that was forgotten.
__device__ __forceinline__ float clip_unit(const unsigned char* __restrict__ fb, unsigned row0, unsigned row1, unsigned c0, unsigned c1, float fx, float fy,
                                           int c) {
    const float a00 = (float)fb[row0 + c0 + c], a01 = (float)fb[row0 + c1 + c];
    const float a10 = (float)fb[row1 + c0 + c], a11 = (float)fb[row1 + c1 + c];
    // The lerps a + f * (b - a) of the kernels above, as the compiler forms them there: one subtraction and one fused multiply-add each.  Here
    // the fusion is written out: with twelve values per lane in flight the vectoriser pairs some lerps and leaves others as a rounded product
    // and a rounded sum, and identity photo rows would no longer give those kernels' bits.
    const float top = fmaf(fx, a01 - a00, a00), bot = fmaf(fx, a11 - a10, a10);
    return fmaf(fy, bot - top, top) / 255.0f;            // ToTensor divides by 255 (not a multiply by 1/255)
}
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float photo_luma(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
// A jitter factor from its bits: !(f >= 0) (NaN included) is 1, values above 16 are 16
__device__ __forceinline__ float photo_factor(int bits) {
    const float f = __int_as_float(bits);
    return !(f >= 0.f) ? 1.f : (f > 16.f ? 16.f : f);
}
// One standard normal draw for element index idx: Box-Muller on two 24-bit uniforms of the project's counter hash; u1 in (0, 1], so the
// logarithm is finite and |z| <= sqrt(48 ln 2) = 5.77
__device__ __forceinline__ float photo_normal(unsigned long long seed, unsigned long long idx) {
    const float u1 = (float)((hyb_hash(seed, 2ull * idx) >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)(hyb_hash(seed, 2ull * idx + 1ull) >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);         // cos(2 pi u2) without a rounded angle and without cosf's large-argument path
}
// One clip's photo row as the kernel uses it: every field clamped (the host never saw it), the contrast pivot formed.  Wave-uniform.
// steps: the three colour ops in the row's order, two bits each (0 brightness, 1 contrast, 2 saturation), first op in the low bits.
struct PhotoRow { float fb, fc, fs, mu, sigma; int steps; bool gray; unsigned long long seed; int ey0, ex0, eh, ew, mode; };
__device__ __forceinline__ PhotoRow photo_row(const int* __restrict__ photo, const long long* __restrict__ luma_sums, long long b, const ClipRow& r,
                                              int Tout, int Ho, int Wo) {
    const int* q = photo + b * 16;
    PhotoRow h;
    h.fb = photo_factor(q[0]);
    h.fc = luma_sums ? photo_factor(q[1]) : 1.f;             // without the sums there is no pivot: the contrast factor counts as 1
    h.fs = photo_factor(q[2]);
    int order = q[3];
    if (order < 0 || order > 5) order = 0;
    // BCS, BSC, CBS, CSB, SBC, SCB
    h.steps = order == 0 ? 0x24 : order == 1 ? 0x18 : order == 2 ? 0x21 : order == 3 ? 0x09 : order == 4 ? 0x12 : 0x06;
    h.gray = q[4] != 0;
    const float s = __int_as_float(q[5]);
    h.sigma = !(s > 0.f) ? 0.f : (s > 1.f ? 1.f : s);
    h.seed = (unsigned long long)(unsigned)q[6] | ((unsigned long long)(unsigned)q[7] << 32);
    h.ey0 = clampi(q[8], 0, Ho); h.ex0 = clampi(q[9], 0, Wo);
    h.eh = clampi(q[10], 0, Ho - h.ey0); h.ew = clampi(q[11], 0, Wo - h.ex0);
    h.mode = q[12];
    if (h.mode < 0 || h.mode > 2) h.mode = 0;
    h.mu = 0.f;
    if (h.fc != 1.f) {
        // the pivot of the clip: the mean luma of the untouched source crop over the clip's Tout frames, exact integers until this division
        long long sum = 0;
        for (int t = 0; t < Tout; ++t) sum += luma_sums[b * Tout + t];
        float mu = (float)((double)sum / (10000.0 * 255.0 * (double)r.ch * (double)r.cw * (double)Tout));
        // brightness in front of contrast moves the pivot with the values
        const bool b_first = (h.steps & 3) == 0 || ((h.steps >> 2 & 3) == 0 && (h.steps & 3) != 1);
        if (b_first) mu = fminf(h.fb * mu, 1.f);
        h.mu = mu;
    }
    return h;
}
// Steps 1-6 of the rule for a lane's VEC pixels of output frame t, all C channels (C is 1 or 3): resample, jitter, gray, noise, normalise, erase
template <int VEC>
__device__ __forceinline__ void photo_values(float (&v)[3][VEC], const ClipRow& r, const ClipTaps<VEC>& k, const PhotoRow& h, int t, int oy, int ox0, int C,
                                             int Tout, int Ho, int Wo, const float* __restrict__ mean_invstd) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= C) break;
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[c][j] = clip_unit(r.fb, k.row0, k.row1, k.c0[j], k.c1[j], k.fx[j], k.fy, c);
    }
#pragma unroll
    for (int step = 0; step < 3; ++step) {
        const int op = h.steps >> (2 * step) & 3;
        if (op == 0) {
            if (h.fb != 1.f) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c >= C) break;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(h.fb * v[c][j]);
                }
            }
        } else if (op == 1) {
            if (h.fc != 1.f) {
                const float add = (1.f - h.fc) * h.mu;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c >= C) break;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(h.fc * v[c][j] + add);
                }
            }
        } else if (h.fs != 1.f && C == 3) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float add = (1.f - h.fs) * photo_luma(v[0][j], v[1][j], v[2][j]);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][j] = clamp01(h.fs * v[c][j] + add);
            }
        }
    }
    if (h.gray && C == 3) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[0][j] = v[1][j] = v[2][j] = photo_luma(v[0][j], v[1][j], v[2][j]);
    }
    const unsigned long long plane = (unsigned long long)Ho * Wo;
    if (h.sigma != 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            const unsigned long long e0 = ((unsigned long long)(t * C + c) * Ho + oy) * Wo + ox0;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(v[c][j] + h.sigma * photo_normal(h.seed, e0 + j));
        }
    }
    if (mean_invstd) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[c][j] = (v[c][j] - mean_invstd[c]) * mean_invstd[C + c];
        }
    }
    if (oy >= h.ey0 && oy < h.ey0 + h.eh && h.ew > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            const unsigned long long e0 = ((unsigned long long)(t * C + c) * Ho + oy) * Wo + ox0 + (unsigned long long)Tout * C * plane;
            const float black = mean_invstd ? (0.f - mean_invstd[c]) * mean_invstd[C + c] : 0.f;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if (ox0 + j >= h.ex0 && ox0 + j < h.ex0 + h.ew) v[c][j] = h.mode == 0 ? 0.f : (h.mode == 1 ? black : photo_normal(h.seed, e0 + j));
            }
        }
    }
}

// Mixup's blend as clips_u8_transform_mix_kernel compiles it: two rounded products and a rounded sum.  There the compiler forms the products as
// one packed multiply and does not fuse; here, with other code around the expression, it would fuse one of them into an fma, and identity photo
// rows would no longer give that kernel's bits (tests/test_gpu_photo.py holds the two together with torch.equal).
__device__ __forceinline__ float mixup_blend(float lam, float own, float oth) {
#pragma clang fp contract(off)
    return lam * own + (1.f - lam) * oth;
}

// blockIdx.x walks the (row, quad) positions of a frame, blockIdx.y the frames: the clip, its three rows, the partner's, the factors, the
// order, the box and the seed are wave-uniform, and an op whose factor is exactly 1 is skipped by a scalar branch.  All C channels of a pixel
// are formed together (the luma needs them), then written as one 16-byte store per channel plane like the kernels above.
template <int VEC>
__global__ __launch_bounds__(256) void clips_u8_transform_photo_kernel(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                                       const int* __restrict__ mix, const int* __restrict__ photo,
                                                                       const long long* __restrict__ luma_sums, const float* __restrict__ mean_invstd,
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
        int kind = 0;
        const int* m = mix ? mix + b * 8 : nullptr;
        if (m) kind = m[1];
        if (kind < 0 || kind > 2) kind = 0;
        float lam = 1.f;
        bool own_needed = true, oth_needed = false, in[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) in[j] = false;
        if (kind == 1) {
            lam = __int_as_float(m[6]);
            lam = !(lam <= 1.f) ? 1.f : (lam < 0.f ? 0.f : lam);        // into [0, 1]; a NaN counts as 1
            oth_needed = true;
        } else if (kind == 2) {
            const int by0 = clampi(m[2], 0, Ho), bx0 = clampi(m[3], 0, Wo);
            const int bh = clampi(m[4], 0, Ho - by0), bw = clampi(m[5], 0, Wo - bx0);
            const bool inrow = oy >= by0 && oy < by0 + bh;
            own_needed = false;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                in[j] = inrow && ox0 + j >= bx0 && ox0 + j < bx0 + bw;
                oth_needed |= in[j];
                own_needed |= !in[j];
            }
        }
        // ONE copy of the chain's instructions serves the clip and its partner (a loop that is not unrolled): a partner's pixel has the bits the
        // partner's own launch position would have written, which is what makes a CutMix composite exact.  A quad wholly inside a CutMix box
        // gathers only the partner, one wholly outside only its own clip.  res holds the clip's own value after side 0 and the mixed one after side 1.
        float res[3][VEC];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) res[c][j] = 0.f;
        }
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            if (!(side == 0 ? own_needed : oth_needed)) continue;
            const long long sb = side == 0 ? b : (long long)clampi(m[0], 0, B - 1);      // the partner's own params and photo rows
            const ClipRow r = clip_row(src, params, sb, t, Tin, Hin, Win, frame_bytes);
            const PhotoRow h = photo_row(photo, luma_sums, sb, r, Tout, Ho, Wo);
            const ClipTaps<VEC> k = clip_taps<VEC>(r, oy, ox0, Win, C, Ho, Wo);
            float cur[3][VEC];
            photo_values<VEC>(cur, r, k, h, t, oy, ox0, C, Tout, Ho, Wo, mean_invstd);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= C) break;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (side == 0) res[c][j] = cur[c][j];
                    else if (kind == 1) res[c][j] = mixup_blend(lam, res[c][j], cur[c][j]);
                    else if (in[j]) res[c][j] = cur[c][j];
                }
            }
        }
        float* out = dst + (f * C * Ho + oy) * (long long)Wo + ox0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            float* oc = out + (long long)c * Ho * Wo;
            if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(oc) = f32x4{res[c][0], res[c][1], res[c][2], res[c][3]};
            else oc[0] = res[c][0];
        }
    }
}

// ---- RandAugment's ops and a hue shift (hyb_clip_aug_u8_transform; include/hybrid_hip.h has the rule in full): one more int32 row of 32 per clip,
// {flags, n, (op, arg) x 8, M[6], fill[3], 0 x 5}.  The kernels above stay as they were written, so photo_values is not touched: aug_photo_tail
// below is its steps 2-6 once more -- a further copy of that arithmetic, see the note above clips_u8_transform_kernel: change all or none.
// tests/test_gpu_randaug.py (identity aug rows against the photo kernel with torch.equal) is what catches a copy that was forgotten.
// The identity photo row, for photo == NULL
__device__ __forceinline__ PhotoRow photo_identity() {
    PhotoRow h;
    h.fb = h.fc = h.fs = 1.f; h.mu = 0.f; h.sigma = 0.f; h.steps = 0x24; h.gray = false; h.seed = 0ull;
    h.ey0 = h.ex0 = h.eh = h.ew = 0; h.mode = 0;
    return h;
}
__device__ __forceinline__ bool aug_finite(int bits) { return (bits & 0x7f800000) != 0x7f800000; }
// The geometry of one aug row: on only with the flag and a finite M.  Wave-uniform.
struct AugGeo { bool on; float m[6], fill[3]; };
__device__ __forceinline__ AugGeo aug_geo(const int* __restrict__ a) {
    AugGeo g;
    g.on = (a[0] & 1) != 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        g.on = g.on && aug_finite(a[18 + i]);
        g.m[i] = __int_as_float(a[18 + i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float f = __int_as_float(a[24 + i]);
        g.fill[i] = !(f >= 0.f) ? 0.f : (f > 1.f ? 1.f : f);
    }
    return g;
}
// Step 1 with the geometry: output pixel -> point of the un-augmented output frame -> point of the crop, ONE bilinear gather there.  The
// coordinates are per lane and per pixel: the VEC pixels of a lane share neither row taps nor the in / out test.  Every operation is rounded as
// written (tests/randaug_ref.py restates them one by one in fp32); the fused ones are written as fmaf.
template <int VEC>
__device__ __forceinline__ void aug_resample(float (&v)[3][VEC], const ClipRow& r, const AugGeo& g, int oy, int ox0, int Win, int C, int Ho, int Wo) {
#pragma clang fp contract(off)
    const float yc = (float)oy + 0.5f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const float xc = (float)(ox0 + j) + 0.5f;
        float x = fmaf(g.m[0], xc, fmaf(g.m[1], yc, g.m[2]));
        const float y = fmaf(g.m[3], xc, fmaf(g.m[4], yc, g.m[5]));
        if (!(x >= 0.f && x < (float)Wo && y >= 0.f && y < (float)Ho)) {      // a NaN is outside
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = g.fill[c];
            continue;
        }
        if (r.flip) x = (float)Wo - x;
        const float sx = (x * (float)r.cw) / (float)Wo - 0.5f, sy = (y * (float)r.ch) / (float)Ho - 0.5f;      // in [-1/2, cw - 1/2] and [-1/2, ch - 1/2)
        const float flx = floorf(sx), fly = floorf(sy);
        const float fx = sx - flx, fy = sy - fly;
        // the taps are clamped into the crop whatever the coordinates were: no value reads outside src
        const int ix = clampi((int)flx, -1, r.cw), iy = clampi((int)fly, -1, r.ch);
        const int ix0 = clampi(ix, 0, r.cw - 1), ix1 = clampi(ix + 1, 0, r.cw - 1);
        const int iy0 = clampi(iy, 0, r.ch - 1), iy1 = clampi(iy + 1, 0, r.ch - 1);
        const unsigned row0 = (unsigned)(((r.y0 + iy0) * Win + r.x0) * C), row1 = (unsigned)(((r.y0 + iy1) * Win + r.x0) * C);      // < 2^30, as in clip_taps
        const unsigned c0 = (unsigned)(ix0 * C), c1 = (unsigned)(ix1 * C);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            v[c][j] = clip_unit(r.fb, row0, row1, c0, c1, fx, fy, c);
        }
    }
}
// The byte of a value in [0, 1]: floor(255 v + 1/2)
__device__ __forceinline__ int aug_byte(float v) { return (int)floorf(255.f * v + 0.5f); }
// torchvision's adjust_hue on one pixel (_rgb2hsv, h <- (h + shift) mod 1, _hsv2rgb), every operation rounded, none fused
__device__ __forceinline__ void aug_hue(float& r, float& g, float& b, float shift) {
#pragma clang fp contract(off)
    const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
    const float cr = mx - mn;
    const bool eq = mx == mn;
    const float s = cr / (eq ? 1.f : mx), d = eq ? 1.f : cr;
    const float rc = (mx - r) / d, gc = (mx - g) / d, bc = (mx - b) / d;
    float hh = mx == r ? bc - gc : (mx == g ? 2.f + rc - bc : 4.f + gc - rc);
    hh = hh / 6.f + 1.f;
    hh = hh - floorf(hh);
    hh = hh + shift;
    hh = hh - floorf(hh);
    const float h6 = hh * 6.f, fl = floorf(h6), f = h6 - fl;
    int i = (int)fl;
    i = i >= 6 ? i - 6 : i;
    const float p = clamp01(mx * (1.f - s)), q = clamp01(mx * (1.f - s * f)), t = clamp01(mx * (1.f - s * (1.f - f)));
    r = i == 0 ? mx : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : mx))));
    g = i == 0 ? t : (i == 1 ? mx : (i == 2 ? mx : (i == 3 ? q : p)));
    b = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? mx : (i == 4 ? mx : q))));
}
// Step 1a: the row's program on a lane's VEC pixels.  The steps are read from the row as they are run (scalar loads, scalar branches).
template <int VEC>
__device__ __forceinline__ void aug_program(float (&v)[3][VEC], const int* __restrict__ a, const long long* __restrict__ luma_sums, long long b,
                                            const ClipRow& r, int C, int Tout) {
    const int n = clampi(a[1], 0, 8);
    bool need_mu = false;
    for (int s = 0; s < n; ++s) need_mu |= a[2 + 2 * s] == 3 && luma_sums && photo_factor(a[3 + 2 * s]) != 1.f;
    float mu = 0.f;
    if (need_mu) {
        // the clip's mean luma as photo_row forms it
        long long sum = 0;
        for (int t = 0; t < Tout; ++t) sum += luma_sums[b * Tout + t];
        mu = (float)((double)sum / (10000.0 * 255.0 * (double)r.ch * (double)r.cw * (double)Tout));
    }
#pragma unroll 1
    for (int s = 0; s < n; ++s) {
        const int op = a[2 + 2 * s], arg = a[3 + 2 * s];
        if (op == 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= C) break;
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[c][j] = 1.f - v[c][j];
            }
            mu = 1.f - mu;
        } else if (op == 2) {
            const float f = photo_factor(arg);
            if (f != 1.f) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c >= C) break;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(f * v[c][j]);
                }
            }
            mu = fminf(f * mu, 1.f);
        } else if (op == 3) {
            const float f = luma_sums ? photo_factor(arg) : 1.f;
            if (f != 1.f) {
                const float add = (1.f - f) * mu;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c >= C) break;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(f * v[c][j] + add);
                }
            }
        } else if (op == 4) {
            const float f = photo_factor(arg);
            if (f != 1.f && C == 3) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float add = (1.f - f) * photo_luma(v[0][j], v[1][j], v[2][j]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c][j] = clamp01(f * v[c][j] + add);
                }
            }
        } else if (op == 5) {
            const int mask = ~((1 << (8 - clampi(arg, 0, 8))) - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= C) break;
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[c][j] = (float)(aug_byte(v[c][j]) & mask) / 255.0f;
            }
        } else if (op == 6) {
            const int thr = clampi(arg, 0, 256);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= C) break;
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[c][j] = aug_byte(v[c][j]) >= thr ? 1.f - v[c][j] : v[c][j];
            }
        } else if (op == 7) {
            const float add = (float)clampi(arg, 0, 255) / 255.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= C) break;
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[c][j] = aug_byte(v[c][j]) < 128 ? fminf(1.f, v[c][j] + add) : v[c][j];
            }
        } else if (op == 8) {
            float h = __int_as_float(arg);
            h = !(h == h) ? 0.f : fminf(fmaxf(h, -0.5f), 0.5f);
            if (h != 0.f && C == 3) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) aug_hue(v[0][j], v[1][j], v[2][j], h);
            }
        }
    }
}
// Steps 2-6 of the photo rule on values that are already resampled: photo_values from its first jitter step on, expression for expression
template <int VEC>
__device__ __forceinline__ void aug_photo_tail(float (&v)[3][VEC], const PhotoRow& h, int t, int oy, int ox0, int C, int Tout, int Ho, int Wo,
                                               const float* __restrict__ mean_invstd) {
#pragma unroll
    for (int step = 0; step < 3; ++step) {
        const int op = h.steps >> (2 * step) & 3;
        if (op == 0) {
            if (h.fb != 1.f) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c >= C) break;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(h.fb * v[c][j]);
                }
            }
        } else if (op == 1) {
            if (h.fc != 1.f) {
                const float add = (1.f - h.fc) * h.mu;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c >= C) break;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(h.fc * v[c][j] + add);
                }
            }
        } else if (h.fs != 1.f && C == 3) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float add = (1.f - h.fs) * photo_luma(v[0][j], v[1][j], v[2][j]);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][j] = clamp01(h.fs * v[c][j] + add);
            }
        }
    }
    if (h.gray && C == 3) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[0][j] = v[1][j] = v[2][j] = photo_luma(v[0][j], v[1][j], v[2][j]);
    }
    const unsigned long long plane = (unsigned long long)Ho * Wo;
    if (h.sigma != 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            const unsigned long long e0 = ((unsigned long long)(t * C + c) * Ho + oy) * Wo + ox0;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[c][j] = clamp01(v[c][j] + h.sigma * photo_normal(h.seed, e0 + j));
        }
    }
    if (mean_invstd) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[c][j] = (v[c][j] - mean_invstd[c]) * mean_invstd[C + c];
        }
    }
    if (oy >= h.ey0 && oy < h.ey0 + h.eh && h.ew > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            const unsigned long long e0 = ((unsigned long long)(t * C + c) * Ho + oy) * Wo + ox0 + (unsigned long long)Tout * C * plane;
            const float black = mean_invstd ? (0.f - mean_invstd[c]) * mean_invstd[C + c] : 0.f;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if (ox0 + j >= h.ex0 && ox0 + j < h.ex0 + h.ew) v[c][j] = h.mode == 0 ? 0.f : (h.mode == 1 ? black : photo_normal(h.seed, e0 + j));
            }
        }
    }
}

// The photo kernel's grid, its stores and its two-sided mix loop; the clip, its four rows, the program and M are wave-uniform, the program's steps
// and "geometry or integer taps" are scalar branches, and only the coordinates and the in / out test of the geometry vary per lane.
template <int VEC>
__global__ __launch_bounds__(256) void clips_u8_transform_aug_kernel(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                                     const int* __restrict__ mix, const int* __restrict__ photo,
                                                                     const int* __restrict__ aug, const long long* __restrict__ luma_sums,
                                                                     const float* __restrict__ mean_invstd, float* __restrict__ dst, long long frames,
                                                                     int B, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo) {
    const int Wq = Wo / VEC;
    const unsigned pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= (unsigned)(Ho * Wq)) return;
    const int oy = (int)(pos / (unsigned)Wq), ox0 = ((int)pos - oy * Wq) * VEC;
    const long long frame_bytes = (long long)Hin * Win * C;
    for (long long f = blockIdx.y; f < frames; f += gridDim.y) {
        const long long b = f / Tout;
        const int t = (int)(f - b * Tout);
        int kind = 0;
        const int* m = mix ? mix + b * 8 : nullptr;
        if (m) kind = m[1];
        if (kind < 0 || kind > 2) kind = 0;
        float lam = 1.f;
        bool own_needed = true, oth_needed = false, in[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) in[j] = false;
        if (kind == 1) {
            lam = __int_as_float(m[6]);
            lam = !(lam <= 1.f) ? 1.f : (lam < 0.f ? 0.f : lam);        // into [0, 1]; a NaN counts as 1
            oth_needed = true;
        } else if (kind == 2) {
            const int by0 = clampi(m[2], 0, Ho), bx0 = clampi(m[3], 0, Wo);
            const int bh = clampi(m[4], 0, Ho - by0), bw = clampi(m[5], 0, Wo - bx0);
            const bool inrow = oy >= by0 && oy < by0 + bh;
            own_needed = false;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                in[j] = inrow && ox0 + j >= bx0 && ox0 + j < bx0 + bw;
                oth_needed |= in[j];
                own_needed |= !in[j];
            }
        }
        // (the photo kernel's loop: one copy of the chain's instructions serves the clip and its partner)
        float res[3][VEC];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) res[c][j] = 0.f;
        }
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            if (!(side == 0 ? own_needed : oth_needed)) continue;
            const long long sb = side == 0 ? b : (long long)clampi(m[0], 0, B - 1);      // the partner's own params, aug and photo rows
            const ClipRow r = clip_row(src, params, sb, t, Tin, Hin, Win, frame_bytes);
            const PhotoRow h = photo ? photo_row(photo, luma_sums, sb, r, Tout, Ho, Wo) : photo_identity();
            const int* a = aug + sb * 32;
            const AugGeo g = aug_geo(a);
            float cur[3][VEC];
            if (g.on) {
                aug_resample<VEC>(cur, r, g, oy, ox0, Win, C, Ho, Wo);
            } else {
                const ClipTaps<VEC> k = clip_taps<VEC>(r, oy, ox0, Win, C, Ho, Wo);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c >= C) break;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) cur[c][j] = clip_unit(r.fb, k.row0, k.row1, k.c0[j], k.c1[j], k.fx[j], k.fy, c);
                }
            }
            aug_program<VEC>(cur, a, luma_sums, sb, r, C, Tout);
            aug_photo_tail<VEC>(cur, h, t, oy, ox0, C, Tout, Ho, Wo, mean_invstd);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= C) break;
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (side == 0) res[c][j] = cur[c][j];
                    else if (kind == 1) res[c][j] = mixup_blend(lam, res[c][j], cur[c][j]);
                    else if (in[j]) res[c][j] = cur[c][j];
                }
            }
        }
        float* out = dst + (f * C * Ho + oy) * (long long)Wo + ox0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= C) break;
            float* oc = out + (long long)c * Ho * Wo;
            if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(oc) = f32x4{res[c][0], res[c][1], res[c][2], res[c][3]};
            else oc[0] = res[c][0];
        }
    }
}

// ---- hyb_clips_u8_luma_sums: the integer luma sum of every output frame's source crop, for the contrast pivot.  blockIdx.y is the output
// frame, the blockIdx.x workgroups of a frame take its crop rows in turn.  A row is a run of cw * C consecutive bytes: its 16-byte aligned
// middle is read as 16-byte loads, one per lane, the up to 15 bytes in front of and behind it one byte per lane.  For C == 3 a chunk's bytes are
// summed by position mod 3 and the three sums go to the channels by the chunk's phase in the row.  Integer arithmetic and integer atomics: the
// result is exact whatever the order; the launch function zeroes sums in front of the kernel.
constexpr int LUMA_SPLIT_ROWS = 32;                                     // crop rows of a frame per workgroup, at most (Hin / split)
__global__ __launch_bounds__(256) void clips_u8_luma_sums_kernel(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                                 unsigned long long* __restrict__ sums, long long frames, int Tin, int Hin, int Win, int C,
                                                                 int Tout) {
    __shared__ unsigned long long red[4];
    const long long frame_bytes = (long long)Hin * Win * C;
    const int tid = threadIdx.x;
    for (long long f = blockIdx.y; f < frames; f += gridDim.y) {
        const long long b = f / Tout;
        const int t = (int)(f - b * Tout);
        const ClipRow r = clip_row(src, params, b, t, Tin, Hin, Win, frame_bytes);
        const int n = r.cw * C;                                          // bytes of a crop row
        unsigned long long ch_sum[3] = {0, 0, 0};                        // C == 1: everything in [0]
        for (int y = blockIdx.x; y < r.ch; y += gridDim.x) {
            const unsigned char* row = r.fb + ((long long)(r.y0 + y) * Win + r.x0) * C;
            const int head = min((int)((16u - (unsigned)((unsigned long long)row & 15u)) & 15u), n);
            const int nchunks = (n - head) >> 4, tail_at = head + (nchunks << 4);
            for (int i = tid; i < nchunks; i += 256) {
                const int at = head + (i << 4);
                const uint4 q = *reinterpret_cast<const uint4*>(row + at);
                const unsigned w[4] = {q.x, q.y, q.z, q.w};
                unsigned s[3] = {0, 0, 0};
#pragma unroll
                for (int j = 0; j < 16; ++j) s[j % 3] += (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                if (C == 1) {
                    ch_sum[0] += s[0] + s[1] + s[2];
                } else {
                    const int p = at % 3;                                // channel of the chunk's first byte
                    ch_sum[0] += p == 0 ? s[0] : (p == 1 ? s[2] : s[1]);
                    ch_sum[1] += p == 0 ? s[1] : (p == 1 ? s[0] : s[2]);
                    ch_sum[2] += p == 0 ? s[2] : (p == 1 ? s[1] : s[0]);
                }
            }
            if (tid < head + (n - tail_at)) {
                const int at = tid < head ? tid : tail_at + (tid - head);
                const unsigned val = row[at];
                if (C == 1) ch_sum[0] += val;
                else {
                    const int c = at % 3;
                    ch_sum[0] += c == 0 ? val : 0u;
                    ch_sum[1] += c == 1 ? val : 0u;
                    ch_sum[2] += c == 2 ? val : 0u;
                }
            }
        }
        unsigned long long tot = C == 1 ? 10000ull * ch_sum[0] : 2989ull * ch_sum[0] + 5870ull * ch_sum[1] + 1140ull * ch_sum[2];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) tot += __shfl_down(tot, d, 64);
        if ((tid & 63) == 0) red[tid >> 6] = tot;
        __syncthreads();
        if (tid == 0) {
            const unsigned long long all = red[0] + red[1] + red[2] + red[3];
            if (all) atomicAdd(sums + f, all);
        }
        __syncthreads();
    }
}
}  // namespace

// ---- Antialiased resize (hyb_clips_u8_transform_aa; include/hybrid_hip.h has the rule in full): torchvision's Resize(antialias=True), i.e.
// F.interpolate(bilinear, align_corners=False, antialias=True).  The kernels above stay as they were written; this one takes clip_row (the clamps,
// the temporal index, the flip) and the views kernel's frame walk from them and nothing else.  Per axis, n crop positions -> m output positions:
//   D = 2 max(n, m);   W(i, k) = max(0, D - |(2k + 1) m - (2i + 1) n|);   S(i) = sum_k W(i, k)          all int32 (<= 2 * 16384^2)
//   out = sum_ky sum_kx (Wy / Sy) (Wx / Sx) a[ky][kx], then / 255 and (x - mean) * invstd as clip_pixel writes them
// A weight is the correctly rounded QUOTIENT float(W) / float(S) of two integers (W <= 2^15 is exact in fp32): 1.0f for the single tap of an
// identity axis and 1/8, 3/8 for n == 2m, so identity rows give the plain kernel's bits and a 2 x down-scale is exact (tests/test_gpu_antialias.py).
// The filter is separable and a down-scale by s has about 2s taps per axis, so the pixels are NOT gathered (4 s^2 bytes each).  A workgroup owns
// AA_TH x TW output pixels of one output frame (TW = AA_QW * VEC) and walks the source rows its tile needs -- a workgroup-uniform span from the
// integer rule, about (AA_TH + 2) n / m rows -- in chunks of AA_R rows:
//   phase 1  lane = (output column, row group): the taps of a column are count * C contiguous bytes of an HWC row; the lane forms each weight once
//            and uses it for its AA_R / RG rows of the chunk, C fp32 sums per row, written to LDS as [row][c][column]
//   barrier
//   phase 2  lane = (output row, VEC columns): adds wy(row) * LDS[row][c][columns] for the chunk rows inside its row's window into VEC x C
//            registers; neighbouring lanes read neighbouring 16 bytes
//   barrier  (the next chunk's, or the next frame's, phase 1 overwrites the LDS)
// LDS is AA_R * 4 * TW * 4 B = 32 KiB (VEC = 4) whatever the scale.  Why LDS: the horizontal sums of a source row are shared by every output row
// whose window holds it (2 for an up-scale, 2 n / m otherwise), and those rows belong to different lanes.
// NO lane returns before the last barrier: lanes outside a partial tile stay in every loop and skip their loads and stores.  The frame loop and the
// chunk loop are bounded by blockIdx, the clip's row and the extents only -- workgroup-uniform.
constexpr int AA_TH = 32;            // output rows of a tile
constexpr int AA_QW = 8;             // lanes along a tile's output row: AA_TH * AA_QW = 256, the tile is AA_QW * VEC columns wide
constexpr int AA_R = 64;             // source rows of a chunk
static_assert(AA_TH * AA_QW == 256, "one lane per (output row, VEC columns) of a tile");

namespace {
// The window of output position i: the source positions k with W(i, k) > 0, clipped to [0, n - 1].  Never empty: the open interval of half-width
// D / (2m) >= 1 around the centre (2i + 1) n / (2m) - 1/2, which lies in (-1/2, n - 1/2), holds the integer next to the centre.
__device__ __forceinline__ int aa_lo(int i, int n, int m, int D) {
    const int num = (2 * i + 1) * n - D - m;                         // k > num / (2m)
    return num < 0 ? 0 : (int)((unsigned)num / (2u * m)) + 1;
}
__device__ __forceinline__ int aa_hi(int i, int n, int m, int D) {
    const unsigned num = (unsigned)((2 * i + 1) * n + D - m - 1);    // k < (num + 1) / (2m); positive: D >= 2m
    return min((int)(num / (2u * m)), n - 1);
}
// W(i, k) with ci = (2i + 1) n; positive for every k of the window
__device__ __forceinline__ int aa_weight(int k, int m, int ci, int D) {
    const int v = (2 * k + 1) * m - ci;
    return D - (v < 0 ? -v : v);
}
__device__ __forceinline__ int aa_sum(int lo, int hi, int m, int ci, int D) {
    int s = 0;
    for (int k = lo; k <= hi; ++k) s += aa_weight(k, m, ci, D);
    return s;
}

// Phase 1 for one lane: the horizontal sums h[j][c] of its RPL chunk rows (row j at byte offset ro[j] from the crop's origin, inside the tile's span
// while RG * j < nrows) over the taps kx_lo .. kx_hi of its output column, a crop row being n positions wide.  The taps of a column are contiguous
// bytes of a row.  They are read in groups of TG whole positions = G 32-bit words (CC = 3: 4 positions in 3 words) at the bytes' own, in general
// unaligned, address.  The groups start at kx_lo, or further left where they would otherwise pass the end of the crop's row: every byte read is a
// byte of the crop.  A position of a group outside the window has the rule's weight max(0, .) = 0, and fmaf(0, a, h) is h, bit for bit: every sum
// is the fmaf chain over the window in ascending k.  A crop narrower than the groups is read one byte at a time.
template <int CC, int RPL, int RG>
__device__ __forceinline__ void aa_hsums(float (&h)[RPL][4], const unsigned char* __restrict__ crop, const unsigned (&ro)[RPL], int nrows, int kx_lo,
                                         int kx_hi, int n, int m, int cx, int D, float sx) {
    constexpr int TG = CC == 3 ? 4 : 4 / CC, G = TG * CC / 4;
    const int ng = (kx_hi - kx_lo + TG) / TG;                         // groups that cover the window
    int k = min(kx_lo, n - ng * TG);                                   // ... moved left where they would leave the crop's row
    const int k_end = k < 0 ? kx_lo : k + ng * TG;                     // a crop narrower than the groups: every tap by bytes
    if (k < 0) k = kx_lo;
    for (; k < k_end; k += TG) {
        float w[TG];
#pragma unroll
        for (int i = 0; i < TG; ++i) w[i] = (float)max(aa_weight(k + i, m, cx, D), 0) / sx;      // a quotient, not a product with 1 / sx: 1.0f stays 1.0f
        const unsigned ko = (unsigned)(k * CC);
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            if (RG * j >= nrows) continue;                             // past the tile's span (and possibly past the crop): not read
            unsigned d[G];
            __builtin_memcpy(d, crop + ro[j] + ko, 4 * G);
#pragma unroll
            for (int i = 0; i < TG * CC; ++i) h[j][i % CC] = fmaf(w[i / CC], (float)((d[i >> 2] >> (8 * (i & 3))) & 0xffu), h[j][i % CC]);
        }
    }
    for (; k <= kx_hi; ++k) {
        const float w = (float)aa_weight(k, m, cx, D) / sx;
        const unsigned ko = (unsigned)(k * CC);
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            if (RG * j >= nrows) continue;
#pragma unroll
            for (int c = 0; c < CC; ++c) h[j][c] = fmaf(w, (float)crop[ro[j] + ko + c], h[j][c]);
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void clips_u8_transform_aa_kernel(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                                    const float* __restrict__ mean_invstd, float* __restrict__ dst, long long frames,
                                                                    int V, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo) {
    constexpr int TW = AA_QW * VEC;          // output columns of a tile
    constexpr int RG = 256 / TW;             // phase 1: lanes per column, each takes the chunk rows rg, rg + RG, ...
    constexpr int RPL = AA_R / RG;           // ... RPL of them
    static_assert(RG * TW == 256 && RPL * RG == AA_R, "phase 1 covers the chunk exactly");
    __shared__ __attribute__((aligned(16))) float hsum[AA_R * 4 * TW];      // [row][c][column]
    const int tid = threadIdx.x;
    const int tiles_x = (Wo + TW - 1) / TW;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)blockIdx.x - ty * tiles_x;
    const int oy_first = ty * AA_TH, oy_last = min(oy_first + AA_TH, Ho) - 1;      // the tile's output rows: workgroup-uniform
    // phase 2 and the store: this lane's output row and VEC columns
    const int oxl = (tid % AA_QW) * VEC, oy = oy_first + tid / AA_QW, ox0 = tx * TW + oxl;
    const bool out_ok = oy < Ho && ox0 < Wo;                                       // (VEC == 4 only with Wo % 4 == 0: the whole quad is inside)
    // phase 1: this lane's output column and row group
    const int col = tid % TW, rg = tid / TW, oxc = tx * TW + col;
    const bool col_ok = oxc < Wo;
    const long long frame_bytes = (long long)Hin * Win * C;
    for (long long g = blockIdx.y; g < frames; g += gridDim.y) {
        // the views kernel's walk: position g is (b, t, v) with v fastest
        const long long bt = g / V;
        const int v = (int)(g - bt * V);
        const long long b = bt / Tout;
        const int t = (int)(bt - b * Tout);
        const long long row = b * V + v;
        const ClipRow r = clip_row(src, params + (row - b) * 8, b, t, Tin, Hin, Win, frame_bytes);
        const unsigned char* crop = r.fb + ((long long)r.y0 * Win + r.x0) * C;      // offsets from here stay below 2^30
        const int Dy = 2 * max(r.ch, Ho), Dx = 2 * max(r.cw, Wo);
        const int span_lo = aa_lo(oy_first, r.ch, Ho, Dy), span_hi = aa_hi(oy_last, r.ch, Ho, Dy);      // source rows of the tile: workgroup-uniform

        const int oxs = col_ok ? (r.flip ? Wo - 1 - oxc : oxc) : 0;
        const int cx = (2 * oxs + 1) * r.cw;
        const int kx_lo = aa_lo(oxs, r.cw, Wo, Dx), kx_hi = aa_hi(oxs, r.cw, Wo, Dx);
        const float sx = (float)aa_sum(kx_lo, kx_hi, Wo, cx, Dx);

        const int oyc = out_ok ? oy : oy_first;
        const int cy = (2 * oyc + 1) * r.ch;
        const int ky_lo = aa_lo(oyc, r.ch, Ho, Dy), ky_hi = out_ok ? aa_hi(oyc, r.ch, Ho, Dy) : -1;      // an empty window for a lane without a pixel
        const float sy = (float)aa_sum(ky_lo, aa_hi(oyc, r.ch, Ho, Dy), Ho, cy, Dy);

        float o[4][VEC];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[c][j] = 0.f;
        }
        for (int c0 = span_lo; c0 <= span_hi; c0 += AA_R) {
            // ---- phase 1: horizontal sums of chunk rows c0 + rg + RG j for output column oxc
            float h[RPL][4];
            unsigned ro[RPL];
#pragma unroll
            for (int j = 0; j < RPL; ++j) {
                ro[j] = (unsigned)((c0 + rg + RG * j) * Win) * (unsigned)C;
#pragma unroll
                for (int c = 0; c < 4; ++c) h[j][c] = 0.f;
            }
            if (col_ok) {
                const int nrows = span_hi - (c0 + rg) + 1;                         // rows j with RG * j < nrows are inside the tile's span
                if (C == 3) aa_hsums<3, RPL, RG>(h, crop, ro, nrows, kx_lo, kx_hi, r.cw, Wo, cx, Dx, sx);
                else if (C == 1) aa_hsums<1, RPL, RG>(h, crop, ro, nrows, kx_lo, kx_hi, r.cw, Wo, cx, Dx, sx);
                else if (C == 4) aa_hsums<4, RPL, RG>(h, crop, ro, nrows, kx_lo, kx_hi, r.cw, Wo, cx, Dx, sx);
                else aa_hsums<2, RPL, RG>(h, crop, ro, nrows, kx_lo, kx_hi, r.cw, Wo, cx, Dx, sx);
            }
#pragma unroll
            for (int j = 0; j < RPL; ++j) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c >= C) break;
                    hsum[((rg + RG * j) * 4 + c) * TW + col] = h[j][c];
                }
            }
            __syncthreads();
            // ---- phase 2: the chunk rows inside this lane's window
            const int lo = max(c0, ky_lo), hi = min(c0 + AA_R - 1, ky_hi);
            for (int k = lo; k <= hi; ++k) {
                const float w = (float)aa_weight(k, Ho, cy, Dy) / sy;
                const float* hp = hsum + (k - c0) * 4 * TW + oxl;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c >= C) break;
                    if constexpr (VEC == 4) {
                        const f32x4 x = *reinterpret_cast<const f32x4*>(hp + c * TW);
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[c][j] = fmaf(w, x[j], o[c][j]);
                    } else {
                        o[c][0] = fmaf(w, hp[c * TW], o[c][0]);
                    }
                }
            }
            __syncthreads();                                                       // the LDS is free for the next chunk or frame
        }
        if (out_ok) {
            float* out = dst + ((row * Tout + t) * C * Ho + oy) * (long long)Wo + ox0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= C) break;
                float val[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    float q = o[c][j] / 255.0f;                                    // ToTensor divides by 255 (not a multiply by 1/255)
                    if (mean_invstd) q = (q - mean_invstd[c]) * mean_invstd[C + c];
                    val[j] = q;
                }
                float* oc = out + (long long)c * Ho * Wo;
                if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(oc) = f32x4{val[0], val[1], val[2], val[3]};
                else oc[0] = val[0];
            }
        }
    }
}
}  // namespace

// ---- The host side: one job, one check, one launch rule.  Every transform entry point fills a HybClipJob and hands it to hyb_clip_ok and
// hyb_clip_launch; nothing below them restates a limit, the 16-byte rule or a grid.  A new variant is a kind, a row in CLIP_KINDS and a case in
// hyb_clip_launch's switch.
namespace {
enum HybClipKind { HYB_CLIP_PLAIN, HYB_CLIP_MIX, HYB_CLIP_VIEWS, HYB_CLIP_PHOTO, HYB_CLIP_AA, HYB_CLIP_AUG };
struct HybClipJob {
    int kind;
    const unsigned char* src; const int* params; const int* mix; const int* photo; const long long* luma_sums; const float* mean_invstd; float* dst;
    int B, V, Tin, Hin, Win, C, Tout, Ho, Wo;
    const int* aug = nullptr;          // the aug rows, behind the extents: the five older jobs are written without them
};
constexpr int CLIP_MAX_EXTENT = 16384;       // Hin, Win, Ho, Wo: the rule's integer products stay below 2^31
// What a kind asks beyond the shared rule: the row pointers it cannot do without, whether it takes V rows per source clip (else V is 1), and
// whether it needs a luma (defined for grey and RGB: C == 1 or C == 3; else C <= 4).  luma_sums and mean_invstd are optional everywhere.
struct ClipKindRule { bool needs_mix, needs_photo, has_views, luma, needs_aug; };
constexpr ClipKindRule CLIP_KINDS[] = {
    /* HYB_CLIP_PLAIN */ {false, false, false, false, false},
    /* HYB_CLIP_MIX   */ {true, false, false, false, false},
    /* HYB_CLIP_VIEWS */ {false, false, true, false, false},
    /* HYB_CLIP_PHOTO */ {false, true, false, true, false},       // (mix is optional here)
    /* HYB_CLIP_AA    */ {false, false, true, false, false},
    /* HYB_CLIP_AUG   */ {false, false, false, true, true},       // (mix and photo are optional here)
};

// The source side of the rule, which hyb_clips_u8_luma_sums shares: the bytes, the parameter rows, their extents and the channel count
bool clip_src_ok(const unsigned char* src, const int* params, int B, int Tin, int Hin, int Win, int C, int Tout, bool luma) {
    return src && params && B > 0 && Tin > 0 && Hin > 0 && Win > 0 && C > 0 && Tout > 0 && Hin <= CLIP_MAX_EXTENT && Win <= CLIP_MAX_EXTENT &&
           (luma ? C == 1 || C == 3 : C <= 4);
}

// The one validity rule; nothing here touches the device, so a refused job has made no HIP call
int hyb_clip_ok(const HybClipJob& j) {
    const ClipKindRule& k = CLIP_KINDS[j.kind];
    HYB_CHECK_ARG(clip_src_ok(j.src, j.params, j.B, j.Tin, j.Hin, j.Win, j.C, j.Tout, k.luma));
    HYB_CHECK_ARG(j.dst && j.Ho > 0 && j.Wo > 0 && j.Ho <= CLIP_MAX_EXTENT && j.Wo <= CLIP_MAX_EXTENT);
    HYB_CHECK_ARG((j.mix || !k.needs_mix) && (j.photo || !k.needs_photo) && (j.aug || !k.needs_aug));
    // the output clips are counted in int
    HYB_CHECK_ARG(k.has_views ? j.V >= 1 && (long long)j.B * j.V <= 2147483647LL : j.V == 1);
    return 0;
}

// The one launch rule.  blockIdx.y walks the B * V * Tout output frames, at most 65535 at a time; a lane owns VEC = 4 output pixels when the rows
// of dst can be written as 16-byte stores; blockIdx.x walks a frame's (row, quad) positions, or its tiles for the antialiased kernel.
int hyb_clip_launch(const HybClipJob& j, hipStream_t st) {
    const long long frames = (long long)j.B * j.V * j.Tout;
    const unsigned gy = (unsigned)(frames < 65535 ? frames : 65535);
    const bool vec = j.Wo % 4 == 0 && ((unsigned long long)j.dst & 15) == 0;
    const int lane_w = vec ? 4 : 1;
    const int gx = j.kind == HYB_CLIP_AA ? hyb_cdiv(j.Ho, AA_TH) * hyb_cdiv(j.Wo, AA_QW * lane_w)       // <= 512 * 2048 tiles
                                         : hyb_cdiv(j.Ho * (j.Wo / lane_w), 256);
    const dim3 grid(gx, gy);
#define CLIP_CASE(KIND, KERNEL, ...)                                                                  \
    case KIND:                                                                                        \
        if (vec) hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, st, __VA_ARGS__);                  \
        else hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, st, __VA_ARGS__);                      \
        break
#define CLIP_EXTENTS j.Tin, j.Hin, j.Win, j.C, j.Tout, j.Ho, j.Wo
    switch (j.kind) {
        CLIP_CASE(HYB_CLIP_PLAIN, clips_u8_transform_kernel, j.src, j.params, j.mean_invstd, j.dst, frames, CLIP_EXTENTS);
        CLIP_CASE(HYB_CLIP_MIX, clips_u8_transform_mix_kernel, j.src, j.params, j.mix, j.mean_invstd, j.dst, frames, j.B, CLIP_EXTENTS);
        CLIP_CASE(HYB_CLIP_VIEWS, clips_u8_transform_views_kernel, j.src, j.params, j.mean_invstd, j.dst, frames, j.V, CLIP_EXTENTS);
        CLIP_CASE(HYB_CLIP_PHOTO, clips_u8_transform_photo_kernel, j.src, j.params, j.mix, j.photo, j.luma_sums, j.mean_invstd, j.dst, frames, j.B,
                  CLIP_EXTENTS);
        CLIP_CASE(HYB_CLIP_AA, clips_u8_transform_aa_kernel, j.src, j.params, j.mean_invstd, j.dst, frames, j.V, CLIP_EXTENTS);
        CLIP_CASE(HYB_CLIP_AUG, clips_u8_transform_aug_kernel, j.src, j.params, j.mix, j.photo, j.aug, j.luma_sums, j.mean_invstd, j.dst, frames, j.B,
                  CLIP_EXTENTS);
    }
#undef CLIP_EXTENTS
#undef CLIP_CASE
    HYB_LAUNCH_CHECK();
    return 0;
}

int hyb_clip_run(const HybClipJob& j, void* stream) {
    const int rc = hyb_clip_ok(j);
    return rc ? rc : hyb_clip_launch(j, (hipStream_t)stream);
}
}  // namespace

extern "C" int hyb_clips_u8_transform(const unsigned char* src, const int* params, const float* mean_invstd, float* dst, int B, int Tin, int Hin,
                                      int Win, int C, int Tout, int Ho, int Wo, void* stream) {
    return hyb_clip_run({HYB_CLIP_PLAIN, src, params, nullptr, nullptr, nullptr, mean_invstd, dst, B, 1, Tin, Hin, Win, C, Tout, Ho, Wo}, stream);
}

extern "C" int hyb_clips_u8_transform_mix(const unsigned char* src, const int* params, const int* mix, const float* mean_invstd, float* dst, int B, int Tin,
                                          int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream) {
    return hyb_clip_run({HYB_CLIP_MIX, src, params, mix, nullptr, nullptr, mean_invstd, dst, B, 1, Tin, Hin, Win, C, Tout, Ho, Wo}, stream);
}

extern "C" int hyb_clips_u8_transform_views(const unsigned char* src, const int* params, const float* mean_invstd, float* dst, int B, int V, int Tin,
                                            int Hin, int Win, int C, int Tout, int Ho, int Wo, void* stream) {
    return hyb_clip_run({HYB_CLIP_VIEWS, src, params, nullptr, nullptr, nullptr, mean_invstd, dst, B, V, Tin, Hin, Win, C, Tout, Ho, Wo}, stream);
}

extern "C" int hyb_clips_u8_transform_photo(const unsigned char* src, const int* params, const int* mix, const int* photo, const long long* luma_sums,
                                            const float* mean_invstd, float* dst, int B, int Tin, int Hin, int Win, int C, int Tout, int Ho, int Wo,
                                            void* stream) {
    return hyb_clip_run({HYB_CLIP_PHOTO, src, params, mix, photo, luma_sums, mean_invstd, dst, B, 1, Tin, Hin, Win, C, Tout, Ho, Wo}, stream);
}

extern "C" int hyb_clips_u8_transform_aa(const unsigned char* src, const int* params, const float* mean_invstd, float* dst, int B, int V, int Tin, int Hin,
                                         int Win, int C, int Tout, int Ho, int Wo, void* stream) {
    return hyb_clip_run({HYB_CLIP_AA, src, params, nullptr, nullptr, nullptr, mean_invstd, dst, B, V, Tin, Hin, Win, C, Tout, Ho, Wo}, stream);
}

extern "C" int hyb_clip_aug_u8_transform(const unsigned char* src, const int* params, const int* mix, const int* photo, const int* aug,
                                         const long long* luma_sums, const float* mean_invstd, float* dst, int B, int Tin, int Hin, int Win, int C, int Tout,
                                         int Ho, int Wo, void* stream) {
    return hyb_clip_run({HYB_CLIP_AUG, src, params, mix, photo, luma_sums, mean_invstd, dst, B, 1, Tin, Hin, Win, C, Tout, Ho, Wo, aug}, stream);
}

// No job: no dst, a memset in front and a grid over the crop rows.  The source side of the check is the jobs'.
extern "C" int hyb_clips_u8_luma_sums(const unsigned char* src, const int* params, long long* sums, int B, int Tin, int Hin, int Win, int C, int Tout,
                                      void* stream) {
    HYB_CHECK_ARG(sums && clip_src_ok(src, params, B, Tin, Hin, Win, C, Tout, true));
    const long long frames = (long long)B * Tout;
    // the workgroups of a frame meet in sums[f] through integer atomics: zeroed here, on the same stream, in every call
    const hipError_t e = hipMemsetAsync(sums, 0, (size_t)frames * sizeof(long long), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const unsigned gy = (unsigned)(frames < 65535 ? frames : 65535);
    const dim3 grid(hyb_cdiv(Hin, LUMA_SPLIT_ROWS), gy);
    hipLaunchKernelGGL(clips_u8_luma_sums_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, params, reinterpret_cast<unsigned long long*>(sums), frames,
                       Tin, Hin, Win, C, Tout);
    HYB_LAUNCH_CHECK();
    return 0;
}
