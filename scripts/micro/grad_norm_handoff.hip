// The cross-workgroup hand-off of hyb_grad_norm, two forms timed on a gradient-sized set of tensors ("fused AdamW"):
//   two-launch : the shipped form (this file includes csrc/optim.hip and calls hyb_grad_norm): per-chunk sums, then a one-workgroup launch;
//   ticket     : the in-launch form that was built first and dropped: partial stored write-through, RELEASE fetch_add on a ticket word at
//                agent scope, ACQUIRE fence + the same final sum in the workgroup that finishes last -- one launch.
// Both give the same bits (checked).  Measured on an MI355X: ticket 38.6 us, two-launch 11.7 us per call.  Build and run:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Itransformer_cnn_hybrid_network_for_video_processing_amd/csrc \
//         scripts/micro/grad_norm_handoff.hip -o scripts/micro/grad_norm_handoff && scripts/micro/grad_norm_handoff
#include "../../transformer_cnn_hybrid_network_for_video_processing_amd/csrc/optim.hip"
#include <cstdio>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

namespace {

__global__ __launch_bounds__(256) void ticket_form_kernel(GradNormArgs a, int total, const double* hyper, float* norm_out, unsigned int* ticket) {
    __shared__ float s_wave[4];
    __shared__ int s_last;
    __shared__ double s_sum[256];
    const float s = grad_chunk_sumsq(a, s_wave);
    if (threadIdx.x == 0) {
        __hip_atomic_store(a.partials + a.chunk_offset + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)total - 1u;
        if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    const float* partials = a.partials;
    grad_norm_finish([partials](int i) { return __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }, total, hyper, norm_out, s_sum);
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

int main() {
    const int T = 40;                                    // 40 tensors of 170 667 floats: 27.3 MB, the model's gradient size; one launch
    const long long N = 170667;
    std::vector<float> host((size_t)N);
    unsigned long long z = 12345;
    for (auto& v : host) { z = z * 6364136223846793005ull + 1442695040888963407ull; v = ((int)(z >> 40) - (1 << 23)) * (1.0f / (1 << 23)); }
    std::vector<const float*> ptrs(T);
    std::vector<long long> numel(T, N);
    for (int i = 0; i < T; ++i) {
        float* d;
        CK(hipMalloc(&d, N * sizeof(float)));
        CK(hipMemcpy(d, host.data(), N * sizeof(float), hipMemcpyHostToDevice));
        ptrs[i] = d;
    }
    const size_t chunks = hyb_grad_norm_workspace(T, numel.data());
    float *partials, *out, *partials2, *out2;
    unsigned int* ticket;
    double* hyper;
    CK(hipMalloc(&partials, chunks * 4)); CK(hipMalloc(&partials2, chunks * 4)); CK(hipMalloc(&out, 8)); CK(hipMalloc(&out2, 8));
    CK(hipMalloc(&ticket, 4)); CK(hipMalloc(&hyper, 48));
    CK(hipMemset(ticket, 0, 4)); CK(hipMemset(partials, 0, chunks * 4)); CK(hipMemset(partials2, 0, chunks * 4));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    if (hyb_adamw_hyper_set(hyper, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 100.0, st) != 0) return 1;

    GradNormArgs a{};
    int c = 0;
    for (int i = 0; i < T; ++i) { a.g[i] = ptrs[i]; a.n[i] = N; a.chunk_begin[i] = c; c += hyb_cdiv(N, ADAM_CHUNK); }
    a.chunk_begin[T] = c; a.count = T; a.chunk_offset = 0; a.partials = partials2;
    auto ticket_form = [&]() {
        hipLaunchKernelGGL(ticket_form_kernel, dim3(c), dim3(256), 0, st, a, c, (const double*)hyper, out2, ticket);
        return (int)hipGetLastError();
    };
    auto two_launch = [&]() { return hyb_grad_norm(T, ptrs.data(), numel.data(), partials, hyper, out, st); };
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int ITER = 300;
    for (int i = 0; i < 20; ++i) { if (ticket_form() != 0 || two_launch() != 0) return 1; }
    CK(hipStreamSynchronize(st));
    for (int round = 0; round < 3; ++round) {
        float ms[2];
        for (int form = 0; form < 2; ++form) {
            CK(hipEventRecord(e0, st));
            for (int i = 0; i < ITER; ++i) { if ((form == 0 ? ticket_form() : two_launch()) != 0) return 1; }
            CK(hipEventRecord(e1, st));
            CK(hipStreamSynchronize(st));
            CK(hipEventElapsedTime(&ms[form], e0, e1));
        }
        printf("round %d: ticket form %.2f us per call, two-launch form %.2f us per call (%zu chunks, %.1f MB)\n", round, ms[0] * 1e3 / ITER,
               ms[1] * 1e3 / ITER, chunks, T * N * 4 / 1e6);
    }
    float r1[2], r2[2];
    unsigned int tk;
    CK(hipMemcpy(r1, out, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(r2, out2, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&tk, ticket, 4, hipMemcpyDeviceToHost));
    printf("norm %.9g / %.9g, coef %.9g / %.9g, bits equal %d, ticket at rest %u\n", r1[0], r2[0], r1[1], r2[1], memcmp(r1, r2, 8) == 0, tk);
    return memcmp(r1, r2, 8) == 0 && tk == 0 ? 0 : 2;
}
