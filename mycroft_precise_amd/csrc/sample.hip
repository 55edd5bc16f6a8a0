// The __global__ entry points of sampled training (pe_trainer_sample_choose / pe_trainer_evaluate_indices) and their
// launchers; the device code is sample_device.h.
#include "sample_device.h"

using namespace pe;

template <bool FROM_ROWS>
__global__ __launch_bounds__(kSampleThreads) void sample_round_kernel(const SampleArgs a) {
    __shared__ unsigned long long keys[kSampleBlock];
    sample_round<FROM_ROWS>(a, keys);
}
__global__ __launch_bounds__(64) void sample_finish_kernel(const SampleArgs a) { sample_finish(a); }
__global__ __launch_bounds__(256) void sample_gather_targets_kernel(const SampleGatherArgs a) { sample_gather_targets(a); }

namespace pe {

// keys_a / keys_b: sample_blocks(n) * k keys each (unused with k = 0); a.counters are zero
hipError_t launch_sample_choose(const SampleArgs& a0, unsigned long long* keys_a, unsigned long long* keys_b, hipStream_t s) {
    if (a0.n < 1 || a0.k < 0 || a0.k > kSampleBlock / 2 || (a0.order != 0 && a0.order != 1)) return hipErrorInvalidValue;
    if (!a0.probs || !a0.targets || !a0.state || !a0.counters || !a0.added || !a0.selection || !a0.report) return hipErrorInvalidValue;
    if (a0.k > 0 && (!keys_a || !keys_b)) return hipErrorInvalidValue;
    SampleArgs a = a0;
    a.m = a.n;
    a.in = nullptr;
    a.out = keys_a;
    int blocks = sample_blocks(a.m);
    hipLaunchKernelGGL(sample_round_kernel<true>, dim3((unsigned)blocks), dim3(kSampleThreads), 0, s, a);
    while (a.k > 0 && blocks > 1) {
        a.m = (long long)blocks * a.k;
        a.in = a.out;
        a.out = a.in == keys_a ? keys_b : keys_a;
        blocks = sample_blocks(a.m);
        hipLaunchKernelGGL(sample_round_kernel<false>, dim3((unsigned)blocks), dim3(kSampleThreads), 0, s, a);
    }
    a.in = a.out;
    hipLaunchKernelGGL(sample_finish_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sample_gather_targets(const SampleGatherArgs& a, hipStream_t s) {
    if (a.n < 1 || !a.targets || !a.indices || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_gather_targets_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe
