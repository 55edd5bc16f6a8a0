// The __global__ entry point of the generating session (pe_generator) and its launcher; the device code is generate_device.h.
#include "generate_device.h"

using namespace pe;

__global__ __launch_bounds__(kGenThreads) void gen_mix_kernel(const GenMixArgs a) { gen_mix(a); }

namespace pe {

hipError_t launch_gen_mix(const GenMixArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const long long blocks = (a.n + kGenThreads - 1) / kGenThreads;
    if (blocks > 0x7fffffffll || a.seg_hi <= a.seg_lo) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gen_mix_kernel, dim3((unsigned)blocks), dim3(kGenThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe
