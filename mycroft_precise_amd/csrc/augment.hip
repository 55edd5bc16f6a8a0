// The __global__ entry points of the augmenting session (pe_augmenter) and their launchers; the device code is augment_device.h.
#include "augment_device.h"

using namespace pe;

__global__ __launch_bounds__(kAugChains) void aug_energy_kernel(const AugEnergyArgs a) {
    __shared__ AugEnergyShared sh;
    if (a.offsets) aug_energy<true>(a, sh); else aug_energy<false>(a, sh);      // clip chains / copy chains: uniform over the launch
}
__global__ __launch_bounds__(kAugMixThreads) void aug_mix_kernel(const AugMixArgs a) { aug_mix(a); }

namespace pe {

namespace {
hipError_t launch_aug_energy(const AugEnergyArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(aug_energy_kernel, dim3((unsigned)((a.n + kAugChains - 1) / kAugChains)), dim3(kAugChains), 0, s, a);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_aug_energy_clips(const AugEnergyArgs& a, hipStream_t s) {
    if (a.n > 0 && (!a.pool || !a.offsets || !a.sum_f32)) return hipErrorInvalidValue;
    return launch_aug_energy(a, s);
}

hipError_t launch_aug_energy_copies(const AugEnergyArgs& a, hipStream_t s) {
    if (a.n > 0 && (!a.pool || a.offsets || !a.first_piece || !a.piece_prefix || !a.piece_src || !a.sum_f64 || !a.zero)) return hipErrorInvalidValue;
    return launch_aug_energy(a, s);
}

hipError_t launch_aug_mix(const AugMixArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const long long blocks = (a.n + kAugMixThreads - 1) / kAugMixThreads;
    if (blocks > 0x7fffffffll || a.n_pieces <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aug_mix_kernel, dim3((unsigned)blocks), dim3(kAugMixThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe
