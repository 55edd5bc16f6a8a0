// The __global__ entry points of the mining session (pe_miner) and their launchers; the device code is mine_device.h.
#include "mine_device.h"

using namespace pe;

__global__ __launch_bounds__(64) void mine_gather_kernel(const MineGatherArgs a) { mine_gather(a); }
__global__ __launch_bounds__(kMineThreads) void mine_count_kernel(const MineCompactArgs a) {
    __shared__ uint32_t wave_total[kMineThreads / 64];
    mine_block_walk<false>(a, wave_total);
}
__global__ __launch_bounds__(64) void mine_scan_counts_kernel(const MineCompactArgs a) { mine_scan_counts(a); }
__global__ __launch_bounds__(kMineThreads) void mine_write_kernel(const MineCompactArgs a) {
    __shared__ uint32_t wave_total[kMineThreads / 64];
    mine_block_walk<true>(a, wave_total);
}
__global__ __launch_bounds__(256) void mine_ring_kernel(const MineRingArgs a) { mine_ring(a); }

namespace pe {

hipError_t launch_mine_gather(const MineGatherArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mine_gather_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mine_compact(const MineCompactArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.n_blocks != mine_blocks(a.n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mine_count_kernel, dim3((unsigned)a.n_blocks), dim3(kMineThreads), 0, s, a);
    hipLaunchKernelGGL(mine_scan_counts_kernel, dim3(1), dim3(64), 0, s, a);
    if (a.capacity > 0) hipLaunchKernelGGL(mine_write_kernel, dim3((unsigned)a.n_blocks), dim3(kMineThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mine_ring(const MineRingArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.buffer_samples <= 0) return hipSuccess;
    if (a.n > 65535) return hipErrorInvalidValue;               // grid.y: the host cuts its passes below that
    hipLaunchKernelGGL(mine_ring_kernel, dim3((unsigned)((a.buffer_samples + 255) / 256), (unsigned)a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe
