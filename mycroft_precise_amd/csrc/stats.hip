// The __global__ entry points of the statistics calls (pe_stats_scores / pe_test_clips / pe_trainer_stats_models) and their
// launcher; the device code is stats_device.h.
#include "stats_device.h"

using namespace pe;

template <bool F32>
__global__ __launch_bounds__(64 * kStatsWaves) void stats_scan_kernel(const StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t stats_bins[];
    stats_scan<F32>(a, stats_bins);
}
__global__ __launch_bounds__(64 * kStatsWaves) void stats_spread_kernel(const StatsArgs a) { stats_spread(a); }
__global__ __launch_bounds__(64) void stats_finish_kernel(const StatsArgs a) { stats_finish(a); }

namespace pe {

hipError_t launch_stats(const StatsArgs& a, int rows, int compare, hipStream_t s) {
    if (rows < 1 || rows > kStatsMaxRows || a.n < 1 || a.n > 0x7fffffffll || a.stride < a.n) return hipErrorInvalidValue;
    if (a.n_words != (uint32_t)((a.n + 63) / 64) || a.n_thresholds < 0 || a.n_thresholds > kStatsMaxThresholds) return hipErrorInvalidValue;
    if (!a.probs || !a.targets || !a.counters || !a.word_x || !a.word_d || !a.summary) return hipErrorInvalidValue;
    if (a.n_thresholds > 0 && (!a.thresholds || !a.hist)) return hipErrorInvalidValue;
    if (compare != 0 && compare != 1) return hipErrorInvalidValue;
    const unsigned want = (a.n_words + kStatsWaves - 1) / kStatsWaves;
    const unsigned blocks = want < (unsigned)kStatsGridCap ? want : (unsigned)kStatsGridCap;
    // two histograms of n_thresholds + 1 bins: 32 776 bytes at 4096 thresholds, within the 48 KB a launch may ask for as it is
    const size_t lds = a.n_thresholds ? (size_t)2 * (a.n_thresholds + 1) * sizeof(uint32_t) : 0;
    const dim3 grid(blocks, (unsigned)rows, a.n_thresholds ? 2 : 1);
    if (compare == 0) hipLaunchKernelGGL(stats_scan_kernel<true>, grid, dim3(64 * kStatsWaves), lds, s, a);
    else hipLaunchKernelGGL(stats_scan_kernel<false>, grid, dim3(64 * kStatsWaves), lds, s, a);
    hipLaunchKernelGGL(stats_spread_kernel, dim3(blocks, (unsigned)rows), dim3(64 * kStatsWaves), 0, s, a);
    hipLaunchKernelGGL(stats_finish_kernel, dim3(1, (unsigned)rows), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe
