// Judging trained models on the device (pe_stats_scores / pe_test_clips / pe_trainer_stats_models): what
// precise-test, precise-graph and precise-calc-threshold compute from predictions and targets (stats.py:46-58,102-107,
// scripts/graph.py:147-151, scripts/calc_threshold.py:66-77, annoyance_estimator.py:83-84) for several rows of predictions
// (one per network) against one row of targets and a table of thresholds.
//
// Three kernels, every one of them with row = blockIdx.y:
//   stats_scan    one wave per word of 64 samples.  The bin of a prediction is the number of thresholds it lies above; a sample
//                 that lies above thresholds[j] is one whose bin is > j, so a histogram of bins, summed from the top on the host,
//                 is the count for every threshold at once.  `p > t` and `p >= t` give two bins: blockIdx.z = 0 takes the first,
//                 blockIdx.z = 1 the second, so a workgroup holds two LDS histograms (positive / negative targets) of T + 1
//                 bins -- 32 KB at T = 4096 -- and adds what it counted to the global one with integer atomics.  The z = 0
//                 workgroups also count the classes by ballot and leave the word's float64 sum of x = -log(1 / p - 1) over the
//                 calibration samples, reduced in a fixed butterfly (absent lanes add +0.0).
//   stats_spread  the second pass of the two-pass deviation: every wave adds the word sums up in word order (the mean), then
//                 leaves the word's sum of (x - mean)^2 in the same fixed shape.
//   stats_finish  one wave per row: both ordered sums again, the mean, the deviation, the summary record.
// No floating-point atomics: every float64 sum has an order that depends on n alone, so a row's two doubles are the same bits
// in every run, alone or among other rows, with any threshold table and any grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pe {

constexpr int kStatsWaves = 4;
constexpr int kStatsMaxRows = 16;            // rows of one call: PE_TRAIN_MAX_MODELS networks
constexpr int kStatsMaxThresholds = 4096;
constexpr int kStatsGridCap = 1024;          // workgroups along x; the words are strided over them

enum { kStatsPos = 0, kStatsNeg, kStatsOther, kStatsNan, kStatsUnsaturated, kStatsFit, kStatsCounters };

struct StatsSummary {       // = pe_stats_summary (precise_engine.h)
    long long n, n_pos, n_neg, n_other, n_nan, n_unsaturated, n_fit;
    double logit_mean, logit_std;
};

struct StatsArgs {
    const float* probs; long long stride;   // [rows][stride], n valid per row
    const float* targets;                   // [n], shared by the rows
    long long n;
    uint32_t n_words;                       // ceil(n / 64)
    const double* thresholds; int n_thresholds;     // non-decreasing, no NaN; may be null / 0
    unsigned long long* hist;               // [rows][2: > / >=][2: positive / negative][n_thresholds + 1], added to
    unsigned long long* counters;           // [rows][kStatsCounters], added to
    double* word_x;                         // [rows][n_words] sums of x
    double* word_d;                         // [rows][n_words] sums of (x - mean)^2
    StatsSummary* summary;                  // [rows]
};

// the logit calc_threshold.py:73 forms: numpy's float32 `1 / outputs - 1`, two roundings, then the logarithm -- in float64 here
__device__ __forceinline__ double stats_logit(float p) {
    const float u = __fsub_rn(__fdiv_rn(1.0f, p), 1.0f);
    return -log((double)u);
}
// save_spots of calc_threshold.py:66 (a NaN is no data either), then targets > 0.5 (:75)
__device__ __forceinline__ bool stats_unsaturated(float p) { return p == p && p != 0.0f && p != 1.0f; }

// thresholds below the prediction (or_equal: not above it).  F32: both sides float32, as numpy compares a float32 array with a
// Python float; else both float64, as it compares one with a float64 array.  The rounding to float32 is monotone, so the
// table stays sorted; a NaN prediction is above nothing.
template <bool F32>
__device__ __forceinline__ int stats_bin(const double* thresholds, int n_thresholds, float p, bool or_equal) {
    const double pd = (double)p;
    int lo = 0, hi = n_thresholds;                  // thresholds[0 .. lo) are below p, thresholds[hi ..) are not
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double t = thresholds[mid];
        bool below;
        if (F32) { const float tf = (float)t; below = or_equal ? tf <= p : tf < p; }
        else below = or_equal ? t <= pd : t < pd;
        if (below) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// words[0] + words[1] + ... in that order, the same value in every lane of the wave
__device__ __forceinline__ double stats_ordered_sum(const double* words, uint32_t n_words, int lane) {
    double s = 0.0;
    for (uint32_t base = 0; base < n_words; base += 64) {
        const double v = base + lane < n_words ? words[base + lane] : 0.0;
        const int m = n_words - base < 64u ? (int)(n_words - base) : 64;
        for (int i = 0; i < m; ++i) s += __shfl(v, i);
    }
    return s;
}

__device__ __forceinline__ double stats_word_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);       // (a + b = b + a: every lane ends with the same bits)
    return v;
}

template <bool F32>
__device__ __forceinline__ void stats_scan(const StatsArgs& a, uint32_t* bins) {
    const int row = (int)blockIdx.y, kind = (int)blockIdx.z, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_bins = a.n_thresholds + 1;
    const bool hist = a.n_thresholds > 0;
    if (hist) {
        for (int i = threadIdx.x; i < 2 * n_bins; i += 64 * kStatsWaves) bins[i] = 0;
        __syncthreads();
    }
    const float* const probs = a.probs + (size_t)row * a.stride;
    unsigned long long count[kStatsCounters] = {};
    for (uint32_t w = blockIdx.x * kStatsWaves + wave; w < a.n_words; w += gridDim.x * kStatsWaves) {
        const long long j = (long long)w * 64 + lane;
        const bool valid = j < a.n;
        const float p = valid ? probs[j] : 0.0f;
        const float y = valid ? a.targets[j] : 0.0f;
        const bool pos = valid && y > 0.5f, neg = valid && y == 0.0f;
        if (hist && (pos || neg)) atomicAdd(&bins[(pos ? 0 : n_bins) + stats_bin<F32>(a.thresholds, a.n_thresholds, p, kind == 1)], 1u);
        if (kind == 0) {
            const bool fit = pos && stats_unsaturated(p);
            count[kStatsPos] += __popcll(__ballot(pos));
            count[kStatsNeg] += __popcll(__ballot(neg));
            count[kStatsOther] += __popcll(__ballot(valid && !pos && !neg));
            count[kStatsNan] += __popcll(__ballot(valid && p != p));
            count[kStatsUnsaturated] += __popcll(__ballot(valid && stats_unsaturated(p)));
            count[kStatsFit] += __popcll(__ballot(fit));
            const double sum = stats_word_sum(fit ? stats_logit(p) : 0.0);
            if (lane == 0) a.word_x[(size_t)row * a.n_words + w] = sum;
        }
    }
    if (kind == 0 && lane == 0)
        for (int k = 0; k < kStatsCounters; ++k)
            if (count[k]) atomicAdd(&a.counters[(size_t)row * kStatsCounters + k], count[k]);
    if (hist) {
        __syncthreads();
        unsigned long long* const out = a.hist + ((size_t)row * 2 + kind) * 2 * n_bins;
        for (int i = threadIdx.x; i < 2 * n_bins; i += 64 * kStatsWaves)
            if (bins[i]) atomicAdd(&out[i], (unsigned long long)bins[i]);
    }
}

__device__ __forceinline__ void stats_spread(const StatsArgs& a) {
#pragma clang fp contract(off)
    const int row = (int)blockIdx.y, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* const probs = a.probs + (size_t)row * a.stride;
    const double* const word_x = a.word_x + (size_t)row * a.n_words;
    const double mean = stats_ordered_sum(word_x, a.n_words, lane) / (double)a.counters[(size_t)row * kStatsCounters + kStatsFit];
    for (uint32_t w = blockIdx.x * kStatsWaves + wave; w < a.n_words; w += gridDim.x * kStatsWaves) {
        const long long j = (long long)w * 64 + lane;
        const bool valid = j < a.n;
        const float p = valid ? probs[j] : 0.0f;
        const bool fit = valid && a.targets[j] > 0.5f && stats_unsaturated(p);
        const double d = fit ? stats_logit(p) - mean : 0.0;
        const double sum = stats_word_sum(d * d);
        if (lane == 0) a.word_d[(size_t)row * a.n_words + w] = sum;
    }
}

__device__ __forceinline__ void stats_finish(const StatsArgs& a) {
    const int row = (int)blockIdx.y, lane = threadIdx.x & 63;
    const unsigned long long* const c = a.counters + (size_t)row * kStatsCounters;
    const double n_fit = (double)c[kStatsFit];          // none: 0 / 0, NaN for both
    const double mean = stats_ordered_sum(a.word_x + (size_t)row * a.n_words, a.n_words, lane) / n_fit;
    const double spread = stats_ordered_sum(a.word_d + (size_t)row * a.n_words, a.n_words, lane) / n_fit;
    if (lane == 0)
        a.summary[row] = StatsSummary{a.n, (long long)c[kStatsPos], (long long)c[kStatsNeg], (long long)c[kStatsOther], (long long)c[kStatsNan],
                                      (long long)c[kStatsUnsaturated], (long long)c[kStatsFit], mean, sqrt(spread)};
}

// the three kernels over `rows` rows; compare: 0 = float32 comparisons, 1 = float64.  a.hist and a.counters are zero on entry.
hipError_t launch_stats(const StatsArgs& a, int rows, int compare, hipStream_t s);

}  // namespace pe
