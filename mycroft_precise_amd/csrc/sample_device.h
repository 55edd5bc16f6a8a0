// Choosing failing samples on the device (pe_trainer_sample_choose): what a cycle of precise-train-sampled
// does between its predict and its fit (scripts/train_sampled.py:62-70), next to the predictions.
//
// Every row of the resident training set has one state byte (bit 0 eligible, bit 1 selected).  A row FAILS when
// (p > 0.5f) != (y > 0.5f) and is a CANDIDATE when it fails, is eligible and is not selected.  The choice is the first
// max_new candidates in a total order, and that order is a 64-bit key, smaller first:
//   order index    key = row                                      (the lowest row first)
//   order error    key = (0xFFFFFFFF - bits(e)) << 32 | row       e = fabsf(__fsub_rn(p, y)) >= 0, whose float32 bits order
//                                                                 as unsigned integers; a NaN e counts as +infinity
// The row makes every key unique, so "the k smallest keys, ascending" has exactly one answer and no launch has to race for
// a position to give it:
//   sample_round<true>    a block owns kSampleBlock consecutive rows: it counts (integers; one atomic add per wave and
//                         counter), puts the keys of its candidates -- kSampleNone for every other row -- into LDS, sorts
//                         them there (bitonic, 2048 x 8 bytes = 16 KB) and writes its k smallest to slot blockIdx.x of `out`;
//   sample_round<false>   the same over the survivors, kSampleBlock keys per block, until one block is left; kSampleNone sorts
//                         behind every key, so a short block pads itself.  k <= 1024 = kSampleBlock / 2: a round halves the
//                         keys at least;
//   sample_finish         one wave: n_added = min(k, candidates); the first n_added keys of the last block are the choice, in
//                         order: their rows are marked selected, appended to the resident selection list and written to
//                         `added`; lane 0 writes the report.
// The sizes of all rounds follow from n and k alone, so the host launches them without reading anything back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pe {

constexpr int kSampleThreads = 512;
constexpr int kSampleBlock = 2048;          // rows (keys) of one selection block: a power of two, 2 * the largest max_new
constexpr unsigned long long kSampleNone = ~0ull;
constexpr uint8_t kSampleEligible = 1, kSampleSelected = 2;

struct SampleReport {                       // pe_sample_report
    long long n, n_correct, n_failed, n_remaining, n_added, n_selected;
};

struct SampleArgs {
    const float* probs;                     // [n] predictions of the chosen network
    const float* targets;                   // [n]
    uint8_t* state;                         // [n]
    int n;                                  // rows of the set
    int k;                                  // max_new; 0: count only
    int order;                              // 0 index, 1 error
    long long m;                            // keys (rows) this round reads
    const unsigned long long* in;           // [m] survivors of the round before (sample_round<false>)
    unsigned long long* out;                // [blocks of this round][k]
    unsigned long long* counters;           // [3] n_correct, n_failed, n_remaining; zero before the first round
    int32_t* added;                         // [k]
    int32_t* selection;                     // [n] the resident selection list
    int n_selected;                         // its length before this call
    SampleReport* report;
};

struct SampleGatherArgs {
    const float* targets;                   // [rows of the set]
    const int32_t* indices;                 // [n]
    int n;
    float* out;                             // [n] targets[indices[i]]
};

inline int sample_blocks(long long m) { return (int)((m + kSampleBlock - 1) / kSampleBlock); }
hipError_t launch_sample_choose(const SampleArgs& a, unsigned long long* keys_a, unsigned long long* keys_b, hipStream_t s);
hipError_t launch_sample_gather_targets(const SampleGatherArgs& a, hipStream_t s);

#if defined(__HIPCC__)

__device__ __forceinline__ uint32_t sample_wave_sum(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <bool FROM_ROWS>
__device__ __forceinline__ void sample_round(const SampleArgs& a, unsigned long long* keys) {
    const int tid = (int)threadIdx.x;
    const long long base = (long long)blockIdx.x * kSampleBlock;
    uint32_t n_ok = 0, n_fail = 0, n_cand = 0;
    for (int s = tid; s < kSampleBlock; s += kSampleThreads) {
        const long long i = base + s;
        unsigned long long key = kSampleNone;
        if (i < a.m) {
            if (FROM_ROWS) {
                const float p = a.probs[i], y = a.targets[i];
                const uint8_t st = a.state[i];
                const bool fail = (p > 0.5f) != (y > 0.5f);         // a NaN p compares false, as numpy's does
                const bool eligible = (st & kSampleEligible) != 0;
                const bool cand = fail && eligible && !(st & kSampleSelected);
                n_ok += fail ? 0u : 1u;
                n_fail += (fail && eligible) ? 1u : 0u;
                n_cand += cand ? 1u : 0u;
                if (cand) {
                    uint32_t hi = 0u;
                    if (a.order == 1) {
                        const float e = fabsf(__fsub_rn(p, y));
                        hi = 0xFFFFFFFFu - (e != e ? 0x7F800000u : __float_as_uint(e));
                    }
                    key = ((unsigned long long)hi << 32) | (unsigned long long)(uint32_t)i;
                }
            } else {
                key = a.in[i];
            }
        }
        keys[s] = key;
    }
    if (FROM_ROWS) {
        n_ok = sample_wave_sum(n_ok);
        n_fail = sample_wave_sum(n_fail);
        n_cand = sample_wave_sum(n_cand);
        if ((tid & 63) == 0) {
            if (n_ok) atomicAdd(&a.counters[0], (unsigned long long)n_ok);
            if (n_fail) atomicAdd(&a.counters[1], (unsigned long long)n_fail);
            if (n_cand) atomicAdd(&a.counters[2], (unsigned long long)n_cand);
        }
    }
    if (a.k <= 0) return;
    for (int size = 2; size <= kSampleBlock; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < kSampleBlock / 2; t += kSampleThreads) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const unsigned long long x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & size) == 0)) { keys[lo] = y; keys[hi] = x; }
            }
        }
    __syncthreads();
    for (int s = tid; s < a.k; s += kSampleThreads) a.out[(size_t)blockIdx.x * a.k + s] = keys[s];
}

// one wave; a.in: the k keys of the last round's only block (unused with k = 0)
__device__ __forceinline__ void sample_finish(const SampleArgs& a) {
    const int lane = (int)threadIdx.x;
    const long long remaining = (long long)a.counters[2];
    const int n_added = remaining < a.k ? (int)remaining : a.k;
    for (int i = lane; i < n_added; i += 64) {
        const int32_t row = (int32_t)(uint32_t)(a.in[i] & 0xFFFFFFFFull);
        a.added[i] = row;
        a.selection[a.n_selected + i] = row;
        a.state[row] = (uint8_t)(a.state[row] | kSampleSelected);      // a byte of its own: the chosen rows are distinct
    }
    if (lane == 0) {
        SampleReport r;
        r.n = a.n;
        r.n_correct = (long long)a.counters[0];
        r.n_failed = (long long)a.counters[1];
        r.n_remaining = remaining;
        r.n_added = n_added;
        r.n_selected = (long long)a.n_selected + n_added;
        *a.report = r;
    }
}

__device__ __forceinline__ void sample_gather_targets(const SampleGatherArgs& a) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < a.n) a.out[i] = a.targets[a.indices[i]];
}

#endif  // __HIPCC__

}  // namespace pe
