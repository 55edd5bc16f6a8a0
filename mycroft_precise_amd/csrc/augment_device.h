// Noise augmentation on the device (pe_augmenter): what precise-add-noise does per sample
// (scripts/add_noise.py:66-90, then save_audio / load_audio, util.py:65,71) for every copy of many clips at once.
//
// The host planner (augment.py) has replayed the script's noise cursor and its one random draw per copy into PIECES:
// consecutive runs of a copy's output samples under which lies one stretch of one noise recording.  Two kernels:
//   aug_energy   the two Python sum() calls of noised_audio (:87-88) as what they are, sequential chains -- one lane per chain,
//                never a tree: S_a = sum(audio ** 2) is a float32 chain over a clip, S_n = sum(noise_data ** 2) a float64 chain
//                over a copy's noise samples in piece order.  The scale sqrt(S_a) / sqrt(S_n) feeds a truncation to int16, so
//                another summation order would flip isolated samples by one step.  The square roots are the host's.
//   aug_mix      one thread per output sample of a pass: adjusted noise, the mix, save_audio's int16 and load_audio's float32,
//                which feeds the clip front end (pe_vectorize_clips' launch: there is no second MFCC).
// Every product and sum is rounded once, as numpy rounds it: the compiler contracts a * b + c into a fused multiply-add by
// default -- through the _rn intrinsics too, which are plain operators that carry the permission with them -- and that is another
// number than numpy's.  So both device functions switch contraction off for their bodies (#pragma clang fp contract(off)) and
// spell the arithmetic with plain operators: each one is then one IEEE operation, rounded to nearest.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pe {

constexpr int kAugMixThreads = 256;
constexpr int kAugChains = 64;                      // chains of an energy block: one wave, one lane per chain
constexpr int kAugRowStride = kAugChains + 1;       // floats between two chains' rows in LDS: lane l reads bank (l + k) % 32

struct AugEnergyArgs {
    const float* pool;              // the samples: the clip pool (clip chains) or the noise pool (copy chains)
    // clip chains: chain c is pool[offsets[c] .. offsets[c + 1])
    const long long* offsets;       // [n + 1]
    // copy chains: chain c walks pieces first_piece[c] .. first_piece[c + 1]; piece q holds output positions
    // piece_prefix[q] .. piece_prefix[q + 1] of the plan and starts at pool[piece_src[q]]
    const long long* first_piece;   // [n + 1]
    const long long* piece_prefix;  // [pieces + 1]
    const long long* piece_src;     // [pieces]
    int n;                          // chains
    float* sum_f32;                 // [n] clip chains: S_a
    double* sum_f64;                // [n] copy chains: S_n
    int32_t* zero;                  // [n] copy chains: 1 where S_n == 0 (the reference divides by sqrt(0): NaN), else 0
};

struct AugSlot {                    // one copy of a pass
    double va, vn, ratio;           // sqrt((double)S_a) of its clip, sqrt(S_n) of its noise, the draw
    float keep;                     // (float)(1.0 - ratio): numpy rounds the Python scalar to the float32 array's type
    int32_t copy;                   // its index in the plan: where its overflows are counted
};
struct AugPiece {                   // one piece of a pass
    long long noise;                // index in the noise pool of the sample under the piece's first sample
    long long clip;                 // index in the clip pool of the same
    int32_t slot;
    int32_t pad;
};

struct AugMixArgs {
    const float* clips;             // clip pool
    const float* noise;             // noise pool
    const AugSlot* slots;           // [copies of the pass]
    const AugPiece* pieces;         // [pieces of the pass]
    const long long* prefix;        // [pieces + 1] exclusive prefix sum of the piece lengths: output positions of the pass
    int n_pieces;
    long long n;                    // samples of the pass: prefix[n_pieces]
    float* reloaded;                // [n] load_audio(save_audio(mix)), or null
    double* mixed;                  // [n] the float64 mix, or null
    int16_t* pcm;                   // [n] what save_audio writes, or null
    unsigned long long* overflowed; // [copies of the plan] += samples whose |mix * 32767| >= 32768, or null
};

hipError_t launch_aug_energy_clips(const AugEnergyArgs& a, hipStream_t s);
hipError_t launch_aug_energy_copies(const AugEnergyArgs& a, hipStream_t s);
hipError_t launch_aug_mix(const AugMixArgs& a, hipStream_t s);

#if defined(__HIPCC__)

// One wave per block, lane l owns chain blockIdx.x * 64 + l.  A lane reading its own chain from memory would touch 64
// different cache lines per step of the wave; instead the wave stages 64 samples of each of its chains through LDS -- row c
// is loaded by all lanes together, coalesced, kAugStage rows in flight at a time -- and lane l then walks row l.  The rows are
// kAugRowStride floats apart, so the lanes' reads fall on different banks.
//   clip chains   s = fl32(s + fl32(a * a)), i ascending from 0                       sum(audio ** 2) on a float32 array
//   copy chains   s = s + (double)n * (double)n (the square of a float32 is exact)    sum(noise_data ** 2) on float64
// A lane keeps the piece under its chain's cursor in registers (where it ends, and where its samples lie) and publishes, per
// step, where its next row starts in the pool and how much of the row the piece covers; lanes past that point of a row (a row
// that crosses into the next piece: rare, pieces are recordings long) walk the piece table themselves.
struct AugEnergyShared {
    float tile[kAugChains * kAugRowStride];
    long long row_src[kAugChains];      // index in the pool of the row's first sample
    long long row_pos[kAugChains];      // copy chains: its position in the plan
    int row_n[kAugChains];              // samples of the row: 0 .. 64
    int row_run[kAugChains];            // the first row_run of them lie in one piece, consecutive from row_src
    int piece[kAugChains];              // that piece
};
constexpr int kAugStage = 64;

template <bool CLIPS>
__device__ __forceinline__ void aug_energy(const AugEnergyArgs& a, AugEnergyShared& sh) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x;
    const int chain = (int)blockIdx.x * kAugChains + lane;
    long long first = 0, len = 0;       // clip chains: in the pool; copy chains: in the plan's output positions
    long long piece_end = 0, src_off = 0;   // the piece under the cursor ends at piece_end; position p of it is pool[src_off + p]
    int q = 0;
    if (chain < a.n) {
        if (CLIPS) {
            first = a.offsets[chain];
            len = a.offsets[chain + 1] - first;
            piece_end = first + len;
        } else {
            q = (int)a.first_piece[chain];
            first = a.piece_prefix[q];
            len = a.piece_prefix[a.first_piece[chain + 1]] - first;
            if (len > 0) { piece_end = a.piece_prefix[q + 1]; src_off = a.piece_src[q] - first; }
        }
    }
    long long longest = len;
    for (int d = 32; d > 0; d >>= 1) {
        const long long other = __shfl_xor(longest, d);
        longest = other > longest ? other : longest;
    }
    float s32 = 0.0f;
    double s64 = 0.0;
    for (long long j0 = 0; j0 < longest; j0 += kAugChains) {
        const long long left = len - j0;
        const int m = left < kAugChains ? (left > 0 ? (int)left : 0) : kAugChains;
        if (m > 0) {
            const long long p = first + j0;                     // p < first + len: the walk ends inside the chain's pieces
            if (!CLIPS)
                while (piece_end <= p) { ++q; piece_end = a.piece_prefix[q + 1]; src_off = a.piece_src[q] - a.piece_prefix[q]; }
            const long long run = piece_end - p;
            sh.row_src[lane] = src_off + p; sh.row_pos[lane] = p; sh.piece[lane] = q;
            sh.row_run[lane] = run < m ? (int)run : m;
        }
        sh.row_n[lane] = m;
        __syncthreads();
        for (int c0 = 0; c0 < kAugChains; c0 += kAugStage) {    // row c: samples j0 .. j0 + 63 of chain c, one per lane
            float v[kAugStage];
#pragma unroll
            for (int u = 0; u < kAugStage; ++u) {
                const int c = c0 + u;
                v[u] = 0.0f;
                if (lane < sh.row_n[c]) {
                    long long index = sh.row_src[c] + lane;
                    if (!CLIPS && lane >= sh.row_run[c]) {
                        const long long p = sh.row_pos[c] + lane;
                        int w = sh.piece[c];
                        while (a.piece_prefix[w + 1] <= p) ++w;
                        index = a.piece_src[w] + (p - a.piece_prefix[w]);
                    }
                    v[u] = a.pool[index];
                }
            }
#pragma unroll
            for (int u = 0; u < kAugStage; ++u) sh.tile[(c0 + u) * kAugRowStride + lane] = v[u];
        }
        __syncthreads();
        // the whole row, whatever the chain has left: past its end the row holds zeros, and s + 0 * 0 is s -- a loop of fixed
        // length, so the LDS reads are issued ahead of the dependent adds instead of one read latency per sample
        const float* row = sh.tile + lane * kAugRowStride;
#pragma unroll
        for (int k = 0; k < kAugChains; ++k) {
            const float x = row[k];
            if (CLIPS) s32 = s32 + x * x;
            else s64 = s64 + (double)x * (double)x;
        }
        __syncthreads();                                        // every lane has read its row before the next ones arrive
    }
    if (chain < a.n) {
        if (CLIPS) a.sum_f32[chain] = s32;
        else { a.sum_f64[chain] = s64; a.zero[chain] = s64 == 0.0 ? 1 : 0; }
    }
}

// One thread per output sample of the pass, its piece found by binary search in the piece prefix (gen_mix's shape: once per
// block, the same search in every lane, then a short walk); consecutive threads read consecutive clip and noise samples.
//   adj = (va * n) / vn                                        audio_volume * noise_data / noise_volume, float64, in that order
//   out = ratio * adj + (double) fl32(keep * a)                noise_ratio * adjusted_noise + (1.0 - noise_ratio) * audio
//   q   = (int16_t)(int)(out * 32767.0)                        save_audio: astype(int16) truncates toward zero
//   reloaded = fl32(q) / 32767.0f                              load_audio
__device__ __forceinline__ void aug_mix(const AugMixArgs& a) {
#pragma clang fp contract(off)
    const long long p0 = (long long)blockIdx.x * kAugMixThreads;
    const long long p = p0 + threadIdx.x;
    if (p >= a.n) return;
    int lo = 0, hi = a.n_pieces;                                // invariant: prefix[lo] <= p0 < prefix[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.prefix[mid] <= p0) lo = mid; else hi = mid;
    }
    while (a.prefix[lo + 1] <= p) ++lo;                         // p < prefix[n_pieces] ends the walk
    const AugPiece piece = a.pieces[lo];
    const AugSlot slot = a.slots[piece.slot];
    const long long o = p - a.prefix[lo];
    const double adj = (slot.va * (double)a.noise[piece.noise + o]) / slot.vn;
    const double out = slot.ratio * adj + (double)(slot.keep * a.clips[piece.clip + o]);
    const double scaled = out * 32767.0;
    const int16_t q = (int16_t)(int)scaled;                     // mine_ring's cast; out of range it is whatever the cast gives
    if (a.overflowed && !(scaled > -32768.0 && scaled < 32768.0)) atomicAdd(a.overflowed + slot.copy, 1ull);
    if (a.mixed) a.mixed[p] = out;
    if (a.pcm) a.pcm[p] = q;
    if (a.reloaded) a.reloaded[p] = (float)q / 32767.0f;
}

#endif  // __HIPCC__

}  // namespace pe
