// Mining false activations on the device (pe_miner): what precise-train-incremental does per chunk
// (scripts/train_incremental.py:113-137) for every chunk of many recordings at once.
//
// The recordings' frames exist once, as float32 rows (the front-end launch of pe_evaluate_clips writes them when the
// session is created); the three kernels here are the seams between those rows, the network and the trainer:
//   mine_gather     the network input Listener.update would have after chunk i (network_runner.py:125-152): a closed form of
//                   the chunk index gives the last emitted frame, the n_features rows before it are copied into an
//                   [n][T][F] batch (literal zero rows where the recording is still too short, network_runner.py:104) that
//                   pe_predict_device scores -- the scan is pe_predict's arithmetic by construction;
//   mine_count / mine_scan_counts / mine_write
//                   `conf > threshold` (train_incremental.py:125; float64, strict) over all predictions and the ascending ids
//                   of the hits: ballot + popcount inside a wave, the waves' totals inside a block, a prefix sum over the
//                   blocks' counts -- positions are computed, never raced for, so the ids come out in order;
//   mine_ring       the audio script saves at a hit (train_incremental.py:79,123,130): the last buffer_samples samples of
//                   all chunks yielded so far -- over earlier recordings too, the ring is never cleared -- through
//                   save_audio / load_audio's int16 round trip (util.py:65,71), as float32 clips for the clip front end
//                   (pe_vectorize_clips' launch: there is no second MFCC).
// Everything is indexed by GLOBAL chunk ids: recording r's chunk i is id chunk_prefix[r] + i, chunk_prefix being the
// exclusive prefix sum of the chunk counts (util.py:30-32: (len - 1) / chunk whole chunks, the last one never ends the file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pe {

constexpr int kMineThreads = 256;           // threads of a compaction block: four waves
constexpr int kMineItems = 16;              // predictions per thread: a block owns 4096 consecutive predictions

struct MineGatherArgs {
    const float* rows;              // [frames of all recordings][row_floats]; recording r's frame 0 is row frame_base[r]
    const long long* chunk_prefix;  // [n_rec + 1]; null: window v is rows [v T, v T + T) as they are (the clip front end's
                                    // padded windows, mine_ring's way into the trainer)
    const long long* frame_base;    // [n_rec + 1] exclusive prefix sum of the recordings' frame counts
    int n_rec;
    long long first;                // global id of window 0 of this launch
    int n;                          // windows of this launch
    int chunk, emit_window, hop;    // emit_window: samples behind the first frame (window; + hop with speechpy)
    int T, F, use_delta, row_floats;
    float* out;                     // [n][T][F], with use_delta [n][T][2 F]: x_t, x_t - x_(t-1) (0 in the first row)
    const int32_t* ids;             // [n] global id of every window (any order, repeats allowed), or null: first + v
};

struct MineCompactArgs {
    const float* raw;               // [n] predictions
    const double* conf;             // [n] decoded predictions (pe_decode's kernel wrote them), or null: (double)raw
    long long n;
    double threshold;
    long long first;                // global id of prediction 0
    uint32_t* block_counts;         // [n_blocks + 1]: hits per block; after mine_scan_counts their exclusive prefix sum,
                                    // [n_blocks] the total
    int n_blocks;
    int32_t* hits;                  // [capacity] ascending global ids of the first `capacity` hits
    long long capacity;
};

struct MineRingArgs {
    const int32_t* hits;            // [n] global chunk ids
    int n;
    const long long* chunk_prefix;  // [n_rec + 1]
    const long long* rec_start;     // [n_rec + 1] first sample of every recording in `audio`
    int n_rec;
    int chunk, buffer_samples;
    int carry_audio;                // 1: the script's ring, filled by every chunk since the start; 0: zeros before the
                                    // recording's own start
    const void* audio;              // float64 or float32 samples (widened: exact)
    int audio_f32;
    float* out;                     // [n][buffer_samples]
};

hipError_t launch_mine_gather(const MineGatherArgs& a, hipStream_t s);
hipError_t launch_mine_compact(const MineCompactArgs& a, hipStream_t s);      // the three compaction kernels in order
hipError_t launch_mine_ring(const MineRingArgs& a, hipStream_t s);
inline int mine_blocks(long long n) { return (int)((n + (long long)kMineThreads * kMineItems - 1) / ((long long)kMineThreads * kMineItems)); }

#if defined(__HIPCC__)

// r with prefix[r] <= g < prefix[r + 1] (a recording without a chunk is never found: its range is empty); 0 <= g < prefix[n]
__device__ __forceinline__ int mine_recording_of(const long long* prefix, const int n, const long long g) {
    int lo = 0, hi = n;                                         // invariant: prefix[lo] <= g < prefix[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// One wave per window.  After chunk i of its recording n = (i + 1) chunk samples have arrived and E(n) = 1 + (n - emit_window) / hop
// frames have been emitted (0 below one window; network_runner.py:137-144); the window is frames E - T .. E - 1, and frames
// before the recording's first are the zero rows a cleared Listener starts with.
__device__ __forceinline__ void mine_gather(const MineGatherArgs& a) {
    const int v = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (v >= a.n) return;
    long long base;             // row of the window's first timestep (may lie before row0)
    long long row0;             // first row that exists
    if (a.chunk_prefix) {
        const long long g = a.ids ? (long long)a.ids[v] : a.first + v;
        const int r = mine_recording_of(a.chunk_prefix, a.n_rec, g);
        const long long n = (g - a.chunk_prefix[r] + 1) * (long long)a.chunk;
        const long long emitted = n >= a.emit_window ? 1 + (n - a.emit_window) / a.hop : 0;
        row0 = a.frame_base[r];
        base = row0 + emitted - a.T;
    } else {
        row0 = (long long)v * a.T;
        base = row0;
    }
    const int width = a.use_delta ? 2 * a.F : a.F;
    float* const out = a.out + (size_t)v * a.T * width;
    for (int i = lane; i < a.T * a.F; i += 64) {
        const int t = i / a.F, f = i - t * a.F;
        const long long row = base + t;
        const float x = row >= row0 ? a.rows[row * a.row_floats + f] : 0.0f;
        out[t * width + f] = x;
        if (a.use_delta) {
            const float before = (t > 0 && row - 1 >= row0) ? a.rows[(row - 1) * a.row_floats + f] : 0.0f;
            out[t * width + a.F + f] = t > 0 ? x - before : 0.0f;
        }
    }
}

__device__ __forceinline__ bool mine_is_hit(const MineCompactArgs& a, const long long i) {
    if (i >= a.n) return false;
    const double v = a.conf ? a.conf[i] : (double)a.raw[i];
    return v > a.threshold;                                     // train_incremental.py:125 (a NaN never fires)
}
// position of this thread's flag among the set flags of its block, in thread order, and the block's count; wave_total: LDS [4]
__device__ __forceinline__ uint32_t mine_block_rank(const bool flag, uint32_t* wave_total, uint32_t* block_total) {
    const unsigned long long ballot = __ballot(flag);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const uint32_t below = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    __syncthreads();                                            // the previous round's totals have been read
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < kMineThreads / 64; ++w) {
        const uint32_t c = wave_total[w];
        if (w < wave) before += c;
        total += c;
    }
    *block_total = total;
    return before + below;
}
// pass 1: hits of the block's predictions.  pass 2 (hits != null after the scan): the same walk, now with the block's offset
template <bool WRITE>
__device__ __forceinline__ void mine_block_walk(const MineCompactArgs& a, uint32_t* wave_total) {
    const long long base = (long long)blockIdx.x * kMineThreads * kMineItems;
    uint32_t running = WRITE ? a.block_counts[blockIdx.x] : 0u;
    for (int it = 0; it < kMineItems; ++it) {
        const long long i = base + (long long)it * kMineThreads + threadIdx.x;
        const bool flag = mine_is_hit(a, i);
        uint32_t total;
        const uint32_t rank = mine_block_rank(flag, wave_total, &total);
        if (WRITE && flag && (long long)(running + rank) < a.capacity) a.hits[running + rank] = (int32_t)(a.first + i);
        running += total;
    }
    if (!WRITE && threadIdx.x == 0) a.block_counts[blockIdx.x] = running;
}
// one wave: the exclusive prefix sum of the blocks' counts, 64 at a time (at most 2^31 - 1 hits: 32 bits hold every sum)
__device__ __forceinline__ void mine_scan_counts(const MineCompactArgs& a) {
    const int lane = (int)threadIdx.x;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < a.n_blocks; b0 += 64) {
        const int b = b0 + lane;
        const uint32_t v = b < a.n_blocks ? a.block_counts[b] : 0u;
        uint32_t sum = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(sum, d);
            if (lane >= d) sum += up;
        }
        if (b < a.n_blocks) a.block_counts[b] = carry + sum - v;
        carry += __shfl(sum, 63);
    }
    if (lane == 0) a.block_counts[a.n_blocks] = carry;
}

// One thread per ring sample.  With carry_audio the ring after global chunk g is positions [(g + 1) chunk - buffer, (g + 1) chunk)
// of the concatenation of ALL chunks in id order (position p lies in chunk p / chunk, found in the prefix sum -- a ring can
// span several short recordings), zeros before position 0; without, the same inside the hit's own recording.
// save_audio: (audio * 32767).astype(int16) on the float64 ring (truncation toward zero); load_audio: float32(q) / 32767.
__device__ __forceinline__ void mine_ring(const MineRingArgs& a) {
    const int h = (int)blockIdx.y;
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= a.buffer_samples) return;
    const long long g = a.hits[h];
    long long index = -1;                                       // sample in `audio`; -1: a zero of the fresh ring
    if (a.carry_audio) {
        const long long pos = (g + 1) * (long long)a.chunk - a.buffer_samples + p;
        if (pos >= 0) {
            const long long gc = pos / a.chunk;
            const int r = mine_recording_of(a.chunk_prefix, a.n_rec, gc);
            index = a.rec_start[r] + (gc - a.chunk_prefix[r]) * (long long)a.chunk + (pos - gc * (long long)a.chunk);
        }
    } else {
        const int r = mine_recording_of(a.chunk_prefix, a.n_rec, g);
        const long long pos = (g - a.chunk_prefix[r] + 1) * (long long)a.chunk - a.buffer_samples + p;
        if (pos >= 0) index = a.rec_start[r] + pos;
    }
    double x = 0.0;
    if (index >= 0) x = a.audio_f32 ? (double)static_cast<const float*>(a.audio)[index] : static_cast<const double*>(a.audio)[index];
    const int16_t q = (int16_t)(int)(x * 32767.0);              // (int): truncation toward zero, as astype does
    a.out[(size_t)h * a.buffer_samples + p] = __fdiv_rn((float)q, 32767.0f);
}

#endif  // __HIPCC__

}  // namespace pe
