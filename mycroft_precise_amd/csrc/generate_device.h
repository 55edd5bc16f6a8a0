// Generating training audio on the device (pe_generator): what precise-train-generated does per chunk
// (scripts/train_generated.py:118-202) for every sample of many background files at once.
//
// The host planner (generated.py) has turned the script's random draws and its piece stream into SEGMENTS: consecutive runs
// of output samples that overlay one stretch of one wake-word / not-wake-word clip -- or silence -- on the background.  The
// segments of a plan tile its output without gaps, file after file, so ONE exclusive prefix sum over all segments maps an
// output position to its segment, and the segment carries where its background and clip samples start.  gen_mix is the only
// kernel: the numpy arithmetic of normalize_volume_to / layer_with / merge, to the bit.  Its float64 output feeds the
// recording front end (launch_rec_front_end) like any resident audio; windows and trainer rows come from mine_gather.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pe {

constexpr int kGenThreads = 256;

struct GenSeg {
    long long clip;         // index in the clip pool of the segment's first sample; -1: silence
    long long bg;           // index in the background pool of the sample under the segment's first sample
    float volume;           // (float)audio_volume of the file: numpy rounds the Python scalar to the array's type
    float rms_bg;           // (float)rms of the background
    float rms_clip;         // (float)rms of the clip (unused in silence)
    float pad;
};

struct GenMixArgs {
    const float* bg;                // background pool
    const float* clips;             // clip pool
    const GenSeg* segs;             // [segments of the plan]
    const long long* seg_prefix;    // [segments + 1] exclusive prefix sum of the segment lengths: output positions of the plan
    int seg_lo, seg_hi;             // the segments this launch can meet: seg_prefix[seg_lo] <= first, first + n <= seg_prefix[seg_hi]
    long long first;                // output position of sample 0 of this launch
    long long n;                    // samples of this launch
    float keep;                     // (float)(1.0 - 0.6): merge's weight of the background, a float32 product
    double* out;                    // [n]
};

hipError_t launch_gen_mix(const GenMixArgs& a, hipStream_t s);

#if defined(__HIPCC__)

// One thread per output sample, its segment found by binary search in the segment prefix (mine_recording_of's shape, once
// per block) and a short walk; consecutive threads read consecutive background and clip samples and write consecutive
// doubles.  Every operation is spelled with an _rn intrinsic: the compiler contracts a * b + c by default, and a fused
// multiply-add here is another number than numpy's.
//   background  b = fl32(fl32(volume * s) / rms_bg)                 volume * sample / calc_volume(sample), float32 throughout
//   overlay     w = (double) fl32(fl32(volume * c) / rms_clip)      the same on the clip, widened by layer_with; 0.0 in silence
//   merge       out = (double) fl32(keep * b) + 0.6 * w             (1.0 - ratio) * a float32, ratio * b and the sum float64
__device__ __forceinline__ void gen_mix(const GenMixArgs& a) {
    const long long i = (long long)blockIdx.x * kGenThreads + threadIdx.x;
    if (i >= a.n) return;
    // the segment of the block's first sample: the same search in every lane, so its loads are the block's, not the lane's ...
    const long long p0 = a.first + (long long)blockIdx.x * kGenThreads;
    int lo = a.seg_lo, hi = a.seg_hi;                           // invariant: seg_prefix[lo] <= p0 < seg_prefix[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.seg_prefix[mid] <= p0) lo = mid; else hi = mid;
    }
    // ... and from there forward to the lane's own (p < seg_prefix[seg_hi] ends the walk; a segment is rarely shorter than a block)
    const long long p = p0 + threadIdx.x;
    while (a.seg_prefix[lo + 1] <= p) ++lo;
    const GenSeg seg = a.segs[lo];
    const long long o = p - a.seg_prefix[lo];
    const float b = __fdiv_rn(__fmul_rn(seg.volume, a.bg[seg.bg + o]), seg.rms_bg);
    double w = 0.0;
    if (seg.clip >= 0) w = (double)__fdiv_rn(__fmul_rn(seg.volume, a.clips[seg.clip + o]), seg.rms_clip);
    a.out[i] = __dadd_rn((double)__fmul_rn(a.keep, b), __dmul_rn(0.6, w));
}

#endif  // __HIPCC__

}  // namespace pe
