// Training of TWO stacked GRU layers, H1 and H2 units of 1..256 each, on the f32 matrix cores.  The network is
// Sequential[GRU(H1, return_sequences), GRU(H2), Dense(1, sigmoid)].  Every piece of a layer's step is that of
// gru_train_wide_device.h, instantiated per layer; this file holds what is layer 1's or the stack's own.
// Layer 1's input is h1_t, the state layer 0 has AFTER step t, under layer 1's own per-gate masks.
//
// A step of one network is nine launches:
//   ts_forward0  tw_steps with TwInputX, no head: layer 0's records.  h1_t is slot 0 of record t + 1; the state after the last
//                step goes to `hfin0` [tile][H1p][16].
//   ts_forward1  tw_steps with TsInputH1: ONE copy of h1_t [H1p][16] in LDS (two buffers: step t + 1 is fetched while step t
//                runs), the three masks [3][H1p][16] next to it, and the float32 product x * m formed where the B operand is
//                read.  Records [h_(t-1) | r h_(t-1) | z | r | c][H2p][16]; the masks of the tile go to `mtape` once (they
//                are the same for every timestep).  Ends with tw_head.
//   ts_pack      tw_pack three times: U0^T, U1^T (the recurrent products of the two chains) and W1^T (the A operand of dx_t)
//   ts_backward1 tw_backward<kWrite> over layer 1's records: dx_t goes out through W1^T under the tile's masks
//   ts_backward0 tw_backward<kRead> over layer 0's records: dx comes in
//   ts_gemm0     tw_gemm over layer 0's records
//   ts_gemm1     tw_gemm<BELOW>: the K = H1 input rows are h1_t m_gate, from layer 0's records and `mtape`
//   ts_reduce    tw_reduce over two layers: RMSprop under three frozen bits
// Forward only (evaluate, stats, sample_choose): ts_forward0<false> writes the sequence h1_0 .. h1_(T-1) to `hfin0`
// [tile][T][H1p][16] and ts_forward1<false> reads it; nothing else is written.  The sequence goes through HBM in both
// forms: one workgroup holding both layers would need both recurrent kernels' streams and both states at once.
//
// Padding is inert as in 4.15: units past H have zero weights, bias and dense weight (selected to zero where they are
// read), so state, delta and D are exact zeros there; samples past n read zero inputs and get ds = 0.  Every record, dx row
// and mask row of a launch is written in full before anything reads it.
#pragma once
#include "gru_train_wide_device.h"

namespace pe {

// key of layer 1's masks from the key of one (seed, step)
__host__ __device__ inline uint64_t train_mask_key_layer1(uint64_t key) { return train_mix64(key ^ kTrainGolden); }
// 1 = keep.  Layer 1: feature < 256
__host__ __device__ inline bool train_mask_keep_layer1(uint64_t key1, int gate, int64_t pos, int feature, float rate) {
    const uint64_t ctr = ((uint64_t)pos << 10) | ((uint64_t)gate << 8) | (uint64_t)feature;
    const uint64_t bits = train_mix64(key1 + kTrainGolden * (ctr + 1));
    return (float)(bits >> 40) * (1.0f / 16777216.0f) >= rate;
}

// flat order: kernel_0 | recurrent_kernel_0 | bias_0 | kernel_1[H1][3H2] | recurrent_kernel_1 | bias_1 | dense_kernel[H2] | dense_bias
__host__ __device__ inline int ts_n_params(int F, int H1, int H2) { return train_n_gru(F, H1) + train_n_gru(H1, H2) + H2 + 1; }

struct TrainStackedArgs {
    int n, T, F, H1, H1p, H2, H2p, n_tiles;
    int backward, apply, frozen_mask, mask_mode;
    float rate, keep_scale, beta, inv_n;
    float lr, rho, eps;
    uint64_t mask_key, mask_key1;
    float* theta;               // flat parameters of THIS network (and accum, grads)
    float* accum;
    float* grads;
    float* loss;                // [1]
    const float* feats;
    const float* targets;
    const int32_t* indices;
    const float* masks0;        // mask_mode 1: [3][n][F]
    const float* masks1;        //              [3][n][H1]
    float* tape0;               // [n_tiles T] records of tw_record(F, H1p)
    float* hfin0;               // backward: [n_tiles][H1p][16]; forward only: [n_tiles T][H1p][16]
    float* tape1;               // [n_tiles T] records of tw_record(0, H2p)
    float* mtape;               // [n_tiles][3][H1p][16]
    float* dx;                  // [n_tiles T][H1p][16]
    float* fin;                 // [n_tiles][H2p][16]
    float* ut0;                 // [3][H1p][H1p]
    float* ut1;                 // [3][H2p][H2p]
    float* w1t;                 // [3][H2p][H1p]
    float* partial;             // [n_tiles][H2 + 3]
    float* gpart0;              // [chunks][train_n_gru(F, H1)]
    float* gpart1;              // [chunks][train_n_gru(H1, H2)]
    float* probs;               // [n]
};

hipError_t launch_train_stacked(const TrainStackedArgs& a, hipStream_t s);
hipError_t launch_train_stacked_apply(const TrainStackedArgs& a, hipStream_t s);      // a.grads is read
size_t ts_forward1_lds(int H1p, int H2p);                                            // bytes
size_t ts_backward1_lds(int H1p, int H2p);

#if defined(__HIPCC__)

// ---- layer 1 ------------------------------------------------------------------------------------------------------------
// LDS in floats: HT[H2p 16] | RHT[H2p 16] | X[2][H1p 16] | MS[3][H1p 16] | SC[kTwMaxWaves 16 + 48]
__host__ __device__ inline int ts_forward1_lds_floats(int H1p, int H2p) { return 2 * H2p * 16 + 5 * H1p * 16 + kTwMaxWaves * 16 + 48; }
__host__ __device__ inline int ts_backward1_lds_floats(int H1p, int H2p) { return 3 * H2p * 16 + 3 * H1p * 16; }
constexpr int kTsPrefetch = 4;          // float4 of h1_(t+1) a thread holds in registers over a step

__device__ inline TwLayer ts_layer0(const TrainStackedArgs& a) {
    return tw_layer(a.theta, a.F, a.H1, a.H1p, tw_record(a.F, a.H1p), a.tape0, a.ut0, a.gpart0);
}
__device__ inline TwLayer ts_layer1(const TrainStackedArgs& a) {
    return tw_layer(a.theta + train_n_gru(a.F, a.H1), a.H1, a.H2, a.H2p, tw_record(0, a.H2p), a.tape1, a.ut1, a.gpart1);
}

// The input policy of layer 1: h1_t [Kp][16] of the tile in LDS, X[2], prefetched one step ahead through registers, and the
// masks MS[3][Kp][16] (also written to `mtape`); x * m is formed on read.
template <bool BACKWARD>
struct TsInputH1 {
    const TrainStackedArgs& a;
    const TwLayer& l;
    const TwThread& th;
    float* X;
    float* MS;
    const float* x;
    f32x4* xnext;
    const f32x4* nsrc;
    f32x4 pf[kTsPrefetch];

    // h1_t [Kp][16]: slot 0 of layer 0's record t + 1, the final state, or row t of the sequence
    __device__ const f32x4* xsrc(int t) const {
        const int T = a.T, Kp = a.H1p, tile = th.tile;
        const float* p;
        if (BACKWARD) p = t + 1 < T ? a.tape0 + ((size_t)tile * T + t + 1) * tw_record(a.F, Kp) : a.hfin0 + (size_t)tile * Kp * 16;
        else p = a.hfin0 + ((size_t)tile * T + t) * Kp * 16;
        return reinterpret_cast<const f32x4*>(p);
    }
    __device__ void masks_init() {
        const int K = a.H1, Kp = a.H1p, tid = th.tid, nt = th.nt, tile = th.tile, first = th.first;
        for (int i = tid; i < 3 * Kp * 16; i += nt) {
            const int g = i / (Kp * 16), k = (i / 16) % Kp, s2 = i % 16;
            const int smp = first + s2;
            float m = 1.0f;
            if (smp < a.n && k < K) {
                if (a.mask_mode == 1) m = a.masks1[((size_t)g * a.n + smp) * K + k];
                else if (a.mask_mode == 2) m = train_mask_keep_layer1(a.mask_key1, g, smp, k, a.rate) ? a.keep_scale : 0.0f;
            }
            MS[i] = m;
            if (BACKWARD) a.mtape[(size_t)tile * 3 * Kp * 16 + i] = m;
        }
    }
    __device__ void stage_first() {
        const int xq = a.H1p * 4;                         // float4 of one h1_t
        const f32x4* src = xsrc(0);
        for (int e = th.tid; e < xq; e += th.nt) reinterpret_cast<f32x4*>(X)[e] = src[e];
    }
    __device__ void fetch(int t) {
        const int Kp = a.H1p, xq = Kp * 4;
        x = X + (t & 1) * Kp * 16;
        xnext = reinterpret_cast<f32x4*>(X + ((t + 1) & 1) * Kp * 16);
        nsrc = t + 1 < a.T ? xsrc(t + 1) : nullptr;
#pragma unroll
        for (int q = 0; q < kTsPrefetch; ++q) {
            const int e = th.tid + q * th.nt;
            pf[q] = (nsrc && e < xq) ? nsrc[e] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __device__ void add_zr(f32x4& az, f32x4& ar, bool aok, int uc) const {
#pragma clang fp contract(off)
        const int K = a.H1, Kp = a.H1p, H = a.H2, H3 = 3 * H, gq = th.gq, j = th.j;
        const float* const MZ = MS;
        const float* const MR = MS + Kp * 16;
        const float* wp = l.W + uc;
        for (int k16 = 0; k16 < Kp; k16 += 16)
#pragma unroll
        for (int k0 = k16; k0 < k16 + 16; k0 += 4) {
            const int k = k0 + gq;
            const bool ok = aok && k < K;
            const int kc = k < K ? k : K - 1;
            const float wz = wp[kc * H3], wr = wp[kc * H3 + H];
            const float xv = x[k * 16 + j];
            az = mfma(ok ? wz : 0.0f, xv * MZ[k * 16 + j], az);
            ar = mfma(ok ? wr : 0.0f, xv * MR[k * 16 + j], ar);
        }
    }
    __device__ void add_c(f32x4& ac, bool aok, int uc) const {
#pragma clang fp contract(off)
        const int K = a.H1, Kp = a.H1p, H = a.H2, H3 = 3 * H, gq = th.gq, j = th.j;
        const float* const MH = MS + 2 * Kp * 16;
        const float* wp = l.W + 2 * H + uc;
        for (int k16 = 0; k16 < Kp; k16 += 16)
#pragma unroll
        for (int k0 = k16; k0 < k16 + 16; k0 += 4) {
            const int k = k0 + gq;
            const int kc = k < K ? k : K - 1;
            const float wh = wp[kc * H3];
            ac = mfma(aok && k < K ? wh : 0.0f, x[k * 16 + j] * MH[k * 16 + j], ac);
        }
    }
    __device__ void stage_next(int, float*) const {
        const int xq = a.H1p * 4, tid = th.tid, nt = th.nt;
        if (nsrc) {
#pragma unroll
            for (int q = 0; q < kTsPrefetch; ++q) {
                const int e = tid + q * nt;
                if (e < xq) xnext[e] = pf[q];
            }
            for (int e = tid + kTsPrefetch * nt; e < xq; e += nt) xnext[e] = nsrc[e];      // a narrow layer 1 under a wide layer 0
        }
    }
    __device__ float* hout(int) const { return nullptr; }
};

template <bool BACKWARD>
__device__ inline void ts_forward0(const TrainStackedArgs& a, float* HT, float* RHT, float* XM, float* MS) {
    const TwThread th;
    const TwLayer l = ts_layer0(a);
    TwInputX<TrainStackedArgs, BACKWARD, true, true> in{a, l, th, a.masks0, a.mask_key, a.hfin0, XM, MS};
    float hown[2][4];
    tw_steps<BACKWARD>(a.T, l, th, in, HT, RHT, hown);
}

template <bool BACKWARD>
__device__ inline void ts_forward1(const TrainStackedArgs& a, float* lds) {
    const int Kp = a.H1p, Hp = a.H2p;
    const TwThread th;
    const TwLayer l = ts_layer1(a);
    float* const HT = lds;
    float* const RHT = HT + Hp * 16;
    float* const X = RHT + Hp * 16;
    float* const MS = X + 2 * Kp * 16;
    float* const SC = MS + 3 * Kp * 16;
    TsInputH1<BACKWARD> in{a, l, th, X, MS};
    float hown[2][4];
    tw_steps<BACKWARD>(a.T, l, th, in, HT, RHT, hown);
    tw_head<BACKWARD>(a, l, th, a.fin, a.partial, hown, HT, SC);
}

// UT0 [3][H1p][H1p], UT1 [3][H2p][H2p], W1T [3][H2p][H1p]: one thread per element
__device__ inline void ts_pack(const TrainStackedArgs& a) {
    const TwLayer l0 = ts_layer0(a), l1 = ts_layer1(a);
    const int n0 = 3 * l0.Hp * l0.Hp, n1 = 3 * l1.Hp * l1.Hp, n2 = 3 * l1.Hp * l0.Hp;
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n0) return tw_pack(l0.ut, l0.U, e, l0.H, l0.Hp, l0.H, l0.Hp);
    e -= n0;
    if (e < n1) return tw_pack(l1.ut, l1.U, e, l1.H, l1.Hp, l1.H, l1.Hp);
    e -= n1;
    if (e < n2) tw_pack(a.w1t, l1.W, e, l1.K, l0.Hp, l1.H, l1.Hp);
}

__device__ inline void ts_apply(const TrainStackedArgs& a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ts_n_params(a.F, a.H1, a.H2)) return;
    const TwLayer l0 = ts_layer0(a), l1 = ts_layer1(a);
    const TwLayer* const l[2] = {&l0, &l1};
    if (!((a.frozen_mask >> tw_layer_of(l, e)) & 1)) train_rmsprop(a.theta[e], a.accum[e], a.grads[e], a.lr, a.rho, a.eps);
}

#endif  // __HIPCC__

}  // namespace pe
