// Training of TWO stacked GRU layers, H1 and H2 units of 1..256 each, on the f32 matrix cores.  The network is
// Sequential[GRU(H1, return_sequences), GRU(H2), Dense(1, sigmoid)]; per layer the arithmetic contract is that of
// gru_train_device.h and the layout that of gru_train_wide_device.h: the problem transposed,
// v_mfma_f32_16x16x4_f32 over tiles of 16 samples, weights the A operand from L2, per-sample operands the B operand from LDS
// as [k][16 samples].  Layer 1's input is h1_t, the state layer 0 has AFTER step t, under layer 1's own per-gate masks.
//
// A step of one network is nine launches:
//   ts_forward0  tw_forward without a head: layer 0's records [h_(t-1) | r h_(t-1) | z | r | c][H1p][16] | x m [3][F][16].  h1_t
//                is slot 0 of record t + 1; the state after the last step goes to `hfin0` [tile][H1p][16].
//   ts_forward1  layer 1 over the tile: ONE copy of h1_t [H1p][16] in LDS (two buffers: step t + 1 is fetched while step t
//                runs), the three masks [3][H1p][16] next to it, and the float32 product x * m formed where the B operand is
//                read.  Records [h_(t-1) | r h_(t-1) | z | r | c][H2p][16]; the masks of the tile go to `mtape` once (they
//                are the same for every timestep).  Ends with tw_forward's head, loss sums, dense partials and delta_T.
//   ts_pack      U0^T, U1^T (the recurrent products of the two chains) and W1^T [gate][u][k] (the A operand of dx_t)
//   ts_backward<1>  4.15's chain over layer 1's records, plus dx_t = m_z (D_z W_z^T) + m_r (D_r W_r^T) + m_h (D_h W_h^T) as
//                three MFMA chains per 16-row tile of H1p, written per (tile, t) as [H1p][16]
//   ts_backward<0>  4.15's chain over layer 0's records; delta starts as dx_(T-1) and dx_(t-1) is added after the recurrent
//                terms of step t
//   tw_gemm      layer 0's weight gradients, the wide path's function on layer 0's records
//   ts_gemm1     layer 1's: the left operand rows are h1_t m_gate (H1 rows: h1_t from layer 0's records, multiplied by the
//                tile's mask as it is loaded), h_(t-1) or r h_(t-1) (H2 rows) and ones; 4.15's chunking rule
//   ts_reduce    chunk partials in chunk order, dense / loss partials in tile order, RMSprop under three frozen bits
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

// ---- layer 0: tw_forward without a head ------------------------------------------------------------------------------------
template <bool BACKWARD>
__device__ inline void ts_forward0(const TrainStackedArgs& a, float* HT, float* RHT, float* XM, float* MS) {
#pragma clang fp contract(off)
    const int T = a.T, F = a.F, H = a.H1, Hp = a.H1p, H3 = 3 * H, NT = Hp / 16;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
    const int gq = lane >> 4, j = lane & 15;
    const int tile = blockIdx.x, first = tile * 16;
    const float* const W = a.theta;
    const float* const U = W + F * H3;
    const float* const Bv = U + H * H3;
    const size_t rec_floats = tw_record(F, Hp);
    const int oRH = Hp * 16, oZ = 2 * Hp * 16, oR = 3 * Hp * 16, oC = 4 * Hp * 16, oX = 5 * Hp * 16;

    for (int i = tid; i < 3 * F * 16; i += nt) {
        const int g = i / (F * 16), f = (i / 16) % F, s2 = i % 16;
        const int smp = first + s2;
        float m = 1.0f;
        if (smp < a.n) {
            if (a.mask_mode == 1) m = a.masks0[((size_t)g * a.n + smp) * F + f];
            else if (a.mask_mode == 2) m = train_mask_keep(a.mask_key, g, smp, f, a.rate) ? a.keep_scale : 0.0f;
        }
        MS[i] = m;
    }
    for (int i = tid; i < Hp * 16; i += nt) HT[i] = 0.0f;
    const float* xrow[3];
    int xdst[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int e = tid + q * nt;
        xrow[q] = nullptr;
        xdst[q] = -1;
        if (e < 16 * F) {
            const int s2 = e / F, f = e % F, smp = first + s2;
            xdst[q] = f * 16 + s2;
            if (smp < a.n) {
                const size_t r = a.indices ? (size_t)a.indices[smp] : (size_t)smp;
                xrow[q] = a.feats + r * (size_t)T * F + f;
            }
        }
    }
    __syncthreads();
    // a block of one wave (H1 <= 16) stages 16 F <= 512 elements with 64 threads: more than three per thread
    const bool few = 3 * nt < 16 * F;
    auto stage_all = [&](int t, float* dst) {              // the slow form: every element through a loop
        for (int e = tid; e < 16 * F; e += nt) {
            const int s2 = e / F, f = e % F, smp = first + s2;
            float x = 0.0f;
            if (smp < a.n) {
                const size_t r = a.indices ? (size_t)a.indices[smp] : (size_t)smp;
                x = a.feats[r * (size_t)T * F + (size_t)t * F + f];
            }
            for (int g = 0; g < 3; ++g) dst[g * F * 16 + f * 16 + s2] = x * MS[g * F * 16 + f * 16 + s2];
        }
    };
    if (few) stage_all(0, XM);
    else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (xdst[q] >= 0) {
                const float x = xrow[q] ? xrow[q][0] : 0.0f;
                for (int g = 0; g < 3; ++g) XM[g * F * 16 + xdst[q]] = x * MS[g * F * 16 + xdst[q]];
            }
    }

    float bz[2][4], br[2][4], bh[2][4], hown[2][4], zown[2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int u = 16 * (wave + jj * nw) + 4 * gq + reg;
            const bool ok = u < H;
            bz[jj][reg] = ok ? Bv[u] : 0.0f;
            br[jj][reg] = ok ? Bv[H + u] : 0.0f;
            bh[jj][reg] = ok ? Bv[2 * H + u] : 0.0f;
            hown[jj][reg] = 0.0f;
            zown[jj][reg] = 0.0f;
        }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float* xm = XM + (t & 1) * kTwLdsX;
        float* const xmn = XM + ((t + 1) & 1) * kTwLdsX;
        float* const rec = BACKWARD ? a.tape0 + ((size_t)tile * T + t) * rec_floats : nullptr;
        // where h1_t goes besides the next record: the sequence (forward only) or the final state
        float* const hout = BACKWARD ? (t + 1 == T ? a.hfin0 + (size_t)tile * Hp * 16 : nullptr)
                                     : a.hfin0 + ((size_t)tile * T + t) * Hp * 16;
        float xn[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) xn[q] = (!few && t + 1 < T && xrow[q]) ? xrow[q][(size_t)(t + 1) * F] : 0.0f;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ua = 16 * tau + j;
            const bool aok = ua < H;
            const int uc = aok ? ua : H - 1;
            f32x4 az, ar;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) { az[reg] = bz[jj][reg]; ar[reg] = br[jj][reg]; }
            for (int k0 = 0; k0 < F; k0 += 4) {
                const int k = k0 + gq;
                const bool ok = aok && k < F;
                const int kc = k < F ? k : F - 1;
                const float wz = W[kc * H3 + uc], wr = W[kc * H3 + H + uc];
                const float xz = xm[kc * 16 + j], xr = xm[(F + kc) * 16 + j];
                az = mfma(ok ? wz : 0.0f, k < F ? xz : 0.0f, az);
                ar = mfma(ok ? wr : 0.0f, k < F ? xr : 0.0f, ar);
            }
            const float* up = U + uc;
            for (int k16 = 0; k16 < Hp; k16 += 16)
#pragma unroll
            for (int k0 = k16; k0 < k16 + 16; k0 += 4) {
                const int k = k0 + gq;
                const bool ok = aok && k < H;
                const int kc = k < H ? k : H - 1;
                const float wz = up[kc * H3], wr = up[kc * H3 + H];
                const float hb = HT[k * 16 + j];
                az = mfma(ok ? wz : 0.0f, hb, az);
                ar = mfma(ok ? wr : 0.0f, hb, ar);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                const float z = hard_sigmoid(az[reg]), r = hard_sigmoid(ar[reg]);
                const float hp = hown[jj][reg], rh = r * hp;
                zown[jj][reg] = z;
                RHT[idx] = rh;
                if (BACKWARD) { rec[idx] = hp; rec[oRH + idx] = rh; rec[oZ + idx] = z; rec[oR + idx] = r; }
            }
        }
        if (BACKWARD)
            for (int i = tid; i < 3 * F * 16; i += nt) rec[oX + i] = xm[i];
        if (few) {
            if (t + 1 < T) stage_all(t + 1, xmn);
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (xdst[q] >= 0)
                    for (int g = 0; g < 3; ++g) xmn[g * F * 16 + xdst[q]] = xn[q] * MS[g * F * 16 + xdst[q]];
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ua = 16 * tau + j;
            const bool aok = ua < H;
            const int uc = aok ? ua : H - 1;
            f32x4 ac;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) ac[reg] = bh[jj][reg];
            for (int k0 = 0; k0 < F; k0 += 4) {
                const int k = k0 + gq;
                const int kc = k < F ? k : F - 1;
                const float wh = W[kc * H3 + 2 * H + uc];
                const float xh = xm[(2 * F + kc) * 16 + j];
                ac = mfma(aok && k < F ? wh : 0.0f, k < F ? xh : 0.0f, ac);
            }
            const float* up = U + 2 * H + uc;
            for (int k16 = 0; k16 < Hp; k16 += 16)
#pragma unroll
            for (int k0 = k16; k0 < k16 + 16; k0 += 4) {
                const int k = k0 + gq;
                const int kc = k < H ? k : H - 1;
                const float wh = up[kc * H3];
                ac = mfma(aok && k < H ? wh : 0.0f, RHT[k * 16 + j], ac);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                const float hn = gru_blend(zown[jj][reg], hown[jj][reg], ac[reg]);
                hown[jj][reg] = hn;
                HT[idx] = hn;
                if (BACKWARD) rec[oC + idx] = ac[reg];
                if (hout) hout[idx] = hn;
            }
        }
        __syncthreads();
    }
}

// ---- layer 1 ------------------------------------------------------------------------------------------------------------
// LDS in floats: HT[H2p 16] | RHT[H2p 16] | X[2][H1p 16] | MS[3][H1p 16] | SC[kTwMaxWaves 16 + 48]
__host__ __device__ inline int ts_forward1_lds_floats(int H1p, int H2p) { return 2 * H2p * 16 + 5 * H1p * 16 + kTwMaxWaves * 16 + 48; }
constexpr int kTsPrefetch = 4;          // float4 of h1_(t+1) a thread holds in registers over a step

template <bool BACKWARD>
__device__ inline void ts_forward1(const TrainStackedArgs& a, float* lds) {
#pragma clang fp contract(off)
    const int T = a.T, K = a.H1, Kp = a.H1p, H = a.H2, Hp = a.H2p, H3 = 3 * H, NT = Hp / 16;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
    const int gq = lane >> 4, j = lane & 15;
    const int tile = blockIdx.x, first = tile * 16;
    float* const HT = lds;
    float* const RHT = HT + Hp * 16;
    float* const X = RHT + Hp * 16;
    float* const MS = X + 2 * Kp * 16;
    float* const SC = MS + 3 * Kp * 16;
    const float* const W = a.theta + train_n_gru(a.F, a.H1);
    const float* const U = W + K * H3;
    const float* const Bv = U + H * H3;
    const float* const WD = Bv + H3;
    const size_t rec_floats = tw_record(0, Hp), rec0 = tw_record(a.F, Kp);
    const int oRH = Hp * 16, oZ = 2 * Hp * 16, oR = 3 * Hp * 16, oC = 4 * Hp * 16;
    const int xq = Kp * 4;                                 // float4 of one h1_t

    // h1_t [Kp][16]: slot 0 of layer 0's record t + 1, the final state, or row t of the sequence
    auto xsrc = [&](int t) -> const f32x4* {
        const float* p;
        if (BACKWARD) p = t + 1 < T ? a.tape0 + ((size_t)tile * T + t + 1) * rec0 : a.hfin0 + (size_t)tile * Kp * 16;
        else p = a.hfin0 + ((size_t)tile * T + t) * Kp * 16;
        return reinterpret_cast<const f32x4*>(p);
    };

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
    for (int i = tid; i < Hp * 16; i += nt) HT[i] = 0.0f;
    {
        const f32x4* src = xsrc(0);
        for (int e = tid; e < xq; e += nt) reinterpret_cast<f32x4*>(X)[e] = src[e];
    }

    float bz[2][4], br[2][4], bh[2][4], hown[2][4], zown[2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int u = 16 * (wave + jj * nw) + 4 * gq + reg;
            const bool ok = u < H;
            bz[jj][reg] = ok ? Bv[u] : 0.0f;
            br[jj][reg] = ok ? Bv[H + u] : 0.0f;
            bh[jj][reg] = ok ? Bv[2 * H + u] : 0.0f;
            hown[jj][reg] = 0.0f;
            zown[jj][reg] = 0.0f;
        }
    __syncthreads();

    const float* const MZ = MS;
    const float* const MR = MS + Kp * 16;
    const float* const MH = MS + 2 * Kp * 16;
    for (int t = 0; t < T; ++t) {
        const float* x = X + (t & 1) * Kp * 16;
        f32x4* const xnext = reinterpret_cast<f32x4*>(X + ((t + 1) & 1) * Kp * 16);
        float* const rec = BACKWARD ? a.tape1 + ((size_t)tile * T + t) * rec_floats : nullptr;
        const f32x4* const nsrc = t + 1 < T ? xsrc(t + 1) : nullptr;
        f32x4 pf[kTsPrefetch];
#pragma unroll
        for (int q = 0; q < kTsPrefetch; ++q) {
            const int e = tid + q * nt;
            pf[q] = (nsrc && e < xq) ? nsrc[e] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // ---- phase 1: z, r ----------------------------------------------------------------------------------------------
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ua = 16 * tau + j;
            const bool aok = ua < H;
            const int uc = aok ? ua : H - 1;
            f32x4 az, ar;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) { az[reg] = bz[jj][reg]; ar[reg] = br[jj][reg]; }
            const float* wp = W + uc;
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
            const float* up = U + uc;
            for (int k16 = 0; k16 < Hp; k16 += 16)
#pragma unroll
            for (int k0 = k16; k0 < k16 + 16; k0 += 4) {
                const int k = k0 + gq;
                const bool ok = aok && k < H;
                const int kc = k < H ? k : H - 1;
                const float wz = up[kc * H3], wr = up[kc * H3 + H];
                const float hb = HT[k * 16 + j];
                az = mfma(ok ? wz : 0.0f, hb, az);
                ar = mfma(ok ? wr : 0.0f, hb, ar);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                const float z = hard_sigmoid(az[reg]), r = hard_sigmoid(ar[reg]);
                const float hp = hown[jj][reg], rh = r * hp;
                zown[jj][reg] = z;
                RHT[idx] = rh;
                if (BACKWARD) { rec[idx] = hp; rec[oRH + idx] = rh; rec[oZ + idx] = z; rec[oR + idx] = r; }
            }
        }
        if (nsrc) {
#pragma unroll
            for (int q = 0; q < kTsPrefetch; ++q) {
                const int e = tid + q * nt;
                if (e < xq) xnext[e] = pf[q];
            }
            for (int e = tid + kTsPrefetch * nt; e < xq; e += nt) xnext[e] = nsrc[e];      // a narrow layer 1 under a wide layer 0
        }
        __syncthreads();
        // ---- phase 2: candidate, state update -------------------------------------------------------------------------------
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ua = 16 * tau + j;
            const bool aok = ua < H;
            const int uc = aok ? ua : H - 1;
            f32x4 ac;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) ac[reg] = bh[jj][reg];
            const float* wp = W + 2 * H + uc;
            for (int k16 = 0; k16 < Kp; k16 += 16)
#pragma unroll
            for (int k0 = k16; k0 < k16 + 16; k0 += 4) {
                const int k = k0 + gq;
                const int kc = k < K ? k : K - 1;
                const float wh = wp[kc * H3];
                ac = mfma(aok && k < K ? wh : 0.0f, x[k * 16 + j] * MH[k * 16 + j], ac);
            }
            const float* up = U + 2 * H + uc;
            for (int k16 = 0; k16 < Hp; k16 += 16)
#pragma unroll
            for (int k0 = k16; k0 < k16 + 16; k0 += 4) {
                const int k = k0 + gq;
                const int kc = k < H ? k : H - 1;
                const float wh = up[kc * H3];
                ac = mfma(aok && k < H ? wh : 0.0f, RHT[k * 16 + j], ac);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                const float hn = gru_blend(zown[jj][reg], hown[jj][reg], ac[reg]);
                hown[jj][reg] = hn;
                HT[idx] = hn;
                if (BACKWARD) rec[oC + idx] = ac[reg];
            }
        }
        __syncthreads();
    }

    // ---- head and loss, as tw_forward: SC = [wave][16] logit parts | ds[16] | la[16] | lb[16] -------------------------------
    float part = 0.0f;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int u = 16 * (wave + jj * nw) + 4 * gq + reg;
            part = __builtin_fmaf(hown[jj][reg], u < H ? WD[u] : 0.0f, part);
        }
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    if (gq == 0) SC[wave * 16 + j] = part;
    __syncthreads();
    float* const SD = SC + kTwMaxWaves * 16;
    if (tid < 16) {
        const int smp = first + tid;
        const bool valid = smp < a.n;
        float logit = WD[H];
        for (int w = 0; w < nw; ++w) logit += SC[w * 16 + tid];
        const float p = 1.0f / (1.0f + expf(-logit));
        const float eps = 1e-7f;
        float y = 0.0f;
        if (valid && a.targets) y = a.targets[a.indices ? (size_t)a.indices[smp] : (size_t)smp];
        const float q = (1.0f - p) + eps, pe = p + eps;
        const float dp = (a.beta * (1.0f - y) / q - (1.0f - a.beta) * y / pe) * a.inv_n;
        SD[tid] = valid ? dp * p * (1.0f - p) : 0.0f;
        SD[16 + tid] = valid ? -(1.0f - y) * logf(q) : 0.0f;
        SD[32 + tid] = valid ? -y * logf(pe) : 0.0f;
        if (valid && a.probs) a.probs[smp] = p;
    }
    __syncthreads();
    float* const pt = a.partial + (size_t)tile * (H + 3);
    if (tid == 0) {
        float la = 0.0f, lb = 0.0f;
        for (int s2 = 0; s2 < 16; ++s2) { la += SD[16 + s2]; lb += SD[32 + s2]; }
        pt[H + 1] = la;
        pt[H + 2] = lb;
    }
    if (!BACKWARD) return;
    for (int u = tid; u <= H; u += nt) {
        float sum = 0.0f;
        for (int s2 = 0; s2 < 16; ++s2) sum += (u < H ? HT[u * 16 + s2] : 1.0f) * SD[s2];
        pt[u] = sum;
    }
    float* const fin = a.fin + (size_t)tile * Hp * 16;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int tau = wave + jj * nw;
        if (tau >= NT) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int u = 16 * tau + 4 * gq + reg;
            fin[u * 16 + j] = SD[j] * (u < H ? WD[u] : 0.0f);
        }
    }
}

// UT0 [3][H1p][H1p], UT1 [3][H2p][H2p] as tw_pack, W1T[g][u][k] = kernel_1[k][g H2 + u] [3][H2p][H1p]: one thread per element
__device__ inline void ts_pack(const TrainStackedArgs& a) {
    const int F = a.F, H1 = a.H1, H1p = a.H1p, H2 = a.H2, H2p = a.H2p;
    const int n0 = 3 * H1p * H1p, n1 = 3 * H2p * H2p, n2 = 3 * H2p * H1p;
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    const float* const U0 = a.theta + F * 3 * H1;
    const float* const W1 = a.theta + train_n_gru(F, H1);
    const float* const U1 = W1 + H1 * 3 * H2;
    if (e < n0) {
        const int g = e / (H1p * H1p), u = (e / H1p) % H1p, k = e % H1p;
        a.ut0[e] = (u < H1 && k < H1) ? U0[k * 3 * H1 + g * H1 + u] : 0.0f;
        return;
    }
    e -= n0;
    if (e < n1) {
        const int g = e / (H2p * H2p), u = (e / H2p) % H2p, k = e % H2p;
        a.ut1[e] = (u < H2 && k < H2) ? U1[k * 3 * H2 + g * H2 + u] : 0.0f;
        return;
    }
    e -= n1;
    if (e < n2) {
        const int g = e / (H2p * H1p), u = (e / H1p) % H2p, k = e % H1p;
        a.w1t[e] = (u < H2 && k < H1) ? W1[k * 3 * H2 + g * H2 + u] : 0.0f;
    }
}

// ---- the backward chain of one layer: tw_backward, with dx_t going out (layer 1) or coming in (layer 0) ------------------------
__host__ __device__ inline int ts_backward1_lds_floats(int H1p, int H2p) { return 3 * H2p * 16 + 3 * H1p * 16; }

template <int LAYER>
__device__ inline void ts_backward(const TrainStackedArgs& a, float* DZ, float* DR, float* DH, float* MS) {
#pragma clang fp contract(off)
    const int T = a.T, Hp = LAYER ? a.H2p : a.H1p, NT = Hp / 16, Kp = a.H1p;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
    const int gq = lane >> 4, j = lane & 15;
    const int tile = blockIdx.x;
    const size_t rec_floats = LAYER ? tw_record(0, Hp) : tw_record(a.F, Hp);
    float* const tape = LAYER ? a.tape1 : a.tape0;
    const float* const ut = LAYER ? a.ut1 : a.ut0;
    const int oZ = 2 * Hp * 16, oR = 3 * Hp * 16, oC = 4 * Hp * 16;
    const float* const UTz = ut;
    const float* const UTr = ut + (size_t)Hp * Hp;
    const float* const UTh = ut + (size_t)2 * Hp * Hp;
    const float* const dxt = a.dx + (size_t)tile * T * Kp * 16;          // dx of this tile: [T][Kp][16]

    if (LAYER) {
        const float* m = a.mtape + (size_t)tile * 3 * Kp * 16;
        for (int i = tid; i < 3 * Kp * 16; i += nt) MS[i] = m[i];
    }
    float delta[2][4], hp[2][4], z[2][4], r[2][4], dn0[2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int tau = wave + jj * nw;
            const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
            const float* const start = LAYER ? a.fin + (size_t)tile * Hp * 16 : dxt + (size_t)(T - 1) * Kp * 16;
            delta[jj][reg] = tau < NT ? start[idx] : 0.0f;
            hp[jj][reg] = z[jj][reg] = r[jj][reg] = dn0[jj][reg] = 0.0f;
        }
    if (LAYER) __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        float* const rec = tape + ((size_t)tile * T + t) * rec_floats;
        float dxin[2][4];                                   // layer 0: dx_(t-1), fetched early
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int tau = wave + jj * nw;
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                dxin[jj][reg] = (!LAYER && t > 0 && tau < NT) ? dxt[(size_t)(t - 1) * Kp * 16 + idx] : 0.0f;
            }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                const float h0 = rec[idx], zz = rec[oZ + idx], rr = rec[oR + idx], c = rec[oC + idx];
                const float d = delta[jj][reg];
                const float dz = d * (h0 - c);
                const float dh = d * (1.0f - zz);
                const float dzv = (zz > 0.0f && zz < 1.0f) ? 0.2f * dz : 0.0f;
                hp[jj][reg] = h0; z[jj][reg] = zz; r[jj][reg] = rr;
                DH[idx] = dh;
                DZ[idx] = dzv;
                rec[oC + idx] = dh;
                rec[oZ + idx] = dzv;
            }
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ka = 16 * tau + j;
            f32x4 g = {0.f, 0.f, 0.f, 0.f}, sz = {0.f, 0.f, 0.f, 0.f};
            for (int u16 = 0; u16 < Hp; u16 += 16)
#pragma unroll
            for (int u0 = u16; u0 < u16 + 16; u0 += 4) {
                const int u = u0 + gq;
                g = mfma(UTh[(size_t)u * Hp + ka], DH[u * 16 + j], g);
                sz = mfma(UTz[(size_t)u * Hp + ka], DZ[u * 16 + j], sz);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                const float rr = r[jj][reg];
                const float dr = g[reg] * hp[jj][reg];
                const float drv = (rr > 0.0f && rr < 1.0f) ? 0.2f * dr : 0.0f;
                DR[idx] = drv;
                rec[oR + idx] = drv;
                dn0[jj][reg] = (delta[jj][reg] * z[jj][reg] + g[reg] * rr) + sz[reg];
            }
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ka = 16 * tau + j;
            f32x4 acc;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) acc[reg] = dn0[jj][reg];
            for (int u16 = 0; u16 < Hp; u16 += 16)
#pragma unroll
            for (int u0 = u16; u0 < u16 + 16; u0 += 4) {
                const int u = u0 + gq;
                acc = mfma(UTr[(size_t)u * Hp + ka], DR[u * 16 + j], acc);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) delta[jj][reg] = LAYER ? acc[reg] : acc[reg] + dxin[jj][reg];
        }
        if (LAYER) {
            // dx_t [Kp][16]: the 16-row tiles of H1p go round the waves
            float* const out = a.dx + ((size_t)tile * T + t) * Kp * 16;
            const float* const WTz = a.w1t;
            const float* const WTr = a.w1t + (size_t)Hp * Kp;
            const float* const WTh = a.w1t + (size_t)2 * Hp * Kp;
            for (int kap = wave; kap < Kp / 16; kap += nw) {
                const int ka = 16 * kap + j;
                f32x4 xz = {0.f, 0.f, 0.f, 0.f}, xr = {0.f, 0.f, 0.f, 0.f}, xh = {0.f, 0.f, 0.f, 0.f};
                for (int u16 = 0; u16 < Hp; u16 += 16)
#pragma unroll
                for (int u0 = u16; u0 < u16 + 16; u0 += 4) {
                    const int u = u0 + gq;
                    xz = mfma(WTz[(size_t)u * Kp + ka], DZ[u * 16 + j], xz);
                    xr = mfma(WTr[(size_t)u * Kp + ka], DR[u * 16 + j], xr);
                    xh = mfma(WTh[(size_t)u * Kp + ka], DH[u * 16 + j], xh);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int idx = (16 * kap + 4 * gq + reg) * 16 + j;
                    out[idx] = (MS[idx] * xz[reg] + MS[Kp * 16 + idx] * xr[reg]) + MS[2 * Kp * 16 + idx] * xh[reg];
                }
            }
        }
        __syncthreads();
    }
}

// ---- layer 1's weight gradients: tw_gemm with the input rows taken from layer 0's records under the tile's mask -------------
__device__ inline void ts_gemm1(const TrainStackedArgs& a) {
#pragma clang fp contract(off)
    const int T = a.T, K = a.H1, Kp = a.H1p, H = a.H2, Hp = a.H2p, NT = Hp / 16, R = K + H + 1;
    const int RB = ((R + 15) / 16 + 1) / 2, CB = (NT + 3) / 4, per_gate = RB * CB;
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= 3 * per_gate) return;
    const int g = b / per_gate, rb = (b % per_gate) / CB, cb = b % CB;
    const int gq = lane >> 4, i = lane & 15;
    const long long records = (long long)a.n_tiles * T;
    const int S = tw_chunks(records), chunk = blockIdx.y;
    const long long c0 = chunk * records / S, c1 = (chunk + 1) * records / S;
    const size_t rec_floats = tw_record(0, Hp), rec0 = tw_record(a.F, Kp);
    const int oRH = Hp * 16;
    const int oD = (g == 0 ? 2 : g == 1 ? 3 : 4) * Hp * 16;

    int aofs[2], akind[2];                                 // kind 0: a zero row, 1: from layer 1's record, 2: ones, 3: h1_t m
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int rho = (rb * 2 + rt) * 16 + i;
        aofs[rt] = 0;
        akind[rt] = 0;
        if (rho < K) { akind[rt] = 3; aofs[rt] = rho * 16 + 4 * gq; }
        else if (rho < K + H) { akind[rt] = 1; aofs[rt] = (g == 2 ? oRH : 0) + (rho - K) * 16 + 4 * gq; }
        else if (rho == K + H) akind[rt] = 2;
    }
    const int nct = NT - cb * 4 < 4 ? NT - cb * 4 : 4;
    int bofs[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bofs[ct] = oD + ((cb * 4 + (ct < nct ? ct : 0)) * 16 + i) * 16 + 4 * gq;

    f32x4 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto load = [&](long long c, f32x4 (&A)[2], f32x4 (&B)[4]) {
        const float* rec = a.tape1 + (size_t)c * rec_floats;
        const long long tile = c / T;
        const int t = (int)(c - tile * T);
        const float* xs = t + 1 < T ? a.tape0 + (size_t)(c + 1) * rec0 : a.hfin0 + (size_t)tile * Kp * 16;
        const float* ms = a.mtape + ((size_t)tile * 3 + g) * Kp * 16;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            if (akind[rt] == 3) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(xs + aofs[rt]);
                const f32x4 m = *reinterpret_cast<const f32x4*>(ms + aofs[rt]);
                A[rt] = f32x4{x[0] * m[0], x[1] * m[1], x[2] * m[2], x[3] * m[3]};
            } else if (akind[rt] == 1) {
                A[rt] = *reinterpret_cast<const f32x4*>(rec + aofs[rt]);
            } else {
                const float fill = akind[rt] == 2 ? 1.0f : 0.0f;
                A[rt] = f32x4{fill, fill, fill, fill};
            }
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) B[ct] = *reinterpret_cast<const f32x4*>(rec + bofs[ct]);
    };
    f32x4 A[2], B[4];
    if (c0 < c1) load(c0, A, B);
    for (long long c = c0; c < c1; ++c) {
        f32x4 An[2], Bn[4];
        load(c + 1 < c1 ? c + 1 : c, An, Bn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    if (ct < nct) acc[rt][ct] = mfma(A[rt][q], B[ct][q], acc[rt][ct]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) A[rt] = An[rt];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) B[ct] = Bn[ct];
    }
    float* const out = a.gpart1 + (size_t)chunk * train_n_gru(K, H);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = (rb * 2 + rt) * 16 + 4 * gq + reg, col = (cb * 4 + ct) * 16 + i;
                if (ct < nct && row < R && col < H) out[(size_t)row * 3 * H + g * H + col] = acc[rt][ct][reg];
            }
}

// the layer of the Sequential (0, 1: the GRUs, 2: Dense) that flat element e belongs to
__device__ inline int ts_layer_of(const TrainStackedArgs& a, int e) {
    const int n0 = train_n_gru(a.F, a.H1);
    return e < n0 ? 0 : e < n0 + train_n_gru(a.H1, a.H2) ? 1 : 2;
}

// One thread per parameter (backward launches), then one for the loss.
__device__ inline void ts_reduce(const TrainStackedArgs& a) {
    const int H = a.H2, n0 = train_n_gru(a.F, a.H1), n1 = train_n_gru(a.H1, a.H2), n_par = a.backward ? n0 + n1 + H + 1 : 0;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_par) {
        float sum = 0.0f;
        const int S = tw_chunks((long long)a.n_tiles * a.T);
        if (e < n0) {
            for (int c = 0; c < S; ++c) sum += a.gpart0[(size_t)c * n0 + e];
        } else if (e < n0 + n1) {
            for (int c = 0; c < S; ++c) sum += a.gpart1[(size_t)c * n1 + (e - n0)];
        } else {
            const float* p = a.partial + (e - n0 - n1);
            for (int b = 0; b < a.n_tiles; ++b) sum += p[(size_t)b * (H + 3)];
        }
        a.grads[e] = sum;
        if (a.apply && !((a.frozen_mask >> ts_layer_of(a, e)) & 1)) train_rmsprop(a.theta[e], a.accum[e], sum, a.lr, a.rho, a.eps);
    } else if (e == n_par) {
        const float* p = a.partial + H + 1;
        float la = 0.0f, lb = 0.0f;
        for (int b = 0; b < a.n_tiles; ++b) { la += p[(size_t)b * (H + 3)]; lb += p[(size_t)b * (H + 3) + 1]; }
        a.loss[0] = a.beta * (la * a.inv_n) + (1.0f - a.beta) * (lb * a.inv_n);
    }
}

__device__ inline void ts_apply(const TrainStackedArgs& a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ts_n_params(a.F, a.H1, a.H2)) return;
    if (!((a.frozen_mask >> ts_layer_of(a, e)) & 1)) train_rmsprop(a.theta[e], a.accum[e], a.grads[e], a.lr, a.rho, a.eps);
}

#endif  // __HIPCC__

}  // namespace pe
