// Training of ONE GRU layer of 33..256 units on the f32 matrix cores.  The arithmetic contract is that of
// gru_train_device.h: forward with per-gate input dropout, weighted_log_loss, the same backward formulas and
// tie rule, float32 with float32 accumulation.  What changes is where the sums run: every per-step product is a chain of
// v_mfma_f32_16x16x4_f32 over a tile of 16 samples, with the problem transposed as in gru_wide_device.h
//     gates^T [units x 16 samples] = W^T [units x K] . operands^T [K x 16 samples]
// so weights are the A operand (streamed from L2 every timestep: the recurrent kernel is 786 KB at 256 units) and the
// per-sample operands the B operand, kept in LDS as [k][16 samples]: lane (g, j) of a wave reads k-slot g of sample j, 64
// consecutive floats per MFMA.
//
// A step of one network is five launches:
//   tw_forward   one workgroup per tile, one wave per 16-unit output tile (at most 8 waves, two tiles each).  Phase 1: z and
//                r of the wave's units, r h_(t-1) to LDS; barrier; phase 2: candidate and state update; barrier.  The tape
//                record of (tile, t) goes to HBM as [h_(t-1) | r h_(t-1) | z | r | c][unit][16 samples] | x m [3][F][16].
//                Ends with the head, the loss sums, the dense gradients of the tile and delta_T = dL/dh_T.
//   tw_pack      UT[gate][u][k] = U[k][gate H + u], zero padded to the tile: the A operands of the three . U^T products
//   tw_backward  the chain t = T-1 .. 0 per tile: the pre-activation gradients D_z, D_r, D_h overwrite z, r, c of the record
//                (the lane that read a value is the one that overwrites it), g = D_h U_h^T, delta' = delta z + g r + D_z U_z^T
//                + D_r U_r^T, three barriers per step
//   tw_gemm      dTheta = L^T D over the n T contraction, as MFMAs straight from the records: a record's 16 samples are the
//                four k-steps of four MFMAs, one 16-byte load per lane and operand.  The contraction is cut into
//                tw_chunks(records) chunks of whole records, chunk c = records [c K / S, (c + 1) K / S): boundaries and the order
//                inside a chunk depend on (n, T) alone.  One wave owns a 2 x 4 block of output tiles of one gate and one chunk.
//   tw_reduce    adds the chunk partials in chunk order and the per-tile dense / loss partials in tile order (no floating-point
//                atomic anywhere), writes the gradient and may apply RMSprop (train_rmsprop, shared with the narrow path)
//
// Padding: units H..Hp-1 have zero weights, zero bias and zero dense weight, so their state, their delta and their D are exact
// zeros; samples past n read zero inputs and get ds = 0, so their D are exact zeros.  Every record of a launch is written in
// full by tw_forward before anything reads it, so what an earlier, larger call left in the scratch is never read.
#pragma once
#include "gru_device.h"
#include "gru_train_device.h"

namespace pe {

constexpr int kTwMaxUnits = 256, kTwMaxWaves = 8, kTwMaxChunks = 64;

inline int tw_pad(int H) { return (H + 15) / 16 * 16; }
inline int tw_waves(int H) { const int nt = tw_pad(H) / 16; return nt < kTwMaxWaves ? nt : kTwMaxWaves; }
__host__ __device__ inline size_t tw_record(int F, int Hp) { return (size_t)(5 * Hp + 3 * F) * 16; }      // floats
__host__ __device__ inline int tw_chunks(long long records) { return records < kTwMaxChunks ? (int)records : kTwMaxChunks; }

// One network of a wide trainer over one batch.
struct TrainWideArgs {
    int n, T, F, H, Hp, n_tiles;
    int backward, apply, frozen_mask, mask_mode;
    float rate, keep_scale, beta, inv_n;
    float lr, rho, eps;
    uint64_t mask_key;
    float* theta;               // flat parameters of THIS network (and accum, grads)
    float* accum;
    float* grads;
    float* loss;                // [1]
    const float* feats;
    const float* targets;
    const int32_t* indices;
    const float* masks;
    float* tape;                // [n_tiles T] records of tw_record(F, Hp) floats
    float* fin;                 // [n_tiles][Hp][16]: dL/dh_T
    float* ut;                  // [3][Hp][Hp]
    float* partial;             // [n_tiles][H + 3]: dense kernel, dense bias, the two loss sums
    float* gpart;               // [chunks][train_n_gru]
    float* probs;               // [n]
};

hipError_t launch_train_wide(const TrainWideArgs& a, hipStream_t s);

#if defined(__HIPCC__)

constexpr int kTwLdsState = kTwMaxUnits * 16, kTwLdsX = 3 * kTrainMaxFeat * 16;

template <bool BACKWARD>
__device__ inline void tw_forward(const TrainWideArgs& a, float* HT, float* RHT, float* XM, float* MS, float* SC) {
#pragma clang fp contract(off)
    const int T = a.T, F = a.F, H = a.H, Hp = a.Hp, H3 = 3 * H, NT = Hp / 16;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
    const int gq = lane >> 4, j = lane & 15;
    const int tile = blockIdx.x, first = tile * 16;
    const float* const W = a.theta;
    const float* const U = W + F * H3;
    const float* const Bv = U + H * H3;
    const float* const WD = Bv + H3;
    const size_t rec_floats = tw_record(F, Hp);
    const int oRH = Hp * 16, oZ = 2 * Hp * 16, oR = 3 * Hp * 16, oC = 4 * Hp * 16, oX = 5 * Hp * 16;

    // ---- masks [gate][f][s], h_0 = 0 ---------------------------------------------------------------------------------------
    for (int i = tid; i < 3 * F * 16; i += nt) {
        const int g = i / (F * 16), f = (i / 16) % F, s2 = i % 16;
        const int smp = first + s2;
        float m = 1.0f;
        if (smp < a.n) {
            if (a.mask_mode == 1) m = a.masks[((size_t)g * a.n + smp) * F + f];
            else if (a.mask_mode == 2) m = train_mask_keep(a.mask_key, g, smp, f, a.rate) ? a.keep_scale : 0.0f;
        }
        MS[i] = m;
    }
    for (int i = tid; i < Hp * 16; i += nt) HT[i] = 0.0f;
    // the input elements this thread stages every step: element e = tid + q nt of [16 samples][F]
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
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (xdst[q] >= 0) {
            const float x = xrow[q] ? xrow[q][0] : 0.0f;
            for (int g = 0; g < 3; ++g) XM[g * F * 16 + xdst[q]] = x * MS[g * F * 16 + xdst[q]];
        }

    // ---- this wave's output tiles: tau = wave + jj nw; lane (gq, j) owns units 16 tau + 4 gq + reg of sample j ---------------
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
        float* const rec = BACKWARD ? a.tape + ((size_t)tile * T + t) * rec_floats : nullptr;
        float xn[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) xn[q] = (t + 1 < T && xrow[q]) ? xrow[q][(size_t)(t + 1) * F] : 0.0f;
        // ---- phase 1: z, r ----------------------------------------------------------------------------------------------
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ua = 16 * tau + j;                      // the unit whose weights this lane feeds as A rows
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
            for (int k0 = k16; k0 < k16 + 16; k0 += 4) {         // Hp is a multiple of 16
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
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (xdst[q] >= 0)
                for (int g = 0; g < 3; ++g) xmn[g * F * 16 + xdst[q]] = xn[q] * MS[g * F * 16 + xdst[q]];
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
            for (int k0 = k16; k0 < k16 + 16; k0 += 4) {         // Hp is a multiple of 16
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

    // ---- head and loss: SC = [wave][16] logit parts | ds[16] | la[16] | lb[16] ---------------------------------------------
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
    for (int u = tid; u <= H; u += nt) {                   // dense kernel (u < H) and dense bias (u == H)
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

// UT[g][u][k] = U[k][g H + u] for u, k < H, zero elsewhere: one thread per element of [3][Hp][Hp]
__device__ inline void tw_pack(const TrainWideArgs& a) {
    const int Hp = a.Hp, H = a.H;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * Hp * Hp) return;
    const int g = e / (Hp * Hp), u = (e / Hp) % Hp, k = e % Hp;
    const float* const U = a.theta + a.F * 3 * H;
    a.ut[e] = (u < H && k < H) ? U[k * 3 * H + g * H + u] : 0.0f;
}

__device__ inline void tw_backward(const TrainWideArgs& a, float* DZ, float* DR, float* DH) {
#pragma clang fp contract(off)
    const int T = a.T, F = a.F, Hp = a.Hp, NT = Hp / 16;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
    const int gq = lane >> 4, j = lane & 15;
    const int tile = blockIdx.x;
    const size_t rec_floats = tw_record(F, Hp);
    const int oZ = 2 * Hp * 16, oR = 3 * Hp * 16, oC = 4 * Hp * 16;
    const float* const UTz = a.ut;
    const float* const UTr = a.ut + (size_t)Hp * Hp;
    const float* const UTh = a.ut + (size_t)2 * Hp * Hp;

    float delta[2][4], hp[2][4], z[2][4], r[2][4], dn0[2][4];
    const float* const fin = a.fin + (size_t)tile * Hp * 16;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int tau = wave + jj * nw;
            delta[jj][reg] = tau < NT ? fin[(16 * tau + 4 * gq + reg) * 16 + j] : 0.0f;
            hp[jj][reg] = z[jj][reg] = r[jj][reg] = dn0[jj][reg] = 0.0f;
        }

    for (int t = T - 1; t >= 0; --t) {
        float* const rec = a.tape + ((size_t)tile * T + t) * rec_floats;
        // ---- D_h, D_z of the own units --------------------------------------------------------------------------------------
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
        // ---- g = D_h U_h^T (and D_z U_z^T next to it), D_r -------------------------------------------------------------------
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
            const int ka = 16 * tau + j;                      // the unit (row of U) this lane feeds as A rows
            f32x4 g = {0.f, 0.f, 0.f, 0.f}, sz = {0.f, 0.f, 0.f, 0.f};
            for (int u16 = 0; u16 < Hp; u16 += 16)
#pragma unroll
            for (int u0 = u16; u0 < u16 + 16; u0 += 4) {         // Hp is a multiple of 16
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
        // ---- delta of the step before -----------------------------------------------------------------------------------------
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
            for (int u0 = u16; u0 < u16 + 16; u0 += 4) {         // Hp is a multiple of 16
                const int u = u0 + gq;
                acc = mfma(UTr[(size_t)u * Hp + ka], DR[u * 16 + j], acc);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) delta[jj][reg] = acc[reg];
        }
        __syncthreads();
    }
}

// One wave: rows [32 rb, 32 rb + 32) x columns [64 cb, 64 cb + 64) of gate g's [F + H + 1][H] block, one chunk of records.
__device__ inline void tw_gemm(const TrainWideArgs& a) {
    const int T = a.T, F = a.F, H = a.H, Hp = a.Hp, NT = Hp / 16, R = F + H + 1;
    const int RB = ((R + 15) / 16 + 1) / 2, CB = (NT + 3) / 4, per_gate = RB * CB;
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= 3 * per_gate) return;
    const int g = b / per_gate, rb = (b % per_gate) / CB, cb = b % CB;
    const int gq = lane >> 4, i = lane & 15;
    const long long records = (long long)a.n_tiles * T;
    const int S = tw_chunks(records), chunk = blockIdx.y;
    const long long c0 = chunk * records / S, c1 = (chunk + 1) * records / S;
    const size_t rec_floats = tw_record(F, Hp);
    const int oRH = Hp * 16, oX = 5 * Hp * 16;
    const int oD = (g == 0 ? 2 : g == 1 ? 3 : 4) * Hp * 16;

    int aofs[2], akind[2];                                 // kind 0: a zero row, 1: loaded, 2: the bias row of ones
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int rho = (rb * 2 + rt) * 16 + i;
        aofs[rt] = 0;
        akind[rt] = 0;
        if (rho < F) { akind[rt] = 1; aofs[rt] = oX + (g * F + rho) * 16 + 4 * gq; }
        else if (rho < F + H) { akind[rt] = 1; aofs[rt] = (g == 2 ? oRH : 0) + (rho - F) * 16 + 4 * gq; }
        else if (rho == F + H) akind[rt] = 2;
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
        const float* rec = a.tape + (size_t)c * rec_floats;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(rec + aofs[rt]);
            const float fill = akind[rt] == 2 ? 1.0f : 0.0f;
            A[rt] = akind[rt] == 1 ? v : f32x4{fill, fill, fill, fill};
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
    float* const out = a.gpart + (size_t)chunk * train_n_gru(F, H);
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

// One thread per parameter (backward launches), then one for the loss.
__device__ inline void tw_reduce(const TrainWideArgs& a) {
    const int F = a.F, H = a.H, n_gru = train_n_gru(F, H), n_par = a.backward ? n_gru + H + 1 : 0;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_par) {
        float sum = 0.0f;
        if (e < n_gru) {
            const int S = tw_chunks((long long)a.n_tiles * a.T);
            for (int c = 0; c < S; ++c) sum += a.gpart[(size_t)c * n_gru + e];
        } else {
            const float* p = a.partial + (e - n_gru);
            for (int b = 0; b < a.n_tiles; ++b) sum += p[(size_t)b * (H + 3)];
        }
        a.grads[e] = sum;
        if (a.apply && !((a.frozen_mask >> (e < n_gru ? 0 : 1)) & 1)) train_rmsprop(a.theta[e], a.accum[e], sum, a.lr, a.rho, a.eps);
    } else if (e == n_par) {
        const float* p = a.partial + H + 1;
        float la = 0.0f, lb = 0.0f;
        for (int b = 0; b < a.n_tiles; ++b) { la += p[(size_t)b * (H + 3)]; lb += p[(size_t)b * (H + 3) + 1]; }
        a.loss[0] = a.beta * (la * a.inv_n) + (1.0f - a.beta) * (lb * a.inv_n);
    }
}

#endif  // __HIPCC__

}  // namespace pe
