// Training of GRU layers of up to 256 units on the f32 matrix cores: every piece of a layer's step, written
// once, for the one-layer trainer of 33..256 units here and for the two-layer stack of gru_train_stacked_device.h.  The
// arithmetic contract is that of gru_train_device.h: forward with per-gate input dropout, weighted_log_loss,
// the same backward formulas and tie rule, float32 with float32 accumulation.  What changes is where the sums run: every
// per-step product is a chain of v_mfma_f32_16x16x4_f32 over a tile of 16 samples, with the problem transposed as in
// gru_wide_device.h
//     gates^T [units x 16 samples] = W^T [units x K] . operands^T [K x 16 samples]
// so weights are the A operand (streamed from L2 every timestep: the recurrent kernel is 786 KB at 256 units) and the
// per-sample operands the B operand, kept in LDS as [k][16 samples]: lane (g, j) of a wave reads k-slot g of sample j, 64
// consecutive floats per MFMA.
//
// The pieces, each over one TwLayer:
//   tw_steps     the time loop of a forward: one workgroup per tile, one wave per 16-unit output tile (at most 8 waves, two
//                tiles each).  Phase 1: z and r of the wave's units, r h_(t-1) to LDS; barrier; phase 2: candidate and state
//                update; barrier.  The tape record of (tile, t) goes to HBM as [h_(t-1) | r h_(t-1) | z | r | c][unit][16
//                samples], then whatever the input policy adds.  Where the layer's input comes from is the policy's business
//                (TwInputX: x m staged in LDS, also the record's x m [3][F][16] block), fixed at compile time.
//   tw_head      the head, the loss sums, the dense gradients of the tile and delta_T = dL/dh_T of the last layer
//   tw_pack      dst[gate][u][k] = src[k][gate H + u], zero padded to the tile: the A operands of the . U^T (and . W^T) products
//   tw_backward  the chain t = T-1 .. 0 per tile: the pre-activation gradients D_z, D_r, D_h overwrite z, r, c of the record
//                (the lane that read a value is the one that overwrites it), g = D_h U_h^T, delta' = delta z + g r + D_z U_z^T
//                + D_r U_r^T, three barriers per step.  What becomes of dx_t is a compile-time choice (TwDx).
//   tw_gemm      dTheta = L^T D over the n T contraction, as MFMAs straight from the records: a record's 16 samples are the
//                four k-steps of four MFMAs, one 16-byte load per lane and operand.  The contraction is cut into
//                tw_chunks(records) chunks of whole records, chunk c = records [c K / S, (c + 1) K / S): boundaries and the order
//                inside a chunk depend on (n, T) alone.  One wave owns a 2 x 4 block of output tiles of one gate and one chunk.
//   tw_reduce    adds the chunk partials in chunk order and the per-tile dense / loss partials in tile order (no floating-point
//                atomic anywhere), writes the gradient and may apply RMSprop (train_rmsprop, shared with the narrow path)
// A step of the one-layer trainer is five launches: tw_forward (tw_steps and tw_head), tw_pack, tw_backward, tw_gemm, tw_reduce.
//
// A kernel forms its TwLayer from its arguments with the pointer arithmetic written here once (tw_layer); the argument structs
// keep their field order.  Against the written-out twins these pieces replaced (profiles/train_layers/isa_compare.txt):
// tw_backward_kernel, tw_gemm_kernel, tw_reduce_kernel, ts_gemm0_kernel and ts_apply_kernel are identical or same-shape; the
// forward kernels (tw_forward_kernel, ts_forward0_kernel, ts_forward1_kernel, <true> and <false>) differ by -14 .. +8 of
// 1769 .. 2483 instructions, scalar compares and branches around the null tests of the staged rows, within -4 .. +8 VGPRs;
// ts_gemm1_kernel +8 of 1782 (scalar loads and waits), ts_reduce_kernel +1, tw_pack_kernel +1 and ts_pack_kernel +3 (s_load
// widths), ts_backward0_kernel +1 and ts_backward1_kernel -1 (one scalar shift).  No kernel has scratch.  tw_steps keeps the
// wave's own state in a local array and hands it out at the end: as a reference parameter it is memory to the passes that run
// before inlining, and the bias preload then compiles to three guarded loads instead of one guarded block.
//
// Padding: units H..Hp-1 have zero weights, zero bias and zero dense weight, so their state, their delta and their D are exact
// zeros; samples past n read zero inputs and get ds = 0, so their D are exact zeros.  Every record of a launch is written in
// full by the forward before anything reads it, so what an earlier, larger call left in the scratch is never read.
#pragma once
#include "gru_device.h"
#include "gru_train_device.h"

namespace pe {

constexpr int kTwMaxUnits = 256, kTwMaxWaves = 8, kTwMaxChunks = 64;

inline int tw_pad(int H) { return (H + 15) / 16 * 16; }
inline int tw_waves(int H) { const int nt = tw_pad(H) / 16; return nt < kTwMaxWaves ? nt : kTwMaxWaves; }
__host__ __device__ inline size_t tw_record(int F, int Hp) { return (size_t)(5 * Hp + 3 * F) * 16; }      // floats
__host__ __device__ inline int tw_chunks(long long records) { return records < kTwMaxChunks ? (int)records : kTwMaxChunks; }

// One GRU layer as the device functions see it: a view that a kernel forms from its arguments (tw_layer).
struct TwLayer {
    int K, H, Hp;               // input width (F, or the units of the layer below), units, units padded to the tile
    const float* W;             // kernel [K][3 H], in theta
    const float* U;             // recurrent kernel [H][3 H]
    const float* B;             // bias [3 H]; what follows it in theta is the next layer, or the dense head
    size_t rec;                 // floats of one tape record
    float* tape;                // [n_tiles T] records
    float* ut;                  // [3][Hp][Hp]
    float* gpart;               // [chunks][train_n_gru(K, H)]
};

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

__device__ inline TwLayer tw_layer(float* theta, int K, int H, int Hp, size_t rec, float* tape, float* ut, float* gpart) {
    const int H3 = 3 * H;
    const float* const W = theta;
    const float* const U = W + K * H3;
    return TwLayer{K, H, Hp, W, U, U + H * H3, rec, tape, ut, gpart};
}
__device__ inline TwLayer tw_layer(const TrainWideArgs& a) {
    return tw_layer(a.theta, a.F, a.H, a.Hp, tw_record(a.F, a.Hp), a.tape, a.ut, a.gpart);
}

// where a thread stands: lane (gq, j) of wave `wave` of the workgroup of tile `tile`
struct TwThread {
    int tid, nt, wave, lane, nw, gq, j, tile, first;
    __device__ TwThread()
        : tid(threadIdx.x), nt(blockDim.x), wave(tid >> 6), lane(tid & 63), nw(nt >> 6), gq(lane >> 4), j(lane & 15),
          tile(blockIdx.x), first(tile * 16) {}
};

// The input policy of layer 0: the features x_t of the tile, x m staged in LDS one step ahead as XM[2][gate][F][16], and
// written to the record's x m block.  FEW: the workgroup may be one wave (a stacked network's layer 0 of at most 16 units),
// which stages 16 F <= 512 elements with 64 threads, more than three per thread.  HFIN: h_t also goes to `hfin`, as the
// final state [tile][Hp][16] (backward) or the sequence [tile][T][Hp][16] (forward only).
template <class Args, bool BACKWARD, bool FEW, bool HFIN>
struct TwInputX {
    const Args& a;
    const TwLayer& l;
    const TwThread& th;
    const float* masks;         // mask_mode 1: [3][n][F]
    uint64_t mask_key;
    float* hfin;
    float* XM;
    float* MS;
    const float* xrow[3];
    int xdst[3];
    float xn[3];
    bool few;
    const float* xm;
    float* xmn;

    __device__ void stage_all(int t, float* dst) const {  // the slow form: every element through a loop
#pragma clang fp contract(off)
        const int F = l.K, tid = th.tid, nt = th.nt, first = th.first, T = a.T;
        for (int e = tid; e < 16 * F; e += nt) {
            const int s2 = e / F, f = e % F, smp = first + s2;
            float x = 0.0f;
            if (smp < a.n) {
                const size_t r = a.indices ? (size_t)a.indices[smp] : (size_t)smp;
                x = a.feats[r * (size_t)T * F + (size_t)t * F + f];
            }
            for (int g = 0; g < 3; ++g) dst[g * F * 16 + f * 16 + s2] = x * MS[g * F * 16 + f * 16 + s2];
        }
    }
    // masks [gate][f][s]
    __device__ void masks_init() {
        const int F = l.K, tid = th.tid, nt = th.nt, first = th.first;
        for (int i = tid; i < 3 * F * 16; i += nt) {
            const int g = i / (F * 16), f = (i / 16) % F, s2 = i % 16;
            const int smp = first + s2;
            float m = 1.0f;
            if (smp < a.n) {
                if (a.mask_mode == 1) m = masks[((size_t)g * a.n + smp) * F + f];
                else if (a.mask_mode == 2) m = train_mask_keep(mask_key, g, smp, f, a.rate) ? a.keep_scale : 0.0f;
            }
            MS[i] = m;
        }
    }
    // the input elements this thread stages every step: element e = tid + q nt of [16 samples][F]; then x_0 m
    __device__ void stage_first() {
#pragma clang fp contract(off)
        const int F = l.K, tid = th.tid, nt = th.nt, first = th.first, T = a.T;
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
        few = FEW && 3 * nt < 16 * F;
        if (FEW && few) stage_all(0, XM);
        else {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (xdst[q] >= 0) {
                    const float x = xrow[q] ? xrow[q][0] : 0.0f;
                    for (int g = 0; g < 3; ++g) XM[g * F * 16 + xdst[q]] = x * MS[g * F * 16 + xdst[q]];
                }
        }
    }
    __device__ void fetch(int t) {
        const int F = l.K, T = a.T;
        xm = XM + (t & 1) * kTwLdsX;
        xmn = XM + ((t + 1) & 1) * kTwLdsX;
#pragma unroll
        for (int q = 0; q < 3; ++q) xn[q] = (!(FEW && few) && t + 1 < T && xrow[q]) ? xrow[q][(size_t)(t + 1) * F] : 0.0f;
    }
    __device__ void add_zr(f32x4& az, f32x4& ar, bool aok, int uc) const {
        const int F = l.K, H = l.H, H3 = 3 * H, gq = th.gq, j = th.j;
        const float* const W = l.W;
        for (int k0 = 0; k0 < F; k0 += 4) {
            const int k = k0 + gq;
            const bool ok = aok && k < F;
            const int kc = k < F ? k : F - 1;
            const float wz = W[kc * H3 + uc], wr = W[kc * H3 + H + uc];
            const float xz = xm[kc * 16 + j], xr = xm[(F + kc) * 16 + j];
            az = mfma(ok ? wz : 0.0f, k < F ? xz : 0.0f, az);
            ar = mfma(ok ? wr : 0.0f, k < F ? xr : 0.0f, ar);
        }
    }
    __device__ void add_c(f32x4& ac, bool aok, int uc) const {
        const int F = l.K, H = l.H, H3 = 3 * H, gq = th.gq, j = th.j;
        const float* const W = l.W;
        for (int k0 = 0; k0 < F; k0 += 4) {
            const int k = k0 + gq;
            const int kc = k < F ? k : F - 1;
            const float wh = W[kc * H3 + 2 * H + uc];
            const float xh = xm[(2 * F + kc) * 16 + j];
            ac = mfma(aok && k < F ? wh : 0.0f, k < F ? xh : 0.0f, ac);
        }
    }
    // between the phases: the record's x m block, and x_(t+1) m for the next step
    __device__ void stage_next(int t, float* rec) const {
#pragma clang fp contract(off)
        const int F = l.K, tid = th.tid, nt = th.nt, oX = 5 * l.Hp * 16;
        if (BACKWARD)
            for (int i = tid; i < 3 * F * 16; i += nt) rec[oX + i] = xm[i];
        if (FEW && few) {
            if (t + 1 < a.T) stage_all(t + 1, xmn);
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (xdst[q] >= 0)
                    for (int g = 0; g < 3; ++g) xmn[g * F * 16 + xdst[q]] = xn[q] * MS[g * F * 16 + xdst[q]];
        }
    }
    // where h_t goes besides the next record
    __device__ float* hout(int t) const {
        if (!HFIN) return nullptr;
        const int T = a.T, Hp = l.Hp, tile = th.tile;
        return BACKWARD ? (t + 1 == T ? hfin + (size_t)tile * Hp * 16 : nullptr) : hfin + ((size_t)tile * T + t) * Hp * 16;
    }
};

// The forward of one layer over the tile: h_0 = 0, then T two-phase steps.  `in` forms the input contribution; the state after
// the last step is left in HT (LDS) and in hlast (this wave's output tiles: tau = wave + jj nw; lane (gq, j) owns units
// 16 tau + 4 gq + reg of sample j).
template <bool BACKWARD, class Input>
__device__ inline void tw_steps(int T, const TwLayer& l, const TwThread& th, Input& in, float* HT, float* RHT, float (&hlast)[2][4]) {
#pragma clang fp contract(off)
    const int H = l.H, Hp = l.Hp, H3 = 3 * H, NT = Hp / 16;
    const int tid = th.tid, nt = th.nt, wave = th.wave, nw = th.nw, gq = th.gq, j = th.j, tile = th.tile;
    const float* const U = l.U;
    const float* const Bv = l.B;
    const size_t rec_floats = l.rec;
    const int oRH = Hp * 16, oZ = 2 * Hp * 16, oR = 3 * Hp * 16, oC = 4 * Hp * 16;

    in.masks_init();
    for (int i = tid; i < Hp * 16; i += nt) HT[i] = 0.0f;
    in.stage_first();

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
        float* const rec = BACKWARD ? l.tape + ((size_t)tile * T + t) * rec_floats : nullptr;
        float* const hout = in.hout(t);
        in.fetch(t);
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
            in.add_zr(az, ar, aok, uc);
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
        in.stage_next(t, rec);
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
            in.add_c(ac, aok, uc);
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
                if (hout) hout[idx] = hn;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) hlast[jj][reg] = hown[jj][reg];
}

// Head and loss of the last layer `l`, whose final state is in HT and hown: SC = [wave][16] logit parts | ds[16] | la[16] |
// lb[16].  Writes the probabilities, the tile's row of `partial` [n_tiles][H + 3] (dense kernel, dense bias, the two loss
// sums) and delta_T = dL/dh_T to `fin` [n_tiles][Hp][16].
template <bool BACKWARD, class Args>
__device__ inline void tw_head(const Args& a, const TwLayer& l, const TwThread& th, float* fin_all, float* partial,
                               const float (&hown)[2][4], const float* HT, float* SC) {
#pragma clang fp contract(off)
    const int H = l.H, Hp = l.Hp, NT = Hp / 16;
    const int tid = th.tid, nt = th.nt, wave = th.wave, nw = th.nw, gq = th.gq, j = th.j, tile = th.tile, first = th.first;
    const float* const WD = l.B + 3 * H;
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
    float* const pt = partial + (size_t)tile * (H + 3);
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
    float* const fin = fin_all + (size_t)tile * Hp * 16;
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

template <bool BACKWARD>
__device__ inline void tw_forward(const TrainWideArgs& a, float* HT, float* RHT, float* XM, float* MS, float* SC) {
    const TwThread th;
    const TwLayer l = tw_layer(a);
    TwInputX<TrainWideArgs, BACKWARD, false, false> in{a, l, th, a.masks, a.mask_key, nullptr, XM, MS};
    float hown[2][4];
    tw_steps<BACKWARD>(a.T, l, th, in, HT, RHT, hown);
    tw_head<BACKWARD>(a, l, th, a.fin, a.partial, hown, HT, SC);
}

// dst[g][u][k] = src[k][g H + u] for u < H, k < K, zero elsewhere: element e of [3][Hp][Kp]
__device__ inline void tw_pack(float* dst, const float* src, int e, int K, int Kp, int H, int Hp) {
    const int g = e / (Hp * Kp), u = (e / Kp) % Hp, k = e % Kp;
    dst[e] = (u < H && k < K) ? src[k * 3 * H + g * H + u] : 0.0f;
}

// What the backward chain of a layer does about dx, the gradient of its input: nothing (the input is the features), write
// dx_t = m_z (D_z W_z^T) + m_r (D_r W_r^T) + m_h (D_h W_h^T) for the layer below (three MFMA chains per 16-row tile of Kp,
// per (tile, t) as [Kp][16]), or be that layer below: delta starts as dx_(T-1), and dx_(t-1) is added after the recurrent
// terms of step t.
enum class TwDx { kNone, kWrite, kRead };
struct TwDxArgs {
    float* dx;                  // [n_tiles T][Kp][16]
    int Kp;                     // the padded units of the layer below (kRead: this layer's own Hp)
    const float* wt;            // kWrite: this layer's W^T [3][Hp][Kp]
    const float* mtape;         // kWrite: this layer's masks per tile [n_tiles][3][Kp][16], and MS the LDS copy of one tile's
    float* MS;
};

template <TwDx DX>
__device__ inline void tw_backward(int T, const TwLayer& l, const float* fin_all, const TwDxArgs& d, float* DZ, float* DR, float* DH) {
#pragma clang fp contract(off)
    const int Hp = l.Hp, NT = Hp / 16, Kp = d.Kp;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
    const int gq = lane >> 4, j = lane & 15;
    const int tile = blockIdx.x;
    const size_t rec_floats = l.rec;
    const int oZ = 2 * Hp * 16, oR = 3 * Hp * 16, oC = 4 * Hp * 16;
    const float* const UTz = l.ut;
    const float* const UTr = l.ut + (size_t)Hp * Hp;
    const float* const UTh = l.ut + (size_t)2 * Hp * Hp;
    const float* const dxt = DX == TwDx::kNone ? nullptr : d.dx + (size_t)tile * T * Kp * 16;      // dx of this tile: [T][Kp][16]
    float* const MS = d.MS;

    if (DX == TwDx::kWrite) {
        const float* m = d.mtape + (size_t)tile * 3 * Kp * 16;
        for (int i = tid; i < 3 * Kp * 16; i += nt) MS[i] = m[i];
    }
    float delta[2][4], hp[2][4], z[2][4], r[2][4], dn0[2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int tau = wave + jj * nw;
            const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
            const float* const start = DX == TwDx::kRead ? dxt + (size_t)(T - 1) * Kp * 16 : fin_all + (size_t)tile * Hp * 16;
            delta[jj][reg] = tau < NT ? start[idx] : 0.0f;
            hp[jj][reg] = z[jj][reg] = r[jj][reg] = dn0[jj][reg] = 0.0f;
        }
    if (DX == TwDx::kWrite) __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        float* const rec = l.tape + ((size_t)tile * T + t) * rec_floats;
        float dxin[2][4];                                   // kRead: dx_(t-1), fetched early
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int tau = wave + jj * nw;
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                dxin[jj][reg] = (DX == TwDx::kRead && t > 0 && tau < NT) ? dxt[(size_t)(t - 1) * Kp * 16 + idx] : 0.0f;
            }
        // ---- D_h, D_z of the own units --------------------------------------------------------------------------------------
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int tau = wave + jj * nw;
            if (tau >= NT) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int idx = (16 * tau + 4 * gq + reg) * 16 + j;
                const float h0 = rec[idx], zz = rec[oZ + idx], rr = rec[oR + idx], c = rec[oC + idx];
                const float dd = delta[jj][reg];
                const float dz = dd * (h0 - c);
                const float dh = dd * (1.0f - zz);
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
            for (int reg = 0; reg < 4; ++reg) delta[jj][reg] = DX == TwDx::kRead ? acc[reg] + dxin[jj][reg] : acc[reg];
        }
        if (DX == TwDx::kWrite) {
            // dx_t [Kp][16]: the 16-row tiles of Kp go round the waves
            float* const out = d.dx + ((size_t)tile * T + t) * Kp * 16;
            const float* const WTz = d.wt;
            const float* const WTr = d.wt + (size_t)Hp * Kp;
            const float* const WTh = d.wt + (size_t)2 * Hp * Kp;
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

// Where the K input rows of a layer's weight-gradient GEMM come from when they are not the record's own x m block: h_t of the
// layer below (slot 0 of its record t + 1, or its final state), multiplied by the tile's mask as it is loaded.
struct TwGemmBelow {
    const float* tape;          // the records of the layer below, `rec` floats each
    size_t rec;
    const float* hfin;          // [n_tiles][Kp][16]
    const float* mtape;         // [n_tiles][3][Kp][16]
    int Kp;
};

// One wave: rows [32 rb, 32 rb + 32) x columns [64 cb, 64 cb + 64) of gate g's [K + H + 1][H] block, one chunk of records.
template <bool BELOW>
__device__ inline void tw_gemm(int T, int n_tiles, const TwLayer& l, const TwGemmBelow& x) {
#pragma clang fp contract(off)
    const int K = l.K, H = l.H, Hp = l.Hp, NT = Hp / 16, R = K + H + 1;
    const int RB = ((R + 15) / 16 + 1) / 2, CB = (NT + 3) / 4, per_gate = RB * CB;
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= 3 * per_gate) return;
    const int g = b / per_gate, rb = (b % per_gate) / CB, cb = b % CB;
    const int gq = lane >> 4, i = lane & 15;
    const long long records = (long long)n_tiles * T;
    const int S = tw_chunks(records), chunk = blockIdx.y;
    const long long c0 = chunk * records / S, c1 = (chunk + 1) * records / S;
    const size_t rec_floats = l.rec;
    const int oRH = Hp * 16, oX = 5 * Hp * 16;
    const int oD = (g == 0 ? 2 : g == 1 ? 3 : 4) * Hp * 16;

    int aofs[2], akind[2];              // kind 0: a zero row, 1: from the record, 2: the bias row of ones, 3: h_t m of the layer below
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int rho = (rb * 2 + rt) * 16 + i;
        aofs[rt] = 0;
        akind[rt] = 0;
        if (rho < K) {
            if (BELOW) { akind[rt] = 3; aofs[rt] = rho * 16 + 4 * gq; }
            else { akind[rt] = 1; aofs[rt] = oX + (g * K + rho) * 16 + 4 * gq; }
        }
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
        const float* rec = l.tape + (size_t)c * rec_floats;
        const float* xs = nullptr;
        const float* ms = nullptr;
        if (BELOW) {
            const long long tile = c / T;
            const int t = (int)(c - tile * T);
            xs = t + 1 < T ? x.tape + (size_t)(c + 1) * x.rec : x.hfin + (size_t)tile * x.Kp * 16;
            ms = x.mtape + ((size_t)tile * 3 + g) * x.Kp * 16;
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            if (BELOW) {
                if (akind[rt] == 3) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + aofs[rt]);
                    const f32x4 m = *reinterpret_cast<const f32x4*>(ms + aofs[rt]);
                    A[rt] = f32x4{xv[0] * m[0], xv[1] * m[1], xv[2] * m[2], xv[3] * m[3]};
                } else if (akind[rt] == 1) {
                    A[rt] = *reinterpret_cast<const f32x4*>(rec + aofs[rt]);
                } else {
                    const float fill = akind[rt] == 2 ? 1.0f : 0.0f;
                    A[rt] = f32x4{fill, fill, fill, fill};
                }
            } else {                                       // no branch: a row that is not loaded reads offset 0 and drops it
                const f32x4 v = *reinterpret_cast<const f32x4*>(rec + aofs[rt]);
                const float fill = akind[rt] == 2 ? 1.0f : 0.0f;
                A[rt] = akind[rt] == 1 ? v : f32x4{fill, fill, fill, fill};
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
    float* const out = l.gpart + (size_t)chunk * train_n_gru(K, H);
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
inline dim3 tw_gemm_grid(int T, int n_tiles, int K, int H) {
    const int R = K + H + 1, RB = ((R + 15) / 16 + 1) / 2, CB = (tw_pad(H) / 16 + 3) / 4;
    return dim3((unsigned)(3 * RB * CB + 3) / 4, (unsigned)tw_chunks((long long)n_tiles * T));
}

// the layer of the Sequential (0 .. LAYERS-1: the GRUs, LAYERS: Dense) that flat element e belongs to: its bit of frozen_mask
template <int LAYERS>
__device__ inline int tw_layer_of(const TwLayer* const (&l)[LAYERS], int e) {
    int layer = LAYERS, end = 0;
#pragma unroll
    for (int i = LAYERS - 1; i >= 0; --i) {
        end = 0;
#pragma unroll
        for (int k = 0; k <= i; ++k) end += train_n_gru(l[k]->K, l[k]->H);
        if (e < end) layer = i;
    }
    return layer;
}

// One thread per parameter (backward launches), then one for the loss.  `l`: the GRU layers in flat order; `partial`
// [n_tiles][H + 3] of the last one.
template <int LAYERS, class Args>
__device__ inline void tw_reduce(const Args& a, const TwLayer* const (&l)[LAYERS], const float* partial) {
    const int H = l[LAYERS - 1]->H;
    int n_gru = 0;
#pragma unroll
    for (int i = 0; i < LAYERS; ++i) n_gru += train_n_gru(l[i]->K, l[i]->H);
    const int n_par = a.backward ? n_gru + H + 1 : 0;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_par) {
        float sum = 0.0f;
        const int layer = tw_layer_of(l, e);
        if (layer < LAYERS) {
            const int S = tw_chunks((long long)a.n_tiles * a.T);
            int ofs = 0;
#pragma unroll
            for (int i = 0; i < LAYERS; ++i) {
                const int n_own = train_n_gru(l[i]->K, l[i]->H);
                if (layer == i)
                    for (int c = 0; c < S; ++c) sum += l[i]->gpart[(size_t)c * n_own + (e - ofs)];
                ofs += n_own;
            }
        } else {
            const float* p = partial + (e - n_gru);
            for (int b = 0; b < a.n_tiles; ++b) sum += p[(size_t)b * (H + 3)];
        }
        a.grads[e] = sum;
        if (a.apply && !((a.frozen_mask >> layer) & 1)) train_rmsprop(a.theta[e], a.accum[e], sum, a.lr, a.rho, a.eps);
    } else if (e == n_par) {
        const float* p = partial + H + 1;
        float la = 0.0f, lb = 0.0f;
        for (int b = 0; b < a.n_tiles; ++b) { la += p[(size_t)b * (H + 3)]; lb += p[(size_t)b * (H + 3) + 1]; }
        a.loss[0] = a.beta * (la * a.inv_n) + (1.0f - a.beta) * (lb * a.inv_n);
    }
}

#endif  // __HIPCC__

}  // namespace pe
