// Wide / stacked GRU + Dense forward with bf16 operands (gru_precision = 1 at 33..256 units, 1-2 layers), on
// v_mfma_f32_16x16x32_bf16, gfx950.  The float32 twin is gru_wide_device.h; the narrow bf16 network gru_bf16_device.h.
//
// CONTRACT (oracle/bf16_gru.py B1-B7 at any width):
//   B1  kernels W, U of every layer: rounded to bf16 once, on the host (pack_gru_weights_wide_bf16).
//   B2  bias: hi = bf16(b), lo = bf16(b - hi); the gates see hi + lo.  Here it enters as the accumulator's initial value:
//       float32(hi + lo) is exact (b - hi is exact in float32 and a multiple of ulp(b)), so this is the same number the
//       narrow kernel gets from two k-slots against 1.0.
//   B3  the feature row: rounded (RNE) as it becomes an operand.
//   B6  h (operand of z, r) and r*h (operand of the candidate) of every layer: rounded as operands.  The state that is
//       carried and blended, and the last layer's state under the Dense head, stay float32.
//   B7  accumulation, gates, blend, Dense weights and bias, sigmoid: float32.
//   B8  two layers: layer 2's input operand at timestep t is bf16(h1_t), layer 1's NEW state rounded -- the same rounded
//       copy layer 1 reads as its own B6 operand at t + 1: one copy in LDS serves both.
//   Padded units (widths run at the next multiple of 64) have zero weights and zero bias: z = r = 1/2, candidate 0, and
//   their state, its rounded copy and their r*h are exactly 0.
//
// One workgroup of 4 waves owns one tile of 16 streams for the whole window, as in gru_wide_device.h:
//   * wave w owns output tiles tau = w TPW + tp of every gate; row i of tile tau is unit 16 tau + i, so lane (g, j) holds
//     units 16 tau + 4 g + q (q = 0..3) of stream j in its four D registers;
//   * k-group kappa of a contraction over a state vector is 32 units; k-slot 8 g + e of it is unit
//     32 kappa + 16 (e >> 2) + 4 g + (e & 3): the four values a lane holds of tile tau are slots e = 4 (tau & 1) + q of
//     k-group tau >> 1 AT ITS OWN LANE.  A tile's rounded state goes to LDS as one ds_write_b64 per lane, and ONE
//     ds_read_b128 per lane brings back the eight k-values of a B operand;
//   * LDS holds ROUNDED operands only, [layer][h | r*h][k-group][lane] x 16 bytes: 1 KB per k-group, 8 KB per vector at
//     256 units, 32 KB for 2 layers -- HALF of the float32 kernel's 64 KB (decision: the float32 state is needed by its
//     owner alone, which keeps it in registers, `hown`; nobody else ever reads an unrounded value).  The array is static
//     and sized for 256 units x 2 layers whatever the width;
//   * weights are streamed from L2 every timestep as A operands, one stream per layer and phase,
//     [wave][k-group: input part, then recurrent part][tile][lane] x 16 bytes (8 bf16), 8 - 16 KB per wave ahead of their
//     use (wide_bf16_phase; trip counts are template constants, so no branch sits in the chain): 1.2 MB per timestep and
//     workgroup at 256 x 2, which is what sets the time (74 % of 64 B/clk/CU from L2; the MFMAs need a fifth);
//   * registers (no scratch, no spills): 112-120 VGPRs at 64 units, 210-214 at 128, 256 + 222-242 AGPRs at 192 / 256;
//   * layer 1's input: lane groups 0, 1 hold features 0..7 / 8..15 of the row, groups 2, 3 zeros: K = 32 swallows the
//     <= 16 features in one MFMA per output tile;
//   * per layer and timestep: phase 1 (z, r), barrier, phase 2 (candidate, blend), barrier.
#pragma once
#include "gru_bf16_device.h"

namespace pe {

constexpr int kWideBf16LdsBytes = 2 * 2 * 8 * 1024;      // 2 layers x {h, r*h} x 8 k-groups (256 units) x 1 KB

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// One phase of one layer: acc[tl] += sum over the phase's k-groups of W . B.  The phase's weights are ONE stream,
// [k-group][tile][lane] x 16 bytes: first the input part -- XREG: one group against the feature row in registers; else KIN
// groups against layer 1's rounded state in LDS, Bin --, then the KG groups of the recurrent part (B operand: h or r*h in
// LDS, Bst; 64 uint4 per k-group).  Weights travel through a register ring D k-groups ahead of their use -- about 16 KB per
// wave in flight: one group ahead (8 KB at most) left the L2 stream latency-bound --, the slot of group k refilled with
// group k + D as soon as its MFMAs are issued.  The group count is a template constant and a multiple of D: the last D
// groups are an unrolled epilogue without prefetch, so there is neither a branch in the chain nor a re-read of the last group.
// DEEP (192 and 256 units): the ring as deep as that (0.313 against 0.345 ms per launch at 256 x 2, 4096 streams).  The narrower
// widths keep 8 KB in flight and fewer registers, so four (64 units) or two (128 units) workgroups share a compute unit and
// hide each other's latency: measured at 128 units, 65 536 streams, 0.60 ms per launch against 0.79 with the deep ring at
// one workgroup per compute unit, and 0.049 either way at 4096 streams.
template <int NT, int KIN, int KG, bool XREG, bool DEEP>
__device__ __forceinline__ void wide_bf16_phase(f32x4 (&acc)[NT], const uint4* __restrict__ w, const bf16x8& x, const uint4* Bin, const uint4* Bst) {
    constexpr int KI = XREG ? 0 : KIN;          // input groups that go through the ring
    constexpr int N = KI + KG;
    constexpr int CAP = DEEP ? (NT >= 8 ? 2 : NT >= 6 ? 3 : NT >= 4 ? 4 : 6) : (NT >= 4 ? 2 : NT >= 2 ? 4 : 8);
    constexpr int D = CAP < N ? CAP : N;
    static_assert(N % D == 0, "the ring depth divides the group count");
    constexpr bool ALLB = D == N && NT <= 2;    // short phases of short MFMA groups: every B operand is requested up front
    uint4 xw[XREG ? NT : 1];
    if constexpr (XREG) {
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) xw[tl] = w[tl * 64];
        w += NT * 64;
    }
    uint4 st[D][NT];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) st[d][tl] = w[(d * NT + tl) * 64];
    auto bsrc = [&](const int k) -> uint4 { return *(k < KI ? Bin + k * 64 : Bst + (k - KI) * 64); };
    uint4 ball[ALLB ? N : 1];
    if constexpr (ALLB) {
#pragma unroll
        for (int k = 0; k < N; ++k) ball[k] = bsrc(k);
    }
    uint4 b = bsrc(0);
    if constexpr (XREG) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) acc[tl] = mfma_bf16(__builtin_bit_cast(bf16x8, xw[tl]), x, acc[tl]);
    }
#pragma unroll 1
    for (int k0 = 0; k0 < N - D; k0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const uint4 bn = bsrc(k0 + u + 1);
            __builtin_amdgcn_sched_barrier(0);                           // the loads are issued HERE, not sunk below the MFMAs
            const bf16x8 bb = __builtin_bit_cast(bf16x8, b);
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) acc[tl] = mfma_bf16(__builtin_bit_cast(bf16x8, st[u][tl]), bb, acc[tl]);
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) st[u][tl] = w[((D + u) * NT + tl) * 64];
            __builtin_amdgcn_sched_barrier(0);
            b = bn;
        }
        w += D * NT * 64;
    }
#pragma unroll
    for (int u = 0; u < D; ++u) {
        uint4 bn = b;
        if (!ALLB && u + 1 < D) bn = bsrc(N - D + u + 1);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 bb = __builtin_bit_cast(bf16x8, ALLB ? ball[u] : b);
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) acc[tl] = mfma_bf16(__builtin_bit_cast(bf16x8, st[u][tl]), bb, acc[tl]);
        __builtin_amdgcn_sched_barrier(0);
        b = bn;
    }
}

// four float32 values -> four bf16 (RNE, v_cvt_pk_bf16_f32) as 8 bytes
__device__ __forceinline__ uint2 round_bf16x4(const float a, const float b, const float c, const float d) {
    bf16x4 o;
    o[0] = (__bf16)a; o[1] = (__bf16)b; o[2] = (__bf16)c; o[3] = (__bf16)d;
    return __builtin_bit_cast(uint2, o);
}

// MODE as in gru_device.h (kFeats / kRing / kRows).  WideArgs as the float32 kernel takes it, read differently: wx1 / wx2
// are the phase's whole stream (input part, then recurrent part) in 16-byte groups of eight bf16, wr1 / wr2 are unused and
// kx4 counts the input part's k-groups of 32.  lds: kWideBf16LdsBytes.
template <int TPW, int MODE>
__device__ __forceinline__ void gru_wide_bf16_tile(const WideArgs& wa, const int tile, const int wave, const int lane, unsigned char* lds) {
#pragma clang fp contract(off)      // every fusion in the gate arithmetic is spelled out: all kernel shapes round alike
    const GruArgs& a = wa.base;
    constexpr int KG = 2 * TPW;                     // k-groups of 32 units per state vector (H = 64 TPW)
    constexpr bool DEEP = TPW >= 3;
    const int g = lane >> 4, j = lane & 15;
    const long long stream = (long long)tile * kTileStreams + j;
    const bool valid = stream < a.n_streams;
    const int T = a.n_features;
    const int L = wa.n_layers;

    // ---- input addressing: lane group g < 2 supplies features 8 g .. 8 g + 7; groups 2, 3 read what group g & 1 reads
    //      (a legal address) and supply zeros ------------------------------------------------------------------------------
    const int fg = 8 * (g & 1);
    const float* xbase = nullptr;
    uint32_t first = 0;
    const uint32_t mask = (uint32_t)(a.ring_slots - 1);
    if (MODE == kRing) {
        const long long sid = gru_stream_of(a, stream, valid);      // the stream whose record and ring rows this lane reads
        const uint32_t ke = gru_window_end(a, sid);
        first = ke - (uint32_t)T;
        xbase = a.ring + gru_ring_cell(a, sid) * kRowFloats + fg;
    } else if (MODE == kRows) {
        xbase = a.feats + ((size_t)(valid ? stream : 0) * a.row_stride) * kRowFloats + fg;
    } else {
        xbase = a.feats + (size_t)(valid ? stream : 0) * T * a.n_in;
    }
    struct XRaw { f32x4 lo, hi; };
    auto load_x = [&](int t) -> XRaw {
        const int tc = t < T ? t : T - 1;
        XRaw r;
        if (MODE == kRing || MODE == kRows) {
            const float* p = MODE == kRing ? xbase + (size_t)((first + (uint32_t)tc) & mask) * kTileStreams * kRowFloats
                                           : xbase + (size_t)tc * kRowFloats;
            r.lo = *reinterpret_cast<const f32x4*>(p);
            r.hi = *reinterpret_cast<const f32x4*>(p + 4);
            return r;
        }
        r.lo = f32x4{0.f, 0.f, 0.f, 0.f}; r.hi = r.lo;
        const float* p = xbase + (size_t)tc * a.n_in;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (valid && fg + i < a.n_in) r.lo[i] = p[fg + i];
            if (valid && fg + 4 + i < a.n_in) r.hi[i] = p[fg + 4 + i];
        }
        return r;
    };
    auto make_x = [&](const XRaw& r) -> bf16x8 {                     // B3: rounded as it becomes an operand
        uint4 u;
        const uint2 p0 = round_bf16x4(r.lo[0], r.lo[1], r.lo[2], r.lo[3]), p1 = round_bf16x4(r.hi[0], r.hi[1], r.hi[2], r.hi[3]);
        u.x = g < 2 ? p0.x : 0u; u.y = g < 2 ? p0.y : 0u; u.z = g < 2 ? p1.x : 0u; u.w = g < 2 ? p1.y : 0u;
        return __builtin_bit_cast(bf16x8, u);
    };

    // ---- LDS operands: h0 = 0 --------------------------------------------------------------------------------------
    uint4* const lds4 = reinterpret_cast<uint4*>(lds);
    uint4* HB[2] = {lds4, lds4 + 2 * 8 * 64};                        // [layer]: h then r*h, 8 k-groups x 64 lanes each
    uint4* RH[2] = {lds4 + 8 * 64, lds4 + 3 * 8 * 64};
    for (int i = threadIdx.x; i < kWideBf16LdsBytes / 16; i += 256) lds4[i] = uint4{0u, 0u, 0u, 0u};
    float hown[2][TPW][4];
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
            for (int q = 0; q < 4; ++q) hown[l][tp][q] = 0.f;
    __syncthreads();

    XRaw xr = load_x(0);
    for (int t = 0; t < T; ++t) {
        const bf16x8 x = make_x(xr);
        xr = load_x(t + 1);
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            if (l >= L) break;
            const WideLayerArgs& W = wa.layer[l];
            const uint4* Xin = l == 0 ? nullptr : HB[l - 1] + lane;          // B8: layer 1's rounded new state
            // ---- phase 1: z and r of this wave's units ----------------------------------------------------
            f32x4 acc[2 * TPW];
#pragma unroll
            for (int tl = 0; tl < 2 * TPW; ++tl)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[tl][q] = W.b1[((wave * 2 * TPW + tl) * 4 + q) * 64 + lane];
            const uint4* w1 = reinterpret_cast<const uint4*>(W.wx1) + (size_t)wave * (W.kx4 + KG) * 2 * TPW * 64 + lane;
            if (l == 0) wide_bf16_phase<2 * TPW, 1, KG, true, DEEP>(acc, w1, x, nullptr, HB[l] + lane);
            else wide_bf16_phase<2 * TPW, KG, KG, false, DEEP>(acc, w1, x, Xin, HB[l] + lane);
            float z[TPW][4];
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) {
                float rh[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    z[tp][q] = hard_sigmoid(acc[tp][q]);
                    rh[q] = hard_sigmoid(acc[TPW + tp][q]) * hown[l][tp][q];
                }
                const int tau = wave * TPW + tp;
                reinterpret_cast<uint2*>(RH[l] + (tau >> 1) * 64 + lane)[tau & 1] = round_bf16x4(rh[0], rh[1], rh[2], rh[3]);
            }
            __syncthreads();
            // ---- phase 2: candidate and state update ---------------------------------------------------------
            f32x4 acc2[TPW];
#pragma unroll
            for (int tl = 0; tl < TPW; ++tl)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc2[tl][q] = W.b2[((wave * TPW + tl) * 4 + q) * 64 + lane];
            const uint4* w2 = reinterpret_cast<const uint4*>(W.wx2) + (size_t)wave * (W.kx4 + KG) * TPW * 64 + lane;
            if (l == 0) wide_bf16_phase<TPW, 1, KG, true, DEEP>(acc2, w2, x, nullptr, RH[l] + lane);
            else wide_bf16_phase<TPW, KG, KG, false, DEEP>(acc2, w2, x, Xin, RH[l] + lane);
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) {
#pragma unroll
                for (int q = 0; q < 4; ++q) hown[l][tp][q] = gru_blend(z[tp][q], hown[l][tp][q], acc2[tp][q]);
                const int tau = wave * TPW + tp;
                reinterpret_cast<uint2*>(HB[l] + (tau >> 1) * 64 + lane)[tau & 1] =
                    round_bf16x4(hown[l][tp][0], hown[l][tp][1], hown[l][tp][2], hown[l][tp][3]);
            }
            __syncthreads();
        }
    }

    // ---- Dense(1) + sigmoid over the last layer's UNROUNDED state: lane -> lane groups -> waves ------------------------
    float part = 0.f;
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float hv = (L == 2) ? hown[1][tp][q] : hown[0][tp][q];
            part = fmaf(hv, wa.wd[((wave * TPW + tp) * 4 + q) * 64 + lane], part);
        }
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    float* const red = reinterpret_cast<float*>(lds);                // (every read of the operands is behind the last barrier)
    if (g == 0) red[wave * 16 + j] = part;
    __syncthreads();
    if (wave == 0 && g == 0 && valid) {
        float logit = red[j];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) logit += red[wv * 16 + j];
        a.out[stream] = 1.0f / (1.0f + expf(-(logit + a.dense_bias)));
    }
}

}  // namespace pe
