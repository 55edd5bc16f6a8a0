// Stock-width float32 GRU (gru_cw_device.h), form 1 CARRIED: the chain of every live window start stays on the device
// between updates, and an update advances each of them by the rows it makes visible instead of running 29 timesteps again.
//
// Consecutive windows of a stream share all but the k rows an update makes visible (k <= 2 for the chunks this form is
// launched for: engine.hip chain_eligible).  The window that ends at emitted row ke - 1 is the chain that started at row
// ke - T; the window of the NEXT update started k rows later.  So a stream keeps the state h of the chain of every start
// s in (ke - T - 1, ke - 1]: T of them, the chain of age a = ke - s having consumed the rows s .. ke - 1.  An update then
//   * computes the input projections of its k new rows ONCE per workgroup, a tile of them per wave, handed round through an LDS
//     mailbox behind one barrier (they were 16 of the 41 MFMAs of every timestep of every window),
//   * advances each of the T chains by min(a, k) steps of CwStep<false>::step -- the function gru_tile_v runs, bit-identical
//     to gru_tile_cw -- (a chain of age a <= k is born in this update: it starts from h = 0),
//   * and the chain that reaches age T is the window: Dense + sigmoid of its state is the output.
// T independent chains of <= 2 steps instead of one chain of 29: a throughput job for the SIMDs of the machine; its only LDS
// is the projections' mailbox and its only barrier the one behind it (gru_tile_chains, "The prologue").
//
// State.  chains: float32 [stream tile][kCwSlots][5 rho][64 lanes]; slot = start row & (kCwSlots - 1), the indexing of the
// feature ring; lane (g, j) holds unit 4 rho + g of stream 16 tile + j (CwStep's h[rho]).  A slot is reused by the chain
// that starts kCwSlots rows later, when its old chain (age > T) is dead.  chain_ke[stream]: the emitted count the stream's
// chains are current to -- a cross-check only (the host decides validity, engine.hip: chain_epoch): a stream whose stamp is
// not the count its record holds gets a quiet NaN for an output, which no caller and no test can miss.
#pragma once
#include "gru_cw_device.h"

namespace pe {

// (ChainArgs: pe_common.h)
constexpr int kChainMaxRows = 2;        // rows one chain launch may make visible per stream
constexpr int kChainSkipAges = 7;       // ages of a stream whose alive bits one of its four lane groups forms (ChainArgs::skip)
static_assert(4 * kChainSkipAges >= kCwSlots - 3 - 1, "the four lane groups cover the ages 1 .. T - 1 of the longest window (chain_eligible)");
// OR over the wave's active lanes: the DPP reduction of the ROCm device library (ockl), the one hip/amd_detail/amd_warp_sync_functions.h
// builds __reduce_or_sync on.  It is no documented interface: checked against ROCm 7.2.0; should a release drop it the link
// fails (nothing falls back quietly), and six __shfl_xor steps in its place give the same value.
extern "C" __device__ uint32_t __ockl_wfred_or_u32(uint32_t);

// first float of the chain that started at a row of slot `slot`, for the lane of lane group g that serves stream sid
__device__ __forceinline__ size_t chain_cell(const long long sid, const uint32_t slot, const int g) {
    return (((size_t)(sid >> 4) * kCwSlots + slot) * 5) * 64 + (size_t)(g * 16) + (size_t)(sid & 15);
}
__device__ __forceinline__ void chain_load(const float* chains, const size_t cell, float (&h)[5]) {
#pragma unroll
    for (int rho = 0; rho < 5; ++rho) h[rho] = chains[cell + (size_t)rho * 64];
}
// WT: the five stores are written through the L2 (relaxed agent-scope atomic stores: global_store_dword ... sc1) instead of left
// dirty in it for the kernel boundary to write back.  A cell's next reader is a later launch, so no value changes; which
// instantiations gain by it is measured (profiles/chain_store/README.md).
template <bool WT>
__device__ __forceinline__ void chain_store(float* chains, const size_t cell, const float (&h)[5], const bool on) {
    if (!on) return;
#pragma unroll
    for (int rho = 0; rho < 5; ++rho) {
        if constexpr (WT) __hip_atomic_store(chains + cell + (size_t)rho * 64, h[rho], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else chains[cell + (size_t)rho * 64] = h[rho];
    }
}

// the timestep's weights, which every wave of this form keeps
struct ChainStep {
    CwStep<false> S;
    // one timestep for the lanes with `on`; the others keep their state (an MFMA column depends on its own B column only, so
    // what the other lanes computed is dropped without a trace in these)
    __device__ __forceinline__ void step_if(float (&h)[5], const f32x4 (&p)[4], const bool on) const {
        float hn[5];
#pragma unroll
        for (int rho = 0; rho < 5; ++rho) hn[rho] = h[rho];
        S.step(hn, p[kTZ], p[kTX], p[kTC], p[kTV]);
#pragma unroll
        for (int rho = 0; rho < 5; ++rho) h[rho] = on ? hn[rho] : h[rho];
    }
};
// ... with the whole input kernel and the biases (the rebuild: every wave projects the rows of its own chains)
struct ChainNet : ChainStep {
    float wx[4][4];
    f32x4 bias[4];
    __device__ __forceinline__ void load(const float* cw, const int lane) {
        S.load(cw, lane);
#pragma unroll
        for (int tl = 0; tl < 4; ++tl)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                wx[tl][kk] = cw[CwPack::WX + (tl * 4 + kk) * 64 + lane];
                bias[tl][kk] = cw[CwPack::BIAS + (tl * 4 + kk) * 64 + lane];
            }
    }
    // x.W + b of the four tiles, as gru_tile_v forms them
    __device__ __forceinline__ void project(const f32x4& x, f32x4 (&p)[4]) const {
        p[kTZ] = cw_xproj(wx[kTZ], bias[kTZ], x); p[kTX] = cw_xproj(wx[kTX], bias[kTX], x);
        p[kTC] = cw_xproj(wx[kTC], bias[kTC], x); p[kTV] = cw_xproj(wx[kTV], bias[kTV], x);
    }
};

// LDS of a chain workgroup (floats): the mailbox of the new rows' projections, at the start of the launch's dynamic LDS
struct ChainLds {
    static constexpr int BOX = 0;                               // [kChainMaxRows][4 tiles][64 lanes][4]
    static constexpr int FLOATS = kChainMaxRows * 4 * 256;
};
constexpr size_t kChainLdsBytes = (size_t)ChainLds::FLOATS * sizeof(float);

// ---- the network role of a chain launch: NW waves per tile, wave w takes the chains of age a = w (mod NW) ----------------
// NW = 4 (one workgroup per tile) when the call names most of the engine's streams: the frame role is then the long pole of
// the launch and every chain wave's MFMAs take issue cycles from it.  NW = 8 (two workgroups per tile) for sparse subset
// calls, where this role is the long pole: a chain of memory round trips and of a wave's chains two at a time, which more
// waves shorten (and there the next two chains' state is requested ahead).
// Measured: profiles/chain_carry/README.md, profiles/chain_launch/README.md.
//
// The prologue.  One round trip for the record, the stamp and the weights; a second for the new rows and the first two
// chains.  The new rows are projected once per WORKGROUP, not once per wave: wave w computes tile w of {TZ, TX, TC, TV} --
// it holds that tile's input kernel and bias only (8 registers, where the whole kernel took 32) --, leaves its f32x4 per row
// in the LDS mailbox, and after one workgroup barrier every wave reads all four.  cw_xproj is a function of (tile, row)
// alone, so the bits are those of a wave that projects for itself; what goes is three quarters of the projections' matrix
// cycles, which an f32-input MFMA takes from every wave of its SIMD, the frame role's included.
// S: the workgroup's dynamic LDS, kChainLdsBytes of it (kernels.hip: launch_fused_chains_t asserts the budget).
//
// The records hold the state BEFORE the update (predict_ke, as for every network role of a fused launch).  Lanes of one
// tile may make different numbers of rows visible (subset calls, streams out of phase): the wave runs the largest trip
// count and every lane keeps what is its own.
// SKIP: ChainArgs::skip, as a template argument.  The two settings are two instantiations behind ONE branch that is uniform across
// the launch (gru_tile_chains, below), not one body with tests inside: with both loops in one body the register allocator spilled
// 48 bytes per lane, and callers whose chunks are at most a hop, or change, keep the stride loop this form always had.
template <int NW, bool SKIP>
__device__ __forceinline__ void gru_tile_chains_t(const GruArgs& a, const ChainArgs& ch, const int tile, const int wave, const int lane, float* const S) {
    // chain_store's policy: the four-wave stride loop was slower with write-through stores, every other instantiation faster
    // (profiles/chain_store/README.md)
    constexpr bool kWriteThrough = SKIP || NW == 8;
    const int g = lane >> 4, j = lane & 15;
    const long long stream = (long long)tile * kTileStreams + j;
    const bool valid = stream < a.n_streams;
    const int T = a.n_features;
    const int wl = wave & 3;                // the wave within its workgroup: the tile it projects
    // ---- one round trip: the record, the stamp, the weights -----------------------------------------------------
    const long long sid = gru_stream_of(a, stream, valid);
    const KeRequest ke_req = gru_ke_request(a, sid);
    const uint32_t stamp = ch.chain_ke[sid];
    ChainStep N;
    N.S.load(a.cw, lane);
    float wx[4];
    f32x4 bias;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        wx[kk] = a.cw[CwPack::WX + (wl * 4 + kk) * 64 + lane];
        bias[kk] = a.cw[CwPack::BIAS + (wl * 4 + kk) * 64 + lane];
    }
    float wd[5];
#pragma unroll
    for (int rho = 0; rho < 5; ++rho) wd[rho] = a.wd[rho * 64 + lane];
    // (gru_ke_resolve's arithmetic with its remainder: the launcher refuses a launch without predict_ke or with ke_plain)
    const StreamRec rec = rec_pick(ke_req.p, rec_side(ke_req.p, a.call));
    const KeStep st = ke_step(rec.q, rec.kc, rec.ke, a.chunk, a.hop, a.frame_len, a.window);
    const uint32_t ke_pre = rec.ke, ke_post = st.ke;
    const uint32_t k = ke_post - ke_pre;
    // (decided here, as a lane mask in scalar registers: left to the compiler the stamp stays in a register through the loop)
    const unsigned long long stale = __ballot(stamp != ke_pre || k > (uint32_t)kChainMaxRows);
    // (the waves of a workgroup serve the same 16 streams, so kmax is uniform across the WORKGROUP, not only across the wave)
    const int kmax = __any(k >= 2u) ? 2 : __any(k >= 1u) ? 1 : 0;       // (k > kChainMaxRows: refused below, never run)
    // ---- the chains this wave advances: bit A of `mine` = the chain of (post-update) age A ---------------------------
    // ch.skip: a chain that no update of a caller who keeps this chunk will hand out (chain_alive_bits, pe_common.h) is neither
    // loaded, stepped nor stored.  A lane group g forms the bits of seven of its stream's ages; the OR over the valid lanes is
    // what the tile acts on (streams of a subset call are out of phase: a chain is skipped only if it is dead for all sixteen;
    // one that rides along for a neighbour computes on stale state in its own MFMA column, and nobody reads it).  Every wave
    // of the tile finds the same mask: they serve the same sixteen streams.  Age T is the window of this update.
    uint32_t alive = (2u << T) - 2u;
    if constexpr (SKIP) {
        const uint32_t own = valid ? chain_alive_bits(st.rem, a.chunk, a.hop, a.window, T, g * kChainSkipAges, kChainSkipAges) : 0u;
        alive = (uint32_t)__builtin_amdgcn_readfirstlane((int)__ockl_wfred_or_u32(own)) | (1u << T);
    }
    // Wave w takes the alive ages = w (mod NW), the head the wave of age T, with or without skipping.  Handing the alive ages
    // round by RANK instead (dead ages lie four or five apart and pile onto one wave) was built and measured too: slower on every
    // path (12.93 against 12.82 us per full update, 10.79 against 10.33 for a quarter subset, profiles/chain_skip/README.md).
    uint32_t mine = alive & ((NW == 4 ? 0x11111111u : 0x01010101u) << wave);
    const int head_wave = T % NW;
    auto pop = [](uint32_t& m) -> int { const int age = m ? __builtin_ctz(m) : 0; m &= m - 1u; return age; };   // lowest age, 0 = none left
    constexpr bool kAhead = NW > 4;
    const uint32_t smask = (uint32_t)(kCwSlots - 1);
    const float* xbase = a.ring + gru_ring_cell(a, sid) * kRowFloats + 4 * g;
    f32x4 p0[4], p1[4];
    // row ke_pre + i is consumed by the chain of (post-update) age A iff it exists then: i < k and i >= k - A
    auto advance = [&](float (&h)[5], const uint32_t A) {
        if (kmax >= 1) N.step_if(h, p0, 0u < k && k <= A);
        if (kmax >= 2) N.step_if(h, p1, 1u < k && k <= A + 1u);
    };
    const bool moved = valid && k > 0u;
    // the pair of chains in flight.  A wave takes its ages in rising order, so on the wave that owns age T the window's state is
    // what its last pair leaves: h1 if that was a pair (last_two), else h0
    float h0[5], h1[5];
    bool last_two = false;
#pragma unroll
    for (int rho = 0; rho < 5; ++rho) h0[rho] = h1[rho] = 0.f;
    if (kmax == 0) {
        // nothing became visible anywhere in the tile: the window is the stored chain of age T
        if (wave == head_wave) chain_load(ch.chains, chain_cell(sid, (ke_post - (uint32_t)T) & smask, g), h0);
    } else {
        // ---- second round trip: the new rows and the first chains -----------------------------------------------
        // (the second row is requested whether or not it is new -- its slot exists: a load under a branch is waited for at the
        //  join, in front of the chains' requests)
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(xbase + (size_t)(ke_pre & smask) * kTileStreams * kRowFloats);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(xbase + (size_t)((ke_pre + 1u) & smask) * kTileStreams * kRowFloats);
        // (age 0 = no chain: the cell of age T is requested in its place and the state dropped)
        auto cell_of = [&](const int age) -> size_t { return chain_cell(sid, (ke_post - (uint32_t)(age ? age : T)) & smask, g); };
        int a0 = pop(mine), a1 = pop(mine);
        float n0[5], n1[5];
        chain_load(ch.chains, cell_of(a0), n0);
        chain_load(ch.chains, cell_of(a1), n1);
        // ---- one projection per workgroup.  This branch is uniform across the workgroup (kmax, above) and no lane-divergent
        // code encloses it, so every wave of the workgroup reaches the barrier.  Only what THIS launch wrote is read back: row
        // 0 is written by all four waves whenever the branch is taken, row 1 is written and read under the same kmax >= 2
        // (what an earlier workgroup left in the LDS is never looked at)
        float* const box = S + ChainLds::BOX + lane * 4;
        *reinterpret_cast<f32x4*>(box + (0 * 4 + wl) * 256) = cw_xproj(wx, bias, x0);
        if (kmax >= 2) *reinterpret_cast<f32x4*>(box + (1 * 4 + wl) * 256) = cw_xproj(wx, bias, x1);
        cw_barrier();
#pragma unroll
        for (int tl = 0; tl < 4; ++tl) {
            p0[tl] = *reinterpret_cast<const f32x4*>(box + (0 * 4 + tl) * 256);
            if (kmax >= 2) p1[tl] = *reinterpret_cast<const f32x4*>(box + (1 * 4 + tl) * 256);
        }
        // two chains at a time: their timesteps are independent, so one's MFMAs fill the other's waits.  The first two came with
        // the rows.  kAhead: the state of the NEXT two is requested before the steps of these (the stores below go to other
        // cells of the same array, which the compiler cannot know: left to it, every pair waits a whole memory round trip for
        // its loads)
        // (fresh: the pair's state is still to be requested; b0, b1: the ages of the wave's next pair, 0 = none)
        auto pair = [&](const int a0, const int a1, const bool fresh, const int b0, const int b1) {
            const uint32_t A0 = (uint32_t)a0, A1 = (uint32_t)a1;
            const bool two = a1 != 0;
            const size_t c0 = cell_of(a0), c1 = cell_of(a1);
            if (!kAhead && fresh) {
                chain_load(ch.chains, c0, n0);
                chain_load(ch.chains, c1, n1);
            }
#pragma unroll
            for (int rho = 0; rho < 5; ++rho) {             // born in this update: from h = 0
                h0[rho] = A0 <= k ? 0.f : n0[rho];
                h1[rho] = A1 <= k ? 0.f : n1[rho];
            }
            if (kAhead && b0) {
                chain_load(ch.chains, cell_of(b0), n0);
                chain_load(ch.chains, cell_of(b1), n1);
            }
            advance(h0, A0);
            if (two) advance(h1, A1);
            chain_store<kWriteThrough>(ch.chains, c0, h0, moved);
            if (two) chain_store<kWriteThrough>(ch.chains, c1, h1, moved);
            last_two = two;
        };
        // Flag clear: the stride of the ages is known.  Flag set: the wave walks the set bits of its part of the mask.
        if constexpr (!SKIP) {
            auto upto = [&](const int age) -> int { return age <= T ? age : 0; };
            for (int s0 = a0; s0; s0 = upto(s0 + 2 * NW))
                pair(s0, upto(s0 + NW), s0 != a0, upto(s0 + 2 * NW), upto(s0 + 3 * NW));
        } else {
            for (bool first = true; a0; first = false) {
                const int b0 = pop(mine), b1 = pop(mine);
                pair(a0, a1, !first, b0, b1);
                a0 = b0; a1 = b1;
            }
        }
    }
    if (wave == head_wave) {
        float hw[5];
#pragma unroll
        for (int rho = 0; rho < 5; ++rho) hw[rho] = last_two ? h1[rho] : h0[rho];
        // a stream whose chains are not current to its record (or that makes more rows visible than this form carries) must
        // not pass for a result
        if ((stale >> lane) & 1ull) hw[0] = __builtin_nanf("");
        cw_head(a, hw, wd, stream, valid, g);
        if (valid && g == 0) ch.chain_ke[sid] = ke_post;
    }
}

template <int NW>
__device__ __forceinline__ void gru_tile_chains(const GruArgs& a, const ChainArgs& ch, const int tile, const int wave, const int lane, float* const S) {
    if (ch.skip) gru_tile_chains_t<NW, true>(a, ch, tile, wave, lane, S);
    else gru_tile_chains_t<NW, false>(a, ch, tile, wave, lane, S);
}

// ---- entering chain mode: all T live chains of every stream from the ring and the records as they stand ------------------
// Chain of age a = a steps from h = 0 over rows ke - a .. ke - 1 (T (T + 1) / 2 steps per stream; once per entry).  Four
// waves per tile, wave w the ages a = w (mod 4), the same step function.
__device__ __forceinline__ void gru_tile_chains_rebuild(const GruArgs& a, const ChainArgs& ch, const int tile, const int wave, const int lane) {
    const int g = lane >> 4, j = lane & 15;
    const long long sid = (long long)tile * kTileStreams + j;       // every stream of the engine, padded ones too (records exist)
    const int T = a.n_features;
    const KeRequest ke_req = gru_ke_request(a, sid);
    ChainNet N;
    N.load(a.cw, lane);
    const uint32_t ke = gru_ke_resolve(a, ke_req);
    const uint32_t smask = (uint32_t)(kCwSlots - 1);
    const float* xbase = a.ring + gru_ring_cell(a, sid) * kRowFloats + 4 * g;
    for (int a0 = wave ? wave : 4; a0 <= T; a0 += 4) {
        float h[5];
#pragma unroll
        for (int rho = 0; rho < 5; ++rho) h[rho] = 0.f;
        const uint32_t start = ke - (uint32_t)a0;
        for (int i = 0; i < a0; ++i) {
            f32x4 p[4];
            N.project(*reinterpret_cast<const f32x4*>(xbase + (size_t)((start + (uint32_t)i) & smask) * kTileStreams * kRowFloats), p);
            N.S.step(h, p[kTZ], p[kTX], p[kTC], p[kTV]);
        }
        chain_store<true>(ch.chains, chain_cell(sid, start & smask, g), h, true);
    }
    if (wave == 0 && g == 0) ch.chain_ke[sid] = ke;
}

}  // namespace pe
