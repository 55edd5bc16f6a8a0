// Every __global__ entry point of libprecise_engine.so and its launcher.  The device code lives
// in mfcc_wave_device.h / mfcc_device.h (MFCC front end: frames / bookkeeping) and gru_*_device.h (GRU + Dense
// on the matrix cores).  What is said once here: a network shape (tile function, threads, LDS) is a Net* functor, run by
// its one-model kernel, by gru_models_kernel and by the pe_update_many kernels (three kernels write the same call out: noted there); a fused update has one body per role layout
// (float32 network, bf16 network) with a compile-time flag for "several models"; every `name` / `name_nopk` pair is one
// PE_KERNEL_PAIR; a runtime mode / flag becomes a template argument through with_const.
// The front end has four kinds of launch (streaming, whole buffer, clip table, recording table) in two families (the stock-shape
// wave kernels, the general front end) and two precisions.  Each kind of each family is ONE launcher here, a template over the
// precision R instantiated for double and float (PE_FRONT_END_LAUNCHERS); the table shape and the mel-row flag of the stock family
// become template arguments in with_frame_shape, the transform length and the mel-row flag of the general family in
// with_general_bits.  Family and precision are chosen by the callers: engine.hip, one function per kind (launch_*_front_end),
// the precision through with_real.
#include <cstdlib>
#include <type_traits>
#include "mfcc_device.h"
#include "mfcc_wave_device.h"
#include "gru_device.h"
#include "gru_cw_device.h"
#include "gru_chain_device.h"
#include "gru_bf16_device.h"
#include "gru_b20_device.h"
#include "gru_x3_device.h"
#include "gru_wide_device.h"
#include "gru_wide_x3_device.h"
#include "gru_wide_bf16_device.h"
#include "mfcc_general_device.h"
#include "gru_train_device.h"

namespace pe {

// ---- MFCC: one frame task per wave (mfcc_wave_device.h), bookkeeping per stream (mfcc_device.h) ------------------
#ifndef PE_FRAME_WPE
#define PE_FRAME_WPE 4          // waves per SIMD the frame role is compiled for (<= 128 VGPRs)
#endif
// workgroups [0, n_frame_blocks): frame tasks; the rest: one bookkeeping workgroup per tile (they read what the
// frame tasks read and write elsewhere, so the two roles share a launch)
// Every 64-byte line of a kernel's argument segment, requested by the first instructions of the kernel.  The role
// selection reads the trailing integers, waits, branches, and only then do the role's own pointers get loaded -- from
// other cache lines, after a second miss of the scalar cache (two memory round trips in series before the first vector
// load can go out; ISA, round 3).  With every line on its way behind ONE wait the later scalar loads hit.
template <int BYTES>
__device__ __forceinline__ void touch_kernel_arguments() {
    const int* ka = (const int*)__builtin_amdgcn_kernarg_segment_ptr();
    static_assert(BYTES <= 12 * 64, "more lines than this helper requests");
    auto line = [&](int i) -> int { return i * 64 < BYTES ? ka[i * 16] : 0; };
    const int v0 = line(0), v1 = line(1), v2 = line(2), v3 = line(3), v4 = line(4), v5 = line(5), v6 = line(6), v7 = line(7),
              v8 = line(8), v9 = line(9), v10 = line(10), v11 = line(11);
    asm volatile("" :: "s"(v0), "s"(v1), "s"(v2), "s"(v3), "s"(v4), "s"(v5), "s"(v6), "s"(v7), "s"(v8), "s"(v9), "s"(v10), "s"(v11));
}

// Every kernel that hosts the FLOAT32 frame role exists twice: `name` (R = double) and `name_nopk` (R = float), the second
// compiled without packed float32 instructions (v_pk_add/mul/fma_f32).  Why: round 4 found ~0.7 % of the float32 frames of
// a fused launch slightly wrong, timing-dependent, beside the five-values bf16 network role (gru_b20_device.h;
// profiles/round4/r4v_b20_fused_corruption.log); the one change that cured it in every run (4 / 4 in round 4, 2 / 2 and the
// 1e8-frame soaks in round 5) is this one, and it is also FASTER: hipcc's SLP pass packs the butterflies' additions, and on
// gfx950 packed float32 shares the XDL datapath (tools/micro/pipe_overlap.hip; MI355X_MICROARCH: "an anti-lever beside MFMAs")
// -- MFCC launch 51.3 vs 52.9 us at 65 536 streams, fused bf16 update 73.1 vs 75.6 us (profiles/round5/r5a_*).  The attribute
// applies to the whole kernel (code generation is per function), which is why it cannot sit on the frame function itself.
#if defined(__HIP_DEVICE_COMPILE__)
#define PE_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PE_NO_PK_F32            // (the host pass only sees the launch stubs)
#endif
#define PE_UNPAREN(...) __VA_ARGS__
// `NAME` and its twin `NAME_nopk` (the same body under PE_NO_PK_F32): TEMPLATE and ATTRS in parentheses, the body last
#define PE_KERNEL_PAIR(TEMPLATE, ATTRS, NAME, PARAMS, ...)                                                   \
    PE_UNPAREN TEMPLATE __global__ PE_UNPAREN ATTRS void NAME PARAMS __VA_ARGS__                            \
    PE_UNPAREN TEMPLATE __global__ PE_UNPAREN ATTRS PE_NO_PK_F32 void NAME##_nopk PARAMS __VA_ARGS__
#define PE_FRAME_KERNEL(THREADS, WPE) (__launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(WPE))))
// launch KERNEL<R, TARGS...> -- its _nopk twin when R is float
#define PE_LAUNCH_R(R, KERNEL, TARGS, ...)                                                                   \
    do {                                                                                                     \
        if constexpr (std::is_same<R, float>::value) hipLaunchKernelGGL((KERNEL##_nopk<R, PE_UNPAREN TARGS>), __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<R, PE_UNPAREN TARGS>), __VA_ARGS__);                                 \
    } while (0)

// A runtime value as a compile-time one: f(std::integral_constant<int, V>{}) for the V that equals v; false if none does.
// The launchers turn the input mode (kRing / kRows / kFeats), flags and small counts into template arguments with it.
template <int... V, class F>
static bool with_const(int v, F&& f) { return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...); }
// (the input mode: anything that is neither the ring nor a row sequence is an explicit batch, as the ladders had it)
template <class F> static bool with_mode(int mode, F&& f) { return with_const<kRing, kRows, kFeats>(mode == kRing || mode == kRows ? mode : kFeats, f); }
template <class F> static bool with_flag(bool on, F&& f) { return with_const<0, 1>(on ? 1 : 0, f); }
#define PE_CONST(X) decltype(X)::value

// SINGLE: one update, no projection rows (the launcher knows): the frame loop without the several-updates arithmetic
// MELS: the rows are the log-mel energies (Vectorizer.mels; mfcc_wave_device.h) -- the two-launch update only: a mel-row engine
// on this kernel (n_filt <= 16) does not fuse (engine.hip can_fuse)
template <class R, class SH, bool SINGLE, bool MELS>
__device__ __forceinline__ void mfcc_kernel_body(const MfccStreamArgs<R>& a, const WaveTables<R>& t, const int n_frame_blocks) {
    touch_kernel_arguments<(int)(sizeof(MfccStreamArgs<R>) + sizeof(WaveTables<R>) + 4)>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if ((int)blockIdx.x < n_frame_blocks) mfcc_frame_tasks<R, SH, SINGLE, SINGLE, MELS>(a, t, smem, (int)blockIdx.x * kFrameWaves, n_frame_blocks * kFrameWaves);
    else mfcc_book_tile<R>(a, (int)blockIdx.x - n_frame_blocks);
}
PE_KERNEL_PAIR((template <class R, class SH, bool SINGLE = false, bool MELS = false>), PE_FRAME_KERNEL(64 * kFrameWaves, SH::WPE), mfcc_kernel,
               (const MfccStreamArgs<R> a, const WaveTables<R> t, const int n_frame_blocks),
               { mfcc_kernel_body<R, SH, SINGLE, MELS>(a, t, n_frame_blocks); })
// a whole buffer's frames (pe_vectorize_raw / pe_vectorize_mels / pe_evaluate)
PE_KERNEL_PAIR((template <class R, class SH, bool MELS = false>), PE_FRAME_KERNEL(64 * kFrameWaves, SH::WPE), mfcc_offline_kernel,
               (const MfccOfflineArgs<R> a, const WaveTables<R> t),
               { extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; mfcc_offline_frames<R, SH, MELS>(a, t, smem); })
// many clips in one launch (pe_vectorize_clips / pe_score_clips): frame tasks found in the clip table (pe_common.h: ClipTable)
PE_KERNEL_PAIR((template <class R, class SH, bool MELS = false>), PE_FRAME_KERNEL(64 * kFrameWaves, SH::WPE), mfcc_clips_kernel,
               (const MfccClipArgs<R> a, const WaveTables<R> t),
               { extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; mfcc_clip_frames<R, SH, MELS>(a, t, smem); })
// many whole recordings in one launch (pe_evaluate_clips / pe_simulate_clips): frame tasks found in the recording table (RecTable)
PE_KERNEL_PAIR((template <class R, class SH, bool MELS = false>), PE_FRAME_KERNEL(64 * kFrameWaves, SH::WPE), mfcc_recs_kernel,
               (const MfccRecArgs<R> a, const WaveTables<R> t),
               { extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; mfcc_rec_frames<R, SH, MELS>(a, t, smem); })

// ---- network shapes: the tile function of a workgroup, its threads and its LDS, said once -------------------------------
// run(a, tile, smem) is the whole network of tile `tile` of the launch `a`.  The one-model kernel of a shape (the names
// the profiles know), gru_models_kernel (K models) and the pe_update_many kernels all run it.  kLds: dynamic LDS of a workgroup;
// kOwnLds: what the shape's one-model kernel asks for at launch (gru_mw_kernel declares its LDS statically).
template <int R, int MODE, bool PROJ, int KX> struct NetSmall {          // one wave per 16-stream tile
    static constexpr int kThreads = 64; static constexpr size_t kLds = 0, kOwnLds = 0;
    static __device__ __forceinline__ void run(const GruArgs& a, int tile, unsigned char*) { gru_tile<R, MODE, PROJ, KX>(a, tile, threadIdx.x); }
};
template <int R, bool PROJ, int KX> struct NetMw {                       // four waves per tile (few tiles: fills all four SIMDs of a CU)
    static constexpr int kThreads = 256; static constexpr size_t kLds = (3 * R * 64 + 256) * sizeof(float), kOwnLds = 0;
    static __device__ __forceinline__ void run(const GruArgs& a, int tile, unsigned char* smem) {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        gru_tile_mw_any<R, PROJ, KX>(a, tile, wave, threadIdx.x & 63, reinterpret_cast<float*>(smem));
    }
};
template <int MODE, bool DELTA> struct NetV {                            // stock width re-tiled (gru_cw_device.h), one wave per tile
    static constexpr int kThreads = 64; static constexpr size_t kLds = 0, kOwnLds = 0;
    static __device__ __forceinline__ void run(const GruArgs& a, int tile, unsigned char*) { gru_tile_v<MODE, DELTA>(a, tile, threadIdx.x); }
};
struct NetCw {                                                           // ... four waves per tile
    static constexpr int kThreads = 256; static constexpr size_t kLds = kCwLdsBytes, kOwnLds = kCwLdsBytes;
    static __device__ __forceinline__ void run(const GruArgs& a, int tile, unsigned char* smem) {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        gru_tile_cw<false>(a, tile, wave, threadIdx.x & 63, reinterpret_cast<float*>(smem));
    }
};
template <int MODE, bool DELTA, bool RB> struct NetBf16 {                // bf16 operands, one wave per tile
    static constexpr int kThreads = 64; static constexpr size_t kLds = 0, kOwnLds = 0;
    static __device__ __forceinline__ void run(const GruArgs& a, int tile, unsigned char*) {
        if (a.b20) { gru_tile_b20<MODE, DELTA, RB>(a, tile, threadIdx.x); return; }      // <= 20 units: five values per lane (gru_b20_device.h)
        gru_tile_bf16<MODE, DELTA, RB>(a, tile, threadIdx.x);
    }
};
template <int MODE> struct NetX3 {                                       // float32 as three bf16 pieces per operand on the XDL pipe
    static constexpr int kThreads = 64; static constexpr size_t kLds = 0, kOwnLds = 0;
    static __device__ __forceinline__ void run(const GruArgs& a, int tile, unsigned char*) { gru_tile_x3<MODE>(a, tile, threadIdx.x); }
};

// ---- the one-model kernel of every shape ----------------------------------------------------------------------------------
template <int R, int MODE, bool PROJ = false, int KX = 1>
__global__ __launch_bounds__(64) void gru_small_kernel(const GruArgs a) {
    touch_kernel_arguments<(int)sizeof(GruArgs)>();
    NetSmall<R, MODE, PROJ, KX>::run(a, blockIdx.x, nullptr);
}
template <int R, bool PROJ = false, int KX = 1>
__global__ __launch_bounds__(256) void gru_mw_kernel(const GruArgs a) {
    // (NetMw<R, PROJ, KX>::run, written out over the kernel's static LDS: through the functor the code of the K-model
    //  kernels of NetMw<7, false, 1> changes)
    __shared__ __attribute__((aligned(16))) float S[3 * R * 64 + 256];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    gru_tile_mw_any<R, PROJ, KX>(a, blockIdx.x, wave, threadIdx.x & 63, S);
}
template <int MODE, bool DELTA>
__global__ __launch_bounds__(64) void gru_v_kernel(const GruArgs a) {
    touch_kernel_arguments<(int)sizeof(GruArgs)>();
    NetV<MODE, DELTA>::run(a, blockIdx.x, nullptr);
}
__global__ __launch_bounds__(256) void gru_cw_kernel(const GruArgs a) {
    touch_kernel_arguments<(int)sizeof(GruArgs)>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    NetCw::run(a, blockIdx.x, smem);
}
// the four-wave shape stages the tile's whole ring in LDS and walks at most 32 timesteps of it
static bool cw_four_waves_ok(const GruArgs& a) { return a.ring_slots == kCwSlots && a.n_features <= kCwSlots; }
template <int MODE, bool DELTA, bool RB = false>
__global__ __launch_bounds__(64) void gru_bf16_kernel(const GruArgs a) {
    touch_kernel_arguments<(int)sizeof(GruArgs)>();
    NetBf16<MODE, DELTA, RB>::run(a, blockIdx.x, nullptr);
}
template <int MODE>
__global__ __launch_bounds__(64) void gru_x3_kernel(const GruArgs a) {
    touch_kernel_arguments<(int)sizeof(GruArgs)>();
    NetX3<MODE>::run(a, blockIdx.x, nullptr);
}

// ---- the network for a whole batch of updates (pe_update_many): workgroup b serves update b / n_tiles, tile b % n_tiles ----
// b becomes the arguments of update u of the call: its row of the emitted-frame history, its block of the output
__device__ __forceinline__ void select_update(GruArgs& b, const int u, const int n_padded) {
    b.ke_plain += (size_t)u * n_padded;
    b.out += (size_t)u * b.n_streams;
    b.predict_ke = 0;
}
template <int R, bool PROJ>
__global__ __launch_bounds__(64) void gru_many_kernel(const GruArgs a, const int n_tiles, const int n_padded) {
    GruArgs b = a;
    select_update(b, blockIdx.x / n_tiles, n_padded);
    NetSmall<R, kRing, PROJ, 1>::run(b, blockIdx.x % n_tiles, nullptr);
}
// (four waves sharing each (update, tile) -- few tiles per SIMD: latency matters more than issue slots)
template <int R, bool PROJ>
__global__ __launch_bounds__(256) void gru_many_mw_kernel(const GruArgs a, const int n_tiles, const int n_padded) {
    __shared__ __attribute__((aligned(16))) float S[3 * R * 64 + 256];
    GruArgs b = a;
    select_update(b, blockIdx.x / n_tiles, n_padded);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    gru_tile_mw_any<R, PROJ>(b, blockIdx.x % n_tiles, wave, threadIdx.x & 63, S);       // (written out, as in gru_mw_kernel)
}
template <bool DELTA>
__global__ __launch_bounds__(64) void gru_many_v_kernel(const GruArgs a, const int n_tiles, const int n_padded) {
    GruArgs b = a;
    select_update(b, blockIdx.x / n_tiles, n_padded);
    NetV<kRing, DELTA>::run(b, blockIdx.x % n_tiles, nullptr);
}
__global__ __launch_bounds__(256) void gru_many_cw_kernel(const GruArgs a, const int n_tiles, const int n_padded) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GruArgs b = a;
    select_update(b, blockIdx.x / n_tiles, n_padded);
    NetCw::run(b, blockIdx.x % n_tiles, smem);
}
template <bool DELTA, bool RB>
__global__ __launch_bounds__(64) void gru_many_bf16_kernel(const GruArgs a, const int n_tiles, const int n_padded) {
    // (NetBf16<kRing, DELTA, RB>::run, written out: through the functor this kernel compiles to other code than it did)
    const int tile = blockIdx.x % n_tiles;
    GruArgs b = a;
    select_update(b, blockIdx.x / n_tiles, n_padded);
    if (b.b20) { gru_tile_b20<kRing, DELTA, RB>(b, tile, threadIdx.x); return; }
    gru_tile_bf16<kRing, DELTA, RB>(b, tile, threadIdx.x);
}
__global__ __launch_bounds__(64) void gru_many_x3_kernel(const GruArgs a, const int n_tiles, const int n_padded) {
    GruArgs b = a;
    select_update(b, blockIdx.x / n_tiles, n_padded);
    NetX3<kRing>::run(b, blockIdx.x % n_tiles, nullptr);
}

// ---- the network of a K-model engine (pe_create_models) in ONE launch, any shape: workgroup b runs block b % per_model of
// model b / per_model with that model's weights (ModelSet); model-major outputs, out_stride apart
template <class NET>
__global__ __launch_bounds__(NET::kThreads) void gru_models_kernel(const GruArgs a, const ModelSet ms, const int per_model, const long long out_stride) {
    touch_kernel_arguments<(int)sizeof(GruArgs)>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int mi = __builtin_amdgcn_readfirstlane(blockIdx.x / per_model);
    NET::run(model_args(a, ms.net[mi], mi, out_stride), blockIdx.x - mi * per_model, smem);
}
// pe_update_many: (model, update, tile) per workgroup, outputs [K][n_updates][windows]
template <class NET>
__global__ __launch_bounds__(NET::kThreads) void gru_many_models_kernel(const GruArgs a, const ModelSet ms, const int n_tiles, const int n_updates, const int n_padded) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int per_model = n_tiles * n_updates;
    const int mi = __builtin_amdgcn_readfirstlane(blockIdx.x / per_model);
    const int w = blockIdx.x - mi * per_model;
    const int u = w / n_tiles, tile = w % n_tiles;
    GruArgs b = model_args(a, ms.net[mi], mi, (long long)n_updates * a.n_streams);
    select_update(b, u, n_padded);
    NET::run(b, tile, smem);
}
// what the launchers below take for a K-model engine (ms == null: the one-model kernels)
struct NetModels { const ModelSet* ms; int n; long long out_stride; };
// one network launch of shape NET: its one-model KERNEL over GRID workgroups, or gru_models_kernel<NET> over GRID x K
#define PE_NET(NET, KERNEL, GRID)                                                                                            \
    do {                                                                                                                     \
        using Net_ = PE_UNPAREN NET;                                                                                         \
        if (mm.ms) hipLaunchKernelGGL((gru_models_kernel<Net_>), dim3((GRID) * mm.n), dim3(Net_::kThreads), Net_::kLds, s, a, *mm.ms, (int)(GRID), mm.out_stride); \
        else hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(Net_::kThreads), Net_::kOwnLds, s, a);                              \
    } while (0)
#define PE_NET_MANY(NET, KERNEL, TILES)                                                                                      \
    do {                                                                                                                     \
        using Net_ = PE_UNPAREN NET;                                                                                         \
        if (mm.ms) hipLaunchKernelGGL((gru_many_models_kernel<Net_>), dim3((TILES) * n_updates * mm.n), dim3(Net_::kThreads), Net_::kLds, s, a, *mm.ms, (TILES), n_updates, n_padded); \
        else hipLaunchKernelGGL(KERNEL, dim3((TILES) * n_updates), dim3(Net_::kThreads), Net_::kOwnLds, s, a, (TILES), n_padded); \
    } while (0)

// ---- wide / stacked GRU: one workgroup per 16-stream tile, weights streamed from L2 -------------------
// k-groups of the layer-0 input of a float32 wide launch: 2 with use_delta or 32-float rows, else 1; 0 where the packed
// weight stream (layer[0].kx4) says otherwise
static int wide_input_groups(const WideArgs& a) {
    const int kx = (a.base.use_delta || a.base.row_floats != kRowFloats) ? 2 : 1;
    if (a.base.use_delta && a.base.row_floats != kRowFloats) return 0;
    return a.layer[0].kx4 == kx ? kx : 0;
}
// KX: 16-input k-groups of layer 0 (2: use_delta or 32-float rows, gru_wide_device.h WideInput)
template <int TPW, int MODE, int WAVES, int KX>
__global__ __launch_bounds__(64 * WAVES) void gru_wide_kernel(const WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef PE_WIDE_STAGGER
    for (int i = (blockIdx.x >> 3) & 31; i > 0; --i) __builtin_amdgcn_s_sleep(PE_WIDE_STAGGER);
#endif
    gru_wide_tile<TPW, MODE, WAVES, KX>(a, blockIdx.x, wave, threadIdx.x & 63, reinterpret_cast<float*>(smem));
}

template <int TPW, int WAVES>
static hipError_t launch_wide_t(const WideArgs& a, int mode, hipStream_t s) {
    const int tiles = (a.base.n_streams + kTileStreams - 1) / kTileStreams;
    if (tiles == 0) return hipSuccess;
    const size_t lds = (size_t)4 * (TPW * WAVES) * 256 * sizeof(float);      // 2 layers x {h, r*h}
    const int kx = wide_input_groups(a);
    if (!kx) return hipErrorInvalidValue;
    if (!with_mode(mode, [&](auto M) { with_const<1, 2>(kx, [&](auto K) {
            hipLaunchKernelGGL((gru_wide_kernel<TPW, PE_CONST(M), WAVES, PE_CONST(K)>), dim3(tiles), dim3(64 * WAVES), lds, s, a); }); })) return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- the same network with the float32 products on the bf16 matrix pipe (gru_wide_x3_device.h; pe_set_gru_tiling(e, 2)) ----
#ifndef PE_WIDE_X3_KS
#define PE_WIDE_X3_KS 2         // 2: eight waves per workgroup, the k-groups of every contraction cut in two (widths that are multiples of 128)
#endif
template <int TPW, int MODE, int KS, int KX>
__global__ __launch_bounds__(256 * KS) void gru_wide_x3_kernel(const WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    gru_wide_x3_tile<TPW, MODE, KS, KX>(a, blockIdx.x, wave, threadIdx.x & 63, smem);
}

template <int TPW>
static hipError_t launch_wide_x3_t(const WideArgs& a, int mode, hipStream_t s) {
    const int tiles = (a.base.n_streams + kTileStreams - 1) / kTileStreams;
    if (tiles == 0) return hipSuccess;
    constexpr int KS = (PE_WIDE_X3_KS == 2 && TPW % 2 == 0) ? 2 : 1;
    const size_t lds = wide_x3_lds_bytes<TPW>();          // three state vectors + partial sums / z / float32 state of the lead waves
    const int kx = wide_input_groups(a);
    if (!kx) return hipErrorInvalidValue;
    if (!with_mode(mode, [&](auto M) { with_const<1, 2>(kx, [&](auto K) {
            hipLaunchKernelGGL((gru_wide_x3_kernel<TPW, PE_CONST(M), KS, PE_CONST(K)>), dim3(tiles), dim3(256 * KS), lds, s, a); }); })) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_gru_wide_x3(const WideArgs& a, int mode, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    with_const<1, 2, 3, 4>(a.units / 64, [&](auto T) { err = launch_wide_x3_t<PE_CONST(T)>(a, mode, s); });
    return err;
}

// ---- the same network with bf16 operands (gru_precision = 1; gru_wide_bf16_device.h): four waves per 16-stream tile ----
// (64 / 128 units: registers for four / two workgroups per compute unit -- wide_bf16_phase)
template <int TPW, int MODE>
__global__ __launch_bounds__(256, TPW == 1 ? 4 : TPW == 2 ? 2 : 1) void gru_wide_bf16_kernel(const WideArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[kWideBf16LdsBytes];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    gru_wide_bf16_tile<TPW, MODE>(a, blockIdx.x, wave, threadIdx.x & 63, smem);
}

template <int TPW>
static hipError_t launch_wide_bf16_t(const WideArgs& a, int mode, hipStream_t s) {
    const int tiles = (a.base.n_streams + kTileStreams - 1) / kTileStreams;
    if (tiles == 0) return hipSuccess;
    if (!with_mode(mode, [&](auto M) { hipLaunchKernelGGL((gru_wide_bf16_kernel<TPW, PE_CONST(M)>), dim3(tiles), dim3(256), 0, s, a); })) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_gru_wide_bf16(const WideArgs& a, int mode, hipStream_t s) {
    hipError_t err = hipErrorInvalidValue;
    with_const<1, 2, 3, 4>(a.units / 64, [&](auto T) { err = launch_wide_bf16_t<PE_CONST(T)>(a, mode, s); });
    return err;
}

// 8 waves per workgroup (two per SIMD) for H = 128 / 256 was measured and is NOT faster: 256 x 2 layers, 4096
// streams: 4 waves 1.254 ms per launch, 8 waves 1.325 ms (tools/gpu_wide.py) -- kept as a build switch only.
#ifndef PE_WIDE8
#define PE_WIDE8 0
#endif
int gru_wide_waves(int units) { return (PE_WIDE8 && units % 128 == 0) ? 8 : 4; }

hipError_t launch_gru_wide(const WideArgs& a, int mode, hipStream_t s) {
    switch (a.units / 64) {
        case 1: return launch_wide_t<1, 4>(a, mode, s);
        case 2: return PE_WIDE8 ? launch_wide_t<1, 8>(a, mode, s) : launch_wide_t<2, 4>(a, mode, s);
        case 3: return launch_wide_t<3, 4>(a, mode, s);
        case 4: return PE_WIDE8 ? launch_wide_t<2, 8>(a, mode, s) : launch_wide_t<4, 4>(a, mode, s);
        default: return hipErrorInvalidValue;
    }
}

// Dispatch order of the roles of a fused launch.  Workgroups are handed to the CUs in blockIdx order; `frames_first`
// puts the (few, long-lived, VALU-bound) frame workgroups in front of the (many, MFMA-bound) network workgroups so
// that at large batches the two kinds are resident TOGETHER -- with the network first, its workgroups fill every
// wave slot and the frame role only starts when they drain (the launch then costs the SUM of the two roles).
// Returns the index in the canonical order [network | frames | bookkeeping].
constexpr int kFramesFirst = 1, kBySimd = 2;       // launch flags of fused_update_kernel (its last argument)
constexpr int kCwRoleSlot = 1984;                  // four ints of the GRU workgroup's LDS between the mailboxes and the staged ring
static_assert(CwBox::END <= kCwRoleSlot && kCwRoleSlot + 4 <= CwLds::XR, "role slots overlap");
__device__ __forceinline__ int role_block(const int b, const int n_gru, const int n_frames, const int frames_first) {
    if (!frames_first || b >= n_gru + n_frames) return b;
    return b < n_frames ? n_gru + b : b - n_frames;
}

// ---- fused update: network role(s) || MFCC frame role || bookkeeping role in ONE launch -------------------------------
// Workgroups [0, n_net) run the network on the feature windows as they will stand after this update (they are dispatched
// first: the long pole); the next n_frame_blocks compute this update's MFCC frames, one frame task per wave; the last
// n_tiles move the leftover samples and the counters.
// MODELS (a K-model engine, pe_create_models): n_models network roles beside ONE frame role and ONE bookkeeping role.  The
// network workgroups are the one-model launch's, n_gru_blocks per model, model-major: workgroup b of the network runs block
// b % n_gru_blocks of model b / n_gru_blocks with that model's weights (ModelSet) and writes that model's block of the output.
// The network roles only READ the ring and the records (the frame and bookkeeping roles write rows and record sides no window
// of this launch reads), so K of them are as independent as one.  !MODELS: ms is not read, n_models is 1.
// network_args: the arguments of network workgroup b -- the launch's own, or (K models) a copy with the model's weights and
// its block of the output; b becomes the block within the model.
__device__ __forceinline__ const GruArgs& network_args(std::false_type, const GruArgs& g, const ModelSet*, const int, int&) { return g; }
__device__ __forceinline__ GruArgs network_args(std::true_type, const GruArgs& g, const ModelSet* ms, const int n_gru_blocks, int& b) {
    const int mi = __builtin_amdgcn_readfirstlane(b / n_gru_blocks);
    b -= mi * n_gru_blocks;
    return model_args(g, ms->net[mi], mi, g.n_streams);
}
// (the argument lines the prologue touches: the integers behind GruArgs -- four, and n_models for a K-model launch, whose
//  ModelSet behind them is read once the model is known)
template <class R, bool MODELS>
static constexpr int kFusedArgBytes = (int)(sizeof(MfccStreamArgs<R>) + sizeof(WaveTables<R>) + sizeof(GruArgs) + (MODELS ? 20 : 16));

// bf16 network role: frames_first bits 8.. = network tiles per workgroup, one wave each (1, 2 or 4: with few tiles, one or
// two network waves on EVERY compute unit disturb the frame waves less than four on every second one)
template <class R, class SH, bool DELTA, bool RB, bool MODELS>
__device__ __forceinline__ void fused_update_bf16_body(const MfccStreamArgs<R>& m, const WaveTables<R>& t, const GruArgs& g, const ModelSet* ms,
                                                       const int n_gru_blocks, const int n_models, const int n_frame_blocks, const int n_tiles, const int frames_first) {
    touch_kernel_arguments<kFusedArgBytes<R, MODELS>>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tpw = frames_first >> 8;
    const int n_net = MODELS ? n_gru_blocks * n_models : n_gru_blocks;
    const int b = role_block(blockIdx.x, n_net, n_frame_blocks, frames_first & 1);
    if (b < n_net) {
        int bl = b;
        const GruArgs& gm = network_args(std::integral_constant<bool, MODELS>{}, g, ms, n_gru_blocks, bl);
        const int wave = threadIdx.x >> 6;
        const int tile = bl * tpw + wave;
        if (wave < tpw && tile < n_tiles) {
            if (gm.b20) { gru_tile_b20<kRing, DELTA, RB>(gm, tile, threadIdx.x & 63); return; }
            gru_tile_bf16<kRing, DELTA, RB>(gm, tile, threadIdx.x & 63);
        }
    } else if (b < n_net + n_frame_blocks) {
        mfcc_frame_tasks<R, SH, true>(m, t, smem, (b - n_net) * kFrameWaves, n_frame_blocks * kFrameWaves);
    } else {
        mfcc_book_tile<R>(m, b - n_net - n_frame_blocks);
    }
}

// float32 network role.  MW = true: one network workgroup per tile, its four waves share the tile (gru_tile_mw / gru_tile_cw);
// MW = false: four tiles per network workgroup, one wave each.  CW: stock width, re-tiled (gru_cw_device.h).
template <class R, class SH, int RG, bool MW, bool PROJ, bool CW, bool MODELS>
__device__ __forceinline__ void fused_update_body(const MfccStreamArgs<R>& m, const WaveTables<R>& t, const GruArgs& g, const ModelSet* ms,
                                                  const int n_gru_blocks, const int n_models, const int n_frame_blocks, const int n_tiles, const int frames_first) {
    static_assert(!(MODELS && PROJ), "input projection rows are per model: pe_set_input_projection refuses K > 1");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    touch_kernel_arguments<kFusedArgBytes<R, MODELS>>();
    const int n_net = MODELS ? n_gru_blocks * n_models : n_gru_blocks;
    const int b = role_block(blockIdx.x, n_net, n_frame_blocks, frames_first & kFramesFirst);
    if (b < n_net) {
        int bl = b;
        const GruArgs& gm = network_args(std::integral_constant<bool, MODELS>{}, g, ms, n_gru_blocks, bl);
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#if defined(PE_PRIO_R)
        if (wave == 0) __builtin_amdgcn_s_setprio(PE_PRIO_R); else __builtin_amdgcn_s_setprio(PE_PRIO_H);
#else
        __builtin_amdgcn_s_setprio(3);          // the network role is the long pole: it wins every issue arbitration
#endif
        if constexpr (CW) {
            static_assert(RG == 5 && !PROJ, "the re-tiled shapes exist for the stock width, without projection rows");
            if (MW) {
                // kBySimd: the four roles sit on SIMDs 0..3 in a fixed order (R on 0, Z1, Z2, P) so that the frame waves of
                // this compute unit know what runs beside them (mfcc_frame_tasks(..., by_simd)).  Roles follow the SIMDs only
                // if the four waves sit on four different ones (they do: a workgroup's waves are spread round-robin;
                // checked, not assumed).
                int role = wave;
                if (frames_first & kBySimd) {
                    int* const slot = reinterpret_cast<int*>(smem) + kCwRoleSlot;
                    const int simd = wave_simd_id();
                    if ((threadIdx.x & 63) == 0) slot[wave] = simd;
                    __syncthreads();
                    if (((1 << slot[0]) | (1 << slot[1]) | (1 << slot[2]) | (1 << slot[3])) == 15) role = simd;
                }
                gru_tile_cw<false>(gm, bl, role, threadIdx.x & 63, reinterpret_cast<float*>(smem));
            } else {
                const int tile = bl * 4 + wave;       // (use_delta on this shape: two launches, engine.hip can_fuse; K models: four waves)
                if (tile < n_tiles) gru_tile_v<kRing, false>(gm, tile, threadIdx.x & 63);
            }
        } else if (MW) {
            gru_tile_mw_any<RG, PROJ>(gm, bl, wave, threadIdx.x & 63, reinterpret_cast<float*>(smem));
        } else {
            const int tile = bl * 4 + wave;
            if (tile < n_tiles) gru_tile<RG, kRing, PROJ>(gm, tile, threadIdx.x & 63);
        }
    } else if (b < n_net + n_frame_blocks) {
        mfcc_frame_tasks<R, SH, true, !PROJ>(m, t, smem, (b - n_net) * kFrameWaves, n_frame_blocks * kFrameWaves, CW && MW && (frames_first & kBySimd));
    } else {
        mfcc_book_tile<R>(m, b - n_net - n_frame_blocks);
    }
}

// The entry points: thin wrappers.  (R = float: the float32 network role inside loses its packed gate arithmetic too -- 16.2 vs
// 15.7 us per fused update at 4096 streams for the float32 front end + float32 network, which is no BASELINE configuration;
// the headline kernel is R = double.)  K models: the integers first -- they sit in the argument lines the prologue touches.
#define PE_FUSED_PARAMS (const MfccStreamArgs<R> m, const WaveTables<R> t, const GruArgs g, const int n_gru_blocks, const int n_frame_blocks, const int n_tiles, const int frames_first)
#define PE_FUSED_MODELS_PARAMS (const MfccStreamArgs<R> m, const WaveTables<R> t, const GruArgs g, const int n_gru_blocks, const int n_models, const int n_frame_blocks, \
                                const int n_tiles, const int frames_first, const ModelSet ms)
PE_KERNEL_PAIR((template <class R, class SH, bool DELTA, bool RB>), PE_FRAME_KERNEL(256, PE_FRAME_WPE), fused_update_bf16_kernel, PE_FUSED_PARAMS,
               { fused_update_bf16_body<R, SH, DELTA, RB, false>(m, t, g, nullptr, n_gru_blocks, 1, n_frame_blocks, n_tiles, frames_first); })
PE_KERNEL_PAIR((template <class R, class SH, bool DELTA, bool RB>), PE_FRAME_KERNEL(256, PE_FRAME_WPE), fused_update_bf16_models_kernel, PE_FUSED_MODELS_PARAMS,
               { fused_update_bf16_body<R, SH, DELTA, RB, true>(m, t, g, &ms, n_gru_blocks, n_models, n_frame_blocks, n_tiles, frames_first); })
PE_KERNEL_PAIR((template <class R, class SH, int RG, bool MW, bool PROJ, bool CW = false>), PE_FRAME_KERNEL(256, PE_FRAME_WPE), fused_update_kernel, PE_FUSED_PARAMS,
               { fused_update_body<R, SH, RG, MW, PROJ, CW, false>(m, t, g, nullptr, n_gru_blocks, 1, n_frame_blocks, n_tiles, frames_first); })
PE_KERNEL_PAIR((template <class R, class SH, int RG, bool MW, bool CW>), PE_FRAME_KERNEL(256, PE_FRAME_WPE), fused_update_models_kernel, PE_FUSED_MODELS_PARAMS,
               { fused_update_body<R, SH, RG, MW, false, CW, true>(m, t, g, &ms, n_gru_blocks, n_models, n_frame_blocks, n_tiles, frames_first); })

// ---- chain launch (gru_chain_device.h): the fused update of form 1 with the window chains CARRIED between updates -----
// The same three roles in the same order; the network role advances the tile's resident chains by the rows this update makes
// visible (four waves; the new rows' projections pass through the workgroup's LDS, one barrier: ChainLds) instead of running
// every window again from h = 0.
template <class R, class SH, int NW>
__device__ __forceinline__ void fused_update_chains_body(const MfccStreamArgs<R>& m, const WaveTables<R>& t, const GruArgs& g, const ChainArgs& ch,
                                                         const int n_gru_blocks, const int n_frame_blocks, const int frames_first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    touch_kernel_arguments<kFusedArgBytes<R, false> + (int)sizeof(ChainArgs)>();
    const int b = role_block(blockIdx.x, n_gru_blocks, n_frame_blocks, frames_first & kFramesFirst);
    if (b < n_gru_blocks) {
        // (no s_setprio here: this role is the SHORT one -- see the frame role below)
        constexpr int per_tile = NW / 4;                // network workgroups per tile
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) + 4 * (b % per_tile);
        gru_tile_chains<NW>(g, ch, b / per_tile, wave, threadIdx.x & 63, reinterpret_cast<float*>(smem));
    } else if (b < n_gru_blocks + n_frame_blocks) {
        // The frame role is the long pole of this launch, and an f32-input MFMA keeps its SIMD from issuing while it runs
        // (DESIGN 4.6): the chain waves' matrix time ADDS to the frame waves' on every SIMD.  With the frame waves winning every
        // issue arbitration the chain waves' MFMAs go into the cycles in which no frame wave has an instruction ready.  The
        // chains load all four SIMDs alike, so the frame waves split their slots evenly (no by-SIMD split).  Measured at 4096
        // streams (profiles/chain_carry/README.md): 14.14 us per update against 15.02 with the plain launch's shape.
        __builtin_amdgcn_s_setprio(3);
        mfcc_frame_tasks<R, SH, true, true>(m, t, smem, (b - n_gru_blocks) * kFrameWaves, n_frame_blocks * kFrameWaves, false);
    } else {
        mfcc_book_tile<R>(m, b - n_gru_blocks - n_frame_blocks);
    }
}
PE_KERNEL_PAIR((template <class R, class SH, int NW>), PE_FRAME_KERNEL(256, PE_FRAME_WPE), fused_update_chains_kernel,
               (const MfccStreamArgs<R> m, const WaveTables<R> t, const GruArgs g, const int n_gru_blocks, const int n_frame_blocks, const int n_tiles,
                const int frames_first, const ChainArgs ch),
               { (void)n_tiles; fused_update_chains_body<R, SH, NW>(m, t, g, ch, n_gru_blocks, n_frame_blocks, frames_first); })
// entering chain mode: every live chain of every stream from the ring as it stands (once per entry: a throughput kernel)
__global__ __launch_bounds__(256) void gru_chains_rebuild_kernel(const GruArgs a, const ChainArgs ch) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    gru_tile_chains_rebuild(a, ch, blockIdx.x, wave, threadIdx.x & 63);
}


// Workgroups of the frame role: one wave per task while that fits the machine (4 workgroups of 4 waves per compute
// unit are resident: LDS and a 128-register budget), more tasks per wave beyond.
static int frame_blocks(long long n_tasks, int n_cus, int per_cu = 4) {      // per_cu: resident frame workgroups per compute unit
    const long long need = (n_tasks + kFrameWaves - 1) / kFrameWaves;
    const long long cap = (long long)n_cus * per_cu;
    return (int)(need < cap ? (need < 1 ? 1 : need) : cap);
}

// frame workgroups of a streaming launch: every wave owns a contiguous run of (stream, row parity) slots
// (mfcc_frame_tasks), as many waves as the resident cap allows, the runs as even as they can be
static int stream_frame_blocks(int n_streams, int n_cus, int per_cu_default = 4) {
    const long long slots = 2LL * n_streams;
    const long long cap_waves = (long long)frame_blocks(slots, n_cus, per_cu_default) * kFrameWaves;
    const long long per_wave = (slots + cap_waves - 1) / cap_waves;
    const long long waves = (slots + per_wave - 1) / per_wave;
    return (int)((waves + kFrameWaves - 1) / kFrameWaves);
}

template <class R>
static size_t frame_lds(const WaveTables<R>& t) { return wave_lds_bytes(sizeof(R), t.L, kFrameWaves); }
// the kernels address the table image with the compile-time section offsets of their shape (mfcc_wave_device.h: wave_bind)
template <class R>
static bool blob_matches_shape(const WaveTables<R>& t) {
    return t.L.mel_pad == ShapeStock::MEL ? shape_layout_matches<R, ShapeStock>(t.L) : shape_layout_matches<R, ShapeAny>(t.L);
}

// The table shape of a stock-family launch (ShapeStock / ShapeAny, by the blob's mel padding) and MELS (mel rows) as template
// arguments: f(SH{}, MELS).  All four launchers of the family go through it: a (shape, rows) pair is spelled nowhere else.
template <class R, class F>
static void with_frame_shape(const WaveTables<R>& t, bool mels, F&& f) {
    with_flag(t.L.mel_pad == ShapeStock::MEL, [&](auto ST) { with_flag(mels, [&](auto ME) {
        f(std::conditional_t<PE_CONST(ST) != 0, ShapeStock, ShapeAny>{}, ME); }); });
}

// The four kinds of launch of the stock family: each ONE template over the precision R, declared in pe_common.h and instantiated
// for double and float at the end of the front-end launchers (PE_FRONT_END_LAUNCHERS); engine.hip chooses R once (with_real).
template <class R>
hipError_t launch_mfcc(const MfccStreamArgs<R>& a, const WaveTables<R>& t, int n_cus, hipStream_t s, bool mels) {
    const int tiles = (a.geo.n_streams + kTileStreams - 1) / kTileStreams;
    const int fb = stream_frame_blocks(a.geo.n_streams, n_cus);
    if (!blob_matches_shape(t)) return hipErrorInvalidValue;
    const bool single = a.n_updates == 1 && !a.proj_ring;
    const dim3 grid(fb + tiles), block(64 * kFrameWaves);
    with_frame_shape(t, mels, [&](auto SH, auto ME) { with_flag(single, [&](auto SI) {
        PE_LAUNCH_R(R, mfcc_kernel, (decltype(SH), PE_CONST(SI) != 0, PE_CONST(ME) != 0), grid, block, frame_lds(t), s, a, t, fb); }); });
    return hipGetLastError();
}

template <class R>
hipError_t launch_mfcc_offline(const MfccOfflineArgs<R>& a, const WaveTables<R>& t, int n_cus, hipStream_t s, bool mels) {
    if (a.n_frames <= 0) return hipSuccess;
    if (!blob_matches_shape(t)) return hipErrorInvalidValue;
    const dim3 grid(frame_blocks(a.n_frames, n_cus)), block(64 * kFrameWaves);
    with_frame_shape(t, mels, [&](auto SH, auto ME) {
        PE_LAUNCH_R(R, mfcc_offline_kernel, (decltype(SH), PE_CONST(ME) != 0), grid, block, frame_lds(t), s, a, t); });
    return hipGetLastError();
}

template <class R>
hipError_t launch_mfcc_clips(const MfccClipArgs<R>& a, const WaveTables<R>& t, int n_cus, hipStream_t s, bool mels) {
    if (a.clips.n_clips <= 0) return hipSuccess;
    if (!blob_matches_shape(t)) return hipErrorInvalidValue;
    // (a launch without frame tasks still stores the pad rows: one workgroup at least)
    const long long work = a.clips.n_tasks > (uint32_t)a.clips.n_clips ? (long long)a.clips.n_tasks : (long long)a.clips.n_clips;
    const dim3 grid(frame_blocks(work, n_cus)), block(64 * kFrameWaves);
    with_frame_shape(t, mels, [&](auto SH, auto ME) {
        PE_LAUNCH_R(R, mfcc_clips_kernel, (decltype(SH), PE_CONST(ME) != 0), grid, block, frame_lds(t), s, a, t); });
    return hipGetLastError();
}

template <class R>
hipError_t launch_mfcc_recs(const MfccRecArgs<R>& a, const WaveTables<R>& t, int n_cus, hipStream_t s, bool mels) {
    if (a.recs.n_tasks == 0) return hipSuccess;
    if (!blob_matches_shape(t)) return hipErrorInvalidValue;
    const dim3 grid(frame_blocks((long long)a.recs.n_tasks, n_cus)), block(64 * kFrameWaves);
    with_frame_shape(t, mels, [&](auto SH, auto ME) {
        PE_LAUNCH_R(R, mfcc_recs_kernel, (decltype(SH), PE_CONST(ME) != 0), grid, block, frame_lds(t), s, a, t); });
    return hipGetLastError();
}

int gru_small_regs(int units) { return (units + 3) / 4; }
int gru_small_tiles(int units) { return (3 * gru_small_regs(units) + 3) / 4; }

template <int R>
static hipError_t launch_r(const GruArgs& a, int mode, hipStream_t s, const NetModels& mm) {
    if (mm.ms && a.proj_ring) return hipErrorInvalidValue;        // (input projection rows are per model: refused for K > 1)
    const int tiles = (a.n_streams + kTileStreams - 1) / kTileStreams;
    if (tiles == 0) return hipSuccess;
    bool ok = true;
    if (a.row_floats == 2 * kRowFloats) {           // 17..32 coefficients per frame: 32-float rows
        // (stock width, few tiles: four waves per tile, as the 16-float rows get.  K models: the one-wave twin -- the same form,
        //  the same bits; a second caller of gru_tile_mw_any<5, false, 2> changes the code generated for gru_mw_kernel<5, false, 2>)
        if constexpr (R == 5) {
            if (mode == kRing && a.waves_per_tile == 4 && !mm.ms) {
                hipLaunchKernelGGL((gru_mw_kernel<R, false, 2>), dim3(tiles), dim3(256), 0, s, a);
                return hipGetLastError();
            }
        }
        ok = with_mode(mode, [&](auto M) { PE_NET((NetSmall<R, PE_CONST(M), false, 2>), (gru_small_kernel<R, PE_CONST(M), false, 2>), tiles); });
        return ok ? hipGetLastError() : hipErrorInvalidValue;
    }
    if constexpr (R == 5) {
        if (a.cw) {
            if (mode == kRing && a.waves_per_tile == 4 && cw_four_waves_ok(a)) PE_NET((NetCw), gru_cw_kernel, tiles);
            else ok = with_mode(mode, [&](auto M) { with_flag(a.use_delta, [&](auto D) {
                PE_NET((NetV<PE_CONST(M), PE_CONST(D)>), (gru_v_kernel<PE_CONST(M), PE_CONST(D)>), tiles); }); });
            return ok ? hipGetLastError() : hipErrorInvalidValue;
        }
        if (mode == kRing && a.proj_ring) {
            if (a.waves_per_tile == 4) hipLaunchKernelGGL((gru_mw_kernel<R, true>), dim3(tiles), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((gru_small_kernel<R, kRing, true>), dim3(tiles), dim3(64), 0, s, a);
            return hipGetLastError();
        }
    }
    if (mode == kRing && a.waves_per_tile == 4) PE_NET((NetMw<R, false, 1>), (gru_mw_kernel<R>), tiles);
    else ok = with_mode(mode, [&](auto M) { PE_NET((NetSmall<R, PE_CONST(M), false, 1>), (gru_small_kernel<R, PE_CONST(M)>), tiles); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_gru_small(const GruArgs& a, int mode, hipStream_t s, const ModelSet* ms, int n_models, long long out_stride) {
    const NetModels mm{ms, n_models, out_stride};
    if (ms && (n_models < 1 || n_models > kMaxModels)) return hipErrorInvalidValue;
    if (a.x3 || a.bf16) {
        const int tiles = (a.n_streams + kTileStreams - 1) / kTileStreams;
        if (tiles == 0) return hipSuccess;
        bool ok = true;
        if (a.x3) ok = with_mode(mode, [&](auto M) { PE_NET((NetX3<PE_CONST(M)>), gru_x3_kernel<PE_CONST(M)>, tiles); });
        else with_flag(a.use_delta, [&](auto D) {          // (bf16 rows: read from the ring only)
            if (mode == kRing && a.ring_bf16) PE_NET((NetBf16<kRing, PE_CONST(D), true>), (gru_bf16_kernel<kRing, PE_CONST(D), true>), tiles);
            else ok = with_mode(mode, [&](auto M) { PE_NET((NetBf16<PE_CONST(M), PE_CONST(D), false>), (gru_bf16_kernel<PE_CONST(M), PE_CONST(D)>), tiles); });
        });
        return ok ? hipGetLastError() : hipErrorInvalidValue;
    }
    hipError_t err = hipErrorInvalidValue;
    with_const<1, 2, 3, 4, 5, 6, 7, 8>(gru_small_regs(a.units), [&](auto R) { err = launch_r<PE_CONST(R)>(a, mode, s, mm); });
    return err;
}

template <int R>
static hipError_t launch_many_r(const GruArgs& a, int n_updates, int n_padded, hipStream_t s, const NetModels& mm) {
    if (mm.ms && a.proj_ring) return hipErrorInvalidValue;
    const int tiles = (a.n_streams + kTileStreams - 1) / kTileStreams;
    // up to ~1.5 windows per SIMD the four-wave kernel wins (4096 streams x 4 updates: 18.1 vs 20.1 us per
    // update), from 2 per SIMD on the one-wave kernel does (x 16: 12.5 vs 14.0)
    const bool few = (long long)tiles * n_updates <= 1536;
    const bool mw = few && !a.use_delta;       // (classic tiling: the delta inputs are on the one-wave kernel only)
    if constexpr (R == 5) {
        if (a.cw) {
            if (few && cw_four_waves_ok(a)) PE_NET_MANY((NetCw), gru_many_cw_kernel, tiles);
            else with_flag(a.use_delta, [&](auto D) { PE_NET_MANY((NetV<kRing, PE_CONST(D)>), gru_many_v_kernel<PE_CONST(D)>, tiles); });
            return hipGetLastError();
        }
        if (a.proj_ring) {
            if (mw) hipLaunchKernelGGL((gru_many_mw_kernel<R, true>), dim3(tiles * n_updates), dim3(256), 0, s, a, tiles, n_padded);
            else hipLaunchKernelGGL((gru_many_kernel<R, true>), dim3(tiles * n_updates), dim3(64), 0, s, a, tiles, n_padded);
            return hipGetLastError();
        }
    }
    if (mw) PE_NET_MANY((NetMw<R, false, 1>), (gru_many_mw_kernel<R, false>), tiles);
    else PE_NET_MANY((NetSmall<R, kRing, false, 1>), (gru_many_kernel<R, false>), tiles);
    return hipGetLastError();
}

hipError_t launch_gru_many(const GruArgs& a, int n_updates, int n_padded, hipStream_t s, const ModelSet* ms, int n_models) {
    const NetModels mm{ms, n_models, 0};
    if (ms && (n_models < 1 || n_models > kMaxModels)) return hipErrorInvalidValue;
    const int tiles = (a.n_streams + kTileStreams - 1) / kTileStreams;
    if (tiles == 0 || n_updates == 0) return hipSuccess;
    if (a.x3) {
        PE_NET_MANY((NetX3<kRing>), gru_many_x3_kernel, tiles);
        return hipGetLastError();
    }
    if (a.bf16) {
        with_flag(a.use_delta, [&](auto D) { with_flag(a.ring_bf16, [&](auto RB) {
            PE_NET_MANY((NetBf16<kRing, PE_CONST(D), PE_CONST(RB)>), (gru_many_bf16_kernel<PE_CONST(D), PE_CONST(RB)>), tiles); }); });
        return hipGetLastError();
    }
    hipError_t err = hipErrorInvalidValue;
    with_const<1, 2, 3, 4, 5, 6, 7, 8>(gru_small_regs(a.units), [&](auto R) { err = launch_many_r<PE_CONST(R)>(a, n_updates, n_padded, s, mm); });
    return err;
}

// The network shape of the K-model fused launch (stock width, form 1), from (K, tiles).  The four-wave workgroup of one tile
// holds 40 KB of LDS (mailboxes + the staged ring), and a launch gives every workgroup the same amount: once more than two of
// them per compute unit are due, the frame role no longer finds room beside them, and the LDS-free one-wave shape (gru_tile_v,
// the same form: the same bits) wins.  Measured at 4096 / 8192 streams, K = 2 / 4 / 8 (running the models of a tile
// one after the other in fewer workgroups was measured too and never won).
static bool fused_models_four_waves(int n_models, int tiles, int n_cus) { return (long long)n_models * tiles <= 2LL * n_cus; }

// what a fused launch is made of once its network shape is known: GB network workgroups per model, then fb frame workgroups,
// then one bookkeeping workgroup per tile; ms != null: the K-model entry point, the same shape with n_models network roles
struct FusedLaunch { const ModelSet* ms; int n_models, fb, tiles; hipStream_t s; };
#define PE_FUSED(KERNEL, MODELS_KERNEL, TARGS, MODELS_TARGS, GB, LDS, FF)                                                    \
    do {                                                                                                                     \
        if (f.ms) PE_LAUNCH_R(R, MODELS_KERNEL, MODELS_TARGS, dim3((GB) * f.n_models + f.fb + f.tiles), dim3(256), LDS, f.s, m, t, g, GB, f.n_models, f.fb, f.tiles, FF, *f.ms); \
        else PE_LAUNCH_R(R, KERNEL, TARGS, dim3((GB) + f.fb + f.tiles), dim3(256), LDS, f.s, m, t, g, GB, f.fb, f.tiles, FF); \
    } while (0)
// float32 network role <MW, PROJ, CW> of RG registers per gate
#define PE_FUSED_F32(MW, PROJ, CW, GB, LDS, FF) \
    PE_FUSED(fused_update_kernel, fused_update_models_kernel, (ShapeStock, RG, MW, PROJ, CW), (ShapeStock, RG, MW, CW), GB, LDS, FF)

template <class R, int RG>
static hipError_t launch_fused_rg(const MfccStreamArgs<R>& m, const WaveTables<R>& t, const GruArgs& g, int n_cus, hipStream_t s,
                                  const ModelSet* ms, int n_models) {
    if (ms && g.proj_ring) return hipErrorInvalidValue;       // (input projection rows are per model: refused for K > 1)
    const int tiles = (m.geo.n_streams + kTileStreams - 1) / kTileStreams;
    const size_t lds = frame_lds(t);
    // more network workgroups than the machine holds at once: frames first, three frame workgroups per CU, the network
    // streams through the remaining wave slots (measured at 16384 / 65536 streams, bf16 network + float32 front end:
    // 31.8 / 103.8 us against 35.5 / 109.0 us network-first; the float64 front end gains nothing either way -- its
    // FP64 multiply-adds and the MFMAs do not overlap on a SIMD)
    // one network tile per compute unit on the critical-wave kernel: roles by SIMD, frame slots split by SIMD load
    const bool by_simd = g.cw && g.waves_per_tile == 4 && cw_four_waves_ok(g) && tiles <= n_cus;
    const int frames_first = ((g.waves_per_tile != 4 && tiles >= 4 * n_cus) ? 1 : 0) | (by_simd ? kBySimd : 0);
    // resident frame workgroups per compute unit: at one network tile per compute unit the launch lasts as long as the
    // network's dependent chain, and two frame workgroups (two streams per wave, the second one's samples prefetched)
    // disturb that chain less than four (measured, 4096 streams: 20.6 vs 20.9 us in phase, 21.1 vs 22.5 us with
    // desynchronised streams); larger batches want every wave slot
    const int fb = stream_frame_blocks(m.geo.n_streams, n_cus, tiles <= n_cus ? 2 : (frames_first & kFramesFirst) ? 3 : 4);
    const FusedLaunch f{ms, n_models, fb, tiles, s};
    const int one_per_tile = tiles, four_per_block = (tiles + 3) / 4;       // network workgroups: four waves per tile / one wave per tile
    if constexpr (RG == 5) {
        if (g.cw) {
            // stock width, re-tiled: the four-wave shape wants its LDS (mailboxes + staged ring).  K models: while it wins
            // (fused_models_four_waves), and always with use_delta -- the one-wave fused shape (gru_tile_v, same form, same bits,
            // no LDS of its own) has no delta inputs, as for one model (engine.hip can_fuse)
            const bool four = g.waves_per_tile == 4 && cw_four_waves_ok(g) && (!ms || g.use_delta || fused_models_four_waves(n_models, tiles, n_cus));
            if (four) PE_FUSED_F32(true, false, true, one_per_tile, lds > kCwLdsBytes ? lds : kCwLdsBytes, frames_first);
            else PE_FUSED_F32(false, false, true, four_per_block, lds, frames_first & ~kBySimd);
            return hipGetLastError();
        }
        if (g.proj_ring) {                   // (projection rows exist for the stock width only, and for one model)
            if (g.waves_per_tile == 4) PE_LAUNCH_R(R, fused_update_kernel, (ShapeStock, RG, true, true), dim3(one_per_tile + fb + tiles), dim3(256), lds, s, m, t, g, one_per_tile, fb, tiles, frames_first);
            else PE_LAUNCH_R(R, fused_update_kernel, (ShapeStock, RG, false, true), dim3(four_per_block + fb + tiles), dim3(256), lds, s, m, t, g, four_per_block, fb, tiles, frames_first);
            return hipGetLastError();
        }
    }
    if (g.waves_per_tile == 4) PE_FUSED_F32(true, false, false, one_per_tile, lds, frames_first);
    else if constexpr (RG <= 5) PE_FUSED_F32(false, false, false, four_per_block, lds, frames_first);
    else return hipErrorInvalidValue;        // (21..32 units on the one-wave kernel: engine.hip takes two launches, can_fuse)
    return hipGetLastError();
}

// (the fused kernels are built for the stock table shape only: engine.hip falls back to two launches otherwise)
template <class R>
static hipError_t launch_fused_t(const MfccStreamArgs<R>& m, const WaveTables<R>& t, const GruArgs& g, int n_cus, hipStream_t s,
                                 const ModelSet* ms, int n_models) {
    if (ms && (n_models < 1 || n_models > kMaxModels)) return hipErrorInvalidValue;
    if (t.L.mel_pad != ShapeStock::MEL || !blob_matches_shape(t)) return hipErrorInvalidValue;
    if (g.bf16) {
        const int tiles = (m.geo.n_streams + kTileStreams - 1) / kTileStreams;
        const int tpw = 4;                     // network tiles per network workgroup
        const int gru_blocks = (tiles + tpw - 1) / tpw;
        const int ff = tiles >= 4 * n_cus ? 1 : 0;
        const int frames_first = (ff & 1) | (tpw << 8);
        const FusedLaunch f{ms, n_models, stream_frame_blocks(m.geo.n_streams, n_cus, ff ? 3 : 4), tiles, s};
        with_flag(g.use_delta, [&](auto D) { with_flag(g.ring_bf16, [&](auto RB) {
            PE_FUSED(fused_update_bf16_kernel, fused_update_bf16_models_kernel, (ShapeStock, PE_CONST(D), PE_CONST(RB)), (ShapeStock, PE_CONST(D), PE_CONST(RB)),
                     gru_blocks, frame_lds(t), frames_first); }); });
        return hipGetLastError();
    }
    hipError_t err = hipErrorInvalidValue;
    with_const<1, 2, 3, 4, 5, 6, 7, 8>(gru_small_regs(g.units), [&](auto RG) { err = launch_fused_rg<R, PE_CONST(RG)>(m, t, g, n_cus, s, ms, n_models); });
    return err;
}

hipError_t launch_fused(const MfccStreamArgs<double>& m, const WaveTables<double>& t, const GruArgs& g, int n_cus, hipStream_t s, const ModelSet* ms, int n_models) {
    return launch_fused_t<double>(m, t, g, n_cus, s, ms, n_models);
}
hipError_t launch_fused(const MfccStreamArgs<float>& m, const WaveTables<float>& t, const GruArgs& g, int n_cus, hipStream_t s, const ModelSet* ms, int n_models) {
    return launch_fused_t<float>(m, t, g, n_cus, s, ms, n_models);
}

// The chain launch of engine.hip do_update (chain_eligible: stock float32 network re-tiled, four waves per tile, one model): one
// network workgroup per tile, two for sparse subset calls (gru_tile_chains<NW>); their mailbox (ChainLds, 8 KB) is the start of
// the dynamic LDS the launch asks for on the frame role's behalf; two resident frame workgroups per compute unit at one tile
// per compute unit, four above, as in launch_fused_rg's four-wave branch.
template <class R>
static hipError_t launch_fused_chains_t(const MfccStreamArgs<R>& m, const WaveTables<R>& t, const GruArgs& g, const ChainArgs& ch, int n_cus, hipStream_t s) {
    if (t.L.mel_pad != ShapeStock::MEL || !blob_matches_shape(t)) return hipErrorInvalidValue;
    if (!g.cw || g.waves_per_tile != 4 || !cw_four_waves_ok(g) || !g.predict_ke || g.ke_plain || !ch.chains || !ch.chain_ke) return hipErrorInvalidValue;
    const int tiles = (m.geo.n_streams + kTileStreams - 1) / kTileStreams;
    if (tiles == 0) return hipSuccess;
    const int fb = stream_frame_blocks(m.geo.n_streams, n_cus, tiles <= n_cus ? 2 : 4);
    // a subset call of at most half of the engine's streams: the network role is the long pole, eight waves share a tile's chains
    const bool sparse = g.ids && 2u * (uint32_t)tiles * kTileStreams <= g.n_padded;
    // the chain workgroups' mailbox (ChainLds) sits at the start of the dynamic LDS every workgroup of the launch is given
    const size_t lds = frame_lds(t);
    if (lds < kChainLdsBytes) return hipErrorInvalidValue;
    if (sparse) PE_LAUNCH_R(R, fused_update_chains_kernel, (ShapeStock, 8), dim3(2 * tiles + fb + tiles), dim3(256), lds, s, m, t, g, 2 * tiles, fb, tiles, 0, ch);
    else PE_LAUNCH_R(R, fused_update_chains_kernel, (ShapeStock, 4), dim3(tiles + fb + tiles), dim3(256), lds, s, m, t, g, tiles, fb, tiles, 0, ch);
    return hipGetLastError();
}
hipError_t launch_fused_chains(const MfccStreamArgs<double>& m, const WaveTables<double>& t, const GruArgs& g, const ChainArgs& ch, int n_cus, hipStream_t s) {
    return launch_fused_chains_t<double>(m, t, g, ch, n_cus, s);
}
hipError_t launch_fused_chains(const MfccStreamArgs<float>& m, const WaveTables<float>& t, const GruArgs& g, const ChainArgs& ch, int n_cus, hipStream_t s) {
    return launch_fused_chains_t<float>(m, t, g, ch, n_cus, s);
}
// a: the engine's network arguments over ALL its streams (no ids, predict_ke = 0: the records as they stand)
hipError_t launch_chains_rebuild(const GruArgs& a, const ChainArgs& ch, int n_padded, hipStream_t s) {
    if (!a.cw || !cw_four_waves_ok(a) || a.ids || a.predict_ke || !ch.chains || !ch.chain_ke) return hipErrorInvalidValue;
    if (n_padded == 0) return hipSuccess;
    hipLaunchKernelGGL(gru_chains_rebuild_kernel, dim3(n_padded / kTileStreams), dim3(256), 0, s, a, ch);
    return hipGetLastError();
}

// ---- general front end (mfcc_general_device.h): one wave per stream / per frame -------------------------------------
// (<= 128 registers: four waves per SIMD -- a wave walks the LDS round trips of one frame at a time, the others hide them;
//  BITS = log2(n_fft / 2): the per-lane loops of a frame are unrolled for the transform length)
// (n_fft = 2048: 25 KB of LDS per wave in float64 leave six waves per compute unit anyway: no register cap there)
// float32 butterflies without packed float32 here too (round 6, advisor r5): the general front end may run beside the
// five-values bf16 network of ANOTHER engine on the same compute unit, the combination whose stock-shape twin went wrong
// with packed instructions (see PE_NO_PK_F32 above); tests/test_gpu_parity.py soaks it
#ifndef PE_GEN_TWO_WAVES
#define PE_GEN_TWO_WAVES 0      // two waves per stream (one per frame-row parity): measured SLOWER (62.6 vs 47.7 us per update at 4096 streams:
                                // the launch is bound by rounds of resident waves, and this doubles the waves)
#endif
#define PE_GENERAL_KERNEL (__launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BITS >= 10 ? 2 : 4))))
PE_KERNEL_PAIR((template <class R, int BITS, bool BLUE = false, bool MELS = false>), PE_GENERAL_KERNEL, mfcc_general_stream_kernel,
               (const GeneralStreamArgs<R> a),
               { extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
                 const int s = PE_GEN_TWO_WAVES ? blockIdx.x >> 1 : blockIdx.x;
                 if (s < a.geo.n_streams) general_stream<R, BITS, BLUE, MELS>(a, reinterpret_cast<R*>(smem), s, PE_GEN_TWO_WAVES ? blockIdx.x & 1 : 0, threadIdx.x, PE_GEN_TWO_WAVES ? 2 : 1); })
PE_KERNEL_PAIR((template <class R, int BITS, bool BLUE = false, bool MELS = false>), PE_GENERAL_KERNEL, mfcc_general_offline_kernel,
               (const GeneralOfflineArgs<R> a),
               { extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; general_offline<R, BITS, BLUE, MELS>(a, reinterpret_cast<R*>(smem), blockIdx.x, gridDim.x, threadIdx.x); })
PE_KERNEL_PAIR((template <class R, int BITS, bool BLUE = false, bool MELS = false>), PE_GENERAL_KERNEL, mfcc_general_clips_kernel,
               (const GeneralClipArgs<R> a),
               { extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; general_clips<R, BITS, BLUE, MELS>(a, reinterpret_cast<R*>(smem), (int)blockIdx.x, (int)gridDim.x, threadIdx.x); })
PE_KERNEL_PAIR((template <class R, int BITS, bool BLUE = false, bool MELS = false>), PE_GENERAL_KERNEL, mfcc_general_recs_kernel,
               (const GeneralRecArgs<R> a),
               { extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; general_recs<R, BITS, BLUE, MELS>(a, reinterpret_cast<R*>(smem), (int)blockIdx.x, (int)gridDim.x, threadIdx.x); })
// the transform length as a template argument, f(BITS, BLUE, MELS): n_fft not a power of two (chirp) = Bluestein over
// L = 2^log2m points (BLUE), each with its own list of lengths; MELS (mel rows, Vectorizer.mels) is one more constant beside them
template <class F>
static bool with_general_bits(const GeneralTables& tab, bool mels, F&& f) {
    bool ok = false;
    with_flag(mels, [&](auto MELS) {
        ok = tab.chirp ? with_const<7, 8, 9, 10, 11>(tab.log2m, [&](auto B) { f(B, std::true_type{}, MELS); })
                       : with_const<5, 6, 7, 8, 9, 10>(tab.log2m, [&](auto B) { f(B, std::false_type{}, MELS); }); });
    return ok;
}
// workgroups of a launch that walks `work` tasks (frames, clips, recordings): one wave each, sixteen per compute unit at most
static unsigned general_blocks(long long work, int n_cus) {
    const long long cap = (long long)n_cus * 16;
    return (unsigned)(work < cap ? work : cap);
}
template <class ARGS>
static size_t general_lds(const ARGS& a, size_t real_bytes) { return general_lds_bytes(real_bytes, a.tab.n_fft, a.tab.n_filt, a.tab.n_rounds); }

// The four kinds of launch of the general family, as the stock family's above: one template each over the precision R
// (declared in mfcc_general_device.h)
template <class R>
hipError_t launch_general_stream(const GeneralStreamArgs<R>& a, hipStream_t s, bool mels) {
    if (a.geo.n_streams == 0) return hipSuccess;
    const dim3 grid((PE_GEN_TWO_WAVES ? 2 : 1) * (unsigned)a.geo.n_streams);
    const bool ok = with_general_bits(a.tab, mels, [&](auto B, auto BLUE, auto MELS) {
        PE_LAUNCH_R(R, mfcc_general_stream_kernel, (PE_CONST(B), PE_CONST(BLUE), PE_CONST(MELS)), grid, dim3(64), general_lds(a, sizeof(R)), s, a); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
template <class R>
hipError_t launch_general_offline(const GeneralOfflineArgs<R>& a, int n_cus, hipStream_t s, bool mels) {
    if (a.n_frames <= 0) return hipSuccess;
    const dim3 grid(general_blocks(a.n_frames, n_cus));
    const bool ok = with_general_bits(a.tab, mels, [&](auto B, auto BLUE, auto MELS) {
        PE_LAUNCH_R(R, mfcc_general_offline_kernel, (PE_CONST(B), PE_CONST(BLUE), PE_CONST(MELS)), grid, dim3(64), general_lds(a, sizeof(R)), s, a); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
template <class R>
hipError_t launch_general_clips(const GeneralClipArgs<R>& a, int n_cus, hipStream_t s, bool mels) {
    if (a.clips.n_clips <= 0) return hipSuccess;
    const long long work = a.clips.n_tasks > (uint32_t)a.clips.n_clips ? (long long)a.clips.n_tasks : (long long)a.clips.n_clips;
    const dim3 grid(general_blocks(work, n_cus));
    const bool ok = with_general_bits(a.tab, mels, [&](auto B, auto BLUE, auto MELS) {
        PE_LAUNCH_R(R, mfcc_general_clips_kernel, (PE_CONST(B), PE_CONST(BLUE), PE_CONST(MELS)), grid, dim3(64), general_lds(a, sizeof(R)), s, a); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
template <class R>
hipError_t launch_general_recs(const GeneralRecArgs<R>& a, int n_cus, hipStream_t s, bool mels) {
    if (a.recs.n_tasks == 0) return hipSuccess;
    const dim3 grid(general_blocks((long long)a.recs.n_tasks, n_cus));
    const bool ok = with_general_bits(a.tab, mels, [&](auto B, auto BLUE, auto MELS) {
        PE_LAUNCH_R(R, mfcc_general_recs_kernel, (PE_CONST(B), PE_CONST(BLUE), PE_CONST(MELS)), grid, dim3(64), general_lds(a, sizeof(R)), s, a); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// the eight front-end launchers for one precision: the only place where a launcher meets a concrete R
#define PE_FRONT_END_LAUNCHERS(R)                                                                                            \
    template hipError_t launch_mfcc(const MfccStreamArgs<R>&, const WaveTables<R>&, int, hipStream_t, bool);                 \
    template hipError_t launch_mfcc_offline(const MfccOfflineArgs<R>&, const WaveTables<R>&, int, hipStream_t, bool);        \
    template hipError_t launch_mfcc_clips(const MfccClipArgs<R>&, const WaveTables<R>&, int, hipStream_t, bool);             \
    template hipError_t launch_mfcc_recs(const MfccRecArgs<R>&, const WaveTables<R>&, int, hipStream_t, bool);               \
    template hipError_t launch_general_stream(const GeneralStreamArgs<R>&, hipStream_t, bool);                               \
    template hipError_t launch_general_offline(const GeneralOfflineArgs<R>&, int, hipStream_t, bool);                        \
    template hipError_t launch_general_clips(const GeneralClipArgs<R>&, int, hipStream_t, bool);                             \
    template hipError_t launch_general_recs(const GeneralRecArgs<R>&, int, hipStream_t, bool);
PE_FRONT_END_LAUNCHERS(double)
PE_FRONT_END_LAUNCHERS(float)

// ---- small utility kernels ---------------------------------------------------------------------
__global__ void gather_kernel(const GatherArgs a) {
    // out[s][t][f] = ring row of frame (ke - T + t) of stream s      (Listener.mfccs, oldest first)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)a.n_streams * a.n_features * a.n_mfcc;
    if (idx >= total) return;
    const int f = (int)(idx % a.n_mfcc);
    const int t = (int)((idx / a.n_mfcc) % a.n_features);
    const long long s = idx / ((long long)a.n_mfcc * a.n_features);
    const RecPair both = rec_request(a.st.rec, a.st.n_padded, s);
    const uint32_t ke = rec_pick(both, rec_side(both, a.st.call)).ke;
    const uint32_t slot = (ke - (uint32_t)a.n_features + (uint32_t)t) & (uint32_t)(a.ring_slots - 1);
    const long long tile = s / kTileStreams;
    const int j = (int)(s % kTileStreams);
    const size_t at = (((size_t)tile * a.ring_slots + slot) * kTileStreams + j) * a.row_floats + f;
    a.out[idx] = a.ring_bf16 ? (float)reinterpret_cast<const __bf16*>(a.ring)[at] : a.ring[at];
}

__global__ void scatter_kernel(const GatherArgs a) {
    // inverse of gather_kernel: the stream restarts with the given [T][F] window already emitted
    // (frames 0..T-1 in slots 0..T-1, nothing held toward the next frame)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int RF = a.row_floats;
    const long long total = (long long)a.n_streams * a.n_features * RF;
    if (idx >= total) return;
    const int f = (int)(idx % RF);
    const int t = (int)((idx / RF) % a.n_features);
    const long long s = idx / ((long long)RF * a.n_features);
    const long long tile = s / kTileStreams;
    const int j = (int)(s % kTileStreams);
    const float v = f < a.n_mfcc ? a.out[(s * a.n_features + t) * a.n_mfcc + f] : 0.0f;
    const size_t at = (((size_t)tile * a.ring_slots + t) * kTileStreams + j) * RF + f;
    if (a.ring_bf16) reinterpret_cast<__bf16*>(const_cast<float*>(a.ring))[at] = (__bf16)v;
    else const_cast<float*>(a.ring)[at] = v;
    if (f == 0 && t == 0) {       // side 0 becomes the current one (stamped with this call), side 1 the older
        a.st.rec[rec_at(a.st.n_padded, s, 0)] = StreamRec{0, (uint32_t)a.n_features, (uint32_t)a.n_features, a.st.call};
        a.st.rec[rec_at(a.st.n_padded, s, 1)] = StreamRec{0, (uint32_t)a.n_features, (uint32_t)a.n_features, a.st.call - 1u};
    }
}

hipError_t launch_scatter(const GatherArgs& a, hipStream_t s) {
    const long long total = (long long)a.n_streams * a.n_features * a.row_floats;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// call numbers wrap after 2^32 calls: long before, every record is renumbered (current side 2, other side 1) and the host
// restarts its counter at 3 -- only the ORDER of a stream's two sides and "not this call" are ever read
__global__ void renumber_kernel(const StreamState st, const int n_padded) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_padded) return;
    const RecPair both = rec_request(st.rec, st.n_padded, s);
    const int side = rec_side(both, st.call);
    st.rec[rec_at(st.n_padded, s, side)].wcall = 2u;
    st.rec[rec_at(st.n_padded, s, side ^ 1)].wcall = 1u;
}
// leaving the keep style (MfccStreamArgs::head): 16 lanes per stream copy its leftover -- the last q samples of its row of the
// kept chunks -- into its current carry side (a rare launch: one per switch of calling styles)
__global__ __launch_bounds__(256) void materialize_carry_kernel(const StreamState st, const int16_t* head, const int head_chunk, const int n_streams) {
    const int s = blockIdx.x * 16 + (threadIdx.x >> 4), r = threadIdx.x & 15;
    if (s >= n_streams) return;
    const RecPair both = rec_request(st.rec, st.n_padded, s);
    const int side = rec_side(both, st.call);
    const int q = side ? both.r1.q : both.r0.q;
    const int16_t* const src = head + (size_t)s * head_chunk + (head_chunk - q);
    int16_t* const dst = st.carry + ((size_t)side * st.n_padded + (size_t)s) * kCarryCap;
    for (int i = r; i < q; i += 16) dst[i] = src[i];
}
hipError_t launch_materialize_carry(const StreamState& st, const int16_t* head, int head_chunk, int n_streams, hipStream_t s) {
    hipLaunchKernelGGL(materialize_carry_kernel, dim3((n_streams + 15) / 16), dim3(256), 0, s, st, head, head_chunk, n_streams);
    return hipGetLastError();
}

hipError_t launch_renumber(const StreamState& st, int n_padded, hipStream_t s) {
    hipLaunchKernelGGL(renumber_kernel, dim3((n_padded + 255) / 256), dim3(256), 0, s, st, n_padded);
    return hipGetLastError();
}

__global__ void clear_kernel(const ClearArgs a) {
    // one workgroup per stream: zero its counters and every ring row
    const long long s = blockIdx.x;
    if (s >= a.n_streams) return;
    if (a.mask && !a.mask[s]) return;
    if (threadIdx.x == 0) {         // side 0 becomes the current one (stamped with this call), side 1 the older
        a.st.rec[rec_at(a.st.n_padded, s, 0)] = StreamRec{0, 0u, 0u, a.st.call};
        a.st.rec[rec_at(a.st.n_padded, s, 1)] = StreamRec{0, 0u, 0u, a.st.call - 1u};
        if (a.activation) a.activation[s] = 0;
    }
    const long long tile = s / kTileStreams;
    const int j = (int)(s % kTileStreams);
    for (int i = threadIdx.x; i < a.ring_slots * a.row_floats; i += blockDim.x) {
        const int slot = i / a.row_floats, f = i % a.row_floats;
        const size_t at = (((size_t)tile * a.ring_slots + slot) * kTileStreams + j) * a.row_floats + f;
        if (a.ring_bf16) reinterpret_cast<__bf16*>(a.ring)[at] = (__bf16)0.0f;
        else a.ring[at] = 0.0f;
    }
    if (a.proj_ring)            // the projection of an all-zero frame is the bias row
        for (int i = threadIdx.x; i < a.ring_slots * kProjRow; i += blockDim.x) {
            const int slot = i / kProjRow, o = i % kProjRow;
            // element o = 16 g + 4 tl + q of stream j sits at [tl][j][g][q] inside the (tile, slot) block
            a.proj_ring[((size_t)tile * a.ring_slots + slot) * kTileStreams * kProjRow + (size_t)((o >> 2) & 3) * (kTileStreams * 16) + j * 16 + (o >> 4) * 4 + (o & 3)] = a.proj_b[o];
        }
}

__global__ void project_rows_kernel(const float* ring, float* proj, const float* w, const float* b, const int n_mfcc, const long long n_rows) {
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int o = threadIdx.x & 63;
    if (row >= n_rows) return;
    float acc = b[o];
    for (int c = 0; c < n_mfcc; ++c) acc = fmaf(ring[row * kRowFloats + c], w[c * kProjRow + o], acc);
    const long long block = row / kTileStreams;          // (tile, slot) block; row % 16 = stream j
    const int j = (int)(row % kTileStreams);
    proj[block * kTileStreams * kProjRow + (size_t)((o >> 2) & 3) * (kTileStreams * 16) + j * 16 + (o >> 4) * 4 + (o & 3)] = acc;
}

hipError_t launch_project_rows(const float* ring, float* proj, const float* w, const float* b, int n_mfcc, long long n_rows, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(project_rows_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, ring, proj, w, b, n_mfcc, n_rows);
    return hipGetLastError();
}

// ThresholdDecoder.decode + TriggerDetector.update of row s (decode_kernel, decode_models_kernel): stream s, or with a.ids
// stream a.ids[s] -- the row's input and outputs stay at s, only the trigger state is the named stream's
__device__ __forceinline__ void decode_stream(const DecodeArgs& a, const int s) {
    const float rawf = a.raw[s];
    const double raw = (double)rawf;
    double conf = raw;
    if (raw != 1.0 && raw != 0.0) {                       // saturated sigmoid passes through (:46-47)
        double cp;
        if (a.out_range == 0) {
            cp = raw > (double)a.min_out ? 1.0 : 0.0;
        } else {
            // asigmoid (functions.py:99-101) on the runner's float32 scalar: numpy evaluates `1 / x - 1` in
            // float32 (two correctly rounded operations), math.log then takes that value as a double
            const float odds = __fsub_rn(__fdiv_rn(1.0f, rawf), 1.0f);
            double ratio = (-log((double)odds) - (double)a.min_out) / (double)a.out_range;
            ratio = fmin(fmax(ratio, 0.0), 1.0);
            cp = a.cd[(int)(ratio * (double)(a.cd_len - 1) + 0.5)];
        }
        conf = cp < a.center ? 0.5 * cp / a.center : 0.5 + 0.5 * (cp - a.center) / (1.0 - a.center);
    }
    if (a.conf_out) a.conf_out[s] = conf;
    if (a.activation) {
        const int t = a.ids ? a.ids[s] : s;
        int act = a.activation[t];
        const bool hot = conf > a.threshold;
        bool fired = false;
        if (!hot && act >= 0) {
            if (act > 0) act -= 1;
        } else {
            act += 1;
            fired = act > a.trigger_level;
            if (fired || (hot && act < 0)) act = a.rearm;
        }
        a.activation[t] = act;
        if (a.fired_out) a.fired_out[s] = fired ? 1 : 0;
    }
}
__global__ void decode_kernel(const DecodeArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_streams) return;
    decode_stream(a, s);
}
// a K-model engine: model blockIdx.y with its own table, thresholds and trigger rows, ONE launch for all models
__global__ void decode_models_kernel(const DecodeSet d) {
    const DecodeArgs& a = d.m[blockIdx.y];
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_streams) return;
    decode_stream(a, s);
}
// the trigger rows of models 1 .. n_rows of a K-model engine, cleared as clear_kernel clears model 0's (mask: the streams cleared)
__global__ void clear_activation_kernel(const uint8_t* mask, int32_t* activation, const int n_streams, const int n_padded) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams || (mask && !mask[s])) return;
    activation[(size_t)(blockIdx.y + 1) * n_padded + s] = 0;
}

hipError_t launch_decode_models(const DecodeSet& d, int n_models, int n_streams, hipStream_t s) {
    if (n_models < 1 || n_models > kMaxModels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_models_kernel, dim3((n_streams + 255) / 256, n_models), dim3(256), 0, s, d);
    return hipGetLastError();
}
hipError_t launch_clear_activation(const uint8_t* mask, int32_t* activation, int n_streams, int n_padded, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_streams < 1) return hipSuccess;
    hipLaunchKernelGGL(clear_activation_kernel, dim3((n_streams + 255) / 256, n_rows), dim3(256), 0, s, mask, activation, n_streams, n_padded);
    return hipGetLastError();
}
hipError_t launch_decode(const DecodeArgs& a, hipStream_t s) {
    if (a.n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(decode_kernel, dim3((a.n_streams + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- the metrics of simulate.py:114-122 / annoyance_estimator.py:70-71 (pe_common.h: SimArgs) --------------------------
// One wave per word of 64 predictions of one recording, model blockIdx.y.  Every comparison is made on the prediction
// widened to float64.  The word's sum is a butterfly over its 64 slots (absent ones add +0.0): a fixed shape, so the sum of a
// recording depends on its predictions alone.  The bin of a prediction is the number of thresholds below it (a NaN
// prediction: none); a workgroup counts bins in LDS and adds what it counted to the global histogram with integer atomics.
constexpr int kSimWaves = 4;
__global__ __launch_bounds__(64 * kSimWaves) void sim_scan_kernel(const SimArgs a) {
    extern __shared__ uint32_t sim_bins[];
    const int m = (int)blockIdx.y, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_bins = a.n_thresholds + 1;
    if (a.hist) {
        for (int i = threadIdx.x; i < n_bins; i += 64 * kSimWaves) sim_bins[i] = 0;
        __syncthreads();
    }
    const auto recs = PE_UNIFORM_PTR(SimRec, a.recs);
    const auto word_prefix = PE_UNIFORM_PTR(uint32_t, a.word_prefix);
    const float* const src = a.src + (size_t)m * a.src_stride;
    float* const dst = a.dst ? a.dst + (size_t)m * a.dst_stride : nullptr;
    const size_t row = (size_t)m * a.n_words;
    int r = 0;
    for (uint32_t w = blockIdx.x * kSimWaves + wave; w < a.n_words; w += gridDim.x * kSimWaves) {
        r = slot_of_task(a.word_prefix, a.n_rec, w, r);
        const long long j = (long long)(w - word_prefix[r]) * 64 + lane;
        const bool valid = j < recs[r].n_windows;
        const float pf = valid ? src[recs[r].src0 + j] : 0.0f;
        if (dst && valid) dst[recs[r].dst0 + j] = pf;
        const double p = (double)pf;
        const unsigned long long chunk = __ballot(valid && p > a.chunk_threshold), trig = __ballot(valid && p > a.trigger_threshold);
        double sum = p;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);        // (a + b = b + a: every lane ends with the same bits)
        if (a.trig && lane == 0) {
            a.trig[row + w] = trig;
            a.chunk_count[row + w] = (uint32_t)__popcll(chunk);
            a.partial[row + w] = sum;
        }
        if (a.hist && valid) {
            int lo = 0, hi = a.n_thresholds;            // thresholds[0 .. lo) < p, thresholds[hi ..) are not
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (a.thresholds[mid] < p) lo = mid + 1; else hi = mid;
            }
            atomicAdd(&sim_bins[lo], 1u);
        }
    }
    if (a.hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_bins; i += 64 * kSimWaves)
            if (sim_bins[i]) atomicAdd(&a.hist[(size_t)m * n_bins + i], (unsigned long long)sim_bins[i]);
    }
}
// One lane per (recording, model blockIdx.y): TriggerDetector.update (runner.py:127-142, decode_stream above) over the
// recording's trigger bits in order, from a fresh detector.  A word without a hot bit met with activation >= 0 only decays the
// counter: the common case, taken in one step.  The word sums are added in word order.
__global__ void sim_fold_kernel(const SimArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x, m = (int)blockIdx.y;
    if (r >= a.n_rec) return;
    const long long n = a.recs[r].n_windows;
    const size_t first = (size_t)m * a.n_words + a.word_prefix[r];
    int act = 0;
    long long fired = 0, chunks = 0;
    double sum = 0.0;
    for (long long k = 0; k * 64 < n; ++k) {
        const unsigned long long word = a.trig[first + k];
        chunks += a.chunk_count[first + k];
        sum += a.partial[first + k];
        const int bits = n - k * 64 < 64 ? (int)(n - k * 64) : 64;
        if (word == 0 && act >= 0) { act = act > bits ? act - bits : 0; continue; }
        for (int b = 0; b < bits; ++b) {
            const bool hot = (word >> b) & 1;
            if (!hot && act >= 0) {
                if (act > 0) act -= 1;
            } else {
                act += 1;
                const bool f = act > a.trigger_level;
                if (f || (hot && act < 0)) act = a.rearm;
                fired += f ? 1 : 0;
            }
        }
    }
    a.metrics[(size_t)m * a.metric_stride + r] = SimMetric{n, chunks, fired, sum};
}
hipError_t launch_simulate(const SimArgs& a, int n_models, int n_cus, hipStream_t s) {
    if (a.n_rec <= 0 || n_models < 1) return hipSuccess;
    if (a.n_words) {
        const long long want = ((long long)a.n_words + kSimWaves - 1) / kSimWaves, cap = (long long)n_cus * 8;
        hipLaunchKernelGGL(sim_scan_kernel, dim3((unsigned)(want < cap ? want : cap), n_models), dim3(64 * kSimWaves),
                           a.hist ? (size_t)(a.n_thresholds + 1) * sizeof(uint32_t) : 0, s, a);
    }
    if (a.metrics) hipLaunchKernelGGL(sim_fold_kernel, dim3((a.n_rec + 63) / 64, n_models), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ---- training (gru_train_device.h) -------------------------------------------------------------------------------------
template <bool BACKWARD>
__global__ __launch_bounds__(64 * 8) void train_tile_kernel(const TrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float train_lds[];
    const int m = blockIdx.x % a.n_models;
    train_tile<BACKWARD>(train_view(a, m), train_lds, blockIdx.x / a.n_models);
}
__global__ __launch_bounds__(256) void train_reduce_kernel(const TrainArgs a) { train_reduce(a); }
__global__ __launch_bounds__(256) void train_apply_kernel(const TrainArgs a) { train_apply(a); }
__global__ __launch_bounds__(kTrainAccThreads) void train_accuracy_kernel(const TrainAccuracyArgs a) {
    __shared__ int32_t hits[kTrainAccThreads];
    train_accuracy(a, hits);
}

size_t train_lds_bytes(int F, int H) { return (size_t)TrainLds(F, H).total * sizeof(float); }

template <bool BACKWARD>
static hipError_t launch_train_t(const TrainArgs& a, hipStream_t s) {
    int widest = 0;
    for (int m = 0; m < a.n_models; ++m) widest = a.model[m].H > widest ? a.model[m].H : widest;
    if (a.threads != train_threads(widest) || a.threads > 64 * 8) return hipErrorInvalidValue;
    const size_t lds = train_lds_bytes(a.F, widest);                 // TrainLds grows with H: the widest network's layout
    if (lds > 48 * 1024) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(&train_tile_kernel<BACKWARD>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(train_tile_kernel<BACKWARD>, dim3((unsigned)a.n_blocks * a.n_models), dim3(a.threads), lds, s, a);
    return hipGetLastError();
}
hipError_t launch_train(const TrainArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.n_models < 1 || a.n_models > kTrainMaxModels) return hipErrorInvalidValue;
    if (a.n_blocks != (a.n + kTrainTile - 1) / kTrainTile) return hipErrorInvalidValue;
    return a.backward ? launch_train_t<true>(a, s) : launch_train_t<false>(a, s);
}
hipError_t launch_train_reduce(const TrainArgs& a, hipStream_t s) {
    const int threads = (a.backward ? a.n_total : 0) + a.n_models;
    hipLaunchKernelGGL(train_reduce_kernel, dim3((threads + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_train_apply(const TrainArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(train_apply_kernel, dim3((a.n_total + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_train_accuracy(const TrainAccuracyArgs& a, int n_models, hipStream_t s) {
    hipLaunchKernelGGL(train_accuracy_kernel, dim3(n_models), dim3(kTrainAccThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gather(const GatherArgs& a, hipStream_t s) {
    const long long total = (long long)a.n_streams * a.n_features * a.n_mfcc;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_clear(const ClearArgs& a, hipStream_t s) {
    if (a.n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(clear_kernel, dim3(a.n_streams), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe

