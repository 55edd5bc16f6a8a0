// The __global__ entry points of stacked training (pe_trainer_create_stacked: two GRU layers of 1..256 units each) and their
// launcher; the device code is gru_train_stacked_device.h.
#include "gru_train_stacked_device.h"

using namespace pe;

template <bool BACKWARD>
__global__ __launch_bounds__(64 * kTwMaxWaves) void ts_forward0_kernel(const TrainStackedArgs a) {
    __shared__ __attribute__((aligned(16))) float HT[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float RHT[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float XM[2 * kTwLdsX];
    __shared__ __attribute__((aligned(16))) float MS[kTwLdsX];
    ts_forward0<BACKWARD>(a, HT, RHT, XM, MS);
}
template <bool BACKWARD>
__global__ __launch_bounds__(64 * kTwMaxWaves) void ts_forward1_kernel(const TrainStackedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ts_lds[];
    ts_forward1<BACKWARD>(a, ts_lds);
}
__global__ __launch_bounds__(256) void ts_pack_kernel(const TrainStackedArgs a) { ts_pack(a); }
__global__ __launch_bounds__(64 * kTwMaxWaves) void ts_backward1_kernel(const TrainStackedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ts_lds[];
    float* const DZ = ts_lds;
    float* const DR = DZ + a.H2p * 16;
    float* const DH = DR + a.H2p * 16;
    tw_backward<TwDx::kWrite>(a.T, ts_layer1(a), a.fin, TwDxArgs{a.dx, a.H1p, a.w1t, a.mtape, DH + a.H2p * 16}, DZ, DR, DH);
}
__global__ __launch_bounds__(64 * kTwMaxWaves) void ts_backward0_kernel(const TrainStackedArgs a) {
    __shared__ __attribute__((aligned(16))) float DZ[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float DR[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float DH[kTwLdsState];
    tw_backward<TwDx::kRead>(a.T, ts_layer0(a), nullptr, TwDxArgs{a.dx, a.H1p, nullptr, nullptr, nullptr}, DZ, DR, DH);
}
__global__ __launch_bounds__(256) void ts_gemm0_kernel(const TrainStackedArgs a) {
    tw_gemm<false>(a.T, a.n_tiles, ts_layer0(a), TwGemmBelow{});
}
__global__ __launch_bounds__(256) void ts_gemm1_kernel(const TrainStackedArgs a) {
    tw_gemm<true>(a.T, a.n_tiles, ts_layer1(a), TwGemmBelow{a.tape0, tw_record(a.F, a.H1p), a.hfin0, a.mtape, a.H1p});
}
__global__ __launch_bounds__(256) void ts_reduce_kernel(const TrainStackedArgs a) {
    const TwLayer l0 = ts_layer0(a), l1 = ts_layer1(a);
    const TwLayer* const l[2] = {&l0, &l1};
    tw_reduce(a, l, a.partial);
}
__global__ __launch_bounds__(256) void ts_apply_kernel(const TrainStackedArgs a) { ts_apply(a); }

namespace pe {

size_t ts_forward1_lds(int H1p, int H2p) { return (size_t)ts_forward1_lds_floats(H1p, H2p) * sizeof(float); }
size_t ts_backward1_lds(int H1p, int H2p) { return (size_t)ts_backward1_lds_floats(H1p, H2p) * sizeof(float); }

namespace {
hipError_t ts_allow_lds(const void* kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

bool ts_shape_ok(const TrainStackedArgs& a) {
    if (a.H1 < 1 || a.H1 > kTwMaxUnits || a.H1p != tw_pad(a.H1) || a.H2 < 1 || a.H2 > kTwMaxUnits || a.H2p != tw_pad(a.H2)) return false;
    return a.F >= 1 && a.F <= kTrainMaxFeat && a.T >= 1;
}
}  // namespace

hipError_t launch_train_stacked(const TrainStackedArgs& a, hipStream_t s) {
    if (!ts_shape_ok(a) || a.n < 1 || a.n_tiles != (a.n + 15) / 16) return hipErrorInvalidValue;
    if (!a.theta || !a.feats || !a.partial || !a.loss || !a.hfin0) return hipErrorInvalidValue;
    if (a.backward && (!a.tape0 || !a.tape1 || !a.mtape || !a.dx || !a.fin || !a.ut0 || !a.ut1 || !a.w1t || !a.gpart0 || !a.gpart1 ||
                       !a.grads || !a.accum))
        return hipErrorInvalidValue;
    if (a.mask_mode == 1 && (!a.masks0 || !a.masks1)) return hipErrorInvalidValue;
    const dim3 tiles((unsigned)a.n_tiles);
    const unsigned th0 = 64u * (unsigned)tw_waves(a.H1), th1 = 64u * (unsigned)tw_waves(a.H2);
    const size_t lf = ts_forward1_lds(a.H1p, a.H2p), lb = ts_backward1_lds(a.H1p, a.H2p);
    hipError_t err;
    if (a.backward) {
        if ((err = ts_allow_lds(reinterpret_cast<const void*>(&ts_forward1_kernel<true>), lf)) != hipSuccess) return err;
        if ((err = ts_allow_lds(reinterpret_cast<const void*>(&ts_backward1_kernel), lb)) != hipSuccess) return err;
        hipLaunchKernelGGL(ts_forward0_kernel<true>, tiles, dim3(th0), 0, s, a);
        hipLaunchKernelGGL(ts_forward1_kernel<true>, tiles, dim3(th1), lf, s, a);
    } else {
        if ((err = ts_allow_lds(reinterpret_cast<const void*>(&ts_forward1_kernel<false>), lf)) != hipSuccess) return err;
        hipLaunchKernelGGL(ts_forward0_kernel<false>, tiles, dim3(th0), 0, s, a);
        hipLaunchKernelGGL(ts_forward1_kernel<false>, tiles, dim3(th1), lf, s, a);
    }
    int n_par = 0;
    if (a.backward) {
        const int packed = 3 * (a.H1p * a.H1p + a.H2p * a.H2p + a.H2p * a.H1p);
        hipLaunchKernelGGL(ts_pack_kernel, dim3((unsigned)(packed + 255) / 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(ts_backward1_kernel, tiles, dim3(th1), lb, s, a);
        hipLaunchKernelGGL(ts_backward0_kernel, tiles, dim3(th0), 0, s, a);
        hipLaunchKernelGGL(ts_gemm0_kernel, tw_gemm_grid(a.T, a.n_tiles, a.F, a.H1), dim3(256), 0, s, a);
        hipLaunchKernelGGL(ts_gemm1_kernel, tw_gemm_grid(a.T, a.n_tiles, a.H1, a.H2), dim3(256), 0, s, a);
        n_par = ts_n_params(a.F, a.H1, a.H2);
    }
    hipLaunchKernelGGL(ts_reduce_kernel, dim3((unsigned)(n_par + 1 + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_train_stacked_apply(const TrainStackedArgs& a, hipStream_t s) {
    if (!ts_shape_ok(a) || !a.theta || !a.accum || !a.grads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ts_apply_kernel, dim3((unsigned)(ts_n_params(a.F, a.H1, a.H2) + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe
