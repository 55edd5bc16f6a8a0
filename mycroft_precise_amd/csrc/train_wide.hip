// The __global__ entry points of wide training (pe_trainer_create_wide: networks of 33..256 units) and their launcher; the
// device code is gru_train_wide_device.h.
#include "gru_train_wide_device.h"

using namespace pe;

template <bool BACKWARD>
__global__ __launch_bounds__(64 * kTwMaxWaves) void tw_forward_kernel(const TrainWideArgs a) {
    __shared__ __attribute__((aligned(16))) float HT[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float RHT[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float XM[2 * kTwLdsX];
    __shared__ __attribute__((aligned(16))) float MS[kTwLdsX];
    __shared__ float SC[kTwMaxWaves * 16 + 48];
    tw_forward<BACKWARD>(a, HT, RHT, XM, MS, SC);
}
__global__ __launch_bounds__(256) void tw_pack_kernel(const TrainWideArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < 3 * a.Hp * a.Hp) tw_pack(a.ut, a.theta + a.F * 3 * a.H, e, a.H, a.Hp, a.H, a.Hp);
}
__global__ __launch_bounds__(64 * kTwMaxWaves) void tw_backward_kernel(const TrainWideArgs a) {
    __shared__ __attribute__((aligned(16))) float DZ[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float DR[kTwLdsState];
    __shared__ __attribute__((aligned(16))) float DH[kTwLdsState];
    tw_backward<TwDx::kNone>(a.T, tw_layer(a), a.fin, TwDxArgs{}, DZ, DR, DH);
}
__global__ __launch_bounds__(256) void tw_gemm_kernel(const TrainWideArgs a) { tw_gemm<false>(a.T, a.n_tiles, tw_layer(a), TwGemmBelow{}); }
__global__ __launch_bounds__(256) void tw_reduce_kernel(const TrainWideArgs a) {
    const TwLayer l0 = tw_layer(a);
    const TwLayer* const l[1] = {&l0};
    tw_reduce(a, l, a.partial);
}

namespace pe {

hipError_t launch_train_wide(const TrainWideArgs& a, hipStream_t s) {
    if (a.H <= kTrainMaxUnits || a.H > kTwMaxUnits || a.Hp != tw_pad(a.H)) return hipErrorInvalidValue;
    if (a.F < 1 || a.F > kTrainMaxFeat || a.T < 1 || a.n < 1 || a.n_tiles != (a.n + 15) / 16) return hipErrorInvalidValue;
    if (!a.theta || !a.feats || !a.partial || !a.loss) return hipErrorInvalidValue;
    if (a.backward && (!a.tape || !a.fin || !a.ut || !a.gpart || !a.grads || !a.accum)) return hipErrorInvalidValue;
    const unsigned threads = 64u * (unsigned)tw_waves(a.H);
    if (a.backward) hipLaunchKernelGGL(tw_forward_kernel<true>, dim3((unsigned)a.n_tiles), dim3(threads), 0, s, a);
    else hipLaunchKernelGGL(tw_forward_kernel<false>, dim3((unsigned)a.n_tiles), dim3(threads), 0, s, a);
    int n_par = 0;
    if (a.backward) {
        hipLaunchKernelGGL(tw_pack_kernel, dim3((unsigned)(3 * a.Hp * a.Hp + 255) / 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(tw_backward_kernel, dim3((unsigned)a.n_tiles), dim3(threads), 0, s, a);
        hipLaunchKernelGGL(tw_gemm_kernel, tw_gemm_grid(a.T, a.n_tiles, a.F, a.H), dim3(256), 0, s, a);
        n_par = train_n_params(a.F, a.H);
    }
    hipLaunchKernelGGL(tw_reduce_kernel, dim3((unsigned)(n_par + 1 + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace pe
