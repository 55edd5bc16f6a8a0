// Training of the one-layer network: forward with a tape, backward, deterministic reduction of the
// weight gradients over workgroups, RMSprop.  Everything float32.
//
// One workgroup trains a tile of 16 samples with one thread per (sample, unit): 16 H threads rounded up to whole
// waves (320 = five waves at the stock 20 units).  The weights, the per-step operands and the per-step gradients of the
// pre-activations live in LDS; the tape (h_(t-1), z, r, c per step: 4 H T floats per sample) goes to HBM, where the
// thread that wrote a value is the one that reads it back, so it needs no ordering beyond program order.
// Weight gradients are outer products over the tile, dTheta[row][col] += sum_s L[s][row] D[s][col], with L the left
// operands of the step (masked inputs | h_(t-1) or r h_(t-1) | 1) and D the pre-activation gradients; every thread keeps a
// fixed set of (row, col) sums in registers over all steps, in a fixed order, and the workgroup writes one partial
// gradient vector.  train_reduce_kernel adds the partials in workgroup order (no floating-point atomic anywhere) and may
// apply RMSprop in the same pass.
//
// Several networks (widths 1..32, their own hyperparameters) train on the same batch in ONE launch over (tile, network),
// network fastest, so the workgroups that gather the same rows run next to each other.  The block is as wide as the widest
// network needs and the LDS is the widest network's layout; a narrower network leaves threads idle (`active`) and strides
// its staging loops, its tape and its gradient elements by the launch's width.  None of that enters a sum: every sum runs
// over samples and timesteps in an order fixed by (F, H) alone, so a network's bits do not depend on its company.  The
// per-network record (TrainModel) is read once per workgroup, outside the timestep loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pe {

constexpr int kTrainTile = 16;          // samples per workgroup
constexpr int kTrainMaxUnits = 32, kTrainMaxFeat = 32, kTrainMaxSteps = 64;
constexpr int kTrainAcc = 13;           // weight-gradient sums per thread: ceil(3 (F + H + 1) H / (16 H)) <= 13 for F, H <= 32

// ---- dropout masks: a pure integer function, the same on the host and on the device -------------------------------------
__host__ __device__ inline uint64_t train_mix64(uint64_t v) {          // the splitmix64 finaliser
    v ^= v >> 30; v *= 0xBF58476D1CE4E5B9ull;
    v ^= v >> 27; v *= 0x94D049BB133111EBull;
    v ^= v >> 31;
    return v;
}
constexpr uint64_t kTrainGolden = 0x9E3779B97F4A7C15ull;
// the key of one (seed, step): computed once per call
__host__ __device__ inline uint64_t train_mask_key(uint64_t seed, uint64_t step) {
    return train_mix64(train_mix64(seed + kTrainGolden) ^ (step + kTrainGolden));
}
// 1 = keep.  gate 0 / 1 / 2 = z / r / h, pos = position in the batch, feature < 32
__host__ __device__ inline bool train_mask_keep(uint64_t key, int gate, int64_t pos, int feature, float rate) {
    const uint64_t ctr = ((uint64_t)pos << 7) | ((uint64_t)gate << 5) | (uint64_t)feature;
    const uint64_t bits = train_mix64(key + kTrainGolden * (ctr + 1));
    return (float)(bits >> 40) * (1.0f / 16777216.0f) >= rate;
}

// ---- flat parameter order: kernel[F][3H] | recurrent_kernel[H][3H] | bias[3H] | dense_kernel[H] | dense_bias -----------
__host__ __device__ inline int train_n_gru(int F, int H) { return (F + H + 1) * 3 * H; }
__host__ __device__ inline int train_n_params(int F, int H) { return train_n_gru(F, H) + H + 1; }
inline int train_threads(int H) { return (kTrainTile * H + 63) / 64 * 64; }

constexpr int kTrainMaxModels = 16;     // PE_TRAIN_MAX_MODELS: 16 records of 64 bytes travel by value in the kernel arguments

// What one workgroup of train_tile works on: the shared batch and ONE network.
struct TrainView {
    int n, T, F, H;
    const float* theta;         // flat parameters of the network
    const float* feats;         // [rows][T][F]
    const float* targets;       // [rows], or null (forward only: read as 0)
    const int32_t* indices;     // [n] rows of feats / targets, or null: row i
    int mask_mode;              // 0 none, 1 masks[3][n][F], 2 generated from mask_key
    const float* masks;
    uint64_t mask_key;
    float rate, keep_scale;     // keep_scale = 1 / (1 - rate), formed once on the host
    float beta, inv_n;
    float* tape;                // [blocks][T][4][threads of the launch]   (training only)
    float* partial;             // [blocks][n_grad + 2]: the gradient, then the two loss sums
    int n_grad;                 // train_n_params, or 0 for a forward-only launch
    float* probs;               // [n] or null
};

// The per-network record of a launch (64 bytes).  Everything not in here is shared by the networks of the launch.
struct TrainModel {
    int H;                      // units
    int ofs;                    // of this network's flat vector in the concatenation (theta, accum, grads alike)
    int mask_mode;
    int frozen_mask;            // bit 0 freezes [0, n_gru), bit 1 the rest
    float rate, keep_scale, beta;
    float lr, rho, eps;
    uint64_t mask_key;
    uint64_t tape_ofs;          // in floats from TrainArgs::tape: [blocks][T][4][threads]
    uint64_t partial_ofs;       // in floats from TrainArgs::partial: [blocks][n_grad + 2]
};

static_assert(sizeof(TrainModel) == 64, "kTrainMaxModels records of 64 bytes are what the kernel arguments are sized for");

// One launch over (tile, network), network fastest: workgroup b works on tile b / n_models for network b % n_models.
// train_tile_kernel and train_reduce_kernel / train_apply_kernel take the same arguments.
struct TrainArgs {
    int n, T, F, n_models;
    int backward;               // 1: gradients (n_grad = train_n_params per network); 0: forward only (n_grad = 0)
    int n_blocks;               // tiles
    int threads;                // of the tile launch: train_threads(widest network)
    int apply;                  // reduction: 1 = RMSprop on theta / accum with the summed gradient
    int n_total;                // floats of the concatenated flat vector
    float inv_n;
    float* theta;               // concatenated flat parameters
    float* accum;
    float* grads;               // [n_total] or null
    float* loss;                // [n_models]
    const float* feats;
    const float* targets;
    const int32_t* indices;
    const float* masks;         // mask_mode 1 (one network only)
    float* tape;
    float* partial;
    float* probs;               // [n_models][n] or null
    TrainModel model[kTrainMaxModels];
};

static_assert(sizeof(TrainArgs) <= 1280, "the kernel arguments stay well below the 4 KB a launch may carry");

struct TrainAccuracyArgs {
    const float* probs;         // [n_models][n]
    const float* targets;       // [n]
    int n;
    int32_t* hits;              // [n_models]: samples with rintf(p) == y
};

hipError_t launch_train(const TrainArgs& a, hipStream_t s);                  // a.threads must be train_threads(widest H)
hipError_t launch_train_reduce(const TrainArgs& a, hipStream_t s);
hipError_t launch_train_apply(const TrainArgs& a, hipStream_t s);           // a.grads is read
hipError_t launch_train_accuracy(const TrainAccuracyArgs& a, int n_models, hipStream_t s);
size_t train_lds_bytes(int F, int H);

#if defined(__HIPCC__)

// The state is float32; the update itself is evaluated in float64 from the float32 state and rounded once.  In float32
// arithmetic theta - lr g / (sqrt(a) + eps) loses every bit the subtraction cancels (the first RMSprop steps move each
// parameter by about 3 lr whatever the gradient: a parameter of that size lands near zero with the rounding errors of the
// quotient, a dozen and more of ITS ulps); one element costs a handful of float64 operations.  Every operation is pinned (no
// contraction), so the fused step and pe_trainer_apply give the same bits.
__device__ inline void train_rmsprop(float& theta, float& accum, const float g, const float lr, const float rho, const float eps) {
    const double gd = (double)g, r = (double)rho;
    const double a = __fma_rn(r, (double)accum, __dmul_rn(__dsub_rn(1.0, r), __dmul_rn(gd, gd)));
    const double step = __ddiv_rn(__dmul_rn((double)lr, gd), __dadd_rn(__dsqrt_rn(a), (double)eps));
    accum = (float)a;
    theta = (float)__dsub_rn((double)theta, step);
}

__device__ inline float train_hard_sigmoid(float a) { return fminf(fmaxf(0.2f * a + 0.5f, 0.0f), 1.0f); }

// LDS layout in floats; the same function sizes the launch
struct TrainLds {
    int W, U, UT, B, WD, MS, XM, HS, RH, D, L, SC, total;
    __host__ __device__ TrainLds(int F, int H) {
        const int R = F + H + 1;
        int o = 0;
        W = o;  o += F * 3 * H;                  // kernel
        U = o;  o += H * 3 * H;                  // recurrent kernel
        UT = o; o += 3 * H * H;                  // its transpose [3H][H]
        B = o;  o += 3 * H;
        WD = o; o += H + 1;                      // dense kernel, dense bias
        MS = o; o += 3 * kTrainTile * F;         // masks [gate][s][f]
        XM = o; o += 2 * 3 * kTrainTile * F;     // masked inputs of the step, two buffers
        HS = o; o += kTrainTile * H;
        RH = o; o += kTrainTile * H;
        D = o;  o += 3 * kTrainTile * H;         // pre-activation gradients [gate][s][j]
        L = o;  o += 3 * kTrainTile * R;         // left operands [gate][s][row]
        SC = o; o += 3 * kTrainTile;
        total = o;
    }
};

template <bool BACKWARD>
__device__ inline void train_tile(const TrainView& a, float* lds, const int blk) {
    const int T = a.T, F = a.F, H = a.H, H3 = 3 * H, R = F + H + 1;
    const int tid = threadIdx.x, nt = blockDim.x;
    const TrainLds o(F, H);
    float* const W = lds + o.W;   float* const U = lds + o.U;   float* const UT = lds + o.UT;
    float* const B = lds + o.B;   float* const WD = lds + o.WD; float* const MS = lds + o.MS;
    float* const XM = lds + o.XM; float* const HS = lds + o.HS; float* const RH = lds + o.RH;
    float* const D = lds + o.D;   float* const L = lds + o.L;   float* const SC = lds + o.SC;
    const bool active = tid < kTrainTile * H;
    const int s = active ? tid / H : 0, j = active ? tid % H : 0;
    const int first = blk * kTrainTile;

    // ---- stage the weights, the masks, h_0 = 0 and the inputs of step 0 ------------------------------------------------
    const float* const th_u = a.theta + F * H3;
    const float* const th_b = th_u + H * H3;
    for (int i = tid; i < F * H3; i += nt) W[i] = a.theta[i];
    for (int i = tid; i < H * H3; i += nt) {
        const float v = th_u[i];
        U[i] = v;
        UT[(i % H3) * H + i / H3] = v;
    }
    for (int i = tid; i < H3; i += nt) B[i] = th_b[i];
    for (int i = tid; i < H + 1; i += nt) WD[i] = th_b[H3 + i];
    for (int i = tid; i < 3 * kTrainTile * F; i += nt) {
        const int g = i / (kTrainTile * F), sf = i % (kTrainTile * F), s2 = sf / F, f = sf % F;
        const int smp = first + s2;
        float m = 1.0f;
        if (smp < a.n) {
            if (a.mask_mode == 1) m = a.masks[((size_t)g * a.n + smp) * F + f];
            else if (a.mask_mode == 2) m = train_mask_keep(a.mask_key, g, smp, f, a.rate) ? a.keep_scale : 0.0f;
        }
        MS[i] = m;
    }
    for (int i = tid; i < kTrainTile * H; i += nt) HS[i] = 0.0f;
    // the row of sample s2 of the tile (null: past the batch, read as zeros)
    auto row_of = [&](int s2) -> const float* {
        const int smp = first + s2;
        if (smp >= a.n) return nullptr;
        const size_t r = a.indices ? (size_t)a.indices[smp] : (size_t)smp;
        return a.feats + r * (size_t)T * F;
    };
    __syncthreads();                                   // MS is read below
    auto stage_x = [&](int t, float* dst, int stride) {      // dst[g][s2][f] = x_t m_g, rows `stride` apart
        for (int i = tid; i < kTrainTile * F; i += nt) {
            const int s2 = i / F, f = i % F;
            const float* row = row_of(s2);
            const float x = row ? row[(size_t)t * F + f] : 0.0f;
            for (int g = 0; g < 3; ++g) dst[(g * kTrainTile + s2) * stride + f] = x * MS[(g * kTrainTile + s2) * F + f];
        }
    };
    stage_x(0, XM, F);
    __syncthreads();

    // ---- forward ------------------------------------------------------------------------------------------------------
    float* const tape = BACKWARD ? a.tape + (size_t)blk * T * 4 * nt + tid : nullptr;
    for (int t = 0; t < T; ++t) {
        const float* xm = XM + (t & 1) * 3 * kTrainTile * F;
        float hp = 0.0f, z = 0.0f, r = 0.0f, ac = 0.0f;
        if (active) {
            float az = B[j], ar = B[H + j];
            ac = B[2 * H + j];
            const float* xz = xm + s * F;
            const float* xr = xz + kTrainTile * F;
            const float* xh = xr + kTrainTile * F;
            for (int f = 0; f < F; ++f) {
                az += xz[f] * W[f * H3 + j];
                ar += xr[f] * W[f * H3 + H + j];
                ac += xh[f] * W[f * H3 + 2 * H + j];
            }
            for (int k = 0; k < H; ++k) {
                const float hk = HS[s * H + k];
                az += hk * U[k * H3 + j];
                ar += hk * U[k * H3 + H + j];
            }
            hp = HS[s * H + j];
            z = train_hard_sigmoid(az);
            r = train_hard_sigmoid(ar);
            RH[s * H + j] = r * hp;
        }
        if (t + 1 < T) stage_x(t + 1, XM + ((t + 1) & 1) * 3 * kTrainTile * F, F);
        __syncthreads();
        if (active) {
            for (int k = 0; k < H; ++k) ac += RH[s * H + k] * U[k * H3 + 2 * H + j];
            HS[s * H + j] = z * hp + (1.0f - z) * ac;
            if (BACKWARD) {
                float* tp = tape + (size_t)t * 4 * nt;
                tp[0] = hp; tp[nt] = z; tp[2 * nt] = r; tp[3 * nt] = ac;
            }
        }
        __syncthreads();
    }

    // ---- head and loss -------------------------------------------------------------------------------------------------
    const int smp = first + s;
    const bool valid = active && smp < a.n;
    float delta = 0.0f;
    {
        float logit = WD[H];
        for (int k = 0; k < H; ++k) logit += HS[s * H + k] * WD[k];
        const float p = 1.0f / (1.0f + expf(-logit));
        const float eps = 1e-7f;
        float y = 0.0f;
        if (valid && a.targets) y = a.targets[a.indices ? (size_t)a.indices[smp] : (size_t)smp];
        const float q = (1.0f - p) + eps, pe = p + eps;
        const float dp = (a.beta * (1.0f - y) / q - (1.0f - a.beta) * y / pe) * a.inv_n;
        const float ds = valid ? dp * p * (1.0f - p) : 0.0f;
        if (active && j == 0) {
            SC[s] = valid ? -(1.0f - y) * logf(q) : 0.0f;
            SC[kTrainTile + s] = valid ? -y * logf(pe) : 0.0f;
            SC[2 * kTrainTile + s] = ds;
            if (valid && a.probs) a.probs[smp] = p;
        }
        delta = ds * WD[j];
    }
    __syncthreads();
    float* const part = a.partial + (size_t)blk * (a.n_grad + 2);
    if (tid == 0) {
        float la = 0.0f, lb = 0.0f;
        for (int s2 = 0; s2 < kTrainTile; ++s2) { la += SC[s2]; lb += SC[kTrainTile + s2]; }
        part[a.n_grad] = la;
        part[a.n_grad + 1] = lb;
    }
    if (!BACKWARD) return;

    const int n_gru = R * H3;
    if (tid <= H) {                                    // dense kernel (tid < H) and dense bias (tid == H)
        float sum = 0.0f;
        for (int s2 = 0; s2 < kTrainTile; ++s2) sum += (tid < H ? HS[s2 * H + tid] : 1.0f) * SC[2 * kTrainTile + s2];
        part[n_gru + tid] = sum;
    }

    // ---- backward -------------------------------------------------------------------------------------------------------
    // this thread's weight-gradient sums: element e = row * 3H + col of the [F + H + 1][3H] block of the flat order
    float acc[kTrainAcc];
    int lo[kTrainAcc], dofs[kTrainAcc];
#pragma unroll
    for (int i = 0; i < kTrainAcc; ++i) {
        acc[i] = 0.0f;
        const int e = tid + i * nt;
        const int row = e / H3, col = e % H3, g = col / H, jj = col % H;
        lo[i] = e < n_gru ? g * kTrainTile * R + row : -1;
        dofs[i] = g * kTrainTile * H + jj;
    }
    for (int i = tid; i < 3 * kTrainTile; i += nt) L[i * R + F + H] = 1.0f;           // the bias row
    for (int t = T - 1; t >= 0; --t) {
        float hp = 0.0f, z = 0.0f, r = 0.0f;
        if (active) {
            const float* tp = tape + (size_t)t * 4 * nt;
            hp = tp[0]; z = tp[nt]; r = tp[2 * nt];
            const float c = tp[3 * nt];
            const float dz = delta * (hp - c);
            D[(2 * kTrainTile + s) * H + j] = delta * (1.0f - z);
            D[s * H + j] = (z > 0.0f && z < 1.0f) ? 0.2f * dz : 0.0f;
            L[s * R + F + j] = hp;
            L[(kTrainTile + s) * R + F + j] = hp;
            L[(2 * kTrainTile + s) * R + F + j] = r * hp;
        }
        stage_x(t, L, R);
        __syncthreads();
        float g = 0.0f;
        if (active) {
            for (int k = 0; k < H; ++k) g += D[(2 * kTrainTile + s) * H + k] * UT[(2 * H + k) * H + j];
            const float dr = g * hp;
            D[(kTrainTile + s) * H + j] = (r > 0.0f && r < 1.0f) ? 0.2f * dr : 0.0f;
        }
        __syncthreads();
        if (active) {
            float dn = delta * z + g * r;
            for (int k = 0; k < H; ++k)
                dn += D[s * H + k] * UT[k * H + j] + D[(kTrainTile + s) * H + k] * UT[(H + k) * H + j];
            delta = dn;
        }
#pragma unroll
        for (int i = 0; i < kTrainAcc; ++i) {
            if (lo[i] >= 0) {
                const float* lp = L + lo[i];
                const float* dp = D + dofs[i];
                float sum = acc[i];
                for (int s2 = 0; s2 < kTrainTile; ++s2) sum += lp[s2 * R] * dp[s2 * H];
                acc[i] = sum;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < kTrainAcc; ++i)
        if (lo[i] >= 0) part[tid + i * nt] = acc[i];
}

// The view of workgroup blockIdx.x: the per-network record is read here, once, and nowhere inside the timestep loops.
__device__ inline TrainView train_view(const TrainArgs& g, const int m) {
    const TrainModel& r = g.model[m];
    TrainView a;
    a.n = g.n; a.T = g.T; a.F = g.F; a.H = r.H;
    a.theta = g.theta + r.ofs;
    a.feats = g.feats; a.targets = g.targets; a.indices = g.indices;
    a.mask_mode = r.mask_mode; a.masks = g.masks; a.mask_key = r.mask_key;
    a.rate = r.rate; a.keep_scale = r.keep_scale;
    a.beta = r.beta; a.inv_n = g.inv_n;
    a.tape = g.tape + r.tape_ofs;
    a.partial = g.partial + r.partial_ofs;
    a.n_grad = g.backward ? train_n_params(g.F, r.H) : 0;
    a.probs = g.probs ? g.probs + (size_t)m * g.n : nullptr;
    return a;
}

// element e of the concatenated flat vector -> its network
__device__ inline int train_model_of(const TrainArgs& a, const int e) {
    int m = 0;
    while (m + 1 < a.n_models && e >= a.model[m + 1].ofs) ++m;
    return m;
}

// One thread per element of the concatenated gradient vector (backward launches), then one per network for its loss.
__device__ inline void train_reduce(const TrainArgs& a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_elem = a.backward ? a.n_total : 0;
    if (e < n_elem) {
        const int m = train_model_of(a, e);
        const TrainModel& r = a.model[m];
        const int le = e - r.ofs;
        const size_t stride = (size_t)train_n_params(a.F, r.H) + 2;
        const float* part = a.partial + r.partial_ofs + le;
        float sum = 0.0f;
        for (int b = 0; b < a.n_blocks; ++b) sum += part[b * stride];
        if (a.grads) a.grads[e] = sum;
        if (a.apply && !((r.frozen_mask >> (le < train_n_gru(a.F, r.H) ? 0 : 1)) & 1))
            train_rmsprop(a.theta[e], a.accum[e], sum, r.lr, r.rho, r.eps);
    } else if (e < n_elem + a.n_models) {
        const int m = e - n_elem;
        const TrainModel& r = a.model[m];
        const int n_grad = a.backward ? train_n_params(a.F, r.H) : 0;
        const size_t stride = (size_t)n_grad + 2;
        const float* part = a.partial + r.partial_ofs + n_grad;
        float la = 0.0f, lb = 0.0f;
        for (int b = 0; b < a.n_blocks; ++b) { la += part[b * stride]; lb += part[b * stride + 1]; }
        a.loss[m] = r.beta * (la * a.inv_n) + (1.0f - r.beta) * (lb * a.inv_n);
    }
}

__device__ inline void train_apply(const TrainArgs& a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_total) return;
    const TrainModel& r = a.model[train_model_of(a, e)];
    if (!((r.frozen_mask >> (e - r.ofs < train_n_gru(a.F, r.H) ? 0 : 1)) & 1))
        train_rmsprop(a.theta[e], a.accum[e], a.grads[e], r.lr, r.rho, r.eps);
}

// Keras binary_accuracy's numerator: one workgroup per network counts round-half-even(p) == y over the n samples, as integers.
constexpr int kTrainAccThreads = 256;
__device__ inline void train_accuracy(const TrainAccuracyArgs& a, int32_t* lds) {
    const float* p = a.probs + (size_t)blockIdx.x * a.n;
    int32_t hits = 0;
    for (int i = threadIdx.x; i < a.n; i += kTrainAccThreads) hits += rintf(p[i]) == a.targets[i] ? 1 : 0;
    lds[threadIdx.x] = hits;
    __syncthreads();
    for (int w = kTrainAccThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.hits[blockIdx.x] = lds[0];
}

#endif  // __HIPCC__

}  // namespace pe
