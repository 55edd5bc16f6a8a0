// C ABI of libprecise_engine.so (declared in include/precise_engine.h): host-side state,
// constant tables, weight packing and kernel sequencing for the MI355X wake-word hot path.
// The arithmetic lives in kernels.hip (mfcc_wave_device.h, gru_*_device.h); nothing here computes on the CPU
// beyond building constant tables once per engine.
#include "../../include/precise_engine.h"
#include "pe_common.h"
#include "gru_cw_pack.h"
#include "mfcc_general_device.h"
#include "gru_train_device.h"
#include "gru_train_wide_device.h"
#include "gru_train_stacked_device.h"
#include "mine_device.h"
#include "sample_device.h"
#include "generate_device.h"
#include "augment_device.h"
#include "stats_device.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pe;

namespace {

thread_local std::string g_global_error;

// pe_vectorize_clips / pe_score_clips work through their clips in passes of about this many bytes of audio (a pass always
// takes at least one clip); at most kClipPassRows window rows per pass bound the result buffers when the clips are tiny
constexpr int64_t kClipPassBytes = 256ll << 20;
constexpr int64_t kClipPassRows = 1ll << 21;

struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// One model's packed network, in every layout the engine's forms read (null where a form does not apply).  A weight field is
// named here and in model_net below (NetPack -> ModelNet, pe_common.h), nowhere else on the host.
struct NetPack {
    float dense_bias = 0.f;
    float* wxd = nullptr; float* wx = nullptr; float* wr1 = nullptr; float* wr2 = nullptr; float* bias = nullptr; float* wd = nullptr;
    float* cw_blob = nullptr;         // the stock width re-tiled (gru_cw_device.h)
    // wide / stacked network (units 64..256, 1-2 layers): weight streams in MFMA A-operand order; per layer: wx1, wr1, wx2, wr2, b1, b2
    float* wide_buf[2][6] = {{nullptr}}; float* wide_wd = nullptr;
    // the same network packed for gru_wide_x3_device.h (row i of tile tau = unit 16 tau + i; k-slot 8 gk + e = source unit 16 kappa + 4 gk + e)
    float* wide3_buf[2][6] = {{nullptr}}; float* wide3_wd = nullptr;
    // ... and with bf16 operands (gru_wide_bf16_device.h; gru_precision = 1): per layer the weight stream of phase 1 and of phase 2 as eight bf16 per lane, b1, b2 as float32(hi + lo)
    uint16_t* wideb_w[2][2] = {{nullptr}}; float* wideb_b[2][2] = {{nullptr}}; float* wideb_wd = nullptr;
    // bf16-operand network (pe_params.gru_precision = 1)
    uint16_t* wx_bf16 = nullptr; uint16_t* wr_bf16 = nullptr; float* wd_bf16 = nullptr;
    uint32_t* b20_blob = nullptr;     // the same network in the layout of gru_b20_device.h (<= 20 units, <= 14 features)
    // float32 network as three bf16 pieces per operand on the XDL pipe (gru_x3_device.h; tiling 2): packed for every
    // float32 network of <= 20 units and <= 15 inputs without delta features
    uint32_t* x3_blob = nullptr;
};
// one model's on-device ThresholdDecoder / TriggerDetector settings (pe_set_decoder[_model] / pe_set_trigger[_model])
struct DecState {
    double* cd = nullptr; int cd_len = 0, min_out = 0, out_range = 0; double center = 0.5;
    double threshold = 0.5; int level = 3, rearm = -8; bool on = false;
};

}  // namespace

struct pe_engine {
    pe_params prm{};
    int device = 0;
    int n_streams = 0, n_tiles = 0, n_padded = 0;
    int units = 0, n_in = 0, n_layers = 0;
    int ring_slots = 0;
    int mel_nnz = 0;
    std::string err;
    std::vector<void*> allocs;
    std::vector<size_t> alloc_bytes;         // bytes behind allocs[i] (dev_upload into an existing buffer checks them)
    int64_t device_bytes = 0;
    // streaming state: per stream two sides of (16-byte record, leftover PCM); a call that advances a stream reads its
    // current side and writes the other (pe_common.h: StreamRec) -- streams that take no part in a call are not touched
    StreamRec* rec = nullptr;                // [n_padded][2 sides]
    int16_t* carry = nullptr;                // [2][n_padded][carry_cap]
    // leftovers kept in place (pe_update_device_keep / pe_update_async): non-null = the chunks of the last call,
    // [n_streams][kept_chunk], still hold every stream's leftover and the carry was NOT written; any call of another style
    // first copies them into the carry (flush_kept).  call_head / call_keep: what the launches of the call being built take.
    const int16_t* kept = nullptr; int kept_chunk = 0;
    const int16_t* call_head = nullptr; int call_head_chunk = 0; bool call_keep = false;
    uint32_t call_no = 1;                    // number of the last call that wrote records (readers of later launches pass call_no + 1)
    uint32_t renumber_at = 0x7fff0000u;      // call number at which every record is renumbered and the count restarts (pe_set_renumber_at: tests)
    bool fused = true;      // MFCC || GRU in one launch when the chunk size allows it
    // carried window chains (gru_chain_device.h; pe_set_chain_carry).  The state is valid while chains_built_epoch ==
    // chain_epoch: every call that moves the streams' state or changes what a chain is made of bumps chain_epoch
    // (begin_state_call and the setters), and only a chain launch -- which moves the chains WITH the streams -- catches up.
    int chain_mode = 1;                      // 0 off, 1 automatic (after kChainEnterAfter eligible calls in a row), 2 eager
    float* chains = nullptr;                 // [n_tiles][kCwSlots][5][64], allocated at the first entry into chain mode
    uint32_t* chain_ke = nullptr;            // [n_padded]
    uint64_t chain_epoch = 1, chains_built_epoch = 0;
    int chain_streak = 0;                    // eligible update calls in a row so far, nothing else bumping the epoch in between
    uint64_t chain_seen_epoch = 0;           // the epoch as the last update call left it
    // chains no update will hand out are not advanced once a caller's chunk holds (do_update, kChainSkipAfter)
    int chain_run = 0, chain_run_chunk = 0;  // eligible update calls in a row with the same chunk, and that chunk
    int chain_skip_chunk = 0;                // the chunk the valid chains were last advanced for with skipping on; 0 = every live chain is current
    int gru_waves = 0;      // 0 = auto (4 waves per tile while tiles <= CUs, else 1), or forced 1 / 4
    // general front end (mfcc_general_device.h): any n_fft / n_filt / n_mfcc the stock-shape wave kernel has no tables for
    bool general = false;
    int row_floats = kRowFloats;   // floats per feature row: 32 when a frame has 17..32 coefficients
    int carry_cap = kCarryCap;     // int16 samples of leftover PCM kept per stream (>= frame length)
    GeneralTables gtab{};
    int gru_tiling = -1;    // -1 = auto (stock width re-tiled while tiles <= 2 CUs; XDL form above 4 tiles per CU), 0 = classic, 1 = re-tiled (gru_cw_device.h), 2 = XDL form (gru_x3_device.h)
    int n_cus = 256;        // compute units of the device (MI355X: 256)
    float* ring = nullptr;
    // input projections x.W + b of every frame beside its feature row (stock-width float32 network, <= kProjMaxTiles
    // tiles): written once by the MFCC stage, read by the network instead of 16 of its 41 MFMAs per timestep
    float* proj_ring = nullptr;
    bool proj_ok = false, proj_on = false;
    std::vector<float> proj_w_host, proj_b_host;
    // several updates per call (pe_reserve_updates / pe_update_many*)
    int max_updates = 1;
    uint32_t* ke_hist = nullptr;
    // constant tables of the MFCC frame kernel, laid out as they sit in LDS (mfcc_wave_tables.h)
    unsigned char* table_blob = nullptr;
    pe_wave::Layout table_layout{};
    // the networks of the engine (pe_create: one; pe_create_models: K on the same streams), each with its own decoder and
    // trigger settings: nets[m] / dec[m] for model m, both of size n_models; `activation` is [n_models][n_padded]
    int n_models = 1;
    std::vector<NetPack> nets;
    std::vector<DecState> dec;
    bool wide = false;      // wide / stacked network (units 64..256, 1-2 layers)
    int wide_kx4[2] = {1, 1};
    // the architecture as pe_create was given it (pe_set_weights takes the same widths only) and the width the streamed-weight
    // kernel runs at
    int layer_units[2] = {0, 0}, layer_n_in[2] = {0, 0}, wide_units = 0;
    std::vector<double> mel_host;            // the filterbank pe_create was given: pe_set_weights rebuilds the table blob's projection rows
    int32_t* activation = nullptr;
    // staging for the host entry points (grown on demand)
    DeviceBuf st_pcm, st_out, st_feats, st_mask, st_audio, st_mfcc, st_conf, st_fired, st_ids;
    DeviceBuf st_clips;                     // pe_vectorize_clips / pe_score_clips: the clip table of a pass
    // pe_evaluate_clips / pe_simulate_*: the tables of a pass, its padded predictions, the call's thresholds + histogram +
    // metrics, a pass's mask words + partial sums
    DeviceBuf st_recs, st_pred, st_sim, st_simw;
    DeviceBuf st_stats;                     // pe_stats_scores / pe_test_clips: the scratch of a call (StatsScratch)
    int64_t clip_pass_bytes = kClipPassBytes;  // audio bytes a pass of those entry points stages (pe_set_clip_pass_bytes: tests)
    std::vector<uint8_t> seen_ids;          // pe_update_subset: duplicate check of the host entry point
    // timing
    bool timing = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool ev_valid = false, ev_has_gru = false;
    // host-fed pipeline (pe_update_async / pe_update_subset_async / pe_wait): a ring of kAsyncDepth updates in flight, each with its own device
    // buffers and pinned staging; the chunk of update u + 1 crosses PCIe (copy stream) while update u runs (compute stream)
    static constexpr int kAsyncDepth = 3;
    struct AsyncSlot {
        // what an update hands back: raw outputs, and from pe_update_subset_async decoded confidence and activations
        struct Out {
            DeviceBuf dev;
            void* pin = nullptr; size_t pin_bytes = 0;          // pinned landing zone for callers whose array is pageable
            void* user = nullptr; size_t bytes = 0;             // this update: where it goes (null: not asked for)
            bool direct = false;                                // ... and whether the DMA writes there itself
        } out[3];                                               // raw, conf, fired
        DeviceBuf dev_in, dev_ids;                              // the chunks and (subset updates) the stream ids of this update
        void* pin_ids = nullptr; size_t pin_ids_bytes = 0;      // the ids as the call found them: the DMA reads them from here
        hipEvent_t copied = nullptr, done = nullptr;
        bool busy = false;
    } aslot[kAsyncDepth];
    hipStream_t s_copy = nullptr, s_compute = nullptr;
    // the stream of the last *_device call that moved the streams' state: pe_update_async runs on the engine's own
    // (non-blocking) streams, which nothing orders behind that work -- not even the NULL stream -- so it waits for it
    // by event, lazily (recorded only when the caller switches styles: the *_device loop itself pays nothing)
    hipStream_t last_user_stream = nullptr;
    bool user_dirty = false;
    hipEvent_t ev_user = nullptr;
    unsigned async_next = 0;
    int async_inflight = 0;
    std::vector<std::pair<char*, size_t>> pinned;               // pe_host_alloc'ed ranges (zero-copy sources / destinations)
};

namespace {

int fail(pe_engine* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf; else g_global_error = buf;
    return code;
}

#define PE_HIP(e, call)                                                                      \
    do {                                                                                     \
        hipError_t _err = (call);                                                            \
        if (_err != hipSuccess)                                                              \
            return fail((e), PE_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_err), \
                        __FILE__, __LINE__);                                                 \
    } while (0)

int drain_async(pe_engine* e);
// every entry point that reads or moves the streams' state first lets the updates of pe_update_async finish (they run on the
// engine's own streams, which no other entry point is ordered against)
#define PE_DRAIN(e) do { int _drc = drain_async(e); if (_drc) return _drc; } while (0)

template <class T>
int dev_alloc(pe_engine* e, T** out, size_t count) {
    void* p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t err = hipMalloc(&p, bytes);
    if (err != hipSuccess) return fail(e, PE_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    e->allocs.push_back(p);
    e->alloc_bytes.push_back(bytes);
    e->device_bytes += (int64_t)bytes;
    *out = static_cast<T*>(p);
    return PE_OK;
}

// *out null: allocate, then copy.  *out set (pe_set_weights packing a network of the same widths again): the buffer
// pe_create made for this very vector is written in place -- it must be one of the engine's and hold exactly this many bytes.
template <class T>
int dev_upload(pe_engine* e, T** out, const std::vector<T>& host) {
    if (!*out) {
        int rc = dev_alloc(e, out, host.size());
        if (rc) return rc;
    } else {
        const size_t bytes = (host.size() ? host.size() : 1) * sizeof(T);
        size_t i = 0;
        while (i < e->allocs.size() && e->allocs[i] != static_cast<void*>(*out)) ++i;
        if (i == e->allocs.size() || e->alloc_bytes[i] != bytes)
            return fail(e, PE_ERR_INVALID, "repacking %zu bytes into a buffer of %zu", bytes, i == e->allocs.size() ? (size_t)0 : e->alloc_bytes[i]);
    }
    if (!host.empty()) PE_HIP(e, hipMemcpy(*out, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return PE_OK;
}

// release one dev_alloc'ed buffer before pe_destroy (tables that are replaced: decoder LUT, ring, ke_hist)
void dev_free(pe_engine* e, void* p, size_t bytes) {
    if (!p) return;
    for (size_t i = 0; i < e->allocs.size(); ++i)
        if (e->allocs[i] == p) { e->allocs.erase(e->allocs.begin() + i); e->alloc_bytes.erase(e->alloc_bytes.begin() + i); break; }
    (void)hipFree(p);
    e->device_bytes -= (int64_t)bytes;
}

int ensure(pe_engine* e, DeviceBuf& b, size_t bytes) {
    if (b.bytes >= bytes) return PE_OK;
    if (b.p) { (void)hipFree(b.p); e->device_bytes -= (int64_t)b.bytes; b.p = nullptr; b.bytes = 0; }
    hipError_t err = hipMalloc(&b.p, bytes);
    if (err != hipSuccess) return fail(e, PE_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    b.bytes = bytes;
    e->device_bytes += (int64_t)bytes;
    return PE_OK;
}

int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// floats of HBM behind the feature ring: 16 floats per row, or 16 bf16 (half of it) with ring_precision = 1
size_t ring_floats(const pe_engine* e) {
    const size_t rows = (size_t)e->n_tiles * e->ring_slots * kTileStreams;
    return e->prm.ring_precision == 1 ? rows * kRowFloats / 2 : rows * (size_t)e->row_floats;
}

// The front end's precision (pe_params::mfcc_precision: 0 float64, 1 float32) as a type: f(R{}) with R = double or float, and what
// f returns.  The ONE place where the parameter becomes a type: table builders and front-end launches are written once, in R.
template <class F>
auto with_real(const pe_params& prm, F&& f) { return prm.mfcc_precision == 0 ? f(double{}) : f(float{}); }

template <class R>
int build_tables(pe_engine* e, const double* mel_filters) {
    std::vector<unsigned char> blob;
    const std::string err = pe_wave::build<R>(mel_filters, e->prm.n_filt, e->prm.n_mfcc, blob, e->table_layout,
                                              e->proj_ok ? e->proj_w_host.data() : nullptr, e->proj_ok ? e->proj_b_host.data() : nullptr);
    if (!err.empty()) return fail(e, PE_ERR_UNSUPPORTED, "%s", err.c_str());
    return dev_upload(e, &e->table_blob, blob);
}

// Tables of the general front end: twiddles of the packed real FFT, the filterbank as CSR, the DCT-II (ortho) matrix.
template <class R>
int build_general_tables(pe_engine* e, const double* mel_filters) {
    const int N = e->prm.n_fft, bins = N / 2 + 1, nf = e->prm.n_filt, nc = e->prm.n_mfcc;
    const long double PI = 3.14159265358979323846264338327950288L;
    const bool pow2 = general_is_pow2(N);
    // power of two: packed real transform of M = N / 2 points;  otherwise Bluestein over L = 2^log2m >= 2 N - 1 points
    const int log2m_blue = general_blue_log2(N);
    const int M = pow2 ? N / 2 : (1 << log2m_blue);           // length of the complex radix-2 transform in LDS
    std::vector<R> tw((size_t)M), wn((size_t)(pow2 ? (M / 2 + 1) * 2 : 2));       // tw: M / 2 complex = M reals
    for (int k = 0; k < M / 2; ++k) {
        tw[2 * k] = (R)cosl(-2.0L * PI * k / M);
        tw[2 * k + 1] = (R)sinl(-2.0L * PI * k / M);
    }
    if (pow2)
        for (int k = 0; k <= M / 2; ++k) {
            wn[2 * k] = (R)cosl(-2.0L * PI * k / N);
            wn[2 * k + 1] = (R)sinl(-2.0L * PI * k / N);
        }
    std::vector<R> chirp, bhat;
    if (!pow2) {
        // w[n] = exp(-i pi n^2 / N): the angle from n^2 mod 2 N (exact integers), so large n lose nothing
        auto wl = [&](long long n, long double& re, long double& im) {
            const long long r = (n * n) % (2LL * N);
            const long double a = -PI * (long double)r / (long double)N;
            re = cosl(a); im = sinl(a);
        };
        chirp.resize((size_t)2 * N);
        for (int n = 0; n < N; ++n) { long double re, im; wl(n, re, im); chirp[2 * n] = (R)re; chirp[2 * n + 1] = (R)im; }
        // b[m mod L] = conj(w[m]) for |m| < N, zero elsewhere; B = DFT_L(b) (direct, long double, roots from an exact table)
        const int L = M;
        std::vector<long double> br((size_t)L, 0.0L), bi((size_t)L, 0.0L), cr((size_t)L), ci((size_t)L);
        for (int m = -(N - 1); m <= N - 1; ++m) { long double re, im; wl(m, re, im); br[(m + L) % L] = re; bi[(m + L) % L] = -im; }
        for (int j = 0; j < L; ++j) { cr[j] = cosl(-2.0L * PI * j / L); ci[j] = sinl(-2.0L * PI * j / L); }
        bhat.resize((size_t)2 * L);
        int bits = 0;
        while ((1 << bits) < L) ++bits;
        for (int k = 0; k < L; ++k) {
            long double sr = 0.0L, si = 0.0L;
            for (int m = 0; m < L; ++m) {
                if (br[m] == 0.0L && bi[m] == 0.0L) continue;
                const int j = (int)(((long long)k * m) % L);
                sr += br[m] * cr[j] - bi[m] * ci[j];
                si += br[m] * ci[j] + bi[m] * cr[j];
            }
            unsigned rev = 0;
            for (int b = 0; b < bits; ++b) rev |= ((unsigned)(k >> b) & 1u) << (bits - 1 - b);
            bhat[2 * (size_t)rev] = (R)(sr / L);               // bit-reversed position, 1 / L of the inverse transform folded in
            bhat[2 * (size_t)rev + 1] = (R)(si / L);
        }
    }
    // filterbank as lane runs (mfcc_general_device.h: GeneralTables): every filter's non-zeros, in bin order, in runs of
    // <= kGeneralRun entries; run r <-> lane r % 64 of round r / 64
    std::vector<int> run_ptr(nf + 1, 0);
    std::vector<std::pair<int, R>> entries;
    std::vector<int> run_first;            // first entry of every run
    std::vector<int> run_len;
    for (int f = 0; f < nf; ++f) {
        int in_run = 0;
        for (int k = 0; k < bins; ++k) {
            const double v = mel_filters[(size_t)f * bins + k];
            if (v == 0.0) continue;
            if (in_run == 0) { run_first.push_back((int)entries.size()); run_len.push_back(0); }
            entries.emplace_back(k, (R)v);
            ++run_len.back();
            if (++in_run == kGeneralRun) in_run = 0;
        }
        run_ptr[f + 1] = (int)run_first.size();
    }
    const int n_runs = (int)run_first.size();
    const int n_rounds = n_runs > 0 ? (n_runs + 63) / 64 : 1;
    std::vector<R> run_w((size_t)n_rounds * kGeneralRun * 64, R(0));
    std::vector<int> run_bin((size_t)n_rounds * kGeneralRun * 64, 0);
    for (int r = 0; r < n_runs; ++r)
        for (int i = 0; i < run_len[r]; ++i) {
            const size_t at = ((size_t)(r / 64) * kGeneralRun + i) * 64 + (r % 64);
            run_bin[at] = entries[run_first[r] + i].first;
            run_w[at] = entries[run_first[r] + i].second;
        }
    std::vector<R> dct_t((size_t)nf * kGeneralDctCols, R(0));
    for (int c = 0; c < nc; ++c)           // scipy.fftpack.dct(type 2, norm='ortho'): y[c] = 2 f(c) sum_n x[n] cos(pi c (2 n + 1) / (2 N))
        for (int f = 0; f < nf; ++f) {
            const long double scale = c == 0 ? sqrtl(1.0L / (4.0L * nf)) : sqrtl(1.0L / (2.0L * nf));
            dct_t[(size_t)f * kGeneralDctCols + c] = (R)(2.0L * scale * cosl(PI * c * (2 * f + 1) / (2.0L * nf)));
        }
    R* d_tw = nullptr; R* d_wn = nullptr; R* d_w = nullptr; R* d_dct = nullptr; int* d_ptr = nullptr; int* d_bin = nullptr;
    int rc;
    if ((rc = dev_upload(e, &d_tw, tw))) return rc;
    if ((rc = dev_upload(e, &d_wn, wn))) return rc;
    if ((rc = dev_upload(e, &d_w, run_w))) return rc;
    if ((rc = dev_upload(e, &d_dct, dct_t))) return rc;
    if ((rc = dev_upload(e, &d_ptr, run_ptr))) return rc;
    if ((rc = dev_upload(e, &d_bin, run_bin))) return rc;
    int log2m = 0;
    while ((1 << log2m) < M) ++log2m;
    R* d_chirp = nullptr; R* d_bhat = nullptr;
    if (!pow2) {
        if ((rc = dev_upload(e, &d_chirp, chirp))) return rc;
        if ((rc = dev_upload(e, &d_bhat, bhat))) return rc;
    }
    e->gtab = GeneralTables{d_tw, d_wn, d_w, d_bin, d_ptr, d_dct, N, log2m, nf, nc, e->prm.vectorizer == 3 ? 1 : 0, n_rounds, d_chirp, d_bhat};
    return PE_OK;
}

// Arrange the Keras matrices as MFMA A-operands (see the layout comment in gru_kernels.hip).
int pack_gru_weights(pe_engine* e, NetPack& n, const pe_gru_layer& L, const float* dense_kernel) {
    const int H = L.units, F = e->n_in;          // F = base features; with use_delta the kernel has 2F rows
    const bool delta = e->prm.use_delta != 0;
    const int R = gru_small_regs(H), NT = gru_small_tiles(H);
    const int KX = e->row_floats / kRowFloats;      // 16-feature groups of a feature row (2: 17..32 coefficients per frame)
    std::vector<float> wx((size_t)KX * NT * 4 * 64, 0.f), wxd((size_t)NT * 4 * 64, 0.f), wr1((size_t)NT * R * 64, 0.f), wr2((size_t)NT * R * 64, 0.f);
    std::vector<float> bias((size_t)NT * 4 * 64, 0.f), wd((size_t)R * 64, 0.f);
    for (int tile = 0; tile < NT; ++tile)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 15, g = lane >> 4;
            {   // A operand: row i of the tile, k-slot g
                const int reg = i & 3, gout = i >> 2;
                const int slot = 4 * tile + reg;
                const int gate = slot / R, rho = slot % R, u = 4 * rho + gout;
                if (slot < 3 * R && u < H) {
                    const int col = gate * H + u;
                    for (int kx = 0; kx < KX; ++kx)
                        for (int kk = 0; kk < 4; ++kk) {
                            const int phi = 16 * kx + 4 * g + kk;
                            if (phi < F) wx[(((size_t)kx * NT + tile) * 4 + kk) * 64 + lane] = L.kernel[(size_t)phi * 3 * H + col];
                            if (kx == 0 && phi < F && delta) wxd[((size_t)tile * 4 + kk) * 64 + lane] = L.kernel[(size_t)(F + phi) * 3 * H + col];
                        }
                    for (int rs = 0; rs < R; ++rs) {
                        const int usrc = 4 * rs + g;
                        if (usrc >= H) continue;
                        const float w = L.recurrent_kernel[(size_t)usrc * 3 * H + col];
                        (gate < 2 ? wr1 : wr2)[((size_t)tile * R + rs) * 64 + lane] = w;
                    }
                }
            }
            for (int q = 0; q < 4; ++q) {   // C operand: this lane's output rows 4g + q
                const int slot = 4 * tile + q;
                const int gate = slot / R, rho = slot % R, u = 4 * rho + g;
                if (slot < 3 * R && u < H) bias[((size_t)tile * 4 + q) * 64 + lane] = L.bias[gate * H + u];
            }
        }
    for (int rho = 0; rho < R; ++rho)
        for (int lane = 0; lane < 64; ++lane) {
            const int u = 4 * rho + (lane >> 4);
            if (u < H) wd[(size_t)rho * 64 + lane] = dense_kernel[u];
        }
    int rc;
    if ((rc = dev_upload(e, &n.wx, wx))) return rc;
    if ((rc = dev_upload(e, &n.wxd, wxd))) return rc;
    if ((rc = dev_upload(e, &n.wr1, wr1))) return rc;
    if ((rc = dev_upload(e, &n.wr2, wr2))) return rc;
    if ((rc = dev_upload(e, &n.bias, bias))) return rc;
    if ((rc = dev_upload(e, &n.wd, wd))) return rc;
    if (R == 5 && KX == 1) {                    // the stock width also in its re-tiled form (gru_cw_device.h)
        const std::vector<float> blob = pack_gru_cw(L.kernel, L.recurrent_kernel, L.bias, F, H, delta);
        if ((rc = dev_upload(e, &n.cw_blob, blob))) return rc;
    }
    return PE_OK;
}

// The input-projection rows of the network (mfcc_wave_device.h epilogue; the engine's only model: pe_set_input_projection
// refuses K > 1), in the slot order of pack_gru_weights: element o = 16 g + 4 tile + q of a row is accumulator q of output
// tile `tile` in lane group g, i.e. slot 4 tile + q, unit 4 rho + g
void pack_projection_rows(pe_engine* e, const pe_gru_layer& L) {
    const int H = L.units, F = e->n_in, R = gru_small_regs(H), NT = gru_small_tiles(H);
    if (NT > 4 || e->prm.use_delta || e->row_floats != kRowFloats) return;
    e->proj_w_host.assign((size_t)F * kProjRow, 0.f);
    e->proj_b_host.assign(kProjRow, 0.f);
    for (int o = 0; o < kProjRow; ++o) {
        const int g = o >> 4, tile = (o >> 2) & 3, q = o & 3;
        const int slot = 4 * tile + q;
        const int gate = slot / R, rho = slot % R, u = 4 * rho + g;
        if (tile >= NT || slot >= 3 * R || u >= H) continue;
        const int col = gate * H + u;
        e->proj_b_host[o] = L.bias[col];
        for (int c = 0; c < F; ++c) e->proj_w_host[(size_t)c * kProjRow + o] = L.kernel[(size_t)c * 3 * H + col];
    }
}

// bf16 network operands (gru_bf16_device.h): unit u = 8 g + i; tile (gate, t): row 4 gout + q <-> unit
// 8 gout + 4 t + q; A operand of lane (row i, k-group g) = 8 consecutive k (features / source units).
uint16_t to_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);     // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                                 // round to nearest even
    return (uint16_t)(u >> 16);
}

int pack_gru_weights_bf16(pe_engine* e, NetPack& n, const pe_gru_layer& L, const float* dense_kernel) {
    // with use_delta the layer has 2 F inputs: features in k = 0..15, their first differences in k = 16..31
    const bool delta = e->prm.use_delta != 0;
    const int H = L.units, F = delta ? L.n_in / 2 : L.n_in;
    if (delta && F > 14) return fail(e, PE_ERR_UNSUPPORTED, "bf16 network with use_delta takes n_mfcc <= 14 (k slots 30, 31 of the input contraction carry the biases)");
    std::vector<uint16_t> wx((size_t)6 * 64 * 8, 0), wr((size_t)6 * 64 * 8, 0);
    std::vector<float> wd((size_t)8 * 64, 0.f);
    for (int tl = 0; tl < 6; ++tl) {
        const int gate = tl >> 1, t = tl & 1;
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 15, g = lane >> 4;
            const int gout = i >> 2, reg = i & 3;
            const int u = 8 * gout + 4 * t + reg;                    // A row i of this tile
            if (u < H) {
                const int col = gate * H + u;
                for (int ek = 0; ek < 8; ++ek) {
                    const int k = 8 * g + ek;
                    if (k < F) wx[((size_t)tl * 64 + lane) * 8 + ek] = to_bf16(L.kernel[(size_t)k * 3 * H + col]);
                    if (delta && k >= 16 && k - 16 < F) wx[((size_t)tl * 64 + lane) * 8 + ek] = to_bf16(L.kernel[(size_t)(F + k - 16) * 3 * H + col]);
                    if (k < H) wr[((size_t)tl * 64 + lane) * 8 + ek] = to_bf16(L.recurrent_kernel[(size_t)k * 3 * H + col]);
                }
                if (g == 3) {                                        // k = 30, 31: the bias as hi + lo against x = 1.0
                    const float b = L.bias[col];
                    const uint16_t hi = to_bf16(b);
                    uint32_t hb = (uint32_t)hi << 16;
                    float hif;
                    std::memcpy(&hif, &hb, 4);
                    wx[((size_t)tl * 64 + lane) * 8 + 6] = hi;
                    wx[((size_t)tl * 64 + lane) * 8 + 7] = to_bf16(b - hif);
                }
            }
        }
    }
    for (int i = 0; i < 8; ++i)
        for (int lane = 0; lane < 64; ++lane) {
            const int u = 8 * (lane >> 4) + i;
            if (u < H) wd[(size_t)i * 64 + lane] = dense_kernel[u];
        }
    int rc;
    if ((rc = dev_upload(e, &n.wx_bf16, wx))) return rc;
    if ((rc = dev_upload(e, &n.wr_bf16, wr))) return rc;
    if ((rc = dev_upload(e, &n.wd_bf16, wd))) return rc;
    return PE_OK;
}

// Float32 network on the XDL pipe (gru_x3_device.h): every weight as three bf16 pieces (round to nearest even of the
// running remainder; hi + mid + lo == the float32 weight exactly), arranged as the A operands of
// v_mfma_f32_16x16x32_bf16: lane (row i = lane & 15, k-group gk = lane >> 4) holds k = 8 gk .. 8 gk + 7.
// Output tiles 0..2 = z / r / candidate of units 0..15 (row i <-> unit i), tile 3 row 4 g + q = gate q of unit 16 + g.
// k-group gk carries the source units 4 gk .. 4 gk + 3 (operands 0..2) and 16 + gk (operand 3) -- the units whose
// values lane group gk owns -- and, on the input side, features 4 gk .. 4 gk + 3 with the bias as pseudo-feature F.
void split3_bf16(float v, uint16_t (&piece)[3]) {
    for (int i = 0; i < 3; ++i) {
        piece[i] = to_bf16(v);
        const uint32_t b = (uint32_t)piece[i] << 16;
        float f;
        std::memcpy(&f, &b, 4);
        v -= f;                      // exact
    }
}

// (<= 20 units, <= 15 inputs, no use_delta: the caller checks x3_eligible)
bool x3_eligible(const pe_params& p, const pe_gru_layer& L) { return p.gru_precision == 0 && !p.use_delta && L.units <= 20 && L.n_in <= 15 && p.n_mfcc <= kRowFloats; }

int pack_gru_weights_x3(pe_engine* e, NetPack& n, const pe_gru_layer& L, const float* dense_kernel) {
    const int H = L.units, F = L.n_in;
    std::vector<uint32_t> blob((size_t)kX3BlobBytes / 4, 0u);
    uint16_t* const half = reinterpret_cast<uint16_t*>(blob.data());
    auto gate_col = [&](int tile, int i, int* col) -> bool {     // A row i of an output tile -> column of the Keras matrices
        int gate, unit;
        if (tile < 3) { gate = tile; unit = i; }
        else { gate = i & 3; unit = 16 + (i >> 2); if (gate == 3) return false; }
        if (unit >= H) return false;
        *col = gate * H + unit;
        return true;
    };
    static const int kPiece3[8] = {0, 0, 1, 1, 0, 2, -1, -1};     // operand 3: [hi, hi, mid, mid, hi, lo, -, -]
    for (int tile = 0; tile < kX3Tiles; ++tile)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 15, gk = lane >> 4;
            int col;
            if (!gate_col(tile, i, &col)) continue;
            for (int m = 0; m < kX3RecOps; ++m)
                for (int ek = 0; ek < 8; ++ek) {
                    const int src = m < 3 ? 4 * gk + (ek & 3) : 16 + gk;
                    const int piece = m == 0 ? 0 : m == 1 ? 1 : m == 2 ? (ek < 4 ? 0 : 2) : kPiece3[ek];
                    if (src >= H || piece < 0) continue;
                    uint16_t pc[3];
                    split3_bf16(L.recurrent_kernel[(size_t)src * 3 * H + col], pc);
                    half[((size_t)(kX3ArOff + (tile * kX3RecOps + m) * 64 + lane)) * 8 + ek] = pc[piece];
                }
            for (int m = 0; m < kX3InOps; ++m)
                for (int ek = 0; ek < 8; ++ek) {
                    const int f = 4 * gk + (ek & 3);
                    const int piece = m == 0 ? 0 : m == 1 ? 1 : (ek < 4 ? 0 : 2);
                    if (f > F) continue;
                    uint16_t pc[3];
                    split3_bf16(f < F ? L.kernel[(size_t)f * 3 * H + col] : L.bias[col], pc);
                    half[((size_t)(kX3AxOff + (tile * kX3InOps + m) * 64 + lane)) * 8 + ek] = pc[piece];
                }
        }
    float* const wd = reinterpret_cast<float*>(blob.data()) + (size_t)kX3WdOff * 4;
    for (int o = 0; o < 5; ++o)
        for (int lane = 0; lane < 64; ++lane) {
            const int u = o < 4 ? 4 * (lane >> 4) + o : 16 + (lane >> 4);
            if (u < H) wd[o * 64 + lane] = dense_kernel[u];
        }
    return dev_upload(e, &n.x3_blob, blob);
}

// bf16 network of <= 20 units in the five-values-per-lane layout (gru_b20_device.h): output tiles 0..2 = z / r / candidate
// of units 0..15 (row i <-> unit i), tile 3 row 4 g + q = gate q of unit 16 + g; recurrent k-slot 8 gk + e <-> source unit
// 4 gk + e (e < 4) / 16 + gk (e = 4); input k-slot 8 gk + e <-> feature 4 gk + e (e < 4; pseudo-features F, F + 1 = bias hi,
// lo), and 8 gk + 4 + e <-> the first difference of that feature (use_delta: kernel rows F .. 2 F - 1).
bool b20_eligible(const pe_params& p, const pe_gru_layer& L) {
    const int F = p.use_delta ? L.n_in / 2 : L.n_in;
    return p.gru_precision == 1 && L.units <= 20 && F <= 14 && p.n_mfcc <= kRowFloats;
}

int pack_gru_weights_b20(pe_engine* e, NetPack& n, const pe_gru_layer& L, const float* dense_kernel) {
    const bool delta = e->prm.use_delta != 0;
    const int H = L.units, F = delta ? L.n_in / 2 : L.n_in;
    std::vector<uint32_t> blob((size_t)kB20BlobBytes / 4, 0u);
    uint16_t* const half = reinterpret_cast<uint16_t*>(blob.data());
    for (int tile = 0; tile < kB20Tiles; ++tile)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 15, gk = lane >> 4;
            int gate, unit;
            if (tile < 3) { gate = tile; unit = i; }
            else { gate = i & 3; unit = 16 + (i >> 2); if (gate == 3) continue; }
            if (unit >= H) continue;
            const int col = gate * H + unit;
            for (int ek = 0; ek < 5; ++ek) {
                const int src = ek < 4 ? 4 * gk + ek : 16 + gk;
                if (src < H) half[((size_t)(kB20ArOff + tile * 64 + lane)) * 8 + ek] = to_bf16(L.recurrent_kernel[(size_t)src * 3 * H + col]);
            }
            for (int ek = 0; ek < 8; ++ek) {
                const int f = 4 * gk + (ek & 3);
                uint16_t v = 0;
                if (ek < 4) {
                    if (f < F) v = to_bf16(L.kernel[(size_t)f * 3 * H + col]);
                    else if (f == F || f == F + 1) {
                        const float b = L.bias[col];
                        const uint16_t hi = to_bf16(b);
                        const uint32_t hb = (uint32_t)hi << 16;
                        float hif;
                        std::memcpy(&hif, &hb, 4);
                        v = f == F ? hi : to_bf16(b - hif);
                    }
                } else if (delta && f < F) v = to_bf16(L.kernel[(size_t)(F + f) * 3 * H + col]);
                half[((size_t)(kB20AxOff + tile * 64 + lane)) * 8 + ek] = v;
            }
        }
    float* const wd = reinterpret_cast<float*>(blob.data()) + (size_t)kB20WdOff * 4;
    for (int o = 0; o < 5; ++o)
        for (int lane = 0; lane < 64; ++lane) {
            const int u = o < 4 ? 4 * (lane >> 4) + o : 16 + (lane >> 4);
            if (u < H) wd[o * 64 + lane] = dense_kernel[u];
        }
    return dev_upload(e, &n.b20_blob, blob);
}

// The layer-0 input of the float32 wide networks (gru_wide_device.h WideInput): one k-group of 16 inputs, or two -- with
// use_delta (inputs [x, x_t - x_(t-1)], 2 n_mfcc <= 32 kernel rows) and with 17..32 coefficients per frame (32-float rows).
int wide_input_groups(const pe_engine* e) { return (e->prm.use_delta || e->prm.n_mfcc > kRowFloats) ? 2 : 1; }
// kernel row of input phi (0..15) of k-group `group`; a row >= the layer's n_in has no weight (zero in the stream)
int wide_input_row(const pe_engine* e, int group, int phi) {
    if (group == 0) return e->prm.use_delta && phi >= e->prm.n_mfcc ? 1 << 30 : phi;      // (delta: rows F .. belong to group 2)
    if (e->prm.use_delta) return phi < e->prm.n_mfcc ? e->prm.n_mfcc + phi : 1 << 30;      // the first difference of feature phi
    return kRowFloats + phi;                                                               // feature 16 + phi of a 32-float row
}

// Wide / stacked network (gru_wide_device.h): wave w owns output tiles tau = w TPW + t of every gate;
// row i of a tile <-> unit 16 tau + 4 (i & 3) + (i >> 2); k-step rho, k-slot gk <-> source unit 4 rho + gk
// (layer 0 input: k-step 4 group + kk <-> input 4 gk + kk of the k-group, wide_input_row).  Streams: [wave][k-group][tile][lane] float4.
int pack_gru_weights_wide(pe_engine* e, NetPack& n, const pe_weights* w) {
    const int H = w->layers[0].units, WV = gru_wide_waves(H), TPW = H / (16 * WV), H16 = H / 16;
    for (int l = 0; l < w->n_layers; ++l) {
        const pe_gru_layer& L = w->layers[l];
        const int kx4 = l == 0 ? wide_input_groups(e) : H16;
        const int F = L.n_in;
        e->wide_kx4[l] = kx4;
        auto in_weight = [&](int rho, int gk, int col) -> float {      // input part, k-step rho, k-slot gk
            if (l == 0) { const int row = wide_input_row(e, rho >> 2, 4 * gk + (rho & 3)); return row < F ? L.kernel[(size_t)row * 3 * H + col] : 0.f; }
            return L.kernel[(size_t)(4 * rho + gk) * 3 * H + col];
        };
        for (int phase = 0; phase < 2; ++phase) {
            const int NT = phase == 0 ? 2 * TPW : TPW;
            std::vector<float> wx((size_t)WV * kx4 * NT * 64 * 4, 0.f), wr((size_t)WV * H16 * NT * 64 * 4, 0.f);
            std::vector<float> bias((size_t)WV * NT * 4 * 64, 0.f);
            for (int wv = 0; wv < WV; ++wv)
                for (int tl = 0; tl < NT; ++tl) {
                    const int gate = phase == 0 ? (tl < TPW ? 0 : 1) : 2;
                    const int tau = wv * TPW + (tl % TPW);
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 15, gk = lane >> 4;
                        const int col = gate * H + 16 * tau + 4 * (i & 3) + (i >> 2);
                        for (int r4 = 0; r4 < kx4; ++r4)
                            for (int q = 0; q < 4; ++q)
                                wx[((((size_t)wv * kx4 + r4) * NT + tl) * 64 + lane) * 4 + q] = in_weight(4 * r4 + q, gk, col);
                        for (int r4 = 0; r4 < H16; ++r4)
                            for (int q = 0; q < 4; ++q)
                                wr[((((size_t)wv * H16 + r4) * NT + tl) * 64 + lane) * 4 + q] =
                                    L.recurrent_kernel[(size_t)(4 * (4 * r4 + q) + gk) * 3 * H + col];
                        for (int q = 0; q < 4; ++q)      // C operand: this lane's output rows 4 gk + q
                            bias[(((size_t)wv * NT + tl) * 4 + q) * 64 + lane] = L.bias[gate * H + 16 * tau + 4 * q + gk];
                    }
                }
            int rc;
            if ((rc = dev_upload(e, &n.wide_buf[l][phase == 0 ? 0 : 2], wx))) return rc;
            if ((rc = dev_upload(e, &n.wide_buf[l][phase == 0 ? 1 : 3], wr))) return rc;
            if ((rc = dev_upload(e, &n.wide_buf[l][phase == 0 ? 4 : 5], bias))) return rc;
        }
    }
    std::vector<float> wd((size_t)WV * TPW * 4 * 64, 0.f);
    for (int wv = 0; wv < WV; ++wv)
        for (int tp = 0; tp < TPW; ++tp)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    wd[(((size_t)wv * TPW + tp) * 4 + q) * 64 + lane] = w->dense_kernel[16 * (wv * TPW + tp) + 4 * q + (lane >> 4)];
    return dev_upload(e, &n.wide_wd, wd);
}

// The same network for gru_wide_x3_device.h: float32 weights (split into bf16 pieces in registers, every timestep), wave w
// owns output tiles tau = w TPW + t of every gate; row i of a tile <-> unit 16 tau + i; k-group kappa, lane (row i, k-group
// slot gk) <-> source units 16 kappa + 4 gk + e, e = 0..3 (layer 0: input 4 gk + e of k-group kappa, wide_input_row).  Streams: [wave][kappa][tile][lane] float4.
int pack_gru_weights_wide_x3(pe_engine* e, NetPack& n, const pe_weights* w) {
    const int H = w->layers[0].units, WV = 4, TPW = H / (16 * WV), H16 = H / 16;
    for (int l = 0; l < w->n_layers; ++l) {
        const pe_gru_layer& L = w->layers[l];
        const int kin = l == 0 ? wide_input_groups(e) : H16;
        const int F = L.n_in;
        for (int phase = 0; phase < 2; ++phase) {
            const int NT = phase == 0 ? 2 * TPW : TPW;
            std::vector<float> wx((size_t)WV * kin * NT * 64 * 4, 0.f), wr((size_t)WV * H16 * NT * 64 * 4, 0.f);
            std::vector<float> bias((size_t)WV * NT * 4 * 64, 0.f);
            for (int wv = 0; wv < WV; ++wv)
                for (int tl = 0; tl < NT; ++tl) {
                    const int gate = phase == 0 ? (tl < TPW ? 0 : 1) : 2;
                    const int tau = wv * TPW + (tl % TPW);
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 15, gk = lane >> 4;
                        const int col = gate * H + 16 * tau + i;
                        // gate-major streams: [gate within the phase][wave][k-group][tile of the gate][lane] float4 (the kernel walks
                        // one gate's TPW tiles at a time: wide_x3_accumulate)
                        const int gsel = phase == 0 ? tl / TPW : 0, tp = tl % TPW;
                        for (int kap = 0; kap < kin; ++kap)
                            for (int q = 0; q < 4; ++q) {
                                const int src = l == 0 ? wide_input_row(e, kap, 4 * gk + q) : 16 * kap + 4 * gk + q;
                                wx[(((((size_t)gsel * WV + wv) * kin + kap) * TPW + tp) * 64 + lane) * 4 + q] = src < F ? L.kernel[(size_t)src * 3 * H + col] : 0.f;
                            }
                        for (int kap = 0; kap < H16; ++kap)
                            for (int q = 0; q < 4; ++q)
                                wr[(((((size_t)gsel * WV + wv) * H16 + kap) * TPW + tp) * 64 + lane) * 4 + q] =
                                    L.recurrent_kernel[(size_t)(16 * kap + 4 * gk + q) * 3 * H + col];
                        for (int q = 0; q < 4; ++q)      // C operand: this lane's output rows 4 gk + q
                            bias[(((size_t)wv * NT + tl) * 4 + q) * 64 + lane] = L.bias[gate * H + 16 * tau + 4 * gk + q];
                    }
                }
            int rc;
            if ((rc = dev_upload(e, &n.wide3_buf[l][phase == 0 ? 0 : 2], wx))) return rc;
            if ((rc = dev_upload(e, &n.wide3_buf[l][phase == 0 ? 1 : 3], wr))) return rc;
            if ((rc = dev_upload(e, &n.wide3_buf[l][phase == 0 ? 4 : 5], bias))) return rc;
        }
    }
    std::vector<float> wd((size_t)WV * TPW * 4 * 64, 0.f);
    for (int wv = 0; wv < WV; ++wv)
        for (int tp = 0; tp < TPW; ++tp)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    wd[(((size_t)wv * TPW + tp) * 4 + q) * 64 + lane] = w->dense_kernel[16 * (wv * TPW + tp) + 4 * (lane >> 4) + q];
    return dev_upload(e, &n.wide3_wd, wd);
}

// The same network with bf16 operands (gru_wide_bf16_device.h; gru_precision = 1): every kernel entry rounded once (B1), the
// bias as float32(hi + lo) for the accumulator (B2: the sum is exact).  Wave w owns output tiles tau = w TPW + t of every gate;
// row i of a tile <-> unit 16 tau + i; k-group kappa, k-slot 8 gk + e <-> source unit 32 kappa + 16 (e >> 2) + 4 gk + (e & 3)
// (layer 0 input: feature 8 gk + e, gk < 2).  Streams: [wave][kappa][tile][lane] x eight bf16.
int pack_gru_weights_wide_bf16(pe_engine* e, NetPack& n, const pe_weights* w) {
    const int H = w->layers[0].units, WV = 4, TPW = H / (16 * WV), KG = H / 32;
    auto widen = [](uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; std::memcpy(&f, &u, 4); return f; };
    for (int l = 0; l < w->n_layers; ++l) {
        const pe_gru_layer& L = w->layers[l];
        const int kin = l == 0 ? 1 : KG;
        const int F = L.n_in;
        for (int phase = 0; phase < 2; ++phase) {
            const int NT = phase == 0 ? 2 * TPW : TPW;
            const int NK = kin + KG;                    // one stream per phase: the input part's k-groups, then the recurrent part's
            std::vector<uint16_t> ws((size_t)WV * NK * NT * 64 * 8, 0);
            std::vector<float> bias((size_t)WV * NT * 4 * 64, 0.f);
            for (int wv = 0; wv < WV; ++wv)
                for (int tl = 0; tl < NT; ++tl) {
                    const int gate = phase == 0 ? (tl < TPW ? 0 : 1) : 2;
                    const int tau = wv * TPW + (tl % TPW);
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 15, gk = lane >> 4;
                        const int col = gate * H + 16 * tau + i;
                        for (int kap = 0; kap < kin; ++kap)
                            for (int ek = 0; ek < 8; ++ek) {
                                const int src = l == 0 ? (gk < 2 ? 8 * gk + ek : F) : 32 * kap + 16 * (ek >> 2) + 4 * gk + (ek & 3);
                                if (src < F) ws[((((size_t)wv * NK + kap) * NT + tl) * 64 + lane) * 8 + ek] = to_bf16(L.kernel[(size_t)src * 3 * H + col]);
                            }
                        for (int kap = 0; kap < KG; ++kap)
                            for (int ek = 0; ek < 8; ++ek) {
                                const int src = 32 * kap + 16 * (ek >> 2) + 4 * gk + (ek & 3);
                                ws[((((size_t)wv * NK + kin + kap) * NT + tl) * 64 + lane) * 8 + ek] = to_bf16(L.recurrent_kernel[(size_t)src * 3 * H + col]);
                            }
                        for (int q = 0; q < 4; ++q) {    // C operand: this lane's output rows 4 gk + q
                            const float b = L.bias[gate * H + 16 * tau + 4 * gk + q];
                            const float hi = widen(to_bf16(b));
                            bias[(((size_t)wv * NT + tl) * 4 + q) * 64 + lane] = hi + widen(to_bf16(b - hi));
                        }
                    }
                }
            int rc;
            if ((rc = dev_upload(e, &n.wideb_w[l][phase], ws))) return rc;
            if ((rc = dev_upload(e, &n.wideb_b[l][phase], bias))) return rc;
        }
    }
    std::vector<float> wd((size_t)WV * TPW * 4 * 64, 0.f);
    for (int wv = 0; wv < WV; ++wv)
        for (int tp = 0; tp < TPW; ++tp)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    wd[(((size_t)wv * TPW + tp) * 4 + q) * 64 + lane] = w->dense_kernel[16 * (wv * TPW + tp) + 4 * (lane >> 4) + q];
    return dev_upload(e, &n.wideb_wd, wd);
}

// Samples of the virtual stream that must have arrived, counted from a frame's first sample, before the
// reference's Listener has that frame in its window: the whole analysis window (sonopy emits one frame per
// full window), plus one hop for the legacy speechpy front end, whose stack_frames returns
// floor((len - window) / hop) frames -- one fewer.
int emit_window(const pe_params& p) { return p.window_samples + (p.vectorizer == 3 ? p.hop_samples : 0); }
int frame_len_of(const pe_params& p) { return p.window_samples < p.n_fft ? p.window_samples : p.n_fft; }
// frames computed (first frame_len samples arrived) but not yet emitted: at most this many exist at any time
int pending_frames(const pe_params& p) { return (emit_window(p) - frame_len_of(p) + p.hop_samples - 1) / p.hop_samples; }
// vectorize_raw on a whole buffer (vectorization.py:46-50): frames the vectorizer returns for n samples
int64_t frames_of_buffer(const pe_params& p, int64_t n) {
    const int64_t ew = emit_window(p);
    return n >= ew ? 1 + (n - ew) / p.hop_samples : 0;
}

// Vectorizer.mels: the front-end launchers run their MELS instantiation (rows = log-mel energies; prm.n_mfcc == prm.n_filt)
bool mel_rows(const pe_engine* e) { return e->prm.vectorizer == 1; }
// floats of one row of a network input window [T][..] (pe_predict, the trainer, mine_gather): with use_delta x_t, x_t - x_(t-1)
int window_floats(const pe_engine* e) { return e->prm.use_delta ? 2 * e->n_in : e->n_in; }

// A pass's task table into one buffer, grown as needed: desc[n], then the uint32 prefix [n + 1] of their tasks.  Fills `t`
// (ClipTable / RecTable) over it; n_tasks is the prefix's last entry.  rc: what ensure said; returns what the two copies said.
template <class Desc, class Table>
hipError_t upload_task_table(pe_engine* e, DeviceBuf& b, const std::vector<Desc>& desc, const std::vector<uint32_t>& prefix, const void* audio,
                             int audio_f32, Table& t, int& rc) {
    const size_t db = desc.size() * sizeof(Desc), pb = prefix.size() * sizeof(uint32_t);
    if ((rc = ensure(e, b, db + pb))) return hipSuccess;
    char* const p = static_cast<char*>(b.p);
    t = Table{reinterpret_cast<const Desc*>(p), reinterpret_cast<const uint32_t*>(p + db), (int)desc.size(), prefix.back(), audio, audio_f32};
    const hipError_t err = hipMemcpy(p, desc.data(), db, hipMemcpyHostToDevice);
    return err != hipSuccess ? err : hipMemcpy(p + db, prefix.data(), pb, hipMemcpyHostToDevice);
}
// vectorize() of a clip of `len` samples that ends at sample `end` of a pass's audio: audio[-max_samples:] (max_samples 0: all
// of it), then feats[-n_features:].  tasks: the kept frames of the pass so far -- the clip's prefix entry -- plus this clip's.
ClipDesc clip_desc(const pe_params& prm, int T, int64_t end, int64_t len, int64_t max_samples, uint32_t& tasks) {
    const int64_t cut = max_samples > 0 && len > max_samples ? max_samples : len;
    const int64_t frames = frames_of_buffer(prm, cut);
    const int64_t kept = frames < T ? frames : T;
    tasks += (uint32_t)kept;
    return ClipDesc{end - cut, (int)(frames - kept), (int)kept, (int)(T - kept), 0};
}

StreamGeom geom(const pe_engine* e) {
    StreamGeom g;
    g.n_streams = e->n_streams;
    g.log_mode = e->prm.vectorizer == 3 ? 1 : 0;
    g.window = emit_window(e->prm);
    g.hop = e->prm.hop_samples;
    g.frame_len = frame_len_of(e->prm);
    g.n_filt = e->prm.n_filt;
    g.n_mfcc = e->prm.n_mfcc;
    g.n_features = e->prm.n_features;
    g.ring_slots = e->ring_slots;
    return g;
}

template <class R>
WaveTables<R> tables(const pe_engine* e) {
    WaveTables<R> t;
    t.blob = e->table_blob;
    t.L = e->table_layout;
    return t;
}

// the most frames one stream can complete in a call of n_updates chunks (a full carry plus the new samples)
int max_frames_per_call(const pe_engine* e, long long new_samples) {
    const long long fmax = ((long long)(e->carry_cap - 1) + new_samples - frame_len_of(e->prm)) / e->prm.hop_samples + 1;
    return (int)(fmax < 1 ? 1 : fmax);
}

StreamState state_of(const pe_engine* e, uint32_t call) {
    StreamState st;
    st.rec = e->rec; st.carry = e->carry; st.n_padded = (uint32_t)e->n_padded; st.call = call;
    return st;
}

// Number of a call that writes records.  Call numbers are 32 bits; only the order of a stream's two sides and "written by
// this very call" are ever read from them, so long before the count wraps every record is renumbered (current side 2, other
// side 1; on the stream this call launches on, in front of its launches) and the count restarts.
int begin_state_call(pe_engine* e, hipStream_t s, uint32_t* call) {
    if (e->call_no >= e->renumber_at) {
        PE_HIP(e, launch_renumber(state_of(e, e->call_no + 1u), e->n_padded, s));
        e->call_no = 2u;
    }
    *call = ++e->call_no;
    ++e->chain_epoch;       // the streams move: carried chains fall behind (a chain launch moves them along and catches up, do_update)
    return PE_OK;
}

// ids / n_active: the streams of this launch (pe_update_subset; device pointer), or null / 0 = all of them in order
template <class R>
MfccStreamArgs<R> mfcc_args(const pe_engine* e, const int16_t* pcm_dev, int chunk, uint32_t call, const int32_t* ids = nullptr, int n_active = 0) {
    MfccStreamArgs<R> a;
    a.geo = geom(e);
    if (ids) a.geo.n_streams = n_active;
    a.pcm = pcm_dev;
    a.chunk = chunk;
    a.pcm_pairs_ok = ((chunk & 1) == 0) && ((reinterpret_cast<uintptr_t>(pcm_dev) & 3u) == 0);
    a.ids = ids;
    a.st = state_of(e, call);
    a.head = ids ? nullptr : e->call_head; a.head_chunk = e->call_head_chunk; a.keep = (!ids && e->call_keep) ? 1 : 0;
    a.ring = e->ring; a.ring_bf16 = e->prm.ring_precision;
    a.proj_ring = e->proj_on ? e->proj_ring : nullptr;
    a.n_updates = 1; a.ke_hist = nullptr; a.n_padded = e->n_padded;
    a.n_frame_rows = max_frames_per_call(e, chunk);
    a.div_hop = FastDiv::make((uint32_t)e->prm.hop_samples);
    a.div_chunk = FastDiv::make((uint32_t)chunk);
    return a;
}

template <class R>
GeneralStreamArgs<R> general_args(const pe_engine* e, const int16_t* pcm_dev, int chunk, uint32_t call, const int32_t* ids = nullptr, int n_active = 0) {
    GeneralStreamArgs<R> a{};
    a.geo = geom(e);
    if (ids) a.geo.n_streams = n_active;
    a.tab = e->gtab;
    a.pcm = pcm_dev; a.chunk = chunk;
    a.pcm_pairs_ok = ((chunk & 1) == 0) && ((reinterpret_cast<uintptr_t>(pcm_dev) & 3u) == 0);
    a.ids = ids;
    a.st = state_of(e, call); a.carry_cap = e->carry_cap;
    a.ring = e->ring; a.row_floats = e->row_floats;
    a.ring_bf16 = e->prm.ring_precision == 1;
    a.n_updates = 1; a.div_chunk = FastDiv::make((uint32_t)chunk); a.ke_hist = nullptr; a.n_padded = e->n_padded;
    return a;
}

// MFCC alone: every stream of the launch goes from its current side to the other one (records stamped `call`).
// The four kinds of front-end launch, each written once: the arguments built generically in the precision R (with_real), the
// family -- general front end or stock wave kernels -- chosen by the one `if (e->general)`.
// Streaming.  n_updates chunks per stream in one call (pe_update_many_device: ke_hist takes every update's emitted count).
int launch_stream_front_end(pe_engine* e, const int16_t* pcm_dev, int chunk, hipStream_t s, uint32_t call, const int32_t* ids = nullptr, int n_active = 0,
                            int n_updates = 1, uint32_t* ke_hist = nullptr) {
    // (no cap on the frames ONE update may complete: Listener.update takes a chunk of any length,
    //  network_runner.py:125-146; the frame tasks skip every row that the ring would overwrite again -- v_first in
    //  mfcc_frame_tasks -- so a long chunk costs its last ring_slots frames plus a scalar walk over the row indices)
    return with_real(e->prm, [&](auto real) -> int {
        using R = decltype(real);
        if (e->general) {
            GeneralStreamArgs<R> a = general_args<R>(e, pcm_dev, chunk, call, ids, n_active);
            a.n_updates = n_updates; a.ke_hist = ke_hist;
            PE_HIP(e, launch_general_stream(a, s, mel_rows(e)));
        } else {
            MfccStreamArgs<R> a = mfcc_args<R>(e, pcm_dev, chunk, call, ids, n_active);
            a.n_updates = n_updates; a.ke_hist = ke_hist; a.n_frame_rows = max_frames_per_call(e, (long long)n_updates * chunk);
            PE_HIP(e, launch_mfcc(a, tables<R>(e), e->n_cus, s, mel_rows(e)));
        }
        return PE_OK;
    });
}

// NetPack -> ModelNet: a model's weights as a launch of the form of `a` reads them.  The form -- which of the blobs b20 / x3 /
// cw a launch reads -- is the engine's (gru_args), the same for every model.
ModelNet model_net(const NetPack& n, const GruArgs& a) {
    return ModelNet{n.wx, n.wxd, n.wr1, n.wr2, n.bias, n.wd, a.cw ? n.cw_blob : nullptr, n.wx_bf16, n.wr_bf16, n.wd_bf16,
                    a.b20 ? n.b20_blob : nullptr, a.x3 ? n.x3_blob : nullptr, n.dense_bias};
}
// a launch's arguments with model m's weights
GruArgs with_model(const pe_engine* e, const GruArgs& a, int m) { return model_args(a, model_net(e->nets[m], a), 0, 0); }
ModelSet model_set(const pe_engine* e, const GruArgs& a) {
    ModelSet ms{};
    for (int m = 0; m < e->n_models; ++m) ms.net[m] = model_net(e->nets[m], a);
    return ms;
}

// the arguments of a network launch: the engine's form, model 0's weights
GruArgs gru_args(const pe_engine* e) {
    const NetPack& n0 = e->nets[0];
    GruArgs a{};
    a.n_streams = e->n_streams;
    a.n_features = e->prm.n_features;
    a.n_in = e->n_in;
    a.units = e->units;
    a.use_delta = e->prm.use_delta;
    a.ring = e->ring; a.ring_slots = e->ring_slots; a.ring_bf16 = e->prm.ring_precision;
    a.ids = nullptr; a.rec = e->rec; a.n_padded = (uint32_t)e->n_padded; a.ke_plain = nullptr;
    a.call = e->call_no + 1u;           // a reader behind every call so far (the network role of a fused launch: that call's own number)
    a.proj_ring = e->proj_on ? e->proj_ring : nullptr;
    a.predict_ke = 0;
    a.chunk = 0;
    a.window = emit_window(e->prm); a.hop = e->prm.hop_samples;
    a.frame_len = frame_len_of(e->prm);
    a.bf16 = e->prm.gru_precision == 1;
    a.b20 = e->gru_tiling == 0 ? nullptr : n0.b20_blob;      // bf16 network: five values per lane where it fits (pe_set_gru_tiling(e, 0): eight)
    a.feats = nullptr; a.out = nullptr; a.row_stride = 0;
    a.row_floats = e->row_floats;
    // Four waves per tile cut the latency of a tile's chain; that only pays while every tile gets a CU of its
    // own next to one MFCC workgroup.  Measured (fused, f64 front end; tools/gpu_policy.py): 4096 streams
    // 21.9 us (4 waves) vs 32.0 (1); 8192: 41.5 vs 33.5; 16384: 76.0 vs 55.3; 65536: 284 vs 199.
    // Stock width: the re-tiled shapes (three full tiles + partial sums; gru_cw_device.h) cut the four-wave kernel's
    // timestep (14.2 vs 16.3 us per window chain, stand-alone) but cost the one-wave kernel 5 % in the throughput
    // regime (two-pass MFMAs + reductions: 81.0 vs 77.3 us at 65 536 streams), so an engine takes ONE tiling for all
    // of its launches -- every shape of a tiling agrees bit for bit -- by its size.  The critical-wave kernel still
    // wins with two tiles per compute unit (8192 streams, fused: 272 vs 254 M windows/s against one wave per tile).
    // Engines with more stream tiles than the machine has SIMDs (> 4 tiles per compute unit: more than 16 384 streams on
    // MI355X) take the XDL form of the float32 network (gru_x3_device.h: every operand as three bf16 pieces): an f32-input
    // MFMA keeps its whole SIMD from issuing for its 8 passes, the bf16 MFMAs cost half the cycles for the same products and
    // do not.  Measured per update, two launches against the fused classic tiling: 54 vs 69 us at 20 480 streams, 59 vs 69 at
    // 24 576, 69 vs 79 at 32 768, 128 vs 154 us at 65 536 -- and 48 vs 43 us at 16 384 (one tile per SIMD: the classic network
    // still runs in one round of waves, and the missing fused launch costs more than the cheaper network saves).
    const bool x3_ok = n0.x3_blob && !a.bf16 && !e->wide && !a.proj_ring && e->row_floats == kRowFloats;
    // ... and so do engines reserved for several updates per call (pe_reserve_updates) whose batched network launch has more
    // (update, tile) windows than the machine has SIMDs: ONE form per engine (every launch of a form agrees bit for bit), chosen
    // for the launch the engine was reserved for -- its single updates then run the one-wave XDL kernel in two launches.
    // Measured at 4096 streams x 8 updates per call: 61.6 us for the batched network on the re-tiled f32-input form against
    // the XDL form's rate of ~26 us for the same 32 768 windows (profiles/round5/r5zz_kernel_stats.csv; round 6: profiles/round6).
    const bool many_windows = e->max_updates > 1 && (long long)e->max_updates * e->n_tiles > 4LL * e->n_cus;
    a.x3 = x3_ok && (e->gru_tiling == 2 || (e->gru_tiling < 0 && (e->n_tiles > 4 * e->n_cus || many_windows))) ? n0.x3_blob : nullptr;
    const bool cw_ok = n0.cw_blob && e->row_floats == kRowFloats && !a.proj_ring && !a.bf16 && !a.x3 && !e->wide;
    const bool retile = cw_ok && (e->gru_tiling == 1 || (e->gru_tiling < 0 && e->n_tiles <= 2 * e->n_cus));
    const int auto_waves = retile ? (e->n_tiles <= 2 * e->n_cus ? 4 : 1) : (e->n_tiles <= e->n_cus ? 4 : 1);
    a.waves_per_tile = a.x3 ? 1 : e->gru_waves ? e->gru_waves : auto_waves;
    if (e->prm.use_delta && !retile) a.waves_per_tile = 1;       // (classic tiling: only the one-wave kernel carries the delta inputs)
    if (e->row_floats != kRowFloats && !(gru_small_regs(e->units) == 5 && !e->prm.use_delta && a.waves_per_tile == 4))
        a.waves_per_tile = 1;       // ... and the 32-float feature rows (stock width: four waves per tile exist, gru_tile_mw5<.., 2>)
    a.cw = retile ? n0.cw_blob : nullptr;
    return with_model(e, a, 0);
}

// which form a wide engine's launches take: the XDL form when asked for (pe_set_gru_tiling(e, 2)); the default stays the
// f32-input MFMA kernel -- measured equal (1.26 ms per launch at 256 x 2, profiles/round5/r5f_wide_forms.log) and float32-exact
bool wide_uses_x3(const pe_engine* e) { return e->wide && e->gru_tiling == 2; }

// The network of every model of the engine over the windows of `g`, for any input mode (0 explicit batch, 1 ring, 2 row
// sequence); model m writes g.out + m * out_stride.  ONE launch (K models: kernels.hip gru_models_kernel, the same tile function);
// the wide / stacked networks take one launch per model -- each fills the machine on its own.
int launch_networks(pe_engine* e, const GruArgs& g, int mode, hipStream_t s, long long out_stride) {
    if (!e->wide) {
        const ModelSet ms = model_set(e, g);
        PE_HIP(e, launch_gru_small(g, mode, s, e->n_models > 1 ? &ms : nullptr, e->n_models, out_stride));
        return PE_OK;
    }
    // two forms of the streamed-weight network (pe_set_gru_tiling): 0 = f32-input MFMAs (gru_wide_device.h), 2 = float32
    // products on the bf16 pipe with the float32 weights split in registers (gru_wide_x3_device.h)
    // ... and, for gru_precision = 1, the bf16-operand network (gru_wide_bf16_device.h), the engine's only form
    if (e->prm.gru_precision == 1) {
        for (int m = 0; m < e->n_models; ++m) {
            const NetPack& n = e->nets[m];
            WideArgs wa{};
            wa.base = with_model(e, g, m);
            wa.base.out = g.out + (size_t)m * (size_t)out_stride;
            wa.n_layers = e->n_layers;
            wa.units = e->units;
            wa.wd = n.wideb_wd;
            for (int l = 0; l < e->n_layers; ++l) {
                wa.layer[l].wx1 = reinterpret_cast<const float4*>(n.wideb_w[l][0]);      // (the whole stream of a phase: input part, then recurrent part)
                wa.layer[l].wx2 = reinterpret_cast<const float4*>(n.wideb_w[l][1]);
                wa.layer[l].b1 = n.wideb_b[l][0];
                wa.layer[l].b2 = n.wideb_b[l][1];
                wa.layer[l].kx4 = l == 0 ? 1 : e->units / 32;
            }
            PE_HIP(e, launch_gru_wide_bf16(wa, mode, s));
        }
        return PE_OK;
    }
    const bool x3 = wide_uses_x3(e);
    for (int m = 0; m < e->n_models; ++m) {
        const NetPack& n = e->nets[m];
        float* const (*buf)[6] = x3 ? n.wide3_buf : n.wide_buf;
        WideArgs wa{};
        wa.base = with_model(e, g, m);
        wa.base.out = g.out + (size_t)m * (size_t)out_stride;
        wa.n_layers = e->n_layers;
        wa.units = e->units;
        wa.wd = x3 ? n.wide3_wd : n.wide_wd;
        for (int l = 0; l < e->n_layers; ++l) {
            wa.layer[l].wx1 = reinterpret_cast<const float4*>(buf[l][0]);
            wa.layer[l].wr1 = reinterpret_cast<const float4*>(buf[l][1]);
            wa.layer[l].wx2 = reinterpret_cast<const float4*>(buf[l][2]);
            wa.layer[l].wr2 = reinterpret_cast<const float4*>(buf[l][3]);
            wa.layer[l].b1 = buf[l][4];
            wa.layer[l].b2 = buf[l][5];
            wa.layer[l].kx4 = e->wide_kx4[l];
        }
        if (x3) PE_HIP(e, launch_gru_wide_x3(wa, mode, s));
        else PE_HIP(e, launch_gru_wide(wa, mode, s));
    }
    return PE_OK;
}
// pe_update_many's batched network: out[model][update][window]
int launch_networks_many(pe_engine* e, const GruArgs& g, int n_updates, hipStream_t s) {
    const ModelSet ms = model_set(e, g);
    PE_HIP(e, launch_gru_many(g, n_updates, e->n_padded, s, e->n_models > 1 ? &ms : nullptr, e->n_models));
    return PE_OK;
}

int launch_gru_ring(pe_engine* e, float* out_dev, hipStream_t s, const int32_t* ids = nullptr, int n_active = 0) {
    GruArgs a = gru_args(e);
    a.out = out_dev;
    if (ids) { a.ids = ids; a.n_streams = n_active; }
    return launch_networks(e, a, 1, s, a.n_streams);
}

// ---- host-fed pipeline -------------------------------------------------------------------------------------------
bool is_pinned(const pe_engine* e, const void* p, size_t bytes) {
    const char* c = static_cast<const char*>(p);
    for (const auto& r : e->pinned)
        if (c >= r.first && c + bytes <= r.first + r.second) return true;
    return false;
}

int async_init(pe_engine* e) {
    if (e->s_compute) return PE_OK;
    PE_HIP(e, hipStreamCreateWithFlags(&e->s_copy, hipStreamNonBlocking));
    PE_HIP(e, hipStreamCreateWithFlags(&e->s_compute, hipStreamNonBlocking));
    for (auto& sl : e->aslot) {
        PE_HIP(e, hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
        PE_HIP(e, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    PE_HIP(e, hipEventCreateWithFlags(&e->ev_user, hipEventDisableTiming));
    return PE_OK;
}

int ensure_pinned(pe_engine* e, void** p, size_t* have, size_t bytes) {
    if (*have >= bytes) return PE_OK;
    if (*p) { (void)hipHostFree(*p); *p = nullptr; *have = 0; }
    hipError_t err = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (err != hipSuccess) return fail(e, PE_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    *have = bytes;
    return PE_OK;
}

// the update in this slot has finished: hand its probabilities to the caller
int finish_slot(pe_engine* e, pe_engine::AsyncSlot& sl) {
    if (!sl.busy) return PE_OK;
    const hipError_t err = hipEventSynchronize(sl.done);
    sl.busy = false;                                  // (also when the wait failed: a slot that stays busy would fail every later drain)
    --e->async_inflight;
    if (err != hipSuccess) return fail(e, PE_ERR_HIP, "hipEventSynchronize(update in flight) failed: %s", hipGetErrorString(err));
    for (auto& o : sl.out)
        if (o.user && !o.direct) std::memcpy(o.user, o.pin, o.bytes);
    return PE_OK;
}

int drain_async(pe_engine* e) {
    if (!e || e->async_inflight == 0) return PE_OK;
    int first_rc = PE_OK;
    for (int i = 0; i < pe_engine::kAsyncDepth; ++i) {                 // oldest first; a failed slot does not keep the others in flight
        const int rc = finish_slot(e, e->aslot[(e->async_next + i) % pe_engine::kAsyncDepth]);
        if (rc && !first_rc) first_rc = rc;
    }
    return first_rc;
}

// a *_device entry point is about to enqueue state-moving work on the caller's stream (see pe_engine::last_user_stream)
void note_user_stream(pe_engine* e, void* stream) {
    e->last_user_stream = static_cast<hipStream_t>(stream);
    e->user_dirty = true;
}

int check_chunk(pe_engine* e, const void* pcm, int chunk) {
    if (!e) return PE_ERR_INVALID;
    if (chunk == 0) return fail(e, PE_ERR_EOF, "empty chunk");
    if (chunk < 0 || !pcm) return fail(e, PE_ERR_INVALID, "bad pcm buffer / chunk_samples=%d", chunk);
    return PE_OK;
}

int check_decoder(pe_engine* e) {
    for (int m = 0; m < e->n_models; ++m) {
        const DecState& d = e->dec[m];
        if (!d.cd && d.out_range != 0) return fail(e, PE_ERR_INVALID, "pe_set_decoder has not been called");
        if (!d.cd_len && !d.cd) return fail(e, PE_ERR_INVALID, m ? "pe_set_decoder has not been called for model %d" : "pe_set_decoder has not been called", m);
    }
    return PE_OK;
}

// every id in range, none twice (two rows for one stream in one launch would race on its record / its trigger state)
int check_ids(pe_engine* e, const int32_t* ids, int n_active) {
    e->seen_ids.assign((size_t)e->n_streams, 0);
    for (int i = 0; i < n_active; ++i) {
        const int32_t id = ids[i];
        if (id < 0 || id >= e->n_streams) return fail(e, PE_ERR_INVALID, "stream_ids[%d]=%d outside 0..%d", i, id, e->n_streams - 1);
        if (e->seen_ids[(size_t)id]) return fail(e, PE_ERR_INVALID, "stream %d is named twice (stream_ids[%d])", id, i);
        e->seen_ids[(size_t)id] = 1;
    }
    return PE_OK;
}

// ONE decode launch (a K-model engine: per-model tables) over n_rows rows per model: every stream in order (ids null,
// n_rows = n_streams), or the streams ids[0 .. n_rows) (device pointer).  raw / conf_out / fired_out: [n_models][n_rows].
int launch_decode_rows(pe_engine* e, const int32_t* ids_dev, int n_rows, const float* raw_dev, double* conf_out_dev,
                       unsigned char* fired_out_dev, hipStream_t s) {
    const size_t n = (size_t)n_rows;
    DecodeSet set{};
    for (int m = 0; m < e->n_models; ++m) {
        DecodeArgs& a = set.m[m];
        a.n_streams = n_rows; a.raw = raw_dev + m * n;
        a.conf_out = conf_out_dev ? conf_out_dev + m * n : nullptr;
        a.fired_out = fired_out_dev ? fired_out_dev + m * n : nullptr;
        const DecState& d = e->dec[m];
        a.cd = d.cd; a.cd_len = d.cd_len;
        a.min_out = d.min_out; a.out_range = d.out_range; a.center = d.center;
        a.activation = d.on ? e->activation + (size_t)m * e->n_padded : nullptr;
        a.threshold = d.threshold; a.trigger_level = d.level; a.rearm = d.rearm;
        a.ids = ids_dev;
    }
    if (e->n_models == 1) PE_HIP(e, launch_decode(set.m[0], s));
    else PE_HIP(e, launch_decode_models(set, e->n_models, n_rows, s));
    return PE_OK;
}

// Leaving the keep style: the leftovers that still lie in the last call's chunks go to the carry (one small launch on the
// stream of the call that needs them there), and the engine forgets the chunks.
int flush_kept(pe_engine* e, hipStream_t s) {
    if (!e->kept) return PE_OK;
    PE_HIP(e, launch_materialize_carry(state_of(e, e->call_no + 1u), e->kept, e->kept_chunk, e->n_streams, s));
    e->kept = nullptr; e->kept_chunk = 0;
    return PE_OK;
}

// May the leftover of an update of these chunks stay in them?  The stock front end (the general one keeps its own carry
// arithmetic), whole sample pairs (the frame role's dword loads), and a chunk that holds any leftover (< frame_len samples).
bool keep_eligible(const pe_engine* e, const int16_t* pcm_dev, int chunk) {
    return !e->general && (chunk & 1) == 0 && (reinterpret_cast<uintptr_t>(pcm_dev) & 3u) == 0 && chunk >= frame_len_of(e->prm) - 1
        && chunk >= e->carry_cap - 1;
}

// True when no frame computed by an update of `chunk` samples can become visible in that same
// update (it needs window - frame_len more samples), so the network does not depend on it.
bool can_fuse(const pe_engine* e, int chunk) {
    // (the fused kernels exist for the stock table shape: filterbanks whose runs need the wide loop bounds take two launches;
    //  so do networks of 21..32 units on the one-wave kernel: their register-resident weights do not fit beside the
    //  frame role's 128-register budget -- fused, that shape spilled 96-240 bytes per lane into the time loop)
    if (mel_rows(e)) return false;      // (mel rows on the stock wave kernel, n_filt <= 16: the frame role of the fused kernels has no MELS instantiation)
    if (!(e->fused && !e->general && !e->wide && e->table_layout.mel_pad == 10 && chunk <= emit_window(e->prm) - frame_len_of(e->prm))) return false;
    // (gru_x3_device.h: ~220 registers per lane against the frame role's ~100, and one kernel has one budget.  The same
    //  concurrency as TWO kernels -- the network on a side stream between two events -- was built and measured: 142 vs
    //  134 us per update at 65 536 streams, 40 vs 24 us at 4096: the event hand-offs cost more than the overlap buys)
    if (gru_args(e).x3) return false;
    if (e->prm.gru_precision == 0 && gru_small_regs(e->units) >= 6 && gru_args(e).waves_per_tile != 4) return false;
    if (e->prm.use_delta && e->prm.gru_precision == 0) {        // re-tiled one-wave shape with delta inputs: no fused instantiation
        // (waves_per_tile == 4 is not enough: the four-wave shape needs the 32-slot ring it stages in LDS -- after
        //  pe_reserve_updates, or with a longer feature window, the launcher falls back to the one-wave shape, whose
        //  fused instantiation has no delta inputs)
        const GruArgs g = gru_args(e);
        if (g.cw && (g.waves_per_tile != 4 || e->ring_slots != kCwSlots || e->prm.n_features > kCwSlots)) return false;
    }
    return true;
}

// Updates in a row that must be eligible before an engine in automatic mode builds its chains (pe_set_chain_carry): hysteresis
// against callers that alternate between eligible and other calls.  Every entry costs one rebuild launch
// (gru_chains_rebuild_kernel: the 435 chain steps of every stream), measured at 4096 streams: 102 us, against 0.99 us that a
// chain launch saves per update (15.13 -> 14.14 us) -- 103 updates to earn it back, rounded up to a power of two.
constexpr int kChainEnterAfter = 128;

// Eligible updates in a row with ONE chunk longer than a hop before a chain launch stops advancing the chains that no update of
// that cadence hands out (gru_chain_device.h, ChainArgs::skip; 1 - hop / chunk of them).  Nothing is rebuilt when skipping
// starts; leaving the cadence costs one rebuild launch in front of the first call with another chunk.  Derived as
// kChainEnterAfter was: that launch, 103.4 us at 4096 streams, against 0.85 us saved per update of 1024 samples (13.67 -> 12.82 us
// by HIP events, profiles/chain_skip/README.md) -- 122 updates to earn it back, rounded up to a power of two.
constexpr int kChainSkipAfter = 128;

// May this update advance carried chains instead of running every window again?  Exactly the headline rows of DESIGN 0:
// the stock float32 network re-tiled on four waves per tile over the 32-slot float32 ring (<= 8192 streams), one model, no
// delta inputs, no projection rows, a chunk the fused launch takes and that makes at most two rows visible, and no explicit
// launch-shape knob.  Full and subset calls, carry and keep styles alike.
bool chain_eligible(const pe_engine* e, int chunk) {
    if (e->chain_mode == 0 || e->n_models != 1 || e->prm.use_delta || e->prm.ring_precision != 0 || e->timing) return false;
    if (e->gru_tiling >= 0 || e->gru_waves != 0 || !e->fused || e->max_updates > 1) return false;
    if (e->ring_slots != kCwSlots || e->prm.n_features > kCwSlots - 3) return false;
    if ((chunk + e->prm.hop_samples - 1) / e->prm.hop_samples > 2) return false;
    if (!can_fuse(e, chunk)) return false;
    const GruArgs g = gru_args(e);
    return g.cw && g.waves_per_tile == 4 && !g.proj_ring && !g.bf16 && !g.x3;
}

// ids / n_active: the streams that take part (pe_update_subset; device pointer, PCM rows and outputs in that order), or
// null / 0 = every stream
// keep: the caller promises that pcm_dev stays alive and unchanged until the NEXT state-moving call's work has completed
// (pe_update_device_keep; pe_update_async: the engine's own ring of device buffers) -- the leftover then stays in the chunk
int do_update(pe_engine* e, const int16_t* pcm_dev, int chunk, float* raw_out_dev, float* feats_out_dev,
              hipStream_t s, const int32_t* ids = nullptr, int n_active = 0, bool keep = false) {
    int rc;
    const bool t = e->timing;
    const bool keep_call = keep && !ids && keep_eligible(e, pcm_dev, chunk);
    if (keep_call && e->kept) {
        // the previous call's chunks must still hold its leftovers: a caller that refills ONE buffer for every call has broken
        // the promise of pe_update_device_keep, and the samples are gone -- refuse instead of computing frames from the wrong audio
        const char* a0 = reinterpret_cast<const char*>(e->kept);
        const char* a1 = a0 + (size_t)e->n_streams * e->kept_chunk * sizeof(int16_t);
        const char* b0 = reinterpret_cast<const char*>(pcm_dev);
        const char* b1 = b0 + (size_t)e->n_streams * chunk * sizeof(int16_t);
        if (b0 < a1 && a0 < b1)
            return fail(e, PE_ERR_INVALID, "pe_update_device_keep: this call's chunks overlap the previous call's (%p), which still hold the "
                        "streams' leftover samples -- alternate between at least two buffers, or use pe_update_device", (const void*)e->kept);
    }
    if (!keep_call && (rc = flush_kept(e, s))) return rc;
    e->call_head = keep_call ? e->kept : nullptr; e->call_head_chunk = e->kept_chunk; e->call_keep = keep_call;
    // (whatever happens below, the launches of later calls must not inherit this call's style)
    struct Reset { pe_engine* e; ~Reset() { e->call_head = nullptr; e->call_head_chunk = 0; e->call_keep = false; } } reset{e};
    e->kept = keep_call ? pcm_dev : nullptr; e->kept_chunk = keep_call ? chunk : 0;
    // carried chains: valid only if nothing but chain launches moved the streams since they were built (decided BEFORE this
    // call's own bump of the epoch)
    const bool chain_call = raw_out_dev && !feats_out_dev && chain_eligible(e, chunk);
    const bool chains_current = chain_call && e->chains && e->chains_built_epoch == e->chain_epoch;
    // (the streak is of eligible calls with nothing else in between: any other bump of the epoch starts it again)
    if (!chain_call || e->chain_epoch != e->chain_seen_epoch) e->chain_streak = 0;
    if (chain_call) ++e->chain_streak;
    const bool chains_enter = chain_call && !chains_current && (e->chain_mode == 2 || e->chain_streak > kChainEnterAfter);
    // (the run is of eligible calls with one chunk; chains left out for another chunk -- or left behind by anything else -- are
    //  made whole again before they are advanced)
    if (!chain_call || e->chain_epoch != e->chain_seen_epoch || chunk != e->chain_run_chunk) e->chain_run = 0;
    if (chain_call) { ++e->chain_run; e->chain_run_chunk = chunk; }
    if (!chains_current) e->chain_skip_chunk = 0;
    const bool chains_leave = e->chain_skip_chunk != 0 && chunk != e->chain_skip_chunk;
    uint32_t call = 0;
    if ((rc = begin_state_call(e, s, &call))) return rc;
    e->chain_seen_epoch = e->chain_epoch;
    if (t) { PE_HIP(e, hipEventRecord(e->ev[0], s)); }
    if (chains_current || chains_enter) {
        if (!e->chains) {
            if ((rc = dev_alloc(e, &e->chain_ke, (size_t)e->n_padded))) return rc;
            if ((rc = dev_alloc(e, &e->chains, (size_t)e->n_tiles * kCwSlots * 5 * 64))) return rc;
        }
        const bool skip = chunk > e->prm.hop_samples && e->chain_run >= kChainSkipAfter;
        const ChainArgs ch{e->chains, e->chain_ke, skip ? 1 : 0};
        GruArgs g = gru_args(e);
        g.call = call;
        // entering, or leaving a cadence that left chains out: every live chain from the ring and the records as they stand
        // before this update, in front of the launch
        if (chains_enter || chains_leave) {
            PE_HIP(e, launch_chains_rebuild(g, ch, e->n_padded, s));
            e->chain_skip_chunk = 0;
        }
        g.predict_ke = 1;
        g.chunk = chunk;
        g.out = raw_out_dev;
        if (ids) { g.ids = ids; g.n_streams = n_active; }
        if ((rc = with_real(e->prm, [&](auto real) -> int {
                using R = decltype(real);
                PE_HIP(e, launch_fused_chains(mfcc_args<R>(e, pcm_dev, chunk, call, ids, n_active), tables<R>(e), g, ch, e->n_cus, s));
                return PE_OK; }))) return rc;
        e->chains_built_epoch = e->chain_epoch;          // (only now: a launch that failed leaves the chains behind the streams)
        if (skip) e->chain_skip_chunk = chunk;
    } else if (raw_out_dev && can_fuse(e, chunk)) {
        GruArgs g = gru_args(e);             // the records as they stand BEFORE the update; the waves predict ke
        g.call = call;                       // (records this launch writes are not read by it)
        g.predict_ke = 1;
        g.chunk = chunk;
        g.out = raw_out_dev;
        if (ids) { g.ids = ids; g.n_streams = n_active; }
        const ModelSet ms = model_set(e, g);             // K > 1: K network roles beside the one frame role, outputs [K][windows]
        const ModelSet* const models = e->n_models > 1 ? &ms : nullptr;
        if ((rc = with_real(e->prm, [&](auto real) -> int {
                using R = decltype(real);
                PE_HIP(e, launch_fused(mfcc_args<R>(e, pcm_dev, chunk, call, ids, n_active), tables<R>(e), g, e->n_cus, s, models, e->n_models));
                return PE_OK; }))) return rc;
        if (t) { PE_HIP(e, hipEventRecord(e->ev[1], s)); PE_HIP(e, hipEventRecord(e->ev[2], s)); e->ev_valid = true; e->ev_has_gru = false; }
    } else {
        if ((rc = launch_stream_front_end(e, pcm_dev, chunk, s, call, ids, n_active))) return rc;
        if (t) { PE_HIP(e, hipEventRecord(e->ev[1], s)); }
        if (raw_out_dev) {
            if ((rc = launch_gru_ring(e, raw_out_dev, s, ids, n_active))) return rc;
        }
        if (t) { PE_HIP(e, hipEventRecord(e->ev[2], s)); e->ev_valid = true; e->ev_has_gru = raw_out_dev != nullptr; }
    }
    if (feats_out_dev) {
        GatherArgs g{e->n_streams, e->prm.n_features, e->prm.n_mfcc, e->ring_slots, e->prm.ring_precision, e->ring, state_of(e, e->call_no + 1u), feats_out_dev, e->row_floats};
        PE_HIP(e, launch_gather(g, s));
    }
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_abi_version(void) { return PE_ABI_VERSION; }
const char* pe_last_global_error(void) { return g_global_error.c_str(); }
const char* pe_last_error(const pe_engine* e) { return e ? e->err.c_str() : g_global_error.c_str(); }

namespace {
// One model's network in every layout the engine's forms read: pe_create fills a fresh NetPack (dev_upload allocates), pe_set_weights
// runs the same routines again over the buffers that exist (same widths: same sizes).
int pack_model(pe_engine* e, NetPack& n, const pe_weights* w, const bool wide, const int wide_units) {
    const pe_gru_layer& L = w->layers[0];
    int rc = PE_OK;
    n.dense_bias = w->dense_bias;
    do {
        if (wide) {
            // Any width 33..256 (and stacked layers of different widths) runs on the streamed-weight kernel at the next
            // multiple of 64: a padded unit has zero weights and zero bias everywhere, so z = r = 1/2, candidate = 0 and
            // its state stays exactly 0 -- it neither receives nor contributes anything.
            const int Hp = wide_units;
            std::vector<std::vector<float>> kp(w->n_layers), rp(w->n_layers), bp(w->n_layers);
            std::vector<pe_gru_layer> lp(w->n_layers);
            for (int l = 0; l < w->n_layers; ++l) {
                const pe_gru_layer& Ls = w->layers[l];
                const int Hs = Ls.units, Fin = Ls.n_in, Fp = l == 0 ? Fin : Hp;
                kp[l].assign((size_t)Fp * 3 * Hp, 0.f); rp[l].assign((size_t)Hp * 3 * Hp, 0.f); bp[l].assign((size_t)3 * Hp, 0.f);
                for (int gate = 0; gate < 3; ++gate)
                    for (int u = 0; u < Hs; ++u) {
                        for (int k = 0; k < Fin; ++k) kp[l][(size_t)k * 3 * Hp + gate * Hp + u] = Ls.kernel[(size_t)k * 3 * Hs + gate * Hs + u];
                        for (int k = 0; k < Hs; ++k) rp[l][(size_t)k * 3 * Hp + gate * Hp + u] = Ls.recurrent_kernel[(size_t)k * 3 * Hs + gate * Hs + u];
                        bp[l][(size_t)gate * Hp + u] = Ls.bias[gate * Hs + u];
                    }
                lp[l] = pe_gru_layer{Fp, Hp, kp[l].data(), rp[l].data(), bp[l].data()};
            }
            std::vector<float> dp(Hp, 0.f);
            const int Hlast = w->layers[w->n_layers - 1].units;
            for (int u = 0; u < Hlast; ++u) dp[u] = w->dense_kernel[u];
            pe_weights wp{w->n_layers, lp.data(), dp.data(), w->dense_bias};
            e->units = Hp;
            if ((rc = pack_gru_weights_wide(e, n, &wp))) break;
            if ((rc = pack_gru_weights_wide_x3(e, n, &wp))) break;
            if (e->prm.gru_precision == 1 && (rc = pack_gru_weights_wide_bf16(e, n, &wp))) break;
        }
        else if ((rc = pack_gru_weights(e, n, L, w->dense_kernel))) break;
        if (!wide && e->prm.gru_precision == 1 && (rc = pack_gru_weights_bf16(e, n, L, w->dense_kernel))) break;
        if (!wide && b20_eligible(e->prm, L) && (rc = pack_gru_weights_b20(e, n, L, w->dense_kernel))) break;
        if (!wide && x3_eligible(e->prm, L) && (rc = pack_gru_weights_x3(e, n, L, w->dense_kernel))) break;
    } while (false);
    return rc;
}

// pe_create / pe_create_models: w[0 .. n_models) (checked against w[0] by pe_create_models before it comes here)
int create_engine(const pe_params* p_given, const double* mel_filters, const pe_weights* w, int32_t n_models, int32_t n_streams,
                  int32_t device, pe_engine** out) {
    if (!p_given || !mel_filters || !w || !out) return fail(nullptr, PE_ERR_INVALID, "null argument to pe_create");
    *out = nullptr;
    // Vectorizer.mels (vectorizer = 1, vectorization.py:32-35): a row is the n_filt log-mel energies, no DCT.  Behind the
    // checks of n_mfcc itself the engine's n_mfcc IS that row width W = n_filt (params.py:99-109: feature_size), so ring rows,
    // window, network inputs and every eligibility rule below are keyed on W; the front-end kernels run their MELS
    // instantiation (mel_rows).  The given n_mfcc is range-checked and otherwise ignored.
    pe_params p_rows = *p_given;
    const pe_params* const p = &p_rows;
    const bool mels = p_given->vectorizer == 1;
    if (p->n_mfcc < 1 || p->n_mfcc > kGeneralMaxMfcc) return fail(nullptr, PE_ERR_UNSUPPORTED, "n_mfcc must be in 1..%d (got %d)", kGeneralMaxMfcc, p->n_mfcc);
    if (mels) {
        if (p->n_filt < 1 || p->n_filt > kGeneralMaxMfcc)
            return fail(nullptr, PE_ERR_UNSUPPORTED, "Vectorizer.mels feeds n_filt values per frame and the networks take up to %d inputs per frame (got n_filt=%d)", kGeneralMaxMfcc, p->n_filt);
        p_rows.n_mfcc = p->n_filt;
    }
    if (n_streams <= 0) return fail(nullptr, PE_ERR_INVALID, "n_streams must be positive, got %d", n_streams);
    // ListenerParams (params.py:28-118): the stock shape (n_fft = 512, <= 64 filters, <= 16 coefficients) runs on the
    // one-frame-per-wave kernel, every other shape on the general front end (mfcc_general_device.h)
    // ... any n_fft from 16 on: powers of two up to 2048 as a packed real transform, every other length up to 1024 (numpy's
    // rfft takes any n) through Bluestein's chirp-z form over the next power of two >= 2 n_fft - 1
    // (general_is_pow2: powers of two from 64 on; 16 and 32 run as Bluestein transforms over 128 points like every other short length)
    if (p->n_fft < 16 || p->n_fft > kGeneralMaxFft || (!general_is_pow2(p->n_fft) && p->n_fft > kGeneralMaxBlueFft))
        return fail(nullptr, PE_ERR_UNSUPPORTED, "n_fft must be any length in 16..%d or a power of two up to %d (got %d)", kGeneralMaxBlueFft, kGeneralMaxFft, p->n_fft);
    if (p->n_filt < 1 || p->n_filt > kGeneralMaxFilt || p->n_mfcc > p->n_filt)
        return fail(nullptr, PE_ERR_UNSUPPORTED, "need 1 <= n_mfcc <= n_filt <= %d (got n_filt=%d n_mfcc=%d)", kGeneralMaxFilt, p->n_filt, p->n_mfcc);
    bool general = p->n_fft != kNfft || p->n_filt > kMaxFilt || p->n_mfcc > kRowFloats;
    if (p->hop_samples < 1 || p->window_samples < 1 || p->n_features < 1)
        return fail(nullptr, PE_ERR_INVALID, "window/hop/n_features must be positive");
    if (p->mfcc_precision != 0 && p->mfcc_precision != 1) return fail(nullptr, PE_ERR_INVALID, "mfcc_precision must be 0 (f64) or 1 (f32)");
    if (p->gru_precision != 0 && p->gru_precision != 1) return fail(nullptr, PE_ERR_INVALID, "gru_precision must be 0 (f32) or 1 (bf16 operands)");
    if (p->vectorizer < 0 || p->vectorizer > 3)
        return fail(nullptr, PE_ERR_UNSUPPORTED, "vectorizer must be 1 (mels), 2 (mfccs) or 3 (speechpy_mfccs), got %d", p->vectorizer);
    if (p->ring_precision != 0 && p->ring_precision != 1) return fail(nullptr, PE_ERR_INVALID, "ring_precision must be 0 (f32 rows) or 1 (bf16 rows)");
    if (p->ring_precision == 1 && p->gru_precision != 1) return fail(nullptr, PE_ERR_UNSUPPORTED, "bf16 feature rows (ring_precision = 1) feed the bf16-operand network only (gru_precision = 1)");
    if (w->n_layers < 1 || w->n_layers > 2 || !w->layers) return fail(nullptr, PE_ERR_UNSUPPORTED, "networks of 1 or 2 GRU layers have kernels (got %d layers)", w->n_layers);
    const pe_gru_layer& L = w->layers[0];
    const bool wide = w->n_layers == 2 || L.units > 32;
    if (!wide && L.units < 1) return fail(nullptr, PE_ERR_INVALID, "units must be positive");
    int wide_units = 0;          // width the streamed-weight kernel runs at: the layers' widths padded to a multiple of 64
    if (wide) {
        int hmax = L.units;
        if (w->n_layers == 2) {
            const pe_gru_layer& L2 = w->layers[1];
            if (!L2.kernel || !L2.recurrent_kernel || !L2.bias) return fail(nullptr, PE_ERR_INVALID, "null weight pointer");
            if (L2.n_in != L.units || L2.units < 1) return fail(nullptr, PE_ERR_INVALID, "layer 2 (n_in=%d, units=%d) does not follow layer 1 (units=%d)", L2.n_in, L2.units, L.units);
            if (L2.units > hmax) hmax = L2.units;
        }
        if (hmax > 256) return fail(nullptr, PE_ERR_UNSUPPORTED, "the streamed-weight GRU kernel holds up to 256 units per layer (got %d)", hmax);
        // the float32 forms take up to 32 inputs per frame as two k-groups of 16 (gru_wide_device.h WideInput): use_delta over
        // <= 16 coefficients, or 17..32 coefficients; the bf16-operand form reads plain rows of <= 16 coefficients
        if (p->use_delta && p->gru_precision == 1)
            return fail(nullptr, PE_ERR_UNSUPPORTED, "use_delta has no bf16-operand wide-GRU kernel (gru_precision = 1 networks of more than 32 units or two layers take plain feature rows)");
        if (p->use_delta && p->n_mfcc > kRowFloats)
            return fail(nullptr, PE_ERR_UNSUPPORTED, "use_delta over more than 16 %s (%s = %d: %d inputs per frame) has no wide-GRU kernel: the first layer takes up to 32 inputs",
                        mels ? "mel values" : "coefficients", mels ? "n_filt" : "n_mfcc", p->n_mfcc, 2 * p->n_mfcc);
        if (p->n_mfcc > kRowFloats && p->gru_precision == 1)
            return fail(nullptr, PE_ERR_UNSUPPORTED, "more than 16 %s per frame (%s = %d) have no bf16-operand wide-GRU kernel: gru_precision = 1 networks of more than 32 units or two layers take rows of <= 16 values",
                        mels ? "mel values" : "coefficients", mels ? "n_filt" : "n_mfcc", p->n_mfcc);
        if (p->ring_precision == 1) return fail(nullptr, PE_ERR_UNSUPPORTED, "bf16 feature rows (ring_precision = 1) have no wide-GRU kernel: the bf16-operand wide network (gru_precision = 1) reads float32 rows");
        wide_units = (hmax + 63) / 64 * 64;
    }
    const int feature_size = p->use_delta ? 2 * p->n_mfcc : p->n_mfcc;          // params.py:99-109
    if (L.n_in != feature_size && mels)
        return fail(nullptr, PE_ERR_UNSUPPORTED, "Vectorizer.mels feeds %d inputs per frame, this network takes %d", feature_size, L.n_in);
    if (L.n_in != feature_size) return fail(nullptr, PE_ERR_INVALID, "layer n_in=%d does not match feature_size=%d", L.n_in, feature_size);
    if (!L.kernel || !L.recurrent_kernel || !L.bias || !w->dense_kernel) return fail(nullptr, PE_ERR_INVALID, "null weight pointer");

    // further models: the same architecture (the K-model kernels run one network shape), checked before any device work
    for (int m = 1; m < n_models; ++m) {
        const pe_weights& wm = w[m];
        if (wm.n_layers != w->n_layers || !wm.layers)
            return fail(nullptr, PE_ERR_UNSUPPORTED, "model %d: n_layers=%d, model 0 has %d (the models of one engine share one architecture)", m, wm.n_layers, w->n_layers);
        for (int l = 0; l < w->n_layers; ++l) {
            if (wm.layers[l].units != w->layers[l].units)
                return fail(nullptr, PE_ERR_UNSUPPORTED, "model %d: layer %d units=%d, model 0 has %d (the models of one engine share one architecture)", m, l, wm.layers[l].units, w->layers[l].units);
            if (wm.layers[l].n_in != w->layers[l].n_in)
                return fail(nullptr, PE_ERR_UNSUPPORTED, "model %d: layer %d n_in=%d, model 0 has %d (the models of one engine share one front end)", m, l, wm.layers[l].n_in, w->layers[l].n_in);
            if (!wm.layers[l].kernel || !wm.layers[l].recurrent_kernel || !wm.layers[l].bias)
                return fail(nullptr, PE_ERR_INVALID, "model %d: null weight pointer", m);
        }
        if (!wm.dense_kernel) return fail(nullptr, PE_ERR_INVALID, "model %d: null weight pointer", m);
    }

    hipError_t herr = hipSetDevice(device);
    if (herr != hipSuccess) return fail(nullptr, PE_ERR_HIP, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(herr));

    {   // the library holds gfx950 code objects only, and every launch-shape rule in here (tiles per compute unit at which the
        // network changes form, frame workgroups per compute unit) was measured on MI355X: refuse anything else by name
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(nullptr, PE_ERR_UNSUPPORTED, "device %d is %s: libprecise_engine.so is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    }
    if (p->n_mfcc > kRowFloats && !wide && (p->use_delta || p->gru_precision != 0))
        return fail(nullptr, PE_ERR_UNSUPPORTED, "more than 16 %s per frame feed a float32 network without delta features only", mels ? "mel values (n_filt)" : "coefficients");
    // (bf16 operands / bf16 rows behind the general front end: the same network kernels, fed from rows of <= 16 coefficients --
    //  more than 16 were refused above)

    pe_engine* e = new pe_engine();
    e->prm = *p;
    e->device = device;
    if (!general) {
        // a stock-shape filterbank whose runs need more than the 64 lanes of the wave kernel also takes the general path
        std::vector<unsigned char> probe;
        pe_wave::Layout lprobe{};
        const std::string perr = with_real(*p, [&](auto real) { return pe_wave::build<decltype(real)>(mel_filters, p->n_filt, p->n_mfcc, probe, lprobe); });
        if (!perr.empty()) general = true;
    }
    e->general = general;
    e->row_floats = p->n_mfcc > kRowFloats ? 2 * kRowFloats : kRowFloats;
    {
        const int fl = frame_len_of(*p);
        e->carry_cap = general ? ((fl + 63) / 64 * 64 > kCarryCap ? (fl + 63) / 64 * 64 : kCarryCap) : kCarryCap;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) e->n_cus = cus;
    }
    e->n_streams = n_streams;
    e->n_tiles = (n_streams + kTileStreams - 1) / kTileStreams;
    e->n_padded = e->n_tiles * kTileStreams;
    e->units = L.units; e->n_in = p->n_mfcc; e->n_layers = w->n_layers; e->wide = wide;
    e->n_models = n_models;
    e->wide_units = wide_units;
    e->mel_host.assign(mel_filters, mel_filters + (size_t)p->n_filt * (p->n_fft / 2 + 1));
    for (int l = 0; l < w->n_layers; ++l) { e->layer_units[l] = w->layers[l].units; e->layer_n_in[l] = w->layers[l].n_in; }
    e->nets.assign((size_t)n_models, NetPack{});
    e->dec.assign((size_t)n_models, DecState{});
    if (e->prm.vectorizer == 0) e->prm.vectorizer = 2;
    // frames computed (first flen samples arrived) but not yet emitted (whole window arrived):
    // at most ceil((window - flen) / hop) of them exist at any time; T + that many rows are live
    e->ring_slots = next_pow2(p->n_features + pending_frames(e->prm));

    int rc = PE_OK;
    do {
        if ((rc = dev_alloc(e, &e->carry, (size_t)2 * e->n_padded * e->carry_cap))) break;
        if ((rc = dev_alloc(e, &e->rec, (size_t)2 * e->n_padded))) break;
        if ((rc = dev_alloc(e, &e->ring, ring_floats(e)))) break;
        for (int m = 0; m < n_models && !rc; ++m) rc = pack_model(e, e->nets[m], &w[m], wide, wide_units);
        if (rc) break;
        if (!wide) pack_projection_rows(e, L);
        // the projection rows exist for the stock-width float32 network (3 R <= 16 slots: 4 output tiles, R = 5) fed
        // from the ring; they pay while the ring stays cache-resident (256 B per frame and stream)
        e->proj_ok = !wide && p->gru_precision == 0 && !p->use_delta && gru_small_regs(L.units) == 5 && !e->proj_w_host.empty();
        e->proj_on = false;          // opt-in (pe_set_input_projection): measured no gain for the MFMA kernels at <= 4096 streams
        rc = with_real(*p, [&](auto real) { return e->general ? build_general_tables<decltype(real)>(e, mel_filters) : build_tables<decltype(real)>(e, mel_filters); });
        if (rc) break;
        if (e->proj_on && (rc = dev_alloc(e, &e->proj_ring, (size_t)e->n_tiles * e->ring_slots * kTileStreams * kProjRow))) break;
        for (auto& ev : e->ev)
            if (hipEventCreate(&ev) != hipSuccess) { rc = fail(e, PE_ERR_HIP, "hipEventCreate failed"); break; }
        if (rc) break;
        const size_t real_bytes = with_real(*p, [](auto real) { return sizeof(real); });
        const size_t lds = e->general ? general_lds_bytes(real_bytes, p->n_fft, p->n_filt, e->gtab.n_rounds)
                                      : (size_t)e->table_layout.total + (size_t)kFrameWaves * pe_wave::kScratchReals * real_bytes;
        if (lds > 64 * 1024) { rc = fail(e, PE_ERR_UNSUPPORTED, "MFCC kernel would need %zu bytes of LDS per workgroup", lds); break; }
        if ((rc = pe_clear(e, nullptr))) break;
        hipError_t se = hipDeviceSynchronize();
        if (se != hipSuccess) { rc = fail(e, PE_ERR_HIP, "device sync after init failed: %s", hipGetErrorString(se)); break; }
    } while (false);
    if (rc) {
        g_global_error = e->err;
        pe_destroy(e);
        return rc;
    }
    *out = e;
    return PE_OK;
}
}  // namespace

int pe_create(const pe_params* p, const double* mel_filters, const pe_weights* w, int32_t n_streams,
              int32_t device, pe_engine** out) {
    return create_engine(p, mel_filters, w, 1, n_streams, device, out);
}

int pe_create_models(const pe_params* p, const double* mel_filters, const pe_weights* weights, int32_t n_models, int32_t n_streams,
                     int32_t device, pe_engine** out) {
    if (out) *out = nullptr;
    if (n_models < 1 || n_models > kMaxModels) return fail(nullptr, PE_ERR_INVALID, "n_models must be in 1..%d, got %d", kMaxModels, n_models);
    if (!weights) return fail(nullptr, PE_ERR_INVALID, "null argument to pe_create_models");
    return create_engine(p, mel_filters, weights, n_models, n_streams, device, out);
}

int pe_get_n_models(const pe_engine* e) { return e ? e->n_models : -1; }

int pe_set_weights(pe_engine* e, const pe_weights* w, int32_t model) {
    if (!e) return PE_ERR_INVALID;
    if (!w || !w->layers || !w->dense_kernel) return fail(e, PE_ERR_INVALID, "null argument to pe_set_weights");
    if (model < 0 || model >= e->n_models) return fail(e, PE_ERR_INVALID, "model %d outside 0..%d", model, e->n_models - 1);
    if (w->n_layers != e->n_layers) return fail(e, PE_ERR_INVALID, "pe_set_weights: n_layers=%d, the engine's network has %d", w->n_layers, e->n_layers);
    for (int l = 0; l < e->n_layers; ++l) {
        const pe_gru_layer& L = w->layers[l];
        if (!L.kernel || !L.recurrent_kernel || !L.bias) return fail(e, PE_ERR_INVALID, "pe_set_weights: null weight pointer");
        if (L.units != e->layer_units[l] || L.n_in != e->layer_n_in[l])
            return fail(e, PE_ERR_INVALID, "pe_set_weights: layer %d is n_in=%d units=%d, the engine's is n_in=%d units=%d (a live engine takes the widths it was created with)",
                        l, L.n_in, L.units, e->layer_n_in[l], e->layer_units[l]);
    }
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    PE_HIP(e, hipDeviceSynchronize());                    // no launch may still read the buffers that are rewritten
    ++e->chain_epoch;                                     // carried chains were made with the old weights
    int rc = pack_model(e, e->nets[(size_t)model], w, e->wide, e->wide_units);
    if (rc) return rc;
    if (e->proj_ok && model == 0 && !e->general) {
        // the input-projection rows (pe_set_input_projection) live in the front end's table blob: built again from the new
        // network, written over the old blob; rows already in the feature ring get their projections again
        pack_projection_rows(e, w->layers[0]);
        rc = with_real(e->prm, [&](auto real) { return build_tables<decltype(real)>(e, e->mel_host.data()); });
        if (rc) return rc;
        if (e->proj_on)
            PE_HIP(e, launch_project_rows(e->ring, e->proj_ring, reinterpret_cast<const float*>(e->table_blob + e->table_layout.proj_w),
                                          reinterpret_cast<const float*>(e->table_blob + e->table_layout.proj_b), e->prm.n_mfcc,
                                          (long long)e->n_tiles * e->ring_slots * kTileStreams, nullptr));
        PE_HIP(e, hipStreamSynchronize(nullptr));
    }
    return PE_OK;
}

int pe_destroy(pe_engine* e) {
    if (!e) return PE_OK;
    (void)hipSetDevice(e->device);
    (void)drain_async(e);
    for (void* p : e->allocs) (void)hipFree(p);
    for (DeviceBuf* b : {&e->st_pcm, &e->st_out, &e->st_feats, &e->st_mask, &e->st_audio, &e->st_mfcc, &e->st_conf, &e->st_fired, &e->st_ids, &e->st_clips, &e->st_recs, &e->st_pred, &e->st_sim, &e->st_simw, &e->st_stats})
        if (b->p) (void)hipFree(b->p);
    for (auto& ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    if (e->s_compute) (void)hipStreamSynchronize(e->s_compute);
    if (e->s_copy) (void)hipStreamSynchronize(e->s_copy);
    for (auto& sl : e->aslot) {
        for (auto& o : sl.out) {
            if (o.pin) (void)hipHostFree(o.pin);
            if (o.dev.p) (void)hipFree(o.dev.p);
        }
        if (sl.dev_in.p) (void)hipFree(sl.dev_in.p);
        if (sl.dev_ids.p) (void)hipFree(sl.dev_ids.p);
        if (sl.pin_ids) (void)hipHostFree(sl.pin_ids);
        if (sl.copied) (void)hipEventDestroy(sl.copied);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (e->ev_user) (void)hipEventDestroy(e->ev_user);
    if (e->s_copy) (void)hipStreamDestroy(e->s_copy);
    if (e->s_compute) (void)hipStreamDestroy(e->s_compute);
    for (auto& r : e->pinned) (void)hipHostFree(r.first);
    delete e;
    return PE_OK;
}

int pe_clear(pe_engine* e, const uint8_t* mask_host) {
    if (!e) return PE_ERR_INVALID;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const uint8_t* mask_dev = nullptr;
    if (mask_host) {
        int rc = ensure(e, e->st_mask, (size_t)e->n_streams);
        if (rc) return rc;
        PE_HIP(e, hipMemcpy(e->st_mask.p, mask_host, (size_t)e->n_streams, hipMemcpyHostToDevice));
        mask_dev = static_cast<const uint8_t*>(e->st_mask.p);
    }
    // (a masked clear leaves the other streams' leftovers where they are: out of kept chunks first; a full clear empties them)
    if (mask_dev) { int frc = flush_kept(e, nullptr); if (frc) return frc; }
    else { e->kept = nullptr; e->kept_chunk = 0; }
    uint32_t call = 0;
    { int crc = begin_state_call(e, nullptr, &call); if (crc) return crc; }
    ClearArgs a{e->n_padded, e->ring_slots, mask_dev, state_of(e, call), e->ring, e->prm.ring_precision, e->activation,
                e->proj_on ? e->proj_ring : nullptr,
                e->proj_on ? reinterpret_cast<const float*>(e->table_blob + e->table_layout.proj_b) : nullptr, e->row_floats};
    if (mask_dev) a.n_streams = e->n_streams;
    PE_HIP(e, launch_clear(a, nullptr));
    if (e->activation)                              // the further models' trigger rows (n_models - 1 of them)
        PE_HIP(e, launch_clear_activation(mask_dev, e->activation, a.n_streams, e->n_padded, e->n_models - 1, nullptr));
    PE_HIP(e, hipStreamSynchronize(nullptr));
    return PE_OK;
}

int pe_update_device(pe_engine* e, const int16_t* pcm_dev, int32_t chunk, float* raw_out_dev, void* stream) {
    int rc = check_chunk(e, pcm_dev, chunk);
    if (rc) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    if (!raw_out_dev) return fail(e, PE_ERR_INVALID, "raw_out_dev is null");
    note_user_stream(e, stream);
    return do_update(e, pcm_dev, chunk, raw_out_dev, nullptr, static_cast<hipStream_t>(stream));
}

// The same update for a caller whose chunks outlive the call (a ring of resident PCM slabs, a capture buffer written ahead):
// the samples left over toward the next frame stay in pcm_dev instead of being copied to the engine's carry, and the next
// call reads the head of its first frame from there.  Any other entry point may follow: it finds the leftovers (one small
// copy launch moves them to the carry first).  Falls back to pe_update_device for chunks that cannot hold a leftover.
int pe_update_device_keep(pe_engine* e, const int16_t* pcm_dev, int32_t chunk, float* raw_out_dev, void* stream) {
    int rc = check_chunk(e, pcm_dev, chunk);
    if (rc) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    if (!raw_out_dev) return fail(e, PE_ERR_INVALID, "raw_out_dev is null");
    note_user_stream(e, stream);
    return do_update(e, pcm_dev, chunk, raw_out_dev, nullptr, static_cast<hipStream_t>(stream), nullptr, 0, true);
}

int pe_update_vectors_device(pe_engine* e, const int16_t* pcm_dev, int32_t chunk, float* feats_out_dev, void* stream) {
    int rc = check_chunk(e, pcm_dev, chunk);
    if (rc) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    note_user_stream(e, stream);
    return do_update(e, pcm_dev, chunk, nullptr, feats_out_dev, static_cast<hipStream_t>(stream));
}

int pe_run_device(pe_engine* e, float* raw_out_dev, void* stream) {
    if (!e || !raw_out_dev) return fail(e, PE_ERR_INVALID, "null argument to pe_run_device");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    note_user_stream(e, stream);
    return launch_gru_ring(e, raw_out_dev, static_cast<hipStream_t>(stream));
}

int pe_update(pe_engine* e, const int16_t* pcm_host, int32_t chunk, float* raw_out_host) {
    int rc = check_chunk(e, pcm_host, chunk);
    if (rc) return rc;
    if (!raw_out_host) return fail(e, PE_ERR_INVALID, "raw_out_host is null");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const size_t pcm_bytes = (size_t)e->n_streams * chunk * sizeof(int16_t);
    if ((rc = ensure(e, e->st_pcm, pcm_bytes))) return rc;
    const size_t out_bytes = (size_t)e->n_models * e->n_streams * sizeof(float);
    if ((rc = ensure(e, e->st_out, out_bytes))) return rc;
    PE_HIP(e, hipMemcpy(e->st_pcm.p, pcm_host, pcm_bytes, hipMemcpyHostToDevice));
    if ((rc = do_update(e, static_cast<const int16_t*>(e->st_pcm.p), chunk, static_cast<float*>(e->st_out.p), nullptr, nullptr))) return rc;
    PE_HIP(e, hipMemcpy(raw_out_host, e->st_out.p, out_bytes, hipMemcpyDeviceToHost));
    return PE_OK;
}

// Streams that advance independently (network_runner.py:125-146: every Listener takes chunks at its own pace; one engine
// process per client, runner/precise_runner/runner.py:54-67): the n_active streams named in stream_ids take one chunk each,
// every other stream keeps its leftover samples, counters and feature window untouched and gets no output.
int pe_update_subset_device(pe_engine* e, const int32_t* stream_ids_dev, int32_t n_active, const int16_t* pcm_dev, int32_t chunk,
                            float* raw_out_dev, void* stream) {
    if (!e) return PE_ERR_INVALID;
    if (n_active < 0 || n_active > e->n_streams) return fail(e, PE_ERR_INVALID, "n_active=%d outside 0..%d", n_active, e->n_streams);
    if (n_active == 0) return PE_OK;                 // nobody has audio: nothing moves
    int rc = check_chunk(e, pcm_dev, chunk);
    if (rc) return rc;
    if (!stream_ids_dev || !raw_out_dev) return fail(e, PE_ERR_INVALID, "null argument to pe_update_subset_device");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    note_user_stream(e, stream);
    return do_update(e, pcm_dev, chunk, raw_out_dev, nullptr, static_cast<hipStream_t>(stream), stream_ids_dev, n_active);
}

int pe_update_subset(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const int16_t* pcm_host, int32_t chunk, float* raw_out_host) {
    if (!e) return PE_ERR_INVALID;
    if (n_active < 0 || n_active > e->n_streams) return fail(e, PE_ERR_INVALID, "n_active=%d outside 0..%d", n_active, e->n_streams);
    if (n_active == 0) return PE_OK;
    int rc = check_chunk(e, pcm_host, chunk);
    if (rc) return rc;
    if (!stream_ids_host || !raw_out_host) return fail(e, PE_ERR_INVALID, "null argument to pe_update_subset");
    // the host entry point checks what the device one cannot
    if ((rc = check_ids(e, stream_ids_host, n_active))) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const size_t pcm_bytes = (size_t)n_active * chunk * sizeof(int16_t), out_bytes = (size_t)e->n_models * n_active * sizeof(float), id_bytes = (size_t)n_active * sizeof(int32_t);
    if ((rc = ensure(e, e->st_pcm, pcm_bytes))) return rc;
    if ((rc = ensure(e, e->st_out, out_bytes))) return rc;
    if ((rc = ensure(e, e->st_ids, id_bytes))) return rc;
    PE_HIP(e, hipMemcpy(e->st_ids.p, stream_ids_host, id_bytes, hipMemcpyHostToDevice));
    PE_HIP(e, hipMemcpy(e->st_pcm.p, pcm_host, pcm_bytes, hipMemcpyHostToDevice));
    if ((rc = do_update(e, static_cast<const int16_t*>(e->st_pcm.p), chunk, static_cast<float*>(e->st_out.p), nullptr, nullptr,
                        static_cast<const int32_t*>(e->st_ids.p), n_active))) return rc;
    PE_HIP(e, hipMemcpy(raw_out_host, e->st_out.p, out_bytes, hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_host_alloc(pe_engine* e, size_t bytes, void** out) {
    if (!e || !out || bytes == 0) return fail(e, PE_ERR_INVALID, "bad arguments to pe_host_alloc");
    PE_HIP(e, hipSetDevice(e->device));
    void* p = nullptr;
    hipError_t err = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (err != hipSuccess) return fail(e, PE_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    e->pinned.emplace_back(static_cast<char*>(p), bytes);
    *out = p;
    return PE_OK;
}

int pe_host_free(pe_engine* e, void* p) {
    if (!e || !p) return PE_ERR_INVALID;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);                                      // an update in flight may still read from / write to it
    for (auto it = e->pinned.begin(); it != e->pinned.end(); ++it)
        if (it->first == static_cast<char*>(p)) {
            e->pinned.erase(it);
            PE_HIP(e, hipHostFree(p));
            return PE_OK;
        }
    return fail(e, PE_ERR_INVALID, "pe_host_free: not a pe_host_alloc'ed pointer of this engine");
}

namespace {
// One update through the host-fed pipeline (pe_update_async: every stream, raw outputs; pe_update_subset_async: the streams
// ids_host[0 .. n_active) or, ids_host null, every stream; decoded confidence and activations on request).  The caller has
// checked every argument: from here on only the runtime can fail.
int update_async(pe_engine* e, const char* who, const int32_t* ids_host, int n_active, const int16_t* pcm_host, int chunk,
                 float* raw_out_host, double* conf_out_host, unsigned char* fired_out_host) {
    int rc;
    if ((rc = async_init(e))) return rc;
    pe_engine::AsyncSlot& sl = e->aslot[e->async_next % pe_engine::kAsyncDepth];
    if ((rc = finish_slot(e, sl))) return rc;          // the ring is full: the oldest update is delivered first
    const size_t rows = (size_t)e->n_models * n_active;
    const size_t pcm_bytes = (size_t)n_active * chunk * sizeof(int16_t), id_bytes = (size_t)n_active * sizeof(int32_t);
    if ((rc = ensure(e, sl.dev_in, pcm_bytes))) return rc;
    if (ids_host) {
        // (a copy of the ids in pinned memory of the slot: the caller's list is free again at once)
        if ((rc = ensure(e, sl.dev_ids, id_bytes))) return rc;
        if ((rc = ensure_pinned(e, &sl.pin_ids, &sl.pin_ids_bytes, id_bytes))) return rc;
        std::memcpy(sl.pin_ids, ids_host, id_bytes);
    }
    // (pageable memory: hipMemcpyAsync stages it through the runtime's own pinned buffers and returns once the last piece is
    //  staged -- the caller gets its buffer back at the return of this call; measured: 207 us per 8.4 MB update that
    //  way against 295 us with a memcpy into a pinned ring of the engine's own, 165 us zero-copy from pe_host_alloc'ed memory.
    //  Memory the runtime knows as pinned -- pe_host_alloc, but also hipHostRegister / torch pin_memory -- is read by the DMA
    //  AFTER this call returns: such a buffer must stay untouched until the update is delivered)
    void* const user[3] = {raw_out_host, conf_out_host, fired_out_host};
    const size_t bytes[3] = {rows * sizeof(float), rows * sizeof(double), rows};
    for (int i = 0; i < 3; ++i) {
        pe_engine::AsyncSlot::Out& o = sl.out[i];
        o.user = nullptr;                              // (set when the update is in flight)
        if (!user[i]) continue;
        if ((rc = ensure(e, o.dev, bytes[i]))) return rc;
        o.direct = is_pinned(e, user[i], bytes[i]);
        if (!o.direct && (rc = ensure_pinned(e, &o.pin, &o.pin_bytes, bytes[i]))) return rc;
    }
    const bool decode = conf_out_host || fired_out_host;
    bool every_trigger = true;                          // a model without a trigger leaves its rows of `fired` alone: zeros
    for (const DecState& d : e->dec) every_trigger = every_trigger && d.on;
    // state-moving work the caller queued through a *_device entry point (on the NULL stream or its own) comes first
    if (e->user_dirty) {
        PE_HIP(e, hipEventRecord(e->ev_user, e->last_user_stream));
        PE_HIP(e, hipStreamWaitEvent(e->s_compute, e->ev_user, 0));
        e->user_dirty = false;
    }
    // From the first enqueue on, a failure must not leave half an update behind: both streams are drained, the slot stays
    // free, and the error goes to the caller (the streams' state may then be one update ahead of what was delivered --
    // the message says so; pe_clear restarts the streams).
    auto enqueue = [&]() -> int {
        // This slot's device chunk may still be read by the update AFTER the one the slot last carried.  Only a full update
        // leaves its leftovers in its chunk (do_update(..., keep); a subset update writes the carry), and only the very next
        // update reads them there: a full one as the `head` of its first frames, a subset one through flush_kept, which it
        // runs on the compute stream in front of its own launches.  Either way that reader is the update in the next slot of
        // the ring, and its `done` event lies behind everything it launched -- so, for any mix of full and subset updates,
        // that update must be through before the copy overwrites the chunk (a slot that is not busy was delivered: through)
        pe_engine::AsyncSlot& reader = e->aslot[(e->async_next + 1) % pe_engine::kAsyncDepth];
        if (reader.busy) PE_HIP(e, hipStreamWaitEvent(e->s_copy, reader.done, 0));
        PE_HIP(e, hipMemcpyAsync(sl.dev_in.p, pcm_host, pcm_bytes, hipMemcpyHostToDevice, e->s_copy));
        PE_HIP(e, hipEventRecord(sl.copied, e->s_copy));
        PE_HIP(e, hipStreamWaitEvent(e->s_compute, sl.copied, 0));
        // the ids cross PCIe on the COMPUTE stream, in front of the update that reads them: the copy stream is what bounds the
        // pipeline, and a second transfer there costs its fixed latency on every update (measured at 4096 ids beside 8 MB of
        // audio: 183.2 us per update against 170.7 us for pe_update_async; here: 169.1 against 168.2, profiles/subset_async)
        if (ids_host) PE_HIP(e, hipMemcpyAsync(sl.dev_ids.p, sl.pin_ids, id_bytes, hipMemcpyHostToDevice, e->s_compute));
        const int32_t* const ids_dev = ids_host ? static_cast<const int32_t*>(sl.dev_ids.p) : nullptr;
        float* const raw_dev = static_cast<float*>(sl.out[0].dev.p);
        int urc = do_update(e, static_cast<const int16_t*>(sl.dev_in.p), chunk, raw_dev, nullptr, e->s_compute, ids_dev, ids_dev ? n_active : 0, true);
        if (urc) return urc;
        if (decode) {
            double* const conf_dev = conf_out_host ? static_cast<double*>(sl.out[1].dev.p) : nullptr;
            unsigned char* const fired_dev = fired_out_host ? static_cast<unsigned char*>(sl.out[2].dev.p) : nullptr;
            if (fired_dev && !every_trigger) PE_HIP(e, hipMemsetAsync(fired_dev, 0, rows, e->s_compute));
            if ((urc = launch_decode_rows(e, ids_dev, n_active, raw_dev, conf_dev, fired_dev, e->s_compute))) return urc;
        }
        for (int i = 0; i < 3; ++i)
            if (user[i]) PE_HIP(e, hipMemcpyAsync(sl.out[i].direct ? user[i] : sl.out[i].pin, sl.out[i].dev.p, bytes[i], hipMemcpyDeviceToHost, e->s_compute));
        PE_HIP(e, hipEventRecord(sl.done, e->s_compute));
        return PE_OK;
    };
    if ((rc = enqueue())) {
        const std::string why = e->err;
        (void)hipStreamSynchronize(e->s_copy);
        (void)hipStreamSynchronize(e->s_compute);
        return fail(e, rc, "%s: %s (this update was not delivered; the engine's streams were drained)", who, why.c_str());
    }
    for (int i = 0; i < 3; ++i) { sl.out[i].user = user[i]; sl.out[i].bytes = bytes[i]; }
    sl.busy = true;
    ++e->async_inflight;
    ++e->async_next;
    return PE_OK;
}
}  // namespace

int pe_update_async(pe_engine* e, const int16_t* pcm_host, int32_t chunk, float* raw_out_host) {
    int rc = check_chunk(e, pcm_host, chunk);
    if (rc) return rc;
    if (!raw_out_host) return fail(e, PE_ERR_INVALID, "raw_out_host is null");
    PE_HIP(e, hipSetDevice(e->device));
    return update_async(e, "pe_update_async", nullptr, e->n_streams, pcm_host, chunk, raw_out_host, nullptr, nullptr);
}

// The pipeline for streams that advance on their own (pe_update_subset's update, then ONE decode launch over the slot's
// raw outputs when conf or fired is asked for -- it moves the named streams' triggers only -- then the copies back).
// stream_ids_host null: every stream (n_active = n_streams), which is pe_update_async's update plus the decode.
int pe_update_subset_async(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const int16_t* pcm_host, int32_t chunk,
                           float* raw_out_host, double* conf_out_host, unsigned char* fired_out_host) {
    if (!e) return fail(e, PE_ERR_INVALID, "null argument to pe_update_subset_async");
    if (n_active < 0 || n_active > e->n_streams) return fail(e, PE_ERR_INVALID, "n_active=%d outside 0..%d", n_active, e->n_streams);
    if (!stream_ids_host && n_active != e->n_streams)
        return fail(e, PE_ERR_INVALID, "stream_ids is null (every stream) but n_active=%d is not n_streams=%d", n_active, e->n_streams);
    if (n_active == 0) return PE_OK;                 // nobody has audio: nothing moves, nothing is enqueued
    int rc = check_chunk(e, pcm_host, chunk);
    if (rc) return rc;
    if (!raw_out_host) return fail(e, PE_ERR_INVALID, "raw_out_host is null");
    if ((conf_out_host || fired_out_host) && (rc = check_decoder(e))) return rc;
    if (stream_ids_host && (rc = check_ids(e, stream_ids_host, n_active))) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    return update_async(e, "pe_update_subset_async", stream_ids_host, n_active, pcm_host, chunk, raw_out_host, conf_out_host, fired_out_host);
}

int pe_wait(pe_engine* e) {
    if (!e) return PE_ERR_INVALID;
    PE_HIP(e, hipSetDevice(e->device));
    return drain_async(e);
}

int pe_update_vectors(pe_engine* e, const int16_t* pcm_host, int32_t chunk, float* feats_out_host) {
    int rc = check_chunk(e, pcm_host, chunk);
    if (rc) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const size_t pcm_bytes = (size_t)e->n_streams * chunk * sizeof(int16_t);
    const size_t feat_bytes = (size_t)e->n_streams * e->prm.n_features * e->prm.n_mfcc * sizeof(float);
    if ((rc = ensure(e, e->st_pcm, pcm_bytes))) return rc;
    if (feats_out_host && (rc = ensure(e, e->st_feats, feat_bytes))) return rc;
    PE_HIP(e, hipMemcpy(e->st_pcm.p, pcm_host, pcm_bytes, hipMemcpyHostToDevice));
    if ((rc = do_update(e, static_cast<const int16_t*>(e->st_pcm.p), chunk, nullptr,
                        feats_out_host ? static_cast<float*>(e->st_feats.p) : nullptr, nullptr))) return rc;
    if (feats_out_host) PE_HIP(e, hipMemcpy(feats_out_host, e->st_feats.p, feat_bytes, hipMemcpyDeviceToHost));
    else PE_HIP(e, hipStreamSynchronize(nullptr));
    return PE_OK;
}

int pe_get_vectors(pe_engine* e, float* feats_out_host) {
    if (!e || !feats_out_host) return fail(e, PE_ERR_INVALID, "null argument to pe_get_vectors");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    int rc;
    const size_t feat_bytes = (size_t)e->n_streams * e->prm.n_features * e->prm.n_mfcc * sizeof(float);
    if ((rc = ensure(e, e->st_feats, feat_bytes))) return rc;
    GatherArgs g{e->n_streams, e->prm.n_features, e->prm.n_mfcc, e->ring_slots, e->prm.ring_precision, e->ring, state_of(e, e->call_no + 1u), static_cast<float*>(e->st_feats.p), e->row_floats};
    PE_HIP(e, launch_gather(g, nullptr));
    PE_HIP(e, hipMemcpy(feats_out_host, e->st_feats.p, feat_bytes, hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_set_vectors(pe_engine* e, const float* feats_host) {
    if (!e || !feats_host) return fail(e, PE_ERR_INVALID, "null argument to pe_set_vectors");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    int rc;
    if ((rc = pe_clear(e, nullptr))) return rc;
    const size_t feat_bytes = (size_t)e->n_streams * e->prm.n_features * e->prm.n_mfcc * sizeof(float);
    if ((rc = ensure(e, e->st_feats, feat_bytes))) return rc;
    PE_HIP(e, hipMemcpy(e->st_feats.p, feats_host, feat_bytes, hipMemcpyHostToDevice));
    uint32_t call = 0;
    if ((rc = begin_state_call(e, nullptr, &call))) return rc;
    GatherArgs g{e->n_streams, e->prm.n_features, e->prm.n_mfcc, e->ring_slots, e->prm.ring_precision, e->ring, state_of(e, call), static_cast<float*>(e->st_feats.p), e->row_floats};
    PE_HIP(e, launch_scatter(g, nullptr));
    if (e->proj_on)
        PE_HIP(e, launch_project_rows(e->ring, e->proj_ring, reinterpret_cast<const float*>(e->table_blob + e->table_layout.proj_w),
                                      reinterpret_cast<const float*>(e->table_blob + e->table_layout.proj_b), e->prm.n_mfcc,
                                      (long long)e->n_tiles * e->ring_slots * kTileStreams, nullptr));
    PE_HIP(e, hipStreamSynchronize(nullptr));
    return PE_OK;
}

int pe_predict_device(pe_engine* e, const float* feats_dev, int32_t n, float* out_dev, void* stream) {
    if (!e) return PE_ERR_INVALID;
    if (n < 0 || (n > 0 && (!feats_dev || !out_dev))) return fail(e, PE_ERR_INVALID, "bad arguments to pe_predict_device");
    if (n == 0) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    GruArgs a = gru_args(e);
    a.n_streams = n;
    a.waves_per_tile = 1;
    a.feats = feats_dev;
    a.out = out_dev;
    { int nrc = launch_networks(e, a, 0, static_cast<hipStream_t>(stream), n); if (nrc) return nrc; }
    return PE_OK;
}

int pe_predict(pe_engine* e, const float* feats_host, int32_t n, float* out_host) {
    if (!e) return PE_ERR_INVALID;
    if (n < 0 || (n > 0 && (!feats_host || !out_host))) return fail(e, PE_ERR_INVALID, "bad arguments to pe_predict");
    if (n == 0) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    int rc;
    const size_t fb = (size_t)n * e->prm.n_features * window_floats(e) * sizeof(float);
    if ((rc = ensure(e, e->st_feats, fb))) return rc;
    if ((rc = ensure(e, e->st_out, (size_t)e->n_models * n * sizeof(float)))) return rc;
    PE_HIP(e, hipMemcpy(e->st_feats.p, feats_host, fb, hipMemcpyHostToDevice));
    if ((rc = pe_predict_device(e, static_cast<const float*>(e->st_feats.p), n, static_cast<float*>(e->st_out.p), nullptr))) return rc;
    PE_HIP(e, hipMemcpy(out_host, e->st_out.p, (size_t)e->n_models * n * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

namespace {
// Whole buffer: every frame of the n_samples float64 samples in st_audio, to whichever of the three outputs is not null
// (float64 coefficients / float32 network rows / float64 log-mel energies)
int launch_buffer_front_end(pe_engine* e, int64_t n_samples, int64_t n_frames, double* dev_out, float* dev_rows, double* dev_mels) {
    return with_real(e->prm, [&](auto real) -> int {
        using R = decltype(real);
        const double* audio = static_cast<const double*>(e->st_audio.p);
        if (e->general) {
            GeneralOfflineArgs<R> a{geom(e), e->gtab, audio, n_frames, dev_out, dev_rows, dev_mels, e->row_floats};
            PE_HIP(e, launch_general_offline(a, e->n_cus, nullptr, mel_rows(e)));
        } else {
            MfccOfflineArgs<R> a{geom(e), audio, n_samples, n_frames, dev_out, dev_rows, dev_mels};
            PE_HIP(e, launch_mfcc_offline(a, tables<R>(e), e->n_cus, nullptr, mel_rows(e)));
        }
        return PE_OK;
    });
}

int vectorize_buffer(pe_engine* e, const double* audio_host, int64_t n_samples, double* feats_out_host,
                     int64_t max_frames, int64_t* n_frames_out, bool mels) {
    if (!e || !n_frames_out) return fail(e, PE_ERR_INVALID, "null argument to pe_vectorize_*");
    if (n_samples < 0 || (n_samples > 0 && !audio_host)) return fail(e, PE_ERR_INVALID, "bad audio buffer");
    const int64_t n_frames = frames_of_buffer(e->prm, n_samples);
    *n_frames_out = n_frames;
    if (n_frames == 0) return PE_OK;
    if (!feats_out_host || max_frames < n_frames) return fail(e, PE_ERR_INVALID, "output holds %lld frames, need %lld", (long long)max_frames, (long long)n_frames);
    PE_HIP(e, hipSetDevice(e->device));
    int rc;
    const int width = mels ? e->prm.n_filt : e->prm.n_mfcc;
    const size_t ab = (size_t)n_samples * sizeof(double), fb = (size_t)n_frames * width * sizeof(double);
    if ((rc = ensure(e, e->st_audio, ab))) return rc;
    if ((rc = ensure(e, e->st_mfcc, fb))) return rc;
    PE_HIP(e, hipMemcpy(e->st_audio.p, audio_host, ab, hipMemcpyHostToDevice));
    double* dev_out = static_cast<double*>(e->st_mfcc.p);
    if ((rc = launch_buffer_front_end(e, n_samples, n_frames, mels ? nullptr : dev_out, nullptr, mels ? dev_out : nullptr))) return rc;
    PE_HIP(e, hipMemcpy(feats_out_host, e->st_mfcc.p, fb, hipMemcpyDeviceToHost));
    return PE_OK;
}
}  // namespace

int pe_vectorize_raw(pe_engine* e, const double* audio_host, int64_t n_samples, double* feats_out_host,
                     int64_t max_frames, int64_t* n_frames_out) {
    return vectorize_buffer(e, audio_host, n_samples, feats_out_host, max_frames, n_frames_out, false);
}

int pe_vectorize_mels(pe_engine* e, const double* audio_host, int64_t n_samples, double* mels_out_host,
                      int64_t max_frames, int64_t* n_frames_out) {
    return vectorize_buffer(e, audio_host, n_samples, mels_out_host, max_frames, n_frames_out, true);
}

int pe_evaluate(pe_engine* e, const double* audio_host, int64_t n_samples, int32_t hop_frames, float* out_host,
                int64_t max_windows, int64_t* n_windows_out) {
    if (!e || !n_windows_out) return fail(e, PE_ERR_INVALID, "null argument to pe_evaluate");
    if (hop_frames < 1) return fail(e, PE_ERR_INVALID, "hop_frames must be >= 1 (chunk_size // hop_samples)");
    if (n_samples < 0 || (n_samples > 0 && !audio_host)) return fail(e, PE_ERR_INVALID, "bad audio buffer");
    const int64_t T = e->prm.n_features;
    const int64_t n_frames = frames_of_buffer(e->prm, n_samples);
    // simulate.py:96-99: windows end at frame i for i in range(T, n_frames, hop_frames)
    const int64_t n_windows = n_frames > T ? (n_frames - T + hop_frames - 1) / hop_frames : 0;
    *n_windows_out = n_windows;
    if (n_windows == 0) return PE_OK;
    if (!out_host || max_windows < n_windows) return fail(e, PE_ERR_INVALID, "output holds %lld windows, need %lld", (long long)max_windows, (long long)n_windows);
    if (n_windows > 0x7fffffff) return fail(e, PE_ERR_INVALID, "too many windows");
    PE_HIP(e, hipSetDevice(e->device));
    int rc;
    const size_t ab = (size_t)n_samples * sizeof(double), rb = (size_t)n_frames * e->row_floats * sizeof(float);
    if ((rc = ensure(e, e->st_audio, ab))) return rc;
    if ((rc = ensure(e, e->st_feats, rb))) return rc;
    if ((rc = ensure(e, e->st_out, (size_t)e->n_models * n_windows * sizeof(float)))) return rc;
    PE_HIP(e, hipMemcpy(e->st_audio.p, audio_host, ab, hipMemcpyHostToDevice));
    if ((rc = launch_buffer_front_end(e, n_samples, n_frames, nullptr, static_cast<float*>(e->st_feats.p), nullptr))) return rc;
    GruArgs g = gru_args(e);
    g.n_streams = (int)n_windows;
    g.feats = static_cast<const float*>(e->st_feats.p);
    g.row_stride = hop_frames;
    g.out = static_cast<float*>(e->st_out.p);
    g.waves_per_tile = 1;
    if ((rc = launch_networks(e, g, 2, nullptr, n_windows))) return rc;
    for (int m = 0; m < e->n_models; ++m)           // out_host[K][max_windows]
        PE_HIP(e, hipMemcpy(out_host + (size_t)m * max_windows, static_cast<float*>(e->st_out.p) + (size_t)m * n_windows, (size_t)n_windows * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

namespace {
// ---- statistics (kernels: stats_device.h) -------------------------------------------------------------
static_assert(sizeof(pe_stats_summary) == sizeof(StatsSummary) && sizeof(StatsSummary) == 72, "pe_stats_summary is what the device writes");
static_assert(sizeof(pe_stats_count) == 32, "four counts per (row, threshold)");

struct StatsRequest {
    const double* thresholds; int32_t n_thresholds, compare;
    pe_stats_count* counts_out; pe_stats_summary* summary_out;
};
// what is wrong with a request over n samples, or nothing; targets_host null: a resident set, checked when it was uploaded
bool stats_request_wrong(std::string& why, const char* who, const StatsRequest& q, const float* targets_host, int64_t n) {
    char buf[256] = "";
    const auto say = [&](const char* fmt, auto... v) { snprintf(buf, sizeof buf, fmt, who, v...); why = buf; return true; };
    if (!q.summary_out) return say("null argument to %s (summary_out)");
    if (n < 1 || n > 0x7fffffffll) return say("%s: n must lie in 1..2^31 - 1, got %lld", (long long)n);
    if (q.compare != PE_STATS_COMPARE_F32 && q.compare != PE_STATS_COMPARE_F64) return say("%s: compare must be 0 (float32) or 1 (float64), got %d", q.compare);
    if (q.n_thresholds < 0 || q.n_thresholds > kStatsMaxThresholds) return say("%s: n_thresholds must lie in 0..4096, got %d", q.n_thresholds);
    if (q.n_thresholds > 0 && (!q.thresholds || !q.counts_out)) return say("null argument to %s (thresholds / counts_out with n_thresholds = %d)", q.n_thresholds);
    for (int32_t j = 0; j < q.n_thresholds; ++j) {
        if (q.thresholds[j] != q.thresholds[j]) return say("%s: thresholds[%d] is NaN", j);
        if (j && q.thresholds[j] < q.thresholds[j - 1]) return say("%s: thresholds decrease at %d (%g after %g)", j, q.thresholds[j], q.thresholds[j - 1]);
    }
    if (targets_host)
        for (int64_t i = 0; i < n; ++i)
            if (!(targets_host[i] >= 0.0f && targets_host[i] <= 1.0f)) return say("%s: targets[%lld] = %g is outside [0, 1]", (long long)i, (double)targets_host[i]);
    return false;
}
// one call's device scratch, as byte offsets: thresholds | histogram | counters | word sums x, d | summaries | the caller's
// targets and predictions where they are not on the device yet
struct StatsScratch {
    size_t thresholds, hist, counters, word_x, word_d, summary, targets, probs, total;
    uint32_t n_words;
};
StatsScratch stats_scratch(int rows, int64_t n, int n_thresholds, bool with_targets, bool with_probs) {
    StatsScratch s{};
    s.n_words = (uint32_t)((n + 63) / 64);
    const size_t words = (size_t)rows * s.n_words * sizeof(double);
    s.thresholds = 0;
    s.hist = s.thresholds + (size_t)n_thresholds * sizeof(double);
    s.counters = s.hist + (n_thresholds ? (size_t)rows * 4 * ((size_t)n_thresholds + 1) * sizeof(unsigned long long) : 0);
    s.word_x = s.counters + (size_t)rows * kStatsCounters * sizeof(unsigned long long);
    s.word_d = s.word_x + words;
    s.summary = s.word_d + words;
    s.targets = s.summary + (size_t)rows * sizeof(StatsSummary);
    s.probs = s.targets + (with_targets ? ((size_t)n * sizeof(float) + 7) / 8 * 8 : 0);
    s.total = s.probs + (with_probs ? (size_t)rows * (size_t)n * sizeof(float) : 0);
    return s;
}
// the kernels over predictions and targets that are on the device, and the results back: the summaries as they are, the
// counts as the histogram's sums from the top (a sample lies above thresholds[j] when its bin is > j)
hipError_t stats_run(char* scratch, const StatsScratch& s, const float* probs_dev, int64_t stride, const float* targets_dev, int64_t n,
                     int rows, const StatsRequest& q) {
    const int T = q.n_thresholds;
    const size_t nb = (size_t)T + 1;
    hipError_t err;
    if (T && (err = hipMemcpy(scratch + s.thresholds, q.thresholds, (size_t)T * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return err;
    if ((err = hipMemsetAsync(scratch + s.hist, 0, s.word_x - s.hist, nullptr)) != hipSuccess) return err;       // histogram and counters
    StatsArgs a{};
    a.probs = probs_dev; a.stride = stride; a.targets = targets_dev; a.n = n; a.n_words = s.n_words;
    a.thresholds = T ? reinterpret_cast<const double*>(scratch + s.thresholds) : nullptr; a.n_thresholds = T;
    a.hist = T ? reinterpret_cast<unsigned long long*>(scratch + s.hist) : nullptr;
    a.counters = reinterpret_cast<unsigned long long*>(scratch + s.counters);
    a.word_x = reinterpret_cast<double*>(scratch + s.word_x);
    a.word_d = reinterpret_cast<double*>(scratch + s.word_d);
    a.summary = reinterpret_cast<StatsSummary*>(scratch + s.summary);
    if ((err = launch_stats(a, rows, q.compare, nullptr)) != hipSuccess) return err;
    std::vector<unsigned long long> hist(T ? (size_t)rows * 4 * nb : 0);
    if (T && (err = hipMemcpy(hist.data(), a.hist, hist.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost)) != hipSuccess) return err;
    if ((err = hipMemcpy(q.summary_out, a.summary, (size_t)rows * sizeof(StatsSummary), hipMemcpyDeviceToHost)) != hipSuccess) return err;
    for (int r = 0; r < rows && T; ++r) {
        const unsigned long long* h = hist.data() + (size_t)r * 4 * nb;        // [> / >=][positive / negative][nb]
        int64_t above[4] = {0, 0, 0, 0};
        for (size_t j = nb - 1; j-- > 0;) {
            for (int k = 0; k < 4; ++k) above[k] += (int64_t)h[(size_t)k * nb + j + 1];
            q.counts_out[(size_t)r * T + j] = pe_stats_count{above[0], above[1], above[2], above[3]};
        }
    }
    return hipSuccess;
}
}  // namespace

namespace {
// the front-end launch over a clip table that is on the device (pe_vectorize_clips / pe_score_clips; pe_miner_vectorize / _append)
int launch_clip_front_end(pe_engine* e, const ClipTable& ct, double* dev_out, float* dev_rows, double* dev_mels) {
    return with_real(e->prm, [&](auto real) -> int {
        using R = decltype(real);
        if (e->general) {
            GeneralClipArgs<R> a{geom(e), e->gtab, ct, dev_out, dev_rows, dev_mels, e->row_floats};
            PE_HIP(e, launch_general_clips(a, e->n_cus, nullptr, mel_rows(e)));
        } else {
            MfccClipArgs<R> a{geom(e), ct, dev_out, dev_rows, dev_mels};
            PE_HIP(e, launch_mfcc_clips(a, tables<R>(e), e->n_cus, nullptr, mel_rows(e)));
        }
        return PE_OK;
    });
}
// ... and over a recording table (pe_evaluate_clips / pe_simulate_clips; pe_miner_create)
int launch_rec_front_end(pe_engine* e, const RecTable& rt, float* dev_rows) {
    return with_real(e->prm, [&](auto real) -> int {
        using R = decltype(real);
        if (e->general) {
            GeneralRecArgs<R> a{geom(e), e->gtab, rt, dev_rows, e->row_floats};
            PE_HIP(e, launch_general_recs(a, e->n_cus, nullptr, mel_rows(e)));
        } else {
            MfccRecArgs<R> a{geom(e), rt, dev_rows};
            PE_HIP(e, launch_mfcc_recs(a, tables<R>(e), e->n_cus, nullptr, mel_rows(e)));
        }
        return PE_OK;
    });
}

// pe_vectorize_clips (feats_out_host) / pe_score_clips (score_out_host) / pe_test_clips (stats; score_out_host may be null):
// validation, then pass by pass one copy in, the front-end launch, the network launch (scores), one copy out -- and, for
// pe_test_clips, the statistics kernels once over the scores of all passes
int run_clips(pe_engine* e, const char* who, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_clips,
              int64_t max_samples, bool mels, double* feats_out_host, float* score_out_host, const StatsRequest* stats = nullptr,
              const float* targets_host = nullptr) {
    if (!e) return fail(e, PE_ERR_INVALID, "null engine handed to %s", who);
    if (n_clips < 0) return fail(e, PE_ERR_INVALID, "%s: n_clips=%d", who, n_clips);
    if (n_clips == 0) return PE_OK;
    if (!audio_host || !offsets_host || !(feats_out_host || score_out_host || stats)) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    if (sample_format != 0 && sample_format != 1) return fail(e, PE_ERR_INVALID, "%s: sample_format must be 0 (float64) or 1 (float32), got %d", who, sample_format);
    if (offsets_host[0] != 0) return fail(e, PE_ERR_INVALID, "%s: offsets[0] must be 0, got %lld", who, (long long)offsets_host[0]);
    for (int32_t c = 0; c < n_clips; ++c) {
        if (offsets_host[c + 1] < offsets_host[c]) return fail(e, PE_ERR_INVALID, "%s: offsets decrease at clip %d (%lld after %lld)", who, c, (long long)offsets_host[c + 1], (long long)offsets_host[c]);
        if (offsets_host[c + 1] == offsets_host[c]) return fail(e, PE_ERR_INVALID, "%s: clip %d is empty (the reference raises InvalidAudio: cannot vectorize empty audio)", who, c);
    }
    if (stats) {            // pe_test_clips: targets_host[n_clips]
        if (!targets_host) return fail(e, PE_ERR_INVALID, "null argument to %s (targets)", who);
        std::string wrong;
        if (stats_request_wrong(wrong, who, *stats, targets_host, n_clips)) return fail(e, PE_ERR_INVALID, "%s", wrong.c_str());
    }
    const bool score = score_out_host || stats;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    int rc;
    const int T = e->prm.n_features;
    const int width = mels ? e->prm.n_filt : e->prm.n_mfcc;
    const size_t elem = sample_format == 1 ? sizeof(float) : sizeof(double);
    if (score && (rc = ensure(e, e->st_out, (size_t)e->n_models * n_clips * sizeof(float)))) return rc;
    std::vector<ClipDesc> desc;
    std::vector<uint32_t> prefix;
    const bool t = e->timing;
    for (int32_t c0 = 0; c0 < n_clips;) {
        // the clips of this pass: at least one, then as many as stay within the byte target (and the row bound)
        int32_t c1 = c0 + 1;
        while (c1 < n_clips && (int64_t)(offsets_host[c1 + 1] - offsets_host[c0]) * (int64_t)elem <= e->clip_pass_bytes && (int64_t)(c1 + 1 - c0) * T <= kClipPassRows) ++c1;
        const int n = c1 - c0;
        const int64_t base = offsets_host[c0], n_samples = offsets_host[c1] - base;
        desc.resize((size_t)n); prefix.resize((size_t)n + 1);
        uint32_t tasks = 0;
        for (int i = 0; i < n; ++i) {
            prefix[(size_t)i] = tasks;
            desc[(size_t)i] = clip_desc(e->prm, T, offsets_host[c0 + i + 1] - base, offsets_host[c0 + i + 1] - offsets_host[c0 + i], max_samples, tasks);
        }
        prefix[(size_t)n] = tasks;
        if ((rc = ensure(e, e->st_audio, (size_t)n_samples * elem))) return rc;
        PE_HIP(e, hipMemcpy(e->st_audio.p, static_cast<const char*>(audio_host) + (size_t)base * elem, (size_t)n_samples * elem, hipMemcpyHostToDevice));
        ClipTable ct;
        PE_HIP(e, upload_task_table(e, e->st_clips, desc, prefix, e->st_audio.p, sample_format == 1 ? 1 : 0, ct, rc));
        if (rc) return rc;
        double* dev_out = nullptr;
        float* dev_rows = nullptr;
        const size_t fb = (size_t)n * T * width * sizeof(double), rb = (size_t)n * T * e->row_floats * sizeof(float);
        if (feats_out_host) { if ((rc = ensure(e, e->st_mfcc, fb))) return rc; dev_out = static_cast<double*>(e->st_mfcc.p); }
        else { if ((rc = ensure(e, e->st_feats, rb))) return rc; dev_rows = static_cast<float*>(e->st_feats.p); }
        if (t) PE_HIP(e, hipEventRecord(e->ev[0], nullptr));
        if ((rc = launch_clip_front_end(e, ct, mels ? nullptr : dev_out, dev_rows, mels ? dev_out : nullptr))) return rc;
        if (t) PE_HIP(e, hipEventRecord(e->ev[1], nullptr));
        if (feats_out_host) {
            PE_HIP(e, hipMemcpy(feats_out_host + (size_t)c0 * T * width, dev_out, fb, hipMemcpyDeviceToHost));
        } else {
            // clip c's window is rows [c T, c T + T) of the pass: the row-sequence input of pe_evaluate with a stride of T rows
            // (its deltas, use_delta, are formed inside a window: zero at the window's first row)
            GruArgs g = gru_args(e);
            g.n_streams = n;
            g.feats = dev_rows;
            g.row_stride = T;
            g.out = static_cast<float*>(e->st_out.p) + c0;          // model m: + m * n_clips
            g.waves_per_tile = 1;
            if ((rc = launch_networks(e, g, 2, nullptr, n_clips))) return rc;
        }
        if (t) { PE_HIP(e, hipEventRecord(e->ev[2], nullptr)); e->ev_valid = true; e->ev_has_gru = score; }
        c0 = c1;
    }
    if (score_out_host) PE_HIP(e, hipMemcpy(score_out_host, e->st_out.p, (size_t)e->n_models * n_clips * sizeof(float), hipMemcpyDeviceToHost));
    if (stats) {            // once, over the scores of every pass
        const StatsScratch s = stats_scratch(e->n_models, n_clips, stats->n_thresholds, true, false);
        if ((rc = ensure(e, e->st_stats, s.total))) return rc;
        char* const scratch = static_cast<char*>(e->st_stats.p);
        PE_HIP(e, hipMemcpy(scratch + s.targets, targets_host, (size_t)n_clips * sizeof(float), hipMemcpyHostToDevice));
        PE_HIP(e, stats_run(scratch, s, static_cast<const float*>(e->st_out.p), n_clips, reinterpret_cast<const float*>(scratch + s.targets), n_clips,
                            e->n_models, *stats));
    }
    return PE_OK;
}
}  // namespace

int pe_vectorize_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_clips,
                       int64_t max_samples, int32_t mels, double* feats_out_host) {
    if (e && n_clips > 0 && !feats_out_host) return fail(e, PE_ERR_INVALID, "null argument to pe_vectorize_clips");
    return run_clips(e, "pe_vectorize_clips", audio_host, sample_format, offsets_host, n_clips, max_samples, mels != 0, feats_out_host, nullptr);
}

int pe_score_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_clips,
                   int64_t max_samples, float* out_host) {
    if (e && n_clips > 0 && !out_host) return fail(e, PE_ERR_INVALID, "null argument to pe_score_clips");
    return run_clips(e, "pe_score_clips", audio_host, sample_format, offsets_host, n_clips, max_samples, false, nullptr, out_host);
}

namespace {
static_assert(sizeof(pe_sim_metric) == sizeof(SimMetric) && sizeof(SimMetric) == 32, "pe_sim_metric is what the device writes");

// what pe_simulate_scores / pe_simulate_clips compute besides predictions (null for pe_evaluate_clips)
struct SimRequest {
    double chunk_threshold, sensitivity;
    int32_t trigger_level, chunk_size;
    const double* thresholds; int32_t n_thresholds;
    pe_sim_metric* metrics_out; int64_t* buckets_out;
};
int check_sim_request(pe_engine* e, const char* who, const SimRequest& q) {
    if (!q.metrics_out) return fail(e, PE_ERR_INVALID, "null argument to %s (metrics_out)", who);
    if (q.chunk_size < 1) return fail(e, PE_ERR_INVALID, "%s: chunk_size must be >= 1, got %d", who, q.chunk_size);
    if (q.sensitivity != q.sensitivity) return fail(e, PE_ERR_INVALID, "%s: sensitivity is NaN", who);
    if (q.chunk_threshold != q.chunk_threshold) return fail(e, PE_ERR_INVALID, "%s: chunk_threshold is NaN", who);
    if (q.n_thresholds < 0 || q.n_thresholds > 4096) return fail(e, PE_ERR_INVALID, "%s: n_thresholds must lie in 0..4096, got %d", who, q.n_thresholds);
    if (q.n_thresholds > 0 && (!q.thresholds || !q.buckets_out)) return fail(e, PE_ERR_INVALID, "null argument to %s (thresholds / buckets_out with n_thresholds = %d)", who, q.n_thresholds);
    for (int32_t j = 0; j < q.n_thresholds; ++j) {
        if (q.thresholds[j] != q.thresholds[j]) return fail(e, PE_ERR_INVALID, "%s: thresholds[%d] is NaN", who, j);
        if (j && q.thresholds[j] < q.thresholds[j - 1]) return fail(e, PE_ERR_INVALID, "%s: thresholds decrease at %d (%g after %g)", who, j, q.thresholds[j], q.thresholds[j - 1]);
    }
    return PE_OK;
}
// windows of every recording as pe_evaluate counts them (simulate.py:96-99), as an exclusive prefix sum [n_rec + 1]
int recording_layout(pe_engine* e, const char* who, const int64_t* offsets, int32_t n_rec, int32_t hop_frames, std::vector<int64_t>& woff) {
    if (hop_frames < 1) return fail(e, PE_ERR_INVALID, "%s: hop_frames must be >= 1 (chunk_size // hop_samples), got %d", who, hop_frames);
    if (offsets[0] != 0) return fail(e, PE_ERR_INVALID, "%s: offsets[0] must be 0, got %lld", who, (long long)offsets[0]);
    const int64_t T = e->prm.n_features;
    woff.assign((size_t)n_rec + 1, 0);
    for (int32_t r = 0; r < n_rec; ++r) {
        if (offsets[r + 1] < offsets[r]) return fail(e, PE_ERR_INVALID, "%s: offsets decrease at recording %d (%lld after %lld)", who, r, (long long)offsets[r + 1], (long long)offsets[r]);
        const int64_t n_frames = frames_of_buffer(e->prm, offsets[r + 1] - offsets[r]);
        const int64_t n_windows = n_frames > T ? (n_frames - T + hop_frames - 1) / hop_frames : 0;
        // frames of one launch are 32-bit tasks, and a recording is never split
        if (n_frames > 0x7fffffff) return fail(e, PE_ERR_INVALID, "%s: recording %d has %lld frames, more than one pass holds (2^31 - 1)", who, r, (long long)n_frames);
        woff[(size_t)r + 1] = woff[(size_t)r] + n_windows;
        if (woff[(size_t)r + 1] > 0x7fffffff) return fail(e, PE_ERR_INVALID, "%s: more than 2^31 - 1 windows in one call (at recording %d)", who, r);
    }
    return PE_OK;
}

// the call-wide device side of a SimRequest: thresholds, a zeroed histogram [K][n_thresholds + 1], metrics [K][n_rec]
struct SimDevice {
    double* thresholds; unsigned long long* hist; SimMetric* metrics;
    double trigger_threshold; int rearm;
};
int sim_begin(pe_engine* e, const SimRequest& q, int32_t n_rec, SimDevice& d) {
    const size_t K = (size_t)e->n_models, nb = (size_t)q.n_thresholds + 1;
    const size_t tb = (size_t)q.n_thresholds * sizeof(double), hb = K * nb * sizeof(unsigned long long), mb = K * (size_t)n_rec * sizeof(SimMetric);
    int rc;
    if ((rc = ensure(e, e->st_sim, tb + hb + mb))) return rc;
    char* p = static_cast<char*>(e->st_sim.p);
    d.thresholds = reinterpret_cast<double*>(p);
    d.hist = q.n_thresholds ? reinterpret_cast<unsigned long long*>(p + tb) : nullptr;
    d.metrics = reinterpret_cast<SimMetric*>(p + tb + hb);
    d.trigger_threshold = 1.0 - q.sensitivity;                                  // runner.py:142
    d.rearm = (int)-((8 * 2048 + (int64_t)q.chunk_size - 1) / q.chunk_size);    // -(8 * 2048) // chunk_size, runner.py:150
    if (q.n_thresholds) {
        PE_HIP(e, hipMemcpy(d.thresholds, q.thresholds, tb, hipMemcpyHostToDevice));
        PE_HIP(e, hipMemset(d.hist, 0, hb));
    }
    return PE_OK;
}
// metrics and histogram back; buckets[m][j] = windows above thresholds[j] = the bins above j (a suffix sum)
int sim_end(pe_engine* e, const SimRequest& q, int32_t n_rec, const SimDevice& d) {
    const size_t K = (size_t)e->n_models, nb = (size_t)q.n_thresholds + 1;
    PE_HIP(e, hipMemcpy(q.metrics_out, d.metrics, K * (size_t)n_rec * sizeof(SimMetric), hipMemcpyDeviceToHost));
    if (!q.n_thresholds) return PE_OK;
    std::vector<unsigned long long> hist(K * nb);
    PE_HIP(e, hipMemcpy(hist.data(), d.hist, hist.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < K; ++m) {
        int64_t above = 0;
        for (size_t j = nb - 1; j-- > 0;) {
            above += (int64_t)hist[m * nb + j + 1];
            q.buckets_out[m * (nb - 1) + j] = above;
        }
    }
    return PE_OK;
}
// the metrics kernels over `n` recordings whose SimRec table and word prefix sum the caller has built on the host
int sim_launch(pe_engine* e, const SimRequest* q, const SimDevice* d, const std::vector<SimRec>& recs, const std::vector<uint32_t>& word_prefix,
               const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int64_t first_rec, int32_t n_rec_call) {
    const int n = (int)recs.size();
    const uint32_t n_words = word_prefix[(size_t)n];
    if (!q && !n_words) return PE_OK;           // nothing to compact
    const size_t K = (size_t)e->n_models, rb = (size_t)n * sizeof(SimRec), pb = ((size_t)n + 1) * sizeof(uint32_t);
    int rc;
    if ((rc = ensure(e, e->st_recs, rb + pb))) return rc;
    PE_HIP(e, hipMemcpy(e->st_recs.p, recs.data(), rb, hipMemcpyHostToDevice));
    PE_HIP(e, hipMemcpy(static_cast<char*>(e->st_recs.p) + rb, word_prefix.data(), pb, hipMemcpyHostToDevice));
    SimArgs a{};
    a.recs = static_cast<const SimRec*>(e->st_recs.p);
    a.word_prefix = reinterpret_cast<const uint32_t*>(static_cast<const char*>(e->st_recs.p) + rb);
    a.n_rec = n; a.n_words = n_words;
    a.src = src; a.src_stride = src_stride; a.dst = dst; a.dst_stride = dst_stride;
    if (q) {
        const size_t wb = K * n_words * sizeof(unsigned long long);
        if ((rc = ensure(e, e->st_simw, 2 * wb + K * n_words * sizeof(uint32_t)))) return rc;
        char* p = static_cast<char*>(e->st_simw.p);
        a.trig = reinterpret_cast<unsigned long long*>(p);
        a.partial = reinterpret_cast<double*>(p + wb);
        a.chunk_count = reinterpret_cast<uint32_t*>(p + 2 * wb);
        a.chunk_threshold = q->chunk_threshold; a.trigger_threshold = d->trigger_threshold;
        a.trigger_level = q->trigger_level; a.rearm = d->rearm;
        a.thresholds = d->thresholds; a.n_thresholds = q->n_thresholds; a.hist = d->hist;
        a.metrics = d->metrics + first_rec; a.metric_stride = n_rec_call;
    }
    PE_HIP(e, launch_simulate(a, e->n_models, e->n_cus, nullptr));
    return PE_OK;
}

// pe_evaluate_clips (q null) / pe_simulate_clips: validation, then pass by pass one copy in, the front-end launch, ONE network
// launch over the padded row layout (pe_common.h: RecDesc), the metrics kernels; one copy out at the end
int run_recordings(pe_engine* e, const char* who, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_rec,
                   int32_t hop_frames, const SimRequest* q, float* out_host, int64_t max_windows) {
    if (!e) return fail(e, PE_ERR_INVALID, "null engine handed to %s", who);
    if (n_rec < 0) return fail(e, PE_ERR_INVALID, "%s: n_rec=%d", who, n_rec);
    if (n_rec == 0) return PE_OK;
    if (!offsets_host || !audio_host || (!q && !out_host)) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    if (sample_format != 0 && sample_format != 1) return fail(e, PE_ERR_INVALID, "%s: sample_format must be 0 (float64) or 1 (float32), got %d", who, sample_format);
    int rc;
    std::vector<int64_t> woff;
    if ((rc = recording_layout(e, who, offsets_host, n_rec, hop_frames, woff))) return rc;
    if (q && (rc = check_sim_request(e, who, *q))) return rc;
    const int64_t total = woff[(size_t)n_rec];
    if (out_host && max_windows < total) return fail(e, PE_ERR_INVALID, "%s: output holds %lld windows per model, need %lld", who, (long long)max_windows, (long long)total);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const int64_t T = e->prm.n_features, hop = hop_frames;
    const size_t elem = sample_format == 1 ? sizeof(float) : sizeof(double);
    SimDevice dev{};
    if (q && (rc = sim_begin(e, *q, n_rec, dev))) return rc;
    if (out_host && (rc = ensure(e, e->st_out, (size_t)e->n_models * (size_t)total * sizeof(float)))) return rc;
    std::vector<RecDesc> desc;
    std::vector<uint32_t> prefix, word_prefix;
    std::vector<SimRec> sim;
    const bool t = e->timing;
    for (int32_t c0 = 0; c0 < n_rec;) {
        // the recordings of this pass: at least one, then as many as stay within the byte target (and 32-bit frame tasks / windows)
        desc.clear(); prefix.clear(); word_prefix.clear(); sim.clear();
        int64_t rows = 0, tasks = 0, words = 0;         // rows: the first free row, a multiple of hop_frames
        int32_t c1 = c0;
        for (; c1 < n_rec; ++c1) {
            const int64_t W = woff[(size_t)c1 + 1] - woff[(size_t)c1];
            const int64_t used = W ? (W - 1) * hop + T : 0;            // frames its windows read; without a window, none
            if (c1 > c0 && ((offsets_host[c1 + 1] - offsets_host[c0]) * (int64_t)elem > e->clip_pass_bytes || tasks + used > 0x7fffffff ||
                            (rows + used + hop) / hop > 0x7fffffff)) break;
            desc.push_back(RecDesc{offsets_host[c1] - offsets_host[c0], rows});
            sim.push_back(SimRec{rows / hop, woff[(size_t)c1] - woff[(size_t)c0], W});
            prefix.push_back((uint32_t)tasks);
            word_prefix.push_back((uint32_t)words);
            tasks += used;
            words += (W + 63) / 64;
            rows = (rows + used + hop - 1) / hop * hop;
        }
        prefix.push_back((uint32_t)tasks);
        word_prefix.push_back((uint32_t)words);
        const int n = c1 - c0;
        // windows of the launch: up to the last one of the last recording that has any; its T rows end the row buffer
        int64_t padded = 0;
        for (int i = 0; i < n; ++i) if (sim[(size_t)i].n_windows) padded = sim[(size_t)i].src0 + sim[(size_t)i].n_windows;
        if (padded > 0) {
            const int64_t base = offsets_host[c0], n_samples = offsets_host[c1] - base;
            const int64_t n_rows = (padded - 1) * hop + T;
            const size_t rb = (size_t)n_rows * e->row_floats * sizeof(float);
            if ((rc = ensure(e, e->st_audio, (size_t)n_samples * elem))) return rc;
            if ((rc = ensure(e, e->st_feats, rb))) return rc;
            if ((rc = ensure(e, e->st_pred, (size_t)e->n_models * (size_t)padded * sizeof(float)))) return rc;
            PE_HIP(e, hipMemcpy(e->st_audio.p, static_cast<const char*>(audio_host) + (size_t)base * elem, (size_t)n_samples * elem, hipMemcpyHostToDevice));
            RecTable rt;
            PE_HIP(e, upload_task_table(e, e->st_clips, desc, prefix, e->st_audio.p, sample_format == 1 ? 1 : 0, rt, rc));
            if (rc) return rc;
            PE_HIP(e, hipMemsetAsync(e->st_feats.p, 0, rb, nullptr));      // the rows between two recordings: read by the windows that are dropped
            float* dev_rows = static_cast<float*>(e->st_feats.p);
            if (t) PE_HIP(e, hipEventRecord(e->ev[0], nullptr));
            if ((rc = launch_rec_front_end(e, rt, dev_rows))) return rc;
            if (t) PE_HIP(e, hipEventRecord(e->ev[1], nullptr));
            // pe_evaluate's network launch: window w = rows [w hop_frames, + T) -- recording i's window j is window src0 + j
            GruArgs g = gru_args(e);
            g.n_streams = (int)padded;
            g.feats = dev_rows;
            g.row_stride = hop_frames;
            g.out = static_cast<float*>(e->st_pred.p);
            g.waves_per_tile = 1;
            if ((rc = launch_networks(e, g, 2, nullptr, padded))) return rc;
            if (t) { PE_HIP(e, hipEventRecord(e->ev[2], nullptr)); e->ev_valid = true; e->ev_has_gru = true; }
        }
        // (a pass without a window still has metrics: all zero)
        if ((rc = sim_launch(e, q, q ? &dev : nullptr, sim, word_prefix, static_cast<const float*>(e->st_pred.p), padded,
                             out_host ? static_cast<float*>(e->st_out.p) + woff[(size_t)c0] : nullptr, total, c0, n_rec))) return rc;
        c0 = c1;
    }
    if (out_host && total > 0)
        for (int m = 0; m < e->n_models; ++m)           // out_host[K][max_windows]
            PE_HIP(e, hipMemcpy(out_host + (size_t)m * max_windows, static_cast<float*>(e->st_out.p) + (size_t)m * total, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
    return q ? sim_end(e, *q, n_rec, dev) : PE_OK;
}
}  // namespace

int pe_evaluate_clips_layout(pe_engine* e, const int64_t* offsets_host, int32_t n_rec, int32_t hop_frames, int64_t* window_offsets_out) {
    const char* who = "pe_evaluate_clips_layout";
    if (!e) return fail(e, PE_ERR_INVALID, "null engine handed to %s", who);
    if (n_rec < 0) return fail(e, PE_ERR_INVALID, "%s: n_rec=%d", who, n_rec);
    if (!window_offsets_out || (n_rec > 0 && !offsets_host)) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    std::vector<int64_t> woff(1, 0);
    int rc;
    if (n_rec > 0 && (rc = recording_layout(e, who, offsets_host, n_rec, hop_frames, woff))) return rc;
    std::copy(woff.begin(), woff.end(), window_offsets_out);
    return PE_OK;
}

int pe_evaluate_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_rec,
                      int32_t hop_frames, float* out_host, int64_t max_windows) {
    return run_recordings(e, "pe_evaluate_clips", audio_host, sample_format, offsets_host, n_rec, hop_frames, nullptr, out_host, max_windows);
}

int pe_simulate_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_rec,
                      int32_t hop_frames, double chunk_threshold, double sensitivity, int32_t trigger_level, int32_t chunk_size,
                      const double* thresholds, int32_t n_thresholds, pe_sim_metric* metrics_out, int64_t* buckets_out,
                      float* out_host, int64_t max_windows) {
    const SimRequest q{chunk_threshold, sensitivity, trigger_level, chunk_size, thresholds, n_thresholds, metrics_out, buckets_out};
    return run_recordings(e, "pe_simulate_clips", audio_host, sample_format, offsets_host, n_rec, hop_frames, &q, out_host, max_windows);
}

int pe_simulate_scores(pe_engine* e, const float* raw_host, int64_t stride, const int64_t* window_offsets, int32_t n_rec,
                       double chunk_threshold, double sensitivity, int32_t trigger_level, int32_t chunk_size,
                       const double* thresholds, int32_t n_thresholds, pe_sim_metric* metrics_out, int64_t* buckets_out) {
    const char* who = "pe_simulate_scores";
    if (!e) return fail(e, PE_ERR_INVALID, "null engine handed to %s", who);
    if (n_rec < 0) return fail(e, PE_ERR_INVALID, "%s: n_rec=%d", who, n_rec);
    if (n_rec == 0) return PE_OK;
    if (!window_offsets || !raw_host) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    if (window_offsets[0] != 0) return fail(e, PE_ERR_INVALID, "%s: window_offsets[0] must be 0, got %lld", who, (long long)window_offsets[0]);
    for (int32_t r = 0; r < n_rec; ++r)
        if (window_offsets[r + 1] < window_offsets[r]) return fail(e, PE_ERR_INVALID, "%s: window_offsets decrease at recording %d (%lld after %lld)", who, r, (long long)window_offsets[r + 1], (long long)window_offsets[r]);
    const int64_t total = window_offsets[n_rec];
    if (total > 0x7fffffff) return fail(e, PE_ERR_INVALID, "%s: more than 2^31 - 1 windows in one call", who);
    if (stride < total) return fail(e, PE_ERR_INVALID, "%s: stride %lld is less than the %lld windows of a model", who, (long long)stride, (long long)total);
    const SimRequest q{chunk_threshold, sensitivity, trigger_level, chunk_size, thresholds, n_thresholds, metrics_out, buckets_out};
    int rc;
    if ((rc = check_sim_request(e, who, q))) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    SimDevice dev{};
    if ((rc = sim_begin(e, q, n_rec, dev))) return rc;
    if ((rc = ensure(e, e->st_pred, (size_t)e->n_models * (size_t)total * sizeof(float)))) return rc;
    if (total > 0)
        for (int m = 0; m < e->n_models; ++m)
            PE_HIP(e, hipMemcpy(static_cast<float*>(e->st_pred.p) + (size_t)m * total, raw_host + (size_t)m * stride, (size_t)total * sizeof(float), hipMemcpyHostToDevice));
    std::vector<SimRec> sim((size_t)n_rec);
    std::vector<uint32_t> word_prefix((size_t)n_rec + 1);
    int64_t words = 0;
    for (int32_t r = 0; r < n_rec; ++r) {
        const int64_t W = window_offsets[r + 1] - window_offsets[r];
        sim[(size_t)r] = SimRec{window_offsets[r], 0, W};
        word_prefix[(size_t)r] = (uint32_t)words;
        words += (W + 63) / 64;
    }
    word_prefix[(size_t)n_rec] = (uint32_t)words;
    if ((rc = sim_launch(e, &q, &dev, sim, word_prefix, static_cast<const float*>(e->st_pred.p), total, nullptr, 0, 0, n_rec))) return rc;
    return sim_end(e, q, n_rec, dev);
}

int pe_test_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_clips,
                  int64_t max_samples, const float* targets_host, const double* thresholds, int32_t n_thresholds, int32_t compare,
                  pe_stats_count* counts_out, pe_stats_summary* summary_out, float* out_host) {
    const StatsRequest q{thresholds, n_thresholds, compare, counts_out, summary_out};
    return run_clips(e, "pe_test_clips", audio_host, sample_format, offsets_host, n_clips, max_samples, false, nullptr, out_host, &q, targets_host);
}

int pe_stats_scores(pe_engine* e, const float* raw_host, int32_t n_rows, int64_t stride, const float* targets_host, int64_t n,
                    const double* thresholds, int32_t n_thresholds, int32_t compare,
                    pe_stats_count* counts_out, pe_stats_summary* summary_out) {
    const char* who = "pe_stats_scores";
    if (!e) return fail(e, PE_ERR_INVALID, "null engine handed to %s", who);
    if (!raw_host || !targets_host) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    if (n_rows < 1 || n_rows > kStatsMaxRows) return fail(e, PE_ERR_INVALID, "%s: n_rows must lie in 1..%d, got %d", who, kStatsMaxRows, n_rows);
    const StatsRequest q{thresholds, n_thresholds, compare, counts_out, summary_out};
    std::string wrong;
    if (stats_request_wrong(wrong, who, q, targets_host, n)) return fail(e, PE_ERR_INVALID, "%s", wrong.c_str());
    if (stride < n) return fail(e, PE_ERR_INVALID, "%s: stride %lld is less than the %lld samples of a row", who, (long long)stride, (long long)n);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const StatsScratch s = stats_scratch(n_rows, n, n_thresholds, true, true);
    int rc;
    if ((rc = ensure(e, e->st_stats, s.total))) return rc;
    char* const scratch = static_cast<char*>(e->st_stats.p);
    float* const probs = reinterpret_cast<float*>(scratch + s.probs);
    PE_HIP(e, hipMemcpy(scratch + s.targets, targets_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    for (int32_t r = 0; r < n_rows; ++r)
        PE_HIP(e, hipMemcpy(probs + (size_t)r * n, raw_host + (size_t)r * stride, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    PE_HIP(e, stats_run(scratch, s, probs, n, reinterpret_cast<const float*>(scratch + s.targets), n, n_rows, q));
    return PE_OK;
}

int pe_set_clip_pass_bytes(pe_engine* e, int64_t bytes) {
    if (!e) return PE_ERR_INVALID;
    if (bytes < 1) return fail(e, PE_ERR_INVALID, "the pass target must be at least 1 byte, got %lld", (long long)bytes);
    e->clip_pass_bytes = bytes;
    return PE_OK;
}

namespace {
int set_decoder(pe_engine* e, int m, const double* cd, int32_t cd_len, int32_t min_out, int32_t out_range, double center) {
    DecState& d = e->dec[m];
    dev_free(e, d.cd, (size_t)(d.cd_len ? d.cd_len : 1) * sizeof(double));
    d.cd = nullptr; d.cd_len = 0;
    std::vector<double> host(cd, cd + cd_len);
    int rc = dev_upload(e, &d.cd, host);
    if (rc) return rc;
    d.cd_len = cd_len; d.min_out = min_out; d.out_range = out_range; d.center = center;
    return PE_OK;
}
int set_trigger(pe_engine* e, int m, int32_t chunk_size_bytes, double sensitivity, int32_t trigger_level) {
    if (!e->activation) {
        int rc = dev_alloc(e, &e->activation, (size_t)e->n_models * e->n_padded);     // [n_models][n_padded]
        if (rc) return rc;
    }
    PE_HIP(e, hipMemset(e->activation + (size_t)m * e->n_padded, 0, (size_t)e->n_padded * sizeof(int32_t)));
    const int n = 8 * 2048;                                // -(8 * 2048) // chunk_size, floor division
    DecState& d = e->dec[m];
    d.threshold = 1.0 - sensitivity; d.level = trigger_level; d.rearm = -((n + chunk_size_bytes - 1) / chunk_size_bytes); d.on = true;
    return PE_OK;
}
}  // namespace

int pe_set_decoder(pe_engine* e, const double* cd, int32_t cd_len, int32_t min_out, int32_t out_range, double center) {
    if (!e || cd_len < 0 || (cd_len > 0 && !cd)) return fail(e, PE_ERR_INVALID, "bad decoder table");
    if (out_range != 0 && cd_len < 1) return fail(e, PE_ERR_INVALID, "decoder needs a non-empty table when out_range != 0");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    PE_HIP(e, hipDeviceSynchronize());                    // no decode launch may still read the old table
    for (int m = 0; m < e->n_models; ++m) {               // (every model of the engine)
        const int rc = set_decoder(e, m, cd, cd_len, min_out, out_range, center);
        if (rc) return rc;
    }
    return PE_OK;
}

int pe_set_decoder_model(pe_engine* e, int32_t model, const double* cd, int32_t cd_len, int32_t min_out, int32_t out_range, double center) {
    if (!e || cd_len < 0 || (cd_len > 0 && !cd)) return fail(e, PE_ERR_INVALID, "bad decoder table");
    if (model < 0 || model >= e->n_models) return fail(e, PE_ERR_INVALID, "model %d outside 0..%d", model, e->n_models - 1);
    if (out_range != 0 && cd_len < 1) return fail(e, PE_ERR_INVALID, "decoder needs a non-empty table when out_range != 0");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    PE_HIP(e, hipDeviceSynchronize());
    return set_decoder(e, model, cd, cd_len, min_out, out_range, center);
}

int pe_set_trigger(pe_engine* e, int32_t chunk_size_bytes, double sensitivity, int32_t trigger_level) {
    if (!e || chunk_size_bytes <= 0) return fail(e, PE_ERR_INVALID, "bad trigger parameters");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    for (int m = 0; m < e->n_models; ++m) {               // (every model of the engine)
        const int rc = set_trigger(e, m, chunk_size_bytes, sensitivity, trigger_level);
        if (rc) return rc;
    }
    return PE_OK;
}

int pe_set_trigger_model(pe_engine* e, int32_t model, int32_t chunk_size_bytes, double sensitivity, int32_t trigger_level) {
    if (!e || chunk_size_bytes <= 0) return fail(e, PE_ERR_INVALID, "bad trigger parameters");
    if (model < 0 || model >= e->n_models) return fail(e, PE_ERR_INVALID, "model %d outside 0..%d", model, e->n_models - 1);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    return set_trigger(e, model, chunk_size_bytes, sensitivity, trigger_level);
}

// raw_dev / conf_out_dev / fired_out_dev: [n_models][n_streams]; ONE decode launch (a K-model engine: per-model tables)
int pe_decode_device(pe_engine* e, const float* raw_dev, double* conf_out_dev, unsigned char* fired_out_dev, void* stream) {
    if (!e || !raw_dev) return fail(e, PE_ERR_INVALID, "null argument to pe_decode_device");
    int rc = check_decoder(e);
    if (rc) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);                                          // (updates in flight may carry decodes: they move the trigger state)
    note_user_stream(e, stream);
    return launch_decode_rows(e, nullptr, e->n_streams, raw_dev, conf_out_dev, fired_out_dev, static_cast<hipStream_t>(stream));
}

int pe_decode(pe_engine* e, const float* raw_host, double* conf_out_host, unsigned char* fired_out_host) {
    if (!e || !raw_host) return fail(e, PE_ERR_INVALID, "null argument to pe_decode");
    PE_HIP(e, hipSetDevice(e->device));
    int rc;
    const size_t n = (size_t)e->n_models * e->n_streams;
    if ((rc = ensure(e, e->st_out, n * sizeof(float)))) return rc;
    if ((rc = ensure(e, e->st_conf, n * sizeof(double)))) return rc;
    if ((rc = ensure(e, e->st_fired, n))) return rc;
    PE_HIP(e, hipMemcpy(e->st_out.p, raw_host, n * sizeof(float), hipMemcpyHostToDevice));
    PE_HIP(e, hipMemset(e->st_fired.p, 0, n));
    if ((rc = pe_decode_device(e, static_cast<const float*>(e->st_out.p), static_cast<double*>(e->st_conf.p),
                               static_cast<unsigned char*>(e->st_fired.p), nullptr))) return rc;
    if (conf_out_host) PE_HIP(e, hipMemcpy(conf_out_host, e->st_conf.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (fired_out_host) PE_HIP(e, hipMemcpy(fired_out_host, e->st_fired.p, n, hipMemcpyDeviceToHost));
    if (!conf_out_host && !fired_out_host) PE_HIP(e, hipStreamSynchronize(nullptr));
    return PE_OK;
}

// The same for streams that advance on their own: rows [n_models][n_active] in the order of the ids; only the named streams'
// trigger state moves (a stream that got no audio neither decays nor fires).  The ids must be distinct and in range (the
// host entry point checks, the device one cannot).
int pe_decode_subset_device(pe_engine* e, const int32_t* stream_ids_dev, int32_t n_active, const float* raw_dev,
                            double* conf_out_dev, unsigned char* fired_out_dev, void* stream) {
    if (!e) return fail(e, PE_ERR_INVALID, "null argument to pe_decode_subset_device");
    if (n_active < 0 || n_active > e->n_streams) return fail(e, PE_ERR_INVALID, "n_active=%d outside 0..%d", n_active, e->n_streams);
    if (n_active == 0) return PE_OK;
    if (!stream_ids_dev || !raw_dev) return fail(e, PE_ERR_INVALID, "null argument to pe_decode_subset_device");
    int rc = check_decoder(e);
    if (rc) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    note_user_stream(e, stream);
    return launch_decode_rows(e, stream_ids_dev, n_active, raw_dev, conf_out_dev, fired_out_dev, static_cast<hipStream_t>(stream));
}

int pe_decode_subset(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const float* raw_host,
                     double* conf_out_host, unsigned char* fired_out_host) {
    if (!e) return fail(e, PE_ERR_INVALID, "null argument to pe_decode_subset");
    if (n_active < 0 || n_active > e->n_streams) return fail(e, PE_ERR_INVALID, "n_active=%d outside 0..%d", n_active, e->n_streams);
    if (n_active == 0) return PE_OK;
    if (!stream_ids_host || !raw_host) return fail(e, PE_ERR_INVALID, "null argument to pe_decode_subset");
    int rc;
    if ((rc = check_ids(e, stream_ids_host, n_active))) return rc;
    PE_HIP(e, hipSetDevice(e->device));
    const size_t n = (size_t)e->n_models * n_active, id_bytes = (size_t)n_active * sizeof(int32_t);
    if ((rc = ensure(e, e->st_out, n * sizeof(float)))) return rc;
    if ((rc = ensure(e, e->st_conf, n * sizeof(double)))) return rc;
    if ((rc = ensure(e, e->st_fired, n))) return rc;
    if ((rc = ensure(e, e->st_ids, id_bytes))) return rc;
    PE_HIP(e, hipMemcpy(e->st_ids.p, stream_ids_host, id_bytes, hipMemcpyHostToDevice));
    PE_HIP(e, hipMemcpy(e->st_out.p, raw_host, n * sizeof(float), hipMemcpyHostToDevice));
    PE_HIP(e, hipMemset(e->st_fired.p, 0, n));
    if ((rc = pe_decode_subset_device(e, static_cast<const int32_t*>(e->st_ids.p), n_active, static_cast<const float*>(e->st_out.p),
                                      static_cast<double*>(e->st_conf.p), static_cast<unsigned char*>(e->st_fired.p), nullptr))) return rc;
    if (conf_out_host) PE_HIP(e, hipMemcpy(conf_out_host, e->st_conf.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (fired_out_host) PE_HIP(e, hipMemcpy(fired_out_host, e->st_fired.p, n, hipMemcpyDeviceToHost));
    if (!conf_out_host && !fired_out_host) PE_HIP(e, hipStreamSynchronize(nullptr));
    return PE_OK;
}

int pe_reserve_updates(pe_engine* e, int32_t max_updates, int32_t max_chunk_samples) {
    if (!e || max_updates < 1 || max_chunk_samples < 1) return fail(e, PE_ERR_INVALID, "bad arguments to pe_reserve_updates");
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    PE_HIP(e, hipDeviceSynchronize());
    const int pending = pending_frames(e->prm);
    const long long frames = ((long long)max_updates * max_chunk_samples + e->prm.hop_samples - 1) / e->prm.hop_samples + 1;
    const int slots = next_pow2((int)(e->prm.n_features + pending + frames));
    if (slots != e->ring_slots) {
        dev_free(e, e->ring, ring_floats(e) * sizeof(float));
        e->ring = nullptr;
        dev_free(e, e->proj_ring, (size_t)e->n_tiles * e->ring_slots * kTileStreams * kProjRow * sizeof(float));
        e->proj_ring = nullptr;
        e->ring_slots = slots;
        int rc = dev_alloc(e, &e->ring, ring_floats(e));
        if (rc) return rc;
        if (e->proj_on && (rc = dev_alloc(e, &e->proj_ring, (size_t)e->n_tiles * e->ring_slots * kTileStreams * kProjRow))) return rc;
    }
    if (!e->ke_hist || max_updates > e->max_updates) {
        if (e->ke_hist) {
            dev_free(e, e->ke_hist, (size_t)e->max_updates * e->n_padded * sizeof(uint32_t));
            e->ke_hist = nullptr;
        }
        int rc = dev_alloc(e, &e->ke_hist, (size_t)max_updates * e->n_padded);
        if (rc) return rc;
    }
    e->max_updates = max_updates;
    ++e->chain_epoch;
    return pe_clear(e, nullptr);          // the ring was re-laid out: streams restart
}

int pe_update_many_device(pe_engine* e, const int16_t* pcm_dev, int32_t chunk, int32_t n_updates, float* raw_out_dev, void* stream) {
    int rc = check_chunk(e, pcm_dev, chunk);
    if (rc) return rc;
    if (!raw_out_dev || n_updates < 1) return fail(e, PE_ERR_INVALID, "bad arguments to pe_update_many_device");
    if (n_updates > e->max_updates || !e->ke_hist) return fail(e, PE_ERR_INVALID, "call pe_reserve_updates(e, >= %d, >= %d) first", n_updates, chunk);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const int pending = pending_frames(e->prm);
    const long long frames = ((long long)n_updates * chunk + e->prm.hop_samples - 1) / e->prm.hop_samples + 1;
    if ((long long)n_updates * chunk >= (1ll << 30)) return fail(e, PE_ERR_INVALID, "n_updates * chunk_samples must stay below 2^30");
    if (e->prm.n_features + pending + frames > e->ring_slots) return fail(e, PE_ERR_INVALID, "reserved ring too small for %d updates of %d samples", n_updates, chunk);
    hipStream_t s = static_cast<hipStream_t>(stream);
    note_user_stream(e, stream);
    if ((rc = flush_kept(e, s))) return rc;
    uint32_t call = 0;
    if ((rc = begin_state_call(e, s, &call))) return rc;
    if (!e->general) {
        // the stock wave kernels: one task row per frame a stream can complete in this call, at most kMaxFrameRows rows
        const int rows = max_frames_per_call(e, (long long)n_updates * chunk);
        if (rows > kMaxFrameRows) return fail(e, PE_ERR_INVALID, "a call may complete at most %d frames per stream (%d updates of %d samples: %d)", kMaxFrameRows, n_updates, chunk, rows);
    }
    // every frame the call completes in ONE front-end launch (either family), then the batched network launch
    if ((rc = launch_stream_front_end(e, pcm_dev, chunk, s, call, nullptr, 0, n_updates, e->ke_hist))) return rc;
    GruArgs g = gru_args(e);
    g.ke_plain = e->ke_hist;
    g.out = raw_out_dev;
    if (e->wide || e->row_floats != kRowFloats) {
        // the streamed-weight network, and every network over 32-float rows (general front end only): one launch per update of the
        // call (each fills the machine on its own), the window of update u found through its row of the emitted-frame history
        for (int u = 0; u < n_updates; ++u) {
            GruArgs gu = g;
            gu.ke_plain = e->ke_hist + (size_t)u * e->n_padded;
            gu.out = raw_out_dev + (size_t)u * e->n_streams;
            int nrc = launch_networks(e, gu, 1, s, (long long)n_updates * e->n_streams);
            if (nrc) return nrc;
        }
        return PE_OK;
    }
    g.waves_per_tile = 1;                                 // (the launcher picks one or four waves per window itself)
    return launch_networks_many(e, g, n_updates, s);
}

int pe_update_many(pe_engine* e, const int16_t* pcm_host, int32_t chunk, int32_t n_updates, float* raw_out_host) {
    int rc = check_chunk(e, pcm_host, chunk);
    if (rc) return rc;
    if (!raw_out_host || n_updates < 1) return fail(e, PE_ERR_INVALID, "bad arguments to pe_update_many");
    PE_HIP(e, hipSetDevice(e->device));
    const size_t pcm_bytes = (size_t)n_updates * e->n_streams * chunk * sizeof(int16_t);
    const size_t out_bytes = (size_t)e->n_models * n_updates * e->n_streams * sizeof(float);
    if ((rc = ensure(e, e->st_pcm, pcm_bytes))) return rc;
    if ((rc = ensure(e, e->st_out, out_bytes))) return rc;
    PE_HIP(e, hipMemcpy(e->st_pcm.p, pcm_host, pcm_bytes, hipMemcpyHostToDevice));
    if ((rc = pe_update_many_device(e, static_cast<const int16_t*>(e->st_pcm.p), chunk, n_updates, static_cast<float*>(e->st_out.p), nullptr))) return rc;
    PE_HIP(e, hipMemcpy(raw_out_host, e->st_out.p, out_bytes, hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_get_info(const pe_engine* e, pe_info* out) {
    if (!e || !out) return PE_ERR_INVALID;
    out->n_streams = e->n_streams;
    out->n_features = e->prm.n_features;
    out->n_mfcc = e->prm.n_mfcc;
    out->units = e->units;
    out->n_layers = e->n_layers;
    out->ring_slots = e->ring_slots;
    out->carry_capacity = e->carry_cap;
    out->mfcc_precision = e->prm.mfcc_precision;
    out->gru_precision = e->prm.gru_precision;
    out->device_bytes = e->device_bytes;
    return PE_OK;
}

int pe_get_stream_state(pe_engine* e, int32_t* q_out, uint32_t* computed_out, uint32_t* emitted_out) {
    if (!e) return PE_ERR_INVALID;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    PE_HIP(e, hipDeviceSynchronize());
    // both sides of every record; the current one is picked here exactly as the kernels pick it (pe_common.h: rec_side)
    std::vector<StreamRec> host((size_t)2 * e->n_padded);
    PE_HIP(e, hipMemcpy(host.data(), e->rec, host.size() * sizeof(StreamRec), hipMemcpyDeviceToHost));
    const uint32_t call = e->call_no + 1u;
    for (int s = 0; s < e->n_streams; ++s) {
        const StreamRec& r0 = host[rec_at((uint32_t)e->n_padded, s, 0)];
        const StreamRec& r1 = host[rec_at((uint32_t)e->n_padded, s, 1)];
        const StreamRec& c = (call - r1.wcall) - 1u < (call - r0.wcall) - 1u ? r1 : r0;
        if (q_out) q_out[s] = c.q;
        if (computed_out) computed_out[s] = c.kc;
        if (emitted_out) emitted_out[s] = c.ke;
    }
    return PE_OK;
}

int pe_set_renumber_at(pe_engine* e, uint32_t call_number) {
    if (!e) return PE_ERR_INVALID;
    if (call_number < 8u || call_number > 0x7fff0000u) return fail(e, PE_ERR_INVALID, "renumbering threshold must be in 8..0x7fff0000");
    e->renumber_at = call_number;
    return PE_OK;
}

int pe_set_fused(pe_engine* e, int32_t enabled) {
    if (!e) return PE_ERR_INVALID;
    PE_DRAIN(e);
    ++e->chain_epoch;
    e->fused = enabled != 0;
    return PE_OK;
}

int pe_set_input_projection(pe_engine* e, int32_t enabled) {
    if (!e) return PE_ERR_INVALID;
    if (enabled != 0 && enabled != 1) return fail(e, PE_ERR_INVALID, "input projection must be 0 or 1");
    if (enabled && !e->proj_ok) return fail(e, PE_ERR_UNSUPPORTED, "input-projection rows exist for the float32 network of 17..20 units without delta features only");
    if (enabled && e->n_models > 1) return fail(e, PE_ERR_UNSUPPORTED, "input-projection rows are per model: an engine of %d models has none", e->n_models);
    if ((enabled != 0) == e->proj_on) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    PE_HIP(e, hipDeviceSynchronize());
    e->proj_on = enabled != 0;
    ++e->chain_epoch;
    if (e->proj_on && !e->proj_ring) {
        int rc = dev_alloc(e, &e->proj_ring, (size_t)e->n_tiles * e->ring_slots * kTileStreams * kProjRow);
        if (rc) { e->proj_on = false; return rc; }
    }
    return pe_clear(e, nullptr);          // rows written so far lack (or no longer need) their projections: streams restart
}

int pe_set_gru_waves(pe_engine* e, int32_t waves) {
    if (!e) return PE_ERR_INVALID;
    if (waves != 0 && waves != 1 && waves != 4) return fail(e, PE_ERR_INVALID, "gru kernel shape must be 0 (auto), 1 or 4 (waves per tile)");
    PE_DRAIN(e);
    ++e->chain_epoch;
    e->gru_waves = waves;
    return PE_OK;
}

int pe_set_gru_tiling(pe_engine* e, int32_t tiling) {
    if (!e) return PE_ERR_INVALID;
    if (tiling < -1 || tiling > 2) return fail(e, PE_ERR_INVALID, "gru tiling must be -1 (auto), 0 (classic), 1 (re-tiled) or 2 (XDL form)");
    if (e->wide && e->prm.gru_precision == 1) {
        if (tiling != 0) return fail(e, PE_ERR_UNSUPPORTED, "the bf16-operand wide network (gru_precision = 1) has one form, 0; forms 0 (f32-input MFMAs) and 2 (float32 products on the bf16 pipe) belong to the float32 wide network");
        return PE_OK;
    }
    if (e->wide) {
        if (tiling == 1) return fail(e, PE_ERR_UNSUPPORTED, "wide networks have two forms: 0 (f32-input MFMAs) and 2 (float32 products on the bf16 pipe)");
        PE_DRAIN(e);
        e->gru_tiling = tiling;
        return PE_OK;
    }
    if (tiling == 2 && !e->nets[0].x3_blob)
        return fail(e, PE_ERR_UNSUPPORTED, "the XDL form of the float32 network (tiling 2) takes <= 20 units, <= 15 inputs, float32 operands, no use_delta");
    if (tiling == 1 && e->prm.gru_precision == 1 && !e->nets[0].b20_blob)
        return fail(e, PE_ERR_UNSUPPORTED, "the five-values layout of the bf16 network (tiling 1) takes <= 20 units and <= 14 features");
    PE_DRAIN(e);
    ++e->chain_epoch;
    e->gru_tiling = tiling;
    return PE_OK;
}

int pe_get_gru_tiling(const pe_engine* e) {
    if (!e) return -2;               // (not PE_ERR_INVALID = 1, which is a valid answer)
    if (e->wide) return e->prm.gru_precision == 0 && wide_uses_x3(e) ? 2 : 0;
    if (e->prm.gru_precision != 0) return gru_args(e).b20 ? 1 : 0;
    const GruArgs a = gru_args(e);
    return a.x3 ? 2 : a.cw ? 1 : 0;
}

int pe_set_timing(pe_engine* e, int32_t enabled) {
    if (!e) return PE_ERR_INVALID;
    e->timing = enabled != 0;
    e->ev_valid = false;
    ++e->chain_epoch;
    return PE_OK;
}

int pe_set_chain_carry(pe_engine* e, int32_t mode) {
    if (!e) return PE_ERR_INVALID;
    if (mode < 0 || mode > 2) return fail(e, PE_ERR_INVALID, "chain carry must be 0 (off), 1 (automatic) or 2 (eager)");
    PE_DRAIN(e);
    ++e->chain_epoch;
    e->chain_streak = 0;
    e->chain_mode = mode;
    return PE_OK;
}

int pe_get_chain_carry(const pe_engine* e, int32_t* mode, int32_t* active) {
    if (!e) return PE_ERR_INVALID;
    if (mode) *mode = e->chain_mode;
    if (active) *active = (e->chain_mode != 0 && e->chains && e->chains_built_epoch == e->chain_epoch) ? 1 : 0;
    return PE_OK;
}

int pe_get_chain_skip(const pe_engine* e, int32_t* chunk) {
    if (!e) return PE_ERR_INVALID;
    if (chunk) *chunk = (e->chain_mode != 0 && e->chains && e->chains_built_epoch == e->chain_epoch) ? e->chain_skip_chunk : 0;
    return PE_OK;
}

uint32_t pe_chain_alive_mask(int32_t q, uint32_t kc, uint32_t ke, int32_t chunk, int32_t hop, int32_t frame_len, int32_t window, int32_t T) {
    // (a record's q is what mfcc_book_tile leaves: avail - nnew * hop, in [frame_len - hop, frame_len) -- negative where a frame is
    //  shorter than a hop and the next one starts beyond the last sample held; anything below that is no record)
    if ((q < 0 && q < frame_len - hop) || chunk < 1 || hop < 1 || frame_len < 1 || window < 1 || T < 1 || T > 31) return 0u;
    const KeStep st = ke_step(q, kc, ke, chunk, hop, frame_len, window);
    return chain_alive_bits(st.rem, chunk, hop, window, T, 0, T - 1) | (1u << T);
}

int pe_get_last_timing(pe_engine* e, float* mfcc_ms, float* gru_ms) {
    if (!e) return PE_ERR_INVALID;
    if (!e->ev_valid) return fail(e, PE_ERR_INVALID, "no timed update recorded (call pe_set_timing(e, 1) first)");
    PE_HIP(e, hipEventSynchronize(e->ev[2]));
    float a = 0.f, b = 0.f;
    PE_HIP(e, hipEventElapsedTime(&a, e->ev[0], e->ev[1]));
    PE_HIP(e, hipEventElapsedTime(&b, e->ev[1], e->ev[2]));
    if (mfcc_ms) *mfcc_ms = a;      // fused launch: the whole update; else the MFCC kernel
    if (gru_ms) *gru_ms = e->ev_has_gru ? b : 0.f;
    return PE_OK;
}

}  // extern "C"

// ---- training (kernels: gru_train_device.h) ----------------------------------------------------------------
static_assert(PE_TRAIN_MAX_MODELS == kTrainMaxModels, "the header's cap is the kernel table's length");

struct TrainSet {                           // a resident set: pe_trainer_set_data / pe_trainer_set_validation
    const float* feats = nullptr;
    const float* targets = nullptr;
    int n = 0;
};

enum TrainBuf {                             // the slots of pe_trainer::buf
    kBufFeats, kBufTargets, kBufMasks, kBufIndices,     // what one call uploads
    kBufTape, kBufPartial,                              // the narrow path's tape and per-block partials
    kBufProbs,                                          // [K][n], every path
    kBufDataFeats, kBufDataTargets,                     // the resident dataset: the targets of a set follow its features
    kBufValFeats, kBufValTargets,                       // the resident validation set
    kBufStats,                                          // the scratch of pe_trainer_stats_models (StatsScratch)
    kBufSampleState, kBufSampleList, kBufSampleScratch, // selection state bytes, selection list, the scratch of pe_trainer_sample_choose
    kBufLayerTape, kBufFin, kBufLayerUt, kBufLayerPartial, kBufLayerGpart,  // wide: records, dL/dh_T, U^T, per-tile and per-chunk partials
    kBufTape1, kBufDx, kBufHfin0, kBufUt1W1t, kBufMtape, kBufGpart1,        // stacked: layer 1's records, dx, layer 0's final state /
    kBufCount                                                               // sequence, U1^T | W1^T, layer 1's masks per tile, its chunk partials
};
constexpr TrainBuf train_targets_of(TrainBuf feats) { return static_cast<TrainBuf>(feats + 1); }

struct pe_trainer {
    int device = 0;
    int T = 0, F = 0, K = 0, n_params = 0;  // n_params: the total over the networks
    int H[kTrainMaxModels] = {}, ofs[kTrainMaxModels + 1] = {};        // units; offset of a network's flat vector
    int H2[kTrainMaxModels] = {};   // pe_trainer_create_stacked: units of the second GRU layer, 0 for a one-layer network
    std::string err;
    float* theta = nullptr;         // concatenated flat parameters
    float* accum = nullptr;         // RMSprop accumulators
    float* grads = nullptr;
    float* loss = nullptr;          // [K] losses, then [K] int32 accuracy counts: one copy brings both back
    TrainSet data, validation;
    // the selection state of the training set (pe_trainer_sample_*): rows [0, sample_n) have their state byte; rows behind
    // them (a fresh or grown set) are eligible and unselected, and get theirs when a sample call next needs it
    int sample_n = 0, n_selected = 0;
    // buffers that grow with the largest call (TrainBuf).  The wide and the stacked path share kBufLayer*: there a stacked
    // network keeps layer 0's records, U0^T and chunk partials, kBufFin is the dL/dh_T of its layer 1, and kBufLayerPartial
    // the per-tile partials of its head.
    DeviceBuf buf[kBufCount];
};

namespace {

int tfail(pe_trainer* t, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (t) t->err = buf; else g_global_error = buf;
    return code;
}

#define PE_THIP(t, call)                                                                                   \
    do {                                                                                                   \
        hipError_t _err = (call);                                                                          \
        if (_err != hipSuccess)                                                                            \
            return tfail((t), PE_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_err), __FILE__, __LINE__); \
    } while (0)

int train_reserve(pe_trainer* t, TrainBuf which, size_t bytes) {
    DeviceBuf& b = t->buf[which];
    if (b.bytes >= bytes && b.p) return PE_OK;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    hipError_t err = hipMalloc(&b.p, bytes ? bytes : 1);
    if (err != hipSuccess) { b.p = nullptr; return tfail(t, PE_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err)); }
    b.bytes = bytes;
    return PE_OK;
}

float train_keep_scale(float rate) { return 1.0f / (1.0f - rate); }

int train_check_targets(pe_trainer* t, const float* y, int n) {
    for (int i = 0; i < n; ++i)
        if (!(y[i] >= 0.0f && y[i] <= 1.0f)) return tfail(t, PE_ERR_INVALID, "targets[%d] = %g is outside [0, 1]", i, (double)y[i]);
    return PE_OK;
}

// "model 2: " in front of a per-network complaint of a trainer of several
std::string train_model_prefix(int n_models, int m) { return n_models > 1 ? "model " + std::to_string(m) + ": " : std::string(); }

// Forward (+ backward) of the networks [m0, m1) (each of at most kTrainMaxUnits units) over n samples in one launch, and the
// reduction.  a0.model[m] holds what the caller set for network m of the trainer.
int train_run_narrow(pe_trainer* t, const TrainArgs& a0, bool backward, int m0, int m1) {
    TrainArgs a = a0;
    const int blocks = (a.n + kTrainTile - 1) / kTrainTile;
    int widest = 0;
    for (int m = m0; m < m1; ++m) widest = std::max(widest, t->H[m]);
    a.T = t->T; a.F = t->F; a.n_models = m1 - m0;
    a.backward = backward ? 1 : 0;
    a.n_blocks = blocks;
    a.threads = train_threads(widest);
    a.n_total = t->ofs[m1] - t->ofs[m0];
    a.inv_n = 1.0f / (float)a.n;
    a.theta = t->theta + t->ofs[m0];
    a.accum = t->accum + t->ofs[m0];
    a.grads = backward ? t->grads + t->ofs[m0] : nullptr;
    a.loss = t->loss + m0;
    size_t tape = 0, partial = 0;
    for (int m = m0; m < m1; ++m) {
        TrainModel& r = a.model[m - m0];
        r = a0.model[m];
        r.H = t->H[m];
        r.ofs = t->ofs[m] - t->ofs[m0];
        r.tape_ofs = tape;
        r.partial_ofs = partial;
        if (backward) tape += (size_t)blocks * t->T * 4 * a.threads;
        partial += (size_t)blocks * ((backward ? t->ofs[m + 1] - t->ofs[m] : 0) + 2);
    }
    int rc = train_reserve(t, kBufPartial, partial * sizeof(float));
    if (rc) return rc;
    if (backward && (rc = train_reserve(t, kBufTape, tape * sizeof(float)))) return rc;
    a.tape = static_cast<float*>(t->buf[kBufTape].p);
    a.partial = static_cast<float*>(t->buf[kBufPartial].p);
    a.probs = static_cast<float*>(t->buf[kBufProbs].p) + (size_t)m0 * a.n;
    PE_THIP(t, launch_train(a, nullptr));
    PE_THIP(t, launch_train_reduce(a, nullptr));
    return PE_OK;
}

// What TrainWideArgs and TrainStackedArgs have in common, for network m of the trainer: the caller's per-call and per-network
// settings (train_run), and where the network's parameters live.  `a0.n` is 0 where nothing runs over samples (pe_trainer_apply).
template <class Args>
void train_fill_common(const pe_trainer* t, const TrainArgs& a0, bool backward, int m, Args* w) {
    const TrainModel& r = a0.model[m];
    w->n = a0.n; w->T = t->T; w->F = t->F;
    w->n_tiles = (a0.n + 15) / 16;
    w->backward = backward ? 1 : 0;
    w->apply = a0.apply;
    w->frozen_mask = r.frozen_mask;
    w->mask_mode = r.mask_mode;
    w->rate = r.rate; w->keep_scale = r.keep_scale; w->beta = r.beta;
    w->inv_n = a0.n > 0 ? 1.0f / (float)a0.n : 0.0f;
    w->lr = r.lr; w->rho = r.rho; w->eps = r.eps;
    w->mask_key = r.mask_key;
    w->theta = t->theta + t->ofs[m];
    w->accum = t->accum + t->ofs[m];
    w->grads = t->grads + t->ofs[m];
    w->loss = t->loss + m;
    w->feats = a0.feats; w->targets = a0.targets; w->indices = a0.indices;
    w->probs = static_cast<float*>(t->buf[kBufProbs].p) + (size_t)m * a0.n;
}

void train_stacked_units(const pe_trainer* t, int m, TrainStackedArgs* w) {
    w->H1 = t->H[m]; w->H1p = tw_pad(w->H1);
    w->H2 = t->H2[m]; w->H2p = tw_pad(w->H2);
}

// The same for ONE network of more than kTrainMaxUnits units (gru_train_wide_device.h)
int train_run_wide(pe_trainer* t, const TrainArgs& a0, bool backward, int m) {
    TrainWideArgs w{};
    train_fill_common(t, a0, backward, m, &w);
    w.H = t->H[m]; w.Hp = tw_pad(w.H);
    w.masks = a0.masks;
    int rc = train_reserve(t, kBufLayerPartial, (size_t)w.n_tiles * (w.H + 3) * sizeof(float));
    if (rc) return rc;
    if (backward) {
        const long long records = (long long)w.n_tiles * w.T;
        if ((rc = train_reserve(t, kBufLayerTape, (size_t)records * tw_record(w.F, w.Hp) * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufFin, (size_t)w.n_tiles * w.Hp * 16 * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufLayerUt, (size_t)3 * w.Hp * w.Hp * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufLayerGpart, (size_t)tw_chunks(records) * train_n_gru(w.F, w.H) * sizeof(float)))) return rc;
    }
    w.tape = static_cast<float*>(t->buf[kBufLayerTape].p);
    w.fin = static_cast<float*>(t->buf[kBufFin].p);
    w.ut = static_cast<float*>(t->buf[kBufLayerUt].p);
    w.partial = static_cast<float*>(t->buf[kBufLayerPartial].p);
    w.gpart = static_cast<float*>(t->buf[kBufLayerGpart].p);
    PE_THIP(t, launch_train_wide(w, nullptr));
    return PE_OK;
}

// The same for ONE network of two GRU layers (gru_train_stacked_device.h)
int train_run_stacked(pe_trainer* t, const TrainArgs& a0, bool backward, int m) {
    TrainStackedArgs w{};
    train_fill_common(t, a0, backward, m, &w);
    train_stacked_units(t, m, &w);
    w.mask_key1 = train_mask_key_layer1(w.mask_key);
    w.masks0 = a0.masks;
    w.masks1 = a0.masks ? a0.masks + (size_t)3 * a0.n * t->F : nullptr;
    const size_t records = (size_t)w.n_tiles * w.T, row1 = (size_t)w.H1p * 16 * sizeof(float);
    int rc = train_reserve(t, kBufLayerPartial, (size_t)w.n_tiles * (w.H2 + 3) * sizeof(float));
    if (rc) return rc;
    if ((rc = train_reserve(t, kBufHfin0, (backward ? (size_t)w.n_tiles : records) * row1))) return rc;
    if (backward) {
        const size_t chunks = (size_t)tw_chunks((long long)records);
        if ((rc = train_reserve(t, kBufLayerTape, records * tw_record(w.F, w.H1p) * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufFin, (size_t)w.n_tiles * w.H2p * 16 * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufLayerUt, (size_t)3 * w.H1p * w.H1p * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufLayerGpart, chunks * train_n_gru(w.F, w.H1) * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufTape1, records * tw_record(0, w.H2p) * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufDx, records * row1))) return rc;
        if ((rc = train_reserve(t, kBufUt1W1t, (size_t)3 * w.H2p * (w.H2p + w.H1p) * sizeof(float)))) return rc;
        if ((rc = train_reserve(t, kBufMtape, (size_t)w.n_tiles * 3 * row1))) return rc;
        if ((rc = train_reserve(t, kBufGpart1, chunks * train_n_gru(w.H1, w.H2) * sizeof(float)))) return rc;
    }
    w.tape0 = static_cast<float*>(t->buf[kBufLayerTape].p);
    w.fin = static_cast<float*>(t->buf[kBufFin].p);
    w.ut0 = static_cast<float*>(t->buf[kBufLayerUt].p);
    w.partial = static_cast<float*>(t->buf[kBufLayerPartial].p);
    w.gpart0 = static_cast<float*>(t->buf[kBufLayerGpart].p);
    w.tape1 = static_cast<float*>(t->buf[kBufTape1].p);
    w.dx = static_cast<float*>(t->buf[kBufDx].p);
    w.hfin0 = static_cast<float*>(t->buf[kBufHfin0].p);
    w.ut1 = static_cast<float*>(t->buf[kBufUt1W1t].p);
    w.w1t = w.ut1 ? w.ut1 + (size_t)3 * w.H2p * w.H2p : nullptr;
    w.mtape = static_cast<float*>(t->buf[kBufMtape].p);
    w.gpart1 = static_cast<float*>(t->buf[kBufGpart1].p);
    PE_THIP(t, launch_train_stacked(w, nullptr));
    return PE_OK;
}

// Forward (+ backward) of every network over n samples, and the reduction.  The caller has filled a.n / feats / targets /
// indices / masks / apply and, per network, mask_* / beta / lr / rho / eps / frozen_mask; the rest is set here.  Runs of
// neighbouring networks of at most kTrainMaxUnits units share a launch, as they do in a pe_trainer_create_models trainer (a
// network's bits do not depend on its company); every wider network has its own launches.
int train_run(pe_trainer* t, TrainArgs& a, bool backward) {
    int rc = train_reserve(t, kBufProbs, (size_t)t->K * a.n * sizeof(float));
    if (rc) return rc;
    a.probs = static_cast<float*>(t->buf[kBufProbs].p);
    for (int m = 0; m < t->K;) {
        if (t->H2[m] > 0) {
            if ((rc = train_run_stacked(t, a, backward, m))) return rc;
            ++m;
            continue;
        }
        if (t->H[m] > kTrainMaxUnits) {
            if ((rc = train_run_wide(t, a, backward, m))) return rc;
            ++m;
            continue;
        }
        int m1 = m + 1;
        while (m1 < t->K && t->H[m1] <= kTrainMaxUnits && t->H2[m1] == 0) ++m1;
        if ((rc = train_run_narrow(t, a, backward, m, m1))) return rc;
        m = m1;
    }
    return PE_OK;
}

int train_upload_batch(pe_trainer* t, const float* feats_host, const float* targets_host, int n, TrainArgs* a) {
    const size_t fb = (size_t)n * t->T * t->F * sizeof(float);
    int rc = train_reserve(t, kBufFeats, fb);
    if (rc) return rc;
    PE_THIP(t, hipMemcpy(t->buf[kBufFeats].p, feats_host, fb, hipMemcpyHostToDevice));
    a->feats = static_cast<const float*>(t->buf[kBufFeats].p);
    a->targets = nullptr;
    if (targets_host) {
        if ((rc = train_reserve(t, kBufTargets, (size_t)n * sizeof(float)))) return rc;
        PE_THIP(t, hipMemcpy(t->buf[kBufTargets].p, targets_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        a->targets = static_cast<const float*>(t->buf[kBufTargets].p);
    }
    a->n = n;
    return PE_OK;
}

int train_upload_set(pe_trainer* t, const char* who, TrainSet* set, TrainBuf slot, const float* feats_host, const float* targets_host, int n) {
    if (!feats_host || !targets_host) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
    if (n <= 0) return tfail(t, PE_ERR_INVALID, "%s: n = %d", who, n);
    int rc = train_check_targets(t, targets_host, n);
    if (rc) return rc;
    PE_THIP(t, hipSetDevice(t->device));
    set->n = 0;
    const size_t fb = (size_t)n * t->T * t->F * sizeof(float);
    if ((rc = train_reserve(t, slot, fb)) || (rc = train_reserve(t, train_targets_of(slot), (size_t)n * sizeof(float)))) return rc;
    PE_THIP(t, hipMemcpy(t->buf[slot].p, feats_host, fb, hipMemcpyHostToDevice));
    PE_THIP(t, hipMemcpy(t->buf[train_targets_of(slot)].p, targets_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    set->feats = static_cast<const float*>(t->buf[slot].p);
    set->targets = static_cast<const float*>(t->buf[train_targets_of(slot)].p);
    set->n = n;
    return PE_OK;
}

int train_step(pe_trainer* t, const char* who, const int32_t* indices_host, int n, uint64_t step, const pe_train_hparams* hp,
               float* loss_out) {
    if (!indices_host || !hp || !loss_out) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
    if (n <= 0) return tfail(t, PE_ERR_INVALID, "%s: n = %d", who, n);
    if (t->data.n <= 0) return tfail(t, PE_ERR_INVALID, "%s: no dataset (call pe_trainer_set_data first)", who);
    for (int m = 0; m < t->K; ++m)
        if (!(hp[m].dropout_rate >= 0.0f && hp[m].dropout_rate < 1.0f))
            return tfail(t, PE_ERR_INVALID, "%sdropout rate %g is outside [0, 1)", train_model_prefix(t->K, m).c_str(), (double)hp[m].dropout_rate);
    for (int i = 0; i < n; ++i)
        if (indices_host[i] < 0 || indices_host[i] >= t->data.n)
            return tfail(t, PE_ERR_INVALID, "indices[%d] = %d is outside the dataset of %d samples", i, indices_host[i], t->data.n);
    PE_THIP(t, hipSetDevice(t->device));
    int rc = train_reserve(t, kBufIndices, (size_t)n * sizeof(int32_t));
    if (rc) return rc;
    PE_THIP(t, hipMemcpy(t->buf[kBufIndices].p, indices_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    TrainArgs a{};
    a.n = n;
    a.feats = t->data.feats;
    a.targets = t->data.targets;
    a.indices = static_cast<const int32_t*>(t->buf[kBufIndices].p);
    a.apply = 1;
    for (int m = 0; m < t->K; ++m) {
        TrainModel& r = a.model[m];
        if (hp[m].dropout_rate > 0.0f) {
            r.mask_mode = 2;
            r.mask_key = train_mask_key(hp[m].seed, step);
            r.rate = hp[m].dropout_rate;
            r.keep_scale = train_keep_scale(hp[m].dropout_rate);
        }
        r.beta = hp[m].loss_bias;
        r.lr = hp[m].lr; r.rho = hp[m].rho; r.eps = hp[m].eps;
        r.frozen_mask = hp[m].frozen_mask;
    }
    if ((rc = train_run(t, a, true))) return rc;
    PE_THIP(t, hipMemcpy(loss_out, t->loss, (size_t)t->K * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

int train_results(pe_trainer* t, const float* probs_dev, const float* targets_dev, int n, float* loss_out, float* acc_out, float* probs_out);

int train_evaluate(pe_trainer* t, const char* who, int source, const float* feats_host, const float* targets_host, int n,
                   const float* loss_bias, float* loss_out, float* acc_out, float* probs_out) {
    const TrainSet* set = nullptr;
    if (source == PE_TRAIN_SOURCE_HOST) {
        if (!feats_host) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
        if (!targets_host && (loss_out || acc_out)) return tfail(t, PE_ERR_INVALID, "%s: loss and accuracy need targets", who);
        if (n <= 0) return tfail(t, PE_ERR_INVALID, "%s: n = %d", who, n);
    } else if (source == PE_TRAIN_SOURCE_DATA || source == PE_TRAIN_SOURCE_VALIDATION) {
        set = source == PE_TRAIN_SOURCE_DATA ? &t->data : &t->validation;
        if (set->n <= 0)
            return tfail(t, PE_ERR_INVALID, "%s: no resident %s set (call %s first)", who, source == PE_TRAIN_SOURCE_DATA ? "training" : "validation",
                         source == PE_TRAIN_SOURCE_DATA ? "pe_trainer_set_data" : "pe_trainer_set_validation");
        n = set->n;
    } else {
        return tfail(t, PE_ERR_INVALID, "%s: source = %d", who, source);
    }
    if (loss_out && !loss_bias) return tfail(t, PE_ERR_INVALID, "%s: a loss needs loss_bias", who);
    int rc = (!set && targets_host) ? train_check_targets(t, targets_host, n) : PE_OK;
    if (rc) return rc;
    PE_THIP(t, hipSetDevice(t->device));
    TrainArgs a{};
    if (set) {
        a.n = n;
        a.feats = set->feats;
        a.targets = set->targets;
    } else if ((rc = train_upload_batch(t, feats_host, targets_host, n, &a))) {
        return rc;
    }
    for (int m = 0; m < t->K; ++m) a.model[m].beta = loss_bias ? loss_bias[m] : 0.0f;
    if ((rc = train_run(t, a, false))) return rc;
    return train_results(t, a.probs, a.targets, n, loss_out, acc_out, probs_out);
}

// what an evaluation brings back after train_run(forward): targets_dev[n] are the targets of the n samples in launch order
int train_results(pe_trainer* t, const float* probs_dev, const float* targets_dev, int n, float* loss_out, float* acc_out, float* probs_out) {
    const int K = t->K;
    int32_t* const hits = reinterpret_cast<int32_t*>(t->loss + K);
    if (acc_out) {
        TrainAccuracyArgs c{probs_dev, targets_dev, n, hits};
        PE_THIP(t, launch_train_accuracy(c, K, nullptr));
    }
    float back[2 * kTrainMaxModels];
    PE_THIP(t, hipMemcpy(back, t->loss, (size_t)(acc_out ? 2 : 1) * K * sizeof(float), hipMemcpyDeviceToHost));
    if (probs_out) PE_THIP(t, hipMemcpy(probs_out, probs_dev, (size_t)K * n * sizeof(float), hipMemcpyDeviceToHost));
    if (loss_out) memcpy(loss_out, back, (size_t)K * sizeof(float));
    if (acc_out)                                       // Keras binary_accuracy: mean(round(p) == y), ties to even
        for (int m = 0; m < K; ++m) {
            int32_t h;
            memcpy(&h, back + K + m, sizeof h);
            acc_out[m] = (float)((double)h / n);
        }
    return PE_OK;
}

int train_one_model_only(pe_trainer* t, const char* who, const char* instead) {
    if (t->K == 1) return PE_OK;
    return tfail(t, PE_ERR_UNSUPPORTED, "%s: this trainer holds n_models = %d networks%s%s", who, t->K, instead ? "; call " : " (one-network entry point)",
                 instead ? instead : "");
}

}  // namespace

extern "C" {

const char* pe_trainer_last_error(const pe_trainer* t) { return t ? t->err.c_str() : g_global_error.c_str(); }

int pe_trainer_destroy(pe_trainer* t) {
    if (!t) return PE_OK;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    for (DeviceBuf& b : t->buf) if (b.p) (void)hipFree(b.p);
    for (float* p : {t->theta, t->accum, t->grads, t->loss}) if (p) (void)hipFree(p);
    delete t;
    return PE_OK;
}

namespace {
int trainer_create(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t n_models, int32_t device, pe_trainer** out,
                   const int max_units, const bool stacked = false) {
    if (!init || !out) return tfail(nullptr, PE_ERR_INVALID, "pe_trainer_create: null argument");
    *out = nullptr;
    if (n_models < 1) return tfail(nullptr, PE_ERR_INVALID, "pe_trainer_create: n_models = %d", n_models);
    if (n_models > PE_TRAIN_MAX_MODELS)
        return tfail(nullptr, PE_ERR_UNSUPPORTED, "training: n_models = %d (1..%d)", n_models, PE_TRAIN_MAX_MODELS);
    if (feature_size < 1 || feature_size > kTrainMaxFeat)
        return tfail(nullptr, PE_ERR_UNSUPPORTED, "training: feature_size = %d (1..%d)", feature_size, kTrainMaxFeat);
    if (n_features < 1 || n_features > kTrainMaxSteps)
        return tfail(nullptr, PE_ERR_UNSUPPORTED, "training: n_features = %d (1..%d)", n_features, kTrainMaxSteps);
    for (int m = 0; m < n_models; ++m) {
        const pe_weights& w = init[m];
        const std::string pre = train_model_prefix(n_models, m);
        if (stacked && (w.n_layers < 1 || w.n_layers > 2))
            return tfail(nullptr, PE_ERR_UNSUPPORTED, "%straining: n_layers = %d (1..2)", pre.c_str(), w.n_layers);
        if (!stacked && w.n_layers != 1)
            return tfail(nullptr, PE_ERR_UNSUPPORTED, "%straining: n_layers = %d (one GRU layer has a training kernel)", pre.c_str(), w.n_layers);
        if (!w.layers || !w.dense_kernel) return tfail(nullptr, PE_ERR_INVALID, "%spe_trainer_create: null weight array", pre.c_str());
        for (int l = 0; l < w.n_layers; ++l)
            if (!w.layers[l].kernel || !w.layers[l].recurrent_kernel || !w.layers[l].bias)
                return tfail(nullptr, PE_ERR_INVALID, "%spe_trainer_create: null weight array", pre.c_str());
        for (int l = 0; l < w.n_layers; ++l) {
            const int H = w.layers[l].units;
            if (H < 1 || H > max_units) return tfail(nullptr, PE_ERR_UNSUPPORTED, "%straining: units = %d (1..%d)", pre.c_str(), H, max_units);
        }
        if (w.layers[0].n_in != feature_size)
            return tfail(nullptr, PE_ERR_INVALID, "%sthe GRU layer takes %d inputs, feature_size is %d", pre.c_str(), w.layers[0].n_in, feature_size);
        if (w.n_layers == 2 && w.layers[1].n_in != w.layers[0].units)
            return tfail(nullptr, PE_ERR_INVALID, "%sGRU layer 1 takes %d inputs, layer 0 has %d units", pre.c_str(), w.layers[1].n_in,
                         w.layers[0].units);
    }
    hipError_t herr = hipSetDevice(device);
    if (herr != hipSuccess) return tfail(nullptr, PE_ERR_HIP, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(herr));
    pe_trainer* t = new pe_trainer;
    t->device = device;
    t->T = n_features; t->F = feature_size; t->K = n_models;
    for (int m = 0; m < n_models; ++m) {
        t->H[m] = init[m].layers[0].units;
        t->H2[m] = init[m].n_layers == 2 ? init[m].layers[1].units : 0;
        t->ofs[m + 1] = t->ofs[m] + (t->H2[m] ? ts_n_params(feature_size, t->H[m], t->H2[m]) : train_n_params(feature_size, t->H[m]));
    }
    t->n_params = t->ofs[n_models];
    const size_t pb = (size_t)t->n_params * sizeof(float);
    for (float** p : {&t->theta, &t->accum, &t->grads, &t->loss}) {
        const size_t bytes = p == &t->loss ? (size_t)2 * kTrainMaxModels * sizeof(float) : pb;
        herr = hipMalloc(reinterpret_cast<void**>(p), bytes);
        if (herr != hipSuccess) {
            *p = nullptr;
            pe_trainer_destroy(t);
            return tfail(nullptr, PE_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(herr));
        }
    }
    std::vector<float> flat((size_t)t->n_params);
    const int F = feature_size;
    for (int m = 0; m < n_models; ++m) {
        const int H = t->H[m], H3 = 3 * H;
        float* f = flat.data() + t->ofs[m];
        memcpy(f, init[m].layers[0].kernel, (size_t)F * H3 * sizeof(float));
        memcpy(f + F * H3, init[m].layers[0].recurrent_kernel, (size_t)H * H3 * sizeof(float));
        memcpy(f + (F + H) * H3, init[m].layers[0].bias, (size_t)H3 * sizeof(float));
        f += (F + H + 1) * H3;
        int last = H;
        if (t->H2[m]) {
            const int G = t->H2[m], G3 = 3 * G;
            memcpy(f, init[m].layers[1].kernel, (size_t)H * G3 * sizeof(float));
            memcpy(f + H * G3, init[m].layers[1].recurrent_kernel, (size_t)G * G3 * sizeof(float));
            memcpy(f + (H + G) * G3, init[m].layers[1].bias, (size_t)G3 * sizeof(float));
            f += (H + G + 1) * G3;
            last = G;
        }
        memcpy(f, init[m].dense_kernel, (size_t)last * sizeof(float));
        f[last] = init[m].dense_bias;
    }
    int rc = pe_trainer_set_weights(t, flat.data());
    if (!rc) rc = pe_trainer_reset_optimizer(t);
    if (rc) {
        g_global_error = t->err;
        pe_trainer_destroy(t);
        return rc;
    }
    *out = t;
    return PE_OK;
}
}  // namespace

int pe_trainer_create_models(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t n_models, int32_t device,
                             pe_trainer** out) {
    return trainer_create(n_features, feature_size, init, n_models, device, out, kTrainMaxUnits);
}

int pe_trainer_create_wide(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t n_models, int32_t device,
                           pe_trainer** out) {
    return trainer_create(n_features, feature_size, init, n_models, device, out, kTwMaxUnits);
}

int pe_trainer_create_stacked(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t n_models, int32_t device,
                              pe_trainer** out) {
    return trainer_create(n_features, feature_size, init, n_models, device, out, kTwMaxUnits, true);
}

int pe_trainer_create(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t device, pe_trainer** out) {
    return pe_trainer_create_models(n_features, feature_size, init, 1, device, out);
}

int pe_trainer_n_models(const pe_trainer* t) { return t ? t->K : -1; }
int pe_trainer_n_params(const pe_trainer* t) { return t ? t->n_params : -1; }
int pe_trainer_n_samples(const pe_trainer* t, int32_t source) {
    if (!t || (source != PE_TRAIN_SOURCE_DATA && source != PE_TRAIN_SOURCE_VALIDATION)) return -1;
    return source == PE_TRAIN_SOURCE_DATA ? t->data.n : t->validation.n;
}
int pe_trainer_n_params_model(const pe_trainer* t, int32_t m) { return t && m >= 0 && m < t->K ? t->ofs[m + 1] - t->ofs[m] : -1; }

int pe_trainer_get_weights(pe_trainer* t, float* flat_out) {
    if (!t) return PE_ERR_INVALID;
    if (!flat_out) return tfail(t, PE_ERR_INVALID, "pe_trainer_get_weights: null pointer");
    PE_THIP(t, hipSetDevice(t->device));
    PE_THIP(t, hipMemcpy(flat_out, t->theta, (size_t)t->n_params * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_trainer_set_weights(pe_trainer* t, const float* flat) {
    if (!t) return PE_ERR_INVALID;
    if (!flat) return tfail(t, PE_ERR_INVALID, "pe_trainer_set_weights: null pointer");
    PE_THIP(t, hipSetDevice(t->device));
    PE_THIP(t, hipMemcpy(t->theta, flat, (size_t)t->n_params * sizeof(float), hipMemcpyHostToDevice));
    return PE_OK;
}

int pe_trainer_get_accumulators(pe_trainer* t, float* flat_out) {
    if (!t) return PE_ERR_INVALID;
    if (!flat_out) return tfail(t, PE_ERR_INVALID, "pe_trainer_get_accumulators: null pointer");
    PE_THIP(t, hipSetDevice(t->device));
    PE_THIP(t, hipMemcpy(flat_out, t->accum, (size_t)t->n_params * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_trainer_reset_optimizer(pe_trainer* t) {
    if (!t) return PE_ERR_INVALID;
    PE_THIP(t, hipSetDevice(t->device));
    PE_THIP(t, hipMemset(t->accum, 0, (size_t)t->n_params * sizeof(float)));
    return PE_OK;
}

int pe_trainer_loss_grad(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n, const float* masks_host,
                         float loss_bias, float* loss_out, float* grads_out, float* probs_out) {
    if (!t) return PE_ERR_INVALID;
    int rc = train_one_model_only(t, "pe_trainer_loss_grad", nullptr);
    if (rc) return rc;
    if (!feats_host || !targets_host || !loss_out || !grads_out) return tfail(t, PE_ERR_INVALID, "pe_trainer_loss_grad: null pointer");
    if (n <= 0) return tfail(t, PE_ERR_INVALID, "pe_trainer_loss_grad: n = %d", n);
    if ((rc = train_check_targets(t, targets_host, n))) return rc;
    PE_THIP(t, hipSetDevice(t->device));
    TrainArgs a{};
    if ((rc = train_upload_batch(t, feats_host, targets_host, n, &a))) return rc;
    if (masks_host) {
        const size_t mb = (size_t)3 * n * (t->F + (t->H2[0] ? t->H[0] : 0)) * sizeof(float);      // stacked: then [3][n][H1]
        if ((rc = train_reserve(t, kBufMasks, mb))) return rc;
        PE_THIP(t, hipMemcpy(t->buf[kBufMasks].p, masks_host, mb, hipMemcpyHostToDevice));
        a.model[0].mask_mode = 1;
        a.masks = static_cast<const float*>(t->buf[kBufMasks].p);
    }
    a.model[0].beta = loss_bias;
    if ((rc = train_run(t, a, true))) return rc;
    PE_THIP(t, hipMemcpy(loss_out, t->loss, sizeof(float), hipMemcpyDeviceToHost));
    PE_THIP(t, hipMemcpy(grads_out, t->grads, (size_t)t->n_params * sizeof(float), hipMemcpyDeviceToHost));
    if (probs_out) PE_THIP(t, hipMemcpy(probs_out, t->buf[kBufProbs].p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_trainer_apply(pe_trainer* t, const float* grads_host, float lr, float rho, float eps, int32_t frozen_mask) {
    if (!t) return PE_ERR_INVALID;
    int rc = train_one_model_only(t, "pe_trainer_apply", nullptr);
    if (rc) return rc;
    if (!grads_host) return tfail(t, PE_ERR_INVALID, "pe_trainer_apply: null pointer");
    PE_THIP(t, hipSetDevice(t->device));
    PE_THIP(t, hipMemcpy(t->grads, grads_host, (size_t)t->n_params * sizeof(float), hipMemcpyHostToDevice));
    TrainArgs a{};
    TrainModel& r = a.model[0];
    r.lr = lr; r.rho = rho; r.eps = eps;
    r.frozen_mask = frozen_mask;
    if (t->H2[0]) {
        TrainStackedArgs w{};
        train_fill_common(t, a, false, 0, &w);
        train_stacked_units(t, 0, &w);
        PE_THIP(t, launch_train_stacked_apply(w, nullptr));
        PE_THIP(t, hipDeviceSynchronize());
        return PE_OK;
    }
    a.F = t->F; a.n_models = 1;
    a.n_total = t->n_params;
    a.grads = t->grads;
    a.theta = t->theta;
    a.accum = t->accum;
    r.H = t->H[0];
    PE_THIP(t, launch_train_apply(a, nullptr));
    PE_THIP(t, hipDeviceSynchronize());
    return PE_OK;
}

int pe_trainer_set_data(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n) {
    if (!t) return PE_ERR_INVALID;
    const int rc = train_upload_set(t, "pe_trainer_set_data", &t->data, kBufDataFeats, feats_host, targets_host, n);
    if (rc == PE_OK || t->data.n == 0) t->sample_n = t->n_selected = 0;      // a new set: nothing selected, every row eligible
    return rc;
}

int pe_trainer_set_validation(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n) {
    if (!t) return PE_ERR_INVALID;
    return train_upload_set(t, "pe_trainer_set_validation", &t->validation, kBufValFeats, feats_host, targets_host, n);
}

int pe_trainer_step_models(pe_trainer* t, const int32_t* indices_host, int32_t n, uint64_t step, const pe_train_hparams* hp,
                           float* loss_out) {
    if (!t) return PE_ERR_INVALID;
    return train_step(t, "pe_trainer_step_models", indices_host, n, step, hp, loss_out);
}

int pe_trainer_step(pe_trainer* t, const int32_t* indices_host, int32_t n, float dropout_rate, uint64_t seed, uint64_t step,
                    float loss_bias, float lr, float rho, float eps, int32_t frozen_mask, float* loss_out) {
    if (!t) return PE_ERR_INVALID;
    int rc = train_one_model_only(t, "pe_trainer_step", "pe_trainer_step_models");
    if (rc) return rc;
    const pe_train_hparams hp{dropout_rate, seed, loss_bias, lr, rho, eps, frozen_mask};
    return train_step(t, "pe_trainer_step", indices_host, n, step, &hp, loss_out);
}

int pe_trainer_evaluate_models(pe_trainer* t, int32_t source, const float* feats_host, const float* targets_host, int32_t n,
                               const float* loss_bias, float* loss_out, float* acc_out, float* probs_out) {
    if (!t) return PE_ERR_INVALID;
    return train_evaluate(t, "pe_trainer_evaluate_models", source, feats_host, targets_host, n, loss_bias, loss_out, acc_out, probs_out);
}

int pe_trainer_stats_models(pe_trainer* t, int32_t source, const float* feats_host, const float* targets_host, int32_t n,
                            const double* thresholds, int32_t n_thresholds, int32_t compare,
                            pe_stats_count* counts_out, pe_stats_summary* summary_out, float* probs_out) {
    const char* who = "pe_trainer_stats_models";
    if (!t) return PE_ERR_INVALID;
    const TrainSet* set = nullptr;
    if (source == PE_TRAIN_SOURCE_HOST) {
        if (!feats_host || !targets_host) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
    } else if (source == PE_TRAIN_SOURCE_DATA || source == PE_TRAIN_SOURCE_VALIDATION) {
        set = source == PE_TRAIN_SOURCE_DATA ? &t->data : &t->validation;
        if (set->n <= 0)
            return tfail(t, PE_ERR_INVALID, "%s: no resident %s set (call %s first)", who, source == PE_TRAIN_SOURCE_DATA ? "training" : "validation",
                         source == PE_TRAIN_SOURCE_DATA ? "pe_trainer_set_data" : "pe_trainer_set_validation");
        n = set->n;
    } else {
        return tfail(t, PE_ERR_INVALID, "%s: source = %d", who, source);
    }
    const StatsRequest q{thresholds, n_thresholds, compare, counts_out, summary_out};
    std::string wrong;
    if (stats_request_wrong(wrong, who, q, set ? nullptr : targets_host, n)) return tfail(t, PE_ERR_INVALID, "%s", wrong.c_str());
    // the forward pass of pe_trainer_evaluate_models: its probabilities stay in buffer 6, host targets arrive in buffer 1
    int rc = train_evaluate(t, who, source, feats_host, targets_host, n, nullptr, nullptr, nullptr, probs_out);
    if (rc) return rc;
    const StatsScratch s = stats_scratch(t->K, n, n_thresholds, false, false);
    if ((rc = train_reserve(t, kBufStats, s.total))) return rc;
    PE_THIP(t, stats_run(static_cast<char*>(t->buf[kBufStats].p), s, static_cast<const float*>(t->buf[kBufProbs].p), n,
                         set ? set->targets : static_cast<const float*>(t->buf[kBufTargets].p), n, t->K, q));
    return PE_OK;
}

int pe_trainer_evaluate(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n, float loss_bias,
                        float* loss_out, float* acc_out, float* probs_out) {
    if (!t) return PE_ERR_INVALID;
    int rc = train_one_model_only(t, "pe_trainer_evaluate", "pe_trainer_evaluate_models");
    if (rc) return rc;
    return train_evaluate(t, "pe_trainer_evaluate", PE_TRAIN_SOURCE_HOST, feats_host, targets_host, n, &loss_bias, loss_out, acc_out, probs_out);
}

int pe_train_dropout_masks(uint64_t seed, uint64_t step, int32_t n, int32_t feature_size, float rate, float* out) {
    if (!out) return tfail(nullptr, PE_ERR_INVALID, "pe_train_dropout_masks: null pointer");
    if (n <= 0) return tfail(nullptr, PE_ERR_INVALID, "pe_train_dropout_masks: n = %d", n);
    if (feature_size < 1 || feature_size > kTrainMaxFeat)
        return tfail(nullptr, PE_ERR_INVALID, "pe_train_dropout_masks: feature_size = %d (1..%d)", feature_size, kTrainMaxFeat);
    if (!(rate >= 0.0f && rate < 1.0f)) return tfail(nullptr, PE_ERR_INVALID, "dropout rate %g is outside [0, 1)", (double)rate);
    const uint64_t key = train_mask_key(seed, step);
    const float scale = train_keep_scale(rate);
    for (int g = 0; g < 3; ++g)
        for (int64_t i = 0; i < n; ++i)
            for (int f = 0; f < feature_size; ++f)
                out[((size_t)g * n + i) * feature_size + f] = train_mask_keep(key, g, i, f, rate) ? scale : 0.0f;
    return PE_OK;
}

int pe_train_dropout_masks_layer(uint64_t seed, uint64_t step, int32_t layer, int32_t n, int32_t width, float rate, float* out) {
    if (layer == 0) return pe_train_dropout_masks(seed, step, n, width, rate, out);
    if (layer != 1) return tfail(nullptr, PE_ERR_INVALID, "pe_train_dropout_masks_layer: layer = %d (0..1)", layer);
    if (!out) return tfail(nullptr, PE_ERR_INVALID, "pe_train_dropout_masks_layer: null pointer");
    if (n <= 0) return tfail(nullptr, PE_ERR_INVALID, "pe_train_dropout_masks_layer: n = %d", n);
    if (width < 1 || width > kTwMaxUnits)
        return tfail(nullptr, PE_ERR_INVALID, "pe_train_dropout_masks_layer: width = %d (1..%d)", width, kTwMaxUnits);
    if (!(rate >= 0.0f && rate < 1.0f)) return tfail(nullptr, PE_ERR_INVALID, "dropout rate %g is outside [0, 1)", (double)rate);
    const uint64_t key = train_mask_key_layer1(train_mask_key(seed, step));
    const float scale = train_keep_scale(rate);
    for (int g = 0; g < 3; ++g)
        for (int64_t i = 0; i < n; ++i)
            for (int f = 0; f < width; ++f)
                out[((size_t)g * n + i) * width + f] = train_mask_keep_layer1(key, g, i, f, rate) ? scale : 0.0f;
    return PE_OK;
}

}  // extern "C"

// ---- resident sets that grow (pe_trainer_append / pe_trainer_get_data; pe_miner_append below) ---------------------------------
namespace {

// buf[slot] holds at least `bytes`, its first `keep` bytes kept (device to device) when it has to move; grows by doubling
int train_grow(pe_trainer* t, TrainBuf slot, size_t keep, size_t bytes) {
    DeviceBuf& b = t->buf[slot];
    if (b.p && b.bytes >= bytes) return PE_OK;
    const size_t want = std::max(bytes, 2 * b.bytes);
    void* p = nullptr;
    hipError_t err = hipMalloc(&p, want ? want : 1);
    if (err != hipSuccess) return tfail(t, PE_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(err));
    if (b.p && keep) {
        err = hipMemcpy(p, b.p, keep, hipMemcpyDeviceToDevice);
        if (err != hipSuccess) { (void)hipFree(p); return tfail(t, PE_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(err)); }
    }
    if (b.p) (void)hipFree(b.p);
    b.p = p; b.bytes = want;
    return PE_OK;
}

// room for n more samples behind the resident set `source`: *set / *slot name it, its pointers follow the buffers
int train_set_room(pe_trainer* t, const char* who, int source, int n, TrainSet** set, TrainBuf* slot) {
    if (source != PE_TRAIN_SOURCE_DATA && source != PE_TRAIN_SOURCE_VALIDATION) return tfail(t, PE_ERR_INVALID, "%s: source = %d", who, source);
    *set = source == PE_TRAIN_SOURCE_DATA ? &t->data : &t->validation;
    *slot = source == PE_TRAIN_SOURCE_DATA ? kBufDataFeats : kBufValFeats;
    const int have = (*set)->n;
    if (n > 0x7fffffff - have) return tfail(t, PE_ERR_INVALID, "%s: %d + %d samples are more than a set holds", who, have, n);
    const size_t row = (size_t)t->T * t->F * sizeof(float);
    int rc;
    // (the set follows each buffer as soon as it has moved: a failure of the second leaves a valid set of `have` samples)
    if ((rc = train_grow(t, *slot, (size_t)have * row, (size_t)(have + n) * row))) return rc;
    (*set)->feats = static_cast<const float*>(t->buf[*slot].p);
    if ((rc = train_grow(t, train_targets_of(*slot), (size_t)have * sizeof(float), (size_t)(have + n) * sizeof(float)))) return rc;
    (*set)->targets = static_cast<const float*>(t->buf[train_targets_of(*slot)].p);
    return PE_OK;
}

// n samples whose rows are on the trainer's device already, every target = `target`
int train_append_device(pe_trainer* t, const char* who, int source, const float* feats_dev, int n, float target) {
    if (!(target >= 0.0f && target <= 1.0f)) return tfail(t, PE_ERR_INVALID, "%s: target %g is outside [0, 1]", who, (double)target);
    TrainSet* set; TrainBuf slot;
    PE_THIP(t, hipSetDevice(t->device));
    int rc = train_set_room(t, who, source, n, &set, &slot);
    if (rc) return rc;
    const size_t row = (size_t)t->T * t->F;
    const std::vector<float> y((size_t)n, target);
    PE_THIP(t, hipMemcpy(static_cast<float*>(t->buf[slot].p) + (size_t)set->n * row, feats_dev, (size_t)n * row * sizeof(float), hipMemcpyDeviceToDevice));
    PE_THIP(t, hipMemcpy(static_cast<float*>(t->buf[train_targets_of(slot)].p) + set->n, y.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    set->n += n;
    return PE_OK;
}

// ... one target per sample, on the device as well (the caller has checked that each lies in [0, 1])
int train_append_device_targets(pe_trainer* t, const char* who, int source, const float* feats_dev, const float* targets_dev, int n) {
    TrainSet* set; TrainBuf slot;
    PE_THIP(t, hipSetDevice(t->device));
    int rc = train_set_room(t, who, source, n, &set, &slot);
    if (rc) return rc;
    const size_t row = (size_t)t->T * t->F;
    PE_THIP(t, hipMemcpy(static_cast<float*>(t->buf[slot].p) + (size_t)set->n * row, feats_dev, (size_t)n * row * sizeof(float), hipMemcpyDeviceToDevice));
    PE_THIP(t, hipMemcpy(static_cast<float*>(t->buf[train_targets_of(slot)].p) + set->n, targets_dev, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice));
    set->n += n;
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_trainer_append(pe_trainer* t, int32_t source, const float* feats_host, const float* targets_host, int32_t n) {
    const char* who = "pe_trainer_append";
    if (!t) return PE_ERR_INVALID;
    if (!feats_host || !targets_host) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
    if (n <= 0) return tfail(t, PE_ERR_INVALID, "%s: n = %d", who, n);
    if (source != PE_TRAIN_SOURCE_DATA && source != PE_TRAIN_SOURCE_VALIDATION) return tfail(t, PE_ERR_INVALID, "%s: source = %d", who, source);
    int rc = train_check_targets(t, targets_host, n);
    if (rc) return rc;
    PE_THIP(t, hipSetDevice(t->device));
    TrainSet* set; TrainBuf slot;
    if ((rc = train_set_room(t, who, source, n, &set, &slot))) return rc;
    const size_t row = (size_t)t->T * t->F;
    PE_THIP(t, hipMemcpy(static_cast<float*>(t->buf[slot].p) + (size_t)set->n * row, feats_host, (size_t)n * row * sizeof(float), hipMemcpyHostToDevice));
    PE_THIP(t, hipMemcpy(static_cast<float*>(t->buf[train_targets_of(slot)].p) + set->n, targets_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    set->n += n;
    return PE_OK;
}

int pe_trainer_get_data(pe_trainer* t, int32_t source, int32_t first, int32_t n, float* feats_out, float* targets_out) {
    const char* who = "pe_trainer_get_data";
    if (!t) return PE_ERR_INVALID;
    if (source != PE_TRAIN_SOURCE_DATA && source != PE_TRAIN_SOURCE_VALIDATION) return tfail(t, PE_ERR_INVALID, "%s: source = %d", who, source);
    const TrainSet& set = source == PE_TRAIN_SOURCE_DATA ? t->data : t->validation;
    if (first < 0 || n < 0 || first > set.n || n > set.n - first)
        return tfail(t, PE_ERR_INVALID, "%s: samples %d .. %d + %d are outside the set of %d", who, first, first, n, set.n);
    if (n == 0) return PE_OK;
    PE_THIP(t, hipSetDevice(t->device));
    const size_t row = (size_t)t->T * t->F;
    if (feats_out) PE_THIP(t, hipMemcpy(feats_out, set.feats + (size_t)first * row, (size_t)n * row * sizeof(float), hipMemcpyDeviceToHost));
    if (targets_out) PE_THIP(t, hipMemcpy(targets_out, set.targets + first, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

}  // extern "C"

// ---- sampled training (pe_trainer_evaluate_indices / pe_trainer_sample_*; kernels: sample_device.h) ------------
static_assert(sizeof(pe_sample_report) == sizeof(SampleReport) && sizeof(SampleReport) == 48, "pe_sample_report is what the device writes");
static_assert(PE_SAMPLE_BLOCK_ROWS == kSampleBlock && PE_SAMPLE_MAX_NEW == kSampleBlock / 2, "a selection round halves the keys at least");

namespace {

// every row of the training set has its state byte, and the selection list has room for all of them
int sample_state_room(pe_trainer* t) {
    const int n = t->data.n;
    int rc;
    if ((rc = train_grow(t, kBufSampleState, (size_t)t->sample_n, (size_t)n))) return rc;
    if ((rc = train_grow(t, kBufSampleList, (size_t)t->n_selected * sizeof(int32_t), (size_t)n * sizeof(int32_t)))) return rc;
    if (t->sample_n < n) {
        PE_THIP(t, hipMemset(static_cast<uint8_t*>(t->buf[kBufSampleState].p) + t->sample_n, kSampleEligible, (size_t)(n - t->sample_n)));
        t->sample_n = n;
    }
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_trainer_evaluate_indices(pe_trainer* t, int32_t source, const int32_t* indices_host, int32_t n, const float* loss_bias,
                                float* loss_out, float* acc_out, float* probs_out) {
    const char* who = "pe_trainer_evaluate_indices";
    if (!t) return PE_ERR_INVALID;
    if (source != PE_TRAIN_SOURCE_DATA && source != PE_TRAIN_SOURCE_VALIDATION) return tfail(t, PE_ERR_INVALID, "%s: source = %d", who, source);
    const TrainSet& set = source == PE_TRAIN_SOURCE_DATA ? t->data : t->validation;
    if (set.n <= 0)
        return tfail(t, PE_ERR_INVALID, "%s: no resident %s set (call %s first)", who, source == PE_TRAIN_SOURCE_DATA ? "training" : "validation",
                     source == PE_TRAIN_SOURCE_DATA ? "pe_trainer_set_data" : "pe_trainer_set_validation");
    if (!indices_host) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
    if (n <= 0) return tfail(t, PE_ERR_INVALID, "%s: n = %d", who, n);
    if (loss_out && !loss_bias) return tfail(t, PE_ERR_INVALID, "%s: a loss needs loss_bias", who);
    for (int i = 0; i < n; ++i)
        if (indices_host[i] < 0 || indices_host[i] >= set.n)
            return tfail(t, PE_ERR_INVALID, "%s: indices[%d] = %d is outside the set of %d samples", who, i, indices_host[i], set.n);
    PE_THIP(t, hipSetDevice(t->device));
    int rc = train_reserve(t, kBufIndices, (size_t)n * sizeof(int32_t));
    if (rc) return rc;
    PE_THIP(t, hipMemcpy(t->buf[kBufIndices].p, indices_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    TrainArgs a{};
    a.n = n;
    a.feats = set.feats;
    a.targets = set.targets;
    a.indices = static_cast<const int32_t*>(t->buf[kBufIndices].p);
    for (int m = 0; m < t->K; ++m) a.model[m].beta = loss_bias ? loss_bias[m] : 0.0f;
    if ((rc = train_run(t, a, false))) return rc;
    const float* targets = nullptr;
    if (acc_out) {                                      // the accuracy count reads targets in launch order
        if ((rc = train_reserve(t, kBufTargets, (size_t)n * sizeof(float)))) return rc;
        SampleGatherArgs g{set.targets, a.indices, n, static_cast<float*>(t->buf[kBufTargets].p)};
        PE_THIP(t, launch_sample_gather_targets(g, nullptr));
        targets = g.out;
    }
    return train_results(t, a.probs, targets, n, loss_out, acc_out, probs_out);
}

int pe_trainer_sample_reset(pe_trainer* t, const uint8_t* eligible_host, const int32_t* selected_host, int32_t n_selected) {
    const char* who = "pe_trainer_sample_reset";
    if (!t) return PE_ERR_INVALID;
    const int n = t->data.n;
    if (n <= 0) return tfail(t, PE_ERR_INVALID, "%s: no resident training set (call pe_trainer_set_data first)", who);
    if (n_selected < 0 || n_selected > n) return tfail(t, PE_ERR_INVALID, "%s: n_selected = %d for a set of %d samples", who, n_selected, n);
    if (n_selected > 0 && !selected_host) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
    std::vector<uint8_t> state((size_t)n);
    for (int i = 0; i < n; ++i) state[i] = (!eligible_host || eligible_host[i]) ? kSampleEligible : 0;
    for (int i = 0; i < n_selected; ++i) {
        const int32_t r = selected_host[i];
        if (r < 0 || r >= n) return tfail(t, PE_ERR_INVALID, "%s: selected[%d] = %d is outside the set of %d samples", who, i, r, n);
        if (state[r] & kSampleSelected) return tfail(t, PE_ERR_INVALID, "%s: selected[%d] = %d is repeated", who, i, r);
        if (!(state[r] & kSampleEligible)) return tfail(t, PE_ERR_INVALID, "%s: selected[%d] = %d is not an eligible row", who, i, r);
        state[r] |= kSampleSelected;
    }
    PE_THIP(t, hipSetDevice(t->device));
    int rc;
    if ((rc = train_grow(t, kBufSampleState, 0, (size_t)n)) || (rc = train_grow(t, kBufSampleList, 0, (size_t)n * sizeof(int32_t)))) return rc;
    PE_THIP(t, hipMemcpy(t->buf[kBufSampleState].p, state.data(), (size_t)n, hipMemcpyHostToDevice));
    if (n_selected) PE_THIP(t, hipMemcpy(t->buf[kBufSampleList].p, selected_host, (size_t)n_selected * sizeof(int32_t), hipMemcpyHostToDevice));
    t->sample_n = n;
    t->n_selected = n_selected;
    return PE_OK;
}

int pe_trainer_sample_choose(pe_trainer* t, int32_t model, int32_t max_new, int32_t order, pe_sample_report* report, int32_t* added_out,
                             float* probs_out) {
    const char* who = "pe_trainer_sample_choose";
    if (!t) return PE_ERR_INVALID;
    if (!report) return tfail(t, PE_ERR_INVALID, "%s: null pointer", who);
    if (model < 0 || model >= t->K) return tfail(t, PE_ERR_INVALID, "%s: model = %d of %d", who, model, t->K);
    if (order != PE_SAMPLE_ORDER_INDEX && order != PE_SAMPLE_ORDER_ERROR) return tfail(t, PE_ERR_INVALID, "%s: order = %d", who, order);
    if (max_new < 0) return tfail(t, PE_ERR_INVALID, "%s: max_new = %d", who, max_new);
    if (max_new > PE_SAMPLE_MAX_NEW) return tfail(t, PE_ERR_UNSUPPORTED, "%s: max_new = %d (at most %d per call)", who, max_new, PE_SAMPLE_MAX_NEW);
    const int n = t->data.n;
    if (n <= 0) return tfail(t, PE_ERR_INVALID, "%s: no resident training set (call pe_trainer_set_data first)", who);
    PE_THIP(t, hipSetDevice(t->device));
    int rc = sample_state_room(t);
    if (rc) return rc;
    // scratch: counters[4] | report | added[PE_SAMPLE_MAX_NEW] | keys_a | keys_b
    const size_t head = 4 * sizeof(unsigned long long), tail = sizeof(SampleReport) + (size_t)PE_SAMPLE_MAX_NEW * sizeof(int32_t);
    const size_t keys = (size_t)sample_blocks(n) * max_new;
    if ((rc = train_reserve(t, kBufSampleScratch, head + tail + 2 * keys * sizeof(unsigned long long)))) return rc;
    char* const scratch = static_cast<char*>(t->buf[kBufSampleScratch].p);
    TrainArgs f{};
    f.n = n;
    f.feats = t->data.feats;
    f.targets = t->data.targets;
    if ((rc = train_run(t, f, false))) return rc;
    SampleArgs a{};
    a.probs = f.probs + (size_t)model * n;
    a.targets = t->data.targets;
    a.state = static_cast<uint8_t*>(t->buf[kBufSampleState].p);
    a.n = n;
    a.k = max_new;
    a.order = order;
    a.counters = reinterpret_cast<unsigned long long*>(scratch);
    a.report = reinterpret_cast<SampleReport*>(scratch + head);
    a.added = reinterpret_cast<int32_t*>(scratch + head + sizeof(SampleReport));
    a.selection = static_cast<int32_t*>(t->buf[kBufSampleList].p);
    a.n_selected = t->n_selected;
    unsigned long long* const keys_a = reinterpret_cast<unsigned long long*>(scratch + head + tail);
    PE_THIP(t, hipMemsetAsync(a.counters, 0, head, nullptr));
    PE_THIP(t, launch_sample_choose(a, keys ? keys_a : nullptr, keys ? keys_a + keys : nullptr, nullptr));
    std::vector<char> back(sizeof(SampleReport) + (size_t)max_new * sizeof(int32_t));       // one copy: the report and the ids
    PE_THIP(t, hipMemcpy(back.data(), a.report, back.size(), hipMemcpyDeviceToHost));
    memcpy(report, back.data(), sizeof(SampleReport));
    if (added_out && report->n_added > 0) memcpy(added_out, back.data() + sizeof(SampleReport), (size_t)report->n_added * sizeof(int32_t));
    t->n_selected = (int)report->n_selected;
    if (probs_out) PE_THIP(t, hipMemcpy(probs_out, a.probs, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_trainer_sample_selected(pe_trainer* t, int32_t* out) {
    if (!t) return PE_ERR_INVALID;
    if (t->n_selected == 0) return PE_OK;
    if (!out) return tfail(t, PE_ERR_INVALID, "pe_trainer_sample_selected: null pointer");
    PE_THIP(t, hipSetDevice(t->device));
    PE_THIP(t, hipMemcpy(out, t->buf[kBufSampleList].p, (size_t)t->n_selected * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_trainer_n_selected(const pe_trainer* t) { return t ? t->n_selected : -1; }

}  // extern "C"

// ---- what the data sessions below share: each step of a session's host side that is not its own, stated once ------------------
namespace {

// A session keeps its device buffers in one array indexed by its enum, as pe_trainer does: the enum declares a buffer, ensure
// grows it, and this gives back all of them when the session goes -- with their bytes, which pe_info.device_bytes counts
void release_buffers(pe_engine* e, DeviceBuf* first, int count) {
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    for (DeviceBuf* b = first; b != first + count; ++b)
        if (b->p) { (void)hipFree(b->p); e->device_bytes -= (int64_t)b->bytes; }
}

// offsets[n + 1] of a pool of recordings (`what`); need_samples: a pool that must hold an entry, and samples in every entry
int check_offsets(pe_engine* e, const char* who, const char* what, const int64_t* offsets, int32_t n, bool need_samples) {
    if (need_samples && n < 1) return fail(e, PE_ERR_INVALID, "%s: %d %ss (at least one is needed)", who, n, what);
    if (n < 0) return fail(e, PE_ERR_INVALID, "%s: %d %ss", who, n, what);
    if (n > 0 && !offsets) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    if (n > 0 && offsets[0] != 0) return fail(e, PE_ERR_INVALID, "%s: %s offsets[0] must be 0, got %lld", who, what, (long long)offsets[0]);
    for (int32_t r = 0; r < n; ++r) {
        if (offsets[r + 1] < offsets[r])
            return fail(e, PE_ERR_INVALID, "%s: offsets decrease at %s %d (%lld after %lld)", who, what, r, (long long)offsets[r + 1], (long long)offsets[r]);
        if (need_samples && offsets[r + 1] == offsets[r]) return fail(e, PE_ERR_INVALID, "%s: %s %d is empty", who, what, r);
    }
    return PE_OK;
}

// the geometry of a mine_gather launch over the engine's rows; where the windows lie is the caller's
MineGatherArgs gather_geometry(const pe_engine* e) {
    MineGatherArgs g{};
    g.T = e->prm.n_features; g.F = e->n_in; g.use_delta = e->prm.use_delta ? 1 : 0; g.row_floats = e->row_floats;
    return g;
}

// may a session of `e` append its windows behind the resident set `source` of `trainer`?
int check_append(pe_engine* e, const char* who, const pe_trainer* trainer, int source) {
    if (!trainer) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    const int width = window_floats(e);
    if (trainer->device != e->device) return fail(e, PE_ERR_INVALID, "%s: the trainer lives on device %d, the engine on %d", who, trainer->device, e->device);
    if (trainer->F != width || trainer->T != e->prm.n_features)
        return fail(e, PE_ERR_INVALID, "%s: the trainer takes [%d][%d] inputs, the engine's windows are [%d][%d]", who, trainer->T, trainer->F, e->prm.n_features, width);
    if (source != PE_TRAIN_SOURCE_DATA && source != PE_TRAIN_SOURCE_VALIDATION) return fail(e, PE_ERR_INVALID, "%s: source = %d", who, source);
    return PE_OK;
}
int check_targets(pe_engine* e, const char* who, const float* targets, int32_t n) {
    for (int32_t i = 0; i < n; ++i)
        if (!(targets[i] >= 0.0f && targets[i] <= 1.0f)) return fail(e, PE_ERR_INVALID, "%s: targets[%d] = %g is outside [0, 1]", who, i, (double)targets[i]);
    return PE_OK;
}

// what a train_append_* call said, as the engine's own error
int trainer_said(pe_engine* e, const pe_trainer* trainer, int trc) { return trc ? fail(e, trc, "%s", trainer->err.c_str()) : PE_OK; }

// the end of a pass that appends: the targets of its k windows go up, the null stream finishes rows_dev, the trainer copies both
int rows_to_trainer(pe_engine* e, const char* who, pe_trainer* trainer, int source, const float* rows_dev, const float* targets_host, int k,
                    DeviceBuf& targets_buf) {
    int rc = ensure(e, targets_buf, (size_t)k * sizeof(float));
    if (rc) return rc;
    PE_HIP(e, hipMemcpy(targets_buf.p, targets_host, (size_t)k * sizeof(float), hipMemcpyHostToDevice));
    PE_HIP(e, hipStreamSynchronize(nullptr));
    return trainer_said(e, trainer, train_append_device_targets(trainer, who, source, rows_dev, static_cast<const float*>(targets_buf.p), k));
}

// ---- mining false activations (pe_miner; kernels: mine_device.h) ----------------------------------------------
enum MinerBuf {
    // resident: the samples as given, the three prefix sums [n_rec + 1] each (chunks, frames, samples), every frame's float32 row
    kMineAudio, kMineTables, kMineRows,
    // grown on demand: a pass's network input and its predictions [n_models][pass]; a scan's predictions, decoded values, block
    // counts and hit ids; a pass's hit ids, saved clips, clip table, float64 rows / float32 rows and packed trainer rows
    kMineBatch, kMinePred, kMineScores, kMineConf, kMineCounts, kMineHits, kMineIds, kMineRing, kMineClips, kMineFeats64, kMineClipRows, kMinePacked, kMineBufCount
};

}  // namespace

struct pe_miner {
    pe_engine* e = nullptr;
    int n_rec = 0, chunk = 0, buffer_samples = 0, carry_audio = 1, audio_f32 = 0;
    int64_t total_chunks = 0, total_frames = 0;
    std::vector<int64_t> chunk_prefix;                  // [n_rec + 1]
    DeviceBuf buf[kMineBufCount];                       // MinerBuf
    const long long* d_chunk_prefix() const { return static_cast<const long long*>(buf[kMineTables].p); }
    const long long* d_frame_base() const { return d_chunk_prefix() + n_rec + 1; }
    const long long* d_rec_start() const { return d_chunk_prefix() + 2 * (n_rec + 1); }
};

namespace {

void miner_free(pe_miner* m) { release_buffers(m->e, m->buf, kMineBufCount); delete m; }

MineGatherArgs miner_gather_args(const pe_miner* m) {
    MineGatherArgs g = gather_geometry(m->e);
    g.chunk = m->chunk; g.emit_window = emit_window(m->e->prm); g.hop = m->e->prm.hop_samples;
    return g;
}

int miner_check_hits(pe_miner* m, const char* who, const int32_t* hits, int32_t n) {
    pe_engine* e = m->e;
    if (n < 0) return fail(e, PE_ERR_INVALID, "%s: n=%d", who, n);
    if (n > 0 && !hits) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    for (int32_t i = 0; i < n; ++i)
        if (hits[i] < 0 || hits[i] >= m->total_chunks)
            return fail(e, PE_ERR_INVALID, "%s: hits[%d] = %d is outside the session's %lld chunks", who, i, hits[i], (long long)m->total_chunks);
    return PE_OK;
}

// The saved samples of hits[0 .. n) in passes: per pass the ids go up, mine_ring builds the clips, the clip front end writes
// their windows -- float64 rows to feats_out_host, or float32 rows that mine_gather packs for the trainer
int miner_rows(pe_miner* m, const char* who, const int32_t* hits, int32_t n, double* feats_out_host, pe_trainer* trainer, int source, float target) {
    pe_engine* e = m->e;
    int rc = miner_check_hits(m, who, hits, n);
    if (rc) return rc;
    if (n == 0) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const int T = e->prm.n_features, B = m->buffer_samples;
    const int width = window_floats(e);
    int64_t per_pass = e->clip_pass_bytes / ((int64_t)B * (int64_t)sizeof(float));
    per_pass = std::max<int64_t>(1, std::min<int64_t>(per_pass, 32768));
    std::vector<ClipDesc> desc;
    std::vector<uint32_t> prefix;
    for (int32_t h0 = 0; h0 < n; h0 += (int32_t)per_pass) {
        const int k = (int)std::min<int64_t>(per_pass, n - h0);
        desc.resize((size_t)k); prefix.resize((size_t)k + 1);
        uint32_t tasks = 0;
        // vectorize() of a clip of B samples (no crop: buffer_samples <= max_samples, params.py:74,95): the same for every hit
        for (int i = 0; i < k; ++i) { prefix[(size_t)i] = tasks; desc[(size_t)i] = clip_desc(e->prm, T, (int64_t)(i + 1) * B, B, 0, tasks); }
        prefix[(size_t)k] = tasks;
        if ((rc = ensure(e, m->buf[kMineIds], (size_t)k * sizeof(int32_t)))) return rc;
        if ((rc = ensure(e, m->buf[kMineRing], (size_t)k * B * sizeof(float)))) return rc;
        PE_HIP(e, hipMemcpy(m->buf[kMineIds].p, hits + h0, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice));
        ClipTable ct;
        PE_HIP(e, upload_task_table(e, m->buf[kMineClips], desc, prefix, m->buf[kMineRing].p, 1, ct, rc));
        if (rc) return rc;
        MineRingArgs r{static_cast<const int32_t*>(m->buf[kMineIds].p), k, m->d_chunk_prefix(), m->d_rec_start(), m->n_rec, m->chunk, B, m->carry_audio,
                       m->buf[kMineAudio].p, m->audio_f32, static_cast<float*>(m->buf[kMineRing].p)};
        PE_HIP(e, launch_mine_ring(r, nullptr));
        if (feats_out_host) {
            const size_t fb = (size_t)k * T * e->prm.n_mfcc * sizeof(double);
            if ((rc = ensure(e, m->buf[kMineFeats64], fb))) return rc;
            if ((rc = launch_clip_front_end(e, ct, static_cast<double*>(m->buf[kMineFeats64].p), nullptr, nullptr))) return rc;
            PE_HIP(e, hipMemcpy(feats_out_host + (size_t)h0 * T * e->prm.n_mfcc, m->buf[kMineFeats64].p, fb, hipMemcpyDeviceToHost));
        } else {
            if ((rc = ensure(e, m->buf[kMineClipRows], (size_t)k * T * e->row_floats * sizeof(float)))) return rc;
            if ((rc = ensure(e, m->buf[kMinePacked], (size_t)k * T * width * sizeof(float)))) return rc;
            if ((rc = launch_clip_front_end(e, ct, nullptr, static_cast<float*>(m->buf[kMineClipRows].p), nullptr))) return rc;
            MineGatherArgs g = miner_gather_args(m);
            g.rows = static_cast<const float*>(m->buf[kMineClipRows].p);
            g.n = k;
            g.out = static_cast<float*>(m->buf[kMinePacked].p);
            PE_HIP(e, launch_mine_gather(g, nullptr));
            PE_HIP(e, hipStreamSynchronize(nullptr));
            if ((rc = trainer_said(e, trainer, train_append_device(trainer, who, source, g.out, k, target)))) return rc;
        }
    }
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_miner_create(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_rec,
                    int32_t chunk_size, int32_t buffer_samples, int32_t carry_audio, pe_miner** out) {
    const char* who = "pe_miner_create";
    if (!e) return fail(e, PE_ERR_INVALID, "null engine handed to %s", who);
    if (!out) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    *out = nullptr;
    if (e && mel_rows(e)) return fail(e, PE_ERR_UNSUPPORTED, "%s: this session has no Vectorizer.mels form (its windows are MFCC rows); create it over an mfccs engine", who);
    if (n_rec < 0) return fail(e, PE_ERR_INVALID, "%s: n_rec=%d", who, n_rec);
    if (n_rec > 0 && !offsets_host) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    if (sample_format != 0 && sample_format != 1) return fail(e, PE_ERR_INVALID, "%s: sample_format must be 0 (float64) or 1 (float32), got %d", who, sample_format);
    if (chunk_size < 1) return fail(e, PE_ERR_INVALID, "%s: chunk_size must be >= 1, got %d", who, chunk_size);
    if (buffer_samples < 1) return fail(e, PE_ERR_INVALID, "%s: buffer_samples must be >= 1, got %d", who, buffer_samples);
    if (n_rec > 0 && offsets_host[0] != 0) return fail(e, PE_ERR_INVALID, "%s: offsets[0] must be 0, got %lld", who, (long long)offsets_host[0]);
    std::vector<int64_t> tab((size_t)3 * (n_rec + 1), 0);       // chunk prefix | frame base | first sample
    int64_t* cp = tab.data(); int64_t* fb = cp + n_rec + 1; int64_t* rs = fb + n_rec + 1;
    for (int32_t r = 0; r < n_rec; ++r) {
        const int64_t len = offsets_host[r + 1] - offsets_host[r];
        if (len < 0) return fail(e, PE_ERR_INVALID, "%s: offsets decrease at recording %d (%lld after %lld)", who, r, (long long)offsets_host[r + 1], (long long)offsets_host[r]);
        cp[r + 1] = cp[r] + (len > 0 ? (len - 1) / chunk_size : 0);        // util.py:30-32
        fb[r + 1] = fb[r] + frames_of_buffer(e->prm, len);
        rs[r] = offsets_host[r];
        if (cp[r + 1] > 0x7fffffff || fb[r + 1] > 0x7fffffff)
            return fail(e, PE_ERR_INVALID, "%s: more than 2^31 - 1 chunks or frames in one session (at recording %d)", who, r);
    }
    const int64_t n_samples = n_rec > 0 ? offsets_host[n_rec] : 0;
    rs[n_rec] = n_samples;
    if (n_samples > 0 && !audio_host) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    pe_miner* m = new pe_miner;
    m->e = e; m->n_rec = n_rec; m->chunk = chunk_size; m->buffer_samples = buffer_samples; m->carry_audio = carry_audio ? 1 : 0;
    m->audio_f32 = sample_format == 1 ? 1 : 0;
    m->total_chunks = cp[n_rec]; m->total_frames = fb[n_rec];
    m->chunk_prefix.assign(cp, cp + n_rec + 1);
    const size_t elem = sample_format == 1 ? sizeof(float) : sizeof(double);
    int rc = PE_OK;
    hipError_t herr = hipSuccess;
    do {
        if ((rc = ensure(e, m->buf[kMineAudio], (size_t)std::max<int64_t>(n_samples, 1) * elem))) break;
        if ((rc = ensure(e, m->buf[kMineTables], tab.size() * sizeof(int64_t)))) break;
        if ((rc = ensure(e, m->buf[kMineRows], (size_t)std::max<int64_t>(m->total_frames, 1) * e->row_floats * sizeof(float)))) break;
        if (n_samples > 0 && (herr = hipMemcpy(m->buf[kMineAudio].p, audio_host, (size_t)n_samples * elem, hipMemcpyHostToDevice)) != hipSuccess) break;
        if ((herr = hipMemcpy(m->buf[kMineTables].p, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess) break;
        if (m->total_frames > 0) {
            // every frame of every recording, once: pe_evaluate_clips' front-end launch with the rows back to back
            std::vector<RecDesc> desc((size_t)n_rec);
            std::vector<uint32_t> prefix((size_t)n_rec + 1);
            for (int32_t r = 0; r < n_rec; ++r) { desc[(size_t)r] = RecDesc{rs[r], fb[r]}; prefix[(size_t)r] = (uint32_t)fb[r]; }
            prefix[(size_t)n_rec] = (uint32_t)fb[n_rec];
            RecTable rt;
            herr = upload_task_table(e, m->buf[kMineClips], desc, prefix, m->buf[kMineAudio].p, m->audio_f32, rt, rc);
            if (rc || herr != hipSuccess) break;
            if ((rc = launch_rec_front_end(e, rt, static_cast<float*>(m->buf[kMineRows].p)))) break;
        }
        herr = hipStreamSynchronize(nullptr);
    } while (false);
    if (!rc && herr != hipSuccess) rc = fail(e, PE_ERR_HIP, "%s: %s", who, hipGetErrorString(herr));
    if (rc) { miner_free(m); return rc; }
    *out = m;
    return PE_OK;
}

int pe_miner_destroy(pe_miner* m) {
    if (m) miner_free(m);
    return PE_OK;
}

int pe_miner_layout(const pe_miner* m, int64_t* chunk_offsets_out) {
    if (!m || !chunk_offsets_out) return PE_ERR_INVALID;
    std::copy(m->chunk_prefix.begin(), m->chunk_prefix.end(), chunk_offsets_out);
    return PE_OK;
}

int pe_miner_scan(pe_miner* m, int32_t model, int64_t first_chunk, double threshold, float* scores_out, int32_t* hits_out,
                  int32_t capacity, int32_t* n_hits, int64_t* n_above) {
    const char* who = "pe_miner_scan";
    if (!m) return PE_ERR_INVALID;
    pe_engine* e = m->e;
    if (!n_hits || !n_above) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    if (model < 0 || model >= e->n_models) return fail(e, PE_ERR_INVALID, "%s: model %d outside 0..%d", who, model, e->n_models - 1);
    if (first_chunk < 0 || first_chunk > m->total_chunks) return fail(e, PE_ERR_INVALID, "%s: first_chunk %lld outside 0..%lld", who, (long long)first_chunk, (long long)m->total_chunks);
    if (threshold != threshold) return fail(e, PE_ERR_INVALID, "%s: threshold is NaN", who);
    if (capacity < 0 || (capacity > 0 && !hits_out)) return fail(e, PE_ERR_INVALID, "%s: capacity=%d without hits_out", who, capacity);
    *n_hits = 0; *n_above = 0;
    const int64_t n = m->total_chunks - first_chunk;
    if (n == 0) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const int T = e->prm.n_features, width = window_floats(e);
    const int64_t window_bytes = (int64_t)T * width * (int64_t)sizeof(float);
    const int64_t per_pass = std::max<int64_t>(1, std::min<int64_t>(e->clip_pass_bytes / window_bytes, 1 << 24));
    int rc;
    if ((rc = ensure(e, m->buf[kMineScores], (size_t)n * sizeof(float)))) return rc;
    float* const scores = static_cast<float*>(m->buf[kMineScores].p);
    MineGatherArgs g = miner_gather_args(m);
    g.rows = static_cast<const float*>(m->buf[kMineRows].p);
    g.chunk_prefix = m->d_chunk_prefix(); g.frame_base = m->d_frame_base(); g.n_rec = m->n_rec;
    for (int64_t c0 = 0; c0 < n; c0 += per_pass) {
        const int k = (int)std::min<int64_t>(per_pass, n - c0);
        if ((rc = ensure(e, m->buf[kMineBatch], (size_t)k * (size_t)window_bytes))) return rc;
        g.first = first_chunk + c0; g.n = k; g.out = static_cast<float*>(m->buf[kMineBatch].p);
        PE_HIP(e, launch_mine_gather(g, nullptr));
        if (e->n_models == 1) {
            if ((rc = pe_predict_device(e, g.out, k, scores + c0, nullptr))) return rc;
        } else {                // a K-model engine predicts all of its models: [K][k]; the scan keeps block `model`
            if ((rc = ensure(e, m->buf[kMinePred], (size_t)e->n_models * k * sizeof(float)))) return rc;
            if ((rc = pe_predict_device(e, g.out, k, static_cast<float*>(m->buf[kMinePred].p), nullptr))) return rc;
            PE_HIP(e, hipMemcpyAsync(scores + c0, static_cast<const float*>(m->buf[kMinePred].p) + (size_t)model * k, (size_t)k * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        }
    }
    // decode (pe_decode's kernel, when model has a table), then the ordered compaction over the whole range
    const DecState& d = e->dec[(size_t)model];
    const double* conf = nullptr;
    if (d.cd) {
        if ((rc = ensure(e, m->buf[kMineConf], (size_t)n * sizeof(double)))) return rc;
        DecodeArgs a{};
        a.n_streams = (int)n; a.raw = scores; a.cd = d.cd; a.cd_len = d.cd_len; a.min_out = d.min_out; a.out_range = d.out_range; a.center = d.center;
        a.conf_out = static_cast<double*>(m->buf[kMineConf].p);
        PE_HIP(e, launch_decode(a, nullptr));
        conf = a.conf_out;
    }
    const int n_blocks = mine_blocks(n);
    if ((rc = ensure(e, m->buf[kMineCounts], ((size_t)n_blocks + 1) * sizeof(uint32_t)))) return rc;
    if (capacity > 0 && (rc = ensure(e, m->buf[kMineHits], (size_t)capacity * sizeof(int32_t)))) return rc;
    MineCompactArgs c{scores, conf, n, threshold, first_chunk, static_cast<uint32_t*>(m->buf[kMineCounts].p), n_blocks,
                      capacity > 0 ? static_cast<int32_t*>(m->buf[kMineHits].p) : nullptr, capacity};
    PE_HIP(e, launch_mine_compact(c, nullptr));
    uint32_t total = 0;
    PE_HIP(e, hipMemcpy(&total, c.block_counts + n_blocks, sizeof total, hipMemcpyDeviceToHost));
    const int32_t got = (int32_t)std::min<int64_t>(total, capacity);
    if (got > 0) PE_HIP(e, hipMemcpy(hits_out, m->buf[kMineHits].p, (size_t)got * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (scores_out) PE_HIP(e, hipMemcpy(scores_out, scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    *n_hits = got; *n_above = (int64_t)total;
    return PE_OK;
}

int pe_miner_vectorize(pe_miner* m, const int32_t* hits, int32_t n, double* feats_out_host) {
    if (!m) return PE_ERR_INVALID;
    if (n > 0 && !feats_out_host) return fail(m->e, PE_ERR_INVALID, "null argument to pe_miner_vectorize");
    return miner_rows(m, "pe_miner_vectorize", hits, n, feats_out_host, nullptr, 0, 0.0f);
}

int pe_miner_append(pe_miner* m, pe_trainer* trainer, int32_t source, const int32_t* hits, int32_t n, float target) {
    const char* who = "pe_miner_append";
    if (!m) return PE_ERR_INVALID;
    pe_engine* e = m->e;
    int rc = check_append(e, who, trainer, source);
    if (rc) return rc;
    if (!(target >= 0.0f && target <= 1.0f)) return fail(e, PE_ERR_INVALID, "%s: target %g is outside [0, 1]", who, (double)target);
    return miner_rows(m, who, hits, n, nullptr, trainer, source, target);
}

}  // extern "C"

// ---- generating training audio (pe_generator; kernel: generate_device.h) --------------------------------------
namespace {
enum GeneratorBuf {
    // resident: the two pools as given; of the plan: chunk prefix | frame base, the segments, their prefix sum, every frame's row
    kGenBg, kGenClips, kGenTables, kGenSegs, kGenSegPrefix, kGenRows,
    // grown on demand: a pass's mixed samples and recording table; a pass's ids, targets and network input; pe_generator_audio's samples
    kGenMixed, kGenRecs, kGenIds, kGenTargets, kGenBatch, kGenAudioOut, kGenBufCount
};
}  // namespace

struct pe_generator {
    pe_engine* e = nullptr;
    int n_bg = 0, n_clips = 0, chunk = 0;
    std::vector<int64_t> bg_offsets, clip_offsets;      // [n_bg + 1], [n_clips + 1]
    // the plan: per file its chunk / frame / sample prefix sums [n_files + 1] and its segment range; per segment its start
    int n_files = 0;
    int64_t n_segments = 0, total_chunks = 0, total_frames = 0;
    std::vector<int64_t> chunk_prefix, frame_base, sample_base, seg_first;
    DeviceBuf buf[kGenBufCount];                        // GeneratorBuf
    const long long* d_chunk_prefix() const { return static_cast<const long long*>(buf[kGenTables].p); }
    const long long* d_frame_base() const { return d_chunk_prefix() + n_files + 1; }
};

namespace {

void generator_free(pe_generator* g) { release_buffers(g->e, g->buf, kGenBufCount); delete g; }

GenMixArgs generator_mix_args(const pe_generator* g) {
    GenMixArgs a{};
    a.bg = static_cast<const float*>(g->buf[kGenBg].p); a.clips = static_cast<const float*>(g->buf[kGenClips].p);
    a.segs = static_cast<const GenSeg*>(g->buf[kGenSegs].p); a.seg_prefix = static_cast<const long long*>(g->buf[kGenSegPrefix].p);
    a.keep = (float)(1.0 - 0.6);                                // train_generated.py:155,185
    return a;
}

void generator_drop_plan(pe_generator* g) {
    g->n_files = 0; g->n_segments = 0; g->total_chunks = 0; g->total_frames = 0;
    g->chunk_prefix.assign(1, 0); g->frame_base.assign(1, 0); g->sample_base.assign(1, 0); g->seg_first.assign(1, 0);
}

// the windows after chunks ids[0 .. n) in passes: the ids (and targets) go up, mine_gather packs the rows, which go to the
// host or behind the trainer's set
int generator_rows(pe_generator* g, const char* who, const int32_t* ids, const float* targets, int32_t n, float* feats_out_host, pe_trainer* trainer, int source) {
    pe_engine* e = g->e;
    if (n < 0) return fail(e, PE_ERR_INVALID, "%s: n=%d", who, n);
    if (n > 0 && !ids) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    for (int32_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= g->total_chunks)
            return fail(e, PE_ERR_INVALID, "%s: ids[%d] = %d is outside the plan's %lld chunks", who, i, ids[i], (long long)g->total_chunks);
    if (n == 0) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const int T = e->prm.n_features, width = window_floats(e);
    const int64_t window_bytes = (int64_t)T * width * (int64_t)sizeof(float);
    const int64_t per_pass = std::max<int64_t>(1, std::min<int64_t>(e->clip_pass_bytes / window_bytes, 1 << 24));
    MineGatherArgs a = gather_geometry(e);
    a.chunk = g->chunk; a.emit_window = emit_window(e->prm); a.hop = e->prm.hop_samples;
    a.rows = static_cast<const float*>(g->buf[kGenRows].p);
    a.chunk_prefix = g->d_chunk_prefix(); a.frame_base = g->d_frame_base(); a.n_rec = g->n_files;
    int rc;
    for (int32_t i0 = 0; i0 < n; i0 += (int32_t)per_pass) {
        const int k = (int)std::min<int64_t>(per_pass, n - i0);
        if ((rc = ensure(e, g->buf[kGenIds], (size_t)k * sizeof(int32_t)))) return rc;
        if ((rc = ensure(e, g->buf[kGenBatch], (size_t)k * (size_t)window_bytes))) return rc;
        PE_HIP(e, hipMemcpy(g->buf[kGenIds].p, ids + i0, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice));
        a.ids = static_cast<const int32_t*>(g->buf[kGenIds].p); a.n = k; a.out = static_cast<float*>(g->buf[kGenBatch].p);
        PE_HIP(e, launch_mine_gather(a, nullptr));
        if (feats_out_host) {
            PE_HIP(e, hipMemcpy(feats_out_host + (size_t)i0 * T * width, g->buf[kGenBatch].p, (size_t)k * (size_t)window_bytes, hipMemcpyDeviceToHost));
        } else if ((rc = rows_to_trainer(e, who, trainer, source, a.out, targets + i0, k, g->buf[kGenTargets]))) return rc;
    }
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_generator_create(pe_engine* e, const float* bg_audio, const int64_t* bg_offsets, int32_t n_bg, const float* clip_audio,
                        const int64_t* clip_offsets, int32_t n_clips, int32_t chunk_size, pe_generator** out) {
    const char* who = "pe_generator_create";
    if (!e) return fail(e, PE_ERR_INVALID, "null engine handed to %s", who);
    if (!out) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    *out = nullptr;
    if (e && mel_rows(e)) return fail(e, PE_ERR_UNSUPPORTED, "%s: this session has no Vectorizer.mels form (its windows are MFCC rows); create it over an mfccs engine", who);
    if (chunk_size < 1) return fail(e, PE_ERR_INVALID, "%s: chunk_size must be >= 1, got %d", who, chunk_size);
    int rc;
    if ((rc = check_offsets(e, who, "background", bg_offsets, n_bg, false))) return rc;
    if ((rc = check_offsets(e, who, "clip", clip_offsets, n_clips, false))) return rc;
    const int64_t bg_samples = n_bg > 0 ? bg_offsets[n_bg] : 0, clip_samples = n_clips > 0 ? clip_offsets[n_clips] : 0;
    if ((bg_samples > 0 && !bg_audio) || (clip_samples > 0 && !clip_audio)) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    pe_generator* g = new pe_generator;
    g->e = e; g->n_bg = n_bg; g->n_clips = n_clips; g->chunk = chunk_size;
    g->bg_offsets.assign(1, 0); g->clip_offsets.assign(1, 0);
    if (n_bg > 0) g->bg_offsets.assign(bg_offsets, bg_offsets + n_bg + 1);
    if (n_clips > 0) g->clip_offsets.assign(clip_offsets, clip_offsets + n_clips + 1);
    generator_drop_plan(g);
    hipError_t herr = hipSuccess;
    do {
        if ((rc = ensure(e, g->buf[kGenBg], (size_t)std::max<int64_t>(bg_samples, 1) * sizeof(float)))) break;
        if ((rc = ensure(e, g->buf[kGenClips], (size_t)std::max<int64_t>(clip_samples, 1) * sizeof(float)))) break;
        if (bg_samples > 0 && (herr = hipMemcpy(g->buf[kGenBg].p, bg_audio, (size_t)bg_samples * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
        if (clip_samples > 0 && (herr = hipMemcpy(g->buf[kGenClips].p, clip_audio, (size_t)clip_samples * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
    } while (false);
    if (!rc && herr != hipSuccess) rc = fail(e, PE_ERR_HIP, "%s: %s", who, hipGetErrorString(herr));
    if (rc) { generator_free(g); return rc; }
    *out = g;
    return PE_OK;
}

int pe_generator_destroy(pe_generator* g) {
    if (g) generator_free(g);
    return PE_OK;
}

int pe_generator_set_plan(pe_generator* g, const pe_gen_file* files, int32_t n_files, const pe_gen_segment* segments, int64_t n_segments) {
    const char* who = "pe_generator_set_plan";
    if (!g) return PE_ERR_INVALID;
    pe_engine* e = g->e;
    if (n_files < 0 || n_segments < 0 || n_segments > 0x7fffffff) return fail(e, PE_ERR_INVALID, "%s: %d files, %lld segments", who, n_files, (long long)n_segments);
    if ((n_files > 0 && !files) || (n_segments > 0 && !segments)) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    // everything is checked on the host before any device work; the resident plan stays as it is when a check fails
    const int64_t C = g->chunk;
    std::vector<int64_t> cp((size_t)n_files + 1, 0), fb((size_t)n_files + 1, 0), sb((size_t)n_files + 1, 0), sf((size_t)n_files + 1, 0);
    std::vector<GenSeg> segs((size_t)n_segments);
    std::vector<int64_t> prefix((size_t)n_segments + 1, 0);
    int64_t next_segment = 0;
    for (int32_t f = 0; f < n_files; ++f) {
        const pe_gen_file& pf = files[f];
        if (pf.background < 0 || pf.background >= g->n_bg) return fail(e, PE_ERR_INVALID, "%s: file %d names background %d of %d", who, f, pf.background, g->n_bg);
        if (pf.first_segment != next_segment || pf.n_segments < 0 || pf.n_segments > n_segments - next_segment)
            return fail(e, PE_ERR_INVALID, "%s: file %d takes segments %lld + %lld, expected them to start at %lld of %lld", who, f,
                        (long long)pf.first_segment, (long long)pf.n_segments, (long long)next_segment, (long long)n_segments);
        const int64_t bg0 = g->bg_offsets[(size_t)pf.background], len = g->bg_offsets[(size_t)pf.background + 1] - bg0;
        const int64_t chunks = len > 0 ? (len - 1) / C : 0;                    // util.py:30-32
        const float volume = (float)pf.audio_volume, rms_bg = (float)pf.rms;
        if (chunks > 0 && !(pf.rms > 0.0 && pf.audio_volume == pf.audio_volume))
            return fail(e, PE_ERR_INVALID, "%s: file %d has rms %g, audio_volume %g", who, f, pf.rms, pf.audio_volume);
        int64_t filled = 0;
        for (int64_t s = next_segment; s < next_segment + pf.n_segments; ++s) {
            const pe_gen_segment& ps = segments[s];
            if (ps.length < 1) return fail(e, PE_ERR_INVALID, "%s: segment %lld has length %lld", who, (long long)s, (long long)ps.length);
            if (ps.clip < -1 || ps.clip >= g->n_clips) return fail(e, PE_ERR_INVALID, "%s: segment %lld names clip %d of %d", who, (long long)s, ps.clip, g->n_clips);
            if (ps.length > chunks * C - filled)
                return fail(e, PE_ERR_INVALID, "%s: the segments of file %d overrun its %lld chunks of %lld samples at segment %lld", who, f, (long long)chunks, (long long)C, (long long)s);
            GenSeg d{-1, bg0 + filled, volume, rms_bg, 1.0f, 0.0f};
            if (ps.clip >= 0) {
                const int64_t c0 = g->clip_offsets[(size_t)ps.clip], clen = g->clip_offsets[(size_t)ps.clip + 1] - c0;
                if (ps.first < 0 || ps.first > clen || ps.length > clen - ps.first)
                    return fail(e, PE_ERR_INVALID, "%s: segment %lld takes samples %lld + %lld of clip %d, which has %lld", who, (long long)s,
                                (long long)ps.first, (long long)ps.length, ps.clip, (long long)clen);
                if (!(ps.rms > 0.0)) return fail(e, PE_ERR_INVALID, "%s: segment %lld (clip %d) has rms %g", who, (long long)s, ps.clip, ps.rms);
                d.clip = c0 + ps.first; d.rms_clip = (float)ps.rms;
            }
            segs[(size_t)s] = d;
            prefix[(size_t)s + 1] = prefix[(size_t)s] + ps.length;
            filled += ps.length;
        }
        if (filled != chunks * C)
            return fail(e, PE_ERR_INVALID, "%s: the segments of file %d hold %lld samples, its %lld chunks of %lld need %lld", who, f,
                        (long long)filled, (long long)chunks, (long long)C, (long long)(chunks * C));
        next_segment += pf.n_segments;
        sf[(size_t)f + 1] = next_segment;
        cp[(size_t)f + 1] = cp[(size_t)f] + chunks;
        fb[(size_t)f + 1] = fb[(size_t)f] + frames_of_buffer(e->prm, chunks * C);
        sb[(size_t)f + 1] = sb[(size_t)f] + chunks * C;
        if (cp[(size_t)f + 1] > 0x7fffffff || fb[(size_t)f + 1] > 0x7fffffff)
            return fail(e, PE_ERR_INVALID, "%s: more than 2^31 - 1 chunks or frames in one plan (at file %d)", who, f);
    }
    if (next_segment != n_segments) return fail(e, PE_ERR_INVALID, "%s: the files take %lld of %lld segments", who, (long long)next_segment, (long long)n_segments);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    generator_drop_plan(g);                     // from here on the old plan is gone, whatever happens
    int rc;
    std::vector<int64_t> tab(cp);
    tab.insert(tab.end(), fb.begin(), fb.end());
    if ((rc = ensure(e, g->buf[kGenTables], tab.size() * sizeof(int64_t)))) return rc;
    if ((rc = ensure(e, g->buf[kGenSegs], std::max<size_t>(segs.size(), 1) * sizeof(GenSeg)))) return rc;
    if ((rc = ensure(e, g->buf[kGenSegPrefix], prefix.size() * sizeof(int64_t)))) return rc;
    if ((rc = ensure(e, g->buf[kGenRows], (size_t)std::max<int64_t>(fb[(size_t)n_files], 1) * e->row_floats * sizeof(float)))) return rc;
    PE_HIP(e, hipMemcpy(g->buf[kGenTables].p, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (!segs.empty()) PE_HIP(e, hipMemcpy(g->buf[kGenSegs].p, segs.data(), segs.size() * sizeof(GenSeg), hipMemcpyHostToDevice));
    PE_HIP(e, hipMemcpy(g->buf[kGenSegPrefix].p, prefix.data(), prefix.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    // passes over whole files: mix, then every frame of the pass's files once (pe_evaluate_clips' front-end launch, rows back to back)
    std::vector<RecDesc> desc;
    std::vector<uint32_t> rprefix;
    for (int32_t f0 = 0; f0 < n_files;) {
        int32_t f1 = f0 + 1;
        while (f1 < n_files && (sb[(size_t)f1 + 1] - sb[(size_t)f0]) * (int64_t)sizeof(double) <= e->clip_pass_bytes) ++f1;
        const int64_t n_samples = sb[(size_t)f1] - sb[(size_t)f0], n_frames = fb[(size_t)f1] - fb[(size_t)f0];
        if (n_samples > 0) {
            if ((rc = ensure(e, g->buf[kGenMixed], (size_t)n_samples * sizeof(double)))) return rc;
            GenMixArgs a = generator_mix_args(g);
            a.seg_lo = (int)sf[(size_t)f0]; a.seg_hi = (int)sf[(size_t)f1];
            a.first = sb[(size_t)f0]; a.n = n_samples; a.out = static_cast<double*>(g->buf[kGenMixed].p);
            PE_HIP(e, launch_gen_mix(a, nullptr));
        }
        if (n_frames > 0) {
            const int n = f1 - f0;
            desc.resize((size_t)n); rprefix.resize((size_t)n + 1);
            for (int i = 0; i < n; ++i) {
                desc[(size_t)i] = RecDesc{sb[(size_t)f0 + i] - sb[(size_t)f0], fb[(size_t)f0 + i]};
                rprefix[(size_t)i] = (uint32_t)(fb[(size_t)f0 + i] - fb[(size_t)f0]);
            }
            rprefix[(size_t)n] = (uint32_t)n_frames;
            RecTable rt;
            PE_HIP(e, upload_task_table(e, g->buf[kGenRecs], desc, rprefix, g->buf[kGenMixed].p, 0, rt, rc));
            if (rc) return rc;
            if ((rc = launch_rec_front_end(e, rt, static_cast<float*>(g->buf[kGenRows].p)))) return rc;
        }
        PE_HIP(e, hipStreamSynchronize(nullptr));               // the next pass reuses the mixed samples and the table
        f0 = f1;
    }
    g->n_files = n_files; g->n_segments = n_segments;
    g->total_chunks = cp[(size_t)n_files]; g->total_frames = fb[(size_t)n_files];
    g->chunk_prefix.swap(cp); g->frame_base.swap(fb); g->sample_base.swap(sb); g->seg_first.swap(sf);
    return PE_OK;
}

int pe_generator_audio(pe_generator* g, int32_t file, int64_t first, int64_t n, double* out_host) {
    const char* who = "pe_generator_audio";
    if (!g) return PE_ERR_INVALID;
    pe_engine* e = g->e;
    if (file < 0 || file >= g->n_files) return fail(e, PE_ERR_INVALID, "%s: file %d is outside the plan's %d files", who, file, g->n_files);
    const int64_t len = g->sample_base[(size_t)file + 1] - g->sample_base[(size_t)file];
    if (first < 0 || n < 0 || first > len || n > len - first)
        return fail(e, PE_ERR_INVALID, "%s: samples %lld + %lld are outside file %d, which has %lld", who, (long long)first, (long long)n, file, (long long)len);
    if (n == 0) return PE_OK;
    if (!out_host) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    int rc;
    if ((rc = ensure(e, g->buf[kGenAudioOut], (size_t)n * sizeof(double)))) return rc;
    GenMixArgs a = generator_mix_args(g);
    a.seg_lo = (int)g->seg_first[(size_t)file]; a.seg_hi = (int)g->seg_first[(size_t)file + 1];
    a.first = g->sample_base[(size_t)file] + first; a.n = n; a.out = static_cast<double*>(g->buf[kGenAudioOut].p);
    PE_HIP(e, launch_gen_mix(a, nullptr));
    PE_HIP(e, hipMemcpy(out_host, g->buf[kGenAudioOut].p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_generator_vectorize(pe_generator* g, const int32_t* ids, int32_t n, float* feats_out_host) {
    if (!g) return PE_ERR_INVALID;
    if (n > 0 && !feats_out_host) return fail(g->e, PE_ERR_INVALID, "null argument to pe_generator_vectorize");
    return generator_rows(g, "pe_generator_vectorize", ids, nullptr, n, feats_out_host, nullptr, 0);
}

int pe_generator_append(pe_generator* g, pe_trainer* trainer, int32_t source, const int32_t* ids, const float* targets, int32_t n) {
    const char* who = "pe_generator_append";
    if (!g) return PE_ERR_INVALID;
    pe_engine* e = g->e;
    if (n > 0 && !targets) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    int rc;
    if ((rc = check_append(e, who, trainer, source)) || (rc = check_targets(e, who, targets, n))) return rc;
    return generator_rows(g, who, ids, targets, n, nullptr, trainer, source);
}

}  // extern "C"

// ---- noise augmentation (pe_augmenter; kernels: augment_device.h) ---------------------------------------------
namespace {
enum AugmenterBuf {
    // resident: the two pools as given
    kAugClips, kAugNoise,
    // grown on demand: the chains' tables and sums; of a pass: its copies, pieces and piece prefix, the reloaded samples, the clip
    // table, the front end's rows, the trainer's rows and targets; pe_augmenter_audio's samples; the plan's overflow counts
    kAugTables, kAugSums, kAugSlots, kAugPassPieces, kAugReloaded, kAugDesc, kAugRows, kAugPacked, kAugTargets, kAugMixed, kAugPcm, kAugOverflow, kAugBufCount
};
}  // namespace

struct pe_augmenter {
    pe_engine* e = nullptr;                             // null: a session that checks plans only
    int n_clips = 0, n_noise = 0;
    std::vector<int64_t> clip_offsets, noise_offsets;   // [n_clips + 1], [n_noise + 1]
    std::vector<double> clip_volume;                    // [n_clips] va = sqrt((double) S_a)
    // the plan, as given, and vn = sqrt(S_n) of every copy
    std::vector<pe_aug_copy> copies;
    std::vector<pe_aug_piece> pieces;
    std::vector<double> noise_volume;
    DeviceBuf buf[kAugBufCount];                        // AugmenterBuf
    int64_t copy_length(int32_t o) const { const int32_t c = copies[(size_t)o].clip; return clip_offsets[(size_t)c + 1] - clip_offsets[(size_t)c]; }
};

namespace {

void augmenter_free(pe_augmenter* g) { if (g->e) release_buffers(g->e, g->buf, kAugBufCount); delete g; }

// Copies ids[0 .. k) as one pass: their slots, pieces and piece prefix go up, aug_mix writes what the caller asks for.
// slot_begin[k + 1]: where every copy starts among the pass's samples.
int augmenter_mix(pe_augmenter* g, const int32_t* ids, int k, std::vector<int64_t>& slot_begin, float* reloaded, double* mixed, int16_t* pcm,
                  unsigned long long* overflowed) {
    pe_engine* e = g->e;
    std::vector<AugSlot> slots((size_t)k);
    std::vector<AugPiece> pieces;
    std::vector<int64_t> prefix(1, 0);
    slot_begin.assign((size_t)k + 1, 0);
    for (int i = 0; i < k; ++i) {
        const pe_aug_copy& c = g->copies[(size_t)ids[i]];
        slots[(size_t)i] = AugSlot{g->clip_volume[(size_t)c.clip], g->noise_volume[(size_t)ids[i]], c.ratio, (float)(1.0 - c.ratio), ids[i]};
        int64_t at = g->clip_offsets[(size_t)c.clip];
        for (int64_t q = c.first_piece; q < c.first_piece + c.n_pieces; ++q) {
            const pe_aug_piece& p = g->pieces[(size_t)q];
            pieces.push_back(AugPiece{g->noise_offsets[(size_t)p.noise] + p.first, at, i, 0});
            prefix.push_back(prefix.back() + p.length);
            at += p.length;
        }
        slot_begin[(size_t)i + 1] = prefix.back();
    }
    if (pieces.size() > 0x7fffffffu) return fail(e, PE_ERR_INVALID, "pe_augmenter: a pass of %d copies holds more than 2^31 - 1 pieces", k);
    int rc;
    const size_t pb = pieces.size() * sizeof(AugPiece), xb = prefix.size() * sizeof(int64_t);
    if ((rc = ensure(e, g->buf[kAugSlots], slots.size() * sizeof(AugSlot)))) return rc;
    if ((rc = ensure(e, g->buf[kAugPassPieces], pb + xb))) return rc;
    PE_HIP(e, hipMemcpy(g->buf[kAugSlots].p, slots.data(), slots.size() * sizeof(AugSlot), hipMemcpyHostToDevice));
    PE_HIP(e, hipMemcpy(g->buf[kAugPassPieces].p, pieces.data(), pb, hipMemcpyHostToDevice));
    PE_HIP(e, hipMemcpy(static_cast<char*>(g->buf[kAugPassPieces].p) + pb, prefix.data(), xb, hipMemcpyHostToDevice));
    AugMixArgs a{};
    a.clips = static_cast<const float*>(g->buf[kAugClips].p); a.noise = static_cast<const float*>(g->buf[kAugNoise].p);
    a.slots = static_cast<const AugSlot*>(g->buf[kAugSlots].p); a.pieces = static_cast<const AugPiece*>(g->buf[kAugPassPieces].p);
    a.prefix = reinterpret_cast<const long long*>(static_cast<const char*>(g->buf[kAugPassPieces].p) + pb);
    a.n_pieces = (int)pieces.size(); a.n = prefix.back();
    a.reloaded = reloaded; a.mixed = mixed; a.pcm = pcm; a.overflowed = overflowed;
    PE_HIP(e, launch_aug_mix(a, nullptr));
    return PE_OK;
}

// the copies of the pass that starts at ids[i0]: at least one, then as many as stay within the byte target (and the bounds
// that keep a pass's tables and row buffers small)
int32_t augmenter_pass_end(const pe_augmenter* g, const int32_t* ids, int32_t i0, int32_t n) {
    const int64_t T = g->e->prm.n_features;
    int64_t samples = g->copy_length(ids[i0]), pieces = g->copies[(size_t)ids[i0]].n_pieces;
    int32_t i1 = i0 + 1;
    while (i1 < n) {
        const int64_t len = g->copy_length(ids[i1]), np = g->copies[(size_t)ids[i1]].n_pieces;
        if ((samples + len) * (int64_t)sizeof(float) > g->e->clip_pass_bytes || (int64_t)(i1 + 1 - i0) * T > kClipPassRows || pieces + np > (1ll << 26)) break;
        samples += len; pieces += np; ++i1;
    }
    return i1;
}

int augmenter_check_ids(pe_augmenter* g, const char* who, const int32_t* ids, int32_t n) {
    pe_engine* e = g->e;
    if (!e) return fail(e, PE_ERR_INVALID, "%s: the session was created without an engine: it checks plans only", who);
    if (n < 0) return fail(e, PE_ERR_INVALID, "%s: n=%d", who, n);
    if (n > 0 && !ids) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    for (int32_t i = 0; i < n; ++i)
        if (ids[i] < 0 || (size_t)ids[i] >= g->copies.size())
            return fail(e, PE_ERR_INVALID, "%s: ids[%d] = %d is outside the plan's %zu copies", who, i, ids[i], g->copies.size());
    return PE_OK;
}

// vectorize() of the reloaded copies ids[0 .. n) in passes: aug_mix writes the float32 clips, the clip front end their windows,
// mine_gather packs them for the trainer; the rows go to the host or behind the trainer's set
int augmenter_rows(pe_augmenter* g, const char* who, const int32_t* ids, const float* targets, int32_t n, int64_t max_samples, float* feats_out_host,
                   pe_trainer* trainer, int source) {
    pe_engine* e = g->e;
    int rc = augmenter_check_ids(g, who, ids, n);
    if (rc) return rc;
    if (n == 0) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const int T = e->prm.n_features, width = window_floats(e);
    std::vector<int64_t> begin;
    std::vector<ClipDesc> desc;
    std::vector<uint32_t> prefix;
    for (int32_t i0 = 0; i0 < n;) {
        const int32_t i1 = augmenter_pass_end(g, ids, i0, n);
        const int k = i1 - i0;
        int64_t n_samples = 0;
        for (int32_t i = i0; i < i1; ++i) n_samples += g->copy_length(ids[i]);
        if ((rc = ensure(e, g->buf[kAugReloaded], (size_t)n_samples * sizeof(float)))) return rc;
        if ((rc = augmenter_mix(g, ids + i0, k, begin, static_cast<float*>(g->buf[kAugReloaded].p), nullptr, nullptr, nullptr))) return rc;
        desc.resize((size_t)k); prefix.resize((size_t)k + 1);
        uint32_t tasks = 0;
        for (int i = 0; i < k; ++i) {
            prefix[(size_t)i] = tasks;
            desc[(size_t)i] = clip_desc(e->prm, T, begin[(size_t)i + 1], begin[(size_t)i + 1] - begin[(size_t)i], max_samples, tasks);
        }
        prefix[(size_t)k] = tasks;
        if ((rc = ensure(e, g->buf[kAugRows], (size_t)k * T * e->row_floats * sizeof(float)))) return rc;
        if ((rc = ensure(e, g->buf[kAugPacked], (size_t)k * T * width * sizeof(float)))) return rc;
        ClipTable ct;
        PE_HIP(e, upload_task_table(e, g->buf[kAugDesc], desc, prefix, g->buf[kAugReloaded].p, 1, ct, rc));
        if (rc) return rc;
        if ((rc = launch_clip_front_end(e, ct, nullptr, static_cast<float*>(g->buf[kAugRows].p), nullptr))) return rc;
        MineGatherArgs a = gather_geometry(e);
        a.rows = static_cast<const float*>(g->buf[kAugRows].p); a.n = k; a.out = static_cast<float*>(g->buf[kAugPacked].p);
        PE_HIP(e, launch_mine_gather(a, nullptr));
        if (feats_out_host) {
            PE_HIP(e, hipMemcpy(feats_out_host + (size_t)i0 * T * width, g->buf[kAugPacked].p, (size_t)k * T * width * sizeof(float), hipMemcpyDeviceToHost));
        } else if ((rc = rows_to_trainer(e, who, trainer, source, a.out, targets + i0, k, g->buf[kAugTargets]))) return rc;
        PE_HIP(e, hipStreamSynchronize(nullptr));               // the next pass reuses the samples and the tables
        i0 = i1;
    }
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_augmenter_create(pe_engine* e, const float* clip_audio, const int64_t* clip_offsets, int32_t n_clips, const float* noise_audio,
                        const int64_t* noise_offsets, int32_t n_noise, pe_augmenter** out) {
    const char* who = "pe_augmenter_create";
    if (!out) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    *out = nullptr;
    if (e && mel_rows(e)) return fail(e, PE_ERR_UNSUPPORTED, "%s: this session has no Vectorizer.mels form (its windows are MFCC rows); create it over an mfccs engine", who);
    int rc;
    if ((rc = check_offsets(e, who, "clip", clip_offsets, n_clips, true))) return rc;
    if ((rc = check_offsets(e, who, "noise recording", noise_offsets, n_noise, true))) return rc;
    if (e && (!clip_audio || !noise_audio)) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    pe_augmenter* g = new pe_augmenter;
    g->e = e; g->n_clips = n_clips; g->n_noise = n_noise;
    g->clip_offsets.assign(clip_offsets, clip_offsets + n_clips + 1);
    g->noise_offsets.assign(noise_offsets, noise_offsets + n_noise + 1);
    g->clip_volume.assign((size_t)n_clips, 0.0);
    if (!e) { *out = g; return PE_OK; }
    const int64_t clip_samples = clip_offsets[n_clips], noise_samples = noise_offsets[n_noise];
    std::vector<float> sums((size_t)n_clips);
    hipError_t herr = hipSuccess;
    do {
        if ((herr = hipSetDevice(e->device)) != hipSuccess) break;
        if ((rc = drain_async(e))) break;
        if ((rc = ensure(e, g->buf[kAugClips], (size_t)clip_samples * sizeof(float)))) break;
        if ((rc = ensure(e, g->buf[kAugNoise], (size_t)noise_samples * sizeof(float)))) break;
        if ((rc = ensure(e, g->buf[kAugTables], ((size_t)n_clips + 1) * sizeof(int64_t)))) break;
        if ((rc = ensure(e, g->buf[kAugSums], (size_t)n_clips * sizeof(float)))) break;
        if ((herr = hipMemcpy(g->buf[kAugClips].p, clip_audio, (size_t)clip_samples * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
        if ((herr = hipMemcpy(g->buf[kAugNoise].p, noise_audio, (size_t)noise_samples * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
        if ((herr = hipMemcpy(g->buf[kAugTables].p, clip_offsets, ((size_t)n_clips + 1) * sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess) break;
        AugEnergyArgs a{};                                      // S_a of every clip: it does not depend on the plan
        a.pool = static_cast<const float*>(g->buf[kAugClips].p); a.offsets = static_cast<const long long*>(g->buf[kAugTables].p);
        a.n = n_clips; a.sum_f32 = static_cast<float*>(g->buf[kAugSums].p);
        if ((herr = launch_aug_energy_clips(a, nullptr)) != hipSuccess) break;
        herr = hipMemcpy(sums.data(), g->buf[kAugSums].p, (size_t)n_clips * sizeof(float), hipMemcpyDeviceToHost);
    } while (false);
    if (!rc && herr != hipSuccess) rc = fail(e, PE_ERR_HIP, "%s: %s", who, hipGetErrorString(herr));
    if (rc) { augmenter_free(g); return rc; }
    for (int32_t c = 0; c < n_clips; ++c) g->clip_volume[(size_t)c] = std::sqrt((double)sums[(size_t)c]);     // sqrt(sum(audio ** 2))
    *out = g;
    return PE_OK;
}

int pe_augmenter_destroy(pe_augmenter* g) {
    if (g) augmenter_free(g);
    return PE_OK;
}

int pe_augmenter_set_plan(pe_augmenter* g, const pe_aug_copy* copies, int32_t n_copies, const pe_aug_piece* pieces, int64_t n_pieces) {
    const char* who = "pe_augmenter_set_plan";
    if (!g) return PE_ERR_INVALID;
    pe_engine* e = g->e;
    if (n_copies < 0 || n_pieces < 0) return fail(e, PE_ERR_INVALID, "%s: %d copies, %lld pieces", who, n_copies, (long long)n_pieces);
    if (n_pieces > 0x7fffffff) return fail(e, PE_ERR_INVALID, "%s: %lld pieces are more than 2^31 - 1", who, (long long)n_pieces);
    if ((n_copies > 0 && !copies) || (n_pieces > 0 && !pieces)) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    // everything is checked on the host before any device work; the resident plan stays as it is when a check fails
    std::vector<int64_t> tab((size_t)n_copies + 1 + (size_t)n_pieces + 1 + (size_t)n_pieces, 0);     // first piece | piece prefix | piece source
    int64_t* const fp = tab.data(); int64_t* const pp = fp + n_copies + 1; int64_t* const ps = pp + n_pieces + 1;
    int64_t next_piece = 0;
    for (int32_t o = 0; o < n_copies; ++o) {
        const pe_aug_copy& c = copies[o];
        if (c.clip < 0 || c.clip >= g->n_clips) return fail(e, PE_ERR_INVALID, "%s: copy %d names clip %d of %d", who, o, c.clip, g->n_clips);
        if (c.ratio != c.ratio) return fail(e, PE_ERR_INVALID, "%s: copy %d has ratio NaN", who, o);
        if (c.first_piece != next_piece || c.n_pieces < 0 || c.n_pieces > n_pieces - next_piece)
            return fail(e, PE_ERR_INVALID, "%s: copy %d takes pieces %lld + %lld, expected them to start at %lld of %lld", who, o,
                        (long long)c.first_piece, (long long)c.n_pieces, (long long)next_piece, (long long)n_pieces);
        const int64_t len = g->clip_offsets[(size_t)c.clip + 1] - g->clip_offsets[(size_t)c.clip];
        int64_t filled = 0;
        for (int64_t q = next_piece; q < next_piece + c.n_pieces; ++q) {
            const pe_aug_piece& p = pieces[q];
            if (p.noise < 0 || p.noise >= g->n_noise) return fail(e, PE_ERR_INVALID, "%s: piece %lld names noise recording %d of %d", who, (long long)q, p.noise, g->n_noise);
            if (p.length < 1) return fail(e, PE_ERR_INVALID, "%s: piece %lld has length %lld", who, (long long)q, (long long)p.length);
            const int64_t n0 = g->noise_offsets[(size_t)p.noise], nlen = g->noise_offsets[(size_t)p.noise + 1] - n0;
            if (p.first < 0 || p.first > nlen || p.length > nlen - p.first)
                return fail(e, PE_ERR_INVALID, "%s: piece %lld takes samples %lld + %lld of noise recording %d, which has %lld", who, (long long)q,
                            (long long)p.first, (long long)p.length, p.noise, (long long)nlen);
            if (p.length > len - filled)
                return fail(e, PE_ERR_INVALID, "%s: the pieces of copy %d overrun the %lld samples of its clip %d at piece %lld", who, o, (long long)len, c.clip, (long long)q);
            ps[q] = n0 + p.first;
            pp[q + 1] = pp[q] + p.length;
            filled += p.length;
        }
        if (filled != len)
            return fail(e, PE_ERR_INVALID, "%s: the pieces of copy %d hold %lld samples, its clip %d has %lld", who, o, (long long)filled, c.clip, (long long)len);
        next_piece += c.n_pieces;
        fp[o + 1] = next_piece;
    }
    if (next_piece != n_pieces) return fail(e, PE_ERR_INVALID, "%s: the copies take %lld of %lld pieces", who, (long long)next_piece, (long long)n_pieces);
    std::vector<double> vn((size_t)n_copies, 0.0);
    if (e && n_copies > 0) {
        // S_n of every copy, and the flags of those whose noise is all zero
        PE_HIP(e, hipSetDevice(e->device));
        PE_DRAIN(e);
        int rc;
        const size_t sb = (size_t)n_copies * sizeof(double), zb = (size_t)n_copies * sizeof(int32_t);
        if ((rc = ensure(e, g->buf[kAugTables], tab.size() * sizeof(int64_t)))) return rc;
        if ((rc = ensure(e, g->buf[kAugSums], sb + zb))) return rc;
        PE_HIP(e, hipMemcpy(g->buf[kAugTables].p, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        AugEnergyArgs a{};
        a.pool = static_cast<const float*>(g->buf[kAugNoise].p);
        a.first_piece = static_cast<const long long*>(g->buf[kAugTables].p); a.piece_prefix = a.first_piece + n_copies + 1; a.piece_src = a.piece_prefix + n_pieces + 1;
        a.n = n_copies; a.sum_f64 = static_cast<double*>(g->buf[kAugSums].p);
        a.zero = reinterpret_cast<int32_t*>(static_cast<char*>(g->buf[kAugSums].p) + sb);
        PE_HIP(e, launch_aug_energy_copies(a, nullptr));
        std::vector<int32_t> zero((size_t)n_copies);
        PE_HIP(e, hipMemcpy(vn.data(), a.sum_f64, sb, hipMemcpyDeviceToHost));
        PE_HIP(e, hipMemcpy(zero.data(), a.zero, zb, hipMemcpyDeviceToHost));
        for (int32_t o = 0; o < n_copies; ++o) {
            if (zero[(size_t)o])
                return fail(e, PE_ERR_INVALID, "%s: the noise under copy %d is all zero: its volume is 0 and the reference divides by it", who, o);
            vn[(size_t)o] = std::sqrt(vn[(size_t)o]);           // sqrt(sum(noise_data ** 2))
        }
    }
    g->copies.assign(copies, copies + n_copies);
    g->pieces.assign(pieces, pieces + n_pieces);
    g->noise_volume.swap(vn);
    return PE_OK;
}

int pe_augmenter_volumes(pe_augmenter* g, double* clip_volume, double* noise_volume, int64_t* overflowed) {
    const char* who = "pe_augmenter_volumes";
    if (!g) return PE_ERR_INVALID;
    pe_engine* e = g->e;
    if (!e) return fail(e, PE_ERR_INVALID, "%s: the session was created without an engine: it checks plans only", who);
    if (clip_volume) std::copy(g->clip_volume.begin(), g->clip_volume.end(), clip_volume);
    if (noise_volume) std::copy(g->noise_volume.begin(), g->noise_volume.end(), noise_volume);
    const int32_t n = (int32_t)g->copies.size();
    if (!overflowed || n == 0) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    int rc;
    if ((rc = ensure(e, g->buf[kAugOverflow], (size_t)n * sizeof(unsigned long long)))) return rc;
    PE_HIP(e, hipMemsetAsync(g->buf[kAugOverflow].p, 0, (size_t)n * sizeof(unsigned long long), nullptr));
    std::vector<int32_t> ids((size_t)n);
    for (int32_t o = 0; o < n; ++o) ids[(size_t)o] = o;
    std::vector<int64_t> begin;
    for (int32_t i0 = 0; i0 < n;) {             // the mix of every copy, nothing written but the counts
        const int32_t i1 = augmenter_pass_end(g, ids.data(), i0, n);
        if ((rc = augmenter_mix(g, ids.data() + i0, i1 - i0, begin, nullptr, nullptr, nullptr, static_cast<unsigned long long*>(g->buf[kAugOverflow].p)))) return rc;
        PE_HIP(e, hipStreamSynchronize(nullptr));
        i0 = i1;
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied out as they are");
    PE_HIP(e, hipMemcpy(overflowed, g->buf[kAugOverflow].p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_augmenter_audio(pe_augmenter* g, int32_t copy, double* mixed_out, int16_t* pcm_out) {
    const char* who = "pe_augmenter_audio";
    if (!g) return PE_ERR_INVALID;
    pe_engine* e = g->e;
    int rc = augmenter_check_ids(g, who, &copy, 1);
    if (rc) return rc;
    if (!mixed_out && !pcm_out) return PE_OK;
    PE_HIP(e, hipSetDevice(e->device));
    PE_DRAIN(e);
    const int64_t len = g->copy_length(copy);
    if (mixed_out && (rc = ensure(e, g->buf[kAugMixed], (size_t)len * sizeof(double)))) return rc;
    if (pcm_out && (rc = ensure(e, g->buf[kAugPcm], (size_t)len * sizeof(int16_t)))) return rc;
    std::vector<int64_t> begin;
    if ((rc = augmenter_mix(g, &copy, 1, begin, nullptr, mixed_out ? static_cast<double*>(g->buf[kAugMixed].p) : nullptr,
                            pcm_out ? static_cast<int16_t*>(g->buf[kAugPcm].p) : nullptr, nullptr))) return rc;
    if (mixed_out) PE_HIP(e, hipMemcpy(mixed_out, g->buf[kAugMixed].p, (size_t)len * sizeof(double), hipMemcpyDeviceToHost));
    if (pcm_out) PE_HIP(e, hipMemcpy(pcm_out, g->buf[kAugPcm].p, (size_t)len * sizeof(int16_t), hipMemcpyDeviceToHost));
    return PE_OK;
}

int pe_augmenter_vectorize(pe_augmenter* g, const int32_t* ids, int32_t n, int64_t max_samples, float* feats_out_host) {
    if (!g) return PE_ERR_INVALID;
    if (n > 0 && !feats_out_host) return fail(g->e, PE_ERR_INVALID, "null argument to pe_augmenter_vectorize");
    return augmenter_rows(g, "pe_augmenter_vectorize", ids, nullptr, n, max_samples, feats_out_host, nullptr, 0);
}

int pe_augmenter_append(pe_augmenter* g, pe_trainer* trainer, int32_t source, const int32_t* ids, const float* targets, int32_t n,
                        int64_t max_samples) {
    const char* who = "pe_augmenter_append";
    if (!g) return PE_ERR_INVALID;
    pe_engine* e = g->e;
    if (!e) return fail(e, PE_ERR_INVALID, "%s: the session was created without an engine: it checks plans only", who);
    if (n > 0 && !targets) return fail(e, PE_ERR_INVALID, "null argument to %s", who);
    int rc;
    if ((rc = check_append(e, who, trainer, source)) || (rc = check_targets(e, who, targets, n))) return rc;
    return augmenter_rows(g, who, ids, targets, n, max_samples, nullptr, trainer, source);
}

}  // extern "C"
