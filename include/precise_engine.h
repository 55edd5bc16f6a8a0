/*
 * precise_engine.h -- C ABI of the MI355X-native wake-word hot path
 * (libprecise_engine.so, built from mycroft_precise_amd/csrc by hipcc for gfx950).
 *
 * The reference (MycroftAI/mycroft-precise) is pure Python, so there is no existing FFI to
 * mirror; each entry point below replaces one Python-level seam of the reference and cites it
 * (paths relative to /root/reference).  A maintainer binds this library with ctypes exactly as
 * mycroft_precise_amd/_lib.py does -- see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns a pe_status (0 = ok); nothing throws across the ABI;
 *     pe_last_error() returns a human-readable message for the last failure on that engine
 *     (pe_last_global_error() for failures of pe_create itself);
 *   - the caller owns every buffer it passes; the engine copies what it keeps;
 *   - an engine owns the state of n_streams independent audio streams (leftover PCM + the
 *     [n_features x n_mfcc] feature window of network_runner.py:102-104) on ONE device; it is
 *     not thread-safe (the reference's Listener is not either, network_runner.py:98-153);
 *   - "host" entry points take host pointers and synchronise; "*_device" entry points take
 *     device pointers of the engine's device plus a hipStream_t (as void*) and are asynchronous;
 *   - PCM is little-endian int16 mono (util.py:35-37), laid out [n_streams][chunk_samples].
 */
#ifndef PRECISE_ENGINE_H
#define PRECISE_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_ABI_VERSION 8

typedef enum pe_status {
    PE_OK = 0,
    PE_ERR_INVALID = 1,      /* bad argument (maps to ValueError)                         */
    PE_ERR_HIP = 2,          /* a HIP runtime call failed                                 */
    PE_ERR_UNSUPPORTED = 3,  /* parameter combination this build has no kernel for        */
    PE_ERR_NOMEM = 4,
    PE_ERR_EOF = 5           /* empty chunk (maps to EOFError, network_runner.py:133-134) */
} pe_status;

/* ListenerParams (precise/params.py:28-118): the derived sizes the hot path reads. */
typedef struct pe_params {
    int32_t sample_rate;     /* 16000                                        params.py:142 */
    int32_t window_samples;  /* 1600   int(sample_rate*window_t+0.5)         params.py:84  */
    int32_t hop_samples;     /* 800    int(sample_rate*hop_t+0.5)            params.py:89  */
    int32_t n_fft;           /* 512    ANY length in 16..1024 (np.fft.rfft takes any n),
                                       or the power of two 2048                       params.py:142 */
    int32_t n_filt;          /* 20     mel filters, 1..128                   params.py:142 */
    int32_t n_mfcc;          /* 13     coefficients kept, 1..32, <= n_filt   params.py:142
                                Front-end kernels: the stock shape (n_fft = 512, <= 64 filters whose runs fit the 64
                                lanes of a wave, <= 16 coefficients) runs on the one-frame-per-wave kernel and the fused
                                launch; EVERY OTHER shape in the ranges above runs on the general front end (same
                                results contract, two launches per update and per pe_update_many call -- one network
                                launch per update of the call for rows of 17..32 coefficients).  17..32 coefficients feed the float32 network
                                (gru_precision = 0) of any width it serves -- <= 32 units, and wide / stacked networks of
                                33..256 units -- without use_delta only: a network's first layer takes up to 32 inputs.  bf16
                                operands / rows take <= 16 coefficients on either front end.  An n_fft that is
                                not a power of two >= 64 (16 and 32 included) runs as Bluestein's chirp-z transform over
                                the next power of two >= max(128, 2 n_fft - 1) (one wave's LDS holds it up to n_fft =
                                1024).  Outside the ranges (n_fft > 2048, not a power of two and > 1024, < 16, ...):
                                PE_ERR_UNSUPPORTED.                                                                    */
    int32_t n_features;      /* 29     T, timesteps per network input        params.py:79  */
    int32_t use_delta;       /* 0      1: network inputs are [x_t, x_t - x_(t-1)]
                                       (vectorization.py:53-59), layer n_in = 2 n_mfcc   params.py:143 */
    int32_t mfcc_precision;  /* 0 = float64 front end (what the reference computes in,
                                network_runner.py:102,137);  1 = float32 front end        */
    int32_t gru_precision;   /* 0 = float32 matrix cores (reference precision, tol 1e-4): every network
                                the trainers save -- 1..256 units, 1-2 layers, up to 32 inputs per frame
                                (use_delta over <= 16 coefficients, or 17..32 coefficients; wide / stacked
                                networks read them as two k-groups of 16);
                                1 = bf16 operands / float32 accumulate (BASELINE configs[4],
                                tol 1e-2), any network the engine serves: <= 32 units, and wide /
                                stacked networks of 33..256 units and 1-2 layers (DESIGN.md 4.4:
                                weights, features, h and r*h of every layer and layer 2's input are
                                rounded as operands; the carried state stays float32).  bf16-operand
                                wide networks take plain rows of <= 16 coefficients: no use_delta; and
                                no wide network takes ring_precision = 1.                    */
    int32_t vectorizer;      /* params.py:121-132: 2 = mfccs (sonopy, the default; pe_vectorize_mels and
                                pe_vectorize_clips(mels = 1) also give its log-mel rows),
                                3 = speechpy_mfccs (legacy .params files without
                                a `vectorizer` key, params.py:147,155): one frame fewer per buffer
                                (a frame is emitted one hop later), exact zeros -- not small values --
                                replaced by eps before the log; the caller supplies that library's
                                filterbank as mel_filters.  0 is read as 2.
                                1 = mels (vectorization.py:32-35 -> sonopy.mel_spec): a row is the n_filt
                                log-mel energies safe_log(power . filters^T) -- no DCT, value 0 NOT replaced
                                by the log power -- over sonopy's filterbank.  The row width W = n_filt stands
                                wherever an mfccs engine has n_mfcc: the window is [n_features][W], the
                                first layer takes W inputs (2 W with use_delta), pe_get_vectors /
                                pe_set_vectors / pe_update_vectors / pe_vectorize_raw / pe_vectorize_clips
                                (whatever its mels flag) are W wide, pe_get_info reports n_mfcc = W; the
                                given n_mfcc keeps its range check and is otherwise ignored.  Limits, each
                                PE_ERR_UNSUPPORTED before any device work: n_filt <= 32; more than 16 values
                                per row feed a float32 network without use_delta and without bf16 rows; a
                                first layer of another width ("Vectorizer.mels feeds 20 inputs per frame,
                                this network takes 13"); pe_miner_create, pe_generator_create and
                                pe_augmenter_create refuse such an engine.  (The filterbank is the
                                caller's table: the Python layer refuses the speechpy one.)  DESIGN 4.17 */
    int32_t ring_precision;  /* 0 = float32 feature rows (64 B per frame and stream);
                                1 = bf16 feature rows (32 B), rounded to nearest even where the row is
                                stored -- needs gru_precision = 1 (BASELINE configs[4])         */
} pe_params;

/* One Keras GRU layer (precise/model.py:77-81), Keras weight layout, gate order z|r|h. */
typedef struct pe_gru_layer {
    int32_t n_in;                    /* F (13) for layer 0, units of the previous layer after */
    int32_t units;                   /* H (20): 1..32 register-resident kernels; 33..256 the streamed-weight
                                        kernel (zero-padded to a multiple of 64 inside)           */
    const float* kernel;             /* [n_in][3*units] row-major                              */
    const float* recurrent_kernel;   /* [units][3*units]                                       */
    const float* bias;               /* [3*units]                                              */
} pe_gru_layer;

/* Sequential([GRU..., Dense(1, sigmoid)])   (precise/model.py:76-82) */
typedef struct pe_weights {
    int32_t n_layers;                /* 1 in the reference; 2 = GRU(H1, return_sequences) -> GRU(H2), widths
                                        33..256 (BASELINE configs[3]: 256, 256)                   */
    const pe_gru_layer* layers;
    const float* dense_kernel;       /* [units_last]                                           */
    float dense_bias;
} pe_weights;

typedef struct pe_engine pe_engine;

int pe_abi_version(void);
const char* pe_last_global_error(void);

/* Replaces Listener.__init__ (network_runner.py:101-108) for n_streams streams at once.
 * mel_filters: [n_filt][n_fft/2+1] float64 row-major triangular filterbank, built by the host
 * exactly as the vectorizer the reference calls does (vectorization.py:36-39 -> sonopy). */
int pe_create(const pe_params* params, const double* mel_filters, const pe_weights* weights,
              int32_t n_streams, int32_t device, pe_engine** out);
int pe_destroy(pe_engine* e);
const char* pe_last_error(const pe_engine* e);

/* Several wake-word models on the same streams (ABI 8).  The reference runs one model per listener:
 * precise/scripts/engine.py builds one Listener(model_name, chunk_size) per process and
 * runner/precise_runner/runner.py PreciseEngine(exe_file, model_file) one model, so two hotwords on the same
 * audio take two listeners -- two front ends over identical PCM.  pe_create_models builds ONE engine with one
 * front end, one feature window per stream and n_models networks: a Listener (network_runner.py:98-153) per
 * model over shared MFCC frames.
 *   - weights[0 .. n_models), 1 <= n_models <= 8 (else PE_ERR_INVALID).  Every model has model 0's n_layers,
 *     units per layer and n_in per layer, else PE_ERR_UNSUPPORTED naming the model and the field; all of
 *     this is checked before any device work.  The models share the whole pe_params (front end, feature
 *     window, use_delta, precisions).  pe_create(...) == pe_create_models(..., n_models = 1, ...).
 *   - Outputs: every entry point that writes network outputs writes n_models blocks, model first; block m is
 *     bit for bit what a one-model engine with model m, the same params, n_streams and form
 *     (pe_get_gru_tiling) writes: pe_update[_device|_device_keep], pe_run_device, pe_update_async (its pinned
 *     landing zones are sized for it) [K][n_streams]; pe_update_subset[_device|_async] [K][n_active]
 *     (pe_decode_subset[_device] and the conf / fired of pe_update_subset_async likewise);
 *     pe_update_many[_device] [K][n_updates][n_streams]; pe_predict[_device] [K][n];
 *     pe_evaluate [K][max_windows] (n_windows_out is the same for every model); pe_decode[_device] reads
 *     raw[K][n_streams] and writes conf / fired [K][n_streams].  Entry points without a network (vectors,
 *     clear, get / set_vectors, vectorize_*) are unchanged.
 *   - Launches: a K-model engine never takes more launches than a one-model engine.  Where one model fuses the
 *     update into one launch, K network roles run beside the one frame role in that launch (the network shape
 *     chosen from K and the stream tiles); where one model takes two launches, the second is ONE
 *     network launch for all K models; pe_update_many, pe_predict and pe_evaluate take one network launch for all
 *     models; pe_decode is one launch over K x n_streams with per-model tables.  Exception: wide / stacked networks
 *     (33..256 units) take one network launch per model -- each fills the machine on its own (configs[3]: 0.79
 *     of the fp32 MFMA peak).
 *   - Knobs apply to every model: pe_set_gru_tiling / pe_set_gru_waves / pe_set_fused give all models one
 *     form; pe_set_input_projection(e, 1) on n_models > 1 returns PE_ERR_UNSUPPORTED (projection rows are
 *     per model); pe_set_decoder / pe_set_trigger set every model, pe_set_decoder_model /
 *     pe_set_trigger_model one (each model's .params threshold_config / threshold_center and each
 *     hotword's sensitivity; one TriggerDetector per (model, stream)). */
int pe_create_models(const pe_params* params, const double* mel_filters, const pe_weights* weights,
                     int32_t n_models, int32_t n_streams, int32_t device, pe_engine** out);
int pe_get_n_models(const pe_engine* e);

/* Replace the network of model `model` in a live engine: what scripts/train_incremental.py:86-88,106 gets by training the very
 * model object its Listener predicts with -- the next chunk is judged by the retrained network, the stream goes on.  Additive to
 * ABI 8.  The weights are packed by the routines pe_create used, into the buffers pe_create made: afterwards every entry
 * point gives, bit for bit, what an engine created with these weights gives (the form, pe_get_gru_tiling, does not change).
 * The stream state -- leftover samples, feature windows, triggers -- is untouched.  Work in flight (pe_update_async, the
 * *_device entry points on any stream) is drained first.
 * PE_ERR_INVALID, before any device work and with the old network still serving: null pointers, a model outside
 * 0 .. n_models - 1, n_layers / units / n_in other than the engine was created with.  The input-projection rows
 * (pe_set_input_projection) are rebuilt from the new network, and with the option on the projections of the frames already in
 * the feature windows are computed again. */
int pe_set_weights(pe_engine* e, const pe_weights* weights, int32_t model);

/* Listener.clear (network_runner.py:121-123).  mask: n_streams bytes, non-zero = clear that
 * stream; NULL = clear all.  Runs on the NULL stream and synchronises: a caller that drives the
 * *_device entry points on a non-blocking stream must synchronise that stream first (the same holds for
 * pe_get_vectors / pe_set_vectors / pe_get_stream_state). */
int pe_clear(pe_engine* e, const uint8_t* mask);

/* Listener.update up to, not including, ThresholdDecoder.decode (network_runner.py:148-152):
 * append one chunk per stream, emit any new MFCC frames into the feature window, run the
 * network on the window.  raw_out[n_streams] = raw sigmoid output (float32).
 * chunk_samples == 0 -> PE_ERR_EOF. */
int pe_update(pe_engine* e, const int16_t* pcm_host, int32_t chunk_samples, float* raw_out_host);
int pe_update_device(pe_engine* e, const int16_t* pcm_dev, int32_t chunk_samples,
                     float* raw_out_dev, void* hip_stream);

/* The same update for a caller whose device chunks OUTLIVE the call (a ring of resident PCM slabs, a capture buffer that is
 * written ahead).  Listener.update_vectors keeps the samples that do not yet fill a frame (network_runner.py:127-131: the
 * `leftover` of chop_array); pe_update_device copies them into the engine's own carry, every call, for every stream.  Here they
 * stay where they lie -- in pcm_dev -- and the NEXT call cuts the head of its first frame from there.  The promise: pcm_dev
 * stays allocated and unchanged until the work of the next call that advances or clears streams on this engine has completed
 * on its stream (or the engine is destroyed).  Any entry point may follow (a call of another style first moves the leftovers
 * to the carry in one small launch); results are bit-identical to pe_update_device.  Chunks that cannot hold a leftover (odd
 * length, fewer than frame_len - 1 samples, an address that is not 4-byte aligned, a non-stock front end) are taken exactly
 * as pe_update_device takes them.  A call whose chunks overlap the previous keep call's is refused (PE_ERR_INVALID: the leftovers
 * would be gone; the streams' state is untouched).  pe_update_async works this way by itself: its device chunks are the engine's own. */
int pe_update_device_keep(pe_engine* e, const int16_t* pcm_dev, int32_t chunk_samples,
                          float* raw_out_dev, void* hip_stream);

/* Streams that advance independently.  Every reference Listener consumes chunks at its own pace (network_runner.py:125-146;
 * one engine process per client, runner/precise_runner/runner.py:54-67, :232-243); a server that multiplexes many clients on
 * one engine has audio for SOME of them at any moment.  pe_update_subset: stream stream_ids[i] (0 <= id < n_streams, each at
 * most once) takes chunk i of pcm[n_active][chunk_samples] and gets raw_out[i]; every other stream keeps its leftover
 * samples, counters and feature window untouched.  Same launches as pe_update (the fused one where pe_update fuses), sized by
 * n_active: cost follows the active streams, not the engine.  Results are those of a private Listener per stream, bit-identical
 * to pe_update whenever the same streams get the same chunks.  n_active == 0 is a no-op (PE_OK); chunk_samples == 0 with
 * n_active > 0 -> PE_ERR_EOF.  Callers with several chunk lengths at once issue one call per length.
 * The host entry point validates the ids (PE_ERR_INVALID: out of range / named twice); the device entry point cannot: ids
 * out of range or repeated are undefined behaviour there. */
int pe_update_subset(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const int16_t* pcm_host,
                     int32_t chunk_samples, float* raw_out_host);
int pe_update_subset_device(pe_engine* e, const int32_t* stream_ids_dev, int32_t n_active, const int16_t* pcm_dev,
                            int32_t chunk_samples, float* raw_out_dev, void* hip_stream);

/* Host-fed pipeline: the reference's engine is handed HOST bytes per chunk (precise/scripts/engine.py:60-63,
 * runner/precise_runner/runner.py:62-67), and pe_update above is copy -> launch -> copy, one after the other.
 * pe_update_async enqueues the same update and returns: the chunk of update u + 1 crosses PCIe (a copy stream of the
 * engine's own) while update u runs (a compute stream of the engine's own), the probabilities come back behind the
 * launch; up to 3 updates are in flight, a 4th call first delivers the oldest.  raw_out_host[n_streams] is valid after
 * pe_wait (or once 3 more updates have been enqueued).  Results are bit-identical to pe_update / pe_update_device.
 *   - pageable pcm_host: staged by the HIP runtime at the call (the caller's PCM buffer is free again when the call
 *     returns); pageable raw_out_host: filled from the engine's pinned ring when the update is delivered;
 *   - buffers from pe_host_alloc (pinned, device-visible; freed by pe_host_free or pe_destroy): ZERO-COPY -- the DMA
 *     reads / writes them directly, which is what reaches PCIe line rate (a CPU memcpy of 8 MB per update does not);
 *     such a PCM buffer must stay untouched until pe_wait or until 3 more updates have been enqueued.
 * Every other entry point that reads or moves the streams' state (pe_update*, pe_clear, pe_get_vectors, ...) first
 * waits for the updates in flight, so the two styles may be mixed; callers that drive the *_device entry points on
 * their own non-blocking stream synchronise that stream before switching to pe_update_async (as for pe_clear). */
int pe_host_alloc(pe_engine* e, size_t bytes, void** out);
int pe_host_free(pe_engine* e, void* p);
int pe_update_async(pe_engine* e, const int16_t* pcm_host, int32_t chunk_samples, float* raw_out_host);
int pe_wait(pe_engine* e);

/* The pipeline for streams that advance independently -- what a server that multiplexes many clients on one engine calls
 * per tick: host PCM for SOME streams in, raw output, decoded confidence and activation per active stream out.  The update
 * is pe_update_subset's (same launch choice, same bits), enqueued on pe_update_async's ring of 3 (the chunks cross PCIe on the
 * copy stream, the ids in front of the update on the compute stream); when conf_out_host or fired_out_host is given, ONE pe_decode_subset launch over the update's raw
 * outputs follows it on the compute stream, then the copies back.  All three outputs are [n_models][n_active] in the order
 * of the ids and valid after pe_wait (or once 3 more updates have been enqueued); each of them is, independently, pageable
 * (filled at delivery) or pe_host_alloc'ed (written by the DMA).  The ids are read at the call.
 *   - stream_ids_host == NULL: every stream in order; n_active must be n_streams.  That is pe_update_async's update plus
 *     the decode -- a pipelined update + pe_decode for lock-step callers;
 *   - refused before anything is enqueued (PE_ERR_INVALID): n_active outside 0..n_streams, ids out of range or named twice,
 *     raw_out_host NULL, conf / fired asked for without pe_set_decoder.  chunk_samples == 0 with n_active > 0 -> PE_ERR_EOF;
 *     n_active == 0 is a no-op (PE_OK) that leaves the outputs untouched;
 *   - a stream named in two updates in flight is served in the order of the calls (one compute stream).
 * pe_update_async and this call may be mixed freely. */
int pe_update_subset_async(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const int16_t* pcm_host,
                           int32_t chunk_samples, float* raw_out_host, double* conf_out_host, unsigned char* fired_out_host);

/* n_updates consecutive pe_update calls in two launches (results bit-identical): chunk u of stream s at
 * pcm[(u * n_streams + s) * chunk_samples], raw_out[u * n_streams + s].  First one launch computes every
 * MFCC frame the call completes (frame-parallel: which samples form which frame is closed-form over
 * leftover ++ chunk 0 ++ ... ++ chunk n-1), then one launch runs the network for all
 * n_updates x n_streams windows -- for callers that can buffer a few chunks (catch-up, bulk
 * replay, latency-tolerant servers) this fills the machine where a single update of a few thousand
 * streams cannot.  pe_reserve_updates sizes the feature ring, the second leftover buffer and the
 * per-update counters for it (and restarts all streams); n_updates * chunk_samples < 2^30.
 * Engines on the general front end (see pe_params) take one front-end launch per call as well, then the batched network
 * launch (rows of 17..32 coefficients: one network launch per update of the call); same bits.  The enlarged ring stays: later single pe_update calls on a reserved engine are unchanged in their
 * results but, up to 8192 streams, use the one-wave network shape (the critical-wave shape stages exactly 32 ring slots in
 * LDS) -- reserve only on engines that use pe_update_many.
 * Network form of a reserved engine (pe_set_gru_tiling -1, the default): when max_updates x stream tiles exceeds four per
 * compute unit (e.g. 4096 streams x 8 updates), the float32 network takes form 2 (float32 products on the bf16 pipe) for ALL
 * launches of the engine -- the batched launch is what the engine was reserved for (402 vs 296 M windows/s at that size), and
 * one form per engine keeps pe_update == pe_update_many bit for bit.  Single updates on such an engine take two launches.  An
 * unreserved engine of the same size runs form 1: the two agree to float32 summation order (<= 1e-6), not bit for bit. */
int pe_reserve_updates(pe_engine* e, int32_t max_updates, int32_t max_chunk_samples);
int pe_update_many(pe_engine* e, const int16_t* pcm_host, int32_t chunk_samples, int32_t n_updates, float* raw_out_host);
int pe_update_many_device(pe_engine* e, const int16_t* pcm_dev, int32_t chunk_samples, int32_t n_updates,
                          float* raw_out_dev, void* hip_stream);

/* Listener.update_vectors (network_runner.py:125-146): as pe_update without the network;
 * feats_out[n_streams][n_features][n_mfcc] float32, oldest row first (may be NULL). */
int pe_update_vectors(pe_engine* e, const int16_t* pcm_host, int32_t chunk_samples,
                      float* feats_out_host);
int pe_update_vectors_device(pe_engine* e, const int16_t* pcm_dev, int32_t chunk_samples,
                             float* feats_out_dev, void* hip_stream);

/* Listener.mfccs (network_runner.py:104,144): copy out the current feature windows,
 * feats_out[n_streams][n_features][n_mfcc] float32, oldest row first; consumes no audio. */
int pe_get_vectors(pe_engine* e, float* feats_out_host);

/* Assignment to Listener.mfccs / a Listener whose runner is replaced after construction
 * (scripts/train_incremental.py:87-88): every stream restarts (pe_clear) with the given feature window
 * already emitted and no leftover audio; feats[n_streams][n_features][n_mfcc] float32, oldest row
 * first.  Feed the leftover samples back with pe_update_vectors to restore a whole Listener state. */
int pe_set_vectors(pe_engine* e, const float* feats_host);

/* Run the network on the current feature windows without consuming audio. */
int pe_run_device(pe_engine* e, float* raw_out_dev, void* hip_stream);

/* Runner.predict (network_runner.py:35-38): feats[n][n_features][feature_size] float32 -> out[n]
 * (feature_size = n_mfcc, or 2 n_mfcc with use_delta: the batch then carries its delta columns). */
int pe_predict(pe_engine* e, const float* feats_host, int32_t n, float* out_host);
int pe_predict_device(pe_engine* e, const float* feats_dev, int32_t n, float* out_dev,
                      void* hip_stream);

/* vectorize_raw (vectorization.py:46-50) for the Vectorizer.mfccs entry (:36-39): stateless
 * MFCC of one whole buffer.  audio: float64 samples in [-1,1) (what the reference's vectorizer
 * receives).  feats_out[max_frames][n_mfcc] float64; *n_frames_out = 1+(n-window)//hop or 0.
 * An engine created with vectorizer = 1 dispatches as vectorize_raw does: the mel rows, [max_frames][n_filt]. */
int pe_vectorize_raw(pe_engine* e, const double* audio_host, int64_t n_samples,
                     double* feats_out_host, int64_t max_frames, int64_t* n_frames_out);

/* The same buffer through the Vectorizer.mels entry (vectorization.py:32-35 -> sonopy.mel_spec): log of the
 * mel filterbank energies, no DCT.  mels_out[max_frames][n_filt] float64.  Any engine has this entry: an mfccs engine
 * gives the log-mel rows beside its MFCC rows (the reference's offline tools under pr.vectorizer = mels), an engine created
 * with vectorizer = 1 gives the rows it streams -- the bits pe_vectorize_raw returns there. */
int pe_vectorize_mels(pe_engine* e, const double* audio_host, int64_t n_samples,
                      double* mels_out_host, int64_t max_frames, int64_t* n_frames_out);

/* The reference's batched offline evaluation (precise/scripts/simulate.py:92-104, also
 * annoyance_estimator.py:114-130): MFCC of one whole recording, one network input per hop_frames
 * (= chunk_size // hop_samples) frames -- windows ending at frame i for i in range(n_features,
 * n_frames, hop_frames) -- all predicted in one batch.  out[n_windows] raw outputs; nothing of the
 * [n_windows][T][F] batch is materialised: the network reads overlapping windows of one row
 * sequence.  Stateless (the engine's streams are untouched). */
int pe_evaluate(pe_engine* e, const double* audio_host, int64_t n_samples, int32_t hop_frames,
                float* out_host, int64_t max_windows, int64_t* n_windows_out);

/* vectorize() of vectorization.py:62-84 for n_clips buffers at once, and the batch the dataset tools build from it
 * (train_data.py:195-196: vectorizer(load_audio(x)) for every wav of a folder; scripts/test.py:48-53 and eval.py:103-105:
 * predict(inputs) over those vectors; vectorize_inhibit, vectorization.py:92-105: cropped copies of one clip).
 * Clip c is samples [offsets[c], offsets[c + 1]) of audio_host; offsets[n_clips + 1] is non-decreasing and starts at 0.
 * sample_format: 0 = float64 samples (as pe_vectorize_raw takes), 1 = float32 samples (what load_audio returns,
 * util.py:45-65), widened on the device -- exact, so both formats give the same bits.
 * Per clip, as vectorize does: the last max_samples samples (max_samples <= 0: no crop), the frames of what is left
 * (anchored at its start; one fewer with vectorizer = 3), the last n_features of them, all-zero rows in front up to
 * n_features; a clip shorter than one window gives an all-zero window.
 * pe_vectorize_clips: feats_out[n_clips][n_features][n_mfcc] float64, or -- mels = 1, the Vectorizer.mels entry --
 * [n_clips][n_features][n_filt] log-mel rows (an engine created with vectorizer = 1: those rows whatever the flag).
 * pe_score_clips: the network over every clip's window, out[n_models][n_clips] raw outputs (use_delta models: the deltas
 * of the padded window, zero in its first row, as vectorize_delta forms them, vectorization.py:87-89).
 * One front-end launch and (scores) one network launch per pass; the clips are staged in passes of 256 MiB of audio (a pass
 * takes at least one clip) and the results do not depend on the pass size.  An empty clip is PE_ERR_INVALID (the
 * reference raises InvalidAudio) and the message names it; so are decreasing offsets, null pointers with n_clips > 0 and
 * n_clips < 0 -- all checked before any device work, the outputs untouched.  n_clips = 0 does nothing.  Stateless (the
 * engine's streams are untouched); updates of pe_update_async still in flight finish first. */
int pe_vectorize_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host,
                       int32_t n_clips, int64_t max_samples, int32_t mels, double* feats_out_host);
int pe_score_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host,
                   int32_t n_clips, int64_t max_samples, float* out_host);
/* Test aid: the audio bytes one pass of the two calls above stages (>= 1; default 256 MiB), so that a small test can cross
 * pass boundaries. */
int pe_set_clip_pass_bytes(pe_engine* e, int64_t bytes);

/* precise-simulate (scripts/simulate.py:106-129) and AnnoyanceEstimator.compute_nww_annoyances (annoyance_estimator.py:56-73)
 * for a whole folder of long recordings in one call: per recording the whole-file MFCC, one prediction every hop_frames
 * frames (pe_evaluate, above), a fresh TriggerDetector over the predictions, three sums, and a count of the predictions
 * above each threshold of a table.
 * Recording r is samples [offsets[r], offsets[r + 1]) of audio_host; audio_host / sample_format / offsets as
 * pe_vectorize_clips takes them.  There is no crop.  A zero-length recording is allowed: it has no window (pe_evaluate with
 * n_samples = 0; simulate.py:110 skips such files).  Frames and windows are counted per recording as pe_evaluate counts them:
 * windows end at frames range(n_features, n_frames, hop_frames).  window_offsets[n_rec + 1] is the exclusive prefix sum of the
 * window counts; pe_evaluate_clips_layout computes it on the host without any device work, so that a caller can size `out`.
 * pe_evaluate_clips: out[n_models][max_windows]; model m, recording r, window j at out[m * max_windows + window_offsets[r] + j],
 * bit for bit what pe_evaluate returns for that recording alone on this engine: the frames are the same function, and the
 * recordings' rows are laid out so that pe_evaluate's network launch serves all of them at once.
 * pe_simulate_scores: the metrics alone, over predictions the caller holds: raw[n_models][stride], recording r's at
 * raw[m * stride + window_offsets[r] ...].  Every comparison is made on (double)p, the float32 prediction widened:
 *   activated_chunks  p > chunk_threshold                                   ((predictions > sensitivity).sum(), simulate.py:119)
 *   activations       True returns of TriggerDetector(chunk_size, sensitivity, trigger_level).update (runner.py:127-142: hot is
 *                     p > 1.0 - sensitivity, rearm is -(8 * 2048) // chunk_size), fresh per (model, recording)  (simulate.py:114,120)
 *   activation_sum    the sum of p in float64, in an order that depends on the recording's length alone: the same bits in
 *                     every run, with any pass size and whatever else the call holds                          (simulate.py:121)
 *   buckets_out[n_models][n_thresholds]: windows of ALL recordings of the call with p > thresholds[j]
 *                     (annoyance_estimator.py:70-71).  thresholds: non-decreasing, no NaN, n_thresholds in 0..4096;
 *                     n_thresholds = 0: buckets_out may be NULL.
 * simulate.py compares against `sensitivity` at :119 and against `1 - sensitivity` at :114/:142, hence two arguments; the
 * script passes its --threshold for both.  (numpy may make the :119 comparison in float32: it differs from this one only
 * where a prediction equals the float32 rounding of the threshold.)
 * pe_simulate_clips: pe_evaluate_clips and pe_simulate_scores in one call, the predictions staying on the device; out
 * (may be NULL) receives them as pe_evaluate_clips lays them out.  metrics_out[n_models][n_rec].
 * Passes as for pe_vectorize_clips (pe_set_clip_pass_bytes applies): whole recordings, at least one per pass -- a recording
 * larger than the target travels alone -- and no result depends on the pass size.  One front-end launch, one network launch
 * and the two metrics kernels per pass.  At most 2^31 - 1 frames per recording and windows per call.
 * PE_ERR_INVALID, checked before any device work and with the outputs untouched: null pointers with n_rec > 0, n_rec < 0,
 * decreasing offsets, offsets[0] != 0, hop_frames < 1, chunk_size < 1, sensitivity or chunk_threshold NaN, max_windows too
 * small when out is given, thresholds out of order or NaN, n_thresholds out of range.  n_rec = 0 does nothing.  Stateless;
 * updates of pe_update_async still in flight finish first. */
typedef struct pe_sim_metric {      /* one (model, recording); simulate.py:116-122 */
    int64_t n_windows;
    int64_t activated_chunks;
    int64_t activations;
    double  activation_sum;
} pe_sim_metric;
int pe_evaluate_clips_layout(pe_engine* e, const int64_t* offsets_host, int32_t n_rec, int32_t hop_frames,
                             int64_t* window_offsets_out);
int pe_evaluate_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_rec,
                      int32_t hop_frames, float* out_host, int64_t max_windows);
int pe_simulate_scores(pe_engine* e, const float* raw_host, int64_t stride, const int64_t* window_offsets, int32_t n_rec,
                       double chunk_threshold, double sensitivity, int32_t trigger_level, int32_t chunk_size,
                       const double* thresholds, int32_t n_thresholds, pe_sim_metric* metrics_out, int64_t* buckets_out);
int pe_simulate_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_rec,
                      int32_t hop_frames, double chunk_threshold, double sensitivity, int32_t trigger_level, int32_t chunk_size,
                      const double* thresholds, int32_t n_thresholds, pe_sim_metric* metrics_out, int64_t* buckets_out,
                      float* out_host, int64_t max_windows);

/* precise-test, precise-graph and precise-calc-threshold (stats.py:46-58,102-107; scripts/graph.py:147-151;
 * scripts/calc_threshold.py:66-77) and the wake-word buckets of the annoyance estimate (annoyance_estimator.py:83-84) for
 * several rows of predictions -- one per network -- against one row of targets and a whole table of thresholds in one call.
 * Targets, shared by the rows: positive is y > 0.5, negative is y == 0; a target in (0, 0.5], which a trainer's resident
 * sets may hold and on which the reference's own definitions disagree (astype(bool) against > 0.5 / < 0.5), is counted in
 * n_other and enters no other count.
 * thresholds: non-decreasing, no NaN, n_thresholds in 0..4096 (duplicates allowed); n_thresholds = 0: counts_out is NULL.
 * compare: PE_STATS_COMPARE_F32 makes every comparison p > (float)t / p >= (float)t, what numpy does when a float32 array
 * meets a Python float (Stats, with the floats ThresholdDecoder.encode returns); PE_STATS_COMPARE_F64 makes it
 * (double)p > t, what numpy does when it meets a float64 array (annoyance_estimator.py:83).  The two differ where a
 * prediction equals the float32 rounding of a threshold: float32(0.1) is above 0.1 in F64 and not in F32.
 * counts_out[n_rows][n_thresholds], per (row, threshold) the samples with p > t (Stats.calc_metric) and with p >= t
 * (Stats.num_correct), by target class: true_pos = pos_gt, false_pos = neg_gt, false_neg = n_pos - pos_gt, true_neg =
 * n_neg - neg_gt, num_correct = pos_ge + n_neg - neg_ge.  A NaN prediction is above no threshold.
 * summary_out[n_rows]: n and the class counts; n_nan, the NaN predictions; n_unsaturated, the predictions that are neither 0,
 * 1 nor NaN (save_spots, calc_threshold.py:66); n_fit, those of them with y > 0.5; and over these n_fit samples
 *   x = -log((double)u), u = fl32(fl32(1 / p) - 1)        (numpy's float32 `1 / outputs - 1`, then the logarithm in float64;
 *                                                          the reference takes it in float32, which is not the same bits on
 *                                                          every host)
 *   logit_mean = sum(x) / n_fit, logit_std = sqrt(sum((x - logit_mean)^2) / n_fit)    (two passes, calc_threshold.py:76-77,
 *                                                          without the smoothing factor; n_fit = 0: NaN for both)
 * with every sum in float64 in an order that depends on n alone: the same bits in every run, for a row alone or among
 * others, whatever the threshold table.
 * pe_stats_scores: predictions the caller holds, raw[n_rows][stride] with n valid per row, 1 <= n_rows <= 16.
 * pe_test_clips: pe_score_clips and pe_stats_scores in one call, the predictions staying on the device: every pass writes
 * its scores into one buffer [n_models][n_clips] and the statistics run once after the last pass, so no result depends on
 * pe_set_clip_pass_bytes.  targets_host[n_clips]; out_host [n_models][n_clips] (may be NULL) is bit for bit what
 * pe_score_clips returns.  n_clips = 0 does nothing.
 * pe_trainer_stats_models: every network of a trainer over host data or a resident set (source, feats_host, targets_host
 * and n as pe_trainer_evaluate_models takes them; host data needs targets); probs_out [n_models][n] (may be NULL) is bit for
 * bit what pe_trainer_evaluate_models returns.  Rows are the networks in model order.
 * PE_ERR_INVALID, checked before any device work and with the outputs untouched: null pointers, n < 1 (but n_clips = 0),
 * n > 2^31 - 1, n_rows outside 1..16, stride < n, thresholds out of order or NaN, n_thresholds outside 0..4096, compare other
 * than 0 or 1, a target outside [0, 1] or NaN, a resident set never uploaded, and whatever pe_score_clips /
 * pe_trainer_evaluate_models refuse.  The engine's streams are untouched; updates of pe_update_async still in flight finish
 * first. */
#define PE_STATS_COMPARE_F32 0
#define PE_STATS_COMPARE_F64 1
typedef struct pe_stats_count {     /* one (row, threshold) */
    int64_t pos_gt, neg_gt, pos_ge, neg_ge;
} pe_stats_count;
typedef struct pe_stats_summary {   /* one row */
    int64_t n, n_pos, n_neg, n_other, n_nan, n_unsaturated, n_fit;
    double logit_mean, logit_std;
} pe_stats_summary;
int pe_stats_scores(pe_engine* e, const float* raw_host, int32_t n_rows, int64_t stride, const float* targets_host, int64_t n,
                    const double* thresholds, int32_t n_thresholds, int32_t compare,
                    pe_stats_count* counts_out, pe_stats_summary* summary_out);
int pe_test_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_clips,
                  int64_t max_samples, const float* targets_host, const double* thresholds, int32_t n_thresholds, int32_t compare,
                  pe_stats_count* counts_out, pe_stats_summary* summary_out, float* out_host);

/* ThresholdDecoder.decode (threshold_decoder.py:45-57) and TriggerDetector.update
 * (runner/precise_runner/runner.py:127-142) for every stream, on the device.
 * pe_set_decoder: cd = the decoder's cumulative table (np.cumsum of the summed normal pdfs,
 * threshold_decoder.py:42,68-70), min_out / out_range / center as the Python object holds them.
 * pe_set_trigger: (re)arms one TriggerDetector per stream (chunk_size in BYTES as in runner.py:122).
 * pe_decode*: raw[n_streams] float32 -> conf[n_streams] float64 (may be NULL) and, when a trigger is
 * set, fired[n_streams] (1 = this prediction caused an activation; may be NULL).  The logit follows the
 * reference's evaluation on the runner's float32 scalar (functions.py:99-101: `1 / x - 1` rounds twice in
 * float32, the logarithm is taken in float64), so the table bin -- and with it the decoded value -- is the
 * one Listener.update returns, not the one a float64 logit would give. */
int pe_set_decoder(pe_engine* e, const double* cd, int32_t cd_len, int32_t min_out, int32_t out_range, double center);
int pe_set_trigger(pe_engine* e, int32_t chunk_size_bytes, double sensitivity, int32_t trigger_level);
/* the same for model `model` of a pe_create_models engine (0 <= model < pe_get_n_models(e)) */
int pe_set_decoder_model(pe_engine* e, int32_t model, const double* cd, int32_t cd_len, int32_t min_out, int32_t out_range, double center);
int pe_set_trigger_model(pe_engine* e, int32_t model, int32_t chunk_size_bytes, double sensitivity, int32_t trigger_level);
int pe_decode_device(pe_engine* e, const float* raw_dev, double* conf_out_dev, unsigned char* fired_out_dev, void* hip_stream);
int pe_decode(pe_engine* e, const float* raw_host, double* conf_out_host, unsigned char* fired_out_host);
/* The same after pe_update_subset: row i of raw / conf / fired ([n_models][n_active], in the order of the ids) belongs to
 * stream stream_ids[i], and only the named streams' TriggerDetectors move -- a stream that received no audio neither decays
 * nor fires (pe_decode would step every stream's).  One launch for all models.  The host entry point validates the ids as
 * pe_update_subset does (PE_ERR_INVALID: out of range / named twice), the device one cannot.  n_active == 0 is a no-op
 * (PE_OK); without pe_set_decoder the error is pe_decode's; without a trigger fired is zeros.
 * All four decode calls, like the setters above, first wait for updates in flight (pe_update_subset_async moves triggers). */
int pe_decode_subset_device(pe_engine* e, const int32_t* stream_ids_dev, int32_t n_active, const float* raw_dev,
                            double* conf_out_dev, unsigned char* fired_out_dev, void* hip_stream);
int pe_decode_subset(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const float* raw_host,
                     double* conf_out_host, unsigned char* fired_out_host);

/* Introspection used by tests and the bench. */
typedef struct pe_info {
    int32_t n_streams, n_features, n_mfcc, units, n_layers, ring_slots, carry_capacity;
    int32_t mfcc_precision, gru_precision;
    int64_t device_bytes;            /* HBM held by this engine                                */
} pe_info;
int pe_get_info(const pe_engine* e, pe_info* out);

/* Per-stream streaming state, for tests: q = samples held toward the next frame (may be
 * negative inside the dead zone between windows), frames computed / emitted so far (mod 2^32). */
int pe_get_stream_state(pe_engine* e, int32_t* q_out, uint32_t* computed_out, uint32_t* emitted_out);

/* Test aid.  Each stream's state is a pair of 16-byte records stamped with the number of the engine call that wrote them
 * (csrc/pe_common.h: StreamRec); the 32-bit call count is renumbered in place long before it wraps (default: at 0x7fff0000
 * calls).  This moves the threshold (8..0x7fff0000) so that a test can cross it. */
int pe_set_renumber_at(pe_engine* e, uint32_t call_number);

/* Kernel sequencing of pe_update*: 1 (default) = when chunk_samples <= window - min(window,
 * n_fft) -- no frame computed by an update can become visible in the same update -- the MFCC
 * and network roles run concurrently inside ONE launch (networks with a fused instantiation:
 * gru_precision 0 / 1 on the stock front-end shape); 0 = always two dependent launches. */
int pe_set_fused(pe_engine* e, int32_t enabled);

/* Input projections: 1 = the MFCC stage stores x.W + b of every frame beside its feature row (256 bytes per frame and
 * stream) and the network starts each timestep from that row instead of recomputing the projection in each of the
 * n_features windows a frame appears in (16 of its 41 MFMAs per timestep); 0 = recompute (the default: measured, the
 * rows cost more to load every timestep than the MFMAs they save, profiles/DESIGN_notebook_r1-r5.md 4.6).  Available for the float32
 * network of 17..20 units without delta features.  Both settings agree to float32 rounding (different summation
 * order), each is deterministic; changing the setting restarts all streams. */
int pe_set_input_projection(pe_engine* e, int32_t enabled);

/* Network kernel shape: 0 (default) = automatic -- four waves share each 16-stream tile while the engine has few
 * tiles (stock width 17..20 units, re-tiled: up to 2 tiles per compute unit = 8192 streams on MI355X, the
 * critical-wave kernel, use_delta included; other widths: up to 1 tile per compute unit, and use_delta on the
 * one-wave kernel), one wave per tile beyond -- 1 / 4 = forced: results are bit-identical. */
int pe_set_gru_waves(pe_engine* e, int32_t waves_per_tile);

/* Form of the float32 network (model.py:76-82), -1 (default) = automatic by engine size:
 *   0 = the classic four output tiles on v_mfma_f32_16x16x4_f32;
 *   1 = stock width (17..20 units) re-tiled: three full MFMA tiles + partial sums for units 16..19 (csrc/gru_cw_device.h:
 *       shortens the four-wave kernel's timestep); automatic while the engine has no more than two tiles per compute unit;
 *   2 = float32 products on the bf16 matrix pipe (csrc/gru_x3_device.h): every operand as three bf16 pieces that add up
 *       to the float32 value exactly, six piece products per multiplication, float32 accumulate / gates / state -- the
 *       float32 tolerance, at the float32 kernels' distance to a float64 evaluation.  <= 20 units, <= 15 inputs, no
 *       use_delta (PE_ERR_UNSUPPORTED otherwise).  On gfx950 an f32-input MFMA keeps its whole SIMD from issuing while
 *       it runs and a bf16 MFMA does not; automatic for engines with more stream tiles than the machine has SIMDs (more
 *       than four per compute unit: above 16 384 streams on MI355X), where it takes two launches per update instead of
 *       the fused one and is still faster.
 * Every kernel shape of ONE form agrees bit for bit (pe_update / pe_update_many / pe_predict / pe_evaluate, one or four
 * waves, fused or not); the forms agree to float32 summation order (<= 1e-6 on the probability).  Ignored with projection
 * rows; use_delta models of the stock width follow 0 / 1.
 * Wide / stacked networks (33..256 units) have two forms: 0 (and -1, the default) = the streamed-weight kernel on f32-input MFMAs
 * (csrc/gru_wide_device.h), 2 = float32 products on the bf16 pipe with the float32 weight stream split into three bf16 pieces in
 * registers, on the matrix pipe, every timestep (csrc/gru_wide_x3_device.h): same tolerance, measured EQUAL in time at 256 x 2
 * units (five 4-pass MFMAs + twelve vector instructions against four 8-pass MFMAs per tile and 16 source units), kept as the
 * form whose matrix time would shrink with a narrower weight stream; 1 is refused.
 * bf16-operand networks (gru_precision = 1) have two layouts of the same arithmetic contract (tolerance 1e-2, each bit-stable
 * across pe_update / pe_update_many / pe_predict): 1 (and -1, the default, where it fits: <= 20 units, <= 14 features) = five
 * gate values per lane (csrc/gru_b20_device.h: 9 MFMAs per timestep), 0 = eight values per lane (csrc/gru_bf16_device.h: 12
 * MFMAs, every width up to 32); 2 is refused.
 * Wide / stacked bf16-operand networks (gru_precision = 1, 33..256 units or two layers; csrc/gru_wide_bf16_device.h) have ONE
 * form: 0 is accepted, every other value is PE_ERR_UNSUPPORTED with a message that names the forms.
 * pe_get_gru_tiling: the form this engine's launches take now (0 / 1 / 2; -2 for a null engine). */
int pe_set_gru_tiling(pe_engine* e, int32_t tiling);
int pe_get_gru_tiling(const pe_engine* e);

/* Carried window chains (csrc/gru_chain_device.h).  Consecutive windows of a stream share all but the rows an update makes
 * visible, so an engine may keep, per stream, the GRU state of the chain of every live window start and advance each by those
 * rows (at most two) instead of running all n_features timesteps again -- the same timestep arithmetic in the same order:
 * bit-identical outputs.  mode: 0 = off; 1 (default) = automatic -- after 128 eligible update calls in a row the engine builds
 * the chains from its feature ring (one extra launch) and the following eligible calls advance them; 2 = eager, the first
 * eligible call already (tests).  Eligible: pe_update[_device|_device_keep], pe_update_subset[_device] and pe_update_async of
 * an engine with ONE float32 network of 17..20 units in its re-tiled four-wave form (pe_get_gru_tiling == 1 by the automatic
 * choice, <= 2 stream tiles per compute unit: 8192 streams on MI355X), n_features <= 29, no use_delta, no input-projection
 * rows, a chunk the fused launch takes (<= window - frame length samples) of at most two hops, and none of
 * pe_set_gru_tiling / pe_set_gru_waves / pe_set_fused(0) / pe_set_timing(1) / pe_reserve_updates in force.  Any other call
 * that moves the streams' state or changes the network -- pe_clear (masked too), pe_set_weights, pe_set_vectors,
 * pe_update_many, pe_update_vectors, an update of an ineligible chunk, the knobs above -- simply runs as it always did and
 * leaves the chains invalid; they are built again after the next 128 eligible calls (what the rebuild costs, in updates saved).  The chain state (2560 bytes per stream)
 * is allocated at the first entry: pe_get_info().device_bytes of an engine that never enters does not change.
 * pe_get_chain_carry: *mode = the setting, *active = 1 while the chains are valid (the next eligible call advances them);
 * either pointer may be null. */
int pe_set_chain_carry(pe_engine* e, int32_t mode);
int pe_get_chain_carry(const pe_engine* e, int32_t* mode, int32_t* active);
/* Chains that are never handed out.  An update returns ONE window per stream, so with chunks longer than a hop the window
 * start that an update emitting two rows steps over is never read: 1 - hop / chunk of all starts under a constant chunk (21.9 %
 * at 1024 samples).  After 128 eligible calls in a row with the same chunk > hop the chain launches stop loading, stepping and
 * storing those chains (bit-identical outputs: the chains that are handed out are advanced as before).  The first eligible call
 * with ANOTHER chunk first builds every live chain again from the feature ring (one extra launch, as at entry), the engine
 * stays active throughout, and skipping resumes after the next 128 calls with one chunk.  Subset calls count like full ones:
 * the run and the chunk belong to the engine, a stream that sits out keeps its phase.
 * pe_get_chain_skip: *chunk = the chunk size chains are currently being skipped for, 0 = none (or chains not valid).
 * pe_chain_alive_mask: the predicate itself, pure arithmetic (no engine, no device): for a stream whose record BEFORE an update
 * of `chunk` samples holds q leftover samples, kc computed frames and ke emitted rows, bit A (1 <= A <= T <= 31) of the result
 * says that the chain of age A after that update -- the one started at row ke_after - A -- will be handed out if the chunk
 * holds; bit T is this update's own window.  q is the record's signed leftover, q >= frame_len - hop (negative where a frame is
 * shorter than a hop: the next frame starts beyond the last sample held).  0 for arguments out of range. */
int pe_get_chain_skip(const pe_engine* e, int32_t* chunk);
uint32_t pe_chain_alive_mask(int32_t q, uint32_t kc, uint32_t ke, int32_t chunk, int32_t hop, int32_t frame_len, int32_t window, int32_t T);

/* HIP-event timing of the kernels launched by the last *_device/host update on this engine
 * (milliseconds; measured on the stream the kernels ran on).  Enabled with pe_set_timing(e,1).
 * With a fused launch mfcc_ms is the whole update and gru_ms is 0.
 * pe_vectorize_clips / pe_score_clips: the front-end launch and the network launch of the LAST pass only (every pass records
 * the same events again; one pass unless the audio exceeds the pass target).  pe_vectorize_clips launches no network:
 * gru_ms is 0 there.  pe_evaluate_clips / pe_simulate_clips: likewise the last pass that had a window; the metrics kernels
 * run after the network launch and are not inside either figure. */
int pe_set_timing(pe_engine* e, int32_t enabled);
int pe_get_last_timing(pe_engine* e, float* mfcc_ms, float* gru_ms);

/* Training: precise-train's model.fit (scripts/train.py:159-166) on Sequential[GRU(units, linear, dropout), Dense(1,
 * sigmoid)] compiled with rmsprop and weighted_log_loss (model.py:76-90, functions.py:39-50).  Additive to ABI 8.  A
 * pe_trainer is independent of every pe_engine: it owns the parameters, the RMSprop accumulators and (pe_trainer_set_data) a
 * dataset on ONE device; it is not thread-safe; every entry point takes host pointers and synchronises.  The arithmetic
 * contract -- forward with Keras' per-gate input dropout, loss, backward, RMSprop -- is DESIGN.md 4.9; everything is float32.
 * Scope of pe_trainer_create[_models]: ONE GRU layer of 1..32 units, feature_size 1..32, n_features 1..64; anything else is
 * PE_ERR_UNSUPPORTED naming the field, before any device work (stacked networks and bf16 have no training kernel).
 * pe_trainer_create_wide has the same scope with units 1..256, pe_trainer_create_stacked also takes networks of
 * two GRU layers; see below.
 * Flat parameter order, used for weights, gradients and accumulators alike (Keras layout, gate order z|r|h):
 *   kernel[F][3H] | recurrent_kernel[H][3H] | bias[3H] | dense_kernel[H] | dense_bias      = pe_trainer_n_params floats.
 * PE_ERR_INVALID, before any device work and with the outputs untouched: null pointers, n <= 0, indices outside the dataset,
 * targets outside [0, 1] (NaN included), a dropout rate outside [0, 1).
 * Several networks: a trainer made by pe_trainer_create_models owns n_models (1..PE_TRAIN_MAX_MODELS) networks and trains all
 * of them on the same batch in one launch.  SHARED by the networks of a trainer: n_features, feature_size, the device, the
 * resident training set (pe_trainer_set_data), the resident validation set (pe_trainer_set_validation) and, per call, the
 * batch: indices, n, step.  PER NETWORK: units (1..32), the parameters and accumulators, and every field of pe_train_hparams.
 * The flat vector of such a trainer -- pe_trainer_get_weights / set_weights / get_accumulators -- is the concatenation of
 * the networks' flat vectors in model order, pe_trainer_n_params its length and pe_trainer_n_params_model one network's
 * share.  Bit for bit: a network trained or evaluated next to others gets the losses, probabilities, parameters and
 * accumulators of the same network in a trainer of its own given the same calls -- whatever the other networks' widths,
 * their order and their hyperparameters (every sum runs in an order that depends on neither the launch's width nor on the
 * company).  A trainer of one network IS the n_models = 1 case: pe_trainer_create, pe_trainer_step and pe_trainer_evaluate
 * call the *_models functions; on a trainer of several they, and the inspection calls pe_trainer_loss_grad and
 * pe_trainer_apply, return PE_ERR_UNSUPPORTED.  A per-network complaint of a trainer of several starts "model <index>: ".
 * pe_trainer_last_error(NULL) returns the message of a failed pe_trainer_create[_models] / pe_train_dropout_masks. */
#define PE_TRAIN_MAX_MODELS 16
typedef struct pe_trainer pe_trainer;
int pe_trainer_create(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t device, pe_trainer** out);
/* init[n_models].  n_models < 1 and null weight arrays are PE_ERR_INVALID, n_models > PE_TRAIN_MAX_MODELS is
 * PE_ERR_UNSUPPORTED naming n_models; every refusal happens before any device work. */
int pe_trainer_create_models(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t n_models, int32_t device,
                             pe_trainer** out);
/* pe_trainer_create_models with units 1..256 per network, in any mix of widths; the refusals and their messages are the same
 * with that range.  The handle is an ordinary pe_trainer: every pe_trainer_* entry point, pe_miner_append,
 * pe_generator_append and pe_augmenter_append work on it unchanged.  A network of at most 32 units gets the bits it has in
 * a pe_trainer_create_models trainer.  A network of 33..256 units trains on the f32 matrix cores (csrc/
 * gru_train_wide_device.h) under the same arithmetic contract; its sums run in an order fixed by (n, n_features,
 * feature_size, units) alone, so the same call gives the same bits every time, next to whatever other networks, and
 * pe_trainer_step equals pe_trainer_loss_grad on the gathered rows followed by pe_trainer_apply.  A step keeps its tape on
 * the device: about 20 (units rounded up to 16) + 12 feature_size bytes per sample and timestep. */
int pe_trainer_create_wide(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t n_models, int32_t device,
                           pe_trainer** out);
/* Stacked networks: every one of the n_models networks has ONE or TWO GRU layers, units 1..256 per layer in
 * any mix.  pe_trainer_create, _models and _wide keep refusing n_layers = 2 by name; this constructor is the only way in.
 * A two-layer network is Sequential[GRU(H1, linear, dropout, return_sequences), GRU(H2, linear, dropout), Dense(1, sigmoid)],
 * both layers under the contract of DESIGN.md 4.9, layer 1 reading h1_t under its own per-gate masks [3][n][H1] (the same
 * for every timestep) and handing dx_t back to layer 0's chain.  It always trains on the f32 matrix cores (csrc/
 * gru_train_stacked_device.h), whatever its widths.  A one-layer network gets the bits it has in a pe_trainer_create_wide
 * trainer.  Refusals, before any device work and with the "model <index>: " prefix in a trainer of several: n_layers
 * outside 1..2 and a layer's units outside 1..256 (PE_ERR_UNSUPPORTED naming the field); layers[1].n_in != layers[0].units,
 * layers[0].n_in != feature_size and null arrays (PE_ERR_INVALID).
 * Flat parameter order of a two-layer network, for weights, gradients and accumulators:
 *   kernel_0[F][3H1] | recurrent_kernel_0[H1][3H1] | bias_0[3H1] | kernel_1[H1][3H2] | recurrent_kernel_1[H2][3H2] |
 *   bias_1[3H2] | dense_kernel[H2] | dense_bias.
 * frozen_mask of a two-layer network has three bits, one per layer of the Sequential: bit 0 = GRU 0, bit 1 = GRU 1, bit 2 =
 * Dense; a one-layer network keeps its two.  pe_trainer_loss_grad reads masks_host as [3][n][feature_size] followed by
 * [3][n][H1].  The handle is an ordinary pe_trainer: every pe_trainer_* entry point, pe_miner_append, pe_generator_append
 * and pe_augmenter_append work on it.  Every sum's order is a function of (n, n_features, feature_size, H1, H2) and the
 * element alone and there is no floating-point atomic: the same call gives the same bits every time, next to whatever other
 * networks, and pe_trainer_step equals pe_trainer_loss_grad on the gathered rows with the generated masks followed by
 * pe_trainer_apply.  A step keeps its tape on the device: with H1p, H2p the widths rounded up to 16, 20 H1p + 12 feature_size
 * (layer 0's records) + 20 H2p (layer 1's) + 4 H1p (dx) bytes per sample and timestep. */
int pe_trainer_create_stacked(int32_t n_features, int32_t feature_size, const pe_weights* init, int32_t n_models, int32_t device,
                              pe_trainer** out);
int pe_trainer_destroy(pe_trainer* t);
const char* pe_trainer_last_error(const pe_trainer* t);
int pe_trainer_n_models(const pe_trainer* t);          /* -1 for a null trainer */
int pe_trainer_n_params(const pe_trainer* t);          /* the total over the networks; -1 for a null trainer */
int pe_trainer_n_params_model(const pe_trainer* t, int32_t m);     /* -1 for a null trainer or an m outside 0 .. n_models - 1 */

/* The parameters / the RMSprop accumulators in the flat order.  pe_trainer_set_weights leaves the accumulators as they are;
 * pe_trainer_reset_optimizer zeroes them (a fresh keras.optimizers.RMSprop). */
int pe_trainer_get_weights(pe_trainer* t, float* flat_out);
int pe_trainer_set_weights(pe_trainer* t, const float* flat);
int pe_trainer_get_accumulators(pe_trainer* t, float* flat_out);
int pe_trainer_reset_optimizer(pe_trainer* t);

/* Loss and its gradient for one batch, no state changed: feats[n][n_features][feature_size], targets[n] in [0, 1],
 * masks[3][n][feature_size] the per-gate (z, r, h) input dropout masks of the batch -- each multiplies x_t before that gate's
 * input product, the same for every timestep -- or NULL for no dropout (a two-layer network of pe_trainer_create_stacked:
 * masks[3][n][feature_size] followed by layer 1's masks[3][n][H1]).  loss_out[1] = weighted_log_loss with
 * loss_bias (functions.py:47-50, both means over the n samples of the call), grads_out in the flat order, probs_out[n]
 * (may be NULL) the network outputs under those masks.  The same inputs give the same bits in every call: partial sums are
 * added in a fixed order, no floating-point atomics. */
int pe_trainer_loss_grad(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n, const float* masks_host,
                         float loss_bias, float* loss_out, float* grads_out, float* probs_out);

/* One RMSprop update from given gradients (keras.optimizers.RMSprop: a = rho a + (1 - rho) g^2, theta -= lr g / (sqrt(a) + eps);
 * Keras 2.2.4 defaults lr 1e-3, rho 0.9, eps 1e-7).  frozen_mask: bit 0 = the GRU layer, bit 1 = the Dense layer keep their
 * parameters AND accumulators (model.py:84-85 freeze_till: layers[:freeze_till] -> mask (1 << freeze_till) - 1).  A two-layer
 * network has three bits: GRU 0, GRU 1, Dense. */
int pe_trainer_apply(pe_trainer* t, const float* grads_host, float lr, float rho, float eps, int32_t frozen_mask);

/* model.fit's inner step without leaving the device: pe_trainer_set_data uploads the dataset once
 * (feats[N][n_features][feature_size], targets[N]); pe_trainer_step gathers rows indices[0 .. n), runs forward, backward,
 * the reduction and the RMSprop update, and returns the batch loss.  Dropout masks are generated in the kernel from
 * (seed, step, gate, position in the batch, feature) -- pe_train_dropout_masks below is the same function on the host.
 * Bit for bit: pe_trainer_loss_grad on the gathered rows with those masks, then pe_trainer_apply. */
int pe_trainer_set_data(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n);
int pe_trainer_step(pe_trainer* t, const int32_t* indices_host, int32_t n, float dropout_rate, uint64_t seed, uint64_t step,
                    float loss_bias, float lr, float rho, float eps, int32_t frozen_mask, float* loss_out);

/* The same step for every network of the trainer: the indices are uploaded once, forward + backward of all networks is
 * ONE launch over (tile, network), the reduction + RMSprop of all of them a second, and loss_out[n_models] comes back in one
 * copy.  hp[n_models] holds each network's hyperparameters; network m's masks are those of (hp[m].seed, step).  A dropout
 * rate outside [0, 1) is refused naming the network.  pe_trainer_step is this call on a trainer of one network. */
typedef struct pe_train_hparams {
    float dropout_rate;
    uint64_t seed;
    float loss_bias;
    float lr, rho, eps;
    int32_t frozen_mask;
} pe_train_hparams;
int pe_trainer_step_models(pe_trainer* t, const int32_t* indices_host, int32_t n, uint64_t step, const pe_train_hparams* hp,
                           float* loss_out);

/* A second resident set, for validation: like pe_trainer_set_data, with buffers of its own. */
int pe_trainer_set_validation(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n);

/* model.evaluate / model.predict: dropout off.  loss_out[1], acc_out[1] = mean(round(p) == y) (Keras binary_accuracy),
 * probs_out[n]; each may be NULL.  targets may be NULL when neither loss nor accuracy is asked for. */
int pe_trainer_evaluate(pe_trainer* t, const float* feats_host, const float* targets_host, int32_t n, float loss_bias,
                        float* loss_out, float* acc_out, float* probs_out);

/* The same for every network in one launch: loss_bias[n_models] (may be NULL when loss_out is), loss_out[n_models],
 * acc_out[n_models], probs_out[n_models][n]; each output may be NULL.  source says where the samples are: host data
 * (feats_host / targets_host / n as in pe_trainer_evaluate, uploaded once for all networks), or one of the resident sets --
 * then the host pointers and n are ignored, n is the set's, and nothing but the results crosses the bus: the hits
 * round(p) == y (ties to even) are counted on the device as integers.  A resident set that was never uploaded is
 * PE_ERR_INVALID. */
#define PE_TRAIN_SOURCE_HOST 0
#define PE_TRAIN_SOURCE_DATA 1             /* pe_trainer_set_data */
#define PE_TRAIN_SOURCE_VALIDATION 2       /* pe_trainer_set_validation */
int pe_trainer_n_samples(const pe_trainer* t, int32_t source);     /* of a resident set; 0 if never uploaded, -1 for a null trainer or another source */
int pe_trainer_evaluate_models(pe_trainer* t, int32_t source, const float* feats_host, const float* targets_host, int32_t n,
                               const float* loss_bias, float* loss_out, float* acc_out, float* probs_out);
/* pe_stats_scores (above) over the predictions of every network, which stay on the device: counts_out[n_models][n_thresholds],
 * summary_out[n_models]; the contract is written out at pe_stats_scores. */
int pe_trainer_stats_models(pe_trainer* t, int32_t source, const float* feats_host, const float* targets_host, int32_t n,
                            const double* thresholds, int32_t n_thresholds, int32_t compare,
                            pe_stats_count* counts_out, pe_stats_summary* summary_out, float* probs_out);

/* The dropout masks of one step, on the host (no GPU call; works on a machine without one): out[3][n][feature_size], gate
 * order z, r, h.  With mix(v) the splitmix64 finaliser (v ^= v >> 30; v *= 0xBF58476D1CE4E5B9; v ^= v >> 27;
 * v *= 0x94D049BB133111EB; v ^= v >> 31), G = 0x9E3779B97F4A7C15 and every operation modulo 2^64:
 *   key  = mix(mix(seed + G) ^ (step + G))
 *   ctr  = (i << 7) | (gate << 5) | f                 i = position in the batch, f = feature
 *   bits = mix(key + G (ctr + 1))
 * and element (gate, i, f) is kept iff (float)(bits >> 40) / 2^24 >= rate (both float32; the quotient is exact).  A kept
 * element is 1 / (1 - rate) evaluated in float32, a dropped one 0. */
int pe_train_dropout_masks(uint64_t seed, uint64_t step, int32_t n, int32_t feature_size, float rate, float* out);
/* The masks of one layer of a stacked network, out[3][n][width].  layer 0 (width 1..32) is pe_train_dropout_masks, byte for
 * byte.  layer 1 (width = H1, 1..256) uses the same mix, G and keep rule with
 *   key_1 = mix(key ^ G)
 *   ctr   = (i << 10) | (gate << 8) | f               f < 256
 *   bits  = mix(key_1 + G (ctr + 1)).
 * Any other layer is PE_ERR_INVALID. */
int pe_train_dropout_masks_layer(uint64_t seed, uint64_t step, int32_t layer, int32_t n, int32_t width, float rate, float* out);

/* A resident set that grows (TrainData.merge of scripts/train_incremental.py:101-102 without a new upload of what is already
 * there).  source = PE_TRAIN_SOURCE_DATA or PE_TRAIN_SOURCE_VALIDATION.
 * pe_trainer_append: n more samples behind the set's own (an empty / never uploaded set becomes these n samples); the samples
 * already resident keep their bits and their indices.  Checks as pe_trainer_set_data makes them.
 * pe_trainer_get_data: samples [first, first + n) of the set, feats_out[n][n_features][feature_size] and targets_out[n] (each
 * may be NULL); a range outside the set is PE_ERR_INVALID. */
int pe_trainer_append(pe_trainer* t, int32_t source, const float* feats_host, const float* targets_host, int32_t n);
int pe_trainer_get_data(pe_trainer* t, int32_t source, int32_t first, int32_t n, float* feats_out, float* targets_out);

/* Sampled training: precise-train-sampled (scripts/train_sampled.py:54-90) predicts its WHOLE training set every cycle, adds at
 * most num_sample_chunk samples the model still gets wrong to a growing selection and fits on the selection only; precise-train
 * -sf FILE [-is] (scripts/train.py:146-157) then trains on that selection or on its complement.  Here the set is resident, the
 * choice is made next to the predictions and a fit reads the chosen rows by index: a cycle uploads nothing.  Additive to ABI 8.
 *
 * pe_trainer_evaluate_indices: pe_trainer_evaluate_models' outputs (loss_out[n_models], acc_out[n_models], probs_out[n_models][n];
 *   each may be NULL) for rows indices_host[0 .. n) of the resident set `source` (PE_TRAIN_SOURCE_DATA or _VALIDATION), in that
 *   order; repeats allowed.  Bit for bit pe_trainer_evaluate_models(PE_TRAIN_SOURCE_HOST) on host copies of those rows.  An index
 *   outside the set is PE_ERR_INVALID before any device work; the outputs are then untouched.
 *
 * The selection state belongs to the training set: per row `eligible` and `selected`, and the list of the selected rows in the
 * order they were chosen.  pe_trainer_set_data empties it (nothing selected, every row eligible); rows that pe_trainer_append
 * (or a miner / generator / augmenter) adds are eligible and unselected.
 * pe_trainer_sample_reset replaces it: eligible_host[n] (non-zero = eligible; NULL = all) and selected_host[n_selected], the
 *   selection in order.  An index outside the set, a repeated index or an ineligible selected row is PE_ERR_INVALID and leaves
 *   the state as it was.  `eligible` is how duplicated samples are handled: the reference keys samples by an md5 of their bytes
 *   and its hash_to_ind keeps the LAST row of every hash, so the caller marks exactly those rows eligible (hashing stays on the
 *   host); identical rows predict identical bits, so a duplicate fails exactly when its eligible twin does.
 * pe_trainer_sample_choose: ONE device call.  (1) the evaluate launch over the whole training set, dropout off; the predictions
 *   p of network `model` stay on the device.  (2) per row fail = (p > 0.5f) != (y > 0.5f) (a NaN p compares false, as numpy's
 *   does), candidate = fail && eligible && !selected; the counts are integers.  (3) the first max_new candidates in `order`:
 *     PE_SAMPLE_ORDER_INDEX   lowest row first -- the reference's loop with sorted(remaining, key=hash_to_ind.get) in front of
 *                             its islice (which otherwise follows Python's set order: it has no reproducible order to match);
 *     PE_SAMPLE_ORDER_ERROR   largest float32 |p - y| first (fabsf of one correctly rounded subtraction; a NaN counts as
 *                             +infinity), ties to the lower row -- "the highest loss" of the script's docstring.
 *   The order is a unique 64-bit key per row and the choice its max_new smallest keys, found by sorting (no atomics decide a
 *   position): the same call on the same state gives the same ids in the same order.  (4) the chosen rows are marked selected
 *   and appended to the selection list; *report and added_out[n_added] (may be NULL) come back in one copy, probs_out[n] (may
 *   be NULL) in a second.  max_new = 0 reports only.  max_new > PE_SAMPLE_MAX_NEW is PE_ERR_UNSUPPORTED (the message names
 *   max_new); model outside the trainer, an unknown order, a negative max_new or no resident training set PE_ERR_INVALID; all
 *   checks happen before any device work.
 * pe_trainer_sample_selected: out[pe_trainer_n_selected(t)], the selection in the order chosen.
 * The samples file itself (hashes, one per selected row) is the host's business: train.py writes a JSON array of hash strings;
 * that the reference's fitipy writer produces exactly that was not verified. */
#define PE_SAMPLE_ORDER_INDEX 0
#define PE_SAMPLE_ORDER_ERROR 1
#define PE_SAMPLE_MAX_NEW 1024
#define PE_SAMPLE_BLOCK_ROWS 2048           /* rows one selection block owns (tests place failing rows at its borders) */
typedef struct pe_sample_report {
    int64_t n;            /* rows of the resident training set */
    int64_t n_correct;    /* rows with (p > 0.5) == (y > 0.5), over ALL rows */
    int64_t n_failed;     /* eligible rows that fail */
    int64_t n_remaining;  /* of those, not selected before this call (the script's "Remaining failed samples") */
    int64_t n_added;      /* min(max_new, n_remaining) */
    int64_t n_selected;   /* size of the selection after this call */
} pe_sample_report;
int pe_trainer_evaluate_indices(pe_trainer* t, int32_t source, const int32_t* indices_host, int32_t n,
                                const float* loss_bias, float* loss_out, float* acc_out, float* probs_out);
int pe_trainer_sample_reset(pe_trainer* t, const uint8_t* eligible_host /* [n] or NULL = all */,
                            const int32_t* selected_host, int32_t n_selected);
int pe_trainer_sample_choose(pe_trainer* t, int32_t model, int32_t max_new, int32_t order,
                             pe_sample_report* report, int32_t* added_out /* [max_new] or NULL */,
                             float* probs_out /* [n] or NULL */);
int pe_trainer_sample_selected(pe_trainer* t, int32_t* out /* [n_selected], in order of selection */);
int pe_trainer_n_selected(const pe_trainer* t);                    /* -1 for a null trainer */

/* Incremental training: precise-train-incremental (scripts/train_incremental.py:113-137) plays hours of not-wake-word audio
 * through a Listener chunk by chunk, saves the last buffer_t seconds whenever the model fires, and retrains.  A pe_miner is
 * that scan as a session over ONE engine: the recordings are uploaded once and every frame of every recording is computed
 * once, when the session is created (frames do not depend on the model); a scan then scores ALL chunks from a position on in
 * a few launches, and the saved samples go from the resident audio into a trainer's resident set without crossing the bus.
 * Additive to ABI 8.  The session is not thread-safe, uses the engine's device and leaves the engine's streams untouched;
 * destroy it before its engine.
 *
 * Chunks (util.py:30-32): chunk i of a recording is samples [i C, (i + 1) C) for (i + 1) C < len -- a recording of len samples
 * has (len - 1) / C chunks (0 for len = 0), the tail and a last chunk that would end exactly at len are never seen.  The chunks
 * of all recordings in order have GLOBAL ids 0 .. total - 1; pe_miner_layout gives the exclusive prefix sum of the counts.
 * Prediction of a chunk (network_runner.py:125-152 on a listener cleared at the start of the recording, :119): after
 * n = (i + 1) C samples 1 + (n - window) / hop frames have been emitted (0 below one window; one fewer with vectorizer = 3);
 * the network input is the last n_features rows of n_features zero rows followed by those frames (use_delta: with the row
 * differences the engine's streaming path forms).  Frames are float32 rows as the engine's feature window holds them, and the
 * batch goes through pe_predict_device: a scan is bit for bit pe_predict of those windows on this engine.
 * Hit (:125): decode(p) > threshold in float64, strict; decode is model's pe_set_decoder table through pe_decode's kernel when
 * one is set, else (double)p.
 * Saved sample (:79,:123,:130 and util.py:65,71): the float64 ring of buffer_samples samples starts as zeros, takes every chunk
 * and is never cleared -- at a hit it holds the last buffer_samples samples of ALL chunks so far, earlier recordings included
 * (carry_audio = 1; 0: zeros before the hit's own recording).  It is written as int16, q = (int16) trunc(x * 32767.0), and read
 * back as (float32) q / 32767.0f, then vectorized: exactly pe_vectorize_clips of that float32 clip (and its launch).
 *
 * pe_miner_create: audio_host / sample_format / offsets / n_rec as pe_evaluate_clips takes them (zero-length recordings
 *   allowed), checked as it checks them; chunk_size >= 1; buffer_samples >= 1 (ListenerParams.buffer_samples, params.py:74).
 *   PRECONDITION: buffer_samples <= ListenerParams.max_samples (params.py:95; true of every ListenerParams, whose
 *   buffer_samples is max_samples rounded down to whole hops): the saved clip is vectorized WITHOUT vectorize()'s crop, which
 *   pe_params does not carry.  mining.Miner refuses a larger value;
 *   at most 2^31 - 1 chunks and frames per session (PE_ERR_INVALID); PE_ERR_NOMEM when the device cannot hold the session.
 * pe_miner_layout: chunk_offsets_out[n_rec + 1].
 * pe_miner_scan: chunks first_chunk .. total - 1 (first_chunk = total: nothing) of model `model`: scores_out[total -
 *   first_chunk] raw predictions (may be NULL), hits_out[capacity] the ascending global ids of the first `capacity` hits (NULL
 *   with capacity 0), *n_hits = min(capacity, hits), *n_above = all hits of the range.  Runs in passes of
 *   pe_set_clip_pass_bytes bytes of network input (at least one chunk); no result depends on the pass size.  A NaN threshold
 *   is PE_ERR_INVALID.
 * pe_miner_vectorize: feats_out[n][n_features][n_mfcc] float64, the saved sample of every hit as vectorize() returns it
 *   (vectorization.py:62-84).  hits: global ids in any order, repeats allowed; an id outside 0 .. total - 1 is PE_ERR_INVALID.
 * pe_miner_append: the same rows as float32 (use_delta: with the delta columns pe_score_clips forms, vectorization.py:87-89)
 *   appended to the trainer's resident set `source`, device to device, every target = `target` (the script saves under
 *   not-wake-word: 0).  The trainer must live on the engine's device with the engine's n_features and feature_size
 *   (PE_ERR_INVALID); the trainer's own failures are reported on the engine with the trainer's message. */
typedef struct pe_miner pe_miner;
int pe_miner_create(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_rec,
                    int32_t chunk_size, int32_t buffer_samples, int32_t carry_audio, pe_miner** out);
int pe_miner_destroy(pe_miner* m);
int pe_miner_layout(const pe_miner* m, int64_t* chunk_offsets_out);
int pe_miner_scan(pe_miner* m, int32_t model, int64_t first_chunk, double threshold, float* scores_out, int32_t* hits_out,
                  int32_t capacity, int32_t* n_hits, int64_t* n_above);
int pe_miner_vectorize(pe_miner* m, const int32_t* hits, int32_t n, double* feats_out_host);
int pe_miner_append(pe_miner* m, pe_trainer* trainer, int32_t source, const int32_t* hits, int32_t n, float target);

/* Generated training data: precise-train-generated (scripts/train_generated.py:118-237) streams every background recording
 * chunk by chunk through a Listener, overlays volume-normalised wake-word / not-wake-word clips with random gaps on it, and
 * feeds (window, target) pairs to fit_generator.  A pe_generator is that stream as a session over ONE engine: both audio pools
 * are uploaded once; a PLAN -- the script's random draws and its piece stream, flattened by the host (generated.py) into
 * segments -- is mixed on the device and every frame of every planned file is computed once; windows then go to the host or
 * straight behind a trainer's resident set.  Additive to ABI 8.  The session is not thread-safe, uses the engine's device and
 * leaves the engine's streams untouched; destroy it before its engine.
 *
 * Plan: file f overlays background `background` (a background may be planned any number of times); its output is the
 * (len - 1) / C whole chunks of that background (util.py:30-32), and its segments first_segment .. + n_segments -- the files'
 * ranges follow one another without gaps from segment 0 -- tile exactly those n_chunks * C samples in order.  Segment: `length`
 * (>= 1) output samples under which lie samples first .. first + length of clip `clip`, or silence (clip = -1: first, rms
 * ignored).  `target` is the host's business (labels come from run lengths over the segments) and is not read.
 * Arithmetic of an output sample, numpy's to the bit (:149-155, with s the background and c the clip sample, all float32):
 *   b = fl32(fl32(fl32(audio_volume) * s) / fl32(file rms));  w = (double) fl32(fl32(fl32(volume) * c) / fl32(segment rms)), 0.0
 *   in silence;  out = (double) fl32(fl32(1.0 - 0.6) * b) + 0.6 * w, the last product and the sum in float64.
 * The planner sets a segment's volume to its file's audio_volume (:182); the device reads the file's.
 * Chunks of all files in order have GLOBAL ids 0 .. total - 1, as pe_miner's.  The network input after chunk i of a file is what
 * a Listener cleared at the start of the file (:180) holds after i + 1 chunks of the mixed samples: pe_miner's window, zero rows
 * before the file's first frame.  With use_delta the delta columns are formed as pe_miner_scan forms them; the reference yields
 * the bare window (:188,202) and so cannot train a use_delta model this way at all.
 *
 * pe_generator_create: float32 pools (what load_audio returns) with offsets[n + 1] each, checked as pe_miner_create checks its
 *   offsets (empty entries allowed); chunk_size >= 1.
 * pe_generator_set_plan: replaces the resident plan.  Everything is checked on the host first -- a background or clip index out
 *   of range, a segment outside its clip, a length < 1, a file rms that is not > 0 (files with chunks) or a segment rms that is
 *   not > 0, segment ranges that do not follow one another, a file whose segment lengths do not sum to n_chunks * chunk_size,
 *   more than 2^31 - 1 chunks, frames or segments: PE_ERR_INVALID naming the file or segment, and the plan that was resident
 *   stays.  Then the files are mixed and their frames computed in passes of pe_set_clip_pass_bytes bytes of mixed float64
 *   samples over whole files (a larger file runs alone); no result depends on the pass size.
 * pe_generator_audio: out_host[n] = mixed samples first .. first + n of planned file `file` (the mix is run again for them).
 * pe_generator_vectorize: feats_out_host[n][n_features][width] float32, width = feature_size (n_mfcc, doubled by use_delta).
 *   ids: global chunk ids in any order, repeats allowed; one outside the plan is PE_ERR_INVALID.
 * pe_generator_append: the same rows behind the trainer's resident set `source`, device to device, sample i with targets[i];
 *   trainer, device and shape checks as pe_miner_append's, every target in [0, 1] (PE_ERR_INVALID naming the index). */
typedef struct pe_generator pe_generator;
typedef struct pe_gen_file {
    int32_t background;
    int32_t reserved;
    double audio_volume;    /* rms * (0.4 + 0.5 u) */
    double rms;             /* of the background */
    int64_t first_segment;
    int64_t n_segments;
} pe_gen_file;
typedef struct pe_gen_segment {
    int32_t clip;           /* -1: silence */
    int32_t target;
    int64_t first;
    int64_t length;
    double volume;
    double rms;             /* of the clip */
} pe_gen_segment;
int pe_generator_create(pe_engine* e, const float* bg_audio, const int64_t* bg_offsets, int32_t n_bg, const float* clip_audio,
                        const int64_t* clip_offsets, int32_t n_clips, int32_t chunk_size, pe_generator** out);
int pe_generator_destroy(pe_generator* g);
int pe_generator_set_plan(pe_generator* g, const pe_gen_file* files, int32_t n_files, const pe_gen_segment* segments, int64_t n_segments);
int pe_generator_audio(pe_generator* g, int32_t file, int64_t first, int64_t n, double* out_host);
int pe_generator_vectorize(pe_generator* g, const int32_t* ids, int32_t n, float* feats_out_host);
int pe_generator_append(pe_generator* g, pe_trainer* trainer, int32_t source, const int32_t* ids, const float* targets, int32_t n);

/* Noise augmentation: precise-add-noise (scripts/add_noise.py:56-90) makes inflation_factor noisy copies of every clip of a
 * dataset -- a cursor walks through a pool of noise recordings, the noise under a copy is scaled to the clip's energy and mixed
 * in at a random ratio, the result is saved as an int16 wav -- and training reads the copies back through load_audio and
 * vectorize.  A pe_augmenter is that loop as a session over ONE engine: the clip pool and the noise pool are uploaded once; a
 * PLAN -- the cursor and the draws, replayed by the host (augment.py) into copies and pieces -- is mixed on the device, and the
 * reloaded copies go through pe_vectorize_clips' front-end launch to the host or straight behind a trainer's resident set.
 * Additive to ABI 8.  The session is not thread-safe, uses the engine's device and leaves the engine's streams untouched;
 * destroy it before its engine.
 *
 * Plan: copy o is a noisy version of clip `clip` at ratio `ratio`; its pieces first_piece .. + n_pieces -- the copies' ranges
 * follow one another without gaps from piece 0 -- tile the clip's samples in order: piece = `length` (>= 1) consecutive output
 * samples under which lie samples first .. first + length of noise recording `noise`.
 * Arithmetic (add_noise.py:66-90, util.py:65,71), every product and sum rounded exactly once.  a[i]: the clip's float32 samples;
 * n[i]: the noise samples under the copy, float32 widened to double (get_fresh_noise concatenates onto np.empty(0): float64);
 * r: the ratio, a double.
 *   S_a = sum(audio ** 2), Python's sum over a float32 array: the float32 left-to-right chain s = fl32(s + fl32(a[i] a[i])), i
 *         ascending, from 0;  va = sqrt((double) S_a).
 *   S_n = sum(noise_data ** 2): the float64 left-to-right chain over the copy's noise samples in piece order (the square of a
 *         float32 is exact in double);  vn = sqrt(S_n).
 *   adj    = (va * n[i]) / vn, two float64 roundings in that order;
 *   out[i] = r * adj + (double) fl32(fl32(1.0 - r) * a[i]): 1.0 - r is formed in double and rounded to float32 when it meets the
 *            float32 array; the first product and the sum are float64;
 *   saved and reloaded: q = (int16_t)(int)(out[i] * 32767.0), training sample fl32(q) / 32767.0f.
 * Both sums are sequential chains on the device too, one lane per chain: the scale va / vn feeds a truncation to int16, and
 * another summation order would flip isolated samples by one step.
 * Where the reference is undefined: vn == 0 (all-zero noise under a copy; NaN in the reference) is flagged by the device and
 * refused by pe_augmenter_set_plan; |out[i] * 32767| >= 32768 is an out-of-range cast (undefined in C, the device gives what
 * (int16_t)(int) gives) and is counted per copy (`overflowed`), so a caller can reject those copies; an empty clip (the reference
 * writes an empty wav) or an empty noise recording (the reference loops forever on an all-empty pool) is refused at creation.
 *
 * pe_augmenter_create: float32 pools (what load_audio returns) with offsets[n + 1] each; at least one clip and one noise
 *   recording, none of them empty: PE_ERR_INVALID naming the clip or the recording.  S_a of every clip is computed here.
 *   A NULL engine makes a session without a device that checks plans only: pe_augmenter_set_plan runs its host checks and keeps
 *   the plan's shape, every other entry point is PE_ERR_INVALID, and messages go to pe_last_global_error.
 * pe_augmenter_set_plan: replaces the resident plan.  Everything is checked on the host first -- a clip, noise or piece index out
 *   of range, a piece outside its recording, a length < 1, a copy whose piece lengths do not sum to its clip's length, piece
 *   ranges that do not follow one another, a ratio that is NaN, more than 2^31 - 1 copies or pieces: PE_ERR_INVALID naming the
 *   copy or piece.  Then S_n of every copy is computed; a copy with vn == 0 is PE_ERR_INVALID naming the copy.  Either way the
 *   plan that was resident stays.
 * pe_augmenter_volumes: clip_volume[n_clips] = va, noise_volume[n_copies] = vn, overflowed[n_copies] = samples of the copy with
 *   |out * 32767| >= 32768 (the mix is run once over the plan to count them); each may be NULL.
 * pe_augmenter_audio: mixed_out[len] = out, pcm_out[len] = q of copy `copy` (len: its clip's length); each may be NULL.
 * pe_augmenter_vectorize: feats_out_host[n][n_features][width] float32, width = feature_size (n_mfcc, doubled by use_delta):
 *   vectorize() (vectorization.py:62-84: the last max_samples samples, max_samples <= 0 = no crop) of the reloaded copy ids[i]
 *   -- pe_vectorize_clips' rows, rounded to float32 as the trainer holds them, with use_delta the delta columns as
 *   pe_miner_append forms them.  ids: copies in any order, repeats allowed; one outside the plan is PE_ERR_INVALID.
 * pe_augmenter_append: the same rows behind the trainer's resident set `source`, device to device, sample i with targets[i];
 *   trainer, device and shape checks as pe_miner_append's, every target in [0, 1] (PE_ERR_INVALID naming the index).
 * The mix, the front end and the append run in passes of pe_set_clip_pass_bytes bytes of mixed samples over whole copies (at
 * least one copy per pass); no result depends on the pass size, and nothing per sample stays resident but the two pools. */
typedef struct pe_augmenter pe_augmenter;
typedef struct pe_aug_copy {
    int32_t clip;
    int32_t reserved;
    double ratio;           /* low + (high - low) u */
    int64_t first_piece;
    int64_t n_pieces;
} pe_aug_copy;
typedef struct pe_aug_piece {
    int32_t noise;
    int32_t reserved;
    int64_t first;
    int64_t length;
} pe_aug_piece;
int pe_augmenter_create(pe_engine* e, const float* clip_audio, const int64_t* clip_offsets, int32_t n_clips, const float* noise_audio,
                        const int64_t* noise_offsets, int32_t n_noise, pe_augmenter** out);
int pe_augmenter_destroy(pe_augmenter* g);
int pe_augmenter_set_plan(pe_augmenter* g, const pe_aug_copy* copies, int32_t n_copies, const pe_aug_piece* pieces, int64_t n_pieces);
int pe_augmenter_volumes(pe_augmenter* g, double* clip_volume, double* noise_volume, int64_t* overflowed);
int pe_augmenter_audio(pe_augmenter* g, int32_t copy, double* mixed_out, int16_t* pcm_out);
int pe_augmenter_vectorize(pe_augmenter* g, const int32_t* ids, int32_t n, int64_t max_samples, float* feats_out_host);
int pe_augmenter_append(pe_augmenter* g, pe_trainer* trainer, int32_t source, const int32_t* ids, const float* targets, int32_t n,
                        int64_t max_samples);

#ifdef __cplusplus
}
#endif
#endif /* PRECISE_ENGINE_H */
