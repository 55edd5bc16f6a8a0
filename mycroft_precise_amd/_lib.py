"""
ctypes binding of libprecise_engine.so (C ABI: include/precise_engine.h).

There is NO CPU fallback: if the HIP library is missing or a call fails this module raises.
"""
import ctypes as C
import importlib.util
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# PE_LIB: load another build of the library (an A/B against an older tree) instead of the in-tree one
LIB_PATH = os.environ.get('PE_LIB') or os.path.join(HERE, 'libprecise_engine.so')

PE_OK, PE_ERR_INVALID, PE_ERR_HIP, PE_ERR_UNSUPPORTED, PE_ERR_NOMEM, PE_ERR_EOF = range(6)
ABI_VERSION = 8


class PeParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        'sample_rate', 'window_samples', 'hop_samples', 'n_fft', 'n_filt', 'n_mfcc', 'n_features',
        'use_delta', 'mfcc_precision', 'gru_precision', 'vectorizer', 'ring_precision')]


class PeGruLayer(C.Structure):
    _fields_ = [('n_in', C.c_int32), ('units', C.c_int32),
                ('kernel', C.POINTER(C.c_float)), ('recurrent_kernel', C.POINTER(C.c_float)),
                ('bias', C.POINTER(C.c_float))]


class PeWeights(C.Structure):
    _fields_ = [('n_layers', C.c_int32), ('layers', C.POINTER(PeGruLayer)),
                ('dense_kernel', C.POINTER(C.c_float)), ('dense_bias', C.c_float)]


class PeTrainHparams(C.Structure):
    """pe_train_hparams: one network's hyperparameters of a training step"""
    _fields_ = [('dropout_rate', C.c_float), ('seed', C.c_uint64), ('loss_bias', C.c_float), ('lr', C.c_float),
                ('rho', C.c_float), ('eps', C.c_float), ('frozen_mask', C.c_int32)]


TRAIN_MAX_MODELS = 16                                                  # PE_TRAIN_MAX_MODELS
TRAIN_SOURCE_HOST, TRAIN_SOURCE_DATA, TRAIN_SOURCE_VALIDATION = 0, 1, 2     # PE_TRAIN_SOURCE_*


class PeSampleReport(C.Structure):
    """pe_sample_report: what pe_trainer_sample_choose counted and did"""
    _fields_ = [(n, C.c_int64) for n in ('n', 'n_correct', 'n_failed', 'n_remaining', 'n_added', 'n_selected')]


SAMPLE_ORDER = {'index': 0, 'error': 1}                                # PE_SAMPLE_ORDER_*
SAMPLE_MAX_NEW, SAMPLE_BLOCK_ROWS = 1024, 2048                         # PE_SAMPLE_MAX_NEW, PE_SAMPLE_BLOCK_ROWS


class PeInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        'n_streams', 'n_features', 'n_mfcc', 'units', 'n_layers', 'ring_slots', 'carry_capacity',
        'mfcc_precision', 'gru_precision')] + [('device_bytes', C.c_int64)]


EXPORTS = {
    # name: (restype, argtypes)
    'pe_abi_version': (C.c_int, []),
    'pe_last_global_error': (C.c_char_p, []),
    'pe_create': (C.c_int, [C.POINTER(PeParams), C.POINTER(C.c_double), C.POINTER(PeWeights), C.c_int32,
                            C.c_int32, C.POINTER(C.c_void_p)]),
    'pe_create_models': (C.c_int, [C.POINTER(PeParams), C.POINTER(C.c_double), C.POINTER(PeWeights), C.c_int32, C.c_int32,
                                   C.c_int32, C.POINTER(C.c_void_p)]),
    'pe_get_n_models': (C.c_int, [C.c_void_p]),
    'pe_set_weights': (C.c_int, [C.c_void_p, C.POINTER(PeWeights), C.c_int32]),
    'pe_destroy': (C.c_int, [C.c_void_p]),
    'pe_last_error': (C.c_char_p, [C.c_void_p]),
    'pe_clear': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_update': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'pe_update_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_update_device_keep': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_update_subset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    'pe_update_subset_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_set_renumber_at': (C.c_int, [C.c_void_p, C.c_uint32]),
    'pe_host_alloc': (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    'pe_host_free': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_update_async': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'pe_wait': (C.c_int, [C.c_void_p]),
    'pe_update_subset_async': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_reserve_updates': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'pe_update_many': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'pe_update_many_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_update_vectors': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'pe_update_vectors_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_get_vectors': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_set_vectors': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_run_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_predict': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'pe_predict_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_vectorize_raw': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                   C.POINTER(C.c_int64)]),
    'pe_vectorize_mels': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                   C.POINTER(C.c_int64)]),
    'pe_evaluate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                              C.POINTER(C.c_int64)]),
    'pe_vectorize_clips': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
    'pe_score_clips': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    'pe_set_clip_pass_bytes': (C.c_int, [C.c_void_p, C.c_int64]),
    'pe_evaluate_clips_layout': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'pe_evaluate_clips': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    'pe_simulate_scores': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_simulate_clips': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    'pe_stats_scores': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_void_p]),
    'pe_test_clips': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_set_decoder': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    'pe_set_trigger': (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int32]),
    'pe_set_decoder_model': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    'pe_set_trigger_model': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32]),
    'pe_decode_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_decode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_decode_subset_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_decode_subset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_get_info': (C.c_int, [C.c_void_p, C.POINTER(PeInfo)]),
    'pe_get_stream_state': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_set_fused': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_set_gru_waves': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_set_gru_tiling': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_get_gru_tiling': (C.c_int, [C.c_void_p]),
    'pe_set_input_projection': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_set_timing': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_set_chain_carry': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_get_chain_carry': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'pe_get_chain_skip': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    'pe_chain_alive_mask': (C.c_uint32, [C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'pe_get_last_timing': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    # training (pe_trainer)
    'pe_trainer_create': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(PeWeights), C.c_int32, C.POINTER(C.c_void_p)]),
    'pe_trainer_destroy': (C.c_int, [C.c_void_p]),
    'pe_trainer_last_error': (C.c_char_p, [C.c_void_p]),
    'pe_trainer_n_params': (C.c_int, [C.c_void_p]),
    'pe_trainer_get_weights': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_trainer_set_weights': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_trainer_get_accumulators': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_trainer_reset_optimizer': (C.c_int, [C.c_void_p]),
    'pe_trainer_loss_grad': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    'pe_trainer_apply': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int32]),
    'pe_trainer_set_data': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    'pe_trainer_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_float, C.c_float,
                                  C.c_float, C.c_float, C.c_int32, C.c_void_p]),
    'pe_trainer_evaluate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_trainer_create_models': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(PeWeights), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'pe_trainer_create_wide': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(PeWeights), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'pe_trainer_create_stacked': (C.c_int, [C.c_int32, C.c_int32, C.POINTER(PeWeights), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'pe_trainer_n_models': (C.c_int, [C.c_void_p]),
    'pe_trainer_n_params_model': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_trainer_step_models': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(PeTrainHparams), C.c_void_p]),
    'pe_trainer_n_samples': (C.c_int, [C.c_void_p, C.c_int32]),
    'pe_trainer_set_validation': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    'pe_trainer_evaluate_models': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    'pe_trainer_stats_models': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_train_dropout_masks': (C.c_int, [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    'pe_train_dropout_masks_layer': (C.c_int, [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    'pe_trainer_append': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]),
    'pe_trainer_get_data': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    # sampled training (pe_trainer_sample_*)
    'pe_trainer_evaluate_indices': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    'pe_trainer_sample_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    'pe_trainer_sample_choose': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PeSampleReport), C.c_void_p,
                                           C.c_void_p]),
    'pe_trainer_sample_selected': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_trainer_n_selected': (C.c_int, [C.c_void_p]),
    # mining false activations (pe_miner)
    'pe_miner_create': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.POINTER(C.c_void_p)]),
    'pe_miner_destroy': (C.c_int, [C.c_void_p]),
    'pe_miner_layout': (C.c_int, [C.c_void_p, C.c_void_p]),
    'pe_miner_scan': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                                C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'pe_miner_vectorize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'pe_miner_append': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float]),
    # generated training data (pe_generator)
    'pe_generator_create': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.POINTER(C.c_void_p)]),
    'pe_generator_destroy': (C.c_int, [C.c_void_p]),
    'pe_generator_set_plan': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    'pe_generator_audio': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
    'pe_generator_vectorize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'pe_generator_append': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]),
    # noise augmentation (pe_augmenter)
    'pe_augmenter_create': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    'pe_augmenter_destroy': (C.c_int, [C.c_void_p]),
    'pe_augmenter_set_plan': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    'pe_augmenter_volumes': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pe_augmenter_audio': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pe_augmenter_vectorize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    'pe_augmenter_append': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
}

# pe_gen_file / pe_gen_segment: the tables of pe_generator_set_plan
GEN_FILE = np.dtype([('background', '<i4'), ('reserved', '<i4'), ('audio_volume', '<f8'), ('rms', '<f8'), ('first_segment', '<i8'),
                     ('n_segments', '<i8')])
GEN_SEGMENT = np.dtype([('clip', '<i4'), ('target', '<i4'), ('first', '<i8'), ('length', '<i8'), ('volume', '<f8'), ('rms', '<f8')])

# pe_aug_copy / pe_aug_piece: the tables of pe_augmenter_set_plan
AUG_COPY = np.dtype([('clip', '<i4'), ('reserved', '<i4'), ('ratio', '<f8'), ('first_piece', '<i8'), ('n_pieces', '<i8')])
AUG_PIECE = np.dtype([('noise', '<i4'), ('reserved', '<i4'), ('first', '<i8'), ('length', '<i8')])

# pe_sim_metric: one (model, recording) of pe_simulate_scores / pe_simulate_clips
SIM_METRIC = np.dtype([('n_windows', '<i8'), ('activated_chunks', '<i8'), ('activations', '<i8'), ('activation_sum', '<f8')])



class PeStatsCount(C.Structure):
    """pe_stats_count: one (row, threshold) of pe_stats_scores / pe_test_clips / pe_trainer_stats_models"""
    _fields_ = [(n, C.c_int64) for n in ('pos_gt', 'neg_gt', 'pos_ge', 'neg_ge')]


class PeStatsSummary(C.Structure):
    """pe_stats_summary: one row of those calls"""
    _fields_ = [(n, C.c_int64) for n in ('n', 'n_pos', 'n_neg', 'n_other', 'n_nan', 'n_unsaturated', 'n_fit')] + \
        [('logit_mean', C.c_double), ('logit_std', C.c_double)]


STATS_COUNT, STATS_SUMMARY = np.dtype(PeStatsCount), np.dtype(PeStatsSummary)
STATS_MAX_ROWS, STATS_MAX_THRESHOLDS = 16, 4096
STATS_COMPARE = {'f32': 0, 'f64': 1}                                   # PE_STATS_COMPARE_*


def stats_request(thresholds, compare):
    """-> (float64 thresholds [T], compare code) of a statistics call, refused here -- before any call into the library --
    with ValueError when the table is not 1-D, holds a NaN, decreases or is longer than 4096, or ``compare`` is neither
    'f32' nor 'f64'."""
    if compare not in STATS_COMPARE:
        raise ValueError("compare must be 'f32' or 'f64', got %r" % (compare,))
    thr = np.zeros(0) if thresholds is None else np.array(thresholds, dtype=np.float64, ndmin=1)
    if thr.ndim != 1:
        raise ValueError('thresholds must be a 1-D table, got shape %r' % (thr.shape,))
    if thr.size > STATS_MAX_THRESHOLDS:
        raise ValueError('at most %d thresholds per call, got %d' % (STATS_MAX_THRESHOLDS, thr.size))
    if np.isnan(thr).any():
        raise ValueError('thresholds[%d] is NaN' % int(np.flatnonzero(np.isnan(thr))[0]))
    if thr.size > 1 and (np.diff(thr) < 0).any():
        raise ValueError('thresholds decrease at %d' % (int(np.flatnonzero(np.diff(thr) < 0)[0]) + 1))
    return np.ascontiguousarray(thr), STATS_COMPARE[compare]


def _stats_out(rows, n_thresholds):
    """zeroed outputs of a statistics call: (counts STATS_COUNT [rows, T], summary STATS_SUMMARY [rows])"""
    return np.zeros((rows, n_thresholds), dtype=STATS_COUNT), np.zeros(rows, dtype=STATS_SUMMARY)


_lib = None


class HipLibraryMissing(ImportError):
    pass


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process do not share devices pointers or streams, so when torch is installed
    its copy is loaded first and libprecise_engine.so binds to it -- whatever the import order."""
    if os.environ.get('PRECISE_AMD_HIP_RUNTIME', '') == 'system':
        return
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    """Load (once) and return the bound library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            'libprecise_engine.so is not built (expected at %s). Build it with '
            '`python -m mycroft_precise_amd._build`; there is no CPU fallback.' % LIB_PATH)
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)       # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.pe_abi_version() != ABI_VERSION:
        raise HipLibraryMissing('libprecise_engine.so ABI %d != expected %d; rebuild' %
                                (lib.pe_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('precise_engine error %d: %s' % (code, msg))
        self.code = code


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _pe_weights(wm, check_dense=True):
    """one weights dict -> (PeWeights, the numpy / ctypes objects its pointers refer to: keep them alive across the call)"""
    layers = wm['gru']
    arr = (PeGruLayer * len(layers))()
    keep = [arr]
    for i, (k, rk, b) in enumerate(layers):
        k = np.ascontiguousarray(k, dtype=np.float32)
        rk = np.ascontiguousarray(rk, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        units = rk.shape[0]
        if k.ndim != 2 or k.shape[1] != 3 * units or rk.shape != (units, 3 * units) or b.shape != (3 * units,):
            raise ValueError('GRU layer %d has inconsistent shapes' % i)
        keep += [k, rk, b]
        arr[i] = PeGruLayer(k.shape[0], units, _fptr(k), _fptr(rk), _fptr(b))
    dk = np.ascontiguousarray(wm['dense_kernel'], dtype=np.float32).reshape(-1)
    if check_dense and dk.size != np.shape(layers[-1][1])[0]:
        raise ValueError('dense_kernel has %d entries for %d units' % (dk.size, np.shape(layers[-1][1])[0]))
    db = float(np.asarray(wm['dense_bias'], dtype=np.float32).reshape(-1)[0])
    keep.append(dk)
    return PeWeights(len(layers), arr, _fptr(dk), db), keep


class HipEngine:
    """
    One C-ABI engine: the streaming state of ``n_streams`` audio streams plus one network on one
    MI355X.  Thin, allocation-free wrapper; the reference-shaped classes live in
    ``network_runner.py``.

    ``gru_precision='f32'`` serves every network the trainers save: 1..256 units, one or two GRU layers, up to 32 inputs per
    frame (``use_delta`` over <= 16 coefficients, or 17..32 coefficients).  ``'bf16'`` serves the same widths on plain rows of
    <= 16 coefficients (<= 32 units: ``use_delta`` over <= 14).  Anything else raises NotImplementedError naming the limit.

    ``params.vectorizer = Vectorizer.mels``: the rows are the ``n_filt`` log-mel energies (no DCT; ``n_mfcc`` is ignored), so
    ``row_width`` -- the width of a window row, of ``get_vectors`` / ``set_vectors`` / ``vectorize_raw`` / ``vectorize_clips`` --
    is ``n_filt``, and the same limits hold for it: up to 32 values, more than 16 for float32 networks without ``use_delta``.

    ``weights`` a LIST of weight dicts (same architecture) builds a K-model engine (pe_create_models): one
    front end for all models, and every network output gains a leading model axis ``[K, ...]`` -- even for K = 1.
    """

    def __init__(self, params, weights, n_streams=1, device=0, mfcc_precision='f64', mel_filters=None,
                 gru_precision='f32', ring_precision='f32'):
        from .vectorization import mel_filterbank, speechpy_filterbank
        from .params import Vectorizer
        self._h = C.c_void_p()
        self._async_keep = []
        self._sessions = weakref.WeakSet()   # HipMiner / HipGenerator / HipAugmenter sessions over this engine: closed before the engine is destroyed
        self._views = 0                # host_array() buffers still referenced by numpy arrays (their memory dies with the engine)
        self._close_pending = False
        self.n_streams = int(n_streams)
        self.n_features = int(params.n_features)
        self.n_mfcc = int(params.n_mfcc)
        self.n_filt = int(params.n_filt)
        prec = {'f64': 0, 'f32': 1}[mfcc_precision]
        vec = int(getattr(params, 'vectorizer', Vectorizer.mfccs))
        self.mels = vec == Vectorizer.mels
        self.row_width = self.n_filt if self.mels else self.n_mfcc          # values per frame (params.py:99-109 without the deltas)
        self.feature_size = self.row_width * (2 if params.use_delta else 1)
        self._multi = isinstance(weights, (list, tuple))
        if self.mels:                       # refused by name before the library is touched
            self._check_mels(params, list(weights) if self._multi else [weights], mel_filters, gru_precision, ring_precision)
        self._lib = load()
        p = PeParams(params.sample_rate, params.window_samples, params.hop_samples, params.n_fft,
                     params.n_filt, params.n_mfcc, params.n_features, int(bool(params.use_delta)), prec,
                     {'f32': 0, 'bf16': 1}[gru_precision], vec, {'f32': 0, 'bf16': 1}[ring_precision])
        if mel_filters is None:
            bank = speechpy_filterbank if vec == Vectorizer.speechpy_mfccs else mel_filterbank
            mel_filters = bank(params.sample_rate, params.n_filt, params.n_fft // 2 + 1)
        mel = np.ascontiguousarray(mel_filters, dtype=np.float64)
        if mel.shape != (params.n_filt, params.n_fft // 2 + 1):
            raise ValueError('mel filterbank has shape %r' % (mel.shape,))
        models = list(weights) if self._multi else [weights]
        if not models:
            raise ValueError('no models')
        keep = []                      # keep numpy buffers alive across the call
        ws = (PeWeights * len(models))()
        for m, wm in enumerate(models):
            ws[m], held = _pe_weights(wm, check_dense=False)
            keep.append(held)
        if self._multi:
            rc = self._lib.pe_create_models(C.byref(p), mel.ctypes.data_as(C.POINTER(C.c_double)), ws, len(models),
                                            self.n_streams, int(device), C.byref(self._h))
        else:
            rc = self._lib.pe_create(C.byref(p), mel.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ws[0]),
                                     self.n_streams, int(device), C.byref(self._h))
        if rc != PE_OK:
            msg = self._lib.pe_last_global_error().decode()
            self._h = C.c_void_p()
            self._raise(rc, msg)
        self.units = models[0]['gru'][-1][1].shape[0]
        self.n_models = len(models)
        self._win_hop = (int(params.window_samples), int(params.hop_samples))

    def _check_mels(self, params, models, mel_filters, gru_precision, ring_precision):
        """The limits of a Vectorizer.mels engine (pe_create names the same ones): NotImplementedError for each."""
        from .vectorization import speechpy_filterbank
        w = self.row_width
        if w > 32:
            raise NotImplementedError('Vectorizer.mels feeds n_filt = %d values per frame: the networks take up to 32 inputs per frame' % w)
        if w > 16 and (params.use_delta or gru_precision != 'f32' or ring_precision != 'f32'):
            raise NotImplementedError('Vectorizer.mels with n_filt = %d: rows of more than 16 values feed a float32 network without '
                                      'use_delta, bf16 operands or bf16 rows (got use_delta=%r, gru_precision=%r, ring_precision=%r)'
                                      % (w, bool(params.use_delta), gru_precision, ring_precision))
        if mel_filters is not None:
            given = np.asarray(mel_filters, dtype=np.float64)
            theirs = speechpy_filterbank(params.sample_rate, params.n_filt, params.n_fft // 2 + 1)
            if given.shape == theirs.shape and np.array_equal(given, theirs):
                raise NotImplementedError('Vectorizer.mels is sonopy\'s mel_spec over sonopy\'s filterbank (mel_filterbank): the speechpy '
                                          'filterbank belongs to Vectorizer.speechpy_mfccs')
        for wm in models:
            n_in = int(np.shape(wm['gru'][0][0])[0])
            if n_in != self.feature_size:
                raise NotImplementedError('Vectorizer.mels feeds %d inputs per frame, this network takes %d' % (self.feature_size, n_in))

    def _lead(self, *shape):
        """shape of a network output: a leading model axis on a K-model engine"""
        return ((self.n_models,) if self._multi else ()) + shape

    def set_weights(self, weights, model: int = 0):
        """Replace the network of ``model`` in the live engine (pe_set_weights): same widths as the engine was created
        with (else ValueError, the old network keeps serving); the streams' state stays, and every entry point then gives the
        bits of an engine created with ``weights``."""
        w, keep = _pe_weights(weights)
        self._check(self._lib.pe_set_weights(self._h, C.byref(w), int(model)))
        del keep

    # -- errors -------------------------------------------------------------------------
    @staticmethod
    def _raise(rc, msg):
        if rc == PE_ERR_EOF:
            raise EOFError
        if rc == PE_ERR_INVALID:
            raise ValueError(msg)
        if rc == PE_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == PE_ERR_NOMEM:
            raise MemoryError(msg)
        raise EngineError(rc, msg)

    def _check(self, rc):
        if rc != PE_OK:
            self._raise(rc, self._lib.pe_last_error(self._h).decode())

    def _pcm(self, pcm):
        pcm = np.ascontiguousarray(pcm, dtype='<i2')
        if pcm.ndim == 1:
            pcm = pcm.reshape(1, -1)
        if pcm.ndim != 2 or pcm.shape[0] != self.n_streams:
            raise ValueError('pcm must be int16 [n_streams=%d, chunk_samples], got %r' %
                             (self.n_streams, pcm.shape))
        return pcm

    # -- host entry points --------------------------------------------------------------
    def update(self, pcm) -> np.ndarray:
        """int16 [n_streams, chunk] -> raw network outputs float32 [n_streams]."""
        pcm = self._pcm(pcm)
        out = np.empty(self._lead(self.n_streams), dtype=np.float32)
        self._check(self._lib.pe_update(self._h, pcm.ctypes.data, pcm.shape[1], out.ctypes.data))
        return out

    def update_subset(self, stream_ids, pcm) -> np.ndarray:
        """The streams named in ``stream_ids`` (unique, in range) take one chunk each -- pcm int16 [len(stream_ids), chunk] --
        and every other stream stays as it is; -> raw outputs float32 [len(stream_ids)] in the order of ``stream_ids``."""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).reshape(-1)
        pcm = np.ascontiguousarray(pcm, dtype='<i2')
        if pcm.ndim == 1:
            pcm = pcm.reshape(1, -1)
        if pcm.ndim != 2 or pcm.shape[0] != ids.size:
            raise ValueError('pcm must be int16 [%d active streams, chunk_samples], got %r' % (ids.size, pcm.shape))
        out = np.empty(self._lead(ids.size), dtype=np.float32)
        self._check(self._lib.pe_update_subset(self._h, ids.ctypes.data, ids.size, pcm.ctypes.data, pcm.shape[1], out.ctypes.data))
        return out

    def update_subset_device(self, ids_ptr: int, n_active: int, pcm_ptr: int, chunk_samples: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.pe_update_subset_device(self._h, ids_ptr, n_active, pcm_ptr, chunk_samples, out_ptr, stream))

    def set_renumber_at(self, call_number: int):
        self._check(self._lib.pe_set_renumber_at(self._h, int(call_number)))

    # -- host-fed pipeline (pe_update_async / pe_wait): scripts/engine.py:60-63 hands over host bytes per chunk ----------
    def host_array(self, shape, dtype) -> np.ndarray:
        """A numpy array over pinned, device-visible host memory of this engine (pe_host_alloc): ``update_async`` reads PCM
        from / writes probabilities to such arrays without a staging copy.  The memory belongs to the engine (pe_destroy frees
        it), so the array keeps the engine alive: ``close()`` -- explicit or by garbage collection -- takes effect only once
        the last such array (and every view of it) is gone."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._check(self._lib.pe_host_alloc(self._h, max(n, 1), C.byref(p)))
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        # `buf` is the base object of `arr` and of every view of it; the finalizer holds the engine (a bound method) until buf dies
        self._views += 1
        weakref.finalize(buf, self._view_released).atexit = False      # (at interpreter exit the HIP runtime may already be gone)
        return arr

    def _view_released(self):
        self._views -= 1
        if self._views == 0 and self._close_pending:
            self.close()

    def update_async(self, pcm: np.ndarray, out: np.ndarray = None) -> np.ndarray:
        """Enqueue one update ([n_streams, chunk] int16) and return the float32 [n_streams] array its probabilities will be
        in after ``wait()`` (or once 3 more updates have been enqueued).  Up to 3 updates are in flight: the next chunk
        crosses PCIe while this one runs.  ``pcm`` is handed to ``hipMemcpyAsync`` as it is: PAGEABLE memory is staged by the
        HIP runtime before the call returns (the array is free again at once); memory the runtime knows as PINNED --
        ``host_array``, but also ``torch.Tensor.pin_memory()`` / hipHostRegister'ed buffers -- is read by the DMA engine after
        the call returns and must stay untouched until ``wait()`` or until 3 more updates have been enqueued."""
        pcm = self._pcm(pcm)
        n_out = self.n_models * self.n_streams
        if out is None:
            out = np.empty(self._lead(self.n_streams), dtype=np.float32)
        if out.dtype != np.float32 or out.size != n_out or not out.flags.c_contiguous:
            raise ValueError('out must be a contiguous float32 array of %d elements' % n_out)
        self._check(self._lib.pe_update_async(self._h, pcm.ctypes.data, pcm.shape[1], out.ctypes.data))
        self._async_keep = (self._async_keep + [(pcm, out)])[-4:]          # the buffers of the updates in flight stay alive
        return out

    def _ids(self, stream_ids) -> np.ndarray:
        """stream ids as int32 [n_active], each in range and named once (checked here: no native call sees a bad list)"""
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.n_streams):
            raise ValueError('stream ids must lie in 0..%d' % (self.n_streams - 1))
        if np.unique(ids).size != ids.size:
            raise ValueError('a stream is named twice')
        return ids

    def _out(self, a, dtype, n_rows, what):
        """an output array of a subset call: float32 / float64 / uint8 [n_rows] ([K, n_rows] on a K-model engine), C order"""
        if a is None:
            return np.zeros(self._lead(n_rows), dtype=dtype)
        if not isinstance(a, np.ndarray) or a.dtype != dtype or a.size != self.n_models * n_rows or not a.flags.c_contiguous:
            raise ValueError('%s must be a contiguous %s array of %d elements' % (what, np.dtype(dtype).name, self.n_models * n_rows))
        return a

    def update_subset_async(self, stream_ids, pcm, out=None, conf=None, fired=None):
        """``update_subset`` through the pipeline of ``update_async`` (pe_update_subset_async): the streams named in
        ``stream_ids`` (unique, in range; None = every stream in order) take one chunk each -- pcm int16 [n_active, chunk].
        -> the float32 [n_active] array (``out`` or a new one) the raw outputs are in after ``wait()`` or once 3 more updates
        have been enqueued.  ``conf`` (float64 [n_active]) and ``fired`` (uint8 [n_active]), when given, receive the decoded
        confidences and the activations of this update at the same moment: one subset decode on the device behind the
        update, which moves the named streams' triggers only.  [K, n_active] each on a K-model engine.  Every array may be
        pageable or from ``host_array``; the rules of ``update_async`` apply to each."""
        ids = None if stream_ids is None else self._ids(stream_ids)
        n = self.n_streams if ids is None else ids.size
        pcm = np.ascontiguousarray(pcm, dtype='<i2')
        if pcm.ndim == 1:
            pcm = pcm.reshape(1, -1)
        if pcm.ndim != 2 or pcm.shape[0] != n:
            raise ValueError('pcm must be int16 [%d active streams, chunk_samples], got %r' % (n, pcm.shape))
        out = self._out(out, np.float32, n, 'out')
        conf = None if conf is None else self._out(conf, np.float64, n, 'conf')
        fired = None if fired is None else self._out(fired, np.uint8, n, 'fired')
        self._check(self._lib.pe_update_subset_async(
            self._h, None if ids is None else ids.ctypes.data, n, pcm.ctypes.data, pcm.shape[1], out.ctypes.data,
            None if conf is None else conf.ctypes.data, None if fired is None else fired.ctypes.data))
        self._async_keep = (self._async_keep + [(ids, pcm, out, conf, fired)])[-4:]
        return out

    def wait(self):
        self._check(self._lib.pe_wait(self._h))
        self._async_keep = []

    def reserve_updates(self, max_updates: int, max_chunk_samples: int):
        """Size the engine for update_many (restarts all streams)."""
        self._check(self._lib.pe_reserve_updates(self._h, int(max_updates), int(max_chunk_samples)))

    def update_many(self, pcm) -> np.ndarray:
        """int16 [n_updates, n_streams, chunk] -> raw outputs float32 [n_updates, n_streams]; identical to
        n_updates consecutive update() calls."""
        pcm = np.ascontiguousarray(pcm, dtype='<i2')
        if pcm.ndim != 3 or pcm.shape[1] != self.n_streams:
            raise ValueError('pcm must be int16 [n_updates, n_streams=%d, chunk_samples], got %r' % (self.n_streams, pcm.shape))
        out = np.empty(self._lead(pcm.shape[0], self.n_streams), dtype=np.float32)
        self._check(self._lib.pe_update_many(self._h, pcm.ctypes.data, pcm.shape[2], pcm.shape[0], out.ctypes.data))
        return out

    def update_many_device(self, pcm_ptr: int, chunk_samples: int, n_updates: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.pe_update_many_device(self._h, pcm_ptr, chunk_samples, n_updates, out_ptr, stream))

    def update_vectors(self, pcm, want_features=True):
        pcm = self._pcm(pcm)
        feats = np.empty((self.n_streams, self.n_features, self.row_width), dtype=np.float32) if want_features else None
        self._check(self._lib.pe_update_vectors(self._h, pcm.ctypes.data, pcm.shape[1],
                                                feats.ctypes.data if want_features else None))
        return feats

    def get_vectors(self) -> np.ndarray:
        """Current feature windows float32 [n_streams, T, F], oldest row first."""
        feats = np.empty((self.n_streams, self.n_features, self.row_width), dtype=np.float32)
        self._check(self._lib.pe_get_vectors(self._h, feats.ctypes.data))
        return feats

    def set_vectors(self, feats):
        """Restart every stream with the given feature windows [n_streams, T, F] already emitted."""
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        if feats.shape != (self.n_streams, self.n_features, self.row_width):
            raise ValueError('expected [%d, %d, %d] features, got %r' % (self.n_streams, self.n_features, self.row_width, feats.shape))
        self._check(self._lib.pe_set_vectors(self._h, feats.ctypes.data))

    def predict(self, feats) -> np.ndarray:
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        if feats.ndim != 3 or feats.shape[1:] != (self.n_features, self.feature_size):
            raise ValueError('inputs must be [N, %d, %d], got %r' % (self.n_features, self.feature_size, feats.shape))
        out = np.empty(self._lead(feats.shape[0], 1), dtype=np.float32)
        self._check(self._lib.pe_predict(self._h, feats.ctypes.data, feats.shape[0], out.ctypes.data))
        return out

    def vectorize_raw(self, audio) -> np.ndarray:
        """float64 audio [n] -> MFCC frames float64 [1 + (n - window)//hop, n_mfcc] (stateless); on a Vectorizer.mels engine
        the log-mel frames [.., n_filt]."""
        audio = np.ascontiguousarray(audio, dtype=np.float64).reshape(-1)
        win, hop = self._win_hop
        max_frames = 1 + (audio.size - win) // hop if audio.size >= win else 0
        out = np.empty((max_frames, self.row_width), dtype=np.float64)
        n = C.c_int64(0)
        self._check(self._lib.pe_vectorize_raw(self._h, audio.ctypes.data if audio.size else None, audio.size,
                                               out.ctypes.data if max_frames else None, max_frames, C.byref(n)))
        return out[:n.value]

    def vectorize_mels(self, audio) -> np.ndarray:
        """float64 audio [n] -> log-mel frames float64 [1 + (n - window)//hop, n_filt] (stateless; Vectorizer.mels)."""
        audio = np.ascontiguousarray(audio, dtype=np.float64).reshape(-1)
        win, hop = self._win_hop
        max_frames = 1 + (audio.size - win) // hop if audio.size >= win else 0
        out = np.empty((max_frames, self.n_filt), dtype=np.float64)
        n = C.c_int64(0)
        self._check(self._lib.pe_vectorize_mels(self._h, audio.ctypes.data if audio.size else None, audio.size,
                                                out.ctypes.data if max_frames else None, max_frames, C.byref(n)))
        return out[:n.value]

    def evaluate(self, audio, hop_frames: int) -> np.ndarray:
        """Whole recording (float64 audio) -> raw outputs [n_windows, 1] of the windows ending at frames
        range(T, n_frames, hop_frames): simulate.py:92-104 in one call."""
        audio = np.ascontiguousarray(audio, dtype=np.float64).reshape(-1)
        win, hop = self._win_hop
        n_frames = 1 + (audio.size - win) // hop if audio.size >= win else 0
        n_win = max(0, -(-(n_frames - self.n_features) // int(hop_frames))) if n_frames > self.n_features else 0
        out = np.empty(self._lead(n_win, 1), dtype=np.float32)
        n = C.c_int64(0)
        self._check(self._lib.pe_evaluate(self._h, audio.ctypes.data if audio.size else None, audio.size,
                                          int(hop_frames), out.ctypes.data if n_win else None, n_win, C.byref(n)))
        return out[:, :n.value] if self._multi else out[:n.value]

    @staticmethod
    def _clips(clips):
        """a sequence of 1-D sample arrays -> (samples concatenated once, int64 offsets [n + 1], sample_format): float32 if
        every clip is float32, else float64"""
        clips = [np.asarray(c) for c in clips]
        for c in clips:
            if c.ndim != 1:
                raise ValueError('every clip must be a 1-D array of samples, got shape %r' % (c.shape,))
        f32 = bool(clips) and all(c.dtype == np.float32 for c in clips)
        dtype = np.float32 if f32 else np.float64
        offsets = np.zeros(len(clips) + 1, dtype=np.int64)
        np.cumsum([c.size for c in clips], out=offsets[1:])
        audio = np.empty(int(offsets[-1]), dtype=dtype)
        if clips:
            np.concatenate(clips, out=audio, casting='same_kind')
        return audio, offsets, int(f32)

    def vectorize_clips(self, clips, max_samples, mels=False, out=None) -> np.ndarray:
        """vectorize (vectorization.py:62-84) of every clip in one call: a sequence of 1-D sample arrays of any lengths ->
        float64 [n, n_features, n_mfcc] (mels, or a Vectorizer.mels engine: [n, n_features, n_filt] log-mel rows);
        max_samples <= 0 = no crop."""
        audio, offsets, fmt = self._clips(clips)
        n = offsets.size - 1
        shape = (n, self.n_features, self.n_filt if mels else self.row_width)
        if out is None:
            out = np.empty(shape, dtype=np.float64)
        if out.dtype != np.float64 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError('out must be a contiguous float64 array of shape %r' % (shape,))
        self._check(self._lib.pe_vectorize_clips(self._h, audio.ctypes.data if n else None, fmt, offsets.ctypes.data, n,
                                                 int(max_samples), int(bool(mels)), out.ctypes.data if n else None))
        return out

    def score_clips(self, clips, max_samples, out=None) -> np.ndarray:
        """The network over vectorize (use_delta models: vectorize_delta) of every clip, without the per-clip loop: raw
        outputs float32 [n, 1] as ``predict`` returns them ([K, n, 1] on a K-model engine)."""
        audio, offsets, fmt = self._clips(clips)
        n = offsets.size - 1
        shape = self._lead(n, 1)
        if out is None:
            out = np.empty(shape, dtype=np.float32)
        if out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError('out must be a contiguous float32 array of shape %r' % (shape,))
        self._check(self._lib.pe_score_clips(self._h, audio.ctypes.data if n else None, fmt, offsets.ctypes.data, n,
                                             int(max_samples), out.ctypes.data if n else None))
        return out

    def set_clip_pass_bytes(self, n_bytes: int):
        """Test aid: audio bytes per pass of vectorize_clips / score_clips / evaluate_clips / simulate_clips (default 256 MiB)."""
        self._check(self._lib.pe_set_clip_pass_bytes(self._h, int(n_bytes)))

    def evaluate_clips_layout(self, offsets, hop_frames: int) -> np.ndarray:
        """int64 sample offsets [n + 1] of n recordings -> int64 window offsets [n + 1]: the exclusive prefix sum of the
        windows ``evaluate`` returns per recording (host arithmetic, pe_evaluate_clips_layout)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.size < 1:
            raise ValueError('offsets must hold n + 1 entries')
        out = np.zeros(offsets.size, dtype=np.int64)
        self._check(self._lib.pe_evaluate_clips_layout(self._h, offsets.ctypes.data, offsets.size - 1, int(hop_frames), out.ctypes.data))
        return out

    def _split(self, flat, window_offsets):
        """[K?, total] predictions -> per recording [n_w, 1] ([K, n_w, 1]) views, as ``evaluate`` shapes them"""
        return [flat[..., a:b, np.newaxis] for a, b in zip(window_offsets[:-1], window_offsets[1:])]

    def evaluate_clips(self, audios, hop_frames: int) -> list:
        """``evaluate`` (simulate.py:92-104) of every recording of a sequence in one call -- one front-end launch and one
        network launch per pass instead of a call per recording: -> a list of raw outputs [n_w, 1] ([K, n_w, 1] on a K-model
        engine), bit for bit what ``evaluate`` gives per recording.  An empty recording has no window."""
        audio, offsets, fmt = self._clips(audios)
        n = offsets.size - 1
        woff = self.evaluate_clips_layout(offsets, hop_frames)
        total = int(woff[-1])
        out = np.empty(self._lead(max(total, 1)), dtype=np.float32)
        if n:
            self._check(self._lib.pe_evaluate_clips(self._h, audio.ctypes.data, fmt, offsets.ctypes.data, n, int(hop_frames),
                                                    out.ctypes.data, out.shape[-1]))
        return self._split(out[..., :total], woff)

    @staticmethod
    def _thresholds(thresholds):
        thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        return thr, (thr.ctypes.data if thr.size else None)

    def simulate_scores(self, scores, chunk_threshold: float, sensitivity: float, trigger_level: int, chunk_size: int,
                        thresholds=None):
        """The metrics of simulate.py:114-122 and the buckets of annoyance_estimator.py:70-71 over predictions the caller
        holds (pe_simulate_scores): ``scores`` a sequence with one array of raw outputs per recording ([n_w] or [n_w, 1];
        [K, n_w] or [K, n_w, 1] on a K-model engine).  -> (metrics, buckets): a SIM_METRIC array [n_rec] ([K, n_rec]) and
        int64 [n_thresholds] ([K, n_thresholds]) counts of windows above each of ``thresholds`` (non-decreasing)."""
        K = self.n_models
        rows = [np.asarray(s, dtype=np.float32).reshape(K, -1) for s in scores]
        n = len(rows)
        woff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([r.shape[1] for r in rows], out=woff[1:])
        raw = np.zeros((K, max(int(woff[-1]), 1)), dtype=np.float32)
        if n:
            raw[:, :woff[-1]] = np.concatenate(rows, axis=1)
        thr, thr_p = self._thresholds(thresholds)
        metrics = np.zeros(self._lead(n), dtype=SIM_METRIC)
        buckets = np.zeros(self._lead(thr.size), dtype=np.int64)
        self._check(self._lib.pe_simulate_scores(self._h, raw.ctypes.data, raw.shape[1], woff.ctypes.data, n, float(chunk_threshold),
                                                 float(sensitivity), int(trigger_level), int(chunk_size), thr_p, thr.size,
                                                 metrics.ctypes.data if n else None, buckets.ctypes.data if thr.size else None))
        return metrics, buckets

    def simulate_clips(self, audios, hop_frames: int, chunk_threshold: float, sensitivity: float, trigger_level: int,
                       chunk_size: int, thresholds=None, return_scores: bool = False):
        """``evaluate_clips`` and ``simulate_scores`` in one call, the predictions staying on the device (pe_simulate_clips):
        -> (metrics, buckets, scores): scores the list ``evaluate_clips`` returns, or None without ``return_scores``."""
        audio, offsets, fmt = self._clips(audios)
        n = offsets.size - 1
        woff = self.evaluate_clips_layout(offsets, hop_frames)
        total = int(woff[-1])
        thr, thr_p = self._thresholds(thresholds)
        metrics = np.zeros(self._lead(n), dtype=SIM_METRIC)
        buckets = np.zeros(self._lead(thr.size), dtype=np.int64)
        out = np.empty(self._lead(max(total, 1)), dtype=np.float32) if return_scores else None
        if n:
            self._check(self._lib.pe_simulate_clips(self._h, audio.ctypes.data, fmt, offsets.ctypes.data, n, int(hop_frames),
                                                    float(chunk_threshold), float(sensitivity), int(trigger_level), int(chunk_size),
                                                    thr_p, thr.size, metrics.ctypes.data, buckets.ctypes.data if thr.size else None,
                                                    out.ctypes.data if return_scores else None, out.shape[-1] if return_scores else 0))
        return metrics, buckets, (self._split(out[..., :total], woff) if return_scores else None)

    def stats_scores(self, scores, targets, thresholds=(0.5,), compare='f32'):
        """Confusion counts for a whole table of thresholds and the calibration summary over predictions the caller holds
        (pe_stats_scores): ``scores`` float32 [rows, n] (or [n]: one row), 1 <= rows <= 16, ``targets`` [n] shared by the rows,
        ``thresholds`` non-decreasing, ``compare`` 'f32' (numpy's float32-against-Python-float comparison, what ``Stats``
        makes) or 'f64' (float32 against a float64 array, the annoyance estimate's).  -> (counts STATS_COUNT [rows, T],
        summary STATS_SUMMARY [rows])."""
        thr, code = stats_request(thresholds, compare)
        raw = np.ascontiguousarray(scores, dtype=np.float32)
        raw = raw.reshape(1, -1) if raw.ndim == 1 else raw.reshape(raw.shape[0], -1)
        rows, n = raw.shape
        y = np.ascontiguousarray(targets, dtype=np.float32).reshape(-1)
        if y.size != n:
            raise ValueError('%d targets for %d predictions per row' % (y.size, n))
        counts, summary = _stats_out(rows, thr.size)
        self._check(self._lib.pe_stats_scores(self._h, raw.ctypes.data if raw.size else None, rows, n, y.ctypes.data if n else None, n,
                                              thr.ctypes.data if thr.size else None, thr.size, code,
                                              counts.ctypes.data if thr.size else None, summary.ctypes.data))
        return counts, summary

    def test_clips(self, clips, max_samples, targets, thresholds=(0.5,), compare='f32', return_scores=False):
        """``score_clips`` and ``stats_scores`` in one call, the predictions staying on the device (pe_test_clips).
        -> (counts STATS_COUNT [K, T], summary STATS_SUMMARY [K], scores float32 [K, n] or None); K = 1 on a one-model
        engine."""
        thr, code = stats_request(thresholds, compare)
        audio, offsets, fmt = self._clips(clips)
        n = offsets.size - 1
        y = np.ascontiguousarray(targets, dtype=np.float32).reshape(-1)
        if y.size != n:
            raise ValueError('%d targets for %d clips' % (y.size, n))
        counts, summary = _stats_out(self.n_models, thr.size)
        out = np.zeros((self.n_models, n), dtype=np.float32) if return_scores else None
        if n:
            self._check(self._lib.pe_test_clips(self._h, audio.ctypes.data, fmt, offsets.ctypes.data, n, int(max_samples), y.ctypes.data,
                                                thr.ctypes.data if thr.size else None, thr.size, code,
                                                counts.ctypes.data if thr.size else None, summary.ctypes.data,
                                                out.ctypes.data if return_scores else None))
        return counts, summary, out

    def set_decoder(self, decoder, model=None):
        """Upload a ThresholdDecoder (its cumulative table and scalars) for pe_decode*: for every model, or for ``model``."""
        cd = np.ascontiguousarray(decoder.cd, dtype=np.float64)
        args = (cd.ctypes.data if cd.size else None, cd.size, int(decoder.min_out), int(decoder.out_range), float(decoder.center))
        if model is None:
            self._check(self._lib.pe_set_decoder(self._h, *args))
        else:
            self._check(self._lib.pe_set_decoder_model(self._h, int(model), *args))

    def set_trigger(self, chunk_size: int, sensitivity: float = 0.5, trigger_level: int = 3, model=None):
        if model is None:
            self._check(self._lib.pe_set_trigger(self._h, int(chunk_size), float(sensitivity), int(trigger_level)))
        else:
            self._check(self._lib.pe_set_trigger_model(self._h, int(model), int(chunk_size), float(sensitivity), int(trigger_level)))

    def decode(self, raw, want_fired=False):
        """raw float32 [n_streams] -> decoded confidences float64 [n_streams] (, fired bool [n_streams]); [K, n_streams]
        each on a K-model engine."""
        raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1)
        if raw.size != self.n_models * self.n_streams:
            raise ValueError('expected %d raw outputs' % (self.n_models * self.n_streams))
        conf = np.empty(self._lead(self.n_streams), dtype=np.float64)
        fired = np.zeros(self._lead(self.n_streams), dtype=np.uint8)
        self._check(self._lib.pe_decode(self._h, raw.ctypes.data, conf.ctypes.data, fired.ctypes.data))
        return (conf, fired.astype(bool)) if want_fired else conf

    def decode_subset(self, stream_ids, raw, want_fired=False):
        """``decode`` after ``update_subset``: raw float32 [n_active] in the order of ``stream_ids`` -> confidences float64
        [n_active] (, fired bool [n_active]); [K, n_active] each on a K-model engine.  Only the named streams' triggers move."""
        ids = self._ids(stream_ids)
        raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1)
        if raw.size != self.n_models * ids.size:
            raise ValueError('expected %d raw outputs for %d streams' % (self.n_models * ids.size, ids.size))
        conf = np.empty(self._lead(ids.size), dtype=np.float64)
        fired = np.zeros(self._lead(ids.size), dtype=np.uint8)
        self._check(self._lib.pe_decode_subset(self._h, ids.ctypes.data, ids.size, raw.ctypes.data, conf.ctypes.data, fired.ctypes.data))
        return (conf, fired.astype(bool)) if want_fired else conf

    def clear(self, mask=None):
        if mask is None:
            self._check(self._lib.pe_clear(self._h, None))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (self.n_streams,):
                raise ValueError('mask must have shape (%d,)' % self.n_streams)
            self._check(self._lib.pe_clear(self._h, m.ctypes.data))

    # -- device entry points (pointers are ints, e.g. torch.Tensor.data_ptr()) ---------------
    def update_device(self, pcm_ptr: int, chunk_samples: int, out_ptr: int, stream: int = 0, keep: bool = False):
        """keep=True: the caller promises the chunks at pcm_ptr stay alive and unchanged until the next update's work is
        done -- the leftover samples then stay there instead of being copied to the engine's carry (pe_update_device_keep)."""
        fn = self._lib.pe_update_device_keep if keep else self._lib.pe_update_device
        self._check(fn(self._h, pcm_ptr, chunk_samples, out_ptr, stream))

    def update_vectors_device(self, pcm_ptr: int, chunk_samples: int, feats_ptr: int = 0, stream: int = 0):
        self._check(self._lib.pe_update_vectors_device(self._h, pcm_ptr, chunk_samples, feats_ptr or None, stream))

    def run_device(self, out_ptr: int, stream: int = 0):
        self._check(self._lib.pe_run_device(self._h, out_ptr, stream))

    def predict_device(self, feats_ptr: int, n: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.pe_predict_device(self._h, feats_ptr, n, out_ptr, stream))

    # -- introspection ------------------------------------------------------------------
    def info(self) -> PeInfo:
        i = PeInfo()
        self._check(self._lib.pe_get_info(self._h, C.byref(i)))
        return i

    def stream_state(self):
        q = np.empty(self.n_streams, dtype=np.int32)
        kc = np.empty(self.n_streams, dtype=np.uint32)
        ke = np.empty(self.n_streams, dtype=np.uint32)
        self._check(self._lib.pe_get_stream_state(self._h, q.ctypes.data, kc.ctypes.data, ke.ctypes.data))
        return q, kc, ke

    def set_fused(self, enabled: bool):
        self._check(self._lib.pe_set_fused(self._h, int(bool(enabled))))

    def set_input_projection(self, enabled: bool):
        """Store x.W + b per frame beside the feature ring (True) or recompute it in the network (False); restarts the streams."""
        self._check(self._lib.pe_set_input_projection(self._h, int(bool(enabled))))

    def set_gru_waves(self, waves: int):
        self._check(self._lib.pe_set_gru_waves(self._h, int(waves)))

    def set_gru_tiling(self, tiling: int):
        """-1 automatic, 0 classic four-tile layout, 1 re-tiled stock width (csrc/gru_cw_device.h), 2 float32 products on the
        bf16 matrix pipe (csrc/gru_x3_device.h; automatic above four stream tiles per compute unit).  bf16 networks: 1 / -1 = five
        gate values per lane where the network fits (csrc/gru_b20_device.h), 0 = eight (csrc/gru_bf16_device.h); wide / stacked
        bf16 networks (csrc/gru_wide_bf16_device.h) have one form, 0: every other value raises NotImplementedError."""
        self._check(self._lib.pe_set_gru_tiling(self._h, int(tiling)))

    def gru_tiling(self) -> int:
        """The form this engine's network launches take now (pe_get_gru_tiling): float32 networks of <= 32 units 0 / 1 / 2 as
        above; wide / stacked networks 0 (f32-input MFMAs) or 2 (float32 products on the bf16 pipe); bf16-operand networks
        1 (five gate values per lane) or 0 (eight; wide / stacked bf16 networks always)."""
        return int(self._lib.pe_get_gru_tiling(self._h))

    def set_chain_carry(self, mode: int):
        """Carried window chains (pe_set_chain_carry): 0 off, 1 automatic (the default: after 128 eligible updates in a row),
        2 eager.  Outputs are bit-identical in every mode."""
        self._check(self._lib.pe_set_chain_carry(self._h, int(mode)))

    def chain_carry(self):
        """(mode, active) of pe_get_chain_carry: the setting, and whether the next eligible update advances carried chains."""
        m, a = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.pe_get_chain_carry(self._h, C.byref(m), C.byref(a)))
        return m.value, bool(a.value)

    def chain_skip(self) -> int:
        """The chunk size for which chain launches currently leave out the chains no update hands out (pe_get_chain_skip), or 0."""
        c = C.c_int32(0)
        self._check(self._lib.pe_get_chain_skip(self._h, C.byref(c)))
        return c.value

    def set_timing(self, enabled: bool):
        self._check(self._lib.pe_set_timing(self._h, int(bool(enabled))))

    def last_timing(self):
        a, b = C.c_float(0), C.c_float(0)
        self._check(self._lib.pe_get_last_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        """pe_destroy.  While arrays from ``host_array`` are still referenced the destruction is deferred until the last one
        is gone (their memory is the engine's): nothing can read freed pinned memory through a stale array."""
        if getattr(self, '_h', None) and self._h.value:
            if getattr(self, '_views', 0) > 0:
                self._close_pending = True
                try:
                    self._lib.pe_wait(self._h)       # nothing of this engine stays in flight behind a "closed" handle
                except Exception:
                    pass
                return
            for session in list(getattr(self, '_sessions', ())):
                session.close()
            self._lib.pe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dropout_masks(seed: int, step: int, n: int, feature_size: int, rate: float, layer: int = 0) -> np.ndarray:
    """The per-gate input dropout masks of one training step, float32 [3, n, feature_size] (pe_train_dropout_masks: host
    arithmetic, no GPU): what ``HipTrainer.step`` generates inside its kernel for the same (seed, step).  ``layer=1``: the masks
    of a stacked network's second GRU layer, ``feature_size`` then being the first layer's units
    (pe_train_dropout_masks_layer)."""
    lib = load()
    out = np.empty((3, int(n), int(feature_size)), dtype=np.float32)
    if int(layer) != 0:
        rc = lib.pe_train_dropout_masks_layer(int(seed), int(step), int(layer), int(n), int(feature_size), float(rate), out.ctypes.data)
    else:
        rc = lib.pe_train_dropout_masks(int(seed), int(step), int(n), int(feature_size), float(rate), out.ctypes.data)
    if rc != PE_OK:
        HipEngine._raise(rc, lib.pe_trainer_last_error(None).decode())
    return out


class HipTrainer:
    """
    One C-ABI trainer (pe_trainer): the parameters of Sequential[GRU(units), Dense(1, sigmoid)], their RMSprop accumulators
    and, after ``set_data``, a dataset on one MI355X.  Parameters, gradients and accumulators travel as ONE flat float32 vector
    (kernel | recurrent_kernel | bias | dense_kernel | dense_bias); ``train.py`` holds the reference-shaped ``Trainer``.

    ``weights`` is one weights dict, or a list of them: then the trainer owns that many networks (their ``units`` may differ),
    trains them on the same batches in one launch (``step_models``) and evaluates them together (``evaluate_models``); the
    flat vector is the concatenation in model order, ``units`` and ``n_params`` are lists, ``n_params_total`` the length.

    ``wide=False``: networks of 1..32 units (pe_trainer_create[_models]); ``wide=True``: 1..256 units in any mix
    (pe_trainer_create_wide), the wider ones trained on the matrix cores.  Everything else is the same trainer.

    ``stacked=True`` (pe_trainer_create_stacked): each network has one or two GRU layers of 1..256 units.  A two-layer network's
    flat vector is kernel_0 | recurrent_kernel_0 | bias_0 | kernel_1 | recurrent_kernel_1 | bias_1 | dense_kernel | dense_bias,
    its ``units`` entry the tuple (H1, H2), its ``frozen_mask`` three bits (GRU 0, GRU 1, Dense) and ``loss_grad`` takes
    ``masks=(m0 [3, n, feature_size], m1 [3, n, H1])``.
    """

    def __init__(self, weights, n_features, feature_size, device=0, wide=False, stacked=False):
        self._lib = load()
        self._h = C.c_void_p()
        many = isinstance(weights, (list, tuple))
        models = list(weights) if many else [weights]
        ws = (PeWeights * max(1, len(models)))()
        keep = []
        for m, wm in enumerate(models):
            ws[m], held = _pe_weights(wm)
            keep.append(held)
        if stacked:
            rc = self._lib.pe_trainer_create_stacked(int(n_features), int(feature_size), ws, len(models), int(device), C.byref(self._h))
        elif wide:
            rc = self._lib.pe_trainer_create_wide(int(n_features), int(feature_size), ws, len(models), int(device), C.byref(self._h))
        elif many:
            rc = self._lib.pe_trainer_create_models(int(n_features), int(feature_size), ws, len(models), int(device), C.byref(self._h))
        else:
            rc = self._lib.pe_trainer_create(int(n_features), int(feature_size), ws, int(device), C.byref(self._h))
        if rc != PE_OK:
            msg = self._lib.pe_trainer_last_error(None).decode()
            self._h = C.c_void_p()
            HipEngine._raise(rc, msg)
        self.n_features, self.feature_size = int(n_features), int(feature_size)
        self.n_models = int(self._lib.pe_trainer_n_models(self._h))
        self.n_params_total = int(self._lib.pe_trainer_n_params(self._h))
        units = [wm['gru'][0][1].shape[0] if len(wm['gru']) == 1 else tuple(layer[1].shape[0] for layer in wm['gru']) for wm in models]
        per_model = [int(self._lib.pe_trainer_n_params_model(self._h, m)) for m in range(self.n_models)]
        self.units = units if many else units[0]
        self.n_params = per_model if many else per_model[0]

    def _check(self, rc):
        if rc != PE_OK:
            HipEngine._raise(rc, self._lib.pe_trainer_last_error(self._h).decode())

    def _feats(self, feats):
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        if feats.ndim != 3 or feats.shape[1:] != (self.n_features, self.feature_size):
            raise ValueError('inputs must be [N, %d, %d], got %r' % (self.n_features, self.feature_size, feats.shape))
        return feats

    @staticmethod
    def _targets(targets, n):
        targets = np.ascontiguousarray(targets, dtype=np.float32).reshape(-1)
        if targets.size != n:
            raise ValueError('%d targets for %d inputs' % (targets.size, n))
        return targets

    def _flat(self, v, what):
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
        if v.size != self.n_params_total:
            raise ValueError('%s must hold %d values, got %d' % (what, self.n_params_total, v.size))
        return v

    def get_weights(self) -> np.ndarray:
        out = np.empty(self.n_params_total, dtype=np.float32)
        self._check(self._lib.pe_trainer_get_weights(self._h, out.ctypes.data))
        return out

    def set_weights(self, flat):
        flat = self._flat(flat, 'weights')
        self._check(self._lib.pe_trainer_set_weights(self._h, flat.ctypes.data))

    def get_accumulators(self) -> np.ndarray:
        out = np.empty(self.n_params_total, dtype=np.float32)
        self._check(self._lib.pe_trainer_get_accumulators(self._h, out.ctypes.data))
        return out

    def reset_optimizer(self):
        self._check(self._lib.pe_trainer_reset_optimizer(self._h))

    def loss_grad(self, feats, targets, masks=None, loss_bias=0.7, want_probs=True):
        """-> (loss, flat gradient float32 [n_params], probabilities float32 [n] or None); changes no state."""
        feats = self._feats(feats)
        n = feats.shape[0]
        targets = self._targets(targets, n)
        if masks is not None and isinstance(self.units, tuple):
            if not isinstance(masks, (tuple, list)) or len(masks) != 2:
                raise ValueError('a stacked network takes masks=(layer 0 [3, n, feature_size], layer 1 [3, n, H1])')
            parts = [np.ascontiguousarray(m, dtype=np.float32) for m in masks]
            for part, width in zip(parts, (self.feature_size, self.units[0])):
                if part.shape != (3, n, width):
                    raise ValueError('masks must be [3, %d, %d], got %r' % (n, width, part.shape))
            masks = np.concatenate([part.reshape(-1) for part in parts])
        elif masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.float32)
            if masks.shape != (3, n, self.feature_size):
                raise ValueError('masks must be [3, %d, %d], got %r' % (n, self.feature_size, masks.shape))
        loss = np.zeros(1, dtype=np.float32)
        grads = np.zeros(self.n_params_total, dtype=np.float32)
        probs = np.zeros(n, dtype=np.float32) if want_probs else None
        self._check(self._lib.pe_trainer_loss_grad(self._h, feats.ctypes.data if n else None, targets.ctypes.data if n else None, n,
                                                   masks.ctypes.data if masks is not None else None, float(loss_bias),
                                                   loss.ctypes.data, grads.ctypes.data, probs.ctypes.data if want_probs else None))
        return float(loss[0]), grads, probs

    def apply(self, grads, lr=1e-3, rho=0.9, eps=1e-7, frozen_mask=0):
        grads = self._flat(grads, 'gradients')
        self._check(self._lib.pe_trainer_apply(self._h, grads.ctypes.data, float(lr), float(rho), float(eps), int(frozen_mask)))

    def set_data(self, feats, targets):
        feats = self._feats(feats)
        targets = self._targets(targets, feats.shape[0])
        self._check(self._lib.pe_trainer_set_data(self._h, feats.ctypes.data if feats.size else None,
                                                  targets.ctypes.data if targets.size else None, feats.shape[0]))

    def step(self, indices, dropout_rate=0.0, seed=0, step=0, loss_bias=0.7, lr=1e-3, rho=0.9, eps=1e-7, frozen_mask=0) -> float:
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        loss = np.zeros(1, dtype=np.float32)
        self._check(self._lib.pe_trainer_step(self._h, idx.ctypes.data if idx.size else None, idx.size, float(dropout_rate), int(seed),
                                              int(step), float(loss_bias), float(lr), float(rho), float(eps), int(frozen_mask),
                                              loss.ctypes.data))
        return float(loss[0])

    def evaluate(self, feats, targets=None, loss_bias=0.7):
        """-> (loss, accuracy, probabilities float32 [n]); loss and accuracy are None without targets.  Dropout off."""
        feats = self._feats(feats)
        n = feats.shape[0]
        probs = np.zeros(n, dtype=np.float32)
        if targets is None:
            self._check(self._lib.pe_trainer_evaluate(self._h, feats.ctypes.data if n else None, None, n, float(loss_bias), None, None,
                                                      probs.ctypes.data))
            return None, None, probs
        targets = self._targets(targets, n)
        loss, acc = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.float32)
        self._check(self._lib.pe_trainer_evaluate(self._h, feats.ctypes.data if n else None, targets.ctypes.data if n else None, n,
                                                  float(loss_bias), loss.ctypes.data, acc.ctypes.data, probs.ctypes.data))
        return float(loss[0]), float(acc[0]), probs

    @staticmethod
    def _source(validation):
        return TRAIN_SOURCE_VALIDATION if validation else TRAIN_SOURCE_DATA

    def n_samples(self, validation=False) -> int:
        """samples of the resident training (validation) set; 0 if never uploaded"""
        return int(self._lib.pe_trainer_n_samples(self._h, self._source(validation)))

    def append(self, feats, targets, validation=False):
        """more samples behind the resident training (validation) set, whose own samples stay where they are (pe_trainer_append)"""
        feats = self._feats(feats)
        targets = self._targets(targets, feats.shape[0])
        if feats.shape[0]:
            self._check(self._lib.pe_trainer_append(self._h, self._source(validation), feats.ctypes.data, targets.ctypes.data, feats.shape[0]))

    def get_data(self, first=0, n=None, validation=False):
        """-> (inputs float32 [n, n_features, feature_size], targets float32 [n]): samples first .. first + n of a resident set
        (n None: to its end), read back from the device (pe_trainer_get_data)"""
        n = self.n_samples(validation) - int(first) if n is None else int(n)
        feats = np.empty((max(n, 0), self.n_features, self.feature_size), dtype=np.float32)
        targets = np.empty(max(n, 0), dtype=np.float32)
        self._check(self._lib.pe_trainer_get_data(self._h, self._source(validation), int(first), n, feats.ctypes.data if n > 0 else None,
                                                  targets.ctypes.data if n > 0 else None))
        return feats, targets

    def split(self, flat):
        """the concatenated flat vector -> one view per network, in model order"""
        sizes = self.n_params if isinstance(self.n_params, list) else [self.n_params]
        return np.split(np.asarray(flat), np.cumsum(sizes)[:-1])

    def set_validation(self, feats, targets):
        """a second resident set (``evaluate_models(source='validation')``), next to the one of ``set_data``"""
        feats = self._feats(feats)
        targets = self._targets(targets, feats.shape[0])
        self._check(self._lib.pe_trainer_set_validation(self._h, feats.ctypes.data if feats.size else None,
                                                        targets.ctypes.data if targets.size else None, feats.shape[0]))

    def _per_model(self, v, what):
        """one value for all networks, or a sequence of one per network -> a plain list (no numpy: a seed keeps all 64 bits)"""
        v = [v] * self.n_models if np.ndim(v) == 0 else list(v)
        if len(v) != self.n_models:
            raise ValueError('%s must hold one value per network (%d), got %d' % (what, self.n_models, len(v)))
        return v

    def step_models(self, indices, step=0, dropout_rate=0.0, seed=0, loss_bias=0.7, lr=1e-3, rho=0.9, eps=1e-7,
                    frozen_mask=0) -> np.ndarray:
        """One optimizer step of every network on the same batch, in one launch.  Each hyperparameter is one value for all
        networks or a sequence with one value per network.  -> the batch losses, float32 [n_models]."""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        cols = [self._per_model(v, name) for v, name in ((dropout_rate, 'dropout_rate'), (seed, 'seed'), (loss_bias, 'loss_bias'),
                                                         (lr, 'lr'), (rho, 'rho'), (eps, 'eps'), (frozen_mask, 'frozen_mask'))]
        hp = (PeTrainHparams * self.n_models)()
        for m in range(self.n_models):
            hp[m] = PeTrainHparams(float(cols[0][m]), int(cols[1][m]), float(cols[2][m]), float(cols[3][m]), float(cols[4][m]),
                                   float(cols[5][m]), int(cols[6][m]))
        loss = np.zeros(self.n_models, dtype=np.float32)
        self._check(self._lib.pe_trainer_step_models(self._h, idx.ctypes.data if idx.size else None, idx.size, int(step), hp,
                                                     loss.ctypes.data))
        return loss

    def evaluate_models(self, feats=None, targets=None, loss_bias=0.7, source='host', want_probs=True):
        """Every network on the same samples, dropout off.  ``source``: 'host' (``feats`` [N, n_features, feature_size] and
        optional ``targets``, uploaded once), 'data' (the set of ``set_data``) or 'validation' (``set_validation``): nothing
        but the results crosses the bus.  -> (losses float32 [n_models], accuracies float32 [n_models], probabilities float32
        [n_models, N] or None); losses and accuracies are None without targets."""
        code = {'host': TRAIN_SOURCE_HOST, 'data': TRAIN_SOURCE_DATA, 'validation': TRAIN_SOURCE_VALIDATION}.get(source)
        if code is None:
            raise ValueError("source must be 'host', 'data' or 'validation', got %r" % (source,))
        K = self.n_models
        bias = np.ascontiguousarray(self._per_model(loss_bias, 'loss_bias'), dtype=np.float32)
        loss, acc = np.zeros(K, dtype=np.float32), np.zeros(K, dtype=np.float32)
        if code == TRAIN_SOURCE_HOST:
            feats = self._feats(feats)
            n = feats.shape[0]
            has_targets = targets is not None
            targets = self._targets(targets, n) if has_targets else None
            probs = np.zeros((K, n), dtype=np.float32)
            self._check(self._lib.pe_trainer_evaluate_models(
                self._h, code, feats.ctypes.data if n else None, targets.ctypes.data if has_targets and n else None, n,
                bias.ctypes.data, loss.ctypes.data if has_targets else None, acc.ctypes.data if has_targets else None,
                probs.ctypes.data))
            return (loss, acc, probs) if has_targets else (None, None, probs)
        probs = None
        if want_probs:
            probs = np.zeros((K, max(0, int(self._lib.pe_trainer_n_samples(self._h, code)))), dtype=np.float32)   # (no set: the call refuses)
        self._check(self._lib.pe_trainer_evaluate_models(self._h, code, None, None, 0, bias.ctypes.data, loss.ctypes.data,
                                                         acc.ctypes.data, probs.ctypes.data if want_probs and probs.size else None))
        return loss, acc, probs

    def stats_models(self, feats=None, targets=None, thresholds=(0.5,), compare='f32', source='host', want_probs=False):
        """``evaluate_models``' forward pass and ``HipEngine.stats_scores`` over its probabilities, which stay on the device
        (pe_trainer_stats_models); ``source`` as ``evaluate_models`` takes it, host data with targets.  -> (counts
        STATS_COUNT [n_models, T], summary STATS_SUMMARY [n_models], probabilities float32 [n_models, N] or None)."""
        code = {'host': TRAIN_SOURCE_HOST, 'data': TRAIN_SOURCE_DATA, 'validation': TRAIN_SOURCE_VALIDATION}.get(source)
        if code is None:
            raise ValueError("source must be 'host', 'data' or 'validation', got %r" % (source,))
        thr, cmp_code = stats_request(thresholds, compare)
        counts, summary = _stats_out(self.n_models, thr.size)
        feats_p = targets_p = None
        if code == TRAIN_SOURCE_HOST:
            feats = self._feats(feats)
            n = feats.shape[0]
            if targets is None:
                raise ValueError('statistics over host data need targets')
            targets = self._targets(targets, n)
            feats_p, targets_p = (feats.ctypes.data, targets.ctypes.data) if n else (None, None)
        else:
            n = max(0, int(self._lib.pe_trainer_n_samples(self._h, code)))        # (no set: the call refuses)
        probs = np.zeros((self.n_models, n), dtype=np.float32) if want_probs else None
        self._check(self._lib.pe_trainer_stats_models(self._h, code, feats_p, targets_p, n, thr.ctypes.data if thr.size else None, thr.size,
                                                      cmp_code, counts.ctypes.data if thr.size else None, summary.ctypes.data,
                                                      probs.ctypes.data if want_probs and probs.size else None))
        return counts, summary, probs

    # -- sampled training (pe_trainer_sample_*) -----------------------------------------------------------------------------
    def evaluate_indices(self, indices, loss_bias=0.7, validation=False, want_probs=True):
        """``evaluate_models`` over rows ``indices`` (any order, repeats allowed) of a resident set, without an upload: ->
        (losses [n_models], accuracies [n_models], probabilities [n_models, len(indices)] or None), bit for bit what
        ``evaluate_models`` gives for host copies of those rows (pe_trainer_evaluate_indices)."""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        K = self.n_models
        bias = np.ascontiguousarray(self._per_model(loss_bias, 'loss_bias'), dtype=np.float32)
        loss, acc = np.zeros(K, dtype=np.float32), np.zeros(K, dtype=np.float32)
        probs = np.zeros((K, idx.size), dtype=np.float32) if want_probs else None
        self._check(self._lib.pe_trainer_evaluate_indices(self._h, self._source(validation), idx.ctypes.data if idx.size else None, idx.size,
                                                          bias.ctypes.data, loss.ctypes.data, acc.ctypes.data,
                                                          probs.ctypes.data if want_probs and idx.size else None))
        return loss, acc, probs

    def sample_reset(self, eligible=None, selected=()):
        """Replace the selection state of the training set: ``eligible`` bool [n] (None: every row), ``selected`` the rows
        selected so far, in order (pe_trainer_sample_reset)."""
        n = self.n_samples()
        if eligible is not None:
            eligible = np.ascontiguousarray(np.asarray(eligible).reshape(-1) != 0, dtype=np.uint8)
            if eligible.size != n:
                raise ValueError('eligible must hold one flag per row (%d), got %d' % (n, eligible.size))
        sel = np.ascontiguousarray(selected, dtype=np.int32).reshape(-1)
        self._check(self._lib.pe_trainer_sample_reset(self._h, eligible.ctypes.data if eligible is not None and n else None,
                                                      sel.ctypes.data if sel.size else None, sel.size))

    def sample_choose(self, max_new, order='index', model=0, want_probs=False):
        """Predict the whole training set with network ``model`` and select the first ``max_new`` failing, eligible, not yet
        selected rows in ``order`` ('index': lowest row first; 'error': largest float32 |p - y| first, ties to the lower row),
        all on the device (pe_trainer_sample_choose).  -> (report dict ``n``, ``n_correct``, ``n_failed``, ``n_remaining``,
        ``n_added``, ``n_selected``; the added rows int32 in order; probabilities float32 [n] or None)."""
        code = SAMPLE_ORDER.get(order)
        if code is None:
            raise ValueError("order must be 'index' or 'error', got %r" % (order,))
        max_new = int(max_new)
        report = PeSampleReport()
        added = np.zeros(min(max(max_new, 0), SAMPLE_MAX_NEW), dtype=np.int32)
        probs = np.zeros(max(0, self.n_samples()), dtype=np.float32) if want_probs else None
        self._check(self._lib.pe_trainer_sample_choose(self._h, int(model), max_new, code, C.byref(report),
                                                       added.ctypes.data if added.size else None,
                                                       probs.ctypes.data if want_probs and probs.size else None))
        return {name: int(getattr(report, name)) for name, _ in PeSampleReport._fields_}, added[:int(report.n_added)].copy(), probs

    def sample_selected(self) -> np.ndarray:
        """the selected rows int32, in the order they were selected (pe_trainer_sample_selected)"""
        out = np.zeros(max(0, int(self._lib.pe_trainer_n_selected(self._h))), dtype=np.int32)
        self._check(self._lib.pe_trainer_sample_selected(self._h, out.ctypes.data if out.size else None))
        return out

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            self._lib.pe_trainer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Session:
    """
    What the device sessions over one ``HipEngine`` share: the handle and its release, the engine's set of open sessions, and
    the checks of ids and targets.  A subclass names its destroy function and the word of its "closed" message.
    """
    _destroy = None     # 'pe_miner_destroy'
    _doing = None       # 'mining'

    def _open(self, engine):
        self._lib = load()
        self._h = C.c_void_p()
        self.engine = engine

    def _opened(self):
        """after the create call: the engine closes every session it still has before it is destroyed itself"""
        if self.engine is not None:
            self.engine._sessions.add(self)

    @staticmethod
    def _ids(ids, n, word):
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise ValueError('%s ids must be in 0..%d' % (word, n - 1))
        return ids.astype(np.int32)

    @staticmethod
    def _targets(targets, ids):
        targets = np.ascontiguousarray(targets, dtype=np.float32).reshape(-1)
        if targets.size != ids.size:
            raise ValueError('%d targets for %d ids' % (targets.size, ids.size))
        return targets

    def _handle(self):
        if not self._h.value:
            raise ValueError('the %s session is closed (close(), or its engine was closed)' % self._doing)
        return self._h

    def close(self):
        """the session's destroy call; the engine calls it for every session it still has when it is closed itself"""
        if getattr(self, '_h', None) and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipMiner(_Session):
    """
    One C-ABI mining session (pe_miner) over one ``HipEngine``: the recordings resident on the device, every frame computed once;
    ``mining.Miner`` is the reference-shaped class.  Chunks carry GLOBAL ids: recording r's chunk i is ``chunk_offsets[r] + i``.
    The session keeps its engine alive; close it before the engine.
    """
    _destroy, _doing = 'pe_miner_destroy', 'mining'

    def __init__(self, engine: HipEngine, audios, chunk_size: int, buffer_samples: int, carry_audio: bool = True):
        self._open(engine)
        audio, offsets, fmt = HipEngine._clips(audios)
        self.n_recordings = offsets.size - 1
        self.chunk_size, self.buffer_samples = int(chunk_size), int(buffer_samples)
        engine._check(self._lib.pe_miner_create(engine._h, audio.ctypes.data if audio.size else None, fmt, offsets.ctypes.data,
                                                self.n_recordings, self.chunk_size, self.buffer_samples, int(bool(carry_audio)),
                                                C.byref(self._h)))
        self._opened()
        self.chunk_offsets = np.zeros(self.n_recordings + 1, dtype=np.int64)
        engine._check(self._lib.pe_miner_layout(self._h, self.chunk_offsets.ctypes.data))
        self.n_chunks = int(self.chunk_offsets[-1])

    def scan(self, first=0, threshold=0.5, capacity=None, return_scores=False, model=0):
        """-> (hits int32 [<= capacity] ascending global ids, n_above, scores float32 [n_chunks - first] or None)"""
        first = int(first)
        n = self.n_chunks - first
        capacity = max(n, 0) if capacity is None else int(capacity)
        hits = np.empty(max(capacity, 0), dtype=np.int32)
        scores = np.empty(max(n, 0), dtype=np.float32) if return_scores else None
        n_hits, n_above = C.c_int32(0), C.c_int64(0)
        self.engine._check(self._lib.pe_miner_scan(self._handle(), int(model), first, float(threshold),
                                                   scores.ctypes.data if return_scores and n > 0 else None,
                                                   hits.ctypes.data if capacity > 0 else None, capacity, C.byref(n_hits), C.byref(n_above)))
        return hits[:n_hits.value], int(n_above.value), scores

    def vectorize(self, hits) -> np.ndarray:
        hits = self._ids(hits, self.n_chunks, 'chunk')
        out = np.empty((hits.size, self.engine.n_features, self.engine.n_mfcc), dtype=np.float64)
        if hits.size:
            self.engine._check(self._lib.pe_miner_vectorize(self._handle(), hits.ctypes.data, hits.size, out.ctypes.data))
        return out

    def append(self, trainer: HipTrainer, hits, validation=False, target=0.0):
        hits = self._ids(hits, self.n_chunks, 'chunk')
        if hits.size:
            self.engine._check(self._lib.pe_miner_append(self._handle(), trainer._h, HipTrainer._source(validation), hits.ctypes.data,
                                                         hits.size, float(target)))


class HipGenerator(_Session):
    """
    One C-ABI generating session (pe_generator) over one ``HipEngine``: the background and clip pools resident on the device, one
    plan at a time mixed and vectorized there; ``generated.Generator`` is the reference-shaped class and the planner.  Chunks
    carry GLOBAL ids over the files of the resident plan.  The session keeps its engine alive; close it before the engine.
    """
    _destroy, _doing = 'pe_generator_destroy', 'generating'

    def __init__(self, engine: HipEngine, backgrounds, clips, chunk_size: int):
        self._open(engine)
        self.chunk_size = int(chunk_size)
        bg, bg_off = self._pool(backgrounds)
        cl, cl_off = self._pool(clips)
        self.background_chunks = np.maximum(np.diff(bg_off) - 1, 0) // max(self.chunk_size, 1)
        engine._check(self._lib.pe_generator_create(engine._h, bg.ctypes.data if bg.size else None, bg_off.ctypes.data, bg_off.size - 1,
                                                    cl.ctypes.data if cl.size else None, cl_off.ctypes.data, cl_off.size - 1,
                                                    self.chunk_size, C.byref(self._h)))
        self._opened()
        self.chunk_offsets = np.zeros(1, dtype=np.int64)

    @staticmethod
    def _pool(audios):
        audios = [np.asarray(a) for a in audios]
        for a in audios:
            if a.ndim != 1 or a.dtype != np.float32:
                raise ValueError('every recording must be a 1-D float32 array (load_audio), got %s %r' % (a.dtype, a.shape))
        offsets = np.zeros(len(audios) + 1, dtype=np.int64)
        np.cumsum([a.size for a in audios], out=offsets[1:])
        return (np.concatenate(audios) if audios else np.empty(0, np.float32)), offsets

    def set_plan(self, files, segments):
        """``files`` / ``segments``: structured arrays of ``GEN_FILE`` / ``GEN_SEGMENT``; mixes and vectorizes every file"""
        files = np.ascontiguousarray(files, dtype=GEN_FILE)
        segments = np.ascontiguousarray(segments, dtype=GEN_SEGMENT)
        self.engine._check(self._lib.pe_generator_set_plan(self._handle(), files.ctypes.data if files.size else None, files.size,
                                                           segments.ctypes.data if segments.size else None, segments.size))
        self.chunk_offsets = np.zeros(files.size + 1, dtype=np.int64)
        np.cumsum(self.background_chunks[files['background']], out=self.chunk_offsets[1:])

    @property
    def n_chunks(self):
        return int(self.chunk_offsets[-1])

    def audio(self, file: int, first: int = 0, n: int = None) -> np.ndarray:
        """float64 mixed samples ``first .. first + n`` (default: to the end) of planned file ``file``"""
        file = int(file)
        if not 0 <= file < self.chunk_offsets.size - 1:
            raise ValueError('file %d is outside the plan of %d files' % (file, self.chunk_offsets.size - 1))
        total = int(self.chunk_offsets[file + 1] - self.chunk_offsets[file]) * self.chunk_size
        n = total - int(first) if n is None else int(n)
        out = np.empty(max(n, 0), dtype=np.float64)
        self.engine._check(self._lib.pe_generator_audio(self._handle(), file, int(first), n, out.ctypes.data if out.size else None))
        return out

    def vectorize(self, ids) -> np.ndarray:
        ids = self._ids(ids, self.n_chunks, 'chunk')
        out = np.empty((ids.size, self.engine.n_features, self.engine.feature_size), dtype=np.float32)
        if ids.size:
            self.engine._check(self._lib.pe_generator_vectorize(self._handle(), ids.ctypes.data, ids.size, out.ctypes.data))
        return out

    def append(self, trainer: HipTrainer, ids, targets, validation=False):
        ids = self._ids(ids, self.n_chunks, 'chunk')
        targets = self._targets(targets, ids)
        if ids.size:
            self.engine._check(self._lib.pe_generator_append(self._handle(), trainer._h, HipTrainer._source(validation), ids.ctypes.data,
                                                             targets.ctypes.data, ids.size))


class HipAugmenter(_Session):
    """
    One C-ABI augmenting session (pe_augmenter) over one ``HipEngine``: the clip and noise pools resident on the device, one plan
    at a time mixed and vectorized there; ``augment.NoiseAugmenter`` is the reference-shaped class and the planner.  The session
    keeps its engine alive; close it before the engine.  ``engine=None`` makes a session without a device that only checks the
    plans handed to ``set_plan``.
    """
    _destroy, _doing = 'pe_augmenter_destroy', 'augmenting'

    def __init__(self, engine, clips, noises):
        self._open(engine)
        cl, cl_off = HipGenerator._pool(clips)
        no, no_off = HipGenerator._pool(noises)
        self.clip_lengths = np.diff(cl_off)
        self.n_copies = 0
        self._copy_clip = np.zeros(0, dtype=np.int64)
        self._check(self._lib.pe_augmenter_create(engine._h if engine is not None else None, cl.ctypes.data if cl.size else None,
                                                  cl_off.ctypes.data, cl_off.size - 1, no.ctypes.data if no.size else None,
                                                  no_off.ctypes.data, no_off.size - 1, C.byref(self._h)))
        self._opened()

    def _check(self, rc):
        if self.engine is not None:
            self.engine._check(rc)
        elif rc != PE_OK:
            HipEngine._raise(rc, self._lib.pe_last_global_error().decode())

    def set_plan(self, copies, pieces):
        """``copies`` / ``pieces``: structured arrays of ``AUG_COPY`` / ``AUG_PIECE``; computes every copy's noise volume"""
        copies = np.ascontiguousarray(copies, dtype=AUG_COPY)
        pieces = np.ascontiguousarray(pieces, dtype=AUG_PIECE)
        self._check(self._lib.pe_augmenter_set_plan(self._handle(), copies.ctypes.data if copies.size else None, copies.size,
                                                    pieces.ctypes.data if pieces.size else None, pieces.size))
        self.n_copies = int(copies.size)
        self._copy_clip = copies['clip'].astype(np.int64)

    def volumes(self, overflowed=True):
        """-> (clip volume float64 [n_clips], noise volume float64 [n_copies], overflowed int64 [n_copies] or None)"""
        va = np.empty(self.clip_lengths.size, dtype=np.float64)
        vn = np.empty(self.n_copies, dtype=np.float64)
        over = np.zeros(self.n_copies, dtype=np.int64) if overflowed else None
        self._check(self._lib.pe_augmenter_volumes(self._handle(), va.ctypes.data, vn.ctypes.data if vn.size else None,
                                                   over.ctypes.data if overflowed and over.size else None))
        return va, vn, over

    def _copy(self, copy):
        copy = int(copy)
        if not 0 <= copy < self.n_copies:
            raise ValueError('copy %d is outside the plan of %d copies' % (copy, self.n_copies))
        return copy, int(self.clip_lengths[self._copy_clip[copy]])

    def audio(self, copy: int) -> np.ndarray:
        """float64: the mix of copy ``copy``, what ``noised_audio`` returns"""
        copy, n = self._copy(copy)
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.pe_augmenter_audio(self._handle(), copy, out.ctypes.data, None))
        return out

    def pcm(self, copy: int) -> np.ndarray:
        """int16: what ``save_audio`` writes for copy ``copy``"""
        copy, n = self._copy(copy)
        out = np.empty(n, dtype=np.int16)
        self._check(self._lib.pe_augmenter_audio(self._handle(), copy, None, out.ctypes.data))
        return out

    def _copies(self, ids):
        return self._ids(np.arange(self.n_copies) if ids is None else ids, self.n_copies, 'copy')

    def vectorize(self, ids=None, max_samples: int = 0) -> np.ndarray:
        ids = self._copies(ids)
        out = np.empty((ids.size, self.engine.n_features, self.engine.feature_size), dtype=np.float32)
        if ids.size:
            self._check(self._lib.pe_augmenter_vectorize(self._handle(), ids.ctypes.data, ids.size, int(max_samples), out.ctypes.data))
        return out

    def append(self, trainer: HipTrainer, ids, targets, validation=False, max_samples: int = 0):
        ids = self._copies(ids)
        targets = self._targets(targets, ids)
        if ids.size:
            self._check(self._lib.pe_augmenter_append(self._handle(), trainer._h, HipTrainer._source(validation), ids.ctypes.data,
                                                      targets.ctypes.data, ids.size, int(max_samples)))
