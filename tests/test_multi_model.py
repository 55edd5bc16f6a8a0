"""
-m gpu: several models on the same streams (pe_create_models).  Block m of every network output of a K-model engine
is bit for bit what a one-model engine with model m, the same params, size and form computes; the decoder and the
trigger run per (model, stream); the oracle checks each model's block.
"""
import warnings

import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P
from mycroft_precise_amd._lib import HipEngine
from oracle import listener as ol

pytestmark = pytest.mark.gpu

CHUNK = 1024


def _models(stock, n_in=13, units=(20,)):
    """K = 3: the golden stock weights (where the shape is the stock one) and two seeded synthetic networks"""
    first = stock if (n_in, units) == (13, (20,)) else synth.make_weights(n_in=n_in, units=units, seed=500)
    return [first, synth.make_weights(n_in=n_in, units=units, seed=501), synth.make_weights(n_in=n_in, units=units, seed=502)]


def _pcm(rng, n_up, n, chunk=CHUNK):
    """[n_up][n][chunk] int16: tones in noise, at most 512 distinct streams (tiled beyond)"""
    d = min(n, 512)
    t = np.arange(n_up * chunk, dtype=np.float64)
    f = rng.uniform(200, 3000, size=(d, 1))
    x = 6000 * np.sin(2 * np.pi * f * t / 16000) + rng.normal(0, 1500, size=(d, n_up * chunk))
    x = np.clip(x, -32768, 32767).astype('<i2').reshape(d, n_up, chunk).transpose(1, 0, 2)
    return np.ascontiguousarray(np.tile(x, (1, -(-n // d), 1))[:, :n])


# every row of DESIGN §0 a K-model engine can take: (name, n_streams, params overrides, front end / gru / ring precision, n_in, units)
CONFIGS = [
    ('form1_fused_256', 256, {}, 'f64', 'f32', 'f32', 13, (20,)),
    ('form1_fused_4096', 4096, {}, 'f64', 'f32', 'f32', 13, (20,)),
    ('form1_fused_4096_f32_front_end', 4096, {}, 'f32', 'f32', 'f32', 13, (20,)),
    ('form0_fused_16384', 16384, {}, 'f64', 'f32', 'f32', 13, (20,)),
    ('form2_two_launches_20480', 20480, {}, 'f64', 'f32', 'f32', 13, (20,)),
    ('bf16_b20_fused_8192', 8192, {}, 'f64', 'bf16', 'bf16', 13, (20,)),
    ('bf16_b20_fused_8192_f32_front_end', 8192, {}, 'f32', 'bf16', 'bf16', 13, (20,)),
    ('bf16_eight_values_use_delta', 96, {'use_delta': True}, 'f64', 'bf16', 'f32', 26, (24,)),
    ('use_delta', 64, {'use_delta': True}, 'f64', 'f32', 'f32', 26, (20,)),
    ('use_delta_one_wave_9000', 9000, {'use_delta': True}, 'f64', 'f32', 'f32', 26, (20,)),
    ('units32', 48, {}, 'f64', 'f32', 'f32', 13, (32,)),
    ('units12_classic', 200, {}, 'f64', 'f32', 'f32', 13, (12,)),
    ('units28_four_waves', 256, {}, 'f64', 'f32', 'f32', 13, (28,)),
    ('general_front_end', 40, {'n_fft': 1024, 'n_filt': 40, 'n_mfcc': 20}, 'f64', 'f32', 'f32', 20, (20,)),
    ('wide64', 64, {}, 'f64', 'f32', 'f32', 13, (64,)),
]


def _params(over):
    p = P.pr.copy()
    p.__dict__.update(over)
    return p


@pytest.mark.parametrize('cfg', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_block_equals_a_one_model_engine(cfg, stock_weights):
    import torch
    name, n, over, mp, gp, rp, n_in, units = cfg
    hpr = _params(over)
    models = _models(stock_weights, n_in, units)
    K = len(models)
    rng = np.random.default_rng(7)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        multi = HipEngine(hpr, models, n_streams=n, mfcc_precision=mp, gru_precision=gp, ring_precision=rp)
        ones = [HipEngine(hpr, w, n_streams=n, mfcc_precision=mp, gru_precision=gp, ring_precision=rp) for w in models]
    assert multi.n_models == K and multi._lib.pe_get_n_models(multi._h) == K
    form = multi.gru_tiling()
    for e in ones:
        e.set_gru_tiling(form)
        assert e.gru_tiling() == form
    engines = [multi] + ones
    n_up = 6 if n <= 4096 else 3
    pcm = _pcm(rng, n_up, n)

    def same(got, wants, what):
        assert got.shape[0] == K, what
        for m in range(K):
            assert np.array_equal(got[m], wants[m]), (name, what, m)

    # pe_update, then pe_set_fused(0) on every engine (two launches: the same bits)
    for u in range(n_up):
        if u == n_up // 2:
            for e in engines:
                e.set_fused(False)
        same(multi.update(pcm[u]), [e.update(pcm[u]) for e in ones], 'update %d' % u)
    for e in engines:
        e.set_fused(True)
    # pe_update_subset at random cadences
    for u in range(3):
        ids = np.sort(rng.choice(n, size=max(1, n // (2 + u)), replace=False)).astype(np.int32)
        chunk = int(rng.choice([512, 1024, 1600]))
        sub = rng.integers(-20000, 20000, size=(ids.size, chunk)).astype('<i2')
        same(multi.update_subset(ids, sub), [e.update_subset(ids, sub) for e in ones], 'subset %d' % u)
    # pe_update_device_keep on alternating resident slabs, pe_run_device
    dev = torch.device('cuda', 0)
    slabs = [torch.from_numpy(pcm[u]).to(dev) for u in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    outs = [torch.empty(K * n, device=dev)] + [torch.empty(n, device=dev) for _ in ones]
    for u in range(4):
        for e, o in zip(engines, outs):
            e.update_device(slabs[u % 2].data_ptr(), CHUNK, o.data_ptr(), st, keep=True)
        torch.cuda.synchronize()
        same(outs[0].cpu().numpy().reshape(K, n), [o.cpu().numpy() for o in outs[1:]], 'keep %d' % u)
    for e, o in zip(engines, outs):
        e.run_device(o.data_ptr(), st)
    torch.cuda.synchronize()
    same(outs[0].cpu().numpy().reshape(K, n), [o.cpu().numpy() for o in outs[1:]], 'run_device')
    # pe_update_async
    got = [multi.update_async(pcm[u]) for u in range(3)]
    want = [[e.update_async(pcm[u]) for u in range(3)] for e in ones]
    for e in engines:
        e.wait()
    for u in range(3):
        same(got[u], [want[m][u] for m in range(K)], 'async %d' % u)
    # pe_predict, pe_evaluate
    feats = rng.normal(0, 5, size=(min(n, 300), hpr.n_features, hpr.feature_size)).astype(np.float32)
    same(multi.predict(feats), [e.predict(feats) for e in ones], 'predict')
    audio = rng.normal(0, 0.2, size=16000 * 3)
    same(multi.evaluate(audio, 2), [e.evaluate(audio, 2) for e in ones], 'evaluate')
    # pe_update_many after pe_reserve_updates (the form may change with the reservation: pinned again)
    for e in engines:
        e.reserve_updates(4, CHUNK)
    form = multi.gru_tiling()
    for e in ones:
        e.set_gru_tiling(form)
    many = _pcm(rng, 4, n)
    same(multi.update_many(many), [e.update_many(many) for e in ones], 'update_many')
    for e in engines:
        e.close()


@pytest.mark.parametrize('K', [2, 4, 8])
def test_fused_shape_of_every_model_count(stock_weights, K):
    """The K-model fused launch picks its network shape from (K, tiles) (kernels.hip fused_models_four_waves): whatever it picks,
    every block equals a one-model engine's, through updates at 4096 streams in both leftover styles."""
    import torch
    n, n_up = 4096, 8
    models = [stock_weights] + [synth.make_weights(seed=700 + k) for k in range(K - 1)]
    multi = HipEngine(P.pr, models, n_streams=n)
    ones = [HipEngine(P.pr, w, n_streams=n) for w in models]
    pcm = _pcm(np.random.default_rng(K), n_up, n)
    dev = torch.device('cuda', 0)
    slabs = [torch.from_numpy(pcm[u]).to(dev) for u in range(n_up)]
    st = torch.cuda.current_stream().cuda_stream
    outs = [torch.empty(K * n, device=dev)] + [torch.empty(n, device=dev) for _ in ones]
    for u in range(n_up):
        for e, o in zip([multi] + ones, outs):
            e.update_device(slabs[u].data_ptr(), CHUNK, o.data_ptr(), st, keep=u >= n_up // 2)
        torch.cuda.synchronize()
        got = outs[0].cpu().numpy().reshape(K, n)
        for m in range(K):
            assert np.array_equal(got[m], outs[1 + m].cpu().numpy()), (K, u, m)


def test_one_model_through_create_models_equals_create(stock_weights):
    n = 300
    pcm = _pcm(np.random.default_rng(3), 8, n)
    a = HipEngine(P.pr, [stock_weights], n_streams=n)
    b = HipEngine(P.pr, stock_weights, n_streams=n)
    for u in range(8):
        ra, rb = a.update(pcm[u]), b.update(pcm[u])
        assert ra.shape == (1, n) and np.array_equal(ra[0], rb), u


@pytest.mark.parametrize('gp,tol', [('f32', 1e-4), ('bf16', 1e-2)])
def test_each_block_matches_the_oracle(stock_weights, gp, tol):
    from mycroft_precise_amd.network_runner import MultiModelListener
    n, n_up = 64, 200
    models = _models(stock_weights)
    pcm = _pcm(np.random.default_rng(11), n_up, n)
    hip = MultiModelListener(models, n, gru_precision=gp, ring_precision=gp)
    refs = [ol.BatchedOracle(w, n) for w in models]
    worst = 0.0
    for u in range(n_up):
        got = hip.update_raw(pcm[u])
        for m, r in enumerate(refs):
            worst = max(worst, float(np.abs(got[m].astype(np.float64) - r.update_raw(pcm[u])).max()))
    assert worst <= tol, worst


def test_decoder_and_trigger_per_model(stock_weights):
    from mycroft_precise_amd.network_runner import MultiModelListener
    from mycroft_precise_amd.runner import TriggerDetector
    from mycroft_precise_amd.threshold_decoder import ThresholdDecoder
    n, n_up = 40, 60
    models = _models(stock_weights)
    hip = MultiModelListener(models, n)
    decs = [ThresholdDecoder(((6, 4),), 0.2), ThresholdDecoder(((6, 4), (4, 3)), 0.5), ThresholdDecoder(((5, 2),), 0.8)]
    trig = [(2048, 0.3, 1), (1024, 0.6, 2), (4096, 0.9, 0)]
    for m in range(3):
        hip.engine.set_decoder(decs[m], model=m)
        hip.set_trigger(*trig[m], model=m)
    dets = [[TriggerDetector(*trig[m]) for _ in range(n)] for m in range(3)]
    pcm = _pcm(np.random.default_rng(5), n_up, n)
    for u in range(n_up):
        raw = hip.update_raw(pcm[u])
        conf, fired = hip.engine.decode(raw, want_fired=True)
        assert conf.shape == fired.shape == (3, n)
        for m in range(3):
            assert np.array_equal(conf[m], decs[m].decode_many(raw[m])), (u, m)
            assert np.array_equal(fired[m], np.array([d.update(float(c)) for d, c in zip(dets[m], conf[m])])), (u, m)
    # crafted raw outputs (bursts near 1 between lulls) so that every model fires and re-arms
    rng = np.random.default_rng(2)
    total = np.zeros(3, int)
    for u in range(120):
        burst = np.sin((np.arange(n) * 0.7 + u) / 5.0) > 0.2
        raw = np.stack([np.clip(np.where(burst, 1 - 1e-4 * rng.random(n), 1e-3 * rng.random(n)), 1e-7, 1 - 1e-7)
                        for _ in range(3)]).astype(np.float32)
        conf, fired = hip.engine.decode(raw, want_fired=True)
        for m in range(3):
            assert np.array_equal(fired[m], np.array([d.update(float(c)) for d, c in zip(dets[m], conf[m])])), (u, m)
        total += fired.sum(axis=1)
    assert (total > 0).all(), total


def test_refusals_and_capacity_smoke(stock_weights):
    w2 = _models(stock_weights)[:2]
    e = HipEngine(P.pr, w2, n_streams=32)
    assert e._lib.pe_get_n_models(e._h) == 2
    with pytest.raises(NotImplementedError):
        e.set_input_projection(True)
    e.close()
    # K = 8 at 65 536 streams runs; 256 streams of every model against the oracle
    n, K, n_up = 65536, 8, 40
    models = [stock_weights] + [synth.make_weights(seed=600 + k) for k in range(K - 1)]
    big = HipEngine(P.pr, models, n_streams=n)
    rng = np.random.default_rng(9)
    pick = np.sort(rng.choice(n, size=256, replace=False))
    refs = [ol.BatchedOracle(w, 256) for w in models]
    sample = _pcm(rng, n_up, 256)
    worst = 0.0
    for u in range(n_up):
        pcm = np.zeros((n, CHUNK), dtype='<i2')
        pcm[pick] = sample[u]
        got = big.update(pcm)
        assert got.shape == (K, n)
        for m in range(K):
            worst = max(worst, float(np.abs(got[m, pick].astype(np.float64) - refs[m].update_raw(sample[u])).max()))
    assert worst <= 1e-4, worst
