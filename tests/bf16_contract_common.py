"""Shared by test_bf16_contract_host.py (CPU) and test_bf16_contract.py (GPU): the input sets, the networks of the cases
and the two-tier rule by which an evaluation of the bf16 contract is compared with oracle/bf16_gru.py.  Not a test module."""

import numpy as np

from mycroft_precise_amd import synth
from oracle import bf16_gru

T = 29                          # stock params: n_features
MAX_OUTSIDE = 0.03              # tier 1: at most this share of the flip-free windows may lie outside TOL_TIGHT
MIN_FLIP_FREE = 0.95            # input condition: at least this share of every input set is flip-free

# the streams of input set (a)
STREAM_KINDS = ['tone_noise'] * 40 + ['zeros', 'square', 'quiet']
N_UPDATES, CHUNK = 36, 1024


def stream_pcm():
    """int16 [36 updates, 43 streams, 1024 samples]"""
    return np.stack([synth.stream_pcm(s, N_UPDATES * CHUNK, k).reshape(N_UPDATES, CHUNK) for s, k in enumerate(STREAM_KINDS)], axis=1)


def oracle_stream_windows(n_in=13, every=3, **params):
    """input set (a) without a GPU: the oracle's MFCC rows of the same streams, the windows after every ``every``-th update
    (the GPU tests read the windows the engine itself holds, get_vectors(): the front end is not part of the comparison)"""
    from oracle import listener as ol
    pcm = stream_pcm()
    o = ol.BatchedOracle(None, pcm.shape[1], ol.Params(n_mfcc=n_in, **params))
    wins = []
    for u in range(N_UPDATES):
        f = o.update_vectors(pcm[u]).astype(np.float32)
        if u % every == every - 1:
            wins.append(f)
    return np.concatenate(wins)


def normal_batch(n, n_in=13, seed=8):
    """input set (b): normal(0, 2) with the first coefficient where MFCC rows have it"""
    x = np.random.default_rng(seed + n).normal(0, 2, (n, T, n_in)).astype(np.float32)
    x[..., 0] -= np.float32(20)
    return x


# Seeds of set (b) for the stock network, the tie weights and the K = 3 models, per batch size: the first seed from 0 on for
# which the reference stays within 1e-2 of the float32 oracle on the stock network AND every one of those networks has
# >= 95 % flip-free windows.  The first condition is rare: with x[..., 0] -= 20 the state grows far beyond what MFCC rows
# produce, 14 % of such windows lie beyond 1e-2, and of 8000 seeds two give 50 windows within it (522 and 5168).
STOCK_B_SEEDS = {1: 0, 17: 14, 50: 5168}


def stock_normal_batches():
    return [normal_batch(n, seed=STOCK_B_SEEDS[n]) for n in (1, 17, 50)]


def onto_ties(v, which=None):
    """float32 values -> the same values with the low mantissa half replaced by 0x8000: exactly half way between two
    bfloat16 values.  ``which``: bool array, True = make the kept bf16 neighbour odd (round to nearest even goes UP, half-up
    goes up, truncation down), False = even (nearest even goes DOWN, half-up up, truncation down); None keeps the bit."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    u = (u & np.uint32(0xffff0000)) | np.uint32(0x8000)
    if which is not None:
        u = np.where(which, u | np.uint32(0x10000), u & np.uint32(0xfffeffff)).astype(np.uint32)
    return u.view(np.float32)


def tie_batch(n=50, n_in=13, seed=31):
    """input set (c): every feature on a bf16 tie, half of them with an even and half with an odd neighbour below"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, (n, T, n_in)).astype(np.float32)
    odd = (np.arange(x.size).reshape(x.shape) % 2).astype(bool)
    out = onto_ties(x, odd)
    low = out.view(np.uint32) & np.uint32(0x1ffff)
    assert np.all((low == 0x8000) | (low == 0x18000)) and abs(int((low == 0x8000).sum()) * 2 - x.size) <= 1
    return out


def tie_weights(n_in=13, units=20, seed=42):
    """input set (d): synth.make_weights with half of the entries of kernel, recurrent kernel and bias moved onto bf16 ties"""
    w = synth.make_weights(n_in=n_in, units=(units,), seed=seed)
    rng = np.random.default_rng(seed + 1000)
    layer = []
    for a in w['gru'][0]:
        pick = rng.random(a.shape) < 0.5
        layer.append(np.where(pick, onto_ties(a), a).astype(np.float32))
    out = dict(w)
    out['gru'] = [tuple(layer)]
    return out


def with_deltas(x):
    """an explicit use_delta batch (vectorization.py:53-59): [n, T, F] -> [n, T, 2 F], float32 differences"""
    x = np.asarray(x, dtype=np.float32)
    d = np.zeros_like(x)
    d[:, 1:] = x[:, 1:] - x[:, :-1]
    return np.concatenate([x, d], axis=2)


# Seeds of the cases, (units, n_in, use_delta) -> (network, normal batches (b), tie batch (c)): the first seeds, from
# (900, 8, 31) on, for which at least 95 % of the windows of every input set of the case are flip-free -- a property of the
# reference alone, which the host test asserts.  (32 units with use_delta round 64 state operands per timestep: on the
# streamed rows most networks stay at 0.89 .. 0.95, and the first seed that reaches 95 % is 3106.)
CASE_SEEDS = {
    (20, 13, False): (900, 8, 42), (20, 13, True): (900, 11, 35), (17, 14, False): (900, 8, 34), (17, 14, True): (900, 8, 33),
    (7, 5, False): (900, 8, 31), (7, 5, True): (900, 8, 31), (1, 13, False): (900, 8, 31), (1, 13, True): (900, 8, 31),
    (24, 13, False): (901, 8, 37), (24, 13, True): (901, 8, 34), (20, 15, False): (901, 8, 46), (20, 15, True): (901, 8, 46),
    (32, 13, False): (1054, 8, 57), (32, 13, True): (3106, 23, 40),
}
MODEL_SEEDS = (905, 908)        # models 1 and 2 of the K = 3 engine, beside the stock network (chosen by the same rule)


def case_weights(units, n_in, delta, seed=None):
    return synth.make_weights(n_in=2 * n_in if delta else n_in, units=(units,), seed=CASE_SEEDS[(units, n_in, delta)][0] if seed is None else seed)


def case_batches(units, n_in, delta):
    """-> (the normal batches of 1, 17 and 50 windows (b), the tie batch (c)) of a case; with use_delta as explicit batches
    that carry their delta columns"""
    _, bs, cs = CASE_SEEDS[(units, n_in, delta)]
    form = with_deltas if delta else (lambda x: x)
    return [form(normal_batch(n, n_in, seed=bs)) for n in (1, 17, 50)], form(tie_batch(50, n_in, seed=cs))


GENERAL_FRONT_END = dict(n_fft=400, n_filt=26)      # 25 ms transforms: not the stock shape, so the general front end serves it
EVALUATE_STREAM = 4             # synth.stream_pcm(EVALUATE_STREAM, 4 s), the recording of the evaluate case: the first stream
                                # from 3 on whose 25 windows are >= 95 % flip-free without and with use_delta
CLIP_LENGTHS = [24000, 30001, 3300, 1600, 12345, 23999]
CLIP_FIRST_STREAM = 50


def evaluate_audio():
    return synth.stream_pcm(EVALUATE_STREAM, 4 * 16000).astype(np.float64) / 32768.0


def evaluate_windows(frames, hop=2):
    """simulate.py:96-99: the windows ending at frames range(T, n_frames, hop)"""
    frames = np.asarray(frames, dtype=np.float32)
    return np.stack([frames[i - T:i] for i in range(T, len(frames), hop)])


def clips():
    return [synth.stream_pcm(CLIP_FIRST_STREAM + i, n).astype(np.float64) / 32768.0 for i, n in enumerate(CLIP_LENGTHS)]


def huge_batch():
    """16 windows of set (b) with one feature at +-1e4 / +-1e30 over the last three timesteps"""
    x = normal_batch(16)
    for i, v in enumerate([1e4, -1e4, 1e30, -1e30] * 4):
        x[i, -3:, (5 * i) % 13] = np.float32(v)
    return x


def saturated(x, weights):
    """float32 [n]: 0.0 / 1.0 where every variant of the reference, rounded to float32, gives exactly that; NaN elsewhere"""
    p = np.stack([bf16_gru.predict(x, weights, variant=v) for v in bf16_gru.VARIANTS]).astype(np.float32)
    same = np.all(p == p[0], axis=0) & ((p[0] == 0) | (p[0] == 1))
    return np.where(same, p[0], np.float32(np.nan)).astype(np.float32)


def non_finite_batch():
    """-> (clean [40, T, 13], the same with inf, -inf, NaN and 3.4e38 (inf as bf16) in one window each, those windows)"""
    clean = normal_batch(40)
    dirty = clean.copy()
    hit = [3, 12, 21, 38]
    for w, t, f, v in zip(hit, (10, 0, 28, 17), (2, 5, 0, 12), (np.inf, -np.inf, np.nan, 3.4e38)):
        dirty[w, t, f] = np.float32(v)
    return clean, dirty, hit


class Reference:
    """What a case needs of the reference for one set of windows: the float64 evaluation, the flip-free mask, the spread
    of the variants on it."""

    def __init__(self, x, weights, **kw):
        self.mask, self.outs = bf16_gru.flip_free(x, weights, **kw)
        self.ref = self.outs['f64']
        self.share = float(self.mask.mean())
        self.spread = bf16_gru.spread(self.outs, self.mask)


def judge(got, ref, mask, tol_tight, tol_flip):
    """The two-tier rule -> (passes, share of flip-free windows outside tol_tight, largest distance over all windows)."""
    d = np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - ref)
    outside = float((~(d[mask] <= tol_tight)).mean()) if mask.any() else 0.0
    worst = float(np.max(np.where(np.isnan(d), np.inf, d))) if d.size else 0.0
    return outside <= MAX_OUTSIDE and worst <= tol_flip, outside, worst
