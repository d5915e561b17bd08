"""Pitch tracks on the GPU: YIN (`HipEngine.pitch`, tts_hip_pitch; de Cheveigne & Kawahara 2002, steps 1 to 5) and probabilistic
YIN (`HipEngine.pyin`, tts_hip_pyin; Mauch & Dixon 2014: every trough of d' a candidate, a Viterbi decode over pitch bins and
voicing) on ragged batches of recordings.  The frame grid is the default mel plan's: with hop = 256, a recording of 1024 samples
or more has as many pitch frames as mel frames, and frame t is centred where mel frame t is.
"""
from __future__ import annotations

import math

PITCH_DEFAULTS = dict(rate=22050, hop=256, win=1024, fmin=60., fmax=500., threshold=0.1)


def hz_to_lags(rate, fmin, fmax):
    """The lags a search between `fmin` and `fmax` Hz covers at `rate` samples a second -> (tau_min, tau_max) =
    (ceil(rate / fmax), floor(rate / fmin)): 45 and 367 at the defaults."""
    if not (fmin == fmin and fmax == fmax and 0 < fmin < fmax < math.inf):
        raise ValueError(f'fmin = {fmin!r} and fmax = {fmax!r} must satisfy 0 < fmin < fmax')
    if rate != int(rate) or int(rate) < 1:
        raise ValueError(f'rate = {rate!r} must be a positive integer')
    return int(math.ceil(int(rate) / fmax)), int(math.floor(int(rate) / fmin))


def frame_count(n, hop=256):
    """Frames of a row of `n` samples: 1 + n // hop"""
    return 1 + int(n) // int(hop)


PYIN_DEFAULTS = dict(rate=22050, hop=256, win=1024, fmin=60., fmax=500., bins_per_semitone=10, beta=(2, 18), n_thresholds=100,
                     max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01)
F0_METHODS = ('yin', 'pyin')


def beta_cdf(x, a, b):
    """The regularised incomplete beta function I_x(a, b) for integers a, b >= 1: the finite binomial sum
    sum_{j = a}^{a + b - 1} C(a + b - 1, j) x^j (1 - x)^(a + b - 1 - j), in float64."""
    if a != int(a) or b != int(b) or int(a) < 1 or int(b) < 1:
        raise ValueError(f'a = {a!r} and b = {b!r} must be integers of at least 1')
    a, b, x = int(a), int(b), float(x)
    n = a + b - 1
    return math.fsum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1))


def beta_prior(a=2, b=18, n=100):
    """The prior of pYIN's thresholds s_i = i / n, i = 1 .. n: the Beta(a, b) mass of each threshold's bin, prior[i - 1] =
    I(s_i) - I(s_{i - 1}) (`beta_cdf`) -> float64 [n], summing to 1."""
    import numpy as np
    if n != int(n) or int(n) < 1:
        raise ValueError(f'n = {n!r} must be a positive integer')
    cdf = np.array([beta_cdf(i / int(n), a, b) for i in range(int(n) + 1)])
    return np.diff(cdf)


def pyin_geometry(rate, hop, fmin, fmax, bps=10, max_transition_rate=35.92):
    """The pitch bins and the largest step of pYIN's decode -> (n_bins, max_step): `bps` bins a semitone from `fmin` up,
    n_bins = floor(12 bps log2(fmax / fmin)) + 1 (368 at the defaults); a track moves at most `max_transition_rate` octaves a
    second, max_step = round(max_transition_rate 12 bps hop / rate) + 1 bins a frame (51 at the defaults)."""
    hz_to_lags(rate, fmin, fmax)
    if bps != int(bps) or int(bps) < 1:
        raise ValueError(f'bps = {bps!r} must be a positive integer')
    if hop != int(hop) or int(hop) < 1:
        raise ValueError(f'hop = {hop!r} must be a positive integer')
    if not (max_transition_rate == max_transition_rate and 0 <= max_transition_rate < math.inf):
        raise ValueError(f'max_transition_rate = {max_transition_rate!r} must be finite and not negative')
    n_bins = int(math.floor(12 * int(bps) * math.log2(fmax / fmin))) + 1
    max_step = int(round(max_transition_rate * 12 * int(bps) * int(hop) / int(rate))) + 1
    return n_bins, max_step


def track_f0(engine, method, audio, lengths=None, stream=None, **cfg):
    """The tracker `method` ('yin': `engine.pitch`, 'pyin': `engine.pyin`) with its keywords `cfg` -> float32 [3, B, F]; plane 0
    is f0 in Hz, 0 where unvoiced, under either."""
    if method not in F0_METHODS:
        raise ValueError(f'the F0 method must be one of {F0_METHODS}, got {method!r}')
    call = getattr(engine, 'pitch' if method == 'yin' else 'pyin', None)
    if call is None:
        raise ValueError(f"F0 method {method!r} needs `{'pitch' if method == 'yin' else 'pyin'}` on the engine")
    return call(audio, lengths, **cfg) if stream is None else call(audio, lengths, stream=stream, **cfg)


def estimate_f0(engine, audio, lengths=None, method='yin', **cfg):
    """The pitch of `audio` [B, N] (`lengths`: the real samples of each row) on `engine`, a `HipEngine` or a `HipRuntime`; `cfg`:
    the keywords of `HipEngine.pitch` -> {'f0' [B, F] in Hz (0 where unvoiced), 'period' [B, F] in samples, 'aperiodicity' [B, F]
    (d' at the chosen lag: near 0 for a clean tone, near 1 for noise), 'voiced' [B, F] bool, 'frames' [B] the frames of each row}:
    numpy for a numpy operand, CUDA tensors for a CUDA tensor ('frames' is always a host int32 array).  method='pyin': `cfg` are
    the keywords of `HipEngine.pyin`, and in place of 'period' and 'aperiodicity' come 'voiced_prob' [B, F] and 'pitch' [B, F]
    (the decoded bin's pitch in Hz, of unvoiced frames too)."""
    import numpy as np
    out = track_f0(engine, method, audio, lengths, **cfg)
    B, hop = int(out.shape[1]), int(cfg.get('hop', PITCH_DEFAULTS['hop']))
    n = int(np.shape(audio)[-1])
    lens = [n] * B if lengths is None else [int(v) for v in (lengths.detach().cpu().numpy() if hasattr(lengths, 'detach') else np.atleast_1d(lengths))]
    frames = np.asarray([frame_count(v, hop) for v in lens], dtype=np.int32)
    if method == 'pyin':
        return {'f0': out[0], 'pitch': out[1], 'voiced_prob': out[2], 'voiced': out[0] > 0, 'frames': frames}
    return {'f0': out[0], 'period': out[1], 'aperiodicity': out[2], 'voiced': out[0] > 0, 'frames': frames}
