"""Pitch tracks on the GPU (`HipEngine.pitch`, tts_hip_pitch): YIN (de Cheveigne & Kawahara 2002, steps 1 to 5) on ragged
batches of recordings.  The frame grid is the default mel plan's: with hop = 256, a recording of 1024 samples or more has as many
pitch frames as mel frames, and frame t is centred where mel frame t is.
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


def estimate_f0(engine, audio, lengths=None, **cfg):
    """The pitch of `audio` [B, N] (`lengths`: the real samples of each row) on `engine`, a `HipEngine` or a `HipRuntime`; `cfg`:
    the keywords of `HipEngine.pitch` -> {'f0' [B, F] in Hz (0 where unvoiced), 'period' [B, F] in samples, 'aperiodicity' [B, F]
    (d' at the chosen lag: near 0 for a clean tone, near 1 for noise), 'voiced' [B, F] bool, 'frames' [B] the frames of each row}:
    numpy for a numpy operand, CUDA tensors for a CUDA tensor ('frames' is always a host int32 array)."""
    import numpy as np
    out = engine.pitch(audio, lengths, **cfg)
    B, hop = int(out.shape[1]), int(cfg.get('hop', PITCH_DEFAULTS['hop']))
    n = int(np.shape(audio)[-1])
    lens = [n] * B if lengths is None else [int(v) for v in (lengths.detach().cpu().numpy() if hasattr(lengths, 'detach') else np.atleast_1d(lengths))]
    return {'f0': out[0], 'period': out[1], 'aperiodicity': out[2], 'voiced': out[0] > 0,
            'frames': np.asarray([frame_count(v, hop) for v in lens], dtype=np.int32)}
