"""Objective figures of a synthesis against its recording, computed on the GPU (`HipEngine.mel_dtw`, tts_hip_mel_dtw;
`HipEngine.f0_error`, tts_hip_f0_error).

Mel-cepstral distortion along a dynamic-time-warping path (MCD-DTW): the two mels are not aligned in time, so each frame of
one is compared with the frame of the other the cheapest monotone path pairs it with.  The cepstra are the orthonormal DCT-II
of the model's own log-mel (coefficients 1 .. n_cep), not WORLD / SPTK mel-cepstra: figures are comparable between
checkpoints of one mel configuration, not with published MCD tables.

F0 error: two pitch tracks (`pitch.estimate_f0`) compared along the same path -- the RMSE of the voiced pairs in cents, the
voicing (V/UV) error rate and the gross pitch error rate (voiced pairs more than 20 % apart).
"""
from __future__ import annotations

import numpy as np

MCD_DB_FACTOR = 10.0 * np.sqrt(2.0) / np.log(10.0)      # mcd [dB] = MCD_DB_FACTOR * (mean cepstral distance along the path)


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def mel_cepstral_distortion(engine, a, b, lengths_a=None, lengths_b=None, *, n_cep=13, include_c0=False, align=True, stream=None):
    """MCD of log-mels `a` [B, Ta, n_mel] against `b` [B, Tb, n_mel] (`lengths_*`: the real frames of each row) on `engine`, a
    `HipEngine` or a `HipRuntime` -> {'mcd' (dB), 'cost' (the summed cepstral distance along the path), 'path_len'}, each [B]:
    numpy for numpy operands, CUDA tensors if either operand is one.  `align=False`: frame t against frame t, no warping."""
    stats = engine.mel_dtw(a, b, lengths_a, lengths_b, n_cep=n_cep, include_c0=include_c0, align=align, stream=stream)
    return {'mcd': stats[2], 'cost': stats[0], 'path_len': stats[1]}


def dtw_path(engine, a, b, lengths_a=None, lengths_b=None, *, n_cep=13, include_c0=False):
    """The warping paths of `mel_cepstral_distortion`: a list of B int32 arrays [path_len, 2], the frame pairs (i, j) of row b
    from (0, 0) to (lengths_a[b] - 1, lengths_b[b] - 1)."""
    stats, path = engine.mel_dtw(a, b, lengths_a, lengths_b, n_cep=n_cep, include_c0=include_c0, return_path=True)
    stats, path = _to_numpy(stats), _to_numpy(path)
    return [path[r, :int(stats[1, r])].copy() for r in range(path.shape[0])]


F0_STATS = ('pairs', 'voiced_pairs', 'rmse_cents', 'mean_cents', 'vuv_errors', 'gross_errors')


def f0_error(engine, f0_a, f0_b, lengths_a=None, lengths_b=None, path=None, **kwargs):
    """F0 tracks `f0_a` [B, Fa] against `f0_b` [B, Fb] (Hz, voiced iff > 0; `lengths_*`: the real frames of each row) along
    `path` on `engine`, a `HipEngine` or a `HipRuntime`; `kwargs`: `gross_cents`, `stream`.  `path`: None (the diagonal), the
    [B, P, 2] array or CUDA tensor of `mel_dtw(return_path=True)` -- taken as it is, it does not leave the GPU -- or the list
    `dtw_path` returns.  -> a dict of the six F0_STATS, each [B], plus 'vuv_error' = vuv_errors / pairs and 'gross_error' =
    gross_errors / voiced_pairs (0 where the denominator is): numpy for numpy operands, CUDA tensors if any operand is one."""
    if isinstance(path, (list, tuple)):
        P = max(1, max(len(p) for p in path))
        dense = np.full((len(path), P, 2), -1, np.int32)
        for r, p in enumerate(path):
            dense[r, :len(p)] = p
        path = dense
    stats = engine.f0_error(f0_a, f0_b, lengths_a, lengths_b, path, **kwargs)
    out = {name: stats[k] for k, name in enumerate(F0_STATS)}
    one = stats[0] * 0 + 1
    out['vuv_error'] = stats[4] / (stats[0] + (stats[0] == 0) * one)
    out['gross_error'] = stats[5] / (stats[1] + (stats[1] == 0) * one)
    return out
