"""Objective figures of a synthesis against its recording, computed on the GPU (`HipEngine.mel_dtw`, tts_hip_mel_dtw).

Mel-cepstral distortion along a dynamic-time-warping path (MCD-DTW): the two mels are not aligned in time, so each frame of
one is compared with the frame of the other the cheapest monotone path pairs it with.  The cepstra are the orthonormal DCT-II
of the model's own log-mel (coefficients 1 .. n_cep), not WORLD / SPTK mel-cepstra: figures are comparable between
checkpoints of one mel configuration, not with published MCD tables.
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
