"""numpy restatement of the reference's waveform clean-up (the checker of the GPU path; the product never imports it).

reduce_noise:  utils/audio/audio_processing.py:65-83 -> utils/audio/noisereducev1.py:175-290 (v1 defaults, librosa >= 0.10
               centre padding = zeros)
trim_silence:  utils/audio/audio_processing.py:274-370 (method='window', reference defaults)
normalize:     utils/audio/audio_processing.py:50-62 (normalize_audio)
Only numpy: the Hann window is written in closed form and the 5 x 9 mask smoothing as a direct stencil.
"""
from __future__ import annotations

import numpy as np

N_FFT, HOP = 2048, 512


def normalize_audio(audio, max_val=1.):
    # audio_processing.py:50-62 (max_val <= 1 -> float32 result)
    dtype = np.float32 if max_val <= 1. else np.int16
    audio = audio - np.mean(audio)
    m = np.max(np.abs(audio))
    if m <= 1e-9:
        return audio.astype(dtype)
    return (audio * (max_val / m)).astype(dtype)


def hann(n=N_FFT):
    # scipy.signal.get_window('hann', n, fftbins=True): periodic Hann
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def stft(y, dft='f64'):
    """librosa.stft(y, n_fft=2048, hop_length=512, win_length=2048, center=True, pad_mode='constant') (noisereducev1.py:35-38).
    dft='f32' does the windowed DFT as an fp32 matrix product (the GPU's form)."""
    y = np.asarray(y, dtype=np.float32)
    yp = np.pad(y, N_FFT // 2)                                        # centre padding with zeros
    F = 1 + (len(yp) - N_FFT) // HOP
    idx = np.arange(F)[:, None] * HOP + np.arange(N_FFT)[None]
    frames = yp[idx]
    w = hann()
    if dft == 'f32':
        k = np.arange(N_FFT // 2 + 1)
        ang = 2 * np.pi * ((k[:, None] * np.arange(N_FFT)[None]) % N_FFT) / N_FFT
        cb = (np.cos(ang) * w).astype(np.float32)
        sb = (-np.sin(ang) * w).astype(np.float32)
        return (cb @ frames.T.astype(np.float32)) + 1j * (sb @ frames.T.astype(np.float32))
    return np.fft.rfft(frames.astype(np.float64) * w, axis=1).T.astype(np.complex64)     # [1025, F]


def istft(S, length):
    """librosa.istft(S, hop_length=512, win_length=2048) + librosa.util.fix_length(size=length) (noisereducev1.py:41-42, 281-282)."""
    F = S.shape[1]
    w = hann()
    frames = np.fft.irfft(S, n=N_FFT, axis=0).T * w                  # [F, 2048]
    n = N_FFT + HOP * (F - 1)
    y = np.zeros(n)
    wss = np.zeros(n)
    for f in range(F):
        y[f * HOP:f * HOP + N_FFT] += frames[f]
        wss[f * HOP:f * HOP + N_FFT] += w ** 2                         # window_sumsquare
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    y = y[N_FFT // 2:-(N_FFT // 2)]                                   # centre trim
    out = np.zeros(length)
    m = min(length, len(y))
    out[:m] = y[:m]
    return out


def amp_to_db(mag):
    # librosa.amplitude_to_db(x, ref=1.0, amin=1e-20, top_db=80.0) (noisereducev1.py:66-67)
    p = np.asarray(mag, np.float32) ** 2
    with np.errstate(divide='ignore'):
        db = np.maximum(10.0 * np.log10(p), np.float32(-400.0))         # = 10 log10(max(p, 1e-40)), without the fp32 denormal
    return np.maximum(db, db.max() - 80.0)


# _smoothing_filter(2, 4) (noisereducev1.py:81-106): outer([1,2,3,2,1]/3, [1,2,3,4,5,4,3,2,1]/5) / 15
SMOOTH_F = np.array([1, 2, 3, 2, 1], np.float64)
SMOOTH_T = np.array([1, 2, 3, 4, 5, 4, 3, 2, 1], np.float64)


def smooth_mask(mask):
    # scipy.signal.fftconvolve(mask, filter, mode='same') (noisereducev1.py:142) as a direct 5 x 9 stencil, zero outside
    K, F = mask.shape
    mp = np.zeros((K + 4, F + 8))
    mp[2:2 + K, 4:4 + F] = mask
    out = np.zeros((K, F))
    for i in range(5):
        for j in range(9):
            out += SMOOTH_F[i] * SMOOTH_T[j] * mp[i:i + K, j:j + F]
    return out / 225.0


def reduce_noise(audio, noise=None, noise_length=None, rate=None, dft='f64'):
    """audio_processing.reduce_noise(audio, rate=rate[, noise=noise]) with noisereducev1's defaults.  float64 result."""
    audio = np.asarray(audio, np.float32)
    if noise is None:
        if noise_length is None:
            noise_length = 0.2
        if isinstance(noise_length, float):
            noise_length = int(noise_length * rate)                 # audio_processing.py:71-73
        noise = audio[:noise_length]
    nsamp = len(audio)
    sig = stft(np.pad(audio, [0, HOP]), dft)                          # pad_clipping (noisereducev1.py:225-228)
    sig_db = amp_to_db(np.abs(sig))
    noise_db = amp_to_db(np.abs(stft(noise, dft)))                    # noisereducev1.py:240-243
    mean = np.mean(noise_db.astype(np.float64), axis=1)
    std = np.std(noise_db.astype(np.float64), axis=1)
    thresh = (mean + 1.5 * std).astype(np.float32)                   # n_std_thresh 1.5 (noisereducev1.py:245-247)
    mask = (sig_db < thresh[:, None]).astype(np.float64)             # noisereducev1.py:252-259
    mask = smooth_mask(mask)                                          # noisereducev1.py:262-266
    S = sig * (1 - mask * 1.0)                                        # prop_decrease 1.0, mask_signal
    return istft(S, nsamp)                                            # noisereducev1.py:276-282


def read_wav(path):
    from scipy.io import wavfile
    return wavfile.read(path)


def trim_window(audio, rate, threshold=0.1, window_length=0.2, add_start=0, add_end=1.5, mode='start_end',
                max_trim_factor=5):
    """trim_silence_window (audio_processing.py:274-370) with power 2, triangular window, adaptive thresholds.
    Returns (start, end) with trimmed = audio[start:end]."""
    audio = np.asarray(audio, np.float32)
    if isinstance(window_length, float):
        window_length = int(window_length * rate)
    window = np.concatenate([np.linspace(0, 1, window_length // 2),
                             np.linspace(1, 0, window_length // 2)]) / (window_length // 2)
    conv = np.convolve(np.power(audio, 2), window, mode='valid')
    return trim_bounds(conv, len(audio), window_length, threshold, add_start, add_end, mode, max_trim_factor)


def trim_bounds(conv, L, window_length, threshold=0.1, add_start=0, add_end=1.5, mode='start_end', max_trim_factor=5):
    """The thresholds and indices of trim_silence_window (audio_processing.py:340-370) from its convolution `conv` of a row
    of L samples; window_length in samples."""
    start, end = 0, L
    if 'end' in mode:
        th_end = min(threshold, max(np.mean(conv[-window_length:]) * 5, threshold / 50))
        idx = np.where(conv > th_end)[0]
        if len(idx) > 0:
            end = min(L, idx[-1] + int(window_length * add_end))
    if 'start' in mode:
        th_start = min(threshold, max(np.mean(conv[:window_length]) * 5, threshold / 50))
        idx = np.where(conv > th_start)[0]
        if len(idx) > 0:
            start = max(0, idx[0] - int(window_length * add_start))
    if max(0, end - start) > L // max_trim_factor:
        return start, end
    return 0, L
