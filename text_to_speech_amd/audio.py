"""Audio input path: wav reading, normalization and the device-side clean-up the reference applies while loading.

Mirrors utils/audio/audio_io.py:100-144 (`load_audio`, `load_mel`) and :186-270 (`read_audio`): resample -> normalize ->
reduce_noise -> normalize again -> trim_silence, in that order.  Normalization is host numpy (as in the reference);
resampling, noise reduction and the trim indices run on the GPU (HipEngine.resample / reduce_noise / trim_silence,
csrc/resample.hip, csrc/audio_proc.hip).  Resampling is opt-in (`resample=True`): by default a file at another rate
raises, as before.  It differs from the reference in one way: the reference resamples the raw int16 samples in float64
(scipy.signal.resample), here they become float32 (exactly) and are resampled in fp32 on the device.

`trim_silence` is the reference's public dispatcher (audio_processing.py:84-98) for one row: method 'window' (the trim
indices above), 'rms', 'threshold' and 'remove' (HipEngine.remove_silence, csrc/silence.hip: silence mask and compaction on
the GPU, sample for sample what the reference's numpy gives).  The 'ffmpeg' method shells out to a program and is refused.
`load_audio` itself still takes method='window' only; trim its result with `trim_silence` for the other methods.
"""
from __future__ import annotations

import numpy as np

_RN_KEYS = ('noise', 'noise_length')
_TRIM_KEYS = ('threshold', 'window_length', 'add_start', 'add_end', 'mode')


def read_wav(filename):
    """(rate, samples) of a .wav file (audio_io.py:272-275: scipy.io.wavfile.read)."""
    from scipy.io import wavfile
    return wavfile.read(filename)


def normalize_audio(audio, max_val=32767, dtype=np.int16):
    """audio_processing.py:50-62: zero mean, peak `max_val`; max_val <= 1 gives float32 in [-1, 1]."""
    if max_val <= 1.:
        dtype = np.float32
    audio = audio - np.mean(audio)
    max_audio_val = np.max(np.abs(audio))
    if max_audio_val <= 1e-9:
        return audio.astype(dtype)
    return (audio * (max_val / max_audio_val)).astype(dtype)


def resampled_length(n, rate, target_rate):
    """Samples after resampling n samples from `rate` to `target_rate`: int(n / rate * target_rate), evaluated in this
    order in IEEE double as utils/audio/audio_processing.py:33 does (not n * target_rate // rate: for 11 200 samples at
    16 000 -> 22 050 Hz the two give 15 434 and 15 435).  csrc/resample.hip uses the same expression."""
    if rate <= 0 or target_rate <= 0:
        raise ValueError(f'resample: rates must be > 0 (got {rate}, {target_rate})')
    m = int(int(n) / rate * target_rate)
    if m < 1:
        raise ValueError(f'resample: {n} samples at {rate} -> {target_rate} Hz give {m} < 1 samples')
    return m


def load_audio(data, rate=None, *, engine, normalize=True, reduce_noise=False, trim_silence=False, method='window',
               resample=False, source_rate=None, **kwargs):
    """A filename or raw samples -> float32 [n] (audio_io.py:100-127 + :186-268).  `rate`: the rate the caller wants.
    resample=False: a file at another rate raises.  resample=True: audio at another rate (the file's header, a dict's
    'rate' entry, or `source_rate=` for raw samples) is resampled to `rate` on `engine` before normalization, as the
    reference does.  Raw samples need `rate`.  kwargs: `noise`, `noise_length` for reduce_noise; `threshold`,
    `window_length`, `add_start`, `add_end`, `mode` for trim_silence.  Only method='window' is accepted here; for 'rms',
    'threshold' or 'remove' load without trimming and pass the result to `trim_silence(audio, engine=..., rate=..., method=...)`."""
    if trim_silence and method != 'window':
        raise ValueError(f"trim_silence: only method='window' is implemented (got {method!r})")
    unknown = set(kwargs) - set(_RN_KEYS) - set(_TRIM_KEYS)
    if unknown:
        raise ValueError(f'load_audio: unknown arguments {sorted(unknown)}')
    if isinstance(data, dict):
        if 'rate' in data and resample and source_rate is None:
            source_rate = data['rate']
        if 'rate' in data and rate is None:
            rate = data['rate']
        data = data['audio'] if 'audio' in data else data.get('filename', data.get('audio_filename'))
    if isinstance(data, bytes):
        data = data.decode()
    if isinstance(data, str):
        file_rate, audio = read_wav(data)
        if rate is not None and int(rate) != int(file_rate) and not resample:
            raise ValueError(f'{data} is sampled at {file_rate} Hz, {rate} Hz requested: resampling is off '
                             f'(pass resample=True)')
        source_rate = int(file_rate)
        rate = int(file_rate) if rate is None else rate
    else:
        if rate is None:
            raise ValueError('load_audio: raw audio needs `rate`')
        audio = data.detach().cpu().numpy() if hasattr(data, 'detach') else np.asarray(data)
    if audio.ndim != 1:
        raise ValueError(f'load_audio: expected mono audio [n], got shape {audio.shape}')

    if resample and source_rate is not None and int(source_rate) != int(rate):
        audio = engine.resample(np.asarray(audio, np.float32), int(source_rate), int(rate))

    if normalize:
        if normalize is True:
            audio = normalize_audio(audio, max_val=1.)
        elif normalize > 1 and np.issubdtype(audio.dtype, np.integer):
            audio = (audio / normalize).astype(np.float32)
    if reduce_noise:
        rn = {k: kwargs[k] for k in _RN_KEYS if k in kwargs}
        audio = engine.reduce_noise(np.asarray(audio, np.float32), rate, renormalize=normalize is True, **rn)
    if trim_silence:
        tr = {k: kwargs[k] for k in _TRIM_KEYS if k in kwargs}
        start, end = engine.trim_silence(np.asarray(audio, np.float32), rate, **tr)
        audio = audio[start:end]
    return audio


TRIM_METHODS = ('window', 'rms', 'threshold', 'remove')
_WINDOW_KEYS = ('threshold', 'window_length', 'add_start', 'add_end', 'mode')
_SILENCE_KEYS = ('mode', 'threshold', 'min_silence', 'block_size', 'replace_by', 'min_voice_time')


def trim_silence(audio, *, engine, rate=None, method='window', **kwargs):
    """audio_processing.trim_silence (:84-98) for one row [n] -> the trimmed float32 row.  'window': engine.trim_silence's
    indices, sliced (keywords threshold, window_length, add_start, add_end, mode).  'rms' (mode, threshold in dB, min_silence,
    block_size, replace_by, min_voice_time), 'threshold' (threshold, mode) and 'remove' (the mean-window method: threshold,
    min_silence): engine.remove_silence, which needs `rate`.  A row in which 'rms' finds no silence comes back unchanged
    (the reference raises IndexError unless mode is 'remove').  'ffmpeg' and unknown names raise ValueError."""
    if isinstance(method, bytes):
        method = method.decode()
    if method not in TRIM_METHODS:
        raise ValueError(f'trim_silence: method {method!r} is not supported (supported: {", ".join(TRIM_METHODS)})')
    allowed = _WINDOW_KEYS if method == 'window' else _SILENCE_KEYS
    unknown = set(kwargs) - set(allowed)
    if unknown:
        raise ValueError(f'trim_silence: unknown arguments {sorted(unknown)} for method {method!r}')
    audio = audio.detach().cpu().numpy() if hasattr(audio, 'detach') else np.asarray(audio)
    if audio.ndim != 1:
        raise ValueError(f'trim_silence: expected one row [n], got shape {audio.shape}')
    audio = np.asarray(audio, np.float32)
    if method == 'window':
        start, end = engine.trim_silence(audio, rate, **kwargs)
        return audio[start:end]
    return engine.remove_silence(audio, rate, method=method, **kwargs)


MEL_RATE = 22050                    # TacotronSTFT's sampling rate (engine.mel_stft's filterbank)


def load_mel(data, rate=MEL_RATE, *, engine, stft_fn=None, resample=False, **kwargs):
    """audio_io.py:129-144: load_audio(data, stft_fn.rate, ...) -> mel [T, n_mel].  Without `stft_fn` the analysis is the
    default TacotronSTFT (engine.mel_stft, 22 050 Hz, 80 mels); with one (text_to_speech_amd.stft: any TacotronSTFT
    configuration or WhisperSTFT) the audio is loaded at `stft_fn.rate` and the mel comes from it on `engine`, and an array
    [..., stft_fn.n_mel_channels] is taken for a mel and passed through, as the reference does.  Like the reference, the
    audio is loaded at the STFT's rate: a file at another rate raises unless resample=True, which resamples it on `engine`
    first."""
    if isinstance(data, dict) and 'mel' in data:
        return data['mel']
    if stft_fn is not None:
        if hasattr(data, 'shape') and len(data.shape) >= 2 and data.shape[-1] == stft_fn.n_mel_channels:
            return data
        audio = load_audio(data, stft_fn.rate, engine=engine, resample=resample, **kwargs)
        return stft_fn.bind(engine)(np.asarray(audio, np.float32))[0]
    if rate != MEL_RATE:
        raise ValueError(f'load_mel: the mel-STFT runs at {MEL_RATE} Hz, got rate={rate}')
    audio = load_audio(data, rate, engine=engine, resample=resample, **kwargs)
    return engine.mel_stft(np.asarray(audio, np.float32))[0]
