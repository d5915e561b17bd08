"""Analysis objects of utils/audio/stft.py -- `MelSTFT`, `TacotronSTFT`, `WhisperSTFT` and the plain `STFT` (magnitude and
phase, with an inverse the reference's class only prepares) -- computed by the engine's mel plans.

The classes carry the reference's constructor arguments, defaults and `get_config()` keys, so a model directory's
`saving/mel_fn.json` is read with `MelSTFT.create(path)` / `load_from_file` and written with `save`.  The arithmetic lives in
csrc/mel_stft.hip: an object is bound to a `HipEngine` (`engine=` at construction or `.bind(engine)`) and `__call__` runs
`HipEngine.mel_fn_run` on the plan of its configuration.  There is no CPU path: a call on an unbound object raises.

One difference from the reference: `normalize_mode='all_feature'` reduces over each row's own cells, not over the whole
batch -- a row's result never depends on its neighbours (include/tts_hip.h).
"""
from __future__ import annotations

import json
import math
import os

import numpy as np


def _samples(value, sampling_rate):
    """A length in samples, or in seconds when <= 1 (stft.py:51-55)."""
    return value if value > 1. else int(value * sampling_rate)


class MelSTFT:
    kind = None                                         # the engine's plan kind; None: an abstract analysis

    def __init__(self, sampling_rate, n_mel_channels=80, *, win_length=1024, hop_length=256, filter_length=1024, mel_fmin=0.0,
                 mel_fmax=8000.0, normalize_mode=None, pre_emph=0., engine=None, **kwargs):
        if normalize_mode not in (None, 'per_feature', 'all_feature'):
            raise ValueError(f"normalize_mode must be None, 'per_feature' or 'all_feature', got {normalize_mode!r}")
        self.n_mel_channels = n_mel_channels
        self.sampling_rate = sampling_rate
        self.win_length = _samples(win_length, sampling_rate)
        self.hop_length = _samples(hop_length, sampling_rate)
        self.filter_length = _samples(filter_length, sampling_rate)
        self.mel_fmin = mel_fmin
        self.mel_fmax = mel_fmax
        self.pre_emph = pre_emph
        self.normalize_mode = normalize_mode
        self._engine = engine

    @property
    def rate(self):
        return self.sampling_rate

    def __str__(self):
        config = self.get_config()
        des = '\n========== {} ==========\n'.format(config.pop('class_name'))
        for k, v in config.items():
            des += '{}\t: {}\n'.format(k, v)
        return des

    def bind(self, engine):
        """Use `engine` for the calls that follow (its plan of this configuration is created on first use).  -> self."""
        self._engine = engine
        return self

    def _plan(self):
        raise NotImplementedError(f'{type(self).__name__} has no mel_spectrogram')

    def __call__(self, audio, lengths=None, stream=None):
        """audio [N] or [B, N] -> mel [B, F, n_mel_channels]; row b holds lengths[b] samples (default N).  numpy in -> numpy
        out, a CUDA tensor in -> a CUDA tensor out (`HipEngine.mel_fn_run`)."""
        if self._engine is None:
            raise RuntimeError(f'{type(self).__name__}: no engine (pass engine= or call .bind(engine)); there is no CPU path')
        plan = self._plan()
        return self._engine.mel_fn_run(plan, audio, lengths=lengths, stream=stream)

    def get_mel_length(self, audio_length):
        return int(math.ceil(max(self.filter_length, audio_length) / self.hop_length))

    def get_audio_length(self, mel_length):
        return mel_length * self.hop_length

    def get_config(self):
        return {
            'class_name': self.__class__.__name__,
            'n_mel_channels': self.n_mel_channels,
            'sampling_rate': self.sampling_rate,
            'win_length': self.win_length,
            'hop_length': self.hop_length,
            'filter_length': self.filter_length,
            'mel_fmin': self.mel_fmin,
            'mel_fmax': self.mel_fmax,
            'pre_emph': self.pre_emph,
            'normalize_mode': self.normalize_mode,
        }

    def save(self, filename):
        if not filename.endswith('.json'):
            filename += '.json'
        with open(filename, 'w', encoding='utf-8') as f:
            json.dump(self.get_config(), f, indent=4)
        return filename

    save_to_file = save

    @classmethod
    def load_from_file(cls, filename, **kwargs):
        return MelSTFT.create(filename, **kwargs)

    @staticmethod
    def create(class_name, *args, **kwargs):
        """An object of the class named `class_name`, or of the configuration in the json file of that name (`engine=` and
        other keywords are passed on)."""
        if class_name in _mel_classes:
            return _mel_classes[class_name](*args, **kwargs)
        if os.path.isfile(class_name):
            with open(class_name, encoding='utf-8') as f:
                config = json.load(f)
            return MelSTFT.create(**{**config, **kwargs})
        raise ValueError('Unknown Mel STFT class !\n  Accepted : {}\n  Got : {}'.format(tuple(_mel_classes.keys()), class_name))


class TacotronSTFT(MelSTFT):
    kind = 'tacotron'

    def __init__(self, sampling_rate=22050, n_mel_channels=80, *, window='hann', periodic=True, **kwargs):
        super().__init__(sampling_rate=sampling_rate, n_mel_channels=n_mel_channels, **kwargs)
        if self.filter_length < self.win_length:
            raise ValueError(f'filter_length = {self.filter_length} < win_length = {self.win_length}')
        self.window = window
        self.periodic = periodic

    def fft_window(self):
        """float64 [win_length] (scipy.signal.get_window(window, win_length, fftbins=periodic)), or None for the periodic
        Hann window, which the engine builds itself."""
        if self.window == 'hann' and self.periodic:
            return None
        from scipy.signal import get_window
        return np.asarray(get_window(self.window, self.win_length, fftbins=bool(self.periodic)), dtype=np.float64)

    def _plan(self):
        cfg = {k: v for k, v in MelSTFT.get_config(self).items() if k != 'class_name'}
        return self._engine.mel_fn(dict(cfg, kind=self.kind), window=self.fft_window())

    @property
    def stft_fn(self):
        """The `STFT` of this geometry, bound to the same engine and sharing this object's plan (stft.py:298-305).  Sharing the
        plan means sharing its steps 1 - 3: with `pre_emph > 0` this `stft_fn` transforms the pre-emphasised signal (and
        zero-pads a row shorter than win_length), which the reference's bare `stft_fn` does not -- build an `STFT` of the
        same geometry for the plain transform."""
        fn = STFT(filter_length=self.filter_length, hop_length=self.hop_length, win_length=self.win_length, window=self.window,
                  periodic=self.periodic, engine=self._engine)
        fn._plan = self._plan
        return fn

    def mel_to_audio(self, mel, lengths=None, n_iters=60, momentum=0.99, init=None, seed=None, streams=None, stream=None):
        """Griffin-Lim over this object's STFT: log-mel [F, n_mel] or [B, F, n_mel] (what `__call__` returns) -> audio
        [B, F * hop_length]; row b holds lengths[b] frames (default F).  The magnitudes are max(0, exp(mel) . Minv) with Minv
        the minimum-norm inverse of the filterbank.  `init` [B, F, bins, 2] is the initial phase as (re, im) pairs; with
        `seed` it is drawn on the device instead, row b's pairs of normals (a normalised pair is uniform on the circle) from
        the row's own Philox stream `runtime.stream_key(seed, PHASE_STREAM, *streams[b])` (streams: one (utterance, part) id
        per row, default (b, 0)), so a seeded row's audio does not depend on its batch."""
        if self._engine is None:
            raise RuntimeError(f'{type(self).__name__}: no engine (pass engine= or call .bind(engine)); there is no CPU path')
        plan = self._plan()
        if seed is not None:
            if init is not None:
                raise ValueError('mel_to_audio: init excludes seed')
            init = seeded_phase(self._engine, mel, self.filter_length // 2 + 1, seed, streams, stream)
            if not hasattr(mel, 'is_cuda'):
                init = init.cpu().numpy()
        return self._engine.griffin_lim(plan, mel, frames=lengths, kind='log_mel', n_iters=n_iters, momentum=momentum, init=init,
                                        stream=stream)

    def get_config(self):
        config = super().get_config()
        config.update({
            'filter_length': self.filter_length,
            'hop_length': self.hop_length,
            'win_length': self.win_length,
            'window': self.window,
            'to_magnitude': True,
            'periodic': self.periodic,
        })
        return config


class WhisperSTFT(TacotronSTFT):
    kind = 'whisper'

    def __init__(self, sampling_rate=16000, n_mel_channels=80, *, win_length=400, hop_length=160, filter_length=400, mel_fmin=0.0,
                 mel_fmax=8000.0, **kwargs):
        super().__init__(sampling_rate=sampling_rate, n_mel_channels=n_mel_channels, win_length=win_length, hop_length=hop_length,
                         filter_length=filter_length, mel_fmin=mel_fmin, mel_fmax=mel_fmax, **kwargs)


PHASE_STREAM = 3                                        # `purpose` of runtime.stream_key for the Griffin-Lim initial phase


def seeded_phase(engine, spec, bins, seed, streams=None, stream=None):
    """float32 CUDA [B, F, bins, 2] normals for a spec [F, C] or [B, F, C]: row b is the head of its own Philox stream."""
    from .runtime import _row_ids, stream_key
    shape = tuple(spec.shape)
    B, F = (1, int(shape[0])) if len(shape) == 2 else (int(shape[0]), int(shape[1]))
    ids = _row_ids(streams, B, 2) if streams is not None else [(b, 0) for b in range(B)]
    keys = [stream_key(seed, PHASE_STREAM, *i) for i in ids]
    return engine.random_normal_rows(F * bins * 2, keys, 0, stream=stream).view(B, F, bins, 2)


class STFT:
    """utils/audio/stft.py:185-284: the windowed DFT as magnitude and phase (`to_magnitude=False`: real and imaginary parts,
    "equivalent of torch.stft"), computed by the engine (csrc/stft_inv.hip) on the plan of a TacotronSTFT of the same
    geometry.  `inverse` is new: the windowed pseudo-inverse basis the reference builds, used for what it is -- complex
    spectrogram -> audio.  `window=None` is a rectangular window.  There is no CPU path."""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window='hann', to_magnitude=True, periodic=True, *,
                 engine=None):
        if filter_length < win_length:
            raise ValueError(f'filter_length = {filter_length} < win_length = {win_length}')
        self.filter_length = filter_length
        self.hop_length = hop_length
        self.win_length = win_length
        self.window = window
        self.to_magnitude = to_magnitude
        self.periodic = periodic
        self._engine = engine

    def bind(self, engine):
        self._engine = engine
        return self

    def fft_window(self):
        if self.window is None:
            return np.ones(self.win_length, dtype=np.float64)
        if self.window == 'hann' and self.periodic:
            return None
        from scipy.signal import get_window
        return np.asarray(get_window(self.window, self.win_length, fftbins=bool(self.periodic)), dtype=np.float64)

    def _plan(self):
        # the analysis needs no filterbank: the mel fields only have to pass the plan's checks
        cfg = dict(kind='tacotron', sampling_rate=22050, n_mel_channels=1, filter_length=self.filter_length,
                   hop_length=self.hop_length, win_length=self.win_length, mel_fmin=0.0, mel_fmax=11025.0)
        return self._need_engine().mel_fn(cfg, window=self.fft_window())

    def _need_engine(self):
        if self._engine is None:
            raise RuntimeError('STFT: no engine (pass engine= or call .bind(engine)); there is no CPU path')
        return self._engine

    @staticmethod
    def _stack(a, b):
        if isinstance(a, np.ndarray):
            return np.stack([a, b], axis=-1)
        import torch
        return torch.stack([a, b], dim=-1)

    def __call__(self, audio, lengths=None):
        return self.transform(audio if len(audio.shape) > 1 else audio[None, :], lengths)[0]

    def transform(self, audio, lengths=None):
        """audio [B, N] -> (magnitude, phase), each [B, F, filter_length // 2 + 1]; with to_magnitude=False the first is the
        real and imaginary parts stacked on a last axis of 2 (stft.py:242-274).  The engine returns two planes per call, so
        to_magnitude=False costs two runs of the transform: one for the phase, one for the parts."""
        eng, plan = self._need_engine(), self._plan()
        magnitude, phase = eng.stft_transform(plan, audio, lengths=lengths, polar=True)
        if not self.to_magnitude:
            magnitude = self._stack(*eng.stft_transform(plan, audio, lengths=lengths, polar=False))
        return magnitude, phase

    def inverse(self, magnitude, phase=None, frames=None):
        """(magnitude, phase), or one [..., 2] array of real and imaginary parts -> audio [B, F * hop_length]; row b holds
        hop * (frames[b] - 1) + filter_length - 2 * (filter_length // 2) samples (default F frames), zeros beyond."""
        eng, plan = self._need_engine(), self._plan()
        if phase is None:
            if magnitude.shape[-1] != 2:
                raise ValueError(f'inverse: without a phase the input must be [..., 2] real / imaginary parts, got {tuple(magnitude.shape)}')
            return eng.stft_inverse(plan, magnitude[..., 0], magnitude[..., 1], frames=frames, polar=False)
        return eng.stft_inverse(plan, magnitude, phase, frames=frames, polar=True)

    def get_config(self):
        return {
            'filter_length': self.filter_length,
            'hop_length': self.hop_length,
            'win_length': self.win_length,
            'window': self.window,
            'to_magnitude': self.to_magnitude,
            'periodic': self.periodic,
        }


_mel_classes = {k: v for k, v in list(globals().items()) if isinstance(v, type) and issubclass(v, MelSTFT)}
