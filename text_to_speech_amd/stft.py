"""Mel analysis objects: `MelSTFT`, `TacotronSTFT` and `WhisperSTFT` of utils/audio/stft.py, computed by the engine's mel plans.

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


_mel_classes = {k: v for k, v in list(globals().items()) if isinstance(v, type) and issubclass(v, MelSTFT)}
