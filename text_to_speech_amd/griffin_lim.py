"""`GriffinLim`: a vocoder that needs no second checkpoint -- Griffin-Lim phase reconstruction over the engine's STFT.

It has the contract `Tacotron2._vocode_parts` / `_vocode_group` expect of a vocoder (`vocoder(mel, lengths=None, streams=None,
**ignored)` -> audio [B, F * hop_length]), so `Tacotron2.infer` / `predict` / `stream` take it as `vocoder=` unchanged; the
arithmetic is csrc/stft_inv.hip through `TacotronSTFT.mel_to_audio`.  It lets one audition a synthesizer checkpoint, a
teacher-forced mel or a `load_mel` result with the synthesizer alone.
"""
from __future__ import annotations

from types import SimpleNamespace

from .stft import TacotronSTFT


class GriffinLim:
    def __init__(self, engine, stft_fn=None, n_iters=60, momentum=0.99, seed=None):
        """`stft_fn`: the `TacotronSTFT` the mels were made with (default: the synthesizer's 22 050 Hz, 1024 / 256 / 1024, 80
        mels).  `seed`: draw the initial phase from per-row streams (reproducible, independent of batching); None: zero phase."""
        self.stft_fn = (stft_fn if stft_fn is not None else TacotronSTFT()).bind(engine)
        self.n_iters = int(n_iters)
        self.momentum = float(momentum)
        self.seed = seed
        self.compiled_infer = SimpleNamespace(engine=engine)       # where `Tacotron2._clean_waveform` finds the engine

    @property
    def rate(self):
        return self.stft_fn.sampling_rate

    def __call__(self, mel, lengths=None, streams=None, **_ignored):
        """mel [F, n_mel] or [B, F, n_mel] -> audio [B, F * hop_length]; row b holds lengths[b] frames (default F)."""
        seeded = {} if self.seed is None else {'seed': self.seed, 'streams': streams}
        return self.stft_fn.mel_to_audio(mel, lengths=lengths, n_iters=self.n_iters, momentum=self.momentum, **seeded)

    infer = __call__
