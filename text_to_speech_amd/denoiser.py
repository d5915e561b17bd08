"""`Denoiser`: the clean-up the published WaveGlow ships with, on the engine.

A WaveGlow checkpoint has a constant model bias: fed a silent mel and no noise it still emits a faint tonal hum.  The denoiser
takes the magnitude spectrum of that hum once per model (`bias`) and subtracts `strength x` it from every frame of a
synthesized waveform, magnitudes clamped at 0 and the phase kept -- spectral subtraction that knows the model, where
`reduce_noise` is a generic gate.  The arithmetic is csrc/stft_inv.hip (`HipEngine.denoise`): the mel plan's transform, one gate
kernel, the plan's inverse.  There is no CPU path.
"""
from __future__ import annotations

import numpy as np

from .engine import _is_torch_cuda
from .stft import STFT

BIAS_FRAMES = 88                    # frames of the silent mel the bias is taken from (the published denoiser's)


class Denoiser:
    def __init__(self, engine, *, precision='f32', filter_length=1024, n_overlap=4, win_length=1024, bias=None):
        """`engine`: the HipEngine that holds the vocoder.  `precision`: the one the vocoder is run in -- the hum of an fp16
        run is not bit for bit the fp32 one.  The STFT has hop_length = filter_length // n_overlap and a Hann window.  `bias`
        (float32 [filter_length // 2 + 1], >= 0) replaces the model's own, e.g. with one taken from a noise mel."""
        self.engine = engine
        self.precision = precision
        self.stft = STFT(filter_length=filter_length, hop_length=filter_length // n_overlap, win_length=win_length, engine=engine)
        self._bias_host = self._bias_dev = None
        if bias is not None:
            bias = bias.detach().cpu().numpy() if hasattr(bias, 'detach') else bias
            bias = np.ascontiguousarray(bias, dtype=np.float32)
            if bias.shape != (filter_length // 2 + 1,):
                raise ValueError(f'bias must be [{filter_length // 2 + 1}], got {bias.shape}')
            self._bias_host = bias

    def _plan(self):
        return self.stft._plan()

    def _model_bias(self):
        """The vocoder's answer to silence: `waveglow_infer` of a zero mel [1, 88, 80] with explicit zero noise and sigma = 0
        in this object's precision, transformed under this object's plan; the magnitude of frame 0."""
        mel = np.zeros((1, BIAS_FRAMES, 80), np.float32)
        z = np.zeros((1, BIAS_FRAMES * 32, 8), np.float32)
        hum = self.engine.waveglow_infer(mel, z=z, sigma=0.0, precision=self.precision)
        magnitude, _ = self.engine.stft_transform(self._plan(), hum)
        return np.ascontiguousarray(magnitude[0, 0], dtype=np.float32)

    @property
    def bias(self):
        """float32 [filter_length // 2 + 1] on the engine's device; computed on first use, then kept."""
        if self._bias_dev is None:
            import torch
            if self._bias_host is None:
                self._bias_host = self._model_bias()
            self._bias_dev = torch.as_tensor(self._bias_host).to(torch.device('cuda', self.engine.device))
        return self._bias_dev

    def __call__(self, audio, strength=0.1, lengths=None, stream=None):
        """audio [N] or [B, N] -> [B, N]; row b holds lengths[b] samples (default N).  numpy in -> numpy out, a CUDA tensor in
        -> a CUDA tensor out (`stream`: enqueued there), as `HipEngine.denoise`."""
        bias = self.bias
        if not _is_torch_cuda(audio):
            bias = self._bias_host
        return self.engine.denoise(self._plan(), audio, bias, strength=strength, lengths=lengths, stream=stream)
