"""Speaking rate and pitch on a waveform: `time_stretch` and `pitch_shift`, on the GPU.

Tacotron2 has no rate input, so both happen on the audio.  `time_stretch` is a phase vocoder with identity phase locking
(Laroche and Dolson 1999; csrc/stft_inv.hip: tts_hip_time_stretch) -- the plain vocoder of `librosa.phase_vocoder` loses most
of a tone's amplitude when it slows down -- and `pitch_shift` is that stretch followed by FFT resampling back to the input's
duration (csrc/resample.hip), as `librosa.effects.pitch_shift` composes it.  Both work on anything `load_audio` returns: a row
[N] or a batch [B, N] with `lengths`; numpy in gives numpy out, a CUDA tensor stays on the device.  There is no CPU path.
"""
import numpy as np

PITCH_RATIO_UNITS = 1_000_000       # pitch_shift resamples by the integer pair (this, round(r * this))


def default_plan(engine):
    """The plan both effects use unless told otherwise: filter_length 1024, hop 256, a periodic Hann window of 1024."""
    from .stft import STFT
    return STFT(filter_length=1024, hop_length=256, win_length=1024, engine=engine)._plan()


def time_stretch(audio, rate, *, engine, plan=None, lengths=None):
    """`audio` [N] or [B, N] played `rate` times as fast (a scalar or one value per row, in [0.25, 4]) at the same pitch ->
    (out, out_lengths): row b holds out_lengths[b] = round(lengths[b] / rate[b]) samples, zeros beyond (`HipEngine.time_stretch`)."""
    return engine.time_stretch(plan or default_plan(engine), audio, rate, lengths=lengths)


def pitch_ratio(n_steps, bins_per_octave=12):
    """(r, p, q): the stretch rate r = 2 ** (-n_steps / bins_per_octave) and the integer rates the resampler takes for it."""
    if not np.isfinite(n_steps) or int(bins_per_octave) != bins_per_octave or bins_per_octave < 1:
        raise ValueError(f'pitch_shift: n_steps must be finite and bins_per_octave a positive integer, got {n_steps!r}, {bins_per_octave!r}')
    r = 2.0 ** (-float(n_steps) / int(bins_per_octave))
    return r, PITCH_RATIO_UNITS, int(round(r * PITCH_RATIO_UNITS))


def fix_length(audio, size):
    """Rows cut or zero-padded on the right to `size` samples (librosa.util.fix_length), on the array's own device."""
    n = audio.shape[-1]
    if n == size:
        return audio
    if n > size:
        return audio[..., :size]
    if isinstance(audio, np.ndarray):
        return np.pad(audio, [(0, 0)] * (audio.ndim - 1) + [(0, size - n)])
    import torch
    return torch.nn.functional.pad(audio, (0, size - n))


def pitch_shift(audio, n_steps, *, engine, plan=None, lengths=None, bins_per_octave=12):
    """`audio` [N] or [B, N] raised by `n_steps` steps of an octave split in `bins_per_octave` (negative: lowered), its
    duration kept -> the input's shape: a stretch by r = 2 ** (-n_steps / bins_per_octave), one `engine.resample` by
    (1_000_000, round(r * 1_000_000)), and every row cut or zero-padded to its input length (behind lengths[b] a row is 0).
    One `n_steps` per call; n_steps = 0 returns the input as it is.  A CUDA tensor stays on the device between the two calls."""
    r, p, q = pitch_ratio(n_steps, bins_per_octave)
    size = int(audio.shape[-1])
    if n_steps == 0:
        return audio
    stretched, out_lengths = time_stretch(audio, r, engine=engine, plan=plan, lengths=lengths)
    out = fix_length(engine.resample(stretched, p, q, lengths=out_lengths), size)
    if lengths is not None:                                      # a row's own samples only (`out` is this call's own array)
        keep = np.asarray(lengths.detach().cpu() if hasattr(lengths, 'detach') else lengths).reshape(-1)
        rows = out if out.ndim == 2 else out[None]
        for b, n in enumerate(keep):
            rows[b, int(n):] = 0
    return out


__all__ = ['time_stretch', 'pitch_shift', 'default_plan', 'pitch_ratio', 'fix_length']
