"""Speaking rate, pitch and formants on a waveform: `time_stretch`, `pitch_shift` and `formant_shift`, on the GPU.

Tacotron2 has no rate input, so both happen on the audio.  `time_stretch` is a phase vocoder with identity phase locking
(Laroche and Dolson 1999; csrc/stft_inv.hip: tts_hip_time_stretch) -- the plain vocoder of `librosa.phase_vocoder` loses most
of a tone's amplitude when it slows down -- and `pitch_shift` is that stretch followed by FFT resampling back to the input's
duration (csrc/resample.hip), as `librosa.effects.pitch_shift` composes it.  Both work on anything `load_audio` returns: a row
[N] or a batch [B, N] with `lengths`; numpy in gives numpy out, a CUDA tensor stays on the device.  There is no CPU path.

A shift by resampling moves the vocal-tract resonances with the harmonics: beyond about two semitones the voice sounds like a
smaller or a larger speaker.  `pitch_shift(..., preserve_formants=True)` puts the input's cepstrally smoothed spectral envelope
back onto the shifted signal (csrc/stft_inv.hip: tts_hip_formant_match), and `formant_shift` / `formant_steps` move that
envelope along frequency on its own: an apparent-speaker-size control.
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


def _zero_tails(out, lengths):
    """Rows of `out` (this call's own array) zeroed behind lengths[b]."""
    if lengths is not None:
        keep = np.asarray(lengths.detach().cpu() if hasattr(lengths, 'detach') else lengths).reshape(-1)
        rows = out if out.ndim == 2 else out[None]
        for b, n in enumerate(keep):
            rows[b, int(n):] = 0
    return out


def formant_warp(n_steps, bins_per_octave=12):
    """The envelope warp 2 ** (n_steps / bins_per_octave) of `n_steps` formant steps."""
    if not np.isfinite(n_steps) or int(bins_per_octave) != bins_per_octave or bins_per_octave < 1:
        raise ValueError(f'formant steps must be finite and bins_per_octave a positive integer, got {n_steps!r}, {bins_per_octave!r}')
    return 2.0 ** (float(n_steps) / int(bins_per_octave))


def _match(audio, source, warp, engine, plan, lengths, lifter, max_gain_db):
    """`engine.formant_match` in the shape `audio` came in."""
    out = engine.formant_match(plan or default_plan(engine), audio, source, warp=warp, lifter=lifter, max_gain_db=max_gain_db,
                               lengths=lengths)
    return out[0] if audio.ndim == 1 else out


def formant_shift(audio, n_steps, *, engine, plan=None, lengths=None, bins_per_octave=12, lifter=None, max_gain_db=24.0):
    """`audio` [N] or [B, N] with its formants moved by `n_steps` steps of an octave split in `bins_per_octave` (positive: up,
    a smaller speaker) and its pitch and duration kept -> the input's shape: `engine.formant_match` of the audio against
    itself with warp = 2 ** (n_steps / bins_per_octave), which must lie in [0.5, 2].  n_steps = 0 returns the input as it is."""
    warp = formant_warp(n_steps, bins_per_octave)
    if n_steps == 0:
        return audio
    return _match(audio, None, warp, engine, plan, lengths, lifter, max_gain_db)


def pitch_shift(audio, n_steps, *, engine, plan=None, lengths=None, bins_per_octave=12, preserve_formants=False, formant_steps=0.0,
                lifter=None, max_gain_db=24.0):
    """`audio` [N] or [B, N] raised by `n_steps` steps of an octave split in `bins_per_octave` (negative: lowered), its
    duration kept -> the input's shape: a stretch by r = 2 ** (-n_steps / bins_per_octave), one `engine.resample` by
    (1_000_000, round(r * 1_000_000)), and every row cut or zero-padded to its input length (behind lengths[b] a row is 0).
    One `n_steps` per call; n_steps = 0 returns the input as it is (with formant_steps != 0: `formant_shift` of it).  A CUDA
    tensor stays on the device between the calls.  `preserve_formants`: the shifted rows then get the input's spectral
    envelope back (`engine.formant_match` against the input; `lifter`, `max_gain_db`), so the voice keeps its size; a non-zero
    `formant_steps` implies that and moves the envelope by that many steps (warp = 2 ** (formant_steps / bins_per_octave)).
    With the defaults neither is called and the result is the plain shift, bit for bit."""
    r, p, q = pitch_ratio(n_steps, bins_per_octave)
    warp = formant_warp(formant_steps, bins_per_octave)
    size = int(audio.shape[-1])
    if n_steps == 0:
        return audio if formant_steps == 0 else _match(audio, None, warp, engine, plan, lengths, lifter, max_gain_db)
    stretched, out_lengths = time_stretch(audio, r, engine=engine, plan=plan, lengths=lengths)
    out = _zero_tails(fix_length(engine.resample(stretched, p, q, lengths=out_lengths), size), lengths)
    if preserve_formants or formant_steps != 0:
        out = _match(out, audio, warp, engine, plan, lengths, lifter, max_gain_db)
    return out


__all__ = ['time_stretch', 'pitch_shift', 'formant_shift', 'default_plan', 'pitch_ratio', 'formant_warp', 'fix_length']
