"""float64 numpy restatement of the WaveGlow denoiser (csrc/stft_inv.hip: tts_hip_denoise), written from its definition in
include/tts_hip.h on top of tests/stft_inv_ref.py (`transform`, `phasor`, `inverse`).  `dtype=np.float32` runs the same code
in float32: the distance of that run from the float64 one is what the GPU bound of the gate is derived from
(tests/test_denoise.py).  `plant` names a deliberate mistake (MISTAKES) of the size a wrong kernel would make.
"""
import numpy as np

import stft_inv_ref as R

# strength ignored (taken as 1), bias shifted by one bin, clamp missing, phase dropped, gate applied to the real and imaginary
# parts separately, gate missing, the cut to lengths[b] missing
MISTAKES = ('no_strength', 'bias_shift', 'no_clamp', 'no_phase', 'gate_parts', 'no_gate', 'no_cut')
GATE_MISTAKES = MISTAKES[:-1]


def magnitude(spec, g):
    re, im = spec[..., :g.cut], spec[..., g.cut:]
    return np.sqrt(re * re + im * im)


def gate(spec, bias, s, g, frames=None, dtype=np.float64, plant=None):
    """spectrum [B, F, 2 cut] -> the inverse's operand [B, F, 2 cut]: per bin max(|X| - s bias[c], 0) X / |X|, 0 at the origin
    and in the frames at and beyond a row's own."""
    spec = np.asarray(spec, dtype)
    re, im = spec[..., :g.cut], spec[..., g.cut:]
    b = np.asarray(bias, dtype)
    if plant == 'bias_shift':
        b = np.roll(b, 1)
    sb = dtype(1.0 if plant == 'no_strength' else s) * b
    if plant == 'gate_parts':
        yr = np.sign(re) * np.maximum(np.abs(re) - sb, 0)
        yi = np.sign(im) * np.maximum(np.abs(im) - sb, 0)
    else:
        m = magnitude(spec, g)
        pr, pi = R.phasor(re, im)
        gm = m if plant == 'no_gate' else m - sb
        if plant != 'no_clamp':
            gm = np.maximum(gm, 0)
        if plant == 'no_phase':
            pr, pi = np.ones_like(pr), np.zeros_like(pi)
        yr, yi = gm * pr, gm * pi
    return R.mask_frames(np.concatenate([yr, yi], axis=-1).astype(dtype), frames)


def clamped_share(spec, bias, s, g):
    """Share of the bins whose gated magnitude is clamped to 0."""
    return float((magnitude(np.asarray(spec, np.float64), g) - s * np.asarray(bias, np.float64) <= 0).mean())


def kept_samples(n, g):
    """Samples a row of n keeps: no more than the g.frames(n) frames of its zero-padded samples overlap-add to."""
    return min(n, g.samples(g.frames(n)))


def padded_row(x, n, g, dtype=np.float64):
    """[1, max(n, win_length)]: the row's own n samples, zero-padded as the plan pads a short row."""
    row = np.zeros((1, max(n, g.wl)), dtype)
    row[0, :n] = x[:n]
    return row


def cut_rows(audio, lengths, g, N, dtype=np.float64, plant=None):
    """The inverse's rows [B, F hop] -> [B, N]: row b keeps min(lengths[b], samples(frames_b)), zeros beyond."""
    out = np.zeros((audio.shape[0], N), dtype)
    for b, n in enumerate(lengths):
        keep = min(g.samples(g.frames(n)), N) if plant == 'no_cut' else kept_samples(n, g)
        out[b, :keep] = audio[b, :keep]
    return out


def denoise(x, bias, s, g, lengths=None, dtype=np.float64, plant=None):
    """audio [B, N] -> [B, N], every row on its own: transform, gate, inverse, cut to the row."""
    x = np.asarray(x)
    B, N = x.shape
    lengths = [N] * B if lengths is None else [int(v) for v in lengths]
    out = np.zeros((B, N), dtype)
    for b, n in enumerate(lengths):
        spec = R.transform(padded_row(x[b], n, g, dtype), g, dtype)
        audio = R.inverse(gate(spec, bias, s, g, None, dtype, plant), g, None, dtype)
        out[b:b + 1] = cut_rows(audio, [n], g, N, dtype, plant)
    return out


def operand_error(got, want, spec, g):
    """Worst frame of max |got - want| over the frame's cells / the INPUT frame's largest pair magnitude (1 for a frame of
    zeros): a gate that closes leaves nothing of its own to hold an error against."""
    got, want, spec = (np.asarray(a, np.float64) for a in (got, want, spec))
    assert got.shape == want.shape == spec.shape, (got.shape, want.shape, spec.shape)
    if not np.isfinite(got).all():
        return float('inf')
    mag = magnitude(spec, g).max(axis=-1)
    return float((np.abs(got - want).max(axis=-1) / np.where(mag > 0, mag, 1.0)).max())
