"""Shared case table of the mel-STFT tests (tests/test_mel_stft.py on the CPU, test_mel_stft_gpu.py on an MI355X).

`melstft_run` (csrc/mel_stft.hip) is a chain of five launches: reflect pad -> windowed-DFT GEMM over overlapping rows of the
padded signal -> magnitude -> filterbank GEMM -> log(max(., 1e-5)).  `HipEngine.mel_stft_probe` stops it after any of the
first four, so every stage is compared on its own against `stages`, a restatement of oracle/mel_stft_ref.py that keeps
every intermediate.  In float64 it is the yardstick (the DFT basis and the filterbank are the reference's float32 tables
cast up: they are the operation's constants, not part of its rounding); in float32 it is the oracle itself.

Errors are `stage_error`: per frame, max abs error over the frame's cells divided by the frame's largest reference
magnitude (times the largest filterbank weight for the linear mel), the worst frame counting.  A scale per frame keeps a
quiet frame next to a loud one honest; a scale from the magnitudes rather than from the mel row keeps a frame whose energy
lies above fmax (the +-1 alternation: all of it in bin 512) from being held to a bound relative to a sum of leakage.
"""
import functools
from typing import NamedTuple

import numpy as np

FL, HOP, CUT, NMEL = 1024, 256, 513, 80
CLIP = 1e-5
TILE_M = 64                 # gemm_small: 64-row tiles (conv_cases.TILE_M)
STAGES = ('padded', 'spectrum', 'magnitude', 'mel_linear')

# ---- bounds ------------------------------------------------------------------------------------------------------------
# About 10x the worst stage_error measured on an MI355X over every case of CASES (test_mel_stft_gpu.py prints them), against
# the float64 reference, fp32 MFMA throughout.  The float32 numpy restatement measures 1.59e-6 / 1.51e-6 / 1.33e-6 on the
# same cases (noise_b5_n3333, speech_b3_n4098), so the GPU is at the float32 floor.  The weakest planted errors of MUTATIONS
# are 4.43e-4 at the spectrum (DFT basis rounded to fp16, impulse_b3_n16384) and 5.61e-4 at the linear mel (filterbank
# rounded to fp16, impulse_b1_n1027): test_mel_stft.py keeps every bound a factor of 3 below what it has to catch.
BOUNDS = {
    'padded': 0.0,              # bit-equal to numpy's reflect pad on every case
    'spectrum': 1.7e-5,         # measured 1.72e-6 (noise_b1_n16127)
    'magnitude': 1.7e-5,        # measured 1.69e-6 (noise_b1_n16127)
    'mel_linear': 1.2e-5,       # measured 1.23e-6 (noise_b5_n3333)
}
LOG_ULPS = 2                    # the logarithm against the float64 log of the same float32 input, in ulps of that value


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    B: int
    N: int
    signal: str
    seed: int = 0

    @property
    def F(self):
        return self.N // HOP + 1


def _signal_row(kind, N, rng, row):
    n = np.arange(N, dtype=np.float64)
    if kind == 'noise':
        return rng.uniform(-1, 1, N)
    if kind in ('tone', 'tone_half'):       # bin 100 exactly / half-way to bin 101; every row its own phase and level
        k = 100.0 if kind == 'tone' else 100.5
        return 0.5 / (1 + row) * np.sin(2 * np.pi * k * n / FL + rng.uniform(0, 2 * np.pi))
    if kind == 'speech':                    # three tones under a slow envelope + noise at -50 dB
        x = sum(a * np.sin(2 * np.pi * k * n / FL + rng.uniform(0, 2 * np.pi))
                for a, k in ((0.4, 7.3), (0.2, 22.8), (0.05, 141.4)))
        env = 0.55 + 0.45 * np.sin(2 * np.pi * n / 3000.0 + rng.uniform(0, 2 * np.pi))
        return x * env + 10 ** (-50 / 20) * rng.standard_normal(N)
    if kind == 'quiet':                     # mel cells just above the clip
        return 3e-5 * rng.standard_normal(N)
    if kind == 'zeros':
        return np.zeros(N)
    if kind == 'dc':
        return np.full(N, 0.25 * (1, -1, 0.5)[row % 3])
    if kind == 'impulse':
        x = np.zeros(N)
        x[int(rng.integers(0, N))] = 1.0
        return x
    if kind == 'alt':                       # +-1 full scale: everything in bin 512, above fmax
        return (1.0 - 2.0 * (np.arange(N) % 2)) * (1, -1)[row % 2]
    raise ValueError(kind)


def audio_of(case):
    """[B, N] float32, seeded by the case."""
    rng = np.random.default_rng(9000 + 7 * case.N + 131 * case.B + case.seed)
    return np.stack([_signal_row(case.signal, case.N, rng, b) for b in range(case.B)]).astype(np.float32)


def _c(B, N, signal, seed=0):
    return Case(f'{signal}_b{B}_n{N}', B, N, signal, seed)


CASES = (
    # every length with noise.  1024 the minimum; 1025 / 1027 N % 4 of 1 / 3; 1279 / 1280 N % 256 of 255 / 0;
    # 16127 / 16128 / 16384: F = 63 / 64 / 65, around one 64-row tile of the DFT GEMM
    _c(1, 1024, 'noise'), _c(1, 1025, 'noise'), _c(1, 1027, 'noise'), _c(1, 1279, 'noise'), _c(1, 1280, 'noise'),
    _c(1, 16127, 'noise'), _c(1, 16128, 'noise'), _c(1, 16384, 'noise'),
    # batches: the row stride NP = N + 1024 rounded up to 4, so N % 4 of 1, 2, 3 leave 3, 2, 1 floats between the rows
    _c(3, 1025, 'noise'), _c(3, 1026, 'noise'), _c(3, 1027, 'noise'),
    # B * F = 70 rows in the filterbank GEMM: row 4's frames sit in two tiles
    _c(5, 3333, 'noise'),
    # every other signal at one or two lengths
    _c(1, 16127, 'tone'), _c(3, 1027, 'tone'),
    _c(1, 16128, 'tone_half'), _c(1, 1025, 'tone_half'),
    _c(1, 16384, 'speech'), _c(3, 4098, 'speech'),
    _c(1, 16127, 'quiet'), _c(1, 1280, 'quiet'),
    _c(1, 1024, 'zeros'), _c(3, 1025, 'zeros'),
    _c(1, 1279, 'dc'), _c(1, 16128, 'dc'),
    _c(1, 1027, 'impulse'), _c(3, 16384, 'impulse'),
    _c(1, 1280, 'alt'), _c(1, 16127, 'alt'),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)
BATCHED = tuple(c.name for c in CASES if c.B > 1)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables(window='periodic'):
    """(basis [1026, 1024], filterbank [80, 513]) float32, as oracle/mel_stft_ref.py builds them (read-only).
    window='symmetric' (a control only) restates forward_basis with scipy's fftbins=False Hann."""
    from oracle import mel_stft_ref as R
    if window == 'periodic':
        basis = R.forward_basis(FL, FL)
    else:
        fb = np.fft.fft(np.eye(FL))
        fb = np.vstack([np.real(fb[:CUT]), np.imag(fb[:CUT])]).astype(np.float32)
        basis = (fb * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FL) / (FL - 1)))[None, :]).astype(np.float32)
    mb = R.mel_filterbank(22050, FL, NMEL, 0.0, 8000.0)
    basis.setflags(write=False)
    mb.setflags(write=False)
    return basis, mb


def fb_max():
    return float(_tables()[1].max())


def _round_fp16(x):
    return x.astype(np.float16).astype(x.dtype)


def _trunc_mantissa(x, bits):
    """float64 values cut (toward zero) to `bits` explicit mantissa bits."""
    u = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return (u & ~np.uint64((1 << (52 - bits)) - 1)).view(np.float64)


def _fb_shift(mb):
    return np.roll(mb, 1, axis=1)


def _fb_drop_last(mb):
    out = mb.copy()
    for j in range(out.shape[0]):
        out[j, np.flatnonzero(out[j])[-1]] = 0
    return out


# name -> (first stage it changes, what it replaces): planted errors of the size a wrong kernel would make
MUTATIONS = {
    'basis_fp16': ('spectrum', {'basis': _round_fp16}),
    'frames_10bit': ('spectrum', {'frames': lambda f: _trunc_mantissa(f, 10)}),
    'filterbank_fp16': ('mel_linear', {'mb': _round_fp16}),
    'hann_symmetric': ('spectrum', {'window': 'symmetric'}),
    'pad_edge': ('padded', {'pad': 'edge'}),
    'filterbank_shift': ('mel_linear', {'mb': _fb_shift}),
    'filterbank_drop_last': ('mel_linear', {'mb': _fb_drop_last}),
    'hop_255': ('spectrum', {'hop': 255}),
}


def stages(audio, dtype=np.float64, mutation=None):
    """{'padded', 'spectrum', 'magnitude', 'mel_linear', 'mel'} of audio [B, N] (N >= 1024), computed in `dtype` as
    oracle.mel_stft_ref.mel_spectrogram computes them; `mutation` (a key of MUTATIONS) plants that error.  A mutated hop
    yields more frames: the first N // 256 + 1 are kept."""
    m = {} if mutation is None else MUTATIONS[mutation][1]
    audio = np.asarray(audio, dtype=np.float32)
    assert audio.ndim == 2 and audio.shape[1] >= FL
    B, N = audio.shape
    F = N // HOP + 1
    basis, mb = _tables(m.get('window', 'periodic'))
    basis = m.get('basis', lambda v: v)(basis.astype(dtype))
    mb = m.get('mb', lambda v: v)(mb.astype(dtype))
    x = np.pad(audio.astype(dtype), [(0, 0), (FL // 2, FL // 2)], mode=m.get('pad', 'reflect'))
    idx = np.arange(F)[:, None] * m.get('hop', HOP) + np.arange(FL)[None, :]
    frames = m.get('frames', lambda v: v)(x[:, idx])
    ft = frames @ basis.T
    mag = np.sqrt(ft[..., :CUT] ** 2 + ft[..., CUT:] ** 2)
    lin = mag @ mb.T
    return {'padded': x, 'spectrum': ft, 'magnitude': mag, 'mel_linear': lin, 'mel': np.log(np.maximum(lin, dtype(CLIP)))}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 stages of a case, computed once (read-only)."""
    out = stages(audio_of(BY_NAME[name]))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------
def frame_scale(stage, ref):
    """[B, F] divisor of a stage's errors: the frame's largest reference magnitude (x the largest filterbank weight for the
    linear mel); 1 for a frame of exact zeros."""
    s = np.asarray(ref['magnitude'], np.float64).max(axis=-1)
    if stage == 'mel_linear':
        s = s * fb_max()
    return np.where(s > 0, s, 1.0)


def stage_error(stage, got, ref):
    """Worst frame of max |got - ref[stage]| / frame_scale; 'padded' has no scale (max abs difference: it must be 0)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(ref[stage], np.float64)
    assert got.shape == want.shape, (stage, got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    if stage == 'padded':
        return float(np.abs(got - want).max())
    return float((np.abs(got - want).max(axis=-1) / frame_scale(stage, ref)).max())


def log_ulp_error(mel, linear):
    """Worst |mel - log(max(linear, 1e-5))| in float32 ulps of the float64 value, `linear` being the float32 linear mel
    the logarithm was taken of."""
    want = np.log(np.maximum(np.asarray(linear, np.float32).astype(np.float64), float(np.float32(CLIP))))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return float((np.abs(np.asarray(mel, np.float64) - want) / ulp).max())


def clip_failures(mel, ref):
    """The clip conditions of a case as a list of failures (empty = all hold): no NaN or inf anywhere, and every cell whose
    float64 reference lies below half the clip holds log(1e-5) within LOG_ULPS.  Cells with a reference in [0.5e-5, 2e-5)
    may land on either side of the clip and are judged by `stage_error` of the linear mel alone, which leaves no cell out."""
    mel = np.asarray(mel)
    if not np.isfinite(mel).all():
        return ['non-finite mel']
    bad = []
    below = np.asarray(ref['mel_linear']) < 0.5 * CLIP
    floor = np.log(float(np.float32(CLIP)))
    if below.any():
        d = np.abs(mel[below].astype(np.float64) - floor).max() / float(np.spacing(np.float32(abs(floor))))
        if d > LOG_ULPS:
            bad.append(f'a cell below 0.5e-5 is {d:.2f} ulps from log(1e-5)')
    return bad
