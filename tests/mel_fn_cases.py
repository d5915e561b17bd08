"""Shared case table of the mel-plan tests (tests/test_mel_fn.py and test_mel_fn_call.py on the CPU, test_mel_fn_gpu.py on an
MI355X): the configurations, the lengths, the signals, and `stages`, a float64 restatement of steps 1 - 8 of the contract in
include/tts_hip.h (zero pad, pre-emphasis, reflect pad, windowed DFT, magnitude, filterbank, logarithm, normalisation or
Whisper clamp) that keeps every intermediate under the names `HipEngine.mel_fn_probe` uses.  It reads oracle/mel_stft_ref.py
(the filterbank, the basis recipe) and tests/mel_stft_cases.py (signals, `stage_error`, BOUNDS) and changes neither.

The DFT basis and the filterbank are float32 tables cast up, as in mel_stft_cases: they are the operation's constants, not
part of its rounding.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

import mel_stft_cases as C
from oracle import mel_stft_ref as R

STAGES = ('padded', 'spectrum', 'magnitude', 'mel_linear', 'mel_log')
TILE_M = 64


class Config(NamedTuple):
    name: str
    kind: str = 'tacotron'
    sampling_rate: int = 22050
    filter_length: int = 1024
    hop_length: int = 256
    win_length: int = 1024
    n_mel_channels: int = 80
    mel_fmin: float = 0.0
    mel_fmax: float = 8000.0
    pre_emph: float = 0.0
    normalize_mode: Optional[str] = None
    periodic: bool = True

    @property
    def half(self):
        return self.filter_length // 2

    @property
    def cut(self):
        return self.filter_length // 2 + 1

    def dft_frames(self, n):
        return (max(n, self.win_length) + 2 * self.half - self.filter_length) // self.hop_length + 1

    def frames(self, n):
        return self.dft_frames(n) - (1 if self.kind == 'whisper' else 0)

    def plan_config(self):
        """What HipEngine.mel_fn takes."""
        d = self._asdict()
        d.pop('name'), d.pop('periodic')
        return d

    def window(self, symmetric=None):
        """float64 [win_length]: scipy.signal.get_window('hann', win_length, fftbins=periodic)."""
        sym = (not self.periodic) if symmetric is None else symmetric
        n = self.win_length
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1 if sym else n))


# the smallest configurations that turn each code path over
CONFIGS = {c.name: c for c in (
    Config('default'),                                                                   # the fixed path
    Config('whisper', 'whisper', 16000, 400, 160, 400),                                  # K = 400, not a multiple of 32
    Config('centred', 'tacotron', 16000, 512, 160, 400, 40, pre_emph=0.97, normalize_mode='per_feature'),
    Config('gather', 'tacotron', 22050, 1102, 275, 1102, normalize_mode='all_feature'),  # hop not a multiple of 4
    Config('odd', 'tacotron', 8000, 255, 64, 255, 23, mel_fmax=4000.0, periodic=False),  # odd filter: F = (L' - 1) // hop + 1
    Config('wide', 'tacotron', 24000, 2048, 300, 1200, 128, 50.0, 12000.0),              # a long K
)}

# ---- bounds ------------------------------------------------------------------------------------------------------------
# K <= 1024 (default, whisper, centred, odd): the project's mel_stft_cases.BOUNDS.  K > 1024 (gather, wide): 10 x the worst
# stage_error test_mel_fn_gpu.py printed on an MI355X against float64 (the margin of BOUNDS: machines of the pool differ in
# association, not in precision), the measured value beside each.
BOUNDS = {name: dict(C.BOUNDS) for name in ('default', 'whisper', 'centred', 'odd')}
BOUNDS['gather'] = {
    'padded': 0.0,
    'spectrum': 1.8e-5,         # measured 1.772e-6 (gather_noise_n17325)
    'magnitude': 1.8e-5,        # measured 1.790e-6 (gather_noise_n17325)
    'mel_linear': 1.6e-5,       # measured 1.525e-6 (gather_noise_n17600)
}
BOUNDS['wide'] = {
    'padded': 0.0,
    'spectrum': 2.0e-5,         # measured 1.911e-6 (wide_ragged)
    'magnitude': 2.0e-5,        # measured 1.902e-6 (wide_ragged)
    'mel_linear': 2.2e-5,       # measured 2.192e-6 (wide_noise_n18899)
}
# The K <= 1024 configurations measured on the same run, under BOUNDS' 1.7e-5 / 1.7e-5 / 1.2e-5: default 1.70e-6 / 1.69e-6 /
# 1.67e-6, whisper 9.4e-7 / 9.2e-7 / 6.7e-7, centred 1.10e-6 / 1.04e-6 / 2.5e-7, odd 9.1e-7 / 9.4e-7 / 2.9e-7; the reference's
# WhisperSTFT fixture through load_mel: 2.3e-5 (tolerance 2e-3).
LOG_ULPS = C.LOG_ULPS
NORM_ULPS = 1                   # the normalised modes: double arithmetic rounded once, against float64 numpy rounded once


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    config: str
    signal: str                 # one of mel_stft_cases' signals, or 'mixed': row b takes MIXED[b % 3]
    N: int
    lengths: Optional[tuple] = None

    @property
    def B(self):
        return 1 if self.lengths is None else len(self.lengths)


MIXED = ('noise', 'zeros', 'tone')


def lengths_of(cfg):
    """1, win_length - 1, win_length, win_length + 1, N % 4 of 1 and 3, and hop * 63 - 1, hop * 63, hop * 64: F goes 63, 64,
    65 across the 64-row GEMM tile (an odd filter: 63, 63, 64)."""
    wl, hop = cfg.win_length, cfg.hop_length
    n1 = wl + 2 + (1 - (wl + 2)) % 4
    n3 = wl + 2 + (3 - (wl + 2)) % 4
    assert n1 % 4 == 1 and n3 % 4 == 3
    return tuple(dict.fromkeys((1, wl - 1, wl, wl + 1, n1, n3, hop * 63 - 1, hop * 63, hop * 64)))


def _cases():
    out = []
    for cfg in CONFIGS.values():
        for n in lengths_of(cfg):
            out.append(Case(f'{cfg.name}_noise_n{n}', cfg.name, 'noise', n))
        n = cfg.hop_length * 63
        for signal in ('tone', 'quiet', 'zeros', 'alt'):            # tonal, quiet, silent, full scale
            out.append(Case(f'{cfg.name}_{signal}_n{n}', cfg.name, signal, n))
        # ragged: B = 3, lengths (N, win_length - 1, about N / 2), NaN behind every row's length
        out.append(Case(f'{cfg.name}_ragged', cfg.name, 'mixed', n + 5, (n, cfg.win_length - 1, n // 2 + 1)))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)
RAGGED = tuple(c.name for c in CASES if c.lengths is not None)


def audio_of(case, tail=np.nan):
    """[B, N] float32 seeded by the case; a ragged case holds `tail` behind every row's length."""
    rng = np.random.default_rng(4000 + 7 * case.N + len(case.config))
    lens = case.lengths or (case.N,)
    rows = []
    for b, L in enumerate(lens):
        kind = MIXED[b % 3] if case.signal == 'mixed' else case.signal
        row = np.full(case.N, tail, np.float64)
        row[:L] = C._signal_row(kind, L, rng, b)
        rows.append(row)
    return np.stack(rows).astype(np.float32)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables(config, window=None, lpad_shift=0):
    """(basis [2 * cut, filter_length], filterbank [n_mel, cut]) float32 of a configuration, built as oracle/mel_stft_ref.py
    builds them.  window = 'swapped' (periodic <-> symmetric) and lpad_shift = 1 are controls only."""
    cfg = CONFIGS[config]
    fl, wl, cut = cfg.filter_length, cfg.win_length, cfg.cut
    fb = np.fft.fft(np.eye(fl))
    fb = np.vstack([np.real(fb[:cut]), np.imag(fb[:cut])]).astype(np.float32)
    win = cfg.window(symmetric=cfg.periodic if window == 'swapped' else None)
    lpad = (fl - wl) // 2 + lpad_shift
    if wl < fl:                                         # librosa.util.pad_center
        win = np.pad(win, (lpad, fl - wl - lpad))
    basis = (fb * win[None, :]).astype(np.float32)
    mb = R.mel_filterbank(cfg.sampling_rate, fl, cfg.n_mel_channels, cfg.mel_fmin, cfg.mel_fmax)
    basis.setflags(write=False)
    mb.setflags(write=False)
    return basis, mb


def padded_row(cfg, x, dtype=np.float64, pre_first=False):
    """Steps 1 - 3 of one row x [L]: zero pad to max(L, win_length), pre-emphasis (one product, one difference in `dtype`),
    reflect pad.  pre_first (a control only): the pre-emphasis before the zero pad."""
    x = np.asarray(x, dtype)

    def emph(v):
        if not cfg.pre_emph > 0:
            return v
        return np.concatenate([v[:1], v[1:] - (dtype(cfg.pre_emph) * v[:-1]).astype(dtype)]).astype(dtype)

    if pre_first:
        x = emph(x)
    if len(x) < cfg.win_length:
        x = np.pad(x, (0, cfg.win_length - len(x)))
    if not pre_first:
        x = emph(x)
    return np.pad(x, (cfg.half, cfg.half), mode='reflect')


def normalize(cfg, x, ddof=0):
    """MelSTFT.normalize on one row x [F, n_mel] in float64: population std, 0 where it is 0."""
    if cfg.normalize_mode is None:
        return x
    kw = dict(axis=0, keepdims=True) if cfg.normalize_mode == 'per_feature' else {}
    mean, std = np.mean(x, **kw), np.std(x, ddof=ddof, **kw)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(std == 0, 0.0, (x - mean) / std)


def whisper_tail(x, rowmax=None):
    """The clamp and the affine map of one row's log10 mel in float32, as the kernel does them."""
    x = np.asarray(x, np.float32)
    m = np.maximum(x, (x.max() if rowmax is None else np.float32(rowmax)) - np.float32(8.0))
    return (m + np.float32(4.0)) / np.float32(4.0)


def final_of(cfg, mel_log_row, ddof=0, rowmax=None):
    """Step 6 / 7 behind the logarithm on one row's own frames [F, n_mel] -> float32."""
    if cfg.kind == 'whisper':
        return whisper_tail(mel_log_row, rowmax)
    return normalize(cfg, np.asarray(mel_log_row, np.float64), ddof).astype(np.float32)


def padded_rows(config, audio, lengths=None, dtype=np.float64, pre_first=False):
    """'padded' [B, max(N, win_length) + 2 * (filter_length // 2)] of audio [B, N]: every row's steps 1 - 3, zeros behind."""
    cfg = CONFIGS[config]
    audio = np.asarray(audio, np.float32)
    B, N = audio.shape
    x = np.zeros((B, max(N, cfg.win_length) + 2 * cfg.half), dtype)
    for b in range(B):
        row = padded_row(cfg, audio[b, :N if lengths is None else lengths[b]], dtype, pre_first)
        x[b, :len(row)] = row
    return x


MUTATIONS = {
    # name -> (the stage it belongs to, keywords of `stages`)
    'window_swapped': ('spectrum', dict(window='swapped')),
    'lpad_off_by_one': ('spectrum', dict(lpad_shift=1)),
    'pre_emph_before_pad': ('padded', dict(pre_first=True)),
    'whisper_last_frame_kept': ('mel', dict(keep_last=True)),
    'sample_std': ('mel', dict(ddof=1)),
    'rowmax_over_batch': ('mel', dict(batch_max=True)),
}


def stages(config, audio, lengths=None, dtype=np.float64, window=None, lpad_shift=0, pre_first=False, keep_last=False, ddof=0,
           batch_max=False):
    """{'padded' [B, P], 'spectrum' [B, Fr, 2 cut], 'magnitude' [B, Fr, cut], 'mel_linear' [B, Fr, n_mel], 'mel_log' and 'mel'
    [B, Fout, n_mel], 'frames' (the result's frames per row)} of audio [B, N], computed in `dtype` per row on its first
    lengths[b] samples; the keywords plant the errors of MUTATIONS.  Frames beyond a row's own: the spectrum, the magnitude
    and the linear mel hold what the zero-padded row gives, 'mel_log' and 'mel' hold 0."""
    cfg = CONFIGS[config]
    audio = np.asarray(audio, np.float32)
    B, N = audio.shape
    lens = [N] * B if lengths is None else list(lengths)
    basis, mb = tables(config, window, lpad_shift)
    basis, mb = basis.astype(dtype), mb.astype(dtype)
    fl, hop, cut = cfg.filter_length, cfg.hop_length, cfg.cut
    P = max(N, cfg.win_length) + 2 * cfg.half
    Fr = cfg.dft_frames(N)
    drop = 1 if cfg.kind == 'whisper' and not keep_last else 0
    x = padded_rows(config, audio, lens, dtype, pre_first)
    assert x.shape == (B, P)
    idx = np.arange(Fr)[:, None] * hop + np.arange(fl)[None, :]
    ft = np.pad(x, [(0, 0), (0, fl)])[:, idx] @ basis.T
    mag = np.sqrt(ft[..., :cut] ** 2 + ft[..., cut:] ** 2)
    lin = mag @ mb.T
    clip, log = (1e-10, np.log10) if cfg.kind == 'whisper' else (1e-5, np.log)
    frames = [cfg.dft_frames(n) - drop for n in lens]
    mel_log = np.zeros((B, Fr - drop, cfg.n_mel_channels), dtype)
    for b in range(B):
        mel_log[b, :frames[b]] = log(np.maximum(lin[b, :frames[b]], dtype(clip)))
    top = max(float(np.float32(mel_log[b, :frames[b]]).max()) for b in range(B)) if batch_max else None
    mel = np.zeros(mel_log.shape, np.float32)
    for b in range(B):
        mel[b, :frames[b]] = final_of(cfg, mel_log[b, :frames[b]].astype(np.float32), ddof, top)
    return {'padded': x, 'spectrum': ft, 'magnitude': mag, 'mel_linear': lin, 'mel_log': mel_log, 'mel': mel, 'frames': frames}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 stages of a case, computed once (read-only)."""
    case = BY_NAME[name]
    out = stages(case.config, audio_of(case, tail=0.0), case.lengths)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------
def own_frames(st, b, n_frames):
    """Row b of a stage dictionary cut to its own DFT frames, in the shape mel_stft_cases.stage_error takes."""
    return {s: np.asarray(st[s])[b:b + 1, :n_frames] for s in ('spectrum', 'magnitude', 'mel_linear')}


def stage_error(stage, got, ref, dft_frames):
    """mel_stft_cases.stage_error over every row's own DFT frames (the worst row counts); 'padded': max abs difference."""
    if stage == 'padded':
        return C.stage_error('padded', got, ref)
    return max(C.stage_error(stage, np.asarray(got)[b:b + 1, :f], own_frames(ref, b, f)) for b, f in enumerate(dft_frames))


def log_ulp_error(cfg, mel_log, linear):
    """Worst |mel_log - log(max(linear, clip))| in float32 ulps of the float64 value (log10 and 1e-10 for Whisper), `linear`
    being the float32 linear mel the logarithm was taken of."""
    clip, log = (1e-10, np.log10) if cfg.kind == 'whisper' else (1e-5, np.log)
    want = log(np.maximum(np.asarray(linear, np.float32).astype(np.float64), float(np.float32(clip))))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return float((np.abs(np.asarray(mel_log, np.float64) - want) / ulp).max())


def final_error(cfg, got, want):
    """Error of the final stage: shapes must agree (else inf); Whisper and no normalisation count differing cells' largest
    absolute difference (the bound is 0: exact), the normalised modes float32 ulps of the reference value."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float('inf')
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if cfg.kind == 'whisper' or cfg.normalize_mode is None:
        return float(d.max())
    return float((d / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).max())


def final_bound(cfg):
    return 0.0 if cfg.kind == 'whisper' or cfg.normalize_mode is None else float(NORM_ULPS)
