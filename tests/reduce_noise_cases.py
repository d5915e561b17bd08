"""Shared case table of the stage-by-stage reduce_noise tests (tests/test_reduce_noise_stages.py on the CPU,
test_reduce_noise_stages_gpu.py on an MI355X).

`reduce_noise_run` (csrc/audio_proc.hip) is a chain of launches: zero pad of the rows and of the noise clips -> two forward
DFT GEMMs over hop-strided rows of the padded samples -> row maxima of |X|^2 -> noise threshold per bin -> gate mask ->
5 x 9 smoothing and gating in place -> inverse DFT GEMM -> overlap-add -> renormalise.  `HipEngine.reduce_noise_probe` stops it
after any of them.  `stages` restates tests/audio_ref.py in the engine's layout (B rows of Fr frame slots; the slots past a
row's own F_b frames are hop-strided reads into the next row's samples, as on the GPU) and keeps every intermediate; the
stage functions it is made of (`padded_rows`, `spectrum_of`, ... `normalized`) are the float64 yardstick.

`compare` judges each stage against the float64 result computed FROM THE PREVIOUS STAGE OF THE SAME RUN, so rounding in the
spectrum cannot leak into the gate decision and each bound speaks about one kernel.  In float64 the DFT is a complex128
rfft: the engine's fp32 basis is part of the kernel's rounding, not a constant of the operation.  dtype=float32 is
audio_ref's dft='f32' form carried on in float32 the way the kernels do; the CPU test puts it in the GPU's place.

Not planted: "imaginary part of bin 1024 kept in the inverse".  Its weight is sin(pi n) = 0 for every integer n, and the
forward DFT gives that imaginary part as 0 as well, so no data a test can produce separates the two; the reference of
`frames` ignores the imaginary parts of bins 0 and 1024 and the 30 pad columns, which pins that they contribute nothing.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

NFFT, HOP, NBIN = 2048, 512, 1025
RATE = 22050
CLIP = 4410                     # int(0.2 * 22050): the default noise clip
STAGES = ('padded', 'noise_padded', 'spectrum', 'noise_spectrum', 'power_max', 'threshold', 'mask', 'gated', 'frames')
WF = np.array([1, 2, 3, 2, 1], np.int64)                 # over bins
WT = np.array([1, 2, 3, 4, 5, 4, 3, 2, 1], np.int64)     # over frames

# ---- bounds ------------------------------------------------------------------------------------------------------------
# 'spectrum', 'noise_spectrum', 'frames', 'threshold' (DB_TOL) and 'e2e' are ten times the worst value measured on an
# MI355X over every case of CASES against float64 (test_reduce_noise_stages_gpu.py prints them); the others follow from
# the arithmetic and were fixed before anything ran.  The float32 numpy form measures 4.9e-7 / 4.6e-7 (spectra), 3.7e-6
# (frames), 1.9e-5 dB and 3.4e-6 (end to end) on the same cases.  With log10f in power_db the threshold measured 2.13e-5 dB,
# which would have put DB_TOL above 1e-4; the logarithm is taken in double since.  The weakest planted errors
# (test_reduce_noise_stages.py prints them) are 4.4e-4 at the spectra (basis in fp16), 3.2 dB at the threshold (sample std)
# and 0.52 at the frames (missing x2).
DB_TOL = 7.7e-5                 # dB; measured 7.62e-6 (dc_5000_1025_6000_quiet3000: dB values near -100)
BOUNDS = {
    'padded': 0.0,              # cells that are not bit-equal
    'noise_padded': 0.0,
    'spectrum': 2.4e-5,         # measured 2.34e-6 (burst_8000)
    'noise_spectrum': 2.3e-5,   # measured 2.28e-6 (dc_5000_1025_6000_quiet3000)
    'power_max': 2.0 ** -22,    # relative: two roundings, with or without fma contraction
    'threshold': DB_TOL,        # absolute dB; also the decision margin of the mask
    'mask': 0.0,                # decidable cells that differ + tie cells set + cells set in a dead frame
    'gated': 2.0 ** -22,        # relative per cell: the gain's division and the product
    'frames': 1.2e-4,           # measured 1.16e-5 (noise_1: one sample, a flat spectrum; 6.9e-6 on the longer rows)
    'out': 2.0 ** -23,          # relative per sample: fp64 sums, one rounding
    'out_norm': 1.0,            # in units of (|mean| / m + 4) * 2^-24, the kernel's four roundings
    'e2e': 6.1e-5,              # measured 6.04e-6 (noise_1_511_4410_20000), relative to the row's peak
}
UNDECIDABLE_CAP = 1e-3          # share of a case's valid cells within DB_TOL of their threshold, tie cells apart


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    lengths: tuple
    signal: str
    clip: Optional[str] = None          # None: the default clip (each row's first min(CLIP, L_b) samples); else its kind
    clip_len: int = CLIP
    tail: int = 0                       # extra samples past the longest row

    @property
    def B(self):
        return len(self.lengths)

    @property
    def N(self):
        return max(self.lengths) + self.tail


def _sine(L, rng, amp=0.02):
    t = np.arange(L) / RATE
    return 0.5 * np.sin(2 * np.pi * 220 * t) * (t > min(0.3, L / RATE / 2)) + amp * rng.standard_normal(L)


def _signal_row(kind, L, rng, row):
    n = np.arange(L, dtype=np.float64)
    if kind == 'noise':
        return 0.1 * rng.standard_normal(L)
    if kind == 'sine':
        return _sine(L, rng)
    if kind == 'speech':                    # tones under a slow envelope + noise at -50 dB
        x = sum(a * np.sin(2 * np.pi * f * n / RATE + rng.uniform(0, 2 * np.pi)) for a, f in ((0.4, 157.), (0.2, 491.), (0.05, 3044.)))
        env = 0.55 + 0.45 * np.sin(2 * np.pi * n / 3000.0 + rng.uniform(0, 2 * np.pi))
        return x * env * (n > min(5000, L // 2)) + 10 ** (-50 / 20) * rng.standard_normal(L)
    if kind == 'zeros':
        return np.zeros(L)
    if kind == 'zero_row1':                 # a silent row between two noisy ones
        return np.zeros(L) if row == 1 else 0.1 * rng.standard_normal(L)
    if kind in ('lead3000', 'lead6000'):    # digital silence, then signal: the clip is partly / wholly silence
        x = _sine(L, rng)
        x[:int(kind[4:])] = 0
        return x
    if kind == 'burst':                     # the row's maximum lies in the frames that signal and clip share; a smooth
        env = (0.5 - 0.5 * np.cos(2 * np.pi * n / 2000)) * (n < 2000)       # envelope keeps its leakage under the floor
        return 0.5 * np.sin(2 * np.pi * 2000 * n / RATE) * env + 1e-5 * rng.standard_normal(L)
    if kind == 'dc':
        return 0.25 * (1, -1, 0.5)[row % 3] + 1e-3 * rng.uniform(-1, 1, L)
    if kind == 'impulse':
        x = np.zeros(L)
        x[int(rng.integers(0, L))] = 1.0
        return x
    if kind == 'alt':                       # everything in bin 1024
        return (1.0 - 2.0 * (np.arange(L) % 2)) * (1, -1)[row % 2]
    raise ValueError(kind)


def _clip_row(kind, L, rng):
    if kind == 'noise':
        return 0.02 * rng.standard_normal(L)
    if kind == 'quiet':                     # far below the DC rows' own noise: the gate lets nearly everything through
        return 1e-6 * rng.uniform(-1, 1, L)
    if kind == 'tone':                      # a loud component over 1e-5 noise: most cells on the top_db floor
        return 0.5 * np.sin(2 * np.pi * 1000 * np.arange(L) / RATE) + 1e-5 * rng.standard_normal(L)
    raise ValueError(kind)


def inputs_of(case):
    """(audio [B, N] float32, lengths int32 [B], noise [B, clip_len] float32 or None, noise_len), seeded by the case.  What
    lies past a row's length is NaN (even rows) or garbage of magnitude 1e30 (odd rows): none of it may appear anywhere."""
    rng = np.random.default_rng(5000 + sum((i + 1) * L for i, L in enumerate(case.lengths)) + 7 * case.clip_len)
    audio = np.zeros((case.B, case.N), np.float32)
    for b, L in enumerate(case.lengths):
        audio[b, :L] = _signal_row(case.signal, L, rng, b)
        audio[b, L:] = np.nan if b % 2 == 0 else 1e30 * rng.standard_normal(case.N - L)
    noise = None
    if case.clip is not None:
        noise = np.stack([_clip_row(case.clip, case.clip_len, rng) for _ in range(case.B)]).astype(np.float32)
    return audio, np.asarray(case.lengths, np.int32), noise, case.clip_len


def _c(lengths, signal, clip=None, clip_len=CLIP, tail=0):
    lengths = (lengths,) if isinstance(lengths, int) else tuple(lengths)
    name = f'{signal}_' + '_'.join(str(L) for L in lengths) + (f'_{clip}{clip_len}' if clip else '') + (f'_t{tail}' if tail else '')
    return Case(name, lengths, signal, clip, clip_len, tail)


CASES = (
    # one row of noise at every length: F_b = 1 + (L + 512) // 512 steps at 512, 1024, 2048; the default clip is the whole
    # row up to 4410 and one sample short of it at 4411; 20480 a multiple of the hop
    *(_c(L, 'noise') for L in (1, 300, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4409, 4410, 4411, 20480)),
    _c(1500, 'noise', tail=500),
    # the same lengths in ragged batches, NaN / 1e30 past every L_b
    _c((1, 300, 511, 512, 513), 'noise'), _c((1023, 1024, 1025, 2047, 2048), 'sine'), _c((2049, 4409, 4410, 4411, 4608), 'speech'),
    _c((1, 511, 4410, 20000), 'noise'),
    # explicit clips: 1 and 511 samples one noise frame, 512 two, 3000 six, 4607 nine, 4608 ten
    _c(3000, 'noise', 'noise', 1), _c(3000, 'noise', 'noise', 511), _c(3000, 'noise', 'noise', 512),
    _c(4608, 'noise', 'noise', 4607), _c(4608, 'noise', 'noise', 4608), _c(4609, 'noise', 'noise', 4608),
    _c((4609, 1500, 20480), 'sine', 'noise', 3000),
    # signals
    _c(4710, 'sine'), _c(8000, 'speech'), _c(2048, 'zeros'), _c((300, 2048, 5000), 'zeros'), _c((3000, 2500, 700), 'zero_row1'),
    _c(10000, 'lead3000'), _c(12000, 'lead6000'), _c(8000, 'burst'), _c((300, 8000), 'burst'),
    _c(6000, 'noise', 'tone', 3000), _c(5000, 'dc', 'quiet', 3000), _c((5000, 1025, 6000), 'dc', 'quiet', 3000), _c(5000, 'dc'), _c(4096, 'impulse'), _c(3000, 'alt'),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)
BATCHED = tuple(c.name for c in CASES if c.B > 1)


# ---- geometry ----------------------------------------------------------------------------------------------------------
class Geom(NamedTuple):
    B: int
    N: int
    lens: np.ndarray        # L_b
    F: np.ndarray           # signal frames of row b
    nl: np.ndarray          # noise clip length of row b
    nF: np.ndarray          # noise frames of row b
    Fr: int                 # frame slots per row
    Frn: int
    default_clip: bool


def geometry(B, N, lengths, noise, noise_len, clip_pad=True):
    lens = np.full(B, N, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    nl = np.full(B, noise_len, np.int64) if noise is not None else np.minimum(noise_len, lens)
    F = 1 + (lens + (HOP if clip_pad else 0)) // HOP
    return Geom(B, N, lens, F, nl, 1 + nl // HOP, -(-(N + 2560) // HOP), -(-(noise_len + NFFT) // HOP), noise is None)


def hann(symmetric=False):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / (NFFT - 1 if symmetric else NFFT))


@functools.lru_cache(maxsize=None)
def _bases(symmetric=False):
    """(forward [2050, 2048], inverse [2048, 2050]) in float64, exact phase reduction, as audio_ref's dft='f32' form."""
    k, n = np.arange(NBIN), np.arange(NFFT)
    ang = 2 * np.pi * ((k[:, None] * n[None]) % NFFT) / NFFT
    w = hann(symmetric)
    fwd = np.concatenate([np.cos(ang) * w, -np.sin(ang) * w])
    ck = np.where((k == 0) | (k == NFFT // 2), 1.0, 2.0)[:, None]
    inv = np.concatenate([ck * np.cos(ang) * w / NFFT, -ck * np.sin(ang) * w / NFFT * ((k != 0) & (k != NFFT // 2))[:, None]]).T
    fwd.setflags(write=False)
    inv.setflags(write=False)
    return fwd, np.ascontiguousarray(inv)


# ---- the stage functions (float64 yardstick; float32 = the kernels' arithmetic) ----------------------------------------------
def padded_rows(rows, width, reflect=False):
    """[B, width] float32: 1024 zeros, the row's samples, zeros (librosa centre padding + the 512 clipping-pad samples)."""
    out = np.zeros((len(rows), width), np.float32)
    for b, r in enumerate(rows):
        r = np.asarray(r, np.float32)
        if reflect:
            r = np.pad(np.pad(r, [0, HOP]), NFFT // 2, mode='reflect')[:width]
            out[b, :len(r)] = r
        else:
            out[b, NFFT // 2:NFFT // 2 + len(r)] = r
    return out


def spectrum_of(padded, slots, dtype=np.float64, m=()):
    """[B, slots, 2050] (real parts, then imaginary parts) of the hop-strided frames of the rows laid end to end."""
    B, NP = padded.shape
    flat = np.concatenate([padded.ravel(), np.zeros(NFFT, padded.dtype)])
    idx = (np.arange(B)[:, None] * NP + np.arange(slots)[None] * HOP).ravel()[:, None] + np.arange(NFFT)[None]
    frames = flat[idx]
    sym = 'hann_symmetric' in m
    if dtype == np.float64 and 'basis_fp16' not in m:
        X = np.fft.rfft(frames.astype(np.float64) * hann(sym), axis=1)
        out = np.concatenate([X.real, X.imag], axis=1)
    else:
        basis = _bases(sym)[0]
        basis = basis.astype(np.float16).astype(dtype) if 'basis_fp16' in m else basis.astype(dtype)
        if dtype == np.float32:             # frame by frame: equal frames give equal bits whatever the number of rows
            out = np.stack([basis @ f for f in frames.astype(dtype)])
        else:
            out = frames.astype(dtype) @ basis.T
    return out.reshape(B, slots, 2 * NBIN)


def power(spec):
    return spec[..., :NBIN] ** 2 + spec[..., NBIN:] ** 2


def power_max_of(spec, counts, dtype=np.float64):
    """[B]: max |X|^2 over each row's own frames."""
    spec = np.asarray(spec, dtype)
    return np.array([power(spec[b, :counts[b]]).max() for b in range(spec.shape[0])], dtype)


def db_of(spec, pmax, dtype=np.float64, floor=True):
    """(dB clamped at the top_db floor, unclamped dB, floor): 10 log10 |X|^2 >= -400, floor = 10 log10(pmax) - 80."""
    with np.errstate(divide='ignore'):
        raw = np.maximum(dtype(10.0) * np.log10(power(np.asarray(spec, dtype))), dtype(-400.0))
        fl = np.maximum(dtype(10.0) * np.log10(dtype(pmax)), dtype(-400.0)) - dtype(80.0)
    return (np.maximum(raw, fl) if floor else raw), raw, fl


def threshold_of(nspec, nF, pmax_n, dtype=np.float64, m=(), pmax_s=None):
    """[B, 1025]: mean + 1.5 population std over the row's noise frames of the clamped dB (sums in float64)."""
    B = nspec.shape[0]
    out = np.zeros((B, NBIN), dtype)
    for b in range(B):
        pm = pmax_s[b] if 'floor_from_signal' in m else pmax_n[b]
        db = db_of(nspec[b, :nF[b]], pm, dtype, floor='no_floor' not in m)[0].astype(np.float64)
        out[b] = db.mean(axis=0) + (2.0 if 'std_2' in m else 1.5) * db.std(axis=0, ddof=1 if 'ddof_1' in m else 0)
    return out


def mask_of(spec, F, pmax_s, thr, dtype=np.float64, m=()):
    """[B, Fr, 1025] of 0 / 1: dB < threshold for f < F_b, else 0."""
    B, Fr = spec.shape[:2]
    out = np.zeros((B, Fr, NBIN), np.float32)
    for b in range(B):
        db = db_of(spec[b, :F[b]], pmax_s[b], dtype)[0]
        t = np.asarray(thr[b], dtype)
        t = t[:F[b], None] if 'thr_by_frame' in m else t[None, :]
        out[b, :F[b]] = (db <= t) if 'le' in m else (db < t)
    return out


def stencil(mask, m=()):
    """(acc, weight sum) of the 5 x 9 integer stencil over mask [F, 1025], zero outside (or as the mutation says)."""
    F, K = mask.shape
    wk, wt = (WT, WF) if 'stencil_transposed' in m else (WF, WT)
    hk, ht = len(wk) // 2, len(wt) // 2
    mi = mask.astype(np.int64)
    mp = np.pad(mi, [(ht, ht), (hk, hk)], mode='wrap') if 'stencil_wrap' in m else np.pad(mi, [(ht, ht), (hk, hk)])
    if 'stencil_wrap' in m:
        mp[:ht] = 0
        mp[-ht:] = 0                        # only the bins wrap
    ones = np.pad(np.ones_like(mi), [(ht, ht), (hk, hk)])
    acc, ws = np.zeros((F, K), np.int64), np.zeros((F, K), np.int64)
    for i in range(len(wt)):
        for j in range(len(wk)):
            acc += wt[i] * wk[j] * mp[i:i + F, j:j + K]
            ws += wt[i] * wk[j] * ones[i:i + F, j:j + K]
    return acc, ws


def gated_of(spec, mask, F, dtype=np.float64, m=()):
    """[B, Fr, 2050]: S * (225 - acc) / 225 for f < F_b, 0 in the dead slots."""
    spec = np.asarray(spec, dtype)
    out = np.zeros(spec.shape, dtype)
    for b in range(spec.shape[0]):
        acc, ws = stencil(np.asarray(mask[b, :F[b]]), m)
        g = (dtype(225) - acc.astype(dtype) * (dtype(225) / ws.astype(dtype))) / dtype(225) if 'stencil_renorm' in m else \
            (dtype(225) - acc.astype(dtype)) / dtype(225)
        out[b, :F[b]] = spec[b, :F[b]] * np.concatenate([g, g], axis=1)
    return out


def frames_of(gated, dtype=np.float64, m=()):
    """[B, Fr, 2048]: irfft x hann of every slot; the imaginary parts of bins 0 and 1024 do not count."""
    g = np.asarray(gated, dtype)
    if dtype == np.float64:
        X = g[..., :NBIN] + 1j * g[..., NBIN:]
        X[..., 0] = X[..., 0].real
        X[..., NBIN - 1] = X[..., NBIN - 1].real
        if 'no_x2' in m:
            X[..., 1:NBIN - 1] *= 0.5
        return np.fft.irfft(X, n=NFFT, axis=-1) * hann()
    return g @ _bases()[1].astype(dtype).T


def out_of(frames, lens, F, N, dtype=np.float64, m=()):
    """[B, N]: overlap-add over each row's own frames / Hann^2 sum, centre trim, fix_length; 0 past L_b."""
    w = hann()
    w2 = w if 'ola_hann_sum' in m else w * w
    out = np.zeros((frames.shape[0], N), dtype)
    for b in range(frames.shape[0]):
        Fb = int(F[b]) - (1 if 'ola_drop_last' in m else 0)
        n = NFFT + HOP * max(Fb - 1, 0)
        y, wss = np.zeros(n), np.zeros(n)
        for f in range(Fb):
            y[f * HOP:f * HOP + NFFT] += np.asarray(frames[b, f], np.float64)
            wss[f * HOP:f * HOP + NFFT] += w2
        nz = wss > np.finfo(np.float32).tiny
        y[nz] /= wss[nz]
        y = y[NFFT // 2:NFFT // 2 + int(lens[b])]
        out[b, :len(y)] = y
    return out


def normalized(out, lens, dtype=np.float64, m=()):
    """[B, N]: normalize_audio(max_val=1.) over each row's own samples; float32 does the kernel's four roundings."""
    res = np.zeros(out.shape, dtype)
    for b in range(out.shape[0]):
        x = np.asarray(out[b, :lens[b]], dtype)
        mean = dtype(0) if 'norm_no_mean' in m else dtype(np.mean(x.astype(np.float64)))
        d = x - mean
        mx = np.abs(d).max()
        res[b, :lens[b]] = d * (dtype(1) / mx) if mx > 1e-9 else d
    return res


# name -> the first stage it changes: planted errors of the size a wrong kernel would make
MUTATIONS = {
    'hann_symmetric': 'spectrum', 'basis_fp16': 'spectrum', 'no_clip_pad': 'mask', 'pad_reflect': 'padded',
    'ddof_1': 'threshold', 'std_2': 'threshold', 'floor_from_signal': 'threshold', 'no_floor': 'threshold',
    'le': 'mask', 'thr_by_frame': 'mask',
    'stencil_renorm': 'gated', 'stencil_wrap': 'gated', 'stencil_transposed': 'gated',
    'no_x2': 'frames', 'ola_drop_last': 'out', 'ola_hann_sum': 'out', 'norm_no_mean': 'out_norm',
}


def stages(audio, lengths=None, noise=None, noise_len=CLIP, dtype=np.float64, mutation=None):
    """Every stage of reduce_noise in the engine's layout (the keys of STAGES, 'out' and 'out_norm'), computed in `dtype`;
    `mutation` (a key of MUTATIONS) plants that error."""
    m = () if mutation is None else (mutation,)
    audio = np.asarray(audio, np.float32)
    B, N = audio.shape
    g = geometry(B, N, lengths, noise, noise_len, clip_pad='no_clip_pad' not in m)
    rows = [audio[b, :g.lens[b]] for b in range(B)]
    clips = [(noise[b] if noise is not None else audio[b])[:g.nl[b]] for b in range(B)]
    s = {'padded': padded_rows(rows, g.Fr * HOP, 'pad_reflect' in m), 'noise_padded': padded_rows(clips, g.Frn * HOP)}
    s['spectrum'] = spectrum_of(s['padded'], g.Fr, dtype, m)
    s['noise_spectrum'] = spectrum_of(s['noise_padded'], g.Frn, dtype, m)
    s['power_max'] = np.stack([power_max_of(s['spectrum'], g.F, dtype), power_max_of(s['noise_spectrum'], g.nF, dtype)])
    s['threshold'] = threshold_of(s['noise_spectrum'], g.nF, s['power_max'][1], dtype, m, s['power_max'][0])
    s['mask'] = mask_of(s['spectrum'], g.F, s['power_max'][0], s['threshold'], dtype, m)
    s['gated'] = gated_of(s['spectrum'], s['mask'], g.F, dtype, m)
    s['frames'] = frames_of(s['gated'], dtype, m)
    o = out_of(s['frames'], g.lens, g.F, N, np.float64, m)
    s['out'] = o.astype(dtype)
    s['out_norm'] = normalized(s['out'], g.lens, dtype, m)
    return s


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 stages of a case, computed once (read-only)."""
    audio, lens, noise, nl = inputs_of(BY_NAME[name])
    out = stages(audio, lens, noise, nl)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------
def _bits_differ(a, b):
    return int((np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)).sum())


def _frame_error(got, want, counts):
    """Worst frame over each row's own frames of max |got - want| / the frame's largest reference magnitude (1 if 0)."""
    worst = 0.0
    for b in range(got.shape[0]):
        g, w = np.asarray(got[b, :counts[b]], np.float64), np.asarray(want[b, :counts[b]], np.float64)
        if not np.isfinite(g).all():
            return float('inf')
        if w.shape[-1] == 2 * NBIN:
            scale = np.sqrt(power(w)).max(axis=-1)
        else:
            scale = np.abs(w).max(axis=-1)
        worst = max(worst, float((np.abs(g - w).max(axis=-1) / np.where(scale > 0, scale, 1.0)).max()))
    return worst


def _rel_error(got, want):
    """max |got - want| / |want|; where want is 0, got must be 0 (else inf)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.isfinite(got).all() or (got[want == 0] != 0).any():
        return float('inf')
    nz = want != 0
    return float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max()) if nz.any() else 0.0


def tie_cells(g, spec, nspec, pmax):
    """[B, Fr, 1025] bool: cells where dB == threshold exactly, by construction, so that `<` must give 0 --
    frame 0 of a row shorter than one hop under the default clip (its one noise frame IS signal frame 0: std 0); every cell
    of an all-zero row (-400 on both sides); cells where the signal and every noise frame of the bin sit on the same top_db
    floor (same row maximum), each by more than DB_TOL."""
    B, Fr = spec.shape[:2]
    tie = np.zeros((B, Fr, NBIN), bool)
    for b in range(B):
        Fb, nF = int(g.F[b]), int(g.nF[b])
        if g.default_clip and g.lens[b] < HOP:
            tie[b, 0] = True
        if pmax[0][b] == 0 and pmax[1][b] == 0:
            tie[b, :Fb] = True
        elif np.float32(pmax[0][b]) == np.float32(pmax[1][b]):
            _, raw_s, fl = db_of(spec[b, :Fb], np.float64(pmax[0][b]))
            _, raw_n, _ = db_of(nspec[b, :nF], np.float64(pmax[1][b]))
            tie[b, :Fb] |= (raw_s < fl - DB_TOL) & (raw_n < fl - DB_TOL).all(axis=0)[None]
    return tie


def compare(inputs, got, end_to_end=True):
    """The error of every stage in `got` (the keys of STAGES, 'out', 'out_norm'; the engine's layout) against the float64
    stage function applied to got's own previous stage, in the units of BOUNDS, plus 'undecidable' (share of the valid
    non-tie cells within DB_TOL of their threshold), 'ties', 'clamped_noise' (share of the valid noise cells on the top_db
    floor), 'mean_over_m' (largest |mean| / max |x - mean| of a row before renormalising), 'norm_gap' (largest distance of a
    renormalised sample from the float64 normalisation of the same row), 'e2e' and 'flips' (GPU mask against the pure float64 mask; information only)."""
    audio, lengths, noise, noise_len = inputs
    audio = np.asarray(audio, np.float32)
    B, N = audio.shape
    g = geometry(B, N, lengths, noise, noise_len)
    rows = [audio[b, :g.lens[b]] for b in range(B)]
    clips = [(noise[b] if noise is not None else audio[b])[:g.nl[b]] for b in range(B)]
    e = {}
    e['padded'] = _bits_differ(got['padded'], padded_rows(rows, g.Fr * HOP))
    e['noise_padded'] = _bits_differ(got['noise_padded'], padded_rows(clips, g.Frn * HOP))
    e['spectrum'] = _frame_error(got['spectrum'], spectrum_of(np.asarray(got['padded'], np.float32), g.Fr), g.F)
    e['noise_spectrum'] = _frame_error(got['noise_spectrum'], spectrum_of(np.asarray(got['noise_padded'], np.float32), g.Frn), g.nF)
    spec, nspec = np.asarray(got['spectrum'], np.float32), np.asarray(got['noise_spectrum'], np.float32)
    pmax = np.asarray(got['power_max'], np.float32)
    e['power_max'] = _rel_error(pmax, np.stack([power_max_of(spec, g.F), power_max_of(nspec, g.nF)]))
    thr = np.asarray(got['threshold'], np.float32)
    e['threshold'] = float(np.abs(thr.astype(np.float64) - threshold_of(nspec, g.nF, pmax[1].astype(np.float64))).max()) \
        if np.isfinite(thr).all() else float('inf')
    # mask
    mask = np.asarray(got['mask'], np.float32)
    tie = tie_cells(g, spec, nspec, pmax)
    bad = int(((mask != 0) & (mask != 1)).sum())
    undecidable = valid = 0
    clamped = ncells = 0
    for b in range(B):
        Fb, nF = int(g.F[b]), int(g.nF[b])
        db = db_of(spec[b, :Fb], np.float64(pmax[0][b]))[0]
        t = thr[b].astype(np.float64)[None]
        und = (np.abs(db - t) <= DB_TOL) & ~tie[b, :Fb]
        want = db < t
        bad += int(((mask[b, :Fb] != want) & ~und & ~tie[b, :Fb]).sum())      # a decidable cell differs
        bad += int((mask[b, :Fb][tie[b, :Fb]] != 0).sum())                      # a tie cell is set
        bad += int((mask[b, Fb:] != 0).sum())                                   # a dead frame is set
        undecidable += int(und.sum())
        valid += int((~tie[b, :Fb]).sum())
        _, raw_n, fl_n = db_of(nspec[b, :nF], np.float64(pmax[1][b]))
        clamped += int((raw_n < fl_n).sum())
        ncells += raw_n.size
    e['mask'], e['ties'] = bad, int(tie.sum())
    e['undecidable'] = undecidable / max(valid, 1)
    e['clamped_noise'] = clamped / ncells
    # gated, frames
    want = gated_of(spec, mask, g.F)
    e['gated'] = _rel_error(got['gated'], want)
    gated = np.asarray(got['gated'], np.float32)
    e['frames'] = _frame_error(got['frames'], frames_of(gated), g.F)
    # output
    out = np.asarray(got['out'], np.float32)
    e['out'] = _rel_error(out, out_of(np.asarray(got['frames'], np.float32), g.lens, g.F, N))
    worst = ratio = gap = 0.0
    nrm, want = np.asarray(got['out_norm'], np.float64), normalized(out, g.lens)
    for b in range(B):
        L = int(g.lens[b])
        x = out[b, :L].astype(np.float64)
        mx = np.abs(x - x.mean()).max()
        d = np.abs(nrm[b, :L] - want[b, :L]).max()
        if not np.isfinite(nrm[b]).all() or nrm[b, L:].any():
            worst = float('inf')
        elif mx <= 1e-9:
            worst = max(worst, 0.0 if d == 0 else float('inf'))               # silence stays exact
        else:
            worst = max(worst, float(d / ((abs(x.mean()) / mx + 4) * 2.0 ** -24)))
            ratio = max(ratio, float(abs(x.mean()) / mx))
            gap = max(gap, float(d))
    e['out_norm'] = worst
    e['mean_over_m'], e['norm_gap'] = ratio, gap
    if end_to_end:                          # the pure float64 chain from the audio, the run's own mask in place of its mask
        p = padded_rows(rows, g.Fr * HOP)
        S = spectrum_of(p, g.Fr)
        pure = out_of(frames_of(gated_of(S, mask, g.F)), g.lens, g.F, N)
        peak = np.array([max(np.abs(pure[b]).max(), 0.0) for b in range(B)])
        diff = np.array([np.abs(out[b, :g.lens[b]].astype(np.float64) - pure[b, :g.lens[b]]).max() for b in range(B)])
        e['e2e'] = float((diff / np.where(peak > 0, peak, 1.0)).max()) if np.isfinite(out).all() else float('inf')
        Sn = spectrum_of(padded_rows(clips, g.Frn * HOP), g.Frn)
        pm = np.stack([power_max_of(S, g.F), power_max_of(Sn, g.nF)])
        pure_mask = mask_of(S, g.F, pm[0], threshold_of(Sn, g.nF, pm[1]))
        e['flips'] = int(sum((pure_mask[b, :g.F[b]] != mask[b, :g.F[b]]).sum() for b in range(B)))
    return e


CHECKED = ('padded', 'noise_padded', 'spectrum', 'noise_spectrum', 'power_max', 'threshold', 'mask', 'gated', 'frames', 'out',
           'out_norm', 'e2e')


def failures(e):
    """The stages of a `compare` result that miss their bound, and the undecidable cap."""
    bad = [(k, e[k], BOUNDS[k]) for k in CHECKED if k in e and not e[k] <= BOUNDS[k]]
    if not e['undecidable'] <= UNDECIDABLE_CAP:
        bad.append(('undecidable', e['undecidable'], UNDECIDABLE_CAP))
    return bad
