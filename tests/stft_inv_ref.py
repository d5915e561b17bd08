"""float64 numpy restatement of the STFT with phase, its inverse, the mel inversion and the Griffin-Lim loop
(csrc/stft_inv.hip), written from the definitions in include/tts_hip.h and the reference's utils/audio/stft.py:194-274, with
the inverse basis taken through scipy.linalg.pinv exactly as the reference builds it.  `dtype=np.float32` runs the same code
in float32: the distance of that run from the float64 one is what the GPU bounds are derived from (tests/test_stft_inv.py).

The windowed bases are the operation's constants: float32 tables (rounded as the reference rounds them) cast up to `dtype`.
`plant` names a deliberate mistake (MISTAKES) of the size a wrong kernel would make; the CPU tests check that every bound
used on the GPU lies well below what each mistake does.
"""
import functools
from typing import NamedTuple

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)


class Geom(NamedTuple):
    fl: int
    wl: int
    hop: int
    window: str = 'hann'          # None: rectangular

    @property
    def cut(self):
        return self.fl // 2 + 1

    @property
    def half(self):
        return self.fl // 2

    @property
    def scale(self):
        return self.fl / self.hop

    def samples(self, frames):
        return self.hop * (frames - 1) + self.fl - 2 * self.half

    def frames(self, n):
        return (max(n, self.wl) + 2 * self.half - self.fl) // self.hop + 1


GEOMS = (Geom(16, 16, 4), Geom(15, 12, 5), Geom(64, 48, 10), Geom(1024, 1024, 256))

MISTAKES = ('no_window', 'ws_from_w', 'no_scale', 'trim_off_by_one', 'ck_edge', 'imag_sign', 'p00_zero', 'momentum_from_c',
            'neighbour_frames', 'reflect_off_by_one')


def centred_window(g):
    """float64 [fl]: the window centred in filter_length (librosa.util.pad_center)."""
    if g.window is None:
        w = np.ones(g.wl)
    elif g.window == 'hann':
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(g.wl) / g.wl)
    else:
        from scipy.signal import get_window
        w = get_window(g.window, g.wl, fftbins=True)
    out = np.zeros(g.fl)
    lpad = (g.fl - g.wl) // 2
    out[lpad:lpad + g.wl] = w
    return out


def fourier_basis(fl):
    """[2 cut, fl] float64: real rows of bins 0 .. cut - 1, then the imaginary rows (stft.py:212-217)."""
    fb = np.fft.fft(np.eye(fl))
    cut = fl // 2 + 1
    return np.vstack([np.real(fb[:cut]), np.imag(fb[:cut])])


def inverse_basis_pinv(fl, hop):
    """[2 cut, fl] float64: transpose(pinv(scale * fourier_basis)) (stft.py:220-222)."""
    from scipy.linalg import pinv
    return np.transpose(pinv((fl / hop) * fourier_basis(fl)))


def inverse_basis_closed(fl, hop, ck_edge=False):
    """The same in closed form: c_k cos(2 pi k n / N) / (N scale) and -c_k sin(2 pi k n / N) / (N scale), c_0 = 1,
    c_{N/2} = 1 for even N, else 2.  ck_edge plants the mistake at the last bin (2 at an even length's Nyquist bin, 1 at an
    odd length's last bin)."""
    cut, scale = fl // 2 + 1, fl / hop
    k = np.arange(cut)[:, None]
    n = np.arange(fl)[None, :]
    c = np.full((cut, 1), 2.0)
    c[0] = 1.0
    if fl % 2 == 0:
        c[-1] = 1.0
    if ck_edge:
        c[-1] = 2.0 if fl % 2 == 0 else 1.0
    ang = 2.0 * np.pi * ((k * n) % fl) / fl
    return np.vstack([c * np.cos(ang), -c * np.sin(ang)]) / (fl * scale)


@functools.lru_cache(maxsize=None)
def tables(g, plant=None):
    """(forward [2 cut, fl], inverse [2 cut, fl], window^2 [fl]) float32 tables, rounded as the reference rounds them: the
    basis to float32, then times the window, to float32."""
    w = centred_window(g)
    fwd = (fourier_basis(g.fl).astype(np.float32).astype(np.float64) * w).astype(np.float32)
    inv = inverse_basis_closed(g.fl, g.hop, True) if plant == 'ck_edge' else inverse_basis_pinv(g.fl, g.hop)
    inv = inv.astype(np.float32).astype(np.float64)
    if plant == 'imag_sign':
        inv[g.cut:] *= -1
    if plant != 'no_window':
        inv = inv * w
    inv = inv.astype(np.float32)
    w2 = ((w if plant == 'ws_from_w' else w * w)).astype(np.float32)
    for t in (fwd, inv, w2):
        t.setflags(write=False)
    return fwd, inv, w2


def reflect_rows(x, g, plant=None):
    half = g.half
    if plant == 'reflect_off_by_one':            # the edge sample repeated: every border sample one off
        return np.pad(x, [(0, 0), (half, half)], mode='symmetric')
    return np.pad(x, [(0, 0), (half, half)], mode='reflect')


def transform(x, g, dtype=np.float64, plant=None):
    """x [B, N] (N >= win_length) -> spectrum [B, F, 2 cut] (real parts, then imaginary parts)."""
    x = np.asarray(x, dtype)
    fwd = tables(g)[0].astype(dtype)
    p = reflect_rows(x, g, plant)
    F = (p.shape[1] - g.fl) // g.hop + 1
    idx = np.arange(F)[:, None] * g.hop + np.arange(g.fl)[None, :]
    return p[:, idx] @ fwd.T


def polar(spec, g):
    re, im = spec[..., :g.cut], spec[..., g.cut:]
    return np.sqrt(re * re + im * im), np.arctan2(im, re)


def time_frames(spec, g, dtype=np.float64, plant=None):
    """spectrum [B, F, 2 cut] -> frames [B, F, fl]."""
    return np.asarray(spec, dtype) @ tables(g, plant if plant in ('ck_edge', 'imag_sign', 'no_window') else None)[1].astype(dtype)


def overlap_add(tf, g, frames=None, dtype=np.float64, plant=None, padded=False):
    """frames [B, F, fl] -> audio [B, F * hop] (row b: samples(frames[b]) samples, zeros beyond), or with padded=True the
    reflect-padded rows [B, hop (F - 1) + fl] the forward transform reads."""
    tf = np.asarray(tf, dtype)
    B, F, fl = tf.shape
    fr = [F] * B if frames is None else [int(v) for v in frames]
    w2 = tables(g, 'ws_from_w' if plant == 'ws_from_w' else None)[2].astype(dtype)
    out = np.zeros((B, (g.hop * (F - 1) + fl) if padded else F * g.hop), dtype)
    for b in range(B):
        Fb = fr[(b + 1) % B] if plant == 'neighbour_frames' else fr[b]
        n = g.hop * (Fb - 1) + fl
        y = np.zeros(n, dtype)
        ws = np.zeros(n, dtype)
        for f in range(Fb):                                          # frame order: what the gather kernel sums in
            y[f * g.hop:f * g.hop + fl] += tf[b, f]
            ws[f * g.hop:f * g.hop + fl] += w2
        ok = ws > dtype(FLT_MIN)
        y[ok] /= ws[ok]
        if plant != 'no_scale':
            y = y * dtype(g.scale)
        lo = g.half + (1 if plant == 'trim_off_by_one' else 0)
        S = g.samples(Fb)
        x = y[lo:lo + S]
        if len(x) < S:
            x = np.concatenate([x, np.zeros(S - len(x), dtype)])
        if padded:
            out[b, :S + 2 * g.half] = reflect_rows(x[None], g, plant)[0]
        else:
            out[b, :S] = x
    return out


def inverse(spec, g, frames=None, dtype=np.float64, plant=None):
    return overlap_add(time_frames(spec, g, dtype, plant), g, frames, dtype, plant)


def phasor(re, im, plant=None):
    """P(re, im) = (re, im) / |(re, im)|, P(0, 0) = (1, 0)."""
    m = np.maximum(np.abs(re), np.abs(im))
    zero = m == 0
    ms = np.where(zero, 1, m)
    a, b = re / ms, im / ms
    n = np.sqrt(a * a + b * b)
    n = np.where(zero, 1, n)
    one = re.dtype.type(0 if plant == 'p00_zero' else 1)
    return np.where(zero, one, a / n), np.where(zero, 0, b / n)


def slaney_filterbank(sr, fl, n_mel, fmin, fmax):
    """float64 [n_mel, cut]: librosa.filters.mel with its defaults (Slaney scale and normalisation)."""
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    to_mel = lambda f: min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp
    to_hz = lambda m: min_log_hz * np.exp(logstep * (m - min_log_mel)) if m >= min_log_mel else f_sp * m
    m0, m1 = to_mel(fmin), to_mel(fmax)
    mel_f = np.array([to_hz(m0 + (m1 - m0) * i / (n_mel + 1)) for i in range(n_mel + 2)])
    cut = fl // 2 + 1
    fr = (sr / 2.0) * np.arange(cut) / (cut - 1)
    W = np.zeros((n_mel, cut))
    for i in range(n_mel):
        lower = (fr - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fr) / (mel_f[i + 2] - mel_f[i + 1])
        W[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[i + 2] - mel_f[i]))
    return W


def mel_inverse(W):
    """Minv [n_mel, cut] with spectrum = mel . Minv: the transpose of the minimum-norm inverse W^T (W W^T)^-1 = pinv(W)."""
    return np.linalg.pinv(W).T


def mel_target(mel, Minv, dtype=np.float64, plant=None):
    """S = max(0, exp(mel) . Minv).  plant 'no_clamp': the maximum missing; 'filterbank': `Minv` is the filterbank itself."""
    S = np.exp(np.asarray(mel, dtype)) @ np.asarray(Minv, dtype)
    return S if plant == 'no_clamp' else np.maximum(0, S)


def target_error(got, want):
    """Worst frame of max |got - want| / the frame's largest target (1 for a frame of zeros)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    scale = want.max(axis=-1)
    return float((np.abs(got - want).max(axis=-1) / np.where(scale > 0, scale, 1.0)).max())


def stack(S, pr, pi):
    return np.concatenate([S * pr, S * pi], axis=-1)


def mask_frames(a, frames):
    if frames is not None:
        a = a.copy()
        for b, Fb in enumerate(frames):
            a[b, int(Fb):] = 0
    return a


def loop_step(S, operand, tprev, g, momentum, frames=None, dtype=np.float64, plant=None):
    """One iteration from its operand S p: -> {'frames', 'signal' (padded rows), 'spectrum', 'phasor', 'operand' (the next
    one), 'tprev'}."""
    tf = time_frames(operand, g, dtype, plant)
    sig = overlap_add(tf, g, frames, dtype, plant, padded=True)
    fwd = tables(g)[0].astype(dtype)
    F = S.shape[1]
    idx = np.arange(F)[:, None] * g.hop + np.arange(g.fl)[None, :]
    Y = sig[:, idx] @ fwd.T
    alpha = dtype(momentum / (1.0 + momentum))
    c = Y - alpha * tprev
    pr, pi = phasor(c[..., :g.cut], c[..., g.cut:], plant)
    nxt = mask_frames(stack(S, pr, pi), frames)
    return {'frames': tf, 'signal': sig, 'spectrum': Y, 'phasor': np.concatenate([pr, pi], -1), 'operand': nxt,
            'tprev': c if plant == 'momentum_from_c' else Y}


def first_operand(S, g, init=None, frames=None, dtype=np.float64, plant=None):
    S = mask_frames(np.asarray(S, dtype), frames)
    if init is None:
        pr, pi = np.ones_like(S), np.zeros_like(S)
    else:
        init = np.asarray(init, dtype)
        pr, pi = phasor(init[..., 0], init[..., 1], plant)
    return S, mask_frames(stack(S, pr, pi), frames)


def griffin_lim(S, g, n_iters, momentum=0.0, init=None, frames=None, dtype=np.float64, plant=None):
    """S [B, F, cut] -> audio [B, F * hop]."""
    S, op = first_operand(S, g, init, frames, dtype, plant)
    tprev = np.zeros_like(op)
    for _ in range(n_iters):
        st = loop_step(S, op, tprev, g, momentum, frames, dtype, plant)
        op, tprev = st['operand'], st['tprev']
    return inverse(op, g, frames, dtype, plant)


def inconsistency(x, S, g):
    """|| |STFT(x)| - S || / || S || of audio x [B, n] against target magnitudes S [B, F, cut] (float64)."""
    mag = polar(transform(np.asarray(x, np.float64), g), g)[0]
    S = np.asarray(S, np.float64)
    return float(np.linalg.norm(mag - S) / np.linalg.norm(S))


# ---- signals -----------------------------------------------------------------------------------------------------------
def signal(kind, n, g, seed=0):
    """float32 [n]: 'tone' (a tone under a slow amplitude modulation plus noise at -40 dB), 'impulse', 'silence', 'full'
    (+-1 full scale)."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n, dtype=np.float64)
    if kind == 'tone':
        k = max(1.3, g.fl / 9.7)
        x = 0.5 * np.sin(2 * np.pi * k * t / g.fl + 0.4) * (0.6 + 0.4 * np.sin(2 * np.pi * t / (7.3 * g.fl)))
        x = x + 0.01 * rng.standard_normal(n)
    elif kind == 'impulse':
        x = np.zeros(n)
        x[n // 3] = 1.0
    elif kind == 'silence':
        x = np.zeros(n)
    elif kind == 'full':
        x = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


# ---- comparison --------------------------------------------------------------------------------------------------------
def frame_error(got, want, g):
    """Worst frame of max |got - want| over the frame's cells / the frame's largest |want| pair magnitude (1 for a frame of
    zeros): [B, F, 2 cut] spectra and operands."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    mag = np.sqrt(want[..., :g.cut] ** 2 + want[..., g.cut:] ** 2).max(axis=-1)
    return float((np.abs(got - want).max(axis=-1) / np.where(mag > 0, mag, 1.0)).max())


def frames_error(got, want, operand, g):
    """Time frames [B, F, fl] of an operand [B, F, 2 cut]: worst frame of max |got - want| / (the operand's largest pair
    magnitude in the frame x the inverse basis' largest absolute column sum) -- a frame is a sum that may cancel, so its
    error is held against what went in (1 for a frame of zeros)."""
    got, want, operand = (np.asarray(a, np.float64) for a in (got, want, operand))
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    gain = float(np.abs(tables(g)[1].astype(np.float64)).sum(axis=0).max())
    mag = np.sqrt(operand[..., :g.cut] ** 2 + operand[..., g.cut:] ** 2).max(axis=-1) * gain
    return float((np.abs(got - want).max(axis=-1) / np.where(mag > 0, mag, 1.0)).max())


def row_error(got, want):
    """Worst row of max |got - want| / the row's largest |want| (1 for a row of zeros): signals and frames [B, ...]."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    B = got.shape[0]
    d = np.abs(got - want).reshape(B, -1).max(axis=1)
    s = np.abs(want).reshape(B, -1).max(axis=1)
    return float((d / np.where(s > 0, s, 1.0)).max())
