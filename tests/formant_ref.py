"""float64 numpy restatement of the cepstral envelope matching behind tts_hip_formant_match (csrc/stft_inv.hip), written from
its definition in include/tts_hip.h (steps 1 - 8) on top of tests/stft_inv_ref.py (`transform`, `time_frames`, `overlap_add`), one
row at a time.  `dtype=np.float32` runs the same code in float32: the distance of that run from the float64 one is what the GPU
bounds are derived from (tests/formant_cases.py).  `plant` names a deliberate mistake (MISTAKES) of the size a wrong kernel or
table would make.  The liftering table is one of the operation's constants: built in float64, rounded once to float32 (as the
library does) and cast up to `dtype`.  At the end: the synthetic vowel of the tests and the measurements taken on it (envelope
peaks, autocorrelation F0, inner RMS).
"""
import functools

import numpy as np

import stft_inv_ref as R

# endpoint weights w_j not 1; v_q not doubled; Q one short / one long; the floor missing; the floor applied to the log; the
# warp inverted (k * beta); no top-bin hold (zeros are read behind the top bin); the clamp applied to Sx before the
# subtraction; G in dB taken as nepers; the energy scaling missing; the energy scale without its square root; source and
# audio swapped; the gain on the real parts only
MISTAKES = ('w_edge', 'v_single', 'Q_minus', 'Q_plus', 'no_floor', 'floor_on_log', 'warp_inverted', 'no_top_hold', 'clamp_sx',
            'db_as_nepers', 'no_energy', 'energy_no_sqrt', 'swapped', 'real_only')
FLOOR = 1e-5
WARP_MIN, WARP_MAX, GAIN_DB_MAX = 0.5, 2.0, 60.0


def default_lifter(fl, sr=22050):
    """max(1, round(0.0015 * sr)) clipped to [1, fl // 2 - 1]."""
    return int(min(max(1, int(round(0.0015 * sr))), max(1, fl // 2 - 1)))


def lifter_table64(fl, Q, plant=None):
    """L [cut, cut] float64: L[j][k] = (w_j / n) sum_{q <= Q} v_q cos(2 pi q j / n) cos(2 pi q k / n); smoothed = row @ L."""
    cut = fl // 2 + 1
    Q = Q - 1 if plant == 'Q_minus' else Q + 1 if plant == 'Q_plus' else Q
    q, k = np.arange(Q + 1), np.arange(cut)
    C = np.cos(2.0 * np.pi * ((q[:, None] * k[None, :]) % fl) / fl)
    v = np.full(Q + 1, 1.0 if plant == 'v_single' else 2.0)
    v[0] = 1.0
    w = np.full(cut, 2.0)
    if plant != 'w_edge':
        w[0] = w[-1] = 1.0
    return (w[:, None] / fl) * ((C.T * v) @ C)


def lifter_table_fft(fl, Q):
    """The same through the transforms: the real cepstrum of every unit row's even extension (irfft), the quefrencies above Q
    zeroed, transformed back (rfft)."""
    cut = fl // 2 + 1
    c = np.fft.irfft(np.eye(cut), n=fl, axis=-1)
    c[:, Q + 1:fl - Q] = 0.0
    return np.fft.rfft(c, axis=-1).real


@functools.lru_cache(maxsize=None)
def lifter_table(fl, Q, plant=None):
    """The float32 table the call multiplies by."""
    t = lifter_table64(fl, Q, plant if plant in ('w_edge', 'v_single', 'Q_minus', 'Q_plus') else None).astype(np.float32)
    t.setflags(write=False)
    return t


def clamp_of(max_gain_db, plant=None):
    """G as the float32 the call uses."""
    return float(np.float32(max_gain_db if plant == 'db_as_nepers' else max_gain_db * np.log(10.0) / 20.0))


def magnitude(spec, g, dtype=np.float64):
    """|z| = sqrt(re * re + im * im), every operation rounded in `dtype`: [..., 2 cut] -> [..., cut]."""
    spec = np.asarray(spec, dtype)
    re, im = spec[..., :g.cut], spec[..., g.cut:]
    return np.sqrt(re * re + im * im)


def logmag(spec, g, dtype=np.float64, plant=None):
    """log(max(|X|, 1e-5)) of a spectrum [..., 2 cut] -> [..., cut]."""
    m = magnitude(spec, g, dtype)
    with np.errstate(divide='ignore'):
        if plant == 'no_floor':
            return np.log(m)
        if plant == 'floor_on_log':
            return np.maximum(np.log(m), dtype(FLOOR))
    return np.log(np.maximum(m, dtype(FLOOR)))


def envelope(l, g, Q, dtype=np.float64, plant=None):
    """S = l . L"""
    return np.asarray(l, dtype) @ lifter_table(g.fl, Q, plant).astype(dtype)


def positions(cut, beta, plant=None):
    """(i [cut], a [cut]): the bin below k / beta and the fraction (rounded to float32) of every bin k."""
    k = np.arange(cut, dtype=np.float64)
    pos = k * float(beta) if plant == 'warp_inverted' else k / float(beta)
    i = np.floor(pos)
    return i.astype(np.int64), (pos - i).astype(np.float32).astype(np.float64)


def warped(Sx, beta, dtype=np.float64, plant=None):
    """Sx [F, cut] read at k / beta: (1 - a) Sx[i] + a Sx[i + 1], the top bin held."""
    Sx = np.asarray(Sx, dtype)
    cut = Sx.shape[-1]
    i, a = positions(cut, beta, plant)
    a = a.astype(dtype)
    ext = np.concatenate([Sx, np.zeros(Sx.shape[:-1] + (cut + 2,), dtype)], axis=-1)    # what lies behind the top bin
    val = (dtype(1) - a) * ext[..., i] + a * ext[..., i + 1]
    if plant == 'no_top_hold':
        return val
    return np.where(i >= cut - 1, Sx[..., cut - 1:cut], val)


def gains(Sx, Sy, Y, g, beta, max_gain_db, dtype=np.float64, plant=None):
    """gain [F, cut] of steps 4 - 6 from the envelopes [F, cut] and the audio's spectrum Y [F, 2 cut]."""
    Sy = np.asarray(Sy, dtype)
    G = dtype(clamp_of(max_gain_db, plant))
    sx = warped(Sx, beta, dtype, plant)
    if plant == 'clamp_sx':
        gg = np.exp(np.clip(sx, -G, G) - Sy)
    else:
        gg = np.exp(np.clip(sx - Sy, -G, G))
    m = magnitude(Y, g, dtype)
    e0 = (m * m).sum(axis=-1, keepdims=True, dtype=dtype)
    e1 = ((gg * m) * (gg * m)).sum(axis=-1, keepdims=True, dtype=dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = e0 / np.where(e1 == 0, 1, e1)
        s = np.where(e1 == 0, 1, ratio if plant == 'energy_no_sqrt' else np.sqrt(ratio)).astype(dtype)
    if plant == 'no_energy':
        s = np.ones_like(s)
    return gg * s


def apply_gain(gain, Y, g, dtype=np.float64, plant=None):
    """Y' = gain * Y, both components."""
    Y, gain = np.asarray(Y, dtype), np.asarray(gain, dtype)
    re, im = gain * Y[..., :g.cut], gain * Y[..., g.cut:]
    return np.concatenate([re, Y[..., g.cut:] if plant == 'real_only' else im], axis=-1)


def row_spectrum(x, n, g, dtype=np.float64):
    """The row's own n samples, zero-padded as the plan pads a short row -> spectrum [F, 2 cut]."""
    row = np.zeros((1, max(n, g.wl)), dtype)
    row[0, :n] = np.asarray(x)[:n]
    return R.transform(row, g, dtype)[0]


def finish(frames, g, n, dtype=np.float64):
    """time frames [F, fl] -> the row's n samples: the leading min(n, samples(F)) of the overlap-add, 0 beyond."""
    F = frames.shape[0]
    audio = R.overlap_add(np.asarray(frames, dtype)[None], g, [F], dtype)[0]
    out = np.zeros(n, dtype)
    keep = max(0, min(n, g.samples(F)))
    out[:keep] = audio[:keep]
    return out


def stages(x, source, g, Q, warp=1.0, max_gain_db=24.0, n=None, dtype=np.float64, plant=None):
    """Every stage of one row x [n] against source [n] (None: x itself): spectrum [2, F, 2 cut] (source, then audio), logmag and
    envelope [2, F, cut], gain [F, cut], operand [F, 2 cut], frames [F, fl], audio [n]."""
    n = len(x) if n is None else n
    source = x if source is None else source
    if plant == 'swapped':
        x, source = source, x
    spec = np.stack([row_spectrum(source, n, g, dtype), row_spectrum(x, n, g, dtype)])
    l = logmag(spec, g, dtype, plant)
    S = envelope(l, g, Q, dtype, plant)
    gain = gains(S[0], S[1], spec[1], g, warp, max_gain_db, dtype, plant)
    op = apply_gain(gain, spec[1], g, dtype, plant)
    tf = R.time_frames(op[None], g, dtype)[0]
    return {'spectrum': spec, 'logmag': l, 'envelope': S, 'gain': gain, 'operand': op, 'frames': tf, 'audio': finish(tf, g, n, dtype)}


def formant_match(x, source, g, Q=None, warp=1.0, max_gain_db=24.0, dtype=np.float64, plant=None):
    Q = default_lifter(g.fl) if Q is None else Q
    return stages(x, source, g, Q, warp, max_gain_db, dtype=dtype, plant=plant)['audio']


# ---- comparison ----------------------------------------------------------------------------------------------------------
def abs_error(got, want):
    """max |got - want| (logarithms and their smoothed rows: values of a few units)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    return float(np.abs(got - want).max()) if got.size else 0.0


def gain_error(got, want):
    """max |got - want| / want (1 where want is 0: the frames behind a row's own)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    return float((np.abs(got - want) / np.where(want > 0, want, 1.0)).max()) if got.size else 0.0


# ---- the vowel and what is measured on it ------------------------------------------------------------------------------------
SR = 22050
F0 = 110.0
FORMANTS = ((700.0, 80.0), (1220.0, 90.0), (2600.0, 120.0))
VOWEL_STEPS = (-5, 4, 7)


@functools.lru_cache(maxsize=None)
def vowel(sr=SR, f0=F0):
    """1 s: an impulse train at f0 through three two-pole resonators, peak-normalised to 0.5."""
    from scipy.signal import lfilter
    x = np.zeros(sr)
    j = 0
    while int(j * sr / f0) < sr:
        x[int(j * sr / f0)] = 1.0
        j += 1
    for f, bw in FORMANTS:
        r = np.exp(-np.pi * bw / sr)
        x = lfilter([1 - r], [1, -2 * r * np.cos(2 * np.pi * f / sr), r * r], x)
    x = 0.5 * x / np.abs(x).max()
    x.setflags(write=False)
    return x


def mean_envelope(x, g, Q=33, edge=8):
    """The smoothed log-spectrum (float64 table) averaged over the frames edge .. F - edge -> [cut]."""
    spec = R.transform(np.asarray(x, np.float64)[None], g)[0]
    S = logmag(spec, g) @ lifter_table64(g.fl, Q)
    return S[edge:S.shape[0] - edge].mean(axis=0)


def envelope_peaks(x, g, Q=33, sr=SR):
    """(bins, Hz) of the local maxima of `mean_envelope`, lowest first."""
    e = mean_envelope(x, g, Q)
    k = np.flatnonzero((e[1:-1] > e[:-2]) & (e[1:-1] >= e[2:])) + 1
    return k, k * sr / g.fl


def nearest_peak(x, g, hz, Q=33, sr=SR):
    """The bin of the envelope peak nearest `hz`."""
    k, f = envelope_peaks(x, g, Q, sr)
    return int(k[np.argmin(np.abs(f - hz))])


def lowest_peak(x, g, Q=33, sr=SR):
    return int(envelope_peaks(x, g, Q, sr)[0][0])


def autocorr_f0(x, sr=SR, lo=60.0, hi=400.0, edge=2048):
    """F0 of the inner samples: the largest autocorrelation lag between sr / hi and sr / lo, refined by a parabola."""
    y = np.asarray(x, np.float64)[edge:len(x) - edge]
    y = y - y.mean()
    n = 1 << int(np.ceil(np.log2(2 * len(y))))
    ac = np.fft.irfft(np.abs(np.fft.rfft(y, n)) ** 2)[:len(y)]
    a, b = int(sr / hi), int(sr / lo)
    k = a + int(np.argmax(ac[a:b]))
    d = (ac[k - 1] - ac[k + 1]) / (2 * (ac[k - 1] - 2 * ac[k] + ac[k + 1]))
    return float(sr / (k + d))


def inner_rms(x, edge=2048):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)[edge:len(x) - edge]))))
