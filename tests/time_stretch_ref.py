"""float64 numpy restatement of the phase-locked vocoder behind tts_hip_time_stretch (csrc/stft_inv.hip), written from its
definition in include/tts_hip.h on top of tests/stft_inv_ref.py (`transform`, `inverse`) with complex numbers, one row at a
time.  `dtype=np.float32` runs the same code in float32 / complex64: the distance of that run from the float64 one is what
the GPU bounds are derived from (tests/time_stretch_cases.py).  `plant` names a deliberate mistake (MISTAKES) of the size a
wrong kernel would make; 'no_locking' is the textbook phase vocoder (librosa.phase_vocoder's recurrence).
"""
import numpy as np

import stft_inv_ref as R

# every bin accumulates its own phase; A[t] where A[t-1] belongs; own of frame t - 1; a tie to the upper peak; a and 1 - a
# swapped; rate inverted; T one short; the zero frame behind the row missing (frame F - 1 repeated); R conjugated; P(0) = 0
MISTAKES = ('no_locking', 'adv_t', 'own_prev', 'tie_up', 'a_swapped', 'rate_inverted', 'T_short', 'no_zero_frame', 'rel_conj',
            'p0_zero')
RATE_MIN, RATE_MAX = 0.25, 4.0


def out_frames(F, r):
    """The smallest T with T * r >= F."""
    T = int(np.ceil(F / r))
    while T > 1 and (T - 1) * r >= F:
        T -= 1
    while T * r < F:
        T += 1
    return T


def out_samples(n, r):
    """llrint(n / r): to nearest, ties to even."""
    return int(np.rint(n / r))


def positions(F, r, plant=None):
    """(i [T], a [T]): the analysis frame and the fraction (rounded to float32) of every output frame."""
    r = float(r)
    if plant == 'rate_inverted':
        r = 1.0 / r
    T = out_frames(F, r)
    if plant == 'T_short':
        T = max(1, T - 1)
    pos = np.arange(T, dtype=np.float64) * r
    i = np.floor(pos)
    return i.astype(np.int64), (pos - i).astype(np.float32).astype(np.float64)


def to_complex(spec, g, dtype=np.float64):
    """[..., 2 cut] (real parts, then imaginary parts) -> complex [..., cut]."""
    spec = np.asarray(spec, dtype)
    return (spec[..., :g.cut] + 1j * spec[..., g.cut:]).astype(np.complex64 if dtype == np.float32 else np.complex128)


def from_complex(z):
    return np.concatenate([z.real, z.imag], axis=-1)


def P(z, plant=None):
    """z / |z|, (1, 0) at the origin."""
    m = np.abs(z)
    zero = m == 0
    out = z / np.where(zero, 1, m)
    return np.where(zero, 0 if plant == 'p0_zero' else 1, out).astype(z.dtype)


def frame_pairs(X, r, plant=None):
    """X complex [F, cut] -> (c0, c1 [T, cut], a [T]); frames at and beyond F are 0."""
    F = X.shape[0]
    i, a = positions(F, r, plant)
    tail = np.zeros((max(0, int(i.max()) + 2 - F), X.shape[1]), X.dtype)
    if plant == 'no_zero_frame' and len(tail):
        tail[0] = X[F - 1]
    Xz = np.concatenate([X, tail])
    return Xz[i], Xz[i + 1], a


def magnitudes(X, r, dtype=np.float64, plant=None):
    """m [T, cut] = (1 - a) |c0| + a |c1|, every operation rounded in `dtype`."""
    c0, c1, a = frame_pairs(X, r, plant)
    a = a.astype(dtype)[:, None]
    m0, m1 = np.abs(c0).astype(dtype), np.abs(c1).astype(dtype)
    if dtype == np.float32:                                     # |z| as the header states it, not numpy's hypot
        m0 = np.sqrt(c0.real * c0.real + c0.imag * c0.imag)
        m1 = np.sqrt(c1.real * c1.real + c1.imag * c1.imag)
    one = dtype(1)
    if plant == 'a_swapped':
        return a * m0 + (one - a) * m1
    return (one - a) * m0 + a * m1


def peaks_of(m):
    """bool [cut]: positive, above both left neighbours, not below both right ones; outside the frame counts as -inf."""
    inf = np.full(2, -np.inf)
    e = np.concatenate([inf, np.asarray(m, np.float64), inf])
    c = e[2:-2]
    return (c > 0) & (c > e[1:-3]) & (c > e[:-4]) & (c >= e[3:-1]) & (c >= e[4:])


def owners_of(m, plant=None):
    """int [cut]: the nearest peak of every bin (a tie goes to the lower one), -1 everywhere in a frame without peaks."""
    cut = len(m)
    pk = np.flatnonzero(peaks_of(m))
    if len(pk) == 0:
        return np.full(cut, -1, np.int64)
    k = np.arange(cut)
    j = np.searchsorted(pk, k)                                  # pk[j] is the first peak at or above k
    big = 4 * cut
    left, right = pk[np.maximum(j - 1, 0)], pk[np.minimum(j, len(pk) - 1)]
    dl = np.where(j > 0, k - left, big)
    dr = np.where(j < len(pk), right - k, big)
    return np.where((dl < dr) if plant == 'tie_up' else (dl <= dr), left, right)


def owners(m, plant=None):
    return np.stack([owners_of(row, plant) for row in np.asarray(m)])


def chain(X, r, m, own, dtype=np.float64, plant=None, lock=True):
    """The operand Y complex [T, cut] from the spectrum X [F, cut], magnitudes m and owners own of the output frames."""
    c0, c1, _ = frame_pairs(X, r, plant)
    T, cut = c0.shape
    m = np.asarray(m, dtype)
    A = P(c1 * np.conj(c0), plant)
    U = P(X[0], plant)
    Y = np.zeros((T, cut), X.dtype)
    Y[0] = m[0] * U
    for t in range(1, T):
        o = own[t - 1] if plant == 'own_prev' else own[t]
        At = A[t] if plant == 'adv_t' else A[t - 1]
        if not lock or plant == 'no_locking' or o[0] < 0:
            U = (U * At).astype(X.dtype)
        else:
            rel = c0[t] * np.conj(c0[t][o])
            Rt = P(np.conj(rel) if plant == 'rel_conj' else rel, plant)
            U = P(((U[o] * At[o]).astype(X.dtype) * Rt).astype(X.dtype), plant)
        Y[t] = m[t] * U
    return Y


def row_spectrum(x, n, g, dtype=np.float64):
    """The row's own n samples, zero-padded as the plan pads a short row -> spectrum [F, 2 cut]."""
    row = np.zeros((1, max(n, g.wl)), dtype)
    row[0, :n] = np.asarray(x)[:n]
    return R.transform(row, g, dtype)[0]


def finish(frames, g, n, r, dtype=np.float64, plant=None):
    """time frames [T, fl] -> the row's out_samples(n, r) samples: the leading min(S, samples(T)) of the overlap-add, 0 beyond."""
    T = frames.shape[0]
    audio = R.overlap_add(np.asarray(frames, dtype)[None], g, [T], dtype)[0]
    S = out_samples(n, 1.0 / r if plant == 'rate_inverted' else r)
    out = np.zeros(S, dtype)
    keep = max(0, min(S, g.samples(T)))
    out[:keep] = audio[:keep]
    return out


def stages(x, g, r, n=None, dtype=np.float64, plant=None, lock=True):
    """Every stage of one row x [n] at rate r: spectrum [F, 2 cut], magnitude [T, cut], owner [T, cut], operand [T, 2 cut],
    frames [T, fl], audio [S]."""
    n = len(x) if n is None else n
    spec = row_spectrum(x, n, g, dtype)
    X = to_complex(spec, g, dtype)
    m = magnitudes(X, r, dtype, plant)
    own = owners(m, plant)
    op = from_complex(chain(X, r, m, own, dtype, plant, lock)).astype(dtype)
    tf = R.time_frames(op[None], g, dtype)[0]
    return {'spectrum': spec, 'magnitude': m, 'owner': own, 'operand': op, 'frames': tf, 'audio': finish(tf, g, n, r, dtype, plant)}


def time_stretch(x, g, r, n=None, dtype=np.float64, plant=None, lock=True):
    return stages(x, g, r, n, dtype, plant, lock)['audio']


def pitch_shift(x, g, n_steps, bins_per_octave=12):
    """float64: the stretch by 2 ** (-n_steps / bins_per_octave), scipy's FFT resampling by (1_000_000, round(r * 1_000_000)),
    cut or zero-padded to the input's length -- what effects.pitch_shift composes."""
    from scipy.signal import resample
    r = 2.0 ** (-n_steps / bins_per_octave)
    p, q = 1_000_000, int(round(r * 1_000_000))
    y = time_stretch(np.asarray(x, np.float64), g, r)
    y = resample(y, int(len(y) / p * q))
    out = np.zeros(len(x))
    out[:min(len(x), len(y))] = y[:len(x)]
    return out


# ---- comparison ----------------------------------------------------------------------------------------------------------
def magnitude_error(got, want):
    """Worst frame of max |got - want| / the frame's largest want (1 for a frame of zeros)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float('inf')
    scale = want.max(axis=-1)
    return float((np.abs(got - want).max(axis=-1) / np.where(scale > 0, scale, 1.0)).max())


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def dominant_hz(x, sr=22050, n_fft=1 << 20):
    """Frequency of the largest bin of a zero-padded FFT."""
    return float(np.argmax(np.abs(np.fft.rfft(np.asarray(x, np.float64), n_fft))) * sr / n_fft)
