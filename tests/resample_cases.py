"""Shared case table of the resampling stage tests (tests/test_resample_stages.py on the CPU, _gpu.py on an MI355X).

csrc/resample.hip resamples a row of N samples to M with two Bluestein chains (tests/resample_ref.py restates the rule set
and the complex64 chain): rfft_N on L_fwd = 2^logf >= N + N // 2 points, irfft_M on L_inv = 2^logi >= 2 M - 1 points, both at
least 64.  Every chain is FFT(signal), FFT(filter), product, inverse FFT, and every FFT of 2^logL points is `rs_fft`:
- logL <= 13: one workgroup per line, `lds_fft` with logP = logL, nl = 1;
- logL >= 14: the four-step split L = 8192 x L2.  Forward: L2-point FFTs down the columns (`lds_fft` with logP = logL - 13,
  nl = 8192 / L2 adjacent columns per workgroup), the twiddle W_L^(n1 k2), then 8192-point FFTs along the rows.  It leaves
  stored[k2 * 8192 + k1] = X[k2 + L2 * k1]; the inverse (rows, twiddle, columns) takes that order and returns the natural
  one, unscaled.
`lds_fft` is a radix-4 Stockham with one radix-2 stage at the end when logP is odd.  Rows of a batch with equal
(logf, logi) form a group that shares one chain of launches; a group's rows find their own N_b / M_b through `rows`, their
spectrum at `row * xstride` (xstride = the group's largest N_b // 2 + 1) of a workspace every group reuses in turn.

This module restates those rules (`rs_lens`, `passes`, `groups`, `stored_index`), restates the passes in numpy at the
granularity a mistake can be planted at (`lds_fft`, `four_step`, `bluestein`, `inverse_input`, `batch_spectra`), and holds
the inputs, the bounds and the cases of both test files.  References are float64: np.fft, or a closed form where one exists.
Errors are max abs error over the reference's max abs (`stage_error`).
"""
import functools
from typing import NamedTuple

import numpy as np

import resample_ref

PMAX, LOG_PMAX = 8192, 13       # points of one workgroup's FFT (64 KiB of LDS)
RS_MAX_LEN = 1 << 24            # samples per row, in and out
FFT_MIN_LOG, FFT_MAX_LOG = 6, 25
LIM31 = 1 << 31                 # bytes the staged buffers may hold

# ---- bounds ------------------------------------------------------------------------------------------------------------
# About 10x the worst error measured on an MI355X over every case of test_resample_stages_gpu.py, as stage_error.  The
# measured values stand next to each bound; DESIGN.md 4.6 has them per length.  What keeps a bound honest is
# test_resample_stages.py: every planted mistake must exceed ten times the bound of the stage it belongs to.
BOUNDS = {
    'fft': 5e-6,            # rs_fft alone, 2^6 .. 2^25, both directions: measured 4.58e-7 (impulses, 2^22 forward); tones 1.20e-7,
                            # random lines 2.04e-7 (2^22 inverse)
    'roundtrip': 3e-6,      # inverse(forward(x)) against L * x, and the other way round: measured 3.00e-7 (2^22)
    'spectrum': 1.2e-5,     # the forward chain, rfft_N bins 0 .. N // 2: measured 1.17e-6 (pow2_2e23_to_2e22, impulse_last)
    'resample': 1.3e-5,     # end to end: measured 1.31e-6 (pow2_2e23_to_2e24, dc_tone); test_resample_gpu.py's white-noise rows
                            # up to 65 537 samples keep their 2e-6
}


# ---- the dispatch rules ------------------------------------------------------------------------------------------------
def ceil_log2(v):
    return max(0, (int(v) - 1).bit_length())


def rs_lens(n, m):
    """(logf, logi) of a row of n samples resampled to m (audio_call.h rs_lens)."""
    return max(6, ceil_log2(n + n // 2)), max(6, ceil_log2(2 * m - 1))


def smallest_n_for_fwd(k):
    """The smallest N whose forward transform has 2^k points: N + N // 2 > 2^(k - 1) (k = 6: every N up to 42 has 64)."""
    n = (1 << (k - 1)) * 2 // 3
    while n + n // 2 <= 1 << (k - 1):
        n += 1
    assert rs_lens(n, 1)[0] == k and (n == 1 or rs_lens(n - 1, 1)[0] < k or k == 6)
    return n


def smallest_m_for_inv(k):
    """The smallest M whose inverse transform has 2^k points: 2 M - 1 > 2^(k - 1)."""
    m = (1 << (k - 2)) + 1
    assert rs_lens(1, m)[1] == k and (rs_lens(1, m - 1)[1] < k or k == 6)
    return m


class Pass(NamedTuple):
    kind: str       # 'lds' one workgroup per line; 'col' / 'row' the two passes of the four-step split
    logP: int       # points per lds_fft line
    nl: int         # lines per workgroup


def passes(logL):
    """The `lds_fft` configurations one forward FFT of 2^logL points launches (the inverse: the same two, rows first)."""
    if logL <= LOG_PMAX:
        return (Pass('lds', logL, 1),)
    c = logL - LOG_PMAX
    return (Pass('col', c, PMAX >> c), Pass('row', LOG_PMAX, 1))


class Group(NamedTuple):
    logf: int
    logi: int
    rows: tuple     # batch rows, ascending
    xstride: int    # complex bins between two rows' spectra in the workspace


def groups(lens, mlens):
    """The groups of a batch in launch order, as resample_run forms them (a std::map keyed by (logf, logi))."""
    by_key = {}
    for b, (n, m) in enumerate(zip(lens, mlens)):
        by_key.setdefault(rs_lens(n, m), []).append(b)
    return [Group(k[0], k[1], tuple(r), max(lens[b] // 2 + 1 for b in r)) for k, r in sorted(by_key.items())]


# ---- the stored order --------------------------------------------------------------------------------------------------
def stored_index(logL, swap=False):
    """idx with stored[i] = X[idx[i]]: the identity up to 2^13, else stored[k2 * 8192 + k1] = X[k2 + L2 * k1].
    swap (a planted mistake): k1 and k2 change roles, stored[k1 * L2 + k2]."""
    L = 1 << logL
    if logL <= LOG_PMAX:
        return np.arange(L)
    L2 = L >> LOG_PMAX
    k2, k1 = np.arange(L2)[:, None], np.arange(PMAX)[None, :]
    idx = k2 + L2 * k1
    return (idx.T if swap else idx).reshape(-1)


def stored_position(logL, k):
    """Where bin k lies in the stored order."""
    if logL <= LOG_PMAX:
        return int(k)
    L2 = 1 << (logL - LOG_PMAX)
    return int(k % L2) * PMAX + int(k // L2)


# ---- numpy restatements of the passes (complex128: only a planted mistake makes them wrong) ------------------------------
def lds_fft(a, inverse=False, skip_tail=False):
    """`lds_fft` on the last axis (2^logP points): radix-4 Stockham stages with Ns = 1, 4, 16, ..., then one radix-2 stage
    when logP is odd.  Unscaled in both directions.  skip_tail (a planted mistake) leaves that stage out."""
    a = np.asarray(a, np.complex128)
    P = a.shape[-1]
    logP = P.bit_length() - 1
    assert 1 << logP == P
    sign = 1.0 if inverse else -1.0
    Ns, logNs = 1, 0
    while logNs + 2 <= logP:
        q = P >> 2
        jj = np.arange(q)
        k = jj & (Ns - 1)
        v = [a[..., jj + r * q] * np.exp(sign * 2j * np.pi * r * k / (4 * Ns)) for r in range(4)]
        s02, d02, s13, d13 = v[0] + v[2], v[0] - v[2], v[1] + v[3], v[1] - v[3]
        mi = sign * 1j * d13                                    # forward -i d13, inverse +i d13
        out = np.empty_like(a)
        base = ((jj >> logNs) << (logNs + 2)) + k
        for r, val in enumerate((s02 + s13, d02 + mi, s02 - s13, d02 - mi)):
            out[..., base + r * Ns] = val
        a, Ns, logNs = out, Ns << 2, logNs + 2
    if logNs < logP and not skip_tail:
        h = P >> 1
        jj = np.arange(h)
        k = jj & (Ns - 1)
        lo, hi = a[..., jj], a[..., jj + h] * np.exp(sign * 2j * np.pi * k / (2 * Ns))
        out = np.empty_like(a)
        base = ((jj >> logNs) << (logNs + 1)) + k
        out[..., base] = lo + hi
        out[..., base + Ns] = lo - hi
        a = out
    return a


def four_step(x, inverse=False, mistake=None):
    """rs_fft<LD_PLAIN, ST_PLAIN> on the last axis: forward natural -> stored order, inverse stored -> natural, unscaled.
    mistake: 'twiddle_j_plus_1' (exponent s * (j + 1)), 'inverse_twiddle_not_conjugated', 'skip_radix2_tail'."""
    x = np.asarray(x, np.complex128)
    L = x.shape[-1]
    logL = L.bit_length() - 1
    tail = mistake == 'skip_radix2_tail'
    if logL <= LOG_PMAX:
        return lds_fft(x, inverse, tail)
    L2 = L >> LOG_PMAX
    u = x.reshape(x.shape[:-1] + (L2, PMAX))                    # element (j, s) at offset s + j * 8192
    s, j = np.arange(PMAX)[None, :], np.arange(L2)[:, None]
    e = s * (j + 1) if mistake == 'twiddle_j_plus_1' else s * j
    sign = 1.0 if inverse and mistake != 'inverse_twiddle_not_conjugated' else -1.0
    tw = np.exp(sign * 2j * np.pi * (e % L) / L)
    if not inverse:                                             # columns and twiddle, then rows
        u = np.swapaxes(lds_fft(np.swapaxes(u, -1, -2), False, tail), -1, -2) * tw
        u = lds_fft(u, False, tail)
    else:                                                       # rows and twiddle, then columns
        u = lds_fft(u, True, tail) * tw
        u = np.swapaxes(lds_fft(np.swapaxes(u, -1, -2), True, tail), -1, -2)
    return u.reshape(x.shape)


def chirp(j, K, fp32_square=False):
    """exp(-i pi j^2 / K) with the phase j^2 mod 2K reduced in integers.  fp32_square (a planted mistake): j * j in fp32."""
    j = np.asarray(j, np.int64)
    sq = (j.astype(np.float32) * j.astype(np.float32)).astype(np.int64) if fp32_square else j * j
    return np.exp(-1j * np.pi * ((sq % (2 * K)) / K))


def bluestein(a, K, K_out, L, fp32_square=False):
    """DFT_K(a)[0 .. K_out) through a circular convolution of L points (resample.hip's chain, in complex128).  L below
    K + K_out - 1 wraps around (a planted mistake: L_fwd one power short)."""
    w = chirp(np.arange(max(K, K_out)), K, fp32_square)
    s = np.zeros(L, np.complex128)
    s[:K] = np.asarray(a)[:K] * w[:K]
    h = np.zeros(L, np.complex128)                              # chirp_filter: conj(w_j) for j < K_out, else conj(w_(L - j))
    j = np.arange(L)                                            # for L - j < K, else 0
    head, tail = j < K_out, (L - j < K) & (j >= K_out)
    h[head] = np.conj(chirp(j[head], K, fp32_square))
    h[tail] = np.conj(chirp(L - j[tail], K, fp32_square))
    c = np.fft.ifft(np.fft.fft(s) * np.fft.fft(h))
    return c[:K_out] * w[:K_out]


def inverse_input(X, N, M, mistake=None):
    """conj(Z) [M] of the LD_INV_IN loads, element by element as the kernel reads it: off < M, mirror = off > M // 2,
    k = M - off or off, kept when k <= min(N, M) // 2; bin n / 2 (n even, M != N) x2 down / x0.5 up; imaginary parts of bin
    0 and, M even, bin M / 2 dropped; conjugated unless mirrored.  mistakes: 'nyquist_factor_swapped', 'nyquist_at_equal_length',
    'nyquist_imag_kept', 'mirror_off_by_one'."""
    X = np.asarray(X, np.complex128)
    off = np.arange(M)
    mirror = off > M // 2
    k = np.where(mirror, (M - off - 1) if mistake == 'mirror_off_by_one' else (M - off), off)
    n = min(N, M)
    keep = (k <= n // 2) & (k >= 0)
    y = np.where(keep, X[np.clip(k, 0, X.size - 1)], 0)
    if n % 2 == 0 and (M != N or mistake == 'nyquist_at_equal_length'):
        f = 2.0 if M < N else 0.5
        if mistake == 'nyquist_factor_swapped':
            f = 1.0 / f
        y = np.where(k == n // 2, y * f, y)
    real_only = (k == 0)
    if M % 2 == 0 and mistake != 'nyquist_imag_kept':
        real_only = real_only | (k == M // 2)
    y = np.where(real_only, y.real, y)
    return np.where(mirror, y, np.conj(y))


def resample_by_passes(x, M, mistake=None, lf_short=False, fp32_square=False):
    """float64 resampling put together from `bluestein` and `inverse_input` the way the kernel chains them."""
    x = np.asarray(x, np.float64)
    N = x.size
    logf, logi = rs_lens(N, M)
    X = bluestein(x, N, N // 2 + 1, 1 << (logf - 1 if lf_short else logf), fp32_square)
    d = bluestein(inverse_input(X, N, M, mistake), M, M, 1 << logi, fp32_square)
    return d.real / N                                           # Re(w_j c_j) / M * (M / N)


def spectrum_by_passes(x, lf_short=False, fp32_square=False):
    x = np.asarray(x, np.float64)
    N = x.size
    return bluestein(x, N, N // 2 + 1, 1 << (rs_lens(N, 1)[0] - 1 if lf_short else rs_lens(N, 1)[0]), fp32_square)


def batch_spectra(a, lens, mlens, mistake=None):
    """The spectrum probe's [B][N // 2 + 1] of a ragged batch with the workspace indexing restated: group by group, row i of a
    group stores rfft_{N_b}(x_b) bins 0 .. N_b // 2 at i * xstride of one flat buffer every group reuses, and the copy-out
    reads it back from there.  mistakes: 'neighbour_length' (row i of a group takes the N_b of row i + 1 of its group),
    'xstride_of_other_group' (the stride of the next group in launch order)."""
    a = np.asarray(a, np.float64)
    B, N = a.shape
    out = np.zeros((B, N // 2 + 1), np.complex128)
    gs = groups(lens, mlens)
    flat = np.zeros(max(len(g.rows) * g.xstride for g in gs) + N // 2 + 1, np.complex128)
    for gi, g in enumerate(gs):
        xs = gs[(gi + 1) % len(gs)].xstride if mistake == 'xstride_of_other_group' else g.xstride
        own = [lens[b] for b in g.rows]
        used = own[1:] + own[:1] if mistake == 'neighbour_length' else own
        for i, b in enumerate(g.rows):
            nb = min(used[i], N)
            flat[i * xs:i * xs + nb // 2 + 1] = np.fft.rfft(a[b, :nb])
        for i, b in enumerate(g.rows):
            nb = lens[b]
            out[b, :nb // 2 + 1] = flat[i * xs:i * xs + nb // 2 + 1]
    return out


# ---- closed forms ------------------------------------------------------------------------------------------------------
def impulse_spectrum(N, n0):
    """rfft_N of a unit impulse at n0: exp(-2 pi i k n0 / N), the phase reduced in integers."""
    k = np.arange(N // 2 + 1, dtype=np.int64)
    return np.exp(-2j * np.pi * ((k * n0) % N) / N)


def impulse_resampled(N, M, n0):
    """scipy.signal.resample(unit impulse at n0 of N samples, M): the periodic sinc (Dirichlet kernel) over the kept bins
    -h .. h, plus the scaled bin n / 2 when n = min(N, M) is even and M != N."""
    if M == N:
        y = np.zeros(M)
        y[n0] = 1.0
        return y
    n = min(N, M)
    h = (n - 1) // 2
    t = np.arange(M, dtype=np.float64) / M - n0 / N
    t -= np.round(t)
    den = np.sin(np.pi * t)
    near = np.abs(den) < 1e-12
    y = np.where(near, 2 * h + 1.0, np.sin(np.pi * (2 * h + 1) * t) / np.where(near, 1.0, den))
    if n % 2 == 0:
        j = np.arange(M, dtype=np.float64)
        if M < N:       # Y[M / 2] = 2 X[M / 2], its real part alternates in sign over the output
            y = y + 2.0 * np.cos(2 * np.pi * ((M // 2 * n0) % N) / N) * np.where(np.arange(M) % 2 == 0, 1.0, -1.0)
        else:           # Y[N / 2] = X[N / 2] / 2 = (-1)^n0 / 2, an inner bin of the M-point transform
            y = y + (1.0 if n0 % 2 == 0 else -1.0) * np.cos(np.pi * j * N / M)
    return y / N


# ---- inputs ------------------------------------------------------------------------------------------------------------
INPUTS = ('noise', 'dc_tone', 'burst', 'impulse_first', 'impulse_last', 'nyquist')


def make_input(kind, N, M, seed=0):
    """One fp32 row of N samples.  'noise' white; 'dc_tone' 0.5 + 0.4 sin + 1e-3 noise; 'burst' 50 samples of noise at 1
    over 1e-3 noise, ending at the last sample; 'impulse_first' / 'impulse_last' one 1 at sample 0 / N - 1; 'nyquist' a
    cosine exactly on bin min(N, M) / 2 of the N-point DFT (even min(N, M))."""
    rng = np.random.default_rng(1000 + seed + N + 7 * M)
    if kind == 'noise':
        x = rng.standard_normal(N)
    elif kind == 'dc_tone':
        x = 0.5 + 0.4 * np.sin(2 * np.pi * 0.0137 * np.arange(N)) + 1e-3 * rng.standard_normal(N)
    elif kind == 'burst':
        x = 1e-3 * rng.standard_normal(N)
        x[max(0, N - 50):] += rng.standard_normal(min(N, 50))
    elif kind in ('impulse_first', 'impulse_last'):
        x = np.zeros(N)
        x[0 if kind == 'impulse_first' else N - 1] = 1.0
    elif kind == 'nyquist':
        n = min(N, M)
        assert n % 2 == 0
        x = np.cos(2 * np.pi * ((n // 2 * np.arange(N, dtype=np.int64)) % N) / N)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def impulse_at(kind, N):
    return {'impulse_first': 0, 'impulse_last': N - 1}.get(kind)


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    """One call on B = len(inputs) rows of N samples each (one group), resampled rate -> target to M samples."""
    name: str
    N: int
    M: int
    rate: int
    target: int
    inputs: tuple

    @property
    def logs(self):
        return rs_lens(self.N, self.M)


def _case(name, N, M, inputs, rate=None, target=None):
    rate, target = (N, M) if rate is None else (rate, target)
    assert int(N / rate * target) == M and rate != target, (name, N, M)
    assert all(k != 'nyquist' or min(N, M) % 2 == 0 for k in inputs)
    return Case(name, N, M, rate, target, tuple(inputs))


ALL_BUT_NYQUIST = INPUTS[:5]
LARGE = ('dc_tone', 'impulse_last')     # the input the complex64 restatement is worst on, and the largest chirp index


def _length_cases():
    out = []
    # one case per power of two: the smallest N with L_fwd = 2^k to the smallest M with L_inv = 2^k (a down-sampling by
    # about 4 : 3); up to 2^20 every input, above it two rows
    for k in range(6, 23):
        out.append(_case(f'len_2e{k}', smallest_n_for_fwd(k), smallest_m_for_inv(k), ALL_BUT_NYQUIST if k <= 20 else LARGE))
    # from L_fwd = 2^23 up a power-of-two N (the float64 reference of an awkward N of this size takes ten seconds)
    for ln, lm in ((22, 21), (22, 23), (23, 22), (23, 24), (24, 23)):
        out.append(_case(f'pow2_2e{ln}_to_2e{lm}', 1 << ln, 1 << lm, LARGE))
    return out


CASES = tuple(_length_cases() + [
    # even min(N, M): the bin the Nyquist rule scales carries the whole signal; one workgroup and four-step
    _case('nyquist_down', 1002, 334, ('nyquist', 'noise', 'impulse_last')),
    _case('nyquist_up', 334, 1002, ('nyquist', 'noise', 'impulse_last')),
    _case('nyquist_down_4step', 40002, 13334, ('nyquist', 'noise', 'impulse_last')),
    _case('nyquist_up_4step', 13334, 40002, ('nyquist', 'noise', 'impulse_last')),
    # M == N with rates that differ: every bin kept, bin N / 2 not scaled
    _case('equal_length', 500, 500, ('nyquist', 'noise', 'impulse_last'), rate=1000, target=1001),
    _case('equal_length_4step', 6000, 6000, ('nyquist', 'noise', 'impulse_last'), rate=12000, target=12001),
    # even M below an even N (the imaginary part of bin M / 2 is dropped), odd M above an even N
    _case('down_even_even', 1000, 500, ('noise', 'dc_tone', 'impulse_last')),
    _case('up_even_odd', 1000, 1501, ('noise', 'dc_tone', 'impulse_last')),
    # L_inv far above L_fwd: up-sampling 1 : 8 into the four-step inverse
    _case('up_1_to_8', 3000, 24000, ('noise', 'burst', 'impulse_last')),
])
BY_NAME = {c.name: c for c in CASES}


class Ragged(NamedTuple):
    """One ragged call: rows of lens[b] samples in a [B, max(lens)] batch with NaN beyond each row."""
    name: str
    lens: tuple
    rate: int
    target: int

    @property
    def mlens(self):
        return tuple(resample_ref.resampled_length(n, self.rate, self.target) for n in self.lens)


# two groups of three non-adjacent rows of different N_b, one four-step group of two, two single rows, interleaved
_GROUP_LENS = (700, 2800, 6000, 30, 900, 3500, 2, 8000, 1000, 4000)
RAGGED = (
    Ragged('groups_down', _GROUP_LENS, 2, 1),                   # L_fwd > L_inv in every group
    Ragged('groups_up', _GROUP_LENS, 1, 2),                     # L_fwd < L_inv
    Ragged('one_sample_out', (3, 5, 4, 1500, 3), 3, 1),         # rows with M_b = 1 next to one of 500
    Ragged('small', (100, 64), 2, 1),                           # the small call between two large ones
)
RAGGED_BY_NAME = {c.name: c for c in RAGGED}


def ragged_batch(case):
    """[B, max(lens)] fp32: dc + tone + noise rows (each row its own frequency), NaN beyond every row's length."""
    rng = np.random.default_rng(77 + len(case.lens) + case.rate)
    N = max(case.lens)
    a = np.full((len(case.lens), N), np.nan, np.float32)
    for b, n in enumerate(case.lens):
        a[b, :n] = 0.3 + 0.4 * np.sin(2 * np.pi * (0.01 + 0.003 * b) * np.arange(n)) + 0.2 * rng.standard_normal(n)
    return a


# FFT probe: bins / samples of the impulses and tones of a 2^logL-point line
def fft_points(logL):
    L = 1 << logL
    rng = np.random.default_rng(logL)
    pts = [0, 1, 8191, 8192, 8193, L // 2, L - 1, int(rng.integers(0, L))]
    out = []
    for p in pts:
        if p < L and p not in out:
            out.append(p)
    return out


FFT_LOGS = tuple(range(FFT_MIN_LOG, FFT_MAX_LOG + 1))
FFT_FULL_CHECK_MAX_LOG = 22     # above: every k2 for a few k1 and every k1 for a few k2; no random lines


def fft_lines_per_call(logL):
    """Lines of one probe call: all of them while lines * 2^logL * 8 bytes stays below 2^31, at most 8 at a time."""
    return max(1, min(8, (LIM31 - 1) // (8 << logL)))


def reached():
    """What the tables reach: ({logL of the FFT probe cases}, {logf}, {logi}) over CASES and RAGGED."""
    logf = {c.logs[0] for c in CASES} | {rs_lens(n, m)[0] for r in RAGGED for n, m in zip(r.lens, r.mlens)}
    logi = {c.logs[1] for c in CASES} | {rs_lens(n, m)[1] for r in RAGGED for n, m in zip(r.lens, r.mlens)}
    return set(FFT_LOGS), logf, logi


# ---- references --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def case_inputs(name):
    """[B, N] fp32 rows of a case (read-only)."""
    c = BY_NAME[name]
    a = np.stack([make_input(k, c.N, c.M, i) for i, k in enumerate(c.inputs)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=4)
def case_reference(name):
    """(spectra [B, N // 2 + 1] complex128, resampled [B, M] float64) of a case, from np.fft in float64 (read-only)."""
    c = BY_NAME[name]
    a = case_inputs(name).astype(np.float64)
    X = np.fft.rfft(a, axis=1)
    y = np.stack([resample_ref.resample(r, c.M) for r in a])
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


# ---- comparison --------------------------------------------------------------------------------------------------------
def stage_error(got, ref):
    """max |got - ref| / max |ref| (|ref| = 0 everywhere: the absolute error)."""
    got, ref = np.asarray(got), np.asarray(ref)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return err / scale if scale > 0 else err


def as_complex(a):
    """Interleaved (re, im) fp32 [..., 2] -> complex64 [...]."""
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.complex64).reshape(a.shape[:-1])
