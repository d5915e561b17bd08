"""numpy restatement of scipy.signal.resample (window=None, real input) as the engine computes it (csrc/resample.hip).

`resample` is the float64 rule set: rfft_N, keep bins 0 .. n//2 (n = min(N, M)), Nyquist x2 (down) or x0.5 (up) when n is
even, irfft_M, times M / N.  `resample_bluestein` restates the GPU algorithm in complex64: both transforms as Bluestein
convolutions of power-of-two length (L_fwd >= N + N//2, L_inv >= 2M - 1, both >= 64) with chirps evaluated in fp64 from
the exact phase j^2 mod 2K and rounded to complex64 once.  numpy's FFT computes in complex128 for complex64 input, so each
FFT result is rounded back to complex64 to model the fp32 passes.
"""
import numpy as np


def resampled_length(n, rate, target_rate):
    return int(n / rate * target_rate)


def _spectrum(X, N, M):
    """Y (M//2 + 1 bins) from X = rfft_N(x): truncate / zero-pad, Nyquist fix-up."""
    n = min(N, M)
    Y = np.zeros(M // 2 + 1, X.dtype)
    Y[:n // 2 + 1] = X[:n // 2 + 1]
    if n % 2 == 0:
        if M < N:
            Y[n // 2] *= 2.
        elif M > N:
            Y[n // 2] *= 0.5
    return Y


def resample(x, M):
    """float64 scipy.signal.resample(x, M)."""
    x = np.asarray(x, np.float64)
    N = x.size
    y = np.fft.irfft(_spectrum(np.fft.rfft(x), N, M), M)
    return y * (float(M) / float(N))


def bluestein_lengths(N, M):
    lf = max(64, 1 << int(np.ceil(np.log2(N + N // 2))))
    li = max(64, 1 << int(np.ceil(np.log2(2 * M - 1)))) if M > 1 else 64
    return lf, li


def _chirp(K, j):
    r = (j.astype(np.int64) ** 2) % (2 * K)
    return np.exp(-1j * np.pi * (r.astype(np.float64) / K)).astype(np.complex64)


def _filter_spectrum(K, K_out, L):
    h = np.zeros(L, np.complex64)
    j = np.arange(K_out)
    h[:K_out] = np.conj(_chirp(K, j))
    t = np.arange(1, K)
    h[L - t] = np.conj(_chirp(K, t))
    return _c64(np.fft.fft(h))


def _c64(a):
    return a.astype(np.complex64)


def _bluestein(a, K, K_out, L):
    """DFT_K(a)[0 .. K_out) in complex64 via a length-L convolution."""
    w = _chirp(K, np.arange(max(K, K_out)))
    s = np.zeros(L, np.complex64)
    s[:K] = _c64(a[:K] * w[:K])
    c = _c64(np.fft.ifft(_c64(_c64(np.fft.fft(s)) * _filter_spectrum(K, K_out, L))))
    return _c64(c[:K_out] * w[:K_out])


def resample_bluestein(x, M):
    """complex64 restatement of the GPU chain; returns float32."""
    x = np.asarray(x, np.float32)
    N = x.size
    lf, li = bluestein_lengths(N, M)
    X = _bluestein(x.astype(np.complex64), N, N // 2 + 1, lf)
    Y = _spectrum(X, N, M)
    Y[0] = Y[0].real
    if M % 2 == 0:
        Y[M // 2] = Y[M // 2].real
    Z = np.zeros(M, np.complex64)
    Z[:M // 2 + 1] = Y
    k = np.arange(M // 2 + 1, M)
    Z[k] = np.conj(Y[M - k])
    d = _bluestein(np.conj(Z), M, M, li)
    return (d.real.astype(np.float64) * (float(M) / float(N) / M)).astype(np.float32)
