"""Shared case table of the trim-convolution tests (tests/test_reduce_noise_stages.py on the CPU,
test_reduce_noise_stages_gpu.py on an MI355X).

`tts_hip_trim_silence` convolves the squared samples with a triangular window of W = 2 * (window_length // 2) taps:
audio_trim_conv_kernel stages TRIM_OUT = 1024 outputs per block and TRIM_JC = 1024 taps per pass (the taps rounded up to a
multiple of 4 with zeros) for rows of at least W samples, audio_trim_conv_short_kernel does the rows shorter than the window.
`HipEngine.trim_silence_probe` returns the convolution itself; the reference is np.convolve in float64 on the float32
squares.  Zeros are exact; every other value lies within (W + 2) * 2^-52 relative: the terms are non-negative (no
cancellation) and summed with fp64 fma, W products and W - 1 sums whatever their order.
"""
import functools
from typing import NamedTuple

import numpy as np

TRIM_OUT = TRIM_JC = 1024
MODES = ('start_end', 'start', 'end')
THRESHOLD_MARGIN = 1e-12        # no convolution value of a case lies this close (relative) to a threshold


class Case(NamedTuple):
    name: str
    wl: int
    lengths: tuple
    tail: int = 0

    @property
    def W(self):
        return 2 * (self.wl // 2)

    @property
    def N(self):
        return max(self.lengths) + self.tail


def _mixed(wl):
    """Rows with L - W + 1 = 2049, 1025, 1024, 1023 and 2 outputs, L = W, and two rows shorter than the window (W - 1 and
    1): both kernels launch."""
    W = 2 * (wl // 2)
    return Case(f'wl{wl}_mixed', wl, (W + 2048, W + 1024, W + 1023, W + 1022, W + 1, W, W - 1, 1), tail=3)


CASES = (
    # window lengths around TRIM_JC with W % 4 of 0 and 2 (5 -> W = 4; 1022, 1026 -> W % 4 = 2), two passes (2048), and the
    # default 0.2 s at 22 050 Hz (4410, W % 4 = 2) and one above it (4411 -> W = 4410)
    *(_mixed(wl) for wl in (4, 5, 1022, 1024, 1026, 2048, 4410, 4411)),
    Case('wl1024_one_output', 1024, (1024,)),
    Case('wl1024_short_only', 1024, (1000, 1, 512, 1023 - 23)),          # N < W: only the short kernel
    Case('wl4410_one_sample', 4410, (1,)),
)
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(c.name for c in CASES)


def audio_of(case):
    """(audio [B, N] float32, lengths int32 [B]): rows of a block of ones, zeros, noise with a loud middle third, in turn --
    in the mixed cases the row that fills one block exactly (1024 outputs, row 2) and the row of L = W (one output, row 5)
    carry noise; NaN (even rows) or 1e30 garbage (odd rows) past L_b."""
    rng = np.random.default_rng(700 + case.wl + 13 * len(case.lengths) + case.N)
    a = np.zeros((len(case.lengths), case.N), np.float32)
    for b, L in enumerate(case.lengths):
        if (b + 1) % 3 == 0:
            x = 0.003 * rng.standard_normal(L)
            x[L // 3:2 * L // 3] += 0.4 * rng.standard_normal(2 * L // 3 - L // 3)
        elif (b + 1) % 3 == 1:
            x = np.zeros(L)
            x[L // 4:L // 4 + max(L // 3, 1)] = 1.0
        else:
            x = np.zeros(L)
        a[b, :L] = x
        a[b, L:] = np.nan if b % 2 == 0 else 1e30 * rng.standard_normal(case.N - L)
    return a, np.asarray(case.lengths, np.int32)


def window(wl):
    h = wl // 2
    return np.concatenate([np.linspace(0, 1, h), np.linspace(1, 0, h)]) / h


@functools.lru_cache(maxsize=None)
def reference(name):
    """[conv_b] of a case: np.convolve(float64(float32(x)^2), window, 'valid') per row (read-only)."""
    case = BY_NAME[name]
    a, lens = audio_of(case)
    out = [np.convolve(np.power(a[b, :L], 2).astype(np.float64), window(case.wl), mode='valid') for b, L in enumerate(lens)]
    for v in out:
        v.setflags(write=False)
    return out


def conv_error(got, want):
    """max |got - want| / want of a row; where want is 0, got must be 0 (else inf)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.isfinite(got).all() or (got[want == 0] != 0).any():
        return float('inf')
    nz = want != 0
    return float((np.abs(got[nz] - want[nz]) / want[nz]).max()) if nz.any() else 0.0


def thresholds(conv, wl, threshold=0.1):
    """(th_end, th_start) of trim_silence_window for a convolution row."""
    return (min(threshold, max(np.mean(conv[-wl:]) * 5, threshold / 50)), min(threshold, max(np.mean(conv[:wl]) * 5, threshold / 50)))
