"""Seeded inputs of the MCD / DTW tests (tests/test_mel_dtw.py on the CPU, tests/test_mel_dtw_gpu.py on the GPU): log-mel-like
frames, smooth in time, clipped to [ln 1e-5, 2], float32.

A case is one pair (la x lb frames) of one kind:
  identical  b = a (la == lb)
  repeat     every frame of a repeated r = lb / la times as b
  warped     b = a read along a monotone time warp, plus noise
  unrelated  two independent draws
The shapes are those of the issue plus one on each side of every size the kernels have: the sweep's strip of 256 columns (3 x 256,
3 x 257, 3 x 512, 3 x 513), the cepstra kernel's chunk of 32 frames and the path kernel's rounds of 64 pairs (32 x 33, 33 x 32:
64 diagonals; 33 x 33: 65), the cepstra kernel's pass of 64 DCT rows (R = 64, 65 on 128 channels), and the un-aligned
reduction's block of 256 threads, each of which takes the diagonal's frames t, t + 256, ... (UNALIGNED: min(la, lb) = 256, 257,
512, 513 beside shorter ones).
"""
import functools

import numpy as np

LOG_FLOOR, LOG_CEIL = float(np.log(1e-5)), 2.0

# name -> (la, lb, kind, n_mel, n_cep, include_c0)
CASES = {}
for la, lb, kind in [(1, 1, 'unrelated'), (1, 70, 'repeat'), (70, 1, 'unrelated'), (2, 2, 'identical'), (5, 64, 'unrelated'),
                     (5, 65, 'repeat'), (64, 5, 'unrelated'), (65, 5, 'unrelated'), (3, 256, 'unrelated'), (3, 257, 'unrelated'),
                     (257, 3, 'unrelated'), (3, 1025, 'unrelated'), (1025, 3, 'unrelated'), (97, 130, 'warped'), (130, 97, 'warped'),
                     (257, 300, 'warped'), (3, 512, 'unrelated'), (3, 513, 'repeat'), (32, 33, 'warped'), (33, 32, 'unrelated'),
                     (33, 33, 'identical'), (256, 300, 'warped'), (520, 512, 'warped'), (520, 513, 'warped')]:
    CASES[f'{la}x{lb}_{kind}'] = (la, lb, kind, 80, 13, False)
CASES['40x52_warped_mel128_cep24'] = (40, 52, 'warped', 128, 24, False)
CASES['40x52_warped_c0'] = (40, 52, 'warped', 80, 13, True)
CASES['9x12_warped_mel128_rows64'] = (9, 12, 'warped', 128, 64, False)
CASES['9x12_warped_mel128_rows65'] = (9, 12, 'warped', 128, 64, True)
# The cases whose float64 path is decided by more than twice the cost bound at every cell (tests/test_mel_dtw.py establishes
# that these are the ones): only there is the GPU's path length held to the float64 path's.
UNSTABLE_PATHS = ('3x257_unrelated', '3x512_unrelated', '3x1025_unrelated', '1025x3_unrelated', '520x512_warped', '520x513_warped')
STABLE_PATHS = tuple(n for n in CASES if n not in UNSTABLE_PATHS)
UNALIGNED = ('1x70_repeat', '97x130_warped', '256x300_warped', '257x300_warped', '520x512_warped', '520x513_warped')
RAGGED = ('97x130_warped', '5x65_repeat', '33x33_identical', '3x257_unrelated', '70x1_unrelated')      # the batch of five


def log_mel(rng, T, n_mel=80):
    """[T, n_mel] float32: a spectral tilt plus noise smoothed over nine frames and five channels, clipped"""
    x = rng.standard_normal((T + 8, n_mel + 4))
    x = sum(x[s:s + T] for s in range(9)) / 3.0
    x = sum(x[:, s:s + n_mel] for s in range(5)) / np.sqrt(5.0)
    m = -4.0 - 4.0 * np.arange(n_mel) / n_mel + 2.5 * x
    return np.clip(m, LOG_FLOOR, LOG_CEIL).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair(name):
    """-> (a [la, n_mel], b [lb, n_mel]) float32"""
    la, lb, kind, n_mel, _, _ = CASES[name]
    rng = np.random.default_rng([la, lb, n_mel, len(kind)])
    a = log_mel(rng, la, n_mel)
    if kind == 'identical':
        assert la == lb
        b = a.copy()
    elif kind == 'repeat':
        assert lb % la == 0
        b = np.repeat(a, lb // la, axis=0)
    elif kind == 'warped':
        t = np.linspace(0.0, 1.0, lb)
        src = np.clip(np.round((t + 0.08 * np.sin(2 * np.pi * t)) * (la - 1)).astype(int), 0, la - 1)
        b = np.clip(a[np.maximum.accumulate(src)] + 0.3 * rng.standard_normal((lb, n_mel)), LOG_FLOOR, LOG_CEIL).astype(np.float32)
    else:
        b = log_mel(rng, lb, n_mel)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def settings(name):
    _, _, _, _, n_cep, c0 = CASES[name]
    return dict(n_cep=n_cep, include_c0=c0)


def ragged_batch(names=RAGGED, fill=np.nan):
    """The rows `names` (all of 80 channels, 13 coefficients) as one padded batch -> (a [B, Ta, 80], b [B, Tb, 80], la, lb);
    `fill` stands at and behind the lengths."""
    pairs = [pair(n) for n in names]
    la, lb = np.array([len(p[0]) for p in pairs], np.int32), np.array([len(p[1]) for p in pairs], np.int32)
    a = np.full((len(pairs), la.max(), 80), fill, np.float32)
    b = np.full((len(pairs), lb.max(), 80), fill, np.float32)
    for r, (x, y) in enumerate(pairs):
        a[r, :len(x)], b[r, :len(y)] = x, y
    return a, b, la, lb
