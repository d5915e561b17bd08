"""Seeded inputs of the pitch tests (tests/test_pitch.py on the CPU, tests/test_pitch_gpu.py on the GPU): the signals and the
shapes -- the smallest at which the kernel can still go wrong.

A workgroup owns a frame, a thread four consecutive lags, and j advances four at a time: the shapes put the lag count on both
sides of a wave of owners (41 lags: 11 owners; 301: 76, not whole waves and above 256 lags; 368: 92; 1025: 257, the lone lag of
a fifth wave), the window on a multiple of four and off it (202), rows shorter than a hop, around a hop and around a window,
and frames that hang over both ends of a row.  One case sits exactly on the threshold (d' = 1 = threshold).
"""
import numpy as np

KINDS = ('sine_int', 'sine_frac', 'missing_fundamental', 'vibrato', 'tone_noise', 'noise', 'zeros', 'dc', 'square', 'full_scale')


def signal(kind, n, period, seed=0):
    """float32 [n]: `kind` at a period of `period` samples (an integer: 'sine_int' and 'square' use it as it is, the others
    a fraction off it)"""
    rng = np.random.default_rng([seed, KINDS.index(kind)])      # a longer row goes on where the shorter one ends
    t = np.arange(n, dtype=np.float64)
    frac = period * 1.0337                                       # no integer and no simple ratio of one
    if kind == 'sine_int':
        x = 0.5 * np.sin(2 * np.pi * t / period)
    elif kind == 'sine_frac':
        x = 0.4 * np.sin(2 * np.pi * t / frac + 0.3)
    elif kind == 'missing_fundamental':                          # harmonics 2 .. 5, the fundamental absent
        x = sum(0.2 / h * np.sin(2 * np.pi * h * t / frac + h) for h in range(2, 6))
    elif kind == 'vibrato':                                      # 3 % of frequency deviation, 5 Hz at 22050 samples a second
        phase = 2 * np.pi * t / frac - 0.03 * (22050 / (5 * frac)) * np.cos(2 * np.pi * 5 * t / 22050)
        x = 0.5 * np.sin(phase)
    elif kind == 'tone_noise':
        x = 0.5 * np.sin(2 * np.pi * t / frac) + 0.03 * rng.standard_normal(n)
    elif kind == 'noise':
        x = 0.3 * rng.standard_normal(n)
    elif kind == 'zeros':
        x = np.zeros(n)
    elif kind == 'dc':
        x = np.full(n, 0.3)
    elif kind == 'square':                                       # d(P) = d(2P) = 0 exactly: the smallest-tau tie
        x = np.where((np.arange(n) % period) < period // 2, 1.0, -1.0)
    elif kind == 'full_scale':
        x = np.sin(2 * np.pi * t / (frac * 0.731))
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def _config(rate, hop, win, fmin, fmax, threshold=0.1):
    """the engine's keywords and the lags they stand for"""
    tau_min, tau_max = int(np.ceil(rate / fmax)), int(np.floor(rate / fmin))
    return dict(rate=rate, hop=hop, win=win, fmin=float(fmin), fmax=float(fmax), threshold=threshold), dict(
        rate=rate, hop=hop, win=win, tau_min=tau_min, tau_max=tau_max, threshold=threshold)


def _batch(rows, lengths, poison=True):
    """[B, N] float32 with NaN behind every length"""
    N = max(len(r) for r in rows)
    audio = np.full((len(rows), N), np.nan if poison else 0.0, np.float32)
    for b, (r, n) in enumerate(zip(rows, lengths)):
        audio[b, :n] = r[:n]
    return audio, np.asarray(lengths, np.int32)


def cases():
    """name -> dict(audio [B, N], lengths [B], kinds [B], kw (HipEngine.pitch keywords), cfg (pitch_ref.track keywords))"""
    out = {}

    def add(name, kinds, n, lengths, period, conf):
        rows = [signal(k, n, period, seed=b) for b, k in enumerate(kinds)]
        audio, lens = _batch(rows, lengths)
        out[name] = dict(audio=audio, lengths=lens, kinds=tuple(kinds), kw=conf[0], cfg=conf[1])

    # lags 2 .. 40 at a window of 64 and a hop of 16: rows of 1 sample, around a hop, around a window and many frames
    add('small', ('sine_int', 'sine_frac', 'square', 'noise', 'tone_noise', 'dc', 'missing_fundamental', 'sine_int'), 500,
        (1, 15, 16, 17, 63, 64, 65, 500), 16, _config(80, 16, 64, 2, 40))
    # the defaults: every signal, 24 frames each
    add('default', KINDS, 6000, (6000,) * len(KINDS), 100, _config(22050, 256, 1024, 60, 500))
    # the limits: window = hop = 2048, lags 1 .. 1024, three frames
    add('limits', ('sine_frac',), 5000, (5000,), 300, _config(1024, 2048, 2048, 1, 1024))
    # 301 lags: above 256, no multiple of 64; a window that is no multiple of four
    add('odd', ('sine_frac', 'square'), 700, (700, 451), 60, _config(300, 50, 202, 1, 100))
    # a ragged batch of five rows at the defaults
    add('ragged', ('vibrato', 'sine_int', 'tone_noise', 'full_scale', 'missing_fundamental'), 3000, (3000, 1024, 1500, 255, 2999), 120,
        _config(22050, 256, 1024, 60, 500))
    # exactly on the threshold: d' of silence and of the inside of a DC row is 1 by rule, and 1 is an allowed threshold -- `<`
    # leaves those frames unvoiced at tau_min, `<=` would call them voiced
    add('on_threshold', ('zeros', 'dc'), 140, (140, 140), 16, _config(80, 16, 64, 2, 40, threshold=1.0))
    return out
