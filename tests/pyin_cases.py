"""Seeded inputs of the probabilistic-YIN tests (tests/test_pyin.py on the CPU, tests/test_pyin_gpu.py on the GPU): the signals of
tests/pitch_cases.py at the shapes where the two kernels change path -- the smallest at which they can still go wrong.

The observation kernel gives a thread four lags and a bin's sum to the first trough of the bin; the decode gives a thread a bin
and a workgroup of whole waves a row.  So: 1, 2, 63, 64, 65, 368 and 1024 bins (one wave, its edge, a second wave, the limit), a
largest step of 1 and of n_bins (a window of three sources, and one that covers every bin from every bin), the lag ranges (2, 3)
(at most one trough), (45, 367) (the defaults) and (1, 1024) (the limit), rows of 1, 2 and 3 frames, a window that is no
multiple of four, silence and DC (d' flat at 1: no trough, v = 0), noise, and two rows of small integers whose d' is exactly 1/2
and 3/4 at a trough -- on a threshold of n_thresholds = 4, where `<=` in place of `<` moves a whole threshold's mass.
"""
import numpy as np

import pitch_cases as pc
import pyin_ref as yr

# d' of frames 1 .. 3 (window 8, hop 8, lags 1 .. 6) holds troughs at exactly 0.5 (row 0) and 0.75, 0.5 (row 1): every sum is
# a small integer, exact in float32, and the quotient is a dyadic rational
ON_THRESHOLD = ([1, -1, 2, 0, 0, 2, 2, 0, 0, -1, -2, -1, -1, 2, -2, 0, 0, 2, 0, 2, 1, 2, -1, 1, -1, 1, 0, 0, -1, 0, -1, 0, -1, 2, 0, 1, 2, 1, 2, 0],
                [-2, -2, 0, 0, 1, 1, 2, 2, 0, 1, 1, 0, 0, 2, 0, -1, 2, 1, -1, 0, -2, -1, -2, -1, 0, -2, 2, -1, 2, 1, 2, 2, 0, 2, 0, 0, -1, -1, -2, 0])


def _config(rate, hop, win, fmin, fmax, bps, n_bins=None, max_step=None, prior=None, **more):
    """the engine's keywords and the restatement's"""
    tau_min, tau_max = int(np.ceil(rate / fmax)), int(np.floor(rate / fmin))
    geo = yr.geometry(rate, hop, fmin, fmax, bps)
    nb = geo[0] if n_bins is None else n_bins
    ms = min(geo[1], nb) if max_step is None else max_step
    table = yr.prior() if prior is None else np.asarray(prior, np.float64)
    table = table.astype(np.float32).astype(np.float64)              # as the library receives it
    kw = dict(rate=rate, hop=hop, win=win, fmin=float(fmin), fmax=float(fmax), bins_per_semitone=bps, n_bins=nb, max_step=ms, **more)
    if prior is not None:
        kw['prior'] = table
    cfg = dict(rate=rate, tau_min=tau_min, tau_max=tau_max, prior_table=table, no_trough_prob=more.get('no_trough_prob', 0.01),
               fmin=float(fmin), bps=bps, n_bins=nb, max_step=ms, switch_prob=more.get('switch_prob', 0.01))
    return kw, cfg, dict(hop=hop, win=win)


def cases():
    """name -> dict(audio [B, N] with NaN behind every length, lengths [B], kinds [B], kw (HipEngine.pyin keywords), cfg
    (pyin_ref.decode keywords), grid (hop, win))"""
    out = {}

    def add(name, rows, lengths, kinds, conf):
        audio, lens = pc._batch(rows, lengths)
        out[name] = dict(audio=audio, lengths=lens, kinds=tuple(kinds), kw=conf[0], cfg=conf[1], grid=conf[2])

    def signals(kinds, n, period):
        return [pc.signal(k, n, period, seed=b) for b, k in enumerate(kinds)]

    # the defaults but the window: 368 bins, a step of 51, lags 45 .. 367; 12 frames and fewer
    kinds = ('vibrato', 'tone_noise', 'noise', 'zeros', 'missing_fundamental', 'sine_frac')
    add('default', signals(kinds, 3000, 120), (3000, 2999, 1500, 700, 3000, 255), kinds, _config(22050, 256, 256, 60, 500, 10))
    # lags 2 .. 3: at most one trough; rows of 1, 2 and 3 frames; 2 bins, a step of 1 and of 2
    kinds = ('sine_int', 'noise', 'tone_noise', 'dc')
    for ms in (1, 2):
        add(f'lags_2_3_step{ms}', signals(kinds, 40, 3), (1, 16, 40, 40), kinds, _config(6, 16, 64, 2, 3, 1, n_bins=2, max_step=ms))
    # the limits: lags 1 .. 1024, 1024 bins (the positions above them clip), a step of 1024 and of 1
    kinds = ('sine_frac', 'tone_noise')
    for ms in (1024, 1):
        add(f'limits_step{ms}', signals(kinds, 1500, 300), (1500, 1100), kinds, _config(1024, 256, 256, 1, 1024, 9, n_bins=1024, max_step=ms))
    # 101 lags, a window that is no multiple of four; the bins on both sides of a wave
    kinds = ('sine_frac', 'square', 'noise')
    for nb, ms in ((1, 1), (63, 63), (64, 1), (65, 65)):
        add(f'bins_{nb}', signals(kinds, 700, 60), (700, 451, 333), kinds, _config(300, 50, 202, 3, 300, 1, n_bins=nb, max_step=ms))
    # exactly on a threshold
    rows = [np.asarray(r, np.float32) for r in ON_THRESHOLD]
    add('on_threshold', rows, (40, 40), ('integers', 'integers'),
        _config(6, 8, 8, 1, 6, 1, prior=(0.4, 0.3, 0.2, 0.1), no_trough_prob=0.25, switch_prob=0.3))
    return out


def quality_signal(sigma, seed=0, rate=22050, seconds=2.0):
    """The condition's signal: three harmonics 0.5 / 0.25 / 0.4 of f(t) = 140 * 2^(0.1 sin(2 pi 5 t)) Hz plus white noise of
    deviation `sigma`; [0.5 s, 0.75 s) holds the noise alone -> (float64 [n], the pitch f [n], voiced bool [n])"""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n) / rate
    f = 140.0 * 2.0 ** (0.1 * np.sin(2 * np.pi * 5 * t))
    phase = 2 * np.pi * np.cumsum(f) / rate
    tone = 0.5 * np.sin(phase) + 0.25 * np.sin(2 * phase) + 0.4 * np.sin(3 * phase)
    voiced = ~((t >= 0.5) & (t < 0.75))
    return tone * voiced + sigma * rng.standard_normal(n), f, voiced
