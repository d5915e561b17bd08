"""numpy restatement of the reference's rms, threshold and mean-window silence removal (utils/audio/audio_processing.py
:100-200, :385-394, :372-383) as csrc/silence.hip computes them, and the deterministic inputs of the silence tests.

The restatement is written from the description of the three methods, not from the reference's code: block peaks in fp32,
silences as (first block, end block) pairs, bounds in seconds as doubles, merging by each gap on its own, sample bounds as
truncated double products.  scripts/make_silence_fixture.py runs the reference itself on the same inputs and records length
and sha256 of every result in tests/golden/silence_fixture.json; tests/test_silence.py holds the restatement to it.

One deliberate difference: in the slice modes the reference raises IndexError for a row without any silence; here (and
on the GPU) the row comes back unchanged.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
WAV = os.path.join(GOLDEN, 'audio_test_16k.wav')
FIXTURE = os.path.join(GOLDEN, 'silence_fixture.json')


def _samples(v, rate):
    return int(v * rate) if isinstance(v, float) else int(v)


# ---------------------------------------------------------------------------------------------------------- rms
def rms_block_peaks(x, bs):
    """fp32 sqrt(max x * x) of every block of bs samples; the last block is zero-padded."""
    x = np.asarray(x, np.float32)
    nb = -(-len(x) // bs)
    sq = np.zeros(nb * bs, np.float32)
    sq[:len(x)] = x * x
    return np.sqrt(sq.reshape(nb, bs).max(axis=1))


def rms_flags(x, rate, threshold=-25, block_size=0.01, **_):
    """1 for every silent block of a row (the last block is zero-padded), uint8."""
    return (rms_block_peaks(x, _samples(block_size, rate)) < np.float32(10 ** (threshold / 20.0))).astype(np.uint8)


def rms_listed(x, rate, threshold=-25, min_silence=0.1, block_size=0.01, **_):
    """The silent runs [i, j) in blocks that last min_silence, in order: the silences before any merging."""
    bt = _samples(block_size, rate) / rate
    silent = rms_flags(x, rate, threshold, block_size)
    edge = np.diff(np.concatenate([[0], silent.astype(np.int8), [0]]))
    first, end = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)         # runs [i, j)
    assert end.size == 0 or end[-1] <= len(silent)
    return [(int(i), int(j)) for i, j in zip(first, end) if int(j - i) * bt >= min_silence]


def rms_links(listed, L, rate, block_size=0.01, min_voice_time=0.2, **_):
    """link[k]: listed silence k + 1 starts less than min_voice_time after silence k ends (Python doubles)."""
    bt = _samples(block_size, rate) / rate
    sil = [(i * bt, min(L / rate, j * bt)) for i, j in listed]
    if not min_voice_time:
        return [False] * max(0, len(sil) - 1)
    return [sil[k + 1][0] - sil[k][1] < min_voice_time for k in range(len(sil) - 1)]


def rms_silences(x, rate, threshold=-25, min_silence=0.1, block_size=0.01, min_voice_time=0.2):
    """The merged silences of a row as (s, e) in seconds (doubles)."""
    L, bs = len(x), _samples(block_size, rate)
    bt = bs / rate
    sil = [(i * bt, min(L / rate, j * bt)) for i, j in rms_listed(x, rate, threshold, min_silence, block_size)]
    if min_voice_time and len(sil) > 1:
        link = [sil[k + 1][0] - sil[k][1] < min_voice_time for k in range(len(sil) - 1)]
        merged, k = [], 0
        while k < len(sil):
            t = k
            while t < len(sil) - 1 and link[t]:
                t += 1
            merged.append((sil[k][0], sil[t][1]))
            k = t + 1
        sil = merged
    return sil


def rms_intervals(x, rate, mode='start_end', threshold=-25, min_silence=0.1, block_size=0.01, replace_by=0.5,
                  min_voice_time=0.2):
    """(dropped sample intervals [(d0, d1)] sorted by d0, tail cut): a row keeps t < cut outside every [d0, d1).  Mode
    remove: one interval per merged silence ((S, S), empty, for the trailing one, which moves the cut, and for one that
    replace_by covers); the slice modes: the one interval [0, a) and the cut b of the slice [a, b)."""
    x = np.asarray(x, np.float32)
    L, rb = len(x), _samples(replace_by, rate)
    sil = rms_silences(x, rate, threshold, min_silence, block_size, min_voice_time)
    if mode == 'remove':
        h, cut, iv = rb // 2, L, []
        for s, e in sil:
            S, E = int(s * rate), int(e * rate)
            if S == 0:
                iv.append((0, max(0, E - rb)))
            elif abs(E - L) <= 1:
                cut = min(cut, L, S + rb)
                iv.append((S, S))
            elif S + h < E - h:
                iv.append((S + h, E - h))
            else:
                iv.append((S, S))
        return iv, cut
    assert mode in ('start', 'end', 'start_end')
    a, b = 0, L
    if sil:
        if 'end' in mode and abs(sil[-1][1] * rate - L) <= 1:
            b = min(L, int(sil[-1][0] * rate) + rb)
        if 'start' in mode and sil[0][0] == 0:
            a = max(0, int(sil[0][1] * rate) - rb)
    return [(0, a)], b


def interval_mask(L, intervals, cut):
    keep = np.arange(L) < cut
    for d0, d1 in intervals:
        keep[d0:max(d0, d1)] = False
    return keep.astype(np.uint8)


def trim_rms(x, rate, mode='start_end', threshold=-25, min_silence=0.1, block_size=0.01, replace_by=0.5,
             min_voice_time=0.2):
    x = np.asarray(x, np.float32)
    L, rb = len(x), _samples(replace_by, rate)
    sil = rms_silences(x, rate, threshold, min_silence, block_size, min_voice_time)
    if mode == 'remove':
        h = rb // 2
        keep = np.ones(L, bool)
        for s, e in sil:
            S, E = int(s * rate), int(e * rate)
            if S == 0:
                keep[:max(0, E - rb)] = False
            elif abs(E - L) <= 1:
                keep[S + rb:] = False
            elif S + h < E - h:
                keep[S + h:E - h] = False
        return x[keep]
    assert mode in ('start', 'end', 'start_end')
    if not sil:
        return x                                    # the reference raises IndexError here
    a, b = 0, L
    if 'end' in mode and abs(sil[-1][1] * rate - L) <= 1:
        b = min(L, int(sil[-1][0] * rate) + rb)
    if 'start' in mode and sil[0][0] == 0:
        a = max(0, int(sil[0][1] * rate) - rb)
    return x[a:b] if a < b else x[:0]


def rms_margin(x, rate, threshold=-25, block_size=0.01, **_):
    """Smallest relative distance of a block peak from the amplitude threshold."""
    thr = np.float32(10 ** (threshold / 20.0))
    return float(np.abs(rms_block_peaks(x, _samples(block_size, rate)).astype(np.float64) / float(thr) - 1).min())


# ---------------------------------------------------------------------------------------------------------- threshold
def trim_threshold(x, threshold=0.1, mode='start_end', **_):
    x = np.asarray(x, np.float32)
    assert mode in ('start', 'end', 'start_end')
    m = np.float32(np.mean(x))
    idx = np.flatnonzero(np.abs(x - m) > np.float32(threshold))
    if idx.size == 0:
        return x
    a = int(idx[0]) if 'start' in mode else 0
    b = int(idx[-1]) if 'end' in mode else len(x)
    return x[a:b] if a < b else x[:0]


def threshold_intervals(x, threshold=0.1, mode='start_end', **_):
    """The slice [a, b) of trim_threshold as ([(0, a)], b)."""
    x = np.asarray(x, np.float32)
    idx = np.flatnonzero(np.abs(x - np.float32(np.mean(x))) > np.float32(threshold))
    if idx.size == 0:
        return [(0, 0)], len(x)
    return [(0, int(idx[0]) if 'start' in mode else 0)], int(idx[-1]) if 'end' in mode else len(x)


def threshold_margin(x, threshold=0.1, **_):
    x = np.asarray(x, np.float32)
    d = np.abs(x.astype(np.float64) - float(np.float32(np.mean(x))))
    return float(np.abs(d - float(np.float32(threshold))).min())


# ---------------------------------------------------------------------------------------------------------- mean window
def mean_window_conv(x, rate, threshold=0.025, min_silence=0.15):
    """np.convolve(x * x, ones(w) / (w * threshold), 'same') as box sums over a double prefix sum."""
    x = np.asarray(x, np.float32)
    L, w = len(x), int(min_silence * rate)
    if L < w:
        raise ValueError(f'a row of L = {L} samples is shorter than the window w = {w}')
    p = np.concatenate([[0.0], np.cumsum((x * x).astype(np.float64))])
    i = np.arange(L)
    hi = np.minimum(L - 1, i + (w - 1) // 2)
    lo = np.maximum(0, i + (w - 1) // 2 - (w - 1))
    return (p[hi + 1] - p[lo]) * (1.0 / (w * threshold))


def trim_mean_window(x, rate, threshold=0.025, min_silence=0.15, **_):
    x = np.asarray(x, np.float32)
    conv = mean_window_conv(x, rate, threshold, min_silence)
    return x[conv > min(threshold, np.mean(conv) / 2)]


def mean_window_margin(x, rate, threshold=0.025, min_silence=0.15, **_):
    conv = mean_window_conv(x, rate, threshold, min_silence)
    th = min(threshold, np.mean(conv) / 2)
    return float(np.abs(conv / th - 1).min())


def square_prefix(x):
    """P[t] = sum of the fp32 squares x[0 .. t) for t in [0, L], accumulated in np.longdouble."""
    x = np.asarray(x, np.float32)
    return np.concatenate([[np.longdouble(0)], np.cumsum((x * x).astype(np.longdouble))])


def mean_window_long(x, rate, threshold=0.025, min_silence=0.15, **_):
    """(keep mask, margin) of the mean-window method with every sum in np.longdouble: what decides a row so long that the
    order of an fp64 summation shows in the last digits of its prefix sums."""
    L, w = len(x), int(min_silence * rate)
    p = square_prefix(x)
    i = np.arange(L)
    hi = np.minimum(L - 1, i + (w - 1) // 2)
    lo = np.maximum(0, i + (w - 1) // 2 - (w - 1))
    conv = (p[hi + 1] - p[lo]) * np.longdouble(1.0 / (w * threshold))
    th = min(np.longdouble(threshold), np.mean(conv) / 2)
    return (conv > th).astype(np.uint8), float(np.abs(conv / th - 1).min())


def keep_mask(method, x, rate, **kw):
    """uint8 [L]: 1 for the samples `run` keeps."""
    x = np.asarray(x, np.float32)
    if method == 'rms':
        return interval_mask(len(x), *rms_intervals(x, rate, **kw))
    if method == 'threshold':
        return interval_mask(len(x), *threshold_intervals(x, **kw))
    conv = mean_window_conv(x, rate, **kw)
    return (conv > min(kw.get('threshold', 0.025), np.mean(conv) / 2)).astype(np.uint8)


METHODS = {'rms': trim_rms, 'threshold': trim_threshold, 'remove': trim_mean_window}


def run(method, x, rate, **kw):
    if method == 'threshold':
        return trim_threshold(x, **kw)
    return METHODS[method](x, rate, **kw)


def margin(method, x, rate, **kw):
    return {'rms': rms_margin, 'remove': mean_window_margin}[method](x, rate, **kw) if method != 'threshold' \
        else threshold_margin(x, **kw)


MARGINS = {'rms': 1e-6, 'threshold': 1e-5, 'remove': 1e-9}     # relative, absolute, relative


# ---------------------------------------------------------------------------------------------------------- inputs
def lcg(n, seed):
    """n values of the LCG s <- 1664525 s + 1013904223 (mod 2^32) after `seed`, built by doubling jumps."""
    a, c, mask = np.uint64(1664525), np.uint64(1013904223), np.uint64(0xffffffff)
    s = np.empty(max(n, 1), np.uint64)
    s[0] = (a * np.uint64(seed & 0xffffffff) + c) & mask
    m, A, C = 1, a, c
    while m < n:
        k = min(m, n - m)
        s[m:m + k] = (A * s[:k] + C) & mask
        C = (A * C + C) & mask
        A = (A * A) & mask
        m *= 2
    return s[:n]


def build(rate, segments, seed=1, tones=((220.0, 0.6), (557.0, 0.3), (1310.0, 0.1)), dither=2e-3, offset=0.0):
    """Sum of sines under a piecewise constant envelope, plus dither of amplitude `dither` and a constant offset.
    segments: (length, amplitude) pairs; a float length is seconds, an int is samples."""
    lens = [_samples(d, rate) for d, _ in segments]
    n = sum(lens)
    env = np.concatenate([np.full(k, amp, np.float64) for k, (_, amp) in zip(lens, segments)]) if n else np.zeros(0)
    t = np.arange(n) / rate
    sig = sum(a * np.sin(2 * np.pi * f * t + 0.3 * i) for i, (f, a) in enumerate(tones))
    noise = ((lcg(n, seed) >> np.uint64(8)).astype(np.float64) / float(1 << 24) - 0.5) * 2 * dither
    return (env * sig + noise + offset).astype(np.float32)


LOUD, Q = 0.5, 0.0
R = 22050


def _long_segments():
    """198 450 samples: leading silence, eight utterances with growing pauses, a last utterance up to the end."""
    seg = [(0.4, Q)]
    for k in range(8):
        seg += [(0.45 + 0.03 * k, LOUD), (0.25 + 0.04 * k, Q)]
    return seg + [(198450 - sum(_samples(d, R) for d, _ in seg), LOUD)]


INPUTS = {
    # one pause inside the utterance, longer / shorter than min_silence = 0.1 s
    'pause_long': (R, [(0.3, LOUD), (0.6, Q), (0.4, LOUD)], 1),
    'pause_short': (R, [(0.3, LOUD), (0.06, Q), (0.4, LOUD)], 2),
    # silence - voice - silence - a 0.12 s burst - silence - voice - silence
    'burst': (R, [(0.25, Q), (0.4, LOUD), (0.3, Q), (0.12, LOUD), (0.3, Q), (0.4, LOUD), (0.2, Q)], 3),
    'ends': (R, [(0.35, Q), (0.5, LOUD), (0.3, Q), (0.3, LOUD), (0.45, Q)], 4),
    # nine loud blocks of 220 samples, then silence: its first sample is (int)(9 * (220 / 22050) * 22050) = 1979
    'block9': (R, [(9 * 220, LOUD), (0.3, Q), (0.2, LOUD)], 5),
    'all_loud': (R, [(0.5, LOUD)], 6),
    'all_silent': (R, [(1.2, Q)], 7),
    'one_sample': (R, [(1, LOUD)], 8),
    'short_row': (R, [(100, LOUD)], 9),
    'tail_kbs': (R, [(0.3, LOUD), (220 * 30, Q)], 10),                  # L = k * bs, trailing silence
    'tail_kbs1': (R, [(0.3, LOUD), (220 * 30 + 1, Q)], 11),             # L = k * bs + 1
    'rate16k': (16000, [(0.2, Q), (0.4, LOUD), (0.35, Q), (0.3, LOUD), (0.25, Q)], 12),
    'rate44k': (44100, [(0.15, Q), (0.3, LOUD), (0.25, Q), (0.2, LOUD), (0.1, Q)], 13),
    # ~9 s with many pauses: the kept samples straddle many tiles of the compaction
    'long': (R, _long_segments(), 14),
    # threshold method: quiet - loud - quiet with an offset (the mean matters), nothing loud, one loud sample
    'thr_mid': (R, [(0.1, 0.05), (0.13, LOUD), (0.08, 0.05)], 15),
    'thr_offset': (R, [(0.12, 0.02), (0.1, 0.4), (0.1, 0.02)], 16),
    'thr_quiet': (R, [(0.2, 0.05)], 17),
    # mean-window method
    'mw_pattern': (R, [(0.3, Q), (0.5, LOUD), (0.4, 0.01), (0.3, LOUD), (0.3, Q)], 18),
    'mw_exact': (R, [(1500, LOUD), (3307 - 1500, Q)], 19),              # L == w
    'mw_16k': (16000, [(0.2, LOUD), (0.5, Q), (0.3, LOUD)], 20),
}
_OFFSETS = {'thr_offset': 0.25}
_cache = {}


def make_input(name):
    """(rate, float32 row) of a named input; 'wav' is the normalized golden recording (16 kHz)."""
    if name not in _cache:
        if name == 'wav':
            from scipy.io import wavfile
            rate, raw = wavfile.read(WAV)
            a = raw - np.mean(raw)
            _cache[name] = (int(rate), (a * (1. / np.max(np.abs(a)))).astype(np.float32))
        elif name == 'thr_spike':
            x = build(R, [(0.1, 0.05)], 21)
            x[1000] = 0.9
            _cache[name] = (R, x)
        else:
            rate, seg, seed = INPUTS[name]
            _cache[name] = (rate, build(rate, seg, seed, offset=_OFFSETS.get(name, 0.0)))
        _cache[name][1].setflags(write=False)
    return _cache[name]


RMS_MODES = ('start_end', 'start', 'end', 'remove')
SLICE_MODES = RMS_MODES[:3]


def _cases():
    c = []

    def add(name, inp, method, **kw):
        c.append((name, inp, method, kw))

    for mode in RMS_MODES:
        add(f'pause_long-{mode}', 'pause_long', 'rms', mode=mode, replace_by=0.2)
        add(f'pause_short-{mode}', 'pause_short', 'rms', mode=mode)
        add(f'ends-{mode}', 'ends', 'rms', mode=mode, replace_by=0.2)
        add(f'ends-{mode}-rb0', 'ends', 'rms', mode=mode, replace_by=0)
        add(f'ends-{mode}-int', 'ends', 'rms', mode=mode, block_size=256, replace_by=1000, min_silence=0.05)
        add(f'all_loud-{mode}', 'all_loud', 'rms', mode=mode)
        add(f'all_silent-{mode}', 'all_silent', 'rms', mode=mode)
        add(f'one_sample-{mode}', 'one_sample', 'rms', mode=mode)
        add(f'short_row-{mode}', 'short_row', 'rms', mode=mode)
        add(f'tail_kbs-{mode}', 'tail_kbs', 'rms', mode=mode, replace_by=0.1)
        add(f'tail_kbs1-{mode}', 'tail_kbs1', 'rms', mode=mode, replace_by=0.1)
        add(f'rate16k-{mode}', 'rate16k', 'rms', mode=mode, replace_by=0.1)
        add(f'rate44k-{mode}', 'rate44k', 'rms', mode=mode, replace_by=0.05, min_voice_time=0)
        for db in (-25, -35, -15):
            add(f'wav-{mode}{db}', 'wav', 'rms', mode=mode, threshold=db, min_silence=0.1, replace_by=0.4)
    add('burst-merged', 'burst', 'rms', mode='remove', replace_by=0.1, min_voice_time=0.2)
    add('burst-kept', 'burst', 'rms', mode='remove', replace_by=0.1, min_voice_time=0)
    add('burst-start_end', 'burst', 'rms', mode='start_end', replace_by=0.1)
    add('pause_long-rb_longer', 'pause_long', 'rms', mode='remove', replace_by=0.8)
    add('pause_long-rb0', 'pause_long', 'rms', mode='remove', replace_by=0)
    add('block9-remove', 'block9', 'rms', mode='remove', replace_by=0.1)
    add('long-remove', 'long', 'rms', mode='remove', replace_by=0.1)
    add('long-start_end', 'long', 'rms', mode='start_end', replace_by=0.1)
    for mode in SLICE_MODES:
        add(f'thr_mid-{mode}', 'thr_mid', 'threshold', mode=mode)
        add(f'thr_offset-{mode}', 'thr_offset', 'threshold', mode=mode, threshold=0.2)
        add(f'thr_spike-{mode}', 'thr_spike', 'threshold', mode=mode, threshold=0.3)
    add('thr_quiet', 'thr_quiet', 'threshold')
    add('wav-threshold', 'wav', 'threshold')
    add('mw_pattern', 'mw_pattern', 'remove')
    add('mw_pattern-even', 'mw_pattern', 'remove', min_silence=0.2, threshold=0.05)
    add('mw_pattern-small', 'mw_pattern', 'remove', min_silence=0.01)
    add('mw_exact', 'mw_exact', 'remove')
    add('mw_16k', 'mw_16k', 'remove')
    add('wav-remove', 'wav', 'remove')
    return c


CASES = _cases()            # (case name, input name, method, keywords)
