"""CPU: the definitions behind time stretching (csrc/stft_inv.hip: tts_hip_time_stretch) -- the float64 restatement of the
phase-locked vocoder (tests/time_stretch_ref.py) on its own: amplitude and frequency at every rate, where the textbook vocoder
loses the amplitude, pitch shifting, the owners at their edges; the bounds the GPU tests use (each above the float32 numpy
copy's own distance from float64 and a factor ten below every planted mistake); the host-only front end (csrc/audio_call.h:
time_stretch_check) through csrc/host_check.cpp's --time-stretch mode, built with -fsanitize=address,undefined as a
stand-alone program; and `speed` / `pitch_steps` through the sentence pipeline on a recording stand-in engine."""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import stft_inv_ref as R
import time_stretch_cases as C
import time_stretch_ref as V
from test_audio_call import carved, ceil_div, checker      # noqa: F401  (checker: the fixture)

G = C.GEOMS['default']
SR = 22050
FREQS = (220.3, 226.1, 1000.0)
CHECK_RATES = (0.25, 0.5, 0.8, 1.25, 1.37, 2.0, 4.0)
RMS_WANT, RMS_TOL, HZ_TOL, EDGE = 0.3808, 0.02, 0.5, 2048


@functools.lru_cache(maxsize=None)
def two_tones(f):
    rng = np.random.default_rng(int(f))
    t = np.arange(SR) / SR
    x = 0.5 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 3.1 * f * t) + 1e-3 * rng.standard_normal(SR)
    x.setflags(write=False)
    return x


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', ['small', 'gapped', 'default'])
def test_rate_one_is_the_stft_round_trip(group):
    g = C.GEOMS[group]
    x = C.signal('noisy', 11 * g.fl // 2 + 3, g, seed=1).astype(np.float64)
    st = V.stages(x, g, 1.0)
    spec = R.transform(x[None], g)
    assert R.frame_error(st['operand'][None], spec, g) <= 1e-12
    keep = g.samples(g.frames(len(x)))
    assert len(st['audio']) == len(x) and keep <= len(x)
    assert np.abs(st['audio'][:keep] - R.inverse(spec, g)[0, :keep]).max() <= 1e-12 and (st['audio'][keep:] == 0).all()
    if group != 'gapped':                                   # the Hann window at hop = filter_length / 4 rebuilds the samples
        assert np.abs(st['audio'][g.fl:keep - g.fl] - x[g.fl:keep - g.fl]).max() <= 1e-5       # the tables are float32


@pytest.mark.parametrize('f', FREQS)
def test_amplitude_and_frequency_survive_every_rate(f):
    for r in CHECK_RATES:
        y = V.time_stretch(two_tones(f), G, r)
        assert len(y) == int(np.rint(SR / r))
        inner = y[EDGE:-EDGE]
        rms, hz = V.rms(inner), V.dominant_hz(inner)
        print(f'f {f} rate {r}: rms {rms:.4f} ({abs(rms / RMS_WANT - 1):.2%}), peak {hz:.3f} Hz')
        assert abs(rms / RMS_WANT - 1) <= RMS_TOL and abs(hz - f) <= HZ_TOL


@pytest.mark.parametrize('f', FREQS)
def test_the_unlocked_vocoder_loses_the_amplitude(f):
    """The textbook phase vocoder (every bin accumulates its own phase) misses the RMS bound by more than 30 % when it slows
    down: the check above tells the algorithm asked for from the one that is easier to write."""
    for r in (0.25, 0.5, 0.8):
        rms = V.rms(V.time_stretch(two_tones(f), G, r, lock=False)[EDGE:-EDGE])
        print(f'f {f} rate {r}: unlocked rms {rms:.4f}')
        assert abs(rms / RMS_WANT - 1) > 0.30
    # ... and is the same vocoder where no peak owns another bin's phase: identical at rate 1
    assert np.array_equal(V.time_stretch(two_tones(f), G, 1.0, lock=False), V.time_stretch(two_tones(f), G, 1.0, plant='no_locking'))


@pytest.mark.parametrize('n_steps', [-12, -3, 2, 7, 12])
def test_pitch_shift_moves_the_peak(n_steps):
    y = V.pitch_shift(two_tones(220.3), G, n_steps)
    assert len(y) == SR
    hz, want = V.dominant_hz(y[EDGE:-EDGE]), 220.3 * 2 ** (n_steps / 12)
    print(f'{n_steps:+d} steps: {hz:.3f} Hz, want {want:.3f}')
    assert abs(hz - want) <= HZ_TOL


def test_frame_and_sample_counts():
    for F, r in itertools.product((1, 2, 3, 44, 87, 801), C.RATES + (1.0 / 3, 3.999)):
        T = V.out_frames(F, r)
        assert T * r >= F and (T - 1) * r < F and T >= 1
        i, a = V.positions(F, r)
        assert len(i) == T and i.max() <= F - 1 and (a >= 0).all() and (a < 1).all()
    assert [V.out_samples(n, 2.0) for n in (1, 3, 5, 9)] == [0, 2, 2, 4]                # ties to even
    assert V.out_samples(1, 4.0) == 0 and V.out_samples(22050, 1.37) == 16095


# ---- owners, by enumeration --------------------------------------------------------------------------------------------
def brute_owners(m):
    cut = len(m)
    at = lambda k: m[k] if 0 <= k < cut else -np.inf
    pk = [k for k in range(cut) if m[k] > 0 and m[k] > at(k - 1) and m[k] > at(k - 2) and m[k] >= at(k + 1) and m[k] >= at(k + 2)]
    if not pk:
        return [-1] * cut
    return [min(pk, key=lambda p: (abs(p - k), p)) for k in range(cut)]


def test_owner_edge_cases():
    own = lambda m: V.owners_of(np.asarray(m, np.float64)).tolist()
    assert own([5, 1, 1, 1, 1, 1, 1, 9]) == [0, 0, 0, 0, 7, 7, 7, 7]                    # peaks at bin 0 and at bin cut - 1
    assert own([1, 2, 3, 9, 3, 2, 1]) == [3] * 7                                        # a single peak
    assert own([1, 4, 4, 4, 1, 1]) == [1] * 6                                           # a plateau: its first bin
    assert own([0, 9, 0, 0, 0, 9, 0]) == [1, 1, 1, 1, 5, 5, 5]                          # the midway tie goes down
    assert V.owners_of(np.asarray([0, 9, 0, 0, 0, 9, 0.]), plant='tie_up').tolist() == [1, 1, 1, 5, 5, 5, 5]
    assert own([0, 0, 0, 0]) == [-1] * 4 and own([0, 0, 3, 0]) == [2] * 4
    assert own([3, 3, 3, 3]) == [0] * 4 and own([1, 2, 3, 4]) == [3] * 4 and own([4, 3, 2, 1]) == [0] * 4
    assert own([2, 1, 2]) == [0, 0, 0]                                                  # m[2] is not above m[0]
    # a frame of zeros between live frames has no owners and the next frame its own
    m = np.array([[1, 5, 1, 1, 6, 1], [0] * 6, [1, 1, 7, 1, 1, 1]], np.float64)
    assert V.owners(m).tolist() == [[1, 1, 1, 4, 4, 4], [-1] * 6, [2] * 6]
    for cut, levels in ((1, 3), (2, 3), (5, 3), (7, 2)):                                # every frame of a few levels
        for m in itertools.product(range(levels), repeat=cut):
            assert V.owners_of(np.asarray(m, np.float64)).tolist() == brute_owners(m), m
    rng = np.random.default_rng(5)
    for _ in range(200):
        m = rng.integers(0, 4, int(rng.integers(1, 40))).astype(np.float64)
        assert V.owners_of(m).tolist() == brute_owners(m.tolist())


def test_a_silent_frame_carries_the_phase_on():
    """In a frame without peaks U advances by A alone and nothing comes out; the frame behind it is locked again."""
    g = C.GEOMS['small']
    st = V.stages(C.signal('gaps', 701, g, seed=701), g, 0.8)
    silent = (st['owner'] < 0).all(axis=1)
    assert silent.any() and not silent.all() and (st['operand'][silent] == 0).all()
    after = np.flatnonzero(silent[:-1] & ~silent[1:]) + 1
    assert len(after) and (np.abs(st['operand'][after]).max(axis=1) > 0).all()
    assert (V.time_stretch(np.zeros(701), g, 0.5) == 0).all() and (V.time_stretch(np.zeros(701), g, 0.5, dtype=np.float32) == 0).all()


def test_short_rows():
    """F = 2 and 3 with T = 1 and 2: one output frame overlap-adds to no sample under an even filter_length."""
    g = C.GEOMS['coarse']
    for name in C.NAMES:
        case = C.BY_NAME[name]
        if case.group != 'coarse':
            continue
        st = V.stages(C.audio_of(name), g, case.rate)
        F, T = g.frames(case.n), st['magnitude'].shape[0]
        assert (F, T) in ((2, 1), (2, 2), (3, 1), (3, 2)) and len(st['audio']) == V.out_samples(case.n, case.rate)
        assert (T == 1) == (not st['audio'].any())
    assert {(g.frames(c.n), V.out_frames(g.frames(c.n), c.rate)) for c in C.CASES if c.group == 'coarse'} == {(2, 1), (2, 2), (3, 1), (3, 2)}


# ---- bounds ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float32_distances():
    worst = {}
    for name in C.NAMES:
        errs = C.stage_errors(name, C.numpy_runner(name))
        assert errs['owner'] == 0, name
        w = worst.setdefault(C.BY_NAME[name].group, {})
        for s, e in errs.items():
            w[s] = max(w.get(s, 0.0), e)
    return worst


def test_bounds_lie_above_float32():
    worst = float32_distances()
    print('float32 numpy distances', {g: {s: f'{e:.3e}' for s, e in w.items()} for g, w in worst.items()})
    assert set(worst) == set(C.BOUNDS) == set(C.GEOMS)
    for group, w in worst.items():
        for s in ('spectrum', 'magnitude', 'operand', 'frames', 'audio'):
            # MARGIN times the distance, rounded up to two digits
            assert C.BOUNDS[group][s] / (1.25 * C.MARGIN) <= w[s] <= C.BOUNDS[group][s] / C.MARGIN, (group, s, w[s], C.BOUNDS[group][s])


def test_zero_rows_come_out_exactly_zero():
    for name in C.NAMES:
        if C.BY_NAME[name].signal == 'zeros':
            runner = C.numpy_runner(name)
            assert all(not np.asarray(runner(s), np.float64).any() for s in ('magnitude', 'operand', 'frames', 'audio'))
            assert (runner('owner') == -1).all()


@pytest.mark.parametrize('plant', V.MISTAKES)
def test_bounds_lie_below_planted_mistakes(plant):
    """A mistake (float64 run with the mistake, judged like a GPU run) moves the stage it first shows in by at least ten times
    that stage's bound on the case it shows best in; a wrong owner is a bin that differs, which the GPU tests hold to none."""
    stage = C.MISTAKE_STAGE[plant]
    effects = []
    for name in C.NAMES:
        case = C.BY_NAME[name]
        if case.signal == 'zeros' or case.group == 'wide':
            continue
        e = C.stage_errors(name, C.numpy_runner(name, np.float64, plant))[stage]
        effects.append((e / (1 if stage == 'owner' else C.BOUNDS[case.group][stage]), e, name))
    best = max(effects)
    print(plant, stage, 'best-showing case', best[1:], 'in bounds', f'{best[0]:.3g}')
    if stage == 'owner':
        assert best[1] >= 1
    else:
        assert best[0] >= 10 and best[1] >= 0.5


# ---- the front end, as a stand-alone program under ASan / UBSan ----------------------------------------------------------
def _run(exe, lengths=(), **settings):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    args = [exe, '--time-stretch'] + [f'{k}={v}' for k, v in settings.items()] + [str(int(n)) for n in lengths]
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    status, _, message = lines[0].partition(' ')
    return int(status), message, [[int(x) for x in line.split()] for line in lines[1:]]


def _plan(g):
    return dict(filter_length=g.fl, hop_length=g.hop, win_length=g.wl)


def _rates(rates):
    return ','.join(repr(float(r)) for r in rates)


def geometry(g, N, lengths, rates):
    """What time_stretch_check derives: the frame slots, M, the vocoder's buffers behind the inverse's workspace, and per row
    F_b, T_b, S_b and the samples kept from the inverse."""
    B, cut = len(lengths), g.cut
    NB = ceil_div(2 * cut, 32) * 32
    F = [g.frames(L) for L in lengths]
    T = [V.out_frames(f, r) for f, r in zip(F, rates)]
    S = [V.out_samples(L, r) for L, r in zip(lengths, rates)]
    rows, cells = B * max(T), B * max(T) * cut
    inverse = [4 * B, rows * NB * 4, rows * g.fl * 4]
    extra = [12 * B, cells * 4, cells * 4, cells * 8, cells * 8]
    offsets = [carved(*inverse, *extra[:i]) for i in range(6)]
    return [[g.frames(N), max(T), max(S)], offsets, F, T, S, [max(0, min(s, g.samples(t))) for s, t in zip(S, T)]]


@pytest.mark.parametrize('group', sorted(C.GEOMS))
def test_geometry(checker, group):
    g = C.GEOMS[group]
    rng = np.random.default_rng(g.fl + g.hop)
    for _ in range(6):
        N = int(rng.integers(g.half + 1, 12 * g.fl))
        B = int(rng.integers(1, 6))
        lengths = [int(v) for v in rng.integers(max(1, g.half + 1 if g.wl <= g.half else 1), N + 1, B)]
        lengths[0] = N
        rates = [float(r) for r in rng.choice(C.RATES + (1 / 3, 2.5), B)]
        want = geometry(g, N, lengths, rates)
        rc, msg, rows = _run(checker, lengths, N=N, M=want[0][2], rates=_rates(rates), **_plan(g))
        assert rc == 0 and rows == want, (msg, N, lengths, rates)
    # lengths NULL, one rate for every row, the probe's stages
    want = geometry(g, 3 * g.fl, [3 * g.fl] * 3, [0.8] * 3)
    for what in (-1, 0, 4):
        assert _run(checker, B=3, N=3 * g.fl, M=want[0][2], rates='0.8', what=what, **_plan(g)) == (0, '', want)


def test_helpers_at_the_limits(checker):
    g = C.GEOMS['small']
    lengths = [1, 3, 9, 64, 65, 701, 22050, 5, 5, 5, 5, 5, 5]
    rates = [4.0, 2.0, 2.0, 0.25, 4.0, 1.37, 1 / 3, 0.25, 4.0, 0.2499999, 4.0000001, float('nan'), float('inf')]
    rc, _, rows = _run(checker, lengths, helpers=1, rates=_rates(rates), **_plan(g))
    want = [[V.out_frames(g.frames(n), r), V.out_samples(n, r)] if V.RATE_MIN <= r <= V.RATE_MAX else [-1, -1] for n, r in zip(lengths, rates)]
    assert rc == 0 and rows == want and rows[0] == [2, 0] and rows[1][1] == 2 and rows[2][1] == 4
    # a row the reflect cannot pad, no samples, a Whisper plan, pre-emphasis
    short = R.Geom(16, 4, 4)
    assert _run(checker, [3, 0, 9], helpers=1, rates='1.0', **_plan(short))[2] == [[-1, -1], [-1, -1], [short.frames(9), 9]]
    assert _run(checker, [64], helpers=1, rates='1.0', mel_kind=1, **_plan(g))[2] == [[-1, -1]]
    assert _run(checker, [64], helpers=1, rates='1.0', pre_emph=0.97, **_plan(g))[2] == [[-1, -1]]


SHORT = R.Geom(16, 4, 4)
OK = dict(N=40, M=40, rates='1.0,2.0', **_plan(SHORT))
OK_LENGTHS = (40, 9)
# every refusal in the documented order: (name, change of the lengths, change of the settings, substrings of the message)
FAULTS = [
    ('null', None, dict(null='audio'), ['bad argument']),
    ('lengths', {0: 0}, {}, ['lengths[0] = 0 outside [1, N = ']),
    ('reflect', {1: 3}, {}, ['row 1: max(L = 3, win_length = 4) samples are not more than filter_length // 2 = 8']),
    ('whisper', None, dict(mel_kind=1), ['refused for a Whisper plan']),
    ('pre_emph', None, dict(pre_emph=0.5), ['pre_emph = 0.5 > 0 cannot be inverted']),
    ('rate', None, dict(rates='1.0,4.5'), ['rates[1] = 4.5 must be finite and lie in [0.25, 4]']),
    ('M', None, dict(M=39), ['M = 39, but max_b llrint(lengths[b] / rates[b]) = 40']),
    ('size', None, dict(N=600000000), ['too large for 31-bit offsets (B <= 65535)']),
    ('mem', None, dict(mem=2), ['bad mem kind 2']),
    ('what', None, dict(what=5), ['no stage 5 (0 .. 4)']),
]


def _faulty(names):
    lengths, settings = list(OK_LENGTHS), dict(OK)
    for name, at, change, _ in FAULTS:
        if name in names:
            for i, v in (at or {}).items():
                lengths[i] = v
            settings.update(change)
    return lengths, settings


def test_the_call_as_it_stands_is_accepted(checker):
    rc, msg, rows = _run(checker, OK_LENGTHS, **OK)
    assert rc == 0 and rows == geometry(SHORT, 40, OK_LENGTHS, (1.0, 2.0)) and rows[4] == [40, 4], msg


@pytest.mark.parametrize('at', range(len(FAULTS)), ids=[f[0] for f in FAULTS])
def test_refusals_in_order(checker, at):
    """Each refusal alone, and with every refusal behind it in the order at the same time: the first match wins."""
    name, needles = FAULTS[at][0], FAULTS[at][3]
    for later in [()] + [(f[0],) for f in FAULTS[at + 1:]] + [tuple(f[0] for f in FAULTS[at + 1:])]:
        lengths, settings = _faulty((name, *later))
        rc, msg, rows = _run(checker, lengths, **settings)
        assert rc == -1 and rows == [] and msg.startswith('who: ') and all(n in msg for n in needles), (later, msg)


def test_more_refusals(checker):
    for settings, needle in ((dict(null='out'), 'bad argument'), (dict(null='fn'), 'bad argument'), (dict(null='rates'), 'bad argument'),
                             (dict(N=0), 'bad argument'), (dict(rates='nan,1'), 'rates[0] = nan'), (dict(rates='1,inf'), 'rates[1] = inf'),
                             (dict(rates='0.2,1'), 'rates[0] = 0.2'), (dict(rates='-1,1'), 'rates[0] = -1'), (dict(what=7), 'no stage 7')):
        rc, msg, _ = _run(checker, OK_LENGTHS, **dict(OK, **settings))
        assert rc == -1 and needle in msg, (settings, msg)
    assert 'bad argument' in _run(checker, B=0, **OK)[1]
    assert 'too large' in _run(checker, B=65536, N=40, M=40, rates='1.0', **_plan(C.GEOMS['small']))[1]
    # rows that stretch to nothing: one sample at rate 4 under a plan that pads it to win_length
    rc, msg, _ = _run(checker, [1, 1], N=1, M=0, rates='4.0', **_plan(C.GEOMS['small']))
    assert rc == -1 and 'every row stretches to 0 samples' in msg
    # the slower the rate, the more frame slots: 0.25 passes 2^31 where 1.0 does not
    big = dict(B=8, N=4100000, **_plan(G))
    assert _run(checker, M=4100000, rates='1.0', **big)[0] == 0
    assert 'too large' in _run(checker, M=16400000, rates='0.25', **big)[1]


# ---- speed and pitch_steps in the sentence pipeline: host logic on a recording stand-in --------------------------------
class _Engine:
    """An engine stand-in that records the calls of the finish stage and returns arrays of the right lengths."""
    device = 0

    def __init__(self):
        self.calls = []

    def mel_fn(self, cfg, window=None):
        self.calls.append(('mel_fn', cfg['filter_length'], cfg['hop_length'], cfg['win_length']))
        return 'plan'

    def time_stretch(self, plan, audio, rate, lengths=None, stream=None):
        self.calls.append(('time_stretch', plan, audio.shape, rate, None if lengths is None else list(lengths)))
        M = V.out_samples(audio.shape[-1], rate)
        return np.full(audio.shape[:-1] + (M,), 2, np.float32), np.asarray([M], np.int32)

    def resample(self, audio, rate, target_rate, lengths=None, stream=None):
        self.calls.append(('resample', audio.shape, rate, target_rate, None if lengths is None else list(lengths)))
        return np.full(audio.shape[:-1] + (int(audio.shape[-1] / rate * target_rate),), 3, np.float32)

    def reduce_noise(self, audio, rate):
        self.calls.append(('reduce_noise', audio.shape, rate))
        return audio

    def trim_silence(self, audio, rate):
        self.calls.append(('trim_silence', audio.shape, rate))
        return 10, len(audio) - 10


def _models(lengths):
    from test_host_logic import FakeSynth, FakeVocoder
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    synth, voc = FakeSynth(lengths), FakeVocoder()
    synth.engine = _Engine()
    return Tacotron2(synth), WaveGlow(voc), synth, voc


TEXT = 'Hello world, this is a test.'


def test_the_defaults_call_nothing():
    model, vocoder, synth, voc = _models([100, 100, 100])
    plain = model.infer(TEXT, vocoder=vocoder)
    same = model.infer(TEXT, vocoder=vocoder, speed=1.0, pitch_steps=0.0)
    ints = model.infer(TEXT, vocoder=vocoder, speed=1, pitch_steps=0)
    assert synth.engine.calls == [] and plain['time'] == same['time'] == ints['time']
    assert np.array_equal(plain['audio'], same['audio']) and np.array_equal(plain['audio'], ints['audio'])
    # neither keyword reaches a model or the cleaner
    assert all('speed' not in kw and 'pitch_steps' not in kw for _, kw in voc.calls)
    assert all('speed' not in kw and 'pitch_steps' not in kw for _, _, kw in synth.calls)


def test_speed_and_pitch_run_before_the_clean_up():
    from text_to_speech_amd.effects import pitch_ratio
    model, vocoder, synth, _ = _models([100])
    n = 100 * 256
    out = model.infer(TEXT, vocoder=vocoder, speed=1.25, pitch_steps=-2, reduce_noise=True, trim_silence=True)
    S = V.out_samples(n, 1.25)
    r, p, q = pitch_ratio(-2)
    S2 = V.out_samples(S, r)
    assert (p, q) == (1_000_000, round(2 ** (2 / 12) * 1_000_000)) and r == 2 ** (2 / 12)
    assert synth.engine.calls == [
        ('mel_fn', 1024, 256, 1024), ('time_stretch', 'plan', (n,), 1.25, None),
        ('mel_fn', 1024, 256, 1024), ('time_stretch', 'plan', (S,), r, None), ('resample', (S2,), p, q, [S2]),
        ('reduce_noise', (S,), 22050), ('trim_silence', (S,), 22050)]
    assert out['audio'].shape == (S - 20,) and out['time'] == (S - 20) / 22050
    # the pitch step keeps the duration: cut or zero-padded to what went in
    got = int(S2 / p * q)
    assert (out['audio'][:min(got, S) - 10] == 3).all() and (out['audio'][min(got, S) - 10:] == 0).all()


def test_time_is_the_new_duration():
    model, vocoder, synth, _ = _models([100, 100])
    n = 100 * 256
    slow = model.infer(TEXT, vocoder=vocoder, speed=0.5)
    assert slow['audio'].shape == (2 * n,) and slow['time'] == 2 * n / 22050 and (slow['audio'] == 2).all()
    high = model.infer(TEXT, vocoder=vocoder, pitch_steps=3.0)
    assert high['audio'].shape == (n,) and high['time'] == n / 22050
    assert [c[0] for c in synth.engine.calls] == ['mel_fn', 'time_stretch', 'mel_fn', 'time_stretch', 'resample']


def test_finish_keywords():
    from text_to_speech_amd.tacotron2 import Tacotron2, _stage_kwargs
    decode, vocode, finish = _stage_kwargs(dict(vocoder='v', speed=1.25, pitch_steps=-2, seed=3))
    assert finish == {'vocoder': 'v', 'speed': 1.25, 'pitch_steps': -2}
    assert 'speed' not in decode and 'pitch_steps' not in vocode and decode['seed'] == vocode['seed'] == 3
    assert 'map.json' in Tacotron2._finish.__doc__ and 'map.json' in Tacotron2.infer.__doc__
    model, vocoder, synth, _ = _models([100])
    synth.engine = None
    with pytest.raises(ValueError, match='speed / pitch_steps need a HIP engine'):
        model.infer(TEXT, vocoder=vocoder, speed=2.0)


def test_effects_compose_what_they_say():
    from text_to_speech_amd import effects
    eng = _Engine()
    x = np.zeros((2, 1000), np.float32)
    assert effects.pitch_shift(x, 0, engine=eng) is x and eng.calls == []
    out = effects.pitch_shift(x, 12, engine=eng, plan='mine', lengths=[1000, 600])
    assert out.shape == (2, 1000) and eng.calls[0] == ('time_stretch', 'mine', (2, 1000), 0.5, [1000, 600])
    assert eng.calls[1][:4] == ('resample', (2, 2000), 1_000_000, 500_000) and (out[1, 600:] == 0).all() and (out[0] == 3).all()
    assert effects.fix_length(np.ones((2, 5)), 3).shape == (2, 3) and effects.fix_length(np.ones(5), 8).tolist() == [1] * 5 + [0] * 3
    with pytest.raises(ValueError, match='n_steps must be finite'):
        effects.pitch_shift(x, float('nan'), engine=eng)
