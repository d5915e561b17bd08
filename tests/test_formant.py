"""CPU: the definitions behind formant-preserving pitch shifting (csrc/stft_inv.hip: tts_hip_formant_match) -- the liftering
table against the irfft / zero / rfft route, the float64 restatement (tests/formant_ref.py) on its own: identity, zeros, a
synthetic vowel shifted by -5, +4 and +7 steps whose formants come back while its pitch stays moved, a formant shift alone; the
bounds the GPU tests use (each above the float32 numpy copy's own distance from float64 and a factor ten below every planted
mistake); the host-only front end (csrc/audio_call.h: formant_match_check) through csrc/host_check.cpp's --formant-match mode,
built with -fsanitize=address,undefined as a stand-alone program; and `preserve_formants` / `formant_steps` through the sentence
pipeline on a recording stand-in engine."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import formant_cases as C
import formant_ref as Fm
import stft_inv_ref as R
import time_stretch_ref as V
from test_audio_call import carved, ceil_div, checker      # noqa: F401  (checker: the fixture)

G = C.GEOMS['default']
BIN_HZ = Fm.SR / G.fl
F2_HZ, F2_BINS, F1_BINS, F2_PLAIN_HZ, F0_TOL, RMS_TOL = 2600.0, 3, 2, 400.0, 1.0, 0.02


# ---- the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fl,Q', [(16, 1), (16, 7), (64, 5), (64, 31), (1024, 33), (1024, 511), (30, 4)])
def test_table_is_the_cepstral_route(fl, Q):
    L = Fm.lifter_table64(fl, Q)
    err = np.abs(L - Fm.lifter_table_fft(fl, Q)).max()
    print(f'fl {fl} Q {Q}: table against irfft / zero / rfft {err:.2e}')
    assert err <= 1e-13
    const = np.full(fl // 2 + 1, -3.25)
    assert np.abs(const @ L - const).max() <= 1e-12                 # a flat spectrum is its own envelope


@pytest.mark.parametrize('fl,Q', [(64, 5), (1024, 33)])
def test_quefrencies_up_to_Q_pass_and_the_others_go(fl, Q):
    k = np.arange(fl // 2 + 1)
    L = Fm.lifter_table64(fl, Q)
    for q in (0, 1, Q - 1, Q):
        row = np.cos(2 * np.pi * q * k / fl)
        assert np.abs(row @ L - row).max() <= 1e-12, q
    for q in (Q + 1, Q + 2, fl // 2 - 1, fl // 2):
        row = np.cos(2 * np.pi * q * k / fl)
        assert np.abs(row @ L).max() <= 1e-12, q
    mixed = 0.7 * np.cos(2 * np.pi * 2 * k / fl) - 1.5 * np.cos(2 * np.pi * (Q + 3) * k / fl) + 0.25
    assert np.abs(mixed @ L - (0.7 * np.cos(2 * np.pi * 2 * k / fl) + 0.25)).max() <= 1e-12


def test_default_lifter():
    assert Fm.default_lifter(1024) == 33 and Fm.default_lifter(64) == 31 and Fm.default_lifter(1024, 16000) == 24
    assert Fm.default_lifter(1024, 100) == 1 and Fm.default_lifter(4, 22050) == 1


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', sorted(C.GEOMS))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_source_equal_to_audio_is_the_stft_round_trip(group, dtype):
    g = C.GEOMS[group]
    x = C.TC.signal('noisy', C.max_len(g), g, seed=2)
    for source in (None, x):
        st = Fm.stages(x, source, g, Fm.default_lifter(g.fl), dtype=dtype)
        assert (st['gain'] == 1).all() and st['gain'].dtype == dtype
        assert np.array_equal(st['operand'], st['spectrum'][1])
        keep = g.samples(g.frames(len(x)))
        want = R.inverse(st['spectrum'][1][None], g, dtype=dtype)[0]
        assert np.array_equal(st['audio'][:keep], want[:keep]) and (st['audio'][keep:] == 0).all()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_zeros_stay_zeros(dtype):
    g = C.GEOMS['small']
    z, x = np.zeros(295, np.float32), C.TC.signal('noisy', 295, g)
    st = Fm.stages(z, None, g, 31, dtype=dtype)
    assert (st['gain'] == 1).all() and not st['operand'].any() and not st['audio'].any()
    st = Fm.stages(z, x, g, 31, warp=0.8, dtype=dtype)              # a live source: finite gains on nothing
    assert np.isfinite(st['gain']).all() and (st['gain'] > 0).all() and not st['operand'].any() and not st['audio'].any()


def test_the_clamp_is_met_from_both_sides():
    for name, sign in (('default_louder', 1), ('default_quieter', -1)):
        case = C.BY_NAME[name]
        S = C.numpy_runner(name, np.float64)('envelope')
        E = S[0, 0] - S[1, 0]
        assert (sign * E > Fm.clamp_of(case.max_gain_db)).mean() > 0.25, name       # a quarter of the bins and more
    case = C.BY_NAME['default_mixed_clamp']
    S = C.numpy_runner(case.name, np.float64)('envelope')
    E, Gc = Fm.warped(S[0, 0], case.warps[0]) - S[1, 0], Fm.clamp_of(case.max_gain_db)
    assert (E > Gc).any() and (E < -Gc).any() and (np.abs(E) < Gc).any()


def vowel_report(shifted, corrected, steps, label=''):
    """The vowel criteria on a shifted and a corrected signal; prints the measured values and returns them."""
    x = Fm.vowel()
    src2, plain2, got2 = (Fm.nearest_peak(s, G, F2_HZ) for s in (x, shifted, corrected))
    src1, got1 = Fm.lowest_peak(x, G), Fm.lowest_peak(corrected, G)
    f0, want_f0 = Fm.autocorr_f0(corrected), Fm.F0 * 2 ** (steps / 12)
    rms = Fm.inner_rms(corrected) / Fm.inner_rms(shifted)
    print(f'{label}{steps:+d} steps: upper peak source {src2 * BIN_HZ:.0f} Hz, shifted {plain2 * BIN_HZ:.0f} Hz, corrected '
          f'{got2 * BIN_HZ:.0f} Hz; lowest peak source {src1 * BIN_HZ:.0f} Hz, corrected {got1 * BIN_HZ:.0f} Hz; F0 {f0:.2f} Hz '
          f'(want {want_f0:.2f}); inner rms ratio {rms:.4f}')
    return dict(src2=src2, plain2=plain2, got2=got2, src1=src1, got1=got1, f0=f0, want_f0=want_f0, rms=rms)


def vowel_check(m):
    assert abs(m['got2'] - m['src2']) <= F2_BINS and abs(m['plain2'] - m['src2']) * BIN_HZ > F2_PLAIN_HZ
    assert abs(m['got1'] - m['src1']) <= F1_BINS
    assert abs(m['f0'] - m['want_f0']) <= F0_TOL
    assert abs(m['rms'] - 1) <= RMS_TOL


@functools.lru_cache(maxsize=None)
def shifted_vowel(steps):
    y = V.pitch_shift(Fm.vowel(), G, steps)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize('steps', Fm.VOWEL_STEPS)
def test_the_vowel_keeps_its_formants(steps):
    y = shifted_vowel(steps)
    vowel_check(vowel_report(y, Fm.formant_match(y, Fm.vowel(), G), steps))


def test_without_the_energy_scaling_the_level_drifts():
    """The bias step 6 removes: at +7 steps the unscaled gain doubles the level."""
    y = shifted_vowel(7)
    ratio = Fm.inner_rms(Fm.formant_match(y, Fm.vowel(), G, plant='no_energy')) / Fm.inner_rms(y)
    print(f'+7 steps without the energy scaling: inner rms ratio {ratio:.3f}')
    assert ratio > 1.5


def test_formant_shift_alone_moves_the_peaks():
    x = Fm.vowel()
    up = 2 ** (3 / 12)
    z = Fm.formant_match(x, None, G, warp=up)
    k1, k2 = Fm.lowest_peak(x, G), Fm.nearest_peak(x, G, F2_HZ)
    got1, got2, f0 = Fm.lowest_peak(z, G), Fm.nearest_peak(z, G, F2_HZ * up), Fm.autocorr_f0(z)
    print(f'+3 formant steps: peaks {got1 * BIN_HZ:.0f} / {got2 * BIN_HZ:.0f} Hz (want {k1 * up * BIN_HZ:.0f} / {k2 * up * BIN_HZ:.0f}), F0 {f0:.2f} Hz')
    assert abs(got1 - k1 * up) <= 3 and abs(got2 - k2 * up) <= 3 and abs(f0 - Fm.F0) <= F0_TOL


# ---- bounds ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float32_distances():
    worst = {}
    for name in C.NAMES:
        w = worst.setdefault(C.BY_NAME[name].group, {})
        for s, e in C.stage_errors(name, C.numpy_runner(name)).items():
            w[s] = max(w.get(s, 0.0), e)
    return worst


def test_cases_cover_what_they_say():
    for group, g in C.GEOMS.items():
        mine = [c for c in C.CASES if c.group == group]
        assert all(max(c.lengths) <= C.max_len(g) and c.N <= C.max_len(g) for c in mine)
        assert {c.Q for c in mine} >= {1, g.fl // 2 - 1, Fm.default_lifter(g.fl)}
        assert {w for c in mine for w in c.warps} >= set(C.WARPS)
        assert any(min(c.lengths) < g.wl for c in mine) and any(c.scale == 1000.0 for c in mine) and any(c.scale == 0.001 for c in mine)
        assert {(c.audio, c.source) for c in mine} >= set(C.UNLIKE) and any(c.source is None for c in mine)
    rows = {c.B * c.geom.frames(c.N) for c in C.CASES if '_rows_' in c.name}
    assert rows == {63, 64, 65, 32, 33}


def test_bounds_lie_above_float32():
    worst = float32_distances()
    print('float32 numpy distances', {g: {s: f'{e:.3e}' for s, e in w.items()} for g, w in worst.items()})
    assert set(worst) == set(C.BOUNDS) == set(C.GEOMS)
    for group, w in worst.items():
        for s in C.STAGES:
            # MARGIN times the distance, rounded up to two digits
            assert C.BOUNDS[group][s] / (1.25 * C.MARGIN) <= w[s] <= C.BOUNDS[group][s] / C.MARGIN, (group, s, w[s], C.BOUNDS[group][s])


@pytest.mark.parametrize('plant', Fm.MISTAKES)
def test_bounds_lie_below_planted_mistakes(plant):
    """A mistake (float64 run with the mistake, judged like a GPU run) moves the stage it first shows in by at least ten times
    that stage's bound on the case it shows best in."""
    stage = C.MISTAKE_STAGE[plant]
    effects = []
    with np.errstate(invalid='ignore'):
        for name in C.NAMES:
            e = C.stage_errors(name, C.numpy_runner(name, np.float64, plant))[stage]
            effects.append((e / C.BOUNDS[C.BY_NAME[name].group][stage], e, name))
    best = max(effects)
    print(plant, stage, 'best-showing case', best[1:], 'in bounds', f'{best[0]:.3g}')
    assert best[0] >= 10


# ---- the front end, as a stand-alone program under ASan / UBSan ----------------------------------------------------------
def _run(exe, lengths=(), **settings):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    args = [exe, '--formant-match'] + [f'{k}={v}' for k, v in settings.items()] + [str(int(n)) for n in lengths]
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f'sanitizer report or crash (exit {r.returncode}):\n{r.stderr[-4000:]}'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    status, _, message = lines[0].partition(' ')
    return int(status), message, lines[1:]


def _ints(lines):
    return [[int(x) for x in line.split()] for line in lines]


def _plan(g):
    return dict(filter_length=g.fl, hop_length=g.hop, win_length=g.wl)


def geometry(g, N, lengths, Q, max_gain_db=24.0, what=-1):
    """What formant_match_check derives: the frame slots, Q and the bits of G, the call's buffers behind the inverse's
    workspace, and per row F_b and the samples kept from the inverse."""
    B, cut = len(lengths), g.cut
    NB, CK = ceil_div(2 * cut, 32) * 32, ceil_div(cut, 32) * 32
    Fr = g.frames(N)
    rows = B * Fr
    inverse = [4 * B, rows * NB * 4, rows * g.fl * 4]
    extra = [8 * B, 2 * rows * CK * 4, 2 * rows * cut * 4, rows * cut * 4 if what == 2 else 0]
    offsets = [carved(*inverse, *extra[:i]) for i in range(5)]
    F = [g.frames(L) for L in lengths]
    gbits = struct.unpack('<I', struct.pack('<f', max_gain_db * np.log(10.0) / 20.0))[0]
    return [[Fr, Q, gbits], offsets, F, [max(0, min(L, g.samples(f))) for L, f in zip(lengths, F)]]


@pytest.mark.parametrize('group', sorted(C.GEOMS))
def test_geometry(checker, group):
    g = C.GEOMS[group]
    rng = np.random.default_rng(g.fl + g.hop)
    for _ in range(6):
        N = int(rng.integers(g.half + 1, 12 * g.fl))
        B = int(rng.integers(1, 6))
        lengths = [int(v) for v in rng.integers(max(1, g.half + 1 if g.wl <= g.half else 1), N + 1, B)]
        lengths[0] = N
        Q, db = int(rng.integers(1, g.fl // 2)), float(rng.choice([0.5, 6.0, 24.0, 60.0]))
        what = int(rng.integers(-1, 5))
        warps = ','.join(repr(float(w)) for w in rng.choice(C.WARPS, B))
        rc, msg, rows = _run(checker, lengths, N=N, Q=Q, max_gain_db=db, what=what, warps=warps, **_plan(g))
        assert rc == 0 and _ints(rows) == geometry(g, N, lengths, Q, db, what), (msg, N, lengths, Q, db, what)
    # lengths NULL, warps NULL, one warp for every row
    want = geometry(g, 3 * g.fl, [3 * g.fl] * 3, 7)
    assert _ints(_run(checker, B=3, N=3 * g.fl, Q=7, **_plan(g))[2]) == want
    assert _ints(_run(checker, B=3, N=3 * g.fl, Q=7, warps='0.5', **_plan(g))[2]) == want


@pytest.mark.parametrize('fl,Q', [(16, 3), (64, 31), (1024, 33)])
def test_the_table_of_the_library(checker, fl, Q):
    rc, _, lines = _run(checker, table=1, Q=Q, filter_length=fl, hop_length=fl // 4, win_length=fl)
    got = np.array([float(v) for v in lines]).reshape(fl // 2 + 1, fl // 2 + 1)
    assert rc == 0 and np.abs(got - Fm.lifter_table64(fl, Q)).max() <= 1e-15


SHORT = R.Geom(16, 4, 4)
OK = dict(N=40, Q=3, max_gain_db=24.0, warps='1.0,2.0', **_plan(SHORT))
OK_LENGTHS = (40, 9)
# every refusal in the documented order: (name, change of the lengths, change of the settings, substrings of the message)
FAULTS = [
    ('null', None, dict(null='audio'), ['bad argument']),
    ('lengths', {0: 0}, {}, ['lengths[0] = 0 outside [1, N = ']),
    ('reflect', {1: 3}, {}, ['row 1: max(L = 3, win_length = 4) samples are not more than filter_length // 2 = 8']),
    ('whisper', None, dict(mel_kind=1), ['refused for a Whisper plan']),
    ('pre_emph', None, dict(pre_emph=0.5), ['pre_emph = 0.5 > 0 cannot be inverted']),
    ('warp', None, dict(warps='1.0,2.5'), ['warps[1] = 2.5 must be finite and lie in [0.5, 2]']),
    ('Q', None, dict(Q=8), ['lifter Q = 8 outside [1, filter_length / 2 - 1 = 7]']),
    ('gain', None, dict(max_gain_db=61), ['max_gain_db = 61 must be finite and lie in (0, 60]']),
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
    assert rc == 0 and _ints(rows) == geometry(SHORT, 40, OK_LENGTHS, 3), msg


@pytest.mark.parametrize('at', range(len(FAULTS)), ids=[f[0] for f in FAULTS])
def test_refusals_in_order(checker, at):
    """Each refusal alone, and with every refusal behind it in the order at the same time: the first match wins."""
    name, needles = FAULTS[at][0], FAULTS[at][3]
    for later in [()] + [(f[0],) for f in FAULTS[at + 1:]] + [tuple(f[0] for f in FAULTS[at + 1:])]:
        lengths, settings = _faulty((name, *later))
        rc, msg, rows = _run(checker, lengths, **settings)
        assert rc == -1 and rows == [] and msg.startswith('who: ') and all(n in msg for n in needles), (later, msg)


def test_more_refusals(checker):
    for settings, needle in ((dict(null='out'), 'bad argument'), (dict(null='fn'), 'bad argument'), (dict(N=0), 'bad argument'),
                             (dict(warps='nan,1'), 'warps[0] = nan'), (dict(warps='1,inf'), 'warps[1] = inf'),
                             (dict(warps='0.49,1'), 'warps[0] = 0.49'), (dict(warps='-1,1'), 'warps[0] = -1'), (dict(Q=0), 'lifter Q = 0'),
                             (dict(Q=-3), 'lifter Q = -3'), (dict(max_gain_db=0), 'max_gain_db = 0'), (dict(max_gain_db='nan'), 'max_gain_db = nan'),
                             (dict(max_gain_db=-6), 'max_gain_db = -6'), (dict(max_gain_db='inf'), 'max_gain_db = inf'), (dict(what=7), 'no stage 7')):
        rc, msg, _ = _run(checker, OK_LENGTHS, **dict(OK, **settings))
        assert rc == -1 and needle in msg, (settings, msg)
    for settings in (dict(warps='0.5,2'), dict(Q=7), dict(Q=1), dict(max_gain_db=60), dict(max_gain_db=1e-3), dict(what=4), dict(what=0)):
        assert _run(checker, OK_LENGTHS, **dict(OK, **settings))[0] == 0, settings
    assert 'bad argument' in _run(checker, B=0, **OK)[1]
    assert 'too large' in _run(checker, B=65536, N=40, Q=3, **_plan(C.GEOMS['small']))[1]
    # the stacked 2 * B * F rows are the largest buffer but for the time frames: rows that the denoiser's limit admits
    big = dict(B=8, N=4100000, Q=33, **_plan(G))
    assert _run(checker, **big)[0] == 0
    assert 'too large' in _run(checker, **dict(big, N=16800000))[1]


# ---- preserve_formants and formant_steps in the sentence pipeline: host logic on a recording stand-in ------------------
from test_time_stretch import TEXT, _Engine as _PlainEngine, _models as _plain_models      # noqa: E402


class _Engine(_PlainEngine):
    def formant_match(self, plan, audio, source=None, *, warp=1.0, lifter=None, max_gain_db=24.0, lengths=None, stream=None):
        self.calls.append(('formant_match', plan, audio.shape, None if source is None else source.shape, warp, lifter, max_gain_db,
                           None if lengths is None else list(lengths)))
        return np.full((1,) * (2 - audio.ndim) + audio.shape, 5, np.float32)


def _models(lengths):
    model, vocoder, synth, voc = _plain_models(lengths)
    synth.engine = _Engine()
    return model, vocoder, synth, voc


def test_the_defaults_call_nothing():
    model, vocoder, synth, voc = _models([100] * 4)                          # one accepted trial per call
    plain = model.infer(TEXT, vocoder=vocoder)
    same = model.infer(TEXT, vocoder=vocoder, preserve_formants=False, formant_steps=0.0)
    alone = model.infer(TEXT, vocoder=vocoder, preserve_formants=True)       # nothing to preserve without a pitch change
    assert synth.engine.calls == [] and np.array_equal(plain['audio'], same['audio']) and np.array_equal(plain['audio'], alone['audio'])
    assert all('preserve_formants' not in kw and 'formant_steps' not in kw for _, kw in voc.calls)
    assert all('preserve_formants' not in kw and 'formant_steps' not in kw for _, _, kw in synth.calls)
    shifted = model.infer(TEXT, vocoder=vocoder, pitch_steps=3.0)
    assert [c[0] for c in synth.engine.calls] == ['mel_fn', 'time_stretch', 'resample'] and (shifted['audio'] == 3).all()


def test_which_calls_with_which_warp_in_which_order():
    model, vocoder, synth, _ = _models([100] * 3)                            # one accepted trial per call
    n = 100 * 256
    out = model.infer(TEXT, vocoder=vocoder, pitch_steps=4, preserve_formants=True, reduce_noise=True)
    r = 2 ** (-4 / 12)
    S = V.out_samples(n, r)
    assert synth.engine.calls == [
        ('mel_fn', 1024, 256, 1024), ('time_stretch', 'plan', (n,), r, None), ('resample', (S,), 1_000_000, round(r * 1_000_000), [S]),
        ('mel_fn', 1024, 256, 1024), ('formant_match', 'plan', (n,), (n,), 1.0, None, 24.0, None), ('reduce_noise', (n,), 22050)]
    assert out['audio'].shape == (n,) and (out['audio'] == 5).all() and out['time'] == n / 22050
    del synth.engine.calls[:]
    model.infer(TEXT, vocoder=vocoder, pitch_steps=-5, formant_steps=2)      # formant_steps implies the matching
    assert [c[0] for c in synth.engine.calls] == ['mel_fn', 'time_stretch', 'resample', 'mel_fn', 'formant_match']
    assert synth.engine.calls[-1][3:5] == ((n,), 2 ** (2 / 12))
    del synth.engine.calls[:]
    out = model.infer(TEXT, vocoder=vocoder, formant_steps=-2, speed=2.0)    # after the tempo, no pitch change: against itself
    assert synth.engine.calls == [('mel_fn', 1024, 256, 1024), ('time_stretch', 'plan', (n,), 2.0, None),
                                  ('mel_fn', 1024, 256, 1024), ('formant_match', 'plan', (n // 2,), None, 2 ** (-2 / 12), None, 24.0, None)]
    assert out['audio'].shape == (n // 2,) and (out['audio'] == 5).all()


def test_finish_keywords():
    from text_to_speech_amd.tacotron2 import Tacotron2, _stage_kwargs
    decode, vocode, finish = _stage_kwargs(dict(vocoder='v', pitch_steps=4, preserve_formants=True, formant_steps=-2, seed=3))
    assert finish == {'vocoder': 'v', 'pitch_steps': 4, 'preserve_formants': True, 'formant_steps': -2}
    assert 'preserve_formants' not in decode and 'formant_steps' not in vocode and decode['seed'] == vocode['seed'] == 3
    for doc in (Tacotron2._finish.__doc__, Tacotron2.infer.__doc__):
        assert 'map.json' in doc and 'preserve_formants' in doc and 'formant_steps' in doc
    model, vocoder, synth, _ = _models([100])
    synth.engine = None
    with pytest.raises(ValueError, match='need a HIP engine'):
        model.infer(TEXT, vocoder=vocoder, formant_steps=2.0)


def test_effects_compose_what_they_say():
    from text_to_speech_amd import effects
    eng = _Engine()
    x = np.zeros((2, 1000), np.float32)
    assert effects.formant_shift(x, 0, engine=eng) is x and effects.pitch_shift(x, 0, engine=eng, preserve_formants=True) is x
    assert eng.calls == []
    out = effects.formant_shift(x, 12, engine=eng, plan='mine', lengths=[1000, 600], lifter=20, max_gain_db=12.0)
    assert out.shape == (2, 1000) and eng.calls == [('formant_match', 'mine', (2, 1000), None, 2.0, 20, 12.0, [1000, 600])]
    del eng.calls[:]
    out = effects.pitch_shift(x, 12, engine=eng, plan='mine', lengths=[1000, 600], preserve_formants=True)
    assert [c[0] for c in eng.calls] == ['time_stretch', 'resample', 'formant_match'] and out.shape == (2, 1000)
    assert eng.calls[2] == ('formant_match', 'mine', (2, 1000), (2, 1000), 1.0, None, 24.0, [1000, 600])
    row = effects.pitch_shift(x[0], 0, engine=eng, plan='mine', formant_steps=-12)
    assert row.shape == (1000,) and eng.calls[-1][3:5] == (None, 0.5)
    with pytest.raises(ValueError, match='must be finite'):
        effects.formant_shift(x, float('nan'), engine=eng)
    assert effects.formant_warp(3) == 2 ** (3 / 12) and effects.formant_warp(-6, 6) == 0.5
