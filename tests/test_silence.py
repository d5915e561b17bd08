"""CPU: the silence-removal fixture, the numpy restatement against what the reference returned, the conditions on the
test inputs, and the host side of remove_silence / audio.trim_silence / the facade (no GPU call).

The tests up to test_mean_window_equals_the_direct_convolution check tests/silence_ref.py and the fixture only: they
establish that the restatement and the inputs are fit to judge the GPU code by (tests/test_silence_gpu.py does that) and
say nothing about the package itself.  The tests below them run the package's host code."""
import hashlib
import json

import numpy as np
import pytest

import silence_ref as sr

R = 22050


@pytest.fixture(scope='module')
def fixture():
    return json.load(open(sr.FIXTURE))['cases']


def _sha(y):
    return hashlib.sha256(np.ascontiguousarray(y, np.float32).tobytes()).hexdigest()


def test_fixture_covers_every_case(fixture):
    assert sorted(fixture) == sorted(name for name, _, _, _ in sr.CASES)
    assert len(set(name for name, _, _, _ in sr.CASES)) == len(sr.CASES)


@pytest.mark.parametrize('case', sr.CASES, ids=[c[0] for c in sr.CASES])
def test_restatement_equals_the_reference(fixture, case):
    name, inp, method, kw = case
    rate, x = sr.make_input(inp)
    y = sr.run(method, x, rate, **kw)
    rec = fixture[name]
    if 'raises' in rec:             # a row without silence in a slice mode: the reference raises, we keep the row
        assert rec['raises'] == 'IndexError' and method == 'rms' and kw['mode'] != 'remove'
        assert sr.rms_silences(x, rate, **{k: v for k, v in kw.items() if k not in ('mode', 'replace_by')}) == []
        assert np.array_equal(y, x)
    else:
        assert (len(y), _sha(y)) == (rec['len'], rec['sha256'])


@pytest.mark.parametrize('case', sr.CASES, ids=[c[0] for c in sr.CASES])
def test_inputs_keep_their_distance_from_the_thresholds(case):
    # conditions on the inputs (not measurements): the float decisions of another summation order cannot flip
    name, inp, method, kw = case
    rate, x = sr.make_input(inp)
    m = sr.margin(method, x, rate, **kw)
    print(f'{name}: margin {m:.3e} (needs {sr.MARGINS[method]:.0e})')
    assert m >= sr.MARGINS[method]


def test_golden_wav_lengths(fixture):
    rate, x = sr.make_input('wav')
    assert rate == 16000 and x.shape == (64880,)
    table = {'start': (64880, 64880, 59280), 'end': (63360, 64800, 56320), 'start_end': (63360, 64800, 50720),
             'remove': (63360, 64800, 50720)}
    for mode, row in table.items():
        for db, n in zip((-25, -35, -15), row):
            assert fixture[f'wav-{mode}{db}']['len'] == n
            assert len(sr.trim_rms(x, rate, mode=mode, threshold=db, min_silence=0.1, replace_by=0.4)) == n
    assert fixture['wav-threshold']['len'] == len(sr.trim_threshold(x)) == 49345
    assert fixture['wav-remove']['len'] == len(sr.trim_mean_window(x, rate)) == 51943


def test_interior_pauses():
    rate, x = sr.make_input('pause_long')                       # 0.3 s voice, 0.6 s pause, 0.4 s voice
    (s, e), = sr.rms_silences(x, rate)
    S, E, rb = int(s * rate), int(e * rate), int(0.2 * rate)
    assert 0.55 < e - s <= 0.6
    y = sr.trim_rms(x, rate, mode='remove', replace_by=0.2)
    assert len(y) == len(x) - ((E - rb // 2) - (S + rb // 2)) and len(x) - len(y) > 0.35 * rate
    assert np.array_equal(y, np.concatenate([x[:S + rb // 2], x[E - rb // 2:]]))
    # replace_by longer than the pause leaves it alone; replace_by = 0 removes all of it
    assert np.array_equal(sr.trim_rms(x, rate, mode='remove', replace_by=0.8), x)
    assert np.array_equal(sr.trim_rms(x, rate, mode='remove', replace_by=0), np.concatenate([x[:S], x[E:]]))
    # a pause shorter than min_silence is kept
    rate, x = sr.make_input('pause_short')
    assert sr.rms_silences(x, rate) == [] and np.array_equal(sr.trim_rms(x, rate, mode='remove'), x)


def test_short_voice_between_silences_is_merged_away():
    rate, x = sr.make_input('burst')
    merged, apart = sr.rms_silences(x, rate, min_voice_time=0.2), sr.rms_silences(x, rate, min_voice_time=0)
    assert len(apart) == 4 and len(merged) == 3
    assert merged[1] == (apart[1][0], apart[2][1])              # the 0.12 s burst lies inside the merged silence
    assert 0.1 < apart[2][0] - apart[1][1] < 0.2
    kept = sr.trim_rms(x, rate, mode='remove', replace_by=0.1, min_voice_time=0)
    gone = sr.trim_rms(x, rate, mode='remove', replace_by=0.1, min_voice_time=0.2)
    # merged, the burst (0.12 s) and one of the two replacement silences (0.1 s) go as well
    assert 0.2 * rate < len(kept) - len(gone) < 0.25 * rate


def test_sample_bounds_are_truncated_double_products():
    rate, x = sr.make_input('block9')
    (s, e), = sr.rms_silences(x, rate)
    assert rate == 22050 and s == 9 * (220 / 22050)
    assert int(s * rate) == 1979 and 9 * 220 != 1979
    y = sr.trim_rms(x, rate, mode='remove', replace_by=0.1)
    assert np.array_equal(y[:1979 + 1102], x[:1979 + 1102]) and y[1979 + 1102] != x[1979 + 1102]


def test_degenerate_rows(fixture):
    rate, loud = sr.make_input('all_loud')
    for mode in sr.RMS_MODES:
        assert np.array_equal(sr.trim_rms(loud, rate, mode=mode), loud)
    assert all(fixture[f'all_loud-{m}'] == {'raises': 'IndexError'} for m in sr.SLICE_MODES)
    assert fixture['all_loud-remove']['len'] == len(loud)
    rate, quiet = sr.make_input('all_silent')
    assert len(sr.trim_rms(quiet, rate, mode='start_end')) == 0 == fixture['all_silent-start_end']['len']
    assert len(sr.trim_rms(quiet, rate, mode='remove')) == int(0.5 * rate) == fixture['all_silent-remove']['len']
    for name, n in (('one_sample', 1), ('short_row', 100)):
        rate, x = sr.make_input(name)
        assert len(x) == n and n < int(0.01 * rate) and np.array_equal(sr.trim_rms(x, rate, mode='remove'), x)
    # trailing silence with L = k * bs and k * bs + 1: the clamp min(L / rate, j * bt) and the |E - L| <= 1 test
    for name, extra in (('tail_kbs', 0), ('tail_kbs1', 1)):
        rate, x = sr.make_input(name)
        assert len(x) % 220 == (int(0.3 * rate) + extra) % 220
        (s, e), = sr.rms_silences(x, rate)
        assert e <= len(x) / rate and abs(int(e * rate) - len(x)) <= 1
        for mode in ('end', 'start_end', 'remove'):
            assert len(sr.trim_rms(x, rate, mode=mode, replace_by=0.1)) == int(s * rate) + int(0.1 * rate)


def test_mean_window_equals_the_direct_convolution():
    rate, x = sr.make_input('mw_pattern')
    for ms, th in ((0.15, 0.025), (0.2, 0.05), (0.01, 0.025)):         # odd, even and small windows
        w = int(ms * rate)
        direct = np.convolve(np.square(x), np.ones((w,)) / (w * th), mode='same')
        # the prefix sums carry the rounding of a running total (<= sum x^2): absolute, and tiny next to the threshold, where
        # the inputs keep a relative distance of 1e-9
        atol = 1e-13 * float(np.sum(np.square(x), dtype=np.float64)) / (w * th)
        assert atol < 1e-9 * th
        assert np.allclose(sr.mean_window_conv(x, rate, th, ms), direct, rtol=1e-12, atol=atol)
    with pytest.raises(ValueError, match='L = 3000.*w = 3307'):
        sr.trim_mean_window(x[:3000], rate)


# ---------------------------------------------------------------------------------------------- host side, no GPU call
class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError(f'engine.{name} touched')


def test_dispatcher_refuses_before_touching_the_engine():
    from text_to_speech_amd.audio import trim_silence
    x = np.zeros(4000, np.float32)
    for method in ('ffmpeg', 'spectral', b'ffmpeg'):
        with pytest.raises(ValueError, match='window, rms, threshold, remove'):
            trim_silence(x, engine=_NoEngine(), rate=R, method=method)
    with pytest.raises(ValueError, match='unknown arguments'):
        trim_silence(x, engine=_NoEngine(), rate=R, method='rms', window_length=0.2)
    with pytest.raises(ValueError, match='one row'):
        trim_silence(np.zeros((2, 4000), np.float32), engine=_NoEngine(), rate=R, method='rms')


def test_argument_errors_before_any_gpu_call():
    # HipEngine's argument checks run before the handle is touched: an object without a handle still raises ValueError
    from text_to_speech_amd.audio import trim_silence
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine.__new__(HipEngine)
    x = np.zeros(3000, np.float32)
    with pytest.raises(ValueError, match="mode 'remove'"):
        trim_silence(x, engine=eng, rate=R, method='threshold', mode='remove')
    with pytest.raises(ValueError, match='L = 3000.*w = 3307'):
        trim_silence(x, engine=eng, rate=R, method='remove')
    with pytest.raises(ValueError, match='L = 100.*w = 3307'):
        eng.remove_silence(np.zeros((2, 4000), np.float32), R, lengths=[4000, 100], method='remove')
    with pytest.raises(ValueError, match='replace_by'):
        trim_silence(x, engine=eng, rate=R, method='rms', replace_by=-1)
    with pytest.raises(ValueError, match='replace_by'):
        eng.remove_silence(x, R, replace_by=-0.5)
    with pytest.raises(ValueError, match='stream'):
        eng.remove_silence(x, R, stream=object())
    with pytest.raises(ValueError, match='block_size'):
        eng.remove_silence(x, R, block_size=0)
    with pytest.raises(ValueError, match='rate'):
        eng.remove_silence(x, None)
    with pytest.raises(ValueError, match='method'):
        eng.remove_silence(x, R, method='ffmpeg')
    with pytest.raises(ValueError, match='mode'):
        eng.remove_silence(x, R, mode='middle')
    with pytest.raises(ValueError, match='threshold'):
        eng.remove_silence(x, R, method='threshold', threshold=-0.1)
    with pytest.raises(ValueError, match='threshold'):
        eng.remove_silence(x, R, threshold=float('nan'))
    with pytest.raises(ValueError, match='min_voice_time'):
        eng.remove_silence(x, R, min_voice_time=-1.)
    with pytest.raises(ValueError, match='lengths'):
        eng.remove_silence(np.zeros((2, 4000), np.float32), R, lengths=[4001, 10])
    with pytest.raises(ValueError, match='too large'):
        eng.remove_silence(np.zeros((1 << 24) + 1, np.float32), R)


def test_dispatcher_routes_methods_to_the_engine():
    from text_to_speech_amd.audio import trim_silence

    class FakeEngine:
        def __init__(self):
            self.calls = []

        def trim_silence(self, audio, rate, **kw):
            self.calls.append(('trim_silence', rate, kw))
            return 5, 15

        def remove_silence(self, audio, rate, **kw):
            self.calls.append(('remove_silence', rate, kw))
            return audio[::2]

    eng, x = FakeEngine(), np.arange(40, dtype=np.float32)
    assert np.array_equal(trim_silence(x, engine=eng, rate=R), x[5:15])
    assert np.array_equal(trim_silence(x, engine=eng, rate=R, method='window', mode='end', add_end=1.), x[5:15])
    for method in ('rms', 'threshold', 'remove'):
        assert np.array_equal(trim_silence(x, engine=eng, rate=R, method=method, threshold=0.5), x[::2])
    assert eng.calls == [('trim_silence', R, {}), ('trim_silence', R, {'mode': 'end', 'add_end': 1.})] + \
        [('remove_silence', R, {'method': m, 'threshold': 0.5}) for m in ('rms', 'threshold', 'remove')]


def test_facade_dict_reaches_remove_silence():
    from test_host_logic import FakeSynth, FakeVocoder
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow

    class FakeEngine:
        def __init__(self):
            self.calls = []

        def reduce_noise(self, audio, rate):
            raise AssertionError('reduce_noise was not asked for')

        def trim_silence(self, audio, rate):
            self.calls.append(('trim_silence', audio.shape, rate))
            return 10, 20

        def remove_silence(self, audio, rate, **kw):
            self.calls.append(('remove_silence', audio.shape, rate, kw))
            return audio[100:300]

    synth, voc = FakeSynth([100]), FakeVocoder()
    synth.engine = FakeEngine()
    text = 'Hello world, this is a test.'
    plain = Tacotron2(synth).infer(text, vocoder=WaveGlow(voc))
    synth.lengths_seq = [100]
    out = Tacotron2(synth).infer(text, vocoder=WaveGlow(voc), trim_silence={'method': 'rms', 'mode': 'remove', 'replace_by': 0.4})
    assert synth.engine.calls == [('remove_silence', (25600,), 22050, {'method': 'rms', 'mode': 'remove', 'replace_by': 0.4})]
    assert np.array_equal(out['audio'], plain['audio'][100:300])
    # True keeps calling trim_silence(audio, rate) and nothing else
    synth.lengths_seq = [100]
    synth.engine.calls.clear()
    out = Tacotron2(synth).infer(text, vocoder=WaveGlow(voc), trim_silence=True)
    assert synth.engine.calls == [('trim_silence', (25600,), 22050)]
    assert np.array_equal(out['audio'], plain['audio'][10:20])
    assert all('trim_silence' not in kw for _, kw in voc.calls) and all('trim_silence' not in kw for _, _, kw in synth.calls)


def test_empty_dict_and_flag_only_entry_points():
    from test_host_logic import FakeSynth, FakeVocoder
    from text_to_speech_amd.pipeline import TTSPipeline
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow
    # an empty dict trims nothing, in _finish and in _clean_waveform alike
    synth, voc = FakeSynth([100]), FakeVocoder()
    synth.engine = _NoEngine()
    text = 'Hello world, this is a test.'
    plain = Tacotron2(synth).infer(text, vocoder=WaveGlow(voc))
    synth.lengths_seq = [100]
    assert np.array_equal(Tacotron2(synth).infer(text, vocoder=WaveGlow(voc), trim_silence={})['audio'], plain['audio'])

    class Half:
        def reduce_noise(self, audio, rate):
            return audio * 0.5

    model = Tacotron2(synth)
    synth.engine = Half()
    x = np.arange(8, dtype=np.float32)
    assert np.array_equal(model._clean_waveform(x, None, True, {}), x * 0.5)
    # synthesize_tokens' trim_silence is a flag: a dict is refused, not read as True
    p = TTSPipeline.__new__(TTSPipeline)
    p.engine = _NoEngine()
    with pytest.raises(ValueError, match='flag'):
        p.synthesize_tokens(np.ones((1, 4), np.int32), trim_silence={'method': 'rms'})


def test_dispatcher_returns_float32_for_every_method():
    from text_to_speech_amd.audio import trim_silence

    class FakeEngine:
        def trim_silence(self, audio, rate, **kw):
            assert audio.dtype == np.float32
            return 2, 6

        def remove_silence(self, audio, rate, **kw):
            assert audio.dtype == np.float32
            return audio[1:]

    for x in (np.arange(8, dtype=np.float64), np.arange(8, dtype=np.int16)):
        y = trim_silence(x, engine=FakeEngine(), rate=R)
        assert y.dtype == np.float32 and np.array_equal(y, x[2:6])
        assert trim_silence(x, engine=FakeEngine(), rate=R, method='rms').dtype == np.float32
