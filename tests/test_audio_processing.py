"""CPU: the waveform clean-up fixtures, the numpy restatement against the reference's goldens, and the host side of
text_to_speech_amd.audio (no GPU call)."""
import hashlib
import os

import numpy as np
import pytest

import audio_ref

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
WAV = os.path.join(GOLDEN, 'audio_test_16k.wav')
FIX = os.path.join(GOLDEN, 'audio_processing_fixture.npz')


@pytest.fixture(scope='module')
def fix():
    return np.load(FIX)


@pytest.fixture(scope='module')
def wav():
    return audio_ref.read_wav(WAV)


def test_fixture_hashes(fix, wav):
    assert hashlib.sha256(open(WAV, 'rb').read()).hexdigest() == str(fix['wav_sha256'])
    rate, raw = wav
    assert rate == 16000 and raw.dtype == np.int16 and raw.shape == (64880,)
    assert fix['reduce_noise'].dtype == np.float32 and fix['reduce_noise'].shape == (64880,)
    assert (int(fix['trim_start']), int(fix['trim_end'])) == (3130, 58805)
    for k in ('reduce_noise_sha256', 'trim_silence_sha256', 'trim_silence_f32_sha256'):
        assert len(str(fix[k])) == 64


def test_restatement_matches_reduce_noise_golden(fix, wav):
    rate, raw = wav
    x = audio_ref.normalize_audio(raw)
    y = audio_ref.normalize_audio(audio_ref.reduce_noise(x, rate=rate))      # load_audio: normalize again after reduce_noise
    err = float(np.abs(y - fix['reduce_noise']).max())
    print('restatement vs golden max-abs', err)
    assert err <= 1e-6


def test_restatement_fp32_dft_matches_reduce_noise_golden(fix, wav):
    # the GPU's form: forward DFT as an fp32 matrix product
    rate, raw = wav
    x = audio_ref.normalize_audio(raw)
    y = audio_ref.normalize_audio(audio_ref.reduce_noise(x, rate=rate, dft='f32'))
    d = y - fix['reduce_noise']
    assert float(np.abs(d).max()) <= 1e-6 and float(np.sqrt(np.mean(d.astype(np.float64) ** 2))) <= 1e-7


def test_restatement_trim_matches_golden(fix, wav):
    rate, raw = wav
    x = audio_ref.normalize_audio(raw)
    start, end = audio_ref.trim_window(x, rate)
    assert (start, end) == (int(fix['trim_start']), int(fix['trim_end']))
    assert hashlib.sha256(x[start:end].astype(np.float32).tobytes()).hexdigest() == str(fix['trim_silence_f32_sha256'])


def test_read_wav_and_normalize(wav):
    from text_to_speech_amd import audio
    rate, raw = audio.read_wav(WAV)
    assert rate == wav[0] and np.array_equal(raw, wav[1])
    a = audio.normalize_audio(raw, max_val=1.)
    b = audio_ref.normalize_audio(raw)
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(audio.normalize_audio(raw), audio_ref.normalize_audio(raw, max_val=32767))
    z = audio.normalize_audio(np.full(10, 3.0), max_val=1.)                 # constant -> zeros, no division
    assert z.dtype == np.float32 and not z.any()


# Trim cases whose indices follow by hand from np.convolve (TRIM_CASES: audio, rate, kwargs, expected (start, end)).
#  * window_length 4 -> window [0, .5, .5, 0]: conv[k] = (x[k+1]^2 + x[k+2]^2) / 2, so a block of ones on [a, b) gives
#    conv > 0 exactly for k in [a - 2, b - 2]; silent edges -> both thresholds threshold / 50 = 0.002;
#    end = last + int(4 * add_end), start = first - int(4 * add_start).
#  * window_length 8 -> window [0, 1/3, 2/3, 1, 1, 2/3, 1/3, 0] / 4; a 6-sample row with x[0] = 1 is shorter than the
#    window: np.convolve swaps the operands, conv[k] = w[k + 5] = [1/6, 1/12, 0]; mean * 5 = 0.42 -> threshold 0.1, so
#    only k = 0 passes: start 0, end = 0 + int(8 * 0.5) = 4.
def _block(n, a, b):
    x = np.zeros(n, np.float32)
    x[a:b] = 1
    return x


TRIM_CASES = [
    (_block(100, 30, 70), dict(window_length=4), (28, 74)),
    (_block(100, 30, 70), dict(window_length=4, mode='start'), (28, 100)),
    (_block(100, 30, 70), dict(window_length=4, mode='end'), (0, 74)),
    (_block(100, 30, 70), dict(window_length=4, add_start=1.0), (24, 74)),
    (_block(100, 40, 45), dict(window_length=4), (0, 100)),              # 49 - 38 = 11 <= 100 // 5: keep the whole row
    (_block(6, 0, 1), dict(window_length=8, add_end=0.5), (0, 4)),       # shorter than the window
]


@pytest.mark.parametrize('x,kw,expected', TRIM_CASES)
def test_restatement_trim_pinned_cases(x, kw, expected):
    assert audio_ref.trim_window(x, 16000, **kw) == expected


class _NoGpu:
    """Stands in for a HipEngine: any call is a failure (argument errors must come first)."""
    def __getattr__(self, name):
        raise AssertionError(f'engine.{name} called')


def test_load_audio_argument_errors():
    from text_to_speech_amd import audio
    eng = _NoGpu()
    with pytest.raises(ValueError, match='resampling'):
        audio.load_audio(WAV, rate=22050, engine=eng, reduce_noise=True)
    with pytest.raises(ValueError, match="method='window'"):
        audio.load_audio(WAV, rate=None, engine=eng, trim_silence=True, method='rms')
    with pytest.raises(ValueError, match='needs `rate`'):
        audio.load_audio(np.zeros(100, np.float32), engine=eng)
    with pytest.raises(ValueError, match='unknown'):
        audio.load_audio(WAV, engine=eng, trim_silence=True, power=3)
    with pytest.raises(ValueError, match='mono'):
        audio.load_audio(np.zeros((2, 100), np.float32), rate=16000, engine=eng)
    with pytest.raises(ValueError, match='resampling'):                    # load_mel loads at the STFT's 22 050 Hz
        audio.load_mel(WAV, engine=eng)
    with pytest.raises(ValueError, match='22050'):
        audio.load_mel(WAV, rate=16000, engine=eng)
    a = audio.load_audio(WAV, rate=16000, engine=eng)                       # no clean-up: host only
    assert a.dtype == np.float32 and a.shape == (64880,)


def test_engine_argument_errors_before_any_gpu_call():
    # HipEngine's argument checks run before the handle is touched: an object without a handle still raises ValueError
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine.__new__(HipEngine)
    a = np.zeros((2, 4000), np.float32)
    with pytest.raises(ValueError, match='lengths'):
        eng.reduce_noise(a, 16000, lengths=[4001, 10])
    with pytest.raises(ValueError, match='lengths'):
        eng.reduce_noise(a, 16000, lengths=[0, 10])
    with pytest.raises(ValueError, match='lengths'):
        eng.trim_silence(a, 16000, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match='noise'):
        eng.reduce_noise(a, 16000, noise=np.zeros((3, 100), np.float32))
    with pytest.raises(ValueError, match='at least one sample'):
        eng.reduce_noise(a, 16000, noise_length=0)
    with pytest.raises(ValueError, match='rate'):
        eng.reduce_noise(a, None)
    with pytest.raises(ValueError, match='mode'):
        eng.trim_silence(a, 16000, mode='middle')
    with pytest.raises(ValueError, match='window_length'):
        eng.trim_silence(a, 16000, window_length=1)
    with pytest.raises(ValueError, match='margins'):
        eng.trim_silence(a, 16000, add_end=-1.0)
    with pytest.raises(ValueError, match='stream'):
        eng.reduce_noise(a, 16000, stream=object())


def test_synthesize_tokens_rejects_trim_on_device():
    from text_to_speech_amd.pipeline import TTSPipeline
    p = TTSPipeline.__new__(TTSPipeline)
    p.engine = _NoGpu()
    with pytest.raises(ValueError, match='on_device'):
        p.synthesize_tokens(np.ones((1, 4), np.int32), on_device=True, trim_silence=True)


def test_facade_cleanup_keywords_reach_the_engine_not_the_vocoder():
    from test_host_logic import FakeSynth, FakeVocoder
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow

    class FakeEngine:
        def __init__(self):
            self.calls = []

        def reduce_noise(self, audio, rate):
            self.calls.append(('reduce_noise', audio.shape, rate))
            return audio * 0.5

        def trim_silence(self, audio, rate):
            self.calls.append(('trim_silence', audio.shape, rate))
            return 10, 20

    synth, voc = FakeSynth([100]), FakeVocoder()
    synth.engine = FakeEngine()
    text = 'Hello world, this is a test.'
    plain = Tacotron2(synth).infer(text, vocoder=WaveGlow(voc))
    assert synth.engine.calls == []
    synth.lengths_seq = [100]
    out = Tacotron2(synth).infer(text, vocoder=WaveGlow(voc), reduce_noise=True, trim_silence=True)
    assert synth.engine.calls == [('reduce_noise', (25600,), 22050), ('trim_silence', (25600,), 22050)]
    assert np.array_equal(out['audio'], plain['audio'][10:20] * 0.5)
    assert all('reduce_noise' not in kw and 'trim_silence' not in kw for _, kw in voc.calls)
    assert all('reduce_noise' not in kw and 'trim_silence' not in kw for _, _, kw in synth.calls)


def test_overlapped_predict_cleans_up_on_the_vocoders_engine():
    # predict(overlap=True): the synthesizer's handle is busy in the producer thread, so the clean-up must use the vocoder's
    from test_host_logic import FakeSynth, FakeVocoder
    from text_to_speech_amd.tacotron2 import Tacotron2
    from text_to_speech_amd.waveglow import WaveGlow

    class Busy:
        def __getattr__(self, name):
            raise AssertionError(f'synthesizer engine.{name} called')

    class FakeEngine:
        def __init__(self):
            self.calls = []

        def reduce_noise(self, audio, rate):
            self.calls.append('reduce_noise')
            return audio

        def trim_silence(self, audio, rate):
            self.calls.append('trim_silence')
            return 0, len(audio)

    synth, voc = FakeSynth([], default=100), FakeVocoder()
    synth.engine, voc.engine = Busy(), FakeEngine()
    texts = ['Hello world, this is a test.', 'A second sentence for the stream.']
    res = Tacotron2(synth).predict(texts, vocoder=WaveGlow(voc), overlap=True, save=False, reduce_noise=True,
                                   trim_silence=True)
    assert len(res) == 2 and voc.engine.calls == ['reduce_noise', 'trim_silence'] * 2
    assert all('reduce_noise' not in kw and 'trim_silence' not in kw for _, kw in voc.calls)
    assert all('reduce_noise' not in kw and 'trim_silence' not in kw for _, _, kw in synth.calls)
