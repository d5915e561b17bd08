"""CPU: the resampling rules (tests/resample_ref.py) against scipy and the reference's golden, the length formula, and the
host side of HipEngine.resample / load_audio(resample=True) (no GPU call)."""
import hashlib
import os

import numpy as np
import pytest

import audio_ref
import resample_ref

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
WAV = os.path.join(GOLDEN, 'audio_test_16k.wav')
FIX = os.path.join(GOLDEN, 'resample_fixture.npz')
RATES = [8000, 16000, 22050, 24000, 44100, 48000]
LENGTHS = [1, 2, 3, 7, 64, 101, 1000, 4096, 11200, 65537]


def test_resampled_length_formula():
    from text_to_speech_amd.audio import resampled_length
    assert resampled_length(11200, 16000, 22050) == 15434           # 11200 * 22050 // 16000 would give 15435
    assert resampled_length(30, 44100, 22050) == 14                 # and 15 here
    assert resampled_length(64880, 16000, 22050) == 89412
    rng = np.random.default_rng(3)
    for n in rng.integers(1, 1 << 22, 200):
        for r, t in ((16000, 22050), (44100, 22050), (48000, 22050), (22050, 24000)):
            m = int(int(n) / r * t)
            if m >= 1:
                assert resampled_length(int(n), r, t) == m
    for bad in ((1, 44100, 22050), (10, 0, 22050), (10, 16000, -1)):
        with pytest.raises(ValueError):
            resampled_length(*bad)


@pytest.mark.parametrize('n', LENGTHS)
def test_restatement_equals_scipy(n):
    from scipy import signal
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    for r in RATES:
        for t in RATES:
            if r == t:
                continue
            m = resample_ref.resampled_length(n, r, t)
            if m < 1:
                continue
            ref = signal.resample(x, m)
            got = resample_ref.resample(x, m)
            assert got.shape == ref.shape == (m,)
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize('n', [1, 2, 3, 7, 64, 101, 4096, 11200, 65537])
def test_bluestein_complex64_close_to_float64(n):
    rng = np.random.default_rng(n + 1)
    x = rng.standard_normal(n).astype(np.float32)
    worst = 0.0
    for r, t in ((16000, 22050), (22050, 16000), (44100, 22050), (8000, 48000)):
        m = resample_ref.resampled_length(n, r, t)
        if m < 1:
            continue
        ref = resample_ref.resample(x.astype(np.float64), m)
        got = resample_ref.resample_bluestein(x, m)
        err = float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))
        worst = max(worst, err)
        assert err <= 2e-6, (n, r, t, err)
    print(f'n={n}: worst relative max-abs {worst:.2e}')


def test_fixture_hashes_and_golden_rebuilt_with_scipy():
    from scipy import signal
    f = np.load(FIX)
    rate, raw = audio_ref.read_wav(WAV)
    assert rate == 16000 and raw.shape == (64880,)
    n = int(f['resample_len'])
    assert n == 89412 and f['resample_every8'].shape == ((n + 7) // 8,) and f['mel'].shape == (350, 80)
    full = audio_ref.normalize_audio(signal.resample(raw, resample_ref.resampled_length(raw.size, rate, 22050)))
    assert full.dtype == np.float32 and full.shape == (n,)
    assert hashlib.sha256(full.tobytes()).hexdigest() == str(f['resample_f32_sha256'])
    assert np.array_equal(full[::8], f['resample_every8'])
    for k in ('resample_sha256', 'mel_sha256'):
        assert len(str(f[k])) == 64


def test_bluestein_restatement_near_golden():
    f = np.load(FIX)
    rate, raw = audio_ref.read_wav(WAV)
    m = resample_ref.resampled_length(raw.size, rate, 22050)
    y = audio_ref.normalize_audio(resample_ref.resample_bluestein(raw.astype(np.float32), m))
    d = (y[::8] - f['resample_every8']).astype(np.float64)
    print(f'complex64 restatement vs golden: max-abs {np.abs(d).max():.2e}, rms {np.sqrt(np.mean(d ** 2)):.2e}')
    assert float(np.abs(d).max()) <= 1e-6 and float(np.sqrt(np.mean(d ** 2))) <= 1e-7


class _NoGpu:
    """Stands in for a HipEngine: any call is a failure (argument errors must come first)."""
    def __getattr__(self, name):
        raise AssertionError(f'engine.{name} called')


def test_resample_argument_errors_before_any_gpu_call():
    from text_to_speech_amd.engine import HipEngine
    eng = HipEngine.__new__(HipEngine)          # no handle: any GPU call would raise AttributeError, not ValueError
    a = np.zeros((2, 4000), np.float32)
    with pytest.raises(ValueError, match='rates'):
        eng.resample(a, 0, 22050)
    with pytest.raises(ValueError, match='rates'):
        eng.resample(a, 16000, -22050)
    with pytest.raises(ValueError, match='< 1'):
        eng.resample(np.zeros(1, np.float32), 44100, 22050)
    with pytest.raises(ValueError, match='lengths'):
        eng.resample(a, 16000, 22050, lengths=[4001, 10])
    with pytest.raises(ValueError, match='lengths'):
        eng.resample(a, 16000, 22050, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match='< 1'):
        eng.resample(a, 44100, 22050, lengths=[1, 4000])               # row 0 resamples to no sample
    with pytest.raises(ValueError, match='2\\^24'):
        eng.resample(np.broadcast_to(np.float32(0), (1, (1 << 24) + 1)), 16000, 8000)
    with pytest.raises(ValueError, match='2\\^24'):
        eng.resample(np.broadcast_to(np.float32(0), (1, 1 << 23)), 16000, 48000)
    with pytest.raises(ValueError, match='31-bit'):
        eng.resample(np.broadcast_to(np.float32(0), (129, 1 << 22)), 16000, 16000)
    with pytest.raises(ValueError, match='stream'):
        eng.resample(a, 16000, 22050, stream=object())
    with pytest.raises(ValueError, match=r'\[N\] or \[B, N\]'):
        eng.resample(np.zeros((1, 2, 3), np.float32), 16000, 22050)


def test_load_audio_resample_off_is_unchanged():
    from text_to_speech_amd import audio
    eng = _NoGpu()
    with pytest.raises(ValueError, match='resampling'):
        audio.load_audio(WAV, rate=22050, engine=eng)
    with pytest.raises(ValueError, match='resampling'):
        audio.load_mel(WAV, engine=eng)
    with pytest.raises(ValueError, match='unknown'):
        audio.load_audio(WAV, engine=eng, resample_rate=3)
    a = audio.load_audio(WAV, rate=16000, engine=eng, resample=True)     # same rate: nothing to resample
    b = audio.load_audio(WAV, rate=16000, engine=eng)
    assert np.array_equal(a, b) and a.shape == (64880,)


class _Recorder:
    """Fake engine: records the calls, resamples with the float64 restatement."""
    def __init__(self):
        self.calls = []

    def resample(self, audio, rate, target_rate):
        self.calls.append(('resample', audio.dtype, audio.copy(), rate, target_rate))
        return resample_ref.resample(audio, resample_ref.resampled_length(audio.size, rate, target_rate)).astype(np.float32)

    def reduce_noise(self, audio, rate, renormalize=False, **kw):
        self.calls.append(('reduce_noise', audio.copy(), rate))
        return audio

    def trim_silence(self, audio, rate, **kw):
        self.calls.append(('trim_silence', audio.copy(), rate))
        return 0, audio.size

    def mel_stft(self, audio):
        self.calls.append(('mel_stft', audio.copy()))
        return np.zeros((1, audio.size // 256 + 1, 80), np.float32)


def test_load_audio_resamples_once_before_normalization():
    from text_to_speech_amd import audio
    rate, raw = audio_ref.read_wav(WAV)
    eng = _Recorder()
    y = audio.load_audio(WAV, 22050, engine=eng, resample=True, reduce_noise=True, trim_silence=True)
    names = [c[0] for c in eng.calls]
    assert names == ['resample', 'reduce_noise', 'trim_silence']
    _, dt, got_in, r, t = eng.calls[0]
    assert (r, t) == (16000, 22050) and dt == np.float32
    assert np.array_equal(got_in, raw.astype(np.float32))            # raw samples, not normalized ones
    assert eng.calls[1][2] == 22050 and eng.calls[2][2] == 22050     # the clean-up runs at the new rate
    expect = audio_ref.normalize_audio(resample_ref.resample(raw.astype(np.float32), 89412).astype(np.float32))
    assert y.shape == (89412,) and np.array_equal(y, expect)


def test_load_audio_resample_sources():
    from text_to_speech_amd import audio
    x = np.sin(np.arange(3000) * 0.01).astype(np.float32)
    eng = _Recorder()
    y = audio.load_audio(x, 22050, engine=eng, resample=True, source_rate=44100)
    assert [c[3:] for c in eng.calls] == [(44100, 22050)] and y.shape == (1500,)
    eng = _Recorder()
    y = audio.load_audio({'audio': x, 'rate': 48000}, 22050, engine=eng, resample=True)
    assert [c[3:] for c in eng.calls] == [(48000, 22050)] and y.shape == (resample_ref.resampled_length(3000, 48000, 22050),)
    eng = _Recorder()
    y = audio.load_audio(x, 22050, engine=eng, resample=True)        # raw samples without source_rate: taken at `rate`
    assert eng.calls == [] and y.shape == (3000,)
    eng = _Recorder()
    audio.load_audio({'audio': x, 'rate': 48000}, 22050, engine=eng)  # resample off: the dict's rate is not used
    assert eng.calls == []
    eng = _Recorder()
    m = audio.load_mel(WAV, engine=eng, resample=True)
    assert [c[0] for c in eng.calls] == ['resample', 'mel_stft'] and eng.calls[0][3:] == (16000, 22050)
    assert m.shape == (350, 80)
