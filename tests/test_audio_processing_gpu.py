"""GPU parity: waveform clean-up (csrc/audio_proc.hip) against the reference's goldens and the numpy restatement."""
import hashlib
import os

import numpy as np
import pytest

import audio_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
WAV = os.path.join(GOLDEN, 'audio_test_16k.wav')
FIX = os.path.join(GOLDEN, 'audio_processing_fixture.npz')
RATE = 22050
# shorter than 2048; between the 4410-sample noise clip and one hop above it; a multiple of 512; ~9 s; shorter than the
# noise clip (its clip is the whole row); a plain length
LENGTHS = [1500, 4410 + 300, 512 * 40, 198450, 3000, 50001]


def _rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


@pytest.fixture(scope='module')
def ragged():
    rng = np.random.default_rng(7)
    N = max(LENGTHS)
    a = np.zeros((len(LENGTHS), N), np.float32)
    for b, L in enumerate(LENGTHS):
        t = np.arange(L) / RATE
        sig = 0.5 * np.sin(2 * np.pi * 220 * t) * (t > min(0.3, L / RATE / 2))
        a[b, :L] = (sig + 0.02 * rng.standard_normal(L)).astype(np.float32)
        a[b, L:] = rng.standard_normal(N - L)          # garbage beyond the row's length must not leak in
    return a


def test_load_audio_reduce_noise_matches_reference_golden(gpu_engine):
    from text_to_speech_amd.audio import load_audio
    f = np.load(FIX)
    y = load_audio(WAV, rate=None, engine=gpu_engine, reduce_noise=True)
    d = y - f['reduce_noise']
    print(f'reduce_noise vs reference golden: max-abs {np.abs(d).max():.3e}, rms {_rms(d):.3e}')
    assert y.dtype == np.float32 and y.shape == (64880,)
    assert float(np.abs(d).max()) <= 1e-5 and _rms(d) <= 1e-6


def test_load_audio_trim_matches_reference_golden(gpu_engine):
    from text_to_speech_amd.audio import load_audio, normalize_audio, read_wav
    f = np.load(FIX)
    y = load_audio(WAV, rate=None, engine=gpu_engine, trim_silence=True, method='window')
    assert hashlib.sha256(y.astype(np.float32).tobytes()).hexdigest() == str(f['trim_silence_f32_sha256'])
    rate, raw = read_wav(WAV)
    assert gpu_engine.trim_silence(normalize_audio(raw, max_val=1.), rate) == (3130, 58805)


def test_load_mel_after_cleanup(gpu_engine):
    from text_to_speech_amd.audio import load_audio, load_mel
    rng = np.random.default_rng(5)
    t = np.arange(30000) / RATE
    raw = (0.5 * np.sin(2 * np.pi * 300 * t) * (t > 0.4) + 0.01 * rng.standard_normal(t.size)).astype(np.float32)
    a = load_audio(raw, RATE, engine=gpu_engine, reduce_noise=True, trim_silence=True)
    m = load_mel(raw, engine=gpu_engine, reduce_noise=True, trim_silence=True)
    assert np.array_equal(m, gpu_engine.mel_stft(a)[0])
    with pytest.raises(ValueError, match='resampling'):          # the 16 kHz wav is not at the STFT's 22 050 Hz
        load_mel(WAV, engine=gpu_engine)


def test_reduce_noise_ragged_batch(gpu_engine, ragged):
    out = gpu_engine.reduce_noise(ragged, RATE, lengths=LENGTHS)
    for b, L in enumerate(LENGTHS):
        ref = audio_ref.reduce_noise(ragged[b, :L], rate=RATE, dft='f32')
        one = gpu_engine.reduce_noise(ragged[b, :L], RATE)
        e_ref, e_one = float(np.abs(out[b, :L] - ref).max()), float(np.abs(out[b, :L] - one).max())
        print(f'row {b} L={L}: vs restatement {e_ref:.2e}, vs one-row call {e_one:.2e}')
        assert e_ref <= 1e-5 and np.array_equal(out[b, :L], one)
        assert not out[b, L:].any()


def test_reduce_noise_renormalize(gpu_engine, ragged):
    out = gpu_engine.reduce_noise(ragged, RATE, lengths=LENGTHS, renormalize=True)
    for b, L in enumerate(LENGTHS):
        ref = audio_ref.normalize_audio(audio_ref.reduce_noise(ragged[b, :L], rate=RATE, dft='f32'))
        assert float(np.abs(out[b, :L] - ref).max()) <= 1e-5
        assert not out[b, L:].any()


def test_reduce_noise_explicit_noise_and_device_paths(gpu_engine, ragged):
    import torch
    rng = np.random.default_rng(3)
    noise = (0.02 * rng.standard_normal((len(LENGTHS), 3000))).astype(np.float32)
    host = gpu_engine.reduce_noise(ragged, RATE, lengths=LENGTHS, noise=noise)
    for b, L in enumerate(LENGTHS):
        ref = audio_ref.reduce_noise(ragged[b, :L], noise=noise[b], dft='f32')
        assert float(np.abs(host[b, :L] - ref).max()) <= 1e-5
    a_d, n_d = torch.as_tensor(ragged, device='cuda:0'), torch.as_tensor(noise, device='cuda:0')
    dev = gpu_engine.reduce_noise(a_d, RATE, lengths=LENGTHS, noise=n_d)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    s = torch.cuda.Stream(device=0)
    asy = gpu_engine.reduce_noise(a_d, RATE, lengths=LENGTHS, noise=n_d, stream=s)
    s.synchronize()
    assert np.array_equal(asy.cpu().numpy(), host)
    h0 = gpu_engine.reduce_noise(ragged, RATE, lengths=LENGTHS)
    d0 = gpu_engine.reduce_noise(a_d, RATE, lengths=LENGTHS, stream=s)
    s.synchronize()
    assert np.array_equal(d0.cpu().numpy(), h0)


@pytest.mark.parametrize('mode', ['start_end', 'start', 'end'])
def test_trim_silence_ragged_batch(gpu_engine, ragged, mode):
    start, end = gpu_engine.trim_silence(ragged, RATE, lengths=LENGTHS, mode=mode)
    for b, L in enumerate(LENGTHS):
        assert (int(start[b]), int(end[b])) == audio_ref.trim_window(ragged[b, :L], RATE, mode=mode), (b, L)
    # a row shorter than the 4410-sample window is among them
    assert min(LENGTHS) < int(0.2 * RATE)


def test_trim_silence_pinned_cases(gpu_engine):
    from test_audio_processing import TRIM_CASES
    for x, kw, expected in TRIM_CASES:
        assert gpu_engine.trim_silence(x, 16000, **kw) == expected, (len(x), kw)


def test_trim_silence_device_input(gpu_engine, ragged):
    import torch
    s0, e0 = gpu_engine.trim_silence(ragged, RATE, lengths=LENGTHS)
    s1, e1 = gpu_engine.trim_silence(torch.as_tensor(ragged, device='cuda:0'), RATE, lengths=LENGTHS)
    assert np.array_equal(s0, s1) and np.array_equal(e0, e1)


def test_synthesize_tokens_cleanup(gpu_engine):
    from text_to_speech_amd.pipeline import TTSPipeline
    rng = np.random.default_rng(11)
    tok = rng.integers(1, 148, (3, 24)).astype(np.int32)
    tok[1, 15:] = 0
    tok[2, 9:] = 0
    p = TTSPipeline(gpu_engine, seed=0)
    kw = dict(deterministic=True, max_length=6.0, early_stopping=False)
    base, n, _ = p.synthesize_tokens(tok, **kw)
    same, n2, _ = p.synthesize_tokens(tok, reduce_noise=False, trim_silence=False, **kw)
    assert np.array_equal(n, n2) and all(np.array_equal(a, b) for a, b in zip(base, same))
    clean, n3, _ = p.synthesize_tokens(tok, reduce_noise=True, trim_silence=True, **kw)
    assert np.array_equal(n, n3)
    for b in range(tok.shape[0]):
        if len(base[b]) == 0:
            assert len(clean[b]) == 0
            continue
        rn = audio_ref.reduce_noise(base[b], rate=RATE, dft='f32').astype(np.float32)
        s, e = audio_ref.trim_window(rn, RATE)
        ref = rn[s:e]
        assert clean[b].shape == ref.shape and float(np.abs(clean[b] - ref).max()) <= 1e-5


def test_argument_errors_launch_nothing(gpu_engine):
    import ctypes
    lib, h = gpu_engine._lib, gpu_engine._h
    a = np.zeros((2, 4096), np.float32)
    out = np.zeros_like(a)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    bad_len = np.array([4097, 10], np.int32)
    assert lib.tts_hip_reduce_noise(h, p(a), 2, 4096, p(bad_len), None, 100, 0, p(out), 0) == -1
    assert b'lengths' in lib.tts_hip_last_error(h)
    assert lib.tts_hip_reduce_noise(h, p(a), 2, 4096, None, None, 0, 0, p(out), 0) == -1
    assert lib.tts_hip_reduce_noise(h, p(a), 2, 4096, None, None, 100, 0, p(out), 7) == -1
    assert lib.tts_hip_reduce_noise(h, p(a), 1 << 14, 1 << 20, None, None, 100, 0, p(out), 1) == -1
    assert b'31-bit' in lib.tts_hip_last_error(h)
    assert lib.tts_hip_reduce_noise_async(h, None, 2, 4096, None, None, 100, 0, p(out), None) == -1
    s, e = np.zeros(2, np.int32), np.zeros(2, np.int32)
    assert lib.tts_hip_trim_silence(h, p(a), 2, 4096, None, 1, 0.1, 0.0, 1.5, 0, p(s), p(e), 0) == -1
    assert lib.tts_hip_trim_silence(h, p(a), 2, 4096, None, 400, 0.1, 0.0, 1.5, 3, p(s), p(e), 0) == -1
    assert lib.tts_hip_trim_silence(h, p(a), 2, 4096, p(bad_len), 400, 0.1, 0.0, 1.5, 0, p(s), p(e), 0) == -1
    assert lib.tts_hip_trim_silence(h, p(a), 2, 4096, None, 400, 0.1, -1.0, 1.5, 0, p(s), p(e), 0) == -1
    assert not out.any()
    # the engine still works after the rejected calls
    assert gpu_engine.trim_silence(np.ones(5000, np.float32), 16000) == (0, 5000)
