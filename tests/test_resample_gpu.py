"""GPU parity: FFT resampling (csrc/resample.hip) against the reference's goldens and the float64 restatement."""
import ctypes
import os

import numpy as np
import pytest

import audio_ref
import resample_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
WAV = os.path.join(GOLDEN, 'audio_test_16k.wav')
FIX = os.path.join(GOLDEN, 'resample_fixture.npz')
# 1, 2, 3, odd, even, a prime, powers of two; 5461 / 5462 put L_fwd on each side of 8192 (one workgroup / four-step)
LENGTHS = [1, 2, 3, 7, 10, 101, 1000, 4096, 5461, 5462, 11200, 32768, 65537]
# (16000, 22050) at n = 2 gives M = N with rates that differ: no Nyquist scaling
PAIRS = [(16000, 22050), (22050, 16000), (44100, 22050), (8000, 48000), (48000, 24000)]


def _rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def test_load_audio_matches_reference_golden(gpu_engine):
    from scipy import signal
    from text_to_speech_amd.audio import load_audio
    f = np.load(FIX)
    y = load_audio(WAV, rate=22050, engine=gpu_engine, resample=True)
    assert y.dtype == np.float32 and y.shape == (89412,)
    rate, raw = audio_ref.read_wav(WAV)
    full = audio_ref.normalize_audio(signal.resample(raw, 89412))
    for name, d in (('every 8th', y[::8] - f['resample_every8']), ('full', y - full)):
        print(f'resample vs reference golden ({name}): max-abs {np.abs(d).max():.3e}, rms {_rms(d):.3e}')
        assert float(np.abs(d).max()) <= 5e-6 and _rms(d) <= 5e-7


def test_load_mel_matches_reference_golden(gpu_engine):
    from text_to_speech_amd.audio import load_mel
    f = np.load(FIX)
    m = load_mel(WAV, engine=gpu_engine, resample=True)
    assert m.shape == (350, 80)
    d = np.abs(m - f['mel'])
    live = f['mel'] > -10.0
    print(f'load_mel(resample=True) vs stft-TacotronSTFT golden: max-abs {d.max():.3e}, '
          f'where the golden is above -10: {d[live].max():.3e} ({live.mean():.1%} of the values)')
    # The reference's 2e-3 holds wherever the log-mel is above -10.  In the near-silent frames (log clamp at -11.51) the
    # log amplifies the fp32 resampling error (~1e-7 absolute): the complex64 restatement gives 4.2e-3 there and scipy on
    # float32 input 3.8e-3, so all 350 rows are held to 5e-3.
    assert float(d[live].max()) <= 2e-3
    assert float(d.max()) <= 5e-3


@pytest.mark.parametrize('n', LENGTHS)
def test_rows_against_float64_restatement(gpu_engine, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    for r, t in PAIRS:
        m = resample_ref.resampled_length(n, r, t)
        if m < 1:
            continue
        y = gpu_engine.resample(x, r, t)
        ref = resample_ref.resample(x.astype(np.float64), m)
        assert y.shape == (m,) and y.dtype == np.float32
        err = float(np.abs(y - ref).max())
        peak = max(float(np.abs(ref).max()), 1e-30)
        print(f'n={n} {r}->{t} (M={m}): max-abs / peak {err / peak:.2e}')
        assert err <= 2e-6 * peak


def test_inverse_across_the_lds_boundary(gpu_engine):
    # M = 4096 gives L_inv = 8192 (one workgroup), M = 4097 gives 16384 (four-step)
    rng = np.random.default_rng(11)
    for n, m in ((2048, 4096), (2048, 4097), (8192, 4096), (8194, 4097)):
        x = rng.standard_normal(n).astype(np.float32)
        y = gpu_engine.resample(x, n, m)
        assert y.shape == (m,)
        ref = resample_ref.resample(x.astype(np.float64), m)
        assert float(np.abs(y - ref).max()) <= 2e-6 * float(np.abs(ref).max())


@pytest.fixture(scope='module')
def ragged():
    rng = np.random.default_rng(7)
    lens = [64880, 1, 5462, 30, 44100, 5461, 999]
    N = max(lens)
    a = rng.standard_normal((len(lens), N)).astype(np.float32) * 0.3
    for b, L in enumerate(lens):
        a[b, L:] = 1e3 * rng.standard_normal(N - L)     # garbage beyond the row's length must not leak in
    return a, lens


def test_ragged_batch_is_bitwise_one_row_calls(gpu_engine, ragged):
    a, lens = ragged
    rate, target = 44100, 48000
    out = gpu_engine.resample(a, rate, target, lengths=lens)
    M = resample_ref.resampled_length(a.shape[1], rate, target)
    assert out.shape == (len(lens), M)
    for b, L in enumerate(lens):
        mb = resample_ref.resampled_length(L, rate, target)
        one = gpu_engine.resample(a[b, :L], rate, target)
        assert one.shape == (mb,)
        assert np.array_equal(out[b, :mb], one), b
        assert not out[b, mb:].any()
    b2 = a.copy()
    b2[:, :] = np.where(np.arange(a.shape[1])[None, :] < np.array(lens)[:, None], a, -7.0)
    assert np.array_equal(gpu_engine.resample(b2, rate, target, lengths=lens), out)


def test_device_tensor_and_stream_paths_match_host(gpu_engine, ragged):
    torch = pytest.importorskip('torch')
    a, lens = ragged
    host = gpu_engine.resample(a, 44100, 48000, lengths=lens)
    dev = torch.as_tensor(a, device=f'cuda:{gpu_engine.device}')
    got = gpu_engine.resample(dev, 44100, 48000, lengths=lens)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), host)
    s = torch.cuda.Stream(device=dev.device)
    got2 = gpu_engine.resample(dev, 44100, 48000, lengths=lens, stream=s)
    s.synchronize()
    assert np.array_equal(got2.cpu().numpy(), host)
    one = gpu_engine.resample(dev[2, :lens[2]], 44100, 48000)
    assert one.shape == (resample_ref.resampled_length(lens[2], 44100, 48000),)
    assert np.array_equal(one.cpu().numpy(), host[2, :one.shape[0]])


def test_refused_abi_calls_write_nothing(gpu_engine):
    from text_to_speech_amd import _lib
    lib, h = _lib.load_library(), gpu_engine._h
    x = np.random.default_rng(1).standard_normal((2, 1000)).astype(np.float32)
    p = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    M = resample_ref.resampled_length(1000, 16000, 22050)
    out = np.full((2, M + 1), 5.0, np.float32)
    bad_lens = np.array([1000, 1001], np.int32)
    short = np.array([1, 1000], np.int32)
    cases = [(p(x), 2, 1000, None, 16000, 22050, M + 1),          # M not the formula's value
             (p(x), 2, 1000, None, 0, 22050, M),                   # rate <= 0
             (p(x), 2, 1000, p(bad_lens), 16000, 22050, M),        # lengths[1] > N
             (p(x), 2, 1000, p(short), 44100, 22050, 500),         # row 0 resamples to 0 samples
             (p(x), 0, 1000, None, 16000, 22050, M)]               # B = 0
    for args in cases:
        rc = lib.tts_hip_resample(h, args[0], args[1], args[2], args[3], args[4], args[5], p(out), args[6], 0)
        assert rc == -1, args
        assert (out == 5.0).all()
    assert b'resample' in lib.tts_hip_last_error(h)
    y = gpu_engine.resample(x, 16000, 22050)                       # the engine still works
    assert np.abs(y - np.stack([resample_ref.resample(r.astype(np.float64), M) for r in x])).max() <= 2e-6 * np.abs(y).max()


def test_load_audio_full_chain_equals_engine_calls(gpu_engine):
    from text_to_speech_amd.audio import load_audio, normalize_audio
    y = load_audio(WAV, 22050, engine=gpu_engine, resample=True, reduce_noise=True, trim_silence=True)
    rate, raw = audio_ref.read_wav(WAV)
    a = gpu_engine.resample(raw.astype(np.float32), rate, 22050)
    a = normalize_audio(a, max_val=1.)
    a = gpu_engine.reduce_noise(a, 22050, renormalize=True)
    s, e = gpu_engine.trim_silence(a, 22050)
    assert np.array_equal(y, a[s:e])
